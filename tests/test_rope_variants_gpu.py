"""Every FUSED rotation site under the RoPE parameters the supported models use (-m gpu): linear scaling, YaRN (ramp + magnitude correction), an attention
factor and frequency factors in both pair layouts (tests/rope_variants.py) -- every other test rotates with plain RoPE, which the stand-alone ROPE kernel
alone sees otherwise (test-backend-ops).  tests/test_rope_variants_host.py shows on the CPU that a site that drops or mis-indexes the factors, takes
freq_scale as 1, skips the ramp or the magnitude correction, or reads a table made for other parameters moves every row past position 16 by NMSE >= 1e-2.

Prefill chains (3a): hand-built q chain, k chain + SET_ROWS into an f16 cache and plain v store, at the smallest shapes that select each kernel of
norm_rope_store (fused.hip): fewer than 32 tokens -- angles in the kernel; from 32 on the per-graph (cos, sin) table, read by k_norm_rope_v4 (D = 128,
NEOX) or k_norm_rope<1> / <2>; the rope-only chain of the llama architecture; two chains with different parameters in one graph.  Every assertion is per
(token, head) row against the reference CPU backend on the same graph: f32 rows NMSE < 1e-7 (the reference's ROPE bar), f16 cache rows < 1e-6
(test_norm_rope_prefill_chains_vs_reference_backend's bar for f16 rows), the v store bit-identical; the float64 restatement is held to the same bars.

One-token sites (3b): a one-layer model (qwen3.Model with the optional rope_* keys) through k_fattn_one, the kernels that take over with option
fattn_one 0, k_fattn_gs and attn_one_sm, with the needle helpers of tests/fattn_needle.py: the keys are built from the REFERENCE's rotated Q, three
consecutive steps run on one graph (eager, capture, replay), and the new token's K cache row -- the sharp observable: the q and k of a launch share one
table -- is read back and held to 1e-6 per KV-head row."""
import types

import numpy as np
import pytest

import fattn_needle as fn
import rope_variants as rv

pytestmark = pytest.mark.gpu

BAR_F32, BAR_F16 = rv.BAR, 1e-6


# ================================================================================================================ 3a: prefill chains
def _build(c, pkg, sets, T, H, HK, n_ctx, norm):
    """sets: [(variant, n_dims or None)] -- one q chain + k chain / store + v store per entry, all over ONE position tensor"""
    F32, F16, I32, I64 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16, pkg.GGML_TYPE_I32, pkg.GGML_TYPE_I64
    ins = dict(pos=c.new_tensor(I32, T), idx=c.new_tensor(I64, T))
    outs = []
    for i, (v, n_dims) in enumerate(sets):
        D = v.D
        t = dict(q=c.new_tensor(F32, D, H, T), k=c.new_tensor(F32, D, HK, T), v=c.new_tensor(F32, D, HK, T),
                 kc=c.new_tensor(F16, HK * D, n_ctx), vc=c.new_tensor(F16, HK * D, n_ctx))
        if norm:
            t.update(qw=c.new_tensor(F32, D), kw=c.new_tensor(F32, D))
        if v.ff:
            t["ff"] = c.new_tensor(F32, D // 2)
        kw = rv.rope_kwargs(v, n_dims)
        qin = c.mul(c.rms_norm(t["q"], 1e-6), t["qw"]) if norm else t["q"]
        Q = c.rope_ext(qin, ins["pos"], t.get("ff"), **kw)
        kin = c.mul(c.rms_norm(t["k"], 1e-6), t["kw"]) if norm else t["k"]
        K = c.rope_ext(kin, ins["pos"], t.get("ff"), **kw)
        ks = c.set_rows(t["kc"], c.view_2d(K, HK * D, T, K.nb[2], 0), ins["idx"])
        vs = c.set_rows(t["vc"], c.view_2d(t["v"], HK * D, T, t["v"].nb[2], 0), ins["idx"])
        ins.update({f"{n}{i}": T_ for n, T_ in t.items()})
        outs += [Q, ks, vs]
    return ins, outs


def _run(pkg, backend, sets, T, H, HK, n_ctx, norm, feeds):
    c = pkg.Context(backend)
    ins, outs = _build(c, pkg, sets, T, H, HK, n_ctx, norm)
    c.alloc()
    for name, t in ins.items():
        backend.tensor_set(t, feeds[name])
    backend.graph_compute(c.graph())
    res = [backend.tensor_get(o).copy() for o in outs]
    c.free()
    return res


def _norm64(x, w, eps=1e-6):
    x = x.astype(np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w.astype(np.float64)


def _chains(pkg, be, ref_be, tag, sets, T, H=8, HK=4, norm=True, fused=True, seed=0):
    """run the graph on the GPU (fusion on, then off for the launch count) and on the reference backend; every row of every output to its bar"""
    n_ctx = 256
    rng = np.random.default_rng(1000 * T + seed)
    pos = rv.positions(T)
    cells = rng.permutation(n_ctx)[:T].astype(np.int64)
    feeds = dict(pos=pos, idx=cells)
    for i, (v, _) in enumerate(sets):
        D = v.D
        feeds.update({f"q{i}": rng.standard_normal((T, H, D)).astype(np.float32), f"k{i}": rng.standard_normal((T, HK, D)).astype(np.float32),
                      f"v{i}": rng.standard_normal((T, HK, D)).astype(np.float32), f"kc{i}": np.zeros((n_ctx, HK * D), np.float16), f"vc{i}": np.zeros((n_ctx, HK * D), np.float16),
                      f"qw{i}": (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), f"kw{i}": (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)})
        if v.ff:
            feeds[f"ff{i}"] = rv.freq_factors(v)
    got = _run(pkg, be, sets, T, H, HK, n_ctx, norm, feeds)
    k_on = int(be.get_stat("kernels_last_graph"))
    be.set_option("fusion", 0)
    try:
        _run(pkg, be, sets, T, H, HK, n_ctx, norm, feeds)
        k_off = int(be.get_stat("kernels_last_graph"))
    finally:
        be.set_option("fusion", 1)
    want = _run(pkg, ref_be, sets, T, H, HK, n_ctx, norm, feeds)
    worst = {}
    for i, (v, n_dims) in enumerate(sets):
        D = v.D
        name = f"{tag} chain {i} ({v.name})"
        Q, kc, vc = (a for a in got[3 * i:3 * i + 3])
        Qr, kcr, vcr = (a for a in want[3 * i:3 * i + 3])
        assert np.isfinite(Q).all() and np.isfinite(kc.astype(np.float32)).all(), name
        qin = _norm64(feeds[f"q{i}"], feeds[f"qw{i}"]) if norm else feeds[f"q{i}"]
        kin = _norm64(feeds[f"k{i}"], feeds[f"kw{i}"]) if norm else feeds[f"k{i}"]
        Q64 = rv.rope_f64(v, qin, pos, feeds.get(f"ff{i}"), n_dims)
        K64 = rv.rope_f64(v, kin, pos, feeds.get(f"ff{i}"), n_dims)
        Q, Qr = Q.reshape(T, H, D), Qr.reshape(T, H, D)
        krows, krows_r = (a.reshape(n_ctx, HK, D)[cells].astype(np.float64) for a in (kc, kcr))
        e = [rv.worst_row(Q, Qr), rv.worst_row(Q, Q64), rv.worst_row(krows, krows_r), rv.worst_row(krows, K64)]
        print(f"{name}: worst (token, head) row NMSE -- f32 rope rows vs the reference backend {e[0][0]:.3e} at {e[0][1]} (position {pos[e[0][1][0]]}), vs float64 {e[1][0]:.3e}; "
              f"f16 cache rows vs the reference backend {e[2][0]:.3e} at {e[2][1]} (position {pos[e[2][1][0]]}), vs float64 {e[3][0]:.3e}; launches {k_on} (fusion off: {k_off})")
        assert e[0][0] < BAR_F32 and e[1][0] < BAR_F32, (name, e[0], e[1])
        assert e[2][0] < BAR_F16 and e[3][0] < BAR_F16, (name, e[2], e[3])
        rest = np.setdiff1d(np.arange(n_ctx), cells)
        assert not kc.reshape(n_ctx, -1)[rest].any() and not vc.reshape(n_ctx, -1)[rest].any(), (name, "a cache row no token names was written")
        assert np.array_equal(vc.view(np.uint16), vcr.view(np.uint16)), (name, "v store")               # v: a pure f32 -> f16 store
        if n_dims is not None:                                            # partial rotary: the channels past n_dims are the ROPE's input, bit for bit
            if not norm:
                assert np.array_equal(Q[..., n_dims:].view(np.uint32), feeds[f"q{i}"][..., n_dims:].view(np.uint32)), name
                assert np.array_equal(kc.reshape(n_ctx, HK, D)[cells][..., n_dims:].view(np.uint16), feeds[f"k{i}"][..., n_dims:].astype(np.float16).view(np.uint16)), name
        worst[name] = max(e[0][0], e[1][0])
    if fused:
        assert k_on < k_off, (tag, k_on, k_off)                           # the chains ran inside the norm + rope launch
    else:                                                                 # the matchers refused: every ROPE and SET_ROWS a launch of its own -- with a norm in front the two
        assert k_on >= k_off - (2 if norm else 0), (tag, k_on, k_off)     # RMS_NORM -> MUL pairs still fold (exec_rms_norm), which is all that may be saved
    return k_on, k_off


D128 = ["plain", "linear", "yarn4", "attn_factor", "ff_neox"]


@pytest.mark.parametrize("name", D128 + ["yarn32_d64", "ff_norm_d64"])
def test_chain_angles_in_kernel(pkg, be, ref_be, name):
    """19 tokens (< 32: no table): k_norm_rope<1> computes rope_angle per (head, token, pair) itself"""
    _chains(pkg, be, ref_be, "T 19, in-kernel angles", [(rv.ALL[name], None)], 19)


@pytest.mark.parametrize("name", D128)
def test_chain_table_16_lanes_per_row(pkg, be, ref_be, name):
    """64 tokens, D = 128, NEOX, 8 / 4 heads: k_rope_table + k_norm_rope_v4"""
    _chains(pkg, be, ref_be, "T 64, table + k_norm_rope_v4", [(rv.ALL[name], None)], 64)


@pytest.mark.parametrize("name", ["ff_norm_d64", "yarn32_d64", "ff_norm_d128"])
def test_chain_table_wave_per_row(pkg, be, ref_be, name):
    """64 tokens at D = 64, and at D = 128 in NORMAL mode (which k_norm_rope_v4 refuses): k_rope_table + k_norm_rope<1>"""
    _chains(pkg, be, ref_be, "T 64, table + k_norm_rope<1>", [(rv.ALL[name], None)], 64)


@pytest.mark.parametrize("T", [19, 64])
def test_chain_two_pairs_per_lane(pkg, be, ref_be, T):
    """D = 256: k_norm_rope<2>, lane l owns pairs l and l + 64 -- the YaRN ramp 51 .. 100 crosses from the first to the second"""
    _chains(pkg, be, ref_be, f"T {T}, k_norm_rope<2>", [(rv.ALL["yarn_d256"], None)], T)


@pytest.mark.parametrize("T", [19, 64])
def test_rope_only_chain(pkg, be, ref_be, T):
    """exec_rope_chain (the llama architecture: no norm): q ROPE, k ROPE -> SET_ROWS, v store in one launch, Llama-3's frequency factors, NORMAL pairs"""
    _chains(pkg, be, ref_be, f"T {T}, rope-only chain", [(rv.ALL["ff_norm_d64"], None)], T, norm=False)


@pytest.mark.parametrize("first,second", [("plain", "yarn4"), ("yarn4", "plain"), ("plain", "plain_base1e4"), ("plain_base1e4", "plain")])
def test_two_chains_with_different_parameters_in_one_graph(pkg, be, ref_be, first, second):
    """two layers' chains over ONE position tensor at 64 tokens: the table record (exec_state::rt) must not hand the second the first one's table --
    each order, so that whichever goes second is tested; the second pair differs in freq_base alone (a Gemma-style graph)"""
    _chains(pkg, be, ref_be, f"T 64, {first} then {second}", [(rv.ALL[first], None), (rv.ALL[second], None)], 64)


@pytest.mark.parametrize("T", [19, 64])
@pytest.mark.parametrize("norm", [True, False], ids=["norm_chain", "rope_only"])
def test_partial_rotary_is_not_fused_and_passes_the_tail_through(pkg, be, ref_be, T, norm):
    """n_dims = 64 of D = 128: match_norm_rope and match_rope_only refuse it -- the graph runs node by node (no fewer launches than with fusion off; in front of a norm
    chain's ROPE the RMS_NORM -> MUL fold remains, one launch per chain), is still right, and channels 64 .. 127 are the ROPE's input bit for bit (compared on the
    rope-only form, where that input is a leaf)"""
    _chains(pkg, be, ref_be, f"T {T}, n_dims 64 of 128", [(rv.ALL["yarn4"], 64)], T, norm=norm, fused=False)


# ================================================================================================================ 3b: one-token sites
def _q4_k_m(cfg):
    from llama_cpp_omni_amd import qwen3
    return qwen3.q4_k_m_types(cfg)


def _q8_0(cfg):
    from llama_cpp_omni_amd import qwen3
    return qwen3.uniform_types(cfg, 8)                                    # GGML_TYPE_Q8_0: the omni TTS decoder's weights


def _site_model(name):
    """(cfg, tensor types, tag): yarn4 / ff_neox on the needle file's one-layer config (4096 wide, 32 / 8 heads of 128), ff_norm_d64 on a one-layer llama-architecture
    config at the TTS decoder's width (768, 12 heads of 64, no q / k norm, NORMAL pairs)"""
    import test_round6_gpu as r6
    v = rv.ALL[name]
    if v.D == 128:
        base, ty = dict(r6.CFG, n_layer=1, n_ff=256, n_vocab=256), _q4_k_m
        assert v.mode == rv.NEOX
    else:
        base, ty = dict(arch="llama", n_embd=768, n_layer=1, n_head=12, n_head_kv=12, head_dim=64, n_ff=256, n_vocab=256, rms_eps=1e-5), _q8_0
        assert v.mode == rv.NORMAL
    cfg = dict(base, rope_base=v.freq_base, n_ctx_orig=v.n_ctx_orig, rope_freq_scale=v.freq_scale, rope_ext_factor=v.ext_factor, rope_attn_factor=v.attn_factor,
               rope_beta_fast=v.beta_fast, rope_beta_slow=v.beta_slow)
    if v.ff:
        cfg["rope_freqs"] = rv.freq_factors(v)
    return types.SimpleNamespace(cfg=cfg, types=ty, tag=name, E=cfg["n_embd"], H=cfg["n_head"], HK=cfg["n_head_kv"], D=cfg["head_dim"])


@pytest.fixture(scope="module", autouse=True)
def _free_models():
    yield
    fn.free_models()


def _k_rows(tag, be, ref_be, M, flash, cell):
    got, want = (fn.k_cache_row(b, M.cfg, M.types, flash, cell, M.tag).astype(np.float64) for b in (be, ref_be))
    e, at = rv.worst_row(got, want)
    print(f"{tag}: the new token's K cache row (cell {cell}), worst KV-head row NMSE vs the reference backend {e:.3e} at {at}")
    assert np.isfinite(got).all() and e < BAR_F16, (tag, e, at)
    return e


def _three_steps(tag, be, ref_be, M, flash, n_kv, pos0, options, width):
    """three consecutive steps at pos0, pos0 + 1, pos0 + 2 on ONE graph object (eager -- the options were just set --, capture, replay), each with its own embedding,
    needles moved over the slice edges, rows and the new K row checked.  Returns kernels_last_graph of the eager step"""
    rng = np.random.default_rng(n_kv + pos0)
    n_eager = None
    for name, val in options:
        be.set_option(name, val)
    be.set_option("fattn_gqa", 1)                                         # (setting an option drops the captured graphs: the first step runs eagerly)
    r0, gs0 = be.get_stat("graph_replays"), be.get_stat("fattn_gs_launches")
    try:
        for s in range(3):
            pos = pos0 + s
            x = rng.standard_normal((1, M.E)).astype(np.float32)
            edges = fn.slice_edges(width, pos)
            cells = [edges[(h + s) % len(edges)] for h in range(M.H)]
            Q, _ = fn.step(ref_be, M.cfg, M.types, flash, "rows", n_kv, pos, x, None, M.tag)
            K, V = fn.needle_caches(rng, Q, cells, pos, n_kv, n_head_kv=M.HK)
            _, rows_ref = fn.step(ref_be, M.cfg, M.types, flash, "rows", n_kv, pos, x, (K, V), M.tag)
            _, rows = fn.step(be, M.cfg, M.types, flash, "rows", n_kv, pos, x, (K, V), M.tag)
            if s == 0:
                n_eager = int(be.get_stat("kernels_last_graph"))
            assert np.isfinite(rows).all(), (tag, s)
            fn.head_rows(f"{tag} step {s} (position {pos})", rows.reshape(M.H, M.D), rows_ref.reshape(M.H, M.D), V, cells)
            _k_rows(f"{tag} step {s} (position {pos})", be, ref_be, M, flash, pos)
        assert be.get_stat("graph_replays") > r0, (tag, "the graph did not replay")
        assert be.get_stat("fattn_gs_launches") == gs0, tag                # (k_fattn_gs has a test of its own)
    finally:
        be.set_option("fattn_gs", -1); be.set_option("fattn_one", 1)
    return n_eager


def _plain_launches(be, M, flash, n_kv, pos):
    x = np.random.default_rng(1).standard_normal((1, M.E)).astype(np.float32)
    return fn.launches(be, M.cfg, M.types, flash, n_kv, pos, x, None, "fusion", M.tag)[0]


# kernels_last_graph of the one-layer llama-architecture step (no q / k norm) with the rows tapped: the table launch is the difference between k_fattn_one and the kernels
# that take over with fattn_one 0, as on the needle file's config (ONE_LAUNCHES there); past 256 cells both count the KV-split scratch once
LLAMA_ONE_LAUNCHES = {256: (8, 7), 300: (9, 8)}
LLAMA_SM_LAUNCHES = 8


@pytest.mark.parametrize("n_kv", [256, 300])
@pytest.mark.parametrize("name", ["yarn4", "ff_neox", "ff_norm_d64"])
def test_one_token_kernel_rotates_with_the_variant(pkg, be, ref_be, name, n_kv):
    """k_fattn_one (option fattn_gs 0) reads a T = 1 table from ensure_rope_table: one slice at 256 cells, two at 300.  Then the same steps with option fattn_one 0:
    the streaming kernel (256 cells) and the sliced decode tiles (300) compute the angle themselves (norm_rope_wave<1> in fattn.hip / fattn_mma.hip)"""
    from test_fattn_needle_gpu import ONE_LAUNCHES
    M = _site_model(name)
    pos0 = n_kv - 3
    n = _three_steps(f"k_fattn_one {name} n_kv {n_kv}", be, ref_be, M, True, n_kv, pos0, [("fattn_gs", 0)], 256)
    n_off = _three_steps(f"fattn_one 0 {name} n_kv {n_kv}", be, ref_be, M, True, n_kv, pos0, [("fattn_gs", 0), ("fattn_one", 0)], 256)
    n_plain = _plain_launches(be, M, True, n_kv, pos0)
    print(f"{name} n_kv {n_kv}: kernels_last_graph {n}, with fattn_one 0 {n_off}, with fusion 0 {n_plain}")
    assert n < n_plain and n_off < n_plain, (n, n_off, n_plain)            # the q / k / v pre-stage is inside the attention launch
    assert (n, n_off) == (ONE_LAUNCHES if M.D == 128 else LLAMA_ONE_LAUNCHES)[n_kv], (n, n_off)      # the one-token kernel ran (+ its table launch), and the option takes it away


@pytest.mark.parametrize("name", ["yarn4", "ff_neox"])
def test_group_slice_kernel_rotates_with_the_variant_through_wo(pkg, be, ref_be, name):
    """k_fattn_gs (D = 128, 4 heads per KV head) leaves partial states that the wo launch folds: the wo output is tapped, bar = the needle file's signal / 10 rule (signal:
    the least distance the reference's wo output moves when one head's needle cell is zeroed); n_kv 224, positions 65, 66, 67 on one graph"""
    from conftest import nmse
    M = _site_model(name)
    n_kv, pos0, flash = 224, 65, True
    rng = np.random.default_rng(n_kv + pos0)
    step = lambda b, pos, x, caches=None: fn.step(b, M.cfg, M.types, flash, "wo", n_kv, pos, x, caches, M.tag)
    be.set_option("fattn_gs", 1)
    r0, gs0 = be.get_stat("graph_replays"), be.get_stat("fattn_gs_launches")
    try:
        for s in range(3):
            pos = pos0 + s
            x = rng.standard_normal((1, M.E)).astype(np.float32)
            edges = fn.slice_edges(64, pos)
            cells = [edges[(h + s) % len(edges)] for h in range(M.H)]
            Q, _ = step(ref_be, pos, x)
            K, V = fn.needle_caches(rng, Q, cells, pos, n_kv, n_head_kv=M.HK)
            _, wo_ref = step(ref_be, pos, x, (K, V))
            signal = np.inf
            for h in range(M.H):
                K0 = K.copy(); K0[cells[h], h // (M.H // M.HK)] = 0
                signal = min(signal, nmse(step(ref_be, pos, x, (K0, V))[1], wo_ref))
            step(ref_be, pos, x, (K, V))                                  # (again: the reference's cache holds this step's K row for the read-back below)
            _, wo = step(be, pos, x, (K, V))
            dist = nmse(wo, wo_ref)
            print(f"k_fattn_gs {name} step {s} (position {pos}): signal {signal:.3e}, GPU to reference {dist:.3e}")
            assert np.isfinite(wo).all() and dist < signal / 10, (name, s, dist, signal)
            _k_rows(f"k_fattn_gs {name} step {s} (position {pos})", be, ref_be, M, flash, pos)
        launched = be.get_stat("fattn_gs_launches") - gs0
        assert launched >= 1, "the steps did not take the group-slice kernel"
        assert be.get_stat("graph_replays") > r0, "the graph did not replay"
    finally:
        be.set_option("fattn_gs", -1)


@pytest.mark.parametrize("name", ["yarn4", "ff_neox", "ff_norm_d64"])
def test_one_token_soft_max_chain_rotates_with_the_variant(pkg, be, ref_be, name):
    """attn_one_sm: flash-attention off (transposed V cache), 512 cells, positions 257, 258, 259 -- a T = 1 table from ensure_rope_table again"""
    from test_fattn_needle_gpu import SM_LAUNCHES
    M = _site_model(name)
    n = _three_steps(f"attn_one_sm {name}", be, ref_be, M, False, 512, 257, [], 256)
    n_plain = _plain_launches(be, M, False, 512, 257)
    print(f"attn_one_sm {name}: kernels_last_graph {n}, with fusion 0 {n_plain}")
    assert n < n_plain, (n, n_plain)                                       # K.q, soft-max, V^T.p, permute + cont and the pre-stage in one launch
    assert n == (SM_LAUNCHES if M.D == 128 else LLAMA_SM_LAUNCHES), n
