"""A Qwen2-VL decoder layer and a block of its vision tower on the GPU (-m gpu), mirrors in llama.cpp-omni_amd/qwen2vl.py.

Fused decode: one llm_build_qwen2vl layer (RMS norm, biased q / k / v, two ggml_rope_multi in mode 8, KV store, attention, FFN) at one token and at five, with
unequal t / h / w positions (tests/mrope_cases.py; the five hold the text token), flash-attention on and off, against the reference CPU backend.  Three
submissions of ONE graph object -- eager, captured, replayed -- each with new embeddings, positions and cache cells.  Two observables carry the rotation:
  * the new tokens' K cache rows, read back after every submission: per (token, KV head) row against the reference backend's at 1e-6, test_rope_variants_gpu's
    bar for f16 cache rows -- k's rotation;
  * the layer's attention rows (a tap), over a cache PRE-FILLED with random keys and values in every cell below the new tokens': the scores are q . k over
    hundreds of fixed keys, so they follow q's rotation (with an empty cache a one-token step attends to its own key alone, where a mistake made on q and k
    alike cancels).  Bar: 5e-4, the reference's NMSE bar for FLASH_ATTN_EXT / MUL_MAT, the ops that produce the rows.
MISTAKES are three wrong rotations a fused site could make, produced on the REFERENCE backend by feeding it other positions: the sections ignored (every row =
t), the h and w rows swapped, and the first submission's positions kept (a table made once, or positions read on the host at capture).  The test prints the
least distance each moves either observable and asserts it stays >= 10 x the bar that observable is held to.  Logits are held to NMSE < 2e-3 as well, the bar
of test_tts_shape_decode_on_a_deep_cache_vs_reference_backend, but see none of this (the residual stream swamps one layer's attention).
The executor's launches -- fusion on and off, and the launches of the rotation classes -- equal those of the same layer built with ggml_rope_ext in NEOX mode
(at five tokens this mirror's node order keeps both layers on the plain kernel; the hand-built chain below takes the norm + rope launch with in-kernel
angles).  With the two ROPE nodes observed as graph outputs their rows meet the ROPE bar (1e-7) against the float64 restatement.

ViT block: 16 patches, 2 heads of 80 channels, q / k rotated in mode 24 with clip.cpp's sections, soft-max attention, against the reference backend within
the reference's bar for the block's last arithmetic op, MUL_MAT(v, soft-max) (test-backend-ops: NMSE 5e-4); the rotated rows themselves are read too."""
import types

import numpy as np
import pytest

import mrope_cases as mc
from conftest import nmse

pytestmark = pytest.mark.gpu

N_KV = 256
BAR_K16, BAR_ATTN = 1e-6, 5e-4
MISTAKES = {
    "sections_ignored": lambda s, pos4, first: np.stack([pos4[0]] * 4),
    "h_w_swapped":      lambda s, pos4, first: pos4[[0, 2, 1, 3]],
    "stale_positions":  lambda s, pos4, first: first,                      # (submission 0 is right under this one)
}


def _models(pkg, backend, flash, mrope):
    from llama_cpp_omni_amd import qwen2vl, qwen3
    cfg = qwen2vl.TINY
    return qwen2vl.Model(backend, cfg, qwen3.uniform_types(cfg, pkg.GGML_TYPE_Q8_0), n_ctx=N_KV, seed=11, flash_attn=flash, mrope=mrope)


def _steps(T):
    """three submissions: (embeddings, positions [4, T], first cache cell); the positions change every time, and so do the cells (100, 140, 180: every
    submission attends to at least 100 pre-filled cells)"""
    rng = np.random.default_rng(40 + T)
    pos = mc.positions(max(T, 5))[:, :T] if T > 1 else mc.positions(1)
    out = []
    for s in range(3):
        p = pos + np.array([[7], [300], [41], [0]], np.int32) * s          # each row moves by its own amount
        if T >= 4:
            p[:, 3] = p[0, 3]                                              # the text token stays a text token
        out.append((rng.standard_normal((T, 512)).astype(np.float32), np.ascontiguousarray(p), 100 + 40 * s))
    return out


def _prefill(mdl, backend):
    """random keys and values in every cache cell (the new tokens overwrite theirs): the same bytes on every backend"""
    rng = np.random.default_rng(77)
    L = mdl.layers[0]
    n = L["k_cache"].ne[0] * L["k_cache"].ne[1]
    backend.tensor_set(L["k_cache"], rng.standard_normal(n).astype(np.float16))
    backend.tensor_set(L["v_cache"], rng.standard_normal(n).astype(np.float16))


def _run(pkg, backend, flash, mrope, T, observe=False, stats=False, mistake=None):
    from llama_cpp_omni_amd import qwen2vl
    HK, D = qwen2vl.TINY["n_head_kv"], qwen2vl.TINY["head_dim"]
    mdl = _models(pkg, backend, flash, mrope)
    _prefill(mdl, backend)
    g, I, logits = mdl.build(T, N_KV, observe_rope=observe, tap_attn=not observe)
    gr = g.graph()
    res = types.SimpleNamespace(logits=[], attn=[], krows=[], q=[], k=[], pre_q=[], pre_k=[], launches=None, launches_unfused=None, classes=None, replays=0)
    r0 = backend.get_stat("graph_replays") if stats else 0
    steps = _steps(T)
    for s, (x, pos4, cell0) in enumerate(steps):
        mdl.set_inputs_mrope(I, x, pos4 if mistake is None else np.ascontiguousarray(MISTAKES[mistake](s, pos4, steps[0][1])), cell0, N_KV)
        backend.graph_compute(gr)
        res.logits.append(backend.tensor_get(logits).copy())
        kc = backend.tensor_get(mdl.layers[0]["k_cache"]).reshape(N_KV, HK, D)
        res.krows.append(kc[cell0:cell0 + T].astype(np.float64))
        if observe:
            res.q.append(backend.tensor_get(g.rope_q).copy()); res.k.append(backend.tensor_get(g.rope_k).copy())
            res.pre_q.append(backend.tensor_get(g.pre_q).copy()); res.pre_k.append(backend.tensor_get(g.pre_k).copy())
        else:
            res.attn.append(backend.tensor_get(g.attn_tap).copy())
        if stats and s == 0:
            res.launches = int(backend.get_stat("kernels_last_graph"))
    if stats:
        res.replays = backend.get_stat("graph_replays") - r0           # (before reset_stats below zeroes the counter)
        x, pos4, cell0 = steps[0]
        backend.set_option("profile", 1); backend.set_option("reset_stats", 1)
        try:
            mdl.set_inputs_mrope(I, x, pos4, cell0, N_KV)
            backend.graph_compute(gr); backend.synchronize()
            res.classes = {c: int(backend.get_stat(f"prof_{c}_n")) for c in ("rope", "norm_rope", "fattn")}
        finally:
            backend.set_option("profile", 0)
        backend.set_option("fusion", 0)
        try:
            backend.graph_compute(gr); backend.synchronize()
            res.launches_unfused = int(backend.get_stat("kernels_last_graph"))
        finally:
            backend.set_option("fusion", 1)
    g.free(); mdl.bctx.free(); mdl.wctx.free()
    return res


def _floors(pkg, ref_be, want, flash, T):
    """the least distance each mistake moves the K cache rows (per row, tokens with unequal positions) and the attention rows (per submission) on the reference"""
    rows = mc.unequal(_steps(T)[0][1])
    fk, fa = {}, {}
    for m in MISTAKES:
        bad = _run(pkg, ref_be, flash, True, T, mistake=m)
        subs = range(1, 3) if m == "stale_positions" else range(3)
        fk[m] = min(float(mc.row_nmse(bad.krows[s], want.krows[s])[rows].min()) for s in subs)
        fa[m] = min(nmse(bad.attn[s], want.attn[s]) for s in subs)
        print(f"T {T} flash {flash} mistake {m} on the reference backend: least K cache row distance {fk[m]:.3e}, least attention rows distance {fa[m]:.3e}")
    return fk, fa


@pytest.mark.parametrize("flash", [True, False], ids=["flash", "soft_max"])
@pytest.mark.parametrize("T", [1, 5])
def test_qwen2vl_layer_eager_captured_replayed(pkg, be, ref_be, T, flash):
    got = _run(pkg, be, flash, True, T, stats=True)
    want = _run(pkg, ref_be, flash, True, T)
    neox = _run(pkg, be, flash, False, T, stats=True)
    fk, fa = _floors(pkg, ref_be, want, flash, T)
    assert min(fk.values()) >= 10 * BAR_K16 and min(fa.values()) >= 10 * BAR_ATTN, (fk, fa)       # the observables see every mistake
    for s in range(3):
        ek, at = mc.worst_row(got.krows[s], want.krows[s])
        ea = nmse(got.attn[s], want.attn[s])
        e = nmse(got.logits[s], want.logits[s])
        print(f"T {T} flash {flash} submission {s}: K cache rows worst (token, head) NMSE vs the reference backend {ek:.3e} at {at}, attention rows {ea:.3e}, logits {e:.3e}")
        assert np.isfinite(got.krows[s]).all() and ek <= BAR_K16, (T, flash, s, ek, at)
        assert np.isfinite(got.attn[s]).all() and ea <= BAR_ATTN, (T, flash, s, ea)
        assert np.isfinite(got.logits[s]).all() and e < 2e-3, (T, flash, s, e)
        assert np.array_equal(got.logits[s].reshape(T, -1).argmax(-1), want.logits[s].reshape(T, -1).argmax(-1)), (T, flash, s)
    assert got.replays >= 1, "the third submission did not replay the captured graph"
    print(f"T {T} flash {flash}: launches {got.launches} (fusion off {got.launches_unfused}), classes {got.classes}; the NEOX layer {neox.launches} ({neox.launches_unfused}), {neox.classes}")
    assert (got.launches, got.launches_unfused, got.classes) == (neox.launches, neox.launches_unfused, neox.classes)
    assert got.launches < got.launches_unfused


@pytest.mark.parametrize("flash", [True, False], ids=["flash", "soft_max"])
@pytest.mark.parametrize("T", [1, 5])
def test_observed_rope_rows_meet_the_rope_bar(pkg, be, T, flash):
    """the two ROPE nodes and the biased projections in front of them flagged as graph outputs: q and k rows of every submission (eager, captured, replayed,
    new positions each) against mrope_f64 of the projections the same submission produced"""
    from llama_cpp_omni_amd import qwen2vl
    v = types.SimpleNamespace(**{**vars(mc.SETS["q2vl"]), "freq_base": qwen2vl.TINY["rope_base"], "n_ctx_orig": qwen2vl.TINY["n_ctx_orig"]})
    assert v.sections == tuple(qwen2vl.TINY["rope_sections"])
    got = _run(pkg, be, flash, True, T, observe=True)
    H, HK, D = qwen2vl.TINY["n_head"], qwen2vl.TINY["n_head_kv"], qwen2vl.TINY["head_dim"]
    for s, (x, pos4, cell0) in enumerate(_steps(T)):
        for name, rows, pre, nh in (("q", got.q[s], got.pre_q[s], H), ("k", got.k[s], got.pre_k[s], HK)):
            e, at = mc.worst_row(rows.reshape(T, nh, D), mc.mrope_f64(v, pre.reshape(T, nh, D), pos4))
            print(f"T {T} flash {flash} submission {s} {name}: worst (token, head) row NMSE vs float64 {e:.3e} at {at}")
            assert np.isfinite(rows).all() and e <= mc.BAR, (T, flash, s, name, e, at)


def _chain_run(pkg, backend, v, T, H, HK, n_ctx, feeds, mrope):
    """q ROPE, k ROPE -> SET_ROWS into an f16 cache, plain v store (the llama-architecture chain of exec_rope_chain) over one position tensor"""
    F32, F16, I32, I64 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16, pkg.GGML_TYPE_I32, pkg.GGML_TYPE_I64
    D = v.D
    c = pkg.Context(backend)
    t = dict(pos=c.new_tensor(I32, (4 if mrope else 1) * T), idx=c.new_tensor(I64, T), q=c.new_tensor(F32, D, H, T), k=c.new_tensor(F32, D, HK, T),
             v=c.new_tensor(F32, D, HK, T), kc=c.new_tensor(F16, HK * D, n_ctx), vc=c.new_tensor(F16, HK * D, n_ctx))
    if v.ff:
        t["ff"] = c.new_tensor(F32, D // 2)
    kw = mc.rope_kwargs(v)
    if mrope:
        rot = lambda x: c.rope_multi(x, t["pos"], t.get("ff"), **kw)
    else:
        kw.pop("sections"); kw["mode"] = 2
        rot = lambda x: c.rope_ext(x, t["pos"], t.get("ff"), **kw)
    Q, K = rot(t["q"]), rot(t["k"])
    ks = c.set_rows(t["kc"], c.view_2d(K, HK * D, T, K.nb[2], 0), t["idx"])
    vs = c.set_rows(t["vc"], c.view_2d(t["v"], HK * D, T, t["v"].nb[2], 0), t["idx"])
    c.alloc()
    for name, T_ in t.items():
        backend.tensor_set(T_, feeds[name] if (name != "pos" or mrope) else np.ascontiguousarray(feeds["pos"][0]))
    backend.graph_compute(c.graph())
    res = [backend.tensor_get(o).copy() for o in (Q, ks, vs)]
    c.free()
    return res


@pytest.mark.parametrize("T", [5, 9])
@pytest.mark.parametrize("name", ["q2vl", "yarn", "extra"])
def test_rope_only_chain_with_in_kernel_angles(pkg, be, ref_be, name, T):
    """exec_rope_chain below 32 tokens: q ROPE, k ROPE -> SET_ROWS and the v store in ONE norm + rope launch whose lanes form the angle themselves
    (rope_angle_tok from the four position rows); head sizes 128 and 64.  f32 rows per (token, head) at the ROPE bar 1e-7 against the reference backend and
    float64, the f16 cache rows at 1e-6 (test_rope_variants_gpu's bar for f16 rows), the v store bit-identical; launches as the NEOX chain's"""
    v = mc.SETS[name]
    H, HK, n_ctx, D = 4, 2, 64, v.D
    rng = np.random.default_rng(100 * T + D)
    pos = mc.positions(T)
    cells = rng.permutation(n_ctx)[:T].astype(np.int64)
    feeds = dict(pos=pos, idx=cells, q=rng.standard_normal((T, H, D)).astype(np.float32), k=rng.standard_normal((T, HK, D)).astype(np.float32),
                 v=rng.standard_normal((T, HK, D)).astype(np.float32), kc=np.zeros((n_ctx, HK * D), np.float16), vc=np.zeros((n_ctx, HK * D), np.float16))
    if v.ff:
        feeds["ff"] = mc.freq_factors(v)
    Q, kc, vc = _chain_run(pkg, be, v, T, H, HK, n_ctx, feeds, True)
    k_on = int(be.get_stat("kernels_last_graph"))
    _chain_run(pkg, be, v, T, H, HK, n_ctx, feeds, False)
    k_neox = int(be.get_stat("kernels_last_graph"))
    be.set_option("fusion", 0)
    try:
        _chain_run(pkg, be, v, T, H, HK, n_ctx, feeds, True)
        k_off = int(be.get_stat("kernels_last_graph"))
    finally:
        be.set_option("fusion", 1)
    Qr, kcr, vcr = _chain_run(pkg, ref_be, v, T, H, HK, n_ctx, feeds, True)
    Q64, K64 = mc.mrope_f64(v, feeds["q"], pos, feeds.get("ff")), mc.mrope_f64(v, feeds["k"], pos, feeds.get("ff"))
    krows, krows_r = (a.reshape(n_ctx, HK, D)[cells].astype(np.float64) for a in (kc, kcr))
    e = [mc.worst_row(Q.reshape(T, H, D), Qr.reshape(T, H, D)), mc.worst_row(Q.reshape(T, H, D), Q64), mc.worst_row(krows, krows_r), mc.worst_row(krows, K64)]
    print(f"{name} T {T}: f32 rows vs the reference backend {e[0][0]:.3e}, vs float64 {e[1][0]:.3e}; f16 cache rows {e[2][0]:.3e}, vs float64 {e[3][0]:.3e}; "
          f"launches {k_on} (NEOX chain {k_neox}, fusion off {k_off})")
    assert np.isfinite(Q).all() and e[0][0] <= mc.BAR and e[1][0] <= mc.BAR, (name, T, e[0], e[1])
    assert e[2][0] <= 1e-6 and e[3][0] <= 1e-6, (name, T, e[2], e[3])
    assert np.array_equal(vc.view(np.uint16), vcr.view(np.uint16))
    assert k_on == k_neox and k_on < k_off, (k_on, k_neox, k_off)


def test_vit_attention_block(pkg, be, ref_be):
    from llama_cpp_omni_amd import qwen2vl
    E, NH, N = 160, 2, 16
    rng = np.random.default_rng(5)
    feeds = {f"{n}_w": (rng.standard_normal((E, E)) / np.sqrt(E)).astype(np.float32) for n in "qkv"}
    feeds.update({f"{n}_b": (0.1 * rng.standard_normal(E)).astype(np.float32) for n in "qkv"})
    x = rng.standard_normal((N, E)).astype(np.float32)
    py, px = np.divmod(np.arange(N, dtype=np.int32), 4)
    pos = np.concatenate([py * 37 + 3, px * 29 + 1, py * 37 + 3, px * 29 + 1]).astype(np.int32)      # clip.cpp's rows: y, x, y, x (spread: a 4 x 4 grid's own indices differ by < 4)
    outs = []
    for backend in (be, ref_be):
        g = pkg.Context(backend)
        X, P = g.new_tensor(pkg.GGML_TYPE_F32, E, N), g.new_tensor(pkg.GGML_TYPE_I32, 4 * N)
        W = {n: g.new_tensor(pkg.GGML_TYPE_F32, *((E, E) if n.endswith("_w") else (E,))) for n in feeds}
        Y = qwen2vl.vit_attention(g, X, P, W, NH)
        g.roots = [g.vit_q, g.vit_k, Y]
        if backend is be:
            assert backend.supports_op(g.vit_q) and backend.supports_op(g.vit_k)
        g.alloc()
        backend.tensor_set(X, x); backend.tensor_set(P, pos)
        for n, T in W.items():
            backend.tensor_set(T, feeds[n])
        backend.graph_compute(g.graph())
        outs.append([backend.tensor_get(t).copy() for t in (g.vit_q, g.vit_k, Y)])
        g.free()
    for name, a, b in zip(("q", "k"), outs[0][:2], outs[1][:2]):
        e, at = mc.worst_row(a.reshape(N, NH, 80), b.reshape(N, NH, 80))
        print(f"ViT block rotated {name}: worst row NMSE vs the reference backend {e:.3e} at {at}")
        assert e <= 5e-4, (name, e, at)                                   # (the rows carry the projection in front, whose bar in test-backend-ops is 5e-4; a rotation mistake moves a row by 1e-2)
    e = nmse(outs[0][2], outs[1][2])
    print(f"ViT block output: NMSE vs the reference backend {e:.3e}")
    assert np.isfinite(outs[0][2]).all() and e < 5e-4, e
