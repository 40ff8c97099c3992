"""FLASH_ATTN_EXT, every kernel form, checked PER OUTPUT ROW on inputs with positioned keys (-m gpu).

The other attention tests draw Gaussian q / k / v and take one NMSE over the whole output: a cell dropped at a tile, slice or causal edge moves
a row by ~1 / n^2 and passes.  Here (tests/fattn_needle.py) a few rows per KV head see one cache cell at score 24 -- their output IS that cell's V
row -- with masked decoys at score 48 right behind each mask edge, a biased cell that must lose, and sinks that make the row exactly a quarter.
tests/test_fattn_needle_host.py shows on the CPU that each such mistake moves its row by per-row NMSE >= 0.1.  Single-node graphs through the
C-ABI, as test_fattn_plan_gpu.py builds them; the same graph is run once per round with the needles moved.

Bar: EVERY output row within NMSE 5e-4 (the project's and the reference's bar for this op, applied per row) of the float64 restatement of
the reference (_attn_f64, test_gpu_parity.py), and of the reference CPU backend where it travelled; the whole output finite.

The kernel form is pinned by the options fattn_gqa / fattn_dma and asserted through kernels_last_graph (launch, + 1 for the mask tile map of the
prefill kernel, + 1 where the executor hands the KV-split scratch over), fattn_dma_launches and fattn_gs_launches; where no counter tells two
forms apart, LAUNCH states the launcher arithmetic (fattn.hip fa_split / fa_decode_nsplit / fa_gqa_plan, fattn_mma.hip launch_fm) that selects it."""
import numpy as np
import pytest

import fattn_needle as fn
from test_gpu_parity import _attn_f64

pytestmark = pytest.mark.gpu

BAR = fn.BAR                                # 5e-4

# name: (option fattn_gqa, option fattn_dma (-1: default), kernels_last_graph with a mask, ring launches)
LAUNCH = {
    # streaming k_fattn_dec (decode tiles off).  fa_split: R = 1 for 1 head per KV head and 1 token; 2 for 2 heads and 1 token; 4 for 2 heads and 2 tokens;
    # 8 for 8 heads.  4 waves for nkv <= 64 ("narrow"), 8 above ("wide", all of these have < 1024 workgroups)
    "dec_r1_narrow":  (0, -1, 1, 0),
    "dec_r2_wide":    (0, -1, 1, 0),      # (20 sequences: the executor's one-token, one-sequence scratch rule of test_fattn_plan_gpu.py's one_257_dec does not apply)
    "dec_r4_wide":    (0, -1, 1, 0),
    "dec_r8":         (0, -1, 1, 0),
    # fa_decode_nsplit: nkv >= 1024 -> nkv / 256 slices (4 and 8; 2 KV heads x 6 / 7 sequences: 48 / 112 workgroups, far below 1024) + k_fattn_merge
    "dec_split4":     (0, -1, 2, 0),
    "dec_split8":     (0, -1, 2, 0),
    # fa_gqa_plan refuses a mask per head and more than 32 heads per KV head: the streaming kernel with the decode tiles ON (33 heads: 5 workgroups of 8 rows per token)
    "dec_per_head":   (1, -1, 1, 0),
    "dec_gq33":       (1, -1, 1, 0),
    # k_fattn_gqa, (nkv + 31) / 32 <= 8 tiles: one workgroup per group finishes the rows
    "gqa_direct_a":   (1, -1, 1, 0),
    "gqa_direct_b":   (1, -1, 1, 0),      # 32 tokens x 4 heads per KV head: 8 tiles exactly, 4 column tiles per KV head
    "gqa_direct_c":   (1, -1, 1, 0),
    # more than 8 tiles: slices of >= 4 tiles + k_fattn_merge (9 tiles: 3 slices; 32 tiles at 1023 and 1024, the last one ragged or full: 8 slices;
    # 47 tiles: 12; 157 tiles: 40; 512 workgroups / (KV heads x sequences) allows more in each)
    "gqa_split_257":  (1, -1, 2, 0),
    "gqa_split_1023": (1, -1, 2, 0),
    "gqa_split_1024": (1, -1, 2, 0),
    "gqa_split_1500": (1, -1, 2, 0),
    "gqa_split_5000": (1, -1, 2, 0),
    # prefill k_fattn_mma (launch_fm).  <= 32 tokens without the decode tiles: <D, 1, 1, 1>
    "mma_1w":         (0, -1, 2, 0),
    "mma_2w_sq1":     (1, -1, 2, 0),      # nkv < 128: <D, 2, 1, 1>
    "mma_2w_sq2":     (1, -1, 2, 0),      # blocks32 = 4 x 8 x 25 = 800 > 768 and nqt4 x nh x ns = 200 < 512: no KV split, <D, 2, 1, 2>
    "mma_ks2":        (1, -1, 2, 0),      # blocks32 = 24 <= 768, 128 <= nkv < 256: two waves split the keys, <D, 2, 2, 1>
    "mma_ks4_d64":    (1, -1, 2, 0),      # blocks32 = 5 x 4 x 2 = 40 <= 512, nkv >= 256: four waves, <D, 2, 4, 1>
    "mma_ks4_d128":   (1, -1, 2, 0),      # blocks32 = 16
    # the LDS-DMA ring (nqt4 = 2): 2 x 32 x 8 = 512 workgroups >= 512 and 2 x 16 x 8 = 256 workgroups of pairs >= 256, 4 heads per KV head: pairs (hw = 2);
    # 2 x 16 x 16 = 512, 1 head per KV head: single.  With fattn_dma 0 the same shapes take the four-wave form <D, 4, 1, 2>
    "ring128_pairs":  (1, 1, 2, 1),
    "ring128_single": (1, 1, 2, 1),
    # head size 64: 2 x 16 x 6 = 192 workgroups >= 192; nkv < 512: plain; nkv = 777 >= 512 and 192 < 257 workgroups: KS2
    "ring64_plain":   (1, 1, 2, 1),
    "ring64_ks2":     (1, 1, 2, 1),
    # the generic kernel: another head size, K and V heads of different size, a quantised / bf16 / f32 cache
    "any_d80":        (1, -1, 1, 0),
    "any_d192_128":   (1, -1, 1, 0),
    "any_q8_0":       (1, -1, 1, 0),
    "any_q4_0":       (1, -1, 1, 0),
    "any_bf16":       (1, -1, 1, 0),
    "any_f32":        (1, -1, 1, 0),
    "any_d576_512":   (1, -1, 1, 0),
}
assert set(LAUNCH) == set(fn.CASES)


class _Graph:
    """one FLASH_ATTN_EXT node, built once, fed and run once per round"""

    def __init__(self, pkg, backend, c):
        self.be = backend
        self.c = ctx = pkg.Context(backend)
        T = fn.KV_TYPES[c.kv_type]
        self.q = ctx.new_tensor(pkg.GGML_TYPE_F32, c.D, c.nq, c.nh, c.ns)
        self.k = ctx.new_tensor(T, c.D, c.nkv, c.nhkv, c.ns)
        self.v = ctx.new_tensor(T, c.Dv, c.nkv, c.nhkv, c.ns)
        self.m = self.sk = None
        if c.mask is not None:
            nm, nq_pad, _ = c.mask.shape
            self.m = ctx.new_tensor(pkg.GGML_TYPE_F16, c.nkv, nq_pad, nm) if nm > 1 else ctx.new_tensor(pkg.GGML_TYPE_F16, c.nkv, nq_pad)
        if c.sinks is not None:
            self.sk = ctx.new_tensor(pkg.GGML_TYPE_F32, c.nh)
        self.y = ctx.flash_attn_ext(self.q, self.k, self.v, self.m, c.scale, c.max_bias, c.softcap, self.sk)
        ctx.alloc()
        self.g = ctx.graph()
        self.shape = (c.ns, c.nq, c.nh, c.Dv)

    def run(self, c):
        be = self.be
        be.tensor_set(self.q, c.q); be.tensor_set(self.k, c.k); be.tensor_set(self.v, c.v)
        if self.m is not None:
            be.tensor_set(self.m, c.mask)
        if self.sk is not None:
            be.tensor_set(self.sk, c.sinks)
        be.graph_compute(self.g)
        return be.tensor_get(self.y).astype(np.float64).reshape(self.shape)

    def free(self):
        self.c.free()


def _ref_backend(request):
    from oracle.ref_backend import ref_available
    return request.getfixturevalue("ref_be") if ref_available() else None


def _judge(tag, c, got, want, ref):
    """print the worst row, then hold every row to the bar"""
    assert np.isfinite(got).all(), tag
    e, at, en = fn.check_rows(got, want, c.needles)
    line = f"{tag}: worst row NMSE vs f64 {e:.3e} at (s, t, h) = {at}, worst needle row {en:.3e}"
    er = None
    if ref is not None:
        er, at_r, _ = fn.check_rows(got, ref, c.needles)
        line += f"; vs reference backend {er:.3e} at {at_r}"
    print(line)
    assert e < BAR, (tag, e, at, [n for n in c.needles if (n[0], n[2], n[1]) == at])
    if er is not None:
        assert er < BAR, (tag, er, at_r)
    return e, er


@pytest.mark.parametrize("cid", fn.case_ids(fn.CASES))
def test_flash_attn_needle_rows(pkg, be, request, cid):
    name, kind = cid.rsplit("-", 1)
    gqa, dma, n_kernels, ring = LAUNCH[name]
    ref_be = _ref_backend(request)
    modes = [dma] if not ring else [1, 0]            # a ring shape runs a second time with the ring off: the four-wave prefill form <D, 4, 1, 2>
    c = fn.build(name, kind, 0)
    graphs = [_Graph(pkg, be, c) for _ in modes]
    gref = _Graph(pkg, ref_be, c) if ref_be is not None else None
    worst = [0.0, 0.0]
    try:
        for rd in range(fn.case_rounds(name, kind)):
            c = fn.build(name, kind, rd) if rd else c
            want = fn.reference(_attn_f64, c)
            ref = gref.run(c) if gref is not None else None
            for g, mode in zip(graphs, modes):
                be.set_option("fattn_gqa", gqa); be.set_option("fattn_dma", mode)
                try:
                    gs0, dma0 = be.get_stat("fattn_gs_launches"), be.get_stat("fattn_dma_launches")
                    got = g.run(c)
                    counts = (be.get_stat("kernels_last_graph"), be.get_stat("fattn_gs_launches") - gs0, be.get_stat("fattn_dma_launches") - dma0)
                finally:
                    be.set_option("fattn_gqa", 1); be.set_option("fattn_dma", -1)
                tag = f"{cid} round {rd}" + (f" fattn_dma {mode}" if ring else "")
                e, er = _judge(tag, c, got, want, ref)
                worst = [max(worst[0], e), max(worst[1], er or 0.0)]
                no_map = c.mask is None and name.startswith(("mma", "ring"))          # the prefill kernel without a mask: no tile map
                assert counts == (n_kernels - no_map, 0, 1 if ring and mode == 1 else 0), (tag, counts)
    finally:
        for g in graphs:
            g.free()
        if gref is not None:
            gref.free()
    print(f"{cid}: worst row over all rounds vs f64 {worst[0]:.3e}" + (f", vs reference backend {worst[1]:.3e}" if gref is not None else ""))


@pytest.mark.parametrize("kind", ["tile_live", "tile_dead"])
@pytest.mark.parametrize("place,qi,ki", fn.TILE_ENTRIES)
def test_mask_tile_map_one_entry(pkg, be, request, place, qi, ki, kind):
    """k_fattn_mask_map classes every 32 x 32 tile of the mask dead / all zero / mixed, and the prefill kernel (<128, 2, 4, 1> at 70 tokens, <128, 2, 2, 1>
    at 40 x 131; 2 heads over 1 KV head, far from the ring) skips dead tiles and does not read the mask of all-zero ones.  tile_live: the ONE live entry
    of a -inf mask holds its row's needle -- a tile classed dead loses the row; tile_dead: the ONE -inf entry of a zero mask hides its row's decoy -- a tile
    classed all zero lets it in.  The second run rewrites the mask (the entry moves to another tile) on the same graph: a map kept from the first run fails it."""
    ref_be = _ref_backend(request)
    cases = [fn.tile_case(place, qi, ki, kind, alt=alt) for alt in (False, True)]
    g = _Graph(pkg, be, cases[0])
    gref = _Graph(pkg, ref_be, cases[0]) if ref_be is not None else None
    try:
        for run, c in enumerate(cases):
            want = fn.reference(_attn_f64, c)
            ref = gref.run(c) if gref is not None else None
            dma0 = be.get_stat("fattn_dma_launches")
            got = g.run(c)
            counts = (be.get_stat("kernels_last_graph"), be.get_stat("fattn_dma_launches") - dma0)
            _judge(f"{place} {kind} entry (row {c.tile[0]}, cell {c.tile[1]}) run {run}", c, got, want, ref)
            assert counts == (2, 0), counts                 # the map is computed again after the mask was written
    finally:
        g.free()
        if gref is not None:
            gref.free()


def _run_chain(pkg, backend, name, c, n_ctx):
    """the five-node chain on the case's inputs -> [1, nq, nh, D]"""
    F32, F16 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16
    D, H, HK, nq, nkv = c.D, c.nh, c.nhkv, c.nq, c.nkv
    g = pkg.Context(backend)
    feeds = []
    if name.startswith("sm_prefill"):                    # the llama -fa 0 graph: q as the rope leaves it, K rows and V^T rows views of caches with room for n_ctx cells
        qc = g.new_tensor(F32, D, H, nq); kc = g.new_tensor(F16, D * HK, n_ctx); vc = g.new_tensor(F16, n_ctx, D * HK)
        q = g.permute(qc, 0, 2, 1, 3)
        k = g.view_3d(kc, D, nkv, HK, D * HK * 2, D * 2, 0)
        v = g.view_3d(vc, nkv, D, HK, n_ctx * 2, n_ctx * 2 * D, 0)
        nq_pad = (nq + 31) // 32 * 32
        m = g.new_tensor(F32, nkv, nq_pad)
        kv = np.zeros((n_ctx, HK, D), np.float16); kv[:nkv] = c.k.reshape(HK, nkv, D).transpose(1, 0, 2)
        vv = np.zeros((HK, D, n_ctx), np.float16); vv[:, :, :nkv] = c.v.reshape(HK, nkv, D).transpose(0, 2, 1)
        feeds = [(qc, c.q[0].transpose(1, 0, 2)), (kc, kv), (vc, vv), (m, c.mask[0, :nq_pad].astype(np.float32))]
    else:                                                # the vision encoder's graph: f32 throughout, V^T as a tensor, no mask
        q = g.new_tensor(F32, D, nq, H); k = g.new_tensor(F32, D, nkv, H); v = g.new_tensor(F32, nkv, D, H)
        m = None
        feeds = [(q, c.q[0]), (k, c.k.reshape(H, nkv, D)), (v, c.v.reshape(H, nkv, D).transpose(0, 2, 1))]
    p = g.soft_max_ext(g.mul_mat(k, q), m, c.scale, 0.0)
    out = g.cont(g.permute(g.mul_mat(v, p), 0, 2, 1, 3), D * H, nq)
    g.alloc()
    for t, val in feeds:
        backend.tensor_set(t, val)
    backend.graph_compute(g.graph())
    got = backend.tensor_get(out).astype(np.float64).reshape(1, nq, H, D)
    g.free()
    return got


@pytest.mark.parametrize("cid", fn.case_ids(fn.CHAINS))
def test_soft_max_attention_chain_needle_rows(pkg, be, request, cid):
    """flash-attention OFF: the node chain runs as one attention launch -- exec_attn_sm_prefill (the prefill kernel reading the transposed V cache as it lies; f32 causal
    mask) and k_attn_f32 (head sizes 72 / 80, f32 operands, no mask) -- on the needle inputs, every row against the float64 attention and the reference CPU backend
    running the same five nodes.  Launch counts as test_round4_gpu.py / test_round6_gpu.py assert them: at most 3 (attention, mask cast, tile map), exactly 1."""
    name, kind = cid.rsplit("-", 1)
    ref_be = _ref_backend(request)
    for rd in range(fn.case_rounds(name, kind)):
        c = fn.build(name, kind, rd)
        c.q = c.q.astype(np.float16).astype(np.float32)      # (the f32 chain keeps q in f32, the float64 restatement rounds it to f16: feed what both read alike)
        n_ctx = (c.nkv + 63) // 64 * 64 + 64
        want = fn.reference(_attn_f64, c)
        got = _run_chain(pkg, be, name, c, n_ctx)
        launches = be.get_stat("kernels_last_graph")
        ref = _run_chain(pkg, ref_be, name, c, n_ctx) if ref_be is not None else None
        _judge(f"{cid} round {rd}", c, got, want, ref)
        assert launches <= 3 if name.startswith("sm_prefill") else launches == 1, launches


# ---- the one-token kernels behind the q / k / v pre-stage (k_fattn_one, k_fattn_gs) and the one-token chain without flash-attention (attn_one_sm) are reached only
# through a layer graph: ONE layer at Qwen3-8B's attention widths (n_embd 4096, 32 / 8 heads of 128: what fattn_gs_ok and the folding wo launch ask for), the smallest
# ffn and vocabulary the K-quant rows take.  The needle directions are the step's own Q after RoPE (g.roots[0]), read from the reference CPU backend on the same weights.
# (the step helpers live in fattn_needle.py: test_rope_variants_gpu.py runs the same steps with other rotations)
def _cfg1():
    import test_round6_gpu as r6
    return dict(r6.CFG, n_layer=1, n_ff=256, n_vocab=256)


def _types(cfg):
    from llama_cpp_omni_amd import qwen3
    return qwen3.q4_k_m_types(cfg)


@pytest.fixture(scope="module", autouse=True)
def _free_models():
    """the one-layer models live for this file only"""
    yield
    fn.free_models()


def _step(pkg, backend, flash, tap, n_kv, pos, x, caches=None):
    return fn.step(backend, _cfg1(), _types, flash, tap, n_kv, pos, x, caches)


def _launches(pkg, be, flash, n_kv, pos, x, caches, option=None):
    return fn.launches(be, _cfg1(), _types, flash, n_kv, pos, x, caches, option)


_needle_caches, _slice_edges, _head_rows = fn.needle_caches, fn.slice_edges, fn.head_rows


# kernels_last_graph of the one-layer step with the rows tapped, as the executor reports it: (the one-token kernel, option fattn_one 0).  k_fattn_one reads the token's
# (cos, sin) table, which a launch of its own prepares; the kernels that take the pre-stage when it is off -- the streaming kernel at 256 cells, the decode tiles with
# their slices past them -- compute the rotation themselves: one launch fewer.  Past 256 cells both sides count the KV-split scratch once.  (With every fusion off
# the step takes 32 / 33 launches, the soft-max chain's 37.)
ONE_LAUNCHES = {256: (8, 7), 300: (9, 8), 1024: (9, 8), 4096: (9, 8)}
SM_LAUNCHES = 8


@pytest.mark.parametrize("n_kv", [256, 300, 1024, 4096])
def test_one_token_kernel_needle_rows(pkg, be, ref_be, n_kv):
    """k_fattn_one (option fattn_gs 0): one slice at 256 cells, 2 / 4 / 16 slices of 256 merged in the kernel through the counters above; each of the 32 heads has its
    needle on a slice edge (255 / 256 / 257 ...), the first cells or the newest ones (pos - 1, pos - 2), moved over the edges from round to round, decoys behind the
    causal edge.  The tapped attention rows per head against the needle's V row and against the reference backend's tap; the launch counts pin the kernel, and the
    kernels that take over with the option off are held to the same rows"""
    pos = n_kv - 3
    rng = np.random.default_rng(n_kv)
    x = rng.standard_normal((1, 4096)).astype(np.float32)
    edges = _slice_edges(256, pos)
    be.set_option("fattn_gs", 0)
    try:
        Q, _ = _step(pkg, ref_be, True, "rows", n_kv, pos, x)
        for rd in range((len(edges) + 31) // 32):
            cells = [edges[(h + 32 * rd) % len(edges)] for h in range(32)]
            K, V = _needle_caches(rng, Q, cells, pos, n_kv)
            gs0 = be.get_stat("fattn_gs_launches")
            _, rows_ref = _step(pkg, ref_be, True, "rows", n_kv, pos, x, (K, V))
            _, rows = _step(pkg, be, True, "rows", n_kv, pos, x, (K, V))
            assert np.isfinite(rows).all() and be.get_stat("fattn_gs_launches") == gs0
            _head_rows(f"k_fattn_one n_kv {n_kv} round {rd}", rows.reshape(32, 128), rows_ref.reshape(32, 128), V, cells)
        n, _ = _launches(pkg, be, True, n_kv, pos, x, (K, V))
        n_off, rows_off = _launches(pkg, be, True, n_kv, pos, x, (K, V), "fattn_one")
        n_plain, _ = _launches(pkg, be, True, n_kv, pos, x, (K, V), "fusion")
        print(f"k_fattn_one n_kv {n_kv}: kernels_last_graph {n}, with fattn_one 0 {n_off}, with fusion 0 {n_plain}")
        _head_rows(f"fattn_one 0, n_kv {n_kv}", rows_off.reshape(32, 128), rows_ref.reshape(32, 128), V, cells)
        assert n < n_plain, (n, n_plain)                                  # the q / k / v pre-stage is inside the attention launch
        assert (n, n_off) == ONE_LAUNCHES[n_kv], (n, n_off)               # the one-token kernel ran, and the option takes it away
    finally:
        be.set_option("fattn_gs", -1)


@pytest.mark.parametrize("n_kv,pos", [(224, 10), (224, 63), (224, 64), (224, 65), (224, 221), (256, 63), (256, 65), (256, 253)])
def test_group_slice_kernel_needle_rows_through_wo(pkg, be, ref_be, n_kv, pos):
    """k_fattn_gs leaves partial states per 64-row slice that the wo launch folds: the rows never exist, so the wo output is tapped.  Needles on the 64-row slice edges,
    the new token's row in slice 0, at 63 / 64 / 65 and in the last slice.  The bar comes from the reference alone: signal = the least distance, over the heads, that the
    reference's wo output moves when that head's needle cell is zeroed; the GPU must be within signal / 10 of the reference."""
    from conftest import nmse
    rng = np.random.default_rng(n_kv + pos)
    x = rng.standard_normal((1, 4096)).astype(np.float32)
    edges = _slice_edges(64, pos)
    Q, _ = _step(pkg, ref_be, True, "wo", n_kv, pos, x)
    cells = [edges[h % len(edges)] for h in range(32)]
    K, V = _needle_caches(rng, Q, cells, pos, n_kv)
    _, wo_ref = _step(pkg, ref_be, True, "wo", n_kv, pos, x, (K, V))
    signal = np.inf
    for h in range(32):
        K0 = K.copy(); K0[cells[h], h // 4] = 0
        _, wo0 = _step(pkg, ref_be, True, "wo", n_kv, pos, x, (K0, V))
        signal = min(signal, nmse(wo0, wo_ref))
    be.set_option("fattn_gs", 1)
    try:
        gs0 = be.get_stat("fattn_gs_launches")
        _, wo = _step(pkg, be, True, "wo", n_kv, pos, x, (K, V))
        launched = be.get_stat("fattn_gs_launches") - gs0
    finally:
        be.set_option("fattn_gs", -1)
    dist = nmse(wo, wo_ref)
    print(f"k_fattn_gs n_kv {n_kv} pos {pos}: signal {signal:.3e}, GPU to reference {dist:.3e}, group-slice launches {launched}")
    assert np.isfinite(wo).all()
    assert launched >= 1, "the step did not take the group-slice kernel"
    assert dist < signal / 10, (dist, signal)


@pytest.mark.parametrize("pos", [255, 256, 257])
def test_one_token_soft_max_chain_needle_rows(pkg, be, ref_be, pos):
    """attn_one_sm: one token with flash-attention off (transposed V cache), the new token's cell on either side of a 256-cell edge; tapped rows as above"""
    n_kv = 512
    rng = np.random.default_rng(pos)
    x = rng.standard_normal((1, 4096)).astype(np.float32)
    edges = _slice_edges(256, pos)
    Q, _ = _step(pkg, ref_be, False, "rows", n_kv, pos, x)
    cells = [edges[h % len(edges)] for h in range(32)]
    K, V = _needle_caches(rng, Q, cells, pos, n_kv)
    _, rows_ref = _step(pkg, ref_be, False, "rows", n_kv, pos, x, (K, V))
    _, rows = _step(pkg, be, False, "rows", n_kv, pos, x, (K, V))
    assert np.isfinite(rows).all()
    _head_rows(f"attn_one_sm pos {pos}", rows.reshape(32, 128), rows_ref.reshape(32, 128), V, cells)
    n, _ = _launches(pkg, be, False, n_kv, pos, x, (K, V))
    n_plain, _ = _launches(pkg, be, False, n_kv, pos, x, (K, V), "fusion")
    print(f"attn_one_sm pos {pos}: kernels_last_graph {n}, with fusion 0 {n_plain}")
    assert n < n_plain, (n, n_plain)                                      # K.q, soft-max, V^T.p, permute + cont and the pre-stage in one launch
    assert n == SM_LAUNCHES, n
