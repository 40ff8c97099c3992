"""FLASH_ATTN_EXT over a Q8_0 / Q4_0 KV cache at head size 64 / 128: k_fattn_q (fattn_q.hip) against the float64 restatement, the generic kernel and the
reference CPU backend (-m gpu).

Needle inputs of tests/fattn_needle.py (a dropped, doubled or leaked cache cell moves its row by NMSE ~1), one FLASH_ATTN_EXT node as test_fattn_needle_gpu.py
builds it, run twice on the same inputs: option "fattn_q" at its default (the new kernel) and at 0 (k_fattn_any).  Per case:
  1. "fattn_q_launches" rises by exactly 1 on the default run and by 0 with the option off;
  2. "kernels_last_graph" is 1 where one workgroup walks the whole range (<= 16 tiles of 32 cells) and 2 where the range is sliced (+ k_fattn_merge);
  3. every row within fn.BAR = 5e-4 of the float64 attention on the de-quantised cache and the Q8_0-quantised query;
  4. the whole output finite and within NMSE 1e-9 of the generic kernel's, and of the reference backend's where it is available -- the project's bar for this
     arithmetic (test_prefill_kernels_gpu.py): integer block sums, f32 soft-max, V accumulated in f32.
Two shapes are the nearest make_case can express: its causal mask ends 3 cells before the end of the view, so "ragged second tile" uses 37 cells (cells 32 and 33
live in a 5-cell tile) where 33 would leave the second tile dead; the window mask is make_case's causal one with every cell before the last 40 masked as well."""
import numpy as np
import pytest

import fattn_needle as fn
from conftest import nmse
from test_gpu_parity import _attn_f64

pytestmark = pytest.mark.gpu

# name: (D, cache type, nq, nh, nhkv, nkv, ns, mask kind, softcap, kernels_last_graph)
CASES = {
    "ragged_second_tile_decode": (128, "q8_0", 1, 4, 1, 37, 1, "causal", 0.0, 1),
    "column_tiles_ragged":       (64, "q4_0", 35, 4, 4, 130, 1, "causal", 0.0, 1),      # 5 column tiles per KV head: two workgroups, the second with three idle waves
    "gq_not_dividing_32":        (128, "q4_0", 5, 6, 2, 70, 1, "causal", 0.0, 1),       # gq 3: 10 tokens per tile, columns 30 / 31 idle
    "gq_33":                     (64, "q8_0", 2, 33, 1, 96, 1, "causal", 0.0, 1),       # two column tiles per token, the second with one head
    "no_mask_two_sequences":     (128, "q8_0", 3, 4, 2, 64, 2, "none", 0.0, 1),
    "softcap_sinks":             (128, "q8_0", 2, 8, 2, 100, 1, "sinks", 30.0, 1),
    "window_dead_tiles":         (64, "q8_0", 4, 4, 2, 300, 1, "window", 0.0, 1),       # tiles 0 .. 7 dead, the ragged tile 9 live
    "direct_limit_plus_one":     (128, "q8_0", 1, 8, 2, 513, 1, "causal", 0.0, 2),      # 17 tiles: 4 slices
    "slices_prefill_columns":    (64, "q4_0", 9, 8, 2, 1100, 1, "causal", 0.0, 2),      # 35 tiles: 7 slices of 5, a 12-cell last tile
    "view_llama_layout":         (128, "q8_0", 3, 8, 2, 70, 1, "view", 0.0, 1),         # K / V views of [n_ctx][(2 heads x 4 + 1) blocks]: cell stride 306, offset 34 bytes
}


def _case(name):
    D, kv_type, nq, nh, nhkv, nkv, ns, kind, softcap, _ = CASES[name]
    c = fn.make_case(D, D, nq, nh, nhkv, nkv, ns, "causal" if kind in ("window", "view") else kind, 0, sum(map(ord, name)), kv_type, softcap)
    if kind == "window":
        c.mask[:, :, :nkv - 40] = fn.NINF                       # (round 0's needles sit on the causal edge, inside the window)
    return c


class _Graph:
    """one FLASH_ATTN_EXT node (test_fattn_needle_gpu.py's), K / V optionally views into caches with room for n_ctx cells of all KV heads plus one block"""

    def __init__(self, pkg, backend, c, view):
        self.be, self.view = backend, view
        self.c = ctx = pkg.Context(backend)
        T = fn.KV_TYPES[c.kv_type]
        self.q = ctx.new_tensor(pkg.GGML_TYPE_F32, c.D, c.nq, c.nh, c.ns)
        if view:
            self.n_ctx, bb = c.nkv + 7, c.k.shape[-1]
            self.kc = ctx.new_tensor(T, c.nhkv * c.D + 32, self.n_ctx); self.vc = ctx.new_tensor(T, c.nhkv * c.D + 32, self.n_ctx)
            nb1, nb2 = (c.nhkv * c.D // 32 + 1) * bb, c.D // 32 * bb
            self.k = ctx.view_3d(self.kc, c.D, c.nkv, c.nhkv, nb1, nb2, bb); self.v = ctx.view_3d(self.vc, c.D, c.nkv, c.nhkv, nb1, nb2, bb)
        else:
            self.k = ctx.new_tensor(T, c.D, c.nkv, c.nhkv, c.ns); self.v = ctx.new_tensor(T, c.D, c.nkv, c.nhkv, c.ns)
        self.m = ctx.new_tensor(pkg.GGML_TYPE_F16, c.nkv, c.mask.shape[1]) if c.mask is not None else None
        self.sk = ctx.new_tensor(pkg.GGML_TYPE_F32, c.nh) if c.sinks is not None else None
        self.y = ctx.flash_attn_ext(self.q, self.k, self.v, self.m, c.scale, c.max_bias, c.softcap, self.sk)
        ctx.alloc()
        self.g = ctx.graph()

    def run(self, c):
        be = self.be
        be.tensor_set(self.q, c.q)
        for t, x in ((self.k, c.k), (self.v, c.v)) if not self.view else ((self.kc, c.k), (self.vc, c.v)):
            if self.view:                                       # cell-major rows: one unused block, then the KV heads' blocks
                nb = c.D // 32
                rows = np.zeros((self.n_ctx, c.nhkv * nb + 1, x.shape[-1]), np.uint8)
                rows[:c.nkv, 1:] = x.reshape(c.nhkv, c.nkv, nb, -1).transpose(1, 0, 2, 3).reshape(c.nkv, c.nhkv * nb, -1)
                x = rows
            be.tensor_set(t, x)
        if self.m is not None:
            be.tensor_set(self.m, c.mask)
        if self.sk is not None:
            be.tensor_set(self.sk, c.sinks)
        be.graph_compute(self.g)
        return be.tensor_get(self.y).astype(np.float64).reshape(c.ns, c.nq, c.nh, c.D)


@pytest.mark.parametrize("name", list(CASES))
def test_flash_attn_quantised_cache_matrix_core_kernel(pkg, be, request, name):
    from oracle.ref_backend import ref_available
    c, n_kernels, view = _case(name), CASES[name][-1], CASES[name][7] == "view"
    want = fn.reference(_attn_f64, c)
    g = _Graph(pkg, be, c, view)
    got = {}
    try:
        for mode in (-1, 0):
            be.set_option("fattn_q", mode)
            try:
                n0 = be.get_stat("fattn_q_launches")
                got[mode] = g.run(c)
                counts = (be.get_stat("fattn_q_launches") - n0, be.get_stat("kernels_last_graph"))
            finally:
                be.set_option("fattn_q", -1)
            assert counts == ((1, n_kernels) if mode else (0, 1)), (name, mode, counts)
    finally:
        g.c.free()
    ref = None
    if ref_available():
        gr = _Graph(pkg, request.getfixturevalue("ref_be"), c, view)
        try:
            ref = gr.run(c)
        finally:
            gr.c.free()
    for mode, out in got.items():
        assert np.isfinite(out).all(), (name, mode)
        e, at, en = fn.check_rows(out, want, c.needles)
        print(f"{name} fattn_q {mode}: worst row NMSE vs f64 {e:.3e} at (s, t, h) = {at}, worst needle row {en:.3e}")
        assert e < fn.BAR, (name, mode, e, at)
    e_any, e_ref = nmse(got[-1], got[0]), nmse(got[-1], ref) if ref is not None else None
    print(f"{name}: k_fattn_q vs k_fattn_any NMSE {e_any:.3e}, vs the reference backend {e_ref if e_ref is None else format(e_ref, '.3e')}")
    assert e_any < 1e-9, (name, e_any)
    assert e_ref is None or e_ref < 1e-9, (name, e_ref)
