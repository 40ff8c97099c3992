"""FLASH_ATTN_EXT at head sizes 256 / 256 (Gemma 2 / 3) and 576 / 512 (DeepSeek MLA): k_fattn_wide (csrc/kernels/fattn_wide.hip), -m gpu.

Single-node graphs through the C-ABI, built as test_fattn_needle_gpu.py builds them, on the positioned inputs of tests/fattn_needle.py: a few rows per
KV head see ONE cache cell at score 24 (their output is that cell's V row), masked decoys at score 48 sit right behind every mask edge, a sink makes
a row exactly a quarter.  tests/test_fattn_needle_host.py shows on the CPU that a cell dropped, read twice or leaked through the mask moves its row
by a per-row NMSE >= 0.1.

Bar: the project's and the reference's bar for this op, NMSE < 5e-4 over the whole output AND per output row, the output finite -- against the float64
restatement (_attn_f64, test_gpu_parity.py) and against the reference CPU backend where it travelled.  The measured figures are printed.

Every case asserts which kernel ran: the "fattn_wide_launches" delta is >= 1 where fa_wide_plan (fattn.hip) takes the shape and 0 where it does not, and
0 again with option "fattn_wide" = 0 (the generic kernel: the cross-check, held to the same bar); kernels_last_graph is 1 with one slice and 2 with
slices + merge.  The plan slices above 16 KV tiles (n_kv > 512) when the un-split grid is small."""
import numpy as np
import pytest

import fattn_needle as fn
from conftest import nmse
from test_fattn_needle_gpu import _Graph, _ref_backend
from test_gpu_parity import _attn_f64

pytestmark = pytest.mark.gpu

BAR = fn.BAR                                # 5e-4
WINDOW = 40                                 # cells a row of the sliding-window mask sees, ending at its own position
WINDOW_END = 150                            # the last row's position: the view's cells behind it are dead tiles

# name: (DK, DV, tokens, heads, KV heads, cache rows, sequences, mask kinds, cache type, softcap, taken by the plan, kernels_last_graph)
CASES = {
    # 40 heads of one KV head: two column tiles, the second with 8 live columns; 70 = 2 * 32 + 6: a ragged last KV tile whose last row is visible (no mask)
    "mla_one":       (576, 512, 1, 40, 1, 70, 1, ("none", "causal"), "f16", 0.0, True, 1),
    # the model's 128 heads: four column tiles on the same staged K / V; two sequences
    "mla_heads128":  (576, 512, 1, 128, 1, 96, 2, ("causal",), "f16", 0.0, True, 1),
    # 17 KV tiles (530 rows, ragged): above the 16-tile threshold, 2 workgroups without a split -> 4 slices of 5 tiles + k_fattn_merge<512>, sinks applied there, once
    "mla_deep":      (576, 512, 1, 40, 1, 530, 2, ("sinks",), "f16", 0.0, True, 2),
    # 8 tokens x 4 heads per column tile, the last tile with one token; causal mask padded to 64 rows; the second half of the view is unused cells: dead tail tiles
    "mla_prefill":   (576, 512, 33, 4, 1, 130, 1, ("padded",), "f16", 0.0, True, 1),
    # 2 live columns of 32; 9 KV tiles; soft-cap before the mask; sinks
    "g_one":         (256, 256, 1, 8, 4, 257, 3, ("sinks",), "f16", 50.0, True, 1),
    # sliding window: leading and trailing dead tiles, columns with nothing visible inside a live tile before they have seen anything (M = -inf meets s = -inf)
    "g_window":      (256, 256, 65, 4, 2, 200, 2, ("window",), "f16", 0.0, True, 1),
    # 3 heads per KV head: 10 tokens x 3 heads per tile, two idle columns
    "g_gq3":         (256, 256, 5, 6, 2, 100, 1, ("causal",), "f16", 0.0, True, 1),
    # no mask; exactly two full KV tiles
    "g_nomask":      (256, 256, 33, 2, 2, 64, 1, ("none",), "f16", 0.0, True, 1),
    # what the plan leaves to the generic kernel
    "gen_per_head":  (256, 256, 4, 4, 2, 100, 1, ("per_head",), "f16", 0.0, False, 1),
    "gen_alibi":     (256, 256, 2, 4, 2, 100, 1, ("alibi",), "f16", 0.0, False, 1),
    "gen_q8_0":      (256, 256, 3, 4, 2, 96, 1, ("causal",), "q8_0", 0.0, False, 1),
    "gen_256_128":   (256, 128, 3, 4, 2, 100, 1, ("causal",), "f16", 0.0, False, 1),
}
MAX_ROUNDS = 3                              # needles moved over the edges; the first rounds hold each row's last live cell and the first cell of its last tile

_base_mask = fn.base_mask


def _mask(kind, nq, nh, nkv, tile=None):
    """fattn_needle.base_mask plus "window": row t at position p = WINDOW_END - (nq - 1) + t sees cells p - WINDOW + 1 .. p"""
    if kind != "window":
        return _base_mask(kind, nq, nh, nkv, tile)
    nq_pad = (nq + 63) // 64 * 64
    m = np.full((1, nq_pad, nkv), fn.NINF, np.float16)
    for t in range(nq_pad):
        p = WINDOW_END - (nq - 1) + min(t, nq - 1)
        m[0, t, p - WINDOW + 1:p + 1] = 0
    return m


@pytest.fixture(autouse=True)
def _window_kind(monkeypatch):
    monkeypatch.setattr(fn, "base_mask", _mask)


def _build(name, kind, rd):
    DK, DV, nq, nh, nhkv, nkv, ns, _, kv_type, softcap, _, _ = CASES[name]
    c = fn.make_case(DK, DV, nq, nh, nhkv, nkv, ns, kind, rd, sum(map(ord, name + kind)), kv_type, softcap)
    if kind == "window":                    # a masked decoy right in FRONT of each needle row's window too (make_case puts one behind it)
        k16 = c.k.reshape(ns, nhkv, nkv, DK)
        for (s, h, t, _) in c.needles:
            x = WINDOW_END - (nq - 1) + t - WINDOW
            qv = c.q[s, h, t].astype(np.float16).astype(np.float64)
            w = 2 * fn.L * qv / (c.scale * (qv * qv).sum())
            k16[s, h // (nh // nhkv), x] = (k16[s, h // (nh // nhkv), x].astype(np.float64) + w).astype(np.float16)
            c.kd[s, h // (nh // nhkv), x] = k16[s, h // (nh // nhkv), x].astype(np.float32)
            c.decoys[(s, h, t)] = c.decoys[(s, h, t)] + [x]
    return c


def _rounds(name, kind):
    DK, DV, nq, nh, nhkv, nkv, ns = CASES[name][:7]
    return min(MAX_ROUNDS, fn.n_rounds(DK, nq, nh, nhkv, nkv, ns, kind))


def _judge(tag, c, got, want, ref):
    """print what is measured, then hold the whole output and every row to the bar"""
    assert np.isfinite(got).all(), tag
    e, at, en = fn.check_rows(got, want, c.needles)
    whole = nmse(got, want)
    line = f"{tag}: NMSE vs f64 {whole:.3e}, worst row {e:.3e} at (s, t, h) = {at}, worst needle row {en:.3e}"
    er = None
    if ref is not None:
        er, at_r, _ = fn.check_rows(got, ref, c.needles)
        line += f"; vs reference backend {nmse(got, ref):.3e}, worst row {er:.3e} at {at_r}"
    print(line)
    assert whole < BAR and e < BAR, (tag, whole, e, at, [n for n in c.needles if (n[0], n[2], n[1]) == at])
    if er is not None:
        assert er < BAR and nmse(got, ref) < BAR, (tag, er, at_r)


def _run_counted(be, run, wide):
    """run() with option fattn_wide = wide -> (output, fattn_wide_launches delta, kernels_last_graph)"""
    be.set_option("fattn_wide", wide)
    try:
        n0 = be.get_stat("fattn_wide_launches")
        got = run()
        return got, int(be.get_stat("fattn_wide_launches") - n0), int(be.get_stat("kernels_last_graph"))
    finally:
        be.set_option("fattn_wide", -1)


def test_inputs_are_sound_on_the_host():
    """the float64 restatement on the new inputs (no GPU): finite, every row has a visible cell, and every needle row IS its needle's V row (x 1/4 under a sink)"""
    for name, cs in CASES.items():
        for kind in cs[7]:
            c = _build(name, kind, 0)
            if c.mask is not None:
                assert (~np.isneginf(c.mask[:, :c.nq])).any(-1).all(), (name, kind)
            want = fn.reference(_attn_f64, c)
            assert np.isfinite(want).all(), (name, kind)
            if kind != "alibi":
                for (s, h, t, cell) in c.needles:
                    assert fn.row_nmse(want[s, t, h][None], fn.expected_row(c, s, h, t, cell)[None])[0] < 1e-6, (name, kind, s, h, t, cell)


@pytest.mark.parametrize("cid", [f"{n}-{k}" for n, cs in CASES.items() for k in cs[7]])
def test_wide_heads_needle_rows(pkg, be, request, cid):
    name, kind = cid.rsplit("-", 1)
    taken, n_kernels = CASES[name][10:12]
    ref_be = _ref_backend(request)
    c = _build(name, kind, 0)
    g = _Graph(pkg, be, c)
    gref = _Graph(pkg, ref_be, c) if ref_be is not None else None
    try:
        for rd in range(_rounds(name, kind)):
            c = _build(name, kind, rd) if rd else c
            want = fn.reference(_attn_f64, c)
            ref = gref.run(c) if gref is not None else None
            got, launched, kernels = _run_counted(be, lambda: g.run(c), -1)
            _judge(f"{cid} round {rd}", c, got, want, ref)
            assert (launched >= 1) == taken and (taken or launched == 0), (cid, launched)
            assert kernels == n_kernels, (cid, kernels)
            if rd == 0:                     # the cross-check: the generic kernel on the same graph
                got0, launched0, kernels0 = _run_counted(be, lambda: g.run(c), 0)
                _judge(f"{cid} fattn_wide 0", c, got0, want, ref)
                assert launched0 == 0 and kernels0 == 1, (cid, launched0, kernels0)
    finally:
        g.free()
        if gref is not None:
            gref.free()


class _Strided:
    """the operands as libllama passes them: Q a permuted view of [D, heads, tokens]; K / V [D, n_kv, n_head_kv] views of caches whose rows hold all KV heads
    and that are longer than n_kv"""

    def __init__(self, pkg, backend, c, n_ctx):
        F32, F16 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16
        self.be, self.n_ctx = backend, n_ctx
        self.c = g = pkg.Context(backend)
        HK = c.nhkv
        self.qc = g.new_tensor(F32, c.D, c.nh, c.nq)
        self.kc = g.new_tensor(F16, c.D * HK, n_ctx)
        self.vc = g.new_tensor(F16, c.Dv * HK, n_ctx)
        q = g.permute(self.qc, 0, 2, 1, 3)
        k = g.view_3d(self.kc, c.D, c.nkv, HK, c.D * HK * 2, c.D * 2, 0)
        v = g.view_3d(self.vc, c.Dv, c.nkv, HK, c.Dv * HK * 2, c.Dv * 2, 0)
        self.m = g.new_tensor(F16, c.nkv, c.mask.shape[1])
        self.y = g.flash_attn_ext(q, k, v, self.m, c.scale, 0.0, 0.0, None)
        g.alloc()
        self.g = g.graph([self.y])

    def run(self, c, rng):
        be, HK = self.be, c.nhkv
        kv = rng.standard_normal((self.n_ctx, HK, c.D)).astype(np.float16)          # the cells past n_kv hold other values: never read
        vv = rng.standard_normal((self.n_ctx, HK, c.Dv)).astype(np.float16)
        kv[:c.nkv] = c.k.reshape(HK, c.nkv, c.D).transpose(1, 0, 2)
        vv[:c.nkv] = c.v.reshape(HK, c.nkv, c.Dv).transpose(1, 0, 2)
        be.tensor_set(self.qc, np.ascontiguousarray(c.q[0].transpose(1, 0, 2)))
        be.tensor_set(self.kc, kv); be.tensor_set(self.vc, vv); be.tensor_set(self.m, c.mask)
        be.graph_compute(self.g)
        return be.tensor_get(self.y).astype(np.float64).reshape(1, c.nq, c.nh, c.Dv)

    def free(self):
        self.c.free()


@pytest.mark.parametrize("DK,DV,nh,nhkv", [(576, 512, 8, 1), (256, 256, 4, 2)])
def test_wide_heads_strided_operands(pkg, be, request, DK, DV, nh, nhkv):
    ref_be = _ref_backend(request)
    nq, nkv, n_ctx = 3, 77, 128
    c = fn.make_case(DK, DV, nq, nh, nhkv, nkv, 1, "causal", 0, DK + nh)
    want = fn.reference(_attn_f64, c)
    g = _Strided(pkg, be, c, n_ctx)
    gref = _Strided(pkg, ref_be, c, n_ctx) if ref_be is not None else None
    try:
        ref = gref.run(c, np.random.default_rng(1)) if gref is not None else None
        got, launched, kernels = _run_counted(be, lambda: g.run(c, np.random.default_rng(1)), -1)
        _judge(f"strided {DK}/{DV}", c, got, want, ref)
        assert launched >= 1 and kernels == 1, (launched, kernels)
        got0, launched0, _ = _run_counted(be, lambda: g.run(c, np.random.default_rng(1)), 0)
        _judge(f"strided {DK}/{DV} fattn_wide 0", c, got0, want, ref)
        assert launched0 == 0, launched0
    finally:
        g.free()
        if gref is not None:
            gref.free()
