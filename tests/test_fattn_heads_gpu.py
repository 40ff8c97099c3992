"""FLASH_ATTN_EXT at head sizes 40, 72, 80, 96, 112 and 192 / 128 on k_fattn_wide (csrc/kernels/fattn_wide.hip), -m gpu.

These sizes are no multiple of the kernel's MFMA extents: DK is padded to 16 (40 -> 48, 72 -> 80), DV to 32 (40 -> 64, 72 / 80 -> 96, 112 -> 128), the
staging loops have idle threads in their last round and the output rows end inside a 32-dim block.  The cases are the smallest shapes on each side of each
of those edges; the method, the inputs (tests/fattn_needle.py: needle rows that see ONE cell at score 24, masked decoys at 48 behind every mask edge, sinks
that make a row exactly a quarter), the single-node graphs and the bars (NMSE < 5e-4 over the whole output AND per output row, the output finite, against
the float64 restatement and against the reference CPU backend where it travelled) are those of tests/test_fattn_wide_gpu.py, whose helpers run here on the
table below.

Every case asserts which kernel ran: the "fattn_wide_launches" delta is >= 1 where fa_wide_plan (fattn.hip) takes the shape and 0 where it does not, and 0
again with option "fattn_wide" = 0 (the generic kernel: the cross-check, held to the same bar); kernels_last_graph is 1 with one slice and 2 with slices +
k_fattn_merge.  Before these head sizes were on fattn_wide_dims every "taken" case ran on the generic kernel: delta 0.

test_padding_is_written_by_the_kernel: the K tile's columns DK .. DKP - 1 enter every score, so they must be zeros the kernel wrote, not what the LDS held.
The same graph runs before and after an attention at 256 / 256 over K and V of magnitude 1e4 -- a workgroup of which fills the whole LDS range the small
heads use -- and must give the same bits."""
import numpy as np
import pytest

import fattn_needle as fn
import test_fattn_wide_gpu as wide
from test_fattn_needle_gpu import _Graph, _ref_backend
from test_fattn_wide_gpu import _judge, _run_counted
from test_gpu_parity import _attn_f64

pytestmark = pytest.mark.gpu

# name: (DK, DV, tokens, heads, KV heads, cache rows, sequences, mask kinds, cache type, softcap, taken by the plan, kernels_last_graph)
CASES = {
    # 4 live columns of 32; 70 = 2 * 32 + 6: a ragged last KV tile whose last row is visible (no mask)
    "h96_one":      (96, 96, 1, 8, 2, 70, 1, ("none", "causal"), "f16", 0.0, True, 1),
    # 40 heads of one KV head: the gq >= 32 branch, the second column tile with 8 live columns
    "h96_heads40":  (96, 96, 2, 40, 1, 70, 1, ("causal",), "f16", 0.0, True, 1),
    # soft-cap before the mask; sinks; 9 KV tiles; three sequences
    "h96_cap":      (96, 96, 1, 8, 4, 257, 3, ("sinks",), "f16", 30.0, True, 1),
    # DV padded 80 -> 96; 320 K chunks and 160 V chunk pairs for 256 threads: guarded last rounds; the second half of the view is unused cells: dead tail tiles
    "h80_prefill":  (80, 80, 33, 4, 2, 130, 1, ("padded",), "f16", 0.0, True, 1),
    # DV padded 112 -> 128; sliding window: columns with nothing visible inside a live tile before they have seen anything (M = -inf meets s = -inf)
    "h112_window":  (112, 112, 65, 4, 2, 200, 2, ("window",), "f16", 0.0, True, 1),
    # 17 KV tiles (530 rows, ragged): 16 workgroups without a split -> min(512 / 16, 17 / 4) = 4 slices of 5 tiles + k_fattn_merge<128>, sinks applied there, once
    "h192_deep":    (192, 128, 1, 8, 8, 530, 2, ("sinks",), "f16", 0.0, True, 2),
    # DK != DV; 3 heads per KV head: 10 tokens x 3 heads per tile, two idle columns
    "h192_gq3":     (192, 128, 5, 6, 2, 100, 1, ("causal",), "f16", 0.0, True, 1),
    # DK padded 40 -> 48 (the last MFMA step half inside the row) and DV 40 -> 64
    "h40_gq3":      (40, 40, 5, 6, 2, 100, 1, ("causal",), "f16", 0.0, True, 1),
    # DK padded 72 -> 80, DV 72 -> 96; no mask; exactly two full KV tiles; one head per KV head
    "h72_nomask":   (72, 72, 33, 4, 4, 64, 1, ("none",), "f16", 0.0, True, 1),
    # what the plan leaves to the generic kernel
    "gen_per_head": (96, 96, 4, 4, 2, 100, 1, ("per_head",), "f16", 0.0, False, 1),
    "gen_alibi":    (96, 96, 2, 4, 2, 100, 1, ("alibi",), "f16", 0.0, False, 1),
    "gen_q8_0":     (96, 96, 3, 4, 2, 96, 1, ("causal",), "q8_0", 0.0, False, 1),
    "gen_48":       (48, 48, 3, 4, 2, 100, 1, ("causal",), "f16", 0.0, False, 1),         # a size that is not on fattn_wide_dims
}
IDS = [f"{n}-{k}" for n, cs in CASES.items() for k in cs[7]]


@pytest.fixture(autouse=True)
def _heads_table(monkeypatch):
    """test_fattn_wide_gpu's _build / _rounds (the "window" mask kind and its second decoy included) look their shapes up in that module's CASES: this table joins it"""
    monkeypatch.setattr(fn, "base_mask", wide._mask)
    monkeypatch.setattr(wide, "CASES", {**wide.CASES, **CASES})


@pytest.mark.parametrize("cid", IDS)
def test_heads_needle_rows(pkg, be, request, cid):
    name, kind = cid.rsplit("-", 1)
    taken, n_kernels = CASES[name][10:12]
    ref_be = _ref_backend(request)
    c = wide._build(name, kind, 0)
    g = _Graph(pkg, be, c)
    gref = _Graph(pkg, ref_be, c) if ref_be is not None else None
    try:
        for rd in range(wide._rounds(name, kind)):
            c = wide._build(name, kind, rd) if rd else c
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


@pytest.mark.parametrize("name,kind", [("h80_prefill", "padded"), ("h40_gq3", "causal")])
def test_padding_is_written_by_the_kernel(pkg, be, name, kind):
    c = wide._build(name, kind, 0)
    big = wide._build("g_nomask", "none", 0)                 # 256 / 256: K tile 16896 + V^T tile 17408 bytes per workgroup, over the 5632 + 6528 (80) and 3584 + 4352 (40) of the small heads
    for key in ("k", "v"):                                   # large and finite in f16
        setattr(big, key, np.clip(getattr(big, key).astype(np.float32) * 1e4, -6e4, 6e4).astype(np.float16))
    g, gb = _Graph(pkg, be, c), _Graph(pkg, be, big)
    try:
        first, launched, _ = _run_counted(be, lambda: g.run(c), -1)
        _judge(f"{name} first run", c, first, fn.reference(_attn_f64, c), None)
        assert launched >= 1, launched
        _, launched_big, _ = _run_counted(be, lambda: gb.run(big), -1)
        assert launched_big >= 1, launched_big
        second, launched, _ = _run_counted(be, lambda: g.run(c), -1)
        assert launched >= 1, launched
        assert np.array_equal(first, second), (name, float(np.abs(first - second).max()))
    finally:
        g.free(); gb.free()
