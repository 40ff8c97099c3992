"""The boundaries FLASH_ATTN_EXT's kernel choice draws (flash_attn_ext_f16 and its predicates, fattn.hip), one shape on each side of each (-m gpu): single-node graphs
through the C-ABI against the reference CPU backend, bar = the reference's FLASH_ATTN_EXT NMSE 5e-4 (the bar of the FLASH_ATTN_EXT
cases in test_gpu_parity.py), plus the launch counters kernels_last_graph, fattn_gs_launches and fattn_dma_launches.  The counters tell
the two sides apart only where the sides differ in launches: 32 / 33 tokens and 8 / 9 tokens without the decode tiles (the mask tile map),
256 / 257 rows, 32 / 33 heads per KV head.  The other pairs -- 1023 / 1024 rows (both report 2), 8 tokens on the decode tiles or the
streaming kernel (both 1), head size 80 and the Q8_0 cache on the generic kernel (1, as a specialised kernel would give) -- are parity-only:
a wrong kernel choice that still computes correct attention would pass them.  A single node has no q / k / v chains in front of it, so the
one-token kernels of the pre-stage are not reached here (tests/test_round6_gpu.py drives them through a model).
All shapes have 2 - 8 heads except the 32 / 33 heads-per-KV-head pair, which needs that many heads over its one KV head."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

# name: (D, nq, nh, nhkv, nkv, mask, cache type, option fattn_gqa, kernels_last_graph)
# kernels_last_graph counts the launch, + 1 for the mask tile map of the prefill kernel, + 1 whenever the executor hands the KV-split
# scratch over (the merge pass; for one token over 257 .. 8192 rows it is handed over -- and counted -- even when the kernel that runs
# takes one slice: the scratch is sized for the one-token kernel's slices there.  For one_257_dec and one_1023_dec that makes the stat say 2
# where ONE launch happens: the value pinned here is what the executor reports today, not a correct count -- whoever fixes the stat changes
# these two to 1, and that is no regression)
CASES = {
    "nq8_gqa":            (128, 8, 4, 2, 96, "shared", "f16", 1, 1),       # <= 8 tokens: matrix-core decode tiles whatever the depth
    "nq9_gqa":            (128, 9, 4, 2, 96, "shared", "f16", 1, 1),       # 9 .. 32 tokens: still the decode tiles (the prefill kernel could)
    "nq32_gqa":           (128, 32, 4, 2, 96, "shared", "f16", 1, 1),
    "nq33_mma":           (128, 33, 4, 2, 96, "shared", "f16", 1, 2),      # more than 32: the prefill kernel + its mask tile map
    "nq9_mma_gqa_off":    (128, 9, 4, 2, 96, "shared", "f16", 0, 2),       # more than 8 without the decode tiles: the prefill kernel
    "nq8_dec_gqa_off":    (128, 8, 4, 2, 96, "shared", "f16", 0, 1),       # ... up to 8: the streaming kernel
    "one_256_stream":     (128, 1, 4, 2, 256, "shared", "f16", 1, 1),      # one token, <= 8 tiles of 32 rows: the streaming kernel
    "one_257_gqa_split":  (128, 1, 4, 2, 257, "shared", "f16", 1, 2),      # 9 tiles: decode tiles, KV slices + merge
    "one_257_dec":        (128, 1, 4, 2, 257, "shared", "f16", 0, 2),      # streaming kernel, one slice, one launch; reported as 2 (see above)
    "one_1023_dec":       (128, 1, 4, 2, 1023, "shared", "f16", 0, 2),     # below the streaming kernel's 1024-row split threshold: one launch, reported as 2
    "one_1024_dec_split": (128, 1, 4, 2, 1024, "shared", "f16", 0, 2),     # at it: four slices + merge
    "one_1023_gqa":       (128, 1, 4, 2, 1023, "shared", "f16", 1, 2),
    "one_1024_gqa":       (128, 1, 4, 2, 1024, "shared", "f16", 1, 2),
    "gq33_dec":           (128, 2, 33, 1, 300, "shared", "f16", 1, 1),     # 33 heads per KV head (one KV head: 33 heads): falls off the 32-column tiles
    "gq32_gqa":           (128, 2, 32, 1, 300, "shared", "f16", 1, 2),     # 32: on them (10 tiles: slices + merge)
    "per_head_mask_dec":  (128, 4, 4, 2, 300, "per_head", "f16", 1, 1),    # a mask per head: the streaming kernel
    "d80_any":            (80, 3, 4, 2, 100, "shared", "f16", 1, 1),       # another head size: the generic kernel
    "q8_0_cache_any":     (128, 2, 4, 2, 96, "shared", "q8_0", 1, 1),      # a quantised cache at head size 128: the generic kernel
    "kv_split_planner":   (64, 2, 8, 2, 2048, "none", "f16", 1, 2),        # deep cache: 16 slices in the scratch as the planner sized it
}

_REF = {}


def _q8_0(x):
    rows, n = x.shape
    b = x.reshape(rows, n // 32, 32)
    d = (np.abs(b).max(-1) / 127.0).astype(np.float16)
    q = np.rint(b / np.where(d == 0, 1, d).astype(np.float32)[..., None]).clip(-127, 127).astype(np.int8)
    out = np.zeros((rows, n // 32, 34), np.uint8)
    out[..., :2] = d[..., None].view(np.uint8).reshape(rows, n // 32, 2); out[..., 2:] = q.view(np.uint8)
    return out


def _run(pkg, backend, name, feeds=None):
    D, nq, nh, nhkv, nkv, mask, kv_type, _, _ = CASES[name]
    if feeds is None:
        rng = np.random.default_rng(sum(map(ord, name)))
        kf = rng.standard_normal((nhkv * nkv, D)).astype(np.float32); vf = rng.standard_normal((nhkv * nkv, D)).astype(np.float32)
        enc = _q8_0 if kv_type == "q8_0" else (lambda x: x.astype(np.float16))
        mv = None
        if mask != "none":                                    # causal over the last rows of the cache, a -inf tail; per head: each head its own window
            nm = nh if mask == "per_head" else 1
            mv = np.zeros((nm, 64, nkv), np.float16)
            for h in range(nm):
                for t in range(64):
                    mv[h, t, max(1, nkv - 37 - 11 * h) + min(t, nq - 1):] = -np.inf
        feeds = (rng.standard_normal((nh, nq, D)).astype(np.float32), enc(kf), enc(vf), mv)
    qv, kv, vv, mv = feeds
    c = pkg.Context(backend)
    T = pkg.GGML_TYPE_Q8_0 if kv_type == "q8_0" else pkg.GGML_TYPE_F16
    q = c.new_tensor(pkg.GGML_TYPE_F32, D, nq, nh); k = c.new_tensor(T, D, nkv, nhkv); v = c.new_tensor(T, D, nkv, nhkv)
    m = None
    if mv is not None:
        m = c.new_tensor(pkg.GGML_TYPE_F16, nkv, 64, mv.shape[0]) if mv.shape[0] > 1 else c.new_tensor(pkg.GGML_TYPE_F16, nkv, 64)
    y = c.flash_attn_ext(q, k, v, m, 1.0 / np.sqrt(D))
    c.alloc()
    backend.tensor_set(q, qv); backend.tensor_set(k, kv); backend.tensor_set(v, vv)
    if m is not None:
        backend.tensor_set(m, mv)
    backend.graph_compute(c.graph())
    out = backend.tensor_get(y).copy()
    c.free()
    return out, feeds


def _reference(pkg, ref_be, name):
    """inputs and the reference CPU backend's rows, once per case"""
    if name not in _REF:
        want, feeds = _run(pkg, ref_be, name)
        want.setflags(write=False)
        _REF[name] = (want, feeds)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_fattn_plan_boundaries(pkg, be, ref_be, name):
    gqa, n_kernels = CASES[name][7:]
    want, feeds = _reference(pkg, ref_be, name)
    be.set_option("fattn_gqa", gqa)
    try:
        gs0, dma0 = be.get_stat("fattn_gs_launches"), be.get_stat("fattn_dma_launches")
        got, _ = _run(pkg, be, name, feeds)
        counts = (be.get_stat("kernels_last_graph"), be.get_stat("fattn_gs_launches") - gs0, be.get_stat("fattn_dma_launches") - dma0)
    finally:
        be.set_option("fattn_gqa", 1)
    e = nmse(got, want)
    print(name, "NMSE", e, "kernels / group-slice / ring launches", counts)
    assert np.isfinite(got).all()
    assert e < 5e-4, (name, e)
    assert counts == (n_kernels, 0, 0), (name, counts)      # no pre-stage: never the group-slice form; under 512 workgroups: never the ring form
