"""Mixed K / V cache types and Q4_1 / Q5_0 / Q5_1 caches (-m gpu): SET_ROWS into such tables byte for byte against the reference CPU backend, and
FLASH_ATTN_EXT at head size 64 / 128 on k_fattn_qx (fattn_qx.hip) against the float64 restatement, the generic kernel (option "fattn_qx" = 0) and the reference
backend.

Attention inputs are tests/fattn_needle.py's needle cases built on f32 caches and then encoded per operand (the needles then score 24 up to the quantisation
error of their key -- every row is still compared with the float64 attention on the values the kernels read).  Per case: "fattn_qx_launches" rises by 1 at the
default and by 0 with the option off, "fattn_q_launches" never moves, the output is finite, every row is within fn.BAR = 5e-4 of the float64 attention on the
de-quantised caches with the query read as Q8_0 blocks (K's vec_dot_type; the Q8_1 form of Q4_1 / Q5_1 K has the same quants and d, its s differs from d * sum
by one f16 rounding), and the whole output is within NMSE 1e-9 of the generic kernel's (both accumulate V in f32) and of the reference backend's -- 5e-4 for
the reference where V is F16: it rounds its accumulator to f16 at every cell (ops.cpp:8069-8083)."""
import numpy as np
import pytest

import fattn_needle as fn
from conftest import nmse
from test_gpu_parity import _attn_f64

pytestmark = pytest.mark.gpu

TYPES = {"f16": 1, "q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}


def _encode(x, t):
    """rows [n, D] f32 -> (block bytes [n, D / 32, bb] -- f16 rows for "f16" --, the f32 values d * q [+ m] a reader de-quantises them to); q4_1 {f16 d, m; qs[16]},
    q5_0 {f16 d; qh[4]; qs[16]}, q5_1 {f16 d, m; qh[4]; qs[16]}: element j in the low nibble of qs[j] and bit j of qh, j + 16 in the high nibble and bit j + 16"""
    if t in ("f16", "q8_0", "q4_0"):
        return fn.encode(x, t)
    b = x.reshape(len(x), -1, 32).astype(np.float32)
    if t == "q5_0":
        d = (np.take_along_axis(b, np.abs(b).argmax(-1)[..., None], -1)[..., 0] / -16.0).astype(np.float16)
        m, off, top = None, 16, 31
    else:
        top = 15 if t == "q4_1" else 31
        m, d, off = b.min(-1).astype(np.float16), ((b.max(-1) - b.min(-1)) / top).astype(np.float16), 0
    d32, m32 = d.astype(np.float32)[..., None], 0 if m is None else m.astype(np.float32)[..., None]
    q = np.clip(np.rint((b - m32) / np.where(d32 == 0, 1, d32)) + off, 0, top).astype(np.uint32)
    qh = ((q >> 4) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
    qs = ((q[..., :16] & 15) | ((q[..., 16:] & 15) << 4)).astype(np.uint8)
    parts = [d[..., None].view(np.uint8)] + ([] if m is None else [m[..., None].view(np.uint8)]) + ([] if t == "q4_1" else [qh[..., None].view(np.uint8)]) + [qs]
    return np.concatenate(parts, -1), (d32 * (q.astype(np.float32) - off) + m32).astype(np.float32).reshape(len(x), -1)


# name: (K type, V type, D, nq, heads, KV heads, n_kv, sequences, mask kind, softcap)
CASES = {
    "ragged_tile_f16_v":     ("q8_0", "f16", 128, 1, 4, 1, 37, 1, "causal", 0.0),       # cells 32 and 33 live in a 5-cell second tile; F16 V staging
    "column_tiles_ragged":   ("q8_0", "q4_0", 64, 35, 4, 4, 130, 1, "causal", 0.0),     # 5 column tiles per KV head: the second workgroup has three idle waves
    "both_mins_gq3":         ("q4_1", "q5_1", 128, 5, 6, 2, 70, 1, "causal", 0.0),      # both min terms; gq 3: columns 30 / 31 idle
    "fifth_bit_gq33":        ("q5_0", "q8_0", 64, 2, 33, 1, 96, 1, "causal", 0.0),      # two column tiles per token, the second with one head
    "no_mask_two_sequences": ("q5_1", "q4_1", 128, 3, 4, 2, 64, 2, "none", 0.0),
    "softcap_sinks":         ("q4_0", "q5_0", 128, 2, 8, 2, 100, 1, "sinks", 30.0),
    "sliced_merge_f16_v":    ("q4_1", "f16", 128, 1, 8, 2, 513, 1, "causal", 0.0),      # 17 tiles: 4 slices + k_fattn_merge
    "view_cell_major":       ("q5_1", "q5_1", 128, 3, 8, 2, 70, 1, "view", 0.0),        # K / V views of [n_ctx][(2 heads x 4 + 1) blocks]: cell stride 216, offset 24 bytes
    "same_type_q8_0":        ("q8_0", "q8_0", 128, 2, 4, 2, 70, 1, "causal", 0.0),      # k_fattn_q's pair: the existing route, untouched
}


def _case(name):
    kt, vt, D, nq, nh, nhkv, nkv, ns, kind, softcap = CASES[name]
    c = fn.make_case(D, D, nq, nh, nhkv, nkv, ns, "causal" if kind == "view" else kind, 0, sum(map(ord, name)), "f32", softcap)
    c.k, kd = _encode(c.kd.reshape(-1, D), kt); c.v, vd = _encode(c.vd.reshape(-1, D), vt)
    c.kd, c.vd, c.kv_type = kd.reshape(c.kd.shape), vd.reshape(c.vd.shape), "q8_0"      # (kv_type: how fn.reference reads the query)
    return c


def _run(pkg, backend, c, kt, vt, view, ours=True):
    """one FLASH_ATTN_EXT node (test_fattn_q_gpu.py's), K / V optionally views into cell-major caches of all KV heads plus one leading block"""
    ctx = pkg.Context(backend)
    try:
        q = ctx.new_tensor(pkg.GGML_TYPE_F32, c.D, c.nq, c.nh, c.ns)
        ops = []
        for t, x in ((kt, c.k), (vt, c.v)):
            if view:
                n_ctx, bb, nb = c.nkv + 7, x.shape[-1], c.D // 32
                cache = ctx.new_tensor(TYPES[t], c.nhkv * c.D + 32, n_ctx)
                rows = np.zeros((n_ctx, c.nhkv * nb + 1, bb), np.uint8)
                rows[:c.nkv, 1:] = x.reshape(c.nhkv, c.nkv, nb, bb).transpose(1, 0, 2, 3).reshape(c.nkv, c.nhkv * nb, bb)
                ops.append((ctx.view_3d(cache, c.D, c.nkv, c.nhkv, (c.nhkv * nb + 1) * bb, nb * bb, bb), cache, rows))
            else:
                T = ctx.new_tensor(TYPES[t], c.D, c.nkv, c.nhkv, c.ns)
                ops.append((T, T, x))
        m = ctx.new_tensor(pkg.GGML_TYPE_F16, c.nkv, c.mask.shape[1]) if c.mask is not None else None
        sk = ctx.new_tensor(pkg.GGML_TYPE_F32, c.nh) if c.sinks is not None else None
        y = ctx.flash_attn_ext(q, ops[0][0], ops[1][0], m, c.scale, c.max_bias, c.softcap, sk)
        ctx.alloc()
        assert not ours or backend.supports_op(y), (kt, vt)
        for t, x in [(q, c.q), (m, c.mask), (sk, c.sinks)] + [(o[1], o[2]) for o in ops]:
            if t is not None:
                backend.tensor_set(t, x)
        backend.graph_compute(ctx.graph())
        return backend.tensor_get(y).astype(np.float64).reshape(c.ns, c.nq, c.nh, c.D)
    finally:
        ctx.free()


@pytest.mark.parametrize("name", list(CASES))
def test_flash_attn_mixed_cache_types(pkg, be, request, name):
    from oracle.ref_backend import ref_available
    kt, vt, kind = CASES[name][0], CASES[name][1], CASES[name][8]
    c, own = _case(name), name != "same_type_q8_0"
    want = fn.reference(_attn_f64, c)
    got = {}
    for mode in (-1, 0):
        be.set_option("fattn_qx", mode)
        try:
            n0 = (be.get_stat("fattn_qx_launches"), be.get_stat("fattn_q_launches"))
            got[mode] = _run(pkg, be, c, kt, vt, kind == "view")
            counts = (be.get_stat("fattn_qx_launches") - n0[0], be.get_stat("fattn_q_launches") - n0[1])
        finally:
            be.set_option("fattn_qx", -1)
        assert counts == ((1 if mode else 0, 0) if own else (0, 1)), (name, mode, counts)
    ref = _run(pkg, request.getfixturevalue("ref_be"), c, kt, vt, kind == "view", False) if ref_available() else None
    for mode, out in got.items():
        assert np.isfinite(out).all(), (name, mode)
        e, at, en = fn.check_rows(out, want, c.needles)
        print(f"{name} fattn_qx {mode}: worst row NMSE vs f64 {e:.3e} at (s, t, h) = {at}, worst needle row {en:.3e}")
        assert e < fn.BAR, (name, mode, e, at)
    e_any, e_ref = nmse(got[-1], got[0]), nmse(got[-1], ref) if ref is not None else None
    print(f"{name}: default route vs k_fattn_any NMSE {e_any:.3e}, vs the reference backend {e_ref if e_ref is None else format(e_ref, '.3e')}")
    assert e_any < 1e-9, (name, e_any)
    assert e_ref is None or e_ref < (5e-4 if vt == "f16" else 1e-9), (name, e_ref)


@pytest.mark.parametrize("n", [64, 160])
@pytest.mark.parametrize("itype", ["i64", "i32"])
@pytest.mark.parametrize("tname", ["q4_1", "q5_0", "q5_1"])
def test_set_rows_q4_1_q5_0_q5_1_bytes_equal_reference_backend(pkg, be, ref_be, tname, itype, n):
    """one row of n elements -- its first block all zeros, its second with a negative maximum -- scattered into row 5 of a 9-row table: quantize_row_q4_1_ref /
    q5_0_ref / q5_1_ref, the CPU backend's from_float of these types"""
    x = np.random.default_rng(n).standard_normal((1, n)).astype(np.float32)
    x[0, :32] = 0.0
    x[0, 32:64] = -np.abs(x[0, 32:64]) - 0.25
    res = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        try:
            tab = c.new_tensor(TYPES[tname], n, 9); src = c.new_tensor(pkg.GGML_TYPE_F32, n, 1)
            ix = c.new_tensor(pkg.GGML_TYPE_I64 if itype == "i64" else pkg.GGML_TYPE_I32, 1)
            out = c.set_rows(tab, src, ix)
            c.alloc()
            assert backend is ref_be or backend.supports_op(out), tname
            backend.tensor_set(tab, np.full(tab.nbytes(), 0x5a, np.uint8))
            backend.tensor_set(src, x); backend.tensor_set(ix, np.array([5], np.int64 if itype == "i64" else np.int32))
            backend.graph_compute(c.graph())
            res.append(np.asarray(backend.tensor_get(out)).copy().view(np.uint8))
        finally:
            c.free()
    assert np.array_equal(res[0], res[1]), (tname, itype, n, np.flatnonzero(res[0] != res[1])[:8])
