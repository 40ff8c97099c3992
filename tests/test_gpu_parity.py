"""GPU parity tests (-m gpu): every case drives libggml-mi355x.so through the ggml backend C-ABI
(buffer_type.alloc_buffer / buffer.set_tensor / backend.graph_compute / buffer.get_tensor) and compares with
  (1) the committed golden vectors produced by the real reference (tests/golden),
  (2) the C oracle (oracle/liboracle.so) on seeded inputs,
  (3) the real reference CPU backend (oracle/_ref) on the same graph when it travelled with the snapshot.
Tolerances: bit-exact for integer / byte / index work (de-quantisation, activation quantisation, KV store, row
gather); the reference's own NMSE bars otherwise (1e-7 default, 5e-4 MUL_MAT / FLASH_ATTN_EXT,
reference tests/test-backend-ops.cpp:996,3300,5085); F16 logits within 1e-3.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import nmse
from oracle import oracle_py as orc

pytestmark = pytest.mark.gpu

TYPES = {"q4_K": 12, "q6_K": 14, "q8_0": 8, "f16": 1, "f32": 0}


def run_graph(be, ctx, outs, feeds):
    ctx.alloc()
    for t, v in feeds:
        be.tensor_set(t, v)
    be.graph_compute(ctx.graph())
    res = [be.tensor_get(o).copy() for o in outs]
    ctx.free()
    return res


# ------------------------------------------------------------------------------------------------ integer stages: bit-exact
@pytest.mark.parametrize("name", ["q4_K", "q6_K", "q8_0"])
def test_dequant_bit_exact_via_get_rows(pkg, be, golden, name):
    """GET_ROWS on a quantised table is dequantize_row_*: must equal the reference bit for bit."""
    g = golden["quant"]
    ty = TYPES[name]
    K = 4096
    c = pkg.Context(be)
    tab = c.new_tensor(ty, K, 3)
    idx = c.new_tensor(pkg.GGML_TYPE_I32, 3)
    out = c.get_rows(tab, idx)
    blocks = g[f"{name}_blocks"]
    (got,) = run_graph(be, c, [out], [(tab, blocks), (idx, np.array([2, 0, 1], np.int32))])
    want = g[f"{name}_deq"].reshape(3, K)[[2, 0, 1]]
    assert np.array_equal(got.reshape(3, K).view(np.uint32), want.view(np.uint32))


def dev_quantize(be, kind, x):
    x = np.ascontiguousarray(x, np.float32)
    rows, K = x.shape
    img = (K + K // 8 + K // 64 + 15) // 16 * 16 if kind == 0 else (K + K // 32 * 4 + 15) // 16 * 16
    out = np.zeros((rows, img), np.uint8)
    n = be.lib.mi355x_debug_quantize(be.be, kind, x.ctypes.data, K, rows, out.ctypes.data)
    assert n == img
    return out


def test_activation_quant_q8_K_bit_exact(be, golden):
    g = golden["quant"]
    rng = np.random.default_rng(1)
    rows = [g["y"][:4096], g["y"][4096:8192], np.concatenate([g["edge"], g["edge"], g["edge"], g["edge"]]),
            (rng.standard_normal(4096) * rng.choice([1e-3, 1.0, 1e3], 4096)).astype(np.float32), np.zeros(4096, np.float32)]
    x = np.stack(rows)
    got = dev_quantize(be, 0, x)
    for r in range(x.shape[0]):
        assert np.array_equal(got[r], orc.q8k_image(x[r])), r
    # and against the reference's own bytes for the golden signal
    blocks = g["y_q8_K"].reshape(-1, 292)[:16]
    assert np.array_equal(got[0][:4096], blocks[:, 4:260].reshape(-1))
    assert np.array_equal(got[0][4096:4096 + 512], blocks[:, 260:292].reshape(-1))
    assert np.array_equal(got[0][4608:4608 + 64], blocks[:, 0:4].reshape(-1))


def test_activation_quant_q8_0_bit_exact(be, golden):
    g = golden["quant"]
    x = np.stack([g["y"][:4096], g["y"][8192:12288], np.zeros(4096, np.float32)])
    got = dev_quantize(be, 1, x)
    for r in range(3):
        ref = orc.quantize_q8_0(x[r]).reshape(-1, 34)
        assert np.array_equal(got[r][:4096], ref[:, 2:].reshape(-1))
        d = ref[:, :2].copy().view(np.float16).astype(np.float32).reshape(-1)
        assert np.array_equal(got[r][4096:4096 + 512].view(np.float32), d)


def test_set_rows_f16_bit_exact(pkg, be, golden):
    g = golden["ops"]
    c = pkg.Context(be)
    tab = c.new_tensor(pkg.GGML_TYPE_F16, 1024, 16)
    src = c.new_tensor(pkg.GGML_TYPE_F32, 1024, 3)
    idx = c.new_tensor(pkg.GGML_TYPE_I64, 3)
    y = c.set_rows(tab, src, idx)
    (got,) = run_graph(be, c, [y], [(tab, np.zeros((16, 1024), np.float16)), (src, g["setrows_src"]), (idx, g["setrows_idx"])])
    assert np.array_equal(got.view(np.uint16).reshape(16, 1024), g["setrows_tab"])


# ------------------------------------------------------------------------------------------------ float stages
def test_rms_norm_mul_golden(pkg, be, golden):
    g = golden["ops"]
    for tag, n, rows in (("rms4096", 4096, 3), ("rms128", 128, 40)):
        for fusion in (1, 0):
            be.set_option("fusion", fusion)
            c = pkg.Context(be)
            x = c.new_tensor(pkg.GGML_TYPE_F32, n, rows)
            w = c.new_tensor(pkg.GGML_TYPE_F32, n)
            y = c.mul(c.rms_norm(x, 1e-6), w)
            (got,) = run_graph(be, c, [y], [(x, g[f"{tag}_x"]), (w, g[f"{tag}_w"])])
            assert nmse(got, g[f"{tag}_y"]) < 1e-12, (tag, fusion)
            # double-precision sum of squares like the reference: rows agree to the last ulp or two
            assert np.abs(got.reshape(rows, n) - g[f"{tag}_y"]).max() <= 2e-6 * np.abs(g[f"{tag}_y"]).max()
    be.set_option("fusion", 1)


@pytest.mark.parametrize("tag,mode,base", [("rope_neox", 2, 1e6), ("rope_norm", 0, 1e4)])
def test_rope_golden(pkg, be, golden, tag, mode, base):
    g = golden["ops"]
    c = pkg.Context(be)
    x = c.new_tensor(pkg.GGML_TYPE_F32, 128, 8, 3)
    p = c.new_tensor(pkg.GGML_TYPE_I32, 3)
    y = c.rope_ext(x, p, None, 128, mode, 40960, base, 1.0, 0.0, 1.0, 32.0, 1.0)
    (got,) = run_graph(be, c, [y], [(x, g[f"{tag}_x"]), (p, g[f"{tag}_pos"])])
    assert nmse(got, g[f"{tag}_y"]) < 1e-7                   # reference bar; theta itself is bit-identical by construction
    assert np.abs(got.reshape(3, 8, 128) - g[f"{tag}_y"]).max() < 2e-5


def test_soft_max_and_swiglu_golden(pkg, be, golden):
    g = golden["ops"]
    c = pkg.Context(be)
    x = c.new_tensor(pkg.GGML_TYPE_F32, 256, 4, 8)
    m = c.new_tensor(pkg.GGML_TYPE_F16, 256, 64)
    y = c.soft_max_ext(x, m, 0.0883883, 0.0)
    (got,) = run_graph(be, c, [y], [(x, g["softmax_x"]), (m, g["softmax_mask"])])
    assert nmse(got, g["softmax_y"]) < 1e-7
    c = pkg.Context(be)
    a = c.new_tensor(pkg.GGML_TYPE_F32, 1024, 2)
    b = c.new_tensor(pkg.GGML_TYPE_F32, 1024, 2)
    y = c.swiglu_split(a, b)
    (got,) = run_graph(be, c, [y], [(a, g["swiglu_a"]), (b, g["swiglu_b"])])
    assert nmse(got, g["swiglu_y"]) < 1e-7


@pytest.mark.parametrize("nkv", [256, 2048])
def test_flash_attn_golden(pkg, be, golden, nkv):
    g = golden["ops"]
    c = pkg.Context(be)
    q = c.new_tensor(pkg.GGML_TYPE_F32, 128, 2, 8)
    k = c.new_tensor(pkg.GGML_TYPE_F16, 128, nkv, 2)
    v = c.new_tensor(pkg.GGML_TYPE_F16, 128, nkv, 2)
    m = c.new_tensor(pkg.GGML_TYPE_F16, nkv, 64)
    y = c.flash_attn_ext(q, k, v, m, 1.0 / np.sqrt(128.0))
    (got,) = run_graph(be, c, [y], [(q, g[f"fa{nkv}_q"]), (k, g[f"fa{nkv}_k"]), (v, g[f"fa{nkv}_v"]), (m, g[f"fa{nkv}_mask"])])
    assert nmse(got, g[f"fa{nkv}_y"]) < 5e-4


def _attn_f64(q, k, v, mask, scale, softcap=0.0, sinks=None, max_bias=0.0):
    """ggml_compute_forward_flash_attn_ext_f16 restated in float64 (ops.cpp:7912-8148): q [ns, nh, nq, D] (rounded to f16),
    k/v [ns, nhkv, nkv, D], mask [nq_pad, nkv] f16 or None -> [ns, nq, nh, D]"""
    ns, nh, nq, D = q.shape
    gq = nh // k.shape[1]
    out = np.zeros((ns, nq, nh, D))
    qh = q.astype(np.float16).astype(np.float64)
    for s in range(ns):
        for h in range(nh):
            kk = k[s, h // gq].astype(np.float64); vv = v[s, h // gq].astype(np.float64)
            sc = qh[s, h] @ kk.T * (scale / softcap if softcap else scale)
            if softcap:
                sc = softcap * np.tanh(sc)
            if mask is not None:
                slope = 1.0
                if max_bias > 0:                             # ALiBi head slopes (ops.cpp:7990-7996, 8008)
                    n2 = 2 ** int(np.floor(np.log2(nh)))
                    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
                    slope = m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1)
                sc = sc + slope * mask[:nq].astype(np.float64)
            mx = sc.max(axis=1, keepdims=True)
            if sinks is not None:
                mx = np.maximum(mx, sinks[h])
            mx = np.where(np.isfinite(mx), mx, 0.0)
            p = np.exp(sc - mx)
            den = p.sum(axis=1, keepdims=True) + (np.exp(sinks[h] - mx) if sinks is not None else 0.0)
            out[s, :, h, :] = (p @ vv) / np.where(den == 0, 1.0, den)
    return out


@pytest.mark.parametrize("D,nq,nh,nhkv,nkv,ns,kind", [
    (128, 35, 4, 2, 113, 1, "causal"), (128, 128, 8, 2, 512, 2, "causal"), (64, 70, 4, 4, 96, 1, "none"),
    (128, 512, 8, 2, 512, 1, "causal"), (128, 33, 4, 1, 256, 1, "padded"), (64, 32, 2, 2, 64, 3, "sinks"), (128, 40, 4, 4, 160, 1, "softcap")])
def test_flash_attn_prefill_mfma(pkg, be, D, nq, nh, nhkv, nkv, ns, kind):
    """batches of query rows take the matrix-core kernel (fattn_mma.hip); bar = the reference's FLASH_ATTN_EXT NMSE 5e-4"""
    rng = np.random.default_rng(D + nq + nkv)
    qv = rng.standard_normal((ns, nh, nq, D)).astype(np.float32)
    kv = rng.standard_normal((ns, nhkv, nkv, D)).astype(np.float16)
    vv = rng.standard_normal((ns, nhkv, nkv, D)).astype(np.float16)
    nq_pad = (nq + 63) // 64 * 64
    mask = None
    if kind != "none":
        mask = np.zeros((nq_pad, nkv), np.float16)
        off = nkv - nq if kind != "padded" else nkv // 2 - nq        # "padded": the second half of the KV view is unused cells
        for i in range(nq_pad):
            mask[i, max(0, min(nkv, off + min(i, nq - 1) + 1)):] = -np.inf
    sinks = rng.standard_normal(nh).astype(np.float32) if kind == "sinks" else None
    softcap = 7.0 if kind == "softcap" else 0.0
    c = pkg.Context(be)
    q = c.new_tensor(pkg.GGML_TYPE_F32, D, nq, nh, ns)
    k = c.new_tensor(pkg.GGML_TYPE_F16, D, nkv, nhkv, ns)
    v = c.new_tensor(pkg.GGML_TYPE_F16, D, nkv, nhkv, ns)
    feeds = [(q, qv), (k, kv), (v, vv)]
    m = sk = None
    if mask is not None:
        m = c.new_tensor(pkg.GGML_TYPE_F16, nkv, nq_pad)
        feeds.append((m, mask))
    if sinks is not None:
        sk = c.new_tensor(pkg.GGML_TYPE_F32, nh)
        feeds.append((sk, sinks))
    scale = 1.0 / np.sqrt(D)
    y = c.flash_attn_ext(q, k, v, m, scale, 0.0, softcap, sk)
    (got,) = run_graph(be, c, [y], feeds)
    want = _attn_f64(qv, kv, vv, mask, scale, softcap, sinks)
    assert np.isfinite(got).all()
    assert nmse(got.reshape(want.shape), want) < 5e-4


@pytest.mark.parametrize("gqa", [1, 0])
@pytest.mark.parametrize("D,nq,nh,nhkv,nkv,ns,kind", [
    (128, 1, 32, 8, 4096, 1, "depth"), (128, 8, 32, 8, 3000, 1, "seqs"), (64, 4, 8, 1, 1500, 2, "none"), (128, 1, 4, 4, 1024, 1, "sinks"),
    (128, 2, 16, 4, 5000, 1, "softcap"), (128, 3, 8, 1, 2048, 1, "depth"), (64, 1, 12, 2, 33000, 1, "depth"),
    (128, 1, 32, 8, 256, 1, "depth"), (128, 1, 32, 8, 77, 1, "depth"), (64, 8, 64, 8, 512, 1, "seqs"), (128, 3, 32, 2, 300, 2, "none"),
    (64, 5, 5, 5, 40, 1, "sinks"), (128, 7, 4, 4, 1, 1, "none"), (128, 2, 8, 2, 640, 1, "alibi"),
    (128, 16, 32, 8, 1100, 1, "seqs"), (128, 32, 8, 2, 700, 1, "seqs"), (64, 20, 8, 8, 96, 2, "depth")])
def test_flash_attn_decode_mfma(pkg, be, D, nq, nh, nhkv, nkv, ns, kind, gqa):
    """a few query tokens: the (token, head) pairs of a KV head form 32-column matrix-core tiles (k_fattn_gqa); shallow caches are
    finished by the workgroup itself, deep ones are cut into KV slices merged by a second pass (k_fattn_merge).  gqa=0 sends the same
    shapes through the streaming kernel (option fattn_gqa).  bar = the reference's FLASH_ATTN_EXT NMSE 5e-4"""
    be.set_option("fattn_gqa", gqa)
    try:
        _decode_attn_case(pkg, be, D, nq, nh, nhkv, nkv, ns, kind)
    finally:
        be.set_option("fattn_gqa", 1)


def _decode_attn_case(pkg, be, D, nq, nh, nhkv, nkv, ns, kind):
    rng = np.random.default_rng(D + nq + nkv)
    qv = rng.standard_normal((ns, nh, nq, D)).astype(np.float32)
    kv = rng.standard_normal((ns, nhkv, nkv, D)).astype(np.float16)
    vv = rng.standard_normal((ns, nhkv, nkv, D)).astype(np.float16)
    mask = None
    if kind != "none":
        mask = np.zeros((64, nkv), np.float16)
        if kind == "seqs":                                   # unified KV cache: token t only sees the cells of its own sequence
            mask[:] = -np.inf
            for t in range(nq):
                mask[t, t::nq] = 0
                mask[t, max(nq, nkv - 200):] = -np.inf
        else:
            for t in range(64):
                mask[t, max(1, nkv - 137) + min(t, nq - 1):] = -np.inf
    sinks = rng.standard_normal(nh).astype(np.float32) if kind == "sinks" else None
    softcap = 7.0 if kind == "softcap" else 0.0
    max_bias = 8.0 if kind == "alibi" else 0.0
    if kind == "alibi":                                       # finite position biases on the live cells
        mask = np.where(np.isinf(mask), mask, -np.abs(np.arange(nkv)[None, :] - (nkv - 137)).astype(np.float16) / 16).astype(np.float16)
    c = pkg.Context(be)
    q = c.new_tensor(pkg.GGML_TYPE_F32, D, nq, nh, ns)
    k = c.new_tensor(pkg.GGML_TYPE_F16, D, nkv, nhkv, ns)
    v = c.new_tensor(pkg.GGML_TYPE_F16, D, nkv, nhkv, ns)
    feeds = [(q, qv), (k, kv), (v, vv)]
    m = sk = None
    if mask is not None:
        m = c.new_tensor(pkg.GGML_TYPE_F16, nkv, 64)
        feeds.append((m, mask))
    if sinks is not None:
        sk = c.new_tensor(pkg.GGML_TYPE_F32, nh)
        feeds.append((sk, sinks))
    scale = 1.0 / np.sqrt(D)
    y = c.flash_attn_ext(q, k, v, m, scale, max_bias, softcap, sk)
    (got,) = run_graph(be, c, [y], feeds)
    want = _attn_f64(qv, kv, vv, mask, scale, softcap, sinks, max_bias)
    assert np.isfinite(got).all()
    assert nmse(got.reshape(want.shape), want) < 5e-4


@pytest.mark.parametrize("name", ["q4_K", "q6_K", "q8_0", "f16"])
def test_mul_mat_golden(pkg, be, golden, name):
    g = golden["ops"]
    for (M, K, N) in ((16, 256, 1), (64, 1024, 3)):
        tag = f"mm_{name}_{M}x{K}x{N}"
        c = pkg.Context(be)
        w = c.new_tensor(TYPES[name], K, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
        y = c.mul_mat(w, x)
        (got,) = run_graph(be, c, [y], [(w, g[tag + "_w"]), (x, g[tag + "_x"])])
        assert nmse(got, g[tag + "_y"]) < 1e-9, tag           # far inside the reference's 5e-4: same integer sums, f32 re-association only


# ------------------------------------------------------------------------------------------------ seeded vs the C oracle, ragged / edge shapes
@pytest.mark.parametrize("name", ["q4_K", "q6_K", "q8_0", "f16", "f32"])
@pytest.mark.parametrize("M,K,N", [(1, 256, 1), (7, 512, 2), (33, 2304, 5), (130, 4096, 8), (257, 768, 9), (4096, 4096, 1), (1024, 12288, 1)])
def test_mul_mat_vs_oracle_shapes(pkg, be, name, M, K, N):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(M * 131 + K + N)
    ty = TYPES[name]
    wv = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    xv = (rng.standard_normal((N, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    c = pkg.Context(be)
    w = c.new_tensor(ty, K, M)
    x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
    y = c.mul_mat(w, x)
    (got,) = run_graph(be, c, [y], [(w, wv), (x, xv)])
    want = orc.mul_mat(ty, wv.view(np.uint8).reshape(M, -1), xv)
    # <= 8 columns: mat-vec path, the oracle's own integer arithmetic; more: MFMA GEMM on f16 operands (reference MUL_MAT bar)
    bar = 1e-9 if (N <= 8 or name in ("f16", "f32", "q4_K", "q6_K")) else 5e-4       # (K-quants at 9..64 columns: mmq.hip, integer sums)
    assert nmse(got, want) < bar, (name, M, K, N)


@pytest.mark.parametrize("name", ["q4_K", "q6_K"])
@pytest.mark.parametrize("M,K,N", [(64, 256, 9), (257, 768, 16), (130, 1024, 33), (33, 2304, 31), (4096, 4096, 12), (1024, 12288, 64), (96, 512, 40),
                                   (130, 4096, 6), (31, 256, 8)])
def test_mul_mat_mmq_vs_oracle(pkg, be, name, M, K, N):
    """6 .. 64 columns against K-quant weights: the int8 matrix-core kernel (mmq.hip) on Q8_K activation images -- the oracle's own
    integer sums (ggml_vec_dot_q4_K_q8_K / _q6_K_q8_K), f32 re-association across blocks only, so the mat-vec bar applies"""
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(M * 17 + K + N)
    ty = TYPES[name]
    wv = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    xv = (rng.standard_normal((N, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    xv[N // 2, : K // 2] = 0.0                                 # (a zero half row: an all-zero Q8_K block, d = 0)
    c = pkg.Context(be)
    w = c.new_tensor(ty, K, M)
    x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
    y = c.mul_mat(w, x)
    (got,) = run_graph(be, c, [y], [(w, wv), (x, xv)])
    want = orc.mul_mat(ty, wv.view(np.uint8).reshape(M, -1), xv)
    assert nmse(got, want) < 1e-9, (name, M, K, N)


@pytest.mark.parametrize("name", ["q4_K", "q6_K", "q8_0", "f16"])
@pytest.mark.parametrize("M,K,N", [(64, 256, 9), (130, 1024, 33), (257, 4096, 128), (1000, 2304, 200)])
def test_mul_mat_gemm_path_vs_oracle(pkg, be, name, M, K, N):
    """batches > 8 columns run on the MFMA GEMM (f16 operands, f32 accumulate; quantised weights de-quantised to f16).
    Against the oracle's exact-integer arithmetic the reference's own MUL_MAT bar applies (NMSE 5e-4); for F16 weights the two
    compute the same products and the error is f32 re-association only."""
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(M + K + N)
    ty = TYPES[name]
    wv = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    c = pkg.Context(be)
    w = c.new_tensor(ty, K, M)
    x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
    y = c.mul_mat(w, x)
    (got,) = run_graph(be, c, [y], [(w, wv), (x, xv)])
    want = orc.mul_mat(ty, wv.view(np.uint8).reshape(M, -1), xv)
    err = nmse(got, want)
    assert err < (1e-9 if name == "f16" else 5e-4), (name, M, K, N, err)


@pytest.mark.parametrize("name", ["q4_K", "q6_K", "q8_0"])
def test_resident_f16_weight_image(pkg, be, name):
    """Quantised tensors in a WEIGHTS buffer get a resident F16 image on their first GEMM (shadow.hpp); rewriting the tensor
    through the buffer interface drops the image, so the next run sees the new weights -- also through hipGraph replays."""
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(99)
    ty, M, K, N = TYPES[name], 192, 1024, 96          # (more columns than the int8 mmq path takes: the F16 GEMM)
    w1 = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    w2 = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    wctx = pkg.Context(be)
    w = wctx.new_tensor(ty, K, M)
    wctx.alloc(usage=pkg.GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
    c = pkg.Context(be)
    wl = c._new(w.type, w.ne, view_src=w, view_offs=0)
    for i in range(4):
        wl.t.nb[i] = w.t.nb[i]
    x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
    # a chain long enough (>= 8 real nodes) to be captured into a hipGraph on its second submission
    y = c.mul_mat(wl, x)
    z = y
    for _ in range(8):
        z = c.scale(z, 1.0)
    c.alloc()
    gr = c.graph()
    be.tensor_set(x, xv)
    n0 = be.get_stat("shadow_tensors")
    for wv in (w1, w2):
        be.tensor_set(w, wv)
        want = orc.mul_mat(ty, wv.view(np.uint8).reshape(M, -1), xv)
        for rep in range(3):                                       # eager, capture, replay
            be.graph_compute(gr)
            assert nmse(be.tensor_get(z), want) < 5e-4, (name, rep)
        assert be.get_stat("shadow_tensors") == n0 + 1
    c.free()
    wctx.free()
    assert be.get_stat("shadow_tensors") == n0                     # freeing the weight buffer drops its images


def test_mul_mat_zero_and_empty(pkg, be):
    """all-zero activations (Q8_K amax == 0 branch) and a zero-column batch"""
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(0)
    wv = qwen3.random_blocks(rng, 12, 64, 1024)
    c = pkg.Context(be)
    w = c.new_tensor(12, 1024, 64)
    x = c.new_tensor(pkg.GGML_TYPE_F32, 1024, 2)
    y = c.mul_mat(w, x)
    xv = np.zeros((2, 1024), np.float32)
    xv[1, 300:500] = 1.0
    (got,) = run_graph(be, c, [y], [(w, wv), (x, xv)])
    got = got.reshape(2, 64)
    assert np.all(got[0] == 0) and np.isfinite(got).all()
    assert nmse(got[1], orc.mul_mat(12, wv, xv)[1]) < 1e-9


# ------------------------------------------------------------------------------------------------ properties at BASELINE.json's full sizes
@pytest.mark.parametrize("name,M,K", [("q4_K", 12288, 4096), ("q4_K", 4096, 12288), ("q6_K", 4096, 12288), ("q6_K", 151936, 4096)])
def test_full_size_properties(pkg, be, name, M, K):
    """Size-independent checks on the real Qwen3-8B matrix shapes (too big for the scalar oracle in seconds):
    (a) a sampled subset of rows equals the oracle; (b) the op is linear in the weights' row index: permuting rows of W
    permutes the output identically; (c) column independence: a 2-column batch equals the two 1-column runs bit for bit."""
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(7)
    ty = TYPES[name]
    base = qwen3.random_blocks(rng, ty, 1024, K, std=0.05)
    perm = rng.permutation(M)
    wv = base[np.arange(M) % 1024]
    xv = rng.standard_normal((2, K)).astype(np.float32)

    def run(wmat, xmat):
        c = pkg.Context(be)
        w = c.new_tensor(ty, K, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, xmat.shape[0])
        y = c.mul_mat(w, x)
        (r,) = run_graph(be, c, [y], [(w, wmat), (x, xmat)])
        return r.reshape(xmat.shape[0], M)

    y2 = run(wv, xv)
    rows = rng.choice(M, 64, replace=False)
    want = orc.mul_mat(ty, wv[rows], xv)
    assert nmse(y2[:, rows], want) < 1e-9
    # one column runs on the batch-1 decode kernels (mmv1.hip), two on the multi-column family (mmvk.hip): the integer sub-block sums are
    # the same, the order of the f32 additions across super-blocks is not -- bit-equality holds inside a family
    be.set_option("mv1", 0)
    try:
        y0, y1 = run(wv, xv[:1]), run(wv, xv[1:])
        assert np.array_equal(y2[0], y0[0]) and np.array_equal(y2[1], y1[0])
    finally:
        be.set_option("mv1", 1)
    y0 = run(wv, xv[:1])
    assert nmse(y0[:, rows], want[:1]) < 1e-9 and nmse(y0[0], y2[0]) < 1e-11
    yp = run(wv[perm], xv[:1])
    assert np.array_equal(yp[0], y0[0][perm])
    assert np.array_equal(y0[0][:1024], y0[0][1024:2048])      # identical weight rows give identical outputs wherever they sit


# ------------------------------------------------------------------------------------------------ whole graphs
def test_tiny_model_tokens_match_reference(pkg, be, golden):
    """Greedy token ids over 32 decode steps on the 2-layer Q4_K_M fixture are identical to the reference CPU backend's,
    final logits within the F16-logit tolerance of the north star (1e-3)."""
    from test_host_mirror import run_tiny
    tm = golden["tiny_model"]
    for fusion, graphs in ((1, 1), (0, 0)):
        be.set_option("fusion", fusion)
        be.set_option("graphs", graphs)
        toks, l = run_tiny(pkg, be, tm, 32)
        assert toks == list(tm["tokens"]), (fusion, graphs)
        # quantised path: the reference's own MUL_MAT / FLASH_ATTN_EXT bar (the CPU accumulates V in f16, we in f32)
        assert nmse(l, tm["final_logits"]) < 5e-4
    be.set_option("fusion", 1)
    be.set_option("graphs", 1)


def test_tiny_model_live_vs_reference_backend(pkg, be, ref_be, golden):
    """Same graphs on both backends right now (FA on and off, multi-token prefill ubatch then decode)."""
    from llama_cpp_omni_amd import qwen3
    from test_host_mirror import tiny_weights
    tm = golden["tiny_model"]
    cfg = qwen3.TINY
    rng = np.random.default_rng(5)
    embd = rng.standard_normal((6, cfg["n_embd"])).astype(np.float32)
    for fa in (True, False):
        outs = []
        for backend in (be, ref_be):
            mdl = qwen3.Model(backend, cfg, qwen3.q4_k_m_types(cfg), n_ctx=256, flash_attn=fa, weights=tiny_weights(tm))
            g, I, logits = mdl.build(5, 256 if fa else 32)             # prefill ubatch of 5 tokens
            mdl.set_inputs(I, embd[:5], 0, 256 if fa else 32)
            backend.graph_compute(g.graph())
            l5 = backend.tensor_get(logits).copy()
            g1, I1, logits1 = mdl.build(1, 256 if fa else 32)          # then one decode step at position 5
            mdl.set_inputs(I1, embd[5:6], 5, 256 if fa else 32)
            backend.graph_compute(g1.graph())
            outs.append((l5, backend.tensor_get(logits1).copy()))
            g.free(); g1.free(); mdl.wctx.free()
        for a, b in zip(outs[0], outs[1]):
            assert nmse(a, b) < 5e-4, fa
            assert np.array_equal(np.argmax(a.reshape(-1, cfg["n_vocab"]), 1), np.argmax(b.reshape(-1, cfg["n_vocab"]), 1))


@pytest.mark.parametrize("wtype", ["q4_k_m", "f16"])
def test_prefill_ubatch_vs_reference_backend(pkg, be, ref_be, wtype):
    """A 2-layer model wide enough (n_embd 2048, n_ff 4096) for every prefill mechanism to engage at a 96-token ubatch: grouped GEMM
    launches, resident F16 weight images, split-K with the reduction folded into the next norm, f16 emission from norm / GLU /
    attention, the MFMA flash-attention with its mask tile map -- against the reference CPU backend on the same graph."""
    from llama_cpp_omni_amd import qwen3
    cfg = dict(n_embd=2048, n_layer=2, n_head=16, n_head_kv=4, head_dim=128, n_ff=4096, n_vocab=1024, rms_eps=1e-6, rope_base=1e6, n_ctx_orig=4096)
    types = qwen3.q4_k_m_types(cfg) if wtype == "q4_k_m" else qwen3.uniform_types(cfg, pkg.GGML_TYPE_F16)
    rng = np.random.default_rng(21)
    T = 96
    embd = rng.standard_normal((T + 1, cfg["n_embd"])).astype(np.float32)
    outs = []
    for backend in (be, ref_be):
        mdl = qwen3.Model(backend, cfg, types, n_ctx=256, seed=9, flash_attn=True)
        g, I, logits = mdl.build(T, 256, n_outputs=T)
        mdl.set_inputs(I, embd[:T], 0, 256)
        if "out_ids" in I:
            backend.tensor_set(I["out_ids"], np.arange(T, dtype=np.int32))
        backend.graph_compute(g.graph())
        lp = backend.tensor_get(logits).copy()
        g1, I1, logits1 = mdl.build(1, 256)                            # one decode step on top of the prefilled cache
        mdl.set_inputs(I1, embd[T:T + 1], T, 256)
        backend.graph_compute(g1.graph())
        outs.append((lp, backend.tensor_get(logits1).copy()))
        g.free(); g1.free(); mdl.wctx.free()
    # F16 weights: both sides multiply the same f16 operands and accumulate in f32 -> tight.  Quantised weights: the CPU quantises the
    # activations to Q8_K (int8 per 256) before its integer dot, the GEMM path keeps them in f16 (what the reference's GPU backends
    # do too) -- per op that difference is ~1e-5 NMSE (test_mul_mat_gemm_path_vs_oracle, bar 5e-4), end to end over two layers and
    # the lm-head it compounds to ~5e-4, almost all of it the CPU's own activation-quantisation noise
    # Per op the quantised path is proven at the pp512 shapes in test_round2_gpu.py::test_prefill_512_tokens_per_op_vs_oracle_and_exact (NMSE
    # vs the oracle < 5e-5, and closer to the exact product than the oracle is).  End to end the bar cannot be the per-op bar: every
    # following mat-mul re-quantises its input to Q8_K on the CPU side, and test_oracle.py::test_reference_decorrelates_under_a_1e6_
    # perturbation shows the reference itself moving by ~1e-3 NMSE under a 1e-6 input perturbation.
    bar = 1e-5 if wtype == "f16" else 2e-3
    for a, b in zip(outs[0], outs[1]):
        assert np.isfinite(a).all()
        assert nmse(a, b) < bar, (wtype, nmse(a, b))
    # arg-max: identical wherever the reference's own top logits are separated by more than the noise between the two runs
    lg, lr = outs[0][0].reshape(T, -1), outs[1][0].reshape(T, -1)
    same = 0
    for t in range(T):
        ig, ir = int(np.argmax(lg[t])), int(np.argmax(lr[t]))
        if ig == ir:
            same += 1
        else:
            rms = float(np.sqrt(np.mean((lg[t] - lr[t]) ** 2)))
            assert lr[t][ig] >= lr[t].max() - 4.0 * rms, (wtype, t)
    assert same >= (0.99 if wtype == "f16" else 0.9) * T, same


@pytest.mark.parametrize("fa", [True, False])
@pytest.mark.parametrize("n_kv,T,steps", [(768, 300, 3), (2048, 1500, 2), (5120, 4200, 2), (9216, 8300, 1)])
def test_decode_on_a_deep_cache_vs_reference_backend(pkg, be, ref_be, n_kv, T, steps, fa):
    """Decode steps on top of a cache of several hundred / thousand rows.  Up to 8192 rows the attention node is the one-token kernel cut
    into 256-row slices (fattn_one.hip: 3, 8 and 20 slices here -- the 16- and the 32-wide fold), the q/k/v pre-stage inside every slice
    (only the slice that owns the new cache row stores it) and the last arriver of a head folding the partial rows inside the launch;
    beyond that (9216 rows) the matrix-core kernel with KV slices (k_fattn_gqa + k_fattn_merge).  fa = False: the reference's soft-max graph on
    the transposed V cache (llama-bench's default) -- k_attn_one_sm with the same slices and in-launch fold up to 8192 rows, the separate
    launches beyond.  Logits against the reference CPU backend on the same graphs."""
    from llama_cpp_omni_amd import qwen3
    cfg = dict(n_embd=1024, n_layer=2, n_head=8, n_head_kv=2, head_dim=128, n_ff=2048, n_vocab=512, rms_eps=1e-6, rope_base=1e6, n_ctx_orig=4096)
    types = qwen3.q4_k_m_types(cfg)
    rng = np.random.default_rng(n_kv)
    embd = rng.standard_normal((T + steps, cfg["n_embd"])).astype(np.float32)
    outs = []
    for backend in (be, ref_be):
        mdl = qwen3.Model(backend, cfg, types, n_ctx=n_kv, seed=4, flash_attn=fa)
        done = 0
        while done < T:                                                # prefill in ubatches of 512 at growing depth
            n = min(512, T - done)
            g, I, logits = mdl.build(n, n_kv)
            mdl.set_inputs(I, embd[done:done + n], done, n_kv)
            backend.graph_compute(g.graph())
            backend.synchronize()
            g.free()
            done += n
        g1, I1, logits1 = mdl.build(1, n_kv)
        gr = g1.graph()
        ls = []
        for k in range(steps):                                         # (second submission onwards: hipGraph replay on the device backend)
            mdl.set_inputs(I1, embd[T + k:T + k + 1], T + k, n_kv)
            backend.graph_compute(gr)
            ls.append(backend.tensor_get(logits1).copy())
        outs.append(np.stack(ls))
        g1.free(); mdl.wctx.free()
    assert np.isfinite(outs[0]).all()
    assert nmse(outs[0], outs[1]) < 2e-3                               # (prefill on f16 operands vs the CPU's Q8_K activations, as test_prefill_ubatch)
    assert np.array_equal(outs[0].argmax(-1), outs[1].argmax(-1))


@pytest.mark.parametrize("fa", [True, False])
def test_tts_shape_decode_on_a_deep_cache_vs_reference_backend(pkg, be, ref_be, fa):
    """The omni TTS decoder's shape (llama architecture: ROPE-only chains, head size 64, Q8_0 weights) decoding on top of 700 cache rows: the
    head-64 instances of the sliced one-token kernels (k_fattn_one<64> / k_attn_one_sm<64>, three slices) against the reference CPU backend."""
    from llama_cpp_omni_amd import qwen3
    cfg = dict(arch="llama", n_embd=768, n_layer=2, n_head=12, n_head_kv=12, head_dim=64, n_ff=3072, n_vocab=1024, rms_eps=1e-5, rope_base=1e4, n_ctx_orig=4096)
    types = qwen3.uniform_types(cfg, pkg.GGML_TYPE_Q8_0)
    rng = np.random.default_rng(64)
    n_kv, T, steps = 768, 700, 3
    embd = rng.standard_normal((T + steps, cfg["n_embd"])).astype(np.float32)
    outs = []
    for backend in (be, ref_be):
        mdl = qwen3.Model(backend, cfg, types, n_ctx=n_kv, seed=6, flash_attn=fa)
        done = 0
        while done < T:
            n = min(512, T - done)
            g, I, logits = mdl.build(n, n_kv)
            mdl.set_inputs(I, embd[done:done + n], done, n_kv)
            backend.graph_compute(g.graph()); backend.synchronize()
            g.free()
            done += n
        g1, I1, logits1 = mdl.build(1, n_kv)
        ls = []
        for k in range(steps):
            mdl.set_inputs(I1, embd[T + k:T + k + 1], T + k, n_kv)
            backend.graph_compute(g1.graph())
            ls.append(backend.tensor_get(logits1).copy())
        outs.append(np.stack(ls))
        g1.free(); mdl.wctx.free()
    assert np.isfinite(outs[0]).all()
    e = nmse(outs[0], outs[1])
    print("TTS shape at depth 700, flash-attention", fa, ": logits NMSE", e)
    assert e < 2e-3, e
    assert np.array_equal(outs[0].argmax(-1), outs[1].argmax(-1))


def test_encoder_block_vs_reference_backend(pkg, be, ref_be):
    """First ops of the omni audio encoder (tools/omni/audition.cpp: conv1d -> GELU -> LayerNorm * w + b -> F16 linear), i.e. IM2COL,
    the F16 x F16 MUL_MAT of ggml_conv_1d, UNARY(GELU), CONT(transpose), NORM, MUL, ADD, MUL_MAT -- against the reference CPU backend."""
    rng = np.random.default_rng(31)
    L, IC, OC, K, F = 96, 16, 32, 3, 64
    xv = rng.standard_normal((1, IC, L)).astype(np.float32)
    kv = (rng.standard_normal((OC, IC, K)) * 0.2).astype(np.float16)
    wv = rng.standard_normal(OC).astype(np.float32); bv = rng.standard_normal(OC).astype(np.float32)
    lv = (rng.standard_normal((F, OC)) * 0.2).astype(np.float16)
    outs = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        x = c.new_tensor(pkg.GGML_TYPE_F32, L, IC, 1)
        kern = c.new_tensor(pkg.GGML_TYPE_F16, K, IC, OC)
        w = c.new_tensor(pkg.GGML_TYPE_F32, OC); b = c.new_tensor(pkg.GGML_TYPE_F32, OC)
        lin = c.new_tensor(pkg.GGML_TYPE_F16, OC, F)
        h = c.conv_1d(kern, x, 1, 1, 1)                                # [OL, OC, 1]
        h = c.unary(h, pkg.UNARY.GELU)
        h = c.cont(c.transpose(c.reshape(h, h.ne[0], h.ne[1])))        # [OC, OL]: features contiguous per frame
        h = c.add(c.mul(c.norm(h, 1e-5), w), b)
        y = c.mul_mat(lin, h)                                          # [F, OL]
        c.alloc()
        for t, v in ((x, xv), (kern, kv), (w, wv), (b, bv), (lin, lv)):
            backend.tensor_set(t, v)
        backend.graph_compute(c.graph())
        outs.append(backend.tensor_get(y).copy())
        c.free()
    assert np.isfinite(outs[0]).all()
    assert nmse(outs[0], outs[1]) < 1e-6


# (type id, block bytes, offsets of the fp16 fields inside a block) of the block formats served through their F16 image
IMAGE_QUANTS = {"q4_0": (2, 18, (0,)), "q4_1": (3, 20, (0, 2)), "q5_0": (6, 22, (0,)), "q5_1": (7, 24, (0, 2)),
                "q2_K": (10, 84, (80, 82)), "q3_K": (11, 110, (108,))}
Q5_K_DESC = (13, 176, (0, 2))


def _random_image_quant_rows(rng, name, M, K):
    """valid random blocks: every quant / scale byte uniform, the fp16 super-scales small positive numbers"""
    _, bs, hoffs = Q5_K_DESC if name == "q5_K" else IMAGE_QUANTS[name]
    nb = K // (32 if bs < 30 else 256)
    raw = rng.integers(0, 256, (M, nb, bs), dtype=np.uint8)
    for o in hoffs:
        raw[:, :, o:o + 2] = rng.uniform(0.002, 0.02, (M, nb, 1)).astype(np.float16).view(np.uint8).reshape(M, nb, 2)
    return raw.reshape(M, -1)


@pytest.mark.parametrize("name", sorted(IMAGE_QUANTS))
@pytest.mark.parametrize("M,K,N", [(48, 512, 1), (130, 1024, 5), (96, 768, 24)])
def test_mul_mat_image_quants_vs_reference_backend(pkg, be, ref_be, name, M, K, N):
    """Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q2_K / Q3_K weights: MUL_MAT on the F16 image of the de-quantised blocks (mat-vec and GEMM
    widths) and GET_ROWS, against the reference CPU backend; bar = the reference's MUL_MAT NMSE 5e-4, GET_ROWS bit-exact."""
    rng = np.random.default_rng(M + K + N)
    ty = IMAGE_QUANTS[name][0]
    wv = _random_image_quant_rows(rng, name, M, K)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    iv = rng.integers(0, M, 7).astype(np.int32)
    outs = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        w = c.new_tensor(ty, K, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
        idx = c.new_tensor(pkg.GGML_TYPE_I32, 7)
        y = c.mul_mat(w, x)
        r = c.get_rows(w, idx)
        c.alloc()
        backend.tensor_set(w, wv); backend.tensor_set(x, xv); backend.tensor_set(idx, iv)
        gr = c.graph()
        backend.graph_compute(gr)
        outs.append((backend.tensor_get(y).copy(), backend.tensor_get(r).copy()))
        c.free()
    assert np.isfinite(outs[0][0]).all()
    assert nmse(outs[0][0], outs[1][0]) < 5e-4, name
    assert np.array_equal(outs[0][1], outs[1][1]), name


@pytest.mark.parametrize("name", ["q4_0", "q5_0"])
@pytest.mark.parametrize("M,K,N", [(48, 512, 1), (130, 1024, 5), (257, 96, 8), (33, 4096, 3), (4096, 4096, 1)])
def test_mul_mat_q4_0_q5_0_integer_path(pkg, be, ref_be, name, M, K, N):
    """Q4_0 / Q5_0 weights up to 8 columns: integer mat-vec on Q8_0 activation images (k_mmv_blocks<q40_form>) -- the integers of
    ggml_vec_dot_q4_0_q8_0 / _q5_0_q8_0, f32 re-association only against the reference CPU backend"""
    rng = np.random.default_rng(M + K + N)
    wv = _random_image_quant_rows(rng, name, M, K)
    xv = (rng.standard_normal((N, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    outs = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        w = c.new_tensor(IMAGE_QUANTS[name][0], K, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
        y = c.mul_mat(w, x)
        c.alloc()
        backend.tensor_set(w, wv); backend.tensor_set(x, xv)
        backend.graph_compute(c.graph())
        outs.append(backend.tensor_get(y).copy())
        c.free()
    assert np.isfinite(outs[0]).all()
    assert nmse(outs[0], outs[1]) < 1e-8, name


@pytest.mark.parametrize("M,K,N", [(48, 512, 1), (130, 1024, 5), (257, 768, 8), (96, 768, 6), (4096, 4096, 1), (64, 2304, 24), (1000, 1024, 40)])
def test_mul_mat_q5_K_vs_reference_backend(pkg, be, ref_be, M, K, N):
    """Q5_K weights take the Q4_K kernels with the fifth bit OR-ed in (dot4 mat-vec up to 5 columns, int8 MFMA from 6): the integer sums
    of ggml_vec_dot_q5_K_q8_K on the same Q8_K activations -- f32 re-association only against the reference CPU backend"""
    rng = np.random.default_rng(M + K + N)
    wv = _random_image_quant_rows(rng, "q5_K", M, K)
    xv = (rng.standard_normal((N, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    outs = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        w = c.new_tensor(13, K, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
        y = c.mul_mat(w, x)
        c.alloc()
        backend.tensor_set(w, wv); backend.tensor_set(x, xv)
        backend.graph_compute(c.graph())
        outs.append(backend.tensor_get(y).copy())
        c.free()
    assert np.isfinite(outs[0]).all()
    assert nmse(outs[0], outs[1]) < 1e-9


@pytest.mark.parametrize("case", ["2d_avg", "2d_max_pad", "2d_f16", "1d_avg5", "1d_max2"])
def test_pool_vs_reference_backend(pkg, be, ref_be, case):
    """POOL_2D / POOL_1D (the omni encoders' pooling: audition.cpp:697 avg k = s = 5 along the token axis; vision.cpp) -- same window
    order and the same division as ggml_compute_forward_pool_2d / _pool_1d_sk_p0, so the bits must match the reference CPU backend."""
    rng = np.random.default_rng(5)
    outs = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        if case.startswith("2d"):
            ty = pkg.GGML_TYPE_F16 if case == "2d_f16" else pkg.GGML_TYPE_F32
            xv = rng.standard_normal((2, 3, 11, 13)).astype(np.float16 if case == "2d_f16" else np.float32)
            x = c.new_tensor(ty, 13, 11, 3, 2)
            y = c.pool_2d(x, 0 if case == "2d_max_pad" else 1, 3, 2, 2, 1, 1 if case == "2d_max_pad" else 0, 1 if case == "2d_max_pad" else 0)
        else:
            xv = rng.standard_normal((1, 2, 24, 40)).astype(np.float32)
            x = c.new_tensor(pkg.GGML_TYPE_F32, 40, 24, 2, 1)
            k = 5 if case == "1d_avg5" else 2
            y = c.pool_1d(x, 1 if case == "1d_avg5" else 0, k, k, 0)
        c.alloc()
        backend.tensor_set(x, xv)
        backend.graph_compute(c.graph())
        outs.append(backend.tensor_get(y).copy())
        c.free()
        rng = np.random.default_rng(5)
    assert outs[0].shape == outs[1].shape and np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])


def test_f16_model_logits_within_1e3(pkg, be, ref_be):
    """north star: F16 logits within 1e-3 of the reference CPU backend (F16 weights, f16-rounded activations, f32 accumulate)."""
    from llama_cpp_omni_amd import qwen3
    cfg = qwen3.TINY
    rng = np.random.default_rng(11)
    embd = rng.standard_normal((4, cfg["n_embd"])).astype(np.float32)
    outs = []
    for backend in (be, ref_be):
        mdl = qwen3.Model(backend, cfg, qwen3.uniform_types(cfg, pkg.GGML_TYPE_F16), n_ctx=256, seed=3, flash_attn=True)
        g, I, logits = mdl.build(1, 256)
        gr = g.graph()
        ls = []
        for step in range(4):
            mdl.set_inputs(I, embd[step:step + 1], step, 256)
            backend.graph_compute(gr)
            ls.append(backend.tensor_get(logits).copy())
        outs.append(np.stack(ls))
        g.free(); mdl.wctx.free()
    assert np.abs(outs[0] - outs[1]).max() < 1e-3 * max(1.0, np.abs(outs[1]).max())
    assert np.array_equal(outs[0].argmax(1), outs[1].argmax(1))


def test_norm_in_kernel_option(pkg, be, golden):
    """opt-in variant of the multi-column family: RMS_NORM + MUL computed inside the consuming mat-vec launches (no stand-alone norm
    kernel) -- same tokens, fewer launches.  (The batch-1 kernels, which always do this and now take every K % 256 == 0, are switched off for
    the comparison and then checked to need fewer launches still.)"""
    from test_host_mirror import run_tiny
    tm = golden["tiny_model"]
    be.set_option("mv1", 0)
    try:
        t0, l0 = run_tiny(pkg, be, tm, 16)
        k0 = be.get_stat("kernels_last_graph")
        be.set_option("norm_in_kernel", 1)
        t1, l1 = run_tiny(pkg, be, tm, 16)
        k1 = be.get_stat("kernels_last_graph")
    finally:
        be.set_option("norm_in_kernel", 0)
        be.set_option("mv1", 1)
    t2, l2 = run_tiny(pkg, be, tm, 16)
    k2 = be.get_stat("kernels_last_graph")
    assert t0 == t1 == t2 == list(tm["tokens"])[:16]
    assert nmse(l1, l0) < 1e-9
    assert nmse(l2, l0) < 5e-4, nmse(l2, l0)                 # (another f32 summation order, re-quantised 16 tokens deep: the golden-logits bar)
    assert k2 <= k1 < k0


def test_graph_replay_is_bit_identical(pkg, be, golden):
    """hipGraph replay of a repeated cgraph gives the same bits as the eager run."""
    from test_host_mirror import run_tiny
    tm = golden["tiny_model"]
    be.set_option("graphs", 0)
    t0, l0 = run_tiny(pkg, be, tm, 8)
    be.set_option("graphs", 1)
    before = be.get_stat("graph_replays")
    t1, l1 = run_tiny(pkg, be, tm, 8)
    assert be.get_stat("graph_replays") > before
    assert t0 == t1 and np.array_equal(l0, l1)
