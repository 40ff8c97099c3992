"""TQ1_0 / TQ2_0 (ternary) weights on the GPU (-m gpu) against the reference CPU backend on the same graph: admission, GET_ROWS (exact) and MUL_MAT on its three paths --
mat-vec forms up to 8 columns, the int8-MFMA kernel on the blocks for 9 .. 64 (both the reference's integers: NMSE <= 1e-8), the F16 image beyond (test_lowbit_gpu.py's 5e-4)."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

TQ1_0, TQ2_0 = 34, 35
BYTES = {TQ1_0: 54, TQ2_0: 66}
TYPES = pytest.mark.parametrize("ty", [TQ1_0, TQ2_0], ids=["tq1_0", "tq2_0"])
CLASSES = ("mmv_tq1", "mmv_tq2", "mmq_tq", "gemm_f16", "dequant_f16", "gemm_any_f16", "gemm_any_f32", "mmq_q4k", "mmq_q6k", "mmq_tile", "mmv_f32", "mmv_f16", "mmv_q4k", "mmv_q6k", "mmv_q80")
STATS = ("mmv_tq1_launches", "mmv_tq2_launches", "mmq_tq_launches")      # CLASSES: the profile class of every launch a dense MUL_MAT can book; STATS: the new kernels' counters


def _weights(ty, M, K):
    from llama_cpp_omni_amd import qwen3
    raw = qwen3.random_blocks(np.random.default_rng(1000 * ty + M + K), ty, M, K)
    qs = raw.reshape(M, K // 256, BYTES[ty])[..., :64]
    assert ty != TQ2_0 or any((((qs >> s) & 3) == 3).any() for s in (0, 2, 4, 6)), "no 2-bit field of 3 (the weight +2) in the fixture"
    return raw


def _run(pkg, backend, make, data):                                  # make(context) -> (leaf tensors, result node); one graph run with `data` in the leaves
    c = pkg.Context(backend)
    leaves, y = make(c)
    c.alloc()
    for t, v in zip(leaves, data):
        backend.tensor_set(t, v)
    backend.graph_compute(c.graph())
    out = backend.tensor_get(y).copy()
    c.free()
    return out


def _mul_mat(pkg, backend, ty, wv, xv, M, K, view=False):           # -> [N, M].  view: the weights a view_2d one block into a parent with rows one block longer (wv: its bytes)
    def make(c):
        w0 = c.new_tensor(ty, K + 256 * view, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, len(xv))
        return (w0, x), c.mul_mat(c.view_2d(w0, K, M, w0.nb[1], BYTES[ty]) if view else w0, x)
    return _run(pkg, backend, make, (wv, xv)).reshape(len(xv), M)


def _gpu_counted(pkg, be, ty, N, *args, image=False):               # the GPU result; exactly the launches of the path that N names were booked, only its counter moved
    name = "mmq_tq" if N > 8 else ("mmv_tq1" if ty == TQ1_0 else "mmv_tq2")
    classes, stats = ({"gemm_f16": 1, "dequant_f16": 1}, {}) if N > 64 or image else ({name: 1}, {name + "_launches": 1})
    before = {k: be.get_stat(k) for k in STATS}
    be.set_option("profile", 1); be.set_option("reset_stats", 1)
    try:
        got = _mul_mat(pkg, be, ty, *args)
        booked = {c: int(be.get_stat("prof_%s_n" % c)) for c in CLASSES}
    finally:
        be.set_option("profile", 0)
    assert {c: n for c, n in booked.items() if n} == classes, booked
    assert {k: int(be.get_stat(k) - before[k]) for k in STATS if be.get_stat(k) != before[k]} == stats
    return got


def _check(got, want, bar):
    assert np.isfinite(want).all() and (want != 0).any(axis=1).all() and np.isfinite(got).all(), "the reference's result is not finite and non-zero"
    errs = [nmse(got, want)] + [nmse(got[c], want[c]) for c in range(want.shape[0])]
    print("nmse all %.2e, worst column %.2e" % (errs[0], max(errs[1:])))
    assert max(errs) <= bar, errs


@TYPES
def test_tq_admission(pkg, be, ty):
    c = pkg.Context(be)
    w = c.new_tensor(ty, 512, 64)
    for N in (1, 9, 65):
        assert be.supports_op(c.mul_mat(w, c.new_tensor(pkg.GGML_TYPE_F32, 512, N))), N
    assert be.supports_op(c.get_rows(w, c.new_tensor(pkg.GGML_TYPE_I32, 3)))
    experts, ids = c.new_tensor(ty, 512, 64, 4), c.new_tensor(pkg.GGML_TYPE_I32, 2, 5)
    assert not be.supports_op(c.mul_mat_id(experts, c.new_tensor(pkg.GGML_TYPE_F32, 512, 2, 5), ids))
    short, x = c.new_tensor(ty, 512, 64), c.new_tensor(pkg.GGML_TYPE_F32, 384, 9)
    short.t.ne[0] = 384                                                  # a row length that is no multiple of the 256-weight block
    assert not be.supports_op(c.mul_mat(short, x))
    c.free()


@TYPES
@pytest.mark.parametrize("K", [256, 768])
def test_tq_get_rows_exact(pkg, be, ref_be, ty, K):
    """(xi - 1) * d is one exact float product: bit for bit the reference's rows, the first and the last row of the table among them"""
    R, idx = 37, np.array([0, 36, 5, 5, 17], np.int32)

    def make(c):
        w, i = c.new_tensor(ty, K, R), c.new_tensor(pkg.GGML_TYPE_I32, idx.size)
        return (w, i), c.get_rows(w, i)
    got, want = (_run(pkg, b, make, (_weights(ty, R, K), idx)) for b in (be, ref_be))
    assert want.size == idx.size * K and np.isfinite(want).all() and (want != 0).any() and np.array_equal(got, want)


# one case per edge: every N at which the path or the column slicing changes; a ragged row tile; K of one block and of nine (uneven over the K split); weight views
CASES = ([(N, 64, 768, False) for N in (1, 5, 8, 9, 31, 32, 33, 64, 65)] + [(5, 70, 768, False), (33, 70, 768, False), (1, 64, 256, False), (33, 64, 256, False),
         (8, 70, 2304, False), (33, 64, 2304, False), (64, 70, 2304, False), (5, 64, 768, True), (33, 64, 768, True), (33, 64, 768, "mmq_tq off")])


@TYPES
@pytest.mark.parametrize("N,M,K,view", CASES)
def test_tq_mul_mat_parity(pkg, be, ref_be, ty, N, M, K, view):
    off, view = view == "mmq_tq off", view is True                     # (the cross-check switch: 9 .. 64 columns land on the F16 image and meet its bar)
    wv = _weights(ty, M, K + 256 * view)
    xv = np.random.default_rng(N + M + K).standard_normal((N, K)).astype(np.float32)
    be.set_option("mmq_tq", int(not off))
    try:
        got = _gpu_counted(pkg, be, ty, N, wv, xv, M, K, view, image=off)
    finally:
        be.set_option("mmq_tq", 1)
    _check(got, _mul_mat(pkg, ref_be, ty, wv, xv, M, K, view), 5e-4 if N > 64 or off else 1e-8)


@TYPES
def test_tq_mmq_columns_independent(pkg, be, ty):
    """every column but two (one per column slice) replaced: the kept ones bit for bit"""
    M, K, keep = 70, 2304, [7, 32]
    wv = _weights(ty, M, K)
    rng = np.random.default_rng(5)
    x1, x2 = rng.standard_normal((33, K)).astype(np.float32), (rng.standard_normal((33, K)) * 3.0).astype(np.float32)
    x2[keep] = x1[keep]
    a, b = _gpu_counted(pkg, be, ty, 33, wv, x1, M, K), _gpu_counted(pkg, be, ty, 33, wv, x2, M, K)
    assert (a[keep] != 0).any() and not np.array_equal(a[0], b[0]) and np.array_equal(a[keep], b[keep])
