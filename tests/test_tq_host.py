"""TQ1_0 / TQ2_0 host side (no GPU): a numpy restatement of dequantize_row_tq1_0 / _tq2_0 against the reference CPU backend's GET_ROWS on qwen3.random_blocks
output, exact -- the generator and the element order that tests/test_tq_gpu.py rests on."""
import numpy as np
import pytest

TQ1_0, TQ2_0 = 34, 35


def _digits(b, n):                                                   # planes 0 .. n - 1 of every byte, (((uint8) (b * 3^p)) * 3) >> 8, the planes ahead of the bytes
    p = (3 ** np.arange(n, dtype=np.uint16))[:, None]
    return ((((b[..., None, :].astype(np.uint16) * p) & 0xFF) * 3) >> 8).reshape(*b.shape[:-1], -1)


def dequant(ty, raw, K):
    R, nb = raw.shape[0], K // 256
    if ty == TQ1_0:                                                  # qs[0..31]: five planes of 32, qs[32..47]: five planes of 16, qh[0..3]: four planes of 4
        b = raw.reshape(R, nb, 54)
        q = np.concatenate([_digits(b[..., 0:32], 5), _digits(b[..., 32:48], 5), _digits(b[..., 48:52], 4)], axis=-1)
    else:                                                            # two groups of 32 bytes, plane l = bits 2l, 2l + 1
        b = raw.reshape(R, nb, 66)
        q = ((b[..., :64].reshape(R, nb, 2, 1, 32) >> (2 * np.arange(4, dtype=np.uint8))[:, None]) & 3).reshape(R, nb, 256)
    d = b[..., -2:].copy().view(np.float16).astype(np.float32)
    return ((q.astype(np.float32) - 1.0) * d).reshape(R, K)


@pytest.mark.parametrize("ty,bs", [(TQ1_0, 54), (TQ2_0, 66)])
def test_tq_dequant_restatement_matches_reference(pkg, ref_be, ty, bs):
    from llama_cpp_omni_amd import qwen3
    R, K = 40, 768
    raw = qwen3.random_blocks(np.random.default_rng(ty), ty, R, K)
    assert raw.shape == (R, 3 * bs) and raw.dtype == np.uint8
    c = pkg.Context(ref_be)
    w, i = c.new_tensor(ty, K, R), c.new_tensor(pkg.GGML_TYPE_I32, R)
    y = c.get_rows(w, i)
    c.alloc()
    ref_be.tensor_set(w, raw); ref_be.tensor_set(i, np.arange(R, dtype=np.int32))
    ref_be.graph_compute(c.graph())
    want = ref_be.tensor_get(y).copy().reshape(R, K)
    c.free()
    assert np.isfinite(want).all() and (want > 0).any() and (want < 0).any()
    assert np.array_equal(dequant(ty, raw, K), want)
