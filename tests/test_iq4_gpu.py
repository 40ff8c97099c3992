"""IQ4_NL / IQ4_XS weights on the GPU (-m gpu): supports_op admits them, GET_ROWS de-quantises them bit for bit, MUL_MAT up to 8 columns
runs the integer mat-vec kernels (k_mmv_blocks with iq4nl_form on Q8_0 activation images, with iq4xs_form on Q8_K images: the integers of
ggml_vec_dot_iq4_nl_q8_0 / _iq4_xs_q8_K, f32 re-association only), from 9 columns on the F16-image GEMM; and the reference's libllama
keeps every layer of an IQ4 model on the plug-in.  Everything is compared with the reference CPU backend at test time."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")

IQ4_NL, IQ4_XS = 20, 23
TYPES = {"iq4_nl": IQ4_NL, "iq4_xs": IQ4_XS}
STAT = {"iq4_nl": "mmv_iq4nl_launches", "iq4_xs": "mmv_iq4xs_launches"}


def _weights(pkg, rng, ty, M, K):
    from llama_cpp_omni_amd import qwen3
    return qwen3.random_blocks(rng, ty, M, K)


def _xs_all_scales(rng, M, K):
    """IQ4_XS rows whose 32-weight sub-blocks run through every ls = 0 .. 63 (K = 2048: 64 sub-blocks per row, ls = (row + j) % 64)"""
    from llama_cpp_omni_amd import qwen3
    raw = qwen3.random_blocks(rng, IQ4_XS, M, K).reshape(M, K // 256, 136)
    for r in range(M):
        ls = (r + np.arange(K // 32)) % 64
        for b in range(K // 256):
            s = ls[8 * b: 8 * b + 8]
            raw[r, b, 2:4] = np.array([sum(int(s[i] >> 4) << (2 * i) for i in range(8))], np.uint16).view(np.uint8)
            raw[r, b, 4:8] = [(s[2 * i] & 0xF) | ((s[2 * i + 1] & 0xF) << 4) for i in range(4)]
    return raw.reshape(M, -1)


def _mul_mat(pkg, backend, ty, wv, xv, w_ne, x_ne, permute_x=False):
    c = pkg.Context(backend)
    w = c.new_tensor(ty, *w_ne)
    if permute_x:                                    # x stored [K, B, N], seen as [K, N, B]: rows of one batch element are not adjacent
        x0 = c.new_tensor(pkg.GGML_TYPE_F32, x_ne[0], x_ne[2], x_ne[1])
        x = c.permute(x0, 0, 2, 1, 3)
    else:
        x0 = x = c.new_tensor(pkg.GGML_TYPE_F32, *x_ne)
    y = c.mul_mat(w, x)
    c.alloc()
    backend.tensor_set(w, wv); backend.tensor_set(x0, xv)
    backend.graph_compute(c.graph())
    out = backend.tensor_get(y).copy()
    c.free()
    return out


@pytest.mark.parametrize("name", ["iq4_nl", "iq4_xs"])
def test_iq4_supports_op(pkg, be, name):
    """MUL_MAT against f32 activations (mat-vec and GEMM widths) and GET_ROWS are admitted for both types"""
    ty = TYPES[name]
    c = pkg.Context(be)
    w = c.new_tensor(ty, 512, 64)
    for n in (1, 8, 9, 64):
        x = c.new_tensor(pkg.GGML_TYPE_F32, 512, n)
        assert be.supports_op(c.mul_mat(w, x)), (name, n)
    idx = c.new_tensor(pkg.GGML_TYPE_I32, 3)
    assert be.supports_op(c.get_rows(w, idx)), name
    if name == "iq4_nl":                             # three blocks: not a multiple of 256 (the rows an IQ4_XS file demotes to IQ4_NL)
        w96 = c.new_tensor(ty, 96, 16)
        assert be.supports_op(c.mul_mat(w96, c.new_tensor(pkg.GGML_TYPE_F32, 96, 2)))
    else:
        w96 = c.new_tensor(ty, 96 * 8, 16)
        assert be.supports_op(c.mul_mat(w96, c.new_tensor(pkg.GGML_TYPE_F32, 96 * 8, 2)))


@pytest.mark.parametrize("name", ["iq4_nl", "iq4_xs"])
def test_iq4_get_rows_bit_exact(pkg, be, ref_be, name):
    """GET_ROWS is dequantize_row_iq4_nl / _iq4_xs: bit for bit the reference's floats; the IQ4_XS rows cover every ls = 0 .. 63"""
    ty, K, M = TYPES[name], 2048, 70
    rng = np.random.default_rng(5)
    wv = _xs_all_scales(rng, M, K) if ty == IQ4_XS else _weights(pkg, rng, ty, M, K)
    iv = rng.permutation(M)[:64].astype(np.int32)
    outs = []
    for backend in (be, ref_be):
        c = pkg.Context(backend)
        tab = c.new_tensor(ty, K, M)
        idx = c.new_tensor(pkg.GGML_TYPE_I32, 64)
        r = c.get_rows(tab, idx)
        c.alloc()
        backend.tensor_set(tab, wv); backend.tensor_set(idx, iv)
        backend.graph_compute(c.graph())
        outs.append(backend.tensor_get(r).copy())
        c.free()
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), name


SHAPES = [(48, 512, 1), (130, 1024, 5), (257, 768, 8), (33, 4096, 3), (4096, 4096, 1), (12288, 4096, 1), (4096, 12288, 1)]


@pytest.mark.parametrize("name,M,K,N", [(n, *s) for n in ("iq4_nl", "iq4_xs") for s in SHAPES] + [("iq4_nl", 40, 96, 1), ("iq4_nl", 70, 96, 7)])
@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0])
def test_iq4_mul_mat_integer_path(pkg, be, ref_be, name, M, K, N, scale):
    """Up to 8 columns: the IQ4 mat-vec kernels (one launch per call, counted), the reference's integers -- NMSE <= 1e-8"""
    ty = TYPES[name]
    rng = np.random.default_rng(M * 7 + K + N)
    wv = _weights(pkg, rng, ty, M, K)
    xv = (rng.standard_normal((N, K)) * scale).astype(np.float32)
    n0 = be.get_stat(STAT[name])
    got = _mul_mat(pkg, be, ty, wv, xv, (K, M), (K, N))
    assert be.get_stat(STAT[name]) - n0 == 1, "the IQ4 mat-vec kernel did not run (or ran more than once)"
    want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M), (K, N))
    assert np.isfinite(got).all()
    e = nmse(got, want)
    assert e <= 1e-8, (name, M, K, N, scale, e)


@pytest.mark.parametrize("name", ["iq4_nl", "iq4_xs"])
@pytest.mark.parametrize("N", [9, 24, 64, 200])
def test_iq4_mul_mat_image_path(pkg, be, ref_be, name, N):
    """9 columns and more: the F16 image of the blocks on the MFMA GEMM -- the reference's MUL_MAT bar (NMSE 5e-4)"""
    ty, M, K = TYPES[name], 320, 1024
    rng = np.random.default_rng(N)
    wv = _weights(pkg, rng, ty, M, K)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    n0 = be.get_stat(STAT[name])
    got = _mul_mat(pkg, be, ty, wv, xv, (K, M), (K, N))
    assert be.get_stat(STAT[name]) == n0                     # (not the mat-vec kernel)
    want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M), (K, N))
    assert np.isfinite(got).all()
    assert nmse(got, want) < 5e-4


@pytest.mark.parametrize("name", ["iq4_nl", "iq4_xs"])
@pytest.mark.parametrize("N", [3, 12])
@pytest.mark.parametrize("permute_x", [False, True])
def test_iq4_mul_mat_broadcast_and_permuted(pkg, be, ref_be, name, N, permute_x):
    """weights [K, M, 2, 1] against activations [K, N, 6, 1] (each weight matrix serves three activation matrices), the activation
    contiguous or seen through a PERMUTE"""
    ty, M, K = TYPES[name], 96, 512
    rng = np.random.default_rng(N + 3 * permute_x)
    wv = np.concatenate([_weights(pkg, rng, ty, M, K) for _ in range(2)])
    xv = rng.standard_normal((6 * N, K)).astype(np.float32)
    got = _mul_mat(pkg, be, ty, wv, xv, (K, M, 2, 1), (K, N, 6, 1), permute_x)
    want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M, 2, 1), (K, N, 6, 1), permute_x)
    assert np.isfinite(got).all()
    assert nmse(got, want) < 5e-4


def _greedy(gguf, ngl, fa, dump, env_extra=None):
    import json
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if env_extra:
        env.update(env_extra)
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "-fa", str(fa), "--greedy", "24", "-t", "4", "--dump-logits", dump],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], np.fromfile(dump, np.float32), out.stderr


@pytest.mark.parametrize("types", ["iq4_xs", "iq4_nl"])
@pytest.mark.parametrize("fa", [1, 0])
def test_iq4_models_stay_on_the_gpu(tmp_path, types, fa):
    """The reference's libllama with the plug-in on a tiny IQ4_XS file (the mixed map of qwen3.iq4_xs_types) and an IQ4_NL one: every layer
    offloaded, no mat-mul handed back to the CPU (the graph-split count of the Q4_0 model), logits inside the reference's bar.  Prefill runs on
    the F16 image (f16-rounded activations, not the CPU's Q8 ones), which can flip a near-tie of this random-weight toy model: 90 % of the
    greedy ids must agree."""
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built")
    gguf = str(tmp_path / "tiny.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gguf.py"), "--config", "tiny", "--types", types, "-o", gguf,
                    "--distinct-layers"], check=True, timeout=300)
    ids_cpu, l_cpu, _ = _greedy(gguf, 0, fa, str(tmp_path / "cpu.bin"))
    ids_gpu, l_gpu, err = _greedy(gguf, 99, fa, str(tmp_path / "gpu.bin"), {"GGML_BACKEND_PATH": LIB})
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err and "graph splits = 2" in err
    nm = float(((l_cpu - l_gpu) ** 2).sum() / (l_cpu ** 2).sum())
    assert nm < 5e-4, nm
    agree = sum(a == b for a, b in zip(ids_gpu, ids_cpu))
    assert agree >= 0.9 * len(ids_cpu), (ids_gpu, ids_cpu)
