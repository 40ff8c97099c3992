"""Q4_1 / Q5_1 / Q2_K / Q3_K weights on the GPU (-m gpu): MUL_MAT up to 8 columns runs the integer mat-vec kernels (k_mmv_blocks with q41_form on Q8_1
activation images, with q2k_form / q3k_form on Q8_K images: the integers of ggml_vec_dot_q4_1_q8_1 / _q5_1_q8_1 / _q2_K_q8_K / _q3_K_q8_K,
f32 re-association only) and builds no F16 image of the weights; from 9 columns on the F16-image GEMM as before; a decode graph and the
reference's libllama stay on the plug-in.  Everything is compared with the reference CPU backend at test time."""
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

Q4_1, Q5_1, Q2_K, Q3_K = 3, 7, 10, 11
TYPES = {"q4_1": Q4_1, "q5_1": Q5_1, "q2_k": Q2_K, "q3_k": Q3_K}
STAT = {"q4_1": "mmv_q41_launches", "q5_1": "mmv_q51_launches", "q2_k": "mmv_q2k_launches", "q3_k": "mmv_q3k_launches"}


def _weights(rng, ty, M, K):
    from llama_cpp_omni_amd import qwen3
    return qwen3.random_blocks(rng, ty, M, K)


def _f16_bytes(v):
    return np.array([v], np.float16).view(np.uint8)


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
    out = backend.tensor_get(y).copy().reshape(-1, w_ne[1])          # [columns (x batch), M]
    c.free()
    return out


# ---- 1. the integer path
SHAPES = [(48, 512, 1), (130, 1024, 5), (257, 768, 8), (33, 4096, 3), (4096, 4096, 1)]
CASES = ([(n, *s) for n in TYPES for s in SHAPES] +
         [(n, *s) for n in ("q4_1", "q5_1") for s in ((40, 96, 1), (70, 96, 7))] +          # three blocks, odd row counts, rows not 16-byte aligned
         [(n, 37, 256, 2) for n in ("q2_k", "q3_k")])                                        # a single super-block


@pytest.mark.parametrize("name,M,K,N", CASES)
@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0])
def test_lowbit_mul_mat_integer_path(pkg, be, ref_be, name, M, K, N, scale):
    """Up to 8 columns: the type's own mat-vec kernel (one launch per call, counted), the reference's integers -- NMSE <= 1e-8, the
    project's bar for its integer mat-vecs (Q4_0 / Q5_0, IQ4)"""
    ty = TYPES[name]
    rng = np.random.default_rng(M * 7 + K + N)
    wv = _weights(rng, ty, M, K)
    xv = (rng.standard_normal((N, K)) * scale).astype(np.float32)
    n0 = be.get_stat(STAT[name])
    got = _mul_mat(pkg, be, ty, wv, xv, (K, M), (K, N))
    assert be.get_stat(STAT[name]) - n0 == 1, "the type's mat-vec kernel did not run (or ran more than once)"
    want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M), (K, N))
    assert np.isfinite(got).all()
    e = nmse(got, want)
    print(name, M, K, N, scale, "nmse", e)
    assert e <= 1e-8, (name, M, K, N, scale, e)


# ---- 2. the Q8_1 quantiser's edge rows, read back through a Q4_1 mat-vec
def test_q8_1_image_edge_rows_bit_exact(pkg, be, ref_be):
    """Q4_1 weights with d = 0 everywhere and m = 1 in exactly one block per row (block row % 4): the output is that block's s = f16(d * sum(qs))
    of the activation column.  Columns: all zeros; one huge value per block; exact .5 rounding ties (amax = 127, so x * id = k + 0.5);
    blocks whose quant sum is negative.  Bits must equal the reference CPU backend's."""
    M, K, nb = 32, 128, 4
    rng = np.random.default_rng(81)
    raw = rng.integers(0, 256, size=(M, nb, 20), dtype=np.uint8)
    raw[..., 0:4] = 0                                                    # d = 0, m = 0
    for r in range(M):
        raw[r, r % nb, 2:4] = _f16_bytes(1.0)
    wv = raw.reshape(M, -1)
    x = np.zeros((4, nb, 32), np.float32)
    x[1] = rng.standard_normal((nb, 32)) * 1e-3
    x[1, np.arange(nb), rng.integers(0, 32, nb)] = [6e4, -6e4, 3e4, -1234.5]
    k = rng.integers(-126, 126, size=(nb, 32))
    x[2] = k + 0.5
    x[2, :, 0] = [127.0, -127.0, 127.0, -127.0]
    x[3] = -np.abs(rng.standard_normal((nb, 32))) * 3.0
    x[3, :, 5] = 0.25                                                    # (mostly negative, one small positive)
    xv = x.reshape(4, K)
    n0 = be.get_stat(STAT["q4_1"])
    got = _mul_mat(pkg, be, Q4_1, wv, xv, (K, M), (K, 4))
    assert be.get_stat(STAT["q4_1"]) - n0 == 1
    want = _mul_mat(pkg, ref_be, Q4_1, wv, xv, (K, M), (K, 4))
    assert np.isfinite(want).all() and (want[0] == 0).all() and (want[3] < 0).all() and (np.abs(want[1]) > 1000).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


# ---- 3. Q3_K scales and masks
def _q3k_all_scales(rng, M, K, hmask):
    """Q3_K rows whose 16-weight groups run through every 6-bit scale 0 .. 63 (K = 1024: 64 groups per row, scale = (row + group) % 64),
    packed as block_q3_K.scales: low nibbles in bytes 0..7 (groups 0..7 low, 8..15 high), the two high bits in bytes 8..11"""
    from llama_cpp_omni_amd import qwen3
    raw = qwen3.random_blocks(rng, Q3_K, M, K).reshape(M, K // 256, 110)
    for r in range(M):
        sc = (r + np.arange(K // 16)) % 64
        for b in range(K // 256):
            s = sc[16 * b: 16 * b + 16]
            sp = np.zeros(12, np.uint8)
            for k in range(16):
                grp, i = k >> 2, k & 3
                sp[(4 if grp & 1 else 0) + i] |= (int(s[k]) & 0xF) << (4 if grp >= 2 else 0)
                sp[8 + i] |= (int(s[k]) >> 4) << (2 * grp)
            raw[r, b, 96:108] = sp
    if hmask == "ones":
        raw[..., 0:32] = 0xFF
    elif hmask == "zeros":
        raw[..., 0:32] = 0
    return raw.reshape(M, -1)


@pytest.mark.parametrize("hmask", ["ones", "zeros", "random"])
@pytest.mark.parametrize("N", [1, 6])
def test_q3_k_every_scale_and_mask(pkg, be, ref_be, hmask, N):
    """every 6-bit scale value in every group position, with the high-bit mask all set (q = low bits), all clear (q = low bits - 4) and random"""
    M, K = 70, 1024
    rng = np.random.default_rng(3 + N)
    wv = _q3k_all_scales(rng, M, K, hmask)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    n0 = be.get_stat(STAT["q3_k"])
    got = _mul_mat(pkg, be, Q3_K, wv, xv, (K, M), (K, N))
    assert be.get_stat(STAT["q3_k"]) - n0 == 1
    want = _mul_mat(pkg, ref_be, Q3_K, wv, xv, (K, M), (K, N))
    assert np.isfinite(got).all()
    e = nmse(got, want)
    print("q3_k", hmask, N, "nmse", e)
    assert e <= 1e-8, (hmask, N, e)


# ---- 4. Q2_K: the scale term and the min term on their own
@pytest.mark.parametrize("N", [1, 4])
def test_q2_k_scale_and_min_terms_separately(pkg, be, ref_be, N):
    """even rows d = 0 (only - dmin * sum m * bsums is left), odd rows dmin = 0 (only d * sum sc * sum(q2 * q8))"""
    M, K = 66, 768
    rng = np.random.default_rng(20 + N)
    raw = _weights(rng, Q2_K, M, K).reshape(M, K // 256, 84)
    raw[0::2, :, 80:82] = 0
    raw[1::2, :, 82:84] = 0
    wv = raw.reshape(M, -1)
    xv = (rng.standard_normal((N, K)) + 0.3).astype(np.float32)             # (a non-zero mean: bsums that do not cancel)
    n0 = be.get_stat(STAT["q2_k"])
    got = _mul_mat(pkg, be, Q2_K, wv, xv, (K, M), (K, N))
    assert be.get_stat(STAT["q2_k"]) - n0 == 1
    want = _mul_mat(pkg, ref_be, Q2_K, wv, xv, (K, M), (K, N))
    assert np.isfinite(got).all() and np.abs(want[:, 0::2]).min() > 0 and np.abs(want[:, 1::2]).max() > 0
    for part, name in ((slice(0, None, 2), "min term"), (slice(1, None, 2), "scale term")):
        e = nmse(got[:, part], want[:, part])
        print("q2_k", name, N, "nmse", e)
        assert e <= 1e-8, (name, N, e)


# ---- 5. from 9 columns on: the F16-image GEMM, and no image for a weight that only ever sees mat-vec widths
@pytest.mark.parametrize("name", sorted(TYPES))
@pytest.mark.parametrize("N", [9, 24, 64, 200])
def test_lowbit_mul_mat_image_path(pkg, be, ref_be, name, N):
    """9 columns and more: the F16 image of the blocks on the MFMA GEMM -- the reference's MUL_MAT bar (NMSE 5e-4)"""
    ty, M, K = TYPES[name], 320, 1024
    rng = np.random.default_rng(N)
    wv = _weights(rng, ty, M, K)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    n0 = be.get_stat(STAT[name])
    got = _mul_mat(pkg, be, ty, wv, xv, (K, M), (K, N))
    assert be.get_stat(STAT[name]) == n0                     # (not the mat-vec kernel)
    want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M), (K, N))
    assert np.isfinite(got).all()
    assert nmse(got, want) < 5e-4


@pytest.mark.parametrize("name", sorted(TYPES))
def test_lowbit_mat_vec_builds_no_weight_image(pkg, be, ref_be, name):
    """a weight in a WEIGHTS-usage buffer: one column builds no resident F16 image (stat shadow_tensors), the first GEMM on it still does"""
    ty, M, K = TYPES[name], 320, 1024
    rng = np.random.default_rng(17)
    wv = _weights(rng, ty, M, K)
    wctx = pkg.Context(be)
    w = wctx.new_tensor(ty, K, M)
    wctx.alloc(usage=pkg.GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
    be.tensor_set(w, wv)
    n0, c0 = be.get_stat("shadow_tensors"), be.get_stat(STAT[name])
    for N, images in ((1, 0), (9, 1)):
        c = pkg.Context(be)
        wl = c._new(w.type, w.ne, view_src=w, view_offs=0)
        for i in range(4):
            wl.t.nb[i] = w.t.nb[i]
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
        y = c.mul_mat(wl, x)
        c.alloc()
        xv = rng.standard_normal((N, K)).astype(np.float32)
        be.tensor_set(x, xv)
        be.graph_compute(c.graph())
        got = be.tensor_get(y).copy().reshape(N, M)
        c.free()
        assert be.get_stat("shadow_tensors") == n0 + images, (name, N)
        want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M), (K, N))
        assert nmse(got, want) < (1e-8 if N == 1 else 5e-4), (name, N)
    assert be.get_stat(STAT[name]) == c0 + 1
    wctx.free()
    assert be.get_stat("shadow_tensors") == n0


# ---- 6. broadcast and permuted activations
@pytest.mark.parametrize("name", sorted(TYPES))
@pytest.mark.parametrize("N", [3, 12])
@pytest.mark.parametrize("permute_x", [False, True])
def test_lowbit_mul_mat_broadcast_and_permuted(pkg, be, ref_be, name, N, permute_x):
    """weights [K, M, 2, 1] against activations [K, N, 6, 1] (each weight matrix serves three activation matrices), the activation
    contiguous or seen through a PERMUTE"""
    ty, M, K = TYPES[name], 96, 512
    rng = np.random.default_rng(N + 3 * permute_x)
    wv = np.concatenate([_weights(rng, ty, M, K) for _ in range(2)])
    xv = rng.standard_normal((6 * N, K)).astype(np.float32)
    got = _mul_mat(pkg, be, ty, wv, xv, (K, M, 2, 1), (K, N, 6, 1), permute_x)
    want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M, 2, 1), (K, N, 6, 1), permute_x)
    assert np.isfinite(got).all()
    assert nmse(got, want) < 5e-4


# ---- 7. a decode graph: none of the K-quant launch forms takes Q2_K / Q3_K
def test_q3_k_q2_k_decode_layer_is_not_mis_fused(pkg, be, ref_be):
    """one Qwen3 layer, Q3_K q / k / v / o / gate / up and Q2_K down (Q6_K head), one token per step: every one of those mat-muls runs its
    type's own kernel (6 Q3_K + 1 Q2_K launches in the eager first step) and the logits of every step stay inside the reference's bar"""
    from llama_cpp_omni_amd import qwen3
    cfg = dict(n_embd=256, n_layer=1, n_head=4, n_head_kv=2, head_dim=64, n_ff=512, n_vocab=512, rms_eps=1e-6, rope_base=1e6, n_ctx_orig=4096)
    types = {"output": 14, 0: dict(attn_q=Q3_K, attn_k=Q3_K, attn_v=Q3_K, attn_output=Q3_K, ffn_gate=Q3_K, ffn_up=Q3_K, ffn_down=Q2_K)}
    steps, n_kv = 3, 256
    embd = np.random.default_rng(9).standard_normal((steps, cfg["n_embd"])).astype(np.float32)
    outs = {}
    for key, backend in (("ref", ref_be), ("gpu", be)):
        mdl = qwen3.Model(backend, cfg, types, n_ctx=n_kv, seed=11, flash_attn=True)
        g, I, logits = mdl.build(1, n_kv)
        gr = g.graph()
        res = []
        for t in range(steps):
            n3, n2 = (be.get_stat(STAT["q3_k"]), be.get_stat(STAT["q2_k"])) if key == "gpu" else (0, 0)
            mdl.set_inputs(I, embd[t:t + 1], t, n_kv)
            backend.graph_compute(gr)
            res.append(backend.tensor_get(logits).copy())
            if key == "gpu" and t == 0:                       # (the eager submission: later ones may replay a captured graph)
                assert be.get_stat(STAT["q3_k"]) - n3 == 6 and be.get_stat(STAT["q2_k"]) - n2 == 1
        g.free(); mdl.wctx.free()
        outs[key] = np.stack(res)
    assert np.isfinite(outs["gpu"]).all()
    for t in range(steps):
        e = nmse(outs["gpu"][t], outs["ref"][t])
        assert e < 5e-4, (t, e)


# ---- 8. libllama
def _greedy(gguf, ngl, fa, dump, env_extra=None):
    import json
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if env_extra:
        env.update(env_extra)
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "-fa", str(fa), "--greedy", "24", "-t", "4", "--dump-all-logits", dump],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], np.fromfile(dump, np.float32).reshape(24, -1), out.stderr


@pytest.mark.parametrize("types", ["q3_k", "q2_k", "q4_1", "q5_1"])
@pytest.mark.parametrize("fa", [1, 0])
def test_lowbit_models_stay_on_the_gpu(tmp_path, types, fa):
    """The reference's libllama with the plug-in on tiny uniform Q3_K / Q2_K / Q4_1 / Q5_1 files, 24 greedy one-token steps: every layer
    offloaded, no mat-mul handed back to the CPU (the graph-split count of the Q4_0 model), logits inside the reference's bar (NMSE < 5e-4),
    90 % of the greedy ids equal.

    The logits are compared at EVERY step at which both runs had been fed the same tokens -- all 24, the last one included, when the ids
    agree; up to and including the first differing id otherwise (what follows it are answers to different inputs).  Measured on an MI355X:
    without flash-attention both backends do the same arithmetic and every step of every type sits at 4e-15 .. 4e-14, ids equal.  With
    it the CPU accumulates V in f16 and this backend in f32: 1e-4 .. 2e-4 per step.  On the Q3_K file that difference flips a near-tie of
    the reference's own at step 11 (its top-2 gap there is 0.0011 at a logit spread of 0.34; with flash-attention off BOTH backends
    pick the token the GPU picks): the ids are then one step apart (22 of 24 equal) and the last step's logits, answers to different
    prefixes, are 1.5e-2 apart -- steps 0 .. 11 are at <= 2.1e-4."""
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built")
    gguf = str(tmp_path / "tiny.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gguf.py"), "--config", "tiny", "--types", types, "-o", gguf,
                    "--distinct-layers"], check=True, timeout=300)
    ids_cpu, l_cpu, _ = _greedy(gguf, 0, fa, str(tmp_path / "cpu.bin"))
    ids_gpu, l_gpu, err = _greedy(gguf, 99, fa, str(tmp_path / "gpu.bin"), {"GGML_BACKEND_PATH": LIB})
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err and "graph splits = 2" in err
    same = [a == b for a, b in zip(ids_gpu, ids_cpu)]
    last = same.index(False) if False in same else len(same) - 1          # the last step whose inputs were the same on both backends
    nms = [float(((l_cpu[t] - l_gpu[t]) ** 2).sum() / (l_cpu[t] ** 2).sum()) for t in range(len(same))]
    print(types, fa, "logits nmse per step", ["%.1e" % v for v in nms], "ids", ids_gpu, ids_cpu)
    assert np.isfinite(l_gpu).all()
    for t in range(last + 1):
        assert nms[t] < 5e-4, (t, nms[t])
    assert sum(same) >= 0.9 * len(ids_cpu), (ids_gpu, ids_cpu)
