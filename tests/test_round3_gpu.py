"""Round-3 GPU parity tests (through the C-ABI, `-m gpu`): the LDS-DMA loader / consumer engine of the batch-1 decode mat-vec (mmv2.hip) in every
launch form the decode step uses -- against the C oracle (the reference's integer dot over its own Q8_K image) and against the register-load
family (mmv1.hip) it replaces -- and the per-node identity check in front of every hipGraph replay.  Nothing here reads /root/reference."""
import numpy as np
import pytest

from conftest import nmse
from oracle import oracle_py as orc

pytestmark = pytest.mark.gpu


def _run(be, c, outs, feeds):
    from test_gpu_parity import run_graph
    return run_graph(be, c, outs, feeds)


def _silu(x):
    return x / (1.0 + np.exp(-x))


def _act(rng, K):
    x = (rng.standard_normal((1, K)) * 2.0).astype(np.float32)
    x[0, 256:512] = 0.0                                       # an all-zero Q8_K block
    x[0, 700] = -x[0, 701]                                    # a +/- tie candidate for the block maximum
    x[0, K - 256:K - 128] = 0.0
    return x


@pytest.mark.parametrize("name", ["q4_K", "q6_K"])
@pytest.mark.parametrize("K,M", [(4096, 4096), (12288, 4096), (4096, 19200)])
def test_engine_single_matrix_vs_oracle_and_register_family(pkg, be, name, K, M):
    """One matrix, plain f32 activation + residual epilogue (the wo / ffn_down launches; M = 19200: 75 rows per workgroup, more steps than the
    LDS ring holds, so slots are re-used behind the consumers).  The engine and mmv1 form the same integer sums; only the order of the f32
    partial sums over super-blocks differs."""
    from llama_cpp_omni_amd import qwen3
    ty = {"q4_K": pkg.GGML_TYPE_Q4_K, "q6_K": pkg.GGML_TYPE_Q6_K}[name]
    rng = np.random.default_rng(K + M)
    x = _act(rng, K)
    r = rng.standard_normal((1, M)).astype(np.float32)
    wv = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    wb = wv.view(np.uint8).reshape(M, -1)
    res = {}
    for mv2 in (1, 0):
        be.set_option("mv2", mv2)
        try:
            c = pkg.Context(be)
            w = c.new_tensor(ty, K, M); xt = c.new_tensor(pkg.GGML_TYPE_F32, K, 1); rt = c.new_tensor(pkg.GGML_TYPE_F32, M, 1)
            y = c.add(c.mul_mat(w, xt), rt)
            (res[mv2],) = _run(be, c, [y], [(w, wv), (xt, x), (rt, r)])
            assert be.get_stat("kernels_last_graph") == 1
        finally:
            be.set_option("mv2", 1)
    want = orc.mul_mat(ty, wb, x) + r
    assert nmse(res[1], want) < 1e-9, nmse(res[1], want)
    assert nmse(res[1], res[0]) < 1e-12, nmse(res[1], res[0])


def test_engine_gate_up_pair_with_norm_and_swiglu(pkg, be):
    """The dominant launch of the decode step: RMS_NORM + MUL folded into the prologue (the sum of squares in double, the scale computed once per
    workgroup), ffn_gate and ffn_up streamed as one pair of rings, SwiGLU in the epilogue -- 12288 x 4096 Q4_K twice, one launch."""
    from llama_cpp_omni_amd import qwen3
    K, M = 4096, 12288
    rng = np.random.default_rng(5)
    x = _act(rng, K)
    nw = rng.standard_normal(K).astype(np.float32)
    ty = pkg.GGML_TYPE_Q4_K
    gv = qwen3.random_blocks(rng, ty, M, K, std=0.05); uv = qwen3.random_blocks(rng, ty, M, K, std=0.05)
    res = {}
    for mv2 in (1, 0):
        be.set_option("mv2", mv2)
        try:
            c = pkg.Context(be)
            wg = c.new_tensor(ty, K, M); wu = c.new_tensor(ty, K, M); xt = c.new_tensor(pkg.GGML_TYPE_F32, K, 1); nt = c.new_tensor(pkg.GGML_TYPE_F32, K)
            xn = c.mul(c.rms_norm(xt, 1e-6), nt)
            up = c.mul_mat(wu, xn); gate = c.mul_mat(wg, xn)
            y = c.swiglu_split(gate, up)
            (res[mv2],) = _run(be, c, [y], [(wg, gv), (wu, uv), (xt, x), (nt, nw)])
            assert be.get_stat("kernels_last_graph") == 1
        finally:
            be.set_option("mv2", 1)
    xn_ref = (orc.rms_norm(x, 1e-6) * nw).astype(np.float32)
    g = orc.mul_mat(ty, gv.view(np.uint8).reshape(M, -1), xn_ref); u = orc.mul_mat(ty, uv.view(np.uint8).reshape(M, -1), xn_ref)
    want = (_silu(g.astype(np.float64)) * u.astype(np.float64)).astype(np.float32)
    assert nmse(res[1], want) < 1e-9, nmse(res[1], want)
    assert nmse(res[1], res[0]) < 1e-12, nmse(res[1], res[0])


@pytest.mark.parametrize("vtype", ["q4_K", "q6_K"])
def test_engine_grouped_qkv_launch(pkg, be, vtype):
    """wq / wk / wv on one normalised activation: three matrices in one launch, workgroups split between them by bytes; with the Q4_K_M map
    attn_v is Q6_K on half the layers, so one launch mixes the two weight formats (and the two ring geometries)."""
    from llama_cpp_omni_amd import qwen3
    K = 4096
    rows = [4096, 1024, 1024]
    types = [pkg.GGML_TYPE_Q4_K, pkg.GGML_TYPE_Q4_K, pkg.GGML_TYPE_Q6_K if vtype == "q6_K" else pkg.GGML_TYPE_Q4_K]
    rng = np.random.default_rng(9)
    x = _act(rng, K)
    nw = rng.standard_normal(K).astype(np.float32)
    wvs = [qwen3.random_blocks(rng, t, m, K, std=0.05) for t, m in zip(types, rows)]
    res = {}
    for mv2 in (1, 0):
        be.set_option("mv2", mv2)
        try:
            c = pkg.Context(be)
            ws = [c.new_tensor(t, K, m) for t, m in zip(types, rows)]
            xt = c.new_tensor(pkg.GGML_TYPE_F32, K, 1); nt = c.new_tensor(pkg.GGML_TYPE_F32, K)
            xn = c.mul(c.rms_norm(xt, 1e-6), nt)
            ys = [c.mul_mat(w, xn) for w in ws]
            res[mv2] = _run(be, c, ys, list(zip(ws, wvs)) + [(xt, x), (nt, nw)])
            assert be.get_stat("kernels_last_graph") == 1
        finally:
            be.set_option("mv2", 1)
    xn_ref = (orc.rms_norm(x, 1e-6) * nw).astype(np.float32)
    for i, (t, m) in enumerate(zip(types, rows)):
        want = orc.mul_mat(t, wvs[i].view(np.uint8).reshape(m, -1), xn_ref)
        assert nmse(res[1][i], want) < 1e-9, (i, nmse(res[1][i], want))
        assert nmse(res[1][i], res[0][i]) < 1e-12, i


def test_replay_is_guarded_by_the_per_node_record_not_by_the_fingerprint(pkg, be):
    """Every cgraph is given the SAME fingerprint (test hook).  Two graphs of identical structure but different tensors are alive together; A is
    submitted until it is captured and replays, then B is submitted: a fingerprint-keyed replay would launch A's capture (and write A's
    output); the per-node record (data pointers, op, type, shape, strides, op_params, source pointers, readers outside the graph) refuses it,
    B runs and is captured on its own, and both keep giving their own results."""
    rng = np.random.default_rng(1)
    n = 1024

    def chain(scale):
        c = pkg.Context(be)
        x = c.new_tensor(pkg.GGML_TYPE_F32, n, 1); b = c.new_tensor(pkg.GGML_TYPE_F32, n, 1)
        y = x
        for _ in range(12):
            y = c.add(y, b)
        c.alloc()
        xv = rng.standard_normal((1, n)).astype(np.float32); bv = (rng.standard_normal((1, n)) * scale).astype(np.float32)
        be.tensor_set(x, xv); be.tensor_set(b, bv)
        want = xv.copy()
        for _ in range(12):
            want = want + bv
        return c, c.graph(), y, want

    be.set_option("graphs", 1)
    be.set_option("fp_collide", 1)
    try:
        ca, ga, ya, wa = chain(1.0)
        cb, gb, yb, wb = chain(3.0)
        mis0, rep0 = be.get_stat("graph_fp_mismatch"), be.get_stat("graph_replays")
        for _ in range(4):
            be.graph_compute(ga)
        assert np.array_equal(be.tensor_get(ya).ravel(), wa.ravel())
        assert be.get_stat("graph_replays") > rep0                       # A is captured and replays
        for _ in range(4):
            be.graph_compute(gb)
        assert np.array_equal(be.tensor_get(yb).ravel(), wb.ravel())                     # B ran as B
        assert be.get_stat("graph_fp_mismatch") > mis0                   # ... after A's capture was refused for it
        be.graph_compute(ga)
        assert np.array_equal(be.tensor_get(ya).ravel(), wa.ravel())
        ca.free(); cb.free()
    finally:
        be.set_option("fp_collide", 0)


def test_batched_small_uploads_keep_stream_order(pkg, be):
    """set_tensor_async of small inputs is staged and written by one launch in front of the next stream work: later writes win over earlier
    ones whatever their size (staged or direct copy), reads see them, and the result equals the one-copy-per-call path."""
    rng = np.random.default_rng(2)
    n_big = 64 * 1024                                            # 256 KB: above the staging limit -> direct copy
    c = pkg.Context(be)
    t = c.new_tensor(pkg.GGML_TYPE_F32, n_big, 1)
    s = c.new_tensor(pkg.GGML_TYPE_F32, 1000, 1)
    y = c.add(s, s)
    c.alloc()
    small = [rng.standard_normal(1000).astype(np.float32) for _ in range(3)]
    big = [rng.standard_normal(n_big).astype(np.float32) for _ in range(2)]
    out = np.empty(n_big, np.float32)
    for batch in (1, 0):
        be.set_option("batch_uploads", batch)
        try:
            be.tensor_set_async(t, big[0])
            be.tensor_set_async(t, small[0])                    # staged, after the direct copy: overwrites the first 1000 values
            be.tensor_get_async(t, out); be.synchronize()
            assert np.array_equal(out[:1000], small[0]) and np.array_equal(out[1000:], big[0][1000:])
            be.tensor_set_async(t, small[1])                    # staged ...
            be.tensor_set_async(t, big[1])                      # ... then a direct copy over it: the direct copy must come second
            be.tensor_get_async(t, out); be.synchronize()
            assert np.array_equal(out, big[1])
            for k in range(70):                                 # more entries than one staging table holds
                be.tensor_set_async(s, small[k % 3])
            be.graph_compute(c.graph())
            assert np.array_equal(be.tensor_get(y).ravel(), small[69 % 3] * 2)
        finally:
            be.set_option("batch_uploads", 1)
    c.free()


# ------------------------------------------------------------------------------------------------ 8B shape through the reference libllama
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")


def _bench_min(gguf, ngl, fa, n, threads, extra, plug):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if plug:
        env["GGML_BACKEND_PATH"] = LIB
    cmd = [BIN, "-m", gguf, "-ngl", str(ngl), "-fa", str(fa), "--greedy", str(n), "-t", str(threads)] + extra
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    if plug:
        assert "MI355X0" in out.stderr and "offloaded 37/37 layers to GPU" in out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"]


def _need_ref(tmp_path):
    import shutil
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    if shutil.disk_usage(str(tmp_path)).free < 7e9:
        pytest.skip("needs 5 GB of scratch disk for the synthetic 8B GGUF")


def test_8b_greedy_ids_identical_on_the_separated_logits_fixture(tmp_path):
    """SURVEY.md 7 / BASELINE 3.4: greedy token ids identical to the CPU backend over the benchmark length.  The 36-layer Qwen3-8B Q4_K_M
    GGUF is written with `--separated 160`: 160 special tokens whose embedding row is ~20x larger than what the 36 random layers add to the
    residual stream, and whose successor's lm-head row is a unit-rms copy of that embedding direction (the generator asserts the runner-up logit
    of the pure embedding direction is < 0.7 of the winner; at n_embd 4096 it is ~0.06).  Every kernel of the decode step still runs on full-size
    random weights; what the fixture removes is the near-ties of a random lm head, so that 128 greedy steps -- NOT teacher-forced: the plug-in
    continues from its own ids -- are IDENTICAL to the reference CPU backend's, with flash-attention off (llama-bench's default) and on, and
    the winning margin is checked against the measured logit difference at every step."""
    _need_ref(tmp_path)
    gguf = str(tmp_path / "q8b_sep.gguf")
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gguf.py"), "--config", "8b", "--types", "q4_k_m", "-o", gguf, "--n-ctx", "4096",
                          "--separated", "160"], check=True, timeout=1800, capture_output=True, text=True)
    start = int(gen.stdout.split("start token")[1].split()[0])
    threads = max(4, min(48, len(os.sched_getaffinity(0)) // 2))
    n = 128
    try:
        for fa in (0, 1):
            ids_cpu = _bench_min(gguf, 0, fa, n, threads, ["--start-token", str(start), "--dump-all-logits", str(tmp_path / "c.bin")], False)
            ids_gpu = _bench_min(gguf, 99, fa, n, threads, ["--start-token", str(start), "--dump-all-logits", str(tmp_path / "g.bin")], True)
            assert len(set(ids_cpu)) == n, "the fixture's cycle is longer than the run"
            assert ids_gpu == ids_cpu, (fa, [i for i in range(n) if ids_gpu[i] != ids_cpu[i]])
            lc = np.fromfile(str(tmp_path / "c.bin"), np.float32).reshape(n, -1); lg = np.fromfile(str(tmp_path / "g.bin"), np.float32).reshape(n, -1)
            worst = 0.0
            for t in range(n):
                top2 = np.partition(lc[t], -2)[-2:]
                rms = float(np.sqrt(np.mean((lg[t] - lc[t]) ** 2)))
                assert top2[1] - top2[0] > 16.0 * rms, (fa, t, top2, rms)           # the margin is what makes identical ids a fair demand
                worst = max(worst, float(((lg[t] - lc[t]) ** 2).sum() / (lc[t] ** 2).sum()))
            print(f"fa={fa}: {n}/{n} greedy ids identical, worst logits NMSE {worst:.2e}")
    finally:
        os.remove(gguf)


def test_8b_layer_by_layer_on_identical_inputs(tmp_path):
    """Per-layer parity at the headline shape: the reference CPU backend decodes 8 tokens of the (ordinary, random-lm-head) synthetic Qwen3-8B Q4_K_M
    GGUF and dumps the residual stream after every layer (`l_out-<il>`, through ggml_backend_sched's eval callback like the reference's
    examples/eval-callback).  The plug-in then decodes the same ids with every `l_out-<il>` OVERWRITTEN by the CPU's values as soon as it is
    computed, so layer il + 1 of the plug-in starts from the CPU's bits: its own output is compared with the CPU's on identical inputs, layer by
    layer -- a one-ulp bug in layer 20 cannot hide behind accumulated rounding noise.  What is compared is the layer's own CONTRIBUTION
    (l_out[il] - l_out[il - 1]), not the residual stream it rides on.
    The cells of the (step, layer) table fall in two groups.  Most are ~1e-13: the integer block sums are identical and the f32 additions across
    super-blocks (64-lane butterfly here, 8-lane SIMD there) differ in the last bit only.  The others are ~1e-5 .. 1e-4: a 1e-7 difference moved ONE
    value of a Q8_K activation image across a rounding boundary (ffn_down's input has 12288 heavy-tailed values: a +-1 step of one of them is
    (max / 127)^2 / |x|^2 ~ 5e-6 .. 2e-5 of the layer's contribution, and P(flip) ~ 2e-5 per value -> about one cell in four).  Any implementation
    with another summation order has these; the bars are therefore: every cell < 3e-4 (a handful of flips), and the MEDIAN cell < 1e-9
    (bit-level agreement wherever no rounding flipped).  With flash-attention on the reference accumulates V in f16 (ops.cpp:8069-8083) where this
    backend keeps f32 -- a documented deviation of ~5e-4 relative on the attention output, which wo's Q8_K quantiser turns into flips in
    every cell: no median bar there, every cell < 5e-4 (measured: median 5e-5, worst 1.8e-4; flash-attention off: median 3.5e-13, worst 9.8e-5)."""
    _need_ref(tmp_path)
    gguf = str(tmp_path / "q8b.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gguf.py"), "--config", "8b", "--types", "q4_k_m", "-o", gguf, "--n-ctx", "4096"], check=True, timeout=1800)
    threads = max(4, min(48, len(os.sched_getaffinity(0)) // 2))
    n, L, E = 8, 36, 4096
    try:
        for fa, bar in ((0, 3e-4), (1, 5e-4)):
            cl, gl = str(tmp_path / "cl.bin"), str(tmp_path / "gl.bin")
            ids_cpu = _bench_min(gguf, 0, fa, n, threads, ["--dump-layers", cl], False)
            _bench_min(gguf, 99, fa, n, threads, ["--force-ids", ",".join(map(str, ids_cpu)), "--force-layers", cl, "--dump-layers", gl], True)
            c = np.fromfile(cl, np.float32).reshape(n, L, E); g = np.fromfile(gl, np.float32).reshape(n, L, E)
            # the quantity a layer adds is what it computed: compare the layer's own contribution (output - input), not the residual stream it rides on
            tab = np.zeros((n, L))
            for t in range(n):
                for il in range(1, L):
                    dc = c[t, il] - c[t, il - 1]; dg = g[t, il] - c[t, il - 1]
                    tab[t, il] = float(((dg - dc) ** 2).sum() / (dc ** 2).sum())
            print(f"fa={fa}: per-layer NMSE of the layer's contribution, worst over 8 steps:", " ".join("%.0e" % tab[:, il].max() for il in range(1, L)))
            med = float(np.median(tab[:, 1:]))
            print(f"fa={fa}: median cell {med:.1e}, worst {tab.max():.1e}, cells above 1e-9: {int((tab[:, 1:] > 1e-9).sum())} of {n * (L - 1)}")
            assert tab.max() < bar, (fa, float(tab.max()), np.unravel_index(tab.argmax(), tab.shape))
            if fa == 0:
                assert med < 1e-9, med
            # layer 0 starts from the embedding row (GET_ROWS: bit-exact dequantisation on both sides): the whole tensor
            e0 = max(float(((g[t, 0] - c[t, 0]) ** 2).sum() / (c[t, 0] ** 2).sum()) for t in range(n))
            assert e0 < bar, e0
    finally:
        os.remove(gguf)


# ------------------------------------------------------------------------------------------------ the reference's omni encoders through the plug-in
ENC = os.path.join(ROOT, "oracle", "_ref", "omni-enc-min")


def _enc_min(module, gguf, out, gpu, extra, threads):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    env.pop("MTMD_BACKEND_DEVICE", None)
    if gpu:
        env["GGML_BACKEND_PATH"] = LIB
        env["MTMD_BACKEND_DEVICE"] = "MI355X0"
        env["MI355X_LOG_STATS"] = "1"
    r = subprocess.run([ENC, module, gguf, out, "--threads", str(threads)] + (["--gpu"] if gpu else []) + extra, env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    if gpu:
        import re                                          # the plug-in's own account of what it ran (printed when the encoder frees its backend)
        m = re.search(r"\[mi355x\] MI355X0: graphs eager=(\d+) captured=(\d+) replayed=(\d+), kernels in last graph=(\d+)", r.stdout + r.stderr)
        assert m and int(m.group(1)) + int(m.group(2)) + int(m.group(3)) >= 2 and int(m.group(4)) > 100, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("module,extra,n_tok", [("apm", ["--chunks", "17", "--frames", "100"], 170), ("vpm", ["--chunks", "2", "--size", "448x448"], 128)])
def test_reference_omni_encoder_code_runs_on_the_plugin(tmp_path, module, extra, n_tok):
    """SURVEY.md 8(f) rank 3/4 with the REFERENCE's graph builders instead of a mirror: tools/omni/audition.cpp (build_whisper :341-715 -- conv stem,
    24 Whisper-medium blocks over the streaming K/V cache, avg-pool, audio projector) and tools/omni/vision.cpp (build_minicpmv :292-380 -- 27 SigLIP
    blocks at 1024 patches, the 64-query resampler), compiled from /root/reference by oracle/Makefile.ref `omni`, load a full-size synthetic module GGUF
    (tools/make_synth_omni_gguf.py, written the way convert_apm.py / convert_vpm.py lay it out) and run it through ggml_backend_sched once on the CPU
    backend and once on the plug-in (MTMD_BACKEND_DEVICE=MI355X0).  Bar: NMSE of every chunk's embeddings <= 5e-6 (f16 weights; the CPU backend rounds
    the activations to f16 for its f16 dot products, the plug-in's MFMA GEMM does the same, the accumulation orders differ)."""
    if not os.path.exists(ENC):
        pytest.skip("oracle/_ref/omni-enc-min not built (make -f oracle/Makefile.ref omni)")
    gguf = str(tmp_path / f"{module}.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_omni_gguf.py"), "--module", module, "-o", gguf], check=True, timeout=900)
    threads = max(4, min(48, len(os.sched_getaffinity(0)) // 2))
    try:
        co, go = str(tmp_path / "c.bin"), str(tmp_path / "g.bin")
        jc = _enc_min(module, gguf, co, False, extra, threads)
        jg = _enc_min(module, gguf, go, True, extra, threads)
        assert jc["tokens"] == jg["tokens"] == n_tok and jc["n_embd"] == 4096
        c = np.fromfile(co, np.float32).reshape(n_tok, 4096); g = np.fromfile(go, np.float32).reshape(n_tok, 4096)
        assert np.isfinite(g).all() and float(c.std()) > 0.05
        n_chunks = int(extra[1]); per = n_tok // n_chunks
        errs = [float(((g[i * per:(i + 1) * per] - c[i * per:(i + 1) * per]) ** 2).sum() / (c[i * per:(i + 1) * per] ** 2).sum()) for i in range(n_chunks)]
        print(f"{module}: plug-in ms per chunk {jg.get('ms_chunks')}"); print(f"{module}: NMSE per chunk {['%.1e' % e for e in errs]}; cpu {jc['ms_last_chunk']:.1f} ms/chunk ({threads} threads), plug-in {jg['ms_last_chunk']:.2f} ms/chunk")
        assert max(errs) <= 5e-6, errs                      # measured 1e-7 (apm) and 7e-8 (vpm)
    finally:
        os.remove(gguf)


# ------------------------------------------------------------------------------------------------ module pinning / multi-GPU forms
def test_bench_two_ranks_over_rccl_when_two_gpus_are_visible(pkg, be):
    """The driver's N > 1 launch of bench.py with NO test hook: backend nccl (= RCCL), one GPU per rank, barrier + max-over-ranks.  Needs two MI355X
    in the box; the same code runs on every 1-GPU box through the gloo hooks (test_round2_gpu.py::test_bench_runs_as_two_ranks_through_its_gloo_hooks)."""
    if int(be.reg.contents.iface.get_device_count(be.reg)) < 2:
        pytest.skip("needs two MI355X in one box")
    env = dict(os.environ, MI355X_BENCH_NO_PP="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("MI355X_BENCH_DIST_BACKEND", "MI355X_BENCH_SHARE_GPU"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29573",
                          os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "8", "--warmup", "2", "--tiny", "--no-cpu-baseline"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["n_gpus"] == 2 and j["value"] > 0


def test_bench_omni_pinned_mode_measures_c4_and_c5_with_real_handoffs():
    """bench.py --omni-pinned: APM / VPM / LLM / TTS on their mi355x_module_device() backends (several streams of device 0 on a 1-GPU box), the
    embeddings moved by mi355x_handoff, TTFT and chunk time MEASURED end to end (not composed from legs).  Plumbing + sanity: finite results, every
    hand-off really went through the library (kind 1 = RCCL, 2 = device copy + event), and the concurrent APM / VPM submission does not take longer
    than the legs one after the other."""
    env = dict(os.environ, MI355X_BENCH_NO_PP="1", MI355X_BENCH_NO_EXTRAS="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "16", "--warmup", "4", "--full", "--no-cpu-baseline", "--no-c3", "--no-libllama", "--omni-pinned"],
                         env=env, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    o = j["omni_pinned"]
    assert "error" not in o, o
    c4, c5 = o["c4_stream_prefill_ttft"], o["c5_llm_to_tts_chunk"]
    print("omni_pinned:", json.dumps(o))
    assert c4["measured_ttft_ms"] and c5["measured_ms"]
    assert set(c4["handoff_kinds"].values()) <= {1, 2} and set(c5["handoff_kinds"].values()) <= {1, 2}
    assert c4["llm_prefill_tokens"] == 394
    assert c4["measured_ttft_ms"] <= 1.15 * c4["sum_of_legs_ms"] + 1.0


# ------------------------------------------------------------------------------------------------ the reference's Token2Wav end to end on the plug-in
T2W = os.path.join(ROOT, "oracle", "_ref", "t2w-min")


def test_reference_token2wav_end_to_end_on_the_plugin(tmp_path):
    """SURVEY.md 8(f) rank 4 / BASELINE configs[4] with the REFERENCE's own module: tools/omni/token2wav/token2wav-impl.cpp (Token2WavSession -- conformer
    token encoder with streaming caches, flow-matching DiT with 10 Euler steps and classifier-free guidance, HiFT vocoder with the f0 predictor, NSF source,
    three transposed-conv stages, snake resblocks and the 16-point iSTFT; compiled from /root/reference by oracle/Makefile.ref `omni`) on the full-size synthetic
    module set of tools/make_synth_omni_gguf.py --module t2w: prompt set-up, then three streaming windows of 25 + 3 tokens -> 3.1 s of 24 kHz audio.
    The module has no scheduler (token2wav-impl.cpp:6287-6345: one backend per sub-model), so a single node the plug-in declined would fail the run: the
    plug-in's stats line must show the graphs, and the waveform must match the CPU backend's.  Bar: NMSE <= 1e-4 over the whole waveform (the reference
    clamps it to +-0.99; f32 weights throughout: the differences are f32 summation order through ~15 000 nodes per window, and the sin / cos / exp of the source
    and iSTFT stages)."""
    if not os.path.exists(T2W):
        pytest.skip("oracle/_ref/t2w-min not built (make -f oracle/Makefile.ref omni)")
    d = str(tmp_path / "t2w")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_omni_gguf.py"), "--module", "t2w", "-o", d], check=True, timeout=900)

    def run(dev, out):
        env = dict(os.environ)
        env.pop("GGML_BACKEND_PATH", None)
        if dev == "gpu":
            env["GGML_BACKEND_PATH"] = LIB
            env["MI355X_LOG_STATS"] = "1"
        r = subprocess.run([T2W, d, out, dev, "--windows", "3"], env=env, capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        if dev == "gpu":
            assert "flowGGUFModelLoader: init_backend device=gpu, gpu_idx=0, backend=MI355X0" in r.stderr and "voc_hg2_model: init_backend device=gpu, gpu_idx=0, backend=MI355X0" in r.stderr, r.stderr[-3000:]
            import re
            m = re.findall(r"\[mi355x\] MI355X0: graphs eager=(\d+) captured=(\d+) replayed=(\d+), kernels in last graph=(\d+)", r.stderr)
            assert len(m) >= 1 and all(int(a) + int(b) + int(c) >= 3 for a, b, c, _ in m), r.stderr[-3000:]        # (printed when a backend is freed: the session frees the flow model's)
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    import shutil
    try:
        jg = run("gpu", str(tmp_path / "g.f32"))
        jc = run("cpu", str(tmp_path / "c.f32"))
        g = np.fromfile(str(tmp_path / "g.f32"), np.float32); c = np.fromfile(str(tmp_path / "c.f32"), np.float32)
        assert g.shape == c.shape and g.size == jc["samples"] == 74880 and np.isfinite(g).all()
        assert float(c.std()) > 0.02 and float((np.abs(c) >= 0.98).mean()) < 0.2           # a live waveform, mostly inside the clamp
        e = float(((g - c) ** 2).sum() / (c ** 2).sum())
        per = [float(((g[i:i + 24000] - c[i:i + 24000]) ** 2).sum() / (c[i:i + 24000] ** 2).sum()) for i in range(0, g.size - 1, 24000)]
        print(f"t2w: waveform NMSE {e:.2e} (per second {['%.1e' % x for x in per]}); plug-in RTF {jg['rtf']:.4f} ({jg['ms_windows']} ms per 1 s window), CPU backend RTF {jc['rtf']:.2f}")
        assert e <= 1e-4, (e, per)
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ------------------------------------------------------------------------------------------------ concurrent module threads on one device
def test_three_module_threads_on_one_device_give_their_single_thread_results(pkg):
    """SURVEY.md 8(b) threading: the omni pipeline drives LLM, TTS / encoders and Token2Wav from separate host threads, each with its own backend (= stream) on the same
    device (omni.h:194-196).  Three threads -- a decoder at the 8B widths (LDS-DMA mat-vec engine, one-token attention, hipGraph replay, staged uploads), a Whisper layer over
    500 frames (f16 MFMA GEMMs, LayerNorm fusion, soft-max) and a Token2Wav DiT block (f32 MFMA products, im2col convolutions, element-wise chains) -- run at the same
    time on three backends of device 0; every output must be bit-identical to what the same thread body produces when it runs alone.  Catches shared state between
    contexts (scratch blocks, weight-image table, arrival counters, kernel-side statics)."""
    import threading
    sys.path.insert(0, ROOT)
    import bench
    from llama_cpp_omni_amd import encoders as E, qwen3, token2wav as T
    cfg = dict(qwen3.QWEN3_8B); cfg["n_layer"] = 2; cfg["n_vocab"] = 4096

    def flat(W):
        out = [v for k, v in W.items() if k != "layers" and hasattr(v, "nelements")]
        for L in W.get("layers", []):
            out += list(L.values())
        return out

    def fill(b, tensors, seed):
        rng = np.random.default_rng(seed)
        for t in tensors:
            n = t.nelements()
            v = (rng.standard_normal(n) * 0.05).astype(np.float32)
            b.tensor_set(t, v.astype(np.float16) if t.type == 1 else (np.abs(v) + 0.5 if t.type == 0 and n <= 4096 else v) if t.type == 0 else np.zeros(n, np.int32))

    def body_llm(out):
        b = pkg.Backend(0)
        dec = bench.Decoder(pkg, b, cfg, qwen3.q4_k_m_types(cfg), n_ctx=256, n_kv=256, flash_attn=True, seed=77)
        for p in range(200):
            dec.step(p)
            out.append(dec.h_logits.copy())
        dec.g.free(); dec.model.wctx.free(); b.close()

    def body_apm(out):
        b = pkg.Backend(0)
        c = pkg.Context(b)
        W = E.whisper_weights(c, E.WHISPER, 1); inp, res = E.whisper(c, E.WHISPER, W, 500)
        c.alloc(); fill(b, flat(W) + [inp], 5)
        g = c.graph()
        for _ in range(120):
            b.graph_compute(g)
            out.append(b.tensor_get(res).copy())
        c.free(); b.close()

    def body_t2w(out):
        b = pkg.Backend(0)
        c = pkg.Context(b)
        W = T.dit_weights(c, T.DIT); x, cond, res = T.dit_block(c, T.DIT, W, 56)
        c.alloc(); fill(b, flat(W) + [x, cond], 9)
        g = c.graph()
        for _ in range(300):
            b.graph_compute(g)
            out.append(b.tensor_get(res).copy())
        c.free(); b.close()
    bodies = (body_llm, body_apm, body_t2w)
    alone = []
    for f in bodies:
        o = []; f(o); alone.append(o)
    together = [[] for _ in bodies]
    errs = []

    def run(f, o):
        try:
            f(o)
        except Exception as e:           # noqa: BLE001
            errs.append(repr(e))
    th = [threading.Thread(target=run, args=(f, o)) for f, o in zip(bodies, together)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert not errs, errs
    for name, a, b in zip(("llm", "apm", "t2w"), alone, together):
        assert len(a) == len(b) and len(a) > 0, name
        assert all(np.isfinite(x).all() for x in b), name
        bad = [i for i, (x, y) in enumerate(zip(a, b)) if not np.array_equal(x, y)]
        assert not bad, (name, bad[:8])


def test_elementwise_chains_are_one_launch_and_bit_identical(pkg, be):
    """k_ew_chain: Token2Wav's Mish spelling (sub / exp / exp / add / log / tanh / mul) and a DiT-style modulation (mul by a row vector, add, add a row vector, scale, leaky_relu)
    over [512, 56]: with fusion on the runs collapse into chain launches, and every value equals the one-launch-per-node result bit for bit (-ffp-contract=off: nothing fuses
    across the ops)."""
    from llama_cpp_omni_amd import token2wav as T
    from llama_cpp_omni_amd.ggml import UNARY
    rng = np.random.default_rng(31)
    res = {}
    for fusion in (0, 1):
        be.set_option("fusion", fusion)
        c = pkg.Context(be)
        x = c.new_tensor(pkg.GGML_TYPE_F32, 512, 56, 1)
        sc = c.new_tensor(pkg.GGML_TYPE_F32, 512, 1, 1); sh = c.new_tensor(pkg.GGML_TYPE_F32, 512, 1, 1)
        m = T.mish(c, x)                                               # 7 nodes
        y = c.add(c.add(m, c.mul(m, sc)), sh)                          # modulate: the first add reads m twice -> a chain boundary
        z = c.leaky_relu(c.scale(y, 0.5, 0.25), 0.1) if hasattr(c, "leaky_relu") else c.scale(y, 0.5, 0.25)
        out = c.unary(z, UNARY.TANH)
        keep = c.scale(out, 1.0)                                       # (a plain reader so that `out` is materialised whatever follows)
        c.alloc()
        rs = np.random.default_rng(32)
        be.tensor_set(x, rs.standard_normal(512 * 56).astype(np.float32))
        be.tensor_set(sc, (rs.standard_normal(512) * 0.2).astype(np.float32)); be.tensor_set(sh, (rs.standard_normal(512) * 0.2).astype(np.float32))
        be.graph_compute(c.graph())
        res[fusion] = (be.tensor_get(keep).copy(), int(be.get_stat("kernels_last_graph")))
        c.free()
    be.set_option("fusion", 1)
    (a, ka), (b, kb) = res[0], res[1]
    print(f"element-wise graph: {ka} launches one per node, {kb} with chains")
    assert np.isfinite(a).all() and np.array_equal(a, b)
    assert kb <= ka - 6, (ka, kb)
