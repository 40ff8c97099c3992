"""Host side of the state-space path (no GPU): the constructors Context.ssm_conv / Context.ssm_scan give the reference's result shapes and reject what
ggml.c:5165-5235 rejects, and one `mamba2` and one `mamba` layer of llama.cpp-omni_amd/mamba.py, run on the reference CPU backend (oracle/_ref), equal a NumPy
float64 restatement of the layer written here: conv, SiLU, soft-plus, scan, skip, gate, grouped norm.  The bar is NMSE <= 1e-10 -- the reference in f32 (F32
weights: no quantisation stage) against exact arithmetic, as the f64 restatements of tests/test_round5_gpu.py."""
import numpy as np
import pytest

from conftest import nmse

F32, F16, I32 = 0, 1, 26


# ------------------------------------------------------------------------------------------------ constructors
def _scan_operands(g, d_state=16, head_dim=4, n_head=6, n_group=2, n_t=3, n_s=2, n_rows=5):
    s = g.new_tensor(F32, d_state, head_dim, n_head, n_rows)
    x = g.new_tensor(F32, head_dim, n_head, n_t, n_s)
    dt = g.new_tensor(F32, n_head, n_t, n_s)
    A = g.new_tensor(F32, 1, n_head)
    B = g.new_tensor(F32, d_state, n_group, n_t, n_s)
    C_ = g.new_tensor(F32, d_state, n_group, n_t, n_s)
    ids = g.new_tensor(I32, n_s)
    return [s, x, dt, A, B, C_, ids]


def test_ssm_conv_constructor(pkg):
    g = pkg.Context(None)
    y = g.ssm_conv(g.new_tensor(F32, 3 + 7, 200, 2), g.new_tensor(F32, 4, 200))
    assert y.ne == (200, 7, 2, 1) and y.type == F32 and y.t.op == pkg.OP.SSM_CONV == 71
    with pytest.raises(AssertionError):
        g.ssm_conv(g.new_tensor(F32, 10, 200, 2), g.new_tensor(F32, 4, 100))               # sx->ne[1] == d_inner
    with pytest.raises(AssertionError):
        g.ssm_conv(g.new_tensor(F32, 10, 200, 2, 2), g.new_tensor(F32, 4, 200))            # sx is 3-D
    with pytest.raises(AssertionError):
        g.ssm_conv(g.new_tensor(F32, 10, 200, 2), g.new_tensor(F32, 4, 200, 2))            # c is a matrix


def test_ssm_scan_constructor(pkg):
    g = pkg.Context(None)
    ops = _scan_operands(g)
    y = g.ssm_scan(*ops)
    assert y.ne == (4 * 6 * 3 * 2 + 16 * 4 * 6 * 2, 1, 1, 1) and y.type == F32 and y.t.op == pkg.OP.SSM_SCAN == 72
    assert [bool(y.t.src[i]) for i in range(8)] == [True] * 7 + [False]                    # seven sources
    per_state = list(ops)
    per_state[3] = g.new_tensor(F32, 16, 6)                                                # Mamba-1: one decay per state element
    assert g.ssm_scan(*per_state).ne[0] == y.ne[0]
    bad = list(ops); bad[6] = g.new_tensor(F32, 2)                                         # ids must be I32
    with pytest.raises(AssertionError):
        g.ssm_scan(*bad)
    bad = list(ops); bad[5] = g.new_tensor(F32, 16, 1, 3, 2)                               # B and C of different shape
    with pytest.raises(AssertionError):
        g.ssm_scan(*bad)
    bad = list(ops); bad[3] = g.new_tensor(F32, 8, 6)                                      # A->ne[0] neither 1 nor d_state
    with pytest.raises(AssertionError):
        g.ssm_scan(*bad)
    bad = list(ops); bad[2] = g.new_tensor(F32, 6, 3, 3)                                   # dt->ne[2] == n_seqs
    with pytest.raises(AssertionError):
        g.ssm_scan(*bad)
    wide = g.new_tensor(F32, 6 * 4 + 8, 3, 2)                                              # x as a view with strided tokens: taken; with strided head rows: refused
    ok = list(ops); ok[1] = g.view_4d(wide, 4, 6, 3, 2, 16, wide.nb[1], wide.nb[2], 0)
    assert g.ssm_scan(*ok).ne[0] == y.ne[0]
    bad = list(ops); bad[1] = g.view_4d(wide, 4, 6, 3, 2, 20, wide.nb[1], wide.nb[2], 0)
    with pytest.raises(AssertionError):
        g.ssm_scan(*bad)


def test_layer_node_sequence(pkg):
    """the order ggml_build_forward_expand gives the reference's builders: zeroing SCALE, GET_ROWS on the states, the extra-state copy, the conv-state and
    ssm-state write-backs in front of what follows them"""
    from llama_cpp_omni_amd import mamba
    OP = pkg.OP
    for hp in (mamba.TINY_MAMBA2, mamba.TINY_MAMBA):
        g = pkg.Context(None)
        x = g.new_tensor(F32, hp["n_embd"], 5)
        s_copy = g.new_tensor(I32, 2)
        rs = dict(copy_main=g.view_1d(s_copy, 1, 0), copy_extra=g.view_1d(s_copy, 1, 4), n_rs=2, head=1, size=3, zero=1)
        names = ["ssm_in", "ssm_conv1d", "ssm_conv1d_b", "ssm_x", "ssm_dt", "ssm_dt_b", "ssm_a", "ssm_d", "ssm_norm", "ssm_out"]
        m2 = hp["arch"] == "mamba2"
        DI, DS, R, G, E = hp["d_inner"], hp["d_state"], hp["dt_rank"], hp["n_group"], hp["n_embd"]
        sh = (dict(ssm_in=(E, 2 * DI + 2 * G * DS + R), ssm_conv1d=(4, DI + 2 * G * DS), ssm_conv1d_b=(DI + 2 * G * DS,), ssm_dt_b=(R,), ssm_a=(1, R), ssm_d=(1, R), ssm_norm=(DI // G, G), ssm_out=(DI, E)) if m2 else
              dict(ssm_in=(E, 2 * DI), ssm_conv1d=(4, DI), ssm_conv1d_b=(DI,), ssm_x=(DI, R + 2 * DS), ssm_dt=(R, DI), ssm_dt_b=(DI,), ssm_a=(DS, DI), ssm_d=(DI,), ssm_out=(DI, E)))
        L = {k: g.new_tensor(F32, *sh[k]) for k in names if k in sh}
        conv_all, ssm_all = g.new_tensor(F32, mamba.n_embd_r(hp) * 3), g.new_tensor(F32, mamba.n_embd_s(hp) * 3)
        roots = []
        out, N = (mamba.build_mamba2_layer if m2 else mamba.build_mamba_layer)(g, x, L, conv_all, ssm_all, rs, hp, 5, 1, roots)
        roots.append(out)
        ops = [n.t.op for n in g.graph_expand(roots).nodes]
        real = [o for o in ops if o not in (OP.RESHAPE, OP.VIEW, OP.TRANSPOSE, OP.PERMUTE)]
        head = [OP.SCALE, OP.GET_ROWS, OP.GET_ROWS, OP.CPY, OP.MUL_MAT, OP.CONCAT, OP.CPY]     # conv states: zero, rows, extra copy; projection; conv_x; conv-state write-back
        assert real[:7] == head, real
        if m2:
            tail = [OP.SCALE, OP.SSM_CONV, OP.ADD, OP.UNARY, OP.CONT, OP.ADD, OP.SSM_SCAN, OP.GET_ROWS, OP.CPY, OP.CPY, OP.CONT, OP.MUL, OP.ADD, OP.GLU, OP.RMS_NORM, OP.MUL, OP.MUL_MAT]
        else:
            tail = [OP.SCALE, OP.SSM_CONV, OP.ADD, OP.UNARY, OP.MUL_MAT, OP.MUL_MAT, OP.ADD, OP.SSM_SCAN, OP.GET_ROWS, OP.CPY, OP.CPY, OP.CONT, OP.MUL, OP.ADD, OP.GLU, OP.MUL_MAT]
        assert real[7:] == tail, real
        scan = N["ssm_scan"]
        assert scan._srcs[6] is rs["copy_main"] and scan.ne[0] == DI * 5 + DS * DI


# ------------------------------------------------------------------------------------------------ a layer on the reference CPU backend against float64
def _silu(v):
    return v / (1.0 + np.exp(-v))


def _softplus(v):
    return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))


def _layer_f64(hp, W, xs, conv_state, ssm_state):
    """-> (out [n_t, n_embd], new conv state [d_xbc, d_conv - 1], new ssm state [n_head, head_dim, d_state]); every array float64"""
    DI, DS, DC, R, G, eps = hp["d_inner"], hp["d_state"], hp["d_conv"], hp["dt_rank"], hp["n_group"], hp["eps"]
    m2 = hp["arch"] == "mamba2"
    n_t = xs.shape[0]
    proj = xs @ W["ssm_in"].T
    if m2:
        d_xbc = DI + 2 * G * DS
        z, xBC, dt = proj[:, :DI], proj[:, DI:DI + d_xbc], proj[:, DI + d_xbc:]
    else:
        d_xbc = DI
        xBC, z = proj[:, :DI], proj[:, DI:]
    cx = np.concatenate([conv_state, xBC.T], axis=1)                                     # [d_xbc, d_conv - 1 + n_t]
    conv = np.stack([(cx[:, t:t + DC] * W["ssm_conv1d"]).sum(1) for t in range(n_t)])      # [n_t, d_xbc]
    xBC = _silu(conv + W["ssm_conv1d_b"].reshape(-1))
    if m2:
        n_head, head_dim = R, DI // R
        x, B, C_ = xBC[:, :DI].reshape(n_t, n_head, head_dim), xBC[:, DI:DI + G * DS].reshape(n_t, G, DS), xBC[:, DI + G * DS:].reshape(n_t, G, DS)
        dt = dt + W["ssm_dt_b"].reshape(-1)
        A = np.broadcast_to(W["ssm_a"].reshape(n_head, 1), (n_head, DS))
        D = W["ssm_d"].reshape(n_head, 1)
    else:
        n_head, head_dim = DI, 1
        x_db = xBC @ W["ssm_x"].T
        dt, B, C_ = x_db[:, :R], x_db[:, R:R + DS].reshape(n_t, 1, DS), x_db[:, R + DS:].reshape(n_t, 1, DS)
        if hp.get("dt_b_c_rms"):
            rms = lambda v, w: v / np.sqrt((v ** 2).mean(-1, keepdims=True) + eps) * w.reshape(-1)
            dt, B, C_ = rms(dt, W["ssm_dt_norm"]), rms(B, W["ssm_b_norm"]), rms(C_, W["ssm_c_norm"])
        dt = dt @ W["ssm_dt"].T + W["ssm_dt_b"].reshape(-1)
        x = xBC.reshape(n_t, n_head, 1)
        A = W["ssm_a"]
        D = W["ssm_d"].reshape(n_head, 1)
    state = ssm_state.copy()
    y = np.zeros((n_t, n_head, head_dim))
    grp = np.arange(n_head) // (n_head // G)
    for t in range(n_t):
        dsp = _softplus(dt[t])                                                           # [n_head]
        dA = np.exp(dsp[:, None] * A)                                                    # [n_head, d_state]
        state = state * dA[:, None, :] + B[t][grp][:, None, :] * (x[t] * dsp[:, None])[:, :, None]
        y[t] = (state * C_[t][grp][:, None, :]).sum(-1)
    y = y + x * D[None]
    y = (_silu(z) * y.reshape(n_t, DI))
    if m2:
        yg = y.reshape(n_t, G, DI // G)
        y = (yg / np.sqrt((yg ** 2).mean(-1, keepdims=True) + eps) * W["ssm_norm"]).reshape(n_t, DI)
    return y @ W["ssm_out"].T, cx[:, n_t:], state


@pytest.mark.parametrize("arch,rms", [("mamba2", False), ("mamba", False), ("mamba", True)])
def test_layer_on_reference_backend_equals_float64(pkg, ref_be, arch, rms):
    from llama_cpp_omni_amd import mamba
    hp = dict(mamba.TINY_MAMBA2 if arch == "mamba2" else mamba.TINY_MAMBA, dt_b_c_rms=rms)
    lay = mamba.MambaLayer(ref_be, hp, rs_size=3, seed=8, in_type=F32, out_type=F32, x_type=F32)
    W = {k: np.asarray(v, np.float64) for k, v in lay.weights.items()}
    DI, DS, DC = hp["d_inner"], hp["d_state"], hp["d_conv"]
    n_r, n_s_ = mamba.n_embd_r(hp), mamba.n_embd_s(hp)
    d_xbc = n_r // (DC - 1)
    n_head = hp["dt_rank"] if arch == "mamba2" else DI
    conv_state, ssm_state = np.zeros((d_xbc, DC - 1)), np.zeros((n_head, DI // n_head, DS))      # the sequence's row is zeroed in the first step
    rng = np.random.default_rng(2)
    for step, (n_t, rs_zero) in enumerate([(5, 1), (1, -1)]):
        xv = rng.standard_normal((n_t, hp["n_embd"])).astype(np.float32)
        g, x, s_copy, N = lay.build(n_t, 1, n_rs=2, rs_head=1, rs_zero=rs_zero)
        ref_be.tensor_set(x, xv)
        ref_be.tensor_set(s_copy, np.array([1, 0], np.int32))
        ref_be.graph_compute(g.graph())
        out = ref_be.tensor_get(N["out"]).copy().reshape(n_t, hp["n_embd"])
        conv_all = ref_be.tensor_get(lay.conv_states).copy().reshape(3, n_r)
        ssm_all = ref_be.tensor_get(lay.ssm_states).copy().reshape(3, n_s_)
        g.free()
        want, conv_state, ssm_state = _layer_f64(hp, W, xv.astype(np.float64), conv_state, ssm_state)
        e = nmse(out, want)
        assert e <= 1e-10, f"{arch} step {step}: NMSE {e:.3e}"
        assert nmse(conv_all[1], conv_state) <= 1e-10 and nmse(ssm_all[1], ssm_state) <= 1e-10
        assert np.array_equal(conv_all[0], W["conv_states"].reshape(3, n_r)[0].astype(np.float32))          # row 0: nobody's
        assert np.array_equal(conv_all[2], conv_all[0]) and np.array_equal(ssm_all[2], ssm_all[0])           # the extra-state copy: row s_copy[1] = 0 onto row head + n_seqs = 2
    lay.wctx.free()


# ------------------------------------------------------------------------------------------------ the GGUF fixtures of tools/make_synth_mamba_gguf.py on the reference CPU backend
import json          # noqa: E402
import os            # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
N_STEPS, V = 32, 512
PROMPT = [(7 * i + 3) % V for i in range(33)]                                              # (tests/test_ssm_model_gpu.py decodes the same prompt)


@pytest.fixture(scope="module", params=["mamba2", "mamba"])
def mamba_gguf(request, tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp(request.param)
    gguf = str(d / f"tiny-{request.param}.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_mamba_gguf.py"), "--arch", request.param, "-o", gguf], check=True, timeout=300, capture_output=True)
    pfile = str(d / "prompt.bin")
    np.asarray(PROMPT, np.int32).tofile(pfile)
    return request.param, gguf, pfile, str(d)


def _cpu(gguf, n, extra):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    out = subprocess.run([BIN, "-m", gguf, "-ngl", "0", "--greedy", str(n), "-t", "4"] + extra, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"]


def test_gguf_loads_in_the_reference_cpu_backend(mamba_gguf):
    arch, gguf, _, _ = mamba_gguf
    ids = _cpu(gguf, 16, [])
    assert len(ids) == 16 and all(0 <= i < V for i in ids)


@pytest.mark.parametrize("start", ["one_token", "prompt33"])
def test_gguf_logit_margins_carry_an_arg_max_check(mamba_gguf, start):
    """at least 29 of the 32 teacher-forced steps have a CPU top-1 / top-2 logit margin above 1e-3 x max|logit|: what the GPU test's arg-max comparison relies on"""
    arch, gguf, pfile, d = mamba_gguf
    dump = os.path.join(d, f"cpu_{start}.bin")
    ids = _cpu(gguf, N_STEPS, (["--start-token", "1"] if start == "one_token" else ["--prompt-file", pfile]) + ["--dump-all-logits", dump])
    lg = np.fromfile(dump, np.float32).reshape(N_STEPS, V)
    assert np.isfinite(lg).all() and [int(x) for x in lg.argmax(1)] == ids
    top = np.sort(lg, axis=1)
    wide = (top[:, -1] - top[:, -2]) > 1e-3 * np.abs(lg).max(axis=1)
    assert wide.sum() >= 29, (arch, start, int(wide.sum()))
