"""Host side of the linear-attention path (no GPU): the constructors Context.rwkv_wkv6 / gated_linear_attn / rwkv_wkv7 / l2_norm give the reference's op numbers,
source counts and result shapes ({S * H, n_tokens + S * n_seqs}: the outputs, then the new states) and reject what ggml.c:5369-5499 rejects; and the rwkv6 (fused and
separate lerp weights), qrwkv (GATED_LINEAR_ATTN) and rwkv7 (first layer with gating, later layer with the value residual) time-mix layers of llama.cpp-omni_amd/rwkv.py,
run on the reference CPU backend (oracle/_ref), equal a NumPy float64 restatement written here, at the NMSE <= 1e-10 of tests/test_ssm_host.py."""
import pytest

F32, F16 = 0, 1


def _ops(g, S=8, H=3, T=6, n_seqs=2, ty=F32):
    t3 = lambda: g.new_tensor(ty, S, H, T)
    return t3, g.new_tensor(ty, S * S * H, n_seqs)


def test_op_numbers(pkg):
    OP = pkg.OP
    assert (OP.L2_NORM, OP.RWKV_WKV6, OP.GATED_LINEAR_ATTN, OP.RWKV_WKV7) == (27, 77, 78, 79)      # ggml.h:491, 541-543


def test_rwkv_wkv6_constructor(pkg):
    g = pkg.Context(None)
    t3, state = _ops(g)
    y = g.rwkv_wkv6(t3(), t3(), t3(), g.new_tensor(F32, 8, 3), t3(), state)
    assert y.ne == (24, 6 + 8 * 2, 1, 1) and y.type == F32 and y.t.op == pkg.OP.RWKV_WKV6
    assert [bool(y.t.src[i]) for i in range(8)] == [True] * 6 + [False] * 2
    y = g.rwkv_wkv6(t3(), t3(), t3(), g.new_tensor(F32, 8, 3), t3(), g.new_tensor(F32, 8, 2, 8, 3))      # a 4-D state {S, n_seqs, S, H}: the loader's probe
    assert y.ne == (24, 6 + 8 * 2, 1, 1)
    with pytest.raises(AssertionError):
        g.rwkv_wkv6(t3(), g.new_tensor(F32, 8, 3, 5), t3(), g.new_tensor(F32, 8, 3), t3(), state)       # v->ne[2] == n_tokens
    with pytest.raises(AssertionError):
        g.rwkv_wkv6(t3(), t3(), t3(), g.new_tensor(F32, 8, 3), t3(), g.new_tensor(F32, 8 * 8 * 3 + 1, 2))      # nelements(state) == S * S * H * n_seqs
    wide = g.new_tensor(F32, 16, 3, 6)
    with pytest.raises(AssertionError):
        g.rwkv_wkv6(g.view_3d(wide, 8, 3, 6, wide.nb[1], wide.nb[2], 0), t3(), t3(), g.new_tensor(F32, 8, 3), t3(), state)      # k is contiguous


def test_gated_linear_attn_constructor(pkg):
    g = pkg.Context(None)
    t3, state = _ops(g)
    y = g.gated_linear_attn(t3(), t3(), t3(), t3(), state, 0.125)
    assert y.ne == (24, 6 + 8 * 2, 1, 1) and y.type == F32 and y.t.op == pkg.OP.GATED_LINEAR_ATTN
    assert [bool(y.t.src[i]) for i in range(8)] == [True] * 5 + [False] * 3
    import struct
    assert struct.unpack("<f", struct.pack("<i", y.t.op_params[0]))[0] == 0.125
    with pytest.raises(AssertionError):
        g.gated_linear_attn(t3(), t3(), t3(), g.new_tensor(F32, 8, 2, 6), state, 0.125)                 # g->ne[1] == H
    with pytest.raises(AssertionError):
        g.gated_linear_attn(t3(), t3(), t3(), t3(), g.new_tensor(F32, 8 * 8 * 3, 2, 2), 0.125)          # nelements(state)


def test_rwkv_wkv7_constructor(pkg):
    g = pkg.Context(None)
    t3, state = _ops(g)
    y = g.rwkv_wkv7(t3(), t3(), t3(), t3(), t3(), t3(), state)
    assert y.ne == (24, 6 + 8 * 2, 1, 1) and y.type == F32 and y.t.op == pkg.OP.RWKV_WKV7
    assert [bool(y.t.src[i]) for i in range(8)] == [True] * 7 + [False]
    with pytest.raises(AssertionError):
        g.rwkv_wkv7(t3(), t3(), t3(), t3(), t3(), g.new_tensor(F32, 4, 3, 6), state)                    # b->ne[0] == S
    with pytest.raises(AssertionError):
        g.rwkv_wkv7(t3(), g.new_tensor(F32, 8, 3, 7), t3(), t3(), t3(), t3(), state)                    # w->ne[2] == n_tokens


def test_l2_norm_constructor(pkg):
    g = pkg.Context(None)
    x = g.new_tensor(F32, 64, 5, 4, 3)
    y = g.l2_norm(x, 1e-12)
    assert y.ne == x.ne and y.type == F32 and y.t.op == pkg.OP.L2_NORM and bool(y.t.src[0]) and not bool(y.t.src[1])
    wide = g.new_tensor(F32, 200, 5)
    v = g.l2_norm(g.view_2d(wide, 64, 5, wide.nb[1], 32), 1e-12)                                        # a strided source: the result is dense
    assert v.ne == (64, 5, 1, 1) and v.nb[1] == 256


# ------------------------------------------------------------------------------------------------ time-mix layers on the reference CPU backend against float64
import numpy as np          # noqa: E402

from conftest import nmse   # noqa: E402


@pytest.fixture(scope="module")
def ref2(pkg):
    """the reference CPU backend with two threads: its WKV6 / GLA kernels never return with more threads than heads (ops.cpp:9192, :9215; 4 heads here)"""
    from oracle.ref_backend import make_ref_cpu_backend, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libggml-ref.so not built (needs the reference sources at build time)")
    return make_ref_cpu_backend(pkg, 2)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _ln(v, w, b, eps):
    m = v.mean(-1, keepdims=True)
    return (v - m) / np.sqrt(((v - m) ** 2).mean(-1, keepdims=True) + eps) * w.reshape(-1) + b.reshape(-1)


def _time_mix_f64(hp, W, x, shift, state, v_first):
    """-> (time-mix output [T, E], new wkv state [H, S, S]); x [T, E] one sequence, shift [E] the att token-shift row, state [H, S, S]; every array float64"""
    E, S = hp["n_embd"], hp["head_size"]
    H, T = E // S, x.shape[0]
    att = _ln(x, W["attn_norm"], W["attn_norm_b"], 1e-5)
    sx = np.concatenate([shift[None], att[:-1]]) - att
    s = state.copy()
    out = np.zeros((T, H, S))
    if hp["arch"] == "rwkv6":
        xxx = att + sx * W["time_mix_lerp_x"].reshape(-1)
        TM = hp["time_mix_extra"]
        t = np.tanh(xxx @ W["time_mix_w1"].T).reshape(T, 5, TM)
        w2 = W["time_mix_w2"].reshape(5, E, TM)
        lerp = W["time_mix_lerp_fused"] if hp["fused"] else np.concatenate([W["time_mix_lerp_" + n] for n in "wkvrg"])
        xw, xk, xv, xr, xg = (att + sx * (t[:, i] @ w2[i].T + lerp[i]) for i in range(5))
        r, k, v = xr @ W["time_mix_receptance"].T, xk @ W["time_mix_key"].T, xv @ W["time_mix_value"].T
        g = xg @ W["time_mix_gate"].T
        g = _sig(g) if hp["qrwkv"] else g * _sig(g)
        w = np.exp(-np.exp(np.tanh(xw @ W["time_mix_decay_w1"].T) @ W["time_mix_decay_w2"].T + W["time_mix_decay"].reshape(-1)))
        if hp["qrwkv"]:
            k = k * (1.0 - w)
        r, k, v, w = (a.reshape(T, H, S) for a in (r, k, v, w))
        for t_ in range(T):
            for h in range(H):
                kv = np.outer(k[t_, h], v[t_, h])
                if hp["qrwkv"]:
                    s[h] = s[h] * w[t_, h][:, None] + kv
                    out[t_, h] = (r[t_, h] * S ** -0.5) @ s[h]
                else:
                    out[t_, h] = r[t_, h] @ (W["time_mix_first"][h][:, None] * kv + s[h])
                    s[h] = s[h] * w[t_, h][:, None] + kv
        if not hp["qrwkv"]:
            out = _ln(out, np.ones(1), np.zeros(1), 64e-5)
            out = out.reshape(T, E) * W["time_mix_ln"].reshape(-1) + W["time_mix_ln_b"].reshape(-1)
        return (out.reshape(T, E) * g) @ W["time_mix_output"].T, s
    lerp = W["time_mix_lerp_fused"]
    xr, xw, xk, xv, xa = (att + sx * lerp[i] for i in range(5))
    r = xr @ W["time_mix_receptance"].T
    w = np.exp(-0.606531 * _sig(np.tanh(xw @ W["time_mix_w1"].T) @ W["time_mix_w2"].T + W["time_mix_w0"].reshape(-1)))
    k, v = xk @ W["time_mix_key"].T, xv @ W["time_mix_value"].T
    if not hp["first"]:
        v = v + (v_first - v) * _sig((xv @ W["time_mix_v1"].T) @ W["time_mix_v2"].T + W["time_mix_v0"].reshape(-1))
    g = _sig((att + sx * lerp[5]) @ W["time_mix_g1"].T) @ W["time_mix_g2"].T if hp["gating"] else None
    a = _sig((xa @ W["time_mix_a1"].T) @ W["time_mix_a2"].T + W["time_mix_a0"].reshape(-1))
    kk = (k * W["time_mix_k_k"].reshape(-1)).reshape(T, H, S)
    kk = kk / np.maximum(np.sqrt((kk ** 2).sum(-1, keepdims=True)), 1e-12)
    ka = k * W["time_mix_k_a"].reshape(-1)
    k = k + a * ka - ka
    r, w, k, v, a = (q.reshape(T, H, S) for q in (r, w, k, v, a))
    for t_ in range(T):
        for h in range(H):
            sa = s[h] @ -kk[t_, h]
            s[h] = s[h] * w[t_, h][None, :] + np.outer(v[t_, h], k[t_, h]) + np.outer(sa, kk[t_, h] * a[t_, h])
            out[t_, h] = s[h] @ r[t_, h]
    out = _ln(out, np.ones(1), np.zeros(1), 64e-5).reshape(T, E) * W["time_mix_ln"].reshape(-1) + W["time_mix_ln_b"].reshape(-1)
    rk = (k * r * W["time_mix_r_k"].reshape(H, S)).sum(-1, keepdims=True)
    out = out + (v * rk).reshape(T, E)
    if g is not None:
        out = out * g
    return out @ W["time_mix_output"].T, s


LAYERS = {"rwkv6": dict(fused=True, qrwkv=False), "rwkv6_separate": dict(fused=False, qrwkv=False), "qrwkv": dict(fused=True, qrwkv=True),
          "rwkv7": dict(first=True, gating=True), "rwkv7_later_ungated": dict(first=False, gating=False)}
# measured on the reference CPU backend (f32) at these shapes: time-mix output NMSE 4e-14 .. 2e-13, wkv state 1e-14 .. 7e-14: f32 alone stays within the 1e-10 of test_ssm_host.py
LAYER_BAR = 1e-10


@pytest.mark.parametrize("n_t", [1, 5])
@pytest.mark.parametrize("variant", list(LAYERS))
def test_time_mix_layer_on_reference_backend_equals_float64(pkg, ref2, variant, n_t):
    """one time-mix layer of rwkv.py (F32 weights: no quantisation stage) on the reference CPU backend against the float64 restatement above; bar: LAYER_BAR"""
    from llama_cpp_omni_amd import rwkv
    hp = dict(rwkv.TINY_RWKV7 if variant.startswith("rwkv7") else rwkv.TINY_RWKV6, **LAYERS[variant])
    E, S = hp["n_embd"], hp["head_size"]
    lay = rwkv.RwkvLayer(ref2, hp, rs_size=3, seed=8)
    W = {k: np.asarray(v, np.float64) for k, v in lay.weights.items()}
    rng = np.random.default_rng(3 + n_t)
    xv, vf = rng.standard_normal((n_t, E)).astype(np.float32), rng.standard_normal((n_t, E)).astype(np.float32)
    g, x, s_copy, v_first, N = lay.build(n_t, 1, n_rs=2, rs_head=1, rs_zero=-1)
    ref2.tensor_set(x, xv)
    if v_first is not None:
        ref2.tensor_set(v_first, vf)
    ref2.tensor_set(s_copy, np.array([1, 0], np.int32))
    ref2.graph_compute(g.graph())
    got = ref2.tensor_get(N["time_mix"]).copy().reshape(n_t, E)
    s_all = ref2.tensor_get(lay.s_states).copy().reshape(3, E * S)
    r_all = ref2.tensor_get(lay.r_states).copy().reshape(3, 2, E)
    g.free()
    lay.wctx.free()
    want, s_new = _time_mix_f64(hp, W, xv.astype(np.float64), W["r_states"].reshape(3, 2, E)[1, 0], W["s_states"].reshape(3, E // S, S, S)[1], vf.astype(np.float64))
    e_o, e_s = nmse(got, want), nmse(s_all[1], s_new)
    print(f"{variant} n_t={n_t}: time-mix NMSE {e_o:.3e}, wkv state NMSE {e_s:.3e}")
    assert e_o <= LAYER_BAR and e_s <= LAYER_BAR, (variant, e_o, e_s)
    att = _ln(xv.astype(np.float64), W["attn_norm"], W["attn_norm_b"], 1e-5)
    assert nmse(r_all[1, 0], att[-1]) <= LAYER_BAR                                       # the token-shift write-back: the last token's attn_norm row
    assert np.array_equal(s_all[0], lay.weights["s_states"].reshape(3, E * S)[0]) and np.array_equal(s_all[2], s_all[0])      # row 0 untouched, copied onto row 2


# ------------------------------------------------------------------------------------------------ the GGUF fixtures of tools/make_synth_rwkv_gguf.py on the reference CPU backend
import json          # noqa: E402
import os            # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
N_STEPS, V = 32, 512
PROMPT = [(7 * i + 3) % V for i in range(33)]                                              # (tests/test_rwkv_model_gpu.py decodes the same prompt)


@pytest.fixture(scope="module", params=["rwkv6", "rwkv7"])
def rwkv_gguf(request, tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp(request.param)
    gguf = str(d / f"tiny-{request.param}.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_rwkv_gguf.py"), "--arch", request.param, "-o", gguf], check=True, timeout=300, capture_output=True)
    pfile = str(d / "prompt.bin")
    np.asarray(PROMPT, np.int32).tofile(pfile)
    return request.param, gguf, pfile, str(d)


def _cpu(gguf, n, extra):
    """-t 4: the fixtures have 4 heads, and the reference's WKV6 kernel never returns with more threads than heads"""
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    out = subprocess.run([BIN, "-m", gguf, "-ngl", "0", "--greedy", str(n), "-t", "4"] + extra, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"]


def test_gguf_loads_in_the_reference_cpu_backend(rwkv_gguf):
    arch, gguf, _, _ = rwkv_gguf
    ids = _cpu(gguf, 16, [])
    assert len(ids) == 16 and all(0 <= i < V for i in ids)


@pytest.mark.parametrize("start", ["one_token", "prompt33"])
def test_gguf_logit_margins_carry_an_arg_max_check(rwkv_gguf, start):
    """at least 29 of the 32 teacher-forced steps have a CPU top-1 / top-2 logit margin above 1e-3 x max|logit|: what the GPU test's arg-max comparison relies on"""
    arch, gguf, pfile, d = rwkv_gguf
    dump = os.path.join(d, f"cpu_{start}.bin")
    ids = _cpu(gguf, N_STEPS, (["--start-token", "1"] if start == "one_token" else ["--prompt-file", pfile]) + ["--dump-all-logits", dump])
    lg = np.fromfile(dump, np.float32).reshape(N_STEPS, V)
    assert np.isfinite(lg).all() and [int(x) for x in lg.argmax(1)] == ids
    top = np.sort(lg, axis=1)
    wide = (top[:, -1] - top[:, -2]) > 1e-3 * np.abs(lg).max(axis=1)
    assert wide.sum() >= 29, (arch, start, int(wide.sum()))
