"""RWKV layers on the GPU (`-m gpu`): the rwkv6 (fused and separate lerp weights), qrwkv (GATED_LINEAR_ATTN) and rwkv7 (first layer with gating; later layer with the
value residual, without gating) layers of llama.cpp-omni_amd/rwkv.py -- time mix, channel mix, token shift and both state write-backs -- through the backend C-ABI
against the reference CPU backend (oracle/ref_backend.py) on the same graph.

Bars, as tests/test_ssm_ops_gpu.py: NMSE <= 1e-6 for the layer output and for the channel mixes run as graphs of their own, and <= 1e-7 for the written-back wkv and token-shift
states.  The layers' projections are F32: the 1e-6 bar of test_ssm_ops_gpu.py rests on both sides running the same integer stages, which holds only while every activation
quantises to the same int8 on both -- measured here with Q4_K / Q6_K projections, a 5-token rwkv6 input had ONE Q8_K rounding of time_mix_gate's activation fall the other
way (its source differs in the last f32 bit between the backends), which put token 0's gate 1.8e-6 and the layer output 2.3e-5 off while all 28 other cases stood at 1e-13.
The quantised projections of these layers are covered at their own bar (5e-4) by tests/test_rwkv_model_gpu.py; the stand-alone channel mixes keep Q4_K / Q6_K.  Only graph results and
the caches are read back: the executor does not write an interior node that a fusion swallowed.  Each layer runs at 1 and 5
tokens per sequence and at 1 and 2 sequences.  In these graphs every WKV / L2_NORM operand is made in the graph (NEG, MUL, EXP, reshaped MUL_MAT results), so the
executor's settling in front of the launch is live; one test submits a graph four times: eager, captured, replayed twice.

The reference CPU backend runs with two threads: its WKV6 / GLA kernels never return with more threads than heads (ops.cpp:9192, :9215; 4 heads here)."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

Q4_K, Q6_K = 12, 14
VARIANTS = {"rwkv6_fused": ("6", dict(fused=True, qrwkv=False)), "rwkv6_separate": ("6", dict(fused=False, qrwkv=False)), "qrwkv": ("6", dict(fused=True, qrwkv=True)),
            "rwkv7_first_gated": ("7", dict(first=True, gating=True)), "rwkv7_later_ungated": ("7", dict(first=False, gating=False))}


@pytest.fixture(scope="module")
def ref_be(pkg):
    from oracle.ref_backend import make_ref_cpu_backend, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libggml-ref.so not built (needs the reference sources at build time)")
    return make_ref_cpu_backend(pkg, 2)


def _hp(variant):
    from llama_cpp_omni_amd import rwkv
    arch, over = VARIANTS[variant]
    return dict(rwkv.TINY_RWKV6 if arch == "6" else rwkv.TINY_RWKV7, **over)


def _steps(b_, lay, n_t, n_s, inputs, repeats=1):
    """the layer graph for n_s sequences of n_t tokens continuing rows 1.. of the caches (row 0 is copied onto the row behind them), submitted `repeats` times with the
    caches reset in between -> [(out, token-shift cache, wkv cache)]"""
    res = []
    g, x, s_copy, v_first, N = lay.build(n_t, n_s, n_rs=n_s + 1, rs_head=1, rs_zero=-1)
    graph = g.graph()
    for _ in range(repeats):
        b_.tensor_set(lay.r_states, lay.weights["r_states"])
        b_.tensor_set(lay.s_states, lay.weights["s_states"])
        b_.tensor_set(x, inputs["x"])
        if v_first is not None:
            b_.tensor_set(v_first, inputs["v_first"])
        b_.tensor_set(s_copy, np.array(list(range(1, n_s + 1)) + [0], np.int32))
        b_.graph_compute(graph)
        res.append(tuple(b_.tensor_get(t).copy() for t in (N["out"], lay.r_states, lay.s_states)))
    g.free()
    return res


def _compare(got, want, what):
    names = ("layer output", "token-shift states", "wkv states")
    errs = [nmse(a, b) for a, b in zip(got, want)]
    print(f"{what}: NMSE " + ", ".join(f"{n} {e:.3e}" for n, e in zip(names, errs)))
    assert all(np.isfinite(a).all() for a in got)
    for n, e, bar in zip(names, errs, (1e-6, 1e-7, 1e-7)):
        assert e <= bar, f"{what}: {n} NMSE {e:.3e} > {bar}"


@pytest.mark.parametrize("n_s", [1, 2])
@pytest.mark.parametrize("n_t", [1, 5])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_layer(pkg, be, ref_be, variant, n_t, n_s):
    from llama_cpp_omni_amd import rwkv
    hp = _hp(variant)
    rng = np.random.default_rng(100 + 10 * n_t + n_s)
    inputs = dict(x=rng.standard_normal((n_t * n_s, hp["n_embd"])).astype(np.float32), v_first=rng.standard_normal((n_t * n_s, hp["n_embd"])).astype(np.float32))
    key = {"rwkv6_fused": "wkv6_launches", "rwkv6_separate": "wkv6_launches", "qrwkv": "gla_launches"}.get(variant, "wkv7_launches")
    res, weights = [], None
    for b_ in (ref_be, be):
        lay = rwkv.RwkvLayer(b_, hp, rs_size=4, seed=11, weights=weights)
        weights = lay.weights
        n0 = (be.get_stat(key), be.get_stat("l2_norm_launches"))
        res.append(_steps(b_, lay, n_t, n_s, inputs)[0])
        if b_ is be:
            assert be.get_stat(key) == n0[0] + 1
            assert be.get_stat("l2_norm_launches") == n0[1] + (1 if hp["arch"] == "rwkv7" else 0)
        lay.wctx.free()
    want, got = res
    _compare(got, want, f"{variant} n_t={n_t} n_s={n_s}")
    E, S = hp["n_embd"], hp["head_size"]
    r0, s0 = weights["r_states"].reshape(4, 2 * E), weights["s_states"].reshape(4, E * S)
    gr, gs = got[1].reshape(4, 2 * E), got[2].reshape(4, E * S)
    assert np.array_equal(gr[0], r0[0]) and np.array_equal(gs[0], s0[0])                               # row 0: nobody's
    assert np.array_equal(gr[1 + n_s], r0[0]) and np.array_equal(gs[1 + n_s], s0[0])                   # the extra-state copy: row 0 onto the row behind the sequences
    assert not np.array_equal(gs[1], s0[1]) and not np.array_equal(gr[1], r0[1])                       # the write-backs landed


@pytest.mark.parametrize("variant", ["rwkv6_fused", "qrwkv", "rwkv7_first_gated"])
def test_layer_eager_captured_replayed(pkg, be, ref_be, variant):
    """one decode-shaped layer graph submitted four times with the caches reset in between: eager, captured, replayed twice; every submission gives the reference's result"""
    from llama_cpp_omni_amd import rwkv
    hp = _hp(variant)
    rng = np.random.default_rng(7)
    inputs = dict(x=rng.standard_normal((1, hp["n_embd"])).astype(np.float32), v_first=None)
    lay = rwkv.RwkvLayer(ref_be, hp, rs_size=4, seed=12)
    weights = lay.weights
    want = _steps(ref_be, lay, 1, 1, inputs)[0]
    lay.wctx.free()
    lay = rwkv.RwkvLayer(be, hp, rs_size=4, seed=12, weights=weights)
    s0 = {k: be.get_stat(k) for k in ("graph_replays", "graph_captures")}
    got = _steps(be, lay, 1, 1, inputs, repeats=4)
    s1 = {k: be.get_stat(k) for k in s0}
    lay.wctx.free()
    for i, g_ in enumerate(got):
        _compare(g_, want, f"{variant} submission {i}")
    assert s1["graph_captures"] - s0["graph_captures"] == 1 and s1["graph_replays"] - s0["graph_replays"] == 2, (s0, s1)


@pytest.mark.parametrize("n_tokens", [1, 5, 10])
@pytest.mark.parametrize("arch", ["6", "7"])
def test_channel_mix(pkg, be, ref_be, arch, n_tokens):
    """build_rwkv6_channel_mix / build_rwkv7_channel_mix as a graph of its own: cur and x_prev {n_embd, n_tokens} in, the mix out"""
    from llama_cpp_omni_amd import rwkv
    hp = dict(rwkv.TINY_RWKV6 if arch == "6" else rwkv.TINY_RWKV7)
    rng = np.random.default_rng(40 + n_tokens)
    cv, pv = (rng.standard_normal((n_tokens, hp["n_embd"])).astype(np.float32) for _ in range(2))
    res, weights = [], None
    for b_ in (ref_be, be):
        lay = rwkv.RwkvLayer(b_, hp, rs_size=2, seed=13, big=Q4_K, out=Q6_K, weights=weights)
        weights = lay.weights
        g = pkg.Context(b_)
        cur, x_prev = g.new_tensor(0, hp["n_embd"], n_tokens), g.new_tensor(0, hp["n_embd"], n_tokens)
        L = {k: lay._w(g, t) for k, t in lay.T.items()}
        out = (rwkv.build_rwkv6_channel_mix if arch == "6" else rwkv.build_rwkv7_channel_mix)(g, cur, x_prev, L)
        g.alloc()
        b_.tensor_set(cur, cv)
        b_.tensor_set(x_prev, pv)
        b_.graph_compute(g.graph())
        res.append(b_.tensor_get(out).copy())
        g.free()
        lay.wctx.free()
    e = nmse(res[1], res[0])
    print(f"channel mix rwkv{arch} n_tokens={n_tokens}: NMSE {e:.3e}")
    assert np.isfinite(res[1]).all() and e <= 1e-6, e
