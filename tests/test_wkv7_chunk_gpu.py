"""RWKV_WKV7 on the chunked matrix-core kernel (kernels/wkv7_chunk.hip, `-m gpu`), against the reference CPU backend (two threads) on the same graph.  Bar: the op's
own, NMSE <= 1e-7 separately over the outputs and over the new states (test_wkv_ops_gpu.BAR, _check).  Every case asserts by how much `wkv7_launches` and
`wkv7_chunk_launches` moved."""
import numpy as np
import pytest

from conftest import nmse
from test_wkv_chunk_gpu import LAWS
from test_wkv_ops_gpu import BAR, _check, _data, _f64, _run, ref_be  # noqa: F401  (ref_be: the two-thread reference backend)

pytestmark = pytest.mark.gpu

KEYS = ["wkv7_launches", "wkv7_chunk_launches"]


def _both(pkg, be, ref_be, S, H, tps, n_seqs, data, delta, what, option=-1, fixture=None):
    """the node on both backends under `option`; the reference against the float64 loop where `fixture` gives a bound; the counters; parity at the bar"""
    T, n_out = tps * n_seqs, S * H * tps * n_seqs
    want = _run(pkg, ref_be, "wkv7", S, H, T, n_seqs, data)
    if fixture is not None:
        host = _f64("wkv7", data, S, H, tps, n_seqs)
        e_fix = max(nmse(want[:n_out], host[:n_out]), nmse(want[n_out:], host[n_out:]))
        print(f"{what}: reference vs float64 loop: NMSE {e_fix:.3e}")
        assert e_fix <= fixture, f"{what}: reference vs float64 loop: NMSE {e_fix:.3e}"
    be.set_option("wkv_chunk", option)
    try:
        n0 = [be.get_stat(k) for k in KEYS]
        got = _run(pkg, be, "wkv7", S, H, T, n_seqs, data)
        moved = [be.get_stat(k) - n for k, n in zip(KEYS, n0)]
    finally:
        be.set_option("wkv_chunk", -1)
    assert moved == [1, delta], f"{what}: {KEYS} moved by {moved}"
    _check(got, want, S, H, T, what)
    return got, want


@pytest.mark.parametrize("tps", [15, 16, 17, 33, 65, 130])
@pytest.mark.parametrize("n_seqs", [1, 3])
@pytest.mark.parametrize("S", [64, 128])
def test_chunk_parity(pkg, be, ref_be, S, n_seqs, tps):
    """a ragged single sub-chunk, exactly one, the first off-diagonal block (S = 64) / second chunk (S = 128), a one-token last chunk past 32 and past 64, several chunks
    with a ragged tail"""
    _both(pkg, be, ref_be, S, 3, tps, n_seqs, _data("wkv7", S, 3, tps * n_seqs, n_seqs, seed=S + 31 * tps + n_seqs), 1, f"wkv7 S={S} {tps}x{n_seqs}", option=2)


@pytest.mark.parametrize("law", list(LAWS))
def test_chunk_decay_ranges(pkg, be, ref_be, law):
    """w outside U(0.3, 1): a model's law, negative ones, exact zeros and 1e-30 (the clamp), and 0.999, where the state that enters the sequence must still shape the
    final state (asserted on the reference: the carry between chunks).  The reference is first held to the float64 loop at 1e-10."""
    S, H, tps, n_seqs = 64, 3, 130, 3
    data = _data("wkv7", S, H, tps * n_seqs, n_seqs, seed=77)
    data["w"] = LAWS[law](np.random.default_rng(78), data["w"].shape).astype(np.float32)
    _, want = _both(pkg, be, ref_be, S, H, tps, n_seqs, data, 1, f"wkv7 {law}", option=2, fixture=1e-10)
    if law == "const":
        n_out = S * H * tps * n_seqs
        zero = _run(pkg, ref_be, "wkv7", S, H, tps * n_seqs, n_seqs, dict(data, state=np.zeros_like(data["state"])))
        assert nmse(zero[n_out:], want[n_out:]) > 1e-2


def test_chunk_harder_solve(pkg, be, ref_be):
    """consecutive kk nearly collinear (base + 0.05 noise, normalised), gate 0.98, w in U(0.9, 1): I - A_ab has off-diagonal entries near 1"""
    S, H, tps = 64, 3, 130
    data = _data("wkv7", S, H, tps, 1, seed=41)
    rng = np.random.default_rng(42)
    kk = rng.standard_normal((1, H, S)) + 0.05 * rng.standard_normal((tps, H, S))
    kk /= np.sqrt((kk ** 2).sum(-1, keepdims=True))
    data.update(a=(-kk).astype(np.float32), b=(kk * 0.98).astype(np.float32), w=rng.uniform(0.9, 1.0, (tps, H, S)).astype(np.float32))
    _both(pkg, be, ref_be, S, H, tps, 1, data, 1, "wkv7 collinear kk", option=2)


def test_chunk_routing(pkg, be, ref_be):
    """at the default option: the threshold in force (both head sizes take the kernel from it), a head size that stays on the serial kernels, option 0, and the two
    kernels against each other"""
    n = int(be.get_stat("wkv7_chunk_min_tokens"))
    assert n > 32
    data = _data("wkv7", 64, 3, n, 1, seed=5)
    _both(pkg, be, ref_be, 64, 3, n - 1, 1, {k: (v if k == "state" else v[:n - 1]) for k, v in data.items()}, 0, f"wkv7 {n - 1} tokens")
    chunked, _ = _both(pkg, be, ref_be, 64, 3, n, 1, data, 1, f"wkv7 {n} tokens")
    n0 = [be.get_stat(k) for k in KEYS]
    _run(pkg, be, "wkv7", 24, 2, n, 1, _data("wkv7", 24, 2, n, 1, seed=6))      # (S = 24: the reference cannot run it, test_wkv_ops_gpu._ref_takes)
    assert [be.get_stat(k) - v for k, v in zip(KEYS, n0)] == [1, 0]
    _both(pkg, be, ref_be, 128, 3, n, 1, _data("wkv7", 128, 3, n, 1, seed=7), 1, "wkv7 S=128")
    serial, _ = _both(pkg, be, ref_be, 64, 3, n, 1, data, 0, "wkv7 option 0", option=0)
    _check(chunked, serial, 64, 3, n, "wkv7 chunked vs serial")


def test_chunk_in_a_layer(pkg, be, ref_be):
    """one rwkv7 time-mix layer of rwkv.py (F32 weights): a 130-token prompt under option 2, then one token from the carried states; bars of test_rwkv_layers_gpu"""
    from llama_cpp_omni_amd import rwkv
    from test_rwkv_layers_gpu import _compare, _hp
    hp = _hp("rwkv7_first_gated")
    rng = np.random.default_rng(23)
    steps = [rng.standard_normal((n_t, hp["n_embd"])).astype(np.float32) for n_t in (130, 1)]
    res, weights, moved = [], None, []
    try:
        for b_ in (ref_be, be):
            lay = rwkv.RwkvLayer(b_, hp, rs_size=4, seed=11, weights=weights)
            weights = lay.weights
            outs = []
            for xv in steps:
                g, x, s_copy, _, N = lay.build(xv.shape[0], 1, n_rs=2, rs_head=1, rs_zero=-1)
                b_.tensor_set(x, xv)
                b_.tensor_set(s_copy, np.array([1, 0], np.int32))
                be.set_option("wkv_chunk", 2 if xv.shape[0] > 1 else -1)
                c0 = be.get_stat("wkv7_chunk_launches")
                b_.graph_compute(g.graph())
                moved.append(be.get_stat("wkv7_chunk_launches") - c0)
                outs.append(tuple(b_.tensor_get(t).copy() for t in (N["out"], lay.r_states, lay.s_states)))
                g.free()
            res.append(outs)
            lay.wctx.free()
    finally:
        be.set_option("wkv_chunk", -1)
    assert moved == [0, 0, 1, 0], moved                      # the prompt on the GPU, and nothing else
    for step, (want, got) in enumerate(zip(*res)):
        _compare(got, want, f"rwkv7_first_gated step {step}")
