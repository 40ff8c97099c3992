"""RWKV_WKV6 / GATED_LINEAR_ATTN on the chunked matrix-core kernel (kernels/wkv_chunk.hip, `-m gpu`), against the reference CPU backend on the same graph, which a fixture
assertion ties to the float64 restatement of test_wkv_ops_gpu (NMSE <= 1e-12).  Bar: the op's own, NMSE <= 1e-7 separately over the outputs and over the new states
(test_wkv_ops_gpu.BAR, _check).  Every case asserts by how much `wkv6_chunk_launches` / `gla_chunk_launches` moved."""
import numpy as np
import pytest

from conftest import nmse
from test_wkv_ops_gpu import BAR, _check, _data, _f64, _run, ref_be  # noqa: F401  (ref_be: the two-thread reference backend)

pytestmark = pytest.mark.gpu

DECAY = {"wkv6": "td", "gla": "g"}
LAWS = {"model": lambda rng, sh: np.exp(-np.exp(rng.normal(-1.0, 2.0, sh))),           # exp(-exp(N(-1, 2))): channels that die within a sub-chunk
        "signs": lambda rng, sh: rng.uniform(-1.0, 1.0, sh),
        "clamp": lambda rng, sh: np.where(rng.random(sh) < 0.05, 0.0, np.where(rng.random(sh) < 0.1, 1e-30, rng.uniform(0.3, 1.0, sh))),
        "const": lambda rng, sh: np.full(sh, 0.999)}


def _both(pkg, be, ref_be, op, S, H, tps, n_seqs, data, delta, what):
    """the node on both backends; the fixture (reference == float64 loop), the counters, parity at the bar"""
    T, n_out = tps * n_seqs, S * H * tps * n_seqs
    want = _run(pkg, ref_be, op, S, H, T, n_seqs, data)
    if op != "wkv7":
        host = _f64(op, data, S, H, tps, n_seqs)
        e_fix = max(nmse(want[:n_out], host[:n_out]), nmse(want[n_out:], host[n_out:]))
        assert e_fix <= 1e-12, f"{what}: reference vs float64 loop: NMSE {e_fix:.3e}"
    keys = [f"{op}_launches"] + [f"{o}_chunk_launches" for o in DECAY]
    n0 = [be.get_stat(k) for k in keys]
    got = _run(pkg, be, op, S, H, T, n_seqs, data)
    moved = [be.get_stat(k) - n for k, n in zip(keys, n0)]
    assert moved == [1] + [delta if o == op else 0 for o in DECAY], f"{what}: {keys} moved by {moved}"
    _check(got, want, S, H, T, what)
    return got, want


@pytest.mark.parametrize("tps", [16, 17, 64, 65, 130])
@pytest.mark.parametrize("n_seqs", [1, 3])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("op", list(DECAY))
def test_chunk_parity(pkg, be, ref_be, op, S, n_seqs, tps):
    """one diagonal block only, the first off-diagonal block, one whole chunk (two at S = 128), a one-token last chunk, a ragged last chunk"""
    be.set_option("wkv_chunk", 2)
    try:
        _both(pkg, be, ref_be, op, S, 3, tps, n_seqs, _data(op, S, 3, tps * n_seqs, n_seqs, seed=S + 31 * tps + n_seqs), 1, f"{op} S={S} {tps}x{n_seqs}")
    finally:
        be.set_option("wkv_chunk", -1)


@pytest.mark.parametrize("law", list(LAWS))
@pytest.mark.parametrize("op", list(DECAY))
def test_chunk_decay_ranges(pkg, be, ref_be, op, law):
    """decays outside U(0.3, 1): a model's law, negative ones, exact zeros and 1e-30 (the clamp), and 0.999, where the state that enters the sequence must still shape
    the final state (asserted on the reference: the carry between chunks)"""
    S, H, tps, n_seqs = 64, 3, 130, 3
    data = _data(op, S, H, tps * n_seqs, n_seqs, seed=77)
    data[DECAY[op]] = LAWS[law](np.random.default_rng(78), data[DECAY[op]].shape).astype(np.float32)
    be.set_option("wkv_chunk", 2)
    try:
        _, want = _both(pkg, be, ref_be, op, S, H, tps, n_seqs, data, 1, f"{op} {law}")
    finally:
        be.set_option("wkv_chunk", -1)
    if law == "const":
        n_out = S * H * tps * n_seqs
        zero = _run(pkg, ref_be, op, S, H, tps * n_seqs, n_seqs, dict(data, state=np.zeros_like(data["state"])))
        assert nmse(zero[n_out:], want[n_out:]) > 1e-2


@pytest.mark.parametrize("op", list(DECAY))
def test_chunk_routing(pkg, be, ref_be, op):
    """at the default option: the threshold in force, the head sizes and the op that stay on the serial kernels, and the two kernels against each other"""
    n = int(be.get_stat("wkv_chunk_min_tokens"))
    assert n > 32
    data = _data(op, 64, 3, n, 1, seed=5)
    _both(pkg, be, ref_be, op, 64, 3, n - 1, 1, {k: (v if k in ("state", "tf") else v[:n - 1]) for k, v in data.items()}, 0, f"{op} {n - 1} tokens")
    chunked, _ = _both(pkg, be, ref_be, op, 64, 3, n, 1, data, 1, f"{op} {n} tokens")
    _both(pkg, be, ref_be, op, 24, 2, n, 1, _data(op, 24, 2, n, 1, seed=6), 0, f"{op} S=24")
    _both(pkg, be, ref_be, "wkv7", 64, 3, n, 1, _data("wkv7", 64, 3, n, 1, seed=7), 0, "wkv7")
    be.set_option("wkv_chunk", 0)
    try:
        serial, _ = _both(pkg, be, ref_be, op, 64, 3, n, 1, data, 0, f"{op} option 0")
    finally:
        be.set_option("wkv_chunk", -1)
    _check(chunked, serial, 64, 3, n, f"{op} chunked vs serial")


@pytest.mark.parametrize("variant,op", [("rwkv6_fused", "wkv6"), ("qrwkv", "gla")])
def test_chunk_in_a_layer(pkg, be, ref_be, variant, op):
    """one time-mix layer of rwkv.py (F32 weights): a 130-token prompt, then one token from the carried states; bars of test_rwkv_layers_gpu"""
    from llama_cpp_omni_amd import rwkv
    from test_rwkv_layers_gpu import _compare, _hp
    hp = _hp(variant)
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
                be.set_option("wkv_chunk", 2 if xv.shape[0] > 1 else -1)      # (2: the 130 tokens whatever the threshold; the one token at the default)
                c0 = be.get_stat(f"{op}_chunk_launches")
                b_.graph_compute(g.graph())
                moved.append(be.get_stat(f"{op}_chunk_launches") - c0)
                outs.append(tuple(b_.tensor_get(t).copy() for t in (N["out"], lay.r_states, lay.s_states)))
                g.free()
            res.append(outs)
            lay.wctx.free()
    finally:
        be.set_option("wkv_chunk", -1)
    assert moved == [0, 0, 1, 0], moved                      # the prompt on the GPU, and nothing else
    for step, (want, got) in enumerate(zip(*res)):
        _compare(got, want, f"{variant} step {step}")
