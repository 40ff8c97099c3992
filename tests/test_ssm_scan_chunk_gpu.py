"""SSM_SCAN on the chunked matrix-core kernel (kernels/ssm_chunk.hip, `-m gpu`): Mamba-2 nodes of 128 tokens and more, against the reference CPU backend on the same
graph and a float64 loop of the recurrence.  Bar: the op's own, NMSE <= 1e-7 separately over y and over the final states (test_ssm_ops_gpu.BAR).  Every case asserts
by how much `ssm_scan_chunk_launches` moved."""
import numpy as np
import pytest

from conftest import nmse
from test_ssm_ops_gpu import BAR, _check_scan, _scan_data, _scan_run

pytestmark = pytest.mark.gpu

MAIN = (128, 64, 6, 2)                                     # (d_state, head_dim, n_head, n_group)


def _scan_f64(shape, n_t, n_s, d):
    """the recurrence in float64.  Its per-token coefficients dt' and exp(dt' A) are rounded to f32 where the op forms them in f32 (log1pf(expf(dt)), expf(dt' * A)):
    with a constant dt that rounding is the same at every token, and 200 tokens of it are no property of the recurrence"""
    d_state, head_dim, n_head, n_group = shape
    di, gs, f32 = head_dim * n_head, n_group * d_state, np.float32
    xBC, dt = d["xBC"].astype(np.float64), d["dt"].astype(np.float64)
    x = xBC[..., :di].reshape(n_s, n_t, n_head, head_dim)
    B, C = (np.repeat(xBC[..., o:o + gs].reshape(n_s, n_t, n_group, d_state), n_head // n_group, axis=2) for o in (di, di + gs))
    dtp = np.where(dt > 20.0, dt, np.log1p(np.exp(dt).astype(f32).astype(np.float64))).astype(f32)
    dA = np.exp((dtp[..., None, None] * d["A"][None, None, :, None, :]).astype(np.float64)).astype(f32).astype(np.float64)
    S, y = d["s"][d["ids"][:n_s]].astype(np.float64), np.empty((n_s, n_t, n_head, head_dim))
    for t in range(n_t):
        S = S * dA[:, t] + (x[:, t] * dtp[:, t, :, None])[..., None] * B[:, t, :, None, :]
        y[:, t] = (S * C[:, t, :, None, :]).sum(-1)
    return np.concatenate([y.ravel(), S.ravel()])


def _both(pkg, be, ref_be, shape, n_t, n_s, data, delta, what="", fixture=1e-12):
    """the node on both backends; the fixture (reference == float64 loop), the counter, parity at the bar"""
    want = _scan_run(pkg, ref_be, shape, n_t, n_s, data)
    e_fix = nmse(want, _scan_f64(shape, n_t, n_s, data))
    assert e_fix <= fixture, f"reference vs float64 loop: NMSE {e_fix:.3e} > {fixture:.1e}"
    n0, c0 = be.get_stat("ssm_scan_launches"), be.get_stat("ssm_scan_chunk_launches")
    got = _scan_run(pkg, be, shape, n_t, n_s, data)
    assert be.get_stat("ssm_scan_launches") == n0 + 1
    assert be.get_stat("ssm_scan_chunk_launches") == c0 + delta, f"ssm_scan_chunk_launches moved by {be.get_stat('ssm_scan_chunk_launches') - c0}, not {delta}"
    _check_scan(got, want, shape, n_t, n_s, what)
    return got, want


@pytest.mark.parametrize("n_s", [1, 3])
@pytest.mark.parametrize("n_t", [128, 129, 200])
@pytest.mark.parametrize("shape", [MAIN, (64, 32, 4, 1), (256, 64, 4, 4), (128, 128, 3, 3)])
def test_chunk_parity(pkg, be, ref_be, shape, n_t, n_s):
    """one, two and four row slices, shared and per-head groups, all three state sizes; two whole chunks, a one-token last chunk, a ragged one"""
    _both(pkg, be, ref_be, shape, n_t, n_s, _scan_data(shape, n_t, n_s, seed=sum(shape) + 31 * n_t + n_s), 1)


@pytest.mark.parametrize("dt_const", [-6.0, 25.0])
def test_chunk_carry_between_chunks(pkg, be, ref_be, dt_const):
    """dt = -6: dt' = 2.5e-3, a decay of ~0.999 per token, so the state that enters a chunk is still there at its end (asserted on the reference); dt = 25: the linear
    softplus branch, decay ~0 per token.
    The fixture bound at dt = -6: a head's decay is ONE f32 value in [0.5, 1) used at all 200 tokens, and the reference's expf may differ from the correctly rounded one
    by an ulp, 2^-24 relative (measured: two of the six heads do, NMSE 1.4e-10 each, 1.2e-11 over all): up to (200 * 2^-24)^2 = 1.4e-10 instead of 1e-12, by that alone"""
    data = _scan_data(MAIN, 200, 3, seed=11, dt_const=dt_const)
    _, want = _both(pkg, be, ref_be, MAIN, 200, 3, data, 1, f"dt={dt_const}", fixture=(200 * 2.0 ** -24) ** 2 if dt_const < 0 else 1e-12)
    if dt_const < 0:
        ny = MAIN[1] * MAIN[2] * 200 * 3
        zero = _scan_run(pkg, ref_be, MAIN, 200, 3, dict(data, s=np.zeros_like(data["s"])))
        assert nmse(zero[ny:], want[ny:]) > 1e-2


@pytest.mark.parametrize("shape,n_t,off", [(MAIN, 127, False), ((16, 1, 200, 1), 200, False), ((64, 20, 4, 1), 200, False), (MAIN, 200, True)],
                         ids=["127_tokens", "mamba1", "head_dim_20", "option_off"])
def test_chunk_leaves_the_rest_to_the_serial_kernel(pkg, be, ref_be, shape, n_t, off):
    data = _scan_data(shape, n_t, 3, seed=13)
    if off:
        be.set_option("ssm_chunk", 0)
    try:
        serial, _ = _both(pkg, be, ref_be, shape, n_t, 3, data, 0, "serial")
    finally:
        be.set_option("ssm_chunk", -1)
    if off:                                                 # the two kernels against each other
        chunked, _ = _both(pkg, be, ref_be, shape, n_t, 3, data, 1, "chunked")
        _check_scan(chunked, serial, shape, n_t, 3, "chunked vs serial")


def test_chunk_in_a_mamba2_layer(pkg, be, ref_be):
    """one mamba2 layer of mamba.py: a 130-token prompt into a zeroed state row, then one token from the cached conv and ssm states.  F32 projection weights: at 130
    columns the block-quantised mat-muls run on their F16 images (bar 5e-4; measured here: conv states 1.3e-5 before the scan is reached), which the bars below do not admit"""
    from llama_cpp_omni_amd import mamba
    hp = dict(mamba.TINY_MAMBA2)
    rng = np.random.default_rng(21)
    steps = [(rng.standard_normal((130, hp["n_embd"])).astype(np.float32), 1), (rng.standard_normal((1, hp["n_embd"])).astype(np.float32), -1)]
    res, weights, moved = [], None, []
    for b_ in (be, ref_be):
        lay = mamba.MambaLayer(b_, hp, rs_size=3, seed=5, in_type=0, out_type=0, weights=weights)
        weights = lay.weights
        outs = []
        for xv, rs_zero in steps:
            g, x, s_copy, N = lay.build(xv.shape[0], 1, n_rs=2, rs_head=1, rs_zero=rs_zero)
            b_.tensor_set(x, xv)
            b_.tensor_set(s_copy, np.array([1, 0], np.int32))
            c0 = be.get_stat("ssm_scan_chunk_launches")
            b_.graph_compute(g.graph())
            moved.append(be.get_stat("ssm_scan_chunk_launches") - c0)
            outs.append((b_.tensor_get(N["out"]).copy(), b_.tensor_get(lay.conv_states).copy(), b_.tensor_get(lay.ssm_states).copy()))
            g.free()
        res.append(outs)
        lay.wctx.free()
    assert moved[0] >= 1 and moved[1:] == [0, 0, 0], moved   # the prompt on the GPU, and nothing else
    for step, (got, want) in enumerate(zip(*res)):
        e_out, e_conv, e_ssm = nmse(got[0], want[0]), nmse(got[1], want[1]), nmse(got[2], want[2])
        print(f"mamba2 step {step}: NMSE out {e_out:.3e} conv states {e_conv:.3e} ssm states {e_ssm:.3e}")
        assert np.isfinite(got[0]).all()
        assert e_out <= 1e-6 and e_conv <= BAR and e_ssm <= BAR, f"step {step}: NMSE out {e_out:.3e} conv {e_conv:.3e} ssm {e_ssm:.3e}"
