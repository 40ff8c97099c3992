"""The frame the nine block-format mat-vec kernels share (k_mmv_blocks<Form, NCOLS, ROWS>, mmvq.hip), at the two edges the per-type
tests do not reach (-m gpu): a wave that owns more than one row group, and a ragged last step behind a full one with U > 1.
Everything is compared with the reference CPU backend at test time."""
import numpy as np
import pytest

from conftest import nmse
from test_lowbit_gpu import _mul_mat, _weights

pytestmark = pytest.mark.gpu

# name: (type id, weights per block, launch counter or None)
FORMS = {"q8_0": (8, 32, None), "q4_0": (2, 32, None), "q5_0": (6, 32, None), "iq4_nl": (20, 32, "mmv_iq4nl_launches"), "iq4_xs": (23, 256, "mmv_iq4xs_launches"),
         "q4_1": (3, 32, "mmv_q41_launches"), "q5_1": (7, 32, "mmv_q51_launches"), "q2_k": (10, 256, "mmv_q2k_launches"), "q3_k": (11, 256, "mmv_q3k_launches")}
# "persist": 16 421 rows (odd) are more than 2 x 8192 row groups at two rows per wave and more than 8192 at one -- the grid stops at 2048
#            workgroups of four waves, so waves walk on to a second and a third group, the last group lacks a row (row clamp) and the one
#            step of a row is partial (three blocks / one super-block: lane clamp)
# "ragged":  65 blocks of 32 weights = two full steps of 32 blocks and one block (U = 2: a full stage, then a stage of one block and a step
#            past the end), or four full steps of Q8_0's 16 and one block (U = 4 / 2); 17 super-blocks = a full step of 16 and one
EDGES = {"persist": (16421, {32: 96, 256: 256}), "ragged": (37, {32: 2080, 256: 4352})}

_CASE = {}


def _case(pkg, ref_be, name, edge):
    """weights, eight activation columns and the reference's answer for them, computed once per (form, edge): a column's result does not
    depend on how many columns go with it"""
    if (name, edge) not in _CASE:
        ty, wpb, _ = FORMS[name]
        M, K = EDGES[edge][0], EDGES[edge][1][wpb]
        rng = np.random.default_rng(ty * 1000 + K)
        wv = _weights(rng, ty, M, K)
        xv = rng.standard_normal((8, K)).astype(np.float32)
        want = _mul_mat(pkg, ref_be, ty, wv, xv, (K, M), (K, 8))
        for a in (wv, xv, want):
            a.setflags(write=False)
        _CASE[(name, edge)] = (M, K, wv, xv, want)
    return _CASE[(name, edge)]


@pytest.mark.parametrize("name", list(FORMS))
@pytest.mark.parametrize("N", [1, 2, 5, 8])
@pytest.mark.parametrize("edge", list(EDGES))
def test_mmv_frame_edges(pkg, be, ref_be, name, N, edge):
    """N = 1, 2: the U-unrolled instances at two rows per wave; N = 5, 8: U = 1 (Q8_0: 2) at one row per wave.  One launch per call where
    the form has a counter; the reference's integers -- NMSE <= 1e-8, the project's bar for these kernels."""
    ty, _, stat = FORMS[name]
    M, K, wv, xv, want = _case(pkg, ref_be, name, edge)
    one_q80 = name == "q8_0" and N == 1                  # (a single Q8_0 column would take the batch-1 kernel of mmv1q.hip)
    if one_q80:
        be.set_option("mv1", 0)
    try:
        n0 = be.get_stat(stat) if stat else 0
        got = _mul_mat(pkg, be, ty, wv, xv[:N], (K, M), (K, N))
        if stat:
            assert be.get_stat(stat) - n0 == 1, "the form's mat-vec kernel did not run (or ran more than once)"
    finally:
        if one_q80:
            be.set_option("mv1", 1)
    assert got.shape == (N, M) and np.isfinite(got).all()
    e = nmse(got, want[:N])
    print(name, edge, M, K, N, "nmse", e)
    assert e <= 1e-8, (name, edge, M, K, N, e)
