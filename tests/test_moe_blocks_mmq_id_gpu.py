"""MUL_MAT_ID of Q8_0 / Q4_0 / Q5_0 / IQ4_NL experts against a prefill ubatch (`-m gpu`): the expert-grouped int8-MFMA path (kernels/mmq_id.hip: k_moe_group
sorts the pairs by expert on the device, k_mmq_id runs one MFMA per 32-weight block and (expert, 32-row tile, <= 32-column slice)), through the backend C-ABI
and against the reference CPU backend on the same graph.

Bars: NMSE <= 1e-8 against the reference over the whole output AND for every (token, slot) pair on its own -- the project's bar for these forms' integer mat-vecs
(test_lowbit_gpu.py, test_iq4_gpu.py): every output is the reference's vec_dot on the same integers (the same int8 products, the same product sumi * (d_y * d_x) per
block), only the order of the f32 additions over the blocks differs.  Position independence is exact (np.array_equal): a column's sum is a function of its own
weights, its own image and the launch's K split, which the host chooses from the shape alone.
The id patterns are written out, so that the tile edges are hit for certain (33 pairs of one expert = a second slice of one column; 32 = exactly one; 31; the last
expert; empty experts; every pair on one expert = many slices of it).  Every case asserts the launch counters and the K split (stat "mmq_id_blocks_ks") the shape
reaches under the launcher's rule, so that a change of the rule cannot take a case off its path unnoticed: KS = 1 and 4 both occur.
The ids are always a strided view of a wider tensor; no test here feeds an out-of-range id (the grouping launch that clamps them is test_moe_mmq_id_gpu's and
test_gptoss_mmq_id_gpu's)."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, I32 = 0, 26
TY = {"q8_0": 8, "q4_0": 2, "q5_0": 6, "iq4_nl": 20}
MIN_TOKENS = 65                                                       # MMQ_ID_BLOCKS_MIN_TOKENS (graph_internal.hpp)
STATS = ("mmq_id_blocks_launches", "mmv_id_blocks_launches", "mmq_id_launches", "mmv_id_launches", "mmq_id_mxfp4_launches", "mmv_id_mxfp4_launches")
GROUPED, PER_PAIR = (1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0)
BAR = 1e-8


def _run(pkg, be_, ty, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, times=1):
    """ids: the first n_used columns of a WIDER [T, n_used + 3] i32 tensor (a strided view, as the top-k view of the argsort result).  -> `times` results [T, n_used, M]"""
    c = pkg.Context(be_)
    as_ = c.new_tensor(ty, K, M, n_expert)
    b = c.new_tensor(F32, K, b_ne1, T)
    wide = c.new_tensor(I32, n_used + 3, T)
    ids = c.view_2d(wide, n_used, T, wide.nb[1], 0)
    y = c.mul_mat_id(as_, b, ids)
    c.alloc()
    assert be_.dev_s is None or be_.supports_op(y), "supports_op refused the node"      # (the reference backend is driven without a device object: nothing to ask)
    full = np.zeros((T, n_used + 3), np.int32)
    full[:, :n_used] = sel
    for t, v in ((as_, wv), (b, bv), (wide, full)):
        be_.tensor_set(t, v)
    res = []
    for _ in range(times):
        be_.graph_compute(c.graph())
        res.append(be_.tensor_get(y).copy().reshape(T, n_used, M))
    c.free()
    return res if times > 1 else res[0]


def _counts(be):
    return tuple(int(be.get_stat(k)) for k in STATS)


def _delta(be, s0):
    return tuple(a - b for a, b in zip(_counts(be), s0))


def _ks_rule(n_expert, n_used, T, M, K):
    """the launcher's rule (mmq_id.hip), restated: row tiles = ceil(M / 32), bound = min(pairs, experts) + pairs / 32, steps of 8 blocks; the split doubles
    while the grid bound stays inside 3072 / 2 waves and every wave keeps at least 4 steps"""
    pairs = n_used * T
    row_tiles, bound, nstep, ks = (M + 31) // 32, min(pairs, n_expert) + pairs // 32, (K // 32 + 7) // 8, 1
    while ks < 8 and row_tiles * bound * ks * 2 <= 3072 and ks * 4 <= nstep:
        ks *= 2
    return ks


def _pair_nmse(got, want):
    """NMSE of every (token, slot) pair on its own: [T, n_used]"""
    g, w = got.astype(np.float64), want.astype(np.float64)
    d, n = ((g - w) ** 2).sum(-1), (w ** 2).sum(-1)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


def _pattern(rng, pattern, n_expert, n_used, T):
    sel = np.empty((T, n_used), np.int32)
    if pattern == "edges":                                            # slot 0: 33 + 31 + 64 pairs on experts 0, 1, 3; slot 1: 32 + 96 on expert 2 and the last; 4, 5, 6 empty
        assert n_expert == 8 and n_used == 2 and T == 128
        sel[:33, 0] = 0; sel[33:64, 0] = 1; sel[64:, 0] = 3
        sel[:32, 1] = 2; sel[32:, 1] = 7
    elif pattern == "one":                                            # every pair names one expert: n_used * T pairs, four and more slices of it
        sel[:] = n_expert - 2
    elif pattern == "rand":                                           # a random permutation per token
        for t in range(T):
            sel[t] = rng.permutation(n_expert)[:n_used]
    elif pattern == "ragged":                                         # slot s: runs of 1, 2, 3, ... tokens on experts s, s + 1, ... (slices of every width, wrapping over the experts)
        for s in range(n_used):
            t, run, e = 0, 1, s
            while t < T:
                sel[t:t + run, s] = e % n_expert
                t += run; run += 1; e += 1
    else:
        raise ValueError(pattern)
    return sel


def _inputs(name, n_expert, n_used, T, M, K, b_ne1, pattern, seed=0):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(seed + TY[name] * 100000 + n_expert * 1000 + n_used * 100 + T + M + K)
    wv = qwen3.random_blocks(rng, TY[name], M * n_expert, K, std=0.05)
    bv = (rng.standard_normal((T, b_ne1, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    return rng, wv, bv, _pattern(rng, pattern, n_expert, n_used, T)


def _check(pkg, be, ref_be, what, name, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, expect=GROUPED):
    """runs the node on the device and on the reference, asserts the launch counters, the K split and both bars; -> (got, want)"""
    s0 = _counts(be)
    got = _run(pkg, be, TY[name], n_expert, n_used, T, M, K, b_ne1, wv, bv, sel)
    assert _delta(be, s0) == expect
    if expect == GROUPED:
        assert be.get_stat("mmq_id_blocks_ks") == _ks_rule(n_expert, n_used, T, M, K)
    want = _run(pkg, ref_be, TY[name], n_expert, n_used, T, M, K, b_ne1, wv, bv, sel)
    assert np.isfinite(want).all() and np.abs(want).max() > 0, "the fixture: the reference's own result is finite and not zero"
    e, pp = nmse(got, want), _pair_nmse(got, want)
    t, i = np.unravel_index(np.argmax(pp), pp.shape)
    print(f"MUL_MAT_ID {name} grouped {what}: experts {n_expert} used {n_used} T {T} M {M} K {K} b_ne1 {b_ne1} KS {int(be.get_stat('mmq_id_blocks_ks'))}: NMSE {e:.3e}, "
          f"worst pair (token {t}, slot {i}, expert {sel[t, i]}) {pp[t, i]:.3e}")
    assert np.isfinite(got).all()
    assert e <= BAR
    assert pp[t, i] <= BAR, (int(t), int(i), int(sel[t, i]), float(pp[t, i]))
    return got, want


# ------------------------------------------------------------------------------------------------ route, counter and option
@pytest.mark.parametrize("name", list(TY))
def test_route_by_token_count_and_option(pkg, be, name):
    n_expert, n_used, M, K = 8, 2, 64, 288
    rng, wv, bv, sel = _inputs(name, n_expert, n_used, MIN_TOKENS, M, K, 1, "rand")
    s0 = _counts(be)
    on = _run(pkg, be, TY[name], n_expert, n_used, MIN_TOKENS, M, K, 1, wv, bv, sel)
    assert _delta(be, s0) == GROUPED                                  # the grouping and the matrix launch count as one node; no per-pair launch, nothing on the other counters
    s1 = _counts(be)
    be.set_option("mmq_id", 0)
    try:
        off = _run(pkg, be, TY[name], n_expert, n_used, MIN_TOKENS, M, K, 1, wv, bv, sel)
        d = _delta(be, s1)
    finally:
        be.set_option("mmq_id", 1)
    assert d == PER_PAIR
    e, pp = nmse(on, off), _pair_nmse(on, off).max()
    print(f"MUL_MAT_ID {name} grouped against per-pair: NMSE {e:.3e}, worst pair {pp:.3e}")
    assert np.isfinite(on).all() and e <= BAR and pp <= BAR           # the cross-check switch: the same integers on both paths
    # one token fewer: the per-pair path with the option on
    T = MIN_TOKENS - 1
    rng, wv, bv, sel = _inputs(name, n_expert, n_used, T, M, K, 1, "rand")
    s2 = _counts(be)
    _run(pkg, be, TY[name], n_expert, n_used, T, M, K, 1, wv, bv, sel)
    assert _delta(be, s2) == PER_PAIR


@pytest.mark.parametrize("name", ["q4_1", "q5_1", "iq4_xs", "q2_K", "q3_K"])
def test_other_block_forms_stay_per_pair(pkg, be, name):
    """the five forms with a min term or super-blocks have no grouped kernel: the per-pair launch at the grouped forms' threshold too"""
    from llama_cpp_omni_amd import qwen3
    ty = {"q4_1": 3, "q5_1": 7, "iq4_xs": 23, "q2_K": 10, "q3_K": 11}[name]
    n_expert, n_used, M, K = 8, 2, 64, 256
    rng = np.random.default_rng(ty)
    wv = qwen3.random_blocks(rng, ty, M * n_expert, K, std=0.05)
    bv = rng.standard_normal((MIN_TOKENS, 1, K)).astype(np.float32)
    s0 = _counts(be)
    got = _run(pkg, be, ty, n_expert, n_used, MIN_TOKENS, M, K, 1, wv, bv, _pattern(rng, "rand", n_expert, n_used, MIN_TOKENS))
    assert _delta(be, s0) == PER_PAIR and np.isfinite(got).all()


# ------------------------------------------------------------------------------------------------ parity against the reference CPU backend
# name, experts, used, T, M, K, b_ne1, pattern, KS.  Per form the four id patterns, over the set: K = 288 (9 blocks: a ragged second fetch step) / 2880 (90 blocks: a
# ragged twelfth step, 12 steps over 4 waves) / 32 (one block); M = 70 (ragged last row tile) / 64; 1 / 2 / 4 slots; b broadcast over the slots (b_ne1 = 1), per slot,
# and 2 of 4; T = 128 and 161.
CASES = [
    ("q8_0", 8, 2, 128, 70, 288, 2, "edges", 1),
    ("q8_0", 8, 4, 128, 64, 2880, 4, "one", 4),
    ("q8_0", 8, 2, 161, 70, 288, 2, "ragged", 1),
    ("q8_0", 8, 4, 128, 70, 2880, 1, "rand", 4),
    ("q4_0", 8, 2, 128, 70, 2880, 1, "edges", 4),
    ("q4_0", 4, 4, 161, 70, 288, 4, "one", 1),
    ("q4_0", 8, 1, 128, 64, 2880, 1, "ragged", 4),
    ("q4_0", 8, 4, 161, 70, 32, 2, "rand", 1),
    ("q5_0", 8, 2, 128, 70, 288, 1, "edges", 1),
    ("q5_0", 8, 4, 128, 70, 2880, 2, "one", 4),
    ("q5_0", 8, 2, 161, 64, 2880, 2, "ragged", 4),
    ("q5_0", 8, 1, 161, 70, 288, 1, "rand", 1),
    ("iq4_nl", 8, 2, 128, 70, 2880, 2, "edges", 4),
    ("iq4_nl", 8, 4, 161, 64, 288, 1, "one", 1),
    ("iq4_nl", 8, 2, 128, 70, 288, 1, "ragged", 1),
    ("iq4_nl", 8, 4, 128, 70, 2880, 4, "rand", 4),
    ("q5_0", 8, 2, 128, 64, 1056, 1, "rand", 2),                      # 33 blocks, 5 steps over 2 waves; and 249 blocks, 32 steps over 8 waves (the widest fold): the
    ("q8_0", 8, 2, 128, 70, 7968, 2, "ragged", 8),                    # splits the MXFP4 table reaches with the same shapes
]


def test_cases_reach_both_splits():
    assert {cs[-1] for cs in CASES} >= {1, 4}                         # KS = 1 and a KS > 1 over the set


@pytest.mark.parametrize("name,n_expert,n_used,T,M,K,b_ne1,pattern,ks", CASES, ids=["-".join(str(v) for v in cs) for cs in CASES])
def test_mmq_id_blocks_vs_reference(pkg, be, ref_be, name, n_expert, n_used, T, M, K, b_ne1, pattern, ks):
    assert _ks_rule(n_expert, n_used, T, M, K) == ks                  # (the fixture: the shape does reach the stated split under the launcher's rule)
    rng, wv, bv, sel = _inputs(name, n_expert, n_used, T, M, K, b_ne1, pattern)
    if pattern == "edges":
        assert np.bincount(sel.ravel(), minlength=n_expert).tolist() == [33, 31, 32, 64, 0, 0, 0, 96]
    if b_ne1 == 2 and n_used == 4:                                    # (the fixture: slots 0 / 2 and 1 / 3 read two different columns, so a wrong i % b_ne1 shows)
        assert not np.array_equal(bv[:, 0], bv[:, 1])
    _check(pkg, be, ref_be, pattern, name, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel)


# ------------------------------------------------------------------------------------------------ position independence, bit for bit
@pytest.mark.parametrize("name,K,b_ne1", [("q8_0", 2880, 1), ("q4_0", 288, 2), ("q5_0", 2880, 2), ("iq4_nl", 288, 1)])
def test_mmq_id_blocks_position_independent_bit_for_bit(pkg, be, name, K, b_ne1):
    n_expert, n_used, T, M = 8, 2, 161, 70
    rng, wv, bv, sel = _inputs(name, n_expert, n_used, T, M, K, b_ne1, "ragged", seed=9)
    s0 = _counts(be)
    a1, a2 = _run(pkg, be, TY[name], n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, times=2)
    assert np.array_equal(a1, a2)                                     # two submissions of the identical inputs
    perm = np.random.default_rng(1).permutation(T)                    # token t of the second run is token perm[t] of the first: other slices, other slice positions
    p1 = _run(pkg, be, TY[name], n_expert, n_used, T, M, K, b_ne1, wv, bv[perm], sel[perm])
    assert _delta(be, s0) == (3, 0, 0, 0, 0, 0)
    assert np.isfinite(a1).all() and np.abs(a1).max() > 0
    assert np.array_equal(p1, a1[perm])
