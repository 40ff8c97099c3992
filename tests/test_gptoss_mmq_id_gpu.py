"""MUL_MAT_ID of MXFP4 experts (gpt-oss) against a prefill ubatch (`-m gpu`): the expert-grouped int8-MFMA path (kernels/mmq_id.hip: k_moe_group sorts the pairs
by expert on the device, k_mmq_id runs one MFMA per 17-byte block and (expert, 32-row tile, <= 32-column slice)), through the backend C-ABI and against the
reference CPU backend on the same graph.

Bars: NMSE <= 1e-9 against the reference over the whole output AND for every (token, slot) pair on its own -- the project's bar for the three id kernels against the
same integers: every output is the reference's vec_dot_mxfp4_q8_0 (the same int8 products, the same product sumi * (d_y * e8m0_half(e)) per block), only the order of
the f32 additions over the blocks differs.  Position independence is exact (np.array_equal): a column's sum is a function of its own weights, its own image and the
launch's K split, which the host chooses from the shape alone.  The build_moe_ffn block -- the selected ids equal, the output inside the reference's own bar for
MUL_MAT_ID in test-backend-ops (NMSE 5e-4).
The id patterns are written out, so that the tile edges are hit for certain (33 pairs of one expert = a second slice of one column; 32 = exactly one; 31; the last
expert; empty experts; every pair on one expert = many slices of it).  Every case asserts the launch counters and the K split (stat "mmq_id_mxfp4_ks") the shape
reaches under the launcher's rule, so that a change of the rule cannot take a case off its path unnoticed: KS = 1, 2, 4 and 8 all occur.
The ids are always a strided view of a wider tensor.  Out-of-range ids are fed in one test only, on experts that are a view inside a larger tensor the test owns."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, I32, MXFP4 = 0, 26, 39
MIN_TOKENS = 128                                                      # MMQ_ID_MXFP4_MIN_TOKENS (graph_internal.hpp)
STATS = ("mmq_id_mxfp4_launches", "mmv_id_mxfp4_launches", "mmq_id_launches", "mmv_id_launches")
GROUPED, PER_PAIR = (1, 0, 0, 0), (0, 1, 0, 0)
BAR = 1e-9


def _run(pkg, be_, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, skip_experts=0, times=1):
    """ids: the first n_used columns of a WIDER [T, n_used + 3] i32 tensor (a strided view, as the top-k view of the argsort result).  skip_experts = 1: the experts
    are a view_3d over experts 1 .. n_expert of a tensor that holds n_expert + 2.  -> `times` results [T, n_used, M]"""
    c = pkg.Context(be_)
    parent = c.new_tensor(MXFP4, K, M, n_expert + 2 * skip_experts)
    as_ = c.view_3d(parent, K, M, n_expert, parent.nb[1], parent.nb[2], skip_experts * parent.nb[2]) if skip_experts else parent
    b = c.new_tensor(F32, K, b_ne1, T)
    wide = c.new_tensor(I32, n_used + 3, T)
    ids = c.view_2d(wide, n_used, T, wide.nb[1], 0)
    y = c.mul_mat_id(as_, b, ids)
    c.alloc()
    assert be_.dev_s is None or be_.supports_op(y), "supports_op refused the node"      # (the reference backend is driven without a device object: nothing to ask)
    full = np.zeros((T, n_used + 3), np.int32)
    full[:, :n_used] = sel
    for t, v in ((parent, wv), (b, bv), (wide, full)):
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
    """the launcher's rule (mmq_id.hip), restated: row tiles = ceil(M / 32), bound = min(pairs, experts) + pairs / 32, steps of 8 blocks"""
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


def _inputs(pkg, n_expert, n_used, T, M, K, b_ne1, pattern, seed=0, n_own=None):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(seed + n_expert * 1000 + n_used * 100 + T + M + K)
    wv = qwen3.random_blocks(rng, MXFP4, M * (n_own or n_expert), K, std=0.05)
    bv = (rng.standard_normal((T, b_ne1, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    return rng, wv, bv, _pattern(rng, pattern, n_expert, n_used, T)


def _check(pkg, be, ref_be, what, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, expect=GROUPED, ref_sel=None, skip_experts=0):
    """runs the node on the device and on the reference (ref_sel: the ids the reference gets, where the device's are out of its range), asserts the launch counters,
    the K split and both bars; -> (got, want)"""
    s0 = _counts(be)
    got = _run(pkg, be, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, skip_experts)
    assert _delta(be, s0) == expect
    if expect == GROUPED:
        assert be.get_stat("mmq_id_mxfp4_ks") == _ks_rule(n_expert, n_used, T, M, K)
    want = _run(pkg, ref_be, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel if ref_sel is None else ref_sel, skip_experts)
    assert np.isfinite(want).all() and np.abs(want).max() > 0, "the fixture: the reference's own result is finite and not zero"
    e, pp = nmse(got, want), _pair_nmse(got, want)
    t, i = np.unravel_index(np.argmax(pp), pp.shape)
    print(f"MUL_MAT_ID mxfp4 grouped {what}: experts {n_expert} used {n_used} T {T} M {M} K {K} b_ne1 {b_ne1} KS {int(be.get_stat('mmq_id_mxfp4_ks'))}: NMSE {e:.3e}, "
          f"worst pair (token {t}, slot {i}, expert {sel[t, i]}) {pp[t, i]:.3e}")
    assert np.isfinite(got).all()
    assert e <= BAR
    assert pp[t, i] <= BAR, (int(t), int(i), int(sel[t, i]), float(pp[t, i]))
    return got, want


# ------------------------------------------------------------------------------------------------ route, counter and option
def test_route_by_token_count_and_option(pkg, be):
    n_expert, n_used, M, K = 8, 2, 64, 288
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, MIN_TOKENS, M, K, 1, "rand")
    s0 = _counts(be)
    on = _run(pkg, be, n_expert, n_used, MIN_TOKENS, M, K, 1, wv, bv, sel)
    assert _delta(be, s0) == GROUPED                                  # the grouping and the matrix launch count as one node; no per-pair launch, nothing on the K-quant counters
    s1 = _counts(be)
    be.set_option("mmq_id", 0)
    try:
        off = _run(pkg, be, n_expert, n_used, MIN_TOKENS, M, K, 1, wv, bv, sel)
        d = _delta(be, s1)
    finally:
        be.set_option("mmq_id", 1)
    assert d == PER_PAIR
    assert np.isfinite(on).all() and nmse(on, off) <= 1e-9            # the cross-check switch: the same integers on both paths
    # one token fewer: the per-pair path with the option on
    T = MIN_TOKENS - 1
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, 1, "rand")
    s2 = _counts(be)
    _run(pkg, be, n_expert, n_used, T, M, K, 1, wv, bv, sel)
    assert _delta(be, s2) == PER_PAIR


# ------------------------------------------------------------------------------------------------ parity against the reference CPU backend
# experts, used, T, M, K, b_ne1, pattern, KS.  One case per edge, not a product: K = 32 (one block) / 288 (9 blocks: a ragged second step) / 2880 (90 blocks: a ragged
# twelfth step, and 12 steps over 4 waves); M = 70 (ragged last row tile) / 64; 1 / 2 / 4 slots; b broadcast over the slots (b_ne1 = 1), per slot, and 2 of 4; T = 128
# and 161.  K = 1056 (33 blocks, 5 steps over 2 waves) and 7968 (249 blocks, 32 steps over 8 waves: the widest fold, LDS near its limit) are there for KS = 2 and 8;
# the last case is the gpt-oss-20b structure at the smallest token count.
CASES = [
    (8, 2, 128, 70, 32, 1, "edges", 1),
    (8, 2, 128, 64, 288, 2, "edges", 1),
    (8, 2, 128, 70, 2880, 1, "edges", 4),
    (8, 4, 128, 64, 2880, 4, "one", 4),
    (4, 4, 161, 70, 288, 4, "one", 1),
    (8, 1, 161, 64, 288, 1, "rand", 1),
    (8, 4, 161, 70, 32, 2, "rand", 1),
    (8, 4, 128, 70, 2880, 1, "rand", 4),
    (8, 2, 161, 70, 288, 2, "ragged", 1),
    (8, 1, 128, 64, 2880, 1, "ragged", 4),
    (8, 2, 128, 64, 1056, 1, "rand", 2),
    (8, 2, 128, 70, 7968, 2, "ragged", 8),
    (32, 4, 128, 2880, 2880, 1, "rand", 1),
]


@pytest.mark.parametrize("n_expert,n_used,T,M,K,b_ne1,pattern,ks", CASES, ids=["-".join(str(v) for v in cs) for cs in CASES])
def test_mmq_id_mxfp4_vs_reference(pkg, be, ref_be, n_expert, n_used, T, M, K, b_ne1, pattern, ks):
    assert _ks_rule(n_expert, n_used, T, M, K) == ks                  # (the fixture: the shape does reach the stated split under the launcher's rule)
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, b_ne1, pattern)
    if pattern == "edges":
        assert np.bincount(sel.ravel(), minlength=n_expert).tolist() == [33, 31, 32, 64, 0, 0, 0, 96]
    if b_ne1 == 2 and n_used == 4:                                    # (the fixture: slots 0 / 2 and 1 / 3 read two different columns, so a wrong i % b_ne1 shows)
        assert not np.array_equal(bv[:, 0], bv[:, 1])
    _check(pkg, be, ref_be, pattern, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel)


# ------------------------------------------------------------------------------------------------ scale edges
def test_mmq_id_mxfp4_denormal_scales(pkg, be, ref_be):
    """every block's e is 0 or 1: half the scale is 2^-128 / 2^-127, an f32 DENORMAL.  Activations uniform in +-1e6 give d_y <= 1e6 / 127, so the reference's outputs
    sumi * (d_y * 2^-128) are normal f32 numbers around 2^-100; a kernel that flushes the denormal scale returns zeros"""
    n_expert, n_used, T, M, K = 8, 4, 128, 70, 288
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, 1, "rand", seed=77)
    wv = wv.reshape(M * n_expert, K // 32, 17).copy()
    wv[..., 0] = rng.integers(0, 2, size=wv.shape[:2])
    wv = wv.reshape(M * n_expert, -1)
    bv = rng.uniform(-1e6, 1e6, (T, 1, K)).astype(np.float32)
    got, want = _check(pkg, be, ref_be, "e in {0, 1}", n_expert, n_used, T, M, K, 1, wv, bv, sel)
    big = np.abs(want) >= 2.0 ** -110
    assert big.mean() > 0.5 and np.abs(want).max() < 2.0 ** -90       # (the fixture: results of about 2^-100, far above the f32 denormal range)
    assert (got[big] != 0).all()


def test_mmq_id_mxfp4_largest_scale(pkg, be, ref_be):
    """one block of every row has e = 254 (half the scale: 2^126) beside ordinary ones; activations of amplitude 0.01 (d_y about 2^-13.6) keep the reference's result
    finite: |sumi| <= 32 * 127 * 12 < 2^15.6, so one such block stays below 2^128 (_check asserts that on the CPU result before it compares)"""
    n_expert, n_used, T, M, K = 8, 2, 128, 70, 288
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, 1, "rand", seed=78)
    wv = wv.reshape(M * n_expert, K // 32, 17).copy()
    wv[np.arange(M * n_expert), rng.integers(0, K // 32, M * n_expert), 0] = 254
    wv = wv.reshape(M * n_expert, -1)
    bv = rng.uniform(-0.01, 0.01, (T, 1, K)).astype(np.float32)
    bv[..., ::32] = 0.01                                              # every block's amax, so d_y = 0.01 / 127
    got, want = _check(pkg, be, ref_be, "e = 254", n_expert, n_used, T, M, K, 1, wv, bv, sel)
    assert np.abs(want).max() > 2.0 ** 110


def test_mmq_id_mxfp4_all_zero_activation_block(pkg, be, ref_be):
    """activation rows with all-zero 32-blocks (d = 0) in the middle of the images"""
    n_expert, n_used, T, M, K = 8, 2, 128, 70, 288
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, 1, "edges", seed=5)
    bv[3, 0, K // 2:] = 0.0
    bv[40, 0, 32:64] = 0.0
    bv[100, 0, :] = 0.0
    _check(pkg, be, ref_be, "zero blocks", n_expert, n_used, T, M, K, 1, wv, bv, sel)


# ------------------------------------------------------------------------------------------------ position independence, bit for bit
@pytest.mark.parametrize("K,b_ne1", [(2880, 1), (288, 2)], ids=["K2880", "K288"])
def test_mmq_id_mxfp4_position_independent_bit_for_bit(pkg, be, K, b_ne1):
    n_expert, n_used, T, M = 8, 2, 161, 70
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, b_ne1, "ragged", seed=9)
    s0 = _counts(be)
    a1, a2 = _run(pkg, be, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, times=2)
    assert np.array_equal(a1, a2)                                     # two submissions of the identical inputs
    perm = np.random.default_rng(1).permutation(T)                    # token t of the second run is token perm[t] of the first: other slices, other slice positions
    p1 = _run(pkg, be, n_expert, n_used, T, M, K, b_ne1, wv, bv[perm], sel[perm])
    assert _delta(be, s0) == (3, 0, 0, 0)
    assert np.isfinite(a1).all() and np.abs(a1).max() > 0
    assert np.array_equal(p1, a1[perm])


# ------------------------------------------------------------------------------------------------ the clamp, in a form that cannot fault
def test_mmq_id_mxfp4_out_of_range_ids_are_clamped(pkg, be, ref_be):
    """the experts are experts 1 .. 8 of a tensor of 10, every expert other random blocks.  Ids -1 and 8 (no other out-of-range value) beside valid ones: clamped
    they name experts 0 and 7 of the view, which is what the reference computes from the ids clipped on the host; unclamped they would name experts 0 and 9 of the
    PARENT -- memory this test owns, other weights, another result"""
    n_expert, n_used, T, M, K = 8, 4, 128, 70, 2880
    rng, wv, bv, sel = _inputs(pkg, n_expert, n_used, T, M, K, 1, "rand", seed=3, n_own=n_expert + 2)
    bad = rng.random((T, n_used)) < 0.4
    sel[bad] = rng.choice(np.array([-1, n_expert], np.int32), int(bad.sum()))
    sel[0] = (-1, n_expert, 3, -1)
    assert (sel == -1).sum() >= 3 and (sel == n_expert).sum() >= 3 and ((sel >= 0) & (sel < n_expert)).sum() >= 3 and sel.min() == -1 and sel.max() == n_expert
    clipped = np.clip(sel, 0, n_expert - 1)
    got, want = _check(pkg, be, ref_be, "clamp", n_expert, n_used, T, M, K, 1, wv, bv, sel, ref_sel=clipped, skip_experts=1)
    # (the fixture: the neighbours do hold other weights -- the reference on the parent's experts 0 and 9 in place of the view's 0 and 7 misses the bar by far)
    blocks = wv.reshape(n_expert + 2, -1)
    stray = np.concatenate([blocks[1:-1], blocks[-1:], blocks[:1]])   # view experts 0 .. 7, then "expert 8" = the parent's last and "expert 9" = the parent's first
    unclamped = np.where(sel == -1, n_expert + 1, sel)
    other = _run(pkg, ref_be, n_expert + 2, n_used, T, M, K, 1, stray.reshape(wv.shape[0], -1), bv, unclamped)
    assert _pair_nmse(other, want)[(sel == -1) | (sel == n_expert)].min() > 1e-3


# ------------------------------------------------------------------------------------------------ the gpt-oss build_moe_ffn block at 128 tokens
def _separated_tokens(rng, gate_inp, gate_inp_b, T, n_used, gap=0.25):
    """T input rows whose biased router logits are well separated around the cut: the n_used + 1 largest of every token at least `gap` apart, so the expert choice
    does not sit on rounding (candidates drawn a batch at a time)"""
    rows = []
    while len(rows) < T:
        x = (rng.standard_normal((4 * T, gate_inp.shape[1])) * 2).astype(np.float32)
        top = -np.sort(-(x.astype(np.float64) @ gate_inp.astype(np.float64).T + gate_inp_b), axis=1)[:, : n_used + 1]
        rows.extend(x[np.min(top[:, :-1] - top[:, 1:], axis=1) >= gap])
    return np.stack(rows[:T])


def _block_run(pkg, be_, weights, xs):
    """runs the block once per input in xs on ONE graph (so a backend that captures graphs replays it); -> [(ids [T, n_used], out [T, n_embd])]"""
    from llama_cpp_omni_amd import gptoss
    blk = gptoss.GptOssBlock(be_, weights=weights)
    g, x, N = blk.build(xs[0].shape[0])
    gr = g.graph()
    res = []
    for xv in xs:
        be_.tensor_set(x, xv)
        be_.graph_compute(gr)
        ids = be_.tensor_get(N["argsort"]).copy().reshape(xv.shape[0], -1)[:, : blk.cfg["n_expert_used"]]
        res.append((ids, be_.tensor_get(N["moe_out"]).copy().reshape(xv.shape[0], -1)))
    g.free()
    blk.wctx.free()
    return res


def test_gptoss_ffn_block_128_tokens_eager_captured_replayed(pkg, be, ref_be):
    """the block eager (first submission), captured (second) and replayed (third, fourth), with a NEW router-separated input at every submission: the grouping
    changes under the replay"""
    from llama_cpp_omni_amd import gptoss
    rng = np.random.default_rng(128)
    blk = gptoss.GptOssBlock(ref_be, seed=6)
    weights = blk.weights
    blk.wctx.free()
    T = MIN_TOKENS
    xs = [_separated_tokens(rng, weights["gate_inp"], weights["gate_inp_b"], T, 4) for _ in range(4)]
    want = _block_run(pkg, ref_be, weights, xs)
    assert len({tuple(w[0].ravel()) for w in want}) == 4              # (the fixture: every submission chooses other experts)
    keys = ("mmq_id_mxfp4_launches", "mmv_id_mxfp4_launches", "graph_replays", "graph_captures")
    s0 = {k: be.get_stat(k) for k in keys}
    got = _block_run(pkg, be, weights, xs)
    d = {k: be.get_stat(k) - s0[k] for k in keys}
    worst = 0.0
    for k, ((gi, go), (wi, wo)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), (k, gi, wi)
        e = nmse(go, wo)
        worst = max(worst, e)
        assert np.isfinite(go).all() and e <= 5e-4, (k, e)
    print(f"gpt-oss build_moe_ffn block T {T}: worst output NMSE over 4 submissions {worst:.3e}")
    # eager, capture, two replays -- the launchers ran for the first two only: 3 expert nodes each, all grouped
    assert d == {"mmq_id_mxfp4_launches": 6, "mmv_id_mxfp4_launches": 0, "graph_replays": 2, "graph_captures": 1}, d
