"""MUL_MAT_ID of K-quant experts against a prefill ubatch (`-m gpu`): the expert-grouped int8-MFMA path (kernels/mmq_id.hip: k_moe_group sorts the pairs by expert on
the device, k_mmq_id runs mmq.hip's body per (expert, 32-row tile, <= 32-column slice)), through the backend C-ABI and against the reference CPU backend on the same graph.

Bars: NMSE <= 1e-9 against the reference -- the project's bar for mmq.hip and k_mmv_id against the same vec_dot_q*_K_q8_K integers (test_mul_mat_mmq_vs_oracle,
test_mul_mat_id_vs_reference): only the f32 summation order over the super-blocks differs.  Position independence is exact (np.array_equal): a column's sum is a function
of its own weights, its own image and the launch's K split, which the host chooses from the shape alone.  The build_moe_ffn block -- the selected ids equal, the output
inside the reference's own bar for MUL_MAT_ID in test-backend-ops (NMSE 5e-4).
The id patterns are written out, so that the tile edges are hit for certain (33 pairs of one expert = a second slice of one column; 32 = exactly one; the last expert;
empty experts; every pair on one expert = four and more slices of it).  No test HERE feeds an out-of-range id (the kernels clamp them, the reference asserts): the clamp,
K >= 4096, 128 and more experts and more than 1024 pairs are test_moe_scale_gpu's."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, I32 = 0, 26
TY = {"q4_K": 12, "q5_K": 13, "q6_K": 14}
MIN_TOKENS = 64                                                       # MMQ_ID_MIN_TOKENS (graph_internal.hpp)


def _mmid_run(pkg, be_, ty, n_expert, n_used, T, M, K, bcast, wv, bv, idv, times=1):
    """ids: the first n_used columns of a WIDER [T, n_expert] i32 tensor (a strided view, as the top-k view of the argsort result); -> `times` results [T, n_used, M]"""
    c = pkg.Context(be_)
    as_ = c.new_tensor(ty, K, M, n_expert)
    b = c.new_tensor(F32, K, 1 if bcast else n_used, T)
    wide = c.new_tensor(I32, n_expert, T)
    ids = c.view_2d(wide, n_used, T, wide.nb[1], 0)
    y = c.mul_mat_id(as_, b, ids)
    c.alloc()
    for t, v in ((as_, wv), (b, bv), (wide, idv)):
        be_.tensor_set(t, v)
    res = []
    for _ in range(times):
        be_.graph_compute(c.graph())
        res.append(be_.tensor_get(y).copy().reshape(T, n_used, M))
    c.free()
    return res if times > 1 else res[0]


def _wide(sel, n_expert):
    """[T, n_used] chosen experts -> the wide [T, n_expert] tensor: the choice in front, the other experts behind (distinct per token where the choice is)"""
    T, n_used = sel.shape
    wide = np.empty((T, n_expert), np.int32)
    for t in range(T):
        rest = [e for e in range(n_expert) if e not in set(sel[t].tolist())]
        row = list(sel[t]) + rest
        wide[t] = (row + [0] * n_expert)[:n_expert]
    return wide


def _pattern(rng, pattern, n_expert, n_used, T):
    sel = np.empty((T, n_used), np.int32)
    if pattern == "edges":                                            # the table of the module's head: 33 + 31 pairs in slot 0, 32 + 32 in slot 1 (the last expert), the rest empty
        assert n_expert == 8 and n_used == 2 and T == 64
        sel[:33, 0] = 0; sel[33:, 0] = 1
        sel[:32, 1] = 2; sel[32:, 1] = 7
    elif pattern == "one":                                            # every pair names one expert: n_used * T pairs, four or more slices of it
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


def _inputs(pkg, name, n_expert, n_used, T, M, K, bcast, pattern, seed=0):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(seed + n_expert * 1000 + n_used * 100 + T + M + K)
    wv = qwen3.random_blocks(rng, TY[name], M * n_expert, K, std=0.05)
    bv = (rng.standard_normal((T, 1 if bcast else n_used, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    sel = _pattern(rng, pattern, n_expert, n_used, T)
    return wv, bv, sel


# ------------------------------------------------------------------------------------------------ counter and option
def test_mmq_id_counter_exists(be):
    assert be.get_stat("mmq_id_launches") >= 0


def _counts(be):
    return be.get_stat("mmq_id_launches"), be.get_stat("mmv_id_launches")


def test_route_by_token_count_and_option(pkg, be):
    args = ("q4_K", 8, 2, MIN_TOKENS, 64, 256, True, "rand")
    wv, bv, sel = _inputs(pkg, *args)
    q0, v0 = _counts(be)
    on = _mmid_run(pkg, be, TY["q4_K"], 8, 2, MIN_TOKENS, 64, 256, True, wv, bv, _wide(sel, 8))
    q1, v1 = _counts(be)
    assert (q1 - q0, v1 - v0) == (1, 0)                               # the grouping and the matrix launch count as one node; no per-pair launch
    be.set_option("mmq_id", 0)
    try:
        off = _mmid_run(pkg, be, TY["q4_K"], 8, 2, MIN_TOKENS, 64, 256, True, wv, bv, _wide(sel, 8))
        q2, v2 = _counts(be)
    finally:
        be.set_option("mmq_id", 1)
    assert (q2 - q1, v2 - v1) == (0, 1)
    assert np.isfinite(on).all() and nmse(on, off) <= 1e-9            # the cross-check switch: the same integers on both paths
    # one token fewer: the per-pair path with the option on
    T = MIN_TOKENS - 1
    wv, bv, sel = _inputs(pkg, "q4_K", 8, 2, T, 64, 256, True, "rand")
    _mmid_run(pkg, be, TY["q4_K"], 8, 2, T, 64, 256, True, wv, bv, _wide(sel, 8))
    q3, v3 = _counts(be)
    assert (q3 - q2, v3 - v2) == (0, 1)


# ------------------------------------------------------------------------------------------------ parity against the reference CPU backend
# one case per edge, not a product: every type; M = 70 (ragged last row tile) / 64; K = 256 (one block: one wave per tile) / 768 / 2304; 1 / 2 / 4 slots; b broadcast over
# the slots and per slot; T = 64 and 97; the written-out id patterns.  ids are always a strided view of a wider tensor.
MMQ_ID_CASES = [
    ("q4_K", 8, 2, 64, 70, 256, True, "edges"),
    ("q6_K", 8, 2, 64, 64, 768, False, "edges"),
    ("q5_K", 8, 2, 64, 70, 2304, True, "edges"),
    ("q4_K", 8, 2, 64, 64, 2304, False, "one"),
    ("q6_K", 4, 4, 97, 70, 256, False, "one"),
    ("q5_K", 8, 1, 97, 64, 768, True, "rand"),
    ("q4_K", 4, 4, 97, 70, 768, False, "rand"),
    ("q6_K", 8, 4, 64, 70, 2304, True, "rand"),
    ("q5_K", 8, 2, 97, 70, 256, False, "ragged"),
    ("q4_K", 8, 1, 64, 64, 768, True, "ragged"),
    ("q6_K", 8, 1, 97, 64, 2304, True, "ragged"),
]


@pytest.mark.parametrize("name,n_expert,n_used,T,M,K,bcast,pattern", MMQ_ID_CASES, ids=["-".join(str(v) for v in cs) for cs in MMQ_ID_CASES])
def test_mmq_id_vs_reference(pkg, be, ref_be, name, n_expert, n_used, T, M, K, bcast, pattern):
    wv, bv, sel = _inputs(pkg, name, n_expert, n_used, T, M, K, bcast, pattern)
    idv = _wide(sel, n_expert)
    q0, v0 = _counts(be)
    got = _mmid_run(pkg, be, TY[name], n_expert, n_used, T, M, K, bcast, wv, bv, idv)
    assert tuple(np.subtract(_counts(be), (q0, v0))) == (1, 0)
    want = _mmid_run(pkg, ref_be, TY[name], n_expert, n_used, T, M, K, bcast, wv, bv, idv)
    e = nmse(got, want)
    print(f"MUL_MAT_ID grouped {name} experts {n_expert} used {n_used} T {T} M {M} K {K} bcast {bcast} {pattern}: NMSE {e:.3e}")
    assert np.isfinite(got).all()
    assert e <= 1e-9


def test_mmq_id_all_zero_activation_block(pkg, be, ref_be):
    """one activation row half zero: an all-zero Q8_K block (d = 0) in the middle of the images, as test_mul_mat_mmq_vs_oracle has it"""
    name, n_expert, n_used, T, M, K = "q4_K", 8, 2, 64, 70, 768
    wv, bv, sel = _inputs(pkg, name, n_expert, n_used, T, M, K, True, "edges", seed=5)
    bv[3, 0, K // 2:] = 0.0
    bv[40, 0, :256] = 0.0
    idv = _wide(sel, n_expert)
    got = _mmid_run(pkg, be, TY[name], n_expert, n_used, T, M, K, True, wv, bv, idv)
    want = _mmid_run(pkg, ref_be, TY[name], n_expert, n_used, T, M, K, True, wv, bv, idv)
    e = nmse(got, want)
    print(f"MUL_MAT_ID grouped, zero blocks: NMSE {e:.3e}")
    assert np.isfinite(got).all() and e <= 1e-9


# ------------------------------------------------------------------------------------------------ position independence, bit for bit
@pytest.mark.parametrize("name,K,bcast", [("q4_K", 2304, True), ("q6_K", 768, False), ("q5_K", 256, False)], ids=["q4_K", "q6_K", "q5_K"])
def test_mmq_id_position_independent_bit_for_bit(pkg, be, name, K, bcast):
    n_expert, n_used, T, M = 8, 2, 97, 70
    wv, bv, sel = _inputs(pkg, name, n_expert, n_used, T, M, K, bcast, "ragged", seed=9)
    q0, _ = _counts(be)
    a1, a2 = _mmid_run(pkg, be, TY[name], n_expert, n_used, T, M, K, bcast, wv, bv, _wide(sel, n_expert), times=2)
    assert np.array_equal(a1, a2)                                     # two submissions of the identical inputs
    perm = np.random.default_rng(1).permutation(T)                    # token t of the second run is token perm[t] of the first: other slices, other slice positions
    p1 = _mmid_run(pkg, be, TY[name], n_expert, n_used, T, M, K, bcast, wv, bv[perm], _wide(sel[perm], n_expert))
    assert be.get_stat("mmq_id_launches") - q0 == 3
    assert np.isfinite(a1).all() and np.abs(a1).max() > 0
    assert np.array_equal(p1, a1[perm])


# ------------------------------------------------------------------------------------------------ the build_moe_ffn block at 64 tokens
def _separated_tokens(rng, gate_inp, T, n_used, gap=0.25):
    """T input rows whose router logits are well separated around the cut: the n_used + 1 largest of every token at least `gap` apart (the logits are O(1);
    8-bit activation noise and f32 re-association move them by 1e-2 at most), so the expert choice does not sit on rounding"""
    rows = []
    while len(rows) < T:
        x = rng.standard_normal(gate_inp.shape[1]).astype(np.float32)
        top = np.sort(gate_inp.astype(np.float64) @ x)[::-1][: n_used + 1]
        if np.min(top[:-1] - top[1:]) >= gap:
            rows.append(x)
    return np.stack(rows)


def _block_run(pkg, be_, weights, xs):
    """runs the block once per input in xs on ONE graph (so a backend that captures graphs replays it); -> [(ids [T, n_used], out [T, n_embd])]"""
    from llama_cpp_omni_amd import qwen3moe
    blk = qwen3moe.MoeBlock(be_, weights=weights)
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


def test_moe_ffn_block_64_tokens_eager_captured_replayed(pkg, be, ref_be):
    """the block eager (first submission), captured (second) and replayed (third, fourth), with a NEW input at every submission: the grouping changes under the replay"""
    from llama_cpp_omni_amd import qwen3moe
    rng = np.random.default_rng(64)
    blk = qwen3moe.MoeBlock(ref_be, seed=5)
    weights = blk.weights
    blk.wctx.free()
    T = MIN_TOKENS
    xs = [_separated_tokens(rng, weights["gate_inp"], T, 2) for _ in range(4)]
    want = _block_run(pkg, ref_be, weights, xs)
    assert len({tuple(w[0].ravel()) for w in want}) == 4              # (the fixture: every submission chooses other experts)
    keys = ("mmq_id_launches", "mmv_id_launches", "graph_replays", "graph_captures")
    s0 = {k: be.get_stat(k) for k in keys}
    got = _block_run(pkg, be, weights, xs)
    d = {k: be.get_stat(k) - s0[k] for k in keys}
    worst = 0.0
    for k, ((gi, go), (wi, wo)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), (k, gi, wi)
        e = nmse(go, wo)
        worst = max(worst, e)
        assert np.isfinite(go).all() and e <= 5e-4, (k, e)
    print(f"build_moe_ffn block T {T}: worst output NMSE over 4 submissions {worst:.3e}")
    # eager, capture, two replays -- the launchers ran for the first two only: 3 expert nodes each, all grouped
    assert d == {"mmq_id_launches": 6, "mmv_id_launches": 0, "graph_replays": 2, "graph_captures": 1}, d
