"""Mixture-of-experts ops on the GPU (`-m gpu`): ARGSORT (kernels/argsort.hip), MUL_MAT_ID on K-quant experts (mmvk.hip k_mmv_id) and the reference's
build_moe_ffn block (llama.cpp-omni_amd/qwen3moe.py), each through the backend C-ABI and against the reference CPU backend (oracle/ref_backend.py) on the same graph.

Bars: ARGSORT -- exact equality of the i32 output (distinct values, as the reference's own test_argsort: its exchange sort is not stable, this kernel puts the
lower index first).  MUL_MAT_ID -- NMSE <= 1e-9, the project's bar for integer mat-vecs against the same integers (test_mul_mat_vs_oracle_shapes): every output
is the vec_dot a MUL_MAT column gets, only the f32 summation order over the super-blocks differs.  The block -- the selected ids equal, the output inside the
reference's own bar for MUL_MAT_ID in test-backend-ops (NMSE 5e-4).
No test HERE feeds an out-of-range id (the kernel clamps them, mmvk.hip; the reference asserts), and every sort key is distinct: the clamp, ties and the
special values are test_moe_scale_gpu's."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, I32 = 0, 26
TY = {"q4_K": 12, "q5_K": 13, "q6_K": 14}


def _compute(be_, c, outs, feeds):
    c.alloc()
    for t, v in feeds:
        be_.tensor_set(t, v)
    be_.graph_compute(c.graph())
    res = [be_.tensor_get(o).copy() for o in outs]
    c.free()
    return res


# ------------------------------------------------------------------------------------------------ supports_op
def _mmid_node(pkg, be, ty, K=256, M=64, n_expert=8, n_used=2, T=3):
    c = pkg.Context(be)
    as_ = c.new_tensor(ty, K, M, n_expert)
    b = c.new_tensor(F32, K, 1, T)
    ids = c.view_2d(c.new_tensor(I32, n_expert, T), n_used, T, n_expert * 4, 0)
    return c, c.mul_mat_id(as_, b, ids)


def test_supports_op_mul_mat_id_q4_k(pkg, be):
    c, y = _mmid_node(pkg, be, TY["q4_K"])
    c.alloc()
    assert be.supports_op(y)
    c.free()


def test_supports_op_argsort_f32(pkg, be):
    c = pkg.Context(be)
    y = c.argsort(c.new_tensor(F32, 128, 5), pkg.SORT_ORDER.DESC)
    c.alloc()
    assert be.supports_op(y)
    c.free()


def test_supports_op_refuses_f16_experts_and_rows_beyond_lds(pkg, be):
    c, y = _mmid_node(pkg, be, 1)                                   # F16 experts: no kernel with the id indirection
    c.alloc()
    assert not be.supports_op(y)
    c.free()
    c = pkg.Context(be)
    ok = c.argsort(c.new_tensor(F32, 16384, 1), pkg.SORT_ORDER.ASC)        # 16384 padded slots x 8 B = 128 KiB: the last that fits
    big = c.argsort(c.new_tensor(F32, 16385, 1), pkg.SORT_ORDER.ASC)       # pads to 32768 slots = 256 KiB
    c.alloc()
    assert be.supports_op(ok) and not be.supports_op(big)
    c.free()


# ------------------------------------------------------------------------------------------------ ARGSORT
def _argsort_rows(ne0, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(ne0) for _ in range(12)]).astype(np.float32).reshape(2, 2, 3, ne0)      # a shuffled arange per row: distinct values


def _argsort_run(pkg, be_, xv, order, pad=0):
    ne0 = xv.shape[-1]
    c = pkg.Context(be_)
    if pad:                                                           # rows read through nb1 > ne0 * 4: a view of a wider tensor
        wide = c.new_tensor(F32, ne0 + pad, 3, 2, 2)
        x = c.view_4d(wide, ne0, 3, 2, 2, wide.nb[1], wide.nb[2], wide.nb[3], 0)
        feed = np.full((2, 2, 3, ne0 + pad), -7.0, np.float32)
        feed[..., :ne0] = xv
        y = c.argsort(x, order)
        (got,) = _compute(be_, c, [y], [(wide, feed)])
    else:
        x = c.new_tensor(F32, ne0, 3, 2, 2)
        y = c.argsort(x, order)
        (got,) = _compute(be_, c, [y], [(x, xv)])
    return got.reshape(2, 2, 3, ne0)


@pytest.mark.parametrize("order", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("ne0", [1, 2, 8, 60, 128, 129, 1024])
def test_argsort_exact(pkg, be, ref_be, ne0, order):
    xv = _argsort_rows(ne0, 100 + ne0)
    got = _argsort_run(pkg, be, xv, order)
    want = _argsort_run(pkg, ref_be, xv, order)
    host = np.argsort(xv if order == 0 else -xv, axis=-1).astype(np.int32)
    assert np.array_equal(want, host)                                 # (the fixture itself: distinct values leave one answer)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("order", [0, 1], ids=["asc", "desc"])
def test_argsort_rows_of_a_wider_view(pkg, be, ref_be, order):
    xv = _argsort_rows(60, 7)
    got = _argsort_run(pkg, be, xv, order, pad=5)
    want = _argsort_run(pkg, ref_be, xv, order, pad=5)
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.argsort(xv if order == 0 else -xv, axis=-1).astype(np.int32))


def test_argsort_launch_counter(pkg, be):
    n0 = be.get_stat("argsort_launches")
    _argsort_run(pkg, be, _argsort_rows(8, 1), 1)
    assert be.get_stat("argsort_launches") == n0 + 1


# ------------------------------------------------------------------------------------------------ MUL_MAT_ID
def _ids(rng, pattern, n_expert, n_used, T):
    """the WIDE [T, n_expert] i32 tensor the node's ids are a strided view of (its first n_used columns)"""
    wide = np.stack([rng.permutation(n_expert) for _ in range(T)]).astype(np.int32)
    if pattern == "last":                                             # every token names expert n_expert - 1 in slot 0
        for t in range(T):
            j = int(np.where(wide[t] == n_expert - 1)[0][0])
            wide[t, [0, j]] = wide[t, [j, 0]]
    elif pattern == "same":                                           # every pair names the same expert
        wide[:, :n_used] = 1
    return wide


def _mmid_run(pkg, be_, ty, n_expert, n_used, T, M, K, bcast, wv, bv, idv):
    c = pkg.Context(be_)
    as_ = c.new_tensor(ty, K, M, n_expert)
    b = c.new_tensor(F32, K, 1 if bcast else n_used, T)
    wide = c.new_tensor(I32, n_expert, T)
    ids = c.view_2d(wide, n_used, T, wide.nb[1], 0)
    y = c.mul_mat_id(as_, b, ids)
    (got,) = _compute(be_, c, [y], [(as_, wv), (b, bv), (wide, idv)])
    return got.reshape(T, n_used, M)


# one case per edge: every type; 4 / 8 experts; 1 / 2 / 4 slots; 1 / 2 / 9 / 33 tokens; M = 70 is no multiple of the 2 rows a wave takes; K = 256 is one
# super-block (less than a wave step of 8), 2304 = nine (a ragged second step), 768 = three; b broadcast over the slots and per slot; an ids pattern that
# uses the last expert, one where all pairs name the same expert, random ones
MMID_CASES = [
    ("q4_K", 8, 2, 1, 64, 256, True, "last"),
    ("q4_K", 4, 4, 2, 70, 768, False, "rand"),
    ("q4_K", 8, 1, 9, 64, 2304, True, "same"),
    ("q4_K", 8, 4, 33, 70, 2304, False, "rand"),
    ("q5_K", 8, 2, 33, 70, 256, True, "rand"),
    ("q5_K", 4, 1, 2, 64, 2304, False, "last"),
    ("q5_K", 8, 4, 9, 64, 768, False, "same"),
    ("q6_K", 8, 4, 9, 70, 768, False, "same"),
    ("q6_K", 4, 2, 33, 64, 2304, True, "rand"),
    ("q6_K", 8, 2, 1, 70, 256, False, "last"),
    ("q6_K", 8, 1, 2, 70, 2304, True, "rand"),
]


@pytest.mark.parametrize("name,n_expert,n_used,T,M,K,bcast,pattern", MMID_CASES, ids=["-".join(str(v) for v in cs) for cs in MMID_CASES])
def test_mul_mat_id_vs_reference(pkg, be, ref_be, name, n_expert, n_used, T, M, K, bcast, pattern):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(n_expert * 1000 + n_used * 100 + T + M + K)
    ty = TY[name]
    wv = qwen3.random_blocks(rng, ty, M * n_expert, K, std=0.05)
    bv = (rng.standard_normal((T, 1 if bcast else n_used, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    idv = _ids(rng, pattern, n_expert, n_used, T)
    n0 = be.get_stat("mmv_id_launches")
    got = _mmid_run(pkg, be, ty, n_expert, n_used, T, M, K, bcast, wv, bv, idv)
    assert be.get_stat("mmv_id_launches") == n0 + 1                   # one launch covers every (slot, token) pair
    want = _mmid_run(pkg, ref_be, ty, n_expert, n_used, T, M, K, bcast, wv, bv, idv)
    e = nmse(got, want)
    print(f"MUL_MAT_ID {name} experts {n_expert} used {n_used} T {T} M {M} K {K} bcast {bcast} {pattern}: NMSE {e:.3e}")
    assert np.isfinite(got).all()
    assert e <= 1e-9


# ------------------------------------------------------------------------------------------------ the build_moe_ffn block
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


def _block_run(pkg, be_, weights, xs, captured=False):
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


@pytest.fixture(scope="module")
def moe_fixture(pkg, ref_be):
    """weights, inputs and the reference's results, computed once: tokens 1 and 5, four different inputs each (eager, capture, two replays)"""
    from llama_cpp_omni_amd import qwen3moe
    rng = np.random.default_rng(42)
    blk = qwen3moe.MoeBlock(ref_be, seed=5)
    weights = blk.weights
    blk.wctx.free()
    fx = {"weights": weights}
    for T in (1, 5):
        xs = [_separated_tokens(rng, weights["gate_inp"], T, 2) for _ in range(4)]
        fx[T] = (xs, _block_run(pkg, ref_be, weights, xs))
    return fx


@pytest.mark.parametrize("fusion", [1, 0], ids=["fusion", "no_fusion"])
@pytest.mark.parametrize("T", [1, 5])
def test_moe_ffn_block_eager_captured_replayed(pkg, be, moe_fixture, T, fusion):
    """the block eager (first submission), captured (second) and replayed (third, fourth), with a NEW router input at every submission so that other
    experts are chosen: the replay must follow the ids the launch reads from device memory"""
    xs, want = moe_fixture[T]
    assert len({tuple(w[0].ravel()) for w in want}) > 1               # (the fixture: the inputs do choose different experts)
    be.set_option("fusion", fusion)
    try:
        s0 = {k: be.get_stat(k) for k in ("mmv_id_launches", "argsort_launches", "graph_replays", "graph_captures")}
        got = _block_run(pkg, be, moe_fixture["weights"], xs)
        s1 = {k: be.get_stat(k) for k in s0}
    finally:
        be.set_option("fusion", 1)
    worst = 0.0
    for k, ((gi, go), (wi, wo)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), (k, gi, wi)
        e = nmse(go, wo)
        worst = max(worst, e)
        assert np.isfinite(go).all() and e <= 5e-4, (k, e)
    print(f"build_moe_ffn block T {T} fusion {fusion}: worst output NMSE over 4 submissions {worst:.3e}")
    # four submissions of one graph: eager, capture, two replays -- the launchers ran for the first two only (3 expert nodes, 1 sort each)
    assert s1["graph_captures"] - s0["graph_captures"] == 1 and s1["graph_replays"] - s0["graph_replays"] == 2
    assert s1["mmv_id_launches"] - s0["mmv_id_launches"] == 6
    assert s1["argsort_launches"] - s0["argsort_launches"] == 2


def test_moe_ffn_block_one_expert_used_cont(pkg, be, ref_be):
    """n_expert_used == 1: the aggregation is the CONT of the one view"""
    from llama_cpp_omni_amd import qwen3moe
    cfg = dict(qwen3moe.TINY_MOE, n_expert_used=1)
    rng = np.random.default_rng(3)
    res = []
    weights = None
    for b_ in (ref_be, be):
        blk = qwen3moe.MoeBlock(b_, cfg=cfg, seed=9, weights=weights)
        weights = blk.weights
        if not res:
            xv = _separated_tokens(rng, weights["gate_inp"], 3, 1)
        g, x, N = blk.build(3)
        b_.tensor_set(x, xv)
        b_.graph_compute(g.graph())
        res.append((b_.tensor_get(N["argsort"]).copy().reshape(3, -1)[:, :1], b_.tensor_get(N["moe_out"]).copy()))
        g.free()
        blk.wctx.free()
    assert np.array_equal(res[0][0], res[1][0])
    assert nmse(res[1][1], res[0][1]) <= 5e-4
