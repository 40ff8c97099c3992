"""MUL_MAT_ID on experts of the nine block formats of mmvq.hip -- Q8_0, Q4_0, Q5_0, IQ4_NL (Q8_0 images), Q4_1, Q5_1 (Q8_1 images), IQ4_XS, Q2_K, Q3_K (Q8_K images) --
on the per-pair kernel (`-m gpu`; kernels/mmvq.hip k_mmv_blocks_id: the dense mat-vec frame at one column behind the id indirection), through the backend C-ABI and
against the reference CPU backend (oracle/ref_backend.py) on the same graph.

Bars: NMSE <= 1e-8 against the reference over the whole output AND for every (token, slot) pair on its own -- the project's bar for these forms' integer mat-vecs
(test_lowbit_gpu.py, test_iq4_gpu.py): every output is the reference's vec_dot on the same integers, only the order of the f32 additions over the blocks differs.
Position independence is exact (np.array_equal): a pair's result is a function of its own expert rows and its own image.  The build_moe_ffn block -- the selected ids
equal, the output inside the reference's own bar for MUL_MAT_ID in test-backend-ops (NMSE 5e-4).
The ids are always a strided view of a wider i32 tensor.  Out-of-range ids are fed in one test only, on experts that are a view inside a larger tensor the test owns."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, F16, I32 = 0, 1, 26
TY = {"q8_0": 8, "q4_0": 2, "q5_0": 6, "iq4_nl": 20, "q4_1": 3, "q5_1": 7, "iq4_xs": 23, "q2_K": 10, "q3_K": 11}
SUPER = ("iq4_xs", "q2_K", "q3_K")                                    # 256-weight super-blocks; the rest: 32-weight blocks
MOE_STATS = ("mmv_id_blocks_launches", "mmv_id_launches", "mmq_id_launches", "mmv_id_mxfp4_launches", "mmq_id_mxfp4_launches", "mmq_id_blocks_launches")
PER_PAIR = (1, 0, 0, 0, 0, 0)
BAR = 1e-8


def _counts(be):
    return tuple(int(be.get_stat(k)) for k in MOE_STATS)


def _delta(be, s0):
    return tuple(a - b for a, b in zip(_counts(be), s0))


def _pair_nmse(got, want):
    """NMSE of every (token, slot) pair on its own: [T, n_used]"""
    g, w = got.astype(np.float64), want.astype(np.float64)
    d, n = ((g - w) ** 2).sum(-1), (w ** 2).sum(-1)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


# ------------------------------------------------------------------------------------------------ 1. admission
def _mmid_node(pkg, be, ty, K, M=64, n_expert=8, n_used=2, T=3, K_decl=None, view_offset=None):
    c = pkg.Context(be)
    as_ = c.new_tensor(ty, K, M, n_expert + (1 if view_offset is not None else 0))
    if view_offset is not None:                                       # experts as a view at a byte offset inside a tensor that holds one expert more
        as_ = c.view_3d(as_, K, M, n_expert, as_.nb[1], as_.nb[2], view_offset)
    b = c.new_tensor(F32, K, 1, T)
    if K_decl is not None:                                            # a row length the constructors refuse: declared on tensors that own room for more
        as_.t.ne[0] = K_decl
        b.t.ne[0] = K_decl
    ids = c.view_2d(c.new_tensor(I32, n_expert, T), n_used, T, n_expert * 4, 0)
    return c, c.mul_mat_id(as_, b, ids)


def _supported(be, c, y):
    c.alloc()
    ok = be.supports_op(y)
    c.free()
    return ok


@pytest.mark.parametrize("name", list(TY))
def test_supports_op_mul_mat_id_block_forms(pkg, be, name):
    assert _supported(be, *_mmid_node(pkg, be, TY[name], 256 if name in SUPER else 96))


def test_supports_op_still_refuses(pkg, be):
    assert not _supported(be, *_mmid_node(pkg, be, F16, 256))                            # F16 experts: no kernel with the id indirection
    assert not _supported(be, *_mmid_node(pkg, be, TY["q8_0"], 64, K_decl=48))           # K no multiple of the 32-weight block
    assert _supported(be, *_mmid_node(pkg, be, TY["q4_1"], 96, view_offset=20))          # (the fixture: the same view one block further in is taken)
    assert not _supported(be, *_mmid_node(pkg, be, TY["q4_1"], 96, view_offset=2))       # a Q4_1 base that is not 4-byte aligned: the form loads dwords


# ------------------------------------------------------------------------------------------------ 2. parity against the reference CPU backend
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


def _mmid_run(pkg, be_, ty, n_expert, n_used, T, M, K, bcast, wv, bv, idv, skip_experts=0):
    """skip_experts = 1: the experts are a view_3d over experts 1 .. n_expert of a tensor that holds n_expert + 2 (wv covers all of them).  -> [T, n_used, M]"""
    c = pkg.Context(be_)
    parent = c.new_tensor(ty, K, M, n_expert + 2 * skip_experts)
    as_ = c.view_3d(parent, K, M, n_expert, parent.nb[1], parent.nb[2], skip_experts * parent.nb[2]) if skip_experts else parent
    b = c.new_tensor(F32, K, 1 if bcast else n_used, T)
    wide = c.new_tensor(I32, idv.shape[1], T)
    ids = c.view_2d(wide, n_used, T, wide.nb[1], 0)
    y = c.mul_mat_id(as_, b, ids)
    c.alloc()
    assert be_.dev_s is None or be_.supports_op(y), "supports_op refused the node"      # (the reference backend is driven without a device object: nothing to ask)
    for t, v in ((parent, wv), (b, bv), (wide, idv)):
        be_.tensor_set(t, v)
    be_.graph_compute(c.graph())
    got = be_.tensor_get(y).copy().reshape(T, n_used, M)
    c.free()
    return got


def _inputs(name, n_expert, n_used, T, M, K, bcast, pattern, n_own=None, seed=0):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(seed + TY[name] * 100000 + n_expert * 1000 + n_used * 100 + T + M + K)
    wv = qwen3.random_blocks(rng, TY[name], M * (n_own or n_expert), K, std=0.05)
    bv = (rng.standard_normal((T, 1 if bcast else n_used, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    return rng, wv, bv, _ids(rng, pattern, n_expert, n_used, T)


def _check(pkg, be, ref_be, what, name, n_expert, n_used, T, M, K, bcast, wv, bv, idv, ref_idv=None, skip_experts=0):
    s0 = _counts(be)
    got = _mmid_run(pkg, be, TY[name], n_expert, n_used, T, M, K, bcast, wv, bv, idv, skip_experts)
    assert _delta(be, s0) == PER_PAIR                                 # one launch covers every (slot, token) pair; no other MoE counter moves
    want = _mmid_run(pkg, ref_be, TY[name], n_expert, n_used, T, M, K, bcast, wv, bv, idv if ref_idv is None else ref_idv, skip_experts)
    assert np.isfinite(want).all() and np.abs(want).max() > 0, "the fixture: the reference's own result is finite and not zero"
    e, pp = nmse(got, want), _pair_nmse(got, want)
    t, i = np.unravel_index(np.argmax(pp), pp.shape)
    print(f"MUL_MAT_ID {name} {what}: experts {n_expert} used {n_used} T {T} M {M} K {K} bcast {bcast}: NMSE {e:.3e}, worst pair (token {t}, slot {i}) {pp[t, i]:.3e}")
    assert np.isfinite(got).all()
    assert e <= BAR
    assert pp[t, i] <= BAR, (int(t), int(i), float(pp[t, i]))
    return got, want


# name, experts, used, T, M, K, b broadcast, id pattern, experts as a view from expert 1.  One case per edge, not a product: every form; 4 / 8 experts; 1 / 2 / 4 slots;
# 1 / 2 / 9 / 33 tokens; M = 70 is no multiple of the 2 rows a wave takes.  32-weight forms: K = 32 is one block (fewer than a wave step), 96 = three (rows of
# 102 / 54 / 66 / 60 / 72 bytes: none 16-byte aligned), 1408 = 44, 2880 = 90 (a ragged last stage).  Super-block forms: K = 256, 768, 2304 = nine super-blocks.
MMID_CASES = [
    ("q8_0", 8, 2, 1, 64, 32, True, "last", 0),
    ("q8_0", 4, 4, 9, 70, 96, False, "rand", 0),
    ("q8_0", 8, 4, 33, 70, 2880, False, "rand", 1),
    ("q8_0", 8, 1, 2, 64, 1408, True, "same", 0),
    ("q4_0", 8, 2, 33, 70, 96, True, "rand", 1),
    ("q4_0", 4, 1, 2, 64, 2880, False, "last", 0),
    ("q4_0", 8, 4, 9, 64, 1408, False, "same", 0),
    ("q5_0", 8, 4, 9, 70, 96, False, "same", 0),
    ("q5_0", 4, 2, 33, 64, 1408, True, "rand", 1),
    ("q5_0", 8, 2, 1, 70, 32, False, "last", 0),
    ("iq4_nl", 8, 1, 2, 70, 2880, True, "rand", 0),
    ("iq4_nl", 8, 4, 33, 64, 96, False, "last", 1),
    ("iq4_nl", 4, 2, 9, 70, 32, False, "same", 0),
    ("q4_1", 8, 2, 9, 70, 96, True, "last", 1),
    ("q4_1", 4, 4, 33, 64, 2880, False, "rand", 0),
    ("q4_1", 8, 1, 1, 70, 32, True, "same", 0),
    ("q5_1", 8, 4, 2, 64, 96, False, "rand", 0),
    ("q5_1", 8, 2, 33, 70, 1408, True, "same", 1),
    ("q5_1", 4, 1, 9, 70, 2880, False, "last", 0),
    ("iq4_xs", 8, 2, 1, 64, 256, True, "last", 0),
    ("iq4_xs", 4, 4, 33, 70, 2304, False, "rand", 1),
    ("iq4_xs", 8, 1, 9, 70, 768, True, "same", 0),
    ("q2_K", 8, 4, 9, 70, 256, False, "same", 1),
    ("q2_K", 4, 2, 33, 64, 2304, True, "rand", 0),
    ("q2_K", 8, 1, 2, 70, 768, False, "last", 0),
    ("q3_K", 8, 2, 33, 70, 768, True, "rand", 1),
    ("q3_K", 4, 1, 1, 64, 2304, False, "last", 0),
    ("q3_K", 8, 4, 2, 70, 256, False, "same", 0),
]


@pytest.mark.parametrize("name,n_expert,n_used,T,M,K,bcast,pattern,skip", MMID_CASES, ids=["-".join(str(v) for v in cs) for cs in MMID_CASES])
def test_mul_mat_id_blocks_vs_reference(pkg, be, ref_be, name, n_expert, n_used, T, M, K, bcast, pattern, skip):
    rng, wv, bv, idv = _inputs(name, n_expert, n_used, T, M, K, bcast, pattern, n_own=n_expert + 2 * skip)
    if pattern == "last":
        assert (idv[:, 0] == n_expert - 1).all()
    _check(pkg, be, ref_be, pattern, name, n_expert, n_used, T, M, K, bcast, wv, bv, idv, skip_experts=skip)


# ------------------------------------------------------------------------------------------------ 3. position independence, bit for bit
@pytest.mark.parametrize("name,K", [("q8_0", 2880), ("q4_1", 96), ("q3_K", 768)])
def test_mul_mat_id_blocks_position_independent_bit_for_bit(pkg, be, name, K):
    """the result of pair (t, i) in a launch of 33 x 2 pairs is the result of the same column and expert run alone at T = 1 (another grid, another workgroup)"""
    n_expert, n_used, T, M = 8, 2, 33, 70
    rng, wv, bv, idv = _inputs(name, n_expert, n_used, T, M, K, False, "rand", seed=9)
    full = _mmid_run(pkg, be, TY[name], n_expert, n_used, T, M, K, False, wv, bv, idv)
    assert np.isfinite(full).all() and np.abs(full).max() > 0
    for t in (0, 17, 32):
        alone = _mmid_run(pkg, be, TY[name], n_expert, n_used, 1, M, K, False, wv, bv[t:t + 1], idv[t:t + 1])
        assert np.array_equal(alone[0], full[t]), t


# ------------------------------------------------------------------------------------------------ 4. the clamp, in a form that cannot fault
@pytest.mark.parametrize("name,K", [("q5_0", 96), ("q2_K", 256)])
def test_mul_mat_id_blocks_out_of_range_ids_are_clamped(pkg, be, ref_be, name, K):
    """the experts are experts 1 .. 8 of a tensor of 10, every expert other random blocks.  Ids -3 and n_expert + 5 beside valid ones: clamped they name experts 0 and 7
    of the view, which is what the reference computes from the ids clipped on the host; unclamped they would name memory outside the view"""
    n_expert, n_used, T, M = 8, 4, 9, 70
    rng, wv, bv, idv = _inputs(name, n_expert, n_used, T, M, K, True, "rand", n_own=n_expert + 2, seed=3)
    bad = rng.random((T, n_used)) < 0.4
    idv[:, :n_used][bad] = rng.choice(np.array([-3, n_expert + 5], np.int32), int(bad.sum()))
    idv[0, :n_used] = (-3, n_expert + 5, 3, -3)
    sel = idv[:, :n_used]
    assert (sel == -3).sum() >= 2 and (sel == n_expert + 5).sum() >= 1 and ((sel >= 0) & (sel < n_expert)).sum() >= 3
    clipped = idv.copy()
    clipped[:, :n_used] = np.clip(sel, 0, n_expert - 1)
    _check(pkg, be, ref_be, "clamp", name, n_expert, n_used, T, M, K, True, wv, bv, idv, ref_idv=clipped, skip_experts=1)


# ------------------------------------------------------------------------------------------------ 5. the build_moe_ffn block, captured and replayed
def _separated_tokens(rng, gate_inp, T, n_used, gap=0.25):
    """T input rows whose router logits are well separated around the cut: the n_used + 1 largest of every token at least `gap` apart, so the expert choice does not
    sit on rounding"""
    rows = []
    while len(rows) < T:
        x = rng.standard_normal(gate_inp.shape[1]).astype(np.float32)
        top = np.sort(gate_inp.astype(np.float64) @ x)[::-1][: n_used + 1]
        if np.min(top[:-1] - top[1:]) >= gap:
            rows.append(x)
    return np.stack(rows)


def _block_run(pkg, be_, weights, types, xs):
    """runs the block once per input in xs on ONE graph (so a backend that captures graphs replays it); -> [(ids [T, n_used], out [T, n_embd])]"""
    from llama_cpp_omni_amd import qwen3moe
    blk = qwen3moe.MoeBlock(be_, weights=weights, gate_up_type=types[0], down_type=types[1])
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


MIXES = {"q4_0-q8_0": (TY["q4_0"], TY["q8_0"]), "q4_K-q5_0": (12, TY["q5_0"])}       # the second: what the quantiser falls back to when n_ff_exp is no multiple of 256


@pytest.fixture(scope="module")
def block_fixture(pkg, ref_be):
    """weights, inputs and the reference's results per type mix, computed once: tokens 1 and 5, four different inputs each (eager, capture, two replays)"""
    from llama_cpp_omni_amd import qwen3moe
    fx = {}
    for mix, types in MIXES.items():
        rng = np.random.default_rng(42 + types[1])
        blk = qwen3moe.MoeBlock(ref_be, seed=5, gate_up_type=types[0], down_type=types[1])
        weights = blk.weights
        blk.wctx.free()
        fx[mix] = {"weights": weights}
        for T in (1, 5):
            xs = [_separated_tokens(rng, weights["gate_inp"], T, 2) for _ in range(4)]
            fx[mix][T] = (xs, _block_run(pkg, ref_be, weights, types, xs))
    return fx


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("mix", list(MIXES))
def test_moe_ffn_block_blocks_eager_captured_replayed(pkg, be, block_fixture, mix, T):
    """the block eager (first submission), captured (second) and replayed (third, fourth), with a NEW router input at every submission so that other experts are
    chosen: the replay must follow the ids the launch reads from device memory"""
    xs, want = block_fixture[mix][T]
    assert len({tuple(w[0].ravel()) for w in want}) > 1               # (the fixture: the inputs do choose different experts)
    keys = ("mmv_id_blocks_launches", "mmv_id_launches", "graph_replays", "graph_captures")
    s0 = {k: be.get_stat(k) for k in keys}
    got = _block_run(pkg, be, block_fixture[mix]["weights"], MIXES[mix], xs)
    d = {k: be.get_stat(k) - s0[k] for k in keys}
    worst = 0.0
    for k, ((gi, go), (wi, wo)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), (k, gi, wi)
        e = nmse(go, wo)
        worst = max(worst, e)
        assert np.isfinite(go).all() and e <= 5e-4, (k, e)
    print(f"build_moe_ffn block {mix} T {T}: worst output NMSE over 4 submissions {worst:.3e}")
    # four submissions of one graph: eager, capture, two replays -- the launchers ran for the first two only (3 expert nodes each)
    n_blocks = 6 if mix == "q4_0-q8_0" else 2                         # q4_K-q5_0: gate and up on the K-quant kernel, down on the block-form kernel
    assert d == {"mmv_id_blocks_launches": n_blocks, "mmv_id_launches": 6 - n_blocks, "graph_replays": 2, "graph_captures": 1}, d
