"""MUL_MAT_ID on BF16 and F32 experts (`-m gpu`; kernels/mm_id_f.hip): the per-pair mat-vec k_mmv_id_f and, for BF16 experts from MM_ID_BF16_MIN_TOKENS tokens on, the
expert-grouped bf16-MFMA kernel k_mm_id_16, through the backend C-ABI.  Reference: float64 numpy on the bf16 weight values and on activations rounded to bf16 as
ggml_compute_fp32_to_bf16 does (F32 experts: unrounded).  Bar: NMSE <= 1e-9 over the whole output AND for every (token, slot) pair on its own -- the project's bar for
F16 / F32 / BF16 weights (test_mul_mat_layouts_gpu.py): both sides sum the same exact products, only the f32 order differs.  Two grouped cases also run on the reference
CPU backend, which pins the rounding rule.  Weights at std 0.05, activations at scale 0.1 / 1 / 10: nothing is subnormal in bf16 (whether the bf16 MFMA flushes subnormal
inputs is not checked here).  The block test uses the project's bar for the build_moe_ffn block (test_moe_ops_gpu.py: ids equal, output NMSE <= 5e-4)."""
import numpy as np
import pytest
from conftest import nmse

pytestmark = pytest.mark.gpu
F32, I32, BF16 = 0, 26, 30
MIN_TOKENS = 32                                                       # MM_ID_BF16_MIN_TOKENS (graph_internal.hpp)
STATS = ("mmv_id_f_launches", "mm_id_bf16_launches", "mmv_id_launches", "mmq_id_launches", "mmv_id_blocks_launches", "mmq_id_blocks_launches", "mmv_id_mxfp4_launches", "mmq_id_mxfp4_launches")
PER_PAIR, GROUPED = (1, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0)

def _to_bf16(x):                                                      # round to nearest even (no NaN among the inputs)
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)

def _value(ty, a):                                                    # what the tensor's bits mean, in float64
    return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64) if ty == BF16 else a.astype(np.float64)

def _inputs(ty, n_used, T, M, K, b_ne1, seed=0):      # -> rng, the 8 experts as the tensor holds them [8, M, K], b [T, b_ne1, K]
    rng = np.random.default_rng(seed + ty * 100000 + n_used * 1000 + T + M + K)
    w = (rng.standard_normal((8, M, K)) * 0.05).astype(np.float32)
    return rng, _to_bf16(w) if ty == BF16 else w, (rng.standard_normal((T, b_ne1, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)

def _ref(ty, raw, bv, sel):
    w, x = _value(ty, raw), _value(ty, _to_bf16(bv) if ty == BF16 else bv)
    e = np.clip(sel, 0, 7)                                            # (the kernels clamp an id before it becomes an address)
    return np.stack([np.stack([w[e[t, i]] @ x[t, i % x.shape[1]] for i in range(sel.shape[1])]) for t in range(sel.shape[0])])

def _run(pkg, be_, ty, raw, bv, sel, times=1, offset=0):
    """ids: a strided view of a WIDER i32 tensor; offset: the experts as a view_3d that many bytes into a tensor one expert larger.  -> (results [T, n_used, M], counter deltas)"""
    (_, M, K), (T, n_used), b_ne1 = raw.shape, sel.shape, bv.shape[1]
    c = pkg.Context(be_)
    big = c.new_tensor(ty, K, M, 8 + (1 if offset else 0))
    as_ = c.view_3d(big, K, M, 8, big.nb[1], big.nb[2], offset) if offset else big
    b, wide = c.new_tensor(F32, K, b_ne1, T), c.new_tensor(I32, n_used + 3, T)
    y = c.mul_mat_id(as_, b, c.view_2d(wide, n_used, T, wide.nb[1], 0))
    c.alloc()
    assert be_.dev_s is None or be_.supports_op(y), "supports_op refused the node"
    full = np.pad(sel, ((0, 0), (0, 3)))
    be_.tensor_set(big, raw, offset=offset); be_.tensor_set(b, bv); be_.tensor_set(wide, full)
    stat = be_.get_stat if be_.dev_s is not None else (lambda k: 0)       # (the reference backend has no counters)
    s0, res = [stat(k) for k in STATS], []
    for _ in range(times):
        be_.graph_compute(c.graph())
        res.append(be_.tensor_get(y).copy().reshape(T, n_used, M))
    c.free()
    return (res if times > 1 else res[0]), tuple(int(stat(k) - s) for k, s in zip(STATS, s0))

def _assert_bar(what, got, want):
    g, w = got.astype(np.float64), want.astype(np.float64)
    pp, e = ((g - w) ** 2).sum(-1) / (w ** 2).sum(-1), nmse(got, want)      # every (token, slot) pair on its own; the whole output
    print(f"MUL_MAT_ID {what}: NMSE {e:.3e}, worst pair {pp.max():.3e}")
    assert np.isfinite(got).all() and np.abs(want).max() > 0 and e <= 1e-9 and pp.max() <= 1e-9, (e, float(pp.max()), np.unravel_index(np.argmax(pp), pp.shape))

def _node(pkg, be, ty, K, K_decl=None):
    c = pkg.Context(be)
    as_, b = c.new_tensor(ty, K, 2, 8), c.new_tensor(F32, K, 1, 3)
    as_.t.ne[0] = b.t.ne[0] = K if K_decl is None else K_decl         # (K_decl: a row length declared on tensors that own room for more)
    y = c.mul_mat_id(as_, b, c.view_2d(c.new_tensor(I32, 8, 3), 2, 3, 32, 0))
    c.alloc(); ok = bool(be.supports_op(y)); c.free()
    return ok

def test_supports_op_takes_bf16_and_f32_experts(pkg, be):
    assert _node(pkg, be, BF16, 256) and _node(pkg, be, F32, 256) and _node(pkg, be, BF16, 50) and _node(pkg, be, F32, 1)
    assert _node(pkg, be, BF16, 77840, K_decl=77824)                  # 152 KiB of bf16: the last column that fits LDS
    assert not _node(pkg, be, BF16, 77840, K_decl=77832) and not _node(pkg, be, F32, 38920, K_decl=38916)

# K = 8: one 16-byte chunk of bf16; 520: one chunk past a 64-lane step of 512 elements; 50: the element-wise path (rows 100 B / 200 B apart); 2880.  "view": the experts one element into their tensor (an unaligned base: no 16-byte loads); "ids": an id of n_expert and of -1 (_ref clamps as the kernel does)
@pytest.mark.parametrize("K,T,b_ne1,mode", [(K, T, b, "") for K in (8, 520, 50, 2880) for T, b in ((1, 1), (5, 2))] + [(520, 5, 1, "view"), (520, 5, 1, "ids")])
@pytest.mark.parametrize("ty", [BF16, F32], ids=["bf16", "f32"])
def test_per_pair(pkg, be, ty, K, T, b_ne1, mode):
    rng, raw, bv = _inputs(ty, 2, T, 70, K, b_ne1)
    sel = np.stack([rng.permutation(8)[:2] for _ in range(T)]).astype(np.int32)
    if mode == "ids": sel[1, 0], sel[3, 1] = 8, -1
    got, d = _run(pkg, be, ty, raw, bv, sel, offset=(2 if ty == BF16 else 4) if mode == "view" else 0)
    assert d == PER_PAIR
    _assert_bar(f"per-pair type {ty} K {K} T {T} b_ne1 {b_ne1} {mode}", got, _ref(ty, raw, bv, sel))

def _pattern(pattern, n_used, T):
    sel = np.empty((T, n_used), np.int32)
    if pattern == "edges":                                            # slot 0: 33 + 31 + 64 pairs on experts 0, 1, 3; slot 1: 32 + 96 on expert 2 and the last; 4, 5, 6 empty
        sel[:33, 0] = 0; sel[33:64, 0] = 1; sel[64:, 0] = 3; sel[:32, 1] = 2; sel[32:, 1] = 7
        assert np.bincount(sel.ravel(), minlength=8).tolist() == [33, 31, 32, 64, 0, 0, 0, 96]
    else:                                                             # "ragged" -- slot s: runs of 1, 2, 3, ... tokens on experts s, s + 1, ... (slices of every width)
        for s in range(n_used):
            t, run, e = 0, 1, s
            while t < T:
                sel[t:t + run, s] = e % 8
                t += run; run += 1; e += 1
    return sel

# n_used, T, M, K, b_ne1, pattern, the KS the shape reaches under the launcher's rule (asserted through the stat mm_id_bf16_ks), also against the reference CPU backend.  K = 16 / 48 / 2880 / 4096: one MFMA step, three, 180, a power of two (256: a two-wave split)
CASES = [(2, 128, 70, 16, 1, "edges", 1, False), (2, 128, 64, 2880, 2, "edges", 8, True), (4, 161, 64, 48, 4, "ragged", 1, True),
         (2, 161, 70, 4096, 1, "ragged", 8, False), (4, 128, 70, 2880, 2, "ragged", 8, False), (4, 128, 70, 256, 1, "ragged", 2, False)]

@pytest.mark.parametrize("n_used,T,M,K,b_ne1,pattern,ks,vs_ref", CASES, ids=["-".join(str(v) for v in cs[:7]) for cs in CASES])
def test_grouped(pkg, be, request, n_used, T, M, K, b_ne1, pattern, ks, vs_ref):
    assert {cs[6] for cs in CASES} >= {1, 8}                          # (the fixture: KS = 1 and a KS > 1 over the set)
    rng, raw, bv = _inputs(BF16, n_used, T, M, K, b_ne1)
    sel = _pattern(pattern, n_used, T)
    got, d = _run(pkg, be, BF16, raw, bv, sel)
    assert d == GROUPED and be.get_stat("mm_id_bf16_ks") == ks
    _assert_bar(f"grouped {pattern} used {n_used} T {T} M {M} K {K} b_ne1 {b_ne1} KS {ks}", got, _ref(BF16, raw, bv, sel))
    if vs_ref:
        _assert_bar("... against the reference CPU backend", got, _run(pkg, request.getfixturevalue("ref_be"), BF16, raw, bv, sel)[0])

def test_route(pkg, be):
    def go(ty, T, K):
        rng, raw, bv = _inputs(ty, 2, T, 64, K, 1)
        return _run(pkg, be, ty, raw, bv, np.stack([rng.permutation(8)[:2] for _ in range(T)]).astype(np.int32))
    on, d = go(BF16, MIN_TOKENS, 32)
    assert d == GROUPED                                               # at the threshold; the grouping and the matrix launch count as one
    be.set_option("mmq_id", 0)
    try:
        off, d = go(BF16, MIN_TOKENS, 32)
    finally:
        be.set_option("mmq_id", 1)
    assert d == PER_PAIR
    _assert_bar("grouped against per-pair (mmq_id = 0)", on, off)
    # per-pair: one token fewer; K no multiple of an MFMA step; F32 experts (no grouped kernel)
    assert go(BF16, MIN_TOKENS - 1, 32)[1] == PER_PAIR and go(BF16, MIN_TOKENS, 24)[1] == PER_PAIR and go(F32, MIN_TOKENS, 32)[1] == PER_PAIR

def test_grouped_position_independent_bit_for_bit(pkg, be):
    rng, raw, bv = _inputs(BF16, 2, 161, 70, 2880, 2, seed=9)
    sel = _pattern("ragged", 2, 161)
    (a1, a2), _ = _run(pkg, be, BF16, raw, bv, sel, times=2)
    assert np.array_equal(a1, a2)                                     # two submissions of the identical inputs
    perm = np.random.default_rng(1).permutation(161)                  # token t of the second run is token perm[t] of the first: other slices, other slice positions
    p1, d = _run(pkg, be, BF16, raw, bv[perm], sel[perm])
    assert d == GROUPED and np.isfinite(a1).all() and np.abs(a1).max() > 0 and np.array_equal(p1, a1[perm])

@pytest.mark.parametrize("T,stat", [(1, "mmv_id_f_launches"), (128, "mm_id_bf16_launches")])
def test_moe_ffn_block_bf16(pkg, be, ref_be, T, stat):
    from llama_cpp_omni_amd import qwen3moe
    E, X, F = (qwen3moe.TINY_MOE[k] for k in ("n_embd", "n_expert", "n_ff_exp"))
    rng = np.random.default_rng(17 + T)
    bits = lambda rows, K: _to_bf16((rng.standard_normal((rows, K)) * 0.05).astype(np.float32))      # (random_blocks has no BF16 form: raw 16-bit words from f32 bits)
    weights = dict(gate_inp=(rng.standard_normal((X, E)) / np.sqrt(E)).astype(np.float32), up_exps=bits(F * X, E), gate_exps=bits(F * X, E), down_exps=bits(E * X, F))
    rows = []
    while len(rows) < T:                                              # router logits well separated around the cut: the expert choice does not sit on rounding
        x = rng.standard_normal(E).astype(np.float32)
        top = np.sort(weights["gate_inp"].astype(np.float64) @ x)[::-1][:3]
        if np.min(top[:-1] - top[1:]) >= 0.25:
            rows.append(x)
    res, s0 = [], be.get_stat(stat)
    for b_ in (be, ref_be):
        blk = qwen3moe.MoeBlock(b_, weights=weights, gate_up_type=BF16, down_type=BF16)
        g, x, N = blk.build(T)
        b_.tensor_set(x, np.stack(rows))
        b_.graph_compute(g.graph())
        res.append((b_.tensor_get(N["argsort"]).copy().reshape(T, -1)[:, :2], b_.tensor_get(N["moe_out"]).copy().reshape(T, -1)))
        g.free(); blk.wctx.free()
    assert be.get_stat(stat) - s0 == 3                                # gate, up and down on the GPU, each on the path its token count takes
    e = nmse(res[0][1], res[1][1]); print(f"build_moe_ffn block, BF16 experts, T {T}: output NMSE {e:.3e}")
    assert np.array_equal(res[0][0], res[1][0]) and np.isfinite(res[0][1]).all() and e <= 5e-4
