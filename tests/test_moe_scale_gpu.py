"""The mixture-of-experts kernels at the structure of a real model (`-m gpu`): MUL_MAT_ID on the three id kernels (mmvk.hip k_mmv_id, mmv_mxfp4.hip,
mmq_id.hip k_moe_group / k_mmq_id) and ARGSORT (argsort.hip), through the backend C-ABI and against the reference CPU backend on the same graph.  The modules beside the
kernels (test_moe_ops_gpu, test_gptoss_ops_gpu, test_moe_mmq_id_gpu) run 4 - 32 experts, at most 388 pairs, K <= 2880, contiguous operands and distinct sort keys; this
one enters what only opens beyond that:
  the grouped kernel   k_mmq_id<8> (K >= 4096, the widest fold, a block count no multiple of 8), the Qwen3-30B-A3B configuration (128 experts, 8 used, 4096 pairs: KS = 1,
                       seven row tiles), every case with stat "mmq_id_ks" asserted so that a change of the launcher's rule cannot take a case off its path unnoticed;
  the grouping kernel  more than 1024 pairs (a second pass of both pair loops), more than 1024 experts (scan chunks of two), the expert limit 4096 and the per-pair
                       fall-back one expert behind it;
  operand forms        b->ne[1] strictly between 1 and n_ids, ids with nb[0] != 4, a b that is not flat (the token-by-token branch of prepare_act), a row-padded b;
  the id clamp         ids -1 and n_expert on experts that are a view into the middle of a larger tensor the test owns: a kernel that did not clamp would read the
                       neighbouring expert (other random blocks) and miss the bar -- it would not leave the tensor;
  ARGSORT              ties (the kernel's contract: the lower index first, in either order -- numpy's stable sort), +-inf, -0.0 / 0.0, NaN (a permutation is all that
                       is asked), and row lengths between 1024 and 16384 that are no power of two (padding slots under the multi-pass loop).

Bars: MUL_MAT_ID -- NMSE <= 1e-9 over the whole output, finite everywhere, AND NMSE <= 1e-9 for every (slot, token) pair on its own (a wrong slice is named, not
averaged away): the kernels form the reference's vec_dot integers, only the f32 order over the (at most 17) blocks differs, which bounds a pair near 1e-11.  ARGSORT --
exact equality.  No case skips or masks an element.
Measured on an MI355X, worst single pair of the module: k_mmq_id 1.1e-13 (the 1500-expert case; 5e-14 at the 4096-pair configuration), k_mmv_id 4.5e-14,
mmv_id_mxfp4 2.3e-14; whole outputs 7e-15 .. 2e-14."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, I32, MXFP4 = 0, 26, 39
TY = {"q4_K": 12, "q5_K": 13, "q6_K": 14, "mxfp4": MXFP4}
MIN_TOKENS = 64                                                       # MMQ_ID_MIN_TOKENS (graph_internal.hpp)
MAX_EXPERTS = 4096                                                    # MMQ_ID_MAX_EXPERTS (kernels.hpp)
STATS = ("mmq_id_launches", "mmv_id_launches", "mmv_id_mxfp4_launches")
GROUPED, PER_PAIR, PER_PAIR_MXFP4 = (1, 0, 0), (0, 1, 0), (0, 0, 1)
BAR = 1e-9


# ------------------------------------------------------------------------------------------------ one node, every operand form
def _node(pkg, be_, ty, n_expert, n_used, T, M, K, b_ne1, ids_form="rows", b_form="plain", skip_experts=0):
    """-> (context, node, feeds) with feeds(wv, bv, sel) -> [(tensor, array)].
    ids_form  rows: the first n_used columns of a wider [T, n_used + 3] tensor (as the top-k view of the argsort result); transposed: nb[0] = 4 * (T + 3), nb[1] = 4
    b_form    plain: [K, b_ne1, T]; slots: the first b_ne1 slots of a [K, b_ne1 + 1, T] tensor (not flat); rowpad: rows K + 32 floats wide
    skip_experts = 1: the experts are a view_3d over experts 1 .. n_expert of a tensor that holds n_expert + 2"""
    c = pkg.Context(be_)
    n_own = n_expert + 2 * skip_experts
    parent = c.new_tensor(ty, K, M, n_own)
    as_ = c.view_3d(parent, K, M, n_expert, parent.nb[1], parent.nb[2], skip_experts * parent.nb[2]) if skip_experts else parent
    if b_form == "plain":
        bt = b = c.new_tensor(F32, K, b_ne1, T)
        pad_b = lambda bv: bv
    elif b_form == "slots":
        bt = c.new_tensor(F32, K, b_ne1 + 1, T)
        b = c.view_3d(bt, K, b_ne1, T, bt.nb[1], bt.nb[2], 0)

        def pad_b(bv):
            full = np.full((T, b_ne1 + 1, K), 1e30, np.float32)
            full[:, :b_ne1] = bv
            return full
    elif b_form == "rowpad":
        bt = c.new_tensor(F32, K + 32, b_ne1, T)
        b = c.view_3d(bt, K, b_ne1, T, bt.nb[1], bt.nb[2], 0)

        def pad_b(bv):
            full = np.full((T, b_ne1, K + 32), 1e30, np.float32)
            full[..., :K] = bv
            return full
    else:
        raise ValueError(b_form)
    if ids_form == "rows":
        W = n_used + 3
        it = c.new_tensor(I32, W, T)
        ids = c.view_2d(it, n_used, T, it.nb[1], 0)

        def pad_ids(sel):
            full = np.zeros((T, W), np.int32)
            full[:, :n_used] = sel
            return full
    elif ids_form == "transposed":                                    # the transposed view of a [T + 3, n_expert] tensor: slot i of token t at 4 * ((T + 3) * i + t)
        Tw = T + 3
        it = c.new_tensor(I32, Tw, n_expert)
        ids = c._new(I32, (n_used, T), view_src=it, view_offs=0)
        ids.t.nb[0], ids.t.nb[1] = 4 * Tw, 4
        ids.t.nb[2] = ids.t.nb[3] = 4 * Tw * n_used

        def pad_ids(sel):
            full = np.zeros((n_expert, Tw), np.int32)
            full[:n_used, :T] = sel.T
            return full
    else:
        raise ValueError(ids_form)
    y = c.mul_mat_id(as_, b, ids)
    return c, y, lambda wv, bv, sel: [(parent, wv), (bt, pad_b(bv)), (it, pad_ids(sel))]


def _run(pkg, be_, ty, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, **form):
    c, y, feeds = _node(pkg, be_, ty, n_expert, n_used, T, M, K, b_ne1, **form)
    c.alloc()
    assert be_.dev_s is None or be_.supports_op(y), "supports_op refused the node"      # (the reference backend is driven without a device object: nothing to ask)
    for t, v in feeds(wv, bv, sel):
        be_.tensor_set(t, v)
    be_.graph_compute(c.graph())
    got = be_.tensor_get(y).copy().reshape(T, n_used, M)
    c.free()
    return got


def _pair_nmse(got, want):
    """NMSE of every (token, slot) pair on its own: [T, n_used]"""
    g, w = got.astype(np.float64), want.astype(np.float64)
    d, n = ((g - w) ** 2).sum(-1), (w ** 2).sum(-1)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


def _check(pkg, be, ref_be, what, name, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, expect, ks=None, ref_sel=None, **form):
    """runs the node on the device and on the reference (ref_sel: the ids the reference gets, where the device's are out of its range), asserts the launch
    counters, the K split where one is stated, and both bars; -> (got, want)"""
    ty = TY[name]
    s0 = [be.get_stat(k) for k in STATS]
    got = _run(pkg, be, ty, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, **form)
    assert tuple(int(be.get_stat(k) - v) for k, v in zip(STATS, s0)) == expect
    if ks is not None:
        assert be.get_stat("mmq_id_ks") == ks, (be.get_stat("mmq_id_ks"), ks)
    want = _run(pkg, ref_be, ty, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel if ref_sel is None else ref_sel, **form)
    assert np.isfinite(want).all() and np.abs(want).max() > 0, "the fixture: the reference's own result is finite and not zero"
    e, pp = nmse(got, want), _pair_nmse(got, want)
    t, i = np.unravel_index(np.argmax(pp), pp.shape)
    print(f"MUL_MAT_ID {what}: {name} experts {n_expert} used {n_used} T {T} M {M} K {K} b_ne1 {b_ne1} {form}: NMSE {e:.3e}, worst pair (token {t}, slot {i}, "
          f"expert {sel[t, i]}) {pp[t, i]:.3e}")
    assert np.isfinite(got).all()
    assert e <= BAR
    assert pp[t, i] <= BAR, (int(t), int(i), int(sel[t, i]), float(pp[t, i]))
    return got, want


def _operands(pkg, name, n_own, M, K, T, b_ne1, seed):
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(seed)
    wv = qwen3.random_blocks(rng, TY[name], M * n_own, K, std=0.05)
    bv = (rng.standard_normal((T, b_ne1, K)) * rng.choice([0.1, 1.0, 10.0])).astype(np.float32)
    return rng, wv, bv


def _rand_sel(rng, n_expert, n_used, T):
    """distinct experts per token, drawn from all of them"""
    return np.stack([rng.choice(n_expert, n_used, replace=False) for _ in range(T)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the statistic
def test_mmq_id_ks_stat_exists(be):
    assert be.get_stat("mmq_id_ks") in (0, 1, 2, 4, 8)                # 0: no grouped launch yet in this process


# ------------------------------------------------------------------------------------------------ grouped kernel: the missing instantiations
def _ks_rule(n_expert, n_used, T, M, K):
    """the launcher's rule (mmq_id.hip), restated: row tiles = ceil(M / 32), bound = min(pairs, experts) + pairs / 32"""
    pairs = n_used * T
    row_tiles, bound, nblk, ks = (M + 31) // 32, min(pairs, n_expert) + pairs // 32, K // 256, 1
    while ks < 8 and row_tiles * bound * ks * 2 <= 3072 and ks * 4 <= nblk:
        ks *= 2
    return ks


def _pattern(rng, pattern, n_expert, n_used, T):
    sel = np.empty((T, n_used), np.int32)
    if pattern == "edges":                                            # 33 + 31 pairs in slot 0, 32 + 32 in slot 1 (the last expert), the rest empty
        assert n_expert == 8 and n_used == 2 and T == 64
        sel[:33, 0] = 0; sel[33:, 0] = 1
        sel[:32, 1] = 2; sel[32:, 1] = 7
    elif pattern == "one":                                            # every pair names one expert: n_used * T pairs, twelve and more slices of it
        sel[:] = n_expert - 2
    elif pattern == "rand":
        sel[:] = _rand_sel(rng, n_expert, n_used, T)
    elif pattern == "ragged":                                         # slot s: runs of 1, 2, 3, ... tokens on experts s, s + 1, ... (slices of every width)
        for s in range(n_used):
            t, run, e = 0, 1, s
            while t < T:
                sel[t:t + run, s] = e % n_expert
                t += run; run += 1; e += 1
    elif pattern == "written":                                        # the 512-token case written out: expert 0 exactly 32 pairs, expert 1 33, expert 127 one, experts 107 .. 126 none
        assert n_expert == 128 and n_used == 8 and T == 512
        pool = np.arange(2, 107)
        for t in range(T):
            sel[t] = rng.choice(pool, n_used, replace=False)
        sel[:32, 0] = 0
        sel[32:65, 0] = 1
        sel[65, 0] = 127
    else:
        raise ValueError(pattern)
    return sel


# name, experts, used, T, M, K, b per slot, pattern, KS.  M = 70 / 200: a ragged last row tile.  K = 4096 / 4352: 16 / 17 blocks over the 8 waves of the widest fold.
SCALE_CASES = [
    ("q4_K", 8, 2, 64, 70, 4096, False, "edges", 8),                  # widest fold
    ("q6_K", 4, 4, 97, 70, 4352, True, "one", 8),                     # widest fold, ragged split: 17 blocks over 8 waves
    ("q5_K", 8, 2, 97, 64, 4096, True, "ragged", 8),                  # widest fold
    ("q4_K", 128, 8, 64, 70, 2048, False, "rand", 4),                 # many experts, few pairs each: one-group tiles
    ("q4_K", 128, 8, 512, 200, 2048, False, "rand", 1),               # the production configuration (gate / up), 4096 pairs: about 32 per expert, both sides of the slice edge
    ("q6_K", 128, 8, 512, 70, 768, True, "rand", 1),                  # the same on the down shape: 3 blocks < 4 per wave, so KS = 1 whatever the grid
    ("q4_K", 128, 8, 512, 200, 2048, False, "written", 1),            # exactly 32 / 33 / 1 pairs, 20 experts empty
]


@pytest.mark.parametrize("name,n_expert,n_used,T,M,K,per_slot,pattern,ks", SCALE_CASES, ids=["-".join(str(v) for v in cs) for cs in SCALE_CASES])
def test_grouped_at_scale_vs_reference(pkg, be, ref_be, name, n_expert, n_used, T, M, K, per_slot, pattern, ks):
    assert _ks_rule(n_expert, n_used, T, M, K) == ks                  # (the fixture: the shape does reach the stated split under the launcher's rule)
    b_ne1 = n_used if per_slot else 1
    rng, wv, bv = _operands(pkg, name, n_expert, M, K, T, b_ne1, seed=n_expert * 1000 + n_used * 100 + T + M + K)
    sel = _pattern(rng, pattern, n_expert, n_used, T)
    cnt = np.bincount(sel.ravel(), minlength=n_expert)
    if pattern == "written":
        assert cnt[0] == 32 and cnt[1] == 33 and cnt[127] == 1 and (cnt == 0).sum() >= 20
    if T == 512:
        assert (cnt > 32).any() and ((cnt > 0) & (cnt < 32)).any()      # (the fixture: slices on both sides of the 32-column edge)
    _check(pkg, be, ref_be, f"grouped {pattern}", name, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, GROUPED, ks=ks)


# ------------------------------------------------------------------------------------------------ grouping kernel: scan and limits
def test_group_scan_chunks_of_two_1500_experts(pkg, be, ref_be):
    """1500 experts: every scan thread owns two; 1280 pairs: a second pass of both pair loops.  The used experts sit on both sides of a chunk and of the
    boundary between threads 511 | 512; expert 1 takes 33 pairs (a second slice), the others 178 or 179"""
    name, n_expert, n_used, T, M, K = "q4_K", 1500, 2, 640, 32, 256
    used = [0, 1, 1022, 1023, 1024, 1025, 1498, 1499]
    rng, wv, bv = _operands(pkg, name, n_expert, M, K, T, 1, seed=1500)
    flat = [1] * 33
    rest = [e for e in used if e != 1]
    for k in range(n_used * T - 33):
        flat.append(rest[k % len(rest)])
    flat = np.sort(np.array(flat, np.int32))                          # entries 640 apart name different experts (none has more than 640 pairs): distinct per token
    sel = np.stack([flat[:T], flat[T:]], axis=1)[rng.permutation(T)]
    cnt = np.bincount(sel.ravel(), minlength=n_expert)
    assert sorted(np.nonzero(cnt)[0].tolist()) == used and cnt[1] == 33 and (sel[:, 0] != sel[:, 1]).all()
    _check(pkg, be, ref_be, "1500 experts", name, n_expert, n_used, T, M, K, 1, wv, bv, sel, GROUPED, ks=1)


def test_tile_table_filled_to_its_bound(pkg, be, ref_be):
    """136 pairs on 8 experts: the table has min(136, 8) + 136 / 32 = 12 entries, and 129 pairs on expert 3 (five slices, the last of one column) with one pair on
    each of the other seven make exactly 12 tiles -- the last entry, directly in front of the pair list, is written and read"""
    name, n_expert, n_used, T, M, K = "q4_K", 8, 2, 68, 32, 256
    rng, wv, bv = _operands(pkg, name, n_expert, M, K, T, n_used, seed=68)
    sel = np.full((T, n_used), 3, np.int32)
    sel[61:, 1] = [0, 1, 2, 4, 5, 6, 7]
    cnt = np.bincount(sel.ravel(), minlength=n_expert)
    assert ((cnt + 31) // 32).sum() == min(n_used * T, n_expert) + n_used * T // 32 == 12
    _check(pkg, be, ref_be, "tile bound", name, n_expert, n_used, T, M, K, n_used, wv, bv, sel, GROUPED, ks=1)


@pytest.mark.parametrize("n_expert,expect", [(MAX_EXPERTS, GROUPED), (MAX_EXPERTS + 1, PER_PAIR)], ids=["4096-grouped", "4097-per-pair"])
def test_expert_limit_both_sides(pkg, be, ref_be, n_expert, expect):
    """the admission limit of the grouped path: at 4096 experts it runs (scan chunks of four), one more and the same node takes the per-pair kernel"""
    name, n_used, T, M, K = "q4_K", 2, MIN_TOKENS, 32, 256
    rng, wv, bv = _operands(pkg, name, n_expert, M, K, T, 1, seed=n_expert)
    sel = _rand_sel(rng, n_expert, n_used, T)
    sel[0] = (0, n_expert - 1)                                        # the first and the last expert are used
    sel[5] = (n_expert - 1, 1023)
    _check(pkg, be, ref_be, "expert limit", name, n_expert, n_used, T, M, K, 1, wv, bv, sel, expect, ks=1 if expect == GROUPED else None)


# ------------------------------------------------------------------------------------------------ operand forms, on each id kernel
KERNELS = {                                                           # name, experts, M, K, T -> the kernel the route takes
    "k_mmv_id": ("q4_K", 8, 70, 768, 9, PER_PAIR),
    "k_mmq_id": ("q4_K", 8, 70, 768, 64, GROUPED),
    "mmv_id_mxfp4": ("mxfp4", 8, 70, 2880, 9, PER_PAIR_MXFP4),
}
FORMS = {                                                             # b_ne1 (of n_used = 4), form
    "b_ne1_2_of_4": (2, {}),
    "ids_transposed": (4, {"ids_form": "transposed"}),
    "b_not_flat": (4, {"b_form": "slots"}),
    "b_row_padded": (4, {"b_form": "rowpad"}),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_operand_forms_vs_reference(pkg, be, ref_be, kernel, form):
    name, n_expert, M, K, T, expect = KERNELS[kernel]
    b_ne1, kw = FORMS[form]
    n_used = 4
    rng, wv, bv = _operands(pkg, name, n_expert, M, K, T, b_ne1, seed=K + T + b_ne1)
    sel = _rand_sel(rng, n_expert, n_used, T)
    got, want = _check(pkg, be, ref_be, f"{kernel} {form}", name, n_expert, n_used, T, M, K, b_ne1, wv, bv, sel, expect, **kw)
    assert np.abs(want).max() < 1e20                                  # (the fixture: nothing read the 1e30 padding of b)
    if form == "b_ne1_2_of_4":                                        # (the fixture: slots 0 / 2 and 1 / 3 read two different columns, so a wrong i % b_ne1 shows)
        assert not np.array_equal(bv[:, 0], bv[:, 1])


# ------------------------------------------------------------------------------------------------ the clamp, in a form that cannot fault
CLAMP = {
    "k_mmv_id-T9": ("q4_K", 768, 9, PER_PAIR),
    "k_mmq_id-T64": ("q4_K", 768, 64, GROUPED),
    "mmv_id_mxfp4-T9": ("mxfp4", 2880, 9, PER_PAIR_MXFP4),
    "mmv_id_mxfp4-T64": ("mxfp4", 2880, 64, PER_PAIR_MXFP4),
}


@pytest.mark.parametrize("case", list(CLAMP))
def test_out_of_range_ids_are_clamped(pkg, be, ref_be, case):
    """the experts are experts 1 .. 8 of a tensor of 10, every expert other random blocks.  Ids -1 and 8 (no other out-of-range value) beside valid ones: clamped
    they name experts 0 and 7 of the view, which is what the reference computes from the ids clipped on the host; unclamped they would name experts 0 and 9 of the
    PARENT -- memory this test owns, other weights, another result"""
    name, K, T, expect = CLAMP[case]
    n_expert, n_used, M = 8, 4, 70
    rng, wv, bv = _operands(pkg, name, n_expert + 2, M, K, T, 1, seed=K + T)
    sel = _rand_sel(rng, n_expert, n_used, T)
    bad = rng.random((T, n_used)) < 0.4
    sel[bad] = rng.choice(np.array([-1, n_expert], np.int32), int(bad.sum()))
    sel[0] = (-1, n_expert, 3, -1)
    assert (sel == -1).sum() >= 3 and (sel == n_expert).sum() >= 3 and ((sel >= 0) & (sel < n_expert)).sum() >= 3 and sel.min() == -1 and sel.max() == n_expert
    clipped = np.clip(sel, 0, n_expert - 1)
    got, want = _check(pkg, be, ref_be, f"clamp {case}", name, n_expert, n_used, T, M, K, 1, wv, bv, sel, expect, ref_sel=clipped, skip_experts=1)
    # (the fixture: the neighbours do hold other weights -- the reference on the parent's experts 0 and 9 in place of the view's 0 and 7 misses the bar by far)
    blocks = wv.reshape(n_expert + 2, -1)
    stray = np.concatenate([blocks[1:-1], blocks[-1:], blocks[:1]])   # view experts 0 .. 7, then "expert 8" = the parent's last and "expert 9" = the parent's first
    unclamped = np.where(sel == -1, n_expert + 1, sel)
    other = _run(pkg, ref_be, TY[name], n_expert + 2, n_used, T, M, K, 1, stray.reshape(wv.shape[0], -1), bv, unclamped)
    assert _pair_nmse(other, want)[(sel == -1) | (sel == n_expert)].min() > 1e-3


# ------------------------------------------------------------------------------------------------ ARGSORT's stated contract
ARGSORT_NE0 = [1, 2, 60, 128, 129, 1500, 5000, 16384]


def _argsort_run(pkg, be_, xv, order):
    ne0 = xv.shape[-1]
    c = pkg.Context(be_)
    x = c.new_tensor(F32, ne0, 3, 2, 2)
    y = c.argsort(x, order)
    c.alloc()
    assert be_.dev_s is None or be_.supports_op(y)
    be_.tensor_set(x, xv)
    be_.graph_compute(c.graph())
    got = be_.tensor_get(y).copy().reshape(2, 2, 3, ne0)
    c.free()
    return got


def _tie_rows(ne0, seed):
    """12 rows: 0 - 3 heavy ties (integers 0 .. 3), 4 all equal, 5 - 7 +-inf among finite values (and among ties), 8 - 9 only -0.0 and 0.0, 10 - 11 all of it"""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, 4, ne0).astype(np.float32) for _ in range(4)]
    rows.append(np.full(ne0, 2.5, np.float32))
    for k in range(3):
        r = rng.standard_normal(ne0).astype(np.float32) if k == 0 else rng.integers(0, 4, ne0).astype(np.float32)
        m = rng.random(ne0)
        r[m < 0.25] = np.inf
        r[m > 0.75] = -np.inf
        rows.append(r)
    for _ in range(2):
        rows.append(np.where(rng.random(ne0) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32))
    for _ in range(2):
        r = rng.integers(-1, 2, ne0).astype(np.float32)
        m = rng.random(ne0)
        r[m < 0.15] = np.inf
        r[(m >= 0.15) & (m < 0.3)] = -np.inf
        r[(m >= 0.3) & (m < 0.45)] = -0.0
        rows.append(r)
    return np.stack(rows).reshape(2, 2, 3, ne0)


@pytest.mark.parametrize("order", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("ne0", ARGSORT_NE0)
def test_argsort_ties_and_specials_lower_index_first(pkg, be, ne0, order):
    xv = _tie_rows(ne0, 300 + ne0)
    if ne0 >= 60:
        assert np.isinf(xv).any() and np.signbit(xv[xv == 0]).any() and not np.signbit(xv[xv == 0]).all()      # (the fixture)
    got = _argsort_run(pkg, be, xv, order)
    want = np.argsort(xv if order == 0 else -xv, axis=-1, kind="stable").astype(np.int32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("order", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("ne0", ARGSORT_NE0)
def test_argsort_nan_rows_are_permutations(pkg, be, ne0, order):
    """NaN compares false with everything, so no order is promised -- but the network only ever exchanges slots: every row is a permutation of 0 .. ne0 - 1"""
    rng = np.random.default_rng(400 + ne0)
    xv = rng.integers(0, 4, (2, 2, 3, ne0)).astype(np.float32)
    xv[rng.random(xv.shape) < 0.3] = np.nan
    xv[0, 0, 0] = np.nan                                              # one row of nothing else
    got = _argsort_run(pkg, be, xv, order)
    assert np.array_equal(np.sort(got, axis=-1), np.broadcast_to(np.arange(ne0, dtype=np.int32), got.shape))


@pytest.mark.parametrize("order", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("ne0", [1500, 5000])
def test_argsort_distinct_multi_pass_padded_rows(pkg, be, ref_be, ne0, order):
    """1500 -> 2048 and 5000 -> 8192 slots: 548 / 3192 padding slots, 1024 / 4096 comparisons per step on 1024 threads"""
    rng = np.random.default_rng(500 + ne0)
    xv = np.stack([rng.permutation(ne0) for _ in range(12)]).astype(np.float32).reshape(2, 2, 3, ne0)
    got = _argsort_run(pkg, be, xv, order)
    want = _argsort_run(pkg, ref_be, xv, order)
    assert np.array_equal(want, np.argsort(xv if order == 0 else -xv, axis=-1).astype(np.int32))      # (the fixture: distinct values leave one answer)
    assert np.array_equal(got, want)
