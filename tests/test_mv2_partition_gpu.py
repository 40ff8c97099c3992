"""The row partition of the LDS-DMA decode mat-vec engine (mmv2.hip k_mv2, `-m gpu`, through the C-ABI): ragged row counts, uneven groups, rows < CUs,
the residual staging limit -- every launch form at shapes where workgroups get q and q + 1 rows, where the last row group of a block-per-lane consumer
is short, where a workgroup has one task or none.  Each case runs on the engine (option mv2 = 1) and on the register family (mv2 = 0), both against the
C oracle (oracle_py.mul_mat, rms_norm where a norm is folded); stat "mv2_launches" says which family ran.

Bars: NMSE against the oracle < 1e-9 and engine against register family < 1e-12 (K-quants) / < 1e-11 (Q8_0) on the whole result -- the project's bars
for these kernels (test_round3_gpu.py, test_round4_gpu.py) -- and the 1e-9 oracle bar on EVERY slice of 64 consecutive output rows as well: a wrong
workgroup or a dropped last row of a group must not be averaged away over tens of thousands of rows.  (Both sides form the same integer sums; only the
f32 order over at most 48 super-block partials differs: ~1e-13 expected.)  Three computes of the engine graph are bit-identical (a ring slot re-used too
early shows as run-to-run differences), and every output is pre-filled with NaN, so a row nobody wrote is seen.

`mv2_plan_py` restates mmv2.hip's mv2_plan; the literal shapes are chosen for 256 CUs, the ids show (q, r) per matrix there, and every case asserts the
property it is named for from the restated plan at the device's own CU count (stat "mv2_cus") -- or skips, with the reason, where the property is lost.

What the cases would catch (by reading, not by running broken code): with `valid` forced true in mv2_consume_q4k_h the lane r = 1 of a short last group
stores row jl's sum over the NEXT workgroup's first row (a: four workgroups of 17 rows) -- a slice error of ~1/64; with the `+ (lw < M.r ? 1 : 0)` dropped
from ntask the first r workgroups never write their last row -- NaN stays in a (r = 4), c (r = 116) and f at 5000 rows (r = 136).

Case n -- a workgroup with NO task (rows (128, 64, 64), Q4_K / Q4_K / Q6_K on 256 CUs: 93 / 47 / 116 workgroups, the Q6_K member q = 0, r = 64, so 52 of
its workgroups have ntask = 0).  Trace of k_mv2 with ntask = 0, G0 = nrows:
  * loader: wbytes = (G0 + 0) w_rs = the whole matrix, a valid descriptor nothing is requested through; T = 0: MV2_PRE issues nothing, mv2_await(rows_issued, RWN)
    completes because the row waves arrive there whatever ntask is; `while (n < T)` is not entered; mv2_drain::go(0, ..) has n > K_ false at every K_, so
    neither a wait nor a poke: nothing was issued, nothing can land late.
  * row loaders: the activation row (and norm weights) as always; the residual loop `b * 64 < ntask` runs zero times (and a packed group has none); all three
    arrivals (rows_issued, x_landed, rows_landed) happen.
  * prologue waves: wait for x_landed / rows_landed (above), build the image, img_cnt reaches 4 NIT = img_need (or C with a ready image: every consumer copies
    and arrives); every consumer's wait on img_cnt completes.
  * consumers: q4k_b / q4k_h have ng = (0 + GR - 1) / GR = 0, the others `j = c < 0` false: no loop body, no mv2_wait_step, no poke; mv2_out_flush stores
    `lane < 0` lanes: nothing.  The residual read is behind `r < ntask`.
Every wait completes and nothing is stored: the plan stays as it is, and case n runs."""
import numpy as np
import pytest

from conftest import nmse
from oracle import oracle_py as orc
from test_round3_gpu import _act, _silu

pytestmark = pytest.mark.gpu

Q8_0, Q4_K, Q6_K = 8, 12, 14                                  # ggml_type (asserted against the package in _check_types)
TNAME = {Q4_K: "q4_K", Q6_K: "q6_K", Q8_0: "q8_0"}
STEP_BYTES = {Q4_K: 144, Q6_K: 210, Q8_0: 272}               # bytes of 256 weights
MV2_Q6_SHARE = 1.7
SLICE = 64


def mv2_plan_py(rows, types, K, cus):
    """mmv2.hip mv2_plan, restated: per matrix (first workgroup, workgroups, q, r) -- workgroup lw of a matrix owns rows lw q + min(lw, r) .. + q + (lw < r).
    A gate / up pair is one matrix (a task = a row of each).  Asserts what the launch relies on: every row owned exactly once, q and r in 16 bits, first
    workgroups in 12."""
    nmat = len(rows)
    assert 1 <= nmat <= 3 and len(types) == nmat and all(m > 0 for m in rows)
    bts = [float(m) * float(STEP_BYTES[t]) * float(K // 256) for m, t in zip(rows, types)]
    if nmat > 1:
        bts = [b * MV2_Q6_SHARE if t == Q6_K else b for b, t in zip(bts, types)]
    total = 0.0
    for b in bts:
        total += b
    grid = max(min(sum(rows), cus), nmat)
    plan, acc_w, acc_b = [], 0, 0.0
    for i in range(nmat):
        acc_b += bts[i]
        end = grid if i == nmat - 1 else int(grid * (acc_b / total) + 0.5)
        end = max(end, acc_w + 1)
        end = min(end, grid - (nmat - 1 - i))
        nwg = end - acc_w
        assert nwg >= 1
        q, r = divmod(rows[i], nwg)
        nxt = 0
        for lw in range(nwg):                                 # every row exactly once, in order
            g0 = lw * q + min(lw, r)
            assert g0 == nxt
            nxt = g0 + q + (1 if lw < r else 0)
        assert nxt == rows[i]
        assert q <= 0xffff and r <= 0xffff and acc_w <= 0xfff
        plan.append((acc_w, nwg, q, r))
        acc_w = end
    assert acc_w == grid and grid <= 4095
    return plan


def _qr(plan):
    return "".join(f"[q{q}r{r}]" for _, _, q, r in plan)


def _ntasks(p):
    """the task counts the workgroups of one matrix run with"""
    _, nwg, q, r = p
    return ([q + 1] if r else []) + ([q] if r < nwg else [])


# ------------------------------------------------------------------------------------------------ shared weights, activations and oracle results
# one random block matrix per (type, K), generated once; a case takes a row range of it, and the oracle's product for a row is computed once
MAXROWS = {(Q4_K, 4096): 32000, (Q6_K, 4096): 32000, (Q8_0, 4096): 22016, (Q4_K, 12288): 16500, (Q6_K, 12288): 16500}
_W, _X, _ORC = {}, {}, {}


def _weights(ty, K):
    if (ty, K) not in _W:
        from llama_cpp_omni_amd import qwen3
        wv = qwen3.random_blocks(np.random.default_rng(1000 * ty + K), ty, MAXROWS[(ty, K)], K, std=0.05)
        wv = wv.view(np.uint8).reshape(MAXROWS[(ty, K)], -1)
        wv.setflags(write=False)
        _W[(ty, K)] = wv
    return _W[(ty, K)]


def _acts(K):
    """the activation row (test_round3_gpu._act: an all-zero Q8_K block, a +/- tie for a block maximum), norm weights, and the normed row as the oracle forms it"""
    if K not in _X:
        rng = np.random.default_rng(77 + K)
        x = _act(rng, K)
        nw = rng.standard_normal(K).astype(np.float32)
        xn = (orc.rms_norm(x, 1e-6) * nw).astype(np.float32)
        for a in (x, nw, xn):
            a.setflags(write=False)
        _X[K] = (x, nw, xn)
    return _X[K]


def _want(ty, K, normed, lo, hi):
    """oracle_py.mul_mat of rows [lo, hi) of the shared (ty, K) matrix on the plain / normed activation row; computed up to `hi` once, kept"""
    key = (ty, K, normed)
    have = _ORC.get(key)
    n = 0 if have is None else have.size
    if n < hi:
        x, _, xn = _acts(K)
        more = orc.mul_mat(ty, _weights(ty, K)[n:hi], xn if normed else x).ravel()
        have = more if have is None else np.concatenate([have, more])
        have.setflags(write=False)
        _ORC[key] = have
    return _ORC[key][lo:hi]


def _check_types(pkg):
    assert (pkg.GGML_TYPE_Q8_0, pkg.GGML_TYPE_Q4_K, pkg.GGML_TYPE_Q6_K) == (Q8_0, Q4_K, Q6_K)


def _cus(be):
    cus = int(be.get_stat("mv2_cus"))
    assert cus > 0, "stat mv2_cus"
    return cus


# ------------------------------------------------------------------------------------------------ running a case on both families
def _compute_both(be, c, outs, feeds, k_engine=1, k_register=1, engine_launches=1):
    """alloc + feed once, then the graph on the engine (three times: bit-identical) and on the register family; returns {1: [...], 0: [...]}.
    Asserts which family ran (mv2_launches), the launch count, and that every output value was written (NaN pre-fill)."""
    c.alloc()
    for t, v in feeds:
        be.tensor_set(t, v)
    g = c.graph()
    res = {}
    try:
        for mv2 in (1, 0):
            be.set_option("mv2", mv2)
            runs = []
            for rep in range(3 if mv2 else 1):
                for o in outs:
                    be.tensor_set(o, np.full(o.nelements(), np.nan, np.float32))
                n0 = be.get_stat("mv2_launches")
                be.graph_compute(g)
                got = [be.tensor_get(o).copy().ravel() for o in outs]
                if rep == 0:                                  # (a later compute may be a replay of a captured graph: no mmv2() call)
                    assert be.get_stat("mv2_launches") - n0 == (engine_launches if mv2 else 0), (mv2, be.get_stat("mv2_launches") - n0)
                    assert be.get_stat("kernels_last_graph") == (k_engine if mv2 else k_register), (mv2, be.get_stat("kernels_last_graph"))
                runs.append(got)
            for i, a in enumerate(runs[0]):
                assert np.isfinite(a).all(), (mv2, i, np.flatnonzero(~np.isfinite(a))[:8])
            for rr in runs[1:]:
                for i, (a, b) in enumerate(zip(runs[0], rr)):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, np.flatnonzero(a != b)[:8])
            res[mv2] = runs[0]
    finally:
        be.set_option("mv2", 1)
        c.free()
    return res


def _slices(got, want):
    return [nmse(got[i:i + SLICE], want[i:i + SLICE]) for i in range(0, want.size, SLICE)]


def _judge(res, wants, q80, label):
    bar_fam = 1e-11 if q80 else 1e-12
    for i, want in enumerate(wants):
        eng, reg = res[1][i], res[0][i]
        assert eng.shape == want.shape == reg.shape
        e_o, r_o, e_r = nmse(eng, want), nmse(reg, want), nmse(eng, reg)
        s_e, s_r = _slices(eng, want), _slices(reg, want)
        print(f"{label} m[{i}] rows {want.size}: NMSE engine/oracle {e_o:.2e} register/oracle {r_o:.2e} engine/register {e_r:.2e}; "
              f"worst {SLICE}-row slice engine {max(s_e):.2e} (at row {SLICE * int(np.argmax(s_e))}) register {max(s_r):.2e}")
        assert r_o < 1e-9 and max(s_r) < 1e-9, (i, r_o, max(s_r))          # the register family: the yardstick's own health
        assert e_o < 1e-9, (i, e_o)
        assert e_r < bar_fam, (i, e_r)
        assert max(s_e) < 1e-9, (i, max(s_e), SLICE * int(np.argmax(s_e)))


def _plan_for(be, rows, types, K, prop, what):
    """the restated plan at the device's CU count, printed; the property the case is named for holds there, or the case is skipped with the reason"""
    cus = _cus(be)
    plan = mv2_plan_py(rows, types, K, cus)
    print(f"mv2_cus {cus}: rows {rows} -> (wg0, nwg, q, r) {plan}")
    if not prop(plan, cus):
        assert cus != 256, (what, plan)                       # the literal shapes are chosen for 256 CUs: there the property must hold
        pytest.skip(f"{what}: lost with {cus} CUs, plan {plan}")
    return plan


# ------------------------------------------------------------------------------------------------ one matrix (cases a - e, g, h)
def _single(pkg, be, ty, K, M, resid, prop, what, rows_of=None, k_engine=1):
    """y = W x (+ r).  rows_of: row i of W is row rows_of[i] of the shared matrix (case h: a 4096-row matrix tiled)."""
    _check_types(pkg)
    _plan_for(be, [M], [ty], K, prop, what)
    x, _, _ = _acts(K)
    if rows_of is None:
        wv, want = _weights(ty, K)[:M], _want(ty, K, False, 0, M)
    else:
        wv, want = _weights(ty, K)[rows_of], _want(ty, K, False, 0, int(rows_of.max()) + 1)[rows_of]
    r = np.random.default_rng(M).standard_normal(M).astype(np.float32)
    c = pkg.Context(be)
    w = c.new_tensor(ty, K, M); xt = c.new_tensor(pkg.GGML_TYPE_F32, K, 1)
    feeds = [(w, wv), (xt, x)]
    y = c.mul_mat(w, xt)
    if resid:
        rt = c.new_tensor(pkg.GGML_TYPE_F32, M, 1)
        y = c.add(y, rt)
        feeds.append((rt, r))
        want = want + r
    res = _compute_both(be, c, [y], feeds, k_engine=k_engine)
    _judge(res, [want], ty == Q8_0, f"{TNAME[ty]} K={K}")


def _ragged(plan, cus):                                       # workgroups of q and q + 1 rows share the launch
    return plan[0][3] != 0


def _short_group4(plan, cus):                                 # a workgroup whose row count is no multiple of the 4-row group
    return any(n % 4 for n in _ntasks(plan[0]))


def _id1(tag, ty, K, M):
    return f"{tag}-{TNAME[ty]}-K{K}-{M}{_qr(mv2_plan_py([M], [ty], K, 256))}"


@pytest.mark.parametrize("ty,K", [pytest.param(t, K, id=_id1("ab"[K > 4096], t, K, 4100)) for K in (4096, 12288) for t in (Q4_K, Q6_K)])
def test_one_matrix_with_residual_q_and_q_plus_1_rows_on_ten_waves(pkg, be, ty, K):
    """Cases a, b: 4100 rows + residual on the ten-wave instances <1,NIT,10> (K = 4096: the half-block consumer, 2-row groups) and <2,NIT,10>.  256 CUs: q = 16,
    r = 4: workgroups of 17 and of 16 rows in one launch, an odd count on the 2-row groups, residuals staged per workgroup."""
    _single(pkg, be, ty, K, 4100, True, lambda p, cus: _ragged(p, cus) and 4100 <= 16384, "r != 0 on the ten-wave instance")


@pytest.mark.parametrize("ty,K", [pytest.param(t, K, id=_id1("cd"[K > 4096], t, K, 16500)) for K, ts in ((4096, (Q4_K,)), (12288, (Q4_K, Q6_K))) for t in ts])
def test_one_plain_matrix_ragged_on_sixteen_waves(pkg, be, ty, K):
    """Cases c, d: 16500 rows (above the ten-wave limit of 16384), no residual: <1,1,16> with 4-row groups (256 CUs: q = 64, r = 116: 65 % 4 = 1), <1,3,16>, <2,3,16>."""
    prop = (lambda p, cus: _ragged(p, cus) and _short_group4(p, cus)) if (ty == Q4_K and K == 4096) else _ragged
    _single(pkg, be, ty, K, 16500, False, prop, "r != 0 (and a short 4-row group) on the sixteen-wave instance")


@pytest.mark.parametrize("ty", [pytest.param(t, id=_id1("e", t, 4096, 32000)) for t in (Q4_K, Q6_K)])
def test_llama2_vocabulary_rows(pkg, be, ty):
    """Case e: 32000 rows (Llama-2's vocabulary).  256 CUs: q = 125 -- <1,1,16>: 125 % 4 = 1, every workgroup ends in a group of one row; Q6_K: <2,1,9>."""
    _single(pkg, be, ty, 4096, 32000, False, _short_group4 if ty == Q4_K else (lambda p, cus: True), "a row count per workgroup that is no multiple of 4")


@pytest.mark.parametrize("ty", [pytest.param(t, id=f"g-{TNAME[t]}") for t in (Q4_K, Q6_K, Q8_0)])
@pytest.mark.parametrize("M", [1, 100, "cus+1"])
def test_fewer_rows_than_cus(pkg, be, ty, M):
    """Case g: grid = rows, one task per workgroup -- fewer tasks than a row group and fewer than there are consumers -- and cus + 1 rows: exactly one
    workgroup with two tasks."""
    cus = _cus(be)
    if M == "cus+1":
        _single(pkg, be, ty, 4096, cus + 1, True, lambda p, c_: p[0][1:] == (c_, 1, 1), "one workgroup of two tasks")
    else:
        _single(pkg, be, ty, 4096, M, True, lambda p, c_: p[0][1:] == (M, 1, 0), "grid = rows, one task each")


@pytest.mark.parametrize("extra", [0, 1], ids=["h-q4_K-cus*256[q256r0]", "h-q4_K-cus*256+1[q256r1]"])
def test_residual_staging_limit(pkg, be, extra):
    """Case h: cus * 256 rows + residual is the last count mmv2_ok accepts: 256 tasks per workgroup fill the 1 KiB residual staging area exactly, one launch.
    One row more: the residual ADD becomes its own launch and the mat-vec stays on the engine (two launches, one of them mmv2).  The matrix is a 4096-row
    random block matrix tiled (the oracle runs on 4096 rows); the residual differs per row, so row identity is still checked."""
    M = _cus(be) * 256 + extra
    rows_of = np.arange(M) % 4096
    _single(pkg, be, Q4_K, 4096, M, True, lambda p, cus: p[0][1:] == (cus, 256, extra), "256 tasks per workgroup", rows_of=rows_of, k_engine=1 + extra)


# ------------------------------------------------------------------------------------------------ gate / up pair (case f)
def _id_pair(ty, M):
    return f"f-{TNAME[ty]}-{M}{_qr(mv2_plan_py([M], [ty], 4096, 256))}"


@pytest.mark.parametrize("ty,M", [pytest.param(t, M, id=_id_pair(t, M)) for t in (Q4_K, Q8_0) for M in (11008, 5000)])
def test_gate_up_pair_odd_and_ragged(pkg, be, ty, M):
    """Case f: RMS_NORM + MUL folded, gate / up as one pair of rings, SwiGLU in the epilogue.  11008 rows (Llama-2-7B's FFN): on 256 CUs 43 pair-tasks per
    workgroup, an odd count on the 2-row pair consumer <1,1,true>; 5000 rows: q = 19, r = 136.  Q8_0: the Q8_0 pair."""
    _check_types(pkg)
    K = 4096
    prop = (lambda p, cus: any(n % 2 for n in _ntasks(p[0]))) if M == 11008 else _ragged
    _plan_for(be, [M], [ty], K, prop, "an odd task count" if M == 11008 else "r != 0")
    x, nw, _ = _acts(K)
    W = _weights(ty, K)
    c = pkg.Context(be)
    wg = c.new_tensor(ty, K, M); wu = c.new_tensor(ty, K, M); xt = c.new_tensor(pkg.GGML_TYPE_F32, K, 1); nt = c.new_tensor(pkg.GGML_TYPE_F32, K)
    xn = c.mul(c.rms_norm(xt, 1e-6), nt)
    up = c.mul_mat(wu, xn); gate = c.mul_mat(wg, xn)
    y = c.swiglu_split(gate, up)
    res = _compute_both(be, c, [y], [(wg, W[:M]), (wu, W[M:2 * M]), (xt, x), (nt, nw)])
    g, u = _want(ty, K, True, 0, M), _want(ty, K, True, M, 2 * M)
    want = (_silu(g.astype(np.float64)) * u.astype(np.float64)).astype(np.float32)
    _judge(res, [want], ty == Q8_0, f"pair {TNAME[ty]}")


# ------------------------------------------------------------------------------------------------ groups (cases i - n)
def _group(pkg, be, K, rows, types, normed, resid_on, prop, what):
    """two or three matrices on one activation (rms_norm(x) * w folded when `normed`), member resid_on (or none) with a residual ADD: ONE launch"""
    _check_types(pkg)
    _plan_for(be, rows, types, K, prop, what)
    x, nw, _ = _acts(K)
    c = pkg.Context(be)
    ws = [c.new_tensor(t, K, m) for t, m in zip(types, rows)]
    xt = c.new_tensor(pkg.GGML_TYPE_F32, K, 1)
    feeds = [(xt, x)]
    if normed:
        nt = c.new_tensor(pkg.GGML_TYPE_F32, K)
        src = c.mul(c.rms_norm(xt, 1e-6), nt)
        feeds.append((nt, nw))
    else:
        src = xt
    ys = [c.mul_mat(w, src) for w in ws]
    wants, off = [], 0
    for i, (t, m) in enumerate(zip(types, rows)):             # member i: rows [off, off + m) of its type's shared matrix
        feeds.append((ws[i], _weights(t, K)[off:off + m]))
        wants.append(_want(t, K, normed, off, off + m).copy())
        off += m
    if resid_on is not None:
        r = np.random.default_rng(rows[resid_on]).standard_normal(rows[resid_on]).astype(np.float32)
        rt = c.new_tensor(pkg.GGML_TYPE_F32, rows[resid_on], 1)
        ys[resid_on] = c.add(ys[resid_on], rt)
        feeds.append((rt, r))
        wants[resid_on] = wants[resid_on] + r
    res = _compute_both(be, c, ys, feeds)
    _judge(res, wants, types[0] == Q8_0, f"group {[TNAME[t] for t in types]} K={K}")


def _idg(tag, rows, types, K):
    return f"{tag}-{'+'.join(TNAME[t] for t in types)}-K{K}-{'+'.join(map(str, rows))}{_qr(mv2_plan_py(rows, types, K, 256))}"


GROUPS = [
    # tag, K, rows, types, normed activation, member with a residual, property of the plan, its name
    ("i", 4096, [512, 512], [Q4_K, Q6_K], True, None, lambda p, cus: len(p) == 2, "a two-member packed group, <3,1,9>"),
    ("j", 4096, [4100, 1028, 1028], [Q4_K, Q4_K, Q6_K], True, 1, lambda p, cus: len(p) == 3, "an unpacked group: mv2_mat of m[1], m[2] from the argument block"),
    ("k", 12288, [300, 300, 300], [Q4_K, Q4_K, Q4_K], False, None, lambda p, cus: len(p) == 3, "a group at K = 12288, <1,3>"),
    ("k", 12288, [300, 300, 300], [Q4_K, Q4_K, Q6_K], False, None, lambda p, cus: len(p) == 3, "a group at K = 12288, <3,3>"),
    ("l", 4096, [4096, 8, 8], [Q4_K, Q4_K, Q4_K], True, None, lambda p, cus: p[1][1] == 1 and p[2][1] == 1, "members held to one workgroup by the plan's floor"),
    ("m", 4096, [4100, 1028, 1028], [Q8_0, Q8_0, Q8_0], True, None, lambda p, cus: p[0][3] != 0, "a Q8_0 group on ten waves with r != 0"),
    ("n", 4096, [128, 64, 64], [Q4_K, Q4_K, Q6_K], True, None, lambda p, cus: p[2][1] > 64 and p[2][2] == 0, "workgroups with no task (more workgroups than rows)"),
]


@pytest.mark.parametrize("tag,K,rows,types,normed,resid_on,prop,what", [pytest.param(*G, id=_idg(G[0], G[2], G[3], G[1])) for G in GROUPS])
def test_group_forms(pkg, be, tag, K, rows, types, normed, resid_on, prop, what):
    """Cases i - n: the executor batches any two or three mat-vecs that read one activation into one k_mv2 launch, workgroups split by bytes (Q6_K counted
    MV2_Q6_SHARE times).  i: two members; j: a residual on the second member (the launch cannot be described by the pre-loaded scalars); k: K = 12288;
    l: tiny members; m: Q8_0; n: the Q6_K member gets more workgroups than it has rows (module docstring: the ntask = 0 trace)."""
    _group(pkg, be, K, rows, types, normed, resid_on, prop, what)
