"""MUL_MAT on every route of route_mul_mat under strided, batched, broadcast and view operands (-m gpu; the table and its builders: mm_layouts.py).

Per case: (1) the profile-class launch counts of the first run equal what the table declares for the route -- a case that lands elsewhere proves nothing; (2) every
output column (n, i12, i13) against its reference, built from weight slice (i12 // r2, i13 // r3): the oracle's integer arithmetic for quantised weights (the C
restatement for Q4_K / Q6_K / Q8_0, the reference CPU backend on dense 2-D operands for the block formats the restatement does not hold), NMSE < 1e-9 on the
integer routes and < 5e-4 on the F16-image GEMM; float64 numpy on activations rounded as the route rounds them for F16 / F32 / BF16 weights, NMSE < 1e-9;
(3) where the route reads an activation image, bit-identity with the same case on a dense src1; (4) every output finite -- the padding of every parent is poisoned;
(5) the profiled run, an eager run, the capture and the replay bit-identical.  The figures are printed before anything is asserted."""
import numpy as np
import pytest

import mm_layouts as L

pytestmark = pytest.mark.gpu

ORACLE_TYPES = (L.Q4_K, L.Q6_K, L.Q8_0)
_twin_results = {}
_ref_cache = {}


def _ref_mul_mat(pkg, request, wtype, Wm, Xc):
    """quantised weights [M, row bytes] against columns [n, K] f32 -> [n, M], the reference's integer arithmetic"""
    if wtype in ORACLE_TYPES:
        import oracle.oracle_py as orc
        return orc.mul_mat(wtype, Wm, Xc)
    from oracle.ref_backend import ref_available
    assert ref_available(), "oracle/_ref/libggml-ref.so is missing: no reference for %s weights (a case is never skipped for that -- build the reference)" % L.TNAME[wtype]
    ref_be = request.getfixturevalue("ref_be")
    c = pkg.Context(ref_be)
    w, x = c.new_tensor(wtype, Xc.shape[1], Wm.shape[0]), c.new_tensor(pkg.GGML_TYPE_F32, Xc.shape[1], Xc.shape[0])
    y = c.mul_mat(w, x)
    c.alloc()
    ref_be.tensor_set(w, Wm)
    ref_be.tensor_set(x, Xc)
    ref_be.graph_compute(c.graph())
    out = ref_be.tensor_get(y).copy().reshape(Xc.shape[0], Wm.shape[0])
    c.free()
    return out


def _expected(pkg, request, case, W, X):
    """[ne13, ne12, N, M] float64 -- one reference product per weight slice, over every column that reads it; shared by a case, its dense twin and its resident-image twin"""
    key = L.twin(case)._replace(wbuf="any", wl="dense")
    if key in _ref_cache:
        return _ref_cache[key]
    ne02, ne03, r2, r3 = case.batch
    ne12, ne13 = L.ne1x(case)
    want = np.empty((ne13, ne12, case.N, case.M), np.float64)
    Xr = None if case.wtype not in L.FLOAT_TYPES else L.round_act(case, X)
    for i03 in range(ne03):
        for i02 in range(ne02):
            sl = (slice(i03 * r3, (i03 + 1) * r3), slice(i02 * r2, (i02 + 1) * r2))
            if case.wtype in L.FLOAT_TYPES:
                want[sl] = Xr[sl] @ L.w_as_f64(case.wtype, W[i03, i02]).T
            else:
                cols = np.ascontiguousarray(X[sl].reshape(-1, case.K), np.float32)
                want[sl] = _ref_mul_mat(pkg, request, case.wtype, W[i03, i02], cols).reshape(r3, r2, case.N, case.M)
    if len(_ref_cache) > 64:
        _ref_cache.clear()
    _ref_cache[key] = want
    return want


def _column_nmse(got, want):
    d = ((got.astype(np.float64) - want) ** 2).sum(axis=-1)
    n = (want ** 2).sum(axis=-1)
    return float((d / n).max())


def _run(pkg, be, case, W, X, profile):
    """-> (results of every run as uint32 bit patterns [ne13, ne12, N, M], launch counts of the first run -- with "kernels", every launch of that run -- or None)"""
    ne12, ne13 = L.ne1x(case)
    wg, xg = L.geometry(case)
    t = L.build_case(pkg, be, case)
    counts, outs = None, []
    try:
        assert be.supports_op(t["y"]), "supports_op refuses a case of the table"
        be.tensor_set(t["w_parent"], L.poisoned_parent(case.wtype, wg, W, True))
        be.tensor_set(t["x_parent"], L.poisoned_parent(case.xtype, xg, X if case.xtype == L.F32 else X.view(np.uint16), False))
        g = t["ctx"].graph()

        def once():
            be.graph_compute(g)
            outs.append(be.tensor_get(t["y"]).copy().view(np.uint32).reshape(ne13, ne12, case.N, case.M))
        if profile:
            be.set_option("profile", 1)
            be.set_option("reset_stats", 1)
            try:
                once()
                counts = {c: int(be.get_stat("prof_%s_n" % c)) for c in L.CLASSES}
                counts["kernels"] = int(be.get_stat("kernels_last_graph"))
            finally:
                be.set_option("profile", 0)
        for _ in range(3):                                           # eager, then captured and replayed where the graph qualifies
            once()
    finally:
        t["ctx"].free()
        t["wctx"].free()
    return outs, counts


def _bar(case):
    if case.wtype in L.FLOAT_TYPES or case.route in L.INTEGER_ROUTES:
        return 1e-9
    return 5e-4                                                      # quantised weights through their F16 image (test_mul_mat_gemm_path_vs_oracle)


def _check(pkg, be, request, case):
    assert be.alignment % 16 == 0
    W, X = L.make_data(case)
    if case.route == "MM_MMQ_TILE":
        be.set_option("mmq_tile", 1)
    try:
        outs, counts = _run(pkg, be, case, W, X, True)
        same_as_twin = None
        if case.xl != "dense" and L.reads_image(case):
            tw = L.twin(case)
            if tw not in _twin_results:
                if len(_twin_results) > 256:
                    _twin_results.clear()
                _twin_results[tw] = _run(pkg, be, tw, W, X, False)[0][0]
            same_as_twin = bool(np.array_equal(outs[0], _twin_results[tw]))
    finally:
        if case.route == "MM_MMQ_TILE":
            be.set_option("mmq_tile", -1)
    got = outs[0].view(np.float32)
    want = _expected(pkg, request, case, W, X)
    finite = bool(np.isfinite(got).all())
    err = _column_nmse(got, want) if finite else float("inf")
    declared = L.launches(case)
    wrong = {c: (counts[c], declared[c]) for c in L.CLASSES if counts[c] != declared[c]}
    repeat = all(np.array_equal(outs[0], o) for o in outs[1:])
    print("MMLAY %s route=%s nmse=%.3e bar=%g finite=%d twin=%s repeat=%d counts_wrong=%s" % (case.id, case.route, err, _bar(case), finite, same_as_twin, repeat, wrong))
    assert not wrong, "launch counts (measured, declared) differ: %s" % wrong
    assert finite, "non-finite output: a read outside a row (the padding is poisoned)"
    assert err < _bar(case), (case.id, err)
    assert same_as_twin is not False, "the result differs from the same case on a dense src1, although the route reads a dense image of it"
    assert repeat, "profiled, eager, captured and replayed runs differ"
    return counts


@pytest.mark.parametrize("case", L.CASES + L.EXTRA_CASES, ids=lambda c: c.id)
def test_mul_mat_layouts(pkg, be, request, case):
    _check(pkg, be, request, case)


def test_heads_past_the_one_launch_conversion(pkg, be, request):
    """7282 heads of 9 q-shaped columns: prepare_act converts slice by slice (65538 rows do not fit convert_f32_f16_rows3's grid).  The profile class books one act_convert
    either way, so the loop is pinned by the launches of the run: one conversion per head, the GEMM, the SCALE tail -- against three heads of the same shape, which take the
    one strided conversion launch"""
    tail = 8
    big = _check(pkg, be, request, L.BIG_HEADS)
    small = _check(pkg, be, request, L.BIG_HEADS._replace(batch=(1, 1, 3, 1)))
    print("MMLAY heads kernels: %d at 7282 heads, %d at 3" % (big["kernels"], small["kernels"]))
    assert small["kernels"] <= 1 + 1 + tail                           # one conversion launch, the GEMM, at most one launch per SCALE node
    assert big["kernels"] >= 7282 + 1                                 # a conversion launch per head and the GEMM (the one-launch form would stay at 1 + 1 + tail)


@pytest.mark.parametrize("name,wtype,K,geo", L.DECLINED, ids=[d[0].split(" (")[0].replace(" ", "_") for d in L.DECLINED])
def test_declined_layouts_are_refused(pkg, be, name, wtype, K, geo):
    """the fixed list of layouts no kernel takes: supports_op says no (so the scheduler keeps the node on the CPU); nothing is computed"""
    wctx, c = pkg.Context(be), pkg.Context(be)
    parent, w = L.build_view(c, wctx, wtype, geo)
    x = c.new_tensor(pkg.GGML_TYPE_F32, K, 5)
    y = c.mul_mat(w, x)
    wctx.alloc()
    c.alloc()
    try:
        assert not be.supports_op(y), name
        if geo.perm is None:                                         # the same matrix, dense: admitted
            c2 = pkg.Context(be)
            y2 = c2.mul_mat(c2.new_tensor(wtype, K, L.M_ROWS), c2.new_tensor(pkg.GGML_TYPE_F32, K, 5))
            c2.alloc()
            try:
                assert be.supports_op(y2)
            finally:
                c2.free()
    finally:
        c.free()
        wctx.free()


# ---- the grouped launches on view operands
def _poisoned_x(pkg, be, c, K, N, rng):
    """a rowpad16 [K, N] f32 view of a poisoned parent -> (view tensor, logical values, upload)"""
    xg = L.x_geo("rowpad16", L.F32, K, N, 1, 1)
    parent, x = L.build_view(c, c, L.F32, xg)
    xv = rng.standard_normal((1, 1, N, K)).astype(np.float32)
    return x, xv[0, 0], (parent, L.poisoned_parent(L.F32, xg, xv, False))


@pytest.mark.parametrize("N", [5, 33])
def test_three_kquant_matrices_share_one_padded_x(pkg, be, N):
    """wq / wk / wv on one rowpad16 x: one grouped mat-vec launch at 5 columns, two grouped int8-MFMA launches at 33 -- against the oracle, per column, and bit-identical
    to the three products computed one by one on a dense x"""
    import oracle.oracle_py as orc
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(100 + N)
    K, Ms, types = 512, (70, 38, 38), (L.Q4_K, L.Q4_K, L.Q6_K)
    Wv = [qwen3.random_blocks(rng, t, m, K, std=0.05) for t, m in zip(types, Ms)]

    def run(layout, grouped):
        res = []
        for sel in ([(0, 1, 2)] if grouped else [(0,), (1,), (2,)]):
            wctx, c = pkg.Context(be), pkg.Context(be)
            ws = [wctx.new_tensor(types[q], K, Ms[q]) for q in sel]
            if layout == "rowpad16":
                x, xv, up = _poisoned_x(pkg, be, c, K, N, np.random.default_rng(7))
            else:
                x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
                xv = np.random.default_rng(7).standard_normal((1, 1, N, K)).astype(np.float32)[0, 0]
                up = (x, xv)
            ys = [c.mul_mat(w, x) for w in ws]
            z = ys[0]
            for _ in range(8):
                z = c.scale(z, 1.0)
            wctx.alloc()
            c.alloc()
            try:
                for w, q in zip(ws, sel):
                    be.tensor_set(w, Wv[q])
                be.tensor_set(*up)
                be.set_option("profile", 1)
                be.set_option("reset_stats", 1)
                try:
                    be.graph_compute(c.graph())
                    first = [be.tensor_get(y).copy().view(np.uint32) for y in ys]
                    n = {k: int(be.get_stat("prof_%s_n" % k)) for k in ("mmv_q4k", "mmv_q6k", "mmq_q4k", "mmq_q6k", "act_convert")}
                finally:
                    be.set_option("profile", 0)
                for _ in range(3):
                    be.graph_compute(c.graph())
                    for a, y in zip(first, ys):
                        assert np.array_equal(a, be.tensor_get(y).view(np.uint32))
                res.append((first, n, xv))
            finally:
                c.free()
                wctx.free()
        return res
    (got, n, xv), = run("rowpad16", True)
    launches = n["mmv_q4k"] + n["mmv_q6k"] + n["mmq_q4k"] + n["mmq_q6k"]
    print("MMLAY grouped N=%d counts=%s" % (N, n))
    assert launches == (1 if N <= 8 else 2) and n["act_convert"] == 1, n          # one launch for the three matrices (per 32 columns on the matrix cores)
    singles = run("dense", False)
    for q in range(3):
        g = got[q].view(np.float32).reshape(N, Ms[q])
        assert np.isfinite(g).all()
        want = orc.mul_mat(types[q], Wv[q], xv).astype(np.float64)
        err = _column_nmse(g, want)
        print("MMLAY grouped N=%d matrix %d nmse=%.3e" % (N, q, err))
        assert err < 1e-9, (q, err)
        assert np.array_equal(got[q], singles[q][0][0]), "grouped launch on the padded x differs from the single product on a dense x"


@pytest.mark.parametrize("wtype,N", [(L.Q4_K, 1), (L.Q4_K, 5), (L.Q6_K, 33), (L.Q4_K, 70)], ids=["q4_K-N1", "q4_K-N5", "q6_K-N33", "q4_K-N70-gemm"])
def test_wo_with_a_residual_that_is_a_padded_view(pkg, be, wtype, N):
    """y = wo . x, out = y + r with r a rowpad16 view (the ADD rides in the mat-mul's epilogue where the launch takes a residual): per column against oracle + r in f32,
    bit-identical to the same graph on a dense r, poisoned padding around r"""
    import oracle.oracle_py as orc
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(200 + N)
    K, M = 512, 72
    Wv = qwen3.random_blocks(rng, wtype, M, K, std=0.05)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    rv = rng.standard_normal((1, 1, N, M)).astype(np.float32)
    cls = "gemm_f16" if N > L.MMQ_MAX_COLS else "mmq_q6k" if N >= L.MMQ_MIN_COLS else "mmv_q4k"
    outs = {}
    for layout in ("rowpad16", "dense"):
        wctx, c = pkg.Context(be), pkg.Context(be)
        w = wctx.new_tensor(wtype, K, M)
        x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
        rg = L.x_geo(layout, L.F32, M, N, 1, 1)
        rp, r = L.build_view(c, c, L.F32, rg)
        out = c.add(c.mul_mat(w, x), r)
        z = out
        for _ in range(8):
            z = c.scale(z, 1.0)
        wctx.alloc()
        c.alloc()
        try:
            be.tensor_set(w, Wv)
            be.tensor_set(x, xv)
            be.tensor_set(rp, L.poisoned_parent(L.F32, rg, rv, False))
            runs = []
            be.set_option("profile", 1)
            be.set_option("reset_stats", 1)
            try:
                be.graph_compute(c.graph())
                runs.append(be.tensor_get(out).copy().view(np.uint32))
                n = {k: int(be.get_stat("prof_%s_n" % k)) for k in ("mmv_q4k", "mmq_q6k", "gemm_f16", "bin")}
            finally:
                be.set_option("profile", 0)
            print("MMLAY residual %s N=%d %s counts=%s" % (L.TNAME[wtype], N, layout, n))
            # the ADD ran in the mat-mul launch's epilogue: the launches of the path (two 32-column passes at 33 columns) and no element-wise launch for the ADD node
            assert n["bin"] == 0, n
            assert n[cls] == (2 if N == 33 else 1), n
            for _ in range(3):
                be.graph_compute(c.graph())
                runs.append(be.tensor_get(out).copy().view(np.uint32))
            assert all(np.array_equal(runs[0], o) for o in runs[1:])
            outs[layout] = runs[0]
        finally:
            c.free()
            wctx.free()
    g = outs["rowpad16"].view(np.float32).reshape(N, M)
    assert np.isfinite(g).all()
    want = orc.mul_mat(wtype, Wv, xv).astype(np.float64) + rv[0, 0]
    err = _column_nmse(g, want)
    print("MMLAY residual %s N=%d nmse=%.3e" % (L.TNAME[wtype], N, err))
    assert err < (5e-4 if N > L.MMQ_MAX_COLS else 1e-9), err
    assert np.array_equal(outs["rowpad16"], outs["dense"])


# ---- a captured graph and its leaf sources
@pytest.mark.parametrize("change", ["type", "stride"])
def test_capture_is_not_replayed_when_a_leaf_source_changes(pkg, be, request, change):
    """The capture records hold a leaf source's data pointer; its type and strides say nothing in the node that reads it (MUL_MAT's result is the same F32 [M, N] for Q4_0 and
    IQ4_NL weights, for dense and for padded rows).  A graph is run until it replays; then its weight leaf -- same address, same node -- becomes IQ4_NL instead of Q4_0 (both
    18-byte blocks: the bytes are valid in either), or takes every second row of its parent: the next run must compute the new product, not replay the old one."""
    from llama_cpp_omni_amd import qwen3
    K, M, N, rs = 96, L.M_ROWS, 5, L.row_size(L.Q4_0, 96)
    rng = np.random.default_rng(77)
    raw = qwen3.random_blocks(rng, L.Q4_0, 2 * M, K, std=0.05)
    xv = rng.standard_normal((N, K)).astype(np.float32)
    wctx, c = pkg.Context(be), pkg.Context(be)
    parent = wctx.new_tensor(L.Q4_0, K, 2 * M)
    w = c._new(L.Q4_0, (K, M), view_src=parent)                       # a leaf of its own (op NONE) over the parent's first M rows
    x = c.new_tensor(pkg.GGML_TYPE_F32, K, N)
    y = c.mul_mat(w, x)
    z = y
    for _ in range(8):
        z = c.scale(z, 1.0)
    wctx.alloc()
    c.alloc()
    try:
        be.tensor_set(parent, raw)
        be.tensor_set(x, xv)
        g = c.graph()

        def run():
            be.graph_compute(g)
            return be.tensor_get(y).copy().reshape(N, M)
        replays = be.get_stat("graph_replays")
        before = [run() for _ in range(3)]
        assert be.get_stat("graph_replays") > replays, "the graph was never replayed: the test proves nothing"
        assert _column_nmse(before[2], _ref_mul_mat(pkg, request, L.Q4_0, raw[:M], xv).astype(np.float64)) < 1e-9
        if change == "type":
            w.t.type, wtype, rows = L.IQ4_NL, L.IQ4_NL, raw[:M]
        else:
            w.t.nb[1], w.t.nb[2], w.t.nb[3] = 2 * rs, 2 * rs * M, 2 * rs * M
            wtype, rows = L.Q4_0, np.ascontiguousarray(raw.reshape(2 * M, rs)[0::2])
        after = [run() for _ in range(3)]
        want = _ref_mul_mat(pkg, request, wtype, rows, xv).astype(np.float64)
        err = _column_nmse(after[0], want)
        print("MMLAY leaf %s change: nmse=%.3e, against the product before the change %.3e" % (change, err, _column_nmse(after[0], before[2].astype(np.float64))))
        assert err < 1e-9, err
        assert all(np.array_equal(after[0], a) for a in after[1:])
    finally:
        c.free()
        wctx.free()
