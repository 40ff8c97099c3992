"""The MUL_MAT layout table (mm_layouts.py) held against itself, without a GPU: every layout's numpy mirror reads the dense logical array back out of the poisoned parent
and leaves every other cell poison; every route appears with every layout and batch tuple its rule allows, every omission carries a reason that the restated
route_mul_mat / supports_op confirm; and the tensors a device-less Context builds carry the mirror's ne / nb."""
import numpy as np
import pytest

import mm_layouts as L


def _logical(case, which):
    """a logical array of distinct, never-poison values: [ne3, ne2, ne1, row bytes] bytes for src0, [ne3, ne2, ne1, K] elements for src1"""
    wg, xg = L.geometry(case)
    if which == "w":
        shape = (wg.ne[3], wg.ne[2], wg.ne[1], L.row_size(case.wtype, wg.ne[0]))
        return (np.arange(int(np.prod(shape)), dtype=np.int64) % 251).astype(np.uint8).reshape(shape), wg, case.wtype          # 0 .. 250: never 0xFF
    shape = (xg.ne[3], xg.ne[2], xg.ne[1], xg.ne[0])
    a = (np.arange(int(np.prod(shape)), dtype=np.int64) % 2039).reshape(shape)
    return (a.astype(np.float32) if case.xtype == L.F32 else a.astype(np.float16).view(np.uint16)), xg, case.xtype


def test_the_table_is_not_empty_and_ids_are_unique():
    ids = [c.id for c in L.ALL_CASES]
    assert len(ids) == len(set(ids)) and len(ids) > 300
    assert {c.route for c in L.CASES} == set(L.ROUTES)


@pytest.mark.parametrize("which", ["w", "x"])
def test_mirror_reads_back_the_logical_array_and_everything_else_is_poison(which):
    done = set()
    for case in L.ALL_CASES:
        logical, geo, t = _logical(case, which)
        key = (t, geo)
        if key in done:
            continue
        done.add(key)
        buf = L.poisoned_parent(t, geo, logical, which == "w")
        assert buf.size == L.parent_bytes(t, geo.pne)
        back = L.np_view(buf, t, geo, which == "w")
        assert np.array_equal(back, logical), case.id
        # the cells the view does not reach: clear the view's cells to poison and the whole parent must be poison again; count them too
        esize = 1 if which == "w" else L.TRAITS[t][1]
        poison = np.array([L.W_POISON], np.uint8) if which == "w" else L.x_poison_bytes(t)
        cells = buf.reshape(-1, esize)
        n_poison = int((cells == poison).all(axis=1).sum())
        assert n_poison == cells.shape[0] - logical.size, (case.id, n_poison, cells.shape[0], logical.size)
        # strides are inside the parent and, for padded / offset layouts, some poison exists
        padded = (which == "w" and case.wl in ("rowpad", "rowoff")) or (which == "x" and case.xl in ("rowpad16", "rowpad4", "gap2"))
        assert (n_poison > 0) == padded, case.id


def test_every_route_meets_every_layout_and_batch_its_rule_allows():
    for route in L.ROUTES:
        mine = [c for c in L.CASES if c.route == route]
        for xl in L.X_LAYOUTS:
            for wl in L.W_LAYOUTS:
                for b in L.BATCHES:
                    allowed = [s for s in L.SHAPES[route] if L.excluded(route, s, xl, wl, b) is None]
                    have = [c for c in mine if (c.xl, c.wl, c.batch) == (xl, wl, b)]
                    if allowed:
                        assert have, (route, xl, wl, b)
                    else:
                        assert not have
                        assert any(o[:4] == (route, xl, wl, b) and o[4] for o in L.OMITTED), (route, xl, wl, b)
        # every shape of the route, with every src0 layout and every src1 layout some batch tuple allows
        for s in L.SHAPES[route]:
            of = [c for c in mine if (c.wtype, c.xtype, c.K, c.M, c.N) == s]
            for wl in L.W_LAYOUTS:
                if any(L.excluded(route, s, xl, wl, b) is None for xl in L.X_LAYOUTS for b in L.BATCHES):
                    assert any(c.wl == wl for c in of), (route, s, wl)
        # every weight type of the route (its activation image kind) with every src1 layout
        for t in {s[0] for s in L.SHAPES[route]}:
            for xl in L.X_LAYOUTS:
                if any(L.excluded(route, s, xl, wl, b) is None for s in L.SHAPES[route] if s[0] == t for wl in L.W_LAYOUTS if wl != "kvperm" for b in L.BATCHES):
                    assert any(c.xl == xl and c.wtype == t for c in mine), (route, t, xl)
    for o in L.OMITTED:
        assert isinstance(o[4], str) and len(o[4]) > 10


def test_quantised_gemm_cases_run_in_both_kinds_of_buffer():
    q = [c for c in L.CASES if c.route == "MM_GEMM_F16" and c.wtype not in L.FLOAT_TYPES]
    assert q and {c.wbuf for c in q} == {"any", "weights"}
    for c in q:
        assert c._replace(wbuf="weights" if c.wbuf == "any" else "any") in q
    assert any(c.batch[2] > 1 and c.batch[0] > 1 for c in q)             # last_w reuse under r2 > 1 with more than one weight slice


def test_every_case_is_admitted_and_takes_the_route_it_names():
    for case in L.ALL_CASES:
        wg, xg = L.geometry(case)
        assert L.admitted(case.wtype, case.xtype, wg, xg), case.id
        assert L.case_route(case)[0] == case.route, (case.id, L.case_route(case))
        n = L.launches(case)
        assert sum(n.values()) >= 1 and all(v >= 0 for v in n.values())
    sp = [c for c in L.CASES if c.route == "MM_GEMM_ANY" and c.K == 520]
    assert sp and all(L.case_route(c)[2] == 512 for c in sp)              # the split form stays the split form under every layout it meets


def test_every_exclusion_that_cites_the_router_is_confirmed_by_it():
    """a combination left out with a line of route_mul_mat as its reason must land on ANOTHER route (or be refused) when it is built all the same"""
    n = 0
    for route in L.ROUTES:
        for s in L.SHAPES[route]:
            for xl in L.X_LAYOUTS:
                for wl in L.W_LAYOUTS:
                    for b in L.BATCHES:
                        why = L.excluded(route, s, xl, wl, b)
                        if why is None or why.startswith("definition"):
                            continue
                        assert why.startswith("route_mul_mat :"), why
                        if L.excluded(route, s, "dense" if xl == "perm0132" else xl, "dense" if wl == "kvperm" else wl, b) is None:
                            continue                                 # (left out by a definition as well)
                        c = L.Case(route, s[0], s[1], s[2], s[3], s[4], b, xl, wl, "any")
                        if (xl == "perm0132" and b[1] * b[3] == 1) or (wl == "kvperm" and (s[0] != L.F16 or b[0] == 1)):
                            continue
                        wg, xg = L.geometry(c)
                        got = L.route_of(c.wtype, c.xtype, wg, xg, mmq_tile=route == "MM_MMQ_TILE")
                        if route == "MM_GEMM_ANY":
                            assert got[2] == 0, (c.id, got)          # the node stays on the any-shape GEMM, but not in its split form
                        else:
                            assert not L.admitted(c.wtype, c.xtype, wg, xg) or got[0] != route, (c.id, got)
                        n += 1
    assert n > 0


def test_declined_list_is_refused_by_the_restated_supports_op():
    for name, wtype, K, geo in L.DECLINED:
        xg = L.x_geo("dense", L.F32, K, 5, 1, 1)
        assert not L.admitted(wtype, L.F32, geo, xg), name
        assert geo.off + (geo.ne[1] - 1) * geo.nb[1] + (L.row_size(wtype, K) if geo.perm is None else 4) <= L.parent_bytes(wtype, geo.pne), name


def test_launch_counts_of_the_spelled_out_examples():
    one = lambda **kw: next(c for c in L.CASES if all(getattr(c, k) == v for k, v in kw.items()))
    c = one(route="MM_MMQ", N=33, batch=(2, 1, 3, 1))
    assert L.launches(c)["mmq_q4k" if c.wtype == L.Q4_K else "mmq_q6k"] == 6 * 2            # two launches per slice
    c = one(route="MM_MMV_HEADS", wtype=L.F16)
    assert L.launches(c)["mmv_f16"] == 1 and L.launches(c)["act_convert"] == 1                # one mat-vec launch for all heads
    c = one(route="MM_GEMM_F16", wbuf="any", batch=(2, 1, 3, 1), wtype=L.Q8_0)
    assert L.launches(c)["gemm_f16"] == 6 and L.launches(c)["dequant_f16"] == 2               # w_scratch reused across the three heads of a weight slice
    c = one(route="MM_GEMM_F16", wbuf="any", batch=(2, 2, 2, 2), wtype=L.Q8_0)
    assert L.launches(c)["gemm_f16"] == 16 and L.launches(c)["dequant_f16"] == 8
    assert L.launches(c._replace(wbuf="weights"))["dequant_f16"] == 4                          # one resident image per weight slice
    assert L.launches(L.BIG_HEADS)["gemm_f16"] == 1 and L.launches(L.BIG_HEADS)["act_convert"] == 1


def test_built_tensors_carry_the_mirrors_shapes_and_strides(pkg):
    """a Context without a device (as test_graph_views_host.py builds one): the view tensors' ne / nb / offset against the mirror"""
    for case in L.ALL_CASES:
        wg, xg = L.geometry(case)
        t = L.build_case(pkg, None, case, tail=0)
        for T, parent, g, ty in ((t["w"], t["w_parent"], wg, case.wtype), (t["x"], t["x_parent"], xg, case.xtype)):
            assert T.type == ty and tuple(T.ne) == tuple(g.ne), case.id
            for d in range(4):
                if d == 0 or g.ne[d] > 1:
                    assert T.nb[d] == g.nb[d], (case.id, d, T.nb, g.nb)
            assert tuple(parent.ne) == tuple(g.pne) and parent.nbytes() == L.parent_bytes(ty, g.pne)
            assert (T.t.view_offs if T is not parent else 0) == g.off
            assert g.off + T.nbytes() <= parent.nbytes(), case.id                # the view lies inside its parent
        y = t["y"]
        ne12, ne13 = L.ne1x(case)
        assert tuple(y.ne) == (case.M, case.N, ne12, ne13)
    for name, wtype, K, geo in L.DECLINED:
        c = pkg.Context(None)
        parent, w = L.build_view(c, c, wtype, geo)
        assert tuple(w.ne) == tuple(geo.ne) and w.nb[1] == geo.nb[1] and w.t.view_offs == geo.off, name
