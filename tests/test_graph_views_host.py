"""Context.graph_parent / Graph.view (ggml.py): the visited hash set, `used` bitset and use counts a scheduler split carries, against the real reference.

The executor decides from these arrays which tensors a later split reads (graph_exec_internal.hpp is_out, graph_internal.hpp whole_use_count), so the GPU tests that
submit split views (test_fusion_observed_gpu.py) are worth what this mirror is worth.  Here it is compared slot for slot with what the reference's own
ggml_new_graph_custom + ggml_build_forward_expand leave behind for the SAME tensors (the reference only walks src pointers, so it takes the Python-made structs as
they are), and ggml_graph_view with Graph.view; a second case builds the tight, crowded table the GPU tests use and asserts what it is built for.  No GPU.
"""
import ctypes as C

import pytest

from graph_views import crowd, home, wraps


def _sample(pkg):
    """a small graph with what moves the counts: a leaf with two readers, a node with two readers, view nodes (RESHAPE, VIEW, PERMUTE), a CPY into a view (two sources), a GLU"""
    F32 = pkg.GGML_TYPE_F32
    c = pkg.Context(None)
    x, w, r = c.new_tensor(F32, 64, 8), c.new_tensor(F32, 64, 32), c.new_tensor(F32, 32, 8)
    cache = c.new_tensor(F32, 32, 16)
    a = c.mul_mat(w, x)                                                 # [32, 8]
    b = c.add(a, r)
    h = c.mul(c.rms_norm(b, 1e-6), c.new_tensor(F32, 32))
    g = c.swiglu_split(h, c.scale(b, 0.5))
    v = c.view_2d(cache, 32, 8, cache.t.nb[1], 4 * cache.t.nb[1])
    st = c.cpy(g, v)
    p = c.cont(c.permute(c.reshape(b, 8, 4, 8), 1, 0, 2, 3))
    out = c.add(c.reshape(p, 32, 8), a)
    return c, [b, h, g, st, out]


def _ref_or_skip():
    from oracle.ref_backend import ref_available, ref_lib
    if not ref_available():
        pytest.skip("oracle/_ref/libggml-ref.so not built")
    lib = ref_lib()
    for name in ("ggml_init", "ggml_free", "ggml_new_graph_custom", "ggml_build_forward_expand", "ggml_graph_overhead_custom", "ggml_tensor_overhead"):
        if not hasattr(lib, name):
            pytest.skip(f"the reference library does not export {name}")
    return lib


class _init_params(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


def _used(bits, i):
    return (bits[i >> 5] >> (i & 31)) & 1


@pytest.mark.parametrize("spare_leafs", [0, "fill"])
def test_parent_table_matches_the_reference_slot_for_slot(pkg, spare_leafs):
    lib = _ref_or_skip()
    c, _ = _sample(pkg)
    nodes = list(c.nodes)
    n = len(nodes)
    g0 = c.graph_parent(nodes)
    spares = []
    if spare_leafs == "fill":                                           # as many leafs as nodes: ggml_new_graph_custom(n) then makes the table exactly ggml_hash_size(nodes + leafs)
        spares = [c.new_tensor(pkg.GGML_TYPE_F32, 1) for _ in range(n - g0.g.n_leafs)]
    assert g0.g.n_leafs + len(spares) <= n
    g = c.graph_parent(nodes, size=2 * n, leafs=spares)

    lib.ggml_init.restype = C.c_void_p
    lib.ggml_init.argtypes = [_init_params]
    lib.ggml_free.argtypes = [C.c_void_p]
    lib.ggml_graph_overhead_custom.restype = C.c_size_t
    lib.ggml_graph_overhead_custom.argtypes = [C.c_size_t, C.c_bool]
    lib.ggml_new_graph_custom.restype = C.POINTER(pkg.ggml_cgraph)
    lib.ggml_new_graph_custom.argtypes = [C.c_void_p, C.c_size_t, C.c_bool]
    lib.ggml_build_forward_expand.restype = None
    lib.ggml_build_forward_expand.argtypes = [C.POINTER(pkg.ggml_cgraph), C.POINTER(pkg.ggml_tensor)]
    ctx = lib.ggml_init(_init_params(lib.ggml_graph_overhead_custom(n, False) + 4096, None, True))
    assert ctx
    try:
        rg = lib.ggml_new_graph_custom(ctx, n, False)
        for T in spares + nodes:                                        # the order graph_parent enters them in
            lib.ggml_build_forward_expand(rg, T.ptr)
        r = rg.contents
        H = r.visited_hash_set.size
        assert H == g.hash_size == pkg.ggml_hash_size(2 * n) == g.g.visited_hash_set.size
        assert r.n_nodes == n == g.g.n_nodes and r.n_leafs == g.g.n_leafs
        for i in range(n):                                              # expanding every node in creation order leaves the nodes in that order
            assert C.addressof(r.nodes[i].contents) == C.addressof(nodes[i].t)
        r_leafs = C.cast(r.leafs, C.POINTER(C.c_void_p))
        assert [r_leafs[i] for i in range(r.n_leafs)] == g.leafs
        r_used = C.cast(r.visited_hash_set.used, C.POINTER(C.c_uint32))
        r_keys = C.cast(r.visited_hash_set.keys, C.POINTER(C.c_void_p))
        r_cnt = C.cast(r.use_counts, C.POINTER(C.c_int32))
        held = 0
        for i in range(H):
            assert _used(r_used, i) == _used(g.used, i), i
            if _used(r_used, i):
                held += 1
                assert r_keys[i] == g.keys[i], i
                assert r_cnt[i] == g.use_counts[i], i
        assert held == n + r.n_leafs
        if spare_leafs == "fill":
            assert held == 2 * n                                        # the tight table
        by = {C.addressof(T.t): T for T in c.tensors}                   # the counts are what this graph says they are: b has three readers, a two, the cache only its view
        assert g.use_count(nodes[1]) == 3 and g.use_count(nodes[0]) == 2 and g.use_count(nodes[-1]) == 0 and len(by) >= held - len(spares)

        # ggml_graph_view against Graph.view
        if not hasattr(lib, "ggml_graph_view"):
            return                                                      # (ggml-impl.h declares it without GGML_API: a build that hides it leaves the parent compared, the view not)
        lib.ggml_graph_view.restype = pkg.ggml_cgraph
        lib.ggml_graph_view.argtypes = [C.POINTER(pkg.ggml_cgraph), C.c_int, C.c_int]
        for i0, i1 in ((0, n), (0, 5), (5, n), (3, 4)):
            rv, v = lib.ggml_graph_view(rg, i0, i1), c.graph_parent(nodes, size=2 * n, leafs=spares).view(i0, i1)
            pv = g.view(i0, i1)
            for vv in (v, pv):
                assert (rv.size, rv.n_nodes, rv.n_leafs, rv.order) == (vv.g.size, vv.g.n_nodes, vv.g.n_leafs, vv.g.order)
                assert not rv.grads and not rv.leafs and not vv.g.grads and not vv.g.leafs
                for i in range(i1 - i0):
                    assert C.addressof(rv.nodes[i].contents) == C.addressof(vv.g.nodes[i].contents) == C.addressof(nodes[i0 + i].t)
                assert rv.visited_hash_set.size == vv.g.visited_hash_set.size
            # the view shares its parent's arrays, on both sides
            assert rv.use_counts == r.use_counts and rv.visited_hash_set.keys == r.visited_hash_set.keys and rv.visited_hash_set.used == r.visited_hash_set.used
            assert pv.g.use_counts == g.g.use_counts and pv.g.visited_hash_set.keys == g.g.visited_hash_set.keys and pv.g.visited_hash_set.used == g.g.visited_hash_set.used
    finally:
        lib.ggml_free(ctx)


def test_plain_graph_carries_no_counts(pkg):
    c, _ = _sample(pkg)
    g = c.graph()
    assert not g.g.use_counts and g.g.visited_hash_set.size == 0 and not g.g.visited_hash_set.keys and not g.g.visited_hash_set.used


def test_tight_table_displaces_a_node_and_wraps(pkg):
    """the construction the GPU tests use: size = nodes + leafs, a spare leaf in the target node's home slot, two spares whose home is the last slot"""
    c, (b, h, g_, st, out) = _sample(pkg)
    nodes = list(c.nodes)
    for target in (b, g_):
        spares, size = crowd(pkg, c, nodes, target)
        g = c.graph_parent(nodes, size=size, leafs=spares)
        assert size == len(nodes) + g.g.n_leafs                         # tight: one slot per tensor asked for, and ggml_hash_size rounds up to the prime
        assert g.hash_size == pkg.ggml_hash_size(size) and g.hash_size - size < size
        slot, hm = g.slot_of(target)
        assert hm == home(target, g.hash_size)
        assert slot is not None and slot != hm                          # the node's key lies off its home slot ...
        assert g.keys[hm] == C.addressof(spares[0].t)                   # ... because a spare sits there
        assert any(wraps(g, T) for T in spares)                         # and a probe sequence runs past the end of the table
        assert wraps(g, spares[2]) and home(spares[2], g.hash_size) == g.hash_size - 1
        # every tensor is found again by probing, with the counts of the roomy table
        roomy = c.graph_parent(nodes)
        for T in nodes:
            assert g.use_count(T) == roomy.use_count(T) >= 0
        for T in spares:
            assert g.use_count(T) == 0
        assert g.use_count(b) == 3
        v = g.view(0, 4)
        assert v.use_count(b) == 3 and v.g.n_nodes == 4
