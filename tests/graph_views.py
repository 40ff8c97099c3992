"""Crowded parent tables for the graph-view tests (test_graph_views_host.py, test_fusion_observed_gpu.py).

Context.graph_parent() builds the visited hash set and use counts a scheduler split carries.  Where a tensor lands in that table depends on its address, which a
test does not choose -- but it can choose its NEIGHBOURS: spare leaf tensors that no node reads, picked from a pool by their home slot and entered first.
crowd() picks them so that a given node's key lies off its home slot and so that one probe sequence runs past the end of the table, in a table exactly as large
as ggml_hash_size(number of nodes + leafs) makes it.
"""
import ctypes as C


def home(T, H):
    return (C.addressof(T.t) >> 4) % H


def crowd(pkg, ctx, nodes, target):
    """-> (spares, size): spare leaf tensors (kept alive by the caller, never allocated: nobody reads them) and the `size` for Context.graph_parent(nodes, size, spares)
    = number of nodes + leafs, spares included.  In that table `target` is displaced by a spare sitting in its home slot, and a spare whose home is the last slot wraps."""
    held = {C.addressof(T.t) for T in nodes}
    todo = [T.t for T in nodes]
    while todo:
        t = todo.pop()
        for k in range(10):
            if t.src[k] and C.addressof(t.src[k].contents) not in held:
                held.add(C.addressof(t.src[k].contents))
                todo.append(t.src[k].contents)
    s0 = len(held)
    primes = [p for p in (37, 67, 131, 257, 521, 1031, 2053) if p >= s0 + 3]
    H, prev = primes[0], max(p for p in (17, 37, 67, 131, 257, 521, 1031) if p < primes[0])
    size = max(prev + 1, s0 + 3)
    assert pkg.ggml_hash_size(size) == H

    def candidate():
        t = pkg.ggml_tensor()
        t.type = pkg.GGML_TYPE_F32
        for i in range(4):
            t.ne[i], t.nb[i] = 1, 4
        return pkg.Tensor(ctx, t)

    pool = [candidate() for _ in range(40 * H)]
    ht = home(target, H)
    at_home = [T for T in pool if home(T, H) == ht]
    at_end = [T for T in pool if home(T, H) == H - 1 and T not in at_home[:1]]
    assert at_home and len(at_end) >= 2, "the pool holds no tensor for a wanted slot"
    spares = [at_home[0], at_end[0], at_end[1]]
    chosen = {id(T) for T in spares}
    for T in pool:
        if len(spares) == size - s0:
            break
        if id(T) not in chosen:
            spares.append(T)
    return spares, size


def wraps(g, T):
    """does T's probe sequence run past the end of the table?  (its slot lies in front of its home slot)"""
    slot, h = g.slot_of(T)
    return slot is not None and slot < h
