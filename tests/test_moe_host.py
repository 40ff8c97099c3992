"""Host side of the mixture-of-experts path (no GPU): llama.cpp-omni_amd/qwen3moe.py emits the node sequence of the reference's build_moe_ffn
(src/llama-graph.cpp:877-1106, as ggml_build_forward_expand orders it), and the new constructors of ggml.py reject what ggml.c:3088-3096 / :4994 reject."""
import pytest

F32, F16, I32, Q4_K, Q6_K = 0, 1, 26, 12, 14


def _block(pkg, n_tokens, n_used, norm_w=True):
    from llama_cpp_omni_amd import qwen3moe
    E, X, F = 256, 8, 256
    g = pkg.Context(None)
    x = g.new_tensor(F32, E, n_tokens)
    gate_inp = g.new_tensor(F32, E, X)
    up, gate, down = g.new_tensor(Q4_K, E, F, X), g.new_tensor(Q4_K, E, F, X), g.new_tensor(Q6_K, F, E, X)
    roots = []
    out, N = qwen3moe.build_moe_ffn(g, x, gate_inp, up, gate, down, X, n_used, norm_w=norm_w, roots=roots)
    roots.append(out)
    return g, g.graph_expand(roots), N, (x, gate_inp, up, gate, down)


def test_moe_ffn_node_sequence(pkg):
    OP = pkg.OP
    g, gr, N, (x, gate_inp, up, gate, down) = _block(pkg, 5, 2)
    want = [OP.MUL_MAT, OP.SOFT_MAX, OP.RESHAPE, OP.ARGSORT, OP.VIEW, OP.GET_ROWS, OP.RESHAPE, OP.SUM_ROWS, OP.DIV, OP.RESHAPE,      # the router chain, expanded first
            OP.RESHAPE, OP.MUL_MAT_ID, OP.MUL_MAT_ID, OP.GLU, OP.MUL_MAT_ID, OP.MUL, OP.VIEW, OP.VIEW, OP.ADD]                       # experts, weighting, views before the adds
    assert [n.t.op for n in gr.nodes] == want
    # shapes and operands of the nodes the backend's new kernels take
    assert N["argsort"].ne == (8, 5, 1, 1) and N["argsort"].type == I32 and N["argsort"].t.op_params[0] == pkg.SORT_ORDER.DESC
    sel = N["selected"]
    assert sel.ne == (2, 5, 1, 1) and sel.nb[1] == 8 * 4 and sel.t.view_offs == 0                  # top-k: a strided view of the [n_expert, n_tokens] sort
    assert N["up"].ne == (256, 2, 5, 1) and N["gate"].ne == (256, 2, 5, 1) and N["experts"].ne == (256, 2, 5, 1)
    ids_of = [n for n in gr.nodes if n.t.op == OP.MUL_MAT_ID]
    assert [n._srcs[0] for n in ids_of] == [gate, up, down]                                        # SWIGLU's src0 is the gate product: it is expanded first
    assert all(n._srcs[2] is sel for n in ids_of)
    assert ids_of[0]._srcs[1] is ids_of[1]._srcs[1] and ids_of[0]._srcs[1].ne == (256, 1, 5, 1)    # gate and up read the same [n_embd, 1, n_tokens] reshape
    assert ids_of[2]._srcs[1] is N["act"] and N["act"].t.op_params[0] == pkg.GLU.SWIGLU
    assert N["weights"].ne == (1, 2, 5, 1)
    views = [n for n in gr.nodes if n.t.op == OP.VIEW][1:]
    assert [v.t.view_offs for v in views] == [0, N["experts"].nb[1]] and all(v.nb[1] == N["experts"].nb[2] and v.ne == (256, 5, 1, 1) for v in views)


def test_moe_ffn_one_expert_used_ends_in_cont_and_norm_w_is_optional(pkg):
    OP = pkg.OP
    g, gr, N, _ = _block(pkg, 3, 1)
    assert [n.t.op for n in gr.nodes][-4:] == [OP.MUL_MAT_ID, OP.MUL, OP.VIEW, OP.CONT]
    g, gr, N, _ = _block(pkg, 3, 2, norm_w=False)
    ops = [n.t.op for n in gr.nodes]
    assert OP.SUM_ROWS not in ops and OP.DIV not in ops and ops[:6] == [OP.MUL_MAT, OP.SOFT_MAX, OP.RESHAPE, OP.ARGSORT, OP.VIEW, OP.GET_ROWS]


def test_mul_mat_id_constructor_asserts(pkg):
    g = pkg.Context(None)
    as_ = g.new_tensor(Q4_K, 256, 64, 8)
    b = g.new_tensor(F32, 256, 1, 5)
    ids = g.new_tensor(I32, 2, 5)
    y = g.mul_mat_id(as_, b, ids)
    assert y.ne == (64, 2, 5, 1) and y.type == F32 and y.t.op == pkg.OP.MUL_MAT_ID
    assert g.mul_mat_id(as_, g.new_tensor(F32, 256, 2, 5), ids).ne == (64, 2, 5, 1)               # b per slot
    bad = [
        (as_, b, g.new_tensor(F32, 2, 5)),                                 # ids not i32
        (g.new_tensor(Q4_K, 256, 64, 8, 2), b, ids),                       # as 4-D
        (as_, g.new_tensor(F32, 256, 1, 5, 2), ids),                       # b 4-D
        (as_, b, g.new_tensor(I32, 2, 5, 2)),                              # ids 3-D
        (as_, b, g.new_tensor(I32, 2, 4)),                                 # no expert list per b row
        (as_, g.new_tensor(F32, 512, 1, 5), ids),                          # K mismatch
        (as_, g.new_tensor(F32, 256, 3, 5), g.new_tensor(I32, 4, 5)),      # 4 slots cannot broadcast 3 columns
        (g.transpose(g.new_tensor(F32, 64, 256, 8)), b, ids),              # as transposed
    ]
    for a_, b_, i_ in bad:
        with pytest.raises(AssertionError):
            g.mul_mat_id(a_, b_, i_)


def test_argsort_and_top_k_constructors(pkg):
    g = pkg.Context(None)
    a = g.new_tensor(F32, 60, 3, 2, 2)
    s = g.argsort(a, pkg.SORT_ORDER.ASC)
    assert s.ne == a.ne and s.type == I32 and s.t.op == pkg.OP.ARGSORT and s.t.op_params[0] == 0
    t = g.top_k(a, 4)
    assert t.t.op == pkg.OP.VIEW and t.ne == (4, 3, 2, 2) and t.nb[1:] == (240, 720, 1440) and t._view_of.t.op_params[0] == 1
    with pytest.raises(AssertionError):
        g.top_k(a, 61)
