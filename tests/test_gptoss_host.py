"""Host side of the gpt-oss path (no GPU): llama.cpp-omni_amd/gptoss.py emits the node sequence of the reference's build_moe_ffn for the arguments of
llm_build_openai_moe_iswa (src/llama-graph.cpp:877-1106, src/llama-model.cpp:18644-18654, as ggml_build_forward_expand orders it), the add_id / swiglu_oai
constructors of ggml.py reject what ggml.c:1985-1988 / :2731-2737 reject, and the MXFP4 type table entry gives the reference's row sizes."""
import struct

import pytest

F32, F16, I32, MXFP4 = 0, 1, 26, 39


def _f32(bits):
    return struct.unpack("<f", struct.pack("<i", bits))[0]


def _block(pkg, n_tokens, n_used):
    from llama_cpp_omni_amd import gptoss
    E, X, F = 256, 8, 288
    g = pkg.Context(None)
    x = g.new_tensor(F32, E, n_tokens)
    w = dict(gate_inp=g.new_tensor(F32, E, X), gate_inp_b=g.new_tensor(F32, X),
             up=g.new_tensor(MXFP4, E, F, X), up_b=g.new_tensor(F32, F, X), gate=g.new_tensor(MXFP4, E, F, X), gate_b=g.new_tensor(F32, F, X),
             down=g.new_tensor(MXFP4, F, E, X), down_b=g.new_tensor(F32, E, X))
    roots = []
    out, N = gptoss.build_moe_ffn(g, x, w["gate_inp"], w["gate_inp_b"], w["up"], w["up_b"], w["gate"], w["gate_b"], w["down"], w["down_b"], X, n_used, roots=roots)
    roots.append(out)
    return g, g.graph_expand(roots), N, w


def test_gptoss_moe_ffn_node_sequence(pkg):
    OP = pkg.OP
    g, gr, N, w = _block(pkg, 5, 4)
    want = [OP.MUL_MAT, OP.ADD, OP.RESHAPE, OP.ARGSORT, OP.VIEW, OP.GET_ROWS, OP.RESHAPE, OP.SOFT_MAX, OP.RESHAPE,                     # the router chain, expanded first
            OP.RESHAPE, OP.MUL_MAT_ID, OP.ADD_ID, OP.MUL_MAT_ID, OP.ADD_ID, OP.GLU, OP.MUL_MAT_ID, OP.ADD_ID, OP.MUL,                  # SWIGLU_OAI's src0 is the gate: expanded first
            OP.VIEW, OP.VIEW, OP.VIEW, OP.VIEW, OP.ADD, OP.ADD, OP.ADD]                                                                # views before the adds
    assert [n.t.op for n in gr.nodes] == want
    sel = N["selected"]
    assert sel.ne == (4, 5, 1, 1) and sel.nb[1] == 8 * 4 and sel.t.view_offs == 0                  # top-k: a strided view of the [n_expert, n_tokens] sort
    assert N["argsort"]._srcs[0] is N["logits"] and N["logits"].t.op == OP.ADD                      # SOFTMAX_WEIGHT: the sort reads the biased logits themselves
    sm = [n for n in gr.nodes if n.t.op == OP.SOFT_MAX]
    assert len(sm) == 1 and sm[0].ne == (4, 5, 1, 1)                                               # ... and the soft-max runs over the SELECTED logits
    ids_of = [n for n in gr.nodes if n.t.op == OP.MUL_MAT_ID]
    assert [n._srcs[0] for n in ids_of] == [w["gate"], w["up"], w["down"]]
    assert all(n._srcs[2] is sel for n in ids_of)
    assert ids_of[0]._srcs[1] is ids_of[1]._srcs[1] and ids_of[0]._srcs[1].ne == (256, 1, 5, 1)    # gate and up read the same [n_embd, 1, n_tokens] reshape
    bias_of = [n for n in gr.nodes if n.t.op == OP.ADD_ID]
    assert [n._srcs[1] for n in bias_of] == [w["gate_b"], w["up_b"], w["down_b"]]
    assert [n._srcs[0] for n in bias_of] == ids_of and all(n._srcs[2] is sel for n in bias_of)     # every bias sits on its expert product, with the same ids
    act = N["act"]
    assert act.ne == (288, 4, 5, 1) and act.t.op_params[0] == pkg.GLU.SWIGLU_OAI == 3 and act.t.op_params[1] == 0
    assert _f32(act.t.op_params[2]) == pytest.approx(1.702, rel=1e-7) and _f32(act.t.op_params[3]) == 7.0
    assert act._srcs[0] is N["gate"] and act._srcs[1] is N["up"] and ids_of[2]._srcs[1] is act
    assert N["experts"].ne == (256, 4, 5, 1) and N["weights"].ne == (1, 4, 5, 1)
    views = [n for n in gr.nodes if n.t.op == OP.VIEW][1:]
    assert [v.t.view_offs for v in views] == [i * N["experts"].nb[1] for i in range(4)] and all(v.nb[1] == N["experts"].nb[2] and v.ne == (256, 5, 1, 1) for v in views)


def test_gptoss_moe_ffn_one_expert_used_ends_in_cont(pkg):
    OP = pkg.OP
    g, gr, N, _ = _block(pkg, 3, 1)
    assert [n.t.op for n in gr.nodes][-5:] == [OP.MUL_MAT_ID, OP.ADD_ID, OP.MUL, OP.VIEW, OP.CONT]


def test_add_id_constructor_asserts(pkg):
    g = pkg.Context(None)
    a, b, ids = g.new_tensor(F32, 288, 4, 5), g.new_tensor(F32, 288, 8), g.new_tensor(I32, 4, 5)
    y = g.add_id(a, b, ids)
    assert y.ne == (288, 4, 5, 1) and y.type == F32 and y.t.op == pkg.OP.ADD_ID == 3
    assert [bool(y.t.src[k]) for k in range(4)] == [True, True, True, False]
    bad = [
        (a, g.new_tensor(F32, 256, 8), ids),                               # row length mismatch
        (a, b, g.new_tensor(I32, 2, 5)),                                   # a.ne1 != ids.ne0
        (a, b, g.new_tensor(I32, 4, 6)),                                   # a.ne2 != ids.ne1
        (a, b, g.new_tensor(F32, 4, 5)),                                   # ids not i32
    ]
    for a_, b_, i_ in bad:
        with pytest.raises(AssertionError):
            g.add_id(a_, b_, i_)


def test_swiglu_oai_constructor(pkg):
    g = pkg.Context(None)
    a, b = g.new_tensor(F32, 128, 2, 2, 2), g.new_tensor(F32, 128, 2, 2, 2)
    y = g.swiglu_oai(a, b, 1.702, 7.0)
    assert y.ne == (128, 2, 2, 2) and y.t.op == pkg.OP.GLU and list(y.t.op_params[:2]) == [3, 0]
    assert _f32(y.t.op_params[2]) == pytest.approx(1.702, rel=1e-7) and _f32(y.t.op_params[3]) == 7.0
    one = g.swiglu_oai(a, None, 0.5, 2.0)                                  # single-tensor form: half the row each
    assert one.ne == (64, 2, 2, 2) and not one.t.src[1] and _f32(one.t.op_params[2]) == 0.5 and _f32(one.t.op_params[3]) == 2.0
    wide = g.new_tensor(F32, 384, 2, 2, 2)
    rows = g.view_4d(wide, 128, 2, 2, 2, wide.nb[1], wide.nb[2], wide.nb[3], 0)      # rows of a 3x wider tensor: contiguous from dimension 1 up
    assert g.swiglu_oai(rows, rows, 1.0, 1.0).ne == (128, 2, 2, 2)
    bad = [
        (a, g.new_tensor(F32, 128, 2, 2, 3)),                              # not the same shape
        (a, g.new_tensor(F16, 128, 2, 2, 2)),                              # not the same type
        (g.permute(a, 0, 2, 1, 3), b),                                     # a not contiguous from dimension 1 up
        (a, g.permute(b, 0, 2, 1, 3)),
    ]
    for a_, b_ in bad:
        with pytest.raises(AssertionError):
            g.swiglu_oai(a_, b_, 1.702, 7.0)


def test_mxfp4_row_size(pkg):
    assert pkg.type_traits(MXFP4)[:2] == (32, 17)
    assert pkg.row_size(MXFP4, 2880) == 1530 and pkg.row_size(MXFP4, 288) == 153 and pkg.row_size(MXFP4, 32) == 17
    with pytest.raises(AssertionError):
        pkg.row_size(MXFP4, 48)
    g = pkg.Context(None)
    t = g.new_tensor(MXFP4, 288, 256, 8)
    assert t.nb == (17, 153, 153 * 256, 153 * 256 * 8) and t.nbytes() == 153 * 256 * 8


def test_random_blocks_mxfp4_are_unit_order(pkg):
    import numpy as np
    from llama_cpp_omni_amd import qwen3
    kv = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], np.float64)
    blk = qwen3.random_blocks(np.random.default_rng(1), MXFP4, 64, 288, std=1.0).reshape(64, 9, 17)
    assert blk.dtype == np.uint8
    w = np.concatenate([kv[blk[..., 1:] & 15], kv[blk[..., 1:] >> 4]], axis=-1) * np.exp2(blk[..., :1].astype(np.float64) - 128)      # value = kv[q] * 2^(e - 127) / 2
    assert 0.4 < w.std() < 2.5 and abs(w.mean()) < 0.1
