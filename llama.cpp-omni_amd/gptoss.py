"""Host-side mirror of the reference's mixture-of-experts feed-forward block (llm_graph_context::build_moe_ffn, reference
src/llama-graph.cpp:877-1106) as gpt-oss calls it (llm_build_openai_moe_iswa, src/llama-model.cpp:18644-18654: a router bias,
SOFTMAX_WEIGHT gating -- the soft-max runs over the SELECTED logits --, per-expert biases through ADD_ID, SWIGLU_OAI with
alpha 1.702 / limit 7, no norm_w, no weight scale), built with the ctypes graph builder of ggml.py.

It emits exactly the node sequence graph_compute receives from libllama for one ubatch, including the two
ggml_build_forward_expand() calls in the middle of the block.  No arithmetic is done here.
"""
import numpy as np

from .ggml import GGML_BACKEND_BUFFER_USAGE_WEIGHTS, GGML_TYPE_F32, GGML_TYPE_MXFP4, Context
from .qwen3 import random_blocks

TINY_GPTOSS = dict(n_embd=256, n_expert=8, n_expert_used=4, n_ff_exp=288)
GPT_OSS_20B = dict(n_embd=2880, n_expert=32, n_expert_used=4, n_ff_exp=2880)
SWIGLU_OAI_ALPHA, SWIGLU_OAI_LIMIT = 1.702, 7.0                                     # (llama-graph.cpp:1047-1048)


def build_moe_ffn(g, cur, gate_inp, gate_inp_b, up_exps, up_exps_b, gate_exps, gate_exps_b, down_exps, down_exps_b, n_expert, n_expert_used, roots=None):
    """cur [n_embd, n_tokens] f32 -> moe_out [n_embd, n_tokens]; returns (moe_out, named intermediate nodes).
    `roots` (a list) receives the tensors ggml_build_forward_expand() is called on inside the block, in call order; the
    caller appends its own root (moe_out or what follows it) behind them."""
    n_embd, n_tokens = cur.ne[0], cur.ne[1]
    roots = roots if roots is not None else []
    N = {}
    logits = g.mul_mat(gate_inp, cur)                                              # [n_expert, n_tokens]   ffn_moe_logits
    logits = g.add(logits, gate_inp_b)                                             #                        ffn_moe_logits_biased
    probs = logits                                                                 # SOFTMAX_WEIGHT         ffn_moe_probs
    selected = g.top_k(probs, n_expert_used)                                       # [n_expert_used, n_tokens] i32: ARGSORT + VIEW   ffn_moe_argsort / ffn_moe_topk
    N.update(logits=logits, argsort=selected._view_of, selected=selected)
    probs3 = g.reshape(probs, 1, n_expert, n_tokens)
    weights = g.get_rows(probs3, selected)                                         # [1, n_expert_used, n_tokens]   ffn_moe_weights
    weights = g.reshape(weights, n_expert_used, n_tokens)
    weights = g.soft_max_ext(weights, None, 1.0, 0.0)                              # ggml_soft_max          ffn_moe_weights_softmax
    weights = g.reshape(weights, 1, n_expert_used, n_tokens)
    roots.append(weights)                                                          # "call early so that topk-moe can be used"
    N["weights"] = weights
    cur = g.reshape(cur, n_embd, 1, n_tokens)
    up = g.mul_mat_id(up_exps, cur, selected)                                      # [n_ff, n_expert_used, n_tokens]   ffn_moe_up
    up = g.add_id(up, up_exps_b, selected)                                         #                                   ffn_moe_up_biased
    gate = g.mul_mat_id(gate_exps, cur, selected)                                  #                                   ffn_moe_gate
    gate = g.add_id(gate, gate_exps_b, selected)                                   #                                   ffn_moe_gate_biased
    act = g.swiglu_oai(gate, up, SWIGLU_OAI_ALPHA, SWIGLU_OAI_LIMIT)               #                                   ffn_moe_swiglu_oai
    experts = g.mul_mat_id(down_exps, act, selected)                               # [n_embd, n_expert_used, n_tokens] ffn_moe_down
    experts = g.add_id(experts, down_exps_b, selected)                             #                                   ffn_moe_down_biased
    experts = g.mul(experts, weights)                                              #                                   ffn_moe_weighted
    N.update(up=up, gate=gate, act=act, experts=experts)
    cur_experts = []
    for i in range(n_expert_used):                                                 # "order the views before the adds"
        v = g.view_2d(experts, n_embd, n_tokens, experts.nb[2], i * experts.nb[1])
        cur_experts.append(v)
        roots.append(v)
    moe_out = cur_experts[0]
    for i in range(1, n_expert_used):
        moe_out = g.add(moe_out, cur_experts[i])
    if n_expert_used == 1:
        moe_out = g.cont(moe_out)                                                  # "avoid returning a non-contiguous tensor"
    N["moe_out"] = moe_out
    return moe_out, N


_WEIGHTS = ("gate_inp", "gate_inp_b", "up_exps", "up_exps_b", "gate_exps", "gate_exps_b", "down_exps", "down_exps_b")


class GptOssBlock:
    """The expert weights and biases of one layer resident in a weights buffer, and the block's graph for one ubatch (tests, tools/moe_mmv_bench.py)."""

    def __init__(self, be, cfg=TINY_GPTOSS, seed=11, weights=None, std=0.05):
        self.be, self.cfg = be, cfg
        E, X, F = cfg["n_embd"], cfg["n_expert"], cfg["n_ff_exp"]
        w = self.wctx = Context(be)
        self.gate_inp = w.new_tensor(GGML_TYPE_F32, E, X)
        self.gate_inp_b = w.new_tensor(GGML_TYPE_F32, X)
        self.up_exps = w.new_tensor(GGML_TYPE_MXFP4, E, F, X)
        self.up_exps_b = w.new_tensor(GGML_TYPE_F32, F, X)
        self.gate_exps = w.new_tensor(GGML_TYPE_MXFP4, E, F, X)
        self.gate_exps_b = w.new_tensor(GGML_TYPE_F32, F, X)
        self.down_exps = w.new_tensor(GGML_TYPE_MXFP4, F, E, X)
        self.down_exps_b = w.new_tensor(GGML_TYPE_F32, E, X)
        w.alloc(usage=GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
        if weights is None:
            rng = np.random.default_rng(seed)
            weights = dict(gate_inp=(rng.standard_normal((X, E)) / np.sqrt(E)).astype(np.float32),
                           gate_inp_b=rng.uniform(-0.05, 0.05, X).astype(np.float32),
                           up_exps=random_blocks(rng, GGML_TYPE_MXFP4, F * X, E, std=std), up_exps_b=rng.standard_normal((X, F)).astype(np.float32),
                           gate_exps=random_blocks(rng, GGML_TYPE_MXFP4, F * X, E, std=std), gate_exps_b=rng.standard_normal((X, F)).astype(np.float32),
                           down_exps=random_blocks(rng, GGML_TYPE_MXFP4, E * X, F, std=std), down_exps_b=rng.standard_normal((X, E)).astype(np.float32))
        self.weights = weights
        for k in _WEIGHTS:
            be.tensor_set(getattr(self, k), weights[k])

    def _w(self, g, real):
        T = g._new(real.type, real.ne, view_src=real, view_offs=0)
        for i in range(4):
            T.t.nb[i] = real.t.nb[i]
        return T

    def build(self, n_tokens):
        """-> (graph context, input tensor [n_embd, n_tokens], named nodes); the graph's node order is ggml_build_forward_expand's over the block's roots"""
        g = Context(self.be)
        x = g.new_tensor(GGML_TYPE_F32, self.cfg["n_embd"], n_tokens)
        roots = []
        out, N = build_moe_ffn(g, x, *[self._w(g, getattr(self, k)) for k in _WEIGHTS], self.cfg["n_expert"], self.cfg["n_expert_used"], roots=roots)
        roots.append(out)
        g.roots = roots
        g.alloc()
        return g, x, N
