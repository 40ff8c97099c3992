"""Host-side mirror of the reference's mixture-of-experts feed-forward block (llm_graph_context::build_moe_ffn, reference
src/llama-graph.cpp:877-1106) as Qwen3-MoE calls it (llm_build_qwen3moe: soft-max gating, norm_w, SwiGLU, no biases, no weight
scale), built with the ctypes graph builder of ggml.py.

It emits exactly the node sequence graph_compute receives from libllama for one ubatch -- including the two
ggml_build_forward_expand() calls in the middle of the block (the weights first, "so that topk-moe can be used", then the
per-slot views "before the adds") and the CONT of the n_expert_used == 1 case.  No arithmetic is done here.
"""
import numpy as np

from .ggml import GGML_BACKEND_BUFFER_USAGE_WEIGHTS, GGML_TYPE_F32, GGML_TYPE_Q4_K, GGML_TYPE_Q6_K, Context
from .qwen3 import random_blocks

TINY_MOE = dict(n_embd=256, n_expert=8, n_expert_used=2, n_ff_exp=256)
QWEN3_30B_A3B = dict(n_embd=2048, n_expert=128, n_expert_used=8, n_ff_exp=768)


def build_moe_ffn(g, cur, gate_inp, up_exps, gate_exps, down_exps, n_expert, n_expert_used, norm_w=True, roots=None):
    """cur [n_embd, n_tokens] f32 -> moe_out [n_embd, n_tokens]; returns (moe_out, named intermediate nodes).
    `roots` (a list) receives the tensors ggml_build_forward_expand() is called on inside the block, in call order; the
    caller appends its own root (moe_out or what follows it) behind them."""
    n_embd, n_tokens = cur.ne[0], cur.ne[1]
    roots = roots if roots is not None else []
    N = {}
    logits = g.mul_mat(gate_inp, cur)                                              # [n_expert, n_tokens]   ffn_moe_logits
    probs = g.soft_max_ext(logits, None, 1.0, 0.0)                                 # ggml_soft_max          ffn_moe_probs
    selected = g.top_k(probs, n_expert_used)                                       # [n_expert_used, n_tokens] i32: ARGSORT + VIEW   ffn_moe_argsort / ffn_moe_topk
    N.update(logits=logits, probs=probs, argsort=selected._view_of, selected=selected)
    probs3 = g.reshape(probs, 1, n_expert, n_tokens)
    weights = g.get_rows(probs3, selected)                                         # [1, n_expert_used, n_tokens]   ffn_moe_weights
    if norm_w:
        weights = g.reshape(weights, n_expert_used, n_tokens)
        weights_sum = g.sum_rows(weights)                                          # [1, n_tokens]          ffn_moe_weights_sum
        weights = g.div(weights, weights_sum)                                      #                        ffn_moe_weights_norm
        weights = g.reshape(weights, 1, n_expert_used, n_tokens)
    roots.append(weights)                                                          # "call early so that topk-moe can be used"
    N["weights"] = weights
    cur = g.reshape(cur, n_embd, 1, n_tokens)
    up = g.mul_mat_id(up_exps, cur, selected)                                      # [n_ff, n_expert_used, n_tokens]   ffn_moe_up
    gate = g.mul_mat_id(gate_exps, cur, selected)                                  #                                   ffn_moe_gate
    act = g.swiglu_split(gate, up)                                                 #                                   ffn_moe_swiglu
    experts = g.mul_mat_id(down_exps, act, selected)                               # [n_embd, n_expert_used, n_tokens] ffn_moe_down
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


class MoeBlock:
    """The expert weights of one layer resident in a weights buffer, and the block's graph for one ubatch (tests, tools/moe_mmv_bench.py)."""

    def __init__(self, be, cfg=TINY_MOE, seed=11, gate_up_type=GGML_TYPE_Q4_K, down_type=GGML_TYPE_Q6_K, weights=None, std=0.05):
        self.be, self.cfg = be, cfg
        E, X, F = cfg["n_embd"], cfg["n_expert"], cfg["n_ff_exp"]
        w = self.wctx = Context(be)
        self.gate_inp = w.new_tensor(GGML_TYPE_F32, E, X)
        self.up_exps = w.new_tensor(gate_up_type, E, F, X)
        self.gate_exps = w.new_tensor(gate_up_type, E, F, X)
        self.down_exps = w.new_tensor(down_type, F, E, X)
        w.alloc(usage=GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
        if weights is None:
            rng = np.random.default_rng(seed)
            weights = dict(gate_inp=(rng.standard_normal((X, E)) / np.sqrt(E)).astype(np.float32),
                           up_exps=random_blocks(rng, gate_up_type, F * X, E, std=std), gate_exps=random_blocks(rng, gate_up_type, F * X, E, std=std),
                           down_exps=random_blocks(rng, down_type, E * X, F, std=std))
        self.weights = weights
        for k in ("gate_inp", "up_exps", "gate_exps", "down_exps"):
            be.tensor_set(getattr(self, k), weights[k])

    def _w(self, g, real):
        T = g._new(real.type, real.ne, view_src=real, view_offs=0)
        for i in range(4):
            T.t.nb[i] = real.t.nb[i]
        return T

    def build(self, n_tokens, norm_w=True):
        """-> (graph context, input tensor [n_embd, n_tokens], named nodes); the graph's node order is ggml_build_forward_expand's over the block's roots"""
        g = Context(self.be)
        x = g.new_tensor(GGML_TYPE_F32, self.cfg["n_embd"], n_tokens)
        roots = []
        out, N = build_moe_ffn(g, x, self._w(g, self.gate_inp), self._w(g, self.up_exps), self._w(g, self.gate_exps), self._w(g, self.down_exps),
                               self.cfg["n_expert"], self.cfg["n_expert_used"], norm_w=norm_w, roots=roots)
        roots.append(out)
        g.roots = roots
        g.alloc()
        return g, x, N
