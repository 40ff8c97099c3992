"""Host-side mirror of the reference's multi-head latent attention block (DeepSeek-V2 / V3 / R1: llm_build_deepseek2, reference
src/llama-model.cpp:13560-13653, the `is_mla` branch) and of what build_attn / build_attn_mha make of it with flash attention on
(reference src/llama-graph.cpp: the K / V cache stores, the get_k / get_v views, FLASH_ATTN_EXT, and the `v_mla` product :1349-1359),
built with the ctypes graph builder of ggml.py.

It emits the node sequence graph_compute receives from libllama for one ubatch: q (wq, or wq_a -> RMS norm -> wq_b), the q_nope / q_pe
views, kv_cmpr_pe = wkv_a_mqa . cur and its kv_cmpr / k_pe views, RoPE on q_pe and k_pe, the RMS norm of kv_cmpr; then the absorption:
q_nope permuted -> MUL_MAT on the 3-D wk_b -> permuted back -> CONCAT(q_pe, q_nope_absorbed) = Qcur [rope + kv_lora_rank, n_head, n_tokens];
Kcur = CONCAT(k_pe, kv_cmpr) [rope + kv_lora_rank, 1, n_tokens] and Vcur = kv_cmpr [kv_lora_rank, 1, n_tokens], stored with SET_ROWS into
SEPARATE F16 K and V caches.  After the absorption the attention is MQA -- one KV head, K rows 576 wide and V rows 512 wide at the model's
sizes -- as one FLASH_ATTN_EXT; its rows are decompressed by wv_b ([kv_lora_rank, v_head, n_head], a batched MUL_MAT between two PERMUTEs),
made contiguous and projected by wo.  No arithmetic is done here.
"""
import math

import numpy as np

from .ggml import GGML_BACKEND_BUFFER_USAGE_WEIGHTS, GGML_TYPE_F16, GGML_TYPE_F32, GGML_TYPE_I32, GGML_TYPE_I64, Context

# the model's head sizes at toy width (DeepSeek-V2-Lite has no q compression: q_lora_rank 0)
TINY_MLA = dict(n_embd=256, n_head=8, kv_lora_rank=512, n_rot=64, n_nope=128, n_v=128, q_lora_rank=0, eps=1e-6, rope_base=10000.0, n_ctx_orig=4096)


def weight_shapes(hp):
    """name -> ne of the block's weights (reference llama-model.cpp load_tensors, LLM_ARCH_DEEPSEEK2 with wk_b / wv_b split from wkv_b)"""
    E, H, R, P, N, V, QL = hp["n_embd"], hp["n_head"], hp["kv_lora_rank"], hp["n_rot"], hp["n_nope"], hp["n_v"], hp["q_lora_rank"]
    sh = dict(wkv_a_mqa=(E, R + P), attn_kv_a_norm=(R,), wk_b=(N, R, H), wv_b=(R, V, H), wo=(H * V, E))
    if QL:
        sh.update(wq_a=(E, QL), attn_q_a_norm=(QL,), wq_b=(QL, H * (N + P)))
    else:
        sh.update(wq=(E, H * (N + P)))
    return sh


def build_mla_attn(g, cur, L, k_cache, v_cache, I, hp, n_tokens, n_kv, n_ctx, roots):
    """llm_build_deepseek2's self-attention with is_mla, flash attention on.  cur [n_embd, n_tokens] (after attn_norm); L: the weights of weight_shapes();
    k_cache f16 [n_rot + kv_lora_rank, n_ctx], v_cache f16 [kv_lora_rank, n_ctx]; I: inp_pos, kq_mask, k_idxs, v_idxs.  -> ([n_embd, n_tokens], named nodes)"""
    H, R, P, N, V = hp["n_head"], hp["kv_lora_rank"], hp["n_rot"], hp["n_nope"], hp["n_v"]
    hk = N + P                                                            # n_embd_head_k of the un-absorbed heads
    f32, f16 = 4, 2
    Nn = {}
    if hp["q_lora_rank"]:
        q = g.mul_mat(L["wq_a"], cur)
        q = g.mul(g.rms_norm(q, hp["eps"]), L["attn_q_a_norm"])
        q = g.mul_mat(L["wq_b"], q)
    else:
        q = g.mul_mat(L["wq"], cur)
    q_nope = g.view_3d(q, N, H, n_tokens, hk * f32, hk * f32 * H, 0)
    q_pe = g.view_3d(q, P, H, n_tokens, hk * f32, hk * f32 * H, N * f32)
    kv_cmpr_pe = g.mul_mat(L["wkv_a_mqa"], cur)
    kv_cmpr = g.view_2d(kv_cmpr_pe, R, n_tokens, (R + P) * f32, 0)
    k_pe = g.view_3d(kv_cmpr_pe, P, 1, n_tokens, (R + P) * f32, (R + P) * f32, R * f32)
    rope = dict(n_dims=P, mode=0, n_ctx_orig=hp["n_ctx_orig"], freq_base=hp["rope_base"], freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0)
    q_pe = g.rope_ext(q_pe, I["inp_pos"], None, **rope)
    k_pe = g.rope_ext(k_pe, I["inp_pos"], None, **rope)
    kv_cmpr = g.mul(g.rms_norm(kv_cmpr, hp["eps"]), L["attn_kv_a_norm"])
    # the absorption: {n_nope, n_tokens, n_head} x wk_b {n_nope, kv_lora_rank, n_head} -> {kv_lora_rank, n_tokens, n_head} -> {kv_lora_rank, n_head, n_tokens}
    q_nope = g.permute(q_nope, 0, 2, 1, 3)
    q_abs = g.mul_mat(L["wk_b"], q_nope)
    Nn["q_nope_absorbed"] = q_abs
    q_abs = g.permute(q_abs, 0, 2, 1, 3)
    Qcur = g.concat(q_pe, q_abs, 0)                                       # "rope must go first for in-place context shifting"
    kv_cmpr = g.reshape(kv_cmpr, R, 1, n_tokens)
    Kcur = g.concat(k_pe, kv_cmpr, 0)
    Vcur = kv_cmpr
    Nn.update(Qcur=Qcur, Kcur=Kcur, Vcur=Vcur)
    # build_attn: MQA, one KV head; the K / V rows of the new tokens go into their caches (cpy_k / cpy_v), the first n_kv cells are attended (get_k / get_v)
    roots += [Qcur, Kcur, Vcur]
    Nn["k_store"] = g.set_rows(k_cache, g.reshape(Kcur, P + R, n_tokens), I["k_idxs"])
    Nn["v_store"] = g.set_rows(v_cache, g.reshape(Vcur, R, n_tokens), I["v_idxs"])
    roots += [Nn["k_store"], Nn["v_store"]]
    k = g.view_4d(k_cache, P + R, 1, n_kv, 1, (P + R) * f16, (P + R) * f16, (P + R) * f16 * n_ctx, 0)
    v = g.view_4d(v_cache, R, 1, n_kv, 1, R * f16, R * f16, R * f16 * n_ctx, 0)
    qp = g.permute(Qcur, 0, 2, 1, 3)
    k = g.permute(k, 0, 2, 1, 3)
    v = g.permute(v, 0, 2, 1, 3)
    kq_scale = 1.0 / math.sqrt(hk)
    fa = g.flash_attn_ext(qp, k, v, I["kq_mask"], kq_scale)               # [kv_lora_rank, n_head, n_tokens]
    Nn["fattn"] = fa
    # v_mla: "the permutations are noops and only change how the tensor data is interpreted"
    y = g.permute(fa, 0, 2, 1, 3)
    y = g.mul_mat(L["wv_b"], y)                                           # [n_v, n_tokens, n_head]
    Nn["fattn_mla"] = y
    y = g.permute(y, 0, 2, 1, 3)
    y = g.cont(y)
    y = g.reshape(y, V * H, n_tokens)
    out = g.mul_mat(L["wo"], y)
    Nn["out"] = out
    return out, Nn


class MLABlock:
    """The block's weights (F16 matrices, F32 norms) and its two caches resident in a buffer, and the block's graph for one ubatch (tests, tools)."""

    def __init__(self, be, hp=TINY_MLA, n_ctx=64, seed=4, weights=None):
        self.be, self.hp, self.n_ctx = be, hp, n_ctx
        w = self.wctx = Context(be)
        shapes = weight_shapes(hp)
        self.types = {k: (GGML_TYPE_F32 if len(ne) == 1 else GGML_TYPE_F16) for k, ne in shapes.items()}
        self.T = {k: w.new_tensor(self.types[k], *ne) for k, ne in shapes.items()}
        self.k_cache = w.new_tensor(GGML_TYPE_F16, hp["n_rot"] + hp["kv_lora_rank"], n_ctx)
        self.v_cache = w.new_tensor(GGML_TYPE_F16, hp["kv_lora_rank"], n_ctx)
        w.alloc(usage=GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
        if weights is None:
            rng = np.random.default_rng(seed)
            weights = {}
            for k, ne in shapes.items():
                if len(ne) == 1:
                    weights[k] = rng.uniform(0.5, 1.5, ne[0]).astype(np.float32)
                else:
                    weights[k] = (rng.standard_normal(ne[::-1]) / np.sqrt(ne[0])).astype(np.float16)
        self.weights = weights
        for k in shapes:
            be.tensor_set(self.T[k], weights[k])
        be.tensor_set(self.k_cache, np.zeros((n_ctx, hp["n_rot"] + hp["kv_lora_rank"]), np.float16))
        be.tensor_set(self.v_cache, np.zeros((n_ctx, hp["kv_lora_rank"]), np.float16))

    def _w(self, g, real):
        T = g._new(real.type, real.ne, view_src=real, view_offs=0)
        for i in range(4):
            T.t.nb[i] = real.t.nb[i]
        return T

    def build(self, n_tokens, n_kv):
        """-> (graph context, inputs dict: x [n_embd, n_tokens], inp_pos, kq_mask f16 [n_kv, pad(n_tokens, 64)], k_idxs / v_idxs i64 [n_tokens]; named nodes);
        the graph's node order is ggml_build_forward_expand's over the block's roots"""
        g = Context(self.be)
        I = dict(x=g.new_tensor(GGML_TYPE_F32, self.hp["n_embd"], n_tokens), inp_pos=g.new_tensor(GGML_TYPE_I32, n_tokens),
                 kq_mask=g.new_tensor(GGML_TYPE_F16, n_kv, (n_tokens + 63) // 64 * 64),
                 k_idxs=g.new_tensor(GGML_TYPE_I64, n_tokens), v_idxs=g.new_tensor(GGML_TYPE_I64, n_tokens))
        L = {k: self._w(g, t) for k, t in self.T.items()}
        roots = []
        out, N = build_mla_attn(g, I["x"], L, self._w(g, self.k_cache), self._w(g, self.v_cache), I, self.hp, n_tokens, n_kv, self.n_ctx, roots)
        roots.append(out)
        g.roots = roots
        g.alloc()
        return g, I, N

    def set_inputs(self, I, x, pos0, n_kv):
        """n_tokens new tokens at positions pos0 .., stored into cells pos0 .., causal over the first n_kv cells (llama_kv_cache::set_input_kq_mask)"""
        be = self.be
        n_tokens = x.shape[0]
        be.tensor_set(I["x"], np.ascontiguousarray(x, np.float32))
        be.tensor_set(I["inp_pos"], np.arange(pos0, pos0 + n_tokens, dtype=np.int32))
        idx = np.arange(pos0, pos0 + n_tokens, dtype=np.int64)
        be.tensor_set(I["k_idxs"], idx); be.tensor_set(I["v_idxs"], idx)
        m = np.full((I["kq_mask"].ne[1], n_kv), -np.inf, np.float32)
        for i in range(n_tokens):
            m[i, :pos0 + i + 1] = 0.0
        m[n_tokens:] = m[n_tokens - 1]
        be.tensor_set(I["kq_mask"], m.astype(np.float16))
