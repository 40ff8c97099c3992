"""Host-side mirrors of the two Qwen2-VL / Qwen2.5-VL graphs that rotate with ggml_rope_multi, built with the ctypes graph builder.  No arithmetic is done here.

Model: the text decoder (llm_build_qwen2vl, reference src/llama-model.cpp): qwen3.Model's layer without the q / k norms, with biased q / k / v projections and
the two rotations in mode GGML_ROPE_TYPE_MROPE over a position tensor of 4 * n_tokens entries (rows t, h, w, e: llama_batch's M-RoPE layout).  mrope=False builds
the same layer with ggml_rope_ext in NEOX mode over n_tokens positions: the graph an M-RoPE layer's launches are compared with.

vit_attention: one attention block of clip.cpp's Qwen2-VL tower (build_qwen2vl): biased q / k / v, the two rotations in mode GGML_ROPE_TYPE_VISION with sections
(d_head / 4) x 4 over 4 * n_patches positions, and soft-max attention without a mask."""
import math

import numpy as np

from . import qwen3
from .ggml import (GGML_BACKEND_BUFFER_USAGE_WEIGHTS, GGML_ROPE_TYPE_MROPE, GGML_ROPE_TYPE_NEOX, GGML_ROPE_TYPE_VISION, GGML_TYPE_F16, GGML_TYPE_F32, GGML_TYPE_I32,
                   GGML_TYPE_I64, Context)

# one layer at Qwen2-VL's head shape (128 channels, sections 16 / 24 / 24), narrow everywhere else
TINY = dict(arch="qwen2vl", n_embd=512, n_layer=1, n_head=4, n_head_kv=2, head_dim=128, n_ff=512, n_vocab=256, rms_eps=1e-6, rope_base=1e6, n_ctx_orig=32768,
            rope_sections=(16, 24, 24, 0))


class Model(qwen3.Model):
    def __init__(self, be, cfg, types, n_ctx=512, seed=1234, flash_attn=True, mrope=True):
        super().__init__(be, cfg, types, n_ctx=n_ctx, seed=seed, flash_attn=flash_attn, host_copy=True)
        self.mrope = mrope
        H, HK, D = cfg["n_head"], cfg["n_head_kv"], cfg["head_dim"]
        self.bctx = Context(be)
        self.biases = [dict(bq=self.bctx.new_tensor(GGML_TYPE_F32, H * D), bk=self.bctx.new_tensor(GGML_TYPE_F32, HK * D), bv=self.bctx.new_tensor(GGML_TYPE_F32, HK * D))
                       for _ in self.layers]
        self.bctx.alloc(usage=GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
        rng = np.random.default_rng(seed + 1)
        for il, B in enumerate(self.biases):
            for name, T in B.items():
                b = (0.5 * rng.standard_normal(T.ne[0])).astype(np.float32)
                be.tensor_set(T, b)
                self.host[(il, name)] = b

    def build(self, n_tokens, n_kv, observe_rope=False, tap_attn=False):
        """one ubatch (llm_build_qwen2vl).  inp_pos: i32 [4 * n_tokens] (mrope) or [n_tokens].  observe_rope: the two ROPE nodes of layer 0 (g.rope_q, g.rope_k)
        and the biased projections they rotate (g.pre_q, g.pre_k) are graph outputs.  tap_attn: a SCALE(., 1.0) reader of layer 0's attention rows is appended to
        the roots as g.attn_tap (as qwen3.Model's tap_attn="rows": the rows stay materialised, the q / k / v stage stays inside the attention launch)"""
        c, be = self.cfg, self.be
        E, H, HK, D = c["n_embd"], c["n_head"], c["n_head_kv"], c["head_dim"]
        g = Context(be)
        roots = []
        I = dict(
            inp_embd=g.new_tensor(GGML_TYPE_F32, E, n_tokens), inp_pos=g.new_tensor(GGML_TYPE_I32, (4 if self.mrope else 1) * n_tokens),
            kq_mask=g.new_tensor(GGML_TYPE_F16 if self.fa else GGML_TYPE_F32, n_kv, (n_tokens + 63) // 64 * 64),
            k_idxs=g.new_tensor(GGML_TYPE_I64, n_tokens), v_idxs=g.new_tensor(GGML_TYPE_I64, n_tokens * (HK * D if self.v_trans else 1)),
        )
        kq_scale = 1.0 / math.sqrt(D)
        rope = dict(n_dims=D, n_ctx_orig=c["n_ctx_orig"], freq_base=c["rope_base"], freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0)

        def rotate(x):
            if self.mrope:
                return g.rope_multi(x, I["inp_pos"], None, sections=c["rope_sections"], mode=GGML_ROPE_TYPE_MROPE, **rope)
            return g.rope_ext(x, I["inp_pos"], None, mode=GGML_ROPE_TYPE_NEOX, **rope)
        f16 = 2
        inpL = I["inp_embd"]
        for il, (L, B) in enumerate(zip(self.layers, self.biases)):
            inpSA = inpL
            cur = g.mul(g.rms_norm(inpL, c["rms_eps"]), self._w(g, L["attn_norm"]))
            Q = g.add(g.mul_mat(self._w(g, L["attn_q"]), cur), self._w(g, B["bq"]))
            K = g.add(g.mul_mat(self._w(g, L["attn_k"]), cur), self._w(g, B["bk"]))
            V = g.add(g.mul_mat(self._w(g, L["attn_v"]), cur), self._w(g, B["bv"]))
            if observe_rope and il == 0:
                g.pre_q, g.pre_k = Q, K
            Q = g.reshape(Q, D, H, n_tokens)
            K = g.reshape(K, D, HK, n_tokens)
            V = g.reshape(V, D, HK, n_tokens)
            Q = rotate(Q)
            K = rotate(K)
            if observe_rope and il == 0:
                g.rope_q, g.rope_k = Q, K
                for t in (g.pre_q, g.pre_k, Q, K):
                    t.t.flags |= 2                                     # GGML_TENSOR_FLAG_OUTPUT
            kc, vc = self._w(g, L["k_cache"]), self._w(g, L["v_cache"])
            roots += [Q, K, V]
            roots.append(g.set_rows(kc, g.view_2d(K, HK * D, n_tokens, K.nb[2], 0), I["k_idxs"]))
            if self.v_trans:
                roots.append(g.set_rows(g.reshape(vc, 1, HK * D * self.n_ctx), g.reshape(g.reshape(V, HK * D, n_tokens), 1, HK * D * n_tokens), I["v_idxs"]))
            else:
                roots.append(g.set_rows(vc, g.view_2d(V, HK * D, n_tokens, V.nb[2], 0), I["v_idxs"]))
            k = g.view_4d(kc, D, HK, n_kv, 1, D * f16, HK * D * f16, HK * D * f16 * self.n_ctx, 0)
            if self.v_trans:
                v = g.view_4d(vc, n_kv, HK, D, 1, self.n_ctx * D * f16, self.n_ctx * f16, self.n_ctx * HK * D * f16, 0)
            else:
                v = g.view_4d(vc, D, HK, n_kv, 1, D * f16, HK * D * f16, HK * D * f16 * self.n_ctx, 0)
            q = g.permute(Q, 0, 2, 1, 3)
            k = g.permute(k, 0, 2, 1, 3)
            v = g.permute(v, 0, 2, 1, 3)
            if self.fa:
                cur = g.reshape(g.flash_attn_ext(q, k, v, I["kq_mask"], kq_scale), H * D, n_tokens)
            else:
                kqs = g.soft_max_ext(g.mul_mat(k, q), I["kq_mask"], kq_scale, 0.0)
                kqv = g.mul_mat(v if self.v_trans else g.cont(g.transpose(v)), kqs)
                cur = g.cont(g.permute(kqv, 0, 2, 1, 3), H * D, n_tokens)
            if tap_attn and il == 0:
                g.attn_tap = g.scale(cur, 1.0)
            cur = g.mul_mat(self._w(g, L["attn_output"]), cur)
            ffn_inp = g.add(cur, inpSA)
            cur = g.mul(g.rms_norm(ffn_inp, c["rms_eps"]), self._w(g, L["ffn_norm"]))
            up = g.mul_mat(self._w(g, L["ffn_up"]), cur)
            gate = g.mul_mat(self._w(g, L["ffn_gate"]), cur)
            cur = g.mul_mat(self._w(g, L["ffn_down"]), g.swiglu_split(gate, up))
            inpL = g.add(cur, ffn_inp)
        cur = g.mul(g.rms_norm(inpL, c["rms_eps"]), self._w(g, self.output_norm))
        if tap_attn:
            roots.append(g.attn_tap)
        logits = g.mul_mat(self._w(g, self.output), cur)
        roots.append(logits)
        g.roots = roots
        g.alloc()
        return g, I, logits

    def set_inputs_mrope(self, I, embd, pos4, cell0, n_kv):
        """tokens at cache cells cell0 .. cell0 + n - 1 (causal over the cells); pos4 [4, n] i32 -- with mrope=False row 0 alone is used"""
        be = self.be
        n = embd.shape[0]
        be.tensor_set(I["inp_embd"], embd.astype(np.float32))
        pos4 = np.ascontiguousarray(pos4, np.int32)
        be.tensor_set(I["inp_pos"], pos4 if self.mrope else np.ascontiguousarray(pos4[0]))
        cells = np.arange(cell0, cell0 + n, dtype=np.int64)
        be.tensor_set(I["k_idxs"], cells)
        if self.v_trans:
            nv = self.cfg["n_head_kv"] * self.cfg["head_dim"]
            be.tensor_set(I["v_idxs"], (np.arange(nv, dtype=np.int64)[None, :] * self.n_ctx + cells[:, None]).ravel())
        else:
            be.tensor_set(I["v_idxs"], cells)
        m = np.full((I["kq_mask"].ne[1], n_kv), -np.inf, dtype=np.float32)
        for i in range(n):
            m[i, : cell0 + i + 1] = 0.0
        be.tensor_set(I["kq_mask"], m.astype(np.float16) if self.fa else m)


def vit_attention(g, x, pos, W, n_head, freq_base=10000.0):
    """x [n_embd, n_patches] f32, pos i32 [4 * n_patches], W: dict of leaf tensors q_w / k_w / v_w [n_embd, n_embd] and q_b / k_b / v_b [n_embd].
    -> the attention rows [n_embd, n_patches] (the last arithmetic op: MUL_MAT(v, soft-max); PERMUTE + CONT lay them out for the output projection)"""
    E, N = x.ne[0], x.ne[1]
    D = E // n_head
    sections = (D // 4,) * 4
    rope = dict(n_dims=D // 2, sections=sections, mode=GGML_ROPE_TYPE_VISION, n_ctx_orig=32768, freq_base=freq_base, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0,
                beta_fast=32.0, beta_slow=1.0)
    Q = g.reshape(g.add(g.mul_mat(W["q_w"], x), W["q_b"]), D, n_head, N)
    K = g.reshape(g.add(g.mul_mat(W["k_w"], x), W["k_b"]), D, n_head, N)
    V = g.reshape(g.add(g.mul_mat(W["v_w"], x), W["v_b"]), D, n_head, N)
    Q = g.rope_multi(Q, pos, None, **rope)
    K = g.rope_multi(K, pos, None, **rope)
    g.vit_q, g.vit_k = Q, K
    q = g.permute(Q, 0, 2, 1, 3)
    k = g.permute(K, 0, 2, 1, 3)
    v = g.cont(g.permute(V, 1, 2, 0, 3))                              # [N, D, n_head]: build_attn's v for the soft-max path
    kq = g.soft_max_ext(g.mul_mat(k, q), None, 1.0 / math.sqrt(D), 0.0)
    kqv = g.mul_mat(v, kq)
    return g.cont(g.permute(kqv, 0, 2, 1, 3), E, N)
