"""Host-side mirror of the reference's RWKV layers (llm_build_rwkv6_base::build_rwkv6_time_mix / build_rwkv6_channel_mix, llm_build_rwkv7_base::build_rwkv7_time_mix /
build_rwkv7_channel_mix and the per-layer bodies of llm_build_rwkv6 / llm_build_rwkv7, reference src/llama-model.cpp:15265-15560 and 15661-15905) and of the token-shift
plumbing they go through (build_rwkv_token_shift_load / _store, reference src/llama-graph.cpp:1835-1874; build_rs is mamba.py's), built with the ctypes graph builder of
ggml.py.

It emits the node sequence graph_compute receives from libllama for one ubatch of n_seqs equal-length sequences: the token-shift rows read through build_rs, the two
norms, x_prev (the shift row in front of the norm's first n_seq_tokens - 1 tokens), the time mix -- the low-rank lerp (fused or five separate weights), the decay, the
wkv-state rows read through build_rs, RWKV_WKV6 (or, without time_mix_first, GATED_LINEAR_ATTN with k * (1 - w), a sigmoid gate and no group norm: is_qrwkv), resp. for
RWKV7 the L2_NORM of kk, RWKV_WKV7 on (-kk, kk * a), the value residual from the first layer and the optional gate --, the wkv-state and token-shift write-backs and the
channel mix.  No arithmetic is done here.
"""
import numpy as np

from .ggml import GGML_BACKEND_BUFFER_USAGE_WEIGHTS, GGML_TYPE_F32, GGML_TYPE_I32, UNARY, Context
from .mamba import build_rs
from .qwen3 import random_blocks

NORM_EPS = 1e-5
# the shapes of tools/make_synth_rwkv_gguf.py: n_embd 256, 4 heads of 64
TINY_RWKV6 = dict(arch="rwkv6", n_embd=256, head_size=64, n_ff=512, time_mix_extra=32, time_decay_extra=64, fused=True, qrwkv=False)
TINY_RWKV7 = dict(arch="rwkv7", n_embd=256, head_size=64, n_ff=512, lora_decay=32, lora_a=32, lora_v=16, lora_g=64, gating=True, first=True)


def n_embd_r(hp):
    """llama_hparams::n_embd_r for RWKV: token_shift_count (2) rows of n_embd"""
    return 2 * hp["n_embd"]


def n_embd_s(hp):
    """llama_hparams::n_embd_s for RWKV: n_embd * wkv_head_size"""
    return hp["n_embd"] * hp["head_size"]


def _norm(g, x, w, b):
    """build_norm(LLM_NORM)"""
    return g.add(g.mul(g.norm(x, NORM_EPS), w), b)


def _wkv_store(g, wkv_output, s_all, rs, hp, n_tokens, n_seqs, roots):
    """the output part of a WKV result, and the copy of its state part onto the cache rows from rs["head"]"""
    E, S = hp["n_embd"], hp["head_size"]
    cur = g.view_1d(wkv_output, E * n_tokens, 0)
    state = g.view_1d(wkv_output, E * S * n_seqs, E * n_tokens * 4)
    store = g.cpy(state, g.view_1d(s_all, n_embd_s(hp) * n_seqs, n_embd_s(hp) * rs["head"] * 4))
    roots.append(store)
    return cur, store


def _group_norm(g, cur, L, E, H, n_tokens):
    """"group norm with head_count groups": NORM over {E / H, H, n_tokens}, then time_mix_ln / ln_b"""
    cur = g.norm(g.reshape(cur, E // H, H, n_tokens), 64e-5)
    cur = g.reshape(cur, E, n_tokens)
    return g.add(g.mul(cur, L["time_mix_ln"]), L["time_mix_ln_b"])


def build_rwkv6_time_mix(g, cur, x_prev, L, s_all, rs, hp, n_seq_tokens, n_seqs, roots, N):
    """build_rwkv6_time_mix.  cur, x_prev {n_embd, n_seq_tokens, n_seqs}; L without "time_mix_first": is_qrwkv -> {n_embd, n_seq_tokens, n_seqs}"""
    E, S = hp["n_embd"], hp["head_size"]
    H, n_tokens = E // S, n_seq_tokens * n_seqs
    qrwkv = L.get("time_mix_first") is None
    sx = g.sub(x_prev, cur)
    sx = g.reshape(sx, E, n_tokens)
    cur = g.reshape(cur, E, n_tokens)
    xxx = g.add(g.mul(sx, L["time_mix_lerp_x"]), cur)
    w1, w2 = L["time_mix_w1"], L["time_mix_w2"]
    xxx = g.reshape(g.unary(g.mul_mat(w1, xxx), UNARY.TANH), w1.ne[1] // 5, 1, 5, n_tokens)
    xxx = g.cont(g.permute(xxx, 0, 1, 3, 2))
    xxx = g.mul_mat(g.reshape(w2, w2.ne[0], w2.ne[1], 1, 5), xxx)
    cut = lambda t, i: g.view_2d(t, E, n_tokens, t.nb[1], E * n_tokens * i * 4)
    if L.get("time_mix_lerp_fused") is not None:
        sx = g.reshape(sx, E, 1, n_tokens)
        cur = g.reshape(cur, E, 1, n_tokens)
        xxx = g.add(g.mul(g.add(xxx, L["time_mix_lerp_fused"]), sx), cur)
        xw, xk, xv, xr, xg = (cut(xxx, i) for i in range(5))
    else:                                                                                  # "for backward compatibility"
        xw, xk, xv, xr, xg = (g.add(g.mul(g.add(cut(xxx, i), L["time_mix_lerp_" + n]), sx), cur) for i, n in enumerate("wkvrg"))
    r = g.mul_mat(L["time_mix_receptance"], xr)
    k = g.mul_mat(L["time_mix_key"], xk)
    v = g.mul_mat(L["time_mix_value"], xv)
    gate = g.unary(g.mul_mat(L["time_mix_gate"], xg), UNARY.SIGMOID if qrwkv else UNARY.SILU)
    N.update(xr=xr, r=r, k=k, v=v, gate=gate)
    k, v, r = (g.reshape(t, S, H, n_tokens) for t in (k, v, r))
    w = g.mul_mat(L["time_mix_decay_w2"], g.unary(g.mul_mat(L["time_mix_decay_w1"], xw), UNARY.TANH))
    w = g.add(w, L["time_mix_decay"])
    w = g.unary(g.unary(g.unary(w, UNARY.EXP), UNARY.NEG), UNARY.EXP)
    w = g.reshape(w, S, H, n_tokens)
    N["w"] = w
    if qrwkv:
        k = g.sub(k, g.mul(k, w))                                                          # k * (1 - w)
    state = build_rs(g, s_all, rs, n_embd_s(hp), n_seqs, roots)
    if qrwkv:
        out = g.gated_linear_attn(k, v, r, w, state, float(S) ** -0.5)
    else:
        out = g.rwkv_wkv6(k, v, r, L["time_mix_first"], w, state)
    N["wkv"] = out
    cur, N["wkv_store"] = _wkv_store(g, out, s_all, rs, hp, n_tokens, n_seqs, roots)
    cur = g.reshape(cur, E, n_tokens) if qrwkv else _group_norm(g, cur, L, E, H, n_tokens)
    N["normed"] = cur
    N["gated"] = g.mul(cur, gate)
    cur = g.mul_mat(L["time_mix_output"], N["gated"])
    return g.reshape(cur, E, n_seq_tokens, n_seqs)


def build_rwkv6_channel_mix(g, cur, x_prev, L):
    """build_rwkv6_channel_mix (LLM_ARCH_RWKV6)"""
    sx = g.sub(x_prev, cur)
    xk = g.add(g.mul(sx, L["channel_mix_lerp_k"]), cur)
    xr = g.add(g.mul(sx, L["channel_mix_lerp_r"]), cur)
    r = g.unary(g.mul_mat(L["channel_mix_receptance"], xr), UNARY.SIGMOID)
    k = g.sqr(g.unary(g.mul_mat(L["channel_mix_key"], xk), UNARY.RELU))
    return g.mul(r, g.mul_mat(L["channel_mix_value"], k))


def build_rwkv7_time_mix(g, cur, x_prev, L, s_all, rs, hp, n_seq_tokens, n_seqs, roots, N, first_layer_value=None):
    """build_rwkv7_time_mix.  first_layer_value None: this is the first layer (its v is returned for the later ones) -> ({n_embd, n_seq_tokens, n_seqs}, first_layer_value)"""
    E, S = hp["n_embd"], hp["head_size"]
    H, n_tokens = E // S, n_seq_tokens * n_seqs
    gating = L.get("time_mix_g1") is not None and L.get("time_mix_g2") is not None
    sx = g.sub(x_prev, cur)
    sx = g.repeat_4d(sx, E, n_seq_tokens, n_seqs, 6 if gating else 5)
    xxx = g.add(g.mul(sx, L["time_mix_lerp_fused"]), cur)
    cut = lambda i: g.view_2d(xxx, E, n_tokens, xxx.nb[1], E * n_tokens * i * 4)
    xr, xw, xk, xv, xa = (cut(i) for i in range(5))
    xg = cut(5) if gating else None
    r = g.mul_mat(L["time_mix_receptance"], xr)
    w = g.add(g.mul_mat(L["time_mix_w2"], g.unary(g.mul_mat(L["time_mix_w1"], xw), UNARY.TANH)), L["time_mix_w0"])
    w = g.unary(g.scale(g.unary(w, UNARY.SIGMOID), -0.606531), UNARY.EXP)
    k = g.mul_mat(L["time_mix_key"], xk)
    v = g.mul_mat(L["time_mix_value"], xv)
    if first_layer_value is None:
        first_layer_value = v
    else:                                                                                  # "Add the first layer value as a residual connection."
        mix = g.unary(g.add(g.mul_mat(L["time_mix_v2"], g.mul_mat(L["time_mix_v1"], xv)), L["time_mix_v0"]), UNARY.SIGMOID)
        v = g.add(v, g.mul(g.sub(first_layer_value, v), mix))
    gate = g.mul_mat(L["time_mix_g2"], g.unary(g.mul_mat(L["time_mix_g1"], xg), UNARY.SIGMOID)) if gating else None
    a = g.unary(g.add(g.mul_mat(L["time_mix_a2"], g.mul_mat(L["time_mix_a1"], xa)), L["time_mix_a0"]), UNARY.SIGMOID)
    kk = g.reshape(g.mul(k, L["time_mix_k_k"]), S, H, n_tokens)
    kk = g.l2_norm(kk, 1e-12)
    N["l2_norm"] = kk
    ka = g.mul(k, L["time_mix_k_a"])
    k = g.add(k, g.sub(g.mul(a, ka), ka))
    r, w, k, v, a = (g.reshape(t, S, H, n_tokens) for t in (r, w, k, v, a))
    state = build_rs(g, s_all, rs, n_embd_s(hp), n_seqs, roots)
    out = g.rwkv_wkv7(r, w, k, v, g.unary(kk, UNARY.NEG), g.mul(kk, a), state)
    N["wkv"] = out
    cur, N["wkv_store"] = _wkv_store(g, out, s_all, rs, hp, n_tokens, n_seqs, roots)
    if L.get("time_mix_ln") is not None and L.get("time_mix_ln_b") is not None:
        cur = _group_norm(g, cur, L, E, H, n_tokens)
    else:
        cur = g.reshape(cur, E, n_tokens)
    rk = g.sum_rows(g.mul(g.mul(k, r), g.reshape(L["time_mix_r_k"], S, H)))
    cur = g.add(cur, g.reshape(g.mul(v, rk), E, n_tokens))
    if gating:
        cur = g.mul(cur, gate)
    cur = g.mul_mat(L["time_mix_output"], cur)
    return g.reshape(cur, E, n_seq_tokens, n_seqs), first_layer_value


def build_rwkv7_channel_mix(g, cur, x_prev, L):
    """build_rwkv7_channel_mix (LLM_ARCH_RWKV7)"""
    sx = g.sub(x_prev, cur)
    xk = g.add(g.mul(sx, L["channel_mix_lerp_k"]), cur)
    k = g.sqr(g.unary(g.mul_mat(L["channel_mix_key"], xk), UNARY.RELU))
    return g.mul_mat(L["channel_mix_value"], k)


def build_layer(g, inpL, L, r_all, s_all, rs, hp, n_seq_tokens, n_seqs, roots, first_layer_value=None):
    """one iteration of the layer loop of llm_build_rwkv6 / llm_build_rwkv7: token-shift load, attn_norm, x_prev, time mix, residual, attn_norm_2, x_prev, token-shift
    store, channel mix, residual.  inpL {n_embd, n_tokens} -> ({n_embd, n_tokens}, named nodes, first_layer_value)"""
    E, n_tokens = hp["n_embd"], n_seq_tokens * n_seqs
    N = {}
    inpL = g.reshape(inpL, E, n_seq_tokens, n_seqs)
    token_shift = g.reshape(build_rs(g, r_all, rs, n_embd_r(hp), n_seqs, roots), E, 2, n_seqs)        # build_rwkv_token_shift_load
    att_shift = g.view_3d(token_shift, E, 1, n_seqs, token_shift.nb[1], token_shift.nb[2], 0)
    ffn_shift = g.view_3d(token_shift, E, 1, n_seqs, token_shift.nb[1], token_shift.nb[2], E * 4)
    att_norm = _norm(g, inpL, L["attn_norm"], L["attn_norm_b"])
    x_prev = g.concat(att_shift, g.view_3d(att_norm, E, n_seq_tokens - 1, n_seqs, att_norm.nb[1], att_norm.nb[2], 0), 1)
    if hp["arch"] == "rwkv7":
        cur, first_layer_value = build_rwkv7_time_mix(g, att_norm, x_prev, L, s_all, rs, hp, n_seq_tokens, n_seqs, roots, N, first_layer_value)
    else:
        cur = build_rwkv6_time_mix(g, att_norm, x_prev, L, s_all, rs, hp, n_seq_tokens, n_seqs, roots, N)
    N["time_mix"] = cur
    ffn_inp = g.add(cur, inpL)
    ffn_norm = _norm(g, ffn_inp, L["attn_norm_2"], L["attn_norm_2_b"])
    x_prev = g.concat(ffn_shift, g.view_3d(ffn_norm, E, n_seq_tokens - 1, n_seqs, ffn_norm.nb[1], ffn_norm.nb[2], 0), 1)
    token_shift = g.concat(g.view_3d(att_norm, E, 1, n_seqs, att_norm.nb[1], att_norm.nb[2], (n_seq_tokens - 1) * E * 4),
                           g.view_3d(ffn_norm, E, 1, n_seqs, ffn_norm.nb[1], ffn_norm.nb[2], (n_seq_tokens - 1) * E * 4), 1)
    N["shift_store"] = g.cpy(g.view_1d(token_shift, E * n_seqs * 2, 0), g.view_1d(r_all, n_embd_r(hp) * n_seqs, n_embd_r(hp) * rs["head"] * 4))      # build_rwkv_token_shift_store
    roots.append(N["shift_store"])
    ffn_inp, ffn_norm, x_prev = (g.reshape(t, E, n_tokens) for t in (ffn_inp, ffn_norm, x_prev))
    cur = (build_rwkv7_channel_mix if hp["arch"] == "rwkv7" else build_rwkv6_channel_mix)(g, ffn_norm, x_prev, L)
    N["channel_mix"] = cur
    cur = g.add(cur, ffn_inp)
    N["out"] = cur
    return cur, N, first_layer_value


def layer_shapes(hp, big=GGML_TYPE_F32, out=GGML_TYPE_F32):
    """name -> (type, *ne) of one layer's weights, as the reference loader creates them (llama-model.cpp:5100-5161 / 5215-5286); `big` / `out`: the types of the n_embd-wide
    projections (time_mix_output and channel_mix_value take `out`)"""
    E, S, FF = hp["n_embd"], hp["head_size"], hp["n_ff"]
    H, F = E // S, GGML_TYPE_F32
    sh = dict(attn_norm=(F, E), attn_norm_b=(F, E), attn_norm_2=(F, E), attn_norm_2_b=(F, E))
    if hp["arch"] == "rwkv7":
        n_lerp = 6 if hp["gating"] else 5
        sh.update(time_mix_lerp_fused=(F, E, 1, 1, n_lerp), time_mix_w0=(F, E), time_mix_w1=(F, E, hp["lora_decay"]), time_mix_w2=(F, hp["lora_decay"], E),
                  time_mix_a0=(F, E), time_mix_a1=(F, E, hp["lora_a"]), time_mix_a2=(F, hp["lora_a"], E), time_mix_k_k=(F, E), time_mix_k_a=(F, E), time_mix_r_k=(F, E),
                  time_mix_key=(big, E, E), time_mix_value=(big, E, E), time_mix_receptance=(big, E, E), time_mix_ln=(F, E), time_mix_ln_b=(F, E), time_mix_output=(out, E, E),
                  channel_mix_lerp_k=(F, E, 1, 1), channel_mix_key=(big, E, FF), channel_mix_value=(out, FF, E))
        if not hp["first"]:
            sh.update(time_mix_v0=(F, E), time_mix_v1=(F, E, hp["lora_v"]), time_mix_v2=(F, hp["lora_v"], E))
        if hp["gating"]:
            sh.update(time_mix_g1=(F, E, hp["lora_g"]), time_mix_g2=(F, hp["lora_g"], E))
        return sh
    TM, TD = hp["time_mix_extra"], hp["time_decay_extra"]
    sh.update(time_mix_w1=(F, E, TM * 5), time_mix_w2=(F, TM, E, 5), time_mix_lerp_x=(F, E, 1, 1), time_mix_decay=(F, E), time_mix_decay_w1=(F, E, TD),
              time_mix_decay_w2=(F, TD, E), time_mix_key=(big, E, E), time_mix_value=(big, E, E), time_mix_receptance=(big, E, E), time_mix_gate=(big, E, E),
              time_mix_output=(out, E, E), channel_mix_lerp_k=(F, E, 1, 1), channel_mix_lerp_r=(F, E, 1, 1), channel_mix_key=(big, E, FF), channel_mix_value=(out, FF, E),
              channel_mix_receptance=(big, E, E))
    if hp["fused"]:
        sh["time_mix_lerp_fused"] = (F, E, 1, 1, 5)
    else:
        sh.update({"time_mix_lerp_" + n: (F, E, 1, 1) for n in "wkvrg"})
    if not hp["qrwkv"]:
        sh.update(time_mix_first=(F, S, H), time_mix_ln=(F, E), time_mix_ln_b=(F, E))
    return sh


def random_weights(hp, shapes, rs_size, seed):
    """seeded weights: projections ~ N(0, 1 / K), lerp weights in (0, 1), norm weights near 1, decays that keep the states bounded"""
    rng = np.random.default_rng(seed)
    W = {}
    for k, sh in shapes.items():
        ne = sh[1:]
        rows = int(np.prod(ne[1:])) if len(ne) > 1 else 1
        if sh[0] != GGML_TYPE_F32:
            W[k] = random_blocks(rng, sh[0], rows, ne[0], std=1.0 / np.sqrt(ne[0]))
        elif "lerp" in k:
            W[k] = rng.uniform(0.0, 1.0, (rows, ne[0])).astype(np.float32)
        elif k in ("attn_norm", "attn_norm_2", "time_mix_ln", "time_mix_k_k", "time_mix_k_a", "time_mix_r_k"):
            W[k] = rng.uniform(0.5, 1.5, (rows, ne[0])).astype(np.float32)
        elif k == "time_mix_decay":
            W[k] = rng.uniform(-4.0, -0.5, (rows, ne[0])).astype(np.float32)               # w = exp(-exp(.)) in (0.55, 0.98)
        elif k.endswith("_b") or k in ("time_mix_w0", "time_mix_a0", "time_mix_v0", "time_mix_first"):
            W[k] = (rng.standard_normal((rows, ne[0])) * 0.3).astype(np.float32)
        else:
            W[k] = (rng.standard_normal((rows, ne[0])) / np.sqrt(ne[0])).astype(np.float32)
    W["r_states"] = rng.standard_normal(n_embd_r(hp) * rs_size).astype(np.float32)
    W["s_states"] = (rng.standard_normal(n_embd_s(hp) * rs_size) * 0.5).astype(np.float32)
    return W


class RwkvLayer:
    """The weights and the two state caches (token shift, wkv) of one RWKV layer resident in a buffer, and the layer's graph for one ubatch (tests, tools)."""

    def __init__(self, be, hp, rs_size=4, seed=5, big=GGML_TYPE_F32, out=GGML_TYPE_F32, weights=None):
        self.be, self.hp, self.rs_size = be, hp, rs_size
        self.shapes = layer_shapes(hp, big, out)
        w = self.wctx = Context(be)
        self.T = {k: w.new_tensor(sh[0], *sh[1:]) for k, sh in self.shapes.items()}
        self.r_states = w.new_tensor(GGML_TYPE_F32, n_embd_r(hp) * rs_size)
        self.s_states = w.new_tensor(GGML_TYPE_F32, n_embd_s(hp) * rs_size)
        w.alloc(usage=GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
        self.weights = weights if weights is not None else random_weights(hp, self.shapes, rs_size, seed)
        for k in self.shapes:
            be.tensor_set(self.T[k], self.weights[k])
        be.tensor_set(self.r_states, self.weights["r_states"])
        be.tensor_set(self.s_states, self.weights["s_states"])

    def _w(self, g, real):
        T = g._new(real.type, real.ne, view_src=real, view_offs=0)
        for i in range(4):
            T.t.nb[i] = real.t.nb[i]
        return T

    def build(self, n_seq_tokens, n_seqs, n_rs, rs_head, rs_zero):
        """-> (graph context, input {n_embd, n_tokens}, s_copy input i32 {n_rs}, first-layer value input or None, named nodes)"""
        g = Context(self.be)
        hp = self.hp
        x = g.new_tensor(GGML_TYPE_F32, hp["n_embd"], n_seq_tokens * n_seqs)
        s_copy = g.new_tensor(GGML_TYPE_I32, n_rs)
        v_first = g.new_tensor(GGML_TYPE_F32, hp["n_embd"], n_seq_tokens * n_seqs) if hp["arch"] == "rwkv7" and not hp["first"] else None
        rs = dict(copy_main=g.view_1d(s_copy, n_seqs, 0), copy_extra=g.view_1d(s_copy, n_rs - n_seqs, n_seqs * 4), n_rs=n_rs, head=rs_head, size=self.rs_size, zero=rs_zero)
        L = {k: self._w(g, t) for k, t in self.T.items()}
        roots = []
        out, N, _ = build_layer(g, x, L, self._w(g, self.r_states), self._w(g, self.s_states), rs, hp, n_seq_tokens, n_seqs, roots, v_first)
        roots.append(out)
        g.roots = roots
        g.alloc()
        return g, x, s_copy, v_first, N
