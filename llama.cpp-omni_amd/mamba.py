"""Host-side mirror of the reference's recurrent layers (llm_graph_context_mamba::build_mamba_layer / build_mamba2_layer, reference
src/llama-model.cpp:11674-11943) and of the recurrent-state plumbing they go through (llm_graph_context::build_rs, reference
src/llama-graph.cpp:1760-1793), built with the ctypes graph builder of ggml.py.

It emits exactly the node sequence graph_compute receives from libllama for one ubatch of n_seqs equal-length sequences: the SCALE
that zeroes one state row (a zero-sized view when no row is to be cleared), the GET_ROWS on the conv states, the copy of the extra
states, the CONCAT of the conv state and the transposed projection, the conv-state write-back, SSM_CONV, bias, SiLU, the SSM_SCAN
that reads its state rows through ids, the ssm-state write-back, the skip, the gate, (Mamba-2) the grouped RMS norm and the
output projection.  No arithmetic is done here.
"""
import numpy as np

from .ggml import GGML_BACKEND_BUFFER_USAGE_WEIGHTS, GGML_TYPE_F32, GGML_TYPE_I32, GGML_TYPE_Q4_K, GGML_TYPE_Q6_K, UNARY, Context
from .qwen3 import random_blocks

# the shapes of tools/make_synth_mamba_gguf.py
TINY_MAMBA2 = dict(arch="mamba2", n_embd=256, d_inner=512, d_state=128, d_conv=4, dt_rank=8, n_group=2, eps=1e-5, dt_b_c_rms=False)
TINY_MAMBA = dict(arch="mamba", n_embd=256, d_inner=512, d_state=16, d_conv=4, dt_rank=16, n_group=1, eps=1e-5, dt_b_c_rms=False)


def n_embd_r(hp):
    """llama_hparams::n_embd_r: the conv state of one sequence"""
    return (hp["d_conv"] - 1) * (hp["d_inner"] + (2 * hp["n_group"] * hp["d_state"] if hp["arch"] == "mamba2" else 0))


def n_embd_s(hp):
    """llama_hparams::n_embd_s: the ssm state of one sequence"""
    return hp["d_state"] * hp["d_inner"]


def build_rs(g, s, rs, state_size, n_seqs, roots, get_state_rows=None):
    """llm_graph_context::build_rs.  s: the layer's state cache (1-D, rs["size"] rows of state_size); rs: dict(copy_main, copy_extra, n_rs,
    head, size, zero) -- the views of the s_copy input and what llama_memory_recurrent_context reports.  -> the state rows of the n_seqs sequences"""
    states = g.reshape(s, state_size, rs["size"])
    z = rs["zero"] >= 0
    state_zero = g.view_1d(states, state_size * z, rs["zero"] * states.nb[1] * z)      # "a no-op when the view is zero-sized"
    roots.append(g.scale_inplace(state_zero, 0.0))
    out = get_state_rows(g, states, rs["copy_main"]) if get_state_rows else g.get_rows(states, rs["copy_main"])
    roots.append(out)
    extra = g.get_rows(states, rs["copy_extra"])                                        # "states which won't be changed further (between n_seqs and n_rs)"
    roots.append(g.cpy(extra, g.view_1d(s, state_size * (rs["n_rs"] - n_seqs), (rs["head"] + n_seqs) * state_size * 4)))
    return out


def _rms(g, x, w, eps):
    """build_norm(LLM_NORM_RMS) without a bias; w None: the norm alone (a plain `mamba` file with ssm.dt_b_c_rms set carries no norm weights: FalconMamba)"""
    y = g.rms_norm(x, eps)
    return g.mul(y, w) if w is not None else y


def build_mamba_layer(g, cur, L, conv_states_all, ssm_states_all, rs, hp, n_seq_tokens, n_seqs, roots):
    """build_mamba_layer.  cur [n_embd, n_tokens]; L: the layer's weights (ssm_in, ssm_conv1d, ssm_conv1d_b, ssm_x, ssm_dt, ssm_dt_b, ssm_a, ssm_d, ssm_out and,
    with hp["dt_b_c_rms"], ssm_dt_norm / ssm_b_norm / ssm_c_norm).  -> ([n_embd, n_tokens], named nodes)"""
    d_conv, d_inner, d_state, dt_rank = hp["d_conv"], hp["d_inner"], hp["d_state"], hp["dt_rank"]
    n_head, head_dim = d_inner, 1
    N = {}
    conv = build_rs(g, conv_states_all, rs, n_embd_r(hp), n_seqs, roots)
    conv = g.reshape(conv, d_conv - 1, d_inner, n_seqs)
    cur = g.reshape(cur, cur.ne[0], n_seq_tokens, n_seqs)
    xz = g.mul_mat(L["ssm_in"], cur)                                                   # [2 * d_inner, n_seq_tokens, n_seqs]
    x = g.view_3d(xz, d_inner, xz.ne[1], xz.ne[2], xz.nb[1], xz.nb[2], 0)
    z = g.view_3d(xz, d_inner, xz.ne[1], xz.ne[2], xz.nb[1], xz.nb[2], d_inner * 4)
    conv_x = g.concat(conv, g.transpose(x), 0)                                         # [d_conv - 1 + n_seq_tokens, d_inner, n_seqs]
    last_conv = g.view_3d(conv_x, d_conv - 1, d_inner, n_seqs, conv_x.nb[1], conv_x.nb[2], n_seq_tokens * conv_x.nb[0])
    N["conv_store"] = g.cpy(last_conv, g.view_1d(conv_states_all, (d_conv - 1) * d_inner * n_seqs, rs["head"] * (d_conv - 1) * d_inner * 4))
    roots.append(N["conv_store"])
    x = g.ssm_conv(conv_x, L["ssm_conv1d"])
    N["ssm_conv"] = x
    x = g.add(x, L["ssm_conv1d_b"])
    x = g.unary(x, UNARY.SILU)
    x_db = g.mul_mat(L["ssm_x"], x)                                                    # [dt_rank + 2 * d_state, n_seq_tokens, n_seqs]
    dt = g.view_3d(x_db, dt_rank, n_seq_tokens, n_seqs, x_db.nb[1], x_db.nb[2], 0)
    B = g.view_4d(x_db, d_state, 1, n_seq_tokens, n_seqs, d_state * x_db.nb[0], x_db.nb[1], x_db.nb[2], 4 * dt_rank)
    C_ = g.view_4d(x_db, d_state, 1, n_seq_tokens, n_seqs, d_state * x_db.nb[0], x_db.nb[1], x_db.nb[2], 4 * (dt_rank + d_state))
    if hp.get("dt_b_c_rms"):                                                           # FalconMamba, Jamba
        dt = _rms(g, dt, L.get("ssm_dt_norm"), hp["eps"])
        B = _rms(g, B, L.get("ssm_b_norm"), hp["eps"])
        C_ = _rms(g, C_, L.get("ssm_c_norm"), hp["eps"])
    dt = g.mul_mat(L["ssm_dt"], dt)
    dt = g.add(dt, L["ssm_dt_b"])
    cur = x
    x = g.reshape(x, head_dim, n_head, n_seq_tokens, n_seqs)

    def get_ssm_rows(g_, states, ids):
        ssm = g_.reshape(states, d_state, head_dim, n_head, rs["size"])
        return g_.ssm_scan(ssm, x, dt, L["ssm_a"], B, C_, ids)

    y_ssm = build_rs(g, ssm_states_all, rs, n_embd_s(hp), n_seqs, roots, get_ssm_rows)
    N["ssm_scan"] = y_ssm
    N["ssm_store"] = g.cpy(g.view_1d(y_ssm, d_state * d_inner * n_seqs, x.nb[3] * x.ne[3]),
                           g.view_1d(ssm_states_all, d_state * d_inner * n_seqs, rs["head"] * d_state * d_inner * 4))
    roots.append(N["ssm_store"])
    y = g.view_3d(y_ssm, d_inner, n_seq_tokens, n_seqs, x.nb[2], x.nb[3], 0)
    y = g.add(y, g.mul(cur, L["ssm_d"]))
    y = g.swiglu_split(g.cont(z), y)
    cur = g.mul_mat(L["ssm_out"], y)
    cur = g.reshape(cur, cur.ne[0], n_seq_tokens * n_seqs)
    N["out"] = cur
    return cur, N


def build_mamba2_layer(g, cur, L, conv_states_all, ssm_states_all, rs, hp, n_seq_tokens, n_seqs, roots):
    """build_mamba2_layer.  L: ssm_in, ssm_conv1d, ssm_conv1d_b, ssm_dt_b, ssm_a {1, n_head}, ssm_d {1, n_head}, ssm_norm {d_inner / n_group, n_group} (or None), ssm_out"""
    d_conv, d_inner, d_state, n_head, n_group = hp["d_conv"], hp["d_inner"], hp["d_state"], hp["dt_rank"], hp["n_group"]
    head_dim = d_inner // n_head
    d_xbc = d_inner + 2 * n_group * d_state
    N = {}
    conv = build_rs(g, conv_states_all, rs, n_embd_r(hp), n_seqs, roots)
    conv = g.reshape(conv, d_conv - 1, d_xbc, n_seqs)
    cur = g.reshape(cur, cur.ne[0], n_seq_tokens, n_seqs)
    zxBCdt = g.mul_mat(L["ssm_in"], cur)                                               # [2 * d_inner + 2 * n_group * d_state + n_head, n_seq_tokens, n_seqs]
    z = g.view_4d(zxBCdt, head_dim, n_head, n_seq_tokens, n_seqs, head_dim * zxBCdt.nb[0], zxBCdt.nb[1], zxBCdt.nb[2], 0)
    xBC = g.view_3d(zxBCdt, d_xbc, n_seq_tokens, n_seqs, zxBCdt.nb[1], zxBCdt.nb[2], d_inner * 4)
    dt = g.view_3d(zxBCdt, n_head, n_seq_tokens, n_seqs, zxBCdt.nb[1], zxBCdt.nb[2], (2 * d_inner + 2 * n_group * d_state) * 4)
    conv_x = g.concat(conv, g.transpose(xBC), 0)                                       # [d_conv - 1 + n_seq_tokens, d_xbc, n_seqs]
    last_conv = g.view_3d(conv_x, d_conv - 1, d_xbc, n_seqs, conv_x.nb[1], conv_x.nb[2], n_seq_tokens * conv_x.nb[0])
    N["conv_store"] = g.cpy(last_conv, g.view_1d(conv_states_all, (d_conv - 1) * d_xbc * n_seqs, rs["head"] * (d_conv - 1) * d_xbc * 4))
    roots.append(N["conv_store"])
    xBC = g.ssm_conv(conv_x, L["ssm_conv1d"])
    N["ssm_conv"] = xBC
    xBC = g.add(xBC, L["ssm_conv1d_b"])
    xBC = g.unary(xBC, UNARY.SILU)
    x = g.view_4d(xBC, head_dim, n_head, n_seq_tokens, n_seqs, head_dim * xBC.nb[0], xBC.nb[1], xBC.nb[2], 0)
    B = g.view_4d(xBC, d_state, n_group, n_seq_tokens, n_seqs, d_state * xBC.nb[0], xBC.nb[1], xBC.nb[2], d_inner * 4)
    C_ = g.view_4d(xBC, d_state, n_group, n_seq_tokens, n_seqs, d_state * xBC.nb[0], xBC.nb[1], xBC.nb[2], (d_inner + n_group * d_state) * 4)
    dt = g.add(g.cont(dt), L["ssm_dt_b"])

    def get_ssm_rows(g_, states, ids):
        ssm = g_.reshape(states, d_state, head_dim, n_head, rs["size"])
        return g_.ssm_scan(ssm, x, dt, L["ssm_a"], B, C_, ids)

    y_ssm = build_rs(g, ssm_states_all, rs, n_embd_s(hp), n_seqs, roots, get_ssm_rows)
    N["ssm_scan"] = y_ssm
    N["ssm_store"] = g.cpy(g.view_1d(y_ssm, d_state * d_inner * n_seqs, x.nelements() * x.nb[0]),
                           g.view_1d(ssm_states_all, d_state * d_inner * n_seqs, rs["head"] * d_state * d_inner * 4))
    roots.append(N["ssm_store"])
    y = g.view_4d(y_ssm, head_dim, n_head, n_seq_tokens, n_seqs, x.nb[1], n_head * x.nb[1], n_seq_tokens * n_head * x.nb[1], 0)
    y = g.add(y, g.mul(x, L["ssm_d"]))                                                 # mamba2_y_add_d
    y = g.swiglu_split(g.cont(z), y)
    if L.get("ssm_norm") is not None:                                                  # grouped RMS norm
        y = g.reshape(y, d_inner // n_group, n_group, n_seq_tokens, n_seqs)
        y = _rms(g, y, L["ssm_norm"], hp["eps"])
        N["ssm_norm"] = y
    y = g.reshape(y, d_inner, n_seq_tokens, n_seqs)
    cur = g.mul_mat(L["ssm_out"], y)
    cur = g.reshape(cur, cur.ne[0], n_seq_tokens * n_seqs)                              # mamba_out
    N["out"] = cur
    return cur, N


class MambaLayer:
    """The weights and the two state caches of one recurrent layer resident in a buffer, and the layer's graph for one ubatch (tests, tools)."""

    def __init__(self, be, hp=TINY_MAMBA2, rs_size=3, seed=5, in_type=GGML_TYPE_Q4_K, out_type=GGML_TYPE_Q6_K, x_type=GGML_TYPE_Q4_K, weights=None, std=0.05):
        self.be, self.hp, self.rs_size = be, hp, rs_size
        E, DI, DS, DC, R, G = hp["n_embd"], hp["d_inner"], hp["d_state"], hp["d_conv"], hp["dt_rank"], hp["n_group"]
        m2 = hp["arch"] == "mamba2"
        w = self.wctx = Context(be)
        T = {}
        if m2:
            d_xbc = DI + 2 * G * DS
            shapes = dict(ssm_in=(in_type, E, 2 * DI + 2 * G * DS + R), ssm_conv1d=(GGML_TYPE_F32, DC, d_xbc), ssm_conv1d_b=(GGML_TYPE_F32, d_xbc), ssm_dt_b=(GGML_TYPE_F32, R),
                          ssm_a=(GGML_TYPE_F32, 1, R), ssm_d=(GGML_TYPE_F32, 1, R), ssm_norm=(GGML_TYPE_F32, DI // G, G), ssm_out=(out_type, DI, E))
        else:
            shapes = dict(ssm_in=(in_type, E, 2 * DI), ssm_conv1d=(GGML_TYPE_F32, DC, DI), ssm_conv1d_b=(GGML_TYPE_F32, DI), ssm_x=(x_type, DI, R + 2 * DS),
                          ssm_dt=(GGML_TYPE_F32, R, DI), ssm_dt_b=(GGML_TYPE_F32, DI), ssm_a=(GGML_TYPE_F32, DS, DI), ssm_d=(GGML_TYPE_F32, DI), ssm_out=(out_type, DI, E))
            if hp.get("dt_b_c_rms"):
                shapes.update(ssm_dt_norm=(GGML_TYPE_F32, R), ssm_b_norm=(GGML_TYPE_F32, DS), ssm_c_norm=(GGML_TYPE_F32, DS))
        for k, sh in shapes.items():
            T[k] = w.new_tensor(sh[0], *sh[1:])
        self.conv_states = w.new_tensor(GGML_TYPE_F32, n_embd_r(hp) * rs_size)
        self.ssm_states = w.new_tensor(GGML_TYPE_F32, n_embd_s(hp) * rs_size)
        w.alloc(usage=GGML_BACKEND_BUFFER_USAGE_WEIGHTS)
        if weights is None:
            rng = np.random.default_rng(seed)
            weights = {}
            for k, sh in shapes.items():
                ne = sh[1:]
                rows = int(np.prod(ne[1:])) if len(ne) > 1 else 1
                if sh[0] != GGML_TYPE_F32:
                    weights[k] = random_blocks(rng, sh[0], rows, ne[0], std=std)
                elif k == "ssm_a":
                    weights[k] = -rng.uniform(0.05, 1.0, (rows, ne[0])).astype(np.float32)      # negative, as real files have it
                elif k in ("ssm_d", "ssm_norm", "ssm_dt_norm", "ssm_b_norm", "ssm_c_norm"):
                    weights[k] = rng.uniform(0.5, 1.5, (rows, ne[0])).astype(np.float32)
                elif k in ("ssm_dt", "ssm_in", "ssm_x", "ssm_out"):
                    weights[k] = (rng.standard_normal((rows, ne[0])) / np.sqrt(ne[0])).astype(np.float32)
                else:
                    weights[k] = (rng.standard_normal((rows, ne[0])) * 0.5).astype(np.float32)
            weights["conv_states"] = rng.standard_normal(n_embd_r(hp) * rs_size).astype(np.float32)
            weights["ssm_states"] = rng.standard_normal(n_embd_s(hp) * rs_size).astype(np.float32)
        self.weights, self.T = weights, T
        for k in shapes:
            be.tensor_set(T[k], weights[k])
        be.tensor_set(self.conv_states, weights["conv_states"])
        be.tensor_set(self.ssm_states, weights["ssm_states"])

    def _w(self, g, real):
        T = g._new(real.type, real.ne, view_src=real, view_offs=0)
        for i in range(4):
            T.t.nb[i] = real.t.nb[i]
        return T

    def build(self, n_seq_tokens, n_seqs, n_rs, rs_head, rs_zero):
        """-> (graph context, input [n_embd, n_tokens], s_copy input i32 [n_rs], named nodes); the graph's node order is ggml_build_forward_expand's over the layer's roots"""
        g = Context(self.be)
        x = g.new_tensor(GGML_TYPE_F32, self.hp["n_embd"], n_seq_tokens * n_seqs)
        s_copy = g.new_tensor(GGML_TYPE_I32, n_rs)
        rs = dict(copy_main=g.view_1d(s_copy, n_seqs, 0), copy_extra=g.view_1d(s_copy, n_rs - n_seqs, n_seqs * 4), n_rs=n_rs, head=rs_head, size=self.rs_size, zero=rs_zero)
        L = {k: self._w(g, t) for k, t in self.T.items()}
        roots = []
        fn = build_mamba2_layer if self.hp["arch"] == "mamba2" else build_mamba_layer
        out, N = fn(g, x, L, self._w(g, self.conv_states), self._w(g, self.ssm_states), rs, self.hp, n_seq_tokens, n_seqs, roots)
        roots.append(out)
        g.roots = roots
        g.alloc()
        return g, x, s_copy, N
