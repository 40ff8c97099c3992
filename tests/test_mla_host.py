"""Host side of the multi-head latent attention block (no GPU): llama.cpp-omni_amd/mla.py emits the node sequence and shapes of the reference's
llm_build_deepseek2 `is_mla` branch (src/llama-model.cpp:13560-13653) and of build_attn_mha's `v_mla` product (src/llama-graph.cpp:1349-1359), and the
block, run on the reference CPU backend (oracle/_ref), equals a NumPy float64 restatement written here.  Bar of the second test: NMSE < 5e-4, the
reference's own bar for FLASH_ATTN_EXT -- the reference rounds the activations of every F16 mat-mul to f16 and accumulates V in f16."""
import numpy as np

from conftest import nmse

F32, F16, I32, I64 = 0, 1, 26, 27


def _graph(pkg, hp, n_tokens, n_kv, n_ctx):
    from llama_cpp_omni_amd import mla
    g = pkg.Context(None)
    L = {k: g.new_tensor(F32 if len(ne) == 1 else F16, *ne) for k, ne in mla.weight_shapes(hp).items()}
    I = dict(inp_pos=g.new_tensor(I32, n_tokens), kq_mask=g.new_tensor(F16, n_kv, 64), k_idxs=g.new_tensor(I64, n_tokens), v_idxs=g.new_tensor(I64, n_tokens))
    kc = g.new_tensor(F16, hp["n_rot"] + hp["kv_lora_rank"], n_ctx)
    vc = g.new_tensor(F16, hp["kv_lora_rank"], n_ctx)
    x = g.new_tensor(F32, hp["n_embd"], n_tokens)
    roots = []
    out, N = mla.build_mla_attn(g, x, L, kc, vc, I, hp, n_tokens, n_kv, n_ctx, roots)
    roots.append(out)
    return g, roots, N, L, (kc, vc)


def test_mla_node_sequence_and_shapes(pkg):
    """the ops named at llama-model.cpp:13560-13653 in ggml_build_forward_expand's order over build_attn's roots (q_cur, k_cur, v_cur, the two stores, the output)"""
    from llama_cpp_omni_amd import mla
    OP = pkg.OP
    for q_lora in (0, 96):
        hp = dict(mla.TINY_MLA, q_lora_rank=q_lora)
        H, R, P, N_, V, E = hp["n_head"], hp["kv_lora_rank"], hp["n_rot"], hp["n_nope"], hp["n_v"], hp["n_embd"]
        nt, n_kv, n_ctx = 5, 32, 64
        g, roots, N, L, (kc, vc) = _graph(pkg, hp, nt, n_kv, n_ctx)
        ops = [n.t.op for n in g.graph_expand(roots).nodes]
        real = [o for o in ops if o not in (OP.RESHAPE, OP.VIEW, OP.TRANSPOSE, OP.PERMUTE)]
        q_ops = [OP.MUL_MAT, OP.RMS_NORM, OP.MUL, OP.MUL_MAT] if q_lora else [OP.MUL_MAT]
        want = (q_ops + [OP.ROPE,                                       # q ; q_pe
                         OP.MUL_MAT, OP.CONCAT,                         # q_nope_absorbed = wk_b . q_nope ; Qcur
                         OP.MUL_MAT, OP.ROPE, OP.RMS_NORM, OP.MUL, OP.CONCAT,      # kv_cmpr_pe ; k_pe ; kv_cmpr norm ; Kcur
                         OP.SET_ROWS, OP.SET_ROWS,                      # cpy_k, cpy_v
                         OP.FLASH_ATTN_EXT, OP.MUL_MAT, OP.CONT, OP.MUL_MAT])      # the attention ; wv_b ; cont ; wo
        assert real == want, real
        assert N["q_nope_absorbed"].ne == (R, nt, H, 1) and N["q_nope_absorbed"]._srcs[0] is L["wk_b"] and L["wk_b"].ne == (N_, R, H, 1)
        assert N["Qcur"].ne == (P + R, H, nt, 1) and N["Kcur"].ne == (P + R, 1, nt, 1) and N["Vcur"].ne == (R, 1, nt, 1)
        assert N["k_store"].t.view_src and N["k_store"].ne == (P + R, n_ctx, 1, 1) and N["v_store"].ne == (R, n_ctx, 1, 1)      # separate K and V caches
        fa = N["fattn"]
        q, k, v = fa._srcs[0], fa._srcs[1], fa._srcs[2]
        assert q.ne == (P + R, nt, H, 1) and k.ne == (P + R, n_kv, 1, 1) and v.ne == (R, n_kv, 1, 1)                             # MQA: one KV head, 576 / 512 at the model's sizes
        assert k.type == F16 and v.type == F16 and (P + R, R) == (576, 512)
        assert fa.ne == (R, H, nt, 1) and N["fattn_mla"].ne == (V, nt, H, 1) and N["fattn_mla"]._srcs[0] is L["wv_b"]
        assert N["out"].ne == (E, nt, 1, 1)


def _rope_norm(x, pos, base):
    """ggml RoPE mode 0 over the whole row: pairs (2i, 2i + 1), theta = pos * base^(-2i / n)"""
    n = x.shape[-1]
    th = pos[:, None] * base ** (-np.arange(0, n, 2) / n)
    c, s = np.cos(th), np.sin(th)
    while c.ndim < x.ndim:
        c, s = c[:, None], s[:, None]
    y = np.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    y[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return y


def _block_f64(hp, W, x, pos0, K, V):
    """x [nt, E]; K [n_ctx, 576] / V [n_ctx, 512] float64 caches, updated in place.  -> (attention rows [nt, H, R], block output [nt, E])"""
    H, R, P, N_, Vd = hp["n_head"], hp["kv_lora_rank"], hp["n_rot"], hp["n_nope"], hp["n_v"]
    nt = x.shape[0]
    pos = np.arange(pos0, pos0 + nt, dtype=np.float64)
    q = (x @ W["wq"].T).reshape(nt, H, N_ + P)
    q_nope, q_pe = q[..., :N_], _rope_norm(q[..., N_:], pos, hp["rope_base"])
    kvp = x @ W["wkv_a_mqa"].T
    kv, k_pe = kvp[:, :R], _rope_norm(kvp[:, R:], pos, hp["rope_base"])
    kv = kv / np.sqrt((kv ** 2).mean(-1, keepdims=True) + hp["eps"]) * W["attn_kv_a_norm"]
    q_abs = np.einsum("thn,hrn->thr", q_nope, W["wk_b"])                 # wk_b [H, R, N]
    Q = np.concatenate([q_pe, q_abs], -1)
    K[pos0:pos0 + nt] = np.concatenate([k_pe, kv], -1).astype(np.float16)
    V[pos0:pos0 + nt] = kv.astype(np.float16)
    rows = np.zeros((nt, H, R))
    for t in range(nt):
        n = pos0 + t + 1
        s = (Q[t].astype(np.float16).astype(np.float64) @ K[:n].T) / np.sqrt(N_ + P)
        p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
        rows[t] = p @ V[:n]
    y = np.einsum("thr,hvr->thv", rows, W["wv_b"]).reshape(nt, H * Vd)    # wv_b [H, V, R]
    return rows, y @ W["wo"].T


def test_mla_block_on_reference_backend_equals_float64(pkg, ref_be):
    from llama_cpp_omni_amd import mla
    hp, n_ctx = mla.TINY_MLA, 64
    blk = mla.MLABlock(ref_be, hp, n_ctx=n_ctx, seed=4)
    W = {k: np.asarray(v, np.float64) for k, v in blk.weights.items()}
    K, V = np.zeros((n_ctx, 576)), np.zeros((n_ctx, 512))
    rng = np.random.default_rng(6)
    pos0 = 0
    for nt, n_kv in [(33, 64), (1, 64)]:
        xv = rng.standard_normal((nt, hp["n_embd"])).astype(np.float32)
        g, I, N = blk.build(nt, n_kv)
        blk.set_inputs(I, xv, pos0, n_kv)
        ref_be.graph_compute(g.graph())
        rows = ref_be.tensor_get(N["fattn"]).copy().reshape(nt, hp["n_head"], 512)
        out = ref_be.tensor_get(N["out"]).copy().reshape(nt, hp["n_embd"])
        g.free()
        want_rows, want = _block_f64(hp, W, xv.astype(np.float64), pos0, K, V)
        e_rows, e_out = nmse(rows, want_rows), nmse(out, want)
        print(f"mla block on the reference backend, {nt} tokens at {pos0}: attention rows NMSE {e_rows:.3e}, block output {e_out:.3e}")
        assert np.isfinite(out).all() and e_rows < 5e-4 and e_out < 5e-4, (nt, e_rows, e_out)
        pos0 += nt
    kc = ref_be.tensor_get(blk.k_cache).copy().reshape(n_ctx, 576).astype(np.float64)
    assert nmse(kc[:pos0], K[:pos0]) < 5e-4 and not kc[pos0:].any()
    blk.wctx.free()
