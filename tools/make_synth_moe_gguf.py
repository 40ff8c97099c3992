#!/usr/bin/env python3
"""tools/make_synth_moe_gguf.py -- write a small synthetic `qwen3moe` GGUF v3 file in the manner of tools/make_synth_gguf.py (whose writer helpers it uses):
2 layers, n_embd 256, 4 / 2 heads of 64, vocabulary 512, 8 experts of n_ff 256 with 2 used; Q4_K attention / token_embd / expert gate and up, Q6_K expert down and
output, F32 router (ffn_gate_inp) and norms, "no_vocab" tokenizer.  What the reference loader asks of the architecture: src/llama-model.cpp:1015-1025 (hparams),
:3297-3340 (tensors); the graph: llm_build_qwen3moe, :9408-9534.

The file is a greedy-decoding fixture with SEPARATED logits, like make_synth_gguf.py --separated: S special tokens whose embedding dominates the residual stream and whose
successor's lm-head row points along it (token s_i -> s_(i+1)), so the winning logit leads by far more than any summation-order noise.  The same is done for the ROUTER:
every layer's ffn_gate_inp is solved (least norm) so that, on the unit-rms direction of special token i, the router logits are a permutation of 0, 1.5, 3, ... chosen for
(layer, i) -- the experts a token picks do not sit on rounding either, and they differ from token to token and layer to layer.  Without it two correct backends could
choose different experts and the ids would diverge.

    python tools/make_synth_moe_gguf.py -o /tmp/tiny-moe.gguf        (prints the special ids: the start token and the cycle)
"""
import argparse
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synth_gguf import ALIGN, GGUF_MAGIC, GGUF_VERSION, _s, dequant_q4_K, dequant_q6_K, kv_f32, kv_str, kv_u32, load_pkg, quant_q6_K  # noqa: E402

CFG = dict(n_embd=256, n_layer=2, n_head=4, n_head_kv=2, head_dim=64, n_vocab=512, n_expert=8, n_expert_used=2, n_ff_exp=256, rms_eps=1e-6, rope_base=1e6)
F32, Q4_K, Q6_K = 0, 12, 14
LOGIT_STEP = 1.5


def special_ids(S, V=CFG["n_vocab"]):
    return [int(V // 16 + (V - V // 8) * i // S) for i in range(S)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--separated", type=int, default=96, metavar="S", help="number of special tokens in the cycle (longer than prompt + run)")
    ap.add_argument("--n-ctx", type=int, default=4096)
    args = ap.parse_args()
    load_pkg()
    from llama_cpp_omni_amd import qwen3
    from llama_cpp_omni_amd.ggml import row_size
    c = CFG
    E, H, HK, D, V, L, X, XU, F = c["n_embd"], c["n_head"], c["n_head_kv"], c["head_dim"], c["n_vocab"], c["n_layer"], c["n_expert"], c["n_expert_used"], c["n_ff_exp"]
    S = args.separated
    assert 2 <= S <= E, "the router rows are solved exactly for up to n_embd directions"

    tensors = [("token_embd.weight", Q4_K, (E, V)), ("output_norm.weight", F32, (E,)), ("output.weight", Q6_K, (E, V))]
    for il in range(L):
        tensors += [(f"blk.{il}.attn_norm.weight", F32, (E,)), (f"blk.{il}.attn_q.weight", Q4_K, (E, H * D)), (f"blk.{il}.attn_k.weight", Q4_K, (E, HK * D)),
                    (f"blk.{il}.attn_v.weight", Q6_K, (E, HK * D)), (f"blk.{il}.attn_output.weight", Q4_K, (H * D, E)),
                    (f"blk.{il}.attn_q_norm.weight", F32, (D,)), (f"blk.{il}.attn_k_norm.weight", F32, (D,)), (f"blk.{il}.ffn_norm.weight", F32, (E,)),
                    (f"blk.{il}.ffn_gate_inp.weight", F32, (E, X)),
                    (f"blk.{il}.ffn_gate_exps.weight", Q4_K, (E, F, X)), (f"blk.{il}.ffn_up_exps.weight", Q4_K, (E, F, X)), (f"blk.{il}.ffn_down_exps.weight", Q6_K, (F, E, X))]

    def nbytes(ty, ne):
        return row_size(ty, ne[0]) * (int(np.prod(ne[1:])) if len(ne) > 1 else 1)

    arch = "qwen3moe"
    kvs = [kv_str("general.architecture", arch), kv_str("general.name", "qwen3moe-tiny-synthetic"), kv_u32("general.file_type", 15), kv_u32("general.quantization_version", 2),
           kv_u32("general.alignment", ALIGN), kv_u32(f"{arch}.block_count", L), kv_u32(f"{arch}.context_length", args.n_ctx), kv_u32(f"{arch}.embedding_length", E),
           kv_u32(f"{arch}.feed_forward_length", F), kv_u32(f"{arch}.expert_feed_forward_length", F), kv_u32(f"{arch}.expert_count", X), kv_u32(f"{arch}.expert_used_count", XU),
           kv_u32(f"{arch}.attention.head_count", H), kv_u32(f"{arch}.attention.head_count_kv", HK), kv_u32(f"{arch}.attention.key_length", D),
           kv_u32(f"{arch}.attention.value_length", D), kv_f32(f"{arch}.attention.layer_norm_rms_epsilon", c["rms_eps"]), kv_f32(f"{arch}.rope.freq_base", c["rope_base"]),
           kv_u32(f"{arch}.vocab_size", V), kv_str("tokenizer.ggml.model", "no_vocab")]

    offs, off = [], 0
    for _, ty, ne in tensors:
        offs.append(off)
        off = (off + nbytes(ty, ne) + ALIGN - 1) // ALIGN * ALIGN
    head = struct.pack("<IIQQ", GGUF_MAGIC, GGUF_VERSION, len(tensors), len(kvs)) + b"".join(kvs)
    for (name, ty, ne), o in zip(tensors, offs):
        head += _s(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", ty, o)
    head += b"\0" * ((-len(head)) % ALIGN)

    # ---- the separated-logits fixture: embedding rows, successor lm-head rows, router rows
    special = special_ids(S, V)
    r2 = np.random.default_rng(args.seed + 77)
    big = qwen3.random_blocks(r2, Q4_K, S, E, std=300.0)                               # embedding rows ~ 20x what the random layers add
    ehat = dequant_q4_K(big.reshape(S, -1), E)
    ehat /= np.sqrt((ehat ** 2).mean(axis=1, keepdims=True))                           # unit rms: what the RMS norms make of a residual stream the embedding dominates
    out_rows = quant_q6_K(ehat)
    logit = dequant_q6_K(out_rows, E) @ ehat.T
    for i in range(S):
        col = logit[:, i].copy(); top = col[i]; col[i] = -np.inf
        assert top > 0.9 * E and col.max() < 0.7 * top, (i, top, col.max())
    embd = qwen3.random_blocks(np.random.default_rng(args.seed), Q4_K, V, E).reshape(V, -1)
    outw = qwen3.random_blocks(np.random.default_rng(args.seed + 78), Q6_K, V, E, std=1e-3).reshape(V, -1)      # every other lm-head row: tiny
    for i in range(S):
        embd[special[i]] = big[i]
        outw[special[(i + 1) % S]] = out_rows[i]
    fixed = {"token_embd.weight": embd.reshape(-1), "output.weight": outw.reshape(-1)}
    r3 = np.random.default_rng(args.seed + 79)
    pinv = np.linalg.pinv(ehat.astype(np.float64).T)                                   # [S, E]: G = C . pinv gives G . ehat^T = C exactly (S <= E independent directions)
    for il in range(L):
        C = np.stack([r3.permutation(X) for _ in range(S)], axis=1).astype(np.float64) * LOGIT_STEP      # [X, S]: token i's router logits in layer il
        G = (C @ pinv).astype(np.float32)                                              # [X, E]
        chk = G.astype(np.float64) @ ehat.T.astype(np.float64)
        assert np.abs(chk - C).max() < 1e-3, np.abs(chk - C).max()
        fixed[f"blk.{il}.ffn_gate_inp.weight"] = G.reshape(-1).view(np.uint8)
    print("separated-logits qwen3moe fixture: start token", special[0], "cycle", special[:4], "...")

    rng = np.random.default_rng(args.seed + 1)
    with open(args.out, "wb") as f:
        f.write(head)
        base = f.tell()
        for (name, ty, ne), o in zip(tensors, offs):
            f.write(b"\0" * (base + o - f.tell()))
            if name in fixed:
                d = fixed[name]
            elif ty == F32:
                d = np.ones(ne[0], np.float32).view(np.uint8)
            else:
                d = qwen3.random_blocks(rng, ty, int(np.prod(ne[1:])), ne[0]).reshape(-1)
            assert d.nbytes == nbytes(ty, ne), (name, d.nbytes, nbytes(ty, ne))
            f.write(d.tobytes())
        f.write(b"\0" * ((-f.tell()) % ALIGN))
    print(f"wrote {args.out}: {len(tensors)} tensors, {os.path.getsize(args.out) / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
