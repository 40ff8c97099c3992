#!/usr/bin/env python3
"""tools/make_synth_gptoss_gguf.py -- write a small synthetic `gpt-oss` GGUF v3 file in the manner of tools/make_synth_moe_gguf.py (whose writer helpers and
separated-logits construction it uses): 2 layers (SWA pattern 2: layer 0 attends through a 16-token sliding window, layer 1 over everything), n_embd 256, 4 / 2 heads
of 64, vocabulary 512, 8 experts with 4 used and n_ff_exp = 288 -- the down experts then have 9-block rows of 153 bytes, so every second row starts at an odd address.
MXFP4 experts, Q4_K attention and token_embd, Q6_K output; F32 norms, attention biases, attention sinks, router, router bias and per-expert biases; "no_vocab" tokenizer.
What the reference loader asks of the architecture: src/llama-model.cpp:1995-2009 (hparams), :5843-5882 (tensors); the graph: llm_build_openai_moe_iswa, :18555 ff.

The file is a greedy-decoding fixture with SEPARATED logits (see make_synth_moe_gguf.py): S special tokens whose embedding dominates the residual stream and whose
successor's lm-head row points along it, and per layer a router solved so that the logits of special token i are a permutation of 0, 1.5, 3, ...; the router BIAS is
kept within +-0.25, so neighbouring logits stay at least 1.0 apart and the four experts a token picks do not sit on rounding.  Sinks and expert biases are random of order 1.

    python tools/make_synth_gptoss_gguf.py -o /tmp/tiny-gptoss.gguf        (prints the special ids: the start token and the cycle)
"""
import argparse
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synth_gguf import ALIGN, GGUF_MAGIC, GGUF_VERSION, _s, dequant_q4_K, dequant_q6_K, kv_f32, kv_str, kv_u32, load_pkg, quant_q6_K  # noqa: E402
from make_synth_moe_gguf import LOGIT_STEP, special_ids  # noqa: E402

CFG = dict(n_embd=256, n_layer=2, n_head=4, n_head_kv=2, head_dim=64, n_vocab=512, n_expert=8, n_expert_used=4, n_ff_exp=288, sliding_window=16, rms_eps=1e-6, rope_base=1e6)
F32, Q4_K, Q6_K, MXFP4 = 0, 12, 14, 39


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
        b = f"blk.{il}."
        tensors += [(b + "attn_norm.weight", F32, (E,)), (b + "post_attention_norm.weight", F32, (E,)),
                    (b + "attn_q.weight", Q4_K, (E, H * D)), (b + "attn_k.weight", Q4_K, (E, HK * D)), (b + "attn_v.weight", Q4_K, (E, HK * D)), (b + "attn_output.weight", Q4_K, (H * D, E)),
                    (b + "attn_sinks.weight", F32, (H,)),
                    (b + "ffn_gate_inp.weight", F32, (E, X)),
                    (b + "ffn_gate_exps.weight", MXFP4, (E, F, X)), (b + "ffn_down_exps.weight", MXFP4, (F, E, X)), (b + "ffn_up_exps.weight", MXFP4, (E, F, X)),
                    (b + "attn_q.bias", F32, (H * D,)), (b + "attn_k.bias", F32, (HK * D,)), (b + "attn_v.bias", F32, (HK * D,)), (b + "attn_output.bias", F32, (E,)),
                    (b + "ffn_gate_inp.bias", F32, (X,)),
                    (b + "ffn_gate_exps.bias", F32, (F, X)), (b + "ffn_down_exps.bias", F32, (E, X)), (b + "ffn_up_exps.bias", F32, (F, X))]

    def nbytes(ty, ne):
        return row_size(ty, ne[0]) * (int(np.prod(ne[1:])) if len(ne) > 1 else 1)

    arch = "gpt-oss"
    kvs = [kv_str("general.architecture", arch), kv_str("general.name", "gpt-oss-tiny-synthetic"), kv_u32("general.file_type", 38), kv_u32("general.quantization_version", 2),
           kv_u32("general.alignment", ALIGN), kv_u32(f"{arch}.block_count", L), kv_u32(f"{arch}.context_length", args.n_ctx), kv_u32(f"{arch}.embedding_length", E),
           kv_u32(f"{arch}.feed_forward_length", F), kv_u32(f"{arch}.expert_feed_forward_length", F), kv_u32(f"{arch}.expert_count", X), kv_u32(f"{arch}.expert_used_count", XU),
           kv_u32(f"{arch}.attention.head_count", H), kv_u32(f"{arch}.attention.head_count_kv", HK), kv_u32(f"{arch}.attention.key_length", D),
           kv_u32(f"{arch}.attention.value_length", D), kv_u32(f"{arch}.attention.sliding_window", c["sliding_window"]),
           kv_f32(f"{arch}.attention.layer_norm_rms_epsilon", c["rms_eps"]), kv_f32(f"{arch}.rope.freq_base", c["rope_base"]),
           kv_u32(f"{arch}.vocab_size", V), kv_str("tokenizer.ggml.model", "no_vocab")]

    offs, off = [], 0
    for _, ty, ne in tensors:
        offs.append(off)
        off = (off + nbytes(ty, ne) + ALIGN - 1) // ALIGN * ALIGN
    head = struct.pack("<IIQQ", GGUF_MAGIC, GGUF_VERSION, len(tensors), len(kvs)) + b"".join(kvs)
    for (name, ty, ne), o in zip(tensors, offs):
        head += _s(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", ty, o)
    head += b"\0" * ((-len(head)) % ALIGN)

    # ---- the separated-logits fixture: embedding rows, successor lm-head rows, router rows and router bias
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
        bias = r3.uniform(-0.25, 0.25, X).astype(np.float32)                           # the 1.5 step still separates: neighbours stay >= 1.0 apart
        srt = np.sort(chk + bias[:, None], axis=0)
        assert np.min(srt[1:] - srt[:-1]) > 0.9
        fixed[f"blk.{il}.ffn_gate_inp.weight"] = G.reshape(-1).view(np.uint8)
        fixed[f"blk.{il}.ffn_gate_inp.bias"] = bias.view(np.uint8)
    print("separated-logits gpt-oss fixture: start token", special[0], "cycle", special[:4], "...")

    rng = np.random.default_rng(args.seed + 1)
    with open(args.out, "wb") as f:
        f.write(head)
        base = f.tell()
        for (name, ty, ne), o in zip(tensors, offs):
            f.write(b"\0" * (base + o - f.tell()))
            n = int(np.prod(ne))
            if name in fixed:
                d = fixed[name]
            elif name.endswith("norm.weight"):
                d = np.ones(n, np.float32).view(np.uint8)
            elif name.endswith("attn_sinks.weight") or "_exps.bias" in name:
                d = rng.standard_normal(n).astype(np.float32).view(np.uint8)             # order 1
            elif ty == F32:
                d = (rng.standard_normal(n) * 0.1).astype(np.float32).view(np.uint8)     # q / k / v / o biases
            else:
                d = qwen3.random_blocks(rng, ty, int(np.prod(ne[1:])), ne[0]).reshape(-1)
            assert d.nbytes == nbytes(ty, ne), (name, d.nbytes, nbytes(ty, ne))
            f.write(d.tobytes())
        f.write(b"\0" * ((-f.tell()) % ALIGN))
    print(f"wrote {args.out}: {len(tensors)} tensors, {os.path.getsize(args.out) / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
