#!/usr/bin/env python3
"""tools/make_synth_rwkv_gguf.py -- write a small synthetic `rwkv6` or `rwkv7` GGUF v3 file in the manner of tools/make_synth_mamba_gguf.py (the writer helpers are
tools/make_synth_gguf.py's): 2 layers, n_embd 256, 4 heads of 64, feed-forward 512, vocabulary 512, "no_vocab" tokenizer, seeded weights.

  --arch rwkv6   time_mix_extra_dim 32, time_decay_extra_dim 64, the fused lerp weight {n_embd, 1, 1, 5}, time_mix_first {64, 4}.
                 What the reference loader asks: src/llama-model.cpp:1739-1749 (hparams), :5100-5161 (tensors); the graph: llm_build_rwkv6.
  --arch rwkv7   decay / iclr / value-residual / gate LoRA ranks 32 / 32 / 16 / 64, lerp {n_embd, 1, 1, 6}; layer 0 carries time_mix_v0..v2 too ("actually not used", at the
                 iclr rank).  Loader: :1763-1773, :5215-5286; the graph: llm_build_rwkv7.

The n_embd-wide projections (time_mix_key / value / receptance / gate, channel_mix_key / receptance) are Q4_K, time_mix_output and channel_mix_value Q6_K, token embedding
Q4_K, lm head Q6_K; everything the graph multiplies element-wise, the norms and the small LoRA matrices F32 (llama.cpp-omni_amd/rwkv.py layer_shapes is the list).  Decays:
rwkv6 time_mix_decay in (-4, -0.5), so w = exp(-exp(.)) stays in (0.55, 0.98); rwkv7's w = exp(-0.6065 sigmoid(.)) lies in (0.54, 1) whatever w0 is: the states stay
bounded over 64 tokens.  tests/test_rwkv_host.py checks for the default seed that the reference CPU backend's top-1 / top-2 logit margin is wide enough on nearly every
teacher-forced step.

    python tools/make_synth_rwkv_gguf.py --arch rwkv7 -o /tmp/tiny-rwkv7.gguf
"""
import argparse
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synth_gguf import ALIGN, GGUF_MAGIC, GGUF_VERSION, _s, kv_f32, kv_str, kv_u32, load_pkg  # noqa: E402

F32, Q4_K, Q6_K = 0, 12, 14
N_LAYER, N_VOCAB = 2, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--arch", choices=["rwkv6", "rwkv7"], default="rwkv6")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--n-ctx", type=int, default=4096)
    args = ap.parse_args()
    load_pkg()
    from llama_cpp_omni_amd import qwen3, rwkv
    from llama_cpp_omni_amd.ggml import row_size
    arch = args.arch
    E, V = 256, N_VOCAB

    tensors = [("token_embd.weight", Q4_K, (E, V)), ("token_embd_norm.weight", F32, (E,)), ("token_embd_norm.bias", F32, (E,)),
               ("output_norm.weight", F32, (E,)), ("output_norm.bias", F32, (E,)), ("output.weight", Q6_K, (E, V))]
    for il in range(N_LAYER):
        if arch == "rwkv6":
            hp = dict(rwkv.TINY_RWKV6)
        else:
            hp = dict(rwkv.TINY_RWKV7, first=False, gating=True)                             # the loader wants v0..v2 in every layer
            if il == 0:
                hp["lora_v"] = hp["lora_a"]
        for k, sh in rwkv.layer_shapes(hp, Q4_K, Q6_K).items():
            name = k[:-2] + ".bias" if k.endswith("_b") else k + ".weight"
            tensors.append((f"blk.{il}.{name}", sh[0], tuple(sh[1:])))
    hp = rwkv.TINY_RWKV6 if arch == "rwkv6" else rwkv.TINY_RWKV7

    def nbytes(ty, ne):
        return row_size(ty, ne[0]) * (int(np.prod(ne[1:])) if len(ne) > 1 else 1)

    kvs = [kv_str("general.architecture", arch), kv_str("general.name", f"{arch}-tiny-synthetic"), kv_u32("general.file_type", 15), kv_u32("general.quantization_version", 2),
           kv_u32("general.alignment", ALIGN), kv_u32(f"{arch}.block_count", N_LAYER), kv_u32(f"{arch}.context_length", args.n_ctx), kv_u32(f"{arch}.embedding_length", E),
           kv_u32(f"{arch}.feed_forward_length", hp["n_ff"]), kv_u32(f"{arch}.attention.head_count", 0), kv_f32(f"{arch}.attention.layer_norm_epsilon", rwkv.NORM_EPS),
           kv_u32(f"{arch}.wkv.head_size", hp["head_size"]), kv_u32(f"{arch}.token_shift_count", 2), kv_u32(f"{arch}.vocab_size", V), kv_str("tokenizer.ggml.model", "no_vocab")]
    if arch == "rwkv6":
        kvs += [kv_u32(f"{arch}.time_mix_extra_dim", hp["time_mix_extra"]), kv_u32(f"{arch}.time_decay_extra_dim", hp["time_decay_extra"])]
    else:
        kvs += [kv_u32(f"{arch}.attention.decay_lora_rank", hp["lora_decay"]), kv_u32(f"{arch}.attention.iclr_lora_rank", hp["lora_a"]),
                kv_u32(f"{arch}.attention.value_residual_mix_lora_rank", hp["lora_v"]), kv_u32(f"{arch}.attention.gate_lora_rank", hp["lora_g"])]

    offs, off = [], 0
    for _, ty, ne in tensors:
        offs.append(off)
        off = (off + nbytes(ty, ne) + ALIGN - 1) // ALIGN * ALIGN
    head = struct.pack("<IIQQ", GGUF_MAGIC, GGUF_VERSION, len(tensors), len(kvs)) + b"".join(kvs)
    for (name, ty, ne), o in zip(tensors, offs):
        head += _s(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", ty, o)
    head += b"\0" * ((-len(head)) % ALIGN)

    rng = np.random.default_rng(args.seed)

    def f32_data(name, ne):
        n = int(np.prod(ne))
        leaf = name.split(".", 2)[-1] if name.startswith("blk.") else name
        if "lerp" in leaf:
            v = rng.uniform(0.0, 1.0, n)
        elif leaf == "time_mix_decay.weight":
            v = rng.uniform(-4.0, -0.5, n)
        elif leaf.endswith("norm.weight") or leaf.endswith("norm_2.weight") or leaf in ("time_mix_ln.weight", "time_mix_k_k.weight", "time_mix_k_a.weight", "time_mix_r_k.weight"):
            v = rng.uniform(0.5, 1.5, n)
        elif leaf.endswith(".bias") or leaf in ("time_mix_w0.weight", "time_mix_a0.weight", "time_mix_v0.weight", "time_mix_first.weight"):
            v = rng.standard_normal(n) * 0.3
        else:
            v = rng.standard_normal(n) / np.sqrt(ne[0])                                    # the LoRA matrices
        return v.astype(np.float32).view(np.uint8)

    with open(args.out, "wb") as f:
        f.write(head)
        base = f.tell()
        for (name, ty, ne), o in zip(tensors, offs):
            f.write(b"\0" * (base + o - f.tell()))
            if ty == F32:
                d = f32_data(name, ne)
            else:
                std = 0.05 if name in ("token_embd.weight", "output.weight") else 1.0 / np.sqrt(ne[0])
                d = qwen3.random_blocks(rng, ty, int(np.prod(ne[1:])), ne[0], std=std).reshape(-1)
            assert d.nbytes == nbytes(ty, ne), (name, d.nbytes, nbytes(ty, ne))
            f.write(d.tobytes())
        f.write(b"\0" * ((-f.tell()) % ALIGN))
    print(f"wrote {args.out}: {arch}, {len(tensors)} tensors, {os.path.getsize(args.out) / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
