#!/usr/bin/env python3
"""tools/make_synth_mamba_gguf.py -- write a small synthetic `mamba2` or `mamba` GGUF v3 file in the manner of tools/make_synth_moe_gguf.py (the writer helpers are
tools/make_synth_gguf.py's): 2 layers, n_embd 256, d_inner 512 (the loader insists on 2 * n_embd), d_conv 4, vocabulary 512, "no_vocab" tokenizer, seeded weights.

  --arch mamba2   d_state 128, 8 heads of 64 (ssm.time_step_rank is the head count), 2 groups; ssm_in Q4_K, ssm_out Q6_K; ssm_conv1d weight and bias, ssm_dt.bias,
                  ssm_a {1, n_head} (negative, as real files have it), ssm_d {1, n_head}, ssm_norm {d_inner / n_group, n_group} (one row per group, the rows differ) F32.
                  What the reference loader asks: src/llama-model.cpp:1296-1304 (hparams), :3906-3953 (tensors); the graph: build_mamba2_layer.
  --arch mamba    d_state 16, dt_rank 16; ssm_in and ssm_x Q4_K, ssm_out Q6_K, ssm_dt.weight (K = 16) F32, ssm_a {16, 512} negative, ssm_d {512}.
                  Loader: :1265-1295, :3859-3905; the graph: build_mamba_layer.
  --dt-b-c-rms    (mamba) sets mamba.ssm.dt_b_c_rms: RMS norms on dt, B and C (FalconMamba).  The reference's loader creates NO ssm_dt_norm / ssm_b_norm / ssm_c_norm
                  tensors for a `mamba` file (:3882-3904) -- build_mamba_layer then runs the three norms WITHOUT a weight (build_norm with mw == NULL).  Norm weights
                  exist only in a `jamba` file (:3954-..., layer.ssm_dt_norm), which also needs that architecture's attention and MoE layers: not written here.

Token embedding Q4_K, lm head Q6_K, norms F32.  Nothing is separated: the weights are plain seeded random blocks; tests/test_ssm_host.py checks for the default
seed that the reference CPU backend's top-1 / top-2 logit margin is wide enough on nearly every teacher-forced step.

    python tools/make_synth_mamba_gguf.py --arch mamba2 -o /tmp/tiny-mamba2.gguf
"""
import argparse
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synth_gguf import ALIGN, GGUF_MAGIC, GGUF_VERSION, _s, kv_bool, kv_f32, kv_str, kv_u32, load_pkg  # noqa: E402

F32, Q4_K, Q6_K = 0, 12, 14
CFG = {"mamba2": dict(n_embd=256, n_layer=2, n_vocab=512, d_inner=512, d_state=128, dt_rank=8, n_group=2, d_conv=4, rms_eps=1e-5),
       "mamba": dict(n_embd=256, n_layer=2, n_vocab=512, d_inner=512, d_state=16, dt_rank=16, n_group=1, d_conv=4, rms_eps=1e-5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--arch", choices=["mamba2", "mamba"], default="mamba2")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--dt-b-c-rms", action="store_true", help="mamba: RMS norms (without weights, as the loader takes a `mamba` file) on dt, B and C")
    ap.add_argument("--n-ctx", type=int, default=4096)
    args = ap.parse_args()
    load_pkg()
    from llama_cpp_omni_amd import qwen3
    from llama_cpp_omni_amd.ggml import row_size
    arch, c = args.arch, CFG[args.arch]
    E, L, V, DI, DS, R, G, DC = c["n_embd"], c["n_layer"], c["n_vocab"], c["d_inner"], c["d_state"], c["dt_rank"], c["n_group"], c["d_conv"]
    assert not (args.dt_b_c_rms and arch != "mamba"), "--dt-b-c-rms is a `mamba` key"

    tensors = [("token_embd.weight", Q4_K, (E, V)), ("output_norm.weight", F32, (E,)), ("output.weight", Q6_K, (E, V))]
    for il in range(L):
        b = f"blk.{il}."
        if arch == "mamba2":
            d_xbc = DI + 2 * G * DS
            tensors += [(b + "attn_norm.weight", F32, (E,)), (b + "ssm_in.weight", Q4_K, (E, 2 * DI + 2 * G * DS + R)), (b + "ssm_conv1d.weight", F32, (DC, d_xbc)),
                        (b + "ssm_conv1d.bias", F32, (d_xbc,)), (b + "ssm_dt.bias", F32, (R,)), (b + "ssm_a", F32, (1, R)), (b + "ssm_d", F32, (1, R)),
                        (b + "ssm_norm.weight", F32, (DI // G, G)), (b + "ssm_out.weight", Q6_K, (DI, E))]
        else:
            tensors += [(b + "attn_norm.weight", F32, (E,)), (b + "ssm_in.weight", Q4_K, (E, 2 * DI)), (b + "ssm_conv1d.weight", F32, (DC, DI)), (b + "ssm_conv1d.bias", F32, (DI,)),
                        (b + "ssm_x.weight", Q4_K, (DI, R + 2 * DS)), (b + "ssm_dt.weight", F32, (R, DI)), (b + "ssm_dt.bias", F32, (DI,)), (b + "ssm_a", F32, (DS, DI)),
                        (b + "ssm_d", F32, (DI,)), (b + "ssm_out.weight", Q6_K, (DI, E))]

    def nbytes(ty, ne):
        return row_size(ty, ne[0]) * (int(np.prod(ne[1:])) if len(ne) > 1 else 1)

    kvs = [kv_str("general.architecture", arch), kv_str("general.name", f"{arch}-tiny-synthetic"), kv_u32("general.file_type", 15), kv_u32("general.quantization_version", 2),
           kv_u32("general.alignment", ALIGN), kv_u32(f"{arch}.block_count", L), kv_u32(f"{arch}.context_length", args.n_ctx), kv_u32(f"{arch}.embedding_length", E),
           kv_u32(f"{arch}.feed_forward_length", 0), kv_u32(f"{arch}.attention.head_count", 0), kv_f32(f"{arch}.attention.layer_norm_rms_epsilon", c["rms_eps"]),
           kv_u32(f"{arch}.ssm.conv_kernel", DC), kv_u32(f"{arch}.ssm.inner_size", DI), kv_u32(f"{arch}.ssm.state_size", DS), kv_u32(f"{arch}.ssm.time_step_rank", R),
           kv_u32(f"{arch}.vocab_size", V), kv_str("tokenizer.ggml.model", "no_vocab")]
    if arch == "mamba2":
        kvs.append(kv_u32(f"{arch}.ssm.group_count", G))
    if args.dt_b_c_rms:
        kvs.append(kv_bool(f"{arch}.ssm.dt_b_c_rms", True))

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
        if name.endswith("ssm_a"):
            v = -rng.uniform(0.1, 2.0, n)                                                 # negative: the state decays
        elif name.endswith("ssm_d") or name.endswith("ssm_norm.weight"):
            v = rng.uniform(0.5, 1.5, n)                                                  # (ssm_norm: the two groups' rows differ)
        elif name.endswith("ssm_conv1d.weight"):
            v = rng.standard_normal(n) * 0.5
        elif name.endswith("ssm_conv1d.bias"):
            v = rng.standard_normal(n) * 0.1
        elif name.endswith("ssm_dt.bias"):
            v = rng.uniform(-2.0, 1.0, n)
        elif name.endswith("ssm_dt.weight"):
            v = rng.standard_normal(n) / np.sqrt(ne[0])
        else:
            v = np.ones(n)                                                                # attn_norm, output_norm
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
