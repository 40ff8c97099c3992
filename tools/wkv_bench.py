#!/usr/bin/env python3
"""tools/wkv_bench.py -- RWKV_WKV6, GATED_LINEAR_ATTN and RWKV_WKV7 (kernels/wkv.hip, kernels/wkv_chunk.hip) at 7B shapes (64 heads of 64), timed as replayed captures through
the backend C-ABI in the manner of tools/ssm_bench.py: device time per launch, the launch's algorithmic bytes (the states read once and written once, 2 x 1 MiB per sequence,
the operands read, the outputs written) and, for the decode cases, the fraction of 8 TB/s.

  decode one token of 1 / 8 / 32 sequences, the three ops.
  prompt WKV6 and GLA at 16 .. 2048 tokens of one sequence, 64 .. 512 tokens of 4 and 8 sequences, and 32 heads of 128 at 1 / 2 / 4 sequences, option "wkv_chunk" alternating in one call: 0 = the serial kernel k_wkv6,
         2 = the chunked matrix-core kernel at every token count and grid (the short and the many-sequence ones are there to locate the crossovers); WKV7, which has no chunked kernel, at 512 tokens.  A
         library without the option (an earlier build, through MI355X_LIB) runs the one leg it has.
  prompt7 WKV7 (kernels/wkv7_chunk.hip) at 16 .. 2048 tokens of one sequence and 64 .. 512 of 4 and 8, 64 heads of 64 and 32 heads of 128, the option alternating the same way: 0 = k_wkv7,
         2 = k_wkv7_chunk.  A build from before that kernel runs k_wkv7 alone.

One cgraph holds N independent nodes, every node with its own operands (N x bytes > --min-mib MiB, default 768: the 256 MiB Infinity Cache cannot serve re-reads); it is
run eager, captured, then replayed (at least 8 nodes); the best of --reps replays is reported per node.  --rounds alternating rounds show the run-to-run spread.

usage: python tools/wkv_bench.py [--reps 5] [--rounds 3] [--min-mib 768] [--legs decode,prompt] > profiles/wkv_bench.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

F32 = 0
HBM = 8.0e12
MAIN = (64, 64)                                          # (head size, heads)
WIDE = (128, 32)
N_OPERANDS = {"wkv6": 4, "gla": 4, "wkv7": 6}           # {S, H, T} operands read per token


def timed(be, g, reps):
    for _ in range(3):
        be.graph_compute(g)                   # eager, capture, first replay
    be.synchronize()
    best = 1e30
    for _ in range(reps):
        a, b = be.timed_event(), be.timed_event()
        be.record(a)
        be.graph_compute(g)
        be.record(b)
        best = min(best, be.elapsed_ms(a, b))
    return best * 1e3


def leg(be, rng, args, label, op, shape, n_t, n_s, chunked=None):
    from llama_cpp_omni_amd.ggml import Context
    S, H = shape
    T = n_t * n_s
    node_bytes = 2 * S * S * H * n_s * 4 + (N_OPERANDS[op] + 1) * S * H * T * 4
    n = max(8, min(256, (args.min_mib << 20) // node_bytes + 1))
    c = Context(be)
    tf = c.new_tensor(F32, S, H)
    ys, ins = [], []
    for _ in range(n):
        t3 = [c.new_tensor(F32, S, H, T) for _ in range(N_OPERANDS[op])]
        st = c.new_tensor(F32, S * S * H, n_s)
        if op == "wkv6":
            ys.append(c.rwkv_wkv6(t3[0], t3[1], t3[2], tf, t3[3], st))
        elif op == "gla":
            ys.append(c.gated_linear_attn(t3[0], t3[1], t3[2], t3[3], st, S ** -0.5))
        else:
            ys.append(c.rwkv_wkv7(*t3, st))
        ins.append((t3, st))
    assert be.supports_op(ys[0])
    c.alloc()
    be.tensor_set(tf, rng.standard_normal((H, S)).astype(np.float32))
    small = (rng.standard_normal((T, H, S)) * 0.1).astype(np.float32)      # every operand small: the states stay bounded over the prompt whatever the operand's role
    decay = rng.uniform(0.3, 1.0, (T, H, S)).astype(np.float32)            # WKV6 / GLA: the decay operand in a model's range
    sv = rng.standard_normal((n_s, S * S * H)).astype(np.float32)
    for t3, st in ins:
        for i, t in enumerate(t3):
            be.tensor_set(t, decay if i == (1 if op == "wkv7" else 3) else small)      # (WKV7: r w k v a b)
        be.tensor_set(st, sv)
    key = f"{op}_chunk_launches"
    k0 = be.get_stat(key) if chunked is not None else 0
    us = timed(be, c.graph(), args.reps) / n
    if chunked is not None:
        d = be.get_stat(key) - k0
        assert d == 2 * n if chunked else d == 0, (label, d)               # eager + capture: the leg ran the kernel it names
    c.free()
    share = f"{node_bytes / us / 1e-6 / HBM:5.3f} of 8 TB/s, " if n_t == 1 else ""
    print(f"{label} {op:4s} S={S:3d} H={H:2d} n_t={n_t:4d} n_s={n_s:2d}: {node_bytes / 1e6:6.1f} MB/launch  {us:8.2f} us ({node_bytes / us / 1e3:7.1f} GB/s, {share}{n} nodes)  "
          f"bytes / 8 TB/s {node_bytes / HBM * 1e6:6.2f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-mib", type=int, default=768)
    ap.add_argument("--legs", default="decode,prompt")
    args = ap.parse_args()
    pkg = load_pkg()
    be = pkg.backend(0)
    rng = np.random.default_rng(0)
    legs = args.legs.split(",")
    for rnd in range(args.rounds):
        if "decode" in legs:
            for op in ("wkv6", "gla", "wkv7"):
                for n_s in (1, 8, 32):
                    leg(be, rng, args, f"round {rnd} decode        ", op, MAIN, 1, n_s)
        if "prompt7" in legs:
            has7 = be.get_stat("wkv7_chunk_min_tokens") > 0                  # (a build from before wkv7_chunk.hip: the one kernel it has)
            for shape, n_t, n_s in ([(MAIN, t, 1) for t in (16, 32, 48, 64, 96, 128, 256, 512, 2048)] + [(MAIN, t, n) for n in (4, 8) for t in (64, 128, 512)]
                                    + [(WIDE, t, 1) for t in (32, 64, 128, 512, 2048)] + [(WIDE, t, n) for n in (4, 8) for t in (64, 512)]):
                for mode, name in ((0, "serial "), (2, "chunked")) if has7 else ((-1, "no kern."),):
                    be.set_option("wkv_chunk", mode)
                    try:
                        leg(be, rng, args, f"round {rnd} prompt {name}", "wkv7", shape, n_t, n_s, chunked=mode == 2 if has7 else None)
                    finally:
                        be.set_option("wkv_chunk", -1)
        if "prompt" not in legs:
            continue
        leg(be, rng, args, f"round {rnd} prompt        ", "wkv7", MAIN, 512, 1)
        for shape, n_t, n_s in [(MAIN, t, 1) for t in (16, 32, 48, 64, 96, 128, 256, 512, 2048)] + [(MAIN, 64, 4), (MAIN, 128, 4), (MAIN, 512, 4), (MAIN, 64, 8), (MAIN, 512, 8)] + [((128, 32), t, n) for t, n in ((64, 1), (128, 1), (512, 1), (64, 2), (512, 2), (512, 4))]:
            for op in ("wkv6", "gla"):
                for mode, name in ((0, "serial "), (2, "chunked")):
                    if be.set_option("wkv_chunk", mode) != 0:
                        if mode == 0:
                            leg(be, rng, args, f"round {rnd} prompt no opt.", op, shape, n_t, n_s)
                        continue
                    try:
                        leg(be, rng, args, f"round {rnd} prompt {name}", op, shape, n_t, n_s, chunked=mode == 2)
                    finally:
                        be.set_option("wkv_chunk", -1)


if __name__ == "__main__":
    main()
