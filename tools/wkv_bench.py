#!/usr/bin/env python3
"""tools/wkv_bench.py -- RWKV_WKV6, GATED_LINEAR_ATTN and RWKV_WKV7 (kernels/wkv.hip) at 7B shapes (64 heads of 64), timed as replayed captures through the backend C-ABI
in the manner of tools/ssm_bench.py: device time per launch, the launch's algorithmic bytes (the states read once and written once, 2 x 1 MiB per sequence, the operands
read, the outputs written) and, for the decode cases, the fraction of 8 TB/s.  Cases: one token of 1 / 8 / 32 sequences, and a 512-token prompt of one sequence.

One cgraph holds N independent nodes, every node with its own operands (N x bytes > --min-mib MiB, default 768: the 256 MiB Infinity Cache cannot serve re-reads); it is
run eager, captured, then replayed (at least 8 nodes); the best of --reps replays is reported per node.  --rounds alternating rounds show the run-to-run spread.

usage: python tools/wkv_bench.py [--reps 5] [--rounds 3] [--min-mib 768] > profiles/wkv_bench.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

F32 = 0
HBM = 8.0e12
S, H = 64, 64
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-mib", type=int, default=768)
    args = ap.parse_args()
    pkg = load_pkg()
    from llama_cpp_omni_amd.ggml import Context
    be = pkg.backend(0)
    rng = np.random.default_rng(0)
    for rnd in range(args.rounds):
        for op in ("wkv6", "gla", "wkv7"):
            for n_t, n_s in [(1, 1), (1, 8), (1, 32), (512, 1)]:
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
                small = (rng.standard_normal((T, H, S)) * 0.1).astype(np.float32)      # every operand small: the states stay bounded over 512 tokens whatever the operand's role
                sv = rng.standard_normal((n_s, S * S * H)).astype(np.float32)
                for t3, st in ins:
                    for t in t3:
                        be.tensor_set(t, small)
                    be.tensor_set(st, sv)
                us = timed(be, c.graph(), args.reps) / n
                c.free()
                share = f"{node_bytes / us / 1e-6 / HBM:5.3f} of 8 TB/s, " if n_t == 1 else ""
                print(f"round {rnd} {op:4s} n_t={n_t:3d} n_s={n_s:2d}: {node_bytes / 1e6:6.1f} MB/launch  {us:8.2f} us ({node_bytes / us / 1e3:7.1f} GB/s, {share}{n} nodes)  "
                      f"bytes / 8 TB/s {node_bytes / HBM * 1e6:6.2f} us", flush=True)


if __name__ == "__main__":
    main()
