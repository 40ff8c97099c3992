#!/usr/bin/env python3
"""tools/ssm_bench.py -- SSM_SCAN and SSM_CONV (kernels/ssm.hip) at Mamba-2 2.7B shapes, timed as replayed captures through the backend C-ABI in the manner of
tools/moe_mmv_bench.py: device time per launch, the launch's algorithmic bytes, and the fraction of 8 TB/s.

  scan   d_state 128, head_dim 64, 80 heads, one group, at (n_t, n_s) = (1, 1), (1, 8), (1, 32), (512, 1).  Bytes: the states read once and written once (2 x 2.6 MB per
         sequence), x, B, C and dt read, y written.
  conv   5376 channels (d_inner 5120 + 2 x 128), d_conv 4, one sequence, at n_t = 1 and 512.  Bytes: the window tile read, y written, the weights.

One cgraph holds N independent nodes, every node with its own operands (N x bytes > --min-mib MiB, default 768: the 256 MiB Infinity Cache cannot serve re-reads); it is
run eager, captured, then replayed (at least 8 nodes: shorter graphs are never captured); the best of --reps replays is reported per node.  --rounds alternating rounds show the run-to-run spread.

usage: python tools/ssm_bench.py [--reps 5] [--rounds 3] [--min-mib 768] > profiles/ssm_bench.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

F32, I32 = 0, 26
HBM = 8.0e12
D_STATE, HEAD_DIM, N_HEAD, N_GROUP, D_CONV = 128, 64, 80, 1, 4
D_INNER = HEAD_DIM * N_HEAD
D_XBC = D_INNER + 2 * N_GROUP * D_STATE


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
        for n_t, n_s in [(1, 1), (1, 8), (1, 32), (512, 1)]:
            state = D_STATE * D_INNER * n_s * 4
            node_bytes = 2 * state + (D_XBC + N_HEAD) * n_t * n_s * 4 + D_INNER * n_t * n_s * 4
            n = max(8, min(256, (args.min_mib << 20) // node_bytes + 1))
            c = Context(be)
            A = c.new_tensor(F32, 1, N_HEAD)
            ids = c.new_tensor(I32, n_s)
            ys, ins = [], []
            for _ in range(n):
                xBC = c.new_tensor(F32, D_XBC, n_t, n_s)
                x = c.view_4d(xBC, HEAD_DIM, N_HEAD, n_t, n_s, HEAD_DIM * 4, xBC.nb[1], xBC.nb[2], 0)
                B = c.view_4d(xBC, D_STATE, N_GROUP, n_t, n_s, D_STATE * 4, xBC.nb[1], xBC.nb[2], D_INNER * 4)
                C_ = c.view_4d(xBC, D_STATE, N_GROUP, n_t, n_s, D_STATE * 4, xBC.nb[1], xBC.nb[2], (D_INNER + N_GROUP * D_STATE) * 4)
                s = c.new_tensor(F32, D_STATE, HEAD_DIM, N_HEAD, n_s)
                dt = c.new_tensor(F32, N_HEAD, n_t, n_s)
                ys.append(c.ssm_scan(s, x, dt, A, B, C_, ids))
                ins.append((xBC, s, dt))
            assert be.supports_op(ys[0])
            c.alloc()
            be.tensor_set(A, -rng.uniform(0.05, 1.0, (N_HEAD, 1)).astype(np.float32))
            be.tensor_set(ids, np.arange(n_s, dtype=np.int32))
            xv, sv, dv = (rng.standard_normal((n_s, n_t, D_XBC)).astype(np.float32), rng.standard_normal((n_s, N_HEAD, HEAD_DIM, D_STATE)).astype(np.float32),
                          rng.uniform(-2.0, 2.0, (n_s, n_t, N_HEAD)).astype(np.float32))
            for xBC, s, dt in ins:
                be.tensor_set(xBC, xv); be.tensor_set(s, sv); be.tensor_set(dt, dv)
            n0 = be.get_stat("ssm_scan_launches")
            us = timed(be, c.graph(), args.reps) / n
            assert be.get_stat("ssm_scan_launches") - n0 in (0, 2 * n)  # eager + capture, every node its own launch (0: a later round found its capture still cached and replayed at once)
            c.free()
            print(f"round {rnd} ssm_scan n_t={n_t:3d} n_s={n_s:2d}: {node_bytes / 1e6:6.1f} MB/launch  {us:8.2f} us ({node_bytes / us / 1e3:7.1f} GB/s, {node_bytes / us / 1e-6 / HBM:5.3f} of 8 TB/s, "
                  f"{n} nodes)  bytes / 8 TB/s {node_bytes / HBM * 1e6:6.2f} us", flush=True)
        for n_t in (1, 512):
            node_bytes = (D_CONV - 1 + n_t) * D_XBC * 4 + n_t * D_XBC * 4 + D_CONV * D_XBC * 4
            n = max(8, min(256, (args.min_mib << 20) // node_bytes + 1))
            c = Context(be)
            w = c.new_tensor(F32, D_CONV, D_XBC)
            sxs = [c.new_tensor(F32, D_CONV - 1 + n_t, D_XBC, 1) for _ in range(n)]
            ys = [c.ssm_conv(sx, w) for sx in sxs]
            assert be.supports_op(ys[0])
            c.alloc()
            be.tensor_set(w, rng.standard_normal((D_XBC, D_CONV)).astype(np.float32))
            xv = rng.standard_normal((1, D_XBC, D_CONV - 1 + n_t)).astype(np.float32)
            for sx in sxs:
                be.tensor_set(sx, xv)
            n0 = be.get_stat("ssm_conv_launches")
            us = timed(be, c.graph(), args.reps) / n
            assert be.get_stat("ssm_conv_launches") - n0 in (0, 2 * n)
            c.free()
            print(f"round {rnd} ssm_conv n_t={n_t:3d} n_s= 1: {node_bytes / 1e6:6.3f} MB/launch  {us:8.2f} us ({node_bytes / us / 1e3:7.1f} GB/s, {node_bytes / us / 1e-6 / HBM:5.3f} of 8 TB/s, "
                  f"{n} nodes)  bytes / 8 TB/s {node_bytes / HBM * 1e6:6.2f} us", flush=True)


if __name__ == "__main__":
    main()
