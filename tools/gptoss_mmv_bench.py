#!/usr/bin/env python3
"""tools/gptoss_mmv_bench.py -- the MXFP4 expert launch of a gpt-oss-20b layer at the decode shape (32 experts, 4 used, 2880 x 2880: 4 x 2880 rows of 1530 bytes = 17.6 MB
per launch), timed as replayed captures through the backend C-ABI, beside the yardstick: the dense IQ4_NL mat-vec kernel (mmvq.hip mmv_iq4_nl) on ONE matrix of the same
row count and K -- the same arithmetic (a 16-entry int8 table against Q8_0 images) on 18-byte, 2-byte aligned blocks without the id indirection.  A sibling of
tools/moe_mmv_bench.py, built the same way: one cgraph holds N nodes (N x bytes > 768 MiB: the 256 MiB Infinity Cache cannot serve re-reads), every MUL_MAT_ID node with
its own 4 ids so that no two nodes of a pass read the same expert; the graph is run eager, captured, then replayed; the best of --reps replays is reported per node,
with time per weight byte, the ratio of the two and the launch's bytes / 8 TB/s.  Three alternating rounds show the run-to-run spread.

usage: python tools/gptoss_mmv_bench.py [--reps 5] [--rounds 3] [--tokens 1]        (MI355X_MXFP4_U=1|2 picks the kernel's steps per stage)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402
from moe_mmv_bench import timed  # noqa: E402

MXFP4, IQ4_NL, F32, I32 = 39, 20, 0, 26
X, XU, K, M = 32, 4, 2880, 2880
HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=1)
    ap.add_argument("--min-mib", type=int, default=768)
    args = ap.parse_args()
    pkg = load_pkg()
    from llama_cpp_omni_amd import qwen3
    from llama_cpp_omni_amd.ggml import Context, row_size
    be = pkg.backend(0)
    rng = np.random.default_rng(0)
    T = args.tokens
    for rnd in range(args.rounds):
        # ---- MUL_MAT_ID on MXFP4 experts
        node_bytes = XU * T * M * row_size(MXFP4, K)
        sets = X // XU                                                # id sets per expert tensor that share no expert
        n_tensors = max(1, ((args.min_mib << 20) // node_bytes + sets) // sets)
        host = qwen3.random_blocks(rng, MXFP4, 1152, K)
        c = Context(be)
        b = c.new_tensor(F32, K, 1, T)
        ws = [c.new_tensor(MXFP4, K, M, X) for _ in range(n_tensors)]
        ids = c.new_tensor(I32, XU, T, n_tensors * sets)
        ys = []
        for i, w in enumerate(ws):
            for s in range(sets):
                ys.append(c.mul_mat_id(w, b, c.view_2d(ids, XU, T, ids.nb[1], (i * sets + s) * ids.nb[2])))
        assert be.supports_op(ys[0])
        c.alloc()
        full = np.tile(host, (M * X // 1152, 1))
        for w in ws:
            be.tensor_set(w, full)
        be.tensor_set(b, rng.standard_normal((T, K)).astype(np.float32))
        idv = np.empty((n_tensors * sets, T, XU), np.int32)
        for i in range(n_tensors):
            perm = rng.permutation(X).reshape(sets, 1, XU)
            idv[i * sets:(i + 1) * sets] = np.repeat(perm, T, axis=1)
        be.tensor_set(ids, idv)
        n0 = be.get_stat("mmv_id_mxfp4_launches")
        us_id = timed(be, c.graph(), args.reps) / len(ys)
        assert be.get_stat("mmv_id_mxfp4_launches") - n0 == 2 * len(ys)      # eager + capture: every node its own launch
        c.free()
        # ---- the yardstick: one dense IQ4_NL matrix of the same row count and K per node
        us_dense, dense_bytes = float("nan"), XU * M * row_size(IQ4_NL, K)
        if T == 1:
            be.set_option("mv1", 0); be.set_option("fusion", 0)
            nd = (args.min_mib << 20) // dense_bytes + 1
            hostd = qwen3.random_blocks(rng, IQ4_NL, 1152, K)
            c = Context(be)
            x = c.new_tensor(F32, K, 1)
            wd = [c.new_tensor(IQ4_NL, K, M * XU) for _ in range(nd)]
            yd = [c.mul_mat(w, x) for w in wd]
            c.alloc()
            fulld = np.tile(hostd, (M * XU // 1152, 1))
            for w in wd:
                be.tensor_set(w, fulld)
            be.tensor_set(x, rng.standard_normal((1, K)).astype(np.float32))
            n0 = be.get_stat("mmv_iq4nl_launches")
            us_dense = timed(be, c.graph(), args.reps) / nd
            assert be.get_stat("mmv_iq4nl_launches") - n0 == 2 * nd
            c.free()
            be.set_option("mv1", 1); be.set_option("fusion", 1)
        per_id, per_dense = us_id / node_bytes, us_dense / dense_bytes
        print(f"round {rnd} MXFP4 experts tokens={T}: {node_bytes / 1e6:5.1f} MB/launch  MUL_MAT_ID {us_id:7.2f} us ({node_bytes / us_id / 1e3:7.1f} GB/s, {len(ys)} nodes)  "
              f"dense mmv_iq4_nl {dense_bytes / 1e6:5.1f} MB {us_dense:7.2f} us ({dense_bytes / us_dense / 1e3:7.1f} GB/s)  time per weight byte ratio {per_id / per_dense:5.3f}  "
              f"bytes / 8 TB/s {node_bytes / HBM * 1e6:5.2f} us", flush=True)


if __name__ == "__main__":
    main()
