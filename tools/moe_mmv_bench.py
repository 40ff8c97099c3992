#!/usr/bin/env python3
"""tools/moe_mmv_bench.py -- the three expert launches of one mixture-of-experts layer at the Qwen3-30B-A3B decode shape (128 experts, 8 used, n_embd 2048, expert n_ff 768;
Q4_K gate / up: 8 x 768 x 2048 weights = 7.1 MB per launch, Q6_K down: 8 x 2048 x 768 = 10.3 MB), timed as replayed captures through the backend C-ABI, beside the yardstick:
mmv_kquant_multi (mmvk.hip) on ONE dense matrix of the same bytes and type -- the same mat-vec bodies without the id indirection (options mv1 = 0 and fusion = 0 put a
one-column K-quant MUL_MAT on exactly that launcher, one matrix per launch).

One cgraph holds N MUL_MAT_ID nodes (N x bytes > 768 MiB: the 256 MiB Infinity Cache cannot serve re-reads) over several expert tensors, every node with its own 8 ids
so that no two nodes of a pass read the same expert; all nodes share one activation, whose Q8_K image is made once per pass.  The graph is run eager, captured, then
replayed; the best of --reps replays is reported per node, with the launch's bytes / 8 TB/s.  Three alternating rounds show the run-to-run spread.

--legs blocks: the gate / up launch (8 x 768 x 2048) on experts of the block formats (mmvq.hip k_mmv_blocks_id; --types, default Q8_0 and Q4_0) beside the Q4_K and Q6_K
launches of k_mmv_id at the same shape, each with its dense one-column mat-vec as the yardstick (profiles/moe_blocks_decode.txt).

usage: python tools/moe_mmv_bench.py [--reps 5] [--rounds 3] [--tokens 1] [--legs kquant|blocks] [--types q8_0,q4_0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

Q4_K, Q6_K, F32, I32 = 12, 14, 0, 26
BLOCKS = {"q8_0": 8, "q4_0": 2, "q5_0": 6, "iq4_nl": 20, "q4_1": 3, "q5_1": 7, "iq4_xs": 23, "q2_K": 10, "q3_K": 11}
X, XU, E, F = 128, 8, 2048, 768
HBM = 8.0e12


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
    ap.add_argument("--tokens", type=int, default=1)
    ap.add_argument("--min-mib", type=int, default=768)
    ap.add_argument("--legs", default="kquant", choices=["kquant", "blocks"])
    ap.add_argument("--types", default="q8_0,q4_0")
    args = ap.parse_args()
    pkg = load_pkg()
    from llama_cpp_omni_amd import qwen3
    from llama_cpp_omni_amd.ggml import Context, row_size
    be = pkg.backend(0)
    rng = np.random.default_rng(0)
    T = args.tokens
    # name, type, K, M (rows per expert), launch counter
    legs = [("gate/up Q4_K", Q4_K, E, F, "mmv_id_launches"), ("down    Q6_K", Q6_K, F, E, "mmv_id_launches")]
    if args.legs == "blocks":
        legs = [("gate/up Q4_K", Q4_K, E, F, "mmv_id_launches"), ("gate/up Q6_K", Q6_K, E, F, "mmv_id_launches")]
        legs += [(f"gate/up {t}", BLOCKS[t], E, F, "mmv_id_blocks_launches") for t in args.types.split(",")]
    for rnd in range(args.rounds):
        for name, ty, K, M, stat in legs:
            node_bytes = XU * T * M * row_size(ty, K)
            sets = X // XU                                            # id sets per expert tensor that share no expert
            n_tensors = max(1, ((args.min_mib << 20) // node_bytes + sets) // sets)
            host = qwen3.random_blocks(rng, ty, 1024, K)
            # ---- MUL_MAT_ID
            c = Context(be)
            b = c.new_tensor(F32, K, 1, T)
            ws = [c.new_tensor(ty, K, M, X) for _ in range(n_tensors)]
            ids = c.new_tensor(I32, XU, T, n_tensors * sets)
            ys = []
            for i, w in enumerate(ws):
                for s in range(sets):
                    ys.append(c.mul_mat_id(w, b, c.view_2d(ids, XU, T, ids.nb[1], (i * sets + s) * ids.nb[2])))
            assert be.supports_op(ys[0])
            c.alloc()
            full = np.tile(host, (M * X // 1024, 1))
            for w in ws:
                be.tensor_set(w, full)
            be.tensor_set(b, rng.standard_normal((T, K)).astype(np.float32))
            idv = np.empty((n_tensors * sets, T, XU), np.int32)
            for i in range(n_tensors):
                perm = rng.permutation(X).reshape(sets, 1, XU)
                idv[i * sets:(i + 1) * sets] = np.repeat(perm, T, axis=1)
            be.tensor_set(ids, idv)
            n0 = be.get_stat(stat)
            us_id = timed(be, c.graph(), args.reps) / len(ys)
            assert be.get_stat(stat) - n0 == 2 * len(ys)      # eager + capture: every node its own launch
            c.free()
            # ---- the yardstick: one dense matrix of the same bytes per node, on mmv_kquant_multi (the block formats: on their k_mmv_blocks launch)
            us_dense = float("nan")
            if T == 1:
                be.set_option("mv1", 0); be.set_option("fusion", 0)
                nd = (args.min_mib << 20) // node_bytes + 1
                c = Context(be)
                x = c.new_tensor(F32, K, 1)
                wd = [c.new_tensor(ty, K, M * XU) for _ in range(nd)]
                yd = [c.mul_mat(w, x) for w in wd]
                c.alloc()
                fulld = np.tile(host, (M * XU // 1024, 1))
                for w in wd:
                    be.tensor_set(w, fulld)
                be.tensor_set(x, rng.standard_normal((1, K)).astype(np.float32))
                us_dense = timed(be, c.graph(), args.reps) / nd
                c.free()
                be.set_option("mv1", 1); be.set_option("fusion", 1)
            floor = node_bytes / HBM * 1e6
            print(f"round {rnd} {name} tokens={T}: {node_bytes / 1e6:5.1f} MB/launch  MUL_MAT_ID {us_id:7.2f} us ({node_bytes / us_id / 1e3:7.1f} GB/s, {len(ys)} nodes)  "
                  f"dense mat-vec {us_dense:7.2f} us  ratio {us_id / us_dense:5.2f}  bytes / 8 TB/s {floor:5.2f} us", flush=True)


if __name__ == "__main__":
    main()
