#!/usr/bin/env python3
"""tools/gptoss_mmq_bench.py -- the expert launches of one gpt-oss-20b layer at the PREFILL shape (32 MXFP4 experts, 4 used, K = M = 2880: a gate / up leg with b
broadcast over the slots, a down leg with b per slot) at 65 / 128 / 512 / 2048 tokens, timed as replayed captures through the backend C-ABI on both MUL_MAT_ID paths in
the same process: option mmq_id = 1 (the expert-grouped int8-MFMA kernel, mmq_id.hip: one grouping launch + one matrix launch per node) and mmq_id = 0 (the
per-pair mat-vec, mmv_mxfp4.hip -- the yardstick: the kernel every token count ran on before the grouped path existed).

The grouped path starts at MMQ_ID_MXFP4_MIN_TOKENS = 128 tokens by default; the tool sets MI355X_MMQ_ID_MXFP4_MIN_TOKENS=65 (unless the environment has a value) before
the library loads, so that the 65-token row runs grouped as well: the case for lowering the constant.

One cgraph holds N >= 8 MUL_MAT_ID nodes cycling over several expert tensors (together > --min-mib, default 768 MiB: the 256 MiB Infinity Cache cannot serve a re-read
of a tensor from the previous use), every node with its own ids, drawn uniformly and distinct per token; all nodes share one activation, whose Q8_0 images are made once
per pass.  The graph is run eager, captured, then replayed; the best of --reps replays is reported per node.  The two paths alternate inside every round, --rounds
rounds show the run-to-run spread.  Per leg and token count:
    us per node on both paths (every round, then best and the spread over the rounds), the ratio,
    floor  = the bytes of the DISTINCT experts a node touches / 8 TB/s   (what a launch that reads every touched expert once cannot beat),
    TOP/s  = 2 * pairs * M * K int8 operations per node / the grouped path's time.

usage: python tools/gptoss_mmq_bench.py [--reps 3] [--rounds 3] [--tokens 65,128,512,2048]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

MXFP4, F32, I32 = 39, 0, 26
X, XU, E = 32, 4, 2880
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", default="65,128,512,2048")
    ap.add_argument("--min-mib", type=int, default=768)
    args = ap.parse_args()
    os.environ.setdefault("MI355X_MMQ_ID_MXFP4_MIN_TOKENS", "65")      # read once by the library, at the first MXFP4 route
    pkg = load_pkg()
    from llama_cpp_omni_amd import qwen3
    from llama_cpp_omni_amd.ggml import Context, row_size
    be = pkg.backend(0)
    rng = np.random.default_rng(0)
    min_tokens = int(os.environ["MI355X_MMQ_ID_MXFP4_MIN_TOKENS"])
    print(f"MI355X_MMQ_ID_MXFP4_MIN_TOKENS={min_tokens}  reps {args.reps}  rounds {args.rounds}", flush=True)
    # name, K, M (rows per expert), b broadcast over the slots
    legs = [("gate/up MXFP4", E, E, True), ("down    MXFP4", E, E, False)]
    for name, K, M, bcast in legs:
        tensor_bytes = X * M * row_size(MXFP4, K)
        n_tensors = ((args.min_mib << 20) + tensor_bytes - 1) // tensor_bytes
        n_nodes = max(8, n_tensors)
        host = qwen3.random_blocks(rng, MXFP4, 960, K)
        full = np.tile(host, (M * X // 960, 1))
        for T in [int(t) for t in args.tokens.split(",")]:
            c = Context(be)
            b = c.new_tensor(F32, K, 1 if bcast else XU, T)
            ws = [c.new_tensor(MXFP4, K, M, X) for _ in range(n_tensors)]
            ids = c.new_tensor(I32, XU, T, n_nodes)
            ys = [c.mul_mat_id(ws[i % n_tensors], b, c.view_2d(ids, XU, T, ids.nb[1], i * ids.nb[2])) for i in range(n_nodes)]
            assert be.supports_op(ys[0])
            c.alloc()
            for w in ws:
                be.tensor_set(w, full)
            be.tensor_set(b, rng.standard_normal((T, 1 if bcast else XU, K)).astype(np.float32))
            idv = np.argsort(rng.random((n_nodes, T, X)), axis=-1)[:, :, :XU].astype(np.int32)      # uniform, distinct per token
            be.tensor_set(ids, idv)
            touched = float(np.mean([len(np.unique(idv[i])) for i in range(n_nodes)]))
            floor = touched * M * row_size(MXFP4, K) / HBM * 1e6
            ops = 2.0 * XU * T * M * K
            grouped_runs = T >= min_tokens                            # below the threshold both modes time the per-pair kernel
            us = {1: [], 0: []}
            try:
                for rnd in range(args.rounds):
                    for mode in (1, 0):
                        be.set_option("mmq_id", mode)
                        key = "mmq_id_mxfp4_launches" if mode and grouped_runs else "mmv_id_mxfp4_launches"
                        n0, r0 = be.get_stat(key), be.get_stat("graph_replays")
                        t = timed(be, c.graph(), args.reps) / n_nodes
                        assert be.get_stat(key) - n0 == 2 * n_nodes and be.get_stat("graph_replays") - r0 == 1 + args.reps      # eager + capture ran the launchers, the rest replayed
                        us[mode].append(t)
            finally:
                be.set_option("mmq_id", 1)
            c.free()
            g, p = min(us[1]), min(us[0])
            print(f"{name} tokens={T:5d} pairs={XU * T:6d} experts touched {touched:6.1f}" + ("" if grouped_runs else " (BELOW the threshold: both columns per-pair)") +
                  f": grouped {g:9.2f} us/node (rounds " + " ".join(f"{v:.2f}" for v in us[1]) +
                  f"; spread {100 * (max(us[1]) - g) / g:.1f}%)  per-pair {p:9.2f} us/node (rounds " + " ".join(f"{v:.2f}" for v in us[0]) + f"; spread {100 * (max(us[0]) - p) / p:.1f}%)  "
                  f"per-pair / grouped {p / g:6.2f}  floor {floor:6.2f} us (grouped = {g / floor:5.2f} x)  int8 {ops / g / 1e6:7.1f} TOP/s", flush=True)


if __name__ == "__main__":
    main()
