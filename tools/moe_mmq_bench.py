#!/usr/bin/env python3
"""tools/moe_mmq_bench.py -- the expert launches of one mixture-of-experts layer at the Qwen3-30B-A3B PREFILL shape (128 experts, 8 used, n_embd 2048, expert n_ff 768;
Q4_K gate / up: K 2048, M 768; Q6_K down: K 768, M 2048) at 64 / 128 / 512 / 2048 tokens, timed as replayed captures through the backend C-ABI on both MUL_MAT_ID paths
in the same process: option mmq_id = 1 (the expert-grouped int8-MFMA kernel, mmq_id.hip: one grouping launch + one matrix launch per node) and mmq_id = 0 (the per-pair
mat-vec, mmvk.hip k_mmv_id -- the yardstick: the kernel every token count ran on before the grouped path existed).

One cgraph holds N >= 8 MUL_MAT_ID nodes cycling over several expert tensors (together > --min-mib, default 768 MiB: the 256 MiB Infinity Cache cannot serve a re-read
of a tensor from the previous use), every node with its own ids, drawn uniformly and distinct per token; all nodes share one activation, whose Q8_K images are made once
per pass.  The graph is run eager, captured, then replayed; the best of --reps replays is reported per node.  The two paths alternate inside every round, --rounds
rounds show the run-to-run spread.  Per leg and token count:
    us per node on both paths (every round, then best and the spread over the rounds), the ratio,
    floor  = the bytes of the DISTINCT experts a node touches / 8 TB/s   (what a launch that reads every touched expert once cannot beat),
    TOP/s  = 2 * pairs * M * K int8 operations per node / the grouped path's time.
MI355X_MMQ_ID_NT4=1 in the environment keeps every tile of the grouped kernel on the four-column-group body (the measurement behind the per-tile branch).

--legs blocks: the same for Q8_0 / Q4_0 / Q5_0 / IQ4_NL experts (mmq_id.hip against mmvq.hip k_mmv_blocks_id), at the Qwen3-30B-A3B gate / up shape and at the
DeepSeek-V2-Lite down shape (64 experts, 6 used, K 1408, M 2048); --types picks among the four.  MI355X_MMQ_ID_BLOCKS_MIN_TOKENS=65 in the environment puts every token
count from 65 on the grouped path (the crossover measurement behind MMQ_ID_BLOCKS_MIN_TOKENS, profiles/moe_blocks_crossover.txt).

usage: python tools/moe_mmq_bench.py [--reps 3] [--rounds 3] [--tokens 64,128,512,2048] [--legs kquant|blocks] [--types q8_0,q4_0,q5_0,iq4_nl]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

Q4_K, Q6_K, F32, I32 = 12, 14, 0, 26
BLOCKS = {"q8_0": 8, "q4_0": 2, "q5_0": 6, "iq4_nl": 20}
E, F = 2048, 768
KQ_STATS, BL_STATS = ("mmq_id_launches", "mmv_id_launches"), ("mmq_id_blocks_launches", "mmv_id_blocks_launches")      # (grouped, per-pair) launch counters
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
    ap.add_argument("--tokens", default="64,128,512,2048")
    ap.add_argument("--min-mib", type=int, default=768)
    ap.add_argument("--legs", default="kquant", choices=["kquant", "blocks"])
    ap.add_argument("--types", default="q8_0,q4_0,q5_0,iq4_nl")
    args = ap.parse_args()
    pkg = load_pkg()
    from llama_cpp_omni_amd import qwen3
    from llama_cpp_omni_amd.ggml import Context, row_size
    be = pkg.backend(0)
    rng = np.random.default_rng(0)
    print(f"MI355X_MMQ_ID_NT4={os.environ.get('MI355X_MMQ_ID_NT4', '0')}  reps {args.reps}  rounds {args.rounds}", flush=True)
    # name, type, K, M (rows per expert), b broadcast over the slots, experts, experts used, (grouped, per-pair) counters
    legs = [("gate/up Q4_K", Q4_K, E, F, True, 128, 8, KQ_STATS), ("down    Q6_K", Q6_K, F, E, False, 128, 8, KQ_STATS)]
    if args.legs == "blocks":
        legs = []
        for t in args.types.split(","):
            legs += [(f"qwen3-30b-a3b gate/up {t}", BLOCKS[t], E, F, True, 128, 8, BL_STATS), (f"deepseek-v2-lite down {t}", BLOCKS[t], 1408, 2048, False, 64, 6, BL_STATS)]
    for name, ty, K, M, bcast, X, XU, stats in legs:
        tensor_bytes = X * M * row_size(ty, K)
        n_tensors = ((args.min_mib << 20) + tensor_bytes - 1) // tensor_bytes
        n_nodes = max(8, n_tensors)
        host = qwen3.random_blocks(rng, ty, 1024, K)
        full = np.tile(host, (M * X // 1024, 1))
        for T in [int(t) for t in args.tokens.split(",")]:
            c = Context(be)
            b = c.new_tensor(F32, K, 1 if bcast else XU, T)
            ws = [c.new_tensor(ty, K, M, X) for _ in range(n_tensors)]
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
            floor = touched * M * row_size(ty, K) / HBM * 1e6
            ops = 2.0 * XU * T * M * K
            us = {1: [], 0: []}
            try:
                for rnd in range(args.rounds):
                    for mode in (1, 0):
                        be.set_option("mmq_id", mode)
                        key = stats[0] if mode else stats[1]
                        n0, r0 = be.get_stat(key), be.get_stat("graph_replays")
                        t = timed(be, c.graph(), args.reps) / n_nodes
                        assert be.get_stat(key) - n0 == 2 * n_nodes and be.get_stat("graph_replays") - r0 == 1 + args.reps, key      # eager + capture ran the launchers (a token count under the path's threshold trips this), the rest replayed
                        us[mode].append(t)
            finally:
                be.set_option("mmq_id", 1)
            c.free()
            g, p = min(us[1]), min(us[0])
            print(f"{name} tokens={T:5d} pairs={XU * T:6d} experts touched {touched:6.1f}: grouped {g:9.2f} us/node (rounds " + " ".join(f"{v:.2f}" for v in us[1]) +
                  f"; spread {100 * (max(us[1]) - g) / g:.1f}%)  per-pair {p:9.2f} us/node (rounds " + " ".join(f"{v:.2f}" for v in us[0]) + f"; spread {100 * (max(us[0]) - p) / p:.1f}%)  "
                  f"per-pair / grouped {p / g:6.2f}  floor {floor:6.2f} us (grouped = {g / floor:5.2f} x)  int8 {ops / g / 1e6:7.1f} TOP/s", flush=True)


if __name__ == "__main__":
    main()
