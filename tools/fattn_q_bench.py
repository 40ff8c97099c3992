#!/usr/bin/env python3
"""tools/fattn_q_bench.py -- FLASH_ATTN_EXT over a quantised KV cache at Qwen3-8B's attention widths (32 heads over 8 KV heads of 128): the generic kernel
(option "fattn_q" = 0, fattn_any.hip) against k_fattn_q (= 1, fattn_q.hip), in one process, alternating.

The method is tools/fattn_wide_bench.py's: a graph of N FLASH_ATTN_EXT nodes, each on its own K / V set (so that decode shapes stream from HBM, not from the
256 MB cache), timed with the backend's timed events around graph_compute; per node time = window / N.  Per shape and option: two warm-up runs after the option
is set (it drops captured graphs), then the windows alternate 0, 1, 0, 1 ...; the median per option is reported with the spread (min .. max).  Decode rows
report the K + V bytes (read once per KV head) over the time against the 8.0 TB/s HBM3E specification; prefill rows the visible (row, cell) pairs per second.

    python tools/fattn_q_bench.py [-o profiles/fattn_q.txt] [--type q8_0|q4_0] [--budget-s 0.3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

HBM_SPEC = 8.0e12
D, NH, NHKV = 128, 32, 8
# (tokens, cache rows, causal)
SHAPES = [(1, 4096, False), (1, 32768, False), (512, 512, True), (512, 8192, True)]


def one_shape(be, kv_type, nq, nkv, causal, budget_s, emit):
    from llama_cpp_omni_amd.ggml import GGML_TYPE_F16, GGML_TYPE_F32, Context
    T, bb = (8, 34) if kv_type == "q8_0" else (2, 18)
    kv_bytes = 2 * nkv * NHKV * (D // 32) * bb
    nsets = int(min(48, max(2, -(-600e6 // kv_bytes)))) if nq == 1 else 2
    c = Context(be)
    q = c.new_tensor(GGML_TYPE_F32, D, nq, NH)
    m = c.new_tensor(GGML_TYPE_F16, nkv, (nq + 63) // 64 * 64)
    sets = [(c.new_tensor(T, D, nkv, NHKV), c.new_tensor(T, D, nkv, NHKV)) for _ in range(nsets)]
    outs = [c.flash_attn_ext(q, k, v, m, 1.0 / np.sqrt(D)) for k, v in sets]
    c.alloc()
    rng = np.random.default_rng(0)
    be.tensor_set(q, rng.standard_normal(q.nelements()).astype(np.float32))
    mk = np.zeros((m.ne[1], nkv), np.float16)
    pairs = nq * nkv
    if causal:
        pairs = 0
        for t in range(m.ne[1]):
            last = nkv - nq + min(t, nq - 1)
            mk[t, last + 1:] = -np.inf
            pairs += (last + 1) if t < nq else 0
    be.tensor_set(m, mk)
    blocks = np.zeros((nkv * NHKV * (D // 32), bb), np.uint8)           # random quants under one finite scale per block
    blocks[:, :2] = rng.uniform(0.005, 0.02, len(blocks)).astype(np.float16)[:, None].view(np.uint8)
    blocks[:, 2:] = rng.integers(0, 256, (len(blocks), bb - 2), dtype=np.uint8)
    for k, v in sets:
        be.tensor_set(k, blocks); be.tensor_set(v, blocks)
    g = c.graph()

    def window():
        a, b = be.timed_event(), be.timed_event()
        be.record(a); be.graph_compute(g); be.record(b)
        return be.elapsed_ms(a, b) * 1e3 / nsets                       # us per node

    times, outv, launches = {0: [], 1: []}, {}, {}
    for mode in (0, 1):                                                 # warm-up, a first estimate, and the outputs for the parity figure
        be.set_option("fattn_q", mode)
        n0 = be.get_stat("fattn_q_launches")
        be.graph_compute(g)
        launches[mode] = int(be.get_stat("fattn_q_launches") - n0)
        be.graph_compute(g); be.synchronize()
        outv[mode] = be.tensor_get(outs[-1]).astype(np.float64)
        times[mode].append(window())
    reps = {mode: int(min(40, max(3, budget_s * 1e6 / (times[mode][0] * nsets)))) for mode in (0, 1)}
    for i in range(max(reps.values())):
        for mode in (0, 1):
            if i >= reps[mode]:
                continue
            be.set_option("fattn_q", mode)
            be.graph_compute(g); be.graph_compute(g); be.synchronize()
            times[mode].append(window())
    be.set_option("fattn_q", -1)
    c.free()
    nm = float(((outv[1] - outv[0]) ** 2).sum() / (outv[0] ** 2).sum())
    t0, t1 = float(np.median(times[0])), float(np.median(times[1]))
    if nq == 1:
        rate = f"K+V {kv_bytes / 1e6:.1f} MB: {kv_bytes / t0 / 1e6:7.3f} -> {kv_bytes / t1 / 1e6:7.3f} TB/s = {100 * kv_bytes / (t1 * 1e-6) / HBM_SPEC:5.1f} % of 8.0 TB/s"
    else:
        rate = f"{pairs * NH / 1e6:.1f} M (row, cell, head) pairs: {pairs * NH / t0:7.1f} -> {pairs * NH / t1:7.1f} per us"
    emit(f"{kv_type} {NH}/{NHKV} x {D} {nq:4d} x {nkv:6d}{' causal' if causal else '       '}: generic {t0:10.1f} us [{min(times[0]):.1f} .. {max(times[0]):.1f}, n={len(times[0])}]  "
         f"k_fattn_q {t1:9.1f} us [{min(times[1]):.1f} .. {max(times[1]):.1f}, n={len(times[1])}]  ratio {t0 / t1:7.1f}x  {rate}  "
         f"(k_fattn_q launches per graph {launches[1]} / {nsets} nodes, with the option off {launches[0]}; NMSE between the two {nm:.2e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=None)
    ap.add_argument("--type", default="q8_0", choices=["q8_0", "q4_0"])
    ap.add_argument("--budget-s", type=float, default=0.3, help="timed work per shape and option")
    args = ap.parse_args()
    be = load_pkg().backend(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.o:
            with open(args.o, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# tools/fattn_q_bench.py on {be.name()} ({be.description()})")
    emit("# us per FLASH_ATTN_EXT node, median of the windows [min .. max, n]; generic = option fattn_q 0 (fattn_any.hip), k_fattn_q = 1 (fattn_q.hip)")
    for nq, nkv, causal in SHAPES:
        one_shape(be, args.type, nq, nkv, causal, args.budget_s, emit)


if __name__ == "__main__":
    main()
