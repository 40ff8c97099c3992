#!/usr/bin/env python3
"""tools/fattn_qx_bench.py -- FLASH_ATTN_EXT over mixed K / V cache types at Qwen3-8B's attention widths (32 heads over 8 KV heads of 128): the generic kernel
(option "fattn_qx" = 0, fattn_any.hip) against k_fattn_qx (= 1, fattn_qx.hip) for the pairs q8_0 / f16, q8_0 / q4_0 and q5_1 / q5_1, and k_fattn_q on
q8_0 / q8_0 at the same shapes (what the f32 V tile costs or saves against the int8 V tile), in one process, alternating.

The method is tools/fattn_q_bench.py's: a graph of N FLASH_ATTN_EXT nodes, each on its own K / V set, timed with the backend's timed events around
graph_compute; per node time = window / N; two warm-up runs after an option is set (it drops captured graphs), then the windows alternate; the median is
reported with the spread (min .. max).

    python tools/fattn_qx_bench.py [-o profiles/fattn_qx.txt] [--budget-s 0.3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

D, NH, NHKV = 128, 32, 8
SHAPES = [(1, 4096, False), (512, 4096, True)]          # (tokens, cache rows, causal)
PAIRS = [("q8_0", "f16"), ("q8_0", "q4_0"), ("q5_1", "q5_1"), ("q8_0", "q8_0")]
# type: (ggml id, bytes per 32 elements, f16 header fields)
TYPES = {"f16": (1, 64, 0), "q4_0": (2, 18, 1), "q5_1": (7, 24, 2), "q8_0": (8, 34, 1)}


def fill(rng, t, nkv):
    """random quants under finite block headers (d, m in 0.005 .. 0.02); F16: unit normals"""
    _, bb, nhdr = TYPES[t]
    if t == "f16":
        return rng.standard_normal((nkv * NHKV, D)).astype(np.float16)
    blocks = rng.integers(0, 256, (nkv * NHKV * (D // 32), bb), dtype=np.uint8)
    blocks[:, :2 * nhdr] = rng.uniform(0.005, 0.02, (len(blocks), nhdr)).astype(np.float16).view(np.uint8)
    return blocks


def one_shape(be, kt, vt, nq, nkv, causal, budget_s, emit):
    from llama_cpp_omni_amd.ggml import GGML_TYPE_F16, GGML_TYPE_F32, Context
    opt = "fattn_q" if kt == vt == "q8_0" else "fattn_qx"
    kv_bytes = nkv * NHKV * (D // 32) * (TYPES[kt][1] + TYPES[vt][1])
    nsets = int(min(48, max(2, -(-600e6 // kv_bytes)))) if nq == 1 else 2
    c = Context(be)
    q = c.new_tensor(GGML_TYPE_F32, D, nq, NH)
    m = c.new_tensor(GGML_TYPE_F16, nkv, (nq + 63) // 64 * 64)
    sets = [(c.new_tensor(TYPES[kt][0], D, nkv, NHKV), c.new_tensor(TYPES[vt][0], D, nkv, NHKV)) for _ in range(nsets)]
    outs = [c.flash_attn_ext(q, k, v, m, 1.0 / np.sqrt(D)) for k, v in sets]
    c.alloc()
    rng = np.random.default_rng(0)
    be.tensor_set(q, rng.standard_normal(q.nelements()).astype(np.float32))
    mk = np.zeros((m.ne[1], nkv), np.float16)
    if causal:
        for t in range(m.ne[1]):
            mk[t, nkv - nq + min(t, nq - 1) + 1:] = -np.inf
    be.tensor_set(m, mk)
    kb, vb = fill(rng, kt, nkv), fill(rng, vt, nkv)
    for k, v in sets:
        be.tensor_set(k, kb); be.tensor_set(v, vb)
    g = c.graph()

    def window():
        a, b = be.timed_event(), be.timed_event()
        be.record(a); be.graph_compute(g); be.record(b)
        return be.elapsed_ms(a, b) * 1e3 / nsets                       # us per node

    times, outv, launches = {0: [], 1: []}, {}, {}
    for mode in (0, 1):                                                 # warm-up, a first estimate, and the outputs for the parity figure
        be.set_option(opt, mode)
        n0 = be.get_stat(opt + "_launches")
        be.graph_compute(g)
        launches[mode] = int(be.get_stat(opt + "_launches") - n0)
        be.graph_compute(g); be.synchronize()
        outv[mode] = be.tensor_get(outs[-1]).astype(np.float64)
        times[mode].append(window())
    reps = {mode: int(min(40, max(3, budget_s * 1e6 / (times[mode][0] * nsets)))) for mode in (0, 1)}
    for i in range(max(reps.values())):
        for mode in (0, 1):
            if i >= reps[mode]:
                continue
            be.set_option(opt, mode)
            be.graph_compute(g); be.graph_compute(g); be.synchronize()
            times[mode].append(window())
    be.set_option(opt, -1)
    c.free()
    nm = float(((outv[1] - outv[0]) ** 2).sum() / (outv[0] ** 2).sum())
    t0, t1 = float(np.median(times[0])), float(np.median(times[1]))
    rate = f"K+V {kv_bytes / 1e6:.1f} MB: {kv_bytes / t1 / 1e6:6.3f} TB/s" if nq == 1 else ""
    emit(f"{kt:>5} / {vt:<5} {nq:4d} x {nkv:5d}{' causal' if causal else '       '}: generic {t0:10.1f} us [{min(times[0]):.1f} .. {max(times[0]):.1f}, n={len(times[0])}]  "
         f"k_{opt} {t1:9.1f} us [{min(times[1]):.1f} .. {max(times[1]):.1f}, n={len(times[1])}]  ratio {t0 / t1:7.1f}x  {rate}  "
         f"({opt}_launches per graph {launches[1]} / {nsets} nodes, with the option off {launches[0]}; NMSE between the two {nm:.2e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=None)
    ap.add_argument("--budget-s", type=float, default=0.3, help="timed work per shape, pair and option")
    args = ap.parse_args()
    be = load_pkg().backend(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.o:
            with open(args.o, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# tools/fattn_qx_bench.py on {be.name()} ({be.description()})")
    emit(f"# {NH} heads / {NHKV} KV heads x {D}; us per FLASH_ATTN_EXT node, median of the windows [min .. max, n]; generic = the option at 0 (fattn_any.hip); the q8_0 / q8_0 rows run k_fattn_q (option fattn_q)")
    for nq, nkv, causal in SHAPES:
        for kt, vt in PAIRS:
            one_shape(be, kt, vt, nq, nkv, causal, args.budget_s, emit)


if __name__ == "__main__":
    main()
