#!/usr/bin/env python3
"""tools/fattn_wide_bench.py -- FLASH_ATTN_EXT at head sizes 256 / 256 (Gemma-2-9B-like: 16 heads over 8 KV heads) and 576 / 512 (DeepSeek MLA: 128 heads
over 1 KV head), and at 96 / 96 (Phi-3-mini: 32 / 32), 192 / 128 (DeepSeek-V2-Lite: 16 / 16), 80 / 80 and 112 / 112: the generic kernel (option "fattn_wide" = 0, fattn_any.hip) against k_fattn_wide (= 1), in one process, alternating.

Single-node graphs' worth of work through the C-ABI: a graph of N FLASH_ATTN_EXT nodes, each on its own K / V set (so that decode shapes stream from HBM, not
from the 256 MB cache), timed with the backend's timed events around graph_compute; per node time = window / N.  Per shape and option: two warm-up runs after
the option is set (it drops captured graphs), then the windows alternate 0, 1, 0, 1 ...; the median per option is reported, with the spread (min .. max).
Decode rows report the K + V bytes (read once per KV head) over the time, against the 8.0 TB/s HBM3E specification (6.29 TB/s is what a copy kernel reaches);
prefill rows report 2 * (DK + DV) * visible (row, cell) pairs * heads FLOP over the time against 2.5 PFLOP/s dense F16.

    python tools/fattn_wide_bench.py [-o profiles/fattn_wide.txt] [--only gemma,mla,phi3,v2lite,h80,h112] [--budget-s 0.4]

Against another build of the library (MI355X_LIB=path: the parent commit's, say) both columns are what that build runs at the shape; for the head sizes it does not
have on fattn_wide.hip that is its generic kernel twice ("launches per graph 0").
"""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_pkg  # noqa: E402

HBM_SPEC, F16_PEAK = 8.0e12, 2.5e15

# (label, DK, DV, heads, KV heads, tokens, cache rows, causal)
SHAPES = [
    ("gemma 256/256 16/8", 256, 256, 16, 8, 1, 64, False),             # (one token over a shallow cache: the class the plan would drop if it were slower)
    ("gemma 256/256 16/8", 256, 256, 16, 8, 1, 512, False),
    ("gemma 256/256 16/8", 256, 256, 16, 8, 1, 4096, False),
    ("gemma 256/256 16/8", 256, 256, 16, 8, 1, 32768, False),
    ("gemma 256/256 16/8", 256, 256, 16, 8, 512, 512, True),
    ("gemma 256/256 16/8", 256, 256, 16, 8, 512, 4096, True),
    ("mla 576/512 128/1", 576, 512, 128, 1, 1, 64, False),
    ("mla 576/512 128/1", 576, 512, 128, 1, 1, 512, False),
    ("mla 576/512 128/1", 576, 512, 128, 1, 1, 4096, False),
    ("mla 576/512 128/1", 576, 512, 128, 1, 1, 32768, False),
    ("mla 576/512 128/1", 576, 512, 128, 1, 512, 512, True),
    # the head sizes that are no multiple of the MFMA extents: Phi-3-mini (96, 32 heads, no GQA), DeepSeek-V2-Lite before the absorption (192 / 128, 16 heads),
    # and 80 (Phi-2) and 112 at the prefill shape
    ("phi3 96/96 32/32", 96, 96, 32, 32, 512, 512, True),
    ("phi3 96/96 32/32", 96, 96, 32, 32, 1, 512, False),
    ("phi3 96/96 32/32", 96, 96, 32, 32, 1, 4096, False),
    ("phi3 96/96 32/32", 96, 96, 32, 32, 1, 32768, False),
    ("v2lite 192/128 16/16", 192, 128, 16, 16, 512, 512, True),
    ("v2lite 192/128 16/16", 192, 128, 16, 16, 1, 512, False),
    ("v2lite 192/128 16/16", 192, 128, 16, 16, 1, 4096, False),
    ("v2lite 192/128 16/16", 192, 128, 16, 16, 1, 32768, False),
    ("h80 80/80 32/32", 80, 80, 32, 32, 512, 512, True),
    ("h112 112/112 32/32", 112, 112, 32, 32, 512, 512, True),
]


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        keep = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(keep) if keep else "clocks: not reported"
    except Exception as e:                                             # noqa: BLE001
        return f"clocks: not read ({type(e).__name__})"


def one_shape(pkg, be, shape, budget_s, emit):
    from llama_cpp_omni_amd.ggml import GGML_TYPE_F16, GGML_TYPE_F32, Context
    label, DK, DV, nh, nhkv, nq, nkv, causal = shape
    kv_bytes = nkv * nhkv * (DK + DV) * 2
    nsets = int(min(48, max(2, -(-600e6 // kv_bytes)))) if nq == 1 else 2
    c = Context(be)
    q = c.new_tensor(GGML_TYPE_F32, DK, nq, nh)
    m = c.new_tensor(GGML_TYPE_F16, nkv, (nq + 63) // 64 * 64)
    sets = [(c.new_tensor(GGML_TYPE_F16, DK, nkv, nhkv), c.new_tensor(GGML_TYPE_F16, DV, nkv, nhkv)) for _ in range(nsets)]
    outs = [c.flash_attn_ext(q, k, v, m, 1.0 / np.sqrt(DK)) for k, v in sets]
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
    kk = (rng.standard_normal(sets[0][0].nelements()) * 0.3).astype(np.float16)
    vv = (rng.standard_normal(sets[0][1].nelements()) * 0.5).astype(np.float16)
    for k, v in sets:
        be.tensor_set(k, kk); be.tensor_set(v, vv)
    g = c.graph()

    def window():
        a, b = be.timed_event(), be.timed_event()
        be.record(a); be.graph_compute(g); be.record(b)
        return be.elapsed_ms(a, b) * 1e3 / nsets                       # us per node

    times, outv, launches = {0: [], 1: []}, {}, {}
    for mode in (0, 1):                                                 # warm-up, a first estimate, and the outputs for the parity figure
        be.set_option("fattn_wide", mode)
        n0 = be.get_stat("fattn_wide_launches")
        be.graph_compute(g)
        launches[mode] = int(be.get_stat("fattn_wide_launches") - n0)
        be.graph_compute(g); be.synchronize()
        outv[mode] = be.tensor_get(outs[-1]).astype(np.float64)
        times[mode].append(window())
    reps = {mode: int(min(40, max(3, budget_s * 1e6 / (times[mode][0] * nsets)))) for mode in (0, 1)}
    for i in range(max(reps.values())):
        for mode in (0, 1):
            if i >= reps[mode]:
                continue
            be.set_option("fattn_wide", mode)
            be.graph_compute(g); be.graph_compute(g); be.synchronize()
            times[mode].append(window())
    be.set_option("fattn_wide", -1)
    c.free()
    nm = float(((outv[1] - outv[0]) ** 2).sum() / (outv[0] ** 2).sum())
    t0, t1 = float(np.median(times[0])), float(np.median(times[1]))
    if nq == 1:
        rate = f"K+V {kv_bytes / 1e6:.1f} MB: {kv_bytes / t0 / 1e6:7.3f} -> {kv_bytes / t1 / 1e6:7.3f} TB/s = {100 * kv_bytes / (t1 * 1e-6) / HBM_SPEC:5.1f} % of 8.0 TB/s"
    else:
        fl = 2.0 * (DK + DV) * pairs * nh
        rate = f"{fl / 1e9:.1f} GFLOP: {fl / t0 / 1e6:7.2f} -> {fl / t1 / 1e6:7.2f} TFLOP/s = {100 * fl / (t1 * 1e-6) / F16_PEAK:5.1f} % of 2.5 PFLOP/s"
    emit(f"{label} {nq:4d} x {nkv:6d}{' causal' if causal else '       '}: generic {t0:10.1f} us [{min(times[0]):.1f} .. {max(times[0]):.1f}, n={len(times[0])}]  "
         f"wide {t1:9.1f} us [{min(times[1]):.1f} .. {max(times[1]):.1f}, n={len(times[1])}]  ratio {t0 / t1:7.1f}x  {rate}  "
         f"(k_fattn_wide launches per graph {launches[1]} / {nsets} nodes, with the option off {launches[0]}; wide vs generic NMSE {nm:.2e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=None)
    ap.add_argument("--only", default="")
    ap.add_argument("--budget-s", type=float, default=0.4, help="timed work per shape and option")
    args = ap.parse_args()
    pkg = load_pkg()
    be = pkg.backend(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.o:
            with open(args.o, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# tools/fattn_wide_bench.py on {be.name()} ({be.description()}); {clocks()}")
    emit("# us per FLASH_ATTN_EXT node, median of the windows [min .. max, n]; generic = option fattn_wide 0 (fattn_any.hip), wide = 1 (fattn_wide.hip)")
    for sh in SHAPES:
        if args.only and not sh[0].startswith(tuple(args.only.split(","))):
            continue
        one_shape(pkg, be, sh, args.budget_s, emit)
    emit(f"# after: {clocks()}")


if __name__ == "__main__":
    main()
