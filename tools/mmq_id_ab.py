#!/usr/bin/env python3
"""tools/mmq_id_ab.py PARENT_LIB [OUT_DIR] -- do the expert-grouped MUL_MAT_ID kernels (k_mmq_id<Body, KS, NT4>, mmq_id.hip) of this tree compute the very
bits the parent library's kernels compute?  One fresh child process per library (MI355X_LIB selects it), each under its own time limit, runs MUL_MAT_ID for
every one of the eight grouped types on shapes of the test tables (M = 70 rows; a 33 / 31 / 32-pair "edges" grouping and a ragged one; K with a ragged last
step; KS = 1, 4 and 8), fixed seeds, and writes the raw outputs and the KS of every launch to an .npz; the two files are then compared byte for byte.  The
parent runs first; if its child fails, this tree's is not started.  Exit status 0: no byte differs.

PARENT_LIB is libggml-mi355x.so built from the parent commit in a git worktree (tools/launch_log_ab.sh shows how)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = 0, 26
# name: (type id, the family's KS stat, [(experts, used, T, M, K)])
STEPPED = [(8, 2, 128, 70, 288), (8, 2, 161, 70, 288), (8, 2, 128, 70, 2880), (8, 2, 161, 70, 7968)]
KQUANT = [(8, 2, 64, 70, 768), (8, 2, 97, 70, 2304), (8, 2, 64, 70, 4096)]
TYPES = {"q4_K": (12, "mmq_id", KQUANT), "q5_K": (13, "mmq_id", KQUANT), "q6_K": (14, "mmq_id", KQUANT), "mxfp4": (39, "mmq_id_mxfp4", STEPPED),
         "q8_0": (8, "mmq_id_blocks", STEPPED), "q4_0": (2, "mmq_id_blocks", STEPPED), "q5_0": (6, "mmq_id_blocks", STEPPED), "iq4_nl": (20, "mmq_id_blocks", STEPPED)}


def ids_of(n_expert, n_used, T):
    """T = 64 / 128: 33 + 31 (+ 64) pairs in slot 0, 32 + the rest on the last expert in slot 1; else slot s: runs of 1, 2, 3, ... tokens on experts s, s + 1, ..."""
    sel = np.empty((T, n_used), np.int32)
    if T in (64, 128):
        sel[:33, 0] = 0; sel[33:64, 0] = 1; sel[64:, 0] = 3
        sel[:32, 1] = 2; sel[32:, 1] = n_expert - 1
    else:
        for s in range(n_used):
            t, run, e = 0, 1, s
            while t < T:
                sel[t:t + run, s] = e % n_expert
                t += run; run += 1; e += 1
    return sel


def child(out):
    sys.path.insert(0, ROOT)
    from bench import load_pkg
    pkg = load_pkg()
    from llama_cpp_omni_amd import qwen3
    be = pkg.backend(0)
    res = {}
    for name, (ty, stat, shapes) in TYPES.items():
        for n_expert, n_used, T, M, K in shapes:
            rng = np.random.default_rng(ty * 100000 + T + K)
            wv = qwen3.random_blocks(rng, ty, M * n_expert, K, std=0.05)
            bv = rng.standard_normal((T, n_used, K)).astype(np.float32)
            c = pkg.Context(be)
            as_, b, ids = c.new_tensor(ty, K, M, n_expert), c.new_tensor(F32, K, n_used, T), c.new_tensor(I32, n_used, T)
            y = c.mul_mat_id(as_, b, ids)
            c.alloc()
            for t, v in ((as_, wv), (b, bv), (ids, ids_of(n_expert, n_used, T))):
                be.tensor_set(t, v)
            n0 = be.get_stat(stat + "_launches")
            be.graph_compute(c.graph())
            assert be.get_stat(stat + "_launches") == n0 + 1, f"{name} T={T} K={K}: not on the grouped kernel"
            key = f"{name} {n_expert}x{n_used} T={T} {M}x{K}"
            res[key] = be.tensor_get(y).copy().view(np.uint32)
            res[key + " KS"] = np.array([int(be.get_stat(stat + "_ks"))], np.uint32)
            c.free()
    np.savez(out, **res)
    print(f"{len(res) // 2} outputs written to {out}; KS: " + " ".join(str(int(res[k][0])) for k in res if k.endswith(" KS")))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else "/tmp/mmq_id_ab"
    os.makedirs(out, exist_ok=True)
    libs = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")}
    for side, lib in libs.items():
        rc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", os.path.join(out, side + ".npz")],
                            env=dict(os.environ, MI355X_LIB=lib)).returncode
        if rc != 0:
            sys.exit(f"{side} ({lib}): exit status {rc} -- stopping")
    a, b = np.load(os.path.join(out, "parent.npz")), np.load(os.path.join(out, "new.npz"))
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 2 * sum(len(s) for _, _, s in TYPES.values())
    nbytes = ndiff = 0
    for k in a.files:
        pa, pb = a[k].tobytes(), b[k].tobytes()
        d = len(pa) != len(pb) or pa != pb
        nbytes += len(pa)
        if d:
            ndiff += 1
            print("DIFFERENT:", k, "--", int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else "shape", "of", a[k].size, "values")
    print(f"{len(a.files) // 2} outputs and their KS, {nbytes} bytes compared: {'identical' if ndiff == 0 else '%d arrays differ' % ndiff}")
    sys.exit(1 if ndiff else 0)


if __name__ == "__main__":
    main()
