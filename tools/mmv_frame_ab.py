#!/usr/bin/env python3
"""tools/mmv_frame_ab.py PARENT_LIB [OUT_DIR] -- do the block-format mat-vec kernels (k_mmv_blocks<Form, NCOLS, ROWS>, mmvq.hip) of this
tree compute the very bits the parent library's kernels compute?  One fresh child process per library (MI355X_LIB selects it), each under
its own time limit, runs MUL_MAT for every one of the nine forms with 1 .. 8 columns on the shapes of tests/test_mmv_frame_gpu.py plus
4096 x 4096, fixed seeds, and writes the raw outputs to an .npz; the two files are then compared byte for byte.  The parent runs first;
if its child fails, this tree's is not started.  Exit status 0: no byte differs.

PARENT_LIB is libggml-mi355x.so built from the parent commit in a git worktree (tools/launch_log_ab.sh shows how)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (type id, weights per block)
FORMS = {"q8_0": (8, 32), "q4_0": (2, 32), "q5_0": (6, 32), "iq4_nl": (20, 32), "iq4_xs": (23, 256), "q4_1": (3, 32), "q5_1": (7, 32), "q2_K": (10, 256), "q3_K": (11, 256)}
SHAPES = {32: [(16421, 96), (37, 2080), (4096, 4096)], 256: [(16421, 256), (37, 4352), (4096, 4096)]}


def child(out):
    sys.path.insert(0, ROOT)
    from bench import load_pkg
    pkg = load_pkg()
    from llama_cpp_omni_amd import qwen3
    be = pkg.backend(0)
    be.set_option("mv1", 0)                  # a single Q8_0 column on mmv_q8_0, not on the batch-1 kernel of mmv1q.hip
    res = {}
    for name, (ty, wpb) in FORMS.items():
        for M, K in SHAPES[wpb]:
            rng = np.random.default_rng(ty * 1000 + K)
            wv = qwen3.random_blocks(rng, ty, M, K)
            xv = rng.standard_normal((8, K)).astype(np.float32)
            for N in range(1, 9):
                c = pkg.Context(be)
                w, x = c.new_tensor(ty, K, M), c.new_tensor(pkg.GGML_TYPE_F32, K, N)
                y = c.mul_mat(w, x)
                c.alloc()
                be.tensor_set(w, wv); be.tensor_set(x, xv[:N])
                be.graph_compute(c.graph())
                res[f"{name} N={N} {M}x{K}"] = be.tensor_get(y).copy().view(np.uint32)
                c.free()
    np.savez(out, **res)
    print(f"{len(res)} outputs written to {out}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else "/tmp/mmv_frame_ab"
    os.makedirs(out, exist_ok=True)
    libs = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")}
    for side, lib in libs.items():
        rc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", os.path.join(out, side + ".npz")],
                            env=dict(os.environ, MI355X_LIB=lib)).returncode
        if rc != 0:
            sys.exit(f"{side} ({lib}): exit status {rc} -- stopping")
    a, b = np.load(os.path.join(out, "parent.npz")), np.load(os.path.join(out, "new.npz"))
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 9 * 3 * 8
    nbytes = ndiff = 0
    for k in a.files:
        pa, pb = a[k].tobytes(), b[k].tobytes()
        d = len(pa) != len(pb) or pa != pb
        nbytes += len(pa)
        if d:
            ndiff += 1
            print("DIFFERENT:", k, "--", int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else "shape", "of", a[k].size, "values")
    print(f"{len(a.files)} outputs, {nbytes} bytes compared: {'identical' if ndiff == 0 else '%d outputs differ' % ndiff}")
    sys.exit(1 if ndiff else 0)


if __name__ == "__main__":
    main()
