"""Q4_1 / Q5_1 / Q2_K / Q3_K host side (no GPU): the synthetic-weight generator, the synthetic GGUF files the reference CPU build loads and
decodes, and the launch counters' names in the public header and the library's stat table."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
Q4_1, Q5_1, Q2_K, Q3_K = 3, 7, 10, 11
# type -> (weights per block, block bytes, byte offsets of the f16 fields)
LAYOUT = {Q4_1: (32, 20, (0, 2)), Q5_1: (32, 24, (0, 2)), Q2_K: (256, 84, (80, 82)), Q3_K: (256, 110, (108,))}
STATS = ("mmv_q41_launches", "mmv_q51_launches", "mmv_q2k_launches", "mmv_q3k_launches")


@pytest.mark.parametrize("ty,K", [(Q4_1, 96), (Q5_1, 96), (Q2_K, 512), (Q3_K, 512)])
def test_lowbit_random_blocks(pkg, ty, K):
    """the right byte count per type; the f16 fields finite, positive and small; every other byte over its full range"""
    from llama_cpp_omni_amd import ggml, qwen3
    blk, bs, f16_at = LAYOUT[ty]
    raw = qwen3.random_blocks(np.random.default_rng(1), ty, 300, K)
    assert raw.shape == (300, K // blk * bs) and raw.dtype == np.uint8
    assert ggml.row_size(ty, K) == K // blk * bs
    b = raw.reshape(300, K // blk, bs)
    rest = np.ones(bs, bool)
    for o in f16_at:
        v = b[..., o:o + 2].copy().view(np.float16).astype(np.float32)
        assert np.isfinite(v).all() and (v > 0).all() and (v < 1e-1).all(), (ty, o)
        rest[o:o + 2] = False
    assert b[..., rest].min() == 0 and b[..., rest].max() == 255


@pytest.mark.parametrize("ty,K,per_d", [(Q4_1, 4096, 4.6), (Q5_1, 4096, 9.2), (Q2_K, 4096, 13.9), (Q3_K, 4096, 43.0)])
def test_lowbit_random_blocks_honour_std(pkg, ty, K, per_d):
    """the block scale follows `std`: d = std / (the format's spread per unit of d) * U(0.5, 1.5)"""
    from llama_cpp_omni_amd import qwen3
    blk, bs, f16_at = LAYOUT[ty]
    for std in (0.02, 0.1):
        b = qwen3.random_blocks(np.random.default_rng(2), ty, 64, K, std=std).reshape(64, K // blk, bs)
        d = b[..., f16_at[0]:f16_at[0] + 2].copy().view(np.float16).astype(np.float32)
        assert abs(float(d.mean()) * per_d / std - 1.0) < 0.05, (ty, std, float(d.mean()))


def test_lowbit_stat_names_are_listed():
    """the four launch counters are named in the public header and answered by mi355x_get_stat"""
    hdr = open(os.path.join(ROOT, "include", "ggml-mi355x.h")).read()
    src = open(os.path.join(ROOT, "llama.cpp-omni_amd", "csrc", "graph.cpp")).read()
    for name in STATS:
        assert '"%s"' % name in hdr, name
        assert '"%s"' % name in src, name


@pytest.mark.parametrize("types", ["q4_1", "q5_1", "q2_k", "q3_k"])
def test_synthetic_lowbit_gguf_loads_on_reference_cpu(tmp_path, types):
    """CPU-only: the files written by tools/make_synth_gguf.py are accepted by the reference loader and decode"""
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built")
    gguf = str(tmp_path / "tiny.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gguf.py"), "--config", "tiny", "--types", types, "-o", gguf,
                    "--distinct-layers"], check=True, timeout=300)
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    out = subprocess.run([BIN, "-m", gguf, "-ngl", "0", "-fa", "1", "--greedy", "24", "-t", "4", "--dump-logits", str(tmp_path / "cpu.bin")],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    ids = json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"]
    logits = np.fromfile(str(tmp_path / "cpu.bin"), np.float32)
    assert len(ids) == 24 and np.isfinite(logits).all() and logits.size == 512
    assert ("type %s" % {"q2_k": "q2_K", "q3_k": "q3_K"}.get(types, types)) in out.stderr
