"""IQ4_NL / IQ4_XS host side (no GPU): the type table, the synthetic-weight generator, the IQ4_XS type map, and a synthetic IQ4_XS GGUF
that the reference CPU build loads and decodes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
IQ4_NL, IQ4_XS, Q5_K, Q6_K = 20, 23, 13, 14


def test_iq4_type_table(pkg):
    from llama_cpp_omni_amd import ggml
    assert (ggml.GGML_TYPE_IQ4_NL, ggml.GGML_TYPE_IQ4_XS) == (IQ4_NL, IQ4_XS)
    assert ggml.row_size(IQ4_NL, 96) == 3 * 18
    assert ggml.row_size(IQ4_XS, 4096) == 16 * 136


@pytest.mark.parametrize("ty,K,bs,blk", [(IQ4_NL, 96, 18, 32), (IQ4_XS, 512, 136, 256)])
def test_iq4_random_blocks(pkg, ty, K, bs, blk):
    """valid blocks: a small positive f16 d, every other byte over its full range"""
    from llama_cpp_omni_amd import qwen3
    raw = qwen3.random_blocks(np.random.default_rng(1), ty, 300, K)
    assert raw.shape == (300, K // blk * bs) and raw.dtype == np.uint8
    b = raw.reshape(300, K // blk, bs)
    d = b[..., 0:2].copy().view(np.float16).astype(np.float32)
    assert (d > 0).all() and (d < 1e-3).all()
    rest = b[..., 2:]
    assert rest.min() == 0 and rest.max() == 255


def test_iq4_xs_type_map(pkg):
    """llama-quant.cpp without an imatrix: attn_v Q5_K at n_gqa >= 4, ffn_down Q5_K in the first n_layer / 8 layers, output Q6_K"""
    from llama_cpp_omni_amd import qwen3
    t = qwen3.iq4_xs_types(qwen3.QWEN3_8B)
    assert t["output"] == Q6_K
    for i in range(36):
        assert t[i]["attn_v"] == Q5_K                                        # 32 / 8 = 4 query heads per KV head
        assert t[i]["ffn_down"] == (Q5_K if i < 4 else IQ4_XS)
        assert all(t[i][k] == IQ4_XS for k in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up"))
    tt = qwen3.iq4_xs_types(qwen3.TINY)                                      # n_gqa 2, n_layer / 8 = 0: everything but the output IQ4_XS
    assert all(v == IQ4_XS for i in range(2) for v in tt[i].values())
    odd = qwen3.iq4_xs_types(dict(qwen3.TINY, n_ff=640))                     # rows of 640 weights: demoted to IQ4_NL (:463)
    assert odd[0]["ffn_down"] == IQ4_NL and odd[0]["ffn_up"] == IQ4_XS


@pytest.mark.parametrize("types", ["iq4_xs", "iq4_nl"])
def test_synthetic_iq4_gguf_loads_on_reference_cpu(tmp_path, types):
    """CPU-only: the IQ4 files written by tools/make_synth_gguf.py are accepted by the reference loader and decode"""
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
    assert ("type iq4_xs" in out.stderr) if types == "iq4_xs" else ("type iq4_nl" in out.stderr)
