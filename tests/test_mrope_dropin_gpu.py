"""A Qwen2-VL-shaped model through the REFERENCE's libllama with this backend as a plug-in (-m gpu; tests/test_llama_dropin.py explains the set-up, whose
runner is restated here): tools/make_synth_gguf.py --config qwen2vl-tiny writes a 2-layer file of arch qwen2vl (attn_q/k/v.bias, no q / k norm,
qwen2vl.rope.dimension_sections), which llm_build_qwen2vl turns into two ggml_rope_multi nodes per layer over a position tensor of 4 * n_tokens entries.
Greedy ids over the same prompt and length as test_llama_dropin's tiny model must equal the CPU backend's, and the scheduler (GGML_SCHED_DEBUG=2) must
place every ROPE node on the plug-in: before modes 8 / 24 were admitted it cut the graph twice per layer around them.

Text tokens give equal t / h / w positions, so this checks loading, supports_op probing and the 4 * n_tokens layout; the sections are checked by
test_mrope_ops_gpu.py and test_mrope_layer_gpu.py."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")
ROPE_LINE = re.compile(r"^node #\s*\d+ \(\s*ROPE\):\s+\S+.*?\[\s*(\S+)[^\]]*\]", re.M)


def _greedy(gguf, ngl, fa, dump, env_extra=None):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if env_extra:
        env.update(env_extra)
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "-fa", str(fa), "--greedy", "24", "-t", "4", "--dump-logits", dump],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], np.fromfile(dump, np.float32), out.stderr


@pytest.mark.parametrize("fa", [1, 0])
def test_reference_libllama_runs_qwen2vl_on_the_plugin(tmp_path, fa):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    gguf = str(tmp_path / "qwen2vl.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gguf.py"), "--config", "qwen2vl-tiny", "--types", "q4_k_m", "-o", gguf,
                    "--distinct-layers"], check=True, timeout=300)
    ids_cpu, l_cpu, _ = _greedy(gguf, 0, fa, str(tmp_path / "cpu.bin"))
    ids_gpu, l_gpu, err = _greedy(gguf, 99, fa, str(tmp_path / "gpu.bin"), {"GGML_BACKEND_PATH": LIB, "GGML_SCHED_DEBUG": "2"})
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err
    placed = ROPE_LINE.findall(err)
    assert len(placed) >= 4, err[-3000:]                                  # two layers, q and k (every graph the scheduler printed)
    assert all(p.startswith("MI355") for p in placed), sorted(set(placed))
    assert ids_gpu == ids_cpu
    nm = float(((l_cpu - l_gpu) ** 2).sum() / (l_cpu ** 2).sum())
    print(f"qwen2vl-tiny fa {fa}: {len(placed)} ROPE nodes on the plug-in, logits NMSE vs the CPU backend {nm:.3e}")
    assert nm < 5e-4
