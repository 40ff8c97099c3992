"""A gpt-oss MODEL whose prompt reaches the expert-grouped MXFP4 kernel (`-m gpu`): the synthetic `gpt-oss` GGUF of tools/make_synth_gptoss_gguf.py (2 layers, 8 MXFP4
experts of n_ff 288 with 4 used; see tests/test_gptoss_model_gpu.py) decoded by oracle/_ref/llama-bench-min through the reference's libllama on the plug-in.  The prompt
file holds the fixture's separated ids, cycled, and is decoded in batches of 160 tokens (`-b 160`), each ONE ubatch that reaches the expert nodes at 160 tokens --
above MMQ_ID_MXFP4_MIN_TOKENS -- on kernels/mmq_id.hip; the 32 greedy steps behind it run at one token on the per-pair kernel.

Why two batches of 160 and not one: only the last token of a batch asks for logits, and libllama cuts the LAST layer down to the rows that are output in front of its
FFN.  So a batch of 160 tokens runs the experts of every layer but the last at 160 tokens and those of the last layer at ONE: 3 x (layers - 1) = 3 grouped nodes, measured
with a single 160-token prompt (stats line: mmv_id_mxfp4=15 mmq_id_mxfp4=3; the ids were equal).  The bar "3 x layers nodes on the grouped kernel" needs a second such
batch, which also crosses the sliding window and reads a cache that the first one wrote.

The 32 greedy ids must equal the reference CPU backend's (-ngl 0), with and without flash attention.  The launch statistics: every graph the plug-in ran through its
launchers (eager or captured) issued 3 MXFP4 MUL_MAT_ID nodes per layer, on one of the two MXFP4 kernels, at least 3 x layers of them on the grouped one; none on a
K-quant id kernel; two graph splits (nothing but the token-embedding lookup on the CPU).
Where the ids differ, the run is repeated with MI355X_MMQ_ID=0 (every node on the per-pair kernel) and the assertion names which of the two the difference follows:
the new path, or the fixture at this prompt length."""
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
S, V, LAYERS, N, UBATCH, PROMPT = 96, 512, 2, 32, 160, 320
SPECIAL = [int(V // 16 + (V - V // 8) * i // S) for i in range(S)]                     # (tools/make_synth_moe_gguf.py special_ids)


@pytest.fixture(scope="module")
def gptoss_gguf(tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp("gptoss_mmq_id")
    gguf = str(d / "tiny-gptoss.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gptoss_gguf.py"), "-o", gguf, "--separated", str(S)], check=True, timeout=300, capture_output=True)
    pfile = str(d / "prompt320.bin")
    np.asarray([SPECIAL[i % S] for i in range(PROMPT)], np.int32).tofile(pfile)
    return gguf, pfile


def _greedy(gguf, ngl, fa, extra_args, plug, env_extra=None):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if plug:
        env.update({"GGML_BACKEND_PATH": LIB, "MI355X_LOG_STATS": "1"})
        env.update(env_extra or {})
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "-fa", str(fa), "--greedy", str(N), "-t", "4"] + extra_args, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], out.stderr


@pytest.mark.parametrize("fa", [1, 0], ids=["fa", "no_fa"])
def test_gptoss_prompt_2x160_greedy_ids_identical_and_prefill_experts_grouped(gptoss_gguf, fa):
    gguf, pfile = gptoss_gguf
    args = ["--prompt-file", pfile, "-b", str(UBATCH)]                # two llama_decode calls of 160 tokens, one ubatch each
    ids_cpu, _ = _greedy(gguf, 0, fa, args, False)
    assert len(ids_cpu) == N
    ids_gpu, err = _greedy(gguf, 99, fa, args, True)
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err and "graph splits = 2" in err, err[-1500:]
    if ids_gpu != ids_cpu:                                            # the new path, or the fixture at 160 tokens?  the same run with every node on the per-pair kernel
        ids_pp, _ = _greedy(gguf, 99, fa, args, True, {"MI355X_MMQ_ID": "0"})
        first = [i for i in range(N) if ids_gpu[i] != ids_cpu[i]][:8]
        assert False, (f"greedy ids differ from -ngl 0 at steps {first}; with MI355X_MMQ_ID=0 they " +
                       ("equal -ngl 0: the difference follows the grouped MXFP4 kernel" if ids_pp == ids_cpu else "differ as well: the fixture at this prompt length, not the grouped kernel"))
    g = re.search(r"graphs eager=(\d+) captured=(\d+) replayed=(\d+)", err)
    m = re.search(r"mixture-of-experts launches \(process-wide\): mmv_id=(\d+) argsort=(\d+) mmv_id_mxfp4=(\d+) add_id=(\d+) mmq_id=(\d+) mmq_id_mxfp4=(\d+)", err)
    assert g and m, err[-1500:]
    eager, captured, replayed = (int(x) for x in g.groups())
    assert eager + captured + replayed >= N + PROMPT // UBATCH, (eager, captured, replayed)      # one llama_decode per greedy step + the prompt's two
    mmv_id, argsort, mmv_mx, add_id, mmq_id, mmq_mx = (int(x) for x in m.groups())
    assert mmq_mx >= 3 * LAYERS, m.groups()                           # the prompt's expert nodes at 160 tokens: 3 x (layers - 1) per batch, two batches
    assert mmq_mx + mmv_mx == 3 * LAYERS * (eager + captured), (m.groups(), eager, captured)
    assert mmv_id == 0 and mmq_id == 0, m.groups()
