"""A gpt-oss MODEL through the reference's libllama on the plug-in (`-m gpu`): the synthetic `gpt-oss` GGUF of tools/make_synth_gptoss_gguf.py (2 layers -- one with a
16-token sliding window, one full --, attention sinks and biases, 8 MXFP4 experts of n_ff 288 with 4 used, router bias, per-expert biases; separated lm-head AND router
logits) decoded by oracle/_ref/llama-bench-min, as tests/test_moe_model_gpu.py does for qwen3moe.  32 greedy ids, from one token and after a 33-token prompt (one ubatch:
MUL_MAT_ID and ADD_ID at 33 tokens; the prompt crosses the window, so the sliding-window mask and the sinks act), with and without flash attention, must equal the
reference CPU backend's (-ngl 0), which in turn must be the fixture's own cycle.  The launch statistics prove that no expert node went to the CPU: every graph the
plug-in ran through its launchers (eager or captured; a replay re-runs the captured launches) issued 3 MXFP4 MUL_MAT_ID and 3 ADD_ID launches per layer -- one launch
covers all slots x tokens pairs of a node -- and one ARGSORT launch per layer, none on the K-quant id kernel, and the scheduler made two splits (the token-embedding
lookup on the CPU, everything else here: SWIGLU_OAI included, or a third split would appear)."""
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
S, V, LAYERS, N = 96, 512, 2, 32
SPECIAL = [int(V // 16 + (V - V // 8) * i // S) for i in range(S)]                     # (tools/make_synth_moe_gguf.py special_ids)


@pytest.fixture(scope="module")
def gptoss_gguf(tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp("gptoss")
    gguf = str(d / "tiny-gptoss.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_gptoss_gguf.py"), "-o", gguf, "--separated", str(S)], check=True, timeout=300, capture_output=True)
    pfile = str(d / "prompt.bin")
    np.asarray(SPECIAL[:33], np.int32).tofile(pfile)
    return gguf, pfile


def _greedy(gguf, ngl, fa, extra_args, plug):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if plug:
        env.update({"GGML_BACKEND_PATH": LIB, "MI355X_LOG_STATS": "1"})
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "-fa", str(fa), "--greedy", str(N), "-t", "4"] + extra_args, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], out.stderr


@pytest.mark.parametrize("fa", [1, 0], ids=["fa", "no_fa"])
@pytest.mark.parametrize("start", ["one_token", "prompt33"])
def test_gptoss_greedy_ids_identical_and_experts_on_the_gpu(gptoss_gguf, start, fa):
    gguf, pfile = gptoss_gguf
    args, want = (["--start-token", str(SPECIAL[0])], SPECIAL[1:1 + N]) if start == "one_token" else (["--prompt-file", pfile], SPECIAL[34:34 + N])
    ids_cpu, _ = _greedy(gguf, 0, fa, args, False)
    assert ids_cpu == want, "the fixture's own continuation"
    ids_gpu, err = _greedy(gguf, 99, fa, args, True)
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err and "graph splits = 2" in err, err[-1500:]
    assert ids_gpu == ids_cpu, [i for i in range(N) if ids_gpu[i] != ids_cpu[i]][:8]
    g = re.search(r"graphs eager=(\d+) captured=(\d+) replayed=(\d+)", err)
    m = re.search(r"mixture-of-experts launches \(process-wide\): mmv_id=(\d+) argsort=(\d+) mmv_id_mxfp4=(\d+) add_id=(\d+)", err)
    assert g and m, err[-1500:]
    eager, captured, replayed = (int(x) for x in g.groups())
    assert eager + captured + replayed >= N + (1 if start == "prompt33" else 0), (eager, captured, replayed)      # one llama_decode per greedy step (+ the prompt)
    mmv_id, argsort, mxfp4, add_id = (int(x) for x in m.groups())
    assert mxfp4 == 3 * LAYERS * (eager + captured), (m.groups(), eager, captured)
    assert add_id == 3 * LAYERS * (eager + captured), (m.groups(), eager, captured)
    assert argsort == LAYERS * (eager + captured)
    assert mmv_id == 0
