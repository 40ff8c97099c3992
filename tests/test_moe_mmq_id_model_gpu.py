"""A mixture-of-experts MODEL whose prompt ubatch takes the expert-grouped MUL_MAT_ID path (`-m gpu`): the synthetic `qwen3moe` GGUF of tools/make_synth_moe_gguf.py
(2 layers, 8 experts, 2 used, Q4_K gate / up and Q6_K down experts; separated lm-head AND router logits) through the reference's libllama on the plug-in, decoded by
oracle/_ref/llama-bench-min as tests/test_moe_model_gpu.py does at 1 and 33 tokens.  Here the prompt is 64 tokens -- one ubatch, MUL_MAT_ID at 64 tokens: the grouped
int8-MFMA kernel (mmq_id.hip) -- followed by 24 greedy ids, which must equal the reference CPU backend's (-ngl 0), which in turn must be the fixture's own cycle.
The launch statistics prove the path.  llama-bench-min asks for the logits of the prompt's LAST token only (as llama-bench's prompt test does), and libllama then cuts
the last layer down to that one row in front of its feed-forward block (the `inp_out_ids` GET_ROWS of every llm_build_*): in the ONE prompt graph the expert nodes of
layers 0 .. LAYERS - 2 see the whole 64-token ubatch and must all go through the grouped launchers, the last layer's three see one token and must take the per-pair
kernel, as the three nodes per layer of every other graph do (eager or captured; a replay re-runs the captured launches without counting them):
    mmq_id == 3 * (LAYERS - 1)
    mmv_id == 3 * LAYERS * (eager + captured - 1) + 3
    mmq_id + mmv_id == 3 * LAYERS * (eager + captured)        -- every expert node of every graph ran on the plug-in, on exactly one of the two paths
(observed: eager + captured = 3, mmq_id = 3, mmv_id = 15.  "3 * LAYERS grouped nodes for the prompt graph" cannot occur with this driver: no kernel choice puts a
one-token node on the 64-token path.  Both layers at 64 tokens, captured and replayed, is what test_moe_ffn_block_64_tokens_eager_captured_replayed covers.)"""
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
S, V, LAYERS, N, PROMPT = 96, 512, 2, 24, 64
SPECIAL = [int(V // 16 + (V - V // 8) * i // S) for i in range(S)]                     # (tools/make_synth_moe_gguf.py special_ids)


@pytest.fixture(scope="module")
def moe_gguf(tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp("moe_mmq_id")
    gguf = str(d / "tiny-moe.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_moe_gguf.py"), "-o", gguf, "--separated", str(S)], check=True, timeout=300, capture_output=True)
    pfile = str(d / "prompt.bin")
    np.asarray(SPECIAL[:PROMPT], np.int32).tofile(pfile)
    return gguf, pfile


def _greedy(gguf, ngl, extra_args, plug):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if plug:
        env.update({"GGML_BACKEND_PATH": LIB, "MI355X_LOG_STATS": "1"})
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "-fa", "1", "--greedy", str(N), "-t", "4"] + extra_args, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], out.stderr


def test_qwen3moe_prompt64_greedy_ids_identical_and_prompt_on_the_grouped_kernel(moe_gguf):
    gguf, pfile = moe_gguf
    args, want = ["--prompt-file", pfile], SPECIAL[PROMPT + 1:PROMPT + 1 + N]
    ids_cpu, _ = _greedy(gguf, 0, args, False)
    assert ids_cpu == want, "the fixture's own continuation"
    ids_gpu, err = _greedy(gguf, 99, args, True)
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err, err[-1500:]
    assert ids_gpu == ids_cpu, [i for i in range(N) if ids_gpu[i] != ids_cpu[i]][:8]
    g = re.search(r"graphs eager=(\d+) captured=(\d+) replayed=(\d+)", err)
    m = re.search(r"mixture-of-experts launches \(process-wide\): mmv_id=(\d+) argsort=(\d+) mmv_id_mxfp4=(\d+) add_id=(\d+) mmq_id=(\d+)", err)
    assert g and m, err[-1500:]
    eager, captured, replayed = (int(x) for x in g.groups())
    assert eager + captured + replayed >= N + 1, (eager, captured, replayed)           # one llama_decode per greedy step + the prompt
    mmv_id, mmq_id = int(m.group(1)), int(m.group(5))
    assert mmq_id == 3 * (LAYERS - 1), m.groups()                                      # the one prompt graph (eager: it is submitted once), every layer that sees the ubatch
    assert mmv_id == 3 * LAYERS * (eager + captured - 1) + 3, (m.groups(), eager, captured)      # every other graph, and the prompt graph's last layer (one row)
    assert mmq_id + mmv_id == 3 * LAYERS * (eager + captured)
    assert int(m.group(2)) == LAYERS * (eager + captured)
