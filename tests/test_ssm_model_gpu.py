"""State-space MODELS through the reference's libllama on the plug-in (`-m gpu`): the synthetic `mamba2` and `mamba` GGUF files of tools/make_synth_mamba_gguf.py
(2 layers, d_inner 512; Q4_K ssm_in / ssm_x, Q6_K ssm_out) decoded by oracle/_ref/llama-bench-min, restated from tests/test_moe_model_gpu.py.  From one token and after a
33-token prompt: the reference CPU backend (-ngl 0) decodes 32 greedy ids; the plug-in (-ngl 99) is teacher-forced with those ids.  Bars: the logits of all 32 steps
within NMSE 5e-4 of the CPU's -- smoke()'s bar for end-to-end logits against the reference CPU backend; the arg-max equal at every step whose CPU top-1 / top-2 margin
exceeds 1e-3 x max|logit| (tests/test_ssm_host.py guarantees at least 29 such steps); the device named, all layers offloaded and no node declined; one SSM_CONV and
one SSM_SCAN launch per layer of every layer graph that went through the launchers (eager or captured), and decode steps that REPLAY a captured graph -- the scan reads
ids on the device and the cache views move, both survive capture.

Placement.  The dense and mixture-of-experts fixtures make two splits (the token-embedding lookup on the CPU, everything else here).  llm_build_mamba cannot: build_rs
calls ggml_build_forward_expand on layer 0's conv-state nodes (the zeroing SCALE, two GET_ROWS, the extra-state CPY) BEFORE anything has visited the token-embedding
GET_ROWS, so the graph's order is [four state nodes: here] [inp_embd: CPU, token_embd.weight lives in a CPU buffer] [everything else: here] -- three splits with every
node admitted (measured: `graph splits = 3`, the scheduler's own dump shows the CPU split holding the one GET_ROWS).  So the test reads that dump (GGML_SCHED_DEBUG=2)
and asserts what the split count stood for, node by node: in EVERY graph the scheduler split, the only node outside the plug-in is inp_embd, and the count is the 3
that this order gives.  Every decode is then two submissions here: the four-node state graph (always eager: nothing to capture) and the layer graph."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "llama-bench-min")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")
V, LAYERS, N = 512, 2, 32
PROMPT = [(7 * i + 3) % V for i in range(33)]


@pytest.fixture(scope="module", params=["mamba2", "mamba"])
def mamba_gguf(request, tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp(request.param)
    gguf = str(d / f"tiny-{request.param}.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_mamba_gguf.py"), "--arch", request.param, "-o", gguf], check=True, timeout=300, capture_output=True)
    pfile = str(d / "prompt.bin")
    np.asarray(PROMPT, np.int32).tofile(pfile)
    return request.param, gguf, pfile, str(d)


def _greedy(gguf, ngl, extra_args, plug):
    env = dict(os.environ)
    env.pop("GGML_BACKEND_PATH", None)
    if plug:
        env.update({"GGML_BACKEND_PATH": LIB, "MI355X_LOG_STATS": "1", "GGML_SCHED_DEBUG": "2"})
    out = subprocess.run([BIN, "-m", gguf, "-ngl", str(ngl), "--greedy", str(N), "-t", "4"] + extra_args, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])["greedy_ids"], out.stderr


@pytest.mark.parametrize("start", ["one_token", "prompt33"])
def test_mamba_logits_placement_and_launches(mamba_gguf, start):
    arch, gguf, pfile, d = mamba_gguf
    args = ["--start-token", "1"] if start == "one_token" else ["--prompt-file", pfile]
    cpu_dump, gpu_dump = os.path.join(d, f"cpu_{start}.bin"), os.path.join(d, f"gpu_{start}.bin")
    ids_cpu, _ = _greedy(gguf, 0, args + ["--dump-all-logits", cpu_dump], False)
    _, err = _greedy(gguf, 99, args + ["--force-ids", ",".join(str(i) for i in ids_cpu), "--dump-all-logits", gpu_dump], True)
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err and "graph splits = 3" in err, err[-2500:]
    split, foreign, n_dumps = None, [], 0
    for line in err.splitlines():                                                             # the scheduler's dump of every graph it split
        h = re.match(r"## SPLIT #(\d+): (\S+)", line)
        if h:
            split = h.group(2)
            n_dumps += h.group(1) == "0"
        elif line.startswith("node #") and split != "MI355X0":
            foreign.append(line[:60])
    assert n_dumps > 0 and foreign and all(re.match(r"node #\s*\d+ \(\s*GET_ROWS\):\s+inp_embd ", l) for l in foreign), foreign[:6]
    assert len(foreign) == n_dumps                                                            # one node per graph: the token-embedding lookup
    cpu, gpu = np.fromfile(cpu_dump, np.float32).reshape(N, V), np.fromfile(gpu_dump, np.float32).reshape(N, V)
    e = nmse(gpu, cpu)
    print(f"{arch} {start}: logits NMSE over {N} steps vs the reference CPU backend = {e:.3e}")
    assert np.isfinite(gpu).all()
    assert e <= 5e-4, f"logits NMSE {e:.3e} > 5e-4"
    top = np.sort(cpu, axis=1)
    wide = (top[:, -1] - top[:, -2]) > 1e-3 * np.abs(cpu).max(axis=1)
    assert wide.sum() >= 29, int(wide.sum())
    bad = [i for i in range(N) if wide[i] and int(gpu[i].argmax()) != int(cpu[i].argmax())]
    assert not bad, bad[:8]
    g = re.search(r"graphs eager=(\d+) captured=(\d+) replayed=(\d+)", err)
    m = re.search(r"state-space launches \(process-wide\): ssm_conv=(\d+) ssm_scan=(\d+)", err)
    assert g and m, err[-1500:]
    eager, captured, replayed = (int(x) for x in g.groups())
    total = eager + captured + replayed
    assert total % 2 == 0 and total // 2 >= N, (eager, captured, replayed)                 # two submissions per llama_decode (the state graph, the layer graph); one decode per greedy step
    assert replayed > 0, (eager, captured, replayed)
    layer_graphs = total // 2 - replayed                                                    # the layer graphs that went through the launchers: eager or captured (the state graphs never replay)
    assert eager == total // 2 + layer_graphs - captured, (eager, captured, replayed)
    assert int(m.group(1)) == int(m.group(2)) == LAYERS * layer_graphs, (m.groups(), eager, captured, replayed)
