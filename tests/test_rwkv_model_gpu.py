"""RWKV MODELS through the reference's libllama on the plug-in (`-m gpu`): the synthetic `rwkv6` and `rwkv7` GGUF files of tools/make_synth_rwkv_gguf.py (2 layers, n_embd 256,
4 heads of 64; Q4_K / Q6_K projections) decoded by oracle/_ref/llama-bench-min, restated from tests/test_ssm_model_gpu.py.  From one token and after a 33-token prompt:
the reference CPU backend (-ngl 0) decodes 32 greedy ids; the plug-in (-ngl 99) is teacher-forced with those ids.  Bars: the logits of all 32 steps within NMSE 5e-4 of
the CPU's; the arg-max equal at every step whose CPU top-1 / top-2 margin exceeds 1e-3 x max|logit| (tests/test_rwkv_host.py guarantees at least 29 such steps); the device
named, all layers offloaded; one WKV launch (rwkv7: and one L2_NORM launch) per layer of every layer graph that went through the launchers, and decode steps that REPLAY a
captured graph.  Both sides run with -t 4: the reference's WKV6 kernel never returns with more threads than heads (4 here).

Placement.  llm_build_rwkv6 / llm_build_rwkv7 expand layer 0's token-shift build_rs nodes (the zeroing SCALE, two GET_ROWS, the extra-state CPY) before anything has visited
the token-embedding GET_ROWS, as llm_build_mamba does: [four state nodes: here] [inp_embd: CPU] [everything else: here].  Two things differ from the Mamba fixtures.  The
graph applies a LayerNorm to the embedding (token_embd_norm), and the loader keeps its weight and bias with the input layer in a CPU buffer: in a one-token graph the
scheduler runs NORM, MUL and ADD beside inp_embd on the CPU -- three splits, four nodes outside the plug-in, none of them refused by supports_op (the same three ops run here
everywhere else in the graph); at 32 tokens and more it offloads them here, copying the two weights in, which cuts the plug-in's part in three -- five splits, inp_embd alone
outside.  Measured: `graph splits = 5 (with bs=512), 3 (with bs=1)`.  So the test reads the scheduler's dump (GGML_SCHED_DEBUG=2) and asserts, node by node, that in EVERY
graph the nodes outside the plug-in are inp_embd and at most that norm's three, and the counts this order gives.  Every decode is two submissions here: the four-node state
graph (always eager) and the layer graph."""
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


@pytest.fixture(scope="module", params=["rwkv6", "rwkv7"])
def rwkv_gguf(request, tmp_path_factory):
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/llama-bench-min not built (make -f oracle/Makefile.ref llama)")
    d = tmp_path_factory.mktemp(request.param)
    gguf = str(d / f"tiny-{request.param}.gguf")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_rwkv_gguf.py"), "--arch", request.param, "-o", gguf], check=True, timeout=300, capture_output=True)
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
def test_rwkv_logits_placement_and_launches(rwkv_gguf, start):
    arch, gguf, pfile, d = rwkv_gguf
    args = ["--start-token", "1"] if start == "one_token" else ["--prompt-file", pfile]
    cpu_dump, gpu_dump = os.path.join(d, f"cpu_{start}.bin"), os.path.join(d, f"gpu_{start}.bin")
    ids_cpu, _ = _greedy(gguf, 0, args + ["--dump-all-logits", cpu_dump], False)
    _, err = _greedy(gguf, 99, args + ["--force-ids", ",".join(str(i) for i in ids_cpu), "--dump-all-logits", gpu_dump], True)
    assert "MI355X0" in err and "offloaded 3/3 layers to GPU" in err and "graph splits = 5 (with bs=512), 3 (with bs=1)" in err, err[-2500:]
    split, foreign, n_dumps = None, [], 0
    for line in err.splitlines():                                                             # the scheduler's dump of every graph it split
        h = re.match(r"## SPLIT #(\d+): (\S+)", line)
        if h:
            split = h.group(2)
            n_dumps += h.group(1) == "0"
        elif line.startswith("node #") and split != "MI355X0":
            foreign.append(line[:60])
    assert n_dumps > 0 and foreign
    pats = (r"node #\s*\d+ \(\s*GET_ROWS\):\s+inp_embd ", r"node #\s*\d+ \(\s*NORM\):\s+norm ", r"node #\s*\d+ \(\s*MUL\):\s+norm_w ", r"node #\s*\d+ \(\s*ADD\):\s+node_\d+ ")
    kinds = [next((k for k, p in enumerate(pats) if re.match(p, l)), -1) for l in foreign]
    assert -1 not in kinds, [l for l, k in zip(foreign, kinds) if k < 0][:6]
    assert kinds.count(0) == n_dumps                                                          # one token-embedding lookup per graph ...
    assert kinds.count(1) == kinds.count(2) == kinds.count(3) <= n_dumps                      # ... and, in the small-batch graphs, the three nodes of the token-embedding norm
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
    m = re.search(r"linear-attention launches \(process-wide\): wkv6=(\d+) gla=(\d+) wkv7=(\d+) l2_norm=(\d+)", err)
    assert g and m, err[-1500:]
    eager, captured, replayed = (int(x) for x in g.groups())
    total = eager + captured + replayed
    extra = 2 if start == "prompt33" else 0                                                 # the 33-token graph: the offloaded token-embedding norm cuts the plug-in's part in three
    assert (total - extra) % 2 == 0 and (total - extra) // 2 >= N, (eager, captured, replayed)      # two submissions per llama_decode (the state graph, the layer graph); one decode per greedy step
    decodes = (total - extra) // 2
    assert replayed > 0, (eager, captured, replayed)
    layer_graphs = decodes - replayed                                                       # the layer graphs that went through the launchers: eager or captured (the state graphs never replay)
    assert eager == decodes + extra + layer_graphs - captured, (eager, captured, replayed)
    wkv6, gla, wkv7, l2 = (int(x) for x in m.groups())
    want = (LAYERS * layer_graphs, 0, 0, 0) if arch == "rwkv6" else (0, 0, LAYERS * layer_graphs, LAYERS * layer_graphs)
    assert (wkv6, gla, wkv7, l2) == want, (m.groups(), eager, captured, replayed)
