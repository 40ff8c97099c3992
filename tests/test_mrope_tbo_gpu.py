"""The reference's OWN op-parity harness on the M-RoPE and vision cases of ROPE (`-m gpu`): `oracle/_ref/test-backend-ops test -b MI355X0 -o ROPE -p <regex>`
against libggml-mi355x.so as the reference's loader finds it through GGML_BACKEND_PATH (tests/test_backend_ops_gpu.py explains the harness; its runner is
restated here, as in test_ssm_tbo_gpu.py).  The regex selects the f32 cases with mode=8 (qwen2vl 2B / 7B head counts, n_dims 128 / 20 / 32) or mode=24
(the ViT: 80 channels, 16 heads), with and without frequency factors, YaRN and a strided source, and the in-place cases.  The harness must report no FAIL,
exit 0, and EVERY case it lists under the filter must have run and be OK: none may be reported as not supported.  The count comes from its own output."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TBO = os.path.join(ROOT, "oracle", "_ref", "test-backend-ops")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")
ANSI = re.compile(r"\x1b\[[0-9;]*m")
FILTER = r"type=f32,.*mode=(8|24),"


def _run(op, params, timeout=300):
    if not os.path.exists(TBO):
        pytest.skip("oracle/_ref/test-backend-ops was not built (it is compiled where the reference sources exist and travels with the snapshot)")
    env = dict(os.environ)
    env["GGML_BACKEND_PATH"] = LIB
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "oracle", "_ref") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([TBO, "test", "-b", "MI355X0", "-o", op, "-p", params], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env, cwd=ROOT)
    out = ANSI.sub("", r.stdout)
    cases = [l for l in out.splitlines() if "): " in l]
    return r.returncode, cases, out


def test_reference_test_backend_ops_rope_mrope_and_vision():
    rc, cases, out = _run("ROPE", FILTER)
    listed = [l for l in cases if l.lstrip().startswith("ROPE(")]
    ok = [l for l in listed if l.rstrip().endswith("OK")]
    fail = [l for l in cases if "FAIL" in l]
    unsupported = [l for l in cases if "not supported" in l]
    assert not fail, "\n".join(fail[:8])
    assert rc == 0, out[-2000:]
    assert not unsupported, "\n".join(unsupported[:8])
    assert all(re.search(FILTER, l) for l in listed) and listed == cases, "the filter let something else through:\n" + "\n".join(cases[:4])
    n8, n24 = (sum(1 for l in listed if f"mode={m}," in l) for m in (8, 24))
    assert n8 > 0 and n24 > 0, out[-1500:]
    assert len(ok) == len(listed), f"{len(ok)} of {len(listed)} listed cases ran OK on the plug-in:\n" + out[-1500:]
    print(f"ROPE, {FILTER}: {len(ok)} cases OK ({n8} M-RoPE, {n24} vision)")
