"""The reference's OWN op-parity harness on the two state-space ops (`-m gpu`): `oracle/_ref/test-backend-ops test -b MI355X0 -o SSM_CONV` and `-o SSM_SCAN`
against libggml-mi355x.so as the reference's loader finds it through GGML_BACKEND_PATH (tests/test_backend_ops_gpu.py explains the harness; its runner is
restated here, as in test_moe_tbo_gpu.py).  The harness holds 18 SSM_CONV cases (d_conv 3 / 4, 1024 / 1536 / 2048 channels, one, five or six tokens, one or four
sequences) and the Mamba-1 / Mamba-2 / Falcon-H1 SSM_SCAN cases (test-backend-ops.cpp:6316-6326).  An op passes when the harness reports no FAIL line, exits 0
and EVERY case ran and is OK: none may be reported as not supported."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TBO = os.path.join(ROOT, "oracle", "_ref", "test-backend-ops")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")
ANSI = re.compile(r"\x1b\[[0-9;]*m")


def _run(op, timeout=300):
    if not os.path.exists(TBO):
        pytest.skip("oracle/_ref/test-backend-ops was not built (it is compiled where the reference sources exist and travels with the snapshot)")
    env = dict(os.environ)
    env["GGML_BACKEND_PATH"] = LIB
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "oracle", "_ref") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([TBO, "test", "-b", "MI355X0", "-o", op], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env, cwd=ROOT)
    out = ANSI.sub("", r.stdout)
    cases = [l for l in out.splitlines() if "): " in l]
    ok = sum(1 for l in cases if l.rstrip().endswith("OK"))
    fail = [l for l in cases if "FAIL" in l]
    unsupported = [l for l in cases if "not supported" in l]
    return r.returncode, ok, fail, unsupported, out


@pytest.mark.parametrize("op,n_cases", [("SSM_CONV", 18), ("SSM_SCAN", 3)])
def test_reference_test_backend_ops_ssm(op, n_cases):
    rc, ok, fail, unsupported, out = _run(op)
    assert not fail, "\n".join(fail[:8])
    assert rc == 0, out[-2000:]
    assert not unsupported, "\n".join(unsupported[:8])
    assert ok == n_cases, f"{ok} of {n_cases} cases of {op} ran OK on the plug-in:\n" + out[-1500:]
    print(f"{op}: {ok} cases OK")
