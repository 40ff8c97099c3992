"""The reference's OWN op-parity harness on the ops of a gpt-oss expert layer (`-m gpu`): `oracle/_ref/test-backend-ops test -b MI355X0 -o ADD_ID` and `-o MUL_MAT_ID`
against libggml-mi355x.so as the reference's loader finds it through GGML_BACKEND_PATH (tests/test_backend_ops_gpu.py explains the harness; its runner is restated
here as in tests/test_moe_tbo_gpu.py).  An op passes when the harness reports no FAIL line, exits 0 and ran at least one supported case; for MUL_MAT_ID at least one
`type_a=mxfp4` case must have run and ended in OK (the expert types without an id kernel are refused by supports_op and reported as not supported)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TBO = os.path.join(ROOT, "oracle", "_ref", "test-backend-ops")
LIB = os.path.join(ROOT, "llama.cpp-omni_amd", "lib", "libggml-mi355x.so")
ANSI = re.compile(r"\x1b\[[0-9;]*m")


def _run(op, timeout=900):
    if not os.path.exists(TBO):
        pytest.skip("oracle/_ref/test-backend-ops was not built (it is compiled where the reference sources exist and travels with the snapshot)")
    env = dict(os.environ)
    env["GGML_BACKEND_PATH"] = LIB
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "oracle", "_ref") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([TBO, "test", "-b", "MI355X0", "-o", op], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env, cwd=ROOT)
    out = ANSI.sub("", r.stdout)
    cases = [l for l in out.splitlines() if "): " in l]
    ok = [l for l in cases if l.rstrip().endswith("OK")]
    fail = [l for l in cases if "FAIL" in l]
    return r.returncode, ok, fail, out


@pytest.mark.parametrize("op", ["ADD_ID", "MUL_MAT_ID"])
def test_reference_test_backend_ops_gptoss(op):
    rc, ok, fail, out = _run(op)
    assert not fail, "\n".join(fail[:8])
    assert rc == 0, out[-2000:]
    assert ok, f"no supported case of {op} ran on the plug-in:\n" + out[-1500:]
    if op == "MUL_MAT_ID":
        mx = [l for l in ok if "type_a=mxfp4" in l]
        assert mx, "no MXFP4 case of MUL_MAT_ID ran on the plug-in:\n" + "\n".join(l for l in out.splitlines() if "mxfp4" in l)[-1500:]
        print(f"{op}: {len(mx)} MXFP4 cases OK")
    print(f"{op}: {len(ok)} supported cases OK")
