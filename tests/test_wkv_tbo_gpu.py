"""The reference's OWN op-parity harness on the four linear-attention ops (`-m gpu`): `oracle/_ref/test-backend-ops test -b MI355X0 -o RWKV_WKV6`, `-o GATED_LINEAR_ATTN`,
`-o RWKV_WKV7` and `-o L2_NORM` against libggml-mi355x.so as the reference's loader finds it through GGML_BACKEND_PATH (tests/test_backend_ops_gpu.py explains the
harness; its runner is restated here, as in test_ssm_tbo_gpu.py).  The harness holds four cases of each WKV op (32 heads of 64; 1 x 1, 32 x 1, 32 x 4 and 128 x 4 tokens x
sequences; the WKV7 graphs put an L2_NORM in front of a and b) and five L2_NORM cases ({64, 5, 4, 3}, eps 0 / 1e-6 / 1e-4 / 1e-1 / 1e-12) (test-backend-ops.cpp:6290-6341).
An op passes when the harness reports no FAIL line, exits 0 and EVERY case ran and is OK: none may be reported as not supported."""
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


@pytest.mark.parametrize("op,n_cases", [("RWKV_WKV6", 4), ("GATED_LINEAR_ATTN", 4), ("RWKV_WKV7", 4), ("L2_NORM", 5)])
def test_reference_test_backend_ops_wkv(op, n_cases):
    rc, ok, fail, unsupported, out = _run(op)
    assert not fail, "\n".join(fail[:8])
    assert rc == 0, out[-2000:]
    assert not unsupported, "\n".join(unsupported[:8])
    assert ok == n_cases, f"{ok} of {n_cases} cases of {op} ran OK on the plug-in:\n" + out[-1500:]
    print(f"{op}: {ok} cases OK")
