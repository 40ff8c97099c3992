"""The linear-attention ops on the GPU (`-m gpu`): RWKV_WKV6, GATED_LINEAR_ATTN, RWKV_WKV7 and L2_NORM (kernels/wkv.hip), each through the backend C-ABI and against
the reference CPU backend (oracle/ref_backend.py) on the same graph.

Bar: NMSE <= 1e-7, the default max_nmse_err of the reference's own harness (test-backend-ops.cpp:996), which the four ops inherit; for the WKV ops it is taken
SEPARATELY over the outputs and over the new states.  Shapes: the two specialised head sizes (64, 128) and two that only the generic kernels take (24, and the 123 of
the loader's probe, with 2 heads); 3 heads, and 32 at S = 64; 1, 5 and 67 tokens per sequence, 1 and 3 sequences -- every S with every token count once.  All of those take
the 8-column form of the WKV6 / GLA kernel (fewer than 512 waves otherwise); WIDE adds the smallest shapes on the other side of that threshold, 43 heads x 3 sequences at
S = 64 and 22 x 3 at S = 128, which take the 16-column form.  Decays lie in (0.3, 1); WKV7 gets
a = -kk, b = kk * sigmoid(.) with kk l2-normalised per head, as the model feeds it.  The reference's result of a case is computed once and shared.

Two properties of the reference CPU backend shape this file.  Its WKV6 / GLA kernels never return when it runs more threads than the graph has heads (ref_be below: two
threads).  Its WKV7 kernel writes out of bounds at head sizes that are no multiple of its vector step (_ref_takes): the generic WKV7 cases (S = 24, 123) are compared with
the float64 restatement written here, which test_reference_equals_float64_restatement ties to the reference at the sizes it can run."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, F16 = 0, 1
BAR = 1e-7
OPS = ["wkv6", "gla", "wkv7"]
# (S, H, tokens per sequence, n_seqs)
CASES = [(64, 3, 1, 1), (64, 3, 5, 3), (64, 3, 67, 1), (64, 32, 1, 3), (64, 32, 5, 1),
         (128, 3, 1, 3), (128, 3, 5, 1), (128, 3, 67, 3),
         (24, 2, 1, 1), (24, 2, 5, 3), (24, 2, 67, 1),
         (123, 2, 1, 3), (123, 2, 5, 1), (123, 2, 67, 3)]
WIDE = [(64, 43, 1, 3), (64, 43, 5, 3), (128, 22, 2, 3)]
GLA_SCALE = 0.37


@pytest.fixture(scope="module")
def ref_be(pkg):
    """The reference CPU backend with TWO threads.  ggml_compute_forward_rwkv_wkv6_f32 and _gla_f32 return early in every thread whose index is not below the head
    count (ops.cpp:9192) and then wait on a barrier of ALL threads (:9215): with more threads than heads the reference never returns.  The smallest head count here is 2."""
    from oracle.ref_backend import make_ref_cpu_backend, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libggml-ref.so not built (needs the reference sources at build time)")
    return make_ref_cpu_backend(pkg, 2)


def _graph(pkg, be_, op, S, H, T, n_seqs, ty=F32, state_ne=None, tf_ne=None):
    c = pkg.Context(be_)
    t3 = lambda: c.new_tensor(ty, S, H, T)
    state = c.new_tensor(ty, *(state_ne or (S * S * H, n_seqs)))
    if op == "wkv6":
        src = dict(k=t3(), v=t3(), r=t3(), tf=c.new_tensor(ty, *(tf_ne or (S, H))), td=t3(), state=state)
        y = c.rwkv_wkv6(*src.values())
    elif op == "gla":
        src = dict(k=t3(), v=t3(), q=t3(), g=t3(), state=state)
        y = c.gated_linear_attn(*src.values(), GLA_SCALE)
    else:
        src = dict(r=t3(), w=t3(), k=t3(), v=t3(), a=t3(), b=t3(), state=state)
        y = c.rwkv_wkv7(*src.values())
    return c, src, y


def _data(op, S, H, T, n_seqs, seed):
    rng = np.random.default_rng(seed)
    n = lambda: (rng.standard_normal((T, H, S)) * 0.5).astype(np.float32)
    decay = lambda: rng.uniform(0.3, 1.0, (T, H, S)).astype(np.float32)
    state = rng.standard_normal((n_seqs, S * S * H)).astype(np.float32)
    if op == "wkv6":
        return dict(k=n(), v=n(), r=n(), tf=(rng.standard_normal((H, S)) * 0.5).astype(np.float32), td=decay(), state=state)
    if op == "gla":
        return dict(k=n(), v=n(), q=n(), g=decay(), state=state)
    kk = rng.standard_normal((T, H, S))
    kk /= np.maximum(np.sqrt((kk ** 2).sum(-1, keepdims=True)), 1e-12)
    gate = 1.0 / (1.0 + np.exp(-rng.standard_normal((T, H, S))))
    return dict(r=n(), w=decay(), k=n(), v=n(), a=(-kk).astype(np.float32), b=(kk * gate).astype(np.float32), state=state)


def _run(pkg, be_, op, S, H, T, n_seqs, data):
    c, src, y = _graph(pkg, be_, op, S, H, T, n_seqs)
    c.alloc()
    for k, t in src.items():
        be_.tensor_set(t, data[k])
    be_.graph_compute(c.graph())
    res = be_.tensor_get(y).copy().ravel()
    c.free()
    return res


def _f64(op, data, S, H, tps, n_seqs):
    """NumPy float64 restatement of the three recurrences -> the result's layout: outputs {T, H, S}, then the new states {n_seqs, H, S, S}"""
    d = {k: np.asarray(v, np.float64) for k, v in data.items()}
    states = d["state"].reshape(n_seqs, H, S, S).copy()
    out = np.zeros((tps * n_seqs, H, S))
    for t in range(tps * n_seqs):
        s = states[t // tps]
        for h in range(H):
            if op == "wkv6":
                kv = np.outer(d["k"][t, h], d["v"][t, h])
                out[t, h] = d["r"][t, h] @ (d["tf"][h][:, None] * kv + s[h])
                s[h] = s[h] * d["td"][t, h][:, None] + kv
            elif op == "gla":
                s[h] = s[h] * d["g"][t, h][:, None] + np.outer(d["k"][t, h], d["v"][t, h])
                out[t, h] = (d["q"][t, h] * GLA_SCALE) @ s[h]
            else:
                sa = s[h] @ d["a"][t, h]
                s[h] = s[h] * d["w"][t, h][None, :] + np.outer(d["v"][t, h], d["k"][t, h]) + np.outer(sa, d["b"][t, h])
                out[t, h] = s[h] @ d["r"][t, h]
    return np.concatenate([out.ravel(), states.ravel()])


def _ref_takes(op, S):
    """ggml_compute_forward_rwkv_wkv7_f32's vector loops step GGML_F32_STEP floats along a state row with no tail (ops.cpp:9699, :9713; "There shouldn't be left-overs
    though"): at a head size that is no multiple of it (24, 123) the reference reads and WRITES past the row and past the result -- the CPU backend corrupts its own heap
    (seen as `double free or corruption` when its buffer is freed).  Those cases are checked against the float64 restatement instead, at the same bar."""
    return op != "wkv7" or S % 64 == 0


_REF = {}


def _ref(pkg, ref_be, op, case):
    """the reference result of a case, computed once: the reference CPU backend's, or (_ref_takes) the float64 restatement"""
    if (op, case) not in _REF:
        S, H, tps, n_seqs = case
        data = _data(op, S, H, tps * n_seqs, n_seqs, seed=OPS.index(op) * 1000 + sum(case))
        want = _run(pkg, ref_be, op, S, H, tps * n_seqs, n_seqs, data) if _ref_takes(op, S) else _f64(op, data, S, H, tps, n_seqs)
        _REF[(op, case)] = (data, want)
    return _REF[(op, case)]


def _check(got, want, S, H, T, what):
    n_out = S * H * T
    assert got.size == want.size and np.isfinite(got).all()
    e_o, e_s = nmse(got[:n_out], want[:n_out]), nmse(got[n_out:], want[n_out:])
    print(f"{what}: NMSE outputs {e_o:.3e} states {e_s:.3e}")
    assert e_o <= BAR, f"{what}: outputs NMSE {e_o:.3e} > {BAR}"
    assert e_s <= BAR, f"{what}: states NMSE {e_s:.3e} > {BAR}"


# ------------------------------------------------------------------------------------------------ the three recurrences
@pytest.mark.parametrize("case", CASES + WIDE, ids=lambda c: "S%d_H%d_t%d_s%d" % c)
@pytest.mark.parametrize("op", OPS)
def test_wkv(pkg, be, ref_be, op, case):
    S, H, tps, n_seqs = case
    data, want = _ref(pkg, ref_be, op, case)
    key = {"wkv6": "wkv6_launches", "gla": "gla_launches", "wkv7": "wkv7_launches"}[op]
    n0 = be.get_stat(key)
    got = _run(pkg, be, op, S, H, tps * n_seqs, n_seqs, data)
    assert be.get_stat(key) == n0 + 1
    assert got.size == S * H * (tps * n_seqs + S * n_seqs)
    _check(got, want, S, H, tps * n_seqs, f"{op} {case}")


def test_reference_equals_float64_restatement(pkg, ref_be):
    """(the fixture: the reference computes what the module's kernels restate, and _f64 is a fair stand-in where the reference cannot run) each op on the reference CPU
    backend against _f64: a generic head size for WKV6 / GLA, 64 for all three, two sequences"""
    for op, case in [("wkv6", (24, 2, 5, 3)), ("gla", (24, 2, 5, 3)), ("wkv6", (64, 3, 5, 3)), ("gla", (64, 3, 5, 3)), ("wkv7", (64, 3, 5, 3))]:
        S, H, tps, n_seqs = case
        data, want = _ref(pkg, ref_be, op, case)
        host = _f64(op, data, S, H, tps, n_seqs)
        n_out = S * H * tps * n_seqs
        assert nmse(want[:n_out], host[:n_out]) <= 1e-10 and nmse(want[n_out:], host[n_out:]) <= 1e-10, (op, case)


@pytest.mark.parametrize("S", [64, 24])
@pytest.mark.parametrize("op", OPS)
def test_state_fed_forward(pkg, be, ref_be, op, S):
    """two one-token graphs, the second starting from the state the first wrote, equal ONE two-token graph on the reference (WKV7 at S = 24: _ref_takes)"""
    H = 3
    data = _data(op, S, H, 2, 1, seed=91 + S)
    want = _run(pkg, ref_be, op, S, H, 2, 1, data) if _ref_takes(op, S) else _f64(op, data, S, H, 2, 1)
    tok = lambda d, t: {k: (v if k in ("state", "tf") else v[t:t + 1]) for k, v in d.items()}
    first = _run(pkg, be, op, S, H, 1, 1, tok(data, 0))
    second = _run(pkg, be, op, S, H, 1, 1, dict(tok(data, 1), state=first[S * H:].reshape(1, -1)))
    got = np.concatenate([first[:S * H], second])
    _check(got, want, S, H, 2, f"{op} S={S} two steps")


@pytest.mark.parametrize("op,which", [("wkv6", "v"), ("gla", "state"), ("wkv7", "k")])
def test_operand_off_16_byte_alignment_takes_the_generic_kernel(pkg, be, ref_be, op, which):
    """S = 64, but one operand is a contiguous view that starts 4 bytes into its tensor: the float4 kernels cannot take it, the launcher falls to the generic form"""
    S, H, T = 64, 3, 5
    data = _data(op, S, H, T, 1, seed=404)
    res = []
    for b_ in (be, ref_be):
        c, src, _ = _graph(pkg, b_, op, S, H, T, 1)
        n = src[which].nelements()
        wide = c.new_tensor(F32, n + 4)
        ne = src[which].ne
        src[which] = c.view_3d(wide, ne[0], ne[1], ne[2], ne[0] * 4, ne[0] * ne[1] * 4, 4)
        y = c.rwkv_wkv6(*src.values()) if op == "wkv6" else c.gated_linear_attn(*src.values(), GLA_SCALE) if op == "gla" else c.rwkv_wkv7(*src.values())
        assert be.supports_op(y)
        c.alloc()
        for k, t in src.items():
            b_.tensor_set(wide if k == which else t, np.concatenate([np.zeros(1, np.float32), data[k].ravel(), np.zeros(3, np.float32)]) if k == which else data[k])
        b_.graph_compute(c.graph([y]))
        res.append(b_.tensor_get(y).copy().ravel())
        c.free()
    _check(res[0], res[1], S, H, T, f"{op} unaligned {which}")


# ------------------------------------------------------------------------------------------------ L2_NORM
@pytest.mark.parametrize("eps", [1e-12, 0.1])
@pytest.mark.parametrize("ne0", [1, 64, 200, 4100])
def test_l2_norm(pkg, be, ref_be, ne0, eps):
    """rows on both sides of the wave-per-row / workgroup-per-row threshold, a ragged tail, a 4-D shape; one row is small enough that eps = 0.1 is the divisor"""
    rng = np.random.default_rng(ne0)
    xv = rng.standard_normal((2, 3, 5, ne0)).astype(np.float32)
    xv[1, 2, 4] *= 1e-3 / np.sqrt(ne0)                                          # |row| ~ 1e-3 < 0.1
    res = []
    n0 = be.get_stat("l2_norm_launches")
    for b_ in (be, ref_be):
        c = pkg.Context(b_)
        x = c.new_tensor(F32, ne0, 5, 3, 2)
        y = c.l2_norm(x, eps)
        c.alloc()
        b_.tensor_set(x, xv)
        b_.graph_compute(c.graph())
        res.append(b_.tensor_get(y).copy().reshape(xv.shape))
        c.free()
    assert be.get_stat("l2_norm_launches") == n0 + 1
    x64 = xv.astype(np.float64)
    host = x64 / np.maximum(np.sqrt((x64 ** 2).sum(-1, keepdims=True)), eps)
    assert nmse(res[1], host) <= 1e-12
    if eps == 0.1:
        assert np.abs(host[1, 2, 4]).max() < 0.1                                 # (eps was the divisor: the row is not unit length)
    e = nmse(res[0], res[1])
    assert np.isfinite(res[0]).all() and e <= BAR, f"NMSE {e:.3e} > {BAR}"
    assert nmse(res[0][1, 2, 4], res[1][1, 2, 4]) <= BAR


def test_l2_norm_strided_source_view(pkg, be, ref_be):
    """the source is a view {48, 3, 5} of a wider {200, 5} tensor: rows 64 floats apart in dim 1, 200 apart in dim 2, from a column offset of 8; read through nb1..nb3"""
    xv = np.random.default_rng(6).standard_normal((5, 200)).astype(np.float32)
    res = []
    for b_ in (be, ref_be):
        c = pkg.Context(b_)
        wide = c.new_tensor(F32, 200, 5)
        x = c.view_3d(wide, 48, 3, 5, 64 * 4, wide.nb[1], 8 * 4)
        y = c.l2_norm(x, 1e-12)
        c.alloc()
        b_.tensor_set(wide, xv)
        b_.graph_compute(c.graph())
        res.append(b_.tensor_get(y).copy().reshape(5, 3, 48))
        c.free()
    cut = np.stack([xv[:, 8 + 64 * i:8 + 64 * i + 48] for i in range(3)], axis=1).astype(np.float64)
    assert nmse(res[1], cut / np.sqrt((cut ** 2).sum(-1, keepdims=True))) <= 1e-12
    assert nmse(res[0], res[1]) <= BAR


# ------------------------------------------------------------------------------------------------ supports_op
def test_supports_op_admits_the_model_shapes(pkg, be):
    for op in OPS:
        for S, H, T, n_seqs in [(64, 64, 1, 1), (64, 64, 512, 1), (64, 32, 32, 32), (128, 32, 1, 1), (128, 28, 66, 2), (64, 4, 1, 1), (64, 4, 33, 1)]:
            c, _, y = _graph(pkg, be, op, S, H, T, n_seqs)
            assert be.supports_op(y), (op, S, H, T, n_seqs)
    c = pkg.Context(be)
    for ne in [(64, 64, 1), (64, 4, 33, 2), (4096, 7)]:
        assert be.supports_op(c.l2_norm(c.new_tensor(F32, *ne), 1e-12)), ne


def test_supports_op_admits_the_loaders_probe_without_data(pkg, be):
    """llama-model.cpp:257-271: S = H = n_tokens = n_seqs = 123, a 4-D state {S, n_seqs, S, H}, time_first the file's own {head_size, n_head} weight, no data anywhere"""
    for tf_ne in [(64, 4), (123, 123)]:
        c, src, y = _graph(pkg, be, "wkv6", 123, 123, 123, 123, state_ne=(123, 123, 123, 123), tf_ne=tf_ne)
        assert not y.t.data and not y.t.buffer and not src["k"].t.data
        assert be.supports_op(y), tf_ne


def test_supports_op_refuses_what_has_no_kernel(pkg, be):
    for op in OPS:
        c, _, y = _graph(pkg, be, op, 64, 3, 4, 1, ty=F16)                       # F16 operands (the constructor takes them, as the reference's does)
        assert not be.supports_op(y), op
        c, _, y = _graph(pkg, be, op, 129, 2, 2, 1)                              # S = 129
        assert not be.supports_op(y), op
        c, _, y = _graph(pkg, be, op, 64, 3, 5, 2)                               # 5 tokens, 2 sequences
        assert not be.supports_op(y), op
        c, src, y = _graph(pkg, be, op, 64, 3, 4, 1)                             # a k that is not contiguous (past the constructor's assert)
        assert be.supports_op(y)
        src["k"].t.nb[2] = src["k"].t.nb[2] * 2
        assert not be.supports_op(y), op
    c = pkg.Context(be)
    assert not be.supports_op(c.l2_norm(c.new_tensor(F16, 64, 3), 1e-12))
