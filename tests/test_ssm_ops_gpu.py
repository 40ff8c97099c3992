"""State-space ops on the GPU (`-m gpu`): SSM_CONV and SSM_SCAN (kernels/ssm.hip) and the recurrent layers of llama.cpp-omni_amd/mamba.py, each through the
backend C-ABI and against the reference CPU backend (oracle/ref_backend.py) on the same graph.

Bars: the two ops -- NMSE <= 1e-7, the default max_nmse_err of the reference's own harness (test-backend-ops.cpp:996), which both ops inherit; for the scan it is
taken SEPARATELY over the y part and the state part of the result.  The layers -- NMSE <= 1e-6 for the layer output (three block-quantised mat-muls in a chain,
each with a harness bar of 5e-4; the same weights and the same integer stages run on both sides) and <= 1e-7 for both written-back states.
Shapes: channel counts that are no multiple of the conv tile (200), token counts on both sides of the token / tile kernel threshold and across a 64-token time
tile (1, 5, 67); for the scan every d_state the kernel is instantiated for that the issue names, head_dim 1 (Mamba-1, one decay per state element), a head_dim
that the rows a wave holds do not divide (20), two groups, and state rows picked through ids out of a larger table."""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu

F32, F16, I32 = 0, 1, 26
BAR = 1e-7


def _run(be_, c, outs, feeds, nodes=None):
    c.alloc()
    for t, v in feeds:
        be_.tensor_set(t, v)
    be_.graph_compute(c.graph(nodes))
    res = [be_.tensor_get(o).copy() for o in outs]
    c.free()
    return res


# ------------------------------------------------------------------------------------------------ graphs
def _conv_graph(pkg, be_, d_conv, d_inner, n_t, n_s, ty=F32):
    c = pkg.Context(be_)
    sx = c.new_tensor(ty, d_conv - 1 + n_t, d_inner, n_s)
    w = c.new_tensor(F32, d_conv, d_inner)
    return c, sx, w, c.ssm_conv(sx, w)


def _scan_graph(pkg, be_, shape, n_t, n_s, a_ne0=None, n_rows=5, x_type=F32):
    """x, B, C: views of one wider [d_inner + 2 * n_group * d_state, n_t, n_s] tensor, cut as build_mamba2_layer cuts xBC"""
    d_state, head_dim, n_head, n_group = shape
    d_inner = head_dim * n_head
    c = pkg.Context(be_)
    es = 2 if x_type == F16 else 4
    xBC = c.new_tensor(x_type, d_inner + 2 * n_group * d_state, n_t, n_s)
    x = c.view_4d(xBC, head_dim, n_head, n_t, n_s, head_dim * es, xBC.nb[1], xBC.nb[2], 0)
    B = c.view_4d(xBC, d_state, n_group, n_t, n_s, d_state * es, xBC.nb[1], xBC.nb[2], d_inner * es)
    C_ = c.view_4d(xBC, d_state, n_group, n_t, n_s, d_state * es, xBC.nb[1], xBC.nb[2], (d_inner + n_group * d_state) * es)
    s = c.new_tensor(F32, d_state, head_dim, n_head, n_rows)
    dt = c.new_tensor(F32, n_head, n_t, n_s)
    A = c.new_tensor(F32, a_ne0 if a_ne0 else (d_state if head_dim == 1 else 1), n_head)
    ids = c.new_tensor(I32, n_s)
    y = c.ssm_scan(s, x, dt, A, B, C_, ids)
    return c, dict(xBC=xBC, s=s, dt=dt, A=A, ids=ids), y


def _scan_data(shape, n_t, n_s, seed, a_ne0=None, n_rows=5, dt_const=None):
    d_state, head_dim, n_head, n_group = shape
    rng = np.random.default_rng(seed)
    W = head_dim * n_head + 2 * n_group * d_state
    return dict(xBC=rng.standard_normal((n_s, n_t, W)).astype(np.float32), s=rng.standard_normal((n_rows, n_head, head_dim, d_state)).astype(np.float32),
                dt=(np.full((n_s, n_t, n_head), dt_const) if dt_const is not None else rng.uniform(-2.0, 2.0, (n_s, n_t, n_head))).astype(np.float32),
                A=rng.uniform(-1.0, -0.05, (n_head, a_ne0 if a_ne0 else (d_state if head_dim == 1 else 1))).astype(np.float32),
                ids=np.array([4, 0, 2][:n_s], np.int32))


def _scan_run(pkg, be_, shape, n_t, n_s, data, a_ne0=None):
    c, T, y = _scan_graph(pkg, be_, shape, n_t, n_s, a_ne0)
    return _run(be_, c, [y], [(T[k], data[k]) for k in T])[0]


def _check_scan(got, want, shape, n_t, n_s, what=""):
    d_state, head_dim, n_head, _ = shape
    ny = head_dim * n_head * n_t * n_s
    assert got.size == want.size == ny + d_state * head_dim * n_head * n_s
    e_y, e_s = nmse(got[:ny], want[:ny]), nmse(got[ny:], want[ny:])
    print(f"ssm_scan {shape} n_t={n_t} n_s={n_s} {what}: NMSE y {e_y:.3e} states {e_s:.3e}")
    assert np.isfinite(got).all()
    assert e_y <= BAR, f"y: NMSE {e_y:.3e} > {BAR}"
    assert e_s <= BAR, f"final states: NMSE {e_s:.3e} > {BAR}"


# ------------------------------------------------------------------------------------------------ supports_op
MODEL_SCANS = [((128, 64, 8, 2), 1, 1), ((128, 64, 8, 2), 512, 1), ((16, 1, 512, 1), 1, 1), ((16, 1, 512, 1), 33, 1), ((128, 64, 80, 1), 1, 32), ((256, 64, 8, 2), 7, 3)]


def test_supports_op_admits_the_model_shapes(pkg, be):
    for d_conv, d_inner, n_t, n_s in [(4, 768, 1, 1), (4, 768, 512, 1), (4, 512, 1, 1), (4, 512, 33, 1), (3, 5376, 1, 32), (4, 5376, 512, 1)]:
        c, _, _, y = _conv_graph(pkg, be, d_conv, d_inner, n_t, n_s)
        c.alloc()
        assert be.supports_op(y), (d_conv, d_inner, n_t, n_s)
        c.free()
    for shape, n_t, n_s in MODEL_SCANS:
        c, _, y = _scan_graph(pkg, be, shape, n_t, n_s, n_rows=max(n_s, 2))
        c.alloc()
        assert be.supports_op(y), (shape, n_t, n_s)
        c.free()


def test_supports_op_needs_no_data_pointer(pkg, be):
    """the loader's probes (llama-model.cpp:233-256) pass tensors with no data and no buffer: admission reads types, shapes and strides only"""
    c, _, _, y = _conv_graph(pkg, be, 4, 768, 1, 1)
    assert not y.t.data and not y.t.buffer and be.supports_op(y)
    c2, _, y2 = _scan_graph(pkg, be, (128, 64, 8, 2), 1, 1)
    assert not y2.t.data and be.supports_op(y2)


def test_supports_op_refuses_what_has_no_kernel(pkg, be):
    c, _, y = _scan_graph(pkg, be, (48, 4, 8, 1), 3, 1)                       # d_state 48
    assert not be.supports_op(y)
    c, _, y = _scan_graph(pkg, be, (128, 64, 8, 2), 3, 1, x_type=F16)        # an F16 x (the constructor takes it, as the reference's does)
    assert not be.supports_op(y)
    c, _, y = _scan_graph(pkg, be, (128, 64, 8, 2), 3, 1)                     # A->ne[0] neither 1 nor d_state (past the constructor's assert)
    y._srcs[3].t.ne[0] = 64
    assert not be.supports_op(y)
    c, _, _, y = _conv_graph(pkg, be, 9, 64, 3, 1)                            # d_conv 9
    assert not be.supports_op(y)
    c, _, _, y = _conv_graph(pkg, be, 4, 64, 3, 1, ty=F16)                    # an F16 sx
    assert not be.supports_op(y)


# ------------------------------------------------------------------------------------------------ SSM_CONV
@pytest.mark.parametrize("n_s", [1, 3])
@pytest.mark.parametrize("n_t", [1, 5, 67])
@pytest.mark.parametrize("d_inner", [200, 1536])
@pytest.mark.parametrize("d_conv", [3, 4])
def test_ssm_conv(pkg, be, ref_be, d_conv, d_inner, n_t, n_s):
    rng = np.random.default_rng(1000 * d_conv + d_inner + 7 * n_t + n_s)
    xv = rng.standard_normal((n_s, d_inner, d_conv - 1 + n_t)).astype(np.float32)
    wv = rng.standard_normal((d_inner, d_conv)).astype(np.float32)
    res = []
    for b_ in (be, ref_be):
        c, sx, w, y = _conv_graph(pkg, b_, d_conv, d_inner, n_t, n_s)
        res.append(_run(b_, c, [y], [(sx, xv), (w, wv)])[0].reshape(n_s, n_t, d_inner))
    win = np.lib.stride_tricks.sliding_window_view(xv.astype(np.float64), d_conv, axis=2)           # [n_s, d_inner, n_t, d_conv]
    host = np.einsum("srtk,rk->str", win, wv.astype(np.float64))
    e = nmse(res[0], res[1])
    assert nmse(res[1], host) <= 1e-12                                                             # (the fixture: the reference computes what the docstring says)
    assert e <= BAR, f"NMSE {e:.3e} > {BAR}"


def test_ssm_conv_launch_counter(pkg, be):
    n0 = be.get_stat("ssm_conv_launches")
    c, sx, w, y = _conv_graph(pkg, be, 4, 64, 2, 1)
    _run(be, c, [y], [(sx, np.ones((1, 64, 5), np.float32)), (w, np.ones((64, 4), np.float32))])
    assert be.get_stat("ssm_conv_launches") == n0 + 1


# ------------------------------------------------------------------------------------------------ SSM_SCAN
SCAN_SHAPES = [(16, 1, 200, 1), (128, 64, 6, 2), (256, 64, 4, 2), (64, 20, 4, 1)]      # (d_state, head_dim, n_head, n_group)


@pytest.mark.parametrize("n_s", [1, 3])
@pytest.mark.parametrize("n_t", [1, 7, 67])
@pytest.mark.parametrize("shape", SCAN_SHAPES)
def test_ssm_scan(pkg, be, ref_be, shape, n_t, n_s):
    data = _scan_data(shape, n_t, n_s, seed=sum(shape) + 31 * n_t + n_s)
    n0 = be.get_stat("ssm_scan_launches")
    got = _scan_run(pkg, be, shape, n_t, n_s, data)
    assert be.get_stat("ssm_scan_launches") == n0 + 1
    _check_scan(got, _scan_run(pkg, ref_be, shape, n_t, n_s, data), shape, n_t, n_s)


@pytest.mark.parametrize("shape,a_ne0", [((128, 64, 6, 2), None), ((16, 1, 200, 1), None), ((64, 20, 4, 1), 64), ((32, 3, 5, 5), None)])
def test_ssm_scan_softplus_linear_branch_and_both_decays(pkg, be, ref_be, shape, a_ne0):
    """dt = 25 > 20: softplus(v) = v; the per-element decay at a head_dim above 1, and d_state 32 with head_dim 3 (one row per sub-group)"""
    data = _scan_data(shape, 7, 3, seed=77, a_ne0=a_ne0, dt_const=25.0)
    _check_scan(_scan_run(pkg, be, shape, 7, 3, data, a_ne0), _scan_run(pkg, ref_be, shape, 7, 3, data, a_ne0), shape, 7, 3, "dt=25")


@pytest.mark.parametrize("shape", [(128, 64, 6, 2), (16, 1, 200, 1)])
def test_ssm_scan_state_carry(pkg, be, ref_be, shape):
    """a scan over 9 tokens == a scan over 5 tokens whose final states are copied into a cache tensor, then a scan over 4 tokens that starts from that cache"""
    d_state, head_dim, n_head, n_group = shape
    n_s, d_inner = 2, head_dim * n_head
    n_state = d_state * d_inner
    data = _scan_data(shape, 9, n_s, seed=5)
    W = data["xBC"].shape[2]

    def run(b_):
        c = pkg.Context(b_)
        xBC = c.new_tensor(F32, W, 9, n_s)
        s = c.new_tensor(F32, d_state, head_dim, n_head, 5)
        A = c.new_tensor(F32, data["A"].shape[1], n_head)
        ids, ids2 = c.new_tensor(I32, n_s), c.new_tensor(I32, n_s)
        dts = {n: c.new_tensor(F32, n_head, n, n_s) for n in (9, 5, 4)}
        cache = c.new_tensor(F32, n_state * 3)

        def cut(t0, n):
            o = t0 * xBC.nb[1]
            return (c.view_4d(xBC, head_dim, n_head, n, n_s, head_dim * 4, xBC.nb[1], xBC.nb[2], o),
                    c.view_4d(xBC, d_state, n_group, n, n_s, d_state * 4, xBC.nb[1], xBC.nb[2], o + d_inner * 4),
                    c.view_4d(xBC, d_state, n_group, n, n_s, d_state * 4, xBC.nb[1], xBC.nb[2], o + (d_inner + n_group * d_state) * 4))
        x9, B9, C9 = cut(0, 9)
        y9 = c.ssm_scan(s, x9, dts[9], A, B9, C9, ids)
        x5, B5, C5 = cut(0, 5)
        y5 = c.ssm_scan(s, x5, dts[5], A, B5, C5, ids)
        store = c.cpy(c.view_1d(y5, n_state * n_s, x5.nelements() * 4), c.view_1d(cache, n_state * n_s, n_state * 4))      # cache rows 1, 2
        x4, B4, C4 = cut(5, 4)
        y4 = c.ssm_scan(c.reshape(c.view_1d(store, n_state * n_s, 0), d_state, head_dim, n_head, n_s), x4, dts[4], A, B4, C4, ids2)
        feeds = [(xBC, data["xBC"]), (s, data["s"]), (A, data["A"]), (ids, data["ids"]), (ids2, np.arange(n_s, dtype=np.int32)), (cache, np.zeros(n_state * 3, np.float32)),
                 (dts[9], data["dt"]), (dts[5], np.ascontiguousarray(data["dt"][:, :5])), (dts[4], np.ascontiguousarray(data["dt"][:, 5:]))]
        return _run(b_, c, [y9, y5, y4], feeds)

    g9, g5, g4 = run(be)
    r9, r5, r4 = run(ref_be)
    _check_scan(g9, r9, shape, 9, n_s, "9 tokens")
    _check_scan(g4, r4, shape, 4, n_s, "4 tokens from the cache")
    ny = d_inner * n_s
    y9 = g9[:ny * 9].reshape(n_s, 9, d_inner)
    y54 = np.concatenate([g5[:ny * 5].reshape(n_s, 5, d_inner), g4[:ny * 4].reshape(n_s, 4, d_inner)], axis=1)
    assert nmse(y54, y9) <= BAR and nmse(g4[ny * 4:], g9[ny * 9:]) <= BAR
    assert nmse(y54, r9[:ny * 9].reshape(n_s, 9, d_inner)) <= BAR and nmse(g4[ny * 4:], r9[ny * 9:]) <= BAR


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("n_t", [1, 3])
def test_ssm_scan_operands_made_in_graph(pkg, be, ref_be, n_t, fusion):
    """dt, B and C each behind RMS_NORM -> MUL, dt behind a CONT as well, in one graph with the scan (Falcon-Mamba / Jamba put the norms there): the deferred norm,
    the lazy copy and the copy queue are live in front of the launch"""
    d_state, n_head, R = 16, 256, 256                                           # Mamba-1 form: head_dim 1, dt_rank == n_head here
    rng = np.random.default_rng(9 + n_t)
    xdb = rng.standard_normal((1, n_t, R + 2 * d_state)).astype(np.float32)
    xv = rng.standard_normal((1, n_t, n_head)).astype(np.float32)
    sv = rng.standard_normal((5, n_head, 1, d_state)).astype(np.float32)
    Av = rng.uniform(-1.0, -0.05, (n_head, d_state)).astype(np.float32)
    wn = [rng.uniform(0.5, 1.5, k).astype(np.float32) for k in (R, d_state, d_state)]

    def run(b_):
        c = pkg.Context(b_)
        x_db = c.new_tensor(F32, R + 2 * d_state, n_t, 1)
        x = c.new_tensor(F32, 1, n_head, n_t, 1)
        s = c.new_tensor(F32, d_state, 1, n_head, 5)
        A = c.new_tensor(F32, d_state, n_head)
        ids = c.new_tensor(I32, 1)
        w = [c.new_tensor(F32, k) for k in (R, d_state, d_state)]
        dt = c.view_3d(x_db, R, n_t, 1, x_db.nb[1], x_db.nb[2], 0)
        B = c.view_4d(x_db, d_state, 1, n_t, 1, d_state * 4, x_db.nb[1], x_db.nb[2], 4 * R)
        C_ = c.view_4d(x_db, d_state, 1, n_t, 1, d_state * 4, x_db.nb[1], x_db.nb[2], 4 * (R + d_state))
        dt = c.cont(c.mul(c.rms_norm(dt, 1e-5), w[0]))
        B = c.mul(c.rms_norm(B, 1e-5), w[1])
        C_ = c.mul(c.rms_norm(C_, 1e-5), w[2])
        y = c.ssm_scan(s, x, dt, A, B, C_, ids)
        return _run(b_, c, [y], [(x_db, xdb), (x, xv), (s, sv), (A, Av), (ids, np.array([3], np.int32))] + list(zip(w, wn)))[0]

    be.set_option("fusion", fusion)
    try:
        got = run(be)
    finally:
        be.set_option("fusion", 1)
    _check_scan(got, run(ref_be), (d_state, 1, n_head, 1), n_t, 1, f"fusion={fusion}")


# ------------------------------------------------------------------------------------------------ the two shapes only these graphs produce
@pytest.mark.parametrize("n_t,n_s", [(1, 1), (5, 1), (3, 2)])
def test_grouped_rms_norm_times_a_two_row_weight(pkg, be, ref_be, n_t, n_s):
    """Mamba-2's grouped norm: RMS_NORM over {d_inner / n_group, n_group, n_t, n_s}, MUL by a weight {d_inner / n_group, n_group}: the weight has two rows"""
    rng = np.random.default_rng(3)
    xv = rng.standard_normal((n_s, n_t, 2, 256)).astype(np.float32)
    wv = rng.uniform(0.5, 1.5, (2, 256)).astype(np.float32)
    res = []
    for b_ in (be, ref_be):
        c = pkg.Context(b_)
        x, w = c.new_tensor(F32, 512, n_t, n_s), c.new_tensor(F32, 256, 2)
        y = c.mul(c.rms_norm(c.reshape(x, 256, 2, n_t, n_s), 1e-5), w)
        res.append(_run(b_, c, [y], [(x, xv), (w, wv)])[0])
    host = xv.astype(np.float64) / np.sqrt((xv.astype(np.float64) ** 2).mean(-1, keepdims=True) + 1e-5) * wv
    assert nmse(res[1], host) <= 1e-12
    assert nmse(res[0], res[1]) <= BAR, nmse(res[0], res[1])


@pytest.mark.parametrize("n_t,n_s", [(1, 1), (5, 2)])
def test_mul_of_a_strided_4d_view_by_one_value_per_head(pkg, be, ref_be, n_t, n_s):
    """mamba2_y_add_d: x, a strided view {head_dim, n_head, n_t, n_s} of the conv result, times ssm_d {1, n_head}, added to a dense y of the same shape"""
    head_dim, n_head, W = 64, 8, 768
    rng = np.random.default_rng(4)
    xv = rng.standard_normal((n_s, n_t, W)).astype(np.float32)
    dv = rng.uniform(0.5, 1.5, (n_head, 1)).astype(np.float32)
    yv = rng.standard_normal((n_s, n_t, n_head, head_dim)).astype(np.float32)
    res = []
    for b_ in (be, ref_be):
        c = pkg.Context(b_)
        xBC, d, y = c.new_tensor(F32, W, n_t, n_s), c.new_tensor(F32, 1, n_head), c.new_tensor(F32, head_dim, n_head, n_t, n_s)
        x = c.view_4d(xBC, head_dim, n_head, n_t, n_s, head_dim * 4, xBC.nb[1], xBC.nb[2], 0)
        out = c.add(y, c.mul(x, d))
        res.append(_run(b_, c, [out], [(xBC, xv), (d, dv), (y, yv)])[0])
    host = yv + xv[:, :, :head_dim * n_head].reshape(n_s, n_t, n_head, head_dim).astype(np.float64) * dv
    assert nmse(res[1], host) <= 1e-12
    assert nmse(res[0], res[1]) <= BAR, nmse(res[0], res[1])


# ------------------------------------------------------------------------------------------------ whole layers
@pytest.mark.parametrize("arch,rms", [("mamba2", False), ("mamba", False), ("mamba", True)])
def test_layer_prompt_then_one_token_from_the_cached_states(pkg, be, ref_be, arch, rms):
    """one layer of mamba.py, two steps: a 5-token prompt into a zeroed state row (the zeroing SCALE, the extra-state copy and both write-backs are live), then one
    token from the cached conv and ssm states"""
    from llama_cpp_omni_amd import mamba
    hp = dict(mamba.TINY_MAMBA2 if arch == "mamba2" else mamba.TINY_MAMBA, dt_b_c_rms=rms)
    rng = np.random.default_rng(21)
    steps = [(rng.standard_normal((5, hp["n_embd"])).astype(np.float32), 1), (rng.standard_normal((1, hp["n_embd"])).astype(np.float32), -1)]
    res, weights = [], None
    for b_ in (be, ref_be):
        lay = mamba.MambaLayer(b_, hp, rs_size=3, seed=5, weights=weights)
        weights = lay.weights
        outs = []
        for xv, rs_zero in steps:
            g, x, s_copy, N = lay.build(xv.shape[0], 1, n_rs=2, rs_head=1, rs_zero=rs_zero)
            b_.tensor_set(x, xv)
            b_.tensor_set(s_copy, np.array([1, 0], np.int32))                   # the sequence continues row 1; row 0 is copied onto row 2
            b_.graph_compute(g.graph())
            outs.append((b_.tensor_get(N["out"]).copy(), b_.tensor_get(lay.conv_states).copy(), b_.tensor_get(lay.ssm_states).copy()))
            g.free()
        res.append(outs)
        lay.wctx.free()
    for step, (got, want) in enumerate(zip(*res)):
        e_out, e_conv, e_ssm = nmse(got[0], want[0]), nmse(got[1], want[1]), nmse(got[2], want[2])
        print(f"{arch} rms={rms} step {step}: NMSE out {e_out:.3e} conv states {e_conv:.3e} ssm states {e_ssm:.3e}")
        assert np.isfinite(got[0]).all()
        assert e_out <= 1e-6, f"step {step}: layer output NMSE {e_out:.3e} > 1e-6 (conv states {e_conv:.3e}, ssm states {e_ssm:.3e})"
        assert e_conv <= BAR, f"step {step}: conv states NMSE {e_conv:.3e} > {BAR}"
        assert e_ssm <= BAR, f"step {step}: ssm states NMSE {e_ssm:.3e} > {BAR}"
