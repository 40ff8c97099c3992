"""GGML_OP_ROPE in modes 8 (M-RoPE, ggml_rope_multi of llm_build_qwen2vl) and 24 (vision, clip.cpp's Qwen2-VL tower) on the GPU (-m gpu): every set of
tests/mrope_cases.py through the C-ABI against the same node on the reference CPU backend, per (token, head) row at NMSE <= 1e-7 (the reference's ROPE
bar), and against the float64 restatement at the same bar.  tests/test_mrope_host.py shows on the CPU that a kernel that ignores the sections, swaps two
rows, never reads p_e, forgets the `% sect_dims`, takes NORMAL pairs for mode 8, pairs vision channels at p + n_dims / 2 or does not restart the vision
thetas moves every row of a token with unequal positions by NMSE >= 1e-2.

test_the_six_sets_are_supported fails without the kernel: the backend used to leave both modes to the CPU."""
import numpy as np
import pytest

import mrope_cases as mc

pytestmark = pytest.mark.gpu

NAMES = list(mc.SETS)


@pytest.fixture(scope="module")
def reference(pkg, ref_be):
    """the reference backend's rows of (set, T, ne3), computed once and shared: the source's layout and an in-place destination do not change them"""
    memo = {}

    def rows(name, T, n3=1):
        if (name, T, n3) not in memo:
            v = mc.SETS[name]
            x, pos, ff = mc.case(v, T, n3)
            y = mc.run_op(pkg, ref_be, v, x, pos, ff)
            y.setflags(write=False)
            memo[(name, T, n3)] = y
        return memo[(name, T, n3)]
    return rows


def _node(pkg, be, v, T=2, H=3, n3=1, sections=None, n_dims=None, n_pos=None, type_=None, mode=None, n_ff=None):
    """an unallocated ROPE node (supports_op decides from types, shapes and parameters only)"""
    c = pkg.Context(be)
    X = c.new_tensor(pkg.GGML_TYPE_F32 if type_ is None else type_, v.D, H, T, n3)
    P = c.new_tensor(pkg.GGML_TYPE_I32, 4 * T)
    FF = c.new_tensor(pkg.GGML_TYPE_F32, n_ff) if n_ff else None
    kw = mc.rope_kwargs(v)
    kw.update(sections=v.sections if sections is None else sections, n_dims=v.n_dims if n_dims is None else n_dims, mode=v.mode if mode is None else mode)
    Y = c.rope_multi(X, P, FF, **kw)
    if n_pos is not None:
        P.t.ne[0] = n_pos
    return c, Y


def test_the_six_sets_are_supported(pkg, be):
    assert len(mc.SETS) >= 6
    for name, v in mc.SETS.items():
        for T in (1, 9):
            c, Y = _node(pkg, be, v, T=T, n_ff=mc.n_pairs(v) if v.ff else None)
            assert be.supports_op(Y), (name, T)
            c.free()


def test_what_the_reference_would_abort_on_or_the_kernel_cannot_read_is_refused(pkg, be):
    q, vit = mc.SETS["q2vl"], mc.SETS["vit"]
    refused = {
        "all-zero sections": _node(pkg, be, q, sections=(0, 0, 0, 0)),
        "only the fourth section": _node(pkg, be, q, sections=(0, 0, 0, 8)),
        "sect_dims > ne0": _node(pkg, be, mc.SETS["extra"], sections=(24, 24, 24, 0)),
        "vision with n_dims != ne0 / 2": _node(pkg, be, vit, n_dims=20),
        "a position tensor of ne2 entries": _node(pkg, be, q, T=2, n_pos=2),
        "a position tensor of ne2 entries, vision": _node(pkg, be, vit, T=2, n_pos=2),
        "F16": _node(pkg, be, q, type_=pkg.GGML_TYPE_F16),
        "F16, vision": _node(pkg, be, vit, type_=pkg.GGML_TYPE_F16),
        "mode 10 (MROPE | NEOX)": _node(pkg, be, q, mode=10),
        "mode 16": _node(pkg, be, q, mode=16),
        "frequency factors short of the rotated pairs": _node(pkg, be, q, n_ff=q.n_dims // 2 - 1),
        "vision factors short of the rotated pairs": _node(pkg, be, vit, n_ff=vit.n_dims // 2),
    }
    for why, (c, Y) in refused.items():
        assert not be.supports_op(Y), why
        c.free()
    c, Y = _node(pkg, be, q, n_ff=q.n_dims // 2)                           # exactly n_dims / 2 factors: supported
    assert be.supports_op(Y)
    c.free()


def _check(tag, got, want, f64):
    e, at = mc.worst_row(got, want)
    e64, at64 = mc.worst_row(got, f64)
    print(f"{tag}: worst (token, head) row NMSE vs the reference backend {e:.3e} at {at}, vs float64 {e64:.3e} at {at64}")
    assert np.isfinite(got).all(), tag
    assert e <= mc.BAR, (tag, e, at)
    assert e64 <= mc.BAR, (tag, e64, at64)


@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("name", NAMES)
def test_set_against_the_reference_backend(pkg, be, reference, name, T):
    """3 heads, one token and nine; the yarn set's frequency factors are a tensor of exactly n_dims / 2 entries"""
    v = mc.SETS[name]
    x, pos, ff = mc.case(v, T)
    assert ff is None or len(ff) == v.n_dims // 2
    got = mc.run_op(pkg, be, v, x, pos, ff)
    _check(f"{name} T {T}", got, reference(name, T), mc.mrope_f64(v, x, pos, ff))
    if v.mode == mc.MROPE and v.n_dims < v.D:
        assert np.array_equal(got[..., v.n_dims:].view(np.uint32), x[..., v.n_dims:].view(np.uint32)), (name, "pass-through channels")


@pytest.mark.parametrize("form", ["strided", "inplace"])
@pytest.mark.parametrize("name", NAMES)
def test_strided_source_and_in_place(pkg, be, reference, name, form):
    """the source a view into a wider tensor (rows of D + 16 floats, heads 1 .. 3 of 5; the bytes around it are checked untouched), and the destination the source"""
    v = mc.SETS[name]
    x, pos, ff = mc.case(v, 9)
    got = mc.run_op(pkg, be, v, x, pos, ff, form)
    _check(f"{name} T 9 {form}", got, reference(name, 9), mc.mrope_f64(v, x, pos, ff))


@pytest.mark.parametrize("name", NAMES)
def test_two_batches_share_the_positions(pkg, be, reference, name):
    """ne3 = 2: both batches rotate with the same 4 x ne2 positions"""
    v = mc.SETS[name]
    x, pos, ff = mc.case(v, 9, 2)
    got = mc.run_op(pkg, be, v, x, pos, ff)
    _check(f"{name} T 9 ne3 2", got, reference(name, 9, 2), mc.mrope_f64(v, x, pos, ff))
