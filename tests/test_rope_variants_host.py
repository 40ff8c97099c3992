"""The RoPE variants of tests/rope_variants.py on the CPU: the float64 restatement, the C oracle (orc.rope takes every parameter and the frequency
factors, but was pinned on plain RoPE only) and the fixture tests/golden/rope_variants.npz -- ggml_rope_ext on the reference CPU backend, written by
oracle/make_golden.py gen_rope_variants -- agree per row within the reference's ROPE bar (NMSE 1e-7), and every mistake of rv.MUTATIONS moves
every row at a position >= 16 by NMSE >= 1e-2: the inputs of test_rope_variants_gpu.py are sharp enough to see each of them."""
import os

import numpy as np
import pytest

import rope_variants as rv
from conftest import GOLDEN

NAMES = list(rv.VARIANTS)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "rope_variants.npz"))


def test_variant_table_is_the_one_the_models_need():
    """the three YaRN ramps lie strictly inside (0, D / 2): extrapolated, mixed and interpolated pairs in one row; the control is plain"""
    for name, (lo, hi) in rv.YARN_RAMPS.items():
        v = rv.VARIANTS[name]
        assert rv.yarn_corr_dims(v.D, v.n_ctx_orig, v.freq_base, v.beta_fast, v.beta_slow) == (lo, hi), name
        assert 0 < lo < hi < v.D // 2 - 1
    p = rv.VARIANTS["plain"]
    assert (p.freq_scale, p.ext_factor, p.attn_factor, p.ff) == (1.0, 0.0, 1.0, False)
    for T in (8, 19, 64):
        pos = rv.positions(T)
        assert len(set(pos.tolist())) == T and {0, 16, 17, 63, 64} <= set(pos.tolist()) and pos.max() >= 4000 and not np.all(np.diff(pos) > 0)
    assert {0, 16, 17, 63, 64} <= set(rv.POS8.tolist()) and rv.POS8.max() >= 4000 and not np.all(np.diff(rv.POS8) > 0)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_oracle_and_reference_fixture_agree_per_row(fixture, name):
    import oracle.oracle_py as orc
    v = rv.VARIANTS[name]
    x, pos, ff = rv.small_case(v)
    assert np.array_equal(fixture["pos"], pos)
    if ff is not None:
        assert np.array_equal(fixture[f"ff_{name}"], ff)                # the fixture was generated from the factors the helper makes today
    ref = fixture[f"y_{name}"]
    f64 = rv.rope_f64(v, x, pos, ff)
    c = orc.rope(x, pos, v.D, v.mode, v.n_ctx_orig, v.freq_base, v.freq_scale, v.ext_factor, v.attn_factor, v.beta_fast, v.beta_slow, ff=ff)
    e1, at1 = rv.worst_row(f64, ref)
    e2, at2 = rv.worst_row(c, ref)
    e3, at3 = rv.worst_row(c, f64)
    print(f"{name}: worst row NMSE restatement vs reference {e1:.3e} at {at1}, oracle vs reference {e2:.3e} at {at2}, oracle vs restatement {e3:.3e} at {at3}")
    assert np.isfinite(ref).all() and ref.shape == x.shape
    assert e1 < rv.BAR and e2 < rv.BAR and e3 < rv.BAR, (name, e1, e2, e3)


@pytest.mark.parametrize("name", list(rv.ALL))
def test_every_mutation_moves_every_row_past_position_16(name):
    v = rv.ALL[name]
    muts = rv.mutations_of(v)
    assert "other_freq_base" in muts and (name.startswith("plain") or len(muts) >= 2), muts
    cases = [rv.small_case(v)] + [(rv.signal(T, 2, v.D, off=T), rv.positions(T), rv.freq_factors(v)) for T in (19, 64)]    # the GPU file's positions too
    for x, pos, ff in cases:
        good = rv.rope_f64(v, x, pos, ff)
        far = np.asarray(pos) >= 16
        assert far.sum() >= len(pos) - 1
        for m in muts:
            e = rv.row_nmse(rv.rope_f64(v, x, pos, ff, mutation=m), good)[far]
            print(f"{name} / {m} ({len(pos)} positions): least row NMSE {e.min():.3e}")
            assert e.min() >= rv.SHARP, (name, m, float(e.min()))


def test_partial_rotary_restatement_passes_the_tail_through():
    v = rv.VARIANTS["plain"]
    x, pos, _ = rv.small_case(v)
    y = rv.rope_f64(v, x, pos, n_dims=64)
    assert np.array_equal(y[..., 64:], x[..., 64:].astype(np.float64)) and not np.allclose(y[2, :, :64], x[2, :, :64])
