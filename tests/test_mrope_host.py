"""The M-RoPE / vision sets of tests/mrope_cases.py on the CPU: the float64 restatement agrees with ggml_rope_multi on the reference CPU backend per
(token, head) row within the reference's ROPE bar (NMSE 1e-7), and every mistake of mc.MUTATIONS moves every row of a token whose four positions differ
by NMSE >= rope_variants.SHARP (1e-2): the inputs of the GPU tests are sharp enough to see each of them.  The measured minima are printed."""
import numpy as np
import pytest

import mrope_cases as mc

NAMES = list(mc.SETS)


def test_the_sets_and_positions_are_the_ones_asked_for():
    want = {"q2vl": (128, 128, (16, 24, 24, 0), 8), "wrap": (128, 32, (2, 3, 3, 0), 8), "extra": (64, 64, (8, 8, 8, 8), 8), "yarn": (128, 128, (16, 24, 24, 0), 8),
            "vit": (80, 40, (20, 20, 20, 20), 24), "vit_xy": (80, 40, (20, 20, 0, 0), 24)}
    assert {n: (v.D, v.n_dims, v.sections, v.mode) for n, v in mc.SETS.items() if n in want} == want
    gap = mc.SETS["vit_gap"]                                                                  # one more: an empty leading section, a wrapping vision split, rows w and e
    assert gap.mode == 24 and gap.sections[0] == 0 and sum(gap.sections) < gap.n_dims and all(mc._reaches(gap, k) for k in (1, 2, 3))
    y = mc.SETS["yarn"]
    assert (y.freq_scale, y.ext_factor, y.ff) == (0.25, 1.0, True) and len(mc.freq_factors(y)) == y.n_dims // 2
    pos = mc.POS9
    for t in range(pos.shape[1]):
        p = np.sort(pos[:, t])
        assert np.all(p == p[0]) or np.all(np.diff(p) >= 16), (t, pos[:, t])
    assert (~mc.unequal(pos)).sum() == 1 and not mc.unequal(mc.positions(5))[3]               # one text token, inside the 5-token layer case
    assert {0, 16, 17, 63, 64} <= set(pos.ravel().tolist()) and pos.max() > 4000 and mc.positions(1).max() > 4000
    assert not any(np.all(np.diff(r) > 0) for r in pos)
    # every mistake is applicable somewhere, and each set sees the ones the issue names for it
    assert {m for v in mc.SETS.values() for m in mc.mutations_of(v)} == set(mc.MUTATIONS)
    assert "no_wrap" in mc.mutations_of(mc.SETS["wrap"]) and "e_never_read" in mc.mutations_of(mc.SETS["extra"])
    for n in ("vit", "vit_xy"):
        assert {"vision_half_pairs", "vision_no_reset"} <= set(mc.mutations_of(mc.SETS[n]))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_agrees_with_the_reference_backend_per_row(pkg, ref_be, name):
    v = mc.SETS[name]
    for T, n3, form in ((9, 1, "plain"), (1, 1, "plain"), (9, 2, "plain"), (9, 1, "strided"), (9, 1, "inplace")):
        x, pos, ff = mc.case(v, T, n3)
        ref = mc.run_op(pkg, ref_be, v, x, pos, ff, form)
        e, at = mc.worst_row(mc.mrope_f64(v, x, pos, ff), ref)
        print(f"{name} T {T} ne3 {n3} {form}: worst row NMSE restatement vs reference backend {e:.3e} at {at}")
        assert np.isfinite(ref).all() and e <= mc.BAR, (name, T, n3, form, e, at)
        if v.mode == mc.MROPE and v.n_dims < v.D:
            assert np.array_equal(ref[..., v.n_dims:], x[..., v.n_dims:])                     # pass-through, bit for bit


@pytest.mark.parametrize("name", NAMES)
def test_every_mutation_moves_every_row_of_a_token_with_unequal_positions(name):
    v = mc.SETS[name]
    muts = mc.mutations_of(v)
    assert len(muts) >= 3, muts
    for T in (9, 5, 1):
        x, pos, ff = mc.case(v, T)
        good = mc.mrope_f64(v, x, pos, ff)
        rows = mc.unequal(pos)
        assert rows.sum() >= T - 1 and rows.sum() >= 1
        for m in muts:
            e = mc.row_nmse(mc.mrope_f64(v, x, pos, ff, mutation=m), good)
            print(f"{name} / {m} (T {T}): least row NMSE over tokens with unequal positions {e[rows].min():.3e}")
            assert e[rows].min() >= mc.SHARP, (name, m, T, float(e[rows].min()))
            if m in ("sections_ignored", "h_w_swapped", "e_never_read") and (~rows).any():
                assert e[~rows].max() == 0.0                                                  # the text token: one position, nothing to confuse
