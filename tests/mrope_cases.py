"""M-RoPE (GGML_ROPE_TYPE_MROPE = 8) and vision (GGML_ROPE_TYPE_VISION = 24) parameter sets for the rotation parity tests (a plain helper module in the
style of tests/rope_variants.py, whose signal, row_nmse, worst_row, cos_sin conventions, BAR and SHARP it reuses; used by test_mrope_host.py and the
test_mrope_*_gpu.py files).

mrope_f64() restates the reference's ggml_compute_forward_rope_f32 with ggml_mrope_cache_init (ggml-cpu/ops.cpp) for ggml_rope_multi nodes: four position
rows (t, h, w, e) per token, the row of a rotation pair chosen by the pair's sector = pair % sum(sections); the four thetas multiplied up sequentially in
f32 (as the reference's cache does), in vision mode put back to their position where their section starts; ramp, magnitude, cos / sin and the rotation
in float64.  Mode 8 rotates NEOX pairs (p, p + n_dims / 2) and passes the channels past n_dims through; mode 24 has n_dims == D / 2 and rotates
(p, p + n_dims) for every p < n_dims.

MUTATIONS are that restatement with one mistake a kernel or a fused site could make; test_mrope_host.py shows that each moves every row of a token whose
four positions differ by NMSE >= rope_variants.SHARP.

The sets are the smallest that still separate the mistakes.  The issue that asked for them left freq_base open: q2vl / yarn take Qwen2-VL's 1e6 and the two
vision sets clip.cpp's 1e4.  `wrap` (n_dims 32 of 128, sectors wrapping twice) takes 100 and `extra` 10: at 1e6 the pairs of wrap's second lap and of extra's
fourth section turn by less than 1e-3 rad per position, and forgetting the `% sect_dims` or never reading p_e moved a row by 1e-8 -- the base was changed,
not the floor."""
import types

import numpy as np

import rope_variants as rv

MROPE, VISION = 8, 24                     # GGML_ROPE_TYPE_MROPE / _VISION
BAR, SHARP = rv.BAR, rv.SHARP
signal, row_nmse, worst_row = rv.signal, rv.row_nmse, rv.worst_row


def _s(D, n_dims, sections, mode, freq_base, n_ctx_orig=32768, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, ff=False):
    return types.SimpleNamespace(D=D, n_dims=n_dims, sections=tuple(sections), mode=mode, n_ctx_orig=n_ctx_orig, freq_base=freq_base, freq_scale=freq_scale,
                                 ext_factor=ext_factor, attn_factor=attn_factor, ff=ff, beta_fast=rv.BETA_FAST, beta_slow=rv.BETA_SLOW)


SETS = {
    "q2vl":   _s(128, 128, (16, 24, 24, 0), MROPE, 1e6),                                       # the models' own split
    "wrap":   _s(128, 32, (2, 3, 3, 0), MROPE, 100.0),                                         # sectors wrap twice; 96 channels pass through
    "extra":  _s(64, 64, (8, 8, 8, 8), MROPE, 10.0),                                           # the fourth row is read
    "yarn":   _s(128, 128, (16, 24, 24, 0), MROPE, 1e6, freq_scale=0.25, ext_factor=1.0, ff=True),
    "vit":    _s(80, 40, (20, 20, 20, 20), VISION, 1e4),                                       # clip.cpp's sections (d_head / 4 each)
    "vit_xy": _s(80, 40, (20, 20, 0, 0), VISION, 1e4),                                         # the op harness's form
    # beyond the six the issue names: the two above reach rows t and h only and never wrap.  Here sect_dims 20 < 40 pairs (two laps), rows h, w and e are
    # reached in vision mode, and the empty t section shares its start with h, so the reference's else-if chain never puts theta_h back (it counts on from pair 0)
    "vit_gap": _s(80, 40, (0, 8, 6, 6), VISION, 1e4),
}
for _name, _set in SETS.items():
    _set.name = _name

# [4, 9]: rows t, h, w, e; per token the four values are distinct and at least 16 apart -- in fact hundreds apart: at Qwen2-VL's base 1e6 the h and w sections
# start at pairs that turn by 0.03 and 0.006 rad per position (a quarter of that under the yarn set), so positions 16 apart could not move a row by SHARP --
# except token 3 (the text case: all equal).  0, 16 / 17, 63 / 64 and values beyond 4000 occur; no row ascends.  The h row holds no 0: in vision mode a
# thetas-not-reset mistake leaves an h section at position 0 unrotated either way
POS9 = np.array([[64, 0, 5000, 33, 16, 1023, 2200, 300, 63],
                 [4097, 2000, 1200, 33, 1800, 63, 800, 3000, 4500],
                 [1500, 900, 6400, 33, 3500, 2500, 0, 1600, 17],
                 [2900, 3100, 17, 33, 700, 4001, 5100, 64, 2400]], np.int32)
HEADS = 3


def positions(T):
    """[4, T] i32, the first T tokens of POS9 (T = 1: one beyond 4000 in it; T >= 4 holds the text token)"""
    assert 1 <= T <= POS9.shape[1]
    return np.ascontiguousarray(POS9[:, :T])


def unequal(pos):
    """the tokens whose four positions are not all the same"""
    return ~np.all(pos == pos[:1], axis=0)


def n_pairs(v):
    """rotated pairs of a row: the frequency factors the kernel may read"""
    return v.n_dims if v.mode == VISION else v.n_dims // 2


def freq_factors(v):
    """exactly n_pairs(v) f32, distinct per pair, uniform in [1.5, 8]; None for a set without"""
    if not v.ff:
        return None
    ff = np.random.default_rng(3000 + v.D).uniform(1.5, 8.0, n_pairs(v)).astype(np.float32)
    assert len(np.unique(ff)) == len(ff)
    return ff


def rope_kwargs(v):
    """the keyword arguments of Context.rope_multi"""
    return dict(n_dims=v.n_dims, sections=v.sections, mode=v.mode, n_ctx_orig=v.n_ctx_orig, freq_base=v.freq_base, freq_scale=v.freq_scale,
                ext_factor=v.ext_factor, attn_factor=v.attn_factor, beta_fast=v.beta_fast, beta_slow=v.beta_slow)


def case(v, T, n3=1):
    """(x [n3 * T, HEADS, D] f32, pos [4, T], ff)"""
    return signal(n3 * T, HEADS, v.D, off=float(sum(map(ord, v.name)) % 7)), positions(T), freq_factors(v)


# ---------------------------------------------------------------------------------------------------------------- the float64 restatement
def _reaches(v, k):
    """does some rotated pair lie in section k?"""
    b = np.concatenate([[0], np.cumsum(v.sections)])
    sect = np.arange(n_pairs(v)) % b[4]
    return bool(((sect >= b[k]) & (sect < b[k + 1])).any())


MUTATIONS = {
    # name: (applies to the set, what the mistake is)
    "sections_ignored":  (lambda v: True, "every pair takes p_t"),
    "h_w_swapped":       (lambda v: _reaches(v, 1) or _reaches(v, 2), "the h and w rows swapped"),
    "e_never_read":      (lambda v: _reaches(v, 3), "p_e never read: the fourth section rotates with p_t"),
    "no_wrap":           (lambda v: n_pairs(v) > sum(v.sections), "sector taken without the % sect_dims"),
    "normal_pairs":      (lambda v: v.mode == MROPE, "mode 8 rotated with NORMAL pairs (2 p, 2 p + 1): the mode value has the NEOX bit clear"),
    "vision_half_pairs": (lambda v: v.mode == VISION, "vision pairs taken at p + n_dims / 2"),
    "vision_no_reset":   (lambda v: v.mode == VISION, "vision thetas not put back to the position at a section start"),
}


def mutations_of(v):
    return [m for m, (applies, _) in MUTATIONS.items() if applies(v)]


def cos_sin(v, pos, ff=None, mutation=None):
    """ggml_mrope_cache_init + rope_yarn: (cos, sin) * mscale, float64 [T, n_pairs]"""
    if mutation is not None:
        assert MUTATIONS[mutation][0](v), (v.name, mutation)
    pos = np.asarray(pos)
    if mutation == "sections_ignored":
        pos = np.stack([pos[0]] * 4)
    elif mutation == "h_w_swapped":
        pos = pos[[0, 2, 1, 3]]
    elif mutation == "e_never_read":
        pos = pos[[0, 1, 2, 0]]
    vision = v.mode == VISION
    indep = vision and mutation != "vision_no_reset"
    npair = n_pairs(v)
    s = v.sections
    sect_dims, sec_w, sec_e = s[0] + s[1] + s[2] + s[3], s[0] + s[1], s[0] + s[1] + s[2]
    theta_scale = np.float32(np.float64(np.float32(v.freq_base)) ** np.float64(np.float32(-2.0) / np.float32(v.n_dims)))     # powf, as rope_variants.cos_sin
    corr0, corr1 = rv.yarn_corr_dims(v.n_dims, v.n_ctx_orig, v.freq_base, v.beta_fast, v.beta_slow)
    base = pos.astype(np.float32)                                      # [4, T]
    th4 = base.copy()
    theta = np.empty((pos.shape[1], npair), np.float32)
    for p in range(npair):
        sector = p if mutation == "no_wrap" else p % sect_dims
        if indep:                                                      # the reference's else-if chain: one reset per pair at the most
            if sector == 0:
                th4[0] = base[0]
            elif sector == s[0]:
                th4[1] = base[1]
            elif sector == sec_w:
                th4[2] = base[2]
            elif sector == sec_e:
                th4[3] = base[3]
        row = 0
        if s[0] <= sector < sec_w:
            row = 1
        elif sec_w <= sector < sec_w + s[2]:
            row = 2
        elif sector >= sec_w + s[2]:
            row = 3
        theta[:, p] = th4[row]
        th4 = (th4 * theta_scale).astype(np.float32)                   # all four, sequentially in f32
    f = np.ones(npair, np.float32) if ff is None else np.asarray(ff, np.float32)[:npair]
    theta_extrap = (theta / f[None, :]).astype(np.float32).astype(np.float64)
    theta_interp = np.float64(np.float32(v.freq_scale)) * theta_extrap
    th, mscale = theta_interp, np.float64(np.float32(v.attn_factor))
    if v.ext_factor != 0.0:
        y = (np.arange(npair, dtype=np.float64) - corr0) / max(0.001, corr1 - corr0)
        ramp_mix = (1.0 - np.minimum(1.0, np.maximum(0.0, y))) * v.ext_factor
        th = theta_interp * (1.0 - ramp_mix)[None, :] + theta_extrap * ramp_mix[None, :]
        mscale = mscale * (1.0 + 0.1 * np.log(1.0 / np.float64(np.float32(v.freq_scale))))
    return np.cos(th) * mscale, np.sin(th) * mscale


def mrope_f64(v, x, pos, ff=None, mutation=None):
    """x [n3 * T, n_head, D] (token index fastest within a batch: row i uses the positions of token i % T) -> float64"""
    pos = np.asarray(pos)
    T = pos.shape[1]
    c, s = cos_sin(v, pos, ff, mutation)
    x = np.asarray(x, np.float64)
    reps = x.shape[0] // T
    assert reps * T == x.shape[0]
    c, s = np.tile(c, (reps, 1))[:, None, :], np.tile(s, (reps, 1))[:, None, :]
    y = x.copy()
    n = v.n_dims
    if v.mode == VISION and mutation != "vision_half_pairs":
        assert 2 * n == v.D
        x0, x1 = x[..., :n], x[..., n:2 * n]
        y[..., :n] = x0 * c - x1 * s
        y[..., n:2 * n] = x0 * s + x1 * c
    elif v.mode == VISION:                                             # the mistake: NEOX pairing of n_dims channels, the rest left alone
        h = n // 2
        x0, x1 = x[..., :h], x[..., h:n]
        y[..., :h] = x0 * c[..., :h] - x1 * s[..., :h]
        y[..., h:n] = x0 * s[..., :h] + x1 * c[..., :h]
    elif mutation == "normal_pairs":
        x0, x1 = x[..., 0:n:2], x[..., 1:n:2]
        y[..., 0:n:2] = x0 * c - x1 * s
        y[..., 1:n:2] = x0 * s + x1 * c
    else:
        h = n // 2
        x0, x1 = x[..., :h], x[..., h:n]
        y[..., :h] = x0 * c - x1 * s
        y[..., h:n] = x0 * s + x1 * c
    return y


# ---------------------------------------------------------------------------------------------------------------- one ROPE node through the C-ABI
def run_op(pkg, backend, v, x, pos, ff, form="plain"):
    """x [n3 * T, H, D] through one ggml_rope_multi node on `backend`; form: plain | strided (the source a view of a wider tensor) | inplace.  -> f32 like x"""
    F32, I32 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_I32
    T = pos.shape[1]
    n3, H, D = x.shape[0] // T, x.shape[1], x.shape[2]
    c = pkg.Context(backend)
    P = c.new_tensor(I32, 4 * T)
    FF = c.new_tensor(F32, len(ff)) if ff is not None else None
    if form == "strided":                                              # heads 1 .. H of H + 2, in rows of D + 16 floats
        W = c.new_tensor(F32, D + 16, H + 2, T, n3)
        X = c.view_4d(W, D, H, T, n3, W.nb[1], W.nb[2], W.nb[3], W.nb[1] + 8 * 4)
        wide = np.full((n3 * T, H + 2, D + 16), 7.0, np.float32)
        wide[:, 1:H + 1, 8:8 + D] = x
        feed = (W, wide)
    else:
        X = c.new_tensor(F32, D, H, T, n3)
        feed = (X, x)
    Y = c.rope_multi(X, P, FF, inplace=form == "inplace", **rope_kwargs(v))
    c.alloc()
    backend.tensor_set(feed[0], feed[1])
    backend.tensor_set(P, np.ascontiguousarray(pos, np.int32))
    if FF is not None:
        backend.tensor_set(FF, ff)
    ok = backend.supports_op(Y) if hasattr(backend, "dev_s") and backend.dev_s else True
    assert ok, (v.name, form, "the backend refuses the node")
    backend.graph_compute(c.graph())
    y = backend.tensor_get(Y).copy().reshape(x.shape)
    if form == "strided":                                              # the source is left as it was
        assert np.array_equal(backend.tensor_get(W).reshape(wide.shape), wide)
    c.free()
    return y
