"""RoPE parameter sets the supported models really use, for the rotation parity tests (a plain helper module, used by test_rope_variants_host.py,
test_rope_variants_gpu.py and oracle/make_golden.py).

Every graph the other tests send through a fused rotation site uses plain RoPE (freq_scale 1, ext_factor 0, attn_factor 1, no frequency factors).
VARIANTS names the forms the models need -- linear scaling, YaRN with its ramp and magnitude correction, an attention factor, frequency factors in
both pair layouts -- with numbers that put the YaRN ramp strictly inside (0, D / 2), so one row holds extrapolated, mixed and interpolated pairs.

rope_f64() restates the reference's ggml_compute_forward_rope_f32 (ggml-cpu/ops.cpp) with rope_yarn, ggml_rope_cache_init and ggml_rope_yarn_corr_dims
(ggml.c).  The angle follows the op's definition -- a float theta_scale multiplied up sequentially in f32, as the reference's cache does: at position
4000 a float64 recurrence would differ from it by more than the bar -- the ramp, magnitude, cos / sin and the rotation are float64.
MUTATIONS are that restatement with one mistake a fused site could make; test_rope_variants_host.py shows that each moves every row at a position
>= 16 by NMSE >= 1e-2, five orders above the bar the GPU tests hold."""
import types

import numpy as np

NORMAL, NEOX = 0, 2                       # GGML_ROPE_TYPE_NORMAL / _NEOX
BETA_FAST, BETA_SLOW = 32.0, 1.0
BAR = 1e-7                                # the reference's NMSE bar for ROPE (test-backend-ops), applied per row
SHARP = 1e-2                              # what every applicable mutation must move every row at a position >= 16 by


def _v(model, D, mode, n_ctx_orig, freq_base, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, ff=False):
    return types.SimpleNamespace(model=model, D=D, mode=mode, n_ctx_orig=n_ctx_orig, freq_base=freq_base, freq_scale=freq_scale, ext_factor=ext_factor,
                                 attn_factor=attn_factor, ff=ff, beta_fast=BETA_FAST, beta_slow=BETA_SLOW)


VARIANTS = {
    "plain":        _v("Qwen3 (the control: what every other test rotates with)", 128, NEOX, 32768, 1e6),
    "linear":       _v("linear position scaling, factor 4", 128, NEOX, 32768, 1e6, freq_scale=0.25),
    "yarn4":        _v("long-context Qwen3: YaRN, factor 4", 128, NEOX, 32768, 1e6, freq_scale=0.25, ext_factor=1.0),
    "yarn32_d64":   _v("gpt-oss: YaRN, factor 32, head size 64", 64, NEOX, 4096, 150000.0, freq_scale=1.0 / 32.0, ext_factor=1.0),
    "attn_factor":  _v("an attention factor alone", 128, NEOX, 32768, 1e6, attn_factor=1.3466),
    "ff_norm_d64":  _v("Llama-3.x: rope_freqs frequency factors, NORMAL pairs, head size 64", 64, NORMAL, 8192, 5e5, ff=True),
    "ff_neox":      _v("frequency factors with NEOX pairs", 128, NEOX, 32768, 1e6, ff=True),
    "yarn_d256":    _v("YaRN at head size 256 (two pairs per lane)", 256, NEOX, 8192, 1e4, freq_scale=0.25, ext_factor=1.0),
}
# two more parameter sets the GPU chains need; not in the fixture, held to the same sharpness floor on the CPU
EXTRA = {
    "ff_norm_d128": _v("Llama-3.x at head size 128: NORMAL pairs, which the 16-lanes-per-row kernel refuses", 128, NORMAL, 8192, 5e5, ff=True),
    "plain_base1e4": _v("the control with another freq_base: a Gemma-style graph changes it from layer to layer", 128, NEOX, 32768, 1e4),
}
ALL = {**VARIANTS, **EXTRA}
for _name, _var in ALL.items():
    _var.name = _name
YARN_RAMPS = {"yarn4": (23, 40), "yarn32_d64": (8, 18), "yarn_d256": (51, 100)}     # corr0 .. corr1 of the three YaRN rows

# positions of the small host / fixture case: 0, neighbours >= 16, 63 / 64, beyond 4000; not ascending
POS8 = np.array([64, 0, 4097, 17, 63, 16, 5000, 1023], np.int32)
HEADS8 = 4


def rope_kwargs(v, n_dims=None):
    """the keyword arguments of Context.rope_ext"""
    return dict(n_dims=v.D if n_dims is None else n_dims, mode=v.mode, n_ctx_orig=v.n_ctx_orig, freq_base=v.freq_base, freq_scale=v.freq_scale,
                ext_factor=v.ext_factor, attn_factor=v.attn_factor, beta_fast=v.beta_fast, beta_slow=v.beta_slow)


def freq_factors(v, seed=0):
    """[D / 2] f32, DISTINCT per pair, uniform in [1.5, 8] (real Llama-3 factors are 1 on most pairs and would hide an indexing mistake); None for a variant without"""
    if not v.ff:
        return None
    rng = np.random.default_rng(1000 + seed + v.D)
    ff = rng.uniform(1.5, 8.0, v.D // 2).astype(np.float32)
    assert len(np.unique(ff)) == len(ff)
    return ff


def positions(T, seed=0):
    """T >= 8 positions: 0, the neighbours 16 / 17, 63 / 64, one beyond 4000 and seeded others below 8192, all distinct, shuffled"""
    assert T >= 8
    rng = np.random.default_rng(2000 + seed + T)
    must = [0, 16, 17, 63, 64, 4000 + int(rng.integers(1, 4000))]
    rest = [p for p in rng.permutation(np.arange(18, 8192)) if p not in must][:T - len(must)]
    pos = np.array(must + [int(p) for p in rest], np.int32)
    pos = pos[rng.permutation(T)]
    if np.all(np.diff(pos) > 0):
        pos = pos[::-1].copy()
    return pos


def signal(n_tok, n_head, D, off=0.0):
    """[n_tok, n_head, D] f32 in closed form (the reference's own test signal 0.1 + 2 cos(i + off), tests/test-quantize-fns.cpp, per row another offset
    and a second incommensurate term): the fixture stores the rotated rows only"""
    i = np.arange(D, dtype=np.float64)[None, None, :]
    r = (np.arange(n_tok, dtype=np.float64)[:, None, None] * n_head + np.arange(n_head, dtype=np.float64)[None, :, None])
    return (0.1 + 2.0 * np.cos(i + off + 0.37 * r) + np.sin(0.618 * i * (1.0 + 0.01 * r) + r)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the float64 restatement
def yarn_corr_dims(n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow):
    """ggml_rope_yarn_corr_dims (f32 arithmetic, as the reference)"""
    f = np.float32

    def corr_dim(n_rot):
        return f(n_dims) * np.log(f(n_ctx_orig) / (f(n_rot) * f(2) * f(np.pi)), dtype=np.float32) / (f(2) * np.log(f(freq_base), dtype=np.float32))
    start, end = np.floor(corr_dim(beta_fast)), np.ceil(corr_dim(beta_slow))
    return float(max(0.0, start)), float(min(n_dims - 1.0, end))


MUTATIONS = {
    # name: (applies to the variant, what the mistake is)
    "ff_dropped":      (lambda v: v.ff, "the frequency factors are not read"),
    "ff_shifted":      (lambda v: v.ff, "the frequency factors are read one pair off (indexed by element instead of by pair at the first pairs)"),
    "freq_scale_1":    (lambda v: v.freq_scale != 1.0, "freq_scale taken as 1"),
    "ext_factor_0":    (lambda v: v.ext_factor != 0.0, "ext_factor taken as 0: no YaRN ramp, no magnitude correction"),
    "no_magnitude":    (lambda v: v.ext_factor != 0.0, "the 1 + 0.1 ln(1 / freq_scale) magnitude correction dropped"),
    "attn_factor_1":   (lambda v: v.attn_factor != 1.0, "attn_factor taken as 1"),
    "other_freq_base": (lambda v: True, "the freq_base (and with it the table) of another variant"),
}


def mutations_of(v):
    return [m for m, (applies, _) in MUTATIONS.items() if applies(v)]


def other_freq_base(v):
    """the table's base farthest from the variant's own (1e4, yarn_d256's; for that one 1e6): a layer reading its neighbour's table in a graph that changes the base"""
    return 1e4 if v.freq_base != 1e4 else 1e6


def cos_sin(v, pos, ff=None, n_dims=None, mutation=None):
    """ggml_rope_cache_init + rope_yarn: (cos, sin) * mscale, float64 [len(pos), n_dims / 2]"""
    n_dims = v.D if n_dims is None else n_dims
    half = n_dims // 2
    freq_base, freq_scale, ext_factor, attn_factor = v.freq_base, v.freq_scale, v.ext_factor, v.attn_factor
    magnitude = True
    if mutation is not None:
        assert MUTATIONS[mutation][0](v), (v.name, mutation)
        if mutation == "ff_dropped":
            ff = None
        elif mutation == "ff_shifted":
            ff = np.roll(ff, 1)
        elif mutation == "freq_scale_1":
            freq_scale = 1.0
        elif mutation == "ext_factor_0":
            ext_factor = 0.0
        elif mutation == "no_magnitude":
            magnitude = False
        elif mutation == "attn_factor_1":
            attn_factor = 1.0
        elif mutation == "other_freq_base":
            freq_base = other_freq_base(v)
    # powf(freq_base, -2.0f / n_dims), correctly rounded as the C library's (numpy's own f32 power is one ulp off for 5e5 ^ (-1 / 32), which costs a row at
    # position 7000 an NMSE of 2e-8)
    theta_scale = np.float32(np.float64(np.float32(freq_base)) ** np.float64(np.float32(-2.0) / np.float32(n_dims)))
    corr0, corr1 = yarn_corr_dims(n_dims, v.n_ctx_orig, freq_base, v.beta_fast, v.beta_slow)
    theta = np.empty((len(pos), half), np.float32)
    t = np.asarray(pos).astype(np.float32)
    for ip in range(half):                                             # theta *= theta_scale, sequentially in f32
        theta[:, ip] = t
        t = (t * theta_scale).astype(np.float32)
    f = np.ones(half, np.float32) if ff is None else np.asarray(ff, np.float32)[:half]
    theta_extrap = (theta / f[None, :]).astype(np.float32).astype(np.float64)                                       # theta / ff: the f32 argument of rope_yarn
    theta_interp = np.float64(np.float32(freq_scale)) * theta_extrap
    th, mscale = theta_interp, np.float64(np.float32(attn_factor))
    if ext_factor != 0.0:
        y = (np.arange(half, dtype=np.float64) - corr0) / max(0.001, corr1 - corr0)                                 # rope_yarn_ramp: i0 / 2 is the pair
        ramp_mix = (1.0 - np.minimum(1.0, np.maximum(0.0, y))) * ext_factor
        th = theta_interp * (1.0 - ramp_mix)[None, :] + theta_extrap * ramp_mix[None, :]
        if magnitude:
            mscale = mscale * (1.0 + 0.1 * np.log(1.0 / np.float64(np.float32(freq_scale))))
    return np.cos(th) * mscale, np.sin(th) * mscale


def rope_f64(v, x, pos, ff=None, n_dims=None, mutation=None):
    """x [n_tok, n_head, D] -> float64, NORMAL pairs (2 i, 2 i + 1) or NEOX pairs (i, i + n_dims / 2); the channels past n_dims pass through"""
    n_dims = v.D if n_dims is None else n_dims
    half = n_dims // 2
    c, s = cos_sin(v, pos, ff, n_dims, mutation)
    c, s = c[:, None, :], s[:, None, :]
    x = np.asarray(x, np.float64)
    y = x.copy()
    if v.mode & NEOX:
        x0, x1 = x[..., :half], x[..., half:n_dims]
        y[..., :half] = x0 * c - x1 * s
        y[..., half:n_dims] = x0 * s + x1 * c
    else:
        x0, x1 = x[..., 0:n_dims:2], x[..., 1:n_dims:2]
        y[..., 0:n_dims:2] = x0 * c - x1 * s
        y[..., 1:n_dims:2] = x0 * s + x1 * c
    return y


# ---------------------------------------------------------------------------------------------------------------- the per-row measure
def row_nmse(got, want):
    """per (token, head) row: sum((a - b)^2) / sum(b^2) over the row's elements"""
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64).reshape(want.shape)
    d = ((got - want) ** 2).sum(-1); n = (want ** 2).sum(-1)
    e = np.where(n > 0, d / np.where(n > 0, n, 1.0), d)
    return np.where(np.isfinite(e), e, np.inf)


def worst_row(got, want):
    """(worst per-row NMSE, its index)"""
    e = row_nmse(got, want)
    i = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[i]), tuple(int(k) for k in i)


def small_case(v):
    """the host / fixture case of a variant: (x [8, 4, D], POS8, ff)"""
    return signal(len(POS8), HEADS8, v.D, off=float(sum(map(ord, v.name)) % 7)), POS8, freq_factors(v)
