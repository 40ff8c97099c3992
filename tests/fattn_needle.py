"""Position-sensitive inputs for attention parity tests (a plain helper module, used by test_fattn_needle_host.py and
test_fattn_needle_gpu.py).

With Gaussian keys every cache cell carries ~1 / n of a row's weight, so a cell dropped, read twice or leaked through the mask moves a row
by NMSE ~ 1 / n^2 -- far below any bar.  Here a few query rows per KV head ("needle rows") carry orthonormal directions scaled so that ONE
cache cell (the row's needle) scores L = 24 against a background of |score| < 1: the output row then IS that cell's V row, and a kernel
that skips the cell, or lets a masked "decoy" (2 x the direction, score 48) in, is wrong by a per-row NMSE of order 1.  Needles are placed
on the edges where kernels go wrong (tile, slice and causal edges) and moved from round to round on the same graph.

make_case() builds one round of one case; reference() evaluates it with a float64 attention (tests/test_gpu_parity.py _attn_f64 is passed
in); check_rows() is the per-row measure."""
import functools
import types

import numpy as np

L = 24.0
MAX_ROUNDS = 8
FLIP_LEAD, FLIP_BIAS = 4.0, -16.0      # the biased cell leads the needle by 4 before its bias and trails it by 12 after: exp(-12) keeps the needle row within 1e-8
EDGE_TOKENS = (0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128, 129)
F32, F16, Q4_0, Q8_0, BF16 = 0, 1, 2, 8, 30          # ggml type ids of the caches
KV_TYPES = {"f16": F16, "f32": F32, "q8_0": Q8_0, "q4_0": Q4_0, "bf16": BF16}
NINF = np.float16(-np.inf)


# ---------------------------------------------------------------------------------------------------------------- cache encodings
def _q8_0(x):
    """block_q8_0 {f16 d; int8 qs[32]} (as _q8_0 of test_fattn_plan_gpu.py)"""
    rows, n = x.shape
    b = x.reshape(rows, n // 32, 32)
    d = (np.abs(b).max(-1) / 127.0).astype(np.float16)
    q = np.rint(b / np.where(d == 0, 1, d).astype(np.float32)[..., None]).clip(-127, 127).astype(np.int8)
    out = np.zeros((rows, n // 32, 34), np.uint8)
    out[..., :2] = d[..., None].view(np.uint8).reshape(rows, n // 32, 2); out[..., 2:] = q.view(np.uint8)
    return out


def _dq8_0(b):
    d = np.ascontiguousarray(b[..., :2]).view(np.float16)[..., 0].astype(np.float32)
    return (d[..., None] * np.ascontiguousarray(b[..., 2:]).view(np.int8).astype(np.float32)).reshape(b.shape[0], -1)


def _q4_0(x):
    """block_q4_0 {f16 d; uint8 qs[16]}: d = (the element of largest magnitude) / -8, element j in the low nibble of qs[j], j + 16 in the high one"""
    rows, n = x.shape
    b = x.reshape(rows, n // 32, 32).astype(np.float32)
    mx = np.take_along_axis(b, np.abs(b).argmax(-1)[..., None], -1)[..., 0]
    d = (mx / -8.0).astype(np.float32)
    inv = np.where(d == 0, 0, 1.0 / np.where(d == 0, 1, d)).astype(np.float32)
    qv = np.minimum(15, (b * inv[..., None] + np.float32(8.5)).astype(np.int32)).astype(np.uint8)
    out = np.zeros((rows, n // 32, 18), np.uint8)
    out[..., :2] = d.astype(np.float16)[..., None].view(np.uint8).reshape(rows, n // 32, 2)
    out[..., 2:] = qv[..., :16] | (qv[..., 16:] << 4)
    return out


def _dq4_0(b):
    d = np.ascontiguousarray(b[..., :2]).view(np.float16)[..., 0].astype(np.float32)
    qs = b[..., 2:]
    qv = np.concatenate([qs & 0xF, qs >> 4], -1).astype(np.float32) - 8.0
    return (d[..., None] * qv).reshape(b.shape[0], -1)


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _dbf16(r):
    return (r.astype(np.uint32) << 16).view(np.float32)


def encode(x, kv_type):
    """rows [n, D] f32 -> (what tensor_set takes, the de-quantised values the kernels and the reference read)"""
    if kv_type == "f16":
        e = x.astype(np.float16); return e, e.astype(np.float32)
    if kv_type == "f32":
        e = x.astype(np.float32); return e, e
    if kv_type == "bf16":
        e = _bf16(x); return e, _dbf16(e)
    if kv_type == "q8_0":
        e = _q8_0(x); return e, _dq8_0(e)
    if kv_type == "q4_0":
        e = _q4_0(x); return e, _dq4_0(e)
    raise ValueError(kv_type)


def q_as_read(q, kv_type):
    """the query row as the reference converts it to K's vec_dot_type (f16 for F16 -- _attn_f64 does that itself --, Q8_0 blocks for Q8_0 / Q4_0, bf16 for BF16)"""
    if kv_type in ("q8_0", "q4_0"):                                  # quantize_row_q8_0: d = amax / 127 and 1 / d in f32, round half away from zero, d stored f16
        b = q.reshape(-1, q.shape[-1] // 32, 32).astype(np.float32)
        d = (np.abs(b).max(-1) / np.float32(127.0)).astype(np.float32)
        t = b * np.where(d == 0, 0, np.float32(1.0) / np.where(d == 0, 1, d)).astype(np.float32)[..., None]
        return (d.astype(np.float16).astype(np.float32)[..., None] * (np.sign(t) * np.floor(np.abs(t) + 0.5))).reshape(q.shape).astype(np.float32)
    if kv_type == "bf16":
        return _dbf16(_bf16(q))
    return q


# ---------------------------------------------------------------------------------------------------------------- edges
def edge_tokens(nq):
    return sorted({t for t in EDGE_TOKENS + (nq - 2, nq - 1) if 0 <= t < nq})


def edge_cells(nkv):
    """E(nkv) without the per-row members (a row's last live cell and the first cell of its last tile: slots 0 and 1 of plan()).  The kernels'
    own slice widths first -- multiples of 256 (the streaming kernel's and the one-token kernel's KV slices), of 128 (the decode tiles' 4-tile
    slices) --, then the issue's strides (64 below 1024, 16 below 128): the order in which a case spends its rows"""
    e = [0, 1, nkv - 2, nkv - 1]
    for m in range(256, nkv + 1, 256):
        e += [m - 1, m, m + 1]
    for m in range(128, min(nkv + 1, 1024), 128):
        e += [m - 1, m, m + 1]
    for m in range(64, min(nkv + 1, 1024), 64):
        e += [m - 1, m, m + 1]
    for m in range(16, min(nkv + 1, 128), 16):
        e += [m - 1, m, m + 1]
    return [c for c in dict.fromkeys(e) if 0 <= c < nkv]


def alibi_slope(h, nh, max_bias):
    if max_bias <= 0:
        return 1.0
    n2 = 2 ** int(np.floor(np.log2(nh)))
    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
    return m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1)


# ---------------------------------------------------------------------------------------------------------------- masks
def base_mask(kind, nq, nh, nkv, tile=None):
    """f16 mask [nm, nq_pad, nkv] (nm = nh for per-head masks, else 1; nq_pad = nq rounded up to 64, the padding rows repeat the last row) or None.
    causal kinds: row t sees cells 0 .. off + t, off chosen so that the last row ends 3 cells before the end of the view (a -inf tail);
    padded: the second half of the view is unused cells; seqs: _decode_attn_case's unified-cache mask (token t sees cells t, t + nq, ...); per_head: each head its own causal window;
    tile_live / tile_dead: see tile_case()."""
    if kind == "none":
        return None
    nq_pad = (nq + 63) // 64 * 64
    nm = nh if kind == "per_head" else 1
    m = np.zeros((nm, nq_pad, nkv), np.float16)
    if kind in ("tile_live", "tile_dead"):
        tq, cell = tile
        if kind == "tile_live":
            m[:] = NINF; m[0, tq, cell] = 0
        else:
            m[0, tq, cell] = NINF
        return m
    if kind == "seqs":
        m[:] = NINF
        for t in range(nq_pad):
            tt = min(t, nq - 1)
            m[0, t, tt::nq] = 0
            m[0, t, max(nq, nkv - min(200, nkv // 4)):] = NINF       # (the last quarter of a short view: unused cells)
        return m
    tail = 3 if nkv - nq >= 4 else 0
    off = nkv // 2 - nq if kind == "padded" else nkv - tail - nq
    for h in range(nm):
        for t in range(nq_pad):
            m[h, t, max(0, off - 11 * h + min(t, nq - 1)) + 1:] = NINF
    if kind == "alibi":                                          # finite position biases on the live cells (needle cells are set to 0 later)
        bias = -(np.abs(np.arange(nkv) - max(0, off + nq - 1)) / 16.0).astype(np.float16)
        m = np.where(np.isinf(m), m, bias[None, None, :]).astype(np.float16)
    return m


def _visible(mask, nq, nh, nkv):
    """vis[h][t]: bool [nkv]"""
    if mask is None:
        return lambda h, t: np.ones(nkv, bool)
    return lambda h, t: ~np.isneginf(mask[h if mask.shape[0] > 1 else 0, t])


# ---------------------------------------------------------------------------------------------------------------- which rows, which cells
def needle_rows(D, nq, nh, nhkv, tile=None):
    """per KV head: at most D / 2 (head, token) rows: the edge tokens first, heads rotating where the group has more rows than that"""
    gq = nh // nhkv
    toks = edge_tokens(nq) if tile is None else [tile[0]]
    cap = D // 2
    quota = max(1, min(gq, cap // len(toks)))
    rows = []
    for g in range(nhkv):
        r = []
        for i, t in enumerate(toks):
            r += [(g * gq + (i * quota + j) % gq, t) for j in range(quota)]
        r = r[:cap]
        rest = [t for t in range(nq) if t not in toks]
        room = min(cap, gq * nq // 2) - len(r)                        # room left: more rows, spread over the other tokens, so that the needles reach more cells --
        if tile is None and rest and room > 0:                        # at least half of the rows stay ordinary ones
            r += list(dict.fromkeys((g * gq + i % gq, rest[i * len(rest) // room]) for i in range(room)))
        rows.append(r)
    return rows


@functools.lru_cache(maxsize=None)
def plan(D, nq, nh, nhkv, nkv, ns, kind, tile=None):
    """the needle cell of every needle row in every slot -- slot rd * ns + s is sequence s of round rd: the mask is shared by the sequences, their
    caches are not, so each sequence carries needles of its own -- as a list of dicts {(h, t): cell}, the targets per KV head and whether every
    target is covered.  Slot 0: each row's last live cell (its causal edge); slot 1: the first cell of its last 32-cell tile; later slots cover what
    is left of E(nkv) -- of ALL live cells where nkv <= 320 -- rows that see least choosing first.  At most MAX_ROUNDS rounds."""
    mask = base_mask(kind, nq, nh, nkv, tile)
    vis = _visible(mask, nq, nh, nkv)
    rows = needle_rows(D, nq, nh, nhkv, tile)
    nslot = MAX_ROUNDS * ns
    slots = [dict() for _ in range(nslot)]
    targets, full, used = [], True, 2
    for g in range(nhkv):
        v = {r: vis(*r) for r in rows[g]}
        seen = np.zeros(nkv, bool)
        for r in rows[g]:
            seen |= v[r]
        order = edge_cells(nkv) + ([c for c in range(nkv)] if nkv <= 320 else [])
        tg = [c for c in dict.fromkeys(order) if seen[c]]
        targets.append(tg)
        left = dict.fromkeys(tg)
        by_view = sorted(rows[g], key=lambda r: int(v[r].sum()))
        for sl in range(nslot):
            if sl >= 2 and not left:
                break
            used = max(used, sl + 1)
            for r in by_view:
                live = np.flatnonzero(v[r])
                if sl == 0:
                    c = int(live[-1])
                elif sl == 1:
                    c = int(live[-1]) // 32 * 32
                    c = c if v[r][c] else int(live[live >= c][0])
                else:
                    c = next((x for x in left if v[r][x]), int(live[(sl * 7 + r[0]) % len(live)]))
                slots[sl][r] = c
                left.pop(c, None)
        full = full and not left
    slots = slots[:(used + ns - 1) // ns * ns]
    for i, sl in enumerate(slots):                                   # a KV head that finished early, and the slots that fill up the last round, repeat the first ones
        for g in range(nhkv):
            for r in rows[g]:
                sl.setdefault(r, slots[i % 2][r])
    return slots, targets, full


def n_rounds(D, nq, nh, nhkv, nkv, ns, kind, tile=None):
    return len(plan(D, nq, nh, nhkv, nkv, ns, kind, tile)[0]) // ns


# ---------------------------------------------------------------------------------------------------------------- exact scores
def _tune(q, kd, scale, target, fine):
    """q [R, D] such that scale * f16(q) . kd = target: rescale, and for `fine` rows walk single f16 elements by one ulp, largest effect first
    (a sink of L + ln 3 gives exactly 1/4 only if the needle scores exactly L)"""
    q = q.astype(np.float16).astype(np.float64)
    for _ in range(3):
        s = scale * (q * kd).sum(-1)
        q = (q * (target / s)[:, None]).astype(np.float16).astype(np.float64)
    idx = np.flatnonzero(fine)
    if len(idx):
        qf, kf = q[idx].astype(np.float16), kd[idx]
        res = target[idx] - scale * (qf.astype(np.float64) * kf).sum(-1)
        up = np.nextafter(qf, np.where(qf >= 0, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
        dn = np.nextafter(qf, np.float16(0))
        cand = np.concatenate([up, dn], -1).astype(np.float64)                        # [R, 2D]
        eff = scale * (cand - np.concatenate([qf, qf], -1).astype(np.float64)) * np.concatenate([kf, kf], -1)
        order = np.argsort(-np.abs(eff), -1)
        Dn = qf.shape[1]
        out = qf.astype(np.float64)
        taken = np.zeros(out.shape, bool)
        ar = np.arange(len(idx))
        for j in range(2 * Dn):
            c = order[:, j]; e = eff[ar, c]; el = c % Dn
            take = (np.abs(res - e) < np.abs(res)) & ~taken[ar, el]
            out[ar[take], el[take]] = cand[ar[take], c[take]]
            taken[ar[take], el[take]] = True
            res = np.where(take, res - e, res)
        q[idx] = out
    return q.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- one round of one case
def make_case(D, Dv, nq, nh, nhkv, nkv, ns, mask_kind, positions, seed, kv_type="f16", softcap=0.0, tile=None):
    """mask_kind: none | causal | padded | sinks | bias | alibi | seqs | per_head | tile_live | tile_dead; positions: the round.
    Returns a namespace with q [ns, nh, nq, D] f32, k / v as tensor_set takes them, kd / vd their de-quantised values [ns, nhkv, nkv, D(v)],
    mask ([nm, nq_pad, nkv] f16 or None), sinks, needles [(s, h, t, cell)], decoys {(s, h, t): [cells]}, flips {(s, h, t): cell},
    factor {(s, h, t): 1 or 1/4} and scale / softcap / max_bias"""
    rng = np.random.default_rng(seed * 1000 + positions)
    gq = nh // nhkv
    scale = 1.0 / np.sqrt(D)
    slots, _, _ = plan(D, nq, nh, nhkv, nkv, ns, mask_kind, tile)
    cells_of = slots[positions * ns:positions * ns + ns]              # per sequence
    mask = base_mask(mask_kind, nq, nh, nkv, tile)
    max_bias = 8.0 if mask_kind == "alibi" else 0.0
    raw = softcap * np.arctanh(L / softcap) if softcap else L             # the score before the cap that gives L after it
    ln = np.sqrt(raw / scale)
    q = rng.standard_normal((ns, nh, nq, D)).astype(np.float32)
    k = (0.05 * rng.standard_normal((ns, nhkv, nkv, D))).astype(np.float32)
    v = rng.standard_normal((ns, nhkv, nkv, Dv)).astype(np.float32)
    sinks = None
    if mask_kind == "sinks":
        sinks = rng.standard_normal(nh).astype(np.float32)
        sinks[1::2] = np.float32(L + np.log(3.0))
    vis = _visible(mask, nq, nh, nkv)
    rows = needle_rows(D, nq, nh, nhkv, tile)
    needles, decoys, flips, factor = [], {}, {}, {}
    # decoys and the biased cells depend on the mask alone: the same in every sequence (a biased cell avoids the needles of every sequence)
    dec_of, flip_of = {}, {}
    for g in range(nhkv):
        for (h, t) in rows[g]:
            vr = vis(h, t)
            assert all(vr[cl[(h, t)]] for cl in cells_of), (h, t)
            d = []
            if mask is not None and mask_kind != "tile_live":
                last = int(np.flatnonzero(vr)[-1])
                if last + 1 < nkv:
                    d.append(last + 1)                                    # the first masked cell behind the row's edge
                if not vr[nkv - 1]:
                    d.append(nkv - 1)                                     # the last cell of the -inf tail
                if mask_kind == "padded":
                    dead = [T for T in range(nkv // 32) if not any(vis(0, tt)[32 * T:32 * T + 32].any() for tt in (0, nq - 1))]
                    if dead:
                        d.append(32 * dead[-1] + 13)                      # a cell of a 32-cell tile no row sees
                if mask_kind == "seqs" and nq > 1:
                    nb = [x for x in range((t + 1) % nq, last + 1, nq)]
                    if nb:
                        d.append(nb[-1])                                  # the neighbour sequence's newest cell
                if mask_kind == "tile_dead":
                    d = [tile[1]]
                d = [x for x in dict.fromkeys(d) if not vr[x]]
            dec_of[(h, t)] = d
    if mask_kind in ("bias", "alibi"):
        taken = {}
        for g in range(nhkv):
            for (h, t) in rows[g]:
                taken.setdefault(t, set()).update(cl[(h, t)] for cl in cells_of)
        for g in range(nhkv):
            for (h, t) in rows[g]:
                free = [x for x in np.flatnonzero(vis(h, t))[::-1] if x not in taken[t]]
                if free:
                    f = int(free[0]); taken[t].add(f); flip_of[(h, t)] = f
                    mask[0, t, f] = np.float16(FLIP_BIAS / alibi_slope(h, nh, max_bias))
                    if t == nq - 1:
                        mask[0, nq:, f] = mask[0, t, f]
        if mask_kind == "alibi":
            for g in range(nhkv):
                for (h, t) in rows[g]:
                    for cl in cells_of:
                        mask[0, t, cl[(h, t)]] = 0
    for s in range(ns):
        for g in range(nhkv):
            Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
            for i, (h, t) in enumerate(rows[g]):
                u = Q[:, i]
                c = cells_of[s][(h, t)]
                q[s, h, t] = ln * u
                k[s, g, c] += ln * u
                for x in dec_of[(h, t)]:
                    k[s, g, x] += 2 * ln * u
                if (h, t) in flip_of:
                    k[s, g, flip_of[(h, t)]] += (raw + FLIP_LEAD) / (scale * ln) * u
                    flips[(s, h, t)] = flip_of[(h, t)]
                needles.append((s, h, t, c))
                decoys[(s, h, t)] = dec_of[(h, t)]
                factor[(s, h, t)] = 0.25 if (sinks is not None and h % 2 == 1) else 1.0
    ke, kd = encode(k.reshape(-1, D), kv_type)
    ve, vd = encode(v.reshape(-1, Dv), kv_type)
    kd = kd.reshape(ns, nhkv, nkv, D); vd = vd.reshape(ns, nhkv, nkv, Dv)
    # the needle's score made exact on the values the kernels read
    qn = np.stack([q[s, h, t] for (s, h, t, _) in needles]).astype(np.float64)
    kn = np.stack([kd[s, h // gq, c] for (s, h, t, c) in needles]).astype(np.float64)
    fine = np.array([factor[(s, h, t)] != 1.0 for (s, h, t, _) in needles])
    qn = _tune(qn, kn, scale, np.full(len(needles), raw), fine)
    for i, (s, h, t, _) in enumerate(needles):
        q[s, h, t] = qn[i]
    return types.SimpleNamespace(D=D, Dv=Dv, nq=nq, nh=nh, nhkv=nhkv, nkv=nkv, ns=ns, kind=mask_kind, kv_type=kv_type, q=q, k=ke, v=ve, kd=kd, vd=vd, mask=mask,
                                 sinks=sinks, tile=tile, needles=needles, decoys=decoys, flips=flips, factor=factor, scale=scale, softcap=softcap, max_bias=max_bias)


def expected_row(c, s, h, t, cell):
    return c.factor[(s, h, t)] * c.vd[s, h // (c.nh // c.nhkv), cell].astype(np.float64)


def reference(attn_f64, c, mask="own", sinks="own", seq=None):
    """[ns, nq, nh, Dv] float64 by attn_f64 (_attn_f64 of test_gpu_parity.py) on the de-quantised caches; mask / sinks replace the case's own
    (the sensitivity checks), seq restricts to one sequence"""
    mask = c.mask if isinstance(mask, str) else mask
    sinks = c.sinks if isinstance(sinks, str) else sinks
    sl = slice(None) if seq is None else slice(seq, seq + 1)
    q = q_as_read(c.q[sl], c.kv_type)
    kd, vd = c.kd[sl], c.vd[sl]
    if c.Dv < c.D:                                                    # attn_f64 sizes its rows by q: pad V's rows with zeros, cut them off again
        vd = np.concatenate([vd, np.zeros(vd.shape[:-1] + (c.D - c.Dv,), vd.dtype)], -1)
    if mask is None or mask.shape[0] == 1:
        out = attn_f64(q, kd, vd, None if mask is None else mask[0], c.scale, c.softcap, sinks, c.max_bias)
    else:                                                             # a mask per head: one head at a time
        gq = c.nh // c.nhkv
        out = np.concatenate([attn_f64(q[:, h:h + 1], kd[:, h // gq:h // gq + 1], vd[:, h // gq:h // gq + 1], mask[h], c.scale, c.softcap,
                                       None if sinks is None else sinks[h:h + 1], 0.0) for h in range(c.nh)], 2)
    return out[..., :c.Dv]


def row_nmse(got, want):
    """per output row [ns, nq, nh]: sum((a - b)^2) / sum(b^2) over the head's elements (the absolute sum where the reference row is zero)"""
    got = np.asarray(got, np.float64).reshape(want.shape); want = np.asarray(want, np.float64)
    d = ((got - want) ** 2).sum(-1); n = (want ** 2).sum(-1)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


def check_rows(got, want, needles=()):
    """worst per-row NMSE over EVERY (s, t, h) row, its index, and the worst needle row"""
    e = row_nmse(got, want)
    e = np.where(np.isfinite(e), e, np.inf)
    i = np.unravel_index(int(np.argmax(e)), e.shape)
    wn = max((float(e[s, t, h]) for (s, h, t, _) in needles), default=0.0)
    return float(e[i]), tuple(int(x) for x in i), wn


# ---------------------------------------------------------------------------------------------------------------- the cases
# name: (D, Dv, nq, nh, nhkv, nkv, ns, kinds, kv type, softcap, max rounds)
# (what each shape selects, and the launcher arithmetic behind it, is stated with the launch options in test_fattn_needle_gpu.py)
CASES = {
    "dec_r1_narrow":    (128, 128, 1, 2, 2, 40, 6, ("causal", "sinks"), "f16", 0.0, 8),
    "dec_r2_wide":      (128, 128, 1, 4, 2, 257, 20, ("causal", "sinks"), "f16", 0.0, 8),
    "dec_r4_wide":      (128, 128, 2, 4, 2, 300, 12, ("causal", "sinks"), "f16", 0.0, 8),
    "dec_r8":           (64, 64, 8, 8, 1, 96, 1, ("causal", "sinks"), "f16", 0.0, 8),
    "dec_split4":       (128, 128, 1, 4, 2, 1024, 6, ("causal", "sinks"), "f16", 0.0, 8),
    "dec_split8":       (64, 64, 1, 4, 2, 2048, 7, ("causal", "sinks"), "f16", 0.0, 8),
    "dec_per_head":     (128, 128, 4, 4, 2, 300, 6, ("per_head",), "f16", 0.0, 8),
    "dec_gq33":         (128, 128, 2, 33, 1, 300, 1, ("causal",), "f16", 0.0, 8),
    "gqa_direct_a":     (128, 128, 8, 4, 2, 96, 2, ("causal", "bias", "seqs"), "f16", 0.0, 8),
    "gqa_direct_b":     (64, 64, 32, 8, 2, 250, 2, ("causal", "bias", "seqs"), "f16", 0.0, 8),
    "gqa_direct_c":     (128, 128, 3, 8, 2, 77, 2, ("causal", "bias", "seqs"), "f16", 0.0, 8),
    "gqa_split_257":    (128, 128, 1, 4, 2, 257, 20, ("causal", "sinks", "alibi"), "f16", 0.0, 8),
    "gqa_split_1023":   (128, 128, 1, 32, 8, 1023, 3, ("causal", "sinks", "alibi"), "f16", 0.0, 8),
    "gqa_split_1024":   (128, 128, 1, 32, 8, 1024, 3, ("causal", "sinks", "alibi"), "f16", 0.0, 8),
    "gqa_split_1500":   (64, 64, 4, 8, 1, 1500, 2, ("causal", "sinks", "alibi"), "f16", 0.0, 8),
    "gqa_split_5000":   (128, 128, 2, 16, 4, 5000, 3, ("causal", "sinks", "alibi"), "f16", 50.0, 8),
    "mma_1w":           (128, 128, 9, 4, 2, 96, 2, ("causal", "padded", "none"), "f16", 0.0, 8),
    "mma_2w_sq1":       (128, 128, 33, 4, 2, 100, 1, ("causal", "padded", "none"), "f16", 0.0, 8),
    "mma_2w_sq2":       (128, 128, 97, 8, 2, 230, 25, ("causal", "padded", "none"), "f16", 0.0, 8),
    "mma_ks2":          (128, 128, 65, 8, 2, 200, 1, ("causal", "padded", "none"), "f16", 0.0, 8),
    "mma_ks4_d64":      (64, 64, 130, 4, 2, 257, 2, ("causal", "padded", "none"), "f16", 0.0, 8),
    "mma_ks4_d128":     (128, 128, 33, 4, 2, 300, 2, ("causal", "padded", "none"), "f16", 0.0, 8),
    "ring128_pairs":    (128, 128, 129, 32, 8, 300, 8, ("causal", "padded", "sinks"), "f16", 0.0, 8),
    "ring128_single":   (128, 128, 129, 16, 16, 333, 16, ("causal", "padded", "sinks"), "f16", 0.0, 8),
    "ring64_plain":     (64, 64, 129, 16, 16, 300, 6, ("causal", "sinks"), "f16", 0.0, 8),
    "ring64_ks2":       (64, 64, 129, 16, 4, 777, 6, ("causal", "sinks"), "f16", 0.0, 8),
    "any_d80":          (80, 80, 3, 4, 2, 100, 3, ("causal",), "f16", 0.0, 8),
    "any_d192_128":     (192, 128, 3, 4, 4, 113, 6, ("causal",), "f16", 0.0, 8),
    "any_q8_0":         (128, 128, 4, 8, 2, 96, 1, ("causal",), "q8_0", 0.0, 8),
    "any_q4_0":         (64, 64, 35, 4, 4, 130, 2, ("causal",), "q4_0", 0.0, 8),
    "any_bf16":         (128, 128, 2, 4, 2, 113, 5, ("causal",), "bf16", 0.0, 8),
    "any_f32":          (128, 128, 2, 4, 2, 113, 5, ("causal",), "f32", 0.0, 8),
    "any_d576_512":     (576, 512, 2, 2, 1, 70, 3, ("causal",), "f16", 0.0, 8),
}


# the fused no-flash-attention chains (MUL_MAT K.q -> SOFT_MAX_EXT -> MUL_MAT V^T.p -> PERMUTE + CONT): the same inputs in the chains' layouts
CHAINS = {
    "sm_prefill_a":    (128, 128, 33, 8, 2, 300, 1, ("causal",), "f16", 0.0, 8),      # exec_attn_sm_prefill: f16 K rows, transposed f16 V cache, f32 causal mask
    "sm_prefill_b":    (64, 64, 70, 4, 4, 130, 1, ("causal",), "f16", 0.0, 8),
    "f32_chain_a":     (72, 72, 64, 2, 2, 508, 1, ("none",), "f32", 0.0, 8),           # k_attn_f32: f32 q / k / v^T, no mask, needles over all cells
    "f32_chain_b":     (80, 80, 77, 2, 2, 516, 1, ("none",), "f32", 0.0, 8),
}
ALL = {**CASES, **CHAINS}


def case_ids(table=None):
    return [f"{n}-{kd}" for n, c in (ALL if table is None else table).items() for kd in c[7]]


def case_rounds(name, kind):
    D, Dv, nq, nh, nhkv, nkv, ns, _, _, _, mx = ALL[name]
    return min(mx, n_rounds(D, nq, nh, nhkv, nkv, ns, kind))


def build(name, kind, rd):
    D, Dv, nq, nh, nhkv, nkv, ns, _, kv_type, softcap, _ = ALL[name]
    return make_case(D, Dv, nq, nh, nhkv, nkv, ns, kind, rd, sum(map(ord, name + kind)), kv_type, softcap)


# ---- the mask tile map (prefill kernel, D = 128, 2 heads over 1 KV head): ONE entry of ONE 32 x 32 tile differs from the rest of the mask
# place: (nq, nkv, query block, kv tile, rows of the block the entry takes, cells of the tile it takes) -- in a ragged tile the cells / rows it has
TILE_PLACES = {
    "interior":     (70, 300, 1, 4, (0, 31), (0, 15, 16, 31)),
    "last_kv_300":  (70, 300, 0, 9, (0, 31), (0, 5, 11)),           # ragged last KV tile of 12 cells: the 16-half vector path sees its first half cut
    "last_kv_307":  (70, 307, 1, 9, (0, 31), (0, 15, 16, 18)),      # ... of 19 cells on rows that are not 16-byte aligned (odd nkv): the scalar path and its tail
    "last_q_block": (70, 300, 2, 3, (0, 5), (0, 15, 16, 31)),       # ragged last query block (rows 64 .. 69)
    "odd_view":     (40, 131, 1, 2, (0, 7), (0, 15, 16, 31)),       # rows of 262 bytes; the block has rows 32 .. 39
}
TILE_ENTRIES = [(p, qi, ki) for p, t in TILE_PLACES.items() for qi in t[4] for ki in t[5]]


def tile_entry(place, qi, ki):
    """(query row, cell) of the entry"""
    nq, nkv, qb, kt, _, _ = TILE_PLACES[place]
    assert qb * 32 + qi < nq and kt * 32 + ki < nkv
    return qb * 32 + qi, kt * 32 + ki


def tile_case(place, qi, ki, kind, alt=False):
    """kind tile_live: a mask of -inf with one live entry, the needle of its row (every other row attends to nothing: zero rows);
    tile_dead: a mask of zeros with one -inf entry, on a cell that holds a decoy of its row.  alt: the entry moved to another query block and
    another KV tile -- the mask a test rewrites the first one with"""
    nq, nkv = TILE_PLACES[place][:2]
    tq, cell = tile_entry(place, qi, ki)
    if alt:
        tq, cell = (tq + 32) % nq, (cell + 64) % nkv
    return make_case(128, 128, nq, 2, 1, nkv, 1, kind, 0, 77 + qi + 3 * ki + alt, tile=(tq, cell))


# ---------------------------------------------------------------------------------------------------------------- one-token steps through a ONE-layer model
# The one-token kernels behind the q / k / v pre-stage (k_fattn_one, k_fattn_gs) and the one-token chain without flash-attention (attn_one_sm) are reached only through
# a layer graph.  The needle directions are the step's own Q after RoPE (g.roots[0]), read from the reference CPU backend on the same weights: a q that the GPU rotates
# differently loses its needle.  Shared by test_fattn_needle_gpu.py and test_rope_variants_gpu.py; `tag` tells the models of one config apart (a config may hold arrays).
BAR = 5e-4                                  # the project's and the reference's bar for FLASH_ATTN_EXT, applied per row
_MODELS = {}


def free_models():
    """the one-layer models live for one test file only (an autouse module fixture of each file calls this)"""
    for mdl, graphs in _MODELS.values():
        for g, *_ in graphs.values():
            g.free()
        mdl.wctx.free()
    _MODELS.clear()


def model(backend, cfg, types, flash, tag="", n_ctx=4096):
    from llama_cpp_omni_amd import qwen3
    key = (id(backend), flash, tag)
    if key not in _MODELS:
        _MODELS[key] = (qwen3.Model(backend, cfg, types(cfg), n_ctx=n_ctx, seed=9, flash_attn=flash), {})
    return _MODELS[key]


def step(backend, cfg, types, flash, tap, n_kv, pos, x, caches=None, tag=""):
    """one decode step at position `pos` over a view of n_kv cells; caches = (K, V) [n_ctx, n_head_kv, head_dim] f16 written first.
    Returns (Q after RoPE [n_head, head_dim], the tap)"""
    mdl, graphs = model(backend, cfg, types, flash, tag)
    if (tap, n_kv) not in graphs:
        g, I, _ = mdl.build(1, n_kv, tap_attn=tap)
        graphs[(tap, n_kv)] = (g, I, g.graph(), g.attn_tap)
    g, I, gr, out = graphs[(tap, n_kv)]
    if caches is not None:
        K, V = caches
        backend.tensor_set(mdl.layers[0]["k_cache"], K)
        backend.tensor_set(mdl.layers[0]["v_cache"], V if not mdl.v_trans else np.ascontiguousarray(V.reshape(V.shape[0], -1).T))
    mdl.set_inputs(I, x, pos, n_kv)
    backend.graph_compute(gr)
    return backend.tensor_get(g.roots[0]).astype(np.float64).reshape(cfg["n_head"], cfg["head_dim"]), backend.tensor_get(out).astype(np.float64).ravel()


def k_cache_row(backend, cfg, types, flash, cell, tag=""):
    """layer 0's K cache row of `cell` as the last step left it: [n_head_kv, head_dim] f16"""
    mdl, _ = model(backend, cfg, types, flash, tag)
    nb = cfg["n_head_kv"] * cfg["head_dim"] * 2
    return backend.tensor_get(mdl.layers[0]["k_cache"], np.float16, cell * nb, nb).copy().reshape(cfg["n_head_kv"], cfg["head_dim"])


def needle_caches(rng, Q, cells, pos, n_kv, n_ctx=4096, n_head_kv=8):
    """K / V caches [n_ctx, n_head_kv, D] f16: head h's needle -- its own query direction, score L -- in cell cells[h] of its KV head, a decoy of every head in the first
    cells behind the causal edge and in the last cell of the view"""
    H, D = Q.shape
    gq = H // n_head_kv
    K = (0.05 * rng.standard_normal((n_ctx, n_head_kv, D))).astype(np.float32)
    V = rng.standard_normal((n_ctx, n_head_kv, D)).astype(np.float16)
    scale = 1.0 / np.sqrt(float(D))
    for h in range(H):
        u = Q[h] / (scale * (Q[h] ** 2).sum())                       # scale * q . u = 1
        K[cells[h], h // gq] += L * u
        for d in {pos + 1, n_kv - 1} - {pos}:
            K[d, h // gq] += 2 * L * u
    return K.astype(np.float16), V


def slice_edges(width, pos):
    """the cells at the edges of `width`-row slices below the new token's cell, the first cells and the newest ones"""
    e = [pos - 1, pos - 2, 0, 1]
    for m in range(width, pos, width):
        e += [m - 1, m, m + 1]
    return [c for c in dict.fromkeys(e) if 0 <= c < pos]


def head_rows(tag, rows_gpu, rows_ref, V, cells):
    """every head's attention row [n_head, D] against its needle's V row and against the reference backend's row; returns the worst of each"""
    H = len(cells)
    gq = H // V.shape[1]
    worst = (0.0, 0.0)
    for h in range(H):
        want = V[cells[h], h // gq].astype(np.float64)
        e_v = float(row_nmse(rows_gpu[h][None], want[None])[0]); e_r = float(row_nmse(rows_gpu[h][None], rows_ref[h][None])[0])
        e_rv = float(row_nmse(rows_ref[h][None], want[None])[0])
        worst = (max(worst[0], e_v), max(worst[1], e_r))
        assert e_rv < 1e-8, (tag, "the reference's row is not its needle's V row", h, cells[h], e_rv)
        assert e_v < BAR and e_r < BAR, (tag, h, cells[h], e_v, e_r)
    print(f"{tag}: worst head row vs its needle's V row {worst[0]:.3e}, vs the reference backend {worst[1]:.3e}")
    return worst


def launches(be, cfg, types, flash, n_kv, pos, x, caches, option=None, tag=""):
    """kernels_last_graph of the step, eager (setting an option drops the captured graphs), with `option` switched off"""
    be.set_option(option or "fattn_gqa", 0 if option else 1)
    try:
        _, rows = step(be, cfg, types, flash, "rows", n_kv, pos, x, caches, tag)
        return int(be.get_stat("kernels_last_graph")), rows
    finally:
        if option:
            be.set_option(option, 1)
