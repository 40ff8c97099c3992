"""The inputs of test_fattn_needle_gpu.py are sharp (CPU only): for every case of its table, with the float64 attention alone,
  (a) every needle row of the reference equals its needle's V row (a quarter of it on sink heads) within per-row NMSE 1e-8,
  (b) masking one needle cell out, unmasking one decoy, applying one sink twice or dropping one bias moves the affected row by per-row NMSE >= 0.1 -- 200 x the
      bar of the GPU test, so a kernel that makes such a mistake fails it,
  (c) the needles cover the edge cells the generator promises.
These are conditions on the inputs, not measurements: a case that misses them is changed, the thresholds are not."""
import numpy as np
import pytest

import fattn_needle as fn
from test_gpu_parity import _attn_f64

IDS = fn.case_ids()


def _split(cid):
    name, kind = cid.rsplit("-", 1)
    return name, kind


def _valid(c, want):
    worst = 0.0
    for (s, h, t, cell) in c.needles:
        e = fn.row_nmse(want[s, t, h][None], fn.expected_row(c, s, h, t, cell)[None])[0]
        worst = max(worst, float(e))
        assert e < 1e-8, (s, h, t, cell, float(e))
    return worst


def _moved(c, base, s, h, t, **kw):
    alt = fn.reference(_attn_f64, c, seq=s, **kw)
    return float(fn.row_nmse(alt[0, t, h][None], base[s, t, h][None])[0])


def _mask_with(c, h, t, cell, value):
    m = np.zeros((1, (c.nq + 63) // 64 * 64, c.nkv), np.float16) if c.mask is None else c.mask.copy()
    m[h if m.shape[0] > 1 else 0, t, cell] = value
    return m


def _sensitive(c, want, rng):
    s, h, t, cell = c.needles[rng.integers(len(c.needles))]
    e = _moved(c, want, s, h, t, mask=_mask_with(c, h, t, cell, -np.inf))
    assert e >= 0.1, ("needle cell masked out", s, h, t, cell, e)
    with_decoy = [n for n in c.needles if c.decoys[n[:3]]]
    assert with_decoy or c.kind in ("none", "tile_live"), "a masked case without a decoy"
    if with_decoy:
        s, h, t, cell = with_decoy[rng.integers(len(with_decoy))]
        for d in c.decoys[(s, h, t)]:
            e = _moved(c, want, s, h, t, mask=_mask_with(c, h, t, d, 0.0))
            assert e >= 0.1, ("decoy unmasked", s, h, t, d, e)
    if c.sinks is not None:
        on_sink = [n for n in c.needles if c.factor[n[:3]] != 1.0]
        s, h, t, cell = on_sink[rng.integers(len(on_sink))]
        twice = c.sinks.copy(); twice[h] += np.float32(np.log(2.0))       # exp(sink) counted twice
        e = _moved(c, want, s, h, t, sinks=twice)
        assert e >= 0.1, ("sink applied twice", s, h, t, e)
    cell_of = {n[:3]: n[3] for n in c.needles}
    for key, f in c.flips.items():                                       # the biased cell outscores the needle before its bias; (a) shows that it loses
        assert f != cell_of[key] and c.mask[0, key[2], f] <= -16
    if c.flips:
        (s, h, t), f = list(c.flips.items())[rng.integers(len(c.flips))]
        e = _moved(c, want, s, h, t, mask=_mask_with(c, h, t, f, 0.0))
        assert e >= 0.1, ("bias of the leading cell dropped", s, h, t, f, e)


@pytest.mark.parametrize("cid", IDS)
def test_needle_inputs_are_valid_and_sensitive(cid):
    name, kind = _split(cid)
    rng = np.random.default_rng(sum(map(ord, cid)))
    for rd in range(fn.case_rounds(name, kind)):
        c = fn.build(name, kind, rd)
        want = fn.reference(_attn_f64, c)
        assert np.isfinite(want).all()
        _valid(c, want)
        if rd == 0:
            _sensitive(c, want, rng)
            if kind in ("bias", "alibi"):
                assert c.flips, "no row of the case has room for a biased cell"


@pytest.mark.parametrize("cid", IDS)
def test_needle_positions_cover_the_edges(cid):
    """(c) over the rounds the GPU test runs, every live member of E(nkv) -- every live cell where nkv <= 320 -- is the needle of a row of EVERY KV head, and
    every needle row has had its own last live cell and the first cell of its last 32-cell tile.  Each sequence of a case carries needles of its own (the
    sequences share the mask, not the cache); the table gives the decodes of one or two rows per KV head enough sequences to hold all members in 8 rounds."""
    name, kind = _split(cid)
    D, Dv, nq, nh, nhkv, nkv, ns, _, _, _, _ = fn.ALL[name]
    slots, targets, full = fn.plan(D, nq, nh, nhkv, nkv, ns, kind)
    run = slots[:fn.case_rounds(name, kind) * ns]
    assert len(run) == len(slots) and len(slots) // ns <= fn.MAX_ROUNDS
    rows = fn.needle_rows(D, nq, nh, nhkv)
    gq = nh // nhkv
    mask = fn.base_mask(kind, nq, nh, nkv)
    want = fn.edge_cells(nkv) + (list(range(nkv)) if nkv <= 320 else [])
    for g in range(nhkv):
        assert 1 <= len(rows[g]) <= D // 2
        assert all(h // gq == g for h, _ in rows[g])
        assert {t for _, t in rows[g]} >= set(fn.edge_tokens(nq)) and len(set(rows[g])) == len(rows[g])
        got, seen = set(), np.zeros(nkv, bool)
        for (h, t) in rows[g]:
            live = np.ones(nkv, bool) if mask is None else ~np.isneginf(mask[h if mask.shape[0] > 1 else 0, t])
            seen |= live
            for sl in run:
                assert live[sl[(h, t)]]                                  # a needle is a cell its row sees
                got.add(sl[(h, t)])
            last = np.flatnonzero(live)[-1]
            first = last // 32 * 32
            assert run[0][(h, t)] == last
            assert run[1][(h, t)] == (first if live[first] else np.flatnonzero(live)[np.flatnonzero(live) >= first][0])
        missing = [c for c in dict.fromkeys(want) if seen[c] and c not in got]
        assert not missing, (g, missing)
    assert full
    print(cid, "sequences", ns, "rounds", len(run) // ns, "members per KV head", [len(t) for t in targets])


@pytest.mark.parametrize("kind", ["tile_live", "tile_dead"])
@pytest.mark.parametrize("place", list(fn.TILE_PLACES))
def test_tile_map_inputs_are_valid_and_sensitive(place, kind):
    rng = np.random.default_rng(5)
    entries = [e for e in fn.TILE_ENTRIES if e[0] == place]
    assert len({fn.tile_entry(*e) for e in entries}) == len(entries)     # distinct entries, all inside the view
    for (_, qi, ki) in entries:
        for alt in (False, True):
            c = fn.tile_case(place, qi, ki, kind, alt=alt)
            want = fn.reference(_attn_f64, c)
            assert np.isfinite(want).all()
            _valid(c, want)
            if not alt:
                _sensitive(c, want, rng)
            tq, cell = c.tile
            if kind == "tile_live":
                assert {n[2:] for n in c.needles} == {(tq, cell)}
                assert (np.delete(want, tq, 1) == 0).all()               # every other row attends to nothing
            else:
                assert all(c.decoys[n[:3]] == [cell] for n in c.needles)
