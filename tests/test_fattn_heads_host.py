"""The inputs of tests/test_fattn_heads_gpu.py on the host (no GPU): the float64 restatement on every case of its table is finite, every mask row has a
visible cell, and every needle row IS its needle's V row (x 1/4 under a sink) -- so a cell the kernel drops, reads twice or lets through the mask shows."""
import numpy as np

import fattn_needle as fn
import test_fattn_wide_gpu as wide
from test_fattn_heads_gpu import CASES, _heads_table  # noqa: F401  (the autouse fixture: the table joins test_fattn_wide_gpu's)
from test_gpu_parity import _attn_f64


def test_inputs_are_sound_on_the_host():
    for name, cs in CASES.items():
        for kind in cs[7]:
            c = wide._build(name, kind, 0)
            assert (c.D, c.Dv, c.nq, c.nh, c.nhkv, c.nkv, c.ns) == cs[:7], (name, kind)
            if c.mask is not None:
                assert (~np.isneginf(c.mask[:, :c.nq])).any(-1).all(), (name, kind)
            want = fn.reference(_attn_f64, c)
            assert want.shape == (c.ns, c.nq, c.nh, c.Dv) and np.isfinite(want).all(), (name, kind)
            if kind != "alibi":
                for (s, h, t, cell) in c.needles:
                    assert fn.row_nmse(want[s, t, h][None], fn.expected_row(c, s, h, t, cell)[None])[0] < 1e-6, (name, kind, s, h, t, cell)
