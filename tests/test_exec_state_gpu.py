"""The executor's deferred and cached state against in-graph writes (graph_internal.hpp exec_state).

graph_exec*.cpp carries state from one node to a later one: the V-rows layout of an encoder's V^T CAST (vplain), the copy queue (cq) and the Token2Wav concat tail,
the RoPE table (rt), the mask tile map (mask_map), the activation image (act), the deferred RMS_NORM (pn), the split-K reductions (pr) and the lazy copies (lazy).
Each is valid only until a node writes the bytes it depends on.  Every case here is a PAIR of small graphs in an explicit node order (Context.graph(), not
graph_expand): a control that takes the fused path -- proved by a launch count below the fusion-off run or by a named counter -- and the same graph with one legal
node that writes those bytes in between (a CPY into a view: how ggml writes in place).  Each graph runs on the backend with its defaults (eager, captured, replayed:
three input sets), with fusion off, and on the reference CPU backend; every output of every run is compared with the reference on the same inputs.  A stale table,
map or layout gives an NMSE of order 1, far above any bar used here.
"""
import numpy as np
import pytest

from conftest import nmse

pytestmark = pytest.mark.gpu


def _pad(c, pkg):
    """eight cheap launches on a leaf of their own behind the case: every graph has the >= 8 launching nodes that make the backend capture and replay it"""
    p = c.new_tensor(pkg.GGML_TYPE_F32, 64)
    t = p
    for _ in range(8):
        t = c.scale(t, 0.5)
    return p, t


def _run(backend, pkg, build, feed_sets, stats=(), counted=True):
    """one allocation, one graph, one graph_compute per input set; returns (outputs per set, kernels_last_graph of the first run, counter moves of the first run)"""
    c = pkg.Context(backend)
    ins, outs = build(c)
    p, t = _pad(c, pkg)
    c.alloc()
    g = c.graph()
    res, k0, moved = [], None, {}
    before = {k: backend.get_stat(k) for k in stats} if counted else {}
    try:
        for n, feeds in enumerate(feed_sets):
            for name, T in ins.items():
                backend.tensor_set(T, feeds[name])
            backend.tensor_set(p, np.ones(64, np.float32))
            backend.graph_compute(g)
            if n == 0 and counted:
                k0 = backend.get_stat("kernels_last_graph")
                moved = {k: backend.get_stat(k) - before[k] for k in stats}
            res.append([backend.tensor_get(o).copy() for o in outs])
    finally:
        c.free()
    return res, k0, moved


def _compare(got, want, bar, what):
    for k, (a, b) in enumerate(zip(got, want)):
        if bar == 0 or a.dtype == np.float16:                              # copies, and masks (which hold -inf): bit-exact
            assert a.tobytes() == b.tobytes(), (what, k, int((a != b).sum()))
        else:
            assert np.isfinite(a).all(), (what, k)
            e = nmse(a, b)
            assert e < bar, (what, k, e)


def drive(pkg, be, ref_be, build, make_feeds, bar, stats=()):
    """defaults (eager, capture, replay on three input sets), fusion off, reference -- every output compared; returns the launch counts and counter moves"""
    feed_sets = [make_feeds(np.random.default_rng(seed)) for seed in (11, 12, 13)]
    r0 = be.get_stat("graph_replays")
    on, k_on, moved = _run(be, pkg, build, feed_sets, stats)
    replayed = be.get_stat("graph_replays") - r0
    be.set_option("fusion", 0)
    try:
        off, k_off, _ = _run(be, pkg, build, feed_sets[:1])
    finally:
        be.set_option("fusion", 1)
    ref, _, _ = _run(ref_be, pkg, build, feed_sets, counted=False)
    _compare(on[0], ref[0], bar, "eager run, fusion on")
    _compare(on[1], ref[1], bar, "captured run")
    _compare(on[2], ref[2], bar, "replayed run")
    _compare(off[0], ref[0], bar, "fusion off")
    assert replayed >= 1, "the graph did not replay"
    return k_on, k_off, moved


# ------------------------------------------------------------------------------------------------ vplain
# Whisper-shaped attention (encoders.py whisper): wq / wk / wv (F16 weights, f32 rows, q and v with a bias) as one grouped GEMM whose epilogue writes the K CAST as K rows and the
# V^T CAST through permute(1, 2, 0, 3) as V ROWS, then K.Q -> SOFT_MAX -> V^T.P -> CONT as one flash-attention launch on those rows.  Interloper: an unrelated f32 CONT between
# the CASTs and K.Q -- its copy is queued, and K.Q flushes the queue before the attention launch.  Bar: 2e-6 NMSE, the soft-max attention chain's (test_round4_gpu.py:250).
@pytest.mark.parametrize("interloper", [False, True])
def test_v_rows_layout_survives_a_queued_copy_before_the_attention(pkg, be, ref_be, interloper):
    F32, F16 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16
    D, H, n = 64, 4, 150
    S = D * H

    def build(c):
        x = c.new_tensor(F32, S, n)
        wq, wk, wv = (c.new_tensor(F16, S, S) for _ in range(3))
        bq, bv = c.new_tensor(F32, S), c.new_tensor(F32, S)
        z = c.new_tensor(F32, 24, 16)
        Q = c.add(c.mul_mat(wq, x), bq)
        K = c.mul_mat(wk, x)
        V = c.add(c.mul_mat(wv, x), bv)
        Qp = c.permute(c.reshape(Q, D, H, n), 0, 2, 1, 3)
        Kp = c.permute(c.cast(c.reshape(K, D, H, n), F16), 0, 2, 1, 3)
        Vt = c.cast(c.permute(c.reshape(V, D, H, n), 1, 2, 0, 3), F16)
        outs = []
        if interloper:
            outs.append(c.cont(c.transpose(z)))
        kq = c.soft_max_ext(c.mul_mat(Kp, Qp), None, 1.0 / np.sqrt(D), 0.0)
        out = c.cont(c.permute(c.mul_mat(Vt, kq), 0, 2, 1, 3), S, n)
        return dict(x=x, wq=wq, wk=wk, wv=wv, bq=bq, bv=bv, z=z), [out] + outs

    def feeds(rng):
        w = lambda: (rng.standard_normal((S, S)) / np.sqrt(S)).astype(np.float16)
        return dict(x=rng.standard_normal((n, S)).astype(np.float32), wq=w(), wk=w(), wv=w(), bq=(0.1 * rng.standard_normal(S)).astype(np.float32),
                    bv=(0.1 * rng.standard_normal(S)).astype(np.float32), z=rng.standard_normal((16, 24)).astype(np.float32))

    k_on, k_off, moved = drive(pkg, be, ref_be, build, feeds, 2e-6, stats=("attn_vrows_launches",))
    assert moved["attn_vrows_launches"] == 1, moved                     # the attention ran on the V rows the GEMM epilogue wrote
    assert k_on < k_off, (k_on, k_off)


# ------------------------------------------------------------------------------------------------ cq + concat tail
# Token2Wav's causal-convolution cache shift (graph_exec_t2w.cpp exec_concat_tail): x = CONT(permute) -> CONT(x) -> CONCAT(cache, ., dim 1) -> CONT -> CONT(VIEW of the last
# frames), run as one copy of the kept frames out of x.  x is the output of a copy that is still queued when the tail runs.  "batched": the tail's copy joins the queue;
# "direct": the copy queue off (option copy_batch 0), the tail launches its own copy.  Pure copies: bit-exact.
@pytest.mark.parametrize("tail", ["batched", "direct"])
def test_concat_tail_reads_a_queued_copy(pkg, be, ref_be, tail):
    F32 = pkg.GGML_TYPE_F32
    C_, P, dt, keep = 64, 3, 8, 3

    def build(c):
        xin = c.new_tensor(F32, dt, C_)
        cache = c.new_tensor(F32, C_, P)
        x = c.cont(c.transpose(c.scale(xin, 2.0)))                      # [C, dt]: a copy of an in-graph result (not a lazy one of a leaf), queued
        n0 = c.cont(x)
        n1 = c.concat(cache, n0, 1)                                     # [C, P + dt]
        n2 = c.cont(n1)
        v = c.view_3d(n2, C_, keep, 1, n2.t.nb[1], n2.t.nb[2], (P + dt - keep) * n2.t.nb[1])      # (a 3-D view, as the reference's builder: the matcher compares nb[2], which a 2-D view sets otherwise)
        n3 = c.cont(v)
        return dict(xin=xin, cache=cache), [n3]

    def feeds(rng):
        return dict(xin=rng.standard_normal((C_, dt)).astype(np.float32), cache=rng.standard_normal((P, C_)).astype(np.float32))

    if tail == "direct":
        be.set_option("copy_batch", 0)
    try:
        k_on, k_off, moved = drive(pkg, be, ref_be, build, feeds, 0, stats=("concat_tails",))
    finally:
        be.set_option("copy_batch", -1)
    assert k_on < k_off, (k_on, k_off)                                  # CONT + CONCAT + CONT + CONT ran as one copy
    assert moved["concat_tails"] == 1, moved                            # ... by exec_concat_tail (the copy queue alone gives the same count)


# ------------------------------------------------------------------------------------------------ rt
# Two RMS_NORM -> MUL(w) -> ROPE prefill chains of T >= 32 tokens (the norm + rope launch with the per-graph (cos, sin) table, graph_exec_llm.cpp) naming one positions leaf.
# Interloper: CPY(new_pos -> pos) between the chains; the second rope reads the CPY's result.  Bar: 1e-7 NMSE, the reference's default (test-backend-ops).
@pytest.mark.parametrize("T", [32, 64])
@pytest.mark.parametrize("interloper", [False, True])
def test_rope_table_is_recomputed_after_a_write_to_the_positions(pkg, be, ref_be, T, interloper):
    F32, I32 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_I32
    D, H = 128, 2

    def build(c):
        x1, x2 = c.new_tensor(F32, D, H, T), c.new_tensor(F32, D, H, T)
        w1, w2 = c.new_tensor(F32, D), c.new_tensor(F32, D)
        pos, new_pos = c.new_tensor(I32, T), c.new_tensor(I32, T)
        rope = lambda a, p: c.rope_ext(a, p, None, D, pkg.GGML_ROPE_TYPE_NEOX, 4096, 1e6, 1.0, 0.0, 1.0, 32.0, 1.0)
        r1 = rope(c.mul(c.rms_norm(x1, 1e-6), w1), pos)
        p2 = c.cpy(new_pos, pos) if interloper else pos
        r2 = rope(c.mul(c.rms_norm(x2, 1e-6), w2), p2)
        return dict(x1=x1, x2=x2, w1=w1, w2=w2, pos=pos, new_pos=new_pos), [r1, r2]

    def feeds(rng):
        p0 = int(rng.integers(0, 200))
        return dict(x1=rng.standard_normal((T, H, D)).astype(np.float32), x2=rng.standard_normal((T, H, D)).astype(np.float32),
                    w1=rng.uniform(0.5, 1.5, D).astype(np.float32), w2=rng.uniform(0.5, 1.5, D).astype(np.float32),
                    pos=np.arange(p0, p0 + T, dtype=np.int32), new_pos=np.arange(p0 + 500, p0 + 500 + T, dtype=np.int32)[::-1].copy())

    k_on, k_off, _ = drive(pkg, be, ref_be, build, feeds, 1e-7)
    assert k_on < k_off, (k_on, k_off)                                  # norm + mul + rope: one launch per chain (or both in one)


# ------------------------------------------------------------------------------------------------ mask_map
# Two prefill FLASH_ATTN_EXT nodes sharing an F16 mask (the matrix-core kernel with the mask tile map computed once per mask and graph run).  Interloper: a CPY of new rows into
# rows 32..63 of the mask between them; control: a CPY over the whole mask.  The new rows mask every key from 16 on where the old ones masked nothing.  Bar: 5e-4 NMSE, the
# reference's FLASH_ATTN_EXT bar (test_gpu_parity.py test_flash_attn_prefill_mfma).
@pytest.mark.parametrize("write", ["whole", "rows"])
def test_mask_tile_map_is_recomputed_after_a_write_into_the_mask(pkg, be, ref_be, write):
    F32, F16 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16
    D, nq, H, nkv = 128, 64, 2, 128
    r0 = 32 if write == "rows" else 0

    def build(c):
        q1, q2 = c.new_tensor(F32, D, nq, H), c.new_tensor(F32, D, nq, H)
        k, v = c.new_tensor(F16, D, nkv, H), c.new_tensor(F16, D, nkv, H)
        m = c.new_tensor(F16, nkv, nq)
        rows = c.new_tensor(F16, nkv, nq - r0)
        a1 = c.flash_attn_ext(q1, k, v, m, 1.0 / np.sqrt(D))
        c.cpy(rows, c.view_2d(m, nkv, nq - r0, m.t.nb[1], r0 * m.t.nb[1]))
        a2 = c.flash_attn_ext(q2, k, v, m, 1.0 / np.sqrt(D))
        return dict(q1=q1, q2=q2, k=k, v=v, m=m, rows=rows), [a1, a2, m]

    def feeds(rng):
        m = np.zeros((nq, nkv), np.float16)
        for i in range(32):
            m[i, 64 + i + 1:] = -np.inf                                 # rows 0..31 causal at an offset, rows 32..63 see every key
        rows = np.zeros((nq - r0, nkv), np.float16)
        rows[:, 16:] = -np.inf
        return dict(q1=rng.standard_normal((H, nq, D)).astype(np.float32), q2=rng.standard_normal((H, nq, D)).astype(np.float32),
                    k=rng.standard_normal((H, nkv, D)).astype(np.float16), v=rng.standard_normal((H, nkv, D)).astype(np.float16), m=m, rows=rows)

    k_on, k_off, _ = drive(pkg, be, ref_be, build, feeds, 5e-4)
    assert k_on < k_off, (k_on, k_off)                                  # the copy queued instead of launched on its own


# ------------------------------------------------------------------------------------------------ act
# MUL_MAT(W1, x), a CPY into one column of x, MUL_MAT(W2, x): the second product must not take the activation image the first one left.  Q4_K weights at 4 columns (the MMVQ
# mat-vec on the Q8_K image), Q8_0 weights at one column (the batch-1 mv1 form).  Bar: 5e-4 NMSE, the reference's MUL_MAT bar.
@pytest.mark.parametrize("wtype,N", [("q4_K", 4), ("q8_0", 1)])
@pytest.mark.parametrize("interloper", [False, True])
def test_activation_image_is_not_reused_after_a_write_into_x(pkg, be, ref_be, wtype, N, interloper):
    from llama_cpp_omni_amd.qwen3 import random_blocks
    F32 = pkg.GGML_TYPE_F32
    WT = pkg.GGML_TYPE_Q4_K if wtype == "q4_K" else pkg.GGML_TYPE_Q8_0
    K, M = 512, 256

    def build(c):
        x = c.new_tensor(F32, K, N)
        w1, w2 = c.new_tensor(WT, K, M), c.new_tensor(WT, K, M)
        row = c.new_tensor(F32, K)
        y1 = c.mul_mat(w1, x)
        if interloper:
            c.cpy(row, c.view_2d(x, K, 1, x.t.nb[1], (N - 1) * x.t.nb[1]))
        y2 = c.mul_mat(w2, x)
        return dict(x=x, w1=w1, w2=w2, row=row), [y1, y2]

    def feeds(rng):
        return dict(x=rng.standard_normal((N, K)).astype(np.float32), w1=random_blocks(rng, WT, M, K, 0.05), w2=random_blocks(rng, WT, M, K, 0.05),
                    row=rng.standard_normal(K).astype(np.float32))

    k_on, k_off, _ = drive(pkg, be, ref_be, build, feeds, 5e-4)
    if not interloper:
        assert k_on < k_off, (k_on, k_off)                              # one image for both products (and both in one launch where they batch)


# ------------------------------------------------------------------------------------------------ pn
# RMS_NORM -> MUL(w) feeding two batch-1 mat-vecs (the deferred norm: a K-quant consumer builds its image from the norm's INPUT in its prologue), with a CPY into the
# norm's input between them.  Q4_K and Q6_K consumers (mmv1 / the LDS-DMA engine), and Q8_0 consumers (mv1q).  Bar: 5e-4 NMSE, the reference's MUL_MAT bar.
@pytest.mark.parametrize("wtype", ["q4_K", "q6_K", "q8_0"])
@pytest.mark.parametrize("interloper", [False, True])
def test_deferred_norm_is_not_recomputed_from_an_overwritten_input(pkg, be, ref_be, wtype, interloper):
    from llama_cpp_omni_amd.qwen3 import random_blocks
    F32 = pkg.GGML_TYPE_F32
    WT = {"q4_K": pkg.GGML_TYPE_Q4_K, "q6_K": pkg.GGML_TYPE_Q6_K, "q8_0": pkg.GGML_TYPE_Q8_0}[wtype]
    K, M = 1024, 512

    def build(c):
        x, w = c.new_tensor(F32, K), c.new_tensor(F32, K)
        wa, wb = c.new_tensor(WT, K, M), c.new_tensor(WT, K, M)
        new_x = c.new_tensor(F32, K)
        h = c.mul(c.rms_norm(x, 1e-6), w)
        ya = c.mul_mat(wa, h)
        if interloper:
            c.cpy(new_x, x)
        yb = c.mul_mat(wb, h)
        return dict(x=x, w=w, wa=wa, wb=wb, new_x=new_x), [ya, yb]

    def feeds(rng):
        return dict(x=rng.standard_normal(K).astype(np.float32), w=rng.uniform(0.5, 1.5, K).astype(np.float32), wa=random_blocks(rng, WT, M, K, 0.05),
                    wb=random_blocks(rng, WT, M, K, 0.05), new_x=(3.0 * rng.standard_normal(K)).astype(np.float32))

    k_on, k_off, _ = drive(pkg, be, ref_be, build, feeds, 5e-4)
    if not interloper:
        assert k_on < k_off, (k_on, k_off)


# ------------------------------------------------------------------------------------------------ pr
# A lone prefill GEMM + residual whose result is left as split-K slabs for the RMS_NORM behind it (gemm_reduce_rms_norm).  Interloper: a SCALE (or a CPY) reads the result
# before the norm does -- the reduction must be materialised first.  Bar: 5e-4 NMSE, the reference's MUL_MAT bar (f16-rounded operands in the GEMM).
@pytest.mark.parametrize("reader", [None, "scale", "cpy"])
def test_split_k_result_is_reduced_before_another_reader(pkg, be, ref_be, reader):
    F32, F16 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16
    K, M, N = 2048, 256, 64

    def build(c):
        x, r = c.new_tensor(F32, K, N), c.new_tensor(F32, M, N)
        w, nw = c.new_tensor(F16, K, M), c.new_tensor(F32, M)
        a = c.add(c.mul_mat(w, x), r)
        outs = []
        if reader == "scale":
            outs.append(c.scale(a, 2.0))
        elif reader == "cpy":
            outs.append(c.cpy(a, c.new_tensor(F32, M, N)))
        y = c.mul(c.rms_norm(a, 1e-6), nw)
        return dict(x=x, r=r, w=w, nw=nw), [y] + outs

    def feeds(rng):
        return dict(x=rng.standard_normal((N, K)).astype(np.float32), r=rng.standard_normal((N, M)).astype(np.float32),
                    w=(rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float16), nw=rng.uniform(0.5, 1.5, M).astype(np.float32))

    k_on, k_off, _ = drive(pkg, be, ref_be, build, feeds, 5e-4)
    assert k_on < k_off, (k_on, k_off)
