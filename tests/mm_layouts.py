"""MUL_MAT under strided, batched and view operands: the case table, its numpy mirror and the tensor builders (test_mul_mat_layouts_host.py, test_mul_mat_layouts_gpu.py).

route_mul_mat (csrc/graph_plan.cpp) sends a MUL_MAT node down one of eight paths and supports_op admits it with almost no condition on layout, so every path has
to honour nb[1..3] of both operands, any ne02 x ne03 batch and any broadcast ratio.  This module states, per route, the shapes that reach it and crosses them with

  src1 layouts  (logical [K, N, ne12, ne13])
    dense     a plain tensor
    rowpad16  rows 16 bytes apart from dense: a view_4d of a parent with K + 4 floats per row
    rowpad4   parent rows of K + 1 floats, the view 4 bytes in: nb[1] % 16 != 0 and a base that is 4-byte aligned only
    perm0213  a parent [K, ne12, N, ne13] through permute(0, 2, 1, 3): the shape libllama gives q
    gap2      the first N of N + 3 rows of each slice: nb[2] > N * nb[1], rows dense
    perm0132  ne13 > 1 with dims 2 and 3 swapped: nb[3] != ne12 * nb[2]
  src0 layouts
    dense
    rowpad    nb[1] = row_size + one block (F16: 16 bytes where the dense row is a multiple of 16 bytes, the rows the F16 GEMM admits)
    rowoff    rows 1 .. M of a parent with M + 1 rows: the base is as aligned as one row is long (Q6_K at K = 256, Q8_0 / Q4_0 at K = 96: 2 bytes; Q4_1 at K = 96: 4)
    kvperm    F16 only: a cache [D, HK, n] seen as [D, n, HK]
  batch / broadcast tuples (ne02, ne03, r2, r3): BATCHES

Every padding cell of a src1 parent holds 1e30 and every padding byte of a src0 parent 0xFF (a NaN scale in every block format), so a read past a row shows.

A combination is left out only where excluded() names the line of route_mul_mat / supports_op that sends it elsewhere; route_of() and admitted() restate those two
functions so that the host test can hold every case, and every exclusion, against them.  launches() states the profile-class counts each case must produce.
No GPU code here.
"""
import zlib
from collections import namedtuple

import numpy as np

F32, F16, Q4_0, Q4_1, Q5_1, Q8_0, Q2_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, BF16 = 0, 1, 2, 3, 7, 8, 10, 12, 13, 14, 20, 23, 30
TRAITS = {F32: (1, 4), F16: (1, 2), BF16: (1, 2), Q4_0: (32, 18), Q4_1: (32, 20), Q5_1: (32, 24), Q8_0: (32, 34), IQ4_NL: (32, 18),
          Q2_K: (256, 84), Q4_K: (256, 144), Q5_K: (256, 176), Q6_K: (256, 210), IQ4_XS: (256, 136)}          # type -> (block elements, block bytes)
TNAME = {F32: "f32", F16: "f16", BF16: "bf16", Q4_0: "q4_0", Q4_1: "q4_1", Q5_1: "q5_1", Q8_0: "q8_0", IQ4_NL: "iq4_nl", Q2_K: "q2_K", Q4_K: "q4_K", Q5_K: "q5_K",
         Q6_K: "q6_K", IQ4_XS: "iq4_xs"}
FLOAT_TYPES = (F32, F16, BF16)
# the activation image each weight type's mat-vec reads, and the profile class its launches are booked under (graph_plan.cpp MMV_ROWS)
ACT = {Q4_K: "q8k", Q5_K: "q8k", Q6_K: "q8k", IQ4_XS: "q8k", Q2_K: "q8k", Q8_0: "q80", Q4_0: "q80", IQ4_NL: "q80", Q4_1: "q81", Q5_1: "q81", F16: "f16", F32: "f32"}
MMV_CLASS = {Q4_K: "mmv_q4k", Q5_K: "mmv_f32", Q6_K: "mmv_q6k", Q8_0: "mmv_q80", Q4_0: "mmv_f32", IQ4_NL: "mmv_iq4nl", IQ4_XS: "mmv_iq4xs", Q4_1: "mmv_q41",
             Q5_1: "mmv_q51", Q2_K: "mmv_q2k", F16: "mmv_f16", F32: "mmv_f32"}
CLASSES = ("gemm_f16", "gemm_any_f16", "gemm_any_f32", "gemm_any_bf16", "mmq_q4k", "mmq_q6k", "mmq_tile", "act_convert", "dequant_f16") + tuple(sorted(set(MMV_CLASS.values())) + ["mmv_q3k"])

ROUTES = ("MM_MMV", "MM_MMV_HEADS", "MM_MMQ", "MM_MMQ_TILE", "MM_GEMM_F16", "MM_GEMM_F16_HEADS", "MM_GEMM_BF16", "MM_GEMM_ANY")
INTEGER_ROUTES = ("MM_MMV", "MM_MMQ", "MM_MMQ_TILE")
X_LAYOUTS = ("dense", "rowpad16", "rowpad4", "perm0213", "gap2", "perm0132")
W_LAYOUTS = ("dense", "rowpad", "rowoff", "kvperm")
BATCHES = ((1, 1, 1, 1), (2, 1, 1, 1), (2, 1, 3, 1), (1, 2, 1, 2), (2, 2, 2, 2))          # (ne02, ne03, r2, r3)
M_ROWS = 70                                                                                    # ragged against the 32- and 64-row tiles
X_POISON, W_POISON = 1e30, 0xFF
MMQ_MIN_COLS, MMQ_MAX_COLS, MMV_MAX_COLS = 6, 64, 8                                            # graph_plan.cpp mmq_min_cols / mmq_max_cols, kernels.hpp MI_MMVQ_MAX_COLS

Case = namedtuple("Case", "route wtype xtype K M N batch xl wl wbuf")
Case.id = property(lambda c: "%s-%s%s-K%d-M%d-N%d-b%d%d%d%d-%s-%s%s" % ((c.route[3:].lower(), TNAME[c.wtype], "xf16" if c.xtype == F16 else "", c.K, c.M, c.N) + tuple(c.batch) +
                                                                       (c.xl, c.wl, "-resident" if c.wbuf == "weights" else "")))
Geo = namedtuple("Geo", "pne ne nb off perm")          # parent shape, view shape, view strides (bytes), view offset (bytes), the permutation that makes the view (or None: view_4d)


def row_size(t, K):
    blck, size = TRAITS[t]
    assert K % blck == 0
    return K // blck * size


def ne1x(case):
    ne02, ne03, r2, r3 = case.batch
    return ne02 * r2, ne03 * r3


# ------------------------------------------------------------------------------------------------ layouts
def x_geo(xl, xtype, K, N, ne12, ne13):
    e = TRAITS[xtype][1]
    if xl == "dense":
        return Geo((K, N, ne12, ne13), (K, N, ne12, ne13), (e, K * e, K * N * e, K * N * ne12 * e), 0, None)
    if xl == "rowpad16":
        P = K + 16 // e
        return Geo((P, N, ne12, ne13), (K, N, ne12, ne13), (e, P * e, P * N * e, P * N * ne12 * e), 0, None)
    if xl == "rowpad4":
        P = K + 4 // e
        return Geo((P, N, ne12, ne13), (K, N, ne12, ne13), (e, P * e, P * N * e, P * N * ne12 * e), 4, None)
    if xl == "perm0213":
        return Geo((K, ne12, N, ne13), (K, N, ne12, ne13), (e, K * ne12 * e, K * e, K * ne12 * N * e), 0, (0, 2, 1, 3))
    if xl == "gap2":
        return Geo((K, N + 3, ne12, ne13), (K, N, ne12, ne13), (e, K * e, K * (N + 3) * e, K * (N + 3) * ne12 * e), 0, None)
    if xl == "perm0132":
        return Geo((K, N, ne13, ne12), (K, N, ne12, ne13), (e, K * e, K * N * ne13 * e, K * N * e), 0, (0, 1, 3, 2))
    raise ValueError(xl)


def w_pad_bytes(wtype, K):
    """rowpad: one block -- for F16, 16 bytes where the dense row is a multiple of 16 bytes (gemm_f16_takes, graph_plan.cpp:307, and k_head, :338, test nb[1] % 16)"""
    if wtype == F16 and row_size(F16, K) % 16 == 0:
        return 16
    return TRAITS[wtype][1]


def w_geo(wl, wtype, K, M, ne02, ne03):
    blck, size = TRAITS[wtype]
    rs = row_size(wtype, K)
    if wl == "dense":
        return Geo((K, M, ne02, ne03), (K, M, ne02, ne03), (size, rs, M * rs, M * ne02 * rs), 0, None)
    if wl == "rowpad":
        pad = w_pad_bytes(wtype, K)
        P, nb1 = K + pad // size * blck, rs + pad
        return Geo((P, M, ne02, ne03), (K, M, ne02, ne03), (size, nb1, M * nb1, M * ne02 * nb1), 0, None)
    if wl == "rowoff":
        return Geo((K, M + 1, ne02, ne03), (K, M, ne02, ne03), (size, rs, (M + 1) * rs, (M + 1) * ne02 * rs), rs, None)
    if wl == "kvperm":
        return Geo((K, ne02, M, ne03), (K, M, ne02, ne03), (size, ne02 * rs, rs, ne02 * M * rs), 0, (0, 2, 1, 3))
    raise ValueError(wl)


def geometry(case):
    ne02, ne03, _, _ = case.batch
    ne12, ne13 = ne1x(case)
    return w_geo(case.wl, case.wtype, case.K, case.M, ne02, ne03), x_geo(case.xl, case.xtype, case.K, case.N, ne12, ne13)


def parent_bytes(t, pne):
    return row_size(t, pne[0]) * pne[1] * pne[2] * pne[3]


def np_view(parent_u8, t, geo, rows_as_bytes):
    """numpy mirror of a view: the parent's bytes seen through (ne, nb, off) as [ne3, ne2, ne1, row] -- row as bytes (block formats) or as elements"""
    _, size = TRAITS[t]
    if rows_as_bytes:
        return np.ndarray((geo.ne[3], geo.ne[2], geo.ne[1], row_size(t, geo.ne[0])), np.uint8, parent_u8, geo.off, (geo.nb[3], geo.nb[2], geo.nb[1], 1))
    dt = {4: np.float32, 2: np.uint16}[size]
    return np.ndarray((geo.ne[3], geo.ne[2], geo.ne[1], geo.ne[0]), dt, parent_u8, geo.off, (geo.nb[3], geo.nb[2], geo.nb[1], geo.nb[0]))


def x_poison_bytes(xtype):
    """1e30 as the parent's element: f32, or f16 -- where it is +inf"""
    return np.array([X_POISON], np.float32).view(np.uint8) if xtype == F32 else np.array([np.inf], np.float16).view(np.uint8)


def poisoned_parent(t, geo, logical, is_weight):
    """the parent's bytes: poison everywhere, the logical array ([ne3, ne2, ne1, row bytes] uint8 for weights, [ne3, ne2, ne1, K] f32 / f16-as-u16 for activations) through the view"""
    n = parent_bytes(t, geo.pne)
    if is_weight:
        buf = np.full(n, W_POISON, np.uint8)
        np_view(buf, t, geo, True)[...] = logical
    else:
        p = x_poison_bytes(t)
        buf = np.tile(p, n // p.size)
        np_view(buf, t, geo, False)[...] = logical
    return buf


# ------------------------------------------------------------------------------------------------ supports_op / route_mul_mat, restated
def _aligned(off, nbs, a):
    return off % a == 0 and all(nb % a == 0 for nb in nbs)


def admitted(wtype, xtype, wg, xg):
    """supports_op, case GGML_OP_MUL_MAT (graph_plan.cpp:15-41), for a dst that is a fresh F32 tensor; bases are at least 16-byte aligned, so a view's alignment is its offset's"""
    K = wg.ne[0]
    if wtype == BF16:
        return xtype == F32 and wg.nb[0] == 2 and xg.nb[0] == 4 and wg.nb[1] >= K * 2 and xg.ne[2] % wg.ne[2] == 0 and xg.ne[3] % wg.ne[3] == 0 and xg.ne[2] * xg.ne[3] <= 65535
    if wtype not in ACT:
        return False
    if xtype != F32 and not (xtype == F16 and ACT[wtype] == "f16"):
        return False
    if K % TRAITS[wtype][0] != 0 or wg.nb[0] != TRAITS[wtype][1] or xg.nb[0] != TRAITS[xtype][1]:
        return False
    if wg.nb[1] < row_size(wtype, K):                                                      # :25 transposed weights
        return False
    if xg.ne[2] % wg.ne[2] != 0 or xg.ne[3] % wg.ne[3] != 0:
        return False
    if ACT[wtype] in ("q8k", "q80", "q81"):                                                # :27-32
        al = 16 if wtype in (Q4_K, Q5_K) else 4 if wtype in (Q4_1, Q5_1, Q2_K) else 2
        if wg.nb[1] % al != 0 or (al == 4 and wg.off % 4 != 0):
            return False
    return True                                                                            # (:35-39, a column past 152 KiB of LDS: no shape here comes near it)


def _mmq_ok(wtype, K, off, nb1):
    if wtype in (Q4_K, Q5_K):
        return K % 256 == 0 and nb1 % 16 == 0 and off % 16 == 0
    if wtype == Q6_K:
        return K % 256 == 0 and nb1 % 2 == 0 and off % 2 == 0
    return False


def _mmq_takes(wtype, xtype, wg, xg):
    K, N = wg.ne[0], xg.ne[1]
    return (wtype in (Q4_K, Q5_K, Q6_K) and xtype == F32 and MMQ_MIN_COLS <= N <= MMQ_MAX_COLS and _mmq_ok(wtype, K, wg.off, wg.nb[1]) and
            (wg.ne[2] == 1 or _mmq_ok(wtype, K, wg.off + wg.nb[2], wg.nb[1])) and (wg.ne[3] == 1 or _mmq_ok(wtype, K, wg.off + wg.nb[3], wg.nb[1])))


def route_of(wtype, xtype, wg, xg, mmq_tile=False):
    """route_mul_mat (graph_plan.cpp:314-346) -> (path, activation image, k_head)"""
    K, M, N, nbatch = wg.ne[0], wg.ne[1], xg.ne[1], xg.ne[2] * xg.ne[3]
    act = ACT.get(wtype)
    if (mmq_tile and wtype == Q4_K and xtype == F32 and N > MMQ_MAX_COLS and nbatch == 1 and wg.ne[2] == 1 and wg.ne[3] == 1 and xg.nb[0] == 4 and      # :276-284
            xg.nb[1] % 16 == 0 and xg.off % 16 == 0 and K % 256 == 0 and wg.nb[1] % 16 == 0 and wg.off % 16 == 0):
        return "MM_MMQ_TILE", "q8kt", 0
    gemm = (N >= MMV_MAX_COLS + 1 and not _mmq_takes(wtype, xtype, wg, xg) and wtype in ACT and wtype != F32 and K % 32 == 0 and                          # :299-312
            not (wtype == F16 and not _aligned(wg.off, wg.nb[1:], 16)) and
            not (wtype == F16 and nbatch > 1 and K % 64 != 0 and xtype == F32 and nbatch <= 65535))
    if gemm:
        if wtype == F16 and 1 < nbatch <= 65535 and K % 64 == 0:                                                                                        # :324
            return "MM_GEMM_F16_HEADS", "f16", 0
        return "MM_GEMM_F16", "f16", 0
    if wtype == BF16:
        return "MM_GEMM_BF16", None, 0
    k_head_sized = K - K % 64 if (wtype == F16 and xtype == F32 and nbatch == 1 and K % 64 != 0 and K >= 512 and N > MMV_MAX_COLS) else 0              # :330
    if wtype in (F32, F16) and N > MMV_MAX_COLS and (xtype == F32 or wtype == F16) and nbatch <= 65535:                                                   # :334-340
        return "MM_GEMM_ANY", act, k_head_sized if (wg.nb[1] % 16 == 0 and wg.off % 16 == 0) else 0
    if (wtype in (F16, F32) and nbatch > 1 and N <= MMV_MAX_COLS and nbatch <= 65535 and
            (act != "f32" or xg.ne[3] == 1 or xg.nb[3] == xg.ne[2] * xg.nb[2])):                                                                        # :342-343
        return "MM_MMV_HEADS", act, 0
    if _mmq_takes(wtype, xtype, wg, xg):                                                                                                                # :344
        return "MM_MMQ", act, 0
    return "MM_MMV", act, 0


def case_route(case):
    wg, xg = geometry(case)
    return route_of(case.wtype, case.xtype, wg, xg, mmq_tile=case.route == "MM_MMQ_TILE")


def reads_image(case):
    """does the route read a dense activation image that prepare_act builds (so that the layout of src1 cannot change one bit of the result)?  Not the mat-vecs on F32
    weights (ACT_F32: the rows in place), not the any-shape GEMM outside its split form (x in place), not BF16 weights (x in place)"""
    path, act, k_head = case_route(case)
    if path in ("MM_MMV", "MM_MMV_HEADS"):
        return act != "f32"
    if path == "MM_GEMM_ANY":
        return k_head > 0
    return path != "MM_GEMM_BF16"


# ------------------------------------------------------------------------------------------------ the launches a case must produce
def launches(case):
    """profile-class counts (prof_<class>_n) of the FIRST run of the case's graph -- one MUL_MAT node and a tail of SCALE nodes -- with option "profile" on, fusion at its default.
    2-D nodes go through the matchers of exec_mul_mat (graph_exec_llm.cpp) in front of op_mul_mat: the grouped GEMM launch (K % 64 == 0), the K-quant multi / batch-1 mat-vec
    launches (which book Q5_K under mmv_q6k), the in-staging de-quantisation of Q4_K / Q6_K blocks without a resident image.  Batched nodes go through op_mul_mat (graph_exec.cpp)."""
    path, act, k_head = case_route(case)
    wg, xg = geometry(case)
    K, N, ne12, ne13 = case.K, case.N, xg.ne[2], xg.ne[3]
    ne02, ne03, r2, r3 = case.batch
    nsl, two_d = ne12 * ne13, ne12 * ne13 == 1 and ne02 * ne03 == 1
    n = dict.fromkeys(CLASSES, 0)
    if path == "MM_MMV":
        cls, per, conv = MMV_CLASS[case.wtype], -(-N // MMV_MAX_COLS), 0 if act == "f32" else 1
        if two_d and case.wtype in (Q4_K, Q5_K, Q6_K):                    # exec_mul_mat (b): one launch for up to 8 columns; one column of Q4_K / Q6_K: the batch-1 kernel, which
            cls, per = "mmv_q4k" if case.wtype == Q4_K else "mmv_q6k", 1   # quantises a 16-byte aligned f32 row itself (mv1_source)
            if N == 1 and case.wtype != Q5_K and xg.off % 16 == 0:
                conv = 0
        if two_d and N == 1 and K <= 4096 and (case.wtype == Q8_0 or (case.wtype == F16 and _aligned(wg.off, wg.nb[1:2], 16))) and xg.off % 16 == 0:
            conv = 0                                                       # the Q8_0 / F16 twin of the batch-1 kernel (mmv1q.hip)
        n[cls] += nsl * per
        n["act_convert"] = conv
    elif path == "MM_MMV_HEADS":
        n[MMV_CLASS[case.wtype]] += 1
        n["act_convert"] = 0 if act == "f32" else 1
    elif path == "MM_MMQ":
        n["mmq_q4k" if case.wtype == Q4_K else "mmq_q6k"] = nsl * -(-N // 32)
        n["act_convert"] = 1
    elif path == "MM_MMQ_TILE":
        n["mmq_tile"], n["act_convert"] = 1, 1
    elif path == "MM_GEMM_F16":
        n["act_convert"] = 1
        quant = case.wtype != F16
        if two_d and K % 64 == 0:                                          # exec_gemm_group
            n["gemm_f16"] = 1
            staging = case.wtype in (Q4_K, Q6_K) and K % 256 == 0 and wg.nb[1] % (16 if case.wtype == Q4_K else 2) == 0 and wg.off % 16 == 0      # kq_in_staging
            n["dequant_f16"] = 0 if not quant or (case.wbuf != "weights" and staging) else 1
        else:                                                              # mm_gemm_f16, slice by slice
            n["gemm_f16"] = nsl
            if quant and case.wbuf == "weights":
                n["dequant_f16"] = ne02 * ne03                             # one resident image per weight slice, built on first use
            elif quant:
                last = None                                                # w_scratch, reused while the weight slice stays (last_w)
                for i13 in range(ne13):
                    for i12 in range(ne12):
                        s = (i12 // r2, i13 // r3)
                        n["dequant_f16"] += s != last
                        last = s
    elif path == "MM_GEMM_F16_HEADS":
        n["gemm_f16"], n["act_convert"] = 1, 1
    elif path == "MM_GEMM_BF16":
        n["gemm_any_bf16"] = 1
    elif path == "MM_GEMM_ANY":
        n["gemm_any_f16" if case.wtype == F16 else "gemm_any_f32"] = 1
        if k_head:
            n["gemm_f16"], n["act_convert"] = 1, 1
    return n


# ------------------------------------------------------------------------------------------------ the table
def _shapes():
    S = {r: [] for r in ROUTES}
    # MM_MMV.  The K-quants with int8-MFMA kernels (Q4_K / Q5_K / Q6_K) leave it at mmq_min_cols() = 6 columns (route_mul_mat :344), so they stop at 5 here; their 8-column
    # case is MM_MMQ's.
    for t in (Q4_K, Q5_K, Q6_K):
        S["MM_MMV"] += [(t, F32, 512, M_ROWS, N) for N in (1, 5)]
    for t in (IQ4_XS, Q2_K):
        S["MM_MMV"] += [(t, F32, 512, M_ROWS, N) for N in (1, 5, 8)]
    for t in (Q8_0, Q4_0, Q4_1, Q5_1, IQ4_NL):
        S["MM_MMV"] += [(t, F32, 96, M_ROWS, N) for N in (1, 5, 8)]
    S["MM_MMV_HEADS"] = [(t, F32, K, M_ROWS, N) for t in (F16, F32) for K in (64, 72) for N in (1, 8)]
    S["MM_MMQ"] = [(t, F32, K, M_ROWS, N) for t in (Q4_K, Q5_K, Q6_K) for K in (256, 1024) for N in (6, 33, 64)]
    S["MM_MMQ_TILE"] = [(Q4_K, F32, 512, M_ROWS, 70)]
    S["MM_GEMM_F16"] = ([(t, F32, 512, M_ROWS, N) for t in (Q4_K, Q6_K) for N in (65, 70)] + [(t, F32, 96, M_ROWS, N) for t in (Q8_0, Q4_1) for N in (9, 70)] +
                        [(IQ4_XS, F32, 512, M_ROWS, N) for N in (9, 70)] + [(F16, F16, 96, M_ROWS, N) for N in (9, 70)])
    S["MM_GEMM_F16_HEADS"] = [(F16, F32, 64, M_ROWS, N) for N in (9, 70)]
    S["MM_GEMM_BF16"] = [(BF16, F32, 100, M_ROWS, N) for N in (1, 5, 70)]
    # MM_GEMM_ANY.  The split form (k_head) is granted to results with 16-byte rows only (mm_gemm_any, graph_exec.cpp: out->nb[1] % 16 == 0): M = 72 there, not 70.
    S["MM_GEMM_ANY"] = [(F32, F32, 72, M_ROWS, 70), (F16, F32, 100, M_ROWS, 70), (F16, F32, 520, 72, 70)]
    return S


SHAPES = _shapes()


def excluded(route, shape, xl, wl, batch):
    """the reason a combination is not in the table, or None.  Each reason is either the layout's own definition or a line of route_mul_mat / supports_op (graph_plan.cpp)
    that sends the node to another route; the host test holds the latter against route_of()."""
    wtype, xtype, K, M, N = shape
    ne02, ne03, r2, r3 = batch
    ne12, ne13 = ne02 * r2, ne03 * r3
    nbatch = ne12 * ne13
    if xl == "perm0132" and ne13 == 1:
        return "definition: perm0132 swaps dims 2 and 3 of a src1 with ne13 > 1"
    if wl == "kvperm" and (wtype != F16 or ne02 == 1):
        return "definition: kvperm is an F16 cache [D, HK, n] seen per head, HK > 1"
    if route == "MM_MMQ_TILE":
        if nbatch != 1:
            return "route_mul_mat :281 (mmq_tile_takes): 2-D operands only"
        if xl == "rowpad4":
            return "route_mul_mat :282 (mmq_tile_takes): src1 rows and base 16-byte aligned, else MM_GEMM_F16"
    if route in ("MM_MMV_HEADS", "MM_GEMM_F16_HEADS") and nbatch == 1:
        return "route_mul_mat :324 / :342: the per-head launches take nbatch > 1"
    if route == "MM_MMV_HEADS" and wtype == F32 and ne13 > 1:
        xg = x_geo(xl, xtype, K, N, ne12, ne13)
        if xg.nb[3] != ne12 * xg.nb[2]:                                 # perm0132, and perm0213 at more than one column
            return "route_mul_mat :343: f32 rows are read in place through ONE batch stride; nb[3] != ne12 * nb[2] goes to MM_MMV (EXTRA_CASES holds it there)"
    if route == "MM_GEMM_ANY" and K >= 512 and nbatch != 1:
        return "route_mul_mat :330: the split form takes 2-D operands (batched it is the plain any-shape launch, which the K = 100 shape covers)"
    return None


def _wbufs(route, shape):
    return ("any", "weights") if route == "MM_GEMM_F16" and shape[0] not in FLOAT_TYPES else ("any",)


def _first(seq, start, ok):
    """the first element of seq, counted cyclically from position start, that ok() accepts -- or None"""
    for k in range(len(seq)):
        e = seq[(start + k) % len(seq)]
        if ok(e):
            return e
    return None


def _build_table():
    """Three rules, per route; a case is (shape, src1 layout, src0 layout, batch tuple), and quantised MM_GEMM_F16 cases come once per kind of buffer (_wbufs):
      1. every (src1 layout, src0 layout, batch) triple with ONE shape -- the t-th triple starts its search at shape t, so the shapes take turns; a triple that no shape of
         the route admits goes to OMITTED with excluded()'s reason;
      2. every shape with every src0 layout (the alignment rules are per type and row length), on some (src1 layout, batch) pair -- the j-th shape starts at pair j;
      3. every weight type with every src1 layout (the image kernels are per activation kind), on some (shape of the type, plain src0 layout, batch)."""
    cases, omitted = [], []
    triples = [(xl, wl, b) for b in BATCHES for wl in W_LAYOUTS for xl in X_LAYOUTS]
    pairs = [(xl, b) for b in BATCHES for xl in X_LAYOUTS]
    plain_w = [wl for wl in W_LAYOUTS if wl != "kvperm"]
    for route in ROUTES:
        shapes = SHAPES[route]
        seen = set()

        def add(shape, xl, wl, b):
            for wbuf in _wbufs(route, shape):
                c = Case(route, shape[0], shape[1], shape[2], shape[3], shape[4], b, xl, wl, wbuf)
                if c not in seen:
                    seen.add(c)
                    cases.append(c)
        for t, (xl, wl, b) in enumerate(triples):                                                      # rule 1
            shape = _first(shapes, t, lambda sh: excluded(route, sh, xl, wl, b) is None)
            if shape is None:
                omitted.append((route, xl, wl, b, excluded(route, shapes[0], xl, wl, b)))
            else:
                add(shape, xl, wl, b)
        for j, shape in enumerate(shapes):                                                             # rule 2
            for wl in W_LAYOUTS:
                pair = _first(pairs, j, lambda p: excluded(route, shape, p[0], wl, p[1]) is None)
                if pair is not None:
                    add(shape, pair[0], wl, pair[1])
        for t in sorted({sh[0] for sh in shapes}):                                                     # rule 3
            rest = [(sh, wl, b) for b in BATCHES for wl in plain_w for sh in shapes if sh[0] == t]
            for a, xl in enumerate(X_LAYOUTS):
                pick = _first(rest, a, lambda r: excluded(route, r[0], xl, r[1], r[2]) is None)
                if pick is not None:
                    add(pick[0], xl, pick[1], pick[2])
    return cases, omitted


CASES, OMITTED = _build_table()

# MM_MMV on F32 weights: the batched node MM_MMV_HEADS refuses (route_mul_mat :343), one launch per slice on the rows in place
EXTRA_CASES = [Case("MM_MMV", F32, F32, K, M_ROWS, N, b, "perm0132", wl, "any") for K, N, b, wl in ((72, 5, (1, 2, 1, 2), "dense"), (64, 8, (2, 2, 2, 2), "rowpad"), (72, 1, (2, 2, 2, 2), "rowoff"))]
# MM_GEMM_F16_HEADS, ne12 = 7282 heads broadcast from one F16 weight slice, q-shaped src1: 9 * 7282 = 65538 rows, one more than convert_f32_f16_rows3's grid takes, so prepare_act
# falls back to its per-slice loop (the only case that does)
BIG_HEADS = Case("MM_GEMM_F16_HEADS", F16, F32, 64, M_ROWS, 9, (1, 1, 7282, 1), "perm0213", "dense", "any")
ALL_CASES = CASES + EXTRA_CASES + [BIG_HEADS]

# what supports_op must refuse (fixed here, not discovered): (name, wtype, K, the src0 view as a Geo)
DECLINED = [
    ("transposed weight (nb[1] < row_size)", F32, 72, Geo((M_ROWS, 72, 1, 1), (72, M_ROWS, 1, 1), (M_ROWS * 4, 4, 72 * M_ROWS * 4, 72 * M_ROWS * 4), 0, "transpose")),
    ("Q4_K with nb[1] % 16 != 0", Q4_K, 512, Geo((512 * (M_ROWS + 2), 1, 1, 1), (512, M_ROWS, 1, 1), (144, 288 + 8, M_ROWS * 296, M_ROWS * 296), 0, None)),
    ("Q4_1 with a base that is not 4-byte aligned", Q4_1, 96, Geo((96 * (M_ROWS + 1), 1, 1, 1), (96, M_ROWS, 1, 1), (20, 60, M_ROWS * 60, M_ROWS * 60), 2, None)),
]


def twin(case):
    """the same case on a dense src1"""
    return case._replace(xl="dense")


# ------------------------------------------------------------------------------------------------ data
def seed_of(case):
    """one seed per logical problem: the layouts of both operands and the kind of buffer do not enter"""
    return zlib.crc32(repr(case._replace(xl="dense", wl="dense", wbuf="any")).encode())


def f32_to_bf16_bits(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def make_data(case):
    """-> (W, X): W uint8 [ne03, ne02, M, row bytes], X [ne13, ne12, N, K] f32 (or f16 for F16 src1) -- the same for a case and its dense twin"""
    from llama_cpp_omni_amd import qwen3
    rng = np.random.default_rng(seed_of(case))
    ne02, ne03, _, _ = case.batch
    ne12, ne13 = ne1x(case)
    K, M, N = case.K, case.M, case.N
    if case.wtype == BF16:
        W = f32_to_bf16_bits((rng.standard_normal((ne03, ne02, M, K)) / np.sqrt(K)).astype(np.float32)).view(np.uint8).reshape(ne03, ne02, M, -1)
    elif case.wtype in (F32, F16):
        W = (rng.standard_normal((ne03, ne02, M, K)) / np.sqrt(K)).astype(np.float32 if case.wtype == F32 else np.float16).view(np.uint8).reshape(ne03, ne02, M, -1)
    else:
        W = qwen3.random_blocks(rng, case.wtype, ne03 * ne02 * M, K, std=0.05)
        if case.wtype in (Q4_1, Q5_1):
            # value = d * q + m: with the min where a quantiser puts it, m = -mid * d, the weights are zero-mean like every other format's here.  Left at random_blocks' positive
            # m every weight is positive, a column's result is mean(w) * sum(x) in every row, and its NMSE against the oracle's integers is the oracle's own Q8_1 rounding of
            # that one sum -- (sum of the rounding errors)^2 / (sum x)^2, heavy-tailed, 8e-4 at worst over a thousand correct columns, whatever M and K are
            blk = W.reshape(W.shape[0], K // 32, TRAITS[case.wtype][1])
            d = blk[..., 0:2].copy().view(np.float16).astype(np.float32)
            blk[..., 2:4] = (d * -(7.5 if case.wtype == Q4_1 else 15.5)).astype(np.float16).view(np.uint8)
        W = W.reshape(ne03, ne02, M, -1)
    X = rng.standard_normal((ne13, ne12, N, K)).astype(np.float32)
    if case.xtype == F16:
        X = X.astype(np.float16)
    return np.ascontiguousarray(W), X


def w_as_f64(wtype, W):
    """float weights [.., M, row bytes] uint8 -> float64 [.., M, K]"""
    if wtype == F32:
        return W.view(np.float32).astype(np.float64)
    if wtype == F16:
        return W.view(np.float16).astype(np.float64)
    assert wtype == BF16
    return bf16_bits_to_f32(W.view(np.uint16)).astype(np.float64)


def round_act(case, X):
    """the activations as the route rounds them, float64: f16 for the F16 images, bf16 against BF16 weights, untouched where the f32 rows are read in place"""
    path, act, k_head = case_route(case)
    X = np.asarray(X, np.float32)
    if path == "MM_GEMM_BF16":
        return bf16_bits_to_f32(f32_to_bf16_bits(X)).reshape(X.shape).astype(np.float64)
    if act == "f16":
        return X.astype(np.float16).astype(np.float64)
    return X.astype(np.float64)


# ------------------------------------------------------------------------------------------------ tensors
def build_view(ctx, parent_ctx, t, geo):
    """-> (parent tensor in parent_ctx, the view in ctx): permute() for the permuted layouts, view_4d for the rest"""
    parent = parent_ctx.new_tensor(t, *geo.pne)
    if geo.perm == "transpose":
        return parent, ctx.transpose(parent)
    if geo.perm is not None:
        return parent, ctx.permute(parent, *geo.perm)
    if geo.pne == geo.ne and geo.off == 0:
        return parent, parent
    return parent, ctx.view_4d(parent, geo.ne[0], geo.ne[1], geo.ne[2], geo.ne[3], geo.nb[1], geo.nb[2], geo.nb[3], geo.off)


def build_case(pkg, be, case, tail=8):
    """Two contexts -- the weights' (an ordinary buffer, or one marked GGML_BACKEND_BUFFER_USAGE_WEIGHTS) and the graph's -- with y = MUL_MAT(w view, x view) and a tail of SCALE
    nodes behind it, long enough for the graph to be captured on its second submission.  With be None nothing is allocated (the host test reads ne / nb).
    -> dict(wctx, ctx, w_parent, w, x_parent, x, y)"""
    wg, xg = geometry(case)
    wctx, ctx = pkg.Context(be), pkg.Context(be)
    wp, w = build_view(ctx, wctx, case.wtype, wg)
    xp, x = build_view(ctx, ctx, case.xtype, xg)
    y = ctx.mul_mat(w, x)
    z = y
    for _ in range(tail):
        z = ctx.scale(z, 1.0)
    if be is not None:
        wctx.alloc(usage=pkg.GGML_BACKEND_BUFFER_USAGE_WEIGHTS if case.wbuf == "weights" else pkg.GGML_BACKEND_BUFFER_USAGE_ANY)
        ctx.alloc()
    return dict(wctx=wctx, ctx=ctx, w_parent=wp, w=w, x_parent=xp, x=x, y=y)
