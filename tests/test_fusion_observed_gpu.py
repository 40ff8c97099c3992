"""Fusions that never write an interior node, with that node read from OUTSIDE the submitted cgraph (graph_exec_internal.hpp:35 is_out).

About twenty fusion sites of the executor skip the f32 result of an interior node: legal only while nobody else reads it.  The one guard is is_out(): the OUTPUT flag, or
exec_state::external -- the tensors whose whole-graph use count (ggml_cgraph::use_counts, found by probing visited_hash_set: graph_internal.hpp whole_use_count) exceeds
their uses inside the submitted split.  Here every site is one small graph (the builder its own test already uses, at the smallest shape its matcher accepts), run as

  control   nobody else reads the interior node; the fused path is taken -- proved by kernels_last_graph below the fusion-off run (the pad's launches taken out
            on both sides) and, where the site has one, by its launch counter
  output    flags |= GGML_TENSOR_FLAG_OUTPUT on the interior node
  split     the parent graph (Context.graph_parent: use counts and hash set as ggml_build_forward_expand leaves them) has one more node that reads the interior node --
            SCALE(t, 1), or for an f16 result a CPY into an f32 leaf -- behind the cut; the backend gets view(0, cut), then view(cut, n) as a second graph_compute, as
            the scheduler submits its splits (Graph.view = ggml_graph_view)
  view      (some sites) the outside reader reads a RESHAPE of the interior node: the view node behind the cut, or in front of it (then the VIEW is what a later split
            reads, and run_nodes' walk along view_src keeps the base's bytes alive)
  crowded   (some sites) split, with a parent table of exactly ggml_hash_size(nodes + leafs) slots in which the interior node's key lies off its home slot
            (graph_views.crowd; the construction test_graph_views_host.py checks against the reference)

Protocol: before the first graph_compute of a run the interior node, every output and the outside reader's result are filled with NaN through tensor_set (nothing left over
from another run can pass; not again in front of the second split, which reads what the first one wrote); three runs on three input sets (eager, captured, replayed; at
least one replay is asserted); in output / split the interior node read back with tensor_get, every final output and the outside reader's result are compared with the
reference CPU backend on the same graph, in control the final outputs.  Bars are each site's existing bar, quoted with file and line; bar 0 = bit-exact (copies, f16 stores
of values that are exact on both sides, and chains of IEEE-exact element-wise ops); everything is finite.  An f16 store of a COMPUTED value (a GEMM result rounded into a
cache) is compared at its site's bar, as its own test does (test_round4_gpu.py:553).  The flip tests run control three times and then submit the same node array with the
outside reader present in the counts, then with the OUTPUT flag: the capture must not be replayed (graph.cpp recs_match on `ext` and `flags`).

Sites covered, by the line of their guard -- graph_exec.cpp compute_node: UNARY f16 image (:668), GLU f16 image and swiglu_q8k (:684), SOFT_MAX f16 image (:730),
CONT(PERMUTE) into the image (:766); run_nodes: cont_sink (:1067 / graph_exec_t2w.cpp:218), exec_ew_chain (graph_exec_t2w.cpp:317); graph_exec_llm.cpp: gate / up + SWIGLU
in the GEMM epilogue (:99), residual ADD in the epilogue (:69, :187) with the f16 CPY (:199) and with the UNARY behind it (:135), grouped split-K left to the norm / rope
launch (:269), the any-shape GEMM's bias / GELU epilogue and siblings (:317-362), gemm_only_consumers / exec_norm (:584, :626, :640), attention slices folded into wo and
the Q8_K image of the attention rows (:844, :858), exec_rms_norm's chains and deferred norms (:1117, :1161, :1204), the soft-max attention of a batch (:1261-1276),
try_alias_vt (:1364-1388).  Two sites write their f32 rows whatever the guard says -- swiglu_q8k (graph_exec.cpp:704) and the attention launch that adds wo's Q8_K image
(:858-870: the image is one more output of the kernel) -- so they have control and output only: a split of them cannot fail, as a build whose `external` stays empty
confirms (every other split, view, crowded and flip case fails under it).  The same holds for the residual ADD in front of the RMS_NORM that sums its split-K slabs: the
norm launch writes the ADD's rows itself, so only the mat-mul in front of it is observed there.

The encoder / Token2Wav side, by the line of its guard -- graph_exec_t2w.cpp: exec_attn_f32 (:107 K.Q, :117 SCALE, :123 SOFT_MAX, :146 the second product, :155 the views in front
of the CONT), match_norm_modulate for exec_norm_modulate and behind exec_gate_norm (:13 NORM, :24 MUL, :25 the first ADD), exec_gate_norm's gate MUL (:57), exec_causal_conv
(:557, :606, :619, :620), exec_concat_tail (:676, :681, :689), exec_conv1d_tc (:730, :744, :749, :765, :772, :776, :781), lazy_try_register (:397, :409: cases A / B in front
of the causal convolution, C / C' in front of the attention chain; an observed copy is never registered, so lazy_net / the matchers' erasing of a record cannot lose it), and
graph_exec.cpp copy_prune (:867: a forwarded copy nobody reads any more is never launched).  For the lazy sites the observed run must also leave fewer copies un-run than the
control (lazy_conts) and launch more kernels or count a materialisation.  Every protocol starts with the backend's captures dropped (_fresh): a Run's node records and device
addresses repeat those of the test before it.  exec_gate_norm writes x = resid + y * gate in every case (it is the norm launch's second output): output only.  exec_concat_tail
compares nb[2] of the tail VIEW with the copy's, which a 2-D view never meets: its site has a batch dimension, and the concat_tails counter, not the launch count (the copy
queue's with or without the matcher), proves its control.  Against a build whose `external` stays empty every new split, view, crowded and flip case fails by assertion (the
interior node keeps its NaNs, or the bytes of the other layout), with nothing that cannot fail but gate_norm / x; every guard named here was found in place on the device.
"""
import numpy as np
import pytest

from conftest import nmse
from graph_views import crowd
from test_exec_state_gpu import _pad

pytestmark = pytest.mark.gpu

OUTPUT = 2                                                              # GGML_TENSOR_FLAG_OUTPUT (ggml.h)
N_SETS = 3


class Case:
    """one site's graph on one backend: c (Context), obs {name: (interior Tensor, bar)}, outs [(Tensor, bar)], set(k) writes input set k, order = the nodes to submit"""

    def __init__(self, c, obs, outs, set_, order=None, close=None, alloc=None, f64=None):
        self.c, self.obs, self.outs, self.set, self.order, self._close = c, obs, outs, set_, list(c.nodes if order is None else order), close
        self.alloc = alloc or {}                                        # keyword arguments of Context.alloc (usage=WEIGHTS: the sites that keep a resident kernel image)
        self.f64 = f64                                                  # f64(k) -> the outputs of input set k restated in float64 (None: not restated), bar F64_BAR

    def close(self):
        self.c.free()
        if self._close:
            self._close()


def _simple(pkg, backend, build, feeds, alloc=None, once=(), f64=None):
    """once: inputs written by the first set() only, from set 0 (a convolution kernel: writing it again drops its resident image, and no image is made inside a capture)"""
    c = pkg.Context(backend)
    ins, obs, outs = build(c)
    sets = [feeds(np.random.default_rng(seed)) for seed in (11, 12, 13)]
    first = [True]

    def set_(k):
        for name, T in ins.items():
            if name in once:
                if first[0]:
                    backend.tensor_set(T, sets[0][name])
            else:
                backend.tensor_set(T, sets[k % N_SETS][name])
        first[0] = False
    return Case(c, obs, outs, set_, alloc=alloc, f64=(lambda k: f64(dict(sets[k % N_SETS], **{n: sets[0][n] for n in once}))) if f64 else None)


def _get(backend, T):
    return backend.tensor_get(T).copy()


def _poison(pkg, backend, T):
    dt = pkg.type_traits(T.type)[2]
    if T.t.view_src or dt not in (np.float32, np.float16):
        return
    backend.tensor_set(T, np.full(T.nbytes() // np.dtype(dt).itemsize, np.nan, dt))


def _cmp(a, b, bar, what):
    if bar == 0:
        assert a.tobytes() == b.tobytes(), (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()))
        return
    a, b = a.astype(np.float32), b.astype(np.float32)
    assert np.isfinite(a).all(), (what, "not finite", int((~np.isfinite(a)).sum()))
    e = nmse(a, b)
    _WORST[0] = max(_WORST[0], (e / bar, e, bar))
    assert e < bar, (what, e, bar)


_WORST = [(0.0, 0.0, 0.0)]                                              # (the comparison closest to its bar since _three_runs last reset it: printed, never asserted)
F64_BAR = 1e-10                                                         # a float64 restatement beside the reference backend (test_round5_gpu.py:336)


_REF = {}


def _reference(pkg, ref_be, name):
    """the reference CPU backend on the site's graph, once per site and shared: every interior node and every output, for the three input sets"""
    if name not in _REF:
        case = SITES[name][0](pkg, ref_be)
        c = case.c
        if c.buffer:
            c.free()
        c.alloc(**case.alloc)
        g = c.graph(case.order)
        runs = []
        for k in range(N_SETS):
            case.set(k)
            ref_be.graph_compute(g)
            runs.append(({n: _get(ref_be, T) for n, (T, _) in case.obs.items()}, [_get(ref_be, T) for T, _ in case.outs]))
        case.close()
        _REF[name] = runs
    return _REF[name]


class Run:
    """the site's graph on the MI355X backend in one variant; submit(k) = poison, input set k, one graph_compute per split, read back"""

    def __init__(self, pkg, be, name, key=None, variant="control", crowded=False):
        F32, F16 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16
        self.pkg, self.be, self.name, self.key, self.variant = pkg, be, name, key, variant
        self.case = case = SITES[name][0](pkg, be)
        c = case.c
        self.t, self.bar = case.obs[key] if key else (None, None)
        self.p, _ = _pad(c, pkg)
        nodes = case.order + c.nodes[-8:]
        behind, self.reader = [], None
        if variant.startswith("split"):
            src = self.t
            if variant != "split":                                      # the outside reader sees the interior node through a view node only
                src = c.reshape(self.t, self.t.nelements())
                (nodes if variant == "split_view_front" else behind).append(src)
            self.reader = c.cpy(src, c.new_tensor(F32, *src.ne)) if self.t.type == F16 else c.scale(src, 1.0)
            behind.append(self.reader)
        self.cut = len(nodes)
        self.nodes = nodes + behind
        if c.buffer:
            c.free()
        c.alloc(**case.alloc)
        self.graphs = {}
        self.spares = None
        if crowded:
            self.spares, self.size = crowd(pkg, c, self.nodes, self.t)
        if variant == "output":
            self.t.t.flags |= OUTPUT
        self.observed = variant != "control"

    def graph(self, with_reader):
        """the split(s) to submit: view(0, cut) of the parent over the first `cut` nodes alone (no outside reader in the counts) or over all nodes, then view(cut, n)"""
        if with_reader not in self.graphs:
            c = self.case.c
            nodes = self.nodes if with_reader else self.nodes[:self.cut]
            parent = c.graph_parent(nodes, size=self.size, leafs=self.spares) if self.spares else c.graph_parent(nodes)
            self.graphs[with_reader] = (parent, [parent.view(0, self.cut)] + ([parent.view(self.cut, len(nodes))] if len(nodes) > self.cut else []))
        return self.graphs[with_reader]

    def submit(self, k, with_reader=None, observed=None):
        pkg, be, case = self.pkg, self.be, self.case
        with_reader = (self.reader is not None) if with_reader is None else with_reader
        observed = self.observed if observed is None else observed
        _, graphs = self.graph(with_reader)
        case.set(k)
        be.tensor_set(self.p, np.ones(64, np.float32))
        for T in ([self.t] if self.t is not None else []) + [T for T, _ in case.outs]:
            _poison(pkg, be, T)
        if self.reader is not None:                                     # (the CPY's result is a view of its f32 destination leaf)
            _poison(pkg, be, self.reader._srcs[1] if self.reader.t.view_src else self.reader)
        self.kernels = None
        for g in graphs:
            be.graph_compute(g)
            if self.kernels is None:
                self.kernels = be.get_stat("kernels_last_graph")
        got = dict(outs=[_get(be, T) for T, _ in case.outs])
        if observed:
            got["obs"] = _get(be, self.t)
        if with_reader and self.reader is not None:
            got["reader"] = _get(be, self.reader)
        return got

    def check(self, got, ref_run, what):
        obs_ref, outs_ref = ref_run
        for i, ((_, bar), a, b) in enumerate(zip(self.case.outs, got["outs"], outs_ref)):
            _cmp(a, b, bar, (what, "output", i))
        if "obs" in got:
            _cmp(got["obs"], obs_ref[self.key], self.bar, (what, "interior node", self.key))
        if "reader" in got:                                             # SCALE(t, 1) / the f16 -> f32 CPY of t: the reference's t, exactly representable in f32
            want = obs_ref[self.key].astype(np.float32)
            _cmp(got["reader"].astype(np.float32), want, self.bar, (what, "outside reader of", self.key))

    def close(self):
        if self.t is not None:
            self.t.t.flags &= ~OUTPUT
        self.case.close()


def _fresh(be):
    """every capture the backend holds is dropped (set_option does that): a run's first submission is eager, not the capture or the replay of an equal-looking graph of the
    test before it -- node records and device addresses repeat from one Run to the next, and a capture cannot make a resident kernel image"""
    be.set_option("fusion", 1)


def _three_runs(pkg, be, ref_be, name, key, variant, crowded=False):
    ref = _reference(pkg, ref_be, name)
    _fresh(be)
    run = Run(pkg, be, name, key, variant, crowded)
    try:
        r0 = be.get_stat("graph_replays")
        k_first = None
        _WORST[0] = (0.0, 0.0, 0.0)
        before = {s: be.get_stat(s) for s in LAZY_STATS}
        for k, what in enumerate(("eager run", "captured run", "replayed run")):
            got = run.submit(k)
            if k == 0:
                k_first = run.kernels
                run.moved = {s: be.get_stat(s) - before[s] for s in LAZY_STATS}       # (of the eager run alone: a replay walks no nodes)
            run.check(got, ref[k], (name, variant, what))
            if run.case.f64:
                for i, (a, want) in enumerate(zip(got["outs"], run.case.f64(k))):
                    _cmp(a, want.reshape(a.shape), F64_BAR, ((name, variant, what), "output against float64", i))
        assert be.get_stat("graph_replays") - r0 >= 1, "the graph did not replay"
        print(f"{name}/{key}/{variant}: closest to its bar NMSE {_WORST[0][1]:.2e} (bar {_WORST[0][2]:g})" if _WORST[0][2] else f"{name}/{key}/{variant}: bit-exact")
        return run, k_first
    except BaseException:
        run.close()
        raise


LAZY_STATS = ("lazy_conts", "lazy_conts_materialised")


# ================================================================================================ the sites
def _types(pkg):
    return pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16


# ---- graph_exec.cpp compute_node :668 -- fc1 -> GELU -> fc2: the unary op writes fc2's f16 image and no f32 rows.  Bar 1e-10 (test_prefill_kernels_gpu.py:309).
def site_unary_f16(pkg, backend):
    from llama_cpp_omni_amd.ggml import UNARY
    F32, F16 = _types(pkg)
    n, rows, M = 512, 100, 192

    def build(c):
        x, w = c.new_tensor(F32, n, rows), c.new_tensor(F16, n, M)
        y = c.unary(x, UNARY.GELU)
        return dict(x=x, w=w), dict(unary=(y, 1e-10)), [(c.mul_mat(w, y), 1e-10)]

    def feeds(rng):
        return dict(x=(rng.standard_normal((rows, n)) * 1.5).astype(np.float32), w=(rng.standard_normal((M, n)) / np.sqrt(n)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- compute_node :684 -- SWIGLU(gate, up) -> ffn_down on the MFMA GEMM: the GLU writes the f16 image, the f32 rows only for a second reader.  Bar 1e-6 (test_round2_gpu.py:578).
def site_glu_f16(pkg, backend):
    F32, F16 = _types(pkg)
    F_, N, E = 512, 100, 192

    def build(c):
        gate, up, wd = c.new_tensor(F32, F_, N), c.new_tensor(F32, F_, N), c.new_tensor(F16, F_, E)
        g = c.swiglu_split(gate, up)
        return dict(gate=gate, up=up, wd=wd), dict(glu=(g, 1e-6)), [(c.mul_mat(wd, g), 1e-6)]

    def feeds(rng):
        return dict(gate=rng.standard_normal((N, F_)).astype(np.float32), up=rng.standard_normal((N, F_)).astype(np.float32),
                    wd=(rng.standard_normal((E, F_)) / np.sqrt(F_)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- compute_node :690 -- SWIGLU -> a K-quant ffn_down at <= 8 columns: swiglu_q8k writes the Q8_K image (and the f32 rows).  Bar 5e-4, the reference's MUL_MAT bar
# (test_exec_state_gpu.py:239).
def site_swiglu_q8k(pkg, backend):
    from llama_cpp_omni_amd.qwen3 import random_blocks
    F32 = pkg.GGML_TYPE_F32
    F_, N, E = 512, 4, 256

    def build(c):
        gate, up, wd = c.new_tensor(F32, F_, N), c.new_tensor(F32, F_, N), c.new_tensor(pkg.GGML_TYPE_Q4_K, F_, E)
        g = c.swiglu_split(gate, up)
        return dict(gate=gate, up=up, wd=wd), dict(glu=(g, 5e-4)), [(c.mul_mat(wd, g), 5e-4)]

    def feeds(rng):
        return dict(gate=rng.standard_normal((N, F_)).astype(np.float32), up=rng.standard_normal((N, F_)).astype(np.float32), wd=random_blocks(rng, pkg.GGML_TYPE_Q4_K, E, F_, 0.05))
    return _simple(pkg, backend, build, feeds)


# ---- compute_node :730 -- SOFT_MAX -> V^T . P per head: the probabilities exist only as the GEMM's f16 image.  Bars 1e-12 / 1e-6 (test_prefill_kernels_gpu.py:95-96).
def site_soft_max_f16(pkg, backend):
    F32, F16 = _types(pkg)
    n, T, H, D = 256, 96, 2, 64

    def build(c):
        x, m, vt = c.new_tensor(F32, n, T, H), c.new_tensor(F16, n, T), c.new_tensor(F16, n, D, H)
        p = c.soft_max_ext(x, m, 0.125, 0.0)
        return dict(x=x, m=m, vt=vt), dict(soft_max=(p, 1e-12)), [(c.mul_mat(vt, p), 1e-6)]

    def feeds(rng):
        mask = np.zeros((T, n), np.float16)
        for t in range(T):
            mask[t, 1 + (t * 7) % n:] = -np.inf
        return dict(x=(rng.standard_normal((H, T, n)) * 4).astype(np.float32), m=mask, vt=rng.standard_normal((H, D, n)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- compute_node :766 -- CONT(PERMUTE(kqv)) -> wo: gathered straight into wo's f16 image, the f32 copy is never written.  The copy is bit-exact; wo's bar 1e-10 is that
# of a GEMM on an emitted f16 image (test_prefill_kernels_gpu.py:309).
def site_cont_permute(pkg, backend):
    F32, F16 = _types(pkg)
    D, nq, H, E = 64, 100, 4, 192

    def build(c):
        kqv, wo = c.new_tensor(F32, D, nq, H), c.new_tensor(F16, D * H, E)
        cc = c.cont(c.permute(kqv, 0, 2, 1, 3), D * H, nq)
        return dict(kqv=kqv, wo=wo), dict(cont=(cc, 0)), [(c.mul_mat(wo, cc), 1e-10)]

    def feeds(rng):
        return dict(kqv=rng.standard_normal((H, nq, D)).astype(np.float32), wo=(rng.standard_normal((E, D * H)) / np.sqrt(D * H)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- run_nodes :1067 (cont_sink, graph_exec_t2w.cpp:218) -- ADD -> CONT: the producer writes into the copy's buffer, its own bytes are never written.  IEEE-exact: bit-exact.
def site_cont_sink(pkg, backend):
    F32 = pkg.GGML_TYPE_F32

    def build(c):
        x, y = c.new_tensor(F32, 512, 56), c.new_tensor(F32, 512, 56)
        p = c.add(x, y)
        return dict(x=x, y=y), dict(producer=(p, 0)), [(c.cont(p), 0)]

    def feeds(rng):
        return dict(x=rng.standard_normal((56, 512)).astype(np.float32), y=rng.standard_normal((56, 512)).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- run_nodes exec_ew_chain (graph_exec_t2w.cpp:317) -- ADD -> MUL -> ADD as one launch; the middle node is never written.  Bit-exact (test_round3_gpu.py:548).
def site_ew_chain(pkg, backend):
    F32 = pkg.GGML_TYPE_F32

    def build(c):
        x, y, z, w = (c.new_tensor(F32, 512, 56) for _ in range(4))
        a = c.add(x, y)
        m = c.mul(a, z)
        return dict(x=x, y=y, z=z, w=w), dict(first=(a, 0), middle=(m, 0)), [(c.add(m, w), 0)]

    def feeds(rng):
        return {k: rng.standard_normal((56, 512)).astype(np.float32) for k in "xyzw"}
    return _simple(pkg, backend, build, feeds)


# ---- graph_exec_llm.cpp :99 -- ffn_up / ffn_gate -> SWIGLU -> ffn_down of a prefill ubatch: one GEMM launch whose epilogue writes ffn_down's f16 image; gate, up and the GLU
# result are never written.  4096 x 1024: the smallest grid gemm_glu_ok takes (128 row blocks x column tiles).  Bar 1e-6 (test_round2_gpu.py:578).
def site_gate_up_swiglu(pkg, backend):
    F32, F16 = _types(pkg)
    E, F_, N = 128, 4096, 1024

    def build(c):
        x = c.new_tensor(F32, E, N)
        tg, tu, td = c.new_tensor(F16, E, F_), c.new_tensor(F16, E, F_), c.new_tensor(F16, F_, E)
        up, gate = c.mul_mat(tu, x), c.mul_mat(tg, x)
        act = c.swiglu_split(gate, up)
        return dict(x=x, tg=tg, tu=tu, td=td), dict(gate=(gate, 1e-6), up=(up, 1e-6), glu=(act, 1e-6)), [(c.mul_mat(td, act), 1e-6)]

    def feeds(rng):
        return dict(x=rng.standard_normal((N, E)).astype(np.float32), tg=(rng.standard_normal((F_, E)) * 0.05).astype(np.float16),
                    tu=(rng.standard_normal((F_, E)) * 0.05).astype(np.float16), td=(rng.standard_normal((E, F_)) * 0.05).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- :69 / :249 -- a lone prefill GEMM + residual ADD in the epilogue (the mat-mul's own rows are never written), its split-K slabs left to the RMS_NORM behind it.  Bar 5e-4,
# the reference's MUL_MAT bar (test_exec_state_gpu.py:299).
def site_gemm_resid_norm(pkg, backend):
    F32, F16 = _types(pkg)
    K, M, N = 2048, 256, 64

    def build(c):
        x, r, w, nw = c.new_tensor(F32, K, N), c.new_tensor(F32, M, N), c.new_tensor(F16, K, M), c.new_tensor(F32, M)
        mm = c.mul_mat(w, x)
        a = c.add(mm, r)
        return dict(x=x, r=r, w=w, nw=nw), dict(mul_mat=(mm, 5e-4)), [(c.mul(c.rms_norm(a, 1e-6), nw), 5e-4)]

    def feeds(rng):
        return dict(x=rng.standard_normal((N, K)).astype(np.float32), r=rng.standard_normal((N, M)).astype(np.float32),
                    w=(rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float16), nw=rng.uniform(0.5, 1.5, M).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- :135 -- fc1 + bias -> GELU -> fc2 on a streaming chunk: the split-K reduction adds the bias, applies the GELU and writes fc2's f16 image; neither the mat-mul's, the ADD's
# nor (fc2 being the next launch) the GELU's f32 rows are written.  Bar 1e-9 (test_round4_gpu.py:499).
def site_gemm_bias_gelu(pkg, backend):
    from llama_cpp_omni_amd.ggml import UNARY
    F32, F16 = _types(pkg)
    E, F_, N, E2 = 1024, 512, 50, 256

    def build(c):
        y, W1, b1, W2 = c.new_tensor(F32, E, N), c.new_tensor(F16, E, F_), c.new_tensor(F32, F_), c.new_tensor(F16, F_, E2)
        mm = c.mul_mat(W1, y)
        pre = c.add(mm, b1)
        u = c.unary(pre, UNARY.GELU)
        return dict(y=y, W1=W1, b1=b1, W2=W2), dict(mul_mat=(mm, 1e-9), add=(pre, 1e-9), gelu=(u, 1e-9)), [(c.mul_mat(W2, u), 1e-9)]

    def feeds(rng):
        return dict(y=rng.standard_normal((N, E)).astype(np.float32), W1=(rng.standard_normal((F_, E)) / np.sqrt(E) * 2).astype(np.float16),
                    b1=(0.2 * rng.standard_normal(F_)).astype(np.float32), W2=(rng.standard_normal((E2, F_)) / np.sqrt(F_)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- :187 / :199 / :1364-1388 -- one attention block of the streaming Whisper graph, chunk 1 (test_round4_gpu.py:504): the K rows and the V rows (+ bias) exist only as the f16
# cells the q / k / v reduction writes into the caches; CONT(TRANSPOSE(V cache window)) and the CAST behind it are never made, the fused attention reads V^T in the cache.  Bar
# 2e-6 for everything (test_round4_gpu.py:553) -- the two skipped copies too: the window they copy holds the cells this very graph stores, f16 roundings of a GEMM result.
def site_stream_encoder(pkg, backend):
    F32, F16 = _types(pkg)
    E, H, D, it, n_tok, kv_size = 1024, 16, 64, 1, 50, 200
    tot = (it + 1) * n_tok

    def build(c):
        x, res = c.new_tensor(F32, E, n_tok), c.new_tensor(F32, E, n_tok)
        W = {k: c.new_tensor(F16, E, E) for k in ("q", "k", "v", "o")}
        B = {k: c.new_tensor(F32, E) for k in ("q", "v", "o", "lw", "lb")}
        kc, vc = c.new_tensor(F16, E * kv_size), c.new_tensor(F16, E * kv_size)
        Q = c.reshape(c.add(c.mul_mat(W["q"], x), B["q"]), D, H, n_tok)
        k_rows = c.mul_mat(W["k"], x)
        Kc = c.reshape(k_rows, D, H, n_tok)
        v_rows = c.add(c.mul_mat(W["v"], x), B["v"])
        Vc = c.reshape(v_rows, D, H, n_tok)
        st_k = c.cpy(Kc, c.view_1d(kc, n_tok * E, 2 * E * it * n_tok))
        st_v = c.cpy(c.transpose(c.reshape(Vc, E, n_tok)), c.view_2d(vc, n_tok, E, 2 * kv_size, 2 * it * n_tok))
        K = c.view_3d(kc, D, tot, H, 2 * E, 2 * D, 0)
        V2t = c.cont(c.transpose(c.view_2d(vc, tot, E, 2 * kv_size, 0)))
        V = c.cast(c.permute(c.reshape(V2t, D, H, tot), 1, 2, 0, 3), F16)
        KQ = c.soft_max_ext(c.mul_mat(K, c.permute(Q, 0, 2, 1, 3)), None, 1.0 / 8.0, 0.0)
        att = c.cont(c.permute(c.mul_mat(V, KQ), 0, 2, 1, 3), E, n_tok)
        x1 = c.add(c.add(c.mul_mat(W["o"], att), B["o"]), res)
        y = c.add(c.mul(c.norm(x1, 1e-5), B["lw"]), B["lb"])
        ins = dict(x=x, res=res, kc=kc, vc=vc, **{"W" + k: v for k, v in W.items()}, **{"B" + k: v for k, v in B.items()})
        obs = dict(k_rows=(k_rows, 2e-6), v_rows=(v_rows, 2e-6), v_window_cont=(V2t, 2e-6), v_cast=(V, 2e-6))
        return ins, obs, [(st_k, 2e-6), (st_v, 2e-6), (c.scale(att, 1.0), 2e-6), (y, 2e-6), (c.scale(x1, 1.0), 2e-6)]

    def feeds(rng):
        f = dict(x=rng.standard_normal((n_tok, E)).astype(np.float32), res=rng.standard_normal((n_tok, E)).astype(np.float32),
                 kc=(rng.standard_normal(E * kv_size) * 0.5).astype(np.float16), vc=(rng.standard_normal(E * kv_size) * 0.5).astype(np.float16))
        for k in ("q", "k", "v", "o"):
            f["W" + k] = (rng.standard_normal((E, E)) / np.sqrt(E)).astype(np.float16)
        for k in ("q", "v", "o", "lb"):
            f["B" + k] = (0.1 * rng.standard_normal(E)).astype(np.float32)
        f["Blw"] = (1 + 0.2 * rng.standard_normal(E)).astype(np.float32)
        return f
    return _simple(pkg, backend, build, feeds)


# ---- :269 -- wq / wk / wv of a prefill ubatch as one grouped split-K launch whose slabs the q / k norm + rope + store launch sums itself: the three products' rows are never
# written.  Bar 5e-4, the reference's MUL_MAT bar (test_exec_state_gpu.py:299), for the products and for everything computed from them.
def site_grouped_split_k(pkg, backend):
    F32, F16, I32, I64 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16, pkg.GGML_TYPE_I32, pkg.GGML_TYPE_I64
    E, D, H, HK, T, n_ctx = 2048, 128, 8, 4, 64, 128                    # (k_norm_rope_v4 sums slabs for head counts that are multiples of 4)
    rope = dict(n_dims=D, mode=2, n_ctx_orig=40960, freq_base=1e6, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0)

    def build(c):
        x = c.new_tensor(F32, E, T)
        wq, wk, wv = c.new_tensor(F16, E, H * D), c.new_tensor(F16, E, HK * D), c.new_tensor(F16, E, HK * D)
        qw, kw, pos, idx = c.new_tensor(F32, D), c.new_tensor(F32, D), c.new_tensor(I32, T), c.new_tensor(I64, T)
        kc, vc = c.new_tensor(F16, HK * D, n_ctx), c.new_tensor(F16, HK * D, n_ctx)
        q, k, v = c.mul_mat(wq, x), c.mul_mat(wk, x), c.mul_mat(wv, x)
        q3, k3, v3 = c.reshape(q, D, H, T), c.reshape(k, D, HK, T), c.reshape(v, D, HK, T)
        Q = c.rope_ext(c.mul(c.rms_norm(q3, 1e-6), qw), pos, None, **rope)
        K = c.rope_ext(c.mul(c.rms_norm(k3, 1e-6), kw), pos, None, **rope)
        ks = c.set_rows(kc, c.view_2d(K, HK * D, T, K.nb[2], 0), idx)
        vs = c.set_rows(vc, c.view_2d(v3, HK * D, T, v3.nb[2], 0), idx)
        ins = dict(x=x, wq=wq, wk=wk, wv=wv, qw=qw, kw=kw, pos=pos, idx=idx, kc=kc, vc=vc)
        return ins, dict(q=(q, 5e-4), k=(k, 5e-4), v=(v, 5e-4)), [(Q, 5e-4), (ks, 5e-4), (vs, 5e-4)]

    def feeds(rng):
        w = lambda m: (rng.standard_normal((m, E)) / np.sqrt(E)).astype(np.float16)
        return dict(x=rng.standard_normal((T, E)).astype(np.float32), wq=w(H * D), wk=w(HK * D), wv=w(HK * D), qw=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
                    kw=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32), pos=(np.arange(T) * 3 + 5).astype(np.int32), idx=rng.permutation(n_ctx)[:T].astype(np.int64),
                    kc=np.zeros((n_ctx, HK * D), np.float16), vc=np.zeros((n_ctx, HK * D), np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- :317 / :362 -- an F32-weight linear layer: MUL_MAT -> ADD(bias) -> GELU in the any-shape GEMM's epilogue; neither the product nor the biased rows are written.  Bars 1e-10
# (test_prefill_kernels_gpu.py:331), 1e-9 behind the GELU's f16 tables (test_round4_gpu.py:499).
def site_gemm_any_bias_gelu(pkg, backend):
    from llama_cpp_omni_amd.ggml import UNARY
    F32 = pkg.GGML_TYPE_F32
    M, N, K = 80, 120, 1000

    def build(c):
        w, x, b = c.new_tensor(F32, K, M), c.new_tensor(F32, K, N), c.new_tensor(F32, M)
        mm = c.mul_mat(w, x)
        a = c.add(mm, b)
        return dict(w=w, x=x, b=b), dict(mul_mat=(mm, 1e-10), add=(a, 1e-10)), [(c.unary(a, UNARY.GELU), 1e-9)]

    def feeds(rng):
        return dict(w=(rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32), x=rng.standard_normal((N, K)).astype(np.float32), b=rng.standard_normal(M).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- :336 -- two F32-weight products of one activation, each with its bias ADD, as one any-shape GEMM launch (the sibling's product is never written).  Bar 1e-10
# (test_prefill_kernels_gpu.py:331).
def site_gemm_any_siblings(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    M, N, K = 80, 120, 1000

    def build(c):
        w, w2, x, b, b2 = c.new_tensor(F32, K, M), c.new_tensor(F32, K, M), c.new_tensor(F32, K, N), c.new_tensor(F32, M), c.new_tensor(F32, M)
        m1 = c.mul_mat(w, x)
        a1 = c.add(m1, b)
        m2 = c.mul_mat(w2, x)
        a2 = c.add(m2, b2)
        return dict(w=w, w2=w2, x=x, b=b, b2=b2), dict(first=(m1, 1e-10), sibling=(m2, 1e-10)), [(a1, 1e-10), (a2, 1e-10)]

    def feeds(rng):
        return dict(w=(rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32), w2=(rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32),
                    x=rng.standard_normal((N, K)).astype(np.float32), b=rng.standard_normal(M).astype(np.float32), b2=rng.standard_normal(M).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- :584 / :626 / :640 -- the encoders' LayerNorm: NORM -> MUL(w) -> ADD(b) as one launch that also writes fc1's f16 image; none of the three f32 results is written.  Bar 1e-10
# (test_prefill_kernels_gpu.py:261).
def site_layer_norm(pkg, backend):
    F32, F16 = _types(pkg)
    n, rows, M = 1024, 100, 256

    def build(c):
        x, w, b, W = c.new_tensor(F32, n, rows), c.new_tensor(F32, n), c.new_tensor(F32, n), c.new_tensor(F16, n, M)
        nn = c.norm(x, 1e-5)
        m = c.mul(nn, w)
        y = c.add(m, b)
        return dict(x=x, w=w, b=b, W=W), dict(norm=(nn, 1e-10), mul=(m, 1e-10), add=(y, 1e-10)), [(c.mul_mat(W, y), 1e-10)]

    def feeds(rng):
        return dict(x=(rng.standard_normal((rows, n)) * 2 + 0.3).astype(np.float32), w=(1 + 0.2 * rng.standard_normal(n)).astype(np.float32),
                    b=(0.1 * rng.standard_normal(n)).astype(np.float32), W=(rng.standard_normal((M, n)) / np.sqrt(n)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- :1117 -- flash-attention off, prefill: RMS_NORM -> MUL -> ROPE whose rows only the per-head K . q GEMM reads: the launch writes that GEMM's f16 image, neither the MUL
# nor the ROPE result exists in f32.  Bars 1e-10 / 1e-6 (test_prefill_kernels_gpu.py:157-158).
def site_rope_chain_f16(pkg, backend):
    F32, F16, I32 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16, pkg.GGML_TYPE_I32
    D, H, HK, T, nkv, n_ctx = 128, 4, 4, 64, 64, 64
    rope = dict(n_dims=D, mode=2, n_ctx_orig=40960, freq_base=1e6, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0)

    def build(c):
        q, qw, pos, kc = c.new_tensor(F32, D, H, T), c.new_tensor(F32, D), c.new_tensor(I32, T), c.new_tensor(F16, D * HK, n_ctx)
        m = c.mul(c.rms_norm(q, 1e-6), qw)
        Q = c.rope_ext(m, pos, None, **rope)
        k = c.view_3d(kc, D, nkv, HK, D * HK * 2, D * 2, 0)
        return dict(q=q, qw=qw, pos=pos, kc=kc), dict(mul=(m, 1e-10), rope=(Q, 1e-10)), [(c.mul_mat(k, c.permute(Q, 0, 2, 1, 3)), 1e-6)]

    def feeds(rng):
        return dict(q=rng.standard_normal((T, H, D)).astype(np.float32), qw=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32), pos=(np.arange(T) * 3 + 5).astype(np.int32),
                    kc=rng.standard_normal((n_ctx, D * HK)).astype(np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- exec_rms_norm's norm -> mul -> rope -> set_rows chain (match_norm_rope, rope_store_of): the k chain's MUL and ROPE rows are never written, only the f16 cache rows.  Bars
# 1e-10 rope rows, 1e-6 f16 cache rows, bit-exact v store (test_prefill_kernels_gpu.py:157-159).
def site_rope_chain_store(pkg, backend):
    F32, F16, I32, I64 = pkg.GGML_TYPE_F32, pkg.GGML_TYPE_F16, pkg.GGML_TYPE_I32, pkg.GGML_TYPE_I64
    D, T, H, HK, n_ctx = 128, 19, 8, 4, 64
    rope = dict(n_dims=D, mode=2, n_ctx_orig=40960, freq_base=1e6, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0)

    def build(c):
        q, k, v = c.new_tensor(F32, D, H, T), c.new_tensor(F32, D, HK, T), c.new_tensor(F32, D, HK, T)
        qw, kw, pos, idx = c.new_tensor(F32, D), c.new_tensor(F32, D), c.new_tensor(I32, T), c.new_tensor(I64, T)
        kc, vc = c.new_tensor(F16, HK * D, n_ctx), c.new_tensor(F16, HK * D, n_ctx)
        Q = c.rope_ext(c.mul(c.rms_norm(q, 1e-6), qw), pos, None, **rope)
        km = c.mul(c.rms_norm(k, 1e-6), kw)
        K = c.rope_ext(km, pos, None, **rope)
        ks = c.set_rows(kc, c.view_2d(K, HK * D, T, K.nb[2], 0), idx)
        vs = c.set_rows(vc, c.view_2d(v, HK * D, T, v.nb[2], 0), idx)
        return dict(q=q, k=k, v=v, qw=qw, kw=kw, pos=pos, idx=idx, kc=kc, vc=vc), dict(k_mul=(km, 1e-10), k_rope=(K, 1e-10)), [(Q, 1e-10), (ks, 1e-6), (vs, 0)]

    def feeds(rng):
        return dict(q=rng.standard_normal((T, H, D)).astype(np.float32), k=rng.standard_normal((T, HK, D)).astype(np.float32), v=rng.standard_normal((T, HK, D)).astype(np.float32),
                    qw=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32), kw=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
                    pos=(np.arange(T) * 3 + 5).astype(np.int32), idx=rng.permutation(n_ctx)[:T].astype(np.int64),
                    kc=np.zeros((n_ctx, HK * D), np.float16), vc=np.zeros((n_ctx, HK * D), np.float16))
    return _simple(pkg, backend, build, feeds)


# ---- :1161 / :1204 -- RMS_NORM -> MUL(w) read by batch-1 mat-vecs only: the norm is deferred into their prologues, its rows are never written.  Q8_0 consumers (mmv1q) and Q4_K
# consumers (mmv1 / the LDS-DMA engine).  Bar 5e-4, the reference's MUL_MAT bar (test_exec_state_gpu.py:270).
def _site_deferred_norm(wname):
    def site(pkg, backend):
        from llama_cpp_omni_amd.qwen3 import random_blocks
        F32 = pkg.GGML_TYPE_F32
        WT = dict(q8_0=pkg.GGML_TYPE_Q8_0, q4_K=pkg.GGML_TYPE_Q4_K)[wname]
        K, M = 1024, 512

        def build(c):
            x, w, wa, wb = c.new_tensor(F32, K), c.new_tensor(F32, K), c.new_tensor(WT, K, M), c.new_tensor(WT, K, M)
            nn = c.rms_norm(x, 1e-6)
            h = c.mul(nn, w)
            return dict(x=x, w=w, wa=wa, wb=wb), dict(norm=(nn, 5e-4), mul=(h, 5e-4)), [(c.mul_mat(wa, h), 5e-4), (c.mul_mat(wb, h), 5e-4)]

        def feeds(rng):
            return dict(x=rng.standard_normal(K).astype(np.float32), w=rng.uniform(0.5, 1.5, K).astype(np.float32), wa=random_blocks(rng, WT, M, K, 0.05),
                        wb=random_blocks(rng, WT, M, K, 0.05))
        return _simple(pkg, backend, build, feeds)
    return site


# ---- :1261-1276 -- flash-attention off, a batch of query rows: K . q -> SOFT_MAX -> V^T . p -> PERMUTE -> CONT as one flash-attention launch; M1, SM and M2 are never written.
# Bar 2e-6 (test_round4_gpu.py:316).
def site_attn_sm_batch(pkg, backend):
    F32, F16 = _types(pkg)
    D, nq, H, HK, nkv, n_ctx = 128, 40, 4, 2, 96, 128
    nq_pad = (nq + 31) // 32 * 32

    def build(c):
        qc, kc, vc, m = c.new_tensor(F32, D, H, nq), c.new_tensor(F16, D * HK, n_ctx), c.new_tensor(F16, n_ctx, D * HK), c.new_tensor(F16, nkv, nq_pad)
        q = c.permute(qc, 0, 2, 1, 3)
        k = c.view_3d(kc, D, nkv, HK, D * HK * 2, D * 2, 0)
        v = c.view_3d(vc, nkv, D, HK, n_ctx * 2, n_ctx * 2 * D, 0)
        kq = c.mul_mat(k, q)
        p = c.soft_max_ext(kq, m, 1.0 / np.sqrt(D), 0.0)
        kqv = c.mul_mat(v, p)
        out = c.cont(c.permute(kqv, 0, 2, 1, 3), D * H, nq)
        return dict(q=qc, k=kc, v=vc, m=m), dict(kq=(kq, 2e-6), soft_max=(p, 2e-6), kqv=(kqv, 2e-6)), [(out, 2e-6)]

    def feeds(rng):
        mv = np.zeros((nq_pad, nkv), np.float16)
        for i in range(nq_pad):
            mv[i, max(1, min(nkv, nkv - nq + min(i, nq - 1) + 1)):] = -np.inf
        return dict(q=rng.standard_normal((nq, H, D)).astype(np.float32), k=rng.standard_normal((n_ctx, D * HK)).astype(np.float16),
                    v=rng.standard_normal((D * HK, n_ctx)).astype(np.float16), m=mv)
    return _simple(pkg, backend, build, feeds)


# ---- :844 / :858 -- one decoder layer at Qwen3-8B's attention widths (what fattn_gs_ok asks for: head size 128, four query heads per KV head) through qwen3.Model.  One
# token: the attention is left as slices' partial states that wo's launch folds (the attention rows are never written); four tokens: the attention launch writes wo's Q8_K
# image.  Bars: the attention rows 5e-4, the reference's FLASH_ATTN_EXT bar (test_exec_state_gpu.py:183); the logits behind Q4_K layers 2e-3 (test_round6_gpu.py:85).
_DEC_CFG = dict(n_embd=4096, n_layer=1, n_head=32, n_head_kv=8, head_dim=128, n_ff=1024, n_vocab=512, rms_eps=1e-6, rope_base=1e6, n_ctx_orig=4096)


def _site_decoder(n_tokens):
    def site(pkg, backend):
        from llama_cpp_omni_amd import qwen3
        from llama_cpp_omni_amd.ggml import OP
        n_kv = 128
        mdl = qwen3.Model(backend, _DEC_CFG, qwen3.q4_k_m_types(_DEC_CFG), n_ctx=n_kv, seed=4, flash_attn=True)
        g, I, logits = mdl.build(n_tokens, n_kv)
        order = g.graph().nodes
        fa = [T for T in order if T.t.op == OP.FLASH_ATTN_EXT]
        assert len(fa) == 1
        embd = np.random.default_rng(61).standard_normal((N_SETS, n_tokens, _DEC_CFG["n_embd"])).astype(np.float32)

        def set_(k):                                                    # (the cache fills as a decode fills it: run k writes the cells behind run k - 1's)
            assert k < N_SETS
            mdl.set_inputs(I, embd[k], k * n_tokens, n_kv)
        return Case(g, dict(attention=(fa[0], 5e-4)), [(logits, 2e-3)], set_, order=order, close=mdl.wctx.free)
    return site


# ================================================================================================ the sites of graph_exec_t2w.cpp (encoders / Token2Wav)
# ---- exec_attn_f32 -- K.Q -> SCALE -> SOFT_MAX -> V^T.P -> RESHAPE / PERMUTE -> CONT, all f32, as one attn_f32 launch (guards :107 K.Q, :117 SCALE, :123 SOFT_MAX, :146 the
# second product, :155 the views in front of the CONT).  The smallest row of test_round5_gpu.py:341 with more than 8 query rows (:111), here with the SCALE node.  Bar 1e-10
# (test_round5_gpu.py:382), which is also the any-shape f32 GEMM's (test_prefill_kernels_gpu.py:331) that runs the two products node by node; the soft-max rows are compared at
# the same bar, not at their own 1e-12 (test_prefill_kernels_gpu.py:95): their input is that GEMM's result, as in attn_sm_batch above.
def site_attn_f32(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    D, nq, nkv, H = 64, 17, 36, 3

    def build(c):
        q, k, vt = c.new_tensor(F32, D, nq, H), c.new_tensor(F32, D, nkv, H), c.new_tensor(F32, nkv, D, H)
        kq = c.mul_mat(k, q)
        sc = c.scale(kq, 0.125)
        p = c.soft_max_ext(sc, None, 1.0)
        o = c.mul_mat(vt, p)
        out = c.cont(c.permute(c.reshape(o, D, nq, H, 1), 0, 2, 1, 3))
        return dict(q=q, k=k, vt=vt), dict(kq=(kq, 1e-10), scale=(sc, 1e-10), soft_max=(p, 1e-10), kqv=(o, 1e-10)), [(out, 1e-10)]

    def feeds(rng):
        return dict(q=rng.standard_normal((H, nq, D)).astype(np.float32), k=rng.standard_normal((H, nkv, D)).astype(np.float32), vt=rng.standard_normal((H, D, nkv)).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


def _ada_chunk(c, ada, C_, B, k):
    """chunk k of the adaLN product [9C, 1, B]: a [C, 1, B] strided view, one row per batch element"""
    return c.view_3d(ada, C_, 1, B, ada.nb[1], ada.nb[2], k * C_ * 4)


def _layer_norm64(x, eps=1e-5):
    x = x.astype(np.float64)
    return (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + eps)


# ---- exec_norm_modulate (match_norm_modulate :13 NORM, :24 MUL, :25 the first ADD) -- the DiT's LayerNorm + modulation, norm * scale + norm + shift with [C, 1, B] views, as one
# norm launch.  The modulated rows carry the OUTPUT flag as in their own test (they are read back, and an element-wise chain must end at them); the gate chain behind them is the
# second output.  Bar 1e-12 (test_round5_gpu.py:333).
def site_norm_modulate(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    C_, T, B = 64, 5, 3

    def build(c):
        x, ada = c.new_tensor(F32, C_, T, B), c.new_tensor(F32, 9 * C_, 1, B)
        h = c.norm(x, 1e-5)
        m = c.mul(h, _ada_chunk(c, ada, C_, B, 1))
        a1 = c.add(h, m)
        a2 = c.add(a1, _ada_chunk(c, ada, C_, B, 0))
        a2.t.flags |= OUTPUT
        g = c.add(x, c.mul(a2, _ada_chunk(c, ada, C_, B, 2)))
        return dict(x=x, ada=ada), dict(norm=(h, 1e-12), mul=(m, 1e-12), add1=(a1, 1e-12)), [(a2, 1e-12), (g, 1e-12)]

    def feeds(rng):
        return dict(x=rng.standard_normal((B, T, C_)).astype(np.float32), ada=rng.standard_normal((B, 1, 9 * C_)).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- exec_gate_norm (:57 the gate MUL; the chain behind it through match_norm_modulate :13 / :24 / :25) -- the DiT's gated residual x = resid + y * gate in front of the next
# LayerNorm + modulation: x is computed AND written by the norm launch, so observing x cannot change what is written (output only, as NO_SPLIT's sites).  x has a second reader
# behind the chain.  Bar 1e-12 against the reference backend (test_round5_gpu.py:333) and, this being the matcher's first test of its own, 1e-10 against a float64 restatement
# (test_round5_gpu.py:336).
def site_gate_norm(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    C_, T, B = 64, 5, 2

    def build(c):
        y, r, ada = c.new_tensor(F32, C_, T, B), c.new_tensor(F32, C_, T, B), c.new_tensor(F32, 9 * C_, 1, B)
        gm = c.mul(y, _ada_chunk(c, ada, C_, B, 2))
        x = c.add(r, gm)
        h = c.norm(x, 1e-5)
        m = c.mul(h, _ada_chunk(c, ada, C_, B, 1))
        a1 = c.add(h, m)
        a2 = c.add(a1, _ada_chunk(c, ada, C_, B, 0))
        a2.t.flags |= OUTPUT
        tail = c.add(x, a2)
        obs = dict(gate_mul=(gm, 1e-12), norm=(h, 1e-12), mul=(m, 1e-12), add1=(a1, 1e-12), x=(x, 1e-12))
        return dict(y=y, r=r, ada=ada), obs, [(a2, 1e-12), (tail, 1e-12)]

    def feeds(rng):
        return dict(y=rng.standard_normal((B, T, C_)).astype(np.float32), r=rng.standard_normal((B, T, C_)).astype(np.float32), ada=rng.standard_normal((B, 1, 9 * C_)).astype(np.float32))

    def f64(f):
        ada = f["ada"].astype(np.float64)
        x = f["r"].astype(np.float64) + f["y"].astype(np.float64) * ada[:, :, 2 * C_:3 * C_]
        h = _layer_norm64(x)
        a2 = h * ada[:, :, C_:2 * C_] + h + ada[:, :, :C_]
        return [a2, x + a2]
    return _simple(pkg, backend, build, feeds, f64=f64)


# ---- exec_causal_conv (:557 the CONT of the concatenated frames, :606 the CONT in front of the bias ADD, :619 CONCAT / IM2COL / MUL_MAT / batch CONCAT, :620 the CONT of the
# transposed x) and, with the layers' caches packed (the cache a strided view of a leaf), lazy_try_register cases A / B (:397, :409): cache_in and cache_tcb are not run, the
# concat reads the frames in the cache.  token2wav.causal_conv1d_chunk node for node, as test_round5_gpu.py:239 builds it; the new cache goes through exec_concat_tail.  The kernel
# lies in a WEIGHTS buffer and is written once (its resident rows are made by the eager run).  y is read through the TANH behind the bias ADD.  Bars: 1e-10 for the GEMM and what
# is computed from it (test_round5_gpu.py:287-289; test_prefill_kernels_gpu.py:331 for the product node by node), copies and the IM2COL gather bit-exact (test_round5_gpu.py:288).
def _site_causal_conv(packed):
    def site(pkg, backend):
        from llama_cpp_omni_amd import token2wav as T2
        from llama_cpp_omni_amd.ggml import OP
        F32 = pkg.GGML_TYPE_F32
        C_, Cout, KW, T, B = 64, 96, 3, 7, 2
        P, W = KW - 1, 2 * C_ if packed else C_

        def build(c):
            w, b = c.new_tensor(F32, KW, C_, Cout), c.new_tensor(F32, Cout)
            x_in, pk = c.new_tensor(F32, C_, T, B), c.new_tensor(F32, W, P, B)
            x = c.scale(x_in, 1.0)
            cache = c.view_3d(pk, C_, P, B, pk.nb[1], pk.nb[2], C_ * 4) if packed else pk
            n0 = len(c.nodes)
            y, nc = T2.causal_conv1d_chunk(c, x, cache, w, b)
            act = c.unary(y, pkg.UNARY.TANH)
            of = lambda op: [t for t in c.nodes[n0:] if t.t.op == op]
            conts, cats, ims, mms = of(OP.CONT), of(OP.CONCAT), of(OP.IM2COL), of(OP.MUL_MAT)
            assert (len(conts), len(cats), len(ims), len(mms)) == (8, 3, 2, 2)      # cache_in, cache_tcb, x_tcb, x_cat, y, x_cont, cat, new cache | frames, batch, tail
            if packed:
                obs = dict(cache_in=(conts[0], 0), cache_tcb=(conts[1], 0))
            else:
                obs = dict(x_t=(conts[2], 0), concat=(cats[0], 0), cont=(conts[3], 0), im2col0=(ims[0], 0), mul_mat1=(mms[1], 1e-10), concat_b=(cats[1], 1e-10), cont_back=(conts[4], 1e-10))
            return dict(w=w, b=b, x_in=x_in, pk=pk), obs, [(act, 1e-10), (nc, 0)]

        def feeds(rng):
            return dict(w=(rng.standard_normal((Cout, C_, KW)) / np.sqrt(C_ * KW)).astype(np.float32), b=rng.standard_normal(Cout).astype(np.float32),
                        x_in=rng.standard_normal((B, T, C_)).astype(np.float32), pk=rng.standard_normal((B, P, W)).astype(np.float32))
        return _simple(pkg, backend, build, feeds, alloc=dict(usage=pkg.GGML_BACKEND_BUFFER_USAGE_WEIGHTS), once=("w", "b"))
    return site


# ---- exec_concat_tail (:676 the CONT of x, :681 the CONCAT, :689 its CONT) -- the causal convolution's cache shift as one copy of the kept frames out of x, which is itself the
# output of a copy still queued (test_exec_state_gpu.py:125: its C, P, dt and kept frames).  The matcher compares the VIEW's nb[2] with the copy's (:695), which a 2-D view never
# meets, so the frames carry a batch dimension (two elements) and the tail is a 3-D view, as token2wav.causal_conv1d_chunk spells it.  The launch count is the copy queue's with
# or without the matcher, so the control is proved by the concat_tails counter.  x has a second reader behind the tail: without one cont_sink lets x's copy write into CONT(x)'s
# buffer, the matcher starts at the CONCAT and CONT(x) is written in every case.  Copies and single multiplications: bit-exact.
def site_concat_tail(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    C_, P, dt, keep, B = 64, 3, 8, 3, 2

    def build(c):
        xin, cache = c.new_tensor(F32, dt, C_, B), c.new_tensor(F32, C_, P, B)
        x = c.cont(c.permute(c.scale(xin, 2.0), 1, 0, 2, 3))
        n0 = c.cont(x)
        n1 = c.concat(cache, n0, 1)
        n2 = c.cont(n1)
        n3 = c.cont(c.view_3d(n2, C_, keep, B, n2.t.nb[1], n2.t.nb[2], (P + dt - keep) * n2.t.nb[1]))
        return dict(xin=xin, cache=cache), dict(cont_x=(n0, 0), concat=(n1, 0), cont=(n2, 0)), [(n3, 0), (c.scale(x, 3.0), 0)]

    def feeds(rng):
        return dict(xin=rng.standard_normal((B, C_, dt)).astype(np.float32), cache=rng.standard_normal((B, P, C_)).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- exec_conv1d_tc (:730 IM2COL, :744 its CONT, :749 the kernel's CONT, :765 the product, :772 the bias' CONT, :776 the product's CONT, :781 REPEAT) -- the vocoder's 'same'
# convolution in the reference's spelling, a CONT behind every reshape (test_round5_gpu.py:387, cont=True, its (77, 20, 24, 3, 2) row), as one conv1d_tc launch.  The kernel lies
# in a WEIGHTS buffer and is written once.  Bars: 1e-10 (test_round5_gpu.py:432; test_prefill_kernels_gpu.py:331 for the product node by node); copies, the zero-padded IM2COL
# gather and the REPEAT bit-exact.
def site_conv1d(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    T, Cin, Cout, KW, dil = 77, 20, 24, 3, 2
    pad = (KW - 1) * dil // 2

    def build(c):
        x, w, b = c.new_tensor(F32, T, Cin, 1), c.new_tensor(F32, KW, Cin, Cout), c.new_tensor(F32, Cout)
        col = c.im2col(w, x, 1, 0, pad, 0, dil, 0, False, F32)
        col2 = c.cont(c.reshape(col, col.ne[0], col.ne[2] * col.ne[1]))
        kc = c.cont(c.reshape(w, KW * Cin, Cout))
        mm = c.mul_mat(col2, kc)
        y = c.cont(c.reshape(mm, col.ne[1], Cout, col.ne[2]))
        bc = c.cont(c.reshape(b, 1, Cout, 1))
        rp = c.repeat(bc, y)
        out = c.add(y, rp)
        obs = dict(im2col=(col, 0), col_cont=(col2, 0), kernel_cont=(kc, 0), mul_mat=(mm, 1e-10), prod_cont=(y, 1e-10), bias_cont=(bc, 0), repeat=(rp, 0))
        return dict(x=x, w=w, b=b), obs, [(out, 1e-10)]

    def feeds(rng):
        return dict(x=rng.standard_normal((Cin, T)).astype(np.float32), w=(rng.standard_normal((Cout, Cin, KW)) / np.sqrt(Cin * KW)).astype(np.float32), b=rng.standard_normal(Cout).astype(np.float32))
    return _simple(pkg, backend, build, feeds, alloc=dict(usage=pkg.GGML_BACKEND_BUFFER_USAGE_WEIGHTS), once=("w", "b"))


# ---- lazy_try_register cases C / C' (:397) feeding exec_attn_f32 -- the DiT attention as test_t2w_gpu.py:258 spells it: Q, K, V [D, H, T, B] flattened by CONT(PERMUTE), V
# transposed by a second CONT(PERMUTE); none of the four copies is run, the attention launch reads the permuted views (:138-141, :176) and erases the records (:188-190).  Bars:
# the copies bit-exact, the merged rows 1e-10 (test_t2w_gpu.py:284).
def site_lazy_attn(pkg, backend):
    F32 = pkg.GGML_TYPE_F32
    D, H, B, Tq, Tk = 64, 2, 2, 17, 36

    def build(c):
        q, k, v = c.new_tensor(F32, D, H, Tq, B), c.new_tensor(F32, D, H, Tk, B), c.new_tensor(F32, D, H, Tk, B)

        def flat(t, T):
            cc = c.cont(c.permute(t, 0, 2, 1, 3))
            return cc, c.reshape(cc, D, T, H * B)
        (qc, qf), (kc, kf), (vc, vfl) = flat(q, Tq), flat(k, Tk), flat(v, Tk)
        vt = c.cont(c.permute(vfl, 1, 0, 2, 3))
        vf = c.reshape(vt, Tk, D, H * B)
        probs = c.soft_max_ext(c.scale(c.mul_mat(kf, qf), 1.0 / 8.0), None, 1.0, 0.0)
        ctx = c.mul_mat(vf, probs)
        merged = c.cont(c.permute(c.reshape(ctx, D, Tq, H, B), 0, 2, 1, 3))
        return dict(q=q, k=k, v=v), dict(q_flat=(qc, 0), k_flat=(kc, 0), v_flat=(vc, 0), v_t=(vt, 0)), [(merged, 1e-10)]

    def feeds(rng):
        return dict(q=rng.standard_normal((B, Tq, H, D)).astype(np.float32), k=rng.standard_normal((B, Tk, H, D)).astype(np.float32), v=rng.standard_normal((B, Tk, H, D)).astype(np.float32))
    return _simple(pkg, backend, build, feeds)


# ---- graph_exec.cpp copy_queue / copy_prune (:867) -- Token2Wav's cache packing in small (test_round6_gpu.py:188, f32): a CONCAT that reads exactly a pending copy's output reads
# that copy's sources instead, and a pending copy nobody reads any more is never launched.  p3 = CONT(PERMUTE(x3)) is read by the last CONCAT of the pack alone, pack = the first
# CONCAT of the chain by the second alone: both forwarded and dropped.  The persistent cache is read through the CPY's result (the graph writes only four of its six rows).  Copies,
# a scale by two and a sum of two equal values: bit-exact (test_round6_gpu.py:238-240).
def site_copy_prune(pkg, backend):
    F32 = pkg.GGML_TYPE_F32

    def build(c):
        x = [c.new_tensor(F32, 8, 5, 3) for _ in range(4)]
        cache = c.new_tensor(F32, 8, 5, 3, 6)
        p = [c.cont(c.permute(t, 0, 2, 1, 3)) for t in x]
        pack1 = c.concat(c.reshape(p[0], 8, 3, 5, 1), c.reshape(p[1], 8, 3, 5, 1), 3)
        pack = c.concat(pack1, c.reshape(p[2], 8, 3, 5, 1), 3)
        pack = c.concat(pack, c.reshape(p[3], 8, 3, 5, 1), 3)
        wide2 = c.concat(c.concat(p[0], p[1], 1), p[2], 1)
        flat = c.cont(c.permute(pack, 0, 2, 1, 3))
        stored = c.cpy(flat, c.view_4d(cache, 8, 5, 3, 4, cache.t.nb[1], cache.t.nb[2], cache.t.nb[3], 2 * cache.t.nb[3]))
        outs = [pack, wide2, stored, c.scale(wide2, 2.0), c.add(c.cont(c.permute(wide2, 0, 2, 1, 3)), c.cont(c.permute(wide2, 0, 2, 1, 3)))]
        return dict(cache=cache, **{f"x{i}": t for i, t in enumerate(x)}), dict(p3=(p[3], 0), pack=(pack1, 0)), [(o, 0) for o in outs]

    def feeds(rng):
        return dict(cache=rng.standard_normal((6, 3, 5, 8)).astype(np.float32), **{f"x{i}": rng.standard_normal((3, 5, 8)).astype(np.float32) for i in range(4)})
    return _simple(pkg, backend, build, feeds)


SITES = {   # name: (builder, proof of the control: None = kernels_last_graph below the fusion-off run, or the launch counters of which one must move)
    "unary_f16": (site_unary_f16, None),
    "glu_f16": (site_glu_f16, None),
    "swiglu_q8k": (site_swiglu_q8k, None),
    "soft_max_f16": (site_soft_max_f16, None),
    "cont_permute": (site_cont_permute, None),
    "cont_sink": (site_cont_sink, None),
    "ew_chain": (site_ew_chain, None),
    "gate_up_swiglu": (site_gate_up_swiglu, ("gemm_glu_launches", "gemm_glu96_launches")),
    "gemm_resid_norm": (site_gemm_resid_norm, None),
    "gemm_bias_gelu": (site_gemm_bias_gelu, None),
    "stream_encoder": (site_stream_encoder, None),
    "grouped_split_k": (site_grouped_split_k, ("norm_rope_split_launches",)),
    "gemm_any_bias_gelu": (site_gemm_any_bias_gelu, None),
    "gemm_any_siblings": (site_gemm_any_siblings, None),
    "layer_norm": (site_layer_norm, None),
    "rope_chain_f16": (site_rope_chain_f16, None),
    "rope_chain_store": (site_rope_chain_store, None),
    "deferred_norm_q8_0": (_site_deferred_norm("q8_0"), None),
    "deferred_norm_q4_K": (_site_deferred_norm("q4_K"), None),
    "attn_sm_batch": (site_attn_sm_batch, None),
    "decode_gs_fold": (_site_decoder(1), ("fattn_gs_launches",)),
    "decode_q8k_image": (_site_decoder(4), None),
    "attn_f32": (site_attn_f32, None),
    "norm_modulate": (site_norm_modulate, None),
    "gate_norm": (site_gate_norm, None),
    "causal_conv": (_site_causal_conv(False), None),
    "concat_tail": (site_concat_tail, ("concat_tails",)),
    "conv1d": (site_conv1d, None),
    "lazy_cache": (_site_causal_conv(True), ("lazy_conts",)),
    "lazy_attn": (site_lazy_attn, ("lazy_conts",)),
    "copy_prune": (site_copy_prune, ("copies_forwarded", "copies_dropped")),
}
T2W_SITES = list(SITES)[list(SITES).index("attn_f32"):]
ALL_MOVE = {"copy_prune"}                                               # (every counter of the proof must move, not one of them)
LAZY = {"lazy_cache": 2, "lazy_attn": 4}                                # copies the control leaves un-run per graph (test_t2w_gpu.py:252, :281)
OBS = {
    "unary_f16": ["unary"], "glu_f16": ["glu"], "swiglu_q8k": ["glu"], "soft_max_f16": ["soft_max"], "cont_permute": ["cont"], "cont_sink": ["producer"],
    "ew_chain": ["first", "middle"], "gate_up_swiglu": ["gate", "up", "glu"], "gemm_resid_norm": ["mul_mat"], "gemm_bias_gelu": ["mul_mat", "add", "gelu"],
    "stream_encoder": ["k_rows", "v_rows", "v_window_cont", "v_cast"], "grouped_split_k": ["q", "k", "v"], "gemm_any_bias_gelu": ["mul_mat", "add"],
    "gemm_any_siblings": ["first", "sibling"], "layer_norm": ["norm", "mul", "add"], "rope_chain_f16": ["mul", "rope"], "rope_chain_store": ["k_mul", "k_rope"],
    "deferred_norm_q8_0": ["norm", "mul"], "deferred_norm_q4_K": ["norm", "mul"], "attn_sm_batch": ["kq", "soft_max", "kqv"], "decode_gs_fold": ["attention"],
    "decode_q8k_image": ["attention"],
    "attn_f32": ["kq", "scale", "soft_max", "kqv"], "norm_modulate": ["norm", "mul", "add1"], "gate_norm": ["gate_mul", "norm", "mul", "add1", "x"],
    "causal_conv": ["x_t", "concat", "cont", "im2col0", "mul_mat1", "concat_b", "cont_back"], "concat_tail": ["cont_x", "concat", "cont"],
    "conv1d": ["im2col", "col_cont", "kernel_cont", "mul_mat", "prod_cont", "bias_cont", "repeat"], "lazy_cache": ["cache_in", "cache_tcb"],
    "lazy_attn": ["q_flat", "k_flat", "v_flat", "v_t"], "copy_prune": ["p3", "pack"],
}
NO_SPLIT = {"swiglu_q8k", "decode_q8k_image", ("gate_norm", "x")}       # (these sites / nodes are written in every case: see the module's docstring)
OBSERVED = [(s, o, v) for s in SITES for o in OBS[s] for v in ("output", "split") if not (v == "split" and (s in NO_SPLIT or (s, o) in NO_SPLIT))]


# ================================================================================================ the tests
@pytest.mark.parametrize("name", list(SITES))
def test_control_takes_the_fused_path(pkg, be, ref_be, name):
    proof = SITES[name][1]
    before = {k: be.get_stat(k) for k in proof or ()}
    run, k_on = _three_runs(pkg, be, ref_be, name, None, "control")
    run.close()
    moved = {k: be.get_stat(k) - before[k] for k in before}
    be.set_option("fusion", 0)
    try:
        off = Run(pkg, be, name)
        try:
            off.check(off.submit(0), _reference(pkg, ref_be, name)[0], (name, "fusion off"))
            k_off = off.kernels
        finally:
            off.close()
    finally:
        be.set_option("fusion", 1)
    print(f"{name}: {k_on} launches fused, {k_off} with fusion off, counters {moved}")
    assert k_on - 1 < k_off - 8, (k_on, k_off)                          # (without the pad: eight launches with fusion off, one element-wise chain with it)
    if proof:
        assert any(v >= 1 for v in moved.values()), moved
    if name in ALL_MOVE:
        assert all(v >= 1 for v in moved.values()), moved
    if name in LAZY:
        assert run.moved["lazy_conts"] == LAZY[name] and run.moved["lazy_conts_materialised"] == 0, run.moved


@pytest.mark.parametrize("name,key,variant", OBSERVED, ids=[f"{s}-{o}-{v}" for s, o, v in OBSERVED])
def test_interior_node_is_written_for_a_reader_outside_the_split(pkg, be, ref_be, name, key, variant):
    run, k_first = _three_runs(pkg, be, ref_be, name, key, variant)
    if name in LAZY:                                                    # an observed lazy copy became real: it was not left un-run, and it was launched or made real later
        k_control = _control_launches(pkg, be, name)
        print(f"{name}/{key}/{variant}: {k_first} launches ({k_control} in the control), {run.moved}")
        assert run.moved["lazy_conts"] < LAZY[name], run.moved
        assert k_first > k_control or run.moved["lazy_conts_materialised"] >= 1, (k_first, k_control, run.moved)
    if variant == "split":                                              # the counts say what the test means them to say: one more use than the split holds
        parent, (first, second) = run.graph(True)
        inside = sum(1 for T in run.nodes[:run.cut] for k in range(10) if T.t.src[k] and _same(T.t.src[k], run.t))
        assert first.use_count(run.t) == inside + 1 and second.g.n_nodes == 1
    run.close()


def _same(p, T):
    import ctypes
    return ctypes.addressof(p.contents) == ctypes.addressof(T.t)


_CONTROL = {}


def _control_launches(pkg, be, name):
    """kernels_last_graph of the site's control, eager (once per site)"""
    if name not in _CONTROL:
        _fresh(be)
        run = Run(pkg, be, name)
        try:
            run.submit(0)
            _CONTROL[name] = run.kernels
        finally:
            run.close()
    return _CONTROL[name]


VIEWED = [("cont_permute", "cont"), ("soft_max_f16", "soft_max"), ("ew_chain", "middle"), ("layer_norm", "add"), ("stream_encoder", "v_cast"),
          ("attn_f32", "soft_max"), ("causal_conv", "cont"), ("conv1d", "prod_cont"), ("lazy_attn", "k_flat"), ("copy_prune", "pack")]


@pytest.mark.parametrize("where", ["split_view", "split_view_front"])
@pytest.mark.parametrize("name,key", VIEWED, ids=[f"{s}-{o}" for s, o in VIEWED])
def test_interior_node_read_through_a_view_node_only(pkg, be, ref_be, name, key, where):
    """split_view: RESHAPE(t) and its reader both lie in the second split (t's count carries the view node).  split_view_front: the RESHAPE lies in the first split, so t's own
    uses are all inside it -- it is the VIEW whose count exceeds its uses there, and run_nodes' walk along view_src (graph_exec.cpp) must keep t's bytes."""
    run, _ = _three_runs(pkg, be, ref_be, name, key, where)
    parent, (first, second) = run.graph(True)
    view = run.reader._srcs[0]
    assert view.t.view_src and _same(view.t.view_src, run.t)
    if where == "split_view_front":
        assert first.use_count(view) == 1 and not any(_same(T.t.src[k], run.t) for T in run.nodes[run.cut:] for k in range(10) if T.t.src[k])
    else:
        assert second.g.n_nodes == 2
    run.close()


CROWDED = [("soft_max_f16", "soft_max"), ("cont_sink", "producer"), ("gemm_any_bias_gelu", "add"), ("lazy_attn", "q_flat"), ("causal_conv", "im2col0")]


@pytest.mark.parametrize("name,key", CROWDED, ids=[f"{s}-{o}" for s, o in CROWDED])
def test_interior_node_displaced_in_a_tight_parent_table(pkg, be, ref_be, name, key):
    run, _ = _three_runs(pkg, be, ref_be, name, key, "split", crowded=True)
    parent, _ = run.graph(True)
    slot, home = parent.slot_of(run.t)
    assert slot is not None and slot != home, (slot, home)             # found only by probing on
    assert run.size == len(run.nodes) + parent.g.n_leafs and parent.hash_size == pkg.ggml_hash_size(run.size)
    assert any(parent.slot_of(T)[0] < parent.slot_of(T)[1] for T in run.spares)      # and one probe sequence of the table wraps
    run.close()


FLIPS = [("soft_max_f16", "soft_max"), ("unary_f16", "unary"), ("cont_sink", "producer"), ("ew_chain", "middle"), ("gemm_any_bias_gelu", "add"), ("layer_norm", "mul"),
         ("rope_chain_store", "k_rope"), ("attn_sm_batch", "soft_max"),
         ("attn_f32", "soft_max"), ("gate_norm", "gate_mul"), ("causal_conv", "cont"), ("lazy_attn", "v_t"), ("concat_tail", "concat"), ("copy_prune", "pack")]


@pytest.mark.parametrize("name,key", FLIPS, ids=[f"{s}-{o}" for s, o in FLIPS])
def test_capture_is_not_replayed_once_the_interior_node_has_an_outside_reader(pkg, be, ref_be, name, key):
    """control three times (eager, capture, replay) on view(0, cut) of a parent WITHOUT the outside reader; then the same node array as view(0, cut) of the parent WITH it
    (same nodes, same data pointers, same fingerprint: only recs_match's `ext` tells them apart), three times; then the control's graph again with the OUTPUT flag set
    (recs_match's `flags`).  The interior node is poisoned before each run and must be written every time it is observed."""
    ref = _reference(pkg, ref_be, name)
    _fresh(be)
    run = Run(pkg, be, name, key, "split")
    try:
        r0 = be.get_stat("graph_replays")
        for k in range(3):
            run.check(run.submit(k, with_reader=False, observed=False), ref[k], (name, "control", k))
        assert be.get_stat("graph_replays") - r0 >= 1, "the control did not replay"
        k_control = run.kernels
        m0 = be.get_stat("graph_fp_mismatch")
        for k in range(3):
            run.check(run.submit(k + 1, with_reader=True, observed=True), ref[(k + 1) % N_SETS], (name, "reader in the counts", k))
            if k == 0:
                assert be.get_stat("graph_fp_mismatch") - m0 == 1, "the capture of the control was not dropped by its record"
        run.t.t.flags |= OUTPUT
        for k in range(3):
            run.check(run.submit(k + 2, with_reader=False, observed=True), ref[(k + 2) % N_SETS], (name, "OUTPUT flag", k))
        run.t.t.flags &= ~OUTPUT
        run.check(run.submit(0, with_reader=False, observed=False), ref[0], (name, "control again"))
        assert run.kernels == k_control, (run.kernels, k_control)
        if name in T2W_SITES:                                           # ... and the control is captured and replayed again (a copy dropped or left lazy in it is dropped again)
            r1 = be.get_stat("graph_replays")
            for k in (1, 2):
                run.check(run.submit(k, with_reader=False, observed=False), ref[k], (name, "control again", k))
            assert be.get_stat("graph_replays") - r1 >= 1 and run.kernels == k_control, (be.get_stat("graph_replays") - r1, run.kernels, k_control)
    finally:
        run.close()
