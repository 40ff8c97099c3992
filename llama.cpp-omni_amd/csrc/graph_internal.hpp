// graph_internal.hpp -- what the three translation units of the graph executor share: graph_plan.cpp (supports_op, which kernel family a MUL_MAT takes, scratch
// sizing), graph_exec.cpp + graph_exec_llm.cpp + graph_exec_t2w.cpp (the node executors and their fusion matchers), graph.cpp (fingerprints, capture records, graph_compute / graph_optimize, options).
#pragma once
#include "graph.hpp"
#include <chrono>
#include "ggml_util.hpp"
#include "kernels.hpp"
#include "shadow.hpp"
#include "../../include/ggml-mi355x.h"
#include <unordered_map>
#include <unordered_set>

namespace mi {

// ------------------------------------------------------------------------------------------------ helpers
static inline tdesc td(const ggml_tensor * t) {
    tdesc d; d.p = t->data;
    for (int i = 0; i < 4; ++i) { d.ne[i] = t->ne[i]; d.nb[i] = t->nb[i]; }
    return d;
}
static inline bool is_noop(const ggml_tensor * t) {
    return t->op == GGML_OP_NONE || t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_PERMUTE ||
           t->op == GGML_OP_TRANSPOSE || is_empty(t);
}
// one step down a view chain: what a RESHAPE / VIEW / PERMUTE / TRANSPOSE node looks at (null: t is no such node)
static inline const ggml_tensor * view_parent(const ggml_tensor * t) {
    return (t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_PERMUTE || t->op == GGML_OP_TRANSPOSE) ? t->src[0] : nullptr;
}
// the ops whose launch is one strided copy: they may join the copy queue instead of flushing it
static inline bool is_plain_copy(int op) { return op == GGML_OP_CONT || op == GGML_OP_CONCAT || op == GGML_OP_CPY || op == GGML_OP_DUP; }
struct byte_range { const char * lo; const char * hi; };
static inline byte_range range_of(const ggml_tensor * t) { const char * p = (const char *) t->data; return { p, p + nbytes(t) }; }
static inline bool overlap(byte_range a, byte_range b) { return a.lo < b.hi && b.lo < a.hi && a.lo != a.hi && b.lo != b.hi; }

enum act_kind { ACT_NONE = 0, ACT_Q8K, ACT_Q80, ACT_F16, ACT_F32, ACT_Q8KT, ACT_F16Q, ACT_Q81 };      // Q81: the Q8_0 image plus the per-block s = d * sum(qs) (Q4_1 / Q5_1 weights)      // F16Q: f16 rows of the Q8_K-quantised values (what the F16-image GEMMs of K-quant weights multiply with)      // Q8KT: the block-major Q8_K image of a whole ubatch (mmq_tile.hip), not a per-row format
// block formats whose only kernels of their own are the integer mat-vecs of mmvq.hip (up to 8 columns: Q4_1 / Q5_1 on Q8_1 images, Q2_K / Q3_K on
// Q8_K images): from 9 columns on every MUL_MAT runs on the F16 image of the weights (resident for model tensors, shadow.hpp, built by the first
// GEMM; else de-quantised into scratch per call) with f16-rounded activations.  Q2_K / Q3_K share the Q8_K image with the K-quants, but none of
// the K-quant launch forms (fusions, mmq, the pair / grouped launches, the k_mv2 engine) takes them: those test is_kquant / the type.
static inline bool is_image_quant(int t) {
    return t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q2_K || t == GGML_TYPE_Q3_K;
}
static inline size_t act_image_bytes(act_kind k, int64_t K) {
    switch (k) {
        case ACT_Q8K: return q8k_image_bytes(K);
        case ACT_Q80: return q80_image_bytes(K);
        case ACT_Q81: return q81_image_bytes(K);
        case ACT_F16: case ACT_F16Q: return ((size_t) K * 2 + 15) & ~(size_t) 15;
        default: return 0;
    }
}

// ------------------------------------------------------------------------------------------------ state the executor carries from one node to a later one
// Each piece says once: where it lives, who sets it, who consumes it, what ends it.  All of it dies with the exec_state (one per graph_compute).
// The three CACHES own their key AND the bytes they were computed from: note_write passes every written range to invalidate(); one that does not hold() costs a launch.
// act -- in act_scratch: x's rows in the format `kind`, row r of the flattened [ne1 * ne2 * ne3] at r * act_image_bytes(kind, K).  Set by seed(): prepare_act, and every
//   producer that writes its result's image in its own launch (materialise_norm, SWIGLU, SOFT_MAX, the gathering CONT, the attention launches; through seed_act_f16: UNARY,
//   GLU, the norms, the GEMM epilogues).  Consumed by prepare_act, op_mul_mat's any-shape GEMM, mv1_source.  Ended by act_begin() -- where every writer of the scratch gets
//   the pointer, so one that forgets to seed leaves no record -- and by a write into x.
struct act_cache {
    const void * src = nullptr; act_kind kind = ACT_NONE; int64_t K = 0, ne[3] = { 0, 0, 0 }; size_t nb[3] = { 0, 0, 0 }; byte_range from = { nullptr, nullptr };
    bool holds(const ggml_tensor * x, act_kind k) const { return holds_row(x, k, x->ne[1]) && nb[0] == x->nb[1] && nb[1] == x->nb[2] && nb[2] == x->nb[3]; }
    // mv1_source's batch-1 mat-vecs ([K, 1, 1, 1] at every caller): one row, whose strides address nothing (a one-row view carries its parent's) -- left out
    bool holds_row(const ggml_tensor * x, act_kind k, int64_t rows = 1) const { return src == x->data && kind == k && K == x->ne[0] && ne[0] == rows && ne[1] == x->ne[2] && ne[2] == x->ne[3]; }
    void seed(const ggml_tensor * x, act_kind k) { src = x->data; kind = k; K = x->ne[0]; from = range_of(x); for (int d = 0; d < 3; ++d) { ne[d] = x->ne[d + 1]; nb[d] = x->nb[d + 1]; } }
    void drop() { src = nullptr; }      void invalidate(byte_range w) { if (src && overlap(w, from)) drop(); }
};
// rt -- in rope_scratch: the (cos, sin) table of T positions x D / 2 pairs (the key rp holds an M-RoPE node's sections).  Set by remember(): ensure_rope_table (the one-token attention launches) and the prefill
//   norm + rope launch, which fills the table itself when told it is not valid.  Consumed by the same (every layer of a graph shares it).  Ended by a write into the
//   positions or frequency factors read.
struct rope_cache {
    const void * pos = nullptr; const void * ff = nullptr; int T = 0, D = 0; rope_params rp; byte_range from_pos = { nullptr, nullptr }, from_ff = { nullptr, nullptr };
    bool holds(const void * p, const void * f, int T_, int D_, const rope_params & r) const { return pos && pos == p && ff == f && T == T_ && D == D_ && memcmp(&rp, &r, sizeof(rope_params)) == 0; }
    void remember(const void * p, const void * f, int T_, int D_, const rope_params & r) {      // T positions (M-RoPE: four rows of T) and D / 2 frequency factors were read
        pos = p; ff = f; T = T_; D = D_; rp = r; from_pos = { (const char *) p, (const char *) p + (size_t) T_ * 4 * (rope_is_mrope(r.mode) ? 4 : 1) }; from_ff = { (const char *) f, f ? (const char *) f + (size_t) (D_ / 2) * 4 : nullptr };
    }
    void drop() { pos = nullptr; }      void invalidate(byte_range w) { if (pos && (overlap(w, from_pos) || overlap(w, from_ff))) drop(); }
};
// mask_map -- at the head of fa_scratch: the tile map of mask `mk` against nq query rows (flash-attention off: an f32 mask's f16 copy behind it).  Set by remember(): the
//   prefill attention launches (exec_fattn on the MFMA kernel, exec_attn_sm_prefill), which compute the map when told it is not valid.  Consumed by the same.  Ended by
//   a write into the mask, and by any other tenant taking the scratch (fa_scratch_take).
struct mask_map_cache {
    const void * mask = nullptr; int64_t ne[4] = { 0, 0, 0, 0 }; size_t nb1 = 0; byte_range from = { nullptr, nullptr };
    bool holds(const ggml_tensor * mk, int64_t nq) const { return mask && mask == mk->data && ne[0] == mk->ne[0] && ne[1] == nq && ne[2] == mk->ne[2] && ne[3] == mk->ne[3] && nb1 == mk->nb[1]; }
    void remember(const ggml_tensor * mk, int64_t nq) { mask = mk->data; ne[0] = mk->ne[0]; ne[1] = nq; ne[2] = mk->ne[2]; ne[3] = mk->ne[3]; nb1 = mk->nb[1]; from = range_of(mk); }
    void drop() { mask = nullptr; }      void invalidate(byte_range w) { if (mask && overlap(w, from)) drop(); }
};

// The scheduler's use counts (ggml_graph_view hands every split the parent's use_counts and visited_hash_set): does the cgraph carry them, and the whole-graph
// use count of t -- ggml_hash_find (ggml-impl.h:257-270): pointer >> 4, linear probing over the `used` bitset -- or -1 for a tensor the table does not hold.
// The one probe: run_nodes derives exec_state::external from it, make_recs / recs_match the capture records' `ext`.
static inline bool graph_has_use_counts(const ggml_cgraph * g) { return g->use_counts && g->visited_hash_set.size > 0 && g->visited_hash_set.keys && g->visited_hash_set.used; }
static inline int whole_use_count(const ggml_cgraph * g, const ggml_tensor * t) {
    const ggml_hash_set & hs = g->visited_hash_set;
    const size_t h = ((size_t) (uintptr_t) t >> 4) % hs.size;
    size_t i = h;
    while ((hs.used[i >> 5] >> (i & 31)) & 1u) {
        if (hs.keys[i] == t) return g->use_counts[i];
        i = (i + 1) % hs.size;
        if (i == h) break;
    }
    return -1;
}

struct exec_state {
    backend_ctx * c;
    hipStream_t   st;
    ggml_cgraph * g = nullptr;
    long          n_kernels = 0, n_fused = 0;
    std::vector<uint8_t> done;                                           // node already covered by a fused item
    std::unordered_map<const ggml_tensor *, int> index;                  // tensor -> node index
    std::unordered_map<const ggml_tensor *, std::vector<int>> users;     // tensor -> consumer node indices (ascending)
    std::unordered_set<const ggml_tensor *> external;                    // tensors with readers outside this cgraph (see is_out)
    bool          capturing = false;
    int           node_lo = 0, node_hi = -1;      // run_nodes walks [node_lo, node_hi) (-1: to the end) -- the slice timer of graph_compute (MI355X_GRAPH_SLICE)
    act_cache      act;
    rope_cache     rt;
    mask_map_cache mask_map;
    // DEFERRED work: a node that did not launch, or whose result is not in its tensor yet.
    // pn -- nowhere yet: RMS_NORM -> MUL(w) = `m`, not computed.  Set by exec_rms_norm.  Consumed by the K-quant / Q8_0 mat-vecs that build the image of m in-kernel
    //   (norm_in_kernel, mv1_source; `left` readers to go).  Ended by the last of them, or by materialise_norm for any other reader (prepare_act, op_mul_mat, settle).
    struct { const ggml_tensor * m = nullptr; const ggml_tensor * x = nullptr; const ggml_tensor * wt = nullptr; float eps = 0; int left = 0; } pn;
    // pq -- nowhere yet: the q chain, k chain + store and v store of a decode layer.  Set by try_defer_qkv_to_attention / _to_softmax_attention (`sm`: the flash-attention-off
    //   form, `fa` = its first MUL_MAT).  Consumed and ended by the attention node `fa`, which runs them in its own launch (exec_fattn / exec_attn_sm_decode).
    struct { int fa = -1; fattn_pre pre; int kst = -1, vst = -1;
             bool sm = false; int sm_soft = -1, sm_mm2 = -1, sm_cont = -1; attn_sm_args sma; } pq;
    // pr -- in gemm_partial: `A` (a mat-mul + residual result; resid2 only in front of a LayerNorm) as `nsplit` split-K slabs.  Set by exec_gemm_group.  Consumed by the
    //   (RMS_)NORM that reads A next and sums the slabs itself (exec_rms_norm, exec_norm).  Ended by that launch, or by materialise_reduce for anybody else (settle).
    struct { const ggml_tensor * A = nullptr; int nsplit = 0; const float * resid = nullptr; size_t resid_cs = 0; const float * resid2 = nullptr; size_t resid2_cs = 0; } pr;
    // prm -- in gemm_partial: the results A[0..n) of a GROUPED launch (wq / wk / wv of a prefill ubatch) as `nsplit` slabs of `slab` floats, matrix q a dense [N][M[q]] block
    //   at + off[q].  Set by exec_gemm_group.  Consumed by the q / k norm + rope + store launch behind it (exec_rms_norm).  Ended by it, or by materialise_group (settle).
    struct { int n = 0; const ggml_tensor * A[3] = { nullptr, nullptr, nullptr }; size_t off[3] = { 0, 0, 0 }; int64_t M[3] = { 0, 0, 0 }; int nsplit = 0; size_t slab = 0; int64_t N = 0; } prm;
    // gs -- in fa_scratch: one-token attention as slices' partial states (k_fattn_gs); the f32 rows of the FLASH_ATTN_EXT node `n` were NOT written.  Set by exec_fattn.
    //   Consumed by `consumer`, the one MUL_MAT (wo) that folds them in its prologue (mv1_source).  Ended by it, or by gs_materialise when anything else runs first (run_nodes).
    struct { const ggml_tensor * n = nullptr; int consumer = -1; int nh = 0, D = 0; } gs;
    // va -- in a transposed V cache: the V^T a fused soft-max attention reads where it LIES instead of from the CONT + CAST copies the graph makes (`cast` = the CAST its second
    //   mat-mul names, `v` = the same elements in the cache).  Set by try_alias_vt.  Consumed and ended by exec_attn_sm_prefill; materialise_vt runs the copies otherwise.
    struct { const ggml_tensor * cast = nullptr; tdesc v; int cont_i = -1, cast_i = -1; } va;
    // vplain -- in the V^T CAST tensor `t` of an encoder: its bytes written as V ROWS ([D, n_tokens, H], like K).  Set by exec_gemm_group once the launch that writes the rows
    //   has taken the CAST.  Consumed and ended by its one reader, the chain exec_attn_sm_prefill runs as plain flash attention (head size 64) -- and by nothing else but the
    //   start of run_nodes.
    struct { const ggml_tensor * t = nullptr; tdesc v; } vplain;
    // CONT nodes that have NOT been run: copies of a view of a tensor from outside the graph (a persistent cache) whose readers may take the view itself (lazy_* in
    // graph_exec.cpp).  `src` = what the copy would read, `deadline` = the first node that writes over those bytes; any other reader materialises the copy first.
    struct lazy_ent { tdesc src; int deadline; };
    std::unordered_map<const ggml_tensor *, lazy_ent> lazy;
    std::unordered_map<const ggml_tensor *, int> lazy_base_deadline;
    // same-type strided copies (CONT / CONCAT / CPY / a lazy copy made real) that have been MET but not launched: mutually independent by byte ranges, they leave as one
    // k_copy_batch launch when a node of another kind is about to run, when a new copy touches bytes a pending one writes (or writes bytes one reads), or at COPY_BATCH_MAX
    // `group` / `Y` / `org`: the node the job belongs to, that node's output, the origin of the job's box in it (a CONCAT is two boxes); `same`: source and destination box have
    // the same shape.  A later copy that reads exactly a pending node's output is FORWARDED: it reads that node's sources instead (copy_queue), so chains of packs leave together
    // `node`: the tensor the group writes -- a group whose tensor has no reader left (every reader so far was forwarded, none comes later, nothing lazy looks at it, it is no
    // output and owns its bytes) is DROPPED instead of launched: the intermediate packs of a CONCAT chain are never written
    struct copy_pending { copy_pair job; const char * rlo, * rhi, * wlo, * whi; int group; tdesc Y; int64_t org[4]; bool same; const ggml_tensor * node; };
    int           cur_node = 0;
    const ggml_tensor * cq_owner = nullptr;          // a node run with its output re-pointed at a CONT sink's buffer (cont_sink): the bytes a queued copy writes belong to the SINK tensor
    struct dead_range { const char * lo, * hi; const ggml_tensor * node; int at; };
    std::vector<dead_range> cq_dead;                 // MI355X_COPY_PRUNE_VERIFY=1: outputs of dropped groups; a later read of one is reported
    int           cq_group = 0;
    std::vector<copy_pending> cq;
    long          n_copies_batched = 0;
};

// ------------------------------------------------------------------------------------------------ profiling
static inline hipEvent_t prof_event(backend_ctx * c) {
    if (!c->prof_event_pool.empty()) { hipEvent_t e = c->prof_event_pool.back(); c->prof_event_pool.pop_back(); return e; }
    hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); return e;
}
struct prof_scope {
    backend_ctx * c; bool on; backend_ctx::pending_prof p;
    prof_scope(exec_state & s, const char * cls, double bytes) : c(s.c), on(s.c->opt_profile && !s.capturing) {
        if (!on) return;
        p.cls = cls; p.bytes = bytes; p.a = prof_event(c); p.b = prof_event(c);
        HIP_CHECK(hipEventRecord(p.a, s.st)); st = s.st;
    }
    ~prof_scope() { if (!on) return; HIP_CHECK(hipEventRecord(p.b, st)); c->prof_pending.push_back(p); }
    hipStream_t st = nullptr;
};
static inline void prof_drain(backend_ctx * c) {
    static const bool each = getenv("MI355X_PROFILE_EACH") != nullptr;            // one line per launch (class, the class's byte / flop figure, us) on stderr
    for (auto & p : c->prof_pending) {
        HIP_CHECK(hipEventSynchronize(p.b));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
        if (each) fprintf(stderr, "[mi355x prof] %-18s %14.0f %9.2f us\n", p.cls.c_str(), p.bytes, ms * 1000.0);
        prof_class & pc = c->prof[p.cls];
        pc.us += ms * 1000.0; pc.bytes += p.bytes; pc.n += 1;
        c->prof_event_pool.push_back(p.a); c->prof_event_pool.push_back(p.b);
    }
    c->prof_pending.clear();
}


// ---- graph_plan.cpp
static const int64_t ROPE_TABLE_MIN_TOKENS = 32;
static const int64_t GEMM_MIN_COLS = MI_MMVQ_MAX_COLS + 1;
// Which kernel family a MUL_MAT node takes: decided once, by route_mul_mat, for the planner (supports_op), the scratch sizing and the executor (op_mul_mat).
enum mm_path { MM_MMQ_TILE, MM_GEMM_F16_HEADS, MM_GEMM_F16, MM_GEMM_BF16, MM_GEMM_ANY, MM_MMV_HEADS, MM_MMQ, MM_MMV };
struct mm_route {
    mm_path  path;
    act_kind act;            // the image of x the path reads (prepare_act; ACT_F32 / ACT_NONE: the f32 rows themselves)
    bool     gemm;           // the F16 GEMM's conditions hold (mm_uses_gemm): MM_GEMM_F16*, and MM_MMQ_TILE as its sub-case -- unless MI355X_NO_GEMM / _MMQ_MAX_COLS under 8 leave the tile kernel alone
    bool     w_image;        // the weights are read through their F16 image (shadow, else w_scratch) rather than as blocks
    int64_t  k_head;         // MM_GEMM_ANY: the K - K % 64 columns the F16 GEMM may take first (0: none)
    int64_t  k_head_sized;   // what graph_gemm_partial_need reserves split-K scratch for: k_head's shape rule alone, on any path behind the F16 GEMM's
};
mm_route route_mul_mat(const ggml_tensor * n);
// ... and a MUL_MAT_ID node: admitted or not (supports_op), the image of b's columns its path reads (both paths of a K-quant node read ACT_Q8K, both of an MXFP4 node
// ACT_Q80, a block-form node the image of its dense mat-vec) and the path: the per-pair mat-vec, or from MMQ_ID_MIN_TOKENS (K-quants) / mmq_id_mxfp4_min_tokens() (MXFP4) /
// mmq_id_blocks_min_tokens() (Q8_0, Q4_0, Q5_0, IQ4_NL) tokens on the expert-grouped int8-MFMA kernel of the type (scratch sizing, the executor's MUL_MAT_ID case)
enum mm_id_path { MM_ID_MMV, MM_ID_MMQ };
struct mm_id_route { bool ok; act_kind act; mm_id_path path; };
mm_id_route route_mul_mat_id(const ggml_tensor * n);
// the token count from which K-quant experts take the grouped kernel.  Above 33: up to there one mmv_id launch per node is what the per-pair tests count.
static const int64_t MMQ_ID_MIN_TOKENS = 64;
static_assert(MMQ_ID_MIN_TOKENS > 33, "the per-pair mat-vec keeps every token count up to 33");
// ... and MXFP4 experts theirs (mmq_id.hip, mxfp4_dec).  Above 64: the per-pair MXFP4 tests count one mmv_id_mxfp4 launch per node up to 64 tokens.  MI355X_MMQ_ID_MXFP4_MIN_TOKENS
// (read once, floor 65) moves it for measurements: mmq_id_mxfp4_min_tokens()
static const int64_t MMQ_ID_MXFP4_MIN_TOKENS = 128;
static_assert(MMQ_ID_MXFP4_MIN_TOKENS > 64, "the per-pair MXFP4 mat-vec keeps every token count up to 64");
int64_t mmq_id_mxfp4_min_tokens();
// ... and Q8_0 / Q4_0 / Q5_0 / IQ4_NL experts theirs (mmq_id.hip, the four f16-header Decs).  Above 64: the per-pair tests keep their path.  65 is the measured value: at the Qwen3-30B-A3B
// and DeepSeek-V2-Lite expert shapes the grouped kernel is level with the per-pair one (Q4_0, 1.00 x) or ahead (up to 2.6 x) at 65 tokens already and ahead from there
// on, for all four forms (profiles/moe_blocks_crossover.txt).  MI355X_MMQ_ID_BLOCKS_MIN_TOKENS (read once, floor 65) moves it for measurements: mmq_id_blocks_min_tokens()
static const int64_t MMQ_ID_BLOCKS_MIN_TOKENS = 65;
static_assert(MMQ_ID_BLOCKS_MIN_TOKENS > 64, "the per-pair block-form mat-vec keeps every token count up to 64");
int64_t mmq_id_blocks_min_tokens();
void mmq_id_set_mode(int m);                            // option "mmq_id": 0 = every node on the per-pair kernel
// one row per admitted weight type (null: none; BF16 has a path of its own): the image its mat-vec kernels read, their launcher (up to 8 columns) and profile class
struct mmv_row { int type; act_kind act; void (*launch)(const mmv_args &, hipStream_t); const char * cls; };
const mmv_row * mmv_row_for(int wtype);
bool mm_uses_mmq(const ggml_tensor * n);                // the views of the route the fusion matchers ask for
bool mm_uses_gemm(const ggml_tensor * n);
bool mm_uses_mmq_tile(const ggml_tensor * n);
bool mm_takes_gemm_any(const ggml_tensor * n);
bool mm_uses_gemm_any_f16(const ggml_tensor * n);
act_kind gemm_act_kind(const ggml_tensor * n);          // ACT_F16, or ACT_F16Q for K-quant weights (option "prefill_q8k")
void prefill_q8k_set_mode(int m);
void mmq_tile_set_mode(int m);
int64_t mmq_max_cols();
size_t graph_act_scratch_need(const ggml_cgraph * g);
size_t graph_w_scratch_need(const ggml_cgraph * g);
size_t graph_moe_scratch_need(const ggml_cgraph * g);
void fill_fattn_args(const ggml_tensor * n, fattn_args & f, tdesc & m);
size_t graph_fa_scratch_need(const ggml_cgraph * g);
size_t graph_rope_scratch_need(const ggml_cgraph * g);
int64_t gemm_group_split_max_cols();
size_t graph_gemm_partial_need(const ggml_cgraph * g);
bool ensure_scratch(backend_ctx * c, void ** p, size_t * have, size_t need);
// ---- graph_exec.cpp
long attn_vrows_launches();                           // flash-attention-off chains run on V rows that exec_gemm_group wrote (graph_exec_llm.cpp)
void run_nodes(exec_state & s, ggml_cgraph * g);
} // namespace mi
