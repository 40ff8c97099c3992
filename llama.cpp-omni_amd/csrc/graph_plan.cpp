// graph_plan.cpp -- planner side of the graph executor: supports_op (what the backend admits), which kernel family a MUL_MAT takes by shape and type,
// and the scratch a cgraph needs before its first launch.  (Split out of graph.cpp in round 4; no behaviour change.)
#include "graph_internal.hpp"
#include <algorithm>

namespace mi {

// ------------------------------------------------------------------------------------------------ supports_op
bool supports_op(const ggml_tensor * op) {
    const ggml_tensor * s0 = op->src[0];
    const ggml_tensor * s1 = op->src[1];
    switch (op->op) {
        case GGML_OP_NONE: case GGML_OP_RESHAPE: case GGML_OP_VIEW: case GGML_OP_PERMUTE: case GGML_OP_TRANSPOSE:
            return true;
        case GGML_OP_MUL_MAT: {
            if (!s0 || !s1) return false;
            if (s0->type == GGML_TYPE_BF16)                          // BF16 weights: the any-shape f32-MFMA GEMM at every column count (gemm_any.hip)
                return s1->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == 2 && s1->nb[0] == 4 && op->nb[0] == 4 && s0->nb[1] >= (size_t) s0->ne[0] * 2 &&
                       s0->ne[2] != 0 && s0->ne[3] != 0 && s1->ne[2] % s0->ne[2] == 0 && s1->ne[3] % s0->ne[3] == 0 && s1->ne[2] * s1->ne[3] <= 65535;
            const act_kind k = mmv_row_for(s0->type) ? mmv_row_for(s0->type)->act : ACT_NONE;
            if (k == ACT_NONE || op->type != GGML_TYPE_F32) return false;
            if (s1->type != GGML_TYPE_F32 && !(s1->type == GGML_TYPE_F16 && k == ACT_F16)) return false;      // F16 x F16: the convolutions' mat-mul
            if (s0->ne[0] % blck_size(s0->type) != 0) return false;
            if (s0->nb[0] != type_size(s0->type) || s1->nb[0] != type_size(s1->type) || op->nb[0] != sizeof(float)) return false;
            if (s0->nb[1] < row_size(s0->type, s0->ne[0])) return false;          // transposed weights: not handled
            if (s0->ne[2] == 0 || s0->ne[3] == 0 || s1->ne[2] % s0->ne[2] != 0 || s1->ne[3] % s0->ne[3] != 0) return false;
            if (k == ACT_Q8K || k == ACT_Q80 || k == ACT_Q81) {
                // 16-B / 4-B / 2-B vector paths assume block-aligned rows (always true for ggml-allocated tensors)
                const int t = s0->type;
                const size_t al = (t == GGML_TYPE_Q4_K || t == GGML_TYPE_Q5_K) ? 16 : (t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q2_K) ? 4 : 2;
                if (s0->nb[1] % al != 0 || (al == 4 && ((uintptr_t) s0->data & 3) != 0)) return false;
            }
            // every mat-vec path (up to 8 columns per launch; F32 weights at any width) stages one activation column in LDS: a column
            // beyond 152 KiB has no kernel (e.g. attention without FLASH_ATTN_EXT past ~77k cache rows: K = n_kv) -> leave it to the CPU
            const mm_route r = route_mul_mat(op);
            if (!r.gemm && r.path != MM_MMQ && r.path != MM_GEMM_ANY) {                  // (gemm_any stages nothing in LDS)
                const size_t col = k == ACT_F32 ? (size_t) s0->ne[0] * 4 : act_image_bytes(k, s0->ne[0]);
                if (col > (size_t) 152 * 1024) return false;
            }
            return true;
        }
        case GGML_OP_MUL_MAT_ID:
            return route_mul_mat_id(op).ok;
        case GGML_OP_ADD_ID: {                                // the asserts of ggml_add_id (ggml.c:1985-1988) and ggml_compute_forward_add_id_f32 (ops.cpp:707-723)
            const ggml_tensor * ids = op->src[2];
            if (!s0 || !s1 || !ids) return false;
            if (op->type != GGML_TYPE_F32 || s0->type != GGML_TYPE_F32 || s1->type != GGML_TYPE_F32 || ids->type != GGML_TYPE_I32) return false;
            if (s0->nb[0] != 4 || s1->nb[0] != 4 || op->nb[0] != 4 || ids->nb[0] % 4 != 0 || ids->nb[1] % 4 != 0) return false;
            return s0->ne[0] == s1->ne[0] && s0->ne[1] == ids->ne[0] && s0->ne[2] == ids->ne[1] && same_shape(s0, op) && s1->ne[1] >= 1 && s1->ne[1] <= INT32_MAX && nrows(op) <= INT32_MAX;
        }
        case GGML_OP_ARGSORT:                                 // one workgroup's LDS holds the padded row (argsort.hip); rows are read through nb1..nb3
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_I32 && s0->nb[0] == 4 && is_contiguous(op) && same_shape(s0, op) && argsort_ok(s0->ne[0]) &&
                   (op_param_i32(op, 0) == 0 || op_param_i32(op, 0) == 1);      // enum ggml_sort_order (ggml.h): ASC = 0, DESC = 1
        case GGML_OP_SSM_CONV: {                              // the asserts of ggml_ssm_conv (ggml.c:5165-5176) and ggml_compute_forward_ssm_conv_f32 (ops.cpp:8520-8523); types, shapes
                                                              // and strides only -- the loader probes with tensors that have no data (llama-model.cpp:233-256)
            if (!s0 || !s1 || s0->type != GGML_TYPE_F32 || s1->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32) return false;
            if (s0->nb[0] != 4 || s0->nb[1] != (size_t) s0->ne[0] * 4 || s1->nb[0] != 4 || op->nb[0] != 4) return false;
            if (s0->ne[3] != 1 || s1->ne[2] != 1 || s1->ne[3] != 1 || op->ne[3] != 1) return false;
            if (op->ne[0] != s0->ne[1] || s1->ne[1] != s0->ne[1] || s0->ne[0] != s1->ne[0] - 1 + op->ne[1] || op->ne[2] != s0->ne[2]) return false;
            return ssm_conv_ok(s1->ne[0], s1->ne[1], op->ne[1], op->ne[2]);          // d_conv 2 .. 8; grid y: tokens (decode) or 64-token tiles, grid z: sequences (<= 65535)
        }
        case GGML_OP_SSM_SCAN: {                              // the asserts of ggml_ssm_scan (ggml.c:5198-5235) and ggml_compute_forward_ssm_scan_f32 (ops.cpp:8599-8607); no ->data
            const ggml_tensor * s = s0, * x = s1, * dt = op->src[2], * A = op->src[3], * B = op->src[4], * Cc = op->src[5], * ids = op->src[6];
            if (!s || !x || !dt || !A || !B || !Cc || !ids) return false;
            if (s->type != GGML_TYPE_F32 || x->type != GGML_TYPE_F32 || dt->type != GGML_TYPE_F32 || A->type != GGML_TYPE_F32 || B->type != GGML_TYPE_F32 || Cc->type != GGML_TYPE_F32 ||
                ids->type != GGML_TYPE_I32 || op->type != GGML_TYPE_F32) return false;
            if (!is_contiguous(s) || !is_contiguous(dt) || !is_contiguous(A) || !is_contiguous(op) || ids->nb[0] != 4) return false;
            if (x->nb[0] != 4 || B->nb[0] != 4 || Cc->nb[0] != 4 || x->nb[1] != (size_t) x->ne[0] * 4 || B->nb[1] != (size_t) B->ne[0] * 4 || Cc->nb[1] != (size_t) Cc->ne[0] * 4) return false;
            if (x->nb[2] % 4 != 0 || x->nb[3] % 4 != 0 || B->nb[2] % 4 != 0 || B->nb[3] % 4 != 0 || Cc->nb[2] % 4 != 0 || Cc->nb[3] % 4 != 0) return false;
            if (!same_shape(B, Cc)) return false;
            const int64_t d_state = s->ne[0], head_dim = x->ne[0], n_head = x->ne[1], n_t = x->ne[2], n_s = x->ne[3], n_group = B->ne[1];
            if (dt->ne[0] != n_head || dt->ne[1] != n_t || dt->ne[2] != n_s || dt->ne[3] != 1 || s->ne[1] != head_dim || s->ne[2] != n_head || s->ne[3] < 1) return false;
            if (B->ne[0] != d_state || B->ne[2] != n_t || B->ne[3] != n_s || ids->ne[0] != n_s || ids->ne[1] != 1 || ids->ne[2] != 1 || ids->ne[3] != 1) return false;
            if (A->ne[1] != n_head || A->ne[2] != 1 || A->ne[3] != 1 || (A->ne[0] != 1 && A->ne[0] != d_state)) return false;      // one decay per head (Mamba-2) or per state element (Mamba-1)
            if (nelements(op) != nelements(x) + d_state * head_dim * n_head * n_s) return false;
            // d_state 16 / 32 / 64 / 128 / 256 (a row lies on d_state / 4 lanes of one wave), n_head % n_group == 0; grid x: the row groups of a sequence, grid y: sequences (<= 65535)
            return ssm_scan_ok(d_state, head_dim, n_head, n_group, n_t, n_s);
        }
        case GGML_OP_RWKV_WKV6: case GGML_OP_GATED_LINEAR_ATTN: case GGML_OP_RWKV_WKV7: {
            // the asserts of ggml_rwkv_wkv6 / ggml_gated_linear_attn / ggml_rwkv_wkv7 (ggml.c:5369-5499); types, shapes and strides only -- the loader probes WKV6 with S = H =
            // n_tokens = n_seqs = 123, a 4-D state {S, n_seqs, S, H} and no data (llama-model.cpp:257-271)
            const int n_src = op->op == GGML_OP_RWKV_WKV6 ? 6 : op->op == GGML_OP_RWKV_WKV7 ? 7 : 5;
            const ggml_tensor * k = op->src[op->op == GGML_OP_RWKV_WKV7 ? 2 : 0], * state = op->src[n_src - 1];
            if (!k || !state || op->type != GGML_TYPE_F32 || !is_contiguous(op)) return false;
            const int64_t S = k->ne[0], H = k->ne[1], T = k->ne[2], n_seqs = state->ne[1];
            for (int q = 0; q < n_src; ++q) {
                const ggml_tensor * t = op->src[q];
                if (!t || t->type != GGML_TYPE_F32 || !is_contiguous(t)) return false;
                if (t == state) continue;
                // time_first: the constructor asserts no shape, and the loader's probe passes the file's own {head_size, n_head} weight beside its 123-sized operands --
                // a refusal there sends the weight to the CPU.  A graph that reaches the executor with anything but S * H elements is an error there.
                if (op->op == GGML_OP_RWKV_WKV6 && q == 3) { if (nelements(t) < 1) return false; continue; }
                if (t->ne[0] != S || t->ne[1] != H || t->ne[2] != T || t->ne[3] != 1) return false;
            }
            if (!wkv_ok(S, H, T, n_seqs)) return false;               // 1 <= S <= 128, T % n_seqs == 0, grid y: heads, grid z: sequences (<= 65535 each)
            return nelements(state) == S * S * H * n_seqs && op->ne[0] == S * H && op->ne[1] == T + S * n_seqs && op->ne[2] == 1 && op->ne[3] == 1;
        }
        case GGML_OP_L2_NORM:                                 // ggml_compute_forward_l2_norm_f32 (ops.cpp:3858-3899): f32 rows with nb[0] == 4, read through nb1..nb3; eps >= 0
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == 4 && op->nb[0] == 4 && same_shape(s0, op) && op_param_f32(op, 0) >= 0.0f &&
                   l2_norm_ok(s0->ne[0], nrows(s0));
        case GGML_OP_ADD: case GGML_OP_SUB: case GGML_OP_MUL: case GGML_OP_DIV:
            return s0 && s1 && s0->type == GGML_TYPE_F32 && s1->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 &&
                   same_shape(s0, op) && can_repeat(s1, s0);
        case GGML_OP_RMS_NORM:
        case GGML_OP_NORM:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == 4 && op->nb[0] == 4;
        case GGML_OP_IM2COL:
            // src0 = kernel (shape only), src1 = f32 image with dense [IH, IW] planes, dst dense f16 / f32
            return s0 && s1 && s1->type == GGML_TYPE_F32 && (op->type == GGML_TYPE_F16 || op->type == GGML_TYPE_F32) && is_contiguous(op) && s1->nb[0] == 4 &&
                   (op_param_i32(op, 6) != 1 || s1->nb[1] == (size_t) s1->ne[0] * 4) && nelements(op) < ((int64_t) 1 << 40);
        case GGML_OP_POOL_2D:
            return s0 && (s0->type == GGML_TYPE_F32 || s0->type == GGML_TYPE_F16) && op->type == GGML_TYPE_F32 && is_contiguous(op) &&
                   s0->nb[0] == (s0->type == GGML_TYPE_F32 ? 4u : 2u) && (s0->ne[3] == 1 || s0->nb[3] == (size_t) s0->ne[2] * s0->nb[2]) &&
                   (op_param_i32(op, 0) == GGML_OP_POOL_AVG || op_param_i32(op, 0) == GGML_OP_POOL_MAX);
        case GGML_OP_POOL_1D:                                 // the reference implements k == s, p == 0 only (ops.cpp:7270-7276)
            return s0 && (s0->type == GGML_TYPE_F32 || s0->type == GGML_TYPE_F16) && op->type == GGML_TYPE_F32 && is_contiguous(op) && is_contiguous(s0) &&
                   op_param_i32(op, 1) == op_param_i32(op, 2) && op_param_i32(op, 3) == 0 &&
                   (op_param_i32(op, 0) == GGML_OP_POOL_AVG || op_param_i32(op, 0) == GGML_OP_POOL_MAX);
        case GGML_OP_SCALE:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && is_contiguous(s0) && is_contiguous(op);
        // ---- the Token2Wav graphs' extra ops (kernels/t2w_ops.hip)
        case GGML_OP_SQR: case GGML_OP_SQRT: case GGML_OP_LOG: case GGML_OP_SIN: case GGML_OP_COS: case GGML_OP_CLAMP: case GGML_OP_LEAKY_RELU:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && is_contiguous(s0) && is_contiguous(op);
        case GGML_OP_CONCAT: {
            if (!s0 || !s1 || s0->type != op->type || s1->type != op->type) return false;
            const int t = op->type;
            return t == GGML_TYPE_F32 || t == GGML_TYPE_I32 || t == GGML_TYPE_F16;
        }
        case GGML_OP_REPEAT: {
            if (!s0 || s0->type != op->type || !can_repeat(s0, op)) return false;
            const int t = op->type;
            return t == GGML_TYPE_F32 || t == GGML_TYPE_I32 || t == GGML_TYPE_F16;
        }
        case GGML_OP_PAD:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == 4 && is_contiguous(op);
        case GGML_OP_PAD_REFLECT_1D:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && op_param_i32(op, 0) < s0->ne[0] && op_param_i32(op, 1) < s0->ne[0];
        case GGML_OP_ARANGE:
            return op->type == GGML_TYPE_F32 && is_contiguous(op);
        case GGML_OP_TIMESTEP_EMBEDDING:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == 4 && op->nb[0] == 4;
        case GGML_OP_SUM_ROWS:
            return s0 && s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == 4;
        case GGML_OP_CONV_TRANSPOSE_1D:          // (ggml_conv_transpose_1d asserts p0 == 0, d0 == 1 and a 2-D src1)
            return s0 && s1 && (s0->type == GGML_TYPE_F16 || s0->type == GGML_TYPE_F32) && s1->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 &&
                   s0->nb[0] == (s0->type == GGML_TYPE_F16 ? 2u : 4u) && s1->nb[0] == 4 && op->nb[0] == 4 && s1->ne[2] == 1 && s1->ne[3] == 1 && s0->ne[3] == 1;
        case GGML_OP_UNARY: {
            if (!s0 || s0->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32 || !is_contiguous(s0) || !is_contiguous(op)) return false;
            switch (op_param_i32(op, 0)) {
                case GGML_UNARY_OP_ABS: case GGML_UNARY_OP_SGN: case GGML_UNARY_OP_NEG: case GGML_UNARY_OP_STEP: case GGML_UNARY_OP_TANH:
                case GGML_UNARY_OP_ELU: case GGML_UNARY_OP_RELU: case GGML_UNARY_OP_SIGMOID: case GGML_UNARY_OP_GELU: case GGML_UNARY_OP_GELU_QUICK:
                case GGML_UNARY_OP_SILU: case GGML_UNARY_OP_HARDSWISH: case GGML_UNARY_OP_HARDSIGMOID: case GGML_UNARY_OP_EXP: case GGML_UNARY_OP_GELU_ERF:
                    return true;
                default: return false;
            }
        }
        case GGML_OP_GLU: {
            if (!s0 || s0->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32) return false;
            if (!is_contiguous_1(s0) || !is_contiguous_1(op) || (s1 && (!is_contiguous_1(s1) || s1->type != GGML_TYPE_F32))) return false;
            switch (op_param_i32(op, 0)) {
                case GGML_GLU_OP_REGLU: case GGML_GLU_OP_GEGLU: case GGML_GLU_OP_SWIGLU: case GGML_GLU_OP_GEGLU_ERF: case GGML_GLU_OP_GEGLU_QUICK: return true;
                case GGML_GLU_OP_SWIGLU_OAI: return true;                 // alpha = op_params[2], limit = op_params[3] (gpt-oss experts)
                default: return false;
            }
        }
        case GGML_OP_ROPE: {
            if (!s0 || !s1 || s0->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32 || s1->type != GGML_TYPE_I32) return false;
            const int mode = op_param_i32(op, 2);
            const int n_dims = op_param_i32(op, 1);
            if (op->src[2] && op->src[2]->type != GGML_TYPE_F32) return false;
            if (mode == GGML_ROPE_TYPE_MROPE || mode == GGML_ROPE_TYPE_VISION) {                // ggml_rope_multi (Qwen2-VL text layers, and its ViT): four rows of positions, sections in op_params[11..14]
                const int sc[4] = { op_param_i32(op, 11), op_param_i32(op, 12), op_param_i32(op, 13), op_param_i32(op, 14) };
                if (sc[0] < 0 || sc[1] < 0 || sc[2] < 0 || sc[3] < 0 || !(sc[0] > 0 || sc[1] > 0 || sc[2] > 0)) return false;       // (the reference asserts a positive t, h or w section ...
                if ((int64_t) sc[0] + sc[1] + sc[2] + sc[3] > s0->ne[0] || s1->ne[0] < 4 * s0->ne[2] || s1->nb[0] != 4) return false;     //  ... and sect_dims <= ne0)
                if (n_dims <= 0 || n_dims > s0->ne[0] || (mode == GGML_ROPE_TYPE_VISION && n_dims != s0->ne[0] / 2)) return false;
                if (op->src[2] && op->src[2]->ne[0] < (mode == GGML_ROPE_TYPE_VISION ? n_dims : n_dims / 2)) return false;           // one factor per rotated pair
            } else if (mode != GGML_ROPE_TYPE_NORMAL && mode != GGML_ROPE_TYPE_NEOX) return false;                                    // every other mode value: CPU.  So are F16 rotation and ROPE_BACK
            return s0->nb[0] == 4 && op->nb[0] == 4 && (n_dims % 2) == 0;
        }
        case GGML_OP_SOFT_MAX:
            if (!s0 || s0->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32 || !is_contiguous(op) || s0->nb[0] != 4) return false;
            if (s1 && s1->type != GGML_TYPE_F16 && s1->type != GGML_TYPE_F32) return false;
            if (s1 && s1->nb[0] != type_size(s1->type)) return false;
            if (op->src[2] && op->src[2]->type != GGML_TYPE_F32) return false;
            return s0->ne[0] * 4 <= 150 * 1024;
        case GGML_OP_CPY: case GGML_OP_CONT: case GGML_OP_DUP: {
            if (!s0) return false;
            const int a = s0->type, b = op->type;
            const bool fl = (a == GGML_TYPE_F32 || a == GGML_TYPE_F16) && (b == GGML_TYPE_F32 || b == GGML_TYPE_F16);
            const bool fi = (a == GGML_TYPE_F32 && b == GGML_TYPE_I32) || (a == GGML_TYPE_I32 && b == GGML_TYPE_F32);      // ggml_cast to / from i32 (Token2Wav masks)
            return (fl || fi || (a == GGML_TYPE_I32 && b == GGML_TYPE_I32)) && nelements(s0) == nelements(op);
        }
        case GGML_OP_GET_ROWS: {
            if (!s0 || !s1 || s1->type != GGML_TYPE_I32 || op->type != GGML_TYPE_F32 || op->nb[0] != 4) return false;
            switch (s0->type) {
                case GGML_TYPE_F32: case GGML_TYPE_F16: case GGML_TYPE_BF16: case GGML_TYPE_Q8_0: case GGML_TYPE_Q4_K: case GGML_TYPE_Q6_K:
                case GGML_TYPE_Q4_0: case GGML_TYPE_Q4_1: case GGML_TYPE_Q5_0: case GGML_TYPE_Q5_1: case GGML_TYPE_Q2_K: case GGML_TYPE_Q3_K: case GGML_TYPE_Q5_K:
                case GGML_TYPE_IQ4_NL: case GGML_TYPE_IQ4_XS:
                    return s0->nb[0] == type_size(s0->type);
                default: return false;
            }
        }
        case GGML_OP_SET_ROWS:
            return s0 && s1 && s0->type == GGML_TYPE_F32 &&
                   (op->type == GGML_TYPE_F16 || op->type == GGML_TYPE_F32 || op->type == GGML_TYPE_BF16 || ((op->type == GGML_TYPE_Q8_0 || op->type == GGML_TYPE_Q4_0) && s0->ne[0] % 32 == 0)) &&
                   (s1->type == GGML_TYPE_I64 || s1->type == GGML_TYPE_I32) && s0->nb[0] == 4 && op->nb[0] == type_size(op->type);
        case GGML_OP_FLASH_ATTN_EXT: {
            const ggml_tensor * q = s0, * k = s1, * v = op->src[2], * m = op->src[3];
            if (!q || !k || !v) return false;
            if (q->type != GGML_TYPE_F32 || k->type != v->type || op->type != GGML_TYPE_F32) return false;
            if (k->type != GGML_TYPE_F16 && k->type != GGML_TYPE_F32 && k->type != GGML_TYPE_BF16 && k->type != GGML_TYPE_Q8_0 && k->type != GGML_TYPE_Q4_0) return false;
            if (q->ne[0] != k->ne[0]) return false;
            // the MFMA / streaming / one-token kernels (F16 cache, head 64 / 128); anything else -- other head sizes, a quantised / BF16 / F32 cache -- fattn_wide.hip where fa_wide_plan takes it, else fattn_any.hip
            const bool special = k->type == GGML_TYPE_F16 && (q->ne[0] == 64 || q->ne[0] == 128) && v->ne[0] == q->ne[0];
            if (!special && (q->ne[0] > 576 || v->ne[0] > 576)) return false;
            if ((k->type == GGML_TYPE_Q8_0 || k->type == GGML_TYPE_Q4_0) && (k->ne[0] % 32 != 0 || v->ne[0] % 32 != 0)) return false;
            if (q->nb[0] != 4 || k->nb[0] != type_size(k->type) || v->nb[0] != type_size(v->type)) return false;
            if (special && (k->nb[1] % 16 != 0 || v->nb[1] % 16 != 0 || k->nb[2] % 16 != 0 || v->nb[2] % 16 != 0)) return false;
            if (m && (m->type != GGML_TYPE_F16 || m->nb[0] != 2)) return false;
            if (op->src[4] && op->src[4]->type != GGML_TYPE_F32) return false;
            if (k->ne[2] == 0 || q->ne[2] % k->ne[2] != 0 || k->ne[2] != v->ne[2] || q->ne[3] != k->ne[3]) return false;
            return is_contiguous(op);
        }
        default:
            return false;
    }
}

// ------------------------------------------------------------------------------------------------ MUL_MAT routing
static const mmv_row MMV_ROWS[] = {
    { GGML_TYPE_Q4_K,   ACT_Q8K, mmv_q4_K,   "mmv_q4k"   },
    { GGML_TYPE_Q5_K,   ACT_Q8K, mmv_q5_K,   "mmv_f32"   },      // (Q5_K, Q4_0 and Q5_0 launches have always been booked under mmv_f32)
    { GGML_TYPE_Q6_K,   ACT_Q8K, mmv_q6_K,   "mmv_q6k"   },
    { GGML_TYPE_Q8_0,   ACT_Q80, mmv_q8_0,   "mmv_q80"   },
    // Q4_0 / Q5_0: integer mat-vec kernels on Q8_0 activations up to 8 columns (mmvq.hip), the F16 image from 9 columns on
    { GGML_TYPE_Q4_0,   ACT_Q80, mmv_q4_0,   "mmv_f32"   },
    { GGML_TYPE_Q5_0,   ACT_Q80, mmv_q5_0,   "mmv_f32"   },
    // IQ4_NL / IQ4_XS: integer mat-vec kernels up to 8 columns (mmvq.hip: IQ4_NL on Q8_0 images, IQ4_XS on Q8_K images), the F16 image from 9 columns on.
    // IQ4_XS shares the Q8_K image with the K-quants, but none of the K-quant launch forms (fusions, mmq, the k_mv2 engine) takes it: those test is_kquant / the type.
    { GGML_TYPE_IQ4_NL, ACT_Q80, mmv_iq4_nl, "mmv_iq4nl" },
    { GGML_TYPE_IQ4_XS, ACT_Q8K, mmv_iq4_xs, "mmv_iq4xs" },
    // Q4_1 / Q5_1 (Q8_1 images) and Q2_K / Q3_K (Q8_K images): integer mat-vec kernels up to 8 columns (mmvq.hip), the F16 image from 9 columns on
    { GGML_TYPE_Q4_1,   ACT_Q81, mmv_q4_1,   "mmv_q41"   },
    { GGML_TYPE_Q5_1,   ACT_Q81, mmv_q5_1,   "mmv_q51"   },
    { GGML_TYPE_Q2_K,   ACT_Q8K, mmv_q2_K,   "mmv_q2k"   },
    { GGML_TYPE_Q3_K,   ACT_Q8K, mmv_q3_K,   "mmv_q3k"   },
    { GGML_TYPE_F16,    ACT_F16, mmv_f16,    "mmv_f16"   },
    { GGML_TYPE_F32,    ACT_F32, mmv_f32,    "mmv_f32"   },
};
const mmv_row * mmv_row_for(int wtype) {
    for (const mmv_row & r : MMV_ROWS) if (r.type == wtype) return &r;
    return nullptr;
}
// batches of more than 8 columns go to the MFMA GEMM (activations rounded to f16; quantised weights de-quantised to f16 first)
// ... except K-quant weights against up to MMQ_MAX_COLS columns (several sequences decoded together, drafts, small ubatches): those
// read the quantised blocks themselves on the int8 matrix cores (mmq.hip) -- 0.56 / 0.82 bytes per weight instead of the 2 of an f16 image
int64_t mmq_max_cols() {
    static const int64_t v = getenv("MI355X_MMQ_MAX_COLS") ? atoll(getenv("MI355X_MMQ_MAX_COLS")) : 64;
    return v;
}
static int64_t mmq_min_cols() {       // narrower batches stay on the dot4 mat-vec kernels (one column: 4.3 TB/s; the MFMA tile would be 1/32 full).
    // measured crossover (12288 x 4096 Q4_K: dot4 8.0 / 11.2 / 19.0 us at 2 / 4 / 8 columns, mmq 13.3 us flat): 6 columns
    static const int64_t v = getenv("MI355X_MMQ_MIN_COLS") ? atoll(getenv("MI355X_MMQ_MIN_COLS")) : 6;
    return v;
}
static bool mmq_takes(const ggml_tensor * n) {
    const ggml_tensor * w = n->src[0], * x = n->src[1];
    return (w->type == GGML_TYPE_Q4_K || w->type == GGML_TYPE_Q5_K || w->type == GGML_TYPE_Q6_K) && x->type == GGML_TYPE_F32 && x->ne[1] >= mmq_min_cols() && x->ne[1] <= mmq_max_cols() &&
           mmq_ok(w->type, w->ne[0], w->data, w->nb[1]) && (w->ne[2] == 1 || mmq_ok(w->type, w->ne[0], (const char *) w->data + w->nb[2], w->nb[1])) &&
           (w->ne[3] == 1 || mmq_ok(w->type, w->ne[0], (const char *) w->data + w->nb[3], w->nb[1]));
}
// Q4_K weights against a prefill ubatch (more than mmq_max_cols() columns): the tiled int8-MFMA kernel on the blocks themselves and the Q8_K-quantised
// activations -- the oracle's integers (mmq_tile.hip).  A sub-case of the F16 GEMM (mm_uses_gemm): the grouping / residual / split-K machinery of the GEMM path serves it.
static int g_mmq_tile = -1;                                   // option "mmq_tile": -1 = MI355X_MMQ_TILE decides (default off), 0 off, 1 on
void mmq_tile_set_mode(int m) { g_mmq_tile = m; }
static bool mmq_tile_takes(const ggml_tensor * n) {
    static const int env = getenv("MI355X_MMQ_TILE") ? atoi(getenv("MI355X_MMQ_TILE")) : 0;      // (off by default: exact, but slower than the F16-image GEMM -- DESIGN.md section 7, profiles/r05_mmq_tile.txt)
    if (!(g_mmq_tile >= 0 ? g_mmq_tile : env)) return false;
    const ggml_tensor * w = n->src[0], * x = n->src[1];
    if (w->type != GGML_TYPE_Q4_K || x->type != GGML_TYPE_F32 || n->type != GGML_TYPE_F32) return false;
    if (x->ne[1] <= mmq_max_cols() || x->ne[2] != 1 || x->ne[3] != 1 || w->ne[2] != 1 || w->ne[3] != 1 || x->nb[0] != 4 || n->nb[0] != 4) return false;
    if (x->nb[1] % 16 != 0 || ((uintptr_t) x->data & 15) != 0) return false;
    return mmq_tile_ok(w->type, w->ne[0], w->data, w->nb[1]);
}
// The activations of an MFMA GEMM node: f16-rounded rows -- or, for K-quant weights (the reference CPU backend quantises src1 to Q8_K for every one of them,
// ggml-cpu.c:1272-1306 with vec_dot_type Q8_K), f16 rows of the Q8_K-QUANTISED values, so that the product on the weights' F16 image differs from the reference's
// integer arithmetic by f16 rounding only (NMSE 2e-6 per mat-mul), not by the reference's own 8-bit quantisation noise (5e-5).  Option "prefill_q8k", default OFF: it costs two
// re-quantisation launches per layer (pp512 44.7 k -> 41.5 k tok/s) and end to end both forms sit on the reference's own rounding-flip floor (tests/test_round5_gpu.py).
static int g_prefill_q8k = -1;
void prefill_q8k_set_mode(int m) { g_prefill_q8k = m; }
act_kind gemm_act_kind(const ggml_tensor * n) {
    static const int env = getenv("MI355X_PREFILL_Q8K") ? atoi(getenv("MI355X_PREFILL_Q8K")) : 0;
    if (!(g_prefill_q8k >= 0 ? g_prefill_q8k : env)) return ACT_F16;
    const ggml_tensor * w = n->src[0], * x = n->src[1];
    const int t = w->type;
    const bool kq = t == GGML_TYPE_Q2_K || t == GGML_TYPE_Q3_K || t == GGML_TYPE_Q4_K || t == GGML_TYPE_Q5_K || t == GGML_TYPE_Q6_K;
    return kq && x->type == GGML_TYPE_F32 && x->ne[0] % 256 == 0 ? ACT_F16Q : ACT_F16;
}
static bool gemm_f16_takes(const ggml_tensor * n) {
    const ggml_tensor * w = n->src[0], * x = n->src[1];
    static const bool no_gemm = getenv("MI355X_NO_GEMM") != nullptr;
    if (x->ne[1] < GEMM_MIN_COLS || no_gemm) return false;
    if (mmq_takes(n)) return false;
    if (!mmv_row_for(w->type) || w->type == GGML_TYPE_F32) return false;         // F16 and every block format, through its F16 image
    const int64_t K = w->ne[0];
    if (K % 32 != 0) return false;
    if (w->type == GGML_TYPE_F16 && (w->nb[1] % 16 != 0 || w->nb[2] % 16 != 0 || w->nb[3] % 16 != 0 || ((uintptr_t) w->data & 15) != 0)) return false;
    // per-head products (an encoder's V^T . P over a growing K/V cache: K = 50, 100, ... positions): the DMA GEMM batches heads only at K % 64 == 0 and would
    // otherwise go out head by head (Whisper streaming chunk 16, K = 800: 384 extra launches); the any-shape f16 kernel takes every head in one launch
    if (w->type == GGML_TYPE_F16 && x->ne[2] * x->ne[3] > 1 && K % 64 != 0 && x->type == GGML_TYPE_F32 && x->ne[2] * x->ne[3] <= 65535) return false;
    return true;
}
// The one place where shape, type, stride and alignment choose the path of a MUL_MAT node that supports_op admits; the order is op_mul_mat's.
mm_route route_mul_mat(const ggml_tensor * n) {
    const ggml_tensor * w = n->src[0], * x = n->src[1];
    const int64_t K = w->ne[0], M = w->ne[1], N = x->ne[1], nbatch = x->ne[2] * x->ne[3];
    const mmv_row * row = mmv_row_for(w->type);
    mm_route r = { MM_MMV, row ? row->act : ACT_NONE, gemm_f16_takes(n), false, 0, 0 };
    if (mmq_tile_takes(n)) { r.path = MM_MMQ_TILE; r.act = ACT_Q8KT; return r; }      // Q4_K x a prefill ubatch: the tiled int8-MFMA kernel on the Q8_K image (mmq_tile.hip)
    if (r.gemm) {
        // ---- prefill: MFMA GEMM.  X -> f16 rows (what the reference does for F16 weights, ggml-cpu.c:1245-1268); quantised W -> f16
        r.act = nbatch == 1 ? gemm_act_kind(n) : ACT_F16;
        // attention without FLASH_ATTN_EXT at prefill: every head's K.Q^T (or V^T.P) product in one launch  (F16 rows here are 16-byte aligned: gemm_f16_takes)
        if (w->type == GGML_TYPE_F16 && nbatch > 1 && nbatch <= 65535 && K % 64 == 0 && n->nb[0] == 4) { r.path = MM_GEMM_F16_HEADS; return r; }
        r.path = MM_GEMM_F16; r.w_image = w->type != GGML_TYPE_F16;
        return r;
    }
    if (w->type == GGML_TYPE_BF16) { r.path = MM_GEMM_BF16; return r; }               // the any-shape f32-MFMA GEMM at every column count (gemm_any.hip)
    // F16 weights, K a few columns past a multiple of 64 (SigLip2's n_ff 4304): the F16 MFMA GEMM takes the first K - K % 64 columns, the any-shape kernel adds the tail
    if (w->type == GGML_TYPE_F16 && x->type == GGML_TYPE_F32 && nbatch == 1 && K % 64 != 0 && K >= 512 && N > MI_MMVQ_MAX_COLS) r.k_head_sized = K - K % 64;
    // more than 8 columns against F32 weights, or F16 weights with a contraction length the F16 GEMM does not take (the omni encoders, Token2Wav):
    // one f32-MFMA launch over every (head, batch) instead of a mat-vec launch per 8 columns per head
    static const bool no_gemm_any = getenv("MI355X_NO_GEMM_ANY") != nullptr;
    if (!no_gemm_any && (w->type == GGML_TYPE_F32 || w->type == GGML_TYPE_F16) && N > MI_MMVQ_MAX_COLS &&
        ((x->type == GGML_TYPE_F32 && x->nb[0] == 4) || (x->type == GGML_TYPE_F16 && x->nb[0] == 2 && w->type == GGML_TYPE_F16)) && w->nb[0] == (w->type == GGML_TYPE_F16 ? 2u : 4u) && n->nb[0] == 4 &&
        nbatch <= 65535 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31)) {
        r.path = MM_GEMM_ANY;
        if (w->nb[1] % 16 == 0 && ((uintptr_t) w->data & 15) == 0) r.k_head = r.k_head_sized;
        return r;
    }
    // attention without FLASH_ATTN_EXT: K / V^T per KV head against one activation per query head -- every head in ONE launch  (f32 rows are read in place: one batch stride)
    if ((w->type == GGML_TYPE_F16 || w->type == GGML_TYPE_F32) && nbatch > 1 && N <= MI_MMVQ_MAX_COLS && nbatch <= 65535 &&
        (r.act != ACT_F32 || x->ne[3] == 1 || x->nb[3] == (size_t) x->ne[2] * x->nb[2])) { r.path = MM_MMV_HEADS; return r; }
    if (mmq_takes(n)) { r.path = MM_MMQ; return r; }                                  // 6 .. 64 columns of a K-quant matrix: int8 MFMA, 32 columns per launch
    return r;                                                                         // the type's own mat-vec kernels, on the blocks (w_image only ever with the GEMM)
}
// The same for MUL_MAT_ID (as [K, M, n_expert], b [K, 1 | n_ids, T] f32, ids [n_ids, T] i32 -> [M, n_ids, T]).  Two paths:
//   MM_ID_MMV  the per-pair mat-vec -- mmvk.hip for K-quant experts (Q8_K images), mmv_mxfp4.hip for MXFP4 experts (gpt-oss; Q8_0 images, 17-byte blocks: no row or
//              expert alignment condition);
//   MM_ID_MMQ  K-quant experts from MMQ_ID_MIN_TOKENS tokens on: the pairs grouped by expert on the device, mmq.hip's int8-MFMA body per (expert, 32 rows, <= 32 columns)
//              (mmq_id.hip) -- a weight block is read once per 32 columns of its expert instead of once per pair.  MXFP4 experts from mmq_id_mxfp4_min_tokens() tokens
//              on: the same grouping and kernel frame, one int8 MFMA per 17-byte block, no alignment condition.  Same images, same admission: the path changes
//              nothing in what supports_op takes.
// Experts of the nine block forms of mmvq.hip (Q8_0, Q4_0/1, Q5_0/1, IQ4_NL/XS, Q2_K, Q3_K):
//   MM_ID_MMV  the dense frame at one column behind the id indirection (mmvq.hip k_mmv_blocks_id), on the image the form's dense mat-vec reads (Q8_0 / Q8_1 / Q8_K);
//              row and expert strides under the form's alignment, as supports_op states for MUL_MAT (4 bytes and a 4-byte-aligned base for Q4_1 / Q5_1 / Q2_K, 2 bytes
//              for the rest);
//   MM_ID_MMQ  Q8_0 / Q4_0 / Q5_0 / IQ4_NL (a 32-weight block against the Q8_0 image, no min term) from mmq_id_blocks_min_tokens() tokens on: the grouping, then one int8
//              MFMA per block (mmq_id.hip, the MXFP4 body with another block decoder).  Q4_1 / Q5_1 / Q2_K / Q3_K / IQ4_XS experts stay per-pair at every token count.
// F16 / F32 / BF16 experts have no kernel with the id indirection: refused, they stay on the CPU.
static int g_mmq_id = -1;                                     // option "mmq_id": -1 = MI355X_MMQ_ID decides (default on), 0 off (the cross-check switch), 1 on
void mmq_id_set_mode(int m) { g_mmq_id = m; }
int64_t mmq_id_mxfp4_min_tokens() {
    static const int64_t v = [] { const char * e = getenv("MI355X_MMQ_ID_MXFP4_MIN_TOKENS"); const int64_t n = e ? atoll(e) : MMQ_ID_MXFP4_MIN_TOKENS; return n < 65 ? (int64_t) 65 : n; }();
    return v;
}
int64_t mmq_id_blocks_min_tokens() {
    static const int64_t v = [] { const char * e = getenv("MI355X_MMQ_ID_BLOCKS_MIN_TOKENS"); const int64_t n = e ? atoll(e) : MMQ_ID_BLOCKS_MIN_TOKENS; return n < 65 ? (int64_t) 65 : n; }();
    return v;
}
// an admitted node takes the grouped path: the option, enough tokens for the type's family, a pair list and an expert histogram of bounded size, the kernel's LDS (the
// columns' block scales: K up to ~70 k for K-quants, ~9 k for the 32-weight blocks) and, for K-quants, the MFMA body's vector-load alignment for expert 0 and (through
// nb[2]) every other expert
static bool mm_id_grouped(const ggml_tensor * as, const ggml_tensor * ids) {
    static const int env = getenv("MI355X_MMQ_ID") ? atoi(getenv("MI355X_MMQ_ID")) : 1;
    const int fam = mmq_id_family(as->type);
    if (fam < 0 || !(g_mmq_id >= 0 ? g_mmq_id : env)) return false;
    const int64_t K = as->ne[0], min_tokens = fam == MMQ_ID_KQUANT ? MMQ_ID_MIN_TOKENS : fam == MMQ_ID_MXFP4 ? mmq_id_mxfp4_min_tokens() : mmq_id_blocks_min_tokens();
    if (ids->ne[1] < min_tokens || ids->ne[0] * ids->ne[1] > MMQ_ID_MAX_PAIRS || as->ne[2] > MMQ_ID_MAX_EXPERTS || mmq_id_lds_bytes(as->type, K) > MMQ_ID_LDS_MAX) return false;
    return fam != MMQ_ID_KQUANT || (mmq_ok(as->type, K, as->data, as->nb[1]) && (as->ne[2] == 1 || mmq_ok(as->type, K, (const char *) as->data + as->nb[2], as->nb[1])));
}
mm_id_route route_mul_mat_id(const ggml_tensor * n) {
    mm_id_route r = { false, ACT_NONE, MM_ID_MMV };
    const ggml_tensor * as = n->src[0], * b = n->src[1], * ids = n->src[2];
    if (!as || !b || !ids) return r;
    const int t = as->type;
    const bool blocks = t == GGML_TYPE_Q8_0 || t == GGML_TYPE_Q4_0 || t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_IQ4_NL ||
                        t == GGML_TYPE_IQ4_XS || t == GGML_TYPE_Q2_K || t == GGML_TYPE_Q3_K;
    if (t != GGML_TYPE_Q4_K && t != GGML_TYPE_Q5_K && t != GGML_TYPE_Q6_K && t != GGML_TYPE_MXFP4 && !blocks) return r;
    if (b->type != GGML_TYPE_F32 || n->type != GGML_TYPE_F32 || ids->type != GGML_TYPE_I32) return r;
    if (as->nb[0] != type_size(t) || b->nb[0] != 4 || n->nb[0] != 4 || ids->nb[0] % 4 != 0 || ids->nb[1] % 4 != 0 || b->nb[1] % 4 != 0) return r;
    if (as->ne[3] != 1 || b->ne[3] != 1 || ids->ne[2] != 1 || ids->ne[3] != 1 || n->ne[3] != 1) return r;                 // the asserts of ggml_mul_mat_id (ggml.c:3088-3096)
    if (as->ne[0] != b->ne[0] || ids->ne[1] != b->ne[2] || b->ne[1] < 1 || ids->ne[0] % b->ne[1] != 0 || as->ne[2] < 1) return r;
    if (n->ne[0] != as->ne[1] || n->ne[1] != ids->ne[0] || n->ne[2] != b->ne[2]) return r;
    if (ids->ne[0] > 65535 || b->ne[2] > 65535 || as->ne[2] > INT32_MAX || as->ne[1] > INT32_MAX) return r;                // grid y / z
    const int64_t K = as->ne[0];
    if (t == GGML_TYPE_MXFP4) {
        if (K < 32 || K % 32 != 0 || K > INT32_MAX || q80_image_bytes(K) > (size_t) 152 * 1024) return r;                 // one column's Q8_0 image in LDS
        if (as->nb[1] < row_size(t, K)) return r;
        r.ok = true; r.act = ACT_Q80;
        if (mm_id_grouped(as, ids)) r.path = MM_ID_MMQ;
        return r;
    }
    if (blocks) {
        const act_kind act = mmv_row_for(t)->act;                                                                         // Q8_0 / Q8_1 / Q8_K: the dense mat-vec's image
        const int64_t wpb = act == ACT_Q8K ? 256 : 32;                                                                    // weights per block
        if (K < wpb || K % wpb != 0 || K > INT32_MAX || act_image_bytes(act, K) > (size_t) 152 * 1024) return r;           // one column's image in LDS
        if (as->nb[1] < row_size(t, K)) return r;
        const size_t al = (t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q2_K) ? 4 : 2;                     // the forms' loads, for every expert's rows
        if (as->nb[1] % al != 0 || as->nb[2] % al != 0 || ((uintptr_t) as->data & (al - 1)) != 0) return r;
        r.ok = true; r.act = act;
        if (mm_id_grouped(as, ids)) r.path = MM_ID_MMQ;                                                                    // (Q8_0 / Q4_0 / Q5_0 / IQ4_NL only: mmq_id_family)
        return r;
    }
    if (K % 256 != 0 || K > INT32_MAX || q8k_image_bytes(K) > (size_t) 152 * 1024) return r;                              // one column's image in LDS
    if (as->nb[1] < row_size(t, K)) return r;
    const size_t al = t == GGML_TYPE_Q6_K ? 2 : 16;                                                                       // the vector loads' row alignment, as MUL_MAT -- for every expert's rows
    if (as->nb[1] % al != 0 || as->nb[2] % al != 0) return r;
    r.ok = true; r.act = ACT_Q8K;
    if (mm_id_grouped(as, ids)) r.path = MM_ID_MMQ;
    return r;
}
bool mm_uses_mmq(const ggml_tensor * n)       { return route_mul_mat(n).path == MM_MMQ; }
bool mm_uses_mmq_tile(const ggml_tensor * n)  { return route_mul_mat(n).path == MM_MMQ_TILE; }
bool mm_takes_gemm_any(const ggml_tensor * n) { return route_mul_mat(n).path == MM_GEMM_ANY; }
bool mm_uses_gemm(const ggml_tensor * n)      { return route_mul_mat(n).gemm; }
// MM_GEMM_ANY on the f16 kernel (gemm_any.hip k_gemm_any_h): F16 weights the DMA GEMMs do not take (odd K, unaligned rows) against more than 8 f32 columns -- it reads
// a ready-made f16 activation image as well as the f32 rows.  MI355X_NO_GEMM_ANY_H: the node stays on its path, but no producer emits the image for it.
bool mm_uses_gemm_any_f16(const ggml_tensor * n) {
    static const bool off = getenv("MI355X_NO_GEMM_ANY_H") != nullptr;
    return !off && n->src[0]->type == GGML_TYPE_F16 && n->src[1]->type == GGML_TYPE_F32 && route_mul_mat(n).path == MM_GEMM_ANY;
}

// ------------------------------------------------------------------------------------------------ scratch sizing
size_t graph_act_scratch_need(const ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        if (n->op == GGML_OP_MUL_MAT_ID && !is_empty(n)) {           // one image per column of b
            const size_t b = act_image_bytes(route_mul_mat_id(n).act, n->src[1]->ne[0]) * (size_t) (n->src[1]->ne[1] * n->src[1]->ne[2] * n->src[1]->ne[3]);
            if (b > need) need = b;
            continue;
        }
        if (n->op != GGML_OP_MUL_MAT || is_empty(n)) continue;
        const mm_route r = route_mul_mat(n);
        const size_t b = r.path == MM_MMQ_TILE ? mmqt_image_bytes(n->src[1]->ne[0], n->src[1]->ne[1])
                                               : act_image_bytes(r.act, n->src[1]->ne[0]) * (size_t) (n->src[1]->ne[1] * n->src[1]->ne[2] * n->src[1]->ne[3]);
        if (b > need) need = b;
    }
    return need;
}
// the grouped MUL_MAT_ID's pair list, tile table and tile count (mmq_id.hip; every family alike): one grouping per node, the largest node's
size_t graph_moe_scratch_need(const ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        if (n->op != GGML_OP_MUL_MAT_ID || is_empty(n) || route_mul_mat_id(n).path != MM_ID_MMQ) continue;
        const size_t b = moe_group_bytes(n->src[2]->ne[0] * n->src[2]->ne[1], n->src[0]->ne[2]);
        if (b > need) need = b;
    }
    return need;
}
size_t graph_w_scratch_need(const ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        if (n->op != GGML_OP_MUL_MAT || is_empty(n) || !route_mul_mat(n).w_image) continue;
        const size_t b = (size_t) n->src[0]->ne[0] * (size_t) n->src[0]->ne[1] * 2;
        if (b > need) need = b;
    }
    return need;
}
void fill_fattn_args(const ggml_tensor * n, fattn_args & f, tdesc & m) {
    f.q = td(n->src[0]); f.k = td(n->src[1]); f.v = td(n->src[2]); f.dst = td(n);
    if (n->src[3]) m = td(n->src[3]);
    f.mask = n->src[3] ? &m : nullptr;
    f.sinks = n->src[4] ? (const float *) n->src[4]->data : nullptr;
    f.scale = op_param_f32(n, 0); f.max_bias = op_param_f32(n, 1); f.logit_softcap = op_param_f32(n, 2);
    f.scratch = nullptr; f.scratch_bytes = 0; f.kv_type = n->src[1]->type;
}
size_t graph_fa_scratch_need(const ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        if (n->op == GGML_OP_SOFT_MAX && !is_empty(n) && n->ne[1] == 1 && n->ne[3] == 1 && n->ne[0] > 256) {      // flash-attention off, one token, deep cache: the slices' partial rows (attn_one_sm)
            const size_t b = (size_t) n->ne[2] * (size_t) ((n->ne[0] + 255) / 256) * (128 + 2) * 4;
            if (b > need) need = b;
            continue;
        }
        if (n->op == GGML_OP_SOFT_MAX && !is_empty(n) && n->ne[1] > 32 && n->src[1] && n->src[1]->ne[2] == 1 && n->src[1]->ne[3] == 1) {      // flash-attention off, a batch of rows: mask tile map + f16 copy of an f32 mask (exec_attn_sm_prefill)
            const size_t b = ((fattn_map_bytes_host(n->ne[1], n->ne[0]) + 255) & ~(size_t) 255) + (size_t) n->src[1]->ne[1] * (size_t) n->ne[0] * 2;
            if (b > need) need = b;
            continue;
        }
        if (n->op != GGML_OP_FLASH_ATTN_EXT || is_empty(n)) continue;
        fattn_args f; tdesc m; fill_fattn_args(n, f, m);
        size_t b = fattn_scratch_bytes(f);
        if (n->src[0]->ne[1] == 1 && n->src[0]->ne[3] == 1 && n->src[0]->ne[0] == 128) b = std::max(b, fattn_gs_parts_bytes((int) n->src[0]->ne[2], 128));     // one token: the slices' partial states (k_fattn_gs)
        if (b > need) need = b;
    }
    return need;
}
size_t graph_rope_scratch_need(const ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        if (n->op != GGML_OP_ROPE || (n->ne[2] < ROPE_TABLE_MIN_TOKENS && n->ne[2] != 1)) continue;     // (one token: the table of fattn_one.hip)
        const size_t b = (size_t) n->ne[2] * (size_t) n->ne[0] * 4;
        if (b > need) need = b;
    }
    return need;
}
int64_t gemm_group_split_max_cols() {                 // grouped launches (wq / wk / wv) may split K up to this many columns
    static const int64_t v = getenv("MI355X_GROUP_SPLIT_MAX_COLS") ? atoll(getenv("MI355X_GROUP_SPLIT_MAX_COLS")) : 512;
    return v;
}
size_t graph_gemm_partial_need(const ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; ++i) {
        const ggml_tensor * n = g->nodes[i];
        if (n->op != GGML_OP_MUL_MAT || is_empty(n)) continue;
        const mm_route r = route_mul_mat(n);
        if (r.path == MM_GEMM_ANY && n->src[0]->type == GGML_TYPE_F32 && n->src[1]->type == GGML_TYPE_F32) {      // small f32 x f32 products may split K over workgroups (gemm_any.hip)
            const int nbatch = (int) (n->src[1]->ne[2] * n->src[1]->ne[3]);
            size_t b = gemm_any_split_scratch_bytes(n->src[0]->ne[1], n->src[1]->ne[1], n->src[0]->ne[0], nbatch, true);
            if (n->src[0]->op == GGML_OP_RESHAPE && n->src[0]->src[0] && n->src[0]->src[0]->op == GGML_OP_IM2COL) {      // a streaming causal convolution's per-batch-element product: run with the roles swapped, both batch elements in one launch (exec_causal_conv)
                const size_t b2 = gemm_any_split_scratch_bytes(n->src[1]->ne[1], n->src[0]->ne[1], n->src[0]->ne[0], 2, true);
                if (b2 > b) b = b2;
            }
            if (b > need) need = b;
        }
        if (n->src[1]->ne[2] != 1 || n->src[1]->ne[3] != 1) continue;
        if (!r.gemm) {                                       // the k_head form of the any-shape GEMM: its MFMA part is a lone, usually under-filled GEMM
            const size_t b = r.k_head_sized ? gemm_split_scratch_bytes(n->src[0]->ne[1], n->src[1]->ne[1], r.k_head_sized) : 0;
            if (b > need) need = b;
            continue;
        }
        int64_t m_sum = n->src[0]->ne[1];                    // the mat-muls that share this activation may go out as one launch (exec_gemm_group)
        if (n->src[1]->ne[1] <= gemm_group_split_max_cols()) {
            int grouped = 1;
            for (int j = i + 1; j < g->n_nodes && j < i + 32 && grouped < 3; ++j) {
                const ggml_tensor * c = g->nodes[j];
                if (c->op == GGML_OP_MUL_MAT && !is_empty(c) && c->src[1]->data == n->src[1]->data && c->src[1]->ne[0] == n->src[1]->ne[0] && c->src[1]->ne[1] == n->src[1]->ne[1]) { m_sum += c->src[0]->ne[1]; ++grouped; }
            }
        }
        size_t b = gemm_split_scratch_bytes(m_sum, n->src[1]->ne[1], n->src[0]->ne[0]);
        if (r.path == MM_MMQ_TILE) {                         // (its own split rule: one workgroup per CU)
            const size_t b1 = mmq_tile_split_scratch_bytes(n->src[0]->ne[1], n->src[1]->ne[1], n->src[0]->ne[0]), b2 = mmq_tile_split_scratch_bytes(m_sum, n->src[1]->ne[1], n->src[0]->ne[0]);
            if (b1 > b) b = b1;
            if (b2 > b) b = b2;
        }
        if (b > need) need = b;
    }
    return need;
}
void drop_graph_execs(backend_ctx * c) {                   // captured graphs bake pointers / fusion decisions in: destroy, do not just forget
    for (auto & e : c->execs) { if (e.exec) (void) hipGraphExecDestroy(e.exec); if (e.graph) (void) hipGraphDestroy(e.graph); }
    c->execs.clear();
}
bool ensure_scratch(backend_ctx * c, void ** p, size_t * have, size_t need) {
    if (need <= *have) return true;
    HIP_CHECK(hipStreamSynchronize(c->stream));             // nothing in flight may still read the old block
    if (*p) HIP_CHECK(hipFree(*p));
    *p = nullptr; *have = 0;
    size_t n = need + need / 4; n = (n + ((size_t) 1 << 20) - 1) & ~(((size_t) 1 << 20) - 1);
    if (hipMalloc(p, n) != hipSuccess) {                    // the resident F16 weight images are the first thing to give back
        (void) hipGetLastError();
        shadow_drop_all(c->device, c->shadow_hold);
        if (hipMalloc(p, n) != hipSuccess) { (void) hipGetLastError(); *p = nullptr; drop_graph_execs(c); return false; }
    }
    *have = n;
    drop_graph_execs(c);                                    // captured graphs baked the old pointer in
    return true;
}

} // namespace mi
