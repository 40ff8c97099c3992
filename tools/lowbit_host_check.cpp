// tools/lowbit_host_check.cpp -- host-side mirror of the index arithmetic behind the Q4_1 / Q5_1 / Q2_K / Q3_K mat-vec path, run under the
// address and undefined-behaviour sanitizers on the CPU (no GPU, no Python):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/lowbit_host_check.cpp -o /tmp/lowbit_host_check && /tmp/lowbit_host_check
// It allocates every buffer at exactly the size the library allocates and touches every byte range the kernels touch:
//   * the Q8_1 image (q81_image_bytes): the quantiser's stores (k_quantize_q81) and the loads of q41_form (k_mmv_blocks, mmvq.hip) for every block of every column;
//   * the Q8_K image as q2k_form / q3k_form read it (qs, the bsums vector of a half, d);
//   * a weight matrix of nrows rows: the frame's clamped block index and row with the per-lane loads of the four forms, last block of the last row included.
#include "../llama.cpp-omni_amd/csrc/common.hpp"
#include <cstring>
#include <vector>

static unsigned long long g_sum = 0;
static void touch(const std::vector<unsigned char> & b, size_t off, size_t n) {          // a load of n bytes at off
    for (size_t i = 0; i < n; ++i) g_sum += b.data()[off + i];
}

static void check_q81_image(int64_t K, int ncols) {
    const size_t img = q81_image_bytes(K);
    const int64_t nb = K / 32;
    if (img % 16 != 0 || img < (size_t) (K + 8 * nb)) { fprintf(stderr, "q81_image_bytes(%lld) = %zu\n", (long long) K, img); exit(1); }
    std::vector<unsigned char> act((size_t) ncols * img, 0);
    for (int c = 0; c < ncols; ++c) {
        unsigned char * im = act.data() + (size_t) c * img;
        for (int64_t ib = 0; ib < nb; ++ib) {                                            // k_quantize_q81
            memset(im + ib * 32, 1, 32);
            const float d = 1.0f, s = 2.0f;
            memcpy(im + K + ib * 4, &d, 4);
            memcpy(im + K + (nb + ib) * 4, &s, 4);
        }
        for (int64_t ib = 0; ib < nb; ++ib)                                              // q41_form::read, both lane halves
            for (int hf = 0; hf < 2; ++hf) {
                touch(act, (size_t) c * img + ib * 32 + 8 * hf, 8); touch(act, (size_t) c * img + ib * 32 + 16 + 8 * hf, 8);
                touch(act, (size_t) c * img + K + ib * 4, 4);       touch(act, (size_t) c * img + K + (nb + ib) * 4, 4);
            }
    }
}

static void check_q8k_reads(int64_t K, int ncols) {
    const size_t img = q8k_image_bytes(K);
    const int64_t nb = K / 256;
    std::vector<unsigned char> act((size_t) ncols * img, 0);
    for (int c = 0; c < ncols; ++c)
        for (int64_t ib = 0; ib < nb; ++ib)
            for (int qq = 0; qq < 4; ++qq) {
                const int n = qq >> 1, sub = qq & 1;
                for (int j = 0; j < 4; ++j) touch(act, (size_t) c * img + ib * 256 + 128 * n + 32 * j + 16 * sub, 16);
                touch(act, (size_t) c * img + K + ib * 32 + 16 * n, 16);
                touch(act, (size_t) c * img + K + K / 8 + ib * 4, 4);
            }
}

// the per-lane weight loads of one wave step, block index and row clamped as the kernels clamp them
static void check_weight_loads(int64_t K, int64_t nrows, int rows_per_wave) {
    struct fmt { int blk, bytes; } F[4] = { { 32, 20 }, { 32, 24 }, { 256, 84 }, { 256, 110 } };
    for (int f = 0; f < 4; ++f) {
        if (K % F[f].blk) continue;
        const int64_t nb = K / F[f].blk;
        const size_t rs = (size_t) nb * F[f].bytes;
        std::vector<unsigned char> W((size_t) nrows * rs, 0);
        const int lanes_per_block = f < 2 ? 2 : 4, blocks_per_step = 64 / lanes_per_block;
        const int64_t nit = (nb + blocks_per_step - 1) / blocks_per_step, ngrp = (nrows + rows_per_wave - 1) / rows_per_wave;
        for (int64_t grp = 0; grp < ngrp; ++grp)
            for (int64_t it = 0; it < nit; ++it)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < rows_per_wave; ++r) {
                        int64_t ib = it * blocks_per_step + lane / lanes_per_block; ib = ib < nb ? ib : nb - 1;
                        int64_t row = grp * rows_per_wave + r; row = row < nrows ? row : nrows - 1;
                        const size_t bp = (size_t) row * rs + (size_t) ib * F[f].bytes;
                        const int sel = lane % lanes_per_block;
                        if (f == 0)      { touch(W, bp, 4); touch(W, bp + 4 + 8 * sel, 8); }
                        else if (f == 1) { touch(W, bp, 4); touch(W, bp + 4, 4); touch(W, bp + 8 + 8 * sel, 8); }
                        else if (f == 2) { touch(W, bp + 8 * (sel >> 1), 8); touch(W, bp + 16 + 16 * sel, 16); touch(W, bp + 80, 4); }
                        else             { touch(W, bp + 16 * (sel & 1), 16); touch(W, bp + 32 + 16 * sel, 16); touch(W, bp + 94, 16); }
                    }
    }
}

int main() {
    const int64_t Ks[] = { 32, 96, 128, 256, 512, 768, 1024, 4096, 12288 };
    for (int64_t K : Ks)
        for (int ncols = 1; ncols <= 8; ++ncols) {
            check_q81_image(K, ncols);
            if (K % 256 == 0) check_q8k_reads(K, ncols);
        }
    const int64_t Ms[] = { 1, 2, 3, 37, 40, 257 };
    for (int64_t K : Ks)
        for (int64_t M : Ms) { check_weight_loads(K, M, 1); check_weight_loads(K, M, 2); }
    printf("lowbit_host_check: ok (%llu)\n", g_sum);
    return 0;
}
