// argsort.hip -- ARGSORT of f32 rows -> i32 indices, both orders (gfx950 / wave64).
//
// What is computed (reference: ggml_compute_forward_argsort_f32, ggml-cpu/ops.cpp:7853-7890): dst[row][r] = index of the r-th smallest (ASC) / largest (DESC)
// element of the row.  ggml_top_k is this node (DESC) plus a view of the first k columns: the expert selection of a mixture-of-experts layer.
//
// TIES: the reference's exchange sort is not stable, so equal values come out in an order its loop structure happens to give.  Here the order is total and
// fixed: of two equal values the LOWER INDEX comes first, in either order.  (The reference's own test_argsort uses distinct values for the same reason.)
//
// One workgroup per row, grid-strided over the rows.  The row's (value, index) pairs sit in LDS, padded to the next power of two; a bitonic network sorts
// them.  Padding slots carry an index >= ne0 and sort behind every real element in either order, so the first ne0 slots of the result are the answer.
// Every __syncthreads is reached by every thread of the workgroup: the network's trip counts depend on ne0 alone, the row loop's on blockIdx alone.
// LDS: 8 bytes per padded slot, so ne0 <= 16384 (128 KiB) under the 152 KiB rule; supports_op refuses longer rows (argsort_ok).
#include "../kernels.hpp"

namespace mi {

extern __shared__ __attribute__((aligned(16))) char argsort_lds[];

// does a sort in front of b?  (a strict total order: no two slots compare equal)
template <bool DESC>
static __device__ __forceinline__ bool as_before(float va, int ia, float vb, int ib, int n) {
    const bool pa = ia >= n, pb = ib >= n;
    if (pa || pb) return pa == pb ? ia < ib : pb;
    if (va != vb) return DESC ? va > vb : va < vb;
    return ia < ib;
}

template <bool DESC>
__global__ void __launch_bounds__(1024) k_argsort(const char * __restrict__ x, size_t nb1, size_t nb2, size_t nb3, int * __restrict__ dst,
                                                   int n, int npad, int ne1, int ne2, long long nrows) {
    float * val = (float *) argsort_lds;
    int *   idx = (int *) (argsort_lds + (size_t) npad * 4);
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const long long i3 = row / ((long long) ne1 * ne2), i2 = (row / ne1) % ne2, i1 = row % ne1;
        const float * src = (const float *) (x + i1 * nb1 + i2 * nb2 + i3 * nb3);
        for (int i = threadIdx.x; i < npad; i += blockDim.x) { val[i] = i < n ? src[i] : 0.0f; idx[i] = i; }
        __syncthreads();
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = threadIdx.x; t < (npad >> 1); t += blockDim.x) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;      // lo has bit j clear; both < npad
                    const float vl = val[lo], vh = val[hi]; const int il = idx[lo], ih = idx[hi];
                    const bool up = (lo & k) == 0;
                    const bool swap = up ? as_before<DESC>(vh, ih, vl, il, n) : as_before<DESC>(vl, il, vh, ih, n);
                    if (swap) { val[lo] = vh; val[hi] = vl; idx[lo] = ih; idx[hi] = il; }
                }
                __syncthreads();
            }
        }
        int * out = dst + row * (long long) n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = idx[i];
        __syncthreads();                                     // the next row overwrites the slots
    }
}

static long g_argsort_launches = 0;
long argsort_launches() { return g_argsort_launches; }

static const size_t ARGSORT_LDS_MAX = 152 * 1024;
static int64_t argsort_pad(int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }
bool argsort_ok(int64_t ne0) { return ne0 >= 1 && ne0 < ((int64_t) 1 << 30) && (size_t) argsort_pad(ne0) * 8 <= ARGSORT_LDS_MAX; }

void argsort_f32(const tdesc & x, int * dst, bool desc, hipStream_t st) {
    const int64_t n = x.ne[0], nrows = x.ne[1] * x.ne[2] * x.ne[3];
    if (n == 0 || nrows == 0) return;
    if (!argsort_ok(n)) { fprintf(stderr, "[mi355x] argsort_f32: a row of %lld elements does not fit one workgroup's LDS\n", (long long) n); abort(); }
    const int64_t npad = argsort_pad(n);
    const size_t lds = (size_t) npad * 8;
    int threads = (int) (npad / 2); threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
    const unsigned grid = (unsigned) (nrows < 8192 ? nrows : 8192);
    auto go = [&](auto kern) {
        if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        kern<<<dim3(grid), dim3(threads), lds, st>>>((const char *) x.p, x.nb[1], x.nb[2], x.nb[3], dst, (int) n, (int) npad, (int) x.ne[1], (int) x.ne[2], (long long) nrows);
    };
    if (desc) go(k_argsort<true>); else go(k_argsort<false>);
    ++g_argsort_launches;
}

} // namespace mi
