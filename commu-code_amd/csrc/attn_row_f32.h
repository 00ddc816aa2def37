// ONE fp32 attention row (reference model.py:283-345), shared by every fp32 attention forward: the parity prefill and the
// linear-cache decode step (relattn_f32_kernel), the ring decode step (decode_attn_ring_f32_kernel), both in
// parity_f32.hip, and the training forward (relattn_fwd_f32_kernel, train_f32.hip).  The kernels differ in where the window
// [lo, hi] comes from and where key j's K / V row lives; the arithmetic -- and so every bit of the result -- is this file's.
// Also here: what the backward kernels of train_f32.hip share with the forward (the visible window, the keep decision of
// the attention dropout, the lane broadcast).
#pragma once
#include "common.h"
#include "attn_drop.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(4))) float f4;

// first visible key of query i among M memory + T new keys (model.py:549-574: causal; same_length hides keys j <= i - s;
// a reset sequence does not see the memory).  The last visible key is i + M.
__device__ __forceinline__ int vis_lo(int same_length, int T, int M, int mem_len, int i, bool rst) {
    int lo = 0;
    if (same_length) {
        const int mask_len = M + T - mem_len;
        const int s = mask_len > 0 ? T - mask_len : T;
        lo = max(0, i - s + 1);
    }
    if (rst && lo < M) lo = M;
    return lo;
}

// keep decision of element (i, j) of (b, h): the DropLane word of that element (lane r16 = j & 15, row 4 g + reg = i & 15)
__device__ __forceinline__ bool att_keep(unsigned seed, unsigned thr_hi, int H, int b, int h, int i, int j) {
    DropLane dl;
    dl.init(seed, b, h, H, (i & 15) >> 2, j & 15);
    unsigned hw[4];
    dl.words(i >> 4, j >> 4, hw);
    return hw[i & 3] >= thr_hi;
}

// (v_readlane reads lane l's value whatever the EXEC mask: with d_head < 64 the lanes that own the keys d_head .. 63 of a
//  chunk are not among the feature lanes of the P . V loop)
__device__ __forceinline__ float rl(float x, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}

// Where key j's K / V row lives: row(j) for the lane that owns key j, next(r) for the walk over a chunk's rows in P . V.
struct RowsLinear {          // projection buffer / linear cache: key j in row j
    __device__ __forceinline__ int row(int j) const { return j; }
    __device__ __forceinline__ int next(int r) const { return r + 1; }
};
struct RowsRing {            // ring of W rows: positions >= wrap in row p - wrap, older ones in row p - wrap + W
    int wrap, W;
    __device__ __forceinline__ int row(int j) const { return j >= wrap ? j - wrap : j - wrap + W; }
    __device__ __forceinline__ int next(int r) const { return r + 1 == W ? 0 : r + 1; }
};

// One wave, one query of head h of sequence b (every pointer already at that head; q = the query's row, kb / vb0 = row 0 of
// the sequence's keys / values, row pitch sj, rd0 = the distance table's row 0; key j has distance hi - j):
//   s_j = ((q + u) . k_j + (q + vbias) . Rd[hi - j]) * scale for lo <= j <= hi,  P = softmax_j(s),
//   DROP: attention dropout on P (keep decision of (i, j); the normaliser stays undropped; the caller applies 1 / (1 - p)).
// Keys in chunks of 64: a lane owns a key, its two dot products run over d in order; online softmax across chunks; P . V
// with a lane per feature.  Returns feature `lane` of the normalised output (lanes < DH; 0 for an empty window) and
// lse = log-sum-exp of the undropped scores (0 for an empty window).
template <int VW, bool DROP, class Rows>
__device__ __forceinline__ float attn_row_f32(const float* __restrict__ q, const float* __restrict__ u,
                                              const float* __restrict__ vbias, const float* __restrict__ kb,
                                              const float* __restrict__ vb0, size_t sj, const Rows rows,
                                              const float* __restrict__ rd0, int ld_rd, int lo, int hi, int DH, float scale,
                                              unsigned drop_seed, unsigned drop_thr_hi, int H, int b, int h, int i, float& lse) {
    __shared__ __attribute__((aligned(16))) float qu[64], qv[64];
    const int lane = threadIdx.x;
    if (lane < DH) {
        const float x = q[lane];
        qu[lane] = x + u[lane];
        qv[lane] = x + vbias[lane];
    }
    __syncthreads();
    float mrun = -INFINITY, lrun = 0.f, acc = 0.f;
    for (int j0 = lo; j0 <= hi; j0 += 64) {
        const int j = j0 + lane;
        float s = -INFINITY;
        if (j <= hi) {          // (ONE loop for both chains: the compiler pairs them into packed fp32 FMAs)
            const float* kr = kb + (size_t)rows.row(j) * sj;
            const float* rr = rd0 + (size_t)(hi - j) * ld_rd;
            float ac = 0.f, bd = 0.f;
            if (VW == 4) {
                for (int d = 0; d < DH; d += 4) {
                    const f4 kx = *(const f4*)(kr + d), rx = *(const f4*)(rr + d);
                    ac = fmaf(qu[d], kx.x, ac); ac = fmaf(qu[d + 1], kx.y, ac); ac = fmaf(qu[d + 2], kx.z, ac); ac = fmaf(qu[d + 3], kx.w, ac);
                    bd = fmaf(qv[d], rx.x, bd); bd = fmaf(qv[d + 1], rx.y, bd); bd = fmaf(qv[d + 2], rx.z, bd); bd = fmaf(qv[d + 3], rx.w, bd);
                }
            } else {
                for (int d = 0; d < DH; ++d) {
                    ac = fmaf(qu[d], kr[d], ac);
                    bd = fmaf(qv[d], rr[d], bd);
                }
            }
            s = (ac + bd) * scale;
        }
        const float mnew = fmaxf(mrun, wave_max(s));
        float p = (j <= hi) ? expf(s - mnew) : 0.f;
        const float corr = (mrun == -INFINITY) ? 0.f : expf(mrun - mnew);
        lrun = lrun * corr + wave_sum(p);          // the normaliser: undropped
        if (DROP && drop_thr_hi && j <= hi && !att_keep(drop_seed, drop_thr_hi, H, b, h, i, j)) p = 0.f;
        acc *= corr;
        const int n = min(64, hi - j0 + 1);
        if (lane < DH) {
            int r = rows.row(j0);
            for (int jj = 0; jj < n; ++jj) {
                acc = fmaf(rl(p, jj), vb0[(size_t)r * sj + lane], acc);
                r = rows.next(r);
            }
        }
        mrun = mnew;
    }
    const bool any = hi >= lo;
    lse = any ? mrun + logf(lrun) : 0.f;
    return any ? acc / lrun : 0.f;
}

}  // namespace
