// fp32 TRAINING MODE (model.fp32_training) and the kernels every fp32 forward shares with it.
//
// The reference trains in fp32 (train.py:48 `amp = None`; train.py:139-169).  This translation unit holds the general fp32
// GEMM (NT / NN / TN, epilogues, deterministic row split: the 64 x 64 tile behind every fp32 Linear, commu_gemm_nt_f32 of
// parity_f32.hip included), LayerNorm forward (statistics optional: the parity forward and the decode step call it without)
// and backward, the relative attention's training forward (attn_row_f32.h with attention dropout on, log-sum-exp out) and
// its backward in three passes, the cross-entropy backward, the embedding backward and an element-wise dropout /
// ReLU-gate kernel.  parity_f32.hip holds what only the generation path needs.
// Rules of every product here: exact fp32 products with fp32 accumulation (v_mfma_f32_16x16x4_f32 or fmaf chains), accurate
// expf / logf, and NO floating-point atomics -- every output element has one writer that sums in a fixed order, so two
// identical passes give bitwise-identical gradients.  Dropout masks are the build's counter-based ones (common.h drop_word,
// attn_drop.h DropLane): the same keep decisions as the bf16 path for the same seeds.
#include "common.h"
#include "commu_hip.h"
#include "attn_row_f32.h"

namespace {

// ------------------------------------------------------------------------------------------------ GEMM
// C[M,N] (+)= op(A)[M,K] . op(B)[K,N] with op(A) = A ([M][K], TA 0) or A^T (A stored [K][M], TA 1) and op(B) = B^T (B stored
// [N][K], TB 1: the nn.Linear form) or B (stored [K][N], TB 0).  NT = Linear forward, NN = dX, TN = dW.
// 64 x 64 tile, 4 waves (each 32 x 32 = 2 x 2 v_mfma_f32_16x16x4_f32 tiles of 16 x 16), K step 16.
#define TG_BM 64
#define TG_BN 64
#define TG_BK 16
#define TG_LD 80          // LDS row pitch in floats: k rows 0 / 1 of a 32-lane read land in banks 0-15 / 16-31

struct GemmEpi {
    const float* bias;          // [N] or null
    const float* resid;         // [M][ldr] or null
    int ldr;
    int relu;
    unsigned drop_seed, drop_thr;   // dropout on the (bias + ReLU) value: element index row * N + col; thr 0: off
    float drop_scale;
    int accumulate;             // C += result
};

// One 64-row x 16-k tile of an operand into S[k][row], zero outside [rows) x [kend).
// Stored [row][k] (row-major): thread (tid >> 2, 4 (tid & 3)) takes 4 consecutive k of one row -- into registers BEFORE the
// barrier that frees the LDS tile (load_rows: the global latency overlaps the previous step's MFMAs), one 16-byte load when
// VEC (leading dimension % 4 == 0 and a 16-byte aligned base: the launcher checks) --, then store_rows.  load_rows takes
// both operands (RA / RB: which of them are row-major) under ONE branch, so that their loads are in flight together.
template <bool RA, bool RB, bool VEC>
__device__ __forceinline__ void load_rows(const float* __restrict__ ap, bool aok, const float* __restrict__ bp, bool bok, int k0,
                                          int kend, int tid, float (&av)[4], float (&bv)[4]) {
    const int kk = k0 + (tid & 3) * 4;
    if (VEC && kk + 3 < kend) {
        if (RA) {
            const f4 x = *(const f4*)(ap + kk);
            av[0] = x.x; av[1] = x.y; av[2] = x.z; av[3] = x.w;
        }
        if (RB) {
            const f4 y = *(const f4*)(bp + kk);
            bv[0] = y.x; bv[1] = y.y; bv[2] = y.z; bv[3] = y.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (RA) av[e] = (kk + e < kend) ? ap[kk + e] : 0.f;
            if (RB) bv[e] = (kk + e < kend) ? bp[kk + e] : 0.f;
        }
    }
    if (RA && !aok) av[0] = av[1] = av[2] = av[3] = 0.f;
    if (RB && !bok) bv[0] = bv[1] = bv[2] = bv[3] = 0.f;
}

__device__ __forceinline__ void store_rows(const float (&x)[4], int tid, float (*S)[TG_LD]) {
    const int r = tid >> 2, kk = (tid & 3) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) S[kk + e][r] = x[e];
}

// Stored [k][row] (transposed): 4 consecutive rows of one k, straight into LDS.
__device__ __forceinline__ void stage_cols(const float* __restrict__ X, int ldx, int r0, int rows, int k0, int kend, int tid,
                                           float (*S)[TG_LD]) {
    const int kk = tid >> 4, r = (tid & 15) * 4;
    const int k = k0 + kk;
    const bool kok = k < kend;
    const float* p = X + (size_t)(kok ? k : 0) * ldx;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int rr = r0 + r + e;
        S[kk][r + e] = (kok && rr < rows) ? p[rr] : 0.f;
    }
}

// gridDim.z > 1: slab z sums k in [z * kchunk, (z + 1) * kchunk) into C + z * slab_stride, no epilogue (the caller reduces
// the slabs in order)
// EPI: the training epilogue (dropout, accumulate, slabs) is compiled in; the plain Linear (bias, ReLU, residual) runs without
// and ignores kchunk / slab_stride (one slab: k in [0, K), C itself)
template <int TA, int TB, bool VEC, bool EPI = true>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                       float* __restrict__ C, int ldc, long long slab_stride, int M, int N, int K,
                                                       int kchunk, GemmEpi e) {
    __shared__ float As[TG_BK][TG_LD];
    __shared__ float Bs[TG_BK][TG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * TG_BM, n0 = blockIdx.x * TG_BN;
    const int kbeg = EPI ? blockIdx.z * kchunk : 0, kend = EPI ? min(K, kbeg + kchunk) : K;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the row of each row-major operand that this thread stages (row 0 where the tile ends: read, then zeroed)
    const int am = m0 + (tid >> 2), bn = n0 + (tid >> 2);
    const float* ap = A + (size_t)(TA == 0 && am < M ? am : 0) * lda;
    const float* bp = B + (size_t)(TB == 1 && bn < N ? bn : 0) * ldb;
    for (int k0 = kbeg; k0 < kend; k0 += TG_BK) {
        float av[4], bv[4];
        load_rows<TA == 0, TB == 1, VEC>(ap, am < M, bp, bn < N, k0, kend, tid, av, bv);
        __syncthreads();          // the previous step's fragment reads are done
        if (TA == 0) store_rows(av, tid, As); else stage_cols(A, lda, m0, M, k0, kend, tid, As);
        if (TB == 1) store_rows(bv, tid, Bs); else stage_cols(B, ldb, n0, N, k0, kend, tid, Bs);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < TG_BK; ks += 4) {
            const int kr = ks + (lane >> 4), c = lane & 15;
            const float a0 = As[kr][wm + c], a1 = As[kr][wm + 16 + c];
            const float b0 = Bs[kr][wn + c], b1 = Bs[kr][wn + 16 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    const bool slab = EPI && gridDim.z > 1;
    float* Cz = EPI ? C + (size_t)blockIdx.z * slab_stride : C;
    DropKey dk{0u, 0u};
    if (EPI && e.drop_thr) dk = drop_key(e.drop_seed);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = n0 + wn + 16 * b + (lane & 15);
            if (col >= N) continue;
            const float bs = (!slab && e.bias) ? e.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + 16 * a + 4 * (lane >> 4) + r;
                if (row >= M) continue;
                float v = acc[a][b][r];
                float* dst = Cz + (size_t)row * ldc + col;
                if (!slab) {
                    v += bs;
                    if (e.relu) v = fmaxf(v, 0.f);
                    if (EPI && e.drop_thr) v = drop_keep(dk, (unsigned)row * (unsigned)N + (unsigned)col, e.drop_thr) ? v * e.drop_scale : 0.f;
                    if (e.resid) v += e.resid[(size_t)row * e.ldr + col];
                    if (EPI && e.accumulate) v += *dst;
                }
                *dst = v;
            }
        }
}

// ------------------------------------------------------------------------------------------------ attention
// reference model.py:283-345 for (query i, key j) of sequence b, head h:
//   s_ij = ((q_i + u) . k_j + (q_i + v) . Rd[i + M - j]) * scale,  visible keys lo_i <= j <= i + M,
//   P = softmax_j(s), attention dropout on P (DropLane mask), out_i = sum_j P_ij keep_ij / (1 - p) v_j.
struct AttF32 {
    const float *q, *k, *v, *rd, *u, *vb;
    const unsigned char* reset;
    const float *o, *dout, *lse_in;
    float *out, *lse, *delta, *dq, *dq_ac, *dq_bd, *dk, *dv, *drd;
    int ld_q, ld_kv, ld_rd, ld_o, ld_do, ld_dq, ld_dkv, ld_drd;
    int T, M, B, H, DH, same_length, mem_len;
    float scale;
    unsigned drop_seed, drop_thr_hi;
    float drop_scale;
};

// first visible key of query i (attn_row_f32.h: one definition for forward and backward)
__device__ __forceinline__ int vis_lo(const AttF32& a, int i, bool rst) { return vis_lo(a.same_length, a.T, a.M, a.mem_len, i, rst); }

// forward: one wave per (h, b, i) runs attn_row_f32 over the projection buffer with the attention dropout on.  Writes out
// and lse[(b H + h) T + i] = log-sum-exp of the UNDROPPED scores.
// (5 waves per SIMD: the register budget the kernel has always had; the mask's hash state sits on top of the row's registers)
template <int VW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void relattn_fwd_f32_kernel(const AttF32 a) {
    const int h = blockIdx.x, b = blockIdx.y, i = blockIdx.z, lane = threadIdx.x, DH = a.DH, B = a.B;
    const size_t hd = (size_t)h * DH;
    float lse;
    const float o = attn_row_f32<VW, true>(a.q + ((size_t)i * B + b) * a.ld_q + hd, a.u + hd, a.vb + hd, a.k + (size_t)b * a.ld_kv + hd,
                                           a.v + (size_t)b * a.ld_kv + hd, (size_t)B * a.ld_kv, RowsLinear{}, a.rd + hd, a.ld_rd,
                                           vis_lo(a, i, a.reset && a.reset[b]), i + a.M, DH, a.scale, a.drop_seed, a.drop_thr_hi,
                                           a.H, b, h, i, lse);
    if (lane < DH) a.out[((size_t)i * B + b) * a.ld_o + hd + lane] = o * a.drop_scale;
    if (lane == 0) a.lse[((size_t)b * a.H + h) * a.T + i] = lse;
}

// sum_d (x[d] (+ xb[d])) * y[d], d in order (the sequence of fmaf of the forward, attn_row_f32.h: every pass
// recomputes the same score)
template <int VW>
__device__ __forceinline__ float dotp(const float* __restrict__ x, const float* __restrict__ xb, const float* __restrict__ y, int DH) {
    float s = 0.f;
    if (VW == 4) {
        for (int d = 0; d < DH; d += 4) {
            f4 xv = *(const f4*)(x + d);
            if (xb) xv += *(const f4*)(xb + d);
            const f4 yv = *(const f4*)(y + d);
            s = fmaf(xv.x, yv.x, s); s = fmaf(xv.y, yv.y, s); s = fmaf(xv.z, yv.z, s); s = fmaf(xv.w, yv.w, s);
        }
    } else {
        for (int d = 0; d < DH; ++d) s = fmaf(xb ? x[d] + xb[d] : x[d], y[d], s);
    }
    return s;
}

// dS_ij * scale of a visible (i, j) from the recomputed score: P = exp(s - lse_i), dP = keep / (1 - p) dO_i . v_j,
// dS = P (dP - delta_i) with delta_i = dO_i . O_i (that holds with dropout too).  pdrop = the dropped probability.
template <int VW>
__device__ __forceinline__ float att_ds(const AttF32& a, int b, int h, int i, int j, const float* qrow, const float* krow,
                                        const float* rrow, const float* dorow, const float* vrow, float& pdrop) {
    const int DH = a.DH;
    const float s = (dotp<VW>(qrow, a.u + h * DH, krow, DH) + dotp<VW>(qrow, a.vb + h * DH, rrow, DH)) * a.scale;
    const size_t r = ((size_t)b * a.H + h) * a.T + i;
    const float p = expf(s - a.lse_in[r]);
    float dp = dotp<VW>(dorow, nullptr, vrow, DH);
    pdrop = p;
    if (a.drop_thr_hi) {
        const bool keep = att_keep(a.drop_seed, a.drop_thr_hi, a.H, b, h, i, j);
        dp = keep ? dp * a.drop_scale : 0.f;
        pdrop = keep ? p * a.drop_scale : 0.f;
    }
    return p * (dp - a.delta[r]) * a.scale;
}

// backward pass 0: delta_i = dO_i . O_i (one wave per (h, b, i))
__global__ __launch_bounds__(64) void relattn_delta_f32_kernel(const AttF32 a) {
    const int h = blockIdx.x, b = blockIdx.y, i = blockIdx.z, lane = threadIdx.x, DH = a.DH;
    float x = 0.f;
    if (lane < DH)
        x = a.dout[((size_t)i * a.B + b) * a.ld_do + (size_t)h * DH + lane] * a.o[((size_t)i * a.B + b) * a.ld_o + (size_t)h * DH + lane];
    x = wave_sum(x);
    if (lane == 0) a.delta[((size_t)b * a.H + h) * a.T + i] = x;
}

// backward pass 1, query-stationary (one wave per (h, b, i)): dq_AC_i = sum_j dS_ij k_j, dq_BD_i = sum_j dS_ij Rd[i + M - j]
// (scale included), dq = their sum.  A lane owns a key of each chunk; the contraction runs with a lane per feature.
template <int VW>
__global__ __launch_bounds__(64) void relattn_bwd_q_f32_kernel(const AttF32 a) {
    const int h = blockIdx.x, b = blockIdx.y, i = blockIdx.z, lane = threadIdx.x, DH = a.DH, B = a.B;
    const int lo = vis_lo(a, i, a.reset && a.reset[b]), hi = i + a.M;
    const size_t sj = (size_t)B * a.ld_kv;
    const float* qrow = a.q + ((size_t)i * B + b) * a.ld_q + (size_t)h * DH;
    const float* dorow = a.dout + ((size_t)i * B + b) * a.ld_do + (size_t)h * DH;
    const float* kb = a.k + (size_t)b * a.ld_kv + (size_t)h * DH;
    const float* vb_ = a.v + (size_t)b * a.ld_kv + (size_t)h * DH;
    const float* rdh = a.rd + (size_t)h * DH;
    float acc_ac = 0.f, acc_bd = 0.f;
    for (int j0 = lo; j0 <= hi; j0 += 64) {
        const int j = j0 + lane;
        float ds = 0.f, pd;
        if (j <= hi) ds = att_ds<VW>(a, b, h, i, j, qrow, kb + j * sj, rdh + (size_t)(i + a.M - j) * a.ld_rd, dorow, vb_ + j * sj, pd);
        const int n = min(64, hi - j0 + 1);
        if (lane < DH) {
            for (int jj = 0; jj < n; ++jj) {
                const float w = rl(ds, jj);
                acc_ac = fmaf(w, kb[(size_t)(j0 + jj) * sj + lane], acc_ac);
                acc_bd = fmaf(w, rdh[(size_t)(i + a.M - j0 - jj) * a.ld_rd + lane], acc_bd);
            }
        }
    }
    if (lane < DH) {
        const size_t row = (size_t)i * B + b, c = (size_t)h * DH + lane, HD = (size_t)a.H * DH;
        a.dq_ac[row * HD + c] = acc_ac;
        a.dq_bd[row * HD + c] = acc_bd;
        a.dq[row * a.ld_dq + c] = acc_ac + acc_bd;
    }
}

// backward pass 2, key-stationary (one wave per (h, b, j), j over ALL K keys, memory rows included):
// dv_j = sum_i P_ij keep / (1 - p) dO_i, dk_j = sum_i dS_ij (q_i + u).  A lane owns a query of each chunk.
template <int VW>
__global__ __launch_bounds__(64) void relattn_bwd_kv_f32_kernel(const AttF32 a) {
    __shared__ __attribute__((aligned(16))) float kj[64], vj[64];
    const int h = blockIdx.x, b = blockIdx.y, j = blockIdx.z, lane = threadIdx.x, DH = a.DH, B = a.B;
    const size_t rowj = ((size_t)j * B + b) * a.ld_kv + (size_t)h * DH;
    if (lane < DH) {
        kj[lane] = a.k[rowj + lane];
        vj[lane] = a.v[rowj + lane];
    }
    __syncthreads();
    const bool rst = a.reset && a.reset[b];
    const float* ub = a.u + h * DH;
    float acc_k = 0.f, acc_v = 0.f;
    for (int i0 = max(0, j - a.M); i0 < a.T; i0 += 64) {
        const int i = i0 + lane;
        float ds = 0.f, pd = 0.f;
        if (i < a.T && j >= vis_lo(a, i, rst)) {          // (j <= i + M: i >= j - M)
            const size_t ri = (size_t)i * B + b;
            ds = att_ds<VW>(a, b, h, i, j, a.q + ri * a.ld_q + (size_t)h * DH, kj, a.rd + (size_t)(i + a.M - j) * a.ld_rd + (size_t)h * DH,
                            a.dout + ri * a.ld_do + (size_t)h * DH, vj, pd);
        }
        const int n = min(64, a.T - i0);
        if (lane < DH) {
            for (int ii = 0; ii < n; ++ii) {
                const size_t ri = (size_t)(i0 + ii) * B + b;
                acc_v = fmaf(rl(pd, ii), a.dout[ri * a.ld_do + (size_t)h * DH + lane], acc_v);
                acc_k = fmaf(rl(ds, ii), a.q[ri * a.ld_q + (size_t)h * DH + lane] + ub[lane], acc_k);
            }
        }
    }
    if (lane < DH) {
        const size_t o = ((size_t)j * B + b) * a.ld_dkv + (size_t)h * DH + lane;
        a.dk[o] = acc_k;
        a.dv[o] = acc_v;
    }
}

// backward pass 3, distance-stationary (one wave per (h, d)): dRd[d] = sum_{b, i} dS[i, i + M - d] (q_i + r_r_bias), the
// sequences in order, the queries of each in order.
template <int VW>
__global__ __launch_bounds__(64) void relattn_bwd_rd_f32_kernel(const AttF32 a) {
    __shared__ __attribute__((aligned(16))) float rdd[64];
    const int h = blockIdx.x, d = blockIdx.y, lane = threadIdx.x, DH = a.DH, B = a.B;
    if (lane < DH) rdd[lane] = a.rd[(size_t)d * a.ld_rd + (size_t)h * DH + lane];
    __syncthreads();
    const float* vbh = a.vb + h * DH;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        const bool rst = a.reset && a.reset[b];
        for (int i0 = max(0, d - a.M); i0 < a.T; i0 += 64) {
            const int i = i0 + lane;
            float ds = 0.f, pd;
            if (i < a.T) {
                const int j = i + a.M - d;          // 0 <= j <= i + M
                if (j >= vis_lo(a, i, rst)) {
                    const size_t ri = (size_t)i * B + b, rj = (size_t)j * B + b;
                    ds = att_ds<VW>(a, b, h, i, j, a.q + ri * a.ld_q + (size_t)h * DH, a.k + rj * a.ld_kv + (size_t)h * DH, rdd,
                                    a.dout + ri * a.ld_do + (size_t)h * DH, a.v + rj * a.ld_kv + (size_t)h * DH, pd);
                }
            }
            const int n = min(64, a.T - i0);
            if (lane < DH)
                for (int ii = 0; ii < n; ++ii)
                    acc = fmaf(rl(ds, ii), a.q[((size_t)(i0 + ii) * B + b) * a.ld_q + (size_t)h * DH + lane] + vbh[lane], acc);
        }
    }
    if (lane < DH) a.drd[(size_t)d * a.ld_drd + (size_t)h * DH + lane] = acc;
}

// ------------------------------------------------------------------------------------------------ LayerNorm
// nn.LayerNorm (model.py:179,352): biased variance, eps inside the root; one wave per row (D <= 1024), two passes over
// registers; STATS: mean / rstd saved for the backward
template <bool STATS>
__global__ __launch_bounds__(256) void layernorm_fwd_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ g,
                                                                const float* __restrict__ bt, float* __restrict__ y, int ldy,
                                                                float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                                int rows, int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * ldx;
    float v[16];          // D <= 1024
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = lane + 64 * e;
        v[e] = c < D ? xr[c] : 0.f;
        s += v[e];
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = lane + 64 * e;
        const float t = c < D ? v[e] - mean : 0.f;
        q += t * t;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = lane + 64 * e;
        if (c < D) y[(size_t)row * ldy + c] = (v[e] - mean) * rstd * g[c] + bt[c];
    }
    if (STATS && lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }
}

// dz = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), dy = dy (+ add); block k takes rows [k rpb, (k + 1) rpb) (its four
// waves every fourth row) and writes its partial dgamma = sum dy xhat, dbeta = sum dy to part[k] / part[nblk + k]
__global__ __launch_bounds__(256) void layernorm_bwd_f32_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ add,
                                                                int ldadd, const float* __restrict__ x, int ldx,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ g, float* __restrict__ dx, int lddx,
                                                                float* __restrict__ part, int nblk, int rows, int D, int rpb) {
    __shared__ float red[4][2][1024];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float pg[16], pb[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) pg[e] = pb[e] = 0.f;
    const int r0 = blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
    for (int row = r0 + w; row < r1; row += 4) {
        const float mu = mean[row], rs = rstd[row];
        float t[16], xh[16];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = lane + 64 * e;
            float d = 0.f, xv = 0.f, gd = 0.f;
            if (c < D) {
                d = dy[(size_t)row * lddy + c];
                if (add) d += add[(size_t)row * ldadd + c];
                xv = (x[(size_t)row * ldx + c] - mu) * rs;
                gd = g[c] * d;
            }
            t[e] = gd;
            xh[e] = xv;
            s1 += gd;
            s2 += gd * xv;
            pg[e] += d * xv;
            pb[e] += d;
        }
        s1 = wave_sum(s1) / (float)D;
        s2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = lane + 64 * e;
            if (c < D) dx[(size_t)row * lddx + c] = rs * (t[e] - s1 - xh[e] * s2);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = lane + 64 * e;
        if (c < D) {
            red[w][0][c] = pg[e];
            red[w][1][c] = pb[e];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256) {
        part[(size_t)blockIdx.x * D + c] = ((red[0][0][c] + red[1][0][c]) + red[2][0][c]) + red[3][0][c];
        part[((size_t)nblk + blockIdx.x) * D + c] = ((red[0][1][c] + red[1][1][c]) + red[2][1][c]) + red[3][1][c];
    }
}

// ------------------------------------------------------------------------------------------------ small kernels
// dlogits[r, c] = g[r] (softmax(logits[r])[c] - [c == target[r]]), fp32 (one wave per row)
__global__ __launch_bounds__(256) void ce_bwd_f32_kernel(const float* __restrict__ logits, int ldl, const long long* __restrict__ target,
                                                         const float* __restrict__ lse, const float* __restrict__ g,
                                                         float* __restrict__ dl, int ldd, int rows, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float l = lse[row], gr = g[row];
    const long long t = target[row];
    for (int c = lane; c < V; c += 64)
        dl[(size_t)row * ldd + c] = gr * (expf(logits[(size_t)row * ldl + c] - l) - (c == t ? 1.f : 0.f));
}

// the same with loss options (label smoothing eps, z-loss zeta; csrc/elementwise.hip states the formulas):
// dlogits[r, c] = g[r] ((1 + 2 zeta lse[r]) softmax(logits[r])[c] - (1 - eps) [c == target[r]] - eps / V), 0 in [V, ldd)
__global__ __launch_bounds__(256) void ce_bwd_opts_f32_kernel(const float* __restrict__ logits, int ldl,
                                                              const long long* __restrict__ target, const float* __restrict__ lse,
                                                              const float* __restrict__ g, float* __restrict__ dl, int ldd, int rows,
                                                              int V, float eps, float zeta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float l = lse[row], gr = g[row];
    const long long t = target[row];
    const float a = 1.f + 2.f * zeta * l, u = eps / (float)V, ut = (1.f - eps) + u;
    for (int c = lane; c < ldd; c += 64)
        dl[(size_t)row * ldd + c] = c < V ? gr * (a * expf(logits[(size_t)row * ldl + c] - l) - (c == t ? ut : u)) : 0.f;
}

// gE[v] += scale * sum over the rows of token v (sorted order: perm / offs of commu_token_order) of drop(dX[row]); the
// dropout is the embedding site's (element index row * D + c).  One workgroup per vocabulary row.
__global__ __launch_bounds__(256) void embed_bwd_f32_kernel(const long long* __restrict__ perm, const long long* __restrict__ offs,
                                                            const float* __restrict__ dx, int ldx, float* __restrict__ gE, int D,
                                                            float scale, unsigned seed, unsigned thr, float ks) {
    const int v = blockIdx.x;
    const long long s0 = offs[v], s1 = offs[v + 1];
    const DropKey dk = drop_key(seed);
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float acc = 0.f;
        for (long long s = s0; s < s1; ++s) {
            const long long row = perm[s];
            float gv = dx[(size_t)row * ldx + c];
            if (thr) gv = drop_keep(dk, (unsigned)row * (unsigned)D + (unsigned)c, thr) ? gv * ks : 0.f;
            acc += gv;
        }
        gE[(size_t)v * D + c] += acc * scale;
    }
}

// y = x * keep / (1 - p) (element index r * cols + c), zero where gate <= 0 (the ReLU backward from the saved activation);
// forward and backward of a dropout site are the same operation.  y may alias x.
__global__ __launch_bounds__(256) void dropout_f32_kernel(const float* x, int ldx, const float* __restrict__ gate, int ldg, float* y,
                                                          int ldy, int rows, int cols, unsigned seed, unsigned thr, float ks) {
    const size_t n = (size_t)rows * cols;
    const DropKey dk = drop_key(seed);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx / cols), c = (int)(idx % cols);
        float v = x[(size_t)r * ldx + c];
        if (thr) v = drop_keep(dk, (unsigned)idx, thr) ? v * ks : 0.f;
        if (gate && !(gate[(size_t)r * ldg + c] > 0.f)) v = 0.f;
        y[(size_t)r * ldy + c] = v;
    }
}

AttF32 att_args(const float* q, int ld_q, const float* k, const float* v, int ld_kv, const float* rd, int ld_rd, const float* u,
                const float* vb, const unsigned char* reset, int T, int M, int B, int H, int DH, int same_length, int mem_len,
                float scale, float drop_p, unsigned drop_seed) {
    AttF32 a{};
    a.q = q; a.k = k; a.v = v; a.rd = rd; a.u = u; a.vb = vb; a.reset = reset;
    a.ld_q = ld_q; a.ld_kv = ld_kv; a.ld_rd = ld_rd;
    a.T = T; a.M = M; a.B = B; a.H = H; a.DH = DH; a.same_length = same_length; a.mem_len = mem_len; a.scale = scale;
    const unsigned thr = drop_threshold16(drop_p);
    a.drop_seed = drop_seed;
    a.drop_thr_hi = thr << 16;
    a.drop_scale = thr ? drop_keep_scale16(thr) : 1.f;
    return a;
}

bool att_vec4(const AttF32& a) {
    return a.DH % 4 == 0 && a.ld_q % 4 == 0 && a.ld_kv % 4 == 0 && a.ld_rd % 4 == 0 && a.ld_do % 4 == 0 &&
           (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.rd | (uintptr_t)a.u | (uintptr_t)a.vb |
             (uintptr_t)a.dout) % 16 == 0);
}

bool att_shape_ok(int T, int M, int B, int H, int DH) {
    return T > 0 && M >= 0 && B > 0 && H > 0 && DH > 0 && DH <= 64 && B <= 65535 && T + M <= 65535 && H <= 65535;
}

}  // namespace

extern "C" int commu_gemm_f32(int ta, int tb, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                              const float* bias, int relu, float drop_p, unsigned drop_seed, const float* resid, int ldr,
                              int accumulate, float* ws, int nslabs, hipStream_t stream) {
    if (M <= 0 || N <= 0 || K <= 0 || ta < 0 || ta > 1 || tb < 0 || tb > 1 || nslabs < 1 || M > 65535 * TG_BM) return -22;
    GemmEpi e{bias, resid, ldr, relu, drop_seed, drop_threshold16(drop_p), 1.f, accumulate};
    if (e.drop_thr) e.drop_scale = drop_keep_scale16(e.drop_thr);
    int kchunk = K;
    float* out = C;
    int ldo = ldc;
    if (nslabs > 1) {          // row split of a long contraction: raw slabs, then the in-order reduction into C
        if (ws == nullptr || ldc != N || bias || relu || e.drop_thr || resid) return -22;
        kchunk = ((K + nslabs - 1) / nslabs + TG_BK - 1) / TG_BK * TG_BK;
        nslabs = (K + kchunk - 1) / kchunk;
        out = ws;
        ldo = N;
    }
    const dim3 grid((N + TG_BN - 1) / TG_BN, (M + TG_BM - 1) / TG_BM, nslabs);
    const long long ss = (long long)M * N;
    // 16-byte staging loads (load_rows) when every row-major operand allows them
    const bool vec = (ta || (lda % 4 == 0 && (uintptr_t)A % 16 == 0)) && (!tb || (ldb % 4 == 0 && (uintptr_t)B % 16 == 0));
#define GEMM_F32_LAUNCH(TA, TB, VEC) \
    COMMU_LAUNCH((gemm_f32_kernel<TA, TB, VEC>), grid, dim3(256), 0, stream, A, lda, B, ldb, out, ldo, ss, M, N, K, kchunk, e)
    if (ta == 1 && tb == 0)
        GEMM_F32_LAUNCH(1, 0, false);          // (no row-major operand)
    else if (ta == 0 && tb == 1 && vec && !e.drop_thr && !accumulate && nslabs == 1)
        COMMU_LAUNCH((gemm_f32_kernel<0, 1, true, false>), grid, dim3(256), 0, stream, A, lda, B, ldb, out, ldo, ss, M, N, K, kchunk, e);
    else if (ta == 0 && tb == 1 && vec)
        GEMM_F32_LAUNCH(0, 1, true);
    else if (ta == 0 && tb == 1)
        GEMM_F32_LAUNCH(0, 1, false);
    else if (ta == 0 && vec)
        GEMM_F32_LAUNCH(0, 0, true);
    else if (ta == 0)
        GEMM_F32_LAUNCH(0, 0, false);
    else if (vec)
        GEMM_F32_LAUNCH(1, 1, true);
    else
        GEMM_F32_LAUNCH(1, 1, false);
#undef GEMM_F32_LAUNCH
    COMMU_LAUNCH_CHECK();
    if (nslabs > 1) return commu_reduce_slabs_f32(C, ws, (size_t)M * N, nslabs, (size_t)M * N, accumulate, 1.f, stream);
    return 0;
}

extern "C" int commu_relattn_fwd_f32(const float* q, int ld_q, const float* k, const float* v, int ld_kv, const float* rd, int ld_rd,
                                     const float* r_w_bias, const float* r_r_bias, const unsigned char* reset, float* out, int ld_o,
                                     float* lse, int T, int M, int B, int H, int DH, int same_length, int mem_len, float scale,
                                     float drop_p, unsigned drop_seed, hipStream_t stream) {
    if (!att_shape_ok(T, M, B, H, DH)) return -22;
    AttF32 a = att_args(q, ld_q, k, v, ld_kv, rd, ld_rd, r_w_bias, r_r_bias, reset, T, M, B, H, DH, same_length, mem_len, scale,
                        drop_p, drop_seed);
    a.out = out; a.ld_o = ld_o; a.lse = lse;
    a.dout = q; a.ld_do = ld_q;          // (no dO in the forward: keeps the alignment test of att_vec4 to the forward operands)
    const dim3 grid(H, B, T);
    if (att_vec4(a))
        COMMU_LAUNCH(relattn_fwd_f32_kernel<4>, grid, dim3(64), 0, stream, a);
    else
        COMMU_LAUNCH(relattn_fwd_f32_kernel<1>, grid, dim3(64), 0, stream, a);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_relattn_bwd_f32(const float* q, int ld_q, const float* k, const float* v, int ld_kv, const float* rd, int ld_rd,
                                     const float* r_w_bias, const float* r_r_bias, const unsigned char* reset, const float* o,
                                     int ld_o, const float* dout, int ld_do, const float* lse, float* delta, float* dq, int ld_dq,
                                     float* dq_ac, float* dq_bd, float* dk, float* dv, int ld_dkv, float* drd, int ld_drd, int T,
                                     int M, int B, int H, int DH, int same_length, int mem_len, float scale, float drop_p,
                                     unsigned drop_seed, hipStream_t stream) {
    if (!att_shape_ok(T, M, B, H, DH)) return -22;
    AttF32 a = att_args(q, ld_q, k, v, ld_kv, rd, ld_rd, r_w_bias, r_r_bias, reset, T, M, B, H, DH, same_length, mem_len, scale,
                        drop_p, drop_seed);
    a.o = o; a.ld_o = ld_o; a.dout = dout; a.ld_do = ld_do; a.lse_in = lse; a.delta = delta;
    a.dq = dq; a.ld_dq = ld_dq; a.dq_ac = dq_ac; a.dq_bd = dq_bd; a.dk = dk; a.dv = dv; a.ld_dkv = ld_dkv;
    a.drd = drd; a.ld_drd = ld_drd;
    const int K = T + M;
    COMMU_LAUNCH(relattn_delta_f32_kernel, dim3(H, B, T), dim3(64), 0, stream, a);
    COMMU_LAUNCH_CHECK();
    if (att_vec4(a)) {
        COMMU_LAUNCH(relattn_bwd_q_f32_kernel<4>, dim3(H, B, T), dim3(64), 0, stream, a);
        COMMU_LAUNCH(relattn_bwd_kv_f32_kernel<4>, dim3(H, B, K), dim3(64), 0, stream, a);
        COMMU_LAUNCH(relattn_bwd_rd_f32_kernel<4>, dim3(H, K), dim3(64), 0, stream, a);
    } else {
        COMMU_LAUNCH(relattn_bwd_q_f32_kernel<1>, dim3(H, B, T), dim3(64), 0, stream, a);
        COMMU_LAUNCH(relattn_bwd_kv_f32_kernel<1>, dim3(H, B, K), dim3(64), 0, stream, a);
        COMMU_LAUNCH(relattn_bwd_rd_f32_kernel<1>, dim3(H, K), dim3(64), 0, stream, a);
    }
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_layernorm_fwd_f32(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* mean,
                                       float* rstd, int rows, int D, float eps, hipStream_t stream) {
    if (rows <= 0 || D <= 0 || D > 1024) return -22;
    if ((mean == nullptr) != (rstd == nullptr)) return -22;
    if (mean)
        COMMU_LAUNCH(layernorm_fwd_f32_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, ldx, gamma, beta, y, ldy, mean,
                     rstd, rows, D, eps);
    else          // (the forward-only callers: parity forward, decode step)
        COMMU_LAUNCH(layernorm_fwd_f32_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, ldx, gamma, beta, y, ldy, mean,
                     rstd, rows, D, eps);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_layernorm_bwd_f32(const float* dy, int lddy, const float* add, int ldadd, const float* x, int ldx,
                                       const float* mean, const float* rstd, const float* gamma, float* dx, int lddx, float* part,
                                       int nblk, float* dgamma, float* dbeta, int rows, int D, hipStream_t stream) {
    if (rows <= 0 || D <= 0 || D > 1024 || nblk <= 0) return -22;
    const int rpb = (rows + nblk - 1) / nblk;
    COMMU_LAUNCH(layernorm_bwd_f32_kernel, dim3(nblk), dim3(256), 0, stream, dy, lddy, add, ldadd, x, ldx, mean, rstd, gamma, dx, lddx,
                 part, nblk, rows, D, rpb);
    COMMU_LAUNCH_CHECK();
    int rc = 0;
    if (dgamma) rc = commu_reduce_slabs_f32(dgamma, part, (size_t)D, nblk, (size_t)D, 1, 1.f, stream);
    if (rc == 0 && dbeta) rc = commu_reduce_slabs_f32(dbeta, part + (size_t)nblk * D, (size_t)D, nblk, (size_t)D, 1, 1.f, stream);
    return rc;
}

extern "C" int commu_ce_bwd_f32(const float* logits, int ldl, const long long* target, const float* lse, const float* g,
                                float* dlogits, int ldd, int rows, int V, hipStream_t stream) {
    if (rows <= 0 || V <= 0) return -22;
    COMMU_LAUNCH(ce_bwd_f32_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, lse, g, dlogits, ldd, rows, V);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// (the fp32 schedule's logits are fp32 like the bf16 one's: the forward with options is commu_ce_fwd_opts under this name)
extern "C" int commu_ce_fwd_opts_f32(const float* logits, int ldl, const long long* target, float* loss, float* nll, float* lse,
                                     int rows, int V, float label_smoothing, float z_loss, hipStream_t stream) {
    return commu_ce_fwd_opts(logits, ldl, (const int64_t*)target, loss, nll, lse, rows, V, label_smoothing, z_loss, stream);
}

extern "C" int commu_ce_bwd_opts_f32(const float* logits, int ldl, const long long* target, const float* lse, const float* g,
                                     float* dlogits, int ldd, int rows, int V, float label_smoothing, float z_loss,
                                     hipStream_t stream) {
    if (rows <= 0 || V <= 0 || ldd < V) return -22;
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f) || !(z_loss >= 0.f && z_loss < INFINITY)) return -22;
    COMMU_LAUNCH(ce_bwd_opts_f32_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, lse, g, dlogits, ldd,
                 rows, V, label_smoothing, z_loss);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_embed_bwd_f32(const long long* perm, const long long* offs, const float* dx, int ldx, float* gE, int V, int D,
                                   float scale, float drop_p, unsigned drop_seed, hipStream_t stream) {
    if (V <= 0 || D <= 0) return -22;
    const unsigned thr = drop_threshold16(drop_p);
    COMMU_LAUNCH(embed_bwd_f32_kernel, dim3(V), dim3(256), 0, stream, perm, offs, dx, ldx, gE, D, scale, drop_seed, thr,
                 thr ? drop_keep_scale16(thr) : 1.f);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_dropout_f32(const float* x, int ldx, const float* gate, int ldg, float* y, int ldy, int rows, int cols,
                                 float drop_p, unsigned drop_seed, hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return -22;
    const unsigned thr = drop_threshold16(drop_p);
    const size_t n = (size_t)rows * cols;
    const int nb = (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
    COMMU_LAUNCH(dropout_f32_kernel, dim3(nb), dim3(256), 0, stream, x, ldx, gate, ldg, y, ldy, rows, cols, drop_seed, thr,
                 thr ? drop_keep_scale16(thr) : 1.f);
    COMMU_LAUNCH_CHECK();
    return 0;
}
