// fp32 PARITY MODE of the generation path (model.parity_fp32 / generate.py --parity).
//
// The reference computes everything in fp32 (train.py:48 `amp = None`; no autocast anywhere in commu/model/model.py), and
// BASELINE.json's north star asks for bit-exact greedy tokens.  The throughput path of this library multiplies bf16
// operands, so its greedy argmax agrees with the reference only where the top-1 / top-2 logit gap exceeds the bf16 error.
// The fp32 forward -- embedding, sinusoid table, Linear, relative-position attention with XL memory, LayerNorm, logits
// (model.py:64-73,142-147,163-181,283-352,409-420,578-626) -- runs on fp32 operands end to end: fp32 master weights (no
// shadows), fp32 activations, fp32 K/V cache, fp32 MFMA for the Linears, accurate expf / sinf / cosf.  What differs from
// the reference's CPU / GPU PyTorch kernels is summation ORDER only (logits agree to ~1e-6 of their range).
// This translation unit holds what only the generation path needs: the Linear's entry point with the decode step's skinny
// kernel (every other shape forwards to commu_gemm_f32, train_f32.hip), the embedding, the sinusoid table, the attention
// entry points over a projection buffer / linear cache and over the ring cache (the row itself: attn_row_f32.h) and the
// K/V appends.  LayerNorm is commu_layernorm_fwd_f32 (train_f32.hip).
// The decode step is HBM-bound either way; fp32 costs 2x the bytes of the bf16 path.
#include "common.h"
#include "commu_hip.h"
#include "attn_row_f32.h"

// ------------------------------------------------------------------------------------------------ Linear
// C[M,N] = A[M,K] . B[N,K]^T (+ bias[n]) (ReLU) (+ resid[m,n]); every operand fp32, row-major with leading dimensions.
// v_mfma_f32_16x16x4_f32: A lane l = A[i = l & 15][k = l >> 4], B lane l = B[k = l >> 4][j = l & 15],
// D lane l, register r = D[i = 4 (l >> 4) + r][j = l & 15].
//
// Decode-step form (M <= 64 rows: one token per sequence): a workgroup owns 16 output columns and all rows, its four waves
// split K four ways and every lane feeds FOUR MFMAs from one 16-byte load per operand -- lane group g of k-block t holds
// k = 16 t + 4 g + s for MFMA s, the same bijection on both operands --, partial tiles are added through LDS.  N / 16
// workgroups stream the weight matrix once (the 64 x 64 tile of gemm_f32_kernel would put 24 workgroups on a [1536, 512]
// weight).
__global__ __launch_bounds__(256) void gemm_nt_f32_skinny_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B,
                                                                 int ldb, float* __restrict__ C, int ldc, int M, int N, int K,
                                                                 const float* __restrict__ bias, const float* __restrict__ resid,
                                                                 int ldr, int relu) {
    __shared__ f32x4 part[4][4][64];          // [wave][row tile][lane]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int ncol = min(n0 + r16, N - 1);
    const float* bp = B + (size_t)ncol * ldb;
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kq = (K + 63) / 64 * 16;          // k per wave, a multiple of 16
    const int kbeg = w * kq, kend = min(K, kbeg + kq);
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        const int kk = k0 + 4 * g;
        const f4 z = {0.f, 0.f, 0.f, 0.f};
        const f4 bv = (kk + 3 < kend) ? *(const f4*)(bp + kk) : z;          // (K % 4 == 0, 16-byte aligned rows: the launcher checks)
        f4 av[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = 16 * mt + r16;
            av[mt] = (row < M && kk + 3 < kend) ? *(const f4*)(A + (size_t)row * lda + kk) : z;
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].x, bv.x, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].y, bv.y, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].z, bv.z, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt].w, bv.w, acc[mt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) part[w][mt][lane] = acc[mt];
    __syncthreads();
    // wave w finishes row tile w: D lane l, register r = C[16 w + 4 (l >> 4) + r][n0 + (l & 15)]
    f32x4 sum = part[0][w][lane];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) sum += part[ww][w][lane];
    const int col = n0 + r16;
    if (col >= N) return;
    const float bs = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * w + 4 * g + r;
        if (row >= M) continue;
        float v = sum[r] + bs;
        if (relu) v = fmaxf(v, 0.f);
        if (resid) v += resid[(size_t)row * ldr + col];
        C[(size_t)row * ldc + col] = v;
    }
}

extern "C" int commu_gemm_nt_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                                 const float* bias, const float* resid, int ldr, int relu, hipStream_t stream) {
    if (M <= 0 || N <= 0 || K <= 0) return -22;
    if (M <= 64 && K % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) % 16 == 0)) {
        COMMU_LAUNCH(gemm_nt_f32_skinny_kernel, dim3((N + 15) / 16), dim3(256), 0, stream, A, lda, B, ldb, C, ldc, M, N, K, bias,
                     resid, ldr, relu);
        COMMU_LAUNCH_CHECK();
        return 0;
    }
    return commu_gemm_f32(0, 1, A, lda, B, ldb, C, ldc, M, N, K, bias, relu, 0.f, 0u, resid, ldr, 0, nullptr, 1, stream);
}

// ------------------------------------------------------------------------------------------------ embedding, sinusoid
// model.py:409-420: out[row] = E[token[row]] * sqrt(d_model)
__global__ void embed_f32_kernel(const long long* __restrict__ tok, const float* __restrict__ E, float* __restrict__ out, int ld,
                                 int rows, int D, float scale) {
    const int row = blockIdx.x;
    const float* e = E + (size_t)tok[row] * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) out[(size_t)row * ld + d] = e[d] * scale;
}

extern "C" int commu_embed_f32(const long long* tok, const float* E, float* out, int ld, int rows, int D, float scale,
                               hipStream_t stream) {
    if (rows <= 0) return -22;
    COMMU_LAUNCH(embed_f32_kernel, dim3(rows), dim3(128), 0, stream, tok, E, out, ld, rows, D, scale);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// model.py:142-147 by DISTANCE: out[d] = [sin(d * inv_freq) | cos(d * inv_freq)], d = 0 .. n - 1 (the reference's row m of a
// K-row table is position K - 1 - m, and the rel-shift pairs query i / key j with position i + M - j: the distance)
__global__ void posemb_f32_kernel(const float* __restrict__ inv_freq, float* __restrict__ out, int ld, int n, int D, int clamp_len) {
    const int d = blockIdx.x;
    const int half = D / 2;
    for (int c = threadIdx.x; c < half; c += blockDim.x) {
        const float x = (float)(clamp_len > 0 ? min(d, clamp_len) : d) * inv_freq[c];          // (torch.ger: one fp32 product per entry; :581-582)
        out[(size_t)d * ld + c] = sinf(x);
        out[(size_t)d * ld + half + c] = cosf(x);
    }
}

extern "C" int commu_posemb_f32(const float* inv_freq, float* out, int ld, int n, int D, int clamp_len, hipStream_t stream) {
    if (n <= 0 || D % 2) return -22;
    COMMU_LAUNCH(posemb_f32_kernel, dim3(n), dim3(128), 0, stream, inv_freq, out, ld, n, D, clamp_len);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ attention
// model.py:283-345 for one (query i, sequence b, head h) per wave:
//   s_j = ((q_i + u) . k_j + (q_i + v) . Rd[i + M_b - j]) * scale,  visible keys: lo_i <= j <= i + M_b,
//   out_i = softmax_j(s) . v.
// The row itself is attn_row_f32 (attn_row_f32.h); this kernel finds the window and the operands.  Element (j, b, h, d) of k / v is at
// base + j * sj + b * sb + h * DH + d: the [K * B, 3 H DH] projection buffer (sj = B * ld, sb = ld) or the decode cache
// [B][Lmax][H DH] (sj = H DH, sb = Lmax * H DH).  klen (optional, int32 [B]): the memory length M_b of sequence b (ragged
// decode batch); otherwise M for every sequence.  Masks as model.py:549-574: causal; same_length (keys j <= i - s hidden, s
// from the sequence's own key count); reset[b] (memory keys hidden).
template <int VW>
__global__ __launch_bounds__(64) void relattn_f32_kernel(const float* __restrict__ q, int ld_q, const float* __restrict__ kbase,
                                                         const float* __restrict__ vbase, long long sj, long long sb,
                                                         const float* __restrict__ rd, int ld_rd, const float* __restrict__ u,
                                                         const float* __restrict__ vbias, const int* __restrict__ klen,
                                                         const unsigned char* __restrict__ reset, float* __restrict__ out,
                                                         int ld_o, int T, int M, int B, int H, int DH, int same_length,
                                                         int mem_len, float scale) {
    const int h = blockIdx.x, b = blockIdx.y, i = blockIdx.z, lane = threadIdx.x;
    const int Mb = klen ? klen[b] : M;
    const int lo = vis_lo(same_length, T, Mb, mem_len, i, reset && reset[b]), hi = i + Mb;
    const size_t hd = (size_t)h * DH;
    float lse;
    const float o = attn_row_f32<VW, false>(q + ((size_t)i * B + b) * ld_q + hd, u + hd, vbias + hd, kbase + (size_t)b * sb + hd,
                                            vbase + (size_t)b * sb + hd, (size_t)sj, RowsLinear{}, rd + hd, ld_rd, lo, hi, DH,
                                            scale, 0u, 0u, H, b, h, i, lse);
    if (lane < DH) out[((size_t)i * B + b) * ld_o + hd + lane] = o;
}

extern "C" int commu_relattn_f32(const float* q, int ld_q, const float* k, const float* v, long long stride_key,
                                 long long stride_seq, const float* rd, int ld_rd, const float* r_w_bias, const float* r_r_bias,
                                 const int* klen, const unsigned char* reset, float* out, int ld_o, int T, int M, int B, int H,
                                 int DH, int same_length, int mem_len, float scale, hipStream_t stream) {
    if (T <= 0 || B <= 0 || H <= 0 || DH <= 0 || DH > 64 || B > 65535 || T > 65535) return -22;
    const dim3 grid(H, B, T);
    const bool v4 = DH % 4 == 0 && stride_key % 4 == 0 && stride_seq % 4 == 0 && ld_rd % 4 == 0 &&
                    (((uintptr_t)k | (uintptr_t)rd) % 16 == 0);
    if (v4)
        COMMU_LAUNCH(relattn_f32_kernel<4>, grid, dim3(64), 0, stream, q, ld_q, k, v, stride_key, stride_seq, rd, ld_rd, r_w_bias,
                     r_r_bias, klen, reset, out, ld_o, T, M, B, H, DH, same_length, mem_len, scale);
    else
        COMMU_LAUNCH(relattn_f32_kernel<1>, grid, dim3(64), 0, stream, q, ld_q, k, v, stride_key, stride_seq, rd, ld_rd, r_w_bias,
                     r_r_bias, klen, reset, out, ld_o, T, M, B, H, DH, same_length, mem_len, scale);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// decode step: the new token's key / value rows (columns HD .. 3 HD of its projection) into row klen[b] of the caches
// [B][Lmax][HD] for the sequences that step (active == NULL: all)
__global__ void kv_append_f32_kernel(const float* __restrict__ qkv, int ld, float* __restrict__ kc, float* __restrict__ vc,
                                     const int* __restrict__ klen, const unsigned char* __restrict__ active, int HD, int Lmax) {
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    const int pos = klen[b];
    if (pos >= Lmax) return;
    const float* src = qkv + (size_t)b * ld;
    float* kd = kc + ((size_t)b * Lmax + pos) * HD;
    float* vd = vc + ((size_t)b * Lmax + pos) * HD;
    for (int c = threadIdx.x; c < HD; c += blockDim.x) {
        kd[c] = src[HD + c];
        vd[c] = src[2 * HD + c];
    }
}

extern "C" int commu_decode_kv_append_f32(const float* qkv, int ld, float* kc, float* vc, const int* klen,
                                          const unsigned char* active, int B, int HD, int Lmax, hipStream_t stream) {
    if (B <= 0) return -22;
    COMMU_LAUNCH(kv_append_f32_kernel, dim3(B), dim3(128), 0, stream, qkv, ld, kc, vc, klen, active, HD, Lmax);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ sliding decode memory
// The cached decode step on a RING of W = mem_len + 1 rows per sequence ([B][W][H DH]): the reference's sliding memory
// (model.py:507-538) with the same_length mask of model.py:549-568 at qlen 1.  klen[b] counts ABSOLUTE positions; position
// p lives in row p mod W.  The new token (position pos = klen[b], already appended) sees positions
// max(0, pos - (W - 1)) .. pos, without the oldest of them when same_length is on and the memory is full; distance
// pos - p.  Keys are visited in CHRONOLOGICAL order by the row function that relattn_f32_kernel calls (attn_row_f32, here
// with the ring's row map; its P . V walk wraps the row incrementally, no modulo per key): before the first wrap the
// result equals the linear cache's bit for bit.
template <int VW>
__global__ __launch_bounds__(64) void decode_attn_ring_f32_kernel(const float* __restrict__ q, int ld_q,
                                                                  const float* __restrict__ kbase,
                                                                  const float* __restrict__ vbase,
                                                                  const float* __restrict__ rd, int ld_rd,
                                                                  const float* __restrict__ u,
                                                                  const float* __restrict__ vbias,
                                                                  const int* __restrict__ klen, float* __restrict__ out,
                                                                  int ld_o, int H, int DH, int W, int same_length,
                                                                  float scale) {
    const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int pos = klen[b], M = W - 1;
    int lo = pos > M ? pos - M : 0;
    if (same_length && pos >= M) lo += 1;
    const size_t hd = (size_t)h * DH, sj = (size_t)H * DH;
    float lse;
    const float o = attn_row_f32<VW, false>(q + (size_t)b * ld_q + hd, u + hd, vbias + hd, kbase + (size_t)b * W * sj + hd,
                                            vbase + (size_t)b * W * sj + hd, sj, RowsRing{(pos / W) * W, W}, rd + hd, ld_rd, lo,
                                            pos, DH, scale, 0u, 0u, H, b, h, 0, lse);
    if (lane < DH) out[(size_t)b * ld_o + hd + lane] = o;
}

extern "C" int commu_decode_attn_ring_f32(const float* q, int ld_q, const float* kc, const float* vc, const float* rd,
                                          int ld_rd, const float* r_w_bias, const float* r_r_bias, const int* klen,
                                          float* out, int ld_o, int B, int H, int DH, int W, int same_length, float scale,
                                          hipStream_t stream) {
    if (B <= 0 || H <= 0 || DH <= 0 || DH > 64 || B > 65535 || W < 2 || klen == nullptr) return -22;
    const dim3 grid(H, B);
    const bool v4 = DH % 4 == 0 && ld_rd % 4 == 0 && (((uintptr_t)kc | (uintptr_t)rd) % 16 == 0);
    if (v4)
        COMMU_LAUNCH(decode_attn_ring_f32_kernel<4>, grid, dim3(64), 0, stream, q, ld_q, kc, vc, rd, ld_rd, r_w_bias, r_r_bias,
                     klen, out, ld_o, H, DH, W, same_length, scale);
    else
        COMMU_LAUNCH(decode_attn_ring_f32_kernel<1>, grid, dim3(64), 0, stream, q, ld_q, kc, vc, rd, ld_rd, r_w_bias, r_r_bias,
                     klen, out, ld_o, H, DH, W, same_length, scale);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// the new token's key / value rows into ring row klen[b] mod W of the caches [B][W][HD]
__global__ void kv_append_ring_f32_kernel(const float* __restrict__ qkv, int ld, float* __restrict__ kc, float* __restrict__ vc,
                                          const int* __restrict__ klen, const unsigned char* __restrict__ active, int HD, int W) {
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    const int row = klen[b] % W;
    const float* src = qkv + (size_t)b * ld;
    float* kd = kc + ((size_t)b * W + row) * HD;
    float* vd = vc + ((size_t)b * W + row) * HD;
    for (int c = threadIdx.x; c < HD; c += blockDim.x) {
        kd[c] = src[HD + c];
        vd[c] = src[2 * HD + c];
    }
}

extern "C" int commu_decode_kv_append_ring_f32(const float* qkv, int ld, float* kc, float* vc, const int* klen,
                                               const unsigned char* active, int B, int HD, int W, hipStream_t stream) {
    if (B <= 0 || W < 1 || klen == nullptr) return -22;
    COMMU_LAUNCH(kv_append_ring_f32_kernel, dim3(B), dim3(128), 0, stream, qkv, ld, kc, vc, klen, active, HD, W);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// Ragged prefill of the fp32 caches [B][Lmax][HD]: key / value columns of the time-major projection rows t * B + b,
// positions lo <= t < len[b] (lo = max(0, len[b] - window) on a ring, else 0), into the rows of slot[b]; klen[slot[b]] =
// len[b].  VW floats per lane (4: 16 bytes); a row's HD floats are consecutive on both sides.  blockIdx.y walks the
// kept range in pieces of 32 positions.
template <int VW>
__global__ __launch_bounds__(256) void prefill_scatter_f32_kernel(const float* __restrict__ qkv, int ld, int T, int B,
                                                                  float* __restrict__ kc, float* __restrict__ vc,
                                                                  int* __restrict__ klen, const int* __restrict__ len,
                                                                  const int* __restrict__ slot, int Bc, int HD, int Lmax,
                                                                  int window) {
    const int b = blockIdx.x;
    const int s = slot != nullptr ? slot[b] : b;
    if (s < 0 || s >= Bc) return;
    const int n = min(max(len[b], 0), T);
    if (blockIdx.y == 0 && threadIdx.x == 0) klen[s] = n;
    const int lo = window > 0 ? max(0, n - window) : 0;
    const int hi = window > 0 ? n : min(n, Lmax);
    const int t0 = lo + blockIdx.y * 32, t1 = min(t0 + 32, hi);
    const int per = HD / VW;
    for (int i = threadIdx.x; i < (t1 - t0) * per; i += blockDim.x) {
        const int t = t0 + i / per, c = (i % per) * VW;
        const float* p = qkv + ((size_t)t * B + b) * ld + HD + c;
        const size_t d = ((size_t)s * Lmax + (window > 0 ? t % Lmax : t)) * HD + c;
        if constexpr (VW == 4) {
            const float4 kq = *reinterpret_cast<const float4*>(p);
            const float4 vq = *reinterpret_cast<const float4*>(p + HD);
            *reinterpret_cast<float4*>(kc + d) = kq;
            *reinterpret_cast<float4*>(vc + d) = vq;
        } else {
            kc[d] = p[0];
            vc[d] = p[HD];
        }
    }
}

extern "C" int commu_decode_prefill_scatter_f32(const float* qkv, int ld, int T, int B, float* kc, float* vc, int* klen,
                                                const int* len, const int* slot, int Bcache, int HD, int Lmax, int window,
                                                hipStream_t stream) {
    if (B <= 0 || T <= 0) return 0;
    if (HD <= 0 || Bcache <= 0 || Lmax <= 0 || window < 0 || (window > 0 && Lmax != window + 1) || ld < 3 * HD) return -22;
    if (klen == nullptr || len == nullptr) return -22;
    const int cap = window > 0 ? window : Lmax;
    const int span = T < cap ? T : cap;
    const dim3 grid(B, (span + 31) / 32);
    if (grid.y > 65535) return -22;
    const bool v4 = HD % 4 == 0 && ld % 4 == 0 && (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc) % 16 == 0);
    if (v4)
        COMMU_LAUNCH(prefill_scatter_f32_kernel<4>, grid, dim3(256), 0, stream, qkv, ld, T, B, kc, vc, klen, len, slot,
                     Bcache, HD, Lmax, window);
    else
        COMMU_LAUNCH(prefill_scatter_f32_kernel<1>, grid, dim3(256), 0, stream, qkv, ld, T, B, kc, vc, klen, len, slot,
                     Bcache, HD, Lmax, window);
    COMMU_LAUNCH_CHECK();
    return 0;
}
