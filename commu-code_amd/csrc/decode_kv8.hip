// Cached decode step over an fp8 K/V cache (gfx950): the opt-in mode of csrc/decode.hip's attention and prefill scatter.
//
// STORAGE (per layer; include/commu_hip.h):  kc8 / vc8 uint8 [B][H][Lmax][DH], OCP e4m3 bytes, head-major like the bf16
// caches;  ks / vs uint8 [B][H][Lmax][DH/32], one E8M0 byte per 32 consecutive features of a row (scale 2^(byte - 127)).
// The quantiser is commu_quant_mxfp8's recipe (csrc/gemm_fp8.hip): sb = clamp(biased exponent of the block's amax - 8,
// 0, 254), elements times 2^(127 - sb), clamped to +-448, rounded to nearest even.  0.516 of the bf16 cache's bytes.
//
// A POSITION HAS ONE K AND ONE V, WHATEVER STEP READS IT: the step that appends a token attends to the quantise ->
// dequantise image of its K and V, taken from registers (the bytes it stores, decoded like every other row), so
// out = contract(dequant(cache after the append)) on every step.
//
// The scales are powers of two: a lane applies the scale of its block to its partial dot product (K) or to the
// probability (V), which is the same number as scaling the 16 elements first, so the error constant of the bf16 kernel
// carries over (tests/kv8_contract.py).  The distance table stays bf16: it is shared by all sequences of a head.
//
// Kernel structure, klen / active / ring-row / hidden-row rules and the split-key protocol: decode_attn_kernel of
// decode.hip, with 16 features (16 cache bytes) per lane, so a wave instruction covers 64 / (DH / 16) rows.
#include "common.h"
#include "commu_hip.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int DEC_MAXK = 4224;      // as in decode.hip: the score row of a pair lives in LDS

// The quantiser, for the lane that holds 16 consecutive features of a row; the lane with the other half of the 32-block
// is its xor-1 neighbour and must be executing too.  q: the 16 e4m3 bytes; returns the E8M0 byte of the block.
__device__ __forceinline__ int quant16_e4m3(const float (&x)[16], uint4& q) {
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
    amax = fmaxf(amax, dpp_f<0xB1>(amax));
    const int eb = (int)((__float_as_uint(amax) >> 23) & 0xFFu);  // biased floor(log2 amax) (0 for zero / denormal blocks)
    int sb = eb - 8;                                               // E8M0 byte: scale 2^(sb - 127)
    sb = sb < 0 ? 0 : (sb > 254 ? 254 : sb);
    const float inv = __uint_as_float((unsigned)(254 - sb) << 23); // 2^(127 - sb)
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = fminf(fmaxf(x[e] * inv, -448.f), 448.f);
    int w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i], v[4 * i + 1], 0, false);
        w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2], v[4 * i + 3], w[i], true);
    }
    q = make_uint4((unsigned)w[0], (unsigned)w[1], (unsigned)w[2], (unsigned)w[3]);
    return sb;
}

__device__ __forceinline__ void bf16x16_to_f32(const bf16x8 a, const bf16x8 b, float (&x)[16]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { x[e] = bf2f(a[e]); x[8 + e] = bf2f(b[e]); }
}

// 16 e4m3 bytes -> floats (unscaled)
__device__ __forceinline__ void dequant16_e4m3(const uint4 q, float (&f)[16]) {
    const int w[4] = {(int)q.x, (int)q.y, (int)q.z, (int)q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
        f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
    }
}

// (a ?: on whole uint4 values goes through the stack; per dword it is four v_cndmask)
__device__ __forceinline__ uint4 sel16(bool c, const uint4 a, const uint4 b) {
    return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// 2^(sb - 127) (sb = 0: the subnormal 2^-127)
__device__ __forceinline__ float e8m0_scale(int sb) { return __uint_as_float(sb > 0 ? (unsigned)sb << 23 : 0x00400000u); }

// sum over the LPR lanes of a row (LPR 4: a quad; LPR 2: a pair)
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
    v += dpp_f<0xB1>(v);
    if (LPR == 4) v += dpp_f<0x4E>(v);
    return v;
}

// one workgroup per (b, h), or per split of it; see decode_attn_kernel (decode.hip) for everything that is not about bytes
template <int DH, bool RING, int UNR = 4>
__global__ __launch_bounds__(256) void decode_attn_kv8_kernel(
    const bf16* __restrict__ qkv, int ld_qkv, const unsigned char* kc, const unsigned char* vc, const unsigned char* ks,
    const unsigned char* vs, const bf16* __restrict__ rd, int ld_rd, const float* __restrict__ u,
    const float* __restrict__ vb, const int* __restrict__ klen, const unsigned char* __restrict__ active,
    bf16* __restrict__ out, int ld_o, int H, int Lmax, float scale, int append, int nsplit, float* split_ws,
    unsigned* split_cnt, int mask_oldest) {
    constexpr int LPR = DH / 16;           // lanes per row (4 for DH 64, 2 for DH 32)
    constexpr int RPW = 64 / LPR;          // rows per wave instruction
    constexpr int NB = DH / 32;            // scale bytes per row
    __shared__ float sS[DEC_MAXK];
    __shared__ float red[8];
    __shared__ float sO[4][RPW][DH];
    __shared__ int s_last;
    const int pair = nsplit > 1 ? blockIdx.x / nsplit : blockIdx.x;
    const int split = nsplit > 1 ? blockIdx.x - pair * nsplit : 0;
    const int b = pair / H, h = pair - b * H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int sub = lane % LPR, rowl = lane / LPR;
    const int apos = klen[b];
    const int pos = RING ? apos % Lmax : apos;          // the new token's cache row
    const unsigned char act = active != nullptr ? active[b] : (unsigned char)1;
    const bf16* qrow = qkv + (size_t)b * ld_qkv + h * DH + 16 * sub;
    float qf[16], xk[16], xv[16];
    bf16x16_to_f32(ld_bf16x8(qrow), ld_bf16x8(qrow + 8), qf);
    bf16x16_to_f32(ld_bf16x8(qrow + H * DH), ld_bf16x8(qrow + H * DH + 8), xk);
    bf16x16_to_f32(ld_bf16x8(qrow + 2 * H * DH), ld_bf16x8(qrow + 2 * H * DH + 8), xv);
    float qu[16], qv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        qu[e] = (qf[e] + u[h * DH + 16 * sub + e]) * scale;
        qv[e] = (qf[e] + vb[h * DH + 16 * sub + e]) * scale;
    }
    if (!act) return;
    // the new token's row as the cache will hold it: every lane quantises the 16 features of its chunk (the lanes of a
    // row's 32-block are neighbours), lanes 0 .. 2 LPR - 1 of split 0 store them, and the step itself reads these
    // registers for row `self`, so nothing waits for the store
    uint4 knew, vnew;
    const int knew_s = quant16_e4m3(xk, knew), vnew_s = quant16_e4m3(xv, vnew);
    const int self = (append && (RING || pos < Lmax)) ? pos : -1;
    const size_t row0 = ((size_t)b * H + h) * Lmax;
    if (self >= 0 && tid < 2 * LPR && split == 0) {
        const bool isk = tid < LPR;
        unsigned char* dst = (unsigned char*)(isk ? kc : vc) + (row0 + pos) * DH + 16 * sub;
        *reinterpret_cast<uint4*>(dst) = sel16(isk, knew, vnew);
        if ((sub & 1) == 0)
            ((unsigned char*)(isk ? ks : vs))[(row0 + pos) * NB + (sub >> 1)] = (unsigned char)(isk ? knew_s : vnew_s);
    }
    const int nall = min(apos + 1, Lmax);
    const int jmask = (RING && mask_oldest && apos >= Lmax - 1) ? (pos + 1 == Lmax ? 0 : pos + 1) : -1;
    int jlo = 0, n = nall, neff = 1;
    if (nsplit > 1) {
        int chunk = (nall + nsplit - 1) / nsplit;
        chunk = max(512, (chunk + 63) & ~63);
        neff = (nall + chunk - 1) / chunk;
        if (split >= neff) return;
        jlo = split * chunk;
        n = min(nall, jlo + chunk);
    }
    const unsigned char* kb = kc + row0 * DH + 16 * sub;
    const unsigned char* vbp = vc + row0 * DH + 16 * sub;
    const unsigned char* ksb = ks + row0 * NB + (sub >> 1);
    const unsigned char* vsb = vs + row0 * NB + (sub >> 1);
    const bf16* rb = rd + h * DH + 16 * sub;
    // ---- scores: RPW keys per wave instruction, software-pipelined as in decode.hip (the loads of batch i + 1 are issued
    // before batch i is consumed).  Every cache row read here is a row below n: written bytes, never stale ones.
    constexpr int STEP = 4 * RPW * UNR;
    float mx = -3.0e38f;
    {
        uint4 kk[UNR], kn[UNR];
        int sk[UNR], sn[UNR];
        bf16x8 r8[UNR][2], rn[UNR][2];
        auto issue = [&](uint4 (&kd)[UNR], int (&sd)[UNR], bf16x8 (&rdst)[UNR][2], int j0) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int jc = min(j0 + 4 * RPW * i + rowl, n - 1);
                kd[i] = *reinterpret_cast<const uint4*>(kb + (size_t)jc * DH);
                sd[i] = ksb[(size_t)jc * NB];
                int d = RING ? pos - jc : (nall - 1) - jc;
                if (RING && d < 0) d += Lmax;          // rows after the new token's hold the OLDEST positions
                rdst[i][0] = ld_bf16x8(rb + (size_t)d * ld_rd);
                rdst[i][1] = ld_bf16x8(rb + (size_t)d * ld_rd + 8);
            }
        };
        auto consume = [&](const uint4 (&kd)[UNR], const int (&sd)[UNR], const bf16x8 (&rdst)[UNR][2], int j0) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int j = j0 + 4 * RPW * i + rowl;
                const bool me = j == self;
                float kf[16];
                dequant16_e4m3(sel16(me, knew, kd[i]), kf);
                float dk = 0.f, sr = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    dk += qu[e] * kf[e] + qu[8 + e] * kf[8 + e];
                    sr += qv[e] * bf2f(rdst[i][0][e]) + qv[8 + e] * bf2f(rdst[i][1][e]);
                }
                float s = row_sum<LPR>(dk * e8m0_scale(me ? knew_s : sd[i]) + sr);
                if (RING && j == jmask) s = -3.0e38f;          // hidden: its probability becomes exactly 0
                if (j < n) {
                    if (sub == 0) sS[j - jlo] = s;
                    mx = fmaxf(mx, s);
                }
            }
        };
        int j0 = jlo + w * RPW;
        if (j0 < n) issue(kk, sk, r8, j0);
        for (; j0 < n; j0 += 2 * STEP) {
            if (j0 + STEP < n) issue(kn, sn, rn, j0 + STEP);
            consume(kk, sk, r8, j0);
            if (j0 + 2 * STEP < n) issue(kk, sk, r8, j0 + 2 * STEP);
            if (j0 + STEP < n) consume(kn, sn, rn, j0 + STEP);
        }
    }
    uint4 v8[UNR], vn[UNR];
    int sv[UNR], svn[UNR];
    auto issue_v = [&](uint4 (&vd)[UNR], int (&sd)[UNR], int j0) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int jc = min(j0 + 4 * RPW * i + rowl, n - 1);
            vd[i] = *reinterpret_cast<const uint4*>(vbp + (size_t)jc * DH);
            sd[i] = vsb[(size_t)jc * NB];
        }
    };
    if (jlo + w * RPW < n) issue_v(v8, sv, jlo + w * RPW);
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int j = tid; j < n - jlo; j += 256) {
        const float p = __expf(sS[j] - mx);
        sS[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + w] = sum;
    __syncthreads();
    const float lsum = red[4] + red[5] + red[6] + red[7];
    const float inv = 1.f / lsum;
    // ---- P.V: lane accumulates 16 features of the keys it visits
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    auto consume_v = [&](const uint4 (&vd)[UNR], const int (&sd)[UNR], int j0) {
        float p[UNR];
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int j = j0 + 4 * RPW * i + rowl;
            p[i] = (j < n) ? sS[j - jlo] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            // (the CLAMPED row: a tail lane past n re-reads row n - 1 with p = 0; where that is the new token's row, whose
            //  store may not have landed -- another workgroup's, with a split --, stale bytes can decode to NaN (0x7F / 0xFF)
            //  and a stale scale byte 0xFF to infinity: 0 x either must not reach acc, so the registers stand in)
            const bool me = min(j0 + 4 * RPW * i + rowl, n - 1) == self;
            float vf[16];
            dequant16_e4m3(sel16(me, vnew, vd[i]), vf);
            const float ps = p[i] * e8m0_scale(me ? vnew_s : sd[i]);
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += ps * vf[e];
        }
    };
    for (int j0 = jlo + w * RPW; j0 < n; j0 += 2 * STEP) {
        if (j0 + STEP < n) issue_v(vn, svn, j0 + STEP);
        consume_v(v8, sv, j0);
        if (j0 + 2 * STEP < n) issue_v(v8, sv, j0 + 2 * STEP);
        if (j0 + STEP < n) consume_v(vn, svn, j0 + STEP);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) sO[w][rowl][16 * sub + e] = acc[e];
    __syncthreads();
    float o = 0.f;
    if (tid < DH) {
        for (int ww = 0; ww < 4; ++ww)
            for (int r = 0; r < RPW; ++r) o += sO[ww][r][tid];
    }
    if (neff == 1) {
        if (tid < DH) out[(size_t)b * ld_o + h * DH + tid] = f2bf(o * inv);
        return;
    }
    // ---- split: publish (o[DH], max, sum), the last arriver of the pair combines (the protocol of decode.hip)
    constexpr int REC = DH + 2;
    float* rec = split_ws + ((size_t)pair * nsplit + split) * REC;
    if (tid < DH) __hip_atomic_store(rec + tid, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == DH) __hip_atomic_store(rec + DH, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == DH + 1) __hip_atomic_store(rec + DH + 1, lsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): every storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(split_cnt + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == (unsigned)(neff - 1);
        if (s_last) __hip_atomic_store(split_cnt + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // next launch
    }
    __syncthreads();
    if (!s_last) return;
    if (tid < DH) {
        const float* base = split_ws + (size_t)pair * nsplit * REC;
        float m = -3.0e38f;
        for (int sidx = 0; sidx < neff; ++sidx)
            m = fmaxf(m, __hip_atomic_load(base + sidx * REC + DH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        float num = 0.f, den = 0.f;
        for (int sidx = 0; sidx < neff; ++sidx) {
            const float f = __expf(__hip_atomic_load(base + sidx * REC + DH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - m);
            num += f * __hip_atomic_load(base + sidx * REC + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            den += f * __hip_atomic_load(base + sidx * REC + DH + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        out[(size_t)b * ld_o + h * DH + tid] = f2bf(num / den);
    }
}

// Ragged prefill with the quantiser on the way: prefill_scatter_kernel of decode.hip, a lane moving 16 features (32
// source bytes, 16 cache bytes) of K and of V; the 4 lanes of a position read one 128-byte line of the source (one head
// at DH 64, two at DH 32); the even lane of a 32-block also writes its scale byte.  Workgroup = 64 positions;
// blockIdx.z walks the kept range in pieces of 256 positions.
template <int DH>
__global__ __launch_bounds__(256) void prefill_scatter_kv8_kernel(const bf16* __restrict__ qkv, int ld, int T, int B,
                                                                  unsigned char* __restrict__ kc,
                                                                  unsigned char* __restrict__ vc,
                                                                  unsigned char* __restrict__ ks,
                                                                  unsigned char* __restrict__ vs, int* __restrict__ klen,
                                                                  const int* __restrict__ len, const int* __restrict__ slot,
                                                                  int Bc, int H, int Lmax, int window) {
    constexpr int HPL = 64 / DH;                      // heads per 128-byte line
    constexpr int NB = DH / 32;
    const int b = blockIdx.y;
    const int s = slot != nullptr ? slot[b] : b;
    if (s < 0 || s >= Bc) return;
    const int n = min(max(len[b], 0), T);
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) klen[s] = n;
    const int lo = window > 0 ? max(0, n - window) : 0;
    const int hi = window > 0 ? n : min(n, Lmax);
    const int c = threadIdx.x & 3;
    const int head = blockIdx.x * HPL + (c * 16) / DH, col = (c * 16) % DH;
    if (head >= H) return;          // (DH 32, odd H: lanes 2, 3 -- a whole 32-block -- leave together)
    const size_t HD = (size_t)H * DH;
    const bf16* src = qkv + (size_t)b * ld + HD + (size_t)head * DH + col;
    const size_t dst0 = ((size_t)s * H + head) * Lmax;
    // (the lanes of a position share t, so the two lanes of a 32-block run the same iterations)
    for (int t = lo + blockIdx.z * 256 + (threadIdx.x >> 2), e = 0; e < 4 && t < hi; ++e, t += 64) {
        const bf16* p = src + (size_t)t * B * ld;
        float xk[16], xv[16];
        bf16x16_to_f32(ld_bf16x8(p), ld_bf16x8(p + 8), xk);
        bf16x16_to_f32(ld_bf16x8(p + HD), ld_bf16x8(p + HD + 8), xv);
        uint4 kq, vq;
        const int ksc = quant16_e4m3(xk, kq), vsc = quant16_e4m3(xv, vq);
        const size_t row = dst0 + (window > 0 ? t % Lmax : t);
        *reinterpret_cast<uint4*>(kc + row * DH + col) = kq;
        *reinterpret_cast<uint4*>(vc + row * DH + col) = vq;
        if ((c & 1) == 0) {
            ks[row * NB + col / 32] = (unsigned char)ksc;
            vs[row * NB + col / 32] = (unsigned char)vsc;
        }
    }
}

}  // namespace

extern "C" int commu_decode_prefill_scatter_kv8(const void* qkv, int ld_qkv, int T, int B, void* kc8, void* vc8, void* ks,
                                                void* vs, int* klen, const int* len, const int* slot, int Bcache, int H,
                                                int DH, int Lmax, int window, hipStream_t stream) {
    if (B <= 0 || T <= 0) return 0;
    if (H <= 0 || Bcache <= 0 || Lmax <= 0 || window < 0 || (window > 0 && Lmax != window + 1) || B > 65535) return -22;
    if (ld_qkv < 3 * H * DH || (ld_qkv % 8) || (((uintptr_t)qkv | (uintptr_t)kc8 | (uintptr_t)vc8) % 16)) return -22;
    if (klen == nullptr || len == nullptr || ks == nullptr || vs == nullptr) return -22;
    const int cap = window > 0 ? window : Lmax;          // positions a sequence can keep
    const int span = T < cap ? T : cap;
    if (DH == 64) {
        COMMU_LAUNCH(prefill_scatter_kv8_kernel<64>, dim3(H, B, (span + 255) / 256), dim3(256), 0, stream, (const bf16*)qkv,
                     ld_qkv, T, B, (unsigned char*)kc8, (unsigned char*)vc8, (unsigned char*)ks, (unsigned char*)vs, klen,
                     len, slot, Bcache, H, Lmax, window);
    } else if (DH == 32) {
        COMMU_LAUNCH(prefill_scatter_kv8_kernel<32>, dim3((H + 1) / 2, B, (span + 255) / 256), dim3(256), 0, stream,
                     (const bf16*)qkv, ld_qkv, T, B, (unsigned char*)kc8, (unsigned char*)vc8, (unsigned char*)ks,
                     (unsigned char*)vs, klen, len, slot, Bcache, H, Lmax, window);
    } else {
        return -22;
    }
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_decode_attn_kv8(const void* qkv, int ld_qkv, void* kc8, void* vc8, void* ks, void* vs, const void* rd,
                                     int ld_rd, const float* r_w_bias, const float* r_r_bias, const int* klen,
                                     const unsigned char* active, void* out, int ld_o, int B, int H, int DH, int Lmax,
                                     float scale, int append, int ring, int mask_oldest, int nsplit, float* split_ws,
                                     unsigned* split_cnt, hipStream_t stream) {
    if (B <= 0) return 0;
    if (H <= 0 || Lmax <= 0 || Lmax > DEC_MAXK || (ld_qkv % 8) || (ld_rd % 8)) return -22;
    if ((((uintptr_t)qkv | (uintptr_t)kc8 | (uintptr_t)vc8 | (uintptr_t)rd) % 16)) return -22;
    if (ring && Lmax < 2) return -22;
    if (nsplit < 1 || nsplit > 16 || (nsplit > 1 && (split_ws == nullptr || split_cnt == nullptr))) return -22;
    const dim3 grid(B * H * nsplit);
    const int mo = (ring && mask_oldest) ? 1 : 0;
#define KV8_LAUNCH(DH_, RING_)                                                                                             \
    COMMU_LAUNCH((decode_attn_kv8_kernel<DH_, RING_>), grid, dim3(256), 0, stream, (const bf16*)qkv, ld_qkv,               \
                 (const unsigned char*)kc8, (const unsigned char*)vc8, (const unsigned char*)ks, (const unsigned char*)vs, \
                 (const bf16*)rd, ld_rd, r_w_bias, r_r_bias, klen, active, (bf16*)out, ld_o, H, Lmax, scale, append,       \
                 nsplit, split_ws, split_cnt, mo)
    if (DH == 64 && !ring) KV8_LAUNCH(64, false);
    else if (DH == 64 && ring) KV8_LAUNCH(64, true);
    else if (DH == 32 && !ring) KV8_LAUNCH(32, false);
    else if (DH == 32 && ring) KV8_LAUNCH(32, true);
    else return -22;
#undef KV8_LAUNCH
    COMMU_LAUNCH_CHECK();
    return 0;
}
