// Cached decode attention with a SHARED PROMPT PREFIX (gfx950; opt-in, DecodeState(shared_prefix=)).
//
// When every slot of a decoder continues the same opening, the K/V rows of that opening are identical in all B slots.
// Here they are held ONCE: pk / pv bf16 [H][Pcap][DH] (head-major like the cache), P = *prefix_len rows valid (a device
// word: a captured graph serves every later load).  The private cache kc / vc [B][H][Lp][DH] holds what a slot generated:
// row r of slot b is absolute position P + r, klen[b] counts PRIVATE rows.  One step of an active pair (b, h) is
//
//   contract(rows = prefix rows 0 .. P-1 of head h ++ private rows 0 .. klen[b] of (b, h),  dist = (P + klen[b]) - position)
//
// -- the same function as csrc/decode.hip over a cache that holds the prefix B times (relative scores depend on the
// distance only), evaluated as partial softmaxes (o[DH], max, sum) that the pair's LAST ARRIVER merges: decode.hip's
// split-key protocol (write-through stores, drained vmcnt, one agent-scope counter per pair that the combiner resets, no
// spinning).  One launch, two kinds of workgroups:
//
//  prefix workgroups (blockIdx < H * ceil(Pcap / CH) * ceil(B / G)), one per (head, chunk of CH prefix rows, group of G
//    slots): stage the chunk's K and V once in LDS (16-byte loads of whole lines), then every wave takes one slot of the
//    group (G = 4: exactly one): scores in fp32 from qu = (q + u) scale, qv = (q + vb) scale and the distance-table rows
//    P + klen[b] - j from global memory, chunk max and sum, un-normalised P.V from LDS, one record per (pair, chunk), one
//    arrival.  The only workgroup barrier is the one after staging.  Chunks that start at or beyond P exit at once.
//  suffix workgroups, one per (pair, split): decode.hip's kernel over the private rows (distance klen[b] - j, the new
//    token from registers, fused append to private row klen[b], the same chunk rule with nsplit > 1).  With a prefix
//    they always publish a record.
//
// Expected arrivals of a pair = suffix chunks + ceil(P / CH), computed by every arriver from prefix_len and klen[b].
// Inactive slots arrive nowhere and their output rows are not written.
// Records: ws fp32 [B H][nsplit + ceil(Pcap / CH)][DH + 2] (suffix splits first), cnt [B H] zero on entry.
#include "common.h"
#include "commu_hip.h"

namespace {

constexpr int PFX_MAXK = 4224;          // private rows (and prefix + private positions) supported, as commu_decode_attn
constexpr int PFX_CH = 128;             // prefix rows per chunk
// slots per prefix workgroup: one per wave.  Measured (tests/probes/prefix_decode.py's model, 64 slots, ms per iteration,
// unshared 0.312 / 0.731 at P 1000 / 3900): G 16 -> 0.401 / 0.939, 8 -> 0.301 / 0.686, 4 -> 0.262 / 0.548, 2 -> 0.296 / 0.639:
// with more slots per workgroup a wave walks its slots one after the other and the launch is bound by that latency chain;
// the chunk is re-read from L2, not from HBM
constexpr int PFX_G = 4;

__device__ __forceinline__ float oct_sum(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    return v;
}
// sum over the LPR lanes of a row (every lane of them gets it)
template <int LPR>
__device__ __forceinline__ float row_lanes_sum(float s) {
    return (LPR == 8) ? oct_sum(s) : (s + dpp_f<0xB1>(s)) + dpp_f<0x4E>(s + dpp_f<0xB1>(s));
}

// decode.hip's chunk rule: keys per suffix workgroup (>= 512, a multiple of 64) and the number of chunks that hold keys
__device__ __forceinline__ int suffix_chunks(int nall, int nsplit, int& chunk) {
    if (nsplit <= 1) {
        chunk = nall;
        return 1;
    }
    chunk = (nall + nsplit - 1) / nsplit;
    chunk = max(512, (chunk + 63) & ~63);
    return (nall + chunk - 1) / chunk;
}

__device__ __forceinline__ float ld_agent(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the last arriver's merge of a pair's records, feature f: suffix records 0 .. neff-1, prefix records nsplit .. nsplit+npc-1
template <int DH>
__device__ __forceinline__ float merge_records(const float* base, int nsplit, int neff, int npc, int f) {
    constexpr int REC = DH + 2;
    float m = -3.0e38f;
    for (int s = 0; s < neff; ++s) m = fmaxf(m, ld_agent(base + s * REC + DH));
    for (int c = 0; c < npc; ++c) m = fmaxf(m, ld_agent(base + (nsplit + c) * REC + DH));
    float num = 0.f, den = 0.f;
    for (int i = 0; i < neff + npc; ++i) {
        const float* r = base + (i < neff ? i : nsplit + (i - neff)) * REC;
        const float w = __expf(ld_agent(r + DH) - m);
        num += w * ld_agent(r + f);
        den += w * ld_agent(r + DH + 1);
    }
    return num / den;
}

template <int DH, int UNR = 4>
__global__ __launch_bounds__(256) void decode_attn_prefix_kernel(
    const bf16* __restrict__ qkv, int ld_qkv, const bf16* __restrict__ pk, const bf16* __restrict__ pv,
    const int* __restrict__ prefix_len, int Pcap, const bf16* kc, const bf16* vc, const bf16* __restrict__ rd, int ld_rd,
    const float* __restrict__ u, const float* __restrict__ vb, const int* __restrict__ klen,
    const unsigned char* __restrict__ active, bf16* __restrict__ out, int ld_o, int B, int H, int Lp, float scale,
    int append, int nsplit, float* ws, unsigned* cnt) {
    constexpr int LPR = DH / 8;            // lanes per row (8 for DH 64, 4 for DH 32)
    constexpr int RPW = 64 / LPR;          // rows per wave instruction
    constexpr int CH = PFX_CH, G = PFX_G;
    constexpr int NI = CH / RPW;           // wave instructions per chunk
    constexpr int REC = DH + 2;
    // LDS, one block for both roles: prefix [K chunk | V chunk] bf16; suffix [scores PFX_MAXK | partial outputs] fp32
    __shared__ __attribute__((aligned(16))) float smem[2 * CH * 64 / 2];          // 32 KB
    __shared__ float red[8];
    __shared__ int s_last;
    static_assert(PFX_MAXK + 4 * RPW * DH <= 2 * CH * 64 / 2, "suffix LDS fits the block");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int sub = lane % LPR, rowl = lane / LPR;
    const int NCH = (Pcap + CH - 1) / CH, NG = (B + G - 1) / G;
    const int NREC = nsplit + NCH;
    const int P = min(max(prefix_len[0], 0), Pcap);
    const int npc = (P + CH - 1) / CH;
    const int npfx = H * NCH * NG;

    if ((int)blockIdx.x < npfx) {
        // ================================================================ prefix workgroup (h, chunk c, slot group g)
        const int g = blockIdx.x % NG;
        const int t = blockIdx.x / NG;
        const int h = t % H, c = t / H;
        const int j0 = c * CH;
        if (j0 >= P) return;
        const int nrow = min(CH, P - j0);
        bf16* sK = (bf16*)smem;
        bf16* sV = sK + CH * DH;
        {
            const uint4* srcK = (const uint4*)(pk + ((size_t)h * Pcap + j0) * DH);
            const uint4* srcV = (const uint4*)(pv + ((size_t)h * Pcap + j0) * DH);
            constexpr int NS = CH * LPR / 256;          // 16-byte pieces per thread and operand
            uint4 kq[NS], vq[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {                // all loads in flight together; rows beyond P re-read row P - 1
                const int i = tid + 256 * s;
                const int off = min(i / LPR, nrow - 1) * LPR + i % LPR;
                kq[s] = srcK[off];
                vq[s] = srcV[off];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {                // ... and are staged as zeros (their probability is 0: 0 x 0)
                const int i = tid + 256 * s;
                const unsigned m = i / LPR < nrow ? 0xffffffffu : 0u;
                ((uint4*)sK)[i] = make_uint4(kq[s].x & m, kq[s].y & m, kq[s].z & m, kq[s].w & m);
                ((uint4*)sV)[i] = make_uint4(vq[s].x & m, vq[s].y & m, vq[s].z & m, vq[s].w & m);
            }
        }
        __syncthreads();
        float ub[8], vbb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { ub[e] = u[h * DH + 8 * sub + e]; vbb[e] = vb[h * DH + 8 * sub + e]; }
        const bf16* rb = rd + h * DH + 8 * sub;
        const int bend = min(B, (g + 1) * G);
        for (int b = g * G + w; b < bend; b += 4) {          // a wave owns one slot at a time
            if (active != nullptr && !active[b]) continue;
            const int nall = min(klen[b] + 1, Lp);            // private keys, the new token included
            const int dnew = P + nall - 1;                    // the new token's absolute position
            const bf16x8 q8 = ld_bf16x8(qkv + (size_t)b * ld_qkv + h * DH + 8 * sub);
            float qu[8], qv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float q = bf2f(q8[e]);
                qu[e] = (q + ub[e]) * scale;
                qv[e] = (q + vbb[e]) * scale;
            }
            bf16x8 r8[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int jc = min(i * RPW + rowl, nrow - 1);
                r8[i] = ld_bf16x8(rb + (size_t)(dnew - (j0 + jc)) * ld_rd);
            }
            float sc[NI];
            float mx = -3.0e38f;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int jl = i * RPW + rowl;
                const bf16x8 kx = ld_bf16x8(sK + jl * DH + 8 * sub);
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) s += qu[e] * bf2f(kx[e]) + qv[e] * bf2f(r8[i][e]);
                s = row_lanes_sum<LPR>(s);
                sc[i] = s;
                if (jl < nrow) mx = fmaxf(mx, s);
            }
            mx = wave_max(mx);
            float sum = 0.f;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int jl = i * RPW + rowl;
                const float p = (jl < nrow) ? __expf(sc[i] - mx) : 0.f;
                if (sub == 0) sum += p;
                const bf16x8 vx = ld_bf16x8(sV + jl * DH + 8 * sub);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += p * bf2f(vx[e]);
            }
            sum = wave_sum(sum);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int o = LPR; o < 64; o <<= 1) acc[e] += __shfl_xor(acc[e], o, 64);
            const int pair = b * H + h;
            float* rec = ws + ((size_t)pair * NREC + nsplit + c) * REC;
            if (rowl == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) st_agent(rec + 8 * sub + e, acc[e]);
            }
            if (lane == LPR) st_agent(rec + DH, mx);
            if (lane == LPR + 1) st_agent(rec + DH + 1, sum);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's write-through stores are drained
            int last = 0, neff = 1;
            if (lane == 0) {
                int chunk;
                neff = suffix_chunks(nall, nsplit, chunk);
                const unsigned old = __hip_atomic_fetch_add(cnt + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = old == (unsigned)(neff + npc - 1);
                if (last) __hip_atomic_store(cnt + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // next launch
            }
            last = __shfl(last, 0, 64);
            neff = __shfl(neff, 0, 64);
            if (last && lane < DH)
                out[(size_t)b * ld_o + h * DH + lane] =
                    f2bf(merge_records<DH>(ws + (size_t)pair * NREC * REC, nsplit, neff, npc, lane));
        }
        return;
    }

    // ==================================================================== suffix workgroup (pair, split): decode.hip's
    // linear kernel over the private rows
    float* sS = smem;
    float (*sO)[RPW][DH] = (float (*)[RPW][DH])(smem + PFX_MAXK);
    const int sid = blockIdx.x - npfx;
    const int pair = nsplit > 1 ? sid / nsplit : sid;
    const int split = nsplit > 1 ? sid - pair * nsplit : 0;
    const int b = pair / H, h = pair - b * H;
    const int pos = klen[b];                                  // the new token's private row
    const unsigned char act = active != nullptr ? active[b] : (unsigned char)1;
    const bf16* qrow = qkv + (size_t)b * ld_qkv + h * DH + 8 * sub;
    const bf16x8 q8 = ld_bf16x8(qrow);
    const bf16x8 knew = ld_bf16x8(qrow + H * DH), vnew = ld_bf16x8(qrow + 2 * H * DH);
    float ub[8], vbb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ub[e] = u[h * DH + 8 * sub + e]; vbb[e] = vb[h * DH + 8 * sub + e]; }
    if (!act) return;
    const int self = (append && pos < Lp) ? pos : -1;
    if (self >= 0 && tid < 2 * LPR && split == 0) {
        bf16* dst = (bf16*)(tid < LPR ? kc : vc) + (((size_t)b * H + h) * Lp + pos) * DH + 8 * sub;
        st_bf16x8(dst, tid < LPR ? knew : vnew);
    }
    const int nall = min(pos + 1, Lp);
    int chunk;
    const int neff = suffix_chunks(nall, nsplit, chunk);
    if (split >= neff) return;
    const int jlo = split * chunk;
    const int n = min(nall, jlo + chunk);
    const bf16* kb = kc + ((size_t)b * H + h) * Lp * DH + 8 * sub;
    const bf16* vbp = vc + ((size_t)b * H + h) * Lp * DH + 8 * sub;
    const bf16* rb = rd + h * DH + 8 * sub;
    float qu[8], qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float q = bf2f(q8[e]);
        qu[e] = (q + ub[e]) * scale;
        qv[e] = (q + vbb[e]) * scale;
    }
    constexpr int STEP = 4 * RPW * UNR;
    float mx = -3.0e38f;
    {
        bf16x8 kk[UNR], r8[UNR], kn[UNR], rn[UNR];
        auto issue = [&](bf16x8 (&kd)[UNR], bf16x8 (&rdst)[UNR], int j0) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int jc = min(j0 + 4 * RPW * i + rowl, n - 1);
                kd[i] = ld_bf16x8(kb + (size_t)jc * DH);
                rdst[i] = ld_bf16x8(rb + (size_t)((nall - 1) - jc) * ld_rd);          // private distance: klen[b] - j
            }
        };
        auto consume = [&](const bf16x8 (&kd)[UNR], const bf16x8 (&rdst)[UNR], int j0) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int j = j0 + 4 * RPW * i + rowl;
                float s = 0.f;
                const bf16x8 kx = (j == self) ? knew : kd[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) s += qu[e] * bf2f(kx[e]) + qv[e] * bf2f(rdst[i][e]);
                s = row_lanes_sum<LPR>(s);
                if (j < n) {
                    if (sub == 0) sS[j - jlo] = s;
                    mx = fmaxf(mx, s);
                }
            }
        };
        int j0 = jlo + w * RPW;
        if (j0 < n) issue(kk, r8, j0);
        for (; j0 < n; j0 += 2 * STEP) {
            if (j0 + STEP < n) issue(kn, rn, j0 + STEP);
            consume(kk, r8, j0);
            if (j0 + 2 * STEP < n) issue(kk, r8, j0 + 2 * STEP);
            if (j0 + STEP < n) consume(kn, rn, j0 + STEP);
        }
    }
    bf16x8 v8[UNR], vn[UNR];
    auto issue_v = [&](bf16x8 (&vd)[UNR], int j0) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) vd[i] = ld_bf16x8(vbp + (size_t)min(j0 + 4 * RPW * i + rowl, n - 1) * DH);
    };
    if (jlo + w * RPW < n) issue_v(v8, jlo + w * RPW);
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
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto consume_v = [&](const bf16x8 (&vd)[UNR], int j0) {
        float p[UNR];
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int j = j0 + 4 * RPW * i + rowl;
            p[i] = (j < n) ? sS[j - jlo] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            // (the CLAMPED row: a tail lane past n re-reads row n - 1 with p = 0; where that is the new token's row, whose
            //  store may not have landed, 0 x stale bits must not reach acc)
            const bf16x8 vx = (min(j0 + 4 * RPW * i + rowl, n - 1) == self) ? vnew : vd[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += p[i] * bf2f(vx[e]);
        }
    };
    for (int j0 = jlo + w * RPW; j0 < n; j0 += 2 * STEP) {
        if (j0 + STEP < n) issue_v(vn, j0 + STEP);
        consume_v(v8, j0);
        if (j0 + 2 * STEP < n) issue_v(v8, j0 + 2 * STEP);
        if (j0 + STEP < n) consume_v(vn, j0 + STEP);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sO[w][rowl][8 * sub + e] = acc[e];
    __syncthreads();
    float o = 0.f;
    if (tid < DH) {
        for (int ww = 0; ww < 4; ++ww)
            for (int r = 0; r < RPW; ++r) o += sO[ww][r][tid];
    }
    const int expected = neff + npc;
    if (expected == 1) {          // (no prefix and one chunk: nothing to merge)
        if (tid < DH) out[(size_t)b * ld_o + h * DH + tid] = f2bf(o / lsum);
        return;
    }
    // ---- publish (o[DH], max, sum); the last arriver of the pair combines
    float* rec = ws + ((size_t)pair * NREC + split) * REC;
    if (tid < DH) st_agent(rec + tid, o);
    if (tid == DH) st_agent(rec + DH, mx);
    if (tid == DH + 1) st_agent(rec + DH + 1, lsum);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(cnt + pair, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == (unsigned)(expected - 1);
        if (s_last) __hip_atomic_store(cnt + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // next launch
    }
    __syncthreads();
    if (!s_last) return;
    if (tid < DH)
        out[(size_t)b * ld_o + h * DH + tid] = f2bf(merge_records<DH>(ws + (size_t)pair * NREC * REC, nsplit, neff, npc, tid));
}

}  // namespace

extern "C" int commu_decode_prefix_chunk(void) { return PFX_CH; }
extern "C" int commu_decode_prefix_group(void) { return PFX_G; }

extern "C" int commu_decode_attn_prefix(const void* qkv, int ld_qkv, const void* pk, const void* pv, const int* prefix_len,
                                        int Pcap, void* kcache, void* vcache, const void* rd, int ld_rd,
                                        const float* r_w_bias, const float* r_r_bias, const int* klen,
                                        const unsigned char* active, void* out, int ld_o, int B, int H, int DH, int Lp,
                                        float scale, int append, int nsplit, float* ws, unsigned* cnt, hipStream_t stream) {
    if (B <= 0) return 0;
    if (H <= 0 || Lp < 1 || Pcap < 1 || Lp > PFX_MAXK || Pcap > PFX_MAXK - Lp || (ld_qkv % 8) || (ld_rd % 8)) return -22;
    if (nsplit < 1 || nsplit > 16 || ws == nullptr || cnt == nullptr || prefix_len == nullptr || klen == nullptr) return -22;
    if (pk == nullptr || pv == nullptr || (((uintptr_t)pk | (uintptr_t)pv | (uintptr_t)kcache | (uintptr_t)vcache |
                                             (uintptr_t)qkv | (uintptr_t)rd) % 16))
        return -22;
    const long long nblk = (long long)H * ((Pcap + PFX_CH - 1) / PFX_CH) * ((B + PFX_G - 1) / PFX_G) + (long long)B * H * nsplit;
    if (nblk > 0x7fffffffLL) return -22;
    dim3 grid((unsigned)nblk);
    if (DH == 64)
        COMMU_LAUNCH((decode_attn_prefix_kernel<64>), grid, dim3(256), 0, stream, (const bf16*)qkv, ld_qkv, (const bf16*)pk,
                     (const bf16*)pv, prefix_len, Pcap, (const bf16*)kcache, (const bf16*)vcache, (const bf16*)rd, ld_rd,
                     r_w_bias, r_r_bias, klen, active, (bf16*)out, ld_o, B, H, Lp, scale, append, nsplit, ws, cnt);
    else if (DH == 32)
        COMMU_LAUNCH((decode_attn_prefix_kernel<32>), grid, dim3(256), 0, stream, (const bf16*)qkv, ld_qkv, (const bf16*)pk,
                     (const bf16*)pv, prefix_len, Pcap, (const bf16*)kcache, (const bf16*)vcache, (const bf16*)rd, ld_rd,
                     r_w_bias, r_r_bias, klen, active, (bf16*)out, ld_o, B, H, Lp, scale, append, nsplit, ws, cnt);
    else
        return -22;
    COMMU_LAUNCH_CHECK();
    return 0;
}
