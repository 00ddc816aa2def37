// HBM-bound kernels of the Transformer-XL hot path (gfx950): embedding gather/scatter,
// sinusoid table, LayerNorm fwd/bwd, column sums (bias grads), log-softmax + NLL fwd/bwd,
// grad-norm + clipped Adam, bf16 shadow cast / transpose, XL-memory window copy.
// One wave (64 lanes) per row wherever a row reduction is needed; 16-byte accesses.
#include "common.h"
#include "commu_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K1: x[m,:] = E[tok[m],:] * sqrt(D)       (commu/model/model.py:409-420)
__global__ void embed_fwd_kernel(const int64_t* __restrict__ tok, const float* __restrict__ E,
                                 bf16* __restrict__ out, int ldo, int ntok, int D, int V, float scale,
                                 unsigned drop_seed, unsigned drop_thr, float drop_scale) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= ntok) return;
    const int lane = threadIdx.x & 63;
    // an id outside the vocabulary (the reference's nn.Embedding raises IndexError) poisons its row with NaN: the
    // loss of that step is NaN instead of a read through a wild pointer
    const long long id = tok[m];
    const bool bad = id < 0 || id >= V;
    const float* src = E + (size_t)(bad ? 0 : id) * D;
    bf16* dst = out + (size_t)m * ldo;
    const int Dz = min(ldo, (D + 63) & ~63);          // zero-padding contract: columns [D, Dz) are written as 0
    if ((D & 7) == 0 && (ldo & 7) == 0) {          // 8 columns per lane: two 16-byte loads, one 16-byte store
        const DropKey key = drop_key(salted(drop_seed));
        for (int c = lane * 8; c < Dz; c += 512) {
            bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c < D) {
                const f32x4 v0 = *(const f32x4*)(src + c), v1 = *(const f32x4*)(src + c + 4);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float x = bad ? __builtin_nanf("") : (e < 4 ? v0[e & 3] : v1[e & 3]) * scale;
                    if (drop_thr) x = drop_keep(key, (unsigned)m * (unsigned)D + (unsigned)(c + e), drop_thr) ? x * drop_scale : 0.f;
                    o[e] = f2bf(x);
                }
            }
            st_bf16x8(dst + c, o);
        }
        return;
    }
    for (int c = lane * 4; c < Dz; c += 256) {
        if (c >= D) { *(bf16x4*)(dst + c) = (bf16x4){0, 0, 0, 0}; continue; }
        f32x4 v = *(const f32x4*)(src + c);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = bad ? __builtin_nanf("") : v[e] * scale;
            if (drop_thr) x = drop_keep(salted(drop_seed), (unsigned)m * (unsigned)D + (unsigned)(c + e), drop_thr) ? x * drop_scale : 0.f;
            o[e] = f2bf(x);
        }
        *(bf16x4*)(dst + c) = o;
    }
}

// dE[v,:] (+)= scale * sum_{m: tok[m]==v} dX[m,:]   -- one workgroup per vocabulary row, no
// atomics, deterministic (V = 729 rows only; the token list is L2 resident).
__global__ __launch_bounds__(256) void embed_bwd_kernel(
    const int64_t* __restrict__ tok, const bf16* __restrict__ dX, int ldx, float* __restrict__ dE,
    int ntok, int D, float scale, int accumulate, unsigned drop_seed, unsigned drop_thr, float drop_scale) {
    __shared__ int hits[1024];
    __shared__ int nhit;
    const int v = blockIdx.x, tid = threadIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};      // column tid + 256*k, D <= 1024
    for (int base = 0; base < ntok; base += 1024) {
        if (tid == 0) nhit = 0;
        __syncthreads();
        for (int i = tid; i < 1024; i += 256) {
            const int m = base + i;
            if (m < ntok && tok[m] == v) hits[atomicAdd(&nhit, 1)] = m;
        }
        __syncthreads();
        const int n = nhit;
        for (int h = 0; h < n; ++h) {
            const int m = hits[h];
            const bf16* row = dX + (size_t)m * ldx;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = tid + 256 * k;
                if (c < D) {
                    float x = bf2f(row[c]);
                    if (drop_thr) x = drop_keep(salted(drop_seed), (unsigned)m * (unsigned)D + (unsigned)c, drop_thr) ? x * drop_scale : 0.f;
                    acc[k] += x;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = tid + 256 * k;
        if (c < D) {
            float* p = dE + (size_t)v * D + c;
            *p = (accumulate ? *p : 0.f) + acc[k] * scale;
        }
    }
}

// The same sums from a token ORDER (stable argsort of the ids + segment offsets per vocabulary row, computed beside the
// backward pass): workgroup (row v, split s) adds the dX rows of its share of v's tokens -- one row per wave and step,
// 16 bytes per lane, the next row in flight -- and writes slab [s][v][:]; commu_reduce_slabs_f32 folds the S slabs into
// the gradient.  No scan of the token list (the kernel above reads it once per vocabulary row: 382 MB at V = 729), no
// atomics (fp32 LDS atomics cost ~170 cycles per wave instruction here: a table-in-LDS version took 185 us), and the
// order of the additions is fixed.
// Load-balanced form (what runs): a vocabulary row that dominates the batch -- the pad / start id 0 is a quarter of
// the tokens of a real batch -- made "one workgroup per (row, split)" walk thousands of rows in sequence (0.64 ms against
// 0.03 ms on uniform ids).  Two passes over the SORTED token list instead:
//   pass 1: every WAVE takes EMB_CHUNK consecutive sorted tokens and adds their dX rows run by run (a run = equal ids);
//           the sum of the run of id v in chunk c goes to partial row v + c (both grow along the list, so v + c is
//           unique; at most V + nchunks rows);
//   pass 2: row v of dE (+)= scale * sum of its partial rows v + c, c = first .. last chunk that holds a token of v.
// Work per wave is bounded by the chunk, the summation order is fixed, no atomics.
constexpr int EMB_CHUNK = 32;
template <int NC>          // NC 8-element chunks per lane: D <= 512 * NC
__global__ __launch_bounds__(256) void embed_bwd_runs_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ offs, const bf16* __restrict__ dX, int ldx,
    float* __restrict__ part, int ntok, int D, int V, unsigned drop_seed, unsigned drop_thr, float drop_scale) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);          // this wave's chunk
    const long long lo = (long long)c * EMB_CHUNK, hi = min((long long)ntok, lo + EMB_CHUNK);
    if (lo >= hi) return;
    const DropKey key = drop_key(salted(drop_seed));
    // id of the first token of the chunk: the largest v with offs[v] <= lo (binary search over the V + 1 offsets)
    int v = 0;
    {
        int a = 0, b = V;          // offs[a] <= lo < offs[b] is maintained where possible (ids outside [0, V): skipped)
        if (lo < offs[0] || lo >= offs[V]) { a = -1; }
        else {
            while (b - a > 1) {
                const int mid = (a + b) >> 1;
                if (offs[mid] <= lo) a = mid; else b = mid;
            }
        }
        v = a;
    }
    float acc[NC][8];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[cc][e] = 0.f;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    int cnt = 0;          // tokens in the current run
    auto flush = [&](int id) {
        const bool wr = id >= 0 && id < V && cnt > 0;          // (ids outside the table and empty runs: nothing to store)
        cnt = 0;
        float* out = part + (size_t)(wr ? id + c : 0) * D;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int col = lane * 8 + 512 * cc;
            if (!wr) {
            } else if (col + 7 < D) {
                *(f32x4*)(out + col) = (f32x4){acc[cc][0], acc[cc][1], acc[cc][2], acc[cc][3]};
                *(f32x4*)(out + col + 4) = (f32x4){acc[cc][4], acc[cc][5], acc[cc][6], acc[cc][7]};
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (col + e < D) out[col + e] = acc[cc][e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[cc][e] = 0.f;
        }
    };
    long long run_end = (v >= 0 && v < V) ? offs[v + 1] : (lo < offs[0] ? offs[0] : (long long)ntok);
    // four rows in flight per wave (a row is one dependent round trip: token index -> 1 KB of dX)
    constexpr int U = 8;
    for (long long k0 = lo; k0 < hi; k0 += U) {
        long long mm[U];
        bf16x8 x[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) mm[u] = k0 + u < hi ? perm[k0 + u] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int col = lane * 8 + 512 * cc;
                x[u][cc] = (col < D && k0 + u < hi) ? ld_bf16x8(dX + (size_t)mm[u] * ldx + col) : zero8;      // (row padding beyond D is readable)
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long k = k0 + u;
            if (k >= hi) break;
            while (k >= run_end) {          // the run of id v ended before this token: store it, move to the next id
                flush(v);
                v = v < 0 ? 0 : v + 1;
                run_end = v < V ? offs[v + 1] : (long long)ntok;
            }
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int col = lane * 8 + 512 * cc;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float f = bf2f(x[u][cc][e]);
                    if (drop_thr) f = drop_keep(key, (unsigned)mm[u] * (unsigned)D + (unsigned)(col + e), drop_thr) ? f * drop_scale : 0.f;
                    acc[cc][e] += f;
                }
            }
            ++cnt;
        }
    }
    flush(v);
}

// pass 2: dE[v][:] = (accumulate ? dE[v][:] : 0) + scale * sum over the chunks that hold tokens of v of part[v + c][:]
__global__ __launch_bounds__(256) void embed_bwd_fold_kernel(const int64_t* __restrict__ offs, const float* __restrict__ part,
                                                             float* __restrict__ dE, int D, int V, float scale, int accumulate) {
    __shared__ f32x4 red[256];
    const int v = blockIdx.x;
    const long long b0 = offs[v], b1 = offs[v + 1];
    const int c0 = (int)(b0 / EMB_CHUNK), c1 = b1 > b0 ? (int)((b1 - 1) / EMB_CHUNK) : c0 - 1;
    // threads = (column group of 4) x (row lane): a long run (the pad id: hundreds of partial rows) is walked by several
    // row lanes, eight rows in flight each, and folded through LDS in row-lane order
    const int ncg = (D + 3) / 4;                       // column groups per pass (D % 4 == 0)
    const int cgs = ncg < 256 ? ncg : 256;             // column groups handled at once
    const int nrl = 256 / cgs;                         // row lanes
    const int cg = threadIdx.x % cgs, rl = threadIdx.x / cgs;
    for (int colbase = 0; colbase < D; colbase += 4 * cgs) {
        const int col = colbase + 4 * cg;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (col < D && rl < nrl) {
            int c = c0 + rl;
            for (; c + 7 * nrl <= c1; c += 8 * nrl) {
                f32x4 t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = *(const f32x4*)(part + (size_t)(v + c + u * nrl) * D + col);
#pragma unroll
                for (int u = 0; u < 8; ++u) a += t[u];
            }
            for (; c <= c1; c += nrl) a += *(const f32x4*)(part + (size_t)(v + c) * D + col);
        }
        red[threadIdx.x] = a;
        __syncthreads();
        if (rl == 0 && col < D) {
            for (int r = 1; r < nrl; ++r) a += red[r * cgs + cg];
            a *= scale;
            f32x4* dst = (f32x4*)(dE + (size_t)v * D + col);
            if (accumulate) a += *dst;
            *dst = a;
        }
        __syncthreads();
    }
}

// K2: sinusoid table indexed by DISTANCE d (pos = d): out[d] = [sin(d f) | cos(d f)]
// (commu/model/model.py:142-147; the reference's row k of pos_emb is distance klen-1-k).
__global__ void posemb_kernel(const float* __restrict__ inv_freq, bf16* __restrict__ out, int ld,
                              int K, int D, int clamp_len, unsigned drop_seed, unsigned drop_thr, float drop_scale) {
    const int half = D >> 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= K * half) return;
    const int d = idx / half, i = idx - d * half;
    // (model.py:581-582: positions above clamp_len share its row; the dropout mask below stays per table row)
    const float ang = (float)(clamp_len > 0 ? min(d, clamp_len) : d) * inv_freq[i];
    float sv = sinf(ang), cv = cosf(ang);
    if (drop_thr) {
        sv = drop_keep(salted(drop_seed), (unsigned)d * (unsigned)D + (unsigned)i, drop_thr) ? sv * drop_scale : 0.f;
        cv = drop_keep(salted(drop_seed), (unsigned)d * (unsigned)D + (unsigned)(half + i), drop_thr) ? cv * drop_scale : 0.f;
    }
    out[(size_t)d * ld + i] = f2bf(sv);
    out[(size_t)d * ld + half + i] = f2bf(cv);
    const int Dz = min(ld, (D + 63) & ~63);
    for (int c = D + i; c < Dz; c += half) out[(size_t)d * ld + c] = f2bf(0.f);      // zero padding [D, Dz)
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over D (eps inside sqrt, biased variance; torch.nn.LayerNorm, model.py:171,214,352,179)
constexpr int LN_MAXC = 2;   // D <= 1024: lane owns 8-element chunks at column 8*lane + 512*c

__global__ __launch_bounds__(256) void layernorm_fwd_kernel(
    const bf16* __restrict__ z, int ldz, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16* __restrict__ y, int ldy, float* __restrict__ mean,
    float* __restrict__ rstd, int rows, int D, float eps, bf16* __restrict__ ydrop, int ldyd,
    unsigned drop_seed, unsigned drop_thr, float drop_scale) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    // zero-padding contract (D % 4 == 0): columns [D, Dz), Dz = roundup(D, 64) clipped to the row pitch, are
    // padding -- ignored on input, written as 0 on output.  A 4-element group is wholly valid or wholly padding.
    const int Dz = min(ldy, (D + 63) & ~63);
    float x[LN_MAXC][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int col = lane * 8 + 512 * c;
        if (col < D) {
            bf16x8 v = ld_bf16x8(z + (size_t)row * ldz + col);
            const bool hi = col + 4 < D;
#pragma unroll
            for (int e = 0; e < 8; ++e) { x[c][e] = (e < 4 || hi) ? bf2f(v[e]) : 0.f; s += x[c][e]; }
        }
    }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int col = lane * 8 + 512 * c;
        if (col < D) {
            const bool hi = col + 4 < D;
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = x[c][e] - mu; q += (e < 4 || hi) ? d * d : 0.f; }
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int col = lane * 8 + 512 * c;
        if (col < D) {
            const bool hi = col + 4 < D;
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            const f32x4 g0 = *(const f32x4*)(gamma + col), g1 = hi ? *(const f32x4*)(gamma + col + 4) : z4;
            const f32x4 b0 = *(const f32x4*)(beta + col), b1 = hi ? *(const f32x4*)(beta + col + 4) : z4;
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[c][e] = (x[c][e] - mu) * rs * g0[e] + b0[e];
                x[c][4 + e] = hi ? (x[c][4 + e] - mu) * rs * g1[e] + b1[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(x[c][e]);
            st_bf16x8(y + (size_t)row * ldy + col, o);
        } else if (col < Dz) {
            st_bf16x8(y + (size_t)row * ldy + col, zero8);
        }
    }
    if (ydrop != nullptr) {
#pragma unroll
        for (int c = 0; c < LN_MAXC; ++c) {
            const int col = lane * 8 + 512 * c;
            if (col < D) {
                const bool hi = col + 4 < D;
                bf16x8 od;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    od[e] = f2bf(((e < 4 || hi) && drop_keep(salted(drop_seed), (unsigned)row * (unsigned)D + (unsigned)(col + e), drop_thr))
                                     ? x[c][e] * drop_scale : 0.f);
                st_bf16x8(ydrop + (size_t)row * ldyd + col, od);
            } else if (col < min(ldyd, (D + 63) & ~63)) {
                st_bf16x8(ydrop + (size_t)row * ldyd + col, zero8);
            }
        }
    }
}

// dz = rstd * (g*dy - mean(g*dy) - xhat * mean(g*dy*xhat));  partial column sums of
// dy*xhat (dgamma), dy (dbeta) and dz (bias grad of the Linear feeding the LN) per block.
constexpr int LNB_ROWS = 32;   // rows per block (8 per wave: 8192 waves at 65536 rows, two per SIMD slot pair)
constexpr int LNB_WROWS = LNB_ROWS / 4;

// Bandwidth kernel (2 reads + 2 writes of a [rows, D] bf16 tensor): a wave walks its rows TWO at a time -- two independent
// reduction chains -- with the next pair's operands and row statistics already in flight (4 rows x 2 x 16 bytes per lane).
// ADD: the incoming gradient is dy + dy2 (the residual branch's gradient as a second addend HERE instead of an auxiliary
// operand in the epilogue of the GEMM that produced dy: that GEMM then takes the pipelined epilogue)
template <int NC, bool ADD = false>          // NC 8-element chunks per lane: D <= 512 * NC
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(
    const bf16* __restrict__ dy, int lddy, const bf16* __restrict__ dy2, int lddy2, const bf16* __restrict__ z, int ldz,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    bf16* __restrict__ dz, int lddz, float* __restrict__ part, int rows, int D, bf16* __restrict__ dzm,
    int lddzm, unsigned drop_seed, unsigned drop_thr, float drop_scale) {
    __shared__ float red[4][3][512 * NC];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float ag[NC][8], ab[NC][8], az[NC][8], gm[NC][8];
    bool act[NC], hi[NC], padc[NC];          // chunk has valid columns / its upper 4 are valid / pure padding to zero
    const int Dz = min(lddz, (D + 63) & ~63);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        act[c] = lane * 8 + 512 * c < D;
        hi[c] = lane * 8 + 512 * c + 4 < D;
        padc[c] = !act[c] && lane * 8 + 512 * c < Dz;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ag[c][e] = ab[c][e] = az[c][e] = 0.f;
            const int col = lane * 8 + 512 * c + e;
            gm[c][e] = (col < D) ? gamma[col] : 0.f;
        }
    }
    const int r0 = blockIdx.x * LNB_ROWS + w * LNB_WROWS;
    const int nr = min(LNB_WROWS, rows - r0);
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const DropKey key = drop_key(salted(drop_seed));
    const float invD = 1.f / (float)D;
    bf16x8 vz[2][NC], vd[2][NC], nz[2][NC], nd[2][NC], ve[2][ADD ? NC : 1], ne[2][ADD ? NC : 1];
    float vmu[2], vrs[2], nmu[2], nrs[2];
    auto fetch = [&](int row) {          // rows row, row+1 (clamped: a pair past the end re-reads the last row, unused)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = min(row + u, rows - 1);
            nmu[u] = mean[r];
            nrs[u] = rstd[r];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int col = lane * 8 + 512 * c;
                nz[u][c] = act[c] ? ld_bf16x8(z + (size_t)r * ldz + col) : zero8;
                nd[u][c] = act[c] ? ld_bf16x8(dy + (size_t)r * lddy + col) : zero8;
                if (ADD) ne[u][c] = act[c] ? ld_bf16x8(dy2 + (size_t)r * lddy2 + col) : zero8;
            }
        }
    };
    if (nr > 0) fetch(r0);
    for (int rr = 0; rr < nr; rr += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            vmu[u] = nmu[u];
            vrs[u] = nrs[u];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                vz[u][c] = nz[u][c];
                vd[u][c] = nd[u][c];
                if (ADD) ve[u][c] = ne[u][c];
            }
        }
        if (rr + 2 < nr) fetch(r0 + rr + 2);          // the next pair's loads fly under this pair's reductions
        float xh[2][NC][8], gy[2][NC][8], s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool live = rr + u < nr;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool ok = live && act[c] && (e < 4 || hi[c]);
                    const float d = ok ? (ADD ? bf2f(vd[u][c][e]) + bf2f(ve[u][c][e]) : bf2f(vd[u][c][e])) : 0.f;
                    xh[u][c][e] = ok ? (bf2f(vz[u][c][e]) - vmu[u]) * vrs[u] : 0.f;
                    gy[u][c][e] = d * gm[c][e];
                    s1[u] += gy[u][c][e];
                    s2[u] += gy[u][c][e] * xh[u][c][e];
                    ag[c][e] += d * xh[u][c][e];
                    ab[c][e] += d;
                }
            }
        }
        float m1[2], m2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) { m1[u] = wave_sum(s1[u]) * invD; m2[u] = wave_sum(s2[u]) * invD; }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = r0 + rr + u;
            if (rr + u >= nr) break;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int col = lane * 8 + 512 * c;
                if (act[c]) {
                    bf16x8 o, om;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = (e < 4 || hi[c]) ? vrs[u] * (gy[u][c][e] - m1[u] - xh[u][c][e] * m2[u]) : 0.f;
                        o[e] = f2bf(v);
                        if (dzm != nullptr) {
                            // gradient w.r.t. the pre-dropout Linear output that fed this LayerNorm
                            const bool keep = drop_keep(key, (unsigned)row * (unsigned)D + (unsigned)(col + e), drop_thr);
                            om[e] = f2bf(keep ? v * drop_scale : 0.f);
                            az[c][e] += bf2f(om[e]);
                        } else {
                            az[c][e] += bf2f(o[e]);
                        }
                    }
                    st_bf16x8(dz + (size_t)row * lddz + col, o);
                    if (dzm != nullptr) st_bf16x8(dzm + (size_t)row * lddzm + col, om);
                } else if (padc[c]) {
                    st_bf16x8(dz + (size_t)row * lddz + col, zero8);
                    if (dzm != nullptr) st_bf16x8(dzm + (size_t)row * lddzm + col, zero8);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = lane * 8 + 512 * c + e;
            if (col < D) { red[w][0][col] = ag[c][e]; red[w][1][col] = ab[c][e]; red[w][2][col] = az[c][e]; }
        }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * D; i += 256) {
        const int k = i / D, col = i - k * D;
        part[((size_t)blockIdx.x * 3 + k) * D + col] =
            red[0][k][col] + red[1][k][col] + red[2][k][col] + red[3][k][col];
    }
}

// Column sums  out[c] += sum_r X[r, c]  WITHOUT atomics (fp32 atomics on ~100 contended addresses made these the slowest
// bandwidth kernels of the step: 65-110 us for 2-130 MB; and the result depended on the arrival order).  Two passes:
//   pass 1: workgroup (bx, by) sums row slab by of a 512-column (bf16, 16-byte loads) / 256-column (fp32) strip and
//           STORES its partial row to ws[by][c];
//   pass 2: out[c] += sum over the slabs, in slab order (deterministic).
// Small inputs (LayerNorm partials, per-tile bias sums: a few MB) take pass 2 alone on the input itself.
template <typename T>
__global__ __launch_bounds__(256) void colsum_slab_kernel(const T* __restrict__ X, int ldx, int rows, int cols,
                                                          float* __restrict__ ws, int rows_per_block) {
    constexpr int V = sizeof(T) == 2 ? 8 : 4;          // elements per 16-byte load
    __shared__ float red[4][64 * V];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0 = blockIdx.x * 64 * V + lane * V;
    const int rbeg = blockIdx.y * rows_per_block, rend = min(rows, rbeg + rows_per_block);
    float a[V];
#pragma unroll
    for (int e = 0; e < V; ++e) a[e] = 0.f;
    if (c0 < cols) {          // (cols rounded up to V by the caller: whole 16-byte chunks inside the row pitch)
        int r = rbeg + w;
        for (; r + 28 < rend; r += 32) {          // eight rows in flight per wave
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(X + (size_t)(r + 4 * u) * ldx + c0);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if constexpr (V == 8) {
                    const bf16x8 b = __builtin_bit_cast(bf16x8, v[u]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[e] += bf2f(b[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] += v[u][e];
                }
            }
        }
        for (; r < rend; r += 4) {
            const f32x4 v = *(const f32x4*)(X + (size_t)r * ldx + c0);
            if constexpr (V == 8) {
                const bf16x8 b = __builtin_bit_cast(bf16x8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += bf2f(b[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] += v[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) red[w][lane * V + e] = a[e];
    __syncthreads();
    for (int t = threadIdx.x; t < 64 * V; t += 256) {
        const int c = blockIdx.x * 64 * V + t;
        if (c < cols) ws[(size_t)blockIdx.y * cols + c] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
    }
}

// out[c] += sum_{r < rows} X[r * ldx + c] for fp32 X, fixed order; up to three planes (blockIdx.y: X + z * plane,
// out = o0 / o1 / o2, a null output is skipped).  One workgroup per SIXTEEN columns: 64 row lanes x 4 float4 column lanes
// (with 64 columns per workgroup a 512-column sum ran on 8 workgroups that each walked up to 1024 partial rows 16 at a
// time: 53 us of dependent round trips on a 256-CU chip; 32-96 workgroups and a quarter of the trips: a few us).
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ X, int ldx, size_t plane, int rows,
                                                           int cols, float* __restrict__ o0, float* __restrict__ o1,
                                                           float* __restrict__ o2, float alpha) {
    __shared__ f32x4 red[64][4];
    const int z = blockIdx.y;
    float* out = z == 0 ? o0 : (z == 1 ? o1 : o2);
    if (out == nullptr) return;
    const float* P = X + (size_t)z * plane;
    const int rl = threadIdx.x >> 2, cl = threadIdx.x & 3;
    const int c0 = blockIdx.x * 16 + cl * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c0 < cols) {
        const bool vec = c0 + 3 < cols && ((ldx & 3) == 0) && ((((size_t)P) & 15) == 0);
        int r = rl;
        if (vec) {
            for (; r + 192 < rows; r += 256) {          // four loads in flight
                f32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(P + (size_t)(r + 64 * u) * ldx + c0);
#pragma unroll
                for (int u = 0; u < 4; ++u) a += v[u];
            }
            for (; r < rows; r += 64) a += *(const f32x4*)(P + (size_t)r * ldx + c0);
        } else {
            for (; r < rows; r += 64)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + e < cols) a[e] += P[(size_t)r * ldx + c0 + e];
        }
    }
    red[rl][cl] = a;
    __syncthreads();
#pragma unroll
    for (int st = 32; st >= 4; st >>= 1) {          // fixed tree over the row lanes
        if (rl < st) red[rl][cl] += red[rl + st][cl];
        __syncthreads();
    }
    if (threadIdx.x < 16) {
        const int c = blockIdx.x * 16 + threadIdx.x;
        if (c < cols) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += red[k][threadIdx.x >> 2][threadIdx.x & 3];
            out[c] += alpha * s;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K10: nll[m] = logsumexp(logits[m, :V]) - logits[m, target[m]]   (model.py:64-73)
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, int ldl,
                                                     const int64_t* __restrict__ target,
                                                     float* __restrict__ nll, float* __restrict__ lse,
                                                     int rows, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    float mx = -3.0e38f;
    for (int c = lane; c < V; c += 64) mx = fmaxf(mx, p[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < V; c += 64) s += expf(p[c] - mx);
    s = wave_sum(s);
    const float l = mx + logf(s);
    if (lane == 0) {
        lse[row] = l;
        const long long tg = target[row];          // (outside [0, V): NaN, the reference's gather would raise)
        nll[row] = (tg >= 0 && tg < V) ? l - p[tg] : __builtin_nanf("");
    }
}

// The same for rows of at most 768 logits with a 16-byte aligned stride (the model's: 729 of 768): the row is read ONCE,
// 16 bytes per lane and load, and kept in registers for both passes.
__global__ __launch_bounds__(256) void ce_fwd_vec_kernel(const float* __restrict__ logits, int ldl,
                                                         const int64_t* __restrict__ target, float* __restrict__ nll,
                                                         float* __restrict__ lse, int rows, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    f32x4 x[3];
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = 4 * lane + 256 * k;
        x[k] = c < ldl ? *(const f32x4*)(p + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e >= V) x[k][e] = -3.0e38f;
            mx = fmaxf(mx, x[k][e]);
        }
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += (4 * lane + 256 * k + e < V) ? expf(x[k][e] - mx) : 0.f;
    s = wave_sum(s);
    const float l = mx + logf(s);
    if (lane == 0) {
        lse[row] = l;
        const long long tg = target[row];          // (outside [0, V): NaN, the reference's gather would raise)
        nll[row] = (tg >= 0 && tg < V) ? l - p[tg] : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void ce_bwd_vec_kernel(const float* __restrict__ logits, int ldl,
                                                         const int64_t* __restrict__ target,
                                                         const float* __restrict__ lse, const float* __restrict__ g,
                                                         bf16* __restrict__ dlogits, int ldd, int rows, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    bf16* o = dlogits + (size_t)row * ldd;
    const float l = lse[row], gr = g[row];
    const int t = (int)target[row];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = 4 * lane + 256 * k;
        if (c >= ldd) break;
        const f32x4 x = c < ldl ? *(const f32x4*)(p + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        bf16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] = f2bf(c + e < V ? gr * (expf(x[e] - l) - (c + e == t ? 1.f : 0.f)) : 0.f);
        *(bf16x4*)(o + c) = v;
    }
}

// dlogits[m, n] = g[m] * (softmax(logits[m])[n] - [n == target[m]]), bf16, zero in pad columns
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, int ldl,
                                                     const int64_t* __restrict__ target,
                                                     const float* __restrict__ lse,
                                                     const float* __restrict__ g,
                                                     bf16* __restrict__ dlogits, int ldd, int rows,
                                                     int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    bf16* o = dlogits + (size_t)row * ldd;
    const float l = lse[row], gr = g[row];
    const int t = (int)target[row];
    for (int c = lane; c < ldd; c += 64) {
        float v = 0.f;
        if (c < V) v = gr * (expf(p[c] - l) - (c == t ? 1.f : 0.f));
        o[c] = f2bf(v);
    }
}

// ---------------------------------------------------------------------------------------------
// The loss with options (not in the reference): label smoothing eps in [0, 1) and z-loss zeta >= 0.  Per row, V real tokens,
//   nll    = lse - l_t                         (written whatever the options: what evaluation and the logs report)
//   smooth = lse - sum_{j<V} l_j / V           (the cross entropy against the uniform distribution over the V tokens)
//   loss   = (1 - eps) nll + eps smooth + zeta lse^2
//   dl_j   = g [(1 + 2 zeta lse) softmax_j - (1 - eps) [j == t] - eps / V],  j < V;  0 in the pad columns
// The kernels are ce_fwd* / ce_bwd* with one more accumulator (sum l_j, from the sweep that feeds the exponentials) and one
// more multiply-add per element; max, sum and lse are computed by the same operations in the same order, so eps = zeta = 0
// gives the plain kernels' bits.
__device__ __forceinline__ void ce_opts_row_out(const float* __restrict__ p, const int64_t* __restrict__ target,
                                                float* __restrict__ loss, float* __restrict__ nll,
                                                float* __restrict__ lse, int row, int V, float l, float sl, float eps,
                                                float zeta) {
    lse[row] = l;
    const long long tg = target[row];          // (outside [0, V): NaN, as ce_fwd)
    const float n = (tg >= 0 && tg < V) ? l - p[tg] : __builtin_nanf("");
    nll[row] = n;
    const float sm = l - sl / (float)V;
    loss[row] = ((1.f - eps) * n + eps * sm) + zeta * (l * l);
}

__global__ __launch_bounds__(256) void ce_fwd_opts_kernel(const float* __restrict__ logits, int ldl,
                                                          const int64_t* __restrict__ target, float* __restrict__ loss,
                                                          float* __restrict__ nll, float* __restrict__ lse, int rows, int V,
                                                          float eps, float zeta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    float mx = -3.0e38f;
    for (int c = lane; c < V; c += 64) mx = fmaxf(mx, p[c]);
    mx = wave_max(mx);
    float s = 0.f, sl = 0.f;
    for (int c = lane; c < V; c += 64) {
        const float x = p[c];
        s += expf(x - mx);
        sl += x;
    }
    s = wave_sum(s);
    sl = wave_sum(sl);
    if (lane == 0) ce_opts_row_out(p, target, loss, nll, lse, row, V, mx + logf(s), sl, eps, zeta);
}

// rows of at most 768 logits with a 16-byte aligned stride: read ONCE into registers (as ce_fwd_vec_kernel)
__global__ __launch_bounds__(256) void ce_fwd_opts_vec_kernel(const float* __restrict__ logits, int ldl,
                                                              const int64_t* __restrict__ target, float* __restrict__ loss,
                                                              float* __restrict__ nll, float* __restrict__ lse, int rows,
                                                              int V, float eps, float zeta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    f32x4 x[3];
    float mx = -3.0e38f, sl = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = 4 * lane + 256 * k;
        x[k] = c < ldl ? *(const f32x4*)(p + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e >= V) x[k][e] = -3.0e38f;
            else sl += x[k][e];
            mx = fmaxf(mx, x[k][e]);
        }
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += (4 * lane + 256 * k + e < V) ? expf(x[k][e] - mx) : 0.f;
    s = wave_sum(s);
    sl = wave_sum(sl);
    if (lane == 0) ce_opts_row_out(p, target, loss, nll, lse, row, V, mx + logf(s), sl, eps, zeta);
}

// per row: a = 1 + 2 zeta lse scales the softmax; the target column loses (1 - eps) + eps / V, every other one eps / V
__global__ __launch_bounds__(256) void ce_bwd_opts_vec_kernel(const float* __restrict__ logits, int ldl,
                                                              const int64_t* __restrict__ target,
                                                              const float* __restrict__ lse, const float* __restrict__ g,
                                                              bf16* __restrict__ dlogits, int ldd, int rows, int V, float eps,
                                                              float zeta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    bf16* o = dlogits + (size_t)row * ldd;
    const float l = lse[row], gr = g[row];
    const int t = (int)target[row];
    const float a = 1.f + 2.f * zeta * l, u = eps / (float)V, ut = (1.f - eps) + u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = 4 * lane + 256 * k;
        if (c >= ldd) break;
        const f32x4 x = c < ldl ? *(const f32x4*)(p + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        bf16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] = f2bf(c + e < V ? gr * (a * expf(x[e] - l) - (c + e == t ? ut : u)) : 0.f);
        *(bf16x4*)(o + c) = v;
    }
}

__global__ __launch_bounds__(256) void ce_bwd_opts_kernel(const float* __restrict__ logits, int ldl,
                                                          const int64_t* __restrict__ target, const float* __restrict__ lse,
                                                          const float* __restrict__ g, bf16* __restrict__ dlogits, int ldd,
                                                          int rows, int V, float eps, float zeta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = logits + (size_t)row * ldl;
    bf16* o = dlogits + (size_t)row * ldd;
    const float l = lse[row], gr = g[row];
    const int t = (int)target[row];
    const float a = 1.f + 2.f * zeta * l, u = eps / (float)V, ut = (1.f - eps) + u;
    for (int c = lane; c < ldd; c += 64) {
        float v = 0.f;
        if (c < V) v = gr * (a * expf(p[c] - l) - (c == t ? ut : u));
        o[c] = f2bf(v);
    }
}

// ---------------------------------------------------------------------------------------------
// Per-family NLL: sum[k] / count[k] over the rows whose target is of class k (class_of_token[target]) and is not the pad id.
// Deterministic: block b takes rows b * 256 + tid, + nblk * 256, ... one after the other, a butterfly joins the lanes, the
// four waves add in order, and one final workgroup adds the blocks' partials in order.  No atomics.
#define NLL_CLASSES_MAX 8
__global__ __launch_bounds__(256) void nll_by_class_partial_kernel(const float* __restrict__ nll, const int64_t* __restrict__ target,
                                                                   const int* __restrict__ class_of_token, int V, int C, int pad,
                                                                   int rows, float* __restrict__ part_sum,
                                                                   int* __restrict__ part_cnt) {
    __shared__ float rs[4][NLL_CLASSES_MAX];
    __shared__ int rc[4][NLL_CLASSES_MAX];
    float acc[NLL_CLASSES_MAX];
    int cnt[NLL_CLASSES_MAX];
#pragma unroll
    for (int k = 0; k < NLL_CLASSES_MAX; ++k) acc[k] = 0.f, cnt[k] = 0;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
        const long long t = target[r];
        if (t < 0 || t >= V || t == pad) continue;
        const int cls = class_of_token[t];
        const float v = nll[r];
#pragma unroll
        for (int k = 0; k < NLL_CLASSES_MAX; ++k)
            if (cls == k) acc[k] += v, cnt[k] += 1;
    }
#pragma unroll
    for (int k = 0; k < NLL_CLASSES_MAX; ++k) {
        acc[k] = wave_sum(acc[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o, 64);
        if ((threadIdx.x & 63) == 0) rs[threadIdx.x >> 6][k] = acc[k], rc[threadIdx.x >> 6][k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int k = threadIdx.x;
        part_sum[(size_t)blockIdx.x * C + k] = ((rs[0][k] + rs[1][k]) + rs[2][k]) + rs[3][k];
        part_cnt[(size_t)blockIdx.x * C + k] = rc[0][k] + rc[1][k] + rc[2][k] + rc[3][k];
    }
}
__global__ void nll_by_class_final_kernel(const float* __restrict__ part_sum, const int* __restrict__ part_cnt, int nblk, int C,
                                          float* __restrict__ sum, int* __restrict__ count) {
    const int k = threadIdx.x;
    if (k >= C) return;
    float s = 0.f;
    int n = 0;
    for (int b = 0; b < nblk; ++b) s += part_sum[(size_t)b * C + k], n += part_cnt[(size_t)b * C + k];
    sum[k] = s;
    count[k] = n;
}

// ---------------------------------------------------------------------------------------------
// K12/K13: global grad norm (deterministic two-stage) and clipped Adam on the flat buffers
// (train.py:159-169; torch.optim.Adam defaults; clip_grad_norm_ coefficient = min(1, c/(n+1e-6)))
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, size_t n,
                                                            float* __restrict__ part) {
    __shared__ float red[4];
    float s = 0.f;
    const size_t step = (size_t)gridDim.x * 1024;
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    for (; i + 3 * step + 3 < n; i += 4 * step) {          // four independent 16-byte loads in flight per lane
        const f32x4 v0 = *(const f32x4*)(g + i), v1 = *(const f32x4*)(g + i + step), v2 = *(const f32x4*)(g + i + 2 * step),
                    v3 = *(const f32x4*)(g + i + 3 * step);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += v0[e] * v0[e] + v1[e] * v1[e] + v2[e] * v2[e] + v3[e] * v3[e];
    }
    for (; i < n; i += step) {
        if (i + 3 < n) {
            f32x4 v = *(const f32x4*)(g + i);
            s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        } else {
            for (size_t j = i; j < n; ++j) s += g[j] * g[j];
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void sumsq_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = sqrtf(s);     // out[0] = total L2 norm
}

// One Adam update of four consecutive elements (16-byte loads / stores: whole lines per wave instruction -- with one dword per
// lane and instruction the four pieces of a 16-byte unit left in four store instructions and the kernel wrote 1.3x its bytes).
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, bf16* __restrict__ pb, size_t n, float coef, float step,
                                            float isb2, float b1, float b2, float eps, bool vec) {
    // (vec = false: a caller's slice that does not start on a 16-byte boundary -- same arithmetic, one element at a time)
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
        if (vec && i + 3 < n) {
            const f32x4 g4 = *(const f32x4*)(g + i), m4 = *(const f32x4*)(m + i), v4 = *(const f32x4*)(v + i), p4 = *(const f32x4*)(p + i);
            f32x4 mo, vo, po;
            bf16x4 pbo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gr = g4[e] * coef;
                const float mm = b1 * m4[e] + (1.f - b1) * gr;
                const float vv = b2 * v4[e] + (1.f - b2) * gr * gr;
                mo[e] = mm;
                vo[e] = vv;
                po[e] = p4[e] - step * mm / (sqrtf(vv) * isb2 + eps);
                pbo[e] = f2bf(po[e]);
            }
            *(f32x4*)(m + i) = mo;
            *(f32x4*)(v + i) = vo;
            *(f32x4*)(p + i) = po;
            if (pb) *(bf16x4*)(pb + i) = pbo;
        } else {
            for (size_t j = i; j < n && j < i + 4; ++j) {
                const float gr = g[j] * coef;
                const float mm = b1 * m[j] + (1.f - b1) * gr;
                const float vv = b2 * v[j] + (1.f - b2) * gr * gr;
                m[j] = mm;
                v[j] = vv;
                const float np = p[j] - step * mm / (sqrtf(vv) * isb2 + eps);
                p[j] = np;
                if (pb) pb[j] = f2bf(np);
            }
        }
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16* __restrict__ pb, size_t n, float lr, float b1,
                                                   float b2, float eps, float bc1, float bc2,
                                                   const float* __restrict__ gnorm, float clip, bool vec) {
    float coef = 1.f;
    if (gnorm != nullptr && clip > 0.f) coef = fminf(1.f, clip / (gnorm[0] + 1e-6f));
    adam_update(p, g, m, v, pb, n, coef, lr / bc1, 1.f / sqrtf(bc2), b1, b2, eps, vec);
}

// the same step with lr and the two bias corrections read from DEVICE memory (scal = {lr, 1 - b1^t, 1 - b2^t}): what a
// hipGraph-captured optimiser step replays -- the host refreshes the three floats before every replay
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       bf16* __restrict__ pb, size_t n, const float* __restrict__ scal,
                                                       float b1, float b2, float eps,
                                                       const float* __restrict__ gnorm, float clip, bool vec) {
    float coef = 1.f;
    if (gnorm != nullptr && clip > 0.f) coef = fminf(1.f, clip / (gnorm[0] + 1e-6f));
    const float lr = scal[0], bc1 = scal[1], bc2 = scal[2];
    adam_update(p, g, m, v, pb, n, coef, lr / bc1, 1.f / sqrtf(bc2), b1, b2, eps, vec);
}

__global__ void scale_clip_kernel(float* __restrict__ g, size_t n, const float* __restrict__ gnorm, float clip) {
    const float coef = fminf(1.f, clip / (gnorm[0] + 1e-6f));
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        g[i] *= coef;
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = f2bf(in[i]);
}
__global__ void cast_bf16_f32_kernel(const bf16* __restrict__ in, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = bf2f(in[i]);
}

// out[c, r] = in[r, c]  (bf16 weight shadows W^T for the dX GEMMs); 64x64 tiles through LDS
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16* __restrict__ in, int ldi,
                                                             bf16* __restrict__ out, int ldo, int rows,
                                                             int cols) {
    __shared__ bf16 t[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const int r = i >> 6, c = i & 63;
        t[r][c] = (r0 + r < rows && c0 + c < cols) ? in[(size_t)(r0 + r) * ldi + c0 + c] : f2bf(0.f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (c0 + c < cols && r0 + r < rows) out[(size_t)(c0 + c) * ldo + r0 + r] = t[r][c];
    }
}

// same with an fp32 source (master weights -> transposed bf16 shadow in one pass)
__global__ __launch_bounds__(256) void transpose_f32_bf16_kernel(const float* __restrict__ in, int ldi,
                                                                 bf16* __restrict__ out, int ldo,
                                                                 int rows, int cols) {
    __shared__ float t[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const int r = i >> 6, c = i & 63;
        t[r][c] = (r0 + r < rows && c0 + c < cols) ? in[(size_t)(r0 + r) * ldi + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (c0 + c < cols && r0 + r < rows) out[(size_t)(c0 + c) * ldo + r0 + r] = f2bf(t[r][c]);
    }
}

// g[m] = (target[m] != pad) ? scale / count : 0      (autograd of the masked mean, train.py:148-149)
__global__ void loss_grad_kernel(const int64_t* __restrict__ target, int n, int pad,
                                 const int* __restrict__ cnt, float scale, float* __restrict__ g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = (target[i] != pad) ? scale / (float)max(cnt[0], 1) : 0.f;
}

// sum of nll over non-pad targets (+ count): the forward of the masked mean
__global__ __launch_bounds__(256) void masked_sum_kernel(const float* __restrict__ nll,
                                                         const int64_t* __restrict__ target, int n,
                                                         int pad, float* __restrict__ sum,
                                                         int* __restrict__ cnt) {
    float s = 0.f;
    int c = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (target[i] != pad) { s += nll[i]; ++c; }
    s = wave_sum(s);
    c = (int)wave_sum((float)c);
    if ((threadIdx.x & 63) == 0) { atomicAdd(sum, s); if (c) atomicAdd(cnt, c); }
}
__global__ void masked_mean_final_kernel(const float* sum, const int* cnt, float scale, float* out) {
    // no non-pad target: the reference's `loss[target != pad].mean()` of an empty selection is NaN (and its gradient
    // is all zeros, which loss_grad produces anyway)
    out[0] = cnt[0] > 0 ? scale * sum[0] / (float)cnt[0] : __builtin_nanf("");
}

// Column-grouped forms: element i of a [T, B] tensor belongs to micro-batch (i % B) / Bc.  They let ONE forward / backward
// over all B columns stand for the reference's `batch_chunk` micro-batches (train.py:136-155: each micro-batch's loss is
// the mean over ITS non-pad targets, divided by batch_chunk): out = scale * sum_g mean_g, g[m] = scale / count_{group(m)}.
constexpr int MAX_GROUPS = 16;
__global__ __launch_bounds__(256) void masked_sum_groups_kernel(const float* __restrict__ nll,
                                                                const int64_t* __restrict__ target, int n, int pad, int B,
                                                                int Bc, int G, float* __restrict__ sum,
                                                                int* __restrict__ cnt) {
    __shared__ float ss[MAX_GROUPS];
    __shared__ int sc[MAX_GROUPS];
    if (threadIdx.x < MAX_GROUPS) { ss[threadIdx.x] = 0.f; sc[threadIdx.x] = 0; }
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (target[i] != pad) {
            const int g = (i % B) / Bc;
            atomicAdd(&ss[g], nll[i]);
            atomicAdd(&sc[g], 1);
        }
    __syncthreads();
    if (threadIdx.x < G && sc[threadIdx.x]) {
        atomicAdd(sum + threadIdx.x, ss[threadIdx.x]);
        atomicAdd(cnt + threadIdx.x, sc[threadIdx.x]);
    }
}
__global__ void masked_mean_groups_final_kernel(const float* sum, const int* cnt, int G, float scale, float* out,
                                                float* sum_all) {
    float tot = 0.f, all = 0.f;
    for (int g = 0; g < G; ++g) {
        tot += cnt[g] > 0 ? sum[g] / (float)cnt[g] : __builtin_nanf("");          // an all-pad micro-batch: NaN, as above
        all += sum[g];
    }
    out[0] = scale * tot;
    if (sum_all != nullptr) sum_all[0] = all;
}
__global__ void loss_grad_groups_kernel(const int64_t* __restrict__ target, int n, int pad, const int* __restrict__ cnt,
                                        float scale, int B, int Bc, float* __restrict__ g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = (target[i] != pad) ? scale / (float)max(cnt[(i % B) / Bc], 1) : 0.f;
}

__global__ void copy_rows_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x)
        ((bf16x8*)dst)[i] = ((const bf16x8*)src)[i];
}

}  // namespace

static inline unsigned cap_blocks(size_t want) {
    return (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
}

static inline unsigned drop_threshold(float p) { return drop_threshold16(p); }          // (common.h: 16-bit, one word per two elements)

extern "C" int commu_embed_fwd(const int64_t* tok, const float* E, void* out, int ldo, int ntok, int D, int V,
                               float scale, unsigned drop_seed, float drop_p, hipStream_t stream) {
    if (ntok <= 0) return 0;
    if (D % 4) return -22;
    COMMU_LAUNCH(embed_fwd_kernel, dim3((ntok + 3) / 4), dim3(256), 0, stream, tok, E, (bf16*)out,
                       ldo, ntok, D, V, scale, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_embed_bwd(const int64_t* tok, const void* dX, int ldx, float* dE, int ntok, int D,
                               int V, float scale, int accumulate, unsigned drop_seed, float drop_p,
                               hipStream_t stream) {
    if (D > 1024) return -22;
    COMMU_LAUNCH(embed_bwd_kernel, dim3(V), dim3(256), 0, stream, tok, (const bf16*)dX, ldx, dE,
                       ntok, D, scale, accumulate, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
    COMMU_LAUNCH_CHECK();
    return 0;
}

// Token order for commu_embed_bwd_sorted without a library sort: a stable counting sort over the V <= 1024 ids.
//   1. histogram of the ids of each of 64 consecutive chunks of the token list (LDS, integer atomics) -> hist[g][V]
//   2. offs[v] = exclusive prefix of the id totals; hist[g][v] becomes the first sorted position of id v in chunk g
//   3. one wave per chunk walks its tokens 64 at a time IN ORDER: the lanes holding the same id find each other with ten
//      ballots (one per id bit), a lane's position is base[g][id] + tokens of that id seen in earlier steps (an LDS
//      counter) + equal-id lanes below it -- a stable argsort whatever the schedule.  (One wave per ID scanning the whole
//      list, the first form, took 307 us: 512 dependent steps per wave; this form 29 us.)
// ids outside [0, V) are left out (offs[V] = number of valid tokens; the tail of perm is zero-filled: readable row 0).
constexpr int TOK_CHUNKS = 64;
__global__ __launch_bounds__(256) void tok_hist_kernel(const int64_t* __restrict__ tok, int ntok, int V, int* __restrict__ hist) {
    __shared__ int h[1024];
    for (int v = threadIdx.x; v < V; v += 256) h[v] = 0;
    __syncthreads();
    const int per = (ntok + TOK_CHUNKS - 1) / TOK_CHUNKS;
    const int lo = blockIdx.x * per, hi = min(ntok, lo + per);
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const int64_t t = tok[i];
        if (t >= 0 && t < V) atomicAdd(&h[(int)t], 1);
    }
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256) hist[blockIdx.x * V + v] = h[v];
}
__global__ __launch_bounds__(1024) void tok_scan_kernel(int* __restrict__ hist, int V, int ntok, int64_t* __restrict__ offs,
                                                        int64_t* __restrict__ perm) {
    __shared__ int tot[1024];
    const int v = threadIdx.x;
    int s = 0;
    if (v < V)
        for (int g = 0; g < TOK_CHUNKS; ++g) s += hist[g * V + v];
    tot[v] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {          // inclusive scan
        const int add = v >= d ? tot[v - d] : 0;
        __syncthreads();
        tot[v] += add;
        __syncthreads();
    }
    if (v < V) {
        offs[v + 1] = tot[v];
        int run = tot[v] - s;                      // first sorted position of id v
        for (int g = 0; g < TOK_CHUNKS; ++g) {
            const int c = hist[g * V + v];
            hist[g * V + v] = run;
            run += c;
        }
    }
    if (v == 0) offs[0] = 0;
    for (int k = tot[V - 1] + v; k < ntok; k += 1024) perm[k] = 0;          // tokens left out
}
__global__ __launch_bounds__(64) void tok_scatter_kernel(const int64_t* __restrict__ tok, int ntok, int V,
                                                         const int* __restrict__ base, int64_t* __restrict__ perm) {
    __shared__ int seen[1024];
    const int lane = threadIdx.x, g = blockIdx.x;
    for (int v = lane; v < V; v += 64) seen[v] = 0;
    __syncthreads();
    const int per = (ntok + TOK_CHUNKS - 1) / TOK_CHUNKS;
    const int lo = g * per, hi = min(ntok, lo + per);
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int p0 = lo; p0 < hi; p0 += 64) {
        const int i = p0 + lane;
        const int64_t t = i < hi ? tok[i] : -1;
        const bool valid = t >= 0 && t < V;
        const int id = valid ? (int)t : 0;
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 10; ++b) {
            const bool bit = (id >> b) & 1;
            const unsigned long long bb = __ballot(valid && bit);
            m &= bit ? bb : ~bb;
        }
        if (valid) {
            const int before = seen[id];                          // (every lane of the group reads before its top lane writes)
            perm[base[g * V + id] + before + __popcll(m & lt)] = i;
            if ((m >> lane) == 1ull) seen[id] = before + __popcll(m);      // the group's top lane
        }
        __syncthreads();
    }
}

extern "C" int commu_token_order(const int64_t* tok, int ntok, int V, int64_t* perm, int64_t* offs, int* ws,
                                 hipStream_t stream) {
    if (ntok <= 0 || V <= 0 || V > 1024) return -22;
    COMMU_LAUNCH(tok_hist_kernel, dim3(TOK_CHUNKS), dim3(256), 0, stream, tok, ntok, V, ws);
    COMMU_LAUNCH(tok_scan_kernel, dim3(1), dim3(1024), 0, stream, ws, V, ntok, offs, perm);
    COMMU_LAUNCH(tok_scatter_kernel, dim3(TOK_CHUNKS), dim3(64), 0, stream, tok, ntok, V, ws, perm);
    COMMU_LAUNCH_CHECK();
    return 0;
}

/* rows (of D floats) of the workspace commu_embed_bwd_sorted needs for ntok tokens and V ids */
extern "C" int commu_embed_bwd_ws_rows(int ntok, int V) { return V + (ntok + EMB_CHUNK - 1) / EMB_CHUNK + 1; }

extern "C" int commu_embed_bwd_sorted(const int64_t* perm, const int64_t* offs, const void* dX, int ldx, float* ws,
                                      int ntok, int D, int V, float* dE, float scale, int accumulate, unsigned drop_seed,
                                      float drop_p, hipStream_t stream) {
    if (V <= 0 || ntok < 0) return 0;
    if (D > 1024 || (D % 4) || ldx < ((D + 7) & ~7) || (ldx % 8)) return -22;
    const int nchunks = (ntok + EMB_CHUNK - 1) / EMB_CHUNK;
    if (nchunks > 0) {
        const dim3 grid((nchunks + 3) / 4);
        if (D <= 512)
            COMMU_LAUNCH(embed_bwd_runs_kernel<1>, grid, dim3(256), 0, stream, perm, offs, (const bf16*)dX, ldx, ws, ntok, D,
                         V, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
        else
            COMMU_LAUNCH(embed_bwd_runs_kernel<2>, grid, dim3(256), 0, stream, perm, offs, (const bf16*)dX, ldx, ws, ntok, D,
                         V, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
    }
    COMMU_LAUNCH(embed_bwd_fold_kernel, dim3(V), dim3(256), 0, stream, offs, ws, dE, D, V, scale, accumulate);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_posemb_fwd(const float* inv_freq, void* out, int ld, int K, int D, int clamp_len, unsigned drop_seed,
                                float drop_p, hipStream_t stream) {
    const int n = K * (D / 2);
    if (n <= 0) return 0;
    COMMU_LAUNCH(posemb_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, inv_freq, (bf16*)out,
                       ld, K, D, clamp_len, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_layernorm_fwd(const void* z, int ldz, const float* gamma, const float* beta, void* y,
                                   int ldy, float* mean, float* rstd, int rows, int D, float eps,
                                   void* y_drop, int ldyd, unsigned drop_seed, float drop_p,
                                   hipStream_t stream) {
    if (rows <= 0) return 0;
    const int D8 = (D + 7) & ~7;
    if (D > 1024 || (D % 4) || (ldz % 8) || (ldy % 8) || ldz < D8 || ldy < D8 || (y_drop != nullptr && ((ldyd % 8) || ldyd < D8)))
        return -22;
    COMMU_LAUNCH(layernorm_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, (const bf16*)z,
                       ldz, gamma, beta, (bf16*)y, ldy, mean, rstd, rows, D, eps, (bf16*)y_drop, ldyd, drop_seed,
                       drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_layernorm_bwd_nblocks(int rows) { return (rows + LNB_ROWS - 1) / LNB_ROWS; }

static int layernorm_bwd_launch(const void* dy, int lddy, const void* dy2, int lddy2, const void* z, int ldz, const float* mean,
                                const float* rstd, const float* gamma, void* dz, int lddz, float* part, int rows, int D,
                                void* dz_masked, int lddzm, unsigned drop_seed, float drop_p, hipStream_t stream) {
    if (rows <= 0) return 0;
    const int D8 = (D + 7) & ~7;
    if (D > 1024 || (D % 4) || (lddy % 8) || (ldz % 8) || (lddz % 8) || lddy < D8 || ldz < D8 || lddz < D8 ||
        (dz_masked != nullptr && lddzm != lddz) || (dy2 != nullptr && ((lddy2 % 8) || lddy2 < D8)))
        return -22;
#define LNB(NCV, ADDV)                                                                                                          \
    COMMU_LAUNCH((layernorm_bwd_kernel<NCV, ADDV>), dim3(commu_layernorm_bwd_nblocks(rows)), dim3(256), 0, stream,               \
                 (const bf16*)dy, lddy, (const bf16*)dy2, lddy2, (const bf16*)z, ldz, mean, rstd, gamma, (bf16*)dz, lddz, part,  \
                 rows, D, (bf16*)dz_masked, lddzm, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)))
    if (D <= 512) {
        if (dy2 != nullptr) LNB(1, true);
        else LNB(1, false);
    } else {
        if (dy2 != nullptr) LNB(2, true);
        else LNB(2, false);
    }
#undef LNB
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_layernorm_bwd(const void* dy, int lddy, const void* z, int ldz, const float* mean,
                                   const float* rstd, const float* gamma, void* dz, int lddz,
                                   float* part, int rows, int D, void* dz_masked, int lddzm,
                                   unsigned drop_seed, float drop_p, hipStream_t stream) {
    return layernorm_bwd_launch(dy, lddy, nullptr, 0, z, ldz, mean, rstd, gamma, dz, lddz, part, rows, D, dz_masked, lddzm,
                                drop_seed, drop_p, stream);
}

extern "C" int commu_layernorm_bwd_add(const void* dy, int lddy, const void* dy2, int lddy2, const void* z, int ldz,
                                       const float* mean, const float* rstd, const float* gamma, void* dz, int lddz,
                                       float* part, int rows, int D, void* dz_masked, int lddzm, unsigned drop_seed,
                                       float drop_p, hipStream_t stream) {
    if (dy2 == nullptr) return -22;
    return layernorm_bwd_launch(dy, lddy, dy2, lddy2, z, ldz, mean, rstd, gamma, dz, lddz, part, rows, D, dz_masked, lddzm,
                                drop_seed, drop_p, stream);
}

/* rows of the fp32 workspace (`cols` rounded up to 8 floats each) the column sum of a rows x cols input needs;
 * 0: none (a small fp32 input is summed by the final pass alone) */
extern "C" int commu_colsum_slabs(int rows, int cols, int elem_bytes) {
    if (rows <= 0 || cols <= 0) return 0;
    const bool small = (size_t)rows * cols * elem_bytes <= ((size_t)4 << 20);
    if (small && elem_bytes == 4) return 0;
    const int strip = elem_bytes == 2 ? 512 : 256;
    const int nx = (cols + strip - 1) / strip;
    const int ny = (rows + 63) / 64;
    const int cap = small ? 256 : (512 + nx - 1) / nx;           // ~512 workgroups on a large input: two per CU, and the
                                                                 // final pass walks at most 512 partial rows
    return ny > cap ? cap : ny;
}

template <typename T>
static int colsum_launch(const T* X, int ldx, int rows, int cols, float* out, float* ws, int ws_rows, float alpha,
                         hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return 0;
    constexpr int V = sizeof(T) == 2 ? 8 : 4;
    const int ny = commu_colsum_slabs(rows, cols, (int)sizeof(T));
    if (ny == 0) {          // small fp32 input
        COMMU_LAUNCH(colsum_final_kernel, dim3((cols + 15) / 16, 1), dim3(256), 0, stream, (const float*)X, ldx, (size_t)0,
                     rows, cols, out, (float*)nullptr, (float*)nullptr, alpha);
        COMMU_LAUNCH_CHECK();
        return 0;
    }
    const int colsv = (cols + V - 1) / V * V;          // whole 16-byte chunks (pad columns are summed and ignored)
    if (ws == nullptr || ws_rows < ny || colsv > ldx || (ldx % V) || (((size_t)X) & 15)) return -22;
    COMMU_LAUNCH((colsum_slab_kernel<T>), dim3((colsv + 64 * V - 1) / (64 * V), ny), dim3(256), 0, stream, X, ldx, rows,
                 colsv, ws, (rows + ny - 1) / ny);
    COMMU_LAUNCH(colsum_final_kernel, dim3((cols + 15) / 16, 1), dim3(256), 0, stream, ws, colsv, (size_t)0, ny, cols, out,
                 (float*)nullptr, (float*)nullptr, alpha);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// Every final pass of a backward step in ONE launch: a task is an output vector (a bias / LayerNorm-parameter / shared
// attention-bias gradient) and the fp32 sources whose column sums it receives -- partial rows of a slab pass or of the
// LayerNorm backward, per-tile sums of the attention kernels --, each with its factor.  Sources of one output are walked by
// the same workgroup one after the other (fixed order, no two workgroups add into one address).  The 37 final passes of a
// step were 37 launches of 8-96 workgroups on a side stream, each waiting ~30 us for free CUs.
struct ColsumGroupArgs {
    commu_colsum_source src[COMMU_COLSUM_MAX_SOURCES];
    commu_colsum_task task[COMMU_COLSUM_MAX_TASKS];
    int wg_begin[COMMU_COLSUM_MAX_TASKS + 1];
    int ntask;
};
__global__ __launch_bounds__(256) void colsum_group_kernel(const ColsumGroupArgs a) {
    __shared__ f32x4 red[64][4];
    int t = 0;
    while (t + 1 < a.ntask && (int)blockIdx.x >= a.wg_begin[t + 1]) ++t;
    const commu_colsum_task tk = a.task[t];
    const int rl = threadIdx.x >> 2, cl = threadIdx.x & 3;
    const int c0 = ((int)blockIdx.x - a.wg_begin[t]) * 16 + cl * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int si = tk.src_begin; si < tk.src_end; ++si) {
        const commu_colsum_source sc = a.src[si];
        const float* P = sc.X;
        const int ldx = sc.ldx, rows = sc.rows;
        f32x4 p = {0.f, 0.f, 0.f, 0.f};
        if (c0 < tk.cols) {
            const bool vec = c0 + 3 < tk.cols && ((ldx & 3) == 0) && ((((size_t)P) & 15) == 0);
            int r = rl;
            if (vec) {
                for (; r + 192 < rows; r += 256) {          // four loads in flight
                    f32x4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(P + (size_t)(r + 64 * u) * ldx + c0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) p += v[u];
                }
                for (; r < rows; r += 64) p += *(const f32x4*)(P + (size_t)r * ldx + c0);
            } else {
                for (; r < rows; r += 64)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c0 + e < tk.cols) p[e] += P[(size_t)r * ldx + c0 + e];
            }
        }
        acc += p * sc.alpha;
    }
    red[rl][cl] = acc;
    __syncthreads();
#pragma unroll
    for (int st = 32; st >= 4; st >>= 1) {
        if (rl < st) red[rl][cl] += red[rl + st][cl];
        __syncthreads();
    }
    if (threadIdx.x < 16) {
        const int c = ((int)blockIdx.x - a.wg_begin[t]) * 16 + threadIdx.x;
        if (c < tk.cols) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += red[k][threadIdx.x >> 2][threadIdx.x & 3];
            tk.out[c] += s;
        }
    }
}

extern "C" int commu_colsum_group_f32(const commu_colsum_task* tasks, int ntask, const commu_colsum_source* srcs, int nsrc,
                                      hipStream_t stream) {
    if (ntask <= 0) return 0;
    if (ntask > COMMU_COLSUM_MAX_TASKS || nsrc > COMMU_COLSUM_MAX_SOURCES || nsrc <= 0) return -22;
    ColsumGroupArgs a = {};
    int wg = 0;
    for (int t = 0; t < ntask; ++t) {
        if (tasks[t].src_begin < 0 || tasks[t].src_end > nsrc || tasks[t].src_begin > tasks[t].src_end ||
            tasks[t].cols <= 0 || tasks[t].out == nullptr) return -22;
        a.task[t] = tasks[t];
        a.wg_begin[t] = wg;
        wg += (tasks[t].cols + 15) / 16;
    }
    a.wg_begin[ntask] = wg;
    a.ntask = ntask;
    for (int i = 0; i < nsrc; ++i) a.src[i] = srcs[i];
    COMMU_LAUNCH(colsum_group_kernel, dim3(wg), dim3(256), 0, stream, a);
    COMMU_LAUNCH_CHECK();
    return 0;
}

/* the slab pass of commu_colsum_bf16 / _f32 alone: partial rows into ws (commu_colsum_slabs rows of `cols` rounded up to
 * 8 / 4 floats); returns the number of partial rows written, 0 when the input needs no slab pass (sum it directly) */
template <typename T>
static int colsum_slabs_only(const T* X, int ldx, int rows, int cols, float* ws, int ws_rows, hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return 0;
    constexpr int V = sizeof(T) == 2 ? 8 : 4;
    const int ny = commu_colsum_slabs(rows, cols, (int)sizeof(T));
    if (ny == 0) return 0;
    const int colsv = (cols + V - 1) / V * V;
    if (ws == nullptr || ws_rows < ny || colsv > ldx || (ldx % V) || (((size_t)X) & 15)) return -22;
    COMMU_LAUNCH((colsum_slab_kernel<T>), dim3((colsv + 64 * V - 1) / (64 * V), ny), dim3(256), 0, stream, X, ldx, rows,
                 colsv, ws, (rows + ny - 1) / ny);
    hipError_t e__ = hipGetLastError();
    if (e__ != hipSuccess) return -(int)e__;
    return ny;
}
extern "C" int commu_colsum_slab_pass(const void* X, int elem_bytes, int ldx, int rows, int cols, float* ws, int ws_rows,
                                      hipStream_t stream) {
    if (elem_bytes == 2) return colsum_slabs_only<bf16>((const bf16*)X, ldx, rows, cols, ws, ws_rows, stream);
    if (elem_bytes == 4) return colsum_slabs_only<float>((const float*)X, ldx, rows, cols, ws, ws_rows, stream);
    return -22;
}

extern "C" int commu_colsum_bf16(const void* X, int ldx, int rows, int cols, float* out, float* ws, int ws_rows,
                                 float alpha, hipStream_t stream) {
    return colsum_launch<bf16>((const bf16*)X, ldx, rows, cols, out, ws, ws_rows, alpha, stream);
}

extern "C" int commu_layernorm_bwd_reduce(const float* part, int nblk, int D, float* dgamma, float* dbeta,
                                          float* dbias, hipStream_t stream) {
    if (nblk <= 0 || D <= 0) return 0;
    // part is [nblk][3][D]: plane z of row r at part + (3 r + z) D  ->  row pitch 3 D, plane offset D
    COMMU_LAUNCH(colsum_final_kernel, dim3((D + 15) / 16, 3), dim3(256), 0, stream, part, 3 * D, (size_t)D, nblk, D,
                 dgamma, dbeta, dbias, 1.f);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_colsum_f32(const float* X, int ldx, int rows, int cols, float* out, float* ws, int ws_rows,
                                float alpha, hipStream_t stream) {
    return colsum_launch<float>(X, ldx, rows, cols, out, ws, ws_rows, alpha, stream);
}

extern "C" int commu_ce_fwd(const float* logits, int ldl, const int64_t* target, float* nll, float* lse,
                            int rows, int V, hipStream_t stream) {
    if (rows <= 0) return 0;
    if (V <= 768 && ldl <= 768 && (ldl % 4) == 0 && (((size_t)logits) & 15) == 0)
        COMMU_LAUNCH(ce_fwd_vec_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, nll, lse, rows, V);
    else
        COMMU_LAUNCH(ce_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, nll,
                       lse, rows, V);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_ce_bwd(const float* logits, int ldl, const int64_t* target, const float* lse,
                            const float* g, void* dlogits, int ldd, int rows, int V, hipStream_t stream) {
    if (rows <= 0) return 0;
    if (V <= 768 && ldl <= 768 && ldd <= 768 && (ldl % 4) == 0 && (ldd % 4) == 0 && ldd <= ldl + 3 && (((size_t)logits) & 15) == 0 &&
        (((size_t)dlogits) & 7) == 0)
        COMMU_LAUNCH(ce_bwd_vec_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, lse, g,
                     (bf16*)dlogits, ldd, rows, V);
    else
        COMMU_LAUNCH(ce_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, lse,
                       g, (bf16*)dlogits, ldd, rows, V);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// (the same layout conditions as commu_ce_fwd / commu_ce_bwd pick the register kernels)
extern "C" int commu_ce_fwd_opts(const float* logits, int ldl, const int64_t* target, float* loss, float* nll, float* lse,
                                 int rows, int V, float label_smoothing, float z_loss, hipStream_t stream) {
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f) || !(z_loss >= 0.f && z_loss < INFINITY) || V <= 0) return -22;
    if (rows <= 0) return 0;
    if (V <= 768 && ldl <= 768 && (ldl % 4) == 0 && (((size_t)logits) & 15) == 0)
        COMMU_LAUNCH(ce_fwd_opts_vec_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, loss, nll, lse,
                     rows, V, label_smoothing, z_loss);
    else
        COMMU_LAUNCH(ce_fwd_opts_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, loss, nll, lse, rows,
                     V, label_smoothing, z_loss);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_ce_bwd_opts(const float* logits, int ldl, const int64_t* target, const float* lse, const float* g,
                                 void* dlogits, int ldd, int rows, int V, float label_smoothing, float z_loss,
                                 hipStream_t stream) {
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f) || !(z_loss >= 0.f && z_loss < INFINITY) || V <= 0) return -22;
    if (rows <= 0) return 0;
    if (V <= 768 && ldl <= 768 && ldd <= 768 && (ldl % 4) == 0 && (ldd % 4) == 0 && ldd <= ldl + 3 && (((size_t)logits) & 15) == 0 &&
        (((size_t)dlogits) & 7) == 0)
        COMMU_LAUNCH(ce_bwd_opts_vec_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, lse, g,
                     (bf16*)dlogits, ldd, rows, V, label_smoothing, z_loss);
    else
        COMMU_LAUNCH(ce_bwd_opts_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, logits, ldl, target, lse, g,
                     (bf16*)dlogits, ldd, rows, V, label_smoothing, z_loss);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_nll_by_class_blocks(int rows) {
    const int n = (rows + 1023) / 1024;          // at least four rows per thread before a second workgroup starts
    return n < 1 ? 1 : (n > 256 ? 256 : n);
}

extern "C" int commu_nll_by_class(const float* nll, const int64_t* target, const int* class_of_token, int V, int C, int pad,
                                  int rows, float* part_sum, int* part_cnt, int nblk, float* sum, int* count,
                                  hipStream_t stream) {
    if (C < 1 || C > NLL_CLASSES_MAX || V <= 0 || rows < 0 || nblk < 1 || nblk > 1024) return -22;
    COMMU_LAUNCH(nll_by_class_partial_kernel, dim3(nblk), dim3(256), 0, stream, nll, target, class_of_token, V, C, pad, rows,
                 part_sum, part_cnt);
    COMMU_LAUNCH(nll_by_class_final_kernel, dim3(1), dim3(64), 0, stream, part_sum, part_cnt, nblk, C, sum, count);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_grad_norm(const float* g, size_t n, float* part, int npart, float* out,
                               hipStream_t stream) {
    if (npart <= 0 || npart > 1024) return -22;
    COMMU_LAUNCH(sumsq_partial_kernel, dim3(npart), dim3(256), 0, stream, g, n, part);
    COMMU_LAUNCH(sumsq_final_kernel, dim3(1), dim3(64), 0, stream, part, npart, out);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// (the vector body moves 16 bytes per lane: fp32 vectors 16-byte aligned, the bf16 shadow 8-byte aligned; any other slice
//  of the flat buffers -- e.g. one parameter at an odd offset -- takes the element-wise body of the same kernel)
static bool adam_misaligned(const void* p, const void* g, const void* m, const void* v, const void* pb) {
    return ((((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) != 0) || (((size_t)pb & 7) != 0);
}

extern "C" int commu_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n,
                               float lr, float beta1, float beta2, float eps, int step,
                               const float* gnorm, float clip, hipStream_t stream) {
    if (n == 0) return 0;
    const bool vec = !adam_misaligned(p, g, m, v, p_bf16);
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    COMMU_LAUNCH(adam_kernel, dim3(cap_blocks((n / 4 + 255) / 256)), dim3(256), 0, stream, p, g, m, v,
                       (bf16*)p_bf16, n, lr, beta1, beta2, eps, bc1, bc2, gnorm, clip, vec);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_adam_step_dev(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n,
                                   const float* scal, float beta1, float beta2, float eps, const float* gnorm,
                                   float clip, hipStream_t stream) {
    if (n == 0) return 0;
    if (scal == nullptr) return -22;
    COMMU_LAUNCH(adam_dev_kernel, dim3(cap_blocks((n / 4 + 255) / 256)), dim3(256), 0, stream, p, g, m, v,
                 (bf16*)p_bf16, n, scal, beta1, beta2, eps, gnorm, clip, !adam_misaligned(p, g, m, v, p_bf16));
    COMMU_LAUNCH_CHECK();
    return 0;
}

/* bias corrections exactly as commu_adam_step computes them (so that a host can fill the device scalars of
 * commu_adam_step_dev with bit-identical values) */
extern "C" int commu_adam_bias_corrections(float beta1, float beta2, int step, float* out2) {
    out2[0] = 1.f - powf(beta1, (float)step);
    out2[1] = 1.f - powf(beta2, (float)step);
    return 0;
}

COMMU_DEFINE_SEED_SALT_SETTER(commu_seed_salt_elementwise)

extern "C" int commu_scale_clip_f32(float* g, size_t n, const float* gnorm, float clip, hipStream_t stream) {
    if (n == 0) return 0;
    COMMU_LAUNCH(scale_clip_kernel, dim3(cap_blocks((n + 255) / 256)), dim3(256), 0, stream, g, n, gnorm,
                       clip);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_cast_f32_bf16(const float* in, void* out, size_t n, hipStream_t stream) {
    if (n == 0) return 0;
    COMMU_LAUNCH(cast_f32_bf16_kernel, dim3(cap_blocks((n + 255) / 256)), dim3(256), 0, stream, in,
                       (bf16*)out, n);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// GELU as a NON-DEFAULT FFN activation (the reference's PositionwiseFF is Linear-ReLU-Dropout-Linear-Dropout,
// model.py:163-169; BASELINE.json's north star names a GELU-FFN): exact erf form of torch.nn.functional.gelu, as an
// element-wise pair around the plain Linear GEMMs -- out = dropout(gelu(z)), dz = dy * keep/(1-p) * gelu'(z) -- with the
// same counter-based mask as a GEMM epilogue at that site (index m * cols + n).  Not on the headline path.
__global__ __launch_bounds__(256) void gelu_kernel(const bf16* __restrict__ z, int ldz, const bf16* __restrict__ dy, int lddy,
                                                   bf16* __restrict__ out, int ldo, int rows, int cols, unsigned drop_seed,
                                                   unsigned drop_thr, float drop_scale) {
    const DropKey key = drop_key(salted(drop_seed));
    const int cg = (cols + 7) / 8;
    const size_t total = (size_t)rows * cg;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const int m = (int)(t / cg), n0 = (int)(t % cg) * 8;
        const bf16x8 zv = ld_bf16x8(z + (size_t)m * ldz + n0);
        bf16x8 gv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (dy != nullptr) gv = ld_bf16x8(dy + (size_t)m * lddy + n0);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = bf2f(zv[e]);
            const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
            float v = dy == nullptr ? x * cdf : bf2f(gv[e]) * (cdf + x * 0.3989422804014327f * __expf(-0.5f * x * x));
            if (drop_thr) v = drop_keep(key, (unsigned)m * (unsigned)cols + (unsigned)(n0 + e), drop_thr) ? v * drop_scale : 0.f;
            o[e] = f2bf(n0 + e < cols ? v : 0.f);
        }
        st_bf16x8(out + (size_t)m * ldo + n0, o);
    }
}
static int gelu_launch(const void* z, int ldz, const void* dy, int lddy, void* out, int ldo, int rows, int cols,
                       unsigned drop_seed, float drop_p, hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return 0;
    const int c8 = (cols + 7) & ~7;
    if ((ldz % 8) || (ldo % 8) || ldz < c8 || ldo < c8 || (dy != nullptr && ((lddy % 8) || lddy < c8))) return -22;
    const size_t total = (size_t)rows * (c8 / 8);
    COMMU_LAUNCH(gelu_kernel, dim3(cap_blocks((total + 255) / 256)), dim3(256), 0, stream, (const bf16*)z, ldz,
                 (const bf16*)dy, lddy, (bf16*)out, ldo, rows, cols, drop_seed, drop_threshold(drop_p), drop_keep_scale16(drop_threshold(drop_p)));
    COMMU_LAUNCH_CHECK();
    return 0;
}
extern "C" int commu_gelu_fwd(const void* z, int ldz, void* out, int ldo, int rows, int cols, unsigned drop_seed, float drop_p,
                              hipStream_t stream) {
    return gelu_launch(z, ldz, nullptr, 0, out, ldo, rows, cols, drop_seed, drop_p, stream);
}
extern "C" int commu_gelu_bwd(const void* dy, int lddy, const void* z, int ldz, void* dz, int lddz, int rows, int cols,
                              unsigned drop_seed, float drop_p, hipStream_t stream) {
    if (dy == nullptr) return -22;
    return gelu_launch(z, ldz, dy, lddy, dz, lddz, rows, cols, drop_seed, drop_p, stream);
}

extern "C" int commu_cast_bf16_f32(const void* in, float* out, size_t n, hipStream_t stream) {
    if (n == 0) return 0;
    COMMU_LAUNCH(cast_bf16_f32_kernel, dim3(cap_blocks((n + 255) / 256)), dim3(256), 0, stream,
                       (const bf16*)in, out, n);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_transpose_bf16(const void* in, int ldi, void* out, int ldo, int rows, int cols,
                                    hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return 0;
    COMMU_LAUNCH(transpose_bf16_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, stream,
                       (const bf16*)in, ldi, (bf16*)out, ldo, rows, cols);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// every transposed weight shadow of an optimiser step in one launch: workgroup -> (item, 64 x 64 tile) by a scan of the
// per-item tile counts (<= 32 items: a few scalar compares)
struct TransposeGroup {
    commu_transpose_item it[32];
    int tile_end[32];          // exclusive prefix of tiles
    int n;
};
__global__ __launch_bounds__(256) void transpose_group_kernel(const TransposeGroup g) {
    __shared__ bf16 t[64][66];
    int k = 0;
    while (k + 1 < g.n && (int)blockIdx.x >= g.tile_end[k]) ++k;
    const commu_transpose_item& it = g.it[k];
    const int local = (int)blockIdx.x - (k ? g.tile_end[k - 1] : 0);
    const int tx = (it.cols + 63) / 64;
    const int r0 = (local / tx) * 64, c0 = (local % tx) * 64;
    const bf16* in = (const bf16*)it.in;
    bf16* out = (bf16*)it.out;
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const int r = i >> 6, c = i & 63;
        t[r][c] = (r0 + r < it.rows && c0 + c < it.cols) ? in[(size_t)(r0 + r) * it.ldi + c0 + c] : f2bf(0.f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4096; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (c0 + c < it.cols && r0 + r < it.rows) out[(size_t)(c0 + c) * it.ldo + r0 + r] = t[r][c];
    }
}

extern "C" int commu_transpose_group_bf16(const commu_transpose_item* items, int n, hipStream_t stream) {
    if (n <= 0) return 0;
    if (n > 32) return -22;
    TransposeGroup g;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        g.it[i] = items[i];
        if (items[i].rows <= 0 || items[i].cols <= 0) return -22;
        total += ((items[i].rows + 63) / 64) * ((items[i].cols + 63) / 64);
        g.tile_end[i] = total;
    }
    g.n = n;
    COMMU_LAUNCH(transpose_group_kernel, dim3(total), dim3(256), 0, stream, g);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_transpose_f32_bf16(const float* in, int ldi, void* out, int ldo, int rows, int cols,
                                        hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return 0;
    COMMU_LAUNCH(transpose_f32_bf16_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0,
                       stream, in, ldi, (bf16*)out, ldo, rows, cols);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_masked_mean(const float* nll, const int64_t* target, int n, int pad, float scale,
                                 float* sum_ws, int* cnt_ws, float* out, hipStream_t stream) {
    // out[0] = scale * mean(nll[target != pad]); cnt_ws keeps the count for commu_loss_grad
    hipMemsetAsync(sum_ws, 0, sizeof(float), stream);
    hipMemsetAsync(cnt_ws, 0, sizeof(int), stream);
    if (n > 0)
        COMMU_LAUNCH(masked_sum_kernel, dim3(cap_blocks((n + 1023) / 1024)), dim3(256), 0, stream, nll,
                           target, n, pad, sum_ws, cnt_ws);
    COMMU_LAUNCH(masked_mean_final_kernel, dim3(1), dim3(1), 0, stream, sum_ws, cnt_ws, scale, out);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_loss_grad(const int64_t* target, int n, int pad, const int* cnt_ws, float scale,
                               float* g, hipStream_t stream) {
    // g[m] = scale * (target[m] != pad) / cnt_ws[0]   (cnt_ws filled by commu_masked_mean)
    if (n <= 0) return 0;
    COMMU_LAUNCH(loss_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, target, n, pad, cnt_ws,
                       scale, g);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_masked_mean_groups(const float* nll, const int64_t* target, int n, int pad, float scale, int B, int Bc,
                                        float* sum_ws, int* cnt_ws, float* out, float* sum_all, hipStream_t stream) {
    // out[0] = scale * sum over the B / Bc column groups of mean(nll[target != pad] within the group); sum_ws / cnt_ws:
    // B / Bc floats / ints (kept for commu_loss_grad_groups); sum_all (optional): the sum over every non-pad target
    if (B <= 0 || Bc <= 0 || (B % Bc) || B / Bc > MAX_GROUPS || n < 0 || (n % B)) return -22;
    const int G = B / Bc;
    hipMemsetAsync(sum_ws, 0, sizeof(float) * G, stream);
    hipMemsetAsync(cnt_ws, 0, sizeof(int) * G, stream);
    if (n > 0)
        COMMU_LAUNCH(masked_sum_groups_kernel, dim3(cap_blocks((n + 1023) / 1024)), dim3(256), 0, stream, nll, target, n,
                     pad, B, Bc, G, sum_ws, cnt_ws);
    COMMU_LAUNCH(masked_mean_groups_final_kernel, dim3(1), dim3(1), 0, stream, sum_ws, cnt_ws, G, scale, out, sum_all);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_loss_grad_groups(const int64_t* target, int n, int pad, const int* cnt_ws, float scale, int B, int Bc,
                                      float* g, hipStream_t stream) {
    if (B <= 0 || Bc <= 0 || (B % Bc) || B / Bc > MAX_GROUPS) return -22;
    if (n <= 0) return 0;
    COMMU_LAUNCH(loss_grad_groups_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, target, n, pad, cnt_ws, scale, B, Bc,
                 g);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_copy_bf16(const void* src, void* dst, size_t n, hipStream_t stream) {
    if (n == 0) return 0;
    if (n % 8) return -22;
    COMMU_LAUNCH(copy_rows_kernel, dim3(cap_blocks((n / 8 + 255) / 256)), dim3(256), 0, stream,
                       (const bf16*)src, (bf16*)dst, n / 8);
    COMMU_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// K9: memory update (reference model.py:507-538  _update_mems: new_mems[l] = cat([mems[l], hids[l]])[beg:end]).
// One launch for all L+1 layers: out[l] = [ mems[l][mem_skip : mem_skip + keep) ; hids[l][hid_skip : hid_skip + take) ]
// (element counts, multiples of 8 -- rows are whole [B, Dp] time steps).  16-byte copies, HBM-bound:
// (keep + take) * 2 bytes read + the same written per layer.  When tgt_len >= mem_len nothing is copied at all: the
// forward writes every layer's output into one [L+1, T, B, Dp] buffer and the new memory is a view of it.
__global__ void __launch_bounds__(256) mems_update_kernel(const bf16* __restrict__ hids, size_t hid_stride, size_t hid_skip,
                                                          size_t take, const bf16* __restrict__ mems, size_t mem_stride,
                                                          size_t mem_skip, size_t keep, bf16* __restrict__ out,
                                                          size_t out_stride) {
    const int l = blockIdx.y;
    const uint4* m = reinterpret_cast<const uint4*>(mems + (size_t)l * mem_stride + mem_skip);
    const uint4* h = reinterpret_cast<const uint4*>(hids + (size_t)l * hid_stride + hid_skip);
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)l * out_stride);
    const size_t nk = keep / 8, n = nk + take / 8;
    // four independent 16-byte loads in flight per thread (one at a time streamed at 1.5 TB/s: 628 us for the 0.94 GB of the
    // released default configuration)
    const size_t step = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * step < n; i += 4 * step) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t j = i + u * step;
            v[u] = j < nk ? m[j] : h[j - nk];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) o[i + u * step] = v[u];
    }
    for (; i < n; i += step) o[i] = i < nk ? m[i] : h[i - nk];
}

extern "C" int commu_mems_update(const void* hids, size_t hid_stride, size_t hid_skip, size_t take, const void* mems,
                                 size_t mem_stride, size_t mem_skip, size_t keep, void* out, size_t out_stride,
                                 int layers, hipStream_t stream) {
    if (layers <= 0 || keep + take == 0) return 0;
    if ((hid_stride | hid_skip | take | mem_stride | mem_skip | keep | out_stride) % 8) return -22;
    if ((keep && !mems) || (take && !hids) || !out) return -22;
    const size_t n = (keep + take) / 8;
    int bx = (int)((n + 255) / 256);
    if (bx > 4096 / layers + 1) bx = 4096 / layers + 1;
    COMMU_LAUNCH(mems_update_kernel, dim3(bx, layers), dim3(256), 0, stream, (const bf16*)hids, hid_stride, hid_skip, take,
                 (const bf16*)mems, mem_stride, mem_skip, keep, (bf16*)out, out_stride);
    COMMU_LAUNCH_CHECK();
    return 0;
}
