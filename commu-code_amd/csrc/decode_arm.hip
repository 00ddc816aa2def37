// Request pool (gfx950): arm decode slots for any request in ONE launch between two replays of the iteration graph.
// The request store holds, per entry, what a slot needs at the start of an attempt (include/commu_hip.h,
// commu_decode_arm_args); a job (slot, entry) copies the entry's K/V image into the slot's first rows and the entry's
// rows into the slot arrays.  Two copy kernels over the one argument block, which differ in how they move the image:
//   commu_decode_arm         one 64-lane wave per (job, layer, head) moves that head's rows of every cache tensor with
//     16-byte loads and stores, so 256 jobs are 256 * L * H independent waves and not one latency chain.  Right for the 16
//     context rows of a pool without prompts, and one dependent load-store loop for a 1000-row image.
//   commu_decode_arm_primed  for the images of replayed prompts, hundreds to thousands of rows: the rows of a (layer, head)
//     are cut into chunks of ARM_CHUNK rows and every chunk is a workgroup of its own: grid (L H, jobs, chunks), 128
//     threads, each thread issuing ARM_UNROLL independent 16-byte loads before its first store (ARM_CHUNK rows of a
//     128-byte row are exactly one such pass: 8 KiB per tensor and workgroup in flight).  A chunk beyond the job's row
//     count exits.
// The slot arrays are one routine for both (arm_slot_arrays): the L H waves of a job -- the L H chunk-0 workgroups of the
// primed launch -- share every row between them (group g of G with T threads takes elements g * T + thread, + G T, ...).
// Plain vector stores only; no atomics, no LDS, no synchronisation.
#include <stdint.h>

#include "common.h"
#include "form.h"
#include "commu_hip.h"

namespace {

constexpr int ARM_CHUNK = 64;            // (primed) image rows per chunk workgroup
constexpr int ARM_THREADS = 128;
constexpr int ARM_UNROLL = 4;            // independent 16-byte loads per thread ahead of the first store

struct ArmRange {          // this wave's / workgroup's share of a job's slot-array rows
    int first, stride;
};

template <typename T>
__device__ __forceinline__ void arm_copy(T* __restrict__ dst, const T* __restrict__ src, int n, ArmRange r) {
    for (int i = r.first; i < n; i += r.stride) dst[i] = src[i];
}

template <typename T>
__device__ __forceinline__ void arm_fill(T* __restrict__ dst, T v, int n, ArmRange r) {
    for (int i = r.first; i < n; i += r.stride) dst[i] = v;
}

// The slot-array half of job j = (slot, entry), for both launches.  klen: what the slot's length becomes; head: how many
// words of the entry's sequence head are copied; r: the caller's share of every row; one: the job's one thread that
// writes the single words; wave: the job's one whole, converged 64-lane wave (lane: its lane) that resets the form state.
// FORM: the launch that also arms the form rule (form.h); without it the kernels are the ones they always were.
template <bool FORM>
__device__ __forceinline__ void arm_slot_arrays(const commu_decode_arm_args& a, int slot, int entry, int j, int klen, int head,
                                                ArmRange r, bool one, bool wave, int lane) {
    const size_t s = (size_t)slot, e = (size_t)entry;
    if (one) a.klen[slot] = klen;
    arm_copy(a.state + s * a.nf, a.e_state + e * a.nf, a.nf, r);
    arm_copy(a.seq + s * a.ld_seq, a.e_seq + e * a.ld_head, head, r);
    arm_copy(a.chord_tok + s * a.ld_chord, a.e_chord_tok + e * a.ld_chord, a.ld_chord, r);
    arm_copy(a.chord_pos + s * a.ld_chord, a.e_chord_pos + e * a.ld_chord, a.ld_chord, r);
    arm_fill(a.wrong + s * a.ld_wrong, (unsigned char)0, a.ld_wrong, r);
    arm_copy(a.utable + s * a.ld_u, a.variates + (size_t)j * a.ld_u, a.ld_u, r);
    if (a.seq_logp != nullptr) arm_fill(a.seq_logp + s * a.ld_seq * 2, __int_as_float(0x7fc00000), 2 * a.ld_seq, r);
    if (a.trace != nullptr && a.ld_trace > 0) {
        if (a.e_trace != nullptr)
            arm_copy(a.trace + s * a.ld_trace, a.e_trace + e * a.ld_trace, a.ld_trace, r);
        else
            arm_fill(a.trace + s * a.ld_trace, 0, a.ld_trace, r);
    }
    if (a.bias != nullptr && a.e_bias != nullptr) arm_copy(a.bias + s * a.ld_bias, a.e_bias + e * a.ld_bias, a.ld_bias, r);
    if (a.cls_ctl != nullptr && a.e_cls != nullptr) arm_copy(a.cls_ctl + s * 32, a.e_cls + e * 32, 32, r);
    if (one) {
        if (a.temperature_rows != nullptr && a.e_temperature != nullptr) a.temperature_rows[slot] = a.e_temperature[entry];
        if (a.top_k_rows != nullptr && a.e_top_k != nullptr) a.top_k_rows[slot] = a.e_top_k[entry];
        if (a.top_p_rows != nullptr && a.e_top_p != nullptr) a.top_p_rows[slot] = a.e_top_p[entry];
        if (a.gram_on != nullptr && a.e_gram_on != nullptr) a.gram_on[slot] = a.e_gram_on[entry];
        if (a.harm_on != nullptr && a.e_harm_on != nullptr) a.harm_on[slot] = a.e_harm_on[entry];
        if (a.order_ctl != nullptr && a.e_order != nullptr) a.order_ctl[slot] = a.e_order[entry];
        if (a.voice_ctl != nullptr && a.e_voice != nullptr) a.voice_ctl[slot] = a.e_voice[entry];
        if (a.density_ctl != nullptr && a.e_density != nullptr) a.density_ctl[slot] = a.e_density[entry];
        if (a.interval_ctl != nullptr && a.e_interval != nullptr) a.interval_ctl[slot] = a.e_interval[entry];
        if (a.onset_ctl != nullptr && a.e_onset != nullptr) a.onset_ctl[slot] = a.e_onset[entry];
        if (a.guide_ctl != nullptr && a.e_guide != nullptr) a.guide_ctl[slot] = a.e_guide[entry];
        if (a.art_ctl != nullptr && a.e_art != nullptr) a.art_ctl[slot] = a.e_art[entry];
    }
    // (FORM) the slot's form word, and its form state as a load leaves it: nothing replayed, the BARs of the entry's sequence
    // head recorded (one wave)
    if constexpr (FORM) {
        if (one) {
            if (a.form_ctl != nullptr && a.e_form != nullptr) a.form_ctl[slot] = a.e_form[entry];
            if (a.form_tok != nullptr) a.form_tok[slot] = -1;
        }
        if (a.form_state != nullptr && wave)
            form_reset_row(a.form_state + s * FS_COUNT, a.e_seq + e * a.ld_head, min(max(a.e_state[e * a.nf], 0), a.ld_head),
                           lane);
    }
}

template <bool FORM>
__global__ __launch_bounds__(64) void decode_arm_kernel(const commu_decode_arm_args a) {
    const int j = blockIdx.y;
    const int slot = a.jobs[2 * j], entry = a.jobs[2 * j + 1];
    if (slot < 0 || slot >= a.B || entry < 0 || entry >= a.Rcap) return;
    const int lane = threadIdx.x;
    const int lh = blockIdx.x;                         // layer * H + head
    const int l = lh / a.H, h = lh - l * a.H;
    const int n = min(max(a.e_klen0[entry], 0), min(a.ctx_rows, a.Lmax));

    // ---- the K/V image: rows 0 .. n - 1 of this (layer, head) in every cache tensor
#pragma unroll
    for (int i = 0; i < 4; ++i) {          // (unrolled: the arrays of the argument block are read at constant offsets)
        if (i >= a.n_cache) break;
        const int rb = a.row_bytes[i];
        unsigned char* dst = static_cast<unsigned char*>(a.cache[i]) + (((size_t)l * a.B + slot) * a.H + h) * a.Lmax * rb;
        const unsigned char* src =
            static_cast<const unsigned char*>(a.image[i]) + (((size_t)l * a.Rcap + entry) * a.H + h) * a.ctx_rows * rb;
        const int bytes = n * rb;
        if ((rb & 15) == 0) {
            uint4* d = reinterpret_cast<uint4*>(dst);
            const uint4* s = reinterpret_cast<const uint4*>(src);
            for (int q = lane; q < bytes / 16; q += 64) d[q] = s[q];
        } else {
            for (int q = lane; q < bytes; q += 64) dst[q] = src[q];
        }
    }

    // ---- the slot arrays: the job's waves share every row; the whole sequence head is the entry's
    arm_slot_arrays<FORM>(a, slot, entry, j, n, a.ld_head, ArmRange{lh * 64 + lane, (int)gridDim.x * 64}, lh == 0 && lane == 0,
                          lh == 0, lane);
}

// rows [drow, drow + rows) of one cache tensor from rows [srow, ..) of its image; rb bytes per row.  Rows are contiguous,
// so a chunk is one span: full passes of ARM_UNROLL independent 16-byte loads per thread ahead of the first store, then
// what is left one vector at a time (at most ARM_UNROLL - 1 per thread).
__device__ __forceinline__ void arm_rows(void* cache, const void* image, int rb, size_t drow, size_t srow, int rows, int tid) {
    unsigned char* dst = static_cast<unsigned char*>(cache) + drow * rb;
    const unsigned char* src = static_cast<const unsigned char*>(image) + srow * rb;
    const int bytes = rows * rb;
    if ((rb & 15) == 0) {
        uint4* d = reinterpret_cast<uint4*>(dst);
        const uint4* s = reinterpret_cast<const uint4*>(src);
        const int nq = bytes >> 4;
        int q = tid;
        static_assert(ARM_UNROLL == 4, "the full pass names four registers");
        for (; q + 3 * ARM_THREADS < nq; q += ARM_UNROLL * ARM_THREADS) {
            const uint4 v0 = s[q], v1 = s[q + ARM_THREADS], v2 = s[q + 2 * ARM_THREADS], v3 = s[q + 3 * ARM_THREADS];
            d[q] = v0;
            d[q + ARM_THREADS] = v1;
            d[q + 2 * ARM_THREADS] = v2;
            d[q + 3 * ARM_THREADS] = v3;
        }
        for (; q < nq; q += ARM_THREADS) d[q] = s[q];
    } else {
        for (int q = tid; q < bytes; q += ARM_THREADS) dst[q] = src[q];
    }
}

__host__ __device__ __forceinline__ int arm_rows_cap(int ctx_rows, int Lmax, int grid_rows) {
    const int r = ctx_rows < Lmax ? ctx_rows : Lmax;
    return (grid_rows > 0 && grid_rows < r) ? grid_rows : r;
}

template <bool FORM>
__global__ __launch_bounds__(ARM_THREADS) void decode_arm_primed_kernel(const commu_decode_arm_args a) {
    const int j = blockIdx.y;
    const int slot = a.jobs[2 * j], entry = a.jobs[2 * j + 1];
    if (slot < 0 || slot >= a.B || entry < 0 || entry >= a.Rcap) return;
    const int tid = threadIdx.x;
    const int lh = blockIdx.x;                         // layer * H + head
    const int l = lh / a.H, h = lh - l * a.H;
    const int k = max(a.e_klen0[entry], 0);
    const int n = min(k, arm_rows_cap(a.ctx_rows, a.Lmax, a.grid_rows));
    const int row0 = (int)blockIdx.z * ARM_CHUNK;
    if (row0 >= n && blockIdx.z != 0) return;          // (chunk 0 stays for the slot arrays, it copies no row when n == 0)

    // ---- the K/V image: rows row0 .. row0 + rows - 1 of this (layer, head) in every cache tensor
    // (one call per tensor: the arrays of the argument block are read at constant offsets)
    const int rows = max(min(ARM_CHUNK, n - row0), 0);
    const size_t drow = (((size_t)l * a.B + slot) * a.H + h) * a.Lmax + row0;
    const size_t srow = (((size_t)l * a.Rcap + entry) * a.H + h) * a.ctx_rows + row0;
    arm_rows(a.cache[0], a.image[0], a.row_bytes[0], drow, srow, rows, tid);
    arm_rows(a.cache[1], a.image[1], a.row_bytes[1], drow, srow, rows, tid);
    if (a.n_cache == 4) {
        arm_rows(a.cache[2], a.image[2], a.row_bytes[2], drow, srow, rows, tid);
        arm_rows(a.cache[3], a.image[3], a.row_bytes[3], drow, srow, rows, tid);
    }
    if (blockIdx.z != 0) return;

    // ---- the slot arrays: the job's chunk-0 workgroups share every row; the sequence head up to the record's length word
    arm_slot_arrays<FORM>(a, slot, entry, j, a.ring != 0 ? k : n, min(max(a.e_state[(size_t)entry * a.nf], 0), a.ld_head),
                          ArmRange{lh * ARM_THREADS + tid, (int)gridDim.x * ARM_THREADS}, lh == 0 && tid == 0,
                          lh == 0 && tid < 64, tid);
}

// What both entry points check, in this order: -22 refused, 0 no job (nothing else is looked at), 1 launch.
int arm_check(const commu_decode_arm_args* p, bool primed) {
    if (p == nullptr || p->struct_bytes != sizeof(commu_decode_arm_args)) return -22;
    if (p->B < 1 || p->Rcap < 1 || p->njobs < 0 || p->njobs > p->B || p->njobs > 65535) return -22;
    if (p->njobs == 0) return 0;
    if (p->L < 1 || p->H < 1 || p->Lmax < 1 || p->ctx_rows < 1 || p->nf < 1 || p->ld_head < 1 || p->ld_head > p->ld_seq ||
        p->ld_chord < 1 || p->ld_wrong < 1 || p->ld_u < 1 || p->ld_trace < 0 || (p->n_cache != 2 && p->n_cache != 4))
        return -22;
    if (primed ? (p->grid_rows < 0 || (p->ring != 0 && p->ctx_rows > p->Lmax)) : (p->ring != 0 || p->grid_rows != 0)) return -22;
    if (p->bias != nullptr && p->e_bias != nullptr && p->ld_bias < 1) return -22;
    if (p->jobs == nullptr || p->variates == nullptr || p->klen == nullptr || p->e_klen0 == nullptr || p->state == nullptr ||
        p->e_state == nullptr || p->seq == nullptr || p->e_seq == nullptr || p->chord_tok == nullptr ||
        p->chord_pos == nullptr || p->e_chord_tok == nullptr || p->e_chord_pos == nullptr || p->wrong == nullptr ||
        p->utable == nullptr)
        return -22;
    if (((reinterpret_cast<uintptr_t>(p->jobs) | reinterpret_cast<uintptr_t>(p->variates)) & 3u) != 0) return -22;
    for (int i = 0; i < p->n_cache; ++i) {
        if (p->row_bytes[i] < 1 || p->cache[i] == nullptr || p->image[i] == nullptr) return -22;
        if ((p->row_bytes[i] & 15) == 0 &&
            ((reinterpret_cast<uintptr_t>(p->cache[i]) | reinterpret_cast<uintptr_t>(p->image[i])) & 15u) != 0)
            return -22;
    }
    if ((long long)p->L * p->H > 2147483647LL) return -22;
    return 1;
}

}  // namespace

extern "C" int commu_decode_arm_args_bytes(void) { return (int)sizeof(commu_decode_arm_args); }

extern "C" int commu_decode_arm_primed_args_bytes(void) { return (int)sizeof(commu_decode_arm_primed_args); }

extern "C" int commu_decode_arm_primed_chunk_rows(void) { return ARM_CHUNK; }

extern "C" int commu_decode_arm(const commu_decode_arm_args* p, hipStream_t stream) {
    const int go = arm_check(p, false);
    if (go != 1) return go;
    if (p->form_ctl != nullptr || p->form_state != nullptr)
        COMMU_LAUNCH(decode_arm_kernel<true>, dim3(p->L * p->H, p->njobs), dim3(64), 0, stream, *p);
    else
        COMMU_LAUNCH(decode_arm_kernel<false>, dim3(p->L * p->H, p->njobs), dim3(64), 0, stream, *p);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_decode_arm_primed(const commu_decode_arm_primed_args* p, hipStream_t stream) {
    const int go = arm_check(p, true);
    if (go != 1) return go;
    const int chunks = (arm_rows_cap(p->ctx_rows, p->Lmax, p->grid_rows) + ARM_CHUNK - 1) / ARM_CHUNK;
    if (chunks > 65535) return -22;
    if (p->form_ctl != nullptr || p->form_state != nullptr)
        COMMU_LAUNCH(decode_arm_primed_kernel<true>, dim3(p->L * p->H, p->njobs, chunks), dim3(ARM_THREADS), 0, stream, *p);
    else
        COMMU_LAUNCH(decode_arm_primed_kernel<false>, dim3(p->L * p->H, p->njobs, chunks), dim3(ARM_THREADS), 0, stream, *p);
    COMMU_LAUNCH_CHECK();
    return 0;
}
