// Request pool (gfx950): arm decode slots for any request in ONE launch between two replays of the iteration graph.
// The request store holds, per entry, what a slot needs at the start of an attempt (include/commu_hip.h,
// commu_decode_arm_args); a job (slot, entry) copies the entry's K/V image into the slot's first rows and the entry's
// rows into the slot arrays.  It is a copy kernel: one 64-lane wave per (job, layer, head) moves that head's rows of
// every cache tensor with 16-byte loads and stores, and the waves of a job share the slot arrays' rows between them
// (wave w of W takes elements w * 64 + lane, + 64 W, ...), so 256 jobs are 256 * L * H independent waves and not one
// latency chain.  Plain vector stores only; no atomics, no LDS, no synchronisation.
#include <stdint.h>

#include "common.h"
#include "form.h"
#include "commu_hip.h"

namespace {

struct ArmRange {          // this wave's share of a job's slot-array rows
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

// FORM: the launch that also arms the form rule (form.h); without it the kernel is the one it always was
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

    // ---- the slot arrays: the job's waves share every row
    const ArmRange r{lh * 64 + lane, (int)gridDim.x * 64};
    const size_t s = (size_t)slot, e = (size_t)entry;
    if (lh == 0 && lane == 0) a.klen[slot] = n;
    arm_copy(a.state + s * a.nf, a.e_state + e * a.nf, a.nf, r);
    arm_copy(a.seq + s * a.ld_seq, a.e_seq + e * a.ld_head, a.ld_head, r);
    arm_copy(a.chord_tok + s * a.ld_chord, a.e_chord_tok + e * a.ld_chord, a.ld_chord, r);
    arm_copy(a.chord_pos + s * a.ld_chord, a.e_chord_pos + e * a.ld_chord, a.ld_chord, r);
    arm_fill(a.wrong + s * a.ld_wrong, (unsigned char)0, a.ld_wrong, r);
    arm_copy(a.utable + s * a.ld_u, a.variates + (size_t)j * a.ld_u, a.ld_u, r);
    if (a.seq_logp != nullptr) arm_fill(a.seq_logp + s * a.ld_seq * 2, __int_as_float(0x7fc00000), 2 * a.ld_seq, r);
    if (a.trace != nullptr && a.ld_trace > 0) arm_fill(a.trace + s * a.ld_trace, 0, a.ld_trace, r);
    if (a.bias != nullptr && a.e_bias != nullptr) arm_copy(a.bias + s * a.ld_bias, a.e_bias + e * a.ld_bias, a.ld_bias, r);
    if (a.cls_ctl != nullptr && a.e_cls != nullptr) arm_copy(a.cls_ctl + s * 32, a.e_cls + e * 32, 32, r);
    if (lh == 0 && lane == 0) {
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
        if (lh == 0 && lane == 0) {
            if (a.form_ctl != nullptr && a.e_form != nullptr) a.form_ctl[slot] = a.e_form[entry];
            if (a.form_tok != nullptr) a.form_tok[slot] = -1;
        }
        if (a.form_state != nullptr && lh == 0 && lane < 64)
            form_reset_row(a.form_state + s * FS_COUNT, a.e_seq + e * a.ld_head, min(max(a.e_state[e * a.nf], 0), a.ld_head),
                           lane);
    }
}

}  // namespace

extern "C" int commu_decode_arm_args_bytes(void) { return (int)sizeof(commu_decode_arm_args); }

extern "C" int commu_decode_arm(const commu_decode_arm_args* p, hipStream_t stream) {
    if (p == nullptr || p->struct_bytes != sizeof(commu_decode_arm_args)) return -22;
    if (p->B < 1 || p->Rcap < 1 || p->njobs < 0 || p->njobs > p->B || p->njobs > 65535) return -22;
    if (p->njobs == 0) return 0;
    if (p->L < 1 || p->H < 1 || p->Lmax < 1 || p->ctx_rows < 1 || p->nf < 1 || p->ld_head < 1 || p->ld_head > p->ld_seq ||
        p->ld_chord < 1 || p->ld_wrong < 1 || p->ld_u < 1 || p->ld_trace < 0 || (p->n_cache != 2 && p->n_cache != 4))
        return -22;
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
    if (p->form_ctl != nullptr || p->form_state != nullptr)
        COMMU_LAUNCH(decode_arm_kernel<true>, dim3(p->L * p->H, p->njobs), dim3(64), 0, stream, *p);
    else
        COMMU_LAUNCH(decode_arm_kernel<false>, dim3(p->L * p->H, p->njobs), dim3(64), 0, stream, *p);
    COMMU_LAUNCH_CHECK();
    return 0;
}
