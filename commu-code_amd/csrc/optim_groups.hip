// Optimiser step with per-tensor groups (gfx950): clipped Adam / AdamW over the WHOLE flat buffers with a learning rate, a
// weight decay and a frozen flag per group, and the global gradient norm over the trainable tensors only.
//
// model._ensure_flat() places every parameter tensor at a multiple of 64 elements and zeroes the gaps, so every 64-element
// block belongs to exactly one tensor: one byte per block (block_group) names the block's group exactly, and a 16-byte unit
// of four elements never straddles a block -- one byte read serves it.  The arithmetic of a unit is adam_update's
// (elementwise.hip) with the group's lr; with one group, decay 0 and nothing frozen the results are bit-identical to it.
#include "common.h"
#include "commu_hip.h"

namespace {

constexpr int MAXG = COMMU_OPTIM_MAX_GROUPS;

struct GroupArgs {          // passed by value: no host-to-device copy per eager step
    float lr[MAXG];
    float wd[MAXG];
    unsigned frozen;        // bit k: group k is frozen
};

// per group {lr_k / bc1, wd_k, 1 - lr_k wd_k, frozen}: staged in LDS once per workgroup
__device__ __forceinline__ f32x4 group_entry(float lr, float wd, bool frozen, float bc1) {
    f32x4 t;
    t[0] = lr / bc1;
    t[1] = wd;
    t[2] = 1.f - lr * wd;
    t[3] = frozen ? 1.f : 0.f;
    return t;
}

template <bool DECOUPLED>
__device__ __forceinline__ void adam_groups_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, bf16* __restrict__ pb, size_t n,
                                                   const unsigned char* __restrict__ block_group, const f32x4* tab, float coef,
                                                   float isb2, float b1, float b2, float eps) {
    // (n is a multiple of 64 and every pointer is 16-byte aligned: checked by the entry points)
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
        const f32x4 t = tab[block_group[i >> 6] & (MAXG - 1)];          // the group of THIS pass's block
        if (t[3] != 0.f) continue;                                      // frozen: nothing read, nothing written
        const float step = t[0], wd = t[1], keep = t[2];
        const f32x4 g4 = *(const f32x4*)(g + i), m4 = *(const f32x4*)(m + i), v4 = *(const f32x4*)(v + i), p4 = *(const f32x4*)(p + i);
        f32x4 mo, vo, po;
        bf16x4 pbo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float gr = g4[e] * coef;
            float pe = p4[e];
            if (DECOUPLED) pe *= keep;                                  // AdamW: p *= 1 - lr_k wd_k, the gradient untouched
            else if (wd != 0.f) gr += wd * pe;                          // Adam: the decay joins the CLIPPED gradient unscaled
            const float mm = b1 * m4[e] + (1.f - b1) * gr;
            const float vv = b2 * v4[e] + (1.f - b2) * gr * gr;
            mo[e] = mm;
            vo[e] = vv;
            po[e] = pe - step * mm / (sqrtf(vv) * isb2 + eps);
            pbo[e] = f2bf(po[e]);
        }
        *(f32x4*)(m + i) = mo;
        *(f32x4*)(v + i) = vo;
        *(f32x4*)(p + i) = po;
        if (pb) *(bf16x4*)(pb + i) = pbo;
    }
}

template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          bf16* __restrict__ pb, size_t n,
                                                          const unsigned char* __restrict__ block_group, GroupArgs ga,
                                                          float b1, float b2, float eps, float bc1, float bc2,
                                                          const float* __restrict__ gnorm, float clip) {
    __shared__ f32x4 tab[MAXG];
    if (threadIdx.x < MAXG)
        tab[threadIdx.x] = group_entry(ga.lr[threadIdx.x], ga.wd[threadIdx.x], (ga.frozen >> threadIdx.x) & 1u, bc1);
    __syncthreads();
    float coef = 1.f;
    if (gnorm != nullptr && clip > 0.f) coef = fminf(1.f, clip / (gnorm[0] + 1e-6f));
    adam_groups_update<DECOUPLED>(p, g, m, v, pb, n, block_group, tab, coef, 1.f / sqrtf(bc2), b1, b2, eps);
}

// the same step with the bias corrections and the group table read from DEVICE memory:
// tab_dev = {1 - b1^t, 1 - b2^t, lr[16], wd[16], frozen[16] (non-zero: frozen)} -- what a captured optimiser graph replays
template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_groups_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ m, float* __restrict__ v,
                                                              bf16* __restrict__ pb, size_t n,
                                                              const unsigned char* __restrict__ block_group,
                                                              const float* __restrict__ tab_dev, float b1, float b2, float eps,
                                                              const float* __restrict__ gnorm, float clip) {
    __shared__ f32x4 tab[MAXG];
    const float bc1 = tab_dev[0], bc2 = tab_dev[1];
    if (threadIdx.x < MAXG)
        tab[threadIdx.x] = group_entry(tab_dev[2 + threadIdx.x], tab_dev[2 + MAXG + threadIdx.x],
                                       tab_dev[2 + 2 * MAXG + threadIdx.x] != 0.f, bc1);
    __syncthreads();
    float coef = 1.f;
    if (gnorm != nullptr && clip > 0.f) coef = fminf(1.f, clip / (gnorm[0] + 1e-6f));
    adam_groups_update<DECOUPLED>(p, g, m, v, pb, n, block_group, tab, coef, 1.f / sqrtf(bc2), b1, b2, eps);
}

// sumsq_partial_kernel (elementwise.hip) with the units of frozen blocks taken as zero WITHOUT being read: the same loop, the
// same order of additions (x + 0 is x), so with nothing frozen the result is commu_grad_norm's bit for bit
__device__ __forceinline__ f32x4 unit_or_zero(const float* __restrict__ g, const unsigned char* __restrict__ block_group,
                                              unsigned frozen, size_t i) {
    if ((frozen >> (block_group[i >> 6] & (MAXG - 1))) & 1u) return (f32x4){0.f, 0.f, 0.f, 0.f};
    return *(const f32x4*)(g + i);
}

__global__ __launch_bounds__(256) void sumsq_groups_partial_kernel(const float* __restrict__ g, size_t n,
                                                                   const unsigned char* __restrict__ block_group,
                                                                   unsigned frozen, float* __restrict__ part) {
    __shared__ float red[4];
    float s = 0.f;
    const size_t step = (size_t)gridDim.x * 1024;
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    for (; i + 3 * step + 3 < n; i += 4 * step) {
        const f32x4 v0 = unit_or_zero(g, block_group, frozen, i), v1 = unit_or_zero(g, block_group, frozen, i + step),
                    v2 = unit_or_zero(g, block_group, frozen, i + 2 * step), v3 = unit_or_zero(g, block_group, frozen, i + 3 * step);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += v0[e] * v0[e] + v1[e] * v1[e] + v2[e] * v2[e] + v3[e] * v3[e];
    }
    for (; i < n; i += step) {          // (n is a multiple of 64: a unit is whole)
        const f32x4 v = unit_or_zero(g, block_group, frozen, i);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void sumsq_groups_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = sqrtf(s);
}

int groups_blocks(size_t n) {
    const size_t b = (n / 4 + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));          // the cap of commu_adam_step's grid
}

bool groups_refused(const void* p, const void* g, const void* m, const void* v, const void* pb, size_t n,
                    const void* block_group) {
    if ((n & 63) != 0 || block_group == nullptr) return true;
    return ((((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) != 0) || (((size_t)pb & 15) != 0);
}

}  // namespace

extern "C" int commu_adam_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n,
                                      const unsigned char* block_group, int ngroups, const float* lr, const float* weight_decay,
                                      unsigned frozen_mask, int decoupled, float beta1, float beta2, float eps, int step,
                                      const float* gnorm, float clip, hipStream_t stream) {
    if (ngroups < 1 || ngroups > MAXG || lr == nullptr || weight_decay == nullptr) return -22;
    if (groups_refused(p, g, m, v, p_bf16, n, block_group)) return -22;
    if (n == 0) return 0;
    GroupArgs ga;
    for (int k = 0; k < MAXG; ++k) {
        ga.lr[k] = k < ngroups ? lr[k] : 0.f;
        ga.wd[k] = k < ngroups ? weight_decay[k] : 0.f;
    }
    ga.frozen = frozen_mask | (ngroups < MAXG ? ~0u << ngroups : 0u);          // a group number past the table: nothing is touched
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    if (decoupled)
        COMMU_LAUNCH(adam_groups_kernel<true>, dim3(groups_blocks(n)), dim3(256), 0, stream, p, g, m, v, (bf16*)p_bf16, n,
                     block_group, ga, beta1, beta2, eps, bc1, bc2, gnorm, clip);
    else
        COMMU_LAUNCH(adam_groups_kernel<false>, dim3(groups_blocks(n)), dim3(256), 0, stream, p, g, m, v, (bf16*)p_bf16, n,
                     block_group, ga, beta1, beta2, eps, bc1, bc2, gnorm, clip);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_adam_step_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n,
                                          const unsigned char* block_group, const float* table, int decoupled, float beta1,
                                          float beta2, float eps, const float* gnorm, float clip, hipStream_t stream) {
    if (table == nullptr) return -22;
    if (groups_refused(p, g, m, v, p_bf16, n, block_group)) return -22;
    if (n == 0) return 0;
    if (decoupled)
        COMMU_LAUNCH(adam_groups_dev_kernel<true>, dim3(groups_blocks(n)), dim3(256), 0, stream, p, g, m, v, (bf16*)p_bf16, n,
                     block_group, table, beta1, beta2, eps, gnorm, clip);
    else
        COMMU_LAUNCH(adam_groups_dev_kernel<false>, dim3(groups_blocks(n)), dim3(256), 0, stream, p, g, m, v, (bf16*)p_bf16, n,
                     block_group, table, beta1, beta2, eps, gnorm, clip);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_grad_norm_groups(const float* g, size_t n, const unsigned char* block_group, unsigned frozen_mask,
                                      float* part, int npart, float* out, hipStream_t stream) {
    if (npart <= 0 || npart > 1024) return -22;
    if ((n & 63) != 0 || block_group == nullptr || (((size_t)g) & 15) != 0) return -22;
    COMMU_LAUNCH(sumsq_groups_partial_kernel, dim3(npart), dim3(256), 0, stream, g, n, block_group, frozen_mask, part);
    COMMU_LAUNCH(sumsq_groups_final_kernel, dim3(1), dim3(64), 0, stream, part, npart, out);
    COMMU_LAUNCH_CHECK();
    return 0;
}
