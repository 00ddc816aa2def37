/* commu_hip.h -- C ABI of libcommu_hip.so: MI355X (gfx950) kernels for ComMU's Transformer-XL
 * training + sampling hot path.
 *
 * The reference (POZAlabs/ComMU-code) is pure Python on PyTorch: it has no FFI layer.  Each
 * entry point below replaces the PyTorch op sequence at the cited reference lines
 * (paths relative to the reference repository root) and is what a binding for that path
 * would call; the ctypes binding a maintainer would add is shown in INTEGRATION.md and
 * shipped as commu-code_amd/commu_amd/_lib.py.
 *
 * Conventions: plain device pointers + sizes, no framework types; every call enqueues work on
 * `stream` and returns 0, a positive hipError_t, or -22 (EINVAL) for an unsupported shape; no
 * call allocates, synchronises or throws.  "bf16" buffers are `void*` to 16-bit bfloat16.
 * Activation rows are time-major, row m = t * B + b, exactly the reference's [T, B, *] layout.
 */
#ifndef COMMU_HIP_H
#define COMMU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- GEMM (nn.Linear forward/backward: model.py:205,212,278,164,167,46; autograd of the same) */
enum {
    COMMU_EPI_BIAS = 1,      /* C += bias[n]                    (Linear bias, model.py:164,167,40) */
    COMMU_EPI_RELU = 2,      /* C = max(C, 0)                   (nn.ReLU, model.py:165)            */
    COMMU_EPI_RESID = 4,     /* C += resid[m, n] (bf16)         (w + attn_out / inp + core_out)    */
    COMMU_EPI_RELUMASK = 8,  /* C = relu_mask[m,n] > 0 ? C : 0  (ReLU backward)                    */
    COMMU_EPI_OUT_F32 = 16,  /* C is fp32 (default bf16)                                           */
    COMMU_EPI_DROPOUT = 32,  /* C = keep(drop_seed, m*N+n) ? C/(1-p) : 0  (nn.Dropout, model.py:166,168,210) */
    /* ReLU backward from ONE BIT per element instead of the bf16 activations (1/16 of the bytes).  SIGNBITS_OUT: the
     * `relu_mask` argument is an OUTPUT of commu_gemm_nt_signbits_words(M, N, K) 32-bit words receiving (C > 0) after the
     * epilogue, in a layout private to the kernel; RELUBITS: `relu_mask` is such a buffer written by a GEMM of the same
     * M x N, C = bit ? C * mask_scale : 0.  Only shapes with a non-zero word count; no RESID / RELUMASK / OUT_F32. */
    COMMU_EPI_SIGNBITS_OUT = 64,
    COMMU_EPI_RELUBITS = 128
};
/* words of the sign-bit buffer for an M x N output (0: this shape / K does not take the flags above) */
long long commu_gemm_nt_signbits_words(int M, int N, int K, int lda, int ldb, int ldc);
/* C[M,N] = A[M,K] . B[N,K]^T with fused epilogue, applied in this order: bias, relu, dropout, resid,
 * relu-mask (kept values times mask_scale).  K % 32 == 0, lda/ldb % 8 == 0, ldc % 4 == 0. */
int commu_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N,
                       int K, const float* bias, const void* resid, int ldr, const void* relu_mask,
                       int ldm, int flags, unsigned drop_seed, float drop_p, float mask_scale,
                       hipStream_t stream);
/* Decode-step form (M <= 64 rows, K % 128 == 0, K <= 1024) with the PRECEDING LayerNorm fused in (model.py:179,352
 * followed by the Linear of :164 / :205 / :46): C = LN(z)[:, :K] . B^T with epilogue flags BIAS, RELU, RESID, OUT_F32;
 * LN over the first D columns of z (gamma, beta, eps; columns D..K-1 are zero padding); a_out (optional, bf16
 * [M][lda_out]) receives LN(z), which the next residual connection adds.  Other shapes: -22. */
int commu_gemm_nt_ln_bf16(const void* z, int ldz, const float* gamma, const float* beta, int D, float eps,
                          void* a_out, int lda_out, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                          const float* bias, const void* resid, int ldr, int flags, hipStream_t stream);
/* batched form: entry z uses A + z*strideA, B + z*strideB, C + z*strideC, resid + z*strideR (element
 * strides); a 64-wide tile is used when N <= 64 (per-head GEMMs).  Epilogue flags: RESID, OUT_F32.
 * Causal band (tri_B > 0): A is dS by distance, row m = i*tri_B + b is zero (or unwritten) beyond column
 * i + tri_M, so a row tile only contracts columns < i_max + tri_M + 1 (rounded up to 64): the caller
 * guarantees ZEROS in each row from column i + tri_M + 1 up to that limit (commu_attn_bwd_desc.dsk_wedge). */
int commu_gemm_nt_bf16_batched(const void* A, int lda, long long strideA, const void* B, int ldb,
                               long long strideB, void* C, int ldc, long long strideC, int M, int N, int K,
                               const void* resid, int ldr, long long strideR, int flags, int batch,
                               int tri_B, int tri_M, hipStream_t stream);
/* slabs[s][n,k] = sum_{m in slice s} A[m,n] * B[m,k]  (weight gradients dW = dY^T X).
 * mode 1: LDS transpose reads (ds_read_b64_tr_b16); mode 0: 16-bit gathers. */
int commu_gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, float* slabs, int ldc,
                       size_t slab_stride, int M, int N, int K, int nslices, int mode, hipStream_t stream);
/* recommended number of m-slices for the tile the TN kernel picks at this shape (fills the 256 CUs) */
int commu_gemm_tn_slices(int M, int N, int K);
/* batched form: slabs[(z*nslices + s)][n,k] for batch entry z.  Causal band (tri_B > 0): column n of A is
 * zero (or unwritten) in rows m < (n - tri_M) * tri_B, so an output tile starting at n0 skips those rows. */
int commu_gemm_tn_bf16_batched(const void* A, int lda, long long strideA, const void* B, int ldb,
                               long long strideB, float* slabs, int ldc, size_t slab_stride, int M, int N, int K,
                               int nslices, int batch, int tri_B, int tri_M, hipStream_t stream);
/* Grouped form for the weight gradients of a layer (autograd of the nn.Linear calls at model.py:163-169,205,212):
 * up to 8 problems out_p[N_p, K_p] = A_p[M, N_p]^T . B_p[M, K_p] sharing the token count M, ONE launch of the
 * 256 x 256 x 64 eight-phase kernel over (token slice, output tile) workgroups; slice s of problem p lands at
 * slabs[s * slab_stride + out_off_p + n * K_p + k] and is summed by commu_reduce_slabs_f32.
 * N_p, K_p >= 128 and % 8 == 0, lda/ldb % 8 == 0 and >= 128, M >= 4096 (else -22: use commu_gemm_tn_bf16). */
typedef struct commu_tn_problem {
    const void* A;      /* bf16 [M][lda]  (dY)          */
    const void* B;      /* bf16 [M][ldb]  (layer input) */
    int lda, ldb, N, K;
    long long out_off;  /* element offset of this problem's [N, K] block inside a slab */
    long long colsum_off; /* >= 0: the slice's column sums of A (sum_m A[m, n]: the bias gradient of the Linear whose dY this
                           * is, commu/model/model.py:163-169) go to slabs[s * slab_stride + colsum_off + n], n < N -- one
                           * extra MFMA per 64 tokens in the workgroups of the first K tile column, instead of a separate
                           * pass over dY; < 0: none */
} commu_tn_problem;
/* number of token slices that fills the 256 CUs for this group (0: a problem is not eligible) */
int commu_gemm_tn_grouped_slices(const commu_tn_problem* probs, int nprob, int M);
/* the same for a workgroup budget: tiles x slices <= budget (the default above is 128: the launch runs on the side stream
 * beside the backward pass and leaves half of every XCD to it; the LAST launch of a pass, which the main stream ends up
 * waiting for, takes 256) */
int commu_gemm_tn_grouped_slices_budget(const commu_tn_problem* probs, int nprob, int M, int budget);
int commu_gemm_tn_bf16_grouped(const commu_tn_problem* probs, int nprob, int M, float* slabs,
                               long long slab_stride, int nslices, hipStream_t stream);
/* dst[z][r*ldd + c] = (accumulate ? dst : 0) + alpha * sum_s src[(z*nslabs + s)*stride + r*cols + c] */
int commu_reduce_slabs2d_f32(float* dst, int ldd, long long dst_batch_stride, const float* src, int rows, int cols,
                             int nslabs, size_t stride, int batch, int accumulate, float alpha, hipStream_t stream);
/* ---- MX-fp8 GEMM (BASELINE.json configs[4] "fp8 MFMA GEMMs"; the reference has no counterpart: it is the bf16 nn.Linear
 * product of commu_gemm_nt_bf16 with both operands in OCP e4m3 and one E8M0 scale per 32 k, OCP microscaling v1.0).
 * commu_quant_mxfp8: X bf16 [rows][ldx] -> Q e4m3 bytes [rows][ldq] + S scale bytes [rows][lds]; K % 32 == 0.
 *   block scale 2^(floor(log2 amax) - 8), elements rounded to nearest even, saturating at +-448.
 * commu_gemm_nt_mxfp8: C bf16 [M][ldc] = A . B^T with the epilogue flags BIAS, RELU, DROPOUT, RESID of
 *   commu_gemm_nt_bf16 (same order, same dropout element index), fp32 accumulation on
 *   v_mfma_scale_f32_16x16x128_f8f6f4; K % 128 == 0, lda/ldb % 16 == 0, ldsa/ldsb % 4 == 0, ldc % 8 == 0, else -22.
 * Tolerance against the bf16 path is set by e4m3's 3 mantissa bits (tests/test_fp8_gemm_gpu.py states it). */
int commu_quant_mxfp8(const void* X, int ldx, void* Q, int ldq, void* S, int lds, int rows, int K, hipStream_t stream);
int commu_gemm_nt_mxfp8(const void* A, int lda, const void* SA, int ldsa, const void* B, int ldb, const void* SB, int ldsb,
                        void* C, int ldc, int M, int N, int K, const float* bias, const void* resid, int ldr, int flags,
                        unsigned drop_seed, float drop_p, hipStream_t stream);

/* cropping form for zero-padded models (d_head 50 -> 64 ...): the slabs hold the padded [rg*rp, cg*cp] product, its
 * [rt, ct] blocks go to dst [rg*rt, cg*ct]:
 *   dst[((a*rt + r)*cg + c)*ct + k] (+)= alpha * sum_s src[s*stride + ((a*rp + r)*cg + c)*cp + k] */
int commu_reduce_slabs_crop_f32(float* dst, const float* src, int rg, int rt, int rp, int cg, int ct, int cp,
                                int nslabs, size_t stride, int accumulate, float alpha, hipStream_t stream);
/* all reductions of a grouped weight-gradient launch in one: item z applies the cropping form to slabs + src_off with
 * its own destination (plain reduction of [rows, cols] out of a padded [rows_p, cols] block: (1, rows, rows_p, 1, cols,
 * cols)); nitems <= 8 */
typedef struct commu_reduce_item {
    float* dst;
    long long src_off;          /* element offset of the item's block inside a slab */
    int rg, rt, rp, cg, ct, cp;
} commu_reduce_item;
int commu_reduce_slabs_group_f32(const commu_reduce_item* items, int nitems, const float* slabs, int nslabs, size_t stride,
                                 int accumulate, float alpha, hipStream_t stream);
/* dst[i] = (accumulate ? dst[i] : 0) + alpha * sum_s src[s*stride + i] */
int commu_reduce_slabs_f32(float* dst, const float* src, size_t n, int nslabs, size_t stride,
                           int accumulate, float alpha, hipStream_t stream);

/* Zero-padding contract of the row-wise kernels below (embed_fwd, posemb_fwd, layernorm_fwd/bwd): a row may be
 * wider than its D features (pitch ld > D, D % 4 == 0); columns [D, min(ld, roundup(D, 64))) are PADDING: ignored
 * on input, written as zeros on output, so the next GEMM can contract over the padded width (d_model 500 -> 512). */
/* ---- embedding (AdaptiveEmbedding.forward, model.py:409-420) and its gradient */
/* (drop_p > 0: dropout of the scaled embedding, `core_out = self.drop(word_emb)`, model.py:585;
 *  every dropout in this ABI is the counter-based mask keep(seed, element index): a 32-bit integer hash of the
 *  index, KEYED by the seed between its two multiply rounds -- see common.h drop_keep and DESIGN.md) */
/* (a token id outside [0, V) -- the reference raises IndexError -- yields a NaN row, hence a NaN loss; likewise
 *  commu_ce_fwd returns NaN for a target outside [0, V): no out-of-bounds access, no silent garbage) */
int commu_embed_fwd(const int64_t* tok, const float* E, void* out_bf16, int ldo, int ntok, int D, int V,
                    float scale, unsigned drop_seed, float drop_p, hipStream_t stream);
int commu_embed_bwd(const int64_t* tok, const void* dX_bf16, int ldx, float* dE, int ntok, int D, int V,
                    float scale, int accumulate, unsigned drop_seed, float drop_p, hipStream_t stream);
/* the same from a token order: perm = stable argsort of tok (int64 [ntok]), offs[v] = first position of id v in the sorted
 * list (int64 [V+1]; ids outside [0, V) fall outside offs[0]..offs[V] and contribute nothing).  Two passes over the
 * sorted list: every wave sums 32 consecutive sorted tokens run by run into the fp32 workspace `ws`
 * (commu_embed_bwd_ws_rows(ntok, V) rows of D floats), then dE[v] (+)= scale * (sum of v's partial rows).  The work of a
 * wave does not depend on how often an id occurs (the pad / start id is a quarter of a real batch); fixed summation order,
 * no atomics. */
int commu_embed_bwd_ws_rows(int ntok, int V);
/* (perm, offs) of the line above from the token ids themselves: a stable counting sort (V <= 1024; -22 otherwise: sort
 * with the framework).  ws: 64 * V ints of scratch.  ids outside [0, V) are left out: offs[V] = number of valid tokens,
 * perm[offs[V] ..) = 0. */
int commu_token_order(const int64_t* tok, int ntok, int V, int64_t* perm, int64_t* offs, int* ws, hipStream_t stream);
int commu_embed_bwd_sorted(const int64_t* perm, const int64_t* offs, const void* dX, int ldx, float* ws, int ntok, int D,
                           int V, float* dE, float scale, int accumulate, unsigned drop_seed, float drop_p,
                           hipStream_t stream);
/* sinusoid table by distance d: out[d] = [sin(p f) | cos(p f)], p = d, or min(d, clamp_len) when clamp_len > 0
 * (PositionalEmbedding, model.py:136-152; cfg.MODEL.clamp_len, model.py:581-582) */
int commu_posemb_fwd(const float* inv_freq, void* out_bf16, int ld, int K, int D, int clamp_len, unsigned drop_seed,
                     float drop_p, hipStream_t stream);

/* ---- LayerNorm (nn.LayerNorm at model.py:171,214; applied :179,352) */
/* y_drop (optional): a second output dropout(y) (the final `self.drop(core_out)`, model.py:601) */
int commu_layernorm_fwd(const void* z, int ldz, const float* gamma, const float* beta, void* y, int ldy,
                        float* mean, float* rstd, int rows, int D, float eps, void* y_drop, int ldyd,
                        unsigned drop_seed, float drop_p, hipStream_t stream);
/* GELU (exact erf form of torch.nn.functional.gelu) as a NON-DEFAULT FFN activation -- the reference's PositionwiseFF uses
 * ReLU (model.py:163-169), which stays the default and the parity mode; BASELINE.json's north star names a GELU-FFN:
 *   fwd: out[m,n] = dropout(gelu(z[m,n]))          bwd: dz[m,n] = dy[m,n] * keep/(1-p) * gelu'(z[m,n])
 * bf16 rows, row strides % 8 == 0 and >= cols rounded up to 8 (pad columns are written as zero); the dropout mask is the
 * GEMM epilogue's at that site: keep(drop_seed, m * cols + n). */
int commu_gelu_fwd(const void* z, int ldz, void* out, int ldo, int rows, int cols, unsigned drop_seed, float drop_p,
                   hipStream_t stream);
int commu_gelu_bwd(const void* dy, int lddy, const void* z, int ldz, void* dz, int lddz, int rows, int cols,
                   unsigned drop_seed, float drop_p, hipStream_t stream);
int commu_layernorm_bwd_nblocks(int rows);
/* part: [nblocks][3][D] partial column sums of (dy*xhat, dy, dz) */
/* dz_masked (optional): dz through the dropout that followed the Linear feeding this LayerNorm
 * (dz * keep/(1-p)); when given, part[:,2] holds ITS column sums (that Linear's bias gradient). */
int commu_layernorm_bwd(const void* dy, int lddy, const void* z, int ldz, const float* mean,
                        const float* rstd, const float* gamma, void* dz, int lddz, float* part, int rows,
                        int D, void* dz_masked, int lddzm, unsigned drop_seed, float drop_p,
                        hipStream_t stream);
/* the same with the incoming gradient dy + dy2 (both bf16, summed in fp32): the gradient of a residual branch as a second
 * addend of the LayerNorm backward instead of an auxiliary operand of the GEMM that produced dy (model.py:174-181,348-352) */
int commu_layernorm_bwd_add(const void* dy, int lddy, const void* dy2, int lddy2, const void* z, int ldz,
                            const float* mean, const float* rstd, const float* gamma, void* dz, int lddz, float* part,
                            int rows, int D, void* dz_masked, int lddzm, unsigned drop_seed, float drop_p,
                            hipStream_t stream);
/* dgamma += sum_blocks part[:,0,:], dbeta += part[:,1,:], dbias += part[:,2,:] (each destination optional) */
int commu_layernorm_bwd_reduce(const float* part, int nblk, int D, float* dgamma, float* dbeta, float* dbias,
                               hipStream_t stream);
/* out[c] += alpha * sum_r X[r,c]   (bias gradients).  No atomics, fixed summation order: row slabs are summed into the fp32
 * workspace `ws` (commu_colsum_slabs(rows, cols, element bytes) rows of round_up(cols, 8) floats; 0 rows: not needed),
 * then over the slabs.  Rows must be 16-byte aligned chunks (ldx % 8 == 0 for bf16, % 4 for fp32, round_up(cols) <= ldx);
 * -22 otherwise or when the workspace is missing. */
int commu_colsum_slabs(int rows, int cols, int elem_bytes);
int commu_colsum_bf16(const void* X, int ldx, int rows, int cols, float* out, float* ws, int ws_rows, float alpha,
                      hipStream_t stream);
int commu_colsum_f32(const float* X, int ldx, int rows, int cols, float* out, float* ws, int ws_rows, float alpha,
                     hipStream_t stream);
/* The final passes of a whole backward step in one launch.  A task adds into out[0 .. cols) the column sums of its sources
 * src[src_begin .. src_end) -- fp32 matrices of `rows` rows with row stride ldx (partial rows of commu_colsum_slab_pass or
 * of commu_layernorm_bwd, per-tile sums of the attention kernels) -- each times its alpha, in the order given.  Two tasks
 * must not share an output.  At most COMMU_COLSUM_MAX_TASKS tasks / COMMU_COLSUM_MAX_SOURCES sources per call. */
#define COMMU_COLSUM_MAX_TASKS 48
#define COMMU_COLSUM_MAX_SOURCES 64
typedef struct commu_colsum_source {
    const float* X;
    int ldx, rows;
    float alpha;
    int pad_;
} commu_colsum_source;
typedef struct commu_colsum_task {
    float* out;
    int cols, src_begin, src_end, pad_;
} commu_colsum_task;
int commu_colsum_group_f32(const commu_colsum_task* tasks, int ntask, const commu_colsum_source* srcs, int nsrc,
                           hipStream_t stream);
/* the slab pass of commu_colsum_bf16 / _f32 on its own (elem_bytes 2 / 4): returns the number of partial rows written to
 * ws (row stride = cols rounded up to 8 / 4), 0 when the input is small fp32 and is summed directly, < 0 on error */
int commu_colsum_slab_pass(const void* X, int elem_bytes, int ldx, int rows, int cols, float* ws, int ws_rows,
                           hipStream_t stream);

/* ---- output layer loss (ProjectedAdaptiveLogSoftmax.forward, n_clusters == 0: model.py:64-73) */
int commu_ce_fwd(const float* logits, int ldl, const int64_t* target, float* nll, float* lse, int rows,
                 int V, hipStream_t stream);
int commu_ce_bwd(const float* logits, int ldl, const int64_t* target, const float* lse, const float* g,
                 void* dlogits_bf16, int ldd, int rows, int V, hipStream_t stream);
/* The loss with options (not in the reference): label_smoothing eps in [0, 1), z_loss zeta >= 0 (else -22).  Per row, over
 * the V real tokens (pad columns [V, ld) never enter a sum; the backward writes them as zero):
 *   nll = lse - l_t,  smooth = lse - sum_j l_j / V,  loss = (1 - eps) nll + eps smooth + zeta lse^2
 *   dlogits_j = g ((1 + 2 zeta lse) softmax_j - (1 - eps) [j == t] - eps / V)
 * The forward writes loss, nll and lse; the backward reads that lse.  eps = zeta = 0: the bits of commu_ce_fwd / commu_ce_bwd. */
int commu_ce_fwd_opts(const float* logits, int ldl, const int64_t* target, float* loss, float* nll, float* lse, int rows,
                      int V, float label_smoothing, float z_loss, hipStream_t stream);
int commu_ce_bwd_opts(const float* logits, int ldl, const int64_t* target, const float* lse, const float* g,
                      void* dlogits_bf16, int ldd, int rows, int V, float label_smoothing, float z_loss, hipStream_t stream);
/* Per-class NLL: sum[k] = sum of nll[r], count[k] = number of rows r < rows with class_of_token[target[r]] == k, over the
 * rows whose target is in [0, V) and is not `pad` (the rows of loss weight 0; pad < 0: none).  C <= 8 classes.  Two passes
 * in a fixed order, no atomics: part_sum / part_cnt hold nblk x C partials (nblk <= 1024; commu_nll_by_class_blocks(rows)
 * is the count the host wrappers use), then one workgroup adds them block after block.  Two runs give the same bits. */
int commu_nll_by_class_blocks(int rows);
int commu_nll_by_class(const float* nll, const int64_t* target, const int* class_of_token, int V, int C, int pad, int rows,
                       float* part_sum, int* part_cnt, int nblk, float* sum, int* count, hipStream_t stream);
/* out[0] = scale * mean(nll[target != pad])   (train.py:148-149); keeps the count in cnt_ws; NaN when every
 * target is the pad id (mean of an empty selection, as in the reference) */
int commu_masked_mean(const float* nll, const int64_t* target, int n, int pad, float scale, float* sum_ws,
                      int* cnt_ws, float* out, hipStream_t stream);
int commu_loss_grad(const int64_t* target, int n, int pad, const int* cnt_ws, float scale, float* g,
                    hipStream_t stream);
/* Column-grouped forms for a [T][B] time-major loss whose B columns are B / Bc micro-batches of Bc columns (the reference's
 * `batch_chunk`, train.py:136-155): out[0] = scale * sum_g mean(nll[target != pad] in group g) (scale = 1 / batch_chunk),
 * g[m] = scale * (target[m] != pad) / count_{group of column m % B}.  One forward / backward over all columns then equals
 * the reference's loop over micro-batches.  sum_ws / cnt_ws: B / Bc (<= 16) words; sum_all (optional): sum over all groups. */
int commu_masked_mean_groups(const float* nll, const int64_t* target, int n, int pad, float scale, int B, int Bc,
                             float* sum_ws, int* cnt_ws, float* out, float* sum_all, hipStream_t stream);
int commu_loss_grad_groups(const int64_t* target, int n, int pad, const int* cnt_ws, float scale, int B, int Bc, float* g,
                           hipStream_t stream);

/* ---- optimiser (clip_grad_norm_ + optim.Adam, train.py:159-165,442) on flat fp32 buffers
 * (commu_adam_step / _dev: the 16-byte vector body needs p, g, m, v 16-byte aligned and p_bf16 8-byte aligned or null; any other
 *  slice runs the element-wise body of the same kernel -- same results) */
int commu_grad_norm(const float* g, size_t n, float* part, int npart, float* out_norm, hipStream_t stream);
int commu_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n, float lr,
                    float beta1, float beta2, float eps, int step, const float* gnorm, float clip,
                    hipStream_t stream);
/* The same step with {lr, 1 - beta1^t, 1 - beta2^t} read from DEVICE memory (`scal`, three floats): the form a
 * hipGraph-captured training step replays; commu_adam_bias_corrections (host-only, no stream) gives the two
 * corrections exactly as commu_adam_step computes them. */
int commu_adam_step_dev(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n, const float* scal,
                        float beta1, float beta2, float eps, const float* gnorm, float clip, hipStream_t stream);
int commu_adam_bias_corrections(float beta1, float beta2, int step, float* out2);
/* ---- the same step with per-tensor GROUPS (optim.Adam's `weight_decay`, train.py:442-443, which the step above lacks;
 * torch.optim param_groups with their own lr / weight_decay; tensors with requires_grad = False).  The buffers are WHOLE
 * flat buffers in which every tensor starts at a multiple of 64 elements and the gaps are zero: block_group (device,
 * n / 64 bytes) holds the group number of every 64-element block.  Per element of group k, coef the clip coefficient:
 *   decoupled == 0 (optim.Adam):  gr = coef g + wd_k p, then the step above with lr_k;
 *   decoupled != 0 (optim.AdamW): p *= 1 - lr_k wd_k,   then the step above with lr_k and gr = coef g;
 *   frozen (bit k of frozen_mask): p, m, v and p_bf16 are neither read nor written.
 * lr, weight_decay: HOST arrays of ngroups (<= COMMU_OPTIM_MAX_GROUPS) floats, passed on as kernel arguments (no copy to
 * the device).  With one group, decay 0 and nothing frozen the results are commu_adam_step's bit for bit.
 * -22: n is not a multiple of 64, a buffer is not 16-byte aligned, ngroups out of range; nothing is launched then. */
#define COMMU_OPTIM_MAX_GROUPS 16
int commu_adam_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n,
                           const unsigned char* block_group, int ngroups, const float* lr, const float* weight_decay,
                           unsigned frozen_mask, int decoupled, float beta1, float beta2, float eps, int step,
                           const float* gnorm, float clip, hipStream_t stream);
/* ... with the bias corrections and the group table read from DEVICE memory, 2 + 3 * 16 floats:
 * table = {1 - beta1^t, 1 - beta2^t, lr[16], weight_decay[16], frozen[16] (non-zero: frozen)}; entries past the groups in
 * use must be marked frozen.  Bit-identical to commu_adam_step_groups; what a captured optimiser graph replays. */
int commu_adam_step_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n,
                               const unsigned char* block_group, const float* table, int decoupled, float beta1,
                               float beta2, float eps, const float* gnorm, float clip, hipStream_t stream);
/* commu_grad_norm over the blocks of the groups that are not frozen (clip_grad_norm_, train.py:159-161, when frozen
 * parameters carry no gradient): frozen blocks are not read; deterministic; with frozen_mask == 0 it is commu_grad_norm bit
 * for bit.  -22 as above. */
int commu_grad_norm_groups(const float* g, size_t n, const unsigned char* block_group, unsigned frozen_mask, float* part,
                           int npart, float* out_norm, hipStream_t stream);
/* Dropout seed salt: every dropout site of every kernel uses (its seed argument + salt); the salt is 0 until this call
 * loads it from device memory (src == NULL: back to 0).  Kernel arguments of a captured hipGraph are frozen, the salt
 * is not: a captured training step starts with this call and draws fresh masks on every replay. */
int commu_set_seed_salt(const unsigned* src, hipStream_t stream);
/* g *= min(1, clip / (gnorm[0] + 1e-6)) */
int commu_scale_clip_f32(float* g, size_t n, const float* gnorm, float clip, hipStream_t stream);
int commu_cast_f32_bf16(const float* in, void* out, size_t n, hipStream_t stream);
int commu_cast_bf16_f32(const void* in, float* out, size_t n, hipStream_t stream);
int commu_transpose_bf16(const void* in, int ldi, void* out, int ldo, int rows, int cols, hipStream_t stream);
int commu_transpose_f32_bf16(const float* in, int ldi, void* out, int ldo, int rows, int cols,
                             hipStream_t stream);
int commu_copy_bf16(const void* src, void* dst, size_t n, hipStream_t stream);
/* Up to 32 bf16 transposes in ONE launch: out_i[c][r] = in_i[r][c] (the W^T shadows of every Linear weight that the
 * dX = dY . W GEMMs read, autograd of model.py:205,212,164,167,46: 26 per optimiser step at 6 layers, each a launch of a
 * few dozen workgroups before).  -22 for n > 32. */
typedef struct commu_transpose_item {
    const void* in;
    void* out;
    int ldi, ldo, rows, cols;
} commu_transpose_item;
int commu_transpose_group_bf16(const commu_transpose_item* items, int n, hipStream_t stream);

/* K9  memory update (reference commu/model/model.py:507-538 _update_mems): for each of `layers` layers
 *   out[l] = [ mems[l][mem_skip : mem_skip+keep) ; hids[l][hid_skip : hid_skip+take) ]
 * all counts/strides in bf16 ELEMENTS and multiples of 8 (a time step is a whole [B, Dp] slab); one launch.
 * -22 on a misaligned count or a missing pointer. */
int commu_mems_update(const void* hids, size_t hid_stride, size_t hid_skip, size_t take, const void* mems,
                      size_t mem_stride, size_t mem_skip, size_t keep, void* out, size_t out_stride, int layers,
                      hipStream_t stream);

/* ---- relative-position attention with XL memory
 * (RelPartialLearnableMultiHeadAttn.forward, model.py:313-345; _rel_shift :251-259; mask :549-574) */
typedef struct commu_attn_desc {
    const void* q;   /* bf16, row i: q + (i*B + b)*ld_qkv + h*DH, i in [0,T)   (current segment) */
    const void* k;   /* bf16, row j: k + (j*B + b)*ld_qkv + h*DH, j in [0,T+M) (memory first)    */
    const void* v;
    const void* rd;  /* bf16 [T+M][ld_rd]: r_net(sinusoid(distance d)), distance d = i + M - j   */
    const float* r_w_bias;          /* [H][DH]  (u) */
    const float* r_r_bias;          /* [H][DH]  (v) */
    const unsigned char* reset;     /* [B] reset_mems flags or NULL (model.py:574) */
    int ld_qkv, ld_rd, ld_o;
    int T, M, B, H, DH;
    int same_length, sshift;        /* same_length mask: j <= i - sshift is masked (model.py:549-568) */
    float scale;                    /* 1/sqrt(d_head), model.py:216 */
    float drop_p;                   /* attention-probability dropout (self.dropatt, model.py:337); 0 = off */
    unsigned drop_seed;
} commu_attn_desc;

/* out: bf16 [T*B][ld_o]; lse: fp32 [B][H][T] (natural log).  qu2/qv2 (both or neither): bf16
 * [T*B][H*DH] copies of (q + r_w_bias) and (q + r_r_bias) times scale*log2(e), the operands the
 * backward kernels re-use. */
int commu_relattn_fwd(const commu_attn_desc* d, void* out, float* lse, void* qu2, void* qv2,
                      hipStream_t stream);
/* The same forward pass, additionally SAVING its probabilities for the backward pass (d_head 64, generation-3 forward
 * only; -22 otherwise): pf = commu_attn_pf_bytes(T, M, B, H) bytes, uninitialised -- per (batch, head, 32-query block,
 * 32-key sub-tile the forward visits) a 2176-byte tile: exp2(s - m) as bf16 in the forward kernel's accumulator order,
 * m = the query's running maximum at that sub-tile, the dropout decision in the sign bit, then the 32 values of m.
 * commu_attn_bwd_desc.pf hands it to the query-stationary backward kernel, which then neither recomputes
 * (q + u) . k, the band product / rel-shift, the masks, exp nor the dropout hash (autograd of model.py:313-345). */
int commu_relattn_fwd_save(const commu_attn_desc* d, void* out, float* lse, void* qu2, void* qv2, void* pf,
                           hipStream_t stream);
long long commu_attn_pf_bytes(int T, int M, int B, int H);
/* Forward kernel generation for d_head 64 (process-wide; returns the previous value).  0 (default) and 3: the 32x32-MFMA /
 * transposed-score kernel (relattn3.hip), with or without attention dropout; 2: the 16x16-layout kernel.  Every attention
 * kernel -- both forward generations and the backward family -- regenerates the same dropout mask (relattn.hip DropLane: one
 * mixed word per 2x2 cell of a 32x32 block, one multiply-add per element), so any forward pairs with the backward. */
int commu_attn_fwd_generation(int gen);
/* Backward kernel pair for d_head 64 with a P scratch (process-wide; returns the previous value).  3: relattn_kv3.hip
 * (32 keys per wave on the 32x32 MFMA) behind the 16x16 query-stationary kernel; 4: both kernels on the 32x32 MFMA
 * (relattn_q3.hip: 32 query rows per wave, transposed scores; relattn_kv3.hip transposes its P blocks through LDS);
 * 2: the 16x16-layout pair; 0: the build's default.  The setting fixes the block order in
 * which commu_relattn_bwd_q writes the scratch: both launches of a backward pass must see the same value. */
int commu_attn_bwd_kv_generation(int gen);

/* Backward of commu_relattn_fwd (autograd of model.py:313-345).  Produces dk, dv, the AC part of dq
 * and dS indexed by distance; the caller finishes with two GEMMs per head:
 *   dq[:, h] = dq_ac[:, h] + dsk[h] . Rd[:, h]          (commu_gemm_nt_bf16, RESID)
 *   dRd[:, h] = dsk[h]^T . qv2[:, h] / (scale*log2 e)   (commu_gemm_tn_bf16)
 * and d r_w_bias = colsum(dq_ac), d r_r_bias = colsum(dq - dq_ac). */
typedef struct commu_attn_bwd_desc {
    const void* dout;     /* gradient of the forward output, bf16 [T*B][ld_o] */
    const float* lse;     /* [B][H][T] from the forward */
    const float* delta;   /* [B][H][T]  sum_f dO*O  (commu_attn_delta) */
    const void* qu2;      /* from the forward */
    const void* qv2;
    void* dq_ac;          /* bf16 [T*B][H*DH] */
    void* dk;             /* bf16 rows like k with ld_dqkv */
    void* dv;
    void* dsk;            /* bf16 [H][T*B][ld_dsk]: dS by distance d = i + M - j.  dsk_wedge == 0: ZERO-INITIALISED by
                             the caller; dsk_wedge > 0: uninitialised -- the kernel writes columns 0..i+M of row
                             (i, b) and zeros columns i+M+1 .. i+M+dsk_wedge; the rest is never read by the band
                             GEMMs (only valid without same_length / reset masks) */
    float* du_part;       /* [B*du_rows][H*DH] column sums of dq_ac per query tile */
    int ld_dqkv, ld_dsk;
    int du_rows;          /* = ceil(T / commu_attn_bwd_qrows(T)) */
    int dsk_wedge;
    int dsk_tiled;        /* != 0: dsk is [H][T*B/64][ld_dsk/128] tiles of [64 rows][128 distances] (the layout
                             commu_relattn_bwd_band reads; needs (T*B) % 64 == 0, ld_dsk % 128 == 0); 0: row-major */
    void* p_scratch;      /* NULL, or (d_head 64 only) commu_attn_p_scratch_elems(T, M, B, H) bf16 elements, uninitialised:
                             the query-stationary kernel stores the probabilities it recomputes there and the
                             key-stationary kernel, which must then run AFTER it on the same stream, reads them
                             back instead of recomputing (q+u).k, the band product / rel-shift, masks and exp.  The
                             buffer is private to that pair of launches: its block order is the key-stationary kernel's
                             read order, and with attention dropout a stored value is NEGATIVE where the mask drops the
                             element (the keep decision travels in the sign; that kernel does not hash) */
    const void* o;        /* NULL, or the forward output (bf16 [T*B][ld_o]): the query-stationary kernel then computes
                             delta[b,h,i] = sum_d o . dout itself (commu_attn_delta is not needed) and WRITES it to
                             `delta` for the key-stationary kernel, which must run after it on the same stream */
    const void* pf;       /* NULL, or the buffer commu_relattn_fwd_save filled for this call (needs p_scratch, d_head 64) */
} commu_attn_bwd_desc;
long long commu_attn_p_scratch_elems(int T, int M, int B, int H);
int commu_attn_bwd_qrows(int T);
int commu_relattn_bwd(const commu_attn_desc* d, const commu_attn_bwd_desc* e, hipStream_t stream);
/* the two kernels of commu_relattn_bwd on their own: query-stationary (dq_ac, dsk, du_part) and key-stationary
 * (dk, dv); same descriptors */
int commu_relattn_bwd_q(const commu_attn_desc* d, const commu_attn_bwd_desc* e, hipStream_t stream);
int commu_relattn_bwd_kv(const commu_attn_desc* d, const commu_attn_bwd_desc* e, hipStream_t stream);
/* The two per-head GEMMs above fused into ONE pass over dsk (band.hip): dq = dq_ac + dsk . Rd (bf16, written in
 * place with row stride ld_dq) and slabs[(h * P + p)][Kp][64] = partial dsk^T . qv2 of token-slice pair p, with
 * P = commu_attn_band_pairs(T, B, H) and Kp = T + M rounded up to 512 (the kernel runs one pass per 512 distances,
 * keeping that part of Rd resident in LDS); the caller finishes with
 *   commu_reduce_slabs2d_f32(dRd, ld, 64, slabs, K, 64, P, Kp * 64, H, 0, 1 / (scale * log2 e)).
 * dsk must be TILED (commu_attn_bwd_desc.dsk_tiled).  Needs DH == 64, T + M <= 4096, ld_dsk % 128 == 0, (T * B) % 64 == 0
 * and >= 8192 (else -22: use the two GEMMs on a row-major dsk).
 * band != 0: rows are causal (see commu_gemm_nt_bf16_batched, tri_B = B, tri_M = M) and only the chunks of 256
 * distances that reach the causal edge are read; what lies beyond the edge inside them must be zero.
 * commu_attn_band_pairs: token-slice pairs per head = min(32, 256 / H) -- H * P workgroups fill the 256 CUs once; with 16
 * heads, 16 pairs write half the slab bytes of 32 -- 0: shape not taken.  commu_attn_band_slabs(T, B) = its upper bound 32
 * (or 0), for callers that size a buffer before the head count is known. */
int commu_attn_band_slabs(int T, int B);
int commu_attn_band_pairs(int T, int B, int H);
int commu_relattn_bwd_band(const void* dsk, int ld_dsk, const void* rd, int ld_rd, const void* qv2, int ld_qv,
                           const void* dq_ac, int ld_ac, void* dq, int ld_dq, float* slabs, int T, int M, int B,
                           int H, int DH, int band, hipStream_t stream);
int commu_attn_delta(const void* o, const void* dout, int ld, float* delta, int T, int B, int H, int DH,
                     hipStream_t stream);
/* dst[((b*H+h)*DH+f)*W + off + j] = src[(j*B+b)*ld + h*DH + f] (+ bias[h*DH+f]); zero elsewhere */
int commu_transpose_heads(const void* src, int ld, const float* bias, void* dst, int J, int B, int H,
                          int DH, int W, int off, hipStream_t stream);

/* ---- sampling step of the decode loop (InferenceTask.calc_probs / apply_sampling / infer_token,
 * commu/midi_generator/midi_inferrer.py:209-237), one wave per sequence.  ONE entry point; its arguments are a struct,
 * documented here field by field.  Without a constraint the step is the reference's:
 *   logits[b][1:V] /= temperature IN PLACE (quirk Q5), softmax, pad column 0 -> 0 (Q6), keep the top_k, zero
 *   wrong[b][id] != 0, renormalise, draw by inverse CDF with uniforms[b].  temperature == 0: one-hot argmax.
 *   token[b] = -1 when nothing can be drawn (Q12).
 * struct_bytes: sizeof(commu_sample_args) as the caller compiled it; a value that differs from the library's
 *   (commu_sample_args_bytes()) is refused with -22 before anything else is looked at.
 * WHAT IS DRAWN FROM
 *   logits fp32 [nseq][ld], the ids drawn from are 1 .. V-1 (2 <= V <= 768); wrong (optional) uint8 [nseq][ldw], the
 *   rejected tokens; uniforms fp32 [nseq]; active (optional) uint8 [nseq]: only sequences with active[b] != 0 are processed.
 * CONTROLS
 *   temperature, top_k (1 .. V), top_p: one value for every sequence.  top_p is a nucleus filter after the top-k /
 *   rejected-token step -- an extra mode, the reference has none (generate.py:43-44 offers top_k and temperature only): in
 *   order of decreasing probability (ties: lowest id first) a token is kept while the probability mass before it is
 *   < top_p; survivors renormalised.  top_p >= 1: off; top_p <= 0: -22.
 *   temperature_rows / top_k_rows / top_p_rows: device arrays [nseq], each optional -- null: the scalar applies to every
 *   sequence; given: the scalar is not looked at (the reference samples one sequence at a time with the request's one
 *   temperature / top_k, midi_inferrer.py:209-237).  Sequence b's result is bit for bit that of the scalar call with b's
 *   triple.  top_k values are clamped to [1, V] in the kernel; validating the arrays is the caller's job.
 * RESULTS
 *   token int32 [nseq]; probs_out (optional) fp32 [nseq][ldp], the distribution that was drawn from; logp_out (optional)
 *   fp32 [nseq][2], for the token just drawn (the reference reports no probabilities):
 *   [0] full: log-softmax over ids 1 .. V-1 of the row as this draw used it -- logits / temperature as written back (the
 *       compounded row on a re-draw, Q5, like calc_probs), the raw row for temperature == 0 -- at the drawn id;
 *   [1] kept: log of the token's probability in the distribution it was drawn from (after top-k, rejected tokens, top-p
 *       and renormalisation: apply_sampling, :221-230); exactly 0 for temperature == 0.
 *   Both NaN when nothing could be drawn (token -1, Q12); sequences with active[b] == 0 keep their entries.
 * CONSTRAINTS on what a sequence may draw (the reference has none: a ComMU request's pitch_range, min/max_velocity and
 * inst are conditioning hints only).  Each is optional and each has kernels of its own: with a null pointer the launch
 * is the kernel that never heard of the constraint, with the instructions and the argument block it always had.  With x
 * the value the step computes without them -- logits / temperature, the raw row for temperature == 0 -- the
 * distribution is built from
 *   y[id] = ((x[id] + bias[b][id]) + gram[c][id]) + harm[r][(id - 3) mod 12]      for 1 <= id < V, in this fp32 order
 *   (the third add at the pitch ids 3 <= id <= 130 only; a term whose pointer is null is not added).
 *   ORDER: bias, then grammar row, then harmony row, then top-k, then the rejected-token mask `wrong`, then top-p -- a
 *   banned id takes none of the k places (`wrong`, quirk Q5 of the reference, does).  Max, sum, top-k, top-p and the draw
 *   all work on y; temperature == 0 takes the argmax of y, ties to the lowest id.  A finite entry re-weights an id, -inf
 *   bans it; NaN and +inf are the caller's to refuse (generate.token_constraints).
 *   NOTHING BUT x IS WRITTEN BACK: after the call the logits are bit for bit what the call without constraints leaves,
 *   and a Q5 re-draw from them adds every term once to the compounded row (it sees the same rows c and r).
 *   probs_out is the constrained distribution, exactly 0 at banned ids.  logp_out[0] (full) is the log-softmax of y over
 *   ids 1 .. V-1 at the drawn id; [1] (kept) as above; full <= kept still holds.  A row whose every id is banned, or
 *   whose remaining ids `wrong` removes, takes the Q12 exit: token -1, NaN pair.  The 12 loads per lane of each term use
 *   the index clamp of the lane's logits loads (lanes past V contribute nothing).
 *   bias: fp32 [nseq][ld_bias], ld_bias >= V (else -22): sequence b's additive row.
 *   gram: the EVENT GRAMMAR, fp32 [8][ld_gram], ld_gram >= V (else -22): a row chosen per draw by the sequence's own
 *     state, so that what is drawn survives the reference's token-to-MIDI step, which keeps only the exact groups
 *     Position, Note Velocity, Note On, Note Duration and Position, Chord and silently drops everything else
 *     (commu/preprocessor/encoder/encoder_utils.py:385-419).  Row c is the row for a draw whose PREVIOUS token
 *     seq[b][state[b][F_LEN] - 1] has class c; classes by id: 0 OTHER (pad 0, EOS 1, ids >= 560), 1 BAR (2), 2 PITCH
 *     (3 .. 130), 3 VELOCITY (131 .. 194), 4 CHORD (195 .. 303), 5 DURATION (304 .. 431), 6 POSITION (432 .. 559), found
 *     by range compares.  ROW 7, zeros by convention, is the OFF ROW: the row of a sequence whose switch gram_on[b] is 0.
 *     gram_on: uint8 [nseq]; null: every sequence is on.  Needs state and seq (ld_seq >= 1), else -22.
 *   harm: the HARMONY table, fp32 [111][ld_harm], ld_harm >= 12 (else -22; 16: a row is one 64-byte line): a row chosen
 *     by the chord the sequence is in, so that the pitches drawn fit the chord that is sounding.  Row r holds 12 values by
 *     MIDI pitch class (column 0: C); token id is MIDI pitch id - 3.  r = t - 195 for the last chord token t (195 .. 303:
 *     12 roots x 9 qualities, then Chord_NN) of seq[b][0 .. F_LEN) when the stage runs, 109 while seq holds none.  ROW 110,
 *     zeros by convention, is the OFF ROW: the row of a sequence whose switch harm_on[b] is 0.  harm_on: uint8 [nseq];
 *     null: every sequence is on.  A chord enters seq only as a forced token that the rules take from
 *     chord_tok[b][F_CUR] while they increment F_CUR, with no draw before it is appended, so the kernel reads
 *     chord_tok[b][state[b][F_CUR] - 1] (none while F_CUR is 0).  ONE kernel serves it, with a bias and a grammar: harm
 *     requires bias, gram, seq, state and chord_tok (ld_chord >= 1), else -22; a caller that has no bias or grammar
 *     passes a zero bias row and gram_on zeros (x + 0 is x and row 7 is zeros: bit for bit the draw without them).
 * CLASS-KEYED CONTROLS (the reference samples every token of a request with one temperature / top_k)
 *   cls_ctl: [nseq][8] records of 16 bytes, {float temperature; int top_k; float top_p; int reserved (0)}: sequence b's
 *     table is one 128-byte line.  A draw of sequence b takes its triple from record cls_ctl[b][c], c the class (the
 *     grammar's classes above, 0 .. 6) of the sequence's PREVIOUS token seq[b][min(max(F_LEN, 1), ld_seq) - 1] -- the
 *     grammar's load with the grammar's clamp, whatever gram_on[b] says.  Record 7 is never selected; the host keeps the
 *     sequence's base triple there.  With cls_ctl the triple comes from that record ONLY: temperature / top_k / top_p and
 *     the three *_rows arrays are not looked at.  Everything after the selection is the step above: top_k clamped to
 *     [1, V], temperature == 0 is greedy, the in-place division uses the selected temperature (a Q5 re-draw sees the same
 *     previous token and compounds by the same temperature), then bias, grammar, harmony, top-k, wrong, top-p.  A draw
 *     with record (t, k, p) is BIT FOR BIT the draw of the call with temperature_rows / top_k_rows / top_p_rows holding
 *     (t, k, p) for that sequence: token, probs_out, the logits written back and the logp_out pair.  ONE kernel serves it,
 *     the harmony kernel with the table: cls_ctl requires state, seq (ld_seq >= 1), bias, gram, harm and chord_tok (pass
 *     the zero bias and all-off switch arrays where there is none) and a 16-byte aligned pointer, else -22.  Validating
 *     the records is the caller's job (generate.class_sampling).  The same field, with the same meaning and the same
 *     refusals, ends commu_decode_loop_args.
 * NOTE ORDER (the reference's encoder sorts a bar's notes by start time: training data never steps back inside a bar and
 * never holds one pitch twice at one position; the reference's sampler does not enforce either)
 *   order_ctl: int32 [nseq], one control word per sequence: -1 off, 0 on, n in 1 .. 128 on with at most n notes per
 *     position.  Defined on seq alone when the stage runs: L = min(max(F_LEN, 0), ld_seq), S = seq[b][0:L]; j the largest
 *     index with S[j] == BAR (2) or a POSITION token (432 .. 559) -- none, or BAR: nothing is banned; else p = S[j], s one
 *     past the largest i < j with S[i] BAR or a POSITION token != p (0: none), the run is S[s:L], D the PITCH tokens
 *     (3 .. 130) in it, n their number with multiplicity.  BANNED: ids 432 .. p - 1; every id in D; p itself when
 *     order_ctl[b] >= 1 and n >= order_ctl[b].  A banned id's y is replaced by -inf after the harmony term (a select):
 *     before top-k, never written back, probs_out exactly 0 there, the logp pair's `full` the log-softmax of y, a row
 *     with nothing left gives token -1.  The bans apply whatever class is drawn and whatever gram_on[b] says.  A draw is
 *     BIT FOR BIT the draw of the call without order_ctl and with bias[b] = -inf at the banned ids; an off sequence, or a
 *     draw with nothing banned, is bit for bit the call without the field.  ONE kernel serves it, the class-control
 *     kernel with the scan of seq: order_ctl requires cls_ctl and everything cls_ctl requires, else -22 (a caller
 *     without class controls passes a table whose eight records all hold the sequence's triple).  Validating the words is
 *     the caller's job (generate.note_order_ctl).  The same field, with the same meaning and the same refusal, ends
 *     commu_decode_loop_args.  Null: the launch that never heard of it.
 * VOICE CAP (the reference's token-to-MIDI step turns every Position, Velocity, Pitch, Duration group into a note
 * [start, start + duration); its sampler does not keep notes from overlapping, nor a pitch from being struck while it sounds)
 *   voice_ctl: int32 [nseq], one control word per sequence: -1 off, else N + 256 r with N in 0 .. 128 the cap (0: none)
 *     and r in {0, 1} (1: no re-striking).  Defined on seq alone when the stage runs, with L and S as for order_ctl.  A NOTE
 *     is an index i, i + 3 < L, with S[i], S[i+1], S[i+2], S[i+3] = POSITION (432 .. 559), VELOCITY (131 .. 194), PITCH
 *     (3 .. 130), DURATION (304 .. 431): start a = S[i] - 432, length d = S[i+3] - 303, pitch S[i+2], beta the number of BAR
 *     tokens in S[i+4 : L], end on the current bar's grid e = min(a + d - 128 beta, 128).  Notes with beta >= 2 are ignored
 *     (a + d <= 255: they end before the current bar), so the walk stops at the second BAR from the end.  CAP (N >= 1): E is
 *     the N-th largest e over the notes with beta <= 1, with multiplicity, 0 when there are fewer than N or the value is
 *     <= 0; BANNED: ids 432 .. 432 + E - 1.  RE-STRIKE (r = 1): with j as for order_ctl (none: nothing) and g0 = 0 for BAR,
 *     S[j] - 432 else; BANNED: the pitch id of every note with beta <= 1 and e > g0.  The bans join order_ctl's in the same
 *     select (positions [432, max of the two ends), the pitch sets united), so all that is said there holds: before top-k,
 *     never written back, probs_out exactly 0, `full` the log-softmax of y, token -1 when nothing is left.  A draw is BIT
 *     FOR BIT the draw of the call without voice_ctl and with bias[b] = -inf at these ids; an off word, or one that bans
 *     nothing, is bit for bit the call without the field.  With order_ctl[b] >= 0 every known note starts at or before any
 *     onset that can still be drawn, which is what makes one range enough; voice_ctl itself does not look at order_ctl[b].
 *     ONE kernel serves it, the note-order kernel with the longer walk: voice_ctl requires order_ctl and everything
 *     order_ctl requires, else -22.  Validating the words is the caller's job (generate.voices_ctl).  The same field, with
 *     the same meaning and the same refusal, is in commu_decode_loop_args.  Null: the launch that never heard of it.
 * NOTE DENSITY (the reference's conditioning has no token for how many notes a bar holds; with BAR allowed at every note
 * boundary its sampler closes bars after one note or none and lets others run to dozens)
 *   density_ctl: int32 [nseq], one control word per sequence: -1 off, else lo + 256 hi with lo, hi in 0 .. 255 (0: that
 *     bound is not set; a word with hi >= 1 has hi >= max(lo, 1)).  Defined on seq alone when the stage runs, with L, S, NOTE
 *     and beta as for voice_ctl.  C is the number of notes with beta == 0: the complete POSITION, VELOCITY, PITCH, DURATION
 *     groups behind the last BAR of S, or anywhere in S when it holds no BAR.  UPPER (hi >= 1 and C >= hi); BANNED: every
 *     POSITION id 432 .. 559 -- of the boundary family only BAR and EOS remain.  LOWER (lo >= 1 and C < lo); BANNED: BAR (2)
 *     and EOS (1), UNLESS the position range that order_ctl, voice_ctl and the upper bound ban together already covers all
 *     128 positions (its end is 560): a bar that cannot take another onset can still end.  The bans join order_ctl's and
 *     voice_ctl's in the same select (positions [432, max of the three ends), the two ids selected to -inf likewise), so all
 *     that is said for order_ctl holds: before top-k, never written back, probs_out exactly 0, `full` the log-softmax of y,
 *     token -1 when nothing is left.  A draw is BIT FOR BIT the draw of the call without density_ctl and with bias[b] = -inf
 *     at these ids; an off word, or one that bans nothing, is bit for bit the call without the field.
 *     NOT COVERED: notes inside a prompt count toward C but are never removed; a note that starts on a FORCED position (a
 *     first chord inside its bar, two chords in one bar) counts but cannot be prevented; a bar that ends because the
 *     generation length ran out; forced tokens are never affected (a forced BAR or EOS closes a bar with C < lo).
 *     ONE kernel serves it, the voices kernel with the count on the same walk: density_ctl requires voice_ctl and
 *     everything voice_ctl requires, else -22.  Validating the words is the caller's job (generate.density_ctl).  The same
 *     field, with the same meaning and the same refusal, is in commu_decode_loop_args.  Null: the launch that never heard of
 *     it.
 * MELODIC INTERVAL (the reference's conditioning has no token for the melodic line; even a monophonic line of its sampler
 * jumps anywhere in the 128-pitch range from one note to the next)
 *   interval_ctl: int32 [nseq], one control word per sequence: -1 off, else up + 256 down + 65536 u with up, down in
 *     0 .. 127 (0: that bound is not set) and u in {0, 1} (1: the pitch may not repeat); word 0 is on and bans nothing.
 *     Defined on seq alone when the stage runs, with L, S, NOTE and beta as for voice_ctl.  The REFERENCE NOTE is the note
 *     with beta <= 1 whose index i is largest, q = S[i+2] its PITCH token; none (the first note of a sequence, a line that
 *     rested for a whole bar or more): nothing is banned.  UP (up >= 1); BANNED: ids q + up + 1 .. 130.  DOWN (down >= 1);
 *     BANNED: ids 3 .. q - down - 1.  UNISON (u = 1); BANNED: id q.  One id is one semitone.  The bans join order_ctl's,
 *     voice_ctl's and density_ctl's in the same select, whatever class is drawn and whatever the grammar's switch says, so
 *     all that is said for order_ctl holds: before top-k, never written back, probs_out exactly 0, `full` the log-softmax of
 *     y, token -1 when nothing is left.  A draw is BIT FOR BIT the draw of the call without interval_ctl and with
 *     bias[b] = -inf at these ids; an off word, word 0, or a word that bans nothing is bit for bit the call without the
 *     field.  The word does not imply the note order, the voice cap or the density: those words stay as they are.
 *     NOT COVERED: the first note, and a note after a full bar without one, have no reference; notes inside a prompt are
 *     not checked against each other (the prompt's last note is the reference of the first draw); several notes at one
 *     position are compared in token order, so the rule also limits the spread of a chord of notes; a bias, harmony,
 *     note-order or re-strike ban that leaves no pitch inside the window ends the attempt by Q12, as before; forced tokens
 *     are never affected.
 *     ONE kernel serves it, the density kernel with one more ballot on the same walk: interval_ctl requires density_ctl
 *     and everything density_ctl requires, else -22.  Validating the words is the caller's job (generate.interval_ctl).
 *     The same field, with the same meaning and the same refusal, is in commu_decode_loop_args.  Null: the launch that
 *     never heard of it.
 * ONSET TEMPLATES (the reference's conditioning has one coarse rhythm token; nothing says WHEN a note may start, so two
 * tracks generated from the same metadata share no groove)
 *   onset_ctl: int32 [nseq], one control word per sequence: -1 off, else base + 4096 R with R in 1 .. 64 the cycle length,
 *     base in 0 .. 4095 and base + R <= onset_rows.  onset_table: uint32 [onset_rows][4], 1 <= onset_rows <= 4096; a row is a
 *     128-bit mask over the bar's 128-step grid: bit g % 32 of word g / 32 set means POSITION id 432 + g may be drawn.  With
 *     nb the BAR tokens in S (taken from the forcing record: state[b][8], which the forcing stage keeps equal to that
 *     count), the OPEN BAR is i = max(nb - 1, 0) -- the stretch before the first BAR uses bar 0's row, as density_ctl counts
 *     it -- and its row is base + (i mod R), clamped to onset_rows - 1 whatever the arrays hold.  BANNED: every POSITION id
 *     whose bit is clear.  i counts a prompt's bars too: a primed sequence continues the cycle in phase.  The bans join
 *     order_ctl's, voice_ctl's, density_ctl's and interval_ctl's in the same select, so all that is said for order_ctl
 *     holds; an all-clear row is a bar of rest.  A draw is BIT FOR BIT the draw of the call without onset_ctl and with
 *     bias[b] = -inf at these ids; an off word, or a word over an all-ones row, is bit for bit the call without the field.
 *     DENSITY WAIVER: with onset_ctl given, density_ctl's LOWER bound bans BAR and EOS unless NO position id is left
 *     unbanned by the merged position range TOGETHER WITH the template row (an off word: the all-ones row, i.e. exactly the
 *     rule above).  It is the one place where the template is more than a bias.
 *     NOT COVERED: forced tokens (the position 0 forced after a BAR, a chord's forced position, and so a note that starts
 *     on either); notes inside a prompt; a bar cut by the generation length; a template, bias or harmony that leaves
 *     nothing to draw in a family ends the attempt by Q12, as before.
 *     ONE kernel serves it, the interval kernel with the row's four words loaded beside the grammar row: onset_ctl
 *     requires interval_ctl and everything interval_ctl requires, a non-null onset_table and 1 <= onset_rows <= 4096,
 *     else -22.  Validating the words is the caller's job (generate.onset_ctl).  The same three fields, with the same
 *     meaning and the same refusals, are in commu_decode_loop_args.  Null onset_ctl: the launch that never heard of it.
 * GUIDE TRACK (an arrangement is built by combining tracks generated separately from shared metadata, and no other rule
 * reads another track's notes: harmony knows the chord symbol, an onset template from a track shares its rhythm, and for
 * PITCH there was nothing)
 *   guide_ctl: int32 [nseq], one control word per sequence: -1 off, else base + 65536 R + 2^23 s with R in 1 .. 64 the
 *     template's bars, s in 0 .. 7 and C = 128 >> s the cells per bar, base in 0 .. 65535, base + R (1 + C) <= guide_rows.
 *     guide_table: uint32 [guide_rows][4], 1 <= guide_rows <= 65536.  Each bar of a template is a block of 1 + C consecutive
 *     rows: row 0 the bar's LIVE ROW, a 128-bit mask over POSITIONS in onset_table's format (bit g set: a note may start at
 *     step g); rows 1 .. C the CELL ROWS, 128-bit masks over PITCHES (bit k % 32 of word k / 32 set: PITCH id 3 + k may be
 *     drawn).  BLOCK OF THE OPEN BAR, as for onset_ctl: i = max(nb - 1, 0) with nb = state[b][8], never counted on a draw,
 *     a prompt's bars included; the block starts at base + (i mod R) (1 + C).
 *     PITCH BAN: j and p are order_ctl's (j the largest index with S[j] BAR or a POSITION).  No such j, or S[j] BAR: no
 *     pitch is banned.  Else g = p - 432, the cell row is block + 1 + (g >> s), and every PITCH id whose bit is clear is
 *     banned.  Ids outside 3 .. 130 are never touched.
 *     POSITION BAN: every POSITION id whose bit in the live row is clear is banned.  The live row is ANDed into the onset
 *     row before that is used, so onset_ctl's position ban AND ITS DENSITY WAIVER apply to the intersection: the waiver lets
 *     a bar end once position range, onset row and live row together leave no position.
 *     The bans join the one select of order_ctl, voice_ctl, density_ctl, interval_ctl and onset_ctl.  A draw is BIT FOR BIT
 *     the draw of the call without guide_ctl and with bias[b] = -inf at these ids (density_ctl's BAR / EOS ban taken under the
 *     waiver on the ANDed row); an off word, or a word over an all-ones live row with all-ones cell rows, is bit for bit the
 *     call without the fields.  Every row index is clamped to guide_rows - 1, whatever the arrays hold.
 *     NOT COVERED: only a note's START is tested -- a drawn note held across a later change of the guide is not checked;
 *     forced tokens (the position 0 forced after a BAR, a chord's forced position); notes inside a prompt; a pitch range,
 *     strict harmony or interval window that together with the cell row leaves no pitch ends the attempt by Q12, as before.
 *     ONE kernel serves it, the onsets kernel with two more scalar 16-byte loads (the live row beside the onset row, the
 *     cell row once the scan has found p): guide_ctl requires onset_ctl and everything onset_ctl requires, a non-null
 *     guide_table and 1 <= guide_rows <= 65536, else -22.  Validating the words is the caller's job (generate.guide_rows /
 *     ForcedDecoder.set_guide).  The same three fields, with the same meaning and the same refusals, are in
 *     commu_decode_loop_args.  Null guide_ctl: the launch that never heard of it.
 *     With art_ctl's h switch (below) a note's held steps are tested against the guide as well.
 * ARTICULATION (a note is the group Position, Velocity, Pitch, Duration; the rules above decide when it starts and which
 * pitch it takes, this one how long it lasts and how loud it is)
 *   art_ctl: int32 [nseq], one control word per sequence: -1 off, else base + 4096 R + 2^19 w + 2^20 h with R in 1 .. 64
 *     the template's bars, base in 0 .. 4095, base + R <= art_rows, w the bar-line switch, h the guide-hold switch.
 *     art_table: uint32 [art_rows][4], 1 <= art_rows <= 4096.  One row is one bar of a template: word 0 is dlo | dhi << 8,
 *     each 0 .. 128 (0: that bound is not set); words 1 and 2 are a 64-bit velocity mask (bit k % 32 of word 1 + k / 32
 *     set: VELOCITY id 131 + k, MIDI velocity 2 k, may be drawn); word 3 is reserved: write 0, it is never read.
 *     ROW OF THE OPEN BAR, as for onset_ctl: i = max(nb - 1, 0) with nb = state[b][8], never counted on a draw, a prompt's
 *     bars included; the row is base + (i mod R), clamped to art_rows - 1 whatever the arrays hold.
 *     VELOCITY BAN: every VELOCITY id 131 .. 194 whose bit is clear is banned.  Ids 130 and 195 are never touched.
 *     DURATION WINDOW (DURATION id 303 + d lasts d steps, 1 .. 128): j and p are order_ctl's; a = p - 432 exists when S[j]
 *     is a POSITION; q = S[L - 1] is the grammar's previous token and k = q - 3 exists when q is a PITCH.  cap = 128,
 *     lowered by each that applies: dhi >= 1: min(cap, dhi); w set and a exists: min(cap, 128 - a), the note ends by the bar
 *     line; h set, guide_ctl[b] on, a and k exist: min(cap, f), f the smallest m in 1 .. 127 such that bit k of the guide's
 *     cell row for step a + m is clear (none: the term does not apply).  The cell row of step a + m < 128 is
 *     block_i + 1 + ((a + m) >> s), of a later step block_{i+1} + 1 + ((a + m - 128) >> s), block_x = base_g +
 *     (x mod R_g) (1 + C) with guide_ctl[b]'s own base_g, R_g, s and C; every row index is clamped to guide_rows - 1.
 *     lo = min(max(dlo, 1), cap); banned are DURATION ids 304 .. 303 + lo - 1 and 304 + cap .. 431.  The window is never
 *     empty (a <= 127, f >= 1): where the bar line or the guide leaves less room than dlo the lower bound gives way.  Ids
 *     303 and 432 are never touched; step a itself is not tested (that is guide_ctl's pitch ban).
 *     The bans apply whatever class is drawn and join the one select of order_ctl .. guide_ctl.  A draw is BIT FOR BIT the
 *     draw of the call without art_ctl and with bias[b] = -inf at these ids; an off word, or a word over a row with
 *     dlo = dhi = 0, an all-ones velocity mask and w = h = 0, is bit for bit the call without the fields.
 *     NOT COVERED: forced tokens, and anything a forced position starts; notes inside a prompt; a note forced shorter than
 *     dlo (above); an empty velocity mask ends the attempt by Q12 as before (the host refuses to build one); the hold term
 *     reads the next bar's block even where the generation length would cut the sequence first; the hold term tests the
 *     guide only (harmony across a chord change is not tested).
 *     ONE kernel serves it, the guide kernel with one more uniform 16-byte load (the row, beside the onset row) and two
 *     one-word loads per lane for the hold term (lane l tests steps a + 1 + l and a + 65 + l; issued with the guide's cell
 *     row, once the scan has found p; two ballots give f).  A host-precomputed run-length table by bar, cell and pitch
 *     would make f one load; it costs 1 MB per 64-bar template and a repack on every change of the guide, and was not
 *     built.  art_ctl requires guide_ctl and everything guide_ctl requires -- callers without a guide pass all -1 guide
 *     words over a one-row table -- a non-null art_table and 1 <= art_rows <= 4096, else -22.  Validating the words is the
 *     caller's job (generate.articulation_rows / ForcedDecoder.set_articulation).  The same three fields, with the same
 *     meaning and the same refusals, are in commu_decode_loop_args.  Null art_ctl: the launch that never heard of it.
 * WHAT gram / harm READ
 *   state: the forcing records, int32 [nseq][commu_forcing_state_ints()]; seq int32 [nseq][ld_seq]; chord_tok int32
 *   [nseq][ld_chord].  Not looked at, and may be null, in a call without gram and harm.
 * REQUIRED POINTERS: logits and token must be valid, readable device arrays -- token [nseq] always receives the result,
 * and the kernel issues every optional load unconditionally: where `active`, a control array or a switch array is null it
 * reads token[b] or logits[b][0] instead and ignores the value, so that these loads share one memory round trip with the
 * logits.  nseq <= 0: nothing is launched, 0. */
typedef struct commu_sample_args {
    unsigned struct_bytes;
    /* what is drawn from */
    float* logits;
    const unsigned char* wrong;
    const float* uniforms;
    const unsigned char* active;
    int ld, nseq, V, ldw;
    /* controls */
    const float* temperature_rows;
    const int* top_k_rows;
    const float* top_p_rows;
    float temperature;
    int top_k;
    float top_p;
    /* results */
    int* token;
    float* probs_out;
    float* logp_out;
    int ldp;
    /* constraints */
    const float* bias;
    const float* gram;
    const unsigned char* gram_on;
    const float* harm;
    const unsigned char* harm_on;
    int ld_bias, ld_gram, ld_harm;
    /* what gram / harm read */
    const int* state;
    const int* seq;
    const int* chord_tok;
    int ld_seq, ld_chord;
    /* articulation (ahead of guide_ctl: the eleven fields behind them keep their places at the struct's end) */
    const int* art_ctl;
    const unsigned* art_table;
    int art_rows;
    /* guide track (ahead of onset_ctl: the eight fields behind them keep their places at the struct's end) */
    const int* guide_ctl;
    const unsigned* guide_table;
    int guide_rows;
    /* onset templates (ahead of interval_ctl: the five fields behind them keep their places at the struct's end) */
    const int* onset_ctl;
    const unsigned* onset_table;
    int onset_rows;
    /* melodic interval (ahead of density_ctl: the four fields behind it keep their places at the struct's end) */
    const int* interval_ctl;
    /* note density (ahead of order_ctl: the three fields behind it keep their places at the struct's end) */
    const int* density_ctl;
    /* note order (placed ahead of cls_ctl, which stays the struct's last field) */
    const int* order_ctl;
    /* voice cap (likewise ahead of cls_ctl) */
    const int* voice_ctl;
    /* class-keyed controls */
    const void* cls_ctl;
} commu_sample_args;
int commu_sample_args_bytes(void);
int commu_sample_topk(const commu_sample_args* a, hipStream_t stream);

/* ---- single-token decode step with a K/V cache (forward_generate with qlen 1, model.py:606-628, as
 * called by midi_inferrer.py:199-207).  Caches are bf16 [B][H][Lmax][DH] per layer; klen[b] = valid rows
 * of sequence b (ragged); the new token sits at row klen[b] and attends rows 0..klen[b]. */
int commu_decode_kv_append(const void* qkv, int ld_qkv, void* kcache, void* vcache, const int* klen,
                           const unsigned char* active, int B, int Lmax, int H, int HD, hipStream_t stream);
/* out[b, h*DH:(h+1)*DH] = softmax_j(((q+u).k_j + (q+v).Rd[klen[b]-j]) * scale) . v_j   (rd: [>= Lmax][ld_rd]) */
/* append != 0: the kernel first writes the new token's K and V (from qkv) to cache row klen[b] itself
 * (commu_decode_kv_append fused in; the caches are then written through kcache / vcache) */
int commu_decode_attn(const void* qkv, int ld_qkv, void* kcache, void* vcache, const void* rd,
                      int ld_rd, const float* r_w_bias, const float* r_r_bias, const int* klen,
                      const unsigned char* active, void* out, int ld_o, int B, int H, int DH, int Lmax,
                      float scale, int append, hipStream_t stream);
/* The same with the keys of a (sequence, head) pair split over up to nsplit (<= 16) workgroups of >= 512 keys each -- for
 * long memories with few live sequences, where one workgroup per pair streams its ~1 MB alone.  split_ws: B * H * nsplit *
 * (DH + 2) floats of scratch; split_cnt: B * H words, ZERO before the first call (the kernel leaves them zero).  Pairs
 * with at most 512 keys take the unsplit path inside the same launch. */
int commu_decode_attn_split(const void* qkv, int ld_qkv, void* kcache, void* vcache, const void* rd, int ld_rd,
                            const float* r_w_bias, const float* r_r_bias, const int* klen, const unsigned char* active,
                            void* out, int ld_o, int B, int H, int DH, int Lmax, float scale, int append, int nsplit,
                            float* split_ws, unsigned* split_cnt, hipStream_t stream);
/* klen[b] += advance[b]  (a step whose memory the reference discards does not advance: quirk Q3) */
int commu_decode_advance(int* klen, const unsigned char* advance, int B, int Lmax, hipStream_t stream);
/* ---- the same step with the reference's SLIDING memory (forward_generate keeps the last mem_len hidden states per layer,
 * commu/model/model.py:507-538; with same_length the oldest key is hidden once the memory is full, model.py:549-568 at
 * qlen 1, mlen = mem_len).  The cache of a (sequence, head) pair is a RING of W = mem_len + 1 rows ([B][H][W][DH],
 * 2 <= W <= 4224); klen[b] counts the ABSOLUTE positions kept so far and is not bounded by W (pass a large Lmax to
 * commu_decode_advance / commu_forcing_post / commu_decode_sample_post_pre); position p lives in row p mod W.  The new
 * token (row klen[b] mod W) attends the min(klen[b] + 1, W) rows written so far, row j at distance (klen[b] - j) mod W
 * (rd: [>= W][ld_rd]); same_length != 0 and klen[b] >= W - 1: the row at distance W - 1 is hidden.  No row is ever moved:
 * a step reads each live row once and writes one.
 * commu_decode_attn_ring: nsplit = 1 is the unsplit kernel (split_ws / split_cnt may be null), nsplit > 1 as
 * commu_decode_attn_split. */
int commu_decode_kv_append_ring(const void* qkv, int ld_qkv, void* kcache, void* vcache, const int* klen,
                                const unsigned char* active, int B, int W, int H, int HD, hipStream_t stream);
int commu_decode_attn_ring(const void* qkv, int ld_qkv, void* kcache, void* vcache, const void* rd, int ld_rd,
                           const float* r_w_bias, const float* r_r_bias, const int* klen, const unsigned char* active,
                           void* out, int ld_o, int B, int H, int DH, int W, float scale, int append, int same_length,
                           int nsplit, float* split_ws, unsigned* split_cnt, hipStream_t stream);
/* The cached decode step over an fp8 K/V cache (csrc/decode_kv8.hip; opt-in, no parity claim).  Per layer:
 *   kc8 / vc8: uint8 [B][H][Lmax][DH], OCP e4m3 bytes, head-major like the bf16 caches;
 *   ks / vs:   uint8 [B][H][Lmax][DH/32], one E8M0 byte per 32 consecutive features of a row: scale 2^(byte - 127).
 * The quantiser is commu_quant_mxfp8's: sb = clamp(biased exponent of the block's amax - 8, 0, 254); the elements are
 * multiplied by 2^(127 - sb), clamped to +-448 and rounded to nearest even.  DH 64 or 32.
 * RULE: a position has one K and one V, whatever step reads it -- the step that appends a token attends to the
 * quantise -> dequantise image of its K and V, so every step computes the attention of commu_decode_attn /
 * commu_decode_attn_ring over the DEQUANTISED cache as it stands after the append.
 * commu_decode_attn_kv8: one entry point for the linear cache (ring 0; mask_oldest ignored) and the ring of Lmax = W rows
 * (ring 1; mask_oldest = the model's same_length), unsplit (nsplit 1; split_ws / split_cnt may be null) or split-key as
 * commu_decode_attn_split.  append 1 also writes the new token's bytes and scale bytes to its row.  qkv, rd, out: bf16.
 * commu_decode_prefill_scatter_kv8: commu_decode_prefill_scatter with the quantiser on the way (one launch per layer). */
int commu_decode_attn_kv8(const void* qkv, int ld_qkv, void* kc8, void* vc8, void* ks, void* vs, const void* rd, int ld_rd,
                          const float* r_w_bias, const float* r_r_bias, const int* klen, const unsigned char* active,
                          void* out, int ld_o, int B, int H, int DH, int Lmax, float scale, int append, int ring,
                          int mask_oldest, int nsplit, float* split_ws, unsigned* split_cnt, hipStream_t stream);
int commu_decode_prefill_scatter_kv8(const void* qkv, int ld_qkv, int T, int B, void* kc8, void* vc8, void* ks, void* vs,
                                     int* klen, const int* len, const int* slot, int Bcache, int H, int DH, int Lmax,
                                     int window, hipStream_t stream);
/* The cached decode attention with a SHARED PROMPT PREFIX (csrc/decode_prefix.hip; opt-in, bf16 linear cache only).
 *   pk / pv:    bf16 [H][Pcap][DH], the K / V of the positions every slot has in common, held once; *prefix_len = P of
 *               them are valid (a device word the kernel reads: nothing of P is baked into a launch);
 *   kc / vc:    bf16 [B][H][Lp][DH], the private rows: row r of slot b is absolute position P + r; klen[b] counts
 *               private rows only, the new token is appended to private row klen[b] (append 1);
 *   rd:         the distance table, at least Pcap + Lp rows (Pcap + Lp <= 4224).
 * An active pair (b, h) attends to prefix rows 0 .. P-1 of head h and private rows 0 .. klen[b] of (b, h), the key of
 * absolute position p at distance P + klen[b] - p: commu_decode_attn over a cache that holds the prefix in every slot.
 * ws: fp32 [B H (nsplit + ceil(Pcap / chunk)) (DH + 2)] records, cnt: [B H] arrival counters, ZERO on entry (the launch
 * leaves them zero); nsplit 1 .. 16 splits the private keys as commu_decode_attn_split does.  Rows of inactive slots are
 * not written.  DH 64 or 32.  commu_decode_prefix_chunk / _group: prefix rows per chunk, slots per prefix workgroup. */
int commu_decode_prefix_chunk(void);
int commu_decode_prefix_group(void);
int commu_decode_attn_prefix(const void* qkv, int ld_qkv, const void* pk, const void* pv, const int* prefix_len, int Pcap,
                             void* kcache, void* vcache, const void* rd, int ld_rd, const float* r_w_bias,
                             const float* r_r_bias, const int* klen, const unsigned char* active, void* out, int ld_o,
                             int B, int H, int DH, int Lp, float scale, int append, int nsplit, float* ws, unsigned* cnt,
                             hipStream_t stream);
/* Everything of a decode-step layer that follows its attention, as ONE launch (csrc/decode_tail.hip):
 *   z1 = vec . Wo^T + h;  a = LN1(z1);  hid = relu(a . W1^T + b1);  z2 = hid . W2^T + b2 + a;  h_out = LN2(z2)
 *   (o_net + residual + LayerNorm model.py:344-352, PositionwiseFF model.py:163-179)
 * and then out_n = h_out . Wn^T: the NEXT layer's qkv_net (logits == 0: Nn = 3 HD, bf16, model.py:297-299) or the
 * tied-embedding logits (logits != 0: + bn, fp32, columns < Nn, model.py:64-73; rows with active[row] == 0 are not
 * written -- active may be null).  The logits launch takes 512 < Nn <= 1024 only (others: -22): its kernels walk two
 * column tiles per workgroup, and the packed copy of a weight with Nn <= 512 rows has one.  vec [B][HD], h / h_out [B][D] bf16;
 * z1 / z2 [B][D] and hid [B][DI] are dense bf16 hand-off buffers that belong to THIS layer; sync:
 * commu_decode_tail_sync_words_for(B) words that must be ZERO on entry (one set per launch of a step): the arrival counter
 * of phase p and row group mg (16 sequences) is word (p G + mg) 64 with G = 4 for B <= 64 and 16 beyond; the launch leaves
 * 32 in the counters of the row groups in use and touches no other word.  commu_decode_tail_sync_words() is the B <= 64
 * value (768).  *err becomes non-zero when a workgroup gave up waiting (the results of that launch are then invalid).
 * commu_decode_tail_supported(B, D, DI, HD) names the shapes this build takes -- (512, 1024, 8 or 10 heads x 64) and the
 * wide (1024, 2048, 16 x 64), 1 .. 256 sequences -- (others: -22; callers use the per-Linear launches).  256 is what
 * stays resident at once: 32 workgroups per 16 sequences, 2 workgroups per CU, 256 CUs (csrc/decode_tail.hip has the
 * derivation).  d_ln: LayerNorm width (<= D; zero-padded models). */
int commu_decode_tail_supported(int B, int D, int DI, int HD);
/* diagnostics: following layer-tail / head launches of up to 64 sequences write 100 MHz timestamps of their phase
 * boundaries to buf[workgroup][16] (device memory, 128 x 16 words; null: off) */
int commu_decode_tail_trace(unsigned long long* buf);
int commu_decode_tail_sync_words(void);
int commu_decode_tail_sync_words_for(int B);
int commu_decode_layer_tail(const void* vec, int ld_vec, const void* h, int ld_h, const void* Wo_packed,
                            const void* W1_packed, const float* b1, const void* W2_packed, const float* b2,
                            const float* g1, const float* be1, float eps1, const float* g2, const float* be2, float eps2,
                            int d_ln, const void* Wn_packed, int Nn, const float* bn, int logits,
                            const unsigned char* active, void* z1, void* hid, void* z2, void* h_out, int ld_ho,
                            void* out_n, int ld_on, int B, int D, int DI, int HD, unsigned* sync, unsigned* err,
                            hipStream_t stream);
/* The four weights of a layer tail (and the head's) are read from PACKED copies: the fragments of one workgroup and
 * wave are consecutive, so every wave instruction reads 1 KB of consecutive bytes.  commu_decode_tail_pack writes the
 * packed copy of a bf16 [N][K] weight (row stride ldw, K % 128 == 0; rows >= N of the last tiles are zero) into `out`
 * (commu_decode_tail_pack_bytes(N, K) bytes); it must be repeated whenever the weight changes. */
long long commu_decode_tail_pack_bytes(int N, int K);
int commu_decode_tail_pack(const void* W, int ldw, int N, int K, void* out, hipStream_t stream);
/* First launch of a decode step on the same workgroup layout: h_out = E[tok] * scale (word embedding, model.py:409-420;
 * fp32 table [V][d_true], ids outside [0, V) give NaN rows) and qkv = h_out . Wqkv^T (layer 0's qkv_net); also clears
 * zero_words[0 .. n_zero) -- the arrival counters of the step's commu_decode_layer_tail launches. */
int commu_decode_head(const int64_t* tok, const float* E, int d_true, int V, float scale, const void* Wqkv_packed,
                      void* h_out, int ld_ho, void* qkv, int ld_qkv, int B, int D, int DI, int HD,
                      unsigned* zero_words, int n_zero, hipStream_t stream);

/* ---- device-resident chord / bar forcing of the decode loop (InferenceTask.generate_sequence +
 * TeacherForceTask, commu/midi_generator/midi_inferrer.py:239-320, :16-144): per-sequence state records of
 * commu_forcing_state_ints() int32 each, fields in this order:
 *   len, forced (-1: none), redo, first, filled, done, failed, iters, nbar, nchord, cur, length_fit, ndraw, ntrace.
 * seq: int32 [B][ld_seq] token buffers; chord_tok / chord_pos: int32 [B][ld_chord] (the progression to force);
 * wrong: uint8 [B][729] rejected-chord bitmap; utable: fp32 [B][ld_u] uniform variates, one per draw.
 * commu_forcing_pre decides this iteration's model step and draw: tok (int64 [B]: token fed), active (step?),
 * keep (does the step's memory stay? quirk Q3), draw (is a token drawn?), uni (its variate); trace (optional,
 * int32 [B][ld_trace]) records (token, keep) of every model step.  commu_forcing_post applies the drawn token
 * (token[b] < 0: nothing could be drawn, Q12).  live (optional): += number of unfinished sequences. */
int commu_forcing_state_ints(void);
/* seq_logp (optional, fp32 [B][ld_seq][2], parallel to seq: the log-probability pair of every token, see
 * commu_sample_args.logp_out): a FORCED token appended here (midi_inferrer.py:247-251) was not drawn and gets NaN, NaN;
 * null: no pairs are kept */
int commu_forcing_pre(int* state, int* seq, int ld_seq, const int* chord_tok, const int* chord_pos, int ld_chord,
                      unsigned char* wrong, const float* utable, int ld_u, int max_iters, long long* tok,
                      unsigned char* active, unsigned char* keep, unsigned char* draw, float* uni, int* trace,
                      int ld_trace, float* seq_logp, int B, hipStream_t stream);
/* klen / keep (optional): the cache lengths of the decode step advance here (klen[b] += keep[b], capped at lmax - 1),
 * which saves the separate commu_decode_advance launch.
 * logp / seq_logp (optional): where the drawn token is appended (midi_inferrer.py:313-317) its pair logp[b][0:2] (fp32
 * [B][2], what commu_sample_topk wrote beside token) is stored at the token's index; a draw that is not appended --
 * rejected chord, position past a pending chord, replaced EOS / bar (:294-311), Q12 -- leaves no entry.  Null: no pairs
 * are kept. */
int commu_forcing_post(int* state, int* seq, int ld_seq, const int* chord_pos, int ld_chord, unsigned char* wrong,
                       const unsigned char* draw, const int* token, int* live, int* klen, const unsigned char* keep,
                       int lmax, const float* logp, float* seq_logp, int B, hipStream_t stream);
/* ---- FORM templates: a bar the loop opens may replay an earlier bar of its own sequence (csrc/decode_loop.h: Form).
 *   form_ctl: int32 [B], one control word per sequence: -1 off, else base + 4096 R with R in 1 .. 64 the form's bars and
 *     base in 0 .. 4095, base + R <= form_rows.  form_table: uint32 [form_rows][4], 1 <= form_rows <= 4096; row base + i is
 *     bar i of the form (bars from R on, and from the 64th on, are free: a form is not cycled).  Word 0 is
 *     src | copy << 6 | (transpose + 64) << 8 with src in 0 .. 63 the bar replayed (src < i, else the row is free), copy 0
 *     (all four tokens of a note) or 1 (rhythm: the pitch is drawn), transpose in -48 .. 48 semitones (0 with rhythm); the
 *     word 0 is a free bar.  Words 1 .. 3 are reserved, written 0 and never read.
 *   form_state: int32 [B][commu_form_state_ints()]: active, cursor, end, k (the phase 0 .. 3 inside the current note group),
 *     the open bar's row word, g (the group the last search found, -1: none), two reserved ints, then bar_at[0 .. 63], the
 *     index in seq of the (i+1)-th BAR token (context and prompt included).  commu_form_reset writes the state a load leaves;
 *     the arm launches write it for the slots they arm.
 *   form_tok: int32 [B]: the replay token commu_forcing_pre_form decided on (-1: none), read by commu_forcing_post_form.
 * THE RULE, on a note group = four consecutive tokens POSITION (432 .. 559), VELOCITY (131 .. 194), PITCH (3 .. 130),
 * DURATION (304 .. 431), with bar i the stretch bar_at[i] < index < bar_at[i + 1]:
 *   a BAR is appended (forced in pre or drawn in post): bar_at takes its index while fewer than 64 are recorded; the new
 *     open bar i = F_NBAR - 1 with a replay row of src j gets active = 1, cursor = bar_at[j] + 1, end = bar_at[j + 1], k = 0,
 *     any other bar active = 0;
 *   pre reaches its "draw" decision with active set: g is the smallest index >= cursor with g + 3 < end whose four tokens
 *     are a note group (none: the replay token is BAR); in rhythm mode at k = 2 a normal draw is made; otherwise the replay
 *     token is seq[g + k], at k = 2 transposed (the MIDI pitch folded by 12 into 0 .. 127).  A replay token consumes no
 *     variate (F_NDRAW does not move) and leaves draw[b] = 0, so the sampling stage skips the slot and its logits are not
 *     divided; the model step runs as for a draw;
 *   post with form_tok[b] >= 0 treats it exactly as a drawn token (every branch applies); appended and not BAR: k += 1, and
 *     at k = 4 cursor = g + 4, k = 0; not appended: nothing moves and it is offered again; its log-probability pair is NaN;
 *   pre forces a chord while k = 1 (the replayed position was the pending chord's): k = 0, the group starts over;
 *   a pitch drawn in rhythm mode goes through post as any draw; appended: k += 1.
 * Not covered: replayed tokens are not checked against any constraint (forced tokens are not either); a replay bar cut by
 * max_iters or ld_seq is not completed; bars past the 64th are free; a source note the bar line cut does not appear; chord
 * tokens are never copied.
 * commu_forcing_pre_form / commu_forcing_post_form: commu_forcing_pre / commu_forcing_post (same leading arguments, same
 * refusals) with the rule; -22 for a null form_ctl, form_table, form_state or form_tok and for form_rows outside 1 .. 4096.
 * In commu_decode_loop_args a null form_ctl launches the kernels that never heard of the rule; a form_ctl without table,
 * state or form_tok, or with form_rows outside 1 .. 4096, is refused with -22.
 * TAKES: a bar may also replay a bar of a finished sequence the caller supplies.  form_src: const int32 [form_src_len], the
 *   tokens of every take the caller knows, one behind the other.  A row with bit 7 of word 0 set is a TAKE ROW: word 0 is
 *   src | copy << 6 | 1 << 7 | (transpose + 64) << 8 (src: the take's bar, kept for the checker, not used by the kernels),
 *   word 1 `begin`, the index in form_src of the first token behind the source bar's BAR, word 2 `end` (exclusive), the index
 *   of the take's next BAR or of the take's end; word 3 stays reserved and is never read.  Rows without bit 7 mean what they
 *   always meant and their words 1 .. 3 are still never read.  When a BAR opens a take row's bar it is a replay bar whatever
 *   its index (bar 0 included: src < i belongs to own-past rows) with cursor = clamp(begin, 0, form_src_len), end =
 *   clamp(end, cursor, form_src_len); the search and the replay token read form_src (indices clamped to form_src_len - 1)
 *   instead of seq, and nothing else differs: k, g, cursor = g + 4, the chord hand-over, rhythm mode, the transposition.
 *   A take row is FREE where form_src is null, form_src_len < 4 or begin >= end -- so through commu_forcing_pre_form /
 *   commu_forcing_post_form, which pass no buffer, every take row is free.
 *   commu_forcing_pre_form_src / commu_forcing_post_form_src: the two stages with the buffer (post opens bars too); a null
 *   form_src is legal, a form_src with form_src_len < 1 is refused with -22.  In commu_decode_loop_args form_src with
 *   form_src_len < 1, or without form_ctl, is refused with -22 before anything is launched.  The arm launches do not know the
 *   buffer: they reset the slot's state, and a take's tokens are the caller's to place before the rows that name them.
 *   commu_form_src_max(): the ints the decoder's buffer holds, 1 << 18 (64 takes of 4096 tokens).
 *   Not covered, beside the above: a take made under another chord progression still gets this sequence's chords (chord
 *   tokens are never copied); generation is left to right, so a bar drawn between kept bars knows only those before it. */
int commu_form_state_ints(void);
int commu_form_src_max(void);
int commu_forcing_pre_form_src(int* state, int* seq, int ld_seq, const int* chord_tok, const int* chord_pos, int ld_chord,
                               unsigned char* wrong, const float* utable, int ld_u, int max_iters, long long* tok,
                               unsigned char* active, unsigned char* keep, unsigned char* draw, float* uni, int* trace,
                               int ld_trace, float* seq_logp, const int* form_ctl, const unsigned* form_table, int form_rows,
                               int* form_state, int* form_tok, const int* form_src, int form_src_len, int B,
                               hipStream_t stream);
int commu_forcing_post_form_src(int* state, int* seq, int ld_seq, const int* chord_pos, int ld_chord, unsigned char* wrong,
                                const unsigned char* draw, const int* token, int* live, int* klen,
                                const unsigned char* keep, int lmax, const float* logp, float* seq_logp, const int* form_ctl,
                                const unsigned* form_table, int form_rows, int* form_state, int* form_tok,
                                const int* form_src, int form_src_len, int B, hipStream_t stream);
int commu_forcing_pre_form(int* state, int* seq, int ld_seq, const int* chord_tok, const int* chord_pos, int ld_chord,
                           unsigned char* wrong, const float* utable, int ld_u, int max_iters, long long* tok,
                           unsigned char* active, unsigned char* keep, unsigned char* draw, float* uni, int* trace,
                           int ld_trace, float* seq_logp, const int* form_ctl, const unsigned* form_table, int form_rows,
                           int* form_state, int* form_tok, int B, hipStream_t stream);
int commu_forcing_post_form(int* state, int* seq, int ld_seq, const int* chord_pos, int ld_chord, unsigned char* wrong,
                            const unsigned char* draw, const int* token, int* live, int* klen, const unsigned char* keep,
                            int lmax, const float* logp, float* seq_logp, const int* form_ctl, const unsigned* form_table,
                            int form_rows, int* form_state, int* form_tok, int B, hipStream_t stream);
/* form_state[b] and form_tok[b] of the slots first .. first + n - 1 as a load leaves them: nothing replayed, form_tok -1,
 * bar_at over seq[b][0 .. state[b][0]) (the record's length word, clamped to ld_seq).  One wave per slot. */
int commu_form_reset(int* form_state, int* form_tok, const int* state, const int* seq, int ld_seq, int first, int n,
                     hipStream_t stream);
/* diagnostics: following commu_decode_sample_post_pre launches write 100 MHz timestamps buf[sequence][4] = kernel start,
 * after the sampling step, after post, after pre (device memory; null: off) */
int commu_decode_loop_trace(unsigned long long* buf);
/* The three per-sequence stages that follow the model step as ONE launch (generate_sequence, midi_inferrer.py:239-320,
 * one iteration), in this order and with the meaning of the separate entry points:
 *   commu_sample_topk (active = draw, uniforms = uni, ldw = 729, nseq = B) -> commu_forcing_post (live = null) ->
 *   commu_forcing_pre (the decision of the NEXT iteration).
 * The fields are those arguments under their names there; what differs:
 *   struct_bytes: sizeof(commu_decode_loop_args) as the caller compiled it; a value that differs from the library's
 *     (commu_decode_loop_args_bytes()) is refused with -22 before anything else is looked at.
 *   V must be 729 (wrong is uint8 [B][729]); ld_seq >= 2, ld_chord >= 1, ld_u >= 1 (else -22).
 *   logp (optional): the pair of the draw reaches the book-keeping stage in registers; logp[b] is written as well when
 *     given.  seq_logp optional, as in the separate stages.
 *   klen / lmax: as commu_forcing_post (a sliding memory passes a large lmax).
 *   bias / gram / gram_on / harm / harm_on: the constraints of commu_sample_args with the same order, the same off rows
 *     7 and 110, the same "nothing but x is written back" and the same kernel selection: a null pointer launches the
 *     kernel that never heard of the constraint (instructions and argument block); harm requires bias and gram (pass a
 *     zero bias and gram_on zeros where there is none), else -22; ld_bias / ld_gram < 729 or ld_harm < 12: -22; a null
 *     switch array: every sequence is on.  The grammar's previous token and the harmony's chord chord_tok[b][F_CUR - 1]
 *     are read through the record the launch holds anyway; the sampling stage issues those two loads right behind its
 *     logits loads.  gram and harm need state and seq, harm chord_tok (else -22).  Forced tokens (midi_inferrer.py:239-320)
 *     and prompts are not draws: not affected, not checked; the rejected-token map stays the forcing rules' own.
 * REQUIRED POINTERS beside those of the stages: token, state, draw and keep (read at the top of the launch, under the
 * sampling stage, and handed to the book-keeping stage in registers; a null klen reads token[b] instead, a null switch
 * array draw[b]).  B <= 0: nothing is launched, 0. */
typedef struct commu_decode_loop_args {
    unsigned struct_bytes;
    /* what is drawn from */
    float* logits;
    unsigned char* wrong;
    int ld, V, B;
    /* controls */
    const float* temperature_rows;
    const int* top_k_rows;
    const float* top_p_rows;
    float temperature;
    int top_k;
    float top_p;
    /* results */
    int* token;
    float* probs_out;
    float* logp;
    float* seq_logp;
    int ldp;
    /* the forcing records and what the rules read */
    int* state;
    int* seq;
    const int* chord_tok;
    const int* chord_pos;
    const float* utable;
    int ld_seq, ld_chord, ld_u, max_iters;
    /* the decision of the next iteration */
    long long* tok;
    unsigned char* active;
    unsigned char* keep;
    unsigned char* draw;
    float* uni;
    int* trace;
    int ld_trace;
    /* cache lengths */
    int* klen;
    int lmax;
    /* constraints */
    const float* bias;
    const float* gram;
    const unsigned char* gram_on;
    const float* harm;
    const unsigned char* harm_on;
    int ld_bias, ld_gram, ld_harm;
    /* the form's take buffer (below: FORM, take rows; optional; likewise ahead of form_ctl) */
    const int* form_src;
    int form_src_len;
    /* form templates (below: FORM; likewise ahead of art_ctl) */
    const int* form_ctl;
    const unsigned* form_table;
    int form_rows;
    int* form_state;
    int* form_tok;
    /* articulation (commu_sample_args.art_ctl / art_table / art_rows; likewise ahead of guide_ctl) */
    const int* art_ctl;
    const unsigned* art_table;
    int art_rows;
    /* guide track (commu_sample_args.guide_ctl / guide_table / guide_rows; likewise ahead of onset_ctl) */
    const int* guide_ctl;
    const unsigned* guide_table;
    int guide_rows;
    /* onset templates (commu_sample_args.onset_ctl / onset_table / onset_rows; likewise ahead of interval_ctl) */
    const int* onset_ctl;
    const unsigned* onset_table;
    int onset_rows;
    /* melodic interval (commu_sample_args.interval_ctl; likewise ahead of density_ctl) */
    const int* interval_ctl;
    /* note density (commu_sample_args.density_ctl; likewise ahead of order_ctl) */
    const int* density_ctl;
    /* note order (commu_sample_args.order_ctl; likewise ahead of cls_ctl) */
    const int* order_ctl;
    /* voice cap (commu_sample_args.voice_ctl; likewise ahead of cls_ctl) */
    const int* voice_ctl;
    /* class-keyed controls (commu_sample_args.cls_ctl) */
    const void* cls_ctl;
} commu_decode_loop_args;
int commu_decode_loop_args_bytes(void);
int commu_decode_sample_post_pre(const commu_decode_loop_args* a, hipStream_t stream);
/* ---- primed generation: enter the loop at an arbitrary point of a sequence (continue a given token prefix).
 * commu_forcing_replay runs the two transitions above over prompt[b][0 .. prompt_len[b]) WITHOUT a model step, starting
 * from the record, seq and klen as a load of the conditioning context leaves them (midi_inferrer.py:186-197): wherever
 * commu_forcing_pre decides to draw, the next prompt token is handed to commu_forcing_post as the drawn token; wherever
 * it feeds a forced token (midi_inferrer.py:239-320), that token must be the next prompt token.  One wave per slot.
 * Results: the record (iters and ndraw reset to 0; ntrace and the optional trace continue), seq, klen[b] (+ 1 per kept
 * model step the loop would have made), fed[b][0 ..] = the tokens of those kept steps in order (int32 [B][ld_fed]; with
 * the discarded first step left out and forced tokens doubled, quirks Q3 / Q4), and diverged[b] = {prompt index,
 * reason} or {-1, -1}: 1 the rules force another token there, 2 the book-keeping does not append the token (a chord
 * token where a draw is expected, a position past a pending chord, an EOS / bar the rules replace), 3 the prompt
 * holds EOS, 4 a token outside [0, 729) or a record that was already finished.  A slot with prompt_len 0 keeps its record
 * bit for bit.  tok / active / keep / draw / uni are the loop's scratch arrays (overwritten); seq_logp optional. */
int commu_forcing_replay(int* state, int* seq, int ld_seq, const int* prompt, int ld_prompt, const int* prompt_len,
                         const int* chord_tok, const int* chord_pos, int ld_chord, unsigned char* wrong,
                         const float* utable, int ld_u, long long* tok, unsigned char* active, unsigned char* keep,
                         unsigned char* draw, float* uni, int* trace, int ld_trace, float* seq_logp, int* klen, int* fed,
                         int ld_fed, int* diverged, int B, hipStream_t stream);
/* Ragged prefill of the K/V caches from ONE layer's time-major projection buffer of a memory-less forward over the
 * padded contexts (midi_inferrer.py:186-197 for B contexts of different lengths): qkv bf16, row t * B + b, row pitch
 * ld_qkv >= 3 H DH, DH 32 or 64.  The K and V of positions max(0, len[b] - window) <= t < len[b] go to cache rows
 * [slot[b]][h][t][DH] (window 0: linear cache, every position below len[b]) or [..][t mod (window + 1)][DH] (ring of
 * Lmax = window + 1 rows), and klen[slot[b]] = len[b].  len / slot: int32 [B] device arrays (slot null: b; slots outside
 * [0, Bcache) are skipped, len is clamped to [0, T]); rows outside the range are not touched. */
int commu_decode_prefill_scatter(const void* qkv, int ld_qkv, int T, int B, void* kcache, void* vcache, int* klen,
                                 const int* len, const int* slot, int Bcache, int H, int DH, int Lmax, int window,
                                 hipStream_t stream);
/* ---- request pool: arm decode slots for ANY request between two replays of the iteration graph (csrc/decode_arm.hip).
 * A REQUEST STORE of Rcap entries holds, per entry, everything a slot needs at the start of an attempt; every e_* array
 * below is the store's [Rcap][.] twin of the slot array [B][.] beside it, with the same row pitch.  The K/V image of an
 * entry is rows 0 .. klen0 - 1 of every layer and head in the cache's own format: image[i] is laid out like cache[i]
 * with Rcap for B and ctx_rows for Lmax ([L][Rcap][H][ctx_rows][row_bytes[i]] against [L][B][H][Lmax][row_bytes[i]]), so
 * that commu_decode_prefill_scatter / _kv8 write an image as they write a cache.  n_cache tensors (2: bf16 K, V; 4: e4m3
 * K, V and their scale bytes); row_bytes[i] is DH * 2, DH or DH / 32.
 * ONE launch arms njobs jobs, 0 <= njobs <= B; job j is (slot, entry) = jobs[2 j], jobs[2 j + 1] (device int32) and its
 * variates are variates[j][0 .. ld_u) (device fp32).  For each job with 0 <= slot < B and 0 <= entry < Rcap (others
 * are skipped), with n = e_klen0[entry] clamped to [0, min(ctx_rows, Lmax)]:
 *   cache[i][l][slot][h][0 .. n) = image[i][l][entry][h][0 .. n) for every i, l, h -- rows >= n and other slots are not
 *     touched; 16-byte vector loads and stores wherever row_bytes[i] is a multiple of 16 (K and V), bytes for the scales;
 *   klen[slot] = n;  state[slot][0 .. nf) = e_state[entry];  seq[slot][0 .. ld_head) = e_seq[entry] (pitch ld_head);
 *   chord_tok / chord_pos [slot][0 .. ld_chord) = e_chord_tok / e_chord_pos [entry];  wrong[slot][0 .. ld_wrong) = 0;
 *   utable[slot][0 .. ld_u) = variates[j];
 *   and, each only where BOTH the slot array and its store twin are given (seq_logp, trace: the slot array), as the
 *   loop's entry point treats a null array:  seq_logp[slot][0 .. 2 ld_seq) = NaN;  trace[slot][0 .. ld_trace) =
 *   e_trace[entry] where e_trace is given (a replay's trace continues into the decode), zeros where only trace is;
 *   temperature_rows / top_k_rows / top_p_rows [slot] = e_temperature / e_top_k / e_top_p [entry];
 *   bias[slot][0 .. ld_bias) = e_bias[entry];  gram_on / harm_on [slot] = e_gram_on / e_harm_on [entry] (bytes);
 *   order_ctl / voice_ctl / density_ctl / interval_ctl / onset_ctl [slot] = e_order / e_voice / e_density / e_interval /
 *   e_onset [entry] (the onset table is the pool's own: no table bytes move per arm);  guide_ctl[slot] = e_guide[entry]
 *   (likewise: the guide table is the pool's own);  art_ctl[slot] = e_art[entry] (likewise);
 *   form_ctl[slot] = e_form[entry] (likewise), and where form_state and form_tok are given the slot's form state as
 *   commu_form_reset leaves it, over the entry's sequence head (bar_at of e_seq[entry][0 .. e_state[entry][0]), so a
 *   prompt's bars are valid sources) and form_tok[slot] = -1;
 *   cls_ctl[slot][0 .. 32) = e_cls[entry] (int32).
 * tok / active / keep / draw are NOT written: an armed slot sits out the iteration whose decision was taken from its
 * finished record and starts with the next one.  Two jobs of one launch must name different slots (the caller's duty).
 * Nothing but njobs varies between launches; there is no host synchronisation.  Grid: one wave per (job, layer, head).
 *   struct_bytes: sizeof(commu_decode_arm_args) as the caller compiled it; a value that differs from the library's
 *     (commu_decode_arm_args_bytes()) is refused with -22 before anything else is looked at.
 *   njobs == 0: nothing is launched, 0.  -22: njobs outside [0, B]; B, Rcap, L, H, Lmax, ctx_rows, nf, ld_head, ld_chord,
 *     ld_wrong or ld_u < 1; ld_head > ld_seq; n_cache not 2 or 4; row_bytes[i] < 1; a null jobs, variates, klen, state,
 *     seq, chord_tok, chord_pos, wrong, utable, cache[i], image[i] or store twin of those; a cache[i] / image[i] with
 *     row_bytes[i] % 16 == 0 that is not 16-byte aligned; jobs / variates not 4-byte aligned; ring != 0 or
 *     grid_rows != 0 (the geometry of commu_decode_arm_primed below, which this launch does not have). */
typedef struct commu_decode_arm_args {
    unsigned struct_bytes;
    int njobs;
    const int* jobs;
    const float* variates;
    int B, Rcap;
    /* K/V caches and the store's images */
    int L, H, Lmax, ctx_rows, n_cache;
    int row_bytes[4];
    void* cache[4];
    const void* image[4];
    int ring, grid_rows;          /* commu_decode_arm_primed only: commu_decode_arm takes 0, 0 */
    /* required slot arrays and their store twins */
    int* klen;
    const int* e_klen0;
    int* state;
    const int* e_state;
    int nf;
    int* seq;
    const int* e_seq;
    int ld_seq, ld_head;
    int* chord_tok;
    int* chord_pos;
    const int* e_chord_tok;
    const int* e_chord_pos;
    int ld_chord;
    unsigned char* wrong;
    int ld_wrong;
    float* utable;
    int ld_u;
    /* optional */
    float* seq_logp;
    int* trace;
    const int* e_trace;
    int ld_trace;
    float* temperature_rows;
    int* top_k_rows;
    float* top_p_rows;
    const float* e_temperature;
    const int* e_top_k;
    const float* e_top_p;
    float* bias;
    const float* e_bias;
    int ld_bias;
    unsigned char* gram_on;
    const unsigned char* e_gram_on;
    unsigned char* harm_on;
    const unsigned char* e_harm_on;
    int* art_ctl;
    const int* e_art;
    int* guide_ctl;
    const int* e_guide;
    int* onset_ctl;
    const int* e_onset;
    int* interval_ctl;
    const int* e_interval;
    int* density_ctl;
    const int* e_density;
    int* order_ctl;
    const int* e_order;
    int* voice_ctl;
    const int* e_voice;
    int* cls_ctl;
    const int* e_cls;
    /* form templates: the slots' control words and their store twin, the state rows and the replay tokens
     * (at the struct's end: every other field keeps its place) */
    int* form_ctl;
    const int* e_form;
    int* form_state;
    int* form_tok;
} commu_decode_arm_args;
int commu_decode_arm_args_bytes(void);
int commu_decode_arm(const commu_decode_arm_args* a, hipStream_t stream);
/* ---- request pool, PRIMED entries: the arm launch of a pool whose requests continue a prompt of their own
 * (csrc/decode_arm.hip, the same file).  It takes the SAME argument block, and every field means what it means above.
 * An entry's K/V image is then as long as its replayed prompt (ctx_rows: hundreds to thousands of rows, not 16), so the
 * image is copied ROW-PARALLEL: grid (L H, njobs, ceil(R / C)) workgroups of 128 threads, R = min(ctx_rows, Lmax)
 * (min(.., grid_rows) where grid_rows > 0), C = commu_decode_arm_primed_chunk_rows(); chunk workgroup z moves rows
 * z C .. min(n, (z + 1) C) - 1 of its (layer, head) in every cache tensor with 16-byte vector loads and stores, four
 * independent loads per thread issued before the first store; a chunk workgroup whose first row is >= n exits (chunk 0
 * stays: the L H workgroups of a job's chunk 0 share the slot arrays' rows as the waves of commu_decode_arm do).  Plain
 * vector stores only; no atomics, no LDS, no synchronisation between workgroups.
 * What differs from commu_decode_arm, per job (slot, entry) with 0 <= slot < B and 0 <= entry < Rcap (others are skipped):
 *   rows: with R as above and k = max(e_klen0[entry], 0), n = min(k, R) rows are copied --
 *     cache[i][l][slot][h][0 .. n) = image[i][l][entry][h][0 .. n) --, rows >= n and other slots are not touched;
 *     ring == 0 (linear cache): klen[slot] = n;
 *     ring != 0 (the cache is a ring of Lmax rows, klen counts POSITIONS and the attention takes the row modulo Lmax):
 *       klen[slot] = k, unclamped; the image is then either no longer than any prompt needs (ctx_rows < Lmax, k <= ctx_rows
 *       is the caller's duty) or a ring with the cache's modulus (ctx_rows == Lmax), so min(k, Lmax) physical rows are the
 *       whole image of a wrapped prompt;
 *   seq[slot][0 .. m) = e_seq[entry][0 .. m), m = e_state[entry][0] (the record's length word) clamped to [0, ld_head];
 *     the words of seq[slot] from m on are not touched;
 *   grid_rows: 0, or an upper bound of every e_klen0 the launch will meet (the pool's longest image): fewer chunk
 *     workgroups are launched; it is part of the clamp of n above, so a longer entry is truncated, never overrun.
 *   Everything else is written as commu_decode_arm writes it (seq_logp NaN: prompt tokens carry no pair).
 * njobs == 0: nothing is launched, 0.  -22: a struct_bytes other than commu_decode_arm_primed_args_bytes() (the same
 * value), and every condition commu_decode_arm refuses but its last (ring, grid_rows); grid_rows < 0; ring != 0 with
 * ctx_rows > Lmax. */
typedef commu_decode_arm_args commu_decode_arm_primed_args;
int commu_decode_arm_primed_args_bytes(void);
int commu_decode_arm_primed_chunk_rows(void);
int commu_decode_arm_primed(const commu_decode_arm_primed_args* a, hipStream_t stream);
/* dst[b][0:n] = src[b][0:n] where mask[b] != 0 */
int commu_copy_rows_masked_f32(float* dst, int ldd, const float* src, int lds, const unsigned char* mask, int rows,
                               int n, hipStream_t stream);

/* ---- fp32 PARITY MODE of the generation path (csrc/parity_f32.hip; model.parity_fp32 / generate.py --parity).
 * The reference computes in fp32 throughout (train.py:48 `amp = None`; no autocast in commu/model/model.py); these entry
 * points restate the forward pass on fp32 operands end to end -- fp32 master weights, activations and K/V cache, fp32
 * MFMA products, accurate expf / sinf / cosf -- so that greedy decoding (midi_inferrer.py:199-237, temperature 0) picks
 * the reference's tokens wherever the top-1 / top-2 logit gap exceeds fp32 summation-order noise (~1e-6 of the range). */
/* nn.Linear (model.py:46,164,167,205,212,278): C[M,N] = A[M,K] . B[N,K]^T (+ bias[n]) (ReLU if relu) (+ resid[m,n]); all
 * fp32 row-major; any M, N, K.  M <= 64 with 16-byte aligned operands (the decode step): a skinny kernel of its own;
 * otherwise commu_gemm_f32 (ta 0, tb 1, one slab).  LayerNorm of this mode: commu_layernorm_fwd_f32 with null mean / rstd. */
int commu_gemm_nt_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                      const float* bias, const float* resid, int ldr, int relu, hipStream_t stream);
/* model.py:409-420: out[row][0:D] = E[tok[row]][0:D] * scale (scale = sqrt(d_model)) */
int commu_embed_f32(const long long* tok, const float* E, float* out, int ld, int rows, int D, float scale,
                    hipStream_t stream);
/* model.py:142-147 indexed by DISTANCE: out[d] = [sin(p * inv_freq) | cos(p * inv_freq)], d = 0 .. n-1, p = d or
 * min(d, clamp_len) when clamp_len > 0 (model.py:581-582) */
int commu_posemb_f32(const float* inv_freq, float* out, int ld, int n, int D, int clamp_len, hipStream_t stream);
/* model.py:283-345 (RelPartialLearnableMultiHeadAttn.forward without the projections), eval mode: q [T*B rows][ld_q]
 * (row i*B+b, head h at column h*DH), element (key j, sequence b, head h, d) of k / v at base + j*stride_key +
 * b*stride_seq + h*DH + d, rd [distance][ld_rd], out [T*B][ld_o].  klen (optional, int32 [B]): memory length of each
 * sequence (ragged decode batch; otherwise M for all); reset (optional, uint8 [B]): hide the memory keys of that
 * sequence; masks of model.py:549-574 with the model's mem_len.  DH <= 64. */
int commu_relattn_f32(const float* q, int ld_q, const float* k, const float* v, long long stride_key,
                      long long stride_seq, const float* rd, int ld_rd, const float* r_w_bias, const float* r_r_bias,
                      const int* klen, const unsigned char* reset, float* out, int ld_o, int T, int M, int B, int H,
                      int DH, int same_length, int mem_len, float scale, hipStream_t stream);
/* decode step: columns [HD, 2HD) / [2HD, 3HD) of row b of the new token's projection into row klen[b] of the fp32 caches
 * kc / vc [B][Lmax][HD], for the sequences with active[b] != 0 (null: all) */
int commu_decode_kv_append_f32(const float* qkv, int ld, float* kc, float* vc, const int* klen,
                               const unsigned char* active, int B, int HD, int Lmax, hipStream_t stream);
/* the decode step of the parity mode with the reference's SLIDING memory (commu/model/model.py:507-538, same_length mask
 * model.py:549-568 at qlen 1): fp32 ring caches kc / vc [B][W][H DH], W = mem_len + 1 >= 2; klen[b] = absolute positions
 * kept so far, position p in row p mod W.  commu_decode_kv_append_ring_f32 writes row klen[b] mod W;
 * commu_decode_attn_ring_f32 (q: row b of the new tokens' projections, already appended) attends positions
 * max(0, klen[b] - (W - 1)) .. klen[b] in chronological order at distance klen[b] - p (rd: [>= W][ld_rd]), the oldest
 * hidden when same_length != 0 and klen[b] >= W - 1.  Before the first wrap the result equals commu_relattn_f32's on
 * the linear cache bit for bit (one row function, csrc/attn_row_f32.h, behind both and behind commu_relattn_fwd_f32). */
int commu_decode_kv_append_ring_f32(const float* qkv, int ld, float* kc, float* vc, const int* klen,
                                    const unsigned char* active, int B, int HD, int W, hipStream_t stream);
int commu_decode_attn_ring_f32(const float* q, int ld_q, const float* kc, const float* vc, const float* rd, int ld_rd,
                               const float* r_w_bias, const float* r_r_bias, const int* klen, float* out, int ld_o, int B,
                               int H, int DH, int W, int same_length, float scale, hipStream_t stream);
/* commu_decode_prefill_scatter on the fp32 caches of this mode, kc / vc [Bcache][Lmax][HD] (midi_inferrer.py:186-197) */
int commu_decode_prefill_scatter_f32(const float* qkv, int ld, int T, int B, float* kc, float* vc, int* klen,
                                     const int* len, const int* slot, int Bcache, int HD, int Lmax, int window,
                                     hipStream_t stream);

/* ---- fp32 TRAINING MODE (csrc/train_f32.hip; model.fp32_training / train.py --parity).
 * The reference trains in fp32 (train.py:48 `amp = None`, train.py:139-169): these entry points add the backward pass
 * and the training-mode (dropout) forward to the fp32 parity forward above.  Exact fp32 products with fp32 accumulation,
 * accurate expf / logf, no floating-point atomics: every output element is written by one thread in a fixed order, so two
 * identical passes give bitwise-identical results.  Dropout sites use the bf16 path's counter-based masks
 * (commu_gemm_nt_bf16 / commu_relattn_fwd): same seed, same keep decisions, kept values scaled by 1 / (1 - thr / 65536). */
/* C[M,N] (+)= op(A)[M,K] . op(B)[K,N]; ta = 0: A stored [M][lda], ta = 1: A stored [K][lda] (op(A) = A^T); tb = 1: B
 * stored [N][ldb] (op(B) = B^T, the nn.Linear form, model.py:46,164,167,205,212,278), tb = 0: B stored [K][ldb].
 * Epilogue in order: + bias[n], ReLU, dropout (drop_p > 0; element index m * N + n), + resid[m][ldr], + C (accumulate).
 * nslabs > 1 (a long contraction, e.g. a weight gradient over T*B rows): k is split into nslabs ranges written to
 * ws [nslabs][M][N] and summed in slab order into C by commu_reduce_slabs_f32 -- needs ldc == N and no epilogue but
 * accumulate. */
int commu_gemm_f32(int ta, int tb, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                   const float* bias, int relu, float drop_p, unsigned drop_seed, const float* resid, int ldr,
                   int accumulate, float* ws, int nslabs, hipStream_t stream);
/* model.py:283-345 in train mode: q [T*B rows][ld_q], k / v [K*B rows][ld_kv] (row j*B+b, head h at column h*DH; rows
 * j < M are the memory), rd [distance][ld_rd] (distance i + M - j), out [T*B][ld_o], lse [B][H][T] = log-sum-exp of the
 * undropped scaled scores.  Masks of model.py:549-574 (causal, same_length with mem_len, reset[b] hides the memory);
 * attention dropout (model.py:327) on the probabilities with the commu_relattn_fwd mask.  DH <= 64, any DH. */
int commu_relattn_fwd_f32(const float* q, int ld_q, const float* k, const float* v, int ld_kv, const float* rd, int ld_rd,
                          const float* r_w_bias, const float* r_r_bias, const unsigned char* reset, float* out, int ld_o,
                          float* lse, int T, int M, int B, int H, int DH, int same_length, int mem_len, float scale,
                          float drop_p, unsigned drop_seed, hipStream_t stream);
/* Backward of commu_relattn_fwd_f32 (operands as there; o = its output, dout = dO, lse = its lse), recomputing S and P:
 * delta [B][H][T] = dO . O (written), then three passes with one writer per output:
 *   query-stationary: dq_ac / dq_bd [T*B][H*DH] = the AC / BD parts of dq (their column sums are the r_w_bias / r_r_bias
 *   gradients, model.py:292-297), dq [T*B][ld_dq] = their sum;
 *   key-stationary: dk, dv [K*B][ld_dkv] for all K keys, memory rows included (model.py:303-306);
 *   distance-stationary: drd [K][ld_drd], drd[d] = sum_{b,i} dS[i, i+M-d] (q_i + r_r_bias). */
int commu_relattn_bwd_f32(const float* q, int ld_q, const float* k, const float* v, int ld_kv, const float* rd, int ld_rd,
                          const float* r_w_bias, const float* r_r_bias, const unsigned char* reset, const float* o,
                          int ld_o, const float* dout, int ld_do, const float* lse, float* delta, float* dq, int ld_dq,
                          float* dq_ac, float* dq_bd, float* dk, float* dv, int ld_dkv, float* drd, int ld_drd, int T,
                          int M, int B, int H, int DH, int same_length, int mem_len, float scale, float drop_p,
                          unsigned drop_seed, hipStream_t stream);
/* nn.LayerNorm (model.py:179,352), D <= 1024; mean / rstd [rows] (both or neither; null: not saved) for the backward */
int commu_layernorm_fwd_f32(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* mean,
                            float* rstd, int rows, int D, float eps, hipStream_t stream);
/* LayerNorm backward: dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) with dy = dy + add (add: optional second
 * incoming gradient, the residual branch).  part [2][nblk][D]: per-block partial dgamma / dbeta (block k takes rows
 * [k r, (k+1) r), r = ceil(rows / nblk)), then dgamma / dbeta (optional) += their in-order sums. */
int commu_layernorm_bwd_f32(const float* dy, int lddy, const float* add, int ldadd, const float* x, int ldx,
                            const float* mean, const float* rstd, const float* gamma, float* dx, int lddx, float* part,
                            int nblk, float* dgamma, float* dbeta, int rows, int D, hipStream_t stream);
/* model.py:64-73 backward in fp32: dlogits[r][c] = g[r] (exp(logits[r][c] - lse[r]) - [c == target[r]]), c < V */
int commu_ce_bwd_f32(const float* logits, int ldl, const long long* target, const float* lse, const float* g,
                     float* dlogits, int ldd, int rows, int V, hipStream_t stream);
/* the fp32 forms of commu_ce_fwd_opts / commu_ce_bwd_opts.  The fp32 schedule's logits are fp32 like the bf16 one's, so the
 * forward is commu_ce_fwd_opts under the name of its schedule; the backward writes fp32 dlogits, columns [V, ldd) as zero */
int commu_ce_fwd_opts_f32(const float* logits, int ldl, const long long* target, float* loss, float* nll, float* lse, int rows,
                          int V, float label_smoothing, float z_loss, hipStream_t stream);
int commu_ce_bwd_opts_f32(const float* logits, int ldl, const long long* target, const float* lse, const float* g,
                          float* dlogits, int ldd, int rows, int V, float label_smoothing, float z_loss, hipStream_t stream);
/* model.py:409-420 + 585-586 backward: gE[v] += scale * sum over the rows of token v, in the order perm / offs of
 * commu_token_order, of dropout(dx[row]) (the embedding site: element index row * D + c) */
int commu_embed_bwd_f32(const long long* perm, const long long* offs, const float* dx, int ldx, float* gE, int V, int D,
                        float scale, float drop_p, unsigned drop_seed, hipStream_t stream);
/* y = x * keep / (1 - p) (element index r * cols + c; drop_p 0: no mask), and 0 where gate (optional) <= 0 -- a dropout
 * site's forward and backward (model.py:166,168,211,585-586,601), and the ReLU backward from the saved activation; y may
 * alias x */
int commu_dropout_f32(const float* x, int ldx, const float* gate, int ldg, float* y, int ldy, int rows, int cols,
                      float drop_p, unsigned drop_seed, hipStream_t stream);

/* library identification */
const char* commu_hip_version(void);

/* Host-side (no GPU): assemble one [T][B] int64 training batch from the flat corpus.  Column c streams sequence
 * seq[c] (-1: none) from position pos[c]: data[r][c] = tokens[offsets[seq[c]] + pos[c] + r] for r < cnt[c], target the
 * same shifted by one, `pad` elsewhere (commu/model/dataset.py:139-170).  Returns the number of non-pad targets
 * (sum of cnt), -22 for B > 1024.  Thread-safe; called without the GIL by the prefetch thread. */
long long commu_pack_batch(const int64_t* tokens, const int64_t* offsets, const int64_t* seq, const int64_t* pos,
                           const int64_t* cnt, int B, int T, int64_t pad, int64_t* data, int64_t* target);

#ifdef __cplusplus
}
#endif
#endif /* COMMU_HIP_H */
