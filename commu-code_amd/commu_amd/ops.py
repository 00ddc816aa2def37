"""Tensor-level wrappers over the C ABI (include/commu_hip.h).

PyTorch is used here only for device memory and the current HIP stream; all arithmetic is done
by the kernels in libcommu_hip.so.  Every wrapper refuses CPU tensors: there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import AttnBwdDesc, AttnDesc, CommuHipError, call

EPI_BIAS, EPI_RELU, EPI_RESID, EPI_RELUMASK, EPI_OUT_F32, EPI_DROPOUT, EPI_SIGNBITS_OUT, EPI_RELUBITS = 1, 2, 4, 8, 16, 32, 64, 128


def site_seed(base_seed: int, site: int) -> int:
    """32-bit seed of one dropout site of one forward call (host-side integer hash)."""
    x = (base_seed * 0x9E3779B9 + site * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _mix32(x):
    x = x & 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _mix32k(x, key):
    x = x & 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x = x ^ key                               # the key enters between the two multiply rounds (common.h mix32k)
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def dropout_keep_mask(seed: int, n: int, p: float, device="cpu"):
    """The kernels' keep mask for element indices 0..n-1 (reference implementation for tests; common.h drop_word): one
    hash word per two consecutive indices -- two 24-bit multiply-add rounds around a xor-shift, keyed by mix32(seed) --, the
    even index takes the low 16 bits, the odd one the high 16, against round(p * 65536).  Kept values are scaled by
    1 / (1 - thr / 65536) in the kernels (within 8e-6 of 1 / (1 - p))."""
    M32, M24 = 0xFFFFFFFF, 0xFFFFFF
    key = int(_mix32(torch.tensor(int(seed) & M32, dtype=torch.int64)))
    k2 = (key * 0x85EBCA6B + 0x6A09E667) & M32
    idx = torch.arange(n, dtype=torch.int64, device=device)
    q = idx >> 1
    y = ((q & M24) * 0xD2B74B + key) & M32
    y = (((q >> 24) & M24) * 0xB5297A + y) & M32
    y = y ^ (y >> 13)
    w = ((y & M24) * 0x9E3779 + k2) & M32
    w = w ^ (w >> 15)
    half = torch.where((idx & 1).bool(), w >> 16, w & 0xFFFF)
    thr = min(65535, max(1, int(p * 65536.0 + 0.5))) if p > 0 else 0
    return half >= thr


BF16 = torch.bfloat16
F32 = torch.float32

# use LDS transpose reads in the dW GEMM (mode 1) unless told otherwise
TN_MODE = 1


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise CommuHipError("commu_amd kernels need GPU tensors (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _s():
    # (the raw handle of torch's current stream: ~0.3 us, against ~8 us for torch.cuda.current_stream().cuda_stream --
    #  a training step makes ~250 kernel calls)
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def attn_dropout_keep_mask(seed: int, B: int, H: int, T: int, K: int, p: float, version: int = 3):
    """The attention kernels' keep mask [B,H,T,K] (reference implementation for tests; relattn.hip DropLane).  One mask for
    every kernel: each 32x32 block (i>>5, j>>5) of a (batch, head) has a 32-bit key k1 from the strong hash; inside the block
    one mixed word per 2x2 cell, y = ((i&31)>>1 << 4 | (j&31)>>1) * C1 + k1, y ^= y >> 12, y &= 0xFFFFFF, and one
    multiply-add per element with the constants of its place in the cell, w = y * CM[i&1][j&1] + k1 * KA[i&1][j&1] +
    KB[i&1][j&1]; keep = w >= round(p * 65536) << 16.  (`version` is accepted for older call sites and ignored.)"""
    thr = max(1, int(p * 65536.0 + 0.5)) if p > 0 else 0
    out = torch.empty(B, H, T, K, dtype=torch.bool)
    rows = torch.arange(T, dtype=torch.int64)[:, None]
    cols = torch.arange(K, dtype=torch.int64)[None, :]
    M32 = 0xFFFFFFFF
    CM = ((0x9E3779, 0x85EBCB), (0xC2B2AF, 0xB5297B))
    KA = ((0x85EBCA6B, 0xC2B2AE35), (0x27D4EB2F, 0x165667B1))
    KB = ((0x6A09E667, 0xBB67AE85), (0x3C6EF372, 0xA54FF53A))
    blk = ((rows >> 5) << 16) | (cols >> 5)
    xc = (((((rows & 31) >> 1) << 4) | ((cols & 31) >> 1)) * 0xD2B74B) & M32
    ri = (rows & 1).expand(T, K)
    ci = (cols & 1).expand(T, K)
    for b in range(B):
        for h in range(H):
            key_bh = int(_mix32(torch.tensor((seed + (b * H + h) * 0x9E3779B1) & M32, dtype=torch.int64)))
            k1 = _mix32k(blk, key_bh)
            y = (xc + k1) & M32
            y = (y ^ (y >> 12)) & 0xFFFFFF
            w = torch.zeros(T, K, dtype=torch.int64)
            for r_ in range(2):
                for c_ in range(2):
                    sel = (ri == r_) & (ci == c_)
                    wv = (y * CM[r_][c_] + ((k1 * KA[r_][c_] + KB[r_][c_]) & M32)) & M32
                    w = torch.where(sel, wv, w)
            out[b, h] = w >= (thr << 16)
    return out, 1.0 - thr / 65536.0


def attn_fwd_generation(gen: int) -> int:
    """commu_attn_fwd_generation: 0 automatic, 2 / 3 force a forward kernel family for d_head 64; returns the previous value."""
    return call("commu_attn_fwd_generation", int(gen))


def attn_bwd_kv_generation(gen: int) -> int:
    """commu_attn_bwd_kv_generation: 0 automatic; 2 / 3 force a key-stationary backward kernel for d_head 64 with stored
    probabilities; 4: both backward kernels on the 32x32 MFMA (relattn_q3.hip + relattn_kv3.hip); returns the previous value."""
    return call("commu_attn_bwd_kv_generation", int(gen))


def _rowmajor2d(t: torch.Tensor, name: str):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D tensor with unit column stride, got {tuple(t.shape)} / {t.stride()}")
    return t.stride(0)


def gemm_nt_layers(A, Bflat, N, K, stride, batch, out=None):
    """out[z] = A @ B_z^T for z < batch, B_z = Bflat[z*stride : z*stride + N*K].view(N, K): ONE launch for the same Linear
    of every layer when its input is shared (r_net on the position table, model.py:278,313)."""
    M = A.shape[0]
    assert A.dtype == BF16 and Bflat.dtype == BF16 and A.shape[1] == K and Bflat.is_contiguous()
    assert Bflat.numel() >= (batch - 1) * stride + N * K
    if out is None:
        out = torch.empty(batch, M, N, device=A.device, dtype=BF16)
    call("commu_gemm_nt_bf16_batched", _p(A), _rowmajor2d(A, "A"), 0, _p(Bflat), K, stride, _p(out), N, M * N, M, N, K,
         None, 0, 0, 0, batch, 0, 0, _s())
    return out


def signbits_words(M, N, K, lda=None, ldb=None, ldc=None):
    """32-bit words of the sign-bit buffer of an M x N GEMM output (gemm_nt sign_bits_out / relu_bits); 0 when the shape
    does not take the one-bit ReLU mask (then the bf16 relu_mask is the path)."""
    return int(call("commu_gemm_nt_signbits_words", M, N, K, K if lda is None else lda, K if ldb is None else ldb,
                    N if ldc is None else ldc))


def gemm_nt(A, B, out=None, *, bias=None, resid=None, relu=False, relu_mask=None, out_f32=False,
            drop_p=0.0, drop_seed=0, mask_scale=1.0, sign_bits_out=None, relu_bits=None):
    """out[M,N] = A[M,K] @ B[N,K]^T with the fused epilogue bias -> relu -> dropout -> +resid ->
    relu-mask (kept values * mask_scale).  A, B bf16.
    sign_bits_out (int32 [signbits_words]): receives one bit per output, (out > 0); relu_bits: such a buffer from a GEMM
    with the same M x N, used instead of relu_mask (out = bit ? out * mask_scale : 0) -- 1/16 of the mask's bytes."""
    lda, ldb = _rowmajor2d(A, "A"), _rowmajor2d(B, "B")
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K and A.dtype == BF16 and B.dtype == BF16
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=F32 if out_f32 else BF16)
    ldc = _rowmajor2d(out, "out")
    flags = 0
    if bias is not None:
        flags |= EPI_BIAS
        assert bias.dtype == F32 and bias.numel() >= N
    if resid is not None:
        flags |= EPI_RESID
        assert resid.dtype == BF16
    if relu:
        flags |= EPI_RELU
    if relu_mask is not None:
        flags |= EPI_RELUMASK
        assert relu_mask.dtype == BF16
    if out.dtype == F32:
        flags |= EPI_OUT_F32
    if drop_p > 0:
        flags |= EPI_DROPOUT
    if sign_bits_out is not None or relu_bits is not None:
        bits = sign_bits_out if sign_bits_out is not None else relu_bits
        assert relu_mask is None and not (sign_bits_out is not None and relu_bits is not None)
        assert bits.dtype == torch.int32 and bits.is_contiguous() and bits.numel() * 32 == M * N
        flags |= EPI_SIGNBITS_OUT if sign_bits_out is not None else EPI_RELUBITS
        relu_mask = bits          # (the C entry point takes the word buffer in the relu_mask argument)
        call("commu_gemm_nt_bf16", _p(A), lda, _p(B), ldb, _p(out), ldc, M, N, K, _p(bias), _p(resid),
             0 if resid is None else _rowmajor2d(resid, "resid"), _p(bits), 0,
             flags, int(drop_seed), float(drop_p), float(mask_scale), _s())
        return out
    call("commu_gemm_nt_bf16", _p(A), lda, _p(B), ldb, _p(out), ldc, M, N, K, _p(bias), _p(resid),
         0 if resid is None else _rowmajor2d(resid, "resid"), _p(relu_mask),
         0 if relu_mask is None else _rowmajor2d(relu_mask, "relu_mask"), flags, int(drop_seed), float(drop_p),
         float(mask_scale), _s())
    return out


def gemm_nt_ln(z, gamma, beta, B, out=None, *, a_out=None, bias=None, resid=None, relu=False, out_f32=False, eps=1e-5):
    """Decode-step Linear with the preceding LayerNorm fused in: out = LN(z) @ B^T (+ bias, relu, resid); `a_out`
    (bf16, same shape as z) receives LN(z).  z: [M <= 64, K] bf16 (K % 128 == 0); LN over gamma.numel() columns."""
    M, K = z.shape
    N = B.shape[0]
    assert z.dtype == BF16 and B.dtype == BF16 and B.shape[1] == K
    if out is None:
        out = torch.empty(M, N, device=z.device, dtype=F32 if out_f32 else BF16)
    if not FUSE_DECODE_LN or M > 64 or K % 128 or K > 1024 or N < 32:
        # shapes the fused kernel does not take (tiny test models, wide batches): the two kernels it replaces
        a, _, _ = layernorm_fwd(z, gamma, beta, y=a_out, eps=eps)
        return gemm_nt(a, B, out=out, bias=bias, resid=resid, relu=relu)
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_RESID if resid is not None else 0) | (EPI_RELU if relu else 0)
    if out.dtype == F32:
        flags |= EPI_OUT_F32
    call("commu_gemm_nt_ln_bf16", _p(z), _rowmajor2d(z, "z"), _p(gamma), _p(beta), gamma.numel(), float(eps),
         _p(a_out), 0 if a_out is None else _rowmajor2d(a_out, "a_out"), _p(B), _rowmajor2d(B, "B"), _p(out),
         _rowmajor2d(out, "out"), M, N, K, _p(bias), _p(resid), 0 if resid is None else _rowmajor2d(resid, "resid"),
         flags, _s())
    return out


def tn_slices(M: int, N: int, K: int) -> int:
    """Number of m-slices the TN kernel wants at this shape (enough workgroups to fill the GPU)."""
    return _lib.load().commu_gemm_tn_slices(int(M), int(N), int(K))


def gemm_tn(A, B, out, *, accumulate=False, slabs=None, mode=None):
    """out[N,K] (+)= A[M,N]^T @ B[M,K]  (fp32 out; bf16 inputs).  Split over M into slabs that
    are summed by commu_reduce_slabs_f32.  `out` may be a strided 2-D view only if contiguous."""
    lda, ldb = _rowmajor2d(A, "A"), _rowmajor2d(B, "B")
    M, N = A.shape
    K = B.shape[1]
    assert B.shape[0] == M and out.shape == (N, K) and out.dtype == F32 and out.is_contiguous()
    ns = tn_slices(M, N, K)
    if slabs is None or slabs.numel() < ns * N * K:
        slabs = torch.empty(ns * N * K, device=A.device, dtype=F32)
    call("commu_gemm_tn_bf16", _p(A), lda, _p(B), ldb, _p(slabs), K, N * K, M, N, K, ns,
         TN_MODE if mode is None else mode, _s())
    call("commu_reduce_slabs_f32", _p(out), _p(slabs), N * K, ns, N * K, 1 if accumulate else 0, 1.0, _s())
    return out


def gemm_tn_raw(A, B, slabs, nslices, mode=None):
    """slabs[s][N,K] = A[m-slice s]^T @ B[m-slice s]; reduce with reduce_slabs."""
    lda, ldb = _rowmajor2d(A, "A"), _rowmajor2d(B, "B")
    M, N = A.shape
    K = B.shape[1]
    assert B.shape[0] == M and slabs.numel() >= nslices * N * K and slabs.dtype == F32
    call("commu_gemm_tn_bf16", _p(A), lda, _p(B), ldb, _p(slabs), K, N * K, M, N, K, nslices,
         TN_MODE if mode is None else mode, _s())
    return slabs


def tn_group(pairs, colsum=None):
    """ctypes problem array for a grouped weight-gradient launch: pairs = [(dY [M,N], X [M,K]), ...] (bf16, shared M).
    Returns (array, M, offsets, total) with offsets[i] = element offset of problem i's [N, K] block inside a slab.
    colsum: per problem, whether the launch also leaves the column sums of dY (the Linear's bias gradient) in the slabs;
    then a fifth value, the slab offset of each problem's [N] vector (None where not asked), is returned."""
    arr = (_lib.TnProblem * len(pairs))()
    M = pairs[0][0].shape[0]
    offs, total = [], 0
    for i, (A, B) in enumerate(pairs):
        assert A.shape[0] == M and B.shape[0] == M and A.dtype == BF16 and B.dtype == BF16
        arr[i].A, arr[i].B = A.data_ptr(), B.data_ptr()
        arr[i].lda, arr[i].ldb = _rowmajor2d(A, "A"), _rowmajor2d(B, "B")
        arr[i].N, arr[i].K = A.shape[1], B.shape[1]
        arr[i].out_off = total
        arr[i].colsum_off = -1
        offs.append(total)
        total += A.shape[1] * B.shape[1]
    if colsum is None:
        return arr, M, offs, total
    cs = []
    for i, want in enumerate(colsum):
        if want:
            arr[i].colsum_off = total
            cs.append(total)
            total += round_up(pairs[i][0].shape[1], 4)
        else:
            cs.append(None)
    return arr, M, offs, total, cs


def tn_group_slices(arr, M, budget=None):
    """Token slices the grouped kernel wants for this group (0: not eligible -> per-problem commu_gemm_tn_bf16).
    budget: workgroups the launch may take (default: the library's 128 = half of every XCD, for a launch beside the backward pass)."""
    if budget is not None:
        return _lib.load().commu_gemm_tn_grouped_slices_budget(arr, len(arr), int(M), int(budget))
    return _lib.load().commu_gemm_tn_grouped_slices(arr, len(arr), int(M))


def gemm_tn_grouped(arr, M, slabs, slab_stride, nslices):
    """slabs[s * slab_stride + off_p + n*K_p + k] = sum over token slice s of A_p[m,n] B_p[m,k], one launch."""
    if not slabs.is_cuda:
        raise CommuHipError("commu_amd kernels need GPU tensors (no CPU fallback)")
    assert slabs.dtype == F32 and slabs.numel() >= nslices * slab_stride
    call("commu_gemm_tn_bf16_grouped", arr, len(arr), int(M), _p(slabs), int(slab_stride), int(nslices), _s())
    return slabs


def reduce_slabs(dst, slabs, n, nslabs, stride, accumulate, alpha=1.0):
    """dst.view(-1)[:n] = (accumulate ? dst : 0) + alpha * sum_s slabs[s*stride : s*stride + n]"""
    assert dst.is_contiguous() and dst.dtype == F32 and dst.numel() >= n
    call("commu_reduce_slabs_f32", _p(dst), _p(slabs), n, nslabs, stride, 1 if accumulate else 0, float(alpha), _s())
    return dst


def quant_mxfp8(X):
    """bf16 [rows, K] -> (e4m3 bytes uint8 [rows, K], E8M0 scale bytes uint8 [rows, K/32])  (OCP MX, block 32)."""
    rows, K = X.shape
    assert X.dtype == BF16 and X.stride(1) == 1 and K % 32 == 0
    Q = torch.empty(rows, K, device=X.device, dtype=torch.uint8)
    S = torch.empty(rows, K // 32, device=X.device, dtype=torch.uint8)
    call("commu_quant_mxfp8", _p(X), X.stride(0), _p(Q), K, _p(S), K // 32, rows, K, _s())
    return Q, S


def gemm_nt_mxfp8(A, SA, B, SB, out=None, bias=None, relu=False, resid=None, drop_p=0.0, drop_seed=0):
    """out bf16 [M, N] = A . B^T with MX-fp8 operands from quant_mxfp8 (A [M, K], B [N, K]); fp32 accumulation; the
    epilogue (bias -> ReLU -> dropout -> residual) is commu_gemm_nt_bf16's."""
    M, K = A.shape
    N = B.shape[0]
    assert A.dtype == torch.uint8 and B.dtype == torch.uint8 and B.shape[1] == K
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=BF16)
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_RELU if relu else 0) | (EPI_RESID if resid is not None else 0) | \
            (EPI_DROPOUT if drop_p > 0 else 0)
    call("commu_gemm_nt_mxfp8", _p(A), A.stride(0), _p(SA), SA.stride(0), _p(B), B.stride(0), _p(SB), SB.stride(0), _p(out),
         out.stride(0), M, N, K, _p(bias), _p(resid), 0 if resid is None else resid.stride(0), flags, int(drop_seed),
         float(drop_p), _s())
    return out


def linear_mxfp8(x, wq, out=None, **epi):
    """x bf16 [M, K] quantised on the fly, wq = (bytes, scales) of the weight: one Linear in MX-fp8."""
    xq, xs = quant_mxfp8(x)
    return gemm_nt_mxfp8(xq, xs, wq[0], wq[1], out=out, **epi)


def reduce_slabs_group(items, slabs, nslabs, stride, accumulate, alpha=1.0):
    """items = [(dst fp32 contiguous, src_off, crop (rg, rt, rp, cg, ct, cp))]: every reduction of a grouped
    weight-gradient launch in ONE launch (<= 8 items)."""
    arr = (_lib.ReduceItem * len(items))()
    for i, (dst, off, crop) in enumerate(items):
        rg, rt, rp, cg, ct, cp = crop
        assert dst.is_contiguous() and dst.dtype == F32 and dst.numel() >= rg * rt * cg * ct
        arr[i].dst, arr[i].src_off = dst.data_ptr(), off
        arr[i].rg, arr[i].rt, arr[i].rp, arr[i].cg, arr[i].ct, arr[i].cp = rg, rt, rp, cg, ct, cp
    call("commu_reduce_slabs_group_f32", arr, len(items), _p(slabs), nslabs, stride, 1 if accumulate else 0, float(alpha), _s())


def reduce_slabs_crop(dst, slabs, crop, nslabs, stride, accumulate, alpha=1.0):
    """crop = (rg, rt, rp, cg, ct, cp): the [rt, ct] blocks of the padded [rg*rp, cg*cp] product (summed over the
    slabs) are added to / stored in dst [rg*rt, cg*ct]."""
    rg, rt, rp, cg, ct, cp = crop
    assert dst.is_contiguous() and dst.dtype == F32 and dst.numel() == rg * rt * cg * ct
    call("commu_reduce_slabs_crop_f32", _p(dst), _p(slabs), rg, rt, rp, cg, ct, cp, nslabs, stride,
         1 if accumulate else 0, float(alpha), _s())
    return dst


def embed_fwd(tok, E, out=None, drop_p=0.0, drop_seed=0, ld=None):
    """ld > D: rows are padded to ld columns (zero-padding contract of commu_hip.h)."""
    ntok = tok.numel()
    D = E.shape[1]
    assert tok.dtype == torch.int64 and E.dtype == F32 and E.is_contiguous() and tok.is_contiguous()
    if out is None:
        out = torch.empty(ntok, D if ld is None else ld, device=E.device, dtype=BF16)
    call("commu_embed_fwd", _p(tok), _p(E), _p(out), out.stride(0), ntok, D, E.shape[0], math.sqrt(D), int(drop_seed),
         float(drop_p), _s())
    return out


def token_order(tok, V):
    """(perm, offs) for embed_bwd: stable argsort of the ids and the first sorted position of every id (int64 [V+1]).
    V <= 1024: the library's counting sort (three small launches, no framework kernels); ids outside [0, V) are left out
    of the order (they contribute nothing either way).  Larger vocabularies: torch.sort + searchsorted."""
    flat = tok.reshape(-1)
    if V <= 1024 and flat.is_cuda and flat.dtype == torch.int64 and flat.is_contiguous():
        n = flat.numel()
        perm = torch.empty(n, device=flat.device, dtype=torch.int64)
        offs = torch.empty(V + 1, device=flat.device, dtype=torch.int64)
        ws = torch.empty(64 * V, device=flat.device, dtype=torch.int32)
        call("commu_token_order", _p(flat), n, V, _p(perm), _p(offs), _p(ws), _s())
        return perm, offs
    vals, perm = torch.sort(flat, stable=True)
    offs = torch.searchsorted(vals, torch.arange(V + 1, device=tok.device, dtype=vals.dtype))
    return perm, offs


def embed_bwd(tok, dX, dE, accumulate=True, drop_p=0.0, drop_seed=0, order=None):
    """dE[v] (+)= sqrt(D) * sum over the tokens with id v of the (dropout-masked) dX rows.  order = token_order(tok, V):
    the sorted two-pass kernel (work per wave independent of how often an id occurs, fixed summation order); None: one
    workgroup per row scans the token list."""
    V, D = dE.shape
    if order is not None and dE.is_contiguous():
        perm, offs = order
        ntok = perm.numel()
        ws = torch.empty(call("commu_embed_bwd_ws_rows", ntok, V), D, device=dE.device, dtype=F32)
        call("commu_embed_bwd_sorted", _p(perm), _p(offs), _p(dX), dX.stride(0), _p(ws), ntok, D, V, _p(dE), math.sqrt(D),
             1 if accumulate else 0, int(drop_seed), float(drop_p), _s())
        return dE
    call("commu_embed_bwd", _p(tok), _p(dX), dX.stride(0), _p(dE), tok.numel(), D, V, math.sqrt(D),
         1 if accumulate else 0, int(drop_seed), float(drop_p), _s())
    return dE


def posemb(inv_freq, K, D, out=None, drop_p=0.0, drop_seed=0, ld=None, clamp_len=-1):
    """Sinusoid table by distance; clamp_len > 0: distances above it share its row (cfg.MODEL.clamp_len, model.py:581-582)."""
    if out is None:
        out = torch.empty(K, D if ld is None else ld, device=inv_freq.device, dtype=BF16)
    call("commu_posemb_fwd", _p(inv_freq), _p(out), out.stride(0), K, D, int(clamp_len), int(drop_seed), float(drop_p), _s())
    return out


def layernorm_fwd(z, gamma, beta, y=None, mean=None, rstd=None, eps=1e-5, y_drop=None, drop_p=0.0, drop_seed=0):
    """y = LN(z) over the first D = gamma.numel() columns (wider rows: zero-padding contract); optionally also
    y_drop = dropout(y) (second output)."""
    rows, D = z.shape[0], gamma.numel()
    y = torch.empty_like(z) if y is None else y
    mean = torch.empty(rows, device=z.device, dtype=F32) if mean is None else mean
    rstd = torch.empty(rows, device=z.device, dtype=F32) if rstd is None else rstd
    call("commu_layernorm_fwd", _p(z), z.stride(0), _p(gamma), _p(beta), _p(y), y.stride(0), _p(mean), _p(rstd),
         rows, D, eps, _p(y_drop), 0 if y_drop is None else y_drop.stride(0), int(drop_seed), float(drop_p), _s())
    return y, mean, rstd


def layernorm_bwd(dy, z, mean, rstd, gamma, dz=None, part=None, dz_masked=None, drop_p=0.0, drop_seed=0, add=None):
    """Returns (dz, part) with part [nblk, 3, D]: partial column sums of dy*xhat, dy, dz (or of
    dz_masked = dz * keep/(1-p) when that second output is requested).  D = gamma.numel().
    add (optional, bf16 like dy): the incoming gradient is dy + add (a residual branch's gradient)."""
    rows, D = z.shape[0], gamma.numel()
    nblk = call("commu_layernorm_bwd_nblocks", rows)
    dz = torch.empty_like(z) if dz is None else dz
    if part is None:
        part = torch.empty(nblk, 3, D, device=z.device, dtype=F32)
    if add is not None:
        call("commu_layernorm_bwd_add", _p(dy), dy.stride(0), _p(add), add.stride(0), _p(z), z.stride(0), _p(mean), _p(rstd),
             _p(gamma), _p(dz), dz.stride(0), _p(part), rows, D, _p(dz_masked), 0 if dz_masked is None else dz_masked.stride(0),
             int(drop_seed), float(drop_p), _s())
        return dz, part[:nblk]
    call("commu_layernorm_bwd", _p(dy), dy.stride(0), _p(z), z.stride(0), _p(mean), _p(rstd), _p(gamma), _p(dz),
         dz.stride(0), _p(part), rows, D, _p(dz_masked), 0 if dz_masked is None else dz_masked.stride(0),
         int(drop_seed), float(drop_p), _s())
    return dz, part[:nblk]


def gelu_fwd(z, drop_p=0.0, drop_seed=0, out=None):
    """out = dropout(gelu(z)) (exact erf form); z bf16 2-D.  Non-default FFN activation (commu_hip.h)."""
    rows, cols = z.shape
    if out is None:
        out = torch.empty(rows, z.stride(0), device=z.device, dtype=BF16)[:, :cols]
    call("commu_gelu_fwd", _p(z), z.stride(0), _p(out), out.stride(0), rows, cols, int(drop_seed), float(drop_p), _s())
    return out


def gelu_bwd(dy, z, drop_p=0.0, drop_seed=0, out=None):
    """dz = dy * keep/(1-p) * gelu'(z)."""
    rows, cols = z.shape
    if out is None:
        out = torch.empty(rows, z.stride(0), device=z.device, dtype=BF16)[:, :cols]
    call("commu_gelu_bwd", _p(dy), dy.stride(0), _p(z), z.stride(0), _p(out), out.stride(0), rows, cols, int(drop_seed),
         float(drop_p), _s())
    return out


class ColsumGroup:
    """Collects the final column-sum passes of a backward step (bias, LayerNorm-parameter and shared attention-bias
    gradients) and runs them as ONE launch (commu_colsum_group_f32): sources that add into the same output are walked by
    the same workgroups, in the order they were added.  colsum(..., group=g) / layernorm_bwd_reduce(..., group=g) only run
    their slab pass (if any) right away; flush() launches the rest on the current stream."""

    def __init__(self):
        self.by_out = {}          # out.data_ptr() -> [out, cols, [(X tensor, ptr, ldx, rows, alpha), ...]]
        self.keep = []

    def add(self, out, cols, X, ptr, ldx, rows, alpha):
        ent = self.by_out.setdefault(out.data_ptr(), [out, cols, []])
        assert ent[1] == cols
        ent[2].append((ptr, ldx, rows, float(alpha)))
        self.keep.append(X)

    def flush(self):
        # (no record_stream on the sources: the caller keeps this object -- and with it every source -- alive until the
        #  streams are joined; recording ~60 cross-stream uses per step made every later allocation poll their events:
        #  the host-bound step at 8 sequences per GPU went from 5.4 to 10-13 ms)
        tasks, srcs = [], []

        def launch():
            if not tasks:
                return
            ta = (_lib.ColsumTask * len(tasks))()
            sa = (_lib.ColsumSource * len(srcs))()
            for i, (o, cols, b, e) in enumerate(tasks):
                ta[i].out, ta[i].cols, ta[i].src_begin, ta[i].src_end = o, cols, b, e
            for i, (ptr, ldx, rows, alpha) in enumerate(srcs):
                sa[i].X, sa[i].ldx, sa[i].rows, sa[i].alpha = ptr, ldx, rows, alpha
            call("commu_colsum_group_f32", ta, len(tasks), sa, len(srcs), _s())
            tasks.clear()
            srcs.clear()
        for out, cols, lst in self.by_out.values():
            if len(tasks) + 1 > 48 or len(srcs) + len(lst) > 64:
                launch()
            b = len(srcs)
            srcs.extend(lst)
            tasks.append((out.data_ptr(), cols, b, len(srcs)))
        launch()
        self.by_out = {}          # (self.keep stays: see above)


def layernorm_bwd_reduce(part, dgamma, dbeta, dbias=None, group=None):
    """One launch for the three partial-sum planes of layernorm_bwd: accumulates into the gradients (group: deferred
    into the step's grouped final pass)."""
    nblk, _, D = part.shape
    assert part.is_contiguous() and part.dtype == F32
    if group is not None:
        for z, dst in enumerate((dgamma, dbeta, dbias)):
            if dst is not None:
                group.add(dst, D, part, part.data_ptr() + 4 * z * D, 3 * D, nblk, 1.0)
        return
    call("commu_layernorm_bwd_reduce", _p(part), nblk, D, _p(dgamma), _p(dbeta), _p(dbias), _s())


def colsum(X, out, alpha=1.0, group=None):
    """out[c] += alpha * sum_r X[r, c]  (X bf16 or fp32; deterministic two-pass sum, no atomics).  group: only the slab
    pass runs now, the final pass joins the group's single launch."""
    rows, cols = X.shape
    bf = X.dtype == BF16
    ny = call("commu_colsum_slabs", rows, cols, 2 if bf else 4)
    ws = torch.empty(ny, round_up(cols, 8 if bf else 4), device=X.device, dtype=F32) if ny > 0 else None
    if group is not None:
        if ny > 0:
            got = call("commu_colsum_slab_pass", _p(X), 2 if bf else 4, X.stride(0), rows, cols, _p(ws), ny, _s())
            if got != ny:
                raise CommuHipError(f"commu_colsum_slab_pass returned {got} (expected {ny})")
            group.add(out, cols, ws, ws.data_ptr(), ws.stride(0), ny, alpha)
        else:
            assert X.dtype == F32
            group.add(out, cols, X, X.data_ptr(), X.stride(0), rows, alpha)
        return out
    call("commu_colsum_bf16" if bf else "commu_colsum_f32", _p(X), X.stride(0), rows, cols, _p(out), _p(ws), ny,
         float(alpha), _s())
    return out


def ce_fwd(logits, target, V):
    rows = logits.shape[0]
    nll = torch.empty(rows, device=logits.device, dtype=F32)
    lse = torch.empty(rows, device=logits.device, dtype=F32)
    call("commu_ce_fwd", _p(logits), logits.stride(0), _p(target), _p(nll), _p(lse), rows, V, _s())
    return nll, lse


def ce_bwd(logits, target, lse, g, V, dlogits=None):
    rows = logits.shape[0]
    if dlogits is None:
        dlogits = torch.empty(rows, logits.stride(0), device=logits.device, dtype=BF16)
    call("commu_ce_bwd", _p(logits), logits.stride(0), _p(target), _p(lse), _p(g), _p(dlogits), dlogits.stride(0),
         rows, V, _s())
    return dlogits


def ce_fwd_opts(logits, target, V, label_smoothing=0.0, z_loss=0.0, entry="commu_ce_fwd_opts"):
    """(loss, nll, lse) [rows] of the loss with options: loss = (1 - eps) nll + eps (lse - mean_j l_j) + zeta lse^2 over the V
    real tokens; nll and lse are ce_fwd's."""
    rows = logits.shape[0]
    loss, nll, lse = (torch.empty(rows, device=logits.device, dtype=F32) for _ in range(3))
    call(entry, _p(logits), logits.stride(0), _p(target), _p(loss), _p(nll), _p(lse), rows, V,
         float(label_smoothing), float(z_loss), _s())
    return loss, nll, lse


def ce_bwd_opts(logits, target, lse, g, V, label_smoothing=0.0, z_loss=0.0, dlogits=None):
    """bf16 dlogits [rows, ld] of ce_fwd_opts' loss weighted by g [rows] (lse: the forward's); pad columns zero."""
    rows = logits.shape[0]
    if dlogits is None:
        dlogits = torch.empty(rows, logits.stride(0), device=logits.device, dtype=BF16)
    call("commu_ce_bwd_opts", _p(logits), logits.stride(0), _p(target), _p(lse), _p(g), _p(dlogits), dlogits.stride(0),
         rows, V, float(label_smoothing), float(z_loss), _s())
    return dlogits


def nll_by_class(nll, target, class_of_token, n_classes, pad=-1):
    """(sum fp32 [n_classes], count int32 [n_classes]) of nll over the rows by the class of their target token
    (class_of_token: int32 [V] on the device); rows whose target is `pad` are left out.  Deterministic (two passes)."""
    rows = nll.numel()
    dev = nll.device
    assert nll.dtype == F32 and nll.is_contiguous() and target.dtype == torch.int64 and target.is_contiguous()
    assert target.numel() == rows and class_of_token.dtype == torch.int32 and class_of_token.is_contiguous()
    nblk = call("commu_nll_by_class_blocks", rows)
    part_sum = torch.empty(nblk, n_classes, device=dev, dtype=F32)
    part_cnt = torch.empty(nblk, n_classes, device=dev, dtype=torch.int32)
    out_sum = torch.empty(n_classes, device=dev, dtype=F32)
    out_cnt = torch.empty(n_classes, device=dev, dtype=torch.int32)
    call("commu_nll_by_class", _p(nll), _p(target), _p(class_of_token), class_of_token.numel(), n_classes, int(pad), rows,
         _p(part_sum), _p(part_cnt), nblk, _p(out_sum), _p(out_cnt), _s())
    return out_sum, out_cnt


def mems_update(hids, mems, out, beg):
    """K9: out[l] = cat(mems[l], hids[l])[beg:]  with hids [L+1, T*B, Dp], mems [L+1, M, B, Dp] (layer stride free),
    out [L+1, n, B, Dp] contiguous, 0 <= beg < M."""
    Lp, _, B, Dp = out.shape
    M = mems.shape[1]
    step = B * Dp
    assert 0 <= beg < M and hids.shape[0] == Lp == mems.shape[0] and out.is_contiguous()
    assert out.shape[1] * step == (M - beg) * step + hids.shape[1] * Dp
    call("commu_mems_update", _p(hids), hids.stride(0), 0, hids.shape[1] * Dp, _p(mems), mems.stride(0), beg * step,
         (M - beg) * step, _p(out), out.stride(0), Lp, _s())
    return out


def masked_mean(nll, target, pad, scale, ws_sum, ws_cnt, out):
    call("commu_masked_mean", _p(nll), _p(target), nll.numel(), pad, scale, _p(ws_sum), _p(ws_cnt), _p(out), _s())
    return out


def masked_sum(nll, target, pad):
    """fp32 [1]: the sum of nll over the targets that are not `pad` (commu_masked_mean's sum workspace; its mean and count
    go to scratch) -- the plain-NLL sum of the logging window when the step trains on a loss with options."""
    ws = torch.empty(3, device=nll.device, dtype=F32)
    call("commu_masked_mean", _p(nll), _p(target), nll.numel(), int(pad), 1.0, _p(ws), ws.data_ptr() + 4, ws.data_ptr() + 8, _s())
    return ws[:1]


def loss_grad(target, pad, ws_cnt, scale, g):
    call("commu_loss_grad", _p(target), target.numel(), pad, _p(ws_cnt), scale, _p(g), _s())
    return g


def masked_mean_groups(nll, target, pad, scale, B, Bc, ws_sum, ws_cnt, out, sum_all=None):
    """[T, B] loss whose columns are B / Bc micro-batches: out = scale * sum over the groups of their masked means."""
    call("commu_masked_mean_groups", _p(nll), _p(target), nll.numel(), pad, scale, B, Bc, _p(ws_sum), _p(ws_cnt), _p(out),
         _p(sum_all), _s())
    return out


def loss_grad_groups(target, pad, ws_cnt, scale, B, Bc, g):
    call("commu_loss_grad_groups", _p(target), target.numel(), pad, _p(ws_cnt), scale, B, Bc, _p(g), _s())
    return g


def grad_norm(g, part, out):
    call("commu_grad_norm", _p(g), g.numel(), _p(part), part.numel(), _p(out), _s())
    return out


def adam_step(p, g, m, v, p_bf16, lr, step, gnorm=None, clip=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    call("commu_adam_step", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), lr, beta1, beta2, eps, step,
         _p(gnorm), clip, _s())


def adam_step_dev(p, g, m, v, p_bf16, scal, gnorm=None, clip=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """adam_step with {lr, 1 - beta1^t, 1 - beta2^t} read from the device tensor `scal` (fp32 [>= 3]): graph-replayable."""
    assert scal.dtype == F32 and scal.numel() >= 3
    call("commu_adam_step_dev", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), _p(scal), beta1, beta2, eps,
         _p(gnorm), clip, _s())


def adam_bias_corrections(beta1, beta2, step):
    """(1 - beta1^step, 1 - beta2^step) in the library's own float arithmetic (bit-identical to commu_adam_step's)."""
    out = (C.c_float * 2)()
    call("commu_adam_bias_corrections", float(beta1), float(beta2), int(step), out)
    return float(out[0]), float(out[1])


OPTIM_MAX_GROUPS = 16          # COMMU_OPTIM_MAX_GROUPS


def _group_args(lrs, wds, frozen):
    k = len(lrs)
    if not (1 <= k <= OPTIM_MAX_GROUPS and len(wds) == k and len(frozen) == k):
        raise CommuHipError(f"1 .. {OPTIM_MAX_GROUPS} optimiser groups, got {k}")
    mask = sum(1 << i for i, f in enumerate(frozen) if f)
    return (C.c_float * k)(*[float(x) for x in lrs]), (C.c_float * k)(*[float(x) for x in wds]), mask


def adam_step_groups(p, g, m, v, p_bf16, block_group, lrs, wds, frozen, step, decoupled=False, gnorm=None, clip=0.0,
                     beta1=0.9, beta2=0.999, eps=1e-8):
    """adam_step over WHOLE flat buffers (every tensor at a multiple of 64 elements) with per-group lr / weight decay /
    frozen flag; block_group: uint8 device tensor, one group number per 64-element block.  decoupled: AdamW's decay."""
    assert block_group.dtype == torch.uint8 and block_group.numel() * 64 == p.numel()
    lr_a, wd_a, mask = _group_args(lrs, wds, frozen)
    call("commu_adam_step_groups", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), _p(block_group), len(lrs), lr_a, wd_a,
         mask, int(bool(decoupled)), beta1, beta2, eps, step, _p(gnorm), clip, _s())


def group_table(lrs, wds, frozen, bc1, bc2):
    """The 2 + 3 * 16 floats commu_adam_step_groups_dev reads (host tensor): entries past the groups in use are frozen."""
    _group_args(lrs, wds, frozen)
    k, G = len(lrs), OPTIM_MAX_GROUPS
    pad = [0.0] * (G - k)
    return torch.tensor([bc1, bc2] + [float(x) for x in lrs] + pad + [float(x) for x in wds] + pad
                        + [1.0 if f else 0.0 for f in frozen] + [1.0] * (G - k), dtype=F32)


def adam_step_groups_dev(p, g, m, v, p_bf16, block_group, table, decoupled=False, gnorm=None, clip=0.0, beta1=0.9, beta2=0.999,
                         eps=1e-8):
    """adam_step_groups with the bias corrections and the group table read from the device tensor `table` (group_table)."""
    assert block_group.dtype == torch.uint8 and block_group.numel() * 64 == p.numel()
    assert table.dtype == F32 and table.numel() >= 2 + 3 * OPTIM_MAX_GROUPS
    call("commu_adam_step_groups_dev", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), _p(block_group), _p(table),
         int(bool(decoupled)), beta1, beta2, eps, _p(gnorm), clip, _s())


def grad_norm_groups(g, block_group, frozen, part, out):
    """grad_norm over the blocks whose group is not frozen (the frozen ones are not read)."""
    assert block_group.dtype == torch.uint8 and block_group.numel() * 64 == g.numel()
    mask = sum(1 << i for i, f in enumerate(frozen) if f)
    call("commu_grad_norm_groups", _p(g), g.numel(), _p(block_group), mask, _p(part), part.numel(), _p(out), _s())
    return out


def set_seed_salt(src):
    """Every dropout site adds the uint32 at device tensor `src` (int32 [1]) to its seed from now on (None: back to 0)."""
    call("commu_set_seed_salt", _p(src), _s())


def scale_clip(g, gnorm, clip):
    """g *= min(1, clip / (gnorm + 1e-6))   (torch.nn.utils.clip_grad_norm_, train.py:159-161)"""
    call("commu_scale_clip_f32", _p(g), g.numel(), _p(gnorm), clip, _s())
    return g


def cast_bf16(x, out=None):
    out = torch.empty(x.shape, device=x.device, dtype=BF16) if out is None else out
    call("commu_cast_f32_bf16", _p(x), _p(out), x.numel(), _s())
    return out


def cast_f32(x, out=None):
    out = torch.empty(x.shape, device=x.device, dtype=F32) if out is None else out
    call("commu_cast_bf16_f32", _p(x), _p(out), x.numel(), _s())
    return out


def transpose_to_bf16(x, out=None):
    """out[c, r] = bf16(x[r, c]) for a 2-D fp32 or bf16 x."""
    rows, cols = x.shape
    out = torch.empty(cols, rows, device=x.device, dtype=BF16) if out is None else out
    name = "commu_transpose_f32_bf16" if x.dtype == F32 else "commu_transpose_bf16"
    call(name, _p(x), x.stride(0), _p(out), out.stride(0), rows, cols, _s())
    return out


def transpose_group_bf16(pairs):
    """out[c, r] = x[r, c] for every (x, out) pair of bf16 2-D tensors, 32 pairs per launch."""
    for i in range(0, len(pairs), 32):
        part = pairs[i:i + 32]
        arr = (_lib.TransposeItem * len(part))()
        for k, (x, out) in enumerate(part):
            if not x.is_cuda:
                raise CommuHipError("commu_amd kernels need GPU tensors (no CPU fallback)")
            assert x.dtype == BF16 and out.dtype == BF16 and x.stride(1) == 1 and out.stride(1) == 1
            rows, cols = x.shape
            assert out.shape[0] == cols and out.shape[1] >= rows
            arr[k].src, arr[k].dst = x.data_ptr(), out.data_ptr()
            arr[k].ldi, arr[k].ldo, arr[k].rows, arr[k].cols = x.stride(0), out.stride(0), rows, cols
        call("commu_transpose_group_bf16", arr, len(part), _s())


def transpose_heads(src, J, B, H, DH, W, off=0, bias=None, out=None):
    """out[b,h,f, off+j] = src[(j*B+b), h*DH+f] (+bias[h*DH+f]); other columns zero.  src is a 2-D view."""
    if out is None:
        out = torch.empty(B, H, DH, W, device=src.device, dtype=BF16)
    call("commu_transpose_heads", _p(src), src.stride(0), _p(bias), _p(out), J, B, H, DH, W, off, _s())
    return out


def round_up(x, m):
    return (x + m - 1) // m * m


def _attn_desc(q, k, v, rd, u, vb, reset, T, M, B, H, DH, ld_o, same_length, mem_len, drop_p=0.0, drop_seed=0,
               scale=None):
    d = AttnDesc()
    d.drop_p, d.drop_seed = float(drop_p), int(drop_seed)
    d.q, d.k, d.v, d.rd = q.data_ptr(), k.data_ptr(), v.data_ptr(), rd.data_ptr()
    d.r_w_bias, d.r_r_bias = u.data_ptr(), vb.data_ptr()
    d.reset = reset.data_ptr() if reset is not None else None
    d.ld_qkv, d.ld_rd, d.ld_o = q.stride(0), rd.stride(0), ld_o
    d.T, d.M, d.B, d.H, d.DH = T, M, B, H, DH
    K = T + M
    # model.py:549-568: mask_len = klen - mem_len; shift = qlen - mask_len if mask_len > 0 else qlen
    d.same_length = 1 if same_length else 0
    mask_len = K - mem_len
    d.sshift = (T - mask_len) if mask_len > 0 else T
    # (scale: 1/sqrt(true d_head) when the head dimension is zero-padded, e.g. 50 -> 64)
    d.scale = 1.0 / math.sqrt(DH) if scale is None else float(scale)
    return d


# Training forward (d_head 64) that SAVES its probabilities for the backward pass (commu_relattn_fwd_save): the
# query-stationary backward kernel then recomputes neither scores, rel-shift, masks, exponentials nor the dropout hash (2 of
# its 4 products remain).  Built, tested (tests/test_kernels_gpu.py "forward_p") and OFF by default: on MI355X the step is
# bound by memory traffic, and the trade buys compute with bytes -- relattn_bwd_q 690 -> 645 us, relattn_fwd3 297 -> 358 us
# (+0.59 GB of stores per launch through a store path that is already the forward's second-largest cost), the step within
# +-1 % (16.48 -> 16.36 ms on one box), +6.8 GB of HBM traffic and +6.4 GB of live memory per step.  Feeding the
# key-stationary kernel from the same tiles (so that no kernel stores P) was built too: that kernel 292 -> 387 us, the step
# 15.80 -> 16.10 ms.  DESIGN.md section 8e.
import os as _os
FWD_SAVES_P = _os.environ.get("COMMU_FWD_SAVES_P", "0") == "1"


def relattn_fwd(q, k, v, rd, u, vb, reset, T, M, B, H, DH, same_length, mem_len, out=None, lse=None,
                save_q=False, drop_p=0.0, drop_seed=0, scale=None, save_p=False):
    """q: 2-D view [T*B, H*DH] (row stride ld_qkv), k, v: [(T+M)*B, H*DH]; rd: [K, H*DH] by distance.
    Returns (out bf16 [T*B, H*DH], lse fp32 [B,H,T], (qu2, qv2) or None); with save_p (d_head 64, generation-3 forward)
    the third value is (qu2, qv2, pf): pf = the forward pass's probabilities for relattn_bwd (None when not available)."""
    if out is None:
        out = torch.empty(T * B, H * DH, device=q.device, dtype=BF16)
    if lse is None:
        lse = torch.empty(B, H, T, device=q.device, dtype=F32)
    qs = None
    if save_q:
        qs = (torch.empty(T * B, H * DH, device=q.device, dtype=BF16), torch.empty(T * B, H * DH, device=q.device, dtype=BF16))
    d = _attn_desc(q, k, v, rd, u, vb, reset, T, M, B, H, DH, out.stride(0), same_length, mem_len, drop_p, drop_seed,
                   scale)
    if save_p and qs is not None:
        pf = None
        if DH == 64 and FWD_SAVES_P and call("commu_attn_fwd_generation", -1) in (0, 3):
            pf = torch.empty(call("commu_attn_pf_bytes", T, M, B, H), device=q.device, dtype=torch.uint8)
            if POISON_SCRATCH:
                pf.fill_(0xFF)          # (bf16 / fp32 NaN patterns: tiles the forward never writes must never be used)
            call("commu_relattn_fwd_save", C.byref(d), _p(out), _p(lse), _p(qs[0]), _p(qs[1]), _p(pf), _s())
            return out, lse, (qs[0], qs[1], pf)
        call("commu_relattn_fwd", C.byref(d), _p(out), _p(lse), _p(qs[0]), _p(qs[1]), _s())
        return out, lse, (qs[0], qs[1], None)
    call("commu_relattn_fwd", C.byref(d), _p(out), _p(lse), _p(qs[0]) if qs else None, _p(qs[1]) if qs else None, _s())
    return out, lse, qs


POISON_SCRATCH = False      # tests: fill uninitialised scratch with NaN to prove nothing reads it
# decode step: LayerNorm inside the consuming Linear (commu_gemm_nt_ln_bf16).  Measured on MI355X (64 sequences, L6
# D512): 0.324 ms / step fused vs 0.293 ms with the separate LayerNorm kernel -- the two LDS reductions and the
# normalisation arithmetic cost a latency-bound skinny GEMM more than the launch they save -- so it is OFF by default.
FUSE_DECODE_LN = False
STORE_ATTN_P = True         # backward: bwd_q stores P for bwd_kv (d_head 64); False: both kernels recompute it
# delta = rowsum(o . dO): the separate commu_attn_delta launch (True, the default) or inside the query-stationary kernel
# (commu_attn_bwd_desc.o).  In the step the two take the same time (round 4: 16.35 / 16.44 vs 16.36 / 16.44 ms; round 5, three
# interleaved pairs: 15.92-15.95 ms both): in-kernel, the 28 us launch and 0.35 GB of HBM traffic per step go (o is read once
# where the launch reads o and dO), but every one of bwd_q's 8192 short-lived workgroups pays a longer prologue (0.588 against
# 0.558 ms per launch in the step).  Equal: the kernel stays lean and the launch stays (COMMU_DELTA_KERNEL=0 selects the other).
DELTA_KERNEL = _os.environ.get("COMMU_DELTA_KERNEL", "1") != "0"
NO_FUSED_BAND = False       # tests / A-B runs: keep the two band GEMMs instead of commu_relattn_bwd_band


def relattn_bwd(q, k, v, rd, u, vb, reset, T, M, B, H, DH, same_length, mem_len, o, dout, lse, qs, dq, dk, dv,
                drd, du, dvb, drop_p=0.0, drop_seed=0, scale=None, scratch=None, defer=None, colsum_group=None,
                dq_colsum=True):
    """Backward of relattn_fwd.  dq/dk/dv: bf16 2-D views (row stride ld_dqkv) written in place;
    drd: fp32 [K, H*DH] (overwritten); du, dvb: fp32 [H*DH] accumulated into.  dq_colsum=False: the caller adds the
    colsum(dq) term of dvb itself (the model takes it from the qkv weight-gradient launch)."""
    dev = q.device
    K = T + M
    HD = H * DH
    qrows = call("commu_attn_bwd_qrows", T)
    QT = (T + qrows - 1) // qrows
    qu2, qv2 = qs[0], qs[1]
    pf = qs[2] if len(qs) > 2 else None          # probabilities saved by the forward pass (relattn_fwd(save_p=True))
    # delta[b,h,i] = sum_d o . dout: computed (and written, for the key-stationary kernel) by the query-stationary kernel
    # from the dout fragments it holds anyway (commu_attn_bwd_desc.o); DELTA_KERNEL: the separate launch instead
    delta = torch.empty(B, H, T, device=dev, dtype=F32)
    if DELTA_KERNEL or o.stride(0) != dout.stride(0):
        call("commu_attn_delta", _p(o), _p(dout), o.stride(0), _p(delta), T, B, H, DH, _s())
    # fused band pass (commu_relattn_bwd_band: dq_BD and dRd in ONE sweep over dS-by-distance) when the shape allows
    band_slabs = call("commu_attn_band_pairs", T, B, H) if (DH == 64 and K <= 4096 and not NO_FUSED_BAND) else 0
    ld_dsk = round_up(K, 128) if band_slabs else round_up(K, 32)
    # dS by distance is lower-triangular (d <= i + M).  Without same_length / reset masks the two GEMMs below only
    # visit the band (half the work) and the kernel only writes the triangle.  What lies right of the causal edge
    # must read as zero: either the kernel also writes a wedge of zeros as wide as a GEMM tile can overhang
    # (fresh, uninitialised scratch) or the caller keeps ONE zero-initialised scratch per shape alive
    # (`scratch` dict, used by the model): nothing ever writes beyond the triangle, so it stays zero -- no 1 GB
    # fill per layer and no wedge.
    # (reset_mems: the kernel writes zeros over the distances of the memory tiles a fresh sequence skips, so the band
    #  structure -- and the persistent scratch -- also hold for the training configurations with XL memory)
    band = not same_length
    key = (T, M, B, H, ld_dsk, str(dev))
    if band and scratch is not None and not POISON_SCRATCH:
        if scratch.get("key") != key:
            scratch["key"], scratch["dsk"] = key, None          # drop the old buffer before allocating the new one
            scratch["dsk"] = torch.zeros(H, T * B, ld_dsk, device=dev, dtype=BF16)
        dsk, wedge = scratch["dsk"], 0
    elif band:
        # (zeros right of the causal edge, as wide as a GEMM tile / a 256-distance chunk of the fused pass overhangs)
        wedge = (136 + (64 + B - 1) // B) if band_slabs else (136 + (128 + B - 1) // B)
        dsk = torch.empty(H, T * B, ld_dsk, device=dev, dtype=BF16)
        if POISON_SCRATCH:
            dsk.fill_(float("nan"))
    else:
        wedge = 0
        dsk = torch.zeros(H, T * B, ld_dsk, device=dev, dtype=BF16)
    tri_B, tri_M = (B, M) if band else (0, 0)
    dq_ac = torch.empty(T * B, HD, device=dev, dtype=BF16)
    du_part = torch.empty(B * QT, HD, device=dev, dtype=F32)
    d = _attn_desc(q, k, v, rd, u, vb, reset, T, M, B, H, DH, o.stride(0), same_length, mem_len, drop_p, drop_seed,
                   scale)
    e = AttnBwdDesc()
    e.dout, e.lse, e.delta = dout.data_ptr(), lse.data_ptr(), delta.data_ptr()
    e.qu2, e.qv2 = qu2.data_ptr(), qv2.data_ptr()
    e.dq_ac, e.dk, e.dv = dq_ac.data_ptr(), dk.data_ptr(), dv.data_ptr()
    e.dsk, e.du_part = dsk.data_ptr(), du_part.data_ptr()
    e.ld_dqkv, e.ld_dsk, e.du_rows, e.dsk_wedge = dk.stride(0), ld_dsk, QT, wedge
    e.dsk_tiled = 1 if band_slabs else 0
    pscr = None
    if DH == 64 and STORE_ATTN_P:
        # the query-stationary kernel stores the probabilities it recomputes, the key-stationary one reads them back
        n = call("commu_attn_p_scratch_elems", T, M, B, H)
        if scratch is not None and not POISON_SCRATCH:
            if scratch.get("p") is None or scratch["p"].numel() < n:
                scratch["p"] = None
                scratch["p"] = torch.empty(n, device=dev, dtype=BF16)
            pscr = scratch["p"]
        else:
            pscr = torch.empty(n, device=dev, dtype=BF16)
            if POISON_SCRATCH:
                pscr.fill_(float("nan"))
        e.p_scratch = pscr.data_ptr()
        if pf is not None:
            e.pf = pf.data_ptr()
    assert dv.stride(0) == dk.stride(0)
    if not (DELTA_KERNEL or o.stride(0) != dout.stride(0)):
        e.o = o.data_ptr()
    call("commu_relattn_bwd_q", C.byref(d), C.byref(e), _s())
    call("commu_relattn_bwd_kv", C.byref(d), C.byref(e), _s())
    c2 = d.scale * 1.4426950408889634
    TB = T * B
    if band_slabs:
        # one pass: dq = dq_ac + dsk . Rd on this stream; the dRd partial slabs are reduced off the critical path
        kpad = round_up(K, 512)          # slab rows: the kernel works in passes of 512 distances
        slabs = torch.empty(H * band_slabs * kpad * DH, device=dev, dtype=F32)
        call("commu_relattn_bwd_band", _p(dsk), ld_dsk, _p(rd), rd.stride(0), _p(qv2), qv2.stride(0), _p(dq_ac), HD,
             _p(dq), dq.stride(0), _p(slabs), T, M, B, H, DH, 1 if band else 0, _s())

        def drd_reduce():
            if defer is not None:
                slabs.record_stream(torch.cuda.current_stream())
            call("commu_reduce_slabs2d_f32", _p(drd), drd.stride(0), DH, _p(slabs), K, DH, band_slabs, kpad * DH, H, 0,
                 1.0 / c2, _s())
        if defer is None:
            drd_reduce()
        else:
            defer(drd_reduce)
        _bias_grads(dq if dq_colsum else None, du_part, du, dvb, HD, dev, defer, colsum_group)
        return delta
    # BD part of dq and dRd: two GEMMs per head over dS-by-distance, batched over the heads
    rdt = transpose_heads(rd, K, 1, H, DH, ld_dsk)                   # [1, H, DH, ld_dsk]
    call("commu_gemm_nt_bf16_batched", _p(dsk), ld_dsk, TB * ld_dsk, _p(rdt), ld_dsk, DH * ld_dsk, _p(dq), dq.stride(0),
         DH, TB, DH, ld_dsk, _p(dq_ac), HD, DH, EPI_RESID, H, tri_B, tri_M, _s())
    def drd_part():
        # dRd only feeds r_net's weight gradient: `defer` (optional) runs it off the critical path (side stream)
        if defer is not None:
            # a call-local dS-by-distance buffer (reset / same_length masks, or no persistent scratch) must outlive
            # this function on the deferring stream: without this the main-stream allocator may hand the block to
            # the next layer while the GEMM below is still reading it
            dsk.record_stream(torch.cuda.current_stream())
            qv2.record_stream(torch.cuda.current_stream())
        ns = tn_slices(TB, ld_dsk, DH * H)
        slabs = torch.empty(H * ns * ld_dsk * DH, device=dev, dtype=F32)
        call("commu_gemm_tn_bf16_batched", _p(dsk), ld_dsk, TB * ld_dsk, _p(qv2), HD, DH, _p(slabs), DH, ld_dsk * DH, TB,
             ld_dsk, DH, ns, H, tri_B, tri_M, _s())
        call("commu_reduce_slabs2d_f32", _p(drd), drd.stride(0), DH, _p(slabs), K, DH, ns, ld_dsk * DH, H, 0, 1.0 / c2, _s())
    if defer is None:
        drd_part()
    else:
        defer(drd_part)
    _bias_grads(dq if dq_colsum else None, du_part, du, dvb, HD, dev, defer, colsum_group)
    return delta


def _bias_grads(dq, du_part, du, dvb, HD, dev, defer, group=None):
    """d r_w_bias += colsum(dq_ac) ; d r_r_bias += colsum(dq) - colsum(dq_ac)   (gradients only: deferrable).
    du_part holds the per-query-tile column sums of dq_ac; three column-sum launches, no temporaries (group: one slab pass
    now, the three final passes in the step's grouped launch)."""
    def bias_part():
        if defer is not None:          # local scratch outlives the caller on the deferring stream
            du_part.record_stream(torch.cuda.current_stream())
        colsum(du_part, du, group=group)
        if dq is not None:
            colsum(dq, dvb, group=group)
        colsum(du_part, dvb, alpha=-1.0, group=group)
    if defer is None:
        bias_part()
    else:
        defer(bias_part)


def _sampling_control(x, name, dtype, nseq, device):
    """A sampling control of sample_topk as (scalar, device array or None): a number applies to every sequence, a tensor
    [nseq] gives each sequence its own value."""
    if not isinstance(x, torch.Tensor):
        return x, None
    if not x.is_cuda or x.device != device:
        raise CommuHipError(f"{name}: a per-sequence control lives on the device of the logits (no CPU fallback)")
    if x.dtype != dtype or x.dim() != 1 or x.numel() != nseq or not x.is_contiguous():
        raise CommuHipError(f"{name}: contiguous {str(dtype).replace('torch.', '')} [{nseq}] expected, got "
                            f"{str(x.dtype).replace('torch.', '')} {tuple(x.shape)}")
    return None, x


def _check_draw_state(kind, device, specs):
    """The device tensors of sample_topk's grammar= / harmony=: specs of (tensor, name, dtype, shape as text, shape test); a
    missing `on` means every sequence is on."""
    for t, name, dtype, shape, fits in specs:
        if t is None and name == "on":
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
            raise CommuHipError(f"{kind} {name}: a tensor on the device of the logits expected (no CPU fallback)")
        if not (t.dtype == dtype and t.is_contiguous() and fits(t)):
            raise CommuHipError(f"{kind} {name}: contiguous {str(dtype).replace('torch.', '')} {shape} expected, got "
                                f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)}")


def sample_topk(logits, temperature, top_k, wrong=None, uniforms=None, active=None, token=None, probs_out=None,
                top_p=1.0, logp_out=None, bias=None, V=729, grammar=None, harmony=None, class_ctl=None,
                note_order=None, voices=None, density=None, interval=None, onsets=None, guide=None, articulation=None):
    """In-place temperature + softmax + top-k + wrong-token mask + inverse-CDF draw per sequence.
    logits: fp32 [nseq, >=V] (row stride = ld), modified in place (logits[:, 1:V] /= temperature).
    top_p < 1: nucleus filter after the top-k / rejected-token step (an extra mode; the reference has top-k only).
    temperature / top_k / top_p: a number for all sequences, or a device tensor [nseq] (fp32 / int32 / fp32) with one
    value per sequence -- sequence b's result is that of the scalar call with b's values.  The values of a tensor are not
    checked here (generate.sampling_rows does that on the host); the kernel clamps top_k to [1, V].
    logp_out: fp32 [nseq, 2], receives per drawn token (full, kept) -- the log-softmax over ids 1 .. V-1 of the row the
    draw used at the drawn id, and the log of the token's probability in the distribution it was drawn from (0 for
    temperature 0); NaN, NaN where nothing could be drawn; untouched where active[b] == 0.
    bias: fp32 [nseq, >=V] on the device of the logits (row stride = ld_bias), a constraint per sequence: the distribution
    is built from logits / temperature + bias (the raw row + bias for temperature 0) -- a finite entry re-weights an id,
    -inf bans it, before top-k.  It is never written back: the logits are left as the call without it leaves them
    (commu_sample_args.bias; generate.token_constraints builds and validates such rows).
    V: the ids drawn from are 1 .. V-1 (2 <= V <= 768; the decode loop's vocabulary by default).
    grammar: (table, on, state, seq) on the device of the logits -- table fp32 [8, >=V] (generate.grammar_table), on uint8
    [nseq] or None (all on), state the int32 forcing records [nseq, commu_forcing_state_ints()], seq int32 [nseq, ld_seq].
    Row c of the table is added after the bias for a sequence whose previous token seq[b][state[b][0] - 1] has class c
    (generate.token_class), row 7 for a sequence that is off; like the bias it is never written back
    (commu_sample_args.gram).
    harmony: (table, on, state, chord_tok) on the device of the logits -- table fp32 [111, >= 12] (generate.harmony_rows), on
    uint8 [nseq] or None (all on), state as above, chord_tok int32 [nseq, ld_chord]: the chords the forcing rules place.
    For the pitch ids 3 .. 130 table[r][(id - 3) mod 12] is added after the grammar row, r = chord_tok[b][state[b][F_CUR] - 1]
    - 195 (109 while F_CUR is 0, 110 for a sequence that is off); no other id is touched and nothing is written back.  One
    kernel serves it, with a bias and a grammar: where the call has none, a zero bias and an all-off grammar are made
    here (x + 0 and the zero row 7 change no bit) (commu_sample_args.harm).
    class_ctl: (records, state, seq) on the device of the logits -- records int32 [nseq, 8, 4], the bit patterns of
    {float temperature; int top_k; float top_p; int 0} per class (generate.class_ctl_records), state and seq as the grammar's.
    Sequence b draws with the triple of record token_class(seq[b][state[b][0] - 1]); temperature / top_k / top_p given
    here are not looked at.  One kernel serves it, the harmony kernel's with the records: where the call has no bias,
    grammar or harmony, a zero bias and all-off tables are made here (commu_sample_args.cls_ctl).
    note_order: int32 [nseq] on the device of the logits, one control word per sequence (generate.note_order_ctl): -1 off,
    0 on, n >= 1 on with at most n notes per position.  A sequence that is on cannot draw a position before the one it
    is at, a pitch its current position already holds, or (n >= 1) the position itself once it holds n notes; the bans
    are read off seq[b][0 : state[b][0]] and replace y by -inf after the harmony term.  One kernel serves it, the class
    kernel's with the scan: class_ctl= is required (a call without class controls passes records that all hold the
    sequence's triple, generate.class_ctl_records) (commu_sample_args.order_ctl).
    voices: int32 [nseq] on the device of the logits, one control word per sequence (generate.voices_ctl): -1 off, else
    N + 256 r -- at most N notes of seq[b][0 : state[b][0]] may sound at the onset drawn next (N = 0: no cap), and with r = 1
    no pitch that still sounds may be drawn.  The bans join the note order's in the same select.  One kernel serves it, the
    note-order kernel's with the scan continued to the second BAR: note_order= is required
    (commu_sample_args.voice_ctl).
    density: int32 [nseq] on the device of the logits, one control word per sequence (generate.density_ctl): -1 off, else
    lo + 256 hi -- with C the complete notes of seq[b][0 : state[b][0]] behind its last BAR, every POSITION id is banned once
    C >= hi >= 1, and BAR and EOS while C < lo unless no position is left to draw.  The bans join the note order's and the
    voice cap's in the same select.  One kernel serves it, the voices kernel's with the count: voices= is required
    (commu_sample_args.density_ctl).
    interval: int32 [nseq] on the device of the logits, one control word per sequence (generate.interval_ctl): -1 off, else
    up + 256 down + 65536 u -- with q the PITCH token of the last note of seq[b][0 : state[b][0]] that at most one BAR follows,
    ids q + up + 1 .. 130 are banned (up >= 1), ids 3 .. q - down - 1 (down >= 1) and q itself (u = 1); no such note: nothing.
    The bans join the note order's, the voice cap's and the density's in the same select.  One kernel serves it, the
    density kernel's with the last note: density= is required (commu_sample_args.interval_ctl).
    onsets: (words, table) on the device of the logits -- words int32 [nseq], one control word per sequence
    (generate.onset_ctl): -1 off, else base + 4096 R; table int32 [rows, 4] contiguous, 1 <= rows <= 4096, the bit patterns of
    the uint32 template rows (generate.onset_rows): bit g % 32 of word g / 32 set means position id 432 + g may be drawn.  The
    row of the open bar is base + (max(nb - 1, 0) mod R) with nb = state[b][8], the record's count of BAR tokens in seq; every
    position id whose bit is clear is banned, in the same select as the four rules above, and the density's lower bound lets
    a bar end once the position range together with the row leaves no position.  One kernel serves it, the interval kernel's
    with the row: interval= is required (commu_sample_args.onset_ctl / onset_table / onset_rows).
    guide: (words, table) on the device of the logits -- words int32 [nseq], one control word per sequence: -1 off, else
    base + 65536 R + 2^23 s (generate.guide_word); table int32 [rows, 4] contiguous, 1 <= rows <= 65536, the bit patterns of
    the uint32 guide rows (generate.guide_rows): per bar a block of 1 + C rows, C = 128 >> s -- the live row over positions
    and C cell rows over pitches (bit k: id 3 + k).  The block of the open bar is base + (max(nb - 1, 0) mod R) (1 + C); with p
    the last BAR-or-POSITION token of seq, a POSITION, the cell row is block + 1 + ((p - 432) >> s) and every pitch id whose
    bit is clear is banned; every position id whose bit in the live row is clear is banned, and the density waiver sees the
    onset row ANDed with the live row.  Row indices are clamped into the table.  One kernel serves it, the onsets kernel's
    with the two rows: onsets= is required -- pass all -1 onset words over a one-row all-ones table where there is no
    template (commu_sample_args.guide_ctl / guide_table / guide_rows).
    articulation: (words, table) on the device of the logits -- words int32 [nseq], one control word per sequence: -1 off,
    else base + 4096 R + 2^19 w + 2^20 h (generate.articulation_word); table int32 [rows, 4] contiguous, 1 <= rows <= 4096,
    the bit patterns of the uint32 articulation rows (generate.articulation_rows): word 0 dlo | dhi << 8, words 1 and 2 the
    64-bit velocity mask (bit k: id 131 + k), word 3 reserved.  The row of the open bar is base + (max(nb - 1, 0) mod R);
    every velocity id whose bit is clear is banned, and of the duration ids 304 .. 431 those outside the window lo .. cap
    steps: cap is 128, dhi where set, 128 - a under w (a the step of the last BAR-or-POSITION token of seq, a POSITION) and,
    under h with the sequence's guide word on and the previous token a pitch, the first step ahead whose guide cell bans
    that pitch; lo = min(max(dlo, 1), cap).  Row indices are clamped into the tables.  One kernel serves it, the guide
    kernel's with the row and the hold term: guide= is required -- pass all -1 guide words over a one-row table where
    there is no guide (commu_sample_args.art_ctl / art_table / art_rows)."""
    nseq = logits.shape[0]
    V = int(V)
    assert logits.dtype == F32 and logits.stride(1) == 1
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or not bias.is_cuda or bias.device != logits.device:
            raise CommuHipError("bias: a tensor on the device of the logits expected (no CPU fallback)")
        if bias.dtype != F32 or bias.dim() != 2 or bias.shape[0] != nseq or bias.shape[1] < V:
            raise CommuHipError(f"bias: float32 [{nseq}, >= {V}] expected, got "
                                f"{str(bias.dtype).replace('torch.', '')} {tuple(bias.shape)}")
        if bias.stride(1) != 1 or (nseq > 1 and bias.stride(0) < V):
            raise CommuHipError(f"bias: rows of unit stride, at least {V} elements apart, expected; got strides "
                                f"{tuple(bias.stride())}")
    t_s, t_r = _sampling_control(temperature, "temperature", F32, nseq, logits.device)
    k_s, k_r = _sampling_control(top_k, "top_k", torch.int32, nseq, logits.device)
    p_s, p_r = _sampling_control(top_p, "top_p", F32, nseq, logits.device)
    if logp_out is not None:
        if not isinstance(logp_out, torch.Tensor) or not logp_out.is_cuda or logp_out.device != logits.device:
            raise CommuHipError("logp_out: a tensor on the device of the logits expected (no CPU fallback)")
        if logp_out.dtype != F32 or tuple(logp_out.shape) != (nseq, 2) or not logp_out.is_contiguous():
            raise CommuHipError(f"logp_out: contiguous float32 [{nseq}, 2] expected, got "
                                f"{str(logp_out.dtype).replace('torch.', '')} {tuple(logp_out.shape)}")
    if token is None:
        token = torch.empty(nseq, device=logits.device, dtype=torch.int32)
    a = _lib.struct_args(
        _lib.SampleArgs, logits=_p(logits), ld=logits.stride(0), nseq=nseq, V=V, wrong=_p(wrong),
        ldw=0 if wrong is None else wrong.stride(0), uniforms=_p(uniforms), active=_p(active),
        temperature=0.0 if t_s is None else float(t_s), top_k=1 if k_s is None else int(k_s),
        top_p=1.0 if p_s is None else float(p_s), temperature_rows=_p(t_r), top_k_rows=_p(k_r), top_p_rows=_p(p_r),
        token=_p(token), probs_out=_p(probs_out), ldp=0 if probs_out is None else probs_out.stride(0), logp_out=_p(logp_out))
    nrec = call("commu_forcing_state_ints") if grammar is not None or harmony is not None or class_ctl is not None else 0
    if class_ctl is not None:
        ctl, cstate, cseq = class_ctl
        _check_draw_state("class_ctl", logits.device, (
            (ctl, "records", torch.int32, "[%d, 8, 4]" % nseq, lambda t: tuple(t.shape) == (nseq, 8, 4)),
            (cstate, "state", torch.int32, "[%d, %d]" % (nseq, nrec), lambda t: tuple(t.shape) == (nseq, nrec)),
            (cseq, "seq", torch.int32, "[%d, ld_seq]" % nseq,
             lambda t: t.dim() == 2 and t.shape[0] == nseq and t.shape[1] >= 1)))
        for other, what in ((grammar, "grammar"), (harmony, "harmony")):
            if other is not None and (not isinstance(other[2], torch.Tensor) or other[2].data_ptr() != cstate.data_ptr()):
                raise CommuHipError(f"class_ctl state: the records the {what} reads expected (one state per sequence)")
        # (as for harmony below: the stand-alone sampler's convenience; ForcedDecoder passes its own buffers)
        if grammar is None:
            grammar = (torch.zeros(8, V, dtype=F32, device=logits.device),
                       torch.zeros(nseq, dtype=torch.uint8, device=logits.device), cstate, cseq)
        if harmony is None:
            harmony = (torch.zeros(111, 16, dtype=F32, device=logits.device),
                       torch.zeros(nseq, dtype=torch.uint8, device=logits.device), cstate,
                       torch.zeros(nseq, 1, dtype=torch.int32, device=logits.device))
        a.cls_ctl = _p(ctl)
    if note_order is not None:
        if class_ctl is None:
            raise CommuHipError("note_order: class_ctl= expected as well (the one kernel reads the class records; pass the "
                                "base-triple table where there are no class controls)")
        _check_draw_state("note_order", logits.device, (
            (note_order, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),))
        a.order_ctl = _p(note_order)
    if voices is not None:
        if note_order is None:
            raise CommuHipError("voices: note_order= expected as well (the one kernel continues the note order's scan; pass "
                                "words that are all -1 where the note order is off)")
        _check_draw_state("voices", logits.device, (
            (voices, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),))
        a.voice_ctl = _p(voices)
    if density is not None:
        if voices is None:
            raise CommuHipError("density: voices= expected as well (the one kernel counts on the voice cap's walk; pass words "
                                "that are all 0 where there is no cap)")
        _check_draw_state("density", logits.device, (
            (density, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),))
        a.density_ctl = _p(density)
    if interval is not None:
        if density is None:
            raise CommuHipError("interval: density= expected as well (the one kernel finds the last note on the density "
                                "kernel's walk; pass words that are all -1 where there is no density)")
        _check_draw_state("interval", logits.device, (
            (interval, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),))
        a.interval_ctl = _p(interval)
    if onsets is not None:
        if interval is None:
            raise CommuHipError("onsets: interval= expected as well (the one kernel is the interval kernel's with the template "
                                "row; pass words that are all -1 where there is no interval)")
        if not isinstance(onsets, (tuple, list)) or len(onsets) != 2:
            raise CommuHipError("onsets: a pair (control words int32 [nseq], table int32 [rows, 4]) expected")
        owords, otable = onsets
        _check_draw_state("onsets", logits.device, (
            (owords, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),
            (otable, "table", torch.int32, "[1 .. 4096, 4]",
             lambda t: t.dim() == 2 and 1 <= t.shape[0] <= 4096 and t.shape[1] == 4)))
        a.onset_ctl, a.onset_table, a.onset_rows = _p(owords), _p(otable), int(otable.shape[0])
    if guide is not None:
        if onsets is None:
            raise CommuHipError("guide: onsets= expected as well (the one kernel is the onsets kernel's with the guide's two "
                                "rows; pass words that are all -1 over a one-row all-ones table where there is no template)")
        if not isinstance(guide, (tuple, list)) or len(guide) != 2:
            raise CommuHipError("guide: a pair (control words int32 [nseq], table int32 [rows, 4]) expected")
        gwords, gtable = guide
        _check_draw_state("guide", logits.device, (
            (gwords, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),
            (gtable, "table", torch.int32, "[1 .. 65536, 4]",
             lambda t: t.dim() == 2 and 1 <= t.shape[0] <= 65536 and t.shape[1] == 4)))
        a.guide_ctl, a.guide_table, a.guide_rows = _p(gwords), _p(gtable), int(gtable.shape[0])
    if articulation is not None:
        if guide is None:
            raise CommuHipError("articulation: guide= expected as well (the one kernel is the guide kernel's with the row and "
                                "the hold term; pass words that are all -1 over a one-row table where there is no guide)")
        if not isinstance(articulation, (tuple, list)) or len(articulation) != 2:
            raise CommuHipError("articulation: a pair (control words int32 [nseq], table int32 [rows, 4]) expected")
        awords, atable = articulation
        _check_draw_state("articulation", logits.device, (
            (awords, "controls", torch.int32, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),
            (atable, "table", torch.int32, "[1 .. 4096, 4]",
             lambda t: t.dim() == 2 and 1 <= t.shape[0] <= 4096 and t.shape[1] == 4)))
        a.art_ctl, a.art_table, a.art_rows = _p(awords), _p(atable), int(atable.shape[0])
    if harmony is not None:
        htable, hon, hstate, chord_tok = harmony
        _check_draw_state("harmony", logits.device, (
            (htable, "table", F32, "[111, >= 12]", lambda t: t.dim() == 2 and t.shape[0] == 111 and t.shape[1] >= 12),
            (hon, "on", torch.uint8, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),
            (hstate, "state", torch.int32, "[%d, %d]" % (nseq, nrec), lambda t: tuple(t.shape) == (nseq, nrec)),
            (chord_tok, "chord_tok", torch.int32, "[%d, ld_chord]" % nseq,
             lambda t: t.dim() == 2 and t.shape[0] == nseq and t.shape[1] >= 1)))
        if grammar is not None and (not isinstance(grammar[2], torch.Tensor) or grammar[2].data_ptr() != hstate.data_ptr()):
            raise CommuHipError("harmony state: the records the grammar reads expected (one state per sequence)")
        # The one harmony kernel reads a bias and a grammar: a call without them gets a zero bias and an all-off grammar,
        # allocated per call.  That serves the stand-alone sampler (tests, probes); ForcedDecoder never takes these two
        # branches -- set_harmony allocates its buffers once and body() passes them.
        if grammar is None:
            grammar = (torch.zeros(8, V, dtype=F32, device=logits.device),
                       torch.zeros(nseq, dtype=torch.uint8, device=logits.device), hstate,
                       torch.zeros(nseq, 1, dtype=torch.int32, device=logits.device))
        if bias is None:
            bias = torch.zeros(nseq, V, dtype=F32, device=logits.device)
        a.harm, a.ld_harm, a.harm_on = _p(htable), htable.stride(0), _p(hon)
        a.chord_tok, a.ld_chord = _p(chord_tok), chord_tok.stride(0)
    if grammar is not None:
        table, on, state, seq = grammar
        _check_draw_state("grammar", logits.device, (
            (table, "table", F32, "[8, >= %d]" % V, lambda t: t.dim() == 2 and t.shape[0] == 8 and t.shape[1] >= V),
            (on, "on", torch.uint8, "[%d]" % nseq, lambda t: tuple(t.shape) == (nseq,)),
            (state, "state", torch.int32, "[%d, %d]" % (nseq, nrec), lambda t: tuple(t.shape) == (nseq, nrec)),
            (seq, "seq", torch.int32, "[%d, ld_seq]" % nseq,
             lambda t: t.dim() == 2 and t.shape[0] == nseq and t.shape[1] >= 1)))
        a.gram, a.ld_gram, a.gram_on = _p(table), table.stride(0), _p(on)
        a.state, a.seq, a.ld_seq = _p(state), _p(seq), seq.stride(0)
    if bias is not None:
        a.bias, a.ld_bias = _p(bias), max(int(bias.stride(0)), V)
    call("commu_sample_topk", C.byref(a), _s())
    return token


# ---------------------------------------------------------------------------------------------- fp32 parity mode
# (csrc/parity_f32.hip: the generation path on fp32 operands end to end -- the reference's arithmetic, train.py:48; its
#  LayerNorm is layernorm_fwd_f32(stats=False) below)
def _f32_2d(t, name):
    if not t.is_cuda:
        raise CommuHipError("commu_amd kernels need GPU tensors (no CPU fallback)")
    assert t.dtype == F32 and t.dim() == 2 and t.stride(1) == 1, f"{name}: fp32 row-major 2-D tensor expected"
    return t.stride(0)


def gemm_nt_f32(A, B, out=None, bias=None, resid=None, relu=False):
    """out fp32 [M, N] = A [M, K] . B [N, K]^T (+ bias) (ReLU) (+ resid): nn.Linear in fp32."""
    lda, ldb = _f32_2d(A, "A"), _f32_2d(B, "B")
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=F32)
    ldc = _f32_2d(out, "out")
    assert out.shape == (M, N)
    if bias is not None:
        assert bias.dtype == F32 and bias.is_contiguous() and bias.numel() >= N
    ldr = 0 if resid is None else _f32_2d(resid, "resid")
    call("commu_gemm_nt_f32", _p(A), lda, _p(B), ldb, _p(out), ldc, M, N, K, _p(bias), _p(resid), ldr, 1 if relu else 0, _s())
    return out


def embed_f32(tok, E, out=None):
    """model.py:409-420: E[tok] * sqrt(d_model), fp32."""
    if not tok.is_cuda:
        raise CommuHipError("commu_amd kernels need GPU tensors (no CPU fallback)")
    tok = tok.contiguous().view(-1)
    assert tok.dtype == torch.long and E.dtype == F32 and E.is_contiguous()
    rows, D = tok.numel(), E.shape[1]
    if out is None:
        out = torch.empty(rows, D, device=E.device, dtype=F32)
    call("commu_embed_f32", _p(tok), _p(E), _p(out), _f32_2d(out, "out"), rows, D, math.sqrt(D), _s())
    return out


def posemb_f32(inv_freq, n, D, out=None, clamp_len=-1):
    """model.py:142-147 by distance: row d = [sin(p * inv_freq) | cos(p * inv_freq)], p = d or min(d, clamp_len)."""
    if out is None:
        out = torch.empty(n, D, device=inv_freq.device, dtype=F32)
    assert inv_freq.dtype == F32 and inv_freq.numel() == D // 2
    call("commu_posemb_f32", _p(inv_freq), _p(out), _f32_2d(out, "out"), n, D, int(clamp_len), _s())
    return out


def relattn_f32(q, k, v, stride_key, stride_seq, rd, u, vb, T, M, B, H, DH, same_length, mem_len, scale, klen=None,
                reset=None, out=None):
    """model.py:283-345 in fp32 (see include/commu_hip.h, commu_relattn_f32).  q: 2-D view [T*B, >= H*DH]; k, v: tensors whose
    data pointer is element (key 0, sequence 0, head 0, 0); rd [>= max distance + 1, >= H*DH]."""
    ld_q = _f32_2d(q, "q")
    ld_rd = _f32_2d(rd, "rd")
    assert k.dtype == F32 and v.dtype == F32 and u.dtype == F32 and vb.dtype == F32
    if out is None:
        out = torch.empty(T * B, H * DH, device=q.device, dtype=F32)
    call("commu_relattn_f32", _p(q), ld_q, _p(k), _p(v), int(stride_key), int(stride_seq), _p(rd), ld_rd, _p(u), _p(vb),
         _p(klen), _p(reset), _p(out), _f32_2d(out, "out"), T, M, B, H, DH, 1 if same_length else 0, int(mem_len), float(scale),
         _s())
    return out


def decode_kv_append_f32(qkv, kc, vc, klen, active, HD, Lmax):
    call("commu_decode_kv_append_f32", _p(qkv), _f32_2d(qkv, "qkv"), _p(kc), _p(vc), _p(klen), _p(active), qkv.shape[0], HD,
         Lmax, _s())


# ---------------------------------------------------------------------------------------------- sliding decode memory
# (the cached decode step on a ring of W = memory_length + 1 rows: include/commu_hip.h, commu_decode_attn_ring)
RING_MAX_ROWS = 4224          # DEC_MAXK of csrc/decode.hip: the score row of a (sequence, head) pair lives in LDS


def _ring_args(cache_k, cache_v, klen, active, B, dtype, shape):
    for t, name in ((cache_k, "kc"), (cache_v, "vc"), (klen, "klen")) + (() if active is None else ((active, "active"),)):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
    for t, name in ((cache_k, "kc"), (cache_v, "vc")):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise CommuHipError(f"{name}: contiguous {dtype} ring cache of shape {shape} expected, got {t.dtype} "
                                f"{tuple(t.shape)}")
    if klen.dtype != torch.int32 or klen.numel() != B or not klen.is_contiguous():
        raise CommuHipError(f"klen: contiguous int32 [{B}] expected")
    if active is not None and (active.dtype != torch.uint8 or active.numel() != B or not active.is_contiguous()):
        raise CommuHipError(f"active: contiguous uint8 [{B}] expected")


def _ring_rows(W):
    W = int(W)
    if W < 2 or W > RING_MAX_ROWS:
        raise CommuHipError(f"ring of {W} rows requested; the decode attention supports 2 .. {RING_MAX_ROWS} "
                            "(memory_length + 1)")
    return W


def decode_kv_append_ring(qkv, kc, vc, klen, active, W):
    """K and V of the new tokens (columns [HD, 3 HD) of qkv, bf16 [B, 3 HD]) into ring row klen[b] mod W of the caches
    kc / vc bf16 [B, H, W, DH], sequences with active[b] != 0 (None: all)."""
    W = _ring_rows(W)
    if kc.dim() != 4:
        raise CommuHipError("kc: [B, H, W, DH] expected")
    B, H, _, DH = kc.shape
    _ring_args(kc, vc, klen, active, B, BF16, (B, H, W, DH))
    if not qkv.is_cuda:
        raise CommuHipError("qkv: commu_amd kernels need GPU tensors (no CPU fallback)")
    if qkv.dtype != BF16 or qkv.dim() != 2 or qkv.shape != (B, 3 * H * DH) or qkv.stride(1) != 1 or qkv.stride(0) % 8:
        raise CommuHipError(f"qkv: bf16 [{B}, {3 * H * DH}] with a row stride that is a multiple of 8 expected")
    call("commu_decode_kv_append_ring", _p(qkv), qkv.stride(0), _p(kc), _p(vc), _p(klen), _p(active), B, W, H, H * DH, _s())


def decode_attn_ring(qkv, kc, vc, rd, u, vb, klen, active, out, W, scale, append=True, same_length=False, nsplit=1,
                     split_ws=None, split_cnt=None):
    """Cached single-token attention over the ring caches kc / vc bf16 [B, H, W, DH] (commu_decode_attn_ring): klen int32
    [B] counts absolute positions, rd bf16 [>= W, >= H DH] is the distance table, out bf16 [B, H DH].  append: the new
    token's K/V are written to row klen[b] mod W by the kernel itself.  nsplit > 1: split_ws fp32 [>= B H nsplit (DH + 2)],
    split_cnt int32 [>= B H] zeroed once."""
    W = _ring_rows(W)
    if kc.dim() != 4:
        raise CommuHipError("kc: [B, H, W, DH] expected")
    B, H, _, DH = kc.shape
    if DH not in (32, 64):
        raise CommuHipError(f"d_head {DH}: the decode attention is built for 32 and 64 (pad the model's head)")
    _ring_args(kc, vc, klen, active, B, BF16, (B, H, W, DH))
    HD = H * DH
    for t, name in ((qkv, "qkv"), (rd, "rd"), (out, "out"), (u, "r_w_bias"), (vb, "r_r_bias")):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
    if qkv.dtype != BF16 or qkv.dim() != 2 or qkv.shape != (B, 3 * HD) or qkv.stride(1) != 1 or qkv.stride(0) % 8:
        raise CommuHipError(f"qkv: bf16 [{B}, {3 * HD}] with a row stride that is a multiple of 8 expected")
    if rd.dtype != BF16 or rd.dim() != 2 or rd.shape[0] < W or rd.shape[1] < HD or rd.stride(1) != 1 or rd.stride(0) % 8:
        raise CommuHipError(f"rd: bf16 [>= {W}, >= {HD}] with a row stride that is a multiple of 8 expected")
    if out.dtype != BF16 or out.dim() != 2 or out.shape != (B, HD) or out.stride(1) != 1:
        raise CommuHipError(f"out: bf16 [{B}, {HD}] expected")
    for t, name in ((u, "r_w_bias"), (vb, "r_r_bias")):
        if t.dtype != F32 or t.numel() < HD or not t.is_contiguous():
            raise CommuHipError(f"{name}: contiguous fp32 [>= {HD}] expected")
    nsplit = int(nsplit)
    if nsplit < 1 or nsplit > 16:
        raise CommuHipError("nsplit: 1 .. 16")
    if nsplit > 1:
        if split_ws is None or split_cnt is None or not split_ws.is_cuda or not split_cnt.is_cuda:
            raise CommuHipError("nsplit > 1 needs split_ws and split_cnt on the GPU")
        if split_ws.dtype != F32 or split_ws.numel() < B * H * nsplit * (DH + 2) or split_cnt.dtype != torch.int32 \
                or split_cnt.numel() < B * H:
            raise CommuHipError("split_ws: fp32 [>= B H nsplit (DH + 2)], split_cnt: int32 [>= B H]")
    call("commu_decode_attn_ring", _p(qkv), qkv.stride(0), _p(kc), _p(vc), _p(rd), rd.stride(0), _p(u), _p(vb), _p(klen),
         _p(active), _p(out), out.stride(0), B, H, DH, W, float(scale), 1 if append else 0, 1 if same_length else 0, nsplit,
         _p(split_ws) if nsplit > 1 else None, _p(split_cnt) if nsplit > 1 else None, _s())
    return out


def decode_kv_append_ring_f32(qkv, kc, vc, klen, active, HD, W):
    """fp32 parity mode: the new tokens' K / V into ring row klen[b] mod W of kc / vc fp32 [B, W, HD]."""
    W = _ring_rows(W)
    ld = _f32_2d(qkv, "qkv")
    B = qkv.shape[0]
    if qkv.shape[1] != 3 * HD:
        raise CommuHipError(f"qkv: fp32 [{B}, {3 * HD}] expected")
    _ring_args(kc, vc, klen, active, B, F32, (B, W, HD))
    call("commu_decode_kv_append_ring_f32", _p(qkv), ld, _p(kc), _p(vc), _p(klen), _p(active), B, HD, W, _s())


def decode_attn_ring_f32(q, kc, vc, rd, u, vb, klen, H, DH, W, same_length, scale, out=None):
    """fp32 parity mode: the cached single-token attention over the ring caches kc / vc fp32 [B, W, H DH]
    (commu_decode_attn_ring_f32).  q: 2-D view [B, >= H DH] of the new tokens' projections; rd fp32 [>= W, >= H DH]."""
    W = _ring_rows(W)
    ld_q = _f32_2d(q, "q")
    ld_rd = _f32_2d(rd, "rd")
    B, HD = q.shape[0], H * DH
    if DH < 1 or DH > 64 or q.shape[1] < HD:
        raise CommuHipError(f"q: fp32 [{B}, >= {HD}] with d_head <= 64 expected")
    _ring_args(kc, vc, klen, None, B, F32, (B, W, HD))
    if rd.shape[0] < W or rd.shape[1] < HD:
        raise CommuHipError(f"rd: fp32 [>= {W}, >= {HD}] expected")
    for t, name in ((u, "r_w_bias"), (vb, "r_r_bias")):
        if not t.is_cuda or t.dtype != F32 or t.numel() < HD or not t.is_contiguous():
            raise CommuHipError(f"{name}: contiguous fp32 [>= {HD}] on the GPU expected")
    if out is None:
        out = torch.empty(B, HD, device=q.device, dtype=F32)
    ld_o = _f32_2d(out, "out")
    if out.shape != (B, HD):
        raise CommuHipError(f"out: fp32 [{B}, {HD}] expected")
    call("commu_decode_attn_ring_f32", _p(q), ld_q, _p(kc), _p(vc), _p(rd), ld_rd, _p(u), _p(vb), _p(klen), _p(out), ld_o, B, H,
         DH, W, 1 if same_length else 0, float(scale), _s())
    return out


# ---------------------------------------------------------------------------------------------- fp32 training mode
# (csrc/train_f32.hip: model.fp32_training -- the backward pass and the dropout forward in the reference's arithmetic)
def f32_slabs(M, N, K):
    """Row split of a long contraction (commu_gemm_f32 nslabs): a function of the shape only, so the summation order and
    the result are the same on every call.  Slabs of >= 1024 rows until the grid has ~1024 workgroups."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    if K < 4096 or tiles >= 1024:
        return 1
    return max(1, min(K // 1024, 1024 // tiles, 128))


def gemm_f32(A, B, out=None, *, ta=False, tb=True, bias=None, relu=False, drop_p=0.0, drop_seed=0, resid=None,
             accumulate=False, slabs=None):
    """out [M, N] (+)= op(A) . op(B) in fp32 (commu_gemm_f32): ta -> A is stored [K, M]; tb -> B is stored [N, K] (nn.Linear).
    NT (ta=False, tb=True) = Linear forward, NN (tb=False) = dX, TN (ta=True, tb=False) = dW.  slabs: None = f32_slabs."""
    lda, ldb = _f32_2d(A, "A"), _f32_2d(B, "B")
    M, K = (A.shape[1], A.shape[0]) if ta else A.shape
    N, Kb = B.shape if tb else (B.shape[1], B.shape[0])
    assert Kb == K, (A.shape, B.shape, ta, tb)
    if out is None:
        assert not accumulate
        out = torch.empty(M, N, device=A.device, dtype=F32)
    ldc = _f32_2d(out, "out")
    assert tuple(out.shape) == (M, N)
    if bias is not None:
        assert bias.dtype == F32 and bias.is_contiguous() and bias.numel() >= N
    ldr = 0 if resid is None else _f32_2d(resid, "resid")
    epi = bias is not None or relu or drop_p > 0 or resid is not None
    ns = 1 if epi or ldc != N else (f32_slabs(M, N, K) if slabs is None else int(slabs))
    ws = torch.empty(ns * M * N, device=A.device, dtype=F32) if ns > 1 else None
    call("commu_gemm_f32", 1 if ta else 0, 1 if tb else 0, _p(A), lda, _p(B), ldb, _p(out), ldc, M, N, K, _p(bias),
         1 if relu else 0, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(resid), ldr, 1 if accumulate else 0, _p(ws), ns, _s())
    return out


def colsum_f32(X, out, ones):
    """out [N] += column sums of X [rows, N] (a bias gradient), deterministic: the TN GEMM of a ones vector (row split in order)."""
    gemm_f32(ones[:X.shape[0]].view(-1, 1), X, out.view(1, -1), ta=True, tb=False, accumulate=True)
    return out


def relattn_fwd_f32(q, k, v, rd, u, vb, reset, T, M, B, H, DH, same_length, mem_len, scale, drop_p=0.0, drop_seed=0,
                    out=None):
    """model.py:283-345 in train mode (commu_relattn_fwd_f32): q [T*B, >= H*DH] view, k / v [K*B, >= H*DH] views with a common
    leading dimension, rd [K, >= H*DH].  Returns (out [T*B, H*DH], lse [B, H, T])."""
    ld_q, ld_kv, ld_rd = _f32_2d(q, "q"), _f32_2d(k, "k"), _f32_2d(rd, "rd")
    assert _f32_2d(v, "v") == ld_kv and k.shape[0] == v.shape[0] == (T + M) * B and rd.shape[0] >= T + M
    assert u.dtype == F32 and vb.dtype == F32 and u.numel() >= H * DH and vb.numel() >= H * DH
    if out is None:
        out = torch.empty(T * B, H * DH, device=q.device, dtype=F32)
    lse = torch.empty(B, H, T, device=q.device, dtype=F32)
    call("commu_relattn_fwd_f32", _p(q), ld_q, _p(k), _p(v), ld_kv, _p(rd), ld_rd, _p(u), _p(vb), _p(reset), _p(out),
         _f32_2d(out, "out"), _p(lse), T, M, B, H, DH, 1 if same_length else 0, int(mem_len), float(scale), float(drop_p),
         int(drop_seed) & 0xFFFFFFFF, _s())
    return out, lse


def relattn_bwd_f32(q, k, v, rd, u, vb, reset, o, dout, lse, T, M, B, H, DH, same_length, mem_len, scale, dq, dk, dv, drd,
                    drop_p=0.0, drop_seed=0):
    """Backward of relattn_fwd_f32 (commu_relattn_bwd_f32): writes dq [T*B, >= H*DH], dk / dv [K*B, >= H*DH] (common leading
    dimension), drd [K, >= H*DH]; returns (dq_ac, dq_bd) [T*B, H*DH] -- their column sums are the r_w_bias / r_r_bias
    gradients."""
    ld_q, ld_kv, ld_rd = _f32_2d(q, "q"), _f32_2d(k, "k"), _f32_2d(rd, "rd")
    assert _f32_2d(v, "v") == ld_kv and _f32_2d(dv, "dv") == _f32_2d(dk, "dk")
    assert dk.shape[0] == (T + M) * B and drd.shape[0] >= T + M and lse.numel() == B * H * T
    dev = q.device
    delta = torch.empty(B * H * T, device=dev, dtype=F32)
    dq_ac = torch.empty(T * B, H * DH, device=dev, dtype=F32)
    dq_bd = torch.empty(T * B, H * DH, device=dev, dtype=F32)
    call("commu_relattn_bwd_f32", _p(q), ld_q, _p(k), _p(v), ld_kv, _p(rd), ld_rd, _p(u), _p(vb), _p(reset), _p(o),
         _f32_2d(o, "o"), _p(dout), _f32_2d(dout, "dout"), _p(lse), _p(delta), _p(dq), _f32_2d(dq, "dq"), _p(dq_ac), _p(dq_bd),
         _p(dk), _p(dv), _f32_2d(dk, "dk"), _p(drd), _f32_2d(drd, "drd"), T, M, B, H, DH, 1 if same_length else 0, int(mem_len),
         float(scale), float(drop_p), int(drop_seed) & 0xFFFFFFFF, _s())
    return dq_ac, dq_bd


def layernorm_fwd_f32(x, gamma, beta, eps=1e-5, out=None, stats=True):
    """nn.LayerNorm in fp32: (out, mean, rstd), the statistics saved for the backward; stats=False: (out, None, None), nothing
    allocated beside out (the forward-only callers; the decode step passes static buffers under graph capture)."""
    ldx = _f32_2d(x, "x")
    rows, D = x.shape
    if out is None:
        out = torch.empty(rows, D, device=x.device, dtype=F32)
    mean = torch.empty(rows, device=x.device, dtype=F32) if stats else None
    rstd = torch.empty(rows, device=x.device, dtype=F32) if stats else None
    assert gamma.dtype == F32 and beta.dtype == F32 and gamma.numel() == D
    call("commu_layernorm_fwd_f32", _p(x), ldx, _p(gamma), _p(beta), _p(out), _f32_2d(out, "out"), _p(mean), _p(rstd), rows, D,
         float(eps), _s())
    return out, mean, rstd


def ln_f32_blocks(rows):
    """Blocks of the LayerNorm backward's partial parameter sums (a function of the row count only: fixed summation order)."""
    return max(1, min(512, (rows + 31) // 32))


def layernorm_bwd_f32(dy, x, mean, rstd, gamma, dgamma=None, dbeta=None, add=None, dx=None):
    """dx of nn.LayerNorm from dy (+ add, the residual branch's gradient); dgamma / dbeta (optional) += their gradients."""
    rows, D = x.shape
    if dx is None:
        dx = torch.empty(rows, D, device=x.device, dtype=F32)
    nblk = ln_f32_blocks(rows)
    part = torch.empty(2 * nblk * D, device=x.device, dtype=F32)
    call("commu_layernorm_bwd_f32", _p(dy), _f32_2d(dy, "dy"), _p(add), 0 if add is None else _f32_2d(add, "add"), _p(x),
         _f32_2d(x, "x"), _p(mean), _p(rstd), _p(gamma), _p(dx), _f32_2d(dx, "dx"), _p(part), nblk, _p(dgamma), _p(dbeta), rows,
         D, _s())
    return dx


def ce_bwd_f32(logits, target, lse, g, V):
    """fp32 dlogits [rows, V] of the per-token NLL (ce_fwd's lse), weighted by g [rows]."""
    rows = logits.shape[0]
    dl = torch.empty(rows, V, device=logits.device, dtype=F32)
    call("commu_ce_bwd_f32", _p(logits), _f32_2d(logits, "logits"), _p(target), _p(lse), _p(g), _p(dl), V, rows, V, _s())
    return dl


def ce_bwd_opts_f32(logits, target, lse, g, V, label_smoothing=0.0, z_loss=0.0, dlogits=None):
    """fp32 dlogits [rows, V] of ce_fwd_opts' loss, weighted by g [rows] (dlogits given: columns [V, stride) are zeroed)."""
    rows = logits.shape[0]
    if dlogits is None:
        dlogits = torch.empty(rows, V, device=logits.device, dtype=F32)
    call("commu_ce_bwd_opts_f32", _p(logits), _f32_2d(logits, "logits"), _p(target), _p(lse), _p(g), _p(dlogits),
         _f32_2d(dlogits, "dlogits"), rows, V, float(label_smoothing), float(z_loss), _s())
    return dlogits


def ce_fwd_opts_f32(logits, target, V, label_smoothing=0.0, z_loss=0.0):
    """ce_fwd_opts under the fp32 schedule's entry point (its logits are fp32 like the bf16 schedule's: the same kernels)."""
    return ce_fwd_opts(logits, target, V, label_smoothing, z_loss, entry="commu_ce_fwd_opts_f32")


def embed_bwd_f32(tok, dx, gE, scale, drop_p=0.0, drop_seed=0, order=None):
    """gE [V, D] += scale * (dropout-backward of dx) scattered by token, deterministic (token-sorted rows)."""
    V, D = gE.shape
    perm, offs = token_order(tok, V) if order is None else order
    assert gE.is_contiguous() and dx.shape[1] == D
    call("commu_embed_bwd_f32", _p(perm), _p(offs), _p(dx), _f32_2d(dx, "dx"), _p(gE), V, D, float(scale), float(drop_p),
         int(drop_seed) & 0xFFFFFFFF, _s())
    return gE


def dropout_f32(x, drop_p=0.0, drop_seed=0, gate=None, out=None):
    """x * keep / (1 - p) with the element-wise site mask (index over x's [rows, cols]), 0 where gate <= 0; out may be x."""
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, cols, device=x.device, dtype=F32)
    call("commu_dropout_f32", _p(x), _f32_2d(x, "x"), _p(gate), 0 if gate is None else _f32_2d(gate, "gate"), _p(out),
         _f32_2d(out, "out"), rows, cols, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _s())
    return out


def _i32_rows(t, n, name):
    if t is not None and (not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous()):
        raise CommuHipError(f"{name}: contiguous int32 [{n}] on the GPU expected")


def decode_prefill_scatter(qkv, T, kc, vc, klen, lens, slots=None, window=0):
    """Ragged prefill of one layer's K/V caches (commu_decode_prefill_scatter / _f32): qkv is the layer's time-major
    projection buffer [T * B, >= 3 H DH] (row t * B + b) of a memory-less forward over B padded contexts; positions
    max(0, lens[b] - window) <= t < lens[b] go to the rows of slot slots[b] (None: b) of kc / vc -- bf16 [Bc, H, Lmax, DH]
    with DH 32 or 64, or the fp32 parity layout [Bc, Lmax, H DH] -- linear (window 0) or ring (Lmax = window + 1) --,
    and klen[slots[b]] = lens[b].  lens / slots / klen: int32 device arrays.  Host-side checks only of what is known on
    the host: the kernel clamps lens to [0, T] and skips slots outside the cache."""
    for t, name in ((qkv, "qkv"), (kc, "kc"), (vc, "vc"), (klen, "klen"), (lens, "lens")):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
    T, window = int(T), int(window)
    if qkv.dim() != 2 or T < 1 or qkv.shape[0] % T or qkv.stride(1) != 1:
        raise CommuHipError(f"qkv: 2-D [T * B, >= 3 H DH] with T = {T} expected, got {tuple(qkv.shape)}")
    B = qkv.shape[0] // T
    if kc.shape != vc.shape or kc.dtype != vc.dtype or not kc.is_contiguous() or not vc.is_contiguous():
        raise CommuHipError("kc / vc: two contiguous caches of one shape and dtype expected")
    Bc = kc.shape[0]
    _i32_rows(lens, B, "lens")
    _i32_rows(slots, B, "slots")
    _i32_rows(klen, Bc, "klen")
    if slots is None and B > Bc:
        raise CommuHipError(f"{B} contexts for a cache of {Bc} slots")
    if qkv.dtype == BF16 and kc.dtype == BF16 and kc.dim() == 4:
        _, H, Lmax, DH = kc.shape
        if DH not in (32, 64):
            raise CommuHipError(f"d_head {DH}: the decode caches are built for 32 and 64 (pad the model's head)")
        HD = H * DH
    elif qkv.dtype == F32 and kc.dtype == F32 and kc.dim() == 3:
        _, Lmax, HD = kc.shape
        H = DH = None
    else:
        raise CommuHipError("qkv / caches: bf16 with [Bc, H, Lmax, DH] caches, or fp32 with [Bc, Lmax, H DH] caches expected")
    if qkv.shape[1] < 3 * HD:
        raise CommuHipError(f"qkv: at least {3 * HD} columns expected, got {qkv.shape[1]}")
    if window < 0 or (window > 0 and Lmax != window + 1):
        raise CommuHipError(f"a ring of window {window} has {window + 1} rows; the caches have {Lmax}")
    if H is not None:
        if qkv.stride(0) % 8:
            raise CommuHipError("qkv: a row stride that is a multiple of 8 expected")
        call("commu_decode_prefill_scatter", _p(qkv), qkv.stride(0), T, B, _p(kc), _p(vc), _p(klen), _p(lens), _p(slots), Bc,
             H, DH, Lmax, window, _s())
    else:
        call("commu_decode_prefill_scatter_f32", _p(qkv), qkv.stride(0), T, B, _p(kc), _p(vc), _p(klen), _p(lens), _p(slots),
             Bc, HD, Lmax, window, _s())


# ---------------------------------------------------------------------------------------------- fp8 K/V cache (opt-in)
# (include/commu_hip.h, commu_decode_attn_kv8: e4m3 bytes [B, H, Lmax, DH] + one E8M0 scale byte per 32 features)
def _kv8_caches(kc8, vc8, ks, vs):
    """(B, H, Lmax, DH) of the four byte tensors of one layer's fp8 K/V cache, checked."""
    for t, name in ((kc8, "kc8"), (vc8, "vc8"), (ks, "ks"), (vs, "vs")):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
        if t.dtype != torch.uint8 or t.dim() != 4 or not t.is_contiguous():
            raise CommuHipError(f"{name}: contiguous uint8 [B, H, Lmax, ...] expected, got {t.dtype} {tuple(t.shape)}")
    B, H, Lmax, DH = kc8.shape
    if DH not in (32, 64):
        raise CommuHipError(f"d_head {DH}: the decode caches are built for 32 and 64 (pad the model's head)")
    if vc8.shape != kc8.shape:
        raise CommuHipError(f"vc8: {tuple(kc8.shape)} like kc8 expected, got {tuple(vc8.shape)}")
    for t, name in ((ks, "ks"), (vs, "vs")):
        if tuple(t.shape) != (B, H, Lmax, DH // 32):
            raise CommuHipError(f"{name}: scale bytes [{B}, {H}, {Lmax}, {DH // 32}] expected, got {tuple(t.shape)}")
    return B, H, Lmax, DH


def decode_attn_kv8(qkv, kc8, vc8, ks, vs, rd, u, vb, klen, active, out, scale, append=True, ring=False, same_length=False,
                    nsplit=1, split_ws=None, split_cnt=None):
    """Cached single-token attention over an fp8 K/V cache (commu_decode_attn_kv8): kc8 / vc8 uint8 [B, H, Lmax, DH] (e4m3
    bytes), ks / vs uint8 [B, H, Lmax, DH / 32] (E8M0 scale bytes); qkv bf16 [B, 3 H DH], rd bf16 [>= Lmax, >= H DH], out
    bf16 [B, H DH], klen int32 [B].  ring: the caches are rings of Lmax = memory_length + 1 rows and klen counts absolute
    positions (same_length hides the oldest row of a full ring); otherwise linear.  append: the kernel quantises the new
    token's K/V into its row and attends to that image.  nsplit > 1: split_ws fp32 [>= B H nsplit (DH + 2)], split_cnt
    int32 [>= B H] zeroed once."""
    B, H, Lmax, DH = _kv8_caches(kc8, vc8, ks, vs)
    if ring:
        _ring_rows(Lmax)
    elif Lmax < 1 or Lmax > RING_MAX_ROWS:
        raise CommuHipError(f"decode cache of {Lmax} positions; the decode attention supports 1 .. {RING_MAX_ROWS}")
    HD = H * DH
    for t, name in ((qkv, "qkv"), (rd, "rd"), (out, "out"), (u, "r_w_bias"), (vb, "r_r_bias"), (klen, "klen")) \
            + (() if active is None else ((active, "active"),)):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
    if klen.dtype != torch.int32 or klen.numel() != B or not klen.is_contiguous():
        raise CommuHipError(f"klen: contiguous int32 [{B}] expected")
    if active is not None and (active.dtype != torch.uint8 or active.numel() != B or not active.is_contiguous()):
        raise CommuHipError(f"active: contiguous uint8 [{B}] expected")
    if qkv.dtype != BF16 or qkv.dim() != 2 or qkv.shape != (B, 3 * HD) or qkv.stride(1) != 1 or qkv.stride(0) % 8:
        raise CommuHipError(f"qkv: bf16 [{B}, {3 * HD}] with a row stride that is a multiple of 8 expected")
    if rd.dtype != BF16 or rd.dim() != 2 or rd.shape[0] < Lmax or rd.shape[1] < HD or rd.stride(1) != 1 or rd.stride(0) % 8:
        raise CommuHipError(f"rd: bf16 [>= {Lmax}, >= {HD}] with a row stride that is a multiple of 8 expected")
    if out.dtype != BF16 or out.dim() != 2 or out.shape != (B, HD) or out.stride(1) != 1:
        raise CommuHipError(f"out: bf16 [{B}, {HD}] expected")
    for t, name in ((u, "r_w_bias"), (vb, "r_r_bias")):
        if t.dtype != F32 or t.numel() < HD or not t.is_contiguous():
            raise CommuHipError(f"{name}: contiguous fp32 [>= {HD}] expected")
    nsplit = int(nsplit)
    if nsplit < 1 or nsplit > 16:
        raise CommuHipError("nsplit: 1 .. 16")
    if nsplit > 1:
        if split_ws is None or split_cnt is None or not split_ws.is_cuda or not split_cnt.is_cuda:
            raise CommuHipError("nsplit > 1 needs split_ws and split_cnt on the GPU")
        if split_ws.dtype != F32 or split_ws.numel() < B * H * nsplit * (DH + 2) or split_cnt.dtype != torch.int32 \
                or split_cnt.numel() < B * H:
            raise CommuHipError("split_ws: fp32 [>= B H nsplit (DH + 2)], split_cnt: int32 [>= B H]")
    call("commu_decode_attn_kv8", _p(qkv), qkv.stride(0), _p(kc8), _p(vc8), _p(ks), _p(vs), _p(rd), rd.stride(0), _p(u),
         _p(vb), _p(klen), _p(active), _p(out), out.stride(0), B, H, DH, Lmax, float(scale), 1 if append else 0,
         1 if ring else 0, 1 if same_length else 0, nsplit, _p(split_ws) if nsplit > 1 else None,
         _p(split_cnt) if nsplit > 1 else None, _s())
    return out


def decode_prefill_scatter_kv8(qkv, T, kc8, vc8, ks, vs, klen, lens, slots=None, window=0):
    """decode_prefill_scatter into an fp8 K/V cache (commu_decode_prefill_scatter_kv8): qkv bf16 [T * B, >= 3 H DH] (row
    t * B + b); the K and V of positions max(0, lens[b] - window) <= t < lens[b] are quantised (decode_attn_kv8's recipe)
    into the rows of slot slots[b] (None: b) of kc8 / vc8 uint8 [Bc, H, Lmax, DH] and ks / vs uint8 [Bc, H, Lmax, DH / 32]
    -- linear (window 0) or ring (Lmax = window + 1) --, and klen[slots[b]] = lens[b]."""
    Bc, H, Lmax, DH = _kv8_caches(kc8, vc8, ks, vs)
    for t, name in ((qkv, "qkv"), (klen, "klen"), (lens, "lens")):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
    T, window = int(T), int(window)
    if qkv.dtype != BF16 or qkv.dim() != 2 or T < 1 or qkv.shape[0] % T or qkv.stride(1) != 1:
        raise CommuHipError(f"qkv: bf16 2-D [T * B, >= 3 H DH] with T = {T} expected, got {qkv.dtype} {tuple(qkv.shape)}")
    B = qkv.shape[0] // T
    _i32_rows(lens, B, "lens")
    _i32_rows(slots, B, "slots")
    _i32_rows(klen, Bc, "klen")
    if slots is None and B > Bc:
        raise CommuHipError(f"{B} contexts for a cache of {Bc} slots")
    if qkv.shape[1] < 3 * H * DH:
        raise CommuHipError(f"qkv: at least {3 * H * DH} columns expected, got {qkv.shape[1]}")
    if window < 0 or (window > 0 and Lmax != window + 1):
        raise CommuHipError(f"a ring of window {window} has {window + 1} rows; the caches have {Lmax}")
    if qkv.stride(0) % 8:
        raise CommuHipError("qkv: a row stride that is a multiple of 8 expected")
    call("commu_decode_prefill_scatter_kv8", _p(qkv), qkv.stride(0), T, B, _p(kc8), _p(vc8), _p(ks), _p(vs), _p(klen),
         _p(lens), _p(slots), Bc, H, DH, Lmax, window, _s())


# ---------------------------------------------------------------------------------------------- request pool (opt-in)
def decode_arm_args(cache, image, **fields):
    """The argument block of commu_decode_arm (include/commu_hip.h), built once per decoder: cache / image are the 2 or
    4 cache tensors [L, B, H, Lmax, row] and the store's images [L, Rcap, H, ctx_rows, row] in the same order; every
    other field by its name in the header, tensors (GPU, contiguous) for the pointers and None for an array the decoder
    does not have.  The geometry (B, Rcap, L, H, Lmax, ctx_rows, row_bytes) is read off the tensors."""
    if len(cache) != len(image) or len(cache) not in (2, 4):
        raise CommuHipError(f"decode_arm: 2 or 4 cache tensors and as many images expected, got {len(cache)} / {len(image)}")
    L, B, H, Lmax = cache[0].shape[:4]
    Rcap, ctx_rows = image[0].shape[1], image[0].shape[3]
    rb = []
    for c, im in zip(cache, image):
        if c.dim() != 5 or im.dim() != 5 or not c.is_contiguous() or not im.is_contiguous() or c.dtype != im.dtype:
            raise CommuHipError("decode_arm: contiguous 5-D caches and images of one dtype expected")
        if tuple(c.shape[:4]) != (L, B, H, Lmax) or tuple(im.shape) != (L, Rcap, H, ctx_rows, c.shape[4]):
            raise CommuHipError(f"decode_arm: cache {tuple(c.shape)} and image {tuple(im.shape)} do not belong together")
        rb.append(c.shape[4] * c.element_size())
    a = _lib.struct_args(_lib.DecodeArmArgs, B=B, Rcap=Rcap, L=L, H=H, Lmax=Lmax, ctx_rows=ctx_rows, n_cache=len(cache))
    for i, (c, im) in enumerate(zip(cache, image)):
        a.row_bytes[i], a.cache[i], a.image[i] = rb[i], c.data_ptr(), im.data_ptr()
    for name, v in fields.items():
        if isinstance(v, torch.Tensor):
            if not v.is_contiguous():
                raise CommuHipError(f"decode_arm: {name} is not contiguous")
            v = _p(v)
        setattr(a, name, v)
    return a


def decode_arm(args, njobs: int):
    """ONE launch that arms njobs (slot, entry) jobs staged at args.jobs / args.variates (commu_decode_arm); 0 jobs launch
    nothing."""
    args.njobs = int(njobs)
    call("commu_decode_arm", C.byref(args), _s())


def decode_arm_primed_args(cache, image, ring=False, grid_rows=0, **fields):
    """The argument block of commu_decode_arm_primed (include/commu_hip.h), the same block: decode_arm_args with the
    store's images [L, Rcap, H, ctx_rows, row] of a primed pool, ring (the caches are rings of Lmax rows: klen counts
    positions), grid_rows (0, or the pool's longest image) and the optional e_trace beside trace."""
    a = decode_arm_args(cache, image, ring=1 if ring else 0, grid_rows=int(grid_rows), **fields)
    return _lib.DecodeArmPrimedArgs.from_buffer_copy(a)


def decode_arm_primed_chunk_rows() -> int:
    """Image rows per chunk workgroup of commu_decode_arm_primed."""
    return int(call("commu_decode_arm_primed_chunk_rows"))


def decode_arm_primed(args, njobs: int):
    """ONE launch that arms njobs (slot, entry) jobs of a primed pool (commu_decode_arm_primed): the image is copied by
    one workgroup per (layer, head, job, chunk of rows); 0 jobs launch nothing."""
    args.njobs = int(njobs)
    call("commu_decode_arm_primed", C.byref(args), _s())


# ---------------------------------------------------------------------------------------------- shared prompt prefix (opt-in)
# (include/commu_hip.h, commu_decode_attn_prefix: the K/V of the positions all slots have in common, held once)
def decode_prefix_chunk() -> int:
    """Prefix rows per chunk (one record per (pair, chunk)) of commu_decode_attn_prefix."""
    return int(call("commu_decode_prefix_chunk"))


def decode_prefix_group() -> int:
    """Slots that one prefix workgroup of commu_decode_attn_prefix serves from its staged chunk."""
    return int(call("commu_decode_prefix_group"))


def decode_prefix_ws_floats(B, H, DH, Pcap, nsplit=1) -> int:
    """fp32 words of the record workspace of decode_attn_prefix: B H (nsplit + ceil(Pcap / chunk)) (DH + 2)."""
    return B * H * (int(nsplit) + -(-int(Pcap) // decode_prefix_chunk())) * (DH + 2)


def decode_attn_prefix(qkv, pk, pv, prefix_len, kc, vc, rd, u, vb, klen, active, out, scale, ws, cnt, append=True, nsplit=1):
    """Cached single-token attention over a shared prefix and private rows (commu_decode_attn_prefix): pk / pv bf16
    [H, Pcap, DH] with prefix_len (int32 [1], on the GPU) valid rows; kc / vc bf16 [B, H, Lp, DH] private rows (row r =
    absolute position prefix_len + r), klen int32 [B] private rows per slot; qkv bf16 [B, >= 3 H DH], rd bf16
    [>= Pcap + Lp, >= H DH], out bf16 [B, >= H DH]; ws fp32 [>= decode_prefix_ws_floats(...)], cnt int32 [>= B H] zeroed
    once (every launch leaves it zero).  nsplit > 1 splits the PRIVATE keys as decode_attn's split-key launch does."""
    for t, name in ((qkv, "qkv"), (pk, "pk"), (pv, "pv"), (prefix_len, "prefix_len"), (kc, "kc"), (vc, "vc"), (rd, "rd"),
                    (out, "out"), (u, "r_w_bias"), (vb, "r_r_bias"), (klen, "klen"), (ws, "ws"), (cnt, "cnt")) \
            + (() if active is None else ((active, "active"),)):
        if not t.is_cuda:
            raise CommuHipError(f"{name}: commu_amd kernels need GPU tensors (no CPU fallback)")
    if kc.dtype != BF16 or kc.dim() != 4 or not kc.is_contiguous() or vc.dtype != BF16 or vc.shape != kc.shape \
            or not vc.is_contiguous():
        raise CommuHipError("kc / vc: two contiguous bf16 caches [B, H, Lp, DH] expected")
    B, H, Lp, DH = kc.shape
    if DH not in (32, 64):
        raise CommuHipError(f"d_head {DH}: the decode caches are built for 32 and 64 (pad the model's head)")
    if pk.dtype != BF16 or pk.dim() != 3 or pk.shape[0] != H or pk.shape[2] != DH or not pk.is_contiguous() \
            or pv.dtype != BF16 or pv.shape != pk.shape or not pv.is_contiguous():
        raise CommuHipError(f"pk / pv: two contiguous bf16 prefixes [{H}, Pcap, {DH}] expected")
    Pcap = pk.shape[1]
    if Lp < 1 or Pcap < 1 or Pcap + Lp > RING_MAX_ROWS:
        raise CommuHipError(f"prefix of {Pcap} and private cache of {Lp} positions; together the decode attention supports "
                            f"{RING_MAX_ROWS}")
    HD = H * DH
    if prefix_len.dtype != torch.int32 or prefix_len.numel() != 1:
        raise CommuHipError("prefix_len: int32 [1] expected")
    if klen.dtype != torch.int32 or klen.numel() != B or not klen.is_contiguous():
        raise CommuHipError(f"klen: contiguous int32 [{B}] expected")
    if active is not None and (active.dtype != torch.uint8 or active.numel() != B or not active.is_contiguous()):
        raise CommuHipError(f"active: contiguous uint8 [{B}] expected")
    if qkv.dtype != BF16 or qkv.dim() != 2 or qkv.shape[0] != B or qkv.shape[1] < 3 * HD or qkv.stride(1) != 1 \
            or qkv.stride(0) % 8:
        raise CommuHipError(f"qkv: bf16 [{B}, >= {3 * HD}] with a row stride that is a multiple of 8 expected")
    if rd.dtype != BF16 or rd.dim() != 2 or rd.shape[0] < Pcap + Lp or rd.shape[1] < HD or rd.stride(1) != 1 \
            or rd.stride(0) % 8:
        raise CommuHipError(f"rd: bf16 [>= {Pcap + Lp}, >= {HD}] with a row stride that is a multiple of 8 expected")
    if out.dtype != BF16 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < HD or out.stride(1) != 1:
        raise CommuHipError(f"out: bf16 [{B}, >= {HD}] expected")
    for t, name in ((u, "r_w_bias"), (vb, "r_r_bias")):
        if t.dtype != F32 or t.numel() < HD or not t.is_contiguous():
            raise CommuHipError(f"{name}: contiguous fp32 [>= {HD}] expected")
    nsplit = int(nsplit)
    if nsplit < 1 or nsplit > 16:
        raise CommuHipError("nsplit: 1 .. 16")
    if ws.dtype != F32 or ws.numel() < decode_prefix_ws_floats(B, H, DH, Pcap, nsplit) or not ws.is_contiguous() \
            or cnt.dtype != torch.int32 or cnt.numel() < B * H or not cnt.is_contiguous():
        raise CommuHipError("ws: fp32 [>= B H (nsplit + ceil(Pcap / chunk)) (DH + 2)], cnt: int32 [>= B H]")
    call("commu_decode_attn_prefix", _p(qkv), qkv.stride(0), _p(pk), _p(pv), _p(prefix_len), Pcap, _p(kc), _p(vc), _p(rd),
         rd.stride(0), _p(u), _p(vb), _p(klen), _p(active), _p(out), out.stride(0), B, H, DH, Lp, float(scale),
         1 if append else 0, nsplit, _p(ws), _p(cnt), _s())
    return out
