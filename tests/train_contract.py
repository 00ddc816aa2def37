"""Float64 contracts of the training step's support kernels (csrc/elementwise.hip).  Plain module: torch and numpy on the
CPU, nothing from the library.  For every kernel family it holds

  * a float64 REFERENCE evaluated on the exact bf16 / fp32 input values,
  * a per-element BOUND derived from rounding (u = 2^-24, the unit roundoff of fp32), never from a kernel's output,
  * INPUT BUILDERS for the edge shapes, and an fp32 EMULATION that mirrors the kernel's index mapping (lane -> columns,
    rows -> block / wave / pair, grid strides) with named, plantable DEFECTS.

tests/test_train_contract_host.py proves on the CPU that the clean emulation stays at or below half of every bound and
that every defect is caught by at least one case; tests/test_train_contract_gpu.py holds the kernels to the same checks.
Every check function returns worst ratios error / bound by name (inf: a NaN, or a guard broken).

THE HALF-BOUND RULE AND THE OUTPUT FORMAT'S OWN ROUNDING.  The clean emulation has to stay at or below 0.5 of a bound.  A
bound's term for the FINAL rounding into the output format cannot have that slack: bf16's unit roundoff IS 2^-8, so
"2^-8 |want|" is used up entirely by a correctly rounded bf16 value just above a power of two, and likewise "u |out_before|"
by the one fp32 add into an accumulated output.  For those outputs a check returns two figures:
  NAME   against the whole bound as stated above (at most 1.0 for a correct kernel), and
  NAME~  rounding-aware: a correctly rounded output g of a value v lies within half an ulp OF g of v, so
         max(0, |g - want| - ulp(g) / 2) is a lower bound of |v - want|, the error of the fp32 arithmetic alone; NAME~ is
         that figure over the REST of the bound (everything but the final-rounding term).  At most 0.5 for the clean
         emulation, at most 1.0 on the GPU -- the sharper of the two checks: half an ulp of g is between 2^-9 |g| and
         2^-8 |g|, so an error hidden in the slack of "2^-8 |want|" shows here.
Outputs without such a term have one figure, held to 0.5 (emulation) and 1.0 (GPU).

BOUNDS AND WHERE THEY COME FROM

LayerNorm forward.  A lane adds its 8 * NC elements one after the other, a 6-level butterfly joins the lanes, a division
follows: depth d = 8 NC + 6 + 2 (NC = 1 for D <= 512, else 2).
  mean   d u sum|x_i| / D.
  rstd   relative 2^-19: the variance is a sum of non-negative terms, relative error <= (d + 4) u (4: subtraction,
         square and the division); half of it carries to rstd, plus 2 u for rsqrtf and the eps add -- (d+4)/2 + 2 <= 16 u
         = 2^-20 at NC = 2; 2^-19 is twice that.
  y      2^-8 |want| + 2^-18 (|xhat gamma| + |beta|): bf16 rounding is 2^-9 |want|; the fp32 chain (subtract, two
         products, one add, the error of rstd) is below 2^-20 relative to |xhat gamma| + |beta|.
         NOTE this bound has no term for the rounding of the MEAN, which moves every xhat of a row by the same absolute
         amount rstd * err(mean).  The builders therefore put every row on a dyadic grid on which the fp32 row sum is
         exact in any order (integers below 2^18 times the grid step), so err(mean) <= u |mean| (the division alone), keep
         |offset| / scale <= 2 and |beta| >= 0.25: the shift is then below 2 u * 1.3 < 2^-18 * 0.25 / 2.  A constant row
         (variance 0, rstd = eps^-1/2 = 316) has an exact mean and gives y = beta.
LayerNorm backward.  Inputs are the float64 mean and rstd ROUNDED TO fp32 (not a forward kernel's output); the reference
uses those same fp32 values.
  dz     2^-8 |want| + 2^-17 rstd (|g dy| + mean|g dy| + |xhat| mean|g dy xhat|): bf16 rounding, then the two means (depth
         d, relative to the mean of the magnitudes: d u < 2^-19) and the three-term combination.  With dz_masked the
         second output is want * keep * scale with the same bound times scale.
  part   planes 0 (sum dy xhat) and 1 (sum dy) per block of 32 rows: 2^-18 sum_rows|term| (8 rows per wave one after the
         other, 4 waves: depth 11, plus xhat's own error 3 u);  plane 2: 2^-19 sum|dz| against the float64 sum of the
         DEVICE'S OWN bf16 dz (or dz_masked) over that block's rows -- this pins the block -> row mapping.
Cross entropy.  lse, nll: 2^-22 (|lse| + |x_t| + |nll|) + 2^-18: the sum of at most 1000 exponentials has depth <= 16 + 6,
each expf 2 ulp, so log(sum) is off by <= 24 u < 2^-19 absolute; max + log and lse - x_t round once each.
  dlogits  2^-8 |want| + |g| (p (|x_c| + |lse| + 4) 2^-23 + 2^-24), p = softmax: x_c - lse rounds by u (|x_c| + |lse|),
         which is a relative error of p; expf adds 2 ulp; the input lse is the fp32-rounded float64 lse.
Column sums (colsum, ColsumGroup, layernorm_bwd_reduce): (rows_total + 8) u sum_s |alpha_s| sum_r |X_s[r, c]|
  + u |out_before|, rows_total = rows of all sources of the output (of the bf16 input when a slab pass ran first): the
  plain running-sum bound, whatever the order.  Two runs must be bit-identical.
Masked means: (n + 8) u scale sum_g sum|nll| / cnt_g;  loss_grad_groups is EXACTLY fp32(scale) / fp32(cnt).  masked_mean
  and the grouped form add in different (and, between workgroups, unspecified) orders, so "B == Bc equals masked_mean bit
  for bit" is asked where the fp32 sum is exact in any order: nll on a 2^-10 grid, sum below 2^14.
grad_norm: a sum of non-negative squares, per-thread depth 4 ceil(n / (1024 npart)), two trees and a short tail: relative
  (depth + 20) u on the sum, half of it plus 2 u on the root.
Adam: the oracle tolerances of tests/test_kernels_gpu.py (1e-6 of max|p| on p, m, v; the bf16 shadow within 2^-8 of its
  element); adam_step_dev bit-identical to adam_step; scale_clip exactly g * fp32(min(1, clip / (gnorm + 1e-6))) in fp32;
  casts and transposes bit-exact.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SENT = -123.0                    # sentinel in output columns no kernel may touch (exact in bf16)
F32 = np.float32


def bf16_round(a):
    """fp32 array -> nearest-even bf16, back as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


def ratio(got, want, bound):
    """max |got - want| / bound; an error of 0 counts 0 whatever the bound, a non-finite `got` counts inf."""
    got, want, bound = (np.asarray(t, dtype=np.float64) for t in (got, want, bound))
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / np.broadcast_to(bound, err.shape))
    r = np.where(np.isfinite(got), r, np.inf)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def half_ulp(g, bits):
    """half a unit in the last place of the finite values g in a format of `bits` significand bits (8: bf16, 24: fp32;
    both share fp32's exponent range, denormals take the smallest normal's spacing)"""
    a = np.abs(np.asarray(g, dtype=np.float64))
    with np.errstate(all="ignore"):
        e = np.where((a > 0) & np.isfinite(a), np.floor(np.log2(np.where(a > 0, a, 1.0))), -126.0)
    return 2.0 ** (np.maximum(e, -126.0) - bits)


def excess(got, want, bits, rest):
    """max (|got - want| - ulp(got) / 2) / rest, floored at 0: the figure NAME~ of the module docstring."""
    got, want, rest = (np.asarray(t, dtype=np.float64) for t in (got, want, rest))
    if got.size == 0:
        return 0.0
    own = half_ulp(got, bits)
    err = np.maximum(np.abs(got - want) - own, 0.0)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / np.broadcast_to(rest, err.shape))
    r = np.where(np.isfinite(got), r, np.inf)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def exact(got, want):
    """0.0 when bit-identical as values (no NaN anywhere), else inf."""
    got, want = np.asarray(got), np.asarray(want)
    return 0.0 if got.shape == want.shape and np.array_equal(got, want) and not np.isnan(got.astype(np.float64)).any() \
        else float("inf")


def wave_sum(v):
    """common.h wave_sum over the last axis (64 lanes): xor butterfly 32, 16, .. 1, fp32."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(F32)
    return v


# =====================================================================================================================
# LayerNorm
# =====================================================================================================================
LN_D = (4, 60, 64, 500, 512, 516, 1020, 1024)
LN_ROWS = (1, 3, 5, 31, 32, 33, 65)
LN_EPS = 1e-5
_LN_ROWKIND = ((0.0, 1.0), (0.5, 0.5), (-1.0, 2.0), (2.0, 1.0), (-0.25, 0.25), (1.0, 4.0), (-2.0, 1.5), (0.125, 0.125))


def ln_pitches(D):
    return ((D + 7) & ~7, (D + 63) // 64 * 64 + 8)


def ln_cases():
    """(D, ld, rows): a thinned cross product in which every D and every row count meets both pitches."""
    return [(D, ln_pitches(D)[k], LN_ROWS[(i + 2 * k + 3 * j) % 7]) for i, D in enumerate(LN_D) for k in range(2)
            for j in range(2)]


class LnInputs:
    """z, dy, dy2: fp32 arrays holding bf16 values, [rows, ld], NaN in the pad columns [D, ld)."""

    def __init__(self, D, ld, rows, seed=0):
        self.D, self.ld, self.rows = D, ld, rows
        g = torch.Generator().manual_seed(1000 * D + 10 * ld + rows + seed)
        rn = torch.randn(rows, D, generator=g).clamp(-4, 4).numpy().astype(np.float64)
        z = np.empty((rows, D))
        for r in range(rows):
            off, sc = _LN_ROWKIND[(r + D + seed) % 8]
            k = math.floor(math.log2(255.0 / (abs(off) + 4 * sc)))          # |x| 2^k <= 255: exact in bf16, exact sums
            z[r] = np.round((off + sc * rn[r]) * 2.0 ** k) / 2.0 ** k
        if rows >= 3:
            z[1] = 1.5                                                       # variance 0
            z[rows - 1] = np.round(rn[rows - 1])                             # one element dominates
            z[rows - 1, D // 3] = 200.0
        self.z = self._pad(z)
        self.gamma = (1 + 0.3 * (2 * torch.rand(D, generator=g) - 1)).numpy().astype(F32)
        sign = np.where(torch.rand(D, generator=g).numpy() < 0.5, -1.0, 1.0)
        self.beta = (sign * (0.25 + 0.25 * torch.rand(D, generator=g).numpy())).astype(F32)
        rs = (0.25 * (1 + np.arange(rows) % 5))[:, None]
        self.dy = self._pad(bf16_round(torch.randn(rows, D, generator=g).numpy() * rs))
        self.dy2 = self._pad(bf16_round(torch.randn(rows, D, generator=g).numpy() * 0.5))
        assert np.array_equal(bf16_round(self.z[:, :D]), self.z[:, :D])

    def _pad(self, a):
        out = np.full((self.rows, self.ld), np.nan, dtype=F32)
        out[:, :self.D] = a
        return out

    def keep(self, seed=5):
        """a stand-in keep mask for the host test (the GPU test takes ops.dropout_keep_mask)"""
        g = torch.Generator().manual_seed(seed + self.D + self.rows)
        return (torch.rand(self.rows, self.D, generator=g) >= 0.25).numpy()


def drop_scale(p):
    """common.h: 1 / (1 - round(p 65536) / 65536) in fp32."""
    thr = min(65535, max(1, int(p * 65536.0 + 0.5))) if p > 0 else 0
    return F32(1.0) / (F32(1.0) - F32(thr) / F32(65536.0))


def ln_ref(inp):
    """float64 forward: mean, rstd [rows], xhat, y [rows, D]."""
    x = inp.z[:, :inp.D].astype(np.float64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + float(F32(LN_EPS)))
    xhat = (x - mean[:, None]) * rstd[:, None]
    return dict(mean=mean, rstd=rstd, xhat=xhat, y=xhat * inp.gamma.astype(np.float64) + inp.beta.astype(np.float64))


def ln_stats32(inp):
    """what the backward receives: the float64 statistics rounded to fp32"""
    ref = ln_ref(inp)
    return ref["mean"].astype(F32), ref["rstd"].astype(F32)


def ln_zero_end(D, ld):
    return min(ld, (D + 63) & ~63)


def _guard_pad(out, D, ld):
    """[D, Dz) zero, [Dz, ld) still the sentinel."""
    Dz = ln_zero_end(D, ld)
    return bool(np.all(out[:, D:Dz] == 0.0) and np.all(out[:, Dz:] == SENT))


def ln_check_fwd(inp, y, mean, rstd):
    """y [rows, ld] (started as SENT), mean, rstd [rows] (started as NaN) -> dict of worst ratios."""
    D, NC = inp.D, (1 if inp.D <= 512 else 2)
    ref = ln_ref(inp)
    x = inp.z[:, :D].astype(np.float64)
    d = 8 * NC + 6 + 2
    g, b = inp.gamma.astype(np.float64), inp.beta.astype(np.float64)
    out = dict(mean=ratio(mean, ref["mean"], d * U * np.abs(x).sum(1) / D),
               rstd=ratio(rstd, ref["rstd"], 2.0 ** -19 * ref["rstd"]),
               y=ratio(y[:, :D], ref["y"], 2.0 ** -8 * np.abs(ref["y"]) + 2.0 ** -18 * (np.abs(ref["xhat"] * g) + np.abs(b))))
    out["y~"] = excess(y[:, :D], ref["y"], 8, 2.0 ** -18 * (np.abs(ref["xhat"] * g) + np.abs(b)))
    out["guard"] = 0.0 if _guard_pad(np.asarray(y), D, inp.ld) else float("inf")
    return out


def ln_bwd_ref(inp, mean32, rstd32, add=False, keep=None, scale=1.0):
    """float64 backward on the fp32 statistics: dz, its bound, the per-row terms of part planes 0 and 1."""
    D = inp.D
    x = inp.z[:, :D].astype(np.float64)
    d = inp.dy[:, :D].astype(np.float64) + (inp.dy2[:, :D].astype(np.float64) if add else 0.0)
    rs = rstd32.astype(np.float64)[:, None]
    xhat = (x - mean32.astype(np.float64)[:, None]) * rs
    gy = d * inp.gamma.astype(np.float64)
    m1, m2 = gy.mean(1, keepdims=True), (gy * xhat).mean(1, keepdims=True)
    dz = rs * (gy - m1 - xhat * m2)
    soft = 2.0 ** -17 * rs * (np.abs(gy) + np.abs(gy).mean(1, keepdims=True) + np.abs(xhat) * np.abs(gy * xhat).mean(1, keepdims=True))
    out = dict(dz=dz, dz_own=2.0 ** -8 * np.abs(dz), dz_rest=soft, t0=d * xhat, t1=d)
    if keep is not None:
        s = float(scale)
        out["dzm"] = np.where(keep, dz * s, 0.0)
        out["dzm_own"], out["dzm_rest"] = np.where(keep, 2.0 ** -8 * np.abs(dz * s), 0.0), np.where(keep, s * soft, 0.0)
    return out


def ln_check_bwd(inp, mean32, rstd32, dz, part, add=False, keep=None, scale=1.0, dzm=None):
    """dz / dzm [rows, ld] (started as SENT), part [nblk, 3, D] (started as NaN)."""
    D, rows = inp.D, inp.rows
    ref = ln_bwd_ref(inp, mean32, rstd32, add, keep, scale)
    dz, part = np.asarray(dz, dtype=np.float64), np.asarray(part, dtype=np.float64)
    out = {"dz": ratio(dz[:, :D], ref["dz"], ref["dz_own"] + ref["dz_rest"]),
           "dz~": excess(dz[:, :D], ref["dz"], 8, ref["dz_rest"])}
    ok = _guard_pad(dz, D, inp.ld)
    last = dz
    if keep is not None:
        dzm = np.asarray(dzm, dtype=np.float64)
        out["dzm"] = ratio(dzm[:, :D], ref["dzm"], ref["dzm_own"] + ref["dzm_rest"])
        out["dzm~"] = excess(dzm[:, :D], ref["dzm"], 8, ref["dzm_rest"] + 1e-300)
        ok = ok and _guard_pad(dzm, D, inp.ld)
        last = dzm
    nblk = (rows + 31) // 32
    ok = ok and part.shape == (nblk, 3, D)
    want = np.zeros((nblk, 3, D))
    bound = np.zeros((nblk, 3, D))
    for b in range(nblk):
        sl = slice(32 * b, min(rows, 32 * b + 32))
        for k, t in enumerate((ref["t0"], ref["t1"])):
            want[b, k], bound[b, k] = t[sl].sum(0), 2.0 ** -18 * np.abs(t[sl]).sum(0)
        own = np.nan_to_num(last[sl, :D])
        want[b, 2], bound[b, 2] = own.sum(0), 2.0 ** -19 * np.abs(own).sum(0)
    if ok:
        out["part01"] = ratio(part[:, :2], want[:, :2], bound[:, :2])
        out["part2"] = ratio(part[:, 2], want[:, 2], bound[:, 2])
    out["guard"] = 0.0 if ok else float("inf")
    return out


def _ln_lanes(D, ld, NC, defect):
    e = np.arange(8)
    base = np.arange(64)[:, None] * 8 + 512 * np.arange(NC)[None, :]          # [64, NC]
    lim = ld if defect == "pad_in_mean" else D                                 # DEFECT: pad columns [D, ld) enter the sums
    act, hi = base < lim, base + 4 < lim
    if defect == "hi_upper":                                                   # DEFECT: upper half-chunk read when !hi
        hi = act
    valid = act[..., None] & ((e < 4) | hi[..., None])
    col = base[..., None] + e
    return base, act, valid, col, np.minimum(col, ld - 1)


def _store_rows(out, rowsel, vals, base, act, D, ld, defect):
    """The kernels' stores of one or more rows: 8-wide chunks where a chunk has valid columns, zeros in [D, Dz)."""
    Dz = ln_zero_end(D, ld)
    if defect == "pad_overwritten":                                            # DEFECT: zeroes up to the pitch
        Dz = ld
    cols = (base[act][:, None] + np.arange(8)).ravel()
    sel = cols < ld
    out[rowsel, cols[sel]] = vals[..., act, :].reshape(*vals.shape[:-3], -1)[..., sel]
    if defect != "pad_not_zeroed":                                             # DEFECT: [D, Dz) left as it was
        padc = ~act & (base < Dz)
        pc = (base[padc][:, None] + np.arange(8)).ravel()
        out[rowsel, pc[pc < ld]] = 0.0


def ln_fwd_emu(inp, defect=None):
    """layernorm_fwd_kernel in fp32, all rows at once: lane l owns columns 8 l + 512 c + e."""
    D, ld, rows = inp.D, inp.ld, inp.rows
    base, act, valid, col, colc = _ln_lanes(D, ld, 2, defect)
    with np.errstate(all="ignore"):
        x = np.where(valid, inp.z[:, colc], F32(0))                            # [rows, 64, 2, 8]
        s = np.zeros((rows, 64), F32)
        for c in range(2):
            for e in range(8):
                s = s + x[:, :, c, e]
        mu = (wave_sum(s)[:, 0] / F32(D)).astype(F32)
        dlt = (x - mu[:, None, None, None]).astype(F32)
        q = np.zeros((rows, 64), F32)
        for c in range(2):
            for e in range(8):
                q = q + np.where(valid[:, c, e], dlt[:, :, c, e] * dlt[:, :, c, e], F32(0))
        rs = (F32(1) / np.sqrt(wave_sum(q)[:, 0] / F32(D) + F32(LN_EPS))).astype(F32)
        g = np.where(col < D, inp.gamma[np.minimum(col, D - 1)], F32(0))
        b = np.where(col < D, inp.beta[np.minimum(col, D - 1)], F32(0))
        v = np.where(valid, dlt * rs[:, None, None, None] * g + b, F32(0)).astype(F32)
    y = np.full((rows, ld), SENT, F32)
    _store_rows(y, slice(None), bf16_round(v), base, base < D, D, ld, defect)
    return y, mu, rs


LN_FWD_DEFECTS = ("hi_upper", "pad_in_mean", "pad_not_zeroed", "pad_overwritten")
LN_BWD_DEFECTS = LN_FWD_DEFECTS + ("pair_swapped", "lookahead_accumulated", "odd_row_skipped", "add_dropped_chunk2")


def ln_bwd_emu(inp, mean32, rstd32, add=False, keep=None, scale=1.0, defect=None):
    """layernorm_bwd_kernel<NC, ADD> in fp32: block = 32 rows, wave w rows r0 .. r0 + 7 two at a time, the pair after
    the last re-reads row rows - 1 (clamped) and must not count."""
    D, ld, rows = inp.D, inp.ld, inp.rows
    NC = 1 if D <= 512 else 2
    base, act, valid, col, colc = _ln_lanes(D, ld, NC, defect)
    gm = np.where(col < D, inp.gamma[np.minimum(col, D - 1)], F32(0)).astype(F32)
    invD, scale = F32(1) / F32(D), F32(scale)
    dz = np.full((rows, ld), SENT, F32)
    dzm = np.full((rows, ld), SENT, F32) if keep is not None else None
    nblk = (rows + 31) // 32
    part = np.full((nblk, 3, D), np.nan, F32)
    zero = np.zeros((64, NC, 8), F32)
    vcol = col[col < D]
    with np.errstate(all="ignore"):
        for blk in range(nblk):
            red = []
            for w in range(4):
                r0 = blk * 32 + w * 8
                nr = min(8, rows - r0)
                ag, ab, az = zero.copy(), zero.copy(), zero.copy()
                for rr in range(0, max(nr, 0), 2):
                    if defect == "odd_row_skipped" and rr + 1 >= nr:           # DEFECT: loop runs while rr + 1 < nr
                        break
                    res = []
                    for u in range(2):
                        live = rr + u < nr
                        r = min(r0 + rr + u, rows - 1)
                        ok = valid if (live or defect == "lookahead_accumulated") else np.zeros_like(valid)
                        d = inp.dy[r, colc]
                        if add:
                            d2 = inp.dy2[r, colc]
                            if defect == "add_dropped_chunk2":                 # DEFECT: the addend of chunk 1 is dropped
                                d2 = np.where(np.arange(NC)[None, :, None] >= 1, F32(0), d2)
                            d = d + d2
                        d = np.where(ok, d, F32(0)).astype(F32)
                        xh = np.where(ok, (inp.z[r, colc] - mean32[r]) * rstd32[r], F32(0)).astype(F32)
                        gy = (d * gm).astype(F32)
                        s1, s2 = np.zeros(64, F32), np.zeros(64, F32)
                        for c in range(NC):
                            for e in range(8):
                                s1 = s1 + gy[:, c, e]
                                s2 = s2 + gy[:, c, e] * xh[:, c, e]
                        ag, ab = ag + d * xh, ab + d
                        res.append((live, gy, xh, wave_sum(s1)[0] * invD, wave_sum(s2)[0] * invD, rstd32[r]))
                    for u, (live, gy, xh, m1, m2, rs) in enumerate(res):
                        if not live:
                            break
                        row = r0 + rr + u
                        v = np.where(valid, rs * (gy - m1 - xh * m2), F32(0)).astype(F32)
                        o = bf16_round(v)
                        if defect == "pair_swapped" and res[1][0]:             # DEFECT: row u written where row 1 - u belongs
                            row = r0 + rr + 1 - u
                        if keep is not None:
                            kp = np.where(col < D, keep[r0 + rr + u, np.minimum(col, D - 1)], False)
                            om = bf16_round(np.where(kp, v * scale, F32(0)))
                            az = az + om
                            _store_rows(dzm, row, om, base, base < D, D, ld, defect)
                        else:
                            az = az + o
                        _store_rows(dz, row, o, base, base < D, D, ld, defect)
                red.append((ag, ab, az))
            for k in range(3):
                tot = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]
                part[blk, k, vcol] = tot[col < D]
    return dz, dzm, part


# =====================================================================================================================
# Cross entropy
# =====================================================================================================================
CE_SHAPES = ((729, 768), (768, 768), (5, 8), (1, 4), (729, 729), (769, 772), (1000, 1000))
CE_ROWS = (1, 5, 9)
CE_BWD_EXTRA = ((729, 768, 736), (729, 736, 768))          # (V, ldl, ldd)


def ce_fwd_cases():
    return [(V, ldl, rows) for V, ldl in CE_SHAPES for rows in CE_ROWS]


def ce_bwd_cases():
    """(V, ldl, ldd, rows)"""
    return [(V, ldl, ldl, rows) for V, ldl, rows in ce_fwd_cases()] + [(V, ldl, ldd, rows) for V, ldl, ldd in CE_BWD_EXTRA
                                                                         for rows in CE_ROWS]


def ce_vec_fwd(V, ldl):
    return V <= 768 and ldl <= 768 and ldl % 4 == 0


def ce_vec_bwd(V, ldl, ldd):
    return V <= 768 and ldl <= 768 and ldd <= 768 and ldl % 4 == 0 and ldd % 4 == 0 and ldd <= ldl + 3


class CeInputs:
    """x [rows, ldl] fp32 with NaN in [V, ldl); target; g (upstream gradient)."""

    def __init__(self, V, ldl, rows, salt=0):
        self.V, self.ldl, self.rows = V, ldl, rows
        g = torch.Generator().manual_seed(7 * V + 3 * ldl + rows)
        x = (3.0 * torch.randn(rows, V, generator=g)).numpy().astype(np.float64)
        cand = [t for t in (0, V - 1, 255, 256, 511, 512, V // 2, 1) if 0 <= t < V]
        rot = V + rows + salt
        self.target = np.array([cand[(i + rot) % len(cand)] for i in range(rows)], dtype=np.int64)
        for i in range(rows):
            x[i] += (-90.0, 0.0, 90.0)[(i + rot) % 3]          # a lost max-subtraction over- or underflows
        if rows > 2 and V > 1:
            x[2, (int(self.target[2]) + V // 2 + 1) % V] += 40.0          # a non-target logit dominates
        self.x = np.full((rows, ldl), np.nan, dtype=F32)
        self.x[:, :V] = x
        self.g = (0.01 * (0.5 + torch.rand(rows, generator=g))).numpy().astype(F32)
        if rows >= 5:
            self.g[3] = 0.0                                    # a pad target's row


def ce_ref(inp):
    x = inp.x[:, :inp.V].astype(np.float64)
    mx = x.max(1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(1))
    xt = x[np.arange(inp.rows), inp.target]
    return dict(lse=lse, nll=lse - xt, xt=xt)


def ce_check_fwd(inp, nll, lse):
    ref = ce_ref(inp)
    bound = 2.0 ** -22 * (np.abs(ref["lse"]) + np.abs(ref["xt"]) + np.abs(ref["nll"])) + 2.0 ** -18
    return dict(lse=ratio(lse, ref["lse"], bound), nll=ratio(nll, ref["nll"], bound))


def ce_lse32(inp):
    return ce_ref(inp)["lse"].astype(F32)


def ce_check_bwd(inp, lse32, dlogits, ldd):
    """dlogits [rows, ldd]: every column of the pitch is written, [V, ldd) as zero."""
    V = inp.V
    x = inp.x[:, :V].astype(np.float64)
    l, g = lse32.astype(np.float64)[:, None], inp.g.astype(np.float64)[:, None]
    p = np.exp(x - l)
    onehot = np.arange(V)[None, :] == inp.target[:, None]
    want = g * (p - onehot)
    own, rest = 2.0 ** -8 * np.abs(want), np.abs(g) * (p * (np.abs(x) + np.abs(l) + 4) * 2.0 ** -23 + 2.0 ** -24) + 1e-300
    d = np.asarray(dlogits, dtype=np.float64)
    ok = d.shape == (inp.rows, ldd) and bool(np.all(d[:, V:] == 0.0))
    return {"dlogits": ratio(d[:, :V], want, own + rest), "dlogits~": excess(d[:, :V], want, 8, rest),
            "guard": 0.0 if ok else float("inf")}


def _ce_index(V, ld, vec):
    if vec:          # lane l holds columns 4 l + 256 k + e, k < 3
        return (4 * np.arange(64)[:, None, None] + 256 * np.arange(3)[None, :, None] + np.arange(4)).reshape(64, 12)
    return np.arange(64)[:, None] + 64 * np.arange((max(V, ld) + 63) // 64)[None, :]


CE_FWD_DEFECTS = ("no_max_subtraction", "pad_in_sum")
CE_BWD_DEFECTS = ("onehot_off_by_one", "pad_in_sum")


def ce_fwd_emu(inp, defect=None):
    V, ldl, rows = inp.V, inp.ldl, inp.rows
    idx = _ce_index(V, ldl, ce_vec_fwd(V, ldl))
    lim = ldl if defect == "pad_in_sum" else V                 # DEFECT: pad columns [V, ldl) enter max and sum
    valid = idx < lim
    with np.errstate(all="ignore"):
        xg = inp.x[:, np.minimum(idx, ldl - 1)]                # [rows, 64, J]
        xm = np.where(valid, xg, F32(-3.0e38))
        mx = xm.reshape(rows, -1).max(1)
        mx = np.where(np.isnan(xm.reshape(rows, -1)).any(1), F32(np.nan), mx).astype(F32)
        if defect == "no_max_subtraction":                     # DEFECT
            mx = np.zeros(rows, F32)
        s = np.zeros((rows, 64), F32)
        for j in range(idx.shape[1]):
            s = s + np.where(valid[:, j], np.exp((xg[:, :, j] - mx[:, None]).astype(F32)), F32(0)).astype(F32)
        lse = (mx + np.log(wave_sum(s)[:, 0])).astype(F32)
        nll = (lse - inp.x[np.arange(rows), inp.target]).astype(F32)
    return nll, lse


def ce_bwd_emu(inp, lse32, ldd, defect=None):
    V, ldl, rows = inp.V, inp.ldl, inp.rows
    c = np.arange(ldd)
    lim = min(ldl, ldd) if defect == "pad_in_sum" else V       # DEFECT: pad columns get a gradient
    t = inp.target + (1 if defect == "onehot_off_by_one" else 0)          # DEFECT
    with np.errstate(all="ignore"):
        xg = inp.x[:, np.minimum(c, ldl - 1)]
        p = np.exp((xg - lse32[:, None]).astype(F32)).astype(F32)
        v = inp.g[:, None] * (p - (c[None, :] == t[:, None]).astype(F32))
        v = np.where(c[None, :] < lim, v, F32(0)).astype(F32)
    return bf16_round(v)


# =====================================================================================================================
# Column sums: colsum, ColsumGroup (one launch for many outputs), layernorm_bwd_reduce
# =====================================================================================================================
COLSUM_MAX_TASKS, COLSUM_MAX_SOURCES = 48, 64
REDUCE_NBLK = (1, 3, 64, 65, 257, 300)
REDUCE_D = (4, 20, 500, 516)


def colsum_slabs(rows, cols, elem_bytes):
    """commu_colsum_slabs: rows of the slab workspace (0: a small fp32 input is summed directly)."""
    if rows <= 0 or cols <= 0:
        return 0
    small = rows * cols * elem_bytes <= (4 << 20)
    if small and elem_bytes == 4:
        return 0
    nx = (cols + (512 if elem_bytes == 2 else 256) - 1) // (512 if elem_bytes == 2 else 256)
    ny = (rows + 63) // 64
    cap = 256 if small else (512 + nx - 1) // nx
    return min(ny, cap)


def slab_pass_emu(X, elem_bytes):
    """colsum_slab_kernel: slab `by` holds rows [by rpb, (by + 1) rpb); wave w adds rows rbeg + w, + 4, ..; then
    wave 0 + 1 + 2 + 3."""
    rows, cols = X.shape
    ny = colsum_slabs(rows, cols, elem_bytes)
    rpb = (rows + ny - 1) // ny
    ws = np.zeros((ny, cols), F32)
    for by in range(ny):
        sl = X[by * rpb:min(rows, (by + 1) * rpb)].astype(F32)
        w = [np.add.reduce(sl[k::4], axis=0, dtype=F32) if sl[k::4].size else np.zeros(cols, F32) for k in range(4)]
        ws[by] = ((w[0] + w[1]) + w[2]) + w[3]
    return ws


def _rowlane_sums(X):
    """p[rl, c] = X[rl, c] + X[rl + 64, c] + ... in that order (fp32)."""
    rows, cols = X.shape
    k = (rows + 63) // 64
    Xp = np.zeros((k * 64, cols), F32)
    Xp[:rows] = X
    p = np.zeros((64, cols), F32)
    for i in range(k):
        p = p + Xp[64 * i:64 * i + 64]
    return p


def _rowlane_tree(acc):
    red = acc.copy()
    for st in (32, 16, 8, 4):
        red[:st] = red[:st] + red[st:2 * st]
    return ((red[0] + red[1]) + red[2]) + red[3]


def colsum_final_emu(out, X, alpha):
    """colsum_final_kernel: out[c] += alpha * tree(row-lane sums)."""
    return (out + F32(alpha) * _rowlane_tree(_rowlane_sums(X))).astype(F32)


def colsum_task_emu(out, sources, defect=None):
    """colsum_group_kernel for one task: sources = [(X fp32 [rows, cols], alpha)], acc += p_s * alpha_s per row lane."""
    acc = np.zeros((64, out.shape[0]), F32)
    for k, (X, alpha) in enumerate(sources):
        if defect == "alpha_shifted":                                          # DEFECT: alpha of source k used for k + 1
            alpha = sources[k - 1][1] if k else 1.0
        acc = acc + _rowlane_sums(X) * F32(alpha)
    return (out + _rowlane_tree(acc)).astype(F32)


def flush_plan(nsrc_per_task, defect=None):
    """ops.ColsumGroup.flush: consecutive tasks share a launch until 48 tasks or 64 sources would be exceeded.
    Returns the launches as lists of task indices."""
    launches, cur, ns = [], [], 0
    for t, k in enumerate(nsrc_per_task):
        if len(cur) + 1 > COLSUM_MAX_TASKS or ns + k > COLSUM_MAX_SOURCES:
            launches.append(cur)
            cur, ns = [], 0
        cur.append(t)
        ns += k
    if cur:
        launches.append(cur)
    if defect == "second_launch_first_task_skipped":                           # DEFECT
        launches = [l if i == 0 else l[1:] for i, l in enumerate(launches)]
    return launches


def colsum_group_emu(tasks, defect=None):
    """tasks = [(out_before fp32 [cols], [(X, alpha), ...])] -> outputs after flush()."""
    outs = [t[0].copy() for t in tasks]
    for launch in flush_plan([len(t[1]) for t in tasks], defect):
        for t in launch:
            outs[t] = colsum_task_emu(tasks[t][0], tasks[t][1], defect)
    return outs


def colsum_check(out, out_before, sources, rows_total=None):
    """sources = [(X float array [rows, cols] of the ORIGINAL input values, alpha)]."""
    want = np.asarray(out_before, dtype=np.float64).copy()
    mag = np.zeros_like(want)
    rt = 0
    for X, alpha in sources:
        X = np.asarray(X, dtype=np.float64)
        want += alpha * X.sum(0)
        mag += abs(alpha) * np.abs(X).sum(0)
        rt += X.shape[0]
    rt = rows_total if rows_total is not None else rt
    own, rest = U * np.abs(out_before), (rt + 8) * U * mag + 1e-300
    return {"sum": ratio(out, want, own + rest), "sum~": excess(out, want, 24, rest)}


def group_cases(seed=0):
    """The two groups of the GPU test, as host data: a list of tasks (out_before, [(kind, X, alpha)]) with
    kind 'bf16' (slab pass first), 'f32' (summed directly) or 'part' (plane of a LayerNorm partial array)."""
    g = torch.Generator().manual_seed(90 + seed)

    def rnd(*s):
        return torch.randn(*s, generator=g).numpy().astype(F32)
    big = bf16_round(rnd(300, 516) + 0.5)
    small = rnd(70, 729) * 3
    part = rnd(65, 3, 500)
    first = [(rnd(516), [("bf16", big, 0.5), ("f32", rnd(130, 516), -2.0)]),
             (rnd(729), [("f32", small, 1.0), ("f32", rnd(5, 729), 0.25), ("f32", rnd(1, 729), 3.0)]),
             (rnd(500), [("part", part[:, 2], 1.0), ("f32", rnd(200, 500), 1.5)])]
    second = []
    for t in range(50):
        cols = (16, 20, 3, 64, 17)[t % 5]
        srcs = [("f32", rnd(1 + (7 * t) % 90, cols) + 1.0, 1.0 + 0.5 * (t % 3))]
        if t >= 20:
            srcs.append(("f32", rnd(1 + (5 * t) % 70, cols) - 1.0, -0.5 - 0.25 * (t % 4)))
        second.append((rnd(cols) * 10, srcs))
    return first, second


def group_host_sources(task):
    """what the final pass of a task sees: slab partial rows for a bf16 source, the array itself otherwise"""
    return [(slab_pass_emu(X, 2) if kind == "bf16" else X, alpha) for kind, X, alpha in task[1]]


# =====================================================================================================================
# Masked means over column groups
# =====================================================================================================================
MM_CASES = ((7, 6, 2), (64, 16, 1), (5, 8, 8), (300, 12, 3))
MM_PAD = 0


class MmInputs:
    def __init__(self, T, B, Bc, all_pad_group=None):
        self.T, self.B, self.Bc, self.G, self.n = T, B, Bc, B // Bc, T * B
        g = torch.Generator().manual_seed(T + 31 * B + Bc)
        i = np.arange(self.n)
        grp = (i % B) // Bc
        frac = torch.randint(0, 1024, (self.n,), generator=g).numpy() / 1024.0
        self.nll = ((1 + grp % 8) * 8.0 + frac).astype(F32)          # a group mix-up moves a mean by >= 8; 2^-10 grid
        self.target = torch.randint(0, 4, (self.n,), generator=g).numpy().astype(np.int64)          # 0 = pad, ~1/4
        self.target[grp == (self.G - 1)] = np.where(i[grp == (self.G - 1)] % 3 == 0, 0, 2)          # uneven counts
        if all_pad_group is not None:
            self.target[grp == all_pad_group] = MM_PAD
        self.scale = F32(1.0 / self.G)


def mm_group_of(i, B, Bc, G, defect=None):
    if defect == "group_is_i_div_Bc":                                          # DEFECT (the kernel would index cnt[] wildly)
        return np.minimum(i // Bc, G - 1)
    return (i % B) // Bc


MM_DEFECTS = ("group_is_i_div_Bc",)


def mm_emu(inp, defect=None):
    """masked_sum_groups + final + loss_grad_groups in fp32 -> out, sum_all, cnt [G], g [n]."""
    i = np.arange(inp.n)
    grp = mm_group_of(i, inp.B, inp.Bc, inp.G, defect)
    live = inp.target != MM_PAD
    sums = np.array([np.add.reduce(inp.nll[live & (grp == k)], dtype=F32) for k in range(inp.G)], dtype=F32)
    cnt = np.array([(live & (grp == k)).sum() for k in range(inp.G)], dtype=np.int32)
    tot, al = F32(0), F32(0)
    with np.errstate(all="ignore"):
        for k in range(inp.G):
            tot = tot + (sums[k] / F32(cnt[k]) if cnt[k] > 0 else F32(np.nan))
            al = al + sums[k]
        g = np.where(live, inp.scale / np.maximum(cnt[grp], 1).astype(F32), F32(0)).astype(F32)
    return F32(inp.scale * tot), F32(al), cnt, g


def mm_check(inp, out, sum_all, cnt, g):
    """sum_all may be None (not requested)."""
    i = np.arange(inp.n)
    grp = (i % inp.B) // inp.Bc
    live = inp.target != MM_PAD
    nll = inp.nll.astype(np.float64)
    cw = np.array([(live & (grp == k)).sum() for k in range(inp.G)])
    sw = np.array([nll[live & (grp == k)].sum() for k in range(inp.G)])
    res = dict(cnt=exact(np.asarray(cnt), cw.astype(np.int32)))
    if (cw == 0).any():
        res["out"] = 0.0 if np.isnan(float(out)) else float("inf")
    else:
        mag = sum(np.abs(nll[live & (grp == k)]).sum() / cw[k] for k in range(inp.G))
        res["out"] = ratio(out, float(inp.scale) * (sw / cw).sum(), (inp.n + 8) * U * float(inp.scale) * mag)
    if sum_all is not None:
        res["sum_all"] = ratio(sum_all, sw.sum(), (inp.n + 8) * U * np.abs(nll[live]).sum() + 1e-300)
    gw = np.where(live, inp.scale / np.maximum(cw[grp], 1).astype(F32), F32(0)).astype(F32)
    res["grad"] = exact(np.asarray(g, dtype=F32), gw)
    return res


# =====================================================================================================================
# Optimiser step: grad_norm, Adam, scale_clip, casts
# =====================================================================================================================
ADAM_N = (3, 1021, 4096 * 1024 + 1027)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_STEP, ADAM_CLIP = 1e-2, 0.9, 0.999, 1e-8, 3, 0.25
GRAD_NORM_CASES = ((40000, 4), (40003, 4), (4099, 1))
CAST_N = (1, 4096 * 256 + 5)
ADAM_DEFECTS = ("tail_past_grid_skipped",)
GRAD_NORM_DEFECTS = ("fourth_load_dropped",)


def adam_inputs(n, seed=0):
    g = torch.Generator().manual_seed(n % 100003 + seed)
    p = torch.randn(n, generator=g).numpy()
    gr = (0.1 * torch.randn(n, generator=g)).numpy()
    m = (0.05 * torch.randn(n, generator=g)).numpy()          # accumulated state starts non-zero
    v = (0.01 * torch.rand(n, generator=g)).numpy() + F32(1e-4)
    return p, gr, m, v


def clip_coef32(gnorm, clip):
    """fp32 min(1, clip / (gnorm + 1e-6))"""
    return min(F32(1), F32(clip) / (F32(gnorm) + F32(1e-6)))


def bias_corrections32(b1, b2, step):
    return F32(1) - F32(F32(b1) ** F32(step)), F32(1) - F32(F32(b2) ** F32(step))


def adam_ref(p, g, m, v, coef, bc1, bc2, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """float64 on the fp32 inputs; coef, bc1, bc2, lr, b1, b2, eps are the fp32 values the kernel receives."""
    p, g, m, v = (t.astype(np.float64) for t in (p, g, m, v))
    b1, b2, lr, eps = (float(F32(t)) for t in (b1, b2, lr, eps))
    gr = g * float(coef)
    mm = b1 * m + (1 - b1) * gr
    vv = b2 * v + (1 - b2) * gr * gr
    return p - (lr / float(bc1)) * mm / (np.sqrt(vv) / math.sqrt(float(bc2)) + eps), mm, vv


def adam_check(want, p, m, v, pb):
    wp, wm, wv = want
    res = dict(p=ratio(p, wp, 1e-6 * np.abs(wp).max()), m=ratio(m, wm, 1e-6 * np.abs(wm).max()),
               v=ratio(v, wv, 1e-6 * np.abs(wv).max()))
    if pb is not None:
        res["shadow"] = ratio(pb, wp, 2.0 ** -8 * np.abs(wp) + 1e-6 * np.abs(wp).max())
        res["shadow~"] = excess(pb, wp, 8, 1e-6 * np.abs(wp).max())
    return res


def adam_covered(n, defect=None):
    """adam_kernel's grid: min(4096, (n / 4 + 255) / 256) blocks of 256 lanes x 4 elements, striding over the rest."""
    if defect == "tail_past_grid_skipped":                                     # DEFECT: one pass, no stride
        blocks = max(1, min(4096, (n // 4 + 255) // 256))
        return min(n, blocks * 1024)
    return n


def adam_emu(p, g, m, v, coef, bc1, bc2, defect=None):
    n = adam_covered(p.shape[0], defect)
    b1, b2, eps = F32(ADAM_B1), F32(ADAM_B2), F32(ADAM_EPS)
    step, isb2 = F32(ADAM_LR) / F32(bc1), F32(1) / np.sqrt(F32(bc2))
    po, mo, vo = p.copy(), m.copy(), v.copy()
    gr = (g[:n] * F32(coef)).astype(F32)
    mo[:n] = b1 * m[:n] + (F32(1) - b1) * gr
    vo[:n] = b2 * v[:n] + (F32(1) - b2) * gr * gr
    po[:n] = p[:n] - step * mo[:n] / (np.sqrt(vo[:n]) * isb2 + eps)
    pb = np.full(p.shape[0], SENT, F32)
    pb[:n] = bf16_round(po[:n])
    return po, mo, vo, pb


def grad_norm_inputs(n, seed=0):
    g = torch.Generator().manual_seed(n + seed)
    x = torch.randn(n, generator=g).numpy()
    return (x * (1 + (np.arange(n) % 7))).astype(F32)          # no two quarters of the buffer weigh the same


def grad_norm_bound(n, npart, want):
    depth = 4 * ((n + 1024 * npart - 1) // (1024 * npart)) + 20
    return (depth / 2 + 2) * U * want


def grad_norm_check(x, npart, got):
    want = math.sqrt(float((x.astype(np.float64) ** 2).sum()))
    return ratio(got, want, grad_norm_bound(x.shape[0], npart, want))


def grad_norm_emu(x, npart, defect=None):
    """sumsq_partial_kernel: thread (b, t) starts at 4 (256 b + t), step 1024 npart; while i + 3 step + 3 < n it takes
    four 16-byte loads at i, i + step, i + 2 step, i + 3 step; then one load per step; then sumsq_final."""
    n, step = x.shape[0], 1024 * npart
    i = 4 * np.arange(256 * npart, dtype=np.int64)
    s = np.zeros(256 * npart, F32)
    xp = np.concatenate([x, np.zeros(4 * step + 8, F32)])
    e = np.arange(4)
    while True:
        go = i + 3 * step + 3 < n
        if not go.any():
            break
        t = np.zeros(256 * npart, F32)
        for k in range(3 if defect == "fourth_load_dropped" else 4):          # DEFECT: v3 never added
            blk = xp[(i + k * step)[:, None] + e]
            t = t + (blk * blk).sum(1, dtype=F32)
        s = np.where(go, s + t, s)
        i = np.where(go, i + 4 * step, i)
    while True:
        go = i < n
        if not go.any():
            break
        blk = xp[i[:, None] + e] * ((i[:, None] + e) < n)
        s = np.where(go, s + (blk * blk).sum(1, dtype=F32), s)
        i = np.where(go, i + step, i)
    parts = np.array([(wave_sum(s[256 * b:256 * b + 256].reshape(4, 64))[:, 0]).sum(dtype=F32) for b in range(npart)], F32)
    return F32(np.sqrt(np.add.reduce(parts, dtype=F32)))


def scale_clip_ref(g, gnorm, clip):
    return (g * clip_coef32(gnorm, clip)).astype(F32)


def cast_inputs(n):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 3).numpy()
    sp = np.array([0.0, -0.0, 1.00390625, 1.01171875, 3.3895314e38, np.inf, -np.inf, 65280.0, 1.0 + 2.0 ** -9],
                  dtype=F32)          # ties to even both ways, the largest finite bf16, infinities
    x[:min(n, sp.size)] = sp[:min(n, sp.size)]
    x[-1] = 1.0 + 2.0 ** -8 + 2.0 ** -9          # the last element: a tie that rounds up
    return x


# =====================================================================================================================
# transpose_group_bf16
# =====================================================================================================================
TRANSPOSE_SHAPES = [(1, 1), (64, 64), (65, 63)] + [(1 + (11 * k) % 70, 1 + (7 * k) % 90) for k in range(30)]          # 33 pairs


def transpose_inputs(k, rows, cols):
    """source [rows, cols + extra] (a strided view for odd k) as bf16-valued fp32"""
    g = torch.Generator().manual_seed(500 + k)
    ldi = cols + (3 if k % 2 else 0)
    return bf16_round(torch.randn(rows, ldi, generator=g).numpy())
