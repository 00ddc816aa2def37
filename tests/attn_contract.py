"""Host-side contract of the training attention (csrc/relattn.hip, relattn3.hip, relattn_q3.hip, relattn_kv3.hip and the
fused band pass csrc/band.hip) and the input sets that the host test and the GPU test share.  Plain module, CPU tensors only.

THE CONTRACT, per pair (b, h), in float64 from the bf16 inputs, in closed form (no autograd: the magnitudes come out of
the same pass):

    s_ij = ((q_i + u) . k_j + (q_i + vb) . Rd[i + M - j]) * scale
    masked: j > i + M,  same_length and j <= i - sshift (sshift as ops._attn_desc),  reset[b] and j < M
    lse_i = logsumexp_j s_ij,  P = softmax,  O = P V
    dV_j = sum_i P_ij dO_i,  dP_ij = dO_i . v_j,  delta_i = O_i . dO_i,  dS_ij = P_ij (dP_ij - delta_i)
    dq_i = scale sum_j dS_ij (k_j + Rd[i+M-j]),  dk_j = scale sum_i dS_ij (q_i + u)
    dRd[d] = scale sum_{b,i} dS_{i,i+M-d} (q_i + vb),  du = scale sum dS_ij k_j,  dvb = scale sum dS_ij Rd[i+M-j]

THE MAGNITUDES A: the same sums over the absolute values of their terms; |dS| is replaced by
P_ij (sum_f |dO_if v_jf| + sum_f |O_if dO_if|) (the cancellation in dP - delta), and every term that carries a P_ij also
carries (1 + m_i), m_i = max over the keys of row i with P_ij >= 2^-16 of scale sum_f (|(q+u)_f k_jf| + |(q+vb)_f Rd_f|):
the kernels round (q + u) scale log2 e to bf16, which moves s_ij by up to 2^-9 m_ij and P_ij by that relative amount.
A of lse_i is 1 + m_i (the score perturbation averaged with the weights P_ij is at most 2^-9 m_i; the 1 carries the fp32
arithmetic of a value of order 1 to 10).

THE BOUND, per element:  |got - want| <= rho |want| + c A,  rho = 2^-8 for the bf16 outputs (out, dq, dk, dv), 0 for the
fp32 ones (lse, drd, du, dvb).  Where A = 0 (no visible term) the result must be exactly zero.  c is one constant per
tensor: 4 e_emu rounded up to a power of two, e_emu = max |emulated - float64| / A over every input set of this module (a
property of the reference and the inputs, never of a kernel; tests/test_attn_contract_host.py prints it and re-checks C).
The emulation is the contract with the kernels' bf16 roundings:

    qu2, qv2 = bf16((q + u) c2), c2 = scale log2 e in fp32      relattn.hip:175-176, 494-495; relattn3.hip:209-210
    P -> bf16 before P . V                                       relattn.hip:304, 609; relattn3.hip:347, 352
    delta from the bf16 output (out -> bf16)                     relattn.hip:332, 690; relattn3.hip:494; delta:
                                                                 relattn.hip:1479 (attn_delta_kernel), 822 (in bwd_q)
    P -> bf16 before P^T . dO; dS = bf16(P (dP - delta)) from    relattn.hip:994-995, 1251-1252, 1421-1422;
    the fp32 P (both kernels)                                    relattn_kv3.hip:262-263
    dk = dS^T qu2 / c2 (the rounded operand)                     relattn.hip:1267
    dq_ac -> bf16 before the band part is added                  relattn.hip:1063; relattn_q3.hip:420
    dq = dq_ac + dS-by-distance . Rd                             band.hip:225; the band GEMM's EPI_RESID epilogue (ops.py)
    drd = dS-by-distance^T qv2 / c2 (the rounded operand)        ops.relattn_bwd (commu_reduce_slabs2d_f32 with 1 / c2)
    du = column sums of the UNROUNDED fp32 dq_ac                 relattn.hip:1074-1091
    dvb = colsum(bf16 dq) - du                                   ops._bias_grads

The final rounding of out, dq, dk and dv to bf16 (relattn.hip:332, 1281-1282, 1469-1470; relattn_kv3.hip:286-287; band.hip:225)
is NOT part of what e_emu measures: rho |want| of the bound pays for it.

(The forward kernels round exp2(s - running max) and divide by the unrounded sum at the end; the emulation rounds the
normalised P: the same relative rounding of every term.)

The factor 4 covers the MFMA accumulation order, the online softmax's rescaling, exp2 (about 2^-22) and the fact that
e_emu is an observed maximum over one realisation of the roundings.

SUMS: the products over features, keys and rows are float64 matrix products (the largest set holds 1.7e7 scores of 64
features: trees of elementwise operations over them would take minutes).  Their summation order moves the float64 values
by parts in 1e-16 of A.  A KNOWN FRAGILITY: where that last place flips a bf16 rounding of the emulation (P, dS, dq_ac, the
bf16 out behind delta), e_emu of out, dq, dk, dv, drd, du and dvb moves with the machine's BLAS, by at most one rounding of
one term of one element; the host test therefore asserts that 4 e_emu keeps 1 % clear of the powers of two on both sides,
and a failure of that assertion on another machine means "re-derive C there", not a defect.  lse is exempt: its emulation
rounds qu2 / qv2 only, in elementwise fp32 arithmetic, so its figure (0.506 c) is the same number everywhere.

INPUTS in which single keys matter (balanced pairs, as tests/decode_contract.py): for a probed row i* of a pair the K rows
of the key under test j* and of an anchor far from it are alpha w / (w . w) / scale, w = q_i* + u, ALPHA = 12: both score
alpha above the rest and share the row's probability (e^12 against at most 1152 keys of score about e^1).  Distance probes
do the same through two rows of Rd (w = q_i* + vb; Rd is shared by the batch, so a head's probes take distinct rows).
Probed rows: 0, 63, 64, 127, 128, T - 1, in the first four sequences and two heads; even sequences probe distances in their
odd rows and keys in the others, odd sequences the other way round; each row takes the candidate it has probed least:
the causal edge, the first visible key (key 0; the same_length edge j = i - sshift + 1, tag sl_edge, which goes first
except in a tile's last row; key M of a reset column, tag reset_first), either side of every 32-key and 64-key seam (tags
seam32-, seam32+, seam64-, seam64+); distances on both sides of 1023/1024 ... 127/128, distance 0, the largest visible one, 15 ... 64.
Four more devices, all needed for the host test's condition (every defect >= 2x its bound):
  * the key just BEYOND a probed causal or lower edge scores alpha + HIDDEN_EXTRA: masked, it does nothing; visible, it
    takes the row;
  * dO of a probed row points along v_j* - v_anchor (norm 8), so that dS of the two keys is as large as the row allows:
    with a random dO the probed terms of dq, dk and drd drown in A's (1 + m_i) sum over 64 absolute feature products;
  * QUIET rows: in the last row of every 64-row tile both V rows and dO are scaled by 2^-8.  Every ratio to the bound
    stays; the row's elements lie far below the floor of a whole-tensor metric, which is how own_key_tile_end passes the
    old relerr.
  * LOUD row: dO of the last row T - 1 (where it is not a quiet one) is 4 times as long, so that the last query tile's share
    of du and dvb stands out of a sum over every token row (du_last_tile on a set with two query tiles).
The bound's limit on drd, du and dvb is written down at ZERO_PASSES (end of the module).
DEFECTS: each the image of one line going wrong; the host test proves that each breaks the bound by >= 2x on its
designated set (DESIGNATED)."""
import functools
import math

import torch

from decode_contract import _randn

ALPHA = 12.0
HIDDEN_EXTRA = 8.0           # a key just beyond a mask edge scores alpha + 8: if it counted it would take the row
PAD = 8                      # NaN pad columns of qkv / rd / dout, sentinel pad columns of out / dqkv
XROWS = 3                    # NaN rows after the last row of qkv and rd
TILE = 64
LOG2E = 1.4426950408889634
OLD_TOL = {"out": 1.2e-2, "dq": 2.5e-2, "dk": 2.5e-2, "dv": 2.5e-2, "drd": 2.5e-2, "du": 2.5e-2, "dvb": 2.5e-2}
RHO = {"out": 2.0 ** -8, "dq": 2.0 ** -8, "dk": 2.0 ** -8, "dv": 2.0 ** -8, "lse": 0.0, "drd": 0.0, "du": 0.0, "dvb": 0.0}
TENSORS = ("out", "lse", "dq", "dk", "dv", "drd", "du", "dvb")
# c = 4 e_emu rounded up to a power of two (measured: docs/EXPERIMENTS.md, 9m; re-checked by the host test)
C = {"out": 2.0 ** -8, "lse": 2.0 ** -7, "dq": 2.0 ** -9, "dk": 2.0 ** -8, "dv": 2.0 ** -7, "drd": 2.0 ** -8,
     "du": 2.0 ** -11, "dvb": 2.0 ** -7}

DEFECTS = ("causal_plus", "own_key_tile_end", "same_length_edge_plus", "same_length_edge_minus", "reset_edge",
           "kv_range_lo", "kv_range_hi", "seam_drop", "seam_dup", "dist_shift", "p_block_neighbour", "band_last_slice",
           "band_pass_seam", "drd_tail_zero", "zero_rows_garbage", "du_last_tile")


def sshift_of(T, M, mem_len):
    """ops._attn_desc (model.py:549-568)."""
    mask_len = T + M - mem_len
    return T - mask_len if mask_len > 0 else T


# ------------------------------------------------------------------------------------------------ the contract
def multiplicity(s, defect=None):
    """[B, T, K] float64: how often row i of sequence b counts key j (0: masked)."""
    T, M, K = s.T, s.M, s.K
    i = torch.arange(T)[:, None]
    j = torch.arange(K)[None, :]
    m = j > i + M + (1 if defect == "causal_plus" else 0)
    if s.same_length:
        m = m | (j <= i - s.sshift + {"same_length_edge_plus": 1, "same_length_edge_minus": -1}.get(defect, 0))
    i0 = i // TILE * TILE
    if defect == "kv_range_lo":                          # the lower key tile from the tile's last row
        jlo = torch.zeros_like(i0)
        if s.same_length:
            jlo = (i0 + TILE - 1 - s.sshift + 1).clamp_min(0)
        m = m | (j < (jlo >> 6) * 64)
    if defect == "kv_range_hi":                          # the upper key tile from the tile's first row
        jhi = (i0 + M).clamp_max(K - 1)
        m = m | (j >= ((jhi >> 6) + 1) * 64)
    mult = (~m).double()
    if defect == "own_key_tile_end":
        rows = torch.arange(TILE - 1, T, TILE)
        mult[rows, rows + M] = 0
    if defect in ("seam_drop", "seam_dup"):              # the first key of a 32-key block
        seam = ((j % 32 == 0) & (j > 0)).expand(T, K)
        mult = torch.where(seam, mult * (0.0 if defect == "seam_drop" else 2.0), mult)
    mult = mult[None].repeat(s.B, 1, 1)
    if s.reset is not None and M > 0:
        mult[s.reset.bool(), :, :M - 1 if defect == "reset_edge" else M] = 0
    return mult


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def contract(s, dtype=torch.float64, defect=None, emulate=False, magnitudes=True):
    """{tensor: (want, A)} of an input set, evaluated in `dtype` (stored as float64; A is None without `magnitudes`).
    Layouts: out, dq [B, H, T, DH]; dk, dv [B, H, K, DH]; lse [B, H, T]; drd [H, K, DH]; du, dvb [H, DH].
    emulate: with the kernels' bf16 roundings (module docstring).  defect: see DEFECTS."""
    T, M, K, B, H, DH, scale = s.T, s.M, s.K, s.B, s.H, s.DH, s.scale
    HD = H * DH
    rnd = _bf if emulate else (lambda x: x)
    qkv = s.qkv[:K * B, :3 * HD].view(K, B, 3, H, DH)
    q_all = qkv[M:, :, 0].permute(1, 2, 0, 3)             # [B, H, T, DH]
    k_all, v_all = qkv[:, :, 1].permute(1, 2, 0, 3), qkv[:, :, 2].permute(1, 2, 0, 3)
    dO_all = s.dout[:, :HD].view(T, B, H, DH).permute(1, 2, 0, 3)
    Rd = s.rd[:K, :HD].view(K, H, DH).permute(1, 0, 2).to(dtype)          # [H, K, DH]
    u, vb = s.u.view(H, 1, DH), s.vb.view(H, 1, DH)
    mult_all = multiplicity(s, defect)
    i = torch.arange(T)[:, None]
    didx = i + M - torch.arange(K)[None, :]               # distance of (i, j); also the key of (i, d)
    valid = (didx >= 0)
    shift = torch.zeros(T, 1, dtype=torch.long)
    if defect == "dist_shift":                            # one 16-row wave tile reads Rd one row off
        r0 = s.dist_shift_row // 16 * 16
        shift[r0:r0 + 16] = 1
    gidx = (didx + shift).clamp(0, K - 1)
    sidx = didx.clamp(0, K - 1)

    def by_key(F, idx=gidx):                              # F[..., i, d] -> [..., i, j] with d = i + M - j
        return torch.gather(F, -1, idx.expand(F.shape)) * valid

    by_dist = functools.partial(by_key, idx=sidx)        # F[..., i, j] -> [..., i, d] with j = i + M - d (zero beyond i + M)
    perm = torch.arange(T)
    if defect == "p_block_neighbour":
        perm = torch.where((perm ^ 16) < T, perm ^ 16, perm)
    band_w = torch.ones(B, T, dtype=dtype)                # which token rows take part in the band pass
    if defect == "band_last_slice":
        rows = torch.arange(T)[None, :] * B + torch.arange(B)[:, None]
        band_w[rows >= T * B - TILE] = 0
    band_w = band_w[:, None, :, None]
    dkeep = torch.ones(K, dtype=dtype)
    if defect == "band_pass_seam":
        dkeep[512] = 0
    res = {n: [] for n in ("out", "lse", "dq", "dk", "dv")}
    mag = {n: [] for n in res}
    acc = {n: torch.zeros((H, K, DH) if n == "drd" else (H, DH), dtype=dtype) for n in ("drd", "du", "dvb")}
    amag = {n: torch.zeros_like(acc[n]) for n in acc}
    c2 = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    step = max(1, (1 << 21) // (H * T * K))
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        q, k, v, dO = (t[sl].to(dtype) for t in (q_all, k_all, v_all, dO_all))
        mult = mult_all[sl, None].to(dtype)
        bw = band_w[sl]
        if emulate:
            qf = q_all[sl].float()
            qu2 = ((qf + u) * c2).to(torch.bfloat16).to(dtype)
            qv2 = ((qf + vb) * c2).to(torch.bfloat16).to(dtype)
            qu_s, qv_s = qu2 / LOG2E, qv2 / LOG2E          # (q + u) scale, (q + vb) scale as the kernels hold them
        else:
            qu_s, qv_s = (q + u.to(dtype)) * scale, (q + vb.to(dtype)) * scale
        sc = qu_s @ k.transpose(-1, -2) + by_key(qv_s @ Rd.transpose(-1, -2))
        sc = sc.masked_fill(mult == 0, -math.inf)
        mx = sc.max(-1, keepdim=True).values
        e = mult * torch.exp((sc - mx).double()).to(dtype)
        den = e.sum(-1, keepdim=True)
        P = e / den
        lse = (mx + torch.log(den.double()).to(dtype))[..., 0]
        O = rnd(P) @ v
        Pb = rnd(P)[:, :, perm]
        dP = dO @ v.transpose(-1, -2)
        delta = (rnd(O) * dO).sum(-1, keepdim=True)          # (emulated: from the bf16 output)
        dS = rnd(P[:, :, perm] * (dP - delta))               # (the kernels round the product of the fp32 P)
        # (p_block_neighbour: dk, dv from the neighbouring row group's block; dq as it should be)
        dS_q = rnd(P * (dP - delta)) if defect == "p_block_neighbour" else dS
        dSd = by_dist(dS_q) * bw * dkeep
        dv = Pb.transpose(-1, -2) @ dO
        dk = dS.transpose(-1, -2) @ qu_s
        ac = scale * (dS_q @ k)
        bd = scale * (dSd @ Rd)
        dq = rnd(ac) + bd
        # (the outputs stay unrounded: their last rounding to bf16 is what rho |want| of the bound is for)
        res["out"].append(O), res["lse"].append(lse), res["dq"].append(dq), res["dk"].append(dk), res["dv"].append(dv)
        acc["drd"] += torch.einsum("bhid,bhif->hdf", dSd, qv_s)
        du_rows = ac
        if defect == "du_last_tile":
            du_rows = ac[:, :, :(T - 1) // TILE * TILE]
        acc["du"] += du_rows.sum((0, 2))
        acc["dvb"] += (rnd(dq).sum((0, 2)) - ac.sum((0, 2))) if emulate else bd.sum((0, 2))
        if not magnitudes:
            continue
        aq_u, aq_v = (q + u.to(dtype)).abs() * scale, (q + vb.to(dtype)).abs() * scale
        mij = aq_u @ k.abs().transpose(-1, -2) + by_key(aq_v @ Rd.abs().transpose(-1, -2), sidx)
        g = 1 + mij.masked_fill(P < 2.0 ** -16, 0).max(-1, keepdim=True).values          # [.., T, 1]
        Pg = P * g
        aS = Pg * (dO.abs() @ v.abs().transpose(-1, -2) + (O * dO).abs().sum(-1, keepdim=True))
        aSd = by_dist(aS)
        mag["out"].append(Pg @ v.abs()), mag["lse"].append(g[..., 0].expand_as(lse).clone())
        aac, abd = scale * (aS @ k.abs()), scale * (aSd @ Rd.abs())
        mag["dq"].append(aac + abd), mag["dk"].append(aS.transpose(-1, -2) @ aq_u)
        mag["dv"].append(Pg.transpose(-1, -2) @ dO.abs())
        amag["drd"] += torch.einsum("bhid,bhif->hdf", aSd, aq_v)
        amag["du"] += aac.sum((0, 2))
        amag["dvb"] += abd.sum((0, 2))
    out = {}
    for n in res:
        out[n] = (torch.cat(res[n]).double(), torch.cat(mag[n]).double() if magnitudes else None)
    for n in acc:
        out[n] = (acc[n].double(), amag[n].double() if magnitudes else None)
    if defect == "drd_tail_zero":                        # every drd row below the old metric's floor is zero
        w = out["drd"][0].clone()
        w[hidden_drd_rows(w)] = 0
        out["drd"] = (w, out["drd"][1])
    return out


def hidden_drd_rows(drd):
    """[H, K] bool: the rows (distances) of drd that lie wholly under the old metric's floor, tolerance x the maximum."""
    return drd.abs().amax(-1) < OLD_TOL["drd"] * drd.abs().max()


def garbage(want, A):
    """zero_rows_garbage: {tensor: got} with 1 % of the tensor's maximum where the contract has no visible term."""
    got = {}
    for n in ("dk", "dv", "drd"):
        w = want[n].clone()
        w[A[n] == 0] = 0.01 * float(w.abs().max())
        got[n] = w
    return got


def bound(n, want, A):
    return RHO[n] * want.abs() + C[n] * A


def ratio(n, got, want, A):
    """|got - want| / bound per element; where the bound is zero: 0 for an exact zero, inf otherwise; NaN stays NaN."""
    err = (got.double() - want).abs()
    bd = bound(n, want, A)
    r = err / bd.clamp_min(1e-300)
    return torch.where((bd == 0) & (err == 0), torch.zeros_like(r), r)


def relerr(got, want):
    """The old metric of tests/test_kernels_gpu.py."""
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-12))


def locate(s, n, idx):
    """Human-readable position of flat index idx of tensor n."""
    DH = s.DH
    f = idx % DH
    if n == "lse":
        b, h, r = idx // (s.H * s.T), idx // s.T % s.H, idx % s.T
        return f"(b {b}, h {h}) row {r}"
    if n in ("du", "dvb"):
        return f"h {idx // DH} element {f}"
    if n == "drd":
        return f"h {idx // (s.K * DH)} distance {idx // DH % s.K} element {f}"
    R = s.T if n in ("out", "dq") else s.K
    b, h, r = idx // (s.H * R * DH), idx // (R * DH) % s.H, idx // DH % R
    return f"(b {b}, h {h}) row {r} element {f}"


def worst(s, n, got, want, A):
    """(worst ratio, message naming the element)."""
    r = ratio(n, got, want, A).nan_to_num(nan=math.inf)
    idx = int(r.argmax())
    return float(r.max()), (f"{n} {locate(s, n, idx)}: got {float(got.reshape(-1)[idx])}, want "
                            f"{float(want.reshape(-1)[idx])}, error {float(r.reshape(-1)[idx]):.3g} x the bound")


# ------------------------------------------------------------------------------------------------ input sets
class Set:
    pass


def _probe_vec(w, alpha, scale):
    w = w.double()
    return (alpha * w / (w * w).sum() / scale).to(torch.bfloat16)


PROBE_ROWS = (0, 63, 64, 127, 128)
DIST_SEAMS = (128, 256, 512, 1024)


def _visible_range(s, b, i):
    lo = 0
    if s.same_length:
        lo = max(lo, i - s.sshift + 1)
    if s.reset is not None and bool(s.reset[b]):
        lo = max(lo, s.M)
    return lo, i + s.M


def _key_candidates(s, b, i):
    """Keys worth probing from row i, most particular first: the causal edge, the first visible key, keys 0 / M / K - 1,
    both sides of every 64-key and 32-key seam in the row's range."""
    lo, hi = _visible_range(s, b, i)
    c = [(hi, "causal_edge"), (lo, "first_visible")]
    if s.reset is not None and bool(s.reset[b]) and lo == s.M:
        c = [(lo, "reset_first")] + c[:1]
    elif s.same_length and lo == i - s.sshift + 1 and lo > 0:
        # the same_length edge, before the causal edge except in the last row of a 64-row tile (own_key_tile_end)
        c = [(hi, "causal_edge"), (lo, "sl_edge")] if i % TILE == TILE - 1 else [(lo, "sl_edge"), (hi, "causal_edge")]
    for x in range(32, s.K, 32):
        for j, side in ((x - 1, "-"), (x, "+")):
            c.append((j, ("seam64" if x % 64 == 0 else "seam32") + side))
    return [(j, t) for j, t in c if lo <= j <= hi]


def _dist_candidates(s, b, i):
    lo, hi = _visible_range(s, b, i)
    dmax, dmin = i + s.M - lo, 0
    c = []
    for x in reversed(DIST_SEAMS):
        c += [(x - 1, f"d{x - 1}"), (x, f"d{x}")]
    c += [(0, "d0"), (dmax, "dmax")] + [(x, "d16") for x in (15, 16, 31, 32, 63, 64)]
    return [(d, t) for d, t in c if dmin <= d <= dmax]


def build(name, T, M, B, H, DH, same_length, mem_len, reset_col, seed):
    s = Set()
    s.name, s.T, s.M, s.B, s.H, s.DH, s.same_length, s.mem_len = name, T, M, B, H, DH, same_length, mem_len
    s.K, s.scale, s.sshift = T + M, 1.0 / math.sqrt(DH), sshift_of(T, M, mem_len)
    K, HD = s.K, H * DH
    s.reset = None
    if reset_col is not None:
        s.reset = torch.zeros(B, dtype=torch.uint8)
        s.reset[reset_col] = 1
    g = torch.Generator().manual_seed(seed)
    s.qkv = torch.full((K * B + XROWS, 3 * HD + PAD), math.nan, dtype=torch.bfloat16)
    s.qkv[:K * B, :3 * HD] = (_randn(g, K * B, 3 * HD) * 0.7).to(torch.bfloat16)
    s.rd = torch.full((K + XROWS, HD + PAD), math.nan, dtype=torch.bfloat16)
    s.rd[:K, :HD] = (_randn(g, K, HD) * 0.7).to(torch.bfloat16)
    s.u, s.vb = _randn(g, HD) * 0.3, _randn(g, HD) * 0.3
    s.dout = torch.full((T * B, HD + PAD), math.nan, dtype=torch.bfloat16)
    s.dout[:, :HD] = _randn(g, T * B, HD).to(torch.bfloat16)
    s.probes = []
    s.dist_shift_row = 0
    rows = sorted({i for i in PROBE_ROWS + (T - 1,) if i < T})
    used_d = {h: set() for h in range(H)}
    count = {}

    def pick(cand, i):
        """The candidate whose tag this row (i: a key probe) or the whole set (None: a distance probe) has probed least
        often so far (ties: the list's order)."""
        best = min(cand, key=lambda x: count.get((x[1], i), 0))
        count[(best[1], i)] = count.get((best[1], i), 0) + 1
        return best

    def aim(b, i, c, ja, jb):
        """dO of the probed row points along v_ja - v_jb, so that dP - delta, and with it dS of the two probed keys, is
        as large as the row allows (norm 8, the norm of a standard-normal row).  QUIET rows -- the last row of a 64-row tile
        -- scale both V rows and dO by 2^-8: every relative property stays, and the row's elements lie far below the floor of
        a whole-tensor metric."""
        quiet = 2.0 ** -8 if i % TILE == TILE - 1 else 1.0
        # LOUD: dO of the last row, where it is not a quiet one, is 4 times as long, so that the last query tile's share of
        # du and dvb, sums over every token row, stands out of the sum (du_last_tile)
        loud = 4.0 if i == T - 1 and quiet == 1.0 else 1.0
        va, vb_ = (s.qkv[j * B + b, 2 * HD:3 * HD][c].float() * quiet for j in (ja, jb))
        s.qkv[ja * B + b, 2 * HD:3 * HD][c], s.qkv[jb * B + b, 2 * HD:3 * HD][c] = va.to(torch.bfloat16), vb_.to(torch.bfloat16)
        dv = (va - vb_).double()
        s.dout[i * B + b, :HD][c] = (dv / (dv * dv).sum().sqrt() * 8.0 * quiet * loud).to(torch.bfloat16)

    for b in range(min(B, 4)):                            # (the first four sequences and two heads carry the probes)
        for h in range(min(H, 2)):
            used_j = set()
            c = slice(h * DH, (h + 1) * DH)
            for r, i in enumerate(rows):
                qrow = s.qkv[(M + i) * B + b, :HD][c].float()
                lo, hi = _visible_range(s, b, i)
                if hi - lo < 1:
                    continue
                if (b % 2 == 0) == (r % 2 == 1):
                    cand = [x for x in _dist_candidates(s, b, i) if x[0] not in used_d[h]]
                    if not cand:
                        continue
                    d, tag = pick(cand, None)
                    far = [x for x in range(0, hi - lo + 1) if x not in used_d[h] and abs(x - d) > (hi - lo) // 3]
                    if not far:
                        continue
                    a = far[len(far) // 2]
                    used_d[h] |= {d, a}
                    vec = _probe_vec(qrow + s.vb[c], ALPHA, s.scale)
                    s.rd[d, c], s.rd[a, c] = vec, vec
                    aim(b, i, c, i + M - d, i + M - a)
                    s.probes.append(dict(kind="dist", b=b, h=h, i=i, d=d, anchor=a, tag=tag))
                    s.dist_shift_row = i
                    continue
                cand = [x for x in _key_candidates(s, b, i) if x[0] not in used_j]
                if not cand:
                    continue
                j, tag = pick(cand, i)
                far = [x for x in range(lo, hi + 1) if x not in used_j and abs(x - j) > (hi - lo) // 3]
                if not far:
                    continue
                a = far[len(far) // 2]
                used_j |= {j, a}
                w = qrow + s.u[c]
                vec = _probe_vec(w, ALPHA, s.scale)
                s.qkv[j * B + b, HD:2 * HD][c], s.qkv[a * B + b, HD:2 * HD][c] = vec, vec
                # the key just beyond the edge would take the whole row if it counted at all
                hid = hi + 1 if tag == "causal_edge" else lo - 1 if tag in ("first_visible", "reset_first", "sl_edge") else None
                if hid is not None and 0 <= hid < K and hid not in used_j:
                    s.qkv[hid * B + b, HD:2 * HD][c] = _probe_vec(w, ALPHA + HIDDEN_EXTRA, s.scale)
                    used_j.add(hid)
                else:
                    hid = None
                aim(b, i, c, j, a)
                s.probes.append(dict(kind="key", b=b, h=h, i=i, j=j, anchor=a, tag=tag, hidden=hid))
    return s


# (T, M, B, H, same_length, mem_len, reset column)
SHAPES_32 = ((65, 0, 3, 2, False, 0, None), (129, 31, 3, 2, False, 31, 1), (1, 77, 2, 2, True, 4146, None),
             (64, 64, 4, 2, True, 64, None))
SHAPES_64 = SHAPES_32 + ((192, 130, 2, 1, True, 100, 1), (63, 0, 1, 1, False, 0, None), (200, 0, 1, 1, False, 0, None))
SHAPES_BAND = ((64, 0, 128, 1, False, 0, None), (128, 1024, 64, 1, False, 1024, None), (96, 32, 96, 2, True, 100, 3),
               (128, 0, 64, 10, False, 0, None), (64, 64, 128, 16, False, 64, None))


def _name(DH, sh):
    T, M, B, H, sl, ml, rc = sh
    return f"dh{DH}-T{T}-M{M}-B{B}-H{H}-{'same' if sl else 'nosame'}-ml{ml}-r{'x' if rc is None else rc}"


def all_sets():
    """(name, DH, shape, band) of every input set."""
    out = [(_name(32, sh), 32, sh, False) for sh in SHAPES_32]
    out += [(_name(64, sh), 64, sh, False) for sh in SHAPES_64]
    out += [(_name(64, sh), 64, sh, True) for sh in SHAPES_BAND]
    return out


NAMES = [x[0] for x in all_sets()]


@functools.lru_cache(maxsize=3)
def get(name):
    """The input set and its float64 contract, built once and shared (read-only)."""
    idx = NAMES.index(name)
    _, DH, sh, band = all_sets()[idx]
    s = build(name, sh[0], sh[1], sh[2], sh[3], DH, sh[4], sh[5], sh[6], 7000 + idx)
    s.band = band
    ref = contract(s)
    s.want = {n: ref[n][0] for n in TENSORS}
    s.A = {n: ref[n][1] for n in TENSORS}
    return s


# the set on which the host test plants each defect
DESIGNATED = {
    "causal_plus": _name(64, SHAPES_64[1]), "own_key_tile_end": _name(64, SHAPES_64[1]),
    "same_length_edge_plus": _name(64, SHAPES_64[4]), "same_length_edge_minus": _name(64, SHAPES_64[4]),
    "reset_edge": _name(64, SHAPES_64[4]), "kv_range_lo": _name(64, SHAPES_64[3]), "kv_range_hi": _name(64, SHAPES_64[1]),
    "seam_drop": _name(64, SHAPES_64[1]), "seam_dup": _name(32, SHAPES_32[1]), "dist_shift": _name(64, SHAPES_64[1]),
    "p_block_neighbour": _name(64, SHAPES_64[1]), "band_last_slice": _name(64, SHAPES_BAND[0]),
    "band_pass_seam": _name(64, SHAPES_BAND[1]), "drd_tail_zero": _name(64, SHAPES_64[6]),
    "zero_rows_garbage": _name(64, SHAPES_64[4]), "du_last_tile": _name(64, SHAPES_64[0]),
}


# WHERE THE BOUND IS BLIND (tests/test_attn_contract_host.py re-checks the lists): drd, du and dvb are sums over every token
# row; A adds the absolute terms, the value is what survives their cancellation (du: 1e-4 of A at 8192 rows), and the one
# constant per tensor is set by the set with the fewest rows (T = 1).  On these sets a result of EXACTLY ZERO passes the
# bound: there the check proves that nothing is read out of place (NaN guards), that the exact zeros hold and that the error
# stays below about the size of the value, and no more.  dvb is blind on every set but one.
ZERO_PASSES = {
    "drd": (NAMES[11],),
    "du": tuple(NAMES[11:]),
    "dvb": tuple(n for n in NAMES if n != _name(64, SHAPES_64[2])),
}
