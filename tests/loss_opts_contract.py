"""Float64 contracts of the loss-option kernels (csrc/elementwise.hip: ce_fwd_opts*, ce_bwd_opts*, nll_by_class*;
csrc/train_f32.hip: ce_bwd_opts_f32), in the manner of tests/train_contract.py, whose inputs, cases and helpers they use.
Plain module: torch and numpy on the CPU, nothing from the library.

THE FORMULAS, per row of V real logits l_j (eps = label smoothing, zeta = z-loss; the reference evaluates them on the fp32
VALUES of eps and zeta, which is what a kernel receives):
  lse    = log sum_j exp(l_j)
  nll    = lse - l_t
  smooth = lse - sum_j l_j / V
  loss   = (1 - eps) nll + eps smooth + zeta lse^2
  dl_j   = g [(1 + 2 zeta lse) softmax_j - (1 - eps) [j == t] - eps / V]

BOUNDS (u = 2^-24).  lse and nll keep train_contract's bound B0 = 2^-22 (|lse| + |l_t| + |nll|) + 2^-18 (ce_check_fwd).
loss   the three terms t1 = (1 - eps) nll, t2 = eps smooth, t3 = zeta lse^2 inherit the errors of their inputs,
         (1 - eps) B0  +  eps (B0 + 23 u mean_j |l_j| + u |smooth|)  +  2 zeta |lse| B0,
       where 23 u mean|l| is the running sum of the logits (a lane adds at most 16 of them, the butterfly 6 levels, one
       division) and u |smooth| its subtraction from lse; and they round at most four times each on the way into the sum
       (1 - eps, the products, lse * lse, the two additions): 4 u (|t1| + |t2| + |t3|).  A fused multiply-add only removes
       roundings.
dlogits  with a = 1 + 2 zeta lse, s_j = (1 - eps) [j == t] + eps / V, p = softmax (from the fp32 lse the kernel is given):
       train_contract's term for p, scaled by |a|:  |a| p (|l_j| + |lse| + 4) 2^-23;  a itself rounds twice
       (u (|2 zeta lse| + |a|), times p), the product a p once (u |a| p), s_j three times (eps / V, 1 - eps, their sum:
       3 u s_j), the difference once (u (|a| p + s_j)), and train_contract's absolute 2^-24 stays:
         rest = |g| (|a| p (|l_j| + |lse| + 4) 2^-23 + 2^-24 (3 |a| p + |2 zeta lse| p + 4 s_j + 1)),
       plus the output format's own rounding of the final product: 2^-8 |want| in bf16, 2^-24 |want| in fp32.  At
       eps = zeta = 0 this is train_contract's bound with 2^-24 (3 p + 4 [j == t]) added.  Figures NAME / NAME~ as there.
nll_by_class  sum[k]: the plain running-sum bound in the form of grad_norm_bound: a thread adds ceil(rows / (256 nblk)) values one
       after the other, the butterfly has 6 levels, the waves 3 additions, the final pass nblk: (depth + 8) u sum |nll|
       over the rows of the class.  count[k] is exact.
"""
import numpy as np
import torch

import train_contract as TC

U, F32 = TC.U, TC.F32
OPTS = ((0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4), (0.0, 0.0))          # (eps, zeta)
N_CLASSES = 8
NLL_ROWS = (1, 33, 4099)


def f32v(x):
    """the value a kernel receives for a float argument, as float64"""
    return float(F32(x))


def opts_ref(inp, eps, zeta):
    eps, zeta = f32v(eps), f32v(zeta)
    ref = TC.ce_ref(inp)
    x = inp.x[:, :inp.V].astype(np.float64)
    smooth = ref["lse"] - x.sum(1) / inp.V
    t1, t2, t3 = (1.0 - eps) * ref["nll"], eps * smooth, zeta * ref["lse"] ** 2
    return dict(ref, smooth=smooth, t1=t1, t2=t2, t3=t3, loss=t1 + t2 + t3, meanabs=np.abs(x).sum(1) / inp.V)


def check_fwd(inp, eps, zeta, loss, nll, lse):
    r = opts_ref(inp, eps, zeta)
    e, z = f32v(eps), f32v(zeta)
    b0 = 2.0 ** -22 * (np.abs(r["lse"]) + np.abs(r["xt"]) + np.abs(r["nll"])) + 2.0 ** -18
    bl = (1.0 - e) * b0 + e * (b0 + 23 * U * r["meanabs"] + U * np.abs(r["smooth"])) + 2.0 * z * np.abs(r["lse"]) * b0 \
        + 4 * U * (np.abs(r["t1"]) + np.abs(r["t2"]) + np.abs(r["t3"]))
    return dict(lse=TC.ratio(lse, r["lse"], b0), nll=TC.ratio(nll, r["nll"], b0), loss=TC.ratio(loss, r["loss"], bl))


def grad_ref(inp, lse32, eps, zeta):
    """(want, rest) [rows, V] in float64, from the fp32 lse the backward kernel is given"""
    eps, zeta = f32v(eps), f32v(zeta)
    V = inp.V
    x = inp.x[:, :V].astype(np.float64)
    l, g = lse32.astype(np.float64)[:, None], inp.g.astype(np.float64)[:, None]
    p = np.exp(x - l)
    a = 1.0 + 2.0 * zeta * l
    s = (1.0 - eps) * (np.arange(V)[None, :] == inp.target[:, None]) + eps / V
    want = g * (a * p - s)
    rest = np.abs(g) * (np.abs(a) * p * (np.abs(x) + np.abs(l) + 4) * 2.0 ** -23
                        + 2.0 ** -24 * (3 * np.abs(a) * p + np.abs(2.0 * zeta * l) * p + 4 * s + 1)) + 1e-300
    return want, rest


def check_bwd(inp, lse32, eps, zeta, dlogits, ldd, bits=8):
    """dlogits [rows, ldd] (bits 8: bf16, 24: fp32): every column of the pitch is written, [V, ldd) as zero."""
    V = inp.V
    want, rest = grad_ref(inp, lse32, eps, zeta)
    own = 2.0 ** -bits * np.abs(want)
    d = np.asarray(dlogits, dtype=np.float64)
    ok = d.shape == (inp.rows, ldd) and bool(np.all(d[:, V:] == 0.0))
    return {"dlogits": TC.ratio(d[:, :V], want, own + rest), "dlogits~": TC.excess(d[:, :V], want, bits, rest),
            "guard": 0.0 if ok else float("inf")}


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulations with the kernels' index mapping (train_contract._ce_index) and plantable defects
FWD_DEFECTS = ("uniform_over_ld", "pad_in_sum", "eps_on_nll")
BWD_DEFECTS = ("uniform_over_ld", "z_on_onehot", "eps_on_nll")


def fwd_emu(inp, eps, zeta, defect=None):
    V, ldl, rows = inp.V, inp.ldl, inp.rows
    eps, zeta = F32(eps), F32(zeta)
    nll, lse = TC.ce_fwd_emu(inp)                              # max, sum and lse: the plain kernel's operations
    idx = TC._ce_index(V, ldl, TC.ce_vec_fwd(V, ldl))
    lim = ldl if defect == "pad_in_sum" else V                 # DEFECT: pad columns [V, ldl) enter sum l_j
    valid = idx < lim
    with np.errstate(all="ignore"):
        xg = inp.x[:, np.minimum(idx, ldl - 1)]
        sl = np.zeros((rows, 64), F32)
        for j in range(idx.shape[1]):
            sl = sl + np.where(valid[:, j], xg[:, :, j], F32(0)).astype(F32)
        sl = TC.wave_sum(sl)[:, 0]
        n = F32(ldl if defect == "uniform_over_ld" else V)     # DEFECT: the uniform term over the row pitch
        sm = (lse - (sl / n).astype(F32)).astype(F32)
        w = eps if defect == "eps_on_nll" else (F32(1) - eps).astype(F32)          # DEFECT: eps weighs the nll too
        loss = (((w * nll).astype(F32) + (eps * sm).astype(F32)).astype(F32) + (zeta * (lse * lse).astype(F32)).astype(F32))
    return loss.astype(F32), nll, lse


def bwd_emu(inp, lse32, eps, zeta, ldd, defect=None, bits=8):
    V, ldl = inp.V, inp.ldl
    eps, zeta = F32(eps), F32(zeta)
    c = np.arange(ldd)
    with np.errstate(all="ignore"):
        l = lse32[:, None]
        a = (F32(1) + (F32(2) * zeta * l).astype(F32)).astype(F32)
        n = F32(ldl if defect == "uniform_over_ld" else V)     # DEFECT: eps / ld
        u = (eps / n).astype(F32)
        w = eps if defect == "eps_on_nll" else (F32(1) - eps).astype(F32)          # DEFECT: eps on the one-hot term
        ut = (w + u).astype(F32)
        xg = inp.x[:, np.minimum(c, ldl - 1)]
        p = np.exp((xg - l).astype(F32)).astype(F32)
        hot = c[None, :] == inp.target[:, None]
        if defect == "z_on_onehot":                            # DEFECT: the z-loss factor scales the one-hot term as well
            v = ((a * (p - np.where(hot, w, F32(0))).astype(F32)).astype(F32) - u).astype(F32)
        else:
            v = ((a * p).astype(F32) - np.where(hot, ut, u)).astype(F32)
        v = (inp.g[:, None] * v).astype(F32)
        v = np.where(c[None, :] < V, v, F32(0)).astype(F32)
    return TC.bf16_round(v) if bits == 8 else v


# ---------------------------------------------------------------------------------------------------------------------
# per-class NLL
class NllInputs:
    """nll [rows] fp32, target [rows] in [0, V) with pad (0) rows, and a class table [V] that uses every class."""

    def __init__(self, rows, V=729, pad=0):
        g = torch.Generator().manual_seed(11 * rows + V)
        self.rows, self.V, self.pad = rows, V, pad
        self.nll = (6.0 * torch.rand(rows, generator=g)).numpy().astype(F32)
        self.target = torch.randint(0, V, (rows,), generator=g).numpy().astype(np.int64)
        self.target[::5] = pad                                 # rows of loss weight 0
        if rows > 1:
            self.target[1] = V - 1
        self.table = ((np.arange(V) * 7) // 3 % N_CLASSES).astype(np.int32)


def nll_blocks(rows):
    """commu_nll_by_class_blocks"""
    return min(max((rows + 1023) // 1024, 1), 256)


def nll_by_class_ref(inp):
    live = inp.target != inp.pad
    cls = inp.table[inp.target]
    sums = np.array([inp.nll[live & (cls == k)].astype(np.float64).sum() for k in range(N_CLASSES)])
    mags = np.array([np.abs(inp.nll[live & (cls == k)].astype(np.float64)).sum() for k in range(N_CLASSES)])
    cnts = np.array([int((live & (cls == k)).sum()) for k in range(N_CLASSES)], dtype=np.int64)
    return sums, mags, cnts


def nll_by_class_bound(rows, nblk, mags):
    depth = (rows + 256 * nblk - 1) // (256 * nblk) + 6 + 3 + nblk
    return (depth + 8) * U * mags + 1e-300


def nll_by_class_check(inp, got_sum, got_cnt):
    sums, mags, cnts = nll_by_class_ref(inp)
    ok = np.array_equal(np.asarray(got_cnt, dtype=np.int64), cnts)
    return {"sum": TC.ratio(got_sum, sums, nll_by_class_bound(inp.rows, nll_blocks(inp.rows), mags)),
            "count": 0.0 if ok else float("inf")}
