"""Host-side contract of the decode layer tail and head (csrc/decode_tail.hip: commu_decode_layer_tail, commu_decode_head,
commu_decode_tail_pack) and the input sets that the kernel test and the host test share.  Plain module, CPU tensors only.

A launch leaves every intermediate in memory, each written once, so the contract is STAGED: every stage is checked from
what the launch itself stored for the stage before it -- one product plus one rounding per stage, nothing propagates.

    S1   z1    = bf16(vec . Wo^T + h)                      from the launch inputs
    S2   hid   = bf16(relu(a . W1^T + b1)),  a = bf16(LN1(z1))   from the stored z1
    S3   z2    = bf16(hid . W2^T + b2 + a)                 from the stored hid and the same a
    S4a  h_out = bf16(LN2(z2))                             from the stored z2
    S4b  out   = h_out . Wn^T   (bf16, QKV mode)  |  + bn (fp32, LOGITS mode)      from the stored h_out
    head h_out = bf16(E[tok] scale), zero pad columns, NaN rows for ids outside [0, V);  qkv = bf16(h_out . Wqkv^T)

PRODUCT STAGES, per element:  |got - want| <= 2^-8 |want| + C_PROD A  for bf16 outputs and  C_PROD A  for fp32 logits, with
A = sum |x| |w| + |bias| + |residual|; want and A in float64.  C_PROD = 16 e32 rounded up to a power of two, where e32 is
the largest |float32 evaluation - float64| / A over every input set of this module; the float32 evaluation runs in the
kernels' order (four K quarters, each accumulated over its 32-wide steps in sequence, then added; a 32-wide step is a
fixed pairwise tree) as elementwise IEEE operations, so it is the same number on every host.  Measured (the host test
prints and re-checks them):  e32 = 5.01e-8 (S1 3.13e-8, S2 5.01e-8, S3 3.29e-8, S4b 3.42e-8, head 3.57e-8: one
constant serves every stage kind), 16 e32 = 8.0e-7, C_PROD = 2^-20 = 9.5e-7.

LAYERNORM STAGES.  S4a is observable: bit equality with bf16(LN in float64) except where the float64 value y lies within
TAU (|(x - mu) rs gamma| + |beta|) of the midpoint of two neighbouring bf16 values; there the other neighbour is allowed
too.  TAU = 16 x the float32-vs-float64 error of the LayerNorm evaluation (kernel order: per lane, pairs of lanes, four
waves; rs = 1 / sqrt) on these inputs relative to that magnitude, rounded up to a power of two: measured eLN = 2.26e-7,
TAU = 2^-18 (ln_rule has the exact wording).  a = bf16(LN1(z1)) is not stored: the S2 bound gains
sum |W1[n, k]| reach(a_k) over the near-tie k (reach = ulp + TAU x magnitude), the S3 bound reach(a_n) where a_n is near
a tie.  The loophole is capped: at most d_ln / 32 near-tie elements in a row (TIE_CAP); the checks return the occupancy
of the cap.  The W2 = 0, b2 = 0 sets make a itself observable (z2 = a exactly) and hold it to the S4a rule.

INPUTS.  Weights O(1 / sqrt K); biases, gamma, beta O(1) and different in every column (|beta| >= 0.25: where beta is 0
and x is next to the mean, the result is the mean's own rounding error and eLN measures nothing else); eps1 = 1e-5,
eps2 = 1e-3.  Row 0 has a tiny variance before LN1 (vec, h ~ 2^-9: var ~ 8e-6 < eps1); row 1, where d_ln is a power of two, is 2 or
2 - 2^-7 (mean 750 x its standard deviation, and every float32 sum of the two-pass evaluation exact, which is what
keeps eLN small; with d_ln = 500 the mean's own rounding would be 2e-4 of the result, so those sets do without).  The
W2 = 0 sets scale gamma1 / beta1 by 2^-6 so that LN2 sees a variance below eps2.  Zero-padded sets (d_ln 500 in D 512,
1000 in 1024): h carries NaN in its pad columns, so z1's come out NaN; W2 / b2 are random in the pad rows, so z2's are
finite garbage; LayerNorm must ignore both, a's and h_out's pad columns must be exactly zero.

DEFECTS (run(..., defect=name)): each the image of one line of decode_tail.hip going wrong; the host test proves that
every one breaks a bound or an exactness check on sub-batches of the sets built here."""
import functools
import math

import torch


def _rng(seed):
    """(generator, randn) with standard-normal-like draws that are the same bits on every machine (as
    decode_contract._randn: the centred sum of six uniform bytes, a pool of 2^20 values sampled with replacement)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 2 ** 48, (2 ** 20,), generator=g)
    pool = sum((r >> (8 * i)) & 255 for i in range(6))
    pool = ((pool - 765).double() / math.sqrt(6 * (256 ** 2 - 1) / 12)).float()
    return g, lambda *shape: pool[torch.randint(0, 2 ** 20, shape, generator=g)]

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
C_PROD = 2.0 ** -20
TAU = 2.0 ** -18
TIE_CAP = 1.0 / 32          # near-tie elements per row, of d_ln
EPS1, EPS2 = 1e-5, 1e-3
SENT = 768.0                 # (exact in bf16)
SYNC_SENT = 0x5A5A5A5A
NGRP, CNT_STRIDE = 32, 64
V = 729
PAD = 8
SHAPES = {"n512": (512, 1024, 512), "n640": (512, 1024, 640), "wide": (1024, 2048, 1024)}

PRODUCT_STAGES = ("S1", "S2", "S3", "S4b")
# defect -> stages it can be planted in ("": no stage argument)
DEFECTS = {
    "drop_chunk": PRODUCT_STAGES, "drop_wave": PRODUCT_STAGES, "tile_swap": PRODUCT_STAGES, "bias_tile0": ("S2", "S3", "S4b"),
    "no_relu": ("",), "relu_before_bias": ("",), "resid_z1": ("",), "p4_reads_z1": ("",),
    "ln_stats_D": ("S2", "S4a"), "ln_stats_pad": ("S2", "S4a"), "ln_one_pass": ("S2",), "ln_clamp_last": ("S2", "S4a"),
    "eps_swap": ("S2", "S4a"), "group0": ("S2", "S3", "S4a"), "inactive_written": ("",), "logits_tail": ("",),
}
HEAD_DEFECTS = ("drop_chunk", "drop_wave", "tile_swap", "no_scale", "bad_id_row0")


# ------------------------------------------------------------------------------------------------ arithmetic
def bf(x):
    return x.to(BF16)


def ulp_bf16(y):
    """Spacing of bf16 at |y| (float64)."""
    _, e = torch.frexp(y.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(y), e - 8)


def _tree32(p):
    """[32, ...] -> [...]: fixed pairwise tree (i with i + 16, then + 8, ...)."""
    n = 32
    while n > 1:
        n //= 2
        p = p[:n] + p[n:2 * n]
    return p[0]


_STEPS = {}


def _steps(W):
    """W [N, K] as float32 [K, N], kept per weight tensor."""
    key = (W.data_ptr(), W._version, tuple(W.shape))
    if key not in _STEPS:
        if len(_STEPS) > 24:
            _STEPS.clear()
        _STEPS[key] = (W, W.float().T.contiguous())
    return _STEPS[key][1]


def prod32(x, W, drop_chunk=None, drop_wave=None):
    """x [B, K] . W [N, K]^T in float32, the kernels' order: wave w takes K quarter w in K / 128 steps of 32, the four
    partial sums are added 0 + 1 + 2 + 3.  drop_chunk (w, ks, g): that 8-element chunk of x is missing; drop_wave: that
    quarter is missing from the sum."""
    x, Wt = x.float(), _steps(W)
    B, K = x.shape
    KS = K // 128
    N = Wt.shape[1]
    if drop_chunk is not None:
        w, ks, g = drop_chunk
        x = x.clone()
        k = w * 32 * KS + 32 * ks + 8 * g
        x[:, k:k + 8] = 0
    out = torch.empty(B, N, dtype=F32)
    for r0 in range(0, B, 8):
        xs = x[r0:r0 + 8].T.contiguous()
        q = []
        for w in range(4):
            acc = torch.zeros(xs.shape[1], N, dtype=F32)
            for ks in range(KS):
                k = w * 32 * KS + 32 * ks
                acc = acc + _tree32(xs[k:k + 32, :, None] * Wt[k:k + 32, None, :])
            q.append(acc)
        if drop_wave is not None:
            q[drop_wave] = torch.zeros_like(q[0])
        out[r0:r0 + 8] = ((q[0] + q[1]) + q[2]) + q[3]
    return out


_DOUBLES = {}


def prod64(x, W):
    """(x . W^T, |x| . |W|^T) in float64 (matrix products: nothing of size B N K is materialised)."""
    key = (W.data_ptr(), W._version, tuple(W.shape))
    if key not in _DOUBLES:
        if len(_DOUBLES) > 24:
            _DOUBLES.clear()
        _DOUBLES[key] = (W, W.double().T.contiguous(), W.double().abs().T.contiguous())
    x = x.double()
    return x @ _DOUBLES[key][1], x.abs() @ _DOUBLES[key][2]


def ln64(x, g, b, eps, d_ln):
    """(y, magnitude) [B, d_ln] of LayerNorm over the first d_ln columns, float64."""
    x = x[:, :d_ln].double()
    mu = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    t = (x - mu) * rs * g.double()
    return t + b.double(), t.abs() + b.double().abs()


def _lane_sum(x, D):
    """Sum over the D columns of x [B, D] in the kernels' order: lane (w, g) adds its 8-element chunks in sequence, the
    four lanes of a row in a wave pair up (g ^ 1, then g ^ 2), the four waves add 0 + 1 + 2 + 3."""
    B = x.shape[0]
    KS = D // 128
    X = x.view(B, 4, KS, 4, 8)
    v = torch.zeros(B, 4, 4, dtype=x.dtype)
    for ks in range(KS):
        for e in range(8):
            v = v + X[:, :, ks, :, e]
    s = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
    return (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3])[:, None]


def ln32(x, g, b, eps, d_ln, defect=None):
    """LayerNorm of x [B, D] (float32 values) in float32 and the kernels' order -> [B, D] float32 with zero pad columns."""
    x = x.float()
    B, D = x.shape
    inr = (torch.arange(D) < d_ln)[None]
    count_pad = defect == "ln_stats_pad"
    xm = x if count_pad else torch.where(inr, x, torch.zeros_like(x))
    n = torch.tensor(float(D if defect in ("ln_stats_D", "ln_stats_pad") else d_ln), dtype=F32)
    mu = _lane_sum(xm, D) / n
    if defect == "ln_one_pass":
        var = _lane_sum(xm * xm, D) / n - mu * mu
    else:
        c = (x - mu) * (x - mu)
        var = _lane_sum(c if count_pad else torch.where(inr, c, torch.zeros_like(c)), D) / n
    rs = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    gg, bb = torch.zeros(D), torch.zeros(D)
    gg[:d_ln], bb[:d_ln] = g, b
    if defect == "ln_clamp_last":          # min(k, d_ln - 8) instead of d_ln - 4: the last chunk gets its neighbour's
        gg[d_ln - 4:d_ln], bb[d_ln - 4:d_ln] = g[d_ln - 8:d_ln - 4], b[d_ln - 8:d_ln - 4]
    y = (x - mu) * rs * gg + bb
    return torch.where(inr, y, torch.zeros_like(y))


def ln_rule(got, x, g, b, eps, d_ln):
    """The LayerNorm rule: (violations, near-tie mask [B, d_ln], bf16(LN64) [B, d_ln] float64, how far a near-tie element
    may be from it).  got [B, >= d_ln] or None.  An element passes if it is the bf16 rounding of some value within TAU x
    magnitude of y: bf16(y) itself everywhere; the other neighbour where y is that close to the midpoint; and where the
    two terms of y cancel below 2^8 TAU of their magnitude (then the window spans several of y's tiny ulps) any bf16
    value inside the window."""
    y, mag = ln64(x, g, b, eps, d_ln)
    r = bf(y.float()).double()
    u = ulp_bf16(y)
    tie = (u / 2 - (y - r).abs()) <= TAU * mag
    reach = (u + TAU * mag) * tie
    if got is None:
        return 0, tie, r, reach
    gd = got[:, :d_ln].double()
    ok = (gd == r) | (tie & ((gd - y).abs() <= u / 2 + TAU * mag))
    return int((~ok).sum()), tie, r, reach


# ------------------------------------------------------------------------------------------------ the layer tail
class TailSet:
    """One layer-tail launch's operands (CPU, logical shapes; pitches and sentinels: buffers())."""

    def sub(self, rows):
        """The same launch restricted to some rows (rows are independent but for their row group)."""
        s = TailSet()
        s.__dict__.update(self.__dict__)
        s.rows = [self.rows[i] for i in rows]
        s.B = len(rows)
        s.vec, s.h = self.vec[rows], self.h[rows]
        s.active = None if self.active is None else self.active[rows]
        return s


@functools.lru_cache(maxsize=8)
def _weights(shape, Nn, seed):
    D, DI, HD = SHAPES[shape]
    g, rn = _rng(seed)
    _randn = lambda g, *shape: rn(*shape)
    w = lambda n, k: bf(_randn(g, n, k) / math.sqrt(k))
    away = lambda t: t + torch.where(t < 0, -0.25, 0.25)          # (|beta| >= 0.25: see INPUTS)
    return dict(Wo=w(D, HD), W1=w(DI, D), W2=w(D, DI), Wn=w(Nn, D), b1=_randn(g, DI), b2=_randn(g, D), bn=_randn(g, Nn),
                g1=1.0 + 0.5 * _randn(g, D), be1=away(_randn(g, D)), g2=1.0 + 0.5 * _randn(g, D), be2=away(_randn(g, D)),
                vec=bf(_randn(g, 64, HD)), h=bf(_randn(g, 64, D)), tiny=bf(_randn(g, D) * 2.0 ** -9), tinyv=bf(_randn(g, HD) * 2.0 ** -9),
                big=bf(2.0 - 2.0 ** -7 * (torch.randperm(D, generator=g) < D // 8 - 3).float()))


def build_tail(shape, B, mode, d_ln, w2zero=False):
    D, DI, HD = SHAPES[shape]
    s = TailSet()
    s.shape, s.D, s.DI, s.HD, s.B, s.mode, s.d_ln, s.w2zero = shape, D, DI, HD, B, mode, d_ln, w2zero
    s.wide = shape == "wide"
    s.Nn = V if mode == "logits" else 3 * HD
    base = _weights(shape, s.Nn, 7000 + D + HD + s.Nn)
    for k in ("Wo", "W1", "W2", "Wn", "b1", "b2", "bn"):
        setattr(s, k, base[k].clone())
    for k in ("g1", "be1", "g2", "be2"):          # (exactly d_ln floats)
        setattr(s, k, base[k][:d_ln].clone())
    if w2zero:
        s.W2.zero_()
        s.b2.zero_()
        s.g1 *= 2.0 ** -6
        s.be1 *= 2.0 ** -6
    s.eps1, s.eps2 = EPS1, EPS2
    s.vec, s.h = base["vec"][:B].clone(), base["h"][:B].clone()
    s.vec[0], s.h[0] = base["tinyv"], base["tiny"]
    s.big_row = None
    if B > 1 and d_ln & (d_ln - 1) == 0:
        s.vec[1], s.h[1] = 0, base["big"]
        s.big_row = 1
    s.h[:, d_ln:] = math.nan
    s.rows = list(range(B))
    s.active = None
    if mode == "logits" and B > 3:
        s.active = torch.ones(B, dtype=torch.uint8)
        s.active[[2, B - 1]] = 0
    return s


def buffers(s):
    """The launch's output buffers before the launch: sentinels everywhere (extra rows, pad columns, the hand-off
    buffers), the arrival counters of the row groups in use zero and every other word of the sync block a sentinel."""
    B = s.B
    out_dt = F32 if s.mode == "logits" else BF16
    nout = 736 if s.mode == "logits" else s.Nn + PAD
    b = dict(z1=torch.full((B + 2, s.D), SENT, dtype=BF16), hid=torch.full((B + 2, s.DI), SENT, dtype=BF16),
             z2=torch.full((B + 2, s.D), SENT, dtype=BF16), h_out=torch.full((B + 2, s.D + PAD), SENT, dtype=BF16),
             out=torch.full((B + 2, nout), SENT, dtype=out_dt),
             sync=torch.full((12 * CNT_STRIDE + 64,), SYNC_SENT, dtype=torch.int32), err=torch.zeros(1, dtype=torch.int32))
    for w in counter_words(s):
        b["sync"][w] = 0
    return b


def counter_words(s):
    ngroups = (max(s.rows) + 16) // 16
    return [(p * 4 + mg) * CNT_STRIDE for p in range(3) for mg in range(ngroups)]


def _swap_tiles(t, ng=3):
    """Column tiles 0 and 1 of workgroup ng exchanged (output columns 16 ng .. + 16 and 16 (ng + 32) .. + 16)."""
    t = t.clone()
    a, b = slice(16 * ng, 16 * ng + 16), slice(16 * (ng + NGRP), 16 * (ng + NGRP) + 16)
    n = min(t.shape[1] - b.start, 16)
    ta = t[:, a].clone()
    t[:, a.start:a.start + n] = t[:, b.start:b.start + n]
    t[:, b.start:b.start + n] = ta[:, :n]
    return t


def _tile0(bias):
    """Tile 0's bias for every tile: column c of tile t reads bias[c - 512 t]."""
    return bias[torch.arange(bias.numel()) % 512]


_FIRST = {"no_relu": "S2", "relu_before_bias": "S2", "resid_z1": "S3", "p4_reads_z1": "S4a", "inactive_written": "S5",
          "logits_tail": "S5", None: "S5"}
_ORDER = ("S1", "S2", "S3", "S4a", "S4b", "S5")


def window(s, defect, stage):
    """The stages that a defect run evaluates anew and that its check looks at."""
    first = _ORDER.index(stage or _FIRST[defect])
    last = max(first, 2) if s.w2zero and first < 3 else first
    return _ORDER[first:last + 1]


def run(s, b, defect=None, stage="", use_active=True, base=None):
    """The launch in float32 and the kernels' order, rounded to the output types, written into the buffers b.  Also leaves
    b["_pre"]: every stage's float32 value before the rounding (for e32 / eLN).  defect / stage: see DEFECTS.  base: the
    buffers of a run of the same set without a defect: only the defect's own stage is evaluated anew (in the W2 = 0 sets
    also S3, which shows a), every other stage is taken over -- for check(..., stages=window(...))."""
    B, D, d_ln = s.B, s.D, s.d_ln
    KSD = D // 128
    pre = {}
    live = _ORDER if base is None else window(s, defect, stage)

    def reuse(name, key):
        if name not in live:
            pre[key] = base["_pre"][key]
            return True
        return False
    chunk = {"S1": (1, 0, 2), "S2": (2, KSD - 1, 3), "S3": (0, 1, 1), "S4b": (3, 0, 0)}

    def product(name, x, W):
        kw = {}
        if stage == name and defect == "drop_chunk":
            kw["drop_chunk"] = chunk[name]
        if stage == name and defect == "drop_wave":
            kw["drop_wave"] = 3
        acc = prod32(x, W, **kw)
        return _swap_tiles(acc) if stage == name and defect == "tile_swap" else acc

    def ln_defect(name):
        return defect if stage == name and defect in ("ln_stats_D", "ln_stats_pad", "ln_one_pass", "ln_clamp_last") else None

    def group0(name, t):          # rows of row groups > 0 read row group 0's rows of the hand-off buffer
        if stage == name and defect == "group0":
            full = torch.zeros(64, t.shape[1], dtype=t.dtype)
            full[s.rows] = t
            return full[[r % 16 for r in s.rows]]
        return t

    e1, e2 = (s.eps2, s.eps1) if defect == "eps_swap" and stage == "S2" else (s.eps1, s.eps2)
    if defect == "eps_swap" and stage == "S4a":
        e2 = s.eps1
    # phase 1
    if not reuse("S1", "S1"):
        pre["S1"] = product("S1", s.vec, s.Wo) + s.h.float()
    z1 = bf(pre["S1"])
    b["z1"][:B] = z1
    # phase 2
    if reuse("S2", "LN1"):
        reuse("S2", "acc2")
    else:
        pre["LN1"] = ln32(group0("S2", z1).float(), s.g1, s.be1, e1, d_ln, ln_defect("S2"))
        if base is not None and defect in ("bias_tile0", "no_relu", "relu_before_bias"):
            pre["acc2"] = base["_pre"]["acc2"]
        else:
            pre["acc2"] = product("S2", bf(pre["LN1"]), s.W1)
    a = bf(pre["LN1"])
    b1 = _tile0(s.b1) if stage == "S2" and defect == "bias_tile0" else s.b1
    acc = pre["acc2"]
    pre["S2"] = acc + b1
    hid = pre["S2"] if defect == "no_relu" else torch.relu(acc) + b1 if defect == "relu_before_bias" else torch.relu(pre["S2"])
    hid = bf(hid)
    b["hid"][:B] = hid
    # phase 3
    b2 = _tile0(s.b2) if stage == "S3" and defect == "bias_tile0" else s.b2
    res = z1.float().nan_to_num(0.0) if defect == "resid_z1" else a.float()
    if not reuse("S3", "S3"):
        pre["S3"] = product("S3", group0("S3", hid), s.W2) + (b2 + res)
    z2 = bf(pre["S3"])
    b["z2"][:B] = z2
    # phase 4
    x4 = z1 if defect == "p4_reads_z1" else z2
    if not reuse("S4a", "LN2"):
        pre["LN2"] = ln32(group0("S4a", x4).float(), s.g2, s.be2, e2, d_ln, ln_defect("S4a"))
    ho = bf(pre["LN2"])
    b["h_out"][:B, :D] = ho
    if not reuse("S4b", "acc4"):
        pre["acc4"] = product("S4b", ho, s.Wn)
    acc = pre["acc4"]
    if s.mode == "logits":
        bn = _tile0(s.bn) if stage == "S4b" and defect == "bias_tile0" else s.bn
        pre["S4b"] = acc + bn
        rows = torch.ones(B, dtype=torch.bool)
        if s.active is not None and use_active and defect != "inactive_written":
            rows = s.active != 0
        b["out"][:B][rows, :s.Nn] = pre["S4b"][rows]
        if defect == "logits_tail":
            n4 = (s.Nn + 3) // 4 * 4
            b["out"][:B][rows, s.Nn:n4] = (acc[:, -1:] + bn[-1])[rows].expand(-1, n4 - s.Nn)
    else:
        pre["S4b"] = acc
        b["out"][:B, :s.Nn] = bf(acc)
    for w in counter_words(s):
        b["sync"][w] = NGRP
    b["_pre"] = pre
    return b


def _ratio(got, want, A, bf16, slack=None):
    bound = (2.0 ** -8 * want.abs() if bf16 else 0) + C_PROD * A
    if slack is not None:
        bound = bound + slack
    r = (got.double() - want).abs() / bound.clamp_min(1e-300)
    return float(r.nan_to_num(nan=math.inf).max()) if r.numel() else 0.0


def _e32(pre, want, A):
    return float(((pre.double() - want).abs() / A.clamp_min(1e-300)).max())


INF = math.inf


def check(s, b, use_active=True, stages=_ORDER):
    """Every stage contract and every guard on the buffers after a launch (or after run()).  Returns {name: ratio}: the worst
    error / bound of the product stages, the number of violations of the exactness checks (S4a, LN1 in the W2 = 0 sets,
    pad columns, sentinels, inactive rows, sync block: 0 is a pass, anything else counts as inf by ok()), "tiecap": the
    occupancy of the tie cap; with b["_pre"] also e32 per stage and eLN.  stages: the stages to look at (others: 0)."""
    B, D, DI, d_ln, Nn = s.B, s.D, s.DI, s.d_ln, s.Nn
    res, pre = {}, b.get("_pre")
    z1, hid, z2, ho, out = b["z1"][:B], b["hid"][:B], b["z2"][:B], b["h_out"][:B, :D], b["out"][:B, :Nn]
    bad = 0
    res.update({k: 0.0 for k in PRODUCT_STAGES + ("tiecap", "S4a")})
    # S1
    if "S1" in stages:
        want, A = prod64(s.vec, s.Wo)
        hh = s.h[:, :d_ln].double()
        want, A = want[:, :d_ln] + hh, A[:, :d_ln] + hh.abs()
        res["S1"] = _ratio(z1[:, :d_ln], want, A, True)
        bad += int((~z1[:, d_ln:].isnan()).sum())                 # (h's pad columns are NaN: so are z1's)
        if pre:
            res["e32_S1"] = _e32(pre["S1"][:, :d_ln], want, A)
    # S2: a = bf16(LN1(z1)) up to its near-tie elements
    _, tie, a, ua = ln_rule(None, z1.float(), s.g1, s.be1, s.eps1, d_ln)
    res["tiecap"] = float(tie.sum(1).max()) / (TIE_CAP * d_ln)
    apad = torch.zeros(B, D, dtype=F64)
    apad[:, :d_ln] = a
    if "S2" in stages:
        want, A = prod64(apad, s.W1)
        want, A = want + s.b1.double(), A + s.b1.double().abs()
        res["S2"] = _ratio(hid, torch.relu(want), A, True, prod64(ua, s.W1[:, :d_ln])[1])
    if pre and "S2" in stages:
        y, mag = ln64(z1.float(), s.g1, s.be1, s.eps1, d_ln)
        res["eLN"] = float(((pre["LN1"][:, :d_ln].double() - y).abs() / mag).max())
        # (e32 from the honest a, which may differ from `a` at a near-tie element: computed only where it does not)
        if torch.equal(bf(pre["LN1"]).double()[:, :d_ln], a):
            res["e32_S2"] = _e32(pre["S2"], want, A)
    # S3
    if "S3" in stages:
        want, A = prod64(hid, s.W2)
        want, A = want + s.b2.double() + apad, A + s.b2.double().abs() + apad.abs()
        slack = torch.zeros(B, D, dtype=F64)
        slack[:, :d_ln] = ua
        res["S3"] = _ratio(z2, want, A, True, slack)
        if pre and "e32_S2" in res:
            res["e32_S3"] = _e32(pre["S3"], want, A)
    if s.w2zero and "S3" in stages:                                                 # z2 is a: LN1's output, observable
        n = ln_rule(z2.float(), z1.float(), s.g1, s.be1, s.eps1, d_ln)[0]
        res["LN1"] = n
        bad += int((z2[:, d_ln:] != 0).sum())
    # S4a
    if "S4a" in stages:
        n, tie2, _, _ = ln_rule(ho.float(), z2.float(), s.g2, s.be2, s.eps2, d_ln)
        res["S4a"] = n
        res["tiecap"] = max(res["tiecap"], float(tie2.sum(1).max()) / (TIE_CAP * d_ln))
        bad += int((ho[:, d_ln:] != 0).sum())
    if pre and "S4a" in stages:
        y, mag = ln64(z2.float(), s.g2, s.be2, s.eps2, d_ln)
        res["eLN"] = max(res.get("eLN", 0.0), float(((pre["LN2"][:, :d_ln].double() - y).abs() / mag).max()))
    # S4b
    rows = torch.ones(B, dtype=torch.bool)
    if s.mode == "logits" and s.active is not None and use_active:
        rows = s.active != 0
        bad += int((out[~rows] != SENT).sum())                    # inactive rows keep their bits
    if "S4b" in stages:
        want, A = prod64(ho, s.Wn)
        if s.mode == "logits":
            want, A = want + s.bn.double(), A + s.bn.double().abs()
        res["S4b"] = _ratio(out[rows], want[rows], A[rows], s.mode != "logits")
        if pre:
            res["e32_S4b"] = _e32(pre["S4b"], want, A)
    # sentinels: extra rows, pad columns, the sync block
    for k in ("z1", "hid", "z2", "h_out", "out"):
        bad += int((b[k][B:] != SENT).sum())
    bad += int((b["h_out"][:B, D:] != SENT).sum()) + int((b["out"][:B, Nn:] != SENT).sum())
    want_sync = torch.full_like(b["sync"], SYNC_SENT)
    want_sync[counter_words(s)] = NGRP
    bad += int((b["sync"] != want_sync).sum()) + int(b["err"][0] != 0)
    res["guards"] = bad
    return res


EXACT = ("S4a", "LN1", "guards")


def worst(res):
    """The largest error / bound over the stage checks of a check() result; a failed exactness check counts as inf."""
    w = max(res[k] for k in PRODUCT_STAGES + ("tiecap",))
    return INF if any(res.get(k, 0) for k in EXACT) else w


def applicable(s, defect, stage):
    """Whether a defect can show in set s at all (it is then REQUIRED to show)."""
    multi = {"S1": s.D > 512, "S2": True, "S3": s.D > 512, "S4b": True}
    if defect in ("tile_swap", "bias_tile0"):
        return multi[stage] and not (defect == "bias_tile0" and stage == "S4b" and s.mode != "logits") \
            and not (s.w2zero and stage == "S3")
    if defect in ("ln_stats_D", "ln_stats_pad"):
        return s.d_ln < s.D
    if defect == "ln_one_pass":
        return s.big_row is not None and s.big_row in s.rows
    if defect == "group0":
        return max(s.rows) >= 16 and not (s.w2zero and stage == "S3")
    if defect == "inactive_written":
        return s.active is not None and not bool(s.active.all())
    if defect == "logits_tail":
        return s.mode == "logits"
    if defect == "eps_swap" and stage == "S4a":
        return s.w2zero                                            # (elsewhere var(z2) ~ 1 dwarfs both eps)
    if s.w2zero and (stage == "S3" or defect in ("no_relu", "relu_before_bias")):
        return False                                               # (hid does not reach z2 there; hid itself is checked)
    return True


def tail_sets():
    """(id, args of build_tail) of every layer-tail launch of the tests: every B of the narrow kernel {1, 16, 17, 37, 64} and
    of the wide one {5, 33}, both modes on every shape, zero-padded widths in both templates, the W2 = 0 sets."""
    out = []
    for shape, B, mode, d_ln in (("n512", 1, "qkv", 512), ("n512", 16, "qkv", 512), ("n512", 37, "qkv", 512),
                                 ("n512", 64, "qkv", 512), ("n512", 17, "logits", 512),
                                 ("n640", 17, "qkv", 500), ("n640", 64, "qkv", 500), ("n640", 1, "logits", 500),
                                 ("n640", 16, "logits", 500), ("n640", 37, "logits", 500),
                                 ("wide", 33, "qkv", 1024), ("wide", 5, "qkv", 1000), ("wide", 5, "logits", 1024),
                                 ("wide", 33, "logits", 1000)):
        out.append((f"{shape}-B{B}-{mode}-ln{d_ln}", (shape, B, mode, d_ln, False)))
    for shape, B, mode, d_ln in (("n512", 17, "qkv", 512), ("n640", 17, "qkv", 500), ("wide", 5, "qkv", 1024)):
        out.append((f"{shape}-B{B}-{mode}-ln{d_ln}-w2zero", (shape, B, mode, d_ln, True)))
    return out


def defect_rows(s):
    """The sub-batch on which the host test plants defects: the special rows, an inactive one, one row of every row group."""
    rows = {0, min(1, s.B - 1), min(2, s.B - 1), s.B - 1}
    rows |= {r for r in (16, 32, 48) if r < s.B}
    return sorted(rows)


# ------------------------------------------------------------------------------------------------ the head
class HeadSet:
    pass


def build_head(shape, B, d_true, probe=False):
    """commu_decode_head operands.  probe: E[v] = unit vector e_((7 v + 3) mod d_true), scale 1 and integer weights
    (37 (n K + k)) mod 251 (exact in bf16), so that qkv[row, n] == Wqkv[n, (7 tok[row] + 3) mod d_true] bit for bit."""
    D, DI, HD = SHAPES[shape]
    s = HeadSet()
    s.shape, s.D, s.DI, s.HD, s.B, s.d_true, s.probe, s.Nn = shape, D, DI, HD, B, d_true, probe, 3 * HD
    g, rn = _rng(9000 + D + HD + d_true + B)
    _randn = lambda g, *shape: rn(*shape)
    s.tok = torch.randint(0, V, (B,), generator=g)
    s.tok[0] = V - 1
    if B > 1:
        s.tok[B - 1] = 0
    if probe:
        s.E = torch.zeros(V, d_true)
        s.E[torch.arange(V), (7 * torch.arange(V) + 3) % d_true] = 1.0
        s.scale = 1.0
        idx = torch.arange(s.Nn)[:, None] * D + torch.arange(D)[None]
        s.W = bf(((37 * idx) % 251).float())
    else:
        s.E = _randn(g, V, d_true)
        s.scale = math.sqrt(d_true)
        s.W = bf(_randn(g, s.Nn, D) / math.sqrt(D))
        if B > 4:
            s.tok[2], s.tok[B - 2] = -1, V                         # ids outside the vocabulary: NaN rows
    s.n_zero = 3 * 12 * CNT_STRIDE + 37                           # (not a multiple of 256)
    return s


def head_buffers(s):
    return dict(h_out=torch.full((s.B + 2, s.D + PAD), SENT, dtype=BF16), out=torch.full((s.B + 2, s.Nn + PAD), SENT, dtype=BF16),
                zero=torch.full((s.n_zero + 64,), SYNC_SENT, dtype=torch.int32))


def head_run(s, b, defect=None):
    B, D = s.B, s.D
    bad = (s.tok < 0) | (s.tok >= V)
    x = s.E[s.tok.clamp(0, V - 1)] * torch.tensor(1.0 if defect == "no_scale" else s.scale, dtype=F32)
    if defect == "bad_id_row0":
        x[bad] = s.E[0] * torch.tensor(s.scale, dtype=F32)
    else:
        x[bad] = math.nan
    ho = torch.zeros(B, D, dtype=BF16)
    ho[:, :s.d_true] = bf(x)
    b["h_out"][:B, :D] = ho
    kw = {"drop_chunk": (1, 1, 2)} if defect == "drop_chunk" else {"drop_wave": 3} if defect == "drop_wave" else {}
    acc = prod32(ho, s.W, **kw)
    b["_pre"] = acc
    b["out"][:B, :s.Nn] = bf(_swap_tiles(acc) if defect == "tile_swap" else acc)
    b["zero"][:s.n_zero] = 0
    return b


def head_check(s, b):
    """{"h_out": violations, "qkv": worst error / bound (the probe: violations of bit equality), "guards": violations}."""
    B, D, Nn = s.B, s.D, s.Nn
    ho, out = b["h_out"][:B, :D], b["out"][:B, :Nn]
    ok_rows = (s.tok >= 0) & (s.tok < V)
    want_h = torch.zeros(B, D, dtype=BF16)
    want_h[:, :s.d_true] = bf(s.E[s.tok.clamp(0, V - 1)] * torch.tensor(s.scale, dtype=F32))
    res = {"h_out": int((ho[ok_rows] != want_h[ok_rows]).sum()) + int((~ho[~ok_rows, :s.d_true].isnan()).sum())
           + int((ho[~ok_rows, s.d_true:] != 0).sum())}
    bad = int((~out[~ok_rows].isnan()).sum())
    if s.probe:
        k = (7 * s.tok + 3) % s.d_true
        res["qkv"] = int((out != s.W[:, k].T).sum())
    else:
        want, A = prod64(ho[ok_rows], s.W)
        res["qkv"] = _ratio(out[ok_rows], want, A, True)
        if "_pre" in b:
            res["e32_head"] = _e32(b["_pre"][ok_rows], want, A)
    for k in ("h_out", "out"):
        bad += int((b[k][B:] != SENT).sum())
    bad += int((b["h_out"][:B, D:] != SENT).sum()) + int((b["out"][:B, Nn:] != SENT).sum())
    bad += int((b["zero"][:s.n_zero] != 0).sum()) + int((b["zero"][s.n_zero:] != SYNC_SENT).sum())
    res["guards"] = bad
    return res


def head_worst(res):
    return INF if res["h_out"] or res["guards"] else float(res["qkv"])


def head_sets():
    return [(f"head-{shape}-B{B}-d{d}", (shape, B, d)) for shape, B, d in (("n512", 37, 512), ("n640", 17, 500), ("wide", 33, 1024),
                                                                           ("n512", 1, 512), ("wide", 5, 1024))]


# ------------------------------------------------------------------------------------------------ exact layout probes
def phase1_probe(shape, B):
    """vec rows are unit vectors e_k(row), h = 0: z1[row, n] == Wo[n, k(row)] exactly.  (set, k)"""
    s = build_tail(shape, B, "qkv", SHAPES[shape][0])
    k = (torch.arange(B) * 37 + 5) % s.HD
    s.vec = torch.zeros(B, s.HD, dtype=BF16)
    s.vec[torch.arange(B), k] = 1.0
    s.h = torch.zeros(B, s.D, dtype=BF16)
    s.big_row = None
    return s, k


def pack_layout(W, N, K):
    """The packed copy of W [N, K] by the formula above load_w (decode_tail.hip): 16-byte chunk
    ((((ng NT + t) 4 + w) KS + ks) 64 + lane) holds W[16 (ng + 32 t) + lane % 16][w 32 KS + 32 ks + 8 (lane / 16) .. + 8],
    NT = ceil(ceil(N / 16) / 32), KS = K / 128; rows >= N are zero."""
    KS, NT = K // 128, ((N + 15) // 16 + NGRP - 1) // NGRP
    c = torch.arange(NGRP * NT * 4 * KS * 64)
    lane, q = c % 64, c // 64
    ks, q = q % KS, q // KS
    w, q = q % 4, q // 4
    t, ng = q % NT, q // NT
    r = 16 * (ng + NGRP * t) + lane % 16
    k = w * 32 * KS + 32 * ks + 8 * (lane // 16)
    Wz = torch.zeros(NGRP * NT * 16, K, dtype=W.dtype)
    Wz[:N] = W[:N, :K]
    return Wz[r[:, None], k[:, None] + torch.arange(8)[None]].reshape(-1)


PACK_CASES = ((729, 512), (1536, 512), (1920, 512), (3072, 1024), (1024, 2048), (512, 640))
