"""Host-side contract of the cached decode attention (csrc/decode.hip, the fp32 linear-cache step of csrc/parity_f32.hip)
and the input sets that the kernel tests and the host test share.  Plain module, CPU tensors only.

One decode step of a (sequence, head) pair: the new token's query q attends to the visible positions; the key of position
p lives in cache row rows[p] and has distance dist[p] to the new token:

    s_j = ((q + u) . k_j + (q + vb) . Rd[dist_j]) * scale,   p = softmax(s),   want = sum_j p_j v_j,
    A   = sum_j p_j |v_j|          (the magnitude that the accumulation error of P . V scales with)

THE BOUND, per output element:  |got - want| <= 2^-8 |want| + C_BF16 A   for bf16 outputs (one round-to-nearest to 8
significand bits: half an ulp is at most 2^-8 relative), and  |got - want| <= C_F32 A  for fp32 outputs.

C_BF16 = C_F32 = 16 e32 rounded up to a power of two, where e32 = max |contract in float32 - contract in float64| / A
over every input set of this module (a property of the reference and the inputs, never of a kernel): measured
e32 = 1.094e-6 (tests/test_decode_contract_host.py prints and re-checks it), 16 e32 = 1.75e-5, so C = 2^-15.  The factor 16 covers the
kernels' summation order (lane-strided over four waves, octet and cross-wave reductions) and __expf's exp2 argument
rounding (about |s - max| 2^-24 relative).  docs/EXPERIMENTS.md, 8j.

INPUTS in which single keys matter (balanced-pair probes): in a pair of a key-probe head the K rows of the key under test
j* and of an anchor key far from it are alpha w / (w . w) / scale with w = q + u, alpha = 12: both score alpha above the
rest and share the probability about equally, so dropping one, counting it twice or giving it the wrong distance moves
the output by O(1) of a value row.  (A single dominating key would not do: p ~ 1 whatever happens to it.)  The heads
with distance probes do the same through two rows of Rd (w = q + vb); Rd is shared by the sequences of a head, so those
heads have the same q in every sequence and klen[b] decides which key sits at the probed distance.

DEFECTS (contract(..., defect=name)): each the image of one line of decode.hip going wrong; the host test proves that
every one of them breaks the bound on the input sets built here."""
import functools
import math

import torch

C_BF16 = 2.0 ** -15
C_F32 = 2.0 ** -15
ALPHA = 12.0
HIDDEN_EXTRA = 20.0          # the ring's hidden key scores alpha + 20: if it counted at all it would take the output
H = 4                        # heads of every set: 0, 1 key probes; 2, 3 distance probes
KEY_HEADS, DIST_HEADS = (0, 1), (2, 3)
PAD = 8                      # pad columns of qkv / rd / out

DEFECTS = ("drop_new", "stale_new", "drop_first", "tail_clamp", "dist_group", "v_shift", "chunk_first_drop",
           "chunk_first_dup", "hidden_plus", "hidden_minus", "ring_no_wrap")


# ------------------------------------------------------------------------------------------------ the contract
def visible(pos, M, same_length):
    """Positions that the token at absolute position pos sees with a memory of M (model.py:507-568 at qlen 1)."""
    lo = max(0, pos - M)
    if same_length and pos >= M:
        lo += 1
    return list(range(lo, pos + 1))


def _tree_sum(x, dim):
    """Sum over `dim` as a pairwise tree in a fixed order."""
    x = x.movedim(dim, 0)
    n = x.shape[0]
    while n > 1:
        h = (n + 1) // 2
        x = torch.cat([x[:n - h] + x[h:n], x[n - h:h]])
        n = h
    return x[0]


def contract_f64(rows, dist, q, u, vb, scale, K, V, Rd, dtype=torch.float64, defect=None, ctx=None):
    """(want[DH], A[DH]) of one (sequence, head) pair.  rows / dist: cache row and distance of every visible position, in
    chronological order (the new token last); q, u, vb [DH]; K, V [cache rows, DH]; Rd [distances, DH] of the head.
    dtype float64: the reference; float32: the honest evaluation in another summation order.  defect: see DEFECTS; ctx
    carries what a defect needs (RPW, new_row, stale_k, stale_v, jstar, hidden, cur, dmax, edge)."""
    rows = torch.as_tensor(rows, dtype=torch.long).clone()
    dist = torch.as_tensor(dist, dtype=torch.long).clone()
    ctx = ctx or {}
    mult = torch.ones(len(rows), dtype=dtype)          # how often a key is counted
    vrows = None
    stale = None

    def at(row):
        i = (rows == row).nonzero()
        assert i.numel() == 1, (defect, row)
        return int(i)

    if defect is None:
        pass
    elif defect == "drop_new":                          # the new token's key is missing (nall = apos instead of apos + 1)
        mult[at(ctx["new_row"])] = 0
    elif defect == "stale_new":                         # the `self` substitution is missing: K/V from the stale cache row
        stale = at(ctx["new_row"])
    elif defect == "drop_first":                        # cache row 0 is missing
        mult[at(0)] = 0
    elif defect == "tail_clamp":                        # min(j, n - 1) without `j < n`: the last row once more per clamped lane
        t = (-int(rows.max() + 1)) % ctx["RPW"] or ctx["RPW"]
        mult[int(rows.argmax())] += t
    elif defect == "dist_group":                        # one wave instruction (RPW rows) reads the wrong row of the table
        g0 = ctx["jstar"] // ctx["RPW"] * ctx["RPW"]
        sel = (rows >= g0) & (rows < g0 + ctx["RPW"])
        dist[sel] = torch.where(dist[sel] < ctx["dmax"], dist[sel] + 1, dist[sel] - 1)          # (stays inside the table)
    elif defect == "v_shift":                           # V of key j with the probability of key j +- RPW
        i = torch.arange(len(rows))
        up, dn = i + ctx["RPW"], i - ctx["RPW"]
        vrows = rows[torch.where(up < len(rows), up, torch.where(dn >= 0, dn, i))]
    elif defect == "chunk_first_drop":                  # a split chunk starts one key late
        mult[at(ctx["edge"])] = 0
    elif defect == "chunk_first_dup":                   # ... or the previous chunk ends one key late
        mult[at(ctx["edge"])] = 2
    elif defect in ("hidden_plus", "hidden_minus"):     # the ring's hidden row off by one: the hidden key counts, and the
        hrow, hdist = ctx["hidden"]                     # oldest visible key (plus) or the new token (minus) does not
        mult[0 if defect == "hidden_plus" else at(ctx["new_row"])] = 0
        rows, dist = torch.cat([torch.tensor([hrow]), rows]), torch.cat([torch.tensor([hdist]), dist])
        mult = torch.cat([torch.ones(1, dtype=dtype), mult])
    elif defect == "ring_no_wrap":                      # rows after the new token's: pos - j without + W (negative: the
        late = rows > ctx["cur"]                        # read leaves the table; the mirrored row j - pos stands in)
        dist[late] = rows[late] - ctx["cur"]
    else:
        raise ValueError(defect)
    k, v = K[rows].to(dtype), V[rows if vrows is None else vrows].to(dtype)
    if stale is not None:
        k[stale], v[stale] = ctx["stale_k"].to(dtype), ctx["stale_v"].to(dtype)
    q, u, vb = q.to(dtype), u.to(dtype), vb.to(dtype)
    # every sum is a pairwise tree of elementwise IEEE operations and exp is evaluated in float64 and rounded: the float32
    # evaluation (and with it e32) is the same number on every machine, whatever BLAS or vector width torch runs on
    s = (_tree_sum(k * (q + u), 1) + _tree_sum(Rd[dist].to(dtype) * (q + vb), 1)) * scale
    s = s.masked_fill(mult == 0, -math.inf)
    e = mult * torch.exp((s - s.max()).double()).to(dtype)
    p = (e / _tree_sum(e, 0))[:, None]
    return _tree_sum(p * v, 0), _tree_sum(p * v.abs(), 0)


def contract_batch(q, kc, vc, rd, u, vb, rows_dist, scale, head_major=True):
    """contract_f64 over a batch: q [B, H, DH]; kc / vc [B, H, L, DH] (head_major) or [B, L, H, DH]; rd [distances, H, DH];
    u, vb [H, DH]; rows_dist[b] = (rows, dist) of sequence b, or None (skipped: zeros).  (want, A) float64 [B, H, DH]."""
    B, Hn, DH = q.shape
    want, A = torch.zeros(B, Hn, DH, dtype=torch.float64), torch.zeros(B, Hn, DH, dtype=torch.float64)
    q, kc, vc, rd, u, vb = (t.cpu() for t in (q, kc, vc, rd, u, vb))
    for b, rdist in enumerate(rows_dist):
        if rdist is None:
            continue
        for h in range(Hn):
            K, V = (kc[b, h], vc[b, h]) if head_major else (kc[b, :, h], vc[b, :, h])
            want[b, h], A[b, h] = contract_f64(rdist[0], rdist[1], q[b, h], u[h], vb[h], scale, K, V, rd[:, h])
    return want, A


def ring_rows_dist(pos_list, M, same_length):
    """(rows, dist) of every sequence of a ring of W = M + 1 rows whose new tokens sit at the absolute positions pos_list."""
    out = []
    for pos in pos_list:
        ps = visible(pos, M, same_length)
        out.append(([p % (M + 1) for p in ps], [pos - p for p in ps]))
    return out


def bound(want, A, bf16=True):
    return 2.0 ** -8 * want.abs() + C_BF16 * A if bf16 else C_F32 * A


def ratio(got, want, A, bf16=True):
    """|got - want| / bound per element (float64); NaN where got is NaN, so compare with `not (r <= 1).all()`."""
    return (got.double() - want).abs() / bound(want, A, bf16).clamp_min(1e-300)


# ------------------------------------------------------------------------------------------------ input sets
class Pair:
    def __init__(self, b, h, rows, dist, ctx):
        self.b, self.h, self.rows, self.dist, self.ctx = b, h, rows, dist, ctx
        self.probes = []          # cache rows of the two probed keys
        self.designed = []        # defects that this pair must catch


class Launch:
    """One kernel launch's operands (CPU).  kind: linear | split | ring | f32.  kc / vc: the caches AFTER the append, in
    the kernel's layout (bf16 [B, H, L, DH]; fp32 [B, L, H DH]); qkv [B, 3 HD + PAD] and rd [rows, HD + PAD] carry NaN
    pad columns; rows that must never be read hold NaN."""

    def kv(self, t, b, h):
        return t[b, h] if self.dtype == torch.bfloat16 else t[b, :, h * self.DH:(h + 1) * self.DH]

    def caches_before(self, append):
        """The caches a launch starts from: with append the new token's row of every active sequence holds NaN."""
        kc, vc = self.kc.clone(), self.vc.clone()
        if append:
            for b in range(self.B):
                if self.active[b]:
                    for h in range(H):
                        self.kv(kc, b, h)[self.new_row[b]] = math.nan
                        self.kv(vc, b, h)[self.new_row[b]] = math.nan
        return kc, vc

    def evaluate(self, dtype=torch.float64, defect=None, pair=None):
        """(want, A) [B, H, DH] in float64 storage over every pair (or one), evaluated in `dtype`."""
        HD = H * self.DH
        want, A = torch.zeros(self.B, H, self.DH, dtype=torch.float64), torch.zeros(self.B, H, self.DH, dtype=torch.float64)
        for p in (self.pairs if pair is None else [pair]):
            c = slice(p.h * self.DH, (p.h + 1) * self.DH)
            w, a = contract_f64(p.rows, p.dist, self.qkv[p.b, :HD][c], self.u[c], self.vb[c], self.scale,
                                self.kv(self.kc, p.b, p.h), self.kv(self.vc, p.b, p.h), self.rd[:, c], dtype, defect, p.ctx)
            want[p.b, p.h], A[p.b, p.h] = w.double(), a.double()
        return want, A


def _randn(g, *shape):
    """Standard-normal-like draws that are the same bits on every machine (torch.randn's are not: its CPU kernels differ
    in the last place with the vector width, and e32 is a maximum over all of them): integer draws only.  A pool of 2^20
    values, each the centred sum of six uniform bytes (Irwin-Hall, |x| <= 4.2), sampled with replacement."""
    r = torch.randint(0, 2 ** 48, (2 ** 20,), generator=g)
    pool = sum((r >> (8 * i)) & 255 for i in range(6))
    pool = ((pool - 765).double() / math.sqrt(6 * (256 ** 2 - 1) / 12)).float()
    return pool[torch.randint(0, 2 ** 20, shape, generator=g)]


@functools.lru_cache(maxsize=2)
def _base(dtype, DH, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    HD = H * DH
    shape = (B, H, L, DH) if dtype == torch.bfloat16 else (B, L, HD)
    return dict(qkv=(_randn(g, B, 3 * HD) * 0.7).to(dtype),
                kc=(_randn(g, *shape) * 0.7).to(dtype), vc=_randn(g, *shape).to(dtype),
                rd=(_randn(g, L + 4, HD) * 0.7).to(dtype),
                u=_randn(g, HD) * 0.3, vb=_randn(g, HD) * 0.3)


def _start(kind, dtype, DH, B, L, scale, klen, inactive, new_row, seed):
    l = Launch()
    l.kind, l.dtype, l.DH, l.B, l.L, l.scale = kind, dtype, DH, B, L, scale
    l.RPW = 64 // (DH // 8) if dtype == torch.bfloat16 else 64
    base = _base(dtype, DH, 24 if dtype == torch.bfloat16 else B, L, seed)
    HD = H * DH
    l.qkv = torch.full((B, 3 * HD + PAD), math.nan, dtype=dtype)
    l.qkv[:, :3 * HD] = base["qkv"][:B]
    for h in DIST_HEADS:                                 # the distance-probe heads: the same q in every sequence
        l.qkv[:, h * DH:(h + 1) * DH] = l.qkv[0, h * DH:(h + 1) * DH]
    l.kc, l.vc = base["kc"][:B].clone(), base["vc"][:B].clone()
    l.rd = torch.full((L + 4, HD + PAD), math.nan, dtype=dtype)
    l.rd[:, :HD] = base["rd"]
    l.u, l.vb = base["u"].clone(), base["vb"].clone()
    l.klen = torch.tensor(klen, dtype=torch.int32)
    l.active = torch.ones(B, dtype=torch.uint8)
    l.active[list(inactive)] = 0
    l.new_row = list(new_row)
    l.nsplit, l.same_length, l.pairs = 1, False, []
    l.stale_k = torch.stack([torch.stack([l.kv(l.kc, b, h)[new_row[b]] for h in range(H)]) for b in range(B)])
    l.stale_v = torch.stack([torch.stack([l.kv(l.vc, b, h)[new_row[b]] for h in range(H)]) for b in range(B)])
    for b in range(B):                                   # the append (the step's own, or an earlier one for append = 0)
        if l.active[b]:
            for h in range(H):
                l.kv(l.kc, b, h)[new_row[b]] = l.qkv[b, HD + h * DH:HD + (h + 1) * DH]
                l.kv(l.vc, b, h)[new_row[b]] = l.qkv[b, 2 * HD + h * DH:2 * HD + (h + 1) * DH]
    return l


def _probe(w, alpha, scale, dtype):
    w = w.double()
    return (alpha * w / _tree_sum(w * w, 0) / scale).to(dtype)


def _key_probe(l, p, row, alpha=ALPHA):
    HD, DH = H * l.DH, l.DH
    c = slice(p.h * DH, (p.h + 1) * DH)
    vec = _probe(l.qkv[p.b, :HD][c].float() + l.u[c], alpha, l.scale, l.dtype)
    l.kv(l.kc, p.b, p.h)[row] = vec
    if row == l.new_row[p.b]:
        l.qkv[p.b, HD:2 * HD][c] = vec


def _dist_probe(l, h, d, alpha=ALPHA):
    DH = l.DH
    c = slice(h * DH, (h + 1) * DH)
    l.rd[d, c] = _probe(l.qkv[0, :H * DH][c].float() + l.vb[c], alpha, l.scale, l.dtype)


def _anchor(rows_sorted, j, RPW):
    """A visible row far from row j: half the memory further on (cyclically), never j itself, and outside j's group of
    RPW rows (one wave instruction) where the memory has another group."""
    n = len(rows_sorted)
    i = rows_sorted.index(j)
    a = (i + n // 2 + 1) % n
    for _ in range(n):
        if a != i and (rows_sorted[a] // RPW != j // RPW or rows_sorted[0] // RPW == rows_sorted[-1] // RPW):
            break
        a = (a + 1) % n
    return rows_sorted[a]


def _finish(l, chunk_of=None):
    """NaN into everything that must never be read; which defects every pair is designed to catch."""
    dmax = 0
    for p in l.pairs:
        dmax = max(dmax, int(max(p.dist)))
        if p.ctx.get("hidden"):
            dmax = max(dmax, p.ctx["hidden"][1])
    if l.kind == "f32":                                  # (no active flag in the fp32 attention: every sequence reads)
        dmax = max(dmax, int(l.klen.max()))
    l.dmax = dmax
    l.rd[dmax + 1:] = math.nan
    for p in l.pairs:
        c = p.ctx
        c.update(RPW=l.RPW, new_row=l.new_row[p.b], stale_k=l.stale_k[p.b, p.h], stale_v=l.stale_v[p.b, p.h], dmax=dmax)
        n, P = len(p.rows), set(p.probes)
        d = p.designed
        if n == 1:
            d.append("stale_new")
        if n < 2 or len(P) < 2:
            continue
        c["jstar"] = p.probes[0]
        if c["new_row"] in P:
            d += ["drop_new", "stale_new"]
        if 0 in P:
            d.append("drop_first")
        if max(p.rows) in P and l.dtype == torch.bfloat16:
            d.append("tail_clamp")
        if len({r // l.RPW for r in P}) == 2:             # (in one group both probes would move together)
            d.append("dist_group")
        if n >= 2 * l.RPW and l.dtype == torch.bfloat16:          # (then every key has a partner RPW further on or back)
            d.append("v_shift")
        if chunk_of is not None:
            chunk = chunk_of(p.b)
            edges = [r for r in p.probes if r and r % chunk == 0 and r < n]
            if edges:
                c["edge"] = edges[0]
                d += ["chunk_first_drop", "chunk_first_dup"]
        if c.get("hidden"):
            d += ["hidden_plus", "hidden_minus"]
        if l.kind == "ring" and any(r > c["cur"] for r in P):
            d.append("ring_no_wrap")
    return l


def split_chunk(n, nsplit):
    """Keys per workgroup of a split launch, by the rule documented in decode.hip."""
    return max(512, (-(-n // nsplit) + 63) // 64 * 64)


# ---- linear cache, bf16 (commu_decode_attn; commu_decode_attn_split)
LINEAR_LENGTHS = (1, 2, 7, 8, 9, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)
LINEAR_VARIANTS = 5


def _linear_candidates(n, DH):
    """j* of the unsplit kernel: key 0, the new token, the last key before and the first after every boundary below n
    (rows per wave instruction, the 4-wave group, STEP and 2 STEP of the ping-pong loop)."""
    RPW = 64 // (DH // 8)
    c = [0, n - 1]
    for x in (RPW, 4 * RPW, 16 * RPW, 32 * RPW):
        c += [j for j in (x - 1, x) if j < n]
    return sorted(set(c))


def _linear_pairs(l, lengths, jstars, dstars):
    """Pairs of a linear-cache set: sequence b has lengths[b] keys; jstars[b] = (j* of head 0, j* of head 1); dstars =
    ((d*, d_anchor) of head 2, of head 3)."""
    for h, (d1, d2) in zip(DIST_HEADS, dstars):
        _dist_probe(l, h, d1)
        _dist_probe(l, h, d2)
    for b, n in enumerate(lengths):
        for t in (l.kc, l.vc):                            # rows >= n are never read
            for h in range(H):
                l.kv(t, b, h)[n:] = math.nan
        if not l.active[b]:
            continue
        rows = list(range(n))
        for h in range(H):
            p = Pair(b, h, rows, [n - 1 - j for j in rows], {})
            if h in KEY_HEADS and n >= 2:
                j = min(jstars[b][h], n - 1)
                p.probes = [j, _anchor(rows, j, l.RPW)]
                for r in p.probes:
                    _key_probe(l, p, r)
            elif h in DIST_HEADS:
                p.probes = [n - 1 - d for d in dstars[h - 2] if d < n]
            l.pairs.append(p)


def build_linear(DH, Lmax, variant):
    lengths = [n for n in LINEAR_LENGTHS if n < Lmax] + [Lmax]
    lengths.insert(3, 40)                                # (an inactive sequence among them)
    B = len(lengths)
    klen = [n - 1 for n in lengths]
    l = _start("linear", torch.bfloat16, DH, B, Lmax, 0.125, klen, [3], klen, 1002 + DH + Lmax)
    jstars = []
    for n in lengths:
        c = _linear_candidates(n, DH)
        jstars.append((c[(2 * variant) % len(c)], c[(2 * variant + 1) % len(c)]))
    # head 2: the new token's distance against one half a short memory away; head 3: distances that move with the variant
    far = (Lmax - 1, 100, 513, 300, 1024)[variant]
    dstars = ((0, 5 + variant), (min(far, Lmax - 1), (1, 7, 8, 31, 127)[variant]))
    _linear_pairs(l, lengths, jstars, dstars)
    return _finish(l)


SPLIT_LENGTHS = (512, 513, 1024, 1025, 1500, 4100, 4224)
SPLIT_LMAX = 4224


def build_split(DH, nsplit):
    """One sequence per (length, interior chunk edge): head 0 probes the last key of the chunk before the edge, head 1 the
    first key after it; the unsplit length probes the new token and key 0 by its key; head 2 probes the new token of
    EVERY sequence by its distance (it lives in the last chunk's workgroup while split 0 does the append)."""
    lengths, jstars = [], []
    for n in SPLIT_LENGTHS:
        chunk = split_chunk(n, nsplit)
        edges = list(range(chunk, n, chunk))
        for e in edges or [n - 1]:
            lengths.append(n)
            jstars.append((e - 1, e) if edges else (n - 1, 0))
    lengths.append(777)                                  # (the inactive sequence)
    jstars.append((776, 0))
    B = len(lengths)
    assert B <= 24
    klen = [n - 1 for n in lengths]
    l = _start("split", torch.bfloat16, DH, B, SPLIT_LMAX, 0.125, klen, [B - 1], klen, 2000 + DH)
    l.nsplit = nsplit
    _linear_pairs(l, lengths, jstars, ((0, 300), (511, 512)))
    return _finish(l, chunk_of=lambda b: split_chunk(lengths[b], nsplit))


# ---- ring cache, bf16 (commu_decode_attn_ring)
def ring_positions(M):
    """Ragged absolute positions: not yet full, exactly full (M - 1, M, M + 1), wrapped once, wrapped several times plus
    an offset, and the two alignments where the hidden row is the last / the first physical row."""
    W = M + 1
    return [5, M - 1, M, M + 1, W + 17, 3 * W + 41, 7 * W + (W - 1), 5 * W, 2 * W - 2, 40]


RING_VARIANTS = 3


def build_ring(DH, M, same_length, variant):
    """variant 0: the new token's row and physical row 0; 1: physical row W - 1 and the oldest visible key; 2: the two
    keys at the first chunk edge of a split over 4 workgroups (rings of >= 2048 rows) or rows 7 / 8.  Heads 2 / 3: the
    oldest distance that must count (M - 1, or M without same_length) against distance 0, and a pair of consecutive
    distances that straddles the seam (rows W - 1 | 0) in the sequence whose new token sits in that row."""
    W = M + 1
    pos_list = ring_positions(M)
    B = len(pos_list)
    l = _start("ring", torch.bfloat16, DH, B, W, 0.125, pos_list, [B - 1], [p % W for p in pos_list], 3000 + DH + M)
    l.same_length, l.M = same_length, M
    oldest = M - 1 if same_length else M
    seam = (17, 41, 16)[variant]                         # cur of position W + 17 / 3 W + 41; 16 | 17 away from the seam
    dstars = ((oldest, 0), (seam, seam + 1))
    for h, (d1, d2) in zip(DIST_HEADS, dstars):
        _dist_probe(l, h, d1)
        _dist_probe(l, h, d2)
        if same_length:                                  # the hidden key's distance
            _dist_probe(l, h, M, ALPHA + HIDDEN_EXTRA)
    edge = split_chunk(W, 4) if W >= 2048 else 8
    for b, pos in enumerate(pos_list):
        nvalid = min(pos + 1, W)
        for t in (l.kc, l.vc):                            # unwritten ring rows are never read
            for h in range(H):
                l.kv(t, b, h)[nvalid:] = math.nan
        if not l.active[b]:
            continue
        ps = visible(pos, M, same_length)
        rows, dist = [p % W for p in ps], [pos - p for p in ps]
        hidden = ((pos - M) % W, M) if same_length and pos >= M else None
        srt = sorted(rows)
        for h in range(H):
            p = Pair(b, h, rows, dist, dict(cur=pos % W, hidden=hidden))
            if h in KEY_HEADS:
                want_row = ((pos % W, 0), (W - 1, rows[0]), (edge - 1, edge))[variant][h]
                j = want_row if want_row in rows else srt[-1]
                p.probes = [j, _anchor(srt, j, l.RPW)]
                for r in p.probes:
                    _key_probe(l, p, r)
                if hidden:
                    _key_probe(l, p, hidden[0], ALPHA + HIDDEN_EXTRA)
            else:
                p.probes = [rows[dist.index(d)] for d in dstars[h - 2] if d in dist]
            l.pairs.append(p)
    return _finish(l, chunk_of=(lambda b: split_chunk(min(pos_list[b] + 1, W), 4)) if W >= 2048 else None)


# ---- linear cache, fp32 (commu_decode_kv_append_f32 + commu_relattn_f32 with klen)
F32_LENGTHS = (1, 2, 63, 64, 65, 128, 129, 1025)
F32_VARIANTS = 3
F32_LMAX = 1032


def build_f32(DH, variant):
    """The attention row visits the keys in chunks of 64 (attn_row_f32.h): j* = key 0, the new token and the keys on both
    sides of the first two chunk boundaries."""
    lengths = list(F32_LENGTHS)
    lengths.insert(3, 40)
    B = len(lengths)
    klen = [n - 1 for n in lengths]
    l = _start("f32", torch.float32, DH, B, F32_LMAX, 1.0 / DH ** 0.5, klen, [3], klen, 4000 + DH)
    cand = ((0, 10 ** 6), (63, 64), (127, 128))[variant]
    dstars = ((0, 5 + variant), ((1024, 64, 128)[variant], (1, 63, 127)[variant]))
    _linear_pairs(l, lengths, [cand] * B, dstars)
    return _finish(l)


def all_sets():
    """(id, builder, args) of every input set of the decode-contract tests."""
    out = []
    for DH in (64, 32):
        for Lmax in (4224, 136):
            out += [(f"linear-dh{DH}-L{Lmax}-v{v}", build_linear, (DH, Lmax, v)) for v in range(LINEAR_VARIANTS)]
        out += [(f"split-dh{DH}-x{ns}", build_split, (DH, ns)) for ns in (2, 3, 8, 16)]
        for M in (96, 2303):
            for sl in (True, False):
                out += [(f"ring-dh{DH}-M{M}-{'same' if sl else 'nosame'}-v{v}", build_ring, (DH, M, sl, v))
                        for v in range(RING_VARIANTS)]
    for DH in (64, 32, 50):
        out += [(f"f32-dh{DH}-v{v}", build_f32, (DH, v)) for v in range(F32_VARIANTS)]
    return out
