"""Host-side contract of the decode attention with a SHARED PROMPT PREFIX (csrc/decode_prefix.hip) and the input sets that
tests/test_prefix_contract_host.py and tests/test_prefix_gpu.py share.  Plain module, CPU tensors only; the contract, the
bound and the probe builders are decode_contract's, unchanged.

One step of an active pair (b, h): the keys are prefix rows 0 .. P-1 of head h (held once for all slots) followed by the
private rows 0 .. klen[b] of (b, h) (the last one is the new token); the key of absolute position p (prefix row p, or
private row p - P) has distance (P + klen[b]) - p.  want / A / bound: decode_contract.contract_f64 over the concatenation.

INPUT SETS: H = 4 (heads 0, 1: key probes; heads 2, 3: distance probes, the same q in every slot), B = 5 slots with one
inactive, private lengths klen = {0, 1, 7, 63, 64}, Lp = 96, P in {1, CH-1, CH, CH+1, 2 CH + 3}; one long set (P = CH + 1,
klen = {600, 513, 0, 1, 7}, nsplit 2: two effective suffix chunks).  Pcap = 2 CH + 8 in every set, so the launch is sized for
three chunks whatever P is.  Balanced-pair key probes (decode_contract) sit on the first and the last key of every prefix
chunk, prefix row P - 1, private row 0 and the new token; a prefix row is shared by the slots, so each probed prefix row
of a head is tuned to ONE slot's q and belongs to that pair.  The distance heads probe distances {0, 5, 66} and {1, 2, 8}:
which key sits there depends on klen[b].

DEFECTS (evaluate(..., defect=name)), each the image of one line of decode_prefix.hip going wrong."""
import functools
import math

import torch

import decode_contract as DC
from decode_contract import ALPHA, DIST_HEADS, H, KEY_HEADS, PAD, bound, contract_f64, ratio  # noqa: F401

CH = 128          # prefix rows per chunk (commu_decode_prefix_chunk)
G = 4             # slots per prefix workgroup (commu_decode_prefix_group)
PCAP = 2 * CH + 8
B = 5
KLENS = (0, 1, 7, 63, 64)
PREFIXES = (1, CH - 1, CH, CH + 1, 2 * CH + 3)
LP = 96
LONG_KLENS = (600, 513, 0, 1, 7)
LONG_LP = 640
DIST_PROBES = ((0, 5, 66), (1, 2, 8))          # heads 2 and 3

DEFECTS = ("prefix_dist_other_klen",      # the prefix distance taken with another slot's klen
           "prefix_dist_no_p",            # the prefix distance without + P (negative: the mirrored table row stands in)
           "private_dist_plus_p",         # the private distance with + P
           "chunk_first_drop",            # a chunk's first key dropped
           "chunk_first_dup",             # a chunk's first key counted twice
           "last_prefix_drop",            # prefix row P - 1 dropped
           "merge_no_rescale",            # records merged without rescaling by their max
           "inactive_arrival",            # an inactive slot's arrival counted: the merge fires one arrival early, without
                                          # the pair's last record (the suffix's)
           "stale_private_row")           # the new token's K/V from its stale cache row (private row 0 at klen 0), not
                                          # from the registers


class Pair:
    def __init__(self, b, h):
        self.b, self.h = b, h
        self.probes = []          # absolute positions of the probed keys (key heads)


class PrefixSet:
    """One launch's operands (CPU): pk / pv bf16 [H, Pcap, DH] (rows >= P: NaN), kc / vc bf16 [B, H, Lp, DH] AFTER the append
    (rows beyond the new token: NaN), qkv [B, 3 HD + PAD] and rd [Pcap + Lp + 4, HD + PAD] with NaN pads."""

    def records(self, b):
        """The key ranges (absolute positions) of the records of slot b's pairs: prefix chunks, then suffix chunks."""
        P, n = self.P, int(self.klen[b]) + 1
        out = [(c, min(P, c + CH)) for c in range(0, P, CH)]
        chunk = n if self.nsplit == 1 else DC.split_chunk(n, self.nsplit)
        out += [(P + c, P + min(n, c + chunk)) for c in range(0, n, chunk)]
        return out

    def operands(self, p):
        DH, c = self.DH, slice(p.h * self.DH, (p.h + 1) * self.DH)
        n = int(self.klen[p.b]) + 1
        K = torch.cat([self.pk[p.h, :self.P], self.kc[p.b, p.h, :n]])
        V = torch.cat([self.pv[p.h, :self.P], self.vc[p.b, p.h, :n]])
        return self.qkv[p.b, :H * DH][c], self.u[c], self.vb[c], K, V, self.rd[:, c]

    def evaluate_pair(self, p, dtype=torch.float64, defect=None):
        """(want, A) [DH] of pair p evaluated in dtype, with a defect planted (None: the contract)."""
        P, k = self.P, int(self.klen[p.b])
        q, u, vb, K, V, Rd = self.operands(p)
        pos = list(range(P + k + 1))
        dist = [P + k - x for x in pos]
        if defect == "prefix_dist_other_klen":
            k2 = next(int(self.klen[b2]) for b2 in list(range(p.b + 1, self.B)) + list(range(p.b))
                      if self.active[b2] and int(self.klen[b2]) != k)
            dist[:P] = [P + k2 - x for x in range(P)]
        elif defect == "prefix_dist_no_p":
            dist[:P] = [abs(k - x) for x in range(P)]
        elif defect == "private_dist_plus_p":
            dist[P:] = [min(P + k - r, self.dmax) for r in range(k + 1)]
        elif defect in ("chunk_first_drop", "chunk_first_dup"):
            edges = [x for x in p.probes if x < P and x % CH == 0] or [0]
            if defect == "chunk_first_drop":
                pos.remove(edges[0])
            else:
                pos.append(edges[0])
            dist = [P + k - x for x in pos]
        elif defect == "last_prefix_drop":
            pos.remove(P - 1)
            dist = [P + k - x for x in pos]
        elif defect == "inactive_arrival":
            pos, dist = pos[:P], dist[:P]
        elif defect == "stale_private_row":
            K, V = K.clone(), V.clone()
            K[P + k], V[P + k] = self.stale_k[p.b, p.h], self.stale_v[p.b, p.h]
        elif defect == "merge_no_rescale":
            return self._merge_no_rescale(p, dtype)
        elif defect is not None:
            raise ValueError(defect)
        return contract_f64(pos, dist, q, u, vb, self.scale, K, V, Rd, dtype)

    def _merge_no_rescale(self, p, dtype):
        """Every record's (o, max, sum) as the kernel forms them, merged as sum o / sum sum: exp(max_r - max) forgotten."""
        P, k = self.P, int(self.klen[p.b])
        q, u, vb, K, V, Rd = (t.to(dtype) for t in self.operands(p))
        dist = torch.tensor([P + k - x for x in range(P + k + 1)])
        s = (DC._tree_sum(K * (q + u), 1) + DC._tree_sum(Rd[dist] * (q + vb), 1)) * self.scale
        num, den, a = 0.0, 0.0, 0.0
        for lo, hi in self.records(p.b):
            e = torch.exp((s[lo:hi] - s[lo:hi].max()).double()).to(dtype)
            num = num + DC._tree_sum(e[:, None] * V[lo:hi], 0)
            a = a + DC._tree_sum(e[:, None] * V[lo:hi].abs(), 0)
            den = den + DC._tree_sum(e, 0)
        return num / den, a / den

    def evaluate(self, dtype=torch.float64, defect=None, pair=None):
        """(want, A) float64 [B, H, DH] over every pair (or one), evaluated in `dtype`."""
        want = torch.zeros(self.B, H, self.DH, dtype=torch.float64)
        A = torch.zeros(self.B, H, self.DH, dtype=torch.float64)
        for p in (self.pairs if pair is None else [pair]):
            w, a = self.evaluate_pair(p, dtype, defect)
            want[p.b, p.h], A[p.b, p.h] = w.double(), a.double()
        return want, A

    def caches_before(self, append):
        """The private caches a launch starts from: with append the new token's row of every active slot holds NaN."""
        kc, vc = self.kc.clone(), self.vc.clone()
        if append:
            for b in range(self.B):
                if self.active[b]:
                    kc[b, :, int(self.klen[b])] = math.nan
                    vc[b, :, int(self.klen[b])] = math.nan
        return kc, vc


@functools.lru_cache(maxsize=4)
def _base(DH, Lp, seed):
    g = torch.Generator().manual_seed(seed)
    HD = H * DH
    bf = torch.bfloat16
    r = DC._randn
    return dict(qkv=(r(g, B, 3 * HD) * 0.7).to(bf), pk=(r(g, H, PCAP, DH) * 0.7).to(bf), pv=r(g, H, PCAP, DH).to(bf),
                kc=(r(g, B, H, Lp, DH) * 0.7).to(bf), vc=r(g, B, H, Lp, DH).to(bf),
                rd=(r(g, PCAP + Lp + 4, HD) * 0.7).to(bf), u=r(g, HD) * 0.3, vb=r(g, HD) * 0.3)


def candidates(P, k):
    """Absolute positions a key probe must visit: the first and the last key of every prefix chunk, prefix row P - 1,
    private row 0, the new token."""
    c = []
    for lo in range(0, P, CH):
        c += [lo, min(P, lo + CH) - 1]
    c += [P - 1, P, P + k]
    return sorted(set(c))


def build(DH, P, klens=KLENS, Lp=LP, nsplit=1, inactive=2, variant=0):
    s = PrefixSet()
    s.DH, s.P, s.B, s.Lp, s.Pcap, s.nsplit, s.scale = DH, P, B, Lp, PCAP, nsplit, 0.125
    s.RPW = 64 // (DH // 8)
    HD = H * DH
    base = _base(DH, Lp, 7000 + DH + Lp)
    bf = torch.bfloat16
    s.qkv = torch.full((B, 3 * HD + PAD), math.nan, dtype=bf)
    s.qkv[:, :3 * HD] = base["qkv"]
    for h in DIST_HEADS:                                  # the distance-probe heads: the same q in every slot
        s.qkv[:, h * DH:(h + 1) * DH] = s.qkv[0, h * DH:(h + 1) * DH]
    s.pk, s.pv = base["pk"].clone(), base["pv"].clone()
    s.kc, s.vc = base["kc"].clone(), base["vc"].clone()
    s.rd = torch.full((PCAP + Lp + 4, HD + PAD), math.nan, dtype=bf)
    s.rd[:, :HD] = base["rd"]
    s.u, s.vb = base["u"].clone(), base["vb"].clone()
    s.klen = torch.tensor(klens, dtype=torch.int32)
    s.active = torch.ones(B, dtype=torch.uint8)
    s.active[inactive] = 0
    s.stale_k = torch.stack([s.kc[b, :, klens[b]] for b in range(B)])          # [B, H, DH]: what the rows held before
    s.stale_v = torch.stack([s.vc[b, :, klens[b]] for b in range(B)])
    for b in range(B):
        if s.active[b]:
            k = klens[b]
            s.kc[b, :, k] = s.qkv[b, HD:2 * HD].view(H, DH)                    # the append
            s.vc[b, :, k] = s.qkv[b, 2 * HD:3 * HD].view(H, DH)
            s.kc[b, :, k + 1:], s.vc[b, :, k + 1:] = math.nan, math.nan        # never read
    s.pk[:, P:], s.pv[:, P:] = math.nan, math.nan                              # never read
    s.dmax = P + max(klens[b] for b in range(B) if s.active[b])
    s.rd[s.dmax + 1:] = math.nan
    for h, ds in zip(DIST_HEADS, DIST_PROBES):
        c = slice(h * DH, (h + 1) * DH)
        for d in ds:
            if d <= s.dmax:
                s.rd[d, c] = DC._probe(s.qkv[0, :HD][c].float() + s.vb[c], ALPHA, s.scale, bf)
    s.pairs = []
    turn = variant
    for h in range(H):
        used = set()                                      # probed prefix rows of this head (each tuned to one slot)
        for b in range(B):
            if not s.active[b]:
                continue
            p = Pair(b, h)
            s.pairs.append(p)
            if h not in KEY_HEADS:
                continue
            k = klens[b]
            todo = [x for x in candidates(P, k) if x < P and x not in used]      # prefix rows nobody has probed yet
            if h == KEY_HEADS[1]:
                todo.reverse()
            first = todo.pop(0) if todo else (P, P + k)[turn % 2]
            second = ((todo.pop(0) if todo else P + k), P, P + k)[turn % 3]
            if second == first:
                second = next((x for x in (P + k, P, *todo) if x != first), None)
            turn += 1
            if second is None:
                continue
            p.probes = [first, second]
            c = slice(h * DH, (h + 1) * DH)
            vec = DC._probe(s.qkv[b, :HD][c].float() + s.u[c], ALPHA, s.scale, bf)
            for x in p.probes:
                if x < P:
                    s.pk[h, x] = vec
                    used.add(x)
                else:
                    s.kc[b, h, x - P] = vec
                    if x == P + k:
                        s.qkv[b, HD:2 * HD][c] = vec
    return s


def all_sets():
    """(id, builder arguments) of every input set."""
    out = []
    for DH in (64, 32):
        for i, P in enumerate(PREFIXES):
            out.append((f"dh{DH}-P{P}", dict(DH=DH, P=P, inactive=i % B, variant=i + (DH == 32))))
        out.append((f"dh{DH}-long", dict(DH=DH, P=CH + 1, klens=LONG_KLENS, Lp=LONG_LP, nsplit=2, inactive=4, variant=1)))
    return out
