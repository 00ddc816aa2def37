"""The training attention against its float64 contract, element by element (tests/attn_contract.py: the contract, the
bound |got - want| <= rho |want| + c A with exact zeros where nothing is visible, the input sets with balanced-pair probes;
tests/test_attn_contract_host.py proves on the CPU that the same sets catch every planted defect):

  forward:  commu_relattn_fwd (d_head 32: relattn_fwd; d_head 64: generations 0 = relattn3.hip and 2 = relattn_fwd2) and
            commu_relattn_fwd_save with a poisoned probability buffer; qu2 / qv2 to one bf16 ulp;
  backward: commu_relattn_bwd_q / _kv through ops.relattn_bwd with poisoned scratch: recompute, stored probabilities with the
            key-stationary generations 0, 2, 3, 4, the forward-saved probabilities, delta inside the query kernel, the fused
            band pass and the two band GEMMs, persistent zero-initialised scratch (launched twice) and fresh poisoned scratch.

Guards on every launch: qkv, rd and dout carry NaN pad columns, qkv and rd continue with NaN rows; out and dqkv are wider
than H DH and their pad columns hold a sentinel that must come back; everything the kernels must write is pre-filled with
the sentinel (drd with NaN); a second launch of every configuration gives the same bits."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_contract as AC  # noqa: E402

DEV = "cuda"
SENT = 768.0          # (exact in bf16)


def ops():
    from commu_amd import ops as o
    return o


class _Dev:
    """An input set on the GPU plus its float64 contract."""

    def __init__(self, name):
        s = self.s = AC.get(name)
        self.HD = s.H * s.DH
        HD, KB = self.HD, s.K * s.B
        self.qkv, self.rd_full = s.qkv.to(DEV), s.rd.to(DEV)
        self.q, self.k, self.v = self.qkv[s.M * s.B:KB, :HD], self.qkv[:KB, HD:2 * HD], self.qkv[:KB, 2 * HD:3 * HD]
        self.rd = self.rd_full[:s.K, :HD]
        self.u, self.vb, self.dout_full = s.u.to(DEV), s.vb.to(DEV), s.dout.to(DEV)
        self.dout = self.dout_full[:, :HD]
        self.reset = None if s.reset is None else s.reset.to(DEV)
        self.want = {n: s.want[n].to(DEV) for n in AC.TENSORS}
        self.A = {n: s.A[n].to(DEV) for n in AC.TENSORS}
        self.worst = {}

    def args(self):
        s = self.s
        return (self.q, self.k, self.v, self.rd, self.u, self.vb, self.reset, s.T, s.M, s.B, s.H, s.DH, s.same_length,
                s.mem_len)

    def check(self, what, n, got):
        """got in the contract's layout; records the worst ratio, raises with the element's name."""
        s = self.s
        w, msg = AC.worst(s, n, got, self.want[n], self.A[n])
        self.worst.setdefault(what, {})[n] = w
        if not w <= 1.0:
            probe = ""
            if n in ("out", "dq", "lse") and s.probes:          # the worst probed row of this tensor, by its probe
                r = AC.ratio(n, got, self.want[n], self.A[n]).nan_to_num(nan=math.inf)
                rows = [float(r[p["b"], p["h"], p["i"]].max()) for p in s.probes]
                k = max(range(len(rows)), key=rows.__getitem__)
                p = s.probes[k]
                probe = (f"; worst probed row: (b {p['b']}, h {p['h']}) row {p['i']} [{p['tag']}, {p['kind']} "
                         f"{p.get('j', p.get('d'))}] at {rows[k]:.3g} x the bound")
            raise AssertionError(f"{s.name} {what}: {msg}{probe}")

    def heads(self, t, rows):
        s = self.s
        return t.view(rows, s.B, s.H, s.DH).permute(1, 2, 0, 3)

    # ---- forward
    def forward(self, what, save_p=False):
        o, s = ops(), self.s
        buf = torch.full((s.T * s.B, self.HD + AC.PAD), SENT, device=DEV, dtype=torch.bfloat16)
        lse = torch.full((s.B, s.H, s.T), math.nan, device=DEV)
        out, lse, qs = o.relattn_fwd(*self.args(), out=buf[:, :self.HD], lse=lse, save_q=True, save_p=save_p)
        torch.cuda.synchronize()
        assert bool((buf[:, self.HD:] == SENT).all()), (s.name, what, "pad columns of out")
        self.check(what, "out", self.heads(out, s.T))
        self.check(what, "lse", lse)
        return buf, lse, qs

    def check_qs(self, qs):
        """qu2 / qv2 = bf16((q + u) scale log2 e) to one ulp."""
        s = self.s
        c2 = torch.tensor(s.scale, dtype=torch.float32) * torch.tensor(AC.LOG2E, dtype=torch.float32)
        for got, bias, n in ((qs[0], self.u, "qu2"), (qs[1], self.vb, "qv2")):
            want = ((self.q.float() + bias) * c2.to(DEV)).to(torch.bfloat16).float()
            err = (got.float() - want).abs()
            assert bool((err <= want.abs() * 2.0 ** -7).all()), (s.name, n, float(err.max()))

    # ---- backward
    def backward(self, what, out_buf, lse, qs, scratch=None):
        o, s = ops(), self.s
        HD, MB = self.HD, s.M * s.B
        dqkv = torch.full((s.K * s.B, 3 * HD + AC.PAD), SENT, device=DEV, dtype=torch.bfloat16)
        dqkv[:MB, :HD] = 0                                # the query columns of the memory rows: nobody writes them
        drd = torch.full((s.K, HD), math.nan, device=DEV)
        du, dvb = torch.zeros(HD, device=DEV), torch.zeros(HD, device=DEV)
        o.relattn_bwd(*self.args(), out_buf[:, :HD], self.dout, lse, qs, dqkv[MB:, :HD], dqkv[:, HD:2 * HD],
                      dqkv[:, 2 * HD:3 * HD], drd, du, dvb, scratch=scratch)
        torch.cuda.synchronize()
        assert bool((dqkv[:, 3 * HD:] == SENT).all()), (s.name, what, "pad columns of dqkv")
        assert bool((dqkv[:MB, :HD] == 0).all()), (s.name, what, "query columns of the memory rows")
        got = {"dq": self.heads(dqkv[MB:, :HD], s.T), "dk": self.heads(dqkv[:, HD:2 * HD], s.K),
               "dv": self.heads(dqkv[:, 2 * HD:3 * HD], s.K), "drd": drd.view(s.K, s.H, s.DH).permute(1, 0, 2),
               "du": du.view(s.H, s.DH), "dvb": dvb.view(s.H, s.DH)}
        for n, t in got.items():
            self.check(what, n, t)
        return dqkv, drd, du, dvb

    def report(self):
        for what, r in self.worst.items():
            print(f"{self.s.name} {what}: worst ratio " + ", ".join(f"{n} {v:.3f}" for n, v in r.items()))


@functools.lru_cache(maxsize=1)
def _dev(name):
    return _Dev(name)


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)) for x, y in zip(a, b))


def _forward(name):
    o, d = ops(), _dev(name)
    d.worst = {}
    gens = (0, 2) if d.s.DH == 64 else (0,)
    prev = o.attn_fwd_generation(0)
    try:
        for gen in gens:
            o.attn_fwd_generation(gen)
            buf, lse, qs = d.forward(f"fwd gen {gen}")
            d.check_qs(qs)
            buf2, lse2, qs2 = d.forward(f"fwd gen {gen}")
            assert _same_bits((buf, lse) + tuple(qs[:2]), (buf2, lse2) + tuple(qs2[:2])), (name, gen, "second launch differs")
    finally:
        o.attn_fwd_generation(prev)
    if d.s.DH == 64:
        keep = o.FWD_SAVES_P, o.POISON_SCRATCH
        o.FWD_SAVES_P, o.POISON_SCRATCH = True, True
        try:
            buf, lse, qs = d.forward("fwd save", save_p=True)
            buf2, lse2, qs2 = d.forward("fwd save", save_p=True)
        finally:
            o.FWD_SAVES_P, o.POISON_SCRATCH = keep
        assert qs[2] is not None
        assert _same_bits((buf, lse) + tuple(qs[:2]), (buf2, lse2) + tuple(qs2[:2])), (name, "fwd save", "second launch differs")
    d.report()


def _bwd_configs(s):
    """(name, STORE_ATTN_P, key-stationary generation, forward-saved P, DELTA_KERNEL, NO_FUSED_BAND)."""
    if s.DH != 64:
        return [("default", True, 0, False, True, False), ("delta in kernel", True, 0, False, False, False)]
    c = [("recompute", False, 0, False, True, False)]
    c += [(f"stored P kv gen {g}", True, g, False, True, False) for g in (0, 2, 3, 4)]
    c += [("forward P kv gen 2", True, 2, True, True, False), ("forward P kv gen 3", True, 3, True, True, False),
          ("delta in kernel", True, 0, False, False, False)]
    if s.band:
        c += [("band GEMMs", True, 0, False, True, True), ("band GEMMs recompute", False, 0, False, True, True)]
    return c


def _backward(name):
    from commu_amd._lib import call
    o, d = ops(), _dev(name)
    d.worst = {}
    s = d.s
    if s.DH == 64:          # the band sets, and only they, take the fused band pass (commu_relattn_bwd_band)
        assert (call("commu_attn_band_pairs", s.T, s.B, s.H) > 0) == s.band, name
    keep = (o.STORE_ATTN_P, o.DELTA_KERNEL, o.NO_FUSED_BAND, o.FWD_SAVES_P, o.POISON_SCRATCH)
    prev_kv = o.attn_bwd_kv_generation(0)
    try:
        fwd = {}
        for fwd_p in (False, True) if s.DH == 64 else (False,):
            o.FWD_SAVES_P, o.POISON_SCRATCH = fwd_p, True
            fwd[fwd_p] = d.forward("fwd for bwd" + (" (saves P)" if fwd_p else ""), save_p=True)
            assert (fwd[fwd_p][2][2] is not None) == fwd_p
        for what, store, gen, fwd_p, delta, nofuse in _bwd_configs(s):          # every configuration twice: the same bits
            o.STORE_ATTN_P, o.DELTA_KERNEL, o.NO_FUSED_BAND, o.POISON_SCRATCH = store, delta, nofuse, True
            o.attn_bwd_kv_generation(gen)
            res = d.backward(what, *fwd[fwd_p])
            assert _same_bits(res, d.backward(what, *fwd[fwd_p])), (name, what, "second launch differs")
        # the persistent zero-initialised scratch of the model (no wedge, nothing poisoned), launched twice on one dict
        for nofuse in (False, True) if s.band else (False,):
            o.STORE_ATTN_P, o.DELTA_KERNEL, o.NO_FUSED_BAND, o.POISON_SCRATCH = True, True, nofuse, False
            o.attn_bwd_kv_generation(0)
            scratch = {}
            what = "persistent scratch" + (" band GEMMs" if nofuse else "")
            a = d.backward(what, *fwd[False], scratch=scratch)
            assert _same_bits(a, d.backward(what, *fwd[False], scratch=scratch)), (name, what, "second launch differs")
    finally:
        o.STORE_ATTN_P, o.DELTA_KERNEL, o.NO_FUSED_BAND, o.FWD_SAVES_P, o.POISON_SCRATCH = keep
        o.attn_bwd_kv_generation(prev_kv)
    d.report()


# (the forward and the backward test of a set run next to each other: one upload and one float64 contract per set)
@pytest.mark.parametrize("name,which", [(n, w) for n in AC.NAMES for w in ("forward", "backward")])
def test_attention(name, which):
    (_forward if which == "forward" else _backward)(name)
