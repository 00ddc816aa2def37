"""The cached decode attention against the float64 contract, element by element (tests/decode_contract.py: the contract,
the bound |got - want| <= 2^-8 |want| + c A, the input sets with balanced-pair probes; tests/test_decode_contract_host.py
proves on the CPU that the same sets catch every planted defect):

  commu_decode_attn (linear cache), commu_decode_attn_split, commu_decode_attn_ring (bf16, csrc/decode.hip),
  commu_decode_kv_append_f32 + commu_relattn_f32 with klen (the fp32 linear-cache step, csrc/parity_f32.hip),
  commu_decode_kv_append and commu_decode_advance on their own.

Guards on every launch: append off and on (the new token's cache row holds NaN before the call and exactly the K/V columns
of qkv after it; every other cache element is bit-identical); cache rows and distance rows that must never be read hold
NaN; qkv, rd and out have pad columns (NaN in the inputs, a sentinel in out that must come back); inactive sequences keep
their rows of out and of the caches; split launches run 3 times and leave their counters at zero."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_contract as DC  # noqa: E402

DEV = "cuda"
SENT = 768.0          # (exact in bf16)
H = DC.H


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Dev:
    """A Launch on the GPU plus its float64 reference."""

    def __init__(self, l):
        self.l = l
        self.HD = H * l.DH
        self.qkv, self.rd, self.u, self.vb = l.qkv.to(DEV), l.rd.to(DEV), l.u.to(DEV), l.vb.to(DEV)
        self.klen, self.active = l.klen.to(DEV), l.active.to(DEV)
        self.kc1, self.vc1 = l.kc.to(DEV), l.vc.to(DEV)          # the caches after the step
        self.want, self.A = l.evaluate()
        self.rows = [b for b in range(l.B) if l.active[b]]
        self.worst = 0.0
        self.before = None

    def caches(self, append):
        if not append:
            return self.kc1.clone(), self.vc1.clone()
        if self.before is None:
            self.before = tuple(t.to(DEV) for t in self.l.caches_before(True))
        return self.before[0].clone(), self.before[1].clone()

    def out(self):
        return torch.full((self.l.B, self.HD + DC.PAD), SENT, device=DEV, dtype=self.l.dtype)

    def check(self, out, kc, vc, what, inactive_untouched=True):
        l = self.l
        torch.cuda.synchronize()
        assert _same_bits(kc, self.kc1) and _same_bits(vc, self.vc1), (what, "caches")
        o = out.cpu()
        assert bool((o[:, self.HD:] == SENT).all()), (what, "pad columns of out")
        if inactive_untouched:
            idle = [b for b in range(l.B) if not l.active[b]]
            assert bool((o[idle] == SENT).all()), (what, "inactive sequences")
        got = o[:, :self.HD].view(l.B, H, l.DH)[self.rows]
        r = DC.ratio(got, self.want[self.rows], self.A[self.rows], l.dtype == torch.bfloat16)
        worst = float(r.nan_to_num(nan=float("inf")).max())
        self.worst = max(self.worst, worst)
        if not bool((r <= 1).all()):
            i = int(r.nan_to_num(nan=float("inf")).argmax())
            b, h, e = i // (H * l.DH), i // l.DH % H, i % l.DH
            raise AssertionError(f"{what}: error {worst:.2f} x the bound at sequence {self.rows[b]} (klen "
                                 f"{int(l.klen[self.rows[b]])}) head {h} element {e}: got {float(got[b, h, e])}, want "
                                 f"{float(self.want[self.rows[b], h, e])}")


def _attn_linear(d, kc, vc, out, append, nsplit=1, ws=None, cnt=None):
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    l = d.l
    args = (_p(d.qkv), d.qkv.stride(0), _p(kc), _p(vc), _p(d.rd), d.rd.stride(0), _p(d.u), _p(d.vb), _p(d.klen),
            _p(d.active), _p(out), out.stride(0), l.B, H, l.DH, l.L, l.scale, 1 if append else 0)
    if nsplit == 1:
        call("commu_decode_attn", *args, _s())
    else:
        call("commu_decode_attn_split", *args, nsplit, _p(ws), _p(cnt), _s())


def _split_ws(l):
    ws = torch.full((l.B * H * 16 * (l.DH + 2),), float("nan"), device=DEV, dtype=torch.float32)
    return ws, torch.zeros(l.B * H, device=DEV, dtype=torch.int32)


@pytest.mark.parametrize("DH,Lmax,v", [(DH, Lmax, v) for DH in (64, 32) for Lmax in (4224, 136)
                                       for v in range(DC.LINEAR_VARIANTS)])
def test_linear_decode_attention_vs_float64_contract(DH, Lmax, v):
    """commu_decode_attn: lengths 1 .. Lmax on both sides of the rows per wave instruction, the 4-wave group, STEP and
    2 STEP of the ping-pong loop (klen = Lmax - 1 included); probes on key 0, the new token and both sides of every such
    boundary (two of them per variant v), through K and through the distance table."""
    d = _Dev(DC.build_linear(DH, Lmax, v))
    for append in (False, True):
        kc, vc = d.caches(append)
        out = d.out()
        _attn_linear(d, kc, vc, out, append)
        d.check(out, kc, vc, f"append {append}")
    print(f"commu_decode_attn d_head {DH} Lmax {Lmax} variant {v}: worst error {d.worst:.3f} of the per-element bound")


@pytest.mark.parametrize("nsplit", [2, 3, 8, 16])
@pytest.mark.parametrize("DH", [64, 32])
def test_split_decode_attention_vs_float64_contract(DH, nsplit):
    """commu_decode_attn_split: one sequence per (length, interior chunk edge) with probes on the last key of a chunk and
    the first key of the next; the new token (last chunk's workgroup; split 0 appends) probed through its distance."""
    d = _Dev(DC.build_split(DH, nsplit))
    ws, cnt = _split_ws(d.l)
    for append in (False, True):
        for rep in range(3):
            kc, vc = d.caches(append)
            out = d.out()
            _attn_linear(d, kc, vc, out, append, nsplit, ws, cnt)
            d.check(out, kc, vc, f"append {append} launch {rep}")
            assert int(cnt.abs().sum()) == 0, (append, rep)
    print(f"commu_decode_attn_split d_head {DH} nsplit {nsplit}: worst error {d.worst:.3f} of the per-element bound")


@pytest.mark.parametrize("DH,M,same_length,v", [(DH, M, sl, v) for DH in (64, 32) for M in (96, 2303) for sl in (True, False)
                                                for v in range(DC.RING_VARIANTS)])
def test_ring_decode_attention_vs_float64_contract(DH, M, same_length, v):
    """commu_decode_attn_ring, unsplit and over 4 workgroups: probes on the new token's row, physical rows 0 and W - 1,
    the oldest visible key, a chunk edge, a distance pair that straddles the seam; with same_length and a full memory the
    hidden key scores alpha + 20 and must contribute exactly nothing."""
    from commu_amd import ops
    d = _Dev(DC.build_ring(DH, M, same_length, v))
    l = d.l
    ws, cnt = _split_ws(l)
    for nsplit in (1, 4):
        for append in (False, True):
            for rep in range(3 if nsplit > 1 else 1):
                kc, vc = d.caches(append)
                out = d.out()
                ops.decode_attn_ring(d.qkv[:, :3 * d.HD], kc, vc, d.rd, d.u, d.vb, d.klen, d.active, out[:, :d.HD], l.L,
                                     l.scale, append=append, same_length=same_length, nsplit=nsplit, split_ws=ws,
                                     split_cnt=cnt)
                d.check(out, kc, vc, f"nsplit {nsplit} append {append} launch {rep}")
                assert int(cnt.abs().sum()) == 0, (nsplit, append, rep)
    print(f"commu_decode_attn_ring d_head {DH} M {M} same_length {same_length} variant {v}: worst error {d.worst:.3f} of the "
          "per-element bound")


@pytest.mark.parametrize("DH,v", [(DH, v) for DH in (64, 32, 50) for v in range(DC.F32_VARIANTS)])
def test_fp32_linear_cache_step_vs_float64_contract(DH, v):
    """ops.decode_kv_append_f32 then ops.relattn_f32(T = 1, klen): caches [B][Lmax][H DH]; d_head 50 runs the
    scalar-load instantiation.  Bound c32 A.  (The fp32 attention has no active flag: only the append skips the inactive
    sequence, whose output is not looked at.)"""
    from commu_amd import ops
    d = _Dev(DC.build_f32(DH, v))
    l = d.l
    for append in (False, True):
        kc, vc = d.caches(append)
        out = d.out()
        if append:
            ops.decode_kv_append_f32(d.qkv, kc, vc, d.klen, d.active, d.HD, l.L)
        ops.relattn_f32(d.qkv[:, :d.HD], kc, vc, d.HD, l.L * d.HD, d.rd, d.u, d.vb, 1, 0, l.B, H, DH, False, 0, l.scale,
                        klen=d.klen, out=out[:, :d.HD])
        d.check(out, kc, vc, f"append {append}", inactive_untouched=False)
    print(f"fp32 linear-cache step d_head {DH} variant {v}: worst error {d.worst:.3f} of the bound c32 A")


@pytest.mark.parametrize("DH", [64, 32])
def test_kv_append_on_its_own_leaves_the_fused_appends_cache(DH):
    """commu_decode_kv_append: the new token's K/V into row klen[b] (klen = Lmax - 1 included) of the active sequences,
    nothing else touched -- the cache that the attention kernel's fused append is held to."""
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    for Lmax in (136, 4224):
        d = _Dev(DC.build_linear(DH, Lmax, 0))
        l = d.l
        assert int(l.klen.max()) == Lmax - 1 and not bool(l.active.all())
        kc, vc = d.caches(True)
        call("commu_decode_kv_append", _p(d.qkv), d.qkv.stride(0), _p(kc), _p(vc), _p(d.klen), _p(d.active), l.B, Lmax, H,
             d.HD, _s())
        torch.cuda.synchronize()
        assert _same_bits(kc, d.kc1) and _same_bits(vc, d.vc1), Lmax


@pytest.mark.parametrize("B", [1, 64, 70, 200])
def test_klen_advance_saturates_below_the_cap(B):
    """commu_decode_advance: klen[b] += 1 where advance[b] != 0 and klen[b] < cap - 1; nothing past element B - 1."""
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    cap = 137
    g = torch.Generator().manual_seed(B)
    klen = torch.randint(0, cap, (B + 8,), generator=g, dtype=torch.int32)
    klen[:: 3] = cap - 1
    klen[1:: 7] = cap - 2
    adv = torch.randint(0, 2, (B + 8,), generator=g).to(torch.uint8) * 3          # (any non-zero byte is a flag)
    adv[B:] = 1
    want = klen.clone()
    step = (adv[:B] != 0) & (klen[:B] < cap - 1)
    want[:B] += step.to(torch.int32)
    assert int(step.sum()) > 0 or B == 1
    kd, ad = klen.to(DEV), adv.to(DEV)
    for _ in range(2):                                    # a second call advances again, up to the cap
        call("commu_decode_advance", _p(kd), _p(ad), B, cap, _s())
    step2 = (adv[:B] != 0) & (want[:B] < cap - 1)
    want[:B] += step2.to(torch.int32)
    assert torch.equal(kd.cpu(), want)
    assert int(want[:B].max()) <= cap - 1
