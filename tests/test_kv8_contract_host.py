"""The contract tests of the fp8 K/V cache have teeth (CPU only): the analogue of tests/test_decode_contract_host.py on every
linear / split / ring input set of decode_contract.all_sets() in fp8 form (tests/kv8_contract.py: caches quantised to e4m3
bytes + E8M0 block scales, the contract evaluated on their dequantised values, the fp8 kernel's rows per wave instruction),

  * the honest evaluation -- the contract in float32, another summation order, rounded to bf16 -- passes the bound;
  * every planted defect that a pair is designed to catch violates the bound in at least one element by >= 2x;
  * every defect expected of a kind of set is planted somewhere;
  * 16 e32 <= C_BF16 <= 2^-13 with e32 recomputed on these sets;
  * the dequantised values are exactly representable in bf16;

and the quantiser emulation itself equals torch.float8_e4m3fn rounding."""
import functools

import pytest
import torch

import decode_contract as DC
import kv8_contract as K8
from test_decode_contract_host import EXPECTED

SETS = [s for s in DC.all_sets() if not s[0].startswith("f32")]
IDS = [s[0] for s in SETS]


@functools.lru_cache(maxsize=None)
def _check(idx):
    """(kind, e32, worst honest ratio, {defect: (pairs, smallest worst-element ratio)}, pairs that miss, exact in bf16)."""
    _, fn, args = SETS[idx]
    l = K8.to_fp8(fn(*args))
    exact = True
    for q, s, t in ((l.kc8, l.ks, l.kc), (l.vc8, l.vs, l.vc)):
        d = K8.dequant(q, s)
        live = ~torch.isnan(d)
        exact = exact and bool((d[live].to(torch.bfloat16).float() == d[live]).all()) and bool((t.float()[live] == d[live]).all())
        assert bool(live.any())
    want, A = l.evaluate()
    f32, _ = l.evaluate(torch.float32)
    e32 = float(((f32 - want).abs() / A.clamp_min(1e-300)).max())
    got = f32.float().to(l.dtype).double()
    honest = float(DC.ratio(got, want, A, True).max())
    caught, missed = {}, []
    for p in l.pairs:
        for d in p.designed:
            bad, _ = l.evaluate(torch.float32, d, p)
            r = float(DC.ratio(bad[p.b, p.h].float().to(l.dtype).double(), want[p.b, p.h], A[p.b, p.h], True).max())
            n, lo = caught.get(d, (0, float("inf")))
            caught[d] = (n + 1, min(lo, r))
            if not r >= 2.0:
                missed.append((d, p.b, p.h, len(p.rows), p.probes, r))
    return l.kind, e32, honest, caught, missed, exact


@pytest.mark.parametrize("idx", range(len(SETS)), ids=IDS)
def test_honest_evaluation_passes_and_every_planted_defect_is_caught_with_fp8_caches(idx):
    kind, e32, honest, caught, missed, exact = _check(idx)
    print(f"{IDS[idx]} (fp8): e32 {e32:.2e}, honest ratio {honest:.3f}, defects "
          + ", ".join(f"{d} x{n} >= {r:.1f}" for d, (n, r) in sorted(caught.items())))
    assert exact, "a dequantised cache value is not a bf16 number"
    assert honest <= 1.0
    assert not missed, missed
    assert caught, "a set without a single planted defect checks nothing"


def test_every_defect_is_planted_in_every_kind_of_fp8_set():
    seen = {}
    for idx in range(len(SETS)):
        kind, _, _, caught, _, _ = _check(idx)
        seen.setdefault(kind, set()).update(caught)
    assert set(seen) == {"linear", "split", "ring"}
    for kind in seen:
        assert EXPECTED[kind] <= seen[kind], (kind, EXPECTED[kind] - seen[kind])


def test_the_constant_of_the_bound_holds_for_fp8_sets():
    """16 e32 <= C_BF16 <= 2^-13 with e32 measured on the dequantised sets (the reference's own error, not a kernel's)."""
    e32 = max(_check(idx)[1] for idx in range(len(SETS)))
    print(f"e32 over {len(SETS)} fp8 input sets (rows per wave instruction {K8.rows_per_wave(64)} / {K8.rows_per_wave(32)}): "
          f"{e32:.3e}; 16 e32 = {16 * e32:.3e}; c = {DC.C_BF16:.3e}")
    assert 16 * e32 <= DC.C_BF16 <= 2.0 ** -13


def _random_bf16(g, n):
    """n bf16 values of every magnitude: random bit patterns without inf / NaN."""
    bits = torch.randint(0, 2 ** 16, (n,), generator=g, dtype=torch.int32)
    bits = torch.where((bits >> 7) & 0xFF == 0xFF, bits & 0x807F | 0x3F80, bits)
    return (bits << 16).view(torch.float32).to(torch.bfloat16)


def test_quantiser_emulation_equals_float8_e4m3fn_rounding():
    """2^16 random bf16 values in blocks of 32 whose scale is known: the bytes equal torch's conversion of x * 2^(127 - sb)
    clamped to +-448, with saturating blocks, zero blocks, blocks at the sb = 0 clamp (denormal amax) and blocks whose
    scale 2^(sb - 127) is subnormal or tiny; the decoder inverts torch's."""
    g = torch.Generator().manual_seed(8)
    x = _random_bf16(g, 2 ** 16).view(-1, 32)
    n = x.shape[0]
    # moderate blocks (a random exponent per block keeps most elements inside e4m3's range)
    mod = (DC._randn(g, n // 2, 32) * torch.exp2(torch.randint(-140, 120, (n // 2, 1), generator=g).float())).to(torch.bfloat16)
    x[: n // 2] = mod
    x[0] = 0.0                                               # a zero block
    x[1] = 0.0
    x[1, 5] = -0.0
    x[2] = torch.tensor(2.0 ** -130).to(torch.bfloat16)      # denormal amax: sb clamps at 0, scale 2^-127 subnormal
    x[2, 3] = -2.0 ** -133
    x[3] = (DC._randn(g, 32) * 2.0 ** -120).to(torch.bfloat16)          # sb = 0 .. 2: the smallest scales
    x[4, :] = 1.0
    x[4, 0], x[4, 1], x[4, 2] = 1.9921875, -1.9921875, 1.875          # 255/128 -> 510 * 2^-8: saturates at 448; 480 too
    x[5] = 3.3895e38                                         # the largest bf16: sb = 246
    q, s = K8.quantise(x)
    xf = x.float()
    amax = xf.abs().amax(-1)
    sb = (torch.where(amax > 0, torch.floor(torch.log2(amax.double())), torch.tensor(-1000.0, dtype=torch.float64)) + 127 - 8)
    sb = sb.clamp(0, 254).to(torch.int64)
    sb = torch.where(amax < 2.0 ** -126, torch.zeros_like(sb), sb)          # (denormal amax: biased exponent 0)
    assert torch.equal(s[:, 0].long(), sb)
    y = (xf.double() * 2.0 ** (127.0 - sb.double())[:, None]).clamp(-448.0, 448.0)
    ref = y.float().to(torch.float8_e4m3fn)
    assert torch.equal(q, ref.view(torch.uint8))
    assert int((q & 0x7F == 0x7E).sum()) >= 3 and int((q & 0x7F == 0x7F).sum()) == 0          # +-448 reached, NaN never
    assert int(s[0, 0]) == 0 and int(q[0].max()) == 0 and int(q[1, 5]) == 0x80 and int(s[2, 0]) == 0 and int(s[5, 0]) == 246
    assert int(q[2, 0]) != 0 and int(q[2, 3]) != 0x80       # (2^-130 * 2^127 = 2^-3; 2^-133 * 2^127 = 2^-6: both survive)
    # the decoder: every byte value, against torch's own decoding
    allb = torch.arange(256, dtype=torch.uint8)
    t = allb.view(torch.float8_e4m3fn).float()
    assert torch.equal(torch.isnan(K8.LUT), torch.isnan(t)) and torch.equal(K8.LUT.nan_to_num(7.0), t.nan_to_num(7.0))
    d = K8.dequant(q, s)
    assert torch.equal(d.double(), ref.float().double() * 2.0 ** (sb.double() - 127.0)[:, None])
    assert bool((d.to(torch.bfloat16).float() == d).all())
    # quantising what was dequantised changes nothing: a position has one K and one V
    q2, s2 = K8.quantise(d)
    d2 = K8.dequant(q2, s2)
    assert torch.equal(d2, d)


def test_never_read_rows_become_nan_bytes():
    t = torch.zeros(1, 2, 3, 64, dtype=torch.bfloat16)
    t[0, 1, 2] = float("nan")
    t[0, 0, 1] = 3.0
    q, s = K8.quantise_rows(t)
    assert int(q[0, 1, 2].min()) == 0x7F and int(s[0, 1, 2].min()) == 0xFF and int(s[0, 0, 1, 0]) == 128 - 8
    d = K8.dequant(q, s)
    assert bool(torch.isnan(d[0, 1, 2]).all()) and int(torch.isnan(d).sum()) == 64 and float(d[0, 0, 1, 0]) == 3.0
    assert K8.rows_per_wave(64) == 16 and K8.rows_per_wave(32) == 32
