"""Host side of the fp8 K/V cache of the cached decode step (csrc/decode_kv8.hip).  Plain module, CPU tensors only.

STORAGE: e4m3 bytes [.., DH] (OCP float8_e4m3fn) + one E8M0 byte per 32 consecutive features [.., DH / 32].
QUANTISER (the kernel's recipe, which is commu_quant_mxfp8's): per block of 32,

    sb = clamp(biased_exponent(amax) - 8, 0, 254),   byte = rne_e4m3(clamp(x * 2^(127 - sb), -448, 448)),

so a block of zeros (or of bf16 denormals) gets sb = 0 and the value of a byte is e4m3(byte) * 2^(sb - 127).  The
emulation below rounds with integer / power-of-two arithmetic of its own; tests/test_kv8_contract_host.py compares it with
torch.float8_e4m3fn.

THE CONTRACT of the fp8 attention: a position has one K and one V, whatever step reads it, so for every launch

    want = decode_contract.contract_f64(dequant(cache after the append)),

with the bound of decode_contract unchanged: the dequantised values are exactly representable in bf16 (3 significand
bits times a power of two inside bf16's range), and the scales are powers of two, so applying one to a lane's partial
dot product is the same number as scaling the elements first.  to_fp8() turns a decode_contract.Launch into that form;
the builders of decode_contract are used as they are."""
import copy

import torch

import decode_contract as DC

NAN_BYTE, NAN_SCALE = 0x7F, 0xFF          # what rows that must never be read hold: e4m3 NaN times 2^128 (inf as a float)


def rows_per_wave(DH):
    """Rows per wave instruction of decode_attn_kv8_kernel: a lane holds 16 features (16 bytes)."""
    return 64 // (DH // 16)


def _pow2(e):
    """2^e as float32 for an int32 tensor e in [-126, 127]."""
    return ((e + 127) << 23).view(torch.float32)


def rne_e4m3(y):
    """float32 |y| <= 448 -> e4m3 bytes, round to nearest even, by the format's definition: below 2^-6 the grid is
    2^-9 (subnormals), at exponent e it is 2^(e - 3)."""
    y = y.float().contiguous()
    bits = y.view(torch.int32)
    a = y.abs()
    e = (((a.view(torch.int32) >> 23) & 0xFF) - 127).clamp(min=-6)
    step = _pow2(e - 3)
    n = torch.round(a / step)                               # half to even; a / step is exact, < 16
    over = n >= 16                                          # rounded up into the next binade
    e = torch.where(over, e + 1, e)
    n = torch.where(over, torch.full_like(n, 8.0), n).to(torch.int32)
    normal = n >= 8
    byte = torch.where(normal, ((e + 7) << 3) | (n - 8), n)          # (subnormals and zero: exponent field 0, n = 0 .. 7)
    byte = byte | torch.where(bits < 0, 0x80, 0)
    return byte.to(torch.uint8)


def quantise(x):
    """x [.., DH] (bf16 or float, DH a multiple of 32) -> (bytes uint8 [.., DH], scale bytes uint8 [.., DH / 32])."""
    x = x.float()
    DH = x.shape[-1]
    assert DH % 32 == 0
    blk = x.reshape(*x.shape[:-1], DH // 32, 32)
    amax = blk.abs().amax(-1).contiguous()
    eb = (amax.view(torch.int32) >> 23) & 0xFF
    sb = (eb - 8).clamp(0, 254)
    inv = ((254 - sb) << 23).view(torch.float32)            # 2^(127 - sb) (a product below 2^-126 rounds to zero anyway)
    y = (blk * inv[..., None]).clamp(-448.0, 448.0)
    return rne_e4m3(y).reshape(x.shape), sb.to(torch.uint8)


def _lut():
    b = torch.arange(256, dtype=torch.int32)
    e, m = (b >> 3) & 15, (b & 7).float()
    v = torch.where(e == 0, m * 2.0 ** -9, (8 + m) * _pow2((e - 10).clamp(min=-126)))
    v = torch.where(b >= 128, -v, v)
    v[0x7F] = v[0xFF] = float("nan")
    return v


LUT = _lut()


def dequant(q, s):
    """bytes [.., DH], scale bytes [.., DH / 32] -> float32 [.., DH] (exact; NaN for byte 0x7F / 0xFF or scale 0xFF)."""
    DH = q.shape[-1]
    v = LUT[q.long()].reshape(*q.shape[:-1], DH // 32, 32).double()
    sc = torch.where(s == 255, torch.full(s.shape, float("nan"), dtype=torch.float64), 2.0 ** (s.double() - 127.0))
    return (v * sc[..., None]).float().reshape(q.shape)


def quantise_rows(t):
    """A cache [B, H, L, DH] whose never-read rows hold NaN -> (bytes, scales) with those rows 0x7F / 0xFF."""
    dead = torch.isnan(t).any(-1)
    q, s = quantise(torch.where(dead[..., None], torch.zeros((), dtype=t.dtype), t))
    q[dead] = NAN_BYTE
    s[dead] = NAN_SCALE
    return q, s


class Launch8(DC.Launch):
    """A decode_contract.Launch in fp8 form: kc8 / vc8 / ks / vs are the stored bytes AFTER the append, kc / vc their
    dequantised values (bf16, exact), so evaluate() of the base class is the contract of the fp8 kernel."""

    def caches_before8(self, append):
        """(kc8, vc8, ks, vs) a launch starts from: with append the new token's row of every active sequence holds NaN."""
        out = [t.clone() for t in (self.kc8, self.vc8, self.ks, self.vs)]
        if append:
            for b in range(self.B):
                if self.active[b]:
                    out[0][b, :, self.new_row[b]] = NAN_BYTE
                    out[1][b, :, self.new_row[b]] = NAN_BYTE
                    out[2][b, :, self.new_row[b]] = NAN_SCALE
                    out[3][b, :, self.new_row[b]] = NAN_SCALE
        return out


def to_fp8(l):
    """The fp8 form of a bf16 Launch (linear | split | ring).  qkv stays bf16: the kernel quantises the new token's K and V
    itself, and kc / vc hold their quantised image in the new row like any other row.  RPW becomes the fp8 kernel's rows per
    wave instruction; the defects whose design depends on it (decode_contract._finish) are kept only where the condition
    still holds with the new grouping (every condition with 2 RPW rows implies the one with RPW rows)."""
    assert l.dtype == torch.bfloat16 and l.kind in ("linear", "split", "ring")
    f = Launch8()
    f.__dict__.update(l.__dict__)
    f.kc8, f.ks = quantise_rows(l.kc)
    f.vc8, f.vs = quantise_rows(l.vc)
    f.kc, f.vc = dequant(f.kc8, f.ks).to(l.dtype), dequant(f.vc8, f.vs).to(l.dtype)
    f.stale_k = dequant(*quantise(l.stale_k)).to(l.dtype)
    f.stale_v = dequant(*quantise(l.stale_v)).to(l.dtype)
    f.RPW = rows_per_wave(l.DH)
    f.pairs = []
    for p in l.pairs:
        c = copy.copy(p.ctx)
        c.update(RPW=f.RPW, stale_k=f.stale_k[p.b, p.h], stale_v=f.stale_v[p.b, p.h])
        q = DC.Pair(p.b, p.h, p.rows, p.dist, c)
        q.probes = list(p.probes)
        q.designed = [d for d in p.designed
                      if not (d == "dist_group" and len({r // f.RPW for r in p.probes}) < 2)
                      and not (d == "v_shift" and len(p.rows) < 2 * f.RPW)]
        f.pairs.append(q)
    return f
