"""commu_decode_layer_tail and commu_decode_head at 65 .. 256 sequences (row groups 4 .. 15) against the staged float64
contract, element by element (tests/tail_slots_contract.py: tail_contract's stage bounds, unchanged, on sets of up to 256
rows; tests/test_tail_slots_contract_host.py proves on the CPU that the same sets catch every planted defect, a row-group
alias included).

Guards on every launch: padded pitches, NaN in the pad columns of the inputs, sentinels in the rows past B and the pad
columns of every output, inactive logits rows (one of a row group >= 4 and the last row among them) keep their bits,
*err == 0, the three arrival counters of every row group in use hold 32, and every other word of the [3][16][64] sync block
(and past it) is untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import tail_slots_contract as SC  # noqa: E402
from test_tail_contract_gpu import DEV, _Dev, _pack  # noqa: E402

SETS = SC.tail_sets()
HEADS = SC.head_sets()


def _launch(d, use_active=True, B=None):
    """One commu_decode_layer_tail launch of the set on the GPU into fresh buffers; the buffers on the CPU."""
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    s = d.s
    b = {k: v.to(DEV) for k, v in SC.buffers(s).items()}
    logits = s.mode == "logits"
    call("commu_decode_layer_tail", _p(d.vec), d.vec.stride(0), _p(d.h), d.h.stride(0), _p(d.packs["Wo"]),
         _p(d.packs["W1"]), _p(d.b1), _p(d.packs["W2"]), _p(d.b2), _p(d.g1), _p(d.be1), s.eps1, _p(d.g2), _p(d.be2), s.eps2,
         s.d_ln, _p(d.packs["Wn"]), s.Nn, _p(d.bn) if logits else None, 1 if logits else 0,
         _p(d.active) if use_active else None, _p(b["z1"]), _p(b["hid"]), _p(b["z2"]), _p(b["h_out"]), b["h_out"].stride(0),
         _p(b["out"]), b["out"].stride(0), s.B if B is None else B, s.D, s.DI, s.HD, _p(b["sync"]), _p(b["err"]), _s())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in b.items()}


def _report(what, res):
    print(what + ": " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert SC.worst(res) <= 1.0, (what, res)


@pytest.mark.parametrize("idx", range(len(SETS)), ids=[s[0] for s in SETS])
def test_layer_tail_vs_staged_float64_contract(idx):
    """Every stage bound, the LayerNorm rule on h_out, the tie cap on the kernel's own z1 / z2, every guard; LOGITS sets
    once more with active = null."""
    s = SC.build_tail(*SETS[idx][1])
    d = _Dev(s)
    _report(f"layer tail {SETS[idx][0]}", SC.check(s, _launch(d)))
    if s.active is not None:
        _report(f"layer tail {SETS[idx][0]} active = null", SC.check(s, _launch(d, use_active=False), use_active=False))


@pytest.mark.parametrize("i", range(len(HEADS)), ids=[h[0] for h in HEADS])
def test_head_vs_float64_contract(i):
    """commu_decode_head: h_out bit for bit, qkv within the product bound of the stored h_out, and the counters of six
    layer-tail launches of this many sequences cleared (n_zero words, not a multiple of 256) and not one word more."""
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    s = SC.build_head(*HEADS[i][1])
    assert s.n_zero == SC.LAYERS * call("commu_decode_tail_sync_words_for", s.B) + 37
    b = {k: v.to(DEV) for k, v in SC.head_buffers(s).items()}
    tok, E, Wp = s.tok.to(DEV), s.E.to(DEV), _pack(s.W)
    call("commu_decode_head", _p(tok), _p(E), s.d_true, SC.V, s.scale, _p(Wp), _p(b["h_out"]), b["h_out"].stride(0),
         _p(b["out"]), b["out"].stride(0), s.B, s.D, s.DI, s.HD, _p(b["zero"]), s.n_zero, _s())
    torch.cuda.synchronize()
    res = SC.head_check(s, {k: v.cpu() for k, v in b.items()})
    print(f"{HEADS[i][0]}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert SC.head_worst(res) <= 1.0, res


def test_supported_range_and_sync_words():
    """1 .. 256 sequences on the three shapes, 257 refused by the query and by both launches (-22, nothing launched: the
    buffers keep their sentinels); the sync block is [3][4][64] words up to 64 sequences and [3][16][64] beyond."""
    from commu_amd._lib import CommuHipError, call
    from commu_amd.ops import _p, _s
    for D, DI, HD in SC.TC.SHAPES.values():
        assert [call("commu_decode_tail_supported", B, D, DI, HD) for B in (0, 1, 64, 65, 128, 256, 257)] == [0, 1, 1, 1, 1, 1, 0]
    assert call("commu_decode_tail_supported", 256, 512, 2048, 512) == 0
    assert call("commu_decode_tail_sync_words_for", 64) == call("commu_decode_tail_sync_words") == 12 * SC.CNT_STRIDE
    assert call("commu_decode_tail_sync_words_for", 1) == 12 * SC.CNT_STRIDE
    assert [call("commu_decode_tail_sync_words_for", B) for B in (65, 256)] == [48 * SC.CNT_STRIDE] * 2
    assert [call("commu_decode_tail_sync_words_for", B) for B in (0, 257)] == [0, 0]
    s = SC.build_tail("n512", 65, "qkv", 512)
    d = _Dev(s)
    with pytest.raises(CommuHipError, match="-22"):
        _launch(d, B=257)
    h = SC.build_head("n512", 65, 512)
    b = {k: v.to(DEV) for k, v in SC.head_buffers(h).items()}
    with pytest.raises(CommuHipError, match="-22"):
        call("commu_decode_head", _p(h.tok.to(DEV)), _p(h.E.to(DEV)), h.d_true, SC.V, h.scale, _p(_pack(h.W)), _p(b["h_out"]),
             b["h_out"].stride(0), _p(b["out"]), b["out"].stride(0), 257, h.D, h.DI, h.HD, _p(b["zero"]), h.n_zero, _s())
    torch.cuda.synchronize()
    assert bool((b["zero"] == SC.SYNC_SENT).all()) and bool((b["out"] == SC.SENT).all())
