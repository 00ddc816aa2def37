"""The decode layer tail and head against the staged float64 contract, element by element (tests/tail_contract.py: the
stage contracts, the bounds, the input sets, the exact layout probes; tests/test_tail_contract_host.py proves on the CPU
that the same sets catch every planted defect):

  commu_decode_layer_tail (decode_tail_kernel 8 and 10 heads, decode_tail_wide_kernel; QKV and LOGITS modes),
  commu_decode_head, commu_decode_tail_pack (csrc/decode_tail.hip),
  and the per-Linear chain that the tail replaces (ops.gemm_nt with bias / relu / resid epilogues at M = B,
  ops.layernorm_fwd), held to the same stage bounds.

Every stage is checked from what the launch itself stored for the stage before it.  Guards on every launch: padded
pitches, NaN in the pad columns of the inputs, sentinels in the extra rows and pad columns of every output (logits
columns 729 .. 735 included), inactive rows keep their bits, *err == 0, the three arrival counters of every row group in
use at 32 and every other word of the sync block (and past it) untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import tail_contract as TC  # noqa: E402

DEV = "cuda"
SETS = TC.tail_sets()
HEADS = TC.head_sets()


def _pack(W):
    """commu_decode_tail_pack of a CPU weight [N, K], read through a padded row pitch."""
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    N, K = W.shape
    Wp = torch.full((N, K + 8), float("nan"), dtype=W.dtype)
    Wp[:, :K] = W
    Wd = Wp.to(DEV)
    nbytes = call("commu_decode_tail_pack_bytes", N, K)
    out = torch.full((nbytes // 2 + 64,), TC.SENT, device=DEV, dtype=torch.bfloat16)
    call("commu_decode_tail_pack", _p(Wd), K + 8, N, K, _p(out), _s())
    torch.cuda.synchronize()
    assert bool((out[nbytes // 2:] == TC.SENT).all())
    return out


def _padded(t, fill=float("nan")):
    p = torch.full((t.shape[0], t.shape[1] + TC.PAD), fill, dtype=t.dtype)
    p[:, :t.shape[1]] = t
    return p.to(DEV)


class _Dev:
    """A TailSet on the GPU."""

    def __init__(self, s):
        self.s = s
        self.vec, self.h = _padded(s.vec), _padded(s.h)
        self.packs = {k: _pack(getattr(s, k)) for k in ("Wo", "W1", "W2", "Wn")}
        for k in ("b1", "b2", "bn", "g1", "be1", "g2", "be2"):
            setattr(self, k, getattr(s, k).clone().to(DEV))
        self.active = None if s.active is None else s.active.to(DEV)

    def launch(self, use_active=True, Nn=None):
        """One commu_decode_layer_tail launch into fresh buffers (the counters zeroed here); the buffers on the CPU."""
        from commu_amd._lib import call
        from commu_amd.ops import _p, _s
        s = self.s
        b = {k: v.to(DEV) for k, v in TC.buffers(s).items()}
        logits = s.mode == "logits"
        call("commu_decode_layer_tail", _p(self.vec), self.vec.stride(0), _p(self.h), self.h.stride(0), _p(self.packs["Wo"]),
             _p(self.packs["W1"]), _p(self.b1), _p(self.packs["W2"]), _p(self.b2), _p(self.g1), _p(self.be1), s.eps1,
             _p(self.g2), _p(self.be2), s.eps2, s.d_ln, _p(self.packs["Wn"]), s.Nn if Nn is None else Nn,
             _p(self.bn) if logits else None, 1 if logits else 0, _p(self.active) if use_active else None, _p(b["z1"]),
             _p(b["hid"]), _p(b["z2"]), _p(b["h_out"]), b["h_out"].stride(0), _p(b["out"]), b["out"].stride(0), s.B, s.D, s.DI,
             s.HD, _p(b["sync"]), _p(b["err"]), _s())
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in b.items()}


def _report(what, res):
    print(what + ": " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert TC.worst(res) <= 1.0, (what, res)


@pytest.mark.parametrize("idx", range(len(SETS)), ids=[s[0] for s in SETS])
def test_layer_tail_vs_staged_float64_contract(idx):
    """commu_decode_layer_tail on every input set: every stage bound, the LayerNorm rule on h_out (and on a in the W2 = 0
    sets), the tie cap on the kernel's own z1 / z2, every guard; LOGITS sets once more with active = null."""
    s = TC.build_tail(*SETS[idx][1])
    d = _Dev(s)
    _report(f"layer tail {SETS[idx][0]}", TC.check(s, d.launch()))
    if s.active is not None:
        _report(f"layer tail {SETS[idx][0]} active = null", TC.check(s, d.launch(use_active=False), use_active=False))


@pytest.mark.parametrize("idx", range(len(SETS)), ids=[s[0] for s in SETS])
def test_per_linear_chain_vs_staged_float64_contract(idx):
    """The chain that the tail replaces, on the same sets and held to the same stage bounds: gemm_nt (+ resid), layernorm_fwd,
    gemm_nt (+ bias, relu), gemm_nt (+ bias, resid), layernorm_fwd, gemm_nt (bf16, or + bias in fp32).  Its LN1 output is
    stored, so it is held to the LayerNorm rule directly as well."""
    from commu_amd import ops
    s = TC.build_tail(*SETS[idx][1])
    B, D, d_ln = s.B, s.D, s.d_ln
    vec, h = _padded(s.vec), _padded(s.h)
    dev = lambda t: t.clone().to(DEV)
    Wo, W1, W2, Wn = dev(s.Wo), dev(s.W1), dev(s.W2), dev(s.Wn)
    b = {k: v.to(DEV) for k, v in TC.buffers(s).items()}
    a = torch.full((B, D), TC.SENT, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt(vec[:, :s.HD], Wo, out=b["z1"][:B], resid=h[:, :D])
    ops.layernorm_fwd(b["z1"][:B], dev(s.g1), dev(s.be1), y=a, eps=s.eps1)
    ops.gemm_nt(a, W1, out=b["hid"][:B], bias=dev(s.b1), relu=True)
    ops.gemm_nt(b["hid"][:B], W2, out=b["z2"][:B], bias=dev(s.b2), resid=a)
    ops.layernorm_fwd(b["z2"][:B], dev(s.g2), dev(s.be2), y=b["h_out"][:B, :D], eps=s.eps2)
    if s.mode == "logits":
        ops.gemm_nt(b["h_out"][:B, :D], Wn, out=b["out"][:B, :s.Nn], bias=dev(s.bn))
    else:
        ops.gemm_nt(b["h_out"][:B, :D], Wn, out=b["out"][:B, :s.Nn])
    torch.cuda.synchronize()
    b = {k: v.cpu() for k, v in b.items()}
    b["sync"][TC.counter_words(s)] = TC.NGRP          # (the chain has no counters: the sync block as a launch leaves it)
    res = TC.check(s, b, use_active=False)
    a = a.cpu()
    res["LN1"] = TC.ln_rule(a.float(), b["z1"][:B].float(), s.g1, s.be1, s.eps1, d_ln)[0] + int((a[:, d_ln:] != 0).sum())
    _report(f"per-Linear chain {SETS[idx][0]}", res)


def _head_launch(s):
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    b = {k: v.to(DEV) for k, v in TC.head_buffers(s).items()}
    tok, E, Wp = s.tok.to(DEV), s.E.to(DEV), _pack(s.W)
    call("commu_decode_head", _p(tok), _p(E), s.d_true, TC.V, s.scale, _p(Wp), _p(b["h_out"]), b["h_out"].stride(0),
         _p(b["out"]), b["out"].stride(0), s.B, s.D, s.DI, s.HD, _p(b["zero"]), s.n_zero, _s())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in b.items()}


@pytest.mark.parametrize("i", range(len(HEADS)), ids=[h[0] for h in HEADS])
def test_head_vs_float64_contract(i):
    """commu_decode_head: h_out bit for bit (zero pad columns, NaN rows for ids outside the vocabulary), qkv within the
    product bound of the stored h_out, n_zero words cleared (not a multiple of 256) and not one more."""
    s = TC.build_head(*HEADS[i][1])
    res = TC.head_check(s, _head_launch(s))
    print(f"{HEADS[i][0]}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert TC.head_worst(res) <= 1.0, res


@pytest.mark.parametrize("shape", list(TC.SHAPES))
def test_exact_layout_probes(shape):
    """No bound at all.  Head probe: E[v] a unit vector and scale 1, so qkv[row, n] == Wqkv[n, k(tok[row])] bit for bit for
    every n < 3 HD (the packed layout and the tile-to-column map of phase 4).  Phase-1 probe: vec rows are unit vectors
    and h = 0, so z1[row, n] == Wo[n, k(row)]."""
    D, DI, HD = TC.SHAPES[shape]
    B = 33 if shape == "wide" else 37
    s = TC.build_head(shape, B, 500 if shape == "n640" else D, probe=True)
    res = TC.head_check(s, _head_launch(s))
    assert TC.head_worst(res) == 0, res
    p, k = TC.phase1_probe(shape, B)
    b = _Dev(p).launch()
    assert int(b["err"][0]) == 0
    assert torch.equal(b["z1"][:B], p.Wo[:, k].T.contiguous())


def test_pack_matches_the_layout_formula_byte_for_byte():
    """commu_decode_tail_pack against the layout formula above load_w, computed on the host (padded ldw; rows >= N zero)."""
    g = torch.Generator().manual_seed(11)
    for N, K in TC.PACK_CASES:
        W = torch.randint(-2 ** 15, 2 ** 15, (N, K), generator=g, dtype=torch.int16)          # (any bit pattern)
        got = _pack(W.view(torch.bfloat16))
        want = TC.pack_layout(W, N, K)
        assert torch.equal(got[:want.numel()].cpu().view(torch.int16), want), (N, K)


def test_logits_launch_refuses_a_vocabulary_of_one_column_tile():
    """Nn <= 512 in LOGITS mode: -22 and nothing launched (the packed copy of such a weight has one column tile per
    workgroup, the LOGITS kernels walk two); 513 .. 1024 are taken (729 in every LOGITS set above)."""
    from commu_amd._lib import CommuHipError
    s = TC.build_tail("n512", 5, "logits", 512)
    d = _Dev(s)
    for Nn in (1, 512, 1025):
        with pytest.raises(CommuHipError, match="-22"):
            d.launch(Nn=Nn)


def test_decode_state_takes_the_layer_tail_only_for_a_two_tile_vocabulary():
    """DecodeState.tail_ok: 512 < V <= 1024 (the LOGITS launch refuses the others); a model with another vocabulary
    decodes through the per-Linear launches instead of raising at its first step."""
    import commu_amd.generate as G
    from test_configs_gpu import build
    model = build(1, 8, 512, 1024, 1, 16, seed=3)[0]
    model.eval()
    assert G.DecodeState(model, 2, 16).tail_ok
    V = model.n_token
    try:
        for v in (400, 512, 1025):
            model.n_token = v
            assert not G.DecodeState(model, 2, 16).tail_ok, v
    finally:
        model.n_token = V
