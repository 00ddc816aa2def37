"""Cached decode with more than 64 slots: the fused layer-tail launches take up to 256 sequences
(commu_decode_layer_tail, row groups 4 .. 15), so a DecodeState of 65 .. 256 slots no longer drops to one launch per Linear.

  * the fused path against the per-Linear chain at 96 slots (narrow model), 80 (wide) and 256 beside a side stream of GEMMs;
  * row independence: slots 0 .. 63 of a 96-slot state compute, bit for bit, what a 64-slot state computes;
  * slot-count invariance of the sampled sequences: ForcedDecoder through its captured graph and generate_stream;
  * the fp8 K/V cache at 96 slots."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]
DATA = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
NARROW, WIDE = (6, 8, 512, 1024), (3, 16, 1024, 2048)


def _model(shape, seed, eos_bias=None):
    from test_configs_gpu import build
    model = build(*shape, 1, 4146, seed=seed)[0]
    model.eval()
    model.same_length = True
    model.reset_length(1, 4146)
    if eos_bias is not None:
        with torch.no_grad():
            bias = model.crit.out_layers[0].bias
            bias.zero_()
            bias[1] = eos_bias                    # EOS
            bias[2] = -1e9                        # no BAR, no chord tokens: every iteration is a model step and a draw
            bias[195:304] = -1e9
    return model


@pytest.mark.parametrize("B,loaded,shape", [(96, False, NARROW), (80, False, WIDE), (256, True, NARROW)])
def test_fused_path_matches_the_per_linear_chain_beyond_64_slots(B, loaded, shape):
    """The body and bounds of test_decode_gpu.test_layer_tail_launch_matches_the_per_linear_chain at 96, 80 and 256 slots, 40
    consecutive steps: every step's logits within 1e-2 of their range of the chain's, the K/V caches within 2e-2, no
    workgroup gave up.  `loaded`: a second stream keeps the GPU busy with large GEMMs meanwhile, so the 16 row groups of
    the 256-slot launch do not start together."""
    import commu_amd.generate as G
    model = _model(shape, 23)
    g = torch.Generator().manual_seed(5 + B)
    ctx = torch.randint(2, 729, (11, B), generator=g).to(DEV)
    NSTEP = 40
    toks = torch.randint(2, 729, (NSTEP, B), generator=g).to(DEV)
    acts = (torch.rand(NSTEP, B, generator=g) < 0.9).to(torch.uint8).to(DEV)
    st_a, st_b = G.DecodeState(model, B, 11 + NSTEP + 8), G.DecodeState(model, B, 11 + NSTEP + 8)
    assert st_a.tail_ok
    assert st_a.t_sync.shape[1] == 48 * 64
    st_a.prefill(ctx)
    st_b.prefill(ctx)
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    worst = 0.0
    for i in range(NSTEP):
        if loaded and i % 4 == 0:
            with torch.cuda.stream(side):
                for _ in range(3):
                    big @ big
        assert G.USE_LAYER_TAIL
        la = st_a.step(toks[i], acts[i], acts[i]).clone()
        G.USE_LAYER_TAIL = False
        try:
            lb = st_b.step(toks[i], acts[i], acts[i]).clone()
        finally:
            G.USE_LAYER_TAIL = True
        rng = float(lb[:, :729].abs().max())
        err = float((la[:, :729] - lb[:, :729]).abs().max()) / rng
        worst = max(worst, err)
        assert err < 1e-2, (i, err)
    torch.cuda.synchronize()
    st_a.check()
    assert torch.equal(st_a.klen, st_b.klen)
    kerr = float((st_a.kc.float() - st_b.kc.float()).abs().max()) / float(st_b.kc.float().abs().max())
    verr = float((st_a.vc.float() - st_b.vc.float()).abs().max()) / float(st_b.vc.float().abs().max())
    print(f"layer tail vs per-Linear chain, {shape}, B={B}, loaded={loaded}: worst logit difference {worst:.2e} of range, "
          f"K cache {kerr:.2e}, V cache {verr:.2e}")
    assert kerr < 2e-2 and verr < 2e-2


def test_more_than_256_slots_keep_the_per_linear_chain():
    import commu_amd.generate as G
    model = _model(NARROW, 23)
    assert G.DecodeState(model, 256, 16).tail_ok
    assert not G.DecodeState(model, 257, 16).tail_ok


def test_a_row_does_not_depend_on_its_row_group_or_on_the_number_of_slots():
    """Slots 0 .. 63 of a 96-slot state carry the context, tokens and active flags of a 64-slot state: after each of 24
    steps their logits rows are EQUAL, bit for bit, and at the end so are their K/V rows.  (The 96-slot launch is the same
    kernel on a larger grid with another counter stride: a row's sums are formed in the same order wherever it sits.)
    Both states decode from the same cache content: the 64 slots' context rows are copied, so that the claim is about the
    decode step (whether the two prefills agree bit for bit is printed, not asserted)."""
    import commu_amd.generate as G
    model = _model(NARROW, 29)
    g = torch.Generator().manual_seed(17)
    T0, NSTEP = 11, 24
    ctx = torch.randint(2, 729, (T0, 96), generator=g).to(DEV)
    toks = torch.randint(2, 729, (NSTEP, 96), generator=g).to(DEV)
    acts = (torch.rand(NSTEP, 96, generator=g) < 0.85).to(torch.uint8).to(DEV)
    s96, s64 = G.DecodeState(model, 96, T0 + NSTEP + 8), G.DecodeState(model, 64, T0 + NSTEP + 8)
    assert s96.tail_ok and s64.tail_ok
    s96.prefill(ctx)
    s64.prefill(ctx[:, :64].contiguous())
    print("prefill of 96 and of 64 contexts bit-equal on the common slots:",
          torch.equal(s96.kc[:, :64], s64.kc) and torch.equal(s96.vc[:, :64], s64.vc))
    s96.kc[:, :64].copy_(s64.kc)
    s96.vc[:, :64].copy_(s64.vc)
    for i in range(NSTEP):
        a = s96.step(toks[i], acts[i], acts[i])
        b = s64.step(toks[i, :64].contiguous(), acts[i, :64].contiguous(), acts[i, :64].contiguous())
        assert torch.equal(a[:64], b), i
    torch.cuda.synchronize()
    s96.check()
    s64.check()
    assert torch.equal(s96.klen[:64], s64.klen)
    assert torch.equal(s96.kc[:, :64], s64.kc) and torch.equal(s96.vc[:, :64], s64.vc)
    assert float(s96.logits[64:, :729].abs().max()) > 0          # (the other 32 slots decoded too)


def _decode(model, B, uni, kv_dtype="bf16"):
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, B, generation_length=40, memory_length=128, temperature=0.95, top_k=32, kv_dtype=kv_dtype)
    dec.load([META] * B, [DATA] * B, uni[:B])
    with torch.no_grad():
        dec.run(use_graph=True)
    assert dec.graph is not None and dec.state.tail_ok
    dec.state.check()
    return dec.sequences()[0]


def test_forced_decoder_sequences_do_not_depend_on_the_number_of_slots():
    """ForcedDecoder through its captured graph, sampled (temperature 0.95, top_k 32), variates by attempt_uniforms: the
    sequences of slots 0 .. 63 of a 96-slot decoder are those of a 64-slot decoder with the same variates."""
    from commu_amd.generate import BatchedGenerator
    model = _model(NARROW, 31, eos_bias=-1e9)
    uni = np.stack([BatchedGenerator.attempt_uniforms(11, a, 41) for a in range(96)])
    s96, s64 = _decode(model, 96, uni), _decode(model, 64, uni)
    assert all(s_ is not None and len(s_) == 12 + 40 for s_ in s96)
    assert s96[:64] == s64
    assert len({tuple(s_) for s_ in s96}) > 20          # the attempts differ


def test_generate_stream_returns_the_same_sequences_at_64_and_at_96_slots():
    """generate_stream(need=96) with an accept rule that rejects some attempts (and EOS likely, so that slots are re-armed at
    different times): slots=96 returns exactly the sequences that slots=64 returns.  The number of attempts STARTED is
    speculative -- a free slot is re-armed while lower-numbered attempts are still in flight, so it depends on how many
    slots there are and on when they are polled (printed) -- unless it is bounded: with max_attempts=96 both runs start
    exactly 96 attempts, and then the counts are equal too."""
    from commu_amd.generate import BatchedGenerator
    model = _model(NARROW, 41, eos_bias=3.5)

    def accept(seq, rep):
        return seq is not None and len(seq) % 3 != 0

    def stream(slots, **kw):
        gen = BatchedGenerator(model, torch.device(DEV), generation_length=40, memory_length=128)
        out, started = gen.generate_stream(META, DATA, 0.95, 32, need=96, accept=accept, slots=slots, seed=5, **kw)
        assert gen._decoders[(min(slots, 96), False, False)].state.tail_ok
        return out, started
    o96, n96 = stream(96)
    o64, n64 = stream(64)
    print(f"attempts started: {n96} with 96 slots, {n64} with 64")
    assert len(o96) == 96 and o96 == o64
    assert len({len(s_) for s_ in o96}) > 1          # ragged lengths
    o96b, n96b = stream(96, max_attempts=96)
    o64b, n64b = stream(64, max_attempts=96)
    assert o96b == o64b and n96b == n64b == 96
    assert 0 < len(o96b) < 96 and o96b == o96[:len(o96b)]          # (some of the first 96 attempts were rejected)


def test_fp8_cache_at_96_slots():
    """kv_dtype="fp8" at 96 slots: the iteration graph is captured with the fused launches and the decode completes."""
    from commu_amd.generate import BatchedGenerator
    model = _model(NARROW, 31, eos_bias=-1e9)
    uni = np.stack([BatchedGenerator.attempt_uniforms(3, a, 41) for a in range(96)])
    seqs = _decode(model, 96, uni, kv_dtype="fp8")
    assert all(s_ is not None and s_[:12] == [0] + META and len(s_) == 12 + 40 for s_ in seqs)
