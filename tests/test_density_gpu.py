"""The note density on the GPU.  The defining property: a draw under the rule is bit for bit the draw the voices kernel makes
for the same inputs with bias[b] = -inf at the ids of tests/density_contract.bans and the rule absent -- so the sampler test
needs no tolerance: the new kernel (commu_sample_args.density_ctl) against the existing one, once and compounding (Q5).  Then
through the decode loop: captured graph == eager == separate launches, off-slots bit for bit a decoder that never heard of
the feature, teeth, a primed slot, in-place switching, the fp8 sliding cache, fp32 parity, the request pool with both arm
launches and the command line."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import density_contract as DC  # noqa: E402
import test_density_host as DH  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_note_order_gpu as NG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
import test_voices_gpu as VG  # noqa: E402
import test_voices_host as VH  # noqa: E402

DEV = "cuda"
V = 729
LD_SEQ = NG.LD_SEQ
NEG = float("-inf")
ROOT = NG.ROOT
bits = SR.bits
CTX = VH.CTX
W, pos, dur, note = DC.word, VH.pos, VH.dur, DH.note
same_row = NG.same_row
fill = VG.fill


# ------------------------------------------------------------------------------------------------ 1. the sampler
def kernel_cases():
    """(name, tokens, F_LEN or None, density word, note-order word, voice word): the rows of the voices test under a cycle
    of density words, the host test's edge cases, then what only the kernel can get wrong."""
    cycle = [W(1), W(0, 1), W(2, 2), -1, W(3), 0, W(1, 1)]
    cases = [(n, t, ln, cycle[i % len(cycle)], o, v) for i, (n, t, ln, v, o) in enumerate(VG.kernel_cases())]
    cases += [(n, t, ln, c, o, v) for n, t, ln, c, o, v, _ in DH.EDGE_CASES]
    three = note(0) + note(4, 61) + note(8, 62)
    # the current bar holds 63 / 64 / 65 tokens since its BAR: the BAR in lane 63 of chunk 0, in lane 0 and in lane 1 of
    # chunk 1; the bar before it holds four notes that must not be counted
    for k in (63, 64, 65):
        t = CTX + [2] + three + note(12, 63) + [2] + three + fill(k - 12)
        assert t[-k - 1] == 2 and 2 not in t[-k:]
        cases += [("bar_of_%d_tokens_lower" % k, t, None, W(4), 0, 0), ("bar_of_%d_tokens_upper" % k, t, None, W(1, 3), 0, 0)]
    # the current bar holds 130 tokens, its notes in three chunks
    t = CTX + [2] + three + [2] + note(0) + fill(58) + note(4, 61) + fill(58) + note(8, 62) + fill(2)
    assert t[-131] == 2 and 2 not in t[-130:]
    cases += [("bar_of_130_tokens_lower", t, None, W(4), 0, 0), ("bar_of_130_tokens_upper", t, None, W(2, 3), 0, 0),
              ("bar_of_130_tokens_neither", t, None, W(3, 4), 0, 0)]
    # the one counted note has its DURATION in lane 0 of chunk 1 (index L - 65), its PITCH .. POSITION in lanes 1 .. 3
    t = CTX + [2] + three + [2] + note(0) + fill(64)
    assert t[-65] == dur(4)
    cases += [("duration_in_lane_0_of_chunk_1_lower", t, None, W(2), 0, 0),
              ("duration_in_lane_0_of_chunk_1_upper", t, None, W(0, 1), 0, 0)]
    # the lower bound with a bias that allows Bar and EOS only: nothing is left (row NOTHING below)
    cases += [("only_bar_and_eos_left", CTX + [2] + note(0), None, W(2), 0, 0)]
    return cases


@pytest.fixture(scope="module")
def rows():
    from commu_amd._lib import call
    from commu_amd.generate import CLASS_CTL_DTYPE, event_grammar, harmony_table
    cases = kernel_cases()
    n = len(cases)
    assert 48 <= n <= 96
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    pick = torch.arange(n) % logits.shape[0]                             # (the 64 rows of the sampling test, tiled)
    logits, wrong, us, t, k, p = logits[pick], wrong[pick], us[pick], t[pick], k[pick], p[pick]
    assert bool((t == 0).any()) and bool((t != 0).any())                  # greedy rows and sampled rows
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(n, nf, dtype=torch.int32)
    seq = torch.full((n, LD_SEQ), 310, dtype=torch.int32)                 # (behind the tokens: durations)
    dctl = torch.zeros(n, dtype=torch.int32)
    octl = torch.zeros(n, dtype=torch.int32)
    vctl = torch.zeros(n, dtype=torch.int32)
    banned = []
    bias = torch.zeros(n, 768)
    for b, (name, tokens, length, c, o, v) in enumerate(cases):
        assert len(tokens) <= LD_SEQ
        seq[b, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32)
        st[b, 0] = len(tokens) if length is None else length
        st[b, 10] = 1                                                     # F_CUR: one chord placed
        dctl[b], octl[b], vctl[b] = c, o, v
        banned.append(DC.bans(seq[b].tolist(), int(st[b, 0]), c, o, v))
        # teeth: the ids the rule takes away are the likely ones -- Bar, and a position that no other rule bans (the last)
        bias[b, [i for i in (2, 559) if i in banned[-1]]] = 14.0
        if name == "only_bar_and_eos_left":
            bias[b] = NEG
            bias[b, 1] = bias[b, 2] = 0.0
    # the hand-written expectations of the host test hold for the padded rows too
    first = len(VG.kernel_cases())
    for i, (name, _, _, _, _, _, want) in enumerate(DH.EDGE_CASES):
        assert cases[first + i][0] == name and banned[first + i] == sorted(want), name
    rec = np.zeros((n, 8), dtype=CLASS_CTL_DTYPE)                         # no class controls: the base-triple table
    for b in range(n):
        rec[b, :] = (float(t[b]), int(k[b]), float(p[b]), 0)
    ct = torch.full((n, 4), 199, dtype=torch.int32)
    return dict(n=n, cases=cases, logits=logits, wrong=wrong, us=us, bias=bias, state=st, seq=seq, chord_tok=ct, ctl=octl,
                vctl=vctl, dctl=dctl, banned=banned, gram=torch.from_numpy(event_grammar()),
                gram_on=torch.tensor([b % 2 for b in range(n)], dtype=torch.uint8), harm=torch.from_numpy(harmony_table()),
                harm_on=torch.tensor([(b // 2) % 2 for b in range(n)], dtype=torch.uint8),
                cls=torch.from_numpy(rec.view(np.int32).reshape(n, 8, 4)))


def launch(r, logits, density="dctl", voices="vctl", order="ctl", bias=None):
    """One launch of commu_sample_topk on fresh device copies (token -7, probs_out -3.0, logp_out 7.0 before it), the
    class records given and the scalars poisoned.  density / voices / order: the rows' words by name, None (a null
    pointer) or a tensor."""
    from commu_amd._lib import SampleArgs, call, struct_args
    n = r["n"]
    d = lambda x: x.to(DEV).contiguous()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    words = lambda x: None if x is None else d(r[x] if isinstance(x, str) else x)
    lg = logits.clone().to(DEV)
    pr = torch.full((n, V), -3.0, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n, 2), 7.0, device=DEV)
    h = {k: d(r[k]) for k in ("wrong", "us", "gram", "gram_on", "harm", "harm_on", "state", "seq", "chord_tok", "cls")}
    bd = d(r["bias"] if bias is None else bias)
    od, vd, dd = words(order), words(voices), words(density)
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=n, V=V, wrong=ptr(h["wrong"]), ldw=V, uniforms=ptr(h["us"]),
        temperature=5.0, top_k=3, top_p=0.3, token=ptr(tok), probs_out=ptr(pr), ldp=V, logp_out=ptr(lp),
        bias=ptr(bd), ld_bias=bd.stride(0), gram=ptr(h["gram"]), ld_gram=h["gram"].stride(0), gram_on=ptr(h["gram_on"]),
        harm=ptr(h["harm"]), ld_harm=h["harm"].stride(0), harm_on=ptr(h["harm_on"]), state=ptr(h["state"]),
        seq=ptr(h["seq"]), ld_seq=LD_SEQ, chord_tok=ptr(h["chord_tok"]), ld_chord=4, cls_ctl=ptr(h["cls"]),
        order_ctl=ptr(od), voice_ctl=ptr(vd), density_ctl=ptr(dd))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()


def banned_bias(r):
    out = r["bias"].clone()
    for b, ids in enumerate(r["banned"]):
        out[b, ids] = NEG
    return out


def test_sampler_equals_the_voices_kernel_with_the_bans_in_the_bias(rows):
    """Fails on the parent: commu_sample_args has no density_ctl."""
    r, n = rows, rows["n"]
    got = launch(r, r["logits"])
    want = launch(r, r["logits"], density=None, bias=banned_bias(r))
    free = launch(r, r["logits"], density=None)
    for b in range(n):
        assert same_row(got, want, b), (r["cases"][b][0], int(got[1][b]), int(want[1][b]))
        for i in r["banned"][b]:
            assert float(got[2][b, i]) == 0.0 or int(got[1][b]) == -1, (r["cases"][b][0], i)
        if int(r["dctl"][b]) < 0 or not r["banned"][b]:                  # off, or nothing banned: the voices kernel's draw
            assert same_row(got, free, b), r["cases"][b][0]
    differ = [r["cases"][b][0] for b in range(n) if int(got[1][b]) != int(free[1][b])]
    print("rows:", n, "; rows whose token differs from the launch without the rule:", len(differ), differ)
    assert len(differ) >= 12
    nothing = [c[0] for c in r["cases"]].index("only_bar_and_eos_left")
    assert int(got[1][nothing]) == -1 and bool(torch.isnan(got[3][nothing]).all()) and bool(torch.isnan(got[2][nothing]).all())
    assert int(free[1][nothing]) in (1, 2)
    assert int((got[1] >= 1).sum()) >= n // 2
    # Q5: the same two launches again on the logits the first ones left -- the same bans on the compounded rows
    got2 = launch(r, got[0])
    want2 = launch(r, want[0], density=None, bias=banned_bias(r))
    for b in range(n):
        assert same_row(got2, want2, b), r["cases"][b][0]
    assert not torch.equal(bits(got2[0]), bits(got[0]))                   # (the sampled rows were divided again)
    # every word off, and every word 0 (on, no bound): the voices kernel bit for bit
    for word in (-1, 0):
        off = launch(r, r["logits"], density=torch.full((n,), word, dtype=torch.int32))
        assert all(same_row(off, free, b) for b in range(n)), word


def test_entry_point_refusal_and_ops(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    r = rows
    with pytest.raises(CommuHipError, match="-22"):
        launch(r, r["logits"], voices=None)                               # density_ctl without voice_ctl
    with pytest.raises(CommuHipError, match="-22"):
        launch(r, r["logits"], order=None)                                # ... without what voice_ctl requires
    d = lambda x: x.to(DEV)
    with pytest.raises(CommuHipError, match="density: voices= expected"):
        ops.sample_topk(d(r["logits"].clone()), 0.9, 32, uniforms=d(r["us"]), density=d(r["dctl"]))
    with pytest.raises(CommuHipError, match="density controls"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, uniforms=d(r["us"]), bias=d(r["bias"]),
                        class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])), note_order=d(r["ctl"]), voices=d(r["vctl"]),
                        density=d(r["dctl"]).float())
    # ops.sample_topk(density=) makes the same launch (it builds the all-off grammar and harmony itself)
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), uniforms=d(r["us"]), top_p=0.3, bias=d(r["bias"]),
                          class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])), note_order=d(r["ctl"]), voices=d(r["vctl"]),
                          density=d(r["dctl"]))
    plain = dict(r, gram_on=torch.zeros_like(r["gram_on"]), harm_on=torch.zeros_like(r["harm_on"]))
    ref = launch(plain, r["logits"])
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 2. through the loop
GLEN = NG.GLEN
run, separate_launches = LBG.run, LBG.separate_launches
fixture_model = NG.fixture_model


def loaded(z, model, B, density=None, **kw):
    """test_voices_gpu.loaded (grammar on, log-probabilities recorded, the steering row) with set_density's value."""
    from commu_amd.generate import ForcedDecoder
    prompts, glen, triple, bias = kw.pop("prompts", None), kw.pop("glen", GLEN), kw.pop("triple", (0.95, 32)), kw.pop("bias", None)
    dec = ForcedDecoder(model, B, glen, 4146, triple[0], triple[1], **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES) if bias is None else bias)
    if density is not None:
        dec.set_density(density)
    HG.reload(z, dec, prompts)
    return dec


def violation(z, seq, lp, word, cut=None):
    """density_violation of a decoded sequence under `word`; a token was DRAWN where its log-probability pair is a number."""
    start = 1 + len(z["encoded_meta"]) if cut is None else cut
    drawn = [not np.isnan(x) for x in np.asarray(lp)[:len(seq), 0]]
    return DC.density_violation(seq, start, word & 255, word >> 8, drawn)


def check_on_slot(z, seq, lp, word):
    from commu_amd.midi_generator.midi_inferrer import count_notes, note_order_violation, parse_events
    start = 1 + len(z["encoded_meta"])
    assert seq is not None and parse_events(seq, start) is None, seq
    assert note_order_violation(seq, start) is None and violation(z, seq, lp, word) is None, (word, seq)
    assert count_notes(seq) > 0


WORDS = (W(2, 4), -1, W(0, 1), -1)


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_alternating_slots_through_the_loop(fixture_model, parity, B):
    """Fails on the parent: ForcedDecoder has no set_density."""
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        plain = loaded(z, model, B)
        assert plain.density_ctl is None and plain.voice_ctl is None and plain.order_ctl is None and plain.cls_ctl is None
        s0, f0, l0 = run(plain)
        free, free_lp = plain.sequences()[0], plain.logprobs()
        words = [WORDS[b % 4] for b in range(B)]
        res = []
        for mode in ("graph", "eager", "separate"):
            dec = loaded(z, model, B, density=words)
            assert dec.state.parity == parity and dec.density_ctl.tolist() == words
            assert dec.voice_ctl.tolist() == [0 if w >= 0 else -1 for w in words]          # voice word 0 where the rule is
            assert dec.order_ctl.tolist() == [0 if w >= 0 else -1 for w in words]          # and the note order
            if mode == "separate":
                res.append(separate_launches(dec, dec.generation_length + 1))
            else:
                res.append(run(dec, use_graph=mode == "graph"))
            if mode == "graph":
                assert dec.graph is not None
                seqs, lps = dec.sequences()[0], dec.logprobs()
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert torch.equal(bits(res[0][2]), bits(other[2]))
        sg, fg, lg = res[0]
        for b in range(B):
            if words[b] >= 0:
                check_on_slot(z, seqs[b], lps[b], words[b])
            else:
                assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
        # teeth: the same request without the rule breaks the bounds, and the rule changed what the on-slots decoded
        broke = [(b, w) for b in range(B) for w in (W(2, 4), W(0, 1))
                 if free[b] is not None and violation(z, free[b], free_lp[b], w) is not None]
        print("without the rule: (slot, word) pairs that break the bounds:", broke)
        assert broke
        assert any(not torch.equal(sg[b], s0[b]) for b in range(B) if words[b] >= 0)
    finally:
        model.parity_fp32 = False


def test_a_primed_slot_whose_open_bar_is_full_draws_no_position(fixture_model):
    """The prompt's open bar holds two notes and the bound is two: greedy with one loud note, the grammar alone draws the loud
    position again; under the rule no position is DRAWN until a Bar stands behind the prompt."""
    z, model = fixture_model
    prompt = HG.PRIME + [440, 150, 63, dur(2)] + [444, 150, 64, dur(2)]
    n_ctx = 1 + len(z["encoded_meta"])
    for name, density in (("grammar", None), ("density", W(0, 2))):
        dec = loaded(z, model, 2, density=density, triple=(0.0, 32), bias=NG.loud_row(), max_prompt=len(prompt),
                     prompts=[prompt] * 2)
        run(dec)
        seq, lp = dec.sequences()[0][0], dec.logprobs()[0]
        cut = n_ctx + len(prompt)
        assert seq[:cut] == NG.z_ctx(z) + prompt and len(seq) > cut + 4, seq
        if density is None:
            assert not np.isnan(lp[cut, 0]) and 432 <= seq[cut] <= 559                      # a draw: a position
        else:
            bar = cut + seq[cut:].index(2) if 2 in seq[cut:] else len(seq)
            assert not any(432 <= seq[i] <= 559 and not np.isnan(lp[i, 0]) for i in range(cut, bar)), seq
            assert violation(z, seq, lp, W(0, 2), cut) is None


def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, density=[-1, W(2, 4), -1, -1])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g = dec.graph
    assert g is not None
    check_on_slot(z, dec.sequences()[0][1], dec.logprobs()[1], W(2, 4))
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_density(None, rows=[1])
    dec.set_voices(None, rows=[1])
    dec.set_note_order(None, rows=[1])
    dec.set_density(W(0, 1), rows=[2])
    uni = HG.reload(z, dec)
    dec.rearm(3, uni[3], density=W(3))
    s, f, l = run(dec)
    assert dec.graph is g and dec.density_ctl.tolist() == [-1, -1, W(0, 1), W(3)]
    assert dec.voice_ctl.tolist() == [-1, -1, 0, 0] and dec.order_ctl.tolist() == [-1, -1, 0, 0]
    second, lps = dec.sequences()[0], dec.logprobs()
    check_on_slot(z, second[2], lps[2], W(0, 1))
    check_on_slot(z, second[3], lps[3], W(3))
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], density=False)
    dec.set_density(None)
    dec.set_voices(None)
    dec.set_note_order(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.density_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


def test_fp8_sliding_cache_feeds_the_same_stage():
    import test_kv8_gpu as K8
    from commu_amd.generate import ForcedDecoder
    from commu_amd.midi_generator.midi_inferrer import count_notes, parse_events
    model, data = K8._loop_model(32)
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)
    words = [W(2, 4), W(0, 1), W(1), W(3, 3)]
    dec = ForcedDecoder(model, 4, generation_length=64, memory_length=32, temperature=0.95, top_k=32, sliding=True,
                        kv_dtype="fp8")
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_density(words)
    outs = []
    for graph in (False, True):
        dec.load([K8.META] * 4, [data] * 4, uni)
        with torch.no_grad():
            dec.run(use_graph=graph)
        torch.cuda.synchronize()
        outs.append(dec.sequences()[0])
    assert dec.state.kv_dtype == "fp8" and dec.graph is not None and outs[0] == outs[1]
    assert int(dec.state.klen.max()) >= 32                                # (the ring is full)
    start = 1 + len(K8.META)
    assert sum(count_notes(s) for s in outs[0] if s is not None) >= 4      # (notes were drawn: the rule had something to see)
    for s, lp, w in zip(outs[0], dec.logprobs(), words):
        assert s is not None and parse_events(s, start) is None, s
        drawn = [not np.isnan(x) for x in lp[:len(s), 0]]
        assert DC.density_violation(s, start, w & 255, w >> 8, drawn) is None, (w, s)


# ------------------------------------------------------------------------------------------------ 3. the request pool
@pytest.mark.parametrize("primed", [False, True], ids=["commu_decode_arm", "commu_decode_arm_primed"])
def test_pool_request_with_density_equals_generate_stream_of_that_request_alone(primed):
    """One request with density= (grammar and note order on; primed: its prompt cut from a sequence generated under the same
    controls) beside a request without it: its sequences equal generate_stream(slots=1, density=) of the request alone, and
    the neighbour's equal its own single-request run -- the arm launch wrote each slot's word."""
    import commu_amd.generate as G
    import pool_contract as PC
    import pool_prime_contract as PP
    import test_pool_gpu as TP
    import test_pool_prime_gpu as TPP
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model = TP._model()
    reqs = PC.four_requests(G)
    word = W(2, 4)
    every = lambda seq, rep: seq is not None
    kw = dict(grammar=True, note_order=True, density=word)
    mine = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, note_order=True, logit_bias=None,
                               density=word)
    if primed:
        own = TPP._own_sequence(TPP._generator(model), mine, 6, **kw)
        mine = dataclasses.replace(mine, prompt=PP.prompt_of(own, len(PC.META), 6))
    want = TPP._alone(TPP._generator(model), mine, **kw)
    other = dataclasses.replace(reqs[0], accept=every, grammar=False)
    other_want = TPP._alone(TPP._generator(model), other)
    gen = TPP._generator(model)
    res = gen.generate_pool([other, mine], slots=3, grammar=True, return_logprobs=True)
    TPP._same_results(res[1], want)
    assert res[0].sequences == other_want[0] and res[0].attempts_started == other_want[1]      # (token for token)
    assert gen.pool_stats["kernel"] == ("commu_decode_arm_primed" if primed else "commu_decode_arm")
    assert len(res[1].sequences) == 2
    cut = TPP.N_CTX + (6 if primed else 0)
    for s, lp in zip(res[1].sequences, res[1].logprobs):
        assert parse_events(s, TPP.N_CTX) is None, s
        drawn = [not np.isnan(x) for x in lp[:len(s), 0]]
        assert DC.density_violation(s, cut, 2, 4, drawn) is None, s
    # teeth: without density= the same request decodes something else
    free = TPP._alone(TPP._generator(model), dataclasses.replace(mine, density=None), grammar=True, note_order=True)
    assert free[0] != want[0]


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_cli_in_a_fresh_process(tmp_path):
    cli = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *a],
                                    capture_output=True, text=True, timeout=120)
    out = cli("--help")
    assert out.returncode == 0 and "--min_notes_per_bar" in out.stdout and "--max_notes_per_bar" in out.stdout
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt"),
              "--num_generate", "1"]
    # (two refusals through the process; the others are test_density_host.test_check_density_of_the_command_line's)
    out = cli(*common, "--max_notes_per_bar", "256")
    assert out.returncode != 0 and "--max_notes_per_bar: an integer in [1, 255] expected, got '256'" in out.stderr, out.stderr
    out = cli(*common, "--min_notes_per_bar", "3", "--max_notes_per_bar", "2")
    assert out.returncode != 0 and "not below --min_notes_per_bar expected, got 2 < 3" in out.stderr, out.stderr
    # accepted values get past the check: the run then stops at the checkpoint that is not there
    out = cli(*common, "--min_notes_per_bar", "2", "--max_notes_per_bar", "6", "--max_voices", "2")
    assert out.returncode != 0 and "notes_per_bar:" not in out.stderr, out.stderr
