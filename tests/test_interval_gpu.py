"""The melodic interval on the GPU.  The defining property: a draw under the rule is bit for bit the draw the density kernel
makes for the same inputs with bias[b] = -inf at the ids of tests/interval_contract.bans and the rule absent -- so the
sampler test needs no tolerance: the new kernel (commu_sample_args.interval_ctl) against the existing one, once and
compounding (Q5).  The rows come in two launches of 48 .. 96 rows each: the density test's rows under a cycle of interval
words, and the host test's edge cases with what only the kernel can get wrong.  Then through the decode loop: captured graph
== eager == separate launches, off-slots bit for bit a decoder that never heard of the feature, teeth, a primed slot,
in-place switching, the fp8 sliding cache, fp32 parity, the request pool with both arm launches and the command line."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import density_contract as DC  # noqa: E402
import interval_contract as IC  # noqa: E402
import test_density_gpu as DG  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_interval_host as IH  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_note_order_gpu as NG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
import test_voices_host as VH  # noqa: E402
import voices_contract as VC  # noqa: E402

DEV = "cuda"
V = 729
LD_SEQ = NG.LD_SEQ
NEG = float("-inf")
bits = SR.bits
CTX = VH.CTX
W, pos, dur, note = IC.word, VH.pos, VH.dur, IH.note
same_row = NG.same_row


def fill(n):
    """n tokens that hold no BAR and no complete note: Position, Chord pairs, and a Position, Velocity pair at the end (an
    incomplete group behind the last note; under the grammar the draw that follows is a pitch)."""
    assert n >= 2
    return ([pos(8), 200] * n)[:n - 2] + [pos(8), 150]


# ------------------------------------------------------------------------------------------------ 1. the sampler
def density_cases():
    """(name, tokens, F_LEN or None, density, note-order, voice, interval word): the density test's rows under a cycle of
    interval words that includes -1 and 0."""
    cycle = [W(7, 7), W(1, 1, True), -1, W(0, 0, True), 0, W(2), W(0, 3), W(12, 12, True)]
    return [(n, t, ln, d, o, v, cycle[i % len(cycle)]) for i, (n, t, ln, d, o, v) in enumerate(DG.kernel_cases())]


def kernel_cases():
    """The host test's edge cases (the other three words off: the rule implies none of them), then what only the kernel can
    get wrong."""
    cases = [(n, t, ln, -1, -1, -1, c) for n, t, ln, c, _ in IH.EDGE_CASES]
    old = note(0, 100)                      # (a note further back: the wrong reference)
    # the reference note's DURATION in lane 63 of chunk 0 (its PITCH in lane 0 of chunk 1: the note straddles the seam), in
    # lane 0 and in lane 1 of chunk 1
    for k in (64, 65, 66):
        t = CTX + [2] + old + note(4, 40) + fill(k - 1)
        assert t[-k] == dur(4) and t[-k - 1] == 40
        cases += [("duration_at_L_minus_%d" % k, t, None, -1, -1, -1, W(2, 3, True)),
                  ("duration_at_L_minus_%d_unison_only" % k, t, None, -1, -1, -1, W(0, 0, True))]
    # the reference note in chunk 2, about 130 filler tokens behind it; once more with a BAR in the filler (beta 1), and with
    # two (beta 2: no reference)
    t = CTX + [2] + old + note(4, 40) + fill(130)
    assert t[-131] == dur(4)
    cases += [("reference_in_chunk_2", t, None, -1, -1, -1, W(2, 3, True))]
    t1 = CTX + [2] + old + note(4, 40) + fill(70) + [2] + fill(59)
    t2 = CTX + [2] + old + note(4, 40) + fill(40) + [2] + fill(40) + [2] + fill(48)
    cases += [("reference_in_chunk_2_beta_1", t1, None, -1, -1, -1, W(2, 3, True)),
              ("no_reference_in_chunk_2_beta_2", t2, None, -1, -1, -1, W(2, 3, True))]
    # a BAR in lane 0 of chunk 1 (index L - 65) between two notes: the note behind it has beta 1 with no BAR in chunk 0 and
    # beta 2 with one there -- the carried count decides; and the note in front of it is the reference when there is one
    a = CTX + [2] + note(4, 40) + [2] + fill(64)
    b = CTX + [2] + note(4, 40) + [2] + fill(30) + [2] + fill(33)
    c = CTX + [2] + note(4, 40) + [2] + note(0, 90) + fill(60)
    assert a[-65] == 2 and b[-65] == 2 and c[-65] == 2 and 2 not in a[-64:] and b[-64:].count(2) == 1
    cases += [("bar_in_lane_0_of_chunk_1_beta_1", a, None, -1, -1, -1, W(2, 3, True)),
              ("bar_in_lane_0_of_chunk_1_beta_2", b, None, -1, -1, -1, W(2, 3, True)),
              ("bar_in_lane_0_of_chunk_1_note_in_front", c, None, -1, -1, -1, W(2, 3, True))]
    # the range ends on lane seams (a lane owns 12 ids): q + up + 1 and q - down at multiples of 12, and one id to either side
    for q, up, down in ((60, 11, 12), (65, 6, 5), (60, 10, 11), (60, 12, 13), (11, 12, 8), (119, 0, 11)):
        cases.append(("seam_q%d_up%d_down%d" % (q, up, down), CTX + [2] + note(0, q) + [pos(8), 150], None, -1, -1, -1,
                      W(up, down)))
    # unison with q the first and the last id of a lane
    for q in (60, 71, 12, 130 - 130 % 12 - 1):
        cases.append(("unison_q%d" % q, CTX + [2] + note(0, q) + [pos(8), 150], None, -1, -1, -1, W(0, 0, True)))
    # all three bans at once, with the note order, the voice cap and the density on in the same row
    busy = CTX + [2] + note(0, 70, 64) + note(8, 61, 2) + [pos(16), 150]
    cases += [("all_three_with_order_voices_density", busy, None, DC.word(1, 4), 0, VC.word(2, True), W(4, 5, True)),
              ("all_three_with_order_cap_and_full_bar", busy, None, DC.word(0, 2), 1, VC.word(1), W(1, 1, True))]
    # a bias that leaves only a banned pitch: nothing is left (row NOTHING below)
    cases += [("only_a_banned_pitch_left", CTX + [2] + note(0, 60) + [pos(8), 150], None, -1, -1, -1, W(7, 7))]
    return cases


NOTHING_PITCH = 72            # (60 + 7 < 72: banned in row only_a_banned_pitch_left; a tone of the rows' chord, so that the
#                               harmony table of the rows that have it on leaves it to the launch without the rule)


def build(cases):
    """test_density_gpu.rows for rows with an interval word: the 64 rows of the sampling test tiled, the words, the bans of
    the density rule and of the interval rule, and a bias that makes what each rule takes away the likely token."""
    from commu_amd._lib import call
    from commu_amd.generate import CLASS_CTL_DTYPE, event_grammar, harmony_table
    n = len(cases)
    assert 48 <= n <= 96, n
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    pick = torch.arange(n) % logits.shape[0]
    logits, wrong, us, t, k, p = logits[pick], wrong[pick], us[pick], t[pick], k[pick], p[pick]
    assert bool((t == 0).any()) and bool((t != 0).any())                  # greedy rows and sampled rows
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(n, nf, dtype=torch.int32)
    seq = torch.full((n, LD_SEQ), 310, dtype=torch.int32)                 # (behind the tokens: durations)
    dctl, octl, vctl, mctl = (torch.zeros(n, dtype=torch.int32) for _ in range(4))
    banned, den_banned = [], []
    bias = torch.zeros(n, 768)
    for b, (name, tokens, length, d, o, v, m) in enumerate(cases):
        assert len(tokens) <= LD_SEQ
        seq[b, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32)
        st[b, 0] = len(tokens) if length is None else length
        st[b, 10] = 1                                                     # F_CUR: one chord placed
        dctl[b], octl[b], vctl[b], mctl[b] = d, o, v, m
        den_banned.append(DC.bans(seq[b].tolist(), int(st[b, 0]), d, o, v))
        banned.append(IC.bans(seq[b].tolist(), int(st[b, 0]), m))
        bias[b, [i for i in (2, 559) if i in den_banned[-1]]] = 14.0       # (the density test's teeth, kept)
        # teeth: a pitch the rule takes away is the likely one -- the first above the window, else the first below, else q
        q = IC.reference_pitch(seq[b].tolist(), int(st[b, 0]))
        if banned[-1]:
            above = [i for i in banned[-1] if i > q]
            bias[b, above[0] if above else (banned[-1][-1] if banned[-1][-1] < q else q)] = 14.0
        if name == "only_bar_and_eos_left":                               # (the density test's row with nothing left)
            bias[b] = NEG
            bias[b, 1] = bias[b, 2] = 0.0
        if name == "only_a_banned_pitch_left":
            assert NOTHING_PITCH in banned[-1]
            bias[b] = NEG
            bias[b, NOTHING_PITCH] = 0.0
    rec = np.zeros((n, 8), dtype=CLASS_CTL_DTYPE)                         # no class controls: the base-triple table
    for b in range(n):
        rec[b, :] = (float(t[b]), int(k[b]), float(p[b]), 0)
    ct = torch.full((n, 4), 199, dtype=torch.int32)
    return dict(n=n, cases=cases, logits=logits, wrong=wrong, us=us, bias=bias, state=st, seq=seq, chord_tok=ct, ctl=octl,
                vctl=vctl, dctl=dctl, mctl=mctl, banned=banned, gram=torch.from_numpy(event_grammar()),
                gram_on=torch.tensor([b % 2 for b in range(n)], dtype=torch.uint8), harm=torch.from_numpy(harmony_table()),
                harm_on=torch.tensor([(b // 2) % 2 for b in range(n)], dtype=torch.uint8),
                cls=torch.from_numpy(rec.view(np.int32).reshape(n, 8, 4)))


@pytest.fixture(scope="module", params=["density_rows", "edge_and_kernel_rows"])
def rows(request):
    r = build(density_cases() if request.param == "density_rows" else kernel_cases())
    if request.param == "edge_and_kernel_rows":
        # the hand-written expectations of the host test hold for the padded rows too
        for i, (name, _, _, _, want) in enumerate(IH.EDGE_CASES):
            assert r["cases"][i][0] == name and r["banned"][i] == sorted(want), name
    return r


def launch(r, logits, interval="mctl", density="dctl", voices="vctl", order="ctl", bias=None):
    """test_density_gpu.launch with interval_ctl: one launch of commu_sample_topk on fresh device copies (token -7,
    probs_out -3.0, logp_out 7.0 before it), the class records given and the scalars poisoned.  interval / density / voices
    / order: the rows' words by name, None (a null pointer) or a tensor."""
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
    od, vd, dd, md = words(order), words(voices), words(density), words(interval)
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=n, V=V, wrong=ptr(h["wrong"]), ldw=V, uniforms=ptr(h["us"]),
        temperature=5.0, top_k=3, top_p=0.3, token=ptr(tok), probs_out=ptr(pr), ldp=V, logp_out=ptr(lp),
        bias=ptr(bd), ld_bias=bd.stride(0), gram=ptr(h["gram"]), ld_gram=h["gram"].stride(0), gram_on=ptr(h["gram_on"]),
        harm=ptr(h["harm"]), ld_harm=h["harm"].stride(0), harm_on=ptr(h["harm_on"]), state=ptr(h["state"]),
        seq=ptr(h["seq"]), ld_seq=LD_SEQ, chord_tok=ptr(h["chord_tok"]), ld_chord=4, cls_ctl=ptr(h["cls"]),
        order_ctl=ptr(od), voice_ctl=ptr(vd), density_ctl=ptr(dd), interval_ctl=ptr(md))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()


def banned_bias(r):
    out = r["bias"].clone()
    for b, ids in enumerate(r["banned"]):
        out[b, ids] = NEG
    return out


def test_sampler_equals_the_density_kernel_with_the_bans_in_the_bias(rows):
    """Fails on the parent: commu_sample_args has no interval_ctl."""
    r, n = rows, rows["n"]
    names = [c[0] for c in r["cases"]]
    got = launch(r, r["logits"])
    want = launch(r, r["logits"], interval=None, bias=banned_bias(r))
    free = launch(r, r["logits"], interval=None)
    for b in range(n):
        assert same_row(got, want, b), (names[b], int(got[1][b]), int(want[1][b]))
        for i in r["banned"][b]:
            assert float(got[2][b, i]) == 0.0 or int(got[1][b]) == -1, (names[b], i)
        if int(r["mctl"][b]) <= 0 or not r["banned"][b]:                 # off, word 0, or nothing banned: the density draw
            assert same_row(got, free, b), names[b]
    # teeth: the bias makes a banned pitch the likely one -- the launch without the rule draws differently on these rows
    differ = [names[b] for b in range(n) if int(got[1][b]) != int(free[1][b])]
    took = [names[b] for b in range(n) if int(free[1][b]) in r["banned"][b]]
    print("rows:", n, "; rows with a ban:", sum(bool(x) for x in r["banned"]), "; rows whose token differs from the launch "
          "without the rule:", len(differ), differ)
    assert len(differ) >= 12 and set(took) <= set(differ) and len(took) >= 12
    assert int((got[1] >= 1).sum()) >= n // 2
    if "only_a_banned_pitch_left" in names:
        nothing = names.index("only_a_banned_pitch_left")
        assert int(got[1][nothing]) == -1 and bool(torch.isnan(got[3][nothing]).all())
        assert bool(torch.isnan(got[2][nothing]).all()) and int(free[1][nothing]) == NOTHING_PITCH
        # the rows whose reference the carried BAR count decides, by name: banned with beta 1, free with beta 2
        for name, some in (("bar_in_lane_0_of_chunk_1_beta_1", True), ("bar_in_lane_0_of_chunk_1_beta_2", False),
                           ("reference_in_chunk_2_beta_1", True), ("no_reference_in_chunk_2_beta_2", False)):
            assert bool(r["banned"][names.index(name)]) == some, name
    # Q5: the same two launches again on the logits the first ones left -- the same bans on the compounded rows
    got2 = launch(r, got[0])
    want2 = launch(r, want[0], interval=None, bias=banned_bias(r))
    for b in range(n):
        assert same_row(got2, want2, b), names[b]
    assert not torch.equal(bits(got2[0]), bits(got[0]))                   # (the sampled rows were divided again)


def test_off_words_and_word_0_are_the_density_kernel_bit_for_bit(rows):
    r, n = rows, rows["n"]
    free = launch(r, r["logits"], interval=None)
    for word in (-1, 0):
        off = launch(r, r["logits"], interval=torch.full((n,), word, dtype=torch.int32))
        assert all(same_row(off, free, b) for b in range(n)), word


def test_entry_point_refusal_and_ops(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    r = rows
    with pytest.raises(CommuHipError, match="-22"):
        launch(r, r["logits"], density=None)                              # interval_ctl without density_ctl
    with pytest.raises(CommuHipError, match="-22"):
        launch(r, r["logits"], voices=None)                               # ... without what density_ctl requires
    d = lambda x: x.to(DEV)
    with pytest.raises(CommuHipError, match="interval: density= expected"):
        ops.sample_topk(d(r["logits"].clone()), 0.9, 32, uniforms=d(r["us"]), interval=d(r["mctl"]))
    with pytest.raises(CommuHipError, match="interval controls"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, uniforms=d(r["us"]), bias=d(r["bias"]),
                        class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])), note_order=d(r["ctl"]), voices=d(r["vctl"]),
                        density=d(r["dctl"]), interval=d(r["mctl"]).float())
    # ops.sample_topk(interval=) makes the same launch (it builds the all-off grammar and harmony itself)
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), uniforms=d(r["us"]), top_p=0.3, bias=d(r["bias"]),
                          class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])), note_order=d(r["ctl"]), voices=d(r["vctl"]),
                          density=d(r["dctl"]), interval=d(r["mctl"]))
    plain = dict(r, gram_on=torch.zeros_like(r["gram_on"]), harm_on=torch.zeros_like(r["harm_on"]))
    ref = launch(plain, r["logits"])
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 2. through the loop
GLEN = NG.GLEN
run, separate_launches = LBG.run, LBG.separate_launches
fixture_model = NG.fixture_model


def loaded(z, model, B, interval=None, **kw):
    """test_density_gpu.loaded (grammar on, log-probabilities recorded, the steering row) with set_interval's value."""
    from commu_amd.generate import ForcedDecoder
    prompts, glen, triple, bias = kw.pop("prompts", None), kw.pop("glen", GLEN), kw.pop("triple", (0.95, 32)), kw.pop("bias", None)
    dec = ForcedDecoder(model, B, glen, 4146, triple[0], triple[1], **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES) if bias is None else bias)
    if interval is not None:
        dec.set_interval(interval)
    HG.reload(z, dec, prompts)
    return dec


def violation(seq, lp, word, start):
    """interval_violation of a decoded sequence under `word`; a token was DRAWN where its log-probability pair is a number."""
    from commu_amd.midi_generator.midi_inferrer import interval_violation
    drawn = [not np.isnan(x) for x in np.asarray(lp)[:len(seq), 0]]
    return interval_violation(seq, start, word & 255, (word >> 8) & 255, bool(word >> 16), drawn)


def check_on_slot(z, seq, lp, word):
    from commu_amd.midi_generator.midi_inferrer import count_notes, parse_events
    start = 1 + len(z["encoded_meta"])
    assert seq is not None and parse_events(seq, start) is None, seq
    assert violation(seq, lp, word, start) is None, (word, seq)
    assert count_notes(seq) > 1


WORDS = (W(7, 7), -1, W(3, 3, True), -1)


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_alternating_slots_through_the_loop(fixture_model, parity, B):
    """Fails on the parent: ForcedDecoder has no set_interval."""
    z, model = fixture_model
    start = 1 + len(z["encoded_meta"])
    model.parity_fp32 = parity
    try:
        plain = loaded(z, model, B)
        assert plain.interval_ctl is None and plain.density_ctl is None and plain.order_ctl is None and plain.cls_ctl is None
        s0, f0, l0 = run(plain)
        free, free_lp = plain.sequences()[0], plain.logprobs()
        words = [WORDS[b % 4] for b in range(B)]
        res = []
        for mode in ("graph", "eager", "separate"):
            dec = loaded(z, model, B, interval=words)
            assert dec.state.parity == parity and dec.interval_ctl.tolist() == words
            # (the rule implies none of the others: their words exist for the one kernel and are off)
            assert dec.density_ctl.tolist() == [-1] * B and dec.voice_ctl.tolist() == [-1] * B
            assert dec.order_ctl.tolist() == [-1] * B
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
        # teeth: the same request without the rule leaps, and the rule changed what the on-slots decoded
        broke = [(b, w) for b in range(B) for w in (W(7, 7), W(3, 3, True))
                 if free[b] is not None and violation(free[b], free_lp[b], w, start) is not None]
        print("without the rule: (slot, word) pairs that break the cap:", broke)
        assert broke
        assert any(not torch.equal(sg[b], s0[b]) for b in range(B) if words[b] >= 0)
    finally:
        model.parity_fp32 = False


def test_a_primed_slot_takes_the_prompts_last_note_as_its_reference(fixture_model):
    """The prompt ends with a note of pitch 63 and the loud row makes 63 the likely pitch: greedy, the grammar alone draws 63
    again; under 2 / 2 / unison the first pitch DRAWN lies within two semitones of 63 and is not 63."""
    z, model = fixture_model
    prompt = HG.PRIME + [440, 150, 63, dur(2)]
    n_ctx = 1 + len(z["encoded_meta"])
    word = W(2, 2, True)
    for name, interval in (("grammar", None), ("interval", word)):
        dec = loaded(z, model, 2, interval=interval, triple=(0.0, 32), bias=NG.loud_row(), max_prompt=len(prompt),
                     prompts=[prompt] * 2)
        run(dec)
        seq, lp = dec.sequences()[0][0], dec.logprobs()[0]
        cut = n_ctx + len(prompt)
        assert seq[:cut] == NG.z_ctx(z) + prompt and len(seq) > cut + 4, seq
        first = next(i for i in range(cut, len(seq)) if 3 <= seq[i] <= 130 and not np.isnan(lp[i, 0]))
        assert 2 not in seq[cut:first]                                   # (the prompt's note is the note before it)
        if interval is None:
            assert seq[first] == 63
            assert violation(seq, lp, word, cut) == first
        else:
            assert seq[first] != 63 and abs(seq[first] - 63) <= 2, seq
            assert violation(seq, lp, word, cut) is None


def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, interval=[-1, W(7, 7), -1, -1])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g = dec.graph
    assert g is not None
    check_on_slot(z, dec.sequences()[0][1], dec.logprobs()[1], W(7, 7))
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_interval(None, rows=[1])
    dec.set_interval(W(0, 0, True), rows=[2])
    uni = HG.reload(z, dec)
    dec.rearm(3, uni[3], interval=W(3, 3))
    s, f, l = run(dec)
    assert dec.graph is g and dec.interval_ctl.tolist() == [-1, -1, W(0, 0, True), W(3, 3)]
    assert dec.density_ctl.tolist() == [-1] * 4 and dec.voice_ctl.tolist() == [-1] * 4 and dec.order_ctl.tolist() == [-1] * 4
    second, lps = dec.sequences()[0], dec.logprobs()
    check_on_slot(z, second[2], lps[2], W(0, 0, True))
    check_on_slot(z, second[3], lps[3], W(3, 3))
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], interval=False)
    dec.set_interval(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.interval_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


def test_fp8_sliding_cache_feeds_the_same_stage():
    import test_kv8_gpu as K8
    from commu_amd.generate import ForcedDecoder
    from commu_amd.midi_generator.midi_inferrer import count_notes, parse_events
    model, data = K8._loop_model(32)
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)
    words = [W(7, 7), W(0, 0, True), W(2), W(1, 1, True)]
    dec = ForcedDecoder(model, 4, generation_length=64, memory_length=32, temperature=0.95, top_k=32, sliding=True,
                        kv_dtype="fp8")
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_interval(words)
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
        assert violation(s, lp, w, start) is None, (w, s)


# ------------------------------------------------------------------------------------------------ 3. the request pool
@pytest.mark.parametrize("primed", [False, True], ids=["commu_decode_arm", "commu_decode_arm_primed"])
def test_pool_requests_with_their_own_words_equal_generate_stream_of_each_alone(primed):
    """Two requests with different interval words (one under the grammar, primed: its prompt cut from a sequence generated
    under the same controls; one without the grammar) and one without a word: each one's sequences equal
    generate_stream(slots=1) of the request alone -- the arm launch wrote each slot's word."""
    import commu_amd.generate as G
    import pool_contract as PC
    import pool_prime_contract as PP
    import test_pool_gpu as TP
    import test_pool_prime_gpu as TPP
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model = TP._model()
    reqs = PC.four_requests(G)
    w1, w2 = W(5, 5), W(2, 9, True)
    every = lambda seq, rep: seq is not None
    mine = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, logit_bias=None, interval=w1)
    if primed:
        own = TPP._own_sequence(TPP._generator(model), mine, 6, grammar=True, interval=w1)
        mine = dataclasses.replace(mine, prompt=PP.prompt_of(own, len(PC.META), 6))
    want = TPP._alone(TPP._generator(model), mine, grammar=True, interval=w1)
    second = dataclasses.replace(reqs[0], accept=every, grammar=False, interval=w2)
    second_want = TPP._alone(TPP._generator(model), second, interval=w2)
    third = dataclasses.replace(reqs[2], accept=every, grammar=False)
    third_want = TPP._alone(TPP._generator(model), third)
    gen = TPP._generator(model)
    res = gen.generate_pool([second, mine, third], slots=3, grammar=True, return_logprobs=True)
    TPP._same_results(res[1], want)
    TPP._same_results(res[0], second_want)
    assert res[2].sequences == third_want[0] and res[2].attempts_started == third_want[1]      # (token for token)
    assert gen.pool_stats["kernel"] == ("commu_decode_arm_primed" if primed else "commu_decode_arm")
    assert len(res[1].sequences) == 2
    cut = TPP.N_CTX + (6 if primed else 0)
    for s, lp in zip(res[1].sequences, res[1].logprobs):
        assert parse_events(s, TPP.N_CTX) is None, s
        assert violation(s, lp, w1, cut) is None, s
    for s, lp in zip(res[0].sequences, res[0].logprobs):
        assert violation(s, lp, w2, TPP.N_CTX) is None, s
    # teeth: without interval= the same request decodes something else
    free = TPP._alone(TPP._generator(model), dataclasses.replace(mine, interval=None), grammar=True)
    assert free[0] != want[0]


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_generate_cli_max_leap_end_to_end(golden_dir, tmp_path, monkeypatch):
    """generate.py --grammar --max_voices 1 --max_leap 7 on the reference-written checkpoint, every sequence that could be
    drawn accepted (a random model rarely passes the validators): no pitch of what it writes leaps more than 7 semitones
    from the note before it; the same run without the flag writes leaps."""
    import test_model_gpu as TM
    from commu_amd.midi_generator.midi_inferrer import (ForcingReport, InferenceTask, interval_violation, parse_events,
                                                         voices_violation)
    z = TM.load(golden_dir, "g10_checkpoint.npz")
    cli = TM._load_script("generate")
    parsers = cli.parse_args()
    prog = "-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8)
    common = ["--checkpoint_dir", os.path.join(golden_dir, "g10_checkpoint.pt"), "--generation_length", "120", "--gpus", "1",
              "--bpm", "70", "--audio_key", "aminor", "--time_signature", "4/4", "--pitch_range", "mid_high",
              "--num_measures", "8", "--inst", "acoustic_piano", "--genre", "newage", "--min_velocity", "60",
              "--max_velocity", "80", "--track_role", "main_melody", "--rhythm", "standard", "--chord_progression",
              prog + "-" + prog, "--num_generate", "2", "--max_rounds", "1", "--decode_slots", "2", "--grammar",
              "--max_voices", "1"]
    monkeypatch.setattr(ForcingReport, "validate_teacher_forced_sequence", lambda self, seq: None)
    monkeypatch.setattr(InferenceTask, "validate_generated_sequence", lambda self, seq: True)

    def run(argv, out):
        argv = common + ["--output_dir", str(tmp_path / out)] + argv
        margs, _ = parsers["model_args"].parse_known_args(argv)
        iargs, _ = parsers["input_args"].parse_known_args(argv)
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
        return json.load(open(tmp_path / out / "sequences.json"))

    got = run(["--max_leap", "7"], "leap")
    free = run([], "free")
    start = 1 + len(got["encoded_meta"])
    assert len(got["sequences"]) >= 1 and len(free["sequences"]) >= 1
    for s in got["sequences"]:
        assert parse_events(s, start) is None and voices_violation(s, start, 1, False) is None, s
        assert sum(1 for t in s[start:] if 3 <= t <= 130) >= 4 and interval_violation(s, start, 7, 7) is None, s
    assert any(interval_violation(s, start, 7, 7) is not None for s in free["sequences"])
