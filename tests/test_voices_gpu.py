"""The voice cap on the GPU.  The defining property: a draw under the rule is bit for bit the draw the note-order kernel makes
for the same inputs with bias[b] = -inf at the ids of tests/voices_contract.bans and the rule absent -- so the sampler test
needs no tolerance: the new kernel (commu_sample_args.voice_ctl) against the existing one, once and compounding (Q5).  Then
through the decode loop: captured graph == eager == separate launches, off-slots bit for bit a decoder that never heard of
the feature, teeth, a primed slot, in-place switching, the fp8 sliding cache, fp32 parity and the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import note_order_contract as NO  # noqa: E402
import test_decode_gpu as TD  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_note_order_gpu as NG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
import test_voices_host as VH  # noqa: E402
import voices_contract as VC  # noqa: E402

DEV = "cuda"
V = 729
LD_SEQ = NG.LD_SEQ
NEG = float("-inf")
ROOT = NG.ROOT
bits = SR.bits
CTX = VH.CTX
W, pos, dur = VC.word, VH.pos, VH.dur
same_row = NG.same_row


# ------------------------------------------------------------------------------------------------ 1. the sampler
def fill(n):
    """n velocity tokens: no breaker, no pitch, no duration, and no note group with what stands around them."""
    return [150] * n


def kernel_cases():
    """(name, tokens, F_LEN or None, voice word, note-order word): the host test's edge cases, then what only the kernel
    can get wrong."""
    cases = [(n, t, ln, c, 0) for n, t, ln, c, _ in VH.EDGE_CASES]
    note = [pos(0), 150, 60, dur(100)]
    # a note whose four tokens straddle the chunk seam: its Duration at index L - 64 (lane 63 of chunk 0) .. L - 67
    for k in (64, 65, 66, 67):
        cases.append(("duration_at_L_minus_%d" % k, CTX + [2] + note + fill(k - 1), None, W(1, True), 0))
        assert cases[-1][1][-k] == dur(100)
    # the second BAR from the end at index L - 64 and L - 65: the walk ends there
    for k in (64, 65):
        t = CTX + [pos(127), 150, 70, dur(128), 2, pos(120), 150, 60, dur(16), 2] + fill(k - 6)
        assert t[-k] == 2 and t.count(2) == 2
        cases.append(("second_bar_at_L_minus_%d" % k, t, None, W(1, True), 0))
    # a BAR in chunk 0, the notes of the bar before it in chunk 2: beta is carried over two chunks
    far = CTX + [2, pos(100), 150, 60, dur(60), pos(110), 150, 62, dur(30)] + fill(130) + [2] + fill(10)
    assert len(far) - far.index(dur(60)) > 128 and far[::-1].index(2) < 64
    cases += [("beta_carried_over_two_chunks", far, None, W(1, True), 0),
              ("beta_carried_cap_2", far, None, W(2, True), 0),
              # (the note order's run ended in chunk 0: the pitches of chunk 2 are none of its business)
              ("beta_carried_no_restrike", far, None, W(1), 0)]
    # three chunks, no BAR at all: the walk ends at index 0, where the note's POSITION stands
    cases.append(("three_chunks_down_to_index_0", [pos(0), 150, 60, dur(128)] + fill(150) + [pos(4), 150], None, W(1, True), 0))
    body = [pos(0), 150, 60, dur(128)] + fill(61)
    cases += [("L_%d" % n, body[:n], None, W(1, True), 0) for n in (63, 64, 65)]
    # pitch ids around a lane boundary of 12 (lane 0 owns ids 0 .. 11, lane 1 ids 12 .. 23) and the last pitch
    chord = []
    for p in (11, 12, 13, 130):
        chord += [pos(0), 150, p, dur(10)]
    cases += [("pitches_11_12_13_130", CTX + [2] + chord + [pos(4), 150], None, W(0, True), -1),
              ("pitches_11_12_13_130_cap_4", CTX + [2] + chord + [pos(4), 150], None, W(4, True), 0),
              ("pitches_11_12_13_130_cap_5", CTX + [2] + chord + [pos(4), 150], None, W(5, True), 0)]
    # off words between on words whose sequences would ban something; the note order off under a voice word
    cases += [("off_between_a", CTX + VH.ONE, None, -1, 0), ("on_between", CTX + VH.ONE, None, W(1, True), 0),
              ("off_between_b", far, None, -1, 0), ("on_between_b", CTX + VH.ONE, None, W(1, True), -1),
              ("both_off", CTX + VH.ONE, None, -1, -1)]
    # bias + bans leave nothing (row NOTHING below): the bias allows pitch 60 and the positions before 440 only
    # (its note order is off: on, it bans the same ids and the launch without the rule has nothing left either)
    cases += [("nothing_left", CTX + [2, pos(0), 150, 60, dur(9), pos(8), 150], None, W(1, True), -1)]
    return cases


@pytest.fixture(scope="module")
def rows():
    from commu_amd._lib import call
    from commu_amd.generate import CLASS_CTL_DTYPE, event_grammar, harmony_table
    cases = kernel_cases()
    n = len(cases)
    assert 40 <= n <= 64
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    logits, wrong, us, t, k, p = logits[:n], wrong[:n], us[:n], t[:n], k[:n], p[:n]
    assert bool((t == 0).any()) and bool((t != 0).any())                  # greedy rows and sampled rows
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(n, nf, dtype=torch.int32)
    seq = torch.full((n, LD_SEQ), 310, dtype=torch.int32)                 # (behind the tokens: durations)
    ctl = torch.zeros(n, dtype=torch.int32)
    octl = torch.zeros(n, dtype=torch.int32)
    banned = []
    bias = torch.zeros(n, 768)
    for b, (name, tokens, length, c, o) in enumerate(cases):
        assert len(tokens) <= LD_SEQ
        seq[b, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32)
        st[b, 0] = len(tokens) if length is None else length
        st[b, 10] = 1                                                     # F_CUR: one chord placed
        ctl[b], octl[b] = c, o
        on = VC.bans(seq[b].tolist(), int(st[b, 0]), c if c >= 0 else W(1, True))      # what the row bans when it is on
        banned.append(VC.bans(seq[b].tolist(), int(st[b, 0]), c))
        # teeth: the ids the rule takes away are the likely ones -- the first banned pitch, the last banned position
        for ids in ([i for i in on if i <= 130][:1], [i for i in on if i >= 432][-1:]):
            bias[b, ids] = 14.0
        if name == "nothing_left":
            bias[b] = NEG
            bias[b, 60] = bias[b, 432:440] = 0.0
    # the hand-written expectations of the host test hold for the padded rows too
    for b, (_, _, _, _, want) in enumerate(VH.EDGE_CASES):
        assert banned[b] == sorted(want), cases[b][0]
    rec = np.zeros((n, 8), dtype=CLASS_CTL_DTYPE)                         # no class controls: the base-triple table
    for b in range(n):
        rec[b, :] = (float(t[b]), int(k[b]), float(p[b]), 0)
    ct = torch.full((n, 4), 199, dtype=torch.int32)
    return dict(n=n, cases=cases, logits=logits, wrong=wrong, us=us, bias=bias, state=st, seq=seq, chord_tok=ct, ctl=octl,
                vctl=ctl, banned=banned, gram=torch.from_numpy(event_grammar()),
                gram_on=torch.tensor([b % 2 for b in range(n)], dtype=torch.uint8), harm=torch.from_numpy(harmony_table()),
                harm_on=torch.tensor([(b // 2) % 2 for b in range(n)], dtype=torch.uint8),
                cls=torch.from_numpy(rec.view(np.int32).reshape(n, 8, 4)))


def launch(r, logits, voices="vctl", order="ctl", bias=None):
    """One launch of commu_sample_topk on fresh device copies (token -7, probs_out -3.0, logp_out 7.0 before it), the
    class records given and the scalars poisoned.  voices / order: the rows' words by name, None (a null pointer) or a
    tensor."""
    from commu_amd._lib import SampleArgs, call, struct_args
    n = r["n"]
    d = lambda x: x.to(DEV).contiguous()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    lg = logits.clone().to(DEV)
    pr = torch.full((n, V), -3.0, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n, 2), 7.0, device=DEV)
    h = {k: d(r[k]) for k in ("wrong", "us", "gram", "gram_on", "harm", "harm_on", "state", "seq", "chord_tok", "cls")}
    bd = d(r["bias"] if bias is None else bias)
    od = None if order is None else d(r[order] if isinstance(order, str) else order)
    vd = None if voices is None else d(r[voices] if isinstance(voices, str) else voices)
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=n, V=V, wrong=ptr(h["wrong"]), ldw=V, uniforms=ptr(h["us"]),
        temperature=5.0, top_k=3, top_p=0.3, token=ptr(tok), probs_out=ptr(pr), ldp=V, logp_out=ptr(lp),
        bias=ptr(bd), ld_bias=bd.stride(0), gram=ptr(h["gram"]), ld_gram=h["gram"].stride(0), gram_on=ptr(h["gram_on"]),
        harm=ptr(h["harm"]), ld_harm=h["harm"].stride(0), harm_on=ptr(h["harm_on"]), state=ptr(h["state"]),
        seq=ptr(h["seq"]), ld_seq=LD_SEQ, chord_tok=ptr(h["chord_tok"]), ld_chord=4, cls_ctl=ptr(h["cls"]),
        order_ctl=ptr(od), voice_ctl=ptr(vd))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()


def banned_bias(r):
    out = r["bias"].clone()
    for b, ids in enumerate(r["banned"]):
        out[b, ids] = NEG
    return out


def test_sampler_equals_the_note_order_kernel_with_the_bans_in_the_bias(rows):
    """Fails on the parent: commu_sample_args has no voice_ctl."""
    r, n = rows, rows["n"]
    got = launch(r, r["logits"])
    want = launch(r, r["logits"], voices=None, bias=banned_bias(r))
    free = launch(r, r["logits"], voices=None)
    for b in range(n):
        assert same_row(got, want, b), (r["cases"][b][0], int(got[1][b]), int(want[1][b]))
        for i in r["banned"][b]:
            assert float(got[2][b, i]) == 0.0 or int(got[1][b]) == -1, (r["cases"][b][0], i)
        if int(r["vctl"][b]) < 0 or not r["banned"][b]:                  # off, or nothing banned: the note-order kernel's draw
            assert same_row(got, free, b), r["cases"][b][0]
    differ = [r["cases"][b][0] for b in range(n) if int(got[1][b]) != int(free[1][b])]
    print("rows whose token differs from the launch without the rule:", len(differ), differ)
    assert len(differ) >= 12
    nothing = [c[0] for c in r["cases"]].index("nothing_left")
    assert int(got[1][nothing]) == -1 and bool(torch.isnan(got[3][nothing]).all()) and bool(torch.isnan(got[2][nothing]).all())
    assert int(free[1][nothing]) >= 1
    assert int((got[1] >= 1).sum()) >= n // 2
    # Q5: the same two launches again on the logits the first ones left -- the same bans on the compounded rows
    got2 = launch(r, got[0])
    want2 = launch(r, want[0], voices=None, bias=banned_bias(r))
    for b in range(n):
        assert same_row(got2, want2, b), r["cases"][b][0]
    assert not torch.equal(bits(got2[0]), bits(got[0]))                   # (the sampled rows were divided again)
    # every word off: the note-order kernel bit for bit
    off = launch(r, r["logits"], voices=torch.full((n,), -1, dtype=torch.int32))
    assert all(same_row(off, free, b) for b in range(n))


def test_entry_point_refusal_and_ops(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    r = rows
    with pytest.raises(CommuHipError, match="-22"):
        launch(r, r["logits"], order=None)                                # voice_ctl without order_ctl
    d = lambda x: x.to(DEV)
    with pytest.raises(CommuHipError, match="voices: note_order= expected"):
        ops.sample_topk(d(r["logits"].clone()), 0.9, 32, uniforms=d(r["us"]), voices=d(r["vctl"]))
    with pytest.raises(CommuHipError, match="voices controls"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, uniforms=d(r["us"]), bias=d(r["bias"]),
                        class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])), note_order=d(r["ctl"]),
                        voices=d(r["vctl"]).float())
    # ops.sample_topk(voices=) makes the same launch (it builds the all-off grammar and harmony itself)
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), uniforms=d(r["us"]), top_p=0.3, bias=d(r["bias"]),
                          class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])), note_order=d(r["ctl"]), voices=d(r["vctl"]))
    plain = dict(r, gram_on=torch.zeros_like(r["gram_on"]), harm_on=torch.zeros_like(r["harm_on"]))
    ref = launch(plain, r["logits"])
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 2. through the loop
GLEN = NG.GLEN
run, separate_launches = LBG.run, LBG.separate_launches
fixture_model = NG.fixture_model


def loaded(z, model, B, voices=None, **kw):
    """test_note_order_gpu.loaded (grammar on, log-probabilities recorded, the steering row) with set_voices' value."""
    from commu_amd.generate import ForcedDecoder
    prompts, glen, triple, bias = kw.pop("prompts", None), kw.pop("glen", GLEN), kw.pop("triple", (0.95, 32)), kw.pop("bias", None)
    order = kw.pop("order", None)
    dec = ForcedDecoder(model, B, glen, 4146, triple[0], triple[1], **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES) if bias is None else bias)
    if order is not None:
        dec.set_note_order(order)
    if voices is not None:
        dec.set_voices(voices)
    HG.reload(z, dec, prompts)
    return dec


def violation(z, seq, n=1, r=True):
    from commu_amd.midi_generator.midi_inferrer import voices_violation
    return voices_violation(seq, 1 + len(z["encoded_meta"]), n, r)


def check_on_slot(z, seq, word):
    from commu_amd.midi_generator.midi_inferrer import count_notes, max_sounding, note_order_violation, parse_events
    start = 1 + len(z["encoded_meta"])
    n, r = word & 255, bool(word >> 8)
    assert seq is not None and parse_events(seq, start) is None, seq
    assert note_order_violation(seq, start) is None and violation(z, seq, n, r) is None, (word, violation(z, seq, n, r), seq)
    most, struck = max_sounding(seq, 1920, start)
    assert (n == 0 or most <= n) and not (r and struck), (word, most, struck, seq)
    assert count_notes(seq) > 0


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_alternating_slots_through_the_loop(fixture_model, parity, B):
    """Fails on the parent: ForcedDecoder has no set_voices."""
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        plain = loaded(z, model, B)
        assert plain.voice_ctl is None and plain.order_ctl is None and plain.cls_ctl is None
        s0, f0, l0 = run(plain)
        free = plain.sequences()[0]
        words = [(W(1, True), -1, W(2), -1)[b % 4] for b in range(B)]
        res = []
        for mode in ("graph", "eager", "separate"):
            dec = loaded(z, model, B, voices=words)
            assert dec.state.parity == parity and dec.voice_ctl.tolist() == words
            assert dec.order_ctl.tolist() == [0 if w >= 0 else -1 for w in words]          # note order on where the rule is
            if mode == "separate":
                res.append(separate_launches(dec, dec.generation_length + 1))
            else:
                res.append(run(dec, use_graph=mode == "graph"))
            if mode == "graph":
                assert dec.graph is not None
                seqs = dec.sequences()[0]
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert torch.equal(bits(res[0][2]), bits(other[2]))
        sg, fg, lg = res[0]
        for b in range(B):
            if words[b] >= 0:
                check_on_slot(z, seqs[b], words[b])
            else:
                assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
        # teeth: the same request under the note order alone breaks the rule, and the rule changed what the on-slots decoded
        ordered = loaded(z, model, B, order=True)
        run(ordered)
        assert any(s is not None and violation(z, s) is not None for s in ordered.sequences()[0])
        assert any(s is not None and violation(z, s) is not None for s in free)
        assert any(not torch.equal(sg[b], s0[b]) for b in range(B) if words[b] >= 0)
    finally:
        model.parity_fp32 = False


def test_a_primed_slot_sees_the_long_note_of_its_prompt(fixture_model):
    """The prompt holds one note that sounds over the whole bar: greedy with one loud note, the grammar alone strikes the
    same pitch on the same onset again; under the rule every position of the bar and the pitch are gone."""
    z, model = fixture_model
    prompt = HG.PRIME + [440, 150, 63, dur(120)]
    n_ctx = 1 + len(z["encoded_meta"])
    from commu_amd.midi_generator.midi_inferrer import voices_violation
    broke = {}
    for name, voices in (("grammar", None), ("voices", W(1, True))):
        dec = loaded(z, model, 2, voices=voices, triple=(0.0, 32), bias=NG.loud_row(), max_prompt=len(prompt),
                     prompts=[prompt] * 2)
        run(dec)
        seq, lp = dec.sequences()[0][0], dec.logprobs()[0]
        cut = n_ctx + len(prompt)
        assert seq[:cut] == NG.z_ctx(z) + prompt and len(seq) > cut + 8
        broke[name] = voices_violation(seq, cut, 1, True)
        if voices is None:
            assert not np.isnan(lp[cut, 0]) and seq[cut] == 440                            # a draw: the loud position again
        else:
            assert not 432 <= seq[cut] <= 559 or np.isnan(lp[cut, 0])                       # no position is DRAWN in this bar
    assert broke["grammar"] == n_ctx + len(prompt) and broke["voices"] is None, broke


def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, voices=[-1, W(1, True), -1, -1])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g = dec.graph
    assert g is not None
    check_on_slot(z, dec.sequences()[0][1], W(1, True))
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_voices(None, rows=[1])
    dec.set_note_order(None, rows=[1])
    dec.set_voices(W(2, True), rows=[2])
    uni = HG.reload(z, dec)
    dec.rearm(3, uni[3], voices=W(1))
    s, f, l = run(dec)
    assert dec.graph is g and dec.voice_ctl.tolist() == [-1, -1, W(2, True), W(1)] and dec.order_ctl.tolist() == [-1, -1, 0, 0]
    second = dec.sequences()[0]
    check_on_slot(z, second[2], W(2, True))
    check_on_slot(z, second[3], W(1))
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], voices=False)
    dec.set_voices(None)
    dec.set_note_order(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.voice_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


def test_requests_switch_the_rule_on_and_off(fixture_model):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    meta, data = z["encoded_meta"].tolist(), TD._data(z, "sample8m")
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN)
    kw = dict(need=8, accept=lambda s, r: True, logit_bias=HG.steer_row(HG.NOTES), grammar=True)
    out = gen.generate_stream(meta, data, 0.95, 32, slots=8, voices=W(1, True), **kw)[0]
    assert len(out) == 8 and all(s is not None and violation(z, s) is None for s in out)
    # a request without voices= switches off what the one before left on the reused decoder
    after = gen.generate_stream(meta, data, 0.95, 32, slots=8, **kw)[0]
    fresh = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN).generate_stream(meta, data, 0.95, 32,
                                                                                             slots=8, **kw)[0]
    assert after == fresh and after != out and any(violation(z, s) is not None for s in after)
    with pytest.raises(CommuHipError, match=r"voices: .*got 129"):
        gen.generate_stream(meta, data, 0.95, 32, slots=8, voices=129, **kw)


def test_fp8_sliding_cache_feeds_the_same_stage():
    import test_kv8_gpu as K8
    from commu_amd.generate import ForcedDecoder
    from commu_amd.midi_generator.midi_inferrer import count_notes, parse_events, voices_violation
    model, data = K8._loop_model(32)
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)
    words = [W(1, True), W(2, True), W(1), W(0, True)]
    dec = ForcedDecoder(model, 4, generation_length=64, memory_length=32, temperature=0.95, top_k=32, sliding=True,
                        kv_dtype="fp8")
    dec.set_grammar(True)
    dec.set_voices(words)
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
    for s, w in zip(outs[0], words):
        assert s is not None and parse_events(s, start) is None, s
        assert voices_violation(s, start, w & 255, bool(w >> 8)) is None, (w, s)


# ------------------------------------------------------------------------------------------------ 3. CLI
def test_cli_in_a_fresh_process(tmp_path):
    cli = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *a],
                                    capture_output=True, text=True, timeout=120)
    out = cli("--help")
    assert out.returncode == 0 and "--max_voices" in out.stdout and "--no_restrike" in out.stdout
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt"),
              "--num_generate", "1"]
    # (one refusal through the process; the others are test_voices_host.test_check_voices_of_the_command_line's)
    out = cli(*common, "--max_voices", "129", "--no_restrike")
    assert out.returncode != 0 and "--max_voices: an integer in [1, 128] expected, got '129'" in out.stderr, out.stderr
    # accepted values get past the check: the run then stops at the checkpoint that is not there
    out = cli(*common, "--max_voices", "1", "--no_restrike")
    assert out.returncode != 0 and "--max_voices" not in out.stderr, out.stderr
