"""The harmony constraint on the GPU: the sampling kernel with a harmony table (commu_sample_args.harm) against the
numpy restatement (harmony_contract.restate_with_harmony: ((x + bias) + gram[c]) + harm[r][(id - 3) mod 12] at the pitch
ids, r from the last chord of seq) and against the launch without one, bit for bit; then through the decode loop
(fused launch, captured graph, fp32 parity), a mid-bar chord change, primed slots, in-place switching, the single-request
API, the fp8 sliding cache and the CLI."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grammar_contract as GC  # noqa: E402
import harmony_contract as HC  # noqa: E402
import test_decode_gpu as TD  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
from sample_launch import sample_launch  # noqa: E402

DEV = "cuda"
V = 729
NEG = float("-inf")
LOGP_TOL = SR.LOGP_TOL          # (the grammar test's: the restatement is fed y as fp32 rounds it, the third add brings no new error)
bits = SR.bits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
# the 24 kernel rows: sampling triple b % 3 (greedy | temperature 0.95, top_k 32 | top_p 0.9), chord case (b // 3) % 5
TRIPLES = [(0.0, 32, 1.0), (0.95, 32, 1.0), (0.95, 32, 0.9)]
CASES = ["row0", "row107", "nn", "none", "off"]
CHORD_OF = {"row0": 195, "row107": 302, "nn": 303}
EDGE_IDS = [2, 3, 14, 15, 130, 131]
TOP32 = [16, 19]                # top_k 32 rows under chord rows 0 / 107 whose 32 most likely ids the chord bans
# previous token of row b (the grammar's key): mostly a velocity, after which the grammar admits pitches only
PREV = [140 if b % 4 else (432, 2, 310, 60, 559, 600)[b // 4] for b in range(N)]


def case_of(b):
    return CASES[(b // 3) % 5]


def records():
    """Forcing records, seq rows and chord rows of the 24 kernel rows, consistent the way the loop keeps them: the chords
    placed so far are chord_tok[b][:F_CUR] and stand in seq in that order; the next, pending chord chord_tok[b][F_CUR]
    and a chord behind the end of seq are decoys.  Returns (state, seq, chord_tok, the token lists)."""
    from commu_amd._lib import call
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(N, nf, dtype=torch.int32)
    seq = torch.full((N, 24), 600, dtype=torch.int32)
    ct = torch.full((N, 6), 250, dtype=torch.int32)
    toks = []
    for b in range(N):
        case = case_of(b)
        placed = [] if case in ("none",) else ([230 + b, CHORD_OF[case]] if case != "off" else [230 + b, 260])
        ct[b, :len(placed)] = torch.tensor(placed, dtype=torch.int32) if placed else ct[b, :0]
        ct[b, len(placed)] = 215 + b                                    # the pending chord: not the row's
        body = [600, 2, 432]
        for c in placed:
            body += [c, 440 + b, 150, 60, 310, 2, 432][:3 + (b % 3) * 2]
        body = body[:20] + [PREV[b]]
        for i, t in enumerate(body):
            seq[b, i] = t
        seq[b, len(body)] = 222                                         # a chord behind the end of seq: not the row's
        st[b, 0] = len(body)
        st[b, 10] = len(placed)                                         # F_CUR
        toks.append(body)
    return st, seq, ct, toks


@pytest.fixture(scope="module")
def rows():
    from commu_amd.generate import harmony_table
    g = torch.Generator().manual_seed(41)
    logits = torch.randn(N, V, generator=g) * 2.5
    logits[:, EDGE_IDS] += 15.0                                         # the edge ids carry mass wherever they are allowed
    strict = harmony_table()
    for b in TOP32:                                                     # the 32 most likely ids are pitches outside the chord
        assert b % 3 == 1 and case_of(b) in ("row0", "row107")
        pcs = HC.pitch_classes(CHORD_OF[case_of(b)])
        out = [i for i in range(20, 120) if (i - 3) % 12 not in pcs][:32]
        logits[b, out] += 20.0
    us = torch.rand(N, generator=g)
    t = torch.tensor([TRIPLES[b % 3][0] for b in range(N)], dtype=torch.float32)
    k = torch.tensor([TRIPLES[b % 3][1] for b in range(N)], dtype=torch.int32)
    p = torch.tensor([TRIPLES[b % 3][2] for b in range(N)], dtype=torch.float32)
    wrong = torch.zeros(N, V, dtype=torch.uint8)
    wrong[::5, 64] = 1
    bias, _ = LBG.bias_rows(logits)
    st, seq, ct, toks = records()
    on = torch.tensor([0 if case_of(b) == "off" else 1 for b in range(N)], dtype=torch.uint8)
    for b in range(N):                                                  # the records say what the definition on seq says
        want = {"row0": 0, "row107": 107, "nn": 108, "none": 109, "off": 110}[case_of(b)]
        assert HC.chord_row(toks[b], bool(on[b])) == want, b
    return dict(logits=logits, wrong=wrong, us=us, t=t, k=k, p=p, bias=bias[:N].contiguous(), state=st, seq=seq, chord_tok=ct,
                toks=toks, on=on, strict=torch.from_numpy(strict))


def launch(r, bias=None, gram=None, gram_on=None, harm=None, harm_on=None, wrong=None, ld_harm=None, state=True,
           chords=True, ld_chord=None):
    """One launch on fresh device copies of the 24 rows (sample_launch); state=False / chords=False: a null record /
    chord_tok pointer (the row stride of chord_tok is still passed)."""
    return sample_launch(r["logits"], r["wrong"] if wrong is None else wrong, r["us"], r["t"], r["k"], r["p"], bias=bias,
                         gram=gram, gram_on=gram_on, harm=harm, ld_harm=ld_harm, harm_on=harm_on,
                         state=r["state"] if state else None, seq=r["seq"], chord_tok=r["chord_tok"] if chords else None,
                         ld_chord=r["chord_tok"].stride(0) if ld_chord is None else ld_chord)


def zero_bias():
    return torch.zeros(N, 768)


def off_grammar():
    return torch.zeros(8, 768), torch.zeros(N, dtype=torch.uint8)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check(r, out, bias, gram, harm, harm_on, wrong=None):
    """Every row against the restatement: the logits written back bit for bit, the token, probs_out (exact zeros at the
    banned ids, the grammar test's tolerance elsewhere), full and kept."""
    lg, tok, pr, lp = out
    worst = [0.0, 0.0, 0.0]
    refs = []
    for b in range(N):
        res = HC.restate_with_harmony(r["logits"][b].numpy(), float(r["t"][b]), int(r["k"][b]), float(r["p"][b]),
                                      (r["wrong"] if wrong is None else wrong)[b].numpy(),
                                      None if bias is None else bias[b].numpy(), float(r["us"][b]),
                                      gram=None if gram is None else np.asarray(gram, dtype=np.float32), prev=PREV[b],
                                      harm=np.asarray(harm, dtype=np.float32), tokens=r["toks"][b], harm_on=bool(harm_on[b]))
        refs.append(res)
        assert np.array_equal(lg[b].numpy().view(np.int32), res.written[:V].view(np.int32)), b
        if res.token < 0:
            assert int(tok[b]) == -1 and bool(torch.isnan(lp[b]).all()) and bool(torch.isnan(pr[b]).all()), b
            continue
        got = pr[b].double().numpy()
        tb = int(tok[b])
        assert ((got > 0) == (res.probs > 0)).all(), b
        assert bool((got[res.y == NEG] == 0.0).all()), b                 # banned ids: exactly 0
        assert tb == res.token or abs(np.cumsum(res.probs)[min(tb, res.token)] - float(r["us"][b])) < 1e-5, b
        assert res.probs[tb] > 0, b
        worst[0] = max(worst[0], np.abs(got - res.probs).max())
        worst[1] = max(worst[1], abs(float(lp[b, 0]) - res.full[tb]))
        worst[2] = max(worst[2], abs(float(lp[b, 1]) - (0.0 if float(r["t"][b]) == 0 else np.log(res.probs[tb]))))
    print("max |probs - float64|, |full - float64|, |kept - log p|:", worst)
    assert max(worst) <= LOGP_TOL, worst
    return refs


def edge_table():
    """Strict on chosen classes: row 0 bans classes 0 and 7 (ids 3, 15, 130) and keeps 11 (id 14), row 107 the other way
    round; every other chord row bans class 5.  Rows 108 .. 110 zeros."""
    t = np.zeros((111, 16), np.float32)
    t[:108, 5] = NEG
    t[0, :12] = 0
    t[0, [0, 7]] = NEG
    t[107, :12] = 0
    t[107, 11] = NEG
    return t


def flat_table(v=-5.0):
    t = np.full((111, 16), v, np.float32)
    t[110] = 0
    t[:, 12:] = 0
    return t


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_separate_sampler_against_the_restatement(rows):
    from commu_amd.generate import event_grammar
    default = torch.from_numpy(event_grammar())
    zg, zon = off_grammar()
    free = launch(rows, chords=False)
    strict = rows["strict"]
    for bias, gram in ((None, None), (rows["bias"], None), (None, default), (rows["bias"], default)):
        kw = dict(bias=zero_bias() if bias is None else bias, gram=zg if gram is None else gram,
                  gram_on=zon if gram is None else None)
        for table in (strict, edge_table(), flat_table()):
            out = launch(rows, harm=table, harm_on=rows["on"], **kw)
            refs = check(rows, out, bias, gram, table, rows["on"])
            assert torch.equal(bits(out[0]), bits(free[0]))              # the written-back logits: the unconstrained call's
            assert sum(1 for x in refs if x.token >= 0) >= 12
            if table is strict:
                for b in range(N):
                    c = CHORD_OF.get(case_of(b))
                    if int(out[1][b]) >= 0 and c in (195, 302) and 3 <= int(out[1][b]) <= 130:
                        assert (int(out[1][b]) - 3) % 12 in HC.pitch_classes(c), b
    # the edge ids on both sides of a ban (no bias, no grammar: every id may carry mass)
    out = launch(rows, bias=zero_bias(), gram=zg, gram_on=zon, harm=edge_table(), harm_on=rows["on"])
    for b in range(N):
        pr = out[2][b]
        if int(out[1][b]) < 0:
            continue
        if case_of(b) == "row0":
            assert pr[3] == 0 and pr[15] == 0 and pr[130] == 0, b
        elif case_of(b) == "row107":
            assert pr[14] == 0, b
        if b % 3 == 1 and b not in TOP32:                                # top-k only, the six edge ids lead: all that may, do
            want = {"row0": [2, 14, 131], "row107": [2, 3, 15, 130, 131]}.get(case_of(b), EDGE_IDS)
            assert (pr[want] > 0).all(), b
    # ids 2 and 131 are untouched by a table whose every entry is -5: their ratio to each other is the free call's, their
    # ratio to a pitch id is e^5 times the free call's
    flat = launch(rows, bias=zero_bias(), gram=zg, gram_on=zon, harm=flat_table(), harm_on=rows["on"])
    fr = launch(rows, bias=zero_bias(), gram=zg, gram_on=zon, chords=False)
    checked = 0
    for b in range(N):
        a, f = flat[2][b].double(), fr[2][b].double()
        if b % 3 != 1 or case_of(b) == "off" or min(a[[2, 3, 130, 131]].min(), f[[2, 3, 130, 131]].min()) <= 0:
            continue
        checked += 1
        assert abs(float(a[2] / a[131]) / float(f[2] / f[131]) - 1) < 1e-5, b
        assert abs(float(a[2] / a[3]) / (float(f[2] / f[3]) * np.exp(5.0)) - 1) < 1e-4, b
        assert abs(float(a[131] / a[130]) / (float(f[131] / f[130]) * np.exp(5.0)) - 1) < 1e-4, b
    assert checked >= 3
    # top_k 32 with the 32 most likely ids banned by the chord: 32 survivors, all chord tones
    out = launch(rows, bias=zero_bias(), gram=zg, gram_on=zon, harm=strict, harm_on=rows["on"])
    seen = 0
    for b in TOP32:
        if case_of(b) in ("row0", "row107"):
            kept = np.flatnonzero(out[2][b].numpy() > 0)
            pcs = HC.pitch_classes(CHORD_OF[case_of(b)])
            assert len(kept) == 32 and all(not 3 <= i <= 130 or (i - 3) % 12 in pcs for i in kept), b
            seen += 1
    assert seen >= 2
    # one row with everything banned: after a velocity the grammar admits pitches only, and row 0 of this table bans all
    dead = edge_table()
    dead[0, :12] = NEG
    out = launch(rows, bias=zero_bias(), gram=default, harm=dead, harm_on=rows["on"])
    hit = [b for b in range(N) if case_of(b) == "row0" and PREV[b] == 140]
    assert hit
    for b in hit:
        assert int(out[1][b]) == -1 and bool(torch.isnan(out[3][b]).all()) and bool(torch.isnan(out[2][b]).all()), b
    check(rows, out, None, default, dead, rows["on"])


# ------------------------------------------------------------------------------------------------ 2. off
def test_off_slots_and_a_zero_table_are_the_gram_entry_point_bit_for_bit(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import event_grammar
    default = torch.from_numpy(event_grammar())
    all_off = torch.zeros(N, dtype=torch.uint8)
    for bias in (zero_bias(), rows["bias"]):
        old = launch(rows, bias=bias, gram=default, chords=False)
        assert same(old, launch(rows, bias=bias, gram=default, harm=rows["strict"], harm_on=all_off))
        assert same(old, launch(rows, bias=bias, gram=default, harm=np.zeros((111, 16), np.float32), harm_on=rows["on"]))
        assert same(old, launch(rows, bias=bias, gram=default, harm=None))          # (same kernel, given a chord_tok)
    assert same(launch(rows, chords=False), launch(rows, bias=zero_bias(), gram=off_grammar()[0], gram_on=off_grammar()[1],
                                             harm=rows["strict"], harm_on=all_off))
    assert int((old[1] >= 1).sum()) >= 12
    assert not same(old, launch(rows, bias=rows["bias"], gram=default, harm=rows["strict"], harm_on=rows["on"]))
    # refusals of the C entry point
    ok = dict(bias=zero_bias(), gram=default, harm=rows["strict"], harm_on=rows["on"])
    for kw in (dict(ld_harm=8), dict(state=False), dict(chords=False), dict(ld_chord=0)):
        with pytest.raises(CommuHipError, match="-22"):
            launch(rows, **ok, **kw)
    # ops.sample_topk(harmony=) is the same launch, and makes the zero bias / off grammar it needs
    d = lambda x: x.to(DEV)
    hargs = (d(rows["strict"]), d(rows["on"]), d(rows["state"]), d(rows["chord_tok"]))
    lg = d(rows["logits"].clone())
    tok = ops.sample_topk(lg, d(rows["t"]), d(rows["k"]), wrong=d(rows["wrong"]), uniforms=d(rows["us"]), top_p=d(rows["p"]),
                          harmony=hargs)
    assert torch.equal(tok.cpu(), launch(rows, bias=zero_bias(), gram=off_grammar()[0], gram_on=off_grammar()[1],
                                         harm=rows["strict"], harm_on=rows["on"])[1])
    lg = d(rows["logits"].clone())
    tok = ops.sample_topk(lg, d(rows["t"]), d(rows["k"]), wrong=d(rows["wrong"]), uniforms=d(rows["us"]), top_p=d(rows["p"]),
                          bias=d(rows["bias"]), grammar=(d(default), None, hargs[2], d(rows["seq"])), harmony=hargs)
    assert torch.equal(tok.cpu(), launch(rows, bias=rows["bias"], gram=default, harm=rows["strict"], harm_on=rows["on"])[1])
    with pytest.raises(CommuHipError, match="harmony table"):
        ops.sample_topk(lg, 0.95, 32, harmony=(rows["strict"],) + hargs[1:])


# ------------------------------------------------------------------------------------------------ 3. through the loop
GLEN = 64
# Every decoder of these tests (with and without harmony) runs the default grammar and a constraint row that keeps EOS
# away, so that no slot ends early.  The fixture model's own bias favours BAR (+3): under the grammar a slot spends half of
# its 64 iterations on bars, forced positions and forced chords and draws 7 to 13 pitches, some of them before its first
# chord (measured on a decoder without harmony: with the bar's logit lowered by 0 / 1 / 2 / 3 the slots drew 7 .. 13 / 11 ..
# 16 / 12 .. 16 / 15 .. 16 pitches, and 0 / 1 / 5 / 7 of 8 slots never saw a chord).  The tests that count pitches under a
# chord therefore start every slot right behind the first forced chord (PRIME: bar, position 0, the request's first
# chord -- what the rules themselves produce) and lower the bar by 2 (NOTES), so that nearly all iterations draw notes.
STEER = {"ban": [1], "bias": {}}
NOTES = {"ban": [1], "bias": {2: -2.0}}
PRIME = [2, 432, 199]


@pytest.fixture(scope="module")
def fixture_model(golden_dir):
    z = TD.load(golden_dir, "g6_decode.npz")
    return z, TD._build(golden_dir, z, z["sample8m_bias"])


def steer_row(steer=STEER):
    from commu_amd.generate import token_constraints
    return token_constraints(ban=steer["ban"], bias=steer["bias"])


def variates(B, n, seed=11):
    return np.random.RandomState(seed).random_sample((B, n)).astype(np.float32)


def loaded(z, model, B, on=None, table=True, tag="sample8m", max_prompt=0, prompts=None, glen=GLEN, steer=STEER, **kw):
    """B slots of a fixture's request, grammar on everywhere, log-probabilities recorded; on: None (a decoder that never
    heard of harmony) or the slots whose harmony is on."""
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, B, glen, 4146, 0.95, 32, max_prompt=max_prompt, **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(steer_row(steer))
    if on is not None:
        dec.set_harmony(table, rows=on)
    reload(z, dec, prompts, tag)
    return dec


def reload(z, dec, prompts=None, tag="sample8m"):
    uni = variates(dec.B, dec.ld_u)
    dec.load([z["encoded_meta"].tolist()] * dec.B, [TD._data(z, tag)] * dec.B, uni, prompts=prompts)
    return uni


run, draws = LBG.run, LBG.draws


def last_chord(seq):
    for t in reversed(seq):
        if 195 <= t <= 303:
            return t
    return None


def drawn_pitches(seq, drawn):
    """(index, pitch token, last chord before it) of every DRAWN pitch of a sequence."""
    return [(i, seq[i], last_chord(seq[:i])) for i in range(len(seq)) if drawn[i] and 3 <= seq[i] <= 130]


def out_of_chord(seq, drawn, table=None):
    """The drawn pitches outside their chord: by the chord's pitch classes (pitches before the first chord or under
    Chord_NN are never out), or by the bans of a table's row."""
    bad = []
    for i, t, c in drawn_pitches(seq, drawn):
        if table is None:
            if c is not None and c != 303 and (t - 3) % 12 not in HC.pitch_classes(c):
                bad.append(i)
        elif table[HC.chord_row(seq[:i]), (t - 3) % 12] == NEG:
            bad.append(i)
    return bad


def under_a_chord(seq, drawn):
    return [x for x in drawn_pitches(seq, drawn) if x[2] not in (None, 303)]


def check_loop(z, plain_out, plain_draws, out, dr, on, B):
    s0, f0, l0 = plain_out
    sg, fg, lg = out
    for b in range(B):
        seq, drawn = dr[b]
        assert seq is not None, b
        if b in on:
            assert out_of_chord(seq, drawn) == [], (b, seq)
            print("slot", b, "pitches drawn:", len(drawn_pitches(seq, drawn)), "under a chord:", len(under_a_chord(seq, drawn)),
                  "twin out of chord:", len(out_of_chord(*plain_draws[b])))
            assert len(under_a_chord(seq, drawn)) >= 10, b
            assert len(out_of_chord(*plain_draws[b])) >= 1, b           # the twin left its chord: the constraint bit
            chords = [t for t in seq if 195 <= t <= 303]
            assert chords == z["sample8m_chord_token"].tolist()[:len(chords)]          # forced tokens are not affected
        else:
            assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_alternating_slots_through_the_loop(fixture_model, parity, B):
    """Slots alternate on / off, grammar on everywhere, per-slot variates, every slot primed behind its first chord (PRIME,
    NOTES).  Graph replay == eager (seq, records, seq_logp
    bit patterns); every pitch an on-slot drew is a tone of the last chord before it; the off-slots decode bit for bit what
    a decoder that never heard of harmony decodes, and the on-slots' twins in that decoder leave their chords."""
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        kw = dict(steer=NOTES, max_prompt=len(PRIME), prompts=[PRIME] * B)
        plain = loaded(z, model, B, **kw)
        assert plain.harm is None
        plain_out = run(plain)
        plain_draws = draws(plain)
        on = list(range(0, B, 2))
        res = []
        for graph in (True, False):
            dec = loaded(z, model, B, on=on, **kw)
            assert dec.state.parity == parity and dec.harm is not None and dec.harm_on.tolist() == [1, 0] * (B // 2)
            res.append(run(dec, use_graph=graph))
            if graph:
                assert dec.graph is not None
                dr = draws(dec)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert torch.equal(bits(res[0][2]), bits(res[1][2]))
        check_loop(z, plain_out, plain_draws, res[0], dr, on, B)
    finally:
        model.parity_fp32 = False


def test_separate_launches_equal_the_fused_launch(fixture_model):
    z, model = fixture_model
    a = loaded(z, model, 4, on=[0, 2])
    fused = run(a, use_graph=False)
    b = loaded(z, model, 4, on=[0, 2])
    sep = LBG.separate_launches(b, b.generation_length + 1)
    assert torch.equal(fused[0], sep[0]) and torch.equal(fused[1], sep[1]) and torch.equal(bits(fused[2]), bits(sep[2]))


# ------------------------------------------------------------------------------------------------ 4. mid-bar chord change
def test_a_mid_bar_chord_change_switches_the_row_at_the_forced_chord(fixture_model):
    """The length_fit-false fixture places every second chord in the middle of a bar (position 496).  A pitch drawn before
    that position follows the old chord, the first pitch after the forced chord the new one: the row is keyed by the
    chords PLACED, not by the one that is pending."""
    z, model = fixture_model
    cpos = z["sample4x_chord_position"].tolist()
    assert 496 in cpos and len(z["sample4x_chord_token"]) != int(float(z["sample4x_cfg"][1]) // 4 * 4)
    dec = loaded(z, model, 8, on=list(range(8)), tag="sample4x", steer=NOTES, max_prompt=len(PRIME), prompts=[PRIME] * 8)
    run(dec)
    before = after = tell_old = tell_new = 0
    for b, (seq, drawn) in enumerate(draws(dec)):
        assert seq is not None and out_of_chord(seq, drawn) == [], (b, seq)
        for i, t in enumerate(seq):
            if not (195 <= t <= 303 and seq[i - 1] == 496):
                continue
            old = last_chord(seq[:i])
            bar = max(j for j in range(i) if seq[j] == 2)
            for j, p, c in drawn_pitches(seq, drawn):
                if bar < j < i:                                          # drawn while chord i was pending
                    assert c == old and (p - 3) % 12 in HC.pitch_classes(old), (b, j)
                    before += 1
                    tell_old += (p - 3) % 12 not in HC.pitch_classes(t)
            nxt = [x for x in drawn_pitches(seq, drawn) if x[0] > i]
            if nxt and nxt[0][2] == t:
                assert (nxt[0][1] - 3) % 12 in HC.pitch_classes(t), (b, nxt[0])
                after += 1
                tell_new += (nxt[0][1] - 3) % 12 not in HC.pitch_classes(old)
    print("pitches before a pending mid-bar chord:", before, "(outside the new chord:", tell_old, ") first pitches after one:",
          after, "(outside the old chord:", tell_new, ")")
    assert tell_old >= 2 and tell_new >= 2


# ------------------------------------------------------------------------------------------------ 5. primed slots
def one_class_table():
    """Row r admits the single pitch class (5 r + 2) mod 12; the no-chord row 109 admits class 5 only."""
    t = np.full((111, 16), NEG, np.float32)
    t[110] = 0
    t[:, 12:] = 0
    for r in range(109):
        t[r, (5 * r + 2) % 12] = 0
    t[109, 5] = 0
    return t


def test_a_primed_slots_first_pitch_is_keyed_by_the_last_chord_of_the_prompt(fixture_model):
    z, model = fixture_model
    src = loaded(z, model, 2, on=[0, 1])
    run(src)
    seq, drawn = draws(src)[0]
    n_ctx = 1 + len(z["encoded_meta"])
    body = seq[n_ctx:]
    # a prompt that ends on a velocity under a chord, the same cut one note earlier (a position: velocity, then the
    # pitch), and a prompt without any chord: position, velocity
    i = next(j for j in range(len(body)) if 131 <= body[j] <= 194 and last_chord(body[:j]) is not None)
    chord = last_chord(body[:i])
    prompts = [body[:i + 1], body[:i], [440, 150]]
    table = one_class_table()
    dec = loaded(z, model, 3, on=[0, 1, 2], table=table, max_prompt=len(prompts[0]), prompts=prompts)
    run(dec)
    for b, (got, dr) in enumerate(draws(dec)):
        cut = n_ctx + len(prompts[b])
        assert got is not None and got[:cut] == seq[:n_ctx] + prompts[b] and not dr[:cut].any() and dr[cut], b
        first = next(x for x in drawn_pitches(got, dr))
        want_row = HC.chord_row(got[:first[0]])
        assert first[0] == cut + (1 if b == 1 else 0)
        assert want_row == (109 if b == 2 else chord - 195), b
        assert (first[1] - 3) % 12 == (5 if b == 2 else (5 * want_row + 2) % 12), (b, first)
        assert out_of_chord(got, dr, table) == [], b


# ------------------------------------------------------------------------------------------------ 6. in place
def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    soft = one_class_table()
    ref_strict = run(loaded(z, model, 4, on=[0, 1, 2, 3]), use_graph=False)
    ref_other = run(loaded(z, model, 4, on=[1, 3], table=soft), use_graph=False)
    dec = loaded(z, model, 4, on=[0, 1, 2, 3])
    assert dec.graph is None
    s, f, l = run(dec)
    g = dec.graph
    assert g is not None and torch.equal(s, ref_strict[0]) and torch.equal(f, ref_strict[1])
    assert torch.equal(bits(l), bits(ref_strict[2])) and not torch.equal(s, s0)
    dec.set_harmony(None)                                               # off
    reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and not bool(dec.harm_on.any())
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))
    dec.set_harmony(soft, rows=[1, 3])                                  # another table, two slots
    reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.harm_on.tolist() == [0, 1, 0, 1]
    assert torch.equal(s, ref_other[0]) and torch.equal(f, ref_other[1]) and torch.equal(bits(l), bits(ref_other[2]))
    for b in (1, 3):
        assert out_of_chord(*draws(dec)[b], soft) == [] and not torch.equal(s[b], s0[b]), b
    ref_rearmed = run(loaded(z, model, 4, on=[2, 3], table=soft), use_graph=False)
    uni = reload(z, dec)                                                # rearm(harmony=) flips one switch
    dec.rearm(1, uni[1], harmony=False)
    dec.rearm(2, uni[2], harmony=True)
    s, f, l = run(dec)
    assert dec.graph is g and dec.harm_on.tolist() == [0, 0, 1, 1]
    assert torch.equal(s, ref_rearmed[0]) and torch.equal(f, ref_rearmed[1]) and torch.equal(bits(l), bits(ref_rearmed[2]))
    assert torch.equal(s[1], s0[1]) and torch.equal(s[0], s0[0])
    assert out_of_chord(*draws(dec)[2], soft) == [] and not torch.equal(s[2], s0[2])


# ------------------------------------------------------------------------------------------------ 7. one request
def test_generate_stream_returns_the_same_attempts_at_2_and_8_slots(fixture_model):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    meta, data = z["encoded_meta"].tolist(), TD._data(z, "sample8m")
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN)
    kw = dict(need=8, accept=lambda s, r: True, logit_bias=steer_row(), return_logprobs=True)
    outs = [gen.generate_stream(meta, data, 0.95, 32, slots=n, grammar=True, harmony=True, **kw) for n in (2, 8)]
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) == 8
    n_pitch = 0
    for s, lp in zip(outs[0][0], outs[0][2]):
        assert s is not None and out_of_chord(s, ~np.isnan(lp[:, 0])) == []
        n_pitch += len(under_a_chord(s, ~np.isnan(lp[:, 0])))
    assert n_pitch >= 20 and len({tuple(s) for s in outs[0][0]}) > 1
    # a request without harmony= clears what the one before left on the reused decoder
    after = gen.generate_stream(meta, data, 0.95, 32, slots=8, grammar=True, **kw)
    fresh = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN).generate_stream(
        meta, data, 0.95, 32, slots=8, grammar=True, **kw)
    assert after[0] == fresh[0] and len(gen._decoders) == 2
    assert any(out_of_chord(s, ~np.isnan(lp[:, 0])) for s, lp in zip(after[0], after[2]))
    with pytest.raises(CommuHipError, match="harmony: one setting for the request expected"):
        gen.generate_stream(meta, data, 0.95, 32, slots=8, harmony=[True] * 8, **kw)
    seqs, _ = gen.generate([meta] * 4, [data] * 4, 0.95, 32, grammar=True, harmony=True, logit_bias=steer_row())
    assert all(s is not None for s in seqs)


# ------------------------------------------------------------------------------------------------ 8. another cache; CLI
def test_fp8_sliding_cache_feeds_the_same_stage():
    """kv_dtype="fp8" with a sliding memory of 32 that wraps: the sampling stage does not care which cache produced the
    logits.  One short run with the assertions of the loop test (check_loop): slots alternate on / off, every slot primed
    behind its first chord with the bar lowered by 2 (PRIME, NOTES); graph replay == eager; every pitch an on-slot drew is a
    tone of its chord, each on-slot drew at least 10 of them and its twin left its chord; the off-slots are a decoder's
    that never heard of harmony."""
    import test_kv8_gpu as K8
    from commu_amd.generate import ForcedDecoder
    model, _ = K8._loop_model(32)
    with torch.no_grad():
        model.crit.out_layers[0].bias[2] = 3.0                           # bars again (K8's model bans them), as in the fixture
    chords = [199, 285, 267, 258]
    assert chords[0] == PRIME[2]
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": chords, "chord_position": [432] * 4})
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)

    def decoder(on):
        dec = ForcedDecoder(model, 4, generation_length=GLEN, memory_length=32, temperature=0.95, top_k=32, sliding=True,
                            kv_dtype="fp8", max_prompt=len(PRIME))
        dec.record_logprobs()
        dec.set_grammar(True)
        dec.set_logit_bias(steer_row(NOTES))
        if on:
            dec.set_harmony(True, rows=on)
        return dec

    def load(dec):
        dec.load([K8.META] * 4, [data] * 4, uni, prompts=[PRIME] * 4)
    plain = decoder(None)
    load(plain)
    plain_out = run(plain)
    plain_draws = draws(plain)
    assert plain.harm is None
    dec = decoder([0, 2])
    outs = []
    for graph in (False, True):
        load(dec)
        outs.append(run(dec, use_graph=graph))
    assert dec.state.kv_dtype == "fp8" and dec.sliding and dec.graph is not None and dec.harm_on.tolist() == [1, 0, 1, 0]
    assert int(dec.state.klen.max()) > 32                                # the ring wrapped
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(bits(outs[0][2]), bits(outs[1][2]))
    check_loop({"sample8m_chord_token": np.asarray(chords)}, plain_out, plain_draws, outs[1], draws(dec), [0, 2], 4)


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *args], capture_output=True,
                          text=True, timeout=120)


def test_cli_help_lists_the_flags():
    out = _cli("--help")
    assert out.returncode == 0 and "--harmony" in out.stdout and "--harmony_penalty" in out.stdout


def test_cli_refuses_an_unreadable_or_ill_shaped_table_before_a_model_is_loaded(tmp_path):
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt"),
              "--num_generate", "1"]
    out = _cli(*common, "--harmony", str(tmp_path / "missing.json"))
    assert out.returncode != 0 and "--harmony: chord, soft or a readable JSON file expected" in out.stderr
    short = tmp_path / "short.json"
    short.write_text(json.dumps([[0.0] * 12] * 109))
    out = _cli(*common, "--harmony", str(short))
    assert out.returncode != 0 and "a list of 110 rows of 12 numbers" in out.stderr
    dead = [[0.0] * 12 for _ in range(110)]
    dead[7] = [None] * 12
    full = tmp_path / "dead.json"
    full.write_text(json.dumps(dead))
    out = _cli(*common, "--harmony", str(full))
    assert out.returncode != 0 and "row 7 bans all 12 pitch classes" in out.stderr
    out = _cli(*common, "--harmony", "soft", "--harmony_penalty", "-1")
    assert out.returncode != 0 and "--harmony_penalty: a finite number >= 0 expected" in out.stderr
    assert not (tmp_path / "out").exists()
