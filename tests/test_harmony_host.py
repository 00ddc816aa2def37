"""The harmony constraint on the host (no GPU): the chord-tone map and the default table of the package against the
spelled-out list (harmony_contract), every refusal of harmony_rows, the invariant the kernel's row lookup rests on -- at
every draw the last chord token of seq is chord_tok[F_CUR - 1] -- walked through the forcing rules on random logits and
from primed states, and the effect of the strict table through the reference loop's restatement."""
import os

import numpy as np
import pytest
import torch

import grammar_contract as GC
import harmony_contract as HC
import logit_bias_contract as LB
import prime_contract as PC
import test_grammar_host as TG

V = 729
NEG = float("-inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the map and the table
def test_chord_pitch_classes_for_all_109_tokens():
    from commu_amd.midi_generator.meta import CHORD_VOCAB, chord_pitch_classes
    assert chord_pitch_classes(195) == frozenset({9, 1, 4}) == HC.pitch_classes(195)          # Chord_a: A, C#, E
    assert chord_pitch_classes(303) == frozenset() == HC.pitch_classes(303)                   # Chord_NN: no statement
    for t in range(195, 304):
        name, pcs = HC.CHORDS[t - 195]
        assert CHORD_VOCAB[name] == t, name                              # (the spelled-out list is in id order)
        assert chord_pitch_classes(t) == frozenset(pcs), (t, name)
        assert chord_pitch_classes(np.int32(t)) == frozenset(pcs)
    assert len({name for name, _ in HC.CHORDS}) == 109
    for bad in (194, 304, 0, -1, 195.5, True, "c"):
        with pytest.raises((ValueError, TypeError)):
            chord_pitch_classes(bad)


def test_default_table_against_the_spelled_out_list():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import harmony_rows, harmony_table
    t = harmony_table()
    assert t.dtype == np.float32 and t.shape == (111, 16)
    assert np.array_equal(t, HC.default_table())
    for tok in range(195, 304):
        pcs = HC.pitch_classes(tok)
        row = t[tok - 195]
        if tok == 303:
            assert not row.any()
        else:
            assert set(np.flatnonzero(row[:12] == 0).tolist()) == set(pcs) and (row[:12][row[:12] != 0] == NEG).all(), tok
    assert not t[108:].any() and not t[:, 12:].any()                    # NN, no chord yet, off; the pad columns
    soft = harmony_table(outside=-4.0, extra=(2, 9))
    assert np.array_equal(soft, HC.default_table(-4.0, (2, 9)))
    c = soft[HC.CHORDS.index(("c", (0, 4, 7)))]
    assert c[:12].tolist() == [0, -4, 0, -4, 0, -4, -4, 0, -4, 0, -4, -4]                     # c e g, and d and a
    assert np.array_equal(harmony_table(outside=0)[:, :12], np.zeros((111, 12), np.float32))
    assert np.array_equal(harmony_rows(t), t) and np.array_equal(harmony_rows(t[:110, :12]), t)
    assert np.array_equal(harmony_rows(torch.from_numpy(soft)), soft)
    for bad in (1.0, float("nan"), True, "x"):
        with pytest.raises(CommuHipError, match="outside"):
            harmony_table(outside=bad)
    for bad in ((1.5,), 3, ("a",)):
        with pytest.raises(CommuHipError, match="extra"):
            harmony_table(extra=bad)


def test_harmony_rows_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import harmony_rows, harmony_table
    t = harmony_table()
    for bad, what in ((t[:109], r"\(109, 16\)"), (t[:, :12], r"\(111, 12\)"), (t[:110], r"\(110, 16\)"), (t[0], r"\(16,\)"),
                      (np.zeros((2, 111, 16), np.float32), r"\(2, 111, 16\)"), ("abc", "str")):
        with pytest.raises(CommuHipError, match=what):
            harmony_rows(bad)
    nan = t.copy()
    nan[17, 3] = np.nan
    with pytest.raises(CommuHipError, match="row 17, entry 3 is nan"):
        harmony_rows(nan)
    inf = t.copy()
    inf[108, 11] = np.inf
    with pytest.raises(CommuHipError, match="row 108, entry 11 is inf"):
        harmony_rows(inf)
    off = t.copy()
    off[110, 5] = -2.5
    with pytest.raises(CommuHipError, match="row 110 .* entry 5 is -2.5"):
        harmony_rows(off)
    pad = t.copy()
    pad[40, 13] = 1.25
    with pytest.raises(CommuHipError, match="row 40, entry 13 is 1.25"):
        harmony_rows(pad)
    empty = t.copy()
    empty[109, :12] = NEG
    with pytest.raises(CommuHipError, match="row 109 bans all 12 pitch classes"):
        harmony_rows(empty)
    with pytest.raises(CommuHipError, match="row 0 bans all 12 pitch classes"):
        harmony_rows(np.full((110, 12), NEG, np.float32))
    almost = t.copy()
    almost[109, :11] = NEG                                              # one class left: fine
    assert harmony_rows(almost)[109, 11] == 0


# ------------------------------------------------------------------------------------------------ 2. the invariant
def last_chord(seq):
    for t in reversed(seq):
        if HC.CHORD_LO <= t <= HC.CHORD_HI:
            return t
    return None


# On plain random logits a BAR is one boundary id in 130, chords are placed only after a bar, and two requests in three never
# see a chord in 200 iterations.  BAR_BOOST on the bar's logit gives most requests several bars (measured on the free runs,
# no code under test involved: 46 / 58 / 60 of the 60 requests leave their chord at a boost of 2 / 3 / 4, 26 at 0).
BAR_BOOST = 3.0


def make_step(seed, seq, gram=None, harm=None, bar_boost=0.0):
    """Random logits per model step (the stream test_grammar_host.run_request uses; bar_boost is added to the bar's
    logit) with the constraints laid over them: the grammar row of the fed token's class, the harmony row of the last
    chord in seq.  Entries are 0 or -inf, so adding them before the division by the temperature is what adding them after
    it is."""
    g = torch.Generator().manual_seed(1000 + seed)
    gt = None if gram is None else torch.from_numpy(gram)

    def step(tok, mems):
        lg = 3.0 * torch.randn(V, generator=g)
        lg[PC.BAR] += bar_boost
        if gt is not None:
            lg = lg + gt[GC.token_class(int(tok)), :V]
        if harm is not None:
            lg = lg + torch.from_numpy(HC.wide_row(harm, HC.chord_row(seq)))
        return lg, mems
    return step


def record_loop(step, s, seq, chord_tok, chord_pos, temperature, top_k, uniforms, max_iters, on_draw):
    """The forcing loop on the device record's restatement (prime_contract.pre / post), one `pre` per iteration as the
    kernels run it; the draw is the oracle's.  on_draw(record, seq, probs, rejected) is called at every draw, before it
    (rejected: the chord tokens drawn and refused since the last chord was placed).  Returns seq, or None where nothing
    could be drawn."""
    from oracle import decode_ref as DR
    wrong, logits, n_draw = [], None, 0
    while True:
        cur0 = s[PC.F_CUR]
        t, act, kp, dr = PC.pre(s, seq, chord_tok, chord_pos, max_iters, 1 << 30)
        if s[PC.F_DONE]:
            return seq
        if s[PC.F_CUR] != cur0:
            wrong = []                                                  # (take_chord clears the rejected tokens)
        if act:
            logits = step(t, None)[0][1:].clone()
        if not dr:
            continue
        probs = DR.apply_sampling(DR.calc_probs(logits, temperature), top_k, wrong)
        on_draw(s, seq, probs, wrong)
        if not bool(torch.isfinite(probs).all()):
            return None
        if temperature == 0:
            token = int(probs.argmax())
        else:
            token = DR.draw_inverse_cdf(probs, uniforms[n_draw])
            n_draw += 1
        cur = s[PC.F_CUR]
        cp = chord_pos[cur] if cur < s[PC.F_NCHORD] else -1
        if cp not in (-1, PC.POS0) and (cp < token < PC.POS0 + PC.POS_RES or token == PC.BAR):
            wrong = []                                                  # (a position past the pending chord: post clears them)
        elif PC.CHORD_LO <= token <= PC.CHORD_HI:
            wrong.append(token)
        PC.post(s, seq, chord_pos, token, 1 << 30)


def run_record(r, gram=None, harm=None, on_draw=lambda s, seq, probs, wrong: None, bar_boost=0.0):
    seq = [0] + TG.META
    s = PC.initial_record(len(TG.META), len(r["chord_token"]), r["num_measures"])
    u = np.random.RandomState(r["seed"]).random_sample(256)
    return record_loop(make_step(r["seed"], seq, gram, harm, bar_boost), s, seq, r["chord_token"], r["chord_position"],
                       r["temperature"], 32, u, 200, on_draw)


def run_oracle(r, gram=None, harm=None, bar_boost=0.0):
    from oracle import decode_ref as DR
    seq = [0] + TG.META
    u = np.random.RandomState(r["seed"]).random_sample(256)
    return DR.generate_sequence(make_step(r["seed"], seq, gram, harm, bar_boost), seq, None, chord_token=r["chord_token"],
                                chord_position=r["chord_position"], num_measures=r["num_measures"],
                                temperature=r["temperature"], top_k=32, uniforms=u, max_iters=200)


def invariant(chord_tok, seen):
    def on_draw(s, seq, probs, wrong):
        cur = s[PC.F_CUR]
        assert 0 <= cur <= len(chord_tok)
        assert (chord_tok[cur - 1] if cur > 0 else None) == last_chord(seq), (cur, seq)
        assert s[PC.F_FORCED] < 0                                       # no chord is waiting to be appended at a draw
        seen[0] += 1
        seen[1] += cur > 0
        seen[2] += cur == 0
        seen[3] += len(wrong) > 0
    return on_draw


def test_the_last_chord_of_seq_is_chord_tok_cur_minus_1_at_every_draw():
    """The 60 random-logit requests of test_grammar_host (free and under the grammar, on its logit stream and on the one
    with more bars): the record loop is the oracle's loop token for token, and at each of its draws the invariant holds --
    also right after a rejected chord draw (Q5), which the free runs make."""
    from commu_amd.generate import event_grammar
    reqs = TG.requests(60)
    assert {r["num_measures"] for r in reqs} == {4.0, 8.0, 5.0}
    assert any(432 + 64 in r["chord_position"] for r in reqs) and any(r["temperature"] == 0 for r in reqs)
    seen = [0, 0, 0, 0]
    for gram, boost in ((None, 0.0), (event_grammar(), 0.0), (None, BAR_BOOST), (event_grammar(), BAR_BOOST)):
        for r in reqs:
            got = run_record(r, gram, None, invariant(r["chord_token"], seen), boost)
            assert got == run_oracle(r, gram, None, boost), r           # the same loop as the oracle's
            if got is not None:
                chords = [t for t in got if 195 <= t <= 303]
                assert chords == r["chord_token"][:len(chords)]
    print("draws checked:", seen[0], "with a chord:", seen[1], "before the first chord:", seen[2], "re-draws:", seen[3])
    assert seen[0] > 6000 and seen[1] > 2000 and seen[2] > 1000 and seen[3] > 0


def test_the_invariant_from_primed_states(golden_dir):
    """Slots primed by the replay (prime_contract.replay) at every cut point of the fixtures: the first draw after the
    prompt, and every draw after it, sees chord_tok[F_CUR - 1] as the last chord of seq -- none for a prompt without one."""
    z = np.load(os.path.join(golden_dir, "g6_decode.npz"))
    seen = [0, 0, 0, 0]
    first_with, first_without = 0, 0
    for k, tag in enumerate(PC.TAGS):
        ctx, ctok, cpos, nm, p = PC.fixture(z, tag)
        for cut in PC.cut_points(p):
            s, seq, fed, div = PC.replay(ctx, ctok, cpos, nm, p[:cut])
            assert div == (-1, -1), (tag, cut)
            assert seq == ctx + p[:cut]
            first = []

            def on_draw(s_, seq_, probs, wrong, inner=invariant(ctok, seen)):
                inner(s_, seq_, probs, wrong)
                if not first:
                    first.append((s_[PC.F_CUR], last_chord(seq_), len(seq_)))
            u = np.random.RandomState(cut).random_sample(64)
            record_loop(make_step(100 * k + cut, seq), s, seq, ctok, cpos, 0.95, 32, u, 40, on_draw)
            assert first and first[0][2] >= len(ctx) + cut, (tag, cut)
            want = last_chord(p[:cut]) if first[0][2] == len(ctx) + cut else first[0][1]
            assert first[0][1] == want
            first_with += first[0][1] is not None
            first_without += first[0][1] is None
    assert first_with >= 5 and first_without >= 5 and seen[0] > 200


# ------------------------------------------------------------------------------------------------ 3. the effect
def out_of_chord(seq, start):
    """Indices of the pitch tokens of seq[start:] outside the pitch classes of the last chord before them (a pitch
    before the first chord, or under Chord_NN, is never out)."""
    bad = []
    for i in range(start, len(seq)):
        if HC.PITCH_LO <= seq[i] <= HC.PITCH_HI:
            c = last_chord(seq[:i])
            if c is not None and c != 303 and (seq[i] - 3) % 12 not in HC.pitch_classes(c):
                bad.append(i)
    return bad


def test_strict_harmony_through_the_reference_loop():
    from commu_amd.generate import event_grammar, harmony_table
    from commu_amd.midi_generator.midi_inferrer import parse_events
    reqs = TG.requests(60)
    gram, harm = event_grammar(), harmony_table()
    start = 1 + len(TG.META)
    free_out = pitches = under_chord = 0
    for r in reqs:
        def on_draw(s, seq, probs, wrong):
            assert bool(torch.isfinite(probs).all()) and float(probs.sum()) > 0, r          # no request fails
            c = last_chord(seq)
            if c is not None and c != 303:                              # the distribution itself: no mass outside the chord
                ids = np.arange(HC.PITCH_LO, HC.PITCH_HI + 1)
                outside = [i for i in ids if (i - 3) % 12 not in HC.pitch_classes(c)]
                assert float(probs[outside].sum()) == 0.0
        seq = run_record(r, gram, harm, on_draw, BAR_BOOST)
        assert seq is not None and seq == run_oracle(r, gram, harm, BAR_BOOST), r
        assert parse_events(seq, start) is None
        assert out_of_chord(seq, start) == [], (r, seq)
        pitches += sum(1 for t in seq[start:] if HC.PITCH_LO <= t <= HC.PITCH_HI)
        under_chord += sum(1 for i in range(start, len(seq)) if HC.PITCH_LO <= seq[i] <= HC.PITCH_HI
                           and last_chord(seq[:i]) not in (None, 303))
        free = run_oracle(r, gram, None, BAR_BOOST)
        assert free is not None
        free_out += bool(out_of_chord(free, start))
    print("pitches drawn:", pitches, "under a chord:", under_chord, "requests with an out-of-chord pitch without harmony:",
          free_out, "of", len(reqs))
    assert under_chord >= 300
    assert free_out >= len(reqs) // 2                                   # the check has teeth


# ------------------------------------------------------------------------------------------------ 4. top-k
def test_a_harmony_ban_takes_none_of_the_top_k_places():
    from commu_amd.generate import event_grammar, harmony_table
    g = np.random.RandomState(5)
    raw = g.standard_normal(768).astype(np.float32)
    chord = 195 + HC.CHORDS.index(("c", (0, 4, 7)))
    outside = [i for i in range(HC.PITCH_LO, HC.PITCH_HI + 1) if (i - 3) % 12 not in (0, 4, 7)]
    top = outside[:32]
    raw[top] += 20.0                                                    # the 32 most likely ids are all out of the chord
    seq = [0, 600, 2, 432, chord, 440, 150]                             # ... velocity: a pitch comes next
    res = HC.restate_with_harmony(raw, 0.95, 32, harm=harmony_table(), tokens=seq, gram=event_grammar(), prev=seq[-1])
    assert LB.ban_is_before_topk(res, outside, 32)
    assert all((i - 3) % 12 in (0, 4, 7) for i in np.flatnonzero(res.probs > 0))
    assert res.probs[[2, 131]].sum() == 0                               # (the grammar's bans, not harmony's)
    free = HC.restate_with_harmony(raw, 0.95, 32, harm=harmony_table(), tokens=seq, harm_on=False)
    assert set(np.flatnonzero(free.probs > 0).tolist()) == set(top)
    # the same bans behind top-k would have left nothing
    late = LB.restate(raw, 0.95, 32, bias=np.where(np.isin(np.arange(768), outside), NEG, 0).astype(np.float32),
                      ban_after_topk=True)
    assert late.token == -1
    # ids 2 and 131 get no third add, 3 and 130 do
    flat = np.full((111, 16), -5.0, np.float32)
    flat[110] = 0
    flat[:, 12:] = 0
    y = HC.restate_with_harmony(raw, 1.0, 728, harm=flat, tokens=seq).y
    x = HC.restate_with_harmony(raw, 1.0, 728, harm=flat, tokens=seq, harm_on=False).y
    assert (y[1:3] == x[1:3]).all() and (y[131:] == x[131:]).all()
    assert (y[3:131] == (x[3:131] + np.float32(-5.0)).astype(np.float32)).all()


# ------------------------------------------------------------------------------------------------ 5. the command line
def test_read_harmony_of_the_command_line(tmp_path):
    import importlib.util
    import json
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import harmony_table
    spec = importlib.util.spec_from_file_location("commu_generate_cli", os.path.join(ROOT, "commu-code_amd", "generate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    margs = cli.parse_args()["model_args"].parse_known_args(["--harmony", "soft", "--harmony_penalty", "2.5"])[0]
    assert margs.harmony == "soft" and margs.harmony_penalty == 2.5
    assert cli.parse_args()["model_args"].parse_known_args([])[0].harmony_penalty == 4.0
    assert cli.read_harmony(None) is None
    assert np.array_equal(cli.read_harmony("chord"), harmony_table())
    assert np.array_equal(cli.read_harmony("soft", 2.5), harmony_table(outside=-2.5))
    doc = [[0.0] * 12 for _ in range(110)]
    doc[3][7] = None
    doc[109][0] = -1.5
    good = tmp_path / "table.json"
    good.write_text(json.dumps(doc))
    t = cli.read_harmony(str(good))
    assert t.shape == (111, 16) and t[3, 7] == NEG and t[109, 0] == -1.5 and not t[110].any() and not t[:, 12:].any()
    with pytest.raises(ValueError, match="chord, soft or a readable JSON file expected"):
        cli.read_harmony(str(tmp_path / "missing.json"))
    for bad in (doc[:109], [r[:11] for r in doc], {"rows": doc}, [["x"] * 12] * 110):
        p = tmp_path / "bad.json"
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError, match="a list of 110 rows of 12 numbers"):
            cli.read_harmony(str(p))
    p.write_text("{not json")
    with pytest.raises(ValueError, match="not JSON"):
        cli.read_harmony(str(p))
    doc[5] = [None] * 12
    p.write_text(json.dumps(doc))
    with pytest.raises(CommuHipError, match="row 5 bans all 12 pitch classes"):
        cli.read_harmony(str(p))
    for pen in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="--harmony_penalty"):
            cli.read_harmony("soft", pen)
