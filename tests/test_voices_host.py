"""The voice cap on the host: the restatement (tests/voices_contract.py) and the package's checkers (midi_inferrer.voice_bans,
voices_violation, max_sounding) on hand-written edge cases and random sequences, the grid-to-ticks argument for four time
signatures, the refusals of voices_ctl and check_voices, the struct mirrors, the walk of the forcing rules that asks whether
a note can start on a forced position, and the rule through the reference loop's restatement on the 60 random-logit requests
of test_grammar_host."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import grammar_contract as GC
import note_order_contract as NO
import prime_contract as PC
import test_grammar_host as GH
import voices_contract as VC

V = 729
CTX = [0] + GH.META          # the 12 context tokens every sequence starts with: no BAR, no POSITION
P = list(range(432, 560))
W = VC.word


def pos(q):
    return 432 + q


def dur(d):
    return 303 + d


# ------------------------------------------------------------------------------------------------ 1. edge cases
ONE = [2, pos(0), 150, 60, dur(32), pos(8), 150]          # one note [0, 32), the bar is at onset 8
# (name, tokens, F_LEN (None: len(tokens)), control word, the banned ids written out by hand)
EDGE_CASES = [
    ("ends_exactly_at_the_next_onset", CTX + [2, pos(0), 150, 60, dur(8), pos(8), 150], None, W(1, True), P[:8]),
    ("ends_one_step_past_it", CTX + [2, pos(0), 150, 60, dur(9), pos(8), 150], None, W(1, True), [60] + P[:9]),
    ("whole_bar_banned", CTX + [2, pos(5), 150, 60, dur(123)], None, W(1, True), [60] + P),
    ("end_clamped_to_128", CTX + [2, pos(100), 150, 60, dur(128)], None, W(1, True), [60] + P),
    ("previous_bar_ends_at_0", CTX + [2, pos(64), 150, 60, dur(64), 2], None, W(1, True), []),
    ("previous_bar_ends_at_1", CTX + [2, pos(64), 150, 60, dur(65), 2], None, W(1, True), [60, 432]),
    ("previous_bar_hangs_over_8_steps", CTX + [2, pos(120), 150, 60, dur(16), 2, pos(0), 150], None, W(1, True),
     [60] + P[:8]),
    ("two_bars_back_is_ignored", CTX + [2, pos(127), 150, 60, dur(128), 2, 2], None, W(1, True), []),
    ("two_bars_back_and_one_bar_back", CTX + [2, pos(127), 150, 60, dur(128), 2, pos(0), 150, 61, dur(4), 2], None,
     W(1, True), []),
    ("tie_n1", CTX + [2, pos(0), 150, 60, dur(16), pos(8), 150, 64, dur(8)], None, W(1), P[:16]),
    ("tie_n2", CTX + [2, pos(0), 150, 60, dur(16), pos(8), 150, 64, dur(8)], None, W(2), P[:16]),
    ("tie_n3", CTX + [2, pos(0), 150, 60, dur(16), pos(8), 150, 64, dur(8)], None, W(3), []),
    ("second_largest_end", CTX + [2, pos(0), 150, 60, dur(16), pos(8), 150, 64, dur(4)], None, W(2), P[:12]),
    ("no_duration_is_no_note", CTX + [2, pos(0), 150, 60], None, W(1, True), []),
    ("no_duration_then_a_position", CTX + [2, pos(0), 150, 60, pos(4), 150], None, W(1, True), []),
    ("chord_group_between_notes",
     CTX + [2, pos(0), 150, 60, dur(32), pos(8), 200, pos(8), 150, 64, dur(8), pos(16), 150], None, W(2, True),
     [60] + P[:16]),
    ("no_cap_with_restrike", CTX + ONE, None, W(0, True), [60]),
    ("cap_without_restrike", CTX + ONE, None, W(1), P[:32]),
    ("off", CTX + ONE, None, -1, []),
    ("restrike_after_a_bar_g0_is_0", CTX + [2, pos(100), 150, 60, dur(40), 2], None, W(0, True), [60]),
    ("same_pitch_twice_one_still_sounds", CTX + [2, pos(0), 150, 60, dur(4), pos(8), 150, 60, dur(4), pos(10), 150], None,
     W(0, True), [60]),
    ("L_0", [pos(0), 150, 60, dur(32)], 0, W(1, True), []),
    ("L_1", [pos(0), 150, 60, dur(32)], 1, W(1, True), []),
    ("L_3", [pos(0), 150, 60, dur(32)], 3, W(1, True), []),
    ("L_4", [pos(0), 150, 60, dur(32)], 4, W(1, True), [60] + P[:32]),
]


@pytest.mark.parametrize("name, tokens, length, ctl, want", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_bans_on_hand_written_cases(name, tokens, length, ctl, want):
    """Fails on the parent: midi_inferrer has no voice_bans."""
    from commu_amd.midi_generator.midi_inferrer import voice_bans
    n = len(tokens) if length is None else length
    assert VC.bans(tokens, n, ctl) == sorted(want)
    assert sorted(voice_bans(tokens[:min(max(n, 0), len(tokens))], ctl)) == sorted(want)


def random_tokens(rs, n):
    """Tokens from a small pool in which notes, bars and chord groups are frequent (and broken groups too)."""
    pool = [2, 2, pos(0), pos(4), pos(64), pos(120), pos(127), 150, 160, 60, 61, 62, dur(1), dur(8), dur(64), dur(128), 200, 1]
    out = []
    while len(out) < n:
        if rs.rand() < 0.5:
            out += [pool[i] for i in rs.randint(2, 7, 1)] + [150, int(rs.choice([60, 61, 62])),
                                                             int(rs.choice([dur(1), dur(8), dur(64), dur(128)]))]
        else:
            out.append(pool[rs.randint(len(pool))])
    return out[:n]


def test_voice_bans_equals_the_contract_on_random_sequences():
    from commu_amd.midi_generator.midi_inferrer import voice_bans
    rs = np.random.RandomState(5)
    some = 0
    for _ in range(1500):
        s = random_tokens(rs, rs.randint(0, 48))
        w = int(rs.choice([-1, 0, 1, 2, 3, 128, 256, 257, 258, 384]))
        n = int(rs.randint(-1, len(s) + 3))
        want = VC.bans(s, n, w)
        assert sorted(voice_bans(s[:min(max(n, 0), len(s))], w)) == want, (s, n, w)
        some += bool(want)
    assert some > 300


# ------------------------------------------------------------------------------------------------ 2. grid -> ticks
def clean_sequence(rs, n_notes, max_voices, restrike):
    """A grammar-clean sequence (bars, chord groups, note groups) drawn at random from what note order and the voice rule
    leave: every candidate token that either rule bans is drawn again."""
    from commu_amd.midi_generator.midi_inferrer import note_order_bans, voice_bans
    word = W(max_voices, restrike)
    seq = list(CTX) + [2]
    for _ in range(n_notes):
        for _try in range(200):
            kind = rs.rand()
            if kind < 0.15:
                group = [2]
            elif kind < 0.25:
                group = [pos(int(rs.randint(128))), 200]
            else:
                group = [pos(int(rs.randint(128))), 150, int(rs.randint(40, 52)),
                         dur(int(rs.choice([1, 2, 3, 8, 17, 64, 100, 128])))]
            ok = True
            for k, t in enumerate(group):
                pre = seq + group[:k]
                if t in note_order_bans(pre, 0) or t in voice_bans(pre, word):
                    ok = False
                    break
            if ok:
                seq += group
                break
    return seq


@pytest.mark.parametrize("sig, ticks_per_bar", [("4/4", 1920), ("3/4", 1440), ("6/8", 1440), ("12/8", 2880)])
def test_no_overlap_on_the_grid_is_no_overlap_in_ticks(sig, ticks_per_bar):
    """The reference places onset q at floor(q T / 128) ticks and gives d steps d int(T / 128) ticks; if q >= a + d then
    floor(q T / 128) >= floor(a T / 128) + d int(T / 128).  Sequences that pass voices_violation on the grid are counted
    here in ticks by max_sounding, which shares no code with it."""
    from commu_amd.midi_generator.midi_inferrer import max_sounding, note_order_violation, parse_events, voices_violation
    assert 480 * int(int(sig.split("/")[0]) / int(sig.split("/")[1]) * 4) == ticks_per_bar
    rs = np.random.RandomState(ticks_per_bar)
    start = len(CTX)
    reached = 0
    for n, r in ((1, True), (2, True), (3, False), (1, False)):
        for _ in range(12):
            seq = clean_sequence(rs, 40, n, r)
            assert parse_events(seq, start) is None and note_order_violation(seq, start) is None
            assert voices_violation(seq, start, n, r) is None
            most, struck = max_sounding(seq, ticks_per_bar, start)
            assert most <= n and not (r and struck), (sig, n, r, most, struck, seq)
            reached += most == n
    assert reached >= 24                                                  # (the cap was reached, not merely respected)
    # teeth of the checker itself: an overlap it must see, in ticks
    two = CTX + [2, pos(0), 150, 60, dur(9), pos(8), 150, 60, dur(4)]
    assert max_sounding(two, ticks_per_bar, start) == (2, True) and voices_violation(two, start, 1, True) == start + 5
    assert voices_violation(two, start, 0, True) == start + 7 and voices_violation(two, start, 2, False) is None
    touch = CTX + [2, pos(0), 150, 60, dur(8), pos(8), 150, 60, dur(4)]
    assert max_sounding(touch, ticks_per_bar, start) == (1, False) and voices_violation(touch, start, 1, True) is None
    over_bar = CTX + [2, pos(120), 150, 60, dur(16), 2, pos(7), 150, 61, dur(1)]
    assert max_sounding(over_bar, ticks_per_bar, start)[0] == 2 and voices_violation(over_bar, start, 1, True) == start + 6


# ------------------------------------------------------------------------------------------------ 3. host surface
def test_voices_ctl_values_and_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import voices_ctl, voices_word
    assert voices_word() == 0 and voices_word(1) == 1 and voices_word(0, True) == 256 and voices_word(128, True) == 384
    assert voices_ctl(None, 3).tolist() == [-1, -1, -1] and voices_ctl(False, 2).tolist() == [-1, -1]
    assert voices_ctl(257, 2).tolist() == [257, 257] and voices_ctl(np.int64(384), 1).tolist() == [384]
    got = voices_ctl([None, False, 0, -1, 1, 128, 256, 2.0], 8)
    assert got.dtype == np.int32 and got.tolist() == [-1, -1, 0, -1, 1, 128, 256, 2]
    assert voices_ctl(np.array([0, 259], dtype=np.int32), 2).tolist() == [0, 259]
    for bad, shown in ((129, "129"), (385, "385"), (512, "512"), (-2, "-2"), (1.5, "1.5"), (float("nan"), "nan"),
                       (True, "True"), ("on", "'on'")):
        with pytest.raises(CommuHipError, match=r"voices: .*\[0, 128\].*got " + shown):
            voices_ctl(bad, 4)
    with pytest.raises(CommuHipError, match=r"voices\[2\]: .*got 200"):
        voices_ctl([0, 1, 200, 0], 4)
    with pytest.raises(CommuHipError, match=r"voices: 4 values expected \(one per sequence\), got 3"):
        voices_ctl([0, 1, 2], 4)
    with pytest.raises(CommuHipError, match="one value per sequence expected"):
        voices_ctl([[0, 1], [1, 0]], 2)


def cli_module():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "commu-code_amd", "generate.py")
    spec = importlib.util.spec_from_file_location("commu_generate_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_check_voices_of_the_command_line():
    cli = cli_module()
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(max_voices=None, no_restrike=False, note_order=False, max_notes=None),
                                                   **kw))
    a = ns()
    assert cli.check_voices(a) is None and a.voices_word is None and a.note_order is False
    a = ns(max_voices="1")
    assert cli.check_voices(a) == 1 and a.note_order is True and cli.check_note_order(a) == 0
    a = ns(no_restrike=True)
    assert cli.check_voices(a) == 256 and a.note_order is True
    a = ns(max_voices="128", no_restrike=True, max_notes="2")
    assert cli.check_voices(a) == 384 and cli.check_note_order(a) == 2
    for bad in ("0", "129", "-1", "two", 1.5):
        with pytest.raises(ValueError, match=r"--max_voices: an integer in \[1, 128\] expected"):
            cli.check_voices(ns(max_voices=bad))


def test_struct_mirrors_carry_the_field_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        names = [n for n, _ in cls._fields_]
        assert names[-3:] == ["order_ctl", "voice_ctl", "cls_ctl"]          # cls_ctl stays the last field
        assert _lib.struct_args(cls).voice_ctl is None                     # null unless named


def stub(B=4):
    """test_note_order_host's decoder without a model or a device, with the two attributes this feature adds."""
    import test_note_order_host as NH
    dec = NH.stub(B)
    dec.voice_ctl = dec._voice_host = None
    return dec


def test_set_voices_allocates_once_switches_note_order_on_and_rewrites_in_place():
    from commu_amd._lib import CommuHipError
    dec = stub()
    dec.set_voices(None)
    dec.set_voices(False, rows=[1])
    assert dec.voice_ctl is None and dec.order_ctl is None and dec.graph == "captured"      # off on a fresh decoder: nothing
    with pytest.raises(CommuHipError, match="got 500"):
        dec.set_voices(500)
    assert dec.voice_ctl is None and dec.order_ctl is None and dec.graph == "captured"      # refused before anything changed
    dec.set_voices(257, rows=[0, 2])
    assert dec.voice_ctl.tolist() == [257, -1, 257, -1] and dec.order_ctl.tolist() == [0, -1, 0, -1] and dec.graph is None
    assert dec.cls_ctl is not None and dec.bias is not None
    words, order = dec.voice_ctl, dec.order_ctl
    dec.graph = "captured again"
    dec.set_note_order(3, rows=[1])
    dec.set_voices([1, 384], rows=[1, 2])                                  # (slot 1 keeps the cap per position it has)
    assert dec.voice_ctl is words and words.tolist() == [257, 1, 384, -1] and dec.order_ctl is order
    assert order.tolist() == [0, 3, 0, -1] and dec.graph == "captured again"
    dec.set_voices(None)
    assert words.tolist() == [-1] * 4 and order.tolist() == [0, 3, 0, -1] and dec.graph == "captured again"
    dec.rearm(3, voices=256)
    assert words.tolist() == [-1, -1, -1, 256] and order.tolist() == [0, 3, 0, 0] and dec.graph == "captured again"
    dec.rearm(3, voices=False)
    assert words.tolist() == [-1] * 4


# ------------------------------------------------------------------------------------------------ 4. the forcing rules
def walk(r, gram, order_ctl, voice_ctl, bar_boost, on_forced_position):
    """The forcing loop on the device record's restatement (prime_contract.pre / post), one `pre` per iteration as the
    kernels run it, on random logits under the grammar, the note order and the voice rule.  on_forced_position(seq, index,
    next) is called for every POSITION token the rules append (not a draw) with what follows it: "forced" when the next
    append is forced too, "draw" when the next thing that happens is a draw, "end" when nothing follows."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    table = torch.from_numpy(gram)
    seq = list(CTX)
    s = PC.initial_record(len(GH.META), len(r["chord_token"]), r["num_measures"])
    u = np.random.RandomState(r["seed"]).random_sample(256)
    wrong, logits, n_draw, pending = [], None, 0, None
    while True:
        cur0, len0 = s[PC.F_CUR], len(seq)
        t, act, kp, dr = PC.pre(s, seq, r["chord_token"], r["chord_position"], 200, 1 << 30)
        if s[PC.F_DONE]:
            if pending is not None:
                on_forced_position(seq, pending, "end")
            return seq
        if len(seq) > len0:                                             # a forced token was appended
            if pending is not None:
                on_forced_position(seq, pending, "forced")
            pending = len0 if 432 <= seq[len0] <= 559 else None
        if s[PC.F_CUR] != cur0:
            wrong = []
        if act:
            lg = 3.0 * torch.randn(V, generator=g)
            lg[2] += bar_boost
            logits = (lg + table[GC.token_class(int(t)), :V])[1:].clone()
        if not dr:
            continue
        if pending is not None:
            on_forced_position(seq, pending, "draw")
            pending = None
        row = logits.clone()
        banned = sorted(set(NO.bans(seq, len(seq), order_ctl)) | set(VC.bans(seq, len(seq), voice_ctl)))
        if banned:
            row[[i - 1 for i in banned]] = float("-inf")
        probs = DR.apply_sampling(DR.calc_probs(row, r["temperature"]), 32, wrong)
        if not bool(torch.isfinite(probs).all()):
            return None
        if r["temperature"] == 0:
            token = int(probs.argmax())
        else:
            token = DR.draw_inverse_cdf(probs, u[n_draw])
            n_draw += 1
        cur = s[PC.F_CUR]
        cp = r["chord_position"][cur] if cur < s[PC.F_NCHORD] else -1
        if cp not in (-1, PC.POS0) and (cp < token < PC.POS0 + PC.POS_RES or token == PC.BAR):
            wrong = []
        elif PC.CHORD_LO <= token <= PC.CHORD_HI:
            wrong.append(token)
        PC.post(s, seq, r["chord_position"], token, 1 << 30)


@pytest.fixture(scope="module")
def grammar():
    from commu_amd.generate import event_grammar
    return event_grammar()


# two requests outside the 60: the first chord not at the start of its bar; as many chords as the bars ask for (F_LENGTH_FIT)
# with two of them inside one bar
MID_BAR_FIRST = dict(seed=3, chord_token=[200, 201, 202, 203], chord_position=[496, 432, 432, 432], num_measures=4.0,
                     temperature=0.9)
MID_BAR_FIT = dict(seed=4, chord_token=[200, 201, 202, 203], chord_position=[432, 496, 432, 496], num_measures=4.0,
                   temperature=0.9)


def test_what_follows_a_forced_position(grammar):
    """The issue's question: is a forced Position (432 after a bar, or a chord's position cp) always followed by a forced
    chord while chords remain, so that no note can start on it?  Walked on the 60 requests, with free-running bars and with
    more of them (test_harmony_host.BAR_BOOST), the rule off and on: YES on all of them -- every forced position is followed
    by its forced chord.  NOT IN GENERAL, and the two requests above show the exception: `post` forces the pending chord's
    position cp (a drawn position past it, or a drawn Bar) whatever the record says, but `pre` forces the chord behind it only
    once the sequence is filled (more than one Bar) and, for a request whose chord count fits its bars (F_LENGTH_FIT), only
    at `Bar, Position 432`.  So with a first chord that is not at 432, or a fitting request with a chord inside a bar, the
    token after the forced position is a DRAW: a note may start there, on an onset the voice rule never saw as a candidate.
    Its pitch is still drawn, so the re-strike ban holds there; the cap does not (README, DESIGN: "anything a forced token
    starts")."""
    reqs = GH.requests(60)
    tally = {"forced": 0, "draw": 0, "end": 0}

    def on_forced(seq, i, nxt):
        tally[nxt] += 1
        if nxt == "forced":
            assert 195 <= seq[i + 1] <= 303, (i, seq)                     # what is forced behind a position is its chord
    for boost in (0.0, 3.0):
        for word in (-1, W(1, True)):
            for r in reqs:
                walk(r, grammar, 0, word, boost, on_forced)
    print("the 60 requests: forced positions followed by a forced chord:", tally["forced"], "by a draw:", tally["draw"],
          "by nothing:", tally["end"])
    assert tally["forced"] > 100 and tally["draw"] == 0
    for r in (MID_BAR_FIRST, MID_BAR_FIT):
        seen = []
        walk(r, grammar, 0, W(1, True), 0.0, lambda seq, i, nxt: seen.append((nxt, seq[i], seq[i - 1])))
        draws = [x for x in seen if x[0] == "draw"]
        print("exception:", r["chord_position"], "forced positions followed by a draw:", len(draws))
        assert draws and all(p == 496 for _, p, _ in draws)               # a chord's position, never `Bar, Position 432`


# ------------------------------------------------------------------------------------------------ 5. the reference loop
def run_request(r, gram, order_ctl, voice_ctl):
    """test_note_order_host.run_request with both rules in the step callback (the loop appends to `seq` in place, so the
    callback sees the sequence as it is when the logits it returns are drawn from)."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    table = torch.from_numpy(gram)
    seq = list(CTX)

    def step(tok, mems):
        lg = 3.0 * torch.randn(V, generator=g) + table[GC.token_class(int(tok)), :V]
        banned = sorted(set(NO.bans(seq, len(seq), order_ctl)) | set(VC.bans(seq, len(seq), voice_ctl)))
        if banned:
            lg[banned] = float("-inf")
        return lg, mems
    u = np.random.RandomState(r["seed"]).random_sample(256)
    return DR.generate_sequence(step, seq, None, chord_token=r["chord_token"], chord_position=r["chord_position"],
                                num_measures=r["num_measures"], temperature=r["temperature"], top_k=32, uniforms=u,
                                max_iters=200)


def test_note_order_alone_lets_notes_overlap(grammar):
    from commu_amd.midi_generator.midi_inferrer import max_sounding, voices_violation
    start = len(CTX)
    seqs = [run_request(r, grammar, 0, -1) for r in GH.requests(60)]
    assert all(s is not None for s in seqs)
    over = sum(max_sounding(s, 1920, start)[0] > 1 for s in seqs)
    struck = sum(max_sounding(s, 1920, start)[1] for s in seqs)
    broken = sum(voices_violation(s, start, 1, True) is not None for s in seqs)
    print("note order only: requests with more than one sounding note:", over, "of 60; with a re-struck pitch:", struck,
          "; that break the rule:", broken)
    assert over >= 30 and broken >= over


def test_the_rule_through_the_reference_loop(grammar):
    """N = 1 with r = 1 on the 60 requests: none ends by Q12, all stay parse_events-clean and pass voices_violation (forced
    tokens included); in ticks no request holds two sounding notes except on an onset that a forced position started (the
    exception test_what_follows_a_forced_position pins), and those are counted and printed, not filtered."""
    from commu_amd.midi_generator.midi_inferrer import (max_sounding, note_order_violation, parse_events,
                                                        voices_violation)
    start = len(CTX)
    q12, over, lengths = 0, [], []
    for r in GH.requests(60):
        seq = run_request(r, grammar, 0, W(1, True))
        if seq is None:
            q12 += 1
            continue
        assert parse_events(seq, start) is None, (r, seq)
        assert note_order_violation(seq, start) is None, (r, seq)
        most, struck = max_sounding(seq, 1920, start)
        if most > 1 or struck or voices_violation(seq, start, 1, True) is not None:
            over.append((r["seed"], most, struck, voices_violation(seq, start, 1, True)))
        lengths.append(len(seq))
    print("N = 1, r = 1: Q12 endings:", q12, "of 60; requests over the cap:", len(over), over, "; mean length",
          np.mean(lengths))
    assert q12 == 0
    assert len(over) == 0
