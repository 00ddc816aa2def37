"""The note density on the host: the restatement (tests/density_contract.py) on hand-written edge cases and against a brute
force on random rows, the refusals of density_ctl and check_density, the struct mirrors, set_density on the model-less stub,
what the forcing rules do when the upper bound closes a bar ahead of a mid-bar chord, and the rule through the reference
loop's restatement on the 60 random-logit requests of test_grammar_host."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import density_contract as DC
import grammar_contract as GC
import note_order_contract as NO
import prime_contract as PC
import test_grammar_host as GH
import test_voices_host as VH
import voices_contract as VC

V = 729
CTX = VH.CTX                 # the 12 context tokens every sequence starts with: no BAR, no POSITION
P = list(range(432, 560))
W = DC.word
pos, dur = VH.pos, VH.dur


def note(q, pitch=60, d=4):
    return [pos(q), 150, pitch, dur(d)]


# ------------------------------------------------------------------------------------------------ 1. edge cases
THREE_BARS = CTX + [2] + note(0) + [2] + note(0) + note(4, 61) + [2] + note(0) + note(1, 61) + note(2, 62)
# (name, tokens, F_LEN (None: len(tokens)), density word, note-order word, voice word, the banned ids written out by hand)
EDGE_CASES = [
    ("no_bar_in_S", CTX + note(0) + note(8, 61), None, W(3), 0, 0, [1, 2]),
    ("no_bar_in_S_upper", CTX + note(0) + note(8, 61), None, W(0, 2), 0, 0, P),
    ("bar_is_the_last_token", CTX + note(0) + [2], None, W(1, 4), 0, 0, [1, 2]),
    ("bar_is_the_last_token_no_lower", CTX + note(0) + [2], None, W(0, 4), 0, 0, []),
    ("C_at_lo_minus_1", CTX + [2] + note(0), None, W(2, 3), 0, 0, [1, 2]),
    ("C_at_lo_and_hi_minus_1", CTX + [2] + note(0) + note(4, 61), None, W(2, 3), 0, 0, []),
    ("C_at_hi", CTX + [2] + note(0) + note(4, 61) + note(8, 62), None, W(2, 3), 0, 0, P),
    ("C_past_hi", CTX + [2] + note(0) + note(4, 61) + note(8, 62), None, W(1, 2), 0, 0, P),
    ("lo_equals_hi", CTX + [2] + note(0) + note(4, 61), None, W(2, 2), 0, 0, P),
    ("incomplete_group_at_the_end", CTX + [2] + note(0) + [pos(8), 150, 61], None, W(2), 0, 0, [1, 2]),
    ("incomplete_group_does_not_count", CTX + [2] + note(0) + [pos(8), 150, 61], None, W(0, 2), 0, 0, []),
    ("chord_group_is_no_note", CTX + [2, pos(0), 200] + note(0), None, W(2, 2), 0, 0, [1, 2]),
    ("beta_0_1_2_lower", THREE_BARS, None, W(4), 0, 0, [1, 2]),
    ("beta_0_1_2_upper", THREE_BARS, None, W(0, 3), 0, 0, P),
    ("beta_0_1_2_neither", THREE_BARS, None, W(3, 4), 0, 0, []),
    ("beta_0_1_2_cut_to_the_second_bar", THREE_BARS, len(CTX) + 14, W(3), 0, 0, [1, 2]),
    ("beta_0_1_2_cut_to_the_second_bar_upper", THREE_BARS, len(CTX) + 14, W(1, 2), 0, 0, P),
    ("waiver_voice_cap_1_note_reaches_the_bar_end", CTX + [2, pos(5), 150, 60, dur(123)], None, W(2), 0, VC.word(1), []),
    ("no_waiver_without_the_cap", CTX + [2, pos(5), 150, 60, dur(123)], None, W(2), 0, 0, [1, 2]),
    ("no_waiver_one_step_short", CTX + [2, pos(5), 150, 60, dur(122)], None, W(2), 0, VC.word(1), [1, 2]),
    ("waiver_note_order_cap_at_the_last_position", CTX + [2] + note(127, 60, 1), None, W(2), 1, 0, []),
    ("no_waiver_note_order_off", CTX + [2] + note(127, 60, 1), None, W(2), -1, -1, [1, 2]),
    ("upper_bound_waives_nothing_it_needs", CTX + [2] + note(0), None, W(1, 1), 0, 0, P),
    ("off", CTX + [2] + note(0), None, -1, 0, 0, []),
    ("word_0_bans_nothing", CTX + [2] + note(0), None, 0, 0, 0, []),
    ("L_0", note(0), 0, W(1, 1), 0, 0, [1, 2]),
    ("L_3", note(0), 3, W(1, 1), 0, 0, [1, 2]),
    ("L_4", note(0), 4, W(1, 1), 0, 0, P),
]


@pytest.mark.parametrize("name, tokens, length, ctl, order, voice, want", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_bans_on_hand_written_cases(name, tokens, length, ctl, order, voice, want):
    n = len(tokens) if length is None else length
    assert DC.bans(tokens, n, ctl, order, voice) == sorted(want)


def brute_bans(tokens, length, ctl, order, voice):
    """The rule once more, differently: the open bar found by its last BAR, its groups counted forward, and the waiver asked
    of the SET of banned positions, not of the ends."""
    if ctl < 0:
        return []
    S = [int(t) for t in tokens[:min(max(length, 0), len(tokens))]]
    last = max([i for i, t in enumerate(S) if t == 2], default=-1)
    bar = S[last + 1:]
    c = sum(1 for i in range(len(bar) - 3) if 432 <= bar[i] <= 559 and 131 <= bar[i + 1] <= 194 and 3 <= bar[i + 2] <= 130
            and 304 <= bar[i + 3] <= 431)
    lo, hi = ctl % 256, ctl // 256
    banned = set(NO.bans(S, len(S), order)) | set(VC.bans(S, len(S), voice))
    out = set()
    if hi and c >= hi:
        out |= set(P)
    if lo and c < lo and not set(P) <= (banned | out):
        out |= {1, 2}
    return sorted(out)


def test_bans_equal_a_brute_force_on_random_rows():
    rs = np.random.RandomState(11)
    some = waived = 0
    for _ in range(1500):
        s = VH.random_tokens(rs, rs.randint(0, 64))
        ctl = int(rs.choice([-1, 0, W(1), W(2), W(3), W(0, 1), W(0, 2), W(1, 1), W(2, 3), W(255, 255)]))
        order, voice = int(rs.choice([-1, 0, 1])), int(rs.choice([-1, 0, 1, 2, 257]))
        n = int(rs.randint(-1, len(s) + 3))
        want = brute_bans(s, n, ctl, order, voice)
        assert DC.bans(s, n, ctl, order, voice) == want, (s, n, ctl, order, voice)
        some += bool(want)
        waived += ctl >= 0 and ctl % 256 > DC.count(s, n) and 2 not in want
    assert some > 300 and waived > 10


# ------------------------------------------------------------------------------------------------ 2. host surface
def test_density_ctl_values_and_refusals():
    """Fails on the parent: generate has no density_ctl."""
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import density_ctl, density_word
    assert density_word() == 0 and density_word(2) == 2 and density_word(0, 6) == 1536 and density_word(2, 6) == 1538
    assert density_word(255, 255) == 65535 and W(2, 6) == density_word(2, 6)
    assert density_ctl(None, 3).tolist() == [-1, -1, -1] and density_ctl(False, 2).tolist() == [-1, -1]
    assert density_ctl(1538, 2).tolist() == [1538, 1538] and density_ctl(np.int64(65535), 1).tolist() == [65535]
    got = density_ctl([None, False, 0, -1, 1, 256, 257, 2.0], 8)
    assert got.dtype == np.int32 and got.tolist() == [-1, -1, 0, -1, 1, 256, 257, 2]
    assert density_ctl(np.array([0, 1538], dtype=np.int32), 2).tolist() == [0, 1538]
    assert density_ctl(torch.tensor([3, -1]), 2).tolist() == [3, -1]
    for bad, shown in ((65536, "65536"), (-2, "-2"), (1.5, "1.5"), (float("nan"), "nan"), (True, "True"), ("on", "'on'"),
                       (W(3, 2), "515"), (W(255, 1), "511")):
        with pytest.raises(CommuHipError, match=r"density: .*\[0, 255\].*got " + shown):
            density_ctl(bad, 4)
    with pytest.raises(CommuHipError, match=r"density\[2\]: .*got 70000"):
        density_ctl([0, 1, 70000, 0], 4)
    with pytest.raises(CommuHipError, match=r"density: 4 values expected \(one per sequence\), got 3"):
        density_ctl([0, 1, 2], 4)
    with pytest.raises(CommuHipError, match="one value per sequence expected"):
        density_ctl([[0, 1], [1, 0]], 2)


def test_check_density_of_the_command_line():
    cli = VH.cli_module()
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(min_notes_per_bar=None, max_notes_per_bar=None, max_voices=None,
                                                        no_restrike=False, note_order=False, max_notes=None), **kw))
    a = ns()
    assert cli.check_density(a) is None and a.density_word is None and a.note_order is False
    a = ns(min_notes_per_bar="2")
    assert cli.check_density(a) == 2 and a.note_order is True and cli.check_note_order(a) == 0
    a = ns(max_notes_per_bar="6")
    assert cli.check_density(a) == 1536 and a.note_order is True
    a = ns(min_notes_per_bar="2", max_notes_per_bar="6", max_voices="1", max_notes="2")
    assert cli.check_density(a) == 1538 and a.density_word == 1538 and cli.check_voices(a) == 1
    assert cli.check_note_order(a) == 2
    assert cli.check_density(ns(min_notes_per_bar="255", max_notes_per_bar="255")) == 65535
    for flag in ("min_notes_per_bar", "max_notes_per_bar"):
        for bad in ("0", "256", "-1", "two", 1.5):
            with pytest.raises(ValueError, match=r"--%s: an integer in \[1, 255\] expected" % flag):
                cli.check_density(ns(**{flag: bad}))
    with pytest.raises(ValueError, match=r"--max_notes_per_bar: not below --min_notes_per_bar expected, got 2 < 3"):
        cli.check_density(ns(min_notes_per_bar="3", max_notes_per_bar="2"))
    args = cli.parse_args.__globals__                                       # (the flags exist on the parser)
    assert args["NOTES_PER_BAR_MIN"] == 1 and args["NOTES_PER_BAR_MAX"] == 255


def test_struct_mirrors_carry_the_field_ahead_of_order_ctl_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    assert C.sizeof(_lib.DecodeArmArgs) == lib.commu_decode_arm_args_bytes()
    assert C.sizeof(_lib.DecodeArmPrimedArgs) == lib.commu_decode_arm_primed_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        names = [n for n, _ in cls._fields_]
        assert names[-4:] == ["density_ctl", "order_ctl", "voice_ctl", "cls_ctl"]
        assert _lib.struct_args(cls).density_ctl is None                   # null unless named
    for cls in (_lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs):
        names = [n for n, _ in cls._fields_]
        assert names[names.index("order_ctl") - 2:names.index("order_ctl")] == ["density_ctl", "e_density"]
        assert _lib.struct_args(cls).density_ctl is None and _lib.struct_args(cls).e_density is None


def stub(B=4):
    """test_voices_host's decoder without a model or a device, with the two attributes this feature adds."""
    dec = VH.stub(B)
    dec.density_ctl = dec._density_host = None
    return dec


def test_set_density_allocates_once_switches_voices_and_note_order_on_and_rewrites_in_place():
    from commu_amd._lib import CommuHipError
    dec = stub()
    dec.set_density(None)
    dec.set_density(False, rows=[1])
    assert dec.density_ctl is None and dec.voice_ctl is None and dec.order_ctl is None and dec.graph == "captured"
    with pytest.raises(CommuHipError, match="got 70000"):
        dec.set_density(70000)
    with pytest.raises(CommuHipError, match="got 515"):
        dec.set_density(W(3, 2))
    assert dec.density_ctl is None and dec.voice_ctl is None and dec.graph == "captured"   # refused before anything changed
    dec.set_density(W(2, 6), rows=[0, 2])
    assert dec.density_ctl.tolist() == [1538, -1, 1538, -1] and dec.voice_ctl.tolist() == [0, -1, 0, -1]
    assert dec.order_ctl.tolist() == [0, -1, 0, -1] and dec.graph is None
    assert dec.cls_ctl is not None and dec.bias is not None
    words, voices, order = dec.density_ctl, dec.voice_ctl, dec.order_ctl
    dec.graph = "captured again"
    dec.set_voices(257, rows=[1])
    dec.set_note_order(3, rows=[3])
    dec.set_density([W(1), W(0, 4), 0], rows=[1, 2, 3])                     # (slots 1 and 3 keep the words they have)
    assert dec.density_ctl is words and words.tolist() == [1538, 1, 1024, 0]
    assert dec.voice_ctl is voices and voices.tolist() == [0, 257, 0, 0]
    assert dec.order_ctl is order and order.tolist() == [0, 0, 0, 3] and dec.graph == "captured again"
    dec.set_density(None)
    assert words.tolist() == [-1] * 4 and voices.tolist() == [0, 257, 0, 0] and order.tolist() == [0, 0, 0, 3]
    assert dec.graph == "captured again"
    dec.rearm(3, density=W(2))
    assert words.tolist() == [-1, -1, -1, 2] and dec.graph == "captured again"
    dec.rearm(3, density=False)
    assert words.tolist() == [-1] * 4


# ------------------------------------------------------------------------------------------------ 3. the forcing rules
def walk(r, gram, order_ctl, voice_ctl, density_ctl, bar_boost=0.0, max_iters=200):
    """test_voices_host.walk with the density rule among the bans and a record of which tokens were DRAWN: the forcing loop
    on the device record's restatement (prime_contract.pre / post), one `pre` per iteration, on random logits under the
    grammar.  Returns (seq, drawn mask, record); seq is None when a row had nothing left (the Q12 exit)."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    table = torch.from_numpy(gram)
    seq = list(CTX)
    drawn = [False] * len(seq)
    s = PC.initial_record(len(GH.META), len(r["chord_token"]), r["num_measures"])
    u = np.random.RandomState(r["seed"]).random_sample(256)
    wrong, logits, n_draw = [], None, 0
    while True:
        cur0 = s[PC.F_CUR]
        t, act, kp, dr = PC.pre(s, seq, r["chord_token"], r["chord_position"], max_iters, 1 << 30)
        drawn += [False] * (len(seq) - len(drawn))                          # (what pre appended was forced)
        if s[PC.F_DONE]:
            return seq, drawn, s
        if s[PC.F_CUR] != cur0:
            wrong = []
        if act:
            lg = 3.0 * torch.randn(V, generator=g)
            lg[2] += bar_boost
            logits = (lg + table[GC.token_class(int(t)), :V])[1:].clone()
        if not dr:
            continue
        row = logits.clone()
        banned = sorted(set(NO.bans(seq, len(seq), order_ctl)) | set(VC.bans(seq, len(seq), voice_ctl)) |
                        set(DC.bans(seq, len(seq), density_ctl, order_ctl, voice_ctl)))
        if banned:
            row[[i - 1 for i in banned]] = float("-inf")
        probs = DR.apply_sampling(DR.calc_probs(row, r["temperature"]), 32, wrong)
        if not bool(torch.isfinite(probs).all()):
            return None, drawn, s
        if r["temperature"] == 0:
            token = int(probs.argmax())
        else:
            token = DR.draw_inverse_cdf(probs, u[n_draw % len(u)])
            n_draw += 1
        cur = s[PC.F_CUR]
        cp = r["chord_position"][cur] if cur < s[PC.F_NCHORD] else -1
        if cp not in (-1, PC.POS0) and (cp < token < PC.POS0 + PC.POS_RES or token == PC.BAR):
            wrong = []
        elif PC.CHORD_LO <= token <= PC.CHORD_HI:
            wrong.append(token)
        if PC.post(s, seq, r["chord_position"], token, 1 << 30):
            drawn.append(True)


@pytest.fixture(scope="module")
def grammar():
    from commu_amd.generate import event_grammar
    return event_grammar()


def bars_of(seq, start):
    """[(notes, index of the token that closed it or None)] of every bar of seq[start:], the stretch before the first BAR
    included."""
    out, n = [], 0
    for i in range(start, len(seq)):
        t = seq[i]
        if t in (1, 2):
            out.append((n, i))
            n = 0
        elif i >= start + 3 and 304 <= t <= 431 and 3 <= seq[i - 1] <= 130 and 131 <= seq[i - 2] <= 194 \
                and 432 <= seq[i - 3] <= 559:
            n += 1
    out.append((n, None))
    return out


def test_density_violation_has_teeth():
    start = len(CTX)
    short = CTX + note(0) + note(4, 61) + [2] + note(0) + [2] + note(0) + note(4, 61) + [1]
    mask = [False] * start + [True] * (len(short) - start)
    assert DC.density_violation(short, start, 2, 6, mask) == start + 13          # the second BAR closes a bar of one note
    assert DC.density_violation(short, start, 1, 6, mask) is None
    forced = list(mask)
    forced[start + 13] = False
    assert DC.density_violation(short, start, 2, 6, forced) is None              # a forced BAR is none
    assert DC.density_violation(short, start, 3, 6, forced) == start + 8         # the stretch before the first BAR is a bar
    forced[start + 8] = False
    assert DC.density_violation(short, start, 3, 6, forced) == len(short) - 1    # the drawn EOS closes a bar of two
    assert DC.density_violation(short, start, 0, 1, mask) == start + 4           # the second note of the first stretch
    forced = list(mask)
    forced[start + 4] = False
    assert DC.density_violation(short, start, 0, 1, forced) == start + 18        # (a note on a forced position is none)
    full = CTX + [2, pos(5), 150, 60, dur(123), 2]
    mask = [False] * start + [False] + [True] * (len(full) - start - 1)
    assert DC.density_violation(full, start, 2, 0, mask, voice_ctl=VC.word(1)) is None      # no position was free
    assert DC.density_violation(full, start, 2, 0, mask) == len(full) - 1


def test_the_upper_bound_ahead_of_a_mid_bar_chord(grammar):
    """The issue's question: what do the forcing rules do when the upper bound closes a bar before a mid-bar chord (position
    cp != 432) was placed?  With C >= hi every position is banned, so the boundary draw is Bar or EOS.  `post` does not append
    either while a chord with cp != 432 is pending: it forces the POSITION cp instead (for a drawn Bar, and for a drawn EOS).
    What follows that forced position is `pre`'s business, and the walk finds the three cases:
      (a) the 60 requests' mid-bar kind (two chords per bar, not F_LENGTH_FIT, the sequence filled): `pre` forces the chord
          behind cp, the pending chord becomes the next bar's (cp = 432), and the Bar drawn next IS appended -- the chord is
          placed, the bar ends one boundary later, and it holds no note more than hi;
      (b) test_voices_host.MID_BAR_FIRST (the first chord inside its bar): the sequence is not filled when the bound is
          reached, so nothing forces the chord: the token after the forced cp is a DRAW, by the grammar a velocity (a note on
          a forced position: it counts, and cannot be prevented) or a chord token, which Q5 rejects;
      (c) test_voices_host.MID_BAR_FIT (F_LENGTH_FIT with a chord inside a bar): `pre` forces a chord only at `Bar, 432`, so
          the same happens at every mid-bar chord.
    In (b) and (c) the bar goes on past hi by notes on the forced position, one per boundary draw, until the rules can place
    the chord or the iteration cap ends the attempt; none of these notes' positions is a draw, so density_violation stays
    None.  That is the voice cap's documented exception ("anything a forced token starts"), met here through the upper bound."""
    start = len(CTX)
    hi = 3
    word = W(0, hi)
    # (a) the mid-bar requests among the 60: every bar within hi, every chord placed
    mid = [r for r in GH.requests(60) if any(p != 432 for p in r["chord_position"])]
    assert len(mid) >= 15
    over_a = 0
    for r in mid:
        seq, drawn, s = walk(r, grammar, 0, 0, word)
        assert seq is not None and DC.density_violation(seq, start, 0, hi, drawn) is None
        over_a += sum(n > hi for n, _ in bars_of(seq, start))
        if s[PC.F_FILLED]:
            # past the first two bars every forced mid-bar position is followed by its forced chord
            second = [i for i, t in enumerate(seq) if t == 2][1]
            for i in range(second, len(seq) - 1):
                if seq[i] == 496 and not drawn[i]:
                    assert 195 <= seq[i + 1] <= 303 and not drawn[i + 1], (r, i, seq)
    # (b), (c): notes on forced positions take a bar past hi; no drawn position does
    over_bc = []
    for r in (VH.MID_BAR_FIRST, VH.MID_BAR_FIT):
        seq, drawn, s = walk(r, grammar, 0, 0, word)
        assert seq is not None and DC.density_violation(seq, start, 0, hi, drawn) is None
        on_forced = sum(1 for i in range(start, len(seq) - 3) if seq[i] == 496 and not drawn[i] and 131 <= seq[i + 1] <= 194)
        over_bc.append((max(n for n, _ in bars_of(seq, start)), on_forced))
    print("upper bound", hi, ": bars over it in the mid-bar requests of the 60:", over_a,
          "; (largest bar, notes on a forced position) in MID_BAR_FIRST, MID_BAR_FIT:", over_bc)
    assert all(most > hi and forced >= most - hi for most, forced in over_bc)


# ------------------------------------------------------------------------------------------------ 4. the reference loop
LO, HI = 2, 6


def tally(gram, density_ctl, voice_ctl):
    """(requests with a violation of (LO, HI), Q12 endings, failures of validate_teacher_forced_sequence, bars outside the
    bounds by any cause) over the 60 requests under the grammar and the note order."""
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, note_order_violation, parse_events
    start = len(CTX)
    broke, q12, invalid, outside = [], [], [], 0
    for r in GH.requests(60):
        seq, drawn, s = walk(r, gram, 0, voice_ctl, density_ctl)
        if seq is None:
            q12.append(r["seed"])
            continue
        assert parse_events(seq, start) is None and note_order_violation(seq, start) is None, (r, seq)
        if DC.density_violation(seq, start, LO, HI, drawn) is not None:
            broke.append(r["seed"])
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
        bars = bars_of(seq, start)                                           # (what precedes the first BAR included)
        outside += sum(1 for n, end in bars if end is not None and not LO <= n <= HI)
    return broke, q12, invalid, outside


@pytest.fixture(scope="module")
def without_the_rule(grammar):
    return tally(grammar, -1, -1)


def test_without_the_rule_the_requests_violate_the_bounds(without_the_rule):
    broke, q12, invalid, outside = without_the_rule
    print("note order only, bounds (%d, %d): requests that violate them:" % (LO, HI), len(broke), "of 60; Q12:", len(q12),
          "; invalid:", len(invalid), "; closed bars outside the bounds:", outside)
    assert len(broke) > 0


def test_the_rule_through_the_reference_loop(grammar, without_the_rule):
    """(LO, HI) = (2, 6) on the 60 requests: density_violation is None for all of them -- what the rule guarantees, not a
    measurement.  The Q12 endings and the sequences validate_teacher_forced_sequence refuses are recorded beside the run
    without the rule (docs/EXPERIMENTS.md 8z), not fixed here."""
    broke, q12, invalid, outside = tally(grammar, W(LO, HI), 0)
    print("with the rule: requests that violate the bounds:", len(broke), "; Q12:", q12, "(without:", without_the_rule[1],
          "); invalid:", invalid, "(without:", without_the_rule[2], "); closed bars outside the bounds:", outside,
          "(without:", without_the_rule[3], ")")
    assert broke == []
