"""The melodic interval on the host: the restatement (tests/interval_contract.py) on hand-written edge cases and against a
brute force on random rows, the refusals of interval_ctl and check_interval, the struct mirrors, set_interval on the
model-less stub, and the rule through the reference loop's restatement on the 60 random-logit requests of
test_grammar_host.  Every test fails on the parent: it has none of the names."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import density_contract as DC
import grammar_contract as GC
import interval_contract as IC
import note_order_contract as NO
import prime_contract as PC
import test_density_host as DH
import test_grammar_host as GH
import test_voices_host as VH
import voices_contract as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 729
CTX = VH.CTX                 # the 12 context tokens every sequence starts with: no BAR, no POSITION, no complete note
W = IC.word
pos, dur = VH.pos, VH.dur


def note(q, pitch=60, d=4):
    return [pos(q), 150, pitch, dur(d)]


def ids(lo, hi):
    """The ids lo .. hi, both included (empty when hi < lo)."""
    return list(range(lo, hi + 1))


# ------------------------------------------------------------------------------------------------ 1. edge cases
# (name, tokens, F_LEN (None: len(tokens)), interval word, the banned ids written out by hand)
EDGE_CASES = [
    ("no_note_at_all", CTX + [2, pos(0), 200], None, W(7, 7, True), []),
    ("only_note_has_beta_2", CTX + note(0) + [2, 2], None, W(7, 7, True), []),
    ("same_note_with_beta_1", CTX + note(0) + [2], None, W(7, 7, True), ids(3, 52) + [60] + ids(68, 130)),
    ("beta_0", CTX + [2] + note(0), None, W(7, 7), ids(3, 52) + ids(68, 130)),
    ("pitch_without_duration_is_no_reference", CTX + [2] + note(0) + [pos(8), 150, 90], None, W(2, 2),
     ids(3, 57) + ids(63, 130)),
    ("position_chord_pair_is_no_reference", CTX + [2] + note(0) + [pos(8), 200], None, W(2, 2), ids(3, 57) + ids(63, 130)),
    ("the_last_of_two_notes", CTX + [2] + note(0, 40) + note(4, 100), None, W(1, 1, True), ids(3, 98) + [100] + ids(102, 130)),
    ("beta_1_behind_a_beta_2", CTX + note(0, 40) + [2] + note(0, 100) + [2], None, W(1, 1), ids(3, 98) + ids(102, 130)),
    ("newer_note_two_bars_back_none_nearer", CTX + note(0, 40) + [2] + note(0, 100) + [2, 2], None, W(1, 1, True), []),
    ("q_3", CTX + [2] + note(0, 3), None, W(5, 5, True), [3] + ids(9, 130)),
    ("q_130", CTX + [2] + note(0, 130), None, W(5, 5, True), ids(3, 124) + [130]),
    ("q_plus_up_is_130", CTX + [2] + note(0, 123), None, W(7, 0), []),
    ("q_plus_up_is_129", CTX + [2] + note(0, 122), None, W(7, 0), [130]),
    ("q_plus_up_past_130", CTX + [2] + note(0, 100), None, W(127, 0), []),
    ("q_minus_down_is_3", CTX + [2] + note(0, 10), None, W(0, 7), []),
    ("q_minus_down_is_4", CTX + [2] + note(0, 11), None, W(0, 7), [3]),
    ("q_minus_down_below_3", CTX + [2] + note(0, 10), None, W(0, 127), []),
    ("up_alone", CTX + [2] + note(0), None, W(7), ids(68, 130)),
    ("down_alone", CTX + [2] + note(0), None, W(0, 7), ids(3, 52)),
    ("u_alone", CTX + [2] + note(0), None, W(0, 0, True), [60]),
    ("word_0_bans_nothing", CTX + [2] + note(0), None, 0, []),
    ("off", CTX + [2] + note(0), None, -1, []),
    ("F_LEN_cuts_the_last_note", CTX + [2] + note(0, 40) + note(4, 100), len(CTX) + 8, W(1, 1), ids(3, 38) + ids(42, 130)),
    ("F_LEN_cuts_the_duration", CTX + [2] + note(0, 40), len(CTX) + 4, W(1, 1, True), []),
    ("F_LEN_0", note(0), 0, W(1, 1, True), []),
    ("F_LEN_3", note(0), 3, W(1, 1, True), []),
    ("F_LEN_4", note(0), 4, W(1, 1, True), ids(3, 58) + [60] + ids(62, 130)),
]


@pytest.mark.parametrize("name, tokens, length, ctl, want", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_bans_on_hand_written_cases(name, tokens, length, ctl, want):
    from commu_amd.midi_generator.midi_inferrer import interval_bans
    n = len(tokens) if length is None else length
    assert IC.bans(tokens, n, ctl) == sorted(want)
    assert sorted(interval_bans(tokens[:n], ctl)) == sorted(want)          # (the package's checker: the same rule)


def brute_bans(tokens, length, ctl):
    """The rule once more, differently: seq read FORWARD with the bars counted as they come, the last complete group that at
    most one later BAR follows, and the window asked of every pitch id."""
    if ctl < 0:
        return []
    S = [int(t) for t in tokens[:min(max(length, 0), len(tokens))]]
    total = sum(1 for t in S if t == 2)
    bars, q = 0, None
    for i, t in enumerate(S):
        bars += t == 2
        if i >= 3 and 304 <= t <= 431 and 3 <= S[i - 1] <= 130 and 131 <= S[i - 2] <= 194 and 432 <= S[i - 3] <= 559 \
                and total - bars <= 1:
            q = S[i - 1]
    if q is None:
        return []
    up, down, u = ctl % 256, ctl // 256 % 256, ctl // 65536
    return [t for t in range(3, 131) if (up and t - q > up) or (down and q - t > down) or (u and t == q)]


def test_bans_equal_a_brute_force_and_the_packages_on_random_rows():
    from commu_amd.midi_generator.midi_inferrer import interval_bans
    rs = np.random.RandomState(13)
    some = free = 0
    for _ in range(1500):
        s = VH.random_tokens(rs, rs.randint(0, 64))
        ctl = int(rs.choice([-1, 0, W(1), W(0, 1), W(1, 1), W(2, 1, True), W(0, 0, True), W(127, 127), W(7, 7, True)]))
        n = int(rs.randint(-1, len(s) + 3))
        want = brute_bans(s, n, ctl)
        assert IC.bans(s, n, ctl) == want, (s, n, ctl)
        assert sorted(interval_bans(s[:min(max(n, 0), len(s))], ctl)) == want, (s, n, ctl)
        some += bool(want)
        free += ctl > 0 and IC.reference_pitch(s, n) is None
    assert some > 300 and free > 50


def test_interval_violation_is_the_forward_reading_and_has_teeth():
    from commu_amd.midi_generator.midi_inferrer import interval_violation
    start = len(CTX)
    line = CTX + [2] + note(0, 60) + note(4, 67) + note(8, 60) + [2, 2] + note(0, 100) + note(4, 100)
    mask = [False] * start + [True] * (len(line) - start)
    for fn in (IC.interval_violation, interval_violation):
        assert fn(line, start, 7, 7) is None                               # (100 follows two bars: no reference)
        assert fn(line, start, 6, 7) == start + 7                          # 60 -> 67
        assert fn(line, start, 7, 6) == start + 11                         # 67 -> 60
        assert fn(line, start, 7, 0) is None and fn(line, start, 0, 7) is None
        assert fn(line, start, 0, 0, True) == len(line) - 2                # 100 -> 100
        assert fn(line, len(line) - 1, 0, 0, True) is None
        forced = list(mask)
        forced[start + 7] = False
        assert fn(line, start, 6, 7, False, forced) is None                # (a pitch that was not drawn is none)
        assert fn(line, start, 6, 7, False, mask) == start + 7
        assert fn(line, start + 8, 6, 7) is None                           # (before start: a prompt's notes are not checked)
        assert fn(line, start, 0, 0) is None                               # (word 0)


# ------------------------------------------------------------------------------------------------ 2. host surface
def test_interval_ctl_values_and_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import INTERVAL_OFF, interval_ctl, interval_word
    assert INTERVAL_OFF == -1
    assert interval_word() == 0 and interval_word(7) == 7 and interval_word(0, 7) == 1792 and interval_word(7, 7) == 1799
    assert interval_word(7, 7, True) == 67335 and interval_word(no_repeat=True) == 65536 and W(5, 9, True) == interval_word(5, 9, True)
    assert interval_word(127, 127, True) == 127 + 256 * 127 + 65536
    assert interval_ctl(None, 3).tolist() == [-1, -1, -1] and interval_ctl(False, 2).tolist() == [-1, -1]
    assert interval_ctl(1799, 2).tolist() == [1799, 1799] and interval_ctl(np.int64(98175), 1).tolist() == [98175]
    got = interval_ctl([None, False, 0, -1, 1, 256, 65536, 7.0], 8)
    assert got.dtype == np.int32 and got.tolist() == [-1, -1, 0, -1, 1, 256, 65536, 7]
    assert interval_ctl(np.array([0, 1799], dtype=np.int32), 2).tolist() == [0, 1799]
    assert interval_ctl(torch.tensor([3, -1]), 2).tolist() == [3, -1]
    for bad, shown in ((131072, "131072"), (-2, "-2"), (1.5, "1.5"), (float("nan"), "nan"), (True, "True"), ("on", "'on'"),
                       (128, "128"), (W(0, 128), "32768"), (W(7, 255, True), "130823")):
        with pytest.raises(CommuHipError, match=r"interval: .*\[0, 127\].*got " + shown):
            interval_ctl(bad, 4)
    with pytest.raises(CommuHipError, match=r"interval\[2\]: .*got 200000"):
        interval_ctl([0, 1, 200000, 0], 4)
    with pytest.raises(CommuHipError, match=r"interval: 4 values expected \(one per sequence\), got 3"):
        interval_ctl([0, 1, 2], 4)
    with pytest.raises(CommuHipError, match="one value per sequence expected"):
        interval_ctl([[0, 1], [1, 0]], 2)


def test_check_interval_of_the_command_line():
    cli = VH.cli_module()
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(max_leap=None, max_leap_up=None, max_leap_down=None,
                                                        no_repeat_pitch=False, note_order=False), **kw))
    a = ns()
    assert cli.check_interval(a) is None and a.interval_word is None
    a = ns(max_leap="7")
    assert cli.check_interval(a) == 1799 and a.interval_word == 1799 and a.note_order is False      # (implies nothing)
    assert cli.check_interval(ns(max_leap_up="5")) == 5 and cli.check_interval(ns(max_leap_down="9")) == 2304
    assert cli.check_interval(ns(max_leap_up="5", max_leap_down="9", no_repeat_pitch=True)) == W(5, 9, True)
    assert cli.check_interval(ns(no_repeat_pitch=True)) == 65536
    assert cli.check_interval(ns(max_leap="127", no_repeat_pitch=True)) == W(127, 127, True)
    for flag in ("max_leap", "max_leap_up", "max_leap_down"):
        for bad in ("0", "128", "-1", "two", 1.5):
            with pytest.raises(ValueError, match=r"--%s: an integer in \[1, 127\] expected, got %r" % (flag, bad)):
                cli.check_interval(ns(**{flag: bad}))
    with pytest.raises(ValueError, match=r"--max_leap_up 5 cannot be combined with --max_leap 7"):
        cli.check_interval(ns(max_leap="7", max_leap_up="5"))
    with pytest.raises(ValueError, match=r"--max_leap_down 9 cannot be combined with --max_leap 7"):
        cli.check_interval(ns(max_leap="7", max_leap_down="9"))


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *args], capture_output=True,
                          text=True, timeout=120)


def test_cli_refuses_before_a_model_is_loaded(tmp_path):
    out = _cli("--help")
    assert out.returncode == 0
    for flag in ("--max_leap N", "--max_leap_up N", "--max_leap_down N", "--no_repeat_pitch"):
        assert flag in out.stdout
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt"),
              "--num_generate", "1"]
    for args, message in ((["--max_leap", "0"], "--max_leap: an integer in [1, 127] expected, got '0'"),
                          (["--max_leap_up", "128"], "--max_leap_up: an integer in [1, 127] expected, got '128'"),
                          (["--max_leap_down", "x"], "--max_leap_down: an integer in [1, 127] expected, got 'x'"),
                          (["--max_leap", "7", "--max_leap_up", "5"], "--max_leap_up 5 cannot be combined with --max_leap 7")):
        out = _cli(*common, *args)
        assert out.returncode != 0 and message in out.stderr, (args, out.stderr[-400:])
        assert "no_such_checkpoint" not in out.stderr                      # (refused before the checkpoint was looked for)


def test_struct_mirrors_carry_the_field_ahead_of_density_ctl_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    assert C.sizeof(_lib.DecodeArmArgs) == lib.commu_decode_arm_args_bytes()
    assert C.sizeof(_lib.DecodeArmPrimedArgs) == lib.commu_decode_arm_primed_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        names = [n for n, _ in cls._fields_]
        assert names[-5:] == ["interval_ctl", "density_ctl", "order_ctl", "voice_ctl", "cls_ctl"]
        assert _lib.struct_args(cls).interval_ctl is None                  # null unless named
    for cls in (_lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs):
        names = [n for n, _ in cls._fields_]
        assert names[names.index("order_ctl") - 4:names.index("order_ctl")] == ["interval_ctl", "e_interval", "density_ctl",
                                                                              "e_density"]
        assert _lib.struct_args(cls).interval_ctl is None and _lib.struct_args(cls).e_interval is None


def stub(B=4):
    """test_density_host's decoder without a model or a device, with the two attributes this feature adds."""
    dec = DH.stub(B)
    dec.interval_ctl = dec._interval_host = None
    return dec


def test_set_interval_allocates_once_implies_no_other_rule_and_rewrites_in_place():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import CLASS_CTL_DTYPE
    dec = stub()
    dec.set_interval(None)
    dec.set_interval(False, rows=[1])
    dec.set_interval([-1, -1, -1, -1])
    assert dec.interval_ctl is None and dec.density_ctl is None and dec.voice_ctl is None and dec.order_ctl is None
    assert dec.cls_ctl is None and dec.graph == "captured"                 # off on a fresh decoder: nothing
    with pytest.raises(CommuHipError, match="got 200000"):
        dec.set_interval(200000)
    with pytest.raises(CommuHipError, match="got 128"):
        dec.set_interval(128)
    with pytest.raises(CommuHipError, match=r"rows: slot numbers in \[0, 4\) expected"):
        dec.set_interval(W(7, 7), rows=[4])
    assert dec.interval_ctl is None and dec.density_ctl is None and dec.graph == "captured"   # refused before anything changed
    dec.set_interval(W(7, 7), rows=[0, 2])
    assert dec.interval_ctl.tolist() == [1799, -1, 1799, -1] and dec.graph is None and dec.rows_on
    # (the other three words exist, because the one kernel reads them, and are all off: the rule implies none of them)
    assert dec.density_ctl.tolist() == [-1] * 4 and dec.voice_ctl.tolist() == [-1] * 4 and dec.order_ctl.tolist() == [-1] * 4
    assert dec.bias is not None and dec.gram is not None and dec.harm is not None
    assert not bool(dec.gram_on.any()) and not bool(dec.harm_on.any()) and not bool(dec.bias.any())
    rec = dec.cls_ctl.numpy().view(CLASS_CTL_DTYPE).reshape(4, 8)
    assert all(rec[b][c].tolist() == (np.float32(0.95), 32, 1.0, 0) for b in range(4) for c in range(8))     # base triples
    words, density, voices, order = dec.interval_ctl, dec.density_ctl, dec.voice_ctl, dec.order_ctl
    dec.graph = "captured again"
    dec.set_voices(257, rows=[1])
    dec.set_density(DC.word(2, 6), rows=[3])
    dec.set_interval([W(5), W(0, 9, True), 0], rows=[1, 2, 3])
    assert dec.interval_ctl is words and words.tolist() == [1799, 5, 2304 + 65536, 0]
    assert dec.density_ctl is density and density.tolist() == [-1, -1, -1, 1538]
    assert dec.voice_ctl is voices and voices.tolist() == [-1, 257, -1, 0]
    assert dec.order_ctl is order and order.tolist() == [-1, 0, -1, 0] and dec.graph == "captured again"
    with pytest.raises(CommuHipError, match="got 32768"):
        dec.set_interval([0, W(0, 128)], rows=[0, 1])
    assert words.tolist() == [1799, 5, 2304 + 65536, 0]                    # (a refused call leaves every word)
    dec.set_interval(None)
    assert words.tolist() == [-1] * 4 and density.tolist() == [-1, -1, -1, 1538] and voices.tolist() == [-1, 257, -1, 0]
    assert dec.graph == "captured again"
    dec.rearm(3, interval=W(7, 7, True))
    assert words.tolist() == [-1, -1, -1, 67335] and dec.graph == "captured again"
    dec.rearm(3)                                                            # (None: the slot keeps its word)
    assert words.tolist() == [-1, -1, -1, 67335]
    dec.rearm(3, interval=False)
    assert dec.interval_ctl is words and words.tolist() == [-1] * 4 and dec.graph == "captured again"


def test_set_interval_on_a_decoder_that_has_the_other_words_keeps_them():
    dec = stub()
    dec.set_density(DC.word(2, 6), rows=[0])
    density, voices, order, cls = dec.density_ctl, dec.voice_ctl, dec.order_ctl, dec.cls_ctl
    dec.graph = "captured"
    dec.set_interval(W(7, 7))
    assert dec.graph is None                                               # (the interval words are new: the graphs go once)
    assert dec.density_ctl is density and dec.voice_ctl is voices and dec.order_ctl is order and dec.cls_ctl is cls
    assert density.tolist() == [1538, -1, -1, -1] and voices.tolist() == [0, -1, -1, -1]
    assert dec.interval_ctl.tolist() == [1799] * 4


# ------------------------------------------------------------------------------------------------ 3. the reference loop
def walk(r, gram, order_ctl, voice_ctl, interval_ctl, max_iters=200):
    """test_density_host.walk with the interval rule among the bans (density off): the forcing loop on the device record's
    restatement (prime_contract.pre / post), one `pre` per iteration, on random logits under the grammar.  Returns (seq,
    drawn mask, record); seq is None when a row had nothing left (the Q12 exit)."""
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
            logits = (lg + table[GC.token_class(int(t)), :V])[1:].clone()
        if not dr:
            continue
        row = logits.clone()
        banned = sorted(set(NO.bans(seq, len(seq), order_ctl)) | set(VC.bans(seq, len(seq), voice_ctl)) |
                        set(IC.bans(seq, len(seq), interval_ctl)))
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


UP, DOWN = 7, 7
SETTINGS = {"note order": (0, -1), "max_voices 1, no re-strike": (0, VC.word(1, True))}


def tally(gram, voice_ctl, interval_ctl):
    """(requests with a drawn leap beyond (UP, DOWN), requests that violate interval_ctl's own rule, Q12 endings, failures of
    validate_teacher_forced_sequence, mean length) over the 60 requests under the grammar and the note order."""
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, interval_violation, note_order_violation, parse_events
    start = len(CTX)
    leaps, broke, q12, invalid, lengths = [], [], [], [], []
    up, down, u = interval_ctl & 255, (interval_ctl >> 8) & 255, (interval_ctl >> 16) & 1
    for r in GH.requests(60):
        seq, drawn, s = walk(r, gram, 0, voice_ctl, interval_ctl)
        if seq is None:
            q12.append(r["seed"])
            continue
        assert parse_events(seq, start) is None and note_order_violation(seq, start) is None, (r, seq)
        lengths.append(len(seq))
        if interval_violation(seq, start, UP, DOWN, False, drawn) is not None:
            leaps.append(r["seed"])
        assert interval_violation(seq, start, UP, DOWN, False, drawn) == IC.interval_violation(seq, start, UP, DOWN, False, drawn)
        if interval_ctl >= 0 and interval_violation(seq, start, up, down, bool(u), drawn) is not None:
            broke.append(r["seed"])
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
    return leaps, broke, q12, invalid, float(np.mean(lengths)) if lengths else 0.0


@pytest.fixture(scope="module")
def without_the_rule(grammar):
    return {name: tally(grammar, voice, -1) for name, (_, voice) in SETTINGS.items()}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_without_the_rule_the_requests_leap(without_the_rule, setting):
    leaps, _, q12, invalid, mean = without_the_rule[setting]
    print("grammar + %s, no interval rule: requests with a drawn leap beyond %d / %d:" % (setting, UP, DOWN), len(leaps),
          "of 60; Q12:", len(q12), "; invalid:", len(invalid), "; mean length: %.1f" % mean)
    assert len(leaps) > 0


@pytest.mark.parametrize("unison", [False, True], ids=["7_7", "7_7_unison"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_rule_through_the_reference_loop(grammar, without_the_rule, setting, unison):
    """Words 7 / 7 and 7 / 7 / unison on the 60 requests: interval_violation is None for all of them and every sequence stays
    parse_events- and note_order_violation-clean (tally asserts it) -- what the rule guarantees.  The Q12 endings and the
    sequences validate_teacher_forced_sequence refuses are no more than without the rule (docs/EXPERIMENTS.md 9a)."""
    base = without_the_rule[setting]
    leaps, broke, q12, invalid, mean = tally(grammar, SETTINGS[setting][1], W(UP, DOWN, unison))
    print("grammar + %s, word %d: leaps beyond %d / %d:" % (setting, W(UP, DOWN, unison), UP, DOWN), len(leaps),
          "; violations of the word:", len(broke), "; Q12:", q12, "(without:", base[2], "); invalid:", len(invalid),
          "(without:", len(base[3]), "); mean length: %.1f (without: %.1f)" % (mean, base[4]))
    assert leaps == [] and broke == []
    assert len(q12) <= len(base[2]) and len(invalid) <= len(base[3])
