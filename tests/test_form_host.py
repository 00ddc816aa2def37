"""Form templates on the host: a drawn bar may replay an earlier bar of its own track (docs/EXPERIMENTS.md 9f).

form_template's forms and refusals, the word and row packing, the struct mirrors, the -22 ladder of the entry points, the
command line's parser, hand-written walks of the rule's plain-Python statement (form_contract, over prime_contract.pre /
post) and the rule through the reference loop on the 60 random-logit requests of test_grammar_host."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import form_contract as FC
import grammar_contract as GC
import note_order_contract as NO
import prime_contract as PC
import test_grammar_host as GH
import test_guide_host as TG
import test_voices_host as VH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 729
CTX = VH.CTX
N0 = len(CTX)
BAR, EOS = 2, 1
RW = FC.row_word


# ------------------------------------------------------------------------------------------------ 1. templates and words
def test_form_template_forms():
    from commu_amd.generate import form_row_fields, form_template, form_word
    rows = form_template("AABA")
    assert rows.dtype == np.uint32 and rows.shape == (4, 4) and not rows[:, 1:].any()
    assert rows[:, 0].tolist() == [0, RW(0), 0, RW(0)]
    assert form_template("ABAB")[:, 0].tolist() == [0, 0, RW(0), RW(1)]
    doc = {"bars": [None, 0, {"of": 0, "transpose": 2}, {"of": 2, "copy": "rhythm"}, {"of": 1, "copy": "all", "transpose": -48}]}
    want = [0, RW(0), RW(0, FC.ALL, 2), RW(2, FC.RHYTHM), RW(1, FC.ALL, -48)]
    assert form_template(doc)[:, 0].tolist() == want
    assert form_template(json.dumps(doc))[:, 0].tolist() == want
    assert form_template('"AABA"')[:, 0].tolist() == rows[:, 0].tolist()
    assert form_template(form_template(doc)) is not None
    # the word and row packing round trip
    for src in (0, 1, 62):
        for copy in ("all", "rhythm"):
            for s in ((0,) if copy == "rhythm" else (-48, -1, 0, 1, 48)):
                w = FC.row_word(src, ("all", "rhythm").index(copy), s)
                assert form_row_fields(w) == (src, copy, s) and FC.fields(w) == (src, ("all", "rhythm").index(copy), s)
                assert 0 < w < 1 << 15
    assert form_row_fields(0) is None and FC.fields(0) is None
    assert form_word(5, 64) == FC.word(5, 64) == 5 + 4096 * 64
    bars64 = {"bars": [None] + [i for i in range(63)]}
    assert form_template(bars64).shape == (64, 4)


def test_form_template_reads_a_file(tmp_path):
    from commu_amd.generate import form_template
    p = tmp_path / "form.json"
    p.write_text(json.dumps({"bars": [None, 0]}))
    assert form_template(str(p))[:, 0].tolist() == [0, RW(0)]
    q = tmp_path / "letters.txt"
    q.write_text("AAB\n")
    assert form_template(str(q))[:, 0].tolist() == [0, RW(0), 0]


@pytest.mark.parametrize("doc, match", [
    ({"bars": [0]}, r"bar 0: \"of\": 0 is not an earlier bar .*bar 0 is always free"),
    ({"bars": [None, 1]}, r"bar 1: \"of\": 1 is not an earlier bar"),
    ({"bars": [None, None, {"of": 5}]}, r"bar 2: \"of\": 5 is not an earlier bar"),
    ({"bars": [None] * 65}, r"1 \.\. 64 bars, got 65"),
    ({"bars": []}, r"1 \.\. 64 bars, got 0"),
    ({"bars": [None, {"of": 0, "transpose": 49}]}, r"bar 1: \"transpose\": semitones in -48 \.\. 48 expected, got 49"),
    ({"bars": [None, {"of": 0, "transpose": 2, "copy": "rhythm"}]}, r"bar 1: \"transpose\": 2 beside \"copy\": \"rhythm\""),
    ({"bars": [None, {"of": 0, "mode": "all"}]}, r"bar 1: unknown key 'mode'"),
    ({"bars": [None, {"of": 0, "copy": "pitch"}]}, r"bar 1: \"copy\""),
    ({"bars": [None, {"copy": "all"}]}, r"bar 1: \"of\""),
    ({"bars": [None, True]}, r"bar 1: null, a bar index"),
    ({"bars": [None], "cycle": 2}, r"letter string or"),
    ("A1", r"letters, JSON text or a readable file"),
    ("{not json", r"not JSON"),
    (np.array([[RW(0), 0, 0, 0]], dtype=np.uint32), r"bar 0: not a row of a form"),
])
def test_form_template_refusals_carry_the_bars_index(doc, match):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import form_template
    with pytest.raises(CommuHipError, match=match):
        form_template(doc)


def test_rhythm_needs_the_grammar_where_the_generator_sees_both():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import _form_needs_grammar, _form_per_slot, form_template
    rh, full = form_template({"bars": [None, {"of": 0, "copy": "rhythm"}]}), form_template("AA")
    _form_needs_grammar([rh, full, None], [0])
    _form_needs_grammar([full], [])
    with pytest.raises(CommuHipError, match=r'"copy": "rhythm" without the event grammar \(sequence 1\)'):
        _form_needs_grammar([rh, rh], [0])
    assert _form_per_slot(None, 3) == [None] * 3 and _form_per_slot(False, 2) == [None] * 2
    assert [None if t is None else t[:, 0].tolist() for t in _form_per_slot(["AA", None, False], 3)] == [[0, RW(0)], None, None]
    with pytest.raises(CommuHipError, match="3 entries expected"):
        _form_per_slot(["AA"], 3)


# ------------------------------------------------------------------------------------------------ 2. structs, entry points
def test_struct_mirrors_carry_the_form_fields_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    assert C.sizeof(_lib.DecodeArmArgs) == lib.commu_decode_arm_args_bytes()
    assert C.sizeof(_lib.DecodeArmPrimedArgs) == lib.commu_decode_arm_primed_args_bytes()
    assert lib.commu_form_state_ints() == FC.NS == 72
    names = [n for n, _ in _lib.DecodeLoopArgs._fields_]
    i = names.index("art_ctl")
    assert names[i - 5:i] == ["form_ctl", "form_table", "form_rows", "form_state", "form_tok"]
    a = _lib.struct_args(_lib.DecodeLoopArgs)
    assert a.form_ctl is None and a.form_table is None and a.form_rows == 0 and a.form_state is None and a.form_tok is None
    assert "form_ctl" not in [n for n, _ in _lib.SampleArgs._fields_]           # (the sampler never hears of the rule)
    for cls in (_lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs):
        names = [n for n, _ in cls._fields_]
        assert names[-4:] == ["form_ctl", "e_form", "form_state", "form_tok"]   # (every other field keeps its place)
        assert _lib.struct_args(cls).form_ctl is None and _lib.struct_args(cls).form_state is None


LOOP_OK = dict(B=1, V=V, ld_seq=64, ld_chord=4, ld_u=4, top_k=32, top_p=1.0)
FORM_OK = dict(form_ctl=1, form_table=1, form_rows=4096, form_state=1, form_tok=1)


@pytest.mark.parametrize("change", [dict(form_table=None), dict(form_state=None), dict(form_tok=None), dict(form_rows=0),
                                    dict(form_rows=4097), dict(form_rows=-1)], ids=lambda c: "%s=%s" % next(iter(c.items())))
def test_the_loop_entry_refuses_a_form_without_what_it_reads(change):
    """-22 before anything is launched (the pointers are made-up addresses that are never dereferenced)."""
    from commu_amd._lib import CommuHipError, DecodeLoopArgs, call, struct_args
    fields = {**LOOP_OK, **FORM_OK, **change}
    fields = {k: (None if v is None else v) for k, v in fields.items()}
    with pytest.raises(CommuHipError, match="-22"):
        call("commu_decode_sample_post_pre", C.byref(struct_args(DecodeLoopArgs, **fields)), None)
    # the complete struct with an empty batch: 0
    assert call("commu_decode_sample_post_pre", C.byref(struct_args(DecodeLoopArgs, **{**LOOP_OK, **FORM_OK, "B": 0})), None) == 0


@pytest.mark.parametrize("missing", ["form_ctl", "form_table", "form_state", "form_tok", "rows0", "rows4097"])
def test_the_stand_alone_stages_refuse_a_form_without_what_it_reads(missing):
    from commu_amd._lib import CommuHipError, call
    f = dict(form_ctl=1, form_table=1, form_rows=4096, form_state=1, form_tok=1)
    if missing.startswith("rows"):
        f["form_rows"] = int(missing[4:])
    else:
        f[missing] = None
    form = (f["form_ctl"], f["form_table"], f["form_rows"], f["form_state"], f["form_tok"])
    with pytest.raises(CommuHipError, match="-22"):
        call("commu_forcing_pre_form", 1, 1, 64, 1, 1, 4, 1, 1, 4, 10, 1, 1, 1, 1, 1, None, 0, None, *form, 1, None)
    with pytest.raises(CommuHipError, match="-22"):
        call("commu_forcing_post_form", 1, 1, 64, 1, 4, 1, 1, 1, None, None, 1, 1, None, None, *form, 1, None)
    # (an empty batch: nothing is looked at)
    assert call("commu_forcing_pre_form", 1, 1, 64, 1, 1, 4, 1, 1, 4, 10, 1, 1, 1, 1, 1, None, 0, None, *form, 0, None) == 0
    assert call("commu_forcing_post_form", 1, 1, 64, 1, 4, 1, 1, 1, None, None, 1, 1, None, None, *form, 0, None) == 0


def stub(B=4):
    """test_guide_host's decoder without a model or a device; the replay state's reset launch is recorded, not made."""
    dec = TG.stub(B)
    dec.resets = []
    dec._form_reset = lambda first, n: dec.resets.append((int(first), int(n)))
    return dec


def test_set_form_allocates_once_rewrites_in_place_and_touches_no_tier():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ForcedDecoder, form_template
    assert ForcedDecoder.form_ctl is None and ForcedDecoder.form_table is None and ForcedDecoder.form_state is None
    dec = stub()
    dec.set_form(None)
    dec.set_form(False, rows=[1])
    dec.set_form([None, False, None, None])
    assert dec.form_ctl is None and dec.form_table is None and dec.form_state is None and dec.form_tok is None
    assert dec.graph == "captured" and dec.resets == []
    with pytest.raises(CommuHipError, match="bar 1"):
        dec.set_form({"bars": [None, 3]})
    with pytest.raises(CommuHipError, match=r"rows: slot numbers in \[0, 4\) expected"):
        dec.set_form("AA", rows=[4])
    many = [{"bars": [None] + [{"of": 0, "transpose": k % 48}] * 62 + [{"of": k // 48}]} for k in range(65)]
    with pytest.raises(CommuHipError, match="more than the table's 4096 rows"):
        stub(65).set_form(many)
    assert dec.form_ctl is None and dec.graph == "captured"                       # refused before anything changed
    dec.set_form("AABA", rows=[0, 2])
    assert dec.form_ctl.tolist() == [FC.word(0, 4), -1, FC.word(0, 4), -1] and dec.graph is None
    assert tuple(dec.form_table.shape) == (4096, 4) and dec.form_table.dtype == torch.int32
    assert tuple(dec.form_state.shape) == (4, FC.NS) and dec.form_tok.tolist() == [-1] * 4 and dec.resets == [(0, 4)]
    assert dec.form_table[:5, 0].tolist() == [0, RW(0), 0, RW(0), 0]
    # (no tier of the sampling step is touched: the rule lives in the forcing stage)
    assert dec.art_ctl is None and dec.onset_ctl is None and dec.order_ctl is None and dec.cls_ctl is None
    assert dec.bias is None and dec.gram is None and not dec.rows_on
    words, table, state = dec.form_ctl, dec.form_table, dec.form_state
    dec.graph = "captured again"
    other = {"bars": [None, {"of": 0, "transpose": 2}]}
    dec.set_form(["AABA", other], rows=[1, 3])                                    # (de-duplicated by bytes; packed behind)
    assert dec.form_ctl is words and words.tolist() == [FC.word(0, 4), FC.word(0, 4), FC.word(0, 4), FC.word(4, 2)]
    assert dec.form_table is table and table[4:6, 0].tolist() == [0, RW(0, 0, 2)] and dec._form_used == 6
    assert dec.form_state is state and dec.graph == "captured again"              # (switching in place: no re-capture)
    dec.rearm(0, form=other)
    assert words.tolist()[0] == FC.word(4, 2) and dec.resets[-1] == (0, 1)
    dec.rearm(0)                                                                  # (None: the slot keeps its word)
    assert words.tolist()[0] == FC.word(4, 2) and dec.resets[-1] == (0, 1) and len(dec.resets) == 3
    dec.rearm(0, form=False)
    assert words.tolist()[0] == -1
    dec.set_form(other)                                                           # (all slots: the table is packed anew)
    assert dec.form_ctl is words and dec.form_table is table and words.tolist() == [FC.word(0, 2)] * 4 and dec._form_used == 2
    assert table[:2, 0].tolist() == form_template(other)[:, 0].tolist()
    dec.set_form(None)
    assert words.tolist() == [-1] * 4 and dec.graph == "captured again"


# ------------------------------------------------------------------------------------------------ 3. the contract by hand
def test_next_group_takes_a_group_that_ends_at_end_minus_one_and_not_one_that_ends_at_end():
    g = [440, 150, 63, 310]
    seq = [BAR, 432, 200] + g + [BAR]
    assert FC.next_group(seq, 1, 7) == 3                # the Duration sits at end - 1
    assert FC.next_group(seq, 1, 6) == -1               # the Duration sits at end: the bar line cut the note
    assert FC.next_group(seq, 4, 7) == -1
    # a Position, Chord pair and a Position, Velocity, Pitch, BAR tail are skipped
    seq = [BAR, 432, 200, 496, 201] + g + [441, 151, 64, BAR]
    assert FC.next_group(seq, 1, len(seq) - 1) == 5
    assert FC.next_group(seq, 9, len(seq) - 1) == -1
    assert FC.fold(3, -1) == 14 and FC.fold(130, 1) == 119 and FC.fold(63, 12) == 75 and FC.fold(3, -48) == 3 + 0 and \
        FC.fold(130, 48) == 3 + 127 - 0 and FC.fold(10, -13) == 3 + 6


# settings: chords of a 4-bar request
ONE = dict(nm=4.0, tok=[200, 201, 202, 203], pos=[432] * 4)                                  # one chord a bar, length_fit
TWO = dict(nm=4.0, tok=list(range(200, 208)), pos=[432, 496] * 4)                            # a mid-bar chord
THREE = dict(nm=4.0, tok=list(range(200, 212)), pos=[432, 464, 496] * 4)                     # two chords inside the bar
LONG = dict(nm=68.0, tok=[200 + i % 100 for i in range(68)], pos=[432] * 68)                 # 68 bars, length_fit
N1, N2, N3 = [440, 150, 63, 310], [450, 151, 65, 312], [460, 152, 70, 305]

WALKS = {
    # name: (setting, the form's bars, the tokens handed out where the loop draws, iterations, what seq holds after CTX)
    "aaba_and_the_forced_eos": (
        ONE, [None, 0, None, 0], [BAR] + N1 + N2 + [BAR] + N3 + [BAR], 80,
        [2, 432, 200] + N1 + N2 + [2, 432, 201] + N1 + N2 + [2, 432, 202] + N3 + [2, 432, 203] + N1 + N2 + [1]),
    "an_empty_source_gives_bar_at_once": (
        ONE, [None, 0, 1, None], [BAR, BAR] + N3 + [BAR], 60,
        [2, 432, 200, 2, 432, 201, 2, 432, 202, 2, 432, 203] + N3 + [1]),
    "a_position_chord_pair_is_skipped_and_a_position_past_the_pending_chord_is_offered_again": (
        TWO, [None, 0], [BAR] + N1 + [500, 500, 160, 80, 320, BAR, EOS], 70,
        [2, 432, 200] + N1 + [496, 201, 500, 160, 80, 320, 2, 432, 202] + N1 + [496, 203, 500, 160, 80, 320, 2, 432, 204]),
    "a_replayed_position_equal_to_the_pending_chords_restarts_the_group": (
        TWO, [None, 0], [BAR, 496, 496, 160, 80, 320, BAR, EOS], 60,
        [2, 432, 200, 496, 201, 496, 160, 80, 320, 2, 432, 202, 496, 203, 496, 160, 80, 320, 2, 432, 204]),
    "bar_with_two_chords_still_inside_the_bar": (
        THREE, [None, 0], [BAR] + N1 + [BAR, BAR, BAR, EOS], 70,
        [2, 432, 200] + N1 + [464, 201, 496, 202, 2, 432, 203] + N1 + [464, 204, 496, 205, 2, 432, 206]),
    "transposition_folds_at_midi_0_and_127": (
        ONE, [None, {"of": 0, "transpose": -1}, {"of": 0, "transpose": 1}, {"of": 1, "transpose": 24}],
        [BAR, 440, 150, 3, 310, 450, 151, 130, 312, BAR], 90,
        [2, 432, 200, 440, 150, 3, 310, 450, 151, 130, 312, 2, 432, 201, 440, 150, 14, 310, 450, 151, 129, 312,
         2, 432, 202, 440, 150, 4, 310, 450, 151, 119, 312, 2, 432, 203, 440, 150, 38, 310, 450, 151, 129, 312, 1]),
    "rhythm_mode_draws_the_pitches": (
        ONE, [None, {"of": 0, "copy": "rhythm"}, None], [BAR] + N1 + N2 + [BAR, 90, 91, BAR, BAR], 70,
        [2, 432, 200] + N1 + N2 + [2, 432, 201, 440, 150, 90, 310, 450, 151, 91, 312, 2, 432, 202, 2, 432, 203, 1]),
    "a_source_that_is_itself_a_replay": (
        ONE, [None, 0, {"of": 1, "transpose": 2}, 2], [BAR] + N1 + [BAR], 80,
        [2, 432, 200] + N1 + [2, 432, 201] + N1 + [2, 432, 202, 440, 150, 65, 310, 2, 432, 203, 440, 150, 65, 310, 1]),
}


def rows_of_form(form):
    from commu_amd.generate import form_template
    return [int(w) for w in form_template(form)[:, 0]]


def rows_of(bars):
    return rows_of_form({"bars": bars})


def drive(setting, words, script, iters, base=0, table=None, ld_seq=1 << 30, snapshots=None):
    """The loop on the contract with no model: one `pre` per iteration; where it draws, the next token of `script` (taken in
    a cycle) is the draw.  words: the form's row words.  Returns (record, state, seq, drawn mask, draws made)."""
    s = PC.initial_record(len(GH.META), len(setting["tok"]), setting["nm"])
    seq = list(CTX)
    st = FC.initial_state(seq)
    table = [[w, 0, 0, 0] for w in words] if table is None else table
    ctl = FC.word(base, len(words)) if words else -1
    drawn, n = [False] * len(seq), 0
    for _ in range(iters):
        t, act, kp, dr, ft = FC.pre(s, st, seq, setting["tok"], setting["pos"], 1 << 30, ld_seq, ctl, table)
        drawn += [False] * (len(seq) - len(drawn))
        tok = None
        if dr:
            tok = script[n % len(script)]
            n += 1
        if snapshots is not None:
            snapshots.append(("pre", list(s), list(st), list(seq), (t, act, kp, dr, ft)))
        if dr or ft >= 0:
            if FC.post(s, st, seq, setting["pos"], ft if ft >= 0 else tok, ld_seq, ctl, table):
                drawn.append(bool(dr))
        if snapshots is not None:
            snapshots.append(("post", list(s), list(st), list(seq), tok))
    return s, st, seq, drawn, n


@pytest.mark.parametrize("name", list(WALKS))
def test_walks_written_out_by_hand(name):
    from commu_amd.generate import form_violation
    setting, bars, script, iters, want = WALKS[name]
    words = rows_of(bars)
    s, st, seq, drawn, n = drive(setting, words, script, iters)
    # (a walk that does not end by EOS goes on drawing from the script: what is written out is how it starts)
    assert (seq[N0:] if want[-1] == EOS else seq[N0:N0 + len(want)]) == want, (seq[N0:], want)
    assert s[PC.F_NBAR] == seq.count(BAR) and st[FC.BAR_AT:FC.BAR_AT + seq.count(BAR)] == [i for i, t in enumerate(seq) if t == BAR]
    assert s[PC.F_NDRAW] == n                                               # a replay token consumes no variate
    assert FC.form_violation(seq, N0, words, drawn) is None and form_violation(seq, N0, {"bars": bars}, drawn) is None
    # (and the same walk without the rule is another sequence)
    assert drive(setting, [], script, iters)[2] != seq


def test_walk_details():
    """What the table above does not show: the draws made, and the offers that were rejected."""
    setting, bars, script, iters, _ = WALKS["aaba_and_the_forced_eos"]
    s, st, seq, drawn, n = drive(setting, rows_of(bars), script, iters)
    assert n == len(script) and s[PC.F_DONE] == 1 and seq[-1] == EOS
    assert [seq[i] for i, d in enumerate(drawn) if d] == script            # bars 1 and 3 hold no drawn token
    # rhythm mode: the two pitches are the only draws of the replay bar
    setting, bars, script, iters, _ = WALKS["rhythm_mode_draws_the_pitches"]
    s, st, seq, drawn, n = drive(setting, rows_of(bars), script, iters)
    b1 = [i for i, t in enumerate(seq) if t == BAR][1]
    assert [seq[i] for i in range(b1 + 1, b1 + 11) if drawn[i]] == [90, 91]
    # the position past the pending chord: offered, rejected (the chord's position is forced), offered again
    name = "a_position_chord_pair_is_skipped_and_a_position_past_the_pending_chord_is_offered_again"
    setting, bars, script, iters, _ = WALKS[name]
    snaps = []
    drive(setting, rows_of(bars), script, iters, snapshots=snaps)
    offers = [x[4][4] for x in snaps if x[0] == "pre" and x[4][4] >= 0]
    assert offers.count(500) == 2 and offers.count(BAR) == 1
    # BAR with two chords inside the bar: offered three times
    setting, bars, script, iters, _ = WALKS["bar_with_two_chords_still_inside_the_bar"]
    snaps = []
    drive(setting, rows_of(bars), script, iters, snapshots=snaps)
    assert [x[4][4] for x in snaps if x[0] == "pre" and x[4][4] >= 0].count(BAR) == 3


LONG_WALKS = {"one_note_a_bar": ([BAR] + N1 + [BAR] + N3, 700, N1), "empty_bars": ([BAR, BAR] + N3, 360, [])}


@pytest.mark.parametrize("name", list(LONG_WALKS))
def test_a_65th_bar_is_free_and_bar_at_holds_64(name):
    """Bars 1 .. 63 replay bar 0; the first free bar after them (the 65th of the sequence) takes the script's N3."""
    script, iters, note = LONG_WALKS[name]
    s, st, seq, drawn, n = drive(LONG, rows_of([None] + [0] * 63), script, iters)
    at = [i for i, t in enumerate(seq) if t == BAR]
    assert len(at) >= 66
    for i in range(1, 64):
        assert seq[at[i] + 3:at[i + 1]] == note, i
    assert seq[at[64] + 3:at[65]] == N3                  # bar 64 is the 65th: free, the draws go in
    assert st[FC.BAR_AT:] == at[:64] and st[FC.ACTIVE] == 0


def test_form_violation_finds_what_breaks_the_form():
    from commu_amd.generate import form_violation
    setting, bars, script, iters, _ = WALKS["aaba_and_the_forced_eos"]
    s, st, seq, drawn, n = drive(setting, rows_of(bars), script, iters)
    at = [i for i, t in enumerate(seq) if t == BAR]
    for checker in (lambda q, d=None: FC.form_violation(q, N0, rows_of(bars), d), lambda q, d=None: form_violation(q, N0, "AABA", d)):
        assert checker(seq) is None and checker(seq, drawn) is None
        bad = list(seq)
        bad[at[1] + 5] += 1                              # a pitch of bar 1
        assert checker(bad)[:2] == (1, 0)
        bad = list(seq)
        del bad[at[3] + 3:at[3] + 7]                     # bar 3 lacks a group
        assert checker(bad)[:2] == (3, 0)
        d = list(drawn)
        d[at[1] + 4] = True                              # a replayed velocity that claims to be drawn
        assert checker(seq, d)[:2] == (1, 0)
        assert checker(seq[:at[3] + 6]) is None          # bar 3 is not closed: not judged
    bad = list(seq)
    bad[at[1] + 5] += 1
    assert form_violation(bad, at[1], "AABA")[:2] == (1, 0)
    assert form_violation(bad, at[1] + 1, "AABA") is None          # (bar 1 was opened inside the prompt: free, not judged)
    assert form_violation(seq, N0, {"bars": [None, {"of": 0, "copy": "rhythm"}]}) is None


# ------------------------------------------------------------------------------------------------ 4. the command line
def test_check_form_of_the_command_line(tmp_path):
    cli = VH.cli_module()
    ns =lambda **kw: types.SimpleNamespace(**{"form": None, "grammar": True, "parity": False, **kw})
    a = ns()
    assert cli.check_form(a) is None and a.form_doc is None
    a = ns(form="AABA")
    assert json.loads(cli.check_form(a)) == {"bars": [None, 0, None, 0]} and json.loads(a.form_doc) == {"bars": [None, 0, None, 0]}
    doc = {"bars": [None, {"of": 0, "copy": "rhythm"}, {"of": 0, "transpose": -3}]}
    assert json.loads(cli.check_form(ns(form=json.dumps(doc)))) == \
        {"bars": [None, {"of": 0, "copy": "rhythm", "transpose": 0}, {"of": 0, "copy": "all", "transpose": -3}]}
    p = tmp_path / "f.json"
    p.write_text(json.dumps(doc))
    assert cli.check_form(ns(form=str(p))) == cli.check_form(ns(form=json.dumps(doc)))
    with pytest.raises(ValueError, match=r"--form: bar 1: \"of\": 4 is not an earlier bar"):
        cli.check_form(ns(form='{"bars": [null, 4]}'))
    with pytest.raises(ValueError, match=r"--form: .*\"copy\": \"rhythm\" without --grammar"):
        cli.check_form(ns(form=json.dumps(doc), grammar=False))
    parsers = cli.parse_args()
    margs, _ = parsers["model_args"].parse_known_args(["--checkpoint_dir", "x", "--form", "AABA"])
    assert margs.form == "AABA"
    assert parsers["model_args"].parse_known_args(["--checkpoint_dir", "x"])[0].form is None


# ------------------------------------------------------------------------------------------------ 5. the reference loop
def walk(r, gram, words, max_iters=400):
    """test_articulation_host.walk with the form rule: the forcing loop on the device record's restatement, one `pre` per
    iteration, on random logits under the grammar and the note order.  Returns (seq, drawn mask, record); seq is None when a
    row had nothing left (the Q12 exit)."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    gtab = torch.from_numpy(gram)
    seq = list(CTX)
    drawn = [False] * len(seq)
    s = PC.initial_record(len(GH.META), len(r["chord_token"]), r["num_measures"])
    st = FC.initial_state(seq)
    table = [[w, 0, 0, 0] for w in words] if words else [[0, 0, 0, 0]]
    ctl = FC.word(0, len(words)) if words else -1
    u = np.random.RandomState(r["seed"]).random_sample(256)
    wrong, logits, n_draw = [], None, 0
    while True:
        cur0 = s[PC.F_CUR]
        t, act, kp, dr, ft = FC.pre(s, st, seq, r["chord_token"], r["chord_position"], max_iters, 1 << 30, ctl, table)
        drawn += [False] * (len(seq) - len(drawn))
        if s[PC.F_DONE]:
            return seq, drawn, s
        if s[PC.F_CUR] != cur0:
            wrong = []
        if act:
            lg = 3.0 * torch.randn(V, generator=g)
            logits = (lg + gtab[GC.token_class(int(t)), :V])[1:].clone()
        if ft >= 0:
            token = ft
        elif not dr:
            continue
        else:
            assert s[PC.F_NBAR] == seq.count(2)
            row = logits.clone()
            banned = sorted(set(NO.bans(seq, len(seq), 0)))
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
        if FC.post(s, st, seq, r["chord_position"], token, 1 << 30, ctl, table):
            drawn.append(ft < 0)


FORMS = {"free_a_free_a": [None, 0, None, 0],
         "rhythm": [None, {"of": 0, "copy": "rhythm"}, None, {"of": 0, "copy": "rhythm"}],
         "transposed_chain": [None, {"of": 0, "transpose": 2}, {"of": 0, "transpose": 4}, {"of": 2, "transpose": -12}]}


@pytest.fixture(scope="module")
def grammar():
    from commu_amd.generate import event_grammar
    return event_grammar()


def closed_bars(seq):
    """[(start, end)] of the bars of seq that a BAR or the final EOS closes."""
    at = [i for i, t in enumerate(seq) if t == BAR]
    ends = at[1:] + ([len(seq) - 1] if seq[-1] == EOS else [])
    return list(zip(at, ends))


def groups_of(seq, lo, hi):
    out, g = [], lo + 1
    while True:
        g = FC.next_group(seq, g, hi)
        if g < 0:
            return out
        out.append(seq[g:g + 4])
        g += 4


def tally(gram, bars):
    """Over the 60 requests: (requests with a closed replay bar, closed replay bars, violations, parse failures, Q12
    endings, seeds the validators refuse, mean length)."""
    from commu_amd.generate import form_violation
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, parse_events
    words = rows_of(bars) if bars else []
    with_bar, closed, bad, unparsed, q12, invalid, lengths = 0, 0, [], [], [], [], []
    for r in GH.requests(60):
        seq, drawn, s = walk(r, gram, words)
        if seq is None:
            q12.append(r["seed"])
            continue
        lengths.append(len(seq))
        if parse_events(seq, N0) is not None:
            unparsed.append(r["seed"])
        if bars:
            cb = closed_bars(seq)
            n = sum(1 for i in range(min(len(cb), len(words))) if FC.fields(words[i]) is not None)
            closed += n
            with_bar += n > 0
            if FC.form_violation(seq, N0, words, drawn) is not None or form_violation(seq, N0, {"bars": bars}, drawn) is not None:
                bad.append(r["seed"])
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
    return with_bar, closed, bad, unparsed, q12, invalid, float(np.mean(lengths))


@pytest.fixture(scope="module")
def without_the_rule(grammar):
    return tally(grammar, None)


def test_without_the_rule_no_bar_repeats_the_one_before(grammar, without_the_rule):
    """Teeth: of the requests with two closed bars, none has a bar 1 whose note groups equal bar 0's."""
    two = same = 0
    for r in GH.requests(60):
        seq, drawn, s = walk(r, grammar, [])
        if seq is None:
            continue
        cb = closed_bars(seq)
        if len(cb) >= 2:
            two += 1
            same += groups_of(seq, *cb[0]) == groups_of(seq, *cb[1])
    print("without the rule: requests with two closed bars:", two, "of 60; bar 1 equals bar 0 in:", same, "; mean length %.1f" %
          without_the_rule[6], "; invalid:", len(without_the_rule[5]), "; Q12:", len(without_the_rule[4]))
    assert two >= 40 and same == 0


@pytest.mark.parametrize("name", list(FORMS))
def test_the_rule_through_the_reference_loop(grammar, without_the_rule, name):
    """Every closed replay bar matches its source, every sequence parses, no request ends by Q12, the validators refuse no
    sequence they accept without the rule, and at least 40 of the 60 requests close a replay bar (docs/EXPERIMENTS.md 9f)."""
    with_bar, closed, bad, unparsed, q12, invalid, mean = tally(grammar, FORMS[name])
    print("form %s: requests with a closed replay bar:" % name, with_bar, "of 60; closed replay bars:", closed, "; violations:",
          bad, "; unparsed:", unparsed, "; Q12:", q12, "; invalid:", len(invalid), "(without:", len(without_the_rule[5]),
          "); mean length %.1f (without: %.1f)" % (mean, without_the_rule[6]))
    assert bad == []
    assert unparsed == []
    assert q12 == []
    assert set(invalid) <= set(without_the_rule[5])
    assert with_bar >= 40 and closed >= with_bar
