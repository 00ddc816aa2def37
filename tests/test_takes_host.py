"""Form takes on the host (docs/EXPERIMENTS.md 9h): a bar may replay a bar of a finished sequence the user already has.

form_template's new documents and their refusals, the word packing, today's return values for today's inputs, the struct
mirror, the -22 cases of the entry points, the take buffer's packing on the stub decoder, form_violation over take rows, the
crafted rows of the GPU transition test on the plain-Python contract (take_contract), and keep / redo / repitch through the
reference loop on the 60 random-logit requests of test_grammar_host."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

import form_contract as FC
import grammar_contract as GC
import note_order_contract as NO
import prime_contract as PC
import take_contract as TC
import test_form_host as FH
import test_grammar_host as GH
import test_voices_host as VH

V = 729
CTX, N0 = FH.CTX, FH.N0
BAR, EOS = 2, 1
N1, N2, N3 = FH.N1, FH.N2, FH.N3
RW, TW = FC.row_word, TC.row_word
TAKE = [0, 5, 6, BAR, 432, 200] + N1 + N2 + [BAR, 432, 201, BAR, 432, 202] + N3 + [EOS]        # bars: 2 notes, none, 1 note
SEAMS = (57, 58, 59, 60, 61, 62, 63, 64, 130)
N_RANDOM = 20


def group_starts(buf, lo, hi):
    """The indices of the note groups of buf[lo .. hi), found one behind the other as the rule finds them."""
    return TC.groups_in(buf, lo, hi)


def groups_in(buf, lo, hi):
    return [list(buf[g:g + 4]) for g in group_starts(buf, lo, hi)]


def bar_groups(seq, i):
    """The note groups of closed bar i of seq."""
    lo, hi = FH.closed_bars(seq)[i]
    return groups_in(seq, lo + 1, hi)


# ------------------------------------------------------------------------------------------------ 1. templates and words
def test_take_documents_and_their_rows():
    from commu_amd.generate import FORM, FORM_SRC_MAX, FormTakes, form_document, form_row_fields, form_take_bars, form_template
    assert form_take_bars(TAKE) == [(4, 14), (15, 17), (18, 25)] and form_take_bars([BAR, BAR] + N1) == [(0, 1), (2, 6)]
    assert FORM_SRC_MAX == TC.SRC_MAX == 1 << 18
    doc = {"takes": [TAKE], "bars": [{"take": 0, "of": 2}, None, 0, {"take": None, "of": 0, "copy": "rhythm"},
                                     {"take": 0, "of": 0, "transpose": -7}, {"of": 1, "transpose": 2}]}
    t = form_template(doc)
    assert isinstance(t, FormTakes) and t.dtype == np.uint32 and t.shape == (6, 4) and not t[:, 3].any()
    assert t.tolist() == [[TW(2), 18, 25, 0], [0, 0, 0, 0], [RW(0), 0, 0, 0], [TW(0, FC.RHYTHM), 4, 14, 0],
                          [TW(0, FC.ALL, -7), 4, 14, 0], [RW(1, FC.ALL, 2), 0, 0, 0]]
    assert t.take_of == (0, -1, -1, 0, 0, -1) and [x.tolist() for x in t.takes] == [TAKE] and t.takes[0].dtype == np.int32
    # the word: bit 7 beside today's fields, which read as they always did
    for src in (0, 1, 63):
        for copy, s in (("all", -48), ("all", 0), ("all", 48), ("rhythm", 0)):
            w = TW(src, ("all", "rhythm").index(copy), s)
            assert w & TC.TAKE and form_row_fields(w) == (src, copy, s) and TC.fields(w) == FC.fields(w & ~TC.TAKE) and w < 1 << 15
    # one take given bare, {"from_tokens": ...}, JSON text
    for takes in (TAKE, {"from_tokens": TAKE}, [{"from_tokens": TAKE}]):
        u = form_template({"takes": takes, "bars": [{"take": 0, "of": 1}]})
        assert u.tolist() == [[TW(1), 15, 17, 0]]
    # (an empty source bar is the stretch of its own Bar token: begin == end would be a free row)
    assert form_template({"takes": [[BAR, BAR] + N1], "bars": [{"take": 0, "of": 0}]}).tolist() == [[TW(0), 0, 1, 0]]
    assert form_template(json.dumps(doc)).tolist() == t.tolist()
    assert form_template(t) is t
    # two takes; the round trip through the written-out document
    other = [BAR] + N3 + [BAR] + N1
    two = form_template({"takes": [TAKE, other], "bars": [{"take": 1, "of": 1}, {"take": 0, "of": 0}]})
    assert two.tolist() == [[TW(1), 6, 10, 0], [TW(0), 4, 14, 0]] and two.take_of == (1, 0)
    for f in (t, two):
        back = form_template(form_document(f))
        assert back.tolist() == f.tolist() and back.take_of == f.take_of and FORM.key(back) == FORM.key(f)
    assert form_document(two) == {"takes": [TAKE, other], "bars": [{"take": 1, "of": 1, "copy": "all", "transpose": 0},
                                                                   {"take": 0, "of": 0, "copy": "all", "transpose": 0}]}
    # equal rows over different takes are different forms; a form without takes keeps its key
    a = form_template({"takes": [[BAR] + N1], "bars": [{"take": 0, "of": 0}]})
    b = form_template({"takes": [[BAR] + N2], "bars": [{"take": 0, "of": 0}]})
    assert a.tolist() == b.tolist() and FORM.key(a) != FORM.key(b)
    assert FORM.key(form_template("AABA")) == form_template("AABA").tobytes()


def test_keep_redo_repitch_is_the_full_form_written_short():
    from commu_amd.generate import form_is_rhythm, form_template
    keep = form_template({"keep": {"from_tokens": TAKE}})
    assert keep.tolist() == [[TW(0), 4, 14, 0], [TW(1), 15, 17, 0], [TW(2), 18, 25, 0]] and keep.take_of == (0, 0, 0)
    t = form_template({"keep": {"from_tokens": TAKE}, "redo": [1], "repitch": [2]})
    assert t.tolist() == [[TW(0), 4, 14, 0], [0, 0, 0, 0], [TW(2, FC.RHYTHM), 18, 25, 0]] and t.take_of == (0, -1, 0)
    assert form_is_rhythm(t) and not form_is_rhythm(keep)
    assert form_template({"keep": TAKE, "redo": [0, 1, 2]}).tolist() == [[0] * 4] * 3
    long = [BAR, 440] * 70
    assert form_template({"keep": long}).shape == (64, 4)          # (the take's bars up to 64)


REFUSALS = [
    ({"takes": [TAKE], "bars": [{"take": 1, "of": 0}]}, r"bar 0: \"take\": 1 is not one of the 1 takes"),
    ({"takes": [TAKE, TAKE], "bars": [None, {"take": None, "of": 0}]}, r"bar 1: \"take\": None is not one of the 2 takes"),
    ({"takes": [TAKE], "bars": [None, {"take": 0, "of": 3}]}, r"bar 1: \"of\": 3 is not a bar of take 0 \(it has 3\)"),
    ({"takes": [TAKE], "bars": [{"take": 0}]}, r"bar 0: \"of\": None is not a bar of take 0"),
    ({"takes": [TAKE], "bars": [{"take": 0, "of": 0, "copy": "pitch"}]}, r"bar 0: \"copy\": \"all\" or \"rhythm\""),
    ({"takes": [TAKE], "bars": [{"take": 0, "of": 0, "transpose": 49}]}, r"bar 0: \"transpose\": semitones in -48 .. 48"),
    ({"takes": [TAKE], "bars": [{"take": 0, "of": 0, "copy": "rhythm", "transpose": 1}]}, r"bar 0: \"transpose\": 1 beside"),
    ({"takes": [TAKE], "bars": [{"take": 0, "of": 0, "from": 1}]}, r"bar 0: unknown key 'from'"),
    ({"takes": [TAKE], "bars": [None, 1]}, r"bar 1: \"of\": 1 is not an earlier bar"),
    ({"takes": [[5, 6, 440]], "bars": [None]}, r"take 0: no Bar token"),
    ({"takes": [TAKE, [BAR, 729]], "bars": [None]}, r"take 1: token 729 at index 1 is outside \[0, 729\)"),
    ({"takes": [[BAR, -1]], "bars": [None]}, r"take 0: token -1 at index 1"),
    ({"takes": [[BAR, 1.5]], "bars": [None]}, r"take 0: a list of token ids expected"),
    ({"takes": [], "bars": [None]}, r"\"takes\""),
    ({"takes": [TAKE], "bars": [None] * 65}, r"a form holds 1 .. 64 bars, got 65 \(bar 64 is one too many\)"),
    ({"takes": [[BAR] * ((1 << 18) + 1)], "bars": [None]}, r"take 0: 262145 tokens, the take buffer holds 262144"),
    ({"keep": TAKE, "redo": [1], "repitch": [1]}, r"bar 1: listed in \"redo\" and in \"repitch\""),
    ({"keep": TAKE, "redo": [3]}, r"bar 3: \"redo\" names a bar the take does not have \(it has 3\)"),
    ({"keep": TAKE, "repitch": [-1]}, r"bar -1: \"repitch\" names a bar the take does not have"),
    ({"keep": [5, 6], "redo": []}, r"take 0: no Bar token"),
    ({"keep": TAKE, "redo": 1}, r"\"redo\": a list of bar indices expected"),
]


@pytest.mark.parametrize("doc, match", REFUSALS, ids=[m[:40] for _, m in REFUSALS])
def test_refusals_name_the_bar_or_the_take(doc, match):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import form_template
    with pytest.raises(CommuHipError, match="form: .*" + match):
        form_template(doc)


def test_todays_inputs_give_todays_values():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import FormTakes, form_template
    for x, want in (("AABA", [0, RW(0), 0, RW(0)]), ({"bars": [None, {"of": 0, "copy": "rhythm"}]}, [0, RW(0, FC.RHYTHM)]),
                    ('{"bars": [null, 0, {"of": 1, "transpose": -3}]}', [0, RW(0), RW(1, FC.ALL, -3)])):
        t = form_template(x)
        assert type(t) is np.ndarray and t.dtype == np.uint32 and t.shape == (len(want), 4)
        assert t[:, 0].tolist() == want and not t[:, 1:].any() and not isinstance(t, FormTakes)
        assert type(form_template(t)) is np.ndarray and form_template(t).tolist() == t.tolist()
    for bad, match in (({"bars": [None, 0], "cycle": 2}, "a letter string or"), ({"bars": [None, 3]}, "bar 1"),
                       (np.array([[0, 0, 0, 0], [RW(0), 1, 0, 0]], dtype=np.uint32), "bar 1: not a row of a form"),
                       (np.array([[0, 0, 0, 0], [RW(1), 0, 0, 0]], dtype=np.uint32), "bar 1: not a row of a form"),
                       # (a take row cannot stand without its take)
                       (np.array([[0, 0, 0, 0], [TW(0), 4, 8, 0]], dtype=np.uint32), "bar 1: not a row of a form"),
                       ({"takes": [TAKE], "bars": [None], "cycle": 2}, "a letter string or")):
        with pytest.raises(CommuHipError, match=match):
            form_template(bad)


def test_a_form_with_takes_handed_back_is_checked_against_its_takes():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import FormTakes, form_template
    t = form_template({"takes": [TAKE], "bars": [{"take": 0, "of": 2}, None, 0, {"take": 0, "of": 0}]})
    assert form_template(t) is t
    with pytest.raises(CommuHipError, match="form: 3 rows beside take_of for 4 bars"):
        form_template(t[1:])                                                      # (a slice keeps take_of: no longer a form)

    def edited(i, col, value, take_of=None):
        u = np.array(t).view(FormTakes)
        u.takes, u.take_of = t.takes, t.take_of if take_of is None else take_of
        u[i, col] = value
        return u
    assert form_template(edited(0, 1, 19)).tolist()[0] == [TW(2), 19, 25, 0]      # (inside the take: a form)
    for bad, bar in ((edited(0, 2, len(TAKE) + 1), 0), (edited(3, 1, 14), 3), (edited(3, 2, 3), 3), (edited(1, 1, 5), 1),
                     (edited(0, 3, 7), 0), (edited(2, 0, RW(2)), 2), (edited(0, 0, RW(2) | TC.TAKE, (1, -1, -1, 0)), 0),
                     (edited(1, 0, 0, (0, 0, -1, 0)), 1), (edited(2, 0, RW(0), (0, -1, 0, 0)), 2)):
        with pytest.raises(CommuHipError, match=f"form: bar {bar}: not a row of a form over its takes"):
            form_template(bad)


def test_rhythm_take_rows_need_the_grammar():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import _form_needs_grammar, form_template
    rp = form_template({"keep": TAKE, "repitch": [2]})
    tk = form_template({"takes": [TAKE], "bars": [{"take": 0, "of": 0, "copy": "rhythm"}]})
    for f in (rp, tk):
        _form_needs_grammar([f], [0])
        with pytest.raises(CommuHipError, match='"copy": "rhythm" without the event grammar'):
            _form_needs_grammar([f], [])
    _form_needs_grammar([form_template({"keep": TAKE, "redo": [2]})], [])
    cli = VH.cli_module()
    ns = lambda **kw: types.SimpleNamespace(**{"form": None, "grammar": True, "parity": False, **kw})
    doc = {"keep": {"from_tokens": TAKE}, "redo": [1]}
    full = {"takes": [TAKE], "bars": [{"take": 0, "of": 0, "copy": "all", "transpose": 0}, None,
                                      {"take": 0, "of": 2, "copy": "all", "transpose": 0}]}
    assert json.loads(cli.check_form(ns(form=json.dumps(doc)))) == full            # (written out: the replicas get the tokens)
    assert cli.form_doc(full, "form") == full
    with pytest.raises(ValueError, match=r'--form: .*"copy": "rhythm" without --grammar'):
        cli.check_form(ns(form=json.dumps({"keep": TAKE, "repitch": [0]}), grammar=False))
    with pytest.raises(ValueError, match=r"--form: bar 5: \"redo\" names a bar the take does not have"):
        cli.check_form(ns(form=json.dumps({"keep": TAKE, "redo": [5]})))


# ------------------------------------------------------------------------------------------------ 2. structs, entry points
def test_the_struct_mirror_carries_the_take_buffer_ahead_of_form_ctl():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    assert lib.commu_form_src_max() == 1 << 18
    names = [n for n, _ in _lib.DecodeLoopArgs._fields_]
    i = names.index("form_ctl")
    assert names[i - 2:i] == ["form_src", "form_src_len"] and names[i - 3] == "ld_harm"
    assert names[i:i + 5] == ["form_ctl", "form_table", "form_rows", "form_state", "form_tok"] and names[-1] == "cls_ctl"
    a = _lib.struct_args(_lib.DecodeLoopArgs)
    assert a.form_src is None and a.form_src_len == 0
    for cls in (_lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs):                    # (the arm launches do not know the buffer)
        assert "form_src" not in [n for n, _ in cls._fields_]
        assert C.sizeof(cls) == getattr(lib, "commu_decode_arm%s_args_bytes" % ("_primed" if "Primed" in cls.__name__ else ""))()


LOOP_OK, FORM_OK = FH.LOOP_OK, FH.FORM_OK


@pytest.mark.parametrize("change", [dict(form_src=1, form_src_len=0), dict(form_src=1, form_src_len=-4),
                                    dict(form_src=1, form_src_len=64, form_ctl=None)],
                         ids=["len=0", "len=-4", "without_form_ctl"])
def test_the_loop_entry_refuses_a_take_buffer_it_cannot_read(change):
    """-22 before anything is launched (the pointers are made-up addresses that are never dereferenced)."""
    from commu_amd._lib import CommuHipError, DecodeLoopArgs, call, struct_args
    with pytest.raises(CommuHipError, match="-22"):
        call("commu_decode_sample_post_pre", C.byref(struct_args(DecodeLoopArgs, **{**LOOP_OK, **FORM_OK, **change})), None)
    # a null buffer is legal, and so is the complete struct: an empty batch is 0
    for ok in (dict(), dict(form_src=1, form_src_len=64), dict(form_src=None, form_src_len=64)):
        assert call("commu_decode_sample_post_pre", C.byref(struct_args(DecodeLoopArgs, **{**LOOP_OK, **FORM_OK, **ok, "B": 0})),
                    None) == 0


def test_the_stand_alone_stages_refuse_a_take_buffer_they_cannot_read():
    from commu_amd._lib import CommuHipError, call
    form = (1, 1, 4096, 1, 1)
    pre = lambda *tail: call("commu_forcing_pre_form_src", 1, 1, 64, 1, 1, 4, 1, 1, 4, 10, 1, 1, 1, 1, 1, None, 0, None, *tail, None)
    post = lambda *tail: call("commu_forcing_post_form_src", 1, 1, 64, 1, 4, 1, 1, 1, None, None, 1, 1, None, None, *tail, None)
    for fn in (pre, post):
        for n in (0, -1):
            with pytest.raises(CommuHipError, match="-22"):
                fn(*form, 1, n, 1)
        with pytest.raises(CommuHipError, match="-22"):
            fn(1, None, 4096, 1, 1, 1, 8, 1)                                      # (the form's own refusals stay)
        with pytest.raises(CommuHipError, match="-22"):
            fn(1, 1, 4097, 1, 1, None, 0, 1)
        assert fn(*form, 1, 0, 0) == 0 and fn(*form, None, 0, 0) == 0              # (an empty batch: nothing is looked at)


# ------------------------------------------------------------------------------------------------ 3. packing on the stub
def src_of(dec, n):
    return dec.form_src[:n].tolist()


def test_takes_are_placed_once_rebased_and_reclaimed():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import FORM_SRC_MAX, ForcedDecoder
    assert ForcedDecoder.form_src is None and ForcedDecoder._form_src_used == 0
    other = [BAR] + N3 + [BAR] + N1 + [EOS]
    keep = lambda t, **kw: {"keep": {"from_tokens": t}, **kw}
    big = [BAR] + [440] * (FORM_SRC_MAX - 1)
    dec = FH.stub()
    with pytest.raises(CommuHipError, match=r"form: the distinct takes need %d tokens" % (FORM_SRC_MAX + len(TAKE))):
        dec.set_form([keep(TAKE), keep(big), None, None])                                         # (a decoder without a form yet)
    assert dec.form_ctl is None and dec.form_state is None and dec.form_src is None and dec.graph == "captured"
    dec.set_form("AABA", rows=[0])
    assert dec.form_ctl is not None and dec.form_src is None and dec._form_src_used == 0        # (no take: nothing new)
    dec.graph = "captured"
    with pytest.raises(CommuHipError, match=r"form: the distinct takes need %d tokens, the take buffer holds %d"
                       % (FORM_SRC_MAX + len(TAKE), FORM_SRC_MAX)):
        dec.set_form([keep(TAKE), keep(big)], rows=[1, 2])
    assert dec.form_src is None and dec.graph == "captured" and dec._form_used == 4               # refused before anything changed
    dec.set_form([keep(TAKE, redo=[1]), keep(TAKE, repitch=[1]), keep(other)], rows=[1, 2, 3])
    assert dec.graph is None                                                                      # (dropped once more)
    assert tuple(dec.form_src.shape) == (FORM_SRC_MAX,) and dec.form_src.dtype == torch.int32
    n = len(TAKE)
    assert dec._form_src_used == n + len(other) and src_of(dec, n + len(other) + 1) == TAKE + other + [0]
    assert dec.form_ctl.tolist() == [FC.word(0, 4), FC.word(4, 3), FC.word(7, 3), FC.word(10, 2)]
    rows = dec.form_table[4:12].numpy().view(np.uint32).tolist()
    assert rows == [[TW(0), 4, 14, 0], [0, 0, 0, 0], [TW(2), 18, 25, 0],
                    [TW(0), 4, 14, 0], [TW(1, FC.RHYTHM), 15, 17, 0], [TW(2), 18, 25, 0],
                    [TW(0), n + 1, n + 5, 0], [TW(1), n + 6, n + 11, 0]]                          # (rebased to the take's place)
    src, table = dec.form_src, dec.form_table
    dec.graph = "captured again"
    dec.set_form(keep(other, redo=[0]), rows=[0])                                                 # (its take is there already)
    assert dec._form_src_used == n + len(other) and dec.form_src is src and dec.graph == "captured again"
    assert dec.form_table[12:14].numpy().view(np.uint32).tolist() == [[0, 0, 0, 0], [TW(1), n + 6, n + 11, 0]]
    dec.set_form(keep(other))                                                                     # (all slots: packed anew)
    assert dec._form_src_used == len(other) and src_of(dec, len(other)) == other and dec.form_src is src
    assert dec.form_table is table and dec.form_table[:2].numpy().view(np.uint32).tolist() == [[TW(0), 1, 5, 0], [TW(1), 6, 11, 0]]
    assert dec.form_ctl.tolist() == [FC.word(0, 2)] * 4 and dec.graph == "captured again"
    dec.set_form(None)
    assert dec._form_src_used == 0 and dec.form_ctl.tolist() == [-1] * 4
    with pytest.raises(CommuHipError, match=r"request 1: form: the distinct takes need %d tokens" % (FORM_SRC_MAX + len(TAKE))):
        from commu_amd.generate import FORM, form_template
        dec._pack(FORM, [form_template(keep(TAKE)), form_template(keep(big)), None], fresh=True, label="request")
    assert dec._form_src_used == 0


# ------------------------------------------------------------------------------------------------ 4. the checker
def test_form_violation_judges_a_take_bar_against_its_take():
    from commu_amd.generate import form_template, form_violation
    take = CTX + TAKE[3:]
    doc = {"keep": {"from_tokens": take}, "repitch": [2]}
    t = form_template(doc)
    seq = CTX + [BAR, 432, 200] + N1 + N2 + [BAR, 432, 201, BAR, 432, 202] + N3[:2] + [99] + N3[3:] + [EOS]
    at = [i for i, x in enumerate(seq) if x == BAR]
    drawn = [False] * len(seq)
    drawn[at[2] + 5] = True                                                        # (the pitch of the rhythm bar)
    for checker in (lambda q, d=None: form_violation(q, N0, doc, d),
                    lambda q, d=None: TC.form_violation(q, N0, t.tolist(), take, d)):
        assert checker(seq) is None and checker(seq, drawn) is None
        bad = list(seq)
        bad[at[0] + 5] += 1                                                        # a planted wrong pitch in kept bar 0
        assert checker(bad)[:2] == (0, 0)
        bad = list(seq)
        del bad[at[0] + 7:at[0] + 11]                                              # bar 0 lacks a group
        assert checker(bad)[:2] == (0, 0)
        bad = seq[:at[1] + 3] + N3 + seq[at[1] + 3:]                               # the empty bar holds a note
        assert checker(bad)[:2] == (1, 1)
        bad = list(seq)
        bad[at[2] + 6] += 1                                                        # the rhythm bar's duration
        assert checker(bad)[:2] == (2, 2)
        d = list(drawn)
        d[at[2] + 5] = False                                                       # a rhythm bar's pitch that was not drawn
        assert checker(seq, d)[:2] == (2, 2)
        d = list(drawn)
        d[at[0] + 4] = True                                                        # a kept velocity that claims to be drawn
        assert checker(seq, d)[:2] == (0, 0)
        assert checker(seq[:at[2] + 5]) is None                                    # bar 2 is not closed: not judged
    bad = list(seq)
    bad[at[0] + 5] += 1
    assert form_violation(bad, at[0], doc)[:2] == (0, 0) and form_violation(bad, at[0] + 1, doc) is None      # (not the loop's bar)
    assert len(form_violation(CTX + [BAR, 432, 200] + N3 + [BAR, EOS], N0, doc)) == 3          # (bar, source, reason)


# ------------------------------------------------------------------------------------------------ 5. the crafted rows
def walk_take(name):
    """The sequence a hand-written walk of test_form_host leaves: the take its source bars are moved into."""
    setting, bars, script, iters, _ = FH.WALKS[name]
    return FH.drive(setting, FH.rows_of(bars), script, iters)[2]


def random_script(rs):
    script = []
    for _ in range(24):
        k = rs.rand()
        grp = [432 + int(rs.randint(128)), 131 + int(rs.randint(64)), 3 + int(rs.randint(128)), 304 + int(rs.randint(128))]
        if k < 0.55:
            script += grp
        elif k < 0.75:
            script.append(BAR)
        elif k < 0.85:
            script.append(432 + int(rs.randint(128)))
        elif k < 0.9:
            script.append(195 + int(rs.randint(109)))          # a chord token: rejected, drawn again
        elif k < 0.95:
            script.append(EOS)
        else:
            script += grp[:3] + [BAR]                            # a note the bar line cuts
    return script


def random_take(rs):
    """A token list with bar lines, note groups, lone positions, position-chord pairs and cut notes."""
    out = [5, 6] if rs.rand() < 0.5 else []
    for _ in range(rs.randint(2, 7)):
        out += [BAR, 432, 195 + int(rs.randint(109))]
        for _ in range(rs.randint(0, 5)):
            grp = [432 + int(rs.randint(128)), 131 + int(rs.randint(64)), 3 + int(rs.randint(128)), 304 + int(rs.randint(128))]
            k = rs.rand()
            out += grp if k < 0.7 else grp[:1] if k < 0.8 else [grp[0], 195 + int(rs.randint(109))] if k < 0.9 else grp[:3]
    return out + ([EOS] if rs.rand() < 0.5 else [])


def random_row(rs):
    setting = (FH.ONE, FH.TWO, FH.THREE, FH.LONG)[rs.randint(4)]
    take = random_take(rs)
    n = take.count(BAR)
    bars = []
    for i in range(rs.randint(2, 8)):
        k = rs.randint(6)
        j = int(rs.randint(n))
        own = int(rs.randint(i)) if i else 0
        bars.append(None if k == 0 or (k in (1, 2) and i == 0) else own if k == 1
                    else {"of": own, "transpose": int(rs.randint(-48, 49))} if k == 2
                    else {"take": 0, "of": j} if k == 3 else {"take": 0, "of": j, "copy": "rhythm"} if k == 4
                    else {"take": 0, "of": j, "transpose": int(rs.randint(-48, 49))})
    return setting, {"takes": [take], "bars": bars}, random_script(rs)


def transition_rows():
    """([(name, setting, table rows with begin / end as indices of the buffer, script)], the take buffer): the hand-written
    walks with their source bars moved into a take, bar 0 replaying a take, take and own-past rows in one form, the chunk
    seams, random rows over random forms and random takes, a take that ends the buffer, and planted rows."""
    from commu_amd.generate import form_template
    buf, rows = [7, 7, 7], []                                       # (three tokens first, so that no take lies at 0)

    def add(name, setting, doc, script):
        t = form_template(doc)
        table = np.array(t, dtype=np.int64)
        off = {}
        for i, k in enumerate(t.take_of):
            if k >= 0:
                if k not in off:
                    off[k] = len(buf)
                    buf.extend(t.takes[k].tolist())
                table[i, 1:3] += off[k]
        rows.append((name, setting, table.tolist(), script))

    for name, (setting, bars, script, iters, want) in FH.WALKS.items():
        moved = [b if b is None else {"take": 0, **({"of": b} if isinstance(b, int) else b)} for b in bars]
        add(name, setting, {"takes": [walk_take(name)], "bars": moved}, script)
    two = [BAR, 432, 200] + N1 + N2 + [BAR, 432, 201] + N3 + [EOS]
    add("bar_0_replays_a_take", FH.ONE, {"takes": [two], "bars": [{"take": 0, "of": 0}, None, {"take": 0, "of": 1}]},
        [BAR] + N3 + [BAR])
    add("take_and_own_past_rows_mixed", FH.ONE,
        {"takes": [two], "bars": [{"take": 0, "of": 1}, 0, {"take": 0, "of": 0, "copy": "rhythm"}, {"of": 2, "transpose": 3}]},
        [BAR, 90, 91, BAR])
    for off in SEAMS:
        add(f"group_at_offset_{off}", FH.ONE,
            {"takes": [[BAR] + [440] * off + [441, 150, 63, 310] + [BAR] + N3], "bars": [None, {"take": 0, "of": 0}]},
            [BAR] + N3 + [BAR])
    rs = np.random.RandomState(11)
    for i in range(N_RANDOM):
        add(f"random_{i}", *random_row(rs))
    # the take that ends the buffer: the Duration of its last group is the buffer's last int
    add("the_take_ends_the_buffer", FH.ONE, {"takes": [[BAR, 432, 200] + N1 + N2], "bars": [None, {"take": 0, "of": 0}]},
        [BAR] + N3 + [BAR])
    L = len(buf)
    assert buf[-4:] == N2
    w = TW(0)
    planted = {"begin_and_end_past_the_buffer": [w, L + 5, L + 9, 9],           # active, nothing to read: an empty bar
               "end_past_the_buffer": [w, L - 6, L + 100, 9],                   # clamped: the buffer's last group
               "begin_equals_end": [w, 10, 10, 9],                              # free
               "begin_above_end": [w, 20, 5, 9],                                # free
               "begin_below_zero": [w, 0xFFFFFFFD, 14, 9],                      # clamped to 0
               "end_below_zero": [w, 0xFFFFFFF0, 0xFFFFFFF8, 9]}                # both clamped to 0: an empty bar
    for name, row in planted.items():
        rows.append((name, FH.ONE, [[0, 9, 9, 9], row, [0, 0, 0, 0]], [BAR] + N3 + [BAR] + N2))
    assert len(rows) <= 64
    return rows, buf


def packed(rows):
    """One table for all rows, every form behind the one before it (a row of garbage first, so that no base is 0), and the
    rows' control words."""
    table, ctl = [[FC.row_word(5, 1, 7) | TC.TAKE, 9, 9, 9]], []
    for _, _, t, _ in rows:
        ctl.append(FC.word(len(table), len(t)))
        table += t
    return table, ctl


def check_rows(rows, buf, ref, src):
    """The rows did what they were written for.  ref[b]: seq, and `replayed`, the tokens handed out from a take."""
    by_name = {rows[b][0]: ref[b] for b in range(len(rows))}
    groups = lambda name, i: bar_groups(by_name[name]["seq"], i)
    if src is None:
        # every take row was free: nothing was replayed from a take, and the walks are other sequences
        assert all(r["replayed"] == 0 for r in ref)
        assert groups("bar_0_replays_a_take", 0) == [N3]
        assert by_name["aaba_and_the_forced_eos"]["seq"][N0:] != FH.WALKS["aaba_and_the_forced_eos"][4]
        return 0
    for name, w in FH.WALKS.items():
        want = w[4]
        have = by_name[name]["seq"][N0:]
        assert (have if want[-1] == EOS else have[:len(want)]) == want, name          # (the walk its own past gave)
    assert groups("bar_0_replays_a_take", 0) == [N1, N2] and groups("bar_0_replays_a_take", 1) == [N3]
    assert groups("bar_0_replays_a_take", 2) == [N3]
    assert groups("take_and_own_past_rows_mixed", 0) == [N3] and groups("take_and_own_past_rows_mixed", 1) == [N3]
    assert groups("take_and_own_past_rows_mixed", 2) == [N1[:2] + [90] + N1[3:], N2[:2] + [91] + N2[3:]]
    assert groups("take_and_own_past_rows_mixed", 3) == [N1[:2] + [93] + N1[3:], N2[:2] + [94] + N2[3:]]
    for off in SEAMS:
        assert groups(f"group_at_offset_{off}", 1) == [[441, 150, 63, 310]], off
    assert groups("the_take_ends_the_buffer", 1) == [N1, N2]
    assert groups("begin_and_end_past_the_buffer", 1) == [] and groups("end_below_zero", 1) == []
    assert groups("end_past_the_buffer", 1) == [N2]
    assert groups("begin_equals_end", 1) == [N2] and groups("begin_above_end", 1) == [N2]
    assert groups("begin_below_zero", 1) == groups_in(buf, 0, 14)
    n_take = sum(r["replayed"] for b, r in enumerate(ref) if rows[b][0].startswith("random"))
    assert n_take >= 4 * N_RANDOM
    return n_take


@pytest.mark.parametrize("entry", ["with_the_buffer", "without_it"])
def test_the_crafted_rows_on_the_contract(entry):
    """The rows of the GPU transition test, driven on the contract alone: they do what they were written for, and every
    sequence keeps its form under the contract's checker."""
    rows, buf = transition_rows()
    src = buf if entry == "with_the_buffer" else None
    table, ctl = packed(rows)
    ref = []
    for b, (name, setting, t, script) in enumerate(rows):
        s = PC.initial_record(len(GH.META), len(setting["tok"]), setting["nm"])
        seq = list(CTX)
        st = TC.initial_state(seq)
        n = replayed = 0
        drawn = [False] * len(seq)
        for _ in range(360):
            f = TC.pre(s, st, seq, setting["tok"], setting["pos"], 1 << 30, 448, ctl[b], table, src)
            drawn += [False] * (len(seq) - len(drawn))
            tok = None
            if f[3]:
                tok = script[n % len(script)]
                n += 1
            replayed += f[4] >= 0 and bool(st[TC.ROW] & TC.TAKE)
            if f[3] or f[4] >= 0:
                if TC.post(s, st, seq, setting["pos"], f[4] if f[4] >= 0 else tok, 448, ctl[b], table, src):
                    drawn.append(bool(f[3]))
        assert s[PC.F_NDRAW] == n, name                                           # a replay token consumes no variate
        # (a random script hands a rhythm bar anything for a pitch: only the written rows are judged)
        assert name.startswith("random") or TC.form_violation(seq, N0, t, src, drawn) is None, name
        ref.append(dict(seq=seq, replayed=replayed))
    n_take = check_rows(rows, buf, ref, src)
    print("random rows: tokens replayed from a take:", n_take)


# ------------------------------------------------------------------------------------------------ 6. the reference loop
def walk(r, gram, table, src, max_iters=400):
    """test_form_host.walk with a take buffer: the forcing loop on the contract, one `pre` per iteration, on random logits
    under the grammar and the note order.  table: the form's rows (begin / end: indices of src), empty: no form."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    gtab = torch.from_numpy(gram)
    seq = list(CTX)
    drawn = [False] * len(seq)
    s = PC.initial_record(len(GH.META), len(r["chord_token"]), r["num_measures"])
    st = TC.initial_state(seq)
    ctl = TC.word(0, len(table)) if table else -1
    table = table or [[0, 0, 0, 0]]
    u = np.random.RandomState(r["seed"]).random_sample(256)
    wrong, logits, n_draw = [], None, 0
    while True:
        cur0 = s[PC.F_CUR]
        t, act, kp, dr, ft = TC.pre(s, st, seq, r["chord_token"], r["chord_position"], max_iters, 1 << 30, ctl, table, src)
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
        if TC.post(s, st, seq, r["chord_position"], token, 1 << 30, ctl, table, src):
            drawn.append(ft < 0)


@pytest.fixture(scope="module")
def grammar():
    from commu_amd.generate import event_grammar
    return event_grammar()


@pytest.fixture(scope="module")
def the_takes(grammar):
    """Each request's sequence WITHOUT the rule -- the take of the runs below -- and the seeds the validators refuse."""
    from commu_amd.midi_generator.midi_inferrer import ForcingReport
    takes, invalid = {}, []
    for r in GH.requests(60):
        seq, drawn, s = walk(r, grammar, [], None)
        assert seq is not None
        takes[r["seed"]] = seq
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
    return takes, invalid


def test_the_walk_without_a_form_is_test_form_hosts(grammar, the_takes):
    """A sanity check of this file's own infrastructure, not of the feature (it passes without it): the walk above, given no
    form, is test_form_host.walk, so the takes below are the sequences 9f's tables were made from."""
    for r in GH.requests(6):
        assert FH.walk(r, grammar, [])[0] == the_takes[0][r["seed"]]


@pytest.mark.parametrize("mode", ["redo", "repitch"])
def test_keep_and_redo_through_the_reference_loop(grammar, the_takes, mode):
    """keep with redo: [1] (or repitch: [1]) over each request's own sequence without the rule: every closed kept bar holds
    the take's groups, a repitch bar the take's positions, velocities and durations around drawn pitches; no request ends by
    Q12, every sequence parses, the validators refuse no sequence they accept without the rule; and of the requests that
    close bar 1 more than half have a redone bar that differs from the take's (docs/EXPERIMENTS.md 9h)."""
    from commu_amd.generate import form_template, form_violation
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, parse_events
    takes, invalid0 = the_takes
    q12, unparsed, bad, invalid = [], [], [], []
    kept = closed1 = differs = 0
    for r in GH.requests(60):
        take = takes[r["seed"]]
        if take.count(BAR) < 2:
            continue
        doc = {"keep": {"from_tokens": take}, mode: [1]}
        t = form_template(doc)
        seq, drawn, s = walk(r, grammar, t.tolist(), take)
        if seq is None:
            q12.append(r["seed"])
            continue
        if parse_events(seq, N0) is not None:
            unparsed.append(r["seed"])
        if form_violation(seq, N0, doc, drawn) is not None or TC.form_violation(seq, N0, t.tolist(), take, drawn) is not None:
            bad.append(r["seed"])
        cb, tb = FH.closed_bars(seq), FH.closed_bars(take)
        take_bars = [(a + 1, e) for a, e in zip([i for i, x in enumerate(take) if x == BAR],
                                                [i for i, x in enumerate(take) if x == BAR][1:] + [len(take)])]
        for i in range(min(len(cb), len(take_bars), 64)):
            mine, theirs = bar_groups(seq, i), groups_in(take, *take_bars[i])
            if i != 1:
                assert mine == theirs, (r["seed"], i)                             # group for group
                kept += 1
                continue
            closed1 += 1
            differs += mine != theirs
            if mode == "repitch":
                assert [g[:2] + g[3:] for g in mine] == [g[:2] + g[3:] for g in theirs], r["seed"]
                lo, hi = cb[1]
                assert all([drawn[g + k] for k in range(4)] == [False, False, True, False]
                           for g in group_starts(seq, lo + 1, hi)), r["seed"]
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
    print("%s: kept bars closed and equal to the take's: %d; requests that close bar 1: %d, of which the bar differs from the "
          "take's: %d; violations: %s; unparsed: %s; Q12: %s; invalid: %d (without the rule: %d)"
          % (mode, kept, closed1, differs, bad, unparsed, q12, len(invalid), len(invalid0)))
    assert bad == [] and unparsed == [] and q12 == []
    assert set(invalid) <= set(invalid0)
    assert closed1 >= 40 and kept >= closed1
    assert 2 * differs > closed1
