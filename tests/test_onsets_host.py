"""Onset templates on the host: the contract's edge cases written out by hand, a brute-force restatement on random rows,
the host surface (onset_rows, onsets_of, set_onsets on a model-less stub, the command line, the struct mirrors), and the rule
through the reference loop's restatement on the 60 random-logit requests of test_grammar_host.  Every test fails on the
parent: it has none of the names."""
import ctypes as C
import json
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
import onsets_contract as OC
import prime_contract as PC
import test_grammar_host as GH
import test_interval_host as IH
import test_voices_host as VH
import voices_contract as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 729
CTX = VH.CTX                 # the 12 context tokens every sequence starts with: no BAR, no POSITION, no complete note
W = OC.word
pos, dur, note = VH.pos, VH.dur, IH.note
P = list(range(432, 560))


def allbut(*gs):
    """Every position id but those of the grid steps gs."""
    return [t for t in P if t - 432 not in gs]


def bars(nb, tail=()):
    """CTX, then nb bars of one note each, then tail."""
    return CTX + ([2] + note(0)) * nb + list(tail)


# ------------------------------------------------------------------------------------------------ 1. edge cases
WORD_SEAMS = (0, 31, 32, 63, 64, 95, 96, 127)
LANE_SEAMS = tuple(range(0, 128, 12))            # 432 + g is a multiple of 12: the first id of lanes 36 .. 46
TABLE = np.concatenate([
    np.full((1, 4), 0xFFFFFFFF, dtype=np.uint32),                                          # 0: all ones
    np.zeros((1, 4), dtype=np.uint32),                                                     # 1: all zero
    np.stack([OC.row_of([g]) for g in WORD_SEAMS]),                                        # 2 .. 9
    np.stack([OC.row_of([g]) for g in LANE_SEAMS]),                                        # 10 .. 20
    np.stack([OC.row_of([0, 32, 64, 96]), OC.row_of([16, 48]), OC.row_of([8])]),           # 21 .. 23: a cycle of three
    np.stack([OC.row_of([k, 127 - k]) for k in range(64)]),                                # 24 .. 87: a cycle of 64
    np.stack([OC.row_of([0, 4, 8])]),                                                      # 88: low steps only
    np.stack([OC.row_of([0, 64]), OC.row_of([11, 12, 119, 120])]),                         # 89, 90: base + R == n_rows
])
N_ROWS = len(TABLE)
assert N_ROWS == 91
TAIL = [pos(8), 150]          # (an incomplete group behind the last note)
AT40 = note(40, 61)           # (a note at step 40: the note order's floor is 472)

# (name, tokens, F_LEN (None: len(tokens)), density, note-order, voice word, onset word, the position ids the TEMPLATE bans
#  written out by hand, the ids the DENSITY bans under the contract's waiver)
EDGE_CASES = [
    ("off", bars(1), None, -1, -1, -1, -1, [], []),
    ("nb_0_uses_bar_0", CTX + TAIL, None, -1, -1, -1, W(21, 3), allbut(0, 32, 64, 96), []),
    ("nb_1_uses_bar_0", bars(1), None, -1, -1, -1, W(21, 3), allbut(0, 32, 64, 96), []),
    ("nb_2_uses_bar_1", bars(2), None, -1, -1, -1, W(21, 3), allbut(16, 48), []),
    ("nb_R_uses_the_last_row", bars(3), None, -1, -1, -1, W(21, 3), allbut(8), []),
    ("nb_R_plus_1_wraps", bars(4), None, -1, -1, -1, W(21, 3), allbut(0, 32, 64, 96), []),
    ("nb_counts_up_to_F_LEN_only", bars(4), len(bars(2)), -1, -1, -1, W(21, 3), allbut(16, 48), []),
    ("R_1_every_bar", bars(5), None, -1, -1, -1, W(23, 1), allbut(8), []),
    ("R_64_bar_63", bars(64), None, -1, -1, -1, W(24, 64), allbut(63, 64), []),
    ("R_64_bar_64_wraps", bars(65), None, -1, -1, -1, W(24, 64), allbut(0, 127), []),
    ("R_64_bar_5", bars(6), None, -1, -1, -1, W(24, 64), allbut(5, 122), []),
    ("base_plus_R_is_n_rows", bars(2), None, -1, -1, -1, W(89, 2), allbut(11, 12, 119, 120), []),
    ("base_plus_R_is_n_rows_bar_0", bars(1), None, -1, -1, -1, W(89, 2), allbut(0, 64), []),
    ("all_ones", bars(1), None, -1, -1, -1, W(0, 1), [], []),
    ("all_zero_is_a_bar_of_rest", bars(1), None, -1, -1, -1, W(1, 1), list(P), []),
] + [
    ("word_seam_g%d" % g, bars(1), None, -1, -1, -1, W(2 + i, 1), allbut(g), []) for i, g in enumerate(WORD_SEAMS)
] + [
    ("lane_seam_g%d" % g, bars(1), None, -1, -1, -1, W(10 + i, 1), allbut(g), []) for i, g in enumerate(LANE_SEAMS)
] + [
    # every set bit below the note order's floor: template and note order together ban every position
    ("bits_below_the_floor_leave_bar_and_eos", bars(1, AT40), None, -1, 0, -1, W(88, 1), allbut(0, 4, 8), []),
    # the waiver: lower bound 2, one note in the bar, positions [432, 472) banned by the note order
    ("waiver_fires_through_the_template_alone", bars(0, [2] + AT40), None, DC.word(2), 0, 0, W(88, 1), allbut(0, 4, 8), []),
    ("waiver_must_not_fire_step_64_is_left", bars(0, [2] + AT40), None, DC.word(2), 0, 0, W(89, 2), allbut(0, 64), [1, 2]),
    ("waiver_off_word_is_the_parents", bars(0, [2] + AT40), None, DC.word(2), 0, 0, -1, [], [1, 2]),
    ("waiver_all_zero_row_lets_the_bar_end", bars(0, [2] + TAIL), None, DC.word(2), -1, 0, W(1, 1), list(P), []),
    ("lower_bound_with_all_ones_row", bars(0, [2] + TAIL), None, DC.word(2), -1, 0, W(0, 1), [], [1, 2]),
    ("upper_bound_and_template", bars(0, [2] + note(0) + note(4)), None, DC.word(0, 2), 0, 0, W(21, 3),
     allbut(0, 32, 64, 96), list(P)),
]


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_edge_cases_written_out_by_hand(case):
    name, tokens, length, d, o, v, w, want, want_den = case
    n = len(tokens) if length is None else length
    assert OC.bans(tokens, n, w, TABLE) == sorted(want), name
    assert OC.density_bans(tokens, n, w, TABLE, d, o, v) == sorted(want_den), name
    if name == "bits_below_the_floor_leave_bar_and_eos":
        assert (set(want) | set(NO.bans(tokens, n, o))) >= set(P)           # (of the boundary family Bar and EOS remain)
    if w < 0 or name in ("all_ones", "lower_bound_with_all_ones_row"):
        assert OC.density_bans(tokens, n, w, TABLE, d, o, v) == DC.bans(tokens, n, d, o, v)      # the parent's waiver


def brute(tokens, length, word, table, d, o, v):
    """The rule once more, on Python integers: (template bans, density bans)."""
    S = [int(t) for t in tokens[:min(max(length, 0), len(tokens))]]
    mask = (1 << 128) - 1
    if word >= 0:
        base, cyc = word & 4095, word >> 12
        i = max(S.count(2) - 1, 0)
        r = table[base + i % cyc]
        mask = sum(int(r[k]) << (32 * k) for k in range(4))
    tb = [432 + g for g in range(128) if word >= 0 and not (mask >> g) & 1]
    db = set()
    if d >= 0:
        lo, hi = d & 255, d >> 8
        c = DC.count(S, len(S))
        if hi and c >= hi:
            db |= set(P)
        end = DC.position_end(S, len(S), d, o, v) - 432
        if lo and c < lo and (mask >> end) != 0:
            db |= {1, 2}
    return tb, sorted(db)


def test_bans_equal_a_brute_force_on_random_rows():
    rs = np.random.RandomState(17)
    table = rs.randint(0, 2 ** 32, size=(40, 4), dtype=np.uint64).astype(np.uint32)
    table[rs.rand(40) < 0.2] = 0
    table[5] = np.uint32(1) << np.array([3, 0, 0, 0], dtype=np.uint32)
    table[5, 1:] = 0
    some = waived = kept = 0
    for _ in range(1200):
        s = VH.random_tokens(rs, rs.randint(0, 64))
        cyc = int(rs.randint(1, 9))
        word = int(rs.choice([-1, W(int(rs.randint(0, 40 - cyc + 1)), cyc)]))
        d = int(rs.choice([-1, DC.word(2), DC.word(1, 3), DC.word(0, 2)]))
        o, v = int(rs.choice([-1, 0, 1])), int(rs.choice([-1, 0, VC.word(1, True)]))
        n = int(rs.randint(-1, len(s) + 3))
        tb, db = brute(s, n, word, table, d, o, v)
        assert OC.bans(s, n, word, table) == tb, (s, n, word)
        assert OC.density_bans(s, n, word, table, d, o, v) == db, (s, n, word, d, o, v)
        some += bool(tb)
        parent = DC.bans(s, n, d, o, v)
        waived += (1 in parent) and (1 not in db)
        kept += 1 in db
    assert some > 300 and waived > 5 and kept > 50


# ------------------------------------------------------------------------------------------------ 2. host surface
def test_onset_rows_values_and_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ONSETS_OFF, onset_rows, onset_word
    assert ONSETS_OFF == -1 and onset_word(5, 3) == W(5, 3) == 5 + 3 * 4096
    r = onset_rows([[0, 31, 32], [], [127]])
    assert r.dtype == np.uint32 and r.tolist() == [[0x80000001, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0x80000000]]
    assert onset_rows({"bars": [[0, 31, 32], [], [127]]}).tolist() == r.tolist()
    assert onset_rows(r) is not None and onset_rows(r).tolist() == r.tolist()
    assert onset_rows({"grid": 1}).tolist() == [[1, 0, 0, 0]]
    assert onset_rows({"grid": 4}).tolist() == [[1, 1, 1, 1]]
    assert onset_rows({"grid": 16}).tolist() == [[0x01010101] * 4]
    assert onset_rows({"grid": 128}).tolist() == [[0xFFFFFFFF] * 4]
    for n in (1, 2, 4, 8, 16, 32, 64, 128):
        assert np.array_equal(onset_rows({"grid": n})[0], OC.row_of(range(0, 128, 128 // n)))
    assert onset_rows([[g] for g in range(64)]).shape == (64, 4)
    for bad, shown in (({"grid": 3}, "got 3"), ({"grid": 0}, "got 0"), ({"grid": 256}, "got 256"), ({"grid": True}, "got True"),
                       ({"grid": 2.0}, "got 2.0"), ({"steps": 4}, "got the keys"), ([], "got 0"),
                       ([[g] for g in range(65)], "got 65"), ([[128]], "got 128"), ([[-1]], "got -1"), ([[1.5]], "got 1.5"),
                       ([0, 4], "a list of bars"), ("grid", "a list of bars"), (7, "a list of bars"),
                       (np.zeros((65, 4), dtype=np.uint32), r"shape \(65, 4\)"), (np.zeros((2, 3), dtype=np.uint32), "shape")):
        with pytest.raises(CommuHipError, match="onsets: .*" + shown):
            onset_rows(bad)


def test_onsets_of_round_trips_a_hand_built_three_bar_line():
    from commu_amd.generate import onset_rows, onsets_of
    # (a pickup before the first Bar belongs to bar 0; a Position that starts no complete group is no onset)
    line = CTX + note(120, 50) + [2] + note(0, 60) + note(32, 62) + [2] + note(16, 64) + note(16, 67) + [2] + [2] \
        + note(127, 60)
    assert onsets_of(line) == [[0, 32, 120], [16], [], [127]]
    assert onsets_of(line[:-4] + [pos(40), 150]) == [[0, 32, 120], [16], [], []]
    assert onsets_of(line, start=len(CTX) + 4) == [[0, 32], [16], [], [127]]
    inv = onsets_of(line, invert=True)
    assert [sorted(set(range(128)) - set(b)) for b in inv] == [[0, 32, 120], [16], [], [127]]
    rows = onset_rows(onsets_of(line))
    # the line obeys its own template and breaks the inverted one at its first note
    assert OC.onsets_violation(line, len(CTX), rows) is None
    assert OC.onsets_violation(line, len(CTX), onset_rows(inv)) == len(CTX)
    # bar by bar the rows are the rule's: the bar index of every note is OC.bar_index of the prefix before it
    for i, t in enumerate(line):
        if 432 <= t <= 559 and i + 3 < len(line) and 304 <= line[i + 3] <= 431:
            assert t - 432 in onsets_of(line)[OC.bar_index(line, i)]
    assert onsets_of([]) == [[]] and onsets_of(CTX) == [[]]


def test_check_onsets_of_the_command_line(tmp_path):
    cli = VH.cli_module()
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(onsets=None, note_order=False), **kw))
    a = ns()
    assert cli.check_onsets(a) is None and a.onsets_bars is None
    a = ns(onsets='{"grid": 4}')
    assert json.loads(cli.check_onsets(a)) == [[0, 32, 64, 96]] and a.note_order is False      # (implies nothing)
    assert json.loads(cli.check_onsets(ns(onsets="[[0, 8], []]"))) == [[0, 8], []]
    assert json.loads(cli.check_onsets(ns(onsets='{"bars": [[5]]}'))) == [[5]]
    line = CTX + [2] + note(0) + note(32) + [2] + note(16)
    doc = {"from_tokens": line}
    assert json.loads(cli.check_onsets(ns(onsets=json.dumps(doc)))) == [[0, 32], [16]]
    got = json.loads(cli.check_onsets(ns(onsets=json.dumps(dict(doc, invert=True)))))
    assert got == [sorted(set(range(128)) - {0, 32}), sorted(set(range(128)) - {16})]
    f = tmp_path / "t.json"
    f.write_text('{"grid": 2}')
    assert json.loads(cli.check_onsets(ns(onsets=str(f)))) == [[0, 64]]
    for bad, message in (('{"grid": 3}', "--onsets: .*power of two.*got 3"), ("{", "--onsets: not JSON"),
                         (str(tmp_path / "none.json"), "--onsets: JSON text or a readable JSON file expected"),
                         ("[[128]]", "--onsets: bar 0: .*got 128"),
                         ('{"from_tokens": [729]}', r"--onsets: from_tokens: a JSON list of token ids in \[0, 729\)"),
                         ('{"from_tokens": [2], "invert": 1}', "--onsets: invert: true or false expected, got 1"),
                         ('{"from_tokens": [2], "grid": 4}', "--onsets: .*got the key 'grid' as well")):
        with pytest.raises(ValueError, match=message):
            cli.check_onsets(ns(onsets=bad))


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *args], capture_output=True,
                          text=True, timeout=120)


def test_cli_refuses_before_a_model_is_loaded(tmp_path):
    out = _cli("--help")
    assert out.returncode == 0 and "--onsets TEMPLATE" in out.stdout
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt")]
    out = _cli(*common, "--num_generate", "1", "--onsets", '{"grid": 5}')
    assert out.returncode != 0 and "power of two from 1 to 128, got 5" in out.stderr, out.stderr[-400:]
    assert "no_such_checkpoint" not in out.stderr                          # (refused before the checkpoint was looked for)
    req = tmp_path / "requests.json"
    req.write_text(json.dumps([{"num_generate": 1, "onsets": {"grid": 4}}, {"num_generate": 1, "onsets": [[200]]}]))
    out = _cli(*common, "--requests", str(req))
    assert out.returncode != 0 and "request 1: onsets: bar 0:" in out.stderr and "got 200" in out.stderr, out.stderr[-400:]
    assert "no_such_checkpoint" not in out.stderr


def test_struct_mirrors_carry_the_fields_ahead_of_interval_ctl_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    assert C.sizeof(_lib.DecodeArmArgs) == lib.commu_decode_arm_args_bytes()
    assert C.sizeof(_lib.DecodeArmPrimedArgs) == lib.commu_decode_arm_primed_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        names = [n for n, _ in cls._fields_]
        assert names[-8:] == ["onset_ctl", "onset_table", "onset_rows", "interval_ctl", "density_ctl", "order_ctl",
                              "voice_ctl", "cls_ctl"]
        a = _lib.struct_args(cls)
        assert a.onset_ctl is None and a.onset_table is None and a.onset_rows == 0       # null unless named
    for cls in (_lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs):
        names = [n for n, _ in cls._fields_]
        i = names.index("interval_ctl")
        assert names[i - 2:i + 2] == ["onset_ctl", "e_onset", "interval_ctl", "e_interval"]
        assert _lib.struct_args(cls).onset_ctl is None and _lib.struct_args(cls).e_onset is None


def stub(B=4):
    """test_interval_host's decoder without a model or a device; the attributes this feature adds are the class's."""
    return IH.stub(B)


def table_rows(dec, word):
    base, cyc = word & 4095, word >> 12
    return dec.onset_table[base:base + cyc].numpy().view(np.uint32).tolist()


def test_set_onsets_allocates_once_rewrites_in_place_and_keeps_the_other_words():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ForcedDecoder, onset_rows
    assert ForcedDecoder.onset_ctl is None and ForcedDecoder.onset_table is None           # (class-level defaults)
    dec = stub()
    dec.set_onsets(None)
    dec.set_onsets(False, rows=[1])
    dec.set_onsets([None, False, None, None])
    assert dec.onset_ctl is None and dec.onset_table is None and dec.interval_ctl is None and dec.graph == "captured"
    with pytest.raises(CommuHipError, match="power of two"):
        dec.set_onsets({"grid": 3})
    with pytest.raises(CommuHipError, match="got 65"):
        dec.set_onsets([[g] for g in range(65)])
    with pytest.raises(CommuHipError, match=r"rows: slot numbers in \[0, 4\) expected"):
        dec.set_onsets({"grid": 4}, rows=[4])
    many = [[[g, h] for g in range(64)] for h in range(64, 128)] + [[[1], [2]]]             # 64 * 64 + 2 rows
    with pytest.raises(CommuHipError, match="more than the table's 4096 rows"):
        stub(65).set_onsets(many)
    assert dec.onset_ctl is None and dec.interval_ctl is None and dec.graph == "captured"   # refused before anything changed
    dec.set_onsets({"grid": 4}, rows=[0, 2])
    assert dec.onset_ctl.tolist() == [W(0, 1), -1, W(0, 1), -1] and dec.graph is None and dec.rows_on
    assert tuple(dec.onset_table.shape) == (4096, 4) and dec.onset_table.dtype == torch.int32
    assert table_rows(dec, W(0, 1)) == [[1, 1, 1, 1]]
    # (the other four words exist, because the one kernel reads them, and are all off: the rule implies none of them)
    assert dec.interval_ctl.tolist() == [-1] * 4 and dec.density_ctl.tolist() == [-1] * 4
    assert dec.voice_ctl.tolist() == [-1] * 4 and dec.order_ctl.tolist() == [-1] * 4
    assert dec.bias is not None and dec.gram is not None and dec.harm is not None and dec.cls_ctl is not None
    words, table, interval, density = dec.onset_ctl, dec.onset_table, dec.interval_ctl, dec.density_ctl
    dec.graph = "captured again"
    dec.set_interval(IC.word(7, 7), rows=[1])
    dec.set_density(DC.word(2, 6), rows=[3])
    alt = [[0, 64], [32, 96]]
    dec.set_onsets([alt, {"grid": 4}, alt], rows=[1, 2, 3])
    # (packed behind the first template; the same template, by its bytes, is stored once)
    assert dec.onset_ctl is words and words.tolist() == [W(0, 1), W(1, 2), W(0, 1), W(1, 2)]
    assert dec.onset_table is table and table_rows(dec, W(1, 2)) == onset_rows(alt).tolist() and dec._onset_used == 3
    assert dec.interval_ctl is interval and interval.tolist() == [-1, 1799, -1, -1]
    assert dec.density_ctl is density and density.tolist() == [-1, -1, -1, 1538] and dec.graph == "captured again"
    with pytest.raises(CommuHipError, match="got 128"):
        dec.set_onsets([alt, [[128]]], rows=[0, 1])
    assert words.tolist() == [W(0, 1), W(1, 2), W(0, 1), W(1, 2)]          # (a refused call leaves every word)
    dec.rearm(0, onsets=[[5]])
    assert words.tolist() == [W(3, 1), W(1, 2), W(0, 1), W(1, 2)] and table_rows(dec, W(3, 1)) == [[32, 0, 0, 0]]
    dec.rearm(0)                                                            # (None: the slot keeps its word)
    assert words.tolist()[0] == W(3, 1)
    dec.rearm(0, onsets=False)
    assert words.tolist() == [-1, W(1, 2), W(0, 1), W(1, 2)]
    dec.set_onsets(alt)                                                     # (all slots: the table is packed anew)
    assert dec.onset_ctl is words and dec.onset_table is table and words.tolist() == [W(0, 2)] * 4 and dec._onset_used == 2
    assert table_rows(dec, W(0, 2)) == onset_rows(alt).tolist()
    dec.set_onsets(None)
    assert words.tolist() == [-1] * 4 and interval.tolist() == [-1, 1799, -1, -1] and dec.graph == "captured again"


# ------------------------------------------------------------------------------------------------ 3. the reference loop
def walk(r, gram, order_ctl, voice_ctl, density_ctl, onset_ctl, table, max_iters=200):
    """test_interval_host.walk with the template among the bans and the density under the contract's waiver: the forcing
    loop on the device record's restatement (prime_contract.pre / post), one `pre` per iteration, on random logits under the
    grammar.  Returns (seq, drawn mask, record); seq is None when a row had nothing left (the Q12 exit)."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    gtab = torch.from_numpy(gram)
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
            logits = (lg + gtab[GC.token_class(int(t)), :V])[1:].clone()
        if not dr:
            continue
        assert s[PC.F_NBAR] == seq.count(2)                                 # (what the kernel takes the bar index from)
        row = logits.clone()
        n = len(seq)
        banned = sorted(set(NO.bans(seq, n, order_ctl)) | set(VC.bans(seq, n, voice_ctl)) |
                        set(OC.bans(seq, n, onset_ctl, table)) |
                        set(OC.density_bans(seq, n, onset_ctl, table, density_ctl, order_ctl, voice_ctl)))
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


def rows_of(x):
    from commu_amd.generate import onset_rows
    return onset_rows(x)


GRID16 = {"grid": 16}
ALTERNATING = [[0, 16, 32, 48, 64, 80, 96, 112], [8, 24, 40, 56, 72, 88, 104, 120]]
SETTINGS = {"note order": (0, -1), "max_voices 1": (0, VC.word(1))}


def tally(gram, voice_ctl, template, check, density_ctl=-1):
    """(requests with a drawn onset off `check`, Q12 endings, failures of validate_teacher_forced_sequence, mean length)
    over the 60 requests under the grammar and the note order, decoded under `template` (None: off)."""
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, note_order_violation, parse_events
    start = len(CTX)
    table = None if template is None else rows_of(template)
    word = -1 if template is None else W(0, len(table))
    off, q12, invalid, lengths = [], [], [], []
    for r in GH.requests(60):
        seq, drawn, s = walk(r, gram, 0, voice_ctl, density_ctl, word, table)
        if seq is None:
            q12.append(r["seed"])
            continue
        assert parse_events(seq, start) is None and note_order_violation(seq, start) is None, (r, seq)
        lengths.append(len(seq))
        if OC.onsets_violation(seq, start, rows_of(check), drawn) is not None:
            off.append(r["seed"])
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
    return off, q12, invalid, float(np.mean(lengths)) if lengths else 0.0


@pytest.fixture(scope="module")
def without_the_rule(grammar):
    return {name: tally(grammar, voice, None, GRID16) for name, (_, voice) in SETTINGS.items()}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_without_the_rule_the_requests_draw_onsets_off_the_grid(without_the_rule, setting):
    off, q12, invalid, mean = without_the_rule[setting]
    print("grammar + %s, no template: requests with a drawn onset off the 16-grid:" % setting, len(off), "of 60; Q12:",
          len(q12), "; invalid:", len(invalid), "; mean length: %.1f" % mean)
    assert len(off) > 0


@pytest.mark.parametrize("template", ["grid_16", "alternating"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_rule_through_the_reference_loop(grammar, without_the_rule, setting, template):
    """{"grid": 16} and a two-bar alternating template on the 60 requests: no DRAWN position lies outside its bar's row and
    every sequence stays parse_events- and note_order_violation-clean (tally asserts it) -- what the rule guarantees.  No
    request ends by Q12 that did not without the rule, and the validators refuse no sequence they accepted without it
    (docs/EXPERIMENTS.md 9b)."""
    base = without_the_rule[setting]
    tmpl = GRID16 if template == "grid_16" else ALTERNATING
    off, q12, invalid, mean = tally(grammar, SETTINGS[setting][1], tmpl, tmpl)
    print("grammar + %s, template %s: drawn onsets off the template:" % (setting, template), len(off), "; Q12:", q12,
          "(without:", base[1], "); invalid:", len(invalid), "(without:", len(base[2]), "); mean length: %.1f (without: %.1f)"
          % (mean, base[3]))
    assert off == []
    assert set(q12) <= set(base[1])
    assert set(invalid) <= set(base[2])


def test_the_waiver_min_notes_2_with_grid_4_ends_no_request_by_q12(grammar):
    """--min_notes_per_bar 2 with {"grid": 4}: the note order leaves a bar whose last onset is at step 96 no position the
    template allows; without the waiver Bar and EOS stay banned there and the row has nothing left of its family."""
    off, q12, invalid, mean = tally(grammar, 0, {"grid": 4}, {"grid": 4}, density_ctl=DC.word(2))
    print("grammar + note order + min 2 notes per bar + grid 4: off the template:", len(off), "; Q12:", q12, "; invalid:",
          len(invalid), "; mean length: %.1f" % mean)
    assert off == [] and q12 == []
