"""The articulation rule on the host: the contract's edge cases written out by hand, a brute force that enumerates every
duration and checks every occupied step on random rows, the host surface (articulation_rows, set_articulation on a model-less
stub, the command line, the struct mirrors), and the rule through the reference loop's restatement on the 60 random-logit
requests of test_grammar_host against the two-bar guide of test_guide_host.  Every test fails on the parent: it has none of
the names."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import articulation_contract as AC
import grammar_contract as GC
import guide_contract as GD
import note_order_contract as NO
import prime_contract as PC
import test_grammar_host as GH
import test_guide_host as TG
import test_interval_host as IH
import test_voices_host as VH
import voices_contract as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 729
CTX = VH.CTX
W = AC.word
pos, dur, note = VH.pos, VH.dur, IH.note
VEL = list(range(131, 195))
DUR = list(range(304, 432))


def durs_outside(lo, cap):
    """Written out: every DURATION id whose length is not in lo .. cap."""
    return [303 + d for d in range(1, 129) if not lo <= d <= cap]


def vels_but(*bins):
    return [131 + k for k in range(64) if k not in bins]


# ------------------------------------------------------------------------------------------------ 1. edge cases
# the articulation table: row 0 [2, 32] every velocity; row 1 no bounds, bins 0, 31, 32, 63; row 2 dlo 100 only; row 3 free;
# row 4 dhi 1, bin 5 only
TABLE = np.stack([AC.row_of(2, 32), AC.row_of(0, 0, [0, 31, 32, 63]), AC.row_of(100, 0), AC.row_of(), AC.row_of(0, 1, [5])])
# the guide: G, base 0, R = 2, s = 3 (16 cells): bar 0 bans MIDI 60 in cell 3 (steps 24 .. 31) and MIDI 64 in cell 0; bar 1 bans
# MIDI 60 in cell 0 and MIDI 62 in cell 15.  H, base 34, R = 1, s = 0 (128 cells): bans MIDI 0 at step 1, MIDI 31 at step 64,
# MIDI 32 at step 65, MIDI 127 at step 127 and MIDI 63 at step 0 (reached through the wrap only).
ALL = range(128)
GUIDE = np.stack(
    TG._block(ALL, {3: [k for k in ALL if k != 60], 0: [k for k in ALL if k != 64]}, 16)
    + TG._block(ALL, {0: [k for k in ALL if k != 60], 15: [k for k in ALL if k != 62]}, 16)
    + TG._block(ALL, {1: [k for k in ALL if k != 0], 64: [k for k in ALL if k != 31], 65: [k for k in ALL if k != 32],
                      127: [k for k in ALL if k != 127], 0: [k for k in ALL if k != 63]}, 128))
assert len(GUIDE) == 34 + 129
G, H = GD.word(0, 2, 3), GD.word(34, 1, 0)


def open_note(step, midi, nbars=1):
    """CTX, nbars BARs (with a note each but the last), then an open group at `step` whose pitch was just drawn."""
    return CTX + ([2] + note(0)) * (nbars - 1) + [2, pos(step), 150, 3 + midi]


# (name, tokens, F_LEN (None: len), articulation word, guide word, the DURATION ids banned, written out by hand, the VELOCITY
#  ids banned)
EDGE_CASES = [
    ("off", open_note(0, 60), None, -1, G, [], []),
    ("window_2_32", open_note(0, 10), None, W(0, 1), -1, durs_outside(2, 32), []),
    ("free_row_is_the_call_without", open_note(0, 60), None, W(3, 1), G, [], []),
    ("nb_0_uses_row_0", CTX + [pos(0), 150, 13], None, W(0, 2), -1, durs_outside(2, 32), []),
    ("nb_2_uses_row_1", open_note(0, 10, 2), None, W(0, 2), -1, [], vels_but(0, 31, 32, 63)),
    ("nb_3_wraps_to_row_0", open_note(0, 10, 3), None, W(0, 2), -1, durs_outside(2, 32), []),
    ("nb_counts_up_to_F_LEN_only", open_note(0, 10, 3), len(open_note(0, 10, 2)), W(0, 2), -1, [], vels_but(0, 31, 32, 63)),
    ("row_clamped_to_the_last_row", open_note(0, 10), None, W(4000, 1), -1, durs_outside(1, 1), vels_but(5)),
    ("bar_line_a_0", open_note(0, 10), None, W(3, 1, True), -1, [], []),
    ("bar_line_a_96", open_note(96, 10), None, W(3, 1, True), -1, durs_outside(1, 32), []),
    ("bar_line_a_127_cap_1", open_note(127, 10), None, W(3, 1, True), -1, durs_outside(1, 1), []),
    ("bar_line_off_a_127", open_note(127, 10), None, W(3, 1), -1, [], []),
    ("dlo_gives_way_to_the_bar_line", open_note(120, 10), None, W(2, 1, True), -1, durs_outside(8, 8), []),
    ("dlo_100_alone", open_note(0, 10), None, W(2, 1), -1, durs_outside(100, 128), []),
    # the hold term: MIDI 60 from step 0 of bar 0 meets its ban at step 24: f = 24
    ("hold_f_24", open_note(0, 60), None, W(3, 1, False, True), G, durs_outside(1, 24), []),
    ("hold_from_inside_the_banned_cell_f_1", open_note(24, 60), None, W(3, 1, False, True), G, durs_outside(1, 1), []),
    ("hold_step_a_itself_is_not_tested", open_note(31, 60), None, W(3, 1, False, True), G, durs_outside(1, 97), []),
    # (from step 31 the next ban of MIDI 60 is bar 1's cell 0: step 128 = a + 97)
    ("hold_into_the_next_bar", open_note(100, 60), None, W(3, 1, False, True), G, durs_outside(1, 28), []),
    ("hold_next_bar_wraps_R_g_2", open_note(100, 64, 2), None, W(3, 1, False, True), G, durs_outside(1, 28), []),
    # (bar 1 is open: the next bar is block 0 again, whose cell 0 bans MIDI 64)
    ("hold_pitch_never_banned", open_note(0, 61), None, W(3, 1, False, True), G, [], []),
    ("hold_with_window", open_note(0, 60), None, W(0, 1, False, True), G, durs_outside(2, 24), []),
    ("hold_dlo_gives_way", open_note(0, 60), None, W(2, 1, False, True), G, durs_outside(24, 24), []),
    ("hold_switch_off", open_note(0, 60), None, W(3, 1), G, [], []),
    ("hold_guide_word_off", open_note(0, 60), None, W(3, 1, False, True), -1, [], []),
    ("hold_prev_not_a_pitch", CTX + [2, pos(0), 150], None, W(3, 1, False, True), G, [], []),
    ("hold_last_breaker_a_BAR", CTX + [2, 63], None, W(3, 1, True, True), G, [], []),
    ("hold_no_breaker_at_all", CTX + [63], None, W(3, 1, True, True), G, [], []),
    # s = 0: the first clear bit at m = 1, 64, 65, 127; R_g = 1 wraps onto the same block
    ("s0_m_1", open_note(0, 0), None, W(3, 1, False, True), H, durs_outside(1, 1), []),
    ("s0_m_64_seam", open_note(0, 31), None, W(3, 1, False, True), H, durs_outside(1, 64), []),
    ("s0_m_65_seam", open_note(0, 32), None, W(3, 1, False, True), H, durs_outside(1, 65), []),
    ("s0_m_127", open_note(0, 127), None, W(3, 1, False, True), H, durs_outside(1, 127), []),
    ("s0_none_m_128_is_not_tested", open_note(0, 63), None, W(3, 1, False, True), H, [], []),
    ("s0_wraps_onto_the_same_block", open_note(100, 63), None, W(3, 1, False, True), H, durs_outside(1, 28), []),
    # (guide base 60000: every cell row clamps to the table's last row, H's step 127, which bans MIDI 127)
    ("guide_rows_clamped_to_the_last_row", open_note(0, 127), None, W(3, 1, False, True), GD.word(60000, 1, 0),
     durs_outside(1, 1), []),
    ("velocity_bits_0_31_32_63", CTX + [2, pos(0)], None, W(1, 1), -1, [], vels_but(0, 31, 32, 63)),
]


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_edge_cases_written_out_by_hand(case):
    name, tokens, length, w, g, want_dur, want_vel = case
    n = len(tokens) if length is None else length
    assert AC.duration_bans(tokens, n, w, TABLE, g, GUIDE) == sorted(want_dur), name
    assert AC.velocity_bans(tokens, n, w, TABLE) == sorted(want_vel), name
    got = AC.bans(tokens, n, w, TABLE, g, GUIDE)
    assert got == sorted(want_dur + want_vel), name
    assert not set(got) & (set(range(0, 131)) | set(range(195, 304)) | set(range(432, V)))     # (130, 195, 303, 432 untouched)
    assert set(DUR) - set(got), name                                                           # (the window is never empty)


def brute(tokens, length, w, table, g, gtable):
    """The rule once more, by enumeration: a duration d is allowed iff it respects dhi, the bar line and -- checking every
    occupied step a + 1 .. a + d - 1 -- the guide; then the lower bound gives way to the largest allowed."""
    S = [int(t) for t in tokens[:min(max(length, 0), len(tokens))]]
    if w < 0:
        return [], []
    nb = max(S.count(2) - 1, 0)
    row = table[min((w & 4095) + nb % ((w >> 12) & 127), len(table) - 1)]
    vb = [131 + k for k in range(64) if not ((int(row[1]) | int(row[2]) << 32) >> k) & 1]
    dlo, dhi = int(row[0]) & 255, (int(row[0]) >> 8) & 255
    brk = [t for t in S if t == 2 or 432 <= t <= 559]
    a = brk[-1] - 432 if brk and brk[-1] != 2 else None
    q = int(tokens[min(max(length, 1), len(tokens)) - 1])
    k = q - 3 if 3 <= q <= 130 else None

    def banned_at(t):
        base, R, s = g & 65535, (g >> 16) & 127, (g >> 23) & 7
        per = 1 + (128 >> s)
        x, st = (nb, t) if t < 128 else (nb + 1, t - 128)
        r = gtable[min(base + (x % R) * per + 1 + (st >> s), len(gtable) - 1)]
        return not (int(r[k // 32]) >> (k % 32)) & 1

    ok = []
    for d in range(1, 129):
        good = not (dhi and d > dhi)
        good = good and not ((w >> 19) & 1 and a is not None and a + d > 128)
        if good and (w >> 20) & 1 and g >= 0 and a is not None and k is not None:
            good = not any(banned_at(a + m) for m in range(1, min(d, 128)))
        ok.append(good)
    cap = max(d for d in range(1, 129) if all(ok[:d]))          # (the allowed lengths are a prefix: every term is a cap)
    lo = min(max(dlo, 1), cap)
    return [303 + d for d in range(1, 129) if not lo <= d <= cap], vb


def test_bans_equal_a_brute_force_on_random_rows():
    rs = np.random.RandomState(29)
    gtable = rs.randint(0, 2 ** 32, size=(300, 4), dtype=np.uint64).astype(np.uint32)
    gtable[rs.rand(300) < 0.5] = 0xFFFFFFFF
    gtable |= rs.randint(0, 2 ** 32, size=(300, 4), dtype=np.uint64).astype(np.uint32)          # (3 of 4 bits set)
    table = np.zeros((20, 4), dtype=np.uint32)
    for r in table:
        lo, hi = sorted(int(x) for x in rs.randint(0, 129, 2))
        r[:] = AC.row_of(int(rs.choice([0, lo])), int(rs.choice([0, hi])), [k for k in range(64) if rs.rand() < 0.7] or [0])
    held = way = barline = clamped = some_vel = 0
    for _ in range(1500):
        s = VH.random_tokens(rs, rs.randint(1, 64))          # (a row of seq holds a token at least: ld_seq >= 1)
        if rs.rand() < 0.7:
            s = s + [pos(int(rs.randint(0, 128))), 150, int(rs.randint(3, 131))]
        sh = int(rs.randint(0, 8))
        g = int(rs.choice([-1, GD.word(int(rs.randint(0, 300)), int(rs.randint(1, 4)), sh)]))
        base, R = int(rs.randint(0, 24)), int(rs.randint(1, 4))
        w = int(rs.choice([-1, W(base, R, bool(rs.randint(2)), bool(rs.randint(2)))]))
        n = int(rs.randint(-1, len(s) + 2)) if rs.rand() < 0.3 else len(s)
        db, vb = brute(s, n, w, table, g, gtable)
        assert AC.duration_bans(s, n, w, table, g, gtable) == db, (s, n, w, g)
        assert AC.velocity_bans(s, n, w, table) == vb, (s, n, w)
        if w >= 0:
            f = AC.first_ban(s, n, g, gtable)
            lo, cap = AC.window(s, n, w, table, g, gtable)
            held += (w >> 20) & 1 and f is not None and cap == f
            row = AC.open_row(s, n, w, table)
            way += lo < (int(row[0]) & 255)
            barline += (w >> 19) & 1 and AC.start_step(s, n) is not None and cap == 128 - AC.start_step(s, n)
            clamped += base + R > 20
            some_vel += bool(vb)
    assert held > 50 and way > 20 and barline > 50 and clamped > 50 and some_vel > 300, (held, way, barline, clamped, some_vel)


def test_the_checkers_agree_on_a_hand_built_sequence():
    """articulation_violation reads the rule forward; held_into_ban measures the finished notes without it."""
    rows = np.stack([AC.row_of(2, 32)])
    seq = CTX + [2] + note(0, 63, 24) + note(0, 63, 25) + note(100, 63, 28) + note(100, 63, 29) + note(8, 64, 1)
    i0 = len(CTX) + 1
    got = AC.held_into_ban(seq, len(CTX), GUIDE[:34], cells=16)
    assert got == [(i0 + 3, False, False), (i0 + 7, True, False), (i0 + 11, False, False), (i0 + 15, True, True),
                   (i0 + 19, False, False)]
    assert AC.articulation_violation(seq, len(CTX), rows, GUIDE[:34], hold_guide=True) == i0 + 7
    assert AC.articulation_violation(seq, i0 + 8, rows, GUIDE[:34], hold_guide=True) == i0 + 15
    assert AC.articulation_violation(seq, i0 + 8, rows, GUIDE[:34], within_bar=True) == i0 + 15       # (100 + 29 > 128)
    assert AC.articulation_violation(seq, i0 + 16, rows, GUIDE[:34], hold_guide=True) == i0 + 19       # (1 < dlo = 2)
    assert AC.articulation_violation(seq, len(CTX), rows, GUIDE[:34], [t == 304 for t in seq]) == i0 + 19
    assert AC.articulation_violation(seq[:i0 + 16], len(CTX), rows) is None


# ------------------------------------------------------------------------------------------------ 2. host surface
FREE = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]


def test_articulation_rows_values_and_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ARTICULATION_OFF, articulation_rows, articulation_template, articulation_word
    assert ARTICULATION_OFF == -1
    assert articulation_word(5, 3) == W(5, 3) == 5 + 3 * 4096
    assert articulation_word(5, 3, True, True) == W(5, 3, True, True) == 5 + 3 * 4096 + (1 << 19) + (1 << 20)
    assert articulation_word(0, 64, hold_guide=True) == 64 * 4096 + (1 << 20)
    r = articulation_rows({"duration": [2, 16]})
    assert r.dtype == np.uint32 and r.tolist() == [[2 | 16 << 8, 0xFFFFFFFF, 0xFFFFFFFF, 0]]
    assert r.tolist() == [AC.row_of(2, 16).tolist()]
    assert articulation_rows({"duration": [None, 128]}).tolist() == [[128 << 8, 0xFFFFFFFF, 0xFFFFFFFF, 0]]
    assert articulation_rows({"duration": [128, None]}).tolist() == [[128, 0xFFFFFFFF, 0xFFFFFFFF, 0]]
    assert articulation_rows({"hold_guide": True}).tolist() == [FREE]
    # MIDI velocities map to the bins floor(lo / 2) .. ceil(hi / 2), capped at 63
    assert articulation_rows({"velocity": [0, 127]}).tolist() == [FREE]
    assert articulation_rows({"velocity": [63, 65]}).tolist() == [[0, 0x80000000, 3, 0]]      # (bins 31, 32, 33)
    assert articulation_rows({"velocity": [64, 64]}).tolist() == [[0, 0, 1, 0]]
    assert articulation_rows({"velocity": [1, 1]}).tolist() == [[0, 3, 0, 0]]                          # (bins 0 and 1)
    assert articulation_rows({"velocity": [127, 127]}).tolist() == [[0, 0, 0x80000000, 0]]
    full = {"bars": [{"duration": [1, 4]}, None, {"velocity": [100, 127], "duration": [None, 8]}], "within_bar": True}
    rows, w, h = articulation_template(full)
    assert (w, h) == (True, False) and rows.tolist() == [[1 | 4 << 8, 0xFFFFFFFF, 0xFFFFFFFF, 0], FREE,
                                                          [8 << 8, 0, 0xFFFC0000, 0]]
    assert articulation_template((rows, True, True))[0].tolist() == rows.tolist()
    assert articulation_rows({"bars": [None] * 64}).shape == (64, 4)
    for bad, shown in (({"bars": [None] * 65}, "1 .. 64 bars, got 65"), ({"bars": []}, "got 0"),
                       ({"bars": [None], "grid": 4}, "unknown key 'grid' beside bars"),
                       ({"duration": [2, 4], "cells": 1}, "unknown key 'cells'"),
                       ({"bars": [None, {"length": [1, 2]}]}, "bar 1: unknown key 'length'"),
                       ({"bars": [{"duration": [5, 4]}]}, r"bar 0: duration: lo <= hi expected, got \[5, 4\]"),
                       ({"duration": [0, 4]}, r"duration: .*got \[0, 4\]"), ({"duration": [1, 129]}, r"got \[1, 129\]"),
                       ({"duration": [1]}, r"got \[1\]"), ({"duration": 4}, "got 4"), ({"duration": [True, 4]}, "got"),
                       ({"bars": [None, None, {"velocity": [90, 80]}]}, r"bar 2: velocity: lo <= hi expected, got \[90, 80\]"),
                       ({"velocity": [0, 128]}, r"velocity: .*got \[0, 128\]"), ({"velocity": [-1, 5]}, r"got \[-1, 5\]"),
                       ({"velocity": [None, 5]}, "velocity: a pair"),
                       ({"within_bar": 1}, "within_bar: true or false expected, got 1"),
                       ({"bars": [None], "hold_guide": "yes"}, "hold_guide: true or false expected, got 'yes'"),
                       ({"bars": [7]}, "bar 0: null or .*got 7"), ([[1, 2]], "expected, got"), (7, "expected, got 7"),
                       ((np.zeros((65, 4), dtype=np.uint32), False, False), r"shape \(65, 4\)"),
                       ((np.zeros((2, 4), dtype=np.uint32), False, False), "bar 0: an empty velocity mask")):
        with pytest.raises(CommuHipError, match="articulation: .*" + shown):
            articulation_template(bad)


def test_check_articulation_of_the_command_line(tmp_path):
    cli = VH.cli_module()
    ns = lambda **kw: types.SimpleNamespace(**dict(dict(articulation=None, guide=None, note_order=False, grammar=False), **kw))
    a = ns()
    assert cli.check_articulation(a) is None and a.articulation_doc is None
    a = ns(articulation='{"duration": [2, 16], "velocity": [60, 100]}')
    assert json.loads(cli.check_articulation(a)) == {"bars": [{"duration": [2, 16], "velocity": [60, 100]}],
                                                     "within_bar": False, "hold_guide": False}
    assert a.note_order is False and a.grammar is False                                   # (implies nothing)
    from commu_amd.generate import articulation_rows
    spec = {"bars": [{"duration": [None, 8], "velocity": [61, 99]}, None], "within_bar": True}
    doc = json.loads(cli.check_articulation(ns(articulation=json.dumps(spec))))
    assert doc["bars"] == [{"duration": [None, 8], "velocity": [60, 100]}, None] and doc["within_bar"] is True
    assert articulation_rows(doc).tolist() == articulation_rows(spec).tolist()            # (the same bins)
    f = tmp_path / "a.json"
    f.write_text('{"duration": [1, 4], "hold_guide": true}')
    a = ns(articulation=str(f), guide='{"cells": 1, "bars": [[null]]}')
    assert json.loads(cli.check_articulation(a))["hold_guide"] is True
    for bad, message in (('{"duration": [5, 4]}', r"--articulation: duration: lo <= hi expected, got \[5, 4\]"),
                         ("{", "--articulation: not JSON"),
                         (str(tmp_path / "none.json"), "--articulation: JSON text or a readable JSON file expected"),
                         ('{"bars": [null, {"velocity": [3, 2]}]}', "--articulation: bar 1: velocity: lo <= hi"),
                         ('{"hold_guide": true}', "--articulation: hold_guide without --guide"),
                         ('{"key": 1}', "--articulation: unknown key 'key'")):
        with pytest.raises(ValueError, match=message):
            cli.check_articulation(ns(articulation=bad))


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *args], capture_output=True,
                          text=True, timeout=120)


def test_cli_refuses_before_a_model_is_loaded(tmp_path):
    out = _cli("--help")
    assert out.returncode == 0 and "--articulation SPEC" in out.stdout
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt")]
    out = _cli(*common, "--num_generate", "1", "--articulation", '{"bars": [null, {"duration": [9, 3]}]}')
    assert out.returncode != 0 and "bar 1: duration: lo <= hi expected, got [9, 3]" in out.stderr, out.stderr[-400:]
    assert "no_such_checkpoint" not in out.stderr                          # (refused before the checkpoint was looked for)
    out = _cli(*common, "--num_generate", "1", "--articulation", '{"hold_guide": true}')
    assert out.returncode != 0 and "hold_guide without --guide" in out.stderr and "no_such_checkpoint" not in out.stderr
    req = tmp_path / "requests.json"
    req.write_text(json.dumps([{"num_generate": 1, "articulation": {"duration": [1, 8]}},
                               {"num_generate": 1, "articulation": {"velocity": [0, 200]}}]))
    out = _cli(*common, "--requests", str(req))
    assert out.returncode != 0 and "request 1: articulation: velocity:" in out.stderr and "[0, 200]" in out.stderr, \
        out.stderr[-400:]
    assert "no_such_checkpoint" not in out.stderr
    # hold_guide in a pool: the request's own guide or the pool's will do, neither is refused with the request's index
    req.write_text(json.dumps([{"num_generate": 1, "articulation": {"hold_guide": True}, "guide": {"cells": 1, "bars": [[None]]}},
                               {"num_generate": 1, "articulation": {"hold_guide": True}}]))
    out = _cli(*common, "--requests", str(req))
    assert out.returncode != 0 and "request 1: articulation: hold_guide without a guide" in out.stderr, out.stderr[-400:]
    assert "no_such_checkpoint" not in out.stderr
    cli = VH.cli_module()
    pool = cli.check_requests(types.SimpleNamespace(articulation=None, guide='{"cells": 1, "bars": [[null]]}'),
                              types.SimpleNamespace(requests=str(req)))
    assert [r["articulation"]["hold_guide"] for r in pool] == [True, True] and pool[1].get("guide") is None
    # the pool-wide --articulation holds for a request without one of its own, and needs a guide there just the same
    req.write_text(json.dumps([{"num_generate": 1, "guide": {"cells": 1, "bars": [[None]]}}, {"num_generate": 1}]))
    with pytest.raises(ValueError, match="request 1: articulation: hold_guide without a guide"):
        cli.check_requests(types.SimpleNamespace(articulation='{"hold_guide": true}', guide=None),
                           types.SimpleNamespace(requests=str(req)))


def test_struct_mirrors_carry_the_fields_ahead_of_guide_ctl_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    assert C.sizeof(_lib.DecodeArmArgs) == lib.commu_decode_arm_args_bytes()
    assert C.sizeof(_lib.DecodeArmPrimedArgs) == lib.commu_decode_arm_primed_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        names = [n for n, _ in cls._fields_]
        assert names[-14:-10] == ["art_ctl", "art_table", "art_rows", "guide_ctl"]
        a = _lib.struct_args(cls)
        assert a.art_ctl is None and a.art_table is None and a.art_rows == 0                # null unless named
    for cls in (_lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs):
        names = [n for n, _ in cls._fields_]
        i = names.index("guide_ctl")
        assert names[i - 2:i + 2] == ["art_ctl", "e_art", "guide_ctl", "e_guide"]
        assert _lib.struct_args(cls).art_ctl is None and _lib.struct_args(cls).e_art is None


def table_rows(dec, base, n):
    return dec.art_table[base:base + n].numpy().view(np.uint32).tolist()


A1 = {"duration": [2, 16]}                                                          # 1 row
A2 = {"bars": [{"velocity": [64, 64]}, None], "within_bar": True}                   # 2 rows


def test_set_articulation_allocates_once_rewrites_in_place_and_keeps_the_other_words():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ForcedDecoder, articulation_rows
    assert ForcedDecoder.art_ctl is None and ForcedDecoder.art_table is None               # (class-level defaults)
    dec = TG.stub()
    dec.set_articulation(None)
    dec.set_articulation(False, rows=[1])
    dec.set_articulation([None, False, None, None])
    assert dec.art_ctl is None and dec.art_table is None and dec.guide_ctl is None and dec.graph == "captured"
    with pytest.raises(CommuHipError, match="lo <= hi"):
        dec.set_articulation({"duration": [3, 2]})
    with pytest.raises(CommuHipError, match=r"rows: slot numbers in \[0, 4\) expected"):
        dec.set_articulation(A1, rows=[4])
    # 65 distinct templates of 64 bars: 4160 rows
    many = [{"bars": [{"duration": [1, 1 + k]}] + [None] * 63} for k in range(65)]
    with pytest.raises(CommuHipError, match="more than the table's 4096 rows"):
        TG.stub(65).set_articulation(many)
    assert dec.art_ctl is None and dec.guide_ctl is None and dec.graph == "captured"       # refused before anything changed
    dec.set_articulation(A1, rows=[0, 2])
    assert dec.art_ctl.tolist() == [W(0, 1), -1, W(0, 1), -1] and dec.graph is None and dec.rows_on
    assert tuple(dec.art_table.shape) == (4096, 4) and dec.art_table.dtype == torch.int32
    assert table_rows(dec, 0, 2) == [articulation_rows(A1)[0].tolist(), FREE]
    # (everything the one kernel reads exists and is all off: the rule implies none of the others)
    assert dec.guide_ctl.tolist() == [-1] * 4 and tuple(dec.guide_table.shape) == (65536, 4)
    assert dec.onset_ctl.tolist() == [-1] * 4 and dec.interval_ctl.tolist() == [-1] * 4
    assert dec.density_ctl.tolist() == [-1] * 4 and dec.voice_ctl.tolist() == [-1] * 4 and dec.order_ctl.tolist() == [-1] * 4
    assert dec.bias is not None and dec.gram is not None and dec.harm is not None and dec.cls_ctl is not None
    words, table, guide = dec.art_ctl, dec.art_table, dec.guide_ctl
    dec.graph = "captured again"
    dec.set_guide(TG.G1, rows=[1])
    dec.set_articulation([A2, {**A1, "hold_guide": True}, A2], rows=[1, 2, 3])
    # (packed behind the first template; the same rows are stored once, the switches live in the word)
    assert dec.art_ctl is words and words.tolist() == [W(0, 1), W(1, 2, True), W(0, 1, False, True), W(1, 2, True)]
    assert dec.art_table is table and table_rows(dec, 1, 2) == articulation_rows(A2).tolist() and dec._art_used == 3
    assert dec.guide_ctl is guide and guide.tolist() == [-1, GD.word(0, 1, 7), -1, -1] and dec.graph == "captured again"
    with pytest.raises(CommuHipError, match=r"got \[0, 4\]"):
        dec.set_articulation([A2, {"duration": [0, 4]}], rows=[0, 1])
    assert words.tolist() == [W(0, 1), W(1, 2, True), W(0, 1, False, True), W(1, 2, True)]  # (a refused call leaves every word)
    dec.rearm(0, articulation={"velocity": [0, 1]})
    assert words.tolist()[0] == W(3, 1) and table_rows(dec, 3, 1) == [[0, 3, 0, 0]]
    dec.rearm(0)                                                            # (None: the slot keeps its word)
    assert words.tolist()[0] == W(3, 1)
    dec.rearm(0, articulation=False)
    assert words.tolist() == [-1, W(1, 2, True), W(0, 1, False, True), W(1, 2, True)]
    dec.set_articulation(A2)                                                # (all slots: the table is packed anew)
    assert dec.art_ctl is words and dec.art_table is table and words.tolist() == [W(0, 2, True)] * 4 and dec._art_used == 2
    assert table_rows(dec, 0, 2) == articulation_rows(A2).tolist()
    dec.set_articulation(None)
    assert words.tolist() == [-1] * 4 and guide.tolist() == [-1, GD.word(0, 1, 7), -1, -1] and dec.graph == "captured again"


def test_hold_guide_needs_a_guide_where_the_generator_sees_both():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import _articulation_needs_guide, articulation_template, guide_template
    hold, plain = articulation_template({"hold_guide": True}), articulation_template(A1)
    g = guide_template(TG.G1)
    _articulation_needs_guide([hold, plain, None], [g, None, None])
    with pytest.raises(CommuHipError, match=r"hold_guide without a guide \(sequence 1\)"):
        _articulation_needs_guide([hold, hold], [g, None])


# ------------------------------------------------------------------------------------------------ 3. the reference loop
def walk(r, gram, order_ctl, voice_ctl, guide_ctl, table, art_ctl, art_table, max_iters=200):
    """test_guide_host.walk with this rule among the bans: the forcing loop on the device record's restatement
    (prime_contract.pre / post), one `pre` per iteration, on random logits under the grammar.  Returns (seq, drawn mask,
    record); seq is None when a row had nothing left (the Q12 exit)."""
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
                        set(GD.bans(seq, n, guide_ctl, table)) | set(AC.bans(seq, n, art_ctl, art_table, guide_ctl, table)))
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


SPEC = {"hold_guide": True, "within_bar": True, "duration": [2, 32]}
SETTINGS = TG.SETTINGS


@pytest.fixture(scope="module")
def grammar():
    from commu_amd.generate import event_grammar
    return event_grammar()


@pytest.fixture(scope="module")
def guide_table():
    from commu_amd.generate import guide_template
    rows, cells = guide_template(TG.GUIDE)
    assert cells == 16 and rows.shape == (34, 4)
    return rows


def tally(gram, voice_ctl, gtable, guide_on, art):
    """Over the 60 requests under the grammar and the note order, the guide `gtable` on or off, the articulation `art`
    ((rows, w, h) or None): (requests with a drawn note held into a ban, drawn notes held into a ban, drawn notes, drawn
    notes crossing the bar line, drawn notes outside the window [2, 32] that no cap forced, Q12 endings, failures of
    validate_teacher_forced_sequence)."""
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, note_order_violation, parse_events
    start = len(CTX)
    gword = GD.word(0, 2, 3) if guide_on else -1
    aword, atable = (-1, np.stack([AC.row_of()])) if art is None else (W(0, len(art[0]), art[1], art[2]), art[0])
    off, held_notes, notes, crossing, outside, q12, invalid = [], 0, 0, 0, 0, [], []
    for r in GH.requests(60):
        seq, drawn, s = walk(r, gram, 0, voice_ctl, gword, gtable, aword, atable)
        if seq is None:
            q12.append(r["seed"])
            continue
        assert parse_events(seq, start) is None and note_order_violation(seq, start) is None, (r, seq)
        res = AC.held_into_ban(seq, start, gtable, drawn, cells=16)
        notes += len(res)
        held_notes += sum(h for _, h, _ in res)
        crossing += sum(c for _, _, c in res)
        if any(h for _, h, _ in res):
            off.append(r["seed"])
        for i, _, _ in res:
            d = seq[i] - 303
            lo, cap = AC.window(seq, i, aword, atable, gword, gtable) if art is not None else (2, 32)
            outside += not (min(2, cap) <= d <= 32)
        if art is not None:
            assert AC.articulation_violation(seq, start, art[0], gtable if guide_on else None, drawn, 16, art[1], art[2]) is None
        rep = ForcingReport(len(r["chord_token"]), r["num_measures"])
        rep.consumed = s[PC.F_CUR]
        try:
            rep.validate_teacher_forced_sequence(seq)
        except Exception:
            invalid.append(r["seed"])
    return off, held_notes, notes, crossing, outside, q12, invalid


@pytest.fixture(scope="module")
def without_the_rule(grammar, guide_table):
    return {name: tally(grammar, voice, guide_table, True, None) for name, (_, voice) in SETTINGS.items()}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_without_the_rule_drawn_notes_are_held_into_steps_the_guide_bans(without_the_rule, setting):
    off, held, notes, crossing, outside, q12, invalid = without_the_rule[setting]
    print("grammar + %s, guide on, no articulation: requests with a held-into-ban note:" % setting, len(off), "of 60; notes held "
          "into a ban:", held, "of", notes, "; crossing the bar line:", crossing, "; outside [2, 32]:", outside, "; Q12:",
          len(q12), "; invalid:", len(invalid))
    assert len(off) > 0


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_rule_through_the_reference_loop(grammar, guide_table, without_the_rule, setting):
    """{"hold_guide": true, "within_bar": true, "duration": [2, 32]} beside the two-bar melody as a guide on the 60 requests:
    no DRAWN note is held into a step whose cell bans its pitch, none crosses the bar line or leaves the window (lengths below
    2 only where the cap forced them), no request ends by Q12, and the validators refuse no sequence they accepted without
    the rule (docs/EXPERIMENTS.md 9d)."""
    from commu_amd.generate import articulation_template
    base = without_the_rule[setting]
    off, held, notes, crossing, outside, q12, invalid = tally(grammar, SETTINGS[setting][1], guide_table, True,
                                                              articulation_template(SPEC))
    print("grammar + %s, guide on, articulation: requests with a held-into-ban note:" % setting, len(off), "; notes held into "
          "a ban:", held, "of", notes, "; crossing the bar line:", crossing, "; outside the window:", outside, "; Q12:", q12,
          "(without:", base[5], "); invalid:", len(invalid), "(without:", len(base[6]), ")")
    assert off == [] and held == 0
    assert crossing == 0 and outside == 0
    assert q12 == []
    assert set(invalid) <= set(base[6])
