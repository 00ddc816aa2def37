"""The articulation rule restated in plain numpy (no GPU, no package code): which DURATION ids and which VELOCITY ids a draw
may not take so that the notes being written follow a per-bar template of lengths and loudness, end by the bar line, and are
not held into a step where the guide track bans their pitch.

Ids: PITCH 3 .. 130 (MIDI pitch = id - 3), VELOCITY 131 .. 194 (bin id - 131, MIDI velocity 2 bin), DURATION 304 .. 431
(d = id - 303 steps, 1 .. 128), POSITION 432 .. 559 (432 + g for step g of the bar's 128-step grid).

  TABLE.  art_table is uint32 [rows][4], 1 <= rows <= 4096.  One row is one bar of a template:
       word 0 is dlo | dhi << 8, each 0 .. 128; 0 means that bound is not set;
       words 1 and 2 are a 64-bit velocity mask: bit k % 32 of word 1 + k // 32 set means VELOCITY id 131 + k may be drawn;
       word 3 is reserved: the host writes 0 and nothing reads it.
  CONTROL WORD.  One int32 per sequence: -1 off, else base + 4096 R + 2^19 w + 2^20 h, base in 0 .. 4095, R in 1 .. 64 the
     cycle length, base + R <= rows, w the bar-line switch, h the guide-hold switch.
  1. ROW OF THE OPEN BAR.  As the onset rule: nb = the number of BAR tokens in S = seq[0 : L], i = max(nb - 1, 0) (a prompt's
     bars included), the row is base + (i mod R), clamped to rows - 1 whatever the arrays hold.
  2. VELOCITY BAN.  Every VELOCITY id whose bit in words 1 and 2 is clear is banned.  Ids 130 and 195 are never touched.
  3. DURATION WINDOW.  j and p are the note order's: j is the largest index with S[j] a BAR or a POSITION; a = p - 432 exists
     when S[j] is a POSITION.  q = S[L - 1] is the grammar's previous token (S[0] of the row while L < 1, as the grammar
     reads it); k = q - 3 exists when q is a PITCH.  cap = 128, lowered by each of these that applies:
       dhi >= 1: cap = min(cap, dhi);
       w set and a exists: cap = min(cap, 128 - a) -- the note ends by the bar line;
       h set, the sequence's guide word on, a and k exist: cap = min(cap, f), f the smallest m in 1 .. 127 such that bit k of
         the guide's cell row for step a + m is clear; no such m: the term does not apply.  The cell row of step a + m < 128
         is block_i + 1 + ((a + m) >> s), of a later step block_{i+1} + 1 + ((a + m - 128) >> s), with block_x = base_g +
         (x mod R_g) (1 + C) and the guide's own base_g, R_g, s, C; every row index is clamped to guide_rows - 1.
     lo = min(max(dlo, 1), cap).  Banned are DURATION ids 304 .. 303 + lo - 1 and 304 + cap .. 431.  The window is never empty
     (a <= 127, f >= 1); where the bar line or the guide leaves less room than dlo the lower bound gives way.  Ids 303 and
     432 are never touched.  Step a itself is not tested: that is the guide's pitch rule.
  4. SELECT.  The bans apply whatever class is drawn and join the one select of the note order .. the guide: a draw is the
     guide draw with bias = -inf at these ids, which is how restate_with_articulation computes it.  An off word is the call
     without the fields; so is a word over a row with dlo = dhi = 0, an all-ones velocity mask and w = h = 0.

NOT COVERED: forced tokens, and anything a forced position starts; notes inside a prompt; a note forced shorter than dlo
(rule 3); an empty velocity mask ends the attempt by Q12 as before (the host refuses to build one); the hold rule reads the
next bar's block even where the generation length would cut the sequence first; the hold rule tests the guide only (harmony
across a chord change is not tested)."""
import numpy as np

import guide_contract as GD
import onsets_contract as OC

V = 729
BAR = 2
PITCH_LO, PITCH_HI = 3, 130
VEL_LO, VEL_HI = 131, 194
DUR_LO, DUR_HI = 304, 431
POS_LO, POS_HI = 432, 559
GRID = 128
OFF = -1
ROWS_MAX, CYCLE_MAX = 4096, 64


def word(base, cycle, within_bar=False, hold_guide=False):
    """The control word of a template of `cycle` rows that starts at table row `base`."""
    return int(base) + 4096 * int(cycle) + (1 << 19) * int(bool(within_bar)) + (1 << 20) * int(bool(hold_guide))


def unpack(ctl):
    """(base, R, w, h) of an on word."""
    ctl = int(ctl)
    return ctl & 4095, min(max((ctl >> 12) & 127, 1), CYCLE_MAX), (ctl >> 19) & 1, (ctl >> 20) & 1


def row_of(dlo=0, dhi=0, velocities=None):
    """uint32 [4]: one bar of a template; velocities: the bins 0 .. 63 that may be drawn (None: all)."""
    r = np.zeros(4, dtype=np.uint32)
    assert 0 <= dlo <= 128 and 0 <= dhi <= 128
    r[0] = int(dlo) | int(dhi) << 8
    for k in (range(64) if velocities is None else velocities):
        k = int(k)
        assert 0 <= k < 64
        r[1 + k // 32] |= np.uint32(1 << (k % 32))
    return r


def open_row(seq_row, length, ctl, table):
    """Rule 1: the four words of the open bar's row (None for an off word)."""
    if int(ctl) < 0:
        return None
    table = np.asarray(table, dtype=np.uint32).reshape(-1, 4)
    assert 1 <= len(table) <= ROWS_MAX
    base, R, _, _ = unpack(ctl)
    return table[min(max(base + OC.bar_index(seq_row, length) % R, 0), len(table) - 1)]


def velocity_bans(seq_row, length, ctl, table):
    """Rule 2: the sorted VELOCITY ids banned."""
    row = open_row(seq_row, length, ctl, table)
    if row is None:
        return []
    return [VEL_LO + k for k in range(64) if not (int(row[1 + k // 32]) >> (k % 32)) & 1]


def start_step(seq_row, length):
    """a of rule 3: the grid step of the note order's last breaker when it is a POSITION, else None."""
    p = GD.last_breaker(seq_row, length)
    return None if (p is None or p == BAR) else p - POS_LO


def previous_token(seq_row, length):
    """q of rule 3: S[L - 1], as the grammar reads it (index clamped into the row)."""
    row = list(seq_row)
    return int(row[min(max(int(length), 1), len(row)) - 1])


def guide_step_row(seq_row, length, guide_ctl, guide_table, t):
    """The guide's cell row for step t = a + m of rule 3 (t in 1 .. 254): the open bar's block below step 128, the next
    bar's past it; the index clamped into the table."""
    base, R, s, C = GD.unpack(guide_ctl)
    i = OC.bar_index(seq_row, length)
    if t < GRID:
        idx = base + (i % R) * (1 + C) + 1 + (t >> s)
    else:
        idx = base + ((i + 1) % R) * (1 + C) + 1 + ((t - GRID) >> s)
    return GD._row(guide_table, idx)


def first_ban(seq_row, length, guide_ctl, guide_table):
    """f of rule 3 (None: a or k does not exist, the guide word is off, or no step 1 .. 127 ahead bans the pitch)."""
    a, q = start_step(seq_row, length), previous_token(seq_row, length)
    if int(guide_ctl) < 0 or a is None or not PITCH_LO <= q <= PITCH_HI:
        return None
    for m in range(1, GRID):
        if not GD.bit(guide_step_row(seq_row, length, guide_ctl, guide_table, a + m), q - PITCH_LO):
            return m
    return None


def window(seq_row, length, ctl, table, guide_ctl=-1, guide_table=None):
    """Rule 3: (lo, cap) -- the durations lo .. cap steps may be drawn; (1, 128) for an off word."""
    row = open_row(seq_row, length, ctl, table)
    if row is None:
        return 1, GRID
    _, _, w, h = unpack(ctl)
    dlo, dhi = int(row[0]) & 255, (int(row[0]) >> 8) & 255
    cap = GRID
    if dhi >= 1:
        cap = min(cap, dhi)
    a = start_step(seq_row, length)
    if w and a is not None:
        cap = min(cap, GRID - a)
    if h:
        f = first_ban(seq_row, length, guide_ctl, guide_table)
        if f is not None:
            cap = min(cap, f)
    return min(max(dlo, 1), cap), cap


def duration_bans(seq_row, length, ctl, table, guide_ctl=-1, guide_table=None):
    lo, cap = window(seq_row, length, ctl, table, guide_ctl, guide_table)
    return list(range(DUR_LO, DUR_LO - 1 + lo)) + list(range(DUR_LO + cap, DUR_HI + 1))


def bans(seq_row, length, ctl, table, guide_ctl=-1, guide_table=None):
    """Rules 2 and 3 together."""
    return sorted(velocity_bans(seq_row, length, ctl, table) + duration_bans(seq_row, length, ctl, table, guide_ctl, guide_table))


def banned_bias(bias, seq_row, length, ctl, table, guide_ctl=-1, guide_table=None):
    """fp32 [V]: the bias row (None: zeros) with -inf at the rule's ids."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl, table, guide_ctl, guide_table)] = -np.inf
    return row


def restate_with_articulation(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl, interval_ctl, onset_ctl,
                              onset_table, guide_ctl, guide_table, art_ctl, art_table, bias=None, **kw):
    """guide_contract.restate_with_guide on the bias with -inf at the articulation's ids (rule 4)."""
    return GD.restate_with_guide(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl, interval_ctl, onset_ctl,
                                 onset_table, guide_ctl, guide_table,
                                 bias=banned_bias(bias, seq_row, length, art_ctl, art_table, guide_ctl, guide_table), **kw)


def articulation_violation(seq, start, rows, guide_rows=None, drawn_mask=None, cells=16, within_bar=False, hold_guide=False):
    """The checker: the first index i >= start whose DURATION or VELOCITY token the template `rows` (uint32 [R][4], base 0,
    with the two switches as given) would have banned given seq[:i] (read FORWARD) under the guide `guide_rows` (uint32
    [R_g (1 + cells)][4], base 0; None: no guide), None when there is none.  With drawn_mask only the indices with
    drawn_mask[i] true count: seq[i] was drawn, not forced and not part of a prompt."""
    seq = [int(t) for t in seq]
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    assert 1 <= len(rows) <= CYCLE_MAX
    w = word(0, len(rows), within_bar, hold_guide)
    gw = -1
    if guide_rows is not None:
        guide_rows = np.asarray(guide_rows, dtype=np.uint32).reshape(-1, 4)
        s = {GRID >> k: k for k in range(8)}[int(cells)]
        per = 1 + (GRID >> s)
        assert len(guide_rows) % per == 0 and 1 <= len(guide_rows) // per <= GD.CYCLE_MAX
        gw = GD.word(0, len(guide_rows) // per, s)
    for i in range(max(int(start), 0), len(seq)):
        if drawn_mask is not None and not drawn_mask[i]:
            continue
        if DUR_LO <= seq[i] <= DUR_HI and seq[i] in duration_bans(seq, i, w, rows, gw, guide_rows):
            return i
        if VEL_LO <= seq[i] <= VEL_HI and seq[i] in velocity_bans(seq, i, w, rows):
            return i
    return None


def held_into_ban(seq, start, guide_rows, drawn_mask=None, cells=16):
    """The measurement the rule exists for, on the finished sequence alone (no rule of this file is used): the complete
    Position, Velocity, Pitch, Duration groups at index >= start (with drawn_mask: whose DURATION was drawn) as (index of the
    duration, held into a ban, crosses the bar line): held into a ban when some step a + 1 .. a + d - 1 lies in a cell whose
    row bans the pitch, the next bar's block past step 127."""
    seq = [int(t) for t in seq]
    guide_rows = np.asarray(guide_rows, dtype=np.uint32).reshape(-1, 4)
    s = {GRID >> k: k for k in range(8)}[int(cells)]
    per = 1 + (GRID >> s)
    R = len(guide_rows) // per
    out = []
    nb = 0
    for i, t in enumerate(seq):
        if t == BAR:
            nb += 1
        if i < start or i + 3 >= len(seq) or not (POS_LO <= t <= POS_HI and VEL_LO <= seq[i + 1] <= VEL_HI and
                                                  PITCH_LO <= seq[i + 2] <= PITCH_HI and DUR_LO <= seq[i + 3] <= DUR_HI):
            continue
        if drawn_mask is not None and not drawn_mask[i + 3]:
            continue
        a, k, d = t - POS_LO, seq[i + 2] - PITCH_LO, seq[i + 3] - (DUR_LO - 1)
        bar = max(nb - 1, 0)
        held = False
        for m in range(1, d):
            x, g = (bar, a + m) if a + m < GRID else (bar + 1, a + m - GRID)
            row = guide_rows[min((x % R) * per + 1 + (g >> s), len(guide_rows) - 1)]
            held = held or not GD.bit(row, k)
        out.append((i + 3, held, a + d > GRID))
    return out
