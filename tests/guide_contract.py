"""The guide track restated in plain numpy (no GPU, no package code): which pitch ids and which position ids a draw may not
take so that the notes being written fit a mask over pitches that is indexed by time -- derived from a finished track, or
given raw.

Ids: EOS 1, BAR 2, PITCH 3 .. 130 (MIDI pitch = id - 3), POSITION 432 .. 559 (432 + g for step g of the bar's 128-step grid).

  TABLE.  guide_table is uint32 [rows][4], 1 <= rows <= 65536.  A template has R bars, 1 <= R <= 64, and C = 128 >> s cells
     per bar, s in 0 .. 7.  Each bar is a BLOCK of 1 + C consecutive rows:
       row 0 of a block is the bar's LIVE ROW, a 128-bit mask over positions in the onset table's format: bit g % 32 of word
         g // 32 set means a note may start at step g;
       rows 1 .. C are the CELL ROWS, 128-bit masks over pitches: bit k % 32 of word k // 32 set means pitch id 3 + k may be
         drawn.
  CONTROL WORD.  One int32 per sequence: -1 off, else base + 65536 R + 2^23 s, with base + R (1 + C) <= rows.
  1. BLOCK OF THE OPEN BAR.  As the onset rule: nb = the number of BAR tokens in S = seq[0 : L], i = max(nb - 1, 0) (a
     prompt's bars included), the block starts at base + (i mod R) (1 + C).
  2. PITCH BAN.  j and p are the note order's: j is the largest index with S[j] a BAR or a POSITION.  No such j, or S[j] is
     BAR: no pitch is banned.  Otherwise g = p - 432, the cell row is block + 1 + (g >> s), and every PITCH id whose bit is
     clear is banned.  Ids outside 3 .. 130 are never touched.
  3. POSITION BAN.  Every POSITION id whose bit in the live row is clear is banned.  The live row is ANDed into the onset
     row before that is used, so the onset rule's position ban AND ITS DENSITY WAIVER (onsets_contract rule 3) apply to the
     intersection: the waiver lets a bar end once range, onset row and live row together leave no position.
  4. BOUNDS.  Every row index is clamped to rows - 1, whatever the arrays hold.

A banned id's y is replaced by -inf in the one select of the note order, the voice cap, the density, the interval and the
onsets: a draw is the onset draw with bias = -inf at these ids (and the density's BAR / EOS ban taken under the waiver on
the ANDed row), which is how restate_with_guide computes it.  An off word is the call without the fields; so is a word over
an all-ones live row with all-ones cell rows.

NOT COVERED: only a note's START is tested (a drawn note held across a later change of the guide is not checked); forced
tokens (position 0 after a BAR, a chord's position); notes inside a prompt; a pitch range, strict harmony or interval window
that together with the cell row leaves no pitch ends the attempt by Q12, as before."""
import numpy as np

import density_contract as DC
import onsets_contract as OC

V = 729
EOS, BAR = 1, 2
PITCH_LO, PITCH_HI = 3, 130
POS_LO, POS_HI = 432, 559
GRID = 128
OFF = -1
ROWS_MAX, CYCLE_MAX = 65536, 64
ONES = np.full(4, 0xFFFFFFFF, dtype=np.uint32)


def word(base, bars, shift):
    """The control word of a template of `bars` blocks of 1 + (128 >> shift) rows that starts at table row `base`."""
    return int(base) + 65536 * int(bars) + (1 << 23) * int(shift)


def unpack(ctl):
    """(base, R, s, C) of an on word."""
    ctl = int(ctl)
    s = (ctl >> 23) & 7
    return ctl & 65535, min(max((ctl >> 16) & 127, 1), CYCLE_MAX), s, GRID >> s


def mask_of(bits):
    """uint32 [4]: the 128-bit row with the given bits set (grid steps for a live row, id - 3 for a cell row)."""
    r = np.zeros(4, dtype=np.uint32)
    for k in bits:
        k = int(k)
        assert 0 <= k < 128
        r[k // 32] |= np.uint32(1 << (k % 32))
    return r


def bit(row, k):
    return bool((int(row[k // 32]) >> (k % 32)) & 1)


def block_of(seq_row, length, ctl):
    """Rule 1: the (unclamped) first row of the open bar's block."""
    base, R, s, C = unpack(ctl)
    return base + (OC.bar_index(seq_row, length) % R) * (1 + C)


def _row(table, idx):
    table = np.asarray(table, dtype=np.uint32).reshape(-1, 4)
    assert 1 <= len(table) <= ROWS_MAX
    return table[min(max(int(idx), 0), len(table) - 1)]          # (rule 4)


def live_row(seq_row, length, ctl, table):
    """The four words of the open bar's live row (all ones for an off word)."""
    if int(ctl) < 0:
        return ONES.copy()
    return _row(table, block_of(seq_row, length, ctl))


def last_breaker(seq_row, length):
    """The note order's S[j]: the last BAR or POSITION token of seq[0 : length], None when there is none."""
    for t in reversed([int(t) for t in list(seq_row)[:max(int(length), 0)]]):
        if t == BAR or POS_LO <= t <= POS_HI:
            return t
    return None


def cell_row(seq_row, length, ctl, table):
    """The four words of the cell row of rule 2 (all ones: off, no breaker, or BAR)."""
    p = last_breaker(seq_row, length)
    if int(ctl) < 0 or p is None or p == BAR:
        return ONES.copy()
    s = unpack(ctl)[2]
    return _row(table, block_of(seq_row, length, ctl) + 1 + ((p - POS_LO) >> s))


def pitch_bans(seq_row, length, ctl, table):
    """Rule 2: the sorted PITCH ids banned for the draw that follows seq_row[0 : length]."""
    row = cell_row(seq_row, length, ctl, table)
    return [PITCH_LO + k for k in range(PITCH_HI - PITCH_LO + 1) if not bit(row, k)]


def position_bans(seq_row, length, ctl, table):
    """Rule 3: the sorted POSITION ids the live row bans."""
    row = live_row(seq_row, length, ctl, table)
    return [POS_LO + g for g in range(GRID) if not bit(row, g)]


def bans(seq_row, length, ctl, table):
    """Rules 2 and 3 together."""
    return sorted(set(pitch_bans(seq_row, length, ctl, table)) | set(position_bans(seq_row, length, ctl, table)))


def merged_row(seq_row, length, ctl, table, onset_ctl, onset_table):
    """The onset row of the open bar ANDed with the live row: what the onset rule's waiver sees."""
    return OC.open_row(seq_row, length, onset_ctl, onset_table) & live_row(seq_row, length, ctl, table)


def density_bans(seq_row, length, ctl, table, onset_ctl, onset_table, density_ctl, order_ctl, voice_ctl):
    """onsets_contract.density_bans with the ANDed row in place of the onset row."""
    density_ctl = int(density_ctl)
    if density_ctl < 0:
        return []
    lo, hi = density_ctl & 255, (density_ctl >> 8) & 255
    c = DC.count(seq_row, length)
    out = set()
    if hi >= 1 and c >= hi:
        out |= set(range(POS_LO, POS_HI + 1))
    if lo >= 1 and c < lo:
        end = DC.position_end(seq_row, length, density_ctl, order_ctl, voice_ctl)
        row = merged_row(seq_row, length, ctl, table, onset_ctl, onset_table)
        if any(bit(row, g) for g in range(end - POS_LO, GRID)):
            out |= {EOS, BAR}
    return sorted(out)


def banned_bias(bias, seq_row, length, ctl, table, onset_ctl, onset_table, density_ctl, order_ctl, voice_ctl):
    """fp32 [V]: the bias row (None: zeros) with -inf at the guide's ids, the onset row's ids and the density's ids under the
    waiver on the ANDed row."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl, table)] = -np.inf
    row[OC.bans(seq_row, length, onset_ctl, onset_table)] = -np.inf
    row[density_bans(seq_row, length, ctl, table, onset_ctl, onset_table, density_ctl, order_ctl, voice_ctl)] = -np.inf
    return row


def restate_with_guide(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl, interval_ctl, onset_ctl,
                       onset_table, guide_ctl, guide_table, bias=None, **kw):
    """interval_contract.restate_with_interval with the density word and the onset word OFF (their bans are in the bias,
    the density's under the waiver on the ANDed row) on the bias with -inf at the guide's ids."""
    import interval_contract as IC
    return IC.restate_with_interval(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, DC.OFF, interval_ctl,
                                    bias=banned_bias(bias, seq_row, length, guide_ctl, guide_table, onset_ctl, onset_table,
                                                     density_ctl, order_ctl, voice_ctl), **kw)


def guide_violation(seq, start, rows, drawn_mask=None, cells=16):
    """The first index i >= start whose PITCH or POSITION token the template `rows` (uint32 [R (1 + cells)][4], base 0)
    would have banned given seq[:i] (read FORWARD), None when there is none.  With drawn_mask only the indices with
    drawn_mask[i] true count: seq[i] was drawn, not forced and not part of a prompt."""
    seq = [int(t) for t in seq]
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    s = {GRID >> k: k for k in range(8)}[int(cells)]
    per = 1 + (GRID >> s)
    assert len(rows) % per == 0 and 1 <= len(rows) // per <= CYCLE_MAX, (len(rows), s)
    w = word(0, len(rows) // per, s)
    for i in range(max(int(start), 0), len(seq)):
        if drawn_mask is not None and not drawn_mask[i]:
            continue
        if PITCH_LO <= seq[i] <= PITCH_HI and seq[i] in pitch_bans(seq, i, w, rows):
            return i
        if POS_LO <= seq[i] <= POS_HI and seq[i] in position_bans(seq, i, w, rows):
            return i
    return None
