"""The onset templates restated in plain numpy (no GPU, no package code): which position ids a draw may not take so that
the notes of the bar being written start only where the bar's row of a rhythm mask allows.

Ids: EOS 1, BAR 2, POSITION 432 .. 559 (432 + g for step g of the bar's 128-step grid).

  TABLE.  onset_table is uint32 [n_rows][4], 1 <= n_rows <= 4096.  A row is a 128-bit mask over the grid: bit g % 32 of word
     g // 32 set means position id 432 + g may be drawn.
  CONTROL WORD.  One int32 per sequence: -1 off, else base + 4096 R with R in 1 .. 64 the cycle length, base in 0 .. 4095 and
     base + R <= n_rows.
  1. ROW OF THE OPEN BAR.  nb = the number of BAR tokens in S = seq[0 : L].  Bar index i = max(nb - 1, 0): the stretch before
     the first BAR uses bar 0's row, as the density rule counts it.  The row is base + (i mod R).  (i counts the bars of a
     prompt too: a primed sequence continues the cycle in phase.)
  2. Banned: every position id whose bit in that row is clear.  An all-clear row is a bar of rest.
  3. DENSITY WAIVER.  density_contract's rule 4 reads "unless END == 560".  With a template it reads "unless no position id
     is left unbanned by the range [432, END) together with the row".  With the template off the row is all ones and the
     waiver is exactly density_contract's.  This coupling is the one place where the rule is more than a bias: without it a
     template combined with a lower bound would end every attempt by Q12 in a bar whose remaining onsets are all masked.

A banned id's y is replaced by -inf in the same select as the note order's, the voice cap's, the density's and the
interval's bans: a draw is the interval draw with bias = -inf at these ids (and, for rule 3, the density's BAR / EOS ban
taken under the new waiver), which is how restate_with_onsets computes it.  The word implies none of the other four."""
import numpy as np

import density_contract as DC
import interval_contract as IC

V = 729
EOS, BAR = 1, 2
POS_LO, POS_HI = 432, 559
GRID = 128
OFF = -1
ROWS_MAX, CYCLE_MAX = 4096, 64


def word(base, cycle):
    """The control word of a template of `cycle` rows that starts at table row `base`."""
    return int(base) + ROWS_MAX * int(cycle)


def row_of(positions):
    """uint32 [4]: the row with the bits of the given grid steps set."""
    r = np.zeros(4, dtype=np.uint32)
    for g in positions:
        g = int(g)
        assert 0 <= g < GRID
        r[g // 32] |= np.uint32(1 << (g % 32))
    return r


def bar_index(seq_row, length):
    """i of rule 1."""
    nb = sum(1 for t in list(seq_row)[:max(int(length), 0)] if int(t) == BAR)
    return max(nb - 1, 0)


def open_row(seq_row, length, ctl, table):
    """The four words of the open bar's row (all ones for an off word)."""
    ctl = int(ctl)
    if ctl < 0:
        return np.full(4, 0xFFFFFFFF, dtype=np.uint32)
    table = np.asarray(table, dtype=np.uint32).reshape(-1, 4)
    base, cyc = ctl % ROWS_MAX, ctl // ROWS_MAX
    assert 1 <= cyc <= CYCLE_MAX and 1 <= len(table) <= ROWS_MAX and base + cyc <= len(table), (ctl, len(table))
    return table[base + bar_index(seq_row, length) % cyc]


def allowed(row, g):
    return bool((int(row[g // 32]) >> (g % 32)) & 1)


def bans(seq_row, length, ctl, table):
    """The sorted list of position ids rule 2 bans for the draw that follows seq_row[0 : length]."""
    if int(ctl) < 0:
        return []
    row = open_row(seq_row, length, ctl, table)
    return [POS_LO + g for g in range(GRID) if not allowed(row, g)]


def position_left(seq_row, length, ctl, table, density_ctl, order_ctl, voice_ctl):
    """Rule 3's test: some position id is banned neither by the range [432, END) nor by the row."""
    end = DC.position_end(seq_row, length, density_ctl, order_ctl, voice_ctl)
    row = open_row(seq_row, length, ctl, table)
    return any(allowed(row, g) for g in range(end - POS_LO, GRID))


def density_bans(seq_row, length, ctl, table, density_ctl, order_ctl, voice_ctl):
    """density_contract.bans under the waiver of rule 3."""
    density_ctl = int(density_ctl)
    if density_ctl < 0:
        return []
    lo, hi = density_ctl & 255, (density_ctl >> 8) & 255
    c = DC.count(seq_row, length)
    out = set()
    if hi >= 1 and c >= hi:
        out |= set(range(POS_LO, POS_HI + 1))
    if lo >= 1 and c < lo and position_left(seq_row, length, ctl, table, density_ctl, order_ctl, voice_ctl):
        out |= {EOS, BAR}
    return sorted(out)


def banned_bias(bias, seq_row, length, ctl, table, density_ctl, order_ctl, voice_ctl):
    """fp32 [V]: the bias row (None: zeros) with -inf at rule 2's ids and at the density's ids under rule 3."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl, table)] = -np.inf
    row[density_bans(seq_row, length, ctl, table, density_ctl, order_ctl, voice_ctl)] = -np.inf
    return row


def restate_with_onsets(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl, interval_ctl, onset_ctl,
                        table, bias=None, **kw):
    """interval_contract.restate_with_interval with the density word OFF (its bans are in the bias, under rule 3) on the
    bias with -inf at the template's ids."""
    return IC.restate_with_interval(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, DC.OFF, interval_ctl,
                                    bias=banned_bias(bias, seq_row, length, onset_ctl, table, density_ctl, order_ctl,
                                                     voice_ctl), **kw)


def onsets_violation(seq, start, rows, drawn_mask=None):
    """The first index i >= start whose POSITION token the template `rows` (uint32 [R][4], base 0, cycle R) would have
    banned given seq[:i] (read FORWARD), None when there is none.  With drawn_mask only the indices with drawn_mask[i] true
    count: seq[i] was drawn, not forced and not part of a prompt."""
    seq = [int(t) for t in seq]
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    w = word(0, len(rows))
    for i in range(max(int(start), 0), len(seq)):
        if drawn_mask is not None and not drawn_mask[i]:
            continue
        if POS_LO <= seq[i] <= POS_HI and seq[i] in bans(seq, i, w, rows):
            return i
    return None
