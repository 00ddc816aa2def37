"""The voice cap restated in plain numpy (no GPU, no package code): which ids a draw may not take so that at most N drawn
notes sound at once and no pitch is struck again while it sounds.

Ids: BAR 2, PITCH 3 .. 130, VELOCITY 131 .. 194, DURATION 304 .. 431, POSITION 432 .. 559.  `word` is the sequence's control
word: -1 off, else N + 256 r with N in 0 .. 128 (0: no cap) and r in {0, 1} (1: no re-striking).  Defined on seq alone when the
sampling stage runs, with L = min(max(length, 0), len(seq_row)) and S = seq_row[0:L]:

  1. A NOTE is an index i with i + 3 < L and S[i], S[i+1], S[i+2], S[i+3] = POSITION, VELOCITY, PITCH, DURATION.  Start
     a = S[i] - 432, length d = S[i+3] - 303 (1 .. 128), pitch S[i+2]; beta = the number of BAR tokens in S[i+4 : L]; its end
     on the current bar's grid is e = min(a + d - 128 beta, 128).  Notes with beta >= 2 are ignored (a + d <= 255).
  2. CAP (N >= 1): E = the N-th largest e over the notes with beta <= 1, with multiplicity; 0 when there are fewer than N
     notes or the value is <= 0.  Banned: ids 432 .. 432 + E - 1.
  3. RE-STRIKE (r = 1): j the largest index with S[j] BAR or POSITION; none: nothing.  g0 = 0 for BAR, else S[j] - 432.
     Banned: the pitch of every note with beta <= 1 and e > g0.

A banned id's y is replaced by -inf in the same select as the note order's bans: a draw is the note-order draw with
bias = -inf at these ids, which is how restate_with_voices computes it."""
import numpy as np

import note_order_contract as NC

V = 729
BAR = 2
PITCH_LO, PITCH_HI = 3, 130
VEL_LO, VEL_HI = 131, 194
DUR_LO, DUR_HI = 304, 431
POS_LO, POS_HI = 432, 559
OFF = -1


def word(n=0, restrike=False):
    """The control word of a cap n (0: none) and the re-strike switch."""
    return int(n) + 256 * int(bool(restrike))


def notes(seq_row, length):
    """[(a, d, pitch, beta, e)] of every note of S, in index order (beta >= 2 included)."""
    L = min(max(int(length), 0), len(seq_row))
    S = [int(t) for t in seq_row[:L]]
    out = []
    for i in range(L - 3):
        if POS_LO <= S[i] <= POS_HI and VEL_LO <= S[i + 1] <= VEL_HI and PITCH_LO <= S[i + 2] <= PITCH_HI \
                and DUR_LO <= S[i + 3] <= DUR_HI:
            a, d = S[i] - POS_LO, S[i + 3] - (DUR_LO - 1)
            beta = sum(1 for t in S[i + 4:L] if t == BAR)
            out.append((a, d, S[i + 2], beta, min(a + d - 128 * beta, 128)))
    return out


def cap_end(seq_row, length, n):
    """E of rule 2 (0 for n == 0)."""
    n = int(n)
    if n < 1:
        return 0
    ends = sorted((e for (_, _, _, beta, e) in notes(seq_row, length) if beta <= 1), reverse=True)
    if len(ends) < n:
        return 0
    return max(ends[n - 1], 0)


def bans(seq_row, length, ctl):
    """The sorted list of ids the voice rule bans for the draw that follows seq_row[0 : length] under control word ctl."""
    ctl = int(ctl)
    if ctl < 0:
        return []
    n, r = ctl & 255, (ctl >> 8) & 1
    L = min(max(int(length), 0), len(seq_row))
    S = [int(t) for t in seq_row[:L]]
    out = set(range(POS_LO, POS_LO + cap_end(seq_row, length, n)))
    if r:
        j = next((i for i in range(L - 1, -1, -1) if S[i] == BAR or POS_LO <= S[i] <= POS_HI), None)
        if j is not None:
            g0 = 0 if S[j] == BAR else S[j] - POS_LO
            out |= {p for (_, _, p, beta, e) in notes(seq_row, length) if beta <= 1 and e > g0}
    return sorted(out)


def banned_bias(bias, seq_row, length, ctl):
    """fp32 [V]: the bias row (None: zeros) with -inf at bans(seq_row, length, ctl)."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl)] = -np.inf
    return row


def restate_with_voices(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, bias=None, **kw):
    """note_order_contract.restate_with_order on the bias with -inf at the voice rule's ids."""
    return NC.restate_with_order(raw, ctl_records, seq_row, length, order_ctl,
                                 bias=banned_bias(bias, seq_row, length, voice_ctl), **kw)
