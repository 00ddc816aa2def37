"""The note-order constraint restated in plain numpy (no GPU, no package code): which ids a draw may not take given what
the sequence already holds at its current position, and the row the sampling step draws from.

Defined on seq alone when the sampling stage runs.  ctl is the sequence's control word: -1 off, 0 on, n in 1 .. 128 on
with at most n notes per position.  With L = min(max(length, 0), len(seq_row)) and S = seq_row[0:L]:

  1. j is the largest index with S[j] == BAR (2) or a POSITION token (432 .. 559); none, or BAR: nothing is banned.
  2. p = S[j]; s is one past the largest i < j with S[i] BAR or a POSITION token != p (0 when there is none); the run is
     S[s:L] -- everything placed at the current position of the current bar, chord groups and repeated `Position p`
     tokens included.
  3. D is the PITCH tokens (3 .. 130) of the run, n their number counted with multiplicity.
  4. banned: ids 432 .. p - 1, every id in D, and p itself when ctl >= 1 and n >= ctl.

A banned id's y is replaced by -inf after the harmony term: y = banned ? -inf : ((x + bias) + gram) + harm.  Since +inf and
NaN are refused in every table, that is the row of class_sampling_contract.restate_with_classes with bias = -inf at the
banned ids, which is how restate_with_order computes it."""
import numpy as np

import class_sampling_contract as CC

V = 729
BAR = 2
PITCH_LO, PITCH_HI = 3, 130
POS_LO, POS_HI = 432, 559
OFF = -1


def _breaker(t):
    return t == BAR or POS_LO <= t <= POS_HI


def bans(seq_row, length, ctl):
    """The sorted list of banned ids for the draw that follows seq_row[0 : length] under control word ctl."""
    ctl = int(ctl)
    if ctl < 0:
        return []
    L = min(max(int(length), 0), len(seq_row))
    S = [int(t) for t in seq_row[:L]]
    j = next((i for i in range(L - 1, -1, -1) if _breaker(S[i])), None)
    if j is None or S[j] == BAR:
        return []
    p = S[j]
    s = next((i + 1 for i in range(j - 1, -1, -1) if _breaker(S[i]) and S[i] != p), 0)
    run = S[s:L]
    pitches = [t for t in run if PITCH_LO <= t <= PITCH_HI]
    out = set(range(POS_LO, p)) | set(pitches)
    if ctl >= 1 and len(pitches) >= ctl:
        out.add(p)
    return sorted(out)


def banned_bias(bias, seq_row, length, ctl):
    """fp32 [V]: the bias row (None: zeros) with -inf at bans(seq_row, length, ctl)."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl)] = -np.inf
    return row


def restate_with_order(raw, ctl_records, seq_row, length, order_ctl, wrong=None, bias=None, u=0.5, gram=None, gram_on=True,
                       harm=None, harm_on=True):
    """class_sampling_contract.restate_with_classes on the bias with -inf at the banned ids.  The previous token (the key of
    the grammar row and of the class record) is seq_row[min(max(length, 1), len(seq_row)) - 1], the tokens that key the
    harmony row are seq_row[0 : length]."""
    n = len(seq_row)
    prev = int(seq_row[min(max(int(length), 1), n) - 1])
    tokens = [int(t) for t in seq_row[:min(max(int(length), 0), n)]]
    return CC.restate_with_classes(raw, ctl_records, wrong=wrong, bias=banned_bias(bias, seq_row, length, order_ctl), u=u,
                                   gram=gram, prev=prev, gram_on=gram_on, harm=harm, tokens=tokens, harm_on=harm_on)
