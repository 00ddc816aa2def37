"""The melodic interval restated in plain numpy (no GPU, no package code): which ids a draw may not take so that the pitch
drawn next lies within a cap of the pitch of the sequence's last note.

Ids: PITCH 3 .. 130, one id one semitone.  `ctl` is the sequence's control word: -1 off, else up + 256 down + 65536 u with
up, down in 0 .. 127 (0: that bound is not set) and u in {0, 1} (1: the pitch may not repeat); word 0 is on and bans nothing.
Defined on seq alone when the sampling stage runs, with L, S, NOTE and beta exactly as voices_contract defines them:

  1. REFERENCE NOTE: the note with beta <= 1 whose index i is largest; q = S[i+2] its pitch token.  None (the first note of a
     sequence, a line that rested for a whole bar or more): nothing is banned.
  2. UP (up >= 1).  Banned: ids q + up + 1 .. 130.
  3. DOWN (down >= 1).  Banned: ids 3 .. q - down - 1.
  4. UNISON (u = 1).  Banned: id q.

A banned id's y is replaced by -inf in the same select as the note order's, the voice cap's and the density's bans: a draw is
the density draw with bias = -inf at these ids, which is how restate_with_interval computes it.  The word implies none of
the other three."""
import numpy as np

import density_contract as DC
import voices_contract as VC

V = 729
PITCH_LO, PITCH_HI = 3, 130
OFF = -1


def word(up=0, down=0, no_repeat=False):
    """The control word of a cap upwards and downwards (0: not set) and the unison switch."""
    return int(up) + 256 * int(down) + 65536 * int(bool(no_repeat))


def reference_pitch(seq_row, length):
    """q of rule 1, None when there is no reference note."""
    near = [p for (_, _, p, beta, _) in VC.notes(seq_row, length) if beta <= 1]          # (index order)
    return near[-1] if near else None


def bans(seq_row, length, ctl):
    """The sorted list of ids the interval rule bans for the draw that follows seq_row[0 : length] under control word ctl."""
    ctl = int(ctl)
    if ctl < 0:
        return []
    up, down, u = ctl & 255, (ctl >> 8) & 255, (ctl >> 16) & 1
    q = reference_pitch(seq_row, length)
    if q is None:
        return []
    out = set()
    if up >= 1:
        out |= set(range(q + up + 1, PITCH_HI + 1))
    if down >= 1:
        out |= set(range(PITCH_LO, q - down))
    if u:
        out.add(q)
    return sorted(out)


def banned_bias(bias, seq_row, length, ctl):
    """fp32 [V]: the bias row (None: zeros) with -inf at bans(seq_row, length, ctl)."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl)] = -np.inf
    return row


def restate_with_interval(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl, interval_ctl, bias=None,
                          **kw):
    """density_contract.restate_with_density on the bias with -inf at the interval rule's ids."""
    return DC.restate_with_density(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl,
                                   bias=banned_bias(bias, seq_row, length, interval_ctl), **kw)


def interval_violation(seq, start, up=0, down=0, no_repeat=False, drawn_mask=None):
    """The first index i >= start whose token the rule would have banned given seq[:i] (read FORWARD: bans(seq, i, word)),
    None when there is none.  With drawn_mask only the indices with drawn_mask[i] true count: seq[i] was drawn, not forced
    and not part of a prompt."""
    seq = [int(t) for t in seq]
    w = word(up, down, no_repeat)
    for i in range(max(int(start), 0), len(seq)):
        if drawn_mask is not None and not drawn_mask[i]:
            continue
        if PITCH_LO <= seq[i] <= PITCH_HI and seq[i] in bans(seq, i, w):
            return i
    return None
