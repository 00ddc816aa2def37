"""The note density restated in plain numpy (no GPU, no package code): which ids a draw may not take so that the bar being
written holds at least lo and at most hi notes.

Ids: EOS 1, BAR 2, POSITION 432 .. 559.  `ctl` is the sequence's control word: -1 off, else lo + 256 hi with lo, hi in
0 .. 255 (0: that bound is not set; hi >= lo where both are).  Defined on seq alone when the sampling stage runs, with L, S,
NOTE and beta exactly as voices_contract defines them:

  1. C = the number of notes with beta == 0: the complete POSITION, VELOCITY, PITCH, DURATION groups behind the last BAR of S,
     or anywhere in S when it holds no BAR.
  2. UPPER (hi >= 1 and C >= hi).  Banned: every POSITION id 432 .. 559.
  3. The position range of the three rules together is [432, END): END = the maximum of 432, the note order's end (one past
     its highest banned position), the voice cap's end 432 + E, and 560 when rule 2 fired.
  4. LOWER (lo >= 1 and C < lo).  Banned: BAR (2) and EOS (1) -- unless END == 560 (no position is left: the bar may end).

A banned id's y is replaced by -inf in the same select as the note order's and the voice cap's bans: a draw is the voices
draw with bias = -inf at these ids, which is how restate_with_density computes it."""
import numpy as np

import note_order_contract as NC
import voices_contract as VC

V = 729
EOS, BAR = 1, 2
POS_LO, POS_HI = 432, 559
OFF = -1


def word(lo=0, hi=0):
    """The control word of a lower and an upper bound (0: not set)."""
    return int(lo) + 256 * int(hi)


def count(seq_row, length):
    """C of rule 1."""
    return sum(1 for (_, _, _, beta, _) in VC.notes(seq_row, length) if beta == 0)


def position_end(seq_row, length, ctl, order_ctl, voice_ctl):
    """END of rule 3."""
    ctl, voice_ctl = int(ctl), int(voice_ctl)
    ends = [POS_LO] + [t + 1 for t in NC.bans(seq_row, length, order_ctl) if POS_LO <= t <= POS_HI]
    if voice_ctl >= 0:
        ends.append(POS_LO + VC.cap_end(seq_row, length, voice_ctl & 255))
    if ctl >= 0 and (ctl >> 8) & 255 >= 1 and count(seq_row, length) >= (ctl >> 8) & 255:
        ends.append(POS_HI + 1)
    return max(ends)


def bans(seq_row, length, ctl, order_ctl, voice_ctl):
    """The sorted list of ids the density rule bans for the draw that follows seq_row[0 : length] under control word ctl; the
    waiver of rule 4 needs the other two rules' position ends, hence their words."""
    ctl = int(ctl)
    if ctl < 0:
        return []
    lo, hi = ctl & 255, (ctl >> 8) & 255
    c = count(seq_row, length)
    out = set()
    if hi >= 1 and c >= hi:
        out |= set(range(POS_LO, POS_HI + 1))
    if lo >= 1 and c < lo and position_end(seq_row, length, ctl, order_ctl, voice_ctl) != POS_HI + 1:
        out |= {EOS, BAR}
    return sorted(out)


def banned_bias(bias, seq_row, length, ctl, order_ctl, voice_ctl):
    """fp32 [V]: the bias row (None: zeros) with -inf at bans(seq_row, length, ctl, order_ctl, voice_ctl)."""
    row = np.zeros(V, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)[:V].copy()
    row[bans(seq_row, length, ctl, order_ctl, voice_ctl)] = -np.inf
    return row


def restate_with_density(raw, ctl_records, seq_row, length, order_ctl, voice_ctl, density_ctl, bias=None, **kw):
    """voices_contract.restate_with_voices on the bias with -inf at the density rule's ids."""
    return VC.restate_with_voices(raw, ctl_records, seq_row, length, order_ctl, voice_ctl,
                                  bias=banned_bias(bias, seq_row, length, density_ctl, order_ctl, voice_ctl), **kw)


def density_violation(seq, start, lo, hi, drawn_mask, order_ctl=0, voice_ctl=0):
    """The first index i >= start at which seq breaks the bounds by a DRAW (drawn_mask[i] true: seq[i] was drawn, not forced
    and not part of a prompt), None when there is none.  Read FORWARD, one bar at a time, with a note counted when its
    DURATION arrives -- not the backward count of `count`:
      - a drawn BAR or EOS at i while the bar it closes holds fewer than lo notes, although a position was still free (the
        position range of the note order under order_ctl and the voice cap under voice_ctl -- the words set_density switches
        on by default -- did not cover all 128 positions of seq[:i]);
      - the POSITION at i was drawn and its note is the (hi + 1)-th of its bar or a later one.
    A bar that a forced BAR or EOS closes, or that the end of seq cuts, is none; a note on a forced position is none."""
    seq = [int(t) for t in seq]
    lo, hi = int(lo), int(hi)
    n = 0                                   # the complete notes of the bar so far
    found = []
    for i, t in enumerate(seq):
        if t == BAR or t == EOS:
            if i >= start and drawn_mask[i] and lo >= 1 and n < lo \
                    and position_end(seq, i, OFF, order_ctl, voice_ctl) != POS_HI + 1:
                found.append(i)
            if t == BAR:
                n = 0
        elif i >= 3 and VC.DUR_LO <= t <= VC.DUR_HI and VC.PITCH_LO <= seq[i - 1] <= VC.PITCH_HI \
                and VC.VEL_LO <= seq[i - 2] <= VC.VEL_HI and POS_LO <= seq[i - 3] <= POS_HI:
            n += 1
            if hi >= 1 and n > hi and i - 3 >= start and drawn_mask[i - 3]:
                found.append(i - 3)
    return min(found) if found else None
