"""The harmony constraint restated in plain numpy (no GPU, no package code): which chord a draw is keyed by, the pitch
classes of the 109 chord tokens spelled out, the default table, and the row the sampling step draws from.

Defined on seq alone: the chord of a draw is the last token t with 195 <= t <= 303 in the sequence's tokens when the
sampling stage runs; its row is r = t - 195 (rows 0 .. 107: 12 roots x 9 qualities, row 108: Chord_NN), r = 109 while there
is none, r = 110 (zeros) for a sequence whose switch is off.  With x = raw / temperature (the raw row for temperature 0)
and c the class of the previous token the softmax sees

    y[id] = ((x[id] + bias[id]) + gram[c][id]) + harm[r][(id - 3) mod 12]        for 3 <= id <= 130

three fp32 adds in this order, and y[id] = (x[id] + bias[id]) + gram[c][id] for every other id.  Column pc of a row is MIDI
pitch class pc (C = 0); token id is MIDI pitch id - 3: the vocabulary list of the reference names id 3 + n "Note On_n"
(commu/preprocessor/encoder/event_tokens.py:3-130, ids = list index + 2 by encoder_utils.py:55) and its write_midi hands
that n to miditoolkit.Note as the pitch (encoder_utils.py:411, :443); ids 195 .. 303 are "Chord_a" .. "Chord_NN"
(event_tokens.py:195-303).  Everything after y is logit_bias_contract.restate."""
import numpy as np

import grammar_contract as GC
import logit_bias_contract as LB

V = 729
CHORD_LO, CHORD_HI = 195, 303
PITCH_LO, PITCH_HI = 3, 130
ROW_NN, ROW_NONE, ROW_OFF, ROWS = 108, 109, 110, 111

# the chord tokens in id order (195, 196, ...) with their pitch classes written out, C = 0 ... B = 11
CHORDS = (
    ("a", (1, 4, 9)), ("a7", (1, 4, 7, 9)), ("a+", (1, 5, 9)), ("adim", (0, 3, 9)), ("am", (0, 4, 9)), ("am7", (0, 4, 7, 9)),
    ("am7b5", (0, 3, 7, 9)), ("amaj7", (1, 4, 8, 9)), ("asus4", (2, 4, 9)),
    ("a#", (2, 5, 10)), ("a#7", (2, 5, 8, 10)), ("a#+", (2, 6, 10)), ("a#dim", (1, 4, 10)), ("a#m", (1, 5, 10)),
    ("a#m7", (1, 5, 8, 10)), ("a#m7b5", (1, 4, 8, 10)), ("a#maj7", (2, 5, 9, 10)), ("a#sus4", (3, 5, 10)),
    ("b", (3, 6, 11)), ("b7", (3, 6, 9, 11)), ("b+", (3, 7, 11)), ("bdim", (2, 5, 11)), ("bm", (2, 6, 11)),
    ("bm7", (2, 6, 9, 11)), ("bm7b5", (2, 5, 9, 11)), ("bmaj7", (3, 6, 10, 11)), ("bsus4", (4, 6, 11)),
    ("c", (0, 4, 7)), ("c7", (0, 4, 7, 10)), ("c+", (0, 4, 8)), ("cdim", (0, 3, 6)), ("cm", (0, 3, 7)), ("cm7", (0, 3, 7, 10)),
    ("cm7b5", (0, 3, 6, 10)), ("cmaj7", (0, 4, 7, 11)), ("csus4", (0, 5, 7)),
    ("c#", (1, 5, 8)), ("c#7", (1, 5, 8, 11)), ("c#+", (1, 5, 9)), ("c#dim", (1, 4, 7)), ("c#m", (1, 4, 8)),
    ("c#m7", (1, 4, 8, 11)), ("c#m7b5", (1, 4, 7, 11)), ("c#maj7", (0, 1, 5, 8)), ("c#sus4", (1, 6, 8)),
    ("d", (2, 6, 9)), ("d7", (0, 2, 6, 9)), ("d+", (2, 6, 10)), ("ddim", (2, 5, 8)), ("dm", (2, 5, 9)), ("dm7", (0, 2, 5, 9)),
    ("dm7b5", (0, 2, 5, 8)), ("dmaj7", (1, 2, 6, 9)), ("dsus4", (2, 7, 9)),
    ("d#", (3, 7, 10)), ("d#7", (1, 3, 7, 10)), ("d#+", (3, 7, 11)), ("d#dim", (3, 6, 9)), ("d#m", (3, 6, 10)),
    ("d#m7", (1, 3, 6, 10)), ("d#m7b5", (1, 3, 6, 9)), ("d#maj7", (2, 3, 7, 10)), ("d#sus4", (3, 8, 10)),
    ("e", (4, 8, 11)), ("e7", (2, 4, 8, 11)), ("e+", (0, 4, 8)), ("edim", (4, 7, 10)), ("em", (4, 7, 11)),
    ("em7", (2, 4, 7, 11)), ("em7b5", (2, 4, 7, 10)), ("emaj7", (3, 4, 8, 11)), ("esus4", (4, 9, 11)),
    ("f", (0, 5, 9)), ("f7", (0, 3, 5, 9)), ("f+", (1, 5, 9)), ("fdim", (5, 8, 11)), ("fm", (0, 5, 8)), ("fm7", (0, 3, 5, 8)),
    ("fm7b5", (3, 5, 8, 11)), ("fmaj7", (0, 4, 5, 9)), ("fsus4", (0, 5, 10)),
    ("f#", (1, 6, 10)), ("f#7", (1, 4, 6, 10)), ("f#+", (2, 6, 10)), ("f#dim", (0, 6, 9)), ("f#m", (1, 6, 9)),
    ("f#m7", (1, 4, 6, 9)), ("f#m7b5", (0, 4, 6, 9)), ("f#maj7", (1, 5, 6, 10)), ("f#sus4", (1, 6, 11)),
    ("g", (2, 7, 11)), ("g7", (2, 5, 7, 11)), ("g+", (3, 7, 11)), ("gdim", (1, 7, 10)), ("gm", (2, 7, 10)),
    ("gm7", (2, 5, 7, 10)), ("gm7b5", (1, 5, 7, 10)), ("gmaj7", (2, 6, 7, 11)), ("gsus4", (0, 2, 7)),
    ("g#", (0, 3, 8)), ("g#7", (0, 3, 6, 8)), ("g#+", (0, 4, 8)), ("g#dim", (2, 8, 11)), ("g#m", (3, 8, 11)),
    ("g#m7", (3, 6, 8, 11)), ("g#m7b5", (2, 6, 8, 11)), ("g#maj7", (0, 3, 7, 8)), ("g#sus4", (1, 3, 8)),
    ("NN", ()),
)
assert len(CHORDS) == CHORD_HI - CHORD_LO + 1 == 109


def pitch_classes(token):
    """The pitch classes of chord token 195 .. 303 (the empty set for Chord_NN: no statement)."""
    return frozenset(CHORDS[token - CHORD_LO][1])


def chord_row(tokens, on=True):
    """The table row of a draw made when the sequence holds `tokens` (the definition on seq)."""
    if not on:
        return ROW_OFF
    for t in reversed(list(tokens)):
        if CHORD_LO <= int(t) <= CHORD_HI:
            return int(t) - CHORD_LO
    return ROW_NONE


def default_table(outside=-np.inf, extra=()):
    """fp32 [111][16]: chord rows hold 0 at the chord's pitch classes (and at root + every interval of `extra`) and
    `outside` elsewhere; rows 108 (NN), 109 (no chord yet) and 110 (off) and the pad columns 12 .. 15 are zeros."""
    t = np.zeros((ROWS, 16), dtype=np.float32)
    for r, (name, pcs) in enumerate(CHORDS[:ROW_NN]):
        root = (9 + r // 9) % 12                  # the roots run a, a#, b, c, ...: a is pitch class 9
        allowed = set(pcs) | {(root + int(i)) % 12 for i in extra}
        for pc in range(12):
            t[r, pc] = 0.0 if pc in allowed else outside
    return t


def wide_row(harm, r):
    """Row r of a [111][>= 12] table laid over the vocabulary: harm[r][(id - 3) mod 12] at the pitch ids, 0 elsewhere
    (where the kernel makes no add at all: adding +0 changes no value)."""
    row = np.zeros(V, dtype=np.float32)
    ids = np.arange(PITCH_LO, PITCH_HI + 1)
    row[ids] = np.asarray(harm, dtype=np.float32)[r, (ids - 3) % 12]
    return row


def restate_with_harmony(raw, temperature, top_k, top_p=1.0, wrong=None, bias=None, u=0.5, gram=None, prev=0, gram_on=True,
                         harm=None, tokens=(), harm_on=True):
    """logit_bias_contract.restate fed ((x + bias) + gram[c]) + harm[r] in that fp32 order.  The first two adds are made
    as grammar_contract.restate_with_grammar makes them (on x as restate will compute it); the third is handed over as
    the one row restate adds.  tokens: the sequence when the stage runs (its last chord keys the row)."""
    raw = np.asarray(raw)
    if harm is None:
        return GC.restate_with_grammar(raw, temperature, top_k, top_p, wrong, bias, u, gram, prev, gram_on)
    t32 = np.float32(temperature)
    x = raw[:V].copy()
    if t32 != 0:
        x[1:] = raw[1:V] / t32
    xb = x if bias is None else (x + np.asarray(bias, dtype=np.float32)[:V]).astype(np.float32)
    if gram is not None:
        g = np.asarray(gram)[GC.token_class(int(prev)) if gram_on else GC.OFF_ROW]
        assert g.dtype == np.float32
        xb = (xb + g[:V]).astype(np.float32)
    row = wide_row(harm, chord_row(tokens, harm_on))
    res = LB.restate(np.concatenate([xb, raw[V:]]).astype(np.float32), 1.0 if t32 != 0 else 0.0, top_k, top_p, wrong, row, u)
    written = raw.copy()
    written[:V] = x
    res.written = written
    return res
