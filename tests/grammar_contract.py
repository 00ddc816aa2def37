"""The event grammar restated in plain numpy (no GPU, no package code): the class of a token id, the default table, the
row the sampling step draws from with a grammar, and the parser that says whether a token list is a chain of the groups
the reference's token-to-MIDI step keeps (commu/preprocessor/encoder/encoder_utils.py:385-419):

    BAR | EOS (last token) | POSITION, CHORD | POSITION, VELOCITY, PITCH, DURATION

With x = raw / temperature (the raw row for temperature 0) and c the class of the sequence's previous token, the softmax
sees y = (x + bias) + gram[c], two fp32 adds in this order; row 7 (zeros) for a sequence whose grammar is off.  Everything
after that is logit_bias_contract.restate."""
import numpy as np

import logit_bias_contract as LB

V = 729
OTHER, BAR, PITCH, VELOCITY, CHORD, DURATION, POSITION = range(7)
OFF_ROW = 7
NAMES = ("OTHER", "BAR", "PITCH", "VELOCITY", "CHORD", "DURATION", "POSITION")
# first id of every range, in id order: pad / EOS, BAR, pitches, velocities, chords, durations, positions, meta
EDGES = ((0, OTHER), (2, BAR), (3, PITCH), (131, VELOCITY), (195, CHORD), (304, DURATION), (432, POSITION), (560, OTHER))
# every id at which the class changes, and the id before it
EDGE_IDS = {0: OTHER, 1: OTHER, 2: BAR, 3: PITCH, 130: PITCH, 131: VELOCITY, 194: VELOCITY, 195: CHORD, 303: CHORD,
            304: DURATION, 431: DURATION, 432: POSITION, 559: POSITION, 560: OTHER, 728: OTHER}


def token_class(t):
    c = OTHER
    for first, cls in EDGES:
        if t >= first:
            c = cls
    return c


def default_table(width=768):
    g = np.full((8, width), -np.inf, dtype=np.float32)
    g[OFF_ROW] = 0
    g[:, 0] = 0
    g[:, V:] = 0
    boundary = [1, 2] + list(range(432, 560))
    for c in (OTHER, BAR, CHORD, DURATION):
        g[c, boundary] = 0
    g[POSITION, 131:195] = 0
    g[VELOCITY, 3:131] = 0
    g[PITCH, 304:432] = 0
    return g


def restate_with_grammar(raw, temperature, top_k, top_p=1.0, wrong=None, bias=None, u=0.5, gram=None, prev=0, on=True):
    """logit_bias_contract.restate fed (x + bias) + gram[c] in that fp32 order: the two adds are folded into the one
    `bias` row restate adds to x, which is exact only for the first -- so the first is made here, on x as restate will
    compute it, and the second is handed over."""
    raw = np.asarray(raw)
    if gram is None:
        return LB.restate(raw, temperature, top_k, top_p, wrong, bias, u)
    row = np.asarray(gram)[token_class(int(prev)) if on else OFF_ROW]
    assert row.dtype == np.float32
    t32 = np.float32(temperature)
    x = raw[:V].copy()
    if t32 != 0:
        x[1:] = raw[1:V] / t32
    xb = x if bias is None else (x + np.asarray(bias, dtype=np.float32)[:V]).astype(np.float32)
    # restate computes x again and adds its `bias` argument once: give it xb as the raw row at temperature 1 ...
    res = LB.restate(np.concatenate([xb, raw[V:]]).astype(np.float32), 1.0 if t32 != 0 else 0.0, top_k, top_p, wrong,
                     row[:V].astype(np.float32), u)
    # ... and put back what the call writes: x, never y
    written = raw.copy()
    written[:V] = x
    res.written = written
    return res


def parse_events(seq, start):
    """Index of the first token of seq[start:] that does not continue a group, None when every token does.  A note group
    cut by the end of the list is fine; EOS is a group of its own and must be the last token."""
    i, n = start, len(seq)
    cls = [token_class(int(t)) for t in seq]
    while i < n:
        if cls[i] == BAR:
            i += 1
        elif int(seq[i]) == 1:
            return None if i == n - 1 else i + 1
        elif cls[i] == POSITION:
            if i + 1 == n:
                return None
            if cls[i + 1] == CHORD:
                i += 2
                continue
            for k, want in enumerate((VELOCITY, PITCH, DURATION), 1):
                if i + k == n:
                    return None
                if cls[i + k] != want:
                    return i + k
            i += 4
        else:
            return i
    return None
