"""Class-keyed sampling restated in plain numpy (no GPU, no package code): the sampling triple of a draw is picked by the
class of the sequence's previous token, and everything after that is harmony_contract.restate_with_harmony.

A slot's table is 8 rows of (temperature, top_k, top_p), fully composed (no NaN): row c for a draw whose previous token
has class c (grammar_contract.token_class: OTHER, BAR, PITCH, VELOCITY, CHORD, DURATION, POSITION), whatever the slot's
grammar switch says; row 7 is never selected and holds the slot's base triple.  Under the default event grammar the
previous token's class fixes what is drawn next (DRAWN_AFTER): a velocity after a position, a pitch after a velocity, a
duration after a pitch, a group boundary (position, bar, EOS) after anything else."""
import numpy as np

import grammar_contract as GC
import harmony_contract as HC

NAMES = ("other", "bar", "pitch", "velocity", "chord", "duration", "position")
DRAWN_AFTER = {"velocity": ("position",), "pitch": ("velocity",), "duration": ("pitch",),
               "boundary": ("other", "bar", "chord", "duration")}
# the ids each `drawn` name stands for: the only finite entries of the default grammar's rows it maps to
DRAWN_IDS = {"velocity": range(131, 195), "pitch": range(3, 131), "duration": range(304, 432),
             "boundary": [1, 2] + list(range(432, 560))}


def compose(table, base):
    """A NaN-table [8][3] over a base triple: the table's entry where it is not NaN, the base value elsewhere, row 7 the
    base triple.  float64 [8][3]."""
    t = np.array(table, dtype=np.float64)
    out = np.where(np.isnan(t), np.asarray(base, dtype=np.float64)[None, :], t)
    out[7] = base
    return out


def selected(ctl, prev):
    """The triple (temperature, top_k, top_p) of a draw whose previous token is `prev`."""
    t, k, p = np.asarray(ctl)[GC.token_class(int(prev))]
    return float(np.float32(t)), int(k), float(np.float32(p))


def restate_with_classes(raw, ctl, wrong=None, bias=None, u=0.5, gram=None, prev=0, gram_on=True, harm=None, tokens=(),
                         harm_on=True):
    """harmony_contract.restate_with_harmony with the triple picked by token_class(prev)."""
    t, k, p = selected(ctl, prev)
    return HC.restate_with_harmony(raw, t, k, p, wrong, bias, u, gram=gram, prev=prev, gram_on=gram_on, harm=harm,
                                   tokens=tokens, harm_on=harm_on)
