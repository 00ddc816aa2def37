"""Batched autoregressive generation: `num_generate` sequences decoded in parallel on one GPU with a per-layer
K/V cache, ragged per-sequence lengths and the reference's chord / bar forcing applied per sequence
(commu/midi_generator/midi_inferrer.py:239-354; the reference itself generates one sequence at a time, batch 1).

The whole loop iteration lives on the device: the forcing rules are a per-sequence state record advanced by two
small kernels (csrc/forcing.hip), between them the batched decode step and the sampling kernel.  One iteration =
one replay of a hipGraph; the host only polls the `done` flags every few iterations.  Per iteration every live
sequence does exactly what one iteration of the reference's `generate_sequence` does for it: at most one model
step (memory kept or discarded, quirks Q3/Q4) and at most one draw (from fresh logits, or from the logits already
divided by the temperature when the previous draw was a rejected chord, quirk Q5).
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import json
import math
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import CommuHipError, DecodeLoopArgs, call, struct_args
from .midi_generator.midi_inferrer import TOKEN_OFFSET, ForcingReport, token_class  # noqa: F401

BF16, F32 = torch.bfloat16, torch.float32
VPAD = 768
# decode step: everything after a layer's attention as one launch (commu_decode_layer_tail) where the shape is supported;
# False: one launch per Linear / LayerNorm (the only path for other shapes)
USE_LAYER_TAIL = True


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _per_row(x, B: int, name: str):
    """x broadcast to B float64 values: a number, or a sequence of exactly B numbers."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if np.ndim(x) == 0:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating, np.ndarray)):
            raise CommuHipError(f"{name}: a number or a sequence of {B} numbers expected, got {x!r}")
        return np.full(B, x, dtype=np.float64)
    try:
        a = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise CommuHipError(f"{name}: a number or a sequence of {B} numbers expected, got {x!r}") from None
    if a.ndim != 1 or a.shape[0] != B:
        raise CommuHipError(f"{name}: {B} values expected (one per sequence), got shape {a.shape}")
    return a


def sampling_rows(B: int, temperature, top_k, top_p=1.0):
    """The sampling controls of B sequences as three numpy arrays (float32 temperature, int32 top_k, float32 top_p): each
    argument is a number for all sequences or a sequence of B numbers.  Pure host code; raises CommuHipError on a
    negative or non-finite temperature, a top_k outside [1, 729] (or not an integer), a top_p outside (0, 1] and on a wrong
    length -- the kernels do not validate what the arrays hold."""
    B = int(B)
    t = _per_row(temperature, B, "temperature")
    k = _per_row(top_k, B, "top_k")
    p = _per_row(top_p, B, "top_p")
    V = TOKEN_OFFSET.VOCAB_SIZE
    if not bool(np.all(np.isfinite(t) & (t >= 0))):
        raise CommuHipError(f"temperature: finite values >= 0 expected (0 = greedy), got {t[~(np.isfinite(t) & (t >= 0))][0]}")
    ok = np.isfinite(k) & (k == np.floor(k)) & (k >= 1) & (k <= V)
    if not bool(np.all(ok)):
        raise CommuHipError(f"top_k: integers in [1, {V}] expected, got {k[~ok][0]}")
    ok = (p > 0) & (p <= 1)          # (NaN fails both comparisons)
    if not bool(np.all(ok)):
        raise CommuHipError(f"top_p: values in (0, 1] expected (1 = off), got {p[~ok][0]}")
    return t.astype(np.float32), k.astype(np.int32), p.astype(np.float32)


# ---- constraints on what a slot may draw: one additive fp32 row per slot, applied by the sampling step to the row its
# softmax sees (logits / temperature + bias, before top-k; commu_sample_args.bias).  A finite entry re-weights an id,
# -inf bans it.  Rows are VPAD wide like the logits rows; ids 0 and >= 729 are never drawn and their entries are ignored.
N_VELOCITY = TOKEN_OFFSET.CHORD_START - TOKEN_OFFSET.NOTE_VELOCITY          # 64 velocity tokens, one per bin of 2
N_PITCH = TOKEN_OFFSET.NOTE_VELOCITY - TOKEN_OFFSET.PITCH                   # 128 pitch tokens, MIDI note numbers


def _check_bias_row(row, what="logit bias"):
    """A constraint row as float32 [VPAD]: [729] or [768] values, no NaN, no +inf, and something left to draw."""
    V = TOKEN_OFFSET.VOCAB_SIZE
    try:
        a = np.asarray(row, dtype=np.float32)
    except (TypeError, ValueError):
        raise CommuHipError(f"{what}: a row of {V} (or {VPAD}) numbers expected, got {type(row).__name__}") from None
    if a.ndim != 1 or a.shape[0] not in (V, VPAD):
        raise CommuHipError(f"{what}: a row of {V} (or {VPAD}) numbers expected, got shape {a.shape}")
    bad = np.isnan(a[:V]) | (a[:V] == np.inf)
    if bool(bad.any()):
        i = int(np.flatnonzero(bad)[0])
        raise CommuHipError(f"{what}: entry {i} is {a[i]}; finite values or -inf (a ban) expected")
    if not bool(np.isfinite(a[1:V]).any()):
        raise CommuHipError(f"{what}: all of ids 1 .. {V - 1} are banned, nothing could be drawn")
    out = np.zeros(VPAD, dtype=np.float32)
    out[:V] = a[:V]
    return out


def token_constraints(ban=(), bias=None, pitch_range=None, velocity_range=None):
    """A constraint row for ForcedDecoder.set_logit_bias / generate(logit_bias=): float32 [768], 0 where an id is left
    alone, a finite re-weighting where `bias` names one, -inf where it is banned.  Pure host code.
    ban: token ids that must not be drawn.  bias: {id: number} (or (id, number) pairs), added to the id's logit on the
    scale the softmax sees (after the division by the temperature); -inf is a ban.
    pitch_range=(lo, hi): MIDI note numbers; the pitch tokens TOKEN_OFFSET.PITCH + p with p outside [lo, hi] are banned.
    velocity_range=(lo, hi): MIDI velocities; of the 64 velocity tokens TOKEN_OFFSET.NOTE_VELOCITY + bin the bins outside
    [floor(lo / 2), ceil(hi / 2)] are banned -- the mapping of the min_velocity / max_velocity meta tokens (meta.encode_meta).
    Raises CommuHipError on an id outside [1, 729), NaN or +inf, an empty range, and a row that bans everything."""
    V = TOKEN_OFFSET.VOCAB_SIZE
    row = np.zeros(VPAD, dtype=np.float32)

    def tid(t, what):
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer, str)):
            raise CommuHipError(f"{what}: a token id in [1, {V}) expected, got {t!r}")
        try:
            i = int(t)          # (JSON object keys arrive as strings)
        except ValueError:
            raise CommuHipError(f"{what}: a token id in [1, {V}) expected, got {t!r}") from None
        if not 1 <= i < V:
            raise CommuHipError(f"{what}: token id {i} is outside [1, {V})")
        return i

    def span(r, what, n, lo_of, hi_of):
        try:
            lo, hi = r
            lo, hi = float(lo), float(hi)
        except (TypeError, ValueError):
            raise CommuHipError(f"{what}: a pair (lo, hi) of numbers expected, got {r!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
            raise CommuHipError(f"{what}: ({lo:g}, {hi:g}) is empty")
        a, b = max(lo_of(lo), 0), min(hi_of(hi), n - 1)
        if a > b or hi < 0 or lo > 127:
            raise CommuHipError(f"{what}: ({lo:g}, {hi:g}) leaves none of the {n} tokens (values 0 .. 127)")
        return a, b

    if pitch_range is not None:
        a, b = span(pitch_range, "pitch_range", N_PITCH, math.ceil, math.floor)
        row[TOKEN_OFFSET.PITCH:TOKEN_OFFSET.PITCH + a] = -np.inf
        row[TOKEN_OFFSET.PITCH + b + 1:TOKEN_OFFSET.NOTE_VELOCITY] = -np.inf
    if velocity_range is not None:
        a, b = span(velocity_range, "velocity_range", N_VELOCITY, lambda v: math.floor(v / 2), lambda v: math.ceil(v / 2))
        row[TOKEN_OFFSET.NOTE_VELOCITY:TOKEN_OFFSET.NOTE_VELOCITY + a] = -np.inf
        row[TOKEN_OFFSET.NOTE_VELOCITY + b + 1:TOKEN_OFFSET.CHORD_START] = -np.inf
    if bias is not None:
        for t, v in (bias.items() if hasattr(bias, "items") else bias):
            i = tid(t, "bias")
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise CommuHipError(f"bias: a number expected for token {i}, got {v!r}")
            v = float(v)
            if math.isnan(v) or v == math.inf:
                raise CommuHipError(f"bias: token {i} has {v}; a finite value or -inf (a ban) expected")
            if row[i] != -np.inf:          # (a ban stays a ban)
                row[i] = np.float32(v)
    for t in ban:
        row[tid(t, "ban")] = -np.inf
    return _check_bias_row(row, "token_constraints")


def read_logit_bias(doc):
    """The {"ban": [ids], "bias": {"id": number}} document of generate.py --logit_bias as token_constraints arguments
    (ban, bias); either key may be missing.  Raises CommuHipError on anything else."""
    if not isinstance(doc, dict) or not set(doc) <= {"ban", "bias"}:
        raise CommuHipError('logit bias: a JSON object {"ban": [ids], "bias": {"id": number}} expected, got '
                            + (f"keys {sorted(doc)}" if isinstance(doc, dict) else type(doc).__name__))
    ban, bias = doc.get("ban", []), doc.get("bias", {})
    if not isinstance(ban, list):
        raise CommuHipError(f'logit bias: "ban" is a list of token ids, got {type(ban).__name__}')
    if not isinstance(bias, dict):
        raise CommuHipError(f'logit bias: "bias" is an object of id: number, got {type(bias).__name__}')
    return ban, bias


def logit_bias_rows(x, n: int):
    """x as float32 [n, VPAD] validated constraint rows: one row ([729] or [768] values) for all n, or n rows."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if not isinstance(x, np.ndarray):
        try:
            x = np.asarray(x, dtype=np.float32)
        except (TypeError, ValueError):
            raise CommuHipError(f"logit bias: one row or {n} rows of numbers expected") from None
    if x.ndim == 1:
        return np.tile(_check_bias_row(x), (n, 1))
    if x.ndim != 2 or x.shape[0] != n:
        raise CommuHipError(f"logit bias: one row or {n} rows expected (one per slot addressed), got shape {x.shape}")
    return np.stack([_check_bias_row(r, f"logit bias, row {i}") for i, r in enumerate(x)])


# ---- the event grammar: a constraint chosen per draw by the slot's own state.  A table is fp32 [8][VPAD]; row c is the
# additive row for a draw whose previous token has class c (midi_inferrer.token_class: OTHER, BAR, PITCH, VELOCITY, CHORD,
# DURATION, POSITION), row 7 is zeros: the row of a slot whose grammar is off (commu_sample_args.gram).
N_CLASSES = 7


def event_grammar():
    """The default table, entries 0 or -inf: after OTHER, BAR, CHORD or DURATION a draw is a position, BAR or EOS (a group
    boundary); after a POSITION a velocity; after a VELOCITY a pitch; after a PITCH a duration.  Chord tokens are never
    drawn (the forcing rules place them).  With it every drawn token continues a group the reference's token-to-MIDI
    step keeps (midi_inferrer.parse_events).  Not enforced by the grammar: positions increasing inside a bar and duplicate
    notes (ForcedDecoder.set_note_order does that), and the contents of a prompt."""
    T = TOKEN_OFFSET
    g = np.full((8, VPAD), -np.inf, dtype=np.float32)
    g[7] = 0.0
    g[:7, 0] = 0.0                     # (ids 0 and >= 729 are never drawn: their entries are ignored)
    g[:7, T.VOCAB_SIZE:] = 0.0
    for c in (0, 1, 4, 5):             # OTHER, BAR, CHORD, DURATION: a group boundary
        g[c, T.POSITION:T.BPM] = 0.0
        g[c, T.BAR] = 0.0
        g[c, T.EOS] = 0.0
    g[6, T.NOTE_VELOCITY:T.CHORD_START] = 0.0        # POSITION -> VELOCITY
    g[3, T.PITCH:T.NOTE_VELOCITY] = 0.0              # VELOCITY -> PITCH
    g[2, T.NOTE_DURATION:T.POSITION] = 0.0           # PITCH -> DURATION
    return g


def grammar_table(x):
    """x as a validated grammar table, float32 [8][VPAD] with a zero row 7: [7 or 8] rows of at least 729 entries, finite
    or -inf (a ban).  Raises CommuHipError on another shape, NaN or +inf, and a class row that bans every id in 1 .. 728
    (a draw after such a token could only fail).  Row 7 of an 8-row table is replaced by zeros: it is the `off` row."""
    V = TOKEN_OFFSET.VOCAB_SIZE
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    try:
        a = np.asarray(x, dtype=np.float32)
    except (TypeError, ValueError):
        raise CommuHipError(f"grammar: a table of 7 or 8 rows of at least {V} numbers expected, got "
                            f"{type(x).__name__}") from None
    if a.ndim != 2 or a.shape[0] not in (N_CLASSES, N_CLASSES + 1) or a.shape[1] < V:
        raise CommuHipError(f"grammar: a table of 7 or 8 rows of at least {V} numbers expected, got shape {a.shape}")
    a = a[:N_CLASSES, :V]
    bad = np.isnan(a) | (a == np.inf)
    if bool(bad.any()):
        c, i = (int(v[0]) for v in np.nonzero(bad))
        raise CommuHipError(f"grammar: row {c}, entry {i} is {a[c, i]}; finite values or -inf (a ban) expected")
    for c in range(N_CLASSES):
        if not bool(np.isfinite(a[c, 1:]).any()):
            raise CommuHipError(f"grammar: row {c} bans all of ids 1 .. {V - 1}, nothing could be drawn after a token of "
                                f"class {c}")
    out = np.zeros((N_CLASSES + 1, VPAD), dtype=np.float32)
    out[:N_CLASSES, :V] = a
    return out


def _grammar_request(grammar, B: int):
    """A request's grammar= as (table or None, slots that are on): None / False, True (the default table), a table
    (grammar_table) for every sequence, or one bool per sequence (the default table where True)."""
    if grammar is None or grammar is False:
        return None, []
    if grammar is True:
        return event_grammar(), list(range(B))
    if isinstance(grammar, torch.Tensor):
        grammar = grammar.detach().cpu().numpy()
    if np.ndim(grammar) == 1 and all(isinstance(v, (bool, np.bool_)) for v in grammar):
        if len(grammar) != B:
            raise CommuHipError(f"grammar: one bool per sequence expected ({B}), got {len(grammar)}")
        on = [b for b, v in enumerate(grammar) if v]
        return (event_grammar() if on else None), on
    return grammar_table(grammar), list(range(B))


# ---- the harmony constraint: a third additive term chosen per draw by the chord the slot is in.  A table is fp32
# [111][16]: row t - 195 for the chord tokens 195 .. 303 (rows 0 .. 107 the 12 roots x 9 qualities, row 108 Chord_NN), row 109
# for a slot whose seq holds no chord yet, row 110 zeros: the row of a slot whose switch is off.  Column pc is MIDI pitch class
# pc (C = 0); columns 12 .. 15 are zero padding, so a row is one 64-byte line (commu_sample_args.harm).
HARM_ROWS, HARM_COLS, HARM_NN, HARM_NO_CHORD, HARM_OFF = 111, 16, 108, 109, 110


def harmony_table(outside=-np.inf, extra=()):
    """The default table: in a chord's row its chord tones (meta.chord_pitch_classes) get 0 and every other pitch class
    gets `outside` -- -inf (strict: only chord tones are drawn) or a finite value <= 0 (soft: the others are discouraged).
    extra: intervals in semitones above the root that are allowed as well (e.g. (2, 9) admits the ninth and the sixth).
    Rows 108 (Chord_NN), 109 (no chord yet) and 110 (off) are zeros: no statement."""
    from .midi_generator.meta import chord_pitch_classes, chord_root
    if isinstance(outside, (bool, np.bool_)) or not isinstance(outside, (int, float, np.integer, np.floating)):
        raise CommuHipError(f"harmony: outside is -inf or a finite number <= 0, got {outside!r}")
    outside = float(outside)
    if math.isnan(outside) or outside > 0:
        raise CommuHipError(f"harmony: outside is -inf or a finite number <= 0, got {outside}")
    given = extra
    try:
        given = list(extra)
        extra = [int(i) for i in given]
        if any(isinstance(i, (bool, np.bool_)) or e != i for e, i in zip(extra, given)):
            raise ValueError
    except (TypeError, ValueError):
        raise CommuHipError(f"harmony: extra is a collection of whole semitone intervals, got {given!r}") from None
    t = np.zeros((HARM_ROWS, HARM_COLS), dtype=np.float32)
    for r in range(HARM_NN):
        allowed = set(chord_pitch_classes(195 + r)) | {(chord_root(195 + r) + i) % 12 for i in extra}
        for pc in range(12):
            t[r, pc] = 0.0 if pc in allowed else outside
    return t


def harmony_rows(x):
    """x as a validated harmony table, float32 [111][16]: [110][12] (chord rows 0 .. 108 and the no-chord row 109) or the
    full [111][16], entries finite or -inf (a ban).  Raises CommuHipError on another shape, NaN or +inf, a row 110 or pad
    columns that are not zero, and a row whose 12 entries are all -inf (after a velocity the slot would have nothing to
    draw)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    what = f"a table of {HARM_OFF} rows of 12 numbers or {HARM_ROWS} rows of {HARM_COLS}"
    try:
        a = np.asarray(x, dtype=np.float32)
    except (TypeError, ValueError):
        raise CommuHipError(f"harmony: {what} expected, got {type(x).__name__}") from None
    if a.shape not in ((HARM_OFF, 12), (HARM_ROWS, HARM_COLS)):
        raise CommuHipError(f"harmony: {what} expected, got shape {a.shape}")
    bad = np.isnan(a) | (a == np.inf)
    if bool(bad.any()):
        r, c = (int(v[0]) for v in np.nonzero(bad))
        raise CommuHipError(f"harmony: row {r}, entry {c} is {a[r, c]}; finite values or -inf (a ban) expected")
    if a.shape[0] == HARM_ROWS:
        for c in np.flatnonzero(a[HARM_OFF]):
            raise CommuHipError(f"harmony: row {HARM_OFF} is the row of a slot that is off and holds zeros, entry {int(c)} is "
                                f"{a[HARM_OFF, c]}")
        for r, c in zip(*np.nonzero(a[:, 12:])):
            raise CommuHipError(f"harmony: columns 12 .. 15 are padding and hold zeros, row {int(r)}, entry {int(c) + 12} is "
                                f"{a[r, c + 12]}")
    for r in range(HARM_OFF):
        if bool((a[r, :12] == -np.inf).all()):
            raise CommuHipError(f"harmony: row {r} bans all 12 pitch classes (every entry is -inf), no pitch could be drawn "
                                f"in that chord")
    out = np.zeros((HARM_ROWS, HARM_COLS), dtype=np.float32)
    out[:HARM_OFF, :12] = a[:HARM_OFF, :12]
    return out


def _harmony_request(harmony):
    """A request's harmony= as a table or None: None / False, True (harmony_table(), strict) or a table (harmony_rows)."""
    if harmony is None or harmony is False:
        return None
    if harmony is True:
        return harmony_table()
    return harmony_rows(harmony)


# ---- class-keyed sampling: a (temperature, top_k, top_p) triple per token class instead of one per slot.  On the host a
# table is float64 [8][3] (columns temperature, top_k, top_p) in which NaN means "inherit the slot's base value"; row c is
# the triple of a draw whose PREVIOUS token has class c (the grammar's key, midi_inferrer.token_class), row 7 is never
# selected.  On the device a slot's table is 8 records of 16 bytes {float temperature; int top_k; float top_p; int 0}, the
# inherited entries filled in from the slot's base triple and row 7 holding the base triple (commu_sample_args.cls_ctl).
CLASS_NAMES = ("other", "bar", "pitch", "velocity", "chord", "duration", "position")
# what is drawn next UNDER THE DEFAULT EVENT GRAMMAR (event_grammar) -> the classes of the previous token it follows
DRAWN_AFTER = {"velocity": ("position",), "pitch": ("velocity",), "duration": ("pitch",),
               "boundary": ("other", "bar", "chord", "duration")}
CLASS_CTL_DTYPE = np.dtype([("temperature", np.float32), ("top_k", np.int32), ("top_p", np.float32), ("reserved", np.int32)])


def _class_entry(entry, what):
    """One entry of class_sampling() as a row (temperature, top_k, top_p), NaN where the entry does not say."""
    V = TOKEN_OFFSET.VOCAB_SIZE
    if not isinstance(entry, dict):
        raise CommuHipError(f"class_sampling: {what}: a dict with any of temperature, top_k, top_p expected, got {entry!r}")
    row = np.full(3, np.nan)
    for key, v in entry.items():
        if key not in ("temperature", "top_k", "top_p"):
            raise CommuHipError(f"class_sampling: {what}: unknown control {key!r} (temperature, top_k, top_p)")
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise CommuHipError(f"class_sampling: {what}: {key} is a number, got {v!r}")
        v = float(v)
        if key == "temperature" and not (np.isfinite(v) and v >= 0):
            raise CommuHipError(f"class_sampling: {what}: temperature: a finite value >= 0 expected (0 = greedy), got {v}")
        if key == "top_k" and not (np.isfinite(v) and v == np.floor(v) and 1 <= v < V):
            raise CommuHipError(f"class_sampling: {what}: top_k: an integer in [1, {V}) expected, got {v}")
        if key == "top_p" and not (0 < v <= 1):
            raise CommuHipError(f"class_sampling: {what}: top_p: a value in (0, 1] expected (1 = off), got {v}")
        row[("temperature", "top_k", "top_p").index(key)] = v
    return row


def class_sampling(drawn=None, after=None):
    """A class-control table, float64 [8][3] with NaN for "inherit the slot's base value" (ForcedDecoder.set_class_sampling,
    generate(class_sampling=)).  after: {class name: {temperature / top_k / top_p: value}} keyed by the class of the
    PREVIOUS token (CLASS_NAMES) -- what the kernel keys on.  drawn: the same keyed by what is drawn next under the default
    event grammar (DRAWN_AFTER): velocity (after a position), pitch (after a velocity), duration (after a pitch), boundary
    (after other, bar, chord, duration: a position, a bar or EOS).  Without the grammar the `drawn` names only say which
    previous classes are meant.  Raises CommuHipError on an unknown name, a class named through both routes, and values
    outside temperature >= 0, top_k in [1, 729), top_p in (0, 1]."""
    table = np.full((N_CLASSES + 1, 3), np.nan)
    named = {}
    for route, entries, names in (("after", after, CLASS_NAMES), ("drawn", drawn, tuple(DRAWN_AFTER))):
        if entries is None:
            continue
        if not isinstance(entries, dict):
            raise CommuHipError(f"class_sampling: {route}: a dict keyed by {', '.join(names)} expected, got {entries!r}")
        for name, entry in entries.items():
            if name not in names:
                raise CommuHipError(f"class_sampling: {route}: unknown name {name!r} (one of {', '.join(names)})")
            row = _class_entry(entry, f"{route} {name!r}")
            for cname in ((name,) if route == "after" else DRAWN_AFTER[name]):
                c = CLASS_NAMES.index(cname)
                if c in named:
                    raise CommuHipError(f"class_sampling: class {c} ({cname}) is named twice: through {named[c]} and through "
                                        f"{route} {name!r}")
                named[c] = f"{route} {name!r}"
                table[c] = row
    return table


def class_sampling_table(x):
    """x as a validated class-control table float64 [8][3] (class_sampling() builds one): 7 or 8 rows of (temperature,
    top_k, top_p), NaN: inherit.  Row 7 is never selected and comes back as NaN."""
    V = TOKEN_OFFSET.VOCAB_SIZE
    try:
        a = np.array(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise CommuHipError(f"class_sampling: a table of 7 or 8 rows of (temperature, top_k, top_p) expected, got "
                            f"{type(x).__name__}") from None
    if a.ndim != 2 or a.shape[0] not in (N_CLASSES, N_CLASSES + 1) or a.shape[1] != 3:
        raise CommuHipError(f"class_sampling: a table of 7 or 8 rows of (temperature, top_k, top_p) expected, got shape "
                            f"{a.shape}")
    out = np.full((N_CLASSES + 1, 3), np.nan)
    out[:N_CLASSES] = a[:N_CLASSES]
    t, k, p = out[:N_CLASSES].T
    for c in range(N_CLASSES):
        if not np.isnan(t[c]) and not (np.isfinite(t[c]) and t[c] >= 0):
            raise CommuHipError(f"class_sampling: row {c}: temperature: a finite value >= 0 expected, got {t[c]}")
        if not np.isnan(k[c]) and not (np.isfinite(k[c]) and k[c] == np.floor(k[c]) and 1 <= k[c] < V):
            raise CommuHipError(f"class_sampling: row {c}: top_k: an integer in [1, {V}) expected, got {k[c]}")
        if not np.isnan(p[c]) and not (0 < p[c] <= 1):
            raise CommuHipError(f"class_sampling: row {c}: top_p: a value in (0, 1] expected, got {p[c]}")
    return out


def class_ctl_records(tables, sampling):
    """The device records of n slots: tables float64 [n][8][3] (NaN: inherit), sampling the slots' base triples as
    sampling_rows returns them ([n] each).  Returns CLASS_CTL_DTYPE [n][8]: entry (c, i) is the table's where it is not NaN
    and the slot's base value elsewhere; row 7 is the base triple; reserved 0."""
    tables = np.asarray(tables, dtype=np.float64)
    n = tables.shape[0]
    base = np.stack([np.asarray(s, dtype=np.float64) for s in sampling], axis=1)          # [n][3]
    full = np.where(np.isnan(tables), base[:, None, :], tables)
    full[:, N_CLASSES] = base
    rec = np.zeros((n, N_CLASSES + 1), dtype=CLASS_CTL_DTYPE)
    rec["temperature"], rec["top_k"], rec["top_p"] = full[..., 0], full[..., 1], full[..., 2]
    return rec


def read_class_sampling(doc):
    """The CLI's --class_sampling document as (table, uses_drawn_names): {"pitch": {...}, "duration": {...}, ...} names
    what is DRAWN (DRAWN_AFTER; meaningful under the default grammar only), {"after": {"velocity": {...}, ...}} the class of
    the previous token; both may stand in one document."""
    if not isinstance(doc, dict):
        raise CommuHipError(f"class_sampling: a JSON object expected, got {type(doc).__name__}")
    after = doc.get("after")
    drawn = {k: v for k, v in doc.items() if k != "after"}
    return class_sampling(drawn=drawn or None, after=after), bool(drawn)


def _class_request(cs):
    """A request's class_sampling= as a table or None: None / False, a table (class_sampling_table) or a dict
    {"drawn": {...}, "after": {...}} (the arguments of class_sampling())."""
    if cs is None or cs is False:
        return None
    if isinstance(cs, dict):
        extra = set(cs) - {"drawn", "after"}
        if extra:
            raise CommuHipError(f"class_sampling: a dict with the keys drawn / after expected, got {sorted(extra)!r}")
        return class_sampling(drawn=cs.get("drawn"), after=cs.get("after"))
    return class_sampling_table(cs)


def _words_per_slot(name: str, word, x, B: int):
    """What the word normalisers share: x as the int32 words of B slots -- one value for all of them or one per slot, each
    through word(value, where), the rule's own check."""
    B = int(B)
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if x is None or np.ndim(x) == 0:
        if isinstance(x, np.ndarray):
            x = x.item()
        return np.full(B, word(x, ""), dtype=np.int32)
    x = list(x)
    if len(x) != B:
        raise CommuHipError(f"{name}: {B} values expected (one per sequence), got {len(x)}")
    if any(np.ndim(v) != 0 for v in x):
        raise CommuHipError(f"{name}: one value per sequence expected, got shape {np.shape(x)}")
    return np.array([word(v.item() if isinstance(v, np.generic) and not isinstance(v, np.bool_) else v, f"[{b}]")
                     for b, v in enumerate(x)], dtype=np.int32)


# ---- note order: one int32 control word per slot (commu_sample_args.order_ctl).  A slot that is on cannot draw a position
# token before the position it is at, a pitch its current position already holds, or -- with a cap n -- the position itself
# once it holds n notes.  The state is read off the slot's seq when the sampling stage runs; nothing else is kept.
NOTE_ORDER_OFF = -1
NOTE_ORDER_MAX = 128          # (a position cannot hold more notes than there are pitches)


def note_order_ctl(x, B: int):
    """A request's note_order= as the int32 control words of B slots: None / False (off, -1), True (on, 0), an integer
    n in 1 .. 128 (on, at most n notes per position; 0 and -1 as the words themselves), or one such value per slot.
    Pure host code; raises CommuHipError on anything else, with the numbers."""
    def word(v, where):
        if v is None or v is False or (isinstance(v, np.bool_) and not v):
            return NOTE_ORDER_OFF
        if v is True or isinstance(v, np.bool_):
            return 0
        ok = isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v) and v == np.floor(v) \
            and -1 <= v <= NOTE_ORDER_MAX
        if not ok:
            raise CommuHipError(f"note_order{where}: None / False (off), True (on) or an integer in [1, {NOTE_ORDER_MAX}] "
                                f"(notes per position; -1 = off, 0 = no cap) expected, got {v!r}")
        return int(v)
    return _words_per_slot("note_order", word, x, B)


# ---- voice cap: one int32 control word per slot (commu_sample_args.voice_ctl).  A slot that is on cannot draw a position at
# which N notes it already holds still sound, nor -- with the re-strike switch -- a pitch that still sounds at the onset it
# is at.  Like the note order it is read off the slot's seq when the sampling stage runs; it relies on the note order (the
# onsets never go back), which set_voices switches on.
VOICES_OFF = -1
VOICES_MAX = 128              # (no more notes can sound than there are pitches)
VOICES_RESTRIKE = 256         # the word's re-strike bit


def voices_word(max_voices: int = 0, no_restrike: bool = False) -> int:
    """The control word N + 256 r of a cap (0: none) and the re-strike ban; voices_ctl validates it."""
    return int(max_voices) + (VOICES_RESTRIKE if no_restrike else 0)


def voices_ctl(x, B: int):
    """A request's voices= as the int32 control words of B slots: None / False (off, -1) or an integer word N + 256 r with N
    in 0 .. 128 (at most N notes sound at once; 0: no cap) and r in {0, 1} (1: a sounding pitch is not struck again) --
    voices_word(N, r) -- or one such value per slot.  Pure host code; raises CommuHipError on anything else, with the
    numbers."""
    def word(v, where):
        if v is None or v is False or (isinstance(v, np.bool_) and not v):
            return VOICES_OFF
        ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) \
            and np.isfinite(v) and v == np.floor(v) and (v == VOICES_OFF or (0 <= v < 2 * VOICES_RESTRIKE and
                                                                            (int(v) & 255) <= VOICES_MAX))
        if not ok:
            raise CommuHipError(f"voices{where}: None / False (off) or an integer word N + {VOICES_RESTRIKE} r with N in "
                                f"[0, {VOICES_MAX}] (notes sounding at once; 0 = no cap) and r in {{0, 1}} (1 = no "
                                f"re-striking; -1 = off) expected, got {v!r}")
        return int(v)
    return _words_per_slot("voices", word, x, B)


# ---- note density: one int32 control word per slot (commu_sample_args.density_ctl).  A slot that is on cannot draw Bar or
# EOS while the bar it is writing holds fewer than `lo` notes (unless no position is left to draw), nor a position once the
# bar holds `hi`.  Like the voice cap it is read off the slot's seq when the sampling stage runs, on the voice cap's walk:
# set_density switches the voice words (and with them the note order) on.
DENSITY_OFF = -1
DENSITY_MAX = 255             # (each bound has one byte of the word)
DENSITY_HI = 256              # the word is lo + DENSITY_HI * hi


def density_word(min_notes: int = 0, max_notes: int = 0) -> int:
    """The control word lo + 256 hi of a lower and an upper bound on a bar's notes (0: none); density_ctl validates it."""
    return int(min_notes) + DENSITY_HI * int(max_notes)


def density_ctl(x, B: int):
    """A request's density= as the int32 control words of B slots: None / False (off, -1) or an integer word lo + 256 hi
    with lo, hi in 0 .. 255 (a bar the slot DRAWS holds at least lo and at most hi notes; 0: that bound is not set; with
    hi >= 1, hi >= max(lo, 1)) -- density_word(lo, hi) -- or one such value per slot.  Pure host code; raises CommuHipError
    on anything else, with the numbers."""
    def word(v, where):
        if v is None or v is False or (isinstance(v, np.bool_) and not v):
            return DENSITY_OFF
        ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) \
            and np.isfinite(v) and v == np.floor(v) and (v == DENSITY_OFF or 0 <= v < DENSITY_HI * (DENSITY_MAX + 1))
        if ok and v >= 0:
            lo, hi = int(v) & 255, int(v) >> 8
            ok = hi == 0 or hi >= max(lo, 1)
        if not ok:
            raise CommuHipError(f"density{where}: None / False (off) or an integer word lo + {DENSITY_HI} hi with lo, hi in "
                                f"[0, {DENSITY_MAX}] (notes per bar at least / at most; 0 = that bound is not set; hi >= lo "
                                f"where both are set; -1 = off) expected, got {v!r}")
        return int(v)
    return _words_per_slot("density", word, x, B)


# ---- melodic interval: one int32 control word per slot (commu_sample_args.interval_ctl).  A slot that is on cannot draw a
# pitch more than `up` semitones above or `down` below the pitch of its last note, nor (u) that pitch itself.  Like the
# density it is read off the slot's seq when the sampling stage runs, on the voice cap's walk -- but it implies none of the
# other words: set_interval allocates them all off and leaves them as the slot has them.
INTERVAL_OFF = -1
INTERVAL_MAX = 127            # (a leap inside the 128-pitch range)
INTERVAL_DOWN = 256           # the word is up + INTERVAL_DOWN * down + INTERVAL_UNISON * u
INTERVAL_UNISON = 65536


def interval_word(up: int = 0, down: int = 0, no_repeat: bool = False) -> int:
    """The control word up + 256 down + 65536 u of a cap on the leap upwards and downwards (semitones; 0: none) and the
    ban on repeating the pitch; interval_ctl validates it."""
    return int(up) + INTERVAL_DOWN * int(down) + (INTERVAL_UNISON if no_repeat else 0)


def interval_ctl(x, B: int):
    """A request's interval= as the int32 control words of B slots: None / False (off, -1) or an integer word
    up + 256 down + 65536 u with up, down in 0 .. 127 (the pitch a slot DRAWS lies at most up semitones above and down below
    the pitch of its last note; 0: that bound is not set) and u in {0, 1} (1: it is not that pitch) -- interval_word(up,
    down, no_repeat) -- or one such value per slot.  Pure host code; raises CommuHipError on anything else, with the
    numbers."""
    def word(v, where):
        if v is None or v is False or (isinstance(v, np.bool_) and not v):
            return INTERVAL_OFF
        ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) \
            and np.isfinite(v) and v == np.floor(v) and (v == INTERVAL_OFF or 0 <= v < 2 * INTERVAL_UNISON)
        if ok and v >= 0:
            up, down = int(v) & 255, (int(v) >> 8) & 255
            ok = up <= INTERVAL_MAX and down <= INTERVAL_MAX
        if not ok:
            raise CommuHipError(f"interval{where}: None / False (off) or an integer word up + {INTERVAL_DOWN} down + "
                                f"{INTERVAL_UNISON} u with up, down in [0, {INTERVAL_MAX}] (semitones above / below the last "
                                f"note; 0 = that bound is not set), u in [0, 1] (1 = no repeated pitch) and no higher bit "
                                f"(-1 = off) expected, got {v!r}")
        return int(v)
    return _words_per_slot("interval", word, x, B)


# ---- onset templates: one int32 control word per slot (commu_sample_args.onset_ctl) and one device table of 128-bit rows
# (onset_table).  A slot that is on can DRAW a position only where the row of the bar being written has a bit: the row is
# base + (i mod R) for bar index i = max(seq.count(BAR) - 1, 0), the bars of a prompt included.  The kernel takes the count
# from the forcing record.  Like the interval it implies none of the other words.
ONSETS_OFF = -1
ONSET_GRID = 128              # grid steps of a bar: position id 432 + g
ONSET_ROWS_MAX = 4096         # rows of the device table; the word is base + ONSET_ROWS_MAX * R
ONSET_CYCLE_MAX = 64          # bars of one template
ONSET_POS0, ONSET_BAR = 432, 2


def onset_word(base: int, cycle: int) -> int:
    """The control word base + 4096 R of a template of R rows that starts at table row base."""
    return int(base) + ONSET_ROWS_MAX * int(cycle)


def onset_rows(x) -> np.ndarray:
    """A template as uint32 [R][4], one 128-bit row per bar of its cycle (bit g % 32 of word g // 32: grid step g may hold an
    onset).  x: a list of bars, each a list of positions 0 .. 127 (an empty bar rests); {"grid": n} with n a power of two
    from 1 to 128 -- one bar, the positions that are multiples of 128 / n; {"bars": [...]} -- the list form; or a uint32 array
    [R][4] that is one already.  1 <= R <= 64.  Pure host code; raises CommuHipError on anything else, with the value."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint32:
        if x.ndim != 2 or x.shape[1] != 4 or not 1 <= x.shape[0] <= ONSET_CYCLE_MAX:
            raise CommuHipError(f"onsets: a uint32 template is [1 .. {ONSET_CYCLE_MAX}][4], got shape {x.shape}")
        return np.ascontiguousarray(x)
    if isinstance(x, dict):
        if set(x) == {"grid"}:
            n = x["grid"]
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= ONSET_GRID or n & (n - 1):
                raise CommuHipError(f'onsets: {{"grid": n}} takes a power of two from 1 to {ONSET_GRID}, got {n!r}')
            x = [list(range(0, ONSET_GRID, ONSET_GRID // int(n)))]
        elif set(x) == {"bars"}:
            x = x["bars"]
        else:
            raise CommuHipError(f'onsets: {{"grid": n}} or {{"bars": [...]}} expected, got the keys {sorted(map(str, x))}')
    if not isinstance(x, (list, tuple)) or not all(isinstance(b, (list, tuple)) for b in x):
        raise CommuHipError(f"onsets: a list of bars, each a list of positions 0 .. {ONSET_GRID - 1}, expected, got {x!r}")
    if not 1 <= len(x) <= ONSET_CYCLE_MAX:
        raise CommuHipError(f"onsets: a template holds 1 .. {ONSET_CYCLE_MAX} bars, got {len(x)}")
    out = np.zeros((len(x), 4), dtype=np.uint32)
    for i, bar in enumerate(x):
        for g in bar:
            if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer)) or not 0 <= g < ONSET_GRID:
                raise CommuHipError(f"onsets: bar {i}: positions are integers 0 .. {ONSET_GRID - 1}, got {g!r}")
            out[i, int(g) // 32] |= np.uint32(1 << (int(g) % 32))
    return out


def _is_note_at(seq, i) -> bool:
    """seq[i : i + 4] is a Position, Velocity, Pitch, Duration group (voices_contract's NOTE)."""
    return i + 3 < len(seq) and 432 <= seq[i] <= 559 and 131 <= seq[i + 1] <= 194 and 3 <= seq[i + 2] <= 130 \
        and 304 <= seq[i + 3] <= 431


def onsets_of(seq, start: int = 0, invert: bool = False) -> List[List[int]]:
    """The onsets of a token sequence, bar by bar in the rule's bar index: element i lists the positions 0 .. 127 at which a
    complete Position, Velocity, Pitch, Duration group of bar i starts, for the groups at index >= start (the stretch before
    the first Bar belongs to bar 0, as the rule counts it).  invert: the positions of each bar that hold NO onset.  What it
    returns is a template in onset_rows' list form: a request given it follows the track (or, inverted, leaves it room).
    A sequence longer than 64 bars gives more bars than a template takes; cut it."""
    seq = [int(t) for t in seq]
    bars: List[set] = [set()]
    nb = 0
    for i, t in enumerate(seq):
        if t == ONSET_BAR:
            nb += 1
            if nb >= 2:
                bars.append(set())
        elif i >= int(start) and _is_note_at(seq, i):
            bars[max(nb - 1, 0)].add(t - ONSET_POS0)
    if invert:
        return [sorted(set(range(ONSET_GRID)) - b) for b in bars]
    return [sorted(b) for b in bars]


def _onsets_per_slot(x, B: int):
    """A request's onsets= as B entries, each None (off) or a uint32 [R][4] template: None / False (all off), one template in
    any form onset_rows takes (all slots), or a list of B entries each None / False or a template.  A list whose elements
    are lists of integers is ONE template (its bars)."""
    B = int(B)
    if x is None or x is False:
        return [None] * B
    if isinstance(x, (list, tuple)) and len(x) and not all(
            isinstance(b, (list, tuple)) and all(isinstance(g, (int, np.integer)) for g in b) for b in x):
        if len(x) != B:
            raise CommuHipError(f"onsets: {B} entries expected (one per sequence), got {len(x)}")
        return [None if (v is None or v is False) else onset_rows(v) for v in x]
    t = onset_rows(x)
    return [t] * B


def _templates_per_slot(name: str, template, x, B: int):
    """What the guide's, the articulation's and the form's normalisers share: None / False (all off), one value in any form
    `template` takes (all slots), or a list of B entries each None / False or such a value."""
    B = int(B)
    if x is None or x is False:
        return [None] * B
    if isinstance(x, list):
        if len(x) != B:
            raise CommuHipError(f"{name}: {B} entries expected (one per sequence), got {len(x)}")
        return [None if (v is None or v is False) else template(v) for v in x]
    return [template(x)] * B


# ---- guide track: one int32 control word per slot (commu_sample_args.guide_ctl) and one device table of 128-bit rows
# (guide_table).  A template has R bars of C = 128 >> s cells; a bar is a block of 1 + C rows: the LIVE ROW (a mask over
# positions, the onset table's format) and C CELL ROWS (masks over pitches: bit k is pitch id 3 + k, MIDI pitch k).  A slot
# that is on DRAWS a pitch only where the cell row of the position its bar is at has a bit, and a position only where the
# live row has one.  The block of the open bar is base + (i mod R) (1 + C), i as for the onsets.  It implies none of the
# other words.
GUIDE_OFF = -1
GUIDE_ROWS_MAX = 65536         # rows of the device table (1 MB); the word is base + 65536 R + 2^23 s
GUIDE_CYCLE_MAX = 64           # bars of one template
GUIDE_KEYS_RAW = {"cells", "bars", "pitch_range"}
GUIDE_KEYS_DERIVED = {"from_tokens", "cells", "avoid_intervals", "no_unison", "below", "above", "pitch_range"}


def guide_word(base: int, bars: int, cells: int) -> int:
    """The control word base + 65536 R + 2^23 s of a template of R bars of `cells` = 128 >> s cells at table row base."""
    return int(base) + 65536 * int(bars) + (1 << 23) * _guide_shift(cells)


def _guide_shift(cells) -> int:
    if isinstance(cells, bool) or not isinstance(cells, (int, np.integer)) or not 1 <= cells <= ONSET_GRID or cells & (cells - 1):
        raise CommuHipError(f"guide: cells is a power of two from 1 to {ONSET_GRID}, got {cells!r}")
    return 7 - (int(cells).bit_length() - 1)


def _guide_range(pitch_range):
    if pitch_range is None:
        return 0, 127
    try:
        lo, hi = pitch_range
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (lo, hi)) and 0 <= lo <= hi <= 127
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise CommuHipError(f"guide: pitch_range is a pair of MIDI pitches 0 <= lo <= hi <= 127, got {pitch_range!r}")
    return int(lo), int(hi)


def sounding_of(seq, start: int = 0):
    """The notes of a token sequence on the absolute grid, with its bars counted as the rule counts them: a list
    (bars, notes), bars the number of bars (the stretch before the first Bar is bar 0) and notes a list of (first step,
    one past the last step, MIDI pitch) for every complete Position, Velocity, Pitch, Duration group at index >= start:
    first step 128 bar + position, length in steps the duration id - 303."""
    seq = [int(t) for t in seq]
    nb, notes = 0, []
    for i, t in enumerate(seq):
        if t == ONSET_BAR:
            nb += 1
        elif i >= int(start) and _is_note_at(seq, i):
            a = ONSET_GRID * max(nb - 1, 0) + (t - ONSET_POS0)
            notes.append((a, a + seq[i + 3] - 303, seq[i + 2] - 3))
    return max(nb, 1), notes


def _guide_cells_of(doc):
    """The derived form as a list of bars of C cells, each cell a 128-bit Python int over MIDI pitches."""
    extra = sorted(set(doc) - GUIDE_KEYS_DERIVED)
    if extra:
        raise CommuHipError(f"guide: unknown key {extra[0]!r} beside from_tokens (known: {sorted(GUIDE_KEYS_DERIVED)})")
    toks = doc["from_tokens"]
    if not isinstance(toks, (list, tuple, np.ndarray)) or not all(
            isinstance(t, (int, np.integer)) and not isinstance(t, bool) and 0 <= t < 729 for t in toks):
        raise CommuHipError("guide: from_tokens: a list of token ids in [0, 729) expected")
    cells = doc.get("cells", 16)
    s = _guide_shift(cells)
    avoid = doc.get("avoid_intervals", [1, 11])
    if not isinstance(avoid, (list, tuple)) or not all(
            isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 11 for v in avoid):
        raise CommuHipError(f"guide: avoid_intervals: interval classes 0 .. 11 expected, got {avoid!r}")
    uni = doc.get("no_unison", False)
    if not isinstance(uni, (bool, np.bool_)):
        raise CommuHipError(f"guide: no_unison: true or false expected, got {uni!r}")
    if "below" in doc and "above" in doc:
        raise CommuHipError(f"guide: below ({doc['below']!r}) beside above ({doc['above']!r}): one of them expected")
    for k in ("below", "above"):
        if k in doc and (isinstance(doc[k], bool) or not isinstance(doc[k], (int, np.integer)) or not 0 <= doc[k] <= 127):
            raise CommuHipError(f"guide: {k}: a number of semitones 0 .. 127 expected, got {doc[k]!r}")
    nbars, notes = sounding_of(toks)
    if nbars > GUIDE_CYCLE_MAX:
        raise CommuHipError(f"guide: a template holds 1 .. {GUIDE_CYCLE_MAX} bars, the track has {nbars}")
    full = (1 << 128) - 1
    steps = [full] * (nbars * ONSET_GRID)
    sound = [[] for _ in steps]
    for a, e, y in notes:
        for t in range(a, min(e, len(steps))):
            sound[t].append(y)
    memo = {}
    for t, ys in enumerate(sound):
        if not ys:
            continue          # (a silent step allows everything)
        key = tuple(sorted(set(ys)))
        if key not in memo:
            m = 0
            for x in range(128):
                ok = all((x - y) % 12 not in avoid for y in key)
                ok = ok and not (uni and x in key)
                ok = ok and not ("below" in doc and x > key[0] - int(doc["below"]))
                ok = ok and not ("above" in doc and x < key[-1] + int(doc["above"]))
                m |= int(ok) << x
            memo[key] = m
        steps[t] = memo[key]
    per = 1 << s
    out = []
    for b in range(nbars):
        bar = []
        for c in range(int(cells)):
            m = full
            for t in range(b * ONSET_GRID + c * per, b * ONSET_GRID + (c + 1) * per):
                m &= steps[t]
            bar.append(m)
        out.append(bar)
    return out, s


def _guide_cells_raw(doc):
    extra = sorted(set(doc) - GUIDE_KEYS_RAW)
    if extra:
        raise CommuHipError(f"guide: unknown key {extra[0]!r} (known: {sorted(GUIDE_KEYS_RAW)}, or the from_tokens form)")
    if "cells" not in doc or "bars" not in doc:
        raise CommuHipError(f'guide: {{"cells": C, "bars": [...]}} or {{"from_tokens": [...], ...}} expected, got the keys '
                            f'{sorted(map(str, doc))}')
    cells = doc["cells"]
    s = _guide_shift(cells)
    bars = doc["bars"]
    if not isinstance(bars, (list, tuple)) or not 1 <= len(bars) <= GUIDE_CYCLE_MAX:
        raise CommuHipError(f"guide: a template holds 1 .. {GUIDE_CYCLE_MAX} bars, got "
                            f"{len(bars) if isinstance(bars, (list, tuple)) else bars!r}")
    full = (1 << 128) - 1
    out = []
    for i, bar in enumerate(bars):
        if not isinstance(bar, (list, tuple)) or len(bar) != cells:
            raise CommuHipError(f"guide: bar {i}: {cells} cells expected, got "
                                f"{len(bar) if isinstance(bar, (list, tuple)) else bar!r}")
        row = []
        for c, cell in enumerate(bar):
            if cell is None:
                row.append(full)
                continue
            if not isinstance(cell, (list, tuple)) or not all(
                    isinstance(x, (int, np.integer)) and not isinstance(x, bool) and 0 <= x <= 127 for x in cell):
                raise CommuHipError(f"guide: bar {i}, cell {c}: null or a list of MIDI pitches 0 .. 127 expected, got {cell!r}")
            m = 0
            for x in cell:
                m |= 1 << int(x)
            row.append(m)
        out.append(row)
    return out, s


def _guide_words4(m: int) -> List[int]:
    return [(m >> (32 * k)) & 0xFFFFFFFF for k in range(4)]


def guide_template(x, pitch_range=None):
    """A guide as (rows, cells): rows uint32 [R (1 + C)][4], per bar the live row and the C cell rows (guide_rows), and C.
    x: the raw form {"cells": C, "bars": [[null | [MIDI pitches], .. C entries], ..]} (null: every pitch); the derived form
    {"from_tokens": [ids], "cells": C = 16, "avoid_intervals": [1, 11], "no_unison": false, "below": m | "above": m}; either
    may carry "pitch_range": [lo, hi], used where the argument is None; or a pair (uint32 [R (1 + C)][4], C) that is one
    already.  Pure host code; raises CommuHipError on anything else, with the value."""
    if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], np.ndarray) and x[0].dtype == np.uint32:
        rows, cells = x
        per = 1 + (ONSET_GRID >> _guide_shift(cells))
        if rows.ndim != 2 or rows.shape[1] != 4 or rows.shape[0] % per or not 1 <= rows.shape[0] // per <= GUIDE_CYCLE_MAX:
            raise CommuHipError(f"guide: a uint32 template of {cells} cells is [R * {per}][4] with R in 1 .. "
                                f"{GUIDE_CYCLE_MAX}, got shape {rows.shape}")
        return np.ascontiguousarray(rows), int(cells)
    if not isinstance(x, dict):
        raise CommuHipError(f'guide: {{"cells": C, "bars": [...]}} or {{"from_tokens": [...], ...}} expected, got {x!r}')
    if pitch_range is None:
        pitch_range = x.get("pitch_range")
    lo, hi = _guide_range(pitch_range)
    bars, s = _guide_cells_of(x) if "from_tokens" in x else _guide_cells_raw(x)
    cells = ONSET_GRID >> s
    inside = ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)
    out = np.zeros((len(bars) * (1 + cells), 4), dtype=np.uint32)
    for b, bar in enumerate(bars):
        live = 0
        for c, m in enumerate(bar):
            out[b * (1 + cells) + 1 + c] = _guide_words4(m)
            if m & inside:          # (the live bits of the cell's steps: the cell leaves a pitch of the range)
                live |= ((1 << (1 << s)) - 1) << (c << s)
        out[b * (1 + cells)] = _guide_words4(live)
    return out, cells


def guide_rows(x, pitch_range=None) -> np.ndarray:
    """A guide's table rows, uint32 [R (1 + C)][4]: per bar one LIVE ROW (bit g % 32 of word g // 32: a note may start at
    step g -- set iff the step's cell, intersected with pitch_range = (lo, hi) MIDI when given, leaves a pitch) and C CELL
    ROWS (bit k % 32 of word k // 32: MIDI pitch k, token id 3 + k, may be drawn).  x as for guide_template.  In the derived
    form the notes of the finished track are its Position, Velocity, Pitch, Duration groups, a note's length in steps its
    duration id - 303, on the absolute grid 128 bar + position with the bars counted as the rule counts them; at a step
    where pitches Y sound, x is allowed iff (x - y) mod 12 is in avoid_intervals for no y, x is not in Y (no_unison),
    x <= min Y - m (below) and x >= max Y + m (above); a silent step allows everything, a cell is the AND over its steps."""
    return guide_template(x, pitch_range)[0]


def _guide_per_slot(x, B: int):
    """A request's guide= as B entries, each None (off) or a template (rows, cells): None / False (all off), one guide in
    any form guide_template takes (all slots), or a list of B entries each None / False or a guide."""
    return _templates_per_slot("guide", guide_template, x, B)


# ---- articulation: one int32 control word per slot (commu_sample_args.art_ctl) and one device table of 128-bit rows
# (art_table).  A row is one bar of a template: word 0 dlo | dhi << 8 (steps, 0: not set), words 1 and 2 the 64-bit mask of
# the velocity bins that may be drawn, word 3 reserved (0).  A slot that is on DRAWS a duration only inside the window of
# its open bar's row -- capped at the bar line (within_bar) and at the first step where the slot's guide bans the pitch just
# drawn (hold_guide) -- and a velocity only where the row has a bit.  The row of the open bar is base + (i mod R), i as for
# the onsets.  It implies none of the other words.
ARTICULATION_OFF = -1
ARTICULATION_ROWS_MAX = 4096   # rows of the device table (64 KB); the word is base + 4096 R + 2^19 w + 2^20 h
ARTICULATION_CYCLE_MAX = 64    # bars of one template
ARTICULATION_KEYS = {"bars", "within_bar", "hold_guide"}
ARTICULATION_BAR_KEYS = {"duration", "velocity"}


def articulation_word(base: int, bars: int, within_bar: bool = False, hold_guide: bool = False) -> int:
    """The control word base + 4096 R + 2^19 w + 2^20 h of a template of R bars at table row base."""
    return int(base) + 4096 * int(bars) + (1 << 19) * int(bool(within_bar)) + (1 << 20) * int(bool(hold_guide))


def _articulation_bar(bar, where: str) -> List[int]:
    """One bar {"duration": [lo, hi], "velocity": [lo, hi]} | None as its four words."""
    if bar is None:
        return [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    if not isinstance(bar, dict):
        raise CommuHipError(f'articulation: {where}null or {{"duration": [lo, hi], "velocity": [lo, hi]}} expected, got {bar!r}')
    extra = sorted(set(bar) - ARTICULATION_BAR_KEYS)
    if extra:
        raise CommuHipError(f"articulation: {where}unknown key {extra[0]!r} (known: {sorted(ARTICULATION_BAR_KEYS)})")
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    dlo = dhi = 0
    if bar.get("duration") is not None:
        d = bar["duration"]
        if not isinstance(d, (list, tuple)) or len(d) != 2 or not all(v is None or (is_int(v) and 1 <= v <= 128) for v in d):
            raise CommuHipError(f"articulation: {where}duration: a pair [lo, hi] of steps 1 .. 128 (either may be null) "
                                f"expected, got {d!r}")
        if d[0] is not None and d[1] is not None and d[0] > d[1]:
            raise CommuHipError(f"articulation: {where}duration: lo <= hi expected, got {list(d)!r}")
        dlo, dhi = int(d[0] or 0), int(d[1] or 0)
    mask = (1 << 64) - 1
    if bar.get("velocity") is not None:
        v = bar["velocity"]
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(is_int(x) and 0 <= x <= 127 for x in v):
            raise CommuHipError(f"articulation: {where}velocity: a pair [lo, hi] of MIDI velocities 0 .. 127 expected, got {v!r}")
        if v[0] > v[1]:
            raise CommuHipError(f"articulation: {where}velocity: lo <= hi expected, got {list(v)!r}")
        # (bins floor(lo / 2) .. ceil(hi / 2), capped at 63: token_constraints(velocity_range=...) maps them the same way)
        b0, b1 = int(v[0]) // 2, min((int(v[1]) + 1) // 2, 63)
        if b0 > b1:
            raise CommuHipError(f"articulation: {where}velocity: the range {list(v)!r} holds no velocity bin")
        mask = ((1 << (b1 + 1)) - 1) & ~((1 << b0) - 1)
    return [dlo | dhi << 8, mask & 0xFFFFFFFF, mask >> 32, 0]


def articulation_template(x):
    """An articulation as (rows, within_bar, hold_guide): rows uint32 [R][4] (articulation_rows) and the two switches.  x: the
    full form {"bars": [{"duration": [lo, hi], "velocity": [lo, hi]} | null, ..], "within_bar": bool, "hold_guide": bool} (at
    most 64 bars, cycled bar by bar; a null bar constrains nothing); the short form, the single bar's keys at top level, e.g.
    {"duration": [2, 16], "hold_guide": true}; or a triple (uint32 [R][4], within_bar, hold_guide) that is one already.
    duration is in steps 1 .. 128, either end may be null; velocity is in MIDI 0 .. 127 and maps to the bins floor(lo / 2) ..
    ceil(hi / 2), capped at 63.  Pure host code; raises CommuHipError on anything else, with the bar index and the value."""
    if isinstance(x, tuple) and len(x) == 3 and isinstance(x[0], np.ndarray) and x[0].dtype == np.uint32:
        rows, w, h = x
        if rows.ndim != 2 or rows.shape[1] != 4 or not 1 <= rows.shape[0] <= ARTICULATION_CYCLE_MAX:
            raise CommuHipError(f"articulation: a uint32 template is [R][4] with R in 1 .. {ARTICULATION_CYCLE_MAX}, got "
                                f"shape {rows.shape}")
        if ((rows[:, 1] | rows[:, 2]) == 0).any():
            raise CommuHipError(f"articulation: bar {int(np.argmax((rows[:, 1] | rows[:, 2]) == 0))}: an empty velocity mask")
        return np.ascontiguousarray(rows), bool(w), bool(h)
    if not isinstance(x, dict):
        raise CommuHipError(f'articulation: {{"bars": [...], "within_bar": bool, "hold_guide": bool}} or {{"duration": '
                            f'[lo, hi], "velocity": [lo, hi], ...}} expected, got {x!r}')
    if "bars" in x:
        extra = sorted(set(x) - ARTICULATION_KEYS)
        if extra:
            raise CommuHipError(f"articulation: unknown key {extra[0]!r} beside bars (known: {sorted(ARTICULATION_KEYS)})")
        bars = x["bars"]
        if not isinstance(bars, (list, tuple)) or not 1 <= len(bars) <= ARTICULATION_CYCLE_MAX:
            raise CommuHipError(f"articulation: a template holds 1 .. {ARTICULATION_CYCLE_MAX} bars, got "
                                f"{len(bars) if isinstance(bars, (list, tuple)) else bars!r}")
        words = [_articulation_bar(b, f"bar {i}: ") for i, b in enumerate(bars)]
    else:
        extra = sorted(set(x) - ARTICULATION_BAR_KEYS - {"within_bar", "hold_guide"})
        if extra:
            raise CommuHipError(f"articulation: unknown key {extra[0]!r} (known: "
                                f"{sorted(ARTICULATION_BAR_KEYS | ARTICULATION_KEYS)})")
        words = [_articulation_bar({k: x[k] for k in ARTICULATION_BAR_KEYS if k in x}, "")]
    for k in ("within_bar", "hold_guide"):
        if not isinstance(x.get(k, False), (bool, np.bool_)):
            raise CommuHipError(f"articulation: {k}: true or false expected, got {x[k]!r}")
    return np.array(words, dtype=np.uint32), bool(x.get("within_bar", False)), bool(x.get("hold_guide", False))


def articulation_rows(x) -> np.ndarray:
    """An articulation's table rows, uint32 [R][4]: per bar word 0 = dlo | dhi << 8 (steps; 0: not set), words 1 and 2 the
    64-bit mask of the velocity bins that may be drawn (bit k % 32 of word 1 + k // 32: id 131 + k, MIDI velocity 2 k),
    word 3 = 0.  x as for articulation_template."""
    return articulation_template(x)[0]


def _articulation_needs_guide(arts, guides):
    """hold_guide reads the sequence's own guide: refused where a sequence asks for it and has none."""
    for i, (a, g) in enumerate(zip(arts, guides)):
        if a is not None and a[2] and g is None:
            raise CommuHipError("articulation: hold_guide without a guide" +
                                (f" (sequence {i})" if len(arts) > 1 else "") + ": it reads the sequence's own guide track")


def _articulation_per_slot(x, B: int):
    """A request's articulation= as B entries, each None (off) or a template (rows, within_bar, hold_guide): None / False
    (all off), one articulation in any form articulation_template takes (all slots), or a list of B entries each None /
    False or an articulation."""
    return _templates_per_slot("articulation", articulation_template, x, B)


# ---- form templates: one int32 control word per slot (commu_decode_loop_args.form_ctl) and one device table of 128-bit rows
# (form_table).  Row base + i is bar i of the form: free, or a REPLAY of an earlier bar of the slot's own sequence.  The rule
# lives in the forcing stage (csrc/decode_loop.h: Form): inside a replay bar the tokens of the source bar's note groups are
# handed to the book-keeping as if drawn.  A form is not cycled: bars past its end are free.
FORM_OFF = -1
FORM_ROWS_MAX = 4096           # rows of the device table (64 KB); the word is base + 4096 R
FORM_BARS_MAX = 64             # bars of one form
FORM_TRANSPOSE_MAX = 48
FORM_COPIES = ("all", "rhythm")
FORM_BAR_KEYS = {"of", "copy", "transpose"}
# ---- takes: a bar may also replay a bar of a finished sequence the user already has.  A TAKE ROW has bit 7 of word 0 set,
# word 1 `begin` and word 2 `end`: the source bar is form_src[begin .. end) of the decoder's take buffer.  In a template the
# two are counted from the take's own start; the decoder rebases them to where it placed the take (ForcedDecoder._pack).
FORM_TAKE_BIT = 1 << 7
FORM_SRC_MAX = 1 << 18         # ints of the decoder's take buffer (1 MiB): 64 takes of 4096 tokens
FORM_TAKE_KEYS = {"take", "of", "copy", "transpose"}
FORM_KEEP_KEYS = {"keep", "redo", "repitch"}


class FormTakes(np.ndarray):
    """A form that names takes: its uint32 [R][4] rows (take rows carry begin / end counted from their take's start) with
    .takes, the takes' tokens as int32 arrays, and .take_of, per bar the index of the take its row reads (-1: none)."""
    takes: tuple = ()
    take_of: tuple = ()

    def __array_finalize__(self, obj):
        self.takes = getattr(obj, "takes", ())
        self.take_of = getattr(obj, "take_of", ())


def form_word(base: int, bars: int) -> int:
    """The control word base + 4096 R of a form of R bars that starts at table row base."""
    return int(base) + FORM_ROWS_MAX * int(bars)


def form_row_word(src: int, copy: str = "all", transpose: int = 0) -> int:
    """Word 0 of a replay row: src | copy << 6 | (transpose + 64) << 8 (a free bar's word is 0)."""
    return int(src) | (FORM_COPIES.index(copy) << 6) | ((int(transpose) + 64) << 8)


def form_row_fields(word: int):
    """(src, copy, transpose) of a row's word 0, None for a free bar."""
    word = int(word)
    if (word >> 8) & 127 == 0:
        return None
    return word & 63, FORM_COPIES[(word >> 6) & 1], ((word >> 8) & 127) - 64


def _form_bar(i: int, bar) -> int:
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if bar is None:
        return 0
    if is_int(bar):
        bar = {"of": bar}
    if not isinstance(bar, dict):
        raise CommuHipError(f'form: bar {i}: null, a bar index or {{"of": j, "copy": "all" | "rhythm", "transpose": s}} '
                            f"expected, got {bar!r}")
    extra = sorted(set(map(str, bar)) - FORM_BAR_KEYS)
    if extra:
        raise CommuHipError(f"form: bar {i}: unknown key {extra[0]!r} (known: {sorted(FORM_BAR_KEYS)})")
    if "of" not in bar or not is_int(bar["of"]) or bar["of"] < 0:
        raise CommuHipError(f'form: bar {i}: "of": the index of an earlier bar expected, got {bar.get("of")!r}')
    if bar["of"] >= i:
        raise CommuHipError(f'form: bar {i}: "of": {bar["of"]} is not an earlier bar (a bar replays one below its own index'
                            + ("; bar 0 is always free)" if i == 0 else ")"))
    return form_row_word(bar["of"], *_form_mode(i, bar))


def _form_mode(i: int, bar: dict):
    """("all" | "rhythm", transpose) of a replay bar's document."""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    copy = bar.get("copy", "all")
    if copy not in FORM_COPIES:
        raise CommuHipError(f'form: bar {i}: "copy": "all" or "rhythm" expected, got {copy!r}')
    s = bar.get("transpose", 0)
    if not is_int(s) or not -FORM_TRANSPOSE_MAX <= s <= FORM_TRANSPOSE_MAX:
        raise CommuHipError(f'form: bar {i}: "transpose": semitones in -{FORM_TRANSPOSE_MAX} .. {FORM_TRANSPOSE_MAX} '
                            f"expected, got {s!r}")
    if s != 0 and copy == "rhythm":
        raise CommuHipError(f'form: bar {i}: "transpose": {s} beside "copy": "rhythm" (the pitches of such a bar are drawn)')
    return copy, s


def form_take_bars(tokens) -> List[tuple]:
    """The bars of a take as (begin, end) index pairs: bar j is the stretch behind the take's (j+1)-th Bar token up to its
    next Bar, the last bar up to the list's end.  An EMPTY bar is given as the one-token stretch of its own Bar token (no
    note group lies in it, so its replay is an empty bar; begin == end would be a free row)."""
    at = [i for i, t in enumerate(tokens) if int(t) == ONSET_BAR]
    ends = at[1:] + [len(tokens)]
    return [(a + 1, e) if a + 1 < e else (a, a + 1) for a, e in zip(at, ends)]


def _form_take_tokens(t: int, ids) -> np.ndarray:
    if isinstance(ids, dict) and set(ids) == {"from_tokens"}:
        ids = ids["from_tokens"]
    try:
        arr = np.asarray(ids)
    except ValueError:
        arr = None
    if arr is None or arr.ndim != 1 or arr.size == 0 or arr.dtype.kind not in "iu":
        raise CommuHipError(f"form: take {t}: a list of token ids expected, got {ids!r:.80}")
    if arr.size > FORM_SRC_MAX:
        raise CommuHipError(f"form: take {t}: {arr.size} tokens, the take buffer holds {FORM_SRC_MAX}")
    bad = np.flatnonzero((arr < 0) | (arr >= TOKEN_OFFSET.VOCAB_SIZE))
    if bad.size:
        raise CommuHipError(f"form: take {t}: token {int(arr[bad[0]])} at index {int(bad[0])} is outside "
                            f"[0, {TOKEN_OFFSET.VOCAB_SIZE})")
    if not (arr == ONSET_BAR).any():
        raise CommuHipError(f"form: take {t}: no Bar token: a take without a bar line has no bar to replay")
    return np.ascontiguousarray(arr, dtype=np.int32)


def _form_with_takes(x) -> "FormTakes":
    """The {"takes": ..., "bars": ...} document as a FormTakes."""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    takes, bars = x["takes"], x["bars"]
    if isinstance(takes, dict) or (isinstance(takes, (list, tuple, np.ndarray)) and len(takes) and is_int(takes[0])):
        takes = [takes]                                        # (one take, given bare)
    if not isinstance(takes, (list, tuple)) or not takes or not isinstance(bars, (list, tuple)):
        raise CommuHipError('form: {"takes": [[ids], ...] | {"from_tokens": [ids]}, "bars": [...]} expected, got '
                            f"{x!r:.120}")
    takes = [_form_take_tokens(t, ids) for t, ids in enumerate(takes)]
    if not 1 <= len(bars) <= FORM_BARS_MAX:
        raise CommuHipError(f"form: a form holds 1 .. {FORM_BARS_MAX} bars, got {len(bars)}" +
                            (f" (bar {FORM_BARS_MAX} is one too many)" if bars else ""))
    spans = [form_take_bars(tk) for tk in takes]
    out = np.zeros((len(bars), 4), dtype=np.uint32)
    take_of = [-1] * len(bars)
    for i, bar in enumerate(bars):
        if not isinstance(bar, dict) or "take" not in bar:
            out[i, 0] = _form_bar(i, bar)
            continue
        extra = sorted(set(map(str, bar)) - FORM_TAKE_KEYS)
        if extra:
            raise CommuHipError(f"form: bar {i}: unknown key {extra[0]!r} (known: {sorted(FORM_TAKE_KEYS)})")
        t = bar["take"]
        if t is None and len(takes) == 1:
            t = 0
        if not is_int(t) or not 0 <= t < len(takes):
            raise CommuHipError(f'form: bar {i}: "take": {t!r} is not one of the {len(takes)} takes')
        j = bar.get("of")
        if not is_int(j) or not 0 <= j < len(spans[t]):
            raise CommuHipError(f'form: bar {i}: "of": {j!r} is not a bar of take {t} (it has {len(spans[t])})')
        if j >= FORM_BARS_MAX:
            raise CommuHipError(f'form: bar {i}: "of": {j}: a row names one of a take\'s first {FORM_BARS_MAX} bars')
        out[i] = (form_row_word(j, *_form_mode(i, bar)) | FORM_TAKE_BIT, spans[t][j][0], spans[t][j][1], 0)
        take_of[i] = int(t)
    res = out.view(FormTakes)
    res.takes, res.take_of = tuple(takes), tuple(take_of)
    return res


def _form_keep(x) -> dict:
    """The short form {"keep": take, "redo": [bars], "repitch": [bars]} written out in full."""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    take = _form_take_tokens(0, x["keep"])
    n = len(form_take_bars(take))
    lists = {}
    for k in ("redo", "repitch"):
        v = x.get(k, [])
        if not isinstance(v, (list, tuple)) or not all(is_int(b) for b in v):
            raise CommuHipError(f'form: "{k}": a list of bar indices expected, got {v!r}')
        for b in v:
            if not 0 <= b < n:
                raise CommuHipError(f'form: bar {b}: "{k}" names a bar the take does not have (it has {n})')
        lists[k] = set(int(b) for b in v)
    both = sorted(lists["redo"] & lists["repitch"])
    if both:
        raise CommuHipError(f'form: bar {both[0]}: listed in "redo" and in "repitch"')
    bars = [None if i in lists["redo"] else
            {"take": 0, "of": i, "copy": "rhythm"} if i in lists["repitch"] else {"take": 0, "of": i}
            for i in range(min(n, FORM_BARS_MAX))]
    return {"takes": [take], "bars": bars}


def form_document(template) -> dict:
    """A form as a document form_template reads, in the full form: {"bars": [...]} and, where it names takes, "takes"."""
    rows = form_template(template)
    take_of = getattr(rows, "take_of", ())
    bars = []
    for i, w in enumerate(rows[:, 0].tolist()):
        f = form_row_fields(w)
        if f is None:
            bars.append(None)
            continue
        bar = {"of": f[0], "copy": f[1], "transpose": f[2]}
        if w & FORM_TAKE_BIT:
            bar = {"take": int(take_of[i]), **bar}
        bars.append(bar)
    if getattr(rows, "takes", ()):
        return {"takes": [tk.tolist() for tk in rows.takes], "bars": bars}
    return {"bars": bars}


def _form_takes_checked(x: "FormTakes") -> "FormTakes":
    """A FormTakes handed back in: the rows must still be the rows of its takes."""
    if x.ndim != 2 or x.shape[1] != 4 or not 1 <= x.shape[0] <= FORM_BARS_MAX or x.dtype != np.uint32:
        raise CommuHipError(f"form: a uint32 form is [1 .. {FORM_BARS_MAX}][4], got {x.dtype} {x.shape}")
    if len(x.take_of) != x.shape[0]:
        raise CommuHipError(f"form: {x.shape[0]} rows beside take_of for {len(x.take_of)} bars (a slice of a form with "
                            "takes is not one)")
    for i, (w, begin, end, w3) in enumerate(np.asarray(x).tolist()):
        f, k = form_row_fields(w), x.take_of[i]
        ok = w >> 15 == 0 and w3 == 0 and (f is None or abs(f[2]) <= FORM_TRANSPOSE_MAX and not (f[1] == "rhythm" and f[2]))
        if f is not None and w & FORM_TAKE_BIT:
            ok = ok and 0 <= k < len(x.takes) and 0 <= begin < end <= x.takes[k].size
        else:
            ok = ok and k < 0 and begin == 0 and end == 0 and (w == 0 if f is None else f[0] < i)
        if not ok:
            raise CommuHipError(f"form: bar {i}: not a row of a form over its takes: {[w, begin, end, w3]}, take_of {k}")
    return x


def form_template(x) -> np.ndarray:
    """A form as uint32 [R][4], one row per bar (word 0: form_row_word, 0 for a free bar; words 1 .. 3 are 0).  x: a letter
    string such as "AABA" -- the first bar with a letter is free, later ones replay it in full; {"bars": [null | j |
    {"of": j, "copy": "all" | "rhythm", "transpose": s}, ...]} -- bar i is free or replays bar j < i, everything or the
    rhythm only (the pitches are then drawn), transposed by s semitones (all only, -48 .. 48); JSON text or the path of a
    file holding either; or a uint32 array [R][4] that is one already.  1 <= R <= 64, bar 0 is always free.  Pure host code;
    raises CommuHipError that names the bar.
    TAKES: {"takes": [[ids], ...] | {"from_tokens": [ids]}, "bars": [null | j | {"of": j, ...} | {"take": t, "of": j,
    "copy": ..., "transpose": s}, ...]} -- a bar with "take" replays bar j of take t (null: the only take), a finished token
    sequence of the user's, whose bars are the stretches behind its Bar tokens (form_take_bars); any bar of the form, bar 0
    included, may name one.  The short form {"keep": {"from_tokens": [ids]}, "redo": [bars], "repitch": [bars]} keeps every
    bar of the take (up to 64) except those listed: a bar in redo is free, a bar in repitch takes the take's rhythm and draws
    its pitches; an entry of redo or repitch from 64 on names a bar the take has and the form does not reach -- no row is
    made for it, bars past the 64th are free.  Such a form comes back as a FormTakes: the rows with the takes' tokens beside
    them; given one, its rows are checked against its takes (a slice or an edited copy whose take_of no longer lines up with
    its rows, or whose begin / end leave the take, is refused).
    ONE INPUT accepted before the takes is refused now: a plain uint32 array whose word 0 has bit 7 set.  The kernels
    ignored the bit then and read it as "a take row" now, so such a row would silently become a free bar."""
    if isinstance(x, FormTakes) and x.takes:
        return _form_takes_checked(x)
    if isinstance(x, np.ndarray) and x.dtype == np.uint32:
        if x.ndim != 2 or x.shape[1] != 4 or not 1 <= x.shape[0] <= FORM_BARS_MAX:
            raise CommuHipError(f"form: a uint32 form is [1 .. {FORM_BARS_MAX}][4], got shape {x.shape}")
        for i, w in enumerate(x[:, 0].tolist()):
            f = form_row_fields(w)
            # (a take row cannot stand without its take: bit 7 belongs to a FormTakes)
            ok = f is None and w == 0 or f is not None and w >> 15 == 0 and f[0] < i and abs(f[2]) <= FORM_TRANSPOSE_MAX \
                and not (f[1] == "rhythm" and f[2] != 0) and not w & FORM_TAKE_BIT
            if not ok or x[i, 1:].any():
                raise CommuHipError(f"form: bar {i}: not a row of a form: {x[i].tolist()}")
        return np.ascontiguousarray(x)
    if isinstance(x, str):
        text = x.strip()
        if not text.isalpha() and not text.startswith(("{", "[", '"')):
            try:
                with open(x) as f:
                    text = f.read().strip()
            except OSError as e:
                raise CommuHipError(f"form: letters, JSON text or a readable file expected, got {x!r} ({e.strerror})") from None
        if text.isalpha():
            first = {}
            x = {"bars": [None if first.setdefault(c, i) == i else first[c] for i, c in enumerate(text)]}
        else:
            try:
                doc = json.loads(text)
            except json.JSONDecodeError as e:
                raise CommuHipError(f"form: not JSON ({e})") from None
            if isinstance(doc, str) and not doc.isalpha():
                raise CommuHipError(f"form: a letter string such as \"AABA\" expected, got {doc!r}")
            return form_template(doc)
    if isinstance(x, dict) and "keep" in x and set(x) <= FORM_KEEP_KEYS:
        x = _form_keep(x)
    if isinstance(x, dict) and set(x) == {"takes", "bars"}:
        return _form_with_takes(x)
    if not isinstance(x, dict) or set(x) != {"bars"} or not isinstance(x["bars"], (list, tuple)):
        raise CommuHipError('form: a letter string or {"bars": [null | j | {"of": j, "copy": ..., "transpose": s}, ...]} '
                            f"expected, got {x!r}")
    bars = x["bars"]
    if not 1 <= len(bars) <= FORM_BARS_MAX:
        raise CommuHipError(f"form: a form holds 1 .. {FORM_BARS_MAX} bars, got {len(bars)}" +
                            (f" (bar {FORM_BARS_MAX} is one too many)" if bars else ""))
    out = np.zeros((len(bars), 4), dtype=np.uint32)
    for i, bar in enumerate(bars):
        out[i, 0] = _form_bar(i, bar)
    return out


def form_is_rhythm(rows) -> bool:
    """Does a form (uint32 rows) hold a bar in rhythm mode?"""
    return any(f is not None and f[1] == "rhythm" for f in map(form_row_fields, rows[:, 0].tolist()))


def _form_needs_grammar(forms, gram_on):
    """A rhythm bar draws its pitches: without the event grammar the draw at that place need not be a pitch.  Refused where
    a sequence asks for one and its grammar is off.  gram_on: the sequences whose grammar is on."""
    on = set(int(b) for b in gram_on)
    for i, f in enumerate(forms):
        if f is not None and form_is_rhythm(f) and i not in on:
            raise CommuHipError('form: "copy": "rhythm" without the event grammar' +
                                (f" (sequence {i})" if len(forms) > 1 else "") +
                                ": the pitch of such a bar is drawn, and only the grammar makes that draw a pitch")


def _form_per_slot(x, B: int):
    """A request's form= as B entries, each None (off) or a form's uint32 rows: None / False (all off), one form in any form
    form_template takes (all slots), or a list of B entries each None / False or a form."""
    return _templates_per_slot("form", form_template, x, B)


def _form_key(t):
    """What tells two forms apart: the rows' bytes and, where they name takes, which take each row reads and its tokens
    (equal rows over different takes are different forms)."""
    takes = getattr(t, "takes", ())
    if not takes:
        return t.tobytes()
    return t.tobytes(), tuple(t.take_of), tuple(tk.tobytes() for tk in takes)


def _form_fold(pitch_token: int, s: int) -> int:
    m = int(pitch_token) - 3 + int(s)
    while m < 0:
        m += 12
    while m > 127:
        m -= 12
    return m + 3


def form_violation(seq, start: int, template, drawn=None):
    """The checker of the form rule, shared by the tests and by users: the first CLOSED replay bar of seq whose note groups
    do not match its source bar under the row's mode, as (bar, source bar, reason), else None.  Bar i is the stretch between
    the (i+1)-th Bar token and the next Bar (or the Eos that replaced it); it is closed when that token exists.  A bar is a
    replay bar when the form's row says so AND the loop opened it itself: its Bar token lies at index >= start (the bar a
    prompt leaves open is free).  Its note groups (Position, Velocity, Pitch, Duration, found one behind the other as the
    rule finds them) must equal the source's one for one -- the pitch transposed and folded into 0 .. 127 (all), or any
    pitch (rhythm).  template: anything form_template takes.  drawn (optional, parallel to seq): True where a token was drawn
    by the sampling step (it has a log-probability); then the replayed tokens must not be, and the pitches of a rhythm bar
    must be.  A take row's source bar is the bar of its take (the returned source bar is the take's), and a take row's bar is
    a replay bar whatever its index."""
    rows = form_template(template)
    seq = [int(t) for t in seq]
    bar_at = [i for i, t in enumerate(seq) if t == ONSET_BAR]

    def close_of(i):
        nxt = bar_at[i + 1] if i + 1 < len(bar_at) else None
        if nxt is None and seq and seq[-1] == 1 and bar_at:            # (the Eos that replaced the last Bar)
            nxt = len(seq) - 1
        return nxt

    def groups_in(buf, g, end):
        out = []
        while g + 3 < end:
            if _is_note_at(buf, g) and g + 3 < end:
                out.append(g)
                g += 4
            else:
                g += 1
        return out

    def groups(i):
        return groups_in(seq, bar_at[i] + 1, close_of(i))
    for i in range(min(len(bar_at), len(rows), FORM_BARS_MAX)):
        f = form_row_fields(rows[i, 0])
        if f is None or bar_at[i] < int(start) or close_of(i) is None or close_of(i) <= bar_at[i]:
            continue
        j, copy, s = f
        from_seq = seq
        if int(rows[i, 0]) & FORM_TAKE_BIT:                    # (a take row: the source bar lies in its take)
            from_seq = [int(t) for t in rows.takes[rows.take_of[i]]]
            src = groups_in(from_seq, int(rows[i, 1]), min(int(rows[i, 2]), len(from_seq)))
        else:
            src = groups(j)
        dst = groups(i)
        if len(src) != len(dst):
            return i, j, f"{len(dst)} note groups, the source has {len(src)}"
        for a, b in zip(src, dst):
            want = [from_seq[a], from_seq[a + 1], _form_fold(from_seq[a + 2], s), from_seq[a + 3]]
            got = seq[b:b + 4]
            if copy == "rhythm":
                want[2] = got[2]
            if want != got:
                return i, j, f"group at index {b} is {got}, the source's at {a} gives {want}"
            if drawn is not None:
                d = [bool(drawn[b + k]) for k in range(4)]
                if d != [False, False, copy == "rhythm", False]:
                    return i, j, f"group at index {b}: drawn flags {d}"
    return None


class DecodeState:
    """K/V caches + distance-indexed R tables for B sequences of up to Lmax positions.

    window=M selects the reference's SLIDING memory (model.py:507-538): the cache of a sequence is a ring of M + 1 rows
    (Lmax is then derived), position p lives in row p mod (M + 1), and klen[b] -- "positions kept so far" in both modes --
    keeps counting beyond the ring (the kernels derive the row from it).  Without a window the cache is linear and klen
    saturates at its last row.

    kv_dtype="fp8" (opt-in; csrc/decode_kv8.hip) stores K and V as e4m3 bytes with one power-of-two scale byte per 32
    features: kc8 / vc8 uint8 [L, B, H, Lmax, DH] and ks / vs uint8 [L, B, H, Lmax, DH / 32] instead of kc / vc, 0.516 of the
    bf16 cache's bytes.  The mode rounds the stored K and V and nothing else (a position has one K and one V, whatever
    step reads it); it carries no parity claim and is refused together with model.parity_fp32.

    shared_prefix=Pcap (opt-in; csrc/decode_prefix.hip) holds the positions that ALL slots have in common once: pk / pv bf16
    [L, H, Pcap, DH] with prefix_len (one int32 word on the device) valid rows, filled by prefill_shared().  The cache
    kc / vc [L, B, H, Lmax, DH] then holds the PRIVATE rows only: row r of slot b is absolute position prefix_len + r, klen[b]
    counts private rows and starts at 0.  Every step computes what the unshared state computes over a cache that holds the
    prefix in every slot (relative scores depend on the distance only).  bf16 linear cache only: refused together with
    window, kv_dtype="fp8" and model.parity_fp32."""

    MAX_POSITIONS = 4224          # cache rows the decode attention kernel supports (commu_decode_attn)
    KLEN_UNBOUNDED = 1 << 30      # the length bound handed to the book-keeping kernels in window mode
    KV_DTYPES = ("bf16", "fp8")

    def __init__(self, model, B: int, Lmax: int, window: Optional[int] = None, kv_dtype: str = "bf16",
                 shared_prefix: Optional[int] = None):
        if kv_dtype not in self.KV_DTYPES:
            raise CommuHipError(f"kv_dtype: one of {self.KV_DTYPES} expected, got {kv_dtype!r}")
        if shared_prefix is not None:          # (refused before anything is allocated; each of the three is a follow-up)
            shared_prefix = int(shared_prefix)
            if window is not None:
                raise CommuHipError("shared_prefix with a sliding window: a ring would wrap over the shared rows; the shared "
                                    "prompt prefix is built for the linear cache only")
            if kv_dtype == "fp8":
                raise CommuHipError("shared_prefix with kv_dtype='fp8': the shared prompt prefix is built for the bf16 cache "
                                    "only")
            if bool(getattr(model, "parity_fp32", False)):
                raise CommuHipError("shared_prefix with the fp32 parity mode (model.parity_fp32): the shared prompt prefix is "
                                    "built for the bf16 cache only")
            if shared_prefix < 1:
                raise CommuHipError(f"shared_prefix: a capacity of at least one position expected, got {shared_prefix}")
            if shared_prefix + Lmax > self.MAX_POSITIONS:
                raise CommuHipError(f"a shared prefix of up to {shared_prefix} positions and {Lmax} private rows need "
                                    f"{shared_prefix + Lmax} positions; this build supports {self.MAX_POSITIONS}")
        self.shared_prefix = shared_prefix
        if kv_dtype == "fp8" and bool(getattr(model, "parity_fp32", False)):
            raise CommuHipError("kv_dtype='fp8' rounds the cached K and V; the fp32 parity mode (model.parity_fp32) exists to be "
                                "exact: choose one")
        self.kv_dtype = kv_dtype
        if window is not None:
            window = int(window)
            if window < 1:
                raise CommuHipError(f"a sliding decode memory needs at least one position, got {window}")
            Lmax = window + 1
        self.window = window
        # what klen saturates at (commu_decode_advance, commu_forcing_post, commu_decode_sample_post_pre)
        self.klen_cap = Lmax if window is None else self.KLEN_UNBOUNDED
        if Lmax > self.MAX_POSITIONS:
            raise CommuHipError(f"decode cache of {Lmax} positions requested; this build supports {self.MAX_POSITIONS} "
                                "(the reference's 1 + 4146 fits)")
        if getattr(model, "ffn_activation", "relu") != "relu":
            raise CommuHipError("the cached decode step is built for the reference's ReLU FFN only")
        self.model, self.B, self.Lmax = model, B, Lmax
        self.attn_splits, self.split_ws, self.split_cnt = 1, None, None
        # fp32 parity mode (model.parity_fp32, read when the state is built): fp32 weights, activations and K/V cache, the
        # kernels of csrc/parity_f32.hip -- the mode that carries the "bit-exact greedy tokens" claim
        self.parity = bool(getattr(model, "parity_fp32", False))
        if self.parity:
            return self._init_f32()
        fl = model._ensure_flat()
        dev = fl["dev"]
        # kernel-side dimensions (zero-padded when the model's are not multiples of 64 / 32, see model.py)
        L, D = model.n_layer, model._Dp
        H, DH = model.n_head, model._DHp
        HD = H * DH
        if kv_dtype == "fp8":
            u8 = torch.uint8          # e4m3 bytes + one E8M0 scale byte per 32 features (include/commu_hip.h)
            self.kc8, self.vc8 = (torch.zeros(L, B, H, Lmax, DH, device=dev, dtype=u8) for _ in range(2))
            self.ks, self.vs = (torch.zeros(L, B, H, Lmax, DH // 32, device=dev, dtype=u8) for _ in range(2))
        else:
            self.kc = torch.zeros(L, B, H, Lmax, DH, device=dev, dtype=BF16)      # head-major: contiguous per (b, h)
            self.vc = torch.zeros(L, B, H, Lmax, DH, device=dev, dtype=BF16)
        self.klen = torch.zeros(B, device=dev, dtype=torch.int32)
        n_dist = Lmax          # rows of the distance tables
        if shared_prefix is not None:
            self.pk = torch.zeros(L, H, shared_prefix, DH, device=dev, dtype=BF16)      # head-major like the cache
            self.pv = torch.zeros(L, H, shared_prefix, DH, device=dev, dtype=BF16)
            self.prefix_len = torch.zeros(1, device=dev, dtype=torch.int32)             # P: read by the kernels
            self.prefix_ws, self.prefix_cnt = None, None
            n_dist = shared_prefix + Lmax          # (a key of the prefix is up to P + Lmax - 1 away)
        self._pd = ops.posemb(model.pos_emb.inv_freq, n_dist, model.d_model, ld=D, clamp_len=int(model.clamp_len))
        self.rd = [ops.gemm_nt(self._pd, model._weights(i)["r"]) for i in range(L)]
        self.logits = torch.zeros(B, VPAD, device=dev, dtype=F32)          # persistent: re-draws read them again (Q5)
        self.logits_new = torch.zeros(B, VPAD, device=dev, dtype=F32)      # this step's logits before the row select
        self.qkv = torch.zeros(B, 3 * HD, device=dev, dtype=BF16)
        self.vec = torch.zeros(B, HD, device=dev, dtype=BF16)
        # layer-tail launches: hand-off buffers per layer, arrival counters per launch, give-up flag
        DI = model._DIp
        # (the logits launch takes 512 < V <= 1024 only: other vocabularies use the per-Linear launches)
        self.tail_ok = bool(call("commu_decode_tail_supported", B, D, DI, HD)) and L > 0 and 512 < model.n_token <= 1024
        if self.tail_ok:
            nw = call("commu_decode_tail_sync_words_for", B)          # (B <= 64: commu_decode_tail_sync_words())
            self.t_z1 = torch.zeros(L, B, D, device=dev, dtype=BF16)
            self.t_hid = torch.zeros(L, B, DI, device=dev, dtype=BF16)
            self.t_z2 = torch.zeros(L, B, D, device=dev, dtype=BF16)
            self.t_h = torch.zeros(L, B, D, device=dev, dtype=BF16)
            self.t_h0 = torch.zeros(B, D, device=dev, dtype=BF16)
            self.t_sync = torch.zeros(L, nw, device=dev, dtype=torch.int32)
            self.t_err = torch.zeros(1, device=dev, dtype=torch.int32)
            self.t_packs = None
            self.repack()

    def cache_tensors(self):
        """The tensors that make up the K/V cache: (kc, vc), or (kc8, vc8, ks, vs) with kv_dtype="fp8".  Position rows are
        dimension 3 ([L, B, H, Lmax, .]); fp32 parity mode: dimension 2 ([L, B, Lmax, H DH]).  shared_prefix: the private
        caches and the prefix, (kc, vc, pk, pv)."""
        if self.shared_prefix is not None:
            return (self.kc, self.vc, self.pk, self.pv)
        return (self.kc8, self.vc8, self.ks, self.vs) if self.kv_dtype == "fp8" else (self.kc, self.vc)

    def cache_bytes(self) -> int:
        """Bytes held by the K/V cache (all layers, slots and rows)."""
        return sum(t.numel() * t.element_size() for t in self.cache_tensors())

    # ---- fp32 parity mode ------------------------------------------------------------------------------------------
    def _init_f32(self):
        m = self.model
        dev = next(m.parameters()).device
        if dev.type != "cuda":
            raise CommuHipError("the decode state lives on an MI355X (no CPU fallback)")
        B, Lmax = self.B, self.Lmax
        L, D, DI, H, DH, V = m.n_layer, m.d_model, m.d_inner, m.n_head, m.d_head, m.n_token
        HD = H * DH
        z = lambda *shape: torch.zeros(*shape, device=dev, dtype=F32)
        self.kc, self.vc = z(L, B, Lmax, HD), z(L, B, Lmax, HD)          # [layer][sequence][position][head * d_head]
        self.klen = torch.zeros(B, device=dev, dtype=torch.int32)
        self._pd = ops.posemb_f32(m.pos_emb.inv_freq, Lmax, D, clamp_len=int(m.clamp_len))
        self.rd = [z(Lmax, HD) for _ in range(L)]
        self.logits, self.logits_new = z(B, VPAD), z(B, VPAD)
        self.tail_ok = False
        self.f32 = {"h0": z(B, D), "qkv": z(B, 3 * HD), "vec": z(B, HD), "z1": z(B, D), "a": z(B, D), "hid": z(B, DI),
                    "z2": z(B, D), "h": [z(B, D) for _ in range(L)]}
        self.repack()

    def _prefill_f32(self, ctx):
        m = self.model
        T0, B = ctx.shape
        _, _, qkvs = m._run_forward_f32(ctx, None, want_kv=True)
        HD = m.n_head * m.d_head
        for i, qkv in enumerate(qkvs):
            kv = qkv.view(T0, B, 3, HD)
            if self.window is not None:
                first, rows = self._ring_rows(T0)
                self.kc[i].index_copy_(1, rows, kv[first:, :, 1].permute(1, 0, 2))
                self.vc[i].index_copy_(1, rows, kv[first:, :, 2].permute(1, 0, 2))
                continue
            self.kc[i, :, :T0].copy_(kv[:, :, 1].permute(1, 0, 2))
            self.vc[i, :, :T0].copy_(kv[:, :, 2].permute(1, 0, 2))
        self.klen.fill_(T0)

    def _ring_rows(self, T0):
        """Window mode: (first kept position, ring rows) of the last min(T0, window) positions of a T0-token context."""
        first = max(0, T0 - self.window)
        return first, (torch.arange(first, T0, device=self.klen.device) % self.Lmax)

    def _step_f32(self, tokens, active, keep, want_logits):
        """step() on fp32 operands: per layer [qkv_net, K/V append, cached attention over the ragged memories, o_net +
        residual, LayerNorm, FFN, LayerNorm], then the tied output layer (model.py:283-352,163-181,46).  Static buffers
        only: capturable."""
        m, f = self.model, self.f32
        B, L, H, DH = self.B, m.n_layer, m.n_head, m.d_head
        HD, V = H * DH, m.n_token
        E = m.word_emb.emb_layers[0].weight
        h = ops.embed_f32(tokens, E, out=f["h0"])
        u, vb = m.r_w_bias, m.r_r_bias
        for i in range(L):
            lay = m.layers[i]
            att, ff = lay.dec_attn, lay.pos_ff
            ops.gemm_nt_f32(h, att.qkv_net.weight, out=f["qkv"])
            if self.window is not None:
                ops.decode_kv_append_ring_f32(f["qkv"], self.kc[i], self.vc[i], self.klen, active, HD, self.Lmax)
                ops.decode_attn_ring_f32(f["qkv"][:, :HD], self.kc[i], self.vc[i], self.rd[i], u, vb, self.klen, H, DH,
                                         self.Lmax, bool(m.same_length), m.attn_scale, out=f["vec"])
            else:
                ops.decode_kv_append_f32(f["qkv"], self.kc[i], self.vc[i], self.klen, active, HD, self.Lmax)
                ops.relattn_f32(f["qkv"][:, :HD], self.kc[i], self.vc[i], HD, self.Lmax * HD, self.rd[i], u, vb, 1, 0, B, H,
                                DH, bool(m.same_length), int(m.mem_len), m.attn_scale, klen=self.klen, out=f["vec"])
            ops.gemm_nt_f32(f["vec"], att.o_net.weight, resid=h, out=f["z1"])
            ops.layernorm_fwd_f32(f["z1"], att.layer_norm.weight, att.layer_norm.bias, att.layer_norm.eps, out=f["a"], stats=False)
            ops.gemm_nt_f32(f["a"], ff.CoreNet[0].weight, bias=ff.CoreNet[0].bias, relu=True, out=f["hid"])
            ops.gemm_nt_f32(f["hid"], ff.CoreNet[3].weight, bias=ff.CoreNet[3].bias, resid=f["a"], out=f["z2"])
            h = ops.layernorm_fwd_f32(f["z2"], ff.layer_norm.weight, ff.layer_norm.bias, ff.layer_norm.eps, out=f["h"][i],
                                      stats=False)[0]
        if keep is not None:
            call("commu_decode_advance", _p(self.klen), _p(keep), B, self.klen_cap, _s())
        if want_logits:
            dst = self.logits if active is None else self.logits_new
            ops.gemm_nt_f32(h, E, bias=m.crit.out_layers[0].bias, out=dst[:, :V])
            if active is not None:
                call("commu_copy_rows_masked_f32", _p(self.logits), VPAD, _p(self.logits_new), VPAD, _p(active), B, V, _s())
        return self.logits

    def prefill(self, ctx: torch.Tensor):
        """ctx: int64 [T0, B] context tokens (midi_inferrer.py:186-197): fills the caches with their K/V
        (same kernels as training, memory-less forward) and sets klen = T0.  Window mode: the context may be longer than
        the window; the K/V of its last min(T0, window) positions go to their ring rows."""
        m = self.model
        T0, B = ctx.shape
        assert B == self.B
        if self.window is None and T0 >= self.Lmax:
            raise CommuHipError(f"context of {T0} tokens does not fit a decode cache of {self.Lmax} positions")
        if self.parity:
            return self._prefill_f32(ctx)
        if self.kv_dtype == "fp8":          # (equal lengths, default slots: the quantising scatter is the only way in)
            return self.prefill_ragged(ctx, [T0] * B)
        _, _, qkvs = m._run_forward(ctx, None, None, None, need_grad=False, want_logits=True, want_kv=True)
        H, DH = m.n_head, m._DHp
        for i, qkv in enumerate(qkvs):
            kv = qkv.view(T0, B, 3, H, DH)
            if self.window is not None:
                first, rows = self._ring_rows(T0)
                self.kc[i].index_copy_(2, rows, kv[first:, :, 1].permute(1, 2, 0, 3))
                self.vc[i].index_copy_(2, rows, kv[first:, :, 2].permute(1, 2, 0, 3))
                continue
            self.kc[i, :, :, :T0].copy_(kv[:, :, 1].permute(1, 2, 0, 3))
            self.vc[i, :, :, :T0].copy_(kv[:, :, 2].permute(1, 2, 0, 3))
        self.klen.fill_(T0)

    def prefill_ragged(self, ctx: torch.Tensor, lens, slots=None):
        """prefill() for contexts of different lengths: ctx int64 [Tmax, Bc] holds context b in ctx[:lens[b], b] (what
        stands beyond is padding: the memory-less forward is causal, no valid row depends on it), lens int32 [Bc] (device
        tensor or a sequence), slots (optional, int32 [Bc]) names the decode slot of each context (default: b).  One
        forward over the padded batch, then ONE launch per layer (commu_decode_prefill_scatter) that moves the K/V of the
        valid positions -- window mode: the last min(lens[b], window) of them, to their ring rows -- and sets
        klen[slot] = lens[b].  Rows of other slots and rows beyond a context are not touched."""
        m = self.model
        Tmax, Bc = ctx.shape
        dev = self.klen.device
        if Tmax < 1 or Bc < 1:
            raise CommuHipError(f"ctx: at least one position and one context expected, got shape {tuple(ctx.shape)}")

        def rows(x, name):
            if x is None:
                return None, None
            host = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(list(x))
            if host.shape != (Bc,):
                raise CommuHipError(f"{name}: {Bc} values expected (one per context), got shape {host.shape}")
            t = x if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() \
                else torch.from_numpy(host.astype(np.int32)).to(dev)
            return t, host
        lens_t, lens_h = rows(lens, "lens")
        slots_t, slots_h = rows(slots, "slots")
        if lens_t is None:
            raise CommuHipError("lens: the length of every context is needed")
        if lens_h.min() < 0 or lens_h.max() > Tmax:
            raise CommuHipError(f"lens: values in [0, {Tmax}] expected, got {int(lens_h.min())} .. {int(lens_h.max())}")
        if slots_h is None and Bc != self.B:
            raise CommuHipError(f"{Bc} contexts for {self.B} slots: name the slots")
        if slots_h is not None and (slots_h.min() < 0 or slots_h.max() >= self.B or len(set(slots_h.tolist())) != Bc):
            raise CommuHipError(f"slots: {Bc} different slot numbers in [0, {self.B}) expected, got {slots_h.tolist()}")
        if self.window is None and int(lens_h.max()) >= self.Lmax:
            raise CommuHipError(f"context of {int(lens_h.max())} tokens does not fit a decode cache of {self.Lmax} positions")
        if self.parity:
            _, _, qkvs = m._run_forward_f32(ctx, None, want_kv=True)
        else:
            _, _, qkvs = m._run_forward(ctx, None, None, None, need_grad=False, want_logits=True, want_kv=True)
        for i, qkv in enumerate(qkvs):
            if self.kv_dtype == "fp8":
                ops.decode_prefill_scatter_kv8(qkv.view(Tmax * Bc, -1), Tmax, self.kc8[i], self.vc8[i], self.ks[i], self.vs[i],
                                               self.klen, lens_t, slots_t, window=self.window or 0)
                continue
            ops.decode_prefill_scatter(qkv.view(Tmax * Bc, -1), Tmax, self.kc[i], self.vc[i], self.klen, lens_t, slots_t,
                                       window=self.window or 0)

    def prefill_shared(self, ctx_column: torch.Tensor):
        """shared_prefix: the K/V of the positions every slot has in common.  ctx_column: int64 [P] (or [P, 1]) tokens; ONE
        memory-less forward over that single column, then one commu_decode_prefill_scatter launch per layer (one context,
        one slot: source and destination layouts are the prefill's) moves them into pk / pv and sets prefix_len = P.  Every
        slot then starts with no private rows (klen = 0)."""
        if self.shared_prefix is None:
            raise CommuHipError("prefill_shared: this decode state was built without shared_prefix")
        col = ctx_column.reshape(-1, 1).to(self.klen.device)
        P = col.shape[0]
        if P < 1 or P > self.shared_prefix:
            raise CommuHipError(f"a shared prefix of {P} positions was given; this state holds 1 .. {self.shared_prefix}")
        _, _, qkvs = self.model._run_forward(col, None, None, None, need_grad=False, want_logits=True, want_kv=True)
        lens = torch.full((1,), P, device=self.klen.device, dtype=torch.int32)
        for i, qkv in enumerate(qkvs):
            ops.decode_prefill_scatter(qkv.view(P, -1), P, self.pk[i].unsqueeze(0), self.pv[i].unsqueeze(0), self.prefix_len,
                                       lens)
        self.klen.zero_()

    def _attn_prefix(self, i, u, vb, active, B, H, DH, scale):
        """_attn with a shared prefix (commu_decode_attn_prefix): one launch does the prefix part once per group of slots,
        the private part per slot and the merge.  attn_splits splits the PRIVATE keys."""
        if self.prefix_ws is None:
            n = ops.decode_prefix_ws_floats(B, H, DH, self.shared_prefix, 16)          # (any nsplit the policy may choose)
            self.prefix_ws = torch.empty(n, device=self.qkv.device, dtype=torch.float32)
            self.prefix_cnt = torch.zeros(B * H, device=self.qkv.device, dtype=torch.int32)
        ops.decode_attn_prefix(self.qkv, self.pk[i], self.pv[i], self.prefix_len, self.kc[i], self.vc[i], self.rd[i], u, vb,
                               self.klen, active, self.vec, scale, self.prefix_ws, self.prefix_cnt, append=True,
                               nsplit=int(self.attn_splits))

    def _attn(self, i, u, vb, active, B, H, DH, scale):
        """Cached attention of layer i (K/V append fused in).  attn_splits > 1: the keys of a (sequence, head) pair over
        several workgroups (long memories, few live sequences); pairs with fewer than 512 keys run unsplit either way.
        Window mode: the ring variant of the same kernel (commu_decode_attn_ring)."""
        if self.shared_prefix is not None:
            return self._attn_prefix(i, u, vb, active, B, H, DH, scale)
        if self.attn_splits > 1 and self.split_ws is None:
            self.split_ws = torch.empty(B * H * 16 * (DH + 2), device=self.qkv.device, dtype=torch.float32)
            self.split_cnt = torch.zeros(B * H, device=self.qkv.device, dtype=torch.int32)
        if self.kv_dtype == "fp8":          # one entry point: linear / ring, unsplit / split-key
            ops.decode_attn_kv8(self.qkv, self.kc8[i], self.vc8[i], self.ks[i], self.vs[i], self.rd[i], u, vb, self.klen,
                                active, self.vec, scale, append=True, ring=self.window is not None,
                                same_length=bool(self.model.same_length), nsplit=int(self.attn_splits),
                                split_ws=self.split_ws, split_cnt=self.split_cnt)
        elif self.window is not None:
            ops.decode_attn_ring(self.qkv, self.kc[i], self.vc[i], self.rd[i], u, vb, self.klen, active, self.vec, self.Lmax,
                                 scale, append=True, same_length=bool(self.model.same_length), nsplit=int(self.attn_splits),
                                 split_ws=self.split_ws, split_cnt=self.split_cnt)
        elif self.attn_splits > 1:
            call("commu_decode_attn_split", _p(self.qkv), self.qkv.stride(0), _p(self.kc[i]), _p(self.vc[i]),
                 _p(self.rd[i]), self.rd[i].stride(0), _p(u), _p(vb), _p(self.klen), _p(active),
                 _p(self.vec), self.vec.stride(0), B, H, DH, self.Lmax, scale, 1, int(self.attn_splits),
                 _p(self.split_ws), _p(self.split_cnt), _s())
        else:
            call("commu_decode_attn", _p(self.qkv), self.qkv.stride(0), _p(self.kc[i]), _p(self.vc[i]),
                 _p(self.rd[i]), self.rd[i].stride(0), _p(u), _p(vb), _p(self.klen), _p(active),
                 _p(self.vec), self.vec.stride(0), B, H, DH, self.Lmax, scale, 1, _s())

    def step(self, tokens: torch.Tensor, active: Optional[torch.Tensor], keep: Optional[torch.Tensor], want_logits=True):
        """One decode step for the sequences with active[b] != 0; klen advances where keep[b] != 0 (keep = None: the
        caller advances the lengths itself, ForcedDecoder does it in its book-keeping kernel).
        tokens int64 [B]; active/keep uint8 [B].  Returns the fp32 logits buffer [B, 768] (rows of inactive
        sequences keep their previous content -- they may still be needed for a re-draw, quirk Q5).
        No host synchronisation, no data-dependent allocation: safe inside a hipGraph capture.

        Kernel chain per layer: QKV Linear -> cached attention (K/V append fused in) -> o_net Linear + residual ->
        FFN Linear 1 -> FFN Linear 2 + residual; the two LayerNorms (model.py:352,179) run INSIDE the Linear that
        consumes them (commu_gemm_nt_ln_bf16), which also stores the normalised rows for the next residual add."""
        m = self.model
        if self.parity:
            return self._step_f32(tokens, active, keep, want_logits)
        B, L, H, DH, D = self.B, m.n_layer, m.n_head, m._DHp, m._Dp
        if USE_LAYER_TAIL and self.tail_ok:
            return self._step_tail(tokens, active, keep, want_logits)
        h = ops.embed_fwd(tokens, m.word_emb.emb_layers[0].weight, ld=D)
        scale = m.attn_scale
        u, vb = m._uv()
        z2, ln2 = None, None          # pre-LayerNorm output of the previous layer's FFN and that LayerNorm
        for i in range(L):
            w = m._weights(i)
            lay = m.layers[i]
            if z2 is None:
                ops.gemm_nt(h, w["qkv"], out=self.qkv)
            else:                     # h = LN2(z2) of the layer below, computed on the fly and stored
                h = torch.empty_like(z2)
                ops.gemm_nt_ln(z2, ln2.weight, ln2.bias, w["qkv"], out=self.qkv, a_out=h, eps=ln2.eps)
            self._attn(i, u, vb, active, B, H, DH, scale)                                    # (K/V append fused in)
            z1 = ops.gemm_nt(self.vec, w["o"], resid=h)
            ln1 = lay.dec_attn.layer_norm
            a = torch.empty_like(z1)
            hid = ops.gemm_nt_ln(z1, ln1.weight, ln1.bias, w["w1"], a_out=a, bias=w["b1"], relu=True, eps=ln1.eps)
            z2 = ops.gemm_nt(hid, w["w2"], bias=w["b2"], resid=a)
            ln2 = lay.pos_ff.layer_norm
        if keep is not None:
            call("commu_decode_advance", _p(self.klen), _p(keep), B, self.klen_cap, _s())
        if want_logits:
            V = m.n_token
            dst = self.logits if active is None else self.logits_new
            ops.gemm_nt_ln(z2, ln2.weight, ln2.bias, m._emb_bf16(), out=dst[:, :V], bias=m.crit.out_layers[0].bias,
                           eps=ln2.eps)
            if active is not None:       # only the rows of the sequences that stepped are replaced
                call("commu_copy_rows_masked_f32", _p(self.logits), VPAD, _p(self.logits_new), VPAD, _p(active),
                     B, V, _s())
        return self.logits


    def repack(self):
        """Refresh what the decode step derives from the weights -- the distance tables and the packed weight copies the
        layer-tail launches read (commu_decode_tail_pack): call again whenever the model's weights changed.  Everything is
        rewritten IN PLACE: a captured graph keeps pointing at the same buffers."""
        m = self.model
        if self.parity:
            for i in range(m.n_layer):
                ops.gemm_nt_f32(self._pd, m.layers[i].dec_attn.r_net.weight, out=self.rd[i])
            return
        for i in range(m.n_layer):          # the distance tables r_net(pos_emb) depend on the weights too
            ops.gemm_nt(self._pd, m._weights(i)["r"], out=self.rd[i])
        if not self.tail_ok:
            return

        def pack(wt, out):
            n, k = wt.shape
            if out is None:
                out = torch.empty(call("commu_decode_tail_pack_bytes", n, k) // 2, device=wt.device, dtype=BF16)
            call("commu_decode_tail_pack", _p(wt), wt.stride(0), n, k, _p(out), _s())
            return out
        old = self.t_packs
        packs = []
        for i in range(m.n_layer):
            w = m._weights(i)
            packs.append({k: pack(w[k], None if old is None else old[i][k]) for k in ("qkv", "o", "w1", "w2")})
        self.t_packs = packs
        self.t_pack_e = pack(m._emb_bf16(), None if old is None else self.t_pack_e)

    def _step_tail(self, tokens, active, keep, want_logits):
        """step() with one launch per layer after the attention (csrc/decode_tail.hip): embedding, layer 0's QKV Linear,
        then per layer [cached attention, layer tail]; the tail of layer i ends with layer i + 1's QKV Linear, the last
        one with the logits."""
        m = self.model
        B, L, H, DH, D = self.B, m.n_layer, m.n_head, m._DHp, m._Dp
        HD, DI = H * DH, m._DIp
        V = m.n_token
        E = m.word_emb.emb_layers[0].weight
        scale = m.attn_scale
        u, vb = m._uv()
        ws = [m._weights(i) for i in range(L)]
        h = self.t_h0
        pk = self.t_packs
        call("commu_decode_head", _p(tokens), _p(E), E.shape[1], E.shape[0], math.sqrt(E.shape[1]), _p(pk[0]["qkv"]),
             _p(h), D, _p(self.qkv), self.qkv.stride(0), B, D, DI, HD, _p(self.t_sync), self.t_sync.numel(), _s())
        dst = self.logits          # (the logits launch skips the rows of the sequences that did not step)
        for i in range(L):
            w, lay = ws[i], m.layers[i]
            self._attn(i, u, vb, active, B, H, DH, scale)
            last = i == L - 1
            if last and not want_logits:
                break
            ln1, ln2 = lay.dec_attn.layer_norm, lay.pos_ff.layer_norm
            if last:
                wn, nn_, bn, out_n, ld_on, h_out = self.t_pack_e, V, m.crit.out_layers[0].bias, dst, dst.stride(0), None
            else:
                wn, nn_, bn, out_n, ld_on, h_out = pk[i + 1]["qkv"], 3 * HD, None, self.qkv, self.qkv.stride(0), self.t_h[i]
            call("commu_decode_layer_tail", _p(self.vec), self.vec.stride(0), _p(h), h.stride(0),
                 _p(pk[i]["o"]), _p(pk[i]["w1"]), _p(w["b1"]), _p(pk[i]["w2"]), _p(w["b2"]), _p(ln1.weight), _p(ln1.bias),
                 float(ln1.eps), _p(ln2.weight), _p(ln2.bias), float(ln2.eps), ln1.weight.numel(), _p(wn), nn_, _p(bn),
                 1 if last else 0, _p(active), _p(self.t_z1[i]), _p(self.t_hid[i]), _p(self.t_z2[i]), _p(h_out), D,
                 _p(out_n), ld_on, B, D, DI, HD, _p(self.t_sync[i]), _p(self.t_err), _s())
            h = h_out
        if keep is not None:
            call("commu_decode_advance", _p(self.klen), _p(keep), B, self.klen_cap, _s())
        return self.logits

    def check(self):
        """Raises when a layer-tail launch gave up waiting for its peers (one D2H read: call it outside the loop)."""
        if self.tail_ok and int(self.t_err.item()) != 0:
            raise CommuHipError(f"decode layer-tail launch timed out at hand-off {int(self.t_err.item())}: its results are "
                                "invalid")


# The constraint tiers of the sampling step, as the kernels order them (csrc/decode_loop.h: Tier): a launch of a tier reads what
# every tier below it reads, so a decoder that enables one allocates, switched off, whatever it lacks below it.
T_NONE, T_GRAM, T_HARM, T_CLS, T_ORD, T_VOX, T_DEN, T_MEL, T_ONS, T_GDE, T_ART = range(11)


class SlotRule(NamedTuple):
    """One per-slot constraint of ForcedDecoder: control words int32 [B] on the device with a host mirror, and for the
    rules that own a template table the table's shape and how a template becomes rows and a word.  Every name follows from
    `stem` and `kw`: the decoder's attributes are <stem>_ctl and _<stem>_host, <stem>_table, _<stem>_table_host,
    _<stem>_used and _<stem>_index (class-level None / 0: a decoder that never enables the rule has none of them); the
    fields of the argument structs are <stem>_ctl, <stem>_table and <stem>_rows; the request store's words are e_<stem>;
    the keyword of every entry point and of ops.sample_topk is `kw`, the setter that holds the contract set_<kw>."""
    tier: int                        # the sampling tier whose launch reads the words; -1: none (the form: forcing stage)
    stem: str
    kw: str
    off: int                         # the word of a slot that is off
    normalize: Callable              # (value, n) -> the words (no table) or templates (None: off) of n slots
    asks: str                        # admit's refusal: what the request asks for that the decoder has no words of
    implies: str = ""                # the kw of the rule a slot that is on needs on too: where that is off it gets word 0
    template: Callable = None        # (table) value -> template
    lists: bool = False              # (table) a Python list is one value per slot, never one template
    rows_max: int = 0                # (table) rows of the device table, allocated once; 0: the rule has no table
    cycle_max: int = 0               # (table) bars of one template
    fill: tuple = ()                 # (table) a row that constrains nothing
    rows_of: Callable = None         # (table) template -> its uint32 [n][4] rows
    key: Callable = None             # (table) template -> what tells distinct templates apart
    bars: Callable = None            # (table) template -> its bars
    word: Callable = None            # (table) (base row, bars, template) -> control word

    ctl = property(lambda r: r.stem + "_ctl")
    host = property(lambda r: "_" + r.stem + "_host")
    table = property(lambda r: r.stem + "_table")
    table_host = property(lambda r: "_" + r.stem + "_table_host")
    used = property(lambda r: "_" + r.stem + "_used")
    index = property(lambda r: "_" + r.stem + "_index")
    entry = property(lambda r: "e_" + r.stem)
    setter = property(lambda r: "set_" + r.kw)

    def one(r, value):
        """A request's single setting, validated: the value itself (no table) or its template, None where it is off.
        Refuses one value per slot."""
        if not r.rows_max:
            if value is not None and np.ndim(value) != 0:
                raise CommuHipError(f"{r.kw}: one setting for the request expected, got shape {np.shape(value)}")
            return value
        if r.lists and isinstance(value, list):
            raise CommuHipError(f"{r.kw}: one setting for the request expected, got a list of {len(value)}")
        return None if (value is None or value is False) else r.template(value)

    def is_on(r, v) -> bool:
        """Is a normalised value (a word, or a template / None) a slot that is on?"""
        return v is not None if r.rows_max else v != r.off


_ONES = (0xFFFFFFFF,) * 4
ORDER = SlotRule(T_ORD, "order", "note_order", NOTE_ORDER_OFF, note_order_ctl,
                 "note order switched on, but the decoder has no note-order words")
VOICES = SlotRule(T_VOX, "voice", "voices", VOICES_OFF, voices_ctl, "a voice cap, but the decoder has no voice words",
                  implies="note_order")
DENSITY = SlotRule(T_DEN, "density", "density", DENSITY_OFF, density_ctl,
                   "a note density, but the decoder has no density words", implies="voices")
INTERVAL = SlotRule(T_MEL, "interval", "interval", INTERVAL_OFF, interval_ctl,
                    "a melodic interval, but the decoder has no interval words")
# (a template is the uint32 rows; a list is a template's bars)
ONSETS = SlotRule(T_ONS, "onset", "onsets", ONSETS_OFF, _onsets_per_slot,
                  "an onset template, but the decoder has no onset words", "", onset_rows, False,
                  ONSET_ROWS_MAX, ONSET_CYCLE_MAX, _ONES,
                  rows_of=lambda t: t, key=lambda t: t.tobytes(), bars=lambda t: t.shape[0],
                  word=lambda base, bars, t: onset_word(base, bars))
# (a template is (rows, cells): a bar is a block of 1 + cells rows, and the same bytes under other cells are another guide)
GUIDE = SlotRule(T_GDE, "guide", "guide", GUIDE_OFF, _guide_per_slot,
                 "a guide track, but the decoder has no guide words", "", guide_template, True,
                 GUIDE_ROWS_MAX, GUIDE_CYCLE_MAX, _ONES,
                 rows_of=lambda t: t[0], key=lambda t: (t[1], t[0].tobytes()), bars=lambda t: t[0].shape[0] // (1 + t[1]),
                 word=lambda base, bars, t: guide_word(base, bars, t[1]))
# (a template is (rows, within_bar, hold_guide): the switches live in the word, so two settings over the same rows share
# them; a free row: no bounds, every velocity bin, the reserved word 0)
ARTICULATION = SlotRule(T_ART, "art", "articulation", ARTICULATION_OFF, _articulation_per_slot,
                        "an articulation, but the decoder has no articulation words", "", articulation_template, True,
                        ARTICULATION_ROWS_MAX, ARTICULATION_CYCLE_MAX, (0, 0xFFFFFFFF, 0xFFFFFFFF, 0),
                        rows_of=lambda t: t[0], key=lambda t: t[0].tobytes(), bars=lambda t: t[0].shape[0],
                        word=lambda base, bars, t: articulation_word(base, bars, t[1], t[2]))
# (the form rule is no tier of the sampling step: it lives in the forcing stage, its switch is its own and its first use
# allocates nothing of the tiers -- the last of the table, tier -1.  A template is the uint32 rows; a free row is all zeros.)
FORM = SlotRule(-1, "form", "form", FORM_OFF, _form_per_slot, "a form, but the decoder has no form words", "",
                form_template, True, FORM_ROWS_MAX, FORM_BARS_MAX, (0, 0, 0, 0),
                rows_of=lambda t: t, key=lambda t: _form_key(t), bars=lambda t: t.shape[0],
                word=lambda base, bars, t: form_word(base, bars))
SLOT_RULES = (ORDER, VOICES, DENSITY, INTERVAL, ONSETS, GUIDE, ARTICULATION, FORM)          # (in tier order, the form last)
SAMPLING_RULES = SLOT_RULES[:-1]                                                            # (the tiers of the sampling step)
RULE_OF = {r.kw: r for r in SLOT_RULES}


def rule_closure(kws):
    """The rules that are on once the rules named kws are: themselves and, transitively, what they imply."""
    out = set()
    for kw in kws:
        while kw and kw not in out:
            out.add(kw)
            kw = RULE_OF[kw].implies
    return out


def pool_tier(kws, class_table: bool = False) -> int:
    """The tier a pool's one first use asks for: the highest any rule its requests switch on needs (a launch of a tier
    reads every word below it, so the implied rules -- all of a lower tier -- come with it), else the class tier where
    the pool has a class table, else none."""
    return max([RULE_OF[kw].tier for kw in rule_closure(kws)] + [T_CLS if class_table else T_NONE])


def _rule_values(rules: dict, default=None) -> dict:
    """The keyword arguments **rules of an entry point that takes one value per rule of SLOT_RULES, checked against the
    table and completed with the default, in the table's order."""
    extra = sorted(set(rules) - set(RULE_OF))
    if extra:
        raise TypeError(f"got an unexpected keyword argument {extra[0]!r}")
    return {r.kw: rules.get(r.kw, default) for r in SLOT_RULES}


def _rules_of(scope: dict) -> dict:
    """The rule keywords of an entry point that spells them out, picked from its locals()."""
    return {r.kw: scope[r.kw] for r in SLOT_RULES}


class ForcedDecoder:
    """The device-resident decode loop for B sequences: state records + token buffers + one hipGraph per iteration.

    load() uploads the conditioning (context tokens, chord progressions, uniform variates), run() replays the
    iteration graph until every sequence is finished, sequences() downloads the results."""

    POLL = 16          # iterations between two looks at the `done` flags (one D2H of B ints)

    # every rule of SLOT_RULES: the slots' control words int32 [B] with their host mirror and, where the rule owns one, the
    # device table of rows_max rows (allocated once, so that its pointer stays fixed under graph capture) with its host
    # mirror, the rows in use and the base row of every template packed so far, by its key.  Class-level: a decoder that
    # never enables a rule has none of them.
    for _r in SLOT_RULES:
        locals().update({_r.ctl: None, _r.host: None, _r.table: None, _r.table_host: None, _r.used: 0, _r.index: None})
    del _r
    # the form keeps two arrays more per slot: the replay state int32 [B][commu_form_state_ints()] and the replay token [B]
    form_state = None
    form_tok = None
    # ... and, from the first form that names a take on, the take buffer int32 [FORM_SRC_MAX] with its mirror and its index
    form_src = None
    _form_src_host = None
    _form_src_index: dict = {}
    _form_src_used = 0

    def __init__(self, model, B: int, generation_length: int, memory_length: int, temperature: float, top_k: int,
                 max_chords: int = 64, record_trace: bool = False, top_p: float = 1.0, sliding: bool = False,
                 max_prompt: int = 0, kv_dtype: str = "bf16", shared_prompt: bool = False):
        """kv_dtype: "bf16", or "fp8" for the opt-in e4m3 K/V cache (DecodeState).
        shared_prompt (opt-in, needs max_prompt > 0): every load() gives all slots the same conditioning tokens, chords and
        prompt; their K/V are computed and held ONCE (DecodeState(shared_prefix=)) and a slot's cache holds only what it
        generates itself: generation_length + 2 private rows.
        sliding: the reference's sliding memory window (DecodeState window mode) -- generation_length is then bounded by
        the token buffers only, not by memory_length.
        max_prompt: the longest token prefix load(prompts=) may prime a slot with (0: the loop starts from the conditioning
        context only; no buffer changes size and no launch is added).  generation_length counts the iterations AFTER the
        prompt."""
        self.model, self.B = model, B
        self.max_prompt = int(max_prompt)
        if self.max_prompt < 0:
            raise CommuHipError(f"max_prompt: a length >= 0 expected, got {max_prompt}")
        self.sliding = bool(sliding)
        self.generation_length, self.temperature, self.top_k = int(generation_length), float(temperature), int(top_k)
        self.top_p = float(top_p)          # nucleus filter after top-k (extra mode; 1.0 = the reference's behaviour)
        dev = next(model.parameters()).device
        self.dev = dev
        self.NF = call("commu_forcing_state_ints")
        self.n_ctx_max = 16
        # a sequence grows by at most one token per iteration; its cache by at most one row per iteration
        kv = {} if kv_dtype == "bf16" else {"kv_dtype": kv_dtype}          # (the default builds its state as it always did)
        self.shared_prompt = bool(shared_prompt)
        self.prefix_P = 0            # shared_prompt: the positions all slots have in common (set by load)
        if self.shared_prompt:
            if self.max_prompt < 1:
                raise CommuHipError("shared_prompt: a decoder that shares a prompt needs max_prompt > 0")
            # what a replay can produce for this max_prompt: the context and the kept tokens of the replayed stream
            pcap = self.n_ctx_max + (self.n_ctx_max + 2 * self.max_prompt)
            lp = self.generation_length + 2
            self._mem_rows = min(int(memory_length) + 1, DecodeState.MAX_POSITIONS)      # shared + private positions
            # (window / fp8 / parity are refused by the state, before it allocates, with the reason)
            self.state = DecodeState(model, B, lp, window=int(memory_length) if self.sliding else None, shared_prefix=pcap,
                                     **kv)
        elif self.sliding:
            M = int(memory_length)
            if M + 1 > DecodeState.MAX_POSITIONS:
                raise CommuHipError(f"a sliding memory of {M} positions needs {M + 1} cache rows; this build supports "
                                    f"{DecodeState.MAX_POSITIONS}")
            if M < self.n_ctx_max:
                raise CommuHipError(f"a sliding memory of {M} positions cannot hold the conditioning context (up to "
                                    f"{self.n_ctx_max} tokens)")
            self.state = DecodeState(model, B, M + 1, window=M, **kv)
        else:
            lmax = min(int(memory_length) + 1, DecodeState.MAX_POSITIONS)
            if self.n_ctx_max + self.generation_length + 1 > lmax:
                raise CommuHipError(
                    f"context + generation_length ({self.generation_length}) exceeds the decode memory of {lmax} positions; "
                    "the reference would start sliding its memory window here, which the K/V-cache step does not implement "
                    "unless it is asked to (sliding=True, --sliding_memory)")
            self.state = DecodeState(model, B, lmax, **kv)
        self._ctx_kv = None          # sliding: the context rows of every slot's K/V cache as load() left them (rearm)
        self.ld_seq = self.n_ctx_max + self.generation_length + 2 + self.max_prompt
        self.ld_chord = max_chords
        self.ld_u = self.generation_length + 1
        i32, u8 = torch.int32, torch.uint8
        self.fsm = torch.zeros(B, self.NF, dtype=i32, device=dev)
        self.seq = torch.zeros(B, self.ld_seq, dtype=i32, device=dev)
        self.chord_tok = torch.zeros(B, max_chords, dtype=i32, device=dev)
        self.chord_pos = torch.zeros(B, max_chords, dtype=i32, device=dev)
        self.wrong = torch.zeros(B, TOKEN_OFFSET.VOCAB_SIZE, dtype=u8, device=dev)
        self.utable = torch.full((B, self.ld_u), 0.5, dtype=F32, device=dev)
        self.tok = torch.zeros(B, dtype=torch.long, device=dev)
        self.active = torch.zeros(B, dtype=u8, device=dev)
        self.keep = torch.zeros(B, dtype=u8, device=dev)
        self.draw = torch.zeros(B, dtype=u8, device=dev)
        self.uni = torch.zeros(B, dtype=F32, device=dev)
        self.token = torch.zeros(B, dtype=i32, device=dev)
        # The sampling controls are per-slot device state the kernels read (a captured graph follows them: set_sampling
        # rewrites them in place); the constructor's triple is every slot's initial value.  TWO MODES: while every slot has
        # the same triple, that triple is what the captured launches hold, and no log-probabilities were asked for, the
        # launches get the scalars and null arrays (the measured cost of the arrays: docs/EXPERIMENTS.md 8i).  Slots that
        # differ, a new triple for launches already captured (a graph holds its scalars), or record_logprobs() switch the
        # decoder to the arrays for good: the captured graphs are dropped once, and from then on settings change in place.
        self.rows_on = False
        self._sampling = sampling_rows(B, self.temperature, self.top_k, self.top_p)          # host mirror
        self.temperature, self.top_p = float(self._sampling[0][0]), float(self._sampling[2][0])      # (as fp32 holds them)
        self.temperature_rows = torch.from_numpy(self._sampling[0]).to(dev)
        self.top_k_rows = torch.from_numpy(self._sampling[1]).to(dev)
        self.top_p_rows = torch.from_numpy(self._sampling[2]).to(dev)
        # log-probability pairs (full, kept) of the tokens in seq, NaN where a token was not drawn (context, forced), and
        # the pair of the current draw beside `token` (the hand-over of the separate launches)
        self.seq_logp = torch.full((B, self.ld_seq, 2), float("nan"), dtype=F32, device=dev)
        self.logp = torch.full((B, 2), float("nan"), dtype=F32, device=dev)
        self.probs = None
        # constraint rows (set_logit_bias): fp32 [B][VPAD], allocated by the first constraint; None: the launches get a null
        # pointer and are the ones a decoder without constraints always made
        self.bias = None
        # event grammar (set_grammar): the table fp32 [8][VPAD] and the slots' switches [B], allocated by the first grammar;
        # None: null pointers, the launches a decoder without a grammar always made
        self.gram = None
        self.gram_on = None
        self._gram_host = None          # host mirror of the table (a re-arm that changes nothing uploads nothing)
        # harmony (set_harmony): the table fp32 [111][16] and the slots' switches [B], allocated by the first table; None:
        # the launches a decoder without harmony always made
        self.harm = None
        self.harm_on = None
        self._harm_host = None
        # class-keyed sampling (set_class_sampling): the slots' control records int32 [B][8][4] (the bit patterns of
        # CLASS_CTL_DTYPE), allocated by the first table, and the host's NaN-tables float64 [B][8][3] they are composed
        # from; None: the launches a decoder without class controls always made
        self.cls_ctl = None
        self._cls_host = None
        # (the words and tables of SLOT_RULES: class-level None until the first call that switches a slot on)
        # (the replay of a prompt token takes at most two iterations: the decision to force it, then its append)
        self.ld_trace = 2 * (self.generation_length + 2 + 2 * self.max_prompt) if record_trace else 0
        self.trace = torch.zeros(B, self.ld_trace, dtype=i32, device=dev) if record_trace else None
        self.graph = None
        self.graph_long = None
        self.n_cond = 0
        # primed generation (load(prompts=)): the prompts, what the replay would have fed the model (kept steps only) and
        # where a prompt leaves the rules; the primed records / lengths / trace as load() left them (rearm)
        self.ld_fed = self.n_ctx_max + 2 * self.max_prompt
        self.klen0 = 0               # the longest memory any slot starts with
        self._primed = None
        if self.max_prompt > 0:
            self.prompt = torch.zeros(B, self.max_prompt, dtype=i32, device=dev)
            self.prompt_len = torch.zeros(B, dtype=i32, device=dev)
            self.fed = torch.zeros(B, self.ld_fed, dtype=i32, device=dev)
            self.diverged = torch.full((B, 2), -1, dtype=i32, device=dev)

    # ---- one loop iteration = decide (pre) -> model step -> sampling step -> book-keeping (post), as kernel launches
    # on the current stream.  The captured graph holds [step, {sample, post, pre of the NEXT iteration} as one launch]
    # (body_pre): run() issues the very first `pre` on its own and the kernel sequence is the same captured or not.
    # pre() / body() are the separate launches (iteration(): tests look at the draws between the stages).
    def _slots(self, rows):
        """The slot numbers a setter addresses (rows=None: all of them), validated."""
        idx = np.arange(self.B) if rows is None else np.asarray(list(rows), dtype=np.int64)
        if idx.ndim != 1 or (idx.size and (idx.min() < 0 or idx.max() >= self.B)):
            raise CommuHipError(f"rows: slot numbers in [0, {self.B}) expected, got {rows!r}")
        return idx

    def _first_use(self, tier=T_NONE, rows=False, bias=False, gram=False):
        """What the first use of a per-slot launch input does, for each one asked for that the decoder does not have yet.
        tier: everything the launch of that tier reads (T_* above) -- from T_HARM up the bias and the grammar, from T_CLS up
        the array launches; below T_HARM the three are independent of each other and asked for by name.  rows uploads the
        host mirror of the sampling controls (scalar mode kept the mirror only); bias / gram / harmony allocate their
        zeroed device buffers (gram and harmony: the table and the [B] switches); the class tier allocates the slots'
        class-control records (set_class_sampling fills them); every rule of SAMPLING_RULES its words, all off, and -- where it
        owns one -- its table of rows that constrain nothing.  When anything was missing the captured graphs are dropped,
        once: they hold the launches without it."""
        new = False
        rows, bias, gram = rows or tier >= T_CLS, bias or tier >= T_HARM, gram or tier >= T_HARM
        if rows and not self.rows_on:
            new = self.rows_on = True
            for dst, src in zip((self.temperature_rows, self.top_k_rows, self.top_p_rows), self._sampling):
                dst.copy_(torch.from_numpy(src))
        if bias and self.bias is None:
            new = True
            self.bias = torch.zeros(self.B, VPAD, dtype=F32, device=self.dev)
        if gram and self.gram is None:
            new = True
            self.gram = torch.zeros(N_CLASSES + 1, VPAD, dtype=F32, device=self.dev)
            self.gram_on = torch.zeros(self.B, dtype=torch.uint8, device=self.dev)
        if tier >= T_HARM and self.harm is None:
            new = True
            self.harm = torch.zeros(HARM_ROWS, HARM_COLS, dtype=F32, device=self.dev)
            self.harm_on = torch.zeros(self.B, dtype=torch.uint8, device=self.dev)
        if tier >= T_CLS and self.cls_ctl is None:
            new = True
            self.cls_ctl = torch.zeros(self.B, N_CLASSES + 1, 4, dtype=torch.int32, device=self.dev)
            self._cls_host = np.full((self.B, N_CLASSES + 1, 3), np.nan)
        for r in SAMPLING_RULES:
            if tier >= r.tier:
                new = self._alloc_rule(r) or new
        if new:
            self.graph = self.graph_long = None

    def _alloc_rule(self, r) -> bool:
        """Rule r's words, all off, with their mirror and -- where it owns one -- its table of rows that constrain nothing,
        unless the decoder has them; returns whether it had not."""
        if getattr(self, r.ctl) is not None:
            return False
        setattr(self, r.ctl, torch.full((self.B,), r.off, dtype=torch.int32, device=self.dev))
        setattr(self, r.host, np.full(self.B, r.off, dtype=np.int32))
        if r.rows_max:
            host = np.tile(np.array(r.fill, dtype=np.uint32), (r.rows_max, 1))
            setattr(self, r.table_host, host)
            # (int32 on the device: the bit patterns of the uint32 rows)
            setattr(self, r.table, torch.from_numpy(host.view(np.int32).copy()).to(self.dev))
            setattr(self, r.used, 0)
            setattr(self, r.index, {})
        return True

    def _first_use_words(self, r):
        """_first_use of a word setter: what rule r's kernel reads; class records that no table ever filled hold every
        slot's base triple in every record.  The form has a first use of its own."""
        if r is FORM:
            return self._first_use_form()
        fresh_cls = self.cls_ctl is None
        self._first_use(r.tier)
        if fresh_cls:
            self._write_class_ctl(None, np.arange(self.B))

    def _write_words(self, r, idx, new, rows):
        """The tail of a word setter: the words `new` of the slots idx, where they differ from the mirror, written in
        place -- the whole array by one copy, or a few slots by device-side fills."""
        host, ctl = getattr(self, r.host), getattr(self, r.ctl)
        if np.array_equal(host[idx], new):
            return
        host[idx] = new
        if rows is None and len(idx) > 4:
            ctl.copy_(torch.from_numpy(host))
        else:
            for j in idx:
                ctl[int(j)].fill_(int(host[j]))

    def _pack(self, r, templates, fresh: bool = False, label: str = ""):
        """The control words of the given templates (None: off) in the table of rule r.  Distinct templates, told apart by
        r.key, are packed one behind the other; a template packed before keeps its rows.  fresh: the table is packed anew
        from these templates alone (every slot's word is about to be rewritten).  Refuses, before anything changes, what
        does not fit.  New rows are written to the device table in place, ordered on the current stream."""
        index = {} if fresh else dict(getattr(self, r.index))
        used = 0 if fresh else getattr(self, r.used)
        todo, words = [], []
        # (the form's takes: each distinct take is placed once in the take buffer, and the rows that read it are rebased to
        # its place; a fresh pack reclaims the takes of forms no longer referenced)
        place = self._form_src_plan(templates, fresh, label) if r is FORM else None
        for t in templates:
            if t is None:
                words.append(r.off)
                continue
            rows, bars = r.rows_of(t), r.bars(t)
            if bars > r.cycle_max:
                raise CommuHipError(f"{r.kw}: a template holds at most {r.cycle_max} bars, got {bars}")
            key = r.key(t)
            if key not in index:
                if used + rows.shape[0] > r.rows_max:
                    raise CommuHipError(f"{r.kw}: the distinct templates need more than the table's {r.rows_max} rows "
                                        f"({used} in use, {rows.shape[0]} more asked for)")
                if place is not None and getattr(t, "takes", ()):
                    rows = np.array(rows, dtype=np.uint32)
                    for i, k in enumerate(t.take_of):
                        if k >= 0:
                            rows[i, 1:3] += np.uint32(place[0][t.takes[k].tobytes()])
                index[key] = used
                todo.append((used, rows))
                used += rows.shape[0]
            words.append(r.word(index[key], bars, t))
        if place is not None:
            self._form_src_write(*place)
        host, table = getattr(self, r.table_host), getattr(self, r.table)
        for base, rows in todo:
            host[base:base + rows.shape[0]] = rows
            table[base:base + rows.shape[0]].copy_(torch.from_numpy(rows.view(np.int32)))
        setattr(self, r.index, index)
        setattr(self, r.used, used)
        return np.array(words, dtype=np.int32)

    def _set_words(self, r, value, rows):
        """The body of a word setter: the values validated before anything changes; nothing for a decoder without the
        rule that switches no slot on; the rule r implies switched on (word 0) where a slot that is switched on has it off
        -- through its setter, which allocates what its kernel reads --; first use; words."""
        idx = self._slots(rows)
        new = r.normalize(value, len(idx))
        if getattr(self, r.ctl) is None and not bool((new != r.off).any()):
            return
        if r.implies:
            dep = RULE_OF[r.implies]
            host = getattr(self, dep.host)
            need = [int(j) for j, w in zip(idx, new) if w != r.off and (host is None or host[j] == dep.off)]
            if need:
                getattr(self, dep.setter)(0, rows=need)
        self._first_use_words(r)
        self._write_words(r, idx, new, rows)

    def _set_templates(self, r, value, rows):
        """The body of a template setter: the values validated before anything changes; nothing for a decoder without the
        rule that is given no template; the capacity check of _pack before anything is allocated; first use; pack; words."""
        idx = self._slots(rows)
        tmpl = r.normalize(value, len(idx))
        if getattr(self, r.ctl) is None:
            if all(t is None for t in tmpl):
                return
            need = sum(r.rows_of(t).shape[0] for t in {r.key(t): t for t in tmpl if t is not None}.values())
            if need > r.rows_max:
                raise CommuHipError(f"{r.kw}: the distinct templates need more than the table's {r.rows_max} rows "
                                    f"(0 in use, {need} asked for)")
            if r is FORM:
                self._form_src_plan(tmpl, True)          # (the takes' capacity too, before the first use allocates)
        self._first_use_words(r)
        self._write_words(r, idx, self._pack(r, tmpl, fresh=rows is None), rows)

    @staticmethod
    def _switch(on, val, rows, idx):
        """The [B] switches `on` of the addressed slots (rows=None: all) set to val, in place."""
        if rows is None:
            on.fill_(val)
        else:
            for j in idx:
                on[int(j)].fill_(val)

    def record_logprobs(self):
        """Keep the log-probability pair of every token from now on (logprobs(), harvest_logprobs()).  Call it before
        load(): tokens appended earlier have no entry.  Switches the decoder to the array launches (see __init__)."""
        self._first_use(rows=True)

    def _rows_args(self):
        """(temperature_rows, top_k_rows, top_p_rows, logp, seq_logp) as the launches get them."""
        if not self.rows_on:
            return None, None, None, None, None
        return self.temperature_rows, self.top_k_rows, self.top_p_rows, self.logp, self.seq_logp

    def set_sampling(self, temperature=None, top_k=None, top_p=None, rows: Optional[Sequence[int]] = None):
        """New sampling controls for all slots (rows=None) or the listed ones: each of temperature / top_k / top_p is None
        (unchanged), a number, or one value per addressed slot.  With the array launches (see __init__) the device arrays
        are rewritten IN PLACE, ordered on the current stream like any launch: a captured graph keeps pointing at them and
        needs no re-capture.  A few slots (rearm) are written by device-side fills -- no host copy, no synchronisation --,
        a whole batch by one copy per array that changed."""
        idx = self._slots(rows)
        cur = self._sampling
        new = sampling_rows(len(idx), *(cur[i][idx] if v is None else v for i, v in enumerate((temperature, top_k, top_p))))
        changed = [not np.array_equal(cur[i][idx], new[i]) for i in range(3)]
        for i in range(3):
            cur[i][idx] = new[i]
        if not self.rows_on:
            if any(bool((c != c[0]).any()) for c in cur):
                return self._first_use(rows=True)       # slots differ (uploads the mirror)
            triple = (float(cur[0][0]), int(cur[1][0]), float(cur[2][0]))
            if triple == (self.temperature, self.top_k, self.top_p):
                return
            if self.graph is not None or self.graph_long is not None:
                return self._first_use(rows=True)       # the captured launches hold the old scalars
            self.temperature, self.top_k, self.top_p = triple
            return
        for i, dst in enumerate((self.temperature_rows, self.top_k_rows, self.top_p_rows)):
            if not changed[i]:
                continue
            if len(idx) <= 4:
                for j in idx:
                    dst[int(j)].fill_(cur[i][j].item())
            elif bool((cur[i] == cur[i][0]).all()):
                dst.fill_(cur[i][0].item())
            else:
                dst.copy_(torch.from_numpy(cur[i]))
        if self.cls_ctl is not None and any(changed):          # (the inherited entries and row 7 follow the base triple)
            self._write_class_ctl(rows, idx)

    def set_logit_bias(self, bias, rows: Optional[Sequence[int]] = None):
        """Constraint rows (token_constraints) for all slots (rows=None) or the listed ones: None (clear), one row for all
        of them, or one row per addressed slot.  The sampling step adds slot b's row to the row its softmax sees, before
        top-k: a finite entry re-weights an id, -inf bans it.  Only DRAWS are constrained: forced tokens (bars, positions,
        chords) are placed by the rules whatever the row says, and a prompt (load(prompts=)) is not checked against it.
        The first constraint allocates the zeroed [B][768] device buffer and drops the captured graphs once (they hold the
        launch without it), the way the per-slot sampling controls do; from then on rows are rewritten IN PLACE, ordered on
        the current stream like any launch, and a captured graph follows them.  A cleared row is zeros: x + 0 is x, so the
        slot draws bit for bit what it draws without a constraint.  A decoder that never got one allocates nothing."""
        idx = self._slots(rows)
        new = None if bias is None else logit_bias_rows(bias, len(idx))          # (validated before anything changes)
        if self.bias is None and new is None:
            return
        self._first_use(bias=True)
        if new is None:
            if rows is None:
                self.bias.zero_()
            else:
                for j in idx:
                    self.bias[int(j)].zero_()
        elif rows is None:
            self.bias.copy_(torch.from_numpy(new))
        else:
            for j, r in zip(idx, new):
                self.bias[int(j)].copy_(torch.from_numpy(r))

    def set_grammar(self, table=True, rows: Optional[Sequence[int]] = None):
        """The event grammar for all slots (rows=None) or the listed ones: True (event_grammar(), the default table), a
        table (grammar_table) or None (off).  A slot that is on draws from (x + bias) + table[c], c the class of the last
        token in its seq when the sampling stage runs -- the last prompt token for the first draw of a primed slot --, so
        every token it draws continues a group of midi_inferrer.parse_events.  Only DRAWS are constrained: forced tokens
        are placed by the rules and a prompt is not checked.  The decoder holds ONE table; a table given here replaces it
        for every slot that is on.  The first grammar allocates the table and the [B] switches and drops the captured
        graphs once (they hold the launch without them), exactly as set_logit_bias does; later calls rewrite in place,
        ordered on the current stream.  A slot that is off reads the zero row 7: it draws bit for bit what it drew
        without the feature.  A decoder that never got a grammar allocates nothing."""
        idx = self._slots(rows)
        if table is False:
            table = None
        new = None if table is None else (event_grammar() if table is True else grammar_table(table))
        if self.gram is None and new is None:
            return
        self._first_use(gram=True)
        if new is not None and (self._gram_host is None or not np.array_equal(new, self._gram_host)):
            self.gram.copy_(torch.from_numpy(new))
            self._gram_host = new
        self._switch(self.gram_on, 0 if new is None else 1, rows, idx)

    def _gram_args(self):
        return None if self.gram is None else (self.gram, self.gram_on, self.fsm, self.seq)

    def set_harmony(self, table=True, rows: Optional[Sequence[int]] = None):
        """The harmony constraint for all slots (rows=None) or the listed ones: True (harmony_table(), strict: only chord
        tones), a table (harmony_rows) or None / False (off).  A slot that is on draws its pitches (ids 3 .. 130, MIDI
        pitch id - 3) from ((x + bias) + grammar row) + table[r][(id - 3) mod 12], r the row of the last chord token in
        its seq when the sampling stage runs (109 while there is none) -- the last chord of the prompt for the first draw
        of a primed slot; no other id is touched.  Only DRAWS are constrained: forced tokens are placed by the rules and a
        prompt is not checked.  The decoder holds ONE table; a table given here replaces it for every slot that is on.
        The first table allocates it and the [B] switches -- and a zero bias buffer and an all-off grammar where the decoder
        has none: the one harmony kernel reads both, and x + 0 and the zero row 7 change no bit -- and drops the captured
        graphs once, exactly as set_grammar does; later calls rewrite in place, ordered on the current stream.  A slot
        that is off reads the zero row 110: it draws bit for bit what it drew without the feature.  A decoder that never
        got a table allocates nothing.  Not enforced: a logit_bias (or a pitch range built from one) that leaves no pitch
        of an allowed class makes the slot fail its draw after a velocity (Q12) when the grammar is on as well."""
        idx = self._slots(rows)
        if table is False:
            table = None
        new = None if table is None else (harmony_table() if table is True else harmony_rows(table))
        if self.harm is None and new is None:
            return
        self._first_use(T_HARM)                               # (the one harmony kernel reads a bias and a grammar)
        if new is not None and (self._harm_host is None or not np.array_equal(new, self._harm_host)):
            self.harm.copy_(torch.from_numpy(new))
            self._harm_host = new
        self._switch(self.harm_on, 0 if new is None else 1, rows, idx)

    def _harm_args(self):
        return None if self.harm is None else (self.harm, self.harm_on, self.fsm, self.chord_tok)

    def set_class_sampling(self, table=None, rows: Optional[Sequence[int]] = None):
        """Class-keyed sampling controls for all slots (rows=None) or the listed ones: a table float64 [8][3]
        (class_sampling(), NaN: inherit) or None (no override).  A slot with a table draws with the triple of record
        c = token_class(previous token) -- the last token of its seq when the sampling stage runs, the grammar's key; the
        last prompt token for the first draw of a primed slot -- and every entry the table leaves NaN is the slot's base
        value (set_sampling, rearm(sampling=)); forced tokens and prompts are not draws.  Under the default event grammar
        the previous token's class fixes what is drawn next (class_sampling(drawn=)); without it the key is still the
        previous token's class.  The first table allocates the slots' records -- and what the one kernel reads besides: the
        array launches (record_logprobs), a zero bias, an all-off grammar and an all-off harmony table -- and drops the
        captured graphs once; later calls rewrite the records IN PLACE, ordered on the current stream, and a captured graph
        follows them.  None writes the slot's base triple into all 8 records: bit for bit what the array launches decode
        without the feature.  set_sampling() and rearm(sampling=) recompose the inherited entries of the slots they touch
        (the NaN-tables stay on the host).  A decoder that never got a table allocates nothing."""
        idx = self._slots(rows)
        new = None if table is None else class_sampling_table(table)          # (validated before anything changes)
        if self.cls_ctl is None and new is None:
            return
        fresh = self.cls_ctl is None
        self._first_use(T_CLS)
        self._cls_host[idx] = np.nan if new is None else new
        if fresh:          # (the slots not addressed get their base triple in every record)
            rows, idx = None, np.arange(self.B)
        self._write_class_ctl(rows, idx)

    def _write_class_ctl(self, rows, idx):
        """The records of the addressed slots composed from their NaN-tables and base triples, written in place."""
        rec = class_ctl_records(self._cls_host[idx], [c[idx] for c in self._sampling])
        words = torch.from_numpy(rec.view(np.int32).reshape(len(idx), N_CLASSES + 1, 4))
        if rows is None:
            self.cls_ctl.copy_(words)
        else:
            for j, w in zip(idx, words):
                self.cls_ctl[int(j)].copy_(w)

    def class_samples(self):
        """Whether a class record of any slot holds a temperature other than 0 (such a draw reads a variate)."""
        return self._cls_host is not None and bool((np.nan_to_num(self._cls_host[..., 0], nan=0.0) != 0).any())

    def _cls_args(self):
        return None if self.cls_ctl is None else (self.cls_ctl, self.fsm, self.seq)

    def _slot_words(self):
        """(rule, control words) for every rule of SAMPLING_RULES the decoder has words for."""
        return [(r, getattr(self, r.ctl)) for r in SAMPLING_RULES if getattr(self, r.ctl) is not None]

    def set_note_order(self, value=True, rows: Optional[Sequence[int]] = None):
        """The note-order constraint for all slots (rows=None) or the listed ones: True (on), an integer n in 1 .. 128 (on,
        at most n notes per position), None / False (off), or one such value per addressed slot (note_order_ctl).  A slot
        that is on cannot DRAW a position token before the position its bar is at, a pitch that position already holds,
        or -- with a cap -- the position itself once it holds n notes: inside a bar the drawn positions never go back and
        no note is doubled; n = 1 gives one note per onset.  The state is read off the slot's seq when the sampling stage
        runs (the prompt of a primed slot included), so a re-draw and a re-armed slot need nothing else.  Only DRAWS are
        constrained: forced tokens are placed by the rules and a prompt is not checked.  The first call that switches a
        slot on allocates the [B] control words -- and what the one kernel reads besides: the array launches, a zero bias,
        an all-off grammar, an all-off harmony table and the class records holding every slot's base triple -- and drops
        the captured graphs once; later calls rewrite the words IN PLACE, ordered on the current stream, and a captured
        graph follows them.  A slot that is off bans nothing: it decodes bit for bit what it decoded without the feature.
        A decoder that never switched a slot on allocates nothing.  Overlapping durations are not this rule's (a cap of 1 is
        one note per onset, not strict monophony): set_voices bans them.  A bias, pitch range or strict harmony that
        leaves fewer pitches than notes asked for at one position ends the slot by Q12."""
        self._set_words(ORDER, value, rows)

    def set_voices(self, value, rows: Optional[Sequence[int]] = None):
        """The voice cap for all slots (rows=None) or the listed ones: a word voices_word(N, r) -- at most N of the slot's
        notes sound at once (N = 0: no cap; N = 1: a monophonic line) and, with r, no pitch is struck while it sounds --
        None / False (off), or one such value per addressed slot (voices_ctl).  A note is a Position, Velocity, Pitch,
        Duration group of the slot's seq, as the token-to-MIDI step reads it; a slot that is on cannot DRAW a position at
        which N notes of the current or the previous bar still sound, nor a pitch that still sounds at the onset the bar is
        at.  The rule relies on the note order (every known note then starts at or before any onset that can still be
        drawn): a slot switched on here whose note order is off gets it switched on (word 0, no cap per position), and
        switching the voices off leaves the note order as it is.  The state is read off seq when the sampling stage runs
        (the prompt of a primed slot included).  Only DRAWS are constrained: notes inside a prompt are not checked against
        each other and a forced token is placed by the rules.  The first call that switches a slot on allocates the [B]
        words and drops the captured graphs once; later calls rewrite the words IN PLACE, ordered on the current stream,
        and a captured graph follows them.  A slot that is off bans nothing.  A decoder that never switched a slot on
        allocates nothing.  When a whole bar's rest is banned only Bar and EOS remain of the boundary family; a pitch range,
        bias or strict harmony that leaves no pitch free ends the slot by Q12."""
        self._set_words(VOICES, value, rows)

    def set_density(self, value, rows: Optional[Sequence[int]] = None):
        """The note density for all slots (rows=None) or the listed ones: a word density_word(lo, hi) -- a bar the slot
        DRAWS holds at least lo and at most hi notes (0: that bound is not set) -- None / False (off), or one such value
        per addressed slot (density_ctl).  A note is a Position, Velocity, Pitch, Duration group of the slot's seq; the bar
        being written is what follows the last Bar.  While it holds fewer than lo notes the slot cannot DRAW Bar or EOS --
        unless the note order, the voice cap and the upper bound together leave no position to draw, in which case the bar
        may end short -- and once it holds hi notes the slot cannot draw a position: only Bar and EOS remain of the
        boundary family.  The count rides on the voice cap's walk over seq: a slot switched on here whose voice word is off
        gets word 0 (no cap, re-striking allowed), and its note order is switched on where it was off (set_voices); switching
        the density off leaves both as they are.  The state is read off seq when the sampling stage runs (the prompt of a
        primed slot included: its notes count, and are never removed).  Only DRAWS are constrained: a forced Bar or EOS may
        close a short bar, a note that starts on a forced position counts but is not prevented, and a bar that the
        generation length cuts stays as it is.  The first call that switches a slot on allocates the [B] words and drops
        the captured graphs once; later calls rewrite the words IN PLACE, ordered on the current stream, and a captured
        graph follows them.  A slot that is off bans nothing.  A decoder that never switched a slot on allocates nothing."""
        self._set_words(DENSITY, value, rows)

    def set_interval(self, value, rows: Optional[Sequence[int]] = None):
        """The melodic interval for all slots (rows=None) or the listed ones: a word interval_word(up, down, no_repeat) --
        the pitch the slot DRAWS lies at most up semitones above and at most down below the pitch of its last note (0: that
        bound is not set) and, with no_repeat, is not that pitch -- None / False (off), or one such value per addressed slot
        (interval_ctl).  A note is a Position, Velocity, Pitch, Duration group of the slot's seq; the last note is the one
        furthest back in seq that at most one Bar follows, so the first note of a sequence, and the first after a whole
        bar's rest, is free.  The state is read off seq when the sampling stage runs (the prompt of a primed slot included:
        its last note is the reference of the first draw, its notes are not checked against each other).  Only DRAWS are
        constrained.  The word implies none of the others: the first call that switches a slot on allocates the [B] words
        and, where the decoder lacks them, everything the one kernel reads besides -- the density, voice and note-order words
        (all off), the array launches, a zero bias, an all-off grammar, an all-off harmony table and the class records
        holding every slot's base triple -- and drops the captured graphs once; later calls rewrite the words IN PLACE,
        ordered on the current stream, and a captured graph follows them.  A slot that is off bans nothing: it decodes bit
        for bit what it decoded without the feature.  A decoder that never switched a slot on allocates nothing.  Several
        notes at one position are compared in token order (the rule is meant for set_voices lines of one voice); a pitch
        range, bias, strict harmony, note-order or re-strike ban that leaves no pitch inside the window ends the slot by
        Q12."""
        self._set_words(INTERVAL, value, rows)

    def set_onsets(self, value, rows: Optional[Sequence[int]] = None):
        """The onset template for all slots (rows=None) or the listed ones: a template in any form onset_rows takes -- a list
        of bars, each a list of the positions 0 .. 127 at which a note may START, {"grid": n}, {"bars": [...]}, a uint32
        [R][4] array -- None / False (off), or one such value per addressed slot.  A slot that is on DRAWS a position only
        where the row of the bar being written has a bit; bar i of the sequence (its Bar tokens counted from the start,
        the prompt's included, the stretch before the first Bar being bar 0) uses row i mod R of its template, so a primed
        slot continues the cycle in phase.  An all-clear row is a bar of rest.  The kernel takes the bar count from the
        slot's forcing record.  Only DRAWS are constrained: the position 0 forced after a Bar, a chord's forced position
        and a prompt are not.  With set_density's lower bound a bar may end short once the template leaves it no onset.
        The rule implies none of the others: the first call that switches a slot on allocates the [B] words, the table of
        4096 rows -- ONCE, so that its address stays fixed under graph capture -- and, where the decoder lacks them,
        everything the one kernel reads besides (the interval, density, voice and note-order words, all off, and what
        set_interval allocates), and drops the captured graphs once; later calls pack new templates behind the ones in the
        table (the same template, by its bytes, is stored once) and rewrite words and rows IN PLACE, ordered on the current
        stream, and a captured graph follows them.  A call for all slots packs the table anew.  Refused with the numbers:
        a template of more than 64 bars, distinct templates of more than 4096 rows together.  A slot that is off decodes
        bit for bit what it decoded without the feature; a decoder that never switched a slot on allocates nothing."""
        self._set_templates(ONSETS, value, rows)

    def set_guide(self, value, rows: Optional[Sequence[int]] = None):
        """The guide track for all slots (rows=None) or the listed ones: a guide in any form guide_template takes -- the raw
        form {"cells": C, "bars": [...]}, the derived form {"from_tokens": [ids], ...}, a pair (uint32 rows, C) -- None /
        False (off), or a list with one such value per addressed slot.  A slot that is on DRAWS a pitch only where the cell
        row of the position its bar is at has a bit, and a position only where the bar's live row has one; bar i of the
        sequence (counted as set_onsets counts it, the prompt's bars included) uses block i mod R.  Only a note's START is
        tested: a drawn note held across a later change of the guide is not checked; nor are forced tokens (the position 0
        after a Bar, a chord's position) or a prompt; a pitch range, strict harmony or interval window that together with
        the cell row leaves no pitch ends the attempt by Q12 as before.
        Exactly like set_onsets: the first call that switches a slot on allocates the [B] words, the table of 65536 rows
        (1 MB) -- ONCE, so that its address stays fixed under graph capture -- and, where the decoder lacks them, the
        off-words of everything the one kernel reads besides (set_onsets' words and table included), and drops the
        captured graphs once; later calls pack new templates behind the ones in the table and rewrite words and rows IN
        PLACE, ordered on the current stream.  A call for all slots packs the table anew.  Refused with the numbers: a
        template of more than 64 bars, distinct templates of more than 65536 rows together.  A slot that is off decodes
        bit for bit what it decoded without the feature; a decoder that never switched a slot on allocates nothing."""
        self._set_templates(GUIDE, value, rows)

    def set_articulation(self, value, rows: Optional[Sequence[int]] = None):
        """The articulation for all slots (rows=None) or the listed ones: an articulation in any form articulation_template
        takes -- the full form {"bars": [...], "within_bar": bool, "hold_guide": bool}, the short form {"duration": [lo, hi],
        "velocity": [lo, hi], ...}, a triple (uint32 rows, within_bar, hold_guide) -- None / False (off), or a list with one
        such value per addressed slot.  A slot that is on DRAWS a velocity only where the row of its open bar has a bit and
        a duration only inside the row's window, capped at the bar line (within_bar) and at the first step where the slot's
        guide (set_guide) bans the pitch just drawn (hold_guide; with the slot's guide off the term does not apply); bar i
        of the sequence (counted as set_onsets counts it, the prompt's bars included) uses row i mod R.  Where the bar line
        or the guide leaves less room than the lower bound, the lower bound gives way.  Not covered: forced tokens and
        anything a forced position starts; a prompt; the hold term reads the guide only, and reads the next bar's block
        even where the generation length would cut the sequence first.
        Exactly like set_guide: the first call that switches a slot on allocates the [B] words, the table of 4096 rows
        (64 KB) -- ONCE, so that its address stays fixed under graph capture -- and, where the decoder lacks them, the
        off-words of everything the one kernel reads besides (set_guide's words and table included), and drops the
        captured graphs once; later calls pack new templates behind the ones in the table and rewrite words and rows IN
        PLACE, ordered on the current stream.  A call for all slots packs the table anew.  Refused with the numbers: a
        template of more than 64 bars, distinct templates of more than 4096 rows together.  A slot that is off decodes
        bit for bit what it decoded without the feature; a decoder that never switched a slot on allocates nothing."""
        self._set_templates(ARTICULATION, value, rows)

    def set_form(self, value, rows: Optional[Sequence[int]] = None):
        """The form for all slots (rows=None) or the listed ones: a form in any form form_template takes -- a letter string
        "AABA", {"bars": [null | j | {"of": j, "copy": "all" | "rhythm", "transpose": s}, ...]}, uint32 rows -- None / False
        (off), or a list with one such value per addressed slot.  A bar that the loop of a slot that is on OPENS ITSELF and
        whose row names an earlier bar REPLAYS that bar's note groups (Position, Velocity, Pitch, Duration) through the
        forcing stage: the tokens are handed to the book-keeping as if drawn, so every forcing rule applies to them -- the
        bar gets the chords of its own place in the progression --, no variate is consumed, and their log-probability pairs
        are NaN.  "rhythm": the pitches are drawn, under every constraint the slot has (the slot's grammar must be on: the
        generator refuses the request otherwise).  A prompt's bars are valid sources; the bar a prompt leaves open is free.
        A form is not cycled: bars past its end (and past the 64th) are free.  Not covered: replayed tokens are not checked
        against any constraint (forced tokens are not either); a replay bar cut by the generation length is not completed; a
        source note the bar line cut does not appear; chord tokens are never copied.
        Like set_articulation: the first call that switches a slot on allocates the [B] words, the table of 4096 rows
        (64 KB) -- ONCE, so that its address stays fixed under graph capture --, the slots' replay state and replay tokens,
        and drops the captured graphs once (the loop launches the form kernels from then on); it allocates nothing of the
        sampling tiers.  Later calls pack new forms behind the ones in the table and rewrite words and rows IN PLACE, ordered
        on the current stream: no re-capture.  A word takes effect at the next Bar the slot appends; load() and rearm()
        reset the slot's replay state.  A call for all slots packs the table anew.  A slot that is off decodes bit for bit
        what it decoded without the feature; a decoder that never switched a slot on allocates nothing and launches the
        kernels it always launched.
        TAKES: a form may name bars of finished sequences of the user's ({"takes": ..., "bars": [... {"take": t, "of": j}]}
        or {"keep": ..., "redo": [...], "repitch": [...]}, form_template): such a bar -- any bar, bar 0 included -- replays
        the take's bar exactly as an own-past row replays its source.  The first form with a take allocates the take buffer
        (FORM_SRC_MAX ints, once, at a fixed address) and drops the graphs once more; each distinct take is placed once,
        de-duplicated by bytes, its rows rebased to its place; a call for all slots reclaims the takes no form names any
        more; what does not fit is refused before anything changes, with the tokens needed against the capacity.
        Unlike a word, which takes effect at the slot's next Bar, a reclaim takes effect AT ONCE: a call for all slots
        rewrites the buffer from its start, and a slot that is inside a take's replay bar at that moment goes on reading
        its old indices -- clamped, so safe, but other tokens -- until its next Bar (an own-past bar has no such hazard, its
        source is its own sequence).  Switch a form with takes for all slots between runs, before load() or rearm(); a call
        for listed slots only appends and disturbs nothing.  Not
        covered beside the above: generation is left to right, so a bar drawn between kept bars knows only those before it;
        a kept bar gets the chords of its own place in this sequence's progression."""
        self._set_templates(FORM, value, rows)

    def _form_src_plan(self, templates, fresh: bool, label: str = ""):
        """Where the takes of the given forms go in the take buffer: (index: a take's bytes -> its first int, ints in use,
        [(first int, tokens)] still to be written).  Nothing changes; refuses what the buffer does not hold."""
        index = {} if fresh else dict(self._form_src_index)
        used = 0 if fresh else self._form_src_used
        todo, over = [], None
        for i, t in enumerate(templates):
            for tk in (getattr(t, "takes", ()) if t is not None else ()):
                key = tk.tobytes()
                if key not in index:
                    index[key] = used
                    todo.append((used, tk))
                    used += int(tk.size)
            if over is None and used > FORM_SRC_MAX:
                over = i
        if over is not None:
            raise CommuHipError((f"{label} {over}: " if label else "") + f"form: the distinct takes need {used} tokens, "
                                f"the take buffer holds {FORM_SRC_MAX}")
        return index, used, todo

    def _form_src_write(self, index, used, todo):
        """The planned takes written to the buffer in place, ordered on the current stream."""
        if todo:
            self._first_use_form(takes=True)
            for first, tk in todo:
                self._form_src_host[first:first + tk.size] = tk
                self.form_src[first:first + tk.size].copy_(torch.from_numpy(tk))
        self._form_src_index, self._form_src_used = index, used

    def _first_use_form(self, takes: bool = False):
        """What the first form allocates: the words (all off), the table (all free), the slots' replay state and replay
        tokens; the captured graphs are dropped, once: they hold the launches without the rule.  takes: the first form that
        names a take allocates the take buffer as well, at full capacity (FORM_SRC_MAX ints, 1 MiB) so that its address
        stays fixed, and drops the graphs once more: they hold the launches without the buffer."""
        if takes and self.form_src is None:
            self._first_use_form()
            self._form_src_host = np.zeros(FORM_SRC_MAX, dtype=np.int32)
            self.form_src = torch.zeros(FORM_SRC_MAX, dtype=torch.int32, device=self.dev)
            self.graph = self.graph_long = None
            return
        if not self._alloc_rule(FORM):
            return
        self.form_state = torch.zeros(self.B, call("commu_form_state_ints"), dtype=torch.int32, device=self.dev)
        self.form_tok = torch.full((self.B,), -1, dtype=torch.int32, device=self.dev)
        self._form_reset(0, self.B)
        self.graph = self.graph_long = None

    def _form_reset(self, first: int, n: int):
        """The replay state of slots first .. first + n - 1 as a load leaves it: nothing replayed, the Bars of seq recorded."""
        if self.form_ctl is not None:
            call("commu_form_reset", _p(self.form_state), _p(self.form_tok), _p(self.fsm), _p(self.seq), self.ld_seq,
                 int(first), int(n), _s())

    def _form_args(self):
        """The form arguments of the stand-alone stages, in order: five, and the take buffer's two where the decoder has
        one (the _src entry points)."""
        five = _p(self.form_ctl), _p(self.form_table), FORM.rows_max, _p(self.form_state), _p(self.form_tok)
        return five if self.form_src is None else five + (_p(self.form_src), FORM_SRC_MAX)

    def pre(self):
        if self.form_ctl is not None:
            call("commu_forcing_pre_form" if self.form_src is None else "commu_forcing_pre_form_src", _p(self.fsm), _p(self.seq), self.ld_seq, _p(self.chord_tok), _p(self.chord_pos),
                 self.ld_chord, _p(self.wrong), _p(self.utable), self.ld_u, self.generation_length, _p(self.tok),
                 _p(self.active), _p(self.keep), _p(self.draw), _p(self.uni), _p(self.trace), self.ld_trace,
                 _p(self._rows_args()[4]), *self._form_args(), self.B, _s())
            return
        call("commu_forcing_pre", _p(self.fsm), _p(self.seq), self.ld_seq, _p(self.chord_tok), _p(self.chord_pos),
             self.ld_chord, _p(self.wrong), _p(self.utable), self.ld_u, self.generation_length, _p(self.tok),
             _p(self.active), _p(self.keep), _p(self.draw), _p(self.uni), _p(self.trace), self.ld_trace,
             _p(self._rows_args()[4]), self.B, _s())

    def body(self, want_probs: bool = False):
        B = self.B
        self.state.step(self.tok, self.active, None)
        if want_probs and self.probs is None:
            self.probs = torch.zeros(B, TOKEN_OFFSET.VOCAB_SIZE, device=self.dev)
        t_r, k_r, p_r, logp, seq_logp = self._rows_args()
        ops.sample_topk(self.state.logits, self.temperature if t_r is None else t_r, self.top_k if k_r is None else k_r,
                        wrong=self.wrong, uniforms=self.uni, active=self.draw, token=self.token,
                        probs_out=self.probs if want_probs else None, top_p=self.top_p if p_r is None else p_r,
                        logp_out=logp, bias=self.bias, **({} if self.gram is None else {"grammar": self._gram_args()}),
                        **({} if self.harm is None else {"harmony": self._harm_args()}),
                        **({} if self.cls_ctl is None else {"class_ctl": self._cls_args()}),
                        **{r.kw: (w, getattr(self, r.table)) if r.rows_max else w for r, w in self._slot_words()})
        if self.form_ctl is not None:
            call("commu_forcing_post_form" if self.form_src is None else "commu_forcing_post_form_src", _p(self.fsm),
                 _p(self.seq), self.ld_seq, _p(self.chord_pos), self.ld_chord, _p(self.wrong), _p(self.draw), _p(self.token), None, _p(self.state.klen), _p(self.keep),
                 self.state.klen_cap, _p(logp), _p(seq_logp), *self._form_args(), B, _s())
            return
        call("commu_forcing_post", _p(self.fsm), _p(self.seq), self.ld_seq, _p(self.chord_pos), self.ld_chord,
             _p(self.wrong), _p(self.draw), _p(self.token), None, _p(self.state.klen), _p(self.keep),
             self.state.klen_cap, _p(logp), _p(seq_logp), B, _s())

    def body_pre(self):
        """body() followed by pre() with the three per-sequence stages (sampling step, post, pre) as one launch: what
        run() issues per iteration, captured or not."""
        st = self.state
        st.step(self.tok, self.active, None)
        t_r, k_r, p_r, _, seq_logp = self._rows_args()          # (fused: the pair reaches post in registers, no hand-over)
        ld = lambda t: 0 if t is None else t.stride(0)
        # (a constraint the decoder never got is a null pointer: the launch that never heard of it; set_harmony allocated
        # the bias and the grammar its kernel reads)
        cons = {}
        for r, w in self._slot_words():
            cons[r.ctl] = _p(w)
            if r.rows_max:
                cons.update({r.table: _p(getattr(self, r.table)), r.stem + "_rows": r.rows_max})
        if self.form_ctl is not None:          # (the form kernels; a decoder that never had a form: the launch it always made)
            cons.update(form_ctl=_p(self.form_ctl), form_table=_p(self.form_table), form_rows=FORM.rows_max,
                        form_state=_p(self.form_state), form_tok=_p(self.form_tok))
            if self.form_src is not None:      # (the take buffer, whole: its rows hold indices the decoder placed)
                cons.update(form_src=_p(self.form_src), form_src_len=FORM_SRC_MAX)
        a = struct_args(
            DecodeLoopArgs, logits=_p(st.logits), ld=st.logits.stride(0), V=TOKEN_OFFSET.VOCAB_SIZE, B=self.B,
            wrong=_p(self.wrong), temperature=self.temperature, top_k=self.top_k, top_p=self.top_p, temperature_rows=_p(t_r),
            top_k_rows=_p(k_r), top_p_rows=_p(p_r), token=_p(self.token), seq_logp=_p(seq_logp), state=_p(self.fsm),
            seq=_p(self.seq), ld_seq=self.ld_seq, chord_tok=_p(self.chord_tok), chord_pos=_p(self.chord_pos),
            ld_chord=self.ld_chord, utable=_p(self.utable), ld_u=self.ld_u, max_iters=self.generation_length,
            tok=_p(self.tok), active=_p(self.active), keep=_p(self.keep), draw=_p(self.draw), uni=_p(self.uni),
            trace=_p(self.trace), ld_trace=self.ld_trace, klen=_p(st.klen), lmax=st.klen_cap,
            bias=_p(self.bias), ld_bias=ld(self.bias), gram=_p(self.gram), ld_gram=ld(self.gram), gram_on=_p(self.gram_on),
            harm=_p(self.harm), ld_harm=ld(self.harm), harm_on=_p(self.harm_on), cls_ctl=_p(self.cls_ctl),
            **cons)
        call("commu_decode_sample_post_pre", C.byref(a), _s())

    def iteration(self, want_probs: bool = False):
        """One complete iteration, eagerly (tests inspect the draws between iterations)."""
        self.pre()
        self.body(want_probs)

    # The split-key iteration graph pays off when FEW sequences are still alive at LONG memories (one workgroup per
    # (sequence, head) pair then streams ~1 MB alone while most of the chip idles); with all 64 sequences alive the plain
    # kernel already fills the chip and the in-launch combine only costs (measured: 0.60 against 0.37 ms per iteration).
    # (tests/probes/decode_long_rows.py, 64 sequences to completion: no split 77.8 k tokens/s; rows <= 16 / 24 / 32 / 48 with
    #  8 splits 88.9 / 93.8 / 89.2 / 85.2 k; rows <= 32 with 4 splits 93.0 k and the 256-sequence stream 107 k)
    LONG_KLEN = 768        # memories beyond this ...
    LONG_ROWS = 32         # ... and at most this many live sequences
    LONG_SPLITS = 4

    def build_graph(self, long: bool = False):
        """Capture [body, pre].  The warm-up run that the capture needs (allocator pools, lazy module state) is made
        on a scratch copy of every buffer the iteration mutates, which is restored afterwards.  long: the variant for
        long memories (commu_decode_attn_split: up to LONG_SPLITS workgroups per (sequence, head) pair)."""
        st = self.state
        # (the K/V rows the warm-up appends at klen are rewritten by the real run: the caches need no copy)
        bufs = (self.fsm, self.seq, self.wrong, st.klen, st.logits, self.tok, self.active, self.keep, self.draw, self.uni,
                self.seq_logp, self.logp)
        if self.form_ctl is not None:
            bufs += (self.form_state, self.form_tok)
        saved = [t.clone() for t in bufs]
        tr = None if self.trace is None else self.trace.clone()
        keep_splits, st.attn_splits = st.attn_splits, (self.LONG_SPLITS if long else 1)
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.body_pre()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.body_pre()
        finally:
            st.attn_splits = keep_splits
        for dst, src in zip(bufs, saved):
            dst.copy_(src)
        if tr is not None:
            self.trace.copy_(tr)
        if long:
            self.graph_long = g
        else:
            self.graph = g
        return g

    REPLAY_REASONS = {1: "the forcing rules put another token there",
                      2: "the rules would not have appended it (a chord token where a draw is expected, a position past a "
                         "pending chord, or an EOS / BAR that the rules replace)",
                      3: "EOS ends a sequence: nothing can follow it",
                      4: "the slot's record was finished before the prompt was"}

    def _check_prompts(self, prompts):
        """prompts as B lists of ints, validated on the host (None: no prompts)."""
        if prompts is None:
            return None
        if len(prompts) != self.B:
            raise CommuHipError(f"prompts: one token list per slot expected ({self.B}), got {len(prompts)}")
        out = []
        V = TOKEN_OFFSET.VOCAB_SIZE
        for b, p in enumerate(prompts):
            p = [] if p is None else [int(t) for t in p]
            if len(p) > self.max_prompt:
                raise CommuHipError(f"prompt of slot {b} has {len(p)} tokens; this decoder was built with max_prompt="
                                    f"{self.max_prompt}")
            bad = next((i for i, t in enumerate(p) if t < 0 or t >= V), None)
            if bad is not None:
                raise CommuHipError(f"prompt of slot {b}: token {p[bad]} at index {bad} is outside [0, {V})")
            out.append(p)
        return out

    def _prime(self, ctx, prompts):
        """Second half of load(prompts=): replay the prompts through the device state machine (commu_forcing_replay, no
        model step), download records / lengths / divergences once, then fill the caches with the K/V of
        [0] + meta[:n-1] + the kept tokens of the replayed stream in one ragged forward.
        What the replay cannot reconstruct: draws the loop rejected leave no mark in a sequence (a sampled continuation
        consumes its variates from the start of the table), and where the loop replaced a draw by a forced mid-bar chord
        position it fed that position twice -- the replay feeds it once, so the cache is one row shorter there."""
        B, n_cond, st = self.B, self.n_cond, self.state
        pr = np.zeros((B, self.max_prompt), dtype=np.int32)
        for b, p in enumerate(prompts):
            pr[b, :len(p)] = p
        self.prompt.copy_(torch.from_numpy(pr))
        self.prompt_len.copy_(torch.tensor([len(p) for p in prompts], dtype=torch.int32))
        self.fed.zero_()
        st.klen.fill_(n_cond)
        call("commu_forcing_replay", _p(self.fsm), _p(self.seq), self.ld_seq, _p(self.prompt), self.max_prompt,
             _p(self.prompt_len), _p(self.chord_tok), _p(self.chord_pos), self.ld_chord, _p(self.wrong), _p(self.utable),
             self.ld_u, _p(self.tok), _p(self.active), _p(self.keep), _p(self.draw), _p(self.uni), _p(self.trace),
             self.ld_trace, _p(self.seq_logp), _p(st.klen), _p(self.fed), self.ld_fed, _p(self.diverged), B, _s())
        got = torch.cat([self.fsm, st.klen[:, None], self.diverged], 1).cpu().numpy()          # the one download
        klen, div = got[:, self.NF], got[:, self.NF + 1:]
        for b in range(B):
            if div[b, 0] >= 0:
                i, why = int(div[b, 0]), int(div[b, 1])
                raise CommuHipError(f"prompt of slot {b} cannot be continued: token {prompts[b][i]} at index {i} of "
                                    f"{len(prompts[b])}: {self.REPLAY_REASONS.get(why, why)} (reason {why})")
        klen0 = int(klen.max())
        if klen0 - n_cond > self.ld_fed:
            raise CommuHipError(f"the replayed stream of {klen0 - n_cond} kept tokens exceeds the buffer of {self.ld_fed}")
        if self.shared_prompt:
            # equal conditioning, chords and prompts were checked on the host: the replays cannot have diverged
            if int(klen.min()) != klen0:
                raise CommuHipError(f"internal error: equal prompts replayed to different memory lengths {klen.tolist()}")
            self._share(klen0, torch.cat([ctx[:, 0].to(self.dev), self.fed[0, :klen0 - n_cond].long()]))
            self._primed = (self.fsm.clone(), st.klen.clone(), None if self.trace is None else self.trace.clone())
            return
        if not self.sliding and klen0 + self.generation_length + 1 > st.Lmax:
            b = int(klen.argmax())
            raise CommuHipError(
                f"slot {b} starts with {klen0} cached positions (context {n_cond} + {klen0 - n_cond} replayed model steps); "
                f"with generation_length {self.generation_length} that needs {klen0 + self.generation_length + 1} "
                f"positions and the decode memory has {st.Lmax} (shorten the prompt or generation_length, or use "
                "sliding=True)")
        full = torch.zeros(klen0, B, dtype=torch.long, device=self.dev)
        full[:n_cond] = ctx.to(self.dev)
        if klen0 > n_cond:
            full[n_cond:] = self.fed[:, :klen0 - n_cond].t()
        st.prefill_ragged(full, klen.astype(np.int32))
        self.klen0 = klen0
        self._primed = (self.fsm.clone(), st.klen.clone(), None if self.trace is None else self.trace.clone())

    def _check_shared(self, encoded_metas, input_datas, prompts):
        """shared_prompt: every slot must carry what slot 0 carries."""
        def chords(d):
            c = d.chord_token_components
            return [int(t) for t in c["chord_token"]], [int(t) for t in c["chord_position"]]
        m0, c0 = [int(t) for t in encoded_metas[0]], chords(input_datas[0])
        for b in range(1, self.B):
            what = None
            if [int(t) for t in encoded_metas[b]] != m0:
                what = "encoded_meta"
            elif chords(input_datas[b])[0] != c0[0]:
                what = "chord tokens"
            elif chords(input_datas[b])[1] != c0[1]:
                what = "chord positions"
            elif float(input_datas[b].num_measures) != float(input_datas[0].num_measures):
                what = "num_measures"
            elif prompts is not None and prompts[b] != prompts[0]:
                what = "prompt"
            if what is not None:
                raise CommuHipError(f"shared_prompt: slot {b} differs from slot 0 in its {what}; a decoder that shares the "
                                    "prompt needs the same conditioning, chords and prompt in every slot")

    def _share(self, P, column):
        """shared_prompt: the P common positions (tokens `column`) become the shared prefix, every slot starts with no
        private rows."""
        st = self.state
        need = P + self.generation_length + 1
        if need > self._mem_rows:
            raise CommuHipError(
                f"every slot starts with {P} shared positions (context {self.n_cond} + {P - self.n_cond} replayed model "
                f"steps); with generation_length {self.generation_length} that needs {need} positions and the decode memory "
                f"has {self._mem_rows} (shorten the prompt or generation_length)")
        if self.generation_length + 1 > st.Lmax:
            raise CommuHipError(f"generation_length {self.generation_length} needs {self.generation_length + 1} private rows; "
                                f"the decode state has {st.Lmax}")
        st.prefill_shared(column)          # (sets prefix_len = P and klen = 0)
        self.prefix_P = P
        self.klen0 = 0                     # the split-key policy looks at the private rows

    def _keep_ring_rows(self, n):
        """Sliding: once a slot's ring has wrapped its first rows are gone: keep physical rows 0 .. n - 1 for rearm()."""
        n = min(int(n), self.state.Lmax)
        self._ctx_rows = n
        if self.state.parity:
            self._ctx_kv = (self.state.kc[:, :, :n].clone(), self.state.vc[:, :, :n].clone())
        else:
            self._ctx_kv = tuple(t[:, :, :, :n].clone() for t in self.state.cache_tensors())

    # ---- the start state of a request, the one statement load(), rearm(), pool_replay() and admit() share
    @staticmethod
    def _start_record(n_cond, rep):
        """The state record a request's attempt starts from, for its report `rep`."""
        # record: len, forced, redo, first, filled, done, failed, iters, nbar, nchord, cur, length_fit, ndraw, ntrace
        return [1 + n_cond, -1, 0, 1, int(rep.num_measures % 4 == 0), 0, 0, 0, 0, rep.n_chords, 0, int(rep.length_fit), 0, 0]

    def _idle_records(self):
        """[B, NF] records of idle slots: len 1 (seq[0] = 0), nothing forced, done -- they decode nothing."""
        idle = np.zeros((self.B, self.NF), dtype=np.int32)
        idle[:, 0], idle[:, 1], idle[:, 5] = 1, -1, 1
        return idle

    def _chord_rows(self, input_data):
        """(chord tokens, chord positions, a fresh ForcingReport) of a request, checked as the reference checks them."""
        comps = input_data.chord_token_components
        ct, cp = list(comps["chord_token"]), list(comps["chord_position"])
        if len(ct) != len(cp):
            raise AssertionError("Wrong Chord Length")                      # midi_inferrer.py:27
        if len(ct) > self.ld_chord:
            raise CommuHipError(f"{len(ct)} chords > max_chords={self.ld_chord}")
        return ct, cp, ForcingReport(len(ct), float(input_data.num_measures))

    def load(self, encoded_metas: Sequence[Sequence[int]], input_datas, uniforms: Optional[np.ndarray] = None,
             prompts: Optional[Sequence[Sequence[int]]] = None):
        """Conditioning of all B sequences: context [0] + meta[:n-1] into the caches (the n-th meta token is fed by
        the first loop iteration, its memory discarded: quirk Q3), chord progressions, variates.
        prompts (needs max_prompt > 0): one token list per slot (lengths may differ, lists may be empty), the tokens that
        FOLLOW the conditioning tokens.  A primed slot starts in the state the free-running loop would be in after
        producing its prompt itself (_prime); a prompt the rules could not have produced raises CommuHipError."""
        B = self.B
        assert len(encoded_metas) == B and len(input_datas) == B
        prompts = self._check_prompts(prompts)
        n_cond = len(encoded_metas[0])
        if n_cond + 1 > self.n_ctx_max or any(len(m) != n_cond for m in encoded_metas):
            raise CommuHipError("encoded_meta: every sequence needs the same number (<= 15) of conditioning tokens")
        if self.shared_prompt:
            self._check_shared(encoded_metas, input_datas, prompts)
        self.n_cond = n_cond
        self._last_load = (encoded_metas, input_datas, uniforms, prompts)
        self._primed, self.klen0 = None, n_cond
        if getattr(self.state, "t_err", None) is not None:
            self.state.t_err.zero_()          # (a hand-off timeout of an earlier request must not fail this one)
        ctx = torch.tensor([[0] + list(m[:n_cond - 1]) for m in encoded_metas], dtype=torch.long).t().contiguous()
        for t in self.state.cache_tensors():
            t.zero_()
        self.state.repack()          # (the model may have been trained since the decoder was built)
        if prompts is None and self.shared_prompt:          # the conditioning context is what the slots share
            self._share(n_cond, ctx[:, 0].to(self.dev))
        elif prompts is None:
            self.state.prefill(ctx.to(self.dev))
            if self.sliding:
                # keep the context rows for rearm() (rows = positions here, the context is shorter than the ring)
                self._keep_ring_rows(n_cond)
        fsm = np.zeros((B, self.NF), dtype=np.int32)
        seq = np.zeros((B, self.ld_seq), dtype=np.int32)
        ctok = np.zeros((B, self.ld_chord), dtype=np.int32)
        cpos = np.zeros((B, self.ld_chord), dtype=np.int32)
        self.reports: List[ForcingReport] = []
        for b, (meta, data) in enumerate(zip(encoded_metas, input_datas)):
            ct, cp, rep = self._chord_rows(data)
            seq[b, 0] = 0
            seq[b, 1:1 + n_cond] = meta[:n_cond]
            ctok[b, :len(ct)], cpos[b, :len(cp)] = ct, cp
            self.reports.append(rep)
            fsm[b] = self._start_record(n_cond, rep)
        self.fsm.copy_(torch.from_numpy(fsm))
        self.seq.copy_(torch.from_numpy(seq))
        self.seq_logp.fill_(float("nan"))          # (the context was not drawn)
        self.logp.fill_(float("nan"))
        self.chord_tok.copy_(torch.from_numpy(ctok))
        self.chord_pos.copy_(torch.from_numpy(cpos))
        self.wrong.zero_()
        if self.trace is not None:
            self.trace.zero_()
        if uniforms is not None:
            u = np.full((B, self.ld_u), 0.5, dtype=np.float32)
            n = min(uniforms.shape[1], self.ld_u)
            u[:, :n] = uniforms[:, :n]
            self.utable.copy_(torch.from_numpy(u))
        if prompts is not None:
            self._prime(ctx, prompts)
            if self.sliding:
                self._keep_ring_rows(self.klen0)
        self._form_reset(0, B)          # (after the replay: a prompt's bars are valid sources, the bar it leaves open is free)

    # ---- slots: a finished sequence's slot can be re-armed for another attempt of the SAME request (same conditioning
    # tokens and chords) without touching the other slots: the context rows of its K/V cache are what they were, so only
    # the state record, the lengths, the rejected-token map and the variates are reset.  The re-armed slot sits out the
    # iteration in flight (its decision was taken from the finished record) and starts with the next one.
    # Sliding memory: the slot's ring may have wrapped over its context rows, so they are restored from the copy load()
    # took -- device-side copies on the decode stream, ordered between two graph replays, no synchronisation (the small
    # host-to-device copies of the state record and the variates are the ones a re-arm always made).
    # Primed slots (load(prompts=)) return to their PRIMED state: record, klen and trace from the device copies load() took;
    # sliding: the physical rows 0 .. min(longest primed memory, ring rows) - 1.
    # shared_prompt: the prefix belongs to no slot and is never written by a step; the slot's private rows are abandoned
    # (klen = 0), nothing is copied.
    # sampling: a (temperature, top_k, top_p) triple for the slot's next attempt (None: the slot keeps its controls).
    # logit_bias: a constraint row for the slot's next attempt (None: the slot keeps its row; set_logit_bias clears one).
    # grammar: True / False switches the slot's event grammar for its next attempt (None: the slot keeps its switch).
    # harmony: True / False switches the slot's harmony constraint for its next attempt (None: the slot keeps its switch).
    # **rules: one keyword per rule of SLOT_RULES (note_order, voices, density, interval, onsets, guide, articulation, form):
    # the slot's setting for its next attempt, the values of the rule's setter with False for off (None: the slot keeps its
    # word).  They are set in the table's order, so what a rule implies is in place before it; the slot's replay state is
    # reset with its record whatever the form.
    def rearm(self, b: int, uniforms_row: Optional[np.ndarray] = None, sampling=None, logit_bias=None, grammar=None,
              harmony=None, **rules):
        for kw, value in _rule_values(rules).items():
            if value is not None:
                getattr(self, RULE_OF[kw].setter)(value, rows=[b])
        if sampling is not None:
            self.set_sampling(*sampling, rows=[b])
        if logit_bias is not None:
            self.set_logit_bias(logit_bias, rows=[b])
        if grammar is not None:
            if self.gram is None or self._gram_host is None:      # (no table yet: set_harmony's all-off grammar holds zeros)
                self.set_grammar(True if grammar else None, rows=[b])
            else:                              # (the table stays: one byte changes)
                self.gram_on[int(b)].fill_(1 if grammar else 0)
        if harmony is not None:
            if self.harm is None or self._harm_host is None:
                self.set_harmony(True if harmony else None, rows=[b])
            else:
                self.harm_on[int(b)].fill_(1 if harmony else 0)
        rep0 = self.reports[b]
        rep = ForcingReport(rep0.n_chords, rep0.num_measures)
        self.reports[b] = rep
        if self._primed is not None:          # back to the primed state: the record as the replay left it (device copy)
            self.fsm[b].copy_(self._primed[0][b])
        else:
            self.fsm[b].copy_(torch.tensor(self._start_record(self.n_cond, rep), dtype=torch.int32))
        self._form_reset(b, 1)                # (seq[b] up to the record's length is the context and the prompt)
        self.wrong[b].zero_()
        self.seq_logp[b].fill_(float("nan"))
        if self.sliding:
            st, n = self.state, self._ctx_rows
            if st.parity:
                ck, cv = self._ctx_kv
                st.kc[:, b, :n].copy_(ck[:, b])
                st.vc[:, b, :n].copy_(cv[:, b])
            else:
                for t, c in zip(st.cache_tensors(), self._ctx_kv):
                    t[:, b, :, :n].copy_(c[:, b])
        if self.shared_prompt:               # no rows to restore: the slot's private rows are simply abandoned
            self.state.klen[b] = 0
        elif self._primed is not None:
            self.state.klen[b].copy_(self._primed[1][b])
        else:
            self.state.klen[b] = self.n_cond
        if uniforms_row is not None:
            u = np.full(self.ld_u, 0.5, dtype=np.float32)
            n = min(len(uniforms_row), self.ld_u)
            u[:n] = uniforms_row[:n]
            self.utable[b].copy_(torch.from_numpy(u))
        if self.trace is not None:
            if self._primed is not None:      # (the recorded trace covers the replayed stream too)
                self.trace[b].copy_(self._primed[2][b])
            else:
                self.trace[b].zero_()

    # ---- request pool: a slot armed for ANY request.  What load() writes for all slots at once -- conditioning K/V
    # rows, chord rows, state record, sequence head, per-slot controls -- is composed ONCE per request into an entry of
    # a device-side request store (admit) and moved into the slots by ONE launch per poll window (arm,
    # commu_decode_arm), between two graph replays.  A decoder that never calls pool_open() allocates none of this and
    # launches what it always launched.
    def pool_image_rows(self) -> int:
        """K/V image rows of a store entry.  A decoder without prompts: the context, n_ctx_max.  A primed decoder
        (max_prompt > 0): what a replay can leave, n_ctx_max + ld_fed, on a linear cache; on a ring of W = Lmax rows
        min(W, n_ctx_max + ld_fed) -- either no prompt wraps (rows are positions), or the image is a ring with the
        cache's own modulus and the prefill scatter's row rule is the cache's."""
        if self.max_prompt == 0:
            return self.n_ctx_max
        rows = self.n_ctx_max + self.ld_fed
        return min(self.state.Lmax, rows)          # (linear: a prompt that does not fit the cache is refused anyway)

    def pool_replay(self, encoded_metas, input_datas, prompts):
        """The primed half of a pool's admission, for ALL its requests before the pool is opened: every non-empty prompt
        is replayed through the device state machine (commu_forcing_replay, no model step) in batches of up to B, the
        slot arrays serving as scratch rows (pool_open resets every one of them afterwards), one download per batch.
        Returns per request None (no prompt) or its replay result on the host -- record, seq[:len], the kept fed tokens,
        klen0, the trace row -- from which admit(primed=) composes the store entry without a synchronisation.  Raises
        CommuHipError naming the request for a prompt that leaves the rules, a replayed stream beyond the fed buffer,
        and, on a linear cache, klen0 + generation_length + 1 > Lmax."""
        if self.max_prompt < 1:
            raise CommuHipError("pool_replay: a decoder built with max_prompt > 0 expected")
        B, NF, st = self.B, self.NF, self.state
        n_cond = len(encoded_metas[0])
        out = [None] * len(prompts)
        todo = [i for i, p in enumerate(prompts) if p]
        for lo in range(0, len(todo), B):
            batch = todo[lo:lo + B]
            fsm = self._idle_records()          # rows beyond the batch: idle, no prompt
            seq = np.zeros((B, self.ld_seq), dtype=np.int32)
            chords = np.zeros((2, B, self.ld_chord), dtype=np.int32)
            pr = np.zeros((B, self.max_prompt), dtype=np.int32)
            plen = np.zeros(B, dtype=np.int32)
            for b, i in enumerate(batch):
                ct, cp, rep = self._chord_rows(input_datas[i])
                fsm[b] = self._start_record(n_cond, rep)
                seq[b, 1:1 + n_cond] = list(encoded_metas[i])
                chords[0, b, :len(ct)], chords[1, b, :len(cp)] = ct, cp
                pr[b, :len(prompts[i])] = prompts[i]
                plen[b] = len(prompts[i])
            up = lambda dst, a: dst.copy_(torch.from_numpy(np.ascontiguousarray(a)))
            up(self.fsm, fsm)
            up(self.seq, seq)
            up(self.chord_tok, chords[0])
            up(self.chord_pos, chords[1])
            up(self.prompt, pr)
            up(self.prompt_len, plen)
            self.wrong.zero_()
            self.fed.zero_()
            st.klen.fill_(n_cond)
            if self.trace is not None:
                self.trace.zero_()
            call("commu_forcing_replay", _p(self.fsm), _p(self.seq), self.ld_seq, _p(self.prompt), self.max_prompt,
                 _p(self.prompt_len), _p(self.chord_tok), _p(self.chord_pos), self.ld_chord, _p(self.wrong), _p(self.utable),
                 self.ld_u, _p(self.tok), _p(self.active), _p(self.keep), _p(self.draw), _p(self.uni), _p(self.trace),
                 self.ld_trace, _p(self.seq_logp), _p(st.klen), _p(self.fed), self.ld_fed, _p(self.diverged), B, _s())
            parts = [self.fsm, st.klen[:, None], self.diverged, self.fed, self.seq[:, :self.n_ctx_max + self.max_prompt]]
            if self.trace is not None:
                parts.append(self.trace)
            got = torch.cat(parts, 1).cpu().numpy()          # the batch's one download
            o_fed = NF + 3
            o_seq = o_fed + self.ld_fed
            o_tr = o_seq + self.n_ctx_max + self.max_prompt
            for b, i in enumerate(batch):
                rec, klen0, div = got[b, :NF].copy(), int(got[b, NF]), got[b, NF + 1:NF + 3]
                if div[0] >= 0:
                    k, why = int(div[0]), int(div[1])
                    raise CommuHipError(f"generate_pool: request {i}: the prompt cannot be continued: token {prompts[i][k]} at "
                                        f"index {k} of {len(prompts[i])}: {self.REPLAY_REASONS.get(why, why)} (reason {why})")
                if klen0 - n_cond > self.ld_fed:
                    raise CommuHipError(f"generate_pool: request {i}: the replayed stream of {klen0 - n_cond} kept tokens "
                                        f"exceeds the buffer of {self.ld_fed}")
                if not self.sliding and klen0 + self.generation_length + 1 > st.Lmax:
                    raise CommuHipError(
                        f"generate_pool: request {i} starts with {klen0} cached positions (context {n_cond} + "
                        f"{klen0 - n_cond} replayed model steps); with generation_length {self.generation_length} that needs "
                        f"{klen0 + self.generation_length + 1} positions and the decode memory has {st.Lmax} (shorten the "
                        "prompt or generation_length, or use sliding=True)")
                out[i] = {"record": rec, "seq": got[b, o_seq:o_seq + int(rec[0])].copy(),
                          "fed": got[b, o_fed:o_fed + klen0 - n_cond].copy(), "klen0": klen0,
                          "trace": None if self.trace is None else got[b, o_tr:o_tr + self.ld_trace].copy()}
        return out

    def pool_open(self, n_cond: int, grid_rows: int = 0):
        """Every slot idle (a finished record that decodes nothing), the store of Rcap = B entries allocated on first
        use: the state a pool starts from instead of load().  n_cond: the number of conditioning tokens of every request
        of the pool.  A decoder built with max_prompt > 0 serves primed entries (admit(primed=)): its store has
        pool_image_rows() image rows and sequence heads of n_ctx_max + max_prompt words per entry, and its arm launch is
        commu_decode_arm_primed; grid_rows: the pool's longest image (0: unknown, every chunk of the store is launched).
        The store is Rcap = B entries of pool_image_rows() rows: B / Lmax * rows of the cache's own bytes (with 256 slots
        and 1000-token prompts about what a 64-slot cache of 8192 positions holds)."""
        if self.shared_prompt:
            raise CommuHipError("request pool: shared-prompt decoders are not served (the prefix belongs to no slot)")
        if self.state.parity:
            raise CommuHipError("request pool: the fp32 parity mode (model.parity_fp32) has a third cache layout that the "
                                "arm launch does not copy")
        n_cond = int(n_cond)
        if n_cond < 1 or n_cond + 1 > self.n_ctx_max:
            raise CommuHipError(f"encoded_meta: 1 .. {self.n_ctx_max - 1} conditioning tokens expected, got {n_cond}")
        if self.sliding and self.state.window < n_cond:
            raise CommuHipError(f"request pool: a sliding window of {self.state.window} positions is shorter than the context "
                                f"of {n_cond} tokens")
        self._first_use(rows=True)          # (requests differ in their triples: the array launches from the start)
        B, st, dev = self.B, self.state, self.dev
        self.n_cond, self.klen0, self._primed, self._last_load = n_cond, n_cond, None, None
        if getattr(st, "t_err", None) is not None:
            st.t_err.zero_()
        for t in st.cache_tensors():
            t.zero_()
        st.repack()
        self.fsm.copy_(torch.from_numpy(self._idle_records()))
        self.seq.zero_()
        self._form_reset(0, B)
        self.seq_logp.fill_(float("nan"))
        self.logp.fill_(float("nan"))
        self.wrong.zero_()
        st.klen.zero_()
        if self.trace is not None:
            self.trace.zero_()
        self.reports = [None] * B
        if getattr(self, "_pool", None) is None:
            R, i32, u8 = B, torch.int32, torch.uint8
            z = lambda *shape, dtype=i32: torch.zeros(*shape, dtype=dtype, device=dev)
            hdr = (2 * B + 3) // 4 * 4          # the jobs, padded so that the variates start at a 16-byte boundary
            words = hdr + B * self.ld_u
            rows = self.pool_image_rows()
            self._pool = {
                "image": tuple(z(t.shape[0], R, t.shape[2], rows, t.shape[4], dtype=t.dtype)
                               for t in st.cache_tensors()),
                "primed": self.max_prompt > 0, "rows": rows, "ld_head": self.n_ctx_max + self.max_prompt,
                "e_trace": z(R, self.ld_trace) if (self.max_prompt > 0 and self.trace is not None) else None,
                "e_klen0": z(R), "e_state": z(R, self.NF), "e_seq": z(R, self.n_ctx_max + self.max_prompt),
                "e_chord_tok": z(R, self.ld_chord), "e_chord_pos": z(R, self.ld_chord),
                "e_temperature": z(R, dtype=F32), "e_top_k": z(R), "e_top_p": z(R, dtype=F32),
                "e_bias": z(R, VPAD, dtype=F32), "e_gram_on": z(R, dtype=u8), "e_harm_on": z(R, dtype=u8),
                **{r.entry: torch.full((R,), r.off, dtype=i32, device=dev) for r in SLOT_RULES},
                "e_cls": z(R, N_CLASSES + 1, 4),
                "hdr": hdr, "stage": z(words),
                # two pinned staging buffers and an event each: the host never overwrites a buffer whose copy is in flight
                "pin": [torch.zeros(words, dtype=i32).pin_memory() for _ in range(2)],
                "ev": [None, None], "turn": 0, "args": None, "sig": None,
                "one": torch.ones(1, dtype=i32, device=dev),
                "meta": [None] * R,          # per entry: (n_chords, num_measures) for the slots' reports
            }
        P = self._pool
        P["grid_rows"] = max(0, min(int(grid_rows), P["rows"]))
        self.klen0 = max(n_cond, P["grid_rows"])

    def pool_store_bytes(self) -> int:
        """Bytes of the request store's K/V images: Rcap = B entries of pool_image_rows() rows in the cache's format."""
        return sum(t.numel() * t.element_size() for t in self._pool["image"])

    @property
    def arm_kernel(self) -> str:
        """The entry point arm() launches."""
        return "commu_decode_arm_primed" if self.max_prompt > 0 else "commu_decode_arm"

    def _pool_args(self):
        """The arm launch's argument block, rebuilt when an optional array was allocated since (a null twin: not written)."""
        P = self._pool
        words = {r: getattr(self, r.ctl) for r in SLOT_RULES}
        opt = (self.bias, self.gram_on, self.harm_on, self.cls_ctl, self.trace) + tuple(words.values())
        sig = tuple(None if t is None else t.data_ptr() for t in opt)
        if P["args"] is None or P["sig"] != sig:
            st = self.state
            on = lambda t, e: {} if t is None else e
            # (the one block of both launches; only a primed pool names the ring mode, the trace twin and grid_rows below)
            primed = {"ring": int(self.sliding), **on(P["e_trace"], {"e_trace": P["e_trace"]})} if P["primed"] else {}
            P["args"] = ops.decode_arm_args(
                st.cache_tensors(), P["image"], jobs=P["stage"], variates=P["stage"][P["hdr"]:].view(F32),
                klen=st.klen, e_klen0=P["e_klen0"], state=self.fsm, e_state=P["e_state"], nf=self.NF,
                seq=self.seq, e_seq=P["e_seq"], ld_seq=self.ld_seq, ld_head=P["ld_head"],
                chord_tok=self.chord_tok, chord_pos=self.chord_pos, e_chord_tok=P["e_chord_tok"],
                e_chord_pos=P["e_chord_pos"], ld_chord=self.ld_chord, wrong=self.wrong, ld_wrong=self.wrong.stride(0),
                utable=self.utable, ld_u=self.ld_u, seq_logp=self.seq_logp, trace=self.trace, ld_trace=self.ld_trace,
                temperature_rows=self.temperature_rows, top_k_rows=self.top_k_rows, top_p_rows=self.top_p_rows,
                e_temperature=P["e_temperature"], e_top_k=P["e_top_k"], e_top_p=P["e_top_p"],
                **on(self.bias, {"bias": self.bias, "e_bias": P["e_bias"], "ld_bias": VPAD}),
                **on(self.gram_on, {"gram_on": self.gram_on, "e_gram_on": P["e_gram_on"]}),
                **on(self.harm_on, {"harm_on": self.harm_on, "e_harm_on": P["e_harm_on"]}),
                **{k: v for r, w in words.items() if w is not None for k, v in ((r.ctl, w), (r.entry, P[r.entry]))},
                **on(self.form_ctl, {"form_state": self.form_state, "form_tok": self.form_tok}),
                **on(self.cls_ctl, {"cls_ctl": self.cls_ctl, "e_cls": P["e_cls"]}), **primed)
            P["sig"] = sig
        if P["primed"]:
            P["args"].grid_rows = P["grid_rows"]          # (this pool's longest image: fewer chunk workgroups)
        return P["args"]

    def admit(self, entry: int, encoded_meta: Sequence[int], input_data, sampling=None, logit_bias=None, grammar=False,
              harmony=False, class_table=None, primed=None, **rules):
        """Compose store entry `entry` for a request and upload it with its K/V image: the state record, sequence head
        and chord rows as load() builds them, klen0 = n_cond, the sampling triple (None: the decoder's), the bias row
        (None: zeros), the grammar and harmony switches (they switch on what the decoder has a table for), the word of
        every rule of SLOT_RULES (**rules: one setting for the request by the rule's keyword, None: off; what a rule
        implies is switched on as its setter does; a template's rows go to the decoder's own table, where the same template
        is stored once -- no table bytes move per arm; the arm launch resets the slot's replay state and records the Bars
        of the entry's sequence head) and, where the decoder has class records, the request's record row
        (class_table: its NaN-table, None: the base triple in every record).  The image is written by ONE memory-less
        forward over this request's single column [n_cond, 1] and the prefill scatter of the cache's format into the
        store: it does not depend on what else is admitted or decoding.  Everything is ordered on the current stream.
        primed (a decoder built with max_prompt > 0): the request's replay result (pool_replay) -- the entry is then the
        record as the replay left it, the sequence head [0] + meta + prompt, the replay's trace row, klen0 as replayed,
        and the image comes from the forward over the single column [0] + meta[:n-1] + fed (T = klen0, B = 1): the forward
        load(prompts=) runs at one slot."""
        rules = _rule_values(rules)
        P = getattr(self, "_pool", None)
        if P is None:
            raise CommuHipError("admit: pool_open() first")
        if primed is not None and not P["primed"]:
            raise CommuHipError("admit: a primed entry, but the decoder was built without prompts (max_prompt=)")
        entry, n_cond = int(entry), self.n_cond
        if entry < 0 or entry >= self.B:
            raise CommuHipError(f"admit: store entries are 0 .. {self.B - 1}, got {entry}")
        if len(encoded_meta) != n_cond:
            raise CommuHipError(f"encoded_meta: the pool was opened for {n_cond} conditioning tokens, got {len(encoded_meta)}")
        t, k, p = sampling_rows(1, *((self.temperature, self.top_k, self.top_p) if sampling is None else sampling))
        bias = None if logit_bias is None else logit_bias_rows(logit_bias, 1)[0]
        vals = {RULE_OF[kw]: RULE_OF[kw].normalize(v, 1) for kw, v in rules.items()}
        for r, v in vals.items():
            if r.is_on(v[0]) and getattr(self, r.ctl) is None:
                raise CommuHipError(f"admit: {r.asks} ({r.setter})")
        _form_needs_grammar(vals[FORM], [0] if grammar else [])
        if grammar and (self.gram is None or self._gram_host is None):
            raise CommuHipError("admit: grammar switched on, but the decoder has no grammar table (set_grammar)")
        if harmony and (self.harm is None or self._harm_host is None):
            raise CommuHipError("admit: harmony switched on, but the decoder has no harmony table (set_harmony)")
        if bias is not None and self.bias is None:
            raise CommuHipError("admit: a logit bias, but the decoder has no bias rows (set_logit_bias)")
        for r in reversed(SAMPLING_RULES):          # (from the top: the density reaches the note order through the voices)
            dep = RULE_OF.get(r.implies)
            if dep is not None and r.is_on(vals[r][0]) and not dep.is_on(vals[dep][0]):
                vals[dep][0] = 0                  # (as the rule's setter: word 0, no cap, where the request leaves it off)
        if class_table is not None and self.cls_ctl is None:
            raise CommuHipError("admit: a class table, but the decoder has no class records (set_class_sampling)")
        ct, cp, rep = self._chord_rows(input_data)
        P["meta"][entry] = (rep.n_chords, rep.num_measures)
        up = lambda dst, a: dst.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        head = np.zeros(P["ld_head"], dtype=np.int32)
        if primed is None:
            up(P["e_state"][entry], np.array(self._start_record(n_cond, rep), dtype=np.int32))
            head[1:1 + n_cond] = list(encoded_meta)
        else:
            up(P["e_state"][entry], primed["record"])
            head[:len(primed["seq"])] = primed["seq"]
        up(P["e_seq"][entry], head)
        if P["e_trace"] is not None:
            if primed is None:
                P["e_trace"][entry].zero_()
            else:
                up(P["e_trace"][entry], primed["trace"])
        chords = np.zeros((2, self.ld_chord), dtype=np.int32)
        chords[0, :len(ct)], chords[1, :len(cp)] = ct, cp
        up(P["e_chord_tok"][entry], chords[0])
        up(P["e_chord_pos"][entry], chords[1])
        P["e_temperature"][entry].fill_(t[0].item())
        P["e_top_k"][entry].fill_(int(k[0]))
        P["e_top_p"][entry].fill_(p[0].item())
        if self.bias is not None:
            if bias is None:
                P["e_bias"][entry].zero_()
            else:
                up(P["e_bias"][entry], bias)
        P["e_gram_on"][entry].fill_(1 if grammar else 0)
        P["e_harm_on"][entry].fill_(1 if harmony else 0)
        for r, v in vals.items():
            word = r.off if not r.is_on(v[0]) else self._pack(r, v)[0] if r.rows_max else v[0]
            P[r.entry][entry].fill_(int(word))
        if self.cls_ctl is not None:
            tab = np.full((1, N_CLASSES + 1, 3), np.nan) if class_table is None else class_sampling_table(class_table)[None]
            rec = class_ctl_records(tab, [t, k, p])
            up(P["e_cls"][entry], rec.view(np.int32).reshape(N_CLASSES + 1, 4))
        # the image: one forward over the request's own column, scattered into the store as into a cache of Rcap slots
        # with n_ctx_max rows (rows = positions: the context is shorter than any ring)
        # (a primed entry: the column goes on with the kept tokens of the replayed stream, T = klen0; where the store's
        #  image is a ring -- a sliding decoder whose image has the cache's Lmax rows -- the scatter's row rule is the ring's)
        col = [0] + [int(x) for x in encoded_meta[:n_cond - 1]] + ([] if primed is None else [int(x) for x in primed["fed"]])
        T = len(col)
        if primed is not None and T != primed["klen0"]:
            raise CommuHipError(f"admit: internal error: a replayed column of {T} tokens for klen0 = {primed['klen0']}")
        ctx = torch.tensor([col], dtype=torch.long).t().contiguous().to(self.dev)
        _, _, qkvs = self.model._run_forward(ctx, None, None, None, need_grad=False, want_logits=True, want_kv=True)
        lens = P["one"] * T
        slot = P["one"] * entry
        img = P["image"]
        ring = {"window": self.state.window} if (P["primed"] and self.sliding and P["rows"] == self.state.Lmax) else {}
        if not ring and T > P["rows"]:
            raise CommuHipError(f"admit: {T} cached positions for a store image of {P['rows']} rows")
        for i, qkv in enumerate(qkvs):
            q2 = qkv.view(T, -1)
            if self.state.kv_dtype == "fp8":
                ops.decode_prefill_scatter_kv8(q2, T, img[0][i], img[1][i], img[2][i], img[3][i], P["e_klen0"], lens, slot,
                                               **ring)
            else:
                ops.decode_prefill_scatter(q2, T, img[0][i], img[1][i], P["e_klen0"], lens, slot, **ring)

    def arm(self, jobs):
        """Arm slots for the window: jobs is a list of (slot, entry, variates row or None), distinct slots.  The jobs and
        their variates are staged in pinned memory, copied to the device block by ONE non-blocking copy, and ONE
        commu_decode_arm launch moves each entry into its slot -- K/V image, klen, record, sequence head, chords,
        variates, controls; wrong zeroed, seq_logp NaN, trace zeroed (a decoder built with max_prompt > 0:
        commu_decode_arm_primed, which copies long images row-parallel and the entry's trace).  self.reports[slot] becomes
        the new attempt's.  No synchronisation: an armed slot sits out the iteration in flight and starts with the next
        one, as after rearm()."""
        P = getattr(self, "_pool", None)
        if P is None:
            raise CommuHipError("arm: pool_open() first")
        jobs = list(jobs)
        if not jobs:
            return
        slots = [int(j[0]) for j in jobs]
        if len(set(slots)) != len(slots) or min(slots) < 0 or max(slots) >= self.B:
            raise CommuHipError(f"arm: distinct slots in [0, {self.B}) expected, got {slots}")
        for _, e, _ in jobs:
            if not 0 <= int(e) < self.B or P["meta"][int(e)] is None:
                raise CommuHipError(f"arm: store entry {e} was not admitted")
        args = self._pool_args()
        turn = P["turn"]
        P["turn"] = 1 - turn
        if P["ev"][turn] is not None:
            P["ev"][turn].synchronize()          # (the copy out of this buffer two arms ago: long done)
        pin = P["pin"][turn].numpy()
        n, hdr, ld_u = len(jobs), P["hdr"], self.ld_u
        pin[:2 * n] = np.array([(int(s), int(e)) for s, e, _ in jobs], dtype=np.int32).reshape(-1)
        uni = pin[hdr:hdr + n * ld_u].view(np.float32).reshape(n, ld_u)
        for j, (_, _, u) in enumerate(jobs):
            uni[j] = 0.5
            if u is not None:
                m = min(len(u), ld_u)
                uni[j, :m] = u[:m]
        words = hdr + n * ld_u
        P["stage"][:words].copy_(P["pin"][turn][:words], non_blocking=True)
        if P["ev"][turn] is None:
            P["ev"][turn] = torch.cuda.Event()
        P["ev"][turn].record()
        if P["primed"]:
            ops.decode_arm_primed(args, n)
        else:
            ops.decode_arm(args, n)
        for s, e, _ in jobs:
            self.reports[int(s)] = ForcingReport(*P["meta"][int(e)])

    def harvest(self, b: int, fsm_row):
        """Token list of slot b (None where nothing could be drawn, Q12) from its downloaded state record."""
        self.reports[b].consumed = int(fsm_row[10])
        if fsm_row[6]:
            return None
        return self.seq[b, :int(fsm_row[0])].cpu().tolist()

    def _need_logprobs(self):
        if not self.rows_on:
            raise CommuHipError("no log-probabilities were recorded: call record_logprobs() (or set_sampling()) before load()")

    def harvest_logprobs(self, b: int, fsm_row):
        """harvest()'s companion: the log-probability pairs (full, kept) of slot b's tokens, numpy [len, 2] with NaN rows
        where a token was not drawn (context, forced); None where the sequence failed."""
        self._need_logprobs()
        if fsm_row[6]:
            return None
        return self.seq_logp[b, :int(fsm_row[0])].cpu().numpy()

    # ---- done flags without stalling the GPU: the flags of window k are copied to pinned memory behind window k and
    # looked at after window k + 1 has been queued, so the device never waits for the host between windows (a
    # synchronous read costs the wake-up + first launch, ~60 us per 16 iterations); the price is that up to POLL
    # iterations are queued beyond the one that finished the last sequence (they do nothing: every slot is inactive)
    def poll_submit(self):
        if getattr(self, "_done_pin", None) is None:
            self._done_pin = torch.zeros(self.B, self.NF, dtype=torch.int32).pin_memory()
            self._done_ev = torch.cuda.Event()
        self._done_pin.copy_(self.fsm, non_blocking=True)
        self._done_ev.record()

    def poll_result(self):
        """The state records as of the last poll_submit (numpy [B, NF]; waits for that copy only)."""
        self._done_ev.synchronize()
        return self._done_pin.numpy().copy()

    def run_iterations(self, n: int, use_graph: bool = True, klen_bound: int = 0, live_rows: Optional[int] = None):
        """n iterations.  klen_bound: an upper bound of the memory lengths during them (0: unknown / short), live_rows: the
        number of sequences still decoding (None: unknown = all): beyond LONG_KLEN with at most LONG_ROWS live sequences
        the split-key iteration graph runs (built on first use)."""
        if self.sliding:          # a ring never holds more keys than it has rows
            klen_bound = min(klen_bound, self.state.Lmax)
        long = klen_bound > self.LONG_KLEN and live_rows is not None and live_rows <= self.LONG_ROWS
        if use_graph and long and getattr(self, "graph_long", None) is None:
            self.build_graph(long=True)
        if use_graph and not long and self.graph is None:          # (dropped by a set_sampling / record_logprobs since)
            self.build_graph()
        g = self.graph_long if (use_graph and long) else self.graph
        if not use_graph:
            keep_splits, self.state.attn_splits = self.state.attn_splits, (self.LONG_SPLITS if long else 1)
        try:
            for _ in range(n):
                if use_graph:
                    g.replay()
                else:
                    self.body_pre()
        finally:
            if not use_graph:
                self.state.attn_splits = keep_splits

    def run(self, use_graph: bool = True):
        try:
            self._run(use_graph)
        except CommuHipError:
            # a layer-tail launch gave up at a hand-off (e.g. the GPU was shared and its workgroups were not co-resident):
            # generate the request again on the chain of per-Linear launches instead of failing it
            if not self.state.tail_ok or getattr(self, "_last_load", None) is None:
                raise
            self.state.tail_ok = False
            self.graph = self.graph_long = None
            self.load(*self._last_load)
            self._run(use_graph)

    def _run(self, use_graph: bool = True):
        if use_graph and self.graph is None:
            self.build_graph()
        self.pre()                                          # decision of the first iteration
        it, pending, live = 0, False, None
        while it < self.generation_length + 1:
            self.run_iterations(self.POLL, use_graph, klen_bound=self.klen0 + it + self.POLL, live_rows=live)
            it += self.POLL
            if pending:
                rec = self.poll_result()                                  # the records one window back: no stall
                if bool(rec[:, 5].all()):
                    break
                live = int((rec[:, 5] == 0).sum())
            self.poll_submit()
            pending = True
        torch.cuda.current_stream().synchronize()
        self.state.check()

    def sequences(self):
        """Token lists (None where nothing could be drawn, Q12) and, per sequence, the model-step trace
        [(fed token, memory length before, after)] when it was recorded (the lengths of the reference's memory tensor)."""
        fsm = self.fsm.cpu().numpy()
        seq = self.seq.cpu().numpy()
        out, traces = [], []
        tr = None if self.trace is None else self.trace.cpu().numpy()
        for b in range(self.B):
            self.reports[b].consumed = int(fsm[b, 10])
            out.append(None if fsm[b, 6] else seq[b, :fsm[b, 0]].tolist())
            if tr is not None:
                klen, t = self.n_cond, []
                # (sliding: the memory the reference would report holds at most `window` positions, model.py:524-536)
                cap = self.state.window if self.sliding else klen + self.ld_trace
                for k in range(min(int(fsm[b, 13]), self.ld_trace // 2)):
                    t.append((int(tr[b, 2 * k]), min(klen, cap), min(klen + 1, cap)))
                    klen += int(tr[b, 2 * k + 1])
                traces.append(t)
        return out, traces

    def logprobs(self):
        """Per sequence the [len, 2] float32 array of (full, kept) log-probabilities of its tokens -- full: log-softmax
        over ids 1 .. 728 of the row the draw used (logits / temperature) at the token; kept: log of the token's probability
        in the distribution it was drawn from (0 for greedy); NaN rows for the context and forced tokens -- or None where
        the sequence failed (Q12)."""
        self._need_logprobs()
        fsm = self.fsm.cpu().numpy()
        lp = self.seq_logp.cpu().numpy()
        return [None if fsm[b, 6] else lp[b, :fsm[b, 0]].copy() for b in range(self.B)]


@dataclasses.dataclass
class PoolRequest:
    """One request of BatchedGenerator.generate_pool: what generate_stream takes for it alone.  accept: a callable
    (seq, report) -> bool, None accepts every sequence that is not None; logit_bias: one row; grammar / harmony: a
    per-request bool (None: on where the pool has a table), they may only switch on what the pool has a table for;
    note_order / voices / density / interval / onsets / guide / articulation / form: the rules of SLOT_RULES, ONE setting
    each as generate_stream takes it (the pool packs its requests' templates into one table per rule; hold_guide needs the
    request's own guide, "copy": "rhythm" its grammar on).  prompt: token ids that follow the conditioning tokens and that
    every attempt of THIS request continues (generate_stream's prompt=); None or [] is an unprimed request."""
    encoded_meta: Sequence[int]
    input_data: object
    need: int
    temperature: float
    top_k: int
    top_p: float = 1.0
    seed: int = 0
    max_attempts: Optional[int] = None
    accept: Optional[object] = None
    logit_bias: Optional[object] = None
    grammar: Optional[bool] = None
    harmony: Optional[bool] = None
    note_order: Optional[object] = None
    voices: Optional[object] = None
    prompt: Optional[Sequence[int]] = None
    density: Optional[object] = None
    interval: Optional[object] = None
    onsets: Optional[object] = None
    guide: Optional[object] = None
    articulation: Optional[object] = None
    form: Optional[object] = None


PoolResult = collections.namedtuple("PoolResult", ["sequences", "attempts_started", "logprobs"])
PoolJob = collections.namedtuple("PoolJob", ["slot", "request", "attempt", "entry", "admit"])


class PoolSchedule:
    """Which attempt of which request a free decode slot takes: the policy of generate_pool, host only.

    Requests are served in list order: a free slot takes the next attempt of the EARLIEST request that still wants one.
    A request wants an attempt while in_flight + accepted < need and started < max_attempts; attempts are numbered
    0, 1, 2, ... per request.  A request is decided when nothing of it is in flight and accepted == need or max_attempts
    is exhausted; its answer is its accepted attempts in attempt order, and its store entry is freed.

    Why that answer is generate_stream's "first `need` accepted attempts in attempt order".  Attempts start in number
    order, so the started ones are 0 .. s - 1.  The cap gives in_flight + accepted <= need at all times, hence never
    more than `need` accepted attempts, and a decision with accepted == need means the accepted attempts are ALL the
    accepted ones among 0 .. s - 1, exactly `need` of them: the first `need`.  s is also the sequential loop's count:
    attempt s - 1 was started while in_flight + accepted < need counted every attempt below it that was not yet
    rejected, so fewer than `need` of 0 .. s - 2 are accepted in the end -- attempt s - 1 is the need-th accepted one,
    where the one-at-a-time loop stops too.  With max_attempts exhausted the answer is every accepted attempt of
    0 .. max_attempts - 1 (fewer than `need`, or the cap would have stopped earlier), as there.

    The store has one entry per slot and that is enough: a rejection frees a slot in the same event that makes its
    request want one, and earlier requests come first, so after every assignment each admitted, undecided request has
    an attempt in flight -- at most `slots` entries are live."""

    def __init__(self, needs: Sequence[int], max_attempts: Sequence[Optional[int]], slots: int):
        self.need = [int(n) for n in needs]
        self.cap = [None if m is None else int(m) for m in max_attempts]
        n = len(self.need)
        self.started, self.in_flight, self.accepted = [0] * n, [0] * n, [0] * n
        self.results = [{} for _ in range(n)]          # attempt -> (accepted, payload)
        self.entry = [None] * n                        # the store entry of an admitted, undecided request
        self.decided = [False] * n
        self.slot = [None] * int(slots)                # (request, attempt) decoding in the slot, None: free
        self.free_entries = list(range(int(slots)))
        self._head = 0                                 # requests below it want nothing any more

    def wants(self, r: int) -> bool:
        return (not self.decided[r] and self.in_flight[r] + self.accepted[r] < self.need[r]
                and (self.cap[r] is None or self.started[r] < self.cap[r]))

    def assign(self) -> List[PoolJob]:
        """Hand every free slot the next attempt of the earliest request that wants one (admit: the request's first
        attempt, its entry is taken here).  Returns the jobs in slot order."""
        jobs = []
        free = [b for b, occ in enumerate(self.slot) if occ is None]
        r = self._head
        for b in free:
            while r < len(self.need) and not self.wants(r):
                r += 1
            if r >= len(self.need) or (self.entry[r] is None and not self.free_entries):
                break                                  # (no entry free: cannot happen, see the class comment)
            admit = self.entry[r] is None
            if admit:
                self.entry[r] = self.free_entries.pop(0)
            a = self.started[r]
            self.started[r] += 1
            self.in_flight[r] += 1
            self.slot[b] = (r, a)
            jobs.append(PoolJob(b, r, a, self.entry[r], admit))
        while self._head < len(self.need) and self.decided[self._head]:
            self._head += 1
        return jobs

    def finish(self, slot: int, accepted: bool, payload=None):
        """The attempt in `slot` has ended and was accepted or not; the slot is free."""
        r, a = self.slot[slot]
        self.slot[slot] = None
        self.in_flight[r] -= 1
        self.accepted[r] += bool(accepted)
        self.results[r][a] = (bool(accepted), payload)

    def collect(self) -> List[int]:
        """The requests decided since the last call, in list order; their entries are freed (and reused)."""
        out = []
        for r in range(self._head, len(self.need)):
            if self.decided[r] or self.in_flight[r]:
                continue
            if self.accepted[r] >= self.need[r] or (self.cap[r] is not None and self.started[r] >= self.cap[r]):
                self.decided[r] = True
                if self.entry[r] is not None:
                    self.free_entries.append(self.entry[r])
                    self.entry[r] = None
                out.append(r)
            elif self.started[r] == 0:
                break                                  # (later requests have not been reached yet)
        return out

    def answer(self, r: int) -> list:
        """The payloads of request r's accepted attempts in attempt order."""
        return [p for _, (ok, p) in sorted(self.results[r].items()) if ok]

    def busy(self) -> bool:
        return any(occ is not None for occ in self.slot)

    def done(self) -> bool:
        return all(self.decided)


class BatchedGenerator:
    """Generates `len(input_datas)` sequences in parallel (per-sequence temperature / top_k / top_p, `num_measures` and
    `chord_token_components`).  Decoders (caches + captured graph) are kept per batch size: the sampling controls are
    device state of the decoder, so a new setting reuses the cache and the capture."""

    def __init__(self, model, device, generation_length=4096, memory_length=4146, sliding=False, kv_dtype="bf16",
                 shared_prompt=False):
        if kv_dtype not in DecodeState.KV_DTYPES:
            raise CommuHipError(f"kv_dtype: one of {DecodeState.KV_DTYPES} expected, got {kv_dtype!r}")
        # opt-in: requests whose sequences all continue ONE prompt hold its K/V once (ForcedDecoder(shared_prompt=True))
        self.shared_prompt = bool(shared_prompt)
        self.kv_dtype = kv_dtype         # "fp8": the opt-in e4m3 K/V cache of the decode step (DecodeState)
        self.model, self.device = model, device
        self.generation_length, self.memory_length = generation_length, memory_length
        self.sliding = bool(sliding)     # the reference's sliding memory window: generation_length may exceed memory_length
        self.uniform_sources = None      # optional list of callables, one per sequence (tests inject fixture variates)
        self.trace = None                # set to a list to receive per-sequence model-step traces
        self.use_graph = True
        self._decoders = {}

    def decoder(self, B, temperature, top_k, max_chords, top_p=1.0, per_slot: bool = False, max_prompt: int = 0,
                logit_bias=None, shared: bool = False, grammar=None, harmony=None, class_sampling=None, **rules):
        """The decoder for B slots, its slots set to the given controls (numbers or one value per slot).  per_slot: the
        caller will read log-probabilities or give slots their own controls later (rearm): the array launches from the
        start.  Otherwise one triple for all slots runs the scalar launches, until a second setting arrives for launches
        that are already captured (ForcedDecoder.__init__).  logit_bias: the request's constraint rows (one for all slots
        or one per slot; None clears what an earlier request left on this decoder).  grammar / harmony: the request's event
        grammar and harmony table (None switches off what an earlier request left).  class_sampling: the request's
        class-control table (None resets every slot to its base triple where an earlier request left one; a decoder that
        never had a table allocates nothing).  **rules: one keyword per rule of SLOT_RULES (note_order, voices, density,
        interval, onsets, guide, articulation, form) -- one value for all sequences or one per sequence, as the rule's
        setter ForcedDecoder.set_<keyword> takes them; None switches off what an earlier request left, and allocates nothing
        on a decoder that never had the rule.  shared: the decoder that holds the request's common prompt once (its own
        cache layout: kept beside the unshared decoder of the same size)."""
        rules = _rule_values(rules)
        rows = sampling_rows(B, temperature, top_k, top_p)          # (validated before anything is built)
        if logit_bias is not None:
            logit_bias = logit_bias_rows(logit_bias, B)
        gram_table, gram_rows = _grammar_request(grammar, B)
        harm_table = _harmony_request(harmony)
        cls_table = _class_request(class_sampling)
        vals = {RULE_OF[kw]: RULE_OF[kw].normalize(v, B) for kw, v in rules.items()}
        _articulation_needs_guide(vals[ARTICULATION], vals[GUIDE])
        _form_needs_grammar(vals[FORM], gram_rows)
        key = (B, self.trace is not None, self.sliding) + (("shared",) if shared else ())
        dec = self._decoders.get(key)
        if dec is None or dec.ld_chord < max_chords or dec.max_prompt < max_prompt:
            # (a decoder built for prompts serves requests without one: its buffers are only longer)
            dec = ForcedDecoder(self.model, B, self.generation_length, self.memory_length, float(rows[0][0]), int(rows[1][0]),
                                max_chords=max(64, max_chords), record_trace=self.trace is not None,
                                top_p=float(rows[2][0]), sliding=self.sliding, kv_dtype=self.kv_dtype,
                                max_prompt=max(max_prompt, 0 if dec is None else dec.max_prompt),
                                **({"shared_prompt": True} if shared else {}))
            self._decoders[key] = dec
        if per_slot:
            dec.record_logprobs()
        dec.set_sampling(*rows)
        dec.set_logit_bias(logit_bias)
        # (grammar: the request's event grammar; a request without one switches off what an earlier one left)
        dec.set_grammar(None)
        if gram_rows:
            dec.set_grammar(gram_table, rows=None if len(gram_rows) == B else gram_rows)
        # (harmony: likewise; None on a decoder that never had a table allocates nothing)
        dec.set_harmony(harm_table)
        # (class-keyed controls: likewise, after set_sampling -- the inherited entries are the slots' base triples)
        dec.set_class_sampling(cls_table)
        # (the rules of SLOT_RULES: likewise, in the table's order -- a first use fills the class records with the base
        # triples set above, and a rule comes after the one it implies, which it switches on where the request left it off)
        for r, v in vals.items():
            getattr(dec, r.setter)(v)
        return dec

    @staticmethod
    def _one_harmony(harmony):
        if harmony is not None and not isinstance(harmony, (bool, np.bool_)) and np.ndim(harmony) != 2:
            raise CommuHipError(f"harmony: one setting for the request expected (True or a table), got shape "
                                f"{np.shape(harmony)}")
        return harmony

    @torch.no_grad()
    def generate(self, encoded_metas: Sequence[Sequence[int]], input_datas, temperature, top_k, top_p=1.0,
                 return_logprobs: bool = False, prompts: Optional[Sequence[Sequence[int]]] = None, logit_bias=None,
                 grammar=None, harmony=None, class_sampling=None, note_order=None, voices=None, density=None,
                 interval=None, onsets=None, guide=None, articulation=None, form=None):
        """temperature / top_k / top_p: a number for the batch or one value per sequence.
        note_order / voices / density / interval / onsets / guide / articulation / form: the rules of SLOT_RULES, each None /
        False (off), one value for the batch or one per sequence (a list with one entry per sequence for guide,
        articulation and form) -- what such a sequence may DRAW, in full at the rule's setter ForcedDecoder.set_<keyword>;
        voices switches the sequence's note order on, density its voice word and note order, the others imply nothing;
        articulation's hold_guide needs the sequence's guide=, a form's "copy": "rhythm" its grammar=.
        class_sampling: None, a table
        (class_sampling()) or its arguments as a dict {"drawn": ..., "after": ...}, one setting for the request -- a triple
        per token class that replaces the sequence's own where the table says so (ForcedDecoder.set_class_sampling).  harmony: None, True (the strict
        default table: only chord tones) or a table (harmony_rows), one setting for the request -- every pitch a sequence
        DRAWS is weighed by the chord it is in (ForcedDecoder.set_harmony).  grammar: None, True (the default
        event grammar), a table (grammar_table) or one bool per sequence -- every token such a sequence DRAWS continues a
        group the token-to-MIDI step keeps (ForcedDecoder.set_grammar).  logit_bias: a constraint row
        (token_constraints) for the request or one per sequence -- what a sequence may DRAW; forced tokens and prompts are
        not affected (ForcedDecoder.set_logit_bias).  return_logprobs: a third return
        value, ForcedDecoder.logprobs() of the batch.  prompts: one token list per sequence (may be empty) that the
        sequence continues (ForcedDecoder.load): every returned sequence is [0] + meta + prompt + what was generated, and
        generation_length counts the iterations after the prompt."""
        rules = _rules_of(locals())
        B = len(input_datas)
        max_chords = max(len(d.chord_token_components["chord_token"]) for d in input_datas)
        if prompts is not None and len(prompts) != B:
            raise CommuHipError(f"prompts: one token list per sequence expected ({B}), got {len(prompts)}")
        max_prompt = 0 if prompts is None else max(len(p) for p in prompts)
        # (shared_prompt: requests with a prompt only -- without one there is nothing but the short context to share)
        dec = self.decoder(B, temperature, top_k, max_chords, top_p, per_slot=return_logprobs, max_prompt=max_prompt,
                           logit_bias=logit_bias, shared=self.shared_prompt and max_prompt > 0, grammar=grammar,
                           harmony=self._one_harmony(harmony), class_sampling=class_sampling, **rules)
        uniforms = None
        if bool((dec._sampling[0] != 0).any()) or dec.class_samples():
            srcs = self.uniform_sources or [np.random.RandomState(1000 + b).random_sample for b in range(B)]
            uniforms = np.array([[float(srcs[b]()) for _ in range(dec.ld_u)] for b in range(B)], dtype=np.float32)
        dec.load(encoded_metas, input_datas, uniforms, prompts=prompts)
        dec.run(use_graph=self.use_graph)
        seqs, traces = dec.sequences()
        if self.trace is not None:
            self.trace[:] = traces
        if return_logprobs:
            return seqs, dec.reports, dec.logprobs()
        return seqs, dec.reports

    @staticmethod
    def attempt_uniforms(seed: int, attempt: int, n: int) -> np.ndarray:
        """The variates of attempt number `attempt` of a request (its own stream: an attempt's sequence does not depend on
        which slot or how many other attempts ran beside it)."""
        return np.random.RandomState((seed + 7919 * attempt) % (2 ** 32)).random_sample(n).astype(np.float32)

    @torch.no_grad()
    def generate_stream(self, encoded_meta: Sequence[int], input_data, temperature, top_k, need: int,
                        accept, top_p=1.0, slots: int = 64, seed: int = 0, max_attempts: Optional[int] = None,
                        return_logprobs: bool = False, prompt: Optional[Sequence[int]] = None, logit_bias=None,
                        share_prompt: bool = False, grammar=None, harmony=None, class_sampling=None, note_order=None,
                        voices=None, density=None, interval=None, onsets=None, guide=None, articulation=None,
                        form=None):
        """Attempts of ONE request (the reference's `while idx != num_generate` loop, midi_inferrer.py:338-354, which tries
        one sequence after the other) decoded in up to `slots` parallel slots, CONTINUOUSLY: a slot whose sequence has
        ended is handed to `accept(sequence, report) -> bool` and re-armed with the next attempt while the other slots keep
        decoding -- the batch does not thin out towards the end of a round.  Returns (the first `need` accepted attempts IN
        ATTEMPT ORDER -- exactly what the reference's sequential loop would return for the same per-attempt variates,
        whatever the number of slots --, attempts started); fewer when `max_attempts` attempts did not yield `need`.
        Attempt a draws from attempt_uniforms(seed, a, .) whichever slot decodes it.
        temperature / top_k / top_p: a number, or a sequence indexed by ATTEMPT NUMBER modulo its length -- like its
        variates, the controls of attempt a do not depend on the slot that decodes it.  return_logprobs: a third return
        value, the log-probability arrays (ForcedDecoder.logprobs) of the returned attempts in the same order.
        prompt: a token list every attempt of the request continues (primed slots, ForcedDecoder.load; a re-armed slot
        returns to the primed state).
        logit_bias: one constraint row (token_constraints) for every attempt of the request.
        grammar: None, True (the default event grammar) or a table (grammar_table): one setting for the request.
        harmony: None, True (harmony_table(), strict) or a table (harmony_rows): one setting for the request.
        class_sampling: None, a table (class_sampling()) or {"drawn": ..., "after": ...}: one setting for the request; the
        entries it leaves open inherit the ATTEMPT's own triple (a re-armed slot recomposes them).
        note_order / voices / density / interval / onsets / guide / articulation / form: the rules of SLOT_RULES, each None /
        False or ONE setting for every attempt of the request, in the form the rule's setter ForcedDecoder.set_<keyword>
        takes for one slot (the state is read off a slot's seq and its forcing record, so a re-armed slot needs nothing; its
        replay state is reset with its record); articulation's hold_guide needs guide=, a form's "copy": "rhythm" grammar=.
        share_prompt (opt-in; also on with BatchedGenerator(shared_prompt=True) when a prompt is given): the K/V of the
        context and the prompt are computed and held once for all slots (ForcedDecoder(shared_prompt=True)); the attempts
        returned are the ones the unshared decoder defines, up to the summation order of the attention."""
        rules = _rules_of(locals())
        B = max(1, min(int(slots), int(need)))
        if share_prompt and not prompt:
            raise CommuHipError("share_prompt: there is no prompt to share (prompt= is empty)")
        share = bool(prompt) and (bool(share_prompt) or self.shared_prompt)
        if logit_bias is not None and np.ndim(logit_bias) != 1:
            raise CommuHipError(f"logit_bias: one row for the request expected, got shape {np.shape(logit_bias)}")
        if grammar is not None and not isinstance(grammar, (bool, np.bool_)) and np.ndim(grammar) != 2:
            raise CommuHipError(f"grammar: one setting for the request expected (True or a table), got shape "
                                f"{np.shape(grammar)}")
        harmony = self._one_harmony(harmony)
        rules = {kw: RULE_OF[kw].one(v) for kw, v in rules.items()}          # (ONE setting each, templates validated)
        max_chords = len(input_data.chord_token_components["chord_token"])
        # each control's schedule, validated on its own (the three may have different lengths)
        n_of = lambda x: 1 if np.ndim(x) == 0 else len(x)
        sched = (sampling_rows(n_of(temperature), temperature, 1, 1.0)[0], sampling_rows(n_of(top_k), 0.0, top_k, 1.0)[1],
                 sampling_rows(n_of(top_p), 0.0, 1, top_p)[2])

        def triple(a):
            return tuple(c[a % len(c)].item() for c in sched)
        first = [triple(a) for a in range(B)]
        varying = any(bool((c != c[0]).any()) for c in sched)          # (one triple for every attempt: nothing to re-arm)
        dec = self.decoder(B, [t[0] for t in first], [t[1] for t in first], max_chords, [t[2] for t in first],
                           per_slot=return_logprobs or varying, max_prompt=0 if prompt is None else len(prompt),
                           logit_bias=logit_bias, shared=share, grammar=grammar, harmony=harmony,
                           class_sampling=class_sampling, **rules)
        started = B
        sampled = bool((sched[0] != 0).any()) or dec.class_samples()          # (a greedy attempt reads no variate)
        uni = np.stack([self.attempt_uniforms(seed, a, dec.ld_u) for a in range(B)]) if sampled else None
        dec.load([list(encoded_meta)] * B, [input_data] * B, uni,
                 prompts=None if prompt is None else [list(prompt)] * B)
        if self.use_graph and dec.graph is None:
            dec.build_graph()
        dec.pre()
        slot_attempt = list(range(B))          # attempt number decoded in each slot; -1: slot retired
        results = {}                           # attempt -> its sequence if accepted, False if rejected
        logps = {}                             # (return_logprobs) accepted attempt -> its log-probability array
        n_ok, out = 0, None
        dec.run_iterations(dec.POLL, self.use_graph)
        kb, nlive = 0, None                    # bound of the memory lengths, live slots (from the polled records)
        while out is None and any(a >= 0 for a in slot_attempt):
            dec.poll_submit()                  # the records after the window just queued ...
            dec.run_iterations(dec.POLL, self.use_graph, klen_bound=kb, live_rows=nlive)      # ... are read while the next window runs
            fsm = dec.poll_result()
            kb = int(fsm[:, 0].max()) + 3 * dec.POLL - (dec.prefix_P if dec.shared_prompt else 0)      # (private rows)
            nlive = sum(1 for b_ in range(B) if slot_attempt[b_] >= 0 and not fsm[b_, 5]) + 1
            for b in range(B):
                a = slot_attempt[b]
                if a < 0 or not fsm[b, 5]:
                    continue
                seq = dec.harvest(b, fsm[b])
                ok = bool(accept(seq, dec.reports[b]))
                results[a] = seq if ok else False
                if ok and return_logprobs:
                    logps[a] = dec.harvest_logprobs(b, fsm[b])
                n_ok += ok
                # no further attempts once enough were accepted: only the lower-numbered ones still in flight can matter
                if n_ok >= need or (max_attempts is not None and started >= max_attempts):
                    slot_attempt[b] = -1
                    continue
                dec.rearm(b, self.attempt_uniforms(seed, started, dec.ld_u) if sampled else None,
                          sampling=triple(started) if varying else None)
                slot_attempt[b] = started
                started += 1
            # the answer: the first `need` accepted attempts IN ATTEMPT ORDER, known once every attempt before the last of
            # them has ended (taking them in order of completion instead would favour short sequences)
            got, a = [], 0
            while a in results and len(got) < need:
                if results[a] is not False:
                    got.append(a)
                a += 1
            if len(got) >= need:
                out = got
        if out is None:                        # max_attempts exhausted: whatever was accepted, in attempt order
            out = [a for a in sorted(results) if results[a] is not False][:need]
        out, out_lp = [results[a] for a in out], [logps.get(a) for a in out]
        try:
            dec.state.check()
        except CommuHipError:
            dec.state.tail_ok, dec.graph, dec.graph_long = False, None, None          # later requests on this decoder: per-Linear launches
            dec.state.t_err.zero_()
            raise
        if return_logprobs:
            return out, started, out_lp
        return out, started

    # ---- request pool: MANY requests decoded in one set of slots (generate_stream serves one; a request of a few
    # sequences leaves most of the slots the machine would carry at the same iteration time empty)
    def _check_pool(self, requests, slots, grammar, harmony):
        """generate_pool's refusals, before anything is allocated; returns (slots, n_cond)."""
        if isinstance(slots, bool) or not isinstance(slots, (int, np.integer)) or not 1 <= int(slots) <= 256:
            raise CommuHipError(f"generate_pool: slots in 1 .. 256 expected, got {slots!r}")
        requests = list(requests)
        if not requests:
            raise CommuHipError("generate_pool: an empty list of requests")
        if self.shared_prompt:
            raise CommuHipError("generate_pool: a generator built for ONE shared prompt (shared_prompt) is not served: the "
                                "shared prefix belongs to no slot; give each request its own (PoolRequest(prompt=))")
        if bool(getattr(self.model, "parity_fp32", False)):
            raise CommuHipError("generate_pool: the fp32 parity mode (model.parity_fp32) has a third cache layout that the "
                                "arm launch does not copy")
        n_cond = len(requests[0].encoded_meta)
        for i, r in enumerate(requests):
            if isinstance(r.need, bool) or not isinstance(r.need, (int, np.integer)) or r.need < 1:
                raise CommuHipError(f"generate_pool: request {i}: need >= 1 expected, got {r.need!r}")
            if len(r.encoded_meta) != n_cond:
                raise CommuHipError(f"generate_pool: request {i} has {len(r.encoded_meta)} conditioning tokens, request 0 "
                                    f"has {n_cond}: one length for the pool expected")
            if r.grammar and grammar is None:
                raise CommuHipError(f"generate_pool: request {i} switches the grammar on, but the pool has no grammar table "
                                    "(generate_pool(grammar=))")
            if r.harmony and harmony is None:
                raise CommuHipError(f"generate_pool: request {i} switches the harmony on, but the pool has no harmony table "
                                    "(generate_pool(harmony=))")
            if r.max_attempts is not None and r.max_attempts < 0:
                raise CommuHipError(f"generate_pool: request {i}: max_attempts >= 0 expected, got {r.max_attempts!r}")
            if r.logit_bias is not None and np.ndim(r.logit_bias) != 1:
                raise CommuHipError(f"generate_pool: request {i}: logit_bias: one row expected, got shape "
                                    f"{np.shape(r.logit_bias)}")
        if n_cond < 1 or n_cond > 15:
            raise CommuHipError(f"generate_pool: 1 .. 15 conditioning tokens expected, got {n_cond}")
        if self.sliding and int(self.memory_length) < n_cond:
            raise CommuHipError(f"generate_pool: a sliding window of {self.memory_length} positions is shorter than the "
                                f"context of {n_cond} tokens")
        return int(slots), n_cond

    @staticmethod
    def _pool_prompts(requests):
        """Every request's prompt as a list of ints (None / [] -> []), its tokens checked against the vocabulary, host only;
        returns (prompts, the longest one's length)."""
        V = TOKEN_OFFSET.VOCAB_SIZE
        prompts = []
        for i, r in enumerate(requests):
            try:
                p = [] if r.prompt is None else [int(t) for t in r.prompt]
            except (TypeError, ValueError):
                raise CommuHipError(f"generate_pool: request {i}: prompt: a list of token ids expected, got "
                                    f"{r.prompt!r}") from None
            bad = next((j for j, t in enumerate(p) if t < 0 or t >= V), None)
            if bad is not None:
                raise CommuHipError(f"generate_pool: request {i}: prompt token {p[bad]} at index {bad} is outside [0, {V})")
            prompts.append(p)
        return prompts, max(len(p) for p in prompts)

    @torch.no_grad()
    def generate_pool(self, requests, slots: int = 64, grammar=None, harmony=None, class_sampling=None,
                      return_logprobs: bool = False, on_result=None):
        """MANY requests (PoolRequest) decoded in ONE decoder of B = min(slots, sum of need) slots: generate_stream's loop
        -- the iteration graph built once, POLL iterations queued ahead, the records polled through the pinned copy,
        finished slots harvested and handed to their request's accept -- in which a free slot takes the next attempt of
        the earliest request that still wants one (PoolSchedule) and all slots that became free in a window are armed by
        ONE launch (ForcedDecoder.arm).  Returns one PoolResult(sequences, attempts_started, logprobs) per request in
        request order; on_result(index, result) is called as each request is decided.
        CONTRACT: a request gets what generate_stream(..., slots=1) returns for it alone -- the same sequences, token for
        token, and the same number of attempts started --, whatever else is in the pool and whichever slots decode it:
        attempt a of a request draws from attempt_uniforms(request.seed, a, .), its conditioning K/V come from a forward
        over its own single column (ForcedDecoder.admit), and the decode step computes every slot on its own.  (Beyond
        512 keys per slot the split-key policy chooses the attention's summation order from the number of live rows, as
        it does for generate_stream.)
        grammar / harmony / class_sampling: ONE table each for the pool (generate_stream's values); a request switches
        grammar and harmony per request, the class table applies to every request over its own base triple.
        Refused, before anything is allocated: slots outside 1 .. 256, an empty list, need < 1, metas of different
        lengths, a per-request switch without a pool table, a shared-prompt generator, model.parity_fp32, a sliding window
        shorter than the context, a prompt token outside [0, 729).
        PROMPTS: a request with prompt= continues its own prompt, as generate_stream(prompt=) does for it alone.  A pool
        without prompts is the pool it always was (same decoder, same store of n_ctx_max image rows, commu_decode_arm).  A
        pool with at least one prompt gets a decoder of its own built with max_prompt = the longest prompt; every prompt
        is replayed (ForcedDecoder.pool_replay) and refused BEFORE the pool is opened -- a token outside [0, 729), a
        prompt that leaves the rules (request index, token, index, reason), on a linear cache klen0 + generation_length
        + 1 > Lmax --; its store holds pool_image_rows() rows per entry (pool_stats["store_bytes"]: B entries of that
        many rows, all layers and heads, in the cache's format) and its slots are armed by commu_decode_arm_primed.
        self.pool_stats holds the run's book-keeping: attempts rejected, the job count of every arm launch, how often a
        slot was armed with another request than it held before, admissions, the arm launch's entry point ("kernel"), the
        store's image rows and bytes, the longest memory a request starts with ("klen0_max")."""
        requests = list(requests)
        slots, n_cond = self._check_pool(requests, slots, grammar, harmony)
        prompts, max_prompt = self._pool_prompts(requests)
        if grammar is not None and not isinstance(grammar, (bool, np.bool_)) and np.ndim(grammar) != 2:
            raise CommuHipError(f"grammar: one setting for the pool expected (True or a table), got shape {np.shape(grammar)}")
        gram_table = None if grammar is None or grammar is False else (event_grammar() if grammar is True
                                                                        else grammar_table(grammar))
        harm_table = _harmony_request(self._one_harmony(harmony))
        cls_table = _class_request(class_sampling)
        # each request's controls, validated before anything is built
        # (a rule's value per request: the word of a rule without a table, else the template or None; the refusals of the
        # rules whose value may be a list name the request)
        triples, biases, vals = [], [], {rule: [] for rule in SLOT_RULES}
        for i, q in enumerate(requests):
            t, k, p = sampling_rows(1, q.temperature, q.top_k, q.top_p)
            triples.append((t[0].item(), int(k[0]), p[0].item()))
            biases.append(None if q.logit_bias is None else logit_bias_rows(q.logit_bias, 1)[0])
            gram_on = (gram_table is not None) if q.grammar is None else bool(q.grammar)
            for rule in SLOT_RULES:
                try:
                    v = getattr(q, rule.kw)
                    vals[rule].append(rule.one(v) if rule.rows_max else int(rule.normalize(v, 1)[0]))
                except CommuHipError as e:
                    if not rule.lists:
                        raise
                    raise CommuHipError(f"request {i}: {e}") from None
            try:
                _articulation_needs_guide(vals[ARTICULATION][-1:], vals[GUIDE][-1:])
                _form_needs_grammar(vals[FORM][-1:], [0] if gram_on else [])
            except CommuHipError as e:
                raise CommuHipError(f"request {i}: {e}") from None
        B = max(1, min(slots, sum(int(r.need) for r in requests)))
        max_chords = max(len(r.input_data.chord_token_components["chord_token"]) for r in requests)
        key = ("pool", B, self.trace is not None, self.sliding)          # (never shared with generate / generate_stream:
        #                                                                    arm() writes the slots' controls on the device only)
        if max_prompt > 0:
            key += ("primed",)          # a pool with prompts: a decoder of its own (longer store images, the primed arm launch)
        dec = self._decoders.get(key)
        if dec is None or dec.ld_chord < max_chords or dec.max_prompt < max_prompt:
            primed_kw = {} if max_prompt == 0 else {"max_prompt": max(max_prompt, 0 if dec is None else dec.max_prompt)}
            dec = ForcedDecoder(self.model, B, self.generation_length, self.memory_length, 1.0, 1,
                                max_chords=max(64, max_chords), record_trace=self.trace is not None, sliding=self.sliding,
                                kv_dtype=self.kv_dtype, **primed_kw)
            self._decoders[key] = dec
        # every prompt replayed and checked before the pool is opened: no store is allocated and nothing is decoded for a
        # list that holds a prompt the rules could not have produced or the cache cannot take
        replays = [None] * len(requests)
        if max_prompt > 0:
            replays = dec.pool_replay([r.encoded_meta for r in requests], [r.input_data for r in requests], prompts)
        # the pool's tables and whatever per-slot arrays its requests need (first use allocates, later pools reuse)
        dec.set_grammar(None)
        if gram_table is not None:
            dec.set_grammar(gram_table)
        dec.set_harmony(harm_table)
        # (one first use, of the highest tier any request needs; the requests' templates go into the tables before the pool
        # is opened: admit finds them by their bytes.  A table rule's kernel reads the tables below it, so every table up
        # to the highest one in use is packed anew -- articulation makes the guide's and the onsets' exist)
        used = {rule for rule in SLOT_RULES if any(rule.is_on(v) for v in vals[rule])}
        dec._first_use(pool_tier({rule.kw for rule in used}, cls_table is not None))
        top = max([rule.tier for rule in used if rule.rows_max] + [T_NONE])
        for rule in SAMPLING_RULES:
            if rule.rows_max and rule.tier <= top:
                dec._pack(rule, vals[rule], fresh=True)
        if any(b is not None for b in biases):
            dec._first_use(bias=True)
        # (the form rule: the requests' forms go into its table before the pool is opened; a later pool without one switches
        # every slot off, and a decoder that never had one allocates nothing)
        dec.set_form(None)
        if FORM in used:
            dec._first_use_form()
            dec._pack(FORM, vals[FORM], fresh=True, label="request")
        klen0_max = max([n_cond] + [p["klen0"] for p in replays if p is not None])
        dec.pool_open(n_cond, grid_rows=klen0_max)
        cls_samples = cls_table is not None and bool((np.nan_to_num(cls_table[..., 0], nan=0.0) != 0).any())
        sched = PoolSchedule([r.need for r in requests], [r.max_attempts for r in requests], B)
        stats = {"rejected": 0, "arms": [], "rearmed_other_request": 0, "admissions": 0, "kernel": dec.arm_kernel,
                 "image_rows": dec.pool_image_rows(), "store_bytes": dec.pool_store_bytes(), "klen0_max": klen0_max,
                 "form_src_tokens": dec._form_src_used}         # (ints of the take buffer in use: shared takes count once)
        self.pool_stats = stats
        held = [None] * B                                # the request each slot decoded last

        def arm_free():
            jobs = sched.assign()
            staged = []
            for j in jobs:
                r = requests[j.request]
                if j.admit:
                    stats["admissions"] += 1
                    dec.admit(j.entry, r.encoded_meta, r.input_data, sampling=triples[j.request],
                              logit_bias=biases[j.request],
                              grammar=(gram_table is not None) if r.grammar is None else bool(r.grammar),
                              harmony=(harm_table is not None) if r.harmony is None else bool(r.harmony),
                              class_table=cls_table, primed=replays[j.request],
                              **{rule.kw: v[j.request] for rule, v in vals.items()})
                sampled = triples[j.request][0] != 0 or cls_samples          # (a greedy attempt reads no variate)
                staged.append((j.slot, j.entry, self.attempt_uniforms(r.seed, j.attempt, dec.ld_u) if sampled else None))
                if held[j.slot] is not None and held[j.slot] != j.request:
                    stats["rearmed_other_request"] += 1
                held[j.slot] = j.request
            if staged:
                stats["arms"].append(len(staged))
                dec.arm(staged)

        results = [None] * len(requests)

        def decide():
            for r in sched.collect():
                got = sched.answer(r)
                results[r] = PoolResult([g[0] for g in got], sched.started[r],
                                        [g[1] for g in got] if return_logprobs else None)
                if on_result is not None:
                    on_result(r, results[r])

        decide()                                         # (requests with max_attempts = 0)
        arm_free()
        if self.use_graph and dec.graph is None:
            dec.build_graph()
        dec.pre()
        dec.run_iterations(dec.POLL, self.use_graph)
        kb, nlive = 0, None
        while sched.busy():
            dec.poll_submit()
            dec.run_iterations(dec.POLL, self.use_graph, klen_bound=kb, live_rows=nlive)
            fsm = dec.poll_result()
            kb = int(fsm[:, 0].max()) + 3 * dec.POLL
            nlive = sum(1 for b in range(B) if sched.slot[b] is not None and not fsm[b, 5]) + 1
            fin = [b for b in range(B) if sched.slot[b] is not None and fsm[b, 5]]
            if fin:
                # the finished slots' rows in ONE download (a finished slot's rows no longer change)
                idx = torch.tensor(fin, dtype=torch.long, device=dec.dev)
                n = int(fsm[fin, 0].max())
                rows = dec.seq.index_select(0, idx)[:, :n].cpu().numpy()
                lps = dec.seq_logp.index_select(0, idx)[:, :n].cpu().numpy() if return_logprobs else None
                for i, b in enumerate(fin):
                    r, _ = sched.slot[b]
                    dec.reports[b].consumed = int(fsm[b, 10])
                    ln = int(fsm[b, 0])
                    seq = None if fsm[b, 6] else rows[i, :ln].tolist()
                    acc = requests[r].accept
                    ok = (seq is not None) if acc is None else bool(acc(seq, dec.reports[b]))
                    stats["rejected"] += not ok
                    lp = lps[i, :ln].copy() if (ok and return_logprobs and seq is not None) else None
                    sched.finish(b, ok, (seq, lp))
                decide()
                arm_free()
        decide()
        try:
            dec.state.check()
        except CommuHipError:
            dec.state.tail_ok, dec.graph, dec.graph_long = False, None, None          # later pools on this decoder: per-Linear launches
            dec.state.t_err.zero_()
            raise
        return results
