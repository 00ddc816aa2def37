"""Decode loop of the hot path behind the reference's task API (commu/midi_generator/midi_inferrer.py).

The reference generates one sequence at a time with a Python loop around `forward_generate`, a sampling step
and the chord-forcing checks of `TeacherForceTask` (:16-169, :239-320).  Here the loop runs on the device for
all requested sequences at once (commu_amd.generate.ForcedDecoder: K/V-cache decode step, sampling kernel and the
forcing rules as two state-transition kernels, one hipGraph replay per iteration).  This module keeps what the
callers of the reference touch:

  * `TOKEN_OFFSET`            -- the token ranges the rules are written in (event_tokens.py:308-329)
  * `ForcingReport`           -- the outcome of the forcing for one sequence + the reference's structural check
                                 `validate_teacher_forced_sequence` (:146-169)
  * `InferenceTask`           -- `__call__(model, input_data, inference_cfg)` / `execute(encoded_meta)` (:172-184,
                                 :338-354) and `validate_generated_sequence` (:322-336)
"""
from __future__ import annotations

import json
import math
from typing import List, Optional

import torch


class TOKEN_OFFSET:
    """commu/preprocessor/encoder/event_tokens.py:308-329 (values only)."""
    EOS = 1
    BAR = 2
    PITCH = 3
    NOTE_VELOCITY = 131
    CHORD_START = 195
    CHORD_END = 303
    NOTE_DURATION = 304
    POSITION = 432
    BPM = 560
    VOCAB_SIZE = 729


DEFAULT_POSITION_RESOLUTION = 128      # commu/preprocessor/utils/constants.py:25

# token classes of one note event, in sequence order: POSITION, VELOCITY, PITCH, DURATION (sequence_postprocessor.py:34-46)
_NOTE_PATTERN = ((TOKEN_OFFSET.POSITION, TOKEN_OFFSET.BPM), (TOKEN_OFFSET.NOTE_VELOCITY, TOKEN_OFFSET.CHORD_START),
                 (TOKEN_OFFSET.PITCH, TOKEN_OFFSET.NOTE_VELOCITY), (TOKEN_OFFSET.NOTE_DURATION, TOKEN_OFFSET.POSITION))


def count_notes(seq: List[int]) -> int:
    """Number of well-formed note events: a velocity token preceded by a position and followed by pitch, duration
    (the scan of validate_generated_sequence, :322-336, which stops two tokens before the end)."""
    n = 0
    for i in range(1, len(seq) - 2):
        window = (seq[i - 1], seq[i], seq[i + 1], seq[i + 2])
        if all(lo <= t < hi for t, (lo, hi) in zip(window, _NOTE_PATTERN)):
            n += 1
    return n


# ---- the event grammar (generate.event_grammar, csrc/decode_loop.h: token_class): token classes by id
CLASS_OTHER, CLASS_BAR, CLASS_PITCH, CLASS_VELOCITY, CLASS_CHORD, CLASS_DURATION, CLASS_POSITION = range(7)


def token_class(t: int) -> int:
    """The class of a token id: OTHER (pad 0, EOS 1, ids >= 560: meta, bpm, ...; anything outside the vocabulary), BAR,
    PITCH, VELOCITY, CHORD, DURATION, POSITION."""
    t = int(t)
    if t < TOKEN_OFFSET.BAR or t >= TOKEN_OFFSET.BPM:
        return CLASS_OTHER
    if t < TOKEN_OFFSET.PITCH:
        return CLASS_BAR
    if t < TOKEN_OFFSET.NOTE_VELOCITY:
        return CLASS_PITCH
    if t < TOKEN_OFFSET.CHORD_START:
        return CLASS_VELOCITY
    if t < TOKEN_OFFSET.NOTE_DURATION:
        return CLASS_CHORD
    if t < TOKEN_OFFSET.POSITION:
        return CLASS_DURATION
    return CLASS_POSITION


def parse_events(seq: List[int], start: int) -> Optional[int]:
    """Whether seq[start:] is a chain of the groups the reference's token-to-MIDI step keeps
    (commu/preprocessor/encoder/encoder_utils.py:385-419; everything else it drops silently): BAR | EOS (the last token) |
    POSITION, CHORD | POSITION, VELOCITY, PITCH, DURATION.  Returns the index of the first token that does not continue a
    group, None when there is none.  A note group cut short by the end of the sequence (the iteration cap) is well formed;
    a sequence that ends in EOS has no such group, since EOS does not continue one."""
    state = 0          # 0: at a group boundary; 1 / 2 / 3: after a position / velocity / pitch; 4: after EOS
    for i in range(max(int(start), 0), len(seq)):
        t = int(seq[i])
        c = token_class(t)
        if state == 4:
            return i                                    # nothing follows EOS
        if state == 0:
            if c == CLASS_POSITION:
                state = 1
            elif t == TOKEN_OFFSET.EOS:
                state = 4
            elif c != CLASS_BAR:
                return i
        elif state == 1:
            if c == CLASS_CHORD:
                state = 0
            elif c == CLASS_VELOCITY:
                state = 2
            else:
                return i
        elif state == 2:
            if c != CLASS_PITCH:
                return i
            state = 3
        else:
            if c != CLASS_DURATION:
                return i
            state = 0
    return None


def note_order_bans(seq: List[int], max_notes: int = 0) -> set:
    """The ids the note-order constraint (ForcedDecoder.set_note_order, csrc/decode_loop.h: NoteOrder) bans for the token
    that follows seq.  With j the last BAR or POSITION token of seq: nothing when there is none or it is BAR; else, p that
    position and the run everything since the last BAR or other position before j: the positions before p, the pitches in
    the run and -- max_notes >= 1 -- p itself once the run holds max_notes pitches."""
    pos_lo, pos_hi = TOKEN_OFFSET.POSITION, TOKEN_OFFSET.BPM
    is_breaker = lambda t: t == TOKEN_OFFSET.BAR or pos_lo <= t < pos_hi
    j = next((i for i in range(len(seq) - 1, -1, -1) if is_breaker(int(seq[i]))), None)
    if j is None or int(seq[j]) == TOKEN_OFFSET.BAR:
        return set()
    p = int(seq[j])
    s = next((i + 1 for i in range(j - 1, -1, -1) if is_breaker(int(seq[i])) and int(seq[i]) != p), 0)
    pitches = [int(t) for t in seq[s:] if TOKEN_OFFSET.PITCH <= int(t) < TOKEN_OFFSET.NOTE_VELOCITY]
    banned = set(range(pos_lo, p)) | set(pitches)
    if max_notes >= 1 and len(pitches) >= max_notes:
        banned.add(p)
    return banned


def note_order_violation(seq: List[int], start: int, max_notes: int = 0) -> Optional[int]:
    """The index of the first token seq[i], i >= start, that the note-order constraint would have banned given seq[:i]
    (note_order_bans): a position that steps back inside its bar, a pitch doubled at one position, or -- max_notes >= 1 --
    a position repeated once it holds max_notes notes.  None when there is none."""
    for i in range(max(int(start), 0), len(seq)):
        if int(seq[i]) in note_order_bans(seq[:i], max_notes):
            return i
    return None


def _grid_notes(seq: List[int]):
    """(start, length, pitch, bars after it) of every Position, Velocity, Pitch, Duration group of seq -- the groups the
    reference's token-to-MIDI step turns into notes (encoder_utils.py:399-404) -- on the 128-step grid of their own bar."""
    T = TOKEN_OFFSET
    seq = [int(t) for t in seq]
    bars_after = [0] * (len(seq) + 1)
    for i in range(len(seq) - 1, -1, -1):
        bars_after[i] = bars_after[i + 1] + (seq[i] == T.BAR)
    out = []
    for i in range(len(seq) - 3):
        if T.POSITION <= seq[i] < T.BPM and T.NOTE_VELOCITY <= seq[i + 1] < T.CHORD_START \
                and T.PITCH <= seq[i + 2] < T.NOTE_VELOCITY and T.NOTE_DURATION <= seq[i + 3] < T.POSITION:
            out.append((seq[i] - T.POSITION, seq[i + 3] - T.NOTE_DURATION + 1, seq[i + 2], bars_after[i + 4]))
    return out


def voice_bans(seq: List[int], word: int) -> set:
    """The ids the voice cap (ForcedDecoder.set_voices, csrc/decode_loop.h: Voices) bans for the token that follows seq.
    word: -1 off, else N + 256 r.  A note of the current bar or the one before ends at e = min(start + length - 128 * (bars
    after it), 128) on the current bar's grid.  N >= 1: the positions before the N-th largest end are banned (at every one
    of them N notes still sound).  r = 1: the pitch of every note that ends past the onset seq is at (0 after a BAR)."""
    word = int(word)
    if word < 0:
        return set()
    cap, strike = word & 255, (word >> 8) & 1
    ends = [(min(a + d - 128 * k, 128), p) for a, d, p, k in _grid_notes(seq) if k <= 1]
    banned = set()
    if cap >= 1 and len(ends) >= cap:
        banned |= set(range(TOKEN_OFFSET.POSITION, TOKEN_OFFSET.POSITION + max(sorted(e for e, _ in ends)[-cap], 0)))
    if strike:
        at = next((int(t) for t in reversed(seq)
                   if int(t) == TOKEN_OFFSET.BAR or TOKEN_OFFSET.POSITION <= int(t) < TOKEN_OFFSET.BPM), None)
        if at is not None:
            g0 = 0 if at == TOKEN_OFFSET.BAR else at - TOKEN_OFFSET.POSITION
            banned |= {p for e, p in ends if e > g0}
    return banned


def voices_violation(seq: List[int], start: int, max_voices: int = 0, restrike: bool = True) -> Optional[int]:
    """The index of the first token seq[i], i >= start, that the voice cap would have banned given seq[:i] (voice_bans with
    N = max_voices, 0: no cap, and r = restrike): a position at which max_voices notes still sound, or a pitch struck while
    it sounds.  A banned position that a chord token follows is none: a Position, Chord group starts no note (the rules
    force `Position 432, Chord` behind a bar whatever still sounds).  None when there is none."""
    word = int(max_voices) + 256 * int(bool(restrike))
    for i in range(max(int(start), 0), len(seq)):
        if int(seq[i]) in voice_bans(seq[:i], word):
            chord_group = TOKEN_OFFSET.POSITION <= int(seq[i]) < TOKEN_OFFSET.BPM and i + 1 < len(seq) \
                and TOKEN_OFFSET.CHORD_START <= int(seq[i + 1]) <= TOKEN_OFFSET.CHORD_END
            if not chord_group:
                return i
    return None


def interval_bans(seq: List[int], word: int) -> set:
    """The ids the melodic interval (ForcedDecoder.set_interval, csrc/decode_loop.h: Interval) bans for the token that
    follows seq.  word: -1 off, else up + 256 down + 65536 u.  The reference is the last note of seq that at most one BAR
    follows, q its pitch token; none: nothing.  up >= 1: the pitches more than up semitones above q; down >= 1: those more
    than down below it; u = 1: q itself."""
    word = int(word)
    if word < 0:
        return set()
    up, down, unison = word & 255, (word >> 8) & 255, (word >> 16) & 1
    near = [p for _, _, p, k in _grid_notes(seq) if k <= 1]
    if not near:
        return set()
    q = near[-1]
    banned = set()
    if up >= 1:
        banned |= set(range(q + up + 1, TOKEN_OFFSET.NOTE_VELOCITY))
    if down >= 1:
        banned |= set(range(TOKEN_OFFSET.PITCH, q - down))
    if unison:
        banned.add(q)
    return banned


def interval_violation(seq: List[int], start: int, up: int = 0, down: int = 0, no_repeat: bool = False,
                       drawn=None) -> Optional[int]:
    """The index of the first token seq[i], i >= start, that the melodic interval would have banned given seq[:i]
    (interval_bans with the word of up, down and no_repeat): a pitch more than up semitones above or down below the pitch of
    the note before it, or -- no_repeat -- that pitch again.  drawn: a mask over seq; only the tokens it marks count (a
    forced token and a prompt are not the rule's).  None when there is none."""
    word = int(up) + 256 * int(down) + 65536 * int(bool(no_repeat))
    for i in range(max(int(start), 0), len(seq)):
        if drawn is not None and not drawn[i]:
            continue
        if TOKEN_OFFSET.PITCH <= int(seq[i]) < TOKEN_OFFSET.NOTE_VELOCITY and int(seq[i]) in interval_bans(seq[:i], word):
            return i
    return None


def max_sounding(seq: List[int], ticks_per_bar: int, start: int = 0):
    """(most notes sounding at one tick, whether a pitch is struck while it sounds) for the notes of seq that begin at
    index >= start, in TICKS as the reference's decoder places them (encoder_utils.py:433-442, encoder.py:79-88): onset q of
    bar k at k * ticks_per_bar + floor(q * ticks_per_bar / 128), a length of d steps d * int(ticks_per_bar / 128) ticks.  A
    note sounds on [on, off); notes that begin before `start` sound too but are not counted against each other."""
    T = TOKEN_OFFSET
    seq = [int(t) for t in seq]
    unit = int(ticks_per_bar / 128)
    notes, bar = [], 0          # (every Bar opens the next bar; only the notes' distances matter)
    for i, t in enumerate(seq):
        if t == T.BAR:
            bar += 1
        if i + 3 < len(seq) and T.POSITION <= t < T.BPM and T.NOTE_VELOCITY <= seq[i + 1] < T.CHORD_START \
                and T.PITCH <= seq[i + 2] < T.NOTE_VELOCITY and T.NOTE_DURATION <= seq[i + 3] < T.POSITION:
            on = bar * int(ticks_per_bar) + ((t - T.POSITION) * int(ticks_per_bar)) // 128
            notes.append((on, on + (seq[i + 3] - T.NOTE_DURATION + 1) * unit, seq[i + 2], i >= start))
    most, struck = 0, False
    for k, (on, off, pitch, drawn) in enumerate(notes):
        if not drawn:
            continue
        # (the note order makes onsets non-decreasing: every note that sounds when this one starts came before it)
        live = [(o, f, p) for o, f, p, _ in notes[:k] if o <= on < f]
        most = max(most, 1 + len(live))
        struck = struck or any(p == pitch for _, _, p in live)
    return most, struck


class ForcingReport:
    """What the forcing state machine was asked to place in one sequence and how far it got."""

    def __init__(self, n_chords: int, num_measures: float):
        self.n_chords, self.num_measures = n_chords, num_measures
        self.length_fit = n_chords == int(num_measures // 4 * 4)          # :48-52 (one chord per bar)
        self.consumed = 0                                                   # chords handed to the sequence

    def validate_teacher_forced_sequence(self, seq: List[int]) -> None:    # :146-169
        bars = seq.count(TOKEN_OFFSET.BAR)
        chords = sum(1 for t in seq if TOKEN_OFFSET.CHORD_START <= t <= TOKEN_OFFSET.CHORD_END)
        if self.consumed != self.n_chords:
            raise Exception(f"remnant chord length: {self.n_chords - self.consumed} \nerror in teacher forcing")
        if bars != int(math.ceil(self.num_measures)):
            raise Exception(f"bar length: {bars} \nerror in bar length")
        if chords != self.n_chords:
            raise Exception(f"num_chord: {chords} vs {self.n_chords} \nerror in chord length")


class InferenceTask:
    """midi_inferrer.py:172-354.  `execute` returns `input_data.num_generate` sequences that passed both of the
    reference's validators; rejected attempts are retried like the reference does (in parallel rounds)."""

    def __init__(self, device: torch.device):
        self.device = device
        self.uniform_seed = 0
        self.attempts = 0

    def __call__(self, model, input_data, inference_cfg):
        self.model = model
        self.input_data = input_data
        self.inference_cfg = inference_cfg

    def validate_generated_sequence(self, seq: List[int]) -> bool:                           # :322-336
        return count_notes(seq) > 0

    def execute(self, encoded_meta, max_rounds: Optional[int] = None, return_logprobs: bool = False,
                prompt: Optional[List[int]] = None, logit_bias=None, grammar=None, harmony=None,
                class_sampling=None, note_order=None, voices=None, density=None, interval=None,
                onsets=None, guide=None, articulation=None, form=None):                                    # :338-354
        """return_logprobs (not in the reference): (sequences, their log-probability arrays -- ForcedDecoder.logprobs).
        prompt (not in the reference): token ids that follow the meta tokens; every attempt continues them (primed
        generation, BatchedGenerator.generate_stream) and every returned sequence starts with [0] + meta + prompt.
        logit_bias (not in the reference): a constraint row (generate.token_constraints) on what every attempt may draw.
        grammar (not in the reference): True or a table (generate.grammar_table) -- every drawn token continues a group the
        token-to-MIDI step keeps (generate.event_grammar, BatchedGenerator.generate_stream).
        harmony (not in the reference): True (only chord tones) or a table (generate.harmony_rows) -- every drawn pitch is
        weighed by the chord that is sounding (generate.harmony_table, ForcedDecoder.set_harmony).
        class_sampling (not in the reference): a table (generate.class_sampling) or its arguments as a dict -- a
        temperature / top_k / top_p per token class (ForcedDecoder.set_class_sampling).
        note_order (not in the reference): True or a cap of 1 .. 128 notes per position -- inside a bar the drawn
        positions never go back and no pitch is drawn twice at one position (ForcedDecoder.set_note_order).
        voices (not in the reference): a word generate.voices_word(N, r) -- at most N drawn notes sound at once and (r) no
        pitch is struck while it sounds; switches the note order on (ForcedDecoder.set_voices).
        density (not in the reference): a word generate.density_word(lo, hi) -- a drawn bar holds at least lo and at most hi
        notes; switches the voice word and the note order on (ForcedDecoder.set_density).
        interval (not in the reference): a word generate.interval_word(up, down, no_repeat) -- a drawn pitch lies at most up
        semitones above and down below the pitch of the note before it; switches nothing else on
        (ForcedDecoder.set_interval).
        onsets (not in the reference): a template in any form generate.onset_rows takes -- a drawn position lies where the
        row of its bar has a bit, bar i using row i mod R; switches nothing else on (ForcedDecoder.set_onsets).
        guide (not in the reference): a guide track in any form generate.guide_template takes -- a drawn pitch lies where the
        guide's cell for the position its bar is at has a bit; switches nothing else on (ForcedDecoder.set_guide).
        articulation (not in the reference): an articulation in any form generate.articulation_template takes -- a drawn
        duration lies in the window of its bar's row, capped at the bar line (within_bar) and where the guide bans the held
        pitch (hold_guide), a drawn velocity where the row has a bit; switches nothing else on
        (ForcedDecoder.set_articulation).
        form (not in the reference): a form in any form generate.form_template takes -- a bar the loop opens itself replays
        the earlier bar its row names, in full (optionally transposed) or its rhythm only; "copy": "rhythm" needs the
        grammar (ForcedDecoder.set_form)."""
        from ..generate import BatchedGenerator
        data = self.input_data
        glen = self.inference_cfg.GENERATION.generation_length
        mlen = getattr(self.inference_cfg.MODEL, "memory_length", 4146) if hasattr(self.inference_cfg, "MODEL") else 4146
        # (not a key of the reference's configuration: set by generate.py --sliding_memory)
        sliding = bool(getattr(self.inference_cfg.GENERATION, "sliding_memory", False))
        # (likewise: generate.py --kv_cache)
        kv_dtype = str(getattr(self.inference_cfg.GENERATION, "kv_cache", "bf16"))
        # (likewise: generate.py --share_prompt; it takes effect for requests with a prompt)
        share = bool(getattr(self.inference_cfg.GENERATION, "share_prompt", False))
        # (likewise: generate.py --decode_slots)
        slots = int(getattr(self.inference_cfg.GENERATION, "decode_slots", 64))
        # (likewise: generate.py --grammar; an argument given here wins)
        if grammar is None and bool(getattr(self.inference_cfg.GENERATION, "grammar", False)):
            grammar = True
        # (likewise: generate.py --class_sampling, the JSON text of its document; an argument given here wins)
        if class_sampling is None and getattr(self.inference_cfg.GENERATION, "class_sampling", None):
            from ..generate import read_class_sampling
            class_sampling = read_class_sampling(json.loads(self.inference_cfg.GENERATION.class_sampling))[0]
        # (likewise: generate.py --note_order / --max_notes, the control word; an argument given here wins)
        if note_order is None and getattr(self.inference_cfg.GENERATION, "note_order", None) is not None:
            note_order = int(self.inference_cfg.GENERATION.note_order)
        # (likewise: generate.py --max_voices / --no_restrike, the voice word)
        if voices is None and getattr(self.inference_cfg.GENERATION, "voices", None) is not None:
            voices = int(self.inference_cfg.GENERATION.voices)
        # (likewise: generate.py --min_notes_per_bar / --max_notes_per_bar, the density word)
        if density is None and getattr(self.inference_cfg.GENERATION, "density", None) is not None:
            density = int(self.inference_cfg.GENERATION.density)
        # (likewise: generate.py --max_leap / --max_leap_up / --max_leap_down / --no_repeat_pitch, the interval word)
        if interval is None and getattr(self.inference_cfg.GENERATION, "interval", None) is not None:
            interval = int(self.inference_cfg.GENERATION.interval)
        # (likewise: generate.py --onsets, the JSON text of the template's bars)
        if onsets is None and getattr(self.inference_cfg.GENERATION, "onsets", None):
            onsets = json.loads(self.inference_cfg.GENERATION.onsets)
        # (likewise: generate.py --guide, the JSON text of the guide's raw form)
        if guide is None and getattr(self.inference_cfg.GENERATION, "guide", None):
            guide = json.loads(self.inference_cfg.GENERATION.guide)
        # (likewise: generate.py --articulation, the JSON text of the articulation's full form)
        if articulation is None and getattr(self.inference_cfg.GENERATION, "articulation", None):
            articulation = json.loads(self.inference_cfg.GENERATION.articulation)
        # (likewise: generate.py --form, the JSON text of the form's bars)
        if form is None and getattr(self.inference_cfg.GENERATION, "form", None):
            form = json.loads(self.inference_cfg.GENERATION.form)
        gen = BatchedGenerator(self.model, self.device, glen, mlen, sliding=sliding, kv_dtype=kv_dtype,
                               **({"shared_prompt": True} if share else {}))

        def accept(seq, rep) -> bool:
            self.attempts += 1
            if seq is None:
                return False
            try:
                rep.validate_teacher_forced_sequence(seq)
            except Exception:
                return False
            return self.validate_generated_sequence(seq)
        # attempts decoded in up to `slots` (64) slots, a finished slot re-armed with the next attempt (the reference tries one
        # sequence after the other until num_generate passed; `max_rounds` bounds the attempts at max_rounds x num_generate)
        res = gen.generate_stream(list(encoded_meta), data, data.temperature, data.top_k, data.num_generate, accept,
                                  top_p=getattr(data, "top_p", 1.0), seed=self.uniform_seed,
                                  max_attempts=None if max_rounds is None else max_rounds * data.num_generate,
                                  return_logprobs=return_logprobs, prompt=None if not prompt else list(prompt),
                                  logit_bias=logit_bias, **({} if slots == 64 else {"slots": slots}),
                                  **({} if grammar is None else {"grammar": grammar}),
                                  **({} if harmony is None else {"harmony": harmony}),
                                  **({} if class_sampling is None else {"class_sampling": class_sampling}),
                                  **({} if note_order is None else {"note_order": note_order}),
                                  **({} if voices is None else {"voices": voices}),
                                  **({} if density is None else {"density": density}),
                                  **({} if interval is None else {"interval": interval}),
                                  **({} if onsets is None else {"onsets": onsets}),
                                  **({} if guide is None else {"guide": guide}),
                                  **({} if articulation is None else {"articulation": articulation}),
                                  **({} if form is None else {"form": form}))
        return (res[0], res[2]) if return_logprobs else res[0]

    def execute_pool(self, items, return_logprobs: bool = False, harmony=None):
        """generate.py --requests (not in the reference): MANY requests in one pool of decode slots
        (BatchedGenerator.generate_pool).  items: one dict per request -- encoded_meta, input_data (its num_generate,
        temperature, top_k, top_p), seed, max_rounds, logit_bias, prompt (token ids the request's sequences continue, None
        or [] for none), onsets (the request's own onset template, None: the pool-wide one of --onsets, if any), guide (likewise: --guide), articulation (likewise: --articulation), form (likewise: --form).  Every request is accepted by the two validators of
        execute() and bounded by max_rounds x num_generate attempts, as there; the pool-wide options (grammar, harmony,
        class_sampling, note_order, voices, density, interval, decode_slots, kv_cache, sliding_memory) come from the inference configuration
        as in execute().  Returns generate_pool's PoolResult list."""
        from ..generate import BatchedGenerator, PoolRequest
        G = self.inference_cfg.GENERATION
        mlen = getattr(self.inference_cfg.MODEL, "memory_length", 4146) if hasattr(self.inference_cfg, "MODEL") else 4146
        gen = BatchedGenerator(self.model, self.device, G.generation_length, mlen,
                               sliding=bool(getattr(G, "sliding_memory", False)), kv_dtype=str(getattr(G, "kv_cache", "bf16")))
        grammar = True if bool(getattr(G, "grammar", False)) else None
        class_sampling = None
        if getattr(G, "class_sampling", None):
            from ..generate import read_class_sampling
            class_sampling = read_class_sampling(json.loads(G.class_sampling))[0]
        note_order = None if getattr(G, "note_order", None) is None else int(G.note_order)
        voices = None if getattr(G, "voices", None) is None else int(G.voices)
        density = None if getattr(G, "density", None) is None else int(G.density)
        interval = None if getattr(G, "interval", None) is None else int(G.interval)
        onsets = json.loads(G.onsets) if getattr(G, "onsets", None) else None
        guide = json.loads(G.guide) if getattr(G, "guide", None) else None
        articulation = json.loads(G.articulation) if getattr(G, "articulation", None) else None
        form = json.loads(G.form) if getattr(G, "form", None) else None

        def accept(seq, rep) -> bool:
            self.attempts += 1
            if seq is None:
                return False
            try:
                rep.validate_teacher_forced_sequence(seq)
            except Exception:
                return False
            return self.validate_generated_sequence(seq)
        reqs = []
        for it in items:
            d = it["input_data"]
            mr = it.get("max_rounds")
            reqs.append(PoolRequest(list(it["encoded_meta"]), d, int(d.num_generate), d.temperature, d.top_k,
                                    top_p=getattr(d, "top_p", 1.0), seed=int(it.get("seed") or 0),
                                    max_attempts=None if mr is None else int(mr) * int(d.num_generate), accept=accept,
                                    logit_bias=it.get("logit_bias"), note_order=note_order, voices=voices,
                                    prompt=None if not it.get("prompt") else list(it["prompt"]), density=density,
                                    interval=interval, onsets=onsets if it.get("onsets") is None else it["onsets"],
                                    guide=guide if it.get("guide") is None else it["guide"],
                                    articulation=articulation if it.get("articulation") is None else it["articulation"],
                                    form=form if it.get("form") is None else it["form"]))
        return gen.generate_pool(reqs, slots=int(getattr(G, "decode_slots", 64)), grammar=grammar, harmony=harmony,
                                 class_sampling=class_sampling, return_logprobs=return_logprobs)
