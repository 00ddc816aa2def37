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
                class_sampling=None, note_order=None):                                                     # :338-354
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
        positions never go back and no pitch is drawn twice at one position (ForcedDecoder.set_note_order)."""
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
            import json

            from ..generate import read_class_sampling
            class_sampling = read_class_sampling(json.loads(self.inference_cfg.GENERATION.class_sampling))[0]
        # (likewise: generate.py --note_order / --max_notes, the control word; an argument given here wins)
        if note_order is None and getattr(self.inference_cfg.GENERATION, "note_order", None) is not None:
            note_order = int(self.inference_cfg.GENERATION.note_order)
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
                                  **({} if note_order is None else {"note_order": note_order}))
        return (res[0], res[2]) if return_logprobs else res[0]
