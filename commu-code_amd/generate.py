#!/usr/bin/env python3
"""Generation driver with the reference's command line (generate.py:8-50):

    python commu-code_amd/generate.py --checkpoint_dir <checkpoint.pt> --output_dir <dir> --bpm 70 \\
        --audio_key aminor --time_signature 4/4 --pitch_range mid_high --num_measures 8 --inst acoustic_piano \\
        --genre newage --min_velocity 60 --max_velocity 80 --track_role main_melody --rhythm standard \\
        --chord_progression Am-Am-...-E --num_generate 3

checkpoint -> model (ModelInitializeTask), arguments -> meta tokens + chord components (PreprocessTask),
`num_generate` sequences decoded in parallel with chord forcing (InferenceTask), both validators.  The token
sequences are written to <output_dir>/sequences.json: turning them into MIDI files (sequence_postprocessor.py,
miditoolkit) is outside the hot path this package replaces -- the lists are exactly what
`PostprocessTask.execute(sequences=...)` takes.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DECODE_SLOTS_MIN, DECODE_SLOTS_MAX, DECODE_SLOTS_DEFAULT = 1, 256, 64          # --decode_slots
MAX_NOTES_MIN, MAX_NOTES_MAX = 1, 128                                             # --max_notes
MAX_VOICES_MIN, MAX_VOICES_MAX = 1, 128                                           # --max_voices
NOTES_PER_BAR_MIN, NOTES_PER_BAR_MAX = 1, 255                                     # --min_notes_per_bar / --max_notes_per_bar
MAX_LEAP_MIN, MAX_LEAP_MAX = 1, 127                                               # --max_leap / --max_leap_up / --max_leap_down


def parse_args():
    from commu_amd.midi_generator import meta
    model_arg_parser = argparse.ArgumentParser(description="Model Arguments")
    input_arg_parser = argparse.ArgumentParser(description="Input Arguments")
    model_arg_parser.add_argument("--checkpoint_dir", type=str)
    # not in the reference (which is fp32 throughout, train.py:48): run generation in the reference's own arithmetic --
    # fp32 weights, activations, K/V cache and products -- instead of the bf16 throughput path.  The mode in which greedy
    # decoding (--temperature 0) reproduces the reference's tokens wherever the top-1 / top-2 logit gap exceeds fp32
    # summation-order noise (~1e-6 of the logit range; the bf16 path needs a gap above its ~1e-2 logit error).
    model_arg_parser.add_argument("--parity", action="store_true")
    # not in the reference (its inference configuration fixes them, config_helper.py:61-80): the length of the
    # Transformer-XL memory and the number of loop iterations.  Without --sliding_memory the K/V cache is linear and
    # context + generation_length must fit into memory_length + 1 positions; with it the cache is a ring of
    # memory_length + 1 rows that slides like the reference's memory (model.py:507-538), so generation_length is free.
    # (not given: the inference configuration's values, the reference's 4146 / 4096)
    model_arg_parser.add_argument("--memory_length", type=int, default=None)
    model_arg_parser.add_argument("--generation_length", type=int, default=None)
    model_arg_parser.add_argument("--sliding_memory", action="store_true")
    # not in the reference: the storage of the decode step's K/V cache.  fp8 = e4m3 bytes with one power-of-two scale byte
    # per 32 features, 0.516 of the bf16 cache's bytes; it rounds the cached K and V (accuracy-bounded, no parity claim:
    # INTEGRATION.md) and is refused together with --parity.
    model_arg_parser.add_argument("--kv_cache", type=str, choices=["bf16", "fp8"], default="bf16")
    # not in the reference: with --prompt_tokens every attempt continues the same opening; hold the K/V of the meta tokens
    # and the prompt ONCE for all decode slots instead of once per slot (the same attention, another summation order).
    # bf16 linear cache only: refused without --prompt_tokens and with --sliding_memory, --kv_cache fp8 or --parity.
    model_arg_parser.add_argument("--share_prompt", action="store_true")
    # not in the reference (whose token-to-MIDI step silently drops every token outside an exact Position, Note Velocity,
    # Note On, Note Duration or Position, Chord group, encoder_utils.py:385-419): the default event grammar -- every DRAWN
    # token continues such a group (commu_amd.generate.event_grammar).  Forced tokens and --prompt_tokens are not affected.
    model_arg_parser.add_argument("--grammar", action="store_true",
                                  help="event grammar: every drawn token continues a note or chord group")
    # not in the reference (whose notes are free to leave the chord chart): weigh every DRAWN pitch by the chord that is
    # sounding (commu_amd.generate.harmony_table).  chord: only chord tones are drawn; soft: the other pitch classes get
    # -X on the scale the softmax sees (--harmony_penalty X); FILE.json: a table of 110 rows (the chord tokens 195 .. 303,
    # then "no chord yet") of 12 numbers by pitch class (C first), null = banned.  Forced tokens and --prompt_tokens are not
    # affected.  Combines with every other option.
    model_arg_parser.add_argument("--harmony", type=str, default=None, metavar="{chord,soft,FILE.json}",
                                  help="harmony constraint: drawn pitches follow the sounding chord (chord: strictly, "
                                       "soft: by --harmony_penalty, or a JSON table of 110 rows of 12 numbers, null = banned)")
    model_arg_parser.add_argument("--harmony_penalty", type=float, default=4.0,
                                  help="what --harmony soft subtracts from the pitches outside the chord (default: %(default)s)")
    # not in the reference (one temperature / top_k for every token of a request): a sampling triple per token family.
    # {"pitch": {"temperature": 1.1, "top_k": 40}, "duration": {"temperature": 0}} names what is DRAWN -- velocity, pitch,
    # duration, boundary (a position, a bar or EOS) -- which the default event grammar fixes from the previous token, so
    # these names need --grammar; {"after": {"velocity": {...}}} names the class of the PREVIOUS token (other, bar, pitch,
    # velocity, chord, duration, position: what the kernel keys on) and needs no grammar.  Controls a family does not
    # name stay --temperature / --top_k / --top_p.  Forced tokens and --prompt_tokens are not affected.
    model_arg_parser.add_argument("--class_sampling", type=str, default=None, metavar="JSON_OR_FILE",
                                  help="sampling controls per token family: {\"pitch\": {\"temperature\": 1.1, \"top_k\": 40}, "
                                       "\"duration\": {\"temperature\": 0}} (drawn names velocity, pitch, duration, boundary "
                                       "need --grammar; {\"after\": {...}} is keyed by the previous token's class)")
    # not in the reference (whose sampler may step back inside a bar or put one pitch twice on one onset -- its training
    # data, sorted by start time with one Position token per note, never does): inside a bar the DRAWN positions never go
    # back and no pitch is drawn twice at one position; --max_notes N (1 .. 128, implies --note_order) also stops a position
    # from being drawn again once it holds N notes (1: one note per onset).  Overlapping durations are --max_voices' business; not enforced: the order
    # inside --prompt_tokens, forced tokens.  Combines with every other option, --parity included.
    model_arg_parser.add_argument("--note_order", action="store_true",
                                  help="note order: inside a bar drawn positions never go back and no note is doubled")
    model_arg_parser.add_argument("--max_notes", default=None, metavar="N",
                                  help=f"at most N notes per position, {MAX_NOTES_MIN} .. {MAX_NOTES_MAX} (implies --note_order; "
                                       "1 = one note per onset)")
    # not in the reference (whose token-to-MIDI step turns every Position, Velocity, Pitch, Duration group into a note
    # [start, start + duration) and lets them overlap): --max_voices N (1 .. 128) -- among the DRAWN notes at most N sound at
    # any tick (1: a monophonic line, for a bass or melody track); --no_restrike -- no drawn pitch is struck while the same
    # pitch still sounds (the first note-off would silence the second note).  Both imply --note_order.  Not covered: notes
    # inside --prompt_tokens against each other, anything a forced token starts; a strict --harmony or pitch range that
    # leaves no pitch free ends that attempt (as with --max_notes).  When the rest of a bar is taken only Bar and EOS remain.
    model_arg_parser.add_argument("--max_voices", default=None, metavar="N",
                                  help=f"at most N drawn notes sound at once, {MAX_VOICES_MIN} .. {MAX_VOICES_MAX} (implies "
                                       "--note_order; 1 = a monophonic line).  Not covered: notes inside --prompt_tokens "
                                       "against each other, anything a forced token starts; a strict --harmony or pitch "
                                       "range that leaves no pitch free ends that attempt")
    model_arg_parser.add_argument("--no_restrike", action="store_true",
                                  help="no drawn pitch is struck while it still sounds (implies --note_order; covers what "
                                       "--max_voices covers)")
    # not in the reference (whose conditioning has no token for how many notes a bar holds: with Bar allowed at every note
    # boundary some bars close after one note or none, others run to dozens): --min_notes_per_bar N -- no Bar or EOS is
    # DRAWN while the bar being written holds fewer than N notes, unless no position is left to draw; --max_notes_per_bar
    # N -- no position is drawn once it holds N (only Bar and EOS remain).  Both imply --note_order.  Not covered: notes
    # inside --prompt_tokens (they count, and are never removed); a note that starts on a forced position (a first chord
    # inside its bar, two chords in one bar: it counts, and cannot be prevented); a bar cut by the generation length; forced
    # tokens (a forced Bar or EOS may close a short bar); a strict --harmony, pitch range or --max_notes that leaves no
    # pitch for a drawn position ends that attempt as before.  With --requests they hold for the whole pool.
    model_arg_parser.add_argument("--min_notes_per_bar", default=None, metavar="N",
                                  help=f"at least N notes in every bar that is drawn, {NOTES_PER_BAR_MIN} .. "
                                       f"{NOTES_PER_BAR_MAX} (implies --note_order; waived when no position is left).  Not "
                                       "covered: bars closed by a forced token or cut by the generation length")
    model_arg_parser.add_argument("--max_notes_per_bar", default=None, metavar="N",
                                  help=f"at most N notes in every bar that is drawn, {NOTES_PER_BAR_MIN} .. "
                                       f"{NOTES_PER_BAR_MAX}, not below --min_notes_per_bar (implies --note_order).  Not "
                                       "covered: notes inside --prompt_tokens, a note that starts on a forced position")
    # not in the reference (whose conditioning has no token for the melodic line: even a monophonic --max_voices 1 line
    # jumps anywhere in the 128-pitch range from one note to the next): --max_leap N -- no pitch is DRAWN more than N
    # semitones above or below the pitch of the note before it; --max_leap_up / --max_leap_down set one direction;
    # --no_repeat_pitch bans that pitch itself.  They imply none of the other constraints and need no --grammar.  NOT
    # covered: the first note, and a note after a full bar without one, have no reference; notes inside --prompt_tokens
    # are not checked against each other (the prompt's last note is the reference of the first draw); several notes at
    # one position are compared in token order, so the rule also limits the spread of a chord of notes (it is meant for
    # --max_voices 1 lines); a pitch range, --logit_bias, strict --harmony, --note_order or --no_restrike ban that leaves
    # no pitch inside the window ends that attempt as before (narrow windows with --no_repeat_pitch are the case); a
    # prompt whose last note lies outside --pitch_min / --pitch_max by more than the cap does so at once.  With
    # --requests they hold for the whole pool.
    model_arg_parser.add_argument("--max_leap", default=None, metavar="N",
                                  help=f"no drawn pitch more than N semitones above or below the note before it, "
                                       f"{MAX_LEAP_MIN} .. {MAX_LEAP_MAX}.  Not covered: the first note and a note after a "
                                       "full bar's rest; notes inside --prompt_tokens")
    model_arg_parser.add_argument("--max_leap_up", default=None, metavar="N",
                                  help=f"the same upwards only, {MAX_LEAP_MIN} .. {MAX_LEAP_MAX} (not beside --max_leap)")
    model_arg_parser.add_argument("--max_leap_down", default=None, metavar="N",
                                  help=f"the same downwards only, {MAX_LEAP_MIN} .. {MAX_LEAP_MAX} (not beside --max_leap)")
    model_arg_parser.add_argument("--no_repeat_pitch", action="store_true",
                                  help="no drawn pitch repeats the pitch of the note before it (same reference note as "
                                       "--max_leap)")
    # not in the reference (whose conditioning has one coarse rhythm token and nothing finer, so that two tracks generated
    # from the same metadata share no groove): --onsets TEMPLATE -- a position is DRAWN only where the template's row for
    # the bar being written allows an onset; bar i uses row i mod R, the bars of --prompt_tokens counted.  TEMPLATE is
    # JSON text or a file holding it: a list of bars, each a list of positions 0 .. 127; {"grid": n}, n a power of two from
    # 1 to 128 (the multiples of 128 / n); {"bars": [...]}; or {"from_tokens": [ids], "invert": bool} -- the onsets of a
    # finished track bar by bar, or with invert the positions it leaves free.  It implies none of the other constraints
    # and needs no --grammar.  NOT covered: forced tokens (the position 0 forced after a Bar, a chord's forced position,
    # and so a note that starts on either), notes inside --prompt_tokens, a bar cut by --generation_length; a template,
    # pitch range or strict --harmony that leaves nothing to draw in a family ends that attempt as before.  With
    # --requests it holds for every request that does not carry an "onsets" of its own.
    model_arg_parser.add_argument("--onsets", default=None, metavar="TEMPLATE",
                                  help='a drawn note starts only where the bar\'s row of the template allows: JSON text or '
                                       'file, [[positions 0 .. 127], ...] per bar (cycled), {"grid": n}, {"bars": [...]} or '
                                       '{"from_tokens": [ids], "invert": bool}.  Not covered: forced positions, notes '
                                       'inside --prompt_tokens')
    # not in the reference (which builds an arrangement by combining tracks generated separately, none of which reads another
    # track's notes): --guide SPEC -- a pitch is DRAWN only where the guide's cell for the position the bar is at allows it,
    # and a position only where its cell leaves a pitch (of --pitch_min .. --pitch_max).  SPEC is JSON text or a file
    # holding it: the raw form {"cells": C, "bars": [[null | [MIDI pitches], .. C entries], ..]} (null: every pitch; C a
    # power of two from 1 to 128; at most 64 bars, cycled), or the derived form {"from_tokens": [ids], "cells": 16,
    # "avoid_intervals": [1, 11], "no_unison": false, "below": m | "above": m} -- the notes of a finished track: where
    # pitches Y sound, x is allowed iff (x - y) mod 12 is in avoid_intervals for no y, x is not in Y (no_unison),
    # x <= min Y - m (below), x >= max Y + m (above); a silent step allows everything; a cell is the AND over its steps.
    # It implies none of the other constraints and needs no --grammar.  NOT covered: only a note's START is tested (a drawn
    # note held across a later change of the guide is not checked; --articulation's hold_guide covers it), forced tokens (the position 0 after a Bar, a chord's
    # position), notes inside --prompt_tokens; a pitch range, strict --harmony or --max_leap window that together with the
    # cell leaves no pitch ends that attempt as before.  With --requests it holds for every request that does not carry a
    # "guide" of its own.
    model_arg_parser.add_argument("--guide", default=None, metavar="SPEC",
                                  help='a drawn pitch fits a mask over pitches indexed by time: JSON text or file, '
                                       '{"cells": C, "bars": [[null | [pitches], ...], ...]} or {"from_tokens": [ids], '
                                       '"cells": 16, "avoid_intervals": [1, 11], "no_unison": false, "below": m | "above": m}'
                                       '.  Not covered: held notes, forced positions, notes inside --prompt_tokens')
    # not in the reference (whose notes take whatever duration and velocity the model draws): --articulation SPEC -- a
    # duration is DRAWN only inside a window of steps and a velocity only inside a range, per bar of a template.  SPEC is
    # JSON text or a file holding it: the full form {"bars": [{"duration": [lo, hi], "velocity": [lo, hi]} | null, ...],
    # "within_bar": bool, "hold_guide": bool} (at most 64 bars, cycled bar by bar; a null bar constrains nothing), or the short
    # form with the single bar's keys at top level, e.g. {"duration": [2, 16], "hold_guide": true}.  duration is in steps
    # 1 .. 128 and either end may be null; velocity is in MIDI 0 .. 127 and maps to the bins floor(lo / 2) .. ceil(hi / 2),
    # capped at 63, as --min_velocity / --max_velocity do.  within_bar: a drawn note ends by the bar line.  hold_guide (needs
    # --guide): a drawn note ends before the first step where the guide bans its pitch -- the guide's own rule tests a
    # note's start only.  Where the bar line or the guide leaves less room than the lower bound, the lower bound gives way.
    # It implies none of the other constraints and needs no --grammar.  NOT covered: forced tokens and anything a forced
    # position starts, notes inside --prompt_tokens; hold_guide reads the next bar's cells even where --generation_length
    # would cut the sequence first, and tests the guide only (--harmony across a chord change is not tested).  With
    # --requests it holds for every request that does not carry an "articulation" of its own.
    model_arg_parser.add_argument("--articulation", default=None, metavar="SPEC",
                                  help='drawn durations and velocities follow a per-bar template: JSON text or file, '
                                       '{"bars": [{"duration": [lo, hi], "velocity": [lo, hi]} | null, ...], "within_bar": '
                                       'bool, "hold_guide": bool} or one bar\'s keys at top level.  Not covered: forced '
                                       'tokens, notes inside --prompt_tokens')
    # not in the reference (whose bars are unrelated draws): --form SPEC -- a bar of the sequence REPLAYS an earlier bar of the
    # same sequence.  SPEC is a letter string such as AABA (the first bar with a letter is free, later ones replay it in
    # full), JSON text {"bars": [null | j | {"of": j, "copy": "all" | "rhythm", "transpose": s}, ...]} (bar i is free or
    # replays bar j < i: every token of its notes, transposed by s semitones in -48 .. 48 and folded into the MIDI range, or
    # its rhythm only -- positions, velocities and durations, the pitches drawn under every constraint in force), or a file
    # holding either.  At most 64 bars, not cycled: bars past the form's end are free; bar 0 is always free.  The replayed
    # tokens go through the chord / bar rules like drawn ones, so the bar gets the chords of its own place in the
    # progression; they consume no random number and carry no log-probability.  "copy": "rhythm" needs --grammar.  The bars
    # of --prompt_tokens are valid sources; the bar a prompt leaves open is free.  It runs under --parity as well (the
    # parity mode decodes through the same loop).  NOT covered: replayed tokens are not checked against any constraint, as
    # forced tokens are not (a strict --harmony under another chord is the user's business: "copy": "rhythm" is the answer);
    # a replay bar cut by --generation_length is not completed; bars past the 64th are free; a note of the source bar that
    # the bar line cut does not appear; chord tokens are never copied.  With --requests it holds for every request that
    # does not carry a "form" of its own.
    model_arg_parser.add_argument("--form", default=None, metavar="SPEC",
                                  help='a bar replays an earlier bar of its own sequence: letters (AABA), JSON text or file, '
                                       '{"bars": [null | j | {"of": j, "copy": "all" | "rhythm", "transpose": s}, ...]}; or a '
                                       'bar of a finished sequence you have: {"keep": {"from_tokens": [ids]}, "redo": [bars], '
                                       '"repitch": [bars]} or {"takes": [[ids], ...], "bars": [... {"take": t, "of": j}]}.  '
                                       'Not covered: a redone bar knows only the bars before it, constraints on replayed '
                                       'tokens, bars past the 64th, a bar cut by '
                                       '--generation_length')
    # not in the reference (which decodes one sequence at a time): how many attempts are decoded side by side.  1 .. 256;
    # up to 256 slots run the fused layer-tail launches ("Supported shapes").  The sequences returned do
    # not depend on it.  (checked by check_decode_slots: the range is named in its message)
    model_arg_parser.add_argument("--decode_slots", default=DECODE_SLOTS_DEFAULT,
                                  help=f"parallel decode slots, {DECODE_SLOTS_MIN} .. {DECODE_SLOTS_MAX} (default: %(default)s)")
    input_arg_parser.add_argument("--output_dir", type=str, required=True)
    input_arg_parser.add_argument("--bpm", type=int)
    input_arg_parser.add_argument("--audio_key", type=str, choices=list(meta.KEY_MAP.keys()))
    input_arg_parser.add_argument("--time_signature", type=str, choices=list(meta.TIME_SIG_MAP.keys()))
    input_arg_parser.add_argument("--pitch_range", type=str, choices=list(meta.PITCH_RANGE_MAP.keys()))
    input_arg_parser.add_argument("--num_measures", type=float)
    input_arg_parser.add_argument("--inst", type=str, choices=list(meta.INST_MAP.keys()))
    input_arg_parser.add_argument("--genre", type=str, default="cinematic", choices=list(meta.GENRE_MAP.keys()))
    input_arg_parser.add_argument("--track_role", type=str, choices=list(meta.TRACK_ROLE_MAP.keys()))
    input_arg_parser.add_argument("--rhythm", type=str, default="standard", choices=list(meta.RHYTHM_MAP.keys()))
    input_arg_parser.add_argument("--min_velocity", type=int, choices=range(1, 128))
    input_arg_parser.add_argument("--max_velocity", type=int, choices=range(1, 128))
    input_arg_parser.add_argument("--chord_progression", type=str, help="Chord progression ex) C-C-E-E-G-G ...")
    input_arg_parser.add_argument("--num_generate", type=int)
    input_arg_parser.add_argument("--top_k", type=int, default=32)
    input_arg_parser.add_argument("--temperature", type=float, default=0.95)
    # not in the reference (top-k only, generate.py:43): nucleus filter applied after top-k; 1.0 = off
    input_arg_parser.add_argument("--top_p", type=float, default=1.0)
    # not in the reference (which retries rejected sequences forever, midi_inferrer.py:342-353): bound the retries
    input_arg_parser.add_argument("--max_rounds", type=int, default=None)
    # not in the reference (which returns token ids only): also write "logprobs" to sequences.json -- per sequence one
    # [full, kept] pair per token (log-softmax of logits / temperature at the token; log of its probability after top-k /
    # top-p and renormalisation), null for the tokens that were not drawn (context, forced bars / positions / chords)
    input_arg_parser.add_argument("--logprobs", action="store_true")
    # not in the reference (which starts every sequence from the meta tokens): a JSON list of token ids that FOLLOW the
    # meta tokens; every generated sequence continues it (primed generation: the loop enters in the state it would be in
    # after producing these tokens itself; a prompt the chord / bar rules could not have produced is refused).
    # --generation_length counts the iterations after the prompt.
    input_arg_parser.add_argument("--prompt_tokens", type=str, default=None, metavar="FILE")
    # not in the reference (where pitch_range / min_velocity / max_velocity / inst are conditioning hints only): constrain
    # what the sequences may DRAW.  --logit_bias: a JSON file {"ban": [ids], "bias": {"id": number}} -- banned ids are never
    # drawn, a number is added to the id's logit on the scale the softmax sees (after the division by the temperature),
    # before top-k.  --pitch_min / --pitch_max: MIDI note numbers, pitch tokens outside them are banned.  Forced tokens
    # (bars, positions, the chord progression) and --prompt_tokens are not affected.
    input_arg_parser.add_argument("--logit_bias", type=str, default=None, metavar="FILE")
    input_arg_parser.add_argument("--pitch_min", type=int, default=None)
    input_arg_parser.add_argument("--pitch_max", type=int, default=None)
    # not in the reference: replicas of the generator, one per GPU (default: every visible GPU, at most num_generate)
    input_arg_parser.add_argument("--gpus", type=int, default=None)
    # not in the reference (one request per process and per model load): MANY requests decoded in one pool of decode slots
    # (commu_amd.generate.BatchedGenerator.generate_pool).  FILE.json: a list of objects whose keys are the input arguments
    # of one request -- bpm .. chord_progression, num_generate, top_k, temperature, top_p, optional seed, max_rounds,
    # pitch_min, pitch_max, logit_bias, prompt_tokens -- each of which gets exactly the sequences a run of its own with
    # --decode_slots 1 and the same seed writes.  prompt_tokens: a list of token ids the request's sequences continue (what
    # --prompt_tokens FILE holds for a single request; every request may carry its own).  The model arguments apply to the
    # whole pool; sequences.json becomes {"requests": [...]}.
    # Refused with any single-request input argument, --prompt_tokens, --share_prompt, --parity, and --gpus above 1.
    input_arg_parser.add_argument("--requests", type=str, default=None, metavar="FILE.json",
                                  help="a JSON list of requests (objects of input arguments: bpm .. chord_progression, "
                                       "num_generate, top_k, temperature, top_p, optional seed, max_rounds, pitch_min, "
                                       "pitch_max, logit_bias, prompt_tokens: a list of token ids the request "
                                       "continues) decoded in ONE pool of --decode_slots slots; sequences.json "
                                       "becomes {\"requests\": [...]}")
    return {"model_args": model_arg_parser, "input_args": input_arg_parser}


def read_prompt_tokens(path):
    """The token ids of a --prompt_tokens file: a JSON list of integers."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, list) or not all(isinstance(t, int) and not isinstance(t, bool) for t in doc):
        raise ValueError(f"{path}: a JSON list of token ids expected")
    return doc


def check_share_prompt(model_args, input_args):
    """--share_prompt against the options it cannot be combined with (host code only; ValueError with the reason)."""
    if not getattr(model_args, "share_prompt", False):
        return
    if not getattr(input_args, "prompt_tokens", None):
        raise ValueError("--share_prompt needs --prompt_tokens: without a prompt there is nothing to share")
    for flag, on in (("--sliding_memory", bool(getattr(model_args, "sliding_memory", False))),
                     ("--kv_cache fp8", getattr(model_args, "kv_cache", "bf16") == "fp8"),
                     ("--parity", bool(getattr(model_args, "parity", False)))):
        if on:
            raise ValueError(f"--share_prompt cannot be combined with {flag}: the shared prompt prefix is built for the "
                             "bf16 linear K/V cache only")


def check_decode_slots(model_args):
    """--decode_slots as an int in [1, 256] (host code only; ValueError that names the range).  Also written back to
    model_args, so that what travels to the replicas is the checked number."""
    v = getattr(model_args, "decode_slots", DECODE_SLOTS_DEFAULT)
    try:
        n = int(v) if not isinstance(v, (bool, float)) else None
    except (TypeError, ValueError):
        n = None
    if n is None or not DECODE_SLOTS_MIN <= n <= DECODE_SLOTS_MAX:
        raise ValueError(f"--decode_slots: an integer in [{DECODE_SLOTS_MIN}, {DECODE_SLOTS_MAX}] expected, got {v!r}")
    model_args.decode_slots = n
    return n


def check_note_order(model_args):
    """--note_order / --max_notes as the note-order control word (None: neither flag; 0: on; N: on with the cap); host
    code only, ValueError that names the range.  Written back to model_args.note_order_word, which travels to the
    replicas (ModelInitializeTask puts it into the inference configuration)."""
    v = getattr(model_args, "max_notes", None)
    word = 0 if getattr(model_args, "note_order", False) else None
    if v is not None:
        try:
            word = int(v) if not isinstance(v, (bool, float)) else None
        except (TypeError, ValueError):
            word = None
        if word is None or not MAX_NOTES_MIN <= word <= MAX_NOTES_MAX:
            raise ValueError(f"--max_notes: an integer in [{MAX_NOTES_MIN}, {MAX_NOTES_MAX}] expected, got {v!r}")
    model_args.note_order_word = word
    return word


def check_voices(model_args):
    """--max_voices / --no_restrike as the voice control word N + 256 r (None: neither flag); host code only, ValueError
    that names the range.  Written back to model_args.voices_word, which travels to the replicas (ModelInitializeTask puts
    it into the inference configuration); either flag switches --note_order on."""
    v = getattr(model_args, "max_voices", None)
    n = 0
    if v is not None:
        try:
            n = int(v) if not isinstance(v, (bool, float)) else None
        except (TypeError, ValueError):
            n = None
        if n is None or not MAX_VOICES_MIN <= n <= MAX_VOICES_MAX:
            raise ValueError(f"--max_voices: an integer in [{MAX_VOICES_MIN}, {MAX_VOICES_MAX}] expected, got {v!r}")
    word = None
    if v is not None or getattr(model_args, "no_restrike", False):
        word = n + (256 if getattr(model_args, "no_restrike", False) else 0)
        model_args.note_order = True
    model_args.voices_word = word
    return word


REQUEST_META_KEYS = ("bpm", "audio_key", "time_signature", "pitch_range", "num_measures", "inst", "genre", "track_role",
                     "rhythm", "min_velocity", "max_velocity", "chord_progression")
REQUEST_KEYS = REQUEST_META_KEYS + ("num_generate", "top_k", "temperature", "top_p", "seed", "max_rounds", "pitch_min",
                                    "pitch_max", "logit_bias")
# (keys a request object may carry and that its parsed dict holds only then: prompt_tokens, the token ids it continues)
# and onsets, its own onset template (--onsets' forms, as JSON values)
# and guide, its own guide track (--guide's forms, as JSON values)
# and articulation, its own articulation (--articulation's forms, as JSON values)
# and form, its own form (--form's forms, as JSON values)
REQUEST_OPTIONAL_KEYS = ("prompt_tokens", "onsets", "guide", "articulation", "form")
# (single-request input arguments that --requests replaces, with the value the parser gives them when they are not named)
SINGLE_REQUEST_ARGS = {**{k: None for k in REQUEST_META_KEYS}, "genre": "cinematic", "rhythm": "standard",
                       "num_generate": None, "top_k": 32, "temperature": 0.95, "top_p": 1.0, "max_rounds": None,
                       "logit_bias": None, "pitch_min": None, "pitch_max": None}


def check_requests(model_args, input_args):
    """--requests FILE.json as a list of per-request argument dicts (None without the flag): every key of REQUEST_KEYS,
    the parser's defaults where an object does not name one (seed 0).  Host code only, run before a model is loaded;
    ValueError that says what is wrong -- a single-request input argument, --prompt_tokens, --share_prompt or --parity
    beside --requests, --gpus above 1, a file that is not a JSON list of objects, an unknown key, a missing
    num_generate, a prompt_tokens value that is not a list of integers or an onsets value that is no template (with the
    index of the request)."""
    path = getattr(input_args, "requests", None)
    if path is None:
        return None
    given = [k for k, d in SINGLE_REQUEST_ARGS.items() if getattr(input_args, k, d) != d]
    if given:
        raise ValueError(f"--requests cannot be combined with the single-request input argument --{given[0]}: every "
                         "request of the file carries its own")
    for flag, on in (("--prompt_tokens", bool(getattr(input_args, "prompt_tokens", None))),
                     ("--share_prompt", bool(getattr(model_args, "share_prompt", False))),
                     ("--parity", bool(getattr(model_args, "parity", False)))):
        if on:
            raise ValueError(f"--requests cannot be combined with {flag}: a request of the pool carries its own prompt "
                             "(\"prompt_tokens\" in its object); the pool runs on the bf16 and fp8 K/V caches")
    gpus = getattr(input_args, "gpus", None)
    if gpus is not None and gpus > 1:
        raise ValueError(f"--requests with --gpus {gpus}: the request pool runs on one GPU (dealing requests to replicas "
                         "is not built)")
    try:
        with open(path) as f:
            doc = json.load(f)
    except OSError as e:
        raise ValueError(f"--requests: a readable JSON file expected, got {path!r} ({e.strerror})") from None
    except json.JSONDecodeError as e:
        raise ValueError(f"--requests: {path}: not JSON ({e})") from None
    if not isinstance(doc, list) or not doc:
        raise ValueError(f"--requests: {path}: a non-empty JSON list of request objects expected")
    out = []
    for i, r in enumerate(doc):
        if not isinstance(r, dict):
            raise ValueError(f"--requests: {path}: request {i}: an object of input arguments expected, got "
                             f"{type(r).__name__}")
        unknown = sorted(set(r) - set(REQUEST_KEYS) - set(REQUEST_OPTIONAL_KEYS))
        if unknown:
            raise ValueError(f"--requests: {path}: request {i}: unknown key {unknown[0]!r} (known: "
                             f"{', '.join(REQUEST_KEYS + REQUEST_OPTIONAL_KEYS)})")
        if "num_generate" not in r:
            raise ValueError(f"--requests: {path}: request {i}: num_generate is missing")
        n = r["num_generate"]
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"--requests: {path}: request {i}: num_generate: an integer >= 1 expected, got {n!r}")
        pt = r.get("prompt_tokens", [])
        if not isinstance(pt, list) or not all(isinstance(t, int) and not isinstance(t, bool) for t in pt):
            raise ValueError(f"--requests: {path}: request {i}: prompt_tokens: a JSON list of token ids expected, got {pt!r}")
        if r.get("onsets") is not None:
            try:
                r = {**r, "onsets": onsets_bars(r["onsets"], "onsets")}
            except ValueError as e:
                raise ValueError(f"--requests: {path}: request {i}: {e}") from None
        if r.get("guide") is not None:
            try:
                r = {**r, "guide": guide_doc(r["guide"], "guide", r.get("pitch_min"), r.get("pitch_max"))}
            except ValueError as e:
                raise ValueError(f"--requests: {path}: request {i}: {e}") from None
        if r.get("articulation") is not None:
            try:
                r = {**r, "articulation": articulation_doc(r["articulation"], "articulation")}
            except ValueError as e:
                raise ValueError(f"--requests: {path}: request {i}: {e}") from None
        if r.get("form") is not None:
            try:
                r = {**r, "form": form_doc(r["form"], "form", bool(getattr(model_args, "grammar", False)))}
            except ValueError as e:
                raise ValueError(f"--requests: {path}: request {i}: {e}") from None
        out.append({**SINGLE_REQUEST_ARGS, "seed": 0, **r})
    # (hold_guide reads the request's guide: its own, or the pool-wide one of --guide)
    pool_art = check_articulation(model_args, needs_guide=False)
    pool_art = None if pool_art is None else json.loads(pool_art)
    for i, r in enumerate(out):
        art = r.get("articulation") if r.get("articulation") is not None else pool_art
        if art is not None and art["hold_guide"] and r.get("guide") is None and getattr(model_args, "guide", None) is None:
            raise ValueError(f"--requests: {path}: request {i}: articulation: hold_guide without a guide (neither the "
                             "request's own \"guide\" nor --guide)")
    return out


def form_doc(doc, what="--form", grammar=True):
    """A form given as a letter string or a JSON value, validated and returned written out: {"bars": [null | {"of": j,
    "copy": "all" | "rhythm", "transpose": s}, ...]}.  A form that names takes -- {"takes": ..., "bars": ...} or the short
    form {"keep": ..., "redo": [...], "repitch": [...]} -- is written out in the full form {"takes": [[ids], ...], "bars":
    [...]}, so that whoever gets the document gets the tokens.  Host code only, ValueError that says what is wrong -- a
    rhythm bar without --grammar among it."""
    from commu_amd.generate import CommuHipError, form_document, form_is_rhythm, form_row_fields, form_template
    try:
        rows = form_template(doc)
    except CommuHipError as e:
        raise ValueError(f"{what}: {str(e).removeprefix('form: ')}") from None
    if form_is_rhythm(rows) and not grammar:
        raise ValueError(f'{what}: "copy": "rhythm" without --grammar: the pitches of such a bar are drawn, and only the '
                         "grammar makes that draw a pitch")
    if getattr(rows, "takes", ()):
        return form_document(rows)
    bars = []
    for w in rows[:, 0].tolist():
        f = form_row_fields(w)
        bars.append(None if f is None else {"of": f[0], "copy": f[1], "transpose": f[2]})
    if all(b is None or (b["copy"] == "all" and b["transpose"] == 0) for b in bars):
        bars = [None if b is None else b["of"] for b in bars]
    return {"bars": bars}


def check_form(model_args):
    """--form as the JSON text of the form written out (None without the flag): the value is a letter string, the JSON
    document itself or the path of a file that holds either.  Host code only, run before a model is loaded; ValueError that
    says what is wrong.  Written back to model_args.form_doc, which travels to the replicas (ModelInitializeTask puts it into
    the inference configuration).  It switches nothing else on."""
    setting = getattr(model_args, "form", None)
    model_args.form_doc = None
    if setting is None:
        return None
    if not isinstance(setting, str):
        raise ValueError(f"--form: letters, JSON text or a readable file expected, got {setting!r}")
    model_args.form_doc = json.dumps(form_doc(setting, "--form", bool(getattr(model_args, "grammar", False))))
    return model_args.form_doc


def articulation_doc(doc, what="--articulation"):
    """An articulation given as a JSON value -- the full form or the short form -- validated and returned as the full form
    {"bars": [...], "within_bar": bool, "hold_guide": bool} with every bar written out ({"duration": [lo | null, hi | null],
    "velocity": [lo, hi]} in MIDI velocities that map back to the same bins, null for a bar that constrains nothing).  Host
    code only, ValueError that says what is wrong."""
    from commu_amd.generate import CommuHipError, articulation_template
    try:
        rows, w, h = articulation_template(doc)
    except CommuHipError as e:
        raise ValueError(f"{what}: {str(e).removeprefix('articulation: ')}") from None
    bars = []
    for r in rows:
        dlo, dhi = int(r[0]) & 255, (int(r[0]) >> 8) & 255
        mask = int(r[1]) | int(r[2]) << 32
        if dlo == 0 and dhi == 0 and mask == (1 << 64) - 1:
            bars.append(None)
            continue
        b0, b1 = (mask & -mask).bit_length() - 1, mask.bit_length() - 1
        bars.append({"duration": [dlo or None, dhi or None], "velocity": [2 * b0, min(2 * b1, 127)]})
    return {"bars": bars, "within_bar": w, "hold_guide": h}


def check_articulation(model_args, needs_guide=True):
    """--articulation as the JSON text of the articulation's full form (None without the flag): the value is the JSON
    document itself or the path of a file that holds it.  Host code only, run before a model is loaded; ValueError that says
    what is wrong -- hold_guide without --guide among it (needs_guide; with --requests a request's own guide will do, and
    check_requests tests it).  Written back to model_args.articulation_doc, which travels to the replicas
    (ModelInitializeTask puts it into the inference configuration).  It switches nothing else on."""
    setting = getattr(model_args, "articulation", None)
    model_args.articulation_doc = None
    if setting is None:
        return None
    text = setting
    if not isinstance(setting, str):
        raise ValueError(f"--articulation: JSON text or a readable JSON file expected, got {setting!r}")
    if not setting.lstrip().startswith(("{", "[")):
        try:
            with open(setting) as f:
                text = f.read()
        except OSError as e:
            raise ValueError(f"--articulation: JSON text or a readable JSON file expected, got {setting!r} "
                             f"({e.strerror})") from None
    try:
        doc = json.loads(text)
    except json.JSONDecodeError as e:
        raise ValueError(f"--articulation: not JSON ({e})") from None
    out = articulation_doc(doc, "--articulation")
    if needs_guide and out["hold_guide"] and getattr(model_args, "guide", None) is None:
        raise ValueError("--articulation: hold_guide without --guide: it ends a note where the guide bans its pitch")
    model_args.articulation_doc = json.dumps(out)
    return model_args.articulation_doc


def guide_doc(doc, what="--guide", pitch_min=None, pitch_max=None):
    """A guide track given as a JSON value -- the raw form or the from_tokens form -- validated and returned as the raw form
    {"cells": C, "bars": [...], "pitch_range": [lo, hi]} (the derived form is worked out here, once); pitch_min / pitch_max
    (None: 0 / 127) feed the pitch range of the live bits unless the value names one.  Host code only, ValueError that says
    what is wrong."""
    from commu_amd.generate import CommuHipError, guide_template
    try:
        if not isinstance(doc, dict):
            raise CommuHipError(f'guide: {{"cells": C, "bars": [...]}} or {{"from_tokens": [...], ...}} expected, got {doc!r}')
        rng = doc.get("pitch_range")
        if rng is None:
            rng = [0 if pitch_min is None else int(pitch_min), 127 if pitch_max is None else int(pitch_max)]
        rows, cells = guide_template(doc, tuple(rng) if isinstance(rng, list) else rng)
    except CommuHipError as e:
        raise ValueError(f"{what}: {str(e).removeprefix('guide: ')}") from None
    bars = []
    for b in range(rows.shape[0] // (1 + cells)):
        bar = []
        for c in range(cells):
            w = rows[b * (1 + cells) + 1 + c]
            ps = [k for k in range(128) if (int(w[k // 32]) >> (k % 32)) & 1]
            bar.append(None if len(ps) == 128 else ps)
        bars.append(bar)
    return {"cells": cells, "bars": bars, "pitch_range": [int(rng[0]), int(rng[1])]}


def check_guide(model_args, input_args=None):
    """--guide as the JSON text of the guide's raw form (None without the flag): the value is the JSON document itself or
    the path of a file that holds it.  Host code only, run before a model is loaded; ValueError that says what is wrong.
    --pitch_min / --pitch_max feed the pitch range of the live bits.  Written back to model_args.guide_doc, which travels
    to the replicas (ModelInitializeTask puts it into the inference configuration).  It switches nothing else on."""
    setting = getattr(model_args, "guide", None)
    model_args.guide_doc = None
    if setting is None:
        return None
    text = setting
    if not isinstance(setting, str):
        raise ValueError(f"--guide: JSON text or a readable JSON file expected, got {setting!r}")
    if not setting.lstrip().startswith(("{", "[")):
        try:
            with open(setting) as f:
                text = f.read()
        except OSError as e:
            raise ValueError(f"--guide: JSON text or a readable JSON file expected, got {setting!r} ({e.strerror})") from None
    try:
        doc = json.loads(text)
    except json.JSONDecodeError as e:
        raise ValueError(f"--guide: not JSON ({e})") from None
    src = input_args if input_args is not None else model_args
    model_args.guide_doc = json.dumps(guide_doc(doc, "--guide", getattr(src, "pitch_min", None),
                                                getattr(src, "pitch_max", None)))
    return model_args.guide_doc


def onsets_bars(doc, what="--onsets"):
    """An onset template given as a JSON value -- a list of bars, {"grid": n}, {"bars": [...]} or {"from_tokens": [ids],
    "invert": bool} -- as its list of bars, each the sorted list of positions 0 .. 127 that may hold an onset; host code
    only, ValueError that says what is wrong."""
    from commu_amd.generate import CommuHipError, onset_rows, onsets_of
    if isinstance(doc, dict) and "from_tokens" in doc:
        extra = sorted(set(doc) - {"from_tokens", "invert"})
        toks, inv = doc["from_tokens"], doc.get("invert", False)
        if extra:
            raise ValueError(f'{what}: {{"from_tokens": [ids], "invert": bool}} expected, got the key {extra[0]!r} as well')
        if not isinstance(toks, list) or not all(isinstance(t, int) and not isinstance(t, bool) and 0 <= t < 729 for t in toks):
            raise ValueError(f"{what}: from_tokens: a JSON list of token ids in [0, 729) expected")
        if not isinstance(inv, bool):
            raise ValueError(f"{what}: invert: true or false expected, got {inv!r}")
        doc = onsets_of(toks, invert=inv)
    try:
        rows = onset_rows(doc)
    except CommuHipError as e:
        raise ValueError(f"{what}: {str(e).removeprefix('onsets: ')}") from None
    return [[g for g in range(128) if (int(row[g // 32]) >> (g % 32)) & 1] for row in rows]


def check_onsets(model_args):
    """--onsets as the JSON text of the template's list of bars (None without the flag): the value is the JSON document
    itself or the path of a file that holds it.  Host code only, run before a model is loaded; ValueError that says what is
    wrong.  Written back to model_args.onsets_bars, which travels to the replicas (ModelInitializeTask puts it into the
    inference configuration).  It switches nothing else on."""
    setting = getattr(model_args, "onsets", None)
    model_args.onsets_bars = None
    if setting is None:
        return None
    text = setting
    if not isinstance(setting, str):
        raise ValueError(f"--onsets: JSON text or a readable JSON file expected, got {setting!r}")
    if not setting.lstrip().startswith(("{", "[")):
        try:
            with open(setting) as f:
                text = f.read()
        except OSError as e:
            raise ValueError(f"--onsets: JSON text or a readable JSON file expected, got {setting!r} ({e.strerror})") from None
    try:
        doc = json.loads(text)
    except json.JSONDecodeError as e:
        raise ValueError(f"--onsets: not JSON ({e})") from None
    model_args.onsets_bars = json.dumps(onsets_bars(doc))
    return model_args.onsets_bars


def check_density(model_args):
    """--min_notes_per_bar / --max_notes_per_bar as the density control word lo + 256 hi (None: neither flag); host code
    only, ValueError that names the range.  Written back to model_args.density_word, which travels to the replicas
    (ModelInitializeTask puts it into the inference configuration); either flag switches --note_order on."""
    got = {}
    for flag in ("min_notes_per_bar", "max_notes_per_bar"):
        v = getattr(model_args, flag, None)
        if v is None:
            continue
        try:
            n = int(v) if not isinstance(v, (bool, float)) else None
        except (TypeError, ValueError):
            n = None
        if n is None or not NOTES_PER_BAR_MIN <= n <= NOTES_PER_BAR_MAX:
            raise ValueError(f"--{flag}: an integer in [{NOTES_PER_BAR_MIN}, {NOTES_PER_BAR_MAX}] expected, got {v!r}")
        got[flag] = n
    lo, hi = got.get("min_notes_per_bar", 0), got.get("max_notes_per_bar", 0)
    if lo and hi and hi < lo:
        raise ValueError(f"--max_notes_per_bar: not below --min_notes_per_bar expected, got {hi} < {lo}")
    word = None
    if got:
        word = lo + 256 * hi
        model_args.note_order = True
    model_args.density_word = word
    return word


def check_interval(model_args):
    """--max_leap / --max_leap_up / --max_leap_down / --no_repeat_pitch as the interval control word
    up + 256 down + 65536 u (None: none of the flags); host code only, ValueError that names the flag and the value.
    Written back to model_args.interval_word, which travels to the replicas (ModelInitializeTask puts it into the
    inference configuration).  It switches nothing else on."""
    got = {}
    for flag in ("max_leap", "max_leap_up", "max_leap_down"):
        v = getattr(model_args, flag, None)
        if v is None:
            continue
        try:
            n = int(v) if not isinstance(v, (bool, float)) else None
        except (TypeError, ValueError):
            n = None
        if n is None or not MAX_LEAP_MIN <= n <= MAX_LEAP_MAX:
            raise ValueError(f"--{flag}: an integer in [{MAX_LEAP_MIN}, {MAX_LEAP_MAX}] expected, got {v!r}")
        got[flag] = n
    for flag in ("max_leap_up", "max_leap_down"):
        if flag in got and "max_leap" in got:
            raise ValueError(f"--{flag} {got[flag]} cannot be combined with --max_leap {got['max_leap']}: --max_leap sets "
                             "both directions")
    unison = bool(getattr(model_args, "no_repeat_pitch", False))
    word = None
    if got or unison:
        word = got.get("max_leap", got.get("max_leap_up", 0)) + 256 * got.get("max_leap", got.get("max_leap_down", 0)) \
            + (65536 if unison else 0)
    model_args.interval_word = word
    return word


def read_constraints(path=None, pitch_min=None, pitch_max=None):
    """The constraint row of --logit_bias / --pitch_min / --pitch_max (None when none of them is given); host code only,
    raises (commu_amd.generate.CommuHipError, ValueError) on a malformed file or an empty range."""
    if path is None and pitch_min is None and pitch_max is None:
        return None
    from commu_amd.generate import read_logit_bias, token_constraints
    ban, bias = [], {}
    if path is not None:
        with open(path) as f:
            try:
                doc = json.load(f)
            except json.JSONDecodeError as e:
                raise ValueError(f"{path}: not JSON ({e})") from None
        ban, bias = read_logit_bias(doc)
    pitch = None
    if pitch_min is not None or pitch_max is not None:
        pitch = (0 if pitch_min is None else pitch_min, 127 if pitch_max is None else pitch_max)
    return token_constraints(ban=ban, bias=bias, pitch_range=pitch)


def read_harmony(setting=None, penalty=4.0):
    """The harmony table of --harmony / --harmony_penalty (None when the flag is not given); host code only, raises
    (commu_amd.generate.CommuHipError, ValueError) on an unreadable or ill-shaped file or a penalty that is no penalty."""
    if setting is None:
        return None
    from commu_amd.generate import harmony_rows, harmony_table
    if setting == "chord":
        return harmony_table()
    if setting == "soft":
        if isinstance(penalty, bool) or not isinstance(penalty, (int, float)) or not 0 <= penalty < float("inf"):
            raise ValueError(f"--harmony_penalty: a finite number >= 0 expected, got {penalty!r}")
        return harmony_table(outside=-float(penalty))
    try:
        with open(setting) as f:
            doc = json.load(f)
    except OSError as e:
        raise ValueError(f"--harmony: chord, soft or a readable JSON file expected, got {setting!r} ({e.strerror})") from None
    except json.JSONDecodeError as e:
        raise ValueError(f"--harmony: {setting}: not JSON ({e})") from None
    if not isinstance(doc, list) or len(doc) != 110 or not all(isinstance(r, list) and len(r) == 12 for r in doc):
        raise ValueError(f"--harmony: {setting}: a list of 110 rows of 12 numbers (null: banned) expected")
    if not all(v is None or (isinstance(v, (int, float)) and not isinstance(v, bool)) for r in doc for v in r):
        raise ValueError(f"--harmony: {setting}: a list of 110 rows of 12 numbers (null: banned) expected")
    return harmony_rows([[float("-inf") if v is None else float(v) for v in r] for r in doc])


def read_class_sampling_arg(setting=None, grammar=False):
    """--class_sampling as the JSON text of its validated document (None when the flag is not given): the value is the
    document itself or the path of a file that holds it.  Host code only; raises (commu_amd.generate.CommuHipError,
    ValueError) on an unreadable value, a malformed document, and on `drawn` names without --grammar."""
    if setting is None:
        return None
    from commu_amd.generate import read_class_sampling
    text = setting
    if not setting.lstrip().startswith("{"):
        try:
            with open(setting) as f:
                text = f.read()
        except OSError as e:
            raise ValueError(f"--class_sampling: a JSON object or a readable JSON file expected, got {setting!r} "
                             f"({e.strerror})") from None
    try:
        doc = json.loads(text)
    except json.JSONDecodeError as e:
        raise ValueError(f"--class_sampling: not JSON ({e})") from None
    _, uses_drawn = read_class_sampling(doc)
    if uses_drawn and not grammar:
        names = sorted(k for k in doc if k != "after")
        raise ValueError(f"--class_sampling: {', '.join(names)} name what is drawn next, which only --grammar fixes from the "
                         "previous token; give --grammar, or key the controls by the previous token's class with "
                         "{\"after\": {...}}")
    return json.dumps(doc)


from commu_amd.midi_generator.replicas import (generate_on_device, generate_requests_on_device, replica_worker,  # noqa: E402
                                               split_num_generate)


def main_requests(model_args, input_args, requests, harmony, want_lp, training_cfg=None, device_index=0):
    """--requests: every request of the file through PreprocessTask, all of them decoded in one pool on one GPU, and
    sequences.json = {"requests": [{"encoded_meta", "sequences", "attempts" (, "logprobs")}, ...]} in file order."""
    for r in requests:          # (malformed constraints are refused before a model is loaded)
        r["logit_bias"] = read_constraints(r.pop("logit_bias", None), r.pop("pitch_min", None), r.pop("pitch_max", None))
    results = generate_requests_on_device(model_args, requests, device_index, training_cfg, want_lp, harmony)
    os.makedirs(input_args.output_dir, exist_ok=True)
    with open(os.path.join(input_args.output_dir, "sequences.json"), "w") as f:
        json.dump({"requests": results}, f)
    return [r["sequences"] for r in results]


def main(model_args, input_args, training_cfg=None, device_indices=None):
    """`num_generate` sequences are independent (the reference produces them one after the other,
    midi_inferrer.py:338-354): with several GPUs visible they are split across them as REPLICAS -- one process per
    GPU, each with its own model copy and its share, no collective -- and concatenated in
    device order.  --gpus 1 (or one visible device) keeps everything in this process.  `device_indices` (tests):
    explicit device of every replica, e.g. [0, 0] = two replica processes on the one GPU of a test box."""
    import torch
    requests = check_requests(model_args, input_args)   # (refused before a model is loaded or a replica started)
    check_share_prompt(model_args, input_args)          # (likewise)
    check_decode_slots(model_args)                      # (likewise)
    check_voices(model_args)                            # (likewise; ahead of the note order, which it switches on)
    check_density(model_args)                           # (likewise)
    check_interval(model_args)                          # (likewise)
    check_onsets(model_args)                            # (likewise)
    check_guide(model_args, input_args)                 # (likewise)
    check_articulation(model_args, needs_guide=requests is None)      # (likewise)
    check_form(model_args)                              # (likewise)
    check_note_order(model_args)                        # (likewise)
    in_args = dict(vars(input_args))
    in_args.pop("requests", None)
    max_rounds = in_args.pop("max_rounds", None)
    gpus = in_args.pop("gpus", None)
    want_lp = bool(in_args.pop("logprobs", False))
    prompt_file = in_args.pop("prompt_tokens", None)
    prompt = read_prompt_tokens(prompt_file) if prompt_file else None
    # (refused here when malformed: before a model is loaded or a replica started)
    logit_bias = read_constraints(in_args.pop("logit_bias", None), in_args.pop("pitch_min", None),
                                  in_args.pop("pitch_max", None))
    harmony = read_harmony(getattr(model_args, "harmony", None), getattr(model_args, "harmony_penalty", 4.0))      # (likewise)
    # (likewise; the checked document travels to the replicas in model_args, ModelInitializeTask puts it into the
    # inference configuration)
    if getattr(model_args, "class_sampling", None) is not None:
        model_args.class_sampling = read_class_sampling_arg(model_args.class_sampling, bool(getattr(model_args, "grammar", False)))
    if requests is not None:
        return main_requests(model_args, input_args, requests, harmony, want_lp, training_cfg,
                             0 if device_indices is None else device_indices[0])
    if device_indices is None:
        n_vis = torch.cuda.device_count()
        device_indices = list(range(max(1, n_vis if gpus is None else min(gpus, n_vis))))
    shares = split_num_generate(in_args["num_generate"], len(device_indices))
    if len(shares) == 1:
        encoded_meta, sequences, *lps = generate_on_device(model_args, in_args, device_indices[0], shares[0], 0, max_rounds,
                                                           training_cfg, want_lp, prompt, logit_bias, harmony)
        logprobs = lps[0] if want_lp else None
    else:
        import torch.multiprocessing as mp
        ctx = mp.get_context("spawn")          # (never fork / exec a process that has initialised the GPU)
        q = ctx.Queue()
        procs = [ctx.Process(target=replica_worker, args=(r, device_indices[r], model_args, in_args, share, max_rounds,
                                                    training_cfg, q, want_lp, prompt, logit_bias, harmony))
                 for r, share in enumerate(shares)]
        for p_ in procs:
            p_.start()
        # a replica that dies natively (GPU fault, OOM kill) never reports: poll the queue and the processes
        import queue as _queue
        results = {}
        while len(results) < len(procs):
            try:
                k_, v_ = q.get(timeout=1.0)
                results[k_] = v_
            except _queue.Empty:
                dead = [(r, p_.exitcode) for r, p_ in enumerate(procs)
                        if r not in results and not p_.is_alive() and p_.exitcode not in (None, 0)]
                if dead:
                    for p_ in procs:
                        if p_.is_alive():
                            p_.terminate()
                    raise RuntimeError(f"generation replica {dead[0][0]} died with exit code {dead[0][1]}")
        for p_ in procs:
            p_.join()
        bad = [v for v in results.values() if isinstance(v, str)]
        if bad:
            raise RuntimeError("generation replica failed:\n" + bad[0])
        encoded_meta = results[0][0]
        sequences = [seq for r in range(len(shares)) for seq in results[r][1]]
        logprobs = [lp for r in range(len(shares)) for lp in results[r][2]] if want_lp else None
    os.makedirs(input_args.output_dir, exist_ok=True)
    with open(os.path.join(input_args.output_dir, "sequences.json"), "w") as f:
        doc = {"encoded_meta": encoded_meta, "sequences": sequences}
        if want_lp:
            doc["logprobs"] = logprobs
        json.dump(doc, f)
    return sequences


if __name__ == "__main__":
    margs, _ = parse_args()["model_args"].parse_known_args()
    iargs, _ = parse_args()["input_args"].parse_known_args()
    main(margs, iargs)
