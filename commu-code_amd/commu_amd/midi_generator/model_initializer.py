"""Checkpoint -> generation-ready model (the reference's ModelInitializeTask,
commu/midi_generator/model_initializer.py:13-56).

`execute()` does what the reference does with a checkpoint file: build `MemTransformerLM` from the training
defaults with `same_length = True` (:36-41), load `checkpoint["model"]` with `strict=False` (:43-47), move to the
device, `eval()`, `reset_length(1, inference_cfg.MODEL.memory_length)` (:48-50).  The file may have been written
by the reference's train.py (:29-54) -- its pickle then names `commu.model.dataset.BaseVocab`, which
`commu_amd.train.read_checkpoint` maps onto this package's class -- or by `commu_amd.train.save_checkpoint`.
The model this returns runs on the GPU only (no CPU fallback).
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Tuple

import torch

from ..model.config_helper import get_default_cfg_inference, get_default_cfg_training
from ..model.dataset import BaseVocab
from ..model.model import MemTransformerLM
from ..train import read_checkpoint


class ModelInitializeTask:
    def __init__(self, model_args, map_location: str = "cpu", device: Optional[torch.device] = None,
                 training_cfg=None):
        """model_args: anything with `.checkpoint_dir` (path of the checkpoint FILE, as in generate.py --checkpoint_dir).
        training_cfg: override of the training defaults for checkpoints of another shape (the reference always
        rebuilds the default shape, quirk Q11)."""
        self.model_args = model_args
        self.map_location = map_location
        self.device = device if device is not None else torch.device("cuda")
        self.inference_cfg = self.initialize_inference_config()
        self._training_cfg = training_cfg

    def initialize_inference_config(self):
        cfg = get_default_cfg_inference()
        # generate.py --memory_length / --generation_length / --sliding_memory (not in the reference, whose inference
        # configuration is fixed at 4146 / 4096 and whose memory always slides)
        mlen, glen = getattr(self.model_args, "memory_length", None), getattr(self.model_args, "generation_length", None)
        cfg.defrost()
        if mlen is not None:
            cfg.MODEL.memory_length = int(mlen)
        if glen is not None:
            cfg.GENERATION.generation_length = int(glen)
        if getattr(self.model_args, "sliding_memory", False):
            cfg.GENERATION.sliding_memory = True
        # generate.py --kv_cache (not in the reference): storage of the decode step's K/V cache, "bf16" or "fp8"
        if getattr(self.model_args, "kv_cache", None) not in (None, "bf16"):
            cfg.GENERATION.kv_cache = str(self.model_args.kv_cache)
        # generate.py --share_prompt (not in the reference): one K/V copy of the prompt for all decode slots
        if getattr(self.model_args, "share_prompt", False):
            cfg.GENERATION.share_prompt = True
        # generate.py --grammar (not in the reference): the default event grammar on every draw
        if getattr(self.model_args, "grammar", False):
            cfg.GENERATION.grammar = True
        # generate.py --class_sampling (not in the reference): sampling controls per token class, the JSON text of the
        # document (generate.read_class_sampling)
        if getattr(self.model_args, "class_sampling", None):
            cfg.GENERATION.class_sampling = str(self.model_args.class_sampling)
        # generate.py --note_order / --max_notes (not in the reference): the note-order control word, 0 = on, N = on with
        # at most N notes per position (generate.py check_note_order)
        word = getattr(self.model_args, "note_order_word", None)
        if word is None and getattr(self.model_args, "max_notes", None) is not None:      # (a caller that skipped the check)
            word = int(self.model_args.max_notes)
        elif word is None and getattr(self.model_args, "note_order", False):
            word = 0
        if word is not None:
            cfg.GENERATION.note_order = int(word)
        # generate.py --max_voices / --no_restrike (not in the reference): the voice word N + 256 r (generate.py check_voices)
        vword = getattr(self.model_args, "voices_word", None)
        if vword is None and (getattr(self.model_args, "max_voices", None) is not None
                              or getattr(self.model_args, "no_restrike", False)):      # (a caller that skipped the check)
            vword = int(getattr(self.model_args, "max_voices", None) or 0) \
                + (256 if getattr(self.model_args, "no_restrike", False) else 0)
        if vword is not None:
            cfg.GENERATION.voices = int(vword)
        # generate.py --min_notes_per_bar / --max_notes_per_bar (not in the reference): the density word lo + 256 hi
        # (generate.py check_density)
        dword = getattr(self.model_args, "density_word", None)
        if dword is None and (getattr(self.model_args, "min_notes_per_bar", None) is not None
                              or getattr(self.model_args, "max_notes_per_bar", None) is not None):   # (a caller that skipped the check)
            dword = int(getattr(self.model_args, "min_notes_per_bar", None) or 0) \
                + 256 * int(getattr(self.model_args, "max_notes_per_bar", None) or 0)
        if dword is not None:
            cfg.GENERATION.density = int(dword)
        # generate.py --max_leap / --max_leap_up / --max_leap_down / --no_repeat_pitch (not in the reference): the interval
        # word up + 256 down + 65536 u (generate.py check_interval)
        iword = getattr(self.model_args, "interval_word", None)
        if iword is not None:
            cfg.GENERATION.interval = int(iword)
        # generate.py --onsets (not in the reference): the onset template as the JSON text of its list of bars
        # (generate.py check_onsets)
        if getattr(self.model_args, "onsets_bars", None) is not None:
            cfg.GENERATION.onsets = str(self.model_args.onsets_bars)
        # generate.py --guide (not in the reference): the guide track as the JSON text of its raw form (generate.py
        # check_guide)
        if getattr(self.model_args, "guide_doc", None) is not None:
            cfg.GENERATION.guide = str(self.model_args.guide_doc)
        # generate.py --articulation (not in the reference): the articulation as the JSON text of its full form (generate.py
        # check_articulation)
        if getattr(self.model_args, "articulation_doc", None) is not None:
            cfg.GENERATION.articulation = str(self.model_args.articulation_doc)
        # generate.py --form (not in the reference): the form as the JSON text of its bars (generate.py check_form)
        if getattr(self.model_args, "form_doc", None) is not None:
            cfg.GENERATION.form = str(self.model_args.form_doc)
        # generate.py --decode_slots (not in the reference): attempts decoded side by side (64 unless the key is set)
        if getattr(self.model_args, "decode_slots", None) not in (None, 64):
            cfg.GENERATION.decode_slots = int(self.model_args.decode_slots)
        cfg.freeze()
        return cfg

    def load_checkpoint_fp(self) -> Tuple[Path, Path]:                       # :25-34
        checkpoint_dir = getattr(self.model_args, "checkpoint_dir", None)
        if checkpoint_dir:
            model_fp = Path(checkpoint_dir)
            return model_fp, model_fp.parent / "config.yml"
        # (the reference falls back to inference_cfg.MODEL.model_directory / checkpoint_name here, fields its own
        #  config does not define: config_helper.py:61-80)
        raise ValueError("--checkpoint_dir (path of the checkpoint file) is required")

    def initialize_training_cfg(self):                                        # :36-41
        cfg = self._training_cfg if self._training_cfg is not None else get_default_cfg_training()
        cfg.defrost()
        cfg.MODEL.same_length = True
        cfg.freeze()
        return cfg

    def initialize_model(self, training_cfg, model_fp):                       # :43-51
        model = MemTransformerLM(training_cfg, BaseVocab())
        checkpoint = read_checkpoint(model_fp, self.map_location)
        model.load_state_dict(checkpoint["model"], strict=False)
        model = model.to(self.device)
        model.eval()
        model.reset_length(1, self.inference_cfg.MODEL.memory_length)
        # generate.py --parity (not in the reference): the fp32 arithmetic of the reference instead of bf16 operands
        model.parity_fp32 = bool(getattr(self.model_args, "parity", False))
        return model

    def execute(self):                                                        # :53-56
        model_fp, _ = self.load_checkpoint_fp()          # (config.yml next to it is never read: quirk Q11)
        return self.initialize_model(self.initialize_training_cfg(), model_fp)
