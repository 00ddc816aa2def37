"""The layer-tail / head contract (tests/tail_contract.py) for launches of 65 .. 256 sequences: row groups 4 .. 15.

What tail_contract.py says about a stage -- the products, the LayerNorm rule, the bounds C_PROD and TAU, run() and check() --
does not depend on the number of sequences and is taken from there unchanged.  What it pins to four row groups is restated
here for sixteen:

  * the arrival counters: [3 phases][G row groups][CNT_STRIDE] words with G = 4 up to 64 sequences and 16 beyond
    (commu_decode_tail_sync_words_for), so counter (p, mg) is word (p G + mg) CNT_STRIDE -- counter_words(), buffers();
  * the 64-row pool of vec / h rows: rows 64 .. 255 are drawn from the same fixed pool of values (tail_contract._rng);
  * the defects that index row groups: `group0` for any number of groups, and a new one, `group_alias` -- rows >= 64 read
    the hand-off buffers of row - 64, which is what a kernel that kept `mg & 3` anywhere would compute.

INPUTS beyond tail_contract's: in the LOGITS sets row 2, row 67 (row group 4) and the last row are inactive."""
import contextlib
import functools
import math

import torch

import tail_contract as TC
from tail_contract import (BF16, C_PROD, CNT_STRIDE, NGRP, PAD, SENT, SYNC_SENT, TAU, V, bf, ln32, ln64, ln_rule,  # noqa: F401
                           prod32, prod64, worst, window, head_buffers, head_run, head_check, head_worst)

MAX_B = 256
LAYERS = 6          # the head launch clears the counters of this many layer-tail launches


def groups(B):
    """G of a launch of B sequences."""
    return 4 if B <= 64 else MAX_B // 16


def sync_words(B):
    return 3 * groups(B) * CNT_STRIDE


def counter_words(s):
    ngroups = (max(s.rows) + 16) // 16
    return [(p * s.G + mg) * CNT_STRIDE for p in range(3) for mg in range(ngroups)]


@contextlib.contextmanager
def _sixteen_groups():
    """tail_contract.run / check look the counter words up by name in their own module: give them this module's."""
    keep = TC.counter_words
    TC.counter_words = counter_words
    try:
        yield
    finally:
        TC.counter_words = keep


@functools.lru_cache(maxsize=8)
def _extra_rows(shape, seed):
    """Rows 64 .. 255 of the vec / h pool (rows 0 .. 63 are tail_contract._weights')."""
    D, DI, HD = TC.SHAPES[shape]
    _, rn = TC._rng(seed + 1)
    return bf(rn(MAX_B - 64, HD)), bf(rn(MAX_B - 64, D))


def build_tail(shape, B, mode, d_ln):
    assert 64 < B <= MAX_B
    s = TC.build_tail(shape, 64, mode, d_ln)          # weights, parameters and rows 0 .. 63 (row 0 tiny, row 1 big)
    vec_x, h_x = _extra_rows(shape, 7000 + s.D + s.HD + s.Nn)
    s.B, s.G = B, groups(B)
    s.vec, s.h = torch.cat([s.vec, vec_x[:B - 64]]), torch.cat([s.h, h_x[:B - 64]])
    s.h[:, d_ln:] = math.nan
    s.rows = list(range(B))
    s.active = None
    if mode == "logits":
        s.active = torch.ones(B, dtype=torch.uint8)
        s.active[[2, 67, B - 1]] = 0
    return s


def buffers(s):
    """tail_contract.buffers with a sync block of 3 G CNT_STRIDE words (+ 64 guard words)."""
    B = s.B
    out_dt = torch.float32 if s.mode == "logits" else BF16
    nout = 736 if s.mode == "logits" else s.Nn + PAD
    b = dict(z1=torch.full((B + 2, s.D), SENT, dtype=BF16), hid=torch.full((B + 2, s.DI), SENT, dtype=BF16),
             z2=torch.full((B + 2, s.D), SENT, dtype=BF16), h_out=torch.full((B + 2, s.D + PAD), SENT, dtype=BF16),
             out=torch.full((B + 2, nout), SENT, dtype=out_dt),
             sync=torch.full((3 * s.G * CNT_STRIDE + 64,), SYNC_SENT, dtype=torch.int32), err=torch.zeros(1, dtype=torch.int32))
    for w in counter_words(s):
        b["sync"][w] = 0
    return b


def run(s, b, defect=None, stage="", use_active=True, base=None):
    if defect in ("group0", "group_alias"):
        return _run_groups(s, b, defect, stage, base)
    with _sixteen_groups():
        return TC.run(s, b, defect, stage, use_active, base)


def check(s, b, use_active=True, stages=TC._ORDER):
    with _sixteen_groups():
        return TC.check(s, b, use_active, stages)


def _run_groups(s, b, defect, stage, base):
    """The honest launch `base` with ONE stage reading other rows of the hand-off buffer it consumes: group0 -- row r reads
    row r % 16; group_alias -- row r >= 64 reads row r - 64.  (Rows that the sub-batch does not hold read zeros.)"""
    src = (lambda r: r % 16) if defect == "group0" else (lambda r: r - 64 if r >= 64 else r)

    def moved(t):
        full = torch.zeros(MAX_B, t.shape[1], dtype=t.dtype)
        full[s.rows] = t
        return full[[src(r) for r in s.rows]]
    B = s.B
    for k, v in base.items():
        b[k] = v.clone() if isinstance(v, torch.Tensor) else v
    pre = base["_pre"]
    if stage == "S2":
        a = bf(ln32(moved(base["z1"][:B]).float(), s.g1, s.be1, s.eps1, s.d_ln))
        b["hid"][:B] = bf(torch.relu(prod32(a, s.W1) + s.b1))
    elif stage == "S3":
        b["z2"][:B] = bf(prod32(moved(base["hid"][:B]), s.W2) + (s.b2 + bf(pre["LN1"]).float()))
    else:
        assert stage == "S4a"
        b["h_out"][:B, :s.D] = bf(ln32(moved(base["z2"][:B]).float(), s.g2, s.be2, s.eps2, s.d_ln))
    return b


GROUP_DEFECTS = {"group0": ("S2", "S3", "S4a"), "group_alias": ("S2", "S3", "S4a")}
DEFECTS = {**{d: st for d, st in TC.DEFECTS.items() if d != "group0"}, **GROUP_DEFECTS}


def applicable(s, defect, stage):
    if defect == "group0":
        return max(s.rows) >= 16
    if defect == "group_alias":
        return max(s.rows) >= 64
    return TC.applicable(s, defect, stage)


def tail_sets():
    """(id, args of build_tail): the first row past four row groups (65), a partial last group (80, 129, 200), every row
    group (256), both modes on every template, zero-padded widths in both templates."""
    return [(f"{shape}-B{B}-{mode}-ln{d_ln}", (shape, B, mode, d_ln)) for shape, B, mode, d_ln in (
        ("n512", 65, "qkv", 512), ("n512", 80, "logits", 512), ("n512", 256, "qkv", 512), ("n512", 256, "logits", 512),
        ("n640", 129, "logits", 500), ("n640", 200, "qkv", 500), ("wide", 65, "qkv", 1000), ("wide", 256, "logits", 1024))]


def defect_rows(s):
    """The sub-batch on which the host test plants defects: the special rows, the inactive ones, and the first row of
    every row group in use (so that row r - 64 of every row r >= 64 in it is there too)."""
    rows = {0, 1, 2, s.B - 1} | set(range(0, s.B, 16))
    if s.B > 67:
        rows.add(67)
    return sorted(rows)


def build_head(shape, B, d_true):
    s = TC.build_head(shape, B, d_true)
    s.n_zero = LAYERS * sync_words(B) + 37          # the counters of LAYERS launches of B sequences (+ 37: not a multiple of 256)
    return s


def head_sets():
    return [(f"head-{shape}-B{B}-d{d}", (shape, B, d)) for shape, B, d in (("n512", 65, 512), ("wide", 256, 1024))]
