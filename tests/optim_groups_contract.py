"""Float64 contract of the grouped optimiser step (csrc/optim_groups.hip: commu_adam_step_groups, its _dev form and
commu_grad_norm_groups).  Plain module in the style of train_contract.py: torch and numpy on the CPU, nothing from the library.

  grouped_ref   float64 over the fp32 inputs, coupled (torch.optim.Adam) and decoupled (torch.optim.AdamW), per-group
                lr / weight decay / frozen flag from a block map (one group number per 64-element block).
  grouped_emu   the same in fp32 as the kernel computes it, with named, plantable DEFECTS -- each the image of one line of the
                kernel going wrong.
  grouped_check the project's own Adam bounds (train_contract.adam_check: 1e-6 of max|p| on p, m, v; the bf16 shadow within
                2^-8 of its element) on the trainable elements, and the guards that have no tolerance: frozen blocks
                bit-identical in all four buffers (the shadow starts as SENT), the gaps after every tensor still zero.
  norm_check    the float64 root of the trainable blocks' sum of squares within train_contract.grad_norm_bound.

tests/test_optim_groups_host.py proves grouped_ref against torch.optim.Adam / AdamW, shows every defect caught on the input
sets below and the clean emulation inside the bounds; tests/test_optim_groups_gpu.py holds the kernels to the same checks.

INPUT SETS.  Tensors of numel 1, 63, 64, 65, 127, 128, 1000, 4099 in this order, each padded to a multiple of 64 (every way a
tensor can end inside or on a block boundary), groups assigned round-robin so that neighbours always differ.  Four groups:
0 default with decay, 1 no decay, 2 half the learning rate (with decay, so that a decay taken with the base lr shows), 3 frozen.
The large set, 4096 * 1024 + 64 * 5 elements, has its group changes inside the part the kernel's grid (at most 4096
workgroups of 1024 elements) reaches only by striding.  State starts non-zero, as train_contract.adam_inputs does."""
import math

import numpy as np

from train_contract import (ADAM_B1, ADAM_B2, ADAM_CLIP, ADAM_EPS, ADAM_LR, ADAM_STEP, F32, SENT, adam_check, adam_inputs,
                            adam_ref, bf16_round, bias_corrections32, clip_coef32, grad_norm_bound, ratio)

BLOCK = 64
NUMELS = (1, 63, 64, 65, 127, 128, 1000, 4099)
BIG_NUMELS = (4096 * 1024, 40, 64, 1, 65)          # 4096 * 1024 + 64 * 5 elements after padding
WD = 0.1
# (lr multiplier, weight decay, frozen)
GROUPS = ((1.0, WD, False), (1.0, 0.0, False), (0.5, WD, False), (1.0, WD, True))
SETS = {"small": NUMELS, "rotated": NUMELS[3:] + NUMELS[:3], "big": BIG_NUMELS}
SET_SHIFT = {"small": 0, "rotated": 1, "big": 0}
NORM_NPART = {"small": 1, "rotated": 4, "big": 256}
DEFECTS = ("decay_scaled_by_clip", "decoupled_base_lr", "frozen_moments_move", "frozen_shadow_written",
           "last_block_next_group", "group_of_first_pass", "norm_counts_frozen")
GRID_ELEMS = 4096 * 1024          # what one pass of the capped grid covers


def padded(numel):
    return (numel + BLOCK - 1) // BLOCK * BLOCK


def layout(numels, tensor_group):
    """offsets, total, block map (uint8 per block), element mask of real (non-gap) elements"""
    offs, total = [], 0
    for k in numels:
        offs.append(total)
        total += padded(k)
    bmap = np.zeros(total // BLOCK, dtype=np.uint8)
    real = np.zeros(total, dtype=bool)
    for off, k, grp in zip(offs, numels, tensor_group):
        bmap[off // BLOCK:(off + padded(k)) // BLOCK] = grp
        real[off:off + k] = True
    return offs, total, bmap, real


class GroupedInputs:
    """Flat fp32 p, g, m, v with zero gaps; tensor_group; block map; the groups' lr / wd / frozen lists."""

    def __init__(self, name, one_group=False):
        self.name, self.numels = name, SETS[name]
        ng = len(GROUPS)
        self.tensor_group = [0 if one_group else (i + SET_SHIFT[name]) % ng for i in range(len(self.numels))]
        self.offs, self.n, self.bmap, self.real = layout(self.numels, self.tensor_group)
        p, g, m, v = adam_inputs(self.n, seed=len(name))
        z = F32(0)
        self.p, self.g, self.m, self.v = (np.where(self.real, t, z).astype(F32) for t in (p, g, m, v))
        groups = ((1.0, 0.0, False),) if one_group else GROUPS
        self.lrs = [float(F32(F32(ADAM_LR) * F32(mult))) for mult, _, _ in groups]
        self.wds = [wd for _, wd, _ in groups]
        self.frozen = [fr for _, _, fr in groups]
        self.elem_group = np.repeat(self.bmap, BLOCK)
        self.elem_frozen = np.asarray(self.frozen)[self.elem_group]
        assert all(a != b for a, b in zip(self.tensor_group, self.tensor_group[1:])) or one_group


def standard_scalars(gnorm=2.0):
    """coef, bc1, bc2 as the fp32 values the kernel works with (a clip that bites: coef = 0.125)"""
    bc1, bc2 = bias_corrections32(ADAM_B1, ADAM_B2, ADAM_STEP)
    return clip_coef32(gnorm, ADAM_CLIP), bc1, bc2


def grouped_ref(p, g, m, v, bmap, lrs, wds, frozen, coef, bc1, bc2, decoupled, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """float64 on the fp32 inputs; lrs / wds are the per-group values the kernel receives (rounded to fp32 here as there).
    Frozen elements come back as they went in."""
    eg = np.repeat(np.asarray(bmap), BLOCK)
    lr = np.array([float(F32(x)) for x in lrs])[eg]
    wd = np.array([float(F32(x)) for x in wds])[eg]
    fr = np.asarray(frozen)[eg]
    p64, g64, m64, v64 = (t.astype(np.float64) for t in (p, g, m, v))
    b1, b2, eps = (float(F32(t)) for t in (b1, b2, eps))
    gr = g64 * float(coef)
    pe = p64
    if decoupled:
        pe = p64 * (1.0 - lr * wd)
    else:
        gr = gr + wd * p64
    mm = b1 * m64 + (1 - b1) * gr
    vv = b2 * v64 + (1 - b2) * gr * gr
    pn = pe - (lr / float(bc1)) * mm / (np.sqrt(vv) / math.sqrt(float(bc2)) + eps)
    return np.where(fr, p64, pn), np.where(fr, m64, mm), np.where(fr, v64, vv)


def grouped_emu(p, g, m, v, bmap, lrs, wds, frozen, coef, bc1, bc2, decoupled, defect=None, tensor_blocks=None):
    """adam_groups_kernel in fp32: the group byte of an element's block, the table {lr_k / bc1, wd_k, 1 - lr_k wd_k, frozen},
    the capped grid and its stride.  tensor_blocks (first block, blocks, group of the NEXT tensor) feeds the
    last_block_next_group defect.  Returns p, m, v, shadow (shadow starts as SENT)."""
    n = p.shape[0]
    bm = np.asarray(bmap).copy()
    if defect == "last_block_next_group":                                      # DEFECT: a tensor's last block takes the next tensor's group
        for first, nb, nxt in tensor_blocks:
            if nxt is not None:
                bm[first + nb - 1] = nxt
    eg = np.repeat(bm, BLOCK)
    if defect == "group_of_first_pass":                                        # DEFECT: the group byte is read before the stride loop
        idx = np.arange(n)
        eg = eg[idx % GRID_ELEMS] if n > GRID_ELEMS else eg
    b1, b2, eps = F32(ADAM_B1), F32(ADAM_B2), F32(ADAM_EPS)
    lr32, wd32 = np.array(lrs, dtype=F32), np.array(wds, dtype=F32)
    step = (lr32 / F32(bc1)).astype(F32)[eg]
    wd = wd32[eg]
    keep_lr = np.full_like(lr32, lr32[0]) if defect == "decoupled_base_lr" else lr32          # DEFECT: the base lr in 1 - lr wd
    keep = (F32(1) - keep_lr * wd32).astype(F32)[eg]
    fr = np.asarray(frozen)[eg]
    isb2 = F32(1) / np.sqrt(F32(bc2))
    gr = (g * F32(coef)).astype(F32)
    pe = p
    if decoupled:
        pe = (p * keep).astype(F32)
    elif defect == "decay_scaled_by_clip":                                     # DEFECT: coef (g + wd p)
        gr = ((g + wd * p).astype(F32) * F32(coef)).astype(F32)
    else:
        gr = (gr + (wd * p).astype(F32)).astype(F32)
    mm = (b1 * m + (F32(1) - b1) * gr).astype(F32)
    vv = (b2 * v + (F32(1) - b2) * gr * gr).astype(F32)
    pn = (pe - step * mm / (np.sqrt(vv) * isb2 + eps)).astype(F32)
    po = np.where(fr, p, pn).astype(F32)
    move = fr & (defect != "frozen_moments_move")                              # DEFECT: m and v of a frozen block are updated
    mo, vo = np.where(move, m, mm).astype(F32), np.where(move, v, vv).astype(F32)
    pb = np.where(fr, F32(SENT), bf16_round(po)).astype(F32)
    if defect == "frozen_shadow_written":                                      # DEFECT: the shadow of a frozen block is stored
        pb = bf16_round(po)
    return po, mo, vo, pb


def tensor_blocks(inp):
    out = []
    for i, (off, k) in enumerate(zip(inp.offs, inp.numels)):
        nxt = inp.tensor_group[i + 1] if i + 1 < len(inp.numels) else None
        out.append((off // BLOCK, padded(k) // BLOCK, nxt))
    return out


def grouped_check(inp, want, p, m, v, pb, pb_before=None):
    """Worst ratios by name.  `want` from grouped_ref on inp's buffers (inp: anything with p, m, v, real, elem_frozen);
    p, m, v, pb what the step left; pb started as pb_before (None: as SENT everywhere)."""
    live = ~inp.elem_frozen
    res = adam_check(tuple(w[live] for w in want), p[live], m[live], v[live], pb[live])
    fz = inp.elem_frozen
    same = all(np.array_equal(a[fz], b[fz]) for a, b in ((p, inp.p), (m, inp.m), (v, inp.v)))
    same = same and bool(np.all(pb[fz] == SENT) if pb_before is None else np.array_equal(pb[fz], pb_before[fz]))
    res["frozen"] = 0.0 if same else float("inf")
    gap = ~inp.real & live
    res["gaps"] = 0.0 if all(bool(np.all(t[gap] == 0.0)) for t in (p, m, v, pb)) else float("inf")
    return res


def norm_inputs(inp, poison=True):
    """the gradient buffer for the norm: frozen blocks filled with NaN, so that a finite result proves they are never read"""
    g = inp.g.copy()
    if poison:
        g[inp.elem_frozen] = np.nan
    return g


def norm_ref(inp):
    g = inp.g.astype(np.float64)
    return math.sqrt(float((g[~inp.elem_frozen] ** 2).sum()))


def norm_check(inp, npart, got):
    want = norm_ref(inp)
    return ratio(got, want, grad_norm_bound(inp.n, npart, want))


def norm_emu(inp, npart, defect=None):
    """sumsq_groups_partial_kernel + final in fp32 through train_contract.grad_norm_emu's loop: frozen units count as zero."""
    from train_contract import grad_norm_emu
    g = norm_inputs(inp)
    if defect != "norm_counts_frozen":                                         # DEFECT: the frozen test is lost
        g = np.where(inp.elem_frozen, F32(0), g).astype(F32)
    return grad_norm_emu(g, npart)
