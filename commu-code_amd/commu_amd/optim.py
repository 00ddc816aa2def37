"""Optimiser side of the training step (reference train.py:159-169,441-461) on the model's flat
fp32 buffers: global-norm clip + Adam as two kernels, no host synchronisation.

`FusedAdam` is a torch.optim.Optimizer (so LambdaLR drives every `param_groups[k]["lr"]` exactly as in
the reference, including lr == 0 on step 0), `clip_grad_norm_` mirrors
torch.nn.utils.clip_grad_norm_ (returns the total norm as a device tensor).

Beyond the reference's single group: `weight_decay` (torch.optim.Adam's coupled form, or AdamW's with `decoupled`), and
per-tensor `groups` with their own learning-rate multiplier, decay and frozen flag.  `resolve_groups` turns the group
specification into per-tensor group numbers and the block map the kernel reads; it is a pure function (no GPU, no model).
The default configuration -- one group, no decay, nothing frozen -- launches the single-group kernels as before:
`FusedAdam.kernel_name()` tells which entry point the next step uses."""
from __future__ import annotations

import fnmatch

import torch

from . import ops
from ._lib import CommuHipError

MAX_GROUPS = ops.OPTIM_MAX_GROUPS
BLOCK = 64          # model._ensure_flat(): every tensor starts at a multiple of 64 elements of the flat buffers


def lr_lambda_factory(warmup_step, lr, lr_min):
    """Inverse-sqrt schedule multiplier of the reference (train.py:448-460)."""
    def lr_lambda(step):
        if step == 0 and warmup_step == 0:
            return 1.0
        if step > warmup_step:
            return max((warmup_step ** 0.5) / (step ** 0.5), lr_min / lr)
        return step / warmup_step
    return lr_lambda


class GroupSpecError(CommuHipError, ValueError):
    """A parameter-group specification that cannot be used; the message names the offending entry."""


_GROUP_KEYS = ("match", "lr_mult", "weight_decay", "frozen")


def _number(entry, key, default):
    x = entry.get(key, default)
    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x or x in (float("inf"), float("-inf")):
        raise GroupSpecError(f"parameter group {entry!r}: '{key}' must be a finite number")
    if x < 0:
        raise GroupSpecError(f"parameter group {entry!r}: '{key}' is negative")
    return float(x)


def resolve_groups(named_numels, weight_decay=0.0, groups=None):
    """(name, numel) of every parameter tensor in model.named_parameters() order + a group specification ->
    {"groups": [{"lr_mult", "weight_decay", "frozen"}], "tensor_group": [group number per tensor], "block_map": bytes
    (one group number per 64-element block of the flat buffers)}.

    groups: list of {"match": glob or list of globs (fnmatch against the names), "lr_mult": 1.0, "weight_decay": the
    default, "frozen": False}.  The first matching entry wins; what nothing matches joins the default group
    (lr_mult 1, the default decay); entries with equal settings share a group; groups that end up empty are dropped.
    Pure: needs neither a GPU nor a model, so a command line can check a specification before it builds anything
    (with named_numels = None only the form of the specification is checked and None is returned)."""
    if isinstance(weight_decay, bool) or not isinstance(weight_decay, (int, float)) or not 0.0 <= weight_decay < float("inf"):
        raise GroupSpecError(f"weight_decay {weight_decay!r} must be a finite number >= 0")
    settings = [(1.0, float(weight_decay), False)]
    entries = []
    if groups is not None:
        if not isinstance(groups, (list, tuple)):
            raise GroupSpecError(f"parameter groups must be a list of dictionaries, got {type(groups).__name__}")
        for e in groups:
            if not isinstance(e, dict):
                raise GroupSpecError(f"parameter group {e!r} is not a dictionary")
            unknown = sorted(set(e) - set(_GROUP_KEYS))
            if unknown:
                raise GroupSpecError(f"parameter group {e!r}: unknown key(s) {unknown} (known: {list(_GROUP_KEYS)})")
            globs = e.get("match")
            globs = [globs] if isinstance(globs, str) else globs
            if not isinstance(globs, (list, tuple)) or not globs or not all(isinstance(s, str) and s for s in globs):
                raise GroupSpecError(f"parameter group {e!r}: 'match' must be a glob or a non-empty list of globs")
            frozen = e.get("frozen", False)
            if not isinstance(frozen, bool):
                raise GroupSpecError(f"parameter group {e!r}: 'frozen' must be true or false")
            entries.append((e, list(globs), (_number(e, "lr_mult", 1.0), _number(e, "weight_decay", float(weight_decay)), frozen)))
    if named_numels is None:
        return None
    named_numels = [(str(n), int(k)) for n, k in named_numels]
    names = [n for n, _ in named_numels]
    for e, globs, _ in entries:
        for pat in globs:
            if not fnmatch.filter(names, pat):
                hint = ""
                if pat.startswith("crit"):
                    hint = (" (the output projection is tied to word_emb.emb_layers.0.weight and appears once, under "
                            "that name)")
                raise GroupSpecError(f"parameter group {e!r}: glob {pat!r} matches no parameter" + hint)
    merged = []          # distinct settings in order of first appearance, the default first
    for s in settings + [s for _, _, s in entries]:
        if s not in merged:
            merged.append(s)
    choice = []
    for n in names:
        s = settings[0]
        for _, globs, es in entries:
            if any(fnmatch.fnmatchcase(n, pat) for pat in globs):
                s = es
                break
        choice.append(merged.index(s))
    used = [k for k in range(len(merged)) if k in set(choice)]
    if len(used) > MAX_GROUPS:
        raise GroupSpecError(f"{len(used)} distinct parameter groups after merging equal ones: at most {MAX_GROUPS} "
                             f"(entries {[e for e, _, _ in entries]!r})")
    renum = {k: i for i, k in enumerate(used)}
    tensor_group = [renum[k] for k in choice]
    out_groups = [dict(lr_mult=merged[k][0], weight_decay=merged[k][1], frozen=merged[k][2]) for k in used]
    if all(g["frozen"] for g in out_groups):
        raise GroupSpecError(f"every parameter is frozen (entries {[e for e, _, _ in entries]!r}): nothing to train")
    block_map = bytearray()
    for (_, numel), k in zip(named_numels, tensor_group):
        block_map += bytes([k]) * ((numel + BLOCK - 1) // BLOCK)
    return {"groups": out_groups, "tensor_group": tensor_group, "block_map": bytes(block_map)}


def load_group_spec(text):
    """--param_groups of the command line: JSON text or the path of a JSON file -> the checked list (form only)."""
    import json
    import os
    src = text
    if not text.lstrip().startswith(("[", "{")) and os.path.exists(text):
        with open(text) as f:
            src = f.read()
    try:
        spec = json.loads(src)
    except ValueError as exc:
        raise GroupSpecError(f"not JSON and not a readable file: {exc}") from None
    resolve_groups(None, 0.0, spec)
    return spec


def _flat_with_grads(model):
    fl = model._ensure_flat()
    params, offs = fl["params"], fl["offs"]
    base = fl["g"].data_ptr()
    for p, off in zip(params, offs):
        if p.grad is None:
            fl["g"][off:off + p.numel()].zero_()
        elif p.grad.data_ptr() != base + 4 * off:           # gradient produced outside the flat buffer
            fl["g"][off:off + p.numel()].copy_(p.grad.reshape(-1))
    return fl


def clip_grad_norm_(model, max_norm, optimizer=None):
    """Global L2 norm of all gradients; scales them by min(1, max_norm/(norm+1e-6)).
    With a FusedAdam `optimizer` the scaling is folded into its next step() (same arithmetic); where that optimiser has
    frozen groups the norm is over the trainable tensors only (what torch sees when frozen parameters carry no gradient)."""
    fl = _flat_with_grads(model)
    if isinstance(optimizer, FusedAdam) and optimizer.any_frozen:
        ops.grad_norm_groups(fl["g"], optimizer._block_map(fl), optimizer.frozen_flags, fl["gpart"], fl["gnorm"])
    else:
        ops.grad_norm(fl["g"], fl["gpart"], fl["gnorm"])
    if isinstance(optimizer, FusedAdam):
        optimizer._pending_clip = float(max_norm)
    else:
        ops.scale_clip(fl["g"], fl["gnorm"], float(max_norm))
    return fl["gnorm"][0]


def _describe(groups):
    return "[" + ", ".join(f"{{{n} tensors, weight_decay {wd:g}{', frozen' if fr else ''}}}" for n, wd, fr in groups) + "]"


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay) semantics (train.py:442-443) -- torch.optim.AdamW's
    with `decoupled` -- as one kernel over the flat parameter buffer; also refreshes the bf16 weight shadows.
    `groups` (see resolve_groups) gives tensors their own lr multiplier / decay / frozen flag: one torch param group per
    resolved group, keys `params`, `lr` (= lr * lr_mult; LambdaLR scales each from its own initial_lr), `weight_decay`,
    `frozen`."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, groups=None):
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or lr < 0:
            raise GroupSpecError(f"lr {lr!r} must be a number >= 0")
        named = list(model.named_parameters())
        res = resolve_groups([(n, p.numel()) for n, p in named], weight_decay, groups)
        self.resolved = res
        self.tensor_group = res["tensor_group"]
        # torch numbers the parameters of a state_dict group after group: position in that order -> position in the model
        self._order = [i for k in range(len(res["groups"])) for i, t in enumerate(self.tensor_group) if t == k]
        pgs = [dict(params=[named[i][1] for i, t in enumerate(self.tensor_group) if t == k], lr=lr * g["lr_mult"],
                    weight_decay=g["weight_decay"], frozen=g["frozen"]) for k, g in enumerate(res["groups"])]
        super().__init__(pgs, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, frozen=False))
        self.model = model
        self.decoupled = bool(decoupled)
        g0 = res["groups"][0]
        self._plain = len(res["groups"]) == 1 and g0["lr_mult"] == 1.0 and g0["weight_decay"] == 0.0 and not g0["frozen"]
        self.frozen_flags = [bool(g["frozen"]) for g in res["groups"]]          # (fixed for the optimiser's life)
        self.any_frozen = any(self.frozen_flags)
        self.step_count = 0
        self._pending_clip = None
        self.dev_scalars = None          # fp32 device tensor {lr, 1 - b1^t, 1 - b2^t}: see step()
        self.dev_table = None            # fp32 device tensor of ops.group_table: the grouped step's form of dev_scalars
        self._map_dev = None

    def kernel_name(self):
        """The entry point the next step() launches: the single-group kernels whenever there is one group with
        lr_mult 1, no decay and nothing frozen."""
        name = "commu_adam_step" if self._plain else "commu_adam_step_groups"
        return name + ("_dev" if self.dev_scalars is not None else "")

    def _block_map(self, fl):
        if self._map_dev is None or self._map_dev[0] != fl["p"].data_ptr():
            bm = self.resolved["block_map"]
            if len(bm) * BLOCK != fl["total"]:
                raise CommuHipError(f"block map of {len(bm)} blocks against flat buffers of {fl['total']} elements")
            self._map_dev = (fl["p"].data_ptr(), torch.frombuffer(bytearray(bm), dtype=torch.uint8).to(fl["dev"]))
        return self._map_dev[1]

    def group_table(self, bc1, bc2):
        """Host tensor for `dev_table`: this step's bias corrections and every group's current lr / decay / frozen flag."""
        pg = self.param_groups
        return ops.group_table([float(g["lr"]) for g in pg], [float(g["weight_decay"]) for g in pg], self.frozen_flags, bc1, bc2)

    @torch.no_grad()
    def step(self, closure=None):
        fl = _flat_with_grads(self.model)
        if fl["m"] is None:
            fl["m"] = torch.zeros_like(fl["p"])
            fl["v"] = torch.zeros_like(fl["p"])
        grp = self.param_groups[0]
        clip = self._pending_clip
        self._pending_clip = None
        kw = dict(gnorm=fl["gnorm"] if clip is not None else None, clip=clip or 0.0, beta1=grp["betas"][0],
                  beta2=grp["betas"][1], eps=grp["eps"])
        if not self._plain:
            pg = self.param_groups
            if self.dev_scalars is not None:
                # graph-replayable form: the owner of the graph writes dev_table -- and advances step_count -- before
                # every replay, as it writes dev_scalars for the single-group step
                ops.adam_step_groups_dev(fl["p"], fl["g"], fl["m"], fl["v"], fl["bf16"], self._block_map(fl), self.dev_table,
                                         decoupled=self.decoupled, **kw)
            else:
                self.step_count += 1
                ops.adam_step_groups(fl["p"], fl["g"], fl["m"], fl["v"], fl["bf16"], self._block_map(fl),
                                     [float(g["lr"]) for g in pg], [float(g["weight_decay"]) for g in pg], self.frozen_flags,
                                     self.step_count, decoupled=self.decoupled, **kw)
        elif self.dev_scalars is not None:
            # graph-replayable form: lr and the bias corrections come from device memory (the owner of the graph writes
            # them -- and advances step_count -- before every replay: Trainer._graph_step)
            ops.adam_step_dev(fl["p"], fl["g"], fl["m"], fl["v"], fl["bf16"], self.dev_scalars, **kw)
        else:
            self.step_count += 1
            ops.adam_step(fl["p"], fl["g"], fl["m"], fl["v"], fl["bf16"], float(grp["lr"]), self.step_count, **kw)
        self.model._refresh_shadows(cast=False)
        fl["version"] = sum(p._version for p in fl["params"])

    # ---- checkpointing in torch.optim.Adam's own layout (train.py:39-41 saves optimizer.state_dict()): state is
    # indexed by parameter position -- group after group, which with one group is model.parameters() order as in the
    # reference.  Frozen parameters have no state entry (torch creates none for a parameter without a gradient).
    def state_dict(self):
        fl = self.model._ensure_flat()
        out_groups, pos = [], 0
        for k, pg in enumerate(self.param_groups):
            grp = {key: v for key, v in pg.items() if key != "params"}
            for key, v in (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                           ("differentiable", False), ("fused", None)):
                grp.setdefault(key, v)
            grp["params"] = list(range(pos, pos + len(pg["params"])))
            pos += len(pg["params"])
            out_groups.append(grp)
        state = {}
        if fl["m"] is not None:
            for idx, i in enumerate(self._order):
                if self.param_groups[self.tensor_group[i]]["frozen"]:
                    continue
                p, off = fl["params"][i], fl["offs"][i]
                n = p.numel()
                state[idx] = {"step": torch.tensor(float(self.step_count)),
                              "exp_avg": fl["m"][off:off + n].view(p.shape).detach().cpu().clone(),
                              "exp_avg_sq": fl["v"][off:off + n].view(p.shape).detach().cpu().clone()}
        return {"state": state, "param_groups": out_groups}

    def _grouping(self):
        return [(len(g["params"]), float(g["weight_decay"]), bool(g["frozen"])) for g in self.param_groups]

    @torch.no_grad()
    def load_state_dict(self, sd):
        fl = self.model._ensure_flat()
        groups = sd["param_groups"]
        mine = self._grouping()
        # (a state written by torch.optim.Adam / AdamW has no `frozen` key: its frozen tensors show as missing state)
        theirs = [(len(g["params"]), float(g.get("weight_decay", 0.0)),
                   bool(g.get("frozen", mine[k][2] if k < len(mine) else False))) for k, g in enumerate(groups)]
        if theirs != mine:
            raise CommuHipError(f"optimizer state has another grouping than this optimiser: the state has {_describe(theirs)}, "
                                f"the optimiser {_describe(mine)}")
        for mg, g in zip(self.param_groups, groups):
            for k in ("lr", "betas", "eps", "initial_lr"):
                if k in g:
                    mg[k] = tuple(g[k]) if k == "betas" else g[k]
        state = sd.get("state", {})
        if not state:
            fl["m"], fl["v"], self.step_count = None, None, 0
            return
        fl["m"] = torch.zeros_like(fl["p"])
        fl["v"] = torch.zeros_like(fl["p"])
        steps = set()
        for idx, i in enumerate(self._order):
            p, off = fl["params"][i], fl["offs"][i]
            st = state.get(idx, state.get(str(idx)))
            if st is None:
                if self.param_groups[self.tensor_group[i]]["frozen"]:
                    continue
                raise CommuHipError(f"optimizer state misses parameter {idx}")
            n = p.numel()
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise CommuHipError(f"optimizer state of parameter {idx} has shape {tuple(st['exp_avg'].shape)}")
            if self.param_groups[self.tensor_group[i]]["frozen"]:
                continue                                            # (moments of a tensor frozen now: not used)
            fl["m"][off:off + n].copy_(st["exp_avg"].reshape(-1).to(fl["m"].device, torch.float32))
            fl["v"][off:off + n].copy_(st["exp_avg_sq"].reshape(-1).to(fl["v"].device, torch.float32))
            steps.add(int(float(st["step"])))
        if len(steps) != 1:
            raise CommuHipError("per-parameter step counts differ: not an Adam state this kernel can resume")
        self.step_count = steps.pop()
