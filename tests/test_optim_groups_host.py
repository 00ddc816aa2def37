"""CPU side of the grouped optimiser step: the float64 reference of optim_groups_contract.py against torch.optim.Adam / AdamW,
every planted defect of the fp32 emulation caught by the checks the GPU test applies (and the clean emulation inside them),
the pure group resolver of commu_amd.optim with each of its refusals, and the training command line's new flags."""
import importlib.util
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_groups_contract as GC  # noqa: E402
import train_contract as TC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worst(res):
    return max(res.values())


# ---------------------------------------------------------------------------------------------------------------------
# grouped_ref is torch.optim.Adam / AdamW
@pytest.mark.parametrize("decoupled", [False, True])
def test_grouped_ref_is_torch(decoupled):
    inp = GC.GroupedInputs("small")
    lrs = [float(TC.F32(x)) for x in inp.lrs]
    wds = [float(TC.F32(x)) for x in inp.wds]
    b1, b2, eps = (float(TC.F32(x)) for x in (TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_EPS))
    params = [torch.tensor(inp.p[o:o + k].astype(np.float64), requires_grad=not inp.frozen[t])
              for o, k, t in zip(inp.offs, inp.numels, inp.tensor_group)]
    pgs = [dict(params=[p for p, t in zip(params, inp.tensor_group) if t == k], lr=lrs[k], weight_decay=wds[k])
           for k in range(len(lrs))]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(pgs, lr=lrs[0], betas=(b1, b2), eps=eps)
    p, m, v = inp.p.astype(np.float64), np.zeros(inp.n), np.zeros(inp.n)
    rng = np.random.RandomState(5)
    clip = 0.25
    for step in range(1, 6):
        g = np.where(inp.real, 0.1 * rng.randn(inp.n), 0.0)
        trainable = [q for q in params if q.requires_grad]
        for q, o, k in zip(params, inp.offs, inp.numels):
            q.grad = torch.tensor(g[o:o + k]) if q.requires_grad else None
        total = float(torch.nn.utils.clip_grad_norm_(trainable, clip))
        opt.step()
        gnorm = math.sqrt(float((g[~inp.elem_frozen] ** 2).sum()))
        assert abs(gnorm - total) <= 1e-12 * total
        coef = min(1.0, clip / (gnorm + 1e-6))
        assert coef < 0.5                                       # the clip bites
        p, m, v = GC.grouped_ref(p, g, m, v, inp.bmap, lrs, wds, inp.frozen, coef, 1 - b1 ** step, 1 - b2 ** step, decoupled)
        for q, o, k, t in zip(params, inp.offs, inp.numels, inp.tensor_group):
            got = q.detach().numpy()
            assert np.abs(p[o:o + k] - got).max() <= 1e-12 * np.abs(got).max(), (step, k)
            if inp.frozen[t]:
                assert np.array_equal(got, inp.p[o:o + k].astype(np.float64)) and q not in opt.state
            else:
                st = opt.state[q]
                assert np.abs(m[o:o + k] - st["exp_avg"].numpy()).max() <= 1e-12 * np.abs(st["exp_avg"].numpy()).max()
                assert np.abs(v[o:o + k] - st["exp_avg_sq"].numpy()).max() <= 1e-12 * np.abs(st["exp_avg_sq"].numpy()).max()


def test_one_group_is_the_plain_reference():
    inp = GC.GroupedInputs("small", one_group=True)
    coef, bc1, bc2 = GC.standard_scalars()
    for decoupled in (False, True):
        a = GC.grouped_ref(inp.p, inp.g, inp.m, inp.v, inp.bmap, inp.lrs, inp.wds, inp.frozen, coef, bc1, bc2, decoupled)
        b = TC.adam_ref(inp.p, inp.g, inp.m, inp.v, coef, bc1, bc2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        pe, me, ve, _ = GC.grouped_emu(inp.p, inp.g, inp.m, inp.v, inp.bmap, inp.lrs, inp.wds, inp.frozen, coef, bc1, bc2, decoupled)
        pa, ma, va, _ = TC.adam_emu(inp.p, inp.g, inp.m, inp.v, coef, bc1, bc2)
        assert np.array_equal(pe, pa) and np.array_equal(me, ma) and np.array_equal(ve, va)


# ---------------------------------------------------------------------------------------------------------------------
# the input sets can fail: every defect breaks a bound of the GPU test, the clean emulation breaks none
def _run(inp, decoupled, defect=None):
    coef, bc1, bc2 = GC.standard_scalars()
    args = (inp.p, inp.g, inp.m, inp.v, inp.bmap, inp.lrs, inp.wds, inp.frozen, coef, bc1, bc2, decoupled)
    want = GC.grouped_ref(*args)
    got = GC.grouped_emu(*args, defect=defect, tensor_blocks=GC.tensor_blocks(inp))
    return GC.grouped_check(inp, want, *got)


def test_sets_are_what_the_contract_says():
    assert GC.SETS["small"] == (1, 63, 64, 65, 127, 128, 1000, 4099)
    big = GC.GroupedInputs("big")
    assert big.n == 4096 * 1024 + 64 * 5 and big.offs[1] == GC.GRID_ELEMS          # every group change past the first pass
    assert len(set(big.tensor_group[1:])) >= 3 and any(big.frozen[t] for t in big.tensor_group[1:])
    for name in GC.SETS:
        inp = GC.GroupedInputs(name)
        assert sorted(set(inp.tensor_group)) == [0, 1, 2, 3]
        assert np.all(inp.m[inp.real] != 0) and np.all(inp.v[inp.real] > 0)         # state starts non-zero
        assert all(np.all(t[~inp.real] == 0) for t in (inp.p, inp.g, inp.m, inp.v))


def test_clean_emulation_and_every_defect():
    caught = {d: False for d in GC.DEFECTS}
    for name in GC.SETS:
        inp = GC.GroupedInputs(name)
        for decoupled in (False, True):
            res = _run(inp, decoupled)
            print(f"clean {name} decoupled={decoupled}: " + ", ".join(f"{k} {x:.3g}" for k, x in res.items()))
            assert worst(res) <= 1.0, (name, decoupled, res)
            defects = ("group_of_first_pass",) if name == "big" else GC.DEFECTS[:5]
            for d in defects:
                caught[d] = caught[d] or worst(_run(inp, decoupled, d)) > 1.0
        npart = GC.NORM_NPART[name]
        clean = GC.norm_check(inp, npart, GC.norm_emu(inp, npart))
        print(f"clean norm {name}: {clean:.3g}")
        assert clean <= 1.0
        caught["norm_counts_frozen"] = caught["norm_counts_frozen"] or GC.norm_check(inp, npart, GC.norm_emu(inp, npart, "norm_counts_frozen")) > 1.0
        # a frozen block's gradient that is merely large (not NaN) shows as well
        g = np.where(inp.elem_frozen, TC.F32(0), inp.g)
        full = math.sqrt(float((inp.g.astype(np.float64) ** 2).sum()))
        assert GC.norm_check(inp, npart, full) > 1.0 or name == "big"
        assert GC.norm_check(inp, npart, math.sqrt(float((g.astype(np.float64) ** 2).sum()))) == 0.0
    assert all(caught.values()), caught
    # each defect that depends on the mode is caught in the mode it lives in
    small = GC.GroupedInputs("small")
    assert worst(_run(small, False, "decay_scaled_by_clip")) > 1.0
    assert worst(_run(small, True, "decoupled_base_lr")) > 1.0
    assert worst(_run(GC.GroupedInputs("small"), True, "group_of_first_pass")) <= 1.0          # needs the stride: the big set
    for decoupled in (False, True):
        assert worst(_run(GC.GroupedInputs("big"), decoupled, "group_of_first_pass")) > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# resolver
NAMES = [("word_emb.emb_layers.0.weight", 1), ("r_w_bias", 63), ("r_r_bias", 64), ("layers.0.dec_attn.qkv_net.weight", 65),
         ("layers.0.dec_attn.layer_norm.weight", 127), ("layers.0.pos_ff.CoreNet.0.bias", 128),
         ("layers.1.dec_attn.qkv_net.weight", 1000), ("layers.1.pos_ff.CoreNet.0.bias", 4099)]


def test_resolver_first_match_default_merge_and_block_map():
    from commu_amd.optim import resolve_groups
    res = resolve_groups(NAMES, 0.1, None)
    assert res["groups"] == [dict(lr_mult=1.0, weight_decay=0.1, frozen=False)] and set(res["tensor_group"]) == {0}
    assert res["block_map"] == bytes(sum(GC.padded(k) // 64 for _, k in NAMES))
    spec = [{"match": "word_emb.*", "frozen": True},
            {"match": ["*.bias", "*layer_norm*"], "weight_decay": 0.0},
            {"match": "r_*_bias", "weight_decay": 0.0, "lr_mult": 1.0},          # equal to the entry above: one group
            {"match": "layers.1.*", "lr_mult": 0.5}]                              # layers.1...bias went to the no-decay entry first
    res = resolve_groups(NAMES, 0.1, spec)
    assert res["groups"] == [dict(lr_mult=1.0, weight_decay=0.1, frozen=False), dict(lr_mult=1.0, weight_decay=0.1, frozen=True),
                             dict(lr_mult=1.0, weight_decay=0.0, frozen=False), dict(lr_mult=0.5, weight_decay=0.1, frozen=False)]
    assert res["tensor_group"] == [1, 2, 2, 0, 2, 2, 3, 2]
    want = b"".join(bytes([k]) * (GC.padded(n) // 64) for (_, n), k in zip(NAMES, res["tensor_group"]))
    assert res["block_map"] == want and len(want) == 1 + 1 + 1 + 2 + 2 + 2 + 16 + 65
    _, _, bmap, _ = GC.layout([n for _, n in NAMES], res["tensor_group"])
    assert bytes(bmap) == res["block_map"]
    # everything matched: the default group is dropped, numbering stays dense
    res = resolve_groups(NAMES[:3], 0.1, [{"match": "*", "lr_mult": 0.25}])
    assert res["groups"] == [dict(lr_mult=0.25, weight_decay=0.1, frozen=False)] and res["tensor_group"] == [0, 0, 0]


def test_resolver_refusals():
    from commu_amd.optim import GroupSpecError, resolve_groups
    with pytest.raises(GroupSpecError, match=r"'nothing\.\*' matches no parameter"):
        resolve_groups(NAMES, 0.0, [{"match": "nothing.*"}])
    with pytest.raises(GroupSpecError, match=r"'crit\.\*' matches no parameter.*tied to word_emb\.emb_layers\.0\.weight"):
        resolve_groups(NAMES, 0.0, [{"match": ["r_w_bias", "crit.*"], "frozen": True}])
    many = [(f"t{i}", 10) for i in range(20)]
    with pytest.raises(GroupSpecError, match=r"17 distinct parameter groups.*at most 16"):
        resolve_groups(many, 0.0, [{"match": f"t{i}", "lr_mult": 1.0 + i} for i in range(1, 17)])
    assert len(resolve_groups(many, 0.0, [{"match": f"t{i}", "lr_mult": 1.0 + i} for i in range(1, 16)])["groups"]) == 16
    with pytest.raises(GroupSpecError, match=r"'lr_mult' is negative"):
        resolve_groups(NAMES, 0.0, [{"match": "*", "lr_mult": -1.0}])
    with pytest.raises(GroupSpecError, match=r"'weight_decay' is negative"):
        resolve_groups(NAMES, 0.0, [{"match": "*", "weight_decay": -0.1}])
    with pytest.raises(GroupSpecError, match=r"weight_decay -0\.5"):
        resolve_groups(NAMES, -0.5, None)
    with pytest.raises(GroupSpecError, match=r"every parameter is frozen.*'match': '\*'"):
        resolve_groups(NAMES, 0.0, [{"match": "*", "frozen": True}])
    for bad, msg in (({"match": "*", "lr": 1}, r"unknown key\(s\) \['lr'\]"), ({"lr_mult": 1.0}, r"'match' must be"),
                     ("*", r"is not a dictionary"), ({"match": "*", "frozen": 1}, r"'frozen' must be true or false"),
                     ({"match": "*", "lr_mult": "2"}, r"'lr_mult' must be a finite number")):
        with pytest.raises(GroupSpecError, match=msg):
            resolve_groups(NAMES, 0.0, [bad])
    with pytest.raises(GroupSpecError, match=r"must be a list"):
        resolve_groups(NAMES, 0.0, {"match": "*"})


# ---------------------------------------------------------------------------------------------------------------------
# command line
def _cli():
    spec = importlib.util.spec_from_file_location("train_cli_groups", os.path.join(ROOT, "commu-code_amd", "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_train_cli_flags_and_refusals(tmp_path, capsys):
    cli = _cli()
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = capsys.readouterr().out
    for flag in ("--init_checkpoint", "--resume", "--lr", "--warmup_step", "--weight_decay", "--adamw", "--param_groups"):
        assert flag in text
    assert text.count("not in the reference") >= 7 and "train_step" in text
    base = ["--data_dir", str(tmp_path / "no_such_data"), "--work_dir", str(tmp_path / "work")]
    ck = tmp_path / "a.pt"
    ck.write_bytes(b"")
    good = tmp_path / "groups.json"
    good.write_text(json.dumps([{"match": "*.bias", "weight_decay": 0.0}]))
    assert cli.check_fine_tune_args(cli.parse_args(base)) is None
    assert cli.check_fine_tune_args(cli.parse_args(base + ["--param_groups", str(good)])) == [{"match": "*.bias", "weight_decay": 0.0}]
    assert cli.check_fine_tune_args(cli.parse_args(base + ["--param_groups", '[{"match": "r_*_bias", "frozen": true}]'])) == \
        [{"match": "r_*_bias", "frozen": True}]
    refusals = ((["--init_checkpoint", str(ck), "--resume", str(ck)], r"--init_checkpoint and --resume"),
                (["--param_groups", '[{"match": "*", "lr_mult": -1}]'], r"--param_groups: .*'lr_mult' is negative"),
                (["--param_groups", '[{"match": "*"'], r"--param_groups: not JSON"),
                (["--param_groups", '{"match": "*"}'], r"--param_groups: .*must be a list"))
    for flags, msg in refusals:
        with pytest.raises(ValueError, match=msg):
            cli.check_fine_tune_args(cli.parse_args(base + flags))
        with pytest.raises(ValueError, match=msg):          # main() refuses before a dataset or a model is built
            cli.main(base + flags)
    assert not (tmp_path / "work").exists()
