"""The grouped optimiser step on the GPU (csrc/optim_groups.hip, commu_amd.optim.FusedAdam with weight decay and groups, the
Trainer's three step forms, checkpoints) against the float64 contract of tests/optim_groups_contract.py.
tests/test_optim_groups_host.py shows on the CPU that the input sets used here catch every planted defect.  Every test
prints its figures before it asserts."""
import math

import numpy as np
import pytest
import torch

import optim_groups_contract as GC
import train_contract as TC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SPEC = [{"match": "word_emb.*", "frozen": True},
        {"match": ["*.bias", "*layer_norm*", "r_*_bias"], "weight_decay": 0.0},
        {"match": "layers.1.*", "lr_mult": 0.5}]
OTHER_SPEC = [{"match": "*.bias", "weight_decay": 0.0}]
WD = 0.1
CLIP = 0.02          # below the tiny model's gradient norm: the clip bites in every step
T, B = 32, 4


def ops():
    from commu_amd import ops as o
    return o


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def settle(name, res):
    if not isinstance(res, dict):
        res = {"": res}
    print("RATIO " + name + " " + " ".join(f"{k}={v:.4f}" for k, v in sorted(res.items())))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (name, bad)


_INPUTS = {}


def inputs(name, one_group=False):
    """the input sets and their references are built once and shared (never modified)"""
    key = (name, one_group)
    if key not in _INPUTS:
        _INPUTS[key] = GC.GroupedInputs(name, one_group)
    return _INPUTS[key]


def buffers(inp):
    return (dev(inp.p), dev(inp.g), dev(inp.m), dev(inp.v), torch.full((inp.n,), TC.SENT, device=DEV, dtype=BF),
            torch.from_numpy(inp.bmap).to(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# kernels
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("name", list(GC.SETS))
def test_grouped_step_contract(name, decoupled):
    o = ops()
    inp = inputs(name)
    gnorm = 2.0
    gn = dev(np.array([gnorm], dtype=TC.F32))
    bc1, bc2 = o.adam_bias_corrections(TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_STEP)
    coef = TC.clip_coef32(gnorm, TC.ADAM_CLIP)
    want = GC.grouped_ref(inp.p, inp.g, inp.m, inp.v, inp.bmap, inp.lrs, inp.wds, inp.frozen, coef, TC.F32(bc1), TC.F32(bc2),
                          decoupled)
    kw = dict(decoupled=decoupled, gnorm=gn, clip=TC.ADAM_CLIP, beta1=TC.ADAM_B1, beta2=TC.ADAM_B2, eps=TC.ADAM_EPS)
    p, g, m, v, pb, bm = buffers(inp)
    o.adam_step_groups(p, g, m, v, pb, bm, inp.lrs, inp.wds, inp.frozen, TC.ADAM_STEP, **kw)
    p2, g2, m2, v2, pb2, _ = buffers(inp)
    table = o.group_table(inp.lrs, inp.wds, inp.frozen, bc1, bc2).to(DEV)
    o.adam_step_groups_dev(p2, g2, m2, v2, pb2, bm, table, **kw)
    torch.cuda.synchronize()
    for a, b in ((p, p2), (m, m2), (v, v2), (pb, pb2)):
        assert torch.equal(a, b)                                # _dev is the eager entry point, bit for bit
    assert torch.equal(g, dev(inp.g))
    settle(f"adam_step_groups {name} decoupled={decoupled}", GC.grouped_check(inp, want, host(p), host(m), host(v), host(pb)))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("name", ["small", "big"])
def test_one_plain_group_is_adam_step(name, decoupled):
    o = ops()
    inp = inputs(name, one_group=True)
    gn = dev(np.array([2.0], dtype=TC.F32))
    kw = dict(gnorm=gn, clip=TC.ADAM_CLIP, beta1=TC.ADAM_B1, beta2=TC.ADAM_B2, eps=TC.ADAM_EPS)
    p, g, m, v, pb, bm = buffers(inp)
    o.adam_step_groups(p, g, m, v, pb, bm, inp.lrs, inp.wds, inp.frozen, TC.ADAM_STEP, decoupled=decoupled, **kw)
    p2, g2, m2, v2, pb2, _ = buffers(inp)
    o.adam_step(p2, g2, m2, v2, pb2, inp.lrs[0], TC.ADAM_STEP, **kw)
    torch.cuda.synchronize()
    for nm, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2), ("shadow", pb, pb2)):
        print(f"one group {name} decoupled={decoupled} {nm}: differing elements {int((a != b).sum())}")
        assert torch.equal(a, b), nm


def test_refusals_leave_the_buffers_untouched():
    import ctypes as C
    from commu_amd import _lib
    from commu_amd._lib import CommuHipError
    o = ops()
    lib = _lib.load()
    inp = inputs("small")
    n = inp.n
    lr = (C.c_float * 4)(*inp.lrs)
    wd = (C.c_float * 4)(*inp.wds)
    stream = o._s()

    def fresh():
        big = [torch.cat([t, t[:64]]) for t in buffers(inp)[:4]]
        pb = torch.full((n + 64,), TC.SENT, device=DEV, dtype=BF)
        return big, pb, torch.from_numpy(inp.bmap).to(DEV)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    cases = {"n % 64": (0, n - 28, 0), "p misaligned": (1, n, 0), "shadow misaligned": (0, n, 4)}
    for what, (off, nn, pboff) in cases.items():
        big, pb, bm = fresh()
        before = [t.clone() for t in big] + [pb.clone()]
        views = [t[off:] for t in big]
        rc = lib.commu_adam_step_groups(ptr(views[0]), ptr(views[1]), ptr(views[2]), ptr(views[3]), ptr(pb[pboff:]), nn, ptr(bm), 4,
                                        lr, wd, 8, 0, TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_EPS, TC.ADAM_STEP, None, 0.0, stream)
        table = o.group_table(inp.lrs, inp.wds, inp.frozen, 0.5, 0.5).to(DEV)
        rc2 = lib.commu_adam_step_groups_dev(ptr(views[0]), ptr(views[1]), ptr(views[2]), ptr(views[3]), ptr(pb[pboff:]), nn,
                                             ptr(bm), ptr(table), 0, TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_EPS, None, 0.0, stream)
        torch.cuda.synchronize()
        print(f"refusal {what}: status {rc} / {rc2}")
        assert rc != 0 and rc2 != 0, what
        assert all(torch.equal(a, b) for a, b in zip(before, big + [pb])), what
    big, pb, bm = fresh()
    part, out = torch.zeros(4, device=DEV), torch.full((1,), -1.0, device=DEV)
    assert lib.commu_grad_norm_groups(ptr(big[1]), n - 28, ptr(bm), 8, ptr(part), 4, ptr(out), stream) != 0
    assert lib.commu_grad_norm_groups(ptr(big[1][1:]), n, ptr(bm), 8, ptr(part), 4, ptr(out), stream) != 0
    assert float(out[0]) == -1.0
    with pytest.raises(CommuHipError):                          # the wrapper raises on the status
        o.adam_step_groups(big[0][1:n + 1], big[1][1:n + 1], big[2][1:n + 1], big[3][1:n + 1], pb[:n], bm, inp.lrs, inp.wds,
                           inp.frozen, 1)
    with pytest.raises(CommuHipError):
        o.adam_step_groups(big[0][:n], big[1][:n], big[2][:n], big[3][:n], pb[:n], bm, inp.lrs * 5, inp.wds * 5, inp.frozen * 5, 1)


@pytest.mark.parametrize("name", list(GC.SETS))
def test_grouped_norm_contract(name):
    o = ops()
    inp = inputs(name)
    npart = GC.NORM_NPART[name]
    bm = torch.from_numpy(inp.bmap).to(DEV)
    g = dev(GC.norm_inputs(inp))                                # NaN in every frozen block: never read
    outs = []
    for _ in range(2):
        part, out = torch.full((npart,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
        o.grad_norm_groups(g, bm, inp.frozen, part, out)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])                        # deterministic
    settle(f"grad_norm_groups {name} npart={npart}", GC.norm_check(inp, npart, host(outs[0])[0]))
    # nothing frozen: commu_grad_norm, bit for bit
    g = dev(inp.g)
    part, a, b = torch.zeros(npart, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    o.grad_norm_groups(g, bm, [False] * 4, part, a)
    o.grad_norm(g, part, b)
    print(f"norm {name}: grouped {float(a[0])!r} plain {float(b[0])!r}")
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# FusedAdam / Trainer on a tiny model
def make_cfg():
    from commu_amd.model.config_helper import get_cfg
    # (warmup 0 and lr_min = lr / 2: the schedule gives lr, lr / 2, lr / 2, .. -- no step with lr 0, and it moves)
    return get_cfg(num_layers=2, num_heads=4, units=128, inner_size=256, tgt_length=T, mem_length=0, batch_size=B, batch_chunk=1,
                   dropout=0.0, attention_dropout=0.0, lr=0.01, lr_min=0.005, warmup_step=0, weight_decay=WD, clip=CLIP)


def make_trainer(seed=1, spec=SPEC, fp32=False, **kw):
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.train import Trainer, build_model
    cfg = make_cfg()
    model = build_model(cfg, BaseVocab(), torch.device(DEV), seed=seed)
    if fp32:
        model.fp32_training = True
    return Trainer(model, cfg, param_groups=spec, **kw)


def batches(k):
    from commu_amd.model.dataset import synthetic_batch
    return [synthetic_batch(T, B, torch.device(DEV), seed=70 + i) for i in range(k)]


class FlatCase:
    """what grouped_check needs, from the flat buffers captured before a step"""

    def __init__(self, tr, p, m, v):
        fl = tr.model._flat
        self.p, self.m, self.v = p, m, v
        bmap = np.frombuffer(tr.optimizer.resolved["block_map"], dtype=np.uint8)
        self.bmap = bmap
        self.elem_frozen = np.repeat(np.asarray(tr.optimizer.frozen_flags)[bmap], 64)
        self.real = np.zeros(fl["total"], dtype=bool)
        for q, off in zip(fl["params"], fl["offs"]):
            self.real[off:off + q.numel()] = True


@pytest.mark.parametrize("mode", ["adam", "adamw", "adam_fp32"])
def test_fused_adam_groups_on_a_tiny_model(mode, monkeypatch):
    from commu_amd import ops as o
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.optim import FusedAdam
    from commu_amd.train import build_model
    decoupled = mode == "adamw"
    tr = make_trainer(fp32=(mode == "adam_fp32"), decoupled=decoupled)
    opt = tr.optimizer
    assert opt.kernel_name() == "commu_adam_step_groups"
    assert [(g["weight_decay"], g["frozen"]) for g in opt.param_groups] == [(WD, False), (WD, True), (0.0, False), (WD, False)]
    assert [g["lr"] for g in opt.param_groups] == [0.01, 0.01, 0.01, 0.005]
    plain = FusedAdam(build_model(make_cfg(), BaseVocab(), torch.device(DEV), seed=2), lr=0.01)
    assert plain.kernel_name() == "commu_adam_step" and len(plain.param_groups) == 1
    emb0 = tr.model.word_emb.emb_layers[0].weight.detach().clone()
    log, real = [], o.adam_step_groups

    def spy(p, g, m, v, pb, bm, lrs, wds, frozen, step, **kw):
        snap = dict(p=host(p), g=host(g), m=host(m), v=host(v), pb=host(pb), lrs=list(lrs), wds=list(wds), frozen=list(frozen),
                    step=step, gnorm=float(kw["gnorm"][0]), clip=kw["clip"], decoupled=kw["decoupled"], bm=bm.cpu().numpy())
        real(p, g, m, v, pb, bm, lrs, wds, frozen, step, **kw)
        snap["after"] = (host(p), host(m), host(v), host(pb))
        log.append(snap)
    monkeypatch.setattr(o, "adam_step_groups", spy)
    want_lr = [0.01, 0.005, 0.005]
    for i, b in enumerate(batches(3)):
        assert math.isfinite(float(tr.step(*b)))
        s = log[-1]
        case = FlatCase(tr, s["p"], s["m"], s["v"])
        assert np.array_equal(s["bm"], case.bmap) and s["decoupled"] == decoupled and s["step"] == i + 1 and s["clip"] == CLIP
        assert s["lrs"] == [want_lr[i], want_lr[i], want_lr[i], want_lr[i] / 2] and s["wds"] == [WD, WD, 0.0, WD]
        # the clip norm is over the trainable tensors only
        gsq = (s["g"].astype(np.float64) ** 2)[~case.elem_frozen].sum()
        settle(f"{mode} step {i} clip norm", TC.ratio(s["gnorm"], math.sqrt(gsq), TC.grad_norm_bound(s["g"].shape[0], 256, math.sqrt(gsq))))
        assert (s["g"][case.elem_frozen] != 0).any()            # (the frozen tensor's gradient exists and is left out)
        bc1, bc2 = o.adam_bias_corrections(0.9, 0.999, s["step"])
        coef = TC.clip_coef32(s["gnorm"], s["clip"])
        assert coef < 1.0, s["gnorm"]
        want = GC.grouped_ref(s["p"], s["g"], s["m"], s["v"], case.bmap, s["lrs"], s["wds"], s["frozen"], coef, TC.F32(bc1),
                              TC.F32(bc2), decoupled, b1=0.9, b2=0.999, eps=1e-8)
        settle(f"{mode} step {i} coef={float(coef):.3f}", GC.grouped_check(case, want, *s["after"], pb_before=s["pb"]))
        # the parameters the model sees ARE the flat buffer
        fl = tr.model._flat
        for q, off in zip(fl["params"], fl["offs"]):
            assert np.array_equal(host(q).ravel(), s["after"][0][off:off + q.numel()])
    assert torch.equal(tr.model.word_emb.emb_layers[0].weight.detach(), emb0)          # frozen from start to end
    assert tr.train_step == 3 and opt.step_count == 3


def test_graph_trainer_matches_eager_with_groups(monkeypatch):
    from commu_amd import ops as o
    calls = {"dev": 0, "norm": 0}
    real_dev, real_norm = o.adam_step_groups_dev, o.grad_norm_groups

    def spy_dev(*a, **k):
        calls["dev"] += 1
        return real_dev(*a, **k)

    def spy_norm(*a, **k):
        calls["norm"] += 1
        return real_norm(*a, **k)
    monkeypatch.setattr(o, "adam_step_groups_dev", spy_dev)
    monkeypatch.setattr(o, "grad_norm_groups", spy_norm)
    bs = batches(5)
    out = {}
    for mode in ("eager", "graph"):
        tr = make_trainer(graph=(mode == "graph"))
        snaps = []
        for b in bs:
            tr.step(*b)
            snaps.append(tr.model._flat["p"].detach().clone())
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr.graph_failed is None, tr.graph_failed
            assert tr._graphs is not None and calls["dev"] == 1          # captured once with the _dev entry point, then replayed
            assert tr.optimizer.kernel_name() == "commu_adam_step_groups" and tr.optimizer.step_count == 5
        else:
            assert calls["dev"] == 0 and calls["norm"] == 5
        out[mode] = (snaps, [g["lr"] for g in tr.optimizer.param_groups])
    for i, (a, b) in enumerate(zip(*[out[m][0] for m in ("eager", "graph")])):
        print(f"graph vs eager after step {i}: differing {int((a != b).sum())} of {a.numel()}, max |diff| {float((a - b).abs().max()):.3e}")
    for a, b in zip(*[out[m][0] for m in ("eager", "graph")]):
        assert torch.equal(a, b)
    assert out["eager"][1] == out["graph"][1]


def test_checkpoint_round_trip_with_groups(tmp_path):
    from commu_amd._lib import CommuHipError
    from commu_amd.train import load_checkpoint, read_checkpoint, save_checkpoint
    from commu_amd.model.dataset import BaseVocab
    bs = batches(4)
    a = make_trainer()
    for b in bs:
        a.step(*b)
    c = make_trainer()
    for b in bs[:2]:
        c.step(*b)
    path = str(tmp_path / "checkpoint_last.pt")
    save_checkpoint(path, c.model, c.optimizer, BaseVocab(), c.train_step, 1.5, c.scheduler)
    r = make_trainer(seed=99)                                   # another initialisation: must be overwritten
    r.train_step, best = load_checkpoint(path, r.model, r.optimizer, r.scheduler)
    assert r.train_step == 2 and best == 1.5 and r.optimizer.step_count == 2
    for b in bs[2:]:
        r.step(*b)
    torch.cuda.synchronize()
    fa, fr = a.model._flat, r.model._flat
    for k in ("p", "m", "v"):
        print(f"round trip {k}: differing {int((fa[k] != fr[k]).sum())}, max |diff| {float((fa[k] - fr[k]).abs().max()):.3e}")
    for k in ("p", "m", "v"):
        assert torch.equal(fa[k], fr[k]), k
    assert [g["lr"] for g in a.optimizer.param_groups] == [g["lr"] for g in r.optimizer.param_groups]
    assert a.train_step == r.train_step == 4

    # torch.optim.Adam with the same grouping takes the state over
    ck = read_checkpoint(path)
    opt = c.optimizer
    cpu = [[torch.nn.Parameter(q.detach().cpu().clone(), requires_grad=not g["frozen"]) for q in g["params"]] for g in opt.param_groups]
    adam = torch.optim.Adam([dict(params=ps, lr=g["lr"], weight_decay=g["weight_decay"]) for ps, g in zip(cpu, opt.param_groups)],
                            lr=0.01)
    adam.load_state_dict(ck["optimizer"])
    fl = c.model._flat
    off_of = {id(q): off for q, off in zip(fl["params"], fl["offs"])}
    for ps, g in zip(cpu, opt.param_groups):
        for q_cpu, q in zip(ps, g["params"]):
            if g["frozen"]:
                assert q_cpu not in adam.state
                continue
            st, off = adam.state[q_cpu], off_of[id(q)]
            assert float(st["step"]) == 2.0
            assert torch.equal(st["exp_avg"].reshape(-1), fl["m"][off:off + q.numel()].cpu())
            assert torch.equal(st["exp_avg_sq"].reshape(-1), fl["v"][off:off + q.numel()].cpu())
    assert [g["weight_decay"] for g in adam.param_groups] == [WD, WD, 0.0, WD]

    other = make_trainer(spec=OTHER_SPEC)
    with pytest.raises(CommuHipError, match=r"another grouping.*the state has \[.*1 tensors, weight_decay 0\.1, frozen.*the optimiser \["):
        load_checkpoint(path, other.model, other.optimizer, other.scheduler)


# ---------------------------------------------------------------------------------------------------------------------
# command line: start from a checkpoint, resume one
def test_train_cli_init_checkpoint_and_resume(tmp_path):
    import os
    import test_model_gpu as TM
    from commu_amd._lib import CommuHipError
    from commu_amd.train import read_checkpoint
    rng = np.random.RandomState(0)
    corpus = {s: [np.concatenate([rng.randint(560, 729, 11), rng.randint(2, 560, rng.randint(20, 90)), [1]])
                  for _ in range(n)] for s, n in (("train", 40), ("valid", 8))}
    data_dir = tmp_path / "output_npy"
    data_dir.mkdir()
    TM._write_output_npy(str(data_dir), corpus)
    cli = TM._load_script("train")
    spec = '[{"match": "word_emb.*", "frozen": true}, {"match": ["*.bias", "*layer_norm*"], "weight_decay": 0}]'
    shape = ["--data_dir", str(data_dir), "--num_layers", "2", "--num_heads", "2", "--units", "64", "--inner_size", "128",
             "--tgt_length", "16", "--mem_length", "16", "--batch_size", "4", "--batch_chunk", "2", "--log_interval", "1"]
    tune = ["--lr", "0.002", "--warmup_step", "2", "--weight_decay", "0.05", "--adamw", "--param_groups", spec]

    def run(name, extra):
        d = cli.main(shape + ["--work_dir", str(tmp_path / name)] + extra)
        return d, open(os.path.join(d, "train_rank0.log")).read()

    d1, log1 = run("a", tune + ["--max_step", "2", "--eval_interval", "2"])
    ck1 = read_checkpoint(os.path.join(d1, "checkpoint_last.pt"))
    groups = ck1["optimizer"]["param_groups"]
    assert ck1["train_step"] == 2 and [(g["weight_decay"], g["frozen"]) for g in groups] == [(0.05, False), (0.05, True), (0.0, False)]
    assert "weight_decay: 0.05" in open(os.path.join(d1, "config.yml")).read()
    emb = ck1["model"]["word_emb.emb_layers.0.weight"]

    d2, log2 = run("b", tune + ["--resume", os.path.join(d1, "checkpoint_last.pt"), "--max_step", "4", "--eval_interval", "4"])
    assert "resumed" in log2 and "at step 2" in log2 and "Train Step 3/4" in log2 and "Train Step 1/4" not in log2
    ck2 = read_checkpoint(os.path.join(d2, "checkpoint_last.pt"))
    assert ck2["train_step"] == 4 and float(ck2["optimizer"]["state"][0]["step"]) == 4.0
    assert torch.equal(ck2["model"]["word_emb.emb_layers.0.weight"], emb)          # frozen across both runs
    assert not torch.equal(ck2["model"]["r_w_bias"], ck1["model"]["r_w_bias"])

    d3, log3 = run("c", ["--init_checkpoint", os.path.join(d1, "checkpoint_last.pt"), "--max_step", "1", "--eval_interval", "9"])
    assert "(missing: [], unexpected: [])" in log3 and "Train Step 1/1" in log3 and "resumed" not in log3

    with pytest.raises(CommuHipError, match=r"another grouping"):          # the flags' grouping differs from the checkpoint's
        run("d", ["--resume", os.path.join(d1, "checkpoint_last.pt"), "--max_step", "4", "--eval_interval", "4"])
