"""Loss options on the GPU: the option kernels (commu_ce_fwd_opts, commu_ce_bwd_opts, commu_ce_bwd_opts_f32) against the
float64 contract of tests/loss_opts_contract.py at train_contract's cross-entropy shapes, a tiny model's training step in both
arithmetics against float64 autograd, commu_nll_by_class, the captured step against the eager one, and the command line's
checkpoint round trip.  tests/test_loss_opts_host.py shows on the CPU that the contract's inputs catch the planted defects."""
import os

import numpy as np
import pytest
import torch

import loss_opts_contract as LC
import train_contract as TC
from test_train_contract_gpu import dev, full, host, ops, settle

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def cos(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("case", TC.ce_bwd_cases(), ids=lambda c: "V%d_ldl%d_ldd%d_r%d" % c)
def test_loss_option_kernels_contract(case):
    o = ops()
    V, ldl, ldd, rows = case
    inp = TC.CeInputs(V, ldl, rows)
    x, target, g = dev(inp.x), dev(inp.target, torch.int64), dev(inp.g)
    assert x.stride(0) == ldl
    lse32 = TC.ce_lse32(inp)
    l32 = dev(lse32)
    vf, vb = ("_vec" if TC.ce_vec_fwd(V, ldl) else "_scalar"), ("_vec" if TC.ce_vec_bwd(V, ldl, ldd) else "_scalar")
    # the plain kernels on the same inputs: what eps = zeta = 0 has to reproduce bit for bit
    pn, pl = full((rows,), float("nan")), full((rows,), float("nan"))
    o.call("commu_ce_fwd", o._p(x), ldl, o._p(target), o._p(pn), o._p(pl), rows, V, o._s())
    pd = full((rows, ldd), TC.SENT, BF)
    o.ce_bwd(x, target, l32, g, V, dlogits=pd)
    pd32 = o.ce_bwd_f32(x[:, :V], target, l32, g, V)
    for eps, zeta in LC.OPTS:
        tag = f" eps={eps} zeta={zeta}"
        loss, nll, lse = (full((rows + 2,), TC.SENT) for _ in range(3))
        o.call("commu_ce_fwd_opts", o._p(x), ldl, o._p(target), o._p(loss), o._p(nll), o._p(lse), rows, V, eps, zeta, o._s())
        settle("ce_fwd_opts" + vf + tag, LC.check_fwd(inp, eps, zeta, host(loss)[:rows], host(nll)[:rows], host(lse)[:rows]))
        # rows past the last one (a workgroup holds four) keep the sentinel, bf16 pad columns are zero: check_bwd's guard
        d = full((rows + 2, ldd), TC.SENT, BF)
        o.ce_bwd_opts(x, target, l32, g, V, eps, zeta, dlogits=d)
        settle("ce_bwd_opts" + vb + tag, LC.check_bwd(inp, lse32, eps, zeta, host(d)[:rows], ldd))
        d32 = full((rows + 2, ldd), TC.SENT)
        o.ce_bwd_opts_f32(x, target, l32, g, V, eps, zeta, dlogits=d32)
        settle("ce_bwd_opts_f32" + tag, LC.check_bwd(inp, lse32, eps, zeta, host(d32)[:rows], ldd, bits=24))
        f32_out = o.ce_fwd_opts_f32(x, target, V, eps, zeta)          # the fp32 schedule's name for the same forward
        assert all(torch.equal(a, b[:rows]) for a, b in zip(f32_out, (loss, nll, lse)))
        for t in (loss, nll, lse, d, d32):
            assert bool((t[rows:] == TC.SENT).all()), "a row past the last one was written"
        if eps == 0.0 and zeta == 0.0:
            assert torch.equal(nll[:rows], pn) and torch.equal(lse[:rows], pl) and torch.equal(loss[:rows], pn)
            assert torch.equal(d[:rows], pd)
            assert torch.equal(d32[:rows, :V], pd32)


def test_loss_option_entry_points_refuse_bad_options():
    o = ops()
    from commu_amd._lib import CommuHipError
    inp = TC.CeInputs(5, 8, 5)
    x, target = dev(inp.x), dev(inp.target, torch.int64)
    for eps, zeta in ((1.0, 0.0), (-0.1, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(CommuHipError):
            o.ce_fwd_opts(x, target, 5, eps, zeta)
        with pytest.raises(CommuHipError):
            o.ce_bwd_opts(x, target, dev(TC.ce_lse32(inp)), dev(inp.g), 5, eps, zeta)


# ------------------------------------------------------------------------------------------------ per-class NLL
@pytest.mark.parametrize("rows", LC.NLL_ROWS)
def test_nll_by_class_contract(rows):
    o = ops()
    inp = LC.NllInputs(rows)
    assert o.call("commu_nll_by_class_blocks", rows) == LC.nll_blocks(rows)
    nll, target, table = dev(inp.nll), dev(inp.target, torch.int64), dev(inp.table, torch.int32)
    a = o.nll_by_class(nll, target, table, LC.N_CLASSES, pad=inp.pad)
    b = o.nll_by_class(nll, target, table, LC.N_CLASSES, pad=inp.pad)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])          # two runs: identical bits
    settle(f"nll_by_class rows={rows}", LC.nll_by_class_check(inp, host(a[0]), a[1].cpu().numpy()))
    every = o.nll_by_class(nll, target, table, LC.N_CLASSES)             # pad < 0: no row is left out
    assert int(every[1].sum()) == rows


# ------------------------------------------------------------------------------------------------ tiny model
EPS, ZETA = 0.1, 1e-4
L_, H_, D_, DI_, T_, B_ = 2, 2, 64, 128, 16, 3


def _tiny(seed=11):
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.model.model import MemTransformerLM
    from oracle import xl_ref as X
    cfg = get_cfg(num_layers=L_, num_heads=H_, units=D_, inner_size=DI_, tgt_length=T_, mem_length=0, batch_size=B_,
                  dropout=0.0, attention_dropout=0.0)
    s = X.XLShape(L_, H_, D_, DI_)
    params = X.init_params(s, seed, std=0.02)
    gen = torch.Generator().manual_seed(seed + 7)
    for k in params:                      # give the zero-initialised biases some signal
        if k.endswith(".bias"):
            params[k] = 0.02 * torch.randn(params[k].shape, generator=gen)
    model = MemTransformerLM(cfg, BaseVocab())
    sd = {k: v.clone() for k, v in params.items()}
    sd["crit.out_layers.0.weight"] = sd["word_emb.emb_layers.0.weight"]
    model.load_state_dict(sd, strict=False)
    data = torch.randint(1, 729, (T_, B_), generator=gen)
    target = torch.randint(1, 729, (T_, B_), generator=gen)
    target[-3:, 1] = 0                    # pad targets: rows of loss weight 0
    return model.to(DEV).eval(), cfg, s, params, data, target


@pytest.fixture(scope="module")
def tiny_reference():
    """float64 autograd of the loss with options through the float64 oracle network: loss [T, B] and every gradient"""
    from oracle import xl_ref as X
    _, _, s, params, data, target = _tiny()
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    hidden, _ = X.forward_hidden(p64, s, data, torch.zeros(B_, dtype=torch.bool), None, 0, False)
    logits = X.logits_from_hidden(p64, hidden)
    e, z = LC.f32v(EPS), LC.f32v(ZETA)
    lse = torch.logsumexp(logits, -1)
    nll = lse - torch.gather(logits, 2, target[..., None]).squeeze(-1)
    loss = (1 - e) * nll + e * (lse - logits.mean(-1)) + z * lse ** 2
    loss[target != 0].mean().backward()
    return loss.detach(), nll.detach(), {k: v.grad for k, v in p64.items() if v.grad is not None}


def _step(model, data, target):
    model.zero_grad()
    loss, _ = model(data.to(DEV), target.to(DEV), torch.zeros(B_, dtype=torch.bool, device=DEV), None)
    loss[target.to(DEV) != 0].float().mean().backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_tiny_model_fp32_step_with_options_vs_float64_autograd(tiny_reference):
    ref_loss, ref_nll, ref_grads = tiny_reference
    model, _, _, _, data, target = _tiny()
    model.fp32_training = True
    model.loss_options = {"label_smoothing": EPS, "z_loss": ZETA}
    assert model.loss_kernel_names() == ("commu_ce_fwd_opts_f32", "commu_ce_bwd_opts_f32")
    loss, grads = _step(model, data, target)
    assert rel(loss, ref_loss) <= 1e-5 and rel(model.last_nll, ref_nll) <= 1e-5
    res = {k: (rel(grads[k], g), cos(grads[k], g)) for k, g in ref_grads.items()}
    print("fp32 grads vs float64:", {k: (f"{r:.2e}", f"{c:.7f}") for k, (r, c) in res.items()})
    assert set(ref_grads) <= set(grads)
    for k, (r, c) in res.items():          # the tolerances of tests/test_train_fp32_gpu.py for the plain loss
        assert r <= 1e-4 and c >= 0.99999, (k, r, c)
    model.parity_fp32 = True               # (the no-grad forward in fp32 as well)
    with torch.no_grad():                  # a no-grad forward is the plain nll whatever the options
        plain, _ = model(data.to(DEV), target.to(DEV), None, None)
    assert rel(plain, ref_nll) <= 1e-5 and rel(plain, ref_loss) > 1e-4


def test_tiny_model_bf16_step_with_options_agrees_with_fp32_mode():
    model, _, _, _, data, target = _tiny()
    model.loss_options = {"label_smoothing": EPS, "z_loss": ZETA}
    assert model.loss_kernel_names() == ("commu_ce_fwd_opts", "commu_ce_bwd_opts")
    loss_b, gb = _step(model, data, target)
    model.fp32_training = True
    loss_f, gf = _step(model, data, target)
    assert float((loss_b - loss_f).abs().max()) < 6e-2
    cosines = {k: cos(gb[k], gf[k]) for k in gf}
    print("bf16 vs fp32-mode gradient cosines:", {k: f"{c:.5f}" for k, c in cosines.items()})
    assert min(cosines.values()) > 0.995, cosines          # the cosine tests/test_model_gpu.py asks of the bf16 path


def test_default_options_launch_the_plain_kernels_and_give_the_same_bits():
    from commu_amd import _lib
    model, _, _, _, data, target = _tiny()
    assert model.loss_options == {"label_smoothing": 0.0, "z_loss": 0.0}
    for f32 in (False, True):
        model.fp32_training = f32
        assert model.loss_kernel_names() == ("commu_ce_fwd", "commu_ce_bwd_f32" if f32 else "commu_ce_bwd")
    names = ["commu_ce_fwd", "commu_ce_bwd", "commu_ce_bwd_f32", "commu_ce_fwd_opts", "commu_ce_bwd_opts", "commu_ce_fwd_opts_f32",
             "commu_ce_bwd_opts_f32"]
    seen = {}
    for tag, f32, opts in (("bf16", False, None), ("fp32", True, None), ("bf16+", False, (EPS, ZETA)), ("fp32+", True, (EPS, ZETA))):
        model.fp32_training = f32
        model.loss_options = {"label_smoothing": opts[0], "z_loss": opts[1]} if opts else {"label_smoothing": 0.0, "z_loss": 0.0}
        _lib.profile_start(names)
        try:
            out = _step(model, data, target)
        finally:
            prof = _lib.profile_stop()
        seen[tag] = ({n for n, v in prof.items() if v}, out)
    assert seen["bf16"][0] == {"commu_ce_fwd", "commu_ce_bwd"} and seen["fp32"][0] == {"commu_ce_fwd", "commu_ce_bwd_f32"}
    assert seen["bf16+"][0] == {"commu_ce_fwd_opts", "commu_ce_bwd_opts"}
    assert seen["fp32+"][0] == {"commu_ce_fwd_opts_f32", "commu_ce_bwd_opts_f32"}
    # options at zero THROUGH the option kernels: the plain step bit for bit (the fp32 backward is deterministic,
    # tests/test_train_fp32_gpu.py; the bf16 one is held to its loss here and to dlogits in the kernel test)
    model._loss_opts = lambda: (0.0, 0.0)
    model.fp32_training = True
    loss0, g0 = _step(model, data, target)
    assert torch.equal(loss0, seen["fp32"][1][0]) and all(torch.equal(g0[k], v) for k, v in seen["fp32"][1][1].items())
    model.fp32_training = False
    assert torch.equal(_step(model, data, target)[0], seen["bf16"][1][0])
    model.loss_options = {"label_smoothing": 1.5, "z_loss": 0.0}
    del model._loss_opts
    with pytest.raises(ValueError):
        model(data.to(DEV), target.to(DEV), None, None)


# ------------------------------------------------------------------------------------------------ trainer
def test_graph_step_with_options_matches_eager_and_refuses_a_change():
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab, synthetic_batch
    from commu_amd.train import Trainer, build_model
    dev_ = torch.device(DEV)
    cfg = get_cfg(num_layers=2, num_heads=2, units=64, inner_size=128, tgt_length=32, mem_length=0, batch_size=4, batch_chunk=2,
                  dropout=0.0, attention_dropout=0.0)
    batches = [synthetic_batch(32, 4, dev_, seed=70 + i) for i in range(5)]
    out = {}
    for mode in ("eager", "graph", "plain"):
        model = build_model(cfg, BaseVocab(), dev_, seed=3)
        if mode != "plain":
            model.loss_options = {"label_smoothing": EPS, "z_loss": ZETA}
        tr = Trainer(model, cfg, graph=(mode == "graph"))
        losses = [float(tr.step(*b)) for b in batches]
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr.graph_failed is None, tr.graph_failed
            assert tr._graphs is not None and tr._graph_state["loss_opts"] == (EPS, ZETA)
            model.loss_options = {"label_smoothing": 0.0, "z_loss": ZETA}
            with pytest.raises(ValueError, match="loss_options"):
                tr.step(*batches[0])
        out[mode] = (losses, {n: p.detach().float().cpu().clone() for n, p in model.named_parameters()}, tr.log_window())
    le, lg = out["eager"][0], out["graph"][0]
    assert all(abs(a - b) < 2e-4 for a, b in zip(le, lg)), (le, lg)          # (the bounds of test_graph_step_matches_eager_step)
    for n, a in out["eager"][1].items():
        b = out["graph"][1][n]
        assert float((a - b).abs().max()) <= 2e-5 + 2e-3 * float(a.abs().max()), n
    assert abs(out["eager"][2][0] - out["graph"][2][0]) < 1e-4 and out["eager"][2][2] == out["graph"][2][2]
    # the step returns the regularised loss, the window logs the plain nll: below it (the added terms are positive here),
    # and the first step's difference is what the options add at initialisation
    assert out["plain"][0][0] < le[0] and out["eager"][2][0] < sum(le) / len(le)
    assert abs(out["eager"][2][0] - out["plain"][2][0]) < 0.5


# ------------------------------------------------------------------------------------------------ command line
def test_cli_checkpoint_keeps_position_and_family_report(tmp_path):
    from commu_amd.midi_generator.meta import TOKEN_FAMILIES
    from commu_amd.train import read_checkpoint
    from test_model_gpu import _load_script, _write_output_npy
    rng = np.random.RandomState(0)
    corpus = {s: [np.concatenate([rng.randint(560, 729, 11), rng.randint(2, 560, rng.randint(20, 90)), [1]])
                  for _ in range(n)] for s, n in (("train", 40), ("valid", 12))}
    data_dir, work = tmp_path / "output_npy", tmp_path / "work"
    data_dir.mkdir()
    _write_output_npy(str(data_dir), corpus)
    cli = _load_script("train")
    shape = ["--data_dir", str(data_dir), "--num_layers", "2", "--num_heads", "2", "--units", "64",
             "--inner_size", "128", "--tgt_length", "16", "--mem_length", "16", "--batch_size", "4", "--batch_chunk", "2",
             "--log_interval", "2", "--eval_interval", "2", "--label_smoothing", "0.1", "--z_loss", "1e-4"]
    # (a run directory is named after the clock's second: every run gets a work_dir of its own)
    run_dir = cli.main(shape + ["--work_dir", str(work), "--max_step", "4", "--report_families"])
    log = open(os.path.join(run_dir, "train_rank0.log")).read()
    assert log.count("families: pad_eos_bar nll=") == 2
    last, best = (read_checkpoint(os.path.join(run_dir, n)) for n in ("checkpoint_last.pt", "checkpoint_best.pt"))
    assert {"model", "optimizer", "train_step", "scheduler", "best_val_loss", "vocab", "amp"} <= set(last)
    pos = last["data_position"]
    assert last["train_step"] == 4 and pos["streams"] == [[1111, 0, 4]]
    assert (pos["world"], pos["batch_size"], pos["bptt"], pos["corpus"][0]) == (1, 4, 16, len(corpus["train"]))
    fam = best["val_families"]
    assert list(fam) == list(TOKEN_FAMILIES) and "val_families" not in last
    ntok = sum(len(s) for s in corpus["valid"])          # every target of the validation split: its tokens but the pad start
    assert sum(v["tokens"] for v in fam.values()) == ntok and fam["other"]["tokens"] == 0
    assert fam["meta"]["tokens"] == 11 * len(corpus["valid"]) and fam["pad_eos_bar"]["tokens"] >= len(corpus["valid"])
    total = sum(v["nll"] * v["tokens"] for v in fam.values() if v["tokens"]) / ntok
    assert abs(total - best["best_val_loss"]) <= 1e-4 * best["best_val_loss"]
    # --resume continues the stream at the stored position ...
    path = os.path.join(run_dir, "checkpoint_last.pt")
    run2 = cli.main(shape + ["--work_dir", str(tmp_path / "work2"), "--max_step", "6", "--resume", path])
    log2 = open(os.path.join(run2, "train_rank0.log")).read()
    assert "batch stream resumed at epoch 0, batch 4 (stream seed 1111)" in log2 and "families:" not in log2
    assert read_checkpoint(os.path.join(run2, "checkpoint_last.pt"))["data_position"]["streams"] == [[1111, 0, 6]]
    # ... and a checkpoint without the key resumes as it always did
    del last["data_position"]
    old = str(tmp_path / "old.pt")
    torch.save(last, old)
    run3 = cli.main(shape + ["--work_dir", str(tmp_path / "work3"), "--max_step", "6", "--resume", old])
    log3 = open(os.path.join(run3, "train_rank0.log")).read()
    assert "resumed " + old in log3 and "batch stream resumed" not in log3 and "End of training" in log3
    # that run drew a fresh shuffle from seed + train_step: its checkpoint names THAT stream, and a second resume replays it
    path3 = os.path.join(run3, "checkpoint_last.pt")
    assert read_checkpoint(path3)["data_position"]["streams"] == [[1111 + 4, 0, 2]]
    run4 = cli.main(shape + ["--work_dir", str(tmp_path / "work4"), "--max_step", "8", "--resume", path3])
    assert "batch stream resumed at epoch 0, batch 2 (stream seed 1115)" in open(os.path.join(run4, "train_rank0.log")).read()
    assert read_checkpoint(os.path.join(run4, "checkpoint_last.pt"))["data_position"]["streams"] == [[1115, 0, 4]]
    # another batch size: the stored position means nothing for it, the run falls back to a fresh shuffle
    other = [a if a != "4" or shape[i - 1] != "--batch_size" else "8" for i, a in enumerate(shape)]
    run5 = cli.main(other + ["--work_dir", str(tmp_path / "work5"), "--max_step", "6", "--resume", path])
    assert "batch stream resumed" not in open(os.path.join(run5, "train_rank0.log")).read()
