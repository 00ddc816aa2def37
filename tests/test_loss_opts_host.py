"""CPU proof for tests/loss_opts_contract.py and the host side of the loss options: the float64 reference against torch and
autograd, the clean fp32 emulations at or below half of every bound with every planted defect caught, the token-family
table, the refusals of the command line, and the batch stream resumed from a stored position."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import loss_opts_contract as LC
import train_contract as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = 0.5
CASES = [TC.CeInputs(V, ldl, rows) for V, ldl, rows in TC.ce_fwd_cases()]


def clean(res):
    """the half-bound rule of tests/test_train_contract_host.py: a figure with a NAME~ companion may reach 1.0"""
    for k, v in res.items():
        if k + "~" in res:
            assert v <= 1.0, (k, v)
    return max(v for k, v in res.items() if k + "~" not in res)


def test_reference_is_torch_cross_entropy_with_label_smoothing():
    for inp, eps in itertools.product(CASES, (0.0, 0.1, 0.5)):
        x = torch.from_numpy(inp.x[:, :inp.V].astype(np.float64))
        want = torch.nn.functional.cross_entropy(x, torch.from_numpy(inp.target), label_smoothing=LC.f32v(eps),
                                                 reduction="none").numpy()
        got = LC.opts_ref(inp, eps, 0.0)["loss"]
        assert np.abs(got - want).max() <= 1e-12, (inp.V, inp.rows, eps, np.abs(got - want).max())


def test_reference_gradient_is_autograd_of_the_loss():
    for inp, (eps, zeta) in itertools.product(CASES, LC.OPTS + ((0.3, 1e-2),)):
        e, z = LC.f32v(eps), LC.f32v(zeta)
        x = torch.from_numpy(inp.x[:, :inp.V].astype(np.float64)).requires_grad_(True)
        t = torch.from_numpy(inp.target)
        lse = torch.logsumexp(x, 1)
        loss = (1 - e) * (lse - x[torch.arange(inp.rows), t]) + e * (lse - x.mean(1)) + z * lse ** 2
        assert np.abs(loss.detach().numpy() - LC.opts_ref(inp, eps, zeta)["loss"]).max() <= 1e-12
        (loss * torch.from_numpy(inp.g.astype(np.float64))).sum().backward()
        want, _ = LC.grad_ref(inp, lse.detach().numpy(), eps, zeta)
        assert np.abs(x.grad.numpy() - want).max() <= 1e-12, (inp.V, inp.rows, eps, zeta)


def test_clean_emulations_stay_below_half_and_defects_are_caught():
    wf = wb = 0.0
    caught_f = {d: False for d in LC.FWD_DEFECTS}
    caught_b = {(d, bits): False for d in LC.BWD_DEFECTS for bits in (8, 24)}
    for V, ldl, ldd, rows in TC.ce_bwd_cases():
        inp = TC.CeInputs(V, ldl, rows)
        l32 = TC.ce_lse32(inp)
        for eps, zeta in LC.OPTS:
            if ldl == ldd:
                wf = max(wf, clean(LC.check_fwd(inp, eps, zeta, *LC.fwd_emu(inp, eps, zeta))))
            for bits in (8, 24):
                wb = max(wb, clean(LC.check_bwd(inp, l32, eps, zeta, LC.bwd_emu(inp, l32, eps, zeta, ldd, bits=bits), ldd, bits)))
        eps, zeta = 0.1, 1e-4
        for d in LC.FWD_DEFECTS:
            if max(LC.check_fwd(inp, eps, zeta, *LC.fwd_emu(inp, eps, zeta, d)).values()) > 1.0:
                caught_f[d] = True
        for d, bits in caught_b:
            if max(LC.check_bwd(inp, l32, eps, zeta, LC.bwd_emu(inp, l32, eps, zeta, ldd, d, bits), ldd, bits).values()) > 1.0:
                caught_b[(d, bits)] = True
    print(f"ce_fwd_opts: worst clean ratio {wf:.3f}; ce_bwd_opts: {wb:.3f}")
    assert wf <= CLEAN and wb <= CLEAN, (wf, wb)
    assert all(caught_f.values()) and all(caught_b.values()), (caught_f, caught_b)


def test_default_options_emulate_the_plain_kernels_bit_for_bit():
    for V, ldl, ldd, rows in TC.ce_bwd_cases():
        inp = TC.CeInputs(V, ldl, rows)
        l32 = TC.ce_lse32(inp)
        loss, nll, lse = LC.fwd_emu(inp, 0.0, 0.0)
        pn, pl = TC.ce_fwd_emu(inp)
        assert TC.exact(nll, pn) == 0.0 and TC.exact(lse, pl) == 0.0 and TC.exact(loss, pn) == 0.0
        assert TC.exact(LC.bwd_emu(inp, l32, 0.0, 0.0, ldd), TC.ce_bwd_emu(inp, l32, ldd)) == 0.0


def test_nll_by_class_reference_and_cases():
    for rows in LC.NLL_ROWS:
        inp = LC.NllInputs(rows)
        sums, mags, cnts = LC.nll_by_class_ref(inp)
        assert cnts.sum() == int((inp.target != inp.pad).sum()) and (rows < 100 or (cnts > 0).all())
        assert LC.nll_by_class_check(inp, sums.astype(np.float32), cnts) == {"sum": pytest.approx(0.0, abs=0.5), "count": 0.0}
        wrong = cnts.copy()
        wrong[int(np.argmax(cnts))] += 1                       # a counted pad row
        assert LC.nll_by_class_check(inp, sums, wrong)["count"] == float("inf")
    assert LC.nll_blocks(4099) > 1 and LC.nll_blocks(33) == 1


def test_every_token_is_in_exactly_one_family():
    from commu_amd.midi_generator import meta
    from commu_amd.midi_generator.midi_inferrer import TOKEN_OFFSET as T
    table = meta.class_of_token(T.VOCAB_SIZE)
    fam = meta.TOKEN_FAMILIES
    assert len(table) == 729 and len(fam) == LC.N_CLASSES and set(table) <= set(range(len(fam)))
    ranges = meta.token_family_ranges()
    hits = np.zeros(729, dtype=int)
    for name, ids in ranges.items():
        hits[list(ids)] += 1
        assert all(table[t] == fam.index(name) for t in ids)
    assert (hits == 1).all()                                   # the seven ranges tile the vocabulary: "other" is empty
    count = {name: table.count(i) for i, name in enumerate(fam)}
    assert count == {"pad_eos_bar": T.PITCH, "pitch": T.NOTE_VELOCITY - T.PITCH, "velocity": T.CHORD_START - T.NOTE_VELOCITY,
                     "chord": T.CHORD_END + 1 - T.CHORD_START, "duration": T.POSITION - T.NOTE_DURATION,
                     "position": meta.POSITION_RESOLUTION, "meta": T.VOCAB_SIZE - T.BPM, "other": 0}
    assert T.POSITION == meta.POSITION_BASE and T.BPM == min(meta._BASE.values())
    assert len(set(meta.CHORD_VOCAB.values())) == count["chord"]
    assert meta.class_of_token(800)[729:] == [fam.index("other")] * 71


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "commu-code_amd"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("commu_train_cli", os.path.join(ROOT, "commu-code_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("flags", (["--label_smoothing", "1.0"], ["--label_smoothing", "-0.1"], ["--label_smoothing", "nan"],
                                   ["--z_loss=-1e-4"], ["--z_loss", "inf"], ["--z_loss", "nan"]))
def test_cli_refuses_bad_loss_options_before_anything_is_built(flags, monkeypatch):
    cli = _cli()
    import commu_amd.model.dataset as D
    import commu_amd.train as TR

    def never(*a, **k):
        raise AssertionError("a dataset or a model was built before the refusal")
    monkeypatch.setattr(D, "ComMUDataset", never)
    monkeypatch.setattr(TR, "build_model", never)
    with pytest.raises(ValueError, match="label_smoothing|z_loss"):
        cli.main(["--data_dir", "/nonexistent", "--work_dir", "/nonexistent"] + flags)


def test_cli_lists_the_flags_and_the_config_keys():
    cli = _cli()
    args = cli.parse_args(["--data_dir", "d", "--work_dir", "w", "--label_smoothing", "0.1", "--z_loss", "1e-4",
                           "--report_families"])
    assert (args.label_smoothing, args.z_loss, args.report_families) == (0.1, 1e-4, True)
    cli.check_loss_args(args)
    from commu_amd.model.config_helper import get_default_cfg_training
    tr = get_default_cfg_training().TRAIN
    assert (tr.label_smoothing, tr.z_loss, tr.report_families) == (0.0, 0.0, False)


def test_model_refuses_bad_loss_options():
    from commu_amd.model.model import check_loss_options
    assert check_loss_options() == (0.0, 0.0) and check_loss_options(0.1, 1e-4) == (0.1, 1e-4)
    for bad in ((1.0, 0.0), (-0.5, 0.0), (0.0, -1.0), (0.0, float("inf")), (float("nan"), 0.0)):
        with pytest.raises(ValueError):
            check_loss_options(*bad)


def _corpus():
    from commu_amd.model.dataset import ComMUDataset
    rng = np.random.default_rng(5)
    seqs = [rng.integers(2, 700, size=int(n)).astype(np.int64) for n in rng.integers(20, 90, size=14)]
    return ComMUDataset(None, None, sequences={"train": seqs, "valid": seqs[:4]})


def _take(it, n):
    """n batches of a stream and the position after each of them"""
    out = []
    gen = it()
    try:
        for _ in range(n):
            d, t, r, ntok = next(gen)
            out.append((d.clone(), t.clone(), r.clone(), ntok, dict(it.position)))
    finally:
        gen.close()
    return out


def test_resumed_stream_equals_the_uninterrupted_one():
    """the native packer on CPU tensors: a stream started at the stored position hands out the batches that followed it,
    inside an epoch, at an epoch's last batch and in a later epoch"""
    ds = _corpus()
    fresh = _take(ds.get_iterator(3, 16, "cpu", "train", True, seed=1111), 40)
    epochs = [b[4]["epoch"] for b in fresh]
    assert epochs[0] == 0 and epochs[-1] >= 2                  # the stream crosses epochs
    last = max(i for i, e in enumerate(epochs) if e == 0)      # the last batch of epoch 0
    for k in (0, 5, last, last + 1, 30):
        pos = fresh[k][4]
        again = _take(ds.get_iterator(3, 16, "cpu", "train", True, seed=1111, start=(pos["epoch"], pos["index"])), 40 - k - 1)
        for a, b in zip(again, fresh[k + 1:]):
            assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]
    other = _take(ds.get_iterator(3, 16, "cpu", "train", True, seed=1112, start=(0, 5)), 1)
    assert not torch.equal(other[0][0], fresh[5][0])           # the position means something only with its seed
    with pytest.raises(ValueError):
        _take(ds.get_iterator(3, 16, "cpu", "train", True, seed=1111, start=(0, 10 ** 6)), 1)
    with pytest.raises(ValueError):
        ds.get_iterator(3, 16, "cpu", "train", False, start=(0, 1))


def test_resume_position_of_a_checkpoint_dictionary():
    """the stored seed is the one the stream was really drawn from (rank 1 below: a fresh shuffle at step 40), and a position
    means something only for the layout it was scheduled for"""
    from commu_amd.train import resume_position, stream_key
    lens = np.array([30, 41, 52, 17])
    key = stream_key(2, 4, 16, lens)
    assert key == {"world": 2, "batch_size": 4, "bptt": 16, "corpus": [4, key["corpus"][1]]}
    ck = {"data_position": dict(key, streams=[[1111, 0, 7], [2151, 1, 3]])}
    assert resume_position(ck, 1, key) == (2151, (1, 3)) and resume_position(ck, 0, key) == (1111, (0, 7))
    for other in (stream_key(1, 4, 16, lens), stream_key(2, 8, 16, lens), stream_key(2, 4, 32, lens),
                  stream_key(2, 4, 16, lens[:3]), stream_key(2, 4, 16, lens + 1)):
        assert resume_position(ck, 0, other) is None
    assert resume_position({"model": {}}, 0, key) is None  # a checkpoint written before the key existed
    assert resume_position({"data_position": {"seed": 1111, "world": 2, "positions": [[0, 7], [1, 3]]}}, 0, key) is None


def test_cli_accepts_the_loss_options_under_parity():
    """--parity trains (fp32 forward, backward and optimiser step): the loss options apply to it and are not refused"""
    cli = _cli()
    args = cli.parse_args(["--data_dir", "d", "--work_dir", "w", "--parity", "--label_smoothing", "0.1", "--z_loss", "1e-4"])
    cli.check_loss_args(args)
    assert args.parity and (args.label_smoothing, args.z_loss) == (0.1, 1e-4)
