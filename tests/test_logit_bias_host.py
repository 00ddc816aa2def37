"""Constrained sampling, host side (no GPU): the constraint rows token_constraints builds and everything it refuses, the
generate.py --logit_bias file form, and the numpy restatement of the sampling step (logit_bias_contract.restate) that
the GPU tests use as their reference -- checked here against the reference's own probabilities with a zero bias."""
import importlib.util
import json
import os

import numpy as np
import pytest

import logit_bias_contract as LB

V = 729
NEG = -np.inf


def _gen():
    from commu_amd import generate
    return generate


def test_rows_for_bans_bias_and_ranges():
    G = _gen()
    row = G.token_constraints()
    assert row.dtype == np.float32 and row.shape == (768,) and not row.any()
    row = G.token_constraints(ban=[5, 728, 1], bias={7: 1.5, "9": -2, 11: NEG})
    assert set(np.flatnonzero(row == NEG)) == {1, 5, 11, 728}
    assert row[7] == np.float32(1.5) and row[9] == -2 and np.count_nonzero(row) == 6
    assert G.token_constraints(ban=[7], bias={7: 3.0})[7] == NEG          # a ban stays a ban
    assert G.token_constraints(bias=[(3, 0.25)])[3] == 0.25               # pairs work like a mapping
    # pitch tokens are 3 + MIDI note number: (60, 72) keeps 63 .. 75
    row = G.token_constraints(pitch_range=(60, 72))
    assert list(np.flatnonzero(row == NEG)) == list(range(3, 63)) + list(range(76, 131))
    assert list(np.flatnonzero(G.token_constraints(pitch_range=(0, 127)) == NEG)) == []
    assert list(np.flatnonzero(G.token_constraints(pitch_range=(59.5, 60.5)) != NEG)[:4]) == [0, 1, 2, 63]
    # velocity tokens are 131 + bin; the meta tokens' mapping: floor(min / 2) .. ceil(max / 2)
    row = G.token_constraints(velocity_range=(60, 81))
    assert list(np.flatnonzero(row == NEG)) == list(range(131, 131 + 30)) + list(range(131 + 42, 195))
    row = G.token_constraints(velocity_range=(1, 127))                   # ceil(127 / 2) = 64 is past the last bin
    assert list(np.flatnonzero(row == NEG)) == []
    both = G.token_constraints(ban=range(195, 304), pitch_range=(40, 80), velocity_range=(40, 100), bias={2: -1.0})
    assert int((both == NEG).sum()) == 109 + (128 - 41) + (64 - 31) and both[2] == -1.0
    assert not both[729:].any() and both[0] == 0


@pytest.mark.parametrize("kw, numbers", [
    (dict(ban=[0]), "0"), (dict(ban=[729]), "729"), (dict(ban=[-3]), "-3"), (dict(bias={900: 1.0}), "900"),
    (dict(ban=[1.5]), "1.5"), (dict(ban=[True]), "True"), (dict(bias={"x": 1.0}), "'x'"),
    (dict(bias={5: float("nan")}), "5 has nan"), (dict(bias={6: float("inf")}), "6 has inf"),
    (dict(bias={6: "1"}), "token 6"),
    (dict(pitch_range=(72, 60)), r"\(72, 60\)"), (dict(pitch_range=(128, 140)), r"\(128, 140\)"),
    (dict(pitch_range=(60.2, 60.8)), r"\(60.2, 60.8\)"), (dict(pitch_range=(60,)), r"\(60,\)"),
    (dict(velocity_range=(90, 30)), r"\(90, 30\)"), (dict(velocity_range=(-9, -1)), r"\(-9, -1\)"),
    (dict(velocity_range=(float("nan"), 3)), "nan"),
    (dict(ban=range(1, 729)), "all of ids 1 .. 728"),
])
def test_refusals_name_the_numbers(kw, numbers):
    G = _gen()
    with pytest.raises(G.CommuHipError, match=numbers):
        G.token_constraints(**kw)


def test_row_validation_of_the_entry_points():
    """What set_logit_bias / generate(logit_bias=) accept: one row or one per slot, 729 or 768 wide, no NaN, no +inf,
    and something left to draw in every row."""
    G = _gen()
    ok = G.token_constraints(ban=[5])
    rows = G.logit_bias_rows(ok, 3)
    assert rows.shape == (3, 768) and rows.dtype == np.float32 and (rows[:, 5] == NEG).all()
    rows = G.logit_bias_rows(np.stack([ok[:729], np.zeros(729, np.float32)]), 2)
    assert rows.shape == (2, 768) and rows[0, 5] == NEG and not rows[1].any()
    for bad, numbers in ((np.zeros(700, np.float32), r"\(700,\)"), (np.zeros((2, 768), np.float32), r"\(2, 768\)"),
                         (np.full(768, np.nan, np.float32), "entry 0 is nan"),
                         (np.where(np.arange(768) == 9, np.inf, 0).astype(np.float32), "entry 9 is inf"),
                         (np.where(np.arange(768) == 0, 0, NEG).astype(np.float32), "1 .. 728 are banned")):
        with pytest.raises(G.CommuHipError, match=numbers):
            G.logit_bias_rows(bad, 3)
    with pytest.raises(G.CommuHipError, match="row 1"):
        G.logit_bias_rows(np.stack([ok, np.full(768, NEG, np.float32)]), 2)


def _cli():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "commu-code_amd", "generate.py")
    spec = importlib.util.spec_from_file_location("commu_generate_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_file_form(tmp_path):
    G, cli = _gen(), _cli()
    f = tmp_path / "bias.json"
    f.write_text(json.dumps({"ban": [200, 201], "bias": {"2": -1.5, "500": 2}}))
    row = cli.read_constraints(str(f), 60, None)
    want = G.token_constraints(ban=[200, 201], bias={2: -1.5, 500: 2.0}, pitch_range=(60, 127))
    assert np.array_equal(row, want) and row[200] == NEG and row[500] == 2 and row[3 + 59] == NEG and row[3 + 60] == 0
    assert cli.read_constraints(None, None, None) is None
    assert np.array_equal(cli.read_constraints(None, None, 72), G.token_constraints(pitch_range=(0, 72)))
    args = cli.parse_args()["input_args"].parse_args(["--output_dir", "o", "--logit_bias", str(f), "--pitch_min", "40",
                                                      "--pitch_max", "90"])
    assert (args.logit_bias, args.pitch_min, args.pitch_max) == (str(f), 40, 90)
    for doc, err in (([1, 2], "JSON object"), ({"bans": [1]}, "bans"), ({"ban": 5}, '"ban" is a list'),
                     ({"bias": [1]}, '"bias" is an object'), ({"ban": [729]}, "729"), ({"bias": {"5": None}}, "token 5")):
        f.write_text(json.dumps(doc))
        with pytest.raises(G.CommuHipError, match=err):
            cli.read_constraints(str(f))
    f.write_text("{not json")
    with pytest.raises(ValueError, match="not JSON"):
        cli.read_constraints(str(f))
    with pytest.raises(G.CommuHipError, match=r"\(80, 40\)"):
        cli.read_constraints(None, 80, 40)


def test_restatement_reproduces_the_reference_probabilities(golden_dir):
    """calc_probs + apply_sampling of the reference (g9_sampling.npz, compounded temperature and greedy included) from the
    restatement with a ZERO bias and with none, within the bound of the oracle's own test (test_g9_sampling_probs)."""
    z = np.load(os.path.join(golden_dir, "g9_sampling.npz"))
    zero = np.zeros(768, np.float32)
    n = 0
    for c in range(int(z["ncase"])):
        row = z[f"c{c}_logits"].astype(np.float32).copy()
        temp = float(z[f"c{c}_temp"])
        for r in range(int(z[f"c{c}_rounds"])):
            wrong = np.zeros(V, np.uint8)
            wrong[z[f"c{c}_r{r}_wrong"].tolist()] = 1
            ref = z[f"c{c}_r{r}_probs"]
            a = LB.restate(row, temp, 32, wrong=wrong, bias=zero)
            b = LB.restate(row, temp, 32, wrong=wrong)
            assert np.abs(a.probs - ref).max() < 1e-6, (c, r)
            assert ((a.probs > 0) == (ref > 0)).all() and a.probs[0] == 0
            assert np.array_equal(a.probs, b.probs) and np.array_equal(a.written, b.written) and a.token == b.token
            row = a.written                                             # the next round divides again (Q5)
            n += 1
    assert n >= 10


def test_restatement_order_and_write_back():
    """The properties the GPU tests lean on, on the restatement itself: the bias is not written back, a ban is an exact
    zero and takes none of the k places -- and the same bans applied AFTER top-k (the place of the rejected-token mask)
    fail that check, so the check tells the two orders apart."""
    g = np.random.RandomState(3)
    raw = (g.standard_normal(768) * 2.5).astype(np.float32)
    k = 8
    top = (np.argsort(-raw[1:V], kind="stable")[:k] + 1).tolist()
    bias = np.zeros(768, np.float32)
    bias[top] = NEG
    bias[40] = 1.25
    free = LB.restate(raw, 0.95, k)
    res = LB.restate(raw, 0.95, k, bias=bias)
    assert np.array_equal(res.written, free.written)                     # never written back
    assert (res.probs[top] == 0).all() and LB.ban_is_before_topk(res, top, k)
    nxt = set((np.argsort(-res.y[1:V], kind="stable")[:k] + 1).tolist())
    assert set(np.flatnonzero(res.probs > 0)) == nxt and not nxt & set(top)
    late = LB.restate(raw, 0.95, k, bias=bias, ban_after_topk=True)
    assert late.token == -1 and np.isnan(late.probs).all()               # zero mass: the Q12 exit
    assert not LB.ban_is_before_topk(late, top, k)
    # full is the log-softmax of y, kept that of the survivors: full <= kept, and the +1.25 moved id 40
    assert res.full[res.token] <= res.kept <= 0
    assert abs((res.full[40] - res.full[41]) - (free.full[40] - free.full[41]) - 1.25) < 1e-5
    # a re-draw adds the bias once to the compounded row
    again = LB.restate(res.written, 0.95, k, bias=bias)
    assert np.array_equal(again.y[50], np.float32(np.float32(raw[50] / np.float32(0.95)) / np.float32(0.95)) + bias[50])
    # greedy: argmax of raw + bias, ties to the lowest id, nothing written
    raw2 = np.zeros(768, np.float32)
    raw2[10], raw2[20], raw2[30] = 5, 3, 9
    b2 = np.zeros(768, np.float32)
    b2[20], b2[30] = 2, NEG
    gr = LB.restate(raw2, 0.0, 32, bias=b2)
    assert gr.token == 10 and gr.kept == 0.0 and np.array_equal(gr.written, raw2)
    # everything banned, and the one allowed id rejected: nothing to draw
    allb = np.full(768, NEG, np.float32)
    assert LB.restate(raw, 0.95, 32, bias=allb).token == -1
    allb[77] = 0
    w = np.zeros(V, np.uint8)
    assert LB.restate(raw, 0.95, 32, bias=allb).token == 77
    w[77] = 1
    assert LB.restate(raw, 0.95, 32, bias=allb, wrong=w).token == -1


def test_cli_refuses_malformed_constraints_before_anything_is_loaded(tmp_path):
    """main() reads the constraints first: a malformed file or an empty range raises before the checkpoint (which does
    not exist here) is looked at."""
    G, cli = _gen(), _cli()
    f = tmp_path / "bias.json"
    f.write_text(json.dumps({"ban": [1000]}))
    parsers = cli.parse_args()
    for extra, err in ((["--logit_bias", str(f)], "1000"), (["--pitch_min", "90", "--pitch_max", "30"], r"\(90, 30\)")):
        argv = ["--checkpoint_dir", str(tmp_path / "missing.pt"), "--output_dir", str(tmp_path / "out"), "--num_generate", "1"]
        margs, _ = parsers["model_args"].parse_known_args(argv + extra)
        iargs, _ = parsers["input_args"].parse_known_args(argv + extra)
        with pytest.raises(G.CommuHipError, match=err):
            cli.main(margs, iargs)
    assert not (tmp_path / "out").exists()
