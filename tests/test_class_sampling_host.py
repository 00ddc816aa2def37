"""Class-keyed sampling on the host (no GPU): the drawn -> after map against the default grammar, every refusal of
class_sampling(), the NaN-inheritance composition of the records through set_sampling / rearm on a decoder stub without a
device, the struct mirrors, the command line, and the numpy restatement (class_sampling_contract) walked through the forcing
rules on the 60 requests of test_grammar_host."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import class_sampling_contract as CS
import grammar_contract as GC
import prime_contract as PC
import test_grammar_host as TG

V = 729
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ 1. the map
def test_drawn_names_map_to_the_rows_of_the_default_grammar():
    from commu_amd.generate import CLASS_NAMES, DRAWN_AFTER, class_sampling, event_grammar
    assert CLASS_NAMES == CS.NAMES == tuple(n.lower() for n in GC.NAMES)
    assert DRAWN_AFTER == CS.DRAWN_AFTER
    table = GC.default_table()
    assert np.array_equal(table, event_grammar())
    claimed = set()
    for name, after in DRAWN_AFTER.items():
        ids = sorted(CS.DRAWN_IDS[name])
        # the rows whose only finite entries (ids 1 .. 728) are this family's ids ...
        rows = [c for c in range(7) if np.flatnonzero(np.isfinite(table[c, 1:V])).tolist() == [i - 1 for i in ids]]
        # ... are exactly the classes the name maps to
        assert sorted(CLASS_NAMES.index(a) for a in after) == rows, name
        claimed.update(rows)
        t = class_sampling(drawn={name: {"top_k": 5}})
        assert np.flatnonzero(~np.isnan(t[:, 1])).tolist() == rows and (t[rows, 1] == 5).all()
        assert np.isnan(t[:, [0, 2]]).all() and np.isnan(t[7]).all()
    assert claimed == set(range(7))                                     # every class is some family's
    t = class_sampling(drawn={"pitch": {"temperature": 1.1, "top_k": 40}, "duration": {"temperature": 0}},
                       after={"bar": {"top_p": 0.8}})
    want = np.full((8, 3), NAN)
    want[3, :2] = (1.1, 40)
    want[2, 0] = 0
    want[1, 2] = 0.8
    assert np.array_equal(t, want, equal_nan=True)
    assert np.isnan(class_sampling()).all()


def test_every_refusal_of_class_sampling():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import class_sampling, class_sampling_table, read_class_sampling
    for kw, msg in (
            (dict(drawn={"note": {}}), r"drawn: unknown name 'note' \(one of velocity, pitch, duration, boundary\)"),
            (dict(after={"pitches": {}}), r"after: unknown name 'pitches' \(one of other, bar, pitch"),
            (dict(drawn={"pitch": {"top_k": 4}}, after={"velocity": {"top_k": 8}}),
             r"class 3 \(velocity\) is named twice: through after 'velocity' and through drawn 'pitch'"),
            (dict(drawn={"boundary": {"top_k": 4}}, after={"chord": {"top_k": 8}}), r"class 4 \(chord\) is named twice"),
            (dict(after={"bar": {"temperature": NAN}}), r"temperature: a finite value >= 0 expected \(0 = greedy\), got nan"),
            (dict(after={"bar": {"temperature": -0.5}}), r"temperature: a finite value >= 0 expected \(0 = greedy\), got -0.5"),
            (dict(after={"bar": {"temperature": float("inf")}}), r"temperature: a finite value >= 0 expected .*got inf"),
            (dict(after={"bar": {"top_k": 0}}), r"top_k: an integer in \[1, 729\) expected, got 0.0"),
            (dict(after={"bar": {"top_k": 729}}), r"top_k: an integer in \[1, 729\) expected, got 729.0"),
            (dict(after={"bar": {"top_k": 2.5}}), r"top_k: an integer in \[1, 729\) expected, got 2.5"),
            (dict(after={"bar": {"top_p": 0}}), r"top_p: a value in \(0, 1\] expected \(1 = off\), got 0.0"),
            (dict(after={"bar": {"top_p": 1.5}}), r"top_p: a value in \(0, 1\] expected \(1 = off\), got 1.5"),
            (dict(after={"bar": {"top_p": NAN}}), r"top_p: a value in \(0, 1\] expected \(1 = off\), got nan"),
            (dict(after={"bar": {"heat": 1}}), r"unknown control 'heat'"),
            (dict(after={"bar": {"top_k": True}}), r"top_k is a number, got True"),
            (dict(after={"bar": 1.0}), r"a dict with any of temperature, top_k, top_p expected"),
            (dict(after=[("bar", {})]), r"after: a dict keyed by other, bar")):
        with pytest.raises(CommuHipError, match=msg):
            class_sampling(**kw)
    assert class_sampling(after={"bar": {"top_k": 728, "top_p": 1.0, "temperature": 0}})[1].tolist() == [0, 728, 1]
    for bad, msg in ((np.zeros((6, 3)), "7 or 8 rows"), (np.zeros((8, 2)), "7 or 8 rows"), ("x", "7 or 8 rows"),
                     (np.full((8, 3), (NAN, 729, NAN)), r"row 0: top_k: an integer in \[1, 729\) expected, got 729.0"),
                     (np.full((8, 3), (-1, NAN, NAN)), "row 0: temperature"), (np.full((8, 3), (NAN, NAN, 0)), "row 0: top_p")):
        with pytest.raises(CommuHipError, match=msg):
            class_sampling_table(bad)
    t = class_sampling_table(np.full((8, 3), (0.5, 3, 0.25)))
    assert (t[:7] == (0.5, 3, 0.25)).all() and np.isnan(t[7]).all()     # row 7 is never selected
    with pytest.raises(CommuHipError, match="a JSON object expected"):
        read_class_sampling([1])
    t, drawn = read_class_sampling({"pitch": {"top_k": 40}, "after": {"bar": {"top_p": 0.5}}})
    assert drawn and t[3, 1] == 40 and t[1, 2] == 0.5
    assert read_class_sampling({"after": {"bar": {"top_p": 0.5}}})[1] is False


# ------------------------------------------------------------------------------------------------ 2. composition
def records(dec):
    from commu_amd.generate import CLASS_CTL_DTYPE
    return dec.cls_ctl.numpy().view(CLASS_CTL_DTYPE).reshape(dec.B, 8)


def stub(B=4, triple=(0.95, 32, 1.0)):
    """A ForcedDecoder without a model or a device: the attributes its setters and rearm() touch, on the CPU."""
    from commu_amd.generate import ForcedDecoder, sampling_rows
    from commu_amd.midi_generator.midi_inferrer import ForcingReport
    dec = ForcedDecoder.__new__(ForcedDecoder)
    dec.B, dec.dev, dec.NF = B, torch.device("cpu"), 14
    dec.rows_on = False
    dec._sampling = sampling_rows(B, *triple)
    dec.temperature, dec.top_k, dec.top_p = triple
    dec.temperature_rows, dec.top_k_rows, dec.top_p_rows = (torch.from_numpy(a.copy()) for a in dec._sampling)
    dec.bias = dec.gram = dec.gram_on = dec._gram_host = dec.harm = dec.harm_on = dec._harm_host = None
    dec.cls_ctl = dec._cls_host = None
    dec.graph, dec.graph_long = "captured", "captured"
    dec.reports = [ForcingReport(4, 4.0) for _ in range(B)]
    dec._primed, dec.n_cond, dec.trace, dec.sliding, dec.shared_prompt = None, 11, None, False, False
    dec.fsm = torch.zeros(B, 14, dtype=torch.int32)
    dec.wrong = torch.zeros(B, V, dtype=torch.uint8)
    dec.seq_logp = torch.zeros(B, 8, 2)
    dec.ld_u = 4
    dec.utable = torch.zeros(B, 4)
    dec.state = types.SimpleNamespace(klen=torch.zeros(B, dtype=torch.int32))
    return dec


def test_inherited_entries_follow_set_sampling_and_rearm():
    from commu_amd.generate import class_ctl_records, class_sampling, sampling_rows
    dec = stub()
    dec.set_class_sampling(None)                                        # a decoder that never had a table: nothing happens
    assert dec.cls_ctl is None and dec.bias is None and dec.graph == "captured" and not dec.rows_on
    table = class_sampling(drawn={"pitch": {"top_k": 40}, "duration": {"temperature": 0}})
    dec.set_class_sampling(table)
    # the first table: the records, the array launches and what the one kernel reads besides; the graphs dropped once
    assert dec.rows_on and dec.graph is None and dec.graph_long is None
    assert dec.cls_ctl.shape == (4, 8, 4) and dec.cls_ctl.dtype == torch.int32
    assert dec.bias is not None and dec.gram is not None and dec.harm is not None
    assert not dec.gram_on.any() and not dec.harm_on.any() and not dec.bias.any()
    rec = records(dec)
    f32 = np.float32
    for b in range(4):
        assert rec[b].tolist() == [(f32(0.95), 32, 1.0, 0), (f32(0.95), 32, 1.0, 0), (0.0, 32, 1.0, 0), (f32(0.95), 40, 1.0, 0)] + \
            [(f32(0.95), 32, 1.0, 0)] * 4, b
    dec.graph = "again"
    ptr = dec.cls_ctl.data_ptr()
    dec.rearm(1, sampling=(0.5, 8, 1.0))                                # inherited entries follow, the override stays
    rec = records(dec)
    assert rec[1].tolist() == [(0.5, 8, 1.0, 0), (0.5, 8, 1.0, 0), (0.0, 8, 1.0, 0), (0.5, 40, 1.0, 0)] + [(0.5, 8, 1.0, 0)] * 4
    assert rec[0].tolist() == rec[2].tolist() == rec[3].tolist() and rec[0][7].tolist() == (f32(0.95), 32, 1.0, 0)
    assert dec.top_k_rows.tolist() == [32, 8, 32, 32]
    dec.set_sampling(top_p=[0.9, 0.8, 0.7, 0.6])                        # a whole batch
    rec = records(dec)
    assert [float(rec[b][c][2]) for b in range(4) for c in (0, 7)] == [float(f32(p)) for p in (0.9, 0.8, 0.7, 0.6) for _ in (0, 1)]
    assert rec[1][3].tolist() == (0.5, 40, f32(0.8), 0) and rec[2][2].tolist() == (0.0, 32, f32(0.7), 0)
    dec.set_class_sampling(class_sampling(after={"bar": {"top_p": 0.25}}), rows=[2])          # one slot, another table
    rec = records(dec)
    assert rec[2].tolist() == [(f32(0.95), 32, f32(0.7), 0), (f32(0.95), 32, 0.25, 0)] + [(f32(0.95), 32, f32(0.7), 0)] * 6
    assert rec[1][3].tolist() == (0.5, 40, f32(0.8), 0)
    dec.set_class_sampling(None)                                        # every record the slot's base triple
    rec = records(dec)
    for b in range(4):
        base = (dec._sampling[0][b], dec._sampling[1][b], dec._sampling[2][b], 0)
        assert rec[b].tolist() == [base] * 8, b
    assert dec.graph == "again" and dec.cls_ctl.data_ptr() == ptr       # in place: nothing re-captured, nothing re-allocated
    # a first table for some slots: the others hold their base triple in every record from the start
    dec = stub()
    dec.set_class_sampling(table, rows=[1])
    rec = records(dec)
    assert rec[1][3].tolist() == (f32(0.95), 40, 1.0, 0) and rec[1][2].tolist() == (0.0, 32, 1.0, 0)
    assert all(rec[b].tolist() == [(f32(0.95), 32, 1.0, 0)] * 8 for b in (0, 2, 3))
    # the composer on its own: NaN inherits, row 7 is the base triple
    r = class_ctl_records(np.stack([table, np.full((8, 3), NAN)]), sampling_rows(2, [0.0, 1.3], [1, 728], [1.0, 0.5]))
    assert r[0][3].tolist() == (0.0, 40, 1.0, 0) and r[0][7].tolist() == (0.0, 1, 1.0, 0) and r.dtype.itemsize == 16
    assert r[1].tolist() == [(f32(1.3), 728, 0.5, 0)] * 8


def test_greedy_base_with_a_sampled_class_needs_variates():
    from commu_amd.generate import class_sampling
    dec = stub(triple=(0.0, 32, 1.0))
    assert not dec.class_samples()
    dec.set_class_sampling(class_sampling(drawn={"duration": {"temperature": 0}}))
    assert not dec.class_samples()
    dec.set_class_sampling(class_sampling(drawn={"pitch": {"temperature": 1.1}}))
    assert dec.class_samples()


# ------------------------------------------------------------------------------------------------ 3. structs, CLI
def test_struct_mirrors_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        name, _ = cls._fields_[-1]
        assert name == "cls_ctl" and getattr(cls, name).offset + 8 == C.sizeof(cls)      # appended: the last field
        assert getattr(_lib.struct_args(cls), name) is None             # null unless named


def _cli_module():
    spec = importlib.util.spec_from_file_location("commu_generate_cli", os.path.join(ROOT, "commu-code_amd", "generate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_read_class_sampling_of_the_command_line(tmp_path):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import read_class_sampling
    cli = _cli_module()
    doc = {"pitch": {"temperature": 1.1, "top_k": 40}, "duration": {"temperature": 0}}
    margs = cli.parse_args()["model_args"].parse_known_args(["--grammar", "--class_sampling", json.dumps(doc)])[0]
    assert json.loads(margs.class_sampling) == doc and margs.grammar
    assert cli.parse_args()["model_args"].parse_known_args([])[0].class_sampling is None
    assert cli.read_class_sampling_arg(None) is None
    text = cli.read_class_sampling_arg(json.dumps(doc), grammar=True)
    t = read_class_sampling(json.loads(text))[0]
    assert t[3, 1] == 40 and t[2, 0] == 0
    f = tmp_path / "cs.json"
    f.write_text(json.dumps({"after": {"velocity": {"top_k": 12}}}))
    assert json.loads(cli.read_class_sampling_arg(str(f), grammar=False)) == {"after": {"velocity": {"top_k": 12}}}
    with pytest.raises(ValueError, match="duration, pitch name what is drawn next, which only --grammar fixes"):
        cli.read_class_sampling_arg(json.dumps(doc), grammar=False)
    with pytest.raises(ValueError, match="a JSON object or a readable JSON file expected"):
        cli.read_class_sampling_arg(str(tmp_path / "missing.json"))
    with pytest.raises(ValueError, match="not JSON"):
        cli.read_class_sampling_arg("{not json", grammar=True)
    with pytest.raises(CommuHipError, match=r"top_k: an integer in \[1, 729\) expected, got 900.0"):
        cli.read_class_sampling_arg(json.dumps({"pitch": {"top_k": 900}}), grammar=True)
    # the checked text reaches the inference configuration through the model arguments
    from commu_amd.midi_generator.model_initializer import ModelInitializeTask
    init = ModelInitializeTask(types.SimpleNamespace(checkpoint_dir=None, class_sampling=text))
    assert json.loads(init.inference_cfg.GENERATION.class_sampling) == doc
    assert not hasattr(ModelInitializeTask(types.SimpleNamespace(checkpoint_dir=None)).inference_cfg.GENERATION,
                       "class_sampling")


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), *args], capture_output=True,
                          text=True, timeout=120)


def test_cli_help_lists_the_flag_and_drawn_names_need_the_grammar(tmp_path):
    out = _cli("--help")
    assert out.returncode == 0 and "--class_sampling JSON_OR_FILE" in out.stdout
    common = ["--output_dir", str(tmp_path / "out"), "--checkpoint_dir", str(tmp_path / "no_such_checkpoint.pt"),
              "--num_generate", "1"]
    out = _cli(*common, "--class_sampling", json.dumps({"pitch": {"top_k": 40}}))
    assert out.returncode != 0 and "--class_sampling: pitch name what is drawn next, which only --grammar" in out.stderr
    out = _cli(*common, "--grammar", "--class_sampling", json.dumps({"pitch": {"top_k": 0}}))
    assert out.returncode != 0 and "top_k: an integer in [1, 729) expected, got 0.0" in out.stderr
    # an {"after": ...} document passes the check without --grammar: the run then fails at the missing checkpoint instead
    out = _cli(*common, "--class_sampling", json.dumps({"after": {"velocity": {"top_k": 40}}}))
    assert out.returncode != 0 and "--class_sampling" not in out.stderr and "class_sampling:" not in out.stderr
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------ 4. the walk
BASE = (0.95, 32, 1.0)


def walk(r, ctl, gram, keyed=True, on_draw=None):
    """The forcing rules (prime_contract.pre / post, one `pre` per iteration as the kernels run it) on the random logits of
    test_grammar_host.run_request, every draw made by the restatement: keyed -- class_sampling_contract with the table `ctl`;
    not keyed -- the plain restatement with the request's one triple.  What a draw writes back is what the next re-draw
    divides again (Q5).  Every draw consumes one variate, as the device loop does.  Returns seq, None after a failed draw."""
    import harmony_contract as HC
    g = torch.Generator().manual_seed(1000 + r["seed"])
    u = np.random.RandomState(r["seed"]).random_sample(256)
    seq = [0] + TG.META
    s = PC.initial_record(len(TG.META), len(r["chord_token"]), r["num_measures"])
    base = (r["temperature"],) + BASE[1:]
    wrong, logits, n_draw = np.zeros(V, np.uint8), None, 0
    while True:
        cur0 = s[PC.F_CUR]
        t, act, kp, dr = PC.pre(s, seq, r["chord_token"], r["chord_position"], 200, 1 << 30)
        if s[PC.F_DONE]:
            return seq
        if s[PC.F_CUR] != cur0:
            wrong[:] = 0
        if act:
            logits = (3.0 * torch.randn(V, generator=g)).numpy()
        if not dr:
            continue
        kw = dict(wrong=wrong, u=u[n_draw], gram=gram, prev=seq[-1])
        n_draw += 1
        if keyed:
            res = CS.restate_with_classes(logits, ctl, **kw)
        else:
            res = HC.restate_with_harmony(logits, *base, **kw)
        if on_draw is not None:
            on_draw(seq, res)
        logits = res.written
        if res.token < 0:
            return None
        token = res.token
        cur = s[PC.F_CUR]
        cp = r["chord_position"][cur] if cur < s[PC.F_NCHORD] else -1
        if cp not in (-1, PC.POS0) and (cp < token < PC.POS0 + PC.POS_RES or token == PC.BAR):
            wrong[:] = 0
        elif PC.CHORD_LO <= token <= PC.CHORD_HI:
            wrong[token] = 1
        PC.post(s, seq, r["chord_position"], token, 1 << 30)


def test_the_restatement_through_the_forcing_rules():
    gram = GC.default_table()
    reqs = TG.requests(60)
    durations = others = differ = 0
    for r in reqs:
        base = (r["temperature"],) + BASE[1:]
        plain = walk(r, None, gram, keyed=False)
        assert plain is not None and GC.parse_events(plain, 1 + len(TG.META)) is None, r
        # every record the base triple: token for token the plain walk
        assert walk(r, CS.compose(np.full((8, 3), NAN), base), gram) == plain, r
        # greedy durations: every token drawn after a pitch is the argmax of its constrained row, ties to the lowest id
        table = np.full((8, 3), NAN)
        table[GC.PITCH, 0] = 0.0
        seen = [0, 0]

        def on_draw(seq, res):
            if GC.token_class(seq[-1]) == GC.PITCH:
                best = int(np.flatnonzero(res.y[1:] == res.y[1:].max())[0]) + 1
                assert res.token == best and 304 <= best <= 431 and res.kept == 0.0, (r, seq)
                assert res.probs[best] == 1.0 and res.probs.sum() == 1.0
                seen[0] += 1
            else:
                assert (res.kept == 0.0) == (r["temperature"] == 0), (r, seq)
                seen[1] += 1
        greedy = walk(r, CS.compose(table, base), gram, on_draw=on_draw)
        assert greedy is not None and GC.parse_events(greedy, 1 + len(TG.META)) is None, r
        durations += seen[0]
        others += seen[1]
        differ += greedy != plain
    print("duration draws", durations, "other draws", others, "requests whose greedy-duration walk differs", differ)
    assert durations >= 100 and others >= 300 and differ >= 10
