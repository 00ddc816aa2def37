"""Form takes on the GPU (docs/EXPERIMENTS.md 9h): a bar may replay a bar of a finished sequence the user supplied.  As for
the form rule itself the defining test needs no model and no tolerance: crafted rows driven through
commu_forcing_pre_form_src / commu_forcing_post_form_src, the test itself writing the drawn tokens, must leave seq, the
record, form_state, form_tok, draw, keep, active and tok equal to the plain-Python contract (take_contract) after every
iteration -- and, through the entry points without a buffer, equal to the contract with every take row free.  Then through the
decode loop (captured graph == eager == separate launches, slots without a take token for token a decoder that never heard of
the rule, takes switched in place under one capture), the request pool through both arm launches and the command line."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import prime_contract as PC  # noqa: E402
import take_contract as TC  # noqa: E402
import test_form_gpu as FG  # noqa: E402
import test_form_host as FH  # noqa: E402
import test_grammar_host as GRH  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_takes_host as TH  # noqa: E402

DEV = "cuda"
V = 729
BAR, EOS = 2, 1
bits, run, separate_launches = FG.bits, FG.run, FG.separate_launches
CTX, N0 = FH.CTX, FH.N0
LD_SEQ, LD_CHORD, ITERS = FG.LD_SEQ, FG.LD_CHORD, FG.ITERS


# ------------------------------------------------------------------------------------------------ 1. the transitions
@pytest.mark.parametrize("entry", ["with_the_buffer", "the_old_entry_points"])
def test_the_transitions_equal_the_contract_after_every_iteration(entry):
    """Fails on the parent: the library has no commu_forcing_pre_form_src.  the_old_entry_points: the same table through
    commu_forcing_pre_form / commu_forcing_post_form, where every take row is free."""
    from commu_amd._lib import call
    rows, buf = TH.transition_rows()          # (test_takes_host drives the same rows on the contract alone)
    B = len(rows)
    src = buf if entry == "with_the_buffer" else None
    NF, NS = call("commu_forcing_state_ints"), call("commu_form_state_ints")
    assert NS == TC.NS and NF == PC.NF
    table, ctl = TH.packed(rows)
    i32 = torch.int32
    dev = lambda a, dt=i32: torch.tensor(a, dtype=dt, device=DEV)
    fsm = np.zeros((B, NF), dtype=np.int32)
    seq = np.zeros((B, LD_SEQ), dtype=np.int32)
    ctok, cpos = np.zeros((B, LD_CHORD), dtype=np.int32), np.zeros((B, LD_CHORD), dtype=np.int32)
    for b, (_, setting, _, _) in enumerate(rows):
        fsm[b] = PC.initial_record(len(GRH.META), len(setting["tok"]), setting["nm"])
        seq[b, :N0] = CTX
        ctok[b, :len(setting["tok"])], cpos[b, :len(setting["pos"])] = setting["tok"], setting["pos"]
    d_fsm, d_seq, d_ctok, d_cpos = dev(fsm), dev(seq), dev(ctok), dev(cpos)
    d_table, d_ctl = dev(np.array(table, dtype=np.uint32).view(np.int32)), dev(ctl)
    d_src = dev(buf)                                                 # (exactly the buffer: nothing behind its last int)
    d_state = torch.full((B, NS), 77, dtype=i32, device=DEV)
    d_ftok = torch.full((B,), 55, dtype=i32, device=DEV)
    d_wrong = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
    d_utable = torch.full((B, 8), 0.5, device=DEV)
    d_tok = torch.zeros(B, dtype=torch.long, device=DEV)
    d_active, d_keep, d_draw = (torch.zeros(B, dtype=torch.uint8, device=DEV) for _ in range(3))
    d_uni = torch.zeros(B, device=DEV)
    ld_trace = 2 * ITERS + 2
    d_trace = torch.zeros(B, ld_trace, dtype=i32, device=DEV)
    d_token = torch.zeros(B, dtype=i32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call("commu_form_reset", p(d_state), p(d_ftok), p(d_fsm), p(d_seq), LD_SEQ, 0, B, s)
    form = (p(d_ctl), p(d_table), len(table), p(d_state), p(d_ftok))
    if src is not None:
        form += (p(d_src), len(buf))
    pre_fn, post_fn = (("commu_forcing_pre_form_src", "commu_forcing_post_form_src") if src is not None
                       else ("commu_forcing_pre_form", "commu_forcing_post_form"))
    ref = [dict(s=list(fsm[b]), st=TC.initial_state(list(CTX)), seq=list(CTX), n=0, replayed=0) for b in range(B)]

    def download():
        return (torch.cat([d_fsm, d_state, d_ftok[:, None], d_draw[:, None].int(), d_keep[:, None].int(),
                           d_active[:, None].int(), d_tok[:, None].int(), d_seq], 1).cpu().numpy())

    def compare(what, it, want_flags=None):
        g = download()
        for b in range(B):
            r, name = ref[b], rows[b][0]
            o = 0
            assert g[b, o:o + NF].tolist() == [int(x) for x in r["s"]], (what, it, name, "record")
            o += NF
            assert g[b, o:o + NS].tolist() == r["st"], (what, it, name, "form_state", g[b, o:o + 8].tolist(), r["st"][:8])
            o += NS
            n = len(r["seq"])
            assert g[b, o + 5:o + 5 + n].tolist() == r["seq"], (what, it, name, "seq")
            if want_flags is not None:
                t, act, kp, dr, ft = want_flags[b]
                assert (g[b, o], g[b, o + 1], g[b, o + 2], g[b, o + 3], g[b, o + 4]) == (ft, dr, kp, act, t), (what, it, name)

    for it in range(ITERS):
        call(pre_fn, p(d_fsm), p(d_seq), LD_SEQ, p(d_ctok), p(d_cpos), LD_CHORD, p(d_wrong), p(d_utable), 8,
             1 << 30, p(d_tok), p(d_active), p(d_keep), p(d_draw), p(d_uni), p(d_trace), ld_trace, None, *form, B, s)
        flags, token = [], np.zeros(B, dtype=np.int32)
        for b, (_, setting, _, script) in enumerate(rows):
            r = ref[b]
            f = TC.pre(r["s"], r["st"], r["seq"], setting["tok"], setting["pos"], 1 << 30, LD_SEQ, ctl[b], table, src)
            flags.append(f)
            if f[3]:
                token[b] = script[r["n"] % len(script)]
                r["n"] += 1
            else:
                token[b] = 600 + b
            r["replayed"] += f[4] >= 0 and bool(r["st"][TC.ROW] & TC.TAKE)
        compare("pre", it, flags)
        d_token.copy_(torch.from_numpy(token))
        call(post_fn, p(d_fsm), p(d_seq), LD_SEQ, p(d_cpos), LD_CHORD, p(d_wrong), p(d_draw), p(d_token), None,
             None, p(d_keep), 1 << 30, None, None, *form, B, s)
        for b, (_, setting, _, _) in enumerate(rows):
            r, (t, act, kp, dr, ft) = ref[b], flags[b]
            if dr or ft >= 0:
                TC.post(r["s"], r["st"], r["seq"], setting["pos"], ft if ft >= 0 else int(token[b]), LD_SEQ, ctl[b], table, src)
        compare("post", it)
    n_take = TH.check_rows(rows, buf, ref, src)          # (the rows did what they were written for)
    print("random rows: tokens replayed from a take:", n_take)


# ------------------------------------------------------------------------------------------------ 2. through the loop
loaded, fixture_model, drawn_mask = FG.loaded, FG.fixture_model, FG.drawn_mask


def check_take_slot(z, seq, lp, form, kept, redone=(), take=None):
    """A slot under a keep form: it parses, the checker and its reference accept it, the bars `kept` are closed and hold
    the take's groups (at least one of them two), the bars `redone` were drawn."""
    from commu_amd.generate import form_template, form_violation
    from commu_amd.midi_generator.midi_inferrer import parse_events
    n_ctx = 1 + len(z["encoded_meta"])
    assert seq is not None and parse_events(seq, n_ctx) is None, seq
    drawn = drawn_mask(seq, lp)
    assert form_violation(seq, n_ctx, form, drawn) is None, seq
    t = form_template(form)
    assert TC.form_violation(seq, n_ctx, t.tolist(), t.takes[0].tolist(), drawn) is None
    cb = FH.closed_bars(seq)
    assert len(cb) > max(kept) and len(FH.closed_bars(take)) > max(kept), seq
    for i in kept:
        assert TH.bar_groups(seq, i) == TH.bar_groups(take, i), i
    assert any(len(TH.bar_groups(seq, i)) >= 2 for i in kept)
    for i in redone:
        if i < len(cb):          # (a position may be forced: a chord's)
            assert all(all(drawn[g + 1:g + 4]) for g in TH.group_starts(seq, cb[i][0] + 1, cb[i][1])), i


def test_take_slots_through_the_loop(fixture_model):
    """Fails on the parent: form_template knows no takes.  Slot 0 keeps its own earlier take except bar 1, slot 2 keeps the
    take of slot 0 and redraws the pitches of bar 1; slots 1 and 3 have no form."""
    z, model = fixture_model
    B = 4
    plain = loaded(z, model, B)
    s0, f0, l0 = run(plain)
    free = plain.sequences()[0]
    take = free[0]
    assert take is not None and take.count(BAR) >= 4, take
    forms = [{"keep": {"from_tokens": take}, "redo": [1]}, None, {"keep": {"from_tokens": take}, "repitch": [1]}, None]
    res = []
    for mode in ("graph", "eager", "separate"):
        dec = loaded(z, model, B, form=list(forms))
        assert dec.form_src is not None and dec._form_src_used == len(take)           # (one take, placed once)
        if mode == "separate":
            res.append(separate_launches(dec, dec.generation_length + 1))
        else:
            res.append(run(dec, use_graph=mode == "graph"))
        if mode == "graph":
            assert dec.graph is not None
            seqs, lps = dec.sequences()[0], dec.logprobs()
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
        assert torch.equal(bits(res[0][2]), bits(other[2]))
    sg, fg, lg = res[0]
    for b in (1, 3):          # (the whole record: F_NDRAW included)
        assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
    check_take_slot(z, seqs[0], lps[0], forms[0], kept=(0, 2), redone=(1,), take=take)
    check_take_slot(z, seqs[2], lps[2], forms[2], kept=(0, 2), take=take)
    # bar 0 of slot 0 is the take's bar 0 -- its own -- but none of it was drawn this time
    cb = FH.closed_bars(seqs[0])
    d0 = drawn_mask(seqs[0], lps[0])
    assert not any(d0[g + k] for g in TH.group_starts(seqs[0], cb[0][0] + 1, cb[0][1]) for k in range(4))
    # slot 2's bar 1: the take's positions, velocities and durations, pitches that were drawn
    d2, c2 = drawn_mask(seqs[2], lps[2]), FH.closed_bars(seqs[2])
    g2, gt = TH.bar_groups(seqs[2], 1), TH.bar_groups(take, 1)
    assert len(g2) == len(gt) >= 1 and [g[:2] + g[3:] for g in g2] == [g[:2] + g[3:] for g in gt]
    for a in TH.group_starts(seqs[2], c2[1][0] + 1, c2[1][1]):
        assert [d2[a + k] for k in range(4)] == [False, False, True, False]
    ndraw = fg[:, PC.F_NDRAW].tolist()
    print("variates consumed per slot:", ndraw, "; without the rule:", f0[:, PC.F_NDRAW].tolist())
    # teeth: a replay token consumes no variate and has no log-probability -- the take slots are other runs
    assert ndraw[0] < int(f0[0, PC.F_NDRAW]) and not torch.equal(bits(lg[0]), bits(l0[0]))
    assert not torch.equal(fg[2], f0[2]) and not torch.equal(bits(lg[2]), bits(l0[2]))


def test_set_form_switches_takes_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    free = plain.sequences()[0]
    take_a, take_b = free[0], free[3]
    assert take_a != take_b and min(take_a.count(BAR), take_b.count(BAR)) >= 4
    keep = lambda t: {"keep": {"from_tokens": t}, "redo": [1]}
    dec = loaded(z, model, 4, form=[None, keep(take_a), None, None])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g, table, src = dec.graph, dec.form_table, dec.form_src
    assert g is not None and src is not None
    check_take_slot(z, dec.sequences()[0][1], dec.logprobs()[1], keep(take_a), kept=(0, 2), redone=(1,), take=take_a)
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_form(keep(take_b), rows=[1])                                  # (another take for the slot: packed behind)
    dec.set_form(keep(take_a), rows=[2])                                  # (the first one again: already there)
    assert dec._form_src_used == len(take_a) + len(take_b)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.form_table is table and dec.form_src is src and dec.form_src.data_ptr() == src.data_ptr()
    seqs, lps = dec.sequences()[0], dec.logprobs()
    check_take_slot(z, seqs[1], lps[1], keep(take_b), kept=(0, 2), redone=(1,), take=take_b)
    check_take_slot(z, seqs[2], lps[2], keep(take_a), kept=(0, 2), redone=(1,), take=take_a)
    for b in (0, 3):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.set_form(None)                                                    # (all slots: the takes are reclaimed)
    assert dec._form_src_used == 0
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.form_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


# ------------------------------------------------------------------------------------------------ 3. the request pool
@pytest.mark.parametrize("primed", [False, True], ids=["commu_decode_arm", "commu_decode_arm_primed"])
def test_pool_requests_with_their_own_takes_equal_generate_stream_of_each_alone(primed):
    """Three requests -- take A, take B, no form -- through one pool: each gets what generate_stream(slots=1) of the request
    alone returns, and every result keeps its take."""
    import commu_amd.generate as G
    import pool_contract as PLC
    import pool_prime_contract as PP
    import test_pool_gpu as TP
    import test_pool_prime_gpu as TPP
    model = TP._model()
    reqs = PLC.four_requests(G)
    every = lambda seq, rep: seq is not None
    one = G.density_word(1, 1)
    base = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, logit_bias=None, density=one)
    takes = TPP._alone(TPP._generator(model), dataclasses.replace(base, need=4), grammar=True, density=one)[0]
    takes = sorted((t for t in takes if t.count(BAR) >= 3), key=len)
    take_a, take_b = takes[-1], takes[-2]
    assert take_a != take_b
    form_a = {"keep": {"from_tokens": take_a}, "redo": [1]}
    form_b = {"keep": {"from_tokens": take_b}, "repitch": [1]}
    first = dataclasses.replace(base, form=form_a)
    if primed:
        own = TPP._own_sequence(TPP._generator(model), first, 6, grammar=True, density=one, form=form_a)
        first = dataclasses.replace(first, prompt=PP.prompt_of(own, len(PLC.META), 6))
    first_want = TPP._alone(TPP._generator(model), first, grammar=True, density=one, form=form_a)
    second = dataclasses.replace(base, seed=base.seed + 1, form=form_b)
    second_want = TPP._alone(TPP._generator(model), second, grammar=True, density=one, form=form_b)
    third = dataclasses.replace(reqs[2], accept=every, grammar=False)
    third_want = TPP._alone(TPP._generator(model), third)
    gen = TPP._generator(model)
    res = gen.generate_pool([first, second, third], slots=3, grammar=True, return_logprobs=True)
    TPP._same_results(res[0], first_want)
    TPP._same_results(res[1], second_want)
    assert res[2].sequences == third_want[0] and res[2].attempts_started == third_want[1]
    assert gen.pool_stats["kernel"] == ("commu_decode_arm_primed" if primed else "commu_decode_arm")
    assert gen.pool_stats["form_src_tokens"] == len(take_a) + len(take_b)
    cut = TPP.N_CTX + (6 if primed else 0)
    n_closed = 0
    for r, form, start in ((res[0], form_a, cut), (res[1], form_b, TPP.N_CTX)):
        assert len(r.sequences) == 2
        for s, lp in zip(r.sequences, r.logprobs):
            assert G.form_violation(s, start, form, drawn_mask(s, lp)) is None, s
            n_closed += sum(1 for lo, hi in FH.closed_bars(s) if lo >= start)
    print("closed bars the loop opened under a keep form:", n_closed)
    assert n_closed >= 4
    # teeth: the take rows decide what is decoded
    free = TPP._alone(TPP._generator(model), dataclasses.replace(second, form=None), grammar=True, density=one)
    assert free[0] != second_want[0]


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_generate_cli_keep_and_redo_from_a_file(golden_dir, tmp_path, monkeypatch):
    """generate.py --grammar --form FILE with {"keep": ..., "redo": [1]} over a sequence an earlier run of the command line
    wrote: what it writes keeps the take's bars."""
    import test_model_gpu as TM
    from commu_amd.generate import form_violation
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, InferenceTask, parse_events
    z = TM.load(golden_dir, "g10_checkpoint.npz")
    cli = TM._load_script("generate")
    parsers = cli.parse_args()
    prog = "-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8)
    common = ["--checkpoint_dir", os.path.join(golden_dir, "g10_checkpoint.pt"), "--generation_length", "120", "--gpus", "1",
              "--bpm", "70", "--audio_key", "aminor", "--time_signature", "4/4", "--pitch_range", "mid_high",
              "--num_measures", "8", "--inst", "acoustic_piano", "--genre", "newage", "--min_velocity", "60",
              "--max_velocity", "80", "--track_role", "main_melody", "--rhythm", "standard", "--chord_progression",
              prog + "-" + prog, "--num_generate", "2", "--max_rounds", "1", "--decode_slots", "2", "--grammar",
              "--min_notes_per_bar", "2", "--max_notes_per_bar", "2"]
    monkeypatch.setattr(ForcingReport, "validate_teacher_forced_sequence", lambda self, seq: None)
    monkeypatch.setattr(InferenceTask, "validate_generated_sequence", lambda self, seq: True)

    def go(argv, out):
        argv = common + ["--output_dir", str(tmp_path / out)] + argv
        margs, _ = parsers["model_args"].parse_known_args(argv)
        iargs, _ = parsers["input_args"].parse_known_args(argv)
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
        return json.load(open(tmp_path / out / "sequences.json"))

    free = go([], "free")
    start = 1 + len(free["encoded_meta"])
    take = max(free["sequences"], key=lambda s: s.count(BAR))
    assert take.count(BAR) >= 3
    doc = {"keep": {"from_tokens": take}, "redo": [1]}
    path = tmp_path / "keep.json"
    path.write_text(json.dumps(doc))
    got = go(["--form", str(path)], "kept")
    assert len(got["sequences"]) >= 1
    tb = FH.closed_bars(take)
    for s in got["sequences"]:
        assert parse_events(s, start) is None, s
        assert form_violation(s, start, doc) is None, s
        cb = FH.closed_bars(s)
        assert len(cb) >= 3 and len(tb) >= 3, s
        assert TH.bar_groups(s, 0) == TH.bar_groups(take, 0) and TH.bar_groups(s, 2) == TH.bar_groups(take, 2), s
    assert any(form_violation(s, start, doc) is not None for s in free["sequences"] if s != take)
