"""Form templates on the GPU (docs/EXPERIMENTS.md 9f).  The rule lives in the forcing stage, so its defining test needs no
model and no tolerance: crafted rows driven through commu_forcing_pre_form / commu_forcing_post_form, the test itself writing
the drawn tokens, must leave seq, the record, form_state, form_tok, draw, keep and tok equal to the plain-Python contract
(form_contract) after every iteration.  Then through the decode loop: captured graph == eager == separate launches, free
slots token for token a decoder that never heard of the feature, a primed slot whose prompt's bars are the sources, in-place
switching under one capture, the request pool through both arm launches and the command line."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import form_contract as FC  # noqa: E402
import prime_contract as PC  # noqa: E402
import test_form_host as FH  # noqa: E402
import test_grammar_host as GRH  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402

DEV = "cuda"
V = 729
BAR, EOS = 2, 1
bits = SR.bits
run, separate_launches = LBG.run, LBG.separate_launches
CTX = FH.CTX
N0 = len(CTX)

# ------------------------------------------------------------------------------------------------ 1. the transitions
LD_SEQ = 448
LD_CHORD = 80
ITERS = 360
N_RANDOM = 20


def seam_row(offset):
    """A source bar whose one note group starts `offset` tokens behind the cursor: BAR, 432, chord, lone positions, the group."""
    return (FH.ONE, [None, 0], [BAR] + [440] * (offset - 2) + [441, 150, 63, 310] + [BAR] + FH.N3)


def random_row(rs):
    setting = (FH.ONE, FH.TWO, FH.THREE, FH.LONG)[rs.randint(4)]
    bars = [None]
    for i in range(1, rs.randint(2, 8)):
        k = rs.randint(4)
        src = int(rs.randint(i))
        bars.append(None if k == 0 else src if k == 1 else {"of": src, "copy": "rhythm"} if k == 2
                    else {"of": src, "transpose": int(rs.randint(-48, 49))})
    script = []
    for _ in range(24):
        k = rs.rand()
        grp = [432 + int(rs.randint(128)), 131 + int(rs.randint(64)), 3 + int(rs.randint(128)), 304 + int(rs.randint(128))]
        if k < 0.55:
            script += grp
        elif k < 0.75:
            script.append(BAR)
        elif k < 0.85:
            script.append(432 + int(rs.randint(128)))
        elif k < 0.9:
            script.append(195 + int(rs.randint(109)))          # a chord token: rejected, drawn again
        elif k < 0.95:
            script.append(EOS)
        else:
            script += grp[:3] + [BAR]                            # a note the bar line cuts
    return setting, bars, script


def transition_rows():
    """(name, setting, the form's bars, script): the host test's walks, the chunk seams, and random rows over random forms."""
    rows = [(name, w[0], w[1], w[2]) for name, w in FH.WALKS.items()]
    rows.append(("a_65th_bar", FH.LONG, [None] + [0] * 63, FH.LONG_WALKS["empty_bars"][0]))
    # a group that starts at offsets 60, 61, 63 and 64 from the cursor (the seam between two chunks); 130: three chunks;
    # 57 .. 59 and 62: with the others, `end` lies 1, 2, 3 short of the chunk's end, at it, and 1, 2, 3, 4 past it
    for off in (57, 58, 59, 60, 61, 62, 63, 64, 130):
        rows.append((f"group_at_offset_{off}",) + seam_row(off))
    rs = np.random.RandomState(5)
    for i in range(N_RANDOM):
        rows.append((f"random_{i}",) + random_row(rs))
    assert len(rows) <= 64
    return rows


def test_the_transitions_equal_the_contract_after_every_iteration():
    """Fails on the parent: the library has no commu_forcing_pre_form."""
    from commu_amd._lib import call
    from commu_amd.generate import form_template
    rows = transition_rows()
    B = len(rows)
    NF, NS = call("commu_forcing_state_ints"), call("commu_form_state_ints")
    assert NS == FC.NS and NF == PC.NF
    # one table for all rows: every form packed behind the one before it (a row of garbage first, so that no base is 0)
    table, ctl = [[FC.row_word(5, 1, 7), 9, 9, 9]], []
    for _, setting, bars, _ in rows:
        words = [int(w) for w in form_template({"bars": bars})[:, 0]]
        ctl.append(FC.word(len(table), len(words)))
        table += [[w, 0, 0, 0] for w in words]
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
    d_state = torch.full((B, NS), 77, dtype=i32, device=DEV)          # (garbage: the reset writes every int)
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
    # the contract's side
    ref = [dict(s=list(fsm[b]), st=FC.initial_state(list(CTX)), seq=list(CTX), n=0) for b in range(B)]
    got = torch.cat([d_state, d_ftok[:, None]], 1).cpu().numpy()
    for b in range(B):
        assert got[b, :NS].tolist() == ref[b]["st"] and got[b, NS] == -1

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

    closed = 0
    for it in range(ITERS):
        call("commu_forcing_pre_form", p(d_fsm), p(d_seq), LD_SEQ, p(d_ctok), p(d_cpos), LD_CHORD, p(d_wrong), p(d_utable), 8,
             1 << 30, p(d_tok), p(d_active), p(d_keep), p(d_draw), p(d_uni), p(d_trace), ld_trace, None, *form, B, s)
        flags, token = [], np.zeros(B, dtype=np.int32)
        for b, (_, setting, _, script) in enumerate(rows):
            r = ref[b]
            f = FC.pre(r["s"], r["st"], r["seq"], setting["tok"], setting["pos"], 1 << 30, LD_SEQ, ctl[b], table)
            flags.append(f)
            if f[3]:
                token[b] = script[r["n"] % len(script)]
                r["n"] += 1
            else:
                token[b] = 600 + b                                   # (never read: the slot does not draw)
        compare("pre", it, flags)
        d_token.copy_(torch.from_numpy(token))
        call("commu_forcing_post_form", p(d_fsm), p(d_seq), LD_SEQ, p(d_cpos), LD_CHORD, p(d_wrong), p(d_draw), p(d_token), None,
             None, p(d_keep), 1 << 30, None, None, *form, B, s)
        for b, (_, setting, _, _) in enumerate(rows):
            r, (t, act, kp, dr, ft) = ref[b], flags[b]
            if dr or ft >= 0:
                FC.post(r["s"], r["st"], r["seq"], setting["pos"], ft if ft >= 0 else int(token[b]), LD_SEQ, ctl[b], table)
        compare("post", it)
    # the rows did what they were written for
    by_name = {rows[b][0]: ref[b] for b in range(B)}
    for name, w in FH.WALKS.items():
        want = w[4]
        have = by_name[name]["seq"][N0:]
        assert (have if want[-1] == EOS else have[:len(want)]) == want, name
    for off in (57, 58, 59, 60, 61, 62, 63, 64, 130):
        sq = by_name[f"group_at_offset_{off}"]["seq"]
        at = [i for i, t in enumerate(sq) if t == BAR]
        assert sq[at[0] + 1 + off:at[0] + 5 + off] == [441, 150, 63, 310] and sq[at[1] + 3:at[2]] == [441, 150, 63, 310], off
    at = [i for i, t in enumerate(by_name["a_65th_bar"]["seq"]) if t == BAR]
    assert len(at) >= 66 and by_name["a_65th_bar"]["st"][FC.BAR_AT:] == at[:64]
    for b in range(B):
        if rows[b][0].startswith("random"):
            words = [int(w) for w in form_template({"bars": rows[b][2]})[:, 0]]
            closed += sum(1 for i in range(min(len(FH.closed_bars(ref[b]["seq"])), len(words))) if FC.fields(words[i]))
    print("random rows: closed replay bars:", closed)
    assert closed >= N_RANDOM


# ------------------------------------------------------------------------------------------------ 2. through the loop
GLEN = 128
FORM_A = "AABA"
FORM_R = {"bars": [None, {"of": 0, "copy": "rhythm"}, {"of": 1, "transpose": 3}, {"of": 0, "copy": "rhythm"}]}
FORMS = (FORM_A, None, FORM_R, None)


def loaded(z, model, B, form=None, **kw):
    """B slots of the fixture's request: grammar on, notes steered in, exactly two notes a bar (the density keeps the bars
    short), log-probabilities recorded; form: set_form's value."""
    from commu_amd.generate import ForcedDecoder, density_word
    prompts, glen = kw.pop("prompts", None), kw.pop("glen", GLEN)
    dec = ForcedDecoder(model, B, glen, 4146, 0.95, 32, **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES))
    dec.set_density(density_word(2, 2))
    if form is not None:
        dec.set_form(form)
    HG.reload(z, dec, prompts)
    return dec


fixture_model = HG.fixture_model


def drawn_mask(seq, lp):
    return [not np.isnan(x) for x in np.asarray(lp)[:len(seq), 0]]


def replay_bars(seq, form, start):
    """The closed replay bars of seq under the form: [(bar, source)]."""
    from commu_amd.generate import form_row_fields, form_template
    rows = form_template(form)
    cb = FH.closed_bars(seq)
    return [(i, form_row_fields(rows[i, 0])[0]) for i in range(min(len(cb), len(rows)))
            if form_row_fields(rows[i, 0]) is not None and cb[i][0] >= start]


def check_on_slot(z, seq, lp, form, start=None):
    from commu_amd.generate import form_violation
    from commu_amd.midi_generator.midi_inferrer import parse_events
    n_ctx = 1 + len(z["encoded_meta"])
    start = n_ctx if start is None else start
    assert seq is not None and parse_events(seq, n_ctx) is None, seq
    drawn = drawn_mask(seq, lp)
    assert form_violation(seq, start, form, drawn) is None, (form, seq)
    assert FC.form_violation(seq, start, FH.rows_of_form(form), drawn) is None
    # non-vacuity: at least 3 BARs, a closed replay bar whose source holds at least 2 note groups
    cb = FH.closed_bars(seq)
    rb = replay_bars(seq, form, start)
    assert seq.count(BAR) >= 3 and rb, seq
    assert any(len(FH.groups_of(seq, *cb[j])) >= 2 for _, j in rb), seq
    # every token of a free bar the loop wrote that is not forced has a number: at least the notes of a free bar
    free = [i for i in range(len(cb)) if cb[i][0] >= start and i not in dict(rb)]
    for i in free:
        lo, hi = cb[i]
        for g in range(lo + 1, hi - 3):
            if FC.is_group(seq, g) and g + 3 < hi:
                assert all(drawn[g + 1:g + 4]), (i, g, seq)         # (a position may be forced: a chord's)


def test_form_slots_through_the_loop(fixture_model):
    """Fails on the parent: ForcedDecoder has no set_form."""
    from commu_amd.generate import form_violation
    z, model = fixture_model
    B = 4
    start = 1 + len(z["encoded_meta"])
    plain = loaded(z, model, B)
    assert plain.form_ctl is None and plain.form_table is None and plain.form_state is None and plain.form_tok is None
    s0, f0, l0 = run(plain)
    free, free_lp = plain.sequences()[0], plain.logprobs()
    res = []
    for mode in ("graph", "eager", "separate"):
        dec = loaded(z, model, B, form=list(FORMS))
        assert dec.form_ctl.tolist() == [FC.word(0, 4), -1, FC.word(4, 4), -1]
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
    for b in range(B):
        if FORMS[b] is not None:
            check_on_slot(z, seqs[b], lps[b], FORMS[b])
        else:          # (the whole record: F_NDRAW included)
            assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
    # a replay token consumes no variate: the form slots drew fewer
    ndraw = fg[:, PC.F_NDRAW].tolist()
    print("variates consumed per slot:", ndraw, "; without the rule:", f0[:, PC.F_NDRAW].tolist())
    # teeth: the same run without the rule violates the form
    for b in (0, 2):
        assert free[b] is not None and form_violation(free[b], start, FORMS[b], drawn_mask(free[b], free_lp[b])) is not None
        assert not torch.equal(sg[b], s0[b])


def test_a_decoder_that_never_enables_the_rule_runs_the_parents_launches(fixture_model):
    z, model = fixture_model
    ref = loaded(z, model, 4)
    assert ref.form_ctl is None
    s0, f0, l0 = run(ref)
    ref.set_form(None)
    ref.set_form([None, False, None, None])
    assert ref.form_ctl is None and ref.form_state is None and ref.graph is not None      # (nothing allocated or dropped)
    dec = loaded(z, model, 4, form=FORM_A)
    run(dec)
    dec.set_form(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.form_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


def test_a_primed_slot_replays_the_bars_of_its_prompt(fixture_model):
    """The prompt is the first two bars of a sequence the loop wrote; under [null, null, 0, 1] bars 2 and 3, which the loop
    opens itself, replay the prompt's bars."""
    z, model = fixture_model
    n_ctx = 1 + len(z["encoded_meta"])
    src = loaded(z, model, 2)
    run(src)
    own = src.sequences()[0][0]
    bars = [i for i, t in enumerate(own) if t == BAR]
    assert len(bars) >= 3, own
    prompt = own[n_ctx:bars[2]]                                   # bars 0 and 1 complete, the third BAR not yet written
    assert prompt.count(BAR) == 2
    form = {"bars": [None, None, 0, 1]}
    dec = loaded(z, model, 2, form=form, max_prompt=len(prompt), prompts=[prompt] * 2)
    st0 = dec.form_state.cpu()[0].tolist()
    assert st0[:8] == [0, 0, 0, 0, 0, -1, 0, 0] and st0[8:10] == bars[:2] and st0[10:] == [0] * 62      # (the prompt's bars)
    run(dec)
    seq, lp = dec.sequences()[0][0], dec.logprobs()[0]
    cut = n_ctx + len(prompt)
    assert seq[:cut] == own[:cut] and len(seq) > cut + 4, seq
    cb = FH.closed_bars(seq)
    assert len(cb) >= 4, seq
    assert FH.groups_of(seq, *cb[2]) == FH.groups_of(seq, *cb[0]) and len(FH.groups_of(seq, *cb[0])) >= 1
    assert FH.groups_of(seq, *cb[3]) == FH.groups_of(seq, *cb[1])
    check_on_slot(z, seq, lp, form, start=cut)
    assert int(dec.fsm.cpu()[0, PC.F_NBAR]) == seq.count(BAR)


def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, form=[None, FORM_A, None, None])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g, table = dec.graph, dec.form_table
    assert g is not None
    check_on_slot(z, dec.sequences()[0][1], dec.logprobs()[1], FORM_A)
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_form(None, rows=[1])
    dec.set_form(FORM_R, rows=[2])
    uni = HG.reload(z, dec)
    dec.rearm(3, uni[3], form=FORM_A)
    s, f, l = run(dec)
    assert dec.graph is g and dec.form_table is table and dec.form_table.data_ptr() == table.data_ptr()
    assert dec.form_ctl.tolist() == [-1, -1, FC.word(4, 4), FC.word(0, 4)]
    second, lps = dec.sequences()[0], dec.logprobs()
    check_on_slot(z, second[2], lps[2], FORM_R)
    check_on_slot(z, second[3], lps[3], FORM_A)
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], form=False)
    dec.set_form(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.form_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


# ------------------------------------------------------------------------------------------------ 3. the request pool
@pytest.mark.parametrize("primed", [False, True], ids=["commu_decode_arm", "commu_decode_arm_primed"])
def test_pool_requests_with_their_own_forms_equal_generate_stream_of_each_alone(primed):
    """Two requests with different forms (one under the grammar in rhythm mode, primed: its prompt cut from a sequence
    generated under the same controls; one without the grammar) and one without a form: each one's sequences equal
    generate_stream(slots=1) of the request alone -- the arm launch wrote each slot's word and reset its replay state."""
    import commu_amd.generate as G
    import pool_contract as PLC
    import pool_prime_contract as PP
    import test_pool_gpu as TP
    import test_pool_prime_gpu as TPP
    from commu_amd._lib import CommuHipError
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model = TP._model()
    reqs = PLC.four_requests(G)
    every = lambda seq, rep: seq is not None
    one = G.density_word(1, 1)
    form_r = {"bars": [None, {"of": 0, "copy": "rhythm"}, {"of": 0, "transpose": 5}, 2]}
    mine = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, logit_bias=None, density=one,
                               form=form_r)
    if primed:
        own = TPP._own_sequence(TPP._generator(model), mine, 6, grammar=True, density=one, form=form_r)
        mine = dataclasses.replace(mine, prompt=PP.prompt_of(own, len(PLC.META), 6))
    want = TPP._alone(TPP._generator(model), mine, grammar=True, density=one, form=form_r)
    second = dataclasses.replace(reqs[0], accept=every, grammar=False, form="AAAA")
    second_want = TPP._alone(TPP._generator(model), second, form="AAAA")
    third = dataclasses.replace(reqs[2], accept=every, grammar=False)
    third_want = TPP._alone(TPP._generator(model), third)
    gen = TPP._generator(model)
    res = gen.generate_pool([second, mine, third], slots=3, grammar=True, return_logprobs=True)
    TPP._same_results(res[1], want)
    TPP._same_results(res[0], second_want)
    assert res[2].sequences == third_want[0] and res[2].attempts_started == third_want[1]      # (token for token)
    assert gen.pool_stats["kernel"] == ("commu_decode_arm_primed" if primed else "commu_decode_arm")
    assert len(res[1].sequences) == 2
    cut = TPP.N_CTX + (6 if primed else 0)
    n_closed = 0
    for s, lp in zip(res[1].sequences, res[1].logprobs):
        assert parse_events(s, TPP.N_CTX) is None, s
        assert G.form_violation(s, cut, form_r, drawn_mask(s, lp)) is None, s
        n_closed += len(replay_bars(s, form_r, cut))
    for s, lp in zip(res[0].sequences, res[0].logprobs):
        assert G.form_violation(s, TPP.N_CTX, "AAAA", drawn_mask(s, lp)) is None, s
    print("closed replay bars of the rhythm request:", n_closed)
    # teeth: without form= the same request decodes something else
    free = TPP._alone(TPP._generator(model), dataclasses.replace(mine, form=None), grammar=True, density=one)
    assert free[0] != want[0]
    with pytest.raises(CommuHipError, match=r"request 0: form: bar 1: \"of\": 3 is not an earlier bar"):
        gen.generate_pool([dataclasses.replace(second, form={"bars": [None, 3]})], slots=1)
    with pytest.raises(CommuHipError, match=r"request 0: form: \"copy\": \"rhythm\" without the event grammar"):
        gen.generate_pool([dataclasses.replace(second, form=form_r)], slots=1)


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_generate_cli_form_end_to_end(golden_dir, tmp_path, monkeypatch):
    """generate.py --grammar --form AABA on the reference-written checkpoint, every sequence that could be drawn accepted
    (a random model rarely passes the validators): what it writes keeps the form; the same run without the flag does not."""
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

    got = go(["--form", "AABA"], "formed")
    free = go([], "free")
    start = 1 + len(got["encoded_meta"])
    assert len(got["sequences"]) >= 1 and len(free["sequences"]) >= 1
    for s in got["sequences"]:
        assert parse_events(s, start) is None, s
        assert form_violation(s, start, "AABA") is None and replay_bars(s, "AABA", start), s
    assert any(form_violation(s, start, "AABA") is not None for s in free["sequences"])
