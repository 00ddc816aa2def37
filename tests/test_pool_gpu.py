"""Request pool on the GPU: the arm launch alone (commu_decode_arm) against its numpy statement, bit for bit, and
generate_pool against what generate_stream(slots=1) returns for each request alone."""
import numpy as np
import pytest
import torch

import form_contract as FC
import pool_contract as PC

pytestmark = pytest.mark.gpu

DEV = "cuda"
JOBS = [(0, 2), (3, 0), (4, 2)]          # one entry into two slots; slots 1 and 2 idle


def _launch_and_compare(c, jobs, seed):
    from commu_amd import ops
    uni = np.random.RandomState(seed).random_sample((max(len(jobs), 1), c.ld_u)).astype(np.float32)
    before = PC.snapshot(c)
    PC.stage_jobs(c, jobs, uni[:len(jobs)])
    ops.decode_arm(c.args, len(jobs))
    torch.cuda.synchronize()
    after, exp = PC.snapshot(c), PC.arm_expected(c, before, jobs, uni)
    for k in exp:
        assert PC.same_bits(after[k], exp[k]), k
    return before, after


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("DH", [32, 64])
def test_arm_launch_alone(kv, DH):
    """5 slots, 24 cache rows, a store of 3 entries with klen0 1, 11 and 16, jobs (0, 2), (3, 0), (4, 2); every slot array
    and cache byte holds a sentinel before.  After the launch: the armed slots' rows 0 .. klen0 - 1 are the entry's in
    every cache tensor, rows from klen0 on and the idle slots are what they were, every slot array row of an armed slot is
    the entry's, wrong is zero, seq_logp NaN, utable the staged variates.  Then: 0 jobs; a slot and an entry out of range
    (skipped, the third job done); every optional pointer null."""
    c = PC.arm_case(torch, kv, DH)
    before, after = _launch_and_compare(c, JOBS, 1)
    e_seq = c.store["e_seq"].cpu().numpy()
    for s, e in JOBS:          # (what arm_expected states, spelled out for the caches once more)
        n = c.klen0[e]
        for i in range(len(c.cache)):
            assert (after[f"cache{i}"][:, s, :, n:] == PC.NAN_BYTE).all()
            assert not (after[f"cache{i}"][:, s, :, :n] == PC.NAN_BYTE).all()
        assert after["klen"][s] == n and not after["wrong"][s].any() and np.isnan(after["seq_logp"][s]).all()
        # the form state: the case plants Bars on both sides of the entry's length word (9 and 12 of 16 head words), so
        # bar_at holds at least two Bars and fewer than the head has; the whole head is copied all the same
        bars = [i for i in range(PC.CTX_ROWS) if e_seq[e, i] == PC.BAR]
        below = [i for i in bars if i < c.lens[e]]
        assert 2 <= len(below) < len(bars)
        assert after["form_state"][s, FC.BAR_AT:FC.BAR_AT + len(bars)].tolist() == below + [0] * (len(bars) - len(below))
        assert after["form_tok"][s] == -1 and PC.same_bits(after["seq"][s, :PC.CTX_ROWS], e_seq[e])
    for s in (1, 2):
        for k in after:
            assert PC.same_bits(after[k][:, s] if k.startswith("cache") else after[k][s],
                                before[k][:, s] if k.startswith("cache") else before[k][s]), (k, s)
    b0, a0 = _launch_and_compare(c, [], 2)
    assert all(PC.same_bits(b0[k], a0[k]) for k in b0)
    _launch_and_compare(c, [(7, 0), (1, 5), (2, 1), (-1, 1)], 3)
    bare = PC.arm_case(torch, kv, DH, optional=False, seed=5)
    _launch_and_compare(bare, JOBS, 4)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_arm_launch_on_a_wrapped_ring(kv):
    """window 16 (17 ring rows), context 11, a slot whose klen has run to 40: after the arm its rows 0 .. 10 are the
    entry's, rows 11 .. 16 what they were, and klen is 11."""
    c = PC.arm_case(torch, kv, 32, Lmax=17, klen0=(11, 11, 11))
    c.slot["klen"][3] = 40
    before, after = _launch_and_compare(c, [(3, 1)], 7)
    assert before["klen"][3] == 40 and after["klen"][3] == 11
    img = c.image[0].view(torch.uint8).cpu().numpy()
    assert PC.same_bits(after["cache0"][:, 3, :, :11], img[:, 1, :, :11])
    assert (after["cache0"][:, 3, :, 11:] == PC.NAN_BYTE).all()


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_arm_launch_with_a_trace_twin(kv):
    """commu_decode_arm honours e_trace as the primed launch does: with the twin the armed slots' trace rows are the
    entries', without it they are zero; the idle slots keep their sentinel."""
    c = PC.arm_case(torch, kv, 32, e_trace=True, seed=3)
    before, after = _launch_and_compare(c, JOBS, 5)
    e_trace = c.store["e_trace"].cpu().numpy()
    for s, e in JOBS:
        assert e_trace[e].any() and PC.same_bits(after["trace"][s], e_trace[e])
    assert PC.same_bits(after["trace"][[1, 2]], before["trace"][[1, 2]])
    zeroed = PC.arm_case(torch, kv, 32, seed=3)
    assert "e_trace" not in zeroed.store and zeroed.args.e_trace is None
    before, after = _launch_and_compare(zeroed, JOBS, 5)
    assert not after["trace"][[0, 3, 4]].any() and PC.same_bits(after["trace"][[1, 2]], before["trace"][[1, 2]])


def test_arm_refuses_the_primed_geometry():
    """On a good block of commu_decode_arm, ring = 1 and grid_rows = 3 each return -22 and launch nothing: every slot array
    and cache byte is what it was; afterwards the good block returns 0."""
    from commu_amd import _lib
    from commu_amd.ops import _s
    import ctypes as C
    lib = _lib.load()
    c = PC.arm_case(torch, "bf16", 32)
    PC.stage_jobs(c, JOBS, np.zeros((len(JOBS), c.ld_u), dtype=np.float32))
    before = PC.snapshot(c)
    c.args.njobs = len(JOBS)
    assert c.args.ring == 0 and c.args.grid_rows == 0
    c.args.ring = 1
    assert lib.commu_decode_arm(C.byref(c.args), _s()) == -22
    c.args.ring, c.args.grid_rows = 0, 3
    assert lib.commu_decode_arm(C.byref(c.args), _s()) == -22
    c.args.grid_rows = 0
    torch.cuda.synchronize()
    after = PC.snapshot(c)
    assert all(PC.same_bits(before[k], after[k]) for k in before)
    assert lib.commu_decode_arm(C.byref(c.args), _s()) == 0          # (the block itself was good)
    torch.cuda.synchronize()
    assert not PC.same_bits(PC.snapshot(c)["klen"], before["klen"])


# ---------------------------------------------------------------------------------------------- end to end
def _model():
    import test_decode_slots_gpu as DS
    model = DS._model(DS.NARROW, 41, eos_bias=3.5)
    with torch.no_grad():
        model.crit.out_layers[0].bias[2] = 2.0          # bars again: the chord progressions are consumed
    return model


def _generator(model, **kw):
    from commu_amd.generate import BatchedGenerator
    kw.setdefault("generation_length", 40)
    kw.setdefault("memory_length", 128)
    return BatchedGenerator(model, torch.device(DEV), **kw)


def _alone(gen, r):
    """generate_stream of the request alone with slots=1: the sequential loop."""
    out, started, lps = gen.generate_stream(r.encoded_meta, r.input_data, r.temperature, r.top_k, need=r.need,
                                            accept=r.accept, top_p=r.top_p, slots=1, seed=r.seed,
                                            max_attempts=r.max_attempts, return_logprobs=True, logit_bias=r.logit_bias)
    return out, started, lps


def _same_results(res, ref):
    assert res.sequences == ref[0]
    assert res.attempts_started == ref[1]
    assert len(res.logprobs) == len(ref[2])
    for a, b in zip(res.logprobs, ref[2]):
        assert PC.same_bits(a, b)


@pytest.fixture(scope="module")
def world():
    import commu_amd.generate as G
    model = _model()
    reqs = PC.four_requests(G)
    gen = _generator(model)
    ref = [_alone(gen, r) for r in reqs]
    return model, reqs, ref


@pytest.mark.parametrize("slots", [2, 5])
def test_pool_request_equals_generate_stream_of_that_request_alone(world, slots):
    """Four requests (last meta token, chords and num_measures, sampling triple, need 1 / 3 / 2 / 2, seed; one with a pitch
    range; each with a deterministic accept rule that rejects some attempts) in a pool of 2 and of 5 slots: every request
    gets, token for token, the sequences and the count of started attempts that generate_stream(slots=1) returns for it
    alone.  The run is not trivial: attempts were rejected, slots changed their request, a window armed two slots."""
    model, reqs, ref = world
    gen = _generator(model)
    seen = []
    res = gen.generate_pool(reqs, slots=slots, return_logprobs=True, on_result=lambda i, r: seen.append(i))
    assert sorted(seen) == [0, 1, 2, 3] and len(res) == 4
    for r, want in zip(res, ref):
        _same_results(r, want)
    assert any(len(r.sequences) for r in res) and len({len(s) for r in res for s in r.sequences}) > 1
    st = gen.pool_stats
    print(f"pool of {slots}: {st}; (sequences, attempts) per request {[(len(r.sequences), r.attempts_started) for r in res]}")
    assert st["rejected"] >= 1
    assert st["rearmed_other_request"] >= 2
    assert any(n >= 2 for n in st["arms"][1:])          # (beyond the first window, which arms every slot)
    assert st["admissions"] == 4


def test_pool_result_does_not_depend_on_the_neighbours(world):
    """The four requests in reversed order, and each one alone in a pool of 5: every request gets bit-identical sequences
    and log-probability pairs.  The claim is made where no slot reaches 512 keys: beyond that the split-key policy
    chooses the attention's summation order from the number of live rows, as it does for generate_stream today; nothing
    here reaches it (generation_length 40)."""
    model, reqs, ref = world
    gen = _generator(model)
    res = gen.generate_pool(reqs[::-1], slots=5, return_logprobs=True)[::-1]
    for r, want in zip(res, ref):
        _same_results(r, want)
    for q, want in zip(reqs, ref):
        (one,) = gen.generate_pool([q], slots=5, return_logprobs=True)
        _same_results(one, want)


@pytest.mark.parametrize("mode", ["fp8", "sliding"])
def test_pool_equals_generate_stream_with_fp8_and_with_a_sliding_window(world, mode):
    """kv_dtype="fp8", and sliding=True with a window of 32 and generation_length 60 (the rings wrap): the pool against
    generate_stream(slots=1) of the same generator settings."""
    model, reqs, _ = world
    kw = {"kv_dtype": "fp8"} if mode == "fp8" else {"sliding": True, "memory_length": 32, "generation_length": 60}
    ref = [_alone(_generator(model, **kw), r) for r in reqs]
    gen = _generator(model, **kw)
    res = gen.generate_pool(reqs, slots=3, return_logprobs=True)
    for r, want in zip(res, ref):
        _same_results(r, want)
    if mode == "sliding":
        assert max(len(s) for r in res for s in r.sequences) > 12 + 32


@pytest.mark.parametrize("shape, kv", [((2, 4, 128, 256), "bf16"), ((2, 4, 128, 256), "fp8"), ((2, 2, 128, 256), "bf16")],
                         ids=["d_head32_bf16", "d_head32_fp8", "d_head64_bf16"])
def test_pool_equals_generate_stream_on_the_small_models(shape, kv):
    """The two small models of the decode tests (d_head 32 and 64; no fused layer tail: the decode step is the chain of
    per-Linear launches, and the image scatter runs at d_head 32): the pool of 3 slots against generate_stream(slots=1)."""
    import commu_amd.generate as G
    import test_decode_slots_gpu as DS
    model = DS._model(shape, 3, eos_bias=3.5)
    with torch.no_grad():
        model.crit.out_layers[0].bias[2] = 2.0
    reqs = PC.four_requests(G)
    kw = {} if kv == "bf16" else {"kv_dtype": kv}
    ref = [_alone(_generator(model, **kw), r) for r in reqs]
    gen = _generator(model, **kw)
    res = gen.generate_pool(reqs, slots=3, return_logprobs=True)
    (dec,) = gen._decoders.values()
    assert dec.state.kv_dtype == kv and dec.state.cache_tensors()[0].shape[4] == shape[2] // shape[1]
    for r, want in zip(res, ref):
        _same_results(r, want)
    assert sum(len(r.sequences) for r in res) >= 3 and gen.pool_stats["rearmed_other_request"] >= 1


def test_pool_tables_and_per_request_switches(world):
    """One pool with the grammar, harmony and class tables: a request with grammar and harmony off draws what it draws in
    a pool that has only the class table; a request with the grammar on returns only well-formed sequences."""
    import commu_amd.generate as G
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model, reqs, _ = world
    cls = G.class_sampling(after={"velocity": {"temperature": 0.7, "top_k": 12}})
    every = lambda seq, rep: seq is not None
    off = G.PoolRequest(reqs[1].encoded_meta, reqs[1].input_data, 2, 0.95, 32, seed=9, accept=every, grammar=False,
                        harmony=False)
    on = G.PoolRequest(reqs[3].encoded_meta, reqs[3].input_data, 3, 0.95, 32, seed=4, accept=every, grammar=True,
                       harmony=False)
    both = G.PoolRequest(reqs[1].encoded_meta, reqs[1].input_data, 2, 0.95, 32, seed=6, accept=every)
    full = _generator(model).generate_pool([off, on, both], slots=4, grammar=True, harmony=True, class_sampling=cls)
    off2 = G.PoolRequest(reqs[1].encoded_meta, reqs[1].input_data, 2, 0.95, 32, seed=9, accept=every)
    plain = _generator(model).generate_pool([off2], slots=4, class_sampling=cls)
    assert full[0].sequences == plain[0].sequences and len(full[0].sequences) == 2
    n_ctx = 1 + len(PC.META)
    assert len(full[1].sequences) == 3 and len(full[2].sequences) == 2
    for s in full[1].sequences + full[2].sequences:
        assert parse_events(s, n_ctx) is None, s


def test_pool_refusals_allocate_nothing(world):
    import commu_amd.generate as G
    model, reqs, _ = world
    gen = _generator(model)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    R = lambda **kw: G.PoolRequest(**{**dict(encoded_meta=PC.META, input_data=PC.data(), need=1, temperature=0.9, top_k=8),
                                      **kw})
    cases = [
        (dict(requests=[R()], slots=0), "slots in 1 .. 256"),
        (dict(requests=[R()], slots=257), "slots in 1 .. 256"),
        (dict(requests=[]), "empty list"),
        (dict(requests=[R(need=0)]), "need >= 1"),
        (dict(requests=[R(), R(encoded_meta=PC.META[:-1])]), "one length for the pool"),
        (dict(requests=[R(grammar=True)]), "no grammar table"),
        (dict(requests=[R(harmony=True)]), "no harmony table"),
    ]
    for kw, msg in cases:
        with pytest.raises(G.CommuHipError, match=msg):
            gen.generate_pool(**kw)
    with pytest.raises(G.CommuHipError, match="shared_prompt"):
        _generator(model, shared_prompt=True).generate_pool([R()])
    model.parity_fp32 = True
    try:
        with pytest.raises(G.CommuHipError, match="parity"):
            gen.generate_pool([R()])
    finally:
        model.parity_fp32 = False
    with pytest.raises(G.CommuHipError, match="shorter than the context"):
        _generator(model, sliding=True, memory_length=8).generate_pool([R()])
    assert torch.cuda.memory_allocated() == before
    assert not gen._decoders


def test_one_iteration_graph_serves_the_whole_pool(world):
    """dec.graph is the same object before and after 20 arms (and the launch count of an arm is one: nothing is captured
    again)."""
    import commu_amd.generate as G
    model, reqs, _ = world
    gen = _generator(model)
    gen.generate_pool(reqs, slots=3)
    (dec,) = gen._decoders.values()
    g = dec.graph
    assert g is not None
    dec.pool_open(len(PC.META))
    for e, r in enumerate(reqs[:3]):
        dec.admit(e, r.encoded_meta, r.input_data, sampling=(r.temperature, r.top_k, r.top_p))
    for i in range(20):
        dec.arm([(i % 3, (i + 1) % 3, G.BatchedGenerator.attempt_uniforms(1, i, dec.ld_u))])
        dec.run_iterations(2)
    torch.cuda.synchronize()
    dec.state.check()
    assert dec.graph is g


def test_generate_cli_requests_file_equals_three_runs_of_one_request(golden_dir, tmp_path, monkeypatch):
    """generate.py --requests FILE.json on the reference-written checkpoint, three requests that differ in bpm, key,
    num_generate and sampling controls: sequences.json is {"requests": [...]} and each request's encoded_meta and
    sequences are what a run of its own with --decode_slots 1 writes.  Once with both validators (a random model rarely
    passes them), once with both validators accepting everything, so that sequences are compared."""
    import json
    import os
    import test_model_gpu as TM
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, InferenceTask
    z = TM.load(golden_dir, "g10_checkpoint.npz")
    cli = TM._load_script("generate")
    parsers = cli.parse_args()
    prog = "-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8)
    base = dict(bpm=70, audio_key="aminor", time_signature="4/4", pitch_range="mid_high", num_measures=8,
                inst="acoustic_piano", genre="newage", min_velocity=60, max_velocity=80, track_role="main_melody",
                rhythm="standard", chord_progression=prog + "-" + prog)
    reqs = [dict(base, num_generate=2, max_rounds=2),
            dict(base, bpm=120, audio_key="cmajor", num_generate=1, max_rounds=3, temperature=1.1, top_k=16),
            dict(base, bpm=90, num_generate=3, max_rounds=1, top_p=0.9, pitch_min=40, pitch_max=90)]
    (tmp_path / "requests.json").write_text(json.dumps(reqs))
    common = ["--checkpoint_dir", os.path.join(golden_dir, "g10_checkpoint.pt"), "--generation_length", "120", "--gpus", "1"]

    def run(argv, out):
        argv = common + ["--output_dir", str(tmp_path / out)] + argv
        margs, _ = parsers["model_args"].parse_known_args(argv)
        iargs, _ = parsers["input_args"].parse_known_args(argv)
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
        return json.load(open(tmp_path / out / "sequences.json"))

    def compare(tag):
        pool = run(["--requests", str(tmp_path / "requests.json"), "--decode_slots", "4"], f"pool_{tag}")
        assert list(pool) == ["requests"] and len(pool["requests"]) == 3
        counts = []
        for i, r in enumerate(reqs):
            argv = ["--decode_slots", "1"]
            for k, v in r.items():
                argv += ["--" + k, str(v)]
            one = run(argv, f"one_{tag}_{i}")
            got = pool["requests"][i]
            assert got["encoded_meta"] == one["encoded_meta"], i
            assert got["sequences"] == one["sequences"], i
            assert 1 <= got["attempts"] <= r["max_rounds"] * r["num_generate"]
            counts.append(len(got["sequences"]))
        return counts
    compare("validated")
    # every sequence that could be drawn is accepted: each request now returns sequences (it would not only if every one of
    # its max_rounds x num_generate attempts ended without a token to draw), and the comparison is about tokens
    monkeypatch.setattr(ForcingReport, "validate_teacher_forced_sequence", lambda self, seq: None)
    monkeypatch.setattr(InferenceTask, "validate_generated_sequence", lambda self, seq: True)
    assert all(n >= 1 for n in compare("accepted"))
