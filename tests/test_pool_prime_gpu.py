"""Primed request pool on the GPU: the primed arm launch alone (commu_decode_arm_primed) against its numpy restatement, bit
for bit, and generate_pool with per-request prompts against what generate_stream(prompt=, slots=1) returns for each
request alone."""
import dataclasses

import numpy as np
import pytest
import torch

import pool_contract as PC
import pool_prime_contract as PP

pytestmark = pytest.mark.gpu

DEV = "cuda"
JOBS = [(0, 2), (3, 0), (4, 2), (-1, 1)]          # one entry into two slots; slots 1 and 2 idle; one job skipped
N_CTX = 1 + len(PC.META)


def _launch_and_compare(c, jobs, seed):
    from commu_amd import ops
    uni = np.random.RandomState(seed).random_sample((max(len(jobs), 1), c.ld_u)).astype(np.float32)
    before = PC.snapshot(c)
    PC.stage_jobs(c, jobs, uni[:len(jobs)])
    ops.decode_arm_primed(c.args, len(jobs))
    torch.cuda.synchronize()
    after, exp = PC.snapshot(c), PP.expected(c, before, jobs, uni)
    for k in exp:
        assert PC.same_bits(after[k], exp[k]), k
    return before, after


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("DH", [32, 64])
def test_primed_arm_launch_alone(kv, DH):
    """5 slots of 200 cache rows, a store of 3 entries with images of 144 rows, jobs (0, 2), (3, 0), (4, 2) and one with slot
    -1; every cache byte holds NAN_BYTE and every slot array a sentinel before.  e_klen0 of the two armed entries runs
    over 1, C - 1, C, C + 1, 2 C + 1, 144 and 150 (clamps to 144), C the kernel's chunk rows; the records' length words over
    0, a middle value, ld_head and beyond it.  After each launch every cache tensor and slot array is the restatement's, bit
    for bit: rows < n the image's, rows >= n and slots 1 and 2 untouched, klen = n, record, seq[:e_len] and nothing of
    seq beyond, the trace copied, seq_logp NaN, wrong 0, variates, every optional control.  Then: no trace twin (zeros), and
    every optional pointer null."""
    from commu_amd import ops
    C = ops.decode_arm_primed_chunk_rows()
    assert 2 * C + 1 <= 144
    pairs = [(1, C - 1), (C, C + 1), (2 * C + 1, 144), (150, C)]          # (entry 0, entry 2)
    for i, (k0, k2) in enumerate(pairs):
        lens = [(0, 17, 48, 70)[i], 5, (33, 48, 1, 60)[i]]
        c = PP.prime_case(torch, kv, DH, klen0=(k0, 7, k2), lens=lens, seed=i)
        before, after = _launch_and_compare(c, JOBS, 10 + i)
        img = [t.view(torch.uint8).cpu().numpy() for t in c.image]
        for s, e in JOBS[:3]:          # (what the restatement states, spelled out once more)
            n = min(c.klen0[e], 144)
            m = min(lens[e], c.ld_head)
            for t in range(len(c.cache)):
                assert PC.same_bits(after[f"cache{t}"][:, s, :, :n], img[t][:, e, :, :n])
                assert (after[f"cache{t}"][:, s, :, n:] == PC.NAN_BYTE).all()
            assert after["klen"][s] == n and not after["wrong"][s].any() and np.isnan(after["seq_logp"][s]).all()
            assert PC.same_bits(after["seq"][s, :m], c.store["e_seq"][e, :m].cpu().numpy())
            assert PC.same_bits(after["seq"][s, m:], before["seq"][s, m:])
            assert PC.same_bits(after["trace"][s], c.store["e_trace"][e].cpu().numpy())
        for s in (1, 2):
            for k in after:
                assert PC.same_bits(after[k][:, s] if k.startswith("cache") else after[k][s],
                                    before[k][:, s] if k.startswith("cache") else before[k][s]), (k, s)
    b0, a0 = _launch_and_compare(c, [], 2)
    assert all(PC.same_bits(b0[k], a0[k]) for k in b0)
    _launch_and_compare(c, [(7, 0), (1, 5), (2, 1), (-1, 1)], 3)
    zeroed = PP.prime_case(torch, kv, DH, klen0=(C + 3, 7, 20), lens=[20, 5, 30], e_trace=False, seed=7)
    _, after = _launch_and_compare(zeroed, JOBS, 4)
    assert not after["trace"][[0, 3, 4]].any()
    bare = PP.prime_case(torch, kv, DH, klen0=(C + 3, 7, 144), lens=[20, 5, 30], optional=False, seed=5)
    _launch_and_compare(bare, JOBS, 5)
    bound = PP.prime_case(torch, kv, DH, klen0=(C + 3, 7, 144), lens=[20, 5, 30], grid_rows=C + 3, seed=6)
    _, after = _launch_and_compare(bound, JOBS, 6)          # (grid_rows is part of the clamp)
    assert after["klen"][[0, 3, 4]].tolist() == [C + 3, C + 3, C + 3]


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_primed_arm_launch_on_a_wrapped_ring(kv):
    """A ring of W = 24 rows whose store image has the ring's 24 rows: an entry with e_klen0 = 40 gets all 24 physical rows
    copied and klen = 40, the position count; one with e_klen0 = 11 gets 11 rows and klen = 11."""
    c = PP.prime_case(torch, kv, 32, klen0=(40, 11, 11), lens=[40, 12, 12], Lmax=24, img_rows=24, ring=True)
    c.slot["klen"][3] = 77
    before, after = _launch_and_compare(c, [(3, 0), (1, 1)], 7)
    img = [t.view(torch.uint8).cpu().numpy() for t in c.image]
    assert after["klen"][3] == 40 and after["klen"][1] == 11
    for t in range(len(c.cache)):
        assert PC.same_bits(after[f"cache{t}"][:, 3], img[t][:, 0])
        assert PC.same_bits(after[f"cache{t}"][:, 1, :, :11], img[t][:, 1, :, :11])
        assert (after[f"cache{t}"][:, 1, :, 11:] == PC.NAN_BYTE).all()


def test_primed_arm_malformed_arguments():
    """A wrong struct_bytes, njobs > B, and an image with 16-byte rows that is not 16-byte aligned return -22 and launch
    nothing: every slot array and cache byte is what it was."""
    from commu_amd import _lib
    from commu_amd.ops import _s
    import ctypes as C
    lib = _lib.load()
    c = PP.prime_case(torch, "bf16", 32, klen0=(5, 7, 9), lens=[5, 5, 5])
    PC.stage_jobs(c, JOBS, np.zeros((len(JOBS), c.ld_u), dtype=np.float32))
    before = PC.snapshot(c)
    good = c.args.struct_bytes
    c.args.njobs = 3
    c.args.struct_bytes = good + 8
    assert lib.commu_decode_arm_primed(C.byref(c.args), _s()) == -22
    c.args.struct_bytes = good
    c.args.njobs = c.B + 1
    assert lib.commu_decode_arm_primed(C.byref(c.args), _s()) == -22
    c.args.njobs = 3
    keep = c.args.image[1]
    c.args.image[1] = keep + 8
    assert lib.commu_decode_arm_primed(C.byref(c.args), _s()) == -22
    c.args.image[1] = keep
    c.args.ring = 1          # (a ring's image cannot have more rows than the ring)
    c.args.Lmax, lmax = 100, c.args.Lmax
    assert lib.commu_decode_arm_primed(C.byref(c.args), _s()) == -22
    c.args.Lmax, c.args.ring = lmax, 0
    torch.cuda.synchronize()
    after = PC.snapshot(c)
    assert all(PC.same_bits(before[k], after[k]) for k in before)
    assert lib.commu_decode_arm_primed(C.byref(c.args), _s()) == 0          # (the block itself was good)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- end to end
def _generator(model, **kw):
    import test_pool_gpu as TP
    return TP._generator(model, **kw)


def _alone(gen, r, **kw):
    """generate_stream of the request alone with slots=1 and its prompt: the sequential loop."""
    return gen.generate_stream(r.encoded_meta, r.input_data, r.temperature, r.top_k, need=r.need, accept=r.accept,
                               top_p=r.top_p, slots=1, seed=r.seed, max_attempts=r.max_attempts, return_logprobs=True,
                               logit_bias=r.logit_bias, prompt=list(r.prompt) if r.prompt else None, **kw)


def _same_results(res, ref):
    assert res.sequences == ref[0]
    assert res.attempts_started == ref[1]
    assert len(res.logprobs) == len(ref[2])
    for a, b in zip(res.logprobs, ref[2]):
        assert PC.same_bits(a, b)


def _own_sequence(gen, r, at_least, **kw):
    """A sequence the model itself generates for the request (every attempt that could be drawn accepted): the longest of
    up to 8, with at least `at_least` tokens after the context and before EOS."""
    out, _ = gen.generate_stream(r.encoded_meta, r.input_data, r.temperature, r.top_k, need=8,
                                 accept=lambda seq, rep: seq is not None, top_p=r.top_p, slots=1, seed=100 + r.seed,
                                 max_attempts=8, logit_bias=r.logit_bias, **kw)
    best = max(out, key=len)
    assert len(best) - N_CTX - 1 >= at_least, [len(s) for s in out]
    return best


@pytest.fixture(scope="module")
def world():
    """test_pool_gpu.world's model and four requests; requests 1 and 3 get prompts of 9 and 4 tokens (the first tokens after
    the meta of a sequence the model generated for that request), request 2 gets prompt=[]; each request's answer alone."""
    import commu_amd.generate as G
    import test_pool_gpu as TP
    model = TP._model()
    reqs = PC.four_requests(G)
    gen = _generator(model)
    reqs[1] = dataclasses.replace(reqs[1], prompt=PP.prompt_of(_own_sequence(gen, reqs[1], 9), len(PC.META), 9))
    reqs[2] = dataclasses.replace(reqs[2], prompt=[])
    reqs[3] = dataclasses.replace(reqs[3], prompt=PP.prompt_of(_own_sequence(gen, reqs[3], 4), len(PC.META), 4))
    assert len(reqs[1].prompt) == 9 and len(reqs[3].prompt) == 4
    ref = [_alone(_generator(model), r) for r in reqs]
    return model, reqs, ref


@pytest.mark.parametrize("slots", [2, 5])
def test_primed_pool_request_equals_generate_stream_of_that_request_alone(world, slots):
    """Two of the four requests continue prompts of different lengths, one carries prompt=[], one none: in pools of 2 and
    of 5 slots every request gets, token for token (and log-probability pair for pair), the sequences and the count of
    started attempts that generate_stream(prompt=, slots=1) returns for it alone.  generation_length 40 keeps every klen far
    below LONG_KLEN.  The primed requests' sequences start with [0] + meta + prompt; the pool launched the primed kernel."""
    model, reqs, ref = world
    gen = _generator(model)
    res = gen.generate_pool(reqs, slots=slots, return_logprobs=True)
    for r, want in zip(res, ref):
        _same_results(r, want)
    for i in (1, 3):
        head = [0] + list(reqs[i].encoded_meta) + list(reqs[i].prompt)
        assert all(s[:len(head)] == head for s in res[i].sequences)
    assert sum(len(res[i].sequences) for i in (1, 3)) >= 1
    st = gen.pool_stats
    print(f"primed pool of {slots}: {st}; (sequences, attempts) {[(len(r.sequences), r.attempts_started) for r in res]}")
    assert st["kernel"] == "commu_decode_arm_primed" and st["admissions"] == 4
    (dec,) = gen._decoders.values()
    assert dec.max_prompt == 9 and st["image_rows"] == dec.n_ctx_max + dec.ld_fed == 16 + 16 + 18
    assert st["store_bytes"] == sum(t.numel() * t.element_size() for t in dec._pool["image"]) > 0
    assert st["klen0_max"] >= len(PC.META) + 8


def test_primed_pool_result_does_not_depend_on_the_neighbours(world):
    """The requests in reversed order, and each primed request alone in a pool of 5 (its prompt then the pool's longest):
    bit-identical sequences and log-probability pairs."""
    model, reqs, ref = world
    gen = _generator(model)
    res = gen.generate_pool(reqs[::-1], slots=5, return_logprobs=True)[::-1]
    for r, want in zip(res, ref):
        _same_results(r, want)
    for i in (1, 3):
        (one,) = _generator(model).generate_pool([reqs[i]], slots=5, return_logprobs=True)
        _same_results(one, ref[i])


@pytest.mark.parametrize("mode", ["fp8", "sliding"])
def test_primed_pool_with_fp8_and_with_a_sliding_window(world, mode):
    """kv_dtype="fp8", and sliding=True with a window of 16 (17 ring rows) and generation_length 60: context 11 + the replayed
    9-token prompt overrun the ring, so the store's image is a ring and wraps, and sequences grow past the window."""
    model, reqs, _ = world
    kw = {"kv_dtype": "fp8"} if mode == "fp8" else {"sliding": True, "memory_length": 16, "generation_length": 60}
    ref = [_alone(_generator(model, **kw), r) for r in reqs]
    gen = _generator(model, **kw)
    res = gen.generate_pool(reqs, slots=3, return_logprobs=True)
    for r, want in zip(res, ref):
        _same_results(r, want)
    assert gen.pool_stats["kernel"] == "commu_decode_arm_primed"
    if mode == "sliding":
        assert gen.pool_stats["image_rows"] == 17 and gen.pool_stats["klen0_max"] > 17
        assert max(len(s) for r in res for s in r.sequences) > 12 + 16
        assert max(len(s) for s in res[1].sequences) > 12 + 16


def test_primed_request_with_grammar_and_note_order(world):
    """One primed request with the event grammar and the note order on (its prompt cut from a sequence generated under the
    same controls), beside an unprimed one: its sequences are well formed (parse_events) and equal the single-request run."""
    import commu_amd.generate as G
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model, reqs, _ = world
    every = lambda seq, rep: seq is not None
    base = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, note_order=True, logit_bias=None)
    own = _own_sequence(_generator(model), base, 6, grammar=True, note_order=True)
    primed = dataclasses.replace(base, prompt=PP.prompt_of(own, len(PC.META), 6))
    want = _alone(_generator(model), primed, grammar=True, note_order=True)
    other = dataclasses.replace(reqs[0], accept=every, grammar=False)
    res = _generator(model).generate_pool([other, primed], slots=3, grammar=True, return_logprobs=True)
    _same_results(res[1], want)
    assert len(res[1].sequences) == 2
    for s in res[1].sequences:
        assert s[N_CTX:N_CTX + 6] == list(primed.prompt)
        assert parse_events(s, N_CTX) is None, s


def test_primed_pool_refusals_come_before_the_pool_is_opened(world):
    """A prompt whose second token breaks the rules in request 2 of 4 (the message names request 2, index 1 and the reason),
    a token >= 729, a prompt that overruns a linear cache (klen0, generation_length and Lmax in the message): each raised
    before pool_open -- the decoder's store is absent, or the object it was."""
    import commu_amd.generate as G
    model, reqs, _ = world
    gen = _generator(model)
    reasons = "|".join(G.ForcedDecoder.REPLAY_REASONS[k][:24] for k in (1, 2))
    bad = list(reqs)
    bad[2] = dataclasses.replace(reqs[2], prompt=[reqs[1].prompt[0], 200])          # (a chord token where a draw is expected)

    def pools():
        return [getattr(d, "_pool", None) for d in gen._decoders.values()]
    with pytest.raises(G.CommuHipError, match=rf"request 2: .*token 200 at index 1 of 2: ({reasons})") as e:
        gen.generate_pool(bad, slots=3)
    print(e.value)
    assert pools() == [None]
    with pytest.raises(G.CommuHipError, match=r"request 3: prompt token 729 at index 1 is outside \[0, 729\)"):
        gen.generate_pool(reqs[:3] + [dataclasses.replace(reqs[3], prompt=[500, 729])], slots=3)
    assert pools() == [None]
    gen.generate_pool(reqs, slots=3)          # (the generator serves the good list after the refusals)
    (dec,) = gen._decoders.values()
    store = dec._pool
    assert store is not None
    with pytest.raises(G.CommuHipError, match="request 2"):
        gen.generate_pool(bad, slots=3)
    assert dec._pool is store
    # a linear cache of 57 positions: the unprimed requests fit (12 + 40 + 1), request 1's replayed prompt does not
    small = _generator(model, memory_length=56)
    with pytest.raises(G.CommuHipError, match=r"request 1 starts with (\d+) cached positions .*generation_length 40 that needs "
                                              r"(\d+) positions and the decode memory has 57") as e:
        small.generate_pool(reqs, slots=3)
    print(e.value)
    assert [getattr(d, "_pool", None) for d in small._decoders.values()] == [None]


def test_one_graph_and_one_arm_launch_per_window(world, monkeypatch):
    """A pool that mixes primed and unprimed requests, twice on one generator: dec.graph is captured once, and every entry of
    pool_stats["arms"] is ONE launch of the primed entry point (the unprimed entries go through it too)."""
    from commu_amd import ops
    model, reqs, ref = world
    gen = _generator(model)
    calls = {"primed": 0, "plain": 0}
    real, real0 = ops.decode_arm_primed, ops.decode_arm
    monkeypatch.setattr(ops, "decode_arm_primed", lambda a, n: (calls.__setitem__("primed", calls["primed"] + 1), real(a, n))[1])
    monkeypatch.setattr(ops, "decode_arm", lambda a, n: (calls.__setitem__("plain", calls["plain"] + 1), real0(a, n))[1])
    gen.generate_pool(reqs, slots=3)
    (dec,) = gen._decoders.values()
    g = dec.graph
    assert g is not None
    n1 = len(gen.pool_stats["arms"])
    assert n1 >= 2 and calls == {"primed": n1, "plain": 0}
    res = gen.generate_pool(reqs[::-1], slots=3, return_logprobs=True)[::-1]
    assert dec.graph is g and len(gen._decoders) == 1
    assert calls == {"primed": n1 + len(gen.pool_stats["arms"]), "plain": 0}
    for r, want in zip(res, ref):
        _same_results(r, want)


def test_a_pool_without_prompts_launches_the_unprimed_kernel(world):
    """No prompt in the list (None and [] only): pool_stats names commu_decode_arm, the store has n_ctx_max image rows, the
    decoder is the one an unprimed pool always had (max_prompt 0, its own key)."""
    model, reqs, _ = world
    gen = _generator(model)
    plain = [dataclasses.replace(r, prompt=None if i % 2 else []) for i, r in enumerate(reqs)]
    gen.generate_pool(plain, slots=3)
    st = gen.pool_stats
    (key, dec), = gen._decoders.items()
    assert st["kernel"] == "commu_decode_arm" and st["image_rows"] == dec.n_ctx_max == 16
    assert dec.max_prompt == 0 and "primed" not in key
    assert all(t.shape[3] == 16 for t in dec._pool["image"]) and dec._pool["e_seq"].shape[1] == 16
    gen.generate_pool(reqs, slots=3)          # (a primed pool on the same generator: a decoder of its own)
    assert len(gen._decoders) == 2 and gen.pool_stats["kernel"] == "commu_decode_arm_primed"


def test_generate_cli_requests_file_with_prompt_tokens(golden_dir, tmp_path, monkeypatch):
    """generate.py --requests FILE.json where two of three requests carry prompt_tokens (the first tokens after the meta of
    a sequence a run of that request wrote): each request's sequences are what a run of its own with --prompt_tokens and
    --decode_slots 1 writes.  Both validators accept every sequence, so that sequences are compared."""
    import json
    import os
    import test_model_gpu as TM
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, InferenceTask
    monkeypatch.setattr(ForcingReport, "validate_teacher_forced_sequence", lambda self, seq: None)
    monkeypatch.setattr(InferenceTask, "validate_generated_sequence", lambda self, seq: True)
    z = TM.load(golden_dir, "g10_checkpoint.npz")
    cli = TM._load_script("generate")
    parsers = cli.parse_args()
    prog = "-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8)
    base = dict(bpm=70, audio_key="aminor", time_signature="4/4", pitch_range="mid_high", num_measures=8,
                inst="acoustic_piano", genre="newage", min_velocity=60, max_velocity=80, track_role="main_melody",
                rhythm="standard", chord_progression=prog + "-" + prog)
    reqs = [dict(base, num_generate=2, max_rounds=2),
            dict(base, bpm=120, audio_key="cmajor", num_generate=1, max_rounds=3, temperature=1.1, top_k=16),
            dict(base, bpm=90, num_generate=2, max_rounds=1, top_p=0.9)]
    common = ["--checkpoint_dir", os.path.join(golden_dir, "g10_checkpoint.pt"), "--generation_length", "60", "--gpus", "1"]

    def run(argv, out):
        argv = common + ["--output_dir", str(tmp_path / out)] + argv
        margs, _ = parsers["model_args"].parse_known_args(argv)
        iargs, _ = parsers["input_args"].parse_known_args(argv)
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
        return json.load(open(tmp_path / out / "sequences.json"))

    def single(r):
        argv = ["--decode_slots", "1"]
        for k, v in r.items():
            argv += ["--" + k, str(v)]
        return argv
    # prompts for requests 0 and 2: from a sequence an unprimed run of the request wrote
    for i, k in ((0, 7), (2, 3)):
        seed = run(single(reqs[i]), f"seed_{i}")
        n_cond = len(seed["encoded_meta"])
        body = max(seed["sequences"], key=len)[1 + n_cond:-1]
        assert len(body) >= k
        reqs[i]["prompt_tokens"] = body[:k]
    (tmp_path / "requests.json").write_text(json.dumps(reqs))
    pool = run(["--requests", str(tmp_path / "requests.json"), "--decode_slots", "4"], "pool")
    assert list(pool) == ["requests"] and len(pool["requests"]) == 3
    for i, r in enumerate(reqs):
        r = dict(r)
        argv = []
        if "prompt_tokens" in r:
            (tmp_path / f"prompt_{i}.json").write_text(json.dumps(r.pop("prompt_tokens")))
            argv = ["--prompt_tokens", str(tmp_path / f"prompt_{i}.json")]
        one = run(single(r) + argv, f"one_{i}")
        got = pool["requests"][i]
        assert got["encoded_meta"] == one["encoded_meta"], i
        assert got["sequences"] == one["sequences"] and len(got["sequences"]) >= 1, i
        if "prompt_tokens" in reqs[i]:
            n = 1 + len(got["encoded_meta"])
            assert all(s[n:n + len(reqs[i]["prompt_tokens"])] == reqs[i]["prompt_tokens"] for s in got["sequences"])
