"""Request pool, host side (no GPU): the policy of generate_pool as PoolSchedule drives it, its answer against the
definition generate_stream gives, and the ABI of the arm launch as far as it can be checked without a launch."""
import ctypes as C
import random

import pytest


def _check(s, n_slots):
    """What must hold after every event."""
    for r in range(len(s.need)):
        assert s.in_flight[r] >= 0 and s.in_flight[r] + s.accepted[r] <= s.need[r], r          # the in-flight cap
        assert s.in_flight[r] == sum(1 for occ in s.slot if occ is not None and occ[0] == r)
        if s.cap[r] is not None:
            assert s.started[r] <= s.cap[r]
        if s.decided[r]:
            assert s.in_flight[r] == 0 and s.entry[r] is None
        elif s.started[r]:
            assert s.entry[r] is not None
    live = [s.entry[r] for r in range(len(s.need)) if s.entry[r] is not None]
    assert len(live) == len(set(live)) and sorted(live + s.free_entries) == list(range(n_slots))


def _assign(s, n_slots):
    """assign() with the checks of an assignment: FIFO service and consecutive attempt numbers."""
    before = list(s.started)
    free = sum(1 for occ in s.slot if occ is None)
    jobs = s.assign()
    nxt = list(before)
    for j in jobs:
        assert j.attempt == nxt[j.request]                     # attempts 0, 1, 2, ... per request
        nxt[j.request] += 1
        assert j.admit == (j.attempt == 0) and j.entry == s.entry[j.request]
    assert [j.request for j in jobs] == sorted(j.request for j in jobs)          # earlier requests first
    if len(jobs) < free:                                       # slots stay free only when nobody wants one
        assert not any(s.wants(r) for r in range(len(s.need)))
    for r in range(len(s.need)):                               # FIFO: nobody is served while an earlier request wants
        if s.wants(r):
            assert not any(j.request > r for j in jobs)
    _check(s, n_slots)
    # after an assignment every admitted, undecided request has an attempt in flight: `slots` entries are enough
    for r in range(len(s.need)):
        if s.entry[r] is not None:
            assert s.in_flight[r] >= 1, r
    return jobs


@pytest.mark.parametrize("n_slots", [2, 3, 4])
def test_schedule_scripted_events(n_slots):
    """Three requests of needs 1, 3 and 2 (request 1 bounded by max_attempts = 4) under scripted finish / accept events:
    the slot that finishes is chosen by a fixed rule that makes attempts finish OUT of attempt order (the highest slot
    first), and attempt a of request r is accepted by the table below."""
    from commu_amd.generate import PoolSchedule
    verdict = {0: [False, True], 1: [True, False, False, True, True], 2: [False, False, True, True]}
    s = PoolSchedule([1, 3, 2], [None, 4, None], n_slots)
    decided_at, freed, reused = {}, [], False
    step = 0
    _assign(s, n_slots)
    while s.busy():
        step += 1
        assert step < 50
        busy = [b for b, occ in enumerate(s.slot) if occ is not None]
        b = busy[-1] if step % 3 else busy[0]                  # out of order
        r, a = s.slot[b]
        entry = s.entry[r]
        ok = verdict[r][a]
        in_flight_before = s.in_flight[r]
        s.finish(b, ok, (r, a))
        _check(s, n_slots)
        for d in s.collect():
            assert s.in_flight[d] == 0                         # decided only when nothing of it is in flight
            decided_at[d] = step
            freed.append(entry if d == r else None)
        if r not in decided_at:
            assert in_flight_before - 1 == s.in_flight[r]
        wanted = s.wants(r)
        jobs = _assign(s, n_slots)
        if not ok and wanted:                                  # a rejected attempt leads to a further attempt
            assert any(j.request == r for j in jobs)
        reused = reused or any(j.admit and j.entry in freed for j in jobs)
    assert s.done() and sorted(decided_at) == [0, 1, 2]
    # answers in attempt order although the attempts finished out of order
    assert s.answer(0) == [(0, 1)] and s.started[0] == 2
    assert s.answer(1) == [(1, 0), (1, 3)] and s.started[1] == 4          # max_attempts exhausted: fewer than need
    assert s.answer(2) == [(2, 2), (2, 3)] and s.started[2] == 4
    if n_slots == 2:                                           # (with more slots all three are admitted at once)
        assert reused                                          # an entry freed on decision was taken again
    assert sorted(s.free_entries) == list(range(n_slots))


def test_answer_is_the_first_need_accepted_attempts_in_attempt_order():
    """200 seeded random accept patterns, needs, caps, slot counts and finishing orders: the pool's answer and its count of
    started attempts against the sequential definition -- try attempts 0, 1, 2, ... one after the other until `need` were
    accepted or max_attempts were tried."""
    from commu_amd.generate import PoolSchedule
    for seed in range(200):
        rng = random.Random(seed)
        n_req, n_slots = rng.randint(1, 6), rng.randint(1, 5)
        needs = [rng.randint(1, 4) for _ in range(n_req)]
        caps = [rng.choice([None, None, rng.randint(1, 8)]) for _ in range(n_req)]
        pattern = [[rng.random() < 0.6 for _ in range(64)] for _ in range(n_req)]
        s = PoolSchedule(needs, caps, n_slots)
        _assign(s, n_slots)
        decided = []
        while s.busy():
            b = rng.choice([b for b, occ in enumerate(s.slot) if occ is not None])
            r, a = s.slot[b]
            s.finish(b, pattern[r][a], a)
            decided += s.collect()
            _assign(s, n_slots)
        decided += s.collect()
        assert s.done() and sorted(decided) == list(range(n_req)), seed
        for r in range(n_req):
            got, a = [], 0
            while len(got) < needs[r] and (caps[r] is None or a < caps[r]):
                if pattern[r][a]:
                    got.append(a)
                a += 1
            assert s.answer(r) == got, (seed, r)
            assert s.started[r] == a, (seed, r)


def test_arm_args_abi():
    """commu_decode_arm_args_bytes() is the ctypes struct's size, and a wrong struct_bytes is refused with -22 before
    anything else is read (every other field of the block is zero / null here: nothing is launched)."""
    from commu_amd import _lib
    lib = _lib.load()
    assert lib.commu_decode_arm_args_bytes() == C.sizeof(_lib.DecodeArmArgs)
    a = _lib.struct_args(_lib.DecodeArmArgs)
    a.struct_bytes += 8
    assert lib.commu_decode_arm(C.byref(a), None) == -22
    assert lib.commu_decode_arm(None, None) == -22
    a = _lib.struct_args(_lib.DecodeArmArgs, njobs=3, B=2, Rcap=2)          # more jobs than slots
    assert lib.commu_decode_arm(C.byref(a), None) == -22
    a = _lib.struct_args(_lib.DecodeArmArgs, njobs=0, B=2, Rcap=2)          # 0 jobs: nothing to do, whatever else is null
    assert lib.commu_decode_arm(C.byref(a), None) == 0
    a = _lib.struct_args(_lib.DecodeArmArgs, njobs=1, B=2, Rcap=2, L=1, H=1, Lmax=4, ctx_rows=4, n_cache=2, nf=14, ld_seq=8,
                         ld_head=4, ld_chord=1, ld_wrong=729, ld_u=1)       # required pointers missing
    assert lib.commu_decode_arm(C.byref(a), None) == -22


def test_both_arm_launches_take_one_argument_block():
    """DecodeArmPrimedArgs is DecodeArmArgs under its own name: the same _fields_ and size, the library's two *_args_bytes()
    agree; ring and grid_rows sit directly behind image[4] and e_trace directly behind trace (offsets and names), the
    image's row count is ctx_rows, the form's four fields stay last; an instance of either class passes for either entry
    point, and 0 jobs return 0 before the geometry -- ring, grid_rows -- is looked at."""
    from commu_amd import _lib
    lib = _lib.load()
    A, P = _lib.DecodeArmArgs, _lib.DecodeArmPrimedArgs
    assert issubclass(P, A) and P.__name__ == "DecodeArmPrimedArgs"
    assert list(P._fields_) == list(A._fields_) and C.sizeof(P) == C.sizeof(A)
    assert lib.commu_decode_arm_args_bytes() == lib.commu_decode_arm_primed_args_bytes() == C.sizeof(A)
    names = [n for n, _ in A._fields_]
    i, t = names.index("image"), names.index("trace")
    assert names[i - 2:i + 4] == ["row_bytes", "cache", "image", "ring", "grid_rows", "klen"]
    assert names[t - 1:t + 3] == ["seq_logp", "trace", "e_trace", "ld_trace"]
    assert names[-4:] == ["form_ctl", "e_form", "form_state", "form_tok"]
    assert "ctx_rows" in names and "img_rows" not in names and len(names) == len(set(names))
    ptr = C.sizeof(C.c_void_p)
    assert A.ring.offset == A.image.offset + 4 * ptr and A.grid_rows.offset == A.ring.offset + 4
    assert A.klen.offset == A.ring.offset + 8 and A.e_trace.offset == A.trace.offset + ptr
    assert A.ld_trace.offset == A.e_trace.offset + ptr and C.sizeof(A) == A.form_tok.offset + ptr
    for cls in (A, P):
        a = _lib.struct_args(cls, njobs=0, B=2, Rcap=2, ring=1, grid_rows=3)
        assert a.e_trace is None and a.struct_bytes == C.sizeof(A)
        assert lib.commu_decode_arm(C.byref(a), None) == 0 and lib.commu_decode_arm_primed(C.byref(a), None) == 0
        a.struct_bytes += 8
        assert lib.commu_decode_arm(C.byref(a), None) == -22 and lib.commu_decode_arm_primed(C.byref(a), None) == -22


# ---------------------------------------------------------------------------------------------- command line
def _cli():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("commu_generate_cli_pool", os.path.join(root, "commu-code_amd", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GOOD = dict(bpm=70, audio_key="aminor", time_signature="4/4", pitch_range="mid_high", num_measures=8, inst="acoustic_piano",
            genre="newage", min_velocity=60, max_velocity=80, track_role="main_melody", rhythm="standard",
            chord_progression="-".join(["Am"] * 32 + ["E"] * 32))


def _args(mod, tmp_path, doc, model=(), inputs=(), raw=None):
    import json
    path = tmp_path / "requests.json"
    path.write_text(raw if raw is not None else json.dumps(doc))
    p = mod.parse_args()
    margs = p["model_args"].parse_known_args(list(model))[0]
    iargs = p["input_args"].parse_known_args(["--output_dir", str(tmp_path), "--requests", str(path)] + list(inputs))[0]
    return margs, iargs


def test_cli_requests(tmp_path):
    """--requests is listed by --help; check_requests() refuses, with its message, every combination and file the
    command line does not serve; a good file parses into the per-request argument dicts."""
    mod = _cli()
    assert "--requests FILE.json" in mod.parse_args()["input_args"].format_help()
    p = mod.parse_args()
    assert mod.check_requests(p["model_args"].parse_known_args([])[0],
                              p["input_args"].parse_known_args(["--output_dir", "x"])[0]) is None
    good = [dict(GOOD, num_generate=3), dict(GOOD, num_generate=1, top_k=8, temperature=1.1, top_p=0.9, seed=7, max_rounds=2,
                                             pitch_min=48, pitch_max=84, genre="cinematic")]
    got = mod.check_requests(*_args(mod, tmp_path, good))
    assert len(got) == 2 and all(set(g) == set(mod.REQUEST_KEYS) for g in got)
    assert got[0] == dict(GOOD, num_generate=3, top_k=32, temperature=0.95, top_p=1.0, seed=0, max_rounds=None,
                          pitch_min=None, pitch_max=None, logit_bias=None)
    assert got[1] == dict(GOOD, num_generate=1, top_k=8, temperature=1.1, top_p=0.9, seed=7, max_rounds=2, pitch_min=48,
                          pitch_max=84, logit_bias=None, genre="cinematic")
    refused = [
        (dict(inputs=["--bpm", "70"]), "single-request input argument --bpm"),
        (dict(inputs=["--num_generate", "3"]), "single-request input argument --num_generate"),
        (dict(inputs=["--temperature", "0.5"]), "single-request input argument --temperature"),
        (dict(inputs=["--pitch_min", "40"]), "single-request input argument --pitch_min"),
        (dict(inputs=["--prompt_tokens", "p.json"]), "cannot be combined with --prompt_tokens"),
        (dict(model=["--share_prompt"]), "cannot be combined with --share_prompt"),
        (dict(model=["--parity"]), "cannot be combined with --parity"),
        (dict(inputs=["--gpus", "2"]), "runs on one GPU"),
    ]
    for kw, msg in refused:
        with pytest.raises(ValueError, match=msg):
            mod.check_requests(*_args(mod, tmp_path, good, **kw))
    assert mod.check_requests(*_args(mod, tmp_path, good, inputs=["--gpus", "1"])) == got
    files = [
        (dict(doc={"requests": good}), "JSON list of request objects"),
        (dict(doc=[]), "JSON list of request objects"),
        (dict(doc=None, raw="[{"), "not JSON"),
        (dict(doc=[good[0], 5]), "request 1: an object"),
        (dict(doc=[good[0], dict(GOOD, num_generate=1, tempo=3)]), "request 1: unknown key 'tempo'"),
        (dict(doc=[good[0], good[1], dict(GOOD)]), "request 2: num_generate is missing"),
        (dict(doc=[dict(GOOD, num_generate=0)]), "request 0: num_generate: an integer >= 1"),
    ]
    for kw, msg in files:
        with pytest.raises(ValueError, match=msg):
            mod.check_requests(*_args(mod, tmp_path, kw.pop("doc"), **kw))
    margs, iargs = _args(mod, tmp_path, good)
    iargs.requests = str(tmp_path / "missing.json")
    with pytest.raises(ValueError, match="readable JSON file"):
        mod.check_requests(margs, iargs)
