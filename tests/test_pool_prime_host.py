"""Primed request pool, host side: the numpy restatement of the primed arm launch against hand-written cases, the
PoolRequest prompt field, the argument block's size, and the command line's requests file with prompt_tokens."""
import ctypes as C
import json

import numpy as np
import pytest

import pool_contract as PC
import pool_prime_contract as PP
from test_pool_host import GOOD, _args, _cli


def _tiny(klen0, length, Lmax=4, img_rows=3, trace=True, e_trace=True):
    """One layer, one head, two slots, one entry, two cache tensors of 2-byte rows; everything spelled out."""
    before = {
        "cache0": np.full((1, 2, 1, Lmax, 2), 0x7F, dtype=np.uint8), "cache1": np.full((1, 2, 1, Lmax, 2), 0x7F, dtype=np.uint8),
        "klen": np.array([-7, -7], dtype=np.int32), "state": np.full((2, PP.NF), -7, dtype=np.int32),
        "seq": np.full((2, 6), -7, dtype=np.int32), "chord_tok": np.full((2, 2), -7, dtype=np.int32),
        "chord_pos": np.full((2, 2), -7, dtype=np.int32), "wrong": np.full((2, 5), 9, dtype=np.uint8),
        "utable": np.full((2, 3), 9.0, dtype=np.float32), "seq_logp": np.full((2, 6, 2), 9.0, dtype=np.float32),
    }
    if trace:
        before["trace"] = np.full((2, 2), -7, dtype=np.int32)
    state = np.arange(PP.NF, dtype=np.int32)[None] + 100
    state[0, 0] = length
    store = {"e_klen0": np.array([klen0], dtype=np.int32), "e_state": state,
             "e_seq": np.array([[0, 11, 12, 13]], dtype=np.int32), "e_chord_tok": np.array([[5, 6]], dtype=np.int32),
             "e_chord_pos": np.array([[7, 8]], dtype=np.int32)}
    if e_trace:
        store["e_trace"] = np.array([[41, 42]], dtype=np.int32)
    images = [np.arange(img_rows * 2, dtype=np.uint8).reshape(1, 1, 1, img_rows, 2) + 1,
              np.arange(img_rows * 2, dtype=np.uint8).reshape(1, 1, 1, img_rows, 2) + 101]
    return before, store, images


def test_restatement_on_a_linear_cache_by_hand():
    """klen0 2, record length 3, job (1, 0): rows 0 and 1 of slot 1 are the image's, rows 2 and 3 and slot 0 keep every
    byte; klen 2; three words of seq, the fourth and later untouched; the trace is the entry's; wrong 0; seq_logp NaN."""
    before, store, images = _tiny(2, 3)
    exp = PP.arm_primed_expected(before, store, images, [(1, 0)], [[0.1, 0.2, 0.3]], 2, 1, 4, 3, 4)
    assert exp["cache0"][0, 1, 0].tolist() == [[1, 2], [3, 4], [0x7F, 0x7F], [0x7F, 0x7F]]
    assert exp["cache1"][0, 1, 0].tolist() == [[101, 102], [103, 104], [0x7F, 0x7F], [0x7F, 0x7F]]
    assert (exp["cache0"][0, 0] == 0x7F).all() and (exp["cache1"][0, 0] == 0x7F).all()
    assert exp["klen"].tolist() == [-7, 2]
    assert exp["state"][1].tolist() == [3] + list(range(101, 100 + PP.NF)) and (exp["state"][0] == -7).all()
    assert exp["seq"].tolist() == [[-7] * 6, [0, 11, 12, -7, -7, -7]]
    assert exp["chord_tok"][1].tolist() == [5, 6] and exp["chord_pos"][1].tolist() == [7, 8]
    assert exp["trace"].tolist() == [[-7, -7], [41, 42]]
    assert not exp["wrong"][1].any() and (exp["wrong"][0] == 9).all()
    assert exp["utable"][1].tolist() == pytest.approx([0.1, 0.2, 0.3]) and (exp["utable"][0] == 9).all()
    assert np.isnan(exp["seq_logp"][1]).all() and (exp["seq_logp"][0] == 9).all()


def test_restatement_clamps_skips_and_zero_fills_by_hand():
    """klen0 above the image clamps to its 3 rows (klen 3); with grid_rows 2 to 2; a negative klen0 copies nothing (klen 0);
    a record length beyond ld_head copies ld_head words, a negative one none; jobs outside the ranges change nothing; a
    store without a trace twin zero-fills the slot's trace."""
    before, store, images = _tiny(9, 50, e_trace=False)
    exp = PP.arm_primed_expected(before, store, images, [(0, 0)], [[0, 0, 0]], 2, 1, 4, 3, 4)
    assert exp["klen"][0] == 3 and exp["cache0"][0, 0, 0].tolist() == [[1, 2], [3, 4], [5, 6], [0x7F, 0x7F]]
    assert exp["seq"][0].tolist() == [0, 11, 12, 13, -7, -7] and exp["trace"][0].tolist() == [0, 0]
    exp = PP.arm_primed_expected(before, store, images, [(0, 0)], [[0, 0, 0]], 2, 1, 4, 3, 4, grid_rows=2)
    assert exp["klen"][0] == 2 and exp["cache0"][0, 0, 0].tolist() == [[1, 2], [3, 4], [0x7F, 0x7F], [0x7F, 0x7F]]
    before, store, images = _tiny(-4, -1)
    exp = PP.arm_primed_expected(before, store, images, [(0, 0)], [[0, 0, 0]], 2, 1, 4, 3, 4)
    assert exp["klen"][0] == 0 and (exp["cache0"] == 0x7F).all() and (exp["seq"] == -7).all()
    exp = PP.arm_primed_expected(before, store, images, [(2, 0), (0, 1), (-1, 0)], [[0] * 3] * 3, 2, 1, 4, 3, 4)
    assert all(PC.same_bits(exp[k], before[k]) for k in before)


def test_restatement_on_a_ring_by_hand():
    """A ring of 3 rows whose image has the ring's 3 rows: klen0 7 copies the 3 physical rows and klen is 7, the position
    count; klen0 2 copies 2 rows and klen is 2."""
    before, store, images = _tiny(7, 2, Lmax=3)
    exp = PP.arm_primed_expected(before, store, images, [(1, 0)], [[0, 0, 0]], 2, 1, 3, 3, 4, ring=True)
    assert exp["klen"][1] == 7 and exp["cache1"][0, 1, 0].tolist() == [[101, 102], [103, 104], [105, 106]]
    before, store, images = _tiny(2, 2, Lmax=3)
    exp = PP.arm_primed_expected(before, store, images, [(1, 0)], [[0, 0, 0]], 2, 1, 3, 3, 4, ring=True)
    assert exp["klen"][1] == 2 and exp["cache1"][0, 1, 0].tolist() == [[101, 102], [103, 104], [0x7F, 0x7F]]


WORDS = ["order_ctl", "voice_ctl", "density_ctl", "interval_ctl", "onset_ctl", "guide_ctl", "art_ctl", "form_ctl"]


def _tiny_form(length):
    """_tiny with a sequence head of 8 words that holds Bars (token 2) at 1, 3, 6 and 7, the eight per-slot rule words with
    their twins (entry values 31 .. 38), the form state rows and the replay tokens."""
    import form_contract as FC
    before, store, images = _tiny(2, length)
    before["seq"] = np.full((2, 10), -7, dtype=np.int32)
    store["e_seq"] = np.array([[0, 2, 11, 2, 12, 13, 2, 2]], dtype=np.int32)
    for i, name in enumerate(WORDS):
        before[name] = np.full(2, -7, dtype=np.int32)
        store[PC.OPTIONAL[name][0]] = np.array([31 + i], dtype=np.int32)
    before["form_state"] = np.full((2, FC.NS), -7, dtype=np.int32)
    before["form_tok"] = np.full(2, -7, dtype=np.int32)
    return before, store, images


def _form_row(bars):
    """A form state row by hand: active, cursor, end, k, row 0, g -1, two reserved 0, then bar_at zero-padded to 64."""
    return [0, 0, 0, 0, 0, -1, 0, 0] + list(bars) + [0] * (64 - len(bars))


def test_restatement_of_the_rule_words_and_the_form_state_by_hand():
    """Length word 5 of a head with Bars at 1, 3, 6, 7: bar_at is [1, 3] in BOTH launches -- the primed one copies 5 words
    of the head and leaves the rest, the unprimed one all 8 --; every rule word is the entry's, form_tok -1, the idle slot
    keeps every sentinel.  A length word beyond ld_head records all four Bars, 0 and a negative one none; a length word
    of 2 stops before the Bar at 3."""
    for whole_head, seq in ((False, [0, 2, 11, 2, 12, -7, -7, -7, -7, -7]), (True, [0, 2, 11, 2, 12, 13, 2, 2, -7, -7])):
        before, store, images = _tiny_form(5)
        exp = PC.arm_restated(before, store, images, [(1, 0)], [[0.1, 0.2, 0.3]], 2, 1, 4, 3, 8, whole_head=whole_head)
        assert exp["seq"].tolist() == [[-7] * 10, seq]
        assert exp["form_state"][1].tolist() == _form_row([1, 3]) and (exp["form_state"][0] == -7).all()
        assert exp["form_tok"].tolist() == [-7, -1]
        assert [exp[name].tolist() for name in WORDS] == [[-7, 31 + i] for i in range(8)]
        assert exp["klen"].tolist() == [-7, 2] and exp["trace"].tolist() == [[-7, -7], [41, 42]]
    assert PC.same_bits(PP.arm_primed_expected(before, store, images, [(1, 0)], [[0.1, 0.2, 0.3]], 2, 1, 4, 3, 8)["seq"],
                        np.array([[-7] * 10, [0, 2, 11, 2, 12, -7, -7, -7, -7, -7]], dtype=np.int32))
    for length, bars in ((50, [1, 3, 6, 7]), (8, [1, 3, 6, 7]), (7, [1, 3, 6]), (2, [1]), (1, []), (0, []), (-3, [])):
        before, store, images = _tiny_form(length)
        for whole_head in (False, True):
            exp = PC.arm_restated(before, store, images, [(0, 0)], [[0, 0, 0]], 2, 1, 4, 3, 8, whole_head=whole_head)
            assert exp["form_state"][0].tolist() == _form_row(bars), (length, whole_head)
            assert exp["form_tok"].tolist() == [-1, -7] and (exp["form_state"][1] == -7).all()
    before, store, images = _tiny_form(5)
    exp = PC.arm_restated(before, store, images, [(2, 0), (0, 1)], [[0] * 3] * 2, 2, 1, 4, 3, 8, whole_head=True)
    assert all(PC.same_bits(exp[k], before[k]) for k in before)


def test_pool_request_prompt_defaults():
    import commu_amd.generate as G
    r = G.PoolRequest(PC.META, PC.data(), 1, 0.9, 8)
    assert r.prompt is None
    r2 = G.PoolRequest(PC.META, PC.data(), 1, 0.9, 8, prompt=[500, 501])
    assert list(r2.prompt) == [500, 501]
    prompts, longest = G.BatchedGenerator._pool_prompts([r, r2, G.PoolRequest(PC.META, PC.data(), 1, 0.9, 8, prompt=[])])
    assert prompts == [[], [500, 501], []] and longest == 2
    with pytest.raises(G.CommuHipError, match=r"request 1: prompt token 729 at index 2 is outside \[0, 729\)"):
        G.BatchedGenerator._pool_prompts([r, G.PoolRequest(PC.META, PC.data(), 1, 0.9, 8, prompt=[500, 501, 729])])
    with pytest.raises(G.CommuHipError, match=r"request 0: prompt token -1 at index 0"):
        G.BatchedGenerator._pool_prompts([G.PoolRequest(PC.META, PC.data(), 1, 0.9, 8, prompt=[-1])])


def test_primed_arm_args_abi():
    """commu_decode_arm_primed_args_bytes() is the ctypes struct's size; a wrong struct_bytes, a null block and more jobs
    than slots are refused with -22, 0 jobs launch nothing (every pointer of the block is null here)."""
    from commu_amd import _lib
    lib = _lib.load()
    assert lib.commu_decode_arm_primed_args_bytes() == C.sizeof(_lib.DecodeArmPrimedArgs)
    assert lib.commu_decode_arm_primed_chunk_rows() >= 1
    a = _lib.struct_args(_lib.DecodeArmPrimedArgs, B=4, Rcap=4, njobs=0)
    a.struct_bytes -= 8
    assert lib.commu_decode_arm_primed(C.byref(a), None) == -22
    assert lib.commu_decode_arm_primed(None, None) == -22
    a = _lib.struct_args(_lib.DecodeArmPrimedArgs, B=4, Rcap=4, njobs=5)
    assert lib.commu_decode_arm_primed(C.byref(a), None) == -22
    a.njobs = 0
    assert lib.commu_decode_arm_primed(C.byref(a), None) == 0
    a.njobs = 1          # (geometry and pointers missing)
    assert lib.commu_decode_arm_primed(C.byref(a), None) == -22


def test_cli_requests_file_with_prompt_tokens(tmp_path):
    """A request object may carry prompt_tokens (a list of integers, kept in its parsed dict; a request without the key
    has none); every malformed value is refused with the request's index; --prompt_tokens and --share_prompt beside
    --requests stay refused."""
    mod = _cli()
    good = [dict(GOOD, num_generate=3), dict(GOOD, num_generate=1, prompt_tokens=[500, 3, 432]),
            dict(GOOD, num_generate=2, prompt_tokens=[])]
    got = mod.check_requests(*_args(mod, tmp_path, good))
    assert "prompt_tokens" not in got[0] and got[1]["prompt_tokens"] == [500, 3, 432] and got[2]["prompt_tokens"] == []
    assert set(got[1]) == set(mod.REQUEST_KEYS) | {"prompt_tokens"}
    for bad in ("500", 500, [500, "3"], [1.5], [True], {"a": 1}, None):
        doc = [good[0], good[1], dict(GOOD, num_generate=1, prompt_tokens=bad)]
        with pytest.raises(ValueError, match="request 2: prompt_tokens: a JSON list of token ids"):
            mod.check_requests(*_args(mod, tmp_path, doc))
    with pytest.raises(ValueError, match="cannot be combined with --prompt_tokens"):
        mod.check_requests(*_args(mod, tmp_path, good, inputs=["--prompt_tokens", "p.json"]))
    with pytest.raises(ValueError, match="cannot be combined with --share_prompt"):
        mod.check_requests(*_args(mod, tmp_path, good, model=["--share_prompt"]))
    assert "prompt_tokens" in mod.parse_args()["input_args"].format_help()
    assert json.loads(json.dumps(got[1]))["prompt_tokens"] == [500, 3, 432]
