"""The note-order constraint on the host: the restatement (tests/note_order_contract.py) and the package's checker
(midi_inferrer.note_order_violation) on hand-written edge cases, the rule through the reference loop's restatement
(oracle/decode_ref.generate_sequence) on the 60 random-logit requests of test_grammar_host, the refusals of note_order_ctl
and the struct mirrors."""
import ctypes as C

import numpy as np
import pytest
import torch

import grammar_contract as GC
import note_order_contract as NO
import test_grammar_host as GH

V = 729
CTX = [0] + GH.META          # the 12 context tokens every sequence starts with: no BAR, no POSITION
P = list(range(432, 560))


# ------------------------------------------------------------------------------------------------ 1. edge cases
# (name, tokens, F_LEN (None: len(tokens)), control word, the banned ids written out by hand)
EDGE_CASES = [
    ("empty", [], None, 0, []),
    ("context_only", CTX, None, 0, []),
    ("last_breaker_is_bar", CTX + [2, 440, 150, 60, 310, 2], None, 0, []),
    ("bar_then_velocity", CTX + [2, 440, 150, 60, 310, 2, 150], None, 1, []),
    ("p432_no_note", CTX + [2, 432, 150], None, 0, []),
    ("p432_one_note", CTX + [2, 432, 150, 60, 310], None, 0, [60]),
    ("p559", CTX + [2, 559, 150], None, 0, P[:127]),
    ("p559_one_note_cap1", CTX + [2, 559, 150, 70, 320], None, 1, [70] + P),
    ("repeated_position", CTX + [2, 440, 150, 60, 310, 440, 151, 64, 311, 440, 150], None, 0, [60, 64] + P[:8]),
    ("chord_group_in_the_run", CTX + [2, 440, 200, 440, 150, 60, 310, 440, 150], None, 0, [60] + P[:8]),
    ("pitches_3_and_130", CTX + [2, 433, 150, 3, 310, 433, 150, 130, 310, 433, 150], None, 0, [3, 130, 432]),
    # (the run starts right behind the last BAR / other position TOKEN, so the note group that follows that token -- the
    # last note of the position before -- lies inside it: its pitch is banned and it counts towards the cap)
    ("last_note_of_the_position_before", CTX + [2, 436, 150, 60, 310, 440, 150], None, 0, [60] + P[:8]),
    ("only_the_last_note_of_the_position_before", CTX + [2, 436, 150, 60, 310, 436, 150, 61, 310, 440, 150], None, 0,
     [61] + P[:8]),
    ("cap_counts_the_note_before", CTX + [2, 436, 150, 60, 310, 440, 150, 62, 310], None, 2, [60, 62] + P[:9]),
    ("bar_ends_the_run", CTX + [2, 440, 150, 60, 310, 2, 440, 150], None, 0, P[:8]),
    ("same_position_in_the_bar_before", CTX + [2, 440, 150, 60, 310, 2, 440, 150, 61, 310], None, 0, [61] + P[:8]),
    ("cap_reached_exactly", CTX + [2, 440, 150, 60, 310, 440, 150, 64, 310], None, 2, [60, 64] + P[:9]),
    ("cap_one_short", CTX + [2, 440, 150, 60, 310, 440, 150, 64, 310], None, 3, [60, 64] + P[:8]),
    ("doubled_note_counts_twice", CTX + [2, 440, 150, 60, 310, 440, 150, 60, 310], None, 2, [60] + P[:9]),
    ("off", CTX + [2, 440, 150, 60, 310], None, -1, []),
    ("f_len_beyond_the_row", CTX + [2, 440, 150, 60, 310, 440, 150, 61], 400, 0, [60, 61] + P[:8]),
    ("f_len_inside_the_row", CTX + [2, 440, 150, 60, 310, 445, 150, 61], 17, 0, [60] + P[:8]),
    ("negative_f_len", CTX + [2, 440, 150, 60, 310], -3, 0, []),
]


@pytest.mark.parametrize("name, tokens, length, ctl, want", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_bans_on_hand_written_cases(name, tokens, length, ctl, want):
    from commu_amd.midi_generator.midi_inferrer import note_order_bans
    n = len(tokens) if length is None else length
    assert NO.bans(tokens, n, ctl) == sorted(want)
    if ctl >= 0:                                # (the package's checker has no off switch: it is asked about a prefix)
        assert sorted(note_order_bans(tokens[:min(max(n, 0), len(tokens))], ctl)) == sorted(want)


def test_note_order_violation_on_hand_written_sequences():
    from commu_amd.midi_generator.midi_inferrer import note_order_violation
    start = len(CTX)
    ok = CTX + [2, 432, 199, 432, 150, 60, 310, 432, 150, 64, 310, 440, 150, 60, 310, 2, 432, 150, 60, 310, 1]
    assert note_order_violation(ok, start) is None and note_order_violation(ok, start, 2) is None
    assert note_order_violation(ok, start, 1) == start + 7           # the second `Position 432` of bar 1: it holds a note
    back = CTX + [2, 440, 150, 60, 310, 436, 150, 61, 310]
    assert note_order_violation(back, start) == start + 5 and note_order_violation(back, start + 6) is None
    doubled = CTX + [2, 440, 150, 60, 310, 440, 151, 60, 311]
    assert note_order_violation(doubled, start) == start + 7 and note_order_violation(doubled, 0, 5) == start + 7
    assert note_order_violation([], 0) is None and note_order_violation(CTX, 0, 1) is None
    assert note_order_violation(back, -4) == start + 5               # (a negative start is 0)
    with_cap = CTX + [2, 440, 150, 60, 310, 440, 150, 61, 310, 440, 150, 62, 310]
    assert note_order_violation(with_cap, start, 2) == start + 9 and note_order_violation(with_cap, start, 3) is None


# ------------------------------------------------------------------------------------------------ 2. the reference loop
def run_request(r, gram, ctl):
    """test_grammar_host.run_request with the rule applied in the step callback: the loop appends to `seq` in place, so the
    callback sees the sequence as it is when the logits it returns are drawn from (a Q5 re-draw reuses them: same bans)."""
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    table = torch.from_numpy(gram)
    seq = list(CTX)

    def step(tok, mems):
        lg = 3.0 * torch.randn(V, generator=g) + table[GC.token_class(int(tok)), :V]
        banned = NO.bans(seq, len(seq), ctl)
        if banned:
            lg[banned] = float("-inf")
        return lg, mems
    u = np.random.RandomState(r["seed"]).random_sample(256)
    return DR.generate_sequence(step, seq, None, chord_token=r["chord_token"], chord_position=r["chord_position"],
                                num_measures=r["num_measures"], temperature=r["temperature"], top_k=32, uniforms=u,
                                max_iters=200)


@pytest.fixture(scope="module")
def grammar():
    from commu_amd.generate import event_grammar
    return event_grammar()


def test_grammar_alone_breaks_the_note_order(grammar):
    from commu_amd.midi_generator.midi_inferrer import note_order_violation
    start = len(CTX)
    seqs = [run_request(r, grammar, -1) for r in GH.requests(60)]
    assert all(s is not None for s in seqs)
    broken = sum(note_order_violation(s, start) is not None for s in seqs)
    print("grammar only: requests that break note order:", broken, "of 60; mean length", np.mean([len(s) for s in seqs]))
    assert broken >= 48


@pytest.mark.parametrize("ctl", [0, 1, 2])
def test_the_rule_through_the_reference_loop(grammar, ctl):
    from commu_amd.midi_generator.midi_inferrer import note_order_violation, parse_events
    start = len(CTX)
    lengths = []
    for r in GH.requests(60):
        seq = run_request(r, grammar, ctl)
        assert seq is not None, r                                        # no Q12
        assert parse_events(seq, start) is None, (r, seq)
        assert note_order_violation(seq, start, ctl) is None, (r, seq)   # forced tokens included
        if ctl >= 1:                                                     # the cap, counted directly
            run, key = 0, None
            for t in seq[start:]:
                if t == 2 or (432 <= t <= 559 and t != key):
                    run, key = 0, (t if t != 2 else None)
                run += 3 <= t <= 130
                assert run <= ctl, (r, seq)
        lengths.append(len(seq))
    print("ctl", ctl, "mean length", np.mean(lengths))


# ------------------------------------------------------------------------------------------------ 3. host surface
def test_note_order_ctl_values_and_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import note_order_ctl
    assert note_order_ctl(None, 3).tolist() == [-1, -1, -1] and note_order_ctl(False, 2).tolist() == [-1, -1]
    assert note_order_ctl(True, 2).tolist() == [0, 0] and note_order_ctl(1, 2).tolist() == [1, 1]
    assert note_order_ctl(128, 1).tolist() == [128] and note_order_ctl(np.int64(7), 1).tolist() == [7]
    got = note_order_ctl([None, False, True, 0, -1, 1, 128, 2.0], 8)
    assert got.dtype == np.int32 and got.tolist() == [-1, -1, 0, 0, -1, 1, 128, 2]
    assert note_order_ctl(np.array([0, 3], dtype=np.int32), 2).tolist() == [0, 3]
    for bad, shown in ((129, "129"), (-2, "-2"), (1.5, "1.5"), (float("nan"), "nan"), (float("inf"), "inf"), ("on", "'on'")):
        with pytest.raises(CommuHipError, match=r"note_order: .*\[1, 128\].*got " + shown):
            note_order_ctl(bad, 4)
    with pytest.raises(CommuHipError, match=r"note_order\[2\]: .*got 200"):
        note_order_ctl([0, 1, 200, 0], 4)
    with pytest.raises(CommuHipError, match=r"note_order: 4 values expected \(one per sequence\), got 3"):
        note_order_ctl([0, 1, 2], 4)
    with pytest.raises(CommuHipError, match="one value per sequence expected"):
        note_order_ctl([[0, 1], [1, 0]], 2)


def test_struct_mirrors_carry_the_field_and_have_the_librarys_size():
    from commu_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SampleArgs) == lib.commu_sample_args_bytes()
    assert C.sizeof(_lib.DecodeLoopArgs) == lib.commu_decode_loop_args_bytes()
    for cls in (_lib.SampleArgs, _lib.DecodeLoopArgs):
        assert "order_ctl" in [n for n, _ in cls._fields_]
        assert _lib.struct_args(cls).order_ctl is None                   # null unless named


def stub(B=4):
    """test_class_sampling_host's decoder without a model or a device, with the two attributes this feature adds."""
    import test_class_sampling_host as CH
    dec = CH.stub(B)
    dec.order_ctl = dec._order_host = None
    return dec


def test_set_note_order_allocates_once_and_rewrites_in_place():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import CLASS_CTL_DTYPE
    dec = stub()
    dec.set_note_order(None)
    dec.set_note_order(False, rows=[1])
    assert dec.order_ctl is None and dec.cls_ctl is None and dec.graph == "captured"      # off on a fresh decoder: nothing
    with pytest.raises(CommuHipError, match="got 500"):
        dec.set_note_order(500)
    assert dec.order_ctl is None and dec.graph == "captured"                               # refused before anything changed
    dec.set_note_order(True, rows=[0, 2])
    assert dec.order_ctl.tolist() == [0, -1, 0, -1] and dec.graph is None and dec.rows_on
    assert dec.bias is not None and dec.gram is not None and dec.harm is not None
    assert not bool(dec.gram_on.any()) and not bool(dec.harm_on.any()) and not bool(dec.bias.any())
    rec = dec.cls_ctl.numpy().view(CLASS_CTL_DTYPE).reshape(4, 8)
    assert all(rec[b][c].tolist() == (np.float32(0.95), 32, 1.0, 0) for b in range(4) for c in range(8))     # base triples
    words = dec.order_ctl
    dec.graph = "captured again"
    dec.set_note_order([1, 128], rows=[1, 2])
    assert dec.order_ctl is words and words.tolist() == [0, 1, 128, -1] and dec.graph == "captured again"
    dec.set_note_order(None)
    assert dec.order_ctl is words and words.tolist() == [-1] * 4 and dec.graph == "captured again"
    dec.set_note_order(2)
    assert words.tolist() == [2] * 4
    dec.rearm(1, note_order=True)
    assert words.tolist() == [2, 0, 2, 2] and dec.graph == "captured again"
    dec.set_sampling(0.5, 8, 1.0, rows=[3])                                                  # the records follow the base triple
    rec = dec.cls_ctl.numpy().view(CLASS_CTL_DTYPE).reshape(4, 8)
    assert rec[3][2].tolist() == (0.5, 8, 1.0, 0) and rec[0][2].tolist() == (np.float32(0.95), 32, 1.0, 0)
