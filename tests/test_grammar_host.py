"""The event grammar on the host (no GPU): the class map and the default table of the package against the plain restatement
(grammar_contract), every refusal of grammar_table, the two parsers against each other, and the rule set driven through
the reference loop's restatement (oracle/decode_ref.generate_sequence) on random logits: with the grammar every request is
well formed and none fails, without it they are not."""
import numpy as np
import pytest
import torch

import grammar_contract as GC

V = 729
NEG = float("-inf")


def test_class_map_at_every_range_edge():
    from commu_amd.midi_generator.midi_inferrer import token_class
    for t, c in GC.EDGE_IDS.items():
        assert token_class(t) == c == GC.token_class(t), t
    for t in range(-3, 800):
        assert token_class(t) == GC.token_class(t), t
    assert sorted(GC.EDGE_IDS) == [0, 1, 2, 3, 130, 131, 194, 195, 303, 304, 431, 432, 559, 560, 728]


def test_default_table_properties():
    from commu_amd.generate import event_grammar, grammar_table
    g = event_grammar()
    assert g.dtype == np.float32 and g.shape == (8, 768)
    assert np.array_equal(g, GC.default_table())
    assert set(np.unique(g).tolist()) == {NEG, 0.0}
    assert not g[7].any()                                           # row 7: the row of a slot that is off
    assert (g[:7, 195:304] == NEG).all()                            # a chord is never drawable
    for c in range(7):
        assert np.isfinite(g[c, 1:V]).any(), c                      # every class row keeps something
    boundary = np.zeros(V, bool)
    boundary[[1, 2]] = boundary[432:560] = True
    for c in (GC.OTHER, GC.BAR, GC.CHORD, GC.DURATION):
        assert ((g[c, 1:V] == 0) == boundary[1:]).all(), c
    for c, lo, hi in ((GC.POSITION, 131, 195), (GC.VELOCITY, 3, 131), (GC.PITCH, 304, 432)):
        allowed = np.flatnonzero(g[c, 1:V] == 0) + 1
        assert allowed.tolist() == list(range(lo, hi)), c
    assert np.array_equal(grammar_table(g), g) and np.array_equal(grammar_table(g[:7, :V]), g)


def test_grammar_table_refusals():
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import event_grammar, grammar_table
    g = event_grammar()
    for bad, what in ((g[:6], r"\(6, 768\)"), (np.zeros((9, 768), np.float32), r"\(9, 768\)"), (g[:, :728], r"\(8, 728\)"),
                      (g[0], r"\(768,\)"), (np.zeros((2, 8, 768), np.float32), r"\(2, 8, 768\)"), ("abc", "str")):
        with pytest.raises(CommuHipError, match=what):
            grammar_table(bad)
    nan = g.copy()
    nan[3, 17] = np.nan
    with pytest.raises(CommuHipError, match="row 3, entry 17 is nan"):
        grammar_table(nan)
    inf = g.copy()
    inf[5, 500] = np.inf
    with pytest.raises(CommuHipError, match="row 5, entry 500 is inf"):
        grammar_table(inf)
    empty = g.copy()
    empty[2, 1:V] = NEG
    empty[2, 0] = empty[2, V:] = 0.0                                # (ids 0 and >= 729 do not count)
    with pytest.raises(CommuHipError, match="row 2 bans all of ids 1 .. 728"):
        grammar_table(empty)
    seven = np.zeros((7, V), np.float32)
    seven[:, 10] = -2.5
    out = grammar_table(seven)
    assert out.shape == (8, 768) and not out[7].any() and (out[:7, 10] == -2.5).all() and not out[:, V:].any()
    junk = g.copy()
    junk[7] = 3.0                                                   # row 7 of a caller's table is replaced by zeros
    assert not grammar_table(junk)[7].any()
    assert np.array_equal(grammar_table(torch.from_numpy(g)), g)


CASES = [([600, 2, 432, 200, 432, 140, 60, 310, 440, 150, 3, 431, 2, 1], None),
         ([600, 432, 140, 60], None), ([600, 432, 140], None), ([600, 432], None), ([600], None),
         ([600, 432, 140, 60, 1], 4), ([600, 432, 1], 2), ([600, 1, 2], 2), ([600, 140], 1), ([600, 432, 60], 2),
         ([600, 432, 140, 310], 3), ([600, 432, 140, 60, 140], 4), ([600, 432, 432], 2), ([600, 200], 1),
         ([600, 2, 2, 432, 200, 310], 5), ([600, 2, 600], 2), ([600, 0], 1), ([600, 432, 140, 60, 310, 310], 5)]


def test_parse_events_and_its_restatement():
    from commu_amd.midi_generator.midi_inferrer import parse_events
    for seq, want in CASES:
        assert parse_events(seq, 1) == want and GC.parse_events(seq, 1) == want, seq
    g = np.random.RandomState(3)
    for _ in range(300):                                            # the two parsers agree on random short lists
        seq = [600] + g.choice([1, 2, 60, 140, 200, 310, 432, 500, 600], size=g.randint(0, 7)).tolist()
        assert parse_events(seq, 1) == GC.parse_events(seq, 1), seq


# ---- the rule set through the reference loop: 60 requests on random logits
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


def requests(n):
    out = []
    for i in range(n):
        nm = (4, 8, 5)[i % 3]
        bars = int(np.ceil(nm))
        kind = (i // 3) % 3
        if kind == 0:                       # one chord per bar, length_fit
            fit = int(nm // 4 * 4)
            tok, pos = [195 + (7 * j + i) % 109 for j in range(fit)], [432] * fit
        elif kind == 1:                     # mid-bar chords: two per bar (length_fit false)
            tok = [195 + (5 * j + i) % 109 for j in range(2 * bars)]
            pos = [432 if j % 2 == 0 else 432 + 64 for j in range(2 * bars)]
        else:                               # fewer chords than bars (length_fit false), none mid-bar
            tok, pos = [195 + (3 * j + i) % 109 for j in range(2)], [432, 432]
        out.append(dict(num_measures=float(nm), chord_token=tok, chord_position=pos,
                        temperature=0.0 if i % 5 == 0 else 0.95, seed=i))
    return out


def run_request(r, gram):
    from oracle import decode_ref as DR
    g = torch.Generator().manual_seed(1000 + r["seed"])
    table = None if gram is None else torch.from_numpy(gram)

    def step(tok, mems):
        lg = 3.0 * torch.randn(V, generator=g)
        if table is not None:
            lg = lg + table[GC.token_class(int(tok)), :V]
        return lg, mems
    u = np.random.RandomState(r["seed"]).random_sample(256)
    seq = [0] + META
    return DR.generate_sequence(step, seq, None, chord_token=r["chord_token"], chord_position=r["chord_position"],
                                num_measures=r["num_measures"], temperature=r["temperature"], top_k=32, uniforms=u,
                                max_iters=200)


def test_the_rule_set_through_the_reference_loop():
    from commu_amd.generate import event_grammar
    from commu_amd.midi_generator.midi_inferrer import parse_events
    reqs = requests(60)
    assert {r["num_measures"] for r in reqs} == {4.0, 8.0, 5.0}
    assert any(432 + 64 in r["chord_position"] for r in reqs) and any(r["temperature"] == 0 for r in reqs)
    fit = [len(r["chord_token"]) == int(r["num_measures"] // 4 * 4) for r in reqs]
    assert any(fit) and not all(fit)
    gram = event_grammar()
    start = 1 + len(META)
    malformed = failed = chords_seen = 0
    for r in reqs:
        seq = run_request(r, gram)
        assert seq is not None, r                                   # no Q12 with the grammar
        assert parse_events(seq, start) is None and GC.parse_events(seq, start) is None, (r, seq)
        chords_seen += sum(1 for t in seq if 195 <= t <= 303)
        free = run_request(r, None)
        failed += free is None
        malformed += free is not None and parse_events(free, start) is not None
    assert chords_seen > 0                                          # (the progressions were placed)
    print("without the grammar: malformed", malformed, "Q12", failed, "of", len(reqs))
    assert malformed >= 1
