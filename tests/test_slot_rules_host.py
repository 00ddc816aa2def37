"""The table of per-slot rules (commu_amd.generate.SLOT_RULES) on the host: every rule of the table, the form included, is
reachable by its keyword at every entry point, its names follow from its stem, its request-scope refusal is the one the
entry points always raised, and what a rule implies -- in the setters, in rearm and in the tier a pool asks for -- follows
from the table.  No GPU."""
import dataclasses
import inspect

import pytest

import test_form_host as FH

KEYWORDS = ("note_order", "voices", "density", "interval", "onsets", "guide", "articulation", "form")
# one setting that switches the rule on, in the form a request gives it
ON = {"note_order": 3, "voices": 2, "density": 2 + 256 * 5, "interval": 7 + 256 * 7, "onsets": [[0, 64]],
      "guide": {"cells": 1, "bars": [[[60]]]}, "articulation": {"velocity": [40, 80]}, "form": "AA"}


def rules():
    from commu_amd.generate import SLOT_RULES
    return SLOT_RULES


def test_the_table_holds_every_rule_in_tier_order_with_the_form_last():
    from commu_amd.generate import FORM, SAMPLING_RULES
    assert tuple(r.kw for r in rules()) == KEYWORDS
    tiers = [r.tier for r in SAMPLING_RULES]
    assert tiers == sorted(tiers) and len(set(tiers)) == len(tiers) and min(tiers) > 0
    assert rules()[-1] is FORM and FORM.tier == -1 and FORM not in SAMPLING_RULES


@pytest.mark.parametrize("kw", KEYWORDS)
def test_every_entry_point_takes_the_rules_keyword(kw):
    from commu_amd.generate import BatchedGenerator, ForcedDecoder, PoolRequest, RULE_OF, _rule_values
    assert kw in RULE_OF and _rule_values({kw: 1})[kw] == 1
    # the public entry points spell the keyword out, default None
    for f in (BatchedGenerator.generate, BatchedGenerator.generate_stream):
        assert inspect.signature(f).parameters[kw].default is None, f.__name__
    fields = {f.name: f for f in dataclasses.fields(PoolRequest)}
    assert kw in fields and fields[kw].default is None
    # the plumbing takes the rules as keywords checked against the table
    for f in (ForcedDecoder.rearm, ForcedDecoder.admit, BatchedGenerator.decoder):
        params = inspect.signature(f).parameters
        assert kw in params or any(p.kind is p.VAR_KEYWORD for p in params.values()), f.__name__


def test_an_unknown_keyword_is_a_type_error_before_anything_happens():
    from commu_amd.generate import BatchedGenerator
    dec = FH.stub()
    with pytest.raises(TypeError, match="unexpected keyword argument 'tempo'"):
        dec.rearm(0, tempo=3)
    with pytest.raises(TypeError, match="unexpected keyword argument 'tempo'"):
        dec.admit(0, [0] * 11, None, tempo=3)
    with pytest.raises(TypeError, match="unexpected keyword argument 'tempo'"):
        BatchedGenerator.__new__(BatchedGenerator).decoder(4, 1.0, 8, 4, tempo=3)
    assert dec.graph == "captured" and all(getattr(dec, r.ctl) is None for r in rules())


@pytest.mark.parametrize("kw", KEYWORDS)
def test_the_names_follow_from_the_stem(kw):
    from commu_amd._lib import DecodeArmArgs, DecodeArmPrimedArgs
    from commu_amd.generate import ForcedDecoder, RULE_OF
    r = RULE_OF[kw]
    for struct in (DecodeArmArgs, DecodeArmPrimedArgs):
        names = {f[0] for f in struct._fields_}
        assert r.stem + "_ctl" in names and "e_" + r.stem in names, struct.__name__
    assert r.ctl == r.stem + "_ctl" and r.entry == "e_" + r.stem
    assert callable(getattr(ForcedDecoder, "set_" + kw)) and r.setter == "set_" + kw
    # the decoder that never enables the rule has nothing of it: the six attributes are the class's
    assert [getattr(ForcedDecoder, a) for a in (r.ctl, r.host, r.table, r.table_host, r.used, r.index)] == \
        [None, None, None, None, 0, None]


@pytest.mark.parametrize("kw", KEYWORDS)
def test_one_takes_a_single_setting_and_refuses_one_per_slot(kw):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import RULE_OF
    r = RULE_OF[kw]
    assert r.one(None) is None
    got = r.one(ON[kw])
    assert r.is_on(r.normalize(got, 1)[0])
    if kw in ("note_order", "voices", "density", "interval"):
        assert got == ON[kw] and r.one(False) is False
        with pytest.raises(CommuHipError, match=rf"^{kw}: one setting for the request expected, got shape \(2,\)$"):
            r.one([ON[kw], ON[kw]])
    elif kw == "onsets":
        # (a list is a template's bars: two bars are ONE template; a list of templates is refused by onset_rows itself)
        assert r.one(False) is None and r.one([[0], [64]]).shape == (2, 4)
        with pytest.raises(CommuHipError, match="^onsets: a list of bars, each a list of positions 0 .. 127, expected"):
            r.one([{"grid": 4}, None])
    else:
        assert r.one(False) is None
        with pytest.raises(CommuHipError, match=rf"^{kw}: one setting for the request expected, got a list of 2$"):
            r.one([ON[kw], None])


def test_the_implications_are_the_tables():
    from commu_amd.generate import RULE_OF, rule_closure
    assert {kw: RULE_OF[kw].implies for kw in KEYWORDS if RULE_OF[kw].implies} == {"voices": "note_order", "density": "voices"}
    assert rule_closure({"density"}) == {"density", "voices", "note_order"}
    assert rule_closure({"voices"}) == {"voices", "note_order"}
    assert rule_closure({"articulation"}) == {"articulation"}
    assert rule_closure({"interval", "form"}) == {"interval", "form"}
    assert rule_closure(()) == set()


def test_the_tier_of_a_pool_is_the_highest_its_requests_need():
    """The literals are what the hand-written cascade of generate_pool chose before the table: T_MEL = 7 for a pool whose
    only rule is an interval, T_DEN = 6 for a density, T_ART = 10 for an articulation; T_VOX = 5 and T_ORD = 4 for a voice
    cap and a note order alone, T_GDE = 9 and T_ONS = 8 for a guide and an onset template, T_CLS = 3 / T_NONE = 0 for a pool
    without a rule with and without a class table; the form asks for no tier."""
    from commu_amd.generate import pool_tier
    assert pool_tier({"interval"}) == 7
    assert pool_tier({"density"}) == 6
    assert pool_tier({"articulation"}) == 10
    assert pool_tier({"voices"}) == 5 and pool_tier({"note_order"}) == 4
    assert pool_tier({"guide"}) == 9 and pool_tier({"onsets"}) == 8
    assert pool_tier({"density", "interval"}) == 7 and pool_tier({"note_order", "guide"}, True) == 9
    assert pool_tier(set(), True) == 3 and pool_tier(set()) == 0
    assert pool_tier({"form"}) == 0 and pool_tier({"form"}, True) == 3


def test_rearm_sets_every_rule_in_the_tables_order_and_what_it_implies():
    from commu_amd.generate import ARTICULATION, DENSITY, FORM, GUIDE, INTERVAL, ONSETS, ORDER, VOICES
    dec = FH.stub()
    dec.rearm(1, density=ON["density"])                        # (the density alone: the voice word and the note order follow)
    assert dec.density_ctl.tolist() == [-1, ON["density"], -1, -1]
    assert dec.voice_ctl.tolist() == [-1, 0, -1, -1] and dec.order_ctl.tolist() == [-1, 0, -1, -1]
    assert dec.interval_ctl is None and dec.form_ctl is None
    dec.rearm(2, **ON)
    for r in (ORDER, VOICES, DENSITY, INTERVAL):
        assert getattr(dec, r.ctl).tolist()[2] == ON[r.kw], r.kw
    for r in (ONSETS, GUIDE, ARTICULATION, FORM):
        words = getattr(dec, r.ctl).tolist()
        assert words[2] != r.off and words[0] == words[3] == r.off, r.kw
    assert dec.resets == [(1, 1), (0, 4), (2, 1)]              # (each re-arm resets its slot; between them the form's first use)
    before = {r.kw: getattr(dec, r.ctl).tolist() for r in rules()}
    dec.rearm(2)                                               # (None: the slot keeps every word)
    assert {r.kw: getattr(dec, r.ctl).tolist() for r in rules()} == before
    dec.rearm(2, **{kw: False for kw in KEYWORDS})
    assert all(getattr(dec, r.ctl).tolist()[2] == r.off for r in rules())
    assert dec.density_ctl.tolist()[1] == ON["density"]        # (the other slots keep theirs)
