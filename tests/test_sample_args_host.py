"""The two argument structs of the sampling stage on the host (the library loads without a GPU, as test_abi.py shows): the
ctypes mirrors have the library's sizeof, an empty batch is a no-op, and a struct of another size is refused before the
empty-batch early-out; and a struct that names a constraint tier without one of its prerequisites is refused by both entry
points before anything is launched."""
import ctypes as C

import pytest

STRUCTS = [("SampleArgs", "commu_sample_args_bytes", "commu_sample_topk", "nseq"),
           ("DecodeLoopArgs", "commu_decode_loop_args_bytes", "commu_decode_sample_post_pre", "B")]


@pytest.mark.parametrize("cls, sizer, entry, count", STRUCTS, ids=[s[0] for s in STRUCTS])
def test_struct_size_and_the_struct_bytes_check(cls, sizer, entry, count):
    from commu_amd import _lib
    from commu_amd._lib import CommuHipError, call, struct_args
    cls = getattr(_lib, cls)
    assert C.sizeof(cls) == call(sizer) > 0
    # An empty batch with the right size: 0, whatever else the struct holds.  The same empty batch from a caller compiled
    # against another layout: -22 -- only the struct_bytes check can say so, and only if it comes BEFORE the empty-batch
    # early-out (without the check, or with it behind the early-out, these calls return 0).  Nothing is launched either way.
    assert call(entry, C.byref(struct_args(cls, **{count: 0})), None) == 0
    for wrong in (0, C.sizeof(cls) - 4, C.sizeof(cls) + 8):
        a = struct_args(cls, **{count: 0})
        a.struct_bytes = wrong
        with pytest.raises(CommuHipError, match="-22"):
            call(entry, C.byref(a), None)
    # and with a batch of 4: refused as well (every other field is zero, so no check behind it would let this struct
    # through to a launch either)
    a = struct_args(cls, **{count: 4})
    a.struct_bytes = C.sizeof(cls) + 8
    with pytest.raises(CommuHipError, match="-22"):
        call(entry, C.byref(a), None)
    assert struct_args(cls).struct_bytes == C.sizeof(cls)


def test_load_refuses_a_library_whose_structs_differ(monkeypatch):
    """load() compares the mirrors with the library before it hands the library out."""
    from commu_amd import _lib
    _lib.load()
    fields = list(_lib.SampleArgs._fields_) + [("extra", C.c_int), ("extra2", C.c_int)]
    bigger = type("SampleArgs", (C.Structure,), {"_fields_": fields})
    monkeypatch.setattr(_lib, "SampleArgs", bigger)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.CommuHipError, match="SampleArgs"):
        _lib.load()
    assert _lib._lib is None


# ------------------------------------------------------------------------------------------------ the refusal ladder
# The constraints are strictly nested tiers: each needs every tier below it, and each entry point refuses (-22, before any
# launch) a struct that names a tier without what that tier reads.  The table is the header's contract (commu_hip.h: "the
# same refusal" in both structs), written out per tier; the pointers are made-up addresses that are never dereferenced,
# since no call below gets as far as a launch: every struct that is passed with a batch of 1 lacks exactly one prerequisite,
# and the complete struct is passed with an empty batch only.
V = 729
TIERS = ["harm", "cls", "order", "voice", "density", "interval", "onset", "guide", "art"]
# per tier: the fields it adds to a valid struct, then the rung below (fields whose absence refuses this tier's pointer)
ADDS = {"harm": dict(bias=1, ld_bias=V, gram=1, ld_gram=V, state=1, seq=1, harm=1, ld_harm=12, chord_tok=1),
        "cls": dict(cls_ctl=1), "order": dict(order_ctl=1), "voice": dict(voice_ctl=1), "density": dict(density_ctl=1),
        "interval": dict(interval_ctl=1), "onset": dict(onset_ctl=1, onset_table=1, onset_rows=1),
        "guide": dict(guide_ctl=1, guide_table=1, guide_rows=1), "art": dict(art_ctl=1, art_table=1, art_rows=1)}
BELOW = {"harm": ["gram", "bias"], "cls": ["harm"], "order": ["cls_ctl"], "voice": ["order_ctl"], "density": ["voice_ctl"],
         "interval": ["density_ctl"], "onset": ["interval_ctl"], "guide": ["onset_ctl"], "art": ["guide_ctl"]}
# what the tier's kernel reads beside the rung below: a null one refuses
READS = {"harm": ["chord_tok"], "cls": ["state", "seq", "bias", "gram", "chord_tok"], "onset": ["onset_table"],
         "guide": ["guide_table"], "art": ["art_table"]}
ROWS_MAX = {"onset": 4096, "guide": 65536, "art": 4096}
BASE = {"SampleArgs": dict(logits=1, token=1, ld=768, V=V, top_k=1, top_p=1.0, ld_seq=2, ld_chord=1),
        "DecodeLoopArgs": dict(logits=1, token=1, ld=768, V=V, top_k=1, top_p=1.0, ld_seq=2, ld_chord=1, ld_u=1, state=1,
                               seq=1, chord_tok=1, chord_pos=1, utable=1, tok=1, active=1, keep=1, draw=1, uni=1, wrong=1)}


def valid_at(cls_name, tier):
    """The fields of a struct that is valid at `tier`: every pointer a distinct made-up address, 16-byte aligned."""
    f = dict(BASE[cls_name])
    for t in TIERS[:TIERS.index(tier) + 1]:
        f.update(ADDS[t])
    ptrs = sorted(k for k, v in f.items() if v == 1 and not k.startswith(("ld", "top_")) and not k.endswith("_rows"))
    f.update({k: 0x10000 + 0x100 * i for i, k in enumerate(ptrs)})
    return f


def removals(tier):
    """(what, field changes): each takes exactly one prerequisite away from a struct that is valid at `tier`."""
    out = [("no " + k, {k: None}) for k in BELOW[tier] + READS.get(tier, [])]
    if tier in ROWS_MAX:
        out += [("no rows", {tier + "_rows": 0}), ("rows above the maximum", {tier + "_rows": ROWS_MAX[tier] + 1})]
    if tier != "harm":
        out.append(("cls_ctl off its 16-byte alignment", {"cls_ctl": "+4"}))
    out += [("ld_bias", {"ld_bias": V - 1}), ("ld_gram", {"ld_gram": V - 1}), ("ld_harm", {"ld_harm": 11}),
            ("ld_seq", {"ld_seq": 0}), ("ld_chord", {"ld_chord": 0})]
    return out


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("cls, sizer, entry, count", STRUCTS, ids=[s[0] for s in STRUCTS])
def test_a_tier_without_one_of_its_prerequisites_is_refused(cls, sizer, entry, count, tier):
    from commu_amd import _lib
    from commu_amd._lib import CommuHipError, call, struct_args
    fields = valid_at(cls, tier)
    cls = getattr(_lib, cls)
    assert call(entry, C.byref(struct_args(cls, **fields, **{count: 0})), None) == 0      # an empty batch: nothing launched
    for what, change in removals(tier):
        f = dict(fields)
        for k, v in change.items():
            f[k] = f[k] + 4 if v == "+4" else v
        with pytest.raises(CommuHipError, match="-22"):
            call(entry, C.byref(struct_args(cls, **f, **{count: 1})), None)
            pytest.fail(f"{entry} at tier {tier} accepted a struct with {what}")
