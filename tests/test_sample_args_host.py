"""The two argument structs of the sampling stage on the host (the library loads without a GPU, as test_abi.py shows): the
ctypes mirrors have the library's sizeof, an empty batch is a no-op, and a struct of another size is refused before the
empty-batch early-out."""
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
