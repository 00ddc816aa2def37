"""The decode-attention contract tests have teeth (CPU only): on every input set that tests/test_decode_contract_gpu.py
launches, built by the same builders (tests/decode_contract.py),

  * the honest evaluation -- the contract in float32, another summation order, rounded to the output type -- passes the
    per-element bound (a condition on the inputs: they are well enough conditioned for the bound to be meetable);
  * every planted defect that a pair is designed to catch violates the bound in at least one element by >= 2x;
  * every defect is planted in every kind of set it applies to;
  * the constant of the bound is at least 16x the float32 reference's own error e32 and at most 2^-13."""
import functools

import pytest
import torch

import decode_contract as DC

SETS = DC.all_sets()
IDS = [s[0] for s in SETS]

# which defects a kind of set must plant somewhere (decode.hip line -> defect: see decode_contract.DEFECTS)
_COMMON = {"drop_new", "stale_new", "drop_first", "dist_group"}
EXPECTED = {
    "linear": _COMMON | {"tail_clamp", "v_shift"},
    "split": _COMMON | {"tail_clamp", "v_shift", "chunk_first_drop", "chunk_first_dup"},
    "ring": _COMMON | {"tail_clamp", "v_shift", "hidden_plus", "hidden_minus", "ring_no_wrap"},
    "f32": _COMMON,
}


@functools.lru_cache(maxsize=None)
def _check(idx):
    """(kind, e32, worst honest ratio, {defect: (pairs, smallest worst-element ratio)}, pairs that miss)."""
    _, fn, args = SETS[idx]
    l = fn(*args)
    bf = l.dtype == torch.bfloat16
    want, A = l.evaluate()
    f32, _ = l.evaluate(torch.float32)
    e32 = float(((f32 - want).abs() / A.clamp_min(1e-300)).max())
    got = f32.float().to(l.dtype).double()
    honest = float(DC.ratio(got, want, A, bf).max())
    caught, missed = {}, []
    for p in l.pairs:
        for d in p.designed:
            bad, _ = l.evaluate(torch.float32, d, p)
            r = float(DC.ratio(bad[p.b, p.h].float().to(l.dtype).double(), want[p.b, p.h], A[p.b, p.h], bf).max())
            n, lo = caught.get(d, (0, float("inf")))
            caught[d] = (n + 1, min(lo, r))
            if not r >= 2.0:
                missed.append((d, p.b, p.h, len(p.rows), p.probes, r))
    return l.kind, e32, honest, caught, missed


@pytest.mark.parametrize("idx", range(len(SETS)), ids=IDS)
def test_honest_evaluation_passes_and_every_planted_defect_is_caught(idx):
    kind, e32, honest, caught, missed = _check(idx)
    print(f"{IDS[idx]}: e32 {e32:.2e}, honest ratio {honest:.3f}, defects "
          + ", ".join(f"{d} x{n} >= {r:.1f}" for d, (n, r) in sorted(caught.items())))
    assert honest <= 1.0
    assert not missed, missed
    assert caught, "a set without a single planted defect checks nothing"


def test_every_defect_is_planted_in_every_kind_of_set():
    seen = {}
    for idx in range(len(SETS)):
        kind, _, _, caught, _ = _check(idx)
        seen.setdefault(kind, set()).update(caught)
    assert set().union(*EXPECTED.values()) == set(DC.DEFECTS)
    for kind, want in EXPECTED.items():
        assert want <= seen[kind], (kind, want - seen[kind])


def test_the_constant_of_the_bound():
    """16 e32 <= c <= 2^-13 (above that the inputs would be too ill-conditioned for the defects to show)."""
    e32 = max(_check(idx)[1] for idx in range(len(SETS)))
    print(f"e32 over {len(SETS)} input sets: {e32:.3e}; 16 e32 = {16 * e32:.3e}; c = {DC.C_BF16:.3e}, c32 = {DC.C_F32:.3e}")
    for c in (DC.C_BF16, DC.C_F32):
        assert 16 * e32 <= c <= 2.0 ** -13
