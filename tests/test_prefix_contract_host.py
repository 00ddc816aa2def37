"""The shared-prefix decode attention's contract tests have teeth (CPU only): on every input set that
tests/test_prefix_gpu.py launches (tests/prefix_contract.py builds them),

  * the honest evaluation -- the contract in float32, another summation order, rounded to bf16 -- stays inside the
    per-element bound of decode_contract, unchanged;
  * every defect of prefix_contract.DEFECTS breaks that bound by >= 2x in some element of at least one set;
  * e32 = max |contract in float32 - contract in float64| / A over the new sets satisfies 16 e32 <= 2^-15, the existing
    constant (a set that violated any of this would have to change its inputs, never the bound)."""
import functools

import pytest

import decode_contract as DC
import prefix_contract as PC

SETS = PC.all_sets()
IDS = [s[0] for s in SETS]


@functools.lru_cache(maxsize=None)
def _check(idx):
    """(e32, worst honest ratio, {defect: worst-element ratio of the pair that shows it best})."""
    s = PC.build(**SETS[idx][1])
    want, A = s.evaluate()
    f32, _ = s.evaluate(PC.torch.float32)
    e32 = float(((f32 - want).abs() / A.clamp_min(1e-300)).max())
    got = f32.float().to(PC.torch.bfloat16).double()
    rows = [b for b in range(s.B) if s.active[b]]
    honest = float(DC.ratio(got[rows], want[rows], A[rows]).max())
    caught = {}
    for d in PC.DEFECTS:
        best = 0.0
        for p in s.pairs:
            bad, _ = s.evaluate_pair(p, PC.torch.float32, d)
            r = DC.ratio(bad.float().to(PC.torch.bfloat16).double(), want[p.b, p.h], A[p.b, p.h])
            best = max(best, float(r.nan_to_num(nan=0.0).max()))
        caught[d] = best
    return e32, honest, caught


@pytest.mark.parametrize("idx", range(len(SETS)), ids=IDS)
def test_honest_evaluation_stays_inside_the_bound(idx):
    e32, honest, caught = _check(idx)
    print(f"{IDS[idx]}: e32 {e32:.3e}, honest ratio {honest:.3f}, defects "
          + ", ".join(f"{d} {r:.1f}" for d, r in caught.items()))
    assert honest <= 1.0


@pytest.mark.parametrize("defect", PC.DEFECTS)
def test_every_defect_breaks_the_bound_on_some_set(defect):
    worst = {IDS[i]: _check(i)[2][defect] for i in range(len(SETS))}
    print(defect, {k: round(v, 1) for k, v in worst.items()})
    assert max(worst.values()) >= 2.0, worst


def test_the_sets_cover_what_the_issue_names():
    """Probes on the first and last key of every prefix chunk, on P - 1, private row 0 and the new token; every private
    length active somewhere; two effective suffix chunks in the long sets."""
    for DH in (64, 32):
        klens = set()
        for name, kw in SETS:
            if kw["DH"] != DH:
                continue
            s = PC.build(**kw)
            prefix, private0, new = set(), 0, 0
            for p in s.pairs:
                k = int(s.klen[p.b])
                klens.add(k)
                prefix |= {x for x in p.probes if x < s.P}
                private0 += s.P in p.probes
                new += s.P + k in p.probes
            assert prefix == {x for x in PC.candidates(s.P, 0) if x < s.P}, (name, prefix)
            assert private0 and new, name
            if kw.get("nsplit", 1) > 1:
                assert max(len(s.records(b)) - -(-s.P // PC.CH) for b in range(s.B)) == 2
        assert set(PC.KLENS) <= klens


def test_the_library_tiles_the_prefix_as_the_sets_assume():
    """The chunk and group sizes the sets are built around are the library's (host calls: no GPU needed)."""
    from commu_amd import ops
    assert ops.decode_prefix_chunk() == PC.CH and ops.decode_prefix_group() == PC.G
    assert PC.B % PC.G and PC.PCAP % PC.CH
    assert ops.decode_prefix_ws_floats(PC.B, PC.H, 64, PC.PCAP, 2) == PC.B * PC.H * (2 + 3) * 66


def test_the_constant_of_the_bound_holds_for_the_new_sets():
    e32 = max(_check(i)[0] for i in range(len(SETS)))
    print(f"e32 over {len(SETS)} shared-prefix input sets: {e32:.3e}; 16 e32 = {16 * e32:.3e}; c = {DC.C_BF16:.3e}")
    assert 16 * e32 <= DC.C_BF16 == 2.0 ** -15
