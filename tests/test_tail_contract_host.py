"""The layer-tail / head contract tests have teeth (CPU only): on every input set that tests/test_tail_contract_gpu.py
launches, built by the same builders (tests/tail_contract.py),

  * the honest evaluation -- float32 in the kernels' order, rounded to the output types -- passes every stage bound, every
    exactness check and stays inside the tie cap;
  * every planted defect breaks a bound by >= 2x, or an exactness check, on a sub-batch of the set's rows (planted in
    the sets of 5, 17, 33 and 37 sequences: every template, mode and LayerNorm width);
  * every defect is planted in every kind of set (template x mode) it applies to;
  * 16 e32 <= C_PROD <= 2^-13, 16 eLN <= TAU, and both are the powers of two next above."""
import functools
import math

import pytest
import torch

import tail_contract as TC

SETS = TC.tail_sets()
IDS = [s[0] for s in SETS]
HEADS = TC.head_sets()


@functools.lru_cache(maxsize=None)
def _check(idx):
    s = TC.build_tail(*SETS[idx][1])
    honest = TC.run(s, TC.buffers(s))
    res = TC.check(s, honest)
    if s.active is not None:                                      # once more with active = null
        r2 = TC.check(s, TC.run(s, TC.buffers(s), use_active=False, base=honest), use_active=False)
        res["null_active"] = TC.worst(r2)
    if s.B in (1, 16, 64):                                        # (defects are planted in the sets of the other batch sizes)
        return s, res, {}, []
    sub = s.sub(TC.defect_rows(s))
    base = TC.run(sub, TC.buffers(sub))
    assert TC.worst(TC.check(sub, base)) <= 1.0
    caught, missed = {}, []
    for d, stages in TC.DEFECTS.items():
        for st in stages:
            if not TC.applicable(sub, d, st):
                continue
            r = TC.worst(TC.check(sub, TC.run(sub, TC.buffers(sub), d, st, base=base), stages=TC.window(sub, d, st)))
            caught[d] = min(caught.get(d, math.inf), r)
            if not r >= 2.0:
                missed.append((d, st, r))
    return s, res, caught, missed


@pytest.mark.parametrize("idx", range(len(SETS)), ids=IDS)
def test_honest_evaluation_passes_and_every_planted_defect_is_caught(idx):
    s, res, caught, missed = _check(idx)
    print(f"{IDS[idx]}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()) + "; defects "
          + ", ".join(f"{d} >= {r:.1f}" for d, r in sorted(caught.items())))
    assert TC.worst(res) <= 1.0, res
    assert res.get("null_active", 0.0) <= 1.0
    assert not missed, missed


def test_every_defect_is_planted_in_every_template_and_mode():
    seen = {}
    for idx in range(len(SETS)):
        s, _, caught, _ = _check(idx)
        seen.setdefault((s.wide, s.mode), set()).update(caught)
    for (wide, mode), got in seen.items():
        want = set(TC.DEFECTS) - ({"inactive_written", "logits_tail"} if mode == "qkv" else set())
        assert want <= got, (wide, mode, want - got)
    assert {(w, m) for w in (False, True) for m in ("qkv", "logits")} == set(seen)


@functools.lru_cache(maxsize=None)
def _head(i):
    s = TC.build_head(*HEADS[i][1])
    res = TC.head_check(s, TC.head_run(s, TC.head_buffers(s)))
    caught = {}
    for d in TC.HEAD_DEFECTS:
        if d == "bad_id_row0" and bool(((s.tok >= 0) & (s.tok < TC.V)).all()):
            continue
        caught[d] = TC.head_worst(TC.head_check(s, TC.head_run(s, TC.head_buffers(s), d)))
    return s, res, caught


@pytest.mark.parametrize("i", range(len(HEADS)), ids=[h[0] for h in HEADS])
def test_head_honest_evaluation_and_defects(i):
    s, res, caught = _head(i)
    print(f"{HEADS[i][0]}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()) + "; defects "
          + ", ".join(f"{d} >= {r:.1f}" for d, r in sorted(caught.items())))
    assert TC.head_worst(res) <= 1.0, res
    assert all(r >= 2.0 for r in caught.values()), caught
    assert set(caught) >= set(TC.HEAD_DEFECTS) - {"bad_id_row0"}
    if s.B > 4:
        assert "bad_id_row0" in caught


@pytest.mark.parametrize("shape", list(TC.SHAPES))
def test_exact_probes_on_the_host(shape):
    """The head probe and the phase-1 probe are exact in the honest evaluation, and a swapped tile breaks them."""
    D, DI, HD = TC.SHAPES[shape]
    s = TC.build_head(shape, 17, 500 if shape == "n640" else D, probe=True)
    assert TC.head_worst(TC.head_check(s, TC.head_run(s, TC.head_buffers(s)))) == 0
    assert TC.head_worst(TC.head_check(s, TC.head_run(s, TC.head_buffers(s), "tile_swap"))) >= 2
    p, k = TC.phase1_probe(shape, 17)
    b = TC.run(p, TC.buffers(p))
    assert torch.equal(b["z1"][:17], p.Wo[:, k].T.contiguous())


def test_pack_layout_is_a_permutation_of_the_weight():
    """pack_layout: every element of W exactly once, zeros for rows >= N, in the order load_w reads."""
    for N, K in TC.PACK_CASES:
        W = (torch.arange(N * K, dtype=torch.int32) + 1).view(N, K)
        p = TC.pack_layout(W, N, K)
        nz = p[p != 0]
        assert nz.numel() == N * K and torch.equal(nz.sort().values, W.reshape(-1))
        # tile t = 0 of workgroup ng = 1, wave 0, step 0, lane 17: W[16 + 1][8 .. 16]
        KS, NT = K // 128, ((N + 15) // 16 + 31) // 32
        c = (((1 * NT + 0) * 4 + 0) * KS + 0) * 64 + 17
        assert torch.equal(p[8 * c:8 * c + 8], W[17, 8:16])


def test_the_constants_of_the_bounds():
    """16 e32 <= C_PROD <= 2^-13 and C_PROD is the power of two next above 16 e32; the same for TAU and eLN."""
    e = {}
    tiecap = 0.0
    lo = math.inf
    for idx in range(len(SETS)):
        _, res, caught, _ = _check(idx)
        for k, v in res.items():
            if k.startswith("e32") or k == "eLN":
                e[k] = max(e.get(k, 0.0), v)
        tiecap = max(tiecap, res["tiecap"])
        lo = min([lo] + list(caught.values()))
    for i in range(len(HEADS)):
        _, res, caught = _head(i)
        e["e32_head"] = max(e.get("e32_head", 0.0), res["e32_head"])
        lo = min([lo] + list(caught.values()))
    e32 = max(v for k, v in e.items() if k.startswith("e32"))
    print("measured: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(e.items())))
    print(f"e32 {e32:.3e}, 16 e32 = {16 * e32:.3e}, C_PROD = {TC.C_PROD:.3e}; eLN {e['eLN']:.3e}, 16 eLN = {16 * e['eLN']:.3e}, "
          f"TAU = {TC.TAU:.3e}; tie-cap occupancy of the honest evaluation {tiecap:.3f}; smallest planted-defect ratio {lo:.1f}")
    assert {"e32_S1", "e32_S2", "e32_S3", "e32_S4b", "e32_head", "eLN"} <= set(e)
    assert 16 * e32 <= TC.C_PROD <= 2.0 ** -13 and TC.C_PROD < 32 * e32
    assert 16 * e["eLN"] <= TC.TAU < 32 * e["eLN"]
    assert tiecap <= 1.0
