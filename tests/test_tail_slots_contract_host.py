"""The layer-tail / head contract for 65 .. 256 sequences has teeth (CPU only; mirrors tests/test_tail_contract_host.py): on
every input set that tests/test_tail_slots_contract_gpu.py launches, built by the same builders (tests/tail_slots_contract.py),

  * the honest evaluation -- float32 in the kernels' order, rounded to the output types -- passes every stage bound, every
    exactness check and stays inside the tie cap (the bounds are tail_contract's, unchanged);
  * every planted defect breaks a bound by >= 2x, or an exactness check, on a sub-batch that holds one row of every row
    group in use;
  * `group_alias` (rows >= 64 read the hand-off buffers of row - 64: a kernel that kept `mg & 3` somewhere) is caught in every
    set and at every hand-off;
  * the sync block is laid out [3][16][64] beyond 64 sequences and [3][4][64] up to 64, where it is tail_contract's."""
import functools
import math

import pytest

import tail_contract as TC
import tail_slots_contract as SC

SETS = SC.tail_sets()
IDS = [s[0] for s in SETS]
HEADS = SC.head_sets()


@functools.lru_cache(maxsize=None)
def _check(idx):
    s = SC.build_tail(*SETS[idx][1])
    honest = SC.run(s, SC.buffers(s))
    res = SC.check(s, honest)
    if s.active is not None:                                      # once more with active = null
        r2 = SC.check(s, SC.run(s, SC.buffers(s), use_active=False, base=honest), use_active=False)
        res["null_active"] = SC.worst(r2)
    sub = s.sub(SC.defect_rows(s))
    assert {r // 16 for r in sub.rows} == set(range((s.B + 15) // 16))
    base = SC.run(sub, SC.buffers(sub))
    assert SC.worst(SC.check(sub, base)) <= 1.0
    caught, missed = {}, []
    for d, stages in SC.DEFECTS.items():
        for st in stages:
            if not SC.applicable(sub, d, st):
                continue
            r = SC.worst(SC.check(sub, SC.run(sub, SC.buffers(sub), d, st, base=base), stages=SC.window(sub, d, st)))
            caught[(d, st)] = r
            if not r >= 2.0:
                missed.append((d, st, r))
    return s, res, caught, missed


@pytest.mark.parametrize("idx", range(len(SETS)), ids=IDS)
def test_honest_evaluation_passes_and_every_planted_defect_is_caught(idx):
    s, res, caught, missed = _check(idx)
    by_defect = {}
    for (d, st), r in caught.items():
        by_defect[d] = min(by_defect.get(d, math.inf), r)
    print(f"{IDS[idx]}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()) + "; defects "
          + ", ".join(f"{d} >= {r:.1f}" for d, r in sorted(by_defect.items())))
    assert SC.worst(res) <= 1.0, res
    assert res.get("null_active", 0.0) <= 1.0
    assert not missed, missed
    # the row-group defects apply to every set here, at every hand-off
    for d in ("group0", "group_alias"):
        assert {st for (dd, st) in caught if dd == d} == {"S2", "S3", "S4a"}, d
    if s.active is not None:
        assert not bool(s.active[67]) and not bool(s.active[s.B - 1]) and ("inactive_written", "") in caught


def test_every_defect_is_planted_in_every_template_and_mode():
    seen = {}
    for idx in range(len(SETS)):
        s, _, caught, _ = _check(idx)
        seen.setdefault((s.wide, s.mode), set()).update(d for d, _ in caught)
    for (wide, mode), got in seen.items():
        want = set(SC.DEFECTS) - ({"inactive_written", "logits_tail"} if mode == "qkv" else set())
        # (one wide set per mode: LayerNorm width 1000 has no big row, width 1024 no pad columns)
        want -= {(True, "qkv"): {"ln_one_pass"}, (True, "logits"): {"ln_stats_D", "ln_stats_pad"}}.get((wide, mode), set())
        assert want <= got, (wide, mode, want - got)
    assert {(w, m) for w in (False, True) for m in ("qkv", "logits")} == set(seen)


@pytest.mark.parametrize("i", range(len(HEADS)), ids=[h[0] for h in HEADS])
def test_head_honest_evaluation_and_defects(i):
    s = SC.build_head(*HEADS[i][1])
    assert s.n_zero > 3 * 12 * SC.CNT_STRIDE * SC.LAYERS          # more words than six launches of 64 sequences have
    res = SC.head_check(s, SC.head_run(s, SC.head_buffers(s)))
    caught = {d: SC.head_worst(SC.head_check(s, SC.head_run(s, SC.head_buffers(s), d))) for d in TC.HEAD_DEFECTS}
    print(f"{HEADS[i][0]}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()) + "; defects "
          + ", ".join(f"{d} >= {r:.1f}" for d, r in sorted(caught.items())))
    assert SC.head_worst(res) <= 1.0, res
    assert all(r >= 2.0 for r in caught.values()), caught


def test_the_sync_block_layout():
    """[3][G][64] words, G = 4 up to 64 sequences -- there counter_words() is tail_contract's, word for word -- and 16
    beyond; the counters of different (phase, row group) pairs never share a word and stay inside the block."""
    for B in (1, 16, 37, 64):
        s = TC.build_tail("n512", B, "qkv", 512)
        s.G = SC.groups(B)
        assert SC.counter_words(s) == TC.counter_words(s) and SC.sync_words(B) == 12 * TC.CNT_STRIDE
    for B in (65, 80, 129, 256):
        s = SC.build_tail("n512", B, "qkv", 512)
        w = SC.counter_words(s)
        assert SC.sync_words(B) == 48 * TC.CNT_STRIDE
        assert len(set(w)) == len(w) == 3 * ((B + 15) // 16) and max(w) < SC.sync_words(B)
        assert w[(B + 15) // 16] == 16 * TC.CNT_STRIDE          # phase 1, row group 0
        assert SC.buffers(s)["sync"].numel() == SC.sync_words(B) + 64


def test_the_bounds_are_tail_contracts_and_keep_their_headroom():
    """C_PROD and TAU are tail_contract's: 16 x the float32 evaluation's error on ITS sets (up to 64 rows), rounded up to a
    power of two, the factor 16 being the room left for a kernel that sums in another order.  The maximum over four times
    as many rows of the same distribution is a little larger (measured here: e32 3.45e-8 against 5.01e-8 -- smaller --,
    eLN 2.55e-7 against 2.26e-7); the constants are NOT widened for that, and at least half of the factor must be left."""
    e32, eln, tiecap = 0.0, 0.0, 0.0
    for idx in range(len(SETS)):
        _, res, _, _ = _check(idx)
        e32 = max([e32] + [v for k, v in res.items() if k.startswith("e32")])
        eln = max(eln, res["eLN"])
        tiecap = max(tiecap, res["tiecap"])
    print(f"e32 {e32:.3e} (16 e32 = {16 * e32:.3e}, C_PROD {SC.C_PROD:.3e}); eLN {eln:.3e} (16 eLN = {16 * eln:.3e}, TAU "
          f"{SC.TAU:.3e}); tie-cap occupancy {tiecap:.3f}")
    assert SC.C_PROD == TC.C_PROD and SC.TAU == TC.TAU
    assert 8 * e32 <= SC.C_PROD and 8 * eln <= SC.TAU and tiecap <= 1.0
