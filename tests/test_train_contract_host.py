"""CPU proof for tests/train_contract.py: on every case set the clean fp32 emulation of a kernel stays at or below HALF of
every bound, and every planted defect exceeds a bound or breaks a guard on at least one case of that kernel's set.  A
defect that no case catches means the case set is too weak (fix the cases); an emulation above 0.5 means the bound does
not follow from rounding (redo the derivation)."""
import numpy as np
import pytest

import train_contract as TC

CLEAN = 0.5


def worst(res):
    return max(res.values()) if isinstance(res, dict) else float(res)


def clean(res):
    """the half-bound rule: a figure with a NAME~ companion (train_contract's docstring) may reach 1.0, its companion and
    every other figure 0.5; returns the worst of the figures held to 0.5"""
    if not isinstance(res, dict):
        return float(res)
    for k, v in res.items():
        if k + "~" in res:
            assert v <= 1.0, (k, v)
    return max(v for k, v in res.items() if k + "~" not in res)


def report(name, w):
    print(f"{name}: worst clean ratio {w:.3f}")


_LN = {}


def ln_inputs(case):
    if case not in _LN:
        inp = TC.LnInputs(*case)
        _LN[case] = (inp,) + TC.ln_stats32(inp)
    return _LN[case]


def test_case_sets_cover_what_the_issue_lists():
    cases = TC.ln_cases()
    for k in range(2):
        assert {D for D, ld, r in cases if ld == TC.ln_pitches(D)[k]} == set(TC.LN_D)
        assert {r for D, ld, r in cases if ld == TC.ln_pitches(D)[k]} == set(TC.LN_ROWS)
    assert any(D % 8 == 4 for D in TC.LN_D) and any(D < 64 for D in TC.LN_D) and 516 in TC.LN_D
    inp = TC.LnInputs(500, 504, 5)
    assert np.isnan(inp.z[:, 500:]).all() and float(inp.z[1, :500].std()) == 0.0
    assert abs(inp.z[4, :500]).max() == 200.0
    # both CE kernels of each direction are reached
    assert {TC.ce_vec_fwd(V, l) for V, l, _ in TC.ce_fwd_cases()} == {True, False}
    assert {TC.ce_vec_bwd(V, l, d) for V, l, d, _ in TC.ce_bwd_cases()} == {True, False}
    assert not TC.ce_vec_bwd(729, 736, 768) and TC.ce_vec_bwd(729, 768, 736)
    tg = {int(t) for V, l, r in TC.ce_fwd_cases() if V >= 729 for t in TC.CeInputs(V, l, r).target}
    assert {0, 255, 256, 511, 512} <= tg and (728 in tg or 767 in tg)
    # the grouped column sum needs two launches, by the task limit or by the source limit
    first, second = TC.group_cases()
    assert len(first) == 3 and len(TC.flush_plan([len(t[1]) for t in second])) == 2
    assert len(TC.TRANSPOSE_SHAPES) == 33
    # the grad_norm cases enter the 4-in-flight loop (the third with every lane once, leaving a 3-element tail)
    assert all(n > 3 * 1024 * p + 3 for n, p in TC.GRAD_NORM_CASES)
    assert TC.ADAM_N[-1] > 4096 * 1024


def test_layernorm_forward_emulation_and_defects():
    w = 0.0
    for case in TC.ln_cases():
        inp = ln_inputs(case)[0]
        w = max(w, clean(TC.ln_check_fwd(inp, *TC.ln_fwd_emu(inp))))
    report("layernorm_fwd", w)
    assert w <= CLEAN
    for defect in TC.LN_FWD_DEFECTS:
        assert any(worst(TC.ln_check_fwd(ln_inputs(c)[0], *TC.ln_fwd_emu(ln_inputs(c)[0], defect))) > 1.0
                   for c in TC.ln_cases()), defect


@pytest.mark.parametrize("add,masked", [(False, False), (True, False), (True, True), (False, True)],
                         ids=["bwd", "bwd_add", "bwd_add_masked", "bwd_masked"])
def test_layernorm_backward_emulation_and_defects(add, masked):
    scale = TC.drop_scale(0.25)

    def run(case, defect=None):
        inp, mu, rs = ln_inputs(case)
        keep = inp.keep() if masked else None
        dz, dzm, part = TC.ln_bwd_emu(inp, mu, rs, add, keep, scale, defect)
        return TC.ln_check_bwd(inp, mu, rs, dz, part, add, keep, scale, dzm)
    w = max(clean(run(c)) for c in TC.ln_cases())
    report("layernorm_bwd", w)
    assert w <= CLEAN
    for defect in TC.LN_BWD_DEFECTS:
        if defect == "add_dropped_chunk2" and not add:
            continue
        assert any(worst(run(c, defect)) > 1.0 for c in TC.ln_cases()), defect


def test_layernorm_defects_need_the_edge_shapes():
    """the comfortable shapes of the older kernel test (D a multiple of 64, pitch = D, even row counts) catch none of
    these: the edge cases are what the defects need"""
    inp = TC.LnInputs(128, 128, 64)
    mu, rs = TC.ln_stats32(inp)
    for defect in ("hi_upper", "pad_in_mean", "pad_not_zeroed", "pad_overwritten", "lookahead_accumulated",
                   "odd_row_skipped", "add_dropped_chunk2"):
        assert worst(TC.ln_check_fwd(inp, *TC.ln_fwd_emu(inp, defect))) <= 1.0, defect
        dz, dzm, part = TC.ln_bwd_emu(inp, mu, rs, True, None, 1.0, defect)
        assert worst(TC.ln_check_bwd(inp, mu, rs, dz, part, True)) <= 1.0, defect


def test_cross_entropy_emulation_and_defects():
    def fwd(c, defect=None):
        inp = TC.CeInputs(*c)
        return TC.ce_check_fwd(inp, *TC.ce_fwd_emu(inp, defect))

    def bwd(c, defect=None):
        V, ldl, ldd, rows = c
        inp = TC.CeInputs(V, ldl, rows)
        l32 = TC.ce_lse32(inp)
        return TC.ce_check_bwd(inp, l32, TC.ce_bwd_emu(inp, l32, ldd, defect), ldd)
    wf, wb = max(clean(fwd(c)) for c in TC.ce_fwd_cases()), max(clean(bwd(c)) for c in TC.ce_bwd_cases())
    report("ce_fwd", wf)
    report("ce_bwd", wb)
    assert wf <= CLEAN and wb <= CLEAN
    for defect in TC.CE_FWD_DEFECTS:
        for vec in (True, False):          # each forward kernel has to be caught on its own cases
            assert any(worst(fwd(c, defect)) > 1.0 for c in TC.ce_fwd_cases() if TC.ce_vec_fwd(c[0], c[1]) == vec), (defect, vec)
    for defect in TC.CE_BWD_DEFECTS:
        for vec in (True, False):
            assert any(worst(bwd(c, defect)) > 1.0 for c in TC.ce_bwd_cases() if TC.ce_vec_bwd(*c[:3]) == vec), (defect, vec)
    # rows without large logits (the older test's) do not notice a lost max-subtraction
    inp = TC.CeInputs(729, 768, 1)
    assert abs(float(inp.x[0, :729].mean())) < 1.0
    assert worst(TC.ce_check_fwd(inp, *TC.ce_fwd_emu(inp, "no_max_subtraction"))) <= 1.0


def test_column_sum_emulation_and_defects():
    w = 0.0
    for nblk in TC.REDUCE_NBLK:          # layernorm_bwd_reduce: three planes of part, accumulated into non-zero outputs
        for D in TC.REDUCE_D:
            g = np.random.default_rng(nblk * D)
            part = g.standard_normal((nblk, 3, D)).astype(TC.F32)
            for z in range(3):
                before = g.standard_normal(D).astype(TC.F32)
                got = TC.colsum_final_emu(before, part[:, z], 1.0)
                w = max(w, clean(TC.colsum_check(got, before, [(part[:, z], 1.0)])))
    for grp in TC.group_cases():
        tasks = [(t[0], TC.group_host_sources(t)) for t in grp]
        for t, out in zip(grp, TC.colsum_group_emu(tasks)):
            w = max(w, clean(TC.colsum_check(out, t[0], [(X, a) for _, X, a in t[1]])))
        for defect in ("alpha_shifted", "second_launch_first_task_skipped"):
            bad = TC.colsum_group_emu(tasks, defect)
            caught = any(worst(TC.colsum_check(out, t[0], [(X, a) for _, X, a in t[1]])) > 1.0 for t, out in zip(grp, bad))
            # (the first group is one launch: only the second can lose the first task of a second launch)
            assert caught or (defect == "second_launch_first_task_skipped" and len(grp) == 3), defect
    report("colsum", w)
    assert w <= CLEAN
    assert TC.flush_plan([1] * 50) == [list(range(48)), [48, 49]]
    assert TC.flush_plan([2] * 50) == [list(range(32)), list(range(32, 50))]


def test_masked_mean_groups_emulation_and_defects():
    w, caught = 0.0, False
    for k, (T, B, Bc) in enumerate(TC.MM_CASES):
        for all_pad in (None, 1 if B // Bc > 1 else None):
            inp = TC.MmInputs(T, B, Bc, all_pad)
            out, sum_all, cnt, g = TC.mm_emu(inp)
            res = TC.mm_check(inp, out, sum_all, cnt, g)
            w = max(w, clean(res))
            if all_pad is not None:
                assert np.isnan(out) and np.isfinite(g).all()
            caught = caught or worst(TC.mm_check(inp, *TC.mm_emu(inp, "group_is_i_div_Bc"))) > 1.0
    report("masked_mean_groups", w)
    assert w <= CLEAN and caught
    # B == Bc: one group, the mapping cannot go wrong -- and the defect is indeed invisible there
    inp = TC.MmInputs(5, 8, 8)
    assert TC.mm_check(inp, *TC.mm_emu(inp, "group_is_i_div_Bc")) == TC.mm_check(inp, *TC.mm_emu(inp))
    # ... and its sums are exact in fp32 whatever the order (what lets the GPU test ask for bit-identity with masked_mean)
    live = inp.target != TC.MM_PAD
    assert float(np.add.reduce(inp.nll[live], dtype=TC.F32)) == float(inp.nll[live].astype(np.float64).sum())


def test_optimiser_emulations_and_defects():
    bc1, bc2 = TC.bias_corrections32(TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_STEP)
    w = 0.0
    for n in TC.ADAM_N:
        p, g, m, v = TC.adam_inputs(n)
        coef = TC.clip_coef32(2.0, TC.ADAM_CLIP)
        want = TC.adam_ref(p, g, m, v, coef, bc1, bc2)
        po, mo, vo, pb = TC.adam_emu(p, g, m, v, coef, bc1, bc2)
        w = max(w, clean(TC.adam_check(want, po, mo, vo, pb)))
        bad = TC.adam_emu(p, g, m, v, coef, bc1, bc2, "tail_past_grid_skipped")
        assert (worst(TC.adam_check(want, *bad)) > 1.0) == (n > 4096 * 1024), n
    report("adam", w)
    assert w <= CLEAN
    wn = 0.0
    for n, npart in TC.GRAD_NORM_CASES:
        x = TC.grad_norm_inputs(n)
        wn = max(wn, TC.grad_norm_check(x, npart, TC.grad_norm_emu(x, npart)))
        bad = TC.grad_norm_check(x, npart, TC.grad_norm_emu(x, npart, "fourth_load_dropped"))
        assert bad > 1.0, (n, npart)
    report("grad_norm", wn)
    assert wn <= CLEAN
    # the older test's shape (n = 10007, 256 partials) never enters the 4-in-flight loop
    x = TC.grad_norm_inputs(10007)
    assert TC.grad_norm_check(x, 256, TC.grad_norm_emu(x, 256, "fourth_load_dropped")) <= 1.0
