"""Constrained sampling on the GPU: the sampling kernel with a per-slot additive bias row (commu_sample_args.bias)
against the launch without one (bit for bit), against the numpy restatement of the documented order
(logit_bias_contract.restate: bias, top-k, rejected tokens, top-p), its write-back and edge rows; then the same rows
through the decode loop (fused launch, captured graph, in-place updates, primed slots) and the single-request API."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import logit_bias_contract as LB  # noqa: E402
import test_decode_gpu as TD  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
from sample_launch import sample_launch  # noqa: E402

DEV = "cuda"
V = 729
NEG = float("-inf")
LOGP_TOL = SR.LOGP_TOL          # (the reference is fed y as fp32 rounds it: the added operation brings no new error)
bits = SR.bits


def bias_rows(logits):
    """One constraint row per kernel row, kind (b // 2) % 4: none (zeros), bans (pitches outside 40 .. 80 and the chord
    tokens), a finite re-weighting (|bias| <= 4 on every id), both."""
    g = torch.Generator().manual_seed(29)
    fin = (torch.rand(64, 768, generator=g) * 8 - 4)
    bias = torch.zeros(64, 768)
    kind = (torch.arange(64) // 2) % 4
    bias[kind >= 2] = fin[kind >= 2]
    ban = torch.zeros(768, dtype=torch.bool)
    ban[3:3 + 40] = ban[3 + 81:131] = ban[195:304] = True
    for b in range(64):
        if kind[b] in (1, 3):
            bias[b, ban] = NEG
    return bias, kind


def launch(logits, wrong, us, t, k, p, active=None, bias=None, ld_bias=None, v=V, logp=True, uniform=None):
    """One launch on fresh device copies (sample_launch); t / k / p: per-row tensors; bias None: a null pointer."""
    u = us if uniform is None else torch.full((logits.shape[0],), uniform, dtype=torch.float32)
    return sample_launch(logits, wrong, u, t, k, p, v=v, active=active, logp=logp, bias=bias, ld_bias=ld_bias)


@pytest.fixture(scope="module")
def rows():
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    active = torch.ones(64, dtype=torch.uint8)
    active[1::4] = 0
    bias, kind = bias_rows(logits)
    return dict(logits=logits, wrong=wrong, us=us, which=which, t=t, k=k, p=p, active=active, bias=bias, kind=kind)


def _args(r):
    return r["logits"], r["wrong"], r["us"], r["t"], r["k"], r["p"]


def same(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. nothing changes
def test_null_bias_zero_bias_and_the_rows_entry_point_agree_bit_for_bit(rows):
    """Tokens, probs_out, the log-probability pair and the written-back logits, with and without an active mask.  (The
    former entry point without a bias argument and the one with a null bias are one call of commu_sample_topk now: `old`.)"""
    for active in (None, rows["active"]):
        old = launch(*_args(rows), active=active)
        zero = launch(*_args(rows), active=active, bias=torch.zeros(64, 768))
        assert same(old, zero)
        assert int((old[1] == -1).sum()) >= 1 and int((old[1] > 0).sum()) >= 40
    # and through ops.sample_topk, which fills the same struct
    lg, tok, pr, lp = SR.run_rows(rows["logits"], rows["wrong"], rows["us"], rows["t"], rows["k"], rows["p"],
                                  rows["active"], logp=True)
    assert same(old, (lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()))


# ------------------------------------------------------------------------------------------------ 2. bans are exact
def test_bans_are_exact_zeros_and_never_drawn(rows):
    bias, kind, on = rows["bias"], rows["kind"], rows["active"].bool()
    banned = bias[:, :V] == NEG
    assert int(banned[kind == 1].sum()) > 1000
    for u in (0.0, 1.0 - 2.0 ** -24, 0.1, 0.37, 0.5, 0.9, 0.999):
        lg, tok, pr, lp = launch(*_args(rows), active=rows["active"], bias=bias, uniform=u)
        drew = on & (tok >= 0)
        assert int(drew.sum()) >= 40
        assert bool((pr[drew][banned[drew]] == 0.0).all())               # exactly 0, not merely small
        assert not bool(banned[drew, tok[drew].long()].any()), u
        assert bool((tok[~on] == -7).all()) and bool((pr[~on] == -3.0).all())


def test_a_ban_takes_none_of_the_k_places(rows):
    """The discriminating case: every row bans its own top_k most likely ids.  Rows without a rejected token and without
    a nucleus must still keep exactly top_k survivors -- the next top_k ids; a ban applied after top-k (where the
    rejected-token mask sits) leaves no mass and ends in Q12 (shown for the restatement in test_logit_bias_host.py).
    Greedy rows draw their (top_k + 1)-th id."""
    logits, k, t, p = rows["logits"], rows["k"], rows["t"], rows["p"]
    order = torch.argsort(logits[:, 1:V], dim=1, descending=True, stable=True) + 1
    bias = torch.zeros(64, 768)
    for b in range(64):
        bias[b, order[b, :int(k[b])]] = NEG
    lg, tok, pr, lp = launch(*_args(rows), bias=bias)
    plain = 0
    for b in range(64):
        kb = int(k[b])
        top, nxt = order[b, :kb], order[b, kb:2 * kb]
        assert bool((pr[b, top] == 0.0).all()) or int(tok[b]) == -1, b
        if float(t[b]) == 0:
            if not bool(rows["wrong"][b, order[b, kb]]):
                assert int(tok[b]) == int(order[b, kb]), b
            continue
        if bool(rows["wrong"][b, nxt].any()) or float(p[b]) < 1:
            continue
        res = LB.restate(logits[b].numpy(), float(t[b]), kb, bias=bias[b].numpy(), u=float(rows["us"][b]))
        assert LB.ban_is_before_topk(res, top.tolist(), kb)
        got = types_ns(tok[b], pr[b])
        assert LB.ban_is_before_topk(got, top.tolist(), kb), b
        assert set(np.flatnonzero(got.probs > 0)) == set(nxt.tolist()), b
        plain += 1
    assert plain >= 12


def types_ns(tok, pr):
    import types
    return types.SimpleNamespace(token=int(tok), probs=pr.double().numpy())


# ------------------------------------------------------------------------------------------------ 3. finite bias
def check_against_restatement(rows, out, rows_in, bias, v=V, tol=LOGP_TOL):
    """probs_out, full and kept of every row against restate() on the fp32 rows `rows_in`; returns the restatements."""
    lg, tok, pr, lp = out
    on = rows["active"].bool()
    worst = [0.0, 0.0, 0.0]
    refs = []
    for b in range(64):
        if not on[b]:
            assert lp[b].tolist() == [7.0, 7.0] and int(tok[b]) == -7
            refs.append(None)
            continue
        res = LB.restate(rows_in[b], float(rows["t"][b]), int(rows["k"][b]), float(rows["p"][b]), rows["wrong"][b].numpy(),
                         None if bias is None else bias[b].numpy(), float(rows["us"][b]), V=v)
        refs.append(res)
        assert np.array_equal(lg[b].numpy().view(np.int32), res.written.view(np.int32)), b
        if res.token < 0:
            assert int(tok[b]) == -1 and bool(torch.isnan(lp[b]).all()) and bool(torch.isnan(pr[b, :v]).all()), b
            continue
        got = pr[b, :v].double().numpy()
        tb = int(tok[b])
        assert ((got > 0) == (res.probs > 0)).all(), b
        assert 1 <= tb < v and res.probs[tb] > 0, b
        worst[0] = max(worst[0], np.abs(got - res.probs).max())
        worst[1] = max(worst[1], abs(float(lp[b, 0]) - res.full[tb]))
        worst[2] = max(worst[2], abs(float(lp[b, 1]) - (0.0 if float(rows["t"][b]) == 0 else np.log(res.probs[tb]))))
        assert float(lp[b, 0]) <= float(lp[b, 1]) + tol
        if float(rows["t"][b]) == 0:
            assert float(lp[b, 1]) == 0.0, b
        assert bool((pr[b, v:] == -3.0).all())
    print("max |probs - float64|, |full - float64|, |kept - log p|:", worst)
    assert max(worst) <= tol, worst
    return refs


def test_finite_bias_against_the_float64_restatement(rows):
    """probs_out, full and kept of the 64 mixed rows (bans, finite bias, both, none; top-k, top-p, rejected tokens, greedy,
    inactive rows) within LOGP_TOL of the restatement, which is fed y as fp32 rounds it.  Then +4 on the id a greedy row
    drew without a bias: it is drawn again and its `full` has moved."""
    bias = rows["bias"]
    out = launch(*_args(rows), active=rows["active"], bias=bias)
    refs = check_against_restatement(rows, out, rows["logits"].numpy(), bias)
    assert sum(1 for r in refs if r is not None and r.token < 0) >= 1
    free = launch(*_args(rows), active=rows["active"])
    greedy = [b for b in range(64) if float(rows["t"][b]) == 0 and int(free[1][b]) >= 1]
    assert len(greedy) >= 4
    plus = torch.zeros(64, 768)
    for b in greedy:
        plus[b, int(free[1][b])] = 4.0
    moved = launch(*_args(rows), active=rows["active"], bias=plus)
    for b in greedy:
        assert int(moved[1][b]) == int(free[1][b])
        assert abs(float(moved[3][b, 0]) - float(free[3][b, 0])) > 1e-3, b
    check_against_restatement(rows, moved, rows["logits"].numpy(), plus)


def test_tail_lanes_and_the_row_stride(rows):
    """V = 600: lanes whose ids lie past V load a clamped index and contribute nothing (the bias holds NaN there, the
    logits +inf); ld_bias = 729: a bias of another row stride gives the same bits."""
    bias = rows["bias"].clone()
    out768 = launch(*_args(rows), active=rows["active"], bias=bias)
    out729 = launch(*_args(rows), active=rows["active"], bias=bias[:, :V].contiguous())
    assert same(out768, out729)
    bias[:, 600:] = float("nan")
    logits = rows["logits"].clone()
    logits[:, 600:] = float("inf")
    out = launch(logits, rows["wrong"], rows["us"], rows["t"], rows["k"], rows["p"], active=rows["active"], bias=bias,
                 v=600)
    check_against_restatement(rows, out, logits.numpy(), bias, v=600)
    assert bool((out[1][rows["active"].bool()] < 600).all())


# ------------------------------------------------------------------------------------------------ 4. write-back
def test_the_bias_is_never_written_back(rows):
    """After a biased call the logits are the unbiased call's, bit for bit; a second draw from them (Q5) reports the
    twice-divided row plus the bias ONCE."""
    bias = rows["bias"]
    first = launch(*_args(rows), active=rows["active"], bias=bias)
    free = launch(*_args(rows), active=rows["active"])
    assert torch.equal(bits(first[0]), bits(free[0]))
    assert not torch.equal(first[1], free[1])                            # (the draws did differ)
    second = launch(first[0], rows["wrong"], rows["us"], rows["t"], rows["k"], rows["p"], active=rows["active"],
                    bias=bias)
    check_against_restatement(rows, second, first[0].numpy(), bias)
    hot = (rows["which"] == 4) & rows["active"].bool() & (first[1] >= 0) & (second[1] >= 0)
    assert float((second[3][hot, 0] - first[3][hot, 0]).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 5. edge rows
def test_edge_rows():
    """Everything banned, and `wrong` removing the one allowed id: token -1 and a NaN pair (Q12), at temperature 0 and
    0.95.  Inactive rows keep their entries.  Greedy: the argmax of raw + bias, ties to the lowest id, kept == 0.0."""
    g = torch.Generator().manual_seed(31)
    logits = torch.randn(8, V, generator=g) * 2.5
    bias = torch.zeros(8, 768)
    wrong = torch.zeros(8, V, dtype=torch.uint8)
    t = torch.tensor([0.0, 0.95, 0.0, 0.95, 0.95, 0.0, 0.0, 0.95])
    k = torch.full((8,), 32, dtype=torch.int32)
    p = torch.ones(8)
    active = torch.ones(8, dtype=torch.uint8)
    bias[0:2, 1:V] = NEG                                                  # rows 0, 1: every id banned
    bias[2:5, 1:V] = NEG                                                  # rows 2, 3: one id left, and it is rejected
    bias[2:5, 77] = 0.5
    wrong[2:4, 77] = 1                                                    # row 4: the same row without the rejection
    active[5] = 0                                                         # row 5: inactive
    logits[6] = 0.0                                                       # row 6: greedy tie after the bias
    logits[6, 10], logits[6, 20], logits[6, 30] = 5.0, 3.0, 9.0
    bias[6, 20], bias[6, 30] = 2.0, NEG
    bias[7, 1:V] = NEG                                                    # row 7: the two smallest ids allowed
    bias[7, 1], bias[7, 2] = 0.0, 0.0
    us = torch.full((8,), 0.5)
    lg, tok, pr, lp = launch(logits, wrong, us, t, k, p, active=active, bias=bias)
    for b in (0, 1, 2, 3):
        assert int(tok[b]) == -1 and bool(torch.isnan(lp[b]).all()) and bool(torch.isnan(pr[b]).all()), b
    assert int(tok[4]) == 77 and float(pr[4, 77]) == 1.0 and int((pr[4] > 0).sum()) == 1
    assert abs(float(lp[4, 0])) <= LOGP_TOL and abs(float(lp[4, 1])) <= LOGP_TOL
    assert int(tok[5]) == -7 and lp[5].tolist() == [7.0, 7.0] and bool((pr[5] == -3.0).all())
    assert torch.equal(lg[5], logits[5])
    assert int(tok[6]) == 10 and float(lp[6, 1]) == 0.0 and float(pr[6, 10]) == 1.0
    ref = LB.restate(logits[6].numpy(), 0.0, 32, bias=bias[6].numpy())
    assert ref.token == 10 and abs(float(lp[6, 0]) - ref.full[10]) <= LOGP_TOL
    assert torch.equal(lg[6], logits[6])                                  # greedy writes nothing
    assert int(tok[7]) in (1, 2) and int((pr[7] > 0).sum()) == 2 and abs(float(pr[7].sum()) - 1) < 1e-6


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_sample_topk_refuses_mismatched_bias_tensors():
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    lg = torch.zeros(4, V, device=DEV)
    for bad in (torch.zeros(4, 768), torch.zeros(4, 768, device=DEV, dtype=torch.float64),
                torch.zeros(4, 768, device=DEV, dtype=torch.bfloat16), torch.zeros(3, 768, device=DEV),
                torch.zeros(4, 700, device=DEV), torch.zeros(768, device=DEV), torch.zeros(4, 1, 768, device=DEV),
                torch.zeros(4, 2 * 768, device=DEV)[:, ::2], torch.zeros(768, 4, device=DEV).t(),
                torch.zeros(1, 768, device=DEV).expand(4, 768), np.zeros((4, 768), np.float32)):
        with pytest.raises(CommuHipError, match="bias"):
            ops.sample_topk(lg, 0.95, 32, bias=bad)
    tok = ops.sample_topk(lg, 0.95, 32, bias=torch.zeros(8, 768, device=DEV)[::2])      # rows further apart are fine
    assert tok.shape == (4,)
    # the C entry point refuses a row stride shorter than the ids it reads
    with pytest.raises(CommuHipError, match="-22"):
        sample_launch(torch.zeros(4, V), None, None, 0.95, 32, 1.0, logp=False, bias=torch.zeros(4, 768), ld_bias=700)


# ------------------------------------------------------------------------------------------------ through the loop
@pytest.fixture(scope="module")
def fixture_model(golden_dir):
    z = TD.load(golden_dir, "g6_decode.npz")
    return z, TD._build(golden_dir, z, z["sample8m_bias"])


def loaded(z, model, B, bias=None, rows=None, max_prompt=0, prompts=None):
    """B slots of the margin fixture's request with its variates, log-probabilities recorded; bias: None (a decoder that
    never heard of constraints) or constraint rows for `rows`."""
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, B, int(z["sample8m_cfg"][3]), 4146, 0.95, 32, max_prompt=max_prompt)
    dec.record_logprobs()
    if bias is not None:
        dec.set_logit_bias(bias, rows=rows)
    reload(z, dec, prompts)
    return dec


def reload(z, dec, prompts=None):
    uni = np.full((dec.B, dec.ld_u), 0.5, dtype=np.float32)
    u = z["sample8m_uniforms"]
    uni[:, :len(u)] = u
    dec.load([z["encoded_meta"].tolist()] * dec.B, [TD._data(z, "sample8m")] * dec.B, uni, prompts=prompts)
    return uni


def run(dec, use_graph=True):
    with torch.no_grad():
        dec.run(use_graph=use_graph)
    torch.cuda.synchronize()
    return dec.seq.clone(), dec.fsm.clone(), dec.seq_logp.clone()


def draws(dec):
    """Per slot: (token list or None, boolean array: the token was drawn)."""
    seqs, lps = dec.sequences()[0], dec.logprobs()
    return [(s, None if s is None else ~np.isnan(lp[:, 0])) for s, lp in zip(seqs, lps)]


def constraint_set(twin_seq, twin_drawn):
    """The constraints of the loop tests, chosen from what the unconstrained twin drew so that they bite.  The fixture's
    small model hardly ever draws a pitch or a velocity token (its sequence is bars, positions and forced chords), so the
    two ranges exclude the twin's lowest drawn pitch / velocity bin where it drew one and are plain ranges otherwise; what
    bites by construction is `common`, the token the twin drew most often (EOS and BAR apart): a -12 re-weighting of it
    (finite), and a ban of it alone (top).  Returns (pitch, vel, fin, chords, top, common)."""
    from commu_amd.generate import token_constraints
    drawn = [t for t, d in zip(twin_seq, twin_drawn) if d]
    pitches = [t - 3 for t in drawn if 3 <= t < 131]
    bins = [t - 131 for t in drawn if 131 <= t < 195]
    lo = min(pitches) + 1 if pitches and min(pitches) < 127 else 60
    pitch = token_constraints(pitch_range=(lo, 127))
    vb = min(bins) + 1 if bins and min(bins) < 63 else 20
    vel = token_constraints(velocity_range=(2 * vb, 127))
    body = [t for t in drawn if t > 2]
    assert len(body) > 20
    common = max(set(body), key=body.count)
    fin = token_constraints(bias={common: -12.0, 2: -0.5, 433: 1.5})
    chords = token_constraints(ban=range(195, 304))
    top = token_constraints(ban=[common])
    return pitch, vel, fin, chords, top, common


def separate_launches(dec, n):
    """The loop with one launch per stage (pre | step, sample, post) instead of the fused one."""
    with torch.no_grad():
        dec.pre()
        for _ in range(n):
            dec.body()
            dec.pre()
    torch.cuda.synchronize()
    return dec.seq.clone(), dec.fsm.clone(), dec.seq_logp.clone()


@pytest.mark.parametrize("parity, B", [(False, 10), (True, 4)], ids=["bf16_10_slots", "parity_fp32_4_slots"])
def test_mixed_batch_through_the_loop(fixture_model, parity, B):
    """Slots: no constraint | pitch range | velocity range | finite bias | chord tokens banned (two of each; parity: none,
    pitch, finite, chords).  Graph replay == eager == separate launches (seq, records, seq_logp bit patterns); the
    unconstrained slots decode what a decoder that never heard of constraints decodes; no draw of a constrained slot is a
    banned id; forced chords still appear; the re-weighted slots (-12 on the twin's most frequent draw) differ from it."""
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        plain = loaded(z, model, B)
        assert plain.bias is None
        s0, f0, l0 = run(plain)
        twin_seq, twin_drawn = draws(plain)[0]
        assert twin_seq is not None and twin_drawn.sum() > 20
        pitch, vel, fin, chords, _, common = constraint_set(twin_seq, twin_drawn)
        zero = np.zeros(768, np.float32)
        per_slot = [zero, zero, pitch, pitch, vel, vel, fin, fin, chords, chords] if B == 10 else [zero, pitch, fin, chords]
        free = [b for b in range(B) if per_slot[b] is zero]
        res = []
        for mode in ("graph", "eager", "separate"):
            dec = loaded(z, model, B, bias=np.stack(per_slot))
            assert dec.state.parity == parity and dec.bias is not None
            if mode == "separate":
                res.append(separate_launches(dec, dec.generation_length + 1))      # (iterations past the end do nothing)
            else:
                res.append(run(dec, use_graph=mode == "graph"))
            if mode == "graph":
                assert dec.graph is not None
                got = draws(dec)
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert torch.equal(bits(res[0][2]), bits(other[2]))
        sg, fg, lg = res[0]
        for b in free:
            assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
        differ = 0
        for b in range(B):
            if per_slot[b] is zero:
                continue
            seq, drawn = got[b]
            assert seq is not None, b
            toks = np.asarray(seq)
            assert not (per_slot[b][toks[drawn]] == NEG).any(), b          # no draw is a banned id
            assert drawn.sum() > 10 and not drawn[:12].any()
            differ += seq != twin_seq
            if per_slot[b] is fin:
                assert seq != twin_seq and toks[drawn].tolist().count(common) < twin_seq.count(common), b
            if per_slot[b] is chords:
                forced = (toks >= 195) & (toks <= 303)          # the progression, placed by the rules: forced, not drawn
                assert forced.sum() >= 1 and not drawn[forced].any(), b
                assert toks[forced].tolist() == z["sample8m_chord_token"].tolist()[:int(forced.sum())]
        assert differ >= 1
    finally:
        model.parity_fp32 = False


def test_rows_change_in_place_under_one_capture(fixture_model):
    """set_logit_bias and rearm(logit_bias=) after the capture keep the graph object; the next run honours the new rows;
    clearing restores the unconstrained tokens.  BatchedGenerator keeps one decoder per batch size whatever the requests
    constrain."""
    from commu_amd.generate import BatchedGenerator, token_constraints
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    twin_seq, twin_drawn = draws(plain)[0]
    pitch, vel, fin, chords, top, common = constraint_set(twin_seq, twin_drawn)
    row1 = token_constraints(ban=list(range(195, 304)) + [common])
    row3 = token_constraints(ban=[common], pitch_range=(60, 72), bias={2: -0.25})
    dec = loaded(z, model, 4, bias=row1, rows=[1])
    assert dec.graph is None
    run(dec)
    g = dec.graph
    first = draws(dec)
    assert g is not None and first[0][0] == twin_seq and first[2][0] == twin_seq and first[1][0] != twin_seq
    assert not (row1[np.asarray(first[1][0])[first[1][1]]] == NEG).any()
    # a new row for slot 2, another one for slot 3 through rearm, slot 1 keeps its row
    dec.set_logit_bias(top, rows=[2])
    uni = reload(z, dec)
    dec.rearm(3, uni[3], logit_bias=row3)
    run(dec)
    assert dec.graph is g
    second = draws(dec)
    assert second[0][0] == twin_seq and second[1][0] == first[1][0]
    for b, row in ((2, top), (3, row3)):
        seq, drawn = second[b]
        assert seq != twin_seq and not (row[np.asarray(seq)[drawn]] == NEG).any(), b
    # clearing: zeros, bit-identical to no constraint
    dec.set_logit_bias(None, rows=[1])
    dec.set_logit_bias(None)
    reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and not bool(dec.bias.any())
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))
    # the single-request API: one decoder, constrained or not; a constraint does not outlive its request
    glen = int(z["sample8m_cfg"][3])
    meta, datas = [z["encoded_meta"].tolist()] * 4, [TD._data(z, "sample8m")] * 4
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
    a, _, lpa = gen.generate(meta, datas, 0.95, 32, return_logprobs=True)
    narrow = token_constraints(ban=[common], pitch_range=(60, 66))
    b_, _, lpb = gen.generate(meta, datas, 0.95, 32, return_logprobs=True, logit_bias=narrow)
    c, _, lpc = gen.generate(meta, datas, 0.95, 32, return_logprobs=True, logit_bias=np.stack([chords, pitch, vel, fin]))
    d, _, _ = gen.generate(meta, datas, 0.95, 32, return_logprobs=True)
    assert len(gen._decoders) == 1 and a == d and b_ != a
    for seq, lp, row in list(zip(b_, lpb, [narrow] * 4)) + list(zip(c, lpc, (chords, pitch, vel, fin))):
        if seq is not None:
            drawn = ~np.isnan(lp[:, 0])
            assert drawn.any() and not (row[np.asarray(seq)[drawn]] == NEG).any()
    out, started, lps = gen.generate_stream(meta[0], datas[0], 0.95, 32, need=4, accept=lambda s, r: True, slots=4,
                                            return_logprobs=True, logit_bias=token_constraints(ban=range(195, 304)))
    assert len(gen._decoders) == 1 and len(out) == 4
    for seq, lp in zip(out, lps):
        if seq is not None:
            drawn = ~np.isnan(lp[:, 0])
            assert not (chords[np.asarray(seq)[drawn]] == NEG).any()


def test_a_primed_slot_with_a_ban(fixture_model):
    """A prompt is not checked against the bans: prompt tokens inside the banned set load fine and stay in the sequence;
    only what is drawn afterwards is constrained."""
    from commu_amd.generate import token_constraints
    z, model = fixture_model
    plain = loaded(z, model, 2)
    run(plain)
    twin_seq, twin_drawn = draws(plain)[0]
    n_ctx = 1 + len(z["encoded_meta"])
    body = twin_seq[n_ctx:]
    common = constraint_set(twin_seq, twin_drawn)[5]
    cut = [i + 1 for i, t in enumerate(body) if t == common][4]          # right after the twin's fifth draw of `common`
    prompt = body[:cut]
    banned = [common]
    row = token_constraints(ban=banned)
    dec = loaded(z, model, 2, bias=row, rows=[1], max_prompt=len(prompt), prompts=[prompt, prompt])
    run(dec)
    (free_seq, _), (seq, drawn) = draws(dec)
    assert seq[:n_ctx + cut] == twin_seq[:n_ctx + cut] and free_seq[:n_ctx + cut] == twin_seq[:n_ctx + cut]
    assert not drawn[:n_ctx + cut].any() and drawn[n_ctx + cut:].any()
    assert set(seq[n_ctx:n_ctx + cut]) & set(banned)                                 # banned ids, from the prompt
    later = np.asarray(seq)[drawn]
    assert not (row[later] == NEG).any()

