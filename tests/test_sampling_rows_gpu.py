"""Per-sequence sampling controls and token log-probabilities of the decode loop: the sampling kernel with device arrays
of temperature / top_k / top_p against the same kernel with scalars (bit for bit), the (full, kept) log-probability pair
against float64, the pair's book-keeping through the forcing stages (seq_logp), and the single-request API on top
(ForcedDecoder.set_sampling, BatchedGenerator.generate / generate_stream with one decoder and one capture)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_decode_gpu as TD  # noqa: E402

DEV = "cuda"
V = 729
# (temperature, top_k, top_p): greedy, the reference's setting, a narrow top-k, a nucleus, a hot nucleus
TRIPLES = [(0.0, 32, 1.0), (0.95, 32, 1.0), (0.95, 8, 1.0), (0.7, 32, 0.5), (1.3, 16, 0.9)]
# |full - float64 log-softmax| and |kept - log(probs_out[token])|.  Derived, not measured: two fp32 subtractions at
# |x / T| <= 18 (ulp 1.9e-6 each), a 12-sequential + 6-level fp32 sum of 728 terms, expf / logf at a few ulp.
LOGP_TOL = 2e-5


def bits(t):
    return t.contiguous().view(torch.int32)


def kernel_rows():
    """64 x 729 logits, the triple of every row (row b: TRIPLES[b % 5]), a rejected-token mask on every third row (token 7
    and the row's most likely token: the greedy rows among them cannot draw, Q12), variates."""
    g = torch.Generator().manual_seed(23)
    logits = torch.randn(64, V, generator=g) * 2.5
    wrong = torch.zeros(64, V, dtype=torch.uint8)
    wrong[::3, 7] = 1
    wrong[torch.arange(0, 64, 3), logits[::3, 1:].argmax(1) + 1] = 1
    us = torch.rand(64, generator=g)
    which = torch.arange(64) % len(TRIPLES)
    t = torch.tensor([TRIPLES[i][0] for i in which], dtype=torch.float32)
    k = torch.tensor([TRIPLES[i][1] for i in which], dtype=torch.int32)
    p = torch.tensor([TRIPLES[i][2] for i in which], dtype=torch.float32)
    return logits, wrong, us, which, t, k, p


def run_rows(logits, wrong, us, t, k, p, active=None, logp=False):
    from commu_amd import ops
    lg = logits.clone().to(DEV)
    pr = torch.full((64, V), -3.0, device=DEV)
    tok = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((64, 2), 7.0, device=DEV) if logp else None
    dev = lambda x: x.to(DEV) if isinstance(x, torch.Tensor) else x
    ops.sample_topk(lg, dev(t), dev(k), wrong=wrong.to(DEV), uniforms=us.to(DEV), active=None if active is None else
                    active.to(DEV), token=tok, probs_out=pr, top_p=dev(p), logp_out=lp)
    return lg, tok, pr, lp


@pytest.mark.parametrize("masked", [False, True], ids=["all_rows", "active_mask"])
def test_per_row_controls_equal_the_scalar_kernel_bit_for_bit(masked):
    """Row b of a launch with per-row arrays is what the scalar launch with b's triple computes for row b: drawn token,
    probs_out and the in-place division of logits[b][1:V] (Q5); rows with active[b] == 0 are untouched."""
    logits, wrong, us, which, t, k, p = kernel_rows()
    active = None
    if masked:
        active = torch.ones(64, dtype=torch.uint8)
        active[1::4] = 0
    lg, tok, pr, _ = run_rows(logits, wrong, us, t, k, p, active)
    on = torch.ones(64, dtype=torch.bool) if active is None else active.bool()
    for i, (ti, ki, pi) in enumerate(TRIPLES):
        lg_s, tok_s, pr_s, _ = run_rows(logits, wrong, us, ti, ki, pi, active)
        rows = ((which == i) & on).nonzero().flatten()
        assert len(rows) >= 8
        assert torch.equal(tok[rows], tok_s[rows]), i
        assert torch.equal(bits(pr[rows]), bits(pr_s[rows])), i          # (bit patterns: the Q12 rows hold NaN)
        assert torch.equal(lg[rows], lg_s[rows]), i
    assert bool((tok[on.to(DEV)] != -7).all()) and bool((tok[on.to(DEV)] == -1).any())
    if masked:
        off = (~on).to(DEV)
        assert torch.equal(lg[off].cpu(), logits[~on]) and bool((tok[off] == -7).all()) and bool((pr[off] == -3.0).all())
    # the rows did sample differently: the scalar launches of two triples disagree somewhere
    assert not torch.equal(run_rows(logits, wrong, us, *TRIPLES[1])[2], run_rows(logits, wrong, us, *TRIPLES[2])[2])


def test_top_k_outside_its_range_is_clamped_in_the_kernel():
    """top_k 0 and 100 000 written straight into the device array (past the host check) behave like 1 and 729."""
    logits, wrong, us, _, _, _, _ = kernel_rows()
    k = torch.empty(64, dtype=torch.int32)
    k[::2], k[1::2] = 0, 100000
    lg, tok, pr, _ = run_rows(logits, wrong, us, 0.95, k, 1.0)
    for rows, kk in ((slice(0, 64, 2), 1), (slice(1, 64, 2), V)):
        lg_s, tok_s, pr_s, _ = run_rows(logits, wrong, us, 0.95, kk, 1.0)
        assert torch.equal(tok[rows], tok_s[rows]) and torch.equal(bits(pr[rows]), bits(pr_s[rows]))
        assert torch.equal(lg[rows], lg_s[rows])
    assert int((pr[1] > 0).sum()) == V - 1 and int((pr[2] > 0).sum()) == 1          # (rows 1, 2 have no rejected token)


def test_log_probabilities_against_float64():
    """full: the float64 log-softmax over ids 1 .. 728 of the row the draw used (the fp32 quotient logits / temperature,
    the raw row for greedy), at the drawn id; kept: log(probs_out[token]); both within LOGP_TOL.  A second draw from the
    same rows (Q5) reports the twice-divided row.  Greedy: kept == 0.0; nothing drawn (Q12): NaN, NaN; inactive rows keep
    their entries."""
    from commu_amd import ops
    logits, wrong, us, which, t, k, p = kernel_rows()
    active = torch.ones(64, dtype=torch.uint8)
    active[1::4] = 0
    on = active.bool()

    def reference(row_f32, b):
        x = row_f32[b, 1:V]
        if float(t[b]) != 0:
            x = x / np.float32(float(t[b]))                   # fp32 division (IEEE), as the kernel writes it back
        assert x.dtype == np.float32
        x = x.astype(np.float64)
        return x - x.max() - np.log(np.exp(x - x.max()).sum())

    def check(lp, tok, pr, rows_in):
        lp, tok, pr = lp.cpu().numpy(), tok.cpu().numpy(), pr.cpu().double().numpy()
        worst = [0.0, 0.0]
        nfail = 0
        for b in range(64):
            if not on[b]:
                assert lp[b, 0] == 7.0 and lp[b, 1] == 7.0, b
                continue
            if tok[b] < 0:
                assert float(t[b]) == 0 and np.isnan(lp[b]).all(), b
                nfail += 1
                continue
            assert tok[b] >= 1 and pr[b, tok[b]] > 0
            worst[0] = max(worst[0], abs(lp[b, 0] - reference(rows_in, b)[tok[b] - 1]))
            worst[1] = max(worst[1], abs(lp[b, 1] - np.log(pr[b, tok[b]])))
            if float(t[b]) == 0:
                assert lp[b, 1] == 0.0, b
        print("max |full - float64|, max |kept - log p|:", worst)
        assert worst[0] <= LOGP_TOL and worst[1] <= LOGP_TOL, worst
        return nfail

    lg, tok, pr, lp = run_rows(logits, wrong, us, t, k, p, active, logp=True)
    assert check(lp, tok, pr, logits.numpy()) >= 1          # (a greedy row whose argmax is rejected)
    # requesting the pair changes nothing else
    lg0, tok0, pr0, _ = run_rows(logits, wrong, us, t, k, p, active)
    assert torch.equal(tok, tok0) and torch.equal(bits(pr), bits(pr0)) and torch.equal(lg, lg0)
    # a second draw from the rows the first one divided: the compounded row
    once = logits.numpy().copy()
    for b in range(64):
        if on[b] and float(t[b]) != 0:
            once[b, 1:V] = once[b, 1:V] / np.float32(float(t[b]))
    pr2 = torch.zeros(64, V, device=DEV)
    lp2 = torch.full((64, 2), 7.0, device=DEV)
    tok2 = ops.sample_topk(lg, t.to(DEV), k.to(DEV), wrong=wrong.to(DEV), uniforms=us.to(DEV), active=active.to(DEV),
                           probs_out=pr2, top_p=p.to(DEV), logp_out=lp2)
    check(lp2, tok2, pr2, once)
    hot = (which == 4) & on          # (T = 1.3: dividing twice flattens the row, the numbers must have moved)
    assert float((lp2[hot.to(DEV), 0] - lp[hot.to(DEV), 0]).abs().max()) > 1e-3


def test_sample_topk_refuses_mismatched_control_tensors():
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    lg = torch.zeros(4, V, device=DEV)
    for kw in (dict(temperature=torch.ones(4)), dict(temperature=torch.ones(3, device=DEV)),
               dict(temperature=torch.ones(4, device=DEV, dtype=torch.float64)),
               dict(top_k=torch.ones(4, device=DEV)), dict(top_k=torch.ones(8, device=DEV, dtype=torch.int32)[::2]),
               dict(top_p=torch.ones(4, 1, device=DEV)), dict(logp_out=torch.zeros(4, 3, device=DEV)),
               dict(logp_out=torch.zeros(4, 2, device=DEV, dtype=torch.float64)), dict(logp_out=torch.zeros(4, 2))):
        args = dict(temperature=0.95, top_k=32, top_p=1.0)
        args.update(kw)
        with pytest.raises(CommuHipError):
            ops.sample_topk(lg, args.pop("temperature"), args.pop("top_k"), **args)


# ------------------------------------------------------------------------------------------------ through the loop
@pytest.fixture(scope="module")
def fixture_model(golden_dir):
    z = TD.load(golden_dir, "g6_decode.npz")
    return z, TD._build(golden_dir, z, z["sample8m_bias"])


def loaded_decoder(z, model, B, triple=(0.95, 32, 1.0), rows=None):
    """B slots of the margin fixture's request with its variates; `rows`: per-slot triples set after construction."""
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, B, int(z["sample8m_cfg"][3]), 4146, triple[0], triple[1], top_p=triple[2])
    if rows is not None:
        dec.set_sampling([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    else:
        dec.record_logprobs()          # (a decoder that was never asked for either runs without the arrays)
    uni = np.full((B, dec.ld_u), 0.5, dtype=np.float32)
    u = z["sample8m_uniforms"]
    uni[:, :len(u)] = u
    dec.load([z["encoded_meta"].tolist()] * B, [TD._data(z, "sample8m")] * B, uni)
    return dec


def test_mixed_batch_graph_equals_eager_and_the_uniform_batches(fixture_model):
    """10 slots, two per triple.  Graph replay == eager launches (token buffers, state records, seq_logp: bit patterns),
    and each slot decodes what it decodes in a batch whose 10 slots all carry its triple (a decoder built the old way)."""
    z, model = fixture_model
    rows = [TRIPLES[b // 2] for b in range(10)]
    res = []
    for use_graph in (True, False):
        dec = loaded_decoder(z, model, 10, rows=rows)
        with torch.no_grad():
            dec.run(use_graph=use_graph)
        torch.cuda.synchronize()
        res.append((dec.seq.clone(), dec.fsm.clone(), dec.seq_logp.clone(), dec.sequences()[0], dec.logprobs()))
    (sg, fg, lg, seqs, lps), (se, fe, le, _, _) = res
    assert torch.equal(sg, se) and torch.equal(fg, fe) and torch.equal(bits(lg), bits(le))
    assert len({None if s is None else tuple(s) for s in seqs}) >= 3          # the triples decode differently
    for i, triple in enumerate(TRIPLES):
        dec = loaded_decoder(z, model, 10, triple=triple)
        with torch.no_grad():
            dec.run(use_graph=True)
        torch.cuda.synchronize()
        s_u, lp_u = dec.sequences()[0], dec.seq_logp
        for b in (2 * i, 2 * i + 1):
            assert seqs[b] == s_u[b], (i, b)
            assert torch.equal(bits(lg[b]), bits(lp_u[b])), (i, b)
            if seqs[b] is None:
                assert lps[b] is None
                continue
            lp = lps[b]
            assert lp.shape == (len(seqs[b]), 2) and np.isnan(lp[:12]).all()
            drawn = ~np.isnan(lp[:, 0])
            assert drawn.any() and (lp[drawn] <= 0).all() and (lp[drawn, 0] <= lp[drawn, 1] + LOGP_TOL).all()
            if triple[0] == 0:
                assert (lp[drawn, 1] == 0).all()


@pytest.mark.parametrize("parity", [False, True], ids=["bf16", "parity_fp32"])
def test_seq_logp_bookkeeping(fixture_model, parity):
    """Per-stage launches, 8 slots, 24 iterations: an appended draw's pair sits at the token's index (kept against the
    distribution the iteration drew from), context and forced tokens hold NaN, a rejected chord leaves the length and
    seq_logp as they were."""
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        dec = loaded_decoder(z, model, 8)
        F_LEN = 0
        seen = {"appended": 0, "forced": 0, "rejected": 0}
        worst = 0.0
        with torch.no_grad():
            for _ in range(24):
                len0, lp0 = dec.fsm[:, F_LEN].cpu().numpy().copy(), dec.seq_logp.cpu()
                dec.iteration(want_probs=True)
                torch.cuda.synchronize()
                ln, lp, seq = dec.fsm[:, F_LEN].cpu().numpy(), dec.seq_logp.cpu(), dec.seq.cpu().numpy()
                drew, tok, pr = dec.draw.cpu().numpy(), dec.token.cpu().numpy(), dec.probs.cpu().double().numpy()
                for b in range(8):
                    assert ln[b] - len0[b] in (0, 1)
                    grew = ln[b] == len0[b] + 1
                    if drew[b] and grew:
                        assert seq[b, ln[b] - 1] == tok[b] and tok[b] >= 1
                        full, kept = lp[b, ln[b] - 1].tolist()
                        worst = max(worst, abs(kept - np.log(pr[b, tok[b]])))
                        assert full <= kept + LOGP_TOL and full > -50
                        seen["appended"] += 1
                    elif grew:          # a forced token
                        assert bool(torch.isnan(lp[b, ln[b] - 1]).all())
                        seen["forced"] += 1
                    if not grew or not drew[b]:
                        keep = torch.ones(dec.ld_seq, dtype=torch.bool)
                        if grew:
                            keep[ln[b] - 1] = False
                        assert torch.equal(bits(lp[b][keep]), bits(lp0[b][keep])), b
                    if drew[b] and 195 <= tok[b] <= 303:          # a chord token: rejected, drawn again
                        assert not grew and torch.equal(bits(lp[b]), bits(lp0[b]))
                        seen["rejected"] += 1
                    assert bool(torch.isnan(lp[b, :12]).all()) and bool(torch.isnan(lp[b, ln[b]:]).all())
        print("max |kept - log p|:", worst, seen)
        assert worst <= LOGP_TOL
        assert min(seen.values()) >= 8, seen
    finally:
        model.parity_fp32 = False


def test_one_decoder_and_one_capture_for_every_setting(fixture_model):
    """Three settings on one generator: one ForcedDecoder, one captured graph, and each result is what a fresh generator
    gives for that setting alone."""
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    glen = int(z["sample8m_cfg"][3])
    meta, datas = [z["encoded_meta"].tolist()] * 8, [TD._data(z, "sample8m")] * 8
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
    graph, outs = None, []
    settings = [(0.95, 32), (0.6, 32), (1.2, 12)]
    for temp, top_k in settings:
        seqs, _, lps = gen.generate(meta, datas, temp, top_k, return_logprobs=True)
        assert len(gen._decoders) == 1
        dec = next(iter(gen._decoders.values()))
        graph = graph or dec.graph
        assert graph is not None and dec.graph is graph
        outs.append((seqs, lps))
    assert outs[0][0] != outs[1][0] and outs[1][0] != outs[2][0]
    for (temp, top_k), (seqs, lps) in zip(settings, outs):
        fresh = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
        s2, _, lp2 = fresh.generate(meta, datas, temp, top_k, return_logprobs=True)
        assert seqs == s2, temp
        for a, b in zip(lps, lp2):
            assert (a is None and b is None) or np.array_equal(a.view(np.int32), b.view(np.int32))


def test_stream_schedule_is_indexed_by_attempt(fixture_model):
    """generate_stream with a temperature schedule: attempt a decodes at schedule[a % 3] whichever slot takes it -- the
    answer and its log-probabilities equal generate() with the per-row triples and the attempts' variates; slots re-armed
    for attempts 6 .. 11 take those attempts' controls (the greedy attempts repeat attempt 0)."""
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    glen = int(z["sample8m_cfg"][3])
    meta, data = z["encoded_meta"].tolist(), TD._data(z, "sample8m")
    sched, seed = [0.0, 0.95, 1.3], 17
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
    out, started, lps = gen.generate_stream(meta, data, sched, 32, need=6, accept=lambda s, r: True, slots=6, seed=seed,
                                            return_logprobs=True)
    assert len(out) == 6 and started >= 6
    ref = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
    ref.uniform_sources = [iter(BatchedGenerator.attempt_uniforms(seed, a, glen + 1).tolist()).__next__ for a in range(6)]
    s_ref, _, lp_ref = ref.generate([meta] * 6, [data] * 6, [sched[a % 3] for a in range(6)], 32, return_logprobs=True)
    assert out == s_ref
    for a, b in zip(lps, lp_ref):
        assert (a is None and b is None) or np.array_equal(a.view(np.int32), b.view(np.int32))
    out12, started12, lp12 = gen.generate_stream(meta, data, sched, 32, need=12, accept=lambda s, r: True, slots=6,
                                                 seed=seed, return_logprobs=True)
    assert len(gen._decoders) == 1 and len(out12) == 12 and started12 >= 12
    assert out12[:6] == out
    assert out12[6] == out12[0] and out12[9] == out12[0]
    assert len({None if s is None else tuple(s) for s in out12}) >= 4
    for a in (6, 9):
        if lp12[a] is not None:
            drawn = ~np.isnan(lp12[a][:, 0])
            assert drawn.any() and (lp12[a][drawn, 1] == 0).all()
    for a in (7, 8, 10, 11):
        if lp12[a] is not None:
            drawn = ~np.isnan(lp12[a][:, 0])
            assert (lp12[a][drawn, 1] < 0).any()


def test_log_probabilities_have_to_be_asked_for(fixture_model):
    """A decoder that was asked for neither per-slot controls nor log-probabilities runs the launches without the arrays
    (the existing decode tests run that path) and says so when log-probabilities are read; asking later drops the captured
    graph once and the same decoder then records them."""
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ForcedDecoder
    z, model = fixture_model
    dec = ForcedDecoder(model, 4, int(z["sample8m_cfg"][3]), 4146, 0.95, 32)
    uni = np.full((4, dec.ld_u), 0.5, dtype=np.float32)
    uni[:, :len(z["sample8m_uniforms"])] = z["sample8m_uniforms"]
    args = ([z["encoded_meta"].tolist()] * 4, [TD._data(z, "sample8m")] * 4, uni)
    dec.load(*args)
    with torch.no_grad():
        dec.run(use_graph=True)
    seqs = dec.sequences()[0]
    assert seqs[0] == z["sample8m_seq"].tolist() and dec.graph is not None
    assert bool(torch.isnan(dec.seq_logp).all())
    with pytest.raises(CommuHipError):
        dec.logprobs()
    dec.record_logprobs()
    assert dec.graph is None
    dec.load(*args)
    with torch.no_grad():
        dec.run(use_graph=True)
    assert dec.sequences()[0] == seqs
    lp = dec.logprobs()[0]
    assert lp.shape == (len(seqs[0]), 2) and (~np.isnan(lp[:, 0])).sum() > 20


def test_one_setting_keeps_the_scalar_launches_and_a_second_one_switches_once(fixture_model):
    """A generator given one scalar setting and no request for log-probabilities stays on the launches without the
    arrays; the same setting again keeps the capture; a second setting (the capture holds the first one's scalars) moves
    the decoder to the arrays -- one new capture -- and further settings change in place.  Every result is what a
    generator on the array launches gives for that setting."""
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    glen = int(z["sample8m_cfg"][3])
    meta, datas = [z["encoded_meta"].tolist()] * 8, [TD._data(z, "sample8m")] * 8
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
    want = {}
    for temp, top_k in ((0.95, 32), (0.6, 32), (1.2, 12)):
        ref = BatchedGenerator(model, torch.device(DEV), generation_length=glen)
        want[(temp, top_k)] = ref.generate(meta, datas, temp, top_k, return_logprobs=True)[0]
        assert next(iter(ref._decoders.values())).rows_on
    assert gen.generate(meta, datas, 0.95, 32)[0] == want[(0.95, 32)]
    dec = next(iter(gen._decoders.values()))
    g0 = dec.graph
    assert not dec.rows_on and g0 is not None
    assert gen.generate(meta, datas, 0.95, 32)[0] == want[(0.95, 32)] and dec.graph is g0 and not dec.rows_on
    assert gen.generate(meta, datas, 0.6, 32)[0] == want[(0.6, 32)]
    g1 = dec.graph
    assert dec.rows_on and g1 is not None and g1 is not g0 and len(gen._decoders) == 1
    assert gen.generate(meta, datas, 1.2, 12)[0] == want[(1.2, 12)] and dec.graph is g1
    assert gen.generate(meta, datas, 0.95, 32)[0] == want[(0.95, 32)] and dec.graph is g1
