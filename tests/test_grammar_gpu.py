"""The event grammar on the GPU: the sampling kernel with a grammar table (commu_sample_args.gram) against the numpy
restatement (grammar_contract.restate_with_grammar: (x + bias) + gram[class of the previous token]) and against the
launches without one, bit for bit; then through the decode loop (fused launch, captured graph, separate launches, fp32
parity), in-place switching, primed slots, the single-request API, one cache combination and the CLI's --help."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grammar_contract as GC  # noqa: E402
import test_decode_gpu as TD  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
from sample_launch import sample_launch  # noqa: E402

DEV = "cuda"
V = 729
NEG = float("-inf")
LOGP_TOL = SR.LOGP_TOL          # (the restatement is fed y as fp32 rounds it: the added operation brings no new error)
bits = SR.bits
N = 16
# previous tokens of the 16 kernel rows: every class and both ends of every id range
PREV = [0, 1, 2, 3, 130, 131, 194, 195, 303, 304, 431, 432, 559, 560, 728, 60]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def records(prev):
    """Forcing records and seq rows whose last token is prev[b] (lengths 5, 6, 7, ...; a decoy behind the last token)."""
    from commu_amd._lib import call
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(len(prev), nf, dtype=torch.int32)
    seq = torch.full((len(prev), 12), 600, dtype=torch.int32)
    for b, t in enumerate(prev):
        n = 5 + b % 3
        st[b, 0] = n
        seq[b, n - 1] = t
        seq[b, n] = 432 if GC.token_class(t) != GC.POSITION else 2
    return st, seq


def launch(r, bias=None, gram=None, on=None, wrong=None, ld_gram=None, state=True):
    """One launch on fresh device copies of the 16 rows (sample_launch); state=False: null record and seq pointers (the
    row stride of seq is still passed)."""
    return sample_launch(r["logits"], r["wrong"] if wrong is None else wrong, r["us"], r["t"], r["k"], r["p"], bias=bias,
                         gram=gram, ld_gram=ld_gram, gram_on=on, state=r["state"] if state else None,
                         seq=r["seq"] if state else None, ld_seq=r["seq"].stride(0))


@pytest.fixture(scope="module")
def rows():
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    bias, kind = LBG.bias_rows(logits)
    st, seq = records(PREV)
    assert {GC.token_class(x) for x in PREV} == set(range(7))
    return dict(logits=logits[:N].contiguous(), wrong=wrong[:N].contiguous(), us=us[:N].contiguous(), t=t[:N].contiguous(),
                k=k[:N].contiguous(), p=p[:N].contiguous(), bias=bias[:N].contiguous(), kind=kind[:N], state=st, seq=seq)


def custom_table():
    """Finite entries everywhere (|g| <= 4), and -2^20 on the duration ids, which a bias of +2^20 there cancels only when
    the adds are made in the documented order: (x + 2^20) - 2^20 keeps x to 1/8, x + (2^20 - 2^20) keeps all of it."""
    g = torch.Generator().manual_seed(37)
    t = torch.rand(8, 768, generator=g) * 8 - 4
    t[:7, 304:432] = -float(2 ** 20)
    t[7] = 0
    return t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check(r, out, bias, gram, on=None, wrong=None):
    lg, tok, pr, lp = out
    worst = [0.0, 0.0, 0.0]
    refs = []
    for b in range(N):
        res = GC.restate_with_grammar(r["logits"][b].numpy(), float(r["t"][b]), int(r["k"][b]), float(r["p"][b]),
                                      (r["wrong"] if wrong is None else wrong)[b].numpy(),
                                      None if bias is None else bias[b].numpy(), float(r["us"][b]),
                                      gram=np.asarray(gram, dtype=np.float32), prev=PREV[b], on=on is None or bool(on[b]))
        refs.append(res)
        assert np.array_equal(lg[b].numpy().view(np.int32), res.written[:V].view(np.int32)), b
        if res.token < 0:
            assert int(tok[b]) == -1 and bool(torch.isnan(lp[b]).all()) and bool(torch.isnan(pr[b]).all()), b
            continue
        got = pr[b].double().numpy()
        tb = int(tok[b])
        assert ((got > 0) == (res.probs > 0)).all(), b
        assert bool((got[res.y == NEG] == 0.0).all()), b                 # banned ids: exactly 0
        assert tb == res.token or abs(np.cumsum(res.probs)[min(tb, res.token)] - float(r["us"][b])) < 1e-5, b
        assert res.probs[tb] > 0, b
        worst[0] = max(worst[0], np.abs(got - res.probs).max())
        worst[1] = max(worst[1], abs(float(lp[b, 0]) - res.full[tb]))
        worst[2] = max(worst[2], abs(float(lp[b, 1]) - (0.0 if float(r["t"][b]) == 0 else np.log(res.probs[tb]))))
    print("max |probs - float64|, |full - float64|, |kept - log p|:", worst)
    assert max(worst) <= LOGP_TOL, worst
    return refs


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_separate_sampler_against_the_restatement(rows):
    from commu_amd.generate import event_grammar
    default = torch.from_numpy(event_grammar())
    free = launch(rows, state=False)
    for bias in (None, rows["bias"]):
        out = launch(rows, bias=bias, gram=default)
        refs = check(rows, out, bias, default)
        assert torch.equal(bits(out[0]), bits(free[0]))                  # the written-back logits: the unconstrained call's
        for b in range(N):
            if int(out[1][b]) >= 0:                                      # the drawn token continues its group
                allowed = np.isfinite(GC.default_table()[GC.token_class(PREV[b]), :V])
                assert allowed[int(out[1][b])], b
        assert sum(1 for x in refs if x.token >= 0) >= 10
    assert not torch.equal(launch(rows, gram=default)[1], free[1])
    # a finite table with a user bias: pins the add order
    table = custom_table()
    big = rows["bias"].clone()
    big[big == NEG] = -3.0
    big[:, 304:432] = float(2 ** 20)
    out = launch(rows, bias=big, gram=table)
    refs = check(rows, out, big, table)
    assert torch.equal(bits(out[0]), bits(free[0]))
    assert sum(1 for x in refs if x.token >= 0 and x.probs[304:432].sum() > 0) >= 4      # (the cancelled ids carry mass)
    # slots that are off read row 7
    on = torch.tensor([b % 2 for b in range(N)], dtype=torch.uint8)
    check(rows, launch(rows, bias=rows["bias"], gram=default, on=on), rows["bias"], default, on=on)
    # grammar + rejected tokens leave nothing: after a pitch (row 15) only durations may follow, and all are rejected
    wrong = rows["wrong"].clone()
    wrong[15, 304:432] = 1
    out = launch(rows, gram=default, wrong=wrong)
    assert int(out[1][15]) == -1 and bool(torch.isnan(out[3][15]).all())
    check(rows, out, None, default, wrong=wrong)


# ------------------------------------------------------------------------------------------------ 2. grammar off
def test_grammar_off_is_the_bias_entry_point_bit_for_bit(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError, call
    from commu_amd.generate import event_grammar
    default = torch.from_numpy(event_grammar())
    off = torch.zeros(N, dtype=torch.uint8)
    for bias in (None, rows["bias"]):
        # (`old`, no grammar and no record / seq pointers, is what the entry point without a grammar argument and the one
        # with gram == null and no state were: one call now)
        old = launch(rows, bias=bias, state=False)
        assert same(old, launch(rows, bias=bias, gram=default, on=off))
        assert same(old, launch(rows, bias=bias, gram=None))
    assert int((old[1] >= 1).sum()) >= 8
    # refusals of the C entry point: a short row stride, a grammar without the record / seq
    for kw in (dict(ld_gram=700), dict(state=False)):
        with pytest.raises(CommuHipError, match="-22"):
            launch(rows, gram=default, **kw)
    # ops.sample_topk(grammar=) is the same launch
    lg = rows["logits"].clone().to(DEV)
    tok = ops.sample_topk(lg, rows["t"].to(DEV), rows["k"].to(DEV), wrong=rows["wrong"].to(DEV), uniforms=rows["us"].to(DEV),
                          top_p=rows["p"].to(DEV), grammar=(default.to(DEV), None, rows["state"].to(DEV), rows["seq"].to(DEV)))
    assert torch.equal(tok.cpu(), launch(rows, gram=default)[1])
    with pytest.raises(CommuHipError, match="grammar table"):
        ops.sample_topk(lg, 0.95, 32, grammar=(default, None, rows["state"].to(DEV), rows["seq"].to(DEV)))
    assert call("commu_forcing_state_ints") == rows["state"].shape[1]


# ------------------------------------------------------------------------------------------------ 3. through the loop
GLEN = 96


@pytest.fixture(scope="module")
def fixture_model(golden_dir):
    z = TD.load(golden_dir, "g6_decode.npz")
    return z, TD._build(golden_dir, z, z["sample8m_bias"])


def variates(B, n):
    return np.random.RandomState(11).random_sample((B, n)).astype(np.float32)


def loaded(z, model, B, on=None, table=True, max_prompt=0, prompts=None, **kw):
    """B slots of the margin fixture's request, log-probabilities recorded; on: None (a decoder that never heard of the
    grammar) or the slots whose grammar is on."""
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, B, GLEN, 4146, 0.95, 32, max_prompt=max_prompt, **kw)
    dec.record_logprobs()
    if on is not None:
        dec.set_grammar(table, rows=on)
    reload(z, dec, prompts)
    return dec


def reload(z, dec, prompts=None):
    uni = variates(dec.B, dec.ld_u)
    dec.load([z["encoded_meta"].tolist()] * dec.B, [TD._data(z, "sample8m")] * dec.B, uni, prompts=prompts)
    return uni


run, separate_launches = LBG.run, LBG.separate_launches


def well_formed(z, seq):
    from commu_amd.midi_generator.midi_inferrer import parse_events
    n_ctx = 1 + len(z["encoded_meta"])
    a, b = parse_events(seq, n_ctx), GC.parse_events(seq, n_ctx)
    assert a == b, seq
    return a is None


def check_on_slot(z, seq):
    from commu_amd.midi_generator.midi_inferrer import count_notes
    assert seq is not None and well_formed(z, seq), seq
    chords = [t for t in seq if 195 <= t <= 303]
    assert len(chords) >= 1 and chords == z["sample8m_chord_token"].tolist()[:len(chords)]
    assert count_notes(seq) > 0


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_alternating_slots_through_the_loop(fixture_model, parity, B):
    """Slots alternate on / off.  Graph replay == eager == separate launches (seq, records, seq_logp bit patterns); the
    on-slots are well formed, keep their forced chords and hold notes; the off-slots decode bit for bit what a decoder
    that never heard of the grammar decodes, and that is malformed (the fixture model's free run is bars, positions and
    forced chords)."""
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        plain = loaded(z, model, B)
        assert plain.gram is None
        s0, f0, l0 = run(plain)
        free_seqs = plain.sequences()[0]
        on = list(range(0, B, 2))
        res = []
        for mode in ("graph", "eager", "separate"):
            dec = loaded(z, model, B, on=on)
            assert dec.state.parity == parity and dec.gram is not None and dec.gram_on.tolist() == [1, 0] * (B // 2)
            if mode == "separate":
                res.append(separate_launches(dec, dec.generation_length + 1))
            else:
                res.append(run(dec, use_graph=mode == "graph"))
            if mode == "graph":
                assert dec.graph is not None
                seqs = dec.sequences()[0]
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert torch.equal(bits(res[0][2]), bits(other[2]))
        sg, fg, lg = res[0]
        for b in range(B):
            if b in on:
                check_on_slot(z, seqs[b])
            else:
                assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
        assert any(s is not None and not well_formed(z, s) for b, s in enumerate(free_seqs) if b not in on)
    finally:
        model.parity_fp32 = False


# ------------------------------------------------------------------------------------------------ 4. in place
def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, on=[1])
    assert dec.graph is None
    run(dec)
    g = dec.graph
    first = dec.sequences()[0]
    assert g is not None
    check_on_slot(z, first[1])
    assert torch.equal(dec.seq[0], s0[0]) and torch.equal(dec.seq[2], s0[2])
    dec.set_grammar(None, rows=[1])
    dec.set_grammar(True, rows=[2])
    uni = reload(z, dec)
    dec.rearm(3, uni[3], grammar=True)
    s, f, l = run(dec)
    assert dec.graph is g and dec.gram_on.tolist() == [0, 0, 1, 1]
    second = dec.sequences()[0]
    check_on_slot(z, second[2])
    check_on_slot(z, second[3])
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], grammar=False)
    dec.set_grammar(None)
    reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and not bool(dec.gram_on.any())
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


# ------------------------------------------------------------------------------------------------ 5. primed slots
def test_a_primed_slots_first_draw_is_keyed_by_the_last_prompt_token(fixture_model):
    z, model = fixture_model
    src = loaded(z, model, 2, on=[0, 1])
    run(src)
    seq = src.sequences()[0][0]
    n_ctx = 1 + len(z["encoded_meta"])
    body = seq[n_ctx:]
    cls = [GC.token_class(t) for t in body]
    i = next(j for j in range(len(body) - 1) if cls[j] == GC.POSITION and cls[j + 1] == GC.VELOCITY)
    prompts = [body[:i + 1], body[:i + 2], body[:i + 3]]                # ... position | velocity | pitch
    dec = loaded(z, model, 3, on=[0, 1, 2], max_prompt=len(prompts[2]), prompts=prompts)
    run(dec)
    got, lps = dec.sequences()[0], dec.logprobs()
    for b, want in enumerate((GC.VELOCITY, GC.PITCH, GC.DURATION)):
        cut = n_ctx + len(prompts[b])
        assert got[b][:cut] == seq[:cut]
        drawn = ~np.isnan(lps[b][:, 0])
        assert not drawn[:cut].any() and drawn[cut], b                    # the first token after the prompt is a draw
        assert GC.token_class(got[b][cut]) == want, b
        assert well_formed(z, got[b])


# ------------------------------------------------------------------------------------------------ 6. one request
def test_generate_stream_returns_the_same_attempts_at_2_and_8_slots(fixture_model):
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    meta, data = z["encoded_meta"].tolist(), TD._data(z, "sample8m")
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN)
    outs = [gen.generate_stream(meta, data, 0.95, 32, need=8, accept=lambda s, r: True, slots=n, grammar=True)[0]
            for n in (2, 8)]
    assert outs[0] == outs[1] and len(outs[0]) == 8
    for s in outs[0]:
        assert s is not None and well_formed(z, s)
    assert len({tuple(s) for s in outs[0]}) > 1
    # a request without grammar= clears what the one before left on the reused decoder
    after = gen.generate_stream(meta, data, 0.95, 32, need=8, accept=lambda s, r: True, slots=8)[0]
    fresh = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN).generate_stream(
        meta, data, 0.95, 32, need=8, accept=lambda s, r: True, slots=8)[0]
    assert after == fresh and len(gen._decoders) == 2
    assert any(s is not None and not well_formed(z, s) for s in after)
    # generate(grammar=[bool per sequence])
    seqs, _ = gen.generate([meta] * 8, [data] * 8, 0.95, 32, grammar=[True, False] * 4)
    for b, s in enumerate(seqs):
        if b % 2 == 0:
            assert s is not None and well_formed(z, s), b


# ------------------------------------------------------------------------------------------------ 7. another cache
def test_fp8_sliding_cache_feeds_the_same_stage():
    """kv_dtype="fp8" with a sliding memory of 32 that wraps: the sampling stage does not care which cache produced the
    logits.  Graph replay == eager, every slot well formed, notes in every slot."""
    import test_kv8_gpu as K8
    from commu_amd.generate import ForcedDecoder
    from commu_amd.midi_generator.midi_inferrer import count_notes, parse_events
    model, data = K8._loop_model(32)
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)
    dec = ForcedDecoder(model, 4, generation_length=64, memory_length=32, temperature=0.95, top_k=32, sliding=True,
                        kv_dtype="fp8")
    dec.set_grammar(True)
    outs = []
    for graph in (False, True):
        dec.load([K8.META] * 4, [data] * 4, uni)
        with torch.no_grad():
            dec.run(use_graph=graph)
        torch.cuda.synchronize()
        outs.append(dec.sequences()[0])
    assert dec.state.kv_dtype == "fp8" and dec.graph is not None and outs[0] == outs[1]
    for s in outs[0]:
        assert len(s) > 12 + 40 and parse_events(s, 1 + len(K8.META)) is None and count_notes(s) >= 10


# ------------------------------------------------------------------------------------------------ 8. CLI
def test_cli_help_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "commu-code_amd", "generate.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--grammar" in out.stdout
