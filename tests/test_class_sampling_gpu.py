"""Class-keyed sampling on the GPU.  The defining property: a draw with control record (t, k, p) is bit for bit the draw
the array-mode harmony kernel makes for a sequence whose temperature_rows / top_k_rows / top_p_rows hold (t, k, p) -- so the
sampler tests need no tolerance: the new kernel (commu_sample_args.cls_ctl) against the existing one through
tests/sample_launch.py, once and compounding (Q5); the fused launch against the separate ones; then through the decode
loop (captured graph, in-place switching, rearm, the single-request API, fp32 parity, the fp8 sliding cache) and the
refusals of the entry point."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import class_sampling_contract as CS  # noqa: E402
import grammar_contract as GC  # noqa: E402
import test_decode_gpu as TD  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
from sample_launch import sample_launch  # noqa: E402

DEV = "cuda"
V = 729
N = 16
bits = SR.bits
# previous token of sequence b: both edges of every class's id range; sequence 13 has F_LEN 0 (the clamp reads seq[b][0])
PREV = [2, 3, 130, 131, 194, 195, 303, 304, 431, 432, 559, 560, 728, 140, 1, 440]
ZERO_LEN = 13
# the records: greedy | top_k 1 | top_k V | top_p 0.5 | ...; neighbours (cyclically) differ in their temperature and none
# is 1.0, so whichever neighbour a draw took by mistake the logits it writes back differ (x / t for two different t, or x / t
# against the untouched row of a greedy draw)
RECORDS = [(0.0, 32, 1.0), (0.7, 1, 1.0), (1.3, V, 1.0), (0.9, 32, 0.5), (1.2, 16, 0.9), (1.1, 40, 1.0), (0.8, 8, 0.7)]
POISON = (5.0, 3, 0.3)          # row 7 and the scalars of a cls_ctl launch: never looked at


def table_of(b):
    """Sequence b's table: class c holds RECORDS[(c + b) % 7], row 7 the poison."""
    return [RECORDS[(c + b) % 7] for c in range(7)] + [POISON]


def ctl_words(tables):
    from commu_amd.generate import CLASS_CTL_DTYPE
    rec = np.zeros((len(tables), 8), dtype=CLASS_CTL_DTYPE)
    for b, t in enumerate(tables):
        for c, (tt, k, p) in enumerate(t):
            rec[b, c] = (tt, k, p, 0)
    return torch.from_numpy(rec.view(np.int32).reshape(len(tables), 8, 4))


@pytest.fixture(scope="module")
def rows():
    from commu_amd._lib import call
    from commu_amd.generate import event_grammar, harmony_table
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(N, V, generator=g) * 2.5
    us = torch.rand(N, generator=g)
    wrong = torch.zeros(N, V, dtype=torch.uint8)
    wrong[::5, 64] = 1
    bias, _ = LBG.bias_rows(logits)
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(N, nf, dtype=torch.int32)
    seq = torch.full((N, 12), 600, dtype=torch.int32)
    ct = torch.full((N, 4), 250, dtype=torch.int32)
    for b in range(N):
        body = [600, 2, 432, 199, 440, 150, PREV[b]]
        if b == ZERO_LEN:
            body = [PREV[b]]
        seq[b, :len(body)] = torch.tensor(body, dtype=torch.int32)
        seq[b, len(body)] = 310                                         # behind the end of seq: not the key
        st[b, 0] = 0 if b == ZERO_LEN else len(body)
        st[b, 10] = 1                                                   # F_CUR: one chord placed, Chord_am
        ct[b, 0] = 199
    cls = [GC.token_class(p) for p in PREV]
    assert set(cls) == set(range(7)) and len(PREV) == N
    return dict(logits=logits, us=us, wrong=wrong, bias=bias[:N].contiguous(), state=st, seq=seq, chord_tok=ct, cls=cls,
                gram=torch.from_numpy(event_grammar()), gram_on=torch.tensor([b % 2 for b in range(N)], dtype=torch.uint8),
                harm=torch.from_numpy(harmony_table()),
                harm_on=torch.tensor([(b // 2) % 2 for b in range(N)], dtype=torch.uint8),
                ctl=ctl_words([table_of(b) for b in range(N)]))


def triples(r, shift=0):
    """The three *_rows arrays holding each sequence's record of class (c + shift) mod 7."""
    sel = [table_of(b)[(r["cls"][b] + shift) % 7] for b in range(N)]
    return (torch.tensor([s[0] for s in sel], dtype=torch.float32), torch.tensor([s[1] for s in sel], dtype=torch.int32),
            torch.tensor([s[2] for s in sel], dtype=torch.float32))


def existing(r, logits, shift=0):
    """Today's harmony kernel with the selected triples in the arrays (tests/sample_launch.py)."""
    t, k, p = triples(r, shift)
    return sample_launch(logits, r["wrong"], r["us"], t, k, p, bias=r["bias"], gram=r["gram"], gram_on=r["gram_on"],
                         harm=r["harm"], harm_on=r["harm_on"], state=r["state"], seq=r["seq"], chord_tok=r["chord_tok"])


def cls_launch(r, logits, ctl=None, offset=0, **null):
    """One launch of commu_sample_topk with cls_ctl on fresh device copies (as sample_launch makes them: token -7,
    probs_out -3.0, logp_out 7.0 before the launch); the scalars hold the poison triple and the arrays are null.  null:
    names of pointers to pass as null; offset: bytes added to the cls_ctl pointer."""
    from commu_amd._lib import SampleArgs, call, struct_args
    d = lambda x: x.to(DEV).contiguous()
    ptr = lambda x, name=None: None if null.get(name) else C.c_void_p(x.data_ptr())
    lg = logits.clone().to(DEV)
    pr = torch.full((N, V), -3.0, device=DEV)
    tok = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((N, 2), 7.0, device=DEV)
    h = {k: d(r[k]) for k in ("wrong", "us", "bias", "gram", "gram_on", "harm", "harm_on", "state", "seq", "chord_tok")}
    words = torch.zeros(N * 32 + 8, dtype=torch.int32, device=DEV)       # (room for a misaligned copy)
    words[offset // 4:offset // 4 + N * 32] = d(r["ctl"] if ctl is None else ctl).view(-1)
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=N, V=V, wrong=ptr(h["wrong"]), ldw=V, uniforms=ptr(h["us"]),
        temperature=POISON[0], top_k=POISON[1], top_p=POISON[2], token=ptr(tok), probs_out=ptr(pr), ldp=V, logp_out=ptr(lp),
        bias=ptr(h["bias"], "bias"), ld_bias=h["bias"].stride(0), gram=ptr(h["gram"], "gram"), ld_gram=h["gram"].stride(0),
        gram_on=ptr(h["gram_on"]), harm=ptr(h["harm"], "harm"), ld_harm=h["harm"].stride(0), harm_on=ptr(h["harm_on"]),
        state=ptr(h["state"], "state"), seq=ptr(h["seq"], "seq"), ld_seq=0 if null.get("ld_seq") else h["seq"].stride(0),
        chord_tok=ptr(h["chord_tok"], "chord_tok"), ld_chord=h["chord_tok"].stride(0),
        cls_ctl=C.c_void_p(words.data_ptr() + offset))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()


def same_row(a, b, i):
    """Outputs (logits, token, probs_out, logp_out) of sequence i equal bit for bit; NaN equals NaN (the Q12 pair)."""
    def eq(x, y):
        if not x.is_floating_point():
            return bool((x == y).all())
        return bool(((bits(x) == bits(y)) | (torch.isnan(x) & torch.isnan(y))).all())
    return all(eq(x[i], y[i]) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. / 2. the sampler
def test_sampler_equals_the_existing_kernel_bit_for_bit_and_compounds(rows):
    """Fails on the parent: commu_sample_args has no cls_ctl."""
    got = cls_launch(rows, rows["logits"])
    want = existing(rows, rows["logits"])
    wrong_class = existing(rows, rows["logits"], shift=1)
    for b in range(N):
        assert same_row(got, want, b), (b, PREV[b], got[1][b], want[1][b])
        assert not same_row(got, wrong_class, b), (b, PREV[b])          # teeth: the neighbouring class's record shows
    assert int((got[1] >= 1).sum()) >= 12 and len({int(t) for t in got[1]}) > 4
    greedy = [b for b in range(N) if table_of(b)[rows["cls"][b]][0] == 0.0]
    assert greedy and all(float(got[3][b, 1]) == 0.0 and torch.equal(got[0][b], rows["logits"][b]) for b in greedy)
    # Q5: the same two calls again on the logits the first ones left -- the class temperature compounds
    got2 = cls_launch(rows, got[0])
    want2 = existing(rows, want[0])
    for b in range(N):
        assert same_row(got2, want2, b), (b, PREV[b])
        t = np.float32(table_of(b)[rows["cls"][b]][0])
        if t != 0:
            twice = (rows["logits"][b, 1:].numpy() / t) / t
            assert np.array_equal(got2[0][b, 1:].numpy().view(np.int32), twice.astype(np.float32).view(np.int32)), b
    # a table whose every record is one triple is the array-mode call with that triple, whatever the class
    flat = ctl_words([[RECORDS[4]] * 7 + [POISON]] * N)
    t, k, p = (torch.full((N,), x, dtype=dt) for x, dt in zip(RECORDS[4], (torch.float32, torch.int32, torch.float32)))
    ref = sample_launch(rows["logits"], rows["wrong"], rows["us"], t, k, p, bias=rows["bias"], gram=rows["gram"],
                        gram_on=rows["gram_on"], harm=rows["harm"], harm_on=rows["harm_on"], state=rows["state"],
                        seq=rows["seq"], chord_tok=rows["chord_tok"])
    out = cls_launch(rows, rows["logits"], ctl=flat)
    assert all(same_row(out, ref, b) for b in range(N))


def test_ops_sample_topk_makes_the_all_off_tables_it_needs(rows):
    from commu_amd import ops
    d = lambda x: x.to(DEV)
    lg = d(rows["logits"].clone())
    tok = ops.sample_topk(lg, POISON[0], POISON[1], wrong=d(rows["wrong"]), uniforms=d(rows["us"]), top_p=POISON[2],
                          class_ctl=(d(rows["ctl"]), d(rows["state"]), d(rows["seq"])))
    t, k, p = triples(rows)
    ref = sample_launch(rows["logits"], rows["wrong"], rows["us"], t, k, p)           # no constraint at all
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_entry_point_refusals(rows):
    from commu_amd._lib import CommuHipError
    for kw in (dict(gram=True), dict(harm=True), dict(bias=True), dict(state=True), dict(seq=True), dict(chord_tok=True),
               dict(ld_seq=True), dict(offset=4), dict(offset=8)):
        with pytest.raises(CommuHipError, match="-22"):
            cls_launch(rows, rows["logits"], **kw)
    cls_launch(rows, rows["logits"], offset=16)                         # 16-byte aligned: accepted


# ------------------------------------------------------------------------------------------------ 3. fused == separate
B3, GLEN3, ITERS3 = 3, 6, 6


@pytest.fixture(scope="module")
def fixture_model(golden_dir):
    z = TD.load(golden_dir, "g6_decode.npz")
    return z, TD._build(golden_dir, z, z["sample8m_bias"])


def test_separate_launches_and_the_fused_launch_agree(fixture_model):
    """test_decode_loop_args_gpu's comparison for the new selector: two host paths fill two structs."""
    from commu_amd.generate import ForcedDecoder, class_sampling, token_constraints
    z, model = fixture_model

    def decoder():
        dec = ForcedDecoder(model, B3, GLEN3, 4146, 0.95, 32)
        dec.set_logit_bias(token_constraints(ban=[1], bias={i: 8.0 for i in range(3, 131)}))
        dec.set_grammar(True, rows=[0, 1])
        # after OTHER (the meta tokens: every slot's first draw), BAR and POSITION the controls are the table's
        dec.set_class_sampling(class_sampling(after={"other": {"temperature": 1.3, "top_k": 5}, "bar": {"top_p": 0.6},
                                                     "position": {"temperature": 0}, "pitch": {"top_k": 2}}), rows=[0, 2])
        assert dec.cls_ctl is not None and dec.harm is not None and dec.rows_on
        uni = np.random.RandomState(5).random_sample((B3, dec.ld_u)).astype(np.float32)
        dec.load([z["encoded_meta"].tolist()] * B3, [TD._data(z, "sample8m")] * B3, uni)
        return dec
    with torch.no_grad():
        sep = decoder()
        sep_tokens = []
        for _ in range(ITERS3):
            sep.iteration()
            sep_tokens.append(sep.token.clone())
        sep.pre()
        fused = decoder()
        fused_tokens = []
        fused.pre()
        for _ in range(ITERS3):
            fused.body_pre()
            fused_tokens.append(fused.token.clone())
    torch.cuda.synchronize()
    sep_tokens, fused_tokens = torch.stack(sep_tokens).cpu(), torch.stack(fused_tokens).cpu()
    assert torch.equal(sep_tokens, fused_tokens), (sep_tokens, fused_tokens)
    assert torch.equal(sep.fsm, fused.fsm) and torch.equal(sep.seq, fused.seq)
    assert torch.equal(bits(sep.seq_logp), bits(fused.seq_logp))
    assert torch.equal(bits(sep.state.logits), bits(fused.state.logits))
    assert torch.equal(sep.state.klen, fused.state.klen)
    assert int((sep_tokens >= 1).sum()) >= ITERS3 and int(sep.fsm[:, 0].min()) > 1 + len(z["encoded_meta"])
    # the table shows: slot 1 (no override) draws its first token with top_k 32, slot 0 / 2 with temperature 1.3
    lp = sep.seq_logp.cpu()
    first = 1 + len(z["encoded_meta"])
    assert not torch.equal(bits(lp[0, first]), bits(lp[1, first]))


# ------------------------------------------------------------------------------------------------ 4. / 7. through the loop
GLEN = 40
run, draws = LBG.run, LBG.draws


def loop_decoder(model, B, on=None, table=None, memory_length=4146, **kw):
    """B slots, grammar on, log-probabilities recorded, base T 0.95 / k 32, the bar lowered (HG.NOTES) so that the untrained
    model draws notes; on: None (a decoder that never received a table) or the slots that carry `table`."""
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, B, GLEN, memory_length, 0.95, 32, max_prompt=len(HG.PRIME), **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES))
    if on is not None:
        dec.set_class_sampling(table, rows=on)
    return dec


def duration_and_other_draws(dec, slots):
    """(kept of every appended draw whose previous token is a pitch, kept of the other appended draws) over `slots`."""
    lps = dec.logprobs()
    dur, other = [], []
    for b in slots:
        seq, drawn = draws(dec)[b]
        assert seq is not None, b
        for i in np.flatnonzero(drawn):
            (dur if GC.token_class(seq[i - 1]) == GC.PITCH else other).append(float(lps[b][i, 1]))
            if GC.token_class(seq[i - 1]) == GC.PITCH:
                assert 304 <= seq[i] <= 431, (b, i)                     # (the grammar: a duration follows a pitch)
    return dur, other


def check_greedy_durations(load, make, B):
    """Even slots carry {"duration": {"temperature": 0}}, odd slots no override.  Every duration draw of an even slot has
    kept == 0.0 exactly, the other draws are sampled; the odd slots decode token for token, and seq_logp bit for bit, what a
    decoder that never received a table decodes with the same variates."""
    from commu_amd.generate import class_sampling
    plain = make(None, None)
    load(plain)
    s0, f0, l0 = run(plain)
    assert plain.cls_ctl is None and plain.harm is None
    on = list(range(0, B, 2))
    dec = make(on, class_sampling(drawn={"duration": {"temperature": 0}}))
    load(dec)
    s, f, l = run(dec)
    assert dec.graph is not None and dec.cls_ctl is not None
    dur, other = duration_and_other_draws(dec, on)
    print("duration draws:", len(dur), "other draws:", len(other), "sampled among the others:", sum(k < 0 for k in other))
    assert len(dur) >= 10 and len(other) >= 10                          # (a condition of the test, not a measurement)
    assert all(k == 0.0 for k in dur)
    assert any(k < 0 for k in other)
    pdur, _ = duration_and_other_draws(plain, on)
    assert any(k < 0 for k in pdur)                                     # (the twin samples its durations: the table bit)
    for b in range(1, B, 2):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    return dec


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_greedy_durations_through_the_loop(fixture_model, parity, B):
    z, model = fixture_model
    model.parity_fp32 = parity
    try:
        uni = HG.variates(B, GLEN + 1)

        def load(dec):
            dec.load([z["encoded_meta"].tolist()] * B, [TD._data(z, "sample8m")] * B, uni, prompts=[HG.PRIME] * B)
        dec = check_greedy_durations(load, lambda on, table: loop_decoder(model, B, on, table), B)
        assert dec.state.parity == parity
    finally:
        model.parity_fp32 = False


def test_fp8_sliding_cache_feeds_the_same_stage():
    import test_kv8_gpu as K8
    model, _ = K8._loop_model(32)
    with torch.no_grad():
        model.crit.out_layers[0].bias[2] = 3.0                           # bars again, as in the fixture (HG's fp8 test)
    chords = [199, 285, 267, 258]
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": chords, "chord_position": [432] * 4})
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)

    def load(dec):
        dec.load([K8.META] * 4, [data] * 4, uni, prompts=[HG.PRIME] * 4)
    dec = check_greedy_durations(
        load, lambda on, table: loop_decoder(model, 4, on, table, sliding=True, kv_dtype="fp8", memory_length=32), 4)
    assert dec.state.kv_dtype == "fp8" and dec.sliding and int(dec.state.klen.max()) > 32      # the ring wrapped


# ------------------------------------------------------------------------------------------------ 5. in place
def device_records(dec):
    from commu_amd.generate import CLASS_CTL_DTYPE
    return dec.cls_ctl.cpu().numpy().view(CLASS_CTL_DTYPE).reshape(dec.B, 8)


def test_switching_in_place_under_one_capture(fixture_model):
    from commu_amd.generate import class_sampling
    z, model = fixture_model
    B = 4
    uni = HG.variates(B, GLEN + 1)

    def load(dec):
        dec.load([z["encoded_meta"].tolist()] * B, [TD._data(z, "sample8m")] * B, uni, prompts=[HG.PRIME] * B)
    plain = loop_decoder(model, B)
    load(plain)
    s0, f0, l0 = run(plain)
    table = class_sampling(drawn={"duration": {"temperature": 0}, "pitch": {"top_k": 40, "temperature": 1.2}})
    dec = loop_decoder(model, B, list(range(B)), table)
    assert dec.graph is None
    load(dec)
    s1, f1, l1 = run(dec)
    g = dec.graph
    assert g is not None and not torch.equal(s1, s0)
    dec.set_class_sampling(None)                                        # every record the base triple
    load(dec)
    s, f, l = run(dec)
    assert dec.graph is g
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))
    dec.set_class_sampling(table)                                       # and back
    load(dec)
    s, f, l = run(dec)
    assert dec.graph is g
    assert torch.equal(s, s1) and torch.equal(f, f1) and torch.equal(bits(l), bits(l1))
    # rearm(sampling=) recomposes the inherited records of its slot and keeps the override
    dec.set_class_sampling(class_sampling(drawn={"pitch": {"top_k": 40}}), rows=[2])
    dec.rearm(2, uni[2], sampling=(0.5, 8, 1.0))
    rec = device_records(dec)
    vel = CS.NAMES.index("velocity")                                    # a pitch is drawn after a velocity
    assert rec[2][vel].tolist() == (0.5, 40, 1.0, 0)
    assert all(rec[2][c].tolist() == (0.5, 8, 1.0, 0) for c in range(8) if c != vel)
    assert rec[1][vel].tolist() == (np.float32(1.2), 40, 1.0, 0) and rec[1][7].tolist() == (np.float32(0.95), 32, 1.0, 0)
    assert dec.graph is g


# ------------------------------------------------------------------------------------------------ 6. one request
def test_generate_stream_returns_the_same_attempts_at_2_and_8_slots(fixture_model):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import BatchedGenerator
    z, model = fixture_model
    meta, data = z["encoded_meta"].tolist(), TD._data(z, "sample8m")
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN)
    kw = dict(need=8, accept=lambda s, r: True, logit_bias=HG.steer_row(HG.NOTES), return_logprobs=True, grammar=True)
    cs = {"drawn": {"duration": {"temperature": 0}, "pitch": {"temperature": 1.1, "top_k": 40}}}
    outs = [gen.generate_stream(meta, data, 0.95, 32, slots=n, class_sampling=cs, **kw) for n in (2, 8)]
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) == 8 and len({tuple(s) for s in outs[0][0]}) > 1
    n_dur = 0
    for s, lp in zip(outs[0][0], outs[0][2]):
        for i in np.flatnonzero(~np.isnan(lp[:, 0])):
            if GC.token_class(s[i - 1]) == GC.PITCH:
                assert float(lp[i, 1]) == 0.0
                n_dur += 1
    assert n_dur >= 10
    # a request without class_sampling= resets what the one before left on the reused decoder
    after = gen.generate_stream(meta, data, 0.95, 32, slots=8, **kw)
    fresh = BatchedGenerator(model, torch.device(DEV), generation_length=GLEN).generate_stream(meta, data, 0.95, 32, slots=8, **kw)
    assert after[0] == fresh[0] and after[0] != outs[1][0]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(after[2], fresh[2]))
    with pytest.raises(CommuHipError, match=r"top_k: an integer in \[1, 729\) expected"):
        gen.generate_stream(meta, data, 0.95, 32, slots=8, class_sampling={"drawn": {"pitch": {"top_k": 729}}}, **kw)
    seqs, _ = gen.generate([meta] * 4, [data] * 4, 0.0, 32, grammar=True, class_sampling=cs, logit_bias=HG.steer_row(HG.NOTES))
    assert all(s is not None for s in seqs) and len({tuple(s) for s in seqs}) > 1      # greedy base, sampled pitches: variates
