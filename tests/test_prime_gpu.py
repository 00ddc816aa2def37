"""Primed generation on the GPU: the replay kernel against the plain-Python contract (tests/prime_contract.py), the
ragged prefill scatter against numpy indexing, prefill_ragged against prefill(), and the primed loop end to end against
the reference's own sequences (tests/golden/g6_decode.npz)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import prime_contract as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "g6_decode.npz"))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 1. the replay kernel
GUARD = -77


def _guarded(rows, cols, dtype, fill):
    """[rows, cols] view into a buffer with one guard row on each side."""
    full = torch.full((rows + 2, cols), fill, dtype=dtype, device=DEV)
    return full, full[1:rows + 1]


def _replay_batch(z, cases):
    """cases: [(tag, prompt)], one slot each, through commu_forcing_replay; every output compared with the contract.
    Returns the kernel's divergences."""
    from commu_amd._lib import call
    B = len(cases)
    NF = call("commu_forcing_state_ints")
    assert NF == P.NF
    n_ctx = 1 + len(META)
    ld_prompt = max(1, max(len(p) for _, p in cases))
    ld_seq = n_ctx + ld_prompt + 3
    ld_fed = 2 * ld_prompt + 5
    ld_trace = 2 * (2 * ld_prompt + 2)
    ld_chord, ld_u = 8, 4
    i32 = torch.int32
    fsm_f, fsm = _guarded(B, NF, i32, GUARD)
    seq_f, seq = _guarded(B, ld_seq, i32, GUARD)
    fed_f, fed = _guarded(B, ld_fed, i32, GUARD)
    klen_f, klen = _guarded(B, 1, i32, GUARD)
    div_f, div = _guarded(B, 2, i32, GUARD)
    tr_f, trace = _guarded(B, ld_trace, i32, GUARD)
    lp_f, seq_logp = _guarded(B, ld_seq * 2, torch.float32, 7.0)
    prompt = torch.full((B, ld_prompt), 5, dtype=i32)
    plen = torch.zeros(B, dtype=i32)
    ctok, cpos = torch.zeros(B, ld_chord, dtype=i32), torch.zeros(B, ld_chord, dtype=i32)
    rec0, want = [], []
    for b, (tag, pr) in enumerate(cases):
        ctx, ct, cp, nm, _ = P.fixture(z, tag)
        r0 = P.initial_record(len(ctx) - 1, len(ct), nm)
        if not pr:          # an untouched record keeps even what a replay would reset
            r0[P.F_ITERS], r0[P.F_NDRAW] = 9, 9
        rec0.append(r0)
        prompt[b, :len(pr)] = torch.tensor(pr, dtype=i32)
        plen[b] = len(pr)
        ctok[b, :len(ct)], cpos[b, :len(cp)] = torch.tensor(ct, dtype=i32), torch.tensor(cp, dtype=i32)
        seq[b, :n_ctx] = torch.tensor(ctx, dtype=i32, device=DEV)
        want.append(P.replay(ctx, ct, cp, nm, pr, ld_seq=ld_seq))
    fsm.copy_(torch.tensor(rec0, dtype=i32))
    klen.fill_(n_ctx - 1)
    wrong = torch.zeros(B, 729, dtype=torch.uint8, device=DEV)
    utable = torch.full((B, ld_u), 0.5, device=DEV)
    tok = torch.zeros(B, dtype=torch.long, device=DEV)
    flags = [torch.zeros(B, dtype=torch.uint8, device=DEV) for _ in range(3)]
    uni = torch.zeros(B, device=DEV)
    prompt, plen, ctok, cpos = prompt.to(DEV), plen.to(DEV), ctok.to(DEV), cpos.to(DEV)
    call("commu_forcing_replay", _p(fsm), _p(seq), ld_seq, _p(prompt), ld_prompt, _p(plen), _p(ctok), _p(cpos), ld_chord,
         _p(wrong), _p(utable), ld_u, _p(tok), _p(flags[0]), _p(flags[1]), _p(flags[2]), _p(uni), _p(trace), ld_trace,
         _p(seq_logp), _p(klen), _p(fed), ld_fed, _p(div), B, _s())
    torch.cuda.synchronize()
    for full in (fsm_f, seq_f, fed_f, klen_f, div_f, tr_f):          # nothing outside the B rows
        assert bool((full[0] == GUARD).all()) and bool((full[-1] == GUARD).all())
    assert bool((lp_f[0] == 7.0).all()) and bool((lp_f[-1] == 7.0).all())
    fsm_h, seq_h, fed_h, klen_h, div_h, tr_h = (t.cpu().numpy() for t in (fsm, seq, fed, klen, div, trace))
    lp_h = seq_logp.cpu().numpy().reshape(B, ld_seq, 2)
    wrong_h = wrong.cpu().numpy()
    for b, (tag, pr) in enumerate(cases):
        s, sq, fd, dv = want[b]
        assert tuple(div_h[b]) == dv, (b, tag, len(pr))
        if not pr:
            assert fsm_h[b].tolist() == rec0[b], (b, tag)          # bit for bit as loaded
        else:
            assert fsm_h[b].tolist() == s, (b, tag, len(pr))
        assert seq_h[b, :len(sq)].tolist() == sq and bool((seq_h[b, len(sq):] == GUARD).all()), (b, tag, len(pr))
        # appended tokens were not drawn by this run: NaN pairs; nothing else is written
        assert np.isnan(lp_h[b, n_ctx:len(sq)]).all() and (lp_h[b, :n_ctx] == 7.0).all() and (lp_h[b, len(sq):] == 7.0).all()
        if dv[0] >= 0:
            continue
        kp = P.kept(fd)
        assert fed_h[b, :len(kp)].tolist() == kp and bool((fed_h[b, len(kp):] == GUARD).all()), (b, tag, len(pr))
        assert int(klen_h[b, 0]) == n_ctx - 1 + len(kp)
        flat = [v for t, k in fd for v in (t, k)]
        assert tr_h[b, :len(flat)].tolist() == flat and bool((tr_h[b, len(flat):] == GUARD).all()), (b, tag, len(pr))
        assert not wrong_h[b].any()
    return div_h


def test_replay_kernel_equals_the_contract_on_the_fixture_cuts(z):
    """The five fixtures, each cut at the empty prompt, one token, right after a BAR, after the forced 432 that follows
    a BAR, after a chord token and at the last token before EOS, ragged in batches of 8 together with the planted
    divergences: record, seq, kept fed stream, klen, trace and divergence equal the contract's integers; guard rows
    around every output are intact; an empty prompt leaves its record as loaded."""
    cases = []
    for tag in P.TAGS:
        p = P.fixture(z, tag)[4]
        cases += [(tag, p[:k]) for k in P.cut_points(p)]
    plant = P.planted(z)
    cases += [(tag, pr) for _, tag, pr, _ in plant]
    cases.append(("greedy8", [500, 729]))                      # a token outside the vocabulary: reason 4 at index 1
    # interleave long and short prompts so that every batch is ragged
    order = sorted(range(len(cases)), key=lambda i: (i % 8, i))
    cases = [cases[i] for i in order]
    ndiv = 0
    for first in range(0, len(cases), 8):
        batch = cases[first:first + 8]
        while len(batch) < 8:
            batch.append(("greedy5", []))
        div = _replay_batch(z, batch)
        ndiv += int((div[:, 0] >= 0).sum())
    assert ndiv == len(plant) + 1
    for name, tag, pr, want in plant:                          # (also against the literal expectations)
        assert tuple(_replay_batch(z, [(tag, pr)] + [("greedy8", [])] * 7)[0]) == want, name


# ------------------------------------------------------------------------------------------------ 2. the scatter kernel
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


@pytest.mark.parametrize("ring", [False, True], ids=["linear", "ring"])
@pytest.mark.parametrize("layout", ["bf16_dh32", "bf16_dh64", "f32_dh32", "f32_dh64", "f32_dh50_unaligned"])
def test_prefill_scatter_kernel_is_numpy_indexing(layout, ring):
    """B = 3, H = 2, T = 37; linear lens [0, 1, 37], ring M = 16 (17 rows) lens [0, 5, 37] (two wraps); padded row pitch,
    more cache rows than needed, a permuted slot map into a cache of 4 slots.  The caches start as NaN: the rows in range
    hold the source bits, every other row still holds its NaN; klen as stated (the unnamed slot keeps its value)."""
    from commu_amd import ops
    B, H, T, Bc = 3, 2, 37, 4
    f32 = layout.startswith("f32")
    DH = int(layout.split("dh")[1].split("_")[0])
    HD = H * DH
    dt = torch.float32 if f32 else torch.bfloat16
    pad = 1 if layout.endswith("unaligned") else 8
    M = 16
    Lmax, window, lens = (M + 1, M, [0, 5, 37]) if ring else (48, 0, [0, 1, 37])
    slots = [2, 0, 3]
    g = torch.Generator().manual_seed(3)
    buf = torch.randn(T * B, 3 * HD + pad, generator=g).to(dt).to(DEV)
    qkv = buf[:, :3 * HD]
    shape = (Bc, Lmax, HD) if f32 else (Bc, H, Lmax, DH)
    kc = torch.full(shape, float("nan"), dtype=dt, device=DEV)
    vc = torch.full(shape, float("nan"), dtype=dt, device=DEV)
    klen = torch.full((Bc,), -9, dtype=torch.int32, device=DEV)
    nan_bits = _bits(kc)[0, 0, 0].copy() if f32 else _bits(kc)[0, 0, 0, 0].copy()
    ops.decode_prefill_scatter(qkv, T, kc, vc, klen, torch.tensor(lens, dtype=torch.int32, device=DEV),
                               torch.tensor(slots, dtype=torch.int32, device=DEV), window=window)
    torch.cuda.synchronize()
    src = _bits(qkv).reshape(T, B, 3, H, DH)
    want_k = np.full(shape, nan_bits, dtype=src.dtype)
    want_v = want_k.copy()
    for b in range(B):
        for t in range(max(0, lens[b] - M) if ring else 0, lens[b]):
            row = t % Lmax if ring else t
            if f32:
                want_k[slots[b], row] = src[t, b, 1].reshape(HD)
                want_v[slots[b], row] = src[t, b, 2].reshape(HD)
            else:
                want_k[slots[b], :, row] = src[t, b, 1]
                want_v[slots[b], :, row] = src[t, b, 2]
    assert np.array_equal(_bits(kc), want_k) and np.array_equal(_bits(vc), want_v)
    want_klen = [-9] * Bc
    for b in range(B):
        want_klen[slots[b]] = lens[b]
    assert klen.tolist() == want_klen


# ------------------------------------------------------------------------------------------------ 3. prefill_ragged
def _fixture_model(golden_dir, z, tag="greedy8", mem=4146, parity=False):
    import test_decode_gpu as TD
    model = TD._build(golden_dir, z, z[f"{tag}_bias"])
    model.reset_length(1, mem)
    model.parity_fp32 = parity
    return model


@pytest.mark.parametrize("window", [None, 16], ids=["linear", "ring16"])
@pytest.mark.parametrize("kind", ["bf16_dh32", "bf16_dh64", "parity_fp32"])
def test_prefill_ragged_equals_prefill_and_ignores_padding(golden_dir, z, kind, window):
    """All lens equal: caches and klen bit-identical to prefill() on the same context.  Ragged lens: two runs whose
    padding holds different tokens give bit-identical caches (the forward is causal: padding cannot reach a valid row).
    A slot map fills the named slots only."""
    from commu_amd.generate import DecodeState
    if kind == "bf16_dh64":
        from test_configs_gpu import build
        model = build(2, 2, 128, 256, 1, 4146 if window is None else window, seed=3)[0]
        model.eval()
        model.same_length = True
        model.reset_length(1, 4146 if window is None else window)
    else:
        model = _fixture_model(golden_dir, z, mem=4146 if window is None else window, parity=kind == "parity_fp32")
    B, T = 4, 37
    Lmax = 48 if window is None else window + 1
    g = torch.Generator().manual_seed(9)
    ctx = torch.randint(2, 729, (T, B), generator=g).to(DEV)
    with torch.no_grad():
        a, b_ = DecodeState(model, B, Lmax, window=window), DecodeState(model, B, Lmax, window=window)
        assert a.parity == (kind == "parity_fp32")
        a.prefill(ctx)
        b_.prefill_ragged(ctx, [T] * B)
        assert torch.equal(a.klen, b_.klen)
        assert np.array_equal(_bits(a.kc), _bits(b_.kc)) and np.array_equal(_bits(a.vc), _bits(b_.vc))
        lens = [37, 1, 20, 5]
        outs = []
        for seed in (1, 2):
            c = ctx.clone()
            junk = torch.randint(2, 729, (T, B), generator=torch.Generator().manual_seed(seed)).to(DEV)
            for b in range(B):
                c[lens[b]:, b] = junk[lens[b]:, b]
            st = DecodeState(model, B, Lmax, window=window)
            st.prefill_ragged(c, torch.tensor(lens, dtype=torch.int32, device=DEV))
            assert st.klen.tolist() == lens
            outs.append((_bits(st.kc), _bits(st.vc)))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        # slots: two contexts into slots 3 and 1 of the four; the others keep their (zero) rows and klen
        st = DecodeState(model, B, Lmax, window=window)
        st.prefill_ragged(ctx[:, :2].contiguous(), [T, 5], slots=[3, 1])
        assert st.klen.tolist() == [0, 5, 0, T]
        kb = _bits(st.kc)
        assert not kb[:, 0].any() and not kb[:, 2].any() and kb[:, 3].any()


# ------------------------------------------------------------------------------------------------ 4. end to end
def _data(z, tag):
    return types.SimpleNamespace(num_measures=float(z[f"{tag}_cfg"][1]), chord_token_components={
        "chord_token": z[f"{tag}_chord_token"].tolist(), "chord_position": z[f"{tag}_chord_position"].tolist()})


def _primed_decoder(model, z, tag, prompts, glen, memory_length=4146, sliding=False, uniforms=None, record_trace=True):
    from commu_amd.generate import ForcedDecoder
    temp, _, top_k, _ = z[f"{tag}_cfg"]
    B = len(prompts)
    dec = ForcedDecoder(model, B, glen, memory_length, float(temp), int(top_k), record_trace=record_trace, sliding=sliding,
                        max_prompt=max(1, max(len(p) for p in prompts)))
    uni = np.full((B, dec.ld_u), 0.5, dtype=np.float32)
    if uniforms is not None:
        n = min(uniforms.shape[1], dec.ld_u)
        uni[:, :n] = uniforms[:, :n]
    dec.load([META] * B, [_data(z, tag)] * B, uni, prompts=prompts)
    return dec


@pytest.mark.parametrize("parity", [False, True], ids=["bf16", "parity_fp32"])
@pytest.mark.parametrize("tag", ["greedy8", "greedy5"])
def test_primed_continuation_reproduces_the_reference_sequence(golden_dir, z, tag, parity):
    """Ragged cuts of the fixture's sequence primed in one batch and run through the captured graph: every slot's tokens
    equal the fixture's sequence and its trace the fixture's trace over its whole length (the replayed part included).
    The fixture's top-1 / top-2 logit gap is > 0.1 against a bf16 logit error of ~2e-3.  Graph replay equals eager
    launches bit for bit.  Slots with an empty prompt hold load()'s record."""
    assert float(z[f"{tag}_min_gap"]) > 0.1
    model = _fixture_model(golden_dir, z, tag, parity=parity)
    assert list(z["encoded_meta"]) == META
    ctx, ct, cp, nm, p = P.fixture(z, tag)
    cuts = P.cut_points(p)
    prompts = [p[:k] for k in cuts]
    glen = int(z[f"{tag}_cfg"][3])
    ref = z[f"{tag}_seq"].tolist()
    ref_trace = [tuple(t) for t in z[f"{tag}_trace"].tolist()]
    results = []
    for use_graph in (True, False):
        dec = _primed_decoder(model, z, tag, prompts, glen)
        assert dec.state.parity == parity
        fsm0, klen0 = dec.fsm.cpu().numpy(), dec.state.klen.cpu().numpy()
        for b, k in enumerate(cuts):
            s, _, fed, _ = P.replay(ctx, ct, cp, nm, p[:k])
            assert fsm0[b].tolist() == s and int(klen0[b]) == len(ctx) - 1 + len(P.kept(fed)), (b, k)
        assert fsm0[0].tolist() == P.initial_record(len(META), len(ct), nm)
        with torch.no_grad():
            dec.run(use_graph=use_graph)
        torch.cuda.synchronize()
        results.append((dec.seq.clone(), dec.fsm.clone(), dec.state.klen.clone(), dec.state.logits.clone(), dec.sequences()))
    (sg, fg, kg, lg, outg), (se, fe, ke, le, _) = results
    assert torch.equal(sg, se) and torch.equal(fg, fe) and torch.equal(kg, ke) and torch.equal(lg, le)
    seqs, traces = outg
    for b, k in enumerate(cuts):
        assert seqs[b][:len(ref)] == ref, (b, k)
        assert traces[b][:len(ref_trace)] == ref_trace, (b, k)
        assert len(seqs[b]) >= len(ref)


# ------------------------------------------------------------------------------------------------ 5. sliding memory
SLIDING_M = 32


def test_primed_continuation_with_a_sliding_memory(golden_dir, z):
    """greedy8 with sliding=True and a memory of 32, primed at a cut whose replayed stream is longer than the ring (the
    ragged prefill wraps).  First the free run's own minimum top-1 / top-2 gap at that window is measured (existing
    code): it must be above 0.05.  Then the primed continuation equals that free run token for token."""
    from commu_amd.generate import ForcedDecoder
    tag, M = "greedy8", SLIDING_M
    model = _fixture_model(golden_dir, z, tag, mem=M)
    glen = int(z[f"{tag}_cfg"][3])
    free = ForcedDecoder(model, 1, glen, M, 0.0, int(z[f"{tag}_cfg"][2]), sliding=True)
    free.load([META], [_data(z, tag)])
    gap = float("inf")
    with torch.no_grad():
        for _ in range(glen + 1):
            free.iteration()
            if int(free.draw[0]):
                top = torch.topk(free.state.logits[0, 1:729], 2).values
                gap = min(gap, float(top[0] - top[1]))
            if int(free.fsm[0, 5]):
                break
    want = free.sequences()[0][0]
    print(f"sliding primed: memory {M}, free run {len(want)} tokens, min top-1/top-2 gap {gap:.4f}")
    assert gap > 0.05
    p = want[1 + len(META):]
    cuts = [60, 100, len(p) - 1]
    fed = [P.kept(P.replay(*P.fixture(z, tag)[:4], p[:k])[2]) for k in cuts]
    assert min(len(f) for f in fed) > M + 1, "the replayed stream must be longer than the ring"
    dec = _primed_decoder(model, z, tag, [p[:k] for k in cuts], glen, memory_length=M, sliding=True, record_trace=False)
    assert dec.state.window == M and int(dec.state.klen.min()) > M + 1
    with torch.no_grad():
        dec.run()
    for b, s in enumerate(dec.sequences()[0]):
        assert s[:len(want)] == want, (b, cuts[b])


# ------------------------------------------------------------------------------------------------ 6. re-arm
@pytest.mark.parametrize("sliding", [False, True], ids=["linear", "sliding32"])
def test_rearmed_primed_slot_repeats_a_fresh_load(golden_dir, z, sliding):
    """A primed slot that has finished and is re-armed returns to its primed state: with the same variates it produces
    bit for bit the seq of a fresh load().  Sampled (sample8m's variates), ragged prompts; sliding: the prompts' streams
    are longer than the ring, so the ring rows must come back too."""
    tag = "sample8m"
    M = 32 if sliding else 4146
    model = _fixture_model(golden_dir, z, tag, mem=M)
    p = P.fixture(z, tag)[4]
    cuts = [40, 55, 70, len(p)] if sliding else [0, 1, 40, len(p)]
    prompts = [p[:k] for k in cuts]
    uni = np.tile(z[f"{tag}_uniforms"][None, 30:].astype(np.float32), (len(cuts), 1))
    glen = 60
    fresh = _primed_decoder(model, z, tag, prompts, glen, memory_length=M, sliding=sliding, uniforms=uni)
    with torch.no_grad():
        fresh.run()
    want_seq, want_fsm, want_klen = fresh.seq.clone(), fresh.fsm.clone(), fresh.state.klen.clone()
    assert bool(want_fsm[:, 5].all())
    dec = _primed_decoder(model, z, tag, prompts, glen, memory_length=M, sliding=sliding, uniforms=uni)
    with torch.no_grad():
        dec.run()
        if sliding:
            assert int(dec.state.klen.min()) > M + 1
        for b in range(len(cuts)):
            dec.rearm(b, uni[b])
        primed = P.replay(*P.fixture(z, tag)[:4], prompts[2])[0]
        assert dec.fsm[2].tolist() == primed
        dec.run()
    assert torch.equal(dec.seq, want_seq) and torch.equal(dec.fsm, want_fsm) and torch.equal(dec.state.klen, want_klen)
    seqs, traces = dec.sequences()
    assert traces == fresh.sequences()[1]          # the re-armed trace covers the replayed stream again
    for b, k in enumerate(cuts):
        assert seqs[b][:1 + len(META) + k] == [0] + META + p[:k]


def test_generate_stream_with_a_prompt_returns_the_sequential_loops_answer():
    """generate_stream(prompt=) re-arms primed slots at different times; its answer is the first `need` accepted
    attempts in attempt order, as decoded by plain primed batches.  Every sequence starts with the prompt; its
    log-probabilities are NaN over context and prompt and present afterwards."""
    from commu_amd.generate import BatchedGenerator, ForcedDecoder
    from test_configs_gpu import build
    model, cfg, s, params = build(6, 8, 512, 1024, 1, 4146, seed=41)
    model.eval()
    model.same_length = True
    model.reset_length(1, 4146)
    with torch.no_grad():
        bias = model.crit.out_layers[0].bias
        bias.zero_()
        bias[1] = 3.0                         # EOS is drawn every few dozen tokens: lengths differ
        bias[2] = -1e9
        bias[195:304] = -1e9
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
    prompt = [500, 64, 310, 520, 70]
    GL, NEED, SLOTS = 65, 24, 16          # (a sequence that runs to the cap has 12 + 5 + 65 = 82 tokens: accepted)
    head = [0] + META + prompt

    def accept(seq, rep):
        return seq is not None and len(seq) % 3 != 0
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=GL, memory_length=4146)
    out, started, lps = gen.generate_stream(META, data, 0.95, 32, need=NEED, accept=accept, slots=SLOTS, seed=5,
                                            return_logprobs=True, prompt=prompt)
    allseq = []
    for first in range(0, 64, SLOTS):
        dec = ForcedDecoder(model, SLOTS, generation_length=GL, memory_length=4146, temperature=0.95, top_k=32,
                            max_prompt=len(prompt))
        uni = np.stack([BatchedGenerator.attempt_uniforms(5, first + b, dec.ld_u) for b in range(SLOTS)])
        dec.load([META] * SLOTS, [data] * SLOTS, uni, prompts=[prompt] * SLOTS)
        with torch.no_grad():
            dec.run(use_graph=False)
        allseq += dec.sequences()[0]
    lens = sorted(len(s_) for s_ in allseq)
    assert lens[0] < lens[-1] - 10, "the attempts should have different lengths"
    want = [s_ for s_ in allseq if accept(s_, None)][:NEED]
    assert len(want) == NEED and out == want
    assert NEED <= started <= 64
    for s_, lp in zip(out, lps):
        assert s_[:len(head)] == head and len(s_) > len(head)
        assert lp.shape == (len(s_), 2)
        assert np.isnan(lp[:len(head)]).all() and np.isfinite(lp[len(head):]).all()
    # generate(prompts=): ragged prompts, one per sequence
    seqs, _ = gen.generate([META] * 3, [data] * 3, 0.0, 32, prompts=[[], prompt[:2], prompt])
    for s_, pr in zip(seqs, ([], prompt[:2], prompt)):
        assert s_[:12 + len(pr)] == [0] + META + pr and len(s_) > 12 + len(pr)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_prompt_refusals_name_the_numbers(golden_dir, z):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ForcedDecoder
    tag = "greedy8"
    model = _fixture_model(golden_dir, z, tag)
    p = P.fixture(z, tag)[4]
    datas = [_data(z, tag)] * 2
    dec = ForcedDecoder(model, 2, 40, 4146, 0.0, 32, max_prompt=20)
    with pytest.raises(CommuHipError, match=r"slot 1 has 21 tokens.*max_prompt=20"):
        dec.load([META] * 2, datas, prompts=[[], p[:21]])
    with pytest.raises(CommuHipError, match=r"slot 0: token 729 at index 2 is outside \[0, 729\)"):
        dec.load([META] * 2, datas, prompts=[[500, 501, 729], []])
    with pytest.raises(CommuHipError, match=r"slot 1: token -1 at index 0"):
        dec.load([META] * 2, datas, prompts=[[], [-1]])
    name, _, bad, (idx, why) = next(c for c in P.planted(z) if c[0] == "wrong chord")
    with pytest.raises(CommuHipError, match=rf"slot 1 cannot be continued: token {bad[idx]} at index {idx} of {len(bad)}.*"
                                            rf"\(reason {why}\)"):
        dec.load([META] * 2, datas, prompts=[p[:3], bad])
    with pytest.raises(CommuHipError, match=r"slot 0 cannot be continued: token 200 at index 0 of 1.*\(reason 2\)"):
        dec.load([META] * 2, datas, prompts=[[200], p[:3]])
    dec.load([META] * 2, datas, prompts=[p[:3], p[:20]])          # (the decoder is usable after a refusal)
    # a decoder built without max_prompt takes no prompt
    with pytest.raises(CommuHipError, match=r"max_prompt=0"):
        ForcedDecoder(model, 2, 40, 4146, 0.0, 32).load([META] * 2, datas, prompts=[[500], []])
    # a linear cache that cannot hold the primed memory plus generation_length
    short = ForcedDecoder(model, 2, 40, 60, 0.0, 32, max_prompt=20)
    s, _, fed, _ = P.replay(*P.fixture(z, tag)[:4], p[:20])
    klen = 11 + len(P.kept(fed))
    assert klen + 40 + 1 > 61
    with pytest.raises(CommuHipError, match=rf"slot 1 starts with {klen} cached positions.*needs {klen + 41}.*has 61"):
        short.load([META] * 2, datas, prompts=[[], p[:20]])
