"""The sliding memory window of the cached decode step (ring K/V cache: csrc/decode.hip, csrc/parity_f32.hip,
commu_amd/generate.py) on the GPU: the ring kernels against the linear kernel and a float64 evaluation of the contract,
the cached step against oracle.xl_ref.forward_generate with a SHORT memory through several wraps, free-running greedy
decoding, the whole forced loop on the reference-shaped fixtures, and re-arming a slot whose ring has wrapped.

Contract (commu/model/model.py:507-568 at qlen 1, mlen = M): the token at absolute position pos sees positions
max(0, pos - M) .. pos at distance pos - p; with same_length and pos >= M the oldest of them is hidden."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import decode_ref as Dz  # noqa: E402
from oracle import xl_ref as X  # noqa: E402
import decode_contract as DC  # noqa: E402
from decode_contract import visible as _visible  # noqa: E402

DEV = "cuda"


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ------------------------------------------------------------------------------------------------ 1. kernels
def _contract_f64(q, kc, vc, rd, u, vb, pos_list, M, same_length, scale, head_major):
    """float64 evaluation of the contract on the ring caches (the new token's K/V already in row pos mod W):
    decode_contract.contract_f64 over the batch.  q [B, H, DH]; kc / vc [B, H, W, DH] (head_major) or [B, W, H, DH];
    rd [>= W, H, DH]; returns (want, A) [B, H, DH]: the output and the magnitude its accumulation error scales with."""
    return DC.contract_batch(q, kc, vc, rd, u, vb, DC.ring_rows_dist(pos_list, M, same_length), scale, head_major)


def _positions(M):
    """Ragged absolute positions: not yet full, exactly full (M - 1, M, M + 1), wrapped once, wrapped several times plus
    an offset, and the two alignments where the hidden row is the last / the first physical row."""
    W = M + 1
    return [5, M - 1, M, M + 1, W + 17, 3 * W + 41, 7 * W + (W - 1), 5 * W, 2 * W - 2, 40]


@pytest.mark.parametrize("same_length", [True, False], ids=["same_length", "no_same_length"])
@pytest.mark.parametrize("DH,M", [(64, 96), (32, 96), (64, 2303), (32, 2303)])
def test_ring_attention_kernel_bf16_vs_linear_kernel(DH, M, same_length):
    """commu_decode_attn_ring (unsplit, and split over 4 workgroups where the ring has >= 2048 rows) against the existing
    linear kernel commu_decode_attn on a DE-ROTATED copy of the same cache: rows back in chronological order, the hidden
    oldest row dropped, klen set accordingly -- the same mathematics in a different summation order with one bf16 output
    rounding, which is what test_split_key_decode_attention_matches_the_unsplit_kernel bounds at 2e-2 of the output's
    max.  With append the new K/V must land in row pos mod W and nowhere else.  Both kernels are also held, element by
    element, to the float64 contract: |got - want| <= 2^-8 |want| + c A (tests/decode_contract.py)."""
    from commu_amd import ops
    from commu_amd._lib import call
    from commu_amd.ops import _p, _s
    H, W, scale = 4, M + 1, 0.125
    pos_list = _positions(M)
    B, HD = len(pos_list), H * DH
    g = torch.Generator().manual_seed(100 + DH + M)
    qkv = (torch.randn(B, 3 * HD, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    kc0 = (torch.randn(B, H, W, DH, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    vc0 = torch.randn(B, H, W, DH, generator=g).to(torch.bfloat16).to(DEV)
    rd = (torch.randn(W, HD, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    u, vb = (torch.randn(HD, generator=g) * 0.3).to(DEV), (torch.randn(HD, generator=g) * 0.3).to(DEV)
    klen = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    active = torch.ones(B, dtype=torch.uint8, device=DEV)
    active[B - 1] = 0
    # the cache after the append, built on the host: row pos mod W of every active sequence <- K / V of qkv
    kc1, vc1 = kc0.clone(), vc0.clone()
    for b, pos in enumerate(pos_list):
        if active[b]:
            kc1[b, :, pos % W] = qkv[b, HD:2 * HD].view(H, DH)
            vc1[b, :, pos % W] = qkv[b, 2 * HD:].view(H, DH)
    # the separate append entry point writes exactly that
    kc, vc = kc0.clone(), vc0.clone()
    ops.decode_kv_append_ring(qkv, kc, vc, klen, active, W)
    assert torch.equal(kc, kc1) and torch.equal(vc, vc1)
    # de-rotated linear copy (chronological, hidden row dropped) for the existing kernel
    kl, vl = torch.zeros_like(kc1), torch.zeros_like(vc1)
    nlin = []
    for b, pos in enumerate(pos_list):
        rows = torch.tensor(_visible(pos, M, same_length), device=DEV) % W
        kl[b, :, :len(rows)] = kc1[b][:, rows]
        vl[b, :, :len(rows)] = vc1[b][:, rows]
        nlin.append(len(rows) - 1)
    klen_lin = torch.tensor(nlin, dtype=torch.int32, device=DEV)
    lin = torch.zeros(B, HD, device=DEV, dtype=torch.bfloat16)
    call("commu_decode_attn", _p(qkv), qkv.stride(0), _p(kl), _p(vl), _p(rd), rd.stride(0), _p(u), _p(vb), _p(klen_lin),
         _p(active), _p(lin), lin.stride(0), B, H, DH, W, scale, 0, _s())
    want, A = (t.view(B, HD) for t in _contract_f64(qkv[:, :HD].view(B, H, DH), kc1, vc1, rd.view(W, H, DH), u.view(H, DH),
                                                    vb.view(H, DH), pos_list, M, same_length, scale, True))
    want[B - 1] = 0
    top = float(lin.float().abs().max())
    err_lin = float((lin.double().cpu() - want).abs().max()) / top
    r_lin = float(DC.ratio(lin.cpu()[:B - 1], want[:B - 1], A[:B - 1]).nan_to_num(nan=float("inf")).max())
    assert r_lin <= 1.0, ("linear kernel vs float64 contract", r_lin)
    ws = torch.full((B * H * 16 * (DH + 2),), float("nan"), device=DEV, dtype=torch.float32)
    cnt = torch.zeros(B * H, device=DEV, dtype=torch.int32)
    for nsplit in ((1, 4) if W >= 2048 else (1,)):
        for append in (False, True):
            for rep in range(3):
                kc, vc = (kc0.clone(), vc0.clone()) if append else (kc1.clone(), vc1.clone())
                out = torch.zeros(B, HD, device=DEV, dtype=torch.bfloat16)
                ops.decode_attn_ring(qkv, kc, vc, rd, u, vb, klen, active, out, W, scale, append=append,
                                     same_length=same_length, nsplit=nsplit, split_ws=ws, split_cnt=cnt)
                torch.cuda.synchronize()
                assert int(cnt.abs().sum()) == 0, (nsplit, rep)
                assert torch.equal(kc, kc1) and torch.equal(vc, vc1), (nsplit, append, "cache rows")
                d = float((out.float() - lin.float()).abs().max())
                err = float((out.double().cpu() - want).abs().max()) / top
                r = float(DC.ratio(out.cpu()[:B - 1], want[:B - 1], A[:B - 1]).nan_to_num(nan=float("inf")).max())
                if rep == 0:
                    print(f"ring decode attention DH {DH} W {W} same_length {same_length} nsplit {nsplit} append {append}: "
                          f"vs linear kernel {d / top:.2e} of max; vs float64 contract: ring {err:.2e}, linear {err_lin:.2e} "
                          f"of max; of the per-element bound: ring {r:.3f}, linear {r_lin:.3f}")
                assert r <= 1.0, (nsplit, append, rep, "ring kernel vs float64 contract", r)
                assert d < 2e-2 * top, (nsplit, append, rep, d, top)
                assert float(out[B - 1].float().abs().max()) == 0          # the inactive sequence is not touched


@pytest.mark.parametrize("same_length", [True, False], ids=["same_length", "no_same_length"])
@pytest.mark.parametrize("DH,M", [(64, 96), (32, 96), (50, 96), (64, 2303)])
def test_ring_attention_kernel_f32_vs_float64(DH, M, same_length):
    """The parity-mode entry points (commu_decode_kv_append_ring_f32, commu_decode_attn_ring_f32) against the float64
    evaluation of the contract: <= 2e-6 of the output's range (the project's bound for its fp32 kernels); the append
    writes row pos mod W of the active sequences and nothing else."""
    from commu_amd import ops
    H, W, scale = 4, M + 1, 1.0 / DH ** 0.5
    pos_list = _positions(M)
    B, HD = len(pos_list), H * DH
    g = torch.Generator().manual_seed(200 + DH + M)
    qkv = (torch.randn(B, 3 * HD, generator=g) * 0.7).to(DEV)
    kc0 = (torch.randn(B, W, HD, generator=g) * 0.7).to(DEV)
    vc0 = torch.randn(B, W, HD, generator=g).to(DEV)
    rd = (torch.randn(W, HD, generator=g) * 0.7).to(DEV)
    u, vb = (torch.randn(HD, generator=g) * 0.3).to(DEV), (torch.randn(HD, generator=g) * 0.3).to(DEV)
    klen = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
    active = torch.ones(B, dtype=torch.uint8, device=DEV)
    active[B - 1] = 0
    kc1, vc1 = kc0.clone(), vc0.clone()
    for b, pos in enumerate(pos_list):
        if active[b]:
            kc1[b, pos % W] = qkv[b, HD:2 * HD]
            vc1[b, pos % W] = qkv[b, 2 * HD:]
    kc, vc = kc0.clone(), vc0.clone()
    ops.decode_kv_append_ring_f32(qkv, kc, vc, klen, active, HD, W)
    assert torch.equal(kc, kc1) and torch.equal(vc, vc1)
    out = ops.decode_attn_ring_f32(qkv[:, :HD], kc, vc, rd, u, vb, klen, H, DH, W, same_length, scale)
    assert torch.equal(kc, kc1) and torch.equal(vc, vc1)
    want = _contract_f64(qkv[:, :HD].view(B, H, DH), kc1.view(B, W, H, DH), vc1.view(B, W, H, DH), rd.view(W, H, DH),
                         u.view(H, DH), vb.view(H, DH), pos_list, M, same_length, scale, False)[0].view(B, HD)
    err = float((out.double().cpu() - want).abs().max()) / float(want.abs().max())
    print(f"fp32 ring decode attention DH {DH} W {W} same_length {same_length}: {err:.2e} of range")
    assert err <= 2e-6


# ------------------------------------------------------------------------------------------------ 2. unwrapped = linear
def _short_model(shape, M, seed, same_length, parity, std=0.02):
    from test_parity_fp32_gpu import _model
    L, H, D, DI = shape
    model, s, params = _model(L, H, D, DI, seed=seed, std=std, mem_len=M)
    model.same_length = same_length
    model.parity_fp32 = parity
    return model, s, params


@pytest.mark.parametrize("parity", [False, True], ids=["bf16", "parity_fp32"])
def test_window_state_equals_linear_state_before_the_first_wrap(parity):
    """DecodeState(model, B, M + 1, window=M) against DecodeState(model, B, M + 1) while context + steps <= M: the ring
    visits the same rows in the same order, so step() logits are equal bit for bit over 32 steps (one of them discarded
    for one sequence, quirk Q3)."""
    from commu_amd.generate import DecodeState
    M, B, T0, NSTEP = 96, 3, 11, 32
    model, _, _ = _short_model((6, 8, 512, 1024), M, 41, True, parity)
    g = torch.Generator().manual_seed(3)
    ctx = torch.randint(2, 729, (T0, B), generator=g).to(DEV)
    lin, win = DecodeState(model, B, M + 1), DecodeState(model, B, M + 1, window=M)
    assert win.Lmax == lin.Lmax and win.kc.shape == lin.kc.shape and win.parity == parity
    lin.prefill(ctx)
    win.prefill(ctx)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    for step in range(NSTEP):
        tok = torch.randint(2, 729, (B,), generator=g).to(DEV)
        keep = ones.clone()
        if step == 3:
            keep[1] = 0
        a = lin.step(tok, ones, keep).clone()
        b = win.step(tok, ones, keep).clone()
        assert torch.equal(a, b), step
    assert torch.equal(lin.klen, win.klen) and int(win.klen[0]) == T0 + NSTEP and int(win.klen[1]) == T0 + NSTEP - 1
    assert torch.equal(lin.kc, win.kc) and torch.equal(lin.vc, win.vc)


# ------------------------------------------------------------------------------------------------ 3. vs the oracle
@pytest.mark.parametrize("same_length", [True, False], ids=["same_length", "no_same_length"])
@pytest.mark.parametrize("T0,NSTEP", [(11, 320), (150, 120)], ids=["ctx11_320steps", "ctx150_120steps"])
@pytest.mark.parametrize("shape", [(6, 8, 512, 1024), (6, 10, 500, 1000)], ids=["L6_D512_dh64", "L6_D500_dh50"])
def test_cached_sliding_step_vs_oracle(shape, T0, NSTEP, same_length):
    """The cached step with a sliding memory of M = 96 against oracle.xl_ref.forward_generate(params, s, tok, mems, 96,
    same_length), which keeps the last 96 hidden states like the reference: a context of 11 tokens and 320 single-token
    steps (three wraps), or a context LONGER than the window (150) and 120 steps; teacher-forced with the same seeded
    random tokens; EVERY step's logits compared.  bf16 <= 2e-2 of the logit range, parity mode <= 1e-4."""
    from commu_amd.generate import DecodeState
    M, B = 96, 3
    model, s, params = _short_model(shape, M, 41, same_length, False)
    g = torch.Generator().manual_seed(19)
    ctx = torch.randint(2, 729, (T0, B), generator=g)
    toks = torch.randint(2, 729, (NSTEP, B), generator=g)
    with torch.no_grad():
        ref0, omems = X.forward_generate(params, s, ctx, None, M, same_length)
    rng = float(ref0.abs().max())
    states = {}
    for name, parity in (("bf16", False), ("parity", True)):
        model.parity_fp32 = parity
        st = DecodeState(model, B, M + 1, window=M)
        assert st.parity == parity
        st.prefill(ctx.to(DEV))
        states[name] = st
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    worst = {"bf16": 0.0, "parity": 0.0}
    bound = {"bf16": 2e-2, "parity": 1e-4}
    for step in range(NSTEP):
        with torch.no_grad():
            ref, omems = X.forward_generate(params, s, toks[step][None], omems, M, same_length)
        assert omems.shape[1] == min(M, T0 + step + 1)
        for name, st in states.items():
            lg = st.step(toks[step].to(DEV), ones, ones)[:, :729].float().cpu()
            err = float((lg - ref[0]).abs().max()) / rng
            worst[name] = max(worst[name], err)
            assert err < bound[name], (name, step, err)
    print(f"sliding cached step {shape} M {M} T0 {T0} steps {NSTEP} same_length {same_length}: worst logit error "
          f"bf16 {worst['bf16']:.2e}, parity {worst['parity']:.2e} of range {rng:.2f}")
    for st in states.values():
        assert st.klen.tolist() == [T0 + NSTEP] * B


# ------------------------------------------------------------------------------------------------ 4. / 5. greedy
@pytest.mark.parametrize("same_length", [True, False], ids=["same_length", "no_same_length"])
@pytest.mark.parametrize("std", [0.02, 0.09], ids=["init_std_0.02", "init_std_0.09"])
def test_free_running_greedy_parity_mode_token_exact_through_the_wraps(std, same_length):
    """L6 D512, memory of 96, context of 11 tokens, 320 FREE-RUNNING greedy steps in parity mode: the cached sliding step
    feeds on its own argmax, the oracle on its own; the sequences must be identical.  The test asserts its own premise
    too -- the achieved logit error x 2.5 stays below the smallest top-1 / top-2 gap the oracle saw -- so that a failure
    says whether the step or the premise broke."""
    from commu_amd.generate import DecodeState
    M, B, T0, NSTEP = 96, 3, 11, 320
    model, s, params = _short_model((6, 8, 512, 1024), M, 77, same_length, True, std=std)
    g = torch.Generator().manual_seed(1)
    ctx = torch.randint(2, 729, (T0, B), generator=g)
    ctx[0] = 0
    with torch.no_grad():
        ref, omems = X.forward_generate(params, s, ctx, None, M, same_length)
    st = DecodeState(model, B, M + 1, window=M)
    assert st.parity and st.kc.dtype == torch.float32
    st.prefill(ctx.to(DEV))
    otok = ref[-1].argmax(-1)
    tok = otok.to(DEV)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    min_gap, worst, rng = float("inf"), 0.0, float(ref.abs().max())
    seq, oseq = [otok.tolist()], [otok.tolist()]
    for step in range(NSTEP):
        with torch.no_grad():
            ref, omems = X.forward_generate(params, s, otok[None], omems, M, same_length)
        lg = st.step(tok, ones, ones)[:, :729]
        top2 = ref[0].topk(2, dim=-1).values
        min_gap = min(min_gap, float((top2[:, 0] - top2[:, 1]).min()))
        if seq == oseq:          # (the logits are comparable while the two trajectories agree)
            worst = max(worst, float((lg.cpu() - ref[0]).abs().max()))
        otok = ref[0].argmax(-1)
        tok = lg.argmax(-1)
        seq.append(tok.cpu().tolist())
        oseq.append(otok.tolist())
    print(f"sliding parity greedy (init std {std}, same_length {same_length}): {NSTEP} steps x {B} sequences, min top1-top2 "
          f"gap {min_gap / rng:.3e} of range, worst logit error {worst / rng:.2e} of range {rng:.2f}")
    assert worst * 2.5 < min_gap, "premise: the logit error must stay below the smallest gap"
    assert seq == oseq
    assert worst / rng < 1e-4
    assert st.klen.tolist() == [T0 + NSTEP] * B


@pytest.mark.parametrize("same_length", [True, False], ids=["same_length", "no_same_length"])
def test_bf16_greedy_agreement_through_the_wraps(same_length):
    """The bf16 sliding step at init std 0.02, teacher-forced on the oracle's greedy token: the argmax agrees at EVERY one
    of the 320 steps (the oracle's smallest top-1 / top-2 gap on this trajectory exceeds 2.5 x the 2e-2 logit bound,
    which the test asserts, so no step is excused)."""
    from commu_amd.generate import DecodeState
    M, B, T0, NSTEP = 96, 3, 11, 320
    model, s, params = _short_model((6, 8, 512, 1024), M, 77, same_length, False)
    g = torch.Generator().manual_seed(1)
    ctx = torch.randint(2, 729, (T0, B), generator=g)
    ctx[0] = 0
    with torch.no_grad():
        ref, omems = X.forward_generate(params, s, ctx, None, M, same_length)
    st = DecodeState(model, B, M + 1, window=M)
    assert not st.parity
    st.prefill(ctx.to(DEV))
    otok = ref[-1].argmax(-1)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    min_gap, worst, rng, bad = float("inf"), 0.0, float(ref.abs().max()), []
    for step in range(NSTEP):
        with torch.no_grad():
            ref, omems = X.forward_generate(params, s, otok[None], omems, M, same_length)
        lg = st.step(otok.to(DEV), ones, ones)[:, :729].float().cpu()
        top2 = ref[0].topk(2, dim=-1).values
        min_gap = min(min_gap, float((top2[:, 0] - top2[:, 1]).min()))
        worst = max(worst, float((lg - ref[0]).abs().max()))
        if not torch.equal(lg.argmax(-1), ref[0].argmax(-1)):
            bad.append(step)
        otok = ref[0].argmax(-1)
    print(f"sliding bf16 greedy (same_length {same_length}): min gap {min_gap / rng:.3f} of range, worst logit error "
          f"{worst / rng:.2e} of range {rng:.2f}, mismatching steps {bad}")
    assert min_gap / rng > 2.5 * 2e-2, "premise: the oracle's gaps must exceed the bf16 logit bound"
    assert worst / rng < 2e-2
    assert not bad


# ------------------------------------------------------------------------------------------------ 6. the whole loop
def _sliding_decoder(model, z, tags, M, glen, record_trace=True):
    from commu_amd.generate import ForcedDecoder
    import test_decode_gpu as TD
    temp, _, top_k, _ = z[f"{tags[0]}_cfg"]
    dec = ForcedDecoder(model, len(tags), glen, M, float(temp), int(top_k), record_trace=record_trace, sliding=True)
    uni = np.full((len(tags), dec.ld_u), 0.5, dtype=np.float32)
    for b, t in enumerate(tags):
        u = z[f"{t}_uniforms"]
        uni[b, :len(u)] = u
    meta = z["encoded_meta"].tolist()
    dec.load([meta] * len(tags), [TD._data(z, t) for t in tags], uni)
    return dec


def _oracle_loop(z, tag, M, glen):
    """oracle.decode_ref.generate_sequence driven by oracle.xl_ref.forward_generate with a memory of M, as
    tests/test_oracle_golden.py drives it with 4146: (sequence, [(fed token, memory before, after)], kept steps, last
    logits)."""
    from test_oracle_golden import params_of, shape_of
    s, p = shape_of(z["meta"]), params_of(z)
    p["crit.out_layers.0.bias"] = torch.from_numpy(z[f"{tag}_bias"]).clone()
    temp, nm, top_k, _ = z[f"{tag}_cfg"]
    meta = [int(t) for t in z["encoded_meta"]]
    calls, last = [], []

    def step(tok, mems):
        with torch.no_grad():
            lg, nm_ = X.forward_generate(p, s, torch.tensor([[int(tok)]]), mems, M, True)
        calls.append((int(tok), mems.shape[1], nm_.shape[1]))
        last[:] = [lg[-1, 0].double()]
        return lg[-1, 0], nm_

    with torch.no_grad():
        _, mems = X.forward_generate(p, s, torch.tensor([0] + meta[:10])[:, None], None, M, True)
    kept = []
    out = Dz.generate_sequence(step, [0] + meta, mems, chord_token=[int(t) for t in z[f"{tag}_chord_token"]],
                               chord_position=[int(t) for t in z[f"{tag}_chord_position"]], num_measures=float(nm),
                               temperature=float(temp), top_k=int(top_k), uniforms=list(z[f"{tag}_uniforms"]),
                               max_iters=int(glen), trace=kept)
    return out, calls, sum(int(k) for _, k in kept), last[0]


@pytest.mark.parametrize("parity", [False, True], ids=["bf16", "parity_fp32"])
@pytest.mark.parametrize("M", [96, 48])
def test_forced_loop_with_sliding_memory_vs_oracle(golden_dir, M, parity):
    """The greedy G6 fixtures (greedy8, greedy5) through ForcedDecoder(..., memory_length=M, sliding=True): the sequences
    run 200 - 260 model steps, several times round the ring.  Sequences and model-step traces (quirks Q3 / Q4) exact; the
    final klen is the ABSOLUTE count context + kept steps (beyond the ring size); the logits after the last iteration match
    the oracle's last logits with the engineered output bias removed on both sides (bf16 <= 2e-2, parity <= 1e-4 of the
    remaining range) -- the tokens alone would not notice a wrong window, the bias dominates them.  Then 64 sequences
    alternating the two fixtures: graph replay equals eager launches bit for bit and every sequence is the oracle's."""
    import test_decode_gpu as TD
    z = load(golden_dir, "g6_decode.npz")
    assert np.array_equal(z["greedy8_bias"], z["greedy5_bias"])
    model = TD._build(golden_dir, z, z["greedy8_bias"])
    model.reset_length(1, M)
    model.parity_fp32 = parity
    bias = torch.from_numpy(z["greedy8_bias"]).double()
    for tag in ("greedy8", "greedy5"):
        glen = int(z[f"{tag}_cfg"][3])
        oseq, ocalls, okept, olast = _oracle_loop(z, tag, M, glen)
        assert oseq == z[f"{tag}_seq"].tolist()          # (the engineered bias dominates: the unlimited-memory tokens)
        assert len(ocalls) > 2 * (M + 1) and ocalls[-1][1:] == (M, M), "the fixture must wrap the ring"
        dec = _sliding_decoder(model, z, [tag], M, glen)
        assert dec.state.parity == parity and dec.state.window == M and dec.state.Lmax == M + 1
        with torch.no_grad():
            dec.run(use_graph=False)
        seqs, traces = dec.sequences()
        assert seqs[0] == oseq, tag
        assert traces[0] == ocalls, tag
        assert int(dec.state.klen[0]) == 11 + okept and 11 + okept > M + 1, tag
        got = dec.state.logits[0, :729].double().cpu() - bias
        want = olast - bias
        err = float((got - want)[1:].abs().max()) / float(want[1:].abs().max())
        print(f"sliding forced loop {tag} M {M} parity {parity}: {len(ocalls)} model steps, klen {int(dec.state.klen[0])}, "
              f"last-logits error {err:.2e} of range (bias removed)")
        assert err < (1e-4 if parity else 2e-2), tag
    tags = ["greedy8", "greedy5", "greedy5", "greedy8"] * 16
    # (one generation_length for the batch: the shorter fixture runs on to it, in the oracle too)
    glen = max(int(z[f"{t}_cfg"][3]) for t in ("greedy8", "greedy5"))
    oracle = {tag: _oracle_loop(z, tag, M, glen) for tag in ("greedy8", "greedy5")}
    results = []
    for use_graph in (True, False):
        dec = _sliding_decoder(model, z, tags, M, glen)
        with torch.no_grad():
            dec.run(use_graph=use_graph)
        torch.cuda.synchronize()
        results.append((dec.seq.clone(), dec.fsm.clone(), dec.state.logits.clone(), dec.state.klen.clone(), dec.sequences()))
    (sg, fg, lg, kg, outg), (se, fe, le, ke, _) = results
    assert torch.equal(sg, se) and torch.equal(fg, fe) and torch.equal(kg, ke)
    assert torch.equal(lg, le)
    seqs, traces = outg
    for b, tag in enumerate(tags):
        oseq, ocalls, okept, _ = oracle[tag]
        assert seqs[b] == oseq and traces[b] == ocalls, (b, tag)
        assert int(kg[b]) == 11 + okept, (b, tag)


def test_both_step_implementations_work_on_the_ring():
    """The layer-tail launches and the chain of per-Linear launches (USE_LAYER_TAIL) on a ring that wraps: both within the
    bf16 bound of the oracle at every step, 64 sequences (the layer tail's shape), memory of 48, 120 steps."""
    from commu_amd import generate as G
    M, B, T0, NSTEP = 48, 64, 11, 120
    model, s, params = _short_model((6, 8, 512, 1024), M, 41, True, False)
    g = torch.Generator().manual_seed(5)
    ctx = torch.randint(2, 729, (T0, B), generator=g)
    toks = torch.randint(2, 729, (NSTEP, B), generator=g)
    with torch.no_grad():
        ref0, omems = X.forward_generate(params, s, ctx, None, M, True)
        rng = float(ref0.abs().max())
        refs = []
        for step in range(NSTEP):
            ref, omems = X.forward_generate(params, s, toks[step][None], omems, M, True)
            refs.append(ref[0])
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    for tail in (True, False):
        G.USE_LAYER_TAIL = tail
        try:
            st = G.DecodeState(model, B, M + 1, window=M)
            if tail:
                assert st.tail_ok
            st.prefill(ctx.to(DEV))
            worst = 0.0
            for step in range(NSTEP):
                lg = st.step(toks[step].to(DEV), ones, ones)[:, :729].float().cpu()
                worst = max(worst, float((lg - refs[step]).abs().max()) / rng)
            st.check()
        finally:
            G.USE_LAYER_TAIL = True
        print(f"ring decode, layer tail {tail}: worst logit error {worst:.2e} of range")
        assert worst < 2e-2


# ------------------------------------------------------------------------------------------------ 7. re-arm after a wrap
def test_generate_stream_rearms_a_slot_whose_ring_has_wrapped():
    """generate_stream with sliding=True, memory_length 32, generation_length 96 (every attempt goes three times round its
    ring and overwrites its context rows), 8 slots, 24 attempts, sampled: the result equals the same attempts decoded
    from fresh decoders, in attempt order.  A re-armed slot must get its context rows back."""
    from commu_amd.generate import BatchedGenerator, ForcedDecoder
    from test_configs_gpu import build
    M, GL = 32, 96
    model, cfg, s, params = build(6, 8, 512, 1024, 1, M, seed=37)
    model.eval()
    model.same_length = True
    model.reset_length(1, M)
    with torch.no_grad():
        bias = model.crit.out_layers[0].bias
        bias.zero_()
        bias[1:3] = -1e9                      # no EOS / BAR, no chord tokens: every attempt runs its 96 iterations
        bias[195:304] = -1e9
    meta = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=GL, memory_length=M, sliding=True)
    out, started = gen.generate_stream(meta, data, 0.95, 32, need=24, accept=lambda seq, rep: True, slots=8, seed=11)
    assert len(out) == 24 and 24 <= started <= 32
    assert all(s_ is not None and s_[:12] == [0] + meta and len(s_) == 12 + GL for s_ in out)
    for first in (0, 8, 16):
        dec = ForcedDecoder(model, 8, generation_length=GL, memory_length=M, temperature=0.95, top_k=32, sliding=True)
        uni = np.stack([BatchedGenerator.attempt_uniforms(11, first + b, dec.ld_u) for b in range(8)])
        dec.load([meta] * 8, [data] * 8, uni)
        with torch.no_grad():
            dec.run(use_graph=False)
        assert int(dec.state.klen.min()) > M + 1
        assert out[first:first + 8] == dec.sequences()[0], first
    assert len({tuple(s_) for s_ in out}) > 4


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_sliding_refusals(golden_dir):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import DecodeState, ForcedDecoder
    import test_decode_gpu as TD
    z = load(golden_dir, "g6_decode.npz")
    model = TD._build(golden_dir, z, z["greedy8_bias"])
    with pytest.raises(CommuHipError):
        ForcedDecoder(model, 2, generation_length=300, memory_length=DecodeState.MAX_POSITIONS, temperature=0.0, top_k=32,
                      sliding=True)
    with pytest.raises(CommuHipError):
        ForcedDecoder(model, 2, generation_length=300, memory_length=15, temperature=0.0, top_k=32, sliding=True)
    ForcedDecoder(model, 2, generation_length=300, memory_length=16, temperature=0.0, top_k=32, sliding=True)
    B, H, DH, W = 2, 4, 64, 33
    HD = H * DH
    bf, f32 = torch.bfloat16, torch.float32
    qkv = torch.zeros(B, 3 * HD, dtype=bf, device=DEV)
    kc, vc = torch.zeros(B, H, W, DH, dtype=bf, device=DEV), torch.zeros(B, H, W, DH, dtype=bf, device=DEV)
    rd = torch.zeros(W, HD, dtype=bf, device=DEV)
    u, vb = torch.zeros(HD, device=DEV), torch.zeros(HD, device=DEV)
    klen = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = torch.zeros(B, HD, dtype=bf, device=DEV)
    ops.decode_attn_ring(qkv, kc, vc, rd, u, vb, klen, None, out, W, 0.125)          # the well-formed call
    bad = [
        dict(kc=kc.float()),                                     # dtype
        dict(kc=kc.cpu()),                                       # device
        dict(klen=klen.long()),
        dict(W=W + 1),                                           # W does not match the cache
        dict(rd=rd[:W - 1]),                                     # distance table too short
        dict(qkv=qkv[:, :HD]),
    ]
    for kw in bad:
        a = dict(qkv=qkv, kc=kc, vc=vc, rd=rd, u=u, vb=vb, klen=klen, active=None, out=out, W=W, scale=0.125)
        a.update(kw)
        with pytest.raises(CommuHipError):
            ops.decode_attn_ring(**a)
    big = torch.zeros(1, 1, 4225, 64, dtype=bf, device=DEV)
    with pytest.raises(CommuHipError):
        ops.decode_attn_ring(qkv[:1, :192], big, big, torch.zeros(4225, 64, dtype=bf, device=DEV), u, vb, klen[:1], None,
                             out[:1, :64], 4225, 0.125)
    with pytest.raises(CommuHipError):
        ops.decode_kv_append_ring(qkv, kc.float(), vc, klen, None, W)
    with pytest.raises(CommuHipError):
        ops.decode_kv_append_ring(qkv, kc, vc, klen, None, 1)
    kf, qf = torch.zeros(B, W, HD, device=DEV), torch.zeros(B, 3 * HD, device=DEV)
    ops.decode_kv_append_ring_f32(qf, kf, kf.clone(), klen, None, HD, W)
    with pytest.raises(CommuHipError):
        ops.decode_kv_append_ring_f32(qf, kf.to(bf), kf, klen, None, HD, W)
    with pytest.raises(CommuHipError):
        ops.decode_kv_append_ring_f32(qf, kf, kf, klen, None, HD, W + 1)
    with pytest.raises(CommuHipError):
        ops.decode_attn_ring_f32(qf[:, :HD], kf, kf, rd.float(), u, vb, klen, H, DH, W + 1, True, 0.125)
    with pytest.raises(CommuHipError):
        ops.decode_attn_ring_f32(qf[:, :HD], kf, kf, rd.float()[:W - 1], u, vb, klen, H, DH, W, True, 0.125)
    with pytest.raises(CommuHipError):
        ops.decode_attn_ring_f32(qf[:, :HD].cpu(), kf, kf, rd.float(), u, vb, klen, H, DH, W, True, 0.125)


# ------------------------------------------------------------------------------------------------ the command line
def test_generate_cli_sliding_memory(golden_dir, tmp_path):
    """`generate.py --memory_length 64 --generation_length 300 --sliding_memory` end to end on the reference-written
    checkpoint: the decoder the run builds slides (ring of 65 rows), sequences.json is written, and two greedy runs agree;
    the same command line WITHOUT --sliding_memory is refused with the decode-memory error, as before."""
    import json
    import test_model_gpu as TM
    from commu_amd import generate as G
    from commu_amd._lib import CommuHipError
    z = load(golden_dir, "g10_checkpoint.npz")
    cli = TM._load_script("generate")
    parsers = cli.parse_args()
    prog = "-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8)
    argv = ["--checkpoint_dir", os.path.join(golden_dir, "g10_checkpoint.pt"), "--output_dir", str(tmp_path / "out"),
            "--memory_length", "64", "--generation_length", "300",
            "--bpm", "70", "--audio_key", "aminor", "--time_signature", "4/4", "--pitch_range", "mid_high",
            "--num_measures", "8", "--inst", "acoustic_piano", "--genre", "newage", "--min_velocity", "60",
            "--max_velocity", "80", "--track_role", "main_melody", "--rhythm", "standard", "--chord_progression",
            prog + "-" + prog, "--num_generate", "1", "--max_rounds", "1", "--temperature", "0", "--gpus", "1"]
    iargs, _ = parsers["input_args"].parse_known_args(argv)
    margs, _ = parsers["model_args"].parse_known_args(argv)
    assert not margs.sliding_memory
    with pytest.raises(CommuHipError, match="exceeds the decode memory"):
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
    margs, _ = parsers["model_args"].parse_known_args(argv + ["--sliding_memory"])
    assert margs.sliding_memory and margs.memory_length == 64 and margs.generation_length == 300
    built = []
    orig_init = G.ForcedDecoder.__init__

    def spy(self, *a, **kw):
        orig_init(self, *a, **kw)
        built.append(self)
    G.ForcedDecoder.__init__ = spy
    try:
        outs = []
        for _ in range(2):
            cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
            outs.append(json.load(open(tmp_path / "out" / "sequences.json")))
    finally:
        G.ForcedDecoder.__init__ = orig_init
    assert built and all(d.sliding and d.state.window == 64 and d.state.Lmax == 65 and d.generation_length == 300
                         for d in built)
    print(f"generate.py --sliding_memory: final memory lengths {built[-1].state.klen.tolist()} on a ring of 65 rows, "
          f"{len(outs[0]['sequences'])} sequence(s) accepted")
    assert outs[0] == outs[1] and outs[0]["encoded_meta"][0] == 574
