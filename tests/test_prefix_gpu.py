"""The shared prompt prefix on the GPU (csrc/decode_prefix.hip, DecodeState(shared_prefix=), ForcedDecoder(shared_prompt=True)):
the kernel against the float64 contract on the input sets of tests/prefix_contract.py (tests/test_prefix_contract_host.py
proves on the CPU that those sets catch every planted defect), the prefix prefill against prefill_ragged, and the shared
decoder end to end: the reference's greedy fixtures, the unshared decoder and the oracle, graph replay across loads,
re-arm, refusals."""
import os
import types

import numpy as np
import pytest
import torch

import decode_contract as DC
import prefix_contract as PC
import prime_contract as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 768.0          # (exact in bf16)
H = DC.H
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]
SETS = PC.all_sets()


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "g6_decode.npz"))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("idx", range(len(SETS)), ids=[s[0] for s in SETS])
def test_prefix_decode_attention_vs_float64_contract(idx):
    """commu_decode_attn_prefix on every set: each output element within 2^-8 |want| + c A of the float64 contract (the
    bound of decode_contract, unchanged).  Guards: append off and on -- the new token's private row holds NaN before the
    call and exactly the K/V columns of qkv after it, every other cache element and the prefix bit-identical --; prefix
    rows >= P, private rows beyond the new token, distance rows beyond the largest distance, the pad columns and the
    record workspace hold NaN; the inactive slot's row of out is untouched; three launches in a row, all pair counters
    zero after each.  The launch is sized for Pcap (three chunks) and B = 5 slots (not a multiple of the group)."""
    from commu_amd import ops
    assert ops.decode_prefix_chunk() == PC.CH and ops.decode_prefix_group() == PC.G and PC.B % PC.G
    s = PC.build(**SETS[idx][1])
    HD = H * s.DH
    want, A = s.evaluate()
    rows = [b for b in range(s.B) if s.active[b]]
    idle = [b for b in range(s.B) if not s.active[b]]
    qkv, rd, u, vb = s.qkv.to(DEV), s.rd.to(DEV), s.u.to(DEV), s.vb.to(DEV)
    klen, active = s.klen.to(DEV), s.active.to(DEV)
    pk, pv = s.pk.to(DEV), s.pv.to(DEV)
    plen = torch.tensor([s.P], dtype=torch.int32, device=DEV)
    kc1, vc1 = s.kc.to(DEV), s.vc.to(DEV)
    ws = torch.full((ops.decode_prefix_ws_floats(s.B, H, s.DH, s.Pcap, s.nsplit),), float("nan"), device=DEV)
    cnt = torch.zeros(s.B * H, dtype=torch.int32, device=DEV)
    worst = 0.0
    for append in (False, True):
        for rep in range(3):
            kc, vc = (t.to(DEV) for t in s.caches_before(append))
            out = torch.full((s.B, HD + DC.PAD), SENT, device=DEV, dtype=torch.bfloat16)
            ops.decode_attn_prefix(qkv, pk, pv, plen, kc, vc, rd, u, vb, klen, active, out, s.scale, ws, cnt, append=append,
                                   nsplit=s.nsplit)
            torch.cuda.synchronize()
            what = (SETS[idx][0], append, rep)
            assert int(cnt.abs().sum()) == 0, what
            assert _same_bits(kc, kc1) and _same_bits(vc, vc1), (what, "private caches")          # the append, bit for bit
            assert _same_bits(pk, s.pk.to(DEV)) and _same_bits(pv, s.pv.to(DEV)), (what, "prefix")
            o = out.cpu()
            assert bool((o[:, HD:] == SENT).all()), (what, "pad columns of out")
            assert bool((o[idle] == SENT).all()), (what, "inactive slot")
            got = o[:, :HD].view(s.B, H, s.DH)[rows]
            r = DC.ratio(got, want[rows], A[rows]).nan_to_num(nan=float("inf"))
            worst = max(worst, float(r.max()))
            if not bool((r <= 1).all()):
                i = int(r.argmax())
                b, h, e = i // (H * s.DH), i // s.DH % H, i % s.DH
                raise AssertionError(f"{what}: error {float(r.max()):.2f} x the bound at slot {rows[b]} (klen "
                                     f"{int(s.klen[rows[b]])}, P {s.P}) head {h} element {e}: got {float(got[b, h, e])}, "
                                     f"want {float(want[rows[b], h, e])}")
    print(f"commu_decode_attn_prefix {SETS[idx][0]}: worst error {worst:.3f} of the per-element bound")


# ------------------------------------------------------------------------------------------------ models
def _model_dh32(golden_dir, z, tag="greedy8"):
    import test_prime_gpu as TP
    return TP._fixture_model(golden_dir, z, tag)


def _model_dh64():
    from test_configs_gpu import build
    model = build(2, 2, 128, 256, 1, 4146, seed=3)[0]
    model.eval()
    model.same_length = True
    model.reset_length(1, 4146)
    return model


def _data(z, tag):
    return types.SimpleNamespace(num_measures=float(z[f"{tag}_cfg"][1]), chord_token_components={
        "chord_token": z[f"{tag}_chord_token"].tolist(), "chord_position": z[f"{tag}_chord_position"].tolist()})


# ------------------------------------------------------------------------------------------------ 2. the prefix prefill
@pytest.mark.parametrize("kind", ["dh32", "dh64"])
def test_prefill_shared_equals_the_rows_prefill_ragged_writes(golden_dir, z, kind):
    """pk / pv of one column of 37 tokens, bit for bit the rows that prefill_ragged writes for that column; prefix_len = 37,
    klen = 0, rows beyond stay as they were; cache_bytes() = prefix + private bytes."""
    from commu_amd.generate import DecodeState
    model = _model_dh32(golden_dir, z) if kind == "dh32" else _model_dh64()
    T, Pcap, Lp, B = 37, 50, 24, 3
    col = torch.randint(2, 729, (T,), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        ref = DecodeState(model, 1, 48)
        ref.prefill_ragged(col[:, None].contiguous(), [T])
        st = DecodeState(model, B, Lp, shared_prefix=Pcap)
        st.klen.fill_(9)
        st.prefill_shared(col)
    torch.cuda.synchronize()
    assert st.pk.shape == (model.n_layer, model.n_head, Pcap, model._DHp) and st.kc.shape[1:4] == (B, model.n_head, Lp)
    assert int(st.prefix_len) == T and st.klen.tolist() == [0] * B
    assert _same_bits(st.pk[:, :, :T], ref.kc[:, 0, :, :T]) and _same_bits(st.pv[:, :, :T], ref.vc[:, 0, :, :T])
    assert not _bits(st.pk[:, :, T:]).any() and not _bits(st.pv[:, :, T:]).any() and bool(_bits(st.pk).any())
    assert st.cache_bytes() == 2 * 2 * (st.pk.numel() + st.kc.numel())
    assert st.cache_bytes() == 2 * 2 * model.n_layer * model.n_head * model._DHp * (Pcap + B * Lp)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _shared_decoder(model, z, tag, B, glen, max_prompt, shared=True, record_trace=False):
    from commu_amd.generate import ForcedDecoder
    temp, _, top_k, _ = z[f"{tag}_cfg"]
    return ForcedDecoder(model, B, glen, 4146, float(temp), int(top_k), record_trace=record_trace, max_prompt=max_prompt,
                         **({"shared_prompt": True} if shared else {}))


def _load(dec, z, tag, prompt, uniforms=None):
    uni = np.full((dec.B, dec.ld_u), 0.5, dtype=np.float32)
    if uniforms is not None:
        n = min(uniforms.shape[1], dec.ld_u)
        uni[:, :n] = uniforms[:, :n]
    dec.load([META] * dec.B, [_data(z, tag)] * dec.B, uni, prompts=None if prompt is None else [list(prompt)] * dec.B)


@pytest.mark.parametrize("tag", ["greedy8", "greedy5"])
def test_primed_continuation_through_the_shared_decoder_reproduces_the_reference(golden_dir, z, tag):
    """ONE shared decoder of two slots, its graph captured once, loaded with four cuts of the fixture's sequence one after
    the other (different P each time): every continuation equals the reference's sequence and trace, token for token
    (the fixture's top-1 / top-2 gap is > 0.1).  The slots hold no private rows after load(), the prefix holds the
    context plus the kept tokens of the replayed stream."""
    assert float(z[f"{tag}_min_gap"]) > 0.1
    model = _model_dh32(golden_dir, z, tag)
    ctx, ct, cp, nm, p = P.fixture(z, tag)
    glen = int(z[f"{tag}_cfg"][3])
    ref = z[f"{tag}_seq"].tolist()
    ref_trace = [tuple(t) for t in z[f"{tag}_trace"].tolist()]
    cuts = P.cut_points(p)
    cuts = sorted({cuts[0], cuts[len(cuts) // 2], cuts[-2], cuts[-1]})
    dec = _shared_decoder(model, z, tag, 2, glen, max(1, len(p)), record_trace=True)
    graph = None
    for k in cuts:
        _load(dec, z, tag, p[:k])
        _, _, fed, _ = P.replay(ctx, ct, cp, nm, p[:k])
        assert dec.state.klen.tolist() == [0, 0] and dec.prefix_P == int(dec.state.prefix_len) == len(ctx) - 1 + len(P.kept(fed))
        with torch.no_grad():
            dec.run(use_graph=True)
        assert graph is None or dec.graph is graph, "one captured graph serves every load"
        graph = dec.graph
        seqs, traces = dec.sequences()
        for b in range(2):
            assert seqs[b][:len(ref)] == ref and len(seqs[b]) >= len(ref), (k, b)
            assert traces[b][:len(ref_trace)] == ref_trace, (k, b)


def test_one_graph_two_loads_equal_eager_runs(golden_dir, z):
    """sample8m's variates, three slots: the graph captured for the first load (a short prompt) is replayed for a second
    load with a longer prompt (another P); both give the tokens, records and logits of eager runs bit for bit."""
    tag = "sample8m"
    model = _model_dh32(golden_dir, z, tag)
    p = P.fixture(z, tag)[4]
    uni = np.stack([np.resize(z[f"{tag}_uniforms"][30 + 7 * b:].astype(np.float32), 61) for b in range(3)])
    dg = _shared_decoder(model, z, tag, 3, 60, len(p))
    de = _shared_decoder(model, z, tag, 3, 60, len(p))
    seen = []
    for k in (3, 40):
        for dec, use_graph in ((dg, True), (de, False)):
            _load(dec, z, tag, p[:k], uni)
            with torch.no_grad():
                dec.run(use_graph=use_graph)
        torch.cuda.synchronize()
        assert torch.equal(dg.seq, de.seq) and torch.equal(dg.fsm, de.fsm) and torch.equal(dg.state.klen, de.state.klen)
        assert torch.equal(dg.state.logits, de.state.logits)
        seen.append(int(dg.state.prefix_len))
        for s_ in dg.sequences()[0]:
            assert s_[:12 + k] == [0] + META + p[:k] and len(s_) > 12 + k
    assert seen[0] < seen[1]
    assert len({tuple(s_) for s_ in dg.sequences()[0]}) > 1, "different variates should give different continuations"


def test_rearmed_shared_slot_repeats_a_fresh_load(golden_dir, z):
    """A finished slot of a shared decoder that is re-armed (record and trace back to the primed state, klen = 0, no rows
    to restore) produces, with the same variates, bit for bit the seq of a fresh load()."""
    tag = "sample8m"
    model = _model_dh32(golden_dir, z, tag)
    p = P.fixture(z, tag)[4]
    B, k, glen = 3, 40, 60
    uni = np.stack([np.resize(z[f"{tag}_uniforms"][30 + 5 * b:].astype(np.float32), glen + 1) for b in range(B)])
    fresh = _shared_decoder(model, z, tag, B, glen, len(p), record_trace=True)
    _load(fresh, z, tag, p[:k], uni)
    with torch.no_grad():
        fresh.run()
    want_seq, want_fsm, want_klen = fresh.seq.clone(), fresh.fsm.clone(), fresh.state.klen.clone()
    assert bool(want_fsm[:, 5].all()) and int(want_klen.min()) > 0
    dec = _shared_decoder(model, z, tag, B, glen, len(p), record_trace=True)
    _load(dec, z, tag, p[:k], uni)
    with torch.no_grad():
        dec.run()
        pk0 = dec.state.pk.clone()
        for b in range(B):
            dec.rearm(b, uni[b])
        assert dec.state.klen.tolist() == [0] * B
        assert dec.fsm[1].tolist() == P.replay(*P.fixture(z, tag)[:4], p[:k])[0]
        dec.run()
    assert torch.equal(dec.seq, want_seq) and torch.equal(dec.fsm, want_fsm) and torch.equal(dec.state.klen, want_klen)
    assert _same_bits(dec.state.pk, pk0)
    assert dec.sequences()[1] == fresh.sequences()[1]


@pytest.mark.parametrize("shape", [(2, 4, 128, 256), (2, 4, 256, 512)], ids=["L2_D128_dh32", "L2_D256_dh64"])
def test_shared_decoder_sits_as_close_to_the_oracle_as_the_unshared_one(shape):
    """L2 D128 H4 (d_head 32) and L2 D256 H4 (d_head 64), B = 4 slots, one prompt, per-slot variates; 32 eager iterations of an unshared and a shared
    decoder, every active slot's logits of every iteration against oracle.xl_ref.forward_generate (fp32, the whole memory
    recomputed per step) fed the unshared decoder's own tokens.  Distance = max |logits - oracle| / oracle's logit range
    over all slots, iterations and the 729 tokens.  The unshared bf16 path is measured first; the shared path's distance
    must be within 1.5 x of it (the summation order differs, the arithmetic does not).  The tokens the two decoders feed
    are the same in all 32 iterations.
    The decoders run at temperature 1: the sampling step leaves logits / temperature in the buffer that is read here.
    Measured on an MI355X: d_head 32: unshared 2.086e-03, shared 2.021e-03 of the logit range (3.08); d_head 64: unshared
    1.398e-03, shared 1.398e-03 (5.52)."""
    from commu_amd.generate import ForcedDecoder
    from oracle import xl_ref as X
    from test_configs_gpu import build
    model, cfg, s, params = build(*shape, 1, 4146, seed=11)
    model.eval()
    model.same_length = True
    model.reset_length(1, 4146)
    with torch.no_grad():
        bias = model.crit.out_layers[0].bias
        bias.zero_()
        bias[1] = bias[2] = -1e9          # no EOS: every slot steps in every iteration
        bias[195:304] = -1e9
        params["crit.out_layers.0.bias"] = bias.detach().float().cpu().clone()
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
    prompt = [500, 64, 310, 520, 70]
    B, GL, NIT = 4, 40, 32
    uni = np.stack([np.random.RandomState(100 + b).random_sample(GL + 1).astype(np.float32) for b in range(B)])
    decs = {}
    for shared in (False, True):
        # (temperature 1: the sampling step leaves logits / temperature in the buffer that is compared below)
        dec = ForcedDecoder(model, B, GL, 4146, 1.0, 32, max_prompt=len(prompt), **({"shared_prompt": True} if shared else {}))
        dec.load([META] * B, [data] * B, uni, prompts=[prompt] * B)
        decs[shared] = dec
    un, sh = decs[False], decs[True]
    nfed = int(un.state.klen[0]) - len(META)
    column = torch.tensor([0] + META[:-1] + un.fed[0, :nfed].tolist(), dtype=torch.long)
    assert int(sh.state.prefix_len) == len(column)
    with torch.no_grad():
        _, mem0 = X.forward_generate(params, s, column[:, None], None, 4146, True)
    mems = [mem0 for _ in range(B)]
    dist = {False: 0.0, True: 0.0}
    rng = 0.0
    with torch.no_grad():
        for it in range(NIT):
            for dec in (un, sh):
                dec.pre()
            assert torch.equal(un.tok, sh.tok) and torch.equal(un.active, sh.active) and torch.equal(un.keep, sh.keep), it
            tok, act, keep = un.tok.cpu(), un.active.cpu(), un.keep.cpu()
            for dec in (un, sh):
                dec.body()
            lg = {k: d.state.logits[:, :729].float().cpu() for k, d in decs.items()}
            for b in range(B):
                if not act[b]:
                    continue
                ref, new = X.forward_generate(params, s, tok[b].view(1, 1), mems[b], 4146, True)
                if keep[b]:
                    mems[b] = new
                ok = torch.isfinite(ref[0, 0]) & (ref[0, 0] > -1e8)
                rng = max(rng, float(ref[0, 0][ok].abs().max()))
                for k in (False, True):
                    dist[k] = max(dist[k], float((lg[k][b] - ref[0, 0])[ok].abs().max()))
    d_un, d_sh = dist[False] / rng, dist[True] / rng
    print(f"{shape}: distance to the oracle over {NIT} iterations x {B} slots: unshared {d_un:.3e}, shared {d_sh:.3e} of the logit "
          f"range {rng:.3f}")
    assert d_un > 0
    assert d_sh <= 1.5 * d_un


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_say_what_is_wrong(golden_dir, z):
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import BatchedGenerator, DecodeState, ForcedDecoder
    tag = "greedy8"
    model = _model_dh32(golden_dir, z, tag)
    p = P.fixture(z, tag)[4]
    free0 = torch.cuda.memory_allocated()
    with pytest.raises(CommuHipError, match=r"shared_prefix with a sliding window"):
        DecodeState(model, 2, 0, window=32, shared_prefix=64)
    with pytest.raises(CommuHipError, match=r"shared_prefix with kv_dtype='fp8'"):
        DecodeState(model, 2, 40, kv_dtype="fp8", shared_prefix=64)
    model.parity_fp32 = True
    try:
        with pytest.raises(CommuHipError, match=r"shared_prefix with the fp32 parity mode"):
            DecodeState(model, 2, 40, shared_prefix=64)
        with pytest.raises(CommuHipError, match=r"parity"):
            ForcedDecoder(model, 2, 40, 4146, 0.0, 32, max_prompt=8, shared_prompt=True)
    finally:
        model.parity_fp32 = False
    with pytest.raises(CommuHipError, match=r"4000 positions and 300 private rows need 4300 positions.*supports 4224"):
        DecodeState(model, 2, 300, shared_prefix=4000)
    assert torch.cuda.memory_allocated() == free0, "refused before any allocation"
    with pytest.raises(CommuHipError, match=r"shared_prompt.*max_prompt > 0"):
        ForcedDecoder(model, 2, 40, 4146, 0.0, 32, shared_prompt=True)
    with pytest.raises(CommuHipError, match=r"sliding window"):
        ForcedDecoder(model, 2, 40, 64, 0.0, 32, sliding=True, max_prompt=8, shared_prompt=True)
    with pytest.raises(CommuHipError, match=r"fp8"):
        ForcedDecoder(model, 2, 40, 4146, 0.0, 32, kv_dtype="fp8", max_prompt=8, shared_prompt=True)
    dec = ForcedDecoder(model, 3, 40, 4146, 0.0, 32, max_prompt=20, shared_prompt=True)
    assert dec.state.shared_prefix == 16 + 16 + 2 * 20 and dec.state.Lmax == 42 and dec.state.klen_cap == 42
    datas = [_data(z, tag)] * 3
    with pytest.raises(CommuHipError, match=r"slot 2 differs from slot 0 in its prompt"):
        dec.load([META] * 3, datas, prompts=[p[:5], p[:5], p[:6]])
    with pytest.raises(CommuHipError, match=r"slot 1 differs from slot 0 in its encoded_meta"):
        dec.load([META, META[:-1] + [726], META], datas, prompts=[p[:5]] * 3)
    other = _data(z, tag)
    other.chord_token_components = dict(other.chord_token_components)
    other.chord_token_components["chord_token"] = list(other.chord_token_components["chord_token"])
    other.chord_token_components["chord_token"][0] += 1
    with pytest.raises(CommuHipError, match=r"slot 1 differs from slot 0 in its chord tokens"):
        dec.load([META] * 3, [datas[0], other, datas[0]], prompts=[p[:5]] * 3)
    dec.load([META] * 3, datas, prompts=[p[:5]] * 3)          # (usable after a refusal)
    assert int(dec.state.prefix_len) > len(META) and dec.state.klen.tolist() == [0, 0, 0]
    dec.load([META] * 3, datas)                               # no prompts: the conditioning context is what is shared
    assert int(dec.state.prefix_len) == len(META) and dec.prefix_P == len(META) and dec.state.klen.tolist() == [0, 0, 0]
    # the shared positions plus generation_length must fit the decode memory
    short = ForcedDecoder(model, 2, 40, 60, 0.0, 32, max_prompt=20, shared_prompt=True)
    _, _, fed, _ = P.replay(*P.fixture(z, tag)[:4], p[:20])
    n = 11 + len(P.kept(fed))
    with pytest.raises(CommuHipError, match=rf"starts with {n} shared positions.*needs {n + 41}.*has 61"):
        short.load([META] * 2, datas[:2], prompts=[p[:20]] * 2)
    gen = BatchedGenerator(model, torch.device(DEV), generation_length=40)
    with pytest.raises(CommuHipError, match=r"share_prompt: there is no prompt to share"):
        gen.generate_stream(META, datas[0], 0.0, 32, need=2, accept=lambda s_, r: True, share_prompt=True)


def test_generate_cli_share_prompt_refusals(tmp_path):
    """generate.py --share_prompt: listed by --help; refused without --prompt_tokens and with --sliding_memory,
    --kv_cache fp8 or --parity, before anything is loaded."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("generate_cli_share", os.path.join(root, "commu-code_amd", "generate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    parsers = cli.parse_args()
    assert "--share_prompt" in parsers["model_args"].format_help()
    assert parsers["model_args"].parse_known_args([])[0].share_prompt is False
    pf = tmp_path / "prompt.json"
    pf.write_text("[500, 64]")

    def args(model, inp):
        m = parsers["model_args"].parse_known_args(model)[0]
        i = parsers["input_args"].parse_known_args(["--output_dir", str(tmp_path)] + inp)[0]
        return m, i
    cli.check_share_prompt(*args([], []))
    cli.check_share_prompt(*args(["--share_prompt"], ["--prompt_tokens", str(pf)]))
    with pytest.raises(ValueError, match=r"--share_prompt needs --prompt_tokens"):
        cli.check_share_prompt(*args(["--share_prompt"], []))
    for flags, what in ((["--sliding_memory"], "--sliding_memory"), (["--kv_cache", "fp8"], "--kv_cache fp8"),
                        (["--parity"], "--parity")):
        with pytest.raises(ValueError, match=rf"--share_prompt cannot be combined with {what}"):
            cli.check_share_prompt(*args(["--share_prompt"] + flags, ["--prompt_tokens", str(pf)]))
        with pytest.raises(ValueError, match=r"--share_prompt"):          # main() refuses before it loads anything
            cli.main(*args(["--share_prompt"] + flags, ["--prompt_tokens", str(pf)]))
