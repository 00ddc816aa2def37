"""The guide track on the GPU.  The defining property: a draw under the six words -- note order, voice cap, density, interval,
onset template and guide -- is bit for bit the draw the class-control kernel makes for the same inputs with none of them and
bias[b] = -inf at the union of the six rules' bans as the contracts state them (the density's under the waiver on the onset
row ANDed with the guide's live row) -- so the sampler test needs no tolerance.  One launch of 85 rows: the host test's edge
cases, the bits at the word seams, rows whose last POSITION lies one and two chunks back, rows beside every other rule, and
random rows over random blocks.  Then through the decode loop: captured graph == eager == separate launches, free slots
token for token a decoder that never heard of the feature, a primed slot that continues the cycle in phase, in-place
switching, the fp8 sliding cache, fp32 parity, the request pool with both arm launches and the command line."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import density_contract as DC  # noqa: E402
import guide_contract as GD  # noqa: E402
import interval_contract as IC  # noqa: E402
import note_order_contract as NO  # noqa: E402
import onsets_contract as OC  # noqa: E402
import test_guide_host as GH  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
import test_logit_bias_gpu as LBG  # noqa: E402
import test_note_order_gpu as NG  # noqa: E402
import test_onsets_host as OH  # noqa: E402
import test_sampling_rows_gpu as SR  # noqa: E402
import test_voices_host as VH  # noqa: E402
import voices_contract as VC  # noqa: E402

DEV = "cuda"
V = 729
LD_SEQ = 256
NEG = float("-inf")
F_NBAR = 8
bits = SR.bits
CTX = VH.CTX
W, pos, dur, note = GD.word, VH.pos, VH.dur, GH.note
same_row = NG.same_row
pitches_but = GH.pitches_but

# ------------------------------------------------------------------------------------------------ 1. the sampler
# the table: the host test's 165 rows (templates A, B, C), then D at base 165 -- one bar of 16 cells whose cells 0 .. 7 allow
# ONE pitch each, the bits on both sides of every word seam, the last bit and the first -- then 34 random blocks of 16 cells
SEAM_BITS = (31, 32, 63, 64, 95, 96, 127, 0)           # ids 34 / 35, 66 / 67, 98 / 99, 130 and 3
D_BASE = GH.N_ROWS
R_BASE = D_BASE + 17
N_RANDOM_BLOCKS = 34


def guide_table():
    rs = np.random.RandomState(31)
    d = GH._block(range(128), {c: [k] for c, k in enumerate(SEAM_BITS)}, 16)
    rnd = rs.randint(0, 2 ** 32, size=(N_RANDOM_BLOCKS * 17, 4), dtype=np.uint64).astype(np.uint32)
    rnd[rs.rand(len(rnd)) < 0.1] = 0
    rnd[rs.rand(len(rnd)) < 0.1] = 0xFFFFFFFF
    table = np.concatenate([GH.TABLE, np.stack(d), rnd])
    # (the host test's two clamp cases, moved to the end of this table: row 755 all ones, the last row pitch / step 127 only)
    table[-5] = 0xFFFFFFFF
    table[-1] = GD.mask_of([127])
    assert len(table) == R_BASE + N_RANDOM_BLOCKS * 17 == 760                 # 3 + 1 + 34 templates, some 40 blocks
    return table


NOTHING = "nothing_left_all_clear_cell_and_bias"


def cases():
    """(name, tokens, F_LEN or None, density, note-order, voice, interval, onset word (over OH.TABLE), guide word)."""
    out = [(n, t, ln, d, o, v, -1, -1, W(755, 1, 3) if n == "cell_row_clamped_to_the_last_row" else w)
           for n, t, ln, d, o, v, w, _, _, _ in GH.EDGE_CASES]
    D = W(D_BASE, 1, 3)
    out += [("seam_bit_%d" % k, CTX + [2, pos(8 * c), 150], None, -1, -1, -1, -1, -1, D) for c, k in enumerate(SEAM_BITS)]
    # no grammar structure behind the position: the first ballot finds j in chunk 1 and in chunk 2, so the cell row is
    # fetched behind the chunk loop
    out += [("position_70_tokens_back", CTX + [2, pos(0), 150] + [200] * 70, None, -1, -1, -1, -1, -1, GH.A),
            ("position_140_tokens_back", CTX + [2, pos(120), 150] + [200] * 140, None, -1, -1, -1, -1, -1, GH.A),
            ("no_breaker_in_150_tokens", CTX + [200] * 150, None, -1, -1, -1, -1, -1, GH.A)]
    busy = CTX + [2] + note(0, 70, 64) + note(8, 61, 2) + [pos(16), 150]
    done = CTX + [2] + note(0, 70, 64) + note(8, 61, 2)
    out += [("all_six_rules_pitch_next", busy, None, DC.word(1, 4), 0, VC.word(2, True), IC.word(4, 5, True), OC.word(21, 3), GH.A),
            ("all_six_rules_position_next", done, None, DC.word(3, 4), 0, VC.word(2, True), IC.word(4, 5, True), OC.word(21, 3),
             GH.A),
            # onset row 88 allows steps 0, 4, 8 and C's live row the same: the note order's floor is past them, the waiver fires
            ("all_six_rules_waiver", done, None, DC.word(3, 4), 1, VC.word(1), IC.word(1, 1), OC.word(88, 1), GH.C_),
            # the onset row (89: steps 0, 64) leaves step 64, the live row (C: 0, 4, 8) does not: only the AND fires the waiver
            ("waiver_fires_only_on_the_anded_row", GH.bars(0, [2] + GH.AT40), None, DC.word(2), 0, 0, -1, OC.word(89, 1), GH.C_),
            (NOTHING, CTX + [2, pos(40), 150], None, -1, -1, -1, -1, -1, GH.A)]
    rs = np.random.RandomState(37)
    for i in range(48):
        n = int(rs.choice([20, 70, 100, 140, 200]))
        t = CTX + VH.random_tokens(rs, n)[:n]
        if i % 3 == 0:                              # (no BAR in the last 140 tokens: the walk does go three chunks)
            t = [x if (x != 2 or j < len(t) - 140) else 200 for j, x in enumerate(t)]
        if i % 4 == 1:                              # (nor a POSITION in the last 70: j is found in a later chunk)
            t = [x if (not (x == 2 or 432 <= x <= 559) or j < len(t) - 70) else 200 for j, x in enumerate(t)]
        R = int(rs.randint(1, 5))
        gw = W(R_BASE + 17 * int(rs.randint(0, N_RANDOM_BLOCKS - R + 1)), R, 3)
        g = int(rs.choice([-1, gw, gw]))
        cyc = int(rs.randint(1, 9))
        w = int(rs.choice([-1, OC.word(int(rs.randint(0, 91 - cyc + 1)), cyc)]))
        d = int(rs.choice([-1, DC.word(2), DC.word(1, 3), DC.word(0, 9)]))
        o = int(rs.choice([-1, 0, 1]))
        v = int(rs.choice([-1, 0, VC.word(1, True), VC.word(2)]))
        m = int(rs.choice([-1, IC.word(7, 7), IC.word(2, 3, True)]))
        out.append(("random_%d_L%d" % (i, len(t)), t, None, d, o, v, m, w, g))
    assert 48 <= len(out) <= 96, len(out)
    return out


def build():
    """The 64 rows of the sampling test tiled, the six words, F_NBAR as the forcing stage keeps it, every rule's bans by its
    contract and a bias that makes what the guide takes away the likely token."""
    from commu_amd._lib import call
    from commu_amd.generate import CLASS_CTL_DTYPE, event_grammar, harmony_table
    cs, table, otable = cases(), guide_table(), OH.TABLE
    n = len(cs)
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    pick = torch.arange(n) % logits.shape[0]
    logits, wrong, us, t, k, p = logits[pick], wrong[pick], us[pick], t[pick], k[pick], p[pick]
    assert bool((t == 0).any()) and bool((t != 0).any())                  # greedy rows and sampled rows
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(n, nf, dtype=torch.int32)
    seq = torch.full((n, LD_SEQ), 310, dtype=torch.int32)                 # (behind the tokens: durations)
    dctl, octl, vctl, mctl, wctl, gctl = (torch.zeros(n, dtype=torch.int32) for _ in range(6))
    banned, guide_banned, onset_only_density = [], [], []
    bias = torch.zeros(n, 768)
    for b, (name, tokens, length, d, o, v, m, w, g) in enumerate(cs):
        assert len(tokens) <= LD_SEQ
        seq[b, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32)
        L = len(tokens) if length is None else length
        st[b, 0] = L
        st[b, F_NBAR] = list(tokens[:L]).count(2)                         # (seq.count(BAR), as forcing_pre / _post keep it)
        st[b, 10] = 1                                                     # F_CUR: one chord placed
        dctl[b], octl[b], vctl[b], mctl[b], wctl[b], gctl[b] = d, o, v, m, w, g
        row = seq[b].tolist()
        gb = GD.bans(row, L, g, table)
        db = GD.density_bans(row, L, g, table, w, otable, d, o, v)
        guide_banned.append(gb)
        onset_only_density.append(OC.density_bans(row, L, w, otable, d, o, v))
        others = set(NO.bans(row, L, o)) | set(VC.bans(row, L, v)) | set(db) | set(IC.bans(row, L, m)) | \
            set(OC.bans(row, L, w, otable))
        banned.append(sorted(others | set(gb)))
        assert not set(gb) & ({0, 1, 2, 131} | set(range(131, 432)))      # (ids 0 .. 2 and 131 are never touched)
        bias[b, [i for i in (2,) if i in db]] = 14.0                      # (the density's teeth)
        # teeth: an id that ONLY the guide takes away is the likely token (none such: any it takes away)
        only = [i for i in gb if i not in others] or gb
        if only:
            bias[b, only[len(only) // 2]] = 14.0
        if name == NOTHING:
            bias[b] = NEG
            bias[b, 40] = bias[b, 90] = 0.0                               # (two pitches, both banned by the all-clear cell)
    rec = np.zeros((n, 8), dtype=CLASS_CTL_DTYPE)                         # no class controls: the base-triple table
    for b in range(n):
        rec[b, :] = (float(t[b]), int(k[b]), float(p[b]), 0)
    ct = torch.full((n, 4), 199, dtype=torch.int32)
    return dict(n=n, cases=cs, logits=logits, wrong=wrong, us=us, bias=bias, state=st, seq=seq, chord_tok=ct, ctl=octl,
                vctl=vctl, dctl=dctl, mctl=mctl, wctl=wctl, gctl=gctl, table=torch.from_numpy(otable.view(np.int32).copy()),
                gtable=torch.from_numpy(table.view(np.int32).copy()), banned=banned, guide_banned=guide_banned,
                onset_only_density=onset_only_density, gram=torch.from_numpy(event_grammar()),
                gram_on=torch.tensor([b % 2 for b in range(n)], dtype=torch.uint8), harm=torch.from_numpy(harmony_table()),
                harm_on=torch.tensor([(b // 2) % 2 for b in range(n)], dtype=torch.uint8),
                cls=torch.from_numpy(rec.view(np.int32).reshape(n, 8, 4)))


@pytest.fixture(scope="module")
def rows():
    r = build()
    # the hand-written expectations of the host test hold for the padded rows too
    for i, (name, *_, wp, wq, _) in enumerate(GH.EDGE_CASES):
        assert r["cases"][i][0] == name and r["guide_banned"][i] == sorted(wp + wq), name
    names = [c[0] for c in r["cases"]]
    for c, k in enumerate(SEAM_BITS):                                       # (one pitch each: ids 34, 35, 66, 67, 98, 99, 130, 3)
        assert r["guide_banned"][names.index("seam_bit_%d" % k)] == pitches_but(k), k
    assert r["guide_banned"][names.index("position_70_tokens_back")] == sorted(pitches_but(60, 64, 67) + GH.P[40:48])
    assert r["guide_banned"][names.index("position_140_tokens_back")] == sorted(pitches_but(0, 127) + GH.P[40:48])
    assert r["guide_banned"][names.index("no_breaker_in_150_tokens")] == GH.P[40:48]
    return r


def launch(r, logits, guide="gctl", onsets="wctl", interval="mctl", density="dctl", voices="vctl", order="ctl", bias=None,
           gtable="gtable", n_rows=None):
    """One launch of commu_sample_topk on fresh device copies (token -7, probs_out -3.0, logp_out 7.0 before it), the class
    records given and the scalars poisoned.  guide / onsets / interval / density / voices / order: the rows' words by name,
    None (a null pointer) or a tensor; gtable: likewise; n_rows: guide_rows (None: the table's)."""
    from commu_amd._lib import SampleArgs, call, struct_args
    n = r["n"]
    d = lambda x: x.to(DEV).contiguous()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    words = lambda x: None if x is None else d(r[x] if isinstance(x, str) else x)
    lg = logits.clone().to(DEV)
    pr = torch.full((n, V), -3.0, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n, 2), 7.0, device=DEV)
    h = {k: d(r[k]) for k in ("wrong", "us", "gram", "gram_on", "harm", "harm_on", "state", "seq", "chord_tok", "cls", "table")}
    bd = d(r["bias"] if bias is None else bias)
    od, vd, dd, md, wd = words(order), words(voices), words(density), words(interval), words(onsets)
    gd, td = words(guide), words(gtable)
    rows_arg = (0 if td is None else td.shape[0]) if n_rows is None else n_rows
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=n, V=V, wrong=ptr(h["wrong"]), ldw=V, uniforms=ptr(h["us"]),
        temperature=5.0, top_k=3, top_p=0.3, token=ptr(tok), probs_out=ptr(pr), ldp=V, logp_out=ptr(lp),
        bias=ptr(bd), ld_bias=bd.stride(0), gram=ptr(h["gram"]), ld_gram=h["gram"].stride(0), gram_on=ptr(h["gram_on"]),
        harm=ptr(h["harm"]), ld_harm=h["harm"].stride(0), harm_on=ptr(h["harm_on"]), state=ptr(h["state"]),
        seq=ptr(h["seq"]), ld_seq=LD_SEQ, chord_tok=ptr(h["chord_tok"]), ld_chord=4, cls_ctl=ptr(h["cls"]),
        order_ctl=ptr(od), voice_ctl=ptr(vd), density_ctl=ptr(dd), interval_ctl=ptr(md),
        **({} if wd is None else {"onset_ctl": ptr(wd), "onset_table": ptr(h["table"]), "onset_rows": h["table"].shape[0]}),
        **({} if gd is None else {"guide_ctl": ptr(gd), "guide_table": ptr(td), "guide_rows": rows_arg}))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()


NONE = dict(guide=None, onsets=None, interval=None, density=None, voices=None, order=None)


def banned_bias(r, which="banned"):
    out = r["bias"].clone()
    for b, ids in enumerate(r[which]):
        out[b, ids] = NEG
    return out


def test_sampler_equals_the_launch_without_the_words_and_the_bans_in_the_bias(rows):
    """Fails on the parent: commu_sample_args has no guide_ctl.  Fails for a kernel that ignores the rows: the bias makes an
    id the guide bans the likely token.  Every row is compared, the Q12 rows included."""
    r, n = rows, rows["n"]
    names = [c[0] for c in r["cases"]]
    got = launch(r, r["logits"])
    want = launch(r, r["logits"], bias=banned_bias(r), **NONE)
    free = launch(r, r["logits"], guide=None)
    for b in range(n):
        assert same_row(got, want, b), (names[b], int(got[1][b]), int(want[1][b]))
        for i in r["banned"][b]:
            assert float(got[2][b, i]) == 0.0 or int(got[1][b]) == -1, (names[b], i)
    # the same against the ONSET kernel (the launch without guide_ctl, every other word on) with the guide's bans as -inf in
    # the bias: every row whose density ban the live row does not change -- the waiver is the one place where the guide is
    # more than a bias
    by_onsets = launch(r, r["logits"], guide=None, bias=banned_bias(r, "guide_banned"))
    moved = [names[b] for b in range(n)
             if r["onset_only_density"][b] != GD.density_bans(r["seq"][b].tolist(), int(r["state"][b, 0]), r["cases"][b][8],
                                                              guide_table(), r["cases"][b][7], OH.TABLE, r["cases"][b][3],
                                                              r["cases"][b][4], r["cases"][b][5])]
    assert "waiver_fires_only_on_the_anded_row" in moved and "waiver_fires_through_the_live_row" in moved and len(moved) < n // 2
    for b in range(n):
        if names[b] not in moved:
            assert same_row(got, by_onsets, b), names[b]
    # teeth: the launch without the guide draws differently on the rows where the bias favours what it bans
    differ = [names[b] for b in range(n) if int(got[1][b]) != int(free[1][b])]
    took = [names[b] for b in range(n) if int(free[1][b]) in r["guide_banned"][b]]
    print("rows:", n, "; rows with a guide ban:", sum(bool(x) for x in r["guide_banned"]), "; rows whose token differs from "
          "the launch without the guide:", len(differ), "; rows whose density ban the live row moves:", moved)
    assert set(took) <= set(differ) and len(took) >= 12
    assert int((got[1] >= 1).sum()) >= n // 2
    # by name: the seam bits, the far positions, the clamp, Q12
    for k in SEAM_BITS:
        b = names.index("seam_bit_%d" % k)
        assert int(got[1][b]) in (-1, 3 + k) or not (3 <= int(got[1][b]) <= 130), (k, int(got[1][b]))
    nothing = names.index(NOTHING)
    assert int(got[1][nothing]) == -1 and bool(torch.isnan(got[3][nothing]).all())
    assert int(free[1][nothing]) in (40, 90)
    fires, stays = names.index("waiver_fires_through_the_live_row"), names.index("waiver_must_not_fire_steps_48_up_are_left")
    assert 2 not in r["banned"][fires] and 2 in r["banned"][stays]
    # Q5: the same two launches again on the logits the first ones left -- the same bans on the compounded rows
    got2 = launch(r, got[0])
    want2 = launch(r, want[0], bias=banned_bias(r), **NONE)
    for b in range(n):
        assert same_row(got2, want2, b), names[b]
    assert not torch.equal(bits(got2[0]), bits(got[0]))                   # (the sampled rows were divided again)


def test_off_words_and_an_all_ones_template_are_the_onset_kernel_bit_for_bit(rows):
    r, n = rows, rows["n"]
    free = launch(r, r["logits"], guide=None)
    off = launch(r, r["logits"], guide=torch.full((n,), -1, dtype=torch.int32))
    # (an all-ones template of two bars of 16 cells, at base 3 of a table of its own)
    ones = torch.full((3 + 34, 4), -1, dtype=torch.int32)
    ones[:3] = 0
    same = launch(r, r["logits"], guide=torch.full((n,), W(3, 2, 3), dtype=torch.int32), gtable=ones)
    for b in range(n):
        assert same_row(off, free, b) and same_row(same, free, b), r["cases"][b][0]


def test_entry_point_refusal_and_ops(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    r = rows
    for kw in (dict(onsets=None), dict(interval=None), dict(gtable=None), dict(n_rows=0), dict(n_rows=65537), dict(n_rows=-1)):
        with pytest.raises(CommuHipError, match="-22"):
            launch(r, r["logits"], **kw)
    d = lambda x: x.to(DEV)
    full = dict(uniforms=d(r["us"]), bias=d(r["bias"]), class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])),
                note_order=d(r["ctl"]), voices=d(r["vctl"]), density=d(r["dctl"]), interval=d(r["mctl"]))
    ons = (d(r["wctl"]), d(r["table"]))
    with pytest.raises(CommuHipError, match="guide: onsets= expected"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, guide=(d(r["gctl"]), d(r["gtable"])), **full)
    with pytest.raises(CommuHipError, match="guide controls"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, onsets=ons, guide=(d(r["gctl"]).float(), d(r["gtable"])), **full)
    with pytest.raises(CommuHipError, match="guide table"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, onsets=ons, guide=(d(r["gctl"]), d(r["gtable"]).reshape(-1, 2)), **full)
    with pytest.raises(CommuHipError, match="guide: a pair"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, onsets=ons, guide=d(r["gctl"]), **full)
    # ops.sample_topk(guide=) makes the same launch (it builds the all-off grammar and harmony itself)
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), top_p=0.3, onsets=ons, guide=(d(r["gctl"]), d(r["gtable"])), **full)
    plain = dict(r, gram_on=torch.zeros_like(r["gram_on"]), harm_on=torch.zeros_like(r["harm_on"]))
    ref = launch(plain, r["logits"])
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))
    # where there is no template: all -1 onset words over a one-row all-ones table
    n = r["n"]
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), top_p=0.3,
                          onsets=(torch.full((n,), -1, dtype=torch.int32, device=DEV),
                                  torch.full((1, 4), -1, dtype=torch.int32, device=DEV)),
                          guide=(d(r["gctl"]), d(r["gtable"])), **full)
    ref = launch(plain, r["logits"], onsets=torch.full((n,), -1, dtype=torch.int32))
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 2. through the loop
GLEN = NG.GLEN
run, separate_launches = LBG.run, LBG.separate_launches
fixture_model = NG.fixture_model
MELODY = GH.GUIDE                         # the host test's two-bar melody: avoid_intervals [1, 11], no_unison, 16 cells
TRIADS = {"cells": 4, "bars": [[[48, 52, 55, 60, 64, 67, 72, 76, 79], None, [50, 53, 57, 62, 65, 69, 74, 77, 81],
                                [43, 47, 50, 55, 59, 62, 67, 71, 74]]]}
EVENS, ODDS = list(range(0, 128, 2)), list(range(1, 128, 2))
PARITY = {"cells": 1, "bars": [[EVENS], [ODDS]]}      # (disjoint bars: a slot out of phase breaks the guide at once)
GUIDES = (MELODY, None, TRIADS, None)


def loaded(z, model, B, guide=None, onsets=None, **kw):
    """test_onsets_gpu.loaded (grammar on, log-probabilities recorded, the steering row) with set_guide's value (and
    set_onsets' where given)."""
    from commu_amd.generate import ForcedDecoder
    prompts, glen, triple, bias = kw.pop("prompts", None), kw.pop("glen", GLEN), kw.pop("triple", (0.95, 32)), kw.pop("bias", None)
    dec = ForcedDecoder(model, B, glen, 4146, triple[0], triple[1], **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES) if bias is None else bias)
    if guide is not None:
        dec.set_guide(guide)
    if onsets is not None:
        dec.set_onsets(onsets)
    HG.reload(z, dec, prompts)
    return dec


def violation(seq, lp, guide, start):
    """guide_violation of a decoded sequence; a token was DRAWN where its log-probability pair is a number."""
    from commu_amd.generate import guide_template
    rows_, cells = guide_template(guide)
    drawn = [not np.isnan(x) for x in np.asarray(lp)[:len(seq), 0]]
    return GD.guide_violation(seq, start, rows_, drawn, cells=cells)


def drawn_pitches(seq, lp, start):
    return [i for i in range(start, len(seq)) if 3 <= seq[i] <= 130 and not np.isnan(np.asarray(lp)[i, 0])]


def check_on_slot(z, seq, lp, guide):
    from commu_amd.midi_generator.midi_inferrer import parse_events
    start = 1 + len(z["encoded_meta"])
    assert seq is not None and parse_events(seq, start) is None, seq
    assert violation(seq, lp, guide, start) is None, (guide, seq)
    assert len(drawn_pitches(seq, lp, start)) >= 1


@pytest.mark.parametrize("parity, B", [(False, 8), (True, 4)], ids=["bf16_8_slots", "parity_fp32_4_slots"])
def test_alternating_slots_through_the_loop(fixture_model, parity, B):
    """Fails on the parent: ForcedDecoder has no set_guide.  Fails for a kernel that ignores the rows: the run without the
    feature draws pitches both guides ban."""
    z, model = fixture_model
    start = 1 + len(z["encoded_meta"])
    model.parity_fp32 = parity
    try:
        plain = loaded(z, model, B)
        assert plain.guide_ctl is None and plain.guide_table is None and plain.onset_ctl is None and plain.cls_ctl is None
        s0, f0, l0 = run(plain)
        free, free_lp = plain.sequences()[0], plain.logprobs()
        guides = [GUIDES[b % 4] for b in range(B)]
        res = []
        for mode in ("graph", "eager", "separate"):
            dec = loaded(z, model, B, guide=guides)
            assert dec.state.parity == parity
            assert dec.guide_ctl.tolist() == [(W(0, 2, 3), -1, W(34, 1, 5), -1)[b % 4] for b in range(B)]
            # (the rule implies none of the others: their words exist for the one kernel and are off)
            assert dec.onset_ctl.tolist() == [-1] * B and dec.interval_ctl.tolist() == [-1] * B
            assert dec.density_ctl.tolist() == [-1] * B and dec.voice_ctl.tolist() == [-1] * B
            assert dec.order_ctl.tolist() == [-1] * B
            if mode == "separate":
                res.append(separate_launches(dec, dec.generation_length + 1))
            else:
                res.append(run(dec, use_graph=mode == "graph"))
            if mode == "graph":
                assert dec.graph is not None
                seqs, lps = dec.sequences()[0], dec.logprobs()
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert torch.equal(bits(res[0][2]), bits(other[2]))
        sg, fg, lg = res[0]
        for b in range(B):
            if guides[b] is not None:
                check_on_slot(z, seqs[b], lps[b], guides[b])
            else:
                assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
        # teeth: the same request without the rule draws pitches the guides ban, and the rule changed the guided slots
        broke = [(b, i) for b in range(B) for i, t in enumerate((MELODY, TRIADS))
                 if free[b] is not None and violation(free[b], free_lp[b], t, start) is not None]
        print("without the rule: (slot, guide) pairs with a drawn pitch the guide bans:", broke)
        assert broke
        assert any(not torch.equal(sg[b], s0[b]) for b in range(B) if guides[b] is not None)
    finally:
        model.parity_fp32 = False


def test_a_primed_slot_continues_the_cycle_in_phase(fixture_model):
    """The prompt is the first bar and a half of a sequence the loop itself wrote under the guide: it holds two Bars, so the
    open bar is bar 1 and the first draws follow block 1 (odd pitches), not block 0 (even) -- the blocks are disjoint, so a
    slot that took bar 0's block would break the guide with its first drawn pitch.  An onset template beside the guide
    ({"grid": 8}: eight onsets a bar) keeps the bars short enough for the sequence to hold three."""
    z, model = fixture_model
    n_ctx = 1 + len(z["encoded_meta"])
    src = loaded(z, model, 2, guide=PARITY, onsets={"grid": 8})
    run(src)
    own, own_lp = src.sequences()[0][0], src.logprobs()[0]
    bars = [i for i, t in enumerate(own) if t == 2]
    assert len(bars) >= 3, own
    # cut behind the first complete note of bar 1 (the token after a DURATION is a draw), else behind bar 1's forced tokens
    ends = [i for i in range(bars[1], bars[2]) if 304 <= own[i] <= 431 and not np.isnan(own_lp[i, 0])]
    cut = (ends[0] + 1) if ends else next(i for i in range(bars[1] + 1, bars[2] + 1) if not np.isnan(own_lp[i, 0]))
    prompt = own[n_ctx:cut]
    assert prompt.count(2) == 2
    for name, guide in (("grammar", None), ("guide", PARITY)):
        dec = loaded(z, model, 2, guide=guide, onsets={"grid": 8}, max_prompt=len(prompt), prompts=[prompt] * 2)
        run(dec)
        seq, lp = dec.sequences()[0][0], dec.logprobs()[0]
        assert seq[:cut] == own[:cut] and len(seq) > cut + 4, seq
        assert int(dec.fsm.cpu()[0, F_NBAR]) == seq.count(2)
        if guide is not None:
            after = drawn_pitches(seq, lp, cut)
            assert after and violation(seq, lp, PARITY, cut) is None, seq
            nxt = [i for i in range(cut, len(seq)) if seq[i] == 2]
            first_bar = [seq[i] - 3 for i in after if not nxt or i < nxt[0]]
            assert all(x % 2 == 1 for x in first_bar), (first_bar, seq)
            # (out of phase -- bar 0's block for the open bar -- the same sequence breaks the guide)
            if first_bar:
                assert violation(seq, lp, {"cells": 1, "bars": [[ODDS], [EVENS]]}, cut) is not None


def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, guide=[None, MELODY, None, None])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g, table = dec.graph, dec.guide_table
    assert g is not None
    check_on_slot(z, dec.sequences()[0][1], dec.logprobs()[1], MELODY)
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_guide(None, rows=[1])
    dec.set_guide(TRIADS, rows=[2])
    uni = HG.reload(z, dec)
    dec.rearm(3, uni[3], guide=PARITY)
    s, f, l = run(dec)
    assert dec.graph is g and dec.guide_table is table and dec.guide_ctl.tolist() == [-1, -1, W(34, 1, 5), W(39, 2, 7)]
    assert dec.onset_ctl.tolist() == [-1] * 4 and dec.interval_ctl.tolist() == [-1] * 4
    second, lps = dec.sequences()[0], dec.logprobs()
    check_on_slot(z, second[2], lps[2], TRIADS)
    check_on_slot(z, second[3], lps[3], PARITY)
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], guide=False)
    dec.set_guide(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.guide_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


def test_fp8_sliding_cache_feeds_the_same_stage():
    import test_kv8_gpu as K8
    from commu_amd.generate import ForcedDecoder
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model, data = K8._loop_model(32)
    uni = np.random.RandomState(4).random_sample((4, 80)).astype(np.float32)
    guides = [MELODY, TRIADS, PARITY, {"cells": 2, "bars": [[[60, 61, 62], [70, 71]]]}]
    dec = ForcedDecoder(model, 4, generation_length=64, memory_length=32, temperature=0.95, top_k=32, sliding=True,
                        kv_dtype="fp8")
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_guide(guides)
    outs = []
    for graph in (False, True):
        dec.load([K8.META] * 4, [data] * 4, uni)
        with torch.no_grad():
            dec.run(use_graph=graph)
        torch.cuda.synchronize()
        outs.append(dec.sequences()[0])
    assert dec.state.kv_dtype == "fp8" and dec.graph is not None and outs[0] == outs[1]
    assert int(dec.state.klen.max()) >= 32                                # (the ring is full)
    start = 1 + len(K8.META)
    lps = dec.logprobs()
    assert sum(len(drawn_pitches(s, lp, start)) for s, lp in zip(outs[0], lps) if s is not None) >= 4
    for s, lp, t in zip(outs[0], lps, guides):
        assert s is not None and parse_events(s, start) is None, s
        assert violation(s, lp, t, start) is None, (t, s)


# ------------------------------------------------------------------------------------------------ 3. the request pool
@pytest.mark.parametrize("primed", [False, True], ids=["commu_decode_arm", "commu_decode_arm_primed"])
def test_pool_requests_with_their_own_guides_equal_generate_stream_of_each_alone(primed):
    """Two requests with different guides (one under the grammar, primed: its prompt cut from a sequence generated under
    the same controls; one without the grammar) and one without a guide: each one's sequences equal
    generate_stream(slots=1) of the request alone -- the arm launch wrote each slot's word, the table is the pool's."""
    import commu_amd.generate as G
    import pool_contract as PC
    import pool_prime_contract as PP
    import test_pool_gpu as TP
    import test_pool_prime_gpu as TPP
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model = TP._model()
    reqs = PC.four_requests(G)
    t1, t2 = PARITY, TRIADS
    every = lambda seq, rep: seq is not None
    mine = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, logit_bias=None, guide=t1)
    if primed:
        own = TPP._own_sequence(TPP._generator(model), mine, 6, grammar=True, guide=t1)
        mine = dataclasses.replace(mine, prompt=PP.prompt_of(own, len(PC.META), 6))
    want = TPP._alone(TPP._generator(model), mine, grammar=True, guide=t1)
    second = dataclasses.replace(reqs[0], accept=every, grammar=False, guide=t2)
    second_want = TPP._alone(TPP._generator(model), second, guide=t2)
    third = dataclasses.replace(reqs[2], accept=every, grammar=False)
    third_want = TPP._alone(TPP._generator(model), third)
    gen = TPP._generator(model)
    res = gen.generate_pool([second, mine, third], slots=3, grammar=True, return_logprobs=True)
    TPP._same_results(res[1], want)
    TPP._same_results(res[0], second_want)
    assert res[2].sequences == third_want[0] and res[2].attempts_started == third_want[1]      # (token for token)
    assert gen.pool_stats["kernel"] == ("commu_decode_arm_primed" if primed else "commu_decode_arm")
    assert len(res[1].sequences) == 2
    cut = TPP.N_CTX + (6 if primed else 0)
    for s, lp in zip(res[1].sequences, res[1].logprobs):
        assert parse_events(s, TPP.N_CTX) is None, s
        assert violation(s, lp, t1, cut) is None, s
    for s, lp in zip(res[0].sequences, res[0].logprobs):
        assert violation(s, lp, t2, TPP.N_CTX) is None, s
    # teeth: without guide= the same request decodes something else
    free = TPP._alone(TPP._generator(model), dataclasses.replace(mine, guide=None), grammar=True)
    assert free[0] != want[0]


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_generate_cli_guide_end_to_end(golden_dir, tmp_path, monkeypatch):
    """generate.py --grammar --guide on the reference-written checkpoint, every sequence that could be drawn accepted (a
    random model rarely passes the validators): every pitch of what it writes is one the guide allows -- a pitch is never a
    forced token; the same run without the flag writes pitches it bans."""
    import test_model_gpu as TM
    from commu_amd.generate import guide_template
    from commu_amd.midi_generator.midi_inferrer import ForcingReport, InferenceTask, parse_events
    z = TM.load(golden_dir, "g10_checkpoint.npz")
    cli = TM._load_script("generate")
    parsers = cli.parse_args()
    prog = "-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8)
    common = ["--checkpoint_dir", os.path.join(golden_dir, "g10_checkpoint.pt"), "--generation_length", "120", "--gpus", "1",
              "--bpm", "70", "--audio_key", "aminor", "--time_signature", "4/4", "--pitch_range", "mid_high",
              "--num_measures", "8", "--inst", "acoustic_piano", "--genre", "newage", "--min_velocity", "60",
              "--max_velocity", "80", "--track_role", "main_melody", "--rhythm", "standard", "--chord_progression",
              prog + "-" + prog, "--num_generate", "2", "--max_rounds", "1", "--decode_slots", "2", "--grammar"]
    monkeypatch.setattr(ForcingReport, "validate_teacher_forced_sequence", lambda self, seq: None)
    monkeypatch.setattr(InferenceTask, "validate_generated_sequence", lambda self, seq: True)

    def run(argv, out):
        argv = common + ["--output_dir", str(tmp_path / out)] + argv
        margs, _ = parsers["model_args"].parse_known_args(argv)
        iargs, _ = parsers["input_args"].parse_known_args(argv)
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
        return json.load(open(tmp_path / out / "sequences.json"))

    got = run(["--guide", json.dumps(PARITY)], "guided")
    free = run([], "free")
    start = 1 + len(got["encoded_meta"])
    rows_, cells = guide_template(PARITY)
    assert len(got["sequences"]) >= 1 and len(free["sequences"]) >= 1
    for s in got["sequences"]:
        assert parse_events(s, start) is None, s
        assert sum(1 for t in s[start:] if 3 <= t <= 130) >= 4 and GD.guide_violation(s, start, rows_, cells=cells) is None, s
    assert any(GD.guide_violation(s, start, rows_, cells=cells) is not None for s in free["sequences"])
