"""The articulation rule on the GPU.  The defining property: a draw under the seven words -- note order, voice cap, density,
interval, onset template, guide and articulation -- is bit for bit the draw the class-control kernel makes for the same inputs
with none of them and bias[b] = -inf at the union of the seven rules' bans as the contracts state them -- so the sampler test
needs no tolerance.  One launch of at most 96 rows: the host test's edge cases (the first clear bit of the hold term at m = 1,
64, 65, 127 and none, the lookahead into the next bar with R_g = 1 and 2, s = 0 and 7, the clamps, the bar line, the lower
bound giving way), pitch bits at the word seams, rows whose last POSITION lies one and two chunks back, rows beside every other
rule, and random rows over random tables.  Then through the decode loop: captured graph == eager == separate launches, free
slots token for token a decoder that never heard of the feature, a primed slot that continues the cycle in phase, in-place
switching, the request pool with both arm launches and the command line."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import articulation_contract as AC  # noqa: E402
import density_contract as DC  # noqa: E402
import guide_contract as GD  # noqa: E402
import interval_contract as IC  # noqa: E402
import note_order_contract as NO  # noqa: E402
import onsets_contract as OC  # noqa: E402
import test_articulation_host as AH  # noqa: E402
import test_guide_gpu as GG  # noqa: E402
import test_guide_host as GH  # noqa: E402
import test_harmony_gpu as HG  # noqa: E402
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
W, pos, dur, note = AC.word, VH.pos, VH.dur, GH.note
same_row = NG.same_row
open_note, durs_outside, vels_but = AH.open_note, AH.durs_outside, AH.vels_but

# ------------------------------------------------------------------------------------------------ 1. the sampler
# the guide table: the host test's 163 rows (G: two bars of 16 cells, H: one bar of 128 cells), then K at base 163 -- one bar
# of ONE cell (s = 7) that bans the pitches at the word seams, MIDI 0, 31, 32, 63, 64, 127 -- then 20 random blocks of 16
# cells, three bits in four set, and a copy of H's last row at the very end (the host test's clamp case)
SEAM_PITCHES = (0, 31, 32, 63, 64, 127)
K_BASE = len(AH.GUIDE)
R_BASE = K_BASE + 2
N_RANDOM_BLOCKS = 20
# the articulation table: the host test's rows 0 .. 3, 20 random rows, and the host test's row 4 at the very end (likewise)
A_RANDOM = 20


def guide_table():
    rs = np.random.RandomState(41)
    k = GH._block(range(128), {0: [x for x in range(128) if x not in SEAM_PITCHES]}, 1)
    rnd = rs.randint(0, 2 ** 32, size=(N_RANDOM_BLOCKS * 17, 4), dtype=np.uint64).astype(np.uint32)
    rnd |= rs.randint(0, 2 ** 32, size=rnd.shape, dtype=np.uint64).astype(np.uint32)
    rnd[rs.rand(len(rnd)) < 0.3] = 0xFFFFFFFF
    rnd[::17] = 0xFFFFFFFF                                   # (the live rows: every position may start a note)
    table = np.concatenate([AH.GUIDE, np.stack(k), rnd, AH.GUIDE[-1:]])
    assert len(table) == R_BASE + N_RANDOM_BLOCKS * 17 + 1 == 506
    return table


def art_table():
    rs = np.random.RandomState(43)
    rnd = np.zeros((A_RANDOM, 4), dtype=np.uint32)
    for r in rnd:
        lo, hi = sorted(int(x) for x in rs.randint(1, 129, 2))
        r[:] = AC.row_of(int(rs.choice([0, lo])), int(rs.choice([0, hi])), [k for k in range(64) if rs.rand() < 0.6] or [7])
        r[3] = rs.randint(0, 2 ** 31)                        # (the reserved word: never read)
    table = np.concatenate([AH.TABLE[:4], rnd, AH.TABLE[4:]])
    assert len(table) == 25
    return table


# what the bias adds to the id a row's teeth sit on: |logit / temperature| <= 18 on these rows (test_sampling_rows_gpu), so
# the id is the likely token by e^4 over any other at the least
TEETH = 40.0
NOTHING = "nothing_left_every_duration_but_one_banned_and_the_bias_bans_that"


def cases():
    """(name, tokens, F_LEN or None, density, note-order, voice, interval, onset word (over OH.TABLE), guide word,
    articulation word)."""
    out = [(n, t, ln, -1, -1, -1, -1, -1, g, w) for n, t, ln, w, g, _, _ in AH.EDGE_CASES]
    K, HOLD = GD.word(K_BASE, 1, 7), W(3, 1, False, True)
    # s = 7: one cell for the whole bar, the banned pitches at the word seams (f = 1), their neighbours free
    out += [("seam_pitch_%d" % k, open_note(5, k), None, -1, -1, -1, -1, -1, K, HOLD) for k in SEAM_PITCHES]
    out += [("seam_neighbour_%d" % k, open_note(5, k), None, -1, -1, -1, -1, -1, K, HOLD) for k in (1, 30, 33, 62, 65, 126)]
    # no grammar structure behind the position: the first ballot finds j in chunk 1 and in chunk 2, so the hold loads go out
    # behind the chunk loop; the previous token is the pitch all the same
    out += [("position_70_tokens_back", CTX + [2, pos(0), 150] + [200] * 70 + [63], None, -1, -1, -1, -1, -1, AH.G, HOLD),
            ("position_140_tokens_back", CTX + [2, pos(100), 150] + [200] * 140 + [63], None, -1, -1, -1, -1, -1, AH.G,
             W(0, 1, True, True)),
            ("no_breaker_in_150_tokens", CTX + [200] * 150 + [63], None, -1, -1, -1, -1, -1, AH.G, W(0, 1, True, True))]
    busy = CTX + [2] + note(0, 70, 64) + note(8, 61, 2) + [pos(16), 150, 63]
    vel = CTX + [2] + note(0, 70, 64) + note(8, 61, 2) + [pos(16)]
    done = CTX + [2] + note(0, 70, 64) + note(8, 61, 2)
    out += [("all_seven_rules_duration_next", busy, None, DC.word(1, 4), 0, VC.word(2, True), IC.word(4, 5, True), OC.word(21, 3),
             AH.G, W(0, 2, True, True)),
            ("all_seven_rules_velocity_next", vel, None, DC.word(1, 4), 0, VC.word(2, True), IC.word(4, 5, True), OC.word(21, 3),
             AH.G, W(1, 1, True, True)),
            ("all_seven_rules_position_next", done, None, DC.word(3, 4), 0, VC.word(2, True), IC.word(4, 5, True), OC.word(21, 3),
             AH.G, W(0, 2, True, True)),
            (NOTHING, open_note(127, 10), None, -1, -1, -1, -1, -1, -1, W(3, 1, True)),
            # the ids right outside the two families are the likely token, beside a row that bans all but one of the family
            ("untouched_130", CTX + [2, pos(0)], None, -1, -1, -1, -1, -1, -1, W(4000, 1)),
            ("untouched_195", CTX + [2, pos(0)], None, -1, -1, -1, -1, -1, -1, W(4000, 1)),
            ("untouched_303", open_note(127, 10), None, -1, -1, -1, -1, -1, -1, W(3, 1, True)),
            ("untouched_432", open_note(0, 10), None, -1, -1, -1, -1, -1, -1, W(0, 1))]
    rs = np.random.RandomState(47)
    for i in range(36):
        n = int(rs.choice([20, 70, 100, 140, 200]))
        t = CTX + VH.random_tokens(rs, n)[:n]
        if i % 3 == 0:                              # (no BAR in the last 140 tokens: the walk does go three chunks)
            t = [x if (x != 2 or j < len(t) - 140) else 200 for j, x in enumerate(t)]
        if i % 4 == 1:                              # (nor a POSITION in the last 70: j is found in a later chunk)
            t = [x if (not (x == 2 or 432 <= x <= 559) or j < len(t) - 70) else 200 for j, x in enumerate(t)]
        if i % 5 != 4:                              # (most rows end in a pitch: a duration comes next)
            t = t + ([pos(int(rs.randint(0, 128))), 150] if i % 4 != 1 else []) + [int(rs.randint(3, 131))]
        R = int(rs.randint(1, 4))
        gw = GD.word(R_BASE + 17 * int(rs.randint(0, N_RANDOM_BLOCKS - R + 1)), R, 3)
        g = int(rs.choice([-1, gw, gw, gw]))
        cyc = int(rs.randint(1, 4))
        aw = W(int(rs.randint(0, 25)), cyc, bool(rs.randint(2)), bool(rs.randint(2)))          # (may reach past the table)
        a = int(rs.choice([-1, aw, aw, aw]))
        w = int(rs.choice([-1, OC.word(int(rs.randint(0, 80)), 2)]))
        d = int(rs.choice([-1, DC.word(2), DC.word(1, 3)]))
        o = int(rs.choice([-1, 0, 1]))
        v = int(rs.choice([-1, 0, VC.word(1, True), VC.word(2)]))
        m = int(rs.choice([-1, IC.word(7, 7), IC.word(2, 3, True)]))
        out.append(("random_%d_L%d" % (i, len(t)), t, None, d, o, v, m, w, g, a))
    assert len(out) <= 96, len(out)
    return out


def build():
    """The 64 rows of the sampling test tiled, the seven words, F_NBAR as the forcing stage keeps it, every rule's bans by its
    contract and a bias that makes what the articulation takes away the likely token."""
    from commu_amd._lib import call
    from commu_amd.generate import CLASS_CTL_DTYPE, event_grammar, harmony_table
    cs, gtable, atable, otable = cases(), guide_table(), art_table(), OH.TABLE
    n = len(cs)
    logits, wrong, us, which, t, k, p = SR.kernel_rows()
    pick = torch.arange(n) % logits.shape[0]
    logits, wrong, us, t, k, p = logits[pick], wrong[pick], us[pick], t[pick], k[pick], p[pick]
    assert bool((t == 0).any()) and bool((t != 0).any())                  # greedy rows and sampled rows
    nf = call("commu_forcing_state_ints")
    st = torch.zeros(n, nf, dtype=torch.int32)
    seq = torch.full((n, LD_SEQ), 310, dtype=torch.int32)                 # (behind the tokens: durations)
    dctl, octl, vctl, mctl, wctl, gctl, actl = (torch.zeros(n, dtype=torch.int32) for _ in range(7))
    banned, art_banned = [], []
    bias = torch.zeros(n, 768)
    gram_on = torch.tensor([b % 2 for b in range(n)], dtype=torch.uint8)
    harm_on = torch.tensor([(b // 2) % 2 for b in range(n)], dtype=torch.uint8)
    for b, (name, tokens, length, d, o, v, m, w, g, a) in enumerate(cs):
        assert len(tokens) <= LD_SEQ
        seq[b, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32)
        L = len(tokens) if length is None else length
        st[b, 0] = L
        st[b, F_NBAR] = list(tokens[:L]).count(2)                         # (seq.count(BAR), as forcing_pre / _post keep it)
        st[b, 10] = 1                                                     # F_CUR: one chord placed
        dctl[b], octl[b], vctl[b], mctl[b], wctl[b], gctl[b], actl[b] = d, o, v, m, w, g, a
        row = seq[b].tolist()
        ab = AC.bans(row, L, a, atable, g, gtable)
        art_banned.append(ab)
        others = set(NO.bans(row, L, o)) | set(VC.bans(row, L, v)) | set(GD.density_bans(row, L, g, gtable, w, otable, d, o, v)) | \
            set(IC.bans(row, L, m)) | set(OC.bans(row, L, w, otable)) | set(GD.bans(row, L, g, gtable))
        banned.append(sorted(others | set(ab)))
        assert not set(ab) & (set(range(0, 131)) | set(range(195, 304)) | set(range(432, V)))      # (130, 195, 303, 432)
        # teeth: an id that ONLY the articulation takes away is the likely token -- the longest duration it bans (what a cap
        # takes away), else the shortest, else a velocity; and the ids right outside the two families are likely too
        only = [i for i in ab if i not in others]
        long_ = [i for i in only if i >= 304]
        if only:
            bias[b, long_[-1] if long_ else only[len(only) // 2]] = TEETH
        if name.startswith("untouched_"):          # (no grammar, no harmony: nothing else takes the id away)
            bias[b] = 0.0
            bias[b, int(name[10:])] = TEETH
            gram_on[b] = harm_on[b] = 0
        if name == NOTHING:
            bias[b] = NEG
            bias[b, 305] = bias[b, 431] = 0.0                             # (two durations, both banned: the cap is 1)
            bias[b, 304] = NEG
    rec = np.zeros((n, 8), dtype=CLASS_CTL_DTYPE)                         # no class controls: the base-triple table
    for b in range(n):
        rec[b, :] = (float(t[b]), int(k[b]), float(p[b]), 0)
    ct = torch.full((n, 4), 199, dtype=torch.int32)
    return dict(n=n, cases=cs, logits=logits, wrong=wrong, us=us, bias=bias, state=st, seq=seq, chord_tok=ct, ctl=octl,
                vctl=vctl, dctl=dctl, mctl=mctl, wctl=wctl, gctl=gctl, actl=actl,
                table=torch.from_numpy(otable.view(np.int32).copy()), gtable=torch.from_numpy(gtable.view(np.int32).copy()),
                atable=torch.from_numpy(atable.view(np.int32).copy()), banned=banned, art_banned=art_banned,
                gram=torch.from_numpy(event_grammar()), gram_on=gram_on, harm=torch.from_numpy(harmony_table()),
                harm_on=harm_on,
                cls=torch.from_numpy(rec.view(np.int32).reshape(n, 8, 4)))


@pytest.fixture(scope="module")
def rows():
    r = build()
    # the hand-written expectations of the host test hold for the padded rows and the longer tables too
    for i, (name, *_, wd, wv) in enumerate(AH.EDGE_CASES):
        assert r["cases"][i][0] == name and r["art_banned"][i] == sorted(wd + wv), name
    names = [c[0] for c in r["cases"]]
    for k in SEAM_PITCHES:
        assert r["art_banned"][names.index("seam_pitch_%d" % k)] == durs_outside(1, 1), k
    for k in (1, 30, 33, 62, 65, 126):
        assert r["art_banned"][names.index("seam_neighbour_%d" % k)] == [], k
    assert r["art_banned"][names.index("position_70_tokens_back")] == durs_outside(1, 24)
    assert r["art_banned"][names.index("position_140_tokens_back")] == durs_outside(2, 28)
    assert r["art_banned"][names.index("no_breaker_in_150_tokens")] == durs_outside(2, 32)
    return r


def launch(r, logits, articulation="actl", atable="atable", n_rows=None, bias=None, guide="gctl"):
    """One launch of commu_sample_topk with the seven words on fresh device copies (token -7, probs_out -3.0, logp_out 7.0
    before it), the class records given and the scalars poisoned.  articulation / guide: the rows' words by name, None (a
    null pointer) or a tensor; atable: likewise; n_rows: art_rows (None: the table's)."""
    from commu_amd._lib import SampleArgs, call, struct_args
    n = r["n"]
    d = lambda x: x.to(DEV).contiguous()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    words = lambda x: None if x is None else d(r[x] if isinstance(x, str) else x)
    lg = logits.clone().to(DEV)
    pr = torch.full((n, V), -3.0, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n, 2), 7.0, device=DEV)
    h = {k: d(r[k]) for k in ("wrong", "us", "gram", "gram_on", "harm", "harm_on", "state", "seq", "chord_tok", "cls", "table",
                              "gtable", "ctl", "vctl", "dctl", "mctl", "wctl")}
    bd = d(r["bias"] if bias is None else bias)
    gd, ad, td = words(guide), words(articulation), words(atable)
    rows_arg = (0 if td is None else td.shape[0]) if n_rows is None else n_rows
    args = struct_args(
        SampleArgs, logits=ptr(lg), ld=lg.stride(0), nseq=n, V=V, wrong=ptr(h["wrong"]), ldw=V, uniforms=ptr(h["us"]),
        temperature=5.0, top_k=3, top_p=0.3, token=ptr(tok), probs_out=ptr(pr), ldp=V, logp_out=ptr(lp),
        bias=ptr(bd), ld_bias=bd.stride(0), gram=ptr(h["gram"]), ld_gram=h["gram"].stride(0), gram_on=ptr(h["gram_on"]),
        harm=ptr(h["harm"]), ld_harm=h["harm"].stride(0), harm_on=ptr(h["harm_on"]), state=ptr(h["state"]),
        seq=ptr(h["seq"]), ld_seq=LD_SEQ, chord_tok=ptr(h["chord_tok"]), ld_chord=4, cls_ctl=ptr(h["cls"]),
        order_ctl=ptr(h["ctl"]), voice_ctl=ptr(h["vctl"]), density_ctl=ptr(h["dctl"]), interval_ctl=ptr(h["mctl"]),
        onset_ctl=ptr(h["wctl"]), onset_table=ptr(h["table"]), onset_rows=h["table"].shape[0],
        **({} if gd is None else {"guide_ctl": ptr(gd), "guide_table": ptr(h["gtable"]), "guide_rows": h["gtable"].shape[0]}),
        **({} if ad is None else {"art_ctl": ptr(ad), "art_table": ptr(td), "art_rows": rows_arg}))
    call("commu_sample_topk", C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return lg.cpu(), tok.cpu(), pr.cpu(), lp.cpu()


def banned_bias(r, which="banned"):
    out = r["bias"].clone()
    for b, ids in enumerate(r[which]):
        out[b, ids] = NEG
    return out


def test_sampler_equals_the_launch_without_the_words_and_the_bans_in_the_bias(rows):
    """Fails on the parent: commu_sample_args has no art_ctl.  Fails for a kernel that ignores the row or the hold term: the
    bias makes an id the articulation bans the likely token.  Every row is compared, the Q12 row included."""
    r, n = rows, rows["n"]
    names = [c[0] for c in r["cases"]]
    got = launch(r, r["logits"])
    want = GG.launch(r, r["logits"], bias=banned_bias(r), **GG.NONE)          # (the class-control launch: none of the words)
    free = GG.launch(r, r["logits"])                                          # (the guide kernel: the other six words)
    for b in range(n):
        assert same_row(got, want, b), (names[b], int(got[1][b]), int(want[1][b]))
        for i in r["banned"][b]:
            assert float(got[2][b, i]) == 0.0 or int(got[1][b]) == -1, (names[b], i)
    # the same against the GUIDE kernel with the articulation's bans as -inf in the bias
    by_guide = GG.launch(r, r["logits"], bias=banned_bias(r, "art_banned"))
    for b in range(n):
        assert same_row(got, by_guide, b), names[b]
    # teeth: the launch without the articulation draws differently on the rows where the bias favours what it bans
    differ = [names[b] for b in range(n) if int(got[1][b]) != int(free[1][b])]
    took = [names[b] for b in range(n) if int(free[1][b]) in r["art_banned"][b]]
    print("rows:", n, "; rows with an articulation ban:", sum(bool(x) for x in r["art_banned"]), "; rows whose token differs "
          "from the launch without the articulation:", len(differ))
    assert set(took) <= set(differ) and len(took) >= 20
    for name in ("hold_f_24", "s0_m_64_seam", "s0_m_65_seam", "s0_m_127", "hold_into_the_next_bar", "hold_next_bar_wraps_R_g_2",
                 "s0_wraps_onto_the_same_block", "bar_line_a_127_cap_1", "seam_pitch_31", "seam_pitch_32", "seam_pitch_127",
                 "position_70_tokens_back", "position_140_tokens_back", "guide_rows_clamped_to_the_last_row",
                 "row_clamped_to_the_last_row", "velocity_bits_0_31_32_63", "dlo_gives_way_to_the_bar_line"):
        assert name in took, name
    for i in (130, 195, 303, 432):
        assert int(got[1][names.index("untouched_%d" % i)]) == i, i
    assert int((got[1] >= 1).sum()) >= n // 2
    nothing = names.index(NOTHING)
    assert int(got[1][nothing]) == -1 and bool(torch.isnan(got[3][nothing]).all())
    assert int(free[1][nothing]) in (305, 431)
    # Q5: the same two launches again on the logits the first ones left -- the same bans on the compounded rows
    got2 = launch(r, got[0])
    want2 = GG.launch(r, want[0], bias=banned_bias(r), **GG.NONE)
    for b in range(n):
        assert same_row(got2, want2, b), names[b]
    assert not torch.equal(bits(got2[0]), bits(got[0]))                   # (the sampled rows were divided again)


def test_off_words_and_a_free_row_are_the_guide_kernel_bit_for_bit(rows):
    r, n = rows, rows["n"]
    free = GG.launch(r, r["logits"])
    off = launch(r, r["logits"], articulation=torch.full((n,), -1, dtype=torch.int32))
    # (a template of two rows that constrain nothing, at base 3 of a table of its own whose other rows ban everything; the
    # reserved word holds anything)
    tab = torch.zeros((8, 4), dtype=torch.int32)
    tab[3:5] = torch.tensor([0, -1, -1, 12345], dtype=torch.int32)
    same = launch(r, r["logits"], articulation=torch.full((n,), W(3, 2), dtype=torch.int32), atable=tab)
    for b in range(n):
        assert same_row(off, free, b) and same_row(same, free, b), r["cases"][b][0]


def test_entry_point_refusal_and_ops(rows):
    from commu_amd import ops
    from commu_amd._lib import CommuHipError
    r, n = rows, rows["n"]
    for kw in (dict(guide=None), dict(atable=None), dict(n_rows=0), dict(n_rows=4097), dict(n_rows=-1)):
        with pytest.raises(CommuHipError, match="-22"):
            launch(r, r["logits"], **kw)
    d = lambda x: x.to(DEV)
    full = dict(uniforms=d(r["us"]), bias=d(r["bias"]), class_ctl=(d(r["cls"]), d(r["state"]), d(r["seq"])),
                note_order=d(r["ctl"]), voices=d(r["vctl"]), density=d(r["dctl"]), interval=d(r["mctl"]),
                onsets=(d(r["wctl"]), d(r["table"])))
    gde, art = (d(r["gctl"]), d(r["gtable"])), (d(r["actl"]), d(r["atable"]))
    with pytest.raises(CommuHipError, match="articulation: guide= expected"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, articulation=art, **full)
    with pytest.raises(CommuHipError, match="articulation controls"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, guide=gde, articulation=(art[0].float(), art[1]), **full)
    with pytest.raises(CommuHipError, match="articulation table"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, guide=gde, articulation=(art[0], art[1].reshape(-1, 2)), **full)
    with pytest.raises(CommuHipError, match="articulation: a pair"):
        ops.sample_topk(d(r["logits"].clone()), 5.0, 3, guide=gde, articulation=art[0], **full)
    # ops.sample_topk(articulation=) makes the same launch (it builds the all-off grammar and harmony itself)
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), top_p=0.3, guide=gde, articulation=art, **full)
    plain = dict(r, gram_on=torch.zeros_like(r["gram_on"]), harm_on=torch.zeros_like(r["harm_on"]))
    ref = launch(plain, r["logits"])
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))
    # where there is no guide: all -1 guide words over a one-row table -- the hold term does not apply
    lg = d(r["logits"].clone())
    tok = ops.sample_topk(lg, 5.0, 3, wrong=d(r["wrong"]), top_p=0.3,
                          guide=(torch.full((n,), -1, dtype=torch.int32, device=DEV),
                                 torch.full((1, 4), -1, dtype=torch.int32, device=DEV)), articulation=art, **full)
    ref = launch(plain, r["logits"], guide=torch.full((n,), -1, dtype=torch.int32))
    assert torch.equal(tok.cpu(), ref[1]) and torch.equal(bits(lg.cpu()), bits(ref[0]))


# ------------------------------------------------------------------------------------------------ 2. through the loop
run, separate_launches = GG.run, GG.separate_launches
fixture_model = NG.fixture_model
MELODY = GH.GUIDE                         # the host test's two-bar melody: avoid_intervals [1, 11], no_unison, 16 cells
HOLD = {"hold_guide": True, "within_bar": True, "duration": [2, 32]}          # (the host test's setting)
SHORT = {"bars": [{"duration": [1, 4], "velocity": [100, 127]}], "within_bar": True}
SOFT, LOUD = {"velocity": [0, 40]}, {"velocity": [90, 127]}
CYCLE = {"bars": [SOFT, LOUD]}            # (disjoint bars: a slot out of phase breaks the template at once)
ARTS = (HOLD, None, SHORT, None)
GUIDES = (MELODY, None, None, None)


def loaded(z, model, B, articulation=None, guide=None, onsets=None, **kw):
    """test_guide_gpu.loaded with set_articulation's value."""
    from commu_amd.generate import ForcedDecoder
    prompts, glen = kw.pop("prompts", None), kw.pop("glen", GG.GLEN)
    dec = ForcedDecoder(model, B, glen, 4146, 0.95, 32, **kw)
    dec.record_logprobs()
    dec.set_grammar(True)
    dec.set_logit_bias(HG.steer_row(HG.NOTES))
    if guide is not None:
        dec.set_guide(guide)
    if onsets is not None:
        dec.set_onsets(onsets)
    if articulation is not None:
        dec.set_articulation(articulation)
    HG.reload(z, dec, prompts)
    return dec


def violation(seq, lp, art, start, guide=None):
    """articulation_violation of a decoded sequence; a token was DRAWN where its log-probability pair is a number."""
    from commu_amd.generate import articulation_template, guide_template
    rows_, w, h = articulation_template(art)
    grows, cells = (None, 16) if guide is None else guide_template(guide)
    drawn = [not np.isnan(x) for x in np.asarray(lp)[:len(seq), 0]]
    return AC.articulation_violation(seq, start, rows_, grows, drawn, cells, w, h)


def drawn_of(seq, lp, start, lo, hi):
    return [i for i in range(start, len(seq)) if lo <= seq[i] <= hi and not np.isnan(np.asarray(lp)[i, 0])]


def check_on_slot(z, seq, lp, art, guide=None):
    from commu_amd.midi_generator.midi_inferrer import parse_events
    start = 1 + len(z["encoded_meta"])
    assert seq is not None and parse_events(seq, start) is None, seq
    assert violation(seq, lp, art, start, guide) is None, (art, seq)
    assert len(drawn_of(seq, lp, start, 304, 431)) >= 1
    if guide is not None:
        from commu_amd.generate import guide_template
        grows, cells = guide_template(guide)
        drawn = [not np.isnan(x) for x in np.asarray(lp)[:len(seq), 0]]
        assert GG.violation(seq, lp, guide, start) is None
        assert not any(h for _, h, _ in AC.held_into_ban(seq, start, grows, drawn, cells))


def test_alternating_slots_through_the_loop(fixture_model):
    """Fails on the parent: ForcedDecoder has no set_articulation.  Fails for a kernel that ignores the rows: the run without
    the feature draws durations and velocities both templates ban."""
    z, model = fixture_model
    B = 4
    start = 1 + len(z["encoded_meta"])
    plain = loaded(z, model, B)
    assert plain.art_ctl is None and plain.art_table is None and plain.guide_ctl is None and plain.cls_ctl is None
    s0, f0, l0 = run(plain)
    free, free_lp = plain.sequences()[0], plain.logprobs()
    res = []
    for mode in ("graph", "eager", "separate"):
        dec = loaded(z, model, B, articulation=list(ARTS), guide=list(GUIDES))
        assert dec.art_ctl.tolist() == [W(0, 1, True, True), -1, W(1, 1, True), -1]
        # (the rule implies none of the others: their words exist for the one kernel and are off where nobody set them)
        assert dec.guide_ctl.tolist() == [GD.word(0, 2, 3), -1, -1, -1] and dec.onset_ctl.tolist() == [-1] * B
        assert dec.interval_ctl.tolist() == [-1] * B and dec.density_ctl.tolist() == [-1] * B
        assert dec.voice_ctl.tolist() == [-1] * B and dec.order_ctl.tolist() == [-1] * B
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
        if ARTS[b] is not None:
            check_on_slot(z, seqs[b], lps[b], ARTS[b], GUIDES[b])
        else:
            assert torch.equal(sg[b], s0[b]) and torch.equal(fg[b], f0[b]) and torch.equal(bits(lg[b]), bits(l0[b])), b
    # teeth: the same request without the rule draws what the templates ban, and the rule changed the slots that are on
    broke = [(b, i) for b in range(B) for i, t in enumerate((HOLD, SHORT))
             if free[b] is not None and violation(free[b], free_lp[b], dict(t, hold_guide=False), start) is not None]
    print("without the rule: (slot, template) pairs with a drawn duration or velocity the template bans:", broke)
    assert broke
    assert any(not torch.equal(sg[b], s0[b]) for b in range(B) if ARTS[b] is not None)


def test_a_decoder_that_never_enables_the_feature_runs_the_parents_launches(fixture_model):
    """A decoder with a guide and no articulation passes no art_ctl: the guide kernel, whose instructions are the parent's
    (docs/EXPERIMENTS.md 9d).  Switching every slot's articulation off afterwards decodes the same tokens."""
    z, model = fixture_model
    ref = loaded(z, model, 4, guide=MELODY)
    assert ref.art_ctl is None and ref.art_table is None
    s0, f0, l0 = run(ref)
    dec = loaded(z, model, 4, guide=MELODY, articulation=HOLD)
    run(dec)
    dec.set_articulation(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.art_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


def test_a_primed_slot_continues_the_cycle_in_phase(fixture_model):
    """The prompt is the first bar and a half of a sequence the loop itself wrote under the template: it holds two Bars, so
    the open bar is bar 1 and the first drawn velocities follow row 1 (loud), not row 0 (soft) -- the rows are disjoint, so a
    slot that took bar 0's row would break the template with its first drawn velocity.  An onset template ({"grid": 8}: eight
    onsets a bar) keeps the bars short enough for the sequence to hold three."""
    z, model = fixture_model
    n_ctx = 1 + len(z["encoded_meta"])
    src = loaded(z, model, 2, articulation=CYCLE, onsets={"grid": 8})
    run(src)
    own, own_lp = src.sequences()[0][0], src.logprobs()[0]
    bars = [i for i, t in enumerate(own) if t == 2]
    assert len(bars) >= 3, own
    ends = [i for i in range(bars[1], bars[2]) if 304 <= own[i] <= 431 and not np.isnan(own_lp[i, 0])]
    cut = (ends[0] + 1) if ends else next(i for i in range(bars[1] + 1, bars[2] + 1) if not np.isnan(own_lp[i, 0]))
    prompt = own[n_ctx:cut]
    assert prompt.count(2) == 2
    dec = loaded(z, model, 2, articulation=CYCLE, onsets={"grid": 8}, max_prompt=len(prompt), prompts=[prompt] * 2)
    run(dec)
    seq, lp = dec.sequences()[0][0], dec.logprobs()[0]
    assert seq[:cut] == own[:cut] and len(seq) > cut + 4, seq
    assert int(dec.fsm.cpu()[0, F_NBAR]) == seq.count(2)
    after = drawn_of(seq, lp, cut, 131, 194)
    assert after and violation(seq, lp, CYCLE, cut) is None, seq
    nxt = [i for i in range(cut, len(seq)) if seq[i] == 2]
    first_bar = [2 * (seq[i] - 131) for i in after if not nxt or i < nxt[0]]
    assert all(v >= 90 for v in first_bar), (first_bar, seq)
    if first_bar:          # (out of phase -- bar 0's row for the open bar -- the same sequence breaks the template)
        assert violation(seq, lp, {"bars": [LOUD, SOFT]}, cut) is not None


def test_switching_in_place_under_one_capture(fixture_model):
    z, model = fixture_model
    plain = loaded(z, model, 4)
    s0, f0, l0 = run(plain)
    dec = loaded(z, model, 4, articulation=[None, SHORT, None, None])
    assert dec.graph is None
    s1, f1, l1 = run(dec)
    g, table = dec.graph, dec.art_table
    assert g is not None
    check_on_slot(z, dec.sequences()[0][1], dec.logprobs()[1], SHORT)
    for b in (0, 2, 3):
        assert torch.equal(s1[b], s0[b]) and torch.equal(bits(l1[b]), bits(l0[b])), b
    dec.set_articulation(None, rows=[1])
    dec.set_articulation(CYCLE, rows=[2])
    uni = HG.reload(z, dec)
    dec.rearm(3, uni[3], articulation=HOLD, guide=MELODY)
    s, f, l = run(dec)
    assert dec.graph is g and dec.art_table is table
    assert dec.art_ctl.tolist() == [-1, -1, W(1, 2), W(3, 1, True, True)] and dec.guide_ctl.tolist() == [-1, -1, -1, GD.word(0, 2, 3)]
    second, lps = dec.sequences()[0], dec.logprobs()
    check_on_slot(z, second[2], lps[2], CYCLE)
    check_on_slot(z, second[3], lps[3], HOLD, MELODY)
    for b in (0, 1):
        assert torch.equal(s[b], s0[b]) and torch.equal(f[b], f0[b]) and torch.equal(bits(l[b]), bits(l0[b])), b
    dec.rearm(3, uni[3], articulation=False, guide=False)
    dec.set_articulation(None)
    HG.reload(z, dec)
    s, f, l = run(dec)
    assert dec.graph is g and dec.art_ctl.tolist() == [-1] * 4
    assert torch.equal(s, s0) and torch.equal(f, f0) and torch.equal(bits(l), bits(l0))


# ------------------------------------------------------------------------------------------------ 3. the request pool
@pytest.mark.parametrize("primed", [False, True], ids=["commu_decode_arm", "commu_decode_arm_primed"])
def test_pool_requests_with_their_own_templates_equal_generate_stream_of_each_alone(primed):
    """Two requests with different articulations (one with hold_guide beside its own guide under the grammar, primed: its
    prompt cut from a sequence generated under the same controls; one without the grammar) and one without: each one's
    sequences equal generate_stream(slots=1) of the request alone -- the arm launch wrote each slot's word, the table is
    the pool's."""
    import commu_amd.generate as G
    import pool_contract as PC
    import pool_prime_contract as PP
    import test_pool_gpu as TP
    import test_pool_prime_gpu as TPP
    from commu_amd._lib import CommuHipError
    from commu_amd.midi_generator.midi_inferrer import parse_events
    model = TP._model()
    reqs = PC.four_requests(G)
    every = lambda seq, rep: seq is not None
    mine = dataclasses.replace(reqs[1], prompt=None, accept=every, need=2, grammar=True, logit_bias=None, guide=MELODY,
                               articulation=HOLD)
    if primed:
        own = TPP._own_sequence(TPP._generator(model), mine, 6, grammar=True, guide=MELODY, articulation=HOLD)
        mine = dataclasses.replace(mine, prompt=PP.prompt_of(own, len(PC.META), 6))
    want = TPP._alone(TPP._generator(model), mine, grammar=True, guide=MELODY, articulation=HOLD)
    second = dataclasses.replace(reqs[0], accept=every, grammar=False, articulation=SHORT)
    second_want = TPP._alone(TPP._generator(model), second, articulation=SHORT)
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
        assert violation(s, lp, HOLD, cut, MELODY) is None, s
    for s, lp in zip(res[0].sequences, res[0].logprobs):
        assert violation(s, lp, SHORT, TPP.N_CTX) is None, s
    # teeth: without articulation= the same request decodes something else
    free = TPP._alone(TPP._generator(model), dataclasses.replace(mine, articulation=None), grammar=True, guide=MELODY)
    assert free[0] != want[0]
    with pytest.raises(CommuHipError, match="request 0: articulation: hold_guide without a guide"):
        gen.generate_pool([dataclasses.replace(second, articulation=HOLD)], slots=1)


# ------------------------------------------------------------------------------------------------ 4. CLI
def test_generate_cli_articulation_end_to_end(golden_dir, tmp_path, monkeypatch):
    """generate.py --grammar --articulation on the reference-written checkpoint, every sequence that could be drawn accepted
    (a random model rarely passes the validators): every duration and velocity of what it writes is one the template allows
    -- neither is ever a forced token; the same run without the flag writes some it bans."""
    import test_model_gpu as TM
    from commu_amd.generate import articulation_template
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

    def go(argv, out):
        argv = common + ["--output_dir", str(tmp_path / out)] + argv
        margs, _ = parsers["model_args"].parse_known_args(argv)
        iargs, _ = parsers["input_args"].parse_known_args(argv)
        cli.main(margs, iargs, training_cfg=TM._g10_cfg(z, False))
        return json.load(open(tmp_path / out / "sequences.json"))

    spec = {"duration": [1, 4], "velocity": [100, 127], "within_bar": True}
    got = go(["--articulation", json.dumps(spec)], "articulated")
    free = go([], "free")
    start = 1 + len(got["encoded_meta"])
    rows_, w, h = articulation_template(spec)
    check = lambda s: AC.articulation_violation(s, start, rows_, within_bar=w, hold_guide=h)
    assert len(got["sequences"]) >= 1 and len(free["sequences"]) >= 1
    for s in got["sequences"]:
        assert parse_events(s, start) is None, s
        assert sum(1 for t in s[start:] if 304 <= t <= 431) >= 4 and check(s) is None, s
    assert any(check(s) is not None for s in free["sequences"])
