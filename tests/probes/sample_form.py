"""What the form rule (ForcedDecoder.set_form, commu_decode_loop_args.form_ctl) costs, and whether the path that exists
moved: the operating point and the method of sample_articulation.py (the bench model L6 D512 H8, 64 slots, graph replay, WARM
warm-up iterations, a timed window of SUB iterations, REPS windows each, decoders INTERLEAVED, every window from the same
restored loop state).

  --rows iter     ms per iteration:
                    null        -- never given a form: the launches every decoder ran before (the parent's kernels);
                    form_off    -- the form kernels with every word off: the header of the slot's state and the replay token
                                   are loaded and stored, nothing is replayed, the slots draw what `null` draws;
                    form_replay -- every slot inside a replay bar for the whole window: its prompt is one bar of 48 notes and
                                   the slot's state is set to replay it (one chunk to scan per search); no draw is made, the
                                   sampling stage skips every slot.
                  A tree from before the feature runs null only.  To compare with the parent run the probe from two trees IN
                  TURN, each process on its own (--pkg DIR, --tag NAME), as sample_voices.py describes.
  --rows kernel   the fused loop launch alone (commu_decode_sample_post_pre, 64 rows, no model step), 200 launches back to back
                  in a captured graph, by HIP events, each window from the same restored state: without the form arguments
                  (the parent's kernel), with every word off, inside a replay bar whose next group lies in the first chunk,
                  and inside one whose next group lies 130 tokens on (three chunks).

JSON lines.    python tests/probes/sample_form.py --rows iter|kernel [--modes null,form_off,form_replay]
                                                  [--pkg DIR] [--tag NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sample_harm as SH  # noqa: E402
import sample_voices as SV  # noqa: E402

B, WARM, SUB, REPS = SV.B, SV.WARM, SV.SUB, SV.REPS
NEW = ("form_off", "form_replay")
N_NOTES = 48
SOURCE = [t for i in range(N_NOTES) for t in (432 + 2 * i, 150, 40 + i % 40, 304)]          # one bar of 48 short notes


def decoder(model, dev, mode):
    import torch
    from commu_amd.generate import ForcedDecoder
    GL = WARM + SUB + 64
    prompt = SH.PRIME + SOURCE          # (the same prompt in every mode: the memory lengths are the same)
    dec = ForcedDecoder(model, B, GL, GL + 128 + len(prompt), 0.95, 32, max_prompt=len(prompt))
    if mode in NEW:
        dec.set_form("AA")
    if mode == "form_off":
        dec.set_form(None)
    uni = torch.rand(B, dec.ld_u, generator=torch.Generator().manual_seed(5)).numpy()
    dec.load([SH.META] * B, [SH.data()] * B, uni, prompts=[prompt] * B)
    if mode == "form_replay":
        # (a probe's liberty: the rule never starts a replay inside a prompt, so the state is set by hand -- active, cursor
        # behind the prompt's BAR, end at the sequence's length, phase 0, the row of a full copy of bar 0, no group yet)
        first = 1 + len(SH.META)
        head = torch.tensor([1, first + 1, first + len(prompt), 0, 64 << 8, -1], dtype=torch.int32, device=dev)
        dec.form_state[:, :6] = head
    dec.pre()
    dec.run_iterations(WARM, True)
    torch.cuda.synchronize()
    st = dec.state
    bufs = (dec.fsm, dec.seq, dec.wrong, st.klen, st.logits, dec.tok, dec.active, dec.keep, dec.draw, dec.uni)
    if mode in NEW:
        bufs += (dec.form_state, dec.form_tok)
    return dec, bufs, [t.clone() for t in bufs]


def iter_rows(model, dev, tag, modes):
    import time

    import torch
    from commu_amd.generate import ForcedDecoder
    if not hasattr(ForcedDecoder, "set_form"):
        modes = tuple(m for m in modes if m not in NEW)
    decs = {m: decoder(model, dev, m) for m in modes}
    times = {m: [] for m in modes}
    for _ in range(REPS):                      # interleaved
        for m, (dec, bufs, saved) in decs.items():
            for dst, src in zip(bufs, saved):
                dst.copy_(src)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.run_iterations(SUB, True)
            torch.cuda.synchronize()
            times[m].append(1e3 * (time.perf_counter() - t0) / SUB)
    done, active, drew = {}, {}, {}
    for m, (dec, _, saved) in decs.items():
        dec.state.check()
        done[m] = int(dec.fsm[:, 5].sum())
        drew[m] = int(dec.fsm[:, 12].sum())
        assert dec.graph is not None and (getattr(dec, "form_ctl", None) is None) == (m not in NEW)
        if m in NEW:
            active[m] = int(dec.form_state[:, 0].sum())
    assert not done.get("null"), "a probe sequence finished early"
    if "form_replay" in decs:
        assert active["form_replay"] == B, "a slot left its replay bar inside the timed window"
    return {"what": "decode iteration, graph replay", "tree": tag, "slots": B, "slots_done": done, "slots_replaying": active,
            "variates_consumed": drew, "ms_per_iteration": {m: SH.spread(times[m]) for m in modes},
            "values": {m: [round(t, 4) for t in times[m]] for m in modes}}


def kernel_rows(dev, tag):
    import ctypes as C

    import torch
    from commu_amd import _lib
    from commu_amd._lib import call, struct_args
    N = 200
    LD = 8192
    NF = call("commu_forcing_state_ints")
    has_form = "form_ctl" in [n for n, _ in _lib.DecodeLoopArgs._fields_]
    i32, u8 = torch.int32, torch.uint8
    logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def world(gap):
        """64 slots behind [meta, BAR, 432, chord] + a source bar whose groups lie `gap` lone positions apart + [BAR, 432,
        chord]: the record as the loop would hold it (two bars, both chords consumed of 64)."""
        body = [0] + SH.META + [2, 432, 199]
        for i in range(N // 4 + 2):
            body += [433] * gap + [434 + i % 90, 150, 40 + i % 40, 304]
        end = len(body)
        body += [2, 432, 285]
        assert len(body) + N + 8 < LD
        seq = torch.zeros(B, LD, dtype=i32, device=dev)
        seq[:, :len(body)] = torch.tensor(body, dtype=i32, device=dev)
        fsm = torch.zeros(B, NF, dtype=i32, device=dev)
        # len, forced, redo, first, filled, done, failed, iters, nbar, nchord, cur, length_fit, ndraw, ntrace
        fsm[:] = torch.tensor([len(body), -1, 0, 0, 1, 0, 0, 0, 2, 64, 2, 1, 0, 0], dtype=i32, device=dev)
        head = [1, 1 + len(SH.META) + 1, end, 0, 64 << 8, -1]
        return seq, fsm, head
    chord_tok = torch.full((B, 64), 199, dtype=i32, device=dev)
    chord_pos = torch.full((B, 64), 432, dtype=i32, device=dev)
    wrong = torch.zeros(B, 729, dtype=u8, device=dev)
    utable = torch.rand(B, N + 8, device=dev)
    tok = torch.zeros(B, dtype=torch.long, device=dev)
    active, keep, draw = (torch.zeros(B, dtype=u8, device=dev) for _ in range(3))
    uni = torch.rand(B, device=dev)
    token = torch.zeros(B, dtype=i32, device=dev)
    work = logits.clone()
    modes = {}

    def add(name, gap, form, replay):
        seq, fsm, head = world(gap)
        kw = {}
        bufs = [fsm, seq, wrong, work, tok, active, keep, draw, uni]
        if form:
            ns = call("commu_form_state_ints")
            state = torch.zeros(B, ns, dtype=i32, device=dev)
            state[:, 5] = -1
            if replay:
                state[:, :6] = torch.tensor(head, dtype=i32, device=dev)
            ctl = torch.full((B,), 2 * 4096 if replay else -1, dtype=i32, device=dev)
            table = torch.zeros(4096, 4, dtype=i32, device=dev)
            table[1, 0] = 64 << 8
            ftok = torch.full((B,), -1, dtype=i32, device=dev)
            kw = dict(form_ctl=p(ctl), form_table=p(table), form_rows=4096, form_state=p(state), form_tok=p(ftok))
            bufs += [state, ftok]
            modes[name + "_keep"] = (ctl, table)
        draw.fill_(0 if replay else 1)
        keep.fill_(1)
        a = struct_args(_lib.DecodeLoopArgs, logits=p(work), ld=768, V=729, B=B, wrong=p(wrong), temperature=0.95, top_k=32,
                        top_p=1.0, token=p(token), state=p(fsm), seq=p(seq), ld_seq=LD, chord_tok=p(chord_tok),
                        chord_pos=p(chord_pos), ld_chord=64, utable=p(utable), ld_u=N + 8, max_iters=1 << 30, tok=p(tok),
                        active=p(active), keep=p(keep), draw=p(draw), uni=p(uni), lmax=1 << 30, **kw)
        saved = [t.clone() for t in bufs]

        def launches():
            for _ in range(N):
                call("commu_decode_sample_post_pre", C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launches()
        modes[name] = (g, bufs, saved, a, fsm, kw.get("form_state") is not None and state)
    add("null", 0, False, False)
    if has_form:
        add("form_off", 0, True, False)
        add("form_replay_1chunk", 0, True, True)
        add("form_replay_3chunks", 130, True, True)
    names = [m for m in modes if not m.endswith("_keep")]
    us = {m: [] for m in names}
    info = {}
    for rep in range(REPS + 1):
        for m in names:
            g, bufs, saved, a, fsm, state = modes[m]
            for dst, src in zip(bufs, saved):
                dst.copy_(src)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            if rep:
                us[m].append(1e3 * s.elapsed_time(e) / N)
            info[m] = {"done": int(fsm[:, 5].sum()), "drawn": int(fsm[:, 12].sum()),
                       "replaying": None if state is False else int(state[:, 0].sum())}
    return {"what": "fused loop launch alone, 200 launches back to back", "tree": tag, "rows": B, "after_the_window": info,
            "us_per_launch_graph_replay": {m: SH.spread(us[m], 3) for m in us}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["iter", "kernel"], default="iter")
    ap.add_argument("--pkg", type=str, default=os.path.join(SH.ROOT, "commu-code_amd"))
    ap.add_argument("--tag", type=str, default="this tree")
    ap.add_argument("--modes", type=str, default="null,form_off,form_replay")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    dev = torch.device("cuda")
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
    with torch.no_grad():
        if a.rows == "iter":
            emit(iter_rows(SH.build(dev), dev, a.tag, tuple(a.modes.split(","))))
        else:
            emit(kernel_rows(dev, a.tag))


if __name__ == "__main__":
    main()
