"""What the articulation rule (ForcedDecoder.set_articulation, commu_decode_loop_args.art_ctl) costs, and whether the paths
that exist moved: the operating point and the method of sample_guide.py (the bench model L6 D512 H8, 64 slots, graph replay,
every slot primed behind its first forced chord, WARM warm-up iterations, a timed window of SUB iterations, REPS windows each,
decoders INTERLEAVED, every window from the same restored loop state).

  --rows iter     ms per iteration:
                    null     -- never given a grammar or a control word: the launch every decoder ran before;
                    gde_off  -- the default grammar, the note order, voice word 0, the density, interval and onset words off
                                and the guide kernel with every guide word off: the kernel the new one extends;
                    art_off  -- the same with the articulation kernel and every articulation word off again: the row is
                                loaded (row 0) and replaced by one that constrains nothing, the hold loads read row 0, nothing
                                more is banned, the slots draw what `gde_off` draws;
                    art_win  -- the same with the static window {"duration": [2, 32]} in every slot (guide words off);
                    art_hold -- sample_guide.py's 16-cell guide in every slot and {"hold_guide": true, "within_bar": true,
                                "duration": [2, 32]}: other tokens are drawn, so the difference to art_off is behaviour too.
                  A tree from before the feature runs null and gde_off only.  To compare with the parent run the probe from
                  two trees IN TURN, each process on its own (--pkg DIR, --tag NAME), as sample_voices.py describes.
  --rows kernel   the stand-alone sampling kernel (64 rows), 200 launches back to back in a captured graph, by HIP events:
                  the guide kernel with every word off on a run of 4 tokens (one chunk) and behind two bars of 80 tokens
                  (three chunks), then the articulation kernel on the same inputs with every word off, with the static window
                  only, and with hold_guide over the 16-cell guide.  The rows end in a pitch, so that a duration comes next and
                  the hold term has its a and its k.

JSON lines.    python tests/probes/sample_articulation.py --rows iter|kernel [--modes null,gde_off,art_off,art_win,art_hold]
                                                          [--pkg DIR] [--tag NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sample_guide as SG  # noqa: E402
import sample_harm as SH  # noqa: E402
import sample_voices as SV  # noqa: E402

B, WARM, SUB, REPS = SV.B, SV.WARM, SV.SUB, SV.REPS
GUIDE = SG.GUIDE
WINDOW = {"duration": [2, 32]}
HOLD = {"hold_guide": True, "within_bar": True, "duration": [2, 32]}
NEW = ("art_off", "art_win", "art_hold")


def decoder(model, dev, mode):
    import torch
    from commu_amd.generate import ForcedDecoder
    GL = WARM + SUB + 64
    dec = ForcedDecoder(model, B, GL, GL + 128, 0.95, 32, max_prompt=len(SH.PRIME))
    if mode != "null":
        dec.set_grammar(True)
        dec.set_note_order(True)
        dec.set_voices(0)
        dec.set_guide(GUIDE)
        if mode != "art_hold":
            dec.set_guide(None)
    if mode in NEW:
        dec.set_articulation(HOLD if mode == "art_hold" else WINDOW)
    if mode == "art_off":
        dec.set_articulation(None)
    uni = torch.rand(B, dec.ld_u, generator=torch.Generator().manual_seed(5)).numpy()
    dec.load([SH.META] * B, [SH.data()] * B, uni, prompts=[SH.PRIME] * B)
    dec.pre()
    dec.run_iterations(WARM, True)
    torch.cuda.synchronize()
    st = dec.state
    bufs = (dec.fsm, dec.seq, dec.wrong, st.klen, st.logits, dec.tok, dec.active, dec.keep, dec.draw, dec.uni)
    return dec, bufs, [t.clone() for t in bufs]


def iter_rows(model, dev, tag, modes):
    import time

    import numpy as np
    import torch
    from commu_amd.generate import ForcedDecoder
    if not hasattr(ForcedDecoder, "set_articulation"):
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
    done, scan = {}, {}
    for m, (dec, _, saved) in decs.items():
        dec.state.check()
        done[m] = int(dec.fsm[:, 5].sum())
        assert dec.graph is not None and (getattr(dec, "art_ctl", None) is None) == (m not in NEW)
        assert (dec.guide_ctl is None) == (m == "null")
        c1 = SV.chunks(dec.fsm.cpu(), dec.seq.cpu())
        scan[m] = {"end_mean": round(float(np.mean(c1)), 2), "end_max": max(c1)}
    assert not done.get("null"), "a probe sequence finished early"
    return {"what": "decode iteration, graph replay", "tree": tag, "slots": B, "slots_done": done, "scan_chunks": scan,
            "ms_per_iteration": {m: SH.spread(times[m]) for m in modes},
            "values": {m: [round(t, 4) for t in times[m]] for m in modes}}


def kernel_rows(dev, tag):
    import numpy as np
    import torch
    from commu_amd import ops
    from commu_amd._lib import call
    from commu_amd.generate import (GUIDE_ROWS_MAX, ONSET_ROWS_MAX, class_ctl_records, event_grammar, guide_template, guide_word,
                                    sampling_rows)
    logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
    gram = torch.from_numpy(event_grammar()).to(dev)
    zero = torch.zeros(111, 16, device=dev)
    zbias = torch.zeros(B, 768, device=dev)
    t = torch.full((B,), 0.95, device=dev)
    k = torch.full((B,), 32, dtype=torch.int32, device=dev)
    p = torch.ones(B, device=dev)
    u = torch.rand(B, device=dev)
    tok = torch.zeros(B, dtype=torch.int32, device=dev)
    chords = torch.tensor([[199 + 9 * (b % 12), 285] for b in range(B)], dtype=torch.int32, device=dev)
    on, off = torch.ones(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    rec = class_ctl_records(np.stack([np.full((8, 3), np.nan)] * B), sampling_rows(B, 0.95, 32, 1.0))
    ctl = torch.from_numpy(rec.view(np.int32).reshape(B, 8, 4)).to(dev)

    def sequences(bars, notes_per_bar):
        """sample_guide.py's with the last group cut behind its PITCH: meta, then `bars` bars of short notes on rising
        onsets; the record's bar count as the forcing stage keeps it."""
        body = [600] * 11
        for _ in range(bars):
            body += [2]
            for i in range(notes_per_bar):
                body += [432 + 4 * i, 150, 40 + i, 304]
        body += [432 + 4 * notes_per_bar, 150, 63]
        state = torch.zeros(B, call("commu_forcing_state_ints"), dtype=torch.int32, device=dev)
        state[:, 0] = len(body)
        state[:, 8] = bars
        state[:, 10] = 1
        seq = torch.full((B, 256), 600, dtype=torch.int32, device=dev)
        seq[:, :len(body)] = torch.tensor(body, dtype=torch.int32, device=dev)
        return state, seq
    s1, s3 = sequences(1, 1), sequences(2, 20)          # 19 tokens: one chunk; 11 + 2 * 81 + 3 tokens: three chunks
    word = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
    otable = torch.full((ONSET_ROWS_MAX, 4), -1, dtype=torch.int32, device=dev)
    rows, cells = guide_template(GUIDE)
    gtable = torch.full((GUIDE_ROWS_MAX, 4), -1, dtype=torch.int32, device=dev)
    gtable[:len(rows)] = torch.from_numpy(rows.view(np.int32)).to(dev)
    g_on = word(guide_word(0, len(rows) // (1 + cells), cells))

    def kw(st, guide, art):
        state, seq = st
        d = {"bias": zbias, "grammar": (gram, off, state, seq), "harmony": (zero, on, state, chords),
             "class_ctl": (ctl, state, seq), "note_order": word(0), "voices": word(0), "density": word(-1),
             "interval": word(-1), "onsets": (word(-1), otable), "guide": (guide, gtable)}
        if art is not None:
            d["articulation"] = art
        return d
    modes = [("gde_off_1chunk", kw(s1, word(-1), None)), ("gde_off_3chunks", kw(s3, word(-1), None))]
    if "articulation" in ops.sample_topk.__code__.co_varnames:
        from commu_amd.generate import ARTICULATION_ROWS_MAX, articulation_template, articulation_word
        atable = torch.zeros((ARTICULATION_ROWS_MAX, 4), dtype=torch.int32, device=dev)
        atable[:, 1:3] = -1
        arows, w, h = articulation_template(HOLD)
        atable[:len(arows)] = torch.from_numpy(arows.view(np.int32)).to(dev)
        a_win, a_hold = word(articulation_word(0, 1)), word(articulation_word(0, 1, w, h))
        for name, st in (("1chunk", s1), ("3chunks", s3)):
            modes += [("art_off_" + name, kw(st, word(-1), (word(-1), atable))),
                      ("art_win_" + name, kw(st, word(-1), (a_win, atable))),
                      ("art_hold_" + name, kw(st, g_on, (a_hold, atable)))]
    work = logits.clone()

    def launches(kw_):
        for _ in range(200):
            ops.sample_topk(work, t, k, uniforms=u, token=tok, top_p=p, **kw_)
    graphs = {}
    for m, kw_ in modes:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches(kw_)
        torch.cuda.current_stream().wait_stream(side)
        graphs[m] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[m]):
            launches(kw_)
    us = {m: [] for m, _ in modes}
    for rep in range(REPS + 1):
        for m, _ in modes:
            work.copy_(logits)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            graphs[m].replay()
            e.record()
            torch.cuda.synchronize()
            if rep:
                us[m].append(1e3 * s.elapsed_time(e) / 200)
    return {"what": "sampling kernel alone, 200 launches back to back", "tree": tag, "rows": B,
            "us_per_launch_graph_replay": {m: SH.spread(us[m], 3) for m in us}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["iter", "kernel"], default="iter")
    ap.add_argument("--pkg", type=str, default=os.path.join(SH.ROOT, "commu-code_amd"))
    ap.add_argument("--tag", type=str, default="this tree")
    ap.add_argument("--modes", type=str, default="null,gde_off,art_off,art_win,art_hold")
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
