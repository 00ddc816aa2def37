"""What class-keyed sampling (ForcedDecoder.set_class_sampling, commu_decode_loop_args.cls_ctl) costs per decode
iteration, and whether the default path moved: the bench model (L6 D512 H8), 64 slots, graph replay, the operating point of
sample_harm.py (every slot primed behind its first forced chord, 15 keys at the start, WARM = 32 warm-up iterations, a
timed window of SUB = 128 iterations from 47 to 175 keys: the "11 keys" rows of docs/EXPERIMENTS.md 8r / 8s).

  --rows iter     ms per iteration, decoders INTERLEAVED, REPS = 8 windows each from the same restored loop state:
                    null    -- never given a table (nor a grammar): the launch every decoder ran before;
                    gram    -- the default event grammar alone (the yardstick of 8r);
                    base    -- an all-inherit table in every slot (with the zero bias and the all-off grammar and harmony the
                               class kernel reads): the table's loads and the selection, no effect on what is drawn;
                    cls     -- the default grammar and {"pitch": T 1.1 / k 40, "duration": greedy, "boundary": T 0.8}.
                  A tree from before the feature runs `null` and `gram` only.  To compare with the parent run the probe
                  from two trees IN TURN, each process on its own (--pkg DIR: the commu-code_amd directory to import, with
                  its library built; --tag names the rows), e.g. parent, new, parent, new: the two runs of one tree give
                  the A/A spread the default path (`null`) of the other has to be inside.
  --rows kernel   the stand-alone sampling kernel (64 rows), 200 launches back to back in a captured graph, by HIP events:
                  no constraint, the default grammar, a zero harmony table (the 8.81 us row of 8s), the class kernel with
                  the same inputs and a table whose every record is the triple of the other rows.

JSON lines.    python tests/probes/sample_class.py --rows iter|kernel [--modes null,gram,base,cls] [--pkg DIR] [--tag NAME]
                                                   [--out FILE]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sample_harm as SH  # noqa: E402

B, WARM, SUB = SH.B, SH.WARM, SH.SUB
REPS = 8
TABLE = {"drawn": {"pitch": {"temperature": 1.1, "top_k": 40}, "duration": {"temperature": 0},
                   "boundary": {"temperature": 0.8}}}


def decoder(model, dev, mode):
    import numpy as np
    import torch
    from commu_amd.generate import ForcedDecoder
    GL = WARM + SUB + 64
    dec = ForcedDecoder(model, B, GL, GL + 128, 0.95, 32, max_prompt=len(SH.PRIME))
    if mode in ("gram", "cls"):
        dec.set_grammar(True)
    if mode == "base":
        dec.set_class_sampling(np.full((8, 3), np.nan))
    if mode == "cls":
        from commu_amd.generate import class_sampling
        dec.set_class_sampling(class_sampling(**TABLE))
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

    import torch
    from commu_amd.generate import ForcedDecoder
    if not hasattr(ForcedDecoder, "set_class_sampling"):
        modes = tuple(m for m in modes if m in ("null", "gram"))
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
    for m, (dec, _, _) in decs.items():
        dec.state.check()
        assert not bool(dec.fsm[:, 5].any()), "a probe sequence finished early"
        assert dec.graph is not None and (getattr(dec, "cls_ctl", None) is None) == (m in ("null", "gram"))
    first = decs[modes[0]]
    keys = [int(first[2][3].max()), int(first[0].state.klen.max())]
    return {"what": "decode iteration, graph replay", "tree": tag, "slots": B, "keys": keys,
            "ms_per_iteration": {m: SH.spread(times[m]) for m in modes},
            "values": {m: [round(t, 4) for t in times[m]] for m in modes}}


def kernel_rows(dev, tag):
    import numpy as np
    import torch
    from commu_amd import ops
    from commu_amd._lib import call
    from commu_amd.generate import event_grammar
    logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
    gram = torch.from_numpy(event_grammar()).to(dev)
    zero = torch.zeros(111, 16, device=dev)
    zbias = torch.zeros(B, 768, device=dev)
    t = torch.full((B,), 0.95, device=dev)
    k = torch.full((B,), 32, dtype=torch.int32, device=dev)
    p = torch.ones(B, device=dev)
    u = torch.rand(B, device=dev)
    tok = torch.zeros(B, dtype=torch.int32, device=dev)
    state = torch.zeros(B, call("commu_forcing_state_ints"), dtype=torch.int32, device=dev)
    state[:, 0] = 12
    state[:, 10] = 1
    seq = torch.full((B, 16), 600, dtype=torch.int32, device=dev)
    seq[:, 11] = 140                                                     # a velocity: the grammar admits pitches next
    chords = torch.tensor([[199 + 9 * (b % 12), 285] for b in range(B)], dtype=torch.int32, device=dev)
    on, off = torch.ones(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    work = logits.clone()
    modes = [("none", {}), ("gram", {"grammar": (gram, on, state, seq)}),
             ("harm_zero", {"bias": zbias, "grammar": (gram, off, state, seq), "harmony": (zero, on, state, chords)})]
    if hasattr(ops.sample_topk, "__code__") and "class_ctl" in ops.sample_topk.__code__.co_varnames:
        from commu_amd.generate import class_ctl_records, sampling_rows
        # every record the triple of the other rows: the 200 launches compound the row by the same temperature (Q5), and what
        # the radix select costs depends on how peaked the row has become -- records that differ would time another row
        table = np.full((8, 3), np.nan)
        rec = class_ctl_records(np.stack([table] * B), sampling_rows(B, 0.95, 32, 1.0))
        ctl = torch.from_numpy(rec.view(np.int32).reshape(B, 8, 4)).to(dev)
        modes.append(("cls", {"bias": zbias, "grammar": (gram, off, state, seq), "harmony": (zero, on, state, chords),
                              "class_ctl": (ctl, state, seq)}))

    def launches(kw):
        for _ in range(200):
            ops.sample_topk(work, t, k, uniforms=u, token=tok, top_p=p, **kw)
    graphs = {}
    for m, kw in modes:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches(kw)
        torch.cuda.current_stream().wait_stream(side)
        graphs[m] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[m]):
            launches(kw)
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
    ap.add_argument("--modes", type=str, default="null,gram,base,cls")
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
