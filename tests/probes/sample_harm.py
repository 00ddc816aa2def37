"""What the harmony constraint (ForcedDecoder.set_harmony, commu_decode_loop_args.harm) costs per decode iteration:
the bench model (L6 D512 H8), 64 slots, graph replay.  Every slot is primed behind its first forced chord (bar, position 0,
Chord_am), so the strict table has a chord row to apply; the model's bias keeps bars, EOS and chord tokens away afterwards,
so every iteration is a model step and a draw.  A slot starts at 15 keys (12 of the context, 3 of the prompt); the WARM = 32
warm-up iterations bring it to 47 and the timed window of SUB = 128 iterations runs from 47 to 175 keys.  That is the
operating point of the "11 keys" rows of sample_grammar.py, the yardstick (it starts at 11 keys, warms and times the same
32 + 128 iterations: docs/EXPERIMENTS.md 8r lists its rows as 42 ... 170 keys), four keys further on because of the prompt,
so the rows compare with the grammar's.  It is not a measurement AT 11 keys (sample_bias.py, with 16 warm-up iterations and
windows of 32, times from 27 keys on): at a shorter memory the sampling stage is a larger share of the iteration.

  --rows iter     ms per iteration, decoders INTERLEAVED, REPS windows of SUB iterations each from the same restored loop
                  state:
                    null    -- never given a table (nor a grammar): the launch every decoder ran before;
                    zero    -- an all-zero table switched on in every slot (with the zero bias and the all-off grammar the
                               harmony kernel reads): the loads and the adds, no effect;
                    gram    -- the default event grammar alone (the yardstick: docs/EXPERIMENTS.md 8r);
                    strict  -- harmony_table() and the default event grammar in every slot.
                  A tree from before the feature runs `null` only.  To compare with the parent run the probe from two
                  checkouts IN TURN, each process on its own (--pkg DIR: the commu-code_amd directory to import, with its
                  library built; --tag names the rows; --modes null: one decoder alone, as the parent's process has), e.g.
                  new, parent, new, parent: the two runs of one tree give the A/A spread.
  --rows kernel   the stand-alone sampling kernel (64 rows), 200 launches back to back in a captured graph, by HIP events:
                  no constraint, the default grammar, a zero harmony table, the strict table with the grammar.

JSON lines.    python tests/probes/sample_harm.py --rows iter|kernel [--modes null,zero,gram,strict] [--pkg DIR] [--tag NAME]
                                                  [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, D, DI = 6, 8, 512, 1024
B = 64
WARM, SUB, REPS = 32, 128, 7
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]
CHORDS = [199, 285, 267, 258]
PRIME = [2, 432, 199]


def build(dev):
    import torch
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.train import build_model
    cfg = get_cfg(num_layers=L, num_heads=H, units=D, inner_size=DI, tgt_length=1, mem_length=4146, dropout=0.0,
                  attention_dropout=0.0, same_length=True)
    model = build_model(cfg, BaseVocab(), dev, seed=1).eval()
    with torch.no_grad():
        bias = model.crit.out_layers[0].bias
        bias.zero_()
        bias[1:3] = -1e9                      # no EOS / BAR, no chord tokens: every iteration is a model step and a draw
        bias[195:304] = -1e9
    return model


def data():
    return types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": CHORDS,
                                                                           "chord_position": [432] * len(CHORDS)})


def spread(ts, digits=4):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def decoder(model, dev, mode):
    import numpy as np
    import torch
    from commu_amd.generate import ForcedDecoder
    GL = WARM + SUB + 64
    dec = ForcedDecoder(model, B, GL, GL + 128, 0.95, 32, max_prompt=len(PRIME))
    if mode in ("gram", "strict"):
        dec.set_grammar(True)
    if mode == "zero":
        dec.set_harmony(np.zeros((111, 16), np.float32))
    if mode == "strict":
        dec.set_harmony(True)
    uni = torch.rand(B, dec.ld_u, generator=torch.Generator().manual_seed(5)).numpy()
    dec.load([META] * B, [data()] * B, uni, prompts=[PRIME] * B)
    dec.pre()
    dec.run_iterations(WARM, True)
    torch.cuda.synchronize()
    st = dec.state
    bufs = (dec.fsm, dec.seq, dec.wrong, st.klen, st.logits, dec.tok, dec.active, dec.keep, dec.draw, dec.uni)
    return dec, bufs, [t.clone() for t in bufs]


def iter_rows(model, dev, tag, modes):
    import torch
    from commu_amd.generate import ForcedDecoder
    if not hasattr(ForcedDecoder, "set_harmony"):
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
        assert bool((dec.fsm[:, 10] == 1).all()), "every slot sits behind its first chord"
        assert dec.graph is not None and (getattr(dec, "harm", None) is None) == (m in ("null", "gram"))
    first = decs[modes[0]]
    keys = [int(first[2][3].max()), int(first[0].state.klen.max())]
    return {"what": "decode iteration, graph replay", "tree": tag, "slots": B, "keys": keys,
            "ms_per_iteration": {m: spread(times[m]) for m in modes}}


def kernel_rows(dev, tag):
    import numpy as np
    import torch
    from commu_amd import ops
    from commu_amd._lib import call
    from commu_amd.generate import event_grammar, harmony_table
    logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
    gram = torch.from_numpy(event_grammar()).to(dev)
    strict = torch.from_numpy(harmony_table()).to(dev)
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
    modes = (("none", {}), ("gram", {"grammar": (gram, on, state, seq)}),
             ("zero", {"bias": zbias, "grammar": (gram, off, state, seq), "harmony": (zero, on, state, chords)}),
             ("strict", {"bias": zbias, "grammar": (gram, on, state, seq), "harmony": (strict, on, state, chords)}))

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
            "us_per_launch_graph_replay": {m: spread(us[m], 3) for m in us}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["iter", "kernel"], default="iter")
    ap.add_argument("--pkg", type=str, default=os.path.join(ROOT, "commu-code_amd"))
    ap.add_argument("--tag", type=str, default="this tree")
    ap.add_argument("--modes", type=str, default="null,zero,gram,strict")
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
            emit(iter_rows(build(dev), dev, a.tag, tuple(a.modes.split(","))))
        else:
            emit(kernel_rows(dev, a.tag))


if __name__ == "__main__":
    main()
