"""What the event grammar (ForcedDecoder.set_grammar, commu_decode_loop_args.gram) costs per decode iteration and what
it buys: the bench model (L6 D512 H8), 64 slots, graph replay.

  --rows iter     ms per iteration at about 11 keys and at 1000 keys, decoders INTERLEAVED, REPS windows of SUB iterations
                  each from the same restored loop state:
                    null     -- never given a grammar: the launch without the pointers (what every decoder ran before);
                    off      -- table and switches allocated, every slot off: the zero row 7 is loaded, nothing changes;
                    default  -- event_grammar() in every slot.
                  A tree from before the feature runs `null` only.  To compare with the parent run the probe from two
                  checkouts IN TURN, each process on its own (--pkg DIR: the commu-code_amd directory to import, with its
                  library built; --tag names the rows; --modes null: this tree with the one decoder the parent's process
                  has -- three decoders interleaved evict each other's caches, one alone does not), e.g. new, parent, new,
                  parent: the two runs of one tree give the A/A spread.
  --rows kernel   the stand-alone sampling kernel (commu_sample_topk with commu_sample_args.gram, 64 rows), 200 launches
                  back to back by HIP events, as a graph replay (the device's time) and from Python (bound by the host):
                  no grammar, every row off, the default table.
  --rows waste    the decode fixture's small UNTRAINED model (tests/golden/g6_decode.npz), 64 slots, generation_length 512,
                  with and without the grammar: notes per sequence (count_notes) and draws per sequence that were not
                  appended (F_NDRAW minus the appended draws).

JSON lines.    python tests/probes/sample_grammar.py --rows iter|kernel|waste [--modes null,off,default] [--pkg DIR] [--tag NAME]
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
    return types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})


def spread(ts, digits=4):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def decoder(model, dev, mode, klen0):
    import torch
    from commu_amd.generate import ForcedDecoder
    GL = WARM + SUB + 64
    dec = ForcedDecoder(model, B, GL, klen0 + GL + 64, 0.95, 32)
    if mode != "null":
        dec.set_grammar(True)
        if mode == "off":
            dec.set_grammar(None)
    uni = torch.rand(B, dec.ld_u, generator=torch.Generator().manual_seed(5)).numpy()
    dec.load([META] * B, [data()] * B, uni)
    if klen0 > 11:
        ctx = torch.randint(3, 729, (klen0, B), generator=torch.Generator().manual_seed(3))
        ctx[0] = 0
        ctx[1:11] = torch.tensor(META[:10])[:, None]
        dec.state.prefill(ctx.to(dev))
    dec.pre()
    dec.run_iterations(WARM, True)
    torch.cuda.synchronize()
    st = dec.state
    bufs = (dec.fsm, dec.seq, dec.wrong, st.klen, st.logits, dec.tok, dec.active, dec.keep, dec.draw, dec.uni)
    return dec, bufs, [t.clone() for t in bufs]


def iter_rows(model, dev, klen0, tag, modes):
    import torch
    from commu_amd.generate import ForcedDecoder
    if not hasattr(ForcedDecoder, "set_grammar"):
        modes = ("null",)
    decs = {m: decoder(model, dev, m, klen0) for m in modes}
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
        assert dec.graph is not None and (getattr(dec, "gram", None) is None) == (m == "null")
    first = decs[modes[0]]
    keys = [int(first[2][3].max()), int(first[0].state.klen.max())]
    return {"what": "decode iteration, graph replay", "tree": tag, "slots": B, "keys": keys,
            "ms_per_iteration": {m: spread(times[m]) for m in modes}}


def kernel_rows(dev, tag):
    import torch
    from commu_amd import ops
    from commu_amd._lib import call
    from commu_amd.generate import event_grammar
    logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
    table = torch.from_numpy(event_grammar()).to(dev)
    t = torch.full((B,), 0.95, device=dev)
    k = torch.full((B,), 32, dtype=torch.int32, device=dev)
    p = torch.ones(B, device=dev)
    u = torch.rand(B, device=dev)
    tok = torch.zeros(B, dtype=torch.int32, device=dev)
    state = torch.zeros(B, call("commu_forcing_state_ints"), dtype=torch.int32, device=dev)
    state[:, 0] = 12
    seq = torch.full((B, 16), 600, dtype=torch.int32, device=dev)
    seq[:, 11] = torch.tensor([(2, 60, 140, 310, 432)[b % 5] for b in range(B)], dtype=torch.int32)
    on, off = torch.ones(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    work = logits.clone()
    modes = (("none", None), ("off", (table, off, state, seq)), ("default", (table, on, state, seq)))

    def launches(g):
        for _ in range(200):
            ops.sample_topk(work, t, k, uniforms=u, token=tok, top_p=p, **({} if g is None else {"grammar": g}))
    # 200 launches per mode captured in a graph: back-to-back launches from Python are bound by the host (about 8 us per
    # call, more with the argument checks of grammar=), a replay is the device's time
    graphs = {}
    for m, g in modes:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches(g)
        torch.cuda.current_stream().wait_stream(side)
        graphs[m] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[m]):
            launches(g)
    us = {m: [] for m, _ in modes}
    host = {m: [] for m, _ in modes}
    for rep in range(REPS + 1):
        for m, g in modes:
            for how, dst in ((graphs[m].replay, us), (lambda: launches(g), host)):
                work.copy_(logits)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                how()
                e.record()
                torch.cuda.synchronize()
                if rep:
                    dst[m].append(1e3 * s.elapsed_time(e) / 200)
    return {"what": "sampling kernel alone, 200 launches back to back", "tree": tag, "rows": B,
            "us_per_launch_graph_replay": {m: spread(us[m], 3) for m in us},
            "us_per_launch_from_python": {m: spread(host[m], 3) for m in host}}


def waste_rows(dev, tag):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_decode_gpu as TD
    from commu_amd.generate import ForcedDecoder
    from commu_amd.midi_generator.midi_inferrer import count_notes
    gold = os.path.join(ROOT, "tests", "golden")
    z = TD.load(gold, "g6_decode.npz")
    model = TD._build(gold, z, z["sample8m_bias"])
    out = []
    for grammar in (False, True):
        dec = ForcedDecoder(model, B, 512, 4146, 0.95, 32)
        dec.record_logprobs()
        if grammar:
            dec.set_grammar(True)
        uni = np.random.RandomState(11).random_sample((B, dec.ld_u)).astype(np.float32)
        dec.load([z["encoded_meta"].tolist()] * B, [TD._data(z, "sample8m")] * B, uni)
        dec.run(use_graph=True)
        torch.cuda.synchronize()
        seqs, lps = dec.sequences()[0], dec.logprobs()
        ndraw = dec.fsm[:, 12].cpu().numpy()
        notes = [count_notes(s) for s in seqs if s is not None]
        redraw = [int(ndraw[b]) - int((~np.isnan(lps[b][:, 0])).sum()) for b in range(B) if seqs[b] is not None]
        out.append({"what": "wasted decisions, untrained fixture model", "tree": tag, "slots": B, "generation_length": 512,
                    "grammar": grammar, "failed_q12": sum(s is None for s in seqs),
                    "tokens_per_sequence": round(float(np.mean([len(s) for s in seqs if s is not None])), 1),
                    "notes_per_sequence": round(float(np.mean(notes)), 2),
                    "draws_not_appended_per_sequence": round(float(np.mean(redraw)), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["iter", "kernel", "waste"], default="iter")
    ap.add_argument("--pkg", type=str, default=os.path.join(ROOT, "commu-code_amd"))
    ap.add_argument("--tag", type=str, default="this tree")
    ap.add_argument("--modes", type=str, default="null,off,default")
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
            model = build(dev)
            for klen0 in (11, 1000):
                emit(iter_rows(model, dev, klen0, a.tag, tuple(a.modes.split(","))))
                torch.cuda.empty_cache()
        elif a.rows == "kernel":
            emit(kernel_rows(dev, a.tag))
        else:
            for r in waste_rows(dev, a.tag):
                emit(r)


if __name__ == "__main__":
    main()
