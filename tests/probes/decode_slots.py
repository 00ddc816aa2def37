"""What the number of decode slots does to the decode iteration: the bench model (L6 D512 H8 DI1024), graph replay, 64 / 128 /
192 / 256 slots.  Up to 256 slots run the fused layer-tail launches (csrc/decode_tail.hip); a tree from before that takes
the per-Linear chain beyond 64.

  --rows iter     ms per iteration and tokens/s (every slot draws one token per iteration: EOS, BAR and the chord tokens
                  are banned) at about 11 keys and at 1000 keys with the bf16 cache, and at 1000 keys with the fp8 cache.
                  A window is SUB iterations from the same state (the loop state is restored before every window, so the
                  keys stay within SUB of the nominal number); windows are repeated until they add up to >= 0.5 s.
  --rows stream   1024 sequences of generation_length 4096 to completion through 64 and through 256 slots
                  (BatchedGenerator.generate_stream), tokens of the returned sequences over the wall time.

To compare a commit with its parent run the probe from two checkouts IN TURN, each process on its own (--pkg DIR: the
commu-code_amd directory to import, with its library built; --tag names the rows), e.g. new, parent, new, parent: the two
runs of one tree give the A/A spread of every row.

JSON lines.    python tests/probes/decode_slots.py --rows iter|stream [--pkg DIR] [--tag NAME] [--slots 64,128,192,256] [--out FILE]
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
WARM, SUB, MIN_SECONDS, MIN_WINDOWS = 32, 128, 0.5, 3
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


def iter_row(model, dev, B, klen0, kv, tag):
    import torch
    from commu_amd.generate import ForcedDecoder
    GL = WARM + SUB + 64
    dec = ForcedDecoder(model, B, GL, klen0 + GL + 64, 0.95, 32, **({} if kv == "bf16" else {"kv_dtype": kv}))
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
    saved = [t.clone() for t in bufs]
    keys0 = int(st.klen.max())
    ts = []
    while len(ts) < MIN_WINDOWS or sum(ts) < MIN_SECONDS:
        for dst, src in zip(bufs, saved):
            dst.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.run_iterations(SUB, True)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    st.check()
    assert not bool(dec.fsm[:, 5].any()), "a probe sequence finished early"
    ms = [1e3 * t / SUB for t in ts]
    med = statistics.median(ms)
    return {"what": "iteration", "tree": tag, "slots": B, "kv": kv, "keys": [keys0, int(st.klen.max())], "fused": bool(st.tail_ok),
            "cache_bytes": st.cache_bytes(), "windows": len(ts), "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "tokens_per_s": round(1e3 * B / med, 0)}


def stream_row(model, dev, slots, tag, need=1024):
    import torch
    from commu_amd.generate import BatchedGenerator
    gen = BatchedGenerator(model, dev, 4096, 4146)
    accept = lambda seq, rep: True
    gen.generate_stream(META, data(), 0.95, 32, need=slots, accept=accept, slots=slots, seed=3)          # (graph build, untimed)
    dec = next(iter(gen._decoders.values()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, started = gen.generate_stream(META, data(), 0.95, 32, need=need, accept=accept, slots=slots, seed=3)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ntok = sum(len(s_) - 12 for s_ in got)
    return {"what": "stream to completion", "tree": tag, "slots": slots, "sequences": len(got), "attempts_started": started,
            "fused": bool(dec.state.tail_ok), "cache_bytes": dec.state.cache_bytes(), "seconds": round(dt, 3), "tokens": ntok,
            "tokens_per_s": round(ntok / dt, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["iter", "stream"], default="iter")
    ap.add_argument("--pkg", type=str, default=os.path.join(ROOT, "commu-code_amd"))
    ap.add_argument("--tag", type=str, default="this tree")
    ap.add_argument("--slots", type=str, default=None)
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
        model = build(dev)
        if a.rows == "iter":
            for kv, klen0 in (("bf16", 11), ("bf16", 1000), ("fp8", 1000)):
                for B in [int(x) for x in (a.slots or "64,128,192,256").split(",")]:
                    emit(iter_row(model, dev, B, klen0, kv, a.tag))
                    torch.cuda.empty_cache()
        else:
            for slots in [int(x) for x in (a.slots or "64,256").split(",")]:
                emit(stream_row(model, dev, slots, a.tag))
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
