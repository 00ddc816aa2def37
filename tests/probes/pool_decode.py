"""What the request pool (BatchedGenerator.generate_pool, csrc/decode_arm.hip) buys and costs: the bench model (L6 D512
H8), generation_length 256, sampled, EOS possible so that lengths are ragged, everything INTERLEAVED in one process.

  small   N requests of need 3 (the README example's meta with a varied last token and chord rows): generate_pool at 64 and
          at 256 slots against the same requests one after the other through generate_stream on ONE BatchedGenerator
          (model loaded once, decoder and graph reused) -- generate_stream's code is the parent commit's, so that leg is
          the parent's number.  tokens/s = generated tokens of the returned sequences / wall time.
  large   one request of need 256 at 64 slots: generate_pool against generate_stream, 5 interleaved runs.
  arm     the arm launch for 1, 16 and 64 jobs (stream events around the launch, and around copy + launch; host time of
          arm()), rearm() of as many slots (host, device), and the admission (host, device) per request.

JSON lines.    python tests/probes/pool_decode.py [--requests 200] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "commu-code_amd"))

L, H, D, DI = 6, 8, 512, 1024
GLEN = 256
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
        bias[1] = 1.5                         # EOS now and then: ragged lengths, slots free up at different times
        bias[2] = 1.5                         # bars: the chord progressions are consumed
        bias[195:304] = -1e9
    return model


def requests(G, n, need):
    out = []
    for i in range(n):
        chords = [199 + (i * 7 + j) % 100 for j in range(4)]
        d = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": chords, "chord_position": [432] * 4})
        out.append(G.PoolRequest(META[:-1] + [700 + i % 28], d, need, 0.95, 32, seed=i))
    return out


def tokens(seqs):
    return sum(len(s) - 1 - len(META) for s in seqs)


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def small(gen, G, n, reps, out):
    reqs = requests(G, n, 3)
    accept = lambda seq, rep: seq is not None

    def sequential():
        return [gen.generate_stream(r.encoded_meta, r.input_data, r.temperature, r.top_k, r.need, accept, seed=r.seed)[0]
                for r in reqs]
    legs = {"sequential": sequential,
            "pool64": lambda: [r.sequences for r in gen.generate_pool(reqs, slots=64)],
            "pool256": lambda: [r.sequences for r in gen.generate_pool(reqs, slots=256)]}
    for fn in legs.values():          # warm-up: decoders, graphs
        fn()
    secs, toks = {k: [] for k in legs}, {}
    for _ in range(reps):
        for k, fn in legs.items():
            t, seqs = wall(fn)
            secs[k].append(t)
            toks[k] = sum(tokens(s) for s in seqs)
    r = {"what": f"{n} requests of need 3", "tokens": toks, "pool_stats_256": {k: (v if k != "arms" else len(v))
                                                                             for k, v in gen.pool_stats.items()}}
    for k in legs:
        r[k] = {"seconds": spread(secs[k]), "tokens_per_s": round(toks[k] / statistics.median(secs[k]), 1)}
    for k in ("pool64", "pool256"):
        r[k + "_over_sequential"] = round(r[k]["tokens_per_s"] / r["sequential"]["tokens_per_s"], 2)
    print(json.dumps(r), flush=True)
    out.append(r)


def large(gen, G, out):
    (req,) = requests(G, 1, 256)
    accept = lambda seq, rep: seq is not None
    legs = {"stream": lambda: gen.generate_stream(req.encoded_meta, req.input_data, 0.95, 32, 256, accept, slots=64,
                                                  seed=req.seed)[0],
            "pool": lambda: gen.generate_pool([req], slots=64)[0].sequences}
    for fn in legs.values():
        fn()
    secs, toks = {k: [] for k in legs}, {}
    for _ in range(5):
        for k, fn in legs.items():
            t, seqs = wall(fn)
            secs[k].append(t)
            toks[k] = tokens(seqs)
    r = {"what": "one request of need 256 at 64 slots", "tokens": toks, "stream_s": spread(secs["stream"]),
         "pool_s": spread(secs["pool"]), "stream_runs": [round(t, 4) for t in secs["stream"]],
         "pool_runs": [round(t, 4) for t in secs["pool"]],
         "pool_over_stream": round(statistics.median(secs["pool"]) / statistics.median(secs["stream"]), 4)}
    print(json.dumps(r), flush=True)
    out.append(r)


def arm(model, G, out):
    import torch
    from commu_amd import ops
    B = 64
    d = requests(G, 1, 1)[0].input_data
    dec = G.ForcedDecoder(model, B, GLEN, 4146, 0.95, 32)
    dec.record_logprobs()
    dec.pool_open(len(META))
    adm = []
    for e in range(B):
        t, _ = wall(lambda: dec.admit(e, META, d, sampling=(0.95, 32, 1.0)))
        adm.append(1e3 * t)
    uni = G.BatchedGenerator.attempt_uniforms(1, 0, dec.ld_u)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    r = {"what": "arm launch, admission, rearm", "slots": B, "ld_u": dec.ld_u,
         "admit_ms_per_request": spread(adm[4:])}
    for n in (1, 16, 64):
        jobs = [(b, b, uni) for b in range(n)]
        host, dev_all, dev_launch = [], [], []
        for _ in range(12):
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            dec.arm(jobs)
            host.append(1e6 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            dev_all.append(1e3 * e0.elapsed_time(e1))
            e2, e3 = ev(), ev()
            e2.record()
            ops.decode_arm(dec._pool_args(), n)
            e3.record()
            torch.cuda.synchronize()
            dev_launch.append(1e3 * e2.elapsed_time(e3))
        r[f"arm_{n}_jobs"] = {"host_us": spread(host[2:]), "copy_and_launch_us": spread(dev_all[2:]),
                              "launch_us": spread(dev_launch[2:])}
    ref = G.ForcedDecoder(model, B, GLEN, 4146, 0.95, 32)
    ref.record_logprobs()
    ref.load([META] * B, [d] * B, None)
    for n in (1, 16, 64):
        host, devt = [], []
        for _ in range(6):
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for b in range(n):
                ref.rearm(b, uni)
            host.append(1e6 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            devt.append(1e3 * e0.elapsed_time(e1))
        r[f"rearm_{n}_slots"] = {"host_us": spread(host[1:]), "device_us": spread(devt[1:])}
    print(json.dumps(r), flush=True)
    out.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import commu_amd.generate as G
    dev = torch.device("cuda")
    rows = []
    with torch.no_grad():
        model = build(dev)
        gen = G.BatchedGenerator(model, dev, generation_length=GLEN, memory_length=4146)
        arm(model, G, rows)
        large(gen, G, rows)
        small(gen, G, a.requests, a.reps, rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
