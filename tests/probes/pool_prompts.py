"""What per-request prompts cost and buy in the request pool (BatchedGenerator.generate_pool with PoolRequest(prompt=),
csrc/decode_arm.hip): the bench model's geometry (L6 D512 H8, d_head 64), everything INTERLEAVED in one process.

  arm       the arm launch alone on synthetic operands: 1, 16 and 64 jobs with images of 16, 256 and 1000 rows, bf16 and
            fp8 -- commu_decode_arm_primed (one workgroup per (layer, head, job, chunk of rows)) against commu_decode_arm (one
            wave per (layer, head, job), the parent's kernel, which takes a store of any ctx_rows) handed the same store;
            stream events around one launch, the two kernels alternating.  Copy bandwidth = bytes read + written over the
            time, beside a 1 GiB device-to-device copy on the same box (what tests/probes/hbm_calib.py moves).
  end       N requests of need 3, each with its own 256-token prompt (cut from a sequence generated for that request with
            EOS banned and bars made rare): generate_pool at 64 and at 256 slots against the same requests one after the
            other through generate_stream(prompt=) -- the parent commit's path.  tokens/s = generated tokens (after the
            prompt) of the returned sequences / wall time.
  unprimed  the EXPERIMENTS 8x row again: N unprimed requests of need 3 through generate_pool at 64 and 256 slots.  --tree
            names the checkout whose package is imported, so that this commit and its parent can be run alternately.

JSON lines.    python tests/probes/pool_prompts.py [arm] [end] [unprimed] [--requests 200] [--reps 3] [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, D, DI, DH = 6, 8, 512, 1024, 64
GLEN = 256
PROMPT = 256
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]
NF = 14


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


def requests(G, n, need, **kw):
    out = []
    for i in range(n):
        chords = [199 + (i * 7 + j) % 100 for j in range(4)]
        d = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": chords, "chord_position": [432] * 4})
        out.append(G.PoolRequest(META[:-1] + [700 + i % 28], d, need, 0.95, 32, seed=i, **kw))
    return out


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def spread(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


# ------------------------------------------------------------------------------------------------------------ arm launch
def arm(out, reps=24):
    import torch
    from commu_amd import ops
    dev, B, R, Lmax, ld_u, ld_seq, ld_chord = "cuda", 64, 64, 1024, GLEN + 1, 16 + GLEN + 2 + PROMPT, 64
    i32 = torch.int32
    ev = lambda: torch.cuda.Event(enable_timing=True)
    # the yardstick: a 1 GiB device-to-device copy (reads 1 GiB, writes 1 GiB)
    a = torch.empty(1 << 28, device=dev, dtype=torch.float32).normal_()
    b = torch.empty_like(a)
    ts = []
    for _ in range(6):
        e0, e1 = ev(), ev()
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    d2d = 2 * (1 << 30) / (statistics.median(ts[2:]) * 1e-3) / 1e9
    del a, b
    print(json.dumps({"what": "1 GiB device-to-device copy", "GB_per_s": round(d2d, 1)}), flush=True)
    out.append({"what": "d2d", "GB_per_s": round(d2d, 1)})
    z = lambda *s, dtype=i32: torch.zeros(*s, dtype=dtype, device=dev)
    for kv in ("bf16", "fp8"):
        rbs = [DH * 2, DH * 2] if kv == "bf16" else [DH, DH, DH // 32, DH // 32]
        cache = tuple(torch.zeros(L, B, H, Lmax, rb, dtype=torch.uint8, device=dev) for rb in rbs)
        for rows in (16, 256, 1000):
            image = tuple(torch.randint(0, 255, (L, R, H, rows, rb), dtype=torch.uint8, device=dev) for rb in rbs)
            hdr = (2 * B + 3) // 4 * 4
            stage = z(hdr + B * ld_u)
            stage[:2 * B] = torch.arange(B, device=dev, dtype=i32).repeat_interleave(2)          # job j: (j, j)
            state = z(R, NF)
            state[:, 0] = 12
            common = dict(jobs=stage, variates=stage[hdr:].view(torch.float32), klen=z(B),
                          e_klen0=torch.full((R,), rows, dtype=i32, device=dev),
                          state=z(B, NF), e_state=state, nf=NF, seq=z(B, ld_seq), ld_seq=ld_seq, chord_tok=z(B, ld_chord),
                          chord_pos=z(B, ld_chord), e_chord_tok=z(R, ld_chord), e_chord_pos=z(R, ld_chord), ld_chord=ld_chord,
                          wrong=z(B, 729, dtype=torch.uint8), ld_wrong=729, utable=z(B, ld_u, dtype=torch.float32), ld_u=ld_u,
                          seq_logp=z(B, ld_seq, 2, dtype=torch.float32), temperature_rows=z(B, dtype=torch.float32),
                          top_k_rows=z(B), top_p_rows=z(B, dtype=torch.float32), e_temperature=z(R, dtype=torch.float32),
                          e_top_k=z(R), e_top_p=z(R, dtype=torch.float32))
            old = ops.decode_arm_args(cache, image, e_seq=z(R, 16), ld_head=16, **common)
            new = ops.decode_arm_primed_args(cache, image, e_seq=z(R, 16 + PROMPT), ld_head=16 + PROMPT, **common)
            for n in (1, 16, 64):
                t = {"old": [], "new": []}
                for _ in range(reps):
                    for k, fn, args in (("old", ops.decode_arm, old), ("new", ops.decode_arm_primed, new)):
                        e0, e1 = ev(), ev()
                        e0.record()
                        fn(args, n)
                        e1.record()
                        torch.cuda.synchronize()
                        t[k].append(1e3 * e0.elapsed_time(e1))
                moved = 2 * n * L * H * rows * sum(rbs)
                r = {"what": "arm launch", "kv": kv, "rows": rows, "jobs": n, "MB_moved": round(moved / 1e6, 2)}
                for k in t:
                    us = t[k][4:]
                    r[k + "_us"] = spread(us, 1)
                    r[k + "_GB_per_s"] = round(moved / (statistics.median(us) * 1e-6) / 1e9, 1)
                    r[k + "_of_d2d"] = round(r[k + "_GB_per_s"] / d2d, 3)
                r["old_over_new"] = round(r["old_us"]["median"] / r["new_us"]["median"], 2)
                print(json.dumps(r), flush=True)
                out.append(r)
            del image, old, new


# ------------------------------------------------------------------------------------------------------------ end to end
def end(gen, G, n, reps, out):
    import numpy as np
    accept = lambda seq, rep: seq is not None
    no_eos = np.zeros(768, dtype=np.float32)          # (prompts of PROMPT tokens: no EOS, and few bars -- the rules end a
    no_eos[1] = -np.inf                               #  sequence after num_measures of them)
    no_eos[2] = -4.0
    plain = requests(G, n, 1, logit_bias=no_eos, accept=accept)
    own = gen.generate_pool(plain, slots=256)
    n_ctx = 1 + len(META)
    reqs = []
    for r, res in zip(requests(G, n, 3, accept=accept), own):
        import dataclasses
        body = res.sequences[0][n_ctx:]
        if body and body[-1] == 1:          # (an EOS the rules forced)
            body = body[:-1]
        reqs.append(dataclasses.replace(r, prompt=body[:PROMPT]))
    plen = [len(r.prompt) for r in reqs]

    def sequential():
        return [gen.generate_stream(r.encoded_meta, r.input_data, r.temperature, r.top_k, r.need, accept, seed=r.seed,
                                    prompt=list(r.prompt))[0] for r in reqs]
    legs = {"sequential": sequential,
            "pool64": lambda: [r.sequences for r in gen.generate_pool(reqs, slots=64)],
            "pool256": lambda: [r.sequences for r in gen.generate_pool(reqs, slots=256)]}
    toks = lambda seqs: sum(len(s) - n_ctx - len(r.prompt) for r, ss in zip(reqs, seqs) for s in ss)
    got = {k: fn() for k, fn in legs.items()}          # warm-up: decoders, graphs
    same = {k: got[k] == got["sequential"] for k in ("pool64", "pool256")}
    secs, tk = {k: [] for k in legs}, {}
    for _ in range(reps):
        for k, fn in legs.items():
            t, seqs = wall(fn)
            secs[k].append(t)
            tk[k] = toks(seqs)
    r = {"what": f"{n} requests of need 3, each with its own prompt", "prompt_tokens": spread(plen, 0), "tokens": tk,
         "pool_equals_sequential": same,
         "pool_stats_256": {k: (v if k != "arms" else len(v)) for k, v in gen.pool_stats.items()}}
    for k in legs:
        r[k] = {"seconds": spread(secs[k]), "tokens_per_s": round(tk[k] / statistics.median(secs[k]), 1)}
    for k in ("pool64", "pool256"):
        r[k + "_over_sequential"] = round(r[k]["tokens_per_s"] / r["sequential"]["tokens_per_s"], 2)
    print(json.dumps(r), flush=True)
    out.append(r)


def unprimed(gen, G, n, reps, out, tree):
    reqs = requests(G, n, 3)
    n_ctx = 1 + len(META)
    legs = {"pool64": lambda: [r.sequences for r in gen.generate_pool(reqs, slots=64)],
            "pool256": lambda: [r.sequences for r in gen.generate_pool(reqs, slots=256)]}
    for fn in legs.values():
        fn()
    secs, tk = {k: [] for k in legs}, {}
    for _ in range(reps):
        for k, fn in legs.items():
            t, seqs = wall(fn)
            secs[k].append(t)
            tk[k] = sum(len(s) - n_ctx for ss in seqs for s in ss)
    r = {"what": f"{n} unprimed requests of need 3", "tree": tree, "tokens": tk, "kernel": gen.pool_stats.get("kernel")}
    for k in legs:
        r[k] = {"seconds": spread(secs[k]), "runs": [round(t, 4) for t in secs[k]],
                "tokens_per_s": round(tk[k] / statistics.median(secs[k]), 1)}
    print(json.dumps(r), flush=True)
    out.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("legs", nargs="*", default=["arm", "end", "unprimed"])
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", type=str, default=ROOT)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "commu-code_amd"))
    import torch
    import commu_amd.generate as G
    dev = torch.device("cuda")
    rows = []
    with torch.no_grad():
        if "arm" in a.legs:
            arm(rows)
        if "end" in a.legs or "unprimed" in a.legs:
            model = build(dev)
            gen = G.BatchedGenerator(model, dev, generation_length=GLEN, memory_length=4146)
            if "end" in a.legs:
                end(gen, G, a.requests, a.reps, rows)
            if "unprimed" in a.legs:
                unprimed(gen, G, a.requests, a.reps, rows, os.path.abspath(a.tree))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
