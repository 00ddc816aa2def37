"""What the shared prompt prefix (ForcedDecoder(shared_prompt=True), csrc/decode_prefix.hip) does to the decode iteration:
the bench model (L6 D512 H8), 64 slots, graph replay, the unshared and the shared decoder INTERLEAVED in one process, REPS
repeats of ITERS iterations each, every configuration measured twice (A/A: the spread between two decoders of one kind).

  --mode shared   P ~ 1000: a real prompt (a free run's own tokens, so the rules accept it) through load(prompts=): load()
                  time, cache_bytes(), ms per iteration early (short suffix) and after 1000 generated tokens.
                  P ~ 3900: the prefix of a decoder built for it (max_prompt 1940: Pcap 3912, which leaves 312 private
                  rows below the 4224 positions of the distance table) filled by prefill_shared / prefill directly, early
                  only.  (A prompt of 3900 tokens itself cannot be loaded: Pcap = 32 + 2 max_prompt.)
  --mode default  the rows of the default decoder (no prompt, nothing of this feature on their path): ms per iteration at
                  11 and 1000 keys and 64 sequences of 4096 iterations to completion -- run it from two checkouts in turn
                  (--pkg DIR: the commu-code_amd directory to import) to compare a commit with its parent.

JSON lines.    python tests/probes/prefix_decode.py --mode shared|default [--pkg DIR] [--out FILE]
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
REPS, ITERS, WARM = 3, 64, 16
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


def build(dev, mem=4146):
    import torch
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.train import build_model
    cfg = get_cfg(num_layers=L, num_heads=H, units=D, inner_size=DI, tgt_length=1, mem_length=mem, dropout=0.0,
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


def uniforms(dec, seed=5):
    import torch
    return torch.rand(dec.B, dec.ld_u, generator=torch.Generator().manual_seed(seed)).numpy()


def timed(decs, reps=REPS, iters=ITERS):
    """Interleaved: {name: [ms per iteration of every repeat]}."""
    import torch
    times = {k: [] for k in decs}
    for _ in range(reps):
        for k, dec in decs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.run_iterations(iters, True)          # (64 live slots: the plain graph)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / iters)
    return times


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def free_run_prompt(model, n, dev):
    """n tokens that the loop itself produced after the conditioning tokens (one slot, sampled)."""
    import torch
    from commu_amd.generate import ForcedDecoder
    dec = ForcedDecoder(model, 1, n, 4146, 0.95, 32)
    dec.load([META], [data()], uniforms(dec, 11))
    dec.run()
    seq = dec.sequences()[0][0]
    return seq[1 + len(META):1 + len(META) + n]


def shared_rows(dev, out):
    import torch
    from commu_amd._lib import CommuHipError
    from commu_amd.generate import ForcedDecoder
    model = build(dev)
    prompt = free_run_prompt(model, 1000, dev)
    kinds = ("unshared_a", "shared_a", "unshared_b", "shared_b")
    # ---- P ~ 1000 through load()
    GL = 1000 + WARM + 2 * REPS * ITERS + 64
    decs, loads = {}, {}
    for k in kinds:
        dec = ForcedDecoder(model, B, GL, 4146, 0.95, 32, max_prompt=len(prompt),
                            **({"shared_prompt": True} if k.startswith("shared") else {}))
        uni = uniforms(dec)
        ts = []
        for _ in range(3):                     # (the first load also pays the lazy allocations: report the later ones)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                dec.load([META] * B, [data()] * B, uni, prompts=[prompt] * B)
            except CommuHipError as e:         # (a draw the free run rejected leaves no mark: the replay may refuse it)
                print(json.dumps({"what": "load refused", "why": str(e)}), flush=True)
                raise
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        decs[k], loads[k] = dec, ts
    P = decs["shared_a"].prefix_P
    r = {"what": "load(prompts=) of 64 slots", "prompt_tokens": len(prompt), "P": P}
    for k in kinds:
        r[k] = {"first_ms": round(loads[k][0], 2), "later_ms": [round(t, 2) for t in loads[k][1:]],
                "cache_bytes": decs[k].state.cache_bytes()}
    print(json.dumps(r), flush=True)
    out.append(r)
    for dec in decs.values():
        dec.pre()
        dec.run_iterations(WARM, True)
    for phase, skip in (("early", 0), ("after 1000 generated tokens", 1000 - WARM - REPS * ITERS)):
        for dec in decs.values():
            for _ in range(skip // 8):
                dec.run_iterations(8, True)
        torch.cuda.synchronize()
        private0 = int(decs["shared_a"].state.klen.max())
        times = timed(decs)
        r = {"what": f"P {P}, {phase}", "slots": B, "private_rows_start": private0,
             "private_rows_end": int(decs["shared_a"].state.klen.max()),
             "keys_unshared_end": int(decs["unshared_a"].state.klen.max())}
        for k in kinds:
            r[k] = stats(times[k])
        r["shared_over_unshared"] = round(min(r["shared_a"]["median_ms"], r["shared_b"]["median_ms"])
                                          / min(r["unshared_a"]["median_ms"], r["unshared_b"]["median_ms"]), 4)
        r["aa_spread"] = round(max(abs(r[a + "_a"]["median_ms"] / r[a + "_b"]["median_ms"] - 1) for a in ("shared", "unshared")), 4)
        print(json.dumps(r), flush=True)
        out.append(r)
    for dec in decs.values():
        dec.state.check()
        assert not bool(dec.fsm[:, 5].any()), "a probe sequence finished early"
    del decs
    torch.cuda.empty_cache()
    # ---- P ~ 3900: the prefix filled directly
    P = 3900
    GL = WARM + REPS * ITERS + 64
    col = torch.randint(3, 729, (P,), generator=torch.Generator().manual_seed(3))
    col[0] = 0
    col[1:11] = torch.tensor(META[:10])
    decs = {}
    for k in kinds:
        shared = k.startswith("shared")
        dec = ForcedDecoder(model, B, GL, 4146, 0.95, 32, max_prompt=1940, **({"shared_prompt": True} if shared else {}))
        dec.load([META] * B, [data()] * B, uniforms(dec))
        for t in dec.state.cache_tensors():
            t.zero_()
        if shared:
            dec.state.prefill_shared(col.to(dev))
        else:
            dec.state.prefill(col[:, None].expand(P, B).contiguous().to(dev))
        decs[k] = dec
    for dec in decs.values():
        dec.pre()
        dec.run_iterations(WARM, True)
    times = timed(decs)
    r = {"what": f"P {P}, early (prefix filled directly)", "slots": B,
         "private_rows_end": int(decs["shared_a"].state.klen.max()), "keys_unshared_end": int(decs["unshared_a"].state.klen.max())}
    for k in kinds:
        r[k] = dict(stats(times[k]), cache_bytes=decs[k].state.cache_bytes())
    r["shared_over_unshared"] = round(min(r["shared_a"]["median_ms"], r["shared_b"]["median_ms"])
                                      / min(r["unshared_a"]["median_ms"], r["unshared_b"]["median_ms"]), 4)
    r["aa_spread"] = round(max(abs(r[a + "_a"]["median_ms"] / r[a + "_b"]["median_ms"] - 1) for a in ("shared", "unshared")), 4)
    print(json.dumps(r), flush=True)
    out.append(r)


def default_rows(dev, out, tag):
    import torch
    from commu_amd.generate import ForcedDecoder
    model = build(dev)
    for klen0 in (11, 1000):
        dec = ForcedDecoder(model, B, WARM + REPS * ITERS + 64, 4146, 0.95, 32)
        dec.load([META] * B, [data()] * B, uniforms(dec))
        if klen0 > 11:
            ctx = torch.randint(3, 729, (klen0, B), generator=torch.Generator().manual_seed(3))
            ctx[0] = 0
            ctx[1:11] = torch.tensor(META[:10])[:, None]
            dec.state.prefill(ctx.to(dev))
        dec.pre()
        dec.run_iterations(WARM, True)
        times = timed({"t": dec})
        r = dict({"what": f"default decoder, {klen0} keys", "tree": tag}, **stats(times["t"]))
        print(json.dumps(r), flush=True)
        out.append(r)
    dec = ForcedDecoder(model, B, 4096, 4146, 0.95, 32)
    ts = []
    for _ in range(2):
        dec.load([META] * B, [data()] * B, uniforms(dec))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.run()
        ts.append(time.perf_counter() - t0)
    ntok = sum(len(s) - 12 for s in dec.sequences()[0])
    r = {"what": "default decoder, 64 sequences to completion", "tree": tag, "seconds": [round(t, 4) for t in ts],
         "tokens": ntok, "tokens_per_s": round(ntok / min(ts), 1)}
    print(json.dumps(r), flush=True)
    out.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["shared", "default"], default="shared")
    ap.add_argument("--pkg", type=str, default=os.path.join(ROOT, "commu-code_amd"))
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    dev = torch.device("cuda")
    rows = []
    with torch.no_grad():
        if a.mode == "shared":
            shared_rows(dev, rows)
        else:
            default_rows(dev, rows, os.path.abspath(a.pkg))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
