"""What a constraint row per slot (ForcedDecoder.set_logit_bias, commu_decode_loop_args.bias) costs per decode
iteration: the bench model (L6 D512 H8), 64 slots at ~11 keys -- where the sampling stage is the largest share of the
iteration --, graph replay, three decoders INTERLEAVED, REPS repeats of ITERS iterations each:

  * null   -- never given a constraint: the launch without the bias pointer (what every decoder ran before);
  * zeros  -- the bias buffer allocated and all zeros: the 3 KB per slot are loaded, nothing changes;
  * rows   -- a pitch range, banned chord tokens and a finite re-weighting in every slot.

Also the stand-alone sampling kernel (commu_sample_topk with commu_sample_args.bias, 64 rows) with and without the rows, by
HIP events.  JSON lines: ms per iteration / us per launch, median and spread.

    python tests/probes/sample_bias.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "commu-code_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from commu_amd import ops  # noqa: E402
from commu_amd.generate import ForcedDecoder, token_constraints  # noqa: E402
from commu_amd.model.config_helper import get_cfg  # noqa: E402
from commu_amd.model.dataset import BaseVocab  # noqa: E402
from commu_amd.train import build_model  # noqa: E402

L, H, D, DI = 6, 8, 512, 1024
B = 64
REPS, ITERS, WARM = 7, 32, 16
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


def build(dev):
    cfg = get_cfg(num_layers=L, num_heads=H, units=D, inner_size=DI, tgt_length=1, mem_length=4146, dropout=0.0,
                  attention_dropout=0.0, same_length=True)
    model = build_model(cfg, BaseVocab(), dev, seed=1).eval()
    with torch.no_grad():
        bias = model.crit.out_layers[0].bias
        bias.zero_()
        bias[1:3] = -1e9                      # no EOS / BAR, no chord tokens: every iteration is a model step and a draw
        bias[195:304] = -1e9
    return model


def constraint_rows():
    g = np.random.RandomState(7)
    rows = []
    for b in range(B):
        lo = 36 + b % 12
        rows.append(token_constraints(ban=range(195, 304), pitch_range=(lo, lo + 36),
                                      bias={int(i): float(v) for i, v in zip(g.choice(np.arange(304, 729), 40, replace=False),
                                                                             g.uniform(-3, 3, 40))}))
    return np.stack(rows)


def decoder(model, mode):
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
    dec = ForcedDecoder(model, B, generation_length=WARM + REPS * ITERS + 64, memory_length=4146, temperature=0.95, top_k=32)
    if mode == "zeros":
        dec.set_logit_bias(np.zeros(768, np.float32))
    elif mode == "rows":
        dec.set_logit_bias(constraint_rows())
    uni = torch.rand(B, dec.ld_u, generator=torch.Generator().manual_seed(5)).numpy()
    dec.load([META] * B, [data] * B, uni)
    return dec


def spread(ts, digits=4):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = []
    with torch.no_grad():
        model = build(dev)
        decs = {m: decoder(model, m) for m in ("null", "zeros", "rows")}
        for dec in decs.values():
            dec.pre()
            dec.run_iterations(WARM, True)
        torch.cuda.synchronize()
        times = {m: [] for m in decs}
        for _ in range(REPS):                  # interleaved
            for m, dec in decs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.run_iterations(ITERS, True)
                torch.cuda.synchronize()
                times[m].append(1e3 * (time.perf_counter() - t0) / ITERS)
        for m, dec in decs.items():
            dec.state.check()
            assert not bool(dec.fsm[:, 5].any()), "a probe sequence finished early"
            assert (dec.bias is None) == (m == "null") and dec.graph is not None
        r = {"what": "decode iteration, graph replay", "slots": B, "klen_start": 11 + WARM,
             "klen_end": int(decs["null"].state.klen.max()), "ms_per_iteration": {m: spread(times[m]) for m in decs}}
        base = r["ms_per_iteration"]["null"]["median"]
        r["over_null"] = {m: round(r["ms_per_iteration"][m]["median"] / base, 4) for m in ("zeros", "rows")}
        r["us_added"] = {m: round(1e3 * (r["ms_per_iteration"][m]["median"] - base), 2) for m in ("zeros", "rows")}
        print(json.dumps(r), flush=True)
        out.append(r)
        # the sampling kernel alone: 64 rows, per-row controls as the loop passes them, 200 launches per repeat
        logits = torch.randn(B, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.5
        rows = torch.from_numpy(constraint_rows()).to(dev)
        t = torch.full((B,), 0.95, device=dev)
        k = torch.full((B,), 32, dtype=torch.int32, device=dev)
        p = torch.ones(B, device=dev)
        u = torch.rand(B, device=dev)
        tok = torch.zeros(B, dtype=torch.int32, device=dev)
        work = logits.clone()
        us = {"null": [], "rows": []}
        for rep in range(REPS + 1):
            for m, bias in (("null", None), ("rows", rows)):
                work.copy_(logits)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(200):
                    ops.sample_topk(work, t, k, uniforms=u, token=tok, top_p=p, bias=bias)
                e.record()
                torch.cuda.synchronize()
                if rep:
                    us[m].append(1e3 * s.elapsed_time(e) / 200)
        r = {"what": "sampling kernel alone, back-to-back launches", "rows": B,
             "us_per_launch": {m: spread(us[m], 3) for m in us}}
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
