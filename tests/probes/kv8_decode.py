"""What the fp8 K/V cache (ForcedDecoder(kv_dtype="fp8"), csrc/decode_kv8.hip) does to the decode iteration: the bench
model (L6 D512 H8), 64 slots, graph replay, bf16 and fp8 caches INTERLEAVED, REPS repeats of ITERS iterations each, after a
real prefill (bench.py's long_memory recipe):

  * linear cache at klen ~ 11, 1000 and 3900 (the "4000" row: 3900 + the iterations stay inside the 4147 rows);
  * a ring of 2048 rows (sliding memory of 2047, full);
  * 8 live sequences at klen ~ 3900 with the split-key graph (attn_splits = 4).

JSON lines: ms per iteration, median and spread of every row, and the cache bytes of both modes.

    python tests/probes/kv8_decode.py [--out FILE]
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
import torch  # noqa: E402

from commu_amd.generate import ForcedDecoder  # noqa: E402
from commu_amd.model.config_helper import get_cfg  # noqa: E402
from commu_amd.model.dataset import BaseVocab  # noqa: E402
from commu_amd.train import build_model  # noqa: E402

L, H, D, DI = 6, 8, 512, 1024
REPS, ITERS, WARM = 3, 64, 16
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


def build(mem, dev):
    cfg = get_cfg(num_layers=L, num_heads=H, units=D, inner_size=DI, tgt_length=1, mem_length=mem, dropout=0.0,
                  attention_dropout=0.0, same_length=True)
    model = build_model(cfg, BaseVocab(), dev, seed=1).eval()
    with torch.no_grad():
        bias = model.crit.out_layers[0].bias
        bias.zero_()
        bias[1:3] = -1e9                      # no EOS / BAR, no chord tokens: every iteration is a model step and a draw
        bias[195:304] = -1e9
    return model


def decoder(model, B, kv, klen0, ring, dev):
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
    dec = ForcedDecoder(model, B, generation_length=WARM + REPS * ITERS + 64, memory_length=ring - 1 if ring else 4146,
                        temperature=0.95, top_k=32, sliding=bool(ring), kv_dtype=kv)
    uni = torch.rand(B, dec.ld_u, generator=torch.Generator().manual_seed(5)).numpy()
    dec.load([META] * B, [data] * B, uni)
    if klen0 > 11:
        g = torch.Generator().manual_seed(3)
        ctx = torch.randint(3, 729, (klen0, B), generator=g)
        ctx[0] = 0
        ctx[1:11] = torch.tensor(META[:10])[:, None]
        for t in dec.state.cache_tensors():
            t.zero_()
        dec.state.prefill(ctx.to(dev))
    return dec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rows = []
    #        name                      B   klen0  ring  live_rows (None: the plain graph)
    cases = [("linear klen 11", 64, 11, 0, None), ("linear klen 1000", 64, 1000, 0, None),
             ("linear klen 3900", 64, 3900, 0, None), ("ring 2048 (full)", 64, 2600, 2048, None),
             ("linear klen 3900, 8 live, 4 splits", 8, 3900, 0, 8)]
    with torch.no_grad():
        for name, B, klen0, ring, live in cases:
            model = build(ring - 1 if ring else 4146, dev)
            decs = {kv: decoder(model, B, kv, klen0, ring, dev) for kv in ("bf16", "fp8")}
            done = {kv: 0 for kv in decs}

            def run(kv, n):
                dec = decs[kv]
                dec.run_iterations(n, True, klen_bound=klen0 + done[kv] + n, live_rows=live)
                done[kv] += n
            for kv, dec in decs.items():
                dec.pre()
                run(kv, WARM)
            torch.cuda.synchronize()
            times = {kv: [] for kv in decs}
            for _ in range(REPS):              # interleaved
                for kv in decs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(kv, ITERS)
                    torch.cuda.synchronize()
                    times[kv].append(1e3 * (time.perf_counter() - t0) / ITERS)
            for kv, dec in decs.items():
                dec.state.check()
                assert not bool(dec.fsm[:, 5].any()), "a probe sequence finished early"
                assert (dec.graph_long if live else dec.graph) is not None
            r = {"what": name, "slots": B, "klen_start": klen0 + WARM, "klen_end": int(decs["fp8"].state.klen.max()),
                 "splits": decs["fp8"].LONG_SPLITS if live else 1}
            for kv in decs:
                ts = times[kv]
                r[kv] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                         "cache_bytes": decs[kv].state.cache_bytes()}
            r["fp8_over_bf16_time"] = round(r["fp8"]["median_ms"] / r["bf16"]["median_ms"], 4)
            r["fp8_over_bf16_bytes"] = round(r["fp8"]["cache_bytes"] / r["bf16"]["cache_bytes"], 4)
            print(json.dumps(r), flush=True)
            rows.append(r)
            del decs, model
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
