"""What priming a decode batch costs: L6 D512, 64 slots, 1000-token contexts.
(i) DecodeState.prefill_ragged (one commu_decode_prefill_scatter launch per layer) with equal lengths against prefill()
    (2 L strided torch copies) on the same context: the whole call (forward + cache fill) and the cache fill alone
    (whole call minus a forward-only call), interleaved, REPS repeats each, linear cache and a ring of 512;
(ii) commu_forcing_replay for a 1000-token prompt in 64 slots (a serial lane-0 loop, once per request).
JSON lines; the median and the spread of every row.

    python tests/probes/prime_prefill.py [--parity] [--out FILE]
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

from commu_amd._lib import call  # noqa: E402
from commu_amd.generate import DecodeState, ForcedDecoder, _p, _s  # noqa: E402
from commu_amd.model.config_helper import get_cfg  # noqa: E402
from commu_amd.model.dataset import BaseVocab  # noqa: E402
from commu_amd.train import build_model  # noqa: E402

B, L, H, D, DI, T = 64, 6, 8, 512, 1024, 1000
REPS = 3
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


def ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def row(name, ts, **kw):
    r = {"what": name, "median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
    r.update(kw)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rows = []
    g = torch.Generator().manual_seed(1)
    ctx = torch.randint(304, 729, (T, B), generator=g).to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    for window in (None, 512):
        mem = 4146 if window is None else window
        cfg = get_cfg(num_layers=L, num_heads=H, units=D, inner_size=DI, tgt_length=1, mem_length=mem, dropout=0.0,
                      attention_dropout=0.0, same_length=True)
        model = build_model(cfg, BaseVocab(), dev, seed=1).eval()
        model.parity_fp32 = bool(a.parity)
        with torch.no_grad():
            st = DecodeState(model, B, mem + 1 if window is None else window + 1, window=window)

            def forward_only():
                if st.parity:
                    model._run_forward_f32(ctx, None, want_kv=True)
                else:
                    model._run_forward(ctx, None, None, None, need_grad=False, want_logits=True, want_kv=True)
            calls = {"prefill": lambda: st.prefill(ctx), "prefill_ragged": lambda: st.prefill_ragged(ctx, lens),
                     "forward_only": forward_only}
            for fn in calls.values():          # warm-up: allocator pools, lazy module state
                fn()
            times = {k: [] for k in calls}
            for _ in range(REPS):              # interleaved
                for k, fn in calls.items():
                    times[k].append(ms(fn))
        tag = {"cache": "linear" if window is None else f"ring{window}", "dtype": "f32" if a.parity else "bf16"}
        for k in calls:
            rows.append(row(k, times[k], **tag))
        fwd = statistics.median(times["forward_only"])
        for k in ("prefill", "prefill_ragged"):
            rows.append(row(k + " minus forward", [t - fwd for t in times[k]], **tag))
        del st, model
        torch.cuda.empty_cache()
    # (ii) the replay kernel alone: 64 slots, one 1000-token prompt each (notes only: every token is a draw that is appended)
    cfg = get_cfg(num_layers=2, num_heads=2, units=128, inner_size=256, tgt_length=1, mem_length=4146, dropout=0.0,
                  attention_dropout=0.0, same_length=True)
    model = build_model(cfg, BaseVocab(), dev, seed=1).eval()
    data = types.SimpleNamespace(num_measures=4.0, chord_token_components={"chord_token": [], "chord_position": []})
    prompts = np.random.RandomState(2).randint(304, 729, size=(B, T)).tolist()
    with torch.no_grad():
        dec = ForcedDecoder(model, B, 64, 4146, 0.95, 32, max_prompt=T)
        ts, ts_load = [], []
        for _ in range(REPS + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            dec.load([META] * B, [data] * B, prompts=prompts)
            torch.cuda.synchronize()
            ts_load.append(1e3 * (time.perf_counter() - t0))
            # the kernel alone: the same launch again on freshly loaded records
            dec.load([META] * B, [data] * B)
            dec.prompt.copy_(torch.tensor(prompts, dtype=torch.int32))
            dec.prompt_len.fill_(T)
            dec.state.klen.fill_(len(META))
            ev0.record()
            call("commu_forcing_replay", _p(dec.fsm), _p(dec.seq), dec.ld_seq, _p(dec.prompt), dec.max_prompt,
                 _p(dec.prompt_len), _p(dec.chord_tok), _p(dec.chord_pos), dec.ld_chord, _p(dec.wrong), _p(dec.utable),
                 dec.ld_u, _p(dec.tok), _p(dec.active), _p(dec.keep), _p(dec.draw), _p(dec.uni), _p(dec.trace),
                 dec.ld_trace, _p(dec.seq_logp), _p(dec.state.klen), _p(dec.fed), dec.ld_fed, _p(dec.diverged), B, _s())
            ev1.record()
            torch.cuda.synchronize()
            ts.append(ev0.elapsed_time(ev1))
            assert int(dec.diverged.max()) == -1 and int(dec.state.klen.min()) == len(META) + T - 1
    rows.append(row("commu_forcing_replay, 64 slots x 1000 tokens", ts[1:]))
    rows.append(row("ForcedDecoder.load(prompts=) whole call, L2 D128 model", ts_load[1:]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
