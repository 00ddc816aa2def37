"""Shared builders of the request-pool tests (tests/test_pool_host.py, tests/test_pool_gpu.py): the arm launch's
operands with sentinels in every byte, its expected result in numpy, and the requests of the end-to-end tests."""
import types

import numpy as np

NAN_BYTE = 0x7F          # (kv8_contract.NAN_BYTE: what rows that must never be read hold)
NF = 14                  # commu_forcing_state_ints()
CTX_ROWS = 16
# slot array -> (store twin, row shape, dtype, sentinel); None twin: written without one
REQUIRED = {"state": ("e_state", (NF,), np.int32), "seq": ("e_seq", None, np.int32),
            "chord_tok": ("e_chord_tok", None, np.int32), "chord_pos": ("e_chord_pos", None, np.int32)}
OPTIONAL = {"temperature_rows": ("e_temperature", (), np.float32), "top_k_rows": ("e_top_k", (), np.int32),
            "top_p_rows": ("e_top_p", (), np.float32), "bias": ("e_bias", (768,), np.float32),
            "gram_on": ("e_gram_on", (), np.uint8), "harm_on": ("e_harm_on", (), np.uint8),
            "order_ctl": ("e_order", (), np.int32), "voice_ctl": ("e_voice", (), np.int32),
            "cls_ctl": ("e_cls", (32,), np.int32)}


def arm_case(torch, kv, DH, B=5, Lmax=24, R=3, klen0=(1, 11, 16), L=2, H=3, ld_u=9, ld_seq=40, ld_chord=6, ld_trace=8,
             optional=True, seed=0, dev="cuda"):
    """Slot arrays and caches full of sentinels, a store of R random entries, the staging block and the launch's
    argument block.  kv: "bf16" (K, V) or "fp8" (K, V bytes and their scale bytes)."""
    from commu_amd import ops
    rng = np.random.RandomState(seed)
    rows = [DH * 2, DH * 2] if kv == "bf16" else [DH, DH, DH // 32, DH // 32]

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def cache_like(n_slots, n_rows, fill):
        out = []
        for rb in rows:
            a = np.full((L, n_slots, H, n_rows, rb), fill, dtype=np.uint8) if fill is not None else \
                rng.randint(0, 256, (L, n_slots, H, n_rows, rb)).astype(np.uint8)
            if kv == "bf16":
                out.append(t(a).view(torch.bfloat16))
            else:
                out.append(t(a))
        return tuple(out)
    c = types.SimpleNamespace(B=B, R=R, L=L, H=H, Lmax=Lmax, ld_u=ld_u, ld_seq=ld_seq, ld_chord=ld_chord, ld_trace=ld_trace,
                              kv=kv, rows=rows, klen0=list(klen0))
    c.cache = cache_like(B, Lmax, NAN_BYTE)
    c.image = cache_like(R, CTX_ROWS, None)
    sent_i, sent_f, sent_b = -777, 123.0, 0xAB
    sent = {np.int32: sent_i, np.float32: sent_f, np.uint8: sent_b}
    widths = {"seq": (ld_seq, CTX_ROWS), "chord_tok": (ld_chord, ld_chord), "chord_pos": (ld_chord, ld_chord)}
    c.slot, c.store = {}, {}
    for name, (twin, shape, dt) in list(REQUIRED.items()) + (list(OPTIONAL.items()) if optional else []):
        if shape is not None:
            s_shape = e_shape = shape
        else:
            s_shape, e_shape = (widths[name][0],), (widths[name][1],)
        c.slot[name] = t(np.full((B,) + s_shape, sent[dt], dtype=dt))
        if dt == np.float32:
            c.store[twin] = t(rng.random_sample((R,) + e_shape).astype(dt))
        else:
            c.store[twin] = t(rng.randint(0, 200, (R,) + e_shape).astype(dt))
    c.store["e_klen0"] = t(np.array(klen0, dtype=np.int32))
    c.slot["klen"] = t(np.full(B, sent_i, dtype=np.int32))
    c.slot["wrong"] = t(np.full((B, 729), sent_b, dtype=np.uint8))
    c.slot["utable"] = t(np.full((B, ld_u), sent_f, dtype=np.float32))
    if optional:
        c.slot["seq_logp"] = t(np.full((B, ld_seq, 2), sent_f, dtype=np.float32))
        c.slot["trace"] = t(np.full((B, ld_trace), sent_i, dtype=np.int32))
    c.hdr = (2 * B + 3) // 4 * 4
    c.stage = t(np.zeros(c.hdr + B * ld_u, dtype=np.int32))
    fields = dict(c.slot)
    fields.update(c.store)
    c.args = ops.decode_arm_args(c.cache, c.image, jobs=c.stage, variates=c.stage[c.hdr:].view(torch.float32), nf=NF,
                                 ld_seq=ld_seq, ld_head=CTX_ROWS, ld_chord=ld_chord, ld_wrong=729, ld_u=ld_u,
                                 ld_trace=ld_trace if optional else 0, ld_bias=768 if optional else 0, **fields)
    return c


def snapshot(c):
    """Every slot array and cache as numpy (caches as bytes)."""
    import torch
    out = {k: v.cpu().numpy().copy() for k, v in c.slot.items()}
    for i, t in enumerate(c.cache):
        out[f"cache{i}"] = t.view(torch.uint8).cpu().numpy().copy()
    return out


def stage_jobs(c, jobs, variates):
    """jobs [(slot, entry)] and their variates rows into the staging block."""
    import torch
    host = np.zeros(c.stage.numel(), dtype=np.int32)
    host[:2 * len(jobs)] = np.array(jobs, dtype=np.int32).reshape(-1)
    host[c.hdr:c.hdr + len(jobs) * c.ld_u] = np.asarray(variates, dtype=np.float32).reshape(-1).view(np.int32)
    c.stage.copy_(torch.from_numpy(host))


def arm_expected(c, before, jobs, variates):
    """What the launch must leave, from the snapshot before it: jobs outside the ranges are skipped."""
    import torch
    exp = {k: v.copy() for k, v in before.items()}
    store = {k: v.cpu().numpy() for k, v in c.store.items()}
    images = [t.view(torch.uint8).cpu().numpy() for t in c.image]
    for j, (s, e) in enumerate(jobs):
        if not (0 <= s < c.B and 0 <= e < c.R):
            continue
        n = min(max(int(store["e_klen0"][e]), 0), min(CTX_ROWS, c.Lmax))
        for i, im in enumerate(images):
            exp[f"cache{i}"][:, s, :, :n] = im[:, e, :, :n]
        exp["klen"][s] = n
        exp["state"][s] = store["e_state"][e]
        exp["seq"][s, :CTX_ROWS] = store["e_seq"][e]
        exp["chord_tok"][s] = store["e_chord_tok"][e]
        exp["chord_pos"][s] = store["e_chord_pos"][e]
        exp["wrong"][s] = 0
        exp["utable"][s] = np.asarray(variates, dtype=np.float32)[j]
        if "seq_logp" in exp:
            exp["seq_logp"][s] = np.nan
            exp["trace"][s] = 0
        for name, (twin, _, _) in OPTIONAL.items():
            if name in exp:
                exp[name][s] = store[twin][e]
    return exp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- end-to-end requests
META = [574, 623, 627, 635, 639, 642, 651, 684, 694, 720, 727]


def data(chords=(), positions=(), num_measures=4.0):
    return types.SimpleNamespace(num_measures=float(num_measures),
                                 chord_token_components={"chord_token": list(chords), "chord_position": list(positions)})


def hash_accept(mod, rem):
    """A deterministic accept rule: rejects the sequences whose token sum is rem modulo mod (and failed ones)."""
    def accept(seq, report):
        return seq is not None and sum(seq) % mod != rem
    return accept


def four_requests(G):
    """Four requests that differ in last meta token, chord rows and num_measures, sampling triple, need and seed; one
    with a pitch range; each with its own accept rule and a bound on its attempts (an accept rule that a request's
    sequences never pass must end the request, not keep the loop turning: the last request's sequences all have an odd
    token sum on the test model, so it exhausts its 12 attempts and returns nothing -- in the pool and alone)."""
    pitch = G.token_constraints(pitch_range=(48, 84))
    specs = [
        dict(last=727, d=data(), need=1, t=0.95, k=32, p=1.0, seed=3, acc=hash_accept(2, 0), bias=None),
        dict(last=726, d=data([199, 285, 267, 258], [432] * 4, 4.0), need=3, t=1.05, k=24, p=0.95, seed=11,
             acc=hash_accept(3, 1), bias=None),
        dict(last=725, d=data([200, 201, 202, 203, 204, 205, 206, 207], [432] * 8, 8.0), need=2, t=0.9, k=40, p=1.0, seed=23,
             acc=hash_accept(3, 0), bias=pitch),
        dict(last=724, d=data([258, 199], [432] * 2, 4.0), need=2, t=0.95, k=32, p=0.9, seed=5, acc=hash_accept(2, 1),
             bias=None),
    ]
    return [G.PoolRequest(META[:-1] + [s["last"]], s["d"], s["need"], s["t"], s["k"], top_p=s["p"], seed=s["seed"],
                          max_attempts=12, accept=s["acc"], logit_bias=s["bias"]) for s in specs]
