"""Shared builders of the request-pool tests (tests/test_pool_host.py, tests/test_pool_gpu.py and their primed twins over
tests/pool_prime_contract.py): the ONE numpy restatement of both arm launches (commu_decode_arm, commu_decode_arm_primed,
include/commu_hip.h) -- the state of every cache tensor and slot array after a launch, given the state before --, the
launches' operands with sentinels in every byte, and the requests of the end-to-end tests."""
import types

import numpy as np

import form_contract as FC

NAN_BYTE = 0x7F          # (kv8_contract.NAN_BYTE: what rows that must never be read hold)
NF = 14                  # commu_forcing_state_ints()
CTX_ROWS = 16
BAR = 2                  # (prime_contract.BAR)
# slot array -> (store twin, row shape, dtype); a None shape: the widths of the case
REQUIRED = {"state": ("e_state", (NF,), np.int32), "seq": ("e_seq", None, np.int32),
            "chord_tok": ("e_chord_tok", None, np.int32), "chord_pos": ("e_chord_pos", None, np.int32)}
# every optional per-slot array the launches move from a store twin
OPTIONAL = {"temperature_rows": ("e_temperature", (), np.float32), "top_k_rows": ("e_top_k", (), np.int32),
            "top_p_rows": ("e_top_p", (), np.float32), "bias": ("e_bias", (768,), np.float32),
            "gram_on": ("e_gram_on", (), np.uint8), "harm_on": ("e_harm_on", (), np.uint8),
            "order_ctl": ("e_order", (), np.int32), "voice_ctl": ("e_voice", (), np.int32),
            "density_ctl": ("e_density", (), np.int32), "interval_ctl": ("e_interval", (), np.int32),
            "onset_ctl": ("e_onset", (), np.int32), "guide_ctl": ("e_guide", (), np.int32),
            "art_ctl": ("e_art", (), np.int32), "form_ctl": ("e_form", (), np.int32),
            "cls_ctl": ("e_cls", (32,), np.int32)}


def arm_restated(before, store, images, jobs, variates, B, R, Lmax, img_rows, ld_head, ring=False, grid_rows=0,
                 whole_head=False):
    """What either launch must leave.  before: {name: array} of the slot arrays ("klen", "state", "seq", "chord_tok",
    "chord_pos", "wrong", "utable", optional "seq_logp", "trace", "form_state", "form_tok" and the controls of OPTIONAL) and
    "cache<i>" byte arrays [L, B, H, Lmax, row]; store: the e_* twins [R, .] (an optional "e_trace"); images: byte arrays
    [L, R, H, img_rows, row]; jobs [(slot, entry)], skipped outside [0, B) x [0, R); variates [njobs, ld_u].
    Rows: k = max(e_klen0, 0), n = min(k, img_rows, Lmax (, grid_rows)) rows of the image go to the slot's rows 0 .. n - 1,
    nothing else of a cache changes; klen = n on a linear cache and k, unclamped, on a ring.  The sequence head is ld_head
    words (whole_head: the unprimed launch) or the record's length word, clamped to [0, ld_head], many (the primed one);
    the trace is the entry's where the store has one, zeros where not.  The form state is form_contract.initial_state over
    the entry's head up to the clamped length word -- in both launches --, and form_tok -1."""
    exp = {k: v.copy() for k, v in before.items()}
    cap = min(img_rows, Lmax)
    if grid_rows > 0:
        cap = min(cap, grid_rows)
    for j, (s, e) in enumerate(jobs):
        if not (0 <= s < B and 0 <= e < R):
            continue
        k = max(int(store["e_klen0"][e]), 0)
        n = min(k, cap)
        for i, im in enumerate(images):
            exp[f"cache{i}"][:, s, :, :n] = im[:, e, :, :n]
        exp["klen"][s] = k if ring else n
        exp["state"][s] = store["e_state"][e]
        length = min(max(int(store["e_state"][e][0]), 0), ld_head)
        m = ld_head if whole_head else length
        exp["seq"][s, :m] = store["e_seq"][e, :m]
        exp["chord_tok"][s] = store["e_chord_tok"][e]
        exp["chord_pos"][s] = store["e_chord_pos"][e]
        exp["wrong"][s] = 0
        exp["utable"][s] = np.asarray(variates, dtype=np.float32)[j]
        if "seq_logp" in exp:
            exp["seq_logp"][s] = np.nan
        if "trace" in exp:
            exp["trace"][s] = store["e_trace"][e] if "e_trace" in store else 0
        for name, (twin, _, _) in OPTIONAL.items():
            if name in exp:
                exp[name][s] = store[twin][e]
        if "form_tok" in exp:
            exp["form_tok"][s] = -1
        if "form_state" in exp:
            exp["form_state"][s] = FC.initial_state([int(x) for x in store["e_seq"][e]], length)
    return exp


def case(torch, kv, DH, klen0, lens, primed, B=5, Lmax=24, R=3, img_rows=CTX_ROWS, L=2, H=3, ld_u=9, ld_seq=40,
         ld_head=CTX_ROWS, ld_chord=6, ld_trace=8, optional=True, e_trace=False, ring=False, grid_rows=0, seed=0, dev="cuda"):
    """Slot arrays full of sentinels and caches full of NAN_BYTE, a store of R random entries with images of img_rows rows,
    e_klen0 = klen0 and the records' length words = lens, the staging block and the argument block of the launch (primed:
    commu_decode_arm_primed's).  kv: "bf16" (K, V) or "fp8" (K, V bytes and their scale bytes).  Every entry's sequence
    head gets Bar tokens planted: two below its length word (clamped to [0, ld_head]) and one at or beyond it, wherever the
    length leaves such positions, so that the form state's bar_at is neither empty nor every Bar of the row."""
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
            out.append(t(a).view(torch.bfloat16) if kv == "bf16" else t(a))
        return tuple(out)
    c = types.SimpleNamespace(B=B, R=R, L=L, H=H, Lmax=Lmax, img_rows=img_rows, ld_u=ld_u, ld_seq=ld_seq, ld_head=ld_head,
                              ld_chord=ld_chord, ld_trace=ld_trace, kv=kv, rows=rows, klen0=list(klen0), lens=list(lens),
                              primed=primed, ring=ring, grid_rows=grid_rows)
    c.cache = cache_like(B, Lmax, NAN_BYTE)
    c.image = cache_like(R, img_rows, None)
    sent = {np.int32: -777, np.float32: 123.0, np.uint8: 0xAB}
    widths = {"seq": (ld_seq, ld_head), "chord_tok": (ld_chord, ld_chord), "chord_pos": (ld_chord, ld_chord)}
    c.slot, store = {}, {}
    for name, (twin, shape, dt) in list(REQUIRED.items()) + (list(OPTIONAL.items()) if optional else []):
        s_shape, e_shape = (shape, shape) if shape is not None else ((widths[name][0],), (widths[name][1],))
        c.slot[name] = t(np.full((B,) + s_shape, sent[dt], dtype=dt))
        if dt == np.float32:
            store[twin] = rng.random_sample((R,) + e_shape).astype(dt)
        else:
            store[twin] = rng.randint(0, 200, (R,) + e_shape).astype(dt)
    store["e_state"][:, 0] = np.array(lens, dtype=np.int32)
    for e in range(R):
        m = min(max(int(lens[e]), 0), ld_head)
        if m > 0:
            store["e_seq"][e, rng.choice(m, size=min(2, m), replace=False)] = BAR
        if m < ld_head:
            store["e_seq"][e, rng.randint(m, ld_head)] = BAR
    store["e_klen0"] = np.array(klen0, dtype=np.int32)
    c.slot["klen"] = t(np.full(B, sent[np.int32], dtype=np.int32))
    c.slot["wrong"] = t(np.full((B, 729), sent[np.uint8], dtype=np.uint8))
    c.slot["utable"] = t(np.full((B, ld_u), sent[np.float32], dtype=np.float32))
    if optional:
        c.slot["seq_logp"] = t(np.full((B, ld_seq, 2), sent[np.float32], dtype=np.float32))
        c.slot["trace"] = t(np.full((B, ld_trace), sent[np.int32], dtype=np.int32))
        c.slot["form_state"] = t(np.full((B, FC.NS), sent[np.int32], dtype=np.int32))
        c.slot["form_tok"] = t(np.full(B, sent[np.int32], dtype=np.int32))
        if e_trace:
            store["e_trace"] = rng.randint(0, 700, (R, ld_trace)).astype(np.int32)
    c.store = {k: t(v) for k, v in store.items()}
    c.hdr = (2 * B + 3) // 4 * 4
    c.stage = t(np.zeros(c.hdr + B * ld_u, dtype=np.int32))
    build = ops.decode_arm_args if not primed else (
        lambda *a, **kw: ops.decode_arm_primed_args(*a, ring=ring, grid_rows=grid_rows, **kw))
    c.args = build(c.cache, c.image, jobs=c.stage, variates=c.stage[c.hdr:].view(torch.float32), nf=NF, ld_seq=ld_seq,
                   ld_head=ld_head, ld_chord=ld_chord, ld_wrong=729, ld_u=ld_u, ld_trace=ld_trace if optional else 0,
                   ld_bias=768 if optional else 0, **c.slot, **c.store)
    return c


def arm_case(torch, kv, DH, B=5, Lmax=24, R=3, klen0=(1, 11, 16), lens=(9, 16, 12), **kw):
    """case() for commu_decode_arm: images of CTX_ROWS rows, sequence heads of CTX_ROWS words.  lens: the records' length
    words; the default leaves two entries room for Bars on both sides of it and gives one the whole head."""
    return case(torch, kv, DH, klen0, lens, False, B=B, Lmax=Lmax, R=R, **kw)


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
    """What the launch of a case (either launch's) must leave, from the snapshot before it: arm_restated on its operands."""
    import torch
    store = {k: v.cpu().numpy() for k, v in c.store.items()}
    images = [t.view(torch.uint8).cpu().numpy() for t in c.image]
    return arm_restated(before, store, images, jobs, variates, c.B, c.R, c.Lmax, c.img_rows, c.ld_head, ring=c.ring,
                        grid_rows=c.grid_rows, whole_head=not c.primed)


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
