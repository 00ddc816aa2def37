"""Shared builders of the primed request-pool tests (tests/test_pool_prime_host.py, tests/test_pool_prime_gpu.py): a numpy
restatement of the primed arm launch (commu_decode_arm_primed, include/commu_hip.h) -- the state of every cache tensor and
slot array after a launch, given the state before --, its operands with sentinels in every byte, and the helpers of the
end-to-end tests."""
import types

import numpy as np

import pool_contract as PC

NF = PC.NF


def arm_primed_expected(before, store, images, jobs, variates, B, R, Lmax, img_rows, ld_head, ring=False, grid_rows=0):
    """What the launch must leave.  before: {name: array} of the slot arrays ("klen", "state", "seq", "chord_tok",
    "chord_pos", "wrong", "utable", optional "seq_logp", "trace" and the optional controls of pool_contract.OPTIONAL) and
    "cache<i>" byte arrays [L, B, H, Lmax, row]; store: the e_* twins [R, .] (an optional "e_trace"); images: byte arrays
    [L, R, H, img_rows, row]; jobs [(slot, entry)], skipped outside [0, B) x [0, R); variates [njobs, ld_u].
    Rows: k = max(e_klen0, 0), n = min(k, img_rows, Lmax (, grid_rows)) rows of the image go to the slot's rows 0 .. n - 1,
    nothing else of a cache changes; klen = n on a linear cache and k, unclamped, on a ring.  The sequence head is
    the record's length word, clamped to [0, ld_head], many words; the trace is the entry's where the store has one."""
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
        m = min(max(int(store["e_state"][e][0]), 0), ld_head)
        exp["seq"][s, :m] = store["e_seq"][e, :m]
        exp["chord_tok"][s] = store["e_chord_tok"][e]
        exp["chord_pos"][s] = store["e_chord_pos"][e]
        exp["wrong"][s] = 0
        exp["utable"][s] = np.asarray(variates, dtype=np.float32)[j]
        if "seq_logp" in exp:
            exp["seq_logp"][s] = np.nan
        if "trace" in exp:
            exp["trace"][s] = store["e_trace"][e] if "e_trace" in store else 0
        for name, (twin, _, _) in PC.OPTIONAL.items():
            if name in exp:
                exp[name][s] = store[twin][e]
    return exp


def prime_case(torch, kv, DH, klen0, lens, B=5, Lmax=200, R=3, img_rows=144, L=2, H=3, ld_u=9, ld_seq=60, ld_head=48,
               ld_chord=6, ld_trace=8, optional=True, e_trace=True, ring=False, grid_rows=0, seed=0, dev="cuda"):
    """pool_contract.arm_case for the primed launch: caches full of NAN_BYTE, slot arrays full of sentinels, a store of R
    random entries with images of img_rows rows, e_klen0 = klen0 and the records' length words = lens."""
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
                              ld_chord=ld_chord, ld_trace=ld_trace, kv=kv, rows=rows, klen0=list(klen0), ring=ring,
                              grid_rows=grid_rows)
    c.cache = cache_like(B, Lmax, PC.NAN_BYTE)
    c.image = cache_like(R, img_rows, None)
    sent = {np.int32: -777, np.float32: 123.0, np.uint8: 0xAB}
    widths = {"seq": (ld_seq, ld_head), "chord_tok": (ld_chord, ld_chord), "chord_pos": (ld_chord, ld_chord)}
    c.slot, c.store = {}, {}
    for name, (twin, shape, dt) in list(PC.REQUIRED.items()) + (list(PC.OPTIONAL.items()) if optional else []):
        s_shape, e_shape = (shape, shape) if shape is not None else ((widths[name][0],), (widths[name][1],))
        c.slot[name] = t(np.full((B,) + s_shape, sent[dt], dtype=dt))
        if dt == np.float32:
            c.store[twin] = t(rng.random_sample((R,) + e_shape).astype(dt))
        else:
            c.store[twin] = t(rng.randint(0, 200, (R,) + e_shape).astype(dt))
    state = c.store["e_state"].cpu().numpy()
    state[:, 0] = np.array(lens, dtype=np.int32)
    c.store["e_state"] = t(state)
    c.store["e_klen0"] = t(np.array(klen0, dtype=np.int32))
    c.slot["klen"] = t(np.full(B, sent[np.int32], dtype=np.int32))
    c.slot["wrong"] = t(np.full((B, 729), sent[np.uint8], dtype=np.uint8))
    c.slot["utable"] = t(np.full((B, ld_u), sent[np.float32], dtype=np.float32))
    if optional:
        c.slot["seq_logp"] = t(np.full((B, ld_seq, 2), sent[np.float32], dtype=np.float32))
        c.slot["trace"] = t(np.full((B, ld_trace), sent[np.int32], dtype=np.int32))
        if e_trace:
            c.store["e_trace"] = t(rng.randint(0, 700, (R, ld_trace)).astype(np.int32))
    c.hdr = (2 * B + 3) // 4 * 4
    c.stage = t(np.zeros(c.hdr + B * ld_u, dtype=np.int32))
    fields = dict(c.slot)
    fields.update(c.store)
    c.args = ops.decode_arm_primed_args(c.cache, c.image, ring=ring, grid_rows=grid_rows, jobs=c.stage,
                                        variates=c.stage[c.hdr:].view(torch.float32), nf=NF, ld_seq=ld_seq, ld_head=ld_head,
                                        ld_chord=ld_chord, ld_wrong=729, ld_u=ld_u, ld_trace=ld_trace if optional else 0,
                                        ld_bias=768 if optional else 0, **fields)
    return c


def expected(c, before, jobs, variates):
    """arm_primed_expected for a prime_case."""
    import torch
    store = {k: v.cpu().numpy() for k, v in c.store.items()}
    images = [t.view(torch.uint8).cpu().numpy() for t in c.image]
    return arm_primed_expected(before, store, images, jobs, variates, c.B, c.R, c.Lmax, c.img_rows, c.ld_head, ring=c.ring,
                               grid_rows=c.grid_rows)


def prompt_of(seq, n_cond, k):
    """The first k tokens after [0] + meta of a sequence the model generated (fewer where it is shorter; its last token,
    EOS, never)."""
    body = list(seq[1 + n_cond:-1])
    return body[:k]
