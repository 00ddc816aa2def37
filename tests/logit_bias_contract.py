"""The sampling step with a constraint row, restated in plain numpy (no GPU, no package code): what
commu_sample_topk computes for ONE sequence with a bias row, in the documented order

    x = raw / temperature (fp32, written back; the raw row for temperature 0)
    y = x + bias                       (fp32, ids 1 .. V-1; never written back)
    softmax of y (float64 from here on) | one-hot at the argmax of y, ties to the lowest id
    top-k (ties: lowest id first)  ->  rejected-token mask `wrong`  ->  renormalise  ->  top-p  ->  renormalise
    draw: the smallest id whose cumulative probability exceeds u

The GPU tests take it as their reference; tests/test_logit_bias_host.py checks it against the reference's own
probabilities (tests/golden/g9_sampling.npz) with a zero bias.  `ban_after_topk` moves the bans (the -inf entries) behind
the top-k step, which is where the rejected-token mask sits: the order a user constraint must NOT have."""
import types

import numpy as np

V = 729


def restate(raw, temperature, top_k, top_p=1.0, wrong=None, bias=None, u=0.5, V=V, ban_after_topk=False):
    """raw: float32 [>= V] logits of one sequence; wrong: bool / uint8 [>= V] or None; bias: float32 [>= V] or None.
    Returns a namespace: written (float32, the row after the call), y (float32 [V], the row the softmax saw; entry 0
    unused), full (float64 [V], log-softmax of y over ids 1 .. V-1; -inf at banned ids), probs (float64 [V], the
    distribution drawn from; NaN everywhere when it has no mass, Q12), token (-1 then), kept (log probs[token]; 0.0 for
    temperature 0; NaN without a token)."""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32 and raw.shape[0] >= V
    t32 = np.float32(temperature)
    written = raw.copy()
    if t32 != 0:
        written[1:V] = raw[1:V] / t32                                   # fp32 division (IEEE), in place: quirk Q5
    x = written[:V]
    y = x.copy()
    banned = np.zeros(V, dtype=bool)
    if bias is not None:
        b32 = np.asarray(bias)[:V]
        assert b32.dtype == np.float32
        if ban_after_topk:
            banned[1:] = b32[1:] == -np.inf
            b32 = np.where(b32 == -np.inf, np.float32(0), b32)
        y[1:] = x[1:] + b32[1:]                                         # one fp32 add
    y[0] = -np.inf                                                      # the pad column is never drawn (Q6)
    out = types.SimpleNamespace(written=written, y=y, token=-1, kept=np.nan, probs=np.full(V, np.nan),
                                full=np.full(V, np.nan))
    y64 = y.astype(np.float64)
    if not np.isfinite(y64[1:]).any():
        return out                                                      # everything banned: nothing to draw
    m = y64[1:].max()
    e = np.exp(y64 - m)
    e[0] = 0.0
    out.full = y64 - m - np.log(e.sum())
    out.full[0] = np.nan
    ids = np.arange(V)
    if t32 == 0:
        p = np.zeros(V)
        p[int(np.flatnonzero(y[1:] == y[1:].max())[0]) + 1] = 1.0       # compared as the kernel compares: in fp32
    else:
        p = e / e.sum()
    order = np.lexsort((ids, -p))                                       # decreasing probability, ties: lowest id first
    q = np.zeros(V)
    keep = order[:int(min(max(top_k, 1), V))]
    q[keep] = p[keep]
    q[banned] = 0.0
    if wrong is not None:
        q[np.asarray(wrong)[:V] != 0] = 0.0
    tot = q.sum()
    if not tot > 0:
        return out
    q /= tot
    if top_p < 1:
        order = np.lexsort((ids, -q))
        before = np.cumsum(q[order]) - q[order]
        drop = order[~(before < np.float64(np.float32(top_p)))]
        q[drop] = 0.0
        q /= q.sum()
    out.probs = q
    cdf = np.cumsum(q)
    hit = np.flatnonzero((cdf > u) & (q > 0))
    out.token = int(hit[0]) if len(hit) else int(np.flatnonzero(q > 0)[-1])
    out.kept = 0.0 if t32 == 0 else float(np.log(q[out.token]))
    return out


def ban_is_before_topk(res, banned_ids, top_k):
    """The discriminating property: with the top_k most likely ids banned (and no rejected token among the next ones) the
    distribution still has exactly top_k survivors, none of them banned."""
    if res.token < 0 or np.isnan(res.probs).any():
        return False
    return int((res.probs > 0).sum()) == top_k and not (res.probs[list(banned_ids)] > 0).any()
