"""Plain-Python statement of the primed-generation replay (test infrastructure; the product never imports it).

The two transition functions of the decode loop -- `pre` (before the model step) and `post` (after the draw), restated
from commu/midi_generator/midi_inferrer.py:239-320 field by field as the device state record holds them -- run over a
prompt with no model step: wherever `pre` decides to draw, the next prompt token is handed to `post` as the drawn
token; wherever `pre` feeds a forced token, that token must be the next prompt token.  replay() returns the record, the
token buffer, the fed stream [(token, keep)] the loop would have given the model, and the divergence (index, reason).
"""
EOS, BAR, CHORD_LO, CHORD_HI, POS0, POS_RES, VOCAB = 1, 2, 195, 303, 432, 128, 729

# field indices of the record
(F_LEN, F_FORCED, F_REDO, F_FIRST, F_FILLED, F_DONE, F_FAILED, F_ITERS, F_NBAR, F_NCHORD, F_CUR, F_LENGTH_FIT, F_NDRAW,
 F_NTRACE) = range(14)
NF = 14

# divergence reasons
FORCED, NOT_APPENDED, HAS_EOS, INVALID = 1, 2, 3, 4


def initial_record(n_cond, n_chords, num_measures):
    """The record as the decoder's load() writes it."""
    length_fit = n_chords == int(num_measures // 4 * 4)
    return [1 + n_cond, -1, 0, 1, int(num_measures % 4 == 0), 0, 0, 0, 0, n_chords, 0, int(length_fit), 0, 0]


def pre(s, seq, chord_tok, chord_pos, max_iters, ld_seq):
    """One `pre` transition: returns (token fed, active, keep, draw); s and seq are updated in place."""
    act = kp = dr = 0
    t = 0
    ln = s[F_LEN]
    last, prev = seq[ln - 1], (seq[ln - 2] if ln >= 2 else -1)
    if not s[F_DONE] and (s[F_ITERS] >= max_iters or last == EOS or ln >= ld_seq):
        s[F_DONE] = 1
    if not s[F_DONE]:
        s[F_ITERS] += 1
        if s[F_FORCED] >= 0:
            f = s[F_FORCED]
            s[F_FORCED] = -1
            seq.append(f)
            s[F_LEN] = ln + 1
            if f == BAR:
                s[F_NBAR] += 1
            t, act, kp = f, 1, 1
        else:
            if s[F_REDO]:
                s[F_REDO] = 0
            elif s[F_FIRST]:
                s[F_FIRST] = 0
                t, act, kp = last, 1, 0
            else:
                t, act, kp = last, 1, 1
            if not s[F_FILLED]:
                s[F_FILLED] = int(s[F_NBAR] > 1)
            cur = s[F_CUR]
            remnant = cur < s[F_NCHORD]
            decided = False
            if s[F_FILLED] and last == BAR:
                s[F_FORCED] = POS0
                decided = True
            elif remnant and s[F_FILLED]:
                cp = chord_pos[cur]
                posfit = prev == BAR and last == POS0
                due = posfit if s[F_LENGTH_FIT] else (posfit or (last == cp and cp != POS0))
                if due:
                    s[F_FORCED] = chord_tok[cur]
                    s[F_CUR] = cur + 1
                    decided = True
            if not decided:
                dr = 1
                s[F_NDRAW] += 1
        if act:
            s[F_NTRACE] += 1
    return t, act, kp, dr


def post(s, seq, chord_pos, t, ld_seq):
    """One `post` transition for a drawn token t; returns True when t was appended."""
    cur = s[F_CUR]
    remnant = cur < s[F_NCHORD]
    cp = chord_pos[cur] if remnant else -1
    inter = remnant and cp != POS0
    if t < 0:
        s[F_FAILED] = s[F_DONE] = 1
    elif inter and ((cp < t < POS0 + POS_RES) or t == BAR):
        s[F_FORCED] = cp
    elif CHORD_LO <= t <= CHORD_HI:
        s[F_REDO] = 1
    elif remnant and t == EOS:
        s[F_FORCED] = cp if inter else BAR
    elif not remnant and t == BAR:
        s[F_FORCED] = EOS
    else:
        if s[F_LEN] < ld_seq:
            seq.append(t)
            s[F_LEN] += 1
            if t == BAR:
                s[F_NBAR] += 1
            return True
        if t == BAR:
            s[F_NBAR] += 1
    return False


def replay(context, chord_tok, chord_pos, num_measures, prompt, ld_seq=1 << 30):
    """context: [0] + meta.  Returns (record, seq, fed, diverged): fed = [(token, keep)] of every model step the loop
    would have made (trace order); diverged = (index, reason) or (-1, -1).  An empty prompt returns the initial record.
    After the replay iters and ndraw are 0; ntrace counts the replayed steps."""
    s = initial_record(len(context) - 1, len(chord_tok), num_measures)
    seq = list(context)
    fed = []
    n = len(prompt)
    if n == 0:
        return s, seq, fed, (-1, -1)
    i, div = 0, (-1, -1)
    for _ in range(2 * n + 2):
        if i >= n:
            break
        if prompt[i] < 0 or prompt[i] >= VOCAB:
            div = (i, INVALID)
            break
        if s[F_FORCED] >= 0 and s[F_FORCED] != prompt[i]:
            div = (i, FORCED)
            break
        len0 = s[F_LEN]
        t, act, kp, dr = pre(s, seq, chord_tok, chord_pos, 0x7fffffff, ld_seq)
        if s[F_DONE]:
            div = (i, INVALID)
            break
        if act:
            fed.append((t, kp))
        if s[F_LEN] > len0:
            if prompt[i] == EOS:
                div = (i, HAS_EOS)
                break
            i += 1
        if dr:
            tv = prompt[i]
            if not post(s, seq, chord_pos, tv, ld_seq):
                div = (i, NOT_APPENDED)
                break
            if tv == EOS:
                div = (i, HAS_EOS)
                break
            i += 1
    if div[0] < 0 and i < n:
        div = (i, INVALID)
    s[F_ITERS] = 0
    s[F_NDRAW] = 0
    return s, seq, fed, div


def kept(fed):
    """The tokens of the kept model steps: what the cache holds after the context, one position each."""
    return [t for t, k in fed if k]


# ---- shared cases of the host and GPU tests (the reference's fixtures, tests/golden/g6_decode.npz)
TAGS = ("greedy8", "greedy5", "sample8", "sample8m", "sample4x")


def fixture(z, tag):
    """(context, chord tokens, chord positions, num_measures, the fixture's sequence after the context without its EOS)."""
    meta = [int(t) for t in z["encoded_meta"]]
    seq = [int(t) for t in z[f"{tag}_seq"]]
    assert seq[:1 + len(meta)] == [0] + meta
    p = seq[1 + len(meta):]
    if p and p[-1] == EOS:
        p = p[:-1]
    return ([0] + meta, [int(t) for t in z[f"{tag}_chord_token"]], [int(t) for t in z[f"{tag}_chord_position"]],
            float(z[f"{tag}_cfg"][1]), p)


def cut_points(p):
    """Prompt lengths worth testing: empty, one token, right after a BAR, after the forced 432 that follows a BAR, after
    a chord token (first and last occurrence of each), and the whole sequence (the last token before EOS)."""
    kinds = {"bar": [], "pos": [], "chord": []}
    for k in range(1, len(p) + 1):
        if p[k - 1] == BAR:
            kinds["bar"].append(k)
        if k >= 2 and p[k - 2] == BAR and p[k - 1] == POS0:
            kinds["pos"].append(k)
        if CHORD_LO <= p[k - 1] <= CHORD_HI:
            kinds["chord"].append(k)
    cuts = {0, 1, len(p)}
    for ks in kinds.values():
        if ks:
            cuts.update((ks[0], ks[-1]))
    return sorted(cuts)


def planted(z):
    """Prompts the rules could not have produced: [(name, fixture tag, prompt, (index, reason))]."""
    g8, s8, s4 = fixture(z, "greedy8")[4], fixture(z, "sample8")[4], fixture(z, "sample4x")[4]
    out = [("chord where a draw is expected", "greedy8", [200], (0, NOT_APPENDED))]
    k = next(k for k in range(2, len(g8)) if g8[k - 2] == BAR and g8[k - 1] == POS0 and CHORD_LO <= g8[k] <= CHORD_HI)
    out.append(("wrong chord", "greedy8", g8[:k] + [g8[k] + 1], (k, FORCED)))
    cp = fixture(z, "sample4x")[2]
    j = next(i for i, c in enumerate(cp) if c != POS0)                      # the first mid-bar chord position
    ct = fixture(z, "sample4x")[1]
    # right after chord j - 1 was forced, chord j (at position cp[j] of the same bar) is pending: a later position skips it
    k = next(k for k in range(1, len(s4)) if s4[k - 1] == ct[j - 1] and sum(CHORD_LO <= t <= CHORD_HI for t in s4[:k]) == j)
    out.append(("position past a pending chord", "sample4x", s4[:k] + [cp[j] + 1], (k, NOT_APPENDED)))
    k = next(k for k in range(1, len(g8)) if CHORD_LO <= g8[k - 1] <= CHORD_HI)      # the token after a chord is drawn
    out.append(("EOS with chords left", "greedy8", g8[:k] + [EOS], (k, NOT_APPENDED)))
    out.append(("BAR with no chord left", "sample8", s8 + [BAR], (len(s8), NOT_APPENDED)))
    out.append(("EOS inside the prompt", "sample8", s8 + [EOS, 500], (len(s8), HAS_EOS)))
    return out
