"""Plain-Python statement of the form rule (test infrastructure; the product never imports it): a bar the decode loop
opens itself may replay an earlier bar of its own sequence.  Written from the rule's text, over prime_contract.pre / post.

A NOTE GROUP is four consecutive tokens Position (432 .. 559), Velocity (131 .. 194), Pitch (3 .. 130), Duration
(304 .. 431).  bar_at[i] is the index of the (i+1)-th BAR token of seq (context and prompt counted); bar i is the stretch
bar_at[i] < index < bar_at[i+1]; the open bar is max(F_NBAR - 1, 0).

A form's row is a word: 0 free, else src | copy << 6 | (transpose + 64) << 8.  A slot's control word is -1 (off) or
base + 4096 R: bar i < min(R, 64) uses table row base + i, later bars are free.

The per-slot state is a list of NS ints: active, cursor, end, k, row, g, two reserved, then bar_at[0 .. 63].
"""
import prime_contract as P

BARS = 64
ROWS_MAX = 4096
ACTIVE, CURSOR, END, K, ROW, G, BAR_AT = 0, 1, 2, 3, 4, 5, 8
NS = BAR_AT + BARS
ALL, RHYTHM = 0, 1


def word(base, bars):
    return base + ROWS_MAX * bars


def row_word(src, copy=ALL, transpose=0):
    return src | (copy << 6) | ((transpose + 64) << 8)


def fields(w):
    """(src, copy, transpose) of a row word, None for a free bar."""
    if (w >> 8) & 127 == 0:
        return None
    return w & 63, (w >> 6) & 1, ((w >> 8) & 127) - 64


def is_group(seq, g):
    return (g + 3 < len(seq) and 432 <= seq[g] <= 559 and 131 <= seq[g + 1] <= 194 and 3 <= seq[g + 2] <= 130
            and 304 <= seq[g + 3] <= 431)


def next_group(seq, cursor, end):
    """The smallest g >= cursor with g + 3 < end whose four tokens are a note group, -1: none."""
    for g in range(max(cursor, 0), end - 3):
        if is_group(seq, g):
            return g
    return -1


def fold(pitch_token, s):
    m = pitch_token - 3 + s
    while m < 0:
        m += 12
    while m > 127:
        m -= 12
    return m + 3


def initial_state(seq, length=None):
    """The state as a load or an arm leaves it: nothing replayed, the BARs of seq[:length] recorded."""
    st = [0] * NS
    st[G] = -1
    n = len(seq) if length is None else length
    bars = [i for i in range(n) if seq[i] == P.BAR]
    for r, i in enumerate(bars[:BARS]):
        st[BAR_AT + r] = i
    return st


def row_of(ctl, table, i):
    """Word 0 of bar i's row for the control word ctl, 0 (free) where the form does not reach."""
    if ctl < 0 or i < 0 or i >= min((ctl >> 12) & 127, BARS):
        return 0
    return int(table[min(max((ctl & (ROWS_MAX - 1)) + i, 0), len(table) - 1)][0])


def bar_appended(st, ctl, table, nb, index):
    """Transition 1: a BAR was appended at `index` as the (nb + 1)-th of the sequence."""
    if 0 <= nb < BARS:
        st[BAR_AT + nb] = index
    w = row_of(ctl, table, nb)
    f = fields(w)
    st[ACTIVE:G + 1] = [0, 0, 0, 0, 0, -1]
    if f is not None and f[0] < nb:
        j = f[0]
        st[ACTIVE], st[CURSOR], st[END], st[K], st[ROW] = 1, st[BAR_AT + j] + 1, st[BAR_AT + j + 1], 0, w & 0x7fff


def replay_token(st, seq):
    """Transition 2, for a slot inside a replay bar whose `pre` reached the draw decision: the replay token, -1 where a
    normal draw is made (rhythm mode at the pitch).  Records the group found."""
    g = next_group(seq, st[CURSOR], st[END])
    st[G] = g
    if g < 0:
        return P.BAR
    _, copy, s = fields(st[ROW])
    if st[K] != 2:
        return seq[g + st[K]]
    if copy == RHYTHM:
        return -1
    return fold(seq[g + 2], s)


def pre(s, st, seq, chord_tok, chord_pos, max_iters, ld_seq, ctl, table):
    """`pre` with the rule: returns (token fed, active, keep, draw, form_tok)."""
    len0, nbar0, cur0, ndraw0 = s[P.F_LEN], s[P.F_NBAR], s[P.F_CUR], s[P.F_NDRAW]
    t, act, kp, dr = P.pre(s, seq, chord_tok, chord_pos, max_iters, ld_seq)
    ft = -1
    if s[P.F_LEN] > len0 and seq[len0] == P.BAR:                 # a forced BAR was appended
        bar_appended(st, ctl, table, nbar0, len0)
    if s[P.F_CUR] != cur0 and st[ACTIVE] and st[K] == 1:         # transition 4: the chord took the replayed position
        st[K] = 0
    if dr and st[ACTIVE]:
        ft = replay_token(st, seq)
        if ft >= 0:                                              # no variate, draw stays 0
            dr = 0
            s[P.F_NDRAW] = ndraw0
    return t, act, kp, dr, ft


def post(s, st, seq, chord_pos, t, ld_seq, ctl, table):
    """`post` for a drawn or replayed token t (transitions 3 and 5); returns True when t was appended."""
    len0, nbar0 = s[P.F_LEN], s[P.F_NBAR]
    appended = P.post(s, seq, chord_pos, t, ld_seq)
    if appended:
        if t == P.BAR:
            bar_appended(st, ctl, table, nbar0, len0)
        elif st[ACTIVE]:
            st[K] += 1
            if st[K] == 4:
                st[CURSOR], st[K] = st[G] + 4, 0
    return appended


def form_violation(seq, start, rows, drawn=None):
    """The reference of generate.form_violation: the first closed replay bar (its BAR at index >= start, closed by the next
    BAR or by the EOS that replaced it) whose note groups differ from its source's under the row's mode, as (bar, source),
    else None.  rows: the form's words 0, one per bar."""
    bar_at = [i for i, t in enumerate(seq) if t == P.BAR]
    ends = bar_at[1:] + ([len(seq) - 1] if seq and seq[-1] == P.EOS else [])

    def groups(i):
        out, g = [], bar_at[i] + 1
        while True:
            g = next_group(seq, g, ends[i])
            if g < 0:
                return out
            out.append(g)
            g += 4
    for i in range(min(len(ends), len(rows), BARS)):
        f = fields(int(rows[i]))
        if f is None or bar_at[i] < start:
            continue
        j, copy, s = f
        src, dst = groups(j), groups(i)
        if len(src) != len(dst):
            return i, j
        for a, b in zip(src, dst):
            want = [seq[a], seq[a + 1], seq[b + 2] if copy == RHYTHM else fold(seq[a + 2], s), seq[a + 3]]
            if want != list(seq[b:b + 4]):
                return i, j
            if drawn is not None and [bool(drawn[b + k]) for k in range(4)] != [False, False, copy == RHYTHM, False]:
                return i, j
    return None
