"""Plain-Python statement of the form rule WITH TAKES (test infrastructure; the product never imports it): a bar the decode
loop opens may replay a bar of a finished sequence the caller supplied.  Written from the rule's text, over form_contract.

The take buffer `src` is a list of ints (None: no buffer), the tokens of every take one behind the other.  A TAKE ROW is a
table row whose word 0 has bit 7 set: src_bar | copy << 6 | 1 << 7 | (transpose + 64) << 8; word 1 is `begin`, the index in
src of the first token behind the source bar's BAR, word 2 `end`, exclusive.  Word 3, and words 1 .. 3 of every other row, are
never read.  A take row's bar is a replay bar whatever its index; it is FREE where there is no buffer, the buffer holds fewer
than 4 tokens or begin >= end.  Everything else is form_contract's.
"""
import form_contract as FC
import prime_contract as P
from form_contract import (ACTIVE, ALL, BAR_AT, BARS, CURSOR, END, G, K, NS, RHYTHM, ROW, ROWS_MAX, fields, fold,  # noqa: F401
                           initial_state, next_group, word)

TAKE = 1 << 7
SRC_MAX = 1 << 18


def row_word(src, copy=ALL, transpose=0):
    return FC.row_word(src, copy, transpose) | TAKE


def take_row(src, begin, end, copy=ALL, transpose=0, w3=0):
    return [row_word(src, copy, transpose), begin & 0xFFFFFFFF, end & 0xFFFFFFFF, w3]


def s32(w):
    w = int(w) & 0xFFFFFFFF
    return w - (1 << 32) if w >> 31 else w


def row_index(ctl, table, i):
    """The table row of bar i for the control word ctl, None where the form does not reach."""
    if ctl < 0 or i < 0 or i >= min((ctl >> 12) & 127, BARS):
        return None
    return min(max((ctl & (ROWS_MAX - 1)) + i, 0), len(table) - 1)


def bar_appended(st, ctl, table, nb, index, src=None):
    """Transition 1: a BAR was appended at `index` as the (nb + 1)-th of the sequence."""
    if 0 <= nb < BARS:
        st[BAR_AT + nb] = index
    r = row_index(ctl, table, nb)
    w = 0 if r is None else int(table[r][0])
    f = fields(w)
    st[ACTIVE:G + 1] = [0, 0, 0, 0, 0, -1]
    if f is None:
        return
    if w & TAKE:
        n = len(src) if src is not None else 0
        begin, end = s32(table[r][1]), s32(table[r][2])
        if n >= 4 and begin < end:
            cursor = min(max(begin, 0), n)
            st[ACTIVE], st[CURSOR], st[END], st[K], st[ROW] = 1, cursor, min(max(end, cursor), n), 0, w & 0x7fff
    elif f[0] < nb:
        j = f[0]
        st[ACTIVE], st[CURSOR], st[END], st[K], st[ROW] = 1, st[BAR_AT + j] + 1, st[BAR_AT + j + 1], 0, w & 0x7fff


def replay_token(st, seq, src=None):
    """Transition 2: the replay token of a slot inside a replay bar, -1 where a normal draw is made.  The four tokens come
    from the take buffer when the open bar's row has bit 7, else from seq."""
    from_take = bool(st[ROW] & TAKE) and src is not None and len(src) >= 1
    buf = src if from_take else seq
    g = next_group(buf, st[CURSOR], min(st[END], len(buf)))
    st[G] = g
    if g < 0:
        return P.BAR
    _, copy, s = fields(st[ROW])
    if st[K] != 2:
        return buf[g + st[K]]
    if copy == RHYTHM:
        return -1
    return fold(buf[g + 2], s)


def pre(s, st, seq, chord_tok, chord_pos, max_iters, ld_seq, ctl, table, src=None):
    """`pre` with the rule: returns (token fed, active, keep, draw, form_tok)."""
    len0, nbar0, cur0, ndraw0 = s[P.F_LEN], s[P.F_NBAR], s[P.F_CUR], s[P.F_NDRAW]
    t, act, kp, dr = P.pre(s, seq, chord_tok, chord_pos, max_iters, ld_seq)
    ft = -1
    if s[P.F_LEN] > len0 and seq[len0] == P.BAR:
        bar_appended(st, ctl, table, nbar0, len0, src)
    if s[P.F_CUR] != cur0 and st[ACTIVE] and st[K] == 1:
        st[K] = 0
    if dr and st[ACTIVE]:
        ft = replay_token(st, seq, src)
        if ft >= 0:
            dr = 0
            s[P.F_NDRAW] = ndraw0
    return t, act, kp, dr, ft


def post(s, st, seq, chord_pos, t, ld_seq, ctl, table, src=None):
    """`post` for a drawn or replayed token t; returns True when t was appended."""
    len0, nbar0 = s[P.F_LEN], s[P.F_NBAR]
    appended = P.post(s, seq, chord_pos, t, ld_seq)
    if appended:
        if t == P.BAR:
            bar_appended(st, ctl, table, nbar0, len0, src)
        elif st[ACTIVE]:
            st[K] += 1
            if st[K] == 4:
                st[CURSOR], st[K] = st[G] + 4, 0
    return appended


def groups_in(buf, lo, hi):
    """The note groups of buf[lo .. hi), found one behind the other as the rule finds them."""
    out, g = [], lo
    while True:
        g = next_group(buf, g, hi)
        if g < 0:
            return out
        out.append(g)
        g += 4


def form_violation(seq, start, table, src, drawn=None):
    """The reference of generate.form_violation with takes: the first closed replay bar (its BAR at index >= start, or bar 0
    of a sequence whose first BAR is the loop's) whose groups differ from its source's under the row's mode, as (bar, source
    bar), else None.  table: the form's rows [w0, begin, end, w3] with begin / end indices in src."""
    bar_at = [i for i, t in enumerate(seq) if t == P.BAR]
    ends = bar_at[1:] + ([len(seq) - 1] if seq and seq[-1] == P.EOS else [])
    for i in range(min(len(ends), len(table), BARS)):
        w = int(table[i][0])
        f = fields(w)
        if f is None or bar_at[i] < start:
            continue
        j, copy, s = f
        if w & TAKE:
            begin, end = s32(table[i][1]), s32(table[i][2])
            if src is None or len(src) < 4 or begin >= end:
                continue
            buf = src
            a_list = groups_in(src, min(max(begin, 0), len(src)), min(max(end, 0), len(src)))
        else:
            if j >= i:
                continue
            buf = seq
            a_list = groups_in(seq, bar_at[j] + 1, ends[j])
        dst = groups_in(seq, bar_at[i] + 1, ends[i])
        if len(a_list) != len(dst):
            return i, j
        for a, b in zip(a_list, dst):
            want = [buf[a], buf[a + 1], seq[b + 2] if copy == RHYTHM else fold(buf[a + 2], s), buf[a + 3]]
            if want != list(seq[b:b + 4]):
                return i, j
            if drawn is not None and [bool(drawn[b + k]) for k in range(4)] != [False, False, copy == RHYTHM, False]:
                return i, j
    return None
