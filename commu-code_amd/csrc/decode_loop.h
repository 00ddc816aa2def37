// Per-sequence stages of the decode loop iteration as device functions (one 64-lane wave per sequence), shared by the
// stand-alone kernels (sample.hip, forcing.hip) and the fused sample -> post -> pre launch (forcing.hip).
#pragma once
#include "common.h"
#include "form.h"

namespace {

// Wave-wide reductions and scans without LDS traffic: DPP inside the rows of 16 lanes, v_readlane across the four rows
// (a __shfl_* is a ds_bpermute_b32 + wait, ~130 cycles each; the sampling step made 54 of them in a row: 3 us).
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ float lane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float wsum_f(float v) {          // uniform result
    v = row16_sum(v);
    return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
__device__ __forceinline__ float wmax_f(float v) {
    v = row16_max(v);
    return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}
__device__ __forceinline__ int wmin_i(int v) {
    v = min(v, dpp_i<0xB1>(v)); v = min(v, dpp_i<0x4E>(v)); v = min(v, dpp_i<0x141>(v)); v = min(v, dpp_i<0x140>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wmax_i(int v) {
    v = max(v, dpp_i<0xB1>(v)); v = max(v, dpp_i<0x4E>(v)); v = max(v, dpp_i<0x141>(v)); v = max(v, dpp_i<0x140>(v));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// inclusive prefix sums in lane order: row_shr 1, 2, 4, 8 (lanes without a source add 0), then the totals of the rows before
__device__ __forceinline__ float wscan_f(float v, int lane) {
    v += dpp_f<0x111>(v); v += dpp_f<0x112>(v); v += dpp_f<0x114>(v); v += dpp_f<0x118>(v);
    const float t0 = lane_f(v, 15), t1 = lane_f(v, 31), t2 = lane_f(v, 47);
    const int r = lane >> 4;
    return v + ((r >= 1 ? t0 : 0.f) + (r >= 2 ? t1 : 0.f) + (r >= 3 ? t2 : 0.f));
}
__device__ __forceinline__ int wscan_i(int v, int lane) {
    v += dpp_i<0x111>(v); v += dpp_i<0x112>(v); v += dpp_i<0x114>(v); v += dpp_i<0x118>(v);
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    const int r = lane >> 4;
    return v + (r >= 1 ? t0 : 0) + (r >= 2 ? t1 : 0) + (r >= 3 ? t2 : 0);
}

// ------------------------------------------------------------------------------------------------ sampling step (K15)
constexpr int PER_LANE = 12;      // 64 * 12 = 768 >= 729: lane l owns ids [12 l, 12 l + 12)
constexpr int TOK_EOS = 1, TOK_BAR = 2, TOK_CHORD_LO = 195, TOK_CHORD_HI = 303, TOK_POS0 = 432, POS_RES = 128;
constexpr int VOCAB = 729;

// The sampling controls of one sequence: scalars for the whole launch, or per-sequence device arrays ([B] each, null: the
// scalar applies) -- the slots of one batch may sample at different settings, and a captured graph follows the arrays.
struct SamplingRows {
    const float* temperature;
    const int* top_k;
    const float* top_p;
};

// the pair of log-probabilities of a drawn token (see sample_topk_body); NaN, NaN: nothing was drawn
struct TokenLogp {
    float full, kept;
};

// one wave per sequence b (lane = threadIdx.x of a 64-thread workgroup)
// want_logp: also compute `lp`, uniform over the wave, for the drawn token (left alone for inactive sequences) --
//   full: log-softmax over ids 1 .. V-1 of the row as this draw used it (logits / temperature as written back, the
//         compounded row on a Q5 re-draw; the raw row for temperature == 0) at the drawn id, as x[id] - max - log(sum);
//   kept: log of the probability the token had in the distribution it was drawn from (after top-k, rejected-token mask,
//         top-p and renormalisation; exactly 0 for greedy);
// and store it to logp_out[b][0:2] when that is not null.
// BIAS (bias fp32 [B][ld_bias], ld_bias >= V): a constraint of the caller's on what sequence b may draw.  With x the
//   value above (logits / temperature, the raw row for greedy) the distribution is built from y[id] = x[id] + bias[b][id],
//   one fp32 add: a finite entry re-weights an id, -inf bans it (its probability is exactly 0 and it takes none of the k
//   places: bias, then top-k, then the rejected-token mask, then top-p).  What is written back is x, never y, so a Q5
//   re-draw adds the bias once to the compounded row; `full` is the log-softmax of y.  A row banned entirely has no
//   mass: the Q12 exit below.  Without BIAS the pointer is not looked at and the code is what it was.
// GRAM (Grammar: table fp32 [8][ld], ld >= V): a constraint chosen by the sequence's own state -- row c of the table is
//   added for a draw whose PREVIOUS token (the last token of seq when the stage runs; the same one on a Q5 re-draw) has
//   class c (token_class), row 7 (zeros by convention) for a sequence whose grammar is off: y[id] = (x[id] + bias[b][id]) +
//   table[c][id], in that fp32 order.  All that is said of the bias holds: before top-k, never written back, -inf bans.
//   The row index is uniform over the wave (scalar), there is no branch on it.  Without GRAM nothing of `g` is looked at.
//   The previous token is a load that depends on the record's length, and the table row one that depends on it: the body
//   issues the first right behind its logits loads, so that the logits, the bias and the rejected-token map travel under
//   the chain record -> previous token -> table row instead of behind it (the caller passes `len` and `on` as it loaded
//   them, without waiting for them).
struct Grammar {
    const float* table;
    int ld;
    const int* seq_row;     // the sequence's row of seq
    int len, ld_seq;        // tokens in it (the record's F_LEN; clamped into the row whatever it holds)
    int on;                 // the sequence's switch
};
// token classes of the event grammar by id ranges (TOKEN_OFFSET): 0 OTHER (pad, EOS, ids >= 560), 1 BAR, 2 PITCH, 3 VELOCITY,
// 4 CHORD, 5 DURATION, 6 POSITION -- range compares, no table in memory; any int is classified (negative: OTHER)
__device__ __forceinline__ int token_class(int t) {
    int c = 0;
    c = t >= 2 ? 1 : c;
    c = t >= 3 ? 2 : c;
    c = t >= 131 ? 3 : c;
    c = t >= 195 ? 4 : c;
    c = t >= 304 ? 5 : c;
    c = t >= 432 ? 6 : c;
    c = t >= 560 ? 0 : c;
    return c;
}
// HARM (Harmony: table fp32 [111][ld], ld >= 12): a third additive term, chosen by the chord the sequence is in.  Row r of
//   the table is 12 values by MIDI pitch class (column 0: C) and is added at the pitch ids only -- token id is MIDI pitch
//   id - 3 (TOK_PITCH_LO .. TOK_PITCH_HI): y[id] = ((x[id] + bias[b][id]) + table[c][id]) + harm[r][(id - 3) mod 12] for
//   3 <= id <= 130, in that fp32 order; every other id gets NO third add.  r = t - 195 for the last chord token t
//   (195 .. 303) of seq when the stage runs, 109 while seq holds none, 110 (zeros by convention) for a sequence whose
//   switch is off.  A chord enters seq only as a forced token, taken from chord_tok[b][F_CUR] when F_CUR is incremented
//   and appended by the next iteration with no draw in between, and a drawn chord is never appended (forcing_pre_body /
//   forcing_post_body; the prompt replay runs the same bodies): at every draw the last chord of seq is
//   chord_tok[b][F_CUR - 1], and there is none while F_CUR == 0 (tests/test_harmony_host.py walks the rules to show it).
//   So the row is record -> chord token -> 12 floats, as many dependent loads as the grammar's record -> previous token ->
//   row.  The chord token load is issued beside the grammar's previous-token load; the row's loads are NOT beside the
//   grammar's: as compiled they go out after the grammar row's, once the switch byte (a vector load queued behind the
//   logits and bias loads) and the chord token are both here, one scalar round trip behind the grammar's chain (measured:
//   docs/EXPERIMENTS.md 8s).
//   The row index is uniform over the wave (scalar, no branch on it), and since a lane owns PER_LANE = 12 consecutive ids
//   the pitch class of its element e is (e + 9) mod 12 for every lane: the 12 values are wave-uniform too, only the range
//   test is per lane.  All that is said of the bias holds: before top-k, never written back, -inf bans.  Without HARM
//   nothing of `h` is looked at.
struct Harmony {
    const float* table;
    int ld;
    const int* chord_row;   // the sequence's row of chord_tok
    int cur, ld_chord;      // chords consumed so far (the record's F_CUR; clamped into the row whatever it holds)
    int on;                 // the sequence's switch
};
constexpr int TOK_PITCH_LO = 3, TOK_PITCH_HI = 130, HARM_NO_CHORD = 109, HARM_OFF = 110;
// CLS (ClassControls: records {float temperature; int top_k; float top_p; int reserved} [8] per sequence, 16 bytes each,
//   one sequence's table one 128-byte line): the sampling triple of a draw is chosen by the class of the sequence's
//   PREVIOUS token -- the grammar's key, the same load with the same clamp, but NOT gated by the grammar's switch: record
//   c = token_class(prev) of the sequence's table, so rows 0 .. 6 are selected and row 7 never is (the host keeps the slot's
//   base triple there).  With CLS the triple comes from that record ONLY: neither the scalars nor `rows` are looked at (their
//   loads are not issued).  Everything after the selection is the code below as it stands -- the clamp of top_k, greedy for
//   temperature == 0, the in-place division by the SELECTED temperature (a Q5 re-draw sees the same previous token, selects
//   the same record and compounds by the same temperature) -- so a draw with record (t, k, p) is bit for bit the draw of
//   the array-mode kernel for a sequence whose rows hold (t, k, p).
//   PLACEMENT: ONE load of record c, issued when the class is known.  Its address is wave-uniform, so it is a scalar
//   load (s_load_dwordx4) that lands in scalar registers and never enters the vector queue; it goes out right behind the
//   grammar row's 12 vector loads, which the first arithmetic waits for anyway, so the extra dependent step of the chain
//   record -> previous token -> class -> control record travels under them.  The other placement -- the slot's whole
//   128-byte table loaded UP FRONT beside the logits (lane l takes record l & 7 as one 16-byte vector load) and the record
//   picked with v_readlane at the scalar index c, so that no load depends on the class -- was built and measured: 0.07 us
//   SLOWER on the kernel alone (8.38 against 8.31 .. 8.32 us; its vector load queues behind the logits and bias loads and
//   the pick waits for it), no difference per iteration (docs/EXPERIMENTS.md 8u).  The three values are wave-uniform and
//   held in scalar registers, so the greedy / radix / nucleus branches stay scalar branches, as with SamplingRows.
//   CLS needs GRAM (the previous token is the grammar's load); callers without a grammar pass the all-off switch array.
struct ClassControls {
    const int4* table;      // the sequence's 8 records
};
// ORD (NoteOrder: one int32 control per sequence, -1 off, 0 on, n in 1 .. 128 on with at most n notes per position): a ban
//   chosen by what the sequence already holds at its current position, defined on seq alone when the stage runs (as the
//   harmony row is: a Q5 re-draw, a re-armed and a primed sequence need no state of their own).  With L = min(max(F_LEN, 0),
//   ld_seq) and S = seq[b][0:L]: j is the largest index with S[j] BAR or a POSITION token; none, or BAR: nothing is
//   banned.  Else p = S[j], s is one past the largest i < j with S[i] BAR or a POSITION token != p (0: none), the RUN is
//   S[s:L], D the PITCH tokens in it and n their number with multiplicity.  Banned: ids 432 .. p - 1 (the position never
//   goes back), every id in D (no doubled note), and p itself when ctl >= 1 and n >= ctl (the cap).  A banned id's y is
//   REPLACED by -inf after the harmony term -- a select, not an add: y = banned ? -inf : ((x + bias) + gram) + harm -- so
//   all that is said of the bias holds (before top-k, never written back, probability exactly 0, `full` the log-softmax of
//   y, a row with nothing left takes the Q12 exit), and a draw is bit for bit the CLS kernel's with bias[b] = -inf at the
//   banned ids.  The bans apply whatever class is drawn and whatever the grammar's switch says.
//   THE SCAN: lane l loads S[L - 1 - l - 64 c] for chunk c = 0, 1, .. (index clamped, lane carries a valid flag).  Chunk 0
//   depends on F_LEN only and is issued beside the grammar's previous-token load, so it travels under the existing chain
//   record -> previous token -> grammar row.  j and s are the lowest set lanes of two ballots ("BAR or POSITION", then "BAR
//   or POSITION != p"; p by v_readlane); a chunk without the breaker looked for loops to the next one -- the trip count is
//   wave-uniform (a scalar branch), bounded by ceil(L / 64), and a normal bar ends it in chunk 0.  p, n and the phase stay
//   in scalar registers.  THE PITCH SET goes through LDS: the lanes of the run that hold a pitch write a flag at their id
//   (192 ints, zeroed first), and the lanes that own the ids 0 .. 191 read their 12 flags back as three 16-byte reads -- one
//   wave, LDS operations complete in order.  (The other design, four 32-bit words OR-reduced over the wave with the DPP
//   helpers, was not built.)  The switch is one scalar: an off sequence runs the same scan and bans nothing, there is no
//   branch on it.  Cost: +0.40 us on the kernel alone, +0.20 us more for a second chunk (docs/EXPERIMENTS.md 8v).
//   ORD needs CLS (and so GRAM: the row of seq and its length are the grammar's).
struct NoteOrder {
    int ctl;                // the sequence's control as the caller loaded it
};
constexpr int ORD_FLAGS = 192;    // LDS flags by token id: 16 lanes * 12 ids >= TOK_PITCH_HI + 1
// VOX (Voices: one int32 control per sequence, -1 off, else N + 256 r with N in 0 .. 128 the voice cap (0: none) and r the
//   re-strike switch): two more bans read off seq, so that at most N drawn notes sound at once and no pitch is struck while
//   it sounds.  With S as above, a NOTE is an index i, i + 3 < L, with S[i .. i+3] = POSITION, VELOCITY, PITCH, DURATION; start
//   a = S[i] - 432, length d = S[i+3] - 303, beta = the BAR tokens in S[i+4 : L], end on the current bar's grid
//   e = min(a + d - 128 beta, 128); notes with beta >= 2 are ignored (a + d <= 255: they ended before this bar).  CAP (N >= 1):
//   E = the N-th largest e with multiplicity (0: fewer than N notes, or the value is <= 0); banned: ids 432 .. 432 + E - 1.
//   RE-STRIKE (r): with j the note order's last breaker and g0 = 0 for BAR, S[j] - 432 else: the pitch of every note with
//   e > g0.  The bans join the note order's in the same select -- hi = max(hi_order, 432 + E), the pitch sets are united --
//   so a draw is bit for bit the ORD kernel's with bias[b] = -inf at these ids.
//   THE SCAN is the note order's, continued to the second BAR from the end (or index 0): the trip count stays wave-uniform.
//   Lane l holds S[idx], idx = start - l, and with VOX also S[idx-1 .. idx-3] (three more clamped loads from the same lines;
//   a note is seen by the lane that holds its DURATION, so a note that straddles a chunk seam needs nothing special).  beta
//   is v_mbcnt of the chunk's BAR ballot (the BARs in lower lanes, i.e. at higher indices) plus a scalar carry from the
//   chunks before.  E FOR EVERY N goes through a 128-bin LDS histogram of the ends 1 .. 128, highest end first: each lane reads
//   two bins, one wscan_i gives #{e > g} for its two grid steps, and E is the smallest g with #{e > g} < N (a wmin_i).
//   THE PITCH SET has flags of its own (the note order's are gated by the note order's switch, these by r).  A lane needs g0
//   when it writes its flag: the first ballot of the chunk has run by then, and while it has found no breaker the lane's own
//   POSITION (in the next chunk) is j, its note starts at g0 and sounds.  N, r, E and g0 stay in scalar registers; an off
//   word runs the same scan and bans nothing.  VOX needs ORD.
struct Voices {
    int ctl;                // the sequence's control as the caller loaded it
};
constexpr int VOX_BINS = 128;     // LDS histogram of the note ends: slot 128 - e for e in 1 .. 128 (lane l reads slots 2l, 2l + 1)
constexpr int TOK_VEL_LO = 131, TOK_VEL_HI = 194, TOK_DUR_LO = 304, TOK_DUR_HI = 431;
// DEN (Density: one int32 control per sequence, -1 off, else lo + 256 hi with lo, hi in 0 .. 255; 0: that bound is not set):
//   bounds on the notes of the bar being written.  With NOTE and beta as for VOX, C = the number of notes with beta == 0 (the
//   complete groups behind the last BAR of S, or anywhere in S when it holds none).  UPPER (hi >= 1 and C >= hi): every
//   POSITION id 432 .. 559 is banned -- the end of the banned position range becomes 560, the maximum of the note order's, the
//   voice cap's and this one.  LOWER (lo >= 1 and C < lo): BAR and EOS are banned, unless that merged end is 560 already: a
//   bar that cannot take another onset can still end (without the waiver such a row would have nothing left of the boundary
//   family and every attempt would end by Q12).  The bans join the select of ORD and VOX, so a draw is bit for bit the VOX
//   kernel's with bias[b] = -inf at these ids.
//   THE COUNT rides on the voice walk, which already visits every note back to the second BAR from the end: one more ballot
//   of `note & beta == 0` per chunk, its popcount carried in a scalar.  No LDS, no load but the control word, the same trip
//   count.  lo, hi, C and the waiver are scalars; BAR and EOS are ids 2 and 1 of lane 0.  An off word runs the same walk and
//   bans nothing.  DEN needs VOX.
struct Density {
    int ctl;                // the sequence's control as the caller loaded it
};
// MEL (Interval: one int32 control per sequence, -1 off, else up + 256 down + 65536 u with up, down in 0 .. 127; 0: that
//   bound is not set; u the unison switch): a cap on the leap from the last note to the pitch drawn next.  With NOTE and beta
//   as for VOX, the REFERENCE NOTE is the note with beta <= 1 whose index is largest and q its PITCH token; none (the first
//   note of a sequence, a line that rested for a whole bar or more): nothing is banned.  UP (up >= 1): ids q + up + 1 .. 130
//   are banned.  DOWN (down >= 1): ids 3 .. q - down - 1.  UNISON (u): id q.  One id is one semitone.  The bans join the
//   select of ORD, VOX and DEN, so a draw is bit for bit the DEN kernel's with bias[b] = -inf at these ids.
//   THE REFERENCE NOTE rides on the voice walk: the lane that holds a note's DURATION has `note` (beta <= 1 is part of it)
//   and the note's PITCH in t1, and lower lanes hold higher indices -- the first chunk from the end whose ballot of `note`
//   is non-zero gives q = v_readlane(t1, lowest set lane).  One more ballot per chunk, no LDS, no load but the control
//   word, the same trip count (the walk goes back to the second BAR from the end, so it passes every note with beta <= 1).
//   q, the found flag, up, down and u are scalars; the bans are two bit ranges and one bit per lane, built like the position
//   range.  An off word runs the same walk and bans nothing.  MEL needs DEN.
struct Interval {
    int ctl;                // the sequence's control as the caller loaded it
};
// ONS (Onsets: one int32 control per sequence, -1 off, else base + 4096 R with R in 1 .. 64 the cycle length, base in
//   0 .. 4095, base + R <= rows; table uint32 [rows][4], 1 <= rows <= 4096): WHEN a note may start.  A row is a 128-bit mask
//   over the bar's grid: bit g % 32 of word g / 32 set means POSITION id 432 + g may be drawn.  With nb the BAR tokens in S,
//   the open bar is i = max(nb - 1, 0) (the stretch before the first BAR uses bar 0's row, as DEN counts it), its row
//   base + (i mod R), and every POSITION id whose bit is clear is banned.  The bans join the select of ORD, VOX, DEN and MEL,
//   so a draw is bit for bit the MEL kernel's with bias[b] = -inf at these ids; an all-clear row is a bar of rest.
//   nb IS NOT COUNTED: it is the record's F_NBAR, which forcing_pre_body / forcing_post_body keep equal to seq.count(BAR)
//   on every path that appends a token (the forced append and the drawn append below; load() writes 0 beside a seq of
//   conditioning tokens, none of which is BAR; the prompt replay runs the same two bodies; rearm / admit / the arm launches
//   copy a record that one of these wrote).  The fused loop has it in registers, the stand-alone launch reads it beside F_LEN.
//   THE ROW is wave-uniform: control word and nb are scalars, so the four words are one scalar load whose address needs the
//   record only; it is issued beside the grammar row's loads and travels under the chain record -> previous token -> grammar
//   row.  The row index is clamped to rows - 1, so the kernel stays in bounds whatever an array holds; an off word
//   substitutes the all-ones row by a select, there is no branch on it.  A lane builds the bits of its 12 ids from the row
//   with one 64-bit shift (ids 432 .. 559 are lanes 36 .. 46; 12 bits span at most two words).
//   THE DENSITY WAIVER changes with ONS: DEN's lower bound bans BAR and EOS unless no position is left, and a position is
//   left only where the merged banned range [432, hi) AND the row leave it -- row AND NOT range, four scalar words tested
//   against zero.  With the all-ones row that is hi != 560, the parent's test.  No LDS, no load but the control word and the
//   row.  ONS needs MEL.
struct Onsets {
    int ctl;                // the sequence's control as the caller loaded it
    const unsigned* table;  // uint32 [rows][4]
    int rows;               // 1 .. 4096 (the entry points refuse anything else)
    int nbar;               // the record's F_NBAR
};
constexpr int ONS_ROWS_MAX = 4096, ONS_CYCLE_MAX = 64;
// GDE (Guide: one int32 control per sequence, -1 off, else base + 65536 R + 2^23 s with R in 1 .. 64 the cycle length in
//   bars, s in 0 .. 7 and C = 128 >> s the cells of a bar, base in 0 .. 65535, base + R (1 + C) <= rows; table uint32
//   [rows][4], 1 <= rows <= 65536): WHICH PITCH a note may take, by the time it starts -- a mask over pitches indexed by time,
//   derived on the host from a finished track or given raw.  A bar of the template is a BLOCK of 1 + C consecutive rows: row 0
//   the bar's LIVE ROW, a 128-bit mask over POSITIONS in the onset table's format (bit g: a note may start at step g); rows
//   1 .. C the CELL ROWS, 128-bit masks over PITCHES (bit k % 32 of word k / 32 set: PITCH id 3 + k may be drawn).
//   THE BLOCK OF THE OPEN BAR mirrors ONS: i = max(nb - 1, 0) with nb the record's F_NBAR (never counted on a draw, a
//   prompt's bars included), block = base + (i mod R) (1 + C).
//   PITCH BAN: j and p are ORD's (j the largest index with S[j] BAR or a POSITION).  No such j, or S[j] BAR: no pitch is
//   banned.  Else g = p - 432, the cell row is block + 1 + (g >> s), and every PITCH id 3 .. 130 whose bit is clear is banned;
//   ids outside 3 .. 130 are never touched (lane 10 owns ids 120 .. 131, and id 131 is a velocity).
//   POSITION BAN: every POSITION id whose bit in the live row is clear is banned -- the live row is ANDed into the four onset
//   words before they are used, so the ONS position ban AND ITS DENSITY WAIVER apply to the intersection with no new code:
//   the waiver lets a bar end once range, onset row and live row together leave no position.
//   The bans join the one select of ORD, VOX, DEN, MEL and ONS, so a draw is bit for bit the ONS kernel's with bias[b] = -inf
//   at these ids (and DEN's BAR / EOS ban taken under the waiver on the ANDed row); an off word, or a word over an all-ones
//   live row with all-ones cell rows, is bit for bit the ONS kernel.  Every row index is clamped to rows - 1, whatever the
//   arrays hold.
//   THE LOADS: the live row is one scalar 16-byte load whose address needs the record and the control word only; it goes out
//   beside the onset row's, ahead of the chain.  The cell row is one scalar 16-byte load whose address needs p: it is issued
//   as soon as the first ballot of the scan has produced j -- behind chunk 0 for a normal bar, behind the chunk loop
//   otherwise (the trip count is wave-uniform already, so is this branch).  Off words select all ones, no branch on the
//   switch.  A lane builds its 12 pitch bits with the 64-bit shift ONS uses; the start bit is base - 3, negative for lane 0,
//   which shifts from bit 0 and moves the result up by 3 instead (ids 0 .. 2 are outside the pitch range and masked out).
//   No LDS, no load but the word and the two rows.  (As compiled the three row loads are s_load_dwordx4 in the stand-alone
//   kernel; in the fused loop kernel, which stores to global memory ahead of them, they come out as uniform-address vector
//   loads, as the onset row's does there: docs/EXPERIMENTS.md 9c.)
//   NOT COVERED: only a note's START is tested (a drawn note held across a later change of the guide is not checked); forced
//   tokens (the position 0 after a BAR, a chord's position); notes inside a prompt; a pitch range, strict harmony or interval
//   window that together with the cell row leaves no pitch ends the attempt by Q12, as before.  GDE needs ONS.
struct Guide {
    int ctl;                // the sequence's control as the caller loaded it
    const unsigned* table;  // uint32 [rows][4]
    int rows;               // 1 .. 65536 (the entry points refuse anything else)
};
constexpr int GDE_ROWS_MAX = 65536, GDE_CYCLE_MAX = 64;
// ART (Articulation: one int32 control per sequence, -1 off, else base + 4096 R + 2^19 w + 2^20 h with R in 1 .. 64 the
//   cycle length in bars, base in 0 .. 4095, base + R <= rows, w the bar-line switch and h the guide-hold switch; table
//   uint32 [rows][4], 1 <= rows <= 4096): HOW LONG a note lasts and HOW LOUD it is.  A row is one bar of a template: word 0
//   is dlo | dhi << 8, each 0 .. 128 (0: that bound is not set); words 1 and 2 a 64-bit mask over velocities (bit k % 32 of
//   word 1 + k / 32 set: VELOCITY id 131 + k may be drawn); word 3 is reserved, written 0 by the host and never read.
//   THE ROW OF THE OPEN BAR mirrors ONS: i = max(nb - 1, 0) with nb the record's F_NBAR (never counted on a draw, a prompt's
//   bars included), row = base + (i mod R), clamped to rows - 1 whatever the arrays hold.
//   VELOCITY BAN: every VELOCITY id 131 .. 194 whose bit is clear is banned; ids 130 and 195 are never touched.
//   DURATION WINDOW: j and p are ORD's; a = p - 432 exists when S[j] is a POSITION; k = q - 3 exists when q, the grammar's
//   previous token, is a PITCH.  cap = 128, lowered to dhi when dhi >= 1, to 128 - a when w is set and a exists (the note
//   ends by the bar line), and to f when h is set, the sequence's GUIDE word is on and a and k exist: f the smallest m in
//   1 .. 127 such that bit k of the guide's cell row for step a + m is clear (none: the term does not apply).  The cell row
//   of step a + m < 128 is block_i + 1 + ((a + m) >> s), of a later step block_{i+1} + 1 + ((a + m - 128) >> s), with
//   block_x = base_g + (x mod R_g) (1 + C) read off the guide word and every row index clamped to the guide's rows - 1.
//   lo = min(max(dlo, 1), cap); banned are DURATION ids 304 .. 303 + lo - 1 and 304 + cap .. 431.  The window is never empty
//   (a <= 127, f >= 1): where the bar line or the guide leaves less room than dlo the lower bound gives way.  Ids 303 and
//   432 are never touched; step a itself is not tested (that is GDE's pitch ban).
//   The bans apply whatever class is drawn and join the one select of ORD .. GDE, so a draw is bit for bit the GDE kernel's
//   with bias[b] = -inf at these ids; an off word, or a word over a row with dlo = dhi = 0, an all-ones velocity mask and
//   w = h = 0, is bit for bit the GDE kernel.
//   THE LOADS: the row is one wave-uniform 16-byte load whose address needs the record and the control word only; it goes
//   out beside the onset row's and the guide's live row, ahead of the chain.  THE HOLD TERM is the new work: lane l tests
//   m = 1 + l and m = 65 + l (m = 128 is masked out); for each it computes the clamped cell-row index and loads the ONE word
//   table[4 row + (k >> 5)] -- two per-lane vector loads, not a row: the 127 steps ahead touch up to 127 rows of 16 bytes,
//   and a lane needs one bit of each.  The addresses need p (the first ballot of the scan) and the previous token, so the
//   loads go out where the guide's cell row does: behind chunk 0 for a normal bar, behind the chunk loop otherwise (that
//   branch is wave-uniform already).  Two ballots of "clear" give f: the lowest set lane of the first, else 64 + that of the
//   second.  An off word, an off guide word, no a or no k reads row 0 and selects "none clear": no branch on the switches.
//   dlo, dhi, w, h, a, k, f, cap and lo stay in scalar registers; the velocity bits of a lane come from the 64-bit shift ONS
//   and GDE use (ids 131 .. 194 are lanes 10 .. 16, 12 bits span at most two words; lane 10's start bit is negative and it
//   shifts from bit 0 and moves the result up, as GDE's lane 0 does); the duration window is two bit ranges per lane, built
//   like the position range.  No LDS, no scratch.  (As compiled the row is scalar loads in the stand-alone kernel and one
//   uniform-address global_load_dwordx3 in the fused loop kernel, as the onset and guide rows are there; the hold term is
//   four global_load_dword, two at each of its two places: docs/EXPERIMENTS.md 9d.)
//   THE OTHER DESIGN -- a run-length table precomputed on the host, indexed by bar, cell and pitch, so that f is one load --
//   costs 1 MB per 64-bar template and a repack on every change of the guide; it was not built.
//   NOT COVERED: forced tokens and anything a forced position starts; notes inside a prompt; a note forced shorter than dlo
//   (above); an empty velocity mask ends the attempt by Q12, as before (the host refuses to build one); the hold term reads
//   the next bar's block even where the generation length would cut the sequence first; the hold term tests the guide only
//   (harmony across a chord change is not tested).  ART needs GDE.
struct Articulation {
    int ctl;                // the sequence's control as the caller loaded it
    const unsigned* table;  // uint32 [rows][4]
    int rows;               // 1 .. 4096 (the entry points refuse anything else)
};
constexpr int ART_ROWS_MAX = 4096, ART_CYCLE_MAX = 64;
// THE TIER.  The constraints above are strictly nested: each one's kernel is the kernel of the one before it with one more
// input, so a launch is described by how far up this list it goes -- grammar, harmony, class controls, note order, voices,
// density, interval, onsets, guide, articulation, in the order of the enum -- and a tier includes every tier below it.  The
// optional bias is the one free switch: tiers T_NONE and T_GRAM exist with and without it, from T_HARM up there is one
// instantiation and it reads a bias (callers without one pass a zero row, and all-off switches / words for the tiers they
// do not use).  A launch of tier T compiles to the code that never heard of the tiers above T: nothing of their arguments
// is looked at.
enum Tier { T_NONE, T_GRAM, T_HARM, T_CLS, T_ORD, T_VOX, T_DEN, T_MEL, T_ONS, T_GDE, T_ART };
template <bool BIAS, int TIER = T_NONE>
__device__ __forceinline__ int sample_topk_body(int b, int lane, float* __restrict__ logits, int ld, int V,
                                                 const unsigned char* __restrict__ wrong, int ldw,
                                                 const float* __restrict__ uni,
                                                 const unsigned char* __restrict__ active, float temperature,
                                                 int top_k, int* __restrict__ token, float* __restrict__ probs_out,
                                                 int ldp, float top_p, SamplingRows rows, bool want_logp,
                                                 float* __restrict__ logp_out, TokenLogp& lp,
                                                 const float* __restrict__ bias = nullptr, int ld_bias = 0,
                                                 Grammar g = Grammar{nullptr, 0, nullptr, 0, 0, 0},
                                                 Harmony h = Harmony{nullptr, 0, nullptr, 0, 0, 0},
                                                 ClassControls cc = ClassControls{nullptr},
                                                 NoteOrder no = NoteOrder{-1}, Voices vx = Voices{-1},
                                                 Density dn = Density{-1}, Interval ml = Interval{-1},
                                                 Onsets os = Onsets{-1, nullptr, 1, 0},
                                                 Guide gd = Guide{-1, nullptr, 1},
                                                 Articulation ar = Articulation{-1, nullptr, 1}) {
    constexpr bool GRAM = TIER >= T_GRAM, HARM = TIER >= T_HARM, CLS = TIER >= T_CLS, ORD = TIER >= T_ORD, VOX = TIER >= T_VOX,
                   DEN = TIER >= T_DEN, MEL = TIER >= T_MEL, ONS = TIER >= T_ONS, GDE = TIER >= T_GDE, ART = TIER >= T_ART;
    float* lg = logits + (size_t)b * ld;
    // The optional per-sequence inputs -- the active flag and this sequence's controls -- are loaded unconditionally: a null
    // array reads a valid word of this sequence instead (token[b], logits[b][0]), which is then ignored.  So they are in
    // flight together with the loads below; behind a branch per array each was a memory round trip of its own.
    const unsigned char act_row = *(active != nullptr ? active + b : reinterpret_cast<const unsigned char*>(token + b));
    float t_row = 0.f, p_row = 0.f;
    int k_row = 0;
    if constexpr (!CLS) {         // (CLS: the triple is the class record's, loaded below; none of these loads is issued)
        t_row = *(rows.temperature != nullptr ? rows.temperature + b : lg);
        k_row = *(rows.top_k != nullptr ? rows.top_k + b : token + b);
        p_row = *(rows.top_p != nullptr ? rows.top_p + b : lg);
    }
    float p[PER_LANE];
    const int base = lane * PER_LANE;
    // every load of the step up front and unconditional (clamped index): one memory round trip, not one per element
    float raw[PER_LANE];
#pragma unroll
    for (int e = 0; e < PER_LANE; ++e) raw[e] = lg[min(base + e, V - 1)];
    int prev = 0;                 // (GRAM) the last token of seq: every lane loads the same word
    if constexpr (GRAM) prev = g.seq_row[min(max(g.len, 1), g.ld_seq) - 1];
    int otok = 0, olen = 0;       // (ORD) chunk 0 of the backward scan: lane l holds seq[L - 1 - l] (clamped; valid: l < L)
    if constexpr (ORD) {
        olen = min(max(g.len, 0), g.ld_seq);
        otok = g.seq_row[max(olen - 1 - lane, 0)];
    }
    int vt1 = 0, vt2 = 0, vt3 = 0;          // (VOX) the three tokens before the lane's: seq[L - 2 - l], [L - 3 - l], [L - 4 - l]
    if constexpr (VOX) {
        vt1 = g.seq_row[max(olen - 2 - lane, 0)];
        vt2 = g.seq_row[max(olen - 3 - lane, 0)];
        vt3 = g.seq_row[max(olen - 4 - lane, 0)];
    }
    int chord = 0;                // (HARM) the last chord placed, chord_tok[b][F_CUR - 1]: likewise one word for all lanes
    if constexpr (HARM) chord = h.chord_row[min(max(h.cur, 1), h.ld_chord) - 1];
    float bv[PER_LANE];           // (BIAS) this lane's entries of the bias row, in the same batch of loads
    if constexpr (BIAS) {
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) bv[e] = bias[(size_t)b * ld_bias + min(base + e, V - 1)];
    }
    // (GRAM) this lane's entries of the grammar row of the previous token's class: issued as soon as the token is here, so
    // that the rejected-token map and the variate below travel under them
    float gv[PER_LANE];
    if constexpr (GRAM) {
        const int row = __builtin_amdgcn_readfirstlane(g.on != 0 ? token_class(prev) : 7);
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) gv[e] = g.table[(size_t)row * g.ld + min(base + e, V - 1)];
    }
    // (ONS) the open bar's template row, the same for every lane: its address needs the record and the control word only,
    // so the one scalar load goes out beside the grammar row's; an off word reads row 0 and selects all ones
    unsigned or0 = ~0u, or1 = ~0u, or2 = ~0u, or3 = ~0u;
    if constexpr (ONS) {
        const int octl = __builtin_amdgcn_readfirstlane(os.ctl);
        const int obar = max(__builtin_amdgcn_readfirstlane(os.nbar) - 1, 0);
        const int ocyc = min(max(octl >> 12, 1), ONS_CYCLE_MAX);
        const int orow = min(max((octl & (ONS_ROWS_MAX - 1)) + obar % ocyc, 0), os.rows - 1);
        const unsigned* ow = os.table + 4 * (size_t)__builtin_amdgcn_readfirstlane(octl >= 0 ? orow : 0);
        const unsigned w0 = ow[0], w1 = ow[1], w2 = ow[2], w3 = ow[3];
        or0 = octl >= 0 ? w0 : ~0u;
        or1 = octl >= 0 ? w1 : ~0u;
        or2 = octl >= 0 ? w2 : ~0u;
        or3 = octl >= 0 ? w3 : ~0u;
    }
    // (GDE) the open bar's block and its live row: like the onset row's, the address needs the record and the control word
    // only, so this scalar load goes out beside it; the live row is ANDed into the onset words here, ahead of every use (the
    // position ban and the density waiver below see the intersection).  An off word reads row 0 and selects all ones.
    int gctl = -1, gshift = 0, gblock = 0;
    if constexpr (GDE) {
        gctl = __builtin_amdgcn_readfirstlane(gd.ctl);
        const int gbar = max(__builtin_amdgcn_readfirstlane(os.nbar) - 1, 0);
        const int gcyc = min(max((gctl >> 16) & 127, 1), GDE_CYCLE_MAX);
        gshift = (gctl >> 23) & 7;
        gblock = (gctl & (GDE_ROWS_MAX - 1)) + (gbar % gcyc) * (1 + (POS_RES >> gshift));
        const int grow = min(max(gblock, 0), gd.rows - 1);
        const unsigned* gw = gd.table + 4 * (size_t)__builtin_amdgcn_readfirstlane(gctl >= 0 ? grow : 0);
        const unsigned w0 = gw[0], w1 = gw[1], w2 = gw[2], w3 = gw[3];
        or0 &= gctl >= 0 ? w0 : ~0u;
        or1 &= gctl >= 0 ? w1 : ~0u;
        or2 &= gctl >= 0 ? w2 : ~0u;
        or3 &= gctl >= 0 ? w3 : ~0u;
    }
    // (ART) the open bar's articulation row: once more the address needs the record and the control word only, so the one
    // uniform 16-byte load goes out beside the two above (word 3 is reserved and not looked at); an off word reads row 0 and
    // selects no bounds, the all-ones velocity mask and both switches off.  The guide's block of the NEXT bar, which the hold
    // term looks into, is worked out here from the guide word as well.
    int adlo = 0, adhi = 0, abarline = 0, ahold = 0, gblock1 = 0;
    unsigned av0 = ~0u, av1 = ~0u;
    if constexpr (ART) {
        const int actl = __builtin_amdgcn_readfirstlane(ar.ctl);
        const int abar = max(__builtin_amdgcn_readfirstlane(os.nbar) - 1, 0);
        const int acyc = min(max((actl >> 12) & 127, 1), ART_CYCLE_MAX);
        const int arow = min(max((actl & (ART_ROWS_MAX - 1)) + abar % acyc, 0), ar.rows - 1);
        const unsigned* aw = ar.table + 4 * (size_t)__builtin_amdgcn_readfirstlane(actl >= 0 ? arow : 0);
        const unsigned w0 = aw[0], w1 = aw[1], w2 = aw[2];
        adlo = actl >= 0 ? (int)(w0 & 255u) : 0;
        adhi = actl >= 0 ? (int)((w0 >> 8) & 255u) : 0;
        av0 = actl >= 0 ? w1 : ~0u;
        av1 = actl >= 0 ? w2 : ~0u;
        abarline = actl >= 0 ? ((actl >> 19) & 1) : 0;
        ahold = (actl >= 0 && gctl >= 0) ? ((actl >> 20) & 1) : 0;
        const int gcyc = min(max((gctl >> 16) & 127, 1), GDE_CYCLE_MAX);
        gblock1 = (gctl & (GDE_ROWS_MAX - 1)) + ((abar + 1) % gcyc) * (1 + (POS_RES >> gshift));
    }
    // (HARM) the 12 pitch-class values of the chord's row, the same for every lane: element e of a lane is id 12 l + e,
    // MIDI pitch 12 l + e - 3, pitch class (e + 9) mod 12
    float hv[PER_LANE];
    if constexpr (HARM) {
        static_assert(PER_LANE == 12, "a lane's element e has pitch class (e + 9) mod 12 only while it owns 12 consecutive ids");
        const bool is_chord = h.cur >= 1 && chord >= TOK_CHORD_LO && chord <= TOK_CHORD_HI;
        const int row = __builtin_amdgcn_readfirstlane(h.on != 0 ? (is_chord ? chord - TOK_CHORD_LO : HARM_NO_CHORD) : HARM_OFF);
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) hv[e] = h.table[(size_t)row * h.ld + (e + 9) % 12];
    }
    unsigned wmask = 0u;          // the rejected ("wrong") tokens of this lane
    if (wrong != nullptr) {
        unsigned char wb[PER_LANE];
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) wb[e] = wrong[(size_t)b * ldw + min(base + e, V - 1)];
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e)
            if (base + e < V && wb[e] != 0) wmask |= 1u << e;
    }
    const float u = uni != nullptr ? uni[b] : 0.5f;
    // one value per wave, kept in scalar registers so that the mode branches below stay scalar branches
    if constexpr (CLS) {
        // the record of the previous token's class (0 <= c <= 6: row 7 is never picked): a uniform address, one scalar load
        const int c = __builtin_amdgcn_readfirstlane(token_class(prev));
        const int4 crec = cc.table[c];
        temperature = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(crec.x));
        top_k = __builtin_amdgcn_readfirstlane(crec.y);
        top_p = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(crec.z));
    } else {
        if (rows.temperature != nullptr)
            temperature = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t_row)));
        if (rows.top_k != nullptr) top_k = __builtin_amdgcn_readfirstlane(k_row);
        if (rows.top_p != nullptr) top_p = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p_row)));
    }
    // the radix select below needs 1 <= top_k <= V (exactly one lane owns the threshold bin); the host validates the
    // values, the clamp keeps the kernel in bounds whatever an array holds
    top_k = min(max(top_k, 1), V);
    unsigned omask = 0u;          // (ORD) the ids of this lane that the note order bans
    if constexpr (ORD) {
        static_assert(PER_LANE == 12 && ORD_FLAGS % PER_LANE == 0 && ORD_FLAGS > TOK_PITCH_HI && ORD_FLAGS <= 3 * 64, "flag owners");
        __shared__ __attribute__((aligned(16))) int oflag[ORD_FLAGS];
#pragma unroll
        for (int q = 0; q < 3; ++q) oflag[lane + 64 * q] = 0;
        int start = __builtin_amdgcn_readfirstlane(olen) - 1;         // seq index of lane 0 of the chunk
        int pos = 0, n = 0, phase = 0;          // phase 0: looking for j; 1: p known, looking for s; 2: the run is complete
        // (VOX) the ends' histogram, the sounding pitches' flags and the BARs passed in the chunks so far
        int *vflag = nullptr, *vhist = nullptr;
        int nbar = 0;
        int dcount = 0;                         // (DEN) the notes with beta == 0 in the chunks so far
        int mq = 0;                             // (MEL) the reference note's PITCH token, once found
        bool mfound = false;
        unsigned gc0 = ~0u, gc1 = ~0u, gc2 = ~0u, gc3 = ~0u;          // (GDE) the cell row's four words, once loaded
        unsigned hw0 = ~0u, hw1 = ~0u;          // (ART) the lane's two words of the hold term, once loaded
        bool hon = false;                       // (ART) the hold term applies: h, the guide word on, a and k exist
        if constexpr (VOX) {
            static_assert(VOX_BINS == 2 * 64, "two bins per lane");
            __shared__ __attribute__((aligned(16))) int vflag_lds[ORD_FLAGS];
            __shared__ __attribute__((aligned(8))) int vhist_lds[VOX_BINS];
            vflag = vflag_lds;
            vhist = vhist_lds;
#pragma unroll
            for (int q = 0; q < 3; ++q) vflag[lane + 64 * q] = 0;
#pragma unroll
            for (int q = 0; q < VOX_BINS / 64; ++q) vhist[lane + 64 * q] = 0;
        }
        auto chunk = [&](int t, int t1 = 0, int t2 = 0, int t3 = 0) {
            const bool valid = start - lane >= 0;
            const bool brk = valid & ((t == TOK_BAR) | ((unsigned)(t - TOK_POS0) < (unsigned)POS_RES));
            bool ran = false;                   // (VOX) the run was complete before this chunk: none of its lanes is in it
            if constexpr (VOX) ran = phase == 2;
            if (phase == 0) {
                const unsigned long long m = __ballot(brk);
                if (m != 0ull) {
                    pos = __builtin_amdgcn_readlane(t, __builtin_ctzll(m));
                    phase = 1;
                }
            }
            unsigned long long take = ~0ull;    // the lanes of this chunk inside the run
            if (phase == 1) {
                // (a last breaker that is BAR differs from every POSITION token and from no BAR: the first ballot's lane
                // itself answers, the run is empty below it and nothing of it is used)
                const unsigned long long m = __ballot(brk & ((t != pos) | (pos == TOK_BAR)));
                if (m != 0ull) {
                    take = (1ull << __builtin_ctzll(m)) - 1ull;
                    phase = 2;
                }
            }
            if constexpr (VOX) take = ran ? 0ull : take;
            const bool hit = valid & ((unsigned)(t - TOK_PITCH_LO) <= (unsigned)(TOK_PITCH_HI - TOK_PITCH_LO)) &
                             (((take >> lane) & 1ull) != 0ull);
            n += __popcll(__ballot(hit));
            if (hit) oflag[t] = 1;
            if constexpr (VOX) {
                // the lane that holds a note's DURATION sees the note (index start - lane - 3 >= 0: the clamped loads
                // of the lanes below that are not looked at)
                const unsigned long long bars = __ballot(valid & (t == TOK_BAR));
                const int beta = nbar + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bars >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((unsigned)bars, 0u));
                const bool note = (start - lane - 3 >= 0) & ((unsigned)(t - TOK_DUR_LO) <= (unsigned)(TOK_DUR_HI - TOK_DUR_LO)) &
                                  ((unsigned)(t1 - TOK_PITCH_LO) <= (unsigned)(TOK_PITCH_HI - TOK_PITCH_LO)) &
                                  ((unsigned)(t2 - TOK_VEL_LO) <= (unsigned)(TOK_VEL_HI - TOK_VEL_LO)) &
                                  ((unsigned)(t3 - TOK_POS0) < (unsigned)POS_RES) & (beta <= 1);
                const int end = min((t3 - TOK_POS0) + (t - (TOK_DUR_LO - 1)) - POS_RES * beta, POS_RES);
                if (note & (end >= 1)) atomicAdd(&vhist[VOX_BINS - end], 1);
                // (phase 0 here: no breaker down to this chunk's last index, so this note's POSITION is j itself)
                const int g0 = pos == TOK_BAR ? 0 : pos - TOK_POS0;
                if (note & ((phase == 0) | (end > g0))) vflag[t1] = 1;
                if constexpr (DEN) dcount += __popcll(__ballot(note & (beta == 0)));
                if constexpr (MEL) {
                    // (the lowest lane of the ballot is the highest index; a later chunk holds lower indices only)
                    const unsigned long long nm = __ballot(note);
                    if (!mfound && nm != 0ull) {
                        mq = __builtin_amdgcn_readlane(t1, __builtin_ctzll(nm));
                        mfound = true;
                    }
                }
                nbar += __popcll(bars);
            }
            start -= 64;
        };
        // chunk 0 in straight-line code: its load went out beside the previous token's and has long arrived (as compiled
        // the scan starts behind the rejected-token map's wait, which is for every load of the step: what the scan costs is
        // its instructions, not a memory round trip)
        if constexpr (VOX) {
            __builtin_amdgcn_s_waitcnt(0xc07f);  // (the zeroes before the first atomic: one wave, LDS completes in order)
            chunk(otok, vt1, vt2, vt3);
            // (GDE) the cell row of the position the bar is at: its address needs p, which the first ballot of the scan
            // gives -- in chunk 0 for a normal bar, so the scalar load goes out here and travels under the rest of the
            // walk; a row whose last breaker lies further back loads behind the loop (a wave-uniform branch like the
            // loop's own).  No breaker, BAR, or an off word: row 0 is read and all ones selected.
            const auto gcell = [&]() {
                const bool gon = gctl >= 0 && phase != 0 && pos != TOK_BAR;
                const int gstep = min(max(pos - TOK_POS0, 0), POS_RES - 1);
                const int grow = min(max(gblock + 1 + (gstep >> gshift), 0), gd.rows - 1);
                const unsigned* gw = gd.table + 4 * (size_t)__builtin_amdgcn_readfirstlane(gon ? grow : 0);
                const unsigned w0 = gw[0], w1 = gw[1], w2 = gw[2], w3 = gw[3];
                gc0 = gon ? w0 : ~0u;
                gc1 = gon ? w1 : ~0u;
                gc2 = gon ? w2 : ~0u;
                gc3 = gon ? w3 : ~0u;
            };
            // (ART) the hold term's two words per lane: bit k of the guide's cell rows for the steps a + 1 + l and
            // a + 65 + l, the second bar's block past step 127.  The addresses need p and the previous token, so the two
            // vector loads go out with the cell row's.  Off, no a or no k: row 0, word 0, and "none clear" is selected below.
            const auto ghold = [&]() {
                const int hstep = min(max(pos - TOK_POS0, 0), POS_RES - 1), hk = min(max(prev - TOK_PITCH_LO, 0), 127);
                hon = ahold != 0 && phase != 0 && pos != TOK_BAR &&
                      (unsigned)(prev - TOK_PITCH_LO) <= (unsigned)(TOK_PITCH_HI - TOK_PITCH_LO);
                const auto word_of = [&](int m) {
                    const int t = hstep + m;          // (1 .. 254)
                    const int r = t < POS_RES ? gblock + 1 + (t >> gshift) : gblock1 + 1 + ((t - POS_RES) >> gshift);
                    return gd.table[hon ? 4 * (size_t)min(max(r, 0), gd.rows - 1) + (hk >> 5) : 0];
                };
                hw0 = word_of(1 + lane);
                hw1 = word_of(65 + lane);
            };
            bool gearly = false;
            if constexpr (GDE) {
                gearly = phase != 0;
                if (gearly) {
                    gcell();
                    if constexpr (ART) ghold();
                }
            }
            // (the run is complete at the first BAR from the end at the latest: the second BAR, or index 0, ends both)
#pragma unroll 1
            while ((phase != 2 || nbar < 2) && start >= 0)
                chunk(g.seq_row[max(start - lane, 0)], g.seq_row[max(start - lane - 1, 0)],
                      g.seq_row[max(start - lane - 2, 0)], g.seq_row[max(start - lane - 3, 0)]);
            if constexpr (GDE) {
                if (!gearly) {
                    gcell();
                    if constexpr (ART) ghold();
                }
            }
        } else {
            chunk(otok);
#pragma unroll 1
            while (phase != 2 && start >= 0) chunk(g.seq_row[max(start - lane, 0)]);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): one wave, LDS operations complete in order
        const int ctl = __builtin_amdgcn_readfirstlane(no.ctl);
        const bool on = ctl >= 0 && phase != 0 && pos != TOK_BAR;
        int hi = on ? pos + ((ctl >= 1 && n >= ctl) ? 1 : 0) : TOK_POS0;               // positions [432, hi) are banned
        unsigned vdm = 0u;                       // (VOX) the lane's ids among the sounding pitches
        if constexpr (VOX) {
            const int vctl = __builtin_amdgcn_readfirstlane(vx.ctl);
            const int cap = vctl >= 0 ? (vctl & 255) : 0, strike = vctl >= 0 ? ((vctl >> 8) & 1) : 0;
            // lane l holds the bins of the ends 128 - 2l and 127 - 2l: `before` notes end past 128 - 2l, before + h.x past
            // 127 - 2l, incl past 126 - 2l; the count falls with g, so the smallest g that leaves fewer than N is the
            // lowest any lane can offer (none: 128, where the count is 0)
            const int2 hb = *reinterpret_cast<const int2*>(vhist + 2 * lane);
            const int incl = wscan_i(hb.x + hb.y, lane), before = incl - (hb.x + hb.y);
            const int mine = incl < cap ? 126 - 2 * lane : (before + hb.x < cap ? 127 - 2 * lane : POS_RES);
            const int E = cap >= 1 ? wmin_i(mine) : 0;
            hi = max(hi, TOK_POS0 + E);
            const int4* vq = reinterpret_cast<const int4*>(vflag + min(base, ORD_FLAGS - PER_LANE));
#pragma unroll
            for (int q = 0; q < PER_LANE / 4; ++q) {
                const int4 f4 = vq[q];
                vdm |= ((unsigned)f4.x << (4 * q)) | ((unsigned)f4.y << (4 * q + 1)) | ((unsigned)f4.z << (4 * q + 2)) |
                       ((unsigned)f4.w << (4 * q + 3));
            }
            vdm = (strike != 0 && base < ORD_FLAGS) ? vdm : 0u;
        }
        bool dend = false;                       // (DEN) BAR and EOS are banned: the open bar holds fewer notes than asked for
        if constexpr (DEN) {
            static_assert(TOK_EOS < PER_LANE && TOK_BAR < PER_LANE, "lane 0 owns BAR and EOS");
            const int dctl = __builtin_amdgcn_readfirstlane(dn.ctl);
            const int dlo = dctl >= 0 ? (dctl & 255) : 0, dhi = dctl >= 0 ? ((dctl >> 8) & 255) : 0;
            hi = (dhi >= 1 && dcount >= dhi) ? TOK_POS0 + POS_RES : hi;
            // (the waiver: every position is banned already, by the three rules together -- the bar may end)
            dend = dlo >= 1 && dcount < dlo && hi != TOK_POS0 + POS_RES;
            if constexpr (ONS) {
                // (the waiver with a template: a position is left only where the merged range and the row both leave it)
                const int ban = hi - TOK_POS0;                 // grid steps 0 .. ban - 1 are banned by the range
                const auto left = [&](unsigned w, int k) {
                    const int nlow = min(max(ban - 32 * k, 0), 32);
                    return nlow >= 32 ? 0u : (w & ~((1u << nlow) - 1u));
                };
                dend = dlo >= 1 && dcount < dlo && (left(or0, 0) | left(or1, 1) | left(or2, 2) | left(or3, 3)) != 0u;
            }
        }
        // the lane's 12 flags as 16-byte LDS reads, unconditional (the lanes past the flags read the last owner's and
        // drop them), packed into a bit mask without a branch: behind a branch per element they were 12 dependent LDS
        // round trips and some 200 instructions
        const int4* fq = reinterpret_cast<const int4*>(oflag + min(base, ORD_FLAGS - PER_LANE));
        unsigned dm = 0u;
#pragma unroll
        for (int q = 0; q < PER_LANE / 4; ++q) {
            const int4 f4 = fq[q];              // (a flag is 0 or 1)
            dm |= ((unsigned)f4.x << (4 * q)) | ((unsigned)f4.y << (4 * q + 1)) | ((unsigned)f4.z << (4 * q + 2)) |
                  ((unsigned)f4.w << (4 * q + 3));
        }
        const int lo_e = min(max(TOK_POS0 - base, 0), PER_LANE), hi_e = min(max(hi - base, 0), PER_LANE);
        const unsigned pm = ((1u << hi_e) - 1u) & ~((1u << lo_e) - 1u);          // (empty while hi <= 432)
        omask = pm | ((on && base < ORD_FLAGS) ? dm : 0u);
        if constexpr (VOX) omask |= vdm;
        if constexpr (DEN) omask |= (dend && base == 0) ? ((1u << TOK_EOS) | (1u << TOK_BAR)) : 0u;
        if constexpr (MEL) {
            const int mctl = __builtin_amdgcn_readfirstlane(ml.ctl);
            const bool mon = mctl >= 0 && mfound;
            const int mup = mon ? (mctl & 255) : 0, mdown = mon ? ((mctl >> 8) & 255) : 0;
            // ids [ulo, 131) and [3, dhi) are banned (empty where the bound is not set or reaches past the pitch range)
            const int ulo = mup >= 1 ? min(mq + mup + 1, TOK_PITCH_HI + 1) : TOK_PITCH_HI + 1;
            const int dhi = mdown >= 1 ? max(mq - mdown, TOK_PITCH_LO) : TOK_PITCH_LO;
            const int same = (mon && ((mctl >> 16) & 1) != 0) ? mq : -1;          // (the one id of the unison ban)
            const int u0 = min(max(ulo - base, 0), PER_LANE), u1 = min(max(TOK_PITCH_HI + 1 - base, 0), PER_LANE);
            const int d0 = min(max(TOK_PITCH_LO - base, 0), PER_LANE), d1 = min(max(dhi - base, 0), PER_LANE);
            omask |= ((1u << u1) - 1u) & ~((1u << u0) - 1u);
            omask |= ((1u << d1) - 1u) & ~((1u << d0) - 1u);
            omask |= (unsigned)(same - base) < (unsigned)PER_LANE ? 1u << (same - base) : 0u;
        }
        if constexpr (ONS) {
            // the lane's 12 bits of the row start at grid step g0 = base - 432 (lanes 36 .. 46: 0, 12, .. 120) and span at most
            // two words; lanes that own no position id have an empty range below and what they shift is dropped
            const int g0 = base - TOK_POS0;
            const int w = (g0 >> 5) & 3;
            const unsigned wlo = w == 0 ? or0 : (w == 1 ? or1 : (w == 2 ? or2 : or3));
            const unsigned whi = w == 0 ? or1 : (w == 1 ? or2 : (w == 2 ? or3 : 0u));
            const unsigned may = (unsigned)(((((unsigned long long)whi) << 32) | wlo) >> (g0 & 31));
            const int p0 = min(max(TOK_POS0 - base, 0), PER_LANE), p1 = min(max(TOK_POS0 + POS_RES - base, 0), PER_LANE);
            omask |= ~may & (((1u << p1) - 1u) & ~((1u << p0) - 1u));
        }
        if constexpr (GDE) {
            // the lane's 12 bits of the cell row start at pitch bit k0 = base - 3 (lanes 0 .. 10: -3, 9, .. 117) and span at
            // most two words; lane 0 shifts from bit 0 and moves the result up by 3 -- ids 0 .. 2 are outside the range
            // below -- and lane 10's bit 11 (id 131, a velocity) is outside it too; lanes past 10 have an empty range
            const int k0 = base - TOK_PITCH_LO, kk = max(k0, 0);
            const int w = (kk >> 5) & 3;
            const unsigned wlo = w == 0 ? gc0 : (w == 1 ? gc1 : (w == 2 ? gc2 : gc3));
            const unsigned whi = w == 0 ? gc1 : (w == 1 ? gc2 : (w == 2 ? gc3 : 0u));
            const unsigned may = (unsigned)(((((unsigned long long)whi) << 32) | wlo) >> (kk & 31)) << (kk - k0);
            const int p0 = min(max(TOK_PITCH_LO - base, 0), PER_LANE), p1 = min(max(TOK_PITCH_HI + 1 - base, 0), PER_LANE);
            omask |= ~may & (((1u << p1) - 1u) & ~((1u << p0) - 1u));
        }
        if constexpr (ART) {
            // the hold term: lane l holds the steps m = 1 + l and m = 65 + l (lane 63's second is m = 128, masked out); f is
            // the lowest clear one, 128 where none is -- which lowers no cap
            const int hb = min(max(prev - TOK_PITCH_LO, 0), 127) & 31;
            const unsigned long long c0 = __ballot(hon & (((hw0 >> hb) & 1u) == 0u));
            const unsigned long long c1 = __ballot(hon & (((hw1 >> hb) & 1u) == 0u)) & ~(1ull << 63);
            const int f = c0 != 0ull ? 1 + __builtin_ctzll(c0) : (c1 != 0ull ? 65 + __builtin_ctzll(c1) : POS_RES);
            const bool aex = phase != 0 && pos != TOK_BAR;
            int cap = adhi >= 1 ? min(adhi, POS_RES) : POS_RES;
            cap = (abarline != 0 && aex) ? min(cap, POS_RES - min(max(pos - TOK_POS0, 0), POS_RES - 1)) : cap;
            cap = min(cap, f);
            const int dlo1 = min(max(adlo, 1), cap);
            // DURATION ids [304, 303 + lo) and [304 + cap, 432) are banned: two bit ranges per lane
            const int s0 = min(max(TOK_DUR_LO - base, 0), PER_LANE), s1 = min(max(TOK_DUR_LO - 1 + dlo1 - base, 0), PER_LANE);
            const int l0 = min(max(TOK_DUR_LO + cap - base, 0), PER_LANE), l1 = min(max(TOK_DUR_HI + 1 - base, 0), PER_LANE);
            omask |= ((1u << s1) - 1u) & ~((1u << s0) - 1u);
            omask |= ((1u << l1) - 1u) & ~((1u << l0) - 1u);
            // the lane's 12 bits of the velocity mask start at bit k0 = base - 131 (lanes 10 .. 16: -11, 1, .. 61) and span at
            // most two words; lane 10 shifts from bit 0 and moves the result up by 11 -- ids 120 .. 130 are outside the range
            // below -- and lane 16's bits past 63 (ids 195 ..) are outside it too
            const int k0 = base - TOK_VEL_LO, kk = min(max(k0, 0), 63);
            const unsigned wlo = (kk >> 5) == 0 ? av0 : av1;
            const unsigned whi = (kk >> 5) == 0 ? av1 : 0u;
            const unsigned may = (unsigned)(((((unsigned long long)whi) << 32) | wlo) >> (kk & 31)) << min(max(kk - k0, 0), 31);
            const int v0 = min(max(TOK_VEL_LO - base, 0), PER_LANE), v1 = min(max(TOK_VEL_HI + 1 - base, 0), PER_LANE);
            omask |= ~may & (((1u << v1) - 1u) & ~((1u << v0) - 1u));
        }
    }
    if (active != nullptr && act_row == 0) return -2;
    // ---- calc_probs
    float lmx = 0.f, lsum = 1.f;          // (want_logp) max and sum of exp(x - max) over ids 1 .. V-1 of the row drawn from
    if (temperature == 0.f) {
        float best = -INFINITY;
        int bi = V;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            const int id = base + e;
            if constexpr (BIAS) raw[e] += bv[e];               // greedy writes nothing back: the row drawn from is y
            if constexpr (GRAM) raw[e] += gv[e];
            if constexpr (HARM) raw[e] = (id >= TOK_PITCH_LO && id <= TOK_PITCH_HI) ? raw[e] + hv[e] : raw[e];
            if constexpr (ORD) raw[e] = ((omask >> e) & 1u) ? -INFINITY : raw[e];
            if (id >= 1 && id < V && raw[e] > best) { best = raw[e]; bi = id; }
        }
        const float wbest = wmax_f(best);                      // ties: the lowest id
        bi = wmin_i(best == wbest ? bi : V);
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) p[e] = (base + e == bi) ? 1.f : 0.f;
        if (want_logp) {                                       // greedy has no softmax: its own max / sum pass
            float sg = 0.f;
#pragma unroll
            for (int e = 0; e < PER_LANE; ++e) {
                const int id = base + e;
                sg += (id >= 1 && id < V) ? expf(raw[e] - wbest) : 0.f;
            }
            lmx = wbest;
            lsum = wsum_f(sg);
        }
    } else {
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            const int id = base + e;
            const bool in = id >= 1 && id < V;
            const float x = in ? raw[e] / temperature : -INFINITY;
            if (in) lg[id] = x;                 // in-place division: compounds on a redo (Q5)
            float y = x;
            if constexpr (BIAS) y = in ? x + bv[e] : -INFINITY;          // (the bias is not written back)
            if constexpr (GRAM) y = in ? y + gv[e] : -INFINITY;          // (nor the grammar row)
            if constexpr (HARM) y = (id >= TOK_PITCH_LO && id <= TOK_PITCH_HI) ? y + hv[e] : y;      // (nor the chord's)
            if constexpr (ORD) y = ((omask >> e) & 1u) ? -INFINITY : y;                                 // (nor the bans)
            p[e] = y;
            mx = fmaxf(mx, y);
        }
        mx = wmax_f(mx);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            p[e] = (p[e] == -INFINITY) ? 0.f : expf(p[e] - mx);
            s += p[e];
        }
        s = wsum_f(s);
        lmx = mx;
        lsum = s;
        const float inv = 1.f / s;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) p[e] *= inv;
    }
    // ---- apply_sampling: top-k (ties: lowest id first).  Probabilities are >= 0, so their bit patterns order like the
    // values: the k-th largest key is found by a radix select, most significant byte first -- per byte one 256-bin
    // histogram of the remaining candidates in LDS, then the bin in which the count from the top reaches k (4 bins per
    // lane, one DPP scan) -- four passes instead of the 32 bit-by-bit counting rounds of the previous version (4.8 us of
    // the step's 8.2); elements equal to the threshold are admitted in id order until k are kept.
    unsigned keep = 0u;
    {
        __shared__ int hist[256];
        unsigned key[PER_LANE];
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) key[e] = (base + e < V) ? __float_as_uint(p[e]) : 0u;
        unsigned thr = 0u, known = 0u;          // bytes of the threshold found so far / mask of those bytes
        int krem = top_k;                        // rank (from the largest) of the threshold among the remaining candidates
#pragma unroll 1
        for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
            for (int q = 0; q < 4; ++q) hist[lane * 4 + q] = 0;
            __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): one wave, LDS operations complete in order
#pragma unroll
            for (int e = 0; e < PER_LANE; ++e)
                if (base + e < V && ((key[e] ^ thr) & known) == 0u) atomicAdd(&hist[(key[e] >> shift) & 255u], 1);
            __builtin_amdgcn_s_waitcnt(0xc07f);
            // lane l owns bins 255 - 4 l ... 252 - 4 l: lane order = descending bin order
            int h[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { h[q] = hist[255 - 4 * lane - q]; tot += h[q]; }
            const int incl = wscan_i(tot, lane), before = incl - tot;
            const bool mine = before < krem && krem <= incl;          // exactly one lane
            int bin = 0, above = 0;
            if (mine) {
                int c = before;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (c < krem && krem <= c + h[q]) { bin = 255 - 4 * lane - q; above = c; }
                    c += h[q];
                }
            }
            const int src = __builtin_ctzll(__ballot(mine));
            bin = __builtin_amdgcn_readlane(bin, src);
            above = __builtin_amdgcn_readlane(above, src);
            thr |= (unsigned)bin << shift;
            known |= 255u << shift;
            krem -= above;
        }
        int ngt = 0, neq_lane = 0;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            ngt += __popcll(__ballot(key[e] > thr));
            neq_lane += (key[e] == thr && base + e < V) ? 1 : 0;
        }
        // exclusive prefix of the per-lane tie counts in lane (= id) order
        const int incl = wscan_i(neq_lane, lane);
        int rank = incl - neq_lane;
        const int room = top_k - ngt;          // ties admitted
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            if (key[e] > thr) keep |= 1u << e;
            else if (key[e] == thr && base + e < V) {
                if (rank < room) keep |= 1u << e;
                ++rank;
            }
        }
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < PER_LANE; ++e) {
        const int id = base + e;
        const bool k = (((keep & ~wmask) >> e) & 1u) && id < V;
        p[e] = k ? p[e] : 0.f;
        s += p[e];
    }
    const float tot = wsum_f(s);
    if (!(tot > 0.f)) {                          // NaN / zero mass: the reference's multinomial raises
        if (lane == 0) token[b] = -1;
        if (probs_out != nullptr)
            for (int e = 0; e < PER_LANE; ++e)
                if (base + e < V) probs_out[(size_t)b * ldp + base + e] = NAN;
        if (want_logp) {
            lp.full = lp.kept = NAN;
            if (logp_out != nullptr && lane == 0) logp_out[2 * b] = logp_out[2 * b + 1] = NAN;
        }
        return -1;
    }
    const float inv = 1.f / tot;
    float ls = 0.f;
#pragma unroll
    for (int e = 0; e < PER_LANE; ++e) { p[e] *= inv; ls += p[e]; }
    // ---- nucleus ("top-p") filter, an extra mode the reference does not have (top_p >= 1: off).  Applied to the
    // distribution left by the top-k / rejected-token step: in order of decreasing probability (ties: lowest id first) a
    // token is kept while the mass BEFORE it is < top_p; the survivors are renormalised.  The smallest kept probability
    // v* is the largest threshold t with mass{p >= t} >= top_p: the same bitwise search as the top-k threshold, on masses.
    if (top_p < 1.f) {
        unsigned key[PER_LANE];
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) key[e] = (base + e < V) ? __float_as_uint(p[e]) : 0u;
        unsigned thr = 0u;
        for (int bit = 30; bit >= 0; --bit) {          // (p <= 1: bit 31 is never set)
            const unsigned cand = thr | (1u << bit);
            float m = 0.f;
#pragma unroll
            for (int e = 0; e < PER_LANE; ++e) m += key[e] >= cand ? p[e] : 0.f;
            if (wsum_f(m) >= top_p) thr = cand;
        }
        float mg = 0.f;
        int neq_lane = 0;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            mg += key[e] > thr ? p[e] : 0.f;
            neq_lane += (thr != 0u && key[e] == thr) ? 1 : 0;
        }
        mg = wsum_f(mg);
        const int incl_t = wscan_i(neq_lane, lane);
        const int nties = __builtin_amdgcn_readlane(incl_t, 63);
        int room = 0;          // ties admitted, in id order: the smallest r >= 1 with mg + r v* >= top_p
        if (thr != 0u) room = max(1, min(nties, (int)ceilf((top_p - mg) / __uint_as_float(thr))));
        int rank = incl_t - neq_lane;
        float s2 = 0.f;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) {
            bool k = key[e] > thr;
            if (thr != 0u && key[e] == thr) { k = rank < room; ++rank; }
            p[e] = k ? p[e] : 0.f;
            s2 += p[e];
        }
        const float inv2 = 1.f / wsum_f(s2);
        ls = 0.f;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e) { p[e] *= inv2; ls += p[e]; }
    }
    if (probs_out != nullptr)
        for (int e = 0; e < PER_LANE; ++e)
            if (base + e < V) probs_out[(size_t)b * ldp + base + e] = p[e];
    // ---- infer_token: smallest id with cdf[id] > u
    const float incl = wscan_f(ls, lane);
    const float excl = incl - ls;
    int cand = 1 << 30;
    float c = excl;
#pragma unroll
    for (int e = 0; e < PER_LANE; ++e) {
        c += p[e];
        if (p[e] > 0.f && c > u && cand == (1 << 30)) cand = base + e;
    }
    // fall-back for u above the accumulated total (rounding): the last token with mass
    int last = -1;
#pragma unroll
    for (int e = 0; e < PER_LANE; ++e)
        if (p[e] > 0.f) last = base + e;
    cand = wmin_i(cand);
    last = wmax_i(last);
    const int drawn = (cand == (1 << 30)) ? last : cand;
    if (lane == 0) token[b] = drawn;
    if (want_logp) {
        // the drawn id's logit and its entry of the distribution, from the lane that owns the id; the row's entry is the
        // division repeated (the value written back above)
        float xd = 0.f, pd = 0.f;
#pragma unroll
        for (int e = 0; e < PER_LANE; ++e)
            if (base + e == drawn) { xd = raw[e]; pd = p[e]; }
        const int owner = max(drawn, 0) / PER_LANE;
        xd = lane_f(xd, owner);
        pd = lane_f(pd, owner);
        if (temperature != 0.f) {
            xd = xd / temperature;
            if constexpr (BIAS) {                  // y at the drawn id, as the softmax above saw it
                float bd = 0.f;
#pragma unroll
                for (int e = 0; e < PER_LANE; ++e)
                    if (base + e == drawn) bd = bv[e];
                xd += lane_f(bd, owner);
            }
            if constexpr (GRAM) {
                float gd = 0.f;
#pragma unroll
                for (int e = 0; e < PER_LANE; ++e)
                    if (base + e == drawn) gd = gv[e];
                xd += lane_f(gd, owner);
            }
            if constexpr (HARM) {
                float hd = 0.f;
#pragma unroll
                for (int e = 0; e < PER_LANE; ++e)
                    if (base + e == drawn) hd = hv[e];
                hd = lane_f(hd, owner);
                xd = (drawn >= TOK_PITCH_LO && drawn <= TOK_PITCH_HI) ? xd + hd : xd;
            }
        }
        lp.full = drawn < 0 ? NAN : (xd - lmx) - logf(lsum);
        lp.kept = drawn < 0 ? NAN : (temperature == 0.f ? 0.f : logf(pd));
        if (logp_out != nullptr && lane == 0) { logp_out[2 * b] = lp.full; logp_out[2 * b + 1] = lp.kept; }
    }
    return drawn;
}


// ------------------------------------------------------------------------------------------------ forcing rules

// field indices of the int32 state record (commu_forcing_state_ints() ints per sequence)
enum {
    F_LEN = 0,      // tokens in seq
    F_FORCED,       // token to feed next iteration, -1: none  (next_tokens_forced holds at most one token)
    F_REDO,         // no_sequence_appended: draw again from the current logits
    F_FIRST,        // first model step after the context: its memory is discarded
    F_FILLED,       // incomplete_filled
    F_DONE,
    F_FAILED,       // nothing could be drawn (Q12)
    F_ITERS,
    F_NBAR,         // seq.count(BAR)
    F_NCHORD,       // chord_length
    F_CUR,          // chords consumed so far
    F_LENGTH_FIT,   // chord_length == int(num_measures // 4 * 4)
    F_NDRAW,        // uniform variates consumed
    F_NTRACE,       // model steps recorded
    F_COUNT
};

// The state record of a sequence as registers of lane 0: loaded with one batch of loads, stored back once (the record's
// fields are read and written many times by the transitions; through memory every access after a store is a round trip).
__device__ __forceinline__ void record_load(int (&r)[F_COUNT], const int* st, int b) {
#pragma unroll
    for (int f = 0; f < F_COUNT; ++f) r[f] = st[(size_t)b * F_COUNT + f];
}
__device__ __forceinline__ void record_store(const int (&r)[F_COUNT], int* st, int b) {
#pragma unroll
    for (int f = 0; f < F_COUNT; ++f) st[(size_t)b * F_COUNT + f] = r[f];
}

// FORM (Form: one int32 control per sequence, -1 off, else base + 4096 R with R in 1 .. 64 the form's bars and base in
//   0 .. 4095, base + R <= rows; table uint32 [rows][4], 1 <= rows <= 4096; the slot's state row of FS_COUNT ints, form.h):
//   a bar the loop opens may REPLAY an earlier bar of its own sequence.  Row base + i is bar i of the form, bars from R on
//   (and from the 64th on) are free: the form is not cycled.  Word 0 is src | copy << 6 | (transpose + 64) << 8 with src in
//   0 .. 63, copy 0 (all) or 1 (rhythm) and transpose in -48 .. 48; 0 is a free bar (a replay row's bits 8 .. 14 are never
//   0).  Words 1 .. 3 are reserved, written 0 by the host and never read.  A row whose src is not below its own bar is
//   treated as free, whatever the table holds; the row index is clamped to rows - 1.
//   The rule lives in the forcing stage, not in the sampler: where `pre` would draw and the slot is inside a replay bar, the
//   next token of the source bar's next complete note group (POSITION, VELOCITY, PITCH, DURATION) is handed to `post` through
//   form_tok[b] as if it had been drawn -- draw[b] stays 0, so the sampling stage skips the slot, no variate is consumed and
//   the logits are not divided -- and `post` runs every rule it has on it (a position past a pending chord forces the chord's
//   position and the token is offered again, BAR with chords left inside the bar forces the next chord's position, BAR with
//   none left forces EOS).  When the source bar has no group left the replay token is BAR.  In rhythm mode the PITCH is a
//   normal draw under every constraint the slot has.  Chord tokens are never copied.
//   THE SEARCH is the wave's work: lane l looks at seq[cursor + l + 64 c .. + 3] with clamped, unconditional loads, one
//   ballot per chunk gives g, and chunk c is taken only while cursor + 64 c + 3 < end: the trip count is wave-uniform.  The
//   token at g + k comes from the finding lane by v_readlane.  No LDS.  Lane 0 keeps the header in registers (FormRegs)
//   through post and pre, as it keeps the record; bar_at is read and written in memory, by lane 0 only.
//   A TAKE ROW (bit 7 of word 0 set: src | copy << 6 | 1 << 7 | (transpose + 64) << 8) replays a bar of a finished sequence
//   the caller supplied: its source is form_src[begin .. end) (words 1 and 2: the first index behind the source bar's BAR and
//   the index of the take's next BAR or end; src is kept for the checker, word 3 stays reserved) instead of a stretch of
//   seq[b].  Such a bar is a replay bar whatever its index, bar 0 included; cursor = clamp(begin, 0, form_src_len), end =
//   clamp(end, cursor, form_src_len); without a buffer, with form_src_len < 4 or with begin >= end the row is free.  The
//   search reads form_src clamped to form_src_len - 1; everything behind the four tokens is the same code.
//   NOT COVERED: replayed tokens are not checked against any constraint, as forced tokens are not; a replay bar cut by the
//   iteration cap or ld_seq is not completed; bars past the 64th are free; a source note that the bar line cut does not
//   appear (g + 3 < end).
struct Form {
    int ctl;                // the sequence's control as the caller loaded it
    const unsigned* table;  // uint32 [rows][4]
    int rows;               // 1 .. 4096 (the entry points refuse anything else)
    int* state;             // the sequence's row of form_state
    int* tok;               // form_tok + b: `pre` writes the replay token (-1: none) ...
    int tokv;               // ... and `post` gets the value the caller loaded
    const int* src;         // (optional) the take buffer int32 [src_len]: the tokens of every take, one behind the other
    int src_len;
};
struct FormRegs {
    int active, cursor, end, k, row, g;
};
__device__ __forceinline__ void form_regs_load(FormRegs& f, const int* fs) {
    f.active = fs[FS_ACTIVE]; f.cursor = fs[FS_CURSOR]; f.end = fs[FS_END]; f.k = fs[FS_K]; f.row = fs[FS_ROW]; f.g = fs[FS_G];
}
__device__ __forceinline__ void form_regs_store(const FormRegs& f, int* fs) {
    fs[FS_ACTIVE] = f.active; fs[FS_CURSOR] = f.cursor; fs[FS_END] = f.end; fs[FS_K] = f.k; fs[FS_ROW] = f.row; fs[FS_G] = f.g;
}
// (lane 0) a BAR was appended at `index` as the (nb + 1)-th of the sequence: record it, and open bar nb under its row
__device__ __forceinline__ void form_bar(const Form& fm, FormRegs& f, int nb, int index) {
    if (nb >= 0 && nb < FORM_BARS) fm.state[FS_BAR_AT + nb] = index;
    const int bars = min((fm.ctl >> 12) & 127, FORM_BARS);
    const bool on = fm.ctl >= 0 && nb >= 0 && nb < bars;
    const int r = min(max((fm.ctl & (FORM_ROWS_MAX - 1)) + (on ? nb : 0), 0), fm.rows - 1);
    const unsigned w = fm.table[4 * (size_t)(on ? r : 0)];
    const int src = (int)(w & 63u);
    const bool row = on && ((w >> 8) & 127u) != 0u;
    // a TAKE row (bit 7): the source bar is form_src[begin .. end), words 1 and 2, whatever nb is; free without a buffer, with
    // one too short for a group or with begin >= end.  Words 1 .. 3 of any other row are not read.
    const bool take = row && (w & 128u) != 0u;
    const int n = fm.src != nullptr ? fm.src_len : 0;
    int tb = 0, te = 0;
    if (take) {
        tb = (int)fm.table[4 * (size_t)r + 1];
        te = (int)fm.table[4 * (size_t)r + 2];
    }
    const bool tak = take && n >= 4 && tb < te;
    const int tc = min(max(tb, 0), n);
    const bool own = row && !take && src < nb;
    const bool rep = own || tak;
    // (field by field, selects: an aggregate assignment behind the branch left two of the fields in scratch)
    const int from = fm.state[FS_BAR_AT + (own ? src : 0)], to = fm.state[FS_BAR_AT + (own ? src + 1 : 0)];
    f.active = rep ? 1 : 0;
    f.cursor = own ? from + 1 : (tak ? tc : 0);
    f.end = own ? (src + 1 == nb ? index : to) : (tak ? min(max(te, tc), n) : 0);
    f.k = 0;
    f.row = rep ? (int)(w & 0x7fffu) : 0;
    f.g = -1;
}
__device__ __forceinline__ bool form_is_group(int t0, int t1, int t2, int t3) {
    return ((unsigned)(t0 - TOK_POS0) < (unsigned)POS_RES) & ((unsigned)(t1 - TOK_VEL_LO) <= (unsigned)(TOK_VEL_HI - TOK_VEL_LO)) &
           ((unsigned)(t2 - TOK_PITCH_LO) <= (unsigned)(TOK_PITCH_HI - TOK_PITCH_LO)) &
           ((unsigned)(t3 - TOK_DUR_LO) <= (unsigned)(TOK_DUR_HI - TOK_DUR_LO));
}
// (the wave) the smallest g >= cursor with g + 3 < end whose four tokens are a note group, -1: none; tk: seq[g + k].
// cursor, end and k are wave-uniform; so are sq and ld_seq, which are the take buffer and its length inside a take's bar.
__device__ __forceinline__ int form_search(const int* __restrict__ sq, int ld_seq, int cursor, int end, int k, int lane, int& tk) {
    int g = -1;
    tk = -1;
    cursor = max(cursor, 0);
    end = min(end, ld_seq);
#pragma unroll 1
    for (int base = cursor; base + 3 < end; base += 64) {
        const int i = base + lane;
        const int t0 = sq[min(i, ld_seq - 1)], t1 = sq[min(i + 1, ld_seq - 1)], t2 = sq[min(i + 2, ld_seq - 1)],
                  t3 = sq[min(i + 3, ld_seq - 1)];
        const unsigned long long m = __ballot((i + 3 < end) & form_is_group(t0, t1, t2, t3));
        if (m != 0ull) {
            const int l = __builtin_ctzll(m);
            g = base + l;
            tk = __builtin_amdgcn_readlane(k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? t2 : t3)), l);
            break;
        }
    }
    return g;
}
// (lane 0) the replay token of a slot inside a replay bar, -1: a normal draw is made (rhythm mode at the pitch)
__device__ __forceinline__ int form_token(const FormRegs& f, int g, int tk) {
    if (g < 0) return TOK_BAR;
    const bool rhythm = ((f.row >> 6) & 1) != 0;
    if (f.k != 2) return tk;
    if (rhythm) return -1;
    const int s = ((f.row >> 8) & 127) - 64;
    int m = tk - TOK_PITCH_LO + s;
    while (m < 0) m += 12;
    while (m > 127) m -= 12;
    return m + TOK_PITCH_LO;
}

template <bool FORM = false>
__device__ __forceinline__ void forcing_pre_body(int b, int lane, int (&s)[F_COUNT], int* seq, int ld_seq,
                                                 const int* __restrict__ chord_tok, const int* __restrict__ chord_pos,
                                                 int ld_chord, unsigned char* wrong, const float* __restrict__ utable,
                                                 int ld_u, int max_iters, long long* tok, unsigned char* active,
                                                 unsigned char* keep, unsigned char* draw, float* uni, int* trace,
                                                 int ld_trace, float* seq_logp,
                                                 Form fm = Form{-1, nullptr, 1, nullptr, nullptr, -1},
                                                 FormRegs* fr = nullptr) {
    int* sq = seq + (size_t)b * ld_seq;
    int clear = 0;
    int fg = -1, ftk = -1;        // (FORM) the source bar's next group and its token of the current phase
    if constexpr (FORM) {
        // the search runs ahead of the decision, for a slot inside a replay bar that has no token to feed: what it reads
        // (cursor, end, k) changes in this stage only where nothing is drawn afterwards
        const bool look = fr->active != 0 && s[F_FORCED] < 0 && !s[F_DONE];
        if (__builtin_amdgcn_readfirstlane((int)look)) {
            // (the open bar's row says where its source lies: lane 0's word, so pointer, bound and trip count stay uniform)
            const bool take = (__builtin_amdgcn_readfirstlane(fr->row) & 128) != 0 && fm.src != nullptr && fm.src_len >= 1;
            fg = form_search(take ? fm.src : sq, take ? fm.src_len : ld_seq, __builtin_amdgcn_readfirstlane(fr->cursor),
                             __builtin_amdgcn_readfirstlane(fr->end), __builtin_amdgcn_readfirstlane(fr->k), lane, ftk);
        }
    }
    if (lane == 0) {
        int act = 0, kp = 0, dr = 0;
        int ft = -1;              // (FORM) the replay token handed to post
        long long t = 0;
        const int len = s[F_LEN];
        const int last = sq[len - 1], prev = len >= 2 ? sq[len - 2] : -1;
        if (!s[F_DONE] && (s[F_ITERS] >= max_iters || last == TOK_EOS || len >= ld_seq)) s[F_DONE] = 1;
        if (!s[F_DONE]) {
            s[F_ITERS] += 1;
            if (s[F_FORCED] >= 0) {                                     // midi_inferrer.py:247-251
                const int f = s[F_FORCED];
                s[F_FORCED] = -1;
                sq[len] = f;
                if (seq_logp != nullptr) {                              // a forced token was not drawn
                    float* q = seq_logp + 2 * ((size_t)b * ld_seq + len);
                    q[0] = q[1] = NAN;
                }
                s[F_LEN] = len + 1;
                if constexpr (FORM) {
                    if (f == TOK_BAR) form_bar(fm, *fr, s[F_NBAR], len);
                }
                if (f == TOK_BAR) s[F_NBAR] += 1;
                t = f; act = 1; kp = 1;
            } else {
                if (s[F_REDO]) {                                        // :253-255
                    s[F_REDO] = 0;
                } else if (s[F_FIRST]) {                                // :256-258
                    s[F_FIRST] = 0;
                    t = last; act = 1; kp = 0;
                } else {                                                // :259-260
                    t = last; act = 1; kp = 1;
                }
                if (!s[F_FILLED]) s[F_FILLED] = s[F_NBAR] > 1;          // :267-268
                const int cur = s[F_CUR];
                const bool remnant = cur < s[F_NCHORD];
                bool decided = false;
                if (s[F_FILLED] && last == TOK_BAR) {                   // :271-273
                    s[F_FORCED] = TOK_POS0;
                    decided = true;
                } else if (remnant && s[F_FILLED]) {                    // :276-283
                    const int cp = chord_pos[(size_t)b * ld_chord + cur];
                    const bool posfit = prev == TOK_BAR && last == TOK_POS0;
                    const bool due = s[F_LENGTH_FIT] ? posfit : (posfit || (last == cp && cp != TOK_POS0));
                    if (due) {
                        s[F_FORCED] = chord_tok[(size_t)b * ld_chord + cur];
                        s[F_CUR] = cur + 1;
                        clear = 1;
                        decided = true;
                        if constexpr (FORM) {                           // the chord took the replayed position: the group starts over
                            if (fr->active && fr->k == 1) fr->k = 0;
                        }
                    }
                }
                if constexpr (FORM) {
                    if (!decided && fr->active) {
                        fr->g = fg;
                        ft = form_token(*fr, fg, ftk);
                        decided = ft >= 0;                              // (no variate, draw[b] stays 0)
                    }
                }
                if (!decided) {
                    dr = 1;
                    const int nd = s[F_NDRAW];
                    uni[b] = utable[(size_t)b * ld_u + (nd < ld_u ? nd : ld_u - 1)];
                    s[F_NDRAW] = nd + 1;
                }
            }
            if (act && trace != nullptr) {
                const int nt = s[F_NTRACE];
                if (2 * nt + 1 < ld_trace) {
                    trace[(size_t)b * ld_trace + 2 * nt] = (int)t;
                    trace[(size_t)b * ld_trace + 2 * nt + 1] = kp;
                }
                s[F_NTRACE] = nt + 1;
            }
        }
        tok[b] = t;
        active[b] = (unsigned char)act;
        keep[b] = (unsigned char)kp;
        draw[b] = (unsigned char)dr;
        if constexpr (FORM) *fm.tok = ft;
    }
    clear = __builtin_amdgcn_readfirstlane(clear);
    if (clear)
        for (int i = lane; i < VOCAB; i += 64) wrong[(size_t)b * VOCAB + i] = 0;
}

// token_val: the token drawn this iteration when the caller has it in a register (>= -1), else (-3) it is read from token[b]
// seq_logp (optional, fp32 [B][ld_seq][2] parallel to seq): an appended draw's log-probability pair goes to the token's
// index -- `lp` with a register token, else logp[b][0:2] (null: NaN); a draw that is not appended leaves no entry
// flags (optional): draw[b], keep[b] and klen[b] as the caller loaded them ahead of the stage (the fused launch has them in
// flight under the sampling step; read here they are three dependent memory round trips)
struct StepFlags {
    int draw, keep, klen;
};
template <bool FORM = false>
__device__ __forceinline__ void forcing_post_body(int b, int lane, int (&s)[F_COUNT], int* seq, int ld_seq,
                                                  const int* __restrict__ chord_pos, int ld_chord, unsigned char* wrong,
                                                  const unsigned char* draw, const int* token, int* live, int* klen,
                                                  const unsigned char* keep, int lmax, int token_val, TokenLogp lp,
                                                  const float* logp, float* seq_logp, const StepFlags* flags = nullptr,
                                                  Form fm = Form{-1, nullptr, 1, nullptr, nullptr, -1},
                                                  FormRegs* fr = nullptr) {
    int clear = 0;
    if (lane == 0) {
        // memory length of the step that just ran: it grows unless the step's memory is discarded (quirk Q3)
        if (klen != nullptr) {
            const int kp = flags != nullptr ? flags->keep : (int)keep[b];
            if (kp) {
                const int kl = flags != nullptr ? flags->klen : klen[b];
                if (kl < lmax - 1) klen[b] = kl + 1;
            }
        }
        bool drew = flags != nullptr ? flags->draw : (int)draw[b];
        if constexpr (FORM) drew = drew || fm.tokv >= 0;                 // (a replay token is treated exactly as a drawn one)
        if (drew) {
            int t = token_val >= -1 ? token_val : token[b];
            if constexpr (FORM) t = fm.tokv >= 0 ? fm.tokv : t;
            const int cur = s[F_CUR];
            const bool remnant = cur < s[F_NCHORD];
            const int cp = remnant ? chord_pos[(size_t)b * ld_chord + cur] : -1;
            const bool inter = remnant && cp != TOK_POS0;
            if (t < 0) {                                                                  // :286-291, Q12
                s[F_FAILED] = 1;
                s[F_DONE] = 1;
            } else if (inter && ((cp < t && t < TOK_POS0 + POS_RES) || t == TOK_BAR)) {    // :294-296
                s[F_FORCED] = cp;
                clear = 1;
            } else if (t >= TOK_CHORD_LO && t <= TOK_CHORD_HI) {                           // :299-301
                s[F_REDO] = 1;
                wrong[(size_t)b * VOCAB + t] = 1;
            } else if (remnant && t == TOK_EOS) {                                         // :304-306
                s[F_FORCED] = inter ? cp : TOK_BAR;
            } else if (!remnant && t == TOK_BAR) {                                        // :309-311
                s[F_FORCED] = TOK_EOS;
            } else {
                const int len = s[F_LEN];
                if (len < ld_seq) {
                    seq[(size_t)b * ld_seq + len] = t;
                    if (seq_logp != nullptr) {
                        float* q = seq_logp + 2 * ((size_t)b * ld_seq + len);
                        if (token_val >= -1) { q[0] = lp.full; q[1] = lp.kept; }
                        else if (logp != nullptr) { q[0] = logp[2 * b]; q[1] = logp[2 * b + 1]; }
                        else q[0] = q[1] = NAN;
                        if constexpr (FORM) {
                            if (fm.tokv >= 0) q[0] = q[1] = NAN;          // (it was not drawn)
                        }
                    }
                    s[F_LEN] = len + 1;
                    if constexpr (FORM) {
                        if (t == TOK_BAR) form_bar(fm, *fr, s[F_NBAR], len);
                        else if (fr->active && ++fr->k == 4) { fr->cursor = fr->g + 4; fr->k = 0; }
                    }
                }
                if (t == TOK_BAR) s[F_NBAR] += 1;
            }
        }
        if (live != nullptr && !s[F_DONE]) atomicAdd(live, 1);
    }
    clear = __builtin_amdgcn_readfirstlane(clear);
    if (clear)
        for (int i = lane; i < VOCAB; i += 64) wrong[(size_t)b * VOCAB + i] = 0;
}


}  // namespace
