// Device-resident chord / bar forcing of the decode loop (gfx950): the per-sequence control flow of
// InferenceTask.generate_sequence + TeacherForceTask (commu/midi_generator/midi_inferrer.py:239-320 and :16-144),
// so that one loop iteration of ALL sequences -- decide, model step, sampling step, book-keeping -- is a chain of
// kernels (captured in a hipGraph by commu_amd/generate.py) with no host round trip.
//
// The reference's rules are held as a per-sequence state record and two transition functions:
//   commu_forcing_pre  : before the model step.   STOP (EOS / iteration cap) | FEED a forced token | then which
//                        model step this iteration takes -- none (re-draw from the logits already divided by the
//                        temperature, quirk Q5), first step whose memory is discarded (Q3), normal step on the last
//                        token (re-feeding the last forced token, Q4) -- and whether a token is drawn or the next
//                        token is forced (position 432 after a bar; the next chord of the progression).
//   commu_forcing_post : after the draw.   position past a pending chord -> force that position | chord token
//                        drawn -> reject, remember it, redo | EOS with chords left -> force position / bar | bar
//                        with no chords left -> force EOS | else append.
// One 64-lane wave per sequence: lane 0 runs the transition, the wave clears the 729-entry rejected-token bitmap.
#include "sample_tier.h"
#include "commu_hip.h"

namespace {

__global__ __launch_bounds__(64) void forcing_pre_kernel(int* st, int* seq, int ld_seq, const int* __restrict__ chord_tok,
                                                         const int* __restrict__ chord_pos, int ld_chord,
                                                         unsigned char* wrong, const float* __restrict__ utable, int ld_u,
                                                         int max_iters, long long* tok, unsigned char* active,
                                                         unsigned char* keep, unsigned char* draw, float* uni, int* trace,
                                                         int ld_trace, float* seq_logp) {
    int rec[F_COUNT];
    if (threadIdx.x == 0) record_load(rec, st, blockIdx.x);
    forcing_pre_body(blockIdx.x, threadIdx.x, rec, seq, ld_seq, chord_tok, chord_pos, ld_chord, wrong, utable, ld_u, max_iters,
                     tok, active, keep, draw, uni, trace, ld_trace, seq_logp);
    if (threadIdx.x == 0) record_store(rec, st, blockIdx.x);
}

__global__ __launch_bounds__(64) void forcing_post_kernel(int* st, int* seq, int ld_seq, const int* __restrict__ chord_pos,
                                                          int ld_chord, unsigned char* wrong, const unsigned char* draw,
                                                          const int* token, int* live, int* klen, const unsigned char* keep,
                                                          int lmax, const float* logp, float* seq_logp) {
    int rec[F_COUNT];
    if (threadIdx.x == 0) record_load(rec, st, blockIdx.x);
    forcing_post_body(blockIdx.x, threadIdx.x, rec, seq, ld_seq, chord_pos, ld_chord, wrong, draw, token, live, klen, keep,
                      lmax, -3, TokenLogp{NAN, NAN}, logp, seq_logp);
    if (threadIdx.x == 0) record_store(rec, st, blockIdx.x);
}

// The two stages with the form rule (decode_loop.h: Form): the header of the slot's form state travels through the stage in
// lane 0's registers beside the record.
__global__ __launch_bounds__(64) void forcing_pre_form_kernel(int* st, int* seq, int ld_seq, const int* __restrict__ chord_tok,
                                                              const int* __restrict__ chord_pos, int ld_chord,
                                                              unsigned char* wrong, const float* __restrict__ utable,
                                                              int ld_u, int max_iters, long long* tok, unsigned char* active,
                                                              unsigned char* keep, unsigned char* draw, float* uni,
                                                              int* trace, int ld_trace, float* seq_logp, const int* form_ctl,
                                                              const unsigned* form_table, int form_rows, int* form_state,
                                                              int* form_tok, const int* form_src, int form_src_len) {
    const int b = blockIdx.x;
    int rec[F_COUNT] = {};
    FormRegs fr{0, 0, 0, 0, 0, -1};
    int* fs = form_state + (size_t)b * FS_COUNT;
    if (threadIdx.x == 0) {
        record_load(rec, st, b);
        form_regs_load(fr, fs);
    }
    forcing_pre_body<true>(b, threadIdx.x, rec, seq, ld_seq, chord_tok, chord_pos, ld_chord, wrong, utable, ld_u, max_iters,
                           tok, active, keep, draw, uni, trace, ld_trace, seq_logp,
                           Form{form_ctl[b], form_table, form_rows, fs, form_tok + b, -1, form_src, form_src_len}, &fr);
    if (threadIdx.x == 0) {
        record_store(rec, st, b);
        form_regs_store(fr, fs);
    }
}

__global__ __launch_bounds__(64) void forcing_post_form_kernel(int* st, int* seq, int ld_seq, const int* __restrict__ chord_pos,
                                                               int ld_chord, unsigned char* wrong, const unsigned char* draw,
                                                               const int* token, int* live, int* klen,
                                                               const unsigned char* keep, int lmax, const float* logp,
                                                               float* seq_logp, const int* form_ctl,
                                                               const unsigned* form_table, int form_rows, int* form_state,
                                                               int* form_tok, const int* form_src, int form_src_len) {
    const int b = blockIdx.x;
    int rec[F_COUNT] = {};
    FormRegs fr{0, 0, 0, 0, 0, -1};
    int* fs = form_state + (size_t)b * FS_COUNT;
    if (threadIdx.x == 0) {
        record_load(rec, st, b);
        form_regs_load(fr, fs);
    }
    forcing_post_body<true>(b, threadIdx.x, rec, seq, ld_seq, chord_pos, ld_chord, wrong, draw, token, live, klen, keep, lmax,
                            -3, TokenLogp{NAN, NAN}, logp, seq_logp, nullptr,
                            Form{form_ctl[b], form_table, form_rows, fs, form_tok + b, form_tok[b], form_src, form_src_len},
                            &fr);
    if (threadIdx.x == 0) {
        record_store(rec, st, b);
        form_regs_store(fr, fs);
    }
}

// form_state and form_tok of the slots first .. first + n - 1 as a load leaves them (form.h: form_reset_row): the BARs of
// seq[b][0 .. F_LEN) recorded, nothing replayed
__global__ __launch_bounds__(64) void form_reset_kernel(int* form_state, int* form_tok, const int* __restrict__ st,
                                                        const int* __restrict__ seq, int ld_seq, int first) {
    const int b = first + blockIdx.x;
    const int len = min(max(st[(size_t)b * F_COUNT + F_LEN], 0), ld_seq);
    form_reset_row(form_state + (size_t)b * FS_COUNT, seq + (size_t)b * ld_seq, len, threadIdx.x);
    if (threadIdx.x == 0) form_tok[b] = -1;
}

// One launch for the three per-sequence stages that follow the model step: sampling step -> book-keeping (post) -> the
// decision of the NEXT iteration (pre).  A sequence's stages only exchange data of that sequence, and one wave runs
// them in order; the workgroup barriers order the wave's own global stores and loads between stages.
// The argument block is a ladder of structs keyed by the tier (decode_loop.h: Tier): LoopArgs<T> is LoopArgs<T - 1> plus what
// tier T reads, and the kernel of tier T takes LoopArgs<T> by value -- so the launch without a constraint keeps its
// instructions AND its argument block (the kernel body is written on its parameter: moved into a device function that takes
// the arguments by reference, the kernels without a grammar came out different).
template <int TIER>
struct LoopArgs;
template <>
struct LoopArgs<T_NONE> {
    float* logits; int ld, V;
    unsigned char* wrong;
    float temperature; int top_k; float top_p;
    SamplingRows rows;              // per-sequence controls (null members: the scalars above)
    int* token; float* probs_out; int ldp;
    float *logp, *seq_logp;         // (optional) the draw's log-probability pair [B][2]; the pairs of the tokens in seq
    int *st, *seq; int ld_seq;
    const int *chord_tok, *chord_pos; int ld_chord;
    const float* utable; int ld_u, max_iters;
    long long* tok;
    unsigned char *active, *keep, *draw;
    float* uni;
    int* step_trace; int ld_trace;
    int* klen; int lmax;
    unsigned long long* trace;      // (diagnostics) [sequence][4] 100 MHz timestamps: start, sampled, post done, pre done
    const float* bias; int ld_bias; // (BIAS) the caller's constraint rows for the sampling step (sample_topk_body)
};
// the grammar table [8][ld_gram] and the slots' switches [B]
template <>
struct LoopArgs<T_GRAM> : LoopArgs<T_NONE> {
    const float* gram; int ld_gram;
    const unsigned char* gram_on;
};
// the harmony table [111][ld_harm] and the slots' switches [B]
template <>
struct LoopArgs<T_HARM> : LoopArgs<T_GRAM> {
    const float* harm; int ld_harm;
    const unsigned char* harm_on;
};
// the class-control records [B][8] (decode_loop.h: ClassControls)
template <>
struct LoopArgs<T_CLS> : LoopArgs<T_HARM> {
    const int4* cls_ctl;
};
// the control words [B] of the note order, the voice cap, the note density and the melodic interval (decode_loop.h:
// NoteOrder, Voices, Density, Interval)
template <>
struct LoopArgs<T_ORD> : LoopArgs<T_CLS> {
    const int* order_ctl;
};
template <>
struct LoopArgs<T_VOX> : LoopArgs<T_ORD> {
    const int* voice_ctl;
};
template <>
struct LoopArgs<T_DEN> : LoopArgs<T_VOX> {
    const int* density_ctl;
};
template <>
struct LoopArgs<T_MEL> : LoopArgs<T_DEN> {
    const int* interval_ctl;
};
// the control words [B], the table [rows][4] and its row count of the onset templates, the guide track and the
// articulation (decode_loop.h: Onsets, Guide, Articulation)
template <>
struct LoopArgs<T_ONS> : LoopArgs<T_MEL> {
    const int* onset_ctl;
    const unsigned* onset_table;
    int onset_rows;
};
template <>
struct LoopArgs<T_GDE> : LoopArgs<T_ONS> {
    const int* guide_ctl;
    const unsigned* guide_table;
    int guide_rows;
};
template <>
struct LoopArgs<T_ART> : LoopArgs<T_GDE> {
    const int* art_ctl;
    const unsigned* art_table;
    int art_rows;
};
// the form rule (decode_loop.h: Form) is a switch of its own beside the tier: the kernel with it takes the block of its tier
// plus these seven (the take buffer is optional: null, 0), the kernel without it the block it always took
template <int TIER>
struct LoopArgsForm : LoopArgs<TIER> {
    const int* form_ctl;
    const unsigned* form_table;
    int form_rows;
    int* form_state;
    int* form_tok;
    const int* form_src;
    int form_src_len;
};
template <bool BIAS, int TIER, bool FORM = false>
__global__ __launch_bounds__(64) void sample_post_pre_kernel(std::conditional_t<FORM, LoopArgsForm<TIER>, LoopArgs<TIER>> a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (a.trace != nullptr && lane == 0) a.trace[b * 4 + 0] = wall_clock64();
    int rec[F_COUNT];                                  // the record travels through the three stages in lane 0's registers;
    record_load(rec, a.st, b);                         // its loads are in flight under the sampling step (every lane loads the
                                                       // same words: behind `if (lane == 0)` the wave waited for them here)
    // what post reads of this iteration's decision, loaded here for the same reason (a null klen reads token[b] instead)
    const StepFlags flags{a.draw[b], a.keep[b], *(a.klen != nullptr ? a.klen + b : a.token + b)};
    TokenLogp lp{NAN, NAN};                            // like `drawn`, the pair reaches post in registers
    // (FORM) the header of the slot's form state, the control word and the replay token of this iteration's decision,
    // loaded with the record: every lane loads the same words
    Form fm{-1, nullptr, 1, nullptr, nullptr, -1};
    FormRegs fr{0, 0, 0, 0, 0, -1};
    if constexpr (FORM) {
        int* fs = a.form_state + (size_t)b * FS_COUNT;
        form_regs_load(fr, fs);
        fm = Form{a.form_ctl[b], a.form_table, a.form_rows, fs, a.form_tok + b, a.form_tok[b], a.form_src, a.form_src_len};
    }
    Grammar g{nullptr, 0, nullptr, 0, 0, 0};
    if constexpr (TIER >= T_GRAM) {
        // the slot's switch is loaded with the flags above (a null gram_on reads draw[b], which is then ignored).  The
        // previous token is one dependent load behind the record: the sampling body issues it right behind its logits
        // loads -- issued here, the wait for the record came BEFORE the logits loads and they sat behind it
        const unsigned char on_b = *(a.gram_on != nullptr ? a.gram_on + b : a.draw + b);
        g = Grammar{a.gram, a.ld_gram, a.seq + (size_t)b * a.ld_seq, rec[F_LEN], a.ld_seq,
                    a.gram_on != nullptr ? (int)on_b : 1};
    }
    Harmony h{nullptr, 0, nullptr, 0, 0, 0};
    if constexpr (TIER >= T_HARM) {
        // the same for the chord: the switch with the flags, the record's chord count as it was loaded; the chord token
        // chord_tok[b][F_CUR - 1] is the body's load, beside the previous token
        const unsigned char on_b = *(a.harm_on != nullptr ? a.harm_on + b : a.draw + b);
        h = Harmony{a.harm, a.ld_harm, a.chord_tok + (size_t)b * a.ld_chord, rec[F_CUR], a.ld_chord,
                    a.harm_on != nullptr ? (int)on_b : 1};
    }
    ClassControls cc{nullptr};
    if constexpr (TIER >= T_CLS) cc = ClassControls{a.cls_ctl + (size_t)b * 8};      // (the body loads the record it selects)
    // the control words are loaded with the flags above; the bar count of the onset row is the record's
    NoteOrder no{-1};
    if constexpr (TIER >= T_ORD) no = NoteOrder{a.order_ctl[b]};
    Voices vx{-1};
    if constexpr (TIER >= T_VOX) vx = Voices{a.voice_ctl[b]};
    Density dn{-1};
    if constexpr (TIER >= T_DEN) dn = Density{a.density_ctl[b]};
    Interval ml{-1};
    if constexpr (TIER >= T_MEL) ml = Interval{a.interval_ctl[b]};
    Onsets os{-1, nullptr, 1, 0};
    if constexpr (TIER >= T_ONS) os = Onsets{a.onset_ctl[b], a.onset_table, a.onset_rows, rec[F_NBAR]};
    Guide gd{-1, nullptr, 1};
    if constexpr (TIER >= T_GDE) gd = Guide{a.guide_ctl[b], a.guide_table, a.guide_rows};
    Articulation ar{-1, nullptr, 1};
    if constexpr (TIER >= T_ART) ar = Articulation{a.art_ctl[b], a.art_table, a.art_rows};
    const int drawn = sample_topk_body<BIAS, TIER>(
        b, lane, a.logits, a.ld, a.V, a.wrong, VOCAB, a.uni, a.draw, a.temperature, a.top_k, a.token, a.probs_out, a.ldp,
        a.top_p, a.rows, a.logp != nullptr || a.seq_logp != nullptr, a.logp, lp, a.bias, a.ld_bias, g, h, cc, no, vx, dn, ml,
        os, gd, ar);
    __syncthreads();
    if (a.trace != nullptr && lane == 0) a.trace[b * 4 + 1] = wall_clock64();
    forcing_post_body<FORM>(b, lane, rec, a.seq, a.ld_seq, a.chord_pos, a.ld_chord, a.wrong, a.draw, a.token, nullptr, a.klen,
                            a.keep, a.lmax, drawn >= -1 ? drawn : -3, lp, a.logp, a.seq_logp, &flags, fm, &fr);
    __syncthreads();
    if (a.trace != nullptr && lane == 0) a.trace[b * 4 + 2] = wall_clock64();
    forcing_pre_body<FORM>(b, lane, rec, a.seq, a.ld_seq, a.chord_tok, a.chord_pos, a.ld_chord, a.wrong, a.utable, a.ld_u,
                           a.max_iters, a.tok, a.active, a.keep, a.draw, a.uni, a.step_trace, a.ld_trace, a.seq_logp, fm, &fr);
    if (lane == 0) record_store(rec, a.st, b);
    if constexpr (FORM) {
        if (lane == 0) form_regs_store(fr, fm.state);
    }
    if (a.trace != nullptr && lane == 0) a.trace[b * 4 + 3] = wall_clock64();
}

// Primed generation: the two transitions replayed over a given token prefix with NO model step, so that a slot enters the
// loop in the state the free-running loop would be in after producing the prefix itself.  Wherever `pre` decides to
// draw, the next prompt token is handed to `post` as the drawn token; wherever `pre` feeds a forced token, that token
// must be the next prompt token.  The replay stops at the first prompt index the rules would not have produced.
// One wave per slot; lane 0 walks the prompt, the wave clears the rejected-token map where the transitions ask for it
// (every loop decision is broadcast, so the wave stays converged through the bodies).
enum { REPLAY_FORCED = 1,        // the rules force another token at this index
       REPLAY_NOT_APPENDED = 2,  // `post` does not append the token (chord where a draw is expected, position past a
                                 // pending chord, EOS / BAR that the rules replace, no room in seq)
       REPLAY_EOS = 3,           // the prompt holds EOS: nothing follows it
       REPLAY_INVALID = 4 };     // token outside [0, 729), or the record was finished before the prompt was
__global__ __launch_bounds__(64) void forcing_replay_kernel(int* st, int* seq, int ld_seq, const int* __restrict__ prompt,
                                                            int ld_prompt, const int* __restrict__ prompt_len,
                                                            const int* __restrict__ chord_tok,
                                                            const int* __restrict__ chord_pos, int ld_chord,
                                                            unsigned char* wrong, const float* __restrict__ utable,
                                                            int ld_u, long long* tok, unsigned char* active,
                                                            unsigned char* keep, unsigned char* draw, float* uni,
                                                            int* trace, int ld_trace, float* seq_logp, int* klen, int* fed,
                                                            int ld_fed, int* diverged) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(prompt_len[b], 0), ld_prompt);
    if (lane == 0) diverged[2 * b] = diverged[2 * b + 1] = -1;
    if (n == 0) return;                                // the record stays exactly as load() wrote it
    const int* pr = prompt + (size_t)b * ld_prompt;
    int rec[F_COUNT] = {};
    if (lane == 0) record_load(rec, st, b);
    int i = 0, nfed = 0, at = -1, why = -1;            // (lane 0) prompt index, kept tokens fed, divergence
    // a prompt token takes at most two iterations (the decision to force it, then its append)
#pragma unroll 1
    for (int it = 0; it < 2 * n + 2; ++it) {
        int stop = 0;
        if (lane == 0) {
            if (i >= n) stop = 1;
            else if (pr[i] < 0 || pr[i] >= VOCAB) { at = i; why = REPLAY_INVALID; stop = 1; }
            else if (rec[F_FORCED] >= 0 && rec[F_FORCED] != pr[i]) { at = i; why = REPLAY_FORCED; stop = 1; }
        }
        if (__builtin_amdgcn_readfirstlane(stop)) break;
        const int len0 = rec[F_LEN];
        forcing_pre_body(b, lane, rec, seq, ld_seq, chord_tok, chord_pos, ld_chord, wrong, utable, ld_u, 0x7fffffff, tok,
                         active, keep, draw, uni, trace, ld_trace, seq_logp);
        int tv = -1, drew = 0;
        if (lane == 0) {
            if (rec[F_DONE]) { at = i; why = REPLAY_INVALID; stop = 1; }
            else {
                if (active[b] && keep[b]) {            // what the loop would have given the model and kept
                    if (nfed < ld_fed) fed[(size_t)b * ld_fed + nfed] = (int)tok[b];
                    ++nfed;
                }
                if (rec[F_LEN] > len0) {               // the forced token pr[i] was appended
                    if (pr[i] == TOK_EOS) { at = i; why = REPLAY_EOS; stop = 1; }
                    ++i;
                }
                drew = draw[b];
                if (drew) tv = pr[i];                  // (a draw and a forced append exclude each other: i < n here)
            }
        }
        if (__builtin_amdgcn_readfirstlane(stop)) break;
        const int len1 = rec[F_LEN];
        forcing_post_body(b, lane, rec, seq, ld_seq, chord_pos, ld_chord, wrong, draw, nullptr, nullptr, klen, keep,
                          1 << 30, tv, TokenLogp{NAN, NAN}, nullptr, seq_logp);
        if (lane == 0 && drew) {
            if (rec[F_LEN] == len1) { at = i; why = REPLAY_NOT_APPENDED; stop = 1; }
            else {
                if (tv == TOK_EOS) { at = i; why = REPLAY_EOS; stop = 1; }
                ++i;
            }
        }
        if (__builtin_amdgcn_readfirstlane(stop)) break;
    }
    if (lane == 0) {
        if (at < 0 && i < n) { at = i; why = REPLAY_INVALID; }
        rec[F_ITERS] = 0;                              // generation_length and the variate table count what follows
        rec[F_NDRAW] = 0;
        record_store(rec, st, b);
        diverged[2 * b] = at;
        diverged[2 * b + 1] = why;
    }
}

// dst[b][0:n] = src[b][0:n] for rows with mask[b] != 0 (the logits of the sequences that stepped: the others keep
// theirs for a possible re-draw, quirk Q5)
__global__ void copy_rows_masked_kernel(float* __restrict__ dst, int ldd, const float* __restrict__ src, int lds_,
                                        const unsigned char* __restrict__ mask, int n) {
    const int b = blockIdx.x;
    if (!mask[b]) return;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[(size_t)b * ldd + i] = src[(size_t)b * lds_ + i];
}

}  // namespace

extern "C" int commu_forcing_state_ints(void) { return F_COUNT; }

extern "C" int commu_forcing_pre(int* state, int* seq, int ld_seq, const int* chord_tok, const int* chord_pos,
                                 int ld_chord, unsigned char* wrong, const float* utable, int ld_u, int max_iters,
                                 long long* tok, unsigned char* active, unsigned char* keep, unsigned char* draw,
                                 float* uni, int* trace, int ld_trace, float* seq_logp, int B, hipStream_t stream) {
    if (B <= 0) return 0;
    if (ld_seq < 2 || ld_chord < 1 || ld_u < 1) return -22;
    COMMU_LAUNCH(forcing_pre_kernel, dim3(B), dim3(64), 0, stream, state, seq, ld_seq, chord_tok, chord_pos, ld_chord,
                 wrong, utable, ld_u, max_iters, tok, active, keep, draw, uni, trace, ld_trace, seq_logp);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_forcing_post(int* state, int* seq, int ld_seq, const int* chord_pos, int ld_chord,
                                  unsigned char* wrong, const unsigned char* draw, const int* token, int* live,
                                  int* klen, const unsigned char* keep, int lmax, const float* logp, float* seq_logp,
                                  int B, hipStream_t stream) {
    if (B <= 0) return 0;
    COMMU_LAUNCH(forcing_post_kernel, dim3(B), dim3(64), 0, stream, state, seq, ld_seq, chord_pos, ld_chord, wrong,
                 draw, token, live, klen, keep, lmax, logp, seq_logp);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_form_state_ints(void) { return FS_COUNT; }

static bool form_args_ok(const int* form_ctl, const unsigned* form_table, int form_rows, const int* form_state,
                         const int* form_tok) {
    return form_ctl != nullptr && form_table != nullptr && form_state != nullptr && form_tok != nullptr && form_rows >= 1 &&
           form_rows <= FORM_ROWS_MAX;
}
// (the take buffer is optional; given, it holds at least one token)
static bool form_src_ok(const int* form_src, int form_src_len) { return form_src == nullptr || form_src_len >= 1; }
constexpr int FORM_SRC_MAX = 1 << 18;      // ints the decoder's take buffer holds: 64 takes of 4096 tokens

extern "C" int commu_form_src_max(void) { return FORM_SRC_MAX; }

extern "C" int commu_forcing_pre_form_src(int* state, int* seq, int ld_seq, const int* chord_tok, const int* chord_pos,
                                          int ld_chord, unsigned char* wrong, const float* utable, int ld_u, int max_iters,
                                          long long* tok, unsigned char* active, unsigned char* keep, unsigned char* draw,
                                          float* uni, int* trace, int ld_trace, float* seq_logp, const int* form_ctl,
                                          const unsigned* form_table, int form_rows, int* form_state, int* form_tok,
                                          const int* form_src, int form_src_len, int B, hipStream_t stream) {
    if (B <= 0) return 0;
    if (ld_seq < 2 || ld_chord < 1 || ld_u < 1) return -22;
    if (!form_args_ok(form_ctl, form_table, form_rows, form_state, form_tok) || !form_src_ok(form_src, form_src_len)) return -22;
    COMMU_LAUNCH(forcing_pre_form_kernel, dim3(B), dim3(64), 0, stream, state, seq, ld_seq, chord_tok, chord_pos, ld_chord,
                 wrong, utable, ld_u, max_iters, tok, active, keep, draw, uni, trace, ld_trace, seq_logp, form_ctl, form_table,
                 form_rows, form_state, form_tok, form_src, form_src_len);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_forcing_pre_form(int* state, int* seq, int ld_seq, const int* chord_tok, const int* chord_pos,
                                      int ld_chord, unsigned char* wrong, const float* utable, int ld_u, int max_iters,
                                      long long* tok, unsigned char* active, unsigned char* keep, unsigned char* draw,
                                      float* uni, int* trace, int ld_trace, float* seq_logp, const int* form_ctl,
                                      const unsigned* form_table, int form_rows, int* form_state, int* form_tok, int B,
                                      hipStream_t stream) {
    return commu_forcing_pre_form_src(state, seq, ld_seq, chord_tok, chord_pos, ld_chord, wrong, utable, ld_u, max_iters, tok,
                                      active, keep, draw, uni, trace, ld_trace, seq_logp, form_ctl, form_table, form_rows,
                                      form_state, form_tok, nullptr, 0, B, stream);
}

extern "C" int commu_forcing_post_form_src(int* state, int* seq, int ld_seq, const int* chord_pos, int ld_chord,
                                           unsigned char* wrong, const unsigned char* draw, const int* token, int* live,
                                           int* klen, const unsigned char* keep, int lmax, const float* logp,
                                           float* seq_logp, const int* form_ctl, const unsigned* form_table, int form_rows,
                                           int* form_state, int* form_tok, const int* form_src, int form_src_len, int B,
                                           hipStream_t stream) {
    if (B <= 0) return 0;
    if (ld_seq < 2 || ld_chord < 1) return -22;
    if (!form_args_ok(form_ctl, form_table, form_rows, form_state, form_tok) || !form_src_ok(form_src, form_src_len)) return -22;
    COMMU_LAUNCH(forcing_post_form_kernel, dim3(B), dim3(64), 0, stream, state, seq, ld_seq, chord_pos, ld_chord, wrong,
                 draw, token, live, klen, keep, lmax, logp, seq_logp, form_ctl, form_table, form_rows, form_state, form_tok,
                 form_src, form_src_len);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_forcing_post_form(int* state, int* seq, int ld_seq, const int* chord_pos, int ld_chord,
                                       unsigned char* wrong, const unsigned char* draw, const int* token, int* live,
                                       int* klen, const unsigned char* keep, int lmax, const float* logp, float* seq_logp,
                                       const int* form_ctl, const unsigned* form_table, int form_rows, int* form_state,
                                       int* form_tok, int B, hipStream_t stream) {
    return commu_forcing_post_form_src(state, seq, ld_seq, chord_pos, ld_chord, wrong, draw, token, live, klen, keep, lmax,
                                       logp, seq_logp, form_ctl, form_table, form_rows, form_state, form_tok, nullptr, 0, B,
                                       stream);
}

extern "C" int commu_form_reset(int* form_state, int* form_tok, const int* state, const int* seq, int ld_seq, int first,
                                int n, hipStream_t stream) {
    if (n <= 0) return 0;
    if (form_state == nullptr || form_tok == nullptr || state == nullptr || seq == nullptr || ld_seq < 1 || first < 0)
        return -22;
    COMMU_LAUNCH(form_reset_kernel, dim3(n), dim3(64), 0, stream, form_state, form_tok, state, seq, ld_seq, first);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_forcing_replay(int* state, int* seq, int ld_seq, const int* prompt, int ld_prompt,
                                    const int* prompt_len, const int* chord_tok, const int* chord_pos, int ld_chord,
                                    unsigned char* wrong, const float* utable, int ld_u, long long* tok,
                                    unsigned char* active, unsigned char* keep, unsigned char* draw, float* uni, int* trace,
                                    int ld_trace, float* seq_logp, int* klen, int* fed, int ld_fed, int* diverged, int B,
                                    hipStream_t stream) {
    if (B <= 0) return 0;
    if (ld_seq < 2 || ld_chord < 1 || ld_u < 1 || ld_prompt < 1 || ld_fed < 1) return -22;
    if (state == nullptr || seq == nullptr || prompt == nullptr || prompt_len == nullptr || wrong == nullptr ||
        utable == nullptr || tok == nullptr || active == nullptr || keep == nullptr || draw == nullptr || uni == nullptr ||
        klen == nullptr || fed == nullptr || diverged == nullptr)
        return -22;
    COMMU_LAUNCH(forcing_replay_kernel, dim3(B), dim3(64), 0, stream, state, seq, ld_seq, prompt, ld_prompt, prompt_len,
                 chord_tok, chord_pos, ld_chord, wrong, utable, ld_u, tok, active, keep, draw, uni, trace, ld_trace, seq_logp,
                 klen, fed, ld_fed, diverged);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_copy_rows_masked_f32(float* dst, int ldd, const float* src, int lds_, const unsigned char* mask,
                                          int rows, int n, hipStream_t stream) {
    if (rows <= 0 || n <= 0) return 0;
    COMMU_LAUNCH(copy_rows_masked_kernel, dim3(rows), dim3(256), 0, stream, dst, ldd, src, lds_, mask, n);
    COMMU_LAUNCH_CHECK();
    return 0;
}

static unsigned long long* g_loop_trace = nullptr;
/* diagnostics: following commu_decode_sample_post_pre launches write buf[sequence][4] timestamps (null: off) */
extern "C" int commu_decode_loop_trace(unsigned long long* buf) {
    g_loop_trace = buf;
    return 0;
}

extern "C" int commu_decode_loop_args_bytes(void) { return (int)sizeof(commu_decode_loop_args); }

// The one host entry point of the fused launch: validate once, then pick the kernel by which constraint pointers are given.
extern "C" int commu_decode_sample_post_pre(const commu_decode_loop_args* p, hipStream_t stream) {
    if (p == nullptr || p->struct_bytes != sizeof(commu_decode_loop_args)) return -22;
    if (p->B <= 0) return 0;
    const int V = p->V;
    if (V != VOCAB || V > 64 * PER_LANE || p->ld_seq < 2 || p->ld_chord < 1 || p->ld_u < 1) return -22;
    // (a scalar that an array replaces is not looked at; the kernel clamps what the arrays hold)
    // (with cls_ctl neither the scalars nor the arrays are looked at)
    if (p->cls_ctl == nullptr &&
        ((p->top_k_rows == nullptr && (p->top_k < 1 || p->top_k > V)) || (p->top_p_rows == nullptr && !(p->top_p > 0.f))))
        return -22;
    if (!check_constraints(*p, V)) return -22;
    // (the form rule: every one of its arrays or none)
    if (p->form_ctl != nullptr && !form_args_ok(p->form_ctl, p->form_table, p->form_rows, p->form_state, p->form_tok))
        return -22;
    // (the take buffer: optional, never without the rule, never empty)
    if (p->form_src != nullptr && (p->form_ctl == nullptr || p->form_src_len < 1)) return -22;
    LoopArgsForm<T_ART> a;
    static_cast<LoopArgs<T_NONE>&>(a) = LoopArgs<T_NONE>{
        p->logits, p->ld, V, p->wrong, p->temperature, p->top_k, p->top_p,
        SamplingRows{p->temperature_rows, p->top_k_rows, p->top_p_rows}, p->token, p->probs_out, p->ldp, p->logp, p->seq_logp,
        p->state, p->seq, p->ld_seq, p->chord_tok, p->chord_pos, p->ld_chord, p->utable, p->ld_u, p->max_iters, p->tok,
        p->active, p->keep, p->draw, p->uni, p->trace, p->ld_trace, p->klen, p->lmax, g_loop_trace, p->bias, p->ld_bias};
    a.gram = p->gram; a.ld_gram = p->ld_gram; a.gram_on = p->gram_on;
    a.harm = p->harm; a.ld_harm = p->ld_harm; a.harm_on = p->harm_on;
    a.cls_ctl = static_cast<const int4*>(p->cls_ctl);
    a.order_ctl = p->order_ctl;
    a.voice_ctl = p->voice_ctl;
    a.density_ctl = p->density_ctl;
    a.interval_ctl = p->interval_ctl;
    a.onset_ctl = p->onset_ctl; a.onset_table = p->onset_table; a.onset_rows = p->onset_rows;
    a.guide_ctl = p->guide_ctl; a.guide_table = p->guide_table; a.guide_rows = p->guide_rows;
    a.art_ctl = p->art_ctl; a.art_table = p->art_table; a.art_rows = p->art_rows;
    a.form_ctl = p->form_ctl; a.form_table = p->form_table; a.form_rows = p->form_rows;
    a.form_state = p->form_state; a.form_tok = p->form_tok;
    a.form_src = p->form_src; a.form_src_len = p->form_src_len;
    const dim3 grid(p->B), block(64);
    // one kernel per tier, each with the argument block of its own tier (by value), so that a launch below a tier is the one
    // it always was: no added load, no added register, no added argument.  Below the harmony tier a bias is optional and
    // the launch without one is a kernel of its own.
    with_tier(tier_of(*p), [&](auto t) {
        constexpr int T = decltype(t)::value;
        const auto& at = static_cast<const LoopArgs<T>&>(a);      // (each kernel gets the block of its own tier)
        if (p->form_ctl != nullptr) {                             // (the form kernels: that block and the form's seven)
            LoopArgsForm<T> af;
            static_cast<LoopArgs<T>&>(af) = at;
            af.form_ctl = a.form_ctl; af.form_table = a.form_table; af.form_rows = a.form_rows;
            af.form_state = a.form_state; af.form_tok = a.form_tok;
            af.form_src = a.form_src; af.form_src_len = a.form_src_len;
            if constexpr (T < T_HARM) {
                if (p->bias == nullptr) {
                    COMMU_LAUNCH((sample_post_pre_kernel<false, T, true>), grid, block, 0, stream, af);
                    return;
                }
            }
            COMMU_LAUNCH((sample_post_pre_kernel<true, T, true>), grid, block, 0, stream, af);
            return;
        }
        if constexpr (T < T_HARM) {
            if (p->bias == nullptr) {
                COMMU_LAUNCH((sample_post_pre_kernel<false, T>), grid, block, 0, stream, at);
                return;
            }
        }
        COMMU_LAUNCH((sample_post_pre_kernel<true, T>), grid, block, 0, stream, at);
    });
    COMMU_LAUNCH_CHECK();
    return 0;
}
