// K15: the sampling step of the decode loop, one wave per sequence, no host round trip inside.
// Reference: commu/midi_generator/midi_inferrer.py:209-237
//   calc_probs    : logits[1:] /= temperature (IN PLACE, quirk Q5), softmax, left-pad 0 (Q6)
//                   (temperature == 0: one-hot at argmax)
//   apply_sampling: keep the top-k probabilities, zero the rejected ("wrong") tokens, renormalise
//   infer_token   : draw one token from the result -- here by inverse CDF with an injected
//                   uniform variate u[b] (torch.multinomial's stream is not reproducible).
// A sequence whose kept mass is 0 (Q12: greedy argmax is a rejected token) gets token -1.
// The controls may be per-sequence device arrays, and the step can report the log-probabilities of the token it drew
// (decode_loop.h: SamplingRows, TokenLogp).  An optional additive row per sequence constrains what may be drawn (bias, then
// top-k: sample_topk_body<BIAS>); a table of such rows, picked by the class of the sequence's previous token, makes an event
// grammar (<GRAM>, kernels of their own); a table of pitch-class rows, picked by the last chord the forcing rules placed, keeps
// the drawn pitches in the sounding chord (<HARM>, one more kernel); without any of them the launch is the kernel that never
// heard of them.  A table of control records per sequence, picked by the same class, gives each token family its own
// temperature / top_k / top_p (<CLS>, a sixth kernel: the harmony kernel with the table).  A control word per sequence
// bans what would break the note order of the bar being written (<ORD>, a seventh: the class kernel with the scan of seq);
// one more caps the notes that sound at once and bans re-striking a sounding pitch (<VOX>, an eighth: the same scan, longer);
// one more bounds the notes of the bar being written from below and above (<DEN>, a ninth: the voices kernel with a count);
// one more caps the leap from the last note to the pitch drawn next (<MEL>, a tenth: the density kernel with the last note);
// one more bans the onsets the open bar's template row leaves clear (<ONS>, an eleventh: the interval kernel with the row).
#include "decode_loop.h"
#include "commu_hip.h"

namespace {

template <bool BIAS>
__global__ __launch_bounds__(64) void sample_topk_kernel(float* __restrict__ logits, int ld, int V,
                                                         const unsigned char* __restrict__ wrong, int ldw,
                                                         const float* __restrict__ uni,
                                                         const unsigned char* __restrict__ active,
                                                         float temperature, int top_k,
                                                         int* __restrict__ token, float* __restrict__ probs_out,
                                                         int ldp, float top_p, SamplingRows rows,
                                                         float* __restrict__ logp_out,
                                                         const float* __restrict__ bias, int ld_bias) {
    TokenLogp lp;
    sample_topk_body<BIAS>(blockIdx.x, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k, token,
                           probs_out, ldp, top_p, rows, logp_out != nullptr, logp_out, lp, bias, ld_bias);
}

// the same with an event grammar: a kernel of its own, so that the launch without one keeps its arguments to the byte
template <bool BIAS>
__global__ __launch_bounds__(64) void sample_topk_gram_kernel(float* __restrict__ logits, int ld, int V,
                                                              const unsigned char* __restrict__ wrong, int ldw,
                                                              const float* __restrict__ uni,
                                                              const unsigned char* __restrict__ active,
                                                              float temperature, int top_k,
                                                              int* __restrict__ token, float* __restrict__ probs_out,
                                                              int ldp, float top_p, SamplingRows rows,
                                                              float* __restrict__ logp_out,
                                                              const float* __restrict__ bias, int ld_bias,
                                                              const float* __restrict__ gram, int ld_gram,
                                                              const unsigned char* __restrict__ gram_on,
                                                              const int* __restrict__ state, const int* __restrict__ seq,
                                                              int ld_seq) {
    TokenLogp lp;
    // the record's length and the switch are loaded here (a null gram_on reads a valid byte of this sequence, which is
    // then ignored); the previous token is the body's load
    const int b = blockIdx.x;
    const unsigned char on_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)on_b : 1};
    sample_topk_body<BIAS, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k, token,
                                 probs_out, ldp, top_p, rows, logp_out != nullptr, logp_out, lp, bias, ld_bias, g);
}

// the same with a harmony table: one instantiation (a bias and a grammar that change nothing are a zero row and an
// all-off switch array), again a kernel of its own with its own arguments
__global__ __launch_bounds__(64) void sample_topk_harm_kernel(float* __restrict__ logits, int ld, int V,
                                                              const unsigned char* __restrict__ wrong, int ldw,
                                                              const float* __restrict__ uni,
                                                              const unsigned char* __restrict__ active,
                                                              float temperature, int top_k,
                                                              int* __restrict__ token, float* __restrict__ probs_out,
                                                              int ldp, float top_p, SamplingRows rows,
                                                              float* __restrict__ logp_out,
                                                              const float* __restrict__ bias, int ld_bias,
                                                              const float* __restrict__ gram, int ld_gram,
                                                              const unsigned char* __restrict__ gram_on,
                                                              const int* __restrict__ state, const int* __restrict__ seq,
                                                              int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                              const unsigned char* __restrict__ harm_on,
                                                              const int* __restrict__ chord_tok, int ld_chord) {
    TokenLogp lp;
    // the record's length and chord count and the two switches are loaded here (a null switch array reads a valid byte
    // of this sequence, which is then ignored); the previous token and the chord token are the body's loads
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    sample_topk_body<true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k, token,
                                       probs_out, ldp, top_p, rows, logp_out != nullptr, logp_out, lp, bias, ld_bias, g, h);
}

// the same with class-keyed sampling controls (ClassControls): the harmony kernel's arguments plus the table of records,
// once more a kernel of its own -- the triple of a draw is record token_class(previous token) of the sequence's table, the
// scalars and the *_rows arrays are not looked at (they stay in the argument block so that the launch helper is shared)
__global__ __launch_bounds__(64) void sample_topk_cls_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    sample_topk_body<true, true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k,
                                             token, probs_out, ldp, top_p, rows, logp_out != nullptr, logp_out, lp, bias,
                                             ld_bias, g, h, cc);
}

// the same with the note-order constraint (NoteOrder): the class kernel's arguments plus the control words, a kernel of
// its own once more; the control word is loaded here, the scan of seq is the body's
__global__ __launch_bounds__(64) void sample_topk_ord_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    sample_topk_body<true, true, true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature,
                                                   top_k, token, probs_out, ldp, top_p, rows, logp_out != nullptr, logp_out,
                                                   lp, bias, ld_bias, g, h, cc, no);
}

// the same with the voice cap (Voices): the note-order kernel's arguments plus the voice words, a kernel of its own once
// more; the scan of seq is the note order's, continued to the second BAR
__global__ __launch_bounds__(64) void sample_topk_vox_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl,
                                                             const int* __restrict__ voice_ctl) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    const Voices vx{voice_ctl[b]};
    sample_topk_body<true, true, true, true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature,
                                                         top_k, token, probs_out, ldp, top_p, rows, logp_out != nullptr,
                                                         logp_out, lp, bias, ld_bias, g, h, cc, no, vx);
}

// the same with the note density (Density): the voices kernel's arguments plus the density words, a kernel of its own once
// more; the walk over seq is the voice cap's, with the count of the open bar's notes
__global__ __launch_bounds__(64) void sample_topk_den_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl,
                                                             const int* __restrict__ voice_ctl,
                                                             const int* __restrict__ density_ctl) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    const Voices vx{voice_ctl[b]};
    const Density dn{density_ctl[b]};
    sample_topk_body<true, true, true, true, true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active,
                                                               temperature, top_k, token, probs_out, ldp, top_p, rows,
                                                               logp_out != nullptr, logp_out, lp, bias, ld_bias, g, h, cc,
                                                               no, vx, dn);
}

// the same with the melodic interval (Interval): the density kernel's arguments plus the interval words, a kernel of its own
// once more; the walk over seq is the voice cap's, which also finds the last note
__global__ __launch_bounds__(64) void sample_topk_mel_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl,
                                                             const int* __restrict__ voice_ctl,
                                                             const int* __restrict__ density_ctl,
                                                             const int* __restrict__ interval_ctl) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    const Voices vx{voice_ctl[b]};
    const Density dn{density_ctl[b]};
    const Interval ml{interval_ctl[b]};
    sample_topk_body<true, true, true, true, true, true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active,
                                                                     temperature, top_k, token, probs_out, ldp, top_p, rows,
                                                                     logp_out != nullptr, logp_out, lp, bias, ld_bias, g, h,
                                                                     cc, no, vx, dn, ml);
}

// the same with the onset templates (Onsets): the interval kernel's arguments plus the control words, the table and its
// row count, a kernel of its own once more; the open bar's index comes from the record (F_NBAR), read beside F_LEN
__global__ __launch_bounds__(64) void sample_topk_ons_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl,
                                                             const int* __restrict__ voice_ctl,
                                                             const int* __restrict__ density_ctl,
                                                             const int* __restrict__ interval_ctl,
                                                             const int* __restrict__ onset_ctl,
                                                             const unsigned* __restrict__ onset_table, int onset_rows) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    const Voices vx{voice_ctl[b]};
    const Density dn{density_ctl[b]};
    const Interval ml{interval_ctl[b]};
    const Onsets os{onset_ctl[b], onset_table, onset_rows, state[(size_t)b * F_COUNT + F_NBAR]};
    sample_topk_body<true, true, true, true, true, true, true, true, true>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni,
                                                                           active, temperature, top_k, token, probs_out, ldp,
                                                                           top_p, rows, logp_out != nullptr, logp_out, lp,
                                                                           bias, ld_bias, g, h, cc, no, vx, dn, ml, os);
}

// the same with the guide track (Guide): the onsets kernel's arguments plus the guide's control words, its table and row
// count, a kernel of its own once more; the open bar's index is the record's F_NBAR, as for the onset row
__global__ __launch_bounds__(64) void sample_topk_gde_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl,
                                                             const int* __restrict__ voice_ctl,
                                                             const int* __restrict__ density_ctl,
                                                             const int* __restrict__ interval_ctl,
                                                             const int* __restrict__ onset_ctl,
                                                             const unsigned* __restrict__ onset_table, int onset_rows,
                                                             const int* __restrict__ guide_ctl,
                                                             const unsigned* __restrict__ guide_table, int guide_rows) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    const Voices vx{voice_ctl[b]};
    const Density dn{density_ctl[b]};
    const Interval ml{interval_ctl[b]};
    const Onsets os{onset_ctl[b], onset_table, onset_rows, state[(size_t)b * F_COUNT + F_NBAR]};
    const Guide gd{guide_ctl[b], guide_table, guide_rows};
    sample_topk_body<true, true, true, true, true, true, true, true, true, true>(
        b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k, token, probs_out, ldp, top_p, rows,
        logp_out != nullptr, logp_out, lp, bias, ld_bias, g, h, cc, no, vx, dn, ml, os, gd);
}

// the same with the articulation (Articulation): the guide kernel's arguments plus the articulation's control words, its
// table and row count, a kernel of its own once more; the open bar's index is the record's F_NBAR, as for the onset row
__global__ __launch_bounds__(64) void sample_topk_art_kernel(float* __restrict__ logits, int ld, int V,
                                                             const unsigned char* __restrict__ wrong, int ldw,
                                                             const float* __restrict__ uni,
                                                             const unsigned char* __restrict__ active,
                                                             float temperature, int top_k,
                                                             int* __restrict__ token, float* __restrict__ probs_out,
                                                             int ldp, float top_p, SamplingRows rows,
                                                             float* __restrict__ logp_out,
                                                             const float* __restrict__ bias, int ld_bias,
                                                             const float* __restrict__ gram, int ld_gram,
                                                             const unsigned char* __restrict__ gram_on,
                                                             const int* __restrict__ state, const int* __restrict__ seq,
                                                             int ld_seq, const float* __restrict__ harm, int ld_harm,
                                                             const unsigned char* __restrict__ harm_on,
                                                             const int* __restrict__ chord_tok, int ld_chord,
                                                             const int4* __restrict__ cls_ctl,
                                                             const int* __restrict__ order_ctl,
                                                             const int* __restrict__ voice_ctl,
                                                             const int* __restrict__ density_ctl,
                                                             const int* __restrict__ interval_ctl,
                                                             const int* __restrict__ onset_ctl,
                                                             const unsigned* __restrict__ onset_table, int onset_rows,
                                                             const int* __restrict__ guide_ctl,
                                                             const unsigned* __restrict__ guide_table, int guide_rows,
                                                             const int* __restrict__ art_ctl,
                                                             const unsigned* __restrict__ art_table, int art_rows) {
    TokenLogp lp;
    const int b = blockIdx.x;
    const unsigned char gon_b = *(gram_on != nullptr ? gram_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const unsigned char hon_b = *(harm_on != nullptr ? harm_on + b : reinterpret_cast<const unsigned char*>(token + b));
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, state[(size_t)b * F_COUNT + F_LEN], ld_seq,
                    gram_on != nullptr ? (int)gon_b : 1};
    const Harmony h{harm, ld_harm, chord_tok + (size_t)b * ld_chord, state[(size_t)b * F_COUNT + F_CUR], ld_chord,
                    harm_on != nullptr ? (int)hon_b : 1};
    const ClassControls cc{cls_ctl + (size_t)b * 8};
    const NoteOrder no{order_ctl[b]};
    const Voices vx{voice_ctl[b]};
    const Density dn{density_ctl[b]};
    const Interval ml{interval_ctl[b]};
    const Onsets os{onset_ctl[b], onset_table, onset_rows, state[(size_t)b * F_COUNT + F_NBAR]};
    const Guide gd{guide_ctl[b], guide_table, guide_rows};
    const Articulation ar{art_ctl[b], art_table, art_rows};
    sample_topk_body<true, true, true, true, true, true, true, true, true, true, true>(
        b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k, token, probs_out, ldp, top_p, rows,
        logp_out != nullptr, logp_out, lp, bias, ld_bias, g, h, cc, no, vx, dn, ml, os, gd, ar);
}

}  // namespace

extern "C" int commu_sample_args_bytes(void) { return (int)sizeof(commu_sample_args); }

// The one host entry point: validate once, then pick the kernel by which constraint pointers are given.
extern "C" int commu_sample_topk(const commu_sample_args* a, hipStream_t stream) {
    if (a == nullptr || a->struct_bytes != sizeof(commu_sample_args)) return -22;
    if (a->nseq <= 0) return 0;
    const int V = a->V;
    // (a scalar that an array replaces is not looked at; the kernel clamps what the arrays hold)
    // (with cls_ctl neither the scalars nor the arrays are looked at)
    if (V > 64 * PER_LANE || V < 2 ||
        (a->cls_ctl == nullptr && ((a->top_k_rows == nullptr && (a->top_k < 1 || a->top_k > V)) ||
                                   (a->top_p_rows == nullptr && !(a->top_p > 0.f)))))
        return -22;
    if (a->bias != nullptr && a->ld_bias < V) return -22;    // (the kernel reads bias[b][0 .. V-1])
    // (the kernel reads gram[0 .. 7][0 .. V-1] and finds the previous token through the record)
    if (a->gram != nullptr && (a->ld_gram < V || a->state == nullptr || a->seq == nullptr || a->ld_seq < 1)) return -22;
    // (the kernel reads harm[0 .. 110][0 .. 11] and finds the chord through the record: chord_tok[b][F_CUR - 1]; one
    // instantiation: the caller passes a zero bias and an all-off grammar where it has none)
    if (a->harm != nullptr && (a->ld_harm < 12 || a->chord_tok == nullptr || a->ld_chord < 1 || a->bias == nullptr ||
                               a->gram == nullptr))
        return -22;
    // (the kernel reads cls_ctl[b][0 .. 7] as 16-byte records and finds the previous token through the record, as the
    // grammar does; one instantiation: it is the harmony kernel's caller that passes the zero bias and the all-off tables)
    if (a->cls_ctl != nullptr && (a->state == nullptr || a->seq == nullptr || a->bias == nullptr || a->gram == nullptr ||
                                  a->harm == nullptr || a->chord_tok == nullptr || a->ld_seq < 1 ||
                                  (reinterpret_cast<uintptr_t>(a->cls_ctl) & 15u) != 0))
        return -22;
    // (the kernel reads order_ctl[b] and walks seq[b] backwards from the record's length; one instantiation, the class
    // kernel's with the scan: a caller without class controls passes the base-triple table)
    if (a->order_ctl != nullptr && a->cls_ctl == nullptr) return -22;
    // (the kernel reads voice_ctl[b] and continues the note order's walk to the second BAR; one instantiation, the
    // note-order kernel's with the longer scan)
    if (a->voice_ctl != nullptr && a->order_ctl == nullptr) return -22;
    // (the kernel reads density_ctl[b] and counts the open bar's notes on the voice cap's walk; one instantiation, the
    // voices kernel's with the count)
    if (a->density_ctl != nullptr && a->voice_ctl == nullptr) return -22;
    // (the kernel reads interval_ctl[b] and finds the reference note on the voice cap's walk; one instantiation, the
    // density kernel's with the last note)
    if (a->interval_ctl != nullptr && a->density_ctl == nullptr) return -22;
    // (the kernel reads onset_ctl[b] and one row of onset_table[0 .. onset_rows - 1][0 .. 3], its index clamped into the
    // table; one instantiation, the interval kernel's with the row)
    if (a->onset_ctl != nullptr && (a->interval_ctl == nullptr || a->onset_table == nullptr || a->onset_rows < 1 ||
                                    a->onset_rows > ONS_ROWS_MAX))
        return -22;
    // (the kernel reads guide_ctl[b] and two rows of guide_table[0 .. guide_rows - 1][0 .. 3], their indices clamped into
    // the table; one instantiation, the onsets kernel's with the live row and the cell row)
    if (a->guide_ctl != nullptr && (a->onset_ctl == nullptr || a->guide_table == nullptr || a->guide_rows < 1 ||
                                    a->guide_rows > GDE_ROWS_MAX))
        return -22;
    // (the kernel reads art_ctl[b], one row of art_table[0 .. art_rows - 1][0 .. 2], its index clamped into the table, and up
    // to two words per lane of guide_table, their row indices clamped likewise; one instantiation, the guide kernel's with
    // the row and the hold term)
    if (a->art_ctl != nullptr && (a->guide_ctl == nullptr || a->art_table == nullptr || a->art_rows < 1 ||
                                  a->art_rows > ART_ROWS_MAX))
        return -22;
    const SamplingRows rows{a->temperature_rows, a->top_k_rows, a->top_p_rows};
    const dim3 grid(a->nseq), block(64);
    // every kernel's parameters begin with the same fifteen, then (bias, ld_bias), then what its constraints add
    auto launch = [&](auto kernel, const float* bias, int ld_bias, auto... more) {
        COMMU_LAUNCH(kernel, grid, block, 0, stream, a->logits, a->ld, V, a->wrong, a->ldw, a->uniforms, a->active,
                     a->temperature, a->top_k, a->token, a->probs_out, a->ldp, a->top_p, rows, a->logp_out, bias, ld_bias,
                     more...);
    };
    // five kernels: without a bias / a grammar / a harmony table the launch is the one it always was (no added load, no
    // added register, no added argument); a sixth for the class-keyed controls, a seventh for the note order, an eighth
    // for the voice cap, a ninth for the note density, a tenth for the melodic interval, an eleventh for the onset templates,
    // a twelfth for the guide track, a thirteenth for the articulation
    if (a->art_ctl != nullptr) {
        launch(sample_topk_art_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl, a->voice_ctl, a->density_ctl, a->interval_ctl, a->onset_ctl, a->onset_table, a->onset_rows,
               a->guide_ctl, a->guide_table, a->guide_rows, a->art_ctl, a->art_table, a->art_rows);
    } else if (a->guide_ctl != nullptr) {
        launch(sample_topk_gde_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl, a->voice_ctl, a->density_ctl, a->interval_ctl, a->onset_ctl, a->onset_table, a->onset_rows,
               a->guide_ctl, a->guide_table, a->guide_rows);
    } else if (a->onset_ctl != nullptr) {
        launch(sample_topk_ons_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl, a->voice_ctl, a->density_ctl, a->interval_ctl, a->onset_ctl, a->onset_table, a->onset_rows);
    } else if (a->interval_ctl != nullptr) {
        launch(sample_topk_mel_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl, a->voice_ctl, a->density_ctl, a->interval_ctl);
    } else if (a->density_ctl != nullptr) {
        launch(sample_topk_den_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl, a->voice_ctl, a->density_ctl);
    } else if (a->voice_ctl != nullptr) {
        launch(sample_topk_vox_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl, a->voice_ctl);
    } else if (a->order_ctl != nullptr) {
        launch(sample_topk_ord_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl),
               a->order_ctl);
    } else if (a->cls_ctl != nullptr) {
        launch(sample_topk_cls_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl));
    } else if (a->harm != nullptr) {
        launch(sample_topk_harm_kernel, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq,
               a->harm, a->ld_harm, a->harm_on, a->chord_tok, a->ld_chord);
    } else if (a->gram != nullptr) {
        if (a->bias != nullptr) {
            launch(sample_topk_gram_kernel<true>, a->bias, a->ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq,
                   a->ld_seq);
        } else {
            launch(sample_topk_gram_kernel<false>, nullptr, 0, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq);
        }
    } else if (a->bias != nullptr) {
        launch(sample_topk_kernel<true>, a->bias, a->ld_bias);
    } else {
        launch(sample_topk_kernel<false>, nullptr, 0);
    }
    COMMU_LAUNCH_CHECK();
    return 0;
}
