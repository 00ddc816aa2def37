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
// heard of them.
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

}  // namespace

extern "C" int commu_sample_topk_topp_harm(float* logits, int ld, int nseq, int V, const unsigned char* wrong, int ldw,
                                           const float* uniforms, const unsigned char* active, float temperature,
                                           int top_k, float top_p, const float* temperature_rows, const int* top_k_rows,
                                           const float* top_p_rows, int* token, float* probs_out, int ldp,
                                           float* logp_out, const float* bias, int ld_bias, const float* gram, int ld_gram,
                                           const unsigned char* gram_on, const int* state, const int* seq, int ld_seq,
                                           const float* harm, int ld_harm, const unsigned char* harm_on,
                                           const int* chord_tok, int ld_chord, hipStream_t stream) {
    if (harm == nullptr)
        return commu_sample_topk_topp_gram(logits, ld, nseq, V, wrong, ldw, uniforms, active, temperature, top_k, top_p,
                                           temperature_rows, top_k_rows, top_p_rows, token, probs_out, ldp, logp_out, bias,
                                           ld_bias, gram, ld_gram, gram_on, state, seq, ld_seq, stream);
    if (nseq <= 0) return 0;
    // (the kernel reads harm[0 .. 110][0 .. 11] and finds the chord through the record: chord_tok[b][F_CUR - 1])
    if (ld_harm < 12 || state == nullptr || chord_tok == nullptr || ld_chord < 1) return -22;
    // (one instantiation: the caller passes a zero bias and an all-off grammar where it has none)
    if (bias == nullptr || ld_bias < V || gram == nullptr || ld_gram < V || seq == nullptr || ld_seq < 1) return -22;
    if (V > 64 * PER_LANE || V < 2 || (top_k_rows == nullptr && (top_k < 1 || top_k > V)) ||
        (top_p_rows == nullptr && !(top_p > 0.f)))
        return -22;
    const SamplingRows rows{temperature_rows, top_k_rows, top_p_rows};
    COMMU_LAUNCH(sample_topk_harm_kernel, dim3(nseq), dim3(64), 0, stream, logits, ld, V, wrong, ldw, uniforms, active,
                 temperature, top_k, token, probs_out, ldp, top_p, rows, logp_out, bias, ld_bias, gram, ld_gram, gram_on,
                 state, seq, ld_seq, harm, ld_harm, harm_on, chord_tok, ld_chord);
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_sample_topk_topp_gram(float* logits, int ld, int nseq, int V, const unsigned char* wrong, int ldw,
                                           const float* uniforms, const unsigned char* active, float temperature,
                                           int top_k, float top_p, const float* temperature_rows, const int* top_k_rows,
                                           const float* top_p_rows, int* token, float* probs_out, int ldp,
                                           float* logp_out, const float* bias, int ld_bias, const float* gram, int ld_gram,
                                           const unsigned char* gram_on, const int* state, const int* seq, int ld_seq,
                                           hipStream_t stream) {
    if (nseq <= 0) return 0;
    if (bias != nullptr && ld_bias < V) return -22;          // (the kernel reads bias[b][0 .. V-1])
    // (the kernel reads gram[0 .. 7][0 .. V-1] and finds the previous token through the record)
    if (gram != nullptr && (ld_gram < V || state == nullptr || seq == nullptr || ld_seq < 1)) return -22;
    // (a scalar that an array replaces is not looked at; the kernel clamps what the arrays hold)
    if (V > 64 * PER_LANE || V < 2 || (top_k_rows == nullptr && (top_k < 1 || top_k > V)) ||
        (top_p_rows == nullptr && !(top_p > 0.f)))
        return -22;
    const SamplingRows rows{temperature_rows, top_k_rows, top_p_rows};
    // four kernels: without a bias / a grammar the launch is the one it always was (no added load, no added register, no
    // added argument)
    if (gram != nullptr) {
        if (bias != nullptr) {
            COMMU_LAUNCH(sample_topk_gram_kernel<true>, dim3(nseq), dim3(64), 0, stream, logits, ld, V, wrong, ldw, uniforms,
                         active, temperature, top_k, token, probs_out, ldp, top_p, rows, logp_out, bias, ld_bias, gram, ld_gram,
                         gram_on, state, seq, ld_seq);
        } else {
            COMMU_LAUNCH(sample_topk_gram_kernel<false>, dim3(nseq), dim3(64), 0, stream, logits, ld, V, wrong, ldw, uniforms,
                         active, temperature, top_k, token, probs_out, ldp, top_p, rows, logp_out, nullptr, 0, gram, ld_gram,
                         gram_on, state, seq, ld_seq);
        }
    } else if (bias != nullptr) {
        COMMU_LAUNCH(sample_topk_kernel<true>, dim3(nseq), dim3(64), 0, stream, logits, ld, V, wrong, ldw, uniforms, active,
                     temperature, top_k, token, probs_out, ldp, top_p, rows, logp_out, bias, ld_bias);
    } else {
        COMMU_LAUNCH(sample_topk_kernel<false>, dim3(nseq), dim3(64), 0, stream, logits, ld, V, wrong, ldw, uniforms, active,
                     temperature, top_k, token, probs_out, ldp, top_p, rows, logp_out, nullptr, 0);
    }
    COMMU_LAUNCH_CHECK();
    return 0;
}

extern "C" int commu_sample_topk_topp_bias(float* logits, int ld, int nseq, int V, const unsigned char* wrong, int ldw,
                                           const float* uniforms, const unsigned char* active, float temperature,
                                           int top_k, float top_p, const float* temperature_rows, const int* top_k_rows,
                                           const float* top_p_rows, int* token, float* probs_out, int ldp,
                                           float* logp_out, const float* bias, int ld_bias, hipStream_t stream) {
    return commu_sample_topk_topp_gram(logits, ld, nseq, V, wrong, ldw, uniforms, active, temperature, top_k, top_p,
                                       temperature_rows, top_k_rows, top_p_rows, token, probs_out, ldp, logp_out, bias,
                                       ld_bias, nullptr, 0, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int commu_sample_topk_topp_rows(float* logits, int ld, int nseq, int V, const unsigned char* wrong, int ldw,
                                           const float* uniforms, const unsigned char* active, float temperature,
                                           int top_k, float top_p, const float* temperature_rows, const int* top_k_rows,
                                           const float* top_p_rows, int* token, float* probs_out, int ldp,
                                           float* logp_out, hipStream_t stream) {
    return commu_sample_topk_topp_bias(logits, ld, nseq, V, wrong, ldw, uniforms, active, temperature, top_k, top_p,
                                       temperature_rows, top_k_rows, top_p_rows, token, probs_out, ldp, logp_out, nullptr, 0,
                                       stream);
}

extern "C" int commu_sample_topk_topp(float* logits, int ld, int nseq, int V, const unsigned char* wrong, int ldw,
                                      const float* uniforms, const unsigned char* active, float temperature,
                                      int top_k, float top_p, int* token, float* probs_out, int ldp,
                                      hipStream_t stream) {
    return commu_sample_topk_topp_rows(logits, ld, nseq, V, wrong, ldw, uniforms, active, temperature, top_k, top_p, nullptr,
                                       nullptr, nullptr, token, probs_out, ldp, nullptr, stream);
}

extern "C" int commu_sample_topk(float* logits, int ld, int nseq, int V, const unsigned char* wrong, int ldw,
                                 const float* uniforms, const unsigned char* active, float temperature,
                                 int top_k, int* token, float* probs_out, int ldp, hipStream_t stream) {
    return commu_sample_topk_topp(logits, ld, nseq, V, wrong, ldw, uniforms, active, temperature, top_k, 1.f, token,
                                  probs_out, ldp, stream);
}
