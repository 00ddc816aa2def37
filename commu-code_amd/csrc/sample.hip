// K15: the sampling step of the decode loop, one wave per sequence, no host round trip inside.
// Reference: commu/midi_generator/midi_inferrer.py:209-237
//   calc_probs    : logits[1:] /= temperature (IN PLACE, quirk Q5), softmax, left-pad 0 (Q6)
//                   (temperature == 0: one-hot at argmax)
//   apply_sampling: keep the top-k probabilities, zero the rejected ("wrong") tokens, renormalise
//   infer_token   : draw one token from the result -- here by inverse CDF with an injected
//                   uniform variate u[b] (torch.multinomial's stream is not reproducible).
// A sequence whose kept mass is 0 (Q12: greedy argmax is a rejected token) gets token -1.
// The controls may be per-sequence device arrays, and the step can report the log-probabilities of the token it drew
// (decode_loop.h: SamplingRows, TokenLogp).  What may be drawn is narrowed by a ladder of constraints, each of which needs all
// those before it: the TIER of a launch (decode_loop.h: Tier, and the comment block of each constraint there).  Two kernel
// templates: sample_topk_kernel<BIAS> is tier none -- the launch that never heard of a constraint, or only of the optional
// additive bias row -- and keeps its arguments to the byte; sample_topk_tier_kernel<BIAS, TIER> is every tier from the
// grammar up, with one flattened argument list of which a tier loads its own part only.
#include "sample_tier.h"
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

// every tier from the grammar up: ONE argument list, the whole ladder flattened (a struct by value changed the code
// materially); a launch of tier T loads none of the arguments of the tiers above it, and the host passes them as they are
template <bool BIAS, int TIER>
__global__ __launch_bounds__(64) void sample_topk_tier_kernel(
    float* __restrict__ logits, int ld, int V, const unsigned char* __restrict__ wrong, int ldw,
    const float* __restrict__ uni, const unsigned char* __restrict__ active, float temperature, int top_k,
    int* __restrict__ token, float* __restrict__ probs_out, int ldp, float top_p, SamplingRows rows,
    float* __restrict__ logp_out, const float* __restrict__ bias, int ld_bias, const float* __restrict__ gram, int ld_gram,
    const unsigned char* __restrict__ gram_on, const int* __restrict__ state, const int* __restrict__ seq, int ld_seq,
    const float* __restrict__ harm, int ld_harm, const unsigned char* __restrict__ harm_on,
    const int* __restrict__ chord_tok, int ld_chord, const int4* __restrict__ cls_ctl, const int* __restrict__ order_ctl,
    const int* __restrict__ voice_ctl, const int* __restrict__ density_ctl, const int* __restrict__ interval_ctl,
    const int* __restrict__ onset_ctl, const unsigned* __restrict__ onset_table, int onset_rows,
    const int* __restrict__ guide_ctl, const unsigned* __restrict__ guide_table, int guide_rows,
    const int* __restrict__ art_ctl, const unsigned* __restrict__ art_table, int art_rows) {
    static_assert(TIER >= T_GRAM, "tier none is sample_topk_kernel");
    TokenLogp lp;
    // What a tier reads of its sequence is loaded here: the record's fields, the switches and the control words (a null
    // switch array reads a valid byte of this sequence, which is then ignored); the previous token, the chord token, the
    // class record, the scan of seq and the table rows are the body's loads.
    const int b = blockIdx.x;
    const int* rec = state + (size_t)b * F_COUNT;
    auto on = [&](const unsigned char* sw) {
        const unsigned char v = *(sw != nullptr ? sw + b : reinterpret_cast<const unsigned char*>(token + b));
        return sw != nullptr ? (int)v : 1;
    };
    const Grammar g{gram, ld_gram, seq + (size_t)b * ld_seq, rec[F_LEN], ld_seq, on(gram_on)};
    Harmony h{nullptr, 0, nullptr, 0, 0, 0};
    if constexpr (TIER >= T_HARM) h = Harmony{harm, ld_harm, chord_tok + (size_t)b * ld_chord, rec[F_CUR], ld_chord, on(harm_on)};
    ClassControls cc{nullptr};
    if constexpr (TIER >= T_CLS) cc = ClassControls{cls_ctl + (size_t)b * 8};
    NoteOrder no{-1};
    if constexpr (TIER >= T_ORD) no = NoteOrder{order_ctl[b]};
    Voices vx{-1};
    if constexpr (TIER >= T_VOX) vx = Voices{voice_ctl[b]};
    Density dn{-1};
    if constexpr (TIER >= T_DEN) dn = Density{density_ctl[b]};
    Interval ml{-1};
    if constexpr (TIER >= T_MEL) ml = Interval{interval_ctl[b]};
    Onsets os{-1, nullptr, 1, 0};
    if constexpr (TIER >= T_ONS) os = Onsets{onset_ctl[b], onset_table, onset_rows, rec[F_NBAR]};
    Guide gd{-1, nullptr, 1};
    if constexpr (TIER >= T_GDE) gd = Guide{guide_ctl[b], guide_table, guide_rows};
    Articulation ar{-1, nullptr, 1};
    if constexpr (TIER >= T_ART) ar = Articulation{art_ctl[b], art_table, art_rows};
    sample_topk_body<BIAS, TIER>(b, threadIdx.x, logits, ld, V, wrong, ldw, uni, active, temperature, top_k, token, probs_out,
                                 ldp, top_p, rows, logp_out != nullptr, logp_out, lp, bias, ld_bias, g, h, cc, no, vx, dn, ml,
                                 os, gd, ar);
}

}  // namespace

extern "C" int commu_sample_args_bytes(void) { return (int)sizeof(commu_sample_args); }

// The one host entry point: validate once, then pick the kernel by the tier the constraint pointers give.
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
    if (!check_constraints(*a, V)) return -22;
    // (this launch takes the rows of seq and chord_tok from the caller, not from a decoder's buffers)
    if ((a->gram != nullptr && a->ld_seq < 1) || (a->harm != nullptr && a->ld_chord < 1)) return -22;
    const SamplingRows rows{a->temperature_rows, a->top_k_rows, a->top_p_rows};
    const dim3 grid(a->nseq), block(64);
    // every kernel's parameters begin with the same fifteen, then (bias, ld_bias), then what the tiers add
    auto launch = [&](auto kernel, const float* bias, int ld_bias, auto... more) {
        COMMU_LAUNCH(kernel, grid, block, 0, stream, a->logits, a->ld, V, a->wrong, a->ldw, a->uniforms, a->active,
                     a->temperature, a->top_k, a->token, a->probs_out, a->ldp, a->top_p, rows, a->logp_out, bias, ld_bias,
                     more...);
    };
    // without a constraint the launch is the one it always was (no added load, no added register, no added argument); below
    // the harmony tier a bias is optional and the launch without one is a kernel of its own
    with_tier(tier_of(*a), [&](auto t) {
        constexpr int T = decltype(t)::value;
        if constexpr (T == T_NONE) {
            if (a->bias != nullptr) launch(sample_topk_kernel<true>, a->bias, a->ld_bias);
            else launch(sample_topk_kernel<false>, nullptr, 0);
        } else {
            auto tier = [&](auto kernel, const float* bias, int ld_bias) {
                launch(kernel, bias, ld_bias, a->gram, a->ld_gram, a->gram_on, a->state, a->seq, a->ld_seq, a->harm, a->ld_harm,
                       a->harm_on, a->chord_tok, a->ld_chord, static_cast<const int4*>(a->cls_ctl), a->order_ctl, a->voice_ctl,
                       a->density_ctl, a->interval_ctl, a->onset_ctl, a->onset_table, a->onset_rows, a->guide_ctl,
                       a->guide_table, a->guide_rows, a->art_ctl, a->art_table, a->art_rows);
            };
            if constexpr (T == T_GRAM) {
                if (a->bias == nullptr) return tier(sample_topk_tier_kernel<false, T>, nullptr, 0);
            }
            tier(sample_topk_tier_kernel<true, T>, a->bias, a->ld_bias);
        }
    });
    COMMU_LAUNCH_CHECK();
    return 0;
}
