// Host side of the constraint tiers (decode_loop.h: Tier), shared by the two entry points that launch the sampling step:
// commu_sample_topk (sample.hip) and commu_decode_sample_post_pre (forcing.hip).  Their argument structs name the constraint
// fields alike (commu_hip.h), so each function here is written once, over the struct.
#pragma once
#include <cstdint>
#include <type_traits>
#include "decode_loop.h"

namespace {

// the tier of a launch: the highest constraint whose pointer is given (check_constraints has seen to those below it)
template <class Args>
int tier_of(const Args& a) {
    return a.art_ctl != nullptr ? T_ART : a.guide_ctl != nullptr ? T_GDE : a.onset_ctl != nullptr ? T_ONS
         : a.interval_ctl != nullptr ? T_MEL : a.density_ctl != nullptr ? T_DEN : a.voice_ctl != nullptr ? T_VOX
         : a.order_ctl != nullptr ? T_ORD : a.cls_ctl != nullptr ? T_CLS : a.harm != nullptr ? T_HARM
         : a.gram != nullptr ? T_GRAM : T_NONE;
}

// what both entry points refuse (false: -22): a constraint without what its kernel reads, or without the tier below it
template <class Args>
bool check_constraints(const Args& a, int V) {
    if (a.bias != nullptr && a.ld_bias < V) return false;    // (the kernel reads bias[b][0 .. V-1])
    // (the kernel reads gram[0 .. 7][0 .. V-1] and finds the previous token through the record)
    if (a.gram != nullptr && (a.ld_gram < V || a.state == nullptr || a.seq == nullptr)) return false;
    // (the kernel reads harm[0 .. 110][0 .. 11] and finds the chord through the record: chord_tok[b][F_CUR - 1]; one
    // instantiation: the caller passes a zero bias and an all-off grammar where it has none)
    if (a.harm != nullptr && (a.ld_harm < 12 || a.chord_tok == nullptr || a.bias == nullptr || a.gram == nullptr))
        return false;
    // (the kernel reads cls_ctl[b][0 .. 7] as 16-byte records and finds the previous token through the record, as the
    // grammar does; one instantiation: it is the harmony kernel's caller that passes the zero bias and the all-off tables)
    if (a.cls_ctl != nullptr && (a.state == nullptr || a.seq == nullptr || a.bias == nullptr || a.gram == nullptr ||
                                 a.harm == nullptr || a.chord_tok == nullptr ||
                                 (reinterpret_cast<uintptr_t>(a.cls_ctl) & 15u) != 0))
        return false;
    // (the kernel reads order_ctl[b] and walks seq[b] backwards from the record's length; one instantiation, the class
    // kernel's with the scan: a caller without class controls passes the base-triple table)
    if (a.order_ctl != nullptr && a.cls_ctl == nullptr) return false;
    // (the kernel reads voice_ctl[b] and continues the note order's walk to the second BAR; one instantiation, the
    // note-order kernel's with the longer scan)
    if (a.voice_ctl != nullptr && a.order_ctl == nullptr) return false;
    // (the kernel reads density_ctl[b] and counts the open bar's notes on the voice cap's walk; one instantiation, the
    // voices kernel's with the count)
    if (a.density_ctl != nullptr && a.voice_ctl == nullptr) return false;
    // (the kernel reads interval_ctl[b] and finds the reference note on the voice cap's walk; one instantiation, the
    // density kernel's with the last note)
    if (a.interval_ctl != nullptr && a.density_ctl == nullptr) return false;
    // (the kernel reads onset_ctl[b] and one row of onset_table[0 .. onset_rows - 1][0 .. 3], its index clamped into the
    // table; one instantiation, the interval kernel's with the row)
    if (a.onset_ctl != nullptr && (a.interval_ctl == nullptr || a.onset_table == nullptr || a.onset_rows < 1 ||
                                   a.onset_rows > ONS_ROWS_MAX))
        return false;
    // (the kernel reads guide_ctl[b] and two rows of guide_table[0 .. guide_rows - 1][0 .. 3], their indices clamped into
    // the table; one instantiation, the onsets kernel's with the live row and the cell row)
    if (a.guide_ctl != nullptr && (a.onset_ctl == nullptr || a.guide_table == nullptr || a.guide_rows < 1 ||
                                   a.guide_rows > GDE_ROWS_MAX))
        return false;
    // (the kernel reads art_ctl[b], one row of art_table[0 .. art_rows - 1][0 .. 2], its index clamped into the table, and up
    // to two words per lane of guide_table, their row indices clamped likewise; one instantiation, the guide kernel's with
    // the row and the hold term)
    if (a.art_ctl != nullptr && (a.guide_ctl == nullptr || a.art_table == nullptr || a.art_rows < 1 ||
                                 a.art_rows > ART_ROWS_MAX))
        return false;
    return true;
}

// the runtime tier handed to f as a compile-time one: f(std::integral_constant<int, tier>{})
template <int T = T_NONE, class F>
void with_tier(int tier, F&& f) {
    if constexpr (T < T_ART) {
        if (tier != T) return with_tier<T + 1>(tier, f);
    }
    f(std::integral_constant<int, T>{});
}

}  // namespace
