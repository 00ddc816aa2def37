// Form templates (gfx950): the per-slot replay state of the forcing stage and what resets it, shared by the forcing kernels
// (decode_loop.h, forcing.hip) and the slot-array routine of the two arm launches (decode_arm.hip).
//
// form_state is int32 [B][FS_COUNT]: a header of FS_BAR_AT ints -- active, cursor, end, k (the phase inside the current note
// group), the open bar's row word, g (the group the last search found, -1: none), two reserved ints written 0 -- and
// bar_at[0 .. 63], the index in seq of the (i+1)-th BAR token, context and prompt included.
#pragma once

namespace {

constexpr int FORM_BARS = 64, FORM_ROWS_MAX = 4096;
enum { FS_ACTIVE = 0, FS_CURSOR, FS_END, FS_K, FS_ROW, FS_G, FS_BAR_AT = 8, FS_COUNT = FS_BAR_AT + FORM_BARS };

// One slot's state as a load or an arm leaves it: nothing is replayed (the bar a prompt leaves open is free), and bar_at holds
// the BARs of sq[0 .. len), so that a prompt's bars are valid sources.  One 64-lane wave; every int of the row has exactly
// one writer.  The trip count is wave-uniform (len is read through lane 0).
__device__ __forceinline__ void form_reset_row(int* __restrict__ fs, const int* __restrict__ sq, int len, int lane) {
    len = __builtin_amdgcn_readfirstlane(len);
    if (lane < FS_BAR_AT) fs[lane] = lane == FS_G ? -1 : 0;
    int nb = 0;
#pragma unroll 1
    for (int base = 0; base < len && nb < FORM_BARS; base += 64) {
        const int i = base + lane;
        const bool bar = i < len && sq[i < len ? i : 0] == 2;          // (TOK_BAR)
        const unsigned long long m = __ballot(bar);
        const int r = nb + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (bar && r < FORM_BARS) fs[FS_BAR_AT + r] = i;
        nb += __popcll(m);
    }
    if (lane >= nb) fs[FS_BAR_AT + lane] = 0;
}

}  // namespace
