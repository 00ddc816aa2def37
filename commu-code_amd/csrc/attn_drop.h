// The attention-probability dropout mask (K16): DropLane and its constants, shared by relattn.hip (16x16 MFMA layout) and
// train_f32.hip (fp32 training: one element at a time).  relattn3.hip / relattn_q3.hip derive the same mask in their
// transposed layouts from the same constants.
#pragma once
#include "common.h"

namespace {

// Attention-probability dropout (K16), ONE mask for every attention kernel (both forward generations, backward).
// keep(b, h, i, j): every 32x32 block (i >> 5, j >> 5) of a (batch, head) has a 32-bit key k1 from the strong hash -- block
// coordinates are wave-uniform in all kernels, so that is SCALAR work -- and inside the block a two-round hash on full-rate
// 24-bit multiplies: one mixed word per 2 x 2 cell,
//     y = ((i & 31) >> 1 << 4 | (j & 31) >> 1) * C1 + k1;  y ^= y >> 12;  y &= 0xFFFFFF
// and one multiply-add per element whose constants depend on the element's place in the cell,
//     w = y * CM[i & 1][j & 1] + (k1 * KA[i & 1][j & 1] + KB[i & 1][j & 1]);     keep = w >= round(p * 65536) << 16.
// Whichever two elements of a cell a lane holds -- two ROWS of one key in the 16x16 layout (registers 0,1 / 2,3), two KEYS of
// one query in the transposed 32x32 layout -- share the first round: 2.5 instructions per element in either layout, so the
// forward of one generation and the backward of the other regenerate the same mask.  (Before: one word per row pair in
// the 16x16 family and one per key pair in relattn3.hip -- two masks, and the faster forward unusable in training.)
// Host mirror: ops.attn_dropout_keep_mask.
constexpr unsigned DROP_C1 = 0xD2B74Bu;
constexpr unsigned DROP_CM[2][2] = {{0x9E3779u, 0x85EBCBu}, {0xC2B2AFu, 0xB5297Bu}};
constexpr unsigned DROP_KA[2][2] = {{0x85EBCA6Bu, 0xC2B2AE35u}, {0x27D4EB2Fu, 0x165667B1u}};
constexpr unsigned DROP_KB[2][2] = {{0x6A09E667u, 0xBB67AE85u}, {0x3C6EF372u, 0xA54FF53Au}};
struct DropLane {
    unsigned xc[2];        // ((2 g + rp) << 4 | r16 >> 1) * C1: the lane's two cells of a 16x16 tile (C layout: rows 4g + reg)
    unsigned cm[2];        // CM[row parity][this lane's key parity]
    bool jodd;
    unsigned key_bh;
    __device__ __forceinline__ void init(unsigned seed, int b, int h, int H, int g, int r16) {
        key_bh = mix32(seed + (unsigned)(b * H + h) * 0x9E3779B1u);
        xc[0] = (unsigned)(((2 * g) << 4) | (r16 >> 1)) * DROP_C1;
        xc[1] = (unsigned)(((2 * g + 1) << 4) | (r16 >> 1)) * DROP_C1;
        jodd = (r16 & 1) != 0;
        cm[0] = jodd ? DROP_CM[0][1] : DROP_CM[0][0];
        cm[1] = jodd ? DROP_CM[1][1] : DROP_CM[1][0];
    }
    // hash words of the lane's four elements (rows 4g + reg) of the 16x16 tile (ib, jb) = (i >> 4, j >> 4); both wave-uniform
    __device__ __forceinline__ void words(int ib, int jb, unsigned (&hw)[4]) const {
        const unsigned k1 = mix32k(((unsigned)(ib >> 1) << 16) | (unsigned)(jb >> 1), key_bh);
        // (the tile's place inside its 32x32 block: + 8 row pairs / + 8 key pairs, folded into the additive key)
        const unsigned kk = k1 + (unsigned)((((ib & 1) << 3) << 4) | ((jb & 1) << 3)) * DROP_C1;
        const unsigned ke0 = k1 * DROP_KA[0][0] + DROP_KB[0][0], ko0 = k1 * DROP_KA[0][1] + DROP_KB[0][1];
        const unsigned ke1 = k1 * DROP_KA[1][0] + DROP_KB[1][0], ko1 = k1 * DROP_KA[1][1] + DROP_KB[1][1];
        const unsigned kr0 = jodd ? ko0 : ke0, kr1 = jodd ? ko1 : ke1;
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            unsigned y = xc[rp] + kk;
            y ^= y >> 12;
            y &= 0xFFFFFFu;
            hw[2 * rp] = y * cm[0] + kr0;
            hw[2 * rp + 1] = y * cm[1] + kr1;
        }
    }
};

}  // namespace
