// bs_layout.h -- the bit-sliced dense tile's register / lane layouts and the
// constants of its butterflies (rs_ff8_bs.hip), as host-side constexpr: which
// piece a register of a lane group holds in every layout, the skew of every
// butterfly and its twists, and the XOR network (gf8_net.h) each butterfly runs.
// The kernel and tests/gf8_const/gf8_net_dump.cpp read the same functions.
#pragma once

#include <cstdint>
#include <initializer_list>

#include "gf8_const.h"
#include "gf8_net.h"

namespace lamd {

// ------------------------------------------------------------ skews --------

constexpr unsigned sidx(unsigned p, unsigned l) { return ((p >> l) | 1u) << l; }
constexpr unsigned skew_at(int off, unsigned p, unsigned l) { return gf8_skew(off + int(sidx(p, l))); }

// ----------------------------------------------------------- layouts -------

// A layout says which piece-index bit each register-index bit (4) and each
// lane-group bit (3, g = lane >> 3) holds: piece(r, g) = the OR of bit i of r
// at position rb[i] and bit j of g at position gb[j].  Packed into a template
// argument: rb[i] in bits 3 i .. 3 i + 2, gb[j] in bits 12 + 3 j ...
constexpr uint32_t lay(unsigned r0, unsigned r1, unsigned r2, unsigned r3, unsigned g0, unsigned g1, unsigned g2) {
    return r0 | r1 << 3 | r2 << 6 | r3 << 9 | g0 << 12 | g1 << 15 | g2 << 18;
}
constexpr unsigned lay_rb(uint32_t L, unsigned i) { return (L >> (3 * i)) & 7u; }
constexpr unsigned lay_gb(uint32_t L, unsigned j) { return (L >> (12 + 3 * j)) & 7u; }
constexpr unsigned piece_of(uint32_t L, unsigned r, unsigned g) {
    unsigned p = 0;
    for (unsigned i = 0; i < 4; ++i) p |= ((r >> i) & 1u) << lay_rb(L, i);
    for (unsigned j = 0; j < 3; ++j) p |= ((g >> j) & 1u) << lay_gb(L, j);
    return p;
}
constexpr int reg_bit_of(uint32_t L, unsigned pbit) {
    for (unsigned i = 0; i < 4; ++i)
        if (lay_rb(L, i) == pbit) return int(i);
    return -1;
}
constexpr bool lay_ok(uint32_t L) {
    unsigned seen = 0;
    for (unsigned i = 0; i < 4; ++i) seen |= 1u << lay_rb(L, i);
    for (unsigned j = 0; j < 3; ++j) seen |= 1u << lay_gb(L, j);
    return seen == 127u;
}

// A layer-l skew depends on the piece bits above l only (sidx).  Those held
// by lane-group bits make it vary over the wave; it is affine in them
// (FFTInitialize builds FFTSkew[first + k 2^(l+1)] as the XOR of one generator
// per bit of k, LeopardFF8.cpp:505-514), so
//   c(r, g) * y = A_r * y  ^  sum over g bits j above l of  (g_j ? H_j * y : 0)
// with A_r = the skew of piece(r, 0) and H_j = the generator of bit gb[j]: the
// "twist", selected per lane by the all-ones masks G[j] (checked here for every
// layout the kernel uses).
//
// Wave bits (WB, the workgroup-cooperative tile below): the low WB bits of g
// are not lane bits but the wave's index in its workgroup, wv.  They are
// wave-uniform, so a code variant per wv folds them into A_r = the skew of
// piece(r, wv) and only the bits j >= WB are twisted.
constexpr unsigned twist_at(int off, uint32_t L, unsigned r, unsigned l, unsigned j, unsigned wv = 0) {
    const unsigned p = piece_of(L, r, wv);
    return lay_gb(L, j) > l ? skew_at(off, p | (1u << lay_gb(L, j)), l) ^ skew_at(off, p, l) : 0u;
}
constexpr bool affine_ok(uint32_t L, unsigned l, unsigned WB = 0) {
    for (int off : {-1, 127})
        for (unsigned r = 0; r < 16; ++r)
            for (unsigned g = 0; g < 8; ++g) {
                const unsigned wv = g & ((1u << WB) - 1u);
                unsigned v = skew_at(off, piece_of(L, r, wv), l);
                for (unsigned j = WB; j < 3; ++j)
                    if ((g >> j) & 1u) v ^= twist_at(off, L, r, l, j, wv);
                if (v != skew_at(off, piece_of(L, r, g), l)) return false;
            }
    return true;
}

// Layouts of the tile (LAMD_BS_SWAPS = 1, the default):
//   kLay0 (load / store, layer 0): registers = piece bits 0-3, lane groups 6, 5, 4;
//   kLay1 (layer 1): piece bit 0 <-> 4 exchanged (v_permlane32_swap: g bit 2 is lane bit 5);
//   kLay2 (layer 2): piece bit 1 <-> 5 exchanged (v_permlane16_swap: g bit 1 is lane bit 4);
//   kLayT (layers 3-6): piece bit 2 <-> 6 exchanged through LDS (g bit 0 is lane bit 3).
// Layer l then varies over the lane groups in 3, 2, 1, 0 bits (l = 0, 1, 2, >= 3),
// the fewest any 4-register-bit layout allows: 6 twisted (layer, bit) pairs per
// transform instead of 9.  LAMD_BS_SWAPS = 0 is the round-5 tile: layers 0-2 in
// kLay0 (lane groups 4, 5, 6), one LDS exchange of all three bits to kLayT.
#ifndef LAMD_BS_SWAPS
#define LAMD_BS_SWAPS 1
#endif
#if LAMD_BS_SWAPS
constexpr uint32_t kLay0 = lay(0, 1, 2, 3, 6, 5, 4);
constexpr uint32_t kLay1 = lay(4, 1, 2, 3, 6, 5, 0);
constexpr uint32_t kLay2 = lay(4, 5, 2, 3, 6, 1, 0);
constexpr uint32_t kLayT = lay(4, 5, 6, 3, 2, 1, 0);
#else
constexpr uint32_t kLay0 = lay(0, 1, 2, 3, 4, 5, 6);
constexpr uint32_t kLay1 = kLay0;
constexpr uint32_t kLay2 = kLay0;
constexpr uint32_t kLayT = lay(3, 4, 5, 6, 0, 1, 2);
#endif
static_assert(lay_ok(kLay0) && lay_ok(kLay1) && lay_ok(kLay2) && lay_ok(kLayT), "layouts are bit permutations");
static_assert(affine_ok(kLay0, 0) && affine_ok(kLay1, 1) && affine_ok(kLay2, 2), "skews are affine in the lane-group bits");
// the workgroup-cooperative tiles: two waves (g bit 0 = piece bit 6 is the wave)
// run the same layouts; four waves (g bits 0, 1 = piece bits 6, 5) have no lane
// bit to trade for piece bit 1 and run layer 2 in kLay1
static_assert(affine_ok(kLay0, 0, 1) && affine_ok(kLay1, 1, 1) && affine_ok(kLay2, 2, 1), "two-wave tile: every wave's variant");
static_assert(affine_ok(kLay0, 0, 2) && affine_ok(kLay1, 1, 2) && affine_ok(kLay1, 2, 2), "four-wave tile: every wave's variant");
static_assert(reg_bit_of(kLay1, 2) == 2 && reg_bit_of(kLay1, 3) == 3 && reg_bit_of(kLay2, 3) == 3, "register bit 3 = piece bit 3 in every low layout");

// The layout the low layers end in (and the exchange to kLayT starts from):
// with two wave bits g bit 1 is a wave bit, so piece bits 1 <-> 5 are not
// traded by a lane swap and layer 2 runs in kLay1.
template <int WB>
constexpr uint32_t kLayLow = WB == 2 ? kLay1 : kLay2;
constexpr uint32_t bs_low_layout(unsigned l, int WB) { return l == 0 ? kLay0 : l == 1 ? kLay1 : WB == 2 ? kLay1 : kLay2; }

// ------------------------------------------------- a butterfly's matrices --

// The butterfly of register r (the lower of its pair) of layer l in layout L,
// skew base off, in the code of wave wv of a tile with WB wave bits: the
// constant A and the twists H[j] of the lane-group bits j >= WB (0: none).
struct BsMats {
    uint64_t A, H[3];
};
constexpr BsMats bs_mats(int off, uint32_t L, unsigned r, unsigned l, int WB = 0, unsigned wv = 0) {
    BsMats m = {gf8_matrix(skew_at(off, piece_of(L, r, wv), l)), {0, 0, 0}};
    for (int j = WB; j < 3; ++j) m.H[j] = gf8_matrix(twist_at(off, L, r, l, unsigned(j), wv));
    return m;
}
// A butterfly x' = x ^ c y, y' = y ^ x' is also y' = x ^ (c ^ 1) y, x' = y' ^ y
// (and the inverse one alike, rs_ff8_bs.hip: butterfly): the same work with the
// two register groups renamed, so each runs the cheaper of the networks of c
// and c ^ 1 (the twists are the same).  True when c ^ 1 is the cheaper.
#ifndef LAMD_BS_ALT
#define LAMD_BS_ALT 1  // 0: every butterfly runs the network of c
#endif
constexpr bool bs_alt_form(const BsMats& m) {
    return LAMD_BS_ALT &&
           net_lookup(m.A ^ kGf8Identity, m.H[0], m.H[1], m.H[2]).gates < net_lookup(m.A, m.H[0], m.H[1], m.H[2]).gates;
}
constexpr int bs_gates(const BsMats& m) {
    return net_lookup(bs_alt_form(m) ? m.A ^ kGf8Identity : m.A, m.H[0], m.H[1], m.H[2]).gates;
}

// Gates of the constant-multiply networks per tile, times 8 (a lane runs 8 of a
// layer's 64 butterflies): both skew bases, layers 0-6 over the 64 butterfly
// groups p with bit l clear, without the twists (counted apart, DESIGN.md
// section 7.9) -- layer 6 of base 127 and of base -1 are one fused butterfly
// with the constant skew(127, 64, 6) ^ skew(-1, 64, 6).  Host side only (tests).
constexpr unsigned bs_tile_network_gates8() {
    int cost[256] = {};
    for (unsigned c = 0; c < 256; ++c) cost[c] = -1;
    const auto gates = [&](unsigned c) {
        if (cost[c] < 0) cost[c] = bs_gates(BsMats{gf8_matrix(c), {0, 0, 0}});
        return unsigned(cost[c]);
    };
    unsigned total = 0;
    for (int off : {-1, 127})
        for (unsigned l = 0; l < 7; ++l) {
            if (off == 127 && l == 6) continue;
            for (unsigned p = 0; p < 128; ++p)
                if (((p >> l) & 1u) == 0) total += gates(skew_at(off, p, l));
        }
    return total + 64u * gates(skew_at(127, 64, 6) ^ skew_at(-1, 64, 6));
}

}  // namespace lamd
