// rs_ff8_bs.hip -- bit-sliced GF(2^8) dense tile for gfx950: batches of K = R = m = 128
// codes (the benchmark's 128 + 128 shape), encode and full-loss decode.
//
// Reference path: ReedSolomonEncode (LeopardFF8.cpp:1602-1672) with one chunk,
//   out = FFT_{-1}( IFFT_{m-1}(data) )            (IFFT_DIT / FFT_DIT, :595-666, :1319-1390)
// and its inverse for a full-loss decode of such a code (rs_ff8.hip:
// launch_ff8_decode_full), data = FFT_{m-1}( IFFT_{-1}(recovery) ).
//
// Why bit slices.  In the byte layout of rs_ff8.hip a multiply by a constant c
// costs 3 v_perm_b32 + 5 selector ops + 2 XORs per 4 elements, and the tile is
// bound by VALU issue.  Here a lane holds 32 elements of
// a piece as 8 bit planes (plane k = bit k of 32 elements), so x ^= c * y is
// the 8 x 8 GF(2) matrix of c applied to the planes: plane i of x takes the XOR
// of the planes j of y that row i selects.  Every skew of the dense tile is
// known at compile time (gf8_const.h), so most butterflies compile to a fixed
// XOR network (~4x cheaper than the byte form, tools/ubench_bitslice8.hip),
// synthesized with shared subexpressions (gf8_net.h; the layouts and every
// butterfly's constants: bs_layout.h).
//
// Tile: ONE wave owns the whole 128-piece transform over a 256-byte column
// strip of every piece.  Lane = 8 * g + l: lane group g (8 groups), lane l of
// the group holds bytes [16 l, 16 l + 16) and [128 + 16 l, 128 + 16 l + 16) of
// the strip (32 elements = 8 dwords -> 8 planes) of 16 pieces:
//   layout 0   (load, IFFT layers 0-2, FFT layers 2-0, store): register r holds
//              piece r | g << 4 (piece bits 0-3 in registers, bits 4-6 = g);
//   layout top (IFFT layers 3-5, fused top layer 6, FFT layers 5-3): register r
//              holds piece g | r << 3 (bits 3-6 in registers, bits 0-2 = g).
// A layer-l butterfly group's skew depends on the piece bits above l only
// (skew index ((i >> l) | 1) << l).  In layout top those are register bits:
// every multiplier is a compile-time constant.  In layout 0 the bits 4-6 come
// from the lane group; the skews are affine in those bits (FFTInitialize builds
// FFTSkew[first + k * 2^(l+1)] as the XOR of one generator per bit of k,
// LeopardFF8.cpp:505-514; checked by static_assert below), so
//   c(g) * y = A * y  ^  sum over bits b of g of  (g_b ? H_b * y : 0)
// with A and H_b compile time and the selection by per-lane masks (v_bitop3).
// The two layouts are exchanged through a wave-private LDS area (no barrier:
// one wave's LDS operations execute in order).  No tables, no workgroup
// barriers: waves are independent, several per SIMD.
//
// Workgroup-cooperative tile (WB wave bits, the product's batches run WB = 2):
// the 1 << WB waves of a workgroup share one tile over a (256 << WB)-byte
// strip.  A piece bit is then held by a register bit (4), a lane-group bit
// (3 - WB) or the wave's index (WB).  A wave bit is wave-uniform: a code variant
// per wave folds it into the constant A, so only 3 - WB lane bits are twisted
// (WB = 2: one masked network in layer 0, none in layers 1-2).  The exchange
// to layout top crosses the waves: one LDS area per workgroup, barriers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "bs_layout.h"
#include "gf8_const.h"
#include "gf8_net.h"
#include "rs_args.h"

namespace lamd {

namespace {

#ifndef LAMD_BS_WAVES
#define LAMD_BS_WAVES 4  // independent tiles (waves) per workgroup
#endif
#ifndef LAMD_BS_OCC
#define LAMD_BS_OCC 2  // waves per SIMD the register budget is sized for
#endif
constexpr int kBsWaves = LAMD_BS_WAVES;
constexpr unsigned kBsBlocksPerCu = 4 * LAMD_BS_OCC / kBsWaves;  // workgroups per CU (LAMD_BS_OCC waves per SIMD)
constexpr unsigned kBsStrip = 256;           // bytes of every piece per wave
constexpr unsigned kBsAreaDw = (128 + 8) * 8 * 2;  // LDS dwords per wave: 136 rows x 8 lanes x 2 planes
#ifndef LAMD_BS_SCHED
#define LAMD_BS_SCHED 1  // 1: a scheduling barrier after every butterfly (bounds the temporaries in flight)
#endif
LDEV void bs_fence() {
    if constexpr (LAMD_BS_SCHED) __builtin_amdgcn_sched_barrier(0);
}
#ifndef LAMD_BS_XFENCE
#define LAMD_BS_XFENCE 1  // transposes between scheduling barriers
#endif
#ifndef LAMD_BS_BFENCE
#define LAMD_BS_BFENCE 1  // butterflies between scheduling barriers
#endif
template <int N>
LDEV void bs_fence_every(int i) {
    if ((i + 1) % N == 0) bs_fence();
}

// ---------------------------------------------------------- bit planes -----

// v_bitop3_b32 truth tables: index = 4 * src0 + 2 * src1 + src2
LDEV uint32_t sel_b(uint32_t a, uint32_t b, uint32_t m) { return __builtin_amdgcn_bitop3_b32(a, b, m, 0xD8); }  // m ? b : a
LDEV uint32_t xor_and(uint32_t a, uint32_t b, uint32_t m) { return __builtin_amdgcn_bitop3_b32(a, b, m, 0x78); }  // a ^ (b & m)

// The transpose's three bit masks in VGPRs: v_bitop3_b32 with an SGPR (or
// literal) operand issues at ~4.2 cycles a wave64 instruction against ~2.5
// with three VGPRs (tools/ubench_issue.hip).
struct XMasks {
    uint32_t m4, m2, m1;
    LDEV XMasks() : m4(0x0F0F0F0Fu), m2(0x33333333u), m1(0x55555555u) {
        asm volatile("" : "+v"(m4), "+v"(m2), "+v"(m1));
    }
};
// Delta-swap stage S on register pairs (lo[i], hi[i]), i = 0, 1, 2, 3: the
// MASK << S bits of lo[i] are exchanged with the MASK bits of hi[i]:
//   lo' = MASK ? lo : hi << S,   hi' = MASK ? lo >> S : hi.
// The shifts run as 64-bit shifts of register pairs (hi[0], hi[1]) and
// (lo[0], lo[1]) (a shift costs ~4 cycles a wave64 instruction whatever its
// width): the bits one dword's shift carries into its neighbour land only where
// the select takes the other operand (MASK has its top S bits clear and MASK << S
// its low S bits).
template <int S>
LDEV void dstage(uint32_t* const (&lo)[4], uint32_t* const (&hi)[4], uint32_t mask) {
    uint32_t hs[4], ls[4];
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        // raw 64-bit shifts (the compiler would keep the carried bits exact
        // with v_alignbit / v_or pairs)
        v2u h0, l0, h, l;
        h0.x = *hi[i], h0.y = *hi[i + 1];
        l0.x = *lo[i], l0.y = *lo[i + 1];
        asm("v_lshlrev_b64 %0, %1, %2" : "=v"(h) : "i"(S), "v"(h0));
        asm("v_lshrrev_b64 %0, %1, %2" : "=v"(l) : "i"(S), "v"(l0));
        hs[i] = h.x, hs[i + 1] = h.y;
        ls[i] = l.x, ls[i + 1] = l.y;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t a = *lo[i], b = *hi[i];
        *lo[i] = sel_b(hs[i], a, mask);
        *hi[i] = sel_b(b, ls[i], mask);
    }
}
// Exact 8 x 8 bit transpose in each byte lane of 8 dwords: afterwards plane k
// bit (8 p + r) = bit k of byte p of dword r.  An involution (bytes <-> planes).
// The three stages commute (each exchanges one register-index bit with one
// bit-in-byte index bit).
LDEV void transpose8(uint32_t* v, const XMasks& m) {
#ifdef ABL_XPOSE
    return;
#endif
    dstage<4>({&v[0], &v[1], &v[2], &v[3]}, {&v[4], &v[5], &v[6], &v[7]}, m.m4);
    dstage<2>({&v[0], &v[1], &v[4], &v[5]}, {&v[2], &v[3], &v[6], &v[7]}, m.m2);
    dstage<1>({&v[0], &v[4], &v[2], &v[6]}, {&v[1], &v[5], &v[3], &v[7]}, m.m1);
}

LDEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
// Keep a value materialised here: the networks are all XORs, and without a
// fence the compiler reassociates them across butterflies and layers into
// long-lived shared subexpressions (200+ VGPRs instead of the tile's 128).
LDEV void pin8(uint32_t* v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(v[k]));
}

// Variable V of a network (gf8_net.h): a plane of y or a temporary.
template <int V>
LDEV uint32_t net_var(const uint32_t* y, const uint32_t* t) {
    if constexpr (V < 8)
        return y[V];
    else
        return t[V - 8];
}
// acc ^ (XOR of the variables of `mask`), as 3-input XORs
template <uint32_t mask>
LDEV uint32_t fold(uint32_t acc, const uint32_t* y, const uint32_t* t) {
    if constexpr (mask == 0) {
        return acc;
    } else {
        constexpr int J = __builtin_ctz(mask);
        constexpr uint32_t rest = mask & (mask - 1u);
        if constexpr (rest == 0) {
            return acc ^ net_var<J>(y, t);
        } else {
            constexpr int K = __builtin_ctz(rest);
            return fold<(rest & (rest - 1u))>(xor3(acc, net_var<J>(y, t), net_var<K>(y, t)), y, t);
        }
    }
}
// XOR of the variables of `mask` (not empty)
template <uint32_t mask>
LDEV uint32_t fold_of(const uint32_t* y, const uint32_t* t) {
    return fold<(mask & (mask - 1u))>(net_var<__builtin_ctz(mask)>(y, t), y, t);
}

// x ^= A y ^ ((H0 y) & G[0]) ^ ((H1 y) & G[1]) ^ ((H2 y) & G[2]): the constant
// and the twists of one butterfly (compile time; G: per-lane all-ones /
// all-zeros masks) as ONE synthesized XOR network, whose temporaries the four
// products share.  The temporaries die here.
template <uint64_t A, uint64_t H0 = 0, uint64_t H1 = 0, uint64_t H2 = 0>
LDEV void mac(uint32_t* x, const uint32_t* y, const uint32_t (&G)[3]) {
    using N = Gf8NetOf<A, H0, H1, H2>;
    uint32_t t[kNetMaxTemps];
    static_for<0, N::net.ntemp>([&](auto K) {
        constexpr int k = decltype(K)::value;
        t[k] = fold_of<N::net.temp[k]>(y, t);
    });
    static_for<0, 8>([&](auto I) {
        constexpr int i = decltype(I)::value;
        x[i] = fold<N::net.row[0][i]>(x[i], y, t);
        static_for<1, kNetMats>([&](auto MI) {
            constexpr int m = decltype(MI)::value;
            if constexpr (N::net.row[m][i] != 0) x[i] = xor_and(x[i], fold_of<N::net.row[m][i]>(y, t), G[m - 1]);
        });
    });
}

#ifndef LAMD_BS_QUEUE
#define LAMD_BS_QUEUE 1  // tile queues (0: every wave codes tiles i, i + n, i + 2 n, ...)
#endif

// ----------------------------------------------------------- butterflies ---

using Reg = uint32_t[16][8];

LDEV void xor8(uint32_t* x, const uint32_t* y) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] ^= y[k];
}
LDEV void swap8(uint32_t* x, uint32_t* y) {  // a renaming: the indices are compile time
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t v = x[k];
        x[k] = y[k];
        y[k] = v;
    }
}
// One butterfly with the multiplier c(g) = M.A ^ the twists M.H the masks G select:
//   FFT_DIT2   a' = a ^ c b, b' = b ^ a'     or, the same,  b' = a ^ (c ^ 1) b, a' = b' ^ b;
//   IFFT_DIT2  b' = a ^ b,   a' = a ^ c b'   or, the same,  b' = a ^ b, a' = b ^ (c ^ 1) b'.
// The second forms leave a' and b' in each other's registers, which costs
// nothing (register names are compile time), so the butterfly runs the network
// of c or of c ^ 1, whichever has fewer gates (bs_alt_form).
template <bool kInverse, uint64_t A, uint64_t H0, uint64_t H1, uint64_t H2>
LDEV void butterfly(uint32_t* a, uint32_t* b, const uint32_t (&G)[3]) {
#ifdef ABL_MASKED
    constexpr BsMats M = {A, {0, 0, 0}};
#else
    constexpr BsMats M = {A, {H0, H1, H2}};
#endif
    // bs_alt_form(M), by the networks this file instantiates anyway
    constexpr bool kAlt = LAMD_BS_ALT && Gf8NetOf<(M.A ^ kGf8Identity), M.H[0], M.H[1], M.H[2]>::net.gates <
                                             Gf8NetOf<M.A, M.H[0], M.H[1], M.H[2]>::net.gates;
    if constexpr (!kAlt) {
        if constexpr (kInverse) xor8(b, a);
        mac<M.A, M.H[0], M.H[1], M.H[2]>(a, b, G);
        if constexpr (!kInverse) xor8(b, a);
    } else if constexpr (kInverse) {
        xor8(a, b);
        mac<(M.A ^ kGf8Identity), M.H[0], M.H[1], M.H[2]>(b, a, G);
        swap8(a, b);
    } else {
        mac<(M.A ^ kGf8Identity), M.H[0], M.H[1], M.H[2]>(a, b, G);
        xor8(b, a);
        swap8(a, b);
    }
}

// Layer L in layout LAY: the pairs (r, r + 2^i) over the register bit i that
// holds piece bit L, restricted to the half of register bit 3 = H (H < 0: all
// 16 registers; the low layers never pair across it, it holds piece bit 3).
// WB, WV: the low WB bits of g are wave bits and this is the code of wave WV.
template <bool kInverse, int kOff, int L, uint32_t LAY, int H = -1, int WB = 0, unsigned WV = 0>
LDEV void layer(Reg& x, const uint32_t (&G)[3]) {
    constexpr int ib = reg_bit_of(LAY, L);
    static_assert(ib >= 0, "the layer's bit is a register bit");
    constexpr unsigned half = 1u << ib;
    static_for<0, 16>([&](auto RI) {
        constexpr unsigned r = decltype(RI)::value;
        if constexpr ((r & half) == 0 && (H < 0 || int(r >> 3) == H)) {
            constexpr BsMats M = bs_mats(kOff, LAY, r, L, WB, WV);
            butterfly<kInverse, M.A, M.H[0], M.H[1], M.H[2]>(x[r], x[r + half], G);
            pin8(x[r]);
            pin8(x[r + half]);
            bs_fence_every<LAMD_BS_BFENCE>(int(r));
        }
    });
}
// The top IFFT layer (skew base kOffI) and the top FFT layer (kOffF) on the
// same pairs as one butterfly with multiplier c1 + c2 (as Tile::fused_top):
// y1 = y ^ x, x2 = x ^ (c1 + c2) y1, y2 = y1 ^ x2.  Piece bit 6 is a register
// bit of kLayT and the skews of layer 6 are the same for every pair.
template <int kOffI, int kOffF>
LDEV void fused_top(Reg& x, const uint32_t (&G)[3]) {
    constexpr int ib = reg_bit_of(kLayT, 6);
    constexpr unsigned half = 1u << ib;
    constexpr uint64_t E = gf8_matrix(skew_at(kOffI, 64, 6) ^ skew_at(kOffF, 64, 6));
    static_for<0, 16>([&](auto RI) {
        constexpr unsigned r = decltype(RI)::value;
        if constexpr ((r & half) == 0) {
            xor8(x[r + half], x[r]);
            butterfly<false, E, 0, 0, 0>(x[r], x[r + half], G);
            pin8(x[r]);
            pin8(x[r + half]);
            bs_fence_every<LAMD_BS_BFENCE>(int(r));
        }
    });
}

// --------------------------------------------------------- exchanges -------

// Register bit IB <-> lane-group bit 2 (lane bit 5, v_permlane32_swap) or 1
// (lane bit 4, v_permlane16_swap) on the registers of half H (register bit 3):
// for each pair (R0, R1) over bit IB the swap leaves R0 = [R0 lanes with the
// bit clear, R1 lanes with it clear], R1 = [R0 set, R1 set] -- the two bits
// trade places, as one VALU instruction per dword pair.
template <int IB, int GBIT, int H>
LDEV void swap_lanes(Reg& x) {
    static_assert(GBIT == 1 || GBIT == 2, "permlane swaps exist for lane bits 4 and 5");
#if defined(ABL_XCH) || defined(ABL_SWAP)
    return;
#endif
    static_for<0, 16>([&](auto RI) {
        constexpr unsigned r = decltype(RI)::value;
        if constexpr (((r >> IB) & 1u) == 0 && int(r >> 3) == H) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if constexpr (GBIT == 2) {
                    const auto v = __builtin_amdgcn_permlane32_swap(x[r][k], x[r | (1u << IB)][k], false, false);
                    x[r][k] = v[0];
                    x[r | (1u << IB)][k] = v[1];
                } else {
                    const auto v = __builtin_amdgcn_permlane16_swap(x[r][k], x[r | (1u << IB)][k], false, false);
                    x[r][k] = v[0];
                    x[r | (1u << IB)][k] = v[1];
                }
            }
        }
    });
}

// Layout FROM -> TO through the wave's LDS area, in 4 rounds of 2 planes: every
// register of every lane written at (piece, lane column) in FROM and read back
// at (piece, lane column) in TO.  Byte address of piece p, column l:
//   64 (p + pad(p)) + 8 l,  pad(p) = p >> 4 for the round-5 tile (its lane groups
// hold pieces 16 apart) and 0 otherwise,
// so that the 8 lane groups of one access fall in 4 different 64-byte bank
// windows (two lanes per bank: the minimum for 8-byte accesses).  The
// per-register part is a compile-time offset (the ds instruction's immediate).
constexpr unsigned kBsPad = LAMD_BS_SWAPS ? 0u : 1u;
constexpr unsigned lds_row(unsigned p) { return p + (kBsPad ? (p >> 4) : 0u); }
template <uint32_t FROM, uint32_t TO>
LDEV void exchange(Reg& x, uint8_t* area, unsigned g, unsigned l) {
#if defined(ABL_XCH) || defined(ABL_LDSX)
    return;
#endif
    Reg y;
    // lane parts: the lane-group bits of FROM / TO (disjoint from every register's
    // piece bits, so row(p(r, g)) = row(p(r, 0)) + row part of g when unpadded;
    // padded rows are exact because the round-5 lane bits are the high bits)
    uint8_t* const wbase = area + 64u * lds_row(piece_of(FROM, 0, g)) + 8u * l;
    uint8_t* const rbase = area + 64u * lds_row(piece_of(TO, 0, g)) + 8u * l;
    static_for<0, 4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        static_for<0, 16>([&](auto RI) {
            constexpr unsigned r = decltype(RI)::value;
            v2u v;
            v.x = x[r][2 * q];
            v.y = x[r][2 * q + 1];
            *reinterpret_cast<v2u*>(wbase + 64u * (lds_row(piece_of(FROM, r, 0)) - lds_row(0))) = v;
        });
        // one wave's LDS operations execute in order: the reads below see the
        // writes above, and the next round's writes follow these reads
        asm volatile("" ::: "memory");
        static_for<0, 16>([&](auto RI) {
            constexpr unsigned r = decltype(RI)::value;
            const v2u v = *reinterpret_cast<const v2u*>(rbase + 64u * (lds_row(piece_of(TO, r, 0)) - lds_row(0)));
            y[r][2 * q] = v.x;
            y[r][2 * q + 1] = v.y;
        });
        asm volatile("" ::: "memory");
    });
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) x[r][k] = y[r][k];
}

// The workgroup-cooperative tile (WB wave bits, 1 << WB waves): the same
// exchange through ONE area of the workgroup, because the low WB bits of g are
// the wave: a register's dwords go to another wave.  A wave has 8 << WB column
// lanes, so piece p, column l is at byte (64 << WB) p + 8 l (32 column lanes
// of 8 bytes cover all 64 banks once).  One round is 8 KiB << WB; a barrier
// between a round's writes and its reads, and one before the next round's
// writes.  Every wave of the workgroup runs every barrier: nothing here may
// depend on anything but WB.
template <int WB>
constexpr unsigned kBsWgAreaBytes = 128u * (64u << WB);
template <uint32_t FROM, uint32_t TO, int WB>
LDEV void exchange_wg(Reg& x, uint8_t* area, unsigned g, unsigned l) {
#if defined(ABL_XCH) || defined(ABL_LDSX)
    __syncthreads();
    return;
#endif
    constexpr unsigned kRow = 64u << WB;
    Reg y;
    uint8_t* const wbase = area + kRow * piece_of(FROM, 0, g) + 8u * l;
    uint8_t* const rbase = area + kRow * piece_of(TO, 0, g) + 8u * l;
    static_for<0, 4>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        static_for<0, 16>([&](auto RI) {
            constexpr unsigned r = decltype(RI)::value;
            v2u v;
            v.x = x[r][2 * q];
            v.y = x[r][2 * q + 1];
            *reinterpret_cast<v2u*>(wbase + kRow * piece_of(FROM, r, 0)) = v;
        });
        __syncthreads();
        static_for<0, 16>([&](auto RI) {
            constexpr unsigned r = decltype(RI)::value;
            const v2u v = *reinterpret_cast<const v2u*>(rbase + kRow * piece_of(TO, r, 0));
            y[r][2 * q] = v.x;
            y[r][2 * q + 1] = v.y;
        });
        __syncthreads();
    });
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) x[r][k] = y[r][k];
}

// ---------------------------------------------------------- tile I/O -----

// Where one tile (object, 256-byte column strip) lives for this lane.
#ifndef LAMD_BS_NT
#define LAMD_BS_NT 3  // nontemporal piece loads (1) and stores (2): +4% on the headline (profiles/r05_v6/nt_ab.txt)
#endif
// Where one tile (object, 256-byte column strip) lives for this lane: the
// strip's column in piece 0 of the object's input / output slab (wave-uniform,
// scalar registers), the slab strides (uniform) and the lane's offsets from
// there: its lane group's first piece, piece_of(kLay0, 0, g), plus its two
// 16-byte segments (a segment past the piece's end re-reads segment 0).  Piece
// register r is at column + r * stride + lane offset: the per-register part is
// scalar arithmetic.  kNarrow (every stride in [0, 2^32 / 128)): 32-bit lane
// offsets, so a load or store is one global_*_dwordx4 with a scalar base and
// a 32-bit vector offset (no 64-bit vector address per instruction).
template <bool kNarrow>
struct BsTile {
    using Off = std::conditional_t<kNarrow, uint32_t, int64_t>;
    uint64_t in, out;
    int32_t in_stride, out_stride;
    Off in0, in1, out0, out1;
};
// WB wave bits: the strip is 256 << WB bytes over the wave's 8 << WB column
// lanes l (the same strip for every wave of the workgroup; the waves differ in
// g), its two segments half a strip apart.
template <bool kNarrow, int WB = 0>
LDEV BsTile<kNarrow> bs_tile(const Ff8SlabBatch& b, unsigned t, unsigned strips, unsigned g, unsigned l) {
    using Off = typename BsTile<kNarrow>::Off;
    constexpr unsigned kStrip = kBsStrip << WB;
    const unsigned obj = t / strips, strip = t - obj * strips;
    const uint32_t rem = b.nunits * 4u - strip * kStrip;  // >= 64 (bytes % 64 == 0)
    const uint32_t o0 = 16u * l, o1 = kStrip / 2 + 16u * l;
    const uint32_t s0 = o0 + 16u <= rem ? o0 : 0u, s1 = o1 + 16u <= rem ? o1 : 0u;
    BsTile<kNarrow> T;
    T.in_stride = b.in_stride[obj];
    T.out_stride = b.out_stride[obj];
    const uint64_t col = uint64_t(strip) * kStrip;
    T.in = b.in_base[obj] + col;
    T.out = b.out_base[obj] + col;
    const Off pg = Off(piece_of(kLay0, 0, g));  // the lane group's pieces: pg | r
    T.in0 = pg * Off(T.in_stride) + s0;
    T.in1 = pg * Off(T.in_stride) + s1;
    T.out0 = pg * Off(T.out_stride) + s0;
    T.out1 = pg * Off(T.out_stride) + s1;
    return T;
}
template <class Off>
LDEV auto bs_addr(uint64_t base_r, Off off) {  // a global (address space 1) pointer
    if constexpr (std::is_same_v<Off, uint32_t>)
        return gptr<v4u>(reinterpret_cast<uint8_t*>(base_r) + uint64_t(off));
    else
        return gptr<v4u>(reinterpret_cast<uint8_t*>(base_r) + off);
}
// One piece register r (piece r | piece_of(kLay0, 0, g)) of a tile: a lane
// group reads 128 contiguous bytes per instruction.
template <bool kNarrow>
LDEV void load_reg(uint32_t* v, const BsTile<kNarrow>& T, int r) {
    const uint64_t base = T.in + uint64_t(int64_t(r) * T.in_stride);
#ifdef ABL_MEM
    v4u v0, v1;
    v0.x = uint32_t(base) + uint32_t(T.in0) + threadIdx.x, v0.y = v0.x * 3, v0.z = v0.x * 5, v0.w = v0.x * 7;
    v1 = v0 * 11u;
#else
#if LAMD_BS_NT & 1
    const v4u v0 = __builtin_nontemporal_load(bs_addr(base, T.in0));
    const v4u v1 = __builtin_nontemporal_load(bs_addr(base, T.in1));
#else
    const v4u v0 = *bs_addr(base, T.in0);
    const v4u v1 = *bs_addr(base, T.in1);
#endif
#endif
    v[0] = v0.x, v[1] = v0.y, v[2] = v0.z, v[3] = v0.w;
    v[4] = v1.x, v[5] = v1.y, v[6] = v1.z, v[7] = v1.w;
}
// Registers R0 .. R1 - 1 of a tile.
template <int R0, int R1 = R0 + 8, bool kNarrow>
LDEV void load_half(Reg& x, const BsTile<kNarrow>& T) {
#pragma unroll
    for (int r = R0; r < R1; ++r) load_reg(x[r], T, r);
}
template <int R0, bool kNarrow>
LDEV void store_half(const Reg& x, const BsTile<kNarrow>& T) {
#pragma unroll
    for (int r = R0; r < R0 + 8; ++r) {
        const uint64_t base = T.out + uint64_t(int64_t(r) * T.out_stride);
        v4u v0, v1;
        v0.x = x[r][0], v0.y = x[r][1], v0.z = x[r][2], v0.w = x[r][3];
        v1.x = x[r][4], v1.y = x[r][5], v1.z = x[r][6], v1.w = x[r][7];
#ifdef ABL_MEM
        const uint32_t acc = v0.x ^ v0.y ^ v0.z ^ v0.w ^ v1.x ^ v1.y ^ v1.z ^ v1.w;
        if (acc == 0x12345679u && T.in_stride == 7) *gptr<uint32_t>(reinterpret_cast<uint8_t*>(base)) = acc;  // keep the values live
        continue;
#endif
        // A segment past the piece's end was loaded from segment 0 of the
        // strip (always inside: pieces are multiples of 64 bytes), and the
        // transform is column by column, so it holds segment 0's output: it is
        // stored there, the same bytes lane 8 g writes (no branch per store).
        const auto p0 = bs_addr(base, T.out0);
        const auto p1 = bs_addr(base, T.out1);
#if LAMD_BS_NT & 2
        __builtin_nontemporal_store(v0, p0);
        __builtin_nontemporal_store(v1, p1);
#else
        *p0 = v0;
        *p1 = v1;
#endif
    }
}
// The verify form's epilogue (leo_amd_verify), verify_issue then verify_check
// in place of store_half: the
// stored recovery segments are loaded from the addresses the stores would have
// used (a segment past the piece's end: segment 0, which this lane then holds
// the output of, as in store_half -- no branch), XORed with the computed
// values, and a lane group that sees a difference in piece pg | r ORs that
// piece's bit into the object's report `rep`.  The 8 << WB lanes of a lane
// group hold the same 16 pieces, other lane groups of the wave hold others: the
// wave's ballot is cut into lane groups and the first flagged lane of a group
// reports for it.  Nothing is written on a clean stripe.
//
// The stored segments of one half (8 registers x 2 segments of 16 bytes), all in
// flight together: one exposed load latency per half.  They are issued behind
// the half's transposes: issued ahead of them (to run under them) the
// cooperative tile spilled 28 VGPRs at LAMD_BS_OCC = 2; here it holds 247
// against the encode tile's 240.
struct BsStored {
    v4u s0[8], s1[8];
};
template <int R0, bool kNarrow>
LDEV void verify_issue(BsStored& st, const BsTile<kNarrow>& T) {
    bs_fence();  // the loads stay here: not hoisted into the butterflies, not sunk to their use
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t base = T.out + uint64_t(int64_t(R0 + i) * T.out_stride);
#if LAMD_BS_NT & 1
        st.s0[i] = __builtin_nontemporal_load(bs_addr(base, T.out0));
        st.s1[i] = __builtin_nontemporal_load(bs_addr(base, T.out1));
#else
        st.s0[i] = *bs_addr(base, T.out0);
        st.s1[i] = *bs_addr(base, T.out1);
#endif
    }
    bs_fence();
}
template <int R0, int WB>
LDEV void verify_check(const Reg& x, const BsStored& st, uint32_t* rep, unsigned g) {
    constexpr unsigned kGroup = 8u << WB;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned first = lane & ~(kGroup - 1u);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = R0 + i;
        const v4u &a = st.s0[i], &b = st.s1[i];
        const uint32_t d = (x[r][0] ^ a.x) | (x[r][1] ^ a.y) | (x[r][2] ^ a.z) | (x[r][3] ^ a.w) |
                           (x[r][4] ^ b.x) | (x[r][5] ^ b.y) | (x[r][6] ^ b.z) | (x[r][7] ^ b.w);
        const uint64_t bad = __builtin_amdgcn_ballot_w64(d != 0);
        const uint64_t mine = (bad >> first) & ((uint64_t(1) << kGroup) - 1u);
        if (mine != 0 && lane == first + unsigned(__builtin_ctzll(mine))) {
            // (computed here, on the rare path: as loop invariants the 16 pieces' bits took 16 VGPRs)
            unsigned gg = g;
            asm volatile("" : "+v"(gg));
            const unsigned p = piece_of(kLay0, unsigned(r), gg);
            atomicOr(rep + (p >> 5), 1u << (p & 31u));
        }
    }
    bs_fence();
}
template <int R0>
LDEV void transpose_half(Reg& x, const XMasks& xm) {
#pragma unroll
    for (int r = R0; r < R0 + 8; ++r) {
        transpose8(x[r], xm);
        pin8(x[r]);
        bs_fence_every<LAMD_BS_XFENCE>(r);
    }
}

#ifdef LAMD_CLOCK
// Diagnostic builds only (tools/bs_clock.py): per wave, (s_memtime,
// s_memrealtime) at entry and exit, for the shader clock under this kernel's
// load and the waves' lifetimes.
__device__ uint64_t* g_bs_clock;
#endif

// -------------------------------------------------------------- kernel -----

// One transform direction's low layers (0-2) on half H, and their inverse order
// (kLayLow<WB>, bs_layout.h: the layout they end in).
template <bool kInverse, int kOff, int H, int WB = 0, unsigned WV = 0>
LDEV void low_layers(Reg& x, const uint32_t (&G)[3]) {
    constexpr bool kSwap1 = LAMD_BS_SWAPS && WB < 2;
    if constexpr (kInverse) {
        layer<true, kOff, 0, kLay0, H, WB, WV>(x, G);
        if constexpr (LAMD_BS_SWAPS) swap_lanes<0, 2, H>(x);
        layer<true, kOff, 1, kLay1, H, WB, WV>(x, G);
        if constexpr (kSwap1) swap_lanes<1, 1, H>(x);
        layer<true, kOff, 2, kLayLow<WB>, H, WB, WV>(x, G);
    } else {
        layer<false, kOff, 2, kLayLow<WB>, H, WB, WV>(x, G);
        if constexpr (kSwap1) swap_lanes<1, 1, H>(x);
        layer<false, kOff, 1, kLay1, H, WB, WV>(x, G);
        if constexpr (LAMD_BS_SWAPS) swap_lanes<0, 2, H>(x);
        layer<false, kOff, 0, kLay0, H, WB, WV>(x, G);
    }
}
// The low layers of wave wv of a workgroup-cooperative tile: one scalar branch
// to the wave's variant (only the butterflies' constants differ; no barrier
// inside, so the waves may take different paths).
template <bool kInverse, int kOff, int H, int WB>
LDEV void low_layers_of(Reg& x, const uint32_t (&G)[3], unsigned wv) {
    if constexpr (WB == 0) {
        low_layers<kInverse, kOff, H>(x, G);
    } else if constexpr (WB == 1) {
        if (wv == 0)
            low_layers<kInverse, kOff, H, 1, 0>(x, G);
        else
            low_layers<kInverse, kOff, H, 1, 1>(x, G);
    } else {
        switch (wv) {
            case 0: low_layers<kInverse, kOff, H, 2, 0>(x, G); break;
            case 1: low_layers<kInverse, kOff, H, 2, 1>(x, G); break;
            case 2: low_layers<kInverse, kOff, H, 2, 2>(x, G); break;
            default: low_layers<kInverse, kOff, H, 2, 3>(x, G); break;
        }
    }
}

// Persistent waves: the grid fills the GPU once (kBsBlocksPerCu workgroups of
// kBsWaves independent waves a CU) and wave i codes tiles i, i + n, ... (tile =
// object * strips + strip).  A tile is software-pipelined in halves (register
// bit 3 = piece bit 3 in every low layout, never paired by layers 0-2 or the
// lane swaps): the last FFT layers, transposes and stores of half 0 run, then
// the next tile's half-0 loads are issued into the freed registers while half 1
// computes; at the top of the next tile half 1's loads are in flight while half
// 0 transposes and runs its IFFT layers.  (Deeper prefetch -- part of the next
// tile a whole tile ahead, by LDS-DMA into the unused LDS or into spare VGPRs --
// addresses latency, which is not what binds: the kernel runs at the board's
// power limit, memory and arithmetic each at full clock alone)
//
// WB > 0, the workgroup-cooperative tile: the 1 << WB waves of a workgroup share
// ONE tile of 128 pieces x (256 << WB) bytes.  The low WB bits of g are the
// wave's index, so the low layers are twisted by 3 - WB lane bits only (a code
// variant per wave, low_layers_of); the exchanges to and from kLayT cross the
// waves (exchange_wg, barriers).  The tile index, the queue and the loop's exit
// are then per workgroup: wave 0 asks the queue and publishes the answer
// through LDS, every wave reads the same word, so all of them take the same
// next tile or leave together -- no wave may return or loop alone, the others
// would wait at a barrier for ever.
//
// kFormV = kFormDenseEnc | kFormVerify: the verify form (verify_issue / verify_check in place of
// store_half; object obj's report at b.report + 4 obj).
template <int kFormV, bool kNarrow, int WB = 0>
__global__ void __launch_bounds__(WB ? (64 << WB) : 64 * kBsWaves) __attribute__((amdgpu_waves_per_eu(LAMD_BS_OCC, LAMD_BS_OCC)))
k_ff8_bs_slab(Ff8SlabBatch b, uint32_t count, uint32_t strips, uint32_t* q, uint32_t* qclear) {
    constexpr int kForm = kFormV & ~kFormVerify;
    constexpr bool kVerify = (kFormV & kFormVerify) != 0;
    static_assert(!kVerify || kForm == kFormDenseEnc, "the verify form of the dense encode tile");
    constexpr int kOffI = kForm == kFormDenseDec ? -1 : 127;  // IFFT skew base
    constexpr int kOffF = kForm == kFormDenseDec ? 127 : -1;  // FFT skew base
    constexpr unsigned kTiles = WB ? 1u : unsigned(kBsWaves);  // tiles in flight per workgroup
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const unsigned wave = threadIdx.x >> 6;
    const unsigned n = gridDim.x * kTiles, total = count * strips;
    uint8_t* const area = reinterpret_cast<uint8_t*>(lds + (WB ? 0u : wave * kBsAreaDw));
    // wave-uniform, so that a tile's pointers are scalar loads (off the vector
    // memory counter the piece loads are waited on with)
    unsigned t = __builtin_amdgcn_readfirstlane(WB ? blockIdx.x : blockIdx.x * kBsWaves + wave);
    if (t >= total) return;  // WB = 0: waves share nothing; WB > 0: the same for the whole workgroup
#ifdef LAMD_CLOCK
    const uint64_t c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned t0 = t;
#endif
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wv = WB ? __builtin_amdgcn_readfirstlane(wave) : 0u;  // the wave bits of g
    const unsigned g = ((lane >> (3 + WB)) << WB) | wv, l = lane & ((8u << WB) - 1u);
    // Tile queues (q != null): after the first round (tile = wave index) a wave
    // takes its next tile from the queue of its XCD (workgroups are dealt to
    // the 8 XCDs round robin): tiles n + xq + 8 k, k = that queue's counter.
    // Waves that run faster take more tiles, so all of a launch's waves end
    // within about one tile of each other (a static share left the two waves
    // of a SIMD ending up to ~35% apart, the second one alone at half the issue
    // rate).  One counter set per launch; this launch zeroes the other set, the
    // previous launch's, for the next one (Workspace::bs_queue).
    if (qclear != nullptr && blockIdx.x == 0 && wave == 0 && lane < 8u) qclear[32u * lane] = 0u;
    const unsigned xq = blockIdx.x & 7u;
    uint32_t* const head = q != nullptr ? q + 32u * xq : nullptr;
    // WB > 0: the queue's answer, behind the exchange area
    volatile uint32_t* const slot = lds + kBsWgAreaBytes<WB> / 4;
    const uint32_t G[3] = {(g & 1u) ? ~0u : 0u, (g & 2u) ? ~0u : 0u, (g & 4u) ? ~0u : 0u};
    const XMasks xm;
    Reg x;
    BsTile<kNarrow> cur = bs_tile<kNarrow, WB>(b, t, strips, g, l);
    load_half<0, 8>(x, cur);
    load_half<8, 16>(x, cur);
    for (;;) {
        // the next tile's index, requested a tile ahead (its latency hidden)
        uint32_t kq = 0;
        if (head != nullptr && lane == 0 && (WB == 0 || wv == 0))
            kq = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifndef ABL_ARITH
        transpose_half<0>(x, xm);
        low_layers_of<true, kOffI, 0, WB>(x, G, wv);
        transpose_half<8>(x, xm);
        low_layers_of<true, kOffI, 1, WB>(x, G, wv);
        if constexpr (WB)
            exchange_wg<kLayLow<WB>, kLayT, WB>(x, area, g, l);
        else
            exchange<kLay2, kLayT>(x, area, g, l);
        layer<true, kOffI, 3, kLayT>(x, G);
        layer<true, kOffI, 4, kLayT>(x, G);
        layer<true, kOffI, 5, kLayT>(x, G);
        fused_top<kOffI, kOffF>(x, G);
        layer<false, kOffF, 5, kLayT>(x, G);
        layer<false, kOffF, 4, kLayT>(x, G);
        layer<false, kOffF, 3, kLayT>(x, G);
        if constexpr (WB) {
            // published by the exchange's first barrier; the slot is written
            // again a whole exchange (8 barriers) after every wave has read it
            if (head != nullptr && lane == 0 && wv == 0) *slot = kq;
            exchange_wg<kLayT, kLayLow<WB>, WB>(x, area, g, l);
            if (head != nullptr) kq = *slot;
        } else {
            exchange<kLayT, kLay2>(x, area, g, l);
        }
#else
#pragma unroll
        for (int r = 0; r < 16; ++r) pin8(x[r]);
        if constexpr (WB) {
            if (head != nullptr && lane == 0 && wv == 0) *slot = kq;
            __syncthreads();
            if (head != nullptr) kq = *slot;
            __syncthreads();
        }
#endif
        const unsigned tn = head != nullptr ? n + xq + 8u * __builtin_amdgcn_readfirstlane(kq) : t + n;
        const bool more = tn < total;
        const BsTile<kNarrow> nxt = bs_tile<kNarrow, WB>(b, more ? tn : t, strips, g, l);
        [[maybe_unused]] BsStored stored;  // verify form
        uint32_t* rep = nullptr;           // verify form: the report of the current tile's object (128 pieces: 4 words)
        if constexpr (kVerify) rep = b.report + size_t(t / strips) * 4u;
#ifndef ABL_ARITH
        low_layers_of<false, kOffF, 0, WB>(x, G, wv);
        transpose_half<0>(x, xm);
#endif
        if constexpr (kVerify) verify_issue<0>(stored, cur);
        if constexpr (kVerify) verify_check<0, WB>(x, stored, rep, g);
        else store_half<0>(x, cur);
        if (more) load_half<0, 8>(x, nxt);
#ifndef ABL_ARITH
        low_layers_of<false, kOffF, 1, WB>(x, G, wv);
        transpose_half<8>(x, xm);
#endif
        if constexpr (kVerify) verify_issue<8>(stored, cur);
        if constexpr (kVerify) verify_check<8, WB>(x, stored, rep, g);
        else store_half<8>(x, cur);
        if (!more) break;
        load_half<8, 16>(x, nxt);
        t = tn;
        cur = nxt;
    }
#ifdef LAMD_CLOCK
    const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63u) == 0 && g_bs_clock != nullptr) {  // null unless tools/bs_clock.py set it
        uint64_t* o = g_bs_clock + 4ull * t0;
        o[0] = c0, o[1] = r0, o[2] = c1, o[3] = r1;
    }
#endif
}

}  // namespace

bool ff8_bs_supported(unsigned T, unsigned K, unsigned R, unsigned nchunks) {
    return T == 7 && K == 128 && R == 128 && nchunks == 1;
}

// Wave bits of the launch's tile.  The workgroup-cooperative tile does the same
// work per wave and per workgroup as four (two) independent waves' tiles, on
// the same grid, so it needs no minimum tile count; what it can lose is lanes
// past the piece's end, since its strips are 256 << WB bytes.  It runs when the
// pieces, padded to whole strips, are at most 1/4 longer than padded to
// 256-byte strips (pieces shorter than a strip never are): at 18% more it still
// measured 20% faster than the one-wave tile (64 objects of 4160-byte pieces,
// DESIGN.md section 7.8).  Experiment builds:
// LEO_AMD_FF8_BS_WAVES = 1 | 2 | 4 forces the waves per tile at every size.
#ifndef LAMD_BS_WB
#define LAMD_BS_WB 2  // the product's workgroup-cooperative tile (0: none)
#endif
namespace {
int bs_wave_bits(uint32_t bytes) {
#if LAMD_EXPERIMENT_ENV
    static const int forced = [] {
        const char* e = std::getenv("LEO_AMD_FF8_BS_WAVES");
        return !e ? -1 : e[0] == '1' ? 0 : e[0] == '2' ? 1 : e[0] == '4' ? 2 : -1;
    }();
    if (forced >= 0) return forced;
#endif
    constexpr int WB = LAMD_BS_WB;
    if (WB == 0) return 0;
    const uint64_t strip = kBsStrip << WB;
    const uint64_t pad = (bytes + strip - 1) / strip * strip, pad0 = (uint64_t(bytes) + kBsStrip - 1) / kBsStrip * kBsStrip;
    return pad * 4u <= pad0 * 5u ? WB : 0;
}
template <int kForm, int WB>
const void* bs_kernel_wg() {
    // product builds hold the one cooperative tile they use
    if constexpr (LAMD_EXPERIMENT_ENV || WB == LAMD_BS_WB)
        return reinterpret_cast<const void*>(&k_ff8_bs_slab<kForm, true, WB>);
    else
        return nullptr;
}
}  // namespace

hipError_t launch_ff8_bs_slab(const Ff8SlabBatch& b, unsigned count, int form, hipStream_t s, unsigned cus,
                              uint32_t* q, uint32_t* qclear) {
    if (count == 0 || count > kSlabObjs || (b.nunits * 4u) % 64u != 0 || b.K != 128 || b.R != 128)
        return hipErrorInvalidValue;
    constexpr int kVer = kFormDenseEnc | kFormVerify;
    if (form != kFormDenseEnc && form != kFormDenseDec && form != kVer) return hipErrorInvalidValue;
    if (form == kVer && b.report == nullptr) return hipErrorInvalidValue;
    cus = std::max(cus, 1u);
    // 32-bit lane offsets when every slab's lane offsets (up to 127 strides + a
    // strip) fit them; the cooperative tile is built for those only
    bool narrow = true, narrow_wg = true;
    for (unsigned o = 0; o < count; ++o)
        for (const int32_t st : {b.in_stride[o], b.out_stride[o]}) {
            narrow = narrow && st >= 0 && uint64_t(st) * 128u + kBsStrip <= (uint64_t(1) << 32);
            narrow_wg = narrow_wg && st >= 0 && uint64_t(st) * 128u + (kBsStrip << 2) <= (uint64_t(1) << 32);
        }
    const int wb = narrow_wg ? bs_wave_bits(b.nunits * 4u) : 0;
    const uint32_t strip = kBsStrip << wb;
    uint32_t strips = (b.nunits * 4u + strip - 1) / strip;
    uint32_t cnt = count;
    const unsigned total = cnt * strips;
    // workgroups: wb = 0, kBsWaves tiles each; wb > 0, one tile of 1 << wb waves
    const unsigned tiles_wg = wb ? 1u : unsigned(kBsWaves), waves_wg = wb ? 1u << wb : unsigned(kBsWaves);
    const unsigned per_cu = wb ? 4u * LAMD_BS_OCC >> wb : kBsBlocksPerCu;
    const unsigned blocks = std::min<unsigned>((total + tiles_wg - 1) / tiles_wg, cus * per_cu);
    const size_t lds = wb ? size_t(8192u << wb) + 16 : size_t(kBsWaves) * kBsAreaDw * 4;
#if LAMD_BS_QUEUE == 0
    q = qclear = nullptr;
#endif
    // the 8 queues each serve the workgroups of one XCD (blockIdx.x & 7): every
    // queue needs workgroups, or static assignment (tiles i, i + n, ...); the
    // next launch's set is still cleared (Workspace::bs_queue alternates them)
    if (blocks < 8) q = nullptr;
    void* params[] = {const_cast<Ff8SlabBatch*>(&b), &cnt, &strips, &q, &qclear};
    const bool dec = form == kFormDenseDec;
    const void* fn = nullptr;
    if (form == kVer)
        fn = wb == 2   ? bs_kernel_wg<kVer, 2>()
             : wb == 1 ? bs_kernel_wg<kVer, 1>()
             : narrow  ? reinterpret_cast<const void*>(&k_ff8_bs_slab<kVer, true>)
                       : reinterpret_cast<const void*>(&k_ff8_bs_slab<kVer, false>);
    else if (wb == 2)
        fn = dec ? bs_kernel_wg<kFormDenseDec, 2>() : bs_kernel_wg<kFormDenseEnc, 2>();
    else if (wb == 1)
        fn = dec ? bs_kernel_wg<kFormDenseDec, 1>() : bs_kernel_wg<kFormDenseEnc, 1>();
    else
        fn = dec ? (narrow ? reinterpret_cast<const void*>(&k_ff8_bs_slab<kFormDenseDec, true>)
                           : reinterpret_cast<const void*>(&k_ff8_bs_slab<kFormDenseDec, false>))
                 : (narrow ? reinterpret_cast<const void*>(&k_ff8_bs_slab<kFormDenseEnc, true>)
                           : reinterpret_cast<const void*>(&k_ff8_bs_slab<kFormDenseEnc, false>));
    if (fn == nullptr) return hipErrorInvalidValue;  // a tile this build does not hold
    return hipLaunchKernel(fn, dim3(blocks), dim3(64 * waves_wg), params, lds, s);
}

}  // namespace lamd

#ifdef LAMD_CLOCK
extern "C" __attribute__((visibility("default"))) int leo_amd_debug_bs_clock(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(lamd::g_bs_clock), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif
