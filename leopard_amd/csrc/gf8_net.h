// gf8_net.h -- XOR networks with shared subexpressions for the multiplies by
// compile-time constants of the bit-sliced tile (rs_ff8_bs.hip), from the 8 x 8
// GF(2) matrices of gf8_const.h.
//
// A network takes the 8 planes y[0..7] and computes, for up to four matrices on
// the same y,
//   x[i] ^= row_i(M0) . y  ^  sum over m = 1..3 of  ((row_i(Mm) . y) & g_m)
// (M0: the butterfly's constant; M1..M3: the twists a lane mask g_m selects).
// It is a straight-line program of 2- and 3-input XOR gates, one v_bitop3 (or
// v_xor) each: first the temporaries, each the XOR of two or three earlier
// variables (variable v < 8 is y[v], variable 8 + k is temporary k), then one
// chain per output row over the variables left in it: an M0 row of w variables
// takes ceil(w / 2) gates with its accumulator x[i], a masked row 1 + floor(w / 2)
// (the last one is x[i] ^ (value & g)).
//
// Synthesis (net_synth): cancellation-free greedy extraction.  Every step takes
// the pair or triple of variables whose extraction as a temporary lowers the
// gate count the most (a triple present in n rows saves n - 1; a pair saves one
// per row whose chain it shortens, less one).  Ties decide how far it gets, so
// the search is repeated with different tie-break rules (8 fixed preferences,
// then hashed orders) and the cheapest program kept.
//
// The search is a constexpr function, but a compiler evaluates it some hundred
// times slower than it runs (minutes for the tile's ~900 networks), so the
// networks of the tiles are committed as a table, gf8_net_table.h, written by
// tools/gen_gf8_net_table.cpp from these same functions with kNetTableRuns
// restarts each.  net_lookup takes a network from the table; matrices the table
// does not hold (experiment layouts) are synthesized during compilation with
// kNetRuns restarts.  Either way every network the kernel runs is evaluated
// symbolically over GF(2) against its matrices by static_assert (net_ok,
// Gf8NetOf), and tests/test_cpu_bs_networks.py runs them on the host against
// the field tables.  Gate counts per tile: DESIGN.md section 7.9.
#pragma once

#include <cstdint>

#include "gf8_const.h"

namespace lamd {

constexpr int kNetMaxTemps = 16;  // temporaries live at once in a butterfly, at most
constexpr int kNetMats = 4;
constexpr unsigned kNetRuns = 8;          // restarts of a synthesis during compilation
constexpr unsigned kNetTableRuns = 1032;  // restarts per network of the committed table

struct Gf8Net {
    int ntemp = 0;
    int gates = 0;                     // instructions: temporaries + row chains
    uint32_t temp[kNetMaxTemps] = {};  // temporary k = XOR of the variables of this mask (2 or 3, all below 8 + k)
    uint32_t row[kNetMats][8] = {};    // row i of matrix m = XOR of the variables of this mask
};

constexpr int net_popc(uint32_t v) { return __builtin_popcount(v); }
constexpr int net_ctz(uint32_t v) { return __builtin_ctz(v); }
constexpr int net_row_gates(uint32_t row, bool masked) {
    const int w = net_popc(row);
    return w == 0 ? 0 : masked ? 1 + w / 2 : (w + 1) / 2;
}

// One greedy pass.  run < 8: bit 0 prefers the candidate in more rows, bit 1
// triples over pairs (else pairs), bit 2 admits pairs that save nothing yet;
// run >= 8: ties by a hash seeded with (run - 8) / 2, its bit 0 as bit 2 above.
constexpr Gf8Net net_greedy(const uint64_t (&M)[kNetMats], unsigned run) {
    Gf8Net n;
    uint32_t rows[8 * kNetMats] = {};
    int nrows = 0;
    for (int m = 0; m < kNetMats; ++m) {
        if (M[m] == 0) continue;
        nrows = 8 * (m + 1);
        for (int i = 0; i < 8; ++i) rows[8 * m + i] = uint32_t(M[m] >> (8 * i)) & 0xFFu;
    }
    const bool hashed = run >= 8;
    const unsigned seed = (run - 8) >> 1;
    const bool zero_ok = hashed ? ((run - 8) & 1u) != 0 : (run & 4u) != 0;
    int nv = 8;
    while (n.ntemp < kNetMaxTemps) {
        uint32_t with[8 + kNetMaxTemps] = {};  // the rows that hold variable v
        uint32_t fav = 0;                      // the rows one variable less makes cheaper
        for (int r = 0; r < nrows; ++r) {
            uint32_t m = rows[r];
            int w = 0;
            for (; m != 0; m &= m - 1, ++w) with[net_ctz(m)] |= 1u << r;
            if (w != 0 && (w & 1) == (r < 8 ? 1 : 0)) fav |= 1u << r;
        }
        // the candidate of the largest gain; among equals the largest tie-break
        // value, then the first (a candidate below the best gain so far is
        // dropped before its tie-break value is worked out: constant evaluation
        // of this loop is most of the file's compile time)
        int best_gain = zero_ok ? 0 : 1;
        uint32_t best_tie = 0, best = 0;
        const uint32_t salt = seed * 40503u + uint32_t(n.ntemp) * 977u;
        const uint32_t by_count = run & 1u, triples_first = (run >> 1) & 1u;
        for (int a = 0; a < nv; ++a) {
            if (with[a] == 0) continue;
            for (int b = a + 1; b < nv; ++b) {
                const uint32_t r2 = with[a] & with[b];
                const int n2 = net_popc(r2);
                if (n2 < 2 || n2 - 1 < best_gain) continue;  // no pair or triple of these rows gains more than n2 - 1
                const uint32_t m2 = (1u << a) | (1u << b);
                for (int c = b; c < nv; ++c) {  // c = b: the pair itself
                    const bool triple = c != b;
                    const int count = triple ? net_popc(r2 & with[c]) : n2;
                    const int gain = (triple ? count : net_popc(r2 & fav)) - 1;
                    if (count < 2 || gain < best_gain || (triple && gain < 1)) continue;
                    const uint32_t m = m2 | (1u << c);
                    uint32_t tie = 0;
                    if (hashed) {
                        tie = m * 2654435761u + salt;
                        tie ^= tie >> 15;
                        tie *= 2246822519u;
                        tie ^= tie >> 13;
                        tie &= 0xFFFFu;
                    } else {
                        tie = (by_count ? uint32_t(count) << 1 : 0u) | (triples_first == uint32_t(triple) ? 1u : 0u);
                    }
                    if (best == 0 || gain > best_gain || tie > best_tie) best_gain = gain, best_tie = tie, best = m;
                }
            }
        }
        if (best == 0) break;
        n.temp[n.ntemp++] = best;
        for (int r = 0; r < nrows; ++r)
            if ((rows[r] & best) == best) rows[r] = (rows[r] & ~best) | (1u << nv);
        ++nv;
    }
    n.gates = n.ntemp;
    for (int r = 0; r < 8 * kNetMats; ++r) {
        n.row[r >> 3][r & 7] = rows[r];
        n.gates += net_row_gates(rows[r], r >= 8);
    }
    return n;
}

// The cheapest program of `runs` passes for x ^= A y ^ ((H0 y) & g0) ^ ((H1 y) & g1) ^ ((H2 y) & g2).
constexpr Gf8Net net_synth(uint64_t A, uint64_t H0 = 0, uint64_t H1 = 0, uint64_t H2 = 0, unsigned runs = kNetRuns) {
    const uint64_t M[kNetMats] = {A, H0, H1, H2};
    Gf8Net best = net_greedy(M, 0);
    for (unsigned run = 1; run < runs; ++run) {
        const Gf8Net n = net_greedy(M, run);
        if (n.gates < best.gates) best = n;
    }
    return best;
}

// The program evaluated symbolically over GF(2): every variable as the set of
// planes of y it is the XOR of; the rows must come to the matrices' rows.
constexpr bool net_ok(const Gf8Net& n, uint64_t A, uint64_t H0 = 0, uint64_t H1 = 0, uint64_t H2 = 0) {
    const uint64_t M[kNetMats] = {A, H0, H1, H2};
    uint32_t val[8 + kNetMaxTemps] = {};
    for (int v = 0; v < 8; ++v) val[v] = 1u << v;
    if (n.ntemp < 0 || n.ntemp > kNetMaxTemps) return false;
    int gates = n.ntemp;
    for (int k = 0; k < n.ntemp; ++k) {
        const uint32_t m = n.temp[k];
        if (m >> (8 + k) != 0 || net_popc(m) < 2 || net_popc(m) > 3) return false;
        for (int v = 0; v < 8 + k; ++v)
            if ((m >> v) & 1u) val[8 + k] ^= val[v];
    }
    for (int m = 0; m < kNetMats; ++m)
        for (int i = 0; i < 8; ++i) {
            if (n.row[m][i] >> (8 + n.ntemp) != 0) return false;
            uint32_t s = 0;
            for (int v = 0; v < 8 + n.ntemp; ++v)
                if ((n.row[m][i] >> v) & 1u) s ^= val[v];
            if (s != (uint32_t(M[m] >> (8 * i)) & 0xFFu)) return false;
            gates += net_row_gates(n.row[m][i], m > 0);
        }
    return gates == n.gates;
}

// The committed networks, sorted by their matrices.
struct Gf8NetEntry {
    uint64_t M[kNetMats];
    Gf8Net net;
};
#ifndef LAMD_GF8_NET_NO_TABLE
#include "gf8_net_table.h"
#else
inline constexpr Gf8NetEntry kGf8NetTable[] = {{{0, 0, 0, 0}, {}}};
#endif
constexpr int kGf8NetTableSize = int(sizeof(kGf8NetTable) / sizeof(kGf8NetTable[0]));

constexpr int net_table_index(uint64_t A, uint64_t H0 = 0, uint64_t H1 = 0, uint64_t H2 = 0) {
    const uint64_t M[kNetMats] = {A, H0, H1, H2};
    int lo = 0, hi = kGf8NetTableSize;  // the first entry not below M
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        bool below = false;
        for (int m = 0; m < kNetMats; ++m)
            if (kGf8NetTable[mid].M[m] != M[m]) {
                below = kGf8NetTable[mid].M[m] < M[m];
                break;
            }
        if (below)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo == kGf8NetTableSize) return -1;
    for (int m = 0; m < kNetMats; ++m)
        if (kGf8NetTable[lo].M[m] != M[m]) return -1;
    return lo;
}
// The network of a set of matrices: the table's, or synthesized here.
constexpr Gf8Net net_lookup(uint64_t A, uint64_t H0 = 0, uint64_t H1 = 0, uint64_t H2 = 0) {
    const int i = net_table_index(A, H0, H1, H2);
    return i >= 0 ? kGf8NetTable[i].net : net_synth(A, H0, H1, H2);
}

// The network of a set of matrices as a compile-time constant, checked.
template <uint64_t A, uint64_t H0 = 0, uint64_t H1 = 0, uint64_t H2 = 0>
struct Gf8NetOf {
    static constexpr Gf8Net net = net_lookup(A, H0, H1, H2);
    static_assert(net_ok(net, A, H0, H1, H2), "the synthesized network is the matrices' product");
};

constexpr uint64_t kGf8Identity = 0x8040201008040201ull;  // gf8_matrix(1)

}  // namespace lamd
