// Test helper (tests/test_cpu_bs_networks.py): runs the synthesized XOR networks
// of the bit-sliced tile (leopard_amd/csrc/gf8_net.h, bs_layout.h) on the host,
// on bit planes that hold every byte value once, and prints what they compute.
//
// Planes: 256 elements, element e = the byte value e, as 8 planes of 256 bits
// (plane k, bit e = bit k of e); the accumulator x holds element e = kX(e).
// A network is executed gate by gate as the kernel does (temporaries, then one
// chain per row, the masked rows through x ^ (value & g)).
//
// Output, one record a line:
//   gates8 N            8 x the per-tile gate total of the constant networks
//   table N MISSING     networks in gf8_net_table.h (each checked by net_ok), and how
//                       many of the networks below were not found in it
//   c C GATES HEX       the network of gf8_matrix(C): 256 result bytes x ^ C * e
//   b OFF L R WB WV A H0 H1 H2 ALT GATES GM HEX
//                       the network a butterfly of the tiles runs (skew base OFF,
//                       layer L, register R, WB wave bits, wave WV): constants
//                       A (as run: c ^ 1 where ALT) and twists H0..H2, with the
//                       lane masks g_j all-ones for the bits j of GM, else zero
#include <cstdint>
#include <cstdio>

#include "bs_layout.h"

using namespace lamd;

namespace {

struct Plane {
    uint32_t w[8];
};
constexpr unsigned kX(unsigned e) { return (e * 37u + 11u) & 255u; }

Plane var_of(const Gf8Net& n, int v, const Plane* y, const Plane* t) { return v < 8 ? y[v] : t[v - 8]; }
Plane xor_of(const Gf8Net& n, uint32_t mask, const Plane* y, const Plane* t) {
    Plane s = {};
    for (int v = 0; v < 8 + kNetMaxTemps; ++v)
        if ((mask >> v) & 1u) {
            const Plane p = var_of(n, v, y, t);
            for (int i = 0; i < 8; ++i) s.w[i] ^= p.w[i];
        }
    return s;
}
// the 256 result bytes of x ^= A y ^ sum ((H_m y) & g_m), g_m all-ones for the bits of gm
void run(const Gf8Net& n, unsigned gm, uint8_t* out) {
    Plane x[8] = {}, y[8] = {}, t[kNetMaxTemps] = {};
    for (unsigned e = 0; e < 256; ++e)
        for (int k = 0; k < 8; ++k) {
            y[k].w[e >> 5] |= ((e >> k) & 1u) << (e & 31u);
            x[k].w[e >> 5] |= ((kX(e) >> k) & 1u) << (e & 31u);
        }
    for (int k = 0; k < n.ntemp; ++k) t[k] = xor_of(n, n.temp[k], y, t);
    for (int i = 0; i < 8; ++i)
        for (int m = 0; m < kNetMats; ++m) {
            const Plane p = xor_of(n, n.row[m][i], y, t);
            const uint32_t g = m == 0 || ((gm >> (m - 1)) & 1u) ? ~0u : 0u;
            for (int j = 0; j < 8; ++j) x[i].w[j] ^= p.w[j] & g;
        }
    for (unsigned e = 0; e < 256; ++e) {
        unsigned v = 0;
        for (int k = 0; k < 8; ++k) v |= ((x[k].w[e >> 5] >> (e & 31u)) & 1u) << k;
        out[e] = uint8_t(v);
    }
}
void print_hex(const uint8_t* out) {
    for (unsigned e = 0; e < 256; ++e) std::printf("%02x", out[e]);
    std::printf("\n");
}
// the element c of a multiply matrix: column 0 is 1 * c
unsigned element_of(uint64_t m) {
    unsigned c = 0;
    for (int i = 0; i < 8; ++i) c |= unsigned((m >> (8 * i)) & 1u) << i;
    return c;
}

}  // namespace

int main() {
    uint8_t out[256];
    unsigned missing = 0;  // networks the tiles run that gf8_net_table.h does not hold
    std::printf("gates8 %u\n", bs_tile_network_gates8());
    for (unsigned c = 0; c < 256; ++c) {
        const Gf8Net n = net_lookup(gf8_matrix(c));
        if (net_table_index(gf8_matrix(c)) < 0) ++missing;
        if (!net_ok(n, gf8_matrix(c))) return 1;
        run(n, 0, out);
        std::printf("c %u %d ", c, n.gates);
        print_hex(out);
    }
    // every butterfly of the low layers of every tile (WB = 0, 1, 2; every wave's
    // code variant); the layers above run constants only (the records c)
    for (int WB = 0; WB <= 2; ++WB)
        for (unsigned wv = 0; wv < (1u << WB); ++wv)
            for (int off : {-1, 127})
                for (unsigned l = 0; l < 3; ++l) {
                    const uint32_t L = bs_low_layout(l, WB);
                    const unsigned half = 1u << reg_bit_of(L, l);
                    for (unsigned r = 0; r < 16; ++r) {
                        if (r & half) continue;
                        BsMats m = bs_mats(off, L, r, l, WB, wv);
                        const bool alt = bs_alt_form(m);
                        if (alt) m.A ^= kGf8Identity;
                        const Gf8Net n = net_lookup(m.A, m.H[0], m.H[1], m.H[2]);
                        if (net_table_index(m.A, m.H[0], m.H[1], m.H[2]) < 0) ++missing;
                        if (!net_ok(n, m.A, m.H[0], m.H[1], m.H[2])) return 1;
                        unsigned present = 0;
                        for (int j = 0; j < 3; ++j) present |= (m.H[j] != 0 ? 1u : 0u) << j;
                        for (unsigned gm = 0; gm < 8; ++gm) {
                            if (gm & ~present) continue;
                            run(n, gm, out);
                            std::printf("b %d %u %u %d %u %u %u %u %u %d %d %u ", off, l, r, WB, wv, element_of(m.A),
                                        element_of(m.H[0]), element_of(m.H[1]), element_of(m.H[2]), int(alt), n.gates, gm);
                            print_hex(out);
                        }
                    }
                }
    for (int i = 0; i < kGf8NetTableSize; ++i) {
        const Gf8NetEntry& e = kGf8NetTable[i];
        if (!net_ok(e.net, e.M[0], e.M[1], e.M[2], e.M[3])) return 1;
    }
    std::printf("table %d %u\n", kGf8NetTableSize, missing);
    return 0;
}
