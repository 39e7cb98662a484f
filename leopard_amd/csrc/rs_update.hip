// rs_update.hip -- in-place recovery update from original-piece deltas
// (leo_amd_update): few inputs, many outputs, accumulate.
//
// The code is linear over its field in every byte column, so when originals
// i_t change by delta_t, recovery piece j changes by XOR_t G[j][i_t] * delta_t
// (G = the encoder's coefficient matrix, obtained by the host from the
// encoder's own kernels on unit pieces, leopard_amd.cpp).  The kernels compute
//   out_j[c] = base_j[c] ^ XOR_{t < NT} g[j][t] * delta_t[c]      (j < R)
// for NT <= kUpdChunk deltas: a wave owns a column strip (V dwords a lane, 16
// bytes at V = 4) and a group of G outputs (1 or 2, launch_update); it loads its NT delta strips and
// computes their byte-permute selectors once, then for each output of its
// group loads base_j, multiply-adds the NT deltas with the output's tables
// (wave-uniform scalar loads from the cached columns) and stores out_j once.
// Every recovery byte is read once and written once, by the same lane, so
// base == out (in place) is safe; every delta byte is read once per output
// group.  No LDS, no barriers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "rs_args.h"

namespace lamd {

namespace {

constexpr unsigned kUpdWaves = 4;  // waves per workgroup, one column strip each

// V dwords of a piece from byte offset `off` through a buffer resource of
// `nbytes` bytes (reads past it return zeros without a memory access)
template <int V>
LDEV void upd_load(uint32_t* v, uint64_t base, uint32_t off, uint32_t nbytes) {
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(base), short(0), int(nbytes), 0x00020000);
    if constexpr (V == 1) {
        v[0] = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
    } else if constexpr (V == 2) {
        const v2u x = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
        v[0] = x.x, v[1] = x.y;
    } else {
        const v4u x = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    }
}
template <int V>
LDEV void upd_store(uint64_t base, uint32_t off, const uint32_t* v) {
    using T = typename VecT<V>::type;
    T x;
    if constexpr (V == 1) x = v[0];
    else if constexpr (V == 2) x = T{v[0], v[1]};
    else x = T{v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(x, gptr<T>(reinterpret_cast<uint8_t*>(base) + off));
}

// Byte offset of lane group g (V dwords; FF16: V low-byte dwords here and
// their high-byte dwords 32 bytes on, the two halves of a 64-byte block).
template <class F, int V>
LDEV uint32_t upd_offset(uint32_t g) {
    if constexpr (F::kDw == 1) {
        return g * (4u * V);
    } else {
        constexpr uint32_t per = 8 / V;  // lane groups per 64-byte block
        return (g / per) * 64u + (g % per) * (4u * V);
    }
}

// the byte-permute selectors of one dword: 3 for its bit fields 0-2, 3-5, 6-7
struct Sel3 {
    uint32_t s0, s1, s2;
};
LDEV Sel3 sel3(uint32_t y) { return Sel3{y & 0x07070707u, (y >> 3) & 0x07070707u, (y >> 6) & 0x03030303u}; }

template <class F, int NT, int V, bool LOGS = false>
LDEV void upd_body(const UpdArgs& a) {
    const unsigned wave = uniform(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t g0 = (blockIdx.x * kUpdWaves + wave) * 64u;
    if (g0 >= a.ngroups) return;  // wave-uniform: a strip past the piece
    const bool live = g0 + lane < a.ngroups;
    // dead lanes re-read the last valid columns and never store
    const uint32_t off = upd_offset<F, V>(live ? g0 + lane : a.ngroups - 1);
    const uint32_t nbytes = a.nbytes;
    constexpr int H = F::kDw;  // dword planes: FF8 one, FF16 low bytes and high bytes
    Sel3 s[NT][H][V];
    {
        uint32_t d[NT][H][V];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < H; ++h) upd_load<V>(d[t][h], a.delta[t], off + 32u * h, nbytes);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < H; ++h)
#pragma unroll
                for (int v = 0; v < V; ++v) s[t][h][v] = sel3(d[t][h][v]);
    }
    const unsigned j0 = blockIdx.y * a.G, j1 = min(j0 + a.G, a.R);
    for (unsigned j = j0; j < j1; ++j) {
        const uint64_t bp = uint64_t(reinterpret_cast<uintptr_t>(a.base.ptr(j)));
        const uint64_t op = uint64_t(reinterpret_cast<uintptr_t>(a.out.ptr(j)));
        uint32_t x[H][V];
#pragma unroll
        for (int h = 0; h < H; ++h) upd_load<V>(x[h], bp, off + 32u * h, nbytes);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint32_t* tp;
            if constexpr (LOGS) tp = a.tab16 + size_t(cload(a.col[t] + j)) * F::kTabDw;
            else tp = a.col[t] + size_t(j) * F::kTabDw;
            const typename F::Tab T = F::tab_at(tp);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if constexpr (H == 1) {
                    const Sel3& y = s[t][0][v];
                    x[0][v] = xor3(x[0][v], perm(T.a1, T.a0, y.s0), perm(T.b1, T.b0, y.s1)) ^ perm(T.c0, T.c0, y.s2);
                } else {
                    const Sel3 &lo = s[t][0][v], &hi = s[t][1][v];
                    uint32_t xv[2] = {x[0][v], x[1][v]};
                    FF16::muladd_sel(xv, FF16::Sel{lo.s0, lo.s1, lo.s2, hi.s0, hi.s1, hi.s2}, T);
                    x[0][v] = xv[0];
                    x[1][v] = xv[1];
                }
            }
        }
        if (live) {
#pragma unroll
            for (int h = 0; h < H; ++h) upd_store<V>(op, off + 32u * h, x[h]);
        }
    }
}

template <int NT, int V>
__global__ void __launch_bounds__(64 * kUpdWaves) k_ff8_upd(UpdArgs a) {
    upd_body<FF8, NT, V>(a);
}
template <int NT, int V>
__global__ void __launch_bounds__(64 * kUpdWaves) k_ff16_upd(UpdArgs a) {
    upd_body<FF16, NT, V>(a);
}
#if LAMD_EXPERIMENT_ENV
// columns as log values: one more dependent scalar load per table (A/B only)
template <int NT, int V>
__global__ void __launch_bounds__(64 * kUpdWaves) k_ff16_upd_logs(UpdArgs a) {
    upd_body<FF16, NT, V, true>(a);
}
#endif

// Widest lanes per field and delta count that keep at least five waves a SIMD
// (kernel-resource-usage: GF(2^16) holds 6 selectors per delta and dword pair,
// GF(2^8) 3 per delta and dword).
constexpr unsigned upd_vmax(bool ff16, unsigned nt) {
    return ff16 ? (nt <= 2 ? 4u : nt <= 4 ? 2u : 1u) : (nt <= 4 ? 4u : 2u);
}
template <bool FF16K, int NT>
const void* upd_kernel_v(unsigned v) {
    constexpr unsigned kMax = upd_vmax(FF16K, NT);
    if constexpr (FF16K) {
        if constexpr (kMax >= 4)
            if (v == 4) return reinterpret_cast<const void*>(&k_ff16_upd<NT, 4>);
        if constexpr (kMax >= 2)
            if (v == 2) return reinterpret_cast<const void*>(&k_ff16_upd<NT, 2>);
        return v == 1 ? reinterpret_cast<const void*>(&k_ff16_upd<NT, 1>) : nullptr;
    } else {
        if constexpr (kMax >= 4)
            if (v == 4) return reinterpret_cast<const void*>(&k_ff8_upd<NT, 4>);
        return v == 2 ? reinterpret_cast<const void*>(&k_ff8_upd<NT, 2>)
             : v == 1 ? reinterpret_cast<const void*>(&k_ff8_upd<NT, 1>)
                      : nullptr;
    }
}
#if LAMD_EXPERIMENT_ENV
template <int NT>
const void* upd_kernel_logs_v(unsigned v) {
    constexpr unsigned kMax = upd_vmax(true, NT);
    if constexpr (kMax >= 4)
        if (v == 4) return reinterpret_cast<const void*>(&k_ff16_upd_logs<NT, 4>);
    if constexpr (kMax >= 2)
        if (v == 2) return reinterpret_cast<const void*>(&k_ff16_upd_logs<NT, 2>);
    return v == 1 ? reinterpret_cast<const void*>(&k_ff16_upd_logs<NT, 1>) : nullptr;
}
const void* upd_kernel_logs(unsigned nt, unsigned v) {
    switch (nt) {
        case 1: return upd_kernel_logs_v<1>(v);
        case 2: return upd_kernel_logs_v<2>(v);
        case 3: return upd_kernel_logs_v<3>(v);
        case 4: return upd_kernel_logs_v<4>(v);
        case 5: return upd_kernel_logs_v<5>(v);
        case 6: return upd_kernel_logs_v<6>(v);
        case 7: return upd_kernel_logs_v<7>(v);
        default: return upd_kernel_logs_v<8>(v);
    }
}
#endif
template <bool FF16K>
const void* upd_kernel(unsigned nt, unsigned v) {
    switch (nt) {
        case 1: return upd_kernel_v<FF16K, 1>(v);
        case 2: return upd_kernel_v<FF16K, 2>(v);
        case 3: return upd_kernel_v<FF16K, 3>(v);
        case 4: return upd_kernel_v<FF16K, 4>(v);
        case 5: return upd_kernel_v<FF16K, 5>(v);
        case 6: return upd_kernel_v<FF16K, 6>(v);
        case 7: return upd_kernel_v<FF16K, 7>(v);
        default: return upd_kernel_v<FF16K, 8>(v);
    }
}

// Tables of one coefficient per thread: column blockIdx.y, output j.
template <bool FF16K>
__global__ void __launch_bounds__(256) k_upd_tabs(UpdTabArgs a) {
    const unsigned j = blockIdx.x * 256u + threadIdx.x, u = blockIdx.y;
    if (j >= a.R || u >= a.n) return;
    const uint8_t* row = a.rows + size_t(j) * 64;
    const unsigned p = a.pos[u];
    if constexpr (FF16K) {
        const unsigned val = row[p] | unsigned(row[32 + p]) << 8;
        const unsigned idx = val ? a.vlog[val] : 65536u;  // zero: the all-zero table
        if (a.logs) {
            a.dst[u][j] = idx;
            return;
        }
        const v4u* src = reinterpret_cast<const v4u*>(a.tabs + size_t(idx) * FF16::kTabDw);
        v4u* dst = reinterpret_cast<v4u*>(a.dst[u] + size_t(j) * FF16::kTabDw);
#pragma unroll
        for (int k = 0; k < int(FF16::kTabDw / 4); ++k) dst[k] = src[k];
    } else {
        const v4u* src = reinterpret_cast<const v4u*>(a.tabs + size_t(row[p]) * FF8::kTabDw);  // entry 0 is all zero
        v4u* dst = reinterpret_cast<v4u*>(a.dst[u] + size_t(j) * FF8::kTabDw);
        dst[0] = src[0];
        dst[1] = src[1];
    }
}

}  // namespace

// Grid: column strips (kUpdWaves a workgroup) x output groups of G.  Widest
// lanes first.  G by measurement: one output a wave for few
// deltas -- consecutive workgroups then sweep one recovery piece after the
// other, and 32768+32768 x 64 KiB runs 764 us at G = 1 against 813 / 898 / 900
// at G = 2 / 4 / 8; with more than two deltas G = 2, where the selectors of
// the deltas are worth sharing (1000+200 x 64 KiB, 8 deltas: 17.6 us against
// 18.6 at G = 1 and 18.4 at G = 4), as long as the GPU still gets a full set
// of waves (8 a SIMD).  A call with fewer workgroups than CUs narrows its lanes.
hipError_t launch_update(bool ff16, const UpdArgs& args, unsigned deltas, unsigned cus, hipStream_t s) {
    if (deltas < 1 || deltas > kUpdChunk || args.R == 0 || args.nbytes == 0 || args.nbytes % 64 != 0 ||
        args.nbytes > kUpdMaxLaunchBytes)
        return hipErrorInvalidValue;
    UpdArgs a = args;
    const uint64_t dwords = ff16 ? a.nbytes / 8 : a.nbytes / 4;  // per plane
    auto blocks = [&](unsigned v) { return (dwords / v + 64 * kUpdWaves - 1) / (64 * kUpdWaves); };
    auto groups = [&](unsigned g) { return uint64_t((a.R + g - 1) / g); };
    unsigned v = upd_vmax(ff16, deltas), g = deltas > 2 ? 2 : 1;
    if (g > 1 && blocks(v) * groups(g) < 8ull * cus) g = 1;
    while (v > 1 && blocks(v) * groups(g) < cus) v /= 2;
#if LAMD_EXPERIMENT_ENV
    // A/B of the grid rule: LEO_AMD_UPD_G = 1, 2, 4, 8; LEO_AMD_UPD_V = 1, 2, 4 (at most upd_vmax)
    static const int force_g = [] { const char* e = std::getenv("LEO_AMD_UPD_G"); return e ? std::atoi(e) : 0; }();
    static const int force_v = [] { const char* e = std::getenv("LEO_AMD_UPD_V"); return e ? std::atoi(e) : 0; }();
    if (force_g == 1 || force_g == 2 || force_g == 4 || force_g == 8) g = unsigned(force_g);
    if (force_v == 1 || force_v == 2 || force_v == 4) v = std::min(unsigned(force_v), upd_vmax(ff16, deltas));
#endif
    a.G = g;
    a.ngroups = uint32_t(dwords / v);
    const dim3 grid(unsigned(blocks(v)), unsigned(groups(g)));
    void* params[] = {&a};
    const void* fn = ff16 ? upd_kernel<true>(deltas, v) : upd_kernel<false>(deltas, v);
#if LAMD_EXPERIMENT_ENV
    if (ff16 && a.col_logs) fn = upd_kernel_logs(deltas, v);
#else
    if (a.col_logs) return hipErrorInvalidValue;
#endif
    if (!fn) return hipErrorInvalidValue;
    return hipLaunchKernel(fn, grid, dim3(64 * kUpdWaves), params, 0, s);
}

hipError_t launch_update_tabs(bool ff16, const UpdTabArgs& a, hipStream_t s) {
    if (a.n < 1 || a.n > kUpdMaxChanged || a.R == 0) return hipErrorInvalidValue;
    const dim3 grid((a.R + 255) / 256, a.n);
    if (ff16) hipLaunchKernelGGL(k_upd_tabs<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_upd_tabs<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace lamd
