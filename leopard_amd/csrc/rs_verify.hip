// rs_verify.hip -- the compare kernel of leo_amd_verify's composed route.
//
// The existing encoder writes the recovery pieces of a column slice into
// workspace scratch; this kernel compares them with the stored pieces and
// reports "any byte differs" per piece.  P pairs a launch (P = R for one
// object, objects x R for a batch): pair p compares the computed piece at
// calc_base + p * calc_stride with the stored piece stored[p] + col0, over
// n16 16-byte columns.  stored[p] == 0 marks a piece that is not checked.
//
// blockIdx.x = pair, blockIdx.y = column block: a workgroup's waves all hold
// one piece, so a whole-wave ballot of "my lanes saw a difference" is that
// piece's verdict for the wave's columns.  Grid-strided over the columns, 16
// bytes a lane and step.  A wave that saw a difference ORs the piece's bit into
// the report with one vector atomic from one lane; a clean stripe writes nothing.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rs_args.h"

namespace lamd {

namespace {

constexpr unsigned kCmpThreads = 256;
constexpr unsigned kCmpUnroll = 4;  // 16-byte columns a lane has in flight per piece and step

__global__ void __launch_bounds__(kCmpThreads) k_verify_cmp(VerifyCmpArgs a) {
    const unsigned p = blockIdx.x;  // < a.pairs (the grid's x extent)
    const uint64_t sp = cload64(a.stored + p);
    if (sp == 0) return;  // not checked (wave-uniform)
    const uint8_t* st = reinterpret_cast<const uint8_t*>(sp) + a.col0;
    const uint8_t* ca = a.calc_base + uint64_t(p) * a.calc_stride;
    const uint64_t step = uint64_t(gridDim.y) * kCmpThreads;
    uint32_t diff = 0;
    uint64_t c = uint64_t(blockIdx.y) * kCmpThreads + threadIdx.x;
    for (; c + (kCmpUnroll - 1) * step < a.n16; c += kCmpUnroll * step) {
        v4u x[kCmpUnroll], y[kCmpUnroll];
#pragma unroll
        for (unsigned u = 0; u < kCmpUnroll; ++u) {
            x[u] = gld<v4u, true>(ca + (c + u * step) * 16);
            y[u] = gld<v4u, true>(st + (c + u * step) * 16);
        }
#pragma unroll
        for (unsigned u = 0; u < kCmpUnroll; ++u) {
            const v4u d = x[u] ^ y[u];
            diff |= d.x | d.y | d.z | d.w;
        }
    }
    for (; c < a.n16; c += step) {
        const v4u d = gld<v4u, true>(ca + c * 16) ^ gld<v4u, true>(st + c * 16);
        diff |= d.x | d.y | d.z | d.w;
    }
    const uint64_t bad = __builtin_amdgcn_ballot_w64(diff != 0);
    if (bad == 0) return;
    if ((threadIdx.x & 63u) == unsigned(__builtin_ctzll(bad))) {
        const unsigned o = p / a.R, j = p % a.R;
        atomicOr(a.report + size_t(o) * a.words + (j >> 5), 1u << (j & 31u));
    }
}

}  // namespace

hipError_t launch_verify_cmp(const VerifyCmpArgs& a, unsigned cus, hipStream_t s) {
    if (a.pairs == 0 || a.n16 == 0) return hipSuccess;
    // column blocks: enough workgroups for every CU's wave slots (8 a CU), no
    // more than the columns give at kCmpUnroll steps a lane, at most 65535
    const uint64_t by_cols = (a.n16 + uint64_t(kCmpThreads) * kCmpUnroll - 1) / (uint64_t(kCmpThreads) * kCmpUnroll);
    const uint64_t want = (uint64_t(cus) * 8 + a.pairs - 1) / a.pairs;
    const unsigned gy = unsigned(std::max<uint64_t>(1, std::min<uint64_t>({by_cols, want, 65535})));
    hipLaunchKernelGGL(k_verify_cmp, dim3(a.pairs, gy), dim3(kCmpThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace lamd
