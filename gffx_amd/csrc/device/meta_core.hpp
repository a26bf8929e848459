// meta_core.hpp -- the rule of `gffx meta` for the host (g++) and the device (hipcc): where the columns of a stranded depth
// profile around a feature lie in the genome.  A feature is [s, e) with L = e - s on the plus or the minus strand.
// An offset t in the feature's own orientation (0 = its 5' end, L = just behind its 3' end) maps to the genome as
//      plus:  g(t) = s + t            minus:  g(t) = e - t                                 (signed 64-bit)
// so a minus feature is the mirror image of a plus one: its first column starts at its last base e - 1 and runs downwards.
// The columns are cut by B + 1 offsets t_0 <= t_1 <= ... <= t_B:
//   point mode   B = (up + down) / bin,  t_k = a0 - up + k bin,  a0 = 0 (tss), L (tes) or floor(L / 2) (center)
//   scaled mode  B = up / bin + M + down / bin:  t_k = -up + k bin up to k = up / bin;  floor(j L / M), j = 0 .. M, over the
//                body (the product in 64 bits; L < M gives body columns of length 0);  L + j bin behind it
// Column j is the offsets [t_j, t_{j+1}): in the genome [g(t_j), g(t_{j+1})) on plus, [g(t_{j+1}), g(t_j)) on minus, every
// boundary clamped to [0, len] (len: the seqid's length, 2^32 - 1 when none is known).  The clamp is monotone, so the clamped
// boundaries x_k = clamp(g(t_k)) are still ordered, column j is the bases between x_j and x_{j+1}, and with the pileup's B(x)
// (pileup_core.hpp) its bases are |B(x_{j+1}) - B(x_j)|: one evaluation per boundary.
//
// Plain C++17 (GFFX_HD inline, no allocation, no HIP calls): the same code runs in k_pileup_meta (pileup.hip) and in the
// sanitizer build of tools/meta_check.cpp.
#pragma once
#include <cstdint>

#include "bgzf_core.hpp"  // GFFX_HD

namespace gffx {
namespace meta {

typedef unsigned long long u64;
typedef long long i64;

enum : uint32_t { kPoint = 0, kScaled = 1 };
enum : uint32_t { kTss = 0, kTes = 1, kCenter = 2 };

struct Layout {  // (the words of gffx_hip_meta_layout)
    uint32_t mode, anchor, up, down, bin, body_bins;
};

// the number of columns, 0 for a layout that is none: bin == 0, up or down no multiple of bin, an unknown mode or anchor,
// point mode with up + down == 0, scaled mode with no body column
GFFX_HD inline u64 columns(const Layout &y) {
    if (y.bin == 0 || y.up % y.bin || y.down % y.bin) return 0;
    const u64 flank = (u64)(y.up / y.bin) + (u64)(y.down / y.bin);
    if (y.mode == kPoint) return y.anchor <= kCenter ? flank : 0;
    if (y.mode == kScaled) return y.body_bins ? flank + y.body_bins : 0;
    return 0;
}

// t_k, k = 0 .. columns(y), of a feature of length L
GFFX_HD inline i64 offset(const Layout &y, uint32_t L, u64 k) {
    if (y.mode == kPoint) {
        const i64 a0 = y.anchor == kTss ? 0 : y.anchor == kTes ? (i64)L : (i64)(L / 2);
        return a0 - (i64)y.up + (i64)k * (i64)y.bin;
    }
    const u64 n_up = y.up / y.bin;
    if (k <= n_up) return (i64)k * (i64)y.bin - (i64)y.up;
    if (k <= n_up + y.body_bins) return (i64)(((k - n_up) * (u64)L) / y.body_bins);  // (j <= M < 2^32, L < 2^32: the product fits)
    return (i64)L + (i64)(k - n_up - y.body_bins) * (i64)y.bin;
}

// x_k: g(t_k) clamped to [0, len]
GFFX_HD inline uint32_t boundary(const Layout &y, uint32_t s, uint32_t e, bool minus, uint32_t len, u64 k) {
    const i64 t = offset(y, e - s, k);
    const i64 g = minus ? (i64)e - t : (i64)s + t;
    return g < 0 ? 0u : g > (i64)len ? len : (uint32_t)g;
}

// column j of the feature in the genome: [*a, *b), empty (a == b) where the clamp took all of it
GFFX_HD inline void column(const Layout &y, uint32_t s, uint32_t e, bool minus, uint32_t len, u64 j, uint32_t *a, uint32_t *b) {
    const uint32_t x0 = boundary(y, s, e, minus, len, j), x1 = boundary(y, s, e, minus, len, j + 1);
    *a = minus ? x1 : x0, *b = minus ? x0 : x1;
}

}  // namespace meta
}  // namespace gffx
