// line_scan.hpp -- the line scan of the text sources (sam.hip: SAM, bed.hip: BED), once: a bit per '\n' from 16-byte loads,
// the count pass and the list pass over tiles of kTile bytes.  Both translation units include this header; the kernels are
// templates on the format's result struct R, of which they use three fields:
//   uint32_t bad_block     != UINT32_MAX: a BGZF member failed to inflate, the text is not complete and the kernels return
//   u64 header_lines       the '\n' before `start` are added to it
//   u64 tail               raised to one past the last listed '\n' (the host set it to `start`)
//
// The text D[0, N) is the previous chunk's unfinished line (the carry) followed by the new bytes; the first `start` bytes are
// skipped (a SAM header; 0 for BED).  Line r is D[r ? nl[r - 1] + 1 : start, nl[r]).  The bytes after the last '\n' are the
// carry into the next chunk; at the stream's end a non-empty carry is the last line (a final line need not end in '\n'): the
// last tile then lists one more line end, at N (final_line).
#pragma once
#include <cstdint>

#include "gffx_device.hpp"

namespace gffx {

constexpr uint32_t kTile = 4096;         // bytes per tile: 4 steps of 64 lanes x 16 bytes
constexpr u64 kMaxText = 0xFFFFFFF0ull;  // a chunk with its carry: line ends are 32-bit offsets

// bit i = D[off + i] == '\n', i < 16, off + i < N (off: a multiple of 16; D: 16-byte aligned)
__device__ __forceinline__ uint32_t nl_bits(const uint8_t *D, u64 N, u64 off) {
    uint32_t m = 0;
    if (off + 16 <= N) {
        const uint4 v = *reinterpret_cast<const uint4 *>(D + off);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x = w[k] ^ 0x0A0A0A0Au;
            const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 in exactly the zero bytes of x
            m |= (((z >> 7) * 0x10204080u) >> 28) << (4 * k);                            // bits 0, 8, 16, 24 -> 0 .. 3
        }
    } else {
        for (uint32_t i = 0; off + i < N; ++i)
            if (D[off + i] == '\n') m |= 1u << i;
    }
    return m;
}
// the bits of positions >= start
__device__ __forceinline__ uint32_t from_start(uint32_t m, u64 off, u64 start) {
    if (off >= start) return m;
    return start - off >= 16 ? 0u : m & ~((1u << (uint32_t)(start - off)) - 1u);
}

// one wave per tile: count[t] = the '\n' at or after `start` in tile t (+ 1 in the last tile when final_line: the line end
// at N); the header's '\n' into res->header_lines; res->tail = one past the last listed '\n' (the host set it to start)
template <class R>
__global__ __launch_bounds__(64) void k_sam_line_count(const uint8_t *D, u64 N, u64 start, uint32_t n_tiles, int final_line,
                                                       uint32_t *count, R *res) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tiles || res->bad_block != 0xFFFFFFFFu) return;
    uint32_t c = 0, hdr = 0;
    u64 last = 0;
    for (uint32_t it = 0; it < kTile / 1024; ++it) {
        const u64 off = (u64)t * kTile + it * 1024 + lane * 16;
        if (off >= N) break;
        const uint32_t all = nl_bits(D, N, off), m = from_start(all, off, start);
        c += __popc(m);
        hdr += __popc(all ^ m);
        if (m) last = off + (31 - __clz(m)) + 1;
    }
    for (int d = 32; d; d >>= 1) {
        c += __shfl_xor(c, d);
        hdr += __shfl_xor(hdr, d);
        const u64 o = __shfl_xor(last, d);
        last = o > last ? o : last;
    }
    if (lane == 0) {
        count[t] = c + ((final_line && t == n_tiles - 1) ? 1u : 0u);
        if (hdr) atomicAdd(&res->header_lines, (u64)hdr);
        if (last) atomicMax(&res->tail, last);
    }
}

// one wave per tile: nl[base[t] ..) = the offsets of the tile's listed '\n' in order (and N after them: see k_sam_line_count)
template <class R>
__global__ __launch_bounds__(64) void k_sam_line_list(const uint8_t *D, u64 N, u64 start, uint32_t n_tiles, int final_line,
                                                      const u64 *base, uint32_t *nl, const R *res) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tiles || res->bad_block != 0xFFFFFFFFu) return;
    u64 o = base[t];
    for (uint32_t it = 0; it < kTile / 1024; ++it) {  // (wave-uniform trip count: the shuffles below need every lane)
        const u64 off = (u64)t * kTile + it * 1024 + lane * 16;
        uint32_t m = off < N ? from_start(nl_bits(D, N, off), off, start) : 0u;
        const uint32_t mine = __popc(m);
        uint32_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if ((int)lane >= d) incl += v;
        }
        u64 at = o + incl - mine;
        while (m) {
            const uint32_t b = __ffs(m) - 1;
            m &= m - 1;
            nl[at++] = (uint32_t)(off + b);
        }
        o += __shfl(incl, 63);
    }
    if (final_line && t == n_tiles - 1 && lane == 0) nl[o] = (uint32_t)N;
}

}  // namespace gffx
