// scan64.hpp -- the 64-bit exclusive prefix sum of genome.hip and seq.hip, in the tile / carry pattern of the pileup
// (reduce-then-scan: nothing spins anywhere):
//   k_scan64_tile_sums   one block per tile of kScan64Tile values: the tile's sum
//   k_scan64_carry       one block: the tile sums <- their exclusive sum, in place
//   k_scan64_apply       out[i] = the sum of in[0, i), i = 0 .. n (out[n]: the total)
// The input is u32 or u64 words.  Both translation units include this header; the kernels are templates.
#pragma once
#include <cstdint>

#include "gffx_device.hpp"

namespace gffx {

constexpr int kScan64Threads = 256;
constexpr uint32_t kScan64Tile = kScan64Threads * 4;

// exclusive sum of v over the block's 256 threads; *total = the block's whole.  s_w: 4 words
__device__ __forceinline__ u64 scan64_block(u64 v, u64 *s_w, u64 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 base = 0, all = 0;
#pragma unroll
    for (int x = 0; x < kScan64Threads / 64; ++x) {
        if (x < wave) base += s_w[x];
        all += s_w[x];
    }
    *total = all;
    return base + inc - v;
}

template <class T>
__global__ __launch_bounds__(kScan64Threads) void k_scan64_tile_sums(const T *in, u64 n, u64 *tile_sum) {
    __shared__ u64 s_w[kScan64Threads / 64];
    const u64 i0 = (u64)blockIdx.x * kScan64Tile + 4ull * threadIdx.x;
    u64 v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v += i0 + j < n ? (u64)in[i0 + j] : 0ull;
    u64 total;
    (void)scan64_block(v, s_w, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

static __global__ __launch_bounds__(kScan64Threads) void k_scan64_carry(u64 *tile_sum, uint32_t tiles) {
    __shared__ u64 s_w[kScan64Threads / 64];
    u64 run = 0;
    for (uint32_t base = 0; base < tiles; base += kScan64Threads) {
        const uint32_t i = base + threadIdx.x;
        u64 all;
        const u64 ex = scan64_block(i < tiles ? tile_sum[i] : 0ull, s_w, &all);
        if (i < tiles) tile_sum[i] = run + ex;
        run += all;
        __syncthreads();  // (s_w is rewritten by the next step)
    }
}

template <class T>
__global__ __launch_bounds__(kScan64Threads) void k_scan64_apply(const T *in, u64 n, const u64 *carry, u64 *out) {
    __shared__ u64 s_w[kScan64Threads / 64];
    const u64 i0 = (u64)blockIdx.x * kScan64Tile + 4ull * threadIdx.x;
    u64 c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = i0 + j < n ? (u64)in[i0 + j] : 0ull;
    u64 total;
    u64 run = carry[blockIdx.x] + scan64_block(c[0] + c[1] + c[2] + c[3], s_w, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) {
            out[i0 + j] = run;
            run += c[j];
            if (i0 + j + 1 == n) out[n] = run;
        }
    if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
}

// tiles of a scan over n values (one at least: n == 0 still writes out[0])
inline uint32_t scan64_tiles(u64 n) { return (uint32_t)std::max<u64>((n + kScan64Tile - 1) / kScan64Tile, 1); }

// out[0 .. n] on stream s; tile_sum: scan64_tiles(n) words of scratch
template <class T>
void launch_scan64(hipStream_t s, const T *in, u64 n, u64 *tile_sum, u64 *out) {
    const uint32_t tiles = scan64_tiles(n);
    hipLaunchKernelGGL(k_scan64_tile_sums<T>, dim3(tiles), dim3(kScan64Threads), 0, s, in, n, tile_sum);
    hipLaunchKernelGGL(k_scan64_carry, dim3(1), dim3(kScan64Threads), 0, s, tile_sum, tiles);
    hipLaunchKernelGGL(k_scan64_apply<T>, dim3(tiles), dim3(kScan64Threads), 0, s, in, n, (const u64 *)tile_sum, out);
}

}  // namespace gffx
