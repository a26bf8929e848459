// string_table.hip -- the two kernels that build a string table of ids_core.hpp on the device, behind the launchers of
// string_table.hpp.
//
//   k_table_fill    one thread per slot: the slot empty, its value where the settling atomic starts from.
//   k_table_insert  one thread per string f: ids::table_insert_one<kLargest>.  Contention: the slots are 2 n or more and the
//                   hash spreads the names, so the returning atomic of a thread meets another thread's only for equal strings
//                   (CDS rows that share an ID) and colliding names; the atomicMax returns nothing.  Under hash_bits < 32 (a
//                   test hook) the chains are long on purpose.
#include "string_table.hpp"

namespace gffx {
namespace ids {

__global__ __launch_bounds__(256) void k_table_fill(u64 *slot, uint32_t *val, uint32_t slots, uint32_t v) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < slots) {
        slot[i] = kEmptyWord;
        val[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_table_insert(u64 *slot, uint32_t *val, const uint8_t *bytes, const u64 *off, uint32_t n,
                                                      uint32_t mask, uint32_t hash_mask) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < n) table_insert_one<Keep::kLargest>(slot, val, bytes, off, f, mask, hash_mask);
}

void launch_table_fill(hipStream_t s, u64 *slot, uint32_t *val, uint32_t slots, Keep keep) {
    hipLaunchKernelGGL(k_table_fill, dim3((slots + 255) / 256), dim3(256), 0, s, slot, val, slots, fill_value(keep));
}

void launch_table_build(hipStream_t s, u64 *slot, uint32_t *val, uint32_t slots, const uint8_t *bytes, const u64 *off, uint32_t n,
                        uint32_t hash_mask) {
    launch_table_fill(s, slot, val, slots, Keep::kLargest);
    if (n) hipLaunchKernelGGL(k_table_insert, dim3((n + 255) / 256), dim3(256), 0, s, slot, val, bytes, off, n, slots - 1, hash_mask);
}

}  // namespace ids
}  // namespace gffx
