// bgzf_device.hpp -- the pieces the source readers of the engine share (bgzf.hip: BAM, sam.hip: SAM): the member directory
// of a BGZF chunk, a growable device array, and launchers of the two kernels both use (defined in bgzf.hip).  The streaming
// pipeline built from them is source_stream.hpp.
#pragma once
#include <algorithm>
#include <vector>

#include "bgzf_core.hpp"
#include "gffx_device.hpp"

namespace gffx {

using u64 = unsigned long long;

struct BgzfDir {  // one member of a chunk
    u64 src;      // offset of the member in the chunk's compressed bytes
    u64 dst;      // offset of its output in D
    uint32_t len;    // the member's length (BSIZE + 1)
    uint32_t isize;  // its output length (the footer's ISIZE)
};

template <class T>
struct DevArr {
    T *p = nullptr;
    size_t cap = 0;
    ~DevArr() {
        if (p) (void)hipFree(p);
    }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        const size_t c = std::max(n, cap + cap / 2);  // (grow by 1.5x at least)
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(&p, c * sizeof(T));
        if (e == hipSuccess) cap = c;
        return e;
    }
};

constexpr uint32_t kMaxBlocksPerBatch = 1u << 16;  // members per sub-batch

// walks the members of buf[0, n): their lengths and ISIZEs.  base: buf's offset in the file (for the message).
int walk_members(const uint8_t *buf, uint64_t n, uint64_t base, std::vector<BgzfDir> *dir);
int check_device(int device);

// k_bgzf_inflate on stream s: members dir[0, nb) of `in` to out + dir[i].dst, one wave per member; status[i] = its
// bgzf::Status, *bad_block = the lowest i whose status is not kOk (the caller initialises it to UINT32_MAX)
void launch_bgzf_inflate(hipStream_t s, const uint8_t *in, const BgzfDir *dir, uint32_t nb, uint8_t *out, int32_t *status,
                         uint32_t *bad_block);
// k_scan on stream s: out[0..n] = exclusive prefix of in[0..n) (out[n] = the total); *total too unless NULL
void launch_scan(hipStream_t s, const uint32_t *in, uint32_t n, u64 *out, u64 *total);

}  // namespace gffx
