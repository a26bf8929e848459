// bgzf_device.hpp -- the pieces the source readers of the engine share (bgzf.hip: BAM, sam.hip: SAM): the member directory
// of a BGZF chunk and the launcher of the inflate kernel (defined in bgzf.hip); the device array and the scan launcher come
// with gffx_device.hpp.  The streaming pipeline built from them is source_stream.hpp.
#pragma once
#include <vector>

#include "bgzf_core.hpp"
#include "gffx_device.hpp"

namespace gffx {

struct BgzfDir {  // one member of a chunk
    u64 src;      // offset of the member in the chunk's compressed bytes
    u64 dst;      // offset of its output in D
    uint32_t len;    // the member's length (BSIZE + 1)
    uint32_t isize;  // its output length (the footer's ISIZE)
};

constexpr uint32_t kMaxBlocksPerBatch = 1u << 16;  // members per sub-batch

// walks the members of buf[0, n): their lengths and ISIZEs.  base: buf's offset in the file (for the message).
int walk_members(const uint8_t *buf, uint64_t n, uint64_t base, std::vector<BgzfDir> *dir);

// k_bgzf_inflate on stream s: members dir[0, nb) of `in` to out + dir[i].dst, one wave per member; status[i] = its
// bgzf::Status, *bad_block = the lowest i whose status is not kOk (the caller initialises it to UINT32_MAX)
void launch_bgzf_inflate(hipStream_t s, const uint8_t *in, const BgzfDir *dir, uint32_t nb, uint8_t *out, int32_t *status,
                         uint32_t *bad_block);

}  // namespace gffx
