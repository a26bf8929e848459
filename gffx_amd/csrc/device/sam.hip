// sam.hip -- SAM sources on the device: line finding, field cutting, CIGAR reading and the RNAME -> seqid lookup that turn the
// text of a .sam file (plain, or BGZF-compressed and inflated by k_bgzf_inflate without leaving the device) into the
// (seqid, start, end) rows of `gffx depth` / `gffx coverage` (reference: commands/depth.rs:297-427, coverage.rs:125-204, which
// read .sam through the reader they use for .bam).  The rules of one line are sam_core.hpp's, shared with the host.
//
// One chunk of text becomes, on one stream:
//   the text D       the previous chunk's unfinished line (the carry) followed by the new bytes: host text copied in, or the
//                    output of k_bgzf_inflate.  The first header_bytes of the stream are skipped (`start`).
//   k_sam_line_count one wave per tile of kTile bytes: 16-byte loads, a bit per '\n', popcount.  The '\n' before `start` are
//                    the header's and only counted for the line numbers of messages.
//   k_scan           the per-tile counts into bases.
//   k_sam_line_list  the same pass again; every '\n' offset in order.  Line r is D[r ? nl[r - 1] + 1 : start, nl[r]).  The
//                    bytes after the last '\n' are the carry into the next chunk; at _finish a non-empty carry is the last
//                    line (a final line need not end in '\n'): the last tile then lists one more line end, at N.
//   k_sam_rows       one wave per tile, over the lines that end in the tile: validate (sam_record), keep or skip, and compact
//                    the kept rows in file order (count pass, scan over the tiles, write pass) -- the shape of k_bam_rows.
//
// LANE SHARING in k_sam_rows: one lane per line, and the lane runs sam_record() as the host does.  Reason: there is one code
// path for a 60-byte line, a 1 MB line and a CIGAR of 70,000 operations -- the one tools/sam_check.cpp runs under the
// sanitizers -- so no length at which a cooperative fast path hands over to a serial one exists to be got wrong.  The lines
// of a wave are adjacent in memory (64 short-read lines span about 20 KB), so the byte loads of a lane hit lines of the cache
// its neighbours pull in too; what it costs is that the loads are not coalesced, and that one long line keeps 63 lanes
// idle while a single lane walks its first ten fields (the tags after field 11, where a long read's bulk often is, are not
// walked).  HYPOTHESIS until measured (tools/sam_bench.py, DESIGN "SAM sources"): for short reads the pass is bound by the
// serial walk of about 200 bytes up to the tenth TAB per lane, not by memory.  The alternative, a group of 8 or 16 lanes that
// loads a line's first 128 to 256 bytes and finds the TABs by ballot, is the documented next step.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "bgzf_device.hpp"
#include "sam_core.hpp"

namespace gffx {

constexpr uint32_t kTile = 4096;               // bytes per tile: 4 steps of 64 lanes x 16 bytes
constexpr u64 kNoBad = 0xFFFFFFFFFFFFFFFFull;
constexpr u64 kMaxText = 0xFFFFFFF0ull;        // a chunk with its carry: line ends are 32-bit offsets

struct SamResult {  // what the host reads back after a chunk (pinned)
    u64 bad;            // (line in the chunk << 8) | sam::Reason of the malformed line with the lowest index (kNoBad: none)
    u64 tail;           // D[tail, N) is the unfinished line (the next chunk's carry)
    u64 lines;          // lines listed
    u64 header_lines;   // '\n' before `start`
    u64 unmapped, no_seq, kept;
    uint32_t bad_block; // first member that failed to inflate (UINT32_MAX: none)
    uint32_t pad;
};

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
__global__ __launch_bounds__(64) void k_sam_line_count(const uint8_t *D, u64 N, u64 start, uint32_t n_tiles, int final_line,
                                                       uint32_t *count, SamResult *res) {
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
__global__ __launch_bounds__(64) void k_sam_line_list(const uint8_t *D, u64 N, u64 start, uint32_t n_tiles, int final_line,
                                                      const u64 *base, uint32_t *nl, const SamResult *res) {
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

// one wave per tile, one lane per line that ends in the tile.  WRITE = 0: kept rows per tile into kept_n, the skip tallies,
// the malformed line with the lowest index (atomicMin: the same line whatever the order the waves run in).  WRITE = 1: the
// kept rows at out_base[t] (compacted in file order); rows holds rows_cap of them, sam::max_kept_lines of the text, so the
// bound on the store is never the one that decides.
template <int WRITE>
__global__ __launch_bounds__(64) void k_sam_rows(const uint8_t *D, u64 start, const u64 *line_base, const uint32_t *nl,
                                                 sam::Names names, uint32_t *kept_n, const u64 *out_base, uint32_t *rows,
                                                 u64 rows_cap, SamResult *res) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (res->bad_block != 0xFFFFFFFFu) return;
    const u64 a = line_base[t], z = line_base[t + 1];
    u64 o = WRITE ? out_base[t] : 0;
    uint32_t unm = 0, noseq = 0;
    for (u64 r0 = a; r0 < z; r0 += 64) {
        const u64 r = r0 + lane;
        bool keep = false;
        sam::Row row{};
        if (r < z) {
            const u64 ls = r ? (u64)nl[r - 1] + 1 : start, le = nl[r];
            const int st = sam::sam_record(D + ls, le - ls, names, &row);
            if (st == bgzf::kMalformed) {
                if (!WRITE) atomicMin(&res->bad, (r << 8) | (u64)(uint32_t)row.reason);
            } else if (st == bgzf::kKeep) {
                keep = true;
            } else if (row.skip == sam::kUnmapped) {
                ++unm;
            } else if (row.skip == sam::kNoSeq) {
                ++noseq;
            }
        }
        const unsigned long long m = __ballot(keep);
        const u64 at = o + __popcll(m & ((1ull << lane) - 1));
        if (WRITE && keep && at < rows_cap) {
            rows[3 * at] = row.seq;
            rows[3 * at + 1] = row.start;
            rows[3 * at + 2] = row.end;
        }
        o += __popcll(m);
    }
    if (!WRITE) {
        for (int d = 32; d; d >>= 1) {
            unm += __shfl_xor(unm, d);
            noseq += __shfl_xor(noseq, d);
        }
        if (lane == 0) {
            kept_n[t] = (uint32_t)o;
            if (unm) atomicAdd(&res->unmapped, (u64)unm);
            if (noseq) atomicAdd(&res->no_seq, (u64)noseq);
        }
    }
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_sam {
    int device = 0;
    bool bgzf = false;
    uint64_t skip = 0;         // header bytes still to skip in the text
    uint64_t chunk_bytes = 0;  // fed bytes per sub-batch (text: exactly, but for the last; BGZF: compressed, at most)
    uint64_t out_cap = 0;      // text bytes per sub-batch (without the carry)
    uint64_t file_off = 0;     // bytes fed so far
    hipStream_t stream = nullptr;       // the kernels, in order
    hipStream_t copy_stream = nullptr;  // host -> device copies of the next sub-batch, beside the kernels of this one
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};  // in[k] / dir[k] have arrived
    uint8_t *stage[2] = {nullptr, nullptr};     // pinned fed bytes, double-buffered
    uint64_t stage_cap[2] = {0, 0};
    int cur_stage = 0;
    BgzfDir *stage_dir[2] = {nullptr, nullptr};
    SamResult *res_host = nullptr;  // pinned
    std::vector<uint8_t> pend;      // text fed in pieces smaller than a sub-batch
    DevArr<uint8_t> in[2], D[2], name_bytes;
    DevArr<BgzfDir> dir[2];  // dst relative to the end of the carry
    DevArr<int32_t> status;
    DevArr<SamResult> res;
    DevArr<sam::NameEntry> table;
    uint32_t table_mask = 0;
    DevArr<uint32_t> count, kept_n, nl, rows;
    DevArr<u64> line_base, out_base;
    // the sub-batch in flight (enqueued, not drained)
    bool in_flight = false;
    int cur = 0;         // D[cur] holds its text
    uint64_t carry = 0;  // bytes of the unfinished line at D[cur]'s start (before the in-flight batch: after drain)
    uint64_t n_D = 0;    // its text length
    std::vector<BgzfDir> fl_dir;  // its members (file offsets for messages)
    uint64_t fl_file_off = 0;
    // results
    std::vector<uint32_t> out_rows;
    uint64_t lines = 0, header_lines = 0, unmapped = 0, no_seq = 0, kept = 0;
    double ms[3] = {0, 0, 0};  // inflate (text: the copy behind the carry), lines, rows
    int error = GFFX_OK;
    std::string error_msg;

    ~gffx_hip_sam() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        for (int k = 0; k < 2; ++k) {
            if (copied[k]) (void)hipEventDestroy(copied[k]);
            if (stage[k]) (void)hipHostFree(stage[k]);
            if (stage_dir[k]) (void)hipHostFree(stage_dir[k]);
        }
        if (res_host) (void)hipHostFree(res_host);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

namespace {
int sticky(gffx_hip_sam *h, int rc) {
    if (rc != GFFX_OK && h->error == GFFX_OK) {
        h->error = rc;
        h->error_msg = g_last_error;
    }
    return rc;
}

// waits for the sub-batch in flight, takes its rows and moves its unfinished line to the other D buffer
int drain(gffx_hip_sam *h) {
    if (!h->in_flight) return GFFX_OK;
    h->in_flight = false;
    GFFX_HIP_TRY(hipStreamSynchronize(h->stream));
    const SamResult r = *h->res_host;
    if (r.bad_block != 0xFFFFFFFFu) {
        int32_t st = 0;
        GFFX_HIP_TRY(hipMemcpy(&st, h->status.p + r.bad_block, sizeof st, hipMemcpyDeviceToHost));
        return fail(GFFX_E_INVALID, "BGZF block at file offset %llu: %s",
                    (unsigned long long)(h->fl_file_off + h->fl_dir[r.bad_block].src), bgzf::status_name(st));
    }
    h->header_lines += r.header_lines;
    if (r.bad != kNoBad)
        return fail(GFFX_E_INVALID, "line %llu: %s", (unsigned long long)(h->header_lines + h->lines + (r.bad >> 8) + 1),
                    sam::status_name((int)(r.bad & 0xFF)));
    float t = 0;
    for (int k = 0; k < 3; ++k)
        if (hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]) == hipSuccess) h->ms[k] += t;
    h->lines += r.lines;
    h->unmapped += r.unmapped;
    h->no_seq += r.no_seq;
    h->kept += r.kept;
    if (r.kept) {
        const size_t at = h->out_rows.size();
        h->out_rows.resize(at + 3 * r.kept);
        GFFX_HIP_TRY(hipMemcpy(h->out_rows.data() + at, h->rows.p, r.kept * 12, hipMemcpyDeviceToHost));
    }
    const uint64_t c = h->n_D - r.tail;
    const int nxt = 1 - h->cur;
    GFFX_HIP_TRY(h->D[nxt].ensure(c + h->out_cap));
    if (c) GFFX_HIP_TRY(hipMemcpyAsync(h->D[nxt].p, h->D[h->cur].p + r.tail, c, hipMemcpyDeviceToDevice, h->stream));
    h->cur = nxt;
    h->carry = c;
    return GFFX_OK;
}

// starts the copies of stage[k] (n_src bytes, nb members) to in[k] / dir[k] on the copy stream.  Their previous contents
// belonged to the sub-batch before last, which has been drained.
int stage_upload(gffx_hip_sam *h, int k, uint32_t nb, uint64_t n_src) {
    GFFX_HIP_TRY(h->in[k].ensure(std::max<uint64_t>(n_src, 1)));
    GFFX_HIP_TRY(hipMemcpyAsync(h->in[k].p, h->stage[k], n_src, hipMemcpyHostToDevice, h->copy_stream));
    if (nb) {
        GFFX_HIP_TRY(h->dir[k].ensure(nb));
        GFFX_HIP_TRY(hipMemcpyAsync(h->dir[k].p, h->stage_dir[k], nb * sizeof(BgzfDir), hipMemcpyHostToDevice, h->copy_stream));
    }
    GFFX_HIP_TRY(hipEventRecord(h->copied[k], h->copy_stream));
    return GFFX_OK;
}

// enqueues the kernels on the carry followed by T new text bytes: in[k]'s n_src bytes themselves (nb == 0), or the output of
// its nb members.  k < 0: the carry alone, as the file's last line (final_line).
int enqueue(gffx_hip_sam *h, int k, uint32_t nb, uint64_t T, uint64_t file_off, int final_line) {
    const uint64_t C = h->carry, N = C + T;
    if (N > kMaxText) return fail(GFFX_E_INVALID, "line %llu: longer than 4 GiB", (unsigned long long)(h->header_lines + h->lines + 1));
    const uint32_t n_tiles = (uint32_t)std::max<uint64_t>((N + kTile - 1) / kTile, 1);
    const u64 start = std::min<u64>(h->skip, N);
    h->skip -= start;
    GFFX_HIP_TRY(h->D[h->cur].ensure(std::max<uint64_t>(N, 1)));  // (no reallocation over a carry: drain sized it)
    GFFX_HIP_TRY(h->status.ensure(std::max<uint32_t>(nb, 1)));
    GFFX_HIP_TRY(h->count.ensure(n_tiles));
    GFFX_HIP_TRY(h->kept_n.ensure(n_tiles));
    GFFX_HIP_TRY(h->line_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->out_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->nl.ensure(N + 1));             // every byte a '\n', and the line end at N
    const uint64_t rows_cap = std::max<uint64_t>(sam::max_kept_lines(N), 1);  // whatever the text: the shortest kept line
    GFFX_HIP_TRY(h->rows.ensure(3 * rows_cap));
    hipStream_t s = h->stream;
    uint8_t *D = h->D[h->cur].p;
    SamResult *res = h->res.p;
    SamResult init{};
    init.bad = kNoBad;
    init.tail = start;
    init.bad_block = 0xFFFFFFFFu;
    *h->res_host = init;
    GFFX_HIP_TRY(hipMemcpyAsync(res, h->res_host, sizeof init, hipMemcpyHostToDevice, s));
    if (k >= 0) GFFX_HIP_TRY(hipStreamWaitEvent(s, h->copied[k], 0));
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    if (k >= 0 && nb) {
        launch_bgzf_inflate(s, h->in[k].p, h->dir[k].p, nb, D + C, h->status.p, &res->bad_block);
        GFFX_HIP_TRY(hipGetLastError());
    } else if (k >= 0 && T) {
        GFFX_HIP_TRY(hipMemcpyAsync(D + C, h->in[k].p, T, hipMemcpyDeviceToDevice, s));
    }
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    hipLaunchKernelGGL(k_sam_line_count, dim3(n_tiles), dim3(64), 0, s, D, N, start, n_tiles, final_line, h->count.p, res);
    launch_scan(s, h->count.p, n_tiles, h->line_base.p, &res->lines);
    hipLaunchKernelGGL(k_sam_line_list, dim3(n_tiles), dim3(64), 0, s, D, N, start, n_tiles, final_line, h->line_base.p, h->nl.p, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[2], s));
    const sam::Names names{h->table.p, h->name_bytes.p, h->table_mask};
    hipLaunchKernelGGL(k_sam_rows<0>, dim3(n_tiles), dim3(64), 0, s, D, start, h->line_base.p, h->nl.p, names, h->kept_n.p, h->out_base.p,
                       h->rows.p, rows_cap, res);
    launch_scan(s, h->kept_n.p, n_tiles, h->out_base.p, &res->kept);
    hipLaunchKernelGGL(k_sam_rows<1>, dim3(n_tiles), dim3(64), 0, s, D, start, h->line_base.p, h->nl.p, names, h->kept_n.p, h->out_base.p,
                       h->rows.p, rows_cap, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[3], s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->res_host, res, sizeof(SamResult), hipMemcpyDeviceToHost, s));
    h->in_flight = true;
    h->n_D = N;
    if (k >= 0 && nb) h->fl_dir.assign(h->stage_dir[k], h->stage_dir[k] + nb);
    else h->fl_dir.clear();
    h->fl_file_off = file_off;
    return GFFX_OK;
}

// the next staging buffer, at least n bytes
int next_stage(gffx_hip_sam *h, uint64_t n, int *k_out) {
    const int k = h->cur_stage;
    h->cur_stage ^= 1;
    if (n > h->stage_cap[k]) {
        if (h->stage[k]) (void)hipHostFree(h->stage[k]);
        h->stage[k] = nullptr;
        h->stage_cap[k] = 0;
        if (hipHostMalloc((void **)&h->stage[k], n) != hipSuccess)
            return fail(GFFX_E_OOM, "gffx_hip_sam_feed: pinned staging of %llu bytes", (unsigned long long)n);
        h->stage_cap[k] = n;
    }
    *k_out = k;
    return GFFX_OK;
}

// one sub-batch of plain text (n <= chunk_bytes)
int submit_text(gffx_hip_sam *h, const uint8_t *p, uint64_t n) {
    int k = 0;
    if (int rc = next_stage(h, n, &k)) return rc;
    std::memcpy(h->stage[k], p, n);  // while the previous sub-batch runs
    if (int rc = stage_upload(h, k, 0, n)) return rc;
    if (int rc = drain(h)) return rc;
    return enqueue(h, k, 0, n, 0, 0);
}

int feed_text(gffx_hip_sam *h, const uint8_t *p, uint64_t n) {
    const uint64_t chunk = h->chunk_bytes;
    while (n) {
        if (h->pend.empty() && n >= chunk) {
            if (int rc = submit_text(h, p, chunk)) return rc;
            p += chunk;
            n -= chunk;
            continue;
        }
        const uint64_t take = std::min<uint64_t>(n, chunk - h->pend.size());
        h->pend.insert(h->pend.end(), p, p + take);
        p += take;
        n -= take;
        if (h->pend.size() == chunk) {
            if (int rc = submit_text(h, h->pend.data(), chunk)) return rc;
            h->pend.clear();
        }
    }
    return GFFX_OK;
}

int feed_bgzf(gffx_hip_sam *h, const uint8_t *bgzf, uint64_t n_bytes) {
    std::vector<BgzfDir> all;
    if (int rc = walk_members(bgzf, n_bytes, h->file_off, &all)) return rc;
    // sub-batches: at most chunk_bytes compressed, out_cap decompressed, kMaxBlocksPerBatch members (at least one member)
    size_t i = 0;
    while (i < all.size()) {
        size_t j = i;
        uint64_t src = 0, dst = 0;
        while (j < all.size() && (j == i || (src + all[j].len <= h->chunk_bytes && dst + all[j].isize <= h->out_cap &&
                                             j - i < kMaxBlocksPerBatch))) {
            src += all[j].len;
            dst += all[j].isize;
            ++j;
        }
        int k = 0;
        if (int rc = next_stage(h, src, &k)) return rc;
        if (!h->stage_dir[k] && hipHostMalloc((void **)&h->stage_dir[k], kMaxBlocksPerBatch * sizeof(BgzfDir)) != hipSuccess)
            return fail(GFFX_E_OOM, "gffx_hip_sam_feed: pinned directory");
        std::memcpy(h->stage[k], bgzf + all[i].src, src);
        for (size_t x = i; x < j; ++x) {
            BgzfDir d = all[x];
            d.src -= all[i].src;
            d.dst -= all[i].dst;
            h->stage_dir[k][x - i] = d;
        }
        if (int rc = stage_upload(h, k, (uint32_t)(j - i), src)) return rc;
        if (int rc = drain(h)) return rc;
        if (int rc = enqueue(h, k, (uint32_t)(j - i), dst, h->file_off + all[i].src, 0)) return rc;
        i = j;
    }
    return GFFX_OK;
}
}  // namespace

extern "C" int gffx_hip_sam_create(int device, uint32_t n_ref, const char *names, const uint64_t *name_off, const uint32_t *ref_seq,
                                   uint64_t header_bytes, uint64_t chunk_bytes, int bgzf, gffx_hip_sam **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_sam_create: out is NULL");
    *out = nullptr;
    if (n_ref && (!names || !name_off || !ref_seq)) return fail(GFFX_E_INVALID, "gffx_hip_sam_create: names, name_off or ref_seq is NULL");
    if (n_ref > (1u << 28)) return fail(GFFX_E_INVALID, "gffx_hip_sam_create: %u references (at most 2^28)", n_ref);
    for (uint32_t r = 0; r < n_ref; ++r)
        if (name_off[r + 1] < name_off[r]) return fail(GFFX_E_INVALID, "gffx_hip_sam_create: name_off is not ascending at %u", r);
    const uint64_t n_name_bytes = n_ref ? name_off[n_ref] : 0;
    if (n_name_bytes >= 0xFFFFFFFFull) return fail(GFFX_E_INVALID, "gffx_hip_sam_create: 4 GiB or more of reference names");
    std::vector<sam::NameEntry> table;
    const long dup = sam::names_build(n_ref, reinterpret_cast<const uint8_t *>(names), name_off, ref_seq, &table);
    if (dup >= 0)
        return fail(GFFX_E_INVALID, "duplicate @SQ SN:%.*s in the header (@SQ line %ld)",
                    (int)std::min<uint64_t>(name_off[dup + 1] - name_off[dup], 200), names + name_off[dup], dup + 1);
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_sam> h(new (std::nothrow) gffx_hip_sam);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_sam_create: out of host memory");
    h->device = device;
    h->bgzf = bgzf != 0;
    h->skip = header_bytes;
    h->chunk_bytes = std::max<uint64_t>(chunk_bytes ? chunk_bytes : (64ull << 20), 1);
    h->chunk_bytes = std::min<uint64_t>(h->chunk_bytes, 1ull << 30);
    h->out_cap = h->bgzf ? std::min<uint64_t>(std::max<uint64_t>(4 * h->chunk_bytes, 1ull << 20), 1ull << 30) : h->chunk_bytes;
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    for (hipEvent_t &e : h->copied) GFFX_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    GFFX_HIP_TRY(hipHostMalloc((void **)&h->res_host, sizeof(SamResult)));
    GFFX_HIP_TRY(h->res.ensure(1));
    GFFX_HIP_TRY(h->table.ensure(table.size()));
    GFFX_HIP_TRY(hipMemcpy(h->table.p, table.data(), table.size() * sizeof(sam::NameEntry), hipMemcpyHostToDevice));
    h->table_mask = (uint32_t)table.size() - 1;
    GFFX_HIP_TRY(h->name_bytes.ensure(std::max<uint64_t>(n_name_bytes, 1)));
    if (n_name_bytes) GFFX_HIP_TRY(hipMemcpy(h->name_bytes.p, names, n_name_bytes, hipMemcpyHostToDevice));
    *out = h.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_feed(gffx_hip_sam *h, const uint8_t *bytes, uint64_t n_bytes) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_feed: NULL handle");
    if (h->error) return fail(h->error, "%s", h->error_msg.c_str());
    if (n_bytes && !bytes) return fail(GFFX_E_INVALID, "gffx_hip_sam_feed: NULL input");
    GFFX_HIP_TRY(hipSetDevice(h->device));
    if (int rc = h->bgzf ? feed_bgzf(h, bytes, n_bytes) : feed_text(h, bytes, n_bytes)) return sticky(h, rc);
    h->file_off += n_bytes;
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_finish(gffx_hip_sam *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_finish: NULL handle");
    if (h->error) return fail(h->error, "%s", h->error_msg.c_str());
    GFFX_HIP_TRY(hipSetDevice(h->device));
    if (!h->pend.empty()) {
        if (int rc = submit_text(h, h->pend.data(), h->pend.size())) return sticky(h, rc);
        h->pend.clear();
    }
    if (int rc = drain(h)) return sticky(h, rc);
    if (h->skip)
        return sticky(h, fail(GFFX_E_INVALID, "the stream ends %llu bytes before the end of its header", (unsigned long long)h->skip));
    if (h->carry) {  // a last line without '\n'
        if (int rc = enqueue(h, -1, 0, 0, h->file_off, 1)) return sticky(h, rc);
        if (int rc = drain(h)) return sticky(h, rc);
        h->carry = 0;
    }
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_sam_rows(const gffx_hip_sam *h) { return h ? h->out_rows.size() / 3 : 0; }

extern "C" int gffx_hip_sam_counts(const gffx_hip_sam *h, uint64_t *lines, uint64_t *unmapped, uint64_t *no_seq, uint64_t *kept) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_counts: NULL handle");
    if (lines) *lines = h->lines;
    if (unmapped) *unmapped = h->unmapped;
    if (no_seq) *no_seq = h->no_seq;
    if (kept) *kept = h->kept;
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_stage_ms(const gffx_hip_sam *h, double *inflate, double *lines, double *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_stage_ms: NULL handle");
    if (inflate) *inflate = h->ms[0];
    if (lines) *lines = h->ms[1];
    if (rows) *rows = h->ms[2];
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_copy_rows(gffx_hip_sam *h, uint32_t *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_copy_rows: NULL handle");
    if (h->in_flight || !h->pend.empty()) return fail(GFFX_E_STATE, "gffx_hip_sam_copy_rows: call gffx_hip_sam_finish first");
    if (!h->out_rows.empty() && !rows) return fail(GFFX_E_INVALID, "gffx_hip_sam_copy_rows: rows is NULL");
    if (!h->out_rows.empty()) std::memcpy(rows, h->out_rows.data(), h->out_rows.size() * sizeof(uint32_t));
    return GFFX_OK;
}

extern "C" void gffx_hip_sam_destroy(gffx_hip_sam *h) { delete h; }
