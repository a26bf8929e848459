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
// Staging, the sub-batches (BGZF members as in bgzf.hip, or plain text in pieces of chunk_bytes), the drain's sync, rows
// and carry, and the sticky failure are the pipeline of source_stream.hpp, shared with bgzf.hip and bed.hip; the two line
// kernels are line_scan.hpp's, shared with bed.hip; this file keeps k_sam_rows, the enqueue, the pending text, the check of
// SamResult in the middle of the drain (the first malformed line) and _finish (a last line without '\n').
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

#include "line_scan.hpp"  // kTile, kMaxText, nl_bits, k_sam_line_count, k_sam_line_list (shared with bed.hip)
#include "source_stream.hpp"
#include "sam_core.hpp"

namespace gffx {

constexpr u64 kNoBad = 0xFFFFFFFFFFFFFFFFull;

struct SamResult {  // what the host reads back after a chunk (pinned)
    u64 bad;            // (line in the chunk << 8) | sam::Reason of the malformed line with the lowest index (kNoBad: none)
    u64 tail;           // D[tail, N) is the unfinished line (the next chunk's carry)
    u64 lines;          // lines listed
    u64 header_lines;   // '\n' before `start`
    u64 unmapped, no_seq, kept;
    uint32_t bad_block; // first member that failed to inflate (UINT32_MAX: none)
    uint32_t pad;
};

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
    bool bgzf = false;
    std::vector<uint8_t> pend;  // text fed in pieces smaller than a sub-batch
    DevArr<uint8_t> name_bytes;
    DevArr<SamResult> res;
    DevArr<sam::NameEntry> table;
    uint32_t table_mask = 0;
    DevArr<uint32_t> count, kept_n, nl;
    DevArr<u64> line_base, out_base;
    uint64_t lines = 0, header_lines = 0;
    SourceStream s;  // (last, so destroyed first: its streams are idle before the arrays above are freed)
};

namespace {
// waits for the sub-batch in flight, takes its rows and moves its unfinished line to the other D buffer
int drain(gffx_hip_sam *h) {
    SourceStream &S = h->s;
    if (!S.in_flight) return GFFX_OK;
    if (int rc = S.drain_front(&S.result<SamResult>()->bad_block)) return rc;
    const SamResult r = *S.result<SamResult>();
    h->header_lines += r.header_lines;
    if (r.bad != kNoBad)
        return fail(GFFX_E_INVALID, "line %llu: %s", (unsigned long long)(h->header_lines + h->lines + (r.bad >> 8) + 1),
                    sam::status_name((int)(r.bad & 0xFF)));
    h->lines += r.lines;
    return S.drain_back(r.tail, r.kept, r.unmapped, r.no_seq);
}

// enqueues the kernels on the carry followed by T new text bytes: in[k]'s n_src bytes themselves (nb == 0), or the output of
// its nb members.  k < 0: the carry alone, as the file's last line (final_line).
int enqueue(gffx_hip_sam *h, int k, uint32_t nb, uint64_t T, uint64_t file_off, int final_line) {
    SourceStream &S = h->s;
    const uint64_t C = S.carry, N = C + T;
    if (N > kMaxText) return fail(GFFX_E_INVALID, "line %llu: longer than 4 GiB", (unsigned long long)(h->header_lines + h->lines + 1));
    const uint32_t n_tiles = (uint32_t)std::max<uint64_t>((N + kTile - 1) / kTile, 1);
    const u64 start = std::min<u64>(S.skip, N);
    S.skip -= start;
    GFFX_HIP_TRY(S.D[S.cur].ensure(std::max<uint64_t>(N, 1)));  // (no reallocation over a carry: drain sized it)
    GFFX_HIP_TRY(S.status.ensure(std::max<uint32_t>(nb, 1)));
    GFFX_HIP_TRY(h->count.ensure(n_tiles));
    GFFX_HIP_TRY(h->kept_n.ensure(n_tiles));
    GFFX_HIP_TRY(h->line_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->out_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->nl.ensure(N + 1));             // every byte a '\n', and the line end at N
    const uint64_t rows_cap = std::max<uint64_t>(sam::max_kept_lines(N), 1);  // whatever the text: the shortest kept line
    GFFX_HIP_TRY(S.rows.ensure(3 * rows_cap));
    hipStream_t s = S.stream;
    uint8_t *D = S.D[S.cur].p;
    SamResult *res = h->res.p, *res_host = S.result<SamResult>();
    SamResult init{};
    init.bad = kNoBad;
    init.tail = start;
    init.bad_block = 0xFFFFFFFFu;
    *res_host = init;
    GFFX_HIP_TRY(hipMemcpyAsync(res, res_host, sizeof init, hipMemcpyHostToDevice, s));
    if (k >= 0) GFFX_HIP_TRY(hipStreamWaitEvent(s, S.copied[k], 0));
    GFFX_HIP_TRY(hipEventRecord(S.ev[0], s));
    if (k >= 0 && nb) {
        launch_bgzf_inflate(s, S.in[k].p, S.dir[k].p, nb, D + C, S.status.p, &res->bad_block);
        GFFX_HIP_TRY(hipGetLastError());
    } else if (k >= 0 && T) {
        GFFX_HIP_TRY(hipMemcpyAsync(D + C, S.in[k].p, T, hipMemcpyDeviceToDevice, s));
    }
    GFFX_HIP_TRY(hipEventRecord(S.ev[1], s));
    hipLaunchKernelGGL(k_sam_line_count<SamResult>, dim3(n_tiles), dim3(64), 0, s, D, N, start, n_tiles, final_line, h->count.p, res);
    launch_scan(s, h->count.p, n_tiles, h->line_base.p, &res->lines);
    hipLaunchKernelGGL(k_sam_line_list<SamResult>, dim3(n_tiles), dim3(64), 0, s, D, N, start, n_tiles, final_line, h->line_base.p, h->nl.p, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[2], s));
    const sam::Names names{h->table.p, h->name_bytes.p, h->table_mask};
    hipLaunchKernelGGL(k_sam_rows<0>, dim3(n_tiles), dim3(64), 0, s, D, start, h->line_base.p, h->nl.p, names, h->kept_n.p, h->out_base.p,
                       S.rows.p, rows_cap, res);
    launch_scan(s, h->kept_n.p, n_tiles, h->out_base.p, &res->kept);
    hipLaunchKernelGGL(k_sam_rows<1>, dim3(n_tiles), dim3(64), 0, s, D, start, h->line_base.p, h->nl.p, names, h->kept_n.p, h->out_base.p,
                       S.rows.p, rows_cap, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[3], s));
    GFFX_HIP_TRY(hipMemcpyAsync(res_host, res, sizeof(SamResult), hipMemcpyDeviceToHost, s));
    S.set_in_flight(N, k, nb, file_off);
    return GFFX_OK;
}

// one sub-batch of plain text (n <= chunk_bytes)
int submit_text(gffx_hip_sam *h, const uint8_t *p, uint64_t n) {
    SourceStream &S = h->s;
    int k = 0;
    if (int rc = S.next_stage(n, &k)) return rc;
    std::memcpy(S.stage[k], p, n);  // while the previous sub-batch runs
    if (int rc = S.stage_upload(k, 0, n)) return rc;
    if (int rc = drain(h)) return rc;
    return enqueue(h, k, 0, n, 0, 0);
}

int feed_text(gffx_hip_sam *h, const uint8_t *p, uint64_t n) {
    const uint64_t chunk = h->s.chunk_bytes;
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
    return h->s.feed_members(bgzf, n_bytes, [h](int k, uint32_t nb, uint64_t T, uint64_t file_off) {
        if (int rc = drain(h)) return rc;
        return enqueue(h, k, nb, T, file_off, 0);
    });
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
    h->bgzf = bgzf != 0;
    h->s.skip = header_bytes;
    h->s.chunk_bytes = std::max<uint64_t>(chunk_bytes ? chunk_bytes : (64ull << 20), 1);
    h->s.chunk_bytes = std::min<uint64_t>(h->s.chunk_bytes, 1ull << 30);
    h->s.out_cap = h->bgzf ? SourceStream::bgzf_out_cap(h->s.chunk_bytes) : h->s.chunk_bytes;
    if (int rc = h->s.init(device, "gffx_hip_sam_feed", sizeof(SamResult))) return rc;
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
    SourceStream &S = h->s;
    if (S.error) return fail(S.error, "%s", S.error_msg.c_str());
    if (n_bytes && !bytes) return fail(GFFX_E_INVALID, "gffx_hip_sam_feed: NULL input");
    GFFX_HIP_TRY(hipSetDevice(S.device));
    if (int rc = h->bgzf ? feed_bgzf(h, bytes, n_bytes) : feed_text(h, bytes, n_bytes)) return S.sticky(rc);
    S.file_off += n_bytes;
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_finish(gffx_hip_sam *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_finish: NULL handle");
    SourceStream &S = h->s;
    if (S.error) return fail(S.error, "%s", S.error_msg.c_str());
    GFFX_HIP_TRY(hipSetDevice(S.device));
    if (!h->pend.empty()) {
        if (int rc = submit_text(h, h->pend.data(), h->pend.size())) return S.sticky(rc);
        h->pend.clear();
    }
    if (int rc = drain(h)) return S.sticky(rc);
    if (S.skip)
        return S.sticky(fail(GFFX_E_INVALID, "the stream ends %llu bytes before the end of its header", (unsigned long long)S.skip));
    if (S.carry) {  // a last line without '\n'
        if (int rc = enqueue(h, -1, 0, 0, S.file_off, 1)) return S.sticky(rc);
        if (int rc = drain(h)) return S.sticky(rc);
        S.carry = 0;
    }
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_sam_rows(const gffx_hip_sam *h) { return h ? h->s.n_rows() : 0; }

extern "C" int gffx_hip_sam_counts(const gffx_hip_sam *h, uint64_t *lines, uint64_t *unmapped, uint64_t *no_seq, uint64_t *kept) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_counts: NULL handle");
    if (lines) *lines = h->lines;
    if (unmapped) *unmapped = h->s.unmapped;
    if (no_seq) *no_seq = h->s.no_seq;
    if (kept) *kept = h->s.kept;
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_stage_ms(const gffx_hip_sam *h, double *inflate, double *lines, double *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_stage_ms: NULL handle");
    h->s.stage_ms(inflate, lines, rows);
    return GFFX_OK;
}

extern "C" int gffx_hip_sam_copy_rows(gffx_hip_sam *h, uint32_t *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_sam_copy_rows: NULL handle");
    if (h->s.in_flight || !h->pend.empty()) return fail(GFFX_E_STATE, "gffx_hip_sam_copy_rows: call gffx_hip_sam_finish first");
    if (h->s.n_rows() && !rows) return fail(GFFX_E_INVALID, "gffx_hip_sam_copy_rows: rows is NULL");
    h->s.copy_rows(rows);
    return GFFX_OK;
}

extern "C" void gffx_hip_sam_destroy(gffx_hip_sam *h) { delete h; }
