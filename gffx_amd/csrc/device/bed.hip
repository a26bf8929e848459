// bed.hip -- BED sources on the device: line finding, field cutting, number reading and the name -> seqid lookup that turn the
// text of a BED file (plain, or BGZF-compressed and inflated by k_bgzf_inflate without leaving the device) into the
// (seqid, start, end) rows of `gffx intersect`, `gffx depth` and `gffx coverage`.  The rules of one line, in the two dialects
// of the host parsers, are bed_core.hpp's, shared with the host.
//
// One chunk of text becomes, on one stream:
//   the text D       the previous chunk's unfinished line (the carry) followed by the new bytes: host text copied in, or the
//                    output of k_bgzf_inflate
//   the line scan    line_scan.hpp, shared with sam.hip: count, scan, list; every '\n' offset in order.  The bytes after the
//                    last '\n' are the carry; at _finish a non-empty carry is the last line.
//   k_bed_rows       one wave per tile, one lane per line that ends in the tile: bed::bed_record, keep or skip, and the kept
//                    rows compacted in file order (count pass, scan over the tiles, write pass) -- the shape of k_sam_rows.
// Staging, the sub-batches, the drain's sync, rows and carry, and the sticky failure are the pipeline of source_stream.hpp.
//
// The first malformed line in file order ends the run: within a sub-batch it is the lowest line index (a 64-bit atomicMin of
// (line << 8) | reason), and sub-batches are drained in order.  Its message is the host parser's; for it the line's bytes
// are copied back from the device -- with a BGZF source the text exists nowhere else.
//
// LANE SHARING: one lane per line, the lane runs bed_record() as the host does (the general per-lane loop; see sam.hip for
// what that costs).  No fast path for the plainest row is built in: tools/bed_device_bench.py measures the stage first.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "line_scan.hpp"
#include "source_stream.hpp"
#include "bed_core.hpp"

namespace gffx {

constexpr u64 kNoBad = 0xFFFFFFFFFFFFFFFFull;

struct BedResult {  // what the host reads back after a chunk (pinned)
    u64 bad;            // (line in the chunk << 8) | bed::Reason of the malformed line with the lowest index (kNoBad: none)
    u64 tail;           // D[tail, N) is the unfinished line (the next chunk's carry)
    u64 lines;          // lines listed
    u64 header_lines;   // (the line scan's; always 0: a BED stream has no header to skip)
    u64 skipped, no_seq, kept;
    uint32_t bad_block; // first member that failed to inflate (UINT32_MAX: none)
    uint32_t pad;
};

// one wave per tile, one lane per line that ends in the tile.  WRITE = 0: kept rows per tile into kept_n, the skip tallies,
// the malformed line with the lowest index (atomicMin: the same line whatever the order the waves run in).  WRITE = 1: the
// kept rows at out_base[t] (compacted in file order); rows holds rows_cap of them, bed::max_kept_lines of the text, so the
// bound on the store is never the one that decides.  Line r is D[r ? nl[r - 1] + 1 : 0, nl[r]); DIALECT kDepth reads it with
// its '\n' (nl[r] < N: the byte at nl[r] is one; nl[r] == N is the file's last line without one).
template <int DIALECT, int WRITE>
__global__ __launch_bounds__(64) void k_bed_rows(const uint8_t *D, u64 N, const u64 *line_base, const uint32_t *nl, sam::Names names,
                                                 uint32_t *kept_n, const u64 *out_base, uint32_t *rows, u64 rows_cap, BedResult *res) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (res->bad_block != 0xFFFFFFFFu) return;
    const u64 a = line_base[t], z = line_base[t + 1];
    u64 o = WRITE ? out_base[t] : 0;
    uint32_t skipped = 0, noseq = 0;
    for (u64 r0 = a; r0 < z; r0 += 64) {
        const u64 r = r0 + lane;
        bool keep = false;
        bed::Row row{};
        if (r < z) {
            const u64 ls = r ? (u64)nl[r - 1] + 1 : 0;
            u64 le = nl[r];
            if (le > N) le = N;  // (never: the list holds offsets below N, and N itself for a final line)
            if (DIALECT == bed::kDepth && le < N) ++le;
            const int st = ls <= le ? bed::bed_record(D + ls, le - ls, DIALECT, names, &row) : (int)bgzf::kSkip;
            if (st == bgzf::kMalformed) {
                if (!WRITE) atomicMin(&res->bad, (r << 8) | (u64)(uint32_t)row.reason);
            } else if (st == bgzf::kKeep) {
                keep = true;
            } else if (row.skip == bed::kNoSeq) {
                ++noseq;
            } else {
                ++skipped;
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
            skipped += __shfl_xor(skipped, d);
            noseq += __shfl_xor(noseq, d);
        }
        if (lane == 0) {
            kept_n[t] = (uint32_t)o;
            if (skipped) atomicAdd(&res->skipped, (u64)skipped);
            if (noseq) atomicAdd(&res->no_seq, (u64)noseq);
        }
    }
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_bed {
    bool bgzf = false;
    int dialect = bed::kIntersect;
    std::vector<uint8_t> pend;  // text fed in pieces smaller than a sub-batch
    DevArr<uint8_t> name_bytes;
    DevArr<BedResult> res;
    DevArr<sam::NameEntry> table;
    uint32_t table_mask = 0;
    DevArr<uint32_t> count, kept_n, nl;
    DevArr<u64> line_base, out_base;
    uint64_t lines = 0;
    SourceStream s;  // (last, so destroyed first: its streams are idle before the arrays above are freed)
};

namespace {
// the sticky failure again, with its first message whole (fail() cuts at 1 KB; a message here may quote a line of any length)
int again(const SourceStream &S) {
    g_last_error = S.error_msg;
    return S.error;
}

// the host parser's message for line `r` of the sub-batch just drained (its text is still in D[cur], its line ends in nl)
int bad_line(gffx_hip_bed *h, u64 r, int reason) {
    if (reason == bed::kBadUtf8) return fail(GFFX_E_INVALID, "invalid utf-8 sequence in BED line");
    SourceStream &S = h->s;
    uint32_t e[2] = {0, 0};  // nl[r - 1], nl[r]
    if (r) GFFX_HIP_TRY(hipMemcpy(e, h->nl.p + (r - 1), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    else GFFX_HIP_TRY(hipMemcpy(e + 1, h->nl.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    const u64 ls = r ? (u64)e[0] + 1 : 0, le = std::min<u64>(e[1], S.n_D);
    std::string line(le > ls ? (size_t)(le - ls) : 0, '\0');
    if (!line.empty()) GFFX_HIP_TRY(hipMemcpy(&line[0], S.D[S.cur].p + ls, line.size(), hipMemcpyDeviceToHost));
    g_last_error = "lexical parse error: invalid BED coordinate in \"" + line + "\"";  // (not through fail(): a line has any length)
    return GFFX_E_INVALID;
}

// waits for the sub-batch in flight, takes its rows and moves its unfinished line to the other D buffer
int drain(gffx_hip_bed *h) {
    SourceStream &S = h->s;
    if (!S.in_flight) return GFFX_OK;
    if (int rc = S.drain_front(&S.result<BedResult>()->bad_block)) return rc;
    const BedResult r = *S.result<BedResult>();
    if (r.bad != kNoBad) return bad_line(h, r.bad >> 8, (int)(r.bad & 0xFF));
    h->lines += r.lines;
    return S.drain_back(r.tail, r.kept, r.skipped, r.no_seq);
}

// enqueues the kernels on the carry followed by T new text bytes: in[k]'s n_src bytes themselves (nb == 0), or the output of
// its nb members.  k < 0: the carry alone, as the file's last line (final_line).
int enqueue(gffx_hip_bed *h, int k, uint32_t nb, uint64_t T, uint64_t file_off, int final_line) {
    SourceStream &S = h->s;
    const uint64_t C = S.carry, N = C + T;
    if (N > kMaxText) return fail(GFFX_E_INVALID, "line %llu: longer than 4 GiB", (unsigned long long)(h->lines + 1));
    const uint32_t n_tiles = (uint32_t)std::max<uint64_t>((N + kTile - 1) / kTile, 1);
    GFFX_HIP_TRY(S.D[S.cur].ensure(std::max<uint64_t>(N, 1)));  // (no reallocation over a carry: drain sized it)
    GFFX_HIP_TRY(S.status.ensure(std::max<uint32_t>(nb, 1)));
    GFFX_HIP_TRY(h->count.ensure(n_tiles));
    GFFX_HIP_TRY(h->kept_n.ensure(n_tiles));
    GFFX_HIP_TRY(h->line_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->out_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->nl.ensure(N + 1));             // every byte a '\n', and the line end at N
    const uint64_t rows_cap = std::max<uint64_t>(bed::max_kept_lines(N), 1);  // whatever the text: the shortest kept line
    GFFX_HIP_TRY(S.rows.ensure(3 * rows_cap));
    hipStream_t s = S.stream;
    uint8_t *D = S.D[S.cur].p;
    BedResult *res = h->res.p, *res_host = S.result<BedResult>();
    BedResult init{};
    init.bad = kNoBad;
    init.tail = 0;
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
    hipLaunchKernelGGL(k_sam_line_count<BedResult>, dim3(n_tiles), dim3(64), 0, s, D, N, 0, n_tiles, final_line, h->count.p, res);
    launch_scan(s, h->count.p, n_tiles, h->line_base.p, &res->lines);
    hipLaunchKernelGGL(k_sam_line_list<BedResult>, dim3(n_tiles), dim3(64), 0, s, D, N, 0, n_tiles, final_line, h->line_base.p, h->nl.p, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[2], s));
    const sam::Names names{h->table.p, h->name_bytes.p, h->table_mask};
    if (h->dialect == bed::kIntersect) {
        hipLaunchKernelGGL((k_bed_rows<bed::kIntersect, 0>), dim3(n_tiles), dim3(64), 0, s, D, N, h->line_base.p, h->nl.p, names, h->kept_n.p,
                           h->out_base.p, S.rows.p, rows_cap, res);
        launch_scan(s, h->kept_n.p, n_tiles, h->out_base.p, &res->kept);
        hipLaunchKernelGGL((k_bed_rows<bed::kIntersect, 1>), dim3(n_tiles), dim3(64), 0, s, D, N, h->line_base.p, h->nl.p, names, h->kept_n.p,
                           h->out_base.p, S.rows.p, rows_cap, res);
    } else {
        hipLaunchKernelGGL((k_bed_rows<bed::kDepth, 0>), dim3(n_tiles), dim3(64), 0, s, D, N, h->line_base.p, h->nl.p, names, h->kept_n.p,
                           h->out_base.p, S.rows.p, rows_cap, res);
        launch_scan(s, h->kept_n.p, n_tiles, h->out_base.p, &res->kept);
        hipLaunchKernelGGL((k_bed_rows<bed::kDepth, 1>), dim3(n_tiles), dim3(64), 0, s, D, N, h->line_base.p, h->nl.p, names, h->kept_n.p,
                           h->out_base.p, S.rows.p, rows_cap, res);
    }
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[3], s));
    GFFX_HIP_TRY(hipMemcpyAsync(res_host, res, sizeof(BedResult), hipMemcpyDeviceToHost, s));
    S.set_in_flight(N, k, nb, file_off);
    return GFFX_OK;
}

// one sub-batch of plain text (n <= chunk_bytes)
int submit_text(gffx_hip_bed *h, const uint8_t *p, uint64_t n) {
    SourceStream &S = h->s;
    int k = 0;
    if (int rc = S.next_stage(n, &k)) return rc;
    std::memcpy(S.stage[k], p, n);  // while the previous sub-batch runs
    if (int rc = S.stage_upload(k, 0, n)) return rc;
    if (int rc = drain(h)) return rc;
    return enqueue(h, k, 0, n, 0, 0);
}

int feed_text(gffx_hip_bed *h, const uint8_t *p, uint64_t n) {
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

int feed_bgzf(gffx_hip_bed *h, const uint8_t *bgzf, uint64_t n_bytes) {
    return h->s.feed_members(bgzf, n_bytes, [h](int k, uint32_t nb, uint64_t T, uint64_t file_off) {
        if (int rc = drain(h)) return rc;
        return enqueue(h, k, nb, T, file_off, 0);
    });
}
}  // namespace

extern "C" int gffx_hip_bed_create(int device, uint32_t n_seq, const char *names, const uint64_t *name_off, int dialect,
                                   uint64_t chunk_bytes, int bgzf, gffx_hip_bed **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_bed_create: out is NULL");
    *out = nullptr;
    if (n_seq && (!names || !name_off)) return fail(GFFX_E_INVALID, "gffx_hip_bed_create: names or name_off is NULL");
    if (n_seq > (1u << 28)) return fail(GFFX_E_INVALID, "gffx_hip_bed_create: %u seqids (at most 2^28)", n_seq);
    if (dialect != bed::kIntersect && dialect != bed::kDepth)
        return fail(GFFX_E_INVALID, "gffx_hip_bed_create: dialect %d (GFFX_BED_INTERSECT or GFFX_BED_DEPTH)", dialect);
    for (uint32_t r = 0; r < n_seq; ++r)
        if (name_off[r + 1] < name_off[r]) return fail(GFFX_E_INVALID, "gffx_hip_bed_create: name_off is not ascending at %u", r);
    const uint64_t n_name_bytes = n_seq ? name_off[n_seq] : 0;
    if (n_name_bytes >= 0xFFFFFFFFull) return fail(GFFX_E_INVALID, "gffx_hip_bed_create: 4 GiB or more of seqid names");
    std::vector<uint32_t> number(n_seq);
    for (uint32_t r = 0; r < n_seq; ++r) number[r] = r;
    std::vector<sam::NameEntry> table;
    const long dup = sam::names_build(n_seq, reinterpret_cast<const uint8_t *>(names), name_off, number.data(), &table);
    if (dup >= 0)
        return fail(GFFX_E_INVALID, "gffx_hip_bed_create: seqid %ld (%.*s) occurs twice", dup,
                    (int)std::min<uint64_t>(name_off[dup + 1] - name_off[dup], 200), names + name_off[dup]);
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_bed> h(new (std::nothrow) gffx_hip_bed);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_bed_create: out of host memory");
    h->bgzf = bgzf != 0;
    h->dialect = dialect;
    h->s.chunk_bytes = std::max<uint64_t>(chunk_bytes ? chunk_bytes : (64ull << 20), 1);
    h->s.chunk_bytes = std::min<uint64_t>(h->s.chunk_bytes, 1ull << 30);
    h->s.out_cap = h->bgzf ? SourceStream::bgzf_out_cap(h->s.chunk_bytes) : h->s.chunk_bytes;
    if (int rc = h->s.init(device, "gffx_hip_bed_feed", sizeof(BedResult))) return rc;
    GFFX_HIP_TRY(h->res.ensure(1));
    GFFX_HIP_TRY(h->table.ensure(table.size()));
    GFFX_HIP_TRY(hipMemcpy(h->table.p, table.data(), table.size() * sizeof(sam::NameEntry), hipMemcpyHostToDevice));
    h->table_mask = (uint32_t)table.size() - 1;
    GFFX_HIP_TRY(h->name_bytes.ensure(std::max<uint64_t>(n_name_bytes, 1)));
    if (n_name_bytes) GFFX_HIP_TRY(hipMemcpy(h->name_bytes.p, names, n_name_bytes, hipMemcpyHostToDevice));
    *out = h.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_bed_feed(gffx_hip_bed *h, const uint8_t *bytes, uint64_t n_bytes) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bed_feed: NULL handle");
    SourceStream &S = h->s;
    if (S.error) return again(S);
    if (n_bytes && !bytes) return fail(GFFX_E_INVALID, "gffx_hip_bed_feed: NULL input");
    GFFX_HIP_TRY(hipSetDevice(S.device));
    if (int rc = h->bgzf ? feed_bgzf(h, bytes, n_bytes) : feed_text(h, bytes, n_bytes)) return S.sticky(rc);
    S.file_off += n_bytes;
    return GFFX_OK;
}

extern "C" int gffx_hip_bed_finish(gffx_hip_bed *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bed_finish: NULL handle");
    SourceStream &S = h->s;
    if (S.error) return again(S);
    GFFX_HIP_TRY(hipSetDevice(S.device));
    if (!h->pend.empty()) {
        if (int rc = submit_text(h, h->pend.data(), h->pend.size())) return S.sticky(rc);
        h->pend.clear();
    }
    if (int rc = drain(h)) return S.sticky(rc);
    if (S.carry) {  // a last line without '\n'
        if (int rc = enqueue(h, -1, 0, 0, S.file_off, 1)) return S.sticky(rc);
        if (int rc = drain(h)) return S.sticky(rc);
        S.carry = 0;
    }
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_bed_rows(const gffx_hip_bed *h) { return h ? h->s.n_rows() : 0; }

extern "C" int gffx_hip_bed_counts(const gffx_hip_bed *h, uint64_t *lines, uint64_t *skipped, uint64_t *no_seq, uint64_t *kept) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bed_counts: NULL handle");
    if (lines) *lines = h->lines;
    if (skipped) *skipped = h->s.unmapped;  // (the pipeline's first skip tally)
    if (no_seq) *no_seq = h->s.no_seq;
    if (kept) *kept = h->s.kept;
    return GFFX_OK;
}

extern "C" int gffx_hip_bed_stage_ms(const gffx_hip_bed *h, double *inflate, double *lines, double *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bed_stage_ms: NULL handle");
    h->s.stage_ms(inflate, lines, rows);
    return GFFX_OK;
}

extern "C" int gffx_hip_bed_copy_rows(gffx_hip_bed *h, uint32_t *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bed_copy_rows: NULL handle");
    if (h->s.error) return again(h->s);  // after an error the rows are refused
    if (h->s.in_flight || !h->pend.empty()) return fail(GFFX_E_STATE, "gffx_hip_bed_copy_rows: call gffx_hip_bed_finish first");
    if (h->s.n_rows() && !rows) return fail(GFFX_E_INVALID, "gffx_hip_bed_copy_rows: rows is NULL");
    h->s.copy_rows(rows);
    return GFFX_OK;
}

extern "C" void gffx_hip_bed_destroy(gffx_hip_bed *h) { delete h; }
