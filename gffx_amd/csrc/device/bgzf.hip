// bgzf.hip -- BAM sources on the device: BGZF inflate, record framing and the (seqid, start, end) rows of `gffx depth` /
// `gffx coverage` (reference: commands/depth.rs:297-427 process_bam, commands/coverage.rs:125-204).
//
// One fed chunk of whole BGZF members becomes, on one stream:
//   k_bgzf_inflate   one wave per member.  Lane 0 builds the Huffman tables in LDS and decodes into a 64 KiB LDS staging
//                    copy of the member's output (back-references are LDS copies); the whole wave then stores the output
//                    and computes its CRC32 (64 stripes, combined with the x^(8n) shift operator).  LDS: 64 KiB output +
//                    3.9 KiB tables + 1.3 KiB CRC table / lane registers = 70.7 KiB per wave, so 2 waves per CU (160 KiB).
//   framing          the decompressed stream D is the previous chunk's unfinished record (the carry, segment 0) followed by
//                    one segment per member.  k_frame_guess: one thread per segment walks the record chain on the guess that
//                    a record starts at the segment's first byte (htslib's writer flushes a block before a record that
//                    would not fit, so this holds for samtools-written files).  k_frame_fix: one thread checks the guesses
//                    by induction from the true start (the header's end, or the carry's start) -- segment s's guess holds
//                    iff the true chain reaches its first byte -- and walks the chain itself through segments where it
//                    does not (files written with records spanning blocks), until chain and segment start align again.
//                    k_frame_list writes every complete record's offset (the scan of the per-segment counts places them).
//   k_bam_rows       one wave per segment, one lane per record: validate (bgzf_core.hpp bam_record), keep or skip, and
//                    compact the kept rows in file order (count pass, scan over the segments, write pass).
// The unfinished record at D's end is carried into the next chunk (any size), so device memory is bounded by the chunk
// size plus the longest record.  Staging, the sub-batches of members, the drain's sync, rows and carry, and the sticky
// failure are the pipeline of source_stream.hpp, shared with sam.hip; this file keeps the kernels, their enqueue, the
// check of ChunkResult in the middle of the drain (a malformed record, named by the member it begins in) and _finish.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "source_stream.hpp"

namespace gffx {

struct ChunkResult {  // what the host reads back after a chunk (pinned)
    u64 tail;                // D[tail, N) is the unfinished record (the next chunk's carry)
    u64 err_off;             // offset in D of a malformed record
    u64 records, unmapped, no_seq, kept;
    uint32_t bad_block;      // first member that failed to inflate (UINT32_MAX: none)
    int32_t frame_status;    // bgzf::kMalformed: a record with block_size < 32 in the chain
    int32_t rows_status;     // bgzf::kMalformed: a record bam_record() rejects
    uint32_t pad;
};

struct __align__(16) InflateLds {
    bgzf::Scratch s;
    uint32_t crc_table[256];
    uint32_t lane_crc[64];
    int32_t status;
    uint32_t n;
    uint8_t out[bgzf::kMaxIsize];
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *in, const BgzfDir *dir, uint32_t n_blocks, uint8_t *out,
                                                     int32_t *status, uint32_t *bad_block) {
    __shared__ InflateLds L;
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_blocks) return;
    for (uint32_t i = lane; i < 256; i += 64) L.crc_table[i] = bgzf::crc_table_entry(i);
    const BgzfDir d = dir[b];
    if (lane == 0) {
        uint32_t total = 0, isize = 0;
        int st = bgzf::member_inflate(in + d.src, d.len, L.out, d.isize, &total, &isize, &L.s, nullptr);
        if (st == bgzf::kOk && (total != d.len || isize != d.isize)) st = bgzf::kIsize;
        L.status = st;
        L.n = st == bgzf::kOk ? isize : 0;
    }
    __syncthreads();
    const uint32_t n = L.n;
    int st = L.status;
    // CRC: lane i's stripe [i * S, min(n, (i + 1) * S)), register from 0; combined by lane 0 with the shift operator
    const uint32_t S = (n + 63) / 64, a = min(n, lane * S), z = min(n, a + S);
    L.lane_crc[lane] = bgzf::crc_raw(L.crc_table, 0u, L.out + a, z - a);
    uint8_t *o = out + d.dst;
    for (uint32_t i = lane; i < n; i += 64) o[i] = L.out[i];
    __syncthreads();
    if (lane == 0) {
        if (st == bgzf::kOk) {
            const uint32_t opS = bgzf::x8n_mod_p(S);
            uint32_t acc = 0;
            for (uint32_t i = 0; i < 64; ++i) {
                const uint32_t ai = min(n, i * S), zi = min(n, ai + S);
                acc = bgzf::gf2_mul(zi - ai == S ? opS : bgzf::x8n_mod_p(zi - ai), acc) ^ L.lane_crc[i];
            }
            const uint32_t crc = acc ^ bgzf::gf2_mul(bgzf::x8n_mod_p(n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
            if (crc != bgzf::le32(in + d.src + d.len - 8)) st = bgzf::kCrc;
        }
        status[b] = st;
        if (st != bgzf::kOk) atomicMin(bad_block, b);
    }
}

__device__ __forceinline__ int32_t rd_i32(const uint8_t *p) { return (int32_t)bgzf::le32(p); }

// one thread per segment: bgzf::frame_guess
__global__ __launch_bounds__(256) void k_frame_guess(const uint8_t *D, u64 N, const u64 *seg, uint32_t n_seg, u64 *guess_end,
                                                     uint32_t *guess_n, const ChunkResult *res) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg || res->bad_block != 0xFFFFFFFFu) return;
    bgzf::frame_guess(D, N, seg[s], seg[s + 1], guess_end + s, guess_n + s);
}

// one thread: bgzf::frame_fix, the true chain from `start` proven segment by segment (see the file comment)
__global__ void k_frame_fix(const uint8_t *D, u64 N, const u64 *seg, uint32_t n_seg, u64 start, const u64 *guess_end,
                            const uint32_t *guess_n, u64 *entry, uint32_t *count, ChunkResult *res) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (res->bad_block != 0xFFFFFFFFu) return;
    u64 tail = N, err = 0;
    if (bgzf::frame_fix(D, N, seg, n_seg, start, guess_end, guess_n, entry, count, &tail, &err) != bgzf::kOk) {
        res->frame_status = bgzf::kMalformed;
        res->err_off = err;
    }
    res->tail = tail;
}

// single block: out[0..n] = exclusive prefix of in[0..n) (out[n] = total); *total too
__global__ __launch_bounds__(1024) void k_scan(const uint32_t *in, uint32_t n, u64 *out, u64 *total) {
    __shared__ u64 part[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023) / 1024, a = min(n, t * per), z = min(n, a + per);
    u64 sum = 0;
    for (uint32_t i = a; i < z; ++i) sum += in[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const u64 v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = part[t] - sum;
    for (uint32_t i = a; i < z; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (t == 1023) {
        out[n] = part[1023];
        if (total) *total = part[1023];
    }
}

__global__ __launch_bounds__(256) void k_frame_list(const uint8_t *D, uint32_t n_seg, const u64 *entry, const uint32_t *count,
                                                    const u64 *base, u64 *rec_off, const ChunkResult *res) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seg || res->bad_block != 0xFFFFFFFFu || res->frame_status) return;
    u64 p = entry[s], o = base[s];
    for (uint32_t c = count[s]; c; --c) {  // (framing proved each of these records complete)
        rec_off[o++] = p;
        p += 4 + (u64)(uint32_t)rd_i32(D + p);
    }
}

// one wave per segment, one lane per record.  WRITE = 0: kept rows per segment into kept_n, the skip tallies, malformed
// records.  WRITE = 1: the kept rows at out_base[s] (compacted in file order).
template <int WRITE>
__global__ __launch_bounds__(64) void k_bam_rows(const uint8_t *D, const u64 *rec_base, const u64 *rec_off, uint32_t n_ref,
                                                 const uint32_t *ref_seq, uint32_t *kept_n, const u64 *out_base, uint32_t *rows,
                                                 ChunkResult *res) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (res->bad_block != 0xFFFFFFFFu || res->frame_status) return;
    const u64 a = rec_base[s], z = rec_base[s + 1];
    u64 o = WRITE ? out_base[s] : 0;
    uint32_t unm = 0, noseq = 0;
    for (u64 r0 = a; r0 < z; r0 += 64) {
        const u64 r = r0 + lane;
        bool keep = false;
        bgzf::Row row{0, 0, 0, 0};
        uint32_t seq = 0xFFFFFFFFu;
        if (r < z) {
            const int st = bgzf::bam_record(D + rec_off[r], n_ref, &row);
            if (st == bgzf::kMalformed) {
                if (!WRITE && atomicCAS(&res->rows_status, 0, (int32_t)bgzf::kMalformed) == 0) res->err_off = rec_off[r];
            } else if (row.flag & 0x4) {
                ++unm;
            } else if (row.tid < 0 || (seq = ref_seq[row.tid]) == 0xFFFFFFFFu) {
                ++noseq;
            } else if (st == bgzf::kKeep) {
                keep = true;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (WRITE && keep) {
            const u64 at = o + __popcll(m & ((1ull << lane) - 1));
            rows[3 * at] = seq;
            rows[3 * at + 1] = row.start;
            rows[3 * at + 2] = row.end;
        }
        o += __popcll(m);
    }
    if (!WRITE) {
        if (lane == 0) {
            kept_n[s] = (uint32_t)o;
            atomicAdd(&res->records, z - a);
        }
        if (unm) atomicAdd(&res->unmapped, (u64)unm);
        if (noseq) atomicAdd(&res->no_seq, (u64)noseq);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// walks the members of buf[0, n): their lengths and ISIZEs.  base: buf's offset in the file (for the message).
int walk_members(const uint8_t *buf, uint64_t n, uint64_t base, std::vector<BgzfDir> *dir) {
    uint64_t at = 0, dst = 0;
    while (at < n) {
        uint32_t total = 0, hdr = 0;
        const int st = bgzf::member_header(buf + at, n - at, &total, &hdr);
        if (st != bgzf::kOk)
            return fail(GFFX_E_INVALID, "BGZF block at file offset %llu: %s", (unsigned long long)(base + at), bgzf::status_name(st));
        const uint32_t isize = bgzf::le32(buf + at + total - 4);
        if (isize > bgzf::kMaxIsize)
            return fail(GFFX_E_INVALID, "BGZF block at file offset %llu: %s", (unsigned long long)(base + at), bgzf::status_name(bgzf::kIsize));
        dir->push_back({at, dst, total, isize});
        dst += isize;
        at += total;
    }
    return GFFX_OK;
}

int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    if (ndev <= 0) return fail(GFFX_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFFX_E_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
    return GFFX_OK;
}

void launch_bgzf_inflate(hipStream_t s, const uint8_t *in, const BgzfDir *dir, uint32_t nb, uint8_t *out, int32_t *status,
                         uint32_t *bad_block) {
    if (nb) hipLaunchKernelGGL(k_bgzf_inflate, dim3(nb), dim3(64), 0, s, in, dir, nb, out, status, bad_block);
}

void launch_scan(hipStream_t s, const uint32_t *in, uint32_t n, u64 *out, u64 *total) {
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, in, n, out, total);
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_bam {
    uint32_t n_ref = 0;
    DevArr<ChunkResult> res;
    DevArr<uint32_t> ref_seq, guess_n, count, kept_n;
    DevArr<u64> seg, guess_end, entry, rec_base, rec_off, out_base;
    // the sub-batch in flight, beside what the pipeline keeps of it
    uint32_t n_blocks = 0;
    uint64_t fl_carry = 0;        // the carry in front of its members in D
    uint64_t carry_file_off = 0;  // file offset of the member in which the carried record begins
    std::vector<u64> seg_host;    // its segment bounds (the source of an asynchronous copy: kept until the next enqueue)
    uint64_t records = 0;
    SourceStream s;  // (last, so destroyed first: its streams are idle before the arrays above are freed)
};

namespace {
// file offset of the member whose output holds byte `off` of the in-flight sub-batch's D (the carry: where its record began)
uint64_t member_of(const gffx_hip_bam *h, uint64_t off) {
    const SourceStream &S = h->s;
    if (off < h->fl_carry || S.fl_dir.empty()) return h->carry_file_off;
    uint64_t m = S.fl_dir[0].src;
    for (const BgzfDir &d : S.fl_dir)
        if (h->fl_carry + d.dst <= off) m = d.src;
    return S.fl_file_off + m;
}

// waits for the sub-batch in flight, takes its rows and moves its unfinished record to the other D buffer.  (The copies of
// the next sub-batch are already on their way: stage_upload runs before this.)
int drain(gffx_hip_bam *h) {
    SourceStream &S = h->s;
    if (!S.in_flight) return GFFX_OK;
    if (int rc = S.drain_front(&S.result<ChunkResult>()->bad_block)) return rc;
    const ChunkResult r = *S.result<ChunkResult>();
    if (r.frame_status || r.rows_status)
        return fail(GFFX_E_INVALID, "malformed BAM record (block_size, read name or CIGAR out of range, or refID not in the header) "
                                    "that begins in the BGZF block at file offset %llu",
                    (unsigned long long)member_of(h, r.err_off));
    h->records += r.records;
    if (S.n_D - r.tail) h->carry_file_off = member_of(h, r.tail);
    return S.drain_back(r.tail, r.kept, r.unmapped, r.no_seq);
}

// enqueues the kernels on members dir[0, nb) of in[k] (once their copies have arrived): inflate after the carry, frame, rows
int enqueue(gffx_hip_bam *h, int k, uint32_t nb, uint64_t file_off) {
    SourceStream &S = h->s;
    const BgzfDir *dir = S.stage_dir[k];
    const uint64_t C = S.carry;
    uint64_t T = 0;
    for (uint32_t i = 0; i < nb; ++i) T += dir[i].isize;
    const uint64_t N = C + T;
    const uint32_t n_seg = nb + 1;
    std::vector<u64> &seg = h->seg_host;
    seg.assign(n_seg + 1, 0);
    for (uint32_t i = 0; i < nb; ++i) seg[i + 1] = C + dir[i].dst;
    seg[n_seg] = N;
    const u64 start = std::min<u64>(S.skip, N);
    S.skip -= start;
    const size_t max_rec = N / 36 + 1;
    GFFX_HIP_TRY(S.D[S.cur].ensure(N));
    GFFX_HIP_TRY(S.status.ensure(nb));
    GFFX_HIP_TRY(h->seg.ensure(n_seg + 1));
    GFFX_HIP_TRY(h->guess_end.ensure(n_seg));
    GFFX_HIP_TRY(h->guess_n.ensure(n_seg));
    GFFX_HIP_TRY(h->entry.ensure(n_seg));
    GFFX_HIP_TRY(h->count.ensure(n_seg));
    GFFX_HIP_TRY(h->kept_n.ensure(n_seg));
    GFFX_HIP_TRY(h->rec_base.ensure(n_seg + 1));
    GFFX_HIP_TRY(h->out_base.ensure(n_seg + 1));
    GFFX_HIP_TRY(h->rec_off.ensure(max_rec));
    GFFX_HIP_TRY(S.rows.ensure(3 * max_rec));
    hipStream_t s = S.stream;
    uint8_t *D = S.D[S.cur].p;
    ChunkResult *res = h->res.p, *res_host = S.result<ChunkResult>();
    ChunkResult init{};
    init.tail = N;
    init.bad_block = 0xFFFFFFFFu;
    *res_host = init;
    GFFX_HIP_TRY(hipMemcpyAsync(res, res_host, sizeof init, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->seg.p, seg.data(), (n_seg + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipStreamWaitEvent(s, S.copied[k], 0));
    GFFX_HIP_TRY(hipEventRecord(S.ev[0], s));
    if (nb) hipLaunchKernelGGL(k_bgzf_inflate, dim3(nb), dim3(64), 0, s, S.in[k].p, S.dir[k].p, nb, D + C, S.status.p, &res->bad_block);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[1], s));
    hipLaunchKernelGGL(k_frame_guess, dim3((n_seg + 255) / 256), dim3(256), 0, s, D, N, h->seg.p, n_seg, h->guess_end.p, h->guess_n.p, res);
    hipLaunchKernelGGL(k_frame_fix, dim3(1), dim3(64), 0, s, D, N, h->seg.p, n_seg, start, h->guess_end.p, h->guess_n.p, h->entry.p,
                       h->count.p, res);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, h->count.p, n_seg, h->rec_base.p, (u64 *)nullptr);
    hipLaunchKernelGGL(k_frame_list, dim3((n_seg + 255) / 256), dim3(256), 0, s, D, n_seg, h->entry.p, h->count.p, h->rec_base.p,
                       h->rec_off.p, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[2], s));
    hipLaunchKernelGGL(k_bam_rows<0>, dim3(n_seg), dim3(64), 0, s, D, h->rec_base.p, h->rec_off.p, h->n_ref, h->ref_seq.p, h->kept_n.p,
                       h->out_base.p, S.rows.p, res);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, h->kept_n.p, n_seg, h->out_base.p, &res->kept);
    hipLaunchKernelGGL(k_bam_rows<1>, dim3(n_seg), dim3(64), 0, s, D, h->rec_base.p, h->rec_off.p, h->n_ref, h->ref_seq.p, h->kept_n.p,
                       h->out_base.p, S.rows.p, res);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(S.ev[3], s));
    GFFX_HIP_TRY(hipMemcpyAsync(res_host, res, sizeof(ChunkResult), hipMemcpyDeviceToHost, s));
    S.set_in_flight(N, k, nb, file_off);
    h->n_blocks = nb;
    h->fl_carry = C;
    return GFFX_OK;
}
}  // namespace

extern "C" int gffx_hip_bam_create(int device, uint32_t n_ref, const uint32_t *ref_seq, uint64_t header_bytes, uint64_t chunk_bytes,
                                   gffx_hip_bam **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_bam_create: out is NULL");
    *out = nullptr;
    if (n_ref && !ref_seq) return fail(GFFX_E_INVALID, "gffx_hip_bam_create: ref_seq is NULL");
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_bam> h(new (std::nothrow) gffx_hip_bam);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_bam_create: out of host memory");
    h->n_ref = n_ref;
    h->s.skip = header_bytes;
    h->s.chunk_bytes = std::max<uint64_t>(chunk_bytes ? chunk_bytes : (256ull << 20), 1);
    h->s.out_cap = SourceStream::bgzf_out_cap(h->s.chunk_bytes);
    if (int rc = h->s.init(device, "gffx_hip_bam_feed", sizeof(ChunkResult))) return rc;
    GFFX_HIP_TRY(h->res.ensure(1));
    GFFX_HIP_TRY(h->ref_seq.ensure(std::max<uint32_t>(n_ref, 1)));
    if (n_ref) GFFX_HIP_TRY(hipMemcpy(h->ref_seq.p, ref_seq, n_ref * sizeof(uint32_t), hipMemcpyHostToDevice));
    *out = h.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_bam_feed(gffx_hip_bam *h, const uint8_t *bgzf, uint64_t n_bytes) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bam_feed: NULL handle");
    SourceStream &S = h->s;
    if (S.error) return fail(S.error, "%s", S.error_msg.c_str());
    if (n_bytes && !bgzf) return fail(GFFX_E_INVALID, "gffx_hip_bam_feed: NULL input");
    GFFX_HIP_TRY(hipSetDevice(S.device));
    const int rc = S.feed_members(bgzf, n_bytes, [h](int k, uint32_t nb, uint64_t, uint64_t file_off) {
        if (int e = drain(h)) return e;
        return enqueue(h, k, nb, file_off);
    });
    if (rc) return S.sticky(rc);
    S.file_off += n_bytes;
    return GFFX_OK;
}

extern "C" int gffx_hip_bam_finish(gffx_hip_bam *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bam_finish: NULL handle");
    SourceStream &S = h->s;
    if (S.error) return fail(S.error, "%s", S.error_msg.c_str());
    GFFX_HIP_TRY(hipSetDevice(S.device));
    if (int rc = drain(h)) return S.sticky(rc);
    if (S.skip) return S.sticky(fail(GFFX_E_INVALID, "BAM file ends inside its header (%llu bytes missing)", (unsigned long long)S.skip));
    if (S.carry)
        return S.sticky(fail(GFFX_E_INVALID, "BAM file ends inside a record (%llu bytes of an unfinished record)", (unsigned long long)S.carry));
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_bam_rows(const gffx_hip_bam *h) { return h ? h->s.n_rows() : 0; }

extern "C" int gffx_hip_bam_counts(const gffx_hip_bam *h, uint64_t *records, uint64_t *unmapped, uint64_t *no_seq, uint64_t *kept) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bam_counts: NULL handle");
    if (records) *records = h->records;
    if (unmapped) *unmapped = h->s.unmapped;
    if (no_seq) *no_seq = h->s.no_seq;
    if (kept) *kept = h->s.kept;
    return GFFX_OK;
}

extern "C" int gffx_hip_bam_stage_ms(const gffx_hip_bam *h, double *inflate, double *frame, double *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bam_stage_ms: NULL handle");
    h->s.stage_ms(inflate, frame, rows);
    return GFFX_OK;
}

extern "C" int gffx_hip_bam_copy_rows(gffx_hip_bam *h, uint32_t *rows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_bam_copy_rows: NULL handle");
    if (h->s.in_flight) return fail(GFFX_E_STATE, "gffx_hip_bam_copy_rows: call gffx_hip_bam_finish first");
    if (h->s.n_rows() && !rows) return fail(GFFX_E_INVALID, "gffx_hip_bam_copy_rows: rows is NULL");
    h->s.copy_rows(rows);
    return GFFX_OK;
}

extern "C" void gffx_hip_bam_destroy(gffx_hip_bam *h) { delete h; }

extern "C" int gffx_hip_bgzf_inflate(int device, const uint8_t *bgzf, uint64_t n_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out) {
    if (!n_out) return fail(GFFX_E_INVALID, "gffx_hip_bgzf_inflate: n_out is NULL");
    if (n_bytes && !bgzf) return fail(GFFX_E_INVALID, "gffx_hip_bgzf_inflate: NULL input");
    std::vector<BgzfDir> dir;
    if (int rc = walk_members(bgzf, n_bytes, 0, &dir)) return rc;
    const uint64_t total = dir.empty() ? 0 : dir.back().dst + dir.back().isize;
    *n_out = total;
    if (!out) return GFFX_OK;  // size query
    if (cap < total) return fail(GFFX_E_INVALID, "gffx_hip_bgzf_inflate: capacity %llu < %llu decompressed bytes",
                                 (unsigned long long)cap, (unsigned long long)total);
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    if (dir.empty()) return GFFX_OK;
    DevArr<uint8_t> in, o;
    DevArr<BgzfDir> dd;
    DevArr<int32_t> st;
    DevArr<ChunkResult> res;
    GFFX_HIP_TRY(in.ensure(n_bytes));
    GFFX_HIP_TRY(o.ensure(std::max<uint64_t>(total, 1)));
    GFFX_HIP_TRY(dd.ensure(dir.size()));
    GFFX_HIP_TRY(st.ensure(dir.size()));
    GFFX_HIP_TRY(res.ensure(1));
    ChunkResult init{};
    init.bad_block = 0xFFFFFFFFu;
    GFFX_HIP_TRY(hipMemcpy(res.p, &init, sizeof init, hipMemcpyHostToDevice));
    GFFX_HIP_TRY(hipMemcpy(in.p, bgzf, n_bytes, hipMemcpyHostToDevice));
    GFFX_HIP_TRY(hipMemcpy(dd.p, dir.data(), dir.size() * sizeof(BgzfDir), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((uint32_t)dir.size()), dim3(64), 0, 0, in.p, dd.p, (uint32_t)dir.size(), o.p, st.p, &res.p->bad_block);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipDeviceSynchronize());
    GFFX_HIP_TRY(hipMemcpy(&init, res.p, sizeof init, hipMemcpyDeviceToHost));
    if (init.bad_block != 0xFFFFFFFFu) {
        int32_t s = 0;
        GFFX_HIP_TRY(hipMemcpy(&s, st.p + init.bad_block, sizeof s, hipMemcpyDeviceToHost));
        return fail(GFFX_E_INVALID, "BGZF block at file offset %llu: %s", (unsigned long long)dir[init.bad_block].src, bgzf::status_name(s));
    }
    GFFX_HIP_TRY(hipMemcpy(out, o.p, total, hipMemcpyDeviceToHost));
    return GFFX_OK;
}
