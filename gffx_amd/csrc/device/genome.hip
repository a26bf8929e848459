// genome.hip -- the genome object of `gffx seq` (C-ABI gffx_hip_genome_*): a plain FASTA text, fed in pieces cut
// anywhere, packed into ONE contiguous arena of bases on the device, with the sequences' names (host), lengths and 64-bit
// arena offsets.  device/seq_core.hpp has the rule of a line.
//
// A piece goes up through one of two pinned staging buffers (the host fills the second while the kernels of the first run) and
// is cut into sub-batches of chunk_bytes.  Per sub-batch of N bytes:
//   k_sam_line_count / k_sam_line_list   (line_scan.hpp) the '\n' from 16-byte loads, per 4 KiB tile, and their offsets
//   k_genome_classify   one thread per line: header, empty or bases and its kept byte count; the headers into a list
//   scan64              (scan64.hpp: tile sums, carry, apply) the lines' 64-bit destinations
//   k_genome_copy       tiled over DESTINATION bytes: a thread owns 16 aligned bytes of the arena, finds their line by one
//                       search over the destinations and gathers forward across line ends -- many short lines per wave, every
//                       store a full aligned 16 bytes; a run inside one line is read with 16-byte (unaligned) loads
// Nothing of the text is carried on the device: a sub-batch may end inside a bases line (the next one begins with its
// continuation, a flag to k_genome_classify), and what must not be cut -- an unfinished header line, a '\r' that may belong to
// a "\r\n" -- is held back on the host and put in front of the next sub-batch.  Headers are few: their names, the duplicate
// check and the sequences' table are the host's.  Errors are sticky (handle_status.hpp).
#include <cstring>
#include <memory>
#include <unordered_map>

#include "handle_status.hpp"
#include "line_scan.hpp"
#include "scan64.hpp"
#include "seq_core.hpp"

using namespace gffx;

namespace {

struct GenomeRes {
    uint32_t bad_block;  // (line_scan.hpp: never set here)
    uint32_t n_headers;
    u64 header_lines;    // (line_scan.hpp: the text has no header part)
    u64 tail;
    u64 first_bases;     // the first non-empty bases line of the sub-batch (only looked for while no sequence is open)
};
struct GenomeHeader {
    uint32_t line, ls, le, pad;  // the line's number in the sub-batch, its bytes D[ls, le) without "\r\n"
    u64 dst;                     // the kept bytes of the sub-batch before it
};

constexpr u64 kNone = ~0ull;
constexpr int kCopyThreads = 256;

__global__ __launch_bounds__(256) void k_genome_classify(const uint8_t *D, u64 N, const uint32_t *nl, u64 n_lines, int final_line, int continuation,
                                                         int want_first, uint32_t *kept, GenomeHeader *hdr, GenomeRes *res) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const u64 ls = i ? (u64)nl[i - 1] + 1 : 0, le = nl[i];
    const bool terminated = !(final_line && i + 1 == n_lines);
    const seq::LineClass c = seq::classify_line(D, ls, le, terminated, continuation && i == 0);
    kept[i] = c.kind == seq::kLineBases ? (uint32_t)c.kept : 0u;
    if (c.kind == seq::kLineHeader) {
        const uint32_t k = atomicAdd(&res->n_headers, 1u);  // (any order: the host sorts the few headers by line)
        const u64 end = terminated && D[le - 1] == '\r' ? le - 1 : le;
        hdr[k] = GenomeHeader{(uint32_t)i, (uint32_t)ls, (uint32_t)end, 0u, 0ull};
    } else if (want_first && c.kind == seq::kLineBases && c.kept) {
        atomicMin(&res->first_bases, i);
    }
    (void)N;
}

__global__ __launch_bounds__(256) void k_genome_header_dst(GenomeHeader *hdr, const u64 *dst, const GenomeRes *res) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < res->n_headers) hdr[k].dst = dst[hdr[k].line];
}

// arena[A + d] = kept byte d of the sub-batch, d < dst[n_lines]
__global__ __launch_bounds__(kCopyThreads) void k_genome_copy(const uint8_t *D, const uint32_t *nl, u64 n_lines, const u64 *dst, uint8_t *arena, u64 A) {
    const u64 total = dst[n_lines];
    const u64 a0 = (A & ~15ull) + 16ull * ((u64)blockIdx.x * kCopyThreads + threadIdx.x);
    const u64 lo = a0 > A ? a0 : A, hi = a0 + 16 < A + total ? a0 + 16 : A + total;
    if (lo >= hi) return;
    const u64 d = lo - A;
    const uint32_t n = (uint32_t)(hi - lo);
    u64 i = seq::last_le(dst, n_lines + 1, d);  // dst[i] <= d < dst[i + 1]: a line with kept bytes
    u64 src = (i ? (u64)nl[i - 1] + 1 : 0) + (d - dst[i]), dend = dst[i + 1];
    if (n == 16 && d + 16 <= dend) {  // the whole run inside one line
        uint4 v;
        __builtin_memcpy(&v, D + src, 16);
        *reinterpret_cast<uint4 *>(arena + lo) = v;
        return;
    }
    uint8_t b[16];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k < n) {
            while (d + k >= dend) {  // (lines without kept bytes are passed here too)
                ++i;
                src = (u64)nl[i - 1] + 1;
                dend = dst[i + 1];
            }
            b[k] = D[src++];
        } else {
            b[k] = 0;
        }
    }
    if (n == 16) {
        uint4 v;
        __builtin_memcpy(&v, b, 16);
        *reinterpret_cast<uint4 *>(arena + lo) = v;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k)
            if (k < n) arena[lo + k] = b[k];
    }
}

}  // namespace

struct gffx_hip_genome : HandleStatus {
    static constexpr const char *kName = "the genome handle", *kNoun = "genome";
    u64 chunk_bytes = 64ull << 20;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    uint8_t *stage[2] = {nullptr, nullptr};  // pinned, double-buffered
    u64 stage_cap[2] = {0, 0};
    int cur_stage = 0;
    GenomeRes *res_host = nullptr;  // pinned
    u64 *n_host = nullptr;          // pinned: the line total, the kept total
    DevArr<uint8_t> D, arena;
    DevArr<uint32_t> count, nl, kept;
    DevArr<u64> line_base, tile_sum, dst, seq_off;
    DevArr<uint32_t> seq_len;
    DevArr<GenomeHeader> hdr;
    DevArr<GenomeRes> res;
    // the text so far
    std::vector<uint8_t> held;  // an unfinished header line, or the '\r' that may belong to a "\r\n"
    bool mid_bases = false;     // the text handed to the device so far ends inside a bases line
    u64 lines_done = 0;         // '\n' handed to the device so far
    u64 arena_used = 0;
    // the sub-batch in flight
    bool in_flight = false;
    int fl_stage = 0;
    u64 fl_lines = 0, fl_lines_before = 0;
    // results
    std::vector<std::string> names;
    std::vector<u64> offs;  // per sequence where it begins in the arena
    std::unordered_map<std::string, uint32_t> by_name;
    std::vector<uint32_t> lens;
    bool finished = false;
    double ms[2] = {0, 0};  // line scan; classify + scan + copy

    ~gffx_hip_genome() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (int k = 0; k < 2; ++k)
            if (stage[k]) (void)hipHostFree(stage[k]);
        if (res_host) (void)hipHostFree(res_host);
        if (n_host) (void)hipHostFree(n_host);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int drain(gffx_hip_genome *h) {
    if (!h->in_flight) return GFFX_OK;
    h->in_flight = false;
    GFFX_HIP_TRY(hipStreamSynchronize(h->stream));
    float t = 0;
    for (int k = 0; k < 2; ++k)
        if (hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]) == hipSuccess) h->ms[k] += t;
    const GenomeRes r = *h->res_host;
    const u64 total = h->n_host[1];
    std::vector<GenomeHeader> hd(r.n_headers);
    if (r.n_headers) GFFX_HIP_TRY(hipMemcpy(hd.data(), h->hdr.p, hd.size() * sizeof(GenomeHeader), hipMemcpyDeviceToHost));
    std::sort(hd.begin(), hd.end(), [](const GenomeHeader &a, const GenomeHeader &b) { return a.line < b.line; });
    if (h->names.empty() && r.first_bases != kNone && (hd.empty() || r.first_bases < hd[0].line))
        return fail(GFFX_E_INVALID, "line %llu: sequence data before the first '>' line", h->fl_lines_before + r.first_bases + 1);
    const uint8_t *text = h->stage[h->fl_stage];
    for (const GenomeHeader &g : hd) {
        const u64 line_no = h->fl_lines_before + g.line + 1;
        const u64 ne = seq::name_end(text, g.ls, g.le);
        if (ne == (u64)g.ls + 1) return fail(GFFX_E_INVALID, "line %llu: a '>' line without a sequence name", line_no);
        std::string name(reinterpret_cast<const char *>(text) + g.ls + 1, (size_t)(ne - g.ls - 1));
        if (!h->by_name.emplace(name, (uint32_t)h->names.size()).second) {
            g_last_error = "line " + std::to_string(line_no) + ": the sequence name \"" + name + "\" is given twice";  // (a name has any length)
            return GFFX_E_INVALID;
        }
        if (h->names.size() >= 0xFFFFFFFEull) return fail(GFFX_E_INVALID, "line %llu: more than 2^32 - 2 sequences", line_no);
        const u64 at = h->arena_used + g.dst;
        if (!h->offs.empty() && at - h->offs.back() > 0xFFFFFFFFull) {
            g_last_error = "FASTA sequence \"" + h->names.back() + "\" has 2^32 bases or more: coordinates are 32-bit";
            return GFFX_E_INVALID;
        }
        h->names.push_back(std::move(name));
        h->offs.push_back(at);
    }
    h->arena_used += total;
    return GFFX_OK;
}

// one sub-batch: the held bytes followed by p[0, n); last: the text ends here
int submit(gffx_hip_genome *h, const uint8_t *p, u64 n, bool last) {
    const int k = h->cur_stage;
    h->cur_stage ^= 1;
    u64 N = h->held.size() + n;
    if (N > h->stage_cap[k]) {
        if (h->stage[k]) (void)hipHostFree(h->stage[k]);
        h->stage[k] = nullptr, h->stage_cap[k] = 0;
        const u64 want = std::max<u64>(N + N / 2, 64u << 10);  // (a piece is at most chunk_bytes: the first full one sizes the buffer)
        if (hipHostMalloc((void **)&h->stage[k], want) != hipSuccess) return fail(GFFX_E_OOM, "gffx_hip_genome_feed: pinned staging of %llu bytes", want);
        h->stage_cap[k] = want;
    }
    uint8_t *S = h->stage[k];  // (filled while the sub-batch before runs)
    if (!h->held.empty()) std::memcpy(S, h->held.data(), h->held.size());
    if (n) std::memcpy(S + h->held.size(), p, n);
    h->held.clear();
    if (!last && N) {
        const void *q = memrchr(S, '\n', N);
        const u64 t0 = q ? (u64)(static_cast<const uint8_t *>(q) - S) + 1 : 0;
        const bool tail_continues = !q && h->mid_bases;
        if (t0 < N) {
            if (!tail_continues && S[t0] == '>') {
                h->held.assign(S + t0, S + N);
                N = t0;
            } else if (S[N - 1] == '\r') {
                h->held.assign(1, '\r');
                N -= 1;
            }
        }
    }
    if (int rc = drain(h)) return rc;
    if (N == 0) return GFFX_OK;
    if (N > kMaxText) return fail(GFFX_E_INVALID, "gffx_hip_genome_feed: a sub-batch of %llu bytes (a header line of 4 GiB?)", N);
    const int final_line = S[N - 1] != '\n';
    const int continuation = h->mid_bases ? 1 : 0;
    const uint32_t n_tiles = (uint32_t)((N + kTile - 1) / kTile);
    hipStream_t s = h->stream;
    GFFX_HIP_TRY(h->D.ensure(N + 16));
    GFFX_HIP_TRY(h->count.ensure(n_tiles));
    GFFX_HIP_TRY(h->line_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->tile_sum.ensure(std::max<u64>(scan64_tiles(n_tiles), scan64_tiles(N + 1))));
    GFFX_HIP_TRY(h->res.ensure(1));
    if (h->arena_used + N + 16 > h->arena.cap) GFFX_HIP_TRY(grow_keep(h->arena, h->arena_used, h->arena_used + N + 16));
    GenomeRes init{};
    init.bad_block = 0xFFFFFFFFu;
    init.first_bases = kNone;
    *h->res_host = init;
    GFFX_HIP_TRY(hipMemcpyAsync(h->res.p, h->res_host, sizeof init, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->D.p, S, N, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_sam_line_count<GenomeRes>, dim3(n_tiles), dim3(64), 0, s, h->D.p, N, 0, n_tiles, final_line, h->count.p, h->res.p);
    launch_scan64(s, h->count.p, (u64)n_tiles, h->tile_sum.p, h->line_base.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipMemcpyAsync(&h->n_host[0], h->line_base.p + n_tiles, sizeof(u64), hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));  // the arrays per line are sized by the line count
    const u64 n_lines = h->n_host[0];
    GFFX_HIP_TRY(h->nl.ensure(n_lines + 1));
    GFFX_HIP_TRY(h->kept.ensure(n_lines + 1));
    GFFX_HIP_TRY(h->dst.ensure(n_lines + 2));
    GFFX_HIP_TRY(h->hdr.ensure(n_lines + 1));
    hipLaunchKernelGGL(k_sam_line_list<GenomeRes>, dim3(n_tiles), dim3(64), 0, s, h->D.p, N, 0, n_tiles, final_line, h->line_base.p, h->nl.p, h->res.p);
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    const uint32_t lb = (uint32_t)((n_lines + 255) / 256);
    hipLaunchKernelGGL(k_genome_classify, dim3(lb), dim3(256), 0, s, h->D.p, N, h->nl.p, n_lines, final_line, continuation, h->names.empty() ? 1 : 0, h->kept.p,
                       h->hdr.p, h->res.p);
    launch_scan64(s, h->kept.p, n_lines, h->tile_sum.p, h->dst.p);
    hipLaunchKernelGGL(k_genome_header_dst, dim3(lb), dim3(256), 0, s, h->hdr.p, h->dst.p, h->res.p);
    const u64 units = N / 16 + 2;  // (16-byte units of the arena that N kept bytes can touch)
    hipLaunchKernelGGL(k_genome_copy, dim3((uint32_t)((units + kCopyThreads - 1) / kCopyThreads)), dim3(kCopyThreads), 0, s, h->D.p, h->nl.p, n_lines, h->dst.p,
                       h->arena.p, h->arena_used);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[2], s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->res_host, h->res.p, sizeof(GenomeRes), hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipMemcpyAsync(&h->n_host[1], h->dst.p + n_lines, sizeof(u64), hipMemcpyDeviceToHost, s));
    h->in_flight = true;
    h->fl_stage = k;
    h->fl_lines = n_lines;
    h->fl_lines_before = h->lines_done;
    h->lines_done += n_lines - (u64)final_line;
    h->mid_bases = final_line != 0;
    return GFFX_OK;
}

}  // namespace

extern "C" int gffx_hip_genome_create(int device, uint64_t chunk_bytes, gffx_hip_genome **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_genome_create: out is NULL");
    *out = nullptr;
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_genome> h(new (std::nothrow) gffx_hip_genome);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_genome_create: out of host memory");
    h->device = device;
    if (chunk_bytes) h->chunk_bytes = std::min<u64>(chunk_bytes, 1ull << 30);
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    GFFX_HIP_TRY(hipHostMalloc((void **)&h->res_host, sizeof(GenomeRes)));
    GFFX_HIP_TRY(hipHostMalloc((void **)&h->n_host, 2 * sizeof(u64)));
    *out = h.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_reserve(gffx_hip_genome *h, uint64_t n_bytes) {
    if (int rc = enter_handle(h, "gffx_hip_genome_reserve")) return rc;
    if (h->finished) return fail(GFFX_E_STATE, "gffx_hip_genome_reserve: the genome is finished");
    GFFX_KEEP_TRY(h, drain(h));
    GFFX_KEEP_HIP(h, grow_keep(h->arena, h->arena_used, n_bytes + 16));
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_feed(gffx_hip_genome *h, const uint8_t *bytes, uint64_t n_bytes) {
    if (int rc = enter_handle(h, "gffx_hip_genome_feed")) return rc;
    if (h->finished) return fail(GFFX_E_STATE, "gffx_hip_genome_feed: the genome is finished");
    if (n_bytes && !bytes) return fail(GFFX_E_INVALID, "gffx_hip_genome_feed: bytes is NULL");
    while (n_bytes) {
        const u64 take = std::min<u64>(n_bytes, h->chunk_bytes);
        GFFX_KEEP_TRY(h, submit(h, bytes, take, false));
        bytes += take;
        n_bytes -= take;
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_finish(gffx_hip_genome *h) {
    if (int rc = enter_handle(h, "gffx_hip_genome_finish")) return rc;
    if (h->finished) return GFFX_OK;
    if (!h->held.empty()) GFFX_KEEP_TRY(h, submit(h, nullptr, 0, true));
    GFFX_KEEP_TRY(h, drain(h));
    const size_t n = h->names.size();
    h->lens.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const u64 len = (i + 1 < n ? h->offs[i + 1] : h->arena_used) - h->offs[i];
        if (len > 0xFFFFFFFFull) {
            g_last_error = "FASTA sequence \"" + h->names[i] + "\" has 2^32 bases or more: coordinates are 32-bit";
            return keep_failure(h, GFFX_E_INVALID);
        }
        h->lens[i] = (uint32_t)len;
    }
    h->offs.push_back(h->arena_used);
    GFFX_KEEP_HIP(h, h->seq_off.ensure(n + 1));
    GFFX_KEEP_HIP(h, h->seq_len.ensure(n + 1));
    GFFX_KEEP_HIP(h, hipMemcpy(h->seq_off.p, h->offs.data(), (n + 1) * sizeof(u64), hipMemcpyHostToDevice));
    if (n) GFFX_KEEP_HIP(h, hipMemcpy(h->seq_len.p, h->lens.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!h->arena.p) GFFX_KEEP_HIP(h, h->arena.ensure(16));
    h->finished = true;
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_device(const gffx_hip_genome *h) { return h ? h->device : -1; }
extern "C" uint32_t gffx_hip_genome_n_seq(const gffx_hip_genome *h) { return h && h->finished ? (uint32_t)h->names.size() : 0; }
extern "C" uint64_t gffx_hip_genome_n_bases(const gffx_hip_genome *h) { return h && h->finished ? h->arena_used : 0; }
extern "C" uint64_t gffx_hip_genome_name_bytes(const gffx_hip_genome *h) {
    uint64_t n = 0;
    if (h && h->finished)
        for (const std::string &s : h->names) n += s.size();
    return n;
}

extern "C" int gffx_hip_genome_copy_names(const gffx_hip_genome *h, uint8_t *names, uint64_t *name_off) {
    if (int rc = enter_handle(h, "gffx_hip_genome_copy_names")) return rc;
    if (!h->finished) return fail(GFFX_E_STATE, "gffx_hip_genome_copy_names: call gffx_hip_genome_finish first");
    uint64_t at = 0;
    for (size_t i = 0; i < h->names.size(); ++i) {
        if (name_off) name_off[i] = at;
        if (names) std::memcpy(names + at, h->names[i].data(), h->names[i].size());
        at += h->names[i].size();
    }
    if (name_off) name_off[h->names.size()] = at;
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_copy_seqs(const gffx_hip_genome *h, uint64_t *offset, uint32_t *length) {
    if (int rc = enter_handle(h, "gffx_hip_genome_copy_seqs")) return rc;
    if (!h->finished) return fail(GFFX_E_STATE, "gffx_hip_genome_copy_seqs: call gffx_hip_genome_finish first");
    if (offset) std::memcpy(offset, h->offs.data(), h->offs.size() * sizeof(u64));
    if (length && !h->lens.empty()) std::memcpy(length, h->lens.data(), h->lens.size() * sizeof(uint32_t));
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_copy_bases(const gffx_hip_genome *h, uint64_t at, uint64_t n, uint8_t *out) {
    if (int rc = enter_handle(h, "gffx_hip_genome_copy_bases")) return rc;
    if (!h->finished) return fail(GFFX_E_STATE, "gffx_hip_genome_copy_bases: call gffx_hip_genome_finish first");
    if (at > h->arena_used || n > h->arena_used - at) return fail(GFFX_E_INVALID, "gffx_hip_genome_copy_bases: [%llu, +%llu) is beyond the %llu bases", at, n, h->arena_used);
    if (n && !out) return fail(GFFX_E_INVALID, "gffx_hip_genome_copy_bases: out is NULL");
    if (n) GFFX_HIP_TRY(hipMemcpy(out, h->arena.p + at, n, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_genome_stage_ms(const gffx_hip_genome *h, double *lines_ms, double *pack_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_genome_stage_ms: the genome handle is NULL");
    if (lines_ms) *lines_ms = h->ms[0];
    if (pack_ms) *pack_ms = h->ms[1];
    return GFFX_OK;
}

extern "C" void gffx_hip_genome_destroy(gffx_hip_genome *h) { delete h; }

// the shape of scan64.hpp: values per tile, and tile sums per step of k_scan64_carry (a block-wide step: one per thread)
extern "C" uint32_t gffx_hip_scan64_tile(void) { return kScan64Tile; }
extern "C" uint32_t gffx_hip_scan64_carry_tiles(void) { return kScan64Threads; }

// what seq.hip reads of a finished genome
namespace gffx {
int genome_view(const gffx_hip_genome *h, const char *who, const uint8_t **arena, const u64 **seq_off, const uint32_t **seq_len, uint32_t *n_seq, int *device) {
    if (int rc = enter_handle(h, who)) return rc;
    if (!h->finished) return fail(GFFX_E_STATE, "%s: call gffx_hip_genome_finish first", who);
    *arena = h->arena.p, *seq_off = h->seq_off.p, *seq_len = h->seq_len.p, *n_seq = (uint32_t)h->names.size(), *device = h->device;
    return GFFX_OK;
}
}  // namespace gffx
