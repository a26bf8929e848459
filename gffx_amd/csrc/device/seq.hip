// seq.hip -- the plan and the emit of `gffx seq` (C-ABI gffx_hip_seq_*).  The host has resolved the names: it hands over
// numeric rows (record, sequence number, start - 1, end) and per record its strand, its phase and whether it is dropped already
// (mixed seqids or strands).  device/seq_core.hpp has the rules.
//
// PLAN (once, at _create):
//   k_seq_keys      (record, start, input order) per row; the device radix sort (radix_sort.hpp) orders them
//   k_seq_rows      per sorted row its length and where its first base lies in the genome's arena; a member on a sequence the
//                   FASTA lacks or beyond its end marks its record dropped; the first row of every record
//   scan64          the rows' lengths: where a row's bases lie in its record
//   k_seq_records   per record its characters (after --translate) and its wrapped body size
//   scan64          one 64-bit body offset per record, which the host reads back
// EMIT (per slice [at, at + n) of the concatenated bodies):
//   k_seq_emit      tiled over OUTPUT bytes: a block owns kSeqTile bytes of the slice, a thread 16 aligned ones.  The block's
//                   first and last record come from two searches over the body offsets, the thread's record from a search
//                   between them and its segment from one over the record's rows; from there the thread walks forward -- to
//                   the next character, segment (backwards on minus) or record.  A 2 Mb gene and a 30-base exon load the
//                   machine alike.  A byte is a newline or character c of its record: one base (complemented, index mirrored on
//                   minus) or, with --translate, the amino acid of three bases each located on its own.  A run that lies in
//                   one segment is read with one 16-byte load.  The complement table sits in LDS.  Every output byte has one
//                   writer: no atomics; full runs are stored as aligned 16 bytes.
// Slices go through two device buffers and two pinned ones (_emit_start / _emit_wait), so the host writes slice k while
// slice k + 1 is produced.
#include <memory>

#include "handle_status.hpp"
#include "radix_sort.hpp"
#include "scan64.hpp"
#include "seq_core.hpp"

using namespace gffx;

namespace gffx {
int genome_view(const gffx_hip_genome *h, const char *who, const uint8_t **arena, const u64 **seq_off, const uint32_t **seq_len, uint32_t *n_seq, int *device);
}

namespace {

constexpr uint32_t kSeqTile = 4096;  // output bytes per block: 256 threads x 16
constexpr int kSeqThreads = 256;
constexpr u64 kNoRow = ~0ull;
enum : uint32_t { kErrRecord = 1u, kErrSort = 2u | 4u, kErrEmptyRow = 8u, kErrEmptyRecord = 16u };
enum : uint8_t { kFlagMinus = 1, kFlagPhase = 6, kFlagDropped = 8 };

__global__ __launch_bounds__(256) void k_seq_keys(const uint32_t *rows, u64 n, u64 n_records, uint32_t *keys, uint32_t *err) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r = reinterpret_cast<const uint4 *>(rows)[i];
    if (r.x >= n_records) atomicOr(err, kErrRecord);
    if (r.z >= r.w) atomicOr(err, kErrEmptyRow);
    keys[3 * i] = r.x, keys[3 * i + 1] = r.z, keys[3 * i + 2] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_seq_rows(const uint32_t *rows, const uint32_t *keys, u64 n, u64 n_records, const u64 *seq_off, const uint32_t *seq_len, uint32_t n_seq,
                                                  uint32_t *len, u64 *src, u64 *rec_first, uint8_t *dropped) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t rec = keys[3 * j], idx = keys[3 * j + 2];
    if (rec >= n_records || idx >= n) {  // (a refused row, or keys of a sort that failed: the error word says which; nothing is indexed with them)
        len[j] = 0, src[j] = 0;
        return;
    }
    const uint4 r = reinterpret_cast<const uint4 *>(rows)[idx];
    len[j] = r.w - r.z;
    const bool servable = r.y < n_seq && r.w <= seq_len[r.y < n_seq ? r.y : 0];
    src[j] = servable ? seq_off[r.y] + r.z : 0ull;
    if (!servable) dropped[rec] = 1;  // (every writer stores the same value)
    if (j == 0 || keys[3 * (j - 1)] != rec) rec_first[rec] = j;
}

__global__ __launch_bounds__(256) void k_seq_records(u64 n_records, const u64 *rec_first, const u64 *pre, const uint8_t *flags, uint8_t *dropped, int translated,
                                                     u64 W, u64 *chars, u64 *body, uint32_t *err) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    const u64 f0 = rec_first[r], f1 = rec_first[r + 1];
    if (f0 == kNoRow || f1 == kNoRow || f1 <= f0) {
        atomicOr(err, kErrEmptyRecord);
        chars[r] = 0, body[r] = 0;
        return;
    }
    const uint8_t fl = flags[r];
    const bool drop = (fl & kFlagDropped) || dropped[r];
    dropped[r] = drop ? 1 : 0;
    const u64 C = drop ? 0 : seq::characters(pre[f1] - pre[f0], (fl & kFlagPhase) >> 1, translated != 0);
    chars[r] = C;
    body[r] = seq::body_bytes(C, W);
}

struct EmitArgs {
    uint8_t *out;
    u64 at, n;  // the slice
    const u64 *body_off, *chars, *rec_first, *pre, *src;
    const uint8_t *flags, *arena;
    u64 n_records, W;
    int translated;
};

// the walk of one thread through the bases of one record
struct Walker {
    const EmitArgs &a;
    const uint8_t *comp;  // LDS
    u64 f0 = 0, f1 = 0, L = 0, ri = kNoRow, seg_lo = 0, seg_hi = 0, seg_src = 0;
    bool minus = false;
    __device__ Walker(const EmitArgs &a_, const uint8_t *comp_) : a(a_), comp(comp_) {}
    __device__ void enter(u64 r) {
        f0 = a.rec_first[r], f1 = a.rec_first[r + 1];
        L = a.pre[f1] - a.pre[f0];
        minus = a.flags[r] & kFlagMinus;
        ri = kNoRow;
    }
    __device__ void seek(u64 x) {  // the row of base x of the concatenation
        if (ri == kNoRow) {
            ri = seq::locate_row(a.pre, f0, f1, x);
        } else {
            while (x >= seg_hi) {
                ++ri;
                seg_hi = a.pre[ri + 1] - a.pre[f0];
            }
            while (x < seg_lo) {
                --ri;
                seg_lo = a.pre[ri] - a.pre[f0];
            }
        }
        seg_lo = a.pre[ri] - a.pre[f0], seg_hi = a.pre[ri + 1] - a.pre[f0];
        seg_src = a.src[ri];
    }
    __device__ uint8_t base(u64 q) {  // transcription position q < L
        const u64 x = minus ? L - 1 - q : q;
        if (ri == kNoRow || x < seg_lo || x >= seg_hi) seek(x);
        const uint8_t b = a.arena[seg_src + (x - seg_lo)];
        return minus ? comp[b] : b;
    }
};

__global__ __launch_bounds__(kSeqThreads) void k_seq_emit(const EmitArgs a) {
    __shared__ uint8_t s_comp[256];
    __shared__ u64 s_range[2];
    s_comp[threadIdx.x] = seq::complement((uint8_t)threadIdx.x);
    const u64 t0 = (u64)blockIdx.x * kSeqTile;
    if (threadIdx.x == 0) {
        const u64 g_last = a.at + (t0 + kSeqTile < a.n ? t0 + kSeqTile : a.n) - 1;
        s_range[0] = seq::last_le(a.body_off, a.n_records + 1, a.at + t0);
        s_range[1] = seq::last_le(a.body_off, a.n_records + 1, g_last);
    }
    __syncthreads();
    const u64 rel = t0 + 16ull * threadIdx.x;
    if (rel >= a.n) return;
    const uint32_t m = (uint32_t)(a.n - rel < 16 ? a.n - rel : 16);
    const u64 g0 = a.at + rel;
    const u64 W = a.W ? a.W : ~0ull;  // (one line: the column never reaches W)
    u64 r = s_range[0] + seq::last_le(a.body_off + s_range[0], s_range[1] - s_range[0] + 1, g0);
    Walker w(a, s_comp);
    u64 rend = 0, C = 0, c = 0, col = 0;
    uint32_t p = 0;
    auto enter = [&](u64 g) {  // g lies in record r's body
        const u64 b = g - a.body_off[r];
        rend = a.body_off[r + 1];
        C = a.chars[r];
        p = (a.flags[r] & kFlagPhase) >> 1;
        if (a.W == 0) {
            c = b, col = b;
        } else {
            const u64 line = b / (a.W + 1);
            col = b % (a.W + 1);
            c = line * a.W + col;
        }
        w.enter(r);
    };
    enter(g0);
    uint8_t o[16];
    uint32_t k = 0;
    // a run inside one line of one record whose bases lie in one segment: one 16-byte load
    if (!a.translated && m == 16 && g0 + 16 <= rend && col + 16 <= W && c + 16 <= C) {
        const u64 x_lo = w.minus ? w.L - 16 - c : c;
        w.seek(x_lo);
        if (x_lo + 16 <= w.seg_hi) {
            uint8_t v[16];
            __builtin_memcpy(v, a.arena + w.seg_src + (x_lo - w.seg_lo), 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) o[j] = w.minus ? s_comp[v[15 - j]] : v[j];
            k = 16;
        }
    }
    for (; k < 16; ++k) {
        if (k >= m) {
            o[k] = 0;
            continue;
        }
        const u64 g = g0 + k;
        if (g >= rend) {
            do ++r;
            while (a.body_off[r + 1] <= g);  // (records without a body are passed)
            enter(g);
        }
        if (col == W || c == C) {
            o[k] = '\n';
            col = 0;
        } else {
            if (a.translated) {
                const u64 q = p + 3 * c;
                const uint8_t b0 = w.base(q), b1 = w.base(q + 1), b2 = w.base(q + 2);
                o[k] = seq::translate(b0, b1, b2);
            } else {
                o[k] = w.base(c);
            }
            ++c, ++col;
        }
    }
    if (m == 16) {
        uint4 v;
        __builtin_memcpy(&v, o, 16);
        *reinterpret_cast<uint4 *>(a.out + rel) = v;
    } else {
        for (uint32_t j = 0; j < m; ++j) a.out[rel + j] = o[j];
    }
}

}  // namespace

struct gffx_hip_seq : HandleStatus {
    static constexpr const char *kName = "the seq handle", *kNoun = "seq plan";
    const uint8_t *arena = nullptr;
    u64 n_rows = 0, n_records = 0, W = 0, total = 0;
    int translated = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr}, slot_ev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // per slot: emit begins, emit ends, the copy is through
    DevArr<uint32_t> rows, keys_a, keys_b, work, err, len;
    DevArr<u64> src, pre, rec_first, chars, body, body_off, tile_sum;
    DevArr<uint8_t> flags, dropped, out[2];
    uint8_t *pinned[2] = {nullptr, nullptr};
    u64 pinned_cap[2] = {0, 0}, slot_n[2] = {0, 0};
    bool slot_busy[2] = {false, false};
    double plan_ms = 0, emit_ms = 0;
    ~gffx_hip_seq() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (int k = 0; k < 2; ++k) {
            if (pinned[k]) (void)hipHostFree(pinned[k]);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            for (int j = 0; j < 3; ++j)
                if (slot_ev[k][j]) (void)hipEventDestroy(slot_ev[k][j]);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int plan(gffx_hip_seq *h, const uint32_t *rows, const uint8_t *rec_flags, const u64 *seq_off, const uint32_t *seq_len, uint32_t n_seq) {
    const u64 n = h->n_rows, R = h->n_records;
    hipStream_t s = h->stream;
    GFFX_HIP_TRY(h->rows.ensure(4 * std::max<u64>(n, 1)));
    GFFX_HIP_TRY(h->keys_a.ensure(3 * std::max<u64>(n, 1)));
    GFFX_HIP_TRY(h->keys_b.ensure(3 * std::max<u64>(n, 1)));
    GFFX_HIP_TRY(h->len.ensure(n + 1));
    GFFX_HIP_TRY(h->src.ensure(n + 1));
    GFFX_HIP_TRY(h->pre.ensure(n + 2));
    GFFX_HIP_TRY(h->rec_first.ensure(R + 2));
    GFFX_HIP_TRY(h->chars.ensure(R + 1));
    GFFX_HIP_TRY(h->body.ensure(R + 1));
    GFFX_HIP_TRY(h->body_off.ensure(R + 2));
    GFFX_HIP_TRY(h->flags.ensure(R + 1));
    GFFX_HIP_TRY(h->dropped.ensure(R + 1));
    GFFX_HIP_TRY(h->err.ensure(1));
    GFFX_HIP_TRY(h->tile_sum.ensure(std::max(scan64_tiles(n), scan64_tiles(R))));
    SortPlan sp{};
    for (int b = 0; b < 4; ++b) sp.word[sp.n_passes] = 1, sp.shift[sp.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < 4 && (b == 0 || ((R - 1) >> (8 * b))); ++b) sp.word[sp.n_passes] = 0, sp.shift[sp.n_passes++] = (uint8_t)(8 * b);
    GFFX_HIP_TRY(h->work.ensure(DeviceSort::work_words(n, sp.n_passes)));
    if (n) GFFX_HIP_TRY(hipMemcpyAsync(h->rows.p, rows, 16 * n, hipMemcpyHostToDevice, s));
    if (R) GFFX_HIP_TRY(hipMemcpyAsync(h->flags.p, rec_flags, R, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    GFFX_HIP_TRY(hipMemsetAsync(h->err.p, 0, 4, s));
    GFFX_HIP_TRY(hipMemsetAsync(h->dropped.p, 0, R + 1, s));
    GFFX_HIP_TRY(hipMemsetAsync(h->rec_first.p, 0xFF, (R + 2) * sizeof(u64), s));
    const uint32_t nb = (uint32_t)((n + 255) / 256), rb = (uint32_t)((R + 255) / 256);
    uint32_t *sorted = h->keys_a.p;
    if (n) {
        hipLaunchKernelGGL(k_seq_keys, dim3(nb), dim3(256), 0, s, h->rows.p, n, R, h->keys_a.p, h->err.p);
        if (int rc = DeviceSort::run<3>(s, h->keys_a.p, h->keys_b.p, n, sp, (uint32_t)std::min<u64>(R, 0xFFFFFFFFull), h->work.p, h->err.p, &sorted)) return rc;
        hipLaunchKernelGGL(k_seq_rows, dim3(nb), dim3(256), 0, s, h->rows.p, sorted, n, R, seq_off, seq_len, n_seq, h->len.p, h->src.p, h->rec_first.p, h->dropped.p);
    }
    GFFX_HIP_TRY(hipMemcpyAsync(h->rec_first.p + R, &h->n_rows, sizeof(u64), hipMemcpyHostToDevice, s));
    launch_scan64(s, h->len.p, n, h->tile_sum.p, h->pre.p);
    if (R) hipLaunchKernelGGL(k_seq_records, dim3(rb), dim3(256), 0, s, R, h->rec_first.p, h->pre.p, h->flags.p, h->dropped.p, h->translated, h->W, h->chars.p, h->body.p,
                              h->err.p);
    launch_scan64(s, h->body.p, R, h->tile_sum.p, h->body_off.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    uint32_t err = 0;
    GFFX_HIP_TRY(hipMemcpyAsync(&err, h->err.p, 4, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipMemcpyAsync(&h->total, h->body_off.p + R, sizeof(u64), hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    float t = 0;
    if (hipEventElapsedTime(&t, h->ev[0], h->ev[1]) == hipSuccess) h->plan_ms = t;
    if (err & kErrRecord) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: a row names a record >= n_records");
    if (err & kErrEmptyRow) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: a row with start >= end");
    if (err & kErrSort) return fail(GFFX_E_HIP, "gffx_hip_seq_create: the device sort failed (error word %u)", err);
    if (err & kErrEmptyRecord) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: a record without a row");
    return GFFX_OK;
}

}  // namespace

extern "C" uint32_t gffx_hip_seq_tile(void) { return kSeqTile; }

extern "C" int gffx_hip_seq_create(const gffx_hip_genome *genome, uint64_t n_rows, const uint32_t *rows, uint64_t n_records, const uint8_t *rec_flags, int translate,
                                   uint32_t width, gffx_hip_seq **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: out is NULL");
    *out = nullptr;
    const uint8_t *arena = nullptr;
    const u64 *seq_off = nullptr;
    const uint32_t *seq_len = nullptr;
    uint32_t n_seq = 0;
    int device = 0;
    if (int rc = genome_view(genome, "gffx_hip_seq_create", &arena, &seq_off, &seq_len, &n_seq, &device)) return rc;
    if ((n_rows && !rows) || (n_records && !rec_flags)) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: rows or rec_flags is NULL");
    if (n_rows >= (1ull << 30) || n_records > n_rows) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: %llu rows, %llu records (at most 2^30 - 1 rows, no record without one)", (u64)n_rows, (u64)n_records);
    for (uint64_t r = 0; r < n_records; ++r)
        if ((rec_flags[r] & ~0xFu) || (rec_flags[r] & kFlagPhase) == kFlagPhase) return fail(GFFX_E_INVALID, "gffx_hip_seq_create: rec_flags[%llu] = %u", (u64)r, rec_flags[r]);
    std::unique_ptr<gffx_hip_seq> h(new (std::nothrow) gffx_hip_seq);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_seq_create: out of host memory");
    h->device = device, h->arena = arena, h->n_rows = n_rows, h->n_records = n_records, h->W = width, h->translated = translate ? 1 : 0;
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    for (auto &pair : h->slot_ev)
        for (hipEvent_t &e : pair) GFFX_HIP_TRY(hipEventCreate(&e));
    if (int rc = plan(h.get(), rows, rec_flags, seq_off, seq_len, n_seq)) return rc;
    *out = h.release();
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_seq_body_bytes(const gffx_hip_seq *h) { return h ? h->total : 0; }

extern "C" int gffx_hip_seq_copy_offsets(const gffx_hip_seq *h, uint64_t *body_off, uint8_t *dropped) {
    if (int rc = enter_handle(h, "gffx_hip_seq_copy_offsets")) return rc;
    if (body_off) GFFX_HIP_TRY(hipMemcpy(body_off, h->body_off.p, (h->n_records + 1) * sizeof(u64), hipMemcpyDeviceToHost));
    if (dropped && h->n_records) GFFX_HIP_TRY(hipMemcpy(dropped, h->dropped.p, h->n_records, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

extern "C" int gffx_hip_seq_emit_start(gffx_hip_seq *h, int slot, uint64_t at, uint64_t n) {
    if (int rc = enter_handle(h, "gffx_hip_seq_emit_start")) return rc;
    if (slot < 0 || slot > 1) return fail(GFFX_E_INVALID, "gffx_hip_seq_emit_start: slot %d (0 or 1)", slot);
    if (h->slot_busy[slot]) return fail(GFFX_E_STATE, "gffx_hip_seq_emit_start: slot %d is in flight: call gffx_hip_seq_emit_wait first", slot);
    if (n == 0 || at > h->total || n > h->total - at) return fail(GFFX_E_INVALID, "gffx_hip_seq_emit_start: [%llu, +%llu) is empty or beyond the %llu body bytes", (u64)at, (u64)n, h->total);
    if (n > 0xFFFFFFFFull * (u64)kSeqTile / 2) return fail(GFFX_E_INVALID, "gffx_hip_seq_emit_start: a slice of %llu bytes", (u64)n);
    if (n > h->pinned_cap[slot]) {
        if (h->pinned[slot]) (void)hipHostFree(h->pinned[slot]);
        h->pinned[slot] = nullptr, h->pinned_cap[slot] = 0;
        if (hipHostMalloc((void **)&h->pinned[slot], n) != hipSuccess) return keep_failure(h, fail(GFFX_E_OOM, "gffx_hip_seq_emit_start: pinned buffer of %llu bytes", (u64)n));
        h->pinned_cap[slot] = n;
    }
    GFFX_KEEP_HIP(h, h->out[slot].ensure(n + 16));
    hipStream_t s = h->stream;
    const EmitArgs a{h->out[slot].p, at, n, h->body_off.p, h->chars.p, h->rec_first.p, h->pre.p, h->src.p, h->flags.p, h->arena, h->n_records, h->W, h->translated};
    GFFX_KEEP_HIP(h, hipEventRecord(h->slot_ev[slot][0], s));
    hipLaunchKernelGGL(k_seq_emit, dim3((uint32_t)((n + kSeqTile - 1) / kSeqTile)), dim3(kSeqThreads), 0, s, a);
    GFFX_KEEP_HIP(h, hipGetLastError());
    GFFX_KEEP_HIP(h, hipEventRecord(h->slot_ev[slot][1], s));
    GFFX_KEEP_HIP(h, hipMemcpyAsync(h->pinned[slot], h->out[slot].p, n, hipMemcpyDeviceToHost, s));
    GFFX_KEEP_HIP(h, hipEventRecord(h->slot_ev[slot][2], s));
    h->slot_busy[slot] = true;
    h->slot_n[slot] = n;
    return GFFX_OK;
}

extern "C" int gffx_hip_seq_emit_wait(gffx_hip_seq *h, int slot, const uint8_t **bytes) {
    if (int rc = enter_handle(h, "gffx_hip_seq_emit_wait")) return rc;
    if (slot < 0 || slot > 1 || !h->slot_busy[slot]) return fail(GFFX_E_STATE, "gffx_hip_seq_emit_wait: slot %d is not in flight", slot);
    h->slot_busy[slot] = false;
    // (the stream runs the slices in order: when this one's copy is through, the other slot may still be running)
    GFFX_KEEP_HIP(h, hipEventSynchronize(h->slot_ev[slot][2]));
    float t = 0;
    if (hipEventElapsedTime(&t, h->slot_ev[slot][0], h->slot_ev[slot][1]) == hipSuccess) h->emit_ms += t;
    if (bytes) *bytes = h->pinned[slot];
    return GFFX_OK;
}

extern "C" int gffx_hip_seq_stage_ms(const gffx_hip_seq *h, double *plan_ms, double *emit_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_seq_stage_ms: the seq handle is NULL");
    if (plan_ms) *plan_ms = h->plan_ms;
    if (emit_ms) *emit_ms = h->emit_ms;
    return GFFX_OK;
}

extern "C" void gffx_hip_seq_destroy(gffx_hip_seq *h) { delete h; }
