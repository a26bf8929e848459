// effect.hip -- the transcripts and the pair pass of `gffx effect` (C-ABI gffx_hip_effect_*).  The host has resolved
// the names: it hands over numeric member rows (transcript, sequence number, start - 1, end, kind) and per transcript its strand,
// its phase and whether it is dropped already, then chunks of allele rows (sequence number, x, REF | ALT << 8).
// device/effect_core.hpp has the rules.
//
// BUILD (once, at _create):
//   k_effect_keys         (transcript * 2 + kind, start, input order) per row; the device radix sort (radix_sort.hpp) orders them
//   k_effect_rows         per sorted row its start, end, length and sequence number
//   scan64                the rows' lengths: pre
//   k_effect_transcripts  one thread per transcript: its rows by three searches over the sorted keys, then one walk over them
//                         (effect::build_transcript): pmax, cmin, cmax, L, the span, and whether it can be kept -- every member
//                         on one sequence the genome has, inside it
//   the spans of the kept transcripts go to the host once (16 bytes each) and into a PRIVATE engine index
//   (gffx_hip_index_create: seqid = sequence number, root_fid = transcript number).  The engine's interval index is what
//   answers "which spans contain x"; nothing of it is written again here.
// RUN (per chunk of alleles, through one of two slots):
//   k_effect_alleles      per allele the one-base region [x - 1, x) as SoA columns for the engine, ref_match from the genome,
//                         and the refusal of a sequence number the genome does not have
//   the slot's engine batch, direct strategy (k_join_count / k_join_emit): the pair CSR in allele order, offsets and
//                         root_fids; gffx_hip_batch_wait grows the pair buffer and replays the emit when a chunk has more pairs
//   k_effect_pairs        one thread per pair in CSR order: its allele by a search over the offsets (between the block's first
//                         and last allele), its place in the allele's segment = the number of smaller transcript numbers
//                         there (a segment is short; the engine lists it by start), then effect::classify -- the D search
//                         and the E search side by side, the three codon bases as independent loads -- and the 32-byte
//                         record as two 16-byte stores.  Every record has one writer: no atomics.
// RUN WITH --indels (_run_any_start): a chunk's rows are (sequence number, x0, d, m, 64-bit arena offset) and come
// with a byte arena that holds R' then A' of every row; the arena goes through the slot's pinned staging.
//   k_effect_alleles_any  per allele the footprint's region [lo - 1, hi), ref_match over R', and the refusals: a bad sequence
//                         number, x0 = 0, d = m = 0, d or m beyond 65 535, an insertion in front of base 1, bytes that leave
//                         the arena
//   k_effect_pairs_any    k_effect_pairs with the wider row: effect::classify for d == m == 1 (the same records), else
//                         effect::classify_any
// The class counts of --summary are summed by the host from the records it formats anyway.
// The records, the offsets and ref_match of a chunk come back through the slot's pinned buffers (_run_start / _run_wait), so the
// host formats chunk k while chunk k + 1 is classified.
#include <cstring>
#include <memory>

#include "effect_core.hpp"
#include "handle_status.hpp"
#include "radix_sort.hpp"
#include "scan64.hpp"

using namespace gffx;

namespace gffx {
int genome_view(const gffx_hip_genome *h, const char *who, const uint8_t **arena, const u64 **seq_off, const uint32_t **seq_len, uint32_t *n_seq, int *device);
}

namespace {

constexpr int kPairThreads = 256;
constexpr uint32_t kNoSeq = 0xFFFFFFFFu;  // an allele on a sequence the genome lacks: no pair, ref_match 0
enum : uint32_t { kErrTranscript = 1u, kErrSort = 2u | 4u, kErrEmptyRow = 8u, kErrEmptyTranscript = 16u, kErrKind = 32u, kErrAllele = 64u, kErrArena = 128u };
constexpr uint32_t kMaxAlleleBytes = 65535;

struct Span {  // what the host reads back per transcript
    uint32_t seq, lo0, hi, dropped;
};

__global__ __launch_bounds__(256) void k_effect_keys(const uint32_t *rows, u64 n, u64 n_tr, uint32_t *keys, uint32_t *err) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *r = rows + 5 * i;
    if (r[0] >= n_tr) atomicOr(err, kErrTranscript);
    if (r[2] >= r[3]) atomicOr(err, kErrEmptyRow);
    if (r[4] > 1u) atomicOr(err, kErrKind);
    keys[3 * i] = 2u * r[0] + (r[4] & 1u), keys[3 * i + 1] = r[2], keys[3 * i + 2] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_effect_rows(const uint32_t *rows, const uint32_t *keys, u64 n, u64 n_tr, uint32_t *start0, uint32_t *end, uint32_t *len,
                                                     uint32_t *row_seq) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t idx = keys[3 * j + 2];
    if ((keys[3 * j] >> 1) >= n_tr || idx >= n) {  // (a refused row, or keys of a sort that failed: the error word says which)
        start0[j] = 0, end[j] = 0, len[j] = 0, row_seq[j] = kNoSeq;
        return;
    }
    const uint32_t *r = rows + 5ull * idx;
    start0[j] = r[2], end[j] = r[3], len[j] = r[3] - r[2], row_seq[j] = r[1];
}

// the first sorted row whose key word 0 is >= want
__device__ inline uint32_t first_key_ge(const uint32_t *keys, uint32_t n, uint32_t want) {
    uint32_t lo = 0, len = n;
    while (len) {
        const uint32_t half = len >> 1;
        if (keys[3ull * (lo + half)] < want) lo += half + 1, len -= half + 1;
        else len = half;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_effect_transcripts(const uint32_t *keys, uint32_t n, uint32_t n_tr, const uint32_t *start0, const uint32_t *end,
                                                            const uint32_t *row_seq, const u64 *pre, uint32_t *pmax, const uint8_t *flags, const u64 *seq_off,
                                                            const uint32_t *seq_len, uint32_t n_seq, effect::Transcript *tr, Span *span, uint32_t *err) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tr) return;
    const uint32_t f0 = first_key_ge(keys, n, 2u * t), f1 = first_key_ge(keys, n, 2u * t + 1u), f2 = first_key_ge(keys, n, 2u * t + 2u);
    effect::Transcript o{};
    Span s{kNoSeq, 0u, 0u, 1u};
    if (f2 <= f0) {
        atomicOr(err, kErrEmptyTranscript);
    } else {
        uint32_t lo0, hi;
        const bool ok = effect::build_transcript(start0, end, row_seq, pre, pmax, f0, f1, f2, seq_len, n_seq, &o, &lo0, &hi);
        const uint8_t fl = flags[t];
        const bool keep = ok && !(fl & effect::kFlagDropped);
        o.flags = fl | (o.flags & effect::kFlagOverlap);
        o.base = keep ? seq_off[o.seq] : 0ull;
        s = Span{o.seq, lo0, hi, keep ? 0u : 1u};
    }
    tr[t] = o;
    span[t] = s;
}

// regions for the engine, ref_match, the refusal of a bad row
__global__ __launch_bounds__(256) void k_effect_alleles(const uint32_t *alleles, u64 n, const uint8_t *arena, const u64 *seq_off, const uint32_t *seq_len, uint32_t n_seq,
                                                        uint32_t *q_chr, uint32_t *q_start, uint32_t *q_end, uint8_t *ref_match, uint32_t *err) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t sq = alleles[3 * i], x = alleles[3 * i + 1], ra = alleles[3 * i + 2];
    const bool bad = (sq >= n_seq && sq != kNoSeq) || x == 0;
    if (bad) atomicOr(err, kErrAllele);
    const bool served = !bad && sq < n_seq && x <= seq_len[sq < n_seq ? sq : 0];
    q_chr[i] = served ? sq : n_seq;  // (seqid n_seq of the private index has no span)
    q_start[i] = served ? x - 1 : 0u;
    q_end[i] = served ? x : 1u;
    ref_match[i] = served ? effect::ref_match((uint8_t)ra, arena[seq_off[sq] + (x - 1)]) : 0;
}

// --indels: regions for the engine from the footprint, ref_match over R', the refusal of a bad row.  Rows of 6 words: sequence
// number, x0, d, m, the offset of R' (d bytes) then A' (m bytes) in bytes[0, n_bytes)
__global__ __launch_bounds__(256) void k_effect_alleles_any(const uint32_t *alleles, u64 n, const uint8_t *bytes, u64 n_bytes, const uint8_t *arena, const u64 *seq_off,
                                                            const uint32_t *seq_len, uint32_t n_seq, uint32_t *q_chr, uint32_t *q_start, uint32_t *q_end, uint8_t *ref_match,
                                                            uint32_t *err) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *row = alleles + 6 * i;
    const uint32_t sq = row[0], x0 = row[1], d = row[2], m = row[3];
    const u64 off = (u64)row[4] | (u64)row[5] << 32;
    const bool bad = (sq >= n_seq && sq != kNoSeq) || x0 == 0 || (d == 0 && (m == 0 || x0 == 1)) || d > kMaxAlleleBytes || m > kMaxAlleleBytes;
    const bool outside = off > n_bytes || (u64)d + m > n_bytes - off;  // (its bytes are not read then)
    if (bad) atomicOr(err, kErrAllele);
    if (outside) atomicOr(err, kErrArena);
    const u64 lo = d ? (u64)x0 : (u64)x0 - 1, hi = d ? (u64)x0 + d - 1 : (u64)x0;  // the footprint, 1-based and closed
    const bool served = !bad && !outside && sq < n_seq && hi <= seq_len[sq < n_seq ? sq : 0];
    q_chr[i] = served ? sq : n_seq;
    q_start[i] = served ? (uint32_t)(lo - 1) : 0u;
    q_end[i] = served ? (uint32_t)hi : 1u;
    ref_match[i] = served ? effect::ref_match_run(bytes + off, d, arena + seq_off[sq] + (x0 - 1)) : 0;
}

struct PairArgs {
    const u64 *offsets;    // n_alleles + 1
    const uint32_t *fids;  // pairs: transcript numbers, an allele's segment in the engine's order
    u64 n_alleles, n_pairs;
    const uint32_t *alleles;
    const uint8_t *ref_match;
    const effect::Transcript *tr;
    effect::Rows rows;
    const uint8_t *arena;
    uint4 *out;  // 2 per pair
};

__global__ __launch_bounds__(kPairThreads) void k_effect_pairs(const PairArgs a) {
    __shared__ u64 s_range[2];
    const u64 o0 = (u64)blockIdx.x * kPairThreads;
    if (threadIdx.x == 0) {
        const u64 o_last = (o0 + kPairThreads < a.n_pairs ? o0 + kPairThreads : a.n_pairs) - 1;
        s_range[0] = seq::last_le(a.offsets, a.n_alleles + 1, o0);
        s_range[1] = seq::last_le(a.offsets, a.n_alleles + 1, o_last);
    }
    __syncthreads();
    const u64 o = o0 + threadIdx.x;
    if (o >= a.n_pairs) return;
    // (with alleles of no pair in between, the LAST allele whose segment begins at or before o owns it)
    const u64 i = s_range[0] + seq::last_le(a.offsets + s_range[0], s_range[1] - s_range[0] + 1, o);
    const u64 seg0 = a.offsets[i], seg1 = a.offsets[i + 1];
    const uint32_t t = a.fids[o];
    const uint32_t x = a.alleles[3 * i + 1], ra = a.alleles[3 * i + 2];
    const uint8_t rm = a.ref_match[i];
    const effect::Transcript tr = a.tr[t];
    uint32_t rank = 0;  // the transcripts of an allele by number: a segment holds every transcript once
    for (u64 j = seg0; j < seg1; ++j) rank += a.fids[j] < t ? 1u : 0u;
    effect::Record r = effect::classify(a.rows, tr, a.arena, x, (uint8_t)(ra >> 8));
    r.transcript = t;
    r.ref_match = rm;
    uint4 w[2];
    __builtin_memcpy(w, &r, 32);
    a.out[2 * (seg0 + rank)] = w[0];
    a.out[2 * (seg0 + rank) + 1] = w[1];
}

struct PairAnyArgs {
    PairArgs a;            // alleles: the rows of 6 words
    const uint8_t *bytes;  // the chunk's arena
};

// one thread per pair, as k_effect_pairs: the same CSR and rank logic, the wider row
__global__ __launch_bounds__(kPairThreads) void k_effect_pairs_any(const PairAnyArgs args) {
    const PairArgs &a = args.a;
    __shared__ u64 s_range[2];
    const u64 o0 = (u64)blockIdx.x * kPairThreads;
    if (threadIdx.x == 0) {
        const u64 o_last = (o0 + kPairThreads < a.n_pairs ? o0 + kPairThreads : a.n_pairs) - 1;
        s_range[0] = seq::last_le(a.offsets, a.n_alleles + 1, o0);
        s_range[1] = seq::last_le(a.offsets, a.n_alleles + 1, o_last);
    }
    __syncthreads();
    const u64 o = o0 + threadIdx.x;
    if (o >= a.n_pairs) return;
    const u64 i = s_range[0] + seq::last_le(a.offsets + s_range[0], s_range[1] - s_range[0] + 1, o);
    const u64 seg0 = a.offsets[i], seg1 = a.offsets[i + 1];
    const uint32_t t = a.fids[o];
    const uint32_t *row = a.alleles + 6 * i;
    const uint32_t x0 = row[1], d = row[2], m = row[3];
    const uint8_t *ins = args.bytes + ((u64)row[4] | (u64)row[5] << 32) + d;  // A' (k_effect_alleles_any has checked the bounds)
    const uint8_t rm = a.ref_match[i];
    const effect::Transcript tr = a.tr[t];
    uint32_t rank = 0;
    for (u64 j = seg0; j < seg1; ++j) rank += a.fids[j] < t ? 1u : 0u;
    effect::Record r = d == 1 && m == 1 ? effect::classify(a.rows, tr, a.arena, x0, ins[0]) : effect::classify_any(a.rows, tr, a.arena, x0, d, m, ins);
    r.transcript = t;
    r.ref_match = rm;
    uint4 w[2];
    __builtin_memcpy(w, &r, 32);
    a.out[2 * (seg0 + rank)] = w[0];
    a.out[2 * (seg0 + rank) + 1] = w[1];
}

}  // namespace

struct gffx_hip_effect : HandleStatus {
    static constexpr const char *kName = "the effect handle", *kNoun = "effect object";
    const uint8_t *arena = nullptr;
    const u64 *seq_off = nullptr;
    const uint32_t *seq_len = nullptr;
    uint32_t n_seq = 0;
    u64 n_rows = 0, n_tr = 0, n_kept = 0, max_alleles = 0, grows = 0, arena_grows = 0;
    hipStream_t stream[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr}, slot_ev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // per slot: classify begins, ends, the copies are through
    DevArr<uint32_t> rows, keys_a, keys_b, work, err, len, start0, end, row_seq, pmax;
    DevArr<u64> pre, tile_sum;
    DevArr<uint8_t> flags;
    DevArr<effect::Transcript> tr;
    DevArr<Span> span;
    std::vector<Span> h_span;
    gffx_hip_index *index = nullptr;  // private: the spans of the kept transcripts
    struct Slot {
        gffx_hip_batch *batch = nullptr;
        DevArr<uint32_t> alleles, q_chr, q_start, q_end;
        DevArr<uint8_t> ref_match;
        DevArr<u64> zero_off;  // the offsets of a chunk when no transcript is kept
        DevArr<uint4> records;
        DevArr<uint8_t> bytes;         // --indels: the chunk's arena
        uint8_t *h_bytes = nullptr;    // its pinned staging; grows like the record buffer
        u64 h_bytes_cap = 0;
        uint8_t *pinned = nullptr;  // offsets, then ref_match, then the records
        u64 pinned_cap = 0, n = 0, pairs = 0;
        uint32_t *h_err = nullptr;  // pinned
        bool busy = false;
    } slot[2];
    double build_ms = 0, pairs_ms = 0, classify_ms = 0;
    ~gffx_hip_effect() {
        for (int k = 0; k < 2; ++k) {
            if (stream[k]) (void)hipStreamSynchronize(stream[k]);
            if (slot[k].batch) gffx_hip_batch_destroy(slot[k].batch);
            if (slot[k].pinned) (void)hipHostFree(slot[k].pinned);
            if (slot[k].h_bytes) (void)hipHostFree(slot[k].h_bytes);
            if (slot[k].h_err) (void)hipHostFree(slot[k].h_err);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            for (int j = 0; j < 3; ++j)
                if (slot_ev[k][j]) (void)hipEventDestroy(slot_ev[k][j]);
        }
        if (index) gffx_hip_index_destroy(index);
        for (int k = 0; k < 2; ++k)
            if (stream[k]) (void)hipStreamDestroy(stream[k]);
    }
};

namespace {

int build(gffx_hip_effect *h, const uint32_t *rows, const uint8_t *flags) {
    const u64 n = h->n_rows, T = h->n_tr;
    hipStream_t s = h->stream[0];
    GFFX_HIP_TRY(h->rows.ensure(5 * std::max<u64>(n, 1)));
    GFFX_HIP_TRY(h->keys_a.ensure(3 * std::max<u64>(n, 1)));
    GFFX_HIP_TRY(h->keys_b.ensure(3 * std::max<u64>(n, 1)));
    for (DevArr<uint32_t> *a : {&h->len, &h->start0, &h->end, &h->row_seq, &h->pmax}) GFFX_HIP_TRY(a->ensure(n + 1));
    GFFX_HIP_TRY(h->pre.ensure(n + 2));
    GFFX_HIP_TRY(h->flags.ensure(T + 1));
    GFFX_HIP_TRY(h->tr.ensure(T + 1));
    GFFX_HIP_TRY(h->span.ensure(T + 1));
    GFFX_HIP_TRY(h->err.ensure(1));
    GFFX_HIP_TRY(h->tile_sum.ensure(scan64_tiles(n)));
    SortPlan sp{};
    for (int b = 0; b < 4; ++b) sp.word[sp.n_passes] = 1, sp.shift[sp.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < 4 && (b == 0 || ((2 * T - 1) >> (8 * b))); ++b) sp.word[sp.n_passes] = 0, sp.shift[sp.n_passes++] = (uint8_t)(8 * b);
    GFFX_HIP_TRY(h->work.ensure(DeviceSort::work_words(n, sp.n_passes)));
    if (n) GFFX_HIP_TRY(hipMemcpyAsync(h->rows.p, rows, 20 * n, hipMemcpyHostToDevice, s));
    if (T) GFFX_HIP_TRY(hipMemcpyAsync(h->flags.p, flags, T, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    GFFX_HIP_TRY(hipMemsetAsync(h->err.p, 0, 4, s));
    const uint32_t nb = (uint32_t)((n + 255) / 256), tb = (uint32_t)((T + 255) / 256);
    uint32_t *sorted = h->keys_a.p;
    if (n) {
        hipLaunchKernelGGL(k_effect_keys, dim3(nb), dim3(256), 0, s, h->rows.p, n, T, h->keys_a.p, h->err.p);
        if (int rc = DeviceSort::run<3>(s, h->keys_a.p, h->keys_b.p, n, sp, (uint32_t)std::min<u64>(2 * T, 0xFFFFFFFFull), h->work.p, h->err.p, &sorted)) return rc;
        hipLaunchKernelGGL(k_effect_rows, dim3(nb), dim3(256), 0, s, h->rows.p, sorted, n, T, h->start0.p, h->end.p, h->len.p, h->row_seq.p);
    }
    launch_scan64(s, h->len.p, n, h->tile_sum.p, h->pre.p);
    if (T)
        hipLaunchKernelGGL(k_effect_transcripts, dim3(tb), dim3(256), 0, s, sorted, (uint32_t)n, (uint32_t)T, h->start0.p, h->end.p, h->row_seq.p, h->pre.p, h->pmax.p,
                           h->flags.p, h->seq_off, h->seq_len, h->n_seq, h->tr.p, h->span.p, h->err.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    uint32_t err = 0;
    h->h_span.resize(T);
    GFFX_HIP_TRY(hipMemcpyAsync(&err, h->err.p, 4, hipMemcpyDeviceToHost, s));
    if (T) GFFX_HIP_TRY(hipMemcpyAsync(h->h_span.data(), h->span.p, T * sizeof(Span), hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    float t = 0;
    if (hipEventElapsedTime(&t, h->ev[0], h->ev[1]) == hipSuccess) h->build_ms = t;
    if (err & kErrTranscript) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: a row names a transcript >= n_transcripts");
    if (err & kErrEmptyRow) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: a row with start >= end");
    if (err & kErrKind) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: a row of a kind other than 0 (CDS) and 1 (exon)");
    if (err & kErrSort) return fail(GFFX_E_HIP, "gffx_hip_effect_create: the device sort failed (error word %u)", err);
    if (err & kErrEmptyTranscript) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: a transcript without a row");
    // the private index over the spans of the kept transcripts, grouped by sequence (a counting sort; 16 bytes per transcript)
    std::vector<uint32_t> off((size_t)h->n_seq + 2, 0);
    for (const Span &sp1 : h->h_span)
        if (!sp1.dropped) ++off[sp1.seq + 1], ++h->n_kept;
    for (size_t c = 0; c + 1 < off.size(); ++c) off[c + 1] += off[c];
    if (h->n_kept) {
        std::vector<uint32_t> at(off.begin(), off.end() - 1), st(h->n_kept), en(h->n_kept), fid(h->n_kept);
        for (u64 k = 0; k < T; ++k) {
            const Span &sp1 = h->h_span[k];
            if (sp1.dropped) continue;
            const uint32_t w = at[sp1.seq]++;
            st[w] = sp1.lo0, en[w] = sp1.hi, fid[w] = (uint32_t)k;
        }
        if (int rc = gffx_hip_index_create(h->n_seq + 1, off.data(), st.data(), en.data(), fid.data(), h->device, &h->index)) return rc;
        for (gffx_hip_effect::Slot &sl : h->slot) {
            if (int rc = gffx_hip_batch_create(h->index, std::max<u64>(h->max_alleles, 1), &sl.batch)) return rc;
            if (int rc = gffx_hip_batch_set_profiling(sl.batch, 1)) return rc;
        }
    }
    return GFFX_OK;
}

}  // namespace

extern "C" uint32_t gffx_hip_effect_record_bytes(void) { return (uint32_t)sizeof(effect::Record); }

extern "C" int gffx_hip_effect_create(const gffx_hip_genome *genome, uint64_t n_rows, const uint32_t *rows, uint64_t n_transcripts, const uint8_t *tr_flags,
                                      uint64_t max_alleles, gffx_hip_effect **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: out is NULL");
    *out = nullptr;
    std::unique_ptr<gffx_hip_effect> h(new (std::nothrow) gffx_hip_effect);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_effect_create: out of host memory");
    if (int rc = genome_view(genome, "gffx_hip_effect_create", &h->arena, &h->seq_off, &h->seq_len, &h->n_seq, &h->device)) return rc;
    if ((n_rows && !rows) || (n_transcripts && !tr_flags)) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: rows or tr_flags is NULL");
    if (n_rows >= (1ull << 30) || n_transcripts > n_rows)
        return fail(GFFX_E_INVALID, "gffx_hip_effect_create: %llu rows, %llu transcripts (at most 2^30 - 1 rows, no transcript without one)", (u64)n_rows, (u64)n_transcripts);
    if (max_alleles == 0 || max_alleles >= (1ull << 31)) return fail(GFFX_E_INVALID, "gffx_hip_effect_create: max_alleles = %llu (1 .. 2^31 - 1)", (u64)max_alleles);
    for (uint64_t t = 0; t < n_transcripts; ++t)
        if ((tr_flags[t] & ~0xFu) || (tr_flags[t] & effect::kFlagPhase) == effect::kFlagPhase)
            return fail(GFFX_E_INVALID, "gffx_hip_effect_create: tr_flags[%llu] = %u", (u64)t, tr_flags[t]);
    h->n_rows = n_rows, h->n_tr = n_transcripts, h->max_alleles = max_alleles;
    for (int k = 0; k < 2; ++k) {
        GFFX_HIP_TRY(hipStreamCreateWithFlags(&h->stream[k], hipStreamNonBlocking));
        GFFX_HIP_TRY(hipEventCreate(&h->ev[k]));
        for (hipEvent_t &e : h->slot_ev[k]) GFFX_HIP_TRY(hipEventCreate(&e));
        GFFX_HIP_TRY(hipHostMalloc((void **)&h->slot[k].h_err, 16));
    }
    if (int rc = build(h.get(), rows, tr_flags)) return rc;
    *out = h.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_effect_copy_transcripts(const gffx_hip_effect *h, uint8_t *dropped, uint32_t *span) {
    if (int rc = enter_handle(h, "gffx_hip_effect_copy_transcripts")) return rc;
    for (u64 t = 0; t < h->n_tr; ++t) {
        if (dropped) dropped[t] = h->h_span[t].dropped ? 1 : 0;
        if (span) span[2 * t] = h->h_span[t].lo0 + 1, span[2 * t + 1] = h->h_span[t].hi;
    }
    return GFFX_OK;
}

namespace {

// _run_start (any == false: rows of 3 words) and _run_any_start (rows of 6 words and an arena) share everything but the two kernels
int run_start(gffx_hip_effect *h, int k, const uint32_t *alleles, uint64_t n, bool any, const uint8_t *ins_bytes, uint64_t n_bytes, const char *who) {
    if (int rc = enter_handle(h, who)) return rc;
    if (k < 0 || k > 1) return fail(GFFX_E_INVALID, "%s: slot %d (0 or 1)", who, k);
    gffx_hip_effect::Slot &sl = h->slot[k];
    if (sl.busy) return fail(GFFX_E_STATE, "%s: slot %d is in flight: call gffx_hip_effect_run_wait first", who, k);
    if (n > h->max_alleles) return fail(GFFX_E_INVALID, "%s: %llu alleles exceed the object's %llu", who, (u64)n, h->max_alleles);
    if (n && !alleles) return fail(GFFX_E_INVALID, "%s: alleles is NULL", who);
    if (any && n_bytes && !ins_bytes) return fail(GFFX_E_INVALID, "%s: arena is NULL", who);
    hipStream_t s = h->stream[k];
    sl.n = n, sl.pairs = 0;
    const u64 m = std::max<u64>(n, 1);
    const u64 words = any ? 6 : 3;
    GFFX_KEEP_HIP(h, sl.alleles.ensure(words * m));
    if (any && n) {
        // the arena: into the slot's pinned staging, which grows by an eighth more than asked, then to the device
        if (n_bytes > sl.h_bytes_cap) {
            h->arena_grows += sl.h_bytes_cap ? 1 : 0;
            if (sl.h_bytes) (void)hipHostFree(sl.h_bytes);
            sl.h_bytes = nullptr, sl.h_bytes_cap = 0;
            const u64 want = n_bytes + n_bytes / 8;
            if (hipHostMalloc((void **)&sl.h_bytes, want) != hipSuccess) return keep_failure(h, fail(GFFX_E_OOM, "%s: pinned arena of %llu bytes", who, want));
            sl.h_bytes_cap = want;
        }
        GFFX_KEEP_HIP(h, sl.bytes.ensure(std::max<u64>(sl.h_bytes_cap, 1)));
        if (n_bytes) {
            std::memcpy(sl.h_bytes, ins_bytes, n_bytes);
            GFFX_KEEP_HIP(h, hipMemcpyAsync(sl.bytes.p, sl.h_bytes, n_bytes, hipMemcpyHostToDevice, s));
        }
    }
    for (DevArr<uint32_t> *a : {&sl.q_chr, &sl.q_start, &sl.q_end}) GFFX_KEEP_HIP(h, a->ensure(m));
    GFFX_KEEP_HIP(h, sl.ref_match.ensure(m));
    const u64 *d_off = nullptr;
    const uint32_t *d_fids = nullptr;
    if (n) {
        GFFX_KEEP_HIP(h, hipMemcpyAsync(sl.alleles.p, alleles, 4 * words * n, hipMemcpyHostToDevice, s));
        GFFX_KEEP_HIP(h, hipMemsetAsync(h->err.p, 0, 4, s));
        if (any)
            hipLaunchKernelGGL(k_effect_alleles_any, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, sl.alleles.p, n, sl.bytes.p, n_bytes, h->arena, h->seq_off,
                               h->seq_len, h->n_seq, sl.q_chr.p, sl.q_start.p, sl.q_end.p, sl.ref_match.p, h->err.p);
        else
            hipLaunchKernelGGL(k_effect_alleles, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, sl.alleles.p, n, h->arena, h->seq_off, h->seq_len, h->n_seq, sl.q_chr.p,
                               sl.q_start.p, sl.q_end.p, sl.ref_match.p, h->err.p);
        GFFX_KEEP_HIP(h, hipGetLastError());
        GFFX_KEEP_HIP(h, hipMemcpyAsync(sl.h_err, h->err.p, 4, hipMemcpyDeviceToHost, s));
        GFFX_KEEP_HIP(h, hipStreamSynchronize(s));  // (the caller's rows are free from here on; the engine's stream may read the columns)
        if (*sl.h_err & kErrAllele)
            return keep_failure(h, any ? fail(GFFX_E_CHR_RANGE, "%s: an allele row with a sequence number >= %u (and not %u), with x0 = 0, with d = m = 0, with d or m above %u, or an insertion at x0 = 1",
                                              who, h->n_seq, kNoSeq, kMaxAlleleBytes)
                                       : fail(GFFX_E_CHR_RANGE, "%s: an allele row with a sequence number >= %u (and not %u) or with x = 0", who, h->n_seq, kNoSeq));
        if (*sl.h_err & kErrArena) return keep_failure(h, fail(GFFX_E_INVALID, "%s: an allele row whose bytes leave the arena of %llu bytes", who, (u64)n_bytes));
    }
    if (n && sl.batch) {
        // the pair CSR: the engine's direct pass, segments in allele order
        GFFX_KEEP_TRY(h, gffx_hip_batch_reset_profile(sl.batch));
        GFFX_KEEP_TRY(h, gffx_hip_batch_set_regions_device(sl.batch, sl.q_chr.p, sl.q_start.p, sl.q_end.p, n));
        GFFX_KEEP_TRY(h, gffx_hip_batch_run(sl.batch, GFFX_MODE_OVERLAP, 0, GFFX_OUT_FIDS | GFFX_OUT_OFFSETS, GFFX_STRATEGY_DIRECT));
        GFFX_KEEP_TRY(h, gffx_hip_batch_wait(sl.batch));
        sl.pairs = gffx_hip_batch_total_hits(sl.batch);
        d_off = reinterpret_cast<const u64 *>(gffx_hip_batch_device_offsets(sl.batch)), d_fids = gffx_hip_batch_device_fids(sl.batch);
        double a = 0, b = 0;
        uint64_t launches = 0;
        if (gffx_hip_batch_kernel_ms(sl.batch, GFFX_K_JOIN_COUNT, &a, &launches) == GFFX_OK && gffx_hip_batch_kernel_ms(sl.batch, GFFX_K_JOIN_EMIT, &b, &launches) == GFFX_OK)
            h->pairs_ms += a + b;
    } else {
        GFFX_KEEP_HIP(h, sl.zero_off.ensure(n + 1));
        GFFX_KEEP_HIP(h, hipMemsetAsync(sl.zero_off.p, 0, (n + 1) * sizeof(u64), s));
        d_off = sl.zero_off.p;
    }
    const u64 need = 2 * std::max<u64>(sl.pairs, 1);
    if (need > sl.records.cap) {
        h->grows += sl.records.cap ? 1 : 0;
        GFFX_KEEP_HIP(h, sl.records.ensure(need));
    }
    const u64 off_bytes = (n + 1) * sizeof(u64), rm_bytes = (n + 15) & ~15ull, bytes = off_bytes + rm_bytes + 32 * sl.pairs;
    if (bytes > sl.pinned_cap) {
        if (sl.pinned) (void)hipHostFree(sl.pinned);
        sl.pinned = nullptr, sl.pinned_cap = 0;
        const u64 want = bytes + bytes / 8;  // (32 bytes per pair: at 4 Mi alleles of a dozen pairs each 1.7 GB per slot)
        if (hipHostMalloc((void **)&sl.pinned, want) != hipSuccess) return keep_failure(h, fail(GFFX_E_OOM, "%s: pinned buffer of %llu bytes", who, want));
        sl.pinned_cap = want;
    }
    GFFX_KEEP_HIP(h, hipEventRecord(h->slot_ev[k][0], s));
    if (sl.pairs) {
        const PairArgs a{d_off,   d_fids,   n, sl.pairs, sl.alleles.p, sl.ref_match.p, h->tr.p, effect::Rows{h->start0.p, h->end.p, h->pre.p, h->pmax.p},
                         h->arena, sl.records.p};
        if (any) hipLaunchKernelGGL(k_effect_pairs_any, dim3((uint32_t)((sl.pairs + kPairThreads - 1) / kPairThreads)), dim3(kPairThreads), 0, s, PairAnyArgs{a, sl.bytes.p});
        else hipLaunchKernelGGL(k_effect_pairs, dim3((uint32_t)((sl.pairs + kPairThreads - 1) / kPairThreads)), dim3(kPairThreads), 0, s, a);
        GFFX_KEEP_HIP(h, hipGetLastError());
    }
    GFFX_KEEP_HIP(h, hipEventRecord(h->slot_ev[k][1], s));
    GFFX_KEEP_HIP(h, hipMemcpyAsync(sl.pinned, d_off, off_bytes, hipMemcpyDeviceToHost, s));
    if (n) GFFX_KEEP_HIP(h, hipMemcpyAsync(sl.pinned + off_bytes, sl.ref_match.p, n, hipMemcpyDeviceToHost, s));
    if (sl.pairs) GFFX_KEEP_HIP(h, hipMemcpyAsync(sl.pinned + off_bytes + rm_bytes, sl.records.p, 32 * sl.pairs, hipMemcpyDeviceToHost, s));
    GFFX_KEEP_HIP(h, hipEventRecord(h->slot_ev[k][2], s));
    sl.busy = true;
    return GFFX_OK;
}

}  // namespace

extern "C" int gffx_hip_effect_run_start(gffx_hip_effect *h, int k, const uint32_t *alleles, uint64_t n) {
    return run_start(h, k, alleles, n, false, nullptr, 0, "gffx_hip_effect_run_start");
}

extern "C" int gffx_hip_effect_run_any_start(gffx_hip_effect *h, int k, const uint32_t *rows, uint64_t n, const uint8_t *arena, uint64_t arena_bytes) {
    return run_start(h, k, rows, n, true, arena, arena_bytes, "gffx_hip_effect_run_any_start");
}

extern "C" int gffx_hip_effect_run_wait(gffx_hip_effect *h, int k, const uint64_t **offsets, const uint8_t **ref_match, const uint8_t **records, uint64_t *n_pairs) {
    if (int rc = enter_handle(h, "gffx_hip_effect_run_wait")) return rc;
    if (k < 0 || k > 1 || !h->slot[k].busy) return fail(GFFX_E_STATE, "gffx_hip_effect_run_wait: slot %d is not in flight", k);
    gffx_hip_effect::Slot &sl = h->slot[k];
    sl.busy = false;
    GFFX_KEEP_HIP(h, hipEventSynchronize(h->slot_ev[k][2]));
    float t = 0;
    if (hipEventElapsedTime(&t, h->slot_ev[k][0], h->slot_ev[k][1]) == hipSuccess) h->classify_ms += t;
    const u64 off_bytes = (sl.n + 1) * sizeof(u64), rm_bytes = (sl.n + 15) & ~15ull;
    if (offsets) *offsets = reinterpret_cast<const uint64_t *>(sl.pinned);
    if (ref_match) *ref_match = sl.pinned + off_bytes;
    if (records) *records = sl.pinned + off_bytes + rm_bytes;
    if (n_pairs) *n_pairs = sl.pairs;
    return GFFX_OK;
}

extern "C" int gffx_hip_effect_stage_ms(const gffx_hip_effect *h, double *build_ms, double *pairs_ms, double *classify_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_effect_stage_ms: the effect handle is NULL");
    if (build_ms) *build_ms = h->build_ms;
    if (pairs_ms) *pairs_ms = h->pairs_ms;
    if (classify_ms) *classify_ms = h->classify_ms;
    return GFFX_OK;
}

extern "C" int gffx_hip_effect_stats(const gffx_hip_effect *h, uint64_t *kept, uint64_t *grows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_effect_stats: the effect handle is NULL");
    if (kept) *kept = h->n_kept;
    if (grows) *grows = h->grows;
    return GFFX_OK;
}

extern "C" int gffx_hip_effect_arena_grows(const gffx_hip_effect *h, uint64_t *grows) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_effect_arena_grows: the effect handle is NULL");
    if (grows) *grows = h->arena_grows;
    return GFFX_OK;
}

extern "C" void gffx_hip_effect_destroy(gffx_hip_effect *h) {
    if (h) (void)hipSetDevice(h->device);
    delete h;
}
