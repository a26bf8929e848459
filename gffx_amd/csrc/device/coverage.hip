// coverage.hip -- `gffx coverage` (BED source): covered bases of feature segments under the union of the regions
// of their seqid (reference: commands/coverage.rs:92-124 merge_intervals / union_len, :339-364 the two-pointer walk).
//
// The reference merges, per root, the regions that hit the root and walks every line of the root's block against
// that list.  A region that overlaps a segment lying inside the root's interval necessarily hits the root, so for
// such segments the per-root list can be replaced by ONE list per seqid: the union U of all regions (sorted,
// touching spans merged like merge_intervals).  With P[k] = total length of U[0..k) the covered bases below x are
//      F(x) = P[k-1] + min(x, U[k-1].end) - U[k-1].start,   k = #{U.start < x}   (0 if k == 0)
// and a segment [a, b) holds F(b) - F(a) covered bases: two searches per segment, each narrowed to one bin of a
// directory over U.start (as in join_b.hip).  Segments that stick out of their root's interval are handled on
// the host (exactly, they are rare).  One thread per segment; 12 B in, 4 B out.  Roofline bound: HBM.
// U is built either on the host inside the one-shot gffx_hip_segments_covered (one thread, std::sort per seqid), or on the device,
// chunk by chunk, by the union builder in the second half of this file (gffx_hip_union_*: what `gffx coverage` uses).
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "gffx_device.hpp"
#include "radix_sort.hpp"
#include "regions_store.hpp"
#include "union_private.hpp"  // struct gffx_hip_union

namespace gffx {

struct UnionView {
    const unsigned long long *u_off;  // n_seq + 1: spans of seqid c are [u_off[c], u_off[c+1])
    const uint32_t *us, *ue;          // sorted, disjoint, non-touching
    const unsigned long long *pb;     // covered bases of the seqid's spans before this one
    const uint32_t *dir;              // directory over us (see join_b.hip)
    const unsigned long long *d_off;  // n_seq + 1
    const uint2 *d_meta;              // per seqid {shift, nb}
    uint32_t n_seq;
};

__device__ __forceinline__ unsigned long long covered_below(const UnionView &U, uint32_t seq, unsigned long long lo,
                                                            unsigned long long hi, uint32_t x) {
    unsigned long long a = lo, b = hi;
    const uint2 m = U.d_meta[seq];
    const uint32_t bin = x >> m.x;
    if (bin >= m.y) {
        a = b = hi;  // beyond the largest start: every span starts below x
    } else {
        const uint32_t *d = U.dir + U.d_off[seq] + bin;
        a = d[0];
        b = d[1];
    }
    while (a < b) {  // first span with start >= x
        const unsigned long long mid = (a + b) >> 1;
        if (U.us[mid] < x)
            a = mid + 1;
        else
            b = mid;
    }
    if (a == lo) return 0ull;
    const unsigned long long k = a - 1;
    return U.pb[k] + (min(x, U.ue[k]) - U.us[k]);
}

__global__ __launch_bounds__(256) void k_segments_covered(UnionView U, unsigned long long n_seg, const uint32_t *seg_seq,
                                                          const uint32_t *seg_start, const uint32_t *seg_end,
                                                          uint32_t *covered) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_seg) return;
    const uint32_t seq = seg_seq[i], a = seg_start[i], b = seg_end[i];
    uint32_t c = 0;
    if (seq < U.n_seq && a < b) {
        const unsigned long long lo = U.u_off[seq], hi = U.u_off[seq + 1];
        if (hi > lo) c = (uint32_t)(covered_below(U, seq, lo, hi, b) - covered_below(U, seq, lo, hi, a));
    }
    covered[i] = c;
}

}  // namespace gffx

using namespace gffx;

extern "C" int gffx_hip_segments_covered(int device, uint64_t n_seg, const uint32_t *seg_seq, const uint32_t *seg_start,
                                         const uint32_t *seg_end, const uint32_t *regions, uint64_t nq, uint32_t n_seq,
                                         uint32_t *covered_out) {
    if (n_seg && (!seg_seq || !seg_start || !seg_end || !covered_out))
        return fail(GFFX_E_INVALID, "gffx_hip_segments_covered: NULL segment array");
    if (nq && !regions) return fail(GFFX_E_INVALID, "gffx_hip_segments_covered: regions is NULL");
    for (uint64_t i = 0; i < nq; i++)
        if (regions[3 * i] >= n_seq)
            return fail(GFFX_E_CHR_RANGE, "gffx_hip_segments_covered: region %llu has chr %u >= %u", (unsigned long long)i,
                        regions[3 * i], n_seq);
    for (uint64_t i = 0; i < n_seg; i++)
        if (seg_seq[i] >= n_seq)
            return fail(GFFX_E_CHR_RANGE, "gffx_hip_segments_covered: segment %llu has chr %u >= %u", (unsigned long long)i,
                        seg_seq[i], n_seq);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    if (ndev <= 0) return fail(GFFX_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFFX_E_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
    if (n_seg == 0) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(device));
    // per seqid: sort by start, merge while s <= current end (coverage.rs:92-109), prefix of the lengths, directory
    std::vector<unsigned long long> q_off(n_seq + 1, 0);
    for (uint64_t i = 0; i < nq; i++) q_off[regions[3 * i] + 1]++;
    for (uint32_t c = 0; c < n_seq; c++) q_off[c + 1] += q_off[c];
    std::vector<uint64_t> key(nq);
    {
        std::vector<unsigned long long> cur(q_off.begin(), q_off.end() - 1);
        for (uint64_t i = 0; i < nq; i++) key[cur[regions[3 * i]]++] = ((uint64_t)regions[3 * i + 1] << 32) | regions[3 * i + 2];
    }
    std::vector<unsigned long long> u_off(n_seq + 1, 0), pb, d_off(n_seq + 1, 0);
    std::vector<uint32_t> us, ue, dir;
    std::vector<uint2> d_meta(n_seq, make_uint2(0, 0));
    for (uint32_t c = 0; c < n_seq; c++) {
        const uint64_t lo = q_off[c], hi = q_off[c + 1];
        const size_t u0 = us.size();
        if (hi > lo) {
            std::sort(key.begin() + lo, key.begin() + hi);
            uint32_t cs = (uint32_t)(key[lo] >> 32), ce = (uint32_t)key[lo];
            if (ce < cs) ce = cs;  // (rows with s >= e never get here: coverage.rs:251)
            unsigned long long acc = 0;
            for (uint64_t i = lo + 1; i < hi; i++) {
                const uint32_t s = (uint32_t)(key[i] >> 32), e = (uint32_t)key[i];
                if (s <= ce) {
                    ce = std::max(ce, e);
                } else {
                    us.push_back(cs);
                    ue.push_back(ce);
                    pb.push_back(acc);
                    acc += ce - cs;
                    cs = s;
                    ce = e;
                }
            }
            us.push_back(cs);
            ue.push_back(ce);
            pb.push_back(acc);
        }
        u_off[c + 1] = us.size();
        d_off[c + 1] = d_off[c];
        const size_t n_u = us.size() - u0;
        if (n_u) {
            const uint32_t vmax = us.back();
            const uint64_t budget = std::max<uint64_t>(2 * n_u, 16);
            uint32_t shift = 0;
            while ((((uint64_t)vmax >> shift) + 1) > budget) shift++;
            const uint32_t nb = (vmax >> shift) + 1;
            d_meta[c] = make_uint2(shift, nb);
            size_t p = u0;
            for (uint32_t b = 0; b < nb; b++) {
                const uint64_t edge = (uint64_t)b << shift;
                while (p < us.size() && us[p] < edge) p++;
                dir.push_back((uint32_t)p);
            }
            dir.push_back((uint32_t)us.size());
            d_off[c + 1] = dir.size();
        }
    }
    if (us.size() >= 0xFFFFFFFFull) return fail(GFFX_E_INVALID, "gffx_hip_segments_covered: too many spans");
    void *bufs[12] = {nullptr};
    int nb_ = 0;
    auto cleanup = [&]() {
        for (int i = 0; i < nb_; i++) (void)hipFree(bufs[i]);
    };
    auto up = [&](const void *src, size_t bytes, void **dst) -> int {
        *dst = nullptr;
        hipError_t e = hipMalloc(dst, std::max<size_t>(bytes, 16));
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? GFFX_E_OOM : GFFX_E_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
        bufs[nb_++] = *dst;
        if (bytes && src) {
            e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(GFFX_E_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
        }
        return GFFX_OK;
    };
    void *d_uoff, *d_us, *d_ue, *d_pb, *d_dir, *d_doff, *d_dmeta, *d_sseq, *d_ss, *d_se, *d_cov;
    int rc;
    if ((rc = up(u_off.data(), u_off.size() * 8, &d_uoff)) || (rc = up(us.data(), us.size() * 4, &d_us)) ||
        (rc = up(ue.data(), ue.size() * 4, &d_ue)) || (rc = up(pb.data(), pb.size() * 8, &d_pb)) ||
        (rc = up(dir.data(), dir.size() * 4, &d_dir)) || (rc = up(d_off.data(), d_off.size() * 8, &d_doff)) ||
        (rc = up(d_meta.data(), d_meta.size() * sizeof(uint2), &d_dmeta)) || (rc = up(seg_seq, n_seg * 4, &d_sseq)) ||
        (rc = up(seg_start, n_seg * 4, &d_ss)) || (rc = up(seg_end, n_seg * 4, &d_se)) || (rc = up(nullptr, n_seg * 4, &d_cov))) {
        cleanup();
        return rc;
    }
    const UnionView U{(const unsigned long long *)d_uoff, (const uint32_t *)d_us, (const uint32_t *)d_ue,
                      (const unsigned long long *)d_pb,   (const uint32_t *)d_dir, (const unsigned long long *)d_doff,
                      (const uint2 *)d_dmeta,             n_seq};
    hipLaunchKernelGGL(k_segments_covered, dim3((uint32_t)((n_seg + 255) / 256)), dim3(256), 0, 0, U,
                       (unsigned long long)n_seg, (const uint32_t *)d_sseq, (const uint32_t *)d_ss, (const uint32_t *)d_se,
                       (uint32_t *)d_cov);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(covered_out, d_cov, n_seg * 4, hipMemcpyDeviceToHost);
    cleanup();
    if (e != hipSuccess) return fail(GFFX_E_HIP, "k_segments_covered failed: %s", hipGetErrorString(e));
    return GFFX_OK;
}

// ------------------------------------------------------------------------------------ the union, built on the device
// gffx_hip_union: the same union U, folded together chunk by chunk in HBM (include/gffx_hip.h "union builder").  One fold takes
// the spans accumulated so far -- they are rows too -- and a chunk of new rows, both as {seqid, start, end} records:
//   DeviceSort           stable LSD radix sort by (seqid, start)                                            radix_sort.hpp
//   k_union_tile_max     per tile of 1024 records the maximum of the 64-bit value (seqid << 32) | end.  The records are sorted by
//                        seqid, so the running maximum of that value is monotone in seqid and its low word is the running maximum
//                        of `end` INSIDE the seqid: the scan restarts at every seqid border without segment flags.
//   k_union_carry        one block: exclusive running maximum over the tiles (reduce-then-scan: nothing spins anywhere)
//   k_union_heads        record i heads a span when i == 0, its seqid differs from the running maximum's before it, or its start
//                        is > the running maximum end before it (merge while s <= current end: touching spans merge,
//                        coverage.rs:92-109); counts the heads per tile;   k_union_carry again: exclusive sum of the counts
//   k_union_emit         span k = the k-th head: its start from the head, its end from the running maximum at the span's last record
// GROUPING DOES NOT MATTER: the spans are the connected components of the rows under "closed intervals touch or overlap", and the
// components of a set do not depend on the order or the grouping in which its members are united.  A span stands for exactly the
// bases of its component, so folding rows chunk by chunk, or adding the spans of another union (gffx_hip_union_add_spans: the
// merge over devices), gives the same spans bit for bit as one merge_intervals over all rows (tests/test_coverage_union_gpu.py).
// Device memory: two record buffers of (spans so far + one fold of <= kUnionFold rows) and the sort's work space; the host keeps
// nothing per row.  _finish copies the SPANS out, adds the per-seqid prefix of their lengths, u_off and the directory on the host
// (one linear pass, nothing is sorted; same shift / nb rule as above) and uploads the tables k_segments_covered reads.
namespace gffx {

constexpr int kUnionThreads = 256;
constexpr uint32_t kUnionTile = 4 * kUnionThreads;  // 4 consecutive records per thread: three 16-byte loads
constexpr uint64_t kUnionFold = 8ull << 20;         // new rows per fold
constexpr uint32_t kUnionErrInverted = 8u;          // err word: a row with start >= end (2 and 4 are the sort's)

struct UnionRows {
    uint32_t seq[4], s[4], e[4];
};

__device__ __forceinline__ void union_load(const uint32_t *rec, unsigned long long n, unsigned long long i0, UnionRows &r) {
    uint32_t w[12];
    if (i0 + 4 <= n) {
        const uint4 *p = reinterpret_cast<const uint4 *>(rec + 3 * i0);  // (48 i0 bytes into a hipMalloc'd buffer: 16-byte aligned)
        const uint4 a = p[0], b = p[1], c = p[2];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w, w[8] = c.x, w[9] = c.y,
        w[10] = c.z, w[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = (i0 + k / 3 < n) ? rec[3 * i0 + k] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) r.seq[j] = w[3 * j], r.s[j] = w[3 * j + 1], r.e[j] = w[3 * j + 2];
}

template <bool SUM>
__device__ __forceinline__ unsigned long long union_op(unsigned long long a, unsigned long long b) {
    return SUM ? a + b : (a > b ? a : b);
}

// exclusive scan of v over the block's 256 threads (0 is the identity of both operations); *total = the block's whole.  s_w: 4 words
template <bool SUM>
__device__ __forceinline__ unsigned long long union_block_scan(unsigned long long v, unsigned long long *s_w, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc = union_op<SUM>(inc, t);
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, all = 0;
#pragma unroll
    for (int x = 0; x < kUnionThreads / 64; ++x) {
        if (x < wave) base = union_op<SUM>(base, s_w[x]);
        all = union_op<SUM>(all, s_w[x]);
    }
    const unsigned long long prev = __shfl_up(inc, 1, 64);
    *total = all;
    return lane ? union_op<SUM>(base, prev) : base;
}

// the tile's records and, per record, the running maximum of (seqid << 32) | end over ALL records before it (ex) and its own value
__device__ __forceinline__ void union_tile_scan(const uint32_t *rec, unsigned long long n, const unsigned long long *carry,
                                                unsigned long long *s_w, UnionRows &r, unsigned long long (&key)[4], unsigned long long (&ex)[4]) {
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kUnionTile + 4ull * threadIdx.x;
    union_load(rec, n, i0, r);
    unsigned long long m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        key[j] = i0 + j < n ? ((unsigned long long)r.seq[j] << 32) | r.e[j] : 0ull;
        m = m > key[j] ? m : key[j];
    }
    unsigned long long total;
    unsigned long long run = union_block_scan<false>(m, s_w, &total);
    const unsigned long long c = carry[blockIdx.x];
    run = run > c ? run : c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ex[j] = run;
        run = run > key[j] ? run : key[j];
    }
}

__device__ __forceinline__ bool union_is_head(unsigned long long i, uint32_t seq, uint32_t s, unsigned long long ex) {
    return i == 0 || (uint32_t)(ex >> 32) != seq || s > (uint32_t)ex;
}

__global__ __launch_bounds__(kUnionThreads) void k_union_tile_max(const uint32_t *rec, unsigned long long n, unsigned long long *tile_max, uint32_t *err) {
    __shared__ unsigned long long s_w[kUnionThreads / 64];
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kUnionTile + 4ull * threadIdx.x;
    UnionRows r;
    union_load(rec, n, i0, r);
    unsigned long long m = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) {
            const unsigned long long k = ((unsigned long long)r.seq[j] << 32) | r.e[j];
            m = m > k ? m : k;
            bad |= r.s[j] >= r.e[j];
        }
    unsigned long long total;
    (void)union_block_scan<false>(m, s_w, &total);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = total;
    if (bad) atomicOr(err, kUnionErrInverted);
}

// one block: v[i] <- the exclusive scan of v (in place), *total <- the whole (may be NULL)
template <bool SUM>
__global__ __launch_bounds__(kUnionThreads) void k_union_carry(unsigned long long *v, uint32_t n, unsigned long long *total) {
    __shared__ unsigned long long s_w[kUnionThreads / 64];
    unsigned long long run = 0;
    for (uint32_t base = 0; base < n; base += kUnionThreads) {
        const uint32_t i = base + threadIdx.x;
        unsigned long long all;
        const unsigned long long ex = union_block_scan<SUM>(i < n ? v[i] : 0ull, s_w, &all);
        if (i < n) v[i] = union_op<SUM>(run, ex);
        run = union_op<SUM>(run, all);
        __syncthreads();  // (s_w is rewritten by the next step)
    }
    if (threadIdx.x == 0 && total) *total = run;
}

__global__ __launch_bounds__(kUnionThreads) void k_union_heads(const uint32_t *rec, unsigned long long n, const unsigned long long *carry,
                                                               unsigned long long *tile_heads) {
    __shared__ unsigned long long s_w[kUnionThreads / 64], s_w2[kUnionThreads / 64];
    UnionRows r;
    unsigned long long key[4], ex[4];
    union_tile_scan(rec, n, carry, s_w, r, key, ex);
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kUnionTile + 4ull * threadIdx.x;
    unsigned long long heads = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n && union_is_head(i0 + j, r.seq[j], r.s[j], ex[j])) heads++;
    unsigned long long total;
    (void)union_block_scan<true>(heads, s_w2, &total);
    if (threadIdx.x == 0) tile_heads[blockIdx.x] = total;
}

// out: span k = {seqid, start of the k-th head, running maximum end at the last record before the next head}
__global__ __launch_bounds__(kUnionThreads) void k_union_emit(const uint32_t *rec, unsigned long long n, const unsigned long long *carry,
                                                              const unsigned long long *tile_base, uint32_t *out) {
    __shared__ unsigned long long s_w[kUnionThreads / 64], s_w2[kUnionThreads / 64];
    UnionRows r;
    unsigned long long key[4], ex[4];
    union_tile_scan(rec, n, carry, s_w, r, key, ex);
    const unsigned long long i0 = (unsigned long long)blockIdx.x * kUnionTile + 4ull * threadIdx.x;
    bool head[4];
    unsigned long long heads = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        head[j] = i0 + j < n && union_is_head(i0 + j, r.seq[j], r.s[j], ex[j]);
        heads += head[j] ? 1 : 0;
    }
    unsigned long long total;
    unsigned long long rank = tile_base[blockIdx.x] + union_block_scan<true>(heads, s_w2, &total);  // heads before my first record
    uint32_t nseq = 0, ns = 0;  // the record behind my fourth
    if (i0 + 4 < n) nseq = rec[3 * (i0 + 4)], ns = rec[3 * (i0 + 4) + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long i = i0 + j;
        if (i >= n) break;
        rank += head[j] ? 1 : 0;  // (record 0 is a head: rank >= 1 from here on)
        const unsigned long long k = rank - 1, inc = ex[j] > key[j] ? ex[j] : key[j];
        if (head[j]) out[3 * k] = r.seq[j], out[3 * k + 1] = r.s[j];
        const uint32_t s1 = j < 3 ? r.seq[j + 1] : nseq, b1 = j < 3 ? r.s[j + 1] : ns;
        if (i + 1 >= n || s1 != r.seq[j] || b1 > (uint32_t)inc) out[3 * k + 2] = (uint32_t)inc;
    }
}

}  // namespace gffx

namespace {

void union_drop_tables(gffx_hip_union *U) {
    for (void *&p : U->tables) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    U->finished = false;
}

// room for the spans so far + m new rows (the spans stay at the front of rec_a)
int union_reserve(gffx_hip_union *U, uint64_t m) {
    const uint64_t n = U->n_spans + m;
    if (n >= (1ull << 30)) return fail(GFFX_E_INVALID, "gffx_hip_union: %llu spans + rows in one fold exceed the limit of 2^30 - 1", (unsigned long long)n);
    int rc;
    if (n > U->cap) {
        const uint64_t cap = n + n / 4 + 1024;
        uint32_t *a = nullptr, *b = nullptr;
        if ((rc = dev_alloc_padded(&a, 3 * cap))) return rc;
        if ((rc = dev_alloc_padded(&b, 3 * cap))) {
            (void)hipFree(a);
            return rc;
        }
        hipError_t e = hipSuccess;
        if (U->n_spans) e = hipMemcpyAsync(a, U->rec_a, U->n_spans * 12, hipMemcpyDeviceToDevice, U->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(U->stream);
        if (e != hipSuccess) {
            (void)hipFree(a);
            (void)hipFree(b);
            return fail(GFFX_E_HIP, "gffx_hip_union: moving the spans failed: %s", hipGetErrorString(e));
        }
        (void)hipFree(U->rec_a);
        (void)hipFree(U->rec_b);
        U->rec_a = a, U->rec_b = b, U->cap = cap;
    }
    const uint64_t want_work = DeviceSort::work_words(U->cap, U->plan.n_passes), want_tiles = (U->cap + kUnionTile - 1) / kUnionTile + 1;
    if (want_work > U->cap_work) {
        if (U->work) GFFX_HIP_TRY(hipFree(U->work));
        U->cap_work = 0;
        if ((rc = dev_alloc_padded(&U->work, want_work))) return rc;
        U->cap_work = want_work;
    }
    if (want_tiles > U->cap_tiles) {
        if (U->tile_a) GFFX_HIP_TRY(hipFree(U->tile_a));
        if (U->tile_b) GFFX_HIP_TRY(hipFree(U->tile_b));
        U->tile_a = U->tile_b = nullptr;
        U->cap_tiles = 0;
        if ((rc = dev_alloc_padded(&U->tile_a, want_tiles)) || (rc = dev_alloc_padded(&U->tile_b, want_tiles))) return rc;
        U->cap_tiles = want_tiles;
    }
    return GFFX_OK;
}

// rec_a = [spans so far | m new rows] (the rows' copy is enqueued on the stream) -> rec_a = [spans of all of them]
int union_fold(gffx_hip_union *U, uint64_t m) {
    const unsigned long long n = U->n_spans + m;
    if (!m) return GFFX_OK;
    union_drop_tables(U);
    GFFX_HIP_TRY(hipMemsetAsync(U->ctl, 0, 32, U->stream));
    GFFX_HIP_TRY(hipEventRecord(U->ev0, U->stream));
    uint32_t *sorted = nullptr;
    int rc = DeviceSort::run<3>(U->stream, U->rec_a, U->rec_b, n, U->plan, U->n_seq, U->work, U->ctl, &sorted);
    if (rc) return rc;
    uint32_t *out = sorted == U->rec_a ? U->rec_b : U->rec_a;
    const uint32_t tiles = (uint32_t)((n + kUnionTile - 1) / kUnionTile);
    unsigned long long *count = reinterpret_cast<unsigned long long *>(U->ctl + 4);
    hipLaunchKernelGGL(k_union_tile_max, dim3(tiles), dim3(kUnionThreads), 0, U->stream, sorted, n, U->tile_a, U->ctl);
    hipLaunchKernelGGL(k_union_carry<false>, dim3(1), dim3(kUnionThreads), 0, U->stream, U->tile_a, tiles, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(k_union_heads, dim3(tiles), dim3(kUnionThreads), 0, U->stream, sorted, n, U->tile_a, U->tile_b);
    hipLaunchKernelGGL(k_union_carry<true>, dim3(1), dim3(kUnionThreads), 0, U->stream, U->tile_b, tiles, count);
    hipLaunchKernelGGL(k_union_emit, dim3(tiles), dim3(kUnionThreads), 0, U->stream, sorted, n, U->tile_a, U->tile_b, out);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(U->ev1, U->stream));
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    GFFX_HIP_TRY(hipMemcpyAsync(h, U->ctl, 32, hipMemcpyDeviceToHost, U->stream));
    GFFX_HIP_TRY(hipStreamSynchronize(U->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, U->ev0, U->ev1) == hipSuccess) U->kernel_ms += ms;
    U->folds++;
    if (h[0] & 2u) return fail(GFFX_E_CHR_RANGE, "gffx_hip_union: a row has chr >= %u", U->n_seq);
    if (h[0] & 4u) return fail(GFFX_E_HIP, "gffx_hip_union: the device sort timed out waiting for an earlier tile");
    if (h[0] & kUnionErrInverted) return fail(GFFX_E_INVALID, "gffx_hip_union: a row has start >= end");
    const uint64_t spans = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
    if (spans >= 0xFFFFFFFFull) return fail(GFFX_E_INVALID, "gffx_hip_union: too many spans");
    U->n_spans = spans;
    if (out != U->rec_a) std::swap(U->rec_a, U->rec_b);  // the spans are the front of rec_a again
    U->rows_added += m;
    return GFFX_OK;
}

}  // namespace

extern "C" void gffx_hip_union_destroy(gffx_hip_union *U) {
    if (!U) return;
    (void)hipSetDevice(U->device);
    if (U->stream) (void)hipStreamSynchronize(U->stream);
    union_drop_tables(U);
    for (void *p : {(void *)U->rec_a, (void *)U->rec_b, (void *)U->work, (void *)U->tile_a, (void *)U->tile_b, (void *)U->ctl, (void *)U->d_seg[0],
                    (void *)U->d_seg[1], (void *)U->d_seg[2], (void *)U->d_seg[3]})
        if (p) (void)hipFree(p);
    if (U->h_stage) (void)hipHostFree(U->h_stage);
    if (U->ev0) (void)hipEventDestroy(U->ev0);
    if (U->ev1) (void)hipEventDestroy(U->ev1);
    if (U->stream) (void)hipStreamDestroy(U->stream);
    delete U;
}

extern "C" int gffx_hip_union_create(int device, uint32_t n_seq, gffx_hip_union **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_union_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    if (ndev <= 0) return fail(GFFX_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFFX_E_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_union, void (*)(gffx_hip_union *)> U(new gffx_hip_union, gffx_hip_union_destroy);
    U->device = device;
    U->n_seq = n_seq;
    // by (seqid, start): the four bytes of the start, then as many bytes of the seqid as n_seq needs (the sort's top-digit
    // shortcut is for <= 256 seqids and is not asked for here)
    int seq_bytes = 1;
    while (seq_bytes < 4 && (n_seq > (1u << (8 * seq_bytes)))) seq_bytes++;
    for (int b = 0; b < 4; ++b) U->plan.word[U->plan.n_passes] = 1, U->plan.shift[U->plan.n_passes++] = (uint8_t)(8 * b);
    for (int b = 0; b < seq_bytes; ++b) U->plan.word[U->plan.n_passes] = 0, U->plan.shift[U->plan.n_passes++] = (uint8_t)(8 * b);
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&U->stream, hipStreamNonBlocking));
    GFFX_HIP_TRY(hipEventCreate(&U->ev0));
    GFFX_HIP_TRY(hipEventCreate(&U->ev1));
    int rc = dev_alloc_padded(&U->ctl, 8);
    if (rc) return rc;
    *out = U.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_union_add_host(gffx_hip_union *U, const uint32_t *rows, uint64_t n_rows) {
    int rc = enter_handle(U, "gffx_hip_union_add_host");
    if (rc) return rc;
    if (n_rows && !rows) return fail(GFFX_E_INVALID, "gffx_hip_union_add_host: rows is NULL");
    const uint64_t want = std::min<uint64_t>(n_rows, kUnionFold);
    if (want > U->cap_stage) {
        if (U->h_stage) (void)hipHostFree(U->h_stage);
        U->h_stage = nullptr, U->cap_stage = 0;
        hipError_t e = hipHostMalloc((void **)&U->h_stage, want * 12, hipHostMallocDefault);
        if (e != hipSuccess) return fail(GFFX_E_OOM, "hipHostMalloc of a %llu-row staging buffer failed: %s", (unsigned long long)want, hipGetErrorString(e));
        U->cap_stage = want;
    }
    for (uint64_t at = 0; at < n_rows; at += kUnionFold) {
        const uint64_t m = std::min<uint64_t>(kUnionFold, n_rows - at);
        GFFX_KEEP_TRY(U, union_reserve(U, m));
        std::memcpy(U->h_stage, rows + 3 * at, m * 12);  // (the fold below ends with a synchronisation: the buffer is free again)
        GFFX_HIP_TRY(hipMemcpyAsync(U->rec_a + 3 * U->n_spans, U->h_stage, m * 12, hipMemcpyHostToDevice, U->stream));
        GFFX_KEEP_TRY(U, union_fold(U, m));
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_union_add_store(gffx_hip_union *U, const gffx_hip_regions *R, int k, uint64_t first, uint64_t n_rows) {
    int rc = enter_handle(U, "gffx_hip_union_add_store");
    if (rc) return rc;
    const uint32_t *src = nullptr;
    if ((rc = store_slot_rows(R, k, first, n_rows, U->device, "gffx_hip_union_add_store", "union", &src))) return rc;
    if (R->pending[k]) GFFX_HIP_TRY(hipStreamWaitEvent(U->stream, R->copied[k], 0));
    for (uint64_t at = 0; at < n_rows; at += kUnionFold) {
        const uint64_t m = std::min<uint64_t>(kUnionFold, n_rows - at);
        GFFX_KEEP_TRY(U, union_reserve(U, m));
        GFFX_HIP_TRY(hipMemcpyAsync(U->rec_a + 3 * U->n_spans, src + 3 * at, m * 12, hipMemcpyDeviceToDevice, U->stream));
        GFFX_KEEP_TRY(U, union_fold(U, m));
    }
    return GFFX_OK;
}

extern "C" int gffx_hip_union_add_spans(gffx_hip_union *U, const uint64_t *u_off, const uint32_t *us, const uint32_t *ue) {
    int rc = enter_handle(U, "gffx_hip_union_add_spans");
    if (rc) return rc;
    if (!u_off) return fail(GFFX_E_INVALID, "gffx_hip_union_add_spans: u_off is NULL");
    const uint64_t n = u_off[U->n_seq];
    if (n && (!us || !ue)) return fail(GFFX_E_INVALID, "gffx_hip_union_add_spans: NULL span array");
    std::vector<uint32_t> rows;
    for (uint32_t c = 0; c < U->n_seq; ++c) {
        if (u_off[c + 1] < u_off[c] || u_off[c + 1] > n) return fail(GFFX_E_INVALID, "gffx_hip_union_add_spans: u_off is not ascending");
        for (uint64_t i = u_off[c]; i < u_off[c + 1]; ++i) {
            rows.push_back(c);
            rows.push_back(us[i]);
            rows.push_back(ue[i]);
        }
    }
    return gffx_hip_union_add_host(U, rows.data(), rows.size() / 3);
}

extern "C" int gffx_hip_union_finish(gffx_hip_union *U) {
    int rc = enter_handle(U, "gffx_hip_union_finish");
    if (rc) return rc;
    if (U->finished) return GFFX_OK;
    const uint32_t n_seq = U->n_seq;
    std::vector<uint32_t> rec(3 * U->n_spans);
    if (U->n_spans) GFFX_HIP_TRY(hipMemcpy(rec.data(), U->rec_a, U->n_spans * 12, hipMemcpyDeviceToHost));
    U->u_off.assign((size_t)n_seq + 1, 0);
    U->us.resize(U->n_spans), U->ue.resize(U->n_spans), U->pb.resize(U->n_spans);
    std::vector<unsigned long long> d_off((size_t)n_seq + 1, 0);
    std::vector<uint32_t> dir;
    std::vector<uint2> d_meta(n_seq, make_uint2(0, 0));
    uint64_t i = 0;
    for (uint32_t c = 0; c < n_seq; ++c) {
        const uint64_t u0 = i;
        unsigned long long acc = 0;
        for (; i < U->n_spans && rec[3 * i] == c; ++i) {
            U->us[i] = rec[3 * i + 1], U->ue[i] = rec[3 * i + 2], U->pb[i] = acc;
            acc += U->ue[i] - U->us[i];
        }
        U->u_off[c + 1] = i;
        d_off[c + 1] = d_off[c];
        const uint64_t n_u = i - u0;
        if (n_u) {  // (the rule of gffx_hip_segments_covered above)
            const uint32_t vmax = U->us[i - 1];
            const uint64_t budget = std::max<uint64_t>(2 * n_u, 16);
            uint32_t shift = 0;
            while ((((uint64_t)vmax >> shift) + 1) > budget) shift++;
            const uint32_t nb = (vmax >> shift) + 1;
            d_meta[c] = make_uint2(shift, nb);
            uint64_t p = u0;
            for (uint32_t b = 0; b < nb; b++) {
                const uint64_t edge = (uint64_t)b << shift;
                while (p < i && U->us[p] < edge) p++;
                dir.push_back((uint32_t)p);
            }
            dir.push_back((uint32_t)i);
            d_off[c + 1] = dir.size();
        }
    }
    if (i != U->n_spans) return keep_failure(U, fail(GFFX_E_HIP, "gffx_hip_union_finish: the spans are not in seqid order"));
    auto up = [&](const void *src, size_t bytes, void **dst) -> int {
        GFFX_HIP_TRY(hipMalloc(dst, std::max<size_t>(bytes, 16)));
        if (bytes) GFFX_HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return GFFX_OK;
    };
    if ((rc = up(U->u_off.data(), U->u_off.size() * 8, &U->tables[0])) || (rc = up(U->us.data(), U->us.size() * 4, &U->tables[1])) ||
        (rc = up(U->ue.data(), U->ue.size() * 4, &U->tables[2])) || (rc = up(U->pb.data(), U->pb.size() * 8, &U->tables[3])) ||
        (rc = up(dir.data(), dir.size() * 4, &U->tables[4])) || (rc = up(d_off.data(), d_off.size() * 8, &U->tables[5])) ||
        (rc = up(d_meta.data(), d_meta.size() * sizeof(uint2), &U->tables[6]))) {
        union_drop_tables(U);
        return keep_failure(U, rc);
    }
    U->finished = true;
    return GFFX_OK;
}

extern "C" uint64_t gffx_hip_union_n_spans(const gffx_hip_union *U) { return U ? U->n_spans : 0; }

extern "C" int gffx_hip_union_copy_spans(gffx_hip_union *U, uint64_t *u_off, uint32_t *us, uint32_t *ue, uint64_t *pb) {
    int rc = enter_handle(U, "gffx_hip_union_copy_spans");
    if (rc) return rc;
    if (!U->finished) return fail(GFFX_E_STATE, "gffx_hip_union_copy_spans: call gffx_hip_union_finish first");
    if (u_off) std::copy(U->u_off.begin(), U->u_off.end(), u_off);
    if (us) std::copy(U->us.begin(), U->us.end(), us);
    if (ue) std::copy(U->ue.begin(), U->ue.end(), ue);
    if (pb) std::copy(U->pb.begin(), U->pb.end(), pb);
    return GFFX_OK;
}

extern "C" int gffx_hip_union_stats(const gffx_hip_union *U, double *kernel_ms, uint64_t *rows, uint64_t *folds) {
    if (!U) return fail(GFFX_E_INVALID, "gffx_hip_union_stats: union is NULL");
    if (kernel_ms) *kernel_ms = U->kernel_ms;
    if (rows) *rows = U->rows_added;
    if (folds) *folds = U->folds;
    return GFFX_OK;
}

extern "C" int gffx_hip_union_segments_covered(gffx_hip_union *U, uint64_t n_seg, const uint32_t *seg_seq, const uint32_t *seg_start,
                                               const uint32_t *seg_end, uint32_t *covered_out) {
    int rc = enter_handle(U, "gffx_hip_union_segments_covered");
    if (rc) return rc;
    if (!U->finished) return fail(GFFX_E_STATE, "gffx_hip_union_segments_covered: call gffx_hip_union_finish first");
    if (n_seg && (!seg_seq || !seg_start || !seg_end || !covered_out))
        return fail(GFFX_E_INVALID, "gffx_hip_union_segments_covered: NULL segment array");
    for (uint64_t i = 0; i < n_seg; i++)
        if (seg_seq[i] >= U->n_seq)
            return fail(GFFX_E_CHR_RANGE, "gffx_hip_union_segments_covered: segment %llu has chr %u >= %u", (unsigned long long)i, seg_seq[i], U->n_seq);
    if (n_seg == 0) return GFFX_OK;
    if (n_seg > U->cap_seg) {
        for (uint32_t *&p : U->d_seg) {
            if (p) GFFX_HIP_TRY(hipFree(p));
            p = nullptr;
        }
        U->cap_seg = 0;
        for (uint32_t *&p : U->d_seg)
            if ((rc = dev_alloc_padded(&p, n_seg))) return rc;
        U->cap_seg = n_seg;
    }
    GFFX_HIP_TRY(hipMemcpyAsync(U->d_seg[0], seg_seq, n_seg * 4, hipMemcpyHostToDevice, U->stream));
    GFFX_HIP_TRY(hipMemcpyAsync(U->d_seg[1], seg_start, n_seg * 4, hipMemcpyHostToDevice, U->stream));
    GFFX_HIP_TRY(hipMemcpyAsync(U->d_seg[2], seg_end, n_seg * 4, hipMemcpyHostToDevice, U->stream));
    const UnionView V{(const unsigned long long *)U->tables[0], (const uint32_t *)U->tables[1], (const uint32_t *)U->tables[2],
                      (const unsigned long long *)U->tables[3], (const uint32_t *)U->tables[4], (const unsigned long long *)U->tables[5],
                      (const uint2 *)U->tables[6],              U->n_seq};
    hipLaunchKernelGGL(k_segments_covered, dim3((uint32_t)((n_seg + 255) / 256)), dim3(256), 0, U->stream, V, (unsigned long long)n_seg,
                       (const uint32_t *)U->d_seg[0], (const uint32_t *)U->d_seg[1], (const uint32_t *)U->d_seg[2], U->d_seg[3]);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipMemcpyAsync(covered_out, U->d_seg[3], n_seg * 4, hipMemcpyDeviceToHost, U->stream));
    GFFX_HIP_TRY(hipStreamSynchronize(U->stream));
    return GFFX_OK;
}
