// gff.hip -- `gffx index --gpu`: the GFF3 text on the device, from the bytes to the arrays behind the side-cars .fts .prt .a2f
// .atn .sqs .gof and the root list of .rit / .rix (reference: index_builder/core.rs:41-242).  The rules of one line are
// gff_core.hpp's, shared with the host and with tools/gff_check.cpp.
//
// One pass (the carry, i.e. the previous pass's unfinished line, followed by at most chunk_bytes new bytes = the text D):
//   k_gff_line_count   one wave per tile of kTile bytes: 16-byte loads, a bit per '\n', popcount
//   k_scan             the per-tile counts into bases                                           (the host reads the total)
//   k_gff_line_list    the same pass again; every '\n' offset in order (64-bit: a pass is not bounded by 4 GiB).  Line r is
//                      D[r ? nl[r - 1] + 1 : 0, nl[r]); the bytes after the last '\n' are the carry; at _finish a non-empty
//                      carry is the last line: the last tile then lists one more line end, at N
//   k_gff_rows<0>      one wave per tile, one lane per line that ends in the tile: gff_record, then per tile the kept rows,
//                      the bytes of their four strings and the type-skipped lines; the tallies; the first error as
//                      atomicMin over (file offset of the line << 3 | kind), the same whatever order the waves run in
//   k_scan x 6         those into bases                                                       (the host reads the totals)
//   k_gff_rows<1>      the same walk again: every kept row appends, in file order, its line offset, start, end and flag
//                      and the bytes of column 1, ID, Parent and the attribute value to four arenas (one end offset per
//                      row and arena: string r = bytes[off[r], off[r + 1])); type-skipped lines append their file offsets
// The two reads by the host make the growth of the arenas exact and let a malformed file fail before anything is appended.
// These line kernels restate sam.hip's with 64-bit line ends and without a header; the BAM/SAM readers are untouched.
//
// _finish, over the whole file (a Parent= may name a later line):
//   k_table_insert     all IDs into the ID table (string_table.hpp: one compare-and-swap, atomicMax: the last row wins)
//   k_gff_resolve      (a launch of its own, after all inserts) fid = the table's value of the row's own ID; prt = the
//                      value of its Parent where it has one that is found, else fid; root = (prt == fid)
//   numbering by first appearance, once for column 1 over the root rows and once for the attribute value over the rows
//   that have one: k_gff_insert_min (the same table, the LOWEST row per string: atomicMin), k_gff_first (a row is the first
//   of its string iff the table returns the row itself), k_scan (the number of a string = the count of first rows before
//   its first row), k_gff_number, and the names themselves compacted in that order (k_gff_name_len, k_scan, k_gff_name_put)
//   k_gff_root_list, k_gff_gof   the root rows compacted in file order; .gof entry k = (fid, seq, line offset of root k, of
//                      root k + 1 / the fed byte count) and the tree input (start, end, fid, seq)
// Every step is one thread per row or per slot; no step's work is (distinct strings x rows).
//
// LANE SHARING in k_gff_rows: one lane per line, as in sam.hip and for its reason -- one code path for a 60-byte line and a
// 1 MB one, the one tools/gff_check.cpp runs under the sanitizers.  HYPOTHESIS until measured (tools/index_bench.py, DESIGN
// 16): the rows kernels are bound by the serial byte walk of a lane over its line (UTF-8 check, TABs, three key searches:
// about five passes over ~250 bytes), not by memory; the finish steps by the latency of dependent, uncoalesced probes.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "gff_core.hpp"
#include "string_table.hpp"
#include "table_handle.hpp"

namespace gffx {

constexpr uint32_t kGffTile = 4096;  // bytes per tile: 4 steps of 64 lanes x 16 bytes
constexpr u64 kNoError = 0xFFFFFFFFFFFFFFFFull;
constexpr u64 kMaxRows = 1ull << 30;  // ids::table_slots is 32-bit
constexpr int kSums = 6;              // per tile: rows, bytes of seq / id / parent / attr, type-skipped lines

struct GffResult {  // what the host reads back after a pass
    u64 error;      // (file offset of the line << 3) | (kind - gff::kFirstError) of the first bad line (kNoError: none)
    u64 tail;       // D[tail, N) is the unfinished line
    u64 lines;
    u64 blank, zero_end;
    u64 total[kSums];
    u64 overflow;  // a tile whose strings of one kind total 4 GiB or more
};

// bit i = D[off + i] == '\n', i < 16, off + i < N (off: a multiple of 16; D: 16-byte aligned)
__device__ __forceinline__ uint32_t gff_nl_bits(const uint8_t *D, u64 N, u64 off) {
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

// one wave per tile: count[t] = the '\n' in tile t (+ 1 in the last tile when final_line: the line end at N);
// res->tail = one past the last '\n'
__global__ __launch_bounds__(64) void k_gff_line_count(const uint8_t *D, u64 N, uint32_t n_tiles, int final_line, uint32_t *count,
                                                       GffResult *res) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tiles) return;
    uint32_t c = 0;
    u64 last = 0;
    for (uint32_t it = 0; it < kGffTile / 1024; ++it) {
        const u64 off = (u64)t * kGffTile + it * 1024 + lane * 16;
        if (off >= N) break;
        const uint32_t m = gff_nl_bits(D, N, off);
        c += __popc(m);
        if (m) last = off + (31 - __clz(m)) + 1;
    }
    for (int d = 32; d; d >>= 1) {
        c += __shfl_xor(c, d);
        const u64 o = __shfl_xor(last, d);
        last = o > last ? o : last;
    }
    if (lane == 0) {
        count[t] = c + ((final_line && t == n_tiles - 1) ? 1u : 0u);
        if (last) atomicMax(&res->tail, last);
    }
}

// one wave per tile: nl[base[t] ..) = the offsets of the tile's '\n' in order (and N after them: see k_gff_line_count)
__global__ __launch_bounds__(64) void k_gff_line_list(const uint8_t *D, u64 N, uint32_t n_tiles, int final_line, const u64 *base, u64 *nl,
                                                      u64 nl_cap) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tiles) return;
    u64 o = base[t];
    for (uint32_t it = 0; it < kGffTile / 1024; ++it) {  // (wave-uniform trip count: the shuffles below need every lane)
        const u64 off = (u64)t * kGffTile + it * 1024 + lane * 16;
        uint32_t m = off < N ? gff_nl_bits(D, N, off) : 0u;
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
            if (at < nl_cap) nl[at] = off + b;
            ++at;
        }
        o += __shfl(incl, 63);
    }
    if (final_line && t == n_tiles - 1 && lane == 0 && o < nl_cap) nl[o] = N;
}

struct GffParams {
    const uint8_t *key;
    uint32_t key_len;
    gff::SkipList skip;
};

struct GffOut {  // the arrays of the whole file; a pass appends behind row_base / the *_base bytes / skip_base
    u64 *line_off;
    uint32_t *start, *end, *flags;
    uint8_t *bytes[4];  // seq, id, parent, attr
    u64 *off[4];        // off[k][r + 1] = the end of row r's string k (off[k][0] = 0)
    u64 base[4];
    u64 row_base, skip_base;
    u64 *skipped;  // file offsets of the type-skipped lines
    u64 row_cap, skip_cap, byte_cap[4];  // never the bounds that decide: the host sized the arrays by the count pass
};

__device__ __forceinline__ u64 wave_excl(u64 v, uint32_t lane, u64 *total) {
    u64 incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(incl, d);
        if ((int)lane >= d) incl += o;
    }
    *total = __shfl(incl, 63);
    return incl - v;
}

// one wave per tile, one lane per line that ends in the tile.  WRITE = 0: the tile's sums (sums[k * n_tiles + t]), the tallies,
// the first error.  WRITE = 1: the kept rows and the type-skipped lines appended at the tile's bases (tile_base[k * (n_tiles + 1) + t]).
template <int WRITE>
__global__ __launch_bounds__(64) void k_gff_rows(const uint8_t *D, u64 d_file_off, const u64 *line_base, const u64 *nl, uint32_t n_tiles,
                                                 GffParams P, uint32_t *sums, const u64 *tile_base, GffOut O, GffResult *res) {
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_tiles) return;
    const u64 a = line_base[t], z = line_base[t + 1];
    u64 o[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) o[k] = WRITE ? tile_base[(u64)k * (n_tiles + 1) + t] : 0;
    uint32_t blank = 0, zero_end = 0;
    for (u64 r0 = a; r0 < z; r0 += 64) {
        const u64 r = r0 + lane;
        gff::Rec rec{};
        int st = gff::kBlank;
        u64 ls = 0;
        bool live = false;
        if (r < z) {
            live = true;
            ls = r ? nl[r - 1] + 1 : 0;
            st = gff::gff_record(D + ls, nl[r] - ls, P.key, P.key_len, P.skip, &rec);
        }
        u64 v[kSums] = {0, 0, 0, 0, 0, 0};
        if (live) {
            if (st == gff::kRow) {
                v[0] = 1;
                v[1] = rec.seq_z - rec.seq_a;
                v[2] = rec.id_z - rec.id_a;
                v[3] = rec.par_z - rec.par_a;
                v[4] = rec.attr_z - rec.attr_a;
            } else if (st == gff::kSkipType) {
                v[5] = 1;
            } else if (st == gff::kBlank) {
                ++blank;
            } else if (st == gff::kZeroEnd) {
                ++zero_end;
            } else if (!WRITE) {
                atomicMin(&res->error, ((d_file_off + ls) << 3) | (u64)(st - gff::kFirstError));
            }
        }
        u64 at[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
            u64 tot;
            at[k] = o[k] + wave_excl(v[k], lane, &tot);
            o[k] += tot;
        }
        if (WRITE && live && st == gff::kRow) {
            const u64 row = O.row_base + at[0];
            if (row < O.row_cap) {
                O.line_off[row] = d_file_off + ls;
                O.start[row] = rec.start;
                O.end[row] = rec.end;
                O.flags[row] = rec.warn;
                const u64 from[4] = {rec.seq_a, rec.id_a, rec.par_a, rec.attr_a};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const u64 dst = O.base[k] + at[k + 1], n = v[k + 1];
                    O.off[k][row + 1] = dst + n;
                    if (dst + n <= O.byte_cap[k])
                        for (u64 i = 0; i < n; ++i) O.bytes[k][dst + i] = D[ls + from[k] + i];
                }
            }
        }
        if (WRITE && live && st == gff::kSkipType) {
            const u64 s = O.skip_base + at[5];
            if (s < O.skip_cap) O.skipped[s] = d_file_off + ls;
        }
    }
    if (!WRITE) {
        for (int d = 32; d; d >>= 1) {
            blank += __shfl_xor(blank, d);
            zero_end += __shfl_xor(zero_end, d);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) {
                sums[(u64)k * n_tiles + t] = (uint32_t)o[k];
                if (o[k] > 0xFFFFFFFFull) atomicAdd(&res->overflow, 1ull);
            }
            if (blank) atomicAdd(&res->blank, (u64)blank);
            if (zero_end) atomicAdd(&res->zero_end, (u64)zero_end);
        }
    }
}

// ---- the finish steps: one thread per slot or per row --------------------------------------------------------------------
// what decides whether row f takes part in a numbering: its root flag (column 1), or that it has a value (attribute)
__device__ __forceinline__ bool gff_eligible(const uint32_t *root, const u64 *off, uint32_t f) {
    return root ? root[f] != 0 : off[f + 1] > off[f];
}

// the rows that take part enter the table with the LOWEST row per string (the values filled for Keep::kSmallest)
__global__ __launch_bounds__(256) void k_gff_insert_min(u64 *slot, uint32_t *val, const uint8_t *bytes, const u64 *off, const uint32_t *root,
                                                        uint32_t n, uint32_t mask, uint32_t hash_mask) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < n && gff_eligible(root, off, f)) ids::table_insert_one<ids::Keep::kSmallest>(slot, val, bytes, off, f, mask, hash_mask);
}

__global__ __launch_bounds__(256) void k_gff_resolve(ids::Table t, const uint8_t *par_bytes, const u64 *par_off, uint32_t n, uint32_t *fid,
                                                     uint32_t *prt, uint32_t *root) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u64 a = t.off[r];
    uint32_t f = ids::table_find(t, t.bytes + a, t.off[r + 1] - a);
    if (f == ids::kNone) f = r;  // (cannot happen: the row's own ID was inserted)
    uint32_t p = f;
    const u64 pa = par_off[r], pn = par_off[r + 1] - pa;
    if (pn) {
        const uint32_t q = ids::table_find(t, par_bytes + pa, pn);
        if (q != ids::kNone) p = q;
    }
    fid[r] = f;
    prt[r] = p;
    root[r] = p == f ? 1u : 0u;
}

// first_row[r] = the lowest row with r's string (kNone: r takes no part); is_first[r] = (first_row[r] == r)
__global__ __launch_bounds__(256) void k_gff_first(ids::Table t, const uint32_t *root, uint32_t n, uint32_t *first_row, uint32_t *is_first) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    uint32_t f = ids::kNone;
    if (gff_eligible(root, t.off, r)) {
        const u64 a = t.off[r];
        f = ids::table_find(t, t.bytes + a, t.off[r + 1] - a);
    }
    first_row[r] = f;
    is_first[r] = f == r ? 1u : 0u;
}

// number[r] = rank[first_row[r]] (the first rows before r's first row), kNone for a row that takes no part;
// name_len[r] = the bytes of a first row's string and its '\n'
__global__ __launch_bounds__(256) void k_gff_number(const uint32_t *first_row, const u64 *rank, const u64 *off, uint32_t n, uint32_t *number,
                                                    uint32_t *name_len) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t f = first_row[r];
    number[r] = f < n ? (uint32_t)rank[f] : ids::kNone;
    name_len[r] = f == r ? (uint32_t)(off[r + 1] - off[r] + 1) : 0u;  // (< 2^32: the pass checked the strings of a tile)
}

__global__ __launch_bounds__(256) void k_gff_name_put(const uint32_t *first_row, const u64 *at, const uint8_t *bytes, const u64 *off, uint32_t n,
                                                      uint8_t *out, u64 out_cap) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n || first_row[r] != r) return;
    const u64 a = off[r], len = off[r + 1] - a, dst = at[r];
    if (dst + len + 1 > out_cap) return;
    for (u64 i = 0; i < len; ++i) out[dst + i] = bytes[a + i];
    out[dst + len] = '\n';
}

// .fts: every ID and a '\n', row after row
__global__ __launch_bounds__(256) void k_gff_fts(const uint8_t *bytes, const u64 *off, uint32_t n, uint8_t *out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u64 a = off[r], len = off[r + 1] - a, dst = a + r;
    for (u64 i = 0; i < len; ++i) out[dst + i] = bytes[a + i];
    out[dst + len] = '\n';
}

__global__ __launch_bounds__(256) void k_gff_root_list(const uint32_t *root, const u64 *at, uint32_t n, uint32_t *root_rows, u64 n_roots) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n && root[r] && at[r] < n_roots) root_rows[at[r]] = r;
}

// gof[6 k ..] = fid, seq, line offset (lo, hi), end offset (lo, hi): the 24 little-endian bytes of a .gof entry;
// roots[4 k ..] = start, end, fid, seq
__global__ __launch_bounds__(256) void k_gff_gof(const uint32_t *root_rows, uint32_t n_roots, const uint32_t *fid, const uint32_t *seq,
                                                 const u64 *line_off, const uint32_t *start, const uint32_t *end, u64 file_bytes, uint32_t *gof,
                                                 uint32_t *roots) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_roots) return;
    const uint32_t r = root_rows[k];
    const u64 a = line_off[r], z = k + 1 < n_roots ? line_off[root_rows[k + 1]] : file_bytes;
    gof[6 * (u64)k] = fid[r];
    gof[6 * (u64)k + 1] = seq[r];
    gof[6 * (u64)k + 2] = (uint32_t)a;
    gof[6 * (u64)k + 3] = (uint32_t)(a >> 32);
    gof[6 * (u64)k + 4] = (uint32_t)z;
    gof[6 * (u64)k + 5] = (uint32_t)(z >> 32);
    roots[4 * (u64)k] = start[r];
    roots[4 * (u64)k + 1] = end[r];
    roots[4 * (u64)k + 2] = fid[r];
    roots[4 * (u64)k + 3] = seq[r];
}

inline dim3 grid256(u64 n) { return dim3((uint32_t)std::max<u64>((n + 255) / 256, 1)); }

}  // namespace gffx

using namespace gffx;

struct gffx_hip_gff : StreamEvents<3> {
    int device = 0;
    uint64_t chunk_bytes = 0;
    int hash_bits = -1;
    GffResult *res_host = nullptr;  // pinned
    DevArr<GffResult> res;
    DevArr<uint8_t> key, skip_bytes;
    DevArr<uint32_t> skip_off;
    uint32_t key_len = 0, n_skip = 0;
    std::vector<uint8_t> pend;  // text fed in pieces smaller than a pass
    // the pass
    DevArr<uint8_t> D[2];
    int cur = 0;
    uint64_t carry = 0, d_file_off = 0, fed = 0;
    DevArr<uint32_t> count, sums;
    DevArr<u64> line_base, tile_base, nl;
    // the whole file
    DevArr<u64> line_off, off[4], skipped;
    DevArr<uint32_t> start, end, flags;
    DevArr<uint8_t> bytes[4];
    uint64_t n_rows = 0, n_skipped = 0, n_bytes[4] = {0, 0, 0, 0};
    uint64_t lines = 0, blank = 0, zero_end = 0;
    // the finish steps
    bool finished = false;
    DevArr<u64> slot, rank, at;
    DevArr<uint32_t> val, fid, prt, root, first_row, is_first, seq, a2f, name_len, root_rows, gof, roots;
    DevArr<uint8_t> fts, sqs, atn;
    uint64_t n_roots = 0, n_seqids = 0, n_attrs = 0, sqs_bytes = 0, atn_bytes = 0;
    double ms[5] = {0, 0, 0, 0, 0};  // line scan, rows kernels, table build, resolve, numbering
    // the first bad line
    bool has_bad = false;
    uint64_t bad_off = 0;
    int bad_kind = 0;
    int error = GFFX_OK;
    std::string error_msg;

    ~gffx_hip_gff() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (res_host) (void)hipHostFree(res_host);
    }
    int sticky(int rc) {
        if (rc != GFFX_OK && error == GFFX_OK) {
            error = rc;
            error_msg = g_last_error;
        }
        return rc;
    }
};

namespace {

// one pass over the carry followed by the T bytes at p; final_line: the carry alone, as the file's last line
int run_pass(gffx_hip_gff *h, const uint8_t *p, uint64_t T, int final_line) {
    const uint64_t C = h->carry, N = C + T;
    if (N == 0) return GFFX_OK;
    hipStream_t s = h->stream;
    GFFX_HIP_TRY(grow_keep(h->D[h->cur], C, N + ids::kPad + (64u << 10)));  // (slack for the usual carry; a line longer than a pass: the buffer grows)
    uint8_t *D = h->D[h->cur].p;
    if (T) GFFX_HIP_TRY(hipMemcpyAsync(D + C, p, T, hipMemcpyHostToDevice, s));
    const uint64_t tiles64 = (N + kGffTile - 1) / kGffTile;
    if (tiles64 > 0x7FFFFFFFull) return fail(GFFX_E_INVALID, "gffx_hip_gff_feed: a pass of %llu bytes (at most 8 TiB)", (unsigned long long)N);
    const uint32_t n_tiles = (uint32_t)tiles64;
    GFFX_HIP_TRY(h->count.ensure(n_tiles));
    GFFX_HIP_TRY(h->line_base.ensure(n_tiles + 1));
    GFFX_HIP_TRY(h->sums.ensure((size_t)kSums * n_tiles));
    GFFX_HIP_TRY(h->tile_base.ensure((size_t)kSums * (n_tiles + 1)));
    GffResult init{};
    init.error = kNoError;
    *h->res_host = init;
    GFFX_HIP_TRY(hipMemcpyAsync(h->res.p, h->res_host, sizeof init, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_gff_line_count, dim3(n_tiles), dim3(64), 0, s, D, N, n_tiles, final_line, h->count.p, h->res.p);
    launch_scan(s, h->count.p, n_tiles, h->line_base.p, &h->res.p->lines);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipMemcpyAsync(h->res_host, h->res.p, sizeof init, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    const uint64_t n_lines = h->res_host->lines, tail = final_line ? N : h->res_host->tail;
    if (n_lines) {
        GFFX_HIP_TRY(h->nl.ensure(n_lines));
        hipLaunchKernelGGL(k_gff_line_list, dim3(n_tiles), dim3(64), 0, s, D, N, n_tiles, final_line, h->line_base.p, h->nl.p, (u64)n_lines);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
        const GffParams P{h->key.p, h->key_len, gff::SkipList{h->skip_bytes.p, h->skip_off.p, h->n_skip}};
        GffOut O{};
        hipLaunchKernelGGL(k_gff_rows<0>, dim3(n_tiles), dim3(64), 0, s, D, (u64)h->d_file_off, h->line_base.p, h->nl.p, n_tiles, P, h->sums.p,
                           h->tile_base.p, O, h->res.p);
        for (int k = 0; k < kSums; ++k)
            launch_scan(s, h->sums.p + (size_t)k * n_tiles, n_tiles, h->tile_base.p + (size_t)k * (n_tiles + 1), &h->res.p->total[k]);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipMemcpyAsync(h->res_host, h->res.p, sizeof init, hipMemcpyDeviceToHost, s));
        GFFX_HIP_TRY(hipStreamSynchronize(s));
        const GffResult r = *h->res_host;
        if (r.error != kNoError) {
            h->has_bad = true;
            h->bad_off = r.error >> 3;
            h->bad_kind = (int)(r.error & 7) + gff::kFirstError;
            return fail(GFFX_E_INVALID, "GFF line at byte %llu: %s", (unsigned long long)h->bad_off, gff::status_name(h->bad_kind));
        }
        if (r.overflow) return fail(GFFX_E_INVALID, "gffx_hip_gff_feed: the strings of the lines that end in one 4 KiB tile total 4 GiB or more");
        const uint64_t rows = r.total[0], skips = r.total[5];
        if (h->n_rows + rows > kMaxRows) return fail(GFFX_E_INVALID, "gffx_hip_gff_feed: more than 2^30 feature rows");
        GFFX_HIP_TRY(grow_keep(h->line_off, h->n_rows, h->n_rows + rows));
        GFFX_HIP_TRY(grow_keep(h->start, h->n_rows, h->n_rows + rows));
        GFFX_HIP_TRY(grow_keep(h->end, h->n_rows, h->n_rows + rows));
        GFFX_HIP_TRY(grow_keep(h->flags, h->n_rows, h->n_rows + rows));
        GFFX_HIP_TRY(grow_keep(h->skipped, h->n_skipped, h->n_skipped + skips));
        for (int k = 0; k < 4; ++k) {
            GFFX_HIP_TRY(grow_keep(h->off[k], h->n_rows + 1, h->n_rows + rows + 1));
            GFFX_HIP_TRY(grow_keep(h->bytes[k], h->n_bytes[k], h->n_bytes[k] + r.total[k + 1] + ids::kPad));
        }
        O.line_off = h->line_off.p;
        O.start = h->start.p;
        O.end = h->end.p;
        O.flags = h->flags.p;
        O.skipped = h->skipped.p;
        O.row_base = h->n_rows;
        O.skip_base = h->n_skipped;
        O.row_cap = h->n_rows + rows;
        O.skip_cap = h->n_skipped + skips;
        for (int k = 0; k < 4; ++k) {
            O.bytes[k] = h->bytes[k].p;
            O.off[k] = h->off[k].p;
            O.base[k] = h->n_bytes[k];
            O.byte_cap[k] = h->n_bytes[k] + r.total[k + 1];
        }
        hipLaunchKernelGGL(k_gff_rows<1>, dim3(n_tiles), dim3(64), 0, s, D, (u64)h->d_file_off, h->line_base.p, h->nl.p, n_tiles, P, h->sums.p,
                           h->tile_base.p, O, h->res.p);
        GFFX_HIP_TRY(hipGetLastError());
        GFFX_HIP_TRY(hipEventRecord(h->ev[2], s));
        GFFX_HIP_TRY(hipStreamSynchronize(s));
        GFFX_HIP_TRY(h->add_ms(&h->ms[0], 0, 1));
        GFFX_HIP_TRY(h->add_ms(&h->ms[1], 1, 2));
        h->n_rows += rows;
        h->n_skipped += skips;
        for (int k = 0; k < 4; ++k) h->n_bytes[k] += r.total[k + 1];
        h->lines += n_lines;
        h->blank += r.blank;
        h->zero_end += r.zero_end;
    }
    // the unfinished line to the front of the other text buffer
    const uint64_t c = N - tail;
    const int nxt = 1 - h->cur;
    if (c) {
        GFFX_HIP_TRY(h->D[nxt].ensure(c + ids::kPad));
        GFFX_HIP_TRY(hipMemcpy(h->D[nxt].p, D + tail, c, hipMemcpyDeviceToDevice));
    }
    h->cur = nxt;
    h->carry = c;
    h->d_file_off += tail;
    return GFFX_OK;
}

int feed_text(gffx_hip_gff *h, const uint8_t *p, uint64_t n) {
    const uint64_t chunk = h->chunk_bytes;
    while (n) {
        if (h->pend.empty() && n >= chunk) {
            if (int rc = run_pass(h, p, chunk, 0)) return rc;
            p += chunk;
            n -= chunk;
            continue;
        }
        const uint64_t take = std::min<uint64_t>(n, chunk - h->pend.size());
        h->pend.insert(h->pend.end(), p, p + take);
        p += take;
        n -= take;
        if (h->pend.size() == chunk) {
            if (int rc = run_pass(h, h->pend.data(), chunk, 0)) return rc;
            h->pend.clear();
        }
    }
    return GFFX_OK;
}

// the numbering by first appearance of string kind k (root != NULL: over the root rows only): number[r], the names with a
// '\n' each in `names`, their count and bytes
int number_strings(gffx_hip_gff *h, int k, const uint32_t *root, uint32_t slots, DevArr<uint32_t> &number, DevArr<uint8_t> &names,
                   uint64_t *n_names, uint64_t *names_bytes) {
    hipStream_t s = h->stream;
    const uint32_t n = (uint32_t)h->n_rows, hm = ids::hash_mask_of(h->hash_bits);
    GFFX_HIP_TRY(number.ensure(std::max<uint32_t>(n, 1)));
    ids::launch_table_fill(s, h->slot.p, h->val.p, slots, ids::Keep::kSmallest);
    hipLaunchKernelGGL(k_gff_insert_min, grid256(n), dim3(256), 0, s, h->slot.p, h->val.p, h->bytes[k].p, h->off[k].p, root, n, slots - 1, hm);
    const ids::Table t{h->slot.p, h->val.p, h->bytes[k].p, h->off[k].p, slots - 1, hm};
    hipLaunchKernelGGL(k_gff_first, grid256(n), dim3(256), 0, s, t, root, n, h->first_row.p, h->is_first.p);
    launch_scan(s, h->is_first.p, n, h->rank.p, &h->res.p->total[0]);
    hipLaunchKernelGGL(k_gff_number, grid256(n), dim3(256), 0, s, h->first_row.p, h->rank.p, h->off[k].p, n, number.p, h->name_len.p);
    launch_scan(s, h->name_len.p, n, h->at.p, &h->res.p->total[1]);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipMemcpyAsync(h->res_host, h->res.p, sizeof(GffResult), hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    *n_names = h->res_host->total[0];
    *names_bytes = h->res_host->total[1];
    GFFX_HIP_TRY(names.ensure(std::max<uint64_t>(*names_bytes, 1)));
    hipLaunchKernelGGL(k_gff_name_put, grid256(n), dim3(256), 0, s, h->first_row.p, h->at.p, h->bytes[k].p, h->off[k].p, n, names.p,
                       (u64)*names_bytes);
    GFFX_HIP_TRY(hipGetLastError());
    return GFFX_OK;
}

int finish_steps(gffx_hip_gff *h) {
    hipStream_t s = h->stream;
    const uint32_t n = (uint32_t)h->n_rows;
    if (n == 0) return GFFX_OK;
    const uint32_t slots = ids::table_slots(n), hm = ids::hash_mask_of(h->hash_bits);
    GFFX_HIP_TRY(h->slot.ensure(slots));
    GFFX_HIP_TRY(h->val.ensure(slots));
    for (DevArr<uint32_t> *a : {&h->fid, &h->prt, &h->root, &h->first_row, &h->is_first, &h->name_len, &h->root_rows}) GFFX_HIP_TRY(a->ensure(n));
    GFFX_HIP_TRY(h->rank.ensure((size_t)n + 1));
    GFFX_HIP_TRY(h->at.ensure((size_t)n + 1));
    GFFX_HIP_TRY(h->fts.ensure(h->n_bytes[1] + n));
    // 1. the ID table, 2. the parents
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    ids::launch_table_build(s, h->slot.p, h->val.p, slots, h->bytes[1].p, h->off[1].p, n, hm);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    const ids::Table t{h->slot.p, h->val.p, h->bytes[1].p, h->off[1].p, slots - 1, hm};
    hipLaunchKernelGGL(k_gff_resolve, grid256(n), dim3(256), 0, s, t, h->bytes[2].p, h->off[2].p, n, h->fid.p, h->prt.p, h->root.p);
    hipLaunchKernelGGL(k_gff_fts, grid256(n), dim3(256), 0, s, h->bytes[1].p, h->off[1].p, n, h->fts.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[2], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    GFFX_HIP_TRY(h->add_ms(&h->ms[2], 0, 1));
    GFFX_HIP_TRY(h->add_ms(&h->ms[3], 1, 2));
    // 3. the numbering of the seqids (root rows) and of the attribute values, 4. the root list
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    if (int rc = number_strings(h, 0, h->root.p, slots, h->seq, h->sqs, &h->n_seqids, &h->sqs_bytes)) return rc;
    if (int rc = number_strings(h, 3, nullptr, slots, h->a2f, h->atn, &h->n_attrs, &h->atn_bytes)) return rc;
    launch_scan(s, h->root.p, n, h->at.p, &h->res.p->total[0]);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipMemcpyAsync(h->res_host, h->res.p, sizeof(GffResult), hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    h->n_roots = h->res_host->total[0];
    if (h->n_roots) {
        GFFX_HIP_TRY(h->gof.ensure(6 * h->n_roots));
        GFFX_HIP_TRY(h->roots.ensure(4 * h->n_roots));
        hipLaunchKernelGGL(k_gff_root_list, grid256(n), dim3(256), 0, s, h->root.p, h->at.p, n, h->root_rows.p, (u64)h->n_roots);
        hipLaunchKernelGGL(k_gff_gof, grid256(h->n_roots), dim3(256), 0, s, h->root_rows.p, (uint32_t)h->n_roots, h->fid.p, h->seq.p, h->line_off.p,
                           h->start.p, h->end.p, (u64)h->fed, h->gof.p, h->roots.p);
        GFFX_HIP_TRY(hipGetLastError());
    }
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    GFFX_HIP_TRY(h->add_ms(&h->ms[4], 0, 1));
    return GFFX_OK;
}

int ready(const gffx_hip_gff *h, const char *who) {
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    if (h->error) return fail(h->error, "%s", h->error_msg.c_str());
    if (!h->finished) return fail(GFFX_E_STATE, "%s: call gffx_hip_gff_finish first", who);
    return GFFX_OK;
}

template <class T>
int copy_out(const gffx_hip_gff *h, const char *who, const T *src, uint64_t n, T *dst) {
    if (int rc = ready(h, who)) return rc;
    if (n == 0) return GFFX_OK;
    if (!dst) return fail(GFFX_E_INVALID, "%s: the output is NULL", who);
    GFFX_HIP_TRY(hipSetDevice(h->device));
    GFFX_HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
    return GFFX_OK;
}

}  // namespace

extern "C" int gffx_hip_gff_create(int device, const char *attr_key, uint32_t n_skip, const char *skip /* concatenated */,
                                   const uint32_t *skip_off /* n_skip + 1 */, uint64_t chunk_bytes, int hash_bits, gffx_hip_gff **out) {
    if (!out) return fail(GFFX_E_INVALID, "gffx_hip_gff_create: out is NULL");
    *out = nullptr;
    if (!attr_key) return fail(GFFX_E_INVALID, "gffx_hip_gff_create: attr_key is NULL");
    if (n_skip && (!skip || !skip_off)) return fail(GFFX_E_INVALID, "gffx_hip_gff_create: skip or skip_off is NULL");
    for (uint32_t k = 0; k < n_skip; ++k)
        if (skip_off[k + 1] < skip_off[k]) return fail(GFFX_E_INVALID, "gffx_hip_gff_create: skip_off is not ascending at %u", k);
    if (hash_bits > 32) return fail(GFFX_E_INVALID, "gffx_hip_gff_create: hash_bits %d (at most 32)", hash_bits);
    const size_t key_len = std::strlen(attr_key);
    if (key_len > 0xFFFFFFu) return fail(GFFX_E_INVALID, "gffx_hip_gff_create: an attribute key of %zu bytes", key_len);
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_gff> h(new (std::nothrow) gffx_hip_gff);
    if (!h) return fail(GFFX_E_OOM, "gffx_hip_gff_create: out of host memory");
    h->device = device;
    h->hash_bits = hash_bits;
    h->chunk_bytes = std::min<uint64_t>(std::max<uint64_t>(chunk_bytes ? chunk_bytes : (64ull << 20), 1), 1ull << 30);
    GFFX_HIP_TRY(h->create_stream());
    GFFX_HIP_TRY(hipHostMalloc((void **)&h->res_host, sizeof(GffResult)));
    GFFX_HIP_TRY(h->res.ensure(1));
    h->key_len = (uint32_t)key_len;
    GFFX_HIP_TRY(h->key.ensure(std::max<size_t>(key_len, 1)));
    if (key_len) GFFX_HIP_TRY(hipMemcpy(h->key.p, attr_key, key_len, hipMemcpyHostToDevice));
    h->n_skip = n_skip;
    const uint32_t skip_n_bytes = n_skip ? skip_off[n_skip] : 0;
    GFFX_HIP_TRY(h->skip_bytes.ensure(std::max<uint32_t>(skip_n_bytes, 1)));
    GFFX_HIP_TRY(h->skip_off.ensure((size_t)n_skip + 1));
    if (skip_n_bytes) GFFX_HIP_TRY(hipMemcpy(h->skip_bytes.p, skip, skip_n_bytes, hipMemcpyHostToDevice));
    if (n_skip) {
        GFFX_HIP_TRY(hipMemcpy(h->skip_off.p, skip_off, ((size_t)n_skip + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    } else {
        GFFX_HIP_TRY(hipMemset(h->skip_off.p, 0, sizeof(uint32_t)));
    }
    for (int k = 0; k < 4; ++k) {  // off[k][0] = 0
        GFFX_HIP_TRY(h->off[k].ensure(1));
        GFFX_HIP_TRY(hipMemset(h->off[k].p, 0, sizeof(u64)));
    }
    *out = h.release();
    return GFFX_OK;
}

extern "C" int gffx_hip_gff_feed(gffx_hip_gff *h, const uint8_t *bytes, uint64_t n_bytes) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_gff_feed: NULL handle");
    if (h->error) return fail(h->error, "%s", h->error_msg.c_str());
    if (h->finished) return fail(GFFX_E_STATE, "gffx_hip_gff_feed: the handle is finished");
    if (n_bytes && !bytes) return fail(GFFX_E_INVALID, "gffx_hip_gff_feed: NULL input");
    GFFX_HIP_TRY(hipSetDevice(h->device));
    h->fed += n_bytes;
    return h->sticky(feed_text(h, bytes, n_bytes));
}

extern "C" int gffx_hip_gff_finish(gffx_hip_gff *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_gff_finish: NULL handle");
    if (h->error) return fail(h->error, "%s", h->error_msg.c_str());
    if (h->finished) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    if (!h->pend.empty()) {
        if (int rc = run_pass(h, h->pend.data(), h->pend.size(), 0)) return h->sticky(rc);
        h->pend.clear();
    }
    if (h->carry)  // a last line without '\n'
        if (int rc = run_pass(h, nullptr, 0, 1)) return h->sticky(rc);
    if (int rc = finish_steps(h)) return h->sticky(rc);
    h->finished = true;
    return GFFX_OK;
}

extern "C" int gffx_hip_gff_error(const gffx_hip_gff *h, uint64_t *line_offset, int *kind) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_gff_error: NULL handle");
    if (line_offset) *line_offset = h->has_bad ? h->bad_off : 0;
    if (kind) *kind = h->has_bad ? h->bad_kind : 0;
    return GFFX_OK;
}

extern "C" int gffx_hip_gff_counts(const gffx_hip_gff *h, uint64_t *lines, uint64_t *blank, uint64_t *skipped_type, uint64_t *zero_end,
                                   uint64_t *rows, uint64_t *roots, uint64_t *seqids, uint64_t *attr_values) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_gff_counts: NULL handle");
    if (lines) *lines = h->lines;
    if (blank) *blank = h->blank;
    if (skipped_type) *skipped_type = h->n_skipped;
    if (zero_end) *zero_end = h->zero_end;
    if (rows) *rows = h->n_rows;
    if (roots) *roots = h->n_roots;
    if (seqids) *seqids = h->n_seqids;
    if (attr_values) *attr_values = h->n_attrs;
    return GFFX_OK;
}

extern "C" int gffx_hip_gff_stage_ms(const gffx_hip_gff *h, double *scan_ms, double *rows_ms, double *table_ms, double *resolve_ms,
                                     double *number_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_gff_stage_ms: NULL handle");
    double *out[5] = {scan_ms, rows_ms, table_ms, resolve_ms, number_ms};
    for (int k = 0; k < 5; ++k)
        if (out[k]) *out[k] = h->ms[k];
    return GFFX_OK;
}

// the size queries: 0 on a handle that is not finished or has failed
extern "C" uint64_t gffx_hip_gff_n_rows(const gffx_hip_gff *h) { return h && h->finished && !h->error ? h->n_rows : 0; }
extern "C" uint64_t gffx_hip_gff_n_roots(const gffx_hip_gff *h) { return h && h->finished && !h->error ? h->n_roots : 0; }
extern "C" uint64_t gffx_hip_gff_fts_bytes(const gffx_hip_gff *h) { return h && h->finished && !h->error ? h->n_bytes[1] + h->n_rows : 0; }
extern "C" uint64_t gffx_hip_gff_atn_bytes(const gffx_hip_gff *h) { return h && h->finished && !h->error ? h->atn_bytes : 0; }
extern "C" uint64_t gffx_hip_gff_seqids_bytes(const gffx_hip_gff *h) { return h && h->finished && !h->error ? h->sqs_bytes : 0; }
extern "C" uint64_t gffx_hip_gff_n_skipped_lines(const gffx_hip_gff *h) { return h && h->finished && !h->error ? h->n_skipped : 0; }
extern "C" uint64_t gffx_hip_gff_n_warn_rows(const gffx_hip_gff *h) {
    if (!h || !h->finished || h->error || h->n_rows == 0) return 0;
    std::vector<uint32_t> f(h->n_rows);
    if (hipSetDevice(h->device) != hipSuccess || hipMemcpy(f.data(), h->flags.p, h->n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return 0;
    uint64_t n = 0;
    for (uint32_t x : f) n += x & 1u;
    return n;
}

extern "C" int gffx_hip_gff_copy_fts(const gffx_hip_gff *h, uint8_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_fts", h ? h->fts.p : nullptr, gffx_hip_gff_fts_bytes(h), out);
}
extern "C" int gffx_hip_gff_copy_fid(const gffx_hip_gff *h, uint32_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_fid", h ? h->fid.p : nullptr, gffx_hip_gff_n_rows(h), out);
}
extern "C" int gffx_hip_gff_copy_prt(const gffx_hip_gff *h, uint32_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_prt", h ? h->prt.p : nullptr, gffx_hip_gff_n_rows(h), out);
}
extern "C" int gffx_hip_gff_copy_a2f(const gffx_hip_gff *h, uint32_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_a2f", h ? h->a2f.p : nullptr, gffx_hip_gff_n_rows(h), out);
}
extern "C" int gffx_hip_gff_copy_atn(const gffx_hip_gff *h, uint8_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_atn", h ? h->atn.p : nullptr, gffx_hip_gff_atn_bytes(h), out);
}
extern "C" int gffx_hip_gff_copy_seqids(const gffx_hip_gff *h, uint8_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_seqids", h ? h->sqs.p : nullptr, gffx_hip_gff_seqids_bytes(h), out);
}
extern "C" int gffx_hip_gff_copy_gof(const gffx_hip_gff *h, uint8_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_gof", h ? reinterpret_cast<const uint8_t *>(h->gof.p) : nullptr, 24 * gffx_hip_gff_n_roots(h), out);
}
extern "C" int gffx_hip_gff_copy_roots(const gffx_hip_gff *h, uint32_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_roots", h ? h->roots.p : nullptr, 4 * gffx_hip_gff_n_roots(h), out);
}
extern "C" int gffx_hip_gff_copy_skipped_lines(const gffx_hip_gff *h, uint64_t *out) {
    return copy_out(h, "gffx_hip_gff_copy_skipped_lines", h ? reinterpret_cast<const uint64_t *>(h->skipped.p) : nullptr,
                    gffx_hip_gff_n_skipped_lines(h), out);
}
extern "C" int gffx_hip_gff_copy_warn_rows(const gffx_hip_gff *h, uint32_t *out) {
    if (int rc = ready(h, "gffx_hip_gff_copy_warn_rows")) return rc;
    if (h->n_rows == 0) return GFFX_OK;
    std::vector<uint32_t> f(h->n_rows);
    GFFX_HIP_TRY(hipSetDevice(h->device));
    GFFX_HIP_TRY(hipMemcpy(f.data(), h->flags.p, h->n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (uint64_t r = 0; r < h->n_rows; ++r)
        if (f[r] & 1u) {
            if (!out) return fail(GFFX_E_INVALID, "gffx_hip_gff_copy_warn_rows: the output is NULL");
            out[n++] = (uint32_t)r;
        }
    return GFFX_OK;
}

extern "C" void gffx_hip_gff_destroy(gffx_hip_gff *h) { delete h; }
