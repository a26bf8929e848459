// ids.hip -- `gffx extract` on the device: the feature-ID table of `.fts`, the lookup of requested names with the parent
// chase through `.prt`, and the per-line ID filter of the hit blocks (reference: commands/extract.rs:37-162,
// index_loader/fts.rs:16-31, index_loader/prt.rs:54-72, utils/common.rs:289-465).  The rules of one name, one chase and one
// line are ids_core.hpp's, shared with the host.
//
//   k_table_insert one thread per `.fts` line f (string_table.hpp): val ends as the LARGEST fid of the string (the last `.fts`
//                  line wins, fts.rs:16-22) whatever the order the threads ran in.
//   k_ids_resolve  one thread per query name: table_find, chase_root, one atomicOr into the requested-fid bitmap and one into
//                  the root bitmap (both stay in the handle and accumulate until _reset).
//   k_ids_roots    one thread per fid: fid_root[f] = chase_root(f).  Run once per handle, when the filter is first used.
//   k_ids_filter   one thread per line of a chunk: keep_line.
//
// LANE SHARING in k_ids_filter: one lane per line, and the lane runs keep_line() as the host does, for the reason sam.hip
// gives for k_sam_rows: one code path for a 60-byte line and a 1 MB line, the one tools/extract_check.cpp runs under the
// sanitizers.  The lines of a wave are adjacent in the chunk, so the byte loads of a lane hit cache lines its neighbours pull
// in too; the loads are not coalesced and one long line keeps 63 lanes idle.  HYPOTHESIS until measured
// (tools/extract_bench.py): the pass is bound by the serial walk to the eighth TAB, not by memory.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "engine_private.hpp"
#include "string_table.hpp"
#include "table_handle.hpp"

namespace gffx {

using ids::kNone;

__global__ __launch_bounds__(256) void k_ids_resolve(ids::Table t, const uint32_t *prt, uint32_t n_prt, const uint8_t *q, const u64 *q_off,
                                                     u64 nq, uint32_t *fid_out, uint32_t *root_out, uint32_t *requested,
                                                     uint32_t *root_bits) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= nq) return;
    const u64 a = q_off[i];
    const uint32_t f = ids::table_find(t, q + a, q_off[i + 1] - a);
    uint32_t r = kNone;
    if (f != kNone) {
        atomicOr(&requested[f >> 5], 1u << (f & 31));
        r = ids::chase_root(prt, n_prt, f);
        if (r != kNone) atomicOr(&root_bits[r >> 5], 1u << (r & 31));
    }
    fid_out[i] = f;
    root_out[i] = r;
}

__global__ __launch_bounds__(256) void k_ids_roots(const uint32_t *prt, uint32_t n_prt, uint32_t n, uint32_t *fid_root) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < n) fid_root[f] = ids::chase_root(prt, n_prt, f);
}

__global__ __launch_bounds__(64) void k_ids_filter(ids::Table t, const uint32_t *requested, const uint32_t *fid_root, ids::Types types,
                                                   const uint8_t *text, const u64 *line_off, const uint32_t *line_root, u64 n_lines,
                                                   uint8_t *keep) {
    const u64 i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n_lines) return;
    const u64 a = line_off[i];
    const uint8_t key[2] = {'I', 'D'};  // extract.rs:142
    keep[i] = ids::keep_line(t, requested, fid_root, types, key, 2, text + a, line_off[i + 1] - a, line_root[i]) ? 1 : 0;
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_ids : StreamEvents<2> {
    int device = 0;
    int hash_bits = 32;
    uint32_t n = 0, n_prt = 0;  // `.fts` lines; `.prt` words
    uint32_t n_bits = 0;        // max(n, n_prt): bits of either bitmap
    ids::StringTable names;
    LineChunk lines;
    DevArr<u64> q_off;
    DevArr<uint32_t> prt, requested, root_bits, fid_root, q_fid, q_root;
    DevArr<uint8_t> q;
    bool have_fid_root = false;
    double ms[3] = {0, 0, 0};  // table build, resolve, line filter (HIP events; a failing read of the events adds nothing)

    uint64_t bitmap_words32() const { return 2 * (((uint64_t)n_bits + 63) / 64); }
};

namespace {
int clear_bitmaps(gffx_hip_ids *h) {
    GFFX_HIP_TRY(hipMemsetAsync(h->requested.p, 0, h->bitmap_words32() * 4, h->stream));
    GFFX_HIP_TRY(hipMemsetAsync(h->root_bits.p, 0, h->bitmap_words32() * 4, h->stream));
    return GFFX_OK;
}
}  // namespace

extern "C" int gffx_hip_ids_create(int device, uint64_t n_names, const uint8_t *names, const uint64_t *name_off, uint64_t n_prt,
                                   const uint32_t *prt, int hash_bits, gffx_hip_ids **out) {
    static const char *who = "gffx_hip_ids_create";
    if (!out) return fail(GFFX_E_INVALID, "%s: out is NULL", who);
    *out = nullptr;
    if (n_names && !name_off) return fail(GFFX_E_INVALID, "%s: name_off is NULL", who);
    if (n_prt && !prt) return fail(GFFX_E_INVALID, "%s: prt is NULL", who);
    if (n_names > (1ull << 28) || n_prt > (1ull << 28))
        return fail(GFFX_E_INVALID, "%s: %llu names, %llu parent words (at most 2^28 each)", who, (unsigned long long)n_names,
                    (unsigned long long)n_prt);
    if (hash_bits > 32) return fail(GFFX_E_INVALID, "%s: hash_bits %d (0 to 32; negative: all 32)", who, hash_bits);
    uint64_t n_bytes = 0;
    if (int rc = check_offsets(who, "name_off", name_off, n_names, &n_bytes)) return rc;
    if (n_bytes && !names) return fail(GFFX_E_INVALID, "%s: names is NULL", who);
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_ids> h(new (std::nothrow) gffx_hip_ids);
    if (!h) return fail(GFFX_E_OOM, "%s: out of host memory", who);
    h->device = device;
    h->hash_bits = hash_bits < 0 ? 32 : hash_bits;
    h->n = (uint32_t)n_names;
    h->n_prt = (uint32_t)n_prt;
    h->n_bits = std::max(h->n, h->n_prt);
    GFFX_HIP_TRY(h->create_stream());
    GFFX_HIP_TRY(h->prt.ensure(std::max<uint64_t>(n_prt, 1)));
    GFFX_HIP_TRY(h->requested.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    GFFX_HIP_TRY(h->root_bits.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    hipStream_t s = h->stream;
    if (n_prt) GFFX_HIP_TRY(hipMemcpyAsync(h->prt.p, prt, n_prt * 4, hipMemcpyHostToDevice, s));
    if (int rc = clear_bitmaps(h.get())) return rc;
    if (int rc = h->names.build(s, n_names, names, name_off, ids::hash_mask_of(h->hash_bits), h->ev[0])) return rc;
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));  // (the caller's arrays have been read)
    (void)h->add_ms(&h->ms[0]);
    *out = h.release();
    return GFFX_OK;
}

extern "C" void gffx_hip_ids_destroy(gffx_hip_ids *h) { delete h; }

extern "C" uint64_t gffx_hip_ids_n(const gffx_hip_ids *h) { return h ? h->n : 0; }

extern "C" int gffx_hip_ids_options(const gffx_hip_ids *h, char *buf, size_t cap) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_ids_options: NULL handle");
    return copy_out(h->hash_bits == 32 ? std::string("{}") : "{\"hash_bits\": " + std::to_string(h->hash_bits) + "}", buf, cap);
}

extern "C" int gffx_hip_ids_resolve(gffx_hip_ids *h, uint64_t nq, const uint8_t *names, const uint64_t *name_off, uint32_t *fid_out,
                                    uint32_t *root_out) {
    static const char *who = "gffx_hip_ids_resolve";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    if (nq && (!name_off || !fid_out || !root_out)) return fail(GFFX_E_INVALID, "%s: name_off, fid_out or root_out is NULL", who);
    if (nq > (1ull << 32)) return fail(GFFX_E_INVALID, "%s: %llu names in one call (at most 2^32)", who, (unsigned long long)nq);
    uint64_t n_bytes = 0;
    if (int rc = check_offsets(who, "name_off", name_off, nq, &n_bytes)) return rc;
    if (n_bytes && !names) return fail(GFFX_E_INVALID, "%s: names is NULL", who);
    if (!nq) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    GFFX_HIP_TRY(h->q.ensure(n_bytes + ids::kPad));
    GFFX_HIP_TRY(h->q_off.ensure(nq + 1));
    GFFX_HIP_TRY(h->q_fid.ensure(nq));
    GFFX_HIP_TRY(h->q_root.ensure(nq));
    hipStream_t s = h->stream;
    if (n_bytes) GFFX_HIP_TRY(hipMemcpyAsync(h->q.p, names, n_bytes, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->q_off.p, name_off, (nq + 1) * 8, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_ids_resolve, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, h->names.table(), h->prt.p, h->n_prt, h->q.p, h->q_off.p,
                       (u64)nq, h->q_fid.p, h->q_root.p, h->requested.p, h->root_bits.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipMemcpyAsync(fid_out, h->q_fid.p, nq * 4, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipMemcpyAsync(root_out, h->q_root.p, nq * 4, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    (void)h->add_ms(&h->ms[1]);
    return GFFX_OK;
}

extern "C" int gffx_hip_ids_reset(gffx_hip_ids *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_ids_reset: NULL handle");
    GFFX_HIP_TRY(hipSetDevice(h->device));
    if (int rc = clear_bitmaps(h)) return rc;
    GFFX_HIP_TRY(hipStreamSynchronize(h->stream));
    return GFFX_OK;
}

extern "C" int gffx_hip_ids_copy_root_bitmap(gffx_hip_ids *h, uint64_t *host, uint64_t n_words) {
    static const char *who = "gffx_hip_ids_copy_root_bitmap";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    return copy_bitmap(who, h->device, h->stream, h->root_bits.p, h->bitmap_words32() / 2, host, n_words);
}

extern "C" int gffx_hip_ids_copy_requested_bitmap(gffx_hip_ids *h, uint64_t *host, uint64_t n_words) {
    static const char *who = "gffx_hip_ids_copy_requested_bitmap";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    return copy_bitmap(who, h->device, h->stream, h->requested.p, h->bitmap_words32() / 2, host, n_words);
}

extern "C" int gffx_hip_ids_filter_lines(gffx_hip_ids *h, const uint8_t *text, uint64_t n_bytes, uint64_t n_lines, const uint64_t *line_off,
                                         const uint32_t *line_root, int by_type, uint32_t n_types, const uint8_t *types,
                                         const uint32_t *type_off, uint8_t *keep_out) {
    static const char *who = "gffx_hip_ids_filter_lines";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    const LineArgs a{text, n_bytes, n_lines, line_off, line_root, by_type, n_types, types, type_off, keep_out};
    if (int rc = LineChunk::check(who, a)) return rc;
    if (!n_lines) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (!h->have_fid_root) {  // once per handle
        GFFX_HIP_TRY(h->fid_root.ensure(std::max<uint32_t>(h->n, 1)));
        if (h->n) hipLaunchKernelGGL(k_ids_roots, dim3((h->n + 255) / 256), dim3(256), 0, s, h->prt.p, h->n_prt, h->n, h->fid_root.p);
        GFFX_HIP_TRY(hipGetLastError());
        h->have_fid_root = true;
    }
    ids::Types ty;
    if (int rc = h->lines.upload(s, a, &ty)) return rc;
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_ids_filter, dim3((unsigned)((n_lines + 63) / 64)), dim3(64), 0, s, h->names.table(), h->requested.p, h->fid_root.p, ty,
                       h->lines.text.p, h->lines.line_off.p, h->lines.line_root.p, (u64)n_lines, h->lines.keep.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    if (int rc = h->lines.download(s, a)) return rc;
    (void)h->add_ms(&h->ms[2]);
    return GFFX_OK;
}

extern "C" int gffx_hip_ids_stage_ms(const gffx_hip_ids *h, double *build_ms, double *resolve_ms, double *filter_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_ids_stage_ms: NULL handle");
    if (build_ms) *build_ms = h->ms[0];
    if (resolve_ms) *resolve_ms = h->ms[1];
    if (filter_ms) *filter_ms = h->ms[2];
    return GFFX_OK;
}
