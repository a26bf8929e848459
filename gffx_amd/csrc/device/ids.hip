// ids.hip -- `gffx extract` on the device: the feature-ID table of `.fts`, the lookup of requested names with the parent
// chase through `.prt`, and the per-line ID filter of the hit blocks (reference: commands/extract.rs:37-162,
// index_loader/fts.rs:16-31, index_loader/prt.rs:54-72, utils/common.rs:289-465).  The rules of one name, one chase and one
// line are ids_core.hpp's, shared with the host.
//
//   k_ids_insert   one thread per `.fts` line f: hash, probe from the hash's slot.  An empty slot is claimed with ONE 64-bit
//                  compare-and-swap of (hash << 32) | f -- whoever wins, the slot's name is that thread's string from then on
//                  --; a slot whose hash and string equal the thread's takes atomicMax(val, f).  So val ends as the LARGEST fid
//                  of the string (the last `.fts` line wins, fts.rs:16-22) whatever the order the threads ran in, and since
//                  names only enter the table a lookup finds every name whatever slot of its chain it got.  Contention: the
//                  slots are 2 n or more and the hash spreads the names, so the returning atomic of a thread meets another
//                  thread's only for equal strings (CDS rows that share an ID) and colliding names; the atomicMax returns
//                  nothing.  Under hash_bits < 32 (a test hook) the chains are long on purpose.
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

#include "bgzf_device.hpp"
#include "engine_private.hpp"
#include "ids_core.hpp"
#include "ids_insert_device.hpp"

namespace gffx {

using ids::kNone;

__global__ __launch_bounds__(256) void k_ids_fill(u64 *slot, uint32_t *val, uint32_t slots) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < slots) ids::table_clear_one(slot, val, i);
}

__global__ __launch_bounds__(256) void k_ids_insert(u64 *slot, uint32_t *val, const uint8_t *bytes, const u64 *off, uint32_t n,
                                                    uint32_t mask, uint32_t hash_mask) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < n) ids::table_insert_one(slot, val, bytes, off, f, mask, hash_mask);
}

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

struct gffx_hip_ids {
    int device = 0;
    int hash_bits = 32;
    uint32_t n = 0, n_prt = 0;  // `.fts` lines; `.prt` words
    uint32_t n_bits = 0;        // max(n, n_prt): bits of either bitmap
    uint32_t mask = 0, hash_mask = 0xFFFFFFFFu;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    DevArr<u64> slot, off, q_off, line_off;
    DevArr<uint32_t> val, prt, requested, root_bits, fid_root, q_fid, q_root, line_root, type_off;
    DevArr<uint8_t> bytes, q, text, type_bytes, keep;
    bool have_fid_root = false;
    double ms[3] = {0, 0, 0};  // table build, resolve, line filter (HIP events)

    ids::Table table() const { return ids::Table{slot.p, val.p, bytes.p, off.p, mask, hash_mask}; }
    uint64_t bitmap_words32() const { return 2 * (((uint64_t)n_bits + 63) / 64); }

    ~gffx_hip_ids() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {
// offsets ascending from 0?  (what every kernel's reads are bounded by)
int check_offsets(const char *who, const char *what, const uint64_t *off, uint64_t n, uint64_t *total) {
    *total = 0;
    if (!n) return GFFX_OK;
    if (off[0] != 0) return fail(GFFX_E_INVALID, "%s: %s[0] is not 0", who, what);
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(GFFX_E_INVALID, "%s: %s is not ascending at %llu", who, what, (unsigned long long)i);
    *total = off[n];
    return GFFX_OK;
}

// elapsed time of the kernels between ev[0] and ev[1] (recorded on h->stream, which has been synchronised) into ms[k]
void add_ms(gffx_hip_ids *h, int k) {
    float t = 0;
    if (hipEventElapsedTime(&t, h->ev[0], h->ev[1]) == hipSuccess) h->ms[k] += t;
}

int clear_bitmaps(gffx_hip_ids *h) {
    GFFX_HIP_TRY(hipMemsetAsync(h->requested.p, 0, h->bitmap_words32() * 4, h->stream));
    GFFX_HIP_TRY(hipMemsetAsync(h->root_bits.p, 0, h->bitmap_words32() * 4, h->stream));
    return GFFX_OK;
}

int copy_bitmap(gffx_hip_ids *h, const uint32_t *d, uint64_t *host, uint64_t n_words, const char *who) {
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    const uint64_t need = h->bitmap_words32() / 2;
    if (n_words < need) return fail(GFFX_E_INVALID, "%s: %llu words given, %llu needed", who, (unsigned long long)n_words, (unsigned long long)need);
    if (need && !host) return fail(GFFX_E_INVALID, "%s: host is NULL", who);
    GFFX_HIP_TRY(hipSetDevice(h->device));
    GFFX_HIP_TRY(hipStreamSynchronize(h->stream));
    if (need) GFFX_HIP_TRY(hipMemcpy(host, d, need * 8, hipMemcpyDeviceToHost));
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
    h->hash_mask = ids::hash_mask_of(h->hash_bits);
    h->n = (uint32_t)n_names;
    h->n_prt = (uint32_t)n_prt;
    h->n_bits = std::max(h->n, h->n_prt);
    const uint32_t slots = ids::table_slots(n_names);
    h->mask = slots - 1;
    GFFX_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev) GFFX_HIP_TRY(hipEventCreate(&e));
    GFFX_HIP_TRY(h->slot.ensure(slots));
    GFFX_HIP_TRY(h->val.ensure(slots));
    GFFX_HIP_TRY(h->bytes.ensure(n_bytes + ids::kPad));
    GFFX_HIP_TRY(h->off.ensure(n_names + 1));
    GFFX_HIP_TRY(h->prt.ensure(std::max<uint64_t>(n_prt, 1)));
    GFFX_HIP_TRY(h->requested.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    GFFX_HIP_TRY(h->root_bits.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    hipStream_t s = h->stream;
    GFFX_HIP_TRY(hipMemsetAsync(h->bytes.p + n_bytes, 0, ids::kPad, s));
    if (n_bytes) GFFX_HIP_TRY(hipMemcpyAsync(h->bytes.p, names, n_bytes, hipMemcpyHostToDevice, s));
    if (n_names) {
        GFFX_HIP_TRY(hipMemcpyAsync(h->off.p, name_off, (n_names + 1) * 8, hipMemcpyHostToDevice, s));
    } else {
        GFFX_HIP_TRY(hipMemsetAsync(h->off.p, 0, 8, s));
    }
    if (n_prt) GFFX_HIP_TRY(hipMemcpyAsync(h->prt.p, prt, n_prt * 4, hipMemcpyHostToDevice, s));
    if (int rc = clear_bitmaps(h.get())) return rc;
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_ids_fill, dim3((slots + 255) / 256), dim3(256), 0, s, h->slot.p, h->val.p, slots);
    if (h->n)
        hipLaunchKernelGGL(k_ids_insert, dim3((h->n + 255) / 256), dim3(256), 0, s, h->slot.p, h->val.p, h->bytes.p, h->off.p, h->n, h->mask,
                           h->hash_mask);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));  // (the caller's arrays have been read)
    add_ms(h.get(), 0);
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
    hipLaunchKernelGGL(k_ids_resolve, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, h->table(), h->prt.p, h->n_prt, h->q.p, h->q_off.p,
                       (u64)nq, h->q_fid.p, h->q_root.p, h->requested.p, h->root_bits.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipMemcpyAsync(fid_out, h->q_fid.p, nq * 4, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipMemcpyAsync(root_out, h->q_root.p, nq * 4, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    add_ms(h, 1);
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
    return copy_bitmap(h, h ? h->root_bits.p : nullptr, host, n_words, "gffx_hip_ids_copy_root_bitmap");
}

extern "C" int gffx_hip_ids_copy_requested_bitmap(gffx_hip_ids *h, uint64_t *host, uint64_t n_words) {
    return copy_bitmap(h, h ? h->requested.p : nullptr, host, n_words, "gffx_hip_ids_copy_requested_bitmap");
}

extern "C" int gffx_hip_ids_filter_lines(gffx_hip_ids *h, const uint8_t *text, uint64_t n_bytes, uint64_t n_lines, const uint64_t *line_off,
                                         const uint32_t *line_root, int by_type, uint32_t n_types, const uint8_t *types,
                                         const uint32_t *type_off, uint8_t *keep_out) {
    static const char *who = "gffx_hip_ids_filter_lines";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    if (n_lines && (!line_off || !line_root || !keep_out)) return fail(GFFX_E_INVALID, "%s: line_off, line_root or keep_out is NULL", who);
    if (n_lines > (1ull << 32)) return fail(GFFX_E_INVALID, "%s: %llu lines in one call (at most 2^32)", who, (unsigned long long)n_lines);
    uint64_t end = 0;
    if (int rc = check_offsets(who, "line_off", line_off, n_lines, &end)) return rc;
    if (end > n_bytes) return fail(GFFX_E_INVALID, "%s: the last line ends at %llu, the text has %llu bytes", who, (unsigned long long)end,
                                   (unsigned long long)n_bytes);
    if (n_bytes && !text) return fail(GFFX_E_INVALID, "%s: text is NULL", who);
    uint32_t type_bytes = 0;
    if (n_types) {
        if (!type_off) return fail(GFFX_E_INVALID, "%s: type_off is NULL", who);
        if (n_types > 65536) return fail(GFFX_E_INVALID, "%s: %u type names (at most 65536)", who, n_types);
        if (type_off[0] != 0) return fail(GFFX_E_INVALID, "%s: type_off[0] is not 0", who);
        for (uint32_t k = 0; k < n_types; ++k)
            if (type_off[k + 1] < type_off[k]) return fail(GFFX_E_INVALID, "%s: type_off is not ascending at %u", who, k);
        type_bytes = type_off[n_types];
        if (type_bytes && !types) return fail(GFFX_E_INVALID, "%s: types is NULL", who);
    }
    if (!n_lines) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (!h->have_fid_root) {  // once per handle
        GFFX_HIP_TRY(h->fid_root.ensure(std::max<uint32_t>(h->n, 1)));
        if (h->n) hipLaunchKernelGGL(k_ids_roots, dim3((h->n + 255) / 256), dim3(256), 0, s, h->prt.p, h->n_prt, h->n, h->fid_root.p);
        GFFX_HIP_TRY(hipGetLastError());
        h->have_fid_root = true;
    }
    GFFX_HIP_TRY(h->text.ensure(n_bytes + ids::kPad));
    GFFX_HIP_TRY(h->line_off.ensure(n_lines + 1));
    GFFX_HIP_TRY(h->line_root.ensure(n_lines));
    GFFX_HIP_TRY(h->keep.ensure(n_lines));
    GFFX_HIP_TRY(h->type_bytes.ensure(std::max<uint32_t>(type_bytes, 1)));
    GFFX_HIP_TRY(h->type_off.ensure(n_types + 1));
    if (n_bytes) GFFX_HIP_TRY(hipMemcpyAsync(h->text.p, text, n_bytes, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->line_off.p, line_off, (n_lines + 1) * 8, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->line_root.p, line_root, n_lines * 4, hipMemcpyHostToDevice, s));
    if (type_bytes) GFFX_HIP_TRY(hipMemcpyAsync(h->type_bytes.p, types, type_bytes, hipMemcpyHostToDevice, s));
    if (n_types) GFFX_HIP_TRY(hipMemcpyAsync(h->type_off.p, type_off, (n_types + 1) * 4, hipMemcpyHostToDevice, s));
    const ids::Types ty{h->type_bytes.p, h->type_off.p, n_types, by_type || n_types ? 1 : 0};
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_ids_filter, dim3((unsigned)((n_lines + 63) / 64)), dim3(64), 0, s, h->table(), h->requested.p, h->fid_root.p, ty, h->text.p,
                       h->line_off.p, h->line_root.p, (u64)n_lines, h->keep.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipMemcpyAsync(keep_out, h->keep.p, n_lines, hipMemcpyDeviceToHost, s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    add_ms(h, 2);
    return GFFX_OK;
}

extern "C" int gffx_hip_ids_stage_ms(const gffx_hip_ids *h, double *build_ms, double *resolve_ms, double *filter_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_ids_stage_ms: NULL handle");
    if (build_ms) *build_ms = h->ms[0];
    if (resolve_ms) *resolve_ms = h->ms[1];
    if (filter_ms) *filter_ms = h->ms[2];
    return GFFX_OK;
}
