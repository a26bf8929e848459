// search.hip -- `gffx search` on the device: the attribute values of `.atn` matched against a list of wanted strings or
// against the DFAs of a regex list, the matched aids resolved through `.a2f` and `.prt` to fids, roots and the
// (value class, root) pair set, and the per-line value filter of the hit blocks (reference: commands/search.rs:55-252,
// index_loader/a2f.rs:77-113, index_loader/prt.rs:54-72, utils/common.rs:289-465).  The rules of one value, one chase and
// one line are search_core.hpp's and ids_core.hpp's, shared with the host.
//
//   k_table_insert      the string table (string_table.hpp) over the `.atn` values, once per handle, and over the wanted
//                       strings of every exact match.
//   k_attr_classes      one thread per aid: class[aid] = the largest aid with the same string (table_find on the value table).
//   k_attr_match_exact  one thread per aid: the value is looked up in the table of the wanted strings; every aid of a
//                       wanted string matches (search.rs:105-110).  One atomicOr into the matched bitmap per match.
//   k_attr_match_dfa    one thread per aid walks the DFA over the value's bytes and the end-of-text symbol.  <true>: the
//                       class map and the transitions are staged in LDS by the block first (256 + 2 x states x classes
//                       bytes, taken when that is at most kLdsBudget); <false>: they are read from global memory.  One
//                       launch per pattern group, ORed into the same bitmap.
//   k_attr_resolve      one thread per fid (`.a2f` word): when its aid is matched, the fid bit, the bounded chase, the root
//                       bit or the invalid bit, and (class, root) into the pair set -- one 64-bit compare-and-swap on an
//                       empty slot of an open-addressing table of >= 2 x n_fids slots.
//   k_attr_filter       one thread per line of a chunk: keep_line_value.
//
// LANE SHARING: one lane per value / per line, as ids.hip's filter and for its reason: one code path for a 6-byte gene name
// and a 1 MB value, the one tools/search_check.cpp runs under the sanitizers.  The values of a wave are adjacent in the
// table, so the byte loads of a lane hit cache lines its neighbours pull in too; they are not coalesced, and a wave runs as
// long as its longest value.  HYPOTHESIS, not measured: at gene-name lengths the DFA walk is bound by the dependent LDS
// read per byte, not by memory.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "engine_private.hpp"
#include "search_core.hpp"
#include "string_table.hpp"
#include "table_handle.hpp"

namespace gffx {

using ids::kNone;

constexpr uint32_t kLdsBudget = 65536;  // bytes of LDS a block of k_attr_match_dfa<true> may take

__global__ __launch_bounds__(256) void k_attr_classes(ids::Table values, uint32_t n, uint32_t *cls) {
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= n) return;
    const u64 s = values.off[a];
    cls[a] = ids::table_find(values, values.bytes + s, values.off[a + 1] - s);
}

__global__ __launch_bounds__(256) void k_attr_match_exact(ids::Table wanted, const uint8_t *bytes, const u64 *off, uint32_t n,
                                                          uint32_t *matched) {
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= n) return;
    const u64 s = off[a];
    if (ids::table_find(wanted, bytes + s, off[a + 1] - s) != kNone) atomicOr(&matched[a >> 5], 1u << (a & 31));
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_attr_match_dfa(search::Dfa d, const uint8_t *bytes, const u64 *off, uint32_t n, uint32_t *matched) {
    extern __shared__ __align__(16) uint8_t lds[];
    if (kLds) {
        // cls at [0, 256), the transitions behind it; trans_words = n_states * n_classes <= (kLdsBudget - 256) / 2 (checked by the host)
        const uint32_t trans_words = d.n_states * d.n_classes;
        uint16_t *t = reinterpret_cast<uint16_t *>(lds + 256);
        for (uint32_t i = threadIdx.x; i < 256; i += 256) lds[i] = d.cls[i];
        for (uint32_t i = threadIdx.x; i < trans_words; i += 256) t[i] = d.trans[i];
        __syncthreads();
        d.cls = lds;
        d.trans = t;
    }
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= n) return;
    const u64 s = off[a];
    if (search::dfa_match(d, bytes + s, off[a + 1] - s)) atomicOr(&matched[a >> 5], 1u << (a & 31));
}

__global__ __launch_bounds__(256) void k_attr_resolve(const uint32_t *a2f, uint32_t n_a2f, const uint32_t *prt, uint32_t n_prt,
                                                      const uint32_t *matched, uint32_t n_values, const uint32_t *cls, uint32_t *fid_bits,
                                                      uint32_t *root_bits, uint32_t *invalid_bits, u64 *pairs, uint32_t pair_mask) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= n_a2f) return;
    const uint32_t aid = a2f[f];  // UINT32_MAX: no attribute (a2f.rs:98) -- and never < n_values
    if (aid >= n_values || !ids::bit_set(matched, aid)) return;
    atomicOr(&fid_bits[f >> 5], 1u << (f & 31));
    const uint32_t r = ids::chase_root(prt, n_prt, f);
    if (r == kNone) {
        atomicOr(&invalid_bits[f >> 5], 1u << (f & 31));
        return;
    }
    atomicOr(&root_bits[r >> 5], 1u << (r & 31));
    const u64 w = search::pair_word(cls[aid], r);
    for (uint32_t i = search::pair_hash(w) & pair_mask, steps = 0; steps <= pair_mask; i = (i + 1) & pair_mask, ++steps) {
        u64 x = pairs[i];
        if (x == w) return;
        if (x == ids::kEmptyWord) {
            x = atomicCAS(&pairs[i], ids::kEmptyWord, w);
            if (x == ids::kEmptyWord || x == w) return;
        }
    }
}

__global__ __launch_bounds__(64) void k_attr_filter(ids::Table values, const u64 *pairs, uint32_t pair_mask, ids::Types types,
                                                    const uint8_t *key, uint32_t key_len, const uint8_t *text, const u64 *line_off,
                                                    const uint32_t *line_root, u64 n_lines, uint8_t *keep) {
    const u64 i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n_lines) return;
    const u64 a = line_off[i];
    keep[i] = search::keep_line_value(values, pairs, pair_mask, types, key, key_len, text + a, line_off[i + 1] - a, line_root[i]) ? 1 : 0;
}

}  // namespace gffx

using namespace gffx;

struct gffx_hip_attrs : StreamEvents<2> {
    int device = 0;
    int hash_bits = 32;
    int dfa_path = 0;                        // 0: by size; 1: LDS (an error when the tables do not fit); 2: global
    uint32_t n = 0, n_a2f = 0, n_prt = 0;    // `.atn` values; `.a2f` words; `.prt` words
    uint32_t n_bits = 0;                     // max(n_a2f, n_prt): bits of the fid, root and invalid bitmaps
    uint32_t pair_mask = 0, key_len = 0;
    ids::StringTable values, wanted;
    LineChunk lines;
    DevArr<u64> pairs;
    DevArr<uint32_t> cls, a2f, prt, matched, fid_bits, root_bits, invalid_bits;
    DevArr<uint8_t> key, dfa_cls;
    DevArr<uint16_t> dfa_trans;
    const char *last_dfa_kernel = "";
    double ms[4] = {0, 0, 0, 0};  // table build, match, resolve, line filter (HIP events; a failing read of the events adds nothing)

    uint64_t matched_words32() const { return 2 * (((uint64_t)n + 63) / 64); }
    uint64_t bitmap_words32() const { return 2 * (((uint64_t)n_bits + 63) / 64); }
};

namespace {
int clear_resolved(gffx_hip_attrs *h) {
    GFFX_HIP_TRY(hipMemsetAsync(h->fid_bits.p, 0, h->bitmap_words32() * 4, h->stream));
    GFFX_HIP_TRY(hipMemsetAsync(h->root_bits.p, 0, h->bitmap_words32() * 4, h->stream));
    GFFX_HIP_TRY(hipMemsetAsync(h->invalid_bits.p, 0, h->bitmap_words32() * 4, h->stream));
    GFFX_HIP_TRY(hipMemsetAsync(h->pairs.p, 0xFF, ((uint64_t)h->pair_mask + 1) * 8, h->stream));
    return GFFX_OK;
}
}  // namespace

extern "C" int gffx_hip_attrs_create(int device, uint64_t n_values, const uint8_t *values, const uint64_t *value_off, uint64_t n_a2f,
                                     const uint32_t *a2f, uint64_t n_prt, const uint32_t *prt, const uint8_t *key, uint32_t key_len,
                                     int hash_bits, int dfa_path, gffx_hip_attrs **out) {
    static const char *who = "gffx_hip_attrs_create";
    if (!out) return fail(GFFX_E_INVALID, "%s: out is NULL", who);
    *out = nullptr;
    if (n_values && !value_off) return fail(GFFX_E_INVALID, "%s: value_off is NULL", who);
    if (n_a2f && !a2f) return fail(GFFX_E_INVALID, "%s: a2f is NULL", who);
    if (n_prt && !prt) return fail(GFFX_E_INVALID, "%s: prt is NULL", who);
    if (key_len && !key) return fail(GFFX_E_INVALID, "%s: key is NULL", who);
    if (n_values > (1ull << 28) || n_a2f > (1ull << 28) || n_prt > (1ull << 28))
        return fail(GFFX_E_INVALID, "%s: %llu values, %llu attribute words, %llu parent words (at most 2^28 each)", who,
                    (unsigned long long)n_values, (unsigned long long)n_a2f, (unsigned long long)n_prt);
    if (hash_bits > 32) return fail(GFFX_E_INVALID, "%s: hash_bits %d (0 to 32; negative: all 32)", who, hash_bits);
    if (dfa_path < 0 || dfa_path > 2) return fail(GFFX_E_INVALID, "%s: dfa_path %d (0: by size, 1: LDS, 2: global)", who, dfa_path);
    uint64_t n_bytes = 0;
    if (int rc = check_offsets(who, "value_off", value_off, n_values, &n_bytes)) return rc;
    if (n_bytes && !values) return fail(GFFX_E_INVALID, "%s: values is NULL", who);
    if (int rc = check_device(device)) return rc;
    GFFX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<gffx_hip_attrs> h(new (std::nothrow) gffx_hip_attrs);
    if (!h) return fail(GFFX_E_OOM, "%s: out of host memory", who);
    h->device = device;
    h->hash_bits = hash_bits < 0 ? 32 : hash_bits;
    h->dfa_path = dfa_path;
    h->n = (uint32_t)n_values;
    h->n_a2f = (uint32_t)n_a2f;
    h->n_prt = (uint32_t)n_prt;
    h->n_bits = std::max(h->n_a2f, h->n_prt);
    h->key_len = key_len;
    h->pair_mask = ids::table_slots(n_a2f) - 1;  // >= 2 x the fids, so >= 2 x the matched ones: a probe always ends
    GFFX_HIP_TRY(h->create_stream());
    GFFX_HIP_TRY(h->cls.ensure(std::max<uint64_t>(n_values, 1)));
    GFFX_HIP_TRY(h->a2f.ensure(std::max<uint64_t>(n_a2f, 1)));
    GFFX_HIP_TRY(h->prt.ensure(std::max<uint64_t>(n_prt, 1)));
    GFFX_HIP_TRY(h->key.ensure(std::max<uint32_t>(key_len, 1)));
    GFFX_HIP_TRY(h->matched.ensure(std::max<uint64_t>(h->matched_words32(), 2)));
    GFFX_HIP_TRY(h->fid_bits.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    GFFX_HIP_TRY(h->root_bits.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    GFFX_HIP_TRY(h->invalid_bits.ensure(std::max<uint64_t>(h->bitmap_words32(), 2)));
    GFFX_HIP_TRY(h->pairs.ensure((uint64_t)h->pair_mask + 1));
    hipStream_t s = h->stream;
    if (n_a2f) GFFX_HIP_TRY(hipMemcpyAsync(h->a2f.p, a2f, n_a2f * 4, hipMemcpyHostToDevice, s));
    if (n_prt) GFFX_HIP_TRY(hipMemcpyAsync(h->prt.p, prt, n_prt * 4, hipMemcpyHostToDevice, s));
    if (key_len) GFFX_HIP_TRY(hipMemcpyAsync(h->key.p, key, key_len, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemsetAsync(h->matched.p, 0, h->matched_words32() * 4, s));
    if (int rc = clear_resolved(h.get())) return rc;
    if (int rc = h->values.build(s, n_values, values, value_off, ids::hash_mask_of(h->hash_bits), h->ev[0])) return rc;
    if (h->n) hipLaunchKernelGGL(k_attr_classes, dim3((h->n + 255) / 256), dim3(256), 0, s, h->values.table(), h->n, h->cls.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));  // (the caller's arrays have been read)
    (void)h->add_ms(&h->ms[0]);
    *out = h.release();
    return GFFX_OK;
}

extern "C" void gffx_hip_attrs_destroy(gffx_hip_attrs *h) { delete h; }

extern "C" uint64_t gffx_hip_attrs_n(const gffx_hip_attrs *h) { return h ? h->n : 0; }

extern "C" int gffx_hip_attrs_options(const gffx_hip_attrs *h, char *buf, size_t cap) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_options: NULL handle");
    std::string s = "{";
    if (h->hash_bits != 32) s += "\"hash_bits\": " + std::to_string(h->hash_bits);
    if (h->dfa_path) s += std::string(s.size() > 1 ? ", " : "") + "\"dfa_path\": \"" + (h->dfa_path == 1 ? "lds" : "global") + "\"";
    return copy_out(s + "}", buf, cap);
}

extern "C" int gffx_hip_attrs_match_exact(gffx_hip_attrs *h, uint64_t n_wanted, const uint8_t *wanted, const uint64_t *wanted_off) {
    static const char *who = "gffx_hip_attrs_match_exact";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    if (n_wanted && !wanted_off) return fail(GFFX_E_INVALID, "%s: wanted_off is NULL", who);
    if (n_wanted > (1ull << 28)) return fail(GFFX_E_INVALID, "%s: %llu wanted strings (at most 2^28)", who, (unsigned long long)n_wanted);
    uint64_t n_bytes = 0;
    if (int rc = check_offsets(who, "wanted_off", wanted_off, n_wanted, &n_bytes)) return rc;
    if (n_bytes && !wanted) return fail(GFFX_E_INVALID, "%s: wanted is NULL", who);
    if (!n_wanted || !h->n) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (int rc = h->wanted.build(s, n_wanted, wanted, wanted_off, h->values.hash_mask, h->ev[0])) return rc;
    hipLaunchKernelGGL(k_attr_match_exact, dim3((h->n + 255) / 256), dim3(256), 0, s, h->wanted.table(), h->values.bytes.p, h->values.off.p, h->n,
                       h->matched.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    (void)h->add_ms(&h->ms[1]);
    return GFFX_OK;
}

extern "C" int gffx_hip_attrs_match_dfa(gffx_hip_attrs *h, uint32_t n_states, uint32_t n_classes, uint32_t init, const uint8_t *cls,
                                        const uint16_t *trans) {
    static const char *who = "gffx_hip_attrs_match_dfa";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    if (!cls || !trans) return fail(GFFX_E_INVALID, "%s: cls or trans is NULL", who);
    if (n_states < 1 || n_states > 65535 || n_classes < 2 || n_classes > 257 || init >= n_states)
        return fail(GFFX_E_INVALID, "%s: %u states (1 to 65535), %u classes (2 to 257), start state %u", who, n_states, n_classes, init);
    // every index the walk can form stays inside the table
    for (int b = 0; b < 256; ++b)
        if (cls[b] >= n_classes - 1) return fail(GFFX_E_INVALID, "%s: byte %d maps to column %u of %u", who, b, cls[b], n_classes);
    const uint64_t words = (uint64_t)n_states * n_classes;
    for (uint64_t i = 0; i < words; ++i)
        if (trans[i] >= n_states) return fail(GFFX_E_INVALID, "%s: a transition to state %u of %u", who, trans[i], n_states);
    const uint64_t lds_bytes = 256 + 2 * words;
    const bool fits = lds_bytes <= kLdsBudget;
    if (h->dfa_path == 1 && !fits)
        return fail(GFFX_E_INVALID, "%s: the tables need %llu bytes of LDS, the budget is %u", who, (unsigned long long)lds_bytes, kLdsBudget);
    const bool use_lds = h->dfa_path == 2 ? false : fits;
    h->last_dfa_kernel = use_lds ? "k_attr_match_dfa<lds>" : "k_attr_match_dfa<global>";
    if (!h->n) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    GFFX_HIP_TRY(h->dfa_cls.ensure(256));
    GFFX_HIP_TRY(h->dfa_trans.ensure(words));
    hipStream_t s = h->stream;
    GFFX_HIP_TRY(hipMemcpyAsync(h->dfa_cls.p, cls, 256, hipMemcpyHostToDevice, s));
    GFFX_HIP_TRY(hipMemcpyAsync(h->dfa_trans.p, trans, words * 2, hipMemcpyHostToDevice, s));
    const search::Dfa d{h->dfa_cls.p, h->dfa_trans.p, n_states, n_classes, init};
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    if (use_lds)
        hipLaunchKernelGGL(k_attr_match_dfa<true>, dim3((h->n + 255) / 256), dim3(256), (size_t)lds_bytes, s, d, h->values.bytes.p, h->values.off.p, h->n,
                           h->matched.p);
    else
        hipLaunchKernelGGL(k_attr_match_dfa<false>, dim3((h->n + 255) / 256), dim3(256), 0, s, d, h->values.bytes.p, h->values.off.p, h->n,
                           h->matched.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));  // (the caller's tables have been read)
    (void)h->add_ms(&h->ms[1]);
    return GFFX_OK;
}

extern "C" const char *gffx_hip_attrs_dfa_kernel(const gffx_hip_attrs *h) { return h ? h->last_dfa_kernel : ""; }

extern "C" int gffx_hip_attrs_reset(gffx_hip_attrs *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_reset: NULL handle");
    GFFX_HIP_TRY(hipSetDevice(h->device));
    GFFX_HIP_TRY(hipMemsetAsync(h->matched.p, 0, h->matched_words32() * 4, h->stream));
    if (int rc = clear_resolved(h)) return rc;
    GFFX_HIP_TRY(hipStreamSynchronize(h->stream));
    return GFFX_OK;
}

extern "C" int gffx_hip_attrs_resolve(gffx_hip_attrs *h) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_resolve: NULL handle");
    GFFX_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (int rc = clear_resolved(h)) return rc;
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    if (h->n_a2f)
        hipLaunchKernelGGL(k_attr_resolve, dim3((h->n_a2f + 255) / 256), dim3(256), 0, s, h->a2f.p, h->n_a2f, h->prt.p, h->n_prt, h->matched.p, h->n,
                           h->cls.p, h->fid_bits.p, h->root_bits.p, h->invalid_bits.p, h->pairs.p, h->pair_mask);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    GFFX_HIP_TRY(hipStreamSynchronize(s));
    (void)h->add_ms(&h->ms[2]);
    return GFFX_OK;
}

extern "C" int gffx_hip_attrs_copy_matched_bitmap(gffx_hip_attrs *h, uint64_t *host, uint64_t n_words) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_copy_matched_bitmap: NULL handle");
    return copy_bitmap("gffx_hip_attrs_copy_matched_bitmap", h->device, h->stream, h->matched.p, h->matched_words32() / 2, host, n_words);
}
extern "C" int gffx_hip_attrs_copy_fid_bitmap(gffx_hip_attrs *h, uint64_t *host, uint64_t n_words) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_copy_fid_bitmap: NULL handle");
    return copy_bitmap("gffx_hip_attrs_copy_fid_bitmap", h->device, h->stream, h->fid_bits.p, h->bitmap_words32() / 2, host, n_words);
}
extern "C" int gffx_hip_attrs_copy_root_bitmap(gffx_hip_attrs *h, uint64_t *host, uint64_t n_words) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_copy_root_bitmap: NULL handle");
    return copy_bitmap("gffx_hip_attrs_copy_root_bitmap", h->device, h->stream, h->root_bits.p, h->bitmap_words32() / 2, host, n_words);
}
extern "C" int gffx_hip_attrs_copy_invalid_bitmap(gffx_hip_attrs *h, uint64_t *host, uint64_t n_words) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_copy_invalid_bitmap: NULL handle");
    return copy_bitmap("gffx_hip_attrs_copy_invalid_bitmap", h->device, h->stream, h->invalid_bits.p, h->bitmap_words32() / 2, host, n_words);
}

extern "C" int gffx_hip_attrs_filter_lines(gffx_hip_attrs *h, const uint8_t *text, uint64_t n_bytes, uint64_t n_lines, const uint64_t *line_off,
                                           const uint32_t *line_root, int by_type, uint32_t n_types, const uint8_t *types,
                                           const uint32_t *type_off, uint8_t *keep_out) {
    static const char *who = "gffx_hip_attrs_filter_lines";
    if (!h) return fail(GFFX_E_INVALID, "%s: NULL handle", who);
    const LineArgs a{text, n_bytes, n_lines, line_off, line_root, by_type, n_types, types, type_off, keep_out};
    if (int rc = LineChunk::check(who, a)) return rc;
    if (!n_lines) return GFFX_OK;
    GFFX_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    ids::Types ty;
    if (int rc = h->lines.upload(s, a, &ty)) return rc;
    GFFX_HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_attr_filter, dim3((unsigned)((n_lines + 63) / 64)), dim3(64), 0, s, h->values.table(), h->pairs.p, h->pair_mask, ty, h->key.p,
                       h->key_len, h->lines.text.p, h->lines.line_off.p, h->lines.line_root.p, (u64)n_lines, h->lines.keep.p);
    GFFX_HIP_TRY(hipGetLastError());
    GFFX_HIP_TRY(hipEventRecord(h->ev[1], s));
    if (int rc = h->lines.download(s, a)) return rc;
    (void)h->add_ms(&h->ms[3]);
    return GFFX_OK;
}

extern "C" int gffx_hip_attrs_stage_ms(const gffx_hip_attrs *h, double *build_ms, double *match_ms, double *resolve_ms, double *filter_ms) {
    if (!h) return fail(GFFX_E_INVALID, "gffx_hip_attrs_stage_ms: NULL handle");
    if (build_ms) *build_ms = h->ms[0];
    if (match_ms) *match_ms = h->ms[1];
    if (resolve_ms) *resolve_ms = h->ms[2];
    if (filter_ms) *filter_ms = h->ms[3];
    return GFFX_OK;
}
