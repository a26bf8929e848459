// table_handle.hpp -- the plumbing the C-ABI handles over a string table share (ids.hip, search.hip, gff.hip): the check of
// an offsets array, the stream with its timing events, the bitmap download and the front half of a filter_lines call.  The
// functions take `who`, the name of the exported function at work, because every message starts with it.
#pragma once
#include "gffx_device.hpp"
#include "ids_core.hpp"

namespace gffx {

// offsets ascending from 0?  (what every kernel's reads are bounded by)
template <class T>
int check_offsets(const char *who, const char *what, const T *off, uint64_t n, uint64_t *total) {
    *total = 0;
    if (!n) return GFFX_OK;
    if (off[0] != 0) return fail(GFFX_E_INVALID, "%s: %s[0] is not 0", who, what);
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(GFFX_E_INVALID, "%s: %s is not ascending at %llu", who, what, (unsigned long long)i);
    *total = off[n];
    return GFFX_OK;
}

// the stream of a handle and the events its stages are timed with
template <int N>
struct StreamEvents {
    hipStream_t stream = nullptr;
    hipEvent_t ev[N] = {};

    hipError_t create_stream() {
        hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        for (int k = 0; k < N && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
        return e;
    }
    // *acc += the milliseconds between ev[a] and ev[b] (recorded on the stream, which has been synchronised)
    hipError_t add_ms(double *acc, int a = 0, int b = 1) const {
        float t = 0;
        const hipError_t e = hipEventElapsedTime(&t, ev[a], ev[b]);
        if (e == hipSuccess) *acc += t;
        return e;
    }
    ~StreamEvents() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// the first `need` 64-bit words of the device bitmap d, once the stream's work is done
inline int copy_bitmap(const char *who, int device, hipStream_t stream, const uint32_t *d, uint64_t need, uint64_t *host, uint64_t n_words) {
    if (n_words < need) return fail(GFFX_E_INVALID, "%s: %llu words given, %llu needed", who, (unsigned long long)n_words, (unsigned long long)need);
    if (need && !host) return fail(GFFX_E_INVALID, "%s: host is NULL", who);
    GFFX_HIP_TRY(hipSetDevice(device));
    GFFX_HIP_TRY(hipStreamSynchronize(stream));
    if (need) GFFX_HIP_TRY(hipMemcpy(host, d, need * 8, hipMemcpyDeviceToHost));
    return GFFX_OK;
}

// the arguments every filter_lines function takes behind its handle
struct LineArgs {
    const uint8_t *text;
    uint64_t n_bytes, n_lines;
    const uint64_t *line_off;
    const uint32_t *line_root;
    int by_type;
    uint32_t n_types;
    const uint8_t *types;
    const uint32_t *type_off;
    uint8_t *keep_out;
};

// one chunk of lines on the device: check(), then (with lines to test) upload(), the caller's kernel, download()
struct LineChunk {
    DevArr<uint8_t> text, type_bytes, keep;
    DevArr<u64> line_off;
    DevArr<uint32_t> line_root, type_off;

    static int check(const char *who, const LineArgs &a) {
        if (a.n_lines && (!a.line_off || !a.line_root || !a.keep_out)) return fail(GFFX_E_INVALID, "%s: line_off, line_root or keep_out is NULL", who);
        if (a.n_lines > (1ull << 32)) return fail(GFFX_E_INVALID, "%s: %llu lines in one call (at most 2^32)", who, (unsigned long long)a.n_lines);
        uint64_t end = 0;
        if (int rc = check_offsets(who, "line_off", a.line_off, a.n_lines, &end)) return rc;
        if (end > a.n_bytes) return fail(GFFX_E_INVALID, "%s: the last line ends at %llu, the text has %llu bytes", who, (unsigned long long)end,
                                         (unsigned long long)a.n_bytes);
        if (a.n_bytes && !a.text) return fail(GFFX_E_INVALID, "%s: text is NULL", who);
        if (a.n_types) {
            if (!a.type_off) return fail(GFFX_E_INVALID, "%s: type_off is NULL", who);
            if (a.n_types > 65536) return fail(GFFX_E_INVALID, "%s: %u type names (at most 65536)", who, a.n_types);
            if (int rc = check_offsets(who, "type_off", a.type_off, a.n_types, &end)) return rc;
            if (end && !a.types) return fail(GFFX_E_INVALID, "%s: types is NULL", who);
        }
        return GFFX_OK;
    }
    // the checked chunk to the device on stream s; *ty: its -T set
    int upload(hipStream_t s, const LineArgs &a, ids::Types *ty) {
        const uint32_t n_type_bytes = a.n_types ? a.type_off[a.n_types] : 0;
        GFFX_HIP_TRY(text.ensure(a.n_bytes + ids::kPad));
        GFFX_HIP_TRY(line_off.ensure(a.n_lines + 1));
        GFFX_HIP_TRY(line_root.ensure(a.n_lines));
        GFFX_HIP_TRY(keep.ensure(a.n_lines));
        GFFX_HIP_TRY(type_bytes.ensure(std::max<uint32_t>(n_type_bytes, 1)));
        GFFX_HIP_TRY(type_off.ensure(a.n_types + 1));
        if (a.n_bytes) GFFX_HIP_TRY(hipMemcpyAsync(text.p, a.text, a.n_bytes, hipMemcpyHostToDevice, s));
        GFFX_HIP_TRY(hipMemcpyAsync(line_off.p, a.line_off, (a.n_lines + 1) * 8, hipMemcpyHostToDevice, s));
        GFFX_HIP_TRY(hipMemcpyAsync(line_root.p, a.line_root, a.n_lines * 4, hipMemcpyHostToDevice, s));
        if (n_type_bytes) GFFX_HIP_TRY(hipMemcpyAsync(type_bytes.p, a.types, n_type_bytes, hipMemcpyHostToDevice, s));
        if (a.n_types) GFFX_HIP_TRY(hipMemcpyAsync(type_off.p, a.type_off, (a.n_types + 1) * 4, hipMemcpyHostToDevice, s));
        *ty = ids::Types{type_bytes.p, type_off.p, a.n_types, a.by_type || a.n_types ? 1 : 0};
        return GFFX_OK;
    }
    // keep[0, n_lines) to the caller; returns with the stream synchronised
    int download(hipStream_t s, const LineArgs &a) {
        GFFX_HIP_TRY(hipMemcpyAsync(a.keep_out, keep.p, a.n_lines, hipMemcpyDeviceToHost, s));
        GFFX_HIP_TRY(hipStreamSynchronize(s));
        return GFFX_OK;
    }
};

}  // namespace gffx
