// source_read.hpp -- what bam.cpp and sam.cpp share around the engine's source handles: the chunk-size knob, the stage
// timer, and the epilogue that reports the stage times and takes the rows and the tallies back.
#pragma once
#include <cstdlib>

#include "bgzf_file.hpp"
#include "gffx.hpp"

namespace gffx::source {

using clock = std::chrono::steady_clock;
inline double ms_since(clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); }

struct Timer {  // a "[TIMER]" line under -v, and the stage of --stats-json
    bool verbose;
    void operator()(const char *what, double ms) const {
        if (verbose) std::fprintf(stderr, "[TIMER] [run] %s took %.3f ms\n", what, ms);
        g_run_stats.stage(what, ms);
    }
};

// a positive decimal number of bytes in the environment variable `name`, or `fallback`
inline uint64_t chunk_bytes_from_env(const char *name, uint64_t fallback) {
    const char *e = std::getenv(name);
    if (e && *e) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end && !*end && v > 0) return v;
    }
    return fallback;
}

// the rows per device batch of depth, coverage and meta in the environment variable `name` (gffx.hpp): a positive decimal
// number, capped at 1 << 28; anything else -- a sign or a blank in front too, which strtoull alone would take -- is ignored
inline size_t batch_rows_from_env(const char *name) {
    const char *e = std::getenv(name);
    if (e && *e >= '0' && *e <= '9') {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end && !*end && v > 0) return static_cast<size_t>(std::min<unsigned long long>(v, 1ull << 28));
    }
    return 4u << 20;
}

template <class H>
struct Reader {  // the read-back entry points of a source handle, and its format's stage names (keys of --stats-json)
    int (*stage_ms)(const H *, double *, double *, double *);
    uint64_t (*n_rows)(const H *);
    int (*copy_rows)(H *, uint32_t *);
    int (*counts)(const H *, uint64_t *, uint64_t *, uint64_t *, uint64_t *);
    const char *label[5];  // the three device stages, the chunks in all, the rows copy
};

// after _finish: the stage times reported, the rows, and counts[4] = the handle's tallies.  engine_error(): the caller's Error.
template <class H, class F>
std::vector<uint32_t> take_rows(H *h, const Reader<H> &r, const Timer &timer, double feed_ms, uint64_t counts[4], F &&engine_error) {
    double ms[3] = {0, 0, 0};
    r.stage_ms(h, &ms[0], &ms[1], &ms[2]);
    for (int k = 0; k < 3; ++k) timer(r.label[k], ms[k]);
    timer(r.label[3], feed_ms);
    const auto t = clock::now();
    std::vector<uint32_t> rows(3 * r.n_rows(h));
    if (r.copy_rows(h, rows.data()) != GFFX_OK) throw engine_error();
    timer(r.label[4], ms_since(t));
    r.counts(h, &counts[0], &counts[1], &counts[2], &counts[3]);
    return rows;
}

}  // namespace gffx::source
