// join_a_stream.cpp -- Join A of `gffx intersect` through include/gffx_hip.h: the one-shot calls and the BED branch's streamed pipeline
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>

#include "intersect_internal.hpp"

namespace gffx::commands::intersect {

namespace {

// a bitmap over the index's roots -> their fids, ascending and unique (intersect.rs:598-615)
std::vector<uint32_t> roots_of_bitmap(const gffx_hip_index *ix, const std::vector<uint64_t> &words) {
    const uint64_t n_roots = gffx_hip_index_n_roots(ix);
    const uint32_t *fids = gffx_hip_index_sorted_fids(ix);
    std::vector<uint32_t> roots;
    for (uint64_t i = 0; i < n_roots; ++i)
        if (words[i >> 6] >> (i & 63) & 1) roots.push_back(fids[i]);
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
    return roots;
}

}  // namespace

std::vector<Region> query_features(TreeIndexData &index_data, const std::vector<Region> &regions, OverlapMode mode,
                                   bool invert, bool verbose, int device) {
    index_data.ensure_device(device);
    if (verbose) std::fprintf(stderr, "[DEBUG] Querying %zu regions on HIP device %d\n", regions.size(), device);
    const std::vector<uint32_t> flat = flatten(regions);
    uint32_t *triples = nullptr;
    uint64_t n = 0;
    if (gffx_hip_query_features(index_data.device_index.get(), flat.data(), regions.size(), static_cast<int>(mode),
                                invert ? 1 : 0, &triples, &n) != GFFX_OK)
        hip_fail("query_features");
    std::vector<Region> out(n);
    for (uint64_t i = 0; i < n; ++i) out[i] = {triples[3 * i], triples[3 * i + 1], triples[3 * i + 2]};
    gffx_hip_free_host(triples);
    return out;
}

std::vector<uint32_t> query_unique_roots(TreeIndexData &index_data, const uint32_t *flat, uint64_t n_regions, OverlapMode mode,
                                         bool invert, bool verbose, int device) {
    StageTimer sub{verbose};
    index_data.ensure_device(device);
    gffx_hip_index *ix = index_data.device_index.get();
    sub.lap("  index upload");
    if (verbose) std::fprintf(stderr, "[DEBUG] Querying %zu regions on HIP device %d\n", static_cast<size_t>(n_regions), device);
    BatchHandle b;
    if (gffx_hip_batch_create(ix, n_regions, OutPtr(b)) != GFFX_OK) hip_fail("batch_create");
    sub.lap("  batch buffers");
    if (gffx_hip_batch_set_regions_host(b.get(), flat, n_regions) != GFFX_OK) hip_fail("set_regions");
    if (gffx_hip_batch_run(b.get(), static_cast<int>(mode), invert ? 1 : 0, GFFX_OUT_ROOT_BITMAP | GFFX_OUT_NO_COUNTS, GFFX_STRATEGY_AUTO) != GFFX_OK)
        hip_fail("batch_run");
    if (gffx_hip_batch_wait(b.get()) != GFFX_OK) hip_fail("query_features");
    sub.lap("  regions H2D + Join A kernel");
    std::vector<uint64_t> words((gffx_hip_index_n_roots(ix) + 63) / 64 + 1, 0);
    if (gffx_hip_batch_copy_root_bitmap(b.get(), words.data(), words.size()) != GFFX_OK) hip_fail("copy_root_bitmap");
    return roots_of_bitmap(ix, words);
}

std::vector<uint32_t> query_unique_roots(TreeIndexData &index_data, const std::vector<Region> &regions,
                                         OverlapMode mode, bool invert, bool verbose, int device) {
    const std::vector<uint32_t> flat = flatten(regions);
    return query_unique_roots(index_data, flat.data(), regions.size(), mode, invert, verbose, device);
}

namespace {

// BED text per chunk; a row is at least 6 bytes ("a\t1\t2\n"), and the two pinned staging buffers and the two batches of a
// device are sized for a chunk of such rows: creating them is on the critical path once the parser is fast (100 M rows,
// "region stores + batches": 101 ms with 128 MB chunks, 70 with 64, 43 with 32, 36 with 16; whole run 0.73 / 0.65 / 0.58 /
// 0.53 s).  GFFX_CHUNK_MB / GFFX_CHUNK_BYTES override the 16 MB (stream_chunk_bytes, intersect_internal.hpp;
// tests/test_chunked_cli_gpu.py); results never depend on either.
static const size_t kChunkBytes = stream_chunk_bytes();
constexpr size_t kMinRowBytes = kMinBedRowBytes;

using Pieces = std::vector<std::vector<uint32_t>>;  // the rows of one chunk, as parse_bed_pieces leaves them

// The parser runs ahead on its own thread (each chunk on `threads` workers) while the caller brings the devices up and then
// feeds them: a bounded queue of parsed chunks, in file order.  The thread never outlives the object, whatever throws.
class ChunkParser {
  public:
    struct Parsed {
        Pieces piece;
        bool last = false;
    };
    ChunkParser(std::string_view text, const SeqidTable &seqids, size_t threads)
        : text_(text), seqids_(seqids), threads_(threads), thread_([this] { run(); }) {}
    ~ChunkParser() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (thread_.joinable()) thread_.join();
    }
    // the next chunk in file order; the parser's error once the chunks parsed before it were served
    Parsed next() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !queue_.empty() || error_; });
        if (queue_.empty()) std::rethrow_exception(error_);
        Parsed pc = std::move(queue_.front());
        queue_.pop_front();
        cv_.notify_all();
        return pc;
    }
    // row buffers of a consumed chunk: reused, so that after the first chunks the parser touches no fresh pages (64 threads
    // faulting in 32 MB per chunk serialise on the address space's lock)
    void recycle(Pieces &&piece) {
        std::lock_guard<std::mutex> lk(mu_);
        spare_.push_back(std::move(piece));
    }
    // after the last chunk was taken: the thread is done; the time it spent in parse_bed_pieces
    double finish() {
        thread_.join();
        return parse_ms_;
    }

  private:
    void run() {
        try {
            WorkerPool workers(text_.size() < (1u << 20) ? 0 : std::min<size_t>(std::max<size_t>(threads_, 1), 64) - 1);
            for_each_line_chunk(text_, kChunkBytes, [&](size_t pos, size_t z, bool last) {
                Parsed pc;
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    if (!spare_.empty()) {
                        pc.piece = std::move(spare_.back());
                        spare_.pop_back();
                    }
                }
                const auto t0 = std::chrono::steady_clock::now();
                parse_bed_pieces(text_, pos, z, last, seqids_, threads_, pc.piece, &workers);
                parse_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                pc.last = last;
                std::unique_lock<std::mutex> lk(mu_);
                // (up to 3 GB of text = ~1.5 GB of parsed rows ahead while the devices come up: HIP start-up + index upload take
                //  ~0.25 s, in which the host threads parse more than that)
                cv_.wait(lk, [&] { return queue_.size() < std::max<size_t>(4, (size_t(3) << 30) / kChunkBytes) || stop_; });
                if (stop_) return false;
                queue_.push_back(std::move(pc));
                cv_.notify_all();
                return true;
            });
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu_);
            error_ = std::current_exception();
            cv_.notify_all();
        }
    }
    const std::string_view text_;
    const SeqidTable &seqids_;
    const size_t threads_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Parsed> queue_;
    std::vector<Pieces> spare_;
    std::exception_ptr error_;
    bool stop_ = false;
    double parse_ms_ = 0;
    std::thread thread_;  // (last: it starts in the constructor and uses the members above)
};

// Per logical device d: a region store (two pinned staging buffers; device 0's keeps every region when Join B follows) and
// two batches, 2 * d + k for staging buffer k; used[2 * d + k]: the batch has run, its bitmap accumulates from now on
struct Lanes {
    std::vector<RegionsHandle> store;
    std::vector<BatchHandle> batch;
    std::vector<char> used;
    std::vector<uint64_t> rows;  // regions served per device
};

Lanes create_lanes(const DeviceSet &devs, const std::vector<gffx_hip_index *> &ix, size_t chunk_rows, size_t keep_rows) {
    const size_t D = devs.size();
    Lanes l{std::vector<RegionsHandle>(D), std::vector<BatchHandle>(2 * D), std::vector<char>(2 * D, 0), std::vector<uint64_t>(D, 0)};
    for (size_t d = 0; d < D; ++d) {
        const bool full = d == 0 && keep_rows;
        if (gffx_hip_regions_create(devs[d], full ? keep_rows : 0, chunk_rows, full ? 1 : 0, OutPtr(l.store[d])) != GFFX_OK) hip_fail("gffx_hip_regions_create");
        for (int k = 0; k < 2; ++k)
            if (gffx_hip_batch_create(ix[d], chunk_rows, OutPtr(l.batch[2 * d + k])) != GFFX_OK) hip_fail("batch_create");
    }
    return l;
}

// the tuning knobs this run did not leave at their defaults (--stats-json "knobs")
std::string knobs_json(const gffx_hip_index *ix, const gffx_hip_batch *b) {
    char ik[512] = "{}", bk[512] = "{}";
    gffx_hip_index_options(ix, ik, sizeof ik);
    gffx_hip_batch_options(b, bk, sizeof bk);
    const std::string a(ik), c(bk);
    return a.size() <= 2 ? c : c.size() <= 2 ? a : a.substr(0, a.size() - 1) + ", " + c.substr(1);
}

// staging buffers k: wait for the copies (and the passes) of the chunk two before this one
void wait_staging(const Lanes &l, int k) {
    for (size_t d = 0; d < l.store.size(); ++d) {
        if (l.used[2 * d + k] && gffx_hip_batch_sync(l.batch[2 * d + k].get()) != GFFX_OK) hip_fail("batch_sync");
        if (gffx_hip_regions_wait_staging(l.store[d].get(), k) != GFFX_OK) hip_fail("wait_staging");
    }
}

// One device: the rows go over in file order; a few copy threads (memory-bound) take the pieces in turn.  Returns the rows;
// with keep_store, has_regions[seqid] is set for the seqids seen.
uint64_t fill_one_device(const Pieces &piece, uint32_t *dst, uint32_t n_seq, bool keep_store, std::vector<char> &has_regions) {
    const size_t T = piece.size();
    std::vector<uint64_t> off(T + 1, 0);
    for (size_t t = 0; t < T; ++t) off[t + 1] = off[t] + piece[t].size() / 3;
    const size_t W = std::min<size_t>(T, 8);
    std::vector<std::vector<char>> seen(W, std::vector<char>(keep_store ? n_seq : 0, 0));
    std::atomic<size_t> next_piece{0};
    parallel_for(W, W, [&](size_t w) {  // (shares by worker, not by piece: seen[w] is the worker's)
        for (;;) {
            const size_t t = next_piece.fetch_add(1);
            if (t >= T) return;
            std::memcpy(dst + 3 * off[t], piece[t].data(), piece[t].size() * 4);
            if (keep_store)
                for (size_t i = 0; i < piece[t].size(); i += 3) seen[w][piece[t][i]] = 1;
        }
    });
    for (size_t w = 0; w < W && keep_store; ++w)
        for (uint32_t c = 0; c < n_seq; ++c) has_regions[c] |= seen[w][c];
    return off[T];
}

// The chunk in staging buffers k (n_dev[d] rows for device d) -> appended to the stores and through Join A, the root bitmap
// kept from the batch's earlier chunks.  Returns the chunk's rows.
uint64_t launch_chunk(Lanes &l, int k, const std::vector<uint64_t> &n_dev, bool keep_store, OverlapMode mode, bool invert, uint64_t &wide_form_passes) {
    const size_t D = n_dev.size();
    uint64_t chunk_total = 0;
    for (size_t d = 0; d < D; ++d) chunk_total += n_dev[d];
    for (size_t d = 0; d < D; ++d) {
        const uint64_t n_up = (d == 0 && keep_store) ? chunk_total : n_dev[d];
        if (gffx_hip_regions_append(l.store[d].get(), k, n_up) != GFFX_OK) hip_fail("regions_append");
        gffx_hip_batch *b = l.batch[2 * d + k].get();
        if (gffx_hip_batch_set_regions_store(b, l.store[d].get(), k, 0, n_dev[d]) != GFFX_OK) hip_fail("set_regions_store");
        const uint32_t flags = static_cast<uint32_t>(GFFX_OUT_ROOT_BITMAP) | static_cast<uint32_t>(GFFX_OUT_NO_COUNTS) |
                               (l.used[2 * d + k] ? static_cast<uint32_t>(GFFX_OUT_BITMAP_KEEP) : 0u);
        if (gffx_hip_batch_run(b, static_cast<int>(mode), invert ? 1 : 0, flags, GFFX_STRATEGY_AUTO) != GFFX_OK) hip_fail("batch_run");
        wide_form_passes += gffx_hip_batch_wide_form(b) ? 1 : 0;
        l.used[2 * d + k] = 1;
        l.rows[d] += n_dev[d];
    }
    return chunk_total;
}

// The results: OR of the batches' bitmaps -> res.roots; {regions, kept pairs} per logical device -> res.per_device, through
// the exchange step when there is more than one device (what the run REPORTS per device -- --stats-json "devices", -v -- is
// what came back from it).
void collect_results(const Lanes &l, const DeviceSet &devs, const gffx_hip_index *ix, bool verbose, StageTimer &sub, StreamResult &res) {
    const size_t D = devs.size();
    std::vector<uint64_t> words((gffx_hip_index_n_roots(ix) + 63) / 64 + 1, 0), tmp(words.size(), 0);
    res.per_device.assign(2 * D, 0);
    for (size_t d = 0; d < D; ++d)
        for (int k = 0; k < 2; ++k) {
            if (!l.used[2 * d + k]) continue;
            gffx_hip_batch *b = l.batch[2 * d + k].get();
            if (gffx_hip_batch_wait(b) != GFFX_OK) hip_fail("query_features");
            if (gffx_hip_batch_copy_root_bitmap(b, tmp.data(), tmp.size()) != GFFX_OK) hip_fail("copy_root_bitmap");
            for (size_t w = 0; w < words.size(); ++w) words[w] |= tmp[w];
            uint64_t kept = 0;  // the kept pairs of every chunk this batch served (the root passes count them per block)
            if (gffx_hip_batch_kept_pairs_accumulated(b, &kept) != GFFX_OK) hip_fail("kept_pairs_accumulated");
            res.per_device[2 * d + 1] += kept;
        }
    sub.lap("  streaming the BED file through Join A");
    for (size_t d = 0; d < D; ++d) res.per_device[2 * d] = l.rows[d];
    if (D > 1) {
        res.exchanged = devs.exchange_counts(res.per_device, "regions", "kept pairs", verbose, /*adopt_gathered=*/true);
        sub.lap("  hit-count exchange");
    }
    res.roots = roots_of_bitmap(ix, words);
}

}  // namespace

// Join A over a whole BED file, streamed: the text is parsed chunk by chunk on the host threads straight into pinned
// staging buffers, every chunk goes to the device(s) while the next one is parsed (two staging buffers / two batches per
// device), the root bitmap accumulates on the device across chunks (GFFX_OUT_BITMAP_KEEP).  With n_gpus > 1 every chunk is
// sharded by chromosome bucket (plan_shards) over the devices, the index is replicated, the per-device bitmaps are OR-ed on
// the host and the per-device {regions, kept pairs} are all-gathered over RCCL (the path's one exchange step).
// keep_store: device 0 keeps ALL regions in HBM (Join B needs them: gffx_hip_lines_test_store).
StreamResult stream_unique_roots(TreeIndexData &index_data, const std::string &bed_path, OverlapMode mode, bool invert, bool verbose,
                                 size_t threads, int device, int n_gpus, bool keep_store) {
    StreamResult res;
    StageTimer sub{verbose};
    // BGZF-compressed, or GFFX_BED_DEVICE=1: the device reader's rows (bed.cpp) enter below as parsed chunks, a second
    // producer beside ChunkParser
    const bool device_rows = bed::route(bed_path) == bed::Route::Device;
    MappedFile f(bed_path);
    const std::string_view text = f.view();
    const SeqidTable seqids(index_data.seqid_to_num);
    std::optional<ChunkParser> parser;
    if (!device_rows) parser.emplace(text, seqids, threads);
    DeviceSet devs = DeviceSet::resolve(device, n_gpus);
    const size_t D = devs.size();
    if (verbose) {  // (only to tell the process's one-off HIP costs from the index's in the stage timers)
        (void)gffx_hip_warmup(devs[0]);
        sub.lap("  HIP runtime + context + code objects");
    }
    index_data.ensure_device(devs[0]);
    std::vector<gffx_hip_index *> ix(D);
    for (size_t d = 0; d < D; ++d) ix[d] = devs.index_on(d, index_data.device_index.get());
    sub.lap("  index upload");
    const uint32_t n_seq = static_cast<uint32_t>(index_data.num_to_seqid.size());
    std::vector<uint32_t> all_rows;  // device_rows: the file's rows (device -> host -> region stores, as BAM and SAM rows travel)
    if (device_rows) {
        all_rows = bed::read_rows(bed_path, index_data.seqid_to_num, bed::kIntersect, devs[0], verbose);
        sub.lap("  BED rows read on the device");
    }
    const size_t n_all = all_rows.size() / 3, per_chunk = kChunkBytes / kMinRowBytes;
    const size_t chunk_rows = device_rows ? std::min(per_chunk, std::max<size_t>(n_all, 1)) + 16
                                          : std::min(kChunkBytes, std::max<size_t>(text.size(), 1)) / kMinRowBytes + 16;
    Lanes lanes = create_lanes(devs, ix, chunk_rows, !keep_store ? 0 : device_rows ? n_all + 16 : text.size() / kMinRowBytes + 16);
    size_t served = 0;
    auto next_chunk = [&]() {
        if (!device_rows) return parser->next();
        ChunkParser::Parsed pc;
        const size_t take = std::min(chunk_rows - 16, n_all - served);
        pc.piece.emplace_back(all_rows.begin() + 3 * served, all_rows.begin() + 3 * (served + take));
        served += take;
        pc.last = served == n_all;
        return pc;
    };
    sub.lap("  region stores + batches");
    res.knobs = knobs_json(ix[0], lanes.batch[0].get());
    res.has_regions.assign(n_seq, 0);
    double t_fill = 0;
    for (size_t chunk = 0;; ++chunk) {
        const int k = static_cast<int>(chunk & 1);
        ChunkParser::Parsed pc = next_chunk();
        const auto t1 = std::chrono::steady_clock::now();
        wait_staging(lanes, k);
        std::vector<uint64_t> n_dev(D, 0);
        if (D == 1) {
            n_dev[0] = fill_one_device(pc.piece, gffx_hip_regions_staging(lanes.store[0].get(), k), n_seq, keep_store, res.has_regions);
        } else {
            std::vector<uint32_t *> stage(D);
            for (size_t d = 0; d < D; ++d) stage[d] = gffx_hip_regions_staging(lanes.store[d].get(), k);
            scatter_chunk_by_bucket(pc.piece, n_seq, keep_store, stage, n_dev, res.has_regions);
        }
        t_fill += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        if (parser) parser->recycle(std::move(pc.piece));  // the rows are in the staging buffers: the parser may fill these vectors again
        res.n_regions += launch_chunk(lanes, k, n_dev, keep_store, mode, invert, res.wide_form_passes);
        if (pc.last) break;
    }
    const double t_parse = parser ? parser->finish() : 0;  // (it pushed its last chunk)
    if (verbose && parser) {
        std::fprintf(stderr, "[TIMER] [run]   BED text parsing (host threads) took %.3f ms\n", t_parse);
        std::fprintf(stderr, "[TIMER] [run]   filling the pinned staging buffers took %.3f ms\n", t_fill);
    }
    collect_results(lanes, devs, index_data.device_index.get(), verbose, sub, res);
    if (keep_store) res.store = std::move(lanes.store[0]);
    return res;
}

}  // namespace gffx::commands::intersect
