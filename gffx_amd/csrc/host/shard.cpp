// shard.cpp -- `gffx intersect --gpus N`: chromosome-bucket sharding of the BED rows over the devices (no HIP call in this file)
#include <algorithm>

#include "intersect_internal.hpp"

namespace gffx::commands::intersect {

// ---- chromosome-bucket sharding of one chunk of regions over the devices (the reference buckets by seqid first:
// intersect.rs:114-120).  Port of gffx_amd/shard.py::plan_shards: whole buckets by LPT (largest first onto the least
// loaded device), a bucket that would overshoot the ideal load is split and the remainder goes back into the pool.
std::vector<std::vector<ShardSlice>> plan_shards(const std::vector<uint64_t> &bucket_sizes, size_t n_ranks, double tolerance) {
    std::vector<std::vector<ShardSlice>> plan(std::max<size_t>(n_ranks, 1));
    uint64_t total = 0;
    for (uint64_t x : bucket_sizes) total += x;
    if (!total || n_ranks == 0) return plan;
    const uint64_t ideal = (total + n_ranks - 1) / n_ranks;
    const uint64_t slack = std::max<uint64_t>(1, static_cast<uint64_t>(ideal * tolerance));
    // pending pieces: largest first, ties by chr, then lo (Python's tuple order on (-size, chr, lo, hi))
    using Piece = std::tuple<uint64_t, uint32_t, uint64_t, uint64_t>;  // size, chr, lo, hi
    auto piece_less = [](const Piece &x, const Piece &y) {
        if (std::get<0>(x) != std::get<0>(y)) return std::get<0>(x) < std::get<0>(y);
        if (std::get<1>(x) != std::get<1>(y)) return std::get<1>(x) > std::get<1>(y);
        return std::get<2>(x) > std::get<2>(y);
    };
    std::vector<Piece> pend;
    for (uint32_t c = 0; c < bucket_sizes.size(); ++c)
        if (bucket_sizes[c]) pend.emplace_back(bucket_sizes[c], c, 0, bucket_sizes[c]);
    std::make_heap(pend.begin(), pend.end(), piece_less);
    using Load = std::pair<uint64_t, size_t>;  // load, rank: least loaded first, ties by rank
    auto load_greater = [](const Load &x, const Load &y) { return x > y; };
    std::vector<Load> loads;
    for (size_t r = 0; r < n_ranks; ++r) loads.emplace_back(0, r);
    std::make_heap(loads.begin(), loads.end(), load_greater);
    while (!pend.empty()) {
        std::pop_heap(pend.begin(), pend.end(), piece_less);
        const auto [sz, c, lo, hi] = pend.back();
        pend.pop_back();
        std::pop_heap(loads.begin(), loads.end(), load_greater);
        const auto [load, r] = loads.back();
        loads.pop_back();
        const uint64_t room = ideal > load ? ideal - load : 0;
        if (sz > room + slack && room > slack) {  // split: fill this device up to the ideal, the rest returns to the pool
            plan[r].push_back({c, lo, lo + room});
            pend.emplace_back(sz - room, c, lo + room, hi);
            std::push_heap(pend.begin(), pend.end(), piece_less);
            loads.emplace_back(load + room, r);
        } else {
            plan[r].push_back({c, lo, hi});
            loads.emplace_back(load + sz, r);
        }
        std::push_heap(loads.begin(), loads.end(), load_greater);
    }
    for (auto &pl : plan)
        std::sort(pl.begin(), pl.end(), [](const ShardSlice &x, const ShardSlice &y) { return std::tie(x.chr, x.lo, x.hi) < std::tie(y.chr, y.lo, y.hi); });
    return plan;
}

// One parsed chunk of a `--gpus N` run -> the devices' staging buffers: bucket sizes of the chunk, the plan (plan_shards:
// chromosome buckets placed by LPT, a bucket that overshoots is split; commands/intersect.rs:114-120 buckets by seqid), then the
// rows are scattered.  W <= 16 workers take CONTIGUOUS runs of the parser's pieces (file order), so a row's rank inside its
// seqid's bucket is (rows of the seqid in earlier workers) + (rows seen so far by this worker): one exclusive prefix over the
// workers, O(n_seq x W) work and memory per chunk whatever the number of pieces (a draft assembly has 10^5 seqids).
// stage[d]: room for the chunk's rows; n_dev[d] (zero on entry) = rows that went to device d; keep_all: device 0 also gets EVERY
// row, as [share 0 | share 1 | ...] (Join B needs all regions on one device).  No HIP call in here: tests/test_sanitizers_cpu.py
// drives it under ThreadSanitizer through gffx_host_shard_bed_file.
void scatter_chunk_by_bucket(const std::vector<std::vector<uint32_t>> &piece, uint32_t n_seq, bool keep_all, const std::vector<uint32_t *> &stage,
                             std::vector<uint64_t> &n_dev, std::vector<char> &has_regions) {
    const size_t D = stage.size(), T = piece.size();
    if (!T || !D) return;
    const size_t W = std::min<size_t>(T, 16);
    auto first_piece = [&](size_t w) { return T * w / W; };
    std::vector<std::vector<uint64_t>> cnt(W, std::vector<uint64_t>(n_seq, 0));
    parallel_for(W, W, [&](size_t w) {
        for (size_t t = first_piece(w); t < first_piece(w + 1); ++t)
            for (size_t i = 0; i < piece[t].size(); i += 3) cnt[w][piece[t][i]]++;
    });
    std::vector<uint64_t> size(n_seq, 0);
    for (uint32_t c = 0; c < n_seq; ++c) {
        uint64_t acc = 0;
        for (size_t w = 0; w < W; ++w) {  // cnt[w][c] becomes the rank of worker w's first row of seqid c
            const uint64_t n = cnt[w][c];
            cnt[w][c] = acc;
            acc += n;
        }
        size[c] = acc;
        has_regions[c] |= acc != 0;
    }
    const auto plan = plan_shards(size, D);
    // per seqid: its slices as (lo, hi, device, offset inside the device's share)
    struct Dest {
        uint64_t lo, hi, off;
        uint32_t d;
    };
    std::vector<std::vector<Dest>> dest(n_seq);
    for (size_t d = 0; d < D; ++d)
        for (const ShardSlice &sl : plan[d]) {
            dest[sl.chr].push_back({sl.lo, sl.hi, n_dev[d], static_cast<uint32_t>(d)});
            n_dev[d] += sl.hi - sl.lo;
        }
    for (auto &v : dest) std::sort(v.begin(), v.end(), [](const Dest &x, const Dest &y) { return x.lo < y.lo; });
    // device 0's store keeps everything when Join B follows: its chunk is [share 0 | share 1 | ...]
    std::vector<uint64_t> all_base(D + 1, 0);
    for (size_t d = 0; d < D; ++d) all_base[d + 1] = all_base[d] + n_dev[d];
    parallel_for(W, W, [&](size_t w) {
        std::vector<uint64_t> &rank = cnt[w];  // bucket rank of this worker's next row of the seqid (file order)
        for (size_t t = first_piece(w); t < first_piece(w + 1); ++t)
            for (size_t i = 0; i < piece[t].size(); i += 3) {
                const uint32_t c = piece[t][i];
                const uint64_t p = rank[c]++;
                const std::vector<Dest> &v = dest[c];
                size_t j = 0;
                while (j + 1 < v.size() && p >= v[j].hi) ++j;
                const uint64_t at = v[j].off + (p - v[j].lo);
                const uint32_t d = v[j].d;
                if (d != 0 || !keep_all) std::copy(piece[t].begin() + i, piece[t].begin() + i + 3, stage[d] + 3 * at);
                if (keep_all) std::copy(piece[t].begin() + i, piece[t].begin() + i + 3, stage[0] + 3 * (all_base[d] + at));
            }
    });
}

// The host half of `gffx intersect --gpus N` without a device: the BED file parsed chunk by chunk on the worker pool, every
// chunk scattered by chromosome bucket into plain memory; per device the rows it would have received, chunk after chunk
// (device 0 with keep_all: every row, each chunk as [share 0 | share 1 | ...]).
std::vector<std::vector<uint32_t>> shard_bed_file_host(const std::string &bed_path, const std::unordered_map<std::string, uint32_t> &seqid_map,
                                                       size_t threads, size_t chunk_bytes, size_t n_dev, bool keep_all) {
    MappedFile f(bed_path);
    const std::string_view text = f.view();
    const SeqidTable seqids(seqid_map);
    uint32_t n_seq = 0;
    for (const auto &kv : seqid_map) n_seq = std::max(n_seq, kv.second + 1);
    WorkerPool workers(std::min<size_t>(std::max<size_t>(threads, 1), 64) - 1);
    std::vector<std::vector<uint32_t>> piece, out(n_dev);
    std::vector<char> has(n_seq, 0);
    for_each_line_chunk(text, chunk_bytes, [&](size_t pos, size_t z, bool last) {
        parse_bed_pieces(text, pos, z, last, seqids, threads, piece, &workers);
        size_t rows = 0;
        for (const auto &v : piece) rows += v.size() / 3;
        std::vector<std::vector<uint32_t>> buf(n_dev, std::vector<uint32_t>(3 * rows));
        std::vector<uint32_t *> stage(n_dev);
        for (size_t d = 0; d < n_dev; ++d) stage[d] = buf[d].data();
        std::vector<uint64_t> got(n_dev, 0);
        scatter_chunk_by_bucket(piece, n_seq, keep_all, stage, got, has);
        for (size_t d = 0; d < n_dev; ++d) out[d].insert(out[d].end(), buf[d].begin(), buf[d].begin() + 3 * ((d == 0 && keep_all) ? rows : got[d]));
        return true;
    });
    return out;
}

}  // namespace gffx::commands::intersect
