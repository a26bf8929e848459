// coverage.cpp -- `gffx coverage` with a BED source over the C-ABI (reference: commands/coverage.rs).
//   collect_by_root_from_bed    coverage.rs:208-275   BED rows -> per root the regions that hit it   -> Join A (root bitmap)
//   finalize_compute_breadth    coverage.rs:383-431   per root: merge_intervals + compute_breadth_for_root
//   compute_breadth_for_root    coverage.rs:277-378   per ID: |merged coverage ∩ union of the ID's lines|, extents
//   write_breadth_results       coverage.rs:452-485   "id\tchr\tstart\tend\tbreadth\tfraction"
// The per-root merged coverage is only needed for segments that stick out of their root's interval; for a segment
// inside it, any region that overlaps the segment hits the root, so the union of ALL regions of the seqid gives the
// same covered bases.  ONE pass over the rows serves both: they go to the devices in batches (round robin with --gpus N,
// one host thread per device, each batch uploaded once into a region store), Join A sets the root bitmap from the resident
// rows and gffx_hip_union_add_store folds the same rows into the device's union.  The bitmaps are OR-ed on the host, the
// other devices' spans (they are small) are folded into device 0's union, and the segments are evaluated once there.
// The rare segments that stick out need the root's OWN merged list.  Which roots can have such a segment is a property of
// the GFF alone (a line of the block outside the root's one interval), so a second, small index of just those roots rides
// along: Join A with root_fids + offsets over the same resident batches pairs rows with them, the host gathers the paired
// rows per root and merges them -- exactly the reference's list (coverage.rs:258-268, :401), with work proportional to the
// pairs instead of rows x such blocks.
// --mean-depth adds a third consumer of the resident batch, a pileup (include/gffx_hip.h "pileup"): the segments of ALL
// blocks are built before the rows stream (which blocks are hit is known only at the end) and stay on every device, each batch
// adds the bases its rows lay on them, and the per-device totals are added here as integers.  Without the flag none of this runs.
// --thresholds / --bedgraph add a fourth, a depth profile (include/gffx_hip.h "depth profile"): every batch is folded into
// the device's canonical points, the points of devices 1 .. N-1 travel to device 0's profile like the spans, and there each threshold T
// becomes a union "depth >= T" on the device against which the segments of the hit blocks are evaluated by the same kernel that serves
// `breadth`.  The depth is that of ALL rows of the segment's seqid (its group's chrom column), as for --mean-depth.  Without the flags
// none of this runs: no object, no kernel, the same bytes out.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>

#include "gffx.hpp"
#include "source_read.hpp"

namespace gffx::commands::coverage {

namespace {

using Span = std::pair<uint32_t, uint32_t>;

// coverage.rs:92-109 merge_intervals: sort by start, merge while s <= current end
std::vector<Span> merge_intervals(std::vector<Span> v) {
    if (v.empty()) return v;
    std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.first < b.first; });
    std::vector<Span> out;
    uint32_t cs = v[0].first, ce = v[0].second;
    for (size_t i = 1; i < v.size(); ++i) {
        if (v[i].first <= ce) {
            ce = std::max(ce, v[i].second);
        } else {
            out.emplace_back(cs, ce);
            cs = v[i].first;
            ce = v[i].second;
        }
    }
    out.emplace_back(cs, ce);
    return out;
}

uint64_t covered(const std::vector<Span> &cov, uint32_t a, uint32_t b) {  // cov sorted and disjoint
    uint64_t t = 0;
    for (const Span &c : cov) {
        if (c.first >= b) break;
        const uint32_t s = std::max(a, c.first), e = std::min(b, c.second);
        if (e > s) t += e - s;
    }
    return t;
}

struct Seg {
    uint32_t group, start, end;
    bool fast;  // (the caller's: evaluated on the device against the union of all rows)
};

// Per (block, ID) group of `blocks` (ascending: file order): the union of the group's lines as disjoint segments, block after
// block and inside a block in line order; built on `threads` host threads over contiguous shares of the list and concatenated in
// order.  g_min / g_max / g_hit (all three or none): the group's extent over ALL its lines (coverage.rs:345-346), and that its
// block was in the list -- a group belongs to one block, so the shares write disjoint entries.
std::vector<Seg> segments_of_blocks(const depth::BlockTable &t, const std::vector<uint32_t> &blocks, size_t threads, std::vector<uint32_t> *g_min,
                                    std::vector<uint32_t> *g_max, std::vector<uint8_t> *g_hit) {
    const size_t parts = blocks.size() < 4096 ? 1 : std::max<size_t>(1, std::min<size_t>(threads, 64));
    std::vector<std::vector<Seg>> piece(parts);
    parallel_for(parts, parts, [&](size_t p) {
        std::vector<Seg> &segs = piece[p];
        std::vector<Span> lines;
        for (size_t k = blocks.size() * p / parts; k < blocks.size() * (p + 1) / parts; ++k) {
            const uint32_t b = blocks[k];
            uint64_t l = t.block_line_off[b];
            const uint64_t le = t.block_line_off[b + 1];
            while (l < le) {
                const uint32_t g = t.line_group[l];
                lines.clear();
                for (; l < le && t.line_group[l] == g; ++l) {
                    lines.emplace_back(t.line_start[l], t.line_end[l]);
                    if (g_min) {
                        (*g_min)[g] = std::min((*g_min)[g], t.line_start[l]);
                        (*g_max)[g] = std::max((*g_max)[g], t.line_end[l]);
                    }
                }
                if (g_hit) (*g_hit)[g] = 1;
                for (const Span &sgm : merge_intervals(lines)) segs.push_back(Seg{g, sgm.first, sgm.second, false});
            }
        }
    });
    if (parts == 1) return std::move(piece[0]);
    std::vector<Seg> all;
    size_t total = 0;
    for (const auto &v : piece) total += v.size();
    all.reserve(total);
    for (const auto &v : piece) all.insert(all.end(), v.begin(), v.end());
    return all;
}

}  // namespace

void run(const CoverageArgs &args) {
    const bool verbose = args.verbose;
    StageTimer timer{verbose};
    const index_loader::GofMap gof = index_loader::load_gof(args.input);  // :501
    const MappedFile gff = map_file_or(args.input, "Cannot open GFF file: \"" + args.input + "\"");  // :502-503
    DeviceWarmup warm(args.device);  // (the runtime comes up beside the loaders and the BED parser)
    TreeIndexData index_data = TreeIndexData::load_tree_index(args.input);  // :511
    const depth::SourceKind kind = depth::source_kind(args.source);  // coverage.rs:520-541
    const size_t threads = capped_threads(args.threads);
    const depth::SourceRows src = depth::read_source_rows(kind, args.source, index_data.seqid_to_num, threads, args.device, verbose, warm);
    const size_t n_regions = src.n_rows;
    if (verbose) std::fprintf(stderr, "[INFO] %zu %s rows kept\n", n_regions, depth::source_label(kind));
    timer.lap(depth::source_lap(kind, true));

    const std::vector<uint32_t> &thresholds = args.thresholds;
    const bool want_profile = !thresholds.empty() || args.bedgraph.has_value();
    std::string out = args.mean_depth ? "id\tchr\tstart\tend\tbreadth\tfraction\tbases\tlength\tmean_depth" : "id\tchr\tstart\tend\tbreadth\tfraction";  // :463
    for (const uint32_t T : thresholds) out += "\tbases_ge" + std::to_string(T) + "\tfraction_ge" + std::to_string(T);
    out.push_back('\n');
    std::string bedgraph;  // (--bedgraph) an empty source gives an empty file
    size_t written = 0;
    if (n_regions) {
        const depth::BlockTable t = depth::load_or_build_block_table(args.input, gof, gff.view(), threads, verbose);
        timer.lap("Line table (image or parse)");
        // the tree intervals of every root_fid (several when root lines share an ID)
        const uint32_t n_seq = static_cast<uint32_t>(index_data.chr_offsets.size() - 1);
        std::unordered_map<uint32_t, std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>> ivs;  // fid -> (seq, start, end)
        for (uint32_t c = 0; c < n_seq; ++c)
            for (uint32_t i = index_data.chr_offsets[c]; i < index_data.chr_offsets[c + 1]; ++i)
                ivs[index_data.root_fid[i]].emplace_back(c, index_data.start[i], index_data.end[i]);
        std::vector<uint32_t> block_fid(t.block_line_off.size() - 1, 0xFFFFFFFFu);
        for (uint32_t f = 0; f < t.block_of_fid.size(); ++f)
            if (t.block_of_fid[f] != 0xFFFFFFFFu) block_fid[t.block_of_fid[f]] = f;
        // Roots that CAN have a segment outside their interval: every block but those whose root has one interval that holds
        // all lines of the block (a superset of the blocks the exact test below finds: a segment is a union of lines).
        std::vector<uint8_t> side_fid(t.block_of_fid.size(), 0);
        for (uint32_t b = 0; b + 1 < t.block_line_off.size(); ++b) {
            if (block_fid[b] == 0xFFFFFFFFu) continue;
            const auto it = ivs.find(block_fid[b]);
            if (it == ivs.end()) continue;  // (no interval: never hit)
            bool all_inside = it->second.size() == 1;
            if (all_inside) {
                const uint32_t rs = std::get<1>(it->second[0]), re = std::get<2>(it->second[0]);
                for (uint64_t l = t.block_line_off[b]; l < t.block_line_off[b + 1] && all_inside; ++l)
                    all_inside = t.line_start[l] >= rs && t.line_end[l] <= re;
            }
            if (!all_inside) side_fid[block_fid[b]] = 1;
        }
        std::vector<uint32_t> side_off(n_seq + 1, 0), side_start, side_end, side_root;
        for (uint32_t c = 0; c < n_seq; ++c) {
            for (uint32_t i = index_data.chr_offsets[c]; i < index_data.chr_offsets[c + 1]; ++i) {
                const uint32_t f = index_data.root_fid[i];
                if (f < side_fid.size() && side_fid[f]) {
                    side_start.push_back(index_data.start[i]);
                    side_end.push_back(index_data.end[i]);
                    side_root.push_back(f);
                }
            }
            side_off[c + 1] = static_cast<uint32_t>(side_start.size());
        }
        const bool have_side = !side_start.empty();
        std::vector<uint32_t> group_block(t.group_id.size(), 0);
        for (uint32_t b = 0; b + 1 < t.block_line_off.size(); ++b)
            for (uint64_t l = t.block_line_off[b]; l < t.block_line_off[b + 1]; ++l) group_block[t.line_group[l]] = b;

        // --mean-depth: the segments of every block, and the ones whose seqid the index knows as the pileup's arrays (a chrom the
        // index does not know has no rows: 0 bases).  A segment's seqid is its group's chrom column, not its root's.  Built on
        // host threads of their own WHILE the devices come up below (runtime, index upload, stores, batches): every device's
        // thread waits for `segs_ready` just before it creates its pileup, the last thing it sets up.
        std::vector<Seg> all_segs;
        std::vector<uint32_t> chrom_num, p_seq, p_start, p_end;
        std::shared_future<void> segs_ready;
        if (args.mean_depth) segs_ready = std::async(std::launch::async, [&] {
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<uint32_t> all_blocks(t.block_line_off.size() - 1);
            for (uint32_t b = 0; b < all_blocks.size(); ++b) all_blocks[b] = b;
            all_segs = segments_of_blocks(t, all_blocks, threads, nullptr, nullptr, nullptr);
            chrom_num.assign(t.chroms.size(), 0xFFFFFFFFu);
            for (size_t k = 0; k < t.chroms.size(); ++k) {
                const auto it = index_data.seqid_to_num.find(t.chroms[k]);
                if (it != index_data.seqid_to_num.end() && it->second < n_seq) chrom_num[k] = it->second;
            }
            p_seq.reserve(all_segs.size()), p_start.reserve(all_segs.size()), p_end.reserve(all_segs.size());
            for (const Seg &sg : all_segs) {
                const uint32_t c = chrom_num[t.group_chrom[sg.group]];
                if (c == 0xFFFFFFFFu) continue;
                p_seq.push_back(c), p_start.push_back(sg.start), p_end.push_back(sg.end);
            }
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (verbose)
                std::fprintf(stderr, "[INFO] pileup: %zu segments of all blocks (%zu on seqids of the index)\n[TIMER] [run] Segments of all blocks (pileup; beside the device set-up) took %.3f ms\n",
                             all_segs.size(), p_seq.size(), ms);
            g_run_stats.stage("Segments of all blocks (pileup; beside the device set-up)", ms);
        }).share();

        // --gpus N: the rows go to the devices in batches, round robin (the root bitmap is an OR and the union does not depend
        // on how the rows are grouped, so any partition gives the same rows out); one host thread drives each device
        warm.wait();
        DeviceSet devs = DeviceSet::resolve(args.device, args.gpus);
        const size_t D = devs.size();
        index_data.ensure_device(devs[0]);
        gffx_hip_index *ix0 = index_data.device_index.get();
        const uint64_t n_words = (gffx_hip_index_n_roots(ix0) + 63) / 64 + 1;
        using RootRows = std::unordered_map<uint32_t, std::vector<Span>>;  // root_fid -> the rows that hit it
        struct PerDevice {
            RegionsHandle store;  // two pinned staging buffers + a ring of two batch slots in HBM
            BatchHandle b[2], c[2];  // Join A on the index (root bitmap) / on the index of the roots above (pairs)
            IndexHandle side;
            UnionHandle u;
            PileupHandle p;
            ProfileHandle prof;  // (--thresholds / --bedgraph)
            std::vector<uint64_t> p_off;  // ... the device's points (devices 1 .. N-1: they travel to device 0's profile)
            std::vector<uint32_t> p_pos, p_depth;
            double profile_ms = 0, profile_stage_ms[4] = {0, 0, 0, 0};
            uint64_t profile_folds = 0;
            std::vector<uint64_t> bases;  // (--mean-depth) the device's totals, one per pileup segment
            double pileup_ms = 0, pileup_stage_ms[4] = {0, 0, 0, 0};
            uint64_t pileup_folds = 0;
            std::vector<uint64_t> words;
            RootRows root_rows;
            std::vector<uint64_t> u_off;
            std::vector<uint32_t> us, ue;
            uint64_t rows = 0, spans = 0, side_pairs = 0;
            double union_ms = 0;
        };
        std::vector<PerDevice> pd(D);
        const size_t kBatch = source::batch_rows_from_env("GFFX_COVERAGE_BATCH_ROWS");
        const size_t cap = std::min(n_regions, kBatch);
        parallel_for(D, D, [&](size_t d) {
            PerDevice &P = pd[d];
            gffx_hip_index *ix = devs.index_on(d, ix0);
            if (have_side &&
                gffx_hip_index_create(n_seq, side_off.data(), side_start.data(), side_end.data(), side_root.data(), devs[d], OutPtr(P.side)) != GFFX_OK)
                hip_fail("gffx_hip_index_create");
            if (gffx_hip_union_create(devs[d], n_seq, OutPtr(P.u)) != GFFX_OK) hip_fail("gffx_hip_union_create");
            if (gffx_hip_regions_create(devs[d], 0, cap, 0, OutPtr(P.store)) != GFFX_OK) hip_fail("gffx_hip_regions_create");
            for (int k = 0; k < 2; ++k) {
                if (gffx_hip_batch_create(ix, cap, OutPtr(P.b[k])) != GFFX_OK) hip_fail("gffx_hip_batch_create");
                if (have_side && gffx_hip_batch_create(P.side.get(), cap, OutPtr(P.c[k])) != GFFX_OK) hip_fail("gffx_hip_batch_create");
            }
            if (args.mean_depth) {
                std::shared_future<void>(segs_ready).get();  // (a copy per thread; rethrows what the builder threw)
                if (gffx_hip_pileup_create(devs[d], n_seq, p_seq.size(), p_seq.data(), p_start.data(), p_end.data(), OutPtr(P.p)) != GFFX_OK)
                    hip_fail("gffx_hip_pileup_create");
            }
            if (want_profile && gffx_hip_profile_create(devs[d], n_seq, OutPtr(P.prof)) != GFFX_OK) hip_fail("gffx_hip_profile_create");
            P.words.assign(n_words, 0);
            bool used[2] = {false, false};
            size_t rows_in[2] = {0, 0};
            std::vector<uint32_t> counts, fids;
            std::vector<uint64_t> offsets;
            // submit(k, n): the passes over the n rows resident in slot k
            auto submit = [&](int k, size_t n) {
                if (gffx_hip_batch_set_regions_store(P.b[k].get(), P.store.get(), k, 0, n) != GFFX_OK) hip_fail("set_regions_store");
                const uint32_t flags = static_cast<uint32_t>(GFFX_OUT_ROOT_BITMAP) | static_cast<uint32_t>(GFFX_OUT_NO_COUNTS) |
                                       (used[k] ? static_cast<uint32_t>(GFFX_OUT_BITMAP_KEEP) : 0u);  // (the bitmap accumulates across batches)
                if (gffx_hip_batch_run(P.b[k].get(), GFFX_MODE_OVERLAP, 0, flags, GFFX_STRATEGY_AUTO) != GFFX_OK) hip_fail("gffx_hip_batch_run");
                if (have_side) {
                    if (gffx_hip_batch_set_regions_store(P.c[k].get(), P.store.get(), k, 0, n) != GFFX_OK) hip_fail("set_regions_store");
                    if (gffx_hip_batch_run(P.c[k].get(), GFFX_MODE_OVERLAP, 0, GFFX_OUT_FIDS | GFFX_OUT_OFFSETS, GFFX_STRATEGY_AUTO) != GFFX_OK)
                        hip_fail("gffx_hip_batch_run");
                }
                used[k] = true;
                rows_in[k] = n;
                // (--mean-depth) the same resident rows into the pileup: returns when they are read, its fold runs beside the union's
                if (args.mean_depth && gffx_hip_pileup_add_store(P.p.get(), P.store.get(), k, 0, n) != GFFX_OK) hip_fail("gffx_hip_pileup_add_store");
                // (--thresholds / --bedgraph) ... and into the depth profile, on its own stream: returns when they are read
                if (want_profile && gffx_hip_profile_add_store(P.prof.get(), P.store.get(), k, 0, n) != GFFX_OK) hip_fail("gffx_hip_profile_add_store");
                // the same resident rows into the union (on the union's own stream, beside Join A; returns when they are read)
                if (gffx_hip_union_add_store(P.u.get(), P.store.get(), k, 0, n) != GFFX_OK) hip_fail("gffx_hip_union_add_store");
            };
            // finish(k): the passes over slot k are through; the rows paired with a root of the side index are gathered from
            // staging buffer k, which still holds the batch.
            auto finish = [&](int k) {
                if (gffx_hip_batch_wait(P.b[k].get()) != GFFX_OK) hip_fail("query_features");
                if (!have_side) return;
                if (gffx_hip_batch_wait(P.c[k].get()) != GFFX_OK) hip_fail("query_features");
                const uint64_t total = gffx_hip_batch_total_hits(P.c[k].get());
                if (!total) return;
                const size_t n = rows_in[k];
                counts.resize(n), offsets.resize(n + 1), fids.resize(total);
                if (gffx_hip_batch_copy_counts(P.c[k].get(), counts.data()) != GFFX_OK) hip_fail("copy_counts");
                if (gffx_hip_batch_copy_offsets(P.c[k].get(), offsets.data()) != GFFX_OK) hip_fail("copy_offsets");
                if (gffx_hip_batch_copy_fids(P.c[k].get(), fids.data()) != GFFX_OK) hip_fail("copy_fids");
                const uint32_t *stage = gffx_hip_regions_staging(P.store.get(), k);
                for (size_t j = 0; j < n; ++j) {
                    if (!counts[j]) continue;
                    uint32_t *f = fids.data() + offsets[j], *fe = f + counts[j];
                    std::sort(f, fe);  // a region once per root (coverage.rs:263-266), also when root lines share an ID
                    fe = std::unique(f, fe);
                    for (; f < fe; ++f) P.root_rows[*f].emplace_back(stage[3 * j + 1], stage[3 * j + 2]);
                }
                P.side_pairs += total;
            };
            const size_t fill_threads = std::max<size_t>(1, std::min<size_t>(threads / D, 8));
            P.rows = depth::run_row_batches(src, P.store.get(), d, D, kBatch, fill_threads, submit, finish);
            std::vector<uint64_t> tmp(n_words, 0);
            for (int k = 0; k < 2; ++k) {
                if (!used[k]) continue;
                if (gffx_hip_batch_copy_root_bitmap(P.b[k].get(), tmp.data(), tmp.size()) != GFFX_OK) hip_fail("copy_root_bitmap");
                for (size_t w = 0; w < n_words; ++w) P.words[w] |= tmp[w];
            }
            P.spans = gffx_hip_union_n_spans(P.u.get());
            if (d > 0) {  // the spans travel to device 0's union
                if (gffx_hip_union_finish(P.u.get()) != GFFX_OK) hip_fail("gffx_hip_union_finish");
                P.u_off.assign(n_seq + 1, 0);
                P.us.assign(std::max<uint64_t>(P.spans, 1), 0);
                P.ue.assign(std::max<uint64_t>(P.spans, 1), 0);
                if (gffx_hip_union_copy_spans(P.u.get(), P.u_off.data(), P.us.data(), P.ue.data(), nullptr) != GFFX_OK) hip_fail("gffx_hip_union_copy_spans");
            }
            if (gffx_hip_union_stats(P.u.get(), &P.union_ms, nullptr, nullptr) != GFFX_OK) hip_fail("gffx_hip_union_stats");
            if (args.mean_depth) {
                P.bases.assign(std::max<size_t>(p_seq.size(), 1), 0);
                if (gffx_hip_pileup_copy(P.p.get(), P.bases.data()) != GFFX_OK) hip_fail("gffx_hip_pileup_copy");
                if (gffx_hip_pileup_stats(P.p.get(), &P.pileup_ms, nullptr, &P.pileup_folds) != GFFX_OK) hip_fail("gffx_hip_pileup_stats");
                if (gffx_hip_pileup_stage_ms(P.p.get(), &P.pileup_stage_ms[0], &P.pileup_stage_ms[1], &P.pileup_stage_ms[2], &P.pileup_stage_ms[3]) != GFFX_OK)
                    hip_fail("gffx_hip_pileup_stage_ms");
            }
            if (want_profile) {
                gffx_hip_profile *pr = P.prof.get();
                if (d > 0) {  // the points travel to device 0's profile
                    if (gffx_hip_profile_finish(pr) != GFFX_OK) hip_fail("gffx_hip_profile_finish");
                    const uint64_t np = gffx_hip_profile_n_points(pr);
                    P.p_off.assign(n_seq + 1, 0);
                    P.p_pos.assign(std::max<uint64_t>(np, 1), 0);
                    P.p_depth.assign(std::max<uint64_t>(np, 1), 0);
                    if (gffx_hip_profile_copy_points(pr, P.p_off.data(), P.p_pos.data(), P.p_depth.data()) != GFFX_OK) hip_fail("gffx_hip_profile_copy_points");
                }
                if (gffx_hip_profile_stats(pr, &P.profile_ms, nullptr, &P.profile_folds) != GFFX_OK) hip_fail("gffx_hip_profile_stats");
                if (gffx_hip_profile_stage_ms(pr, &P.profile_stage_ms[0], &P.profile_stage_ms[1], &P.profile_stage_ms[2], &P.profile_stage_ms[3]) != GFFX_OK)
                    hip_fail("gffx_hip_profile_stage_ms");
            }
        });
        // merge over the devices: OR of the bitmaps, the spans into device 0's union
        std::vector<uint64_t> words(n_words, 0);
        for (const PerDevice &P : pd)
            for (size_t w = 0; w < n_words; ++w) words[w] |= P.words[w];
        std::vector<uint32_t> hit_roots;  // by_root's key set (coverage.rs:258-268), ascending and unique
        {
            const uint64_t n_roots = gffx_hip_index_n_roots(ix0);
            const uint32_t *sorted_fids = gffx_hip_index_sorted_fids(ix0);
            for (uint64_t i = 0; i < n_roots; ++i)
                if (words[i >> 6] >> (i & 63) & 1) hit_roots.push_back(sorted_fids[i]);
            std::sort(hit_roots.begin(), hit_roots.end());
            hit_roots.erase(std::unique(hit_roots.begin(), hit_roots.end()), hit_roots.end());
        }
        gffx_hip_union *U = pd[0].u.get();
        for (size_t d = 1; d < D; ++d)
            if (gffx_hip_union_add_spans(U, pd[d].u_off.data(), pd[d].us.data(), pd[d].ue.data()) != GFFX_OK) hip_fail("gffx_hip_union_add_spans");
        if (gffx_hip_union_finish(U) != GFFX_OK) hip_fail("gffx_hip_union_finish");
        const uint64_t union_spans = gffx_hip_union_n_spans(U);
        double union_ms = 0;
        uint64_t side_pairs = 0;
        std::vector<uint64_t> counts(2 * D, 0);
        std::string per_device = "[";
        for (size_t d = 0; d < D; ++d) {
            counts[2 * d] = pd[d].rows, counts[2 * d + 1] = pd[d].spans;
            union_ms += pd[d].union_ms;
            side_pairs += pd[d].side_pairs;
            per_device += std::string(d ? ", " : "") + "{\"rows\": " + std::to_string(pd[d].rows) + ", \"spans\": " + std::to_string(pd[d].spans) + "}";
        }
        per_device += "]";
        // the exchange step: per-device {rows, spans} (bitmaps and spans are complete on the host by now)
        if (D > 1) devs.exchange_counts(counts, "rows", "union spans", verbose, /*adopt_gathered=*/false);
        if (verbose)
            std::fprintf(stderr, "[INFO] rows uploaded once: %llu bytes for %zu rows; union of %llu spans (sort + span kernels %.3f ms); %llu pairs with roots that can have outside segments\n",
                         12ull * n_regions, n_regions, (unsigned long long)union_spans, union_ms, (unsigned long long)side_pairs);
        g_run_stats.count("gpus", static_cast<double>(D));
        g_run_stats.count("rows", static_cast<double>(n_regions));
        g_run_stats.count("upload_bytes", 12.0 * static_cast<double>(n_regions));
        g_run_stats.count("union_spans", static_cast<double>(union_spans));
        g_run_stats.count("union_kernels_ms", union_ms);
        g_run_stats.extra("devices", per_device);
        timer.lap("Join A + union build on the device (one upload per batch, kernels, bitmaps and spans D2H)");
        // (--mean-depth) the devices' totals added as integers, then per group: its bases and the bases of its segments
        std::vector<uint64_t> group_bases, group_len;
        if (args.mean_depth) {
            group_bases.assign(t.group_id.size(), 0), group_len.assign(t.group_id.size(), 0);
            double pileup_ms = 0, st[4] = {0, 0, 0, 0};
            size_t pi = 0;
            uint64_t folds = 0;
            for (const Seg &sg : all_segs) {
                if (sg.end > sg.start) group_len[sg.group] += sg.end - sg.start;
                if (chrom_num[t.group_chrom[sg.group]] == 0xFFFFFFFFu) continue;
                for (const PerDevice &P : pd) group_bases[sg.group] += P.bases[pi];
                ++pi;
            }
            for (const PerDevice &P : pd) {
                pileup_ms += P.pileup_ms;
                folds += P.pileup_folds;
                for (int k = 0; k < 4; ++k) st[k] += P.pileup_stage_ms[k];
            }
            if (verbose)
                std::fprintf(stderr, "[INFO] pileup of %zu segments: %llu folds, kernels %.3f ms (keys %.3f, two sorts %.3f, prefix sums %.3f, segments %.3f)\n",
                             p_seq.size(), (unsigned long long)folds, pileup_ms, st[0], st[1], st[2], st[3]);
            g_run_stats.count("pileup_segments", static_cast<double>(p_seq.size()));
            g_run_stats.count("pileup_kernels_ms", pileup_ms);
            g_run_stats.count("pileup_folds", static_cast<double>(folds));
            g_run_stats.count("pileup_keys_ms", st[0]);
            g_run_stats.count("pileup_sorts_ms", st[1]);
            g_run_stats.count("pileup_scan_ms", st[2]);
            g_run_stats.count("pileup_segments_ms", st[3]);
            timer.lap("Pileup (device)");
        }

        // per (block, ID) group of the hit blocks: the union of its lines as disjoint segments, and its extent
        std::vector<uint32_t> seg_seq, seg_start, seg_end;  // the device's share
        std::vector<uint32_t> g_min(t.group_id.size(), 0xFFFFFFFFu), g_max(t.group_id.size(), 0);
        std::vector<uint8_t> g_hit(t.group_id.size(), 0);
        std::vector<uint32_t> hit_blocks;
        for (uint32_t fid : hit_roots)
            if (fid < t.block_of_fid.size() && t.block_of_fid[fid] != 0xFFFFFFFFu) hit_blocks.push_back(t.block_of_fid[fid]);
        std::sort(hit_blocks.begin(), hit_blocks.end());  // file order
        std::vector<Seg> segs = segments_of_blocks(t, hit_blocks, 1, &g_min, &g_max, &g_hit);
        {
            uint32_t cur = 0xFFFFFFFFu;
            const std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> *root_iv = nullptr;
            bool one_seq = false;
            for (Seg &sg : segs) {
                const uint32_t b = group_block[sg.group];
                if (b != cur) {
                    cur = b;
                    root_iv = &ivs[block_fid[b]];
                    one_seq = !root_iv->empty();
                    for (const auto &iv : *root_iv) one_seq = one_seq && std::get<0>(iv) == std::get<0>((*root_iv)[0]);
                }
                bool inside = false;
                if (one_seq)
                    for (const auto &iv : *root_iv) inside = inside || (sg.start >= std::get<1>(iv) && sg.end <= std::get<2>(iv));
                sg.fast = inside;
                if (inside) {
                    seg_seq.push_back(std::get<0>((*root_iv)[0]));
                    seg_start.push_back(sg.start);
                    seg_end.push_back(sg.end);
                }
            }
        }
        if (verbose)
            std::fprintf(stderr, "[INFO] %zu hit blocks, %zu segments (%zu evaluated on the host)\n", hit_blocks.size(),
                         segs.size(), segs.size() - seg_seq.size());
        timer.lap("Segments of the hit blocks");
        // (--thresholds / --bedgraph) the merged profile on device 0; per threshold the bases at depth >= T of every segment of the
        // hit blocks, on the seqid of the segment's group (a chrom the index does not know has no rows: 0), summed per group
        std::vector<std::vector<uint64_t>> group_ge(thresholds.size());
        std::vector<uint64_t> group_seg_len;
        if (want_profile) {
            gffx_hip_profile *pr = pd[0].prof.get();
            for (size_t d = 1; d < D; ++d)
                if (gffx_hip_profile_add_points(pr, pd[d].p_off.data(), pd[d].p_pos.data(), pd[d].p_depth.data()) != GFFX_OK) hip_fail("gffx_hip_profile_add_points");
            if (gffx_hip_profile_finish(pr) != GFFX_OK) hip_fail("gffx_hip_profile_finish");
            const uint64_t n_points = gffx_hip_profile_n_points(pr);
            std::vector<uint32_t> cn(t.chroms.size(), 0xFFFFFFFFu);
            for (size_t k = 0; k < t.chroms.size(); ++k) {
                const auto it = index_data.seqid_to_num.find(t.chroms[k]);
                if (it != index_data.seqid_to_num.end() && it->second < n_seq) cn[k] = it->second;
            }
            std::vector<uint32_t> q_seq, q_start, q_end, q_group;
            group_seg_len.assign(t.group_id.size(), 0);
            for (const Seg &sg : segs) {
                if (sg.end > sg.start) group_seg_len[sg.group] += sg.end - sg.start;
                const uint32_t c = cn[t.group_chrom[sg.group]];
                if (c == 0xFFFFFFFFu) continue;
                q_seq.push_back(c), q_start.push_back(sg.start), q_end.push_back(sg.end), q_group.push_back(sg.group);
            }
            std::vector<uint32_t> ge(std::max<size_t>(q_seq.size(), 1), 0);
            for (size_t k = 0; k < thresholds.size(); ++k) {
                UnionHandle at_least;
                if (gffx_hip_profile_union_at_least(pr, thresholds[k], OutPtr(at_least)) != GFFX_OK) hip_fail("gffx_hip_profile_union_at_least");
                if (gffx_hip_union_segments_covered(at_least.get(), q_seq.size(), q_seq.data(), q_start.data(), q_end.data(), ge.data()) != GFFX_OK)
                    hip_fail("gffx_hip_union_segments_covered");
                group_ge[k].assign(t.group_id.size(), 0);
                for (size_t i = 0; i < q_seq.size(); ++i) group_ge[k][q_group[i]] += ge[i];
            }  // (the handle destroys the union)
            if (args.bedgraph) {
                std::vector<uint64_t> p_off(n_seq + 1, 0);
                std::vector<uint32_t> pos(std::max<uint64_t>(n_points, 1), 0), dep(std::max<uint64_t>(n_points, 1), 0);
                if (gffx_hip_profile_copy_points(pr, p_off.data(), pos.data(), dep.data()) != GFFX_OK) hip_fail("gffx_hip_profile_copy_points");
                for (uint32_t c = 0; c < n_seq; ++c)
                    for (uint64_t i = p_off[c]; i + 1 < p_off[c + 1]; ++i) {  // (a seqid's last point has depth 0)
                        if (!dep[i]) continue;
                        bedgraph += index_data.num_to_seqid[c];
                        bedgraph.push_back('\t');
                        bedgraph += std::to_string(pos[i]);
                        bedgraph.push_back('\t');
                        bedgraph += std::to_string(pos[i + 1]);
                        bedgraph.push_back('\t');
                        bedgraph += std::to_string(dep[i]);
                        bedgraph.push_back('\n');
                    }
            }
            double profile_ms = 0, st[4] = {0, 0, 0, 0};
            uint64_t folds = 0;
            for (const PerDevice &P : pd) {
                profile_ms += P.profile_ms;
                folds += P.profile_folds;
                for (int k = 0; k < 4; ++k) st[k] += P.profile_stage_ms[k];
            }
            if (verbose)
                std::fprintf(stderr, "[INFO] depth profile of %llu points: %llu folds, kernels %.3f ms (events %.3f, sort %.3f, running depth %.3f, points %.3f); %zu thresholds over %zu segments\n",
                             (unsigned long long)n_points, (unsigned long long)folds, profile_ms, st[0], st[1], st[2], st[3], thresholds.size(), q_seq.size());
            g_run_stats.count("profile_points", static_cast<double>(n_points));
            g_run_stats.count("profile_folds", static_cast<double>(folds));
            g_run_stats.count("profile_kernels_ms", profile_ms);
            g_run_stats.count("profile_events_ms", st[0]);
            g_run_stats.count("profile_sort_ms", st[1]);
            g_run_stats.count("profile_scan_ms", st[2]);
            g_run_stats.count("profile_points_ms", st[3]);
            timer.lap("Depth profile (device)");
        }
        // device 0: covered bases of the segments inside their root, under the union of all regions of the seqid
        std::vector<uint32_t> cov_fast(std::max<size_t>(seg_seq.size(), 1), 0);
        if (gffx_hip_union_segments_covered(U, seg_seq.size(), seg_seq.data(), seg_start.data(), seg_end.data(), cov_fast.data()) != GFFX_OK)
            hip_fail("gffx_hip_union_segments_covered");
        timer.lap("Covered bases on the device (segments H2D, kernel, D2H)");
        // host: the segments that stick out of their root, against the root's own merged list (coverage.rs:401) -- the rows
        // Join A paired with the root on the side index, from all devices
        std::vector<uint64_t> breadth(t.group_id.size(), 0);
        std::unordered_map<uint32_t, std::vector<Span>> root_cov;  // block -> merged regions that hit its root
        size_t fi = 0;
        for (const Seg &sg : segs) {
            if (sg.fast) {
                breadth[sg.group] += cov_fast[fi++];
                continue;
            }
            const uint32_t b = group_block[sg.group];
            auto it = root_cov.find(b);
            if (it == root_cov.end()) {
                const uint32_t fid = block_fid[b];
                if (!(fid < side_fid.size() && side_fid[fid])) throw Error("coverage: a segment outside its root in a block that has none");
                std::vector<Span> hit;
                for (PerDevice &P : pd) {
                    const auto rr = P.root_rows.find(fid);
                    if (rr != P.root_rows.end()) hit.insert(hit.end(), rr->second.begin(), rr->second.end());
                }
                it = root_cov.emplace(b, merge_intervals(std::move(hit))).first;
            }
            breadth[sg.group] += covered(it->second, sg.start, sg.end);
        }
        // merge the groups of an ID (coverage.rs:417-428) in block order; a row if length > 0 || breadth > 0 (:372)
        struct Row {
            bool set = false;
            const std::string *chrom = nullptr;
            uint32_t s = 0, e = 0;
            uint64_t b = 0;
        };
        std::vector<Row> rows(t.n_ids());
        std::vector<uint64_t> id_bases(args.mean_depth ? t.n_ids() : 0, 0), id_len(id_bases.size(), 0);  // (--mean-depth; empty without it)
        std::vector<std::vector<uint64_t>> id_ge(thresholds.size(), std::vector<uint64_t>(t.n_ids(), 0));  // (--thresholds)
        std::vector<uint64_t> id_seg_len(thresholds.empty() ? 0 : t.n_ids(), 0);
        std::vector<uint32_t> order;
        for (uint32_t g = 0; g < t.group_id.size(); ++g) {
            if (!g_hit[g]) continue;
            const uint64_t length = g_max[g] > g_min[g] ? g_max[g] - g_min[g] : 0;
            if (length == 0 && breadth[g] == 0) continue;
            Row &r = rows[t.group_id[g]];
            if (!r.set) {
                r.set = true;
                r.chrom = &t.chroms[t.group_chrom[g]];
                r.s = g_min[g];
                r.e = g_max[g];
                r.b = breadth[g];
                order.push_back(t.group_id[g]);
            } else {
                r.s = std::min(r.s, g_min[g]);
                r.e = std::max(r.e, g_max[g]);
                r.b += breadth[g];
            }
            if (args.mean_depth) id_bases[t.group_id[g]] += group_bases[g], id_len[t.group_id[g]] += group_len[g];
            if (!thresholds.empty()) {
                id_seg_len[t.group_id[g]] += group_seg_len[g];
                for (size_t k = 0; k < thresholds.size(); ++k) id_ge[k][t.group_id[g]] += group_ge[k][g];
            }
        }
        append_rows_parallel(out, order.size(), threads, [&](size_t k, std::string &o) {  // coverage.rs:465-473
            const uint32_t i = order[k];
            const Row &r = rows[i];
            const uint64_t length = r.e > r.s ? r.e - r.s : 0;
            const double fraction = length > 0 ? static_cast<double>(r.b) / static_cast<double>(length) : 0.0;
            char num[64];
            o += t.id(i);
            o.push_back('\t');
            o += *r.chrom;
            o.push_back('\t');
            o += std::to_string(r.s);
            o.push_back('\t');
            o += std::to_string(r.e);
            o.push_back('\t');
            o += std::to_string(r.b);
            if (args.mean_depth) {
                char more[128];
                const uint64_t bases = id_bases[i], len = id_len[i];
                const double mean = len > 0 ? static_cast<double>(bases) / static_cast<double>(len) : 0.0;
                std::snprintf(more, sizeof more, "\t%.6f\t%llu\t%llu\t%.6f", fraction, static_cast<unsigned long long>(bases), static_cast<unsigned long long>(len), mean);
                o += more;
            } else {
                std::snprintf(num, sizeof num, "\t%.6f", fraction);
                o += num;
            }
            for (size_t k = 0; k < thresholds.size(); ++k) {
                const uint64_t ge = id_ge[k][i], len = id_seg_len[i];
                std::snprintf(num, sizeof num, "\t%llu\t%.6f", static_cast<unsigned long long>(ge), len > 0 ? static_cast<double>(ge) / static_cast<double>(len) : 0.0);
                o += num;
            }
            o.push_back('\n');
        });
        written = order.size();
    }
    if (args.output) {
        write_whole_file(*args.output, out);
    } else {
        std::fwrite(out.data(), 1, out.size(), stdout);
        std::fflush(stdout);
    }
    if (args.bedgraph) write_whole_file(*args.bedgraph, bedgraph);
    if (verbose) std::fprintf(stderr, "[INFO] Wrote %zu feature coverage rows.\n", written);
    timer.lap("Merging groups and writing rows");
    g_run_stats.write("coverage", timer.total());
}

}  // namespace gffx::commands::coverage
