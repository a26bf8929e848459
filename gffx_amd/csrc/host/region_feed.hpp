// region_feed.hpp -- the regions of `gffx closest`, `gffx annotate` and `gffx enrich` on their way through a device region
// store: one region (-r), the device reader's rows of a BED file in slices (bgzipped, or GFFX_BED_DEVICE=1: bed::route), or
// the rows of a plain BED file parsed chunk of text by chunk of text (GFFX_CHUNK_BYTES / GFFX_CHUNK_MB).  The rows go through
// the store's two pinned staging buffers by turns; the caller's serve(store, k, stage_rows, n) takes the n rows that sit in
// staging buffer k to the store, through the device and to its output before the next chunk is parsed, so memory is bounded
// by a chunk.  depth::run_row_batches (gffx.hpp) serves the batch commands the same way.
#pragma once
#include <cstring>

#include "intersect_internal.hpp"

namespace gffx::commands {

class RegionFeed {
  public:
    // Step one, before the device is touched: the region parsed, or the BED file routed and mapped (a malformed -r or a
    // missing file ends the run here).
    RegionFeed(const std::optional<std::string> &region, const std::optional<std::string> &bed, const TreeIndexData &index, const CommonArgs &common)
        : bed_(bed), index_(index) {
        if (region) {
            const auto [chr, s, e] = intersect::parse_region(*region, index.seqid_to_num, common);
            all_rows_ = {chr, s, e};
        } else {
            device_rows_ = bed::route(*bed) == bed::Route::Device;
            bed_file_.emplace(*bed);
        }
    }

    // Step two, once the device is up: the device reader's rows (a lap of their own) and the rows per chunk.
    void open(int device, bool verbose, StageTimer &timer) {
        if (bed_ && device_rows_) {
            all_rows_ = bed::read_rows(*bed_, index_.seqid_to_num, bed::kIntersect, device, verbose);
            timer.lap("BED rows read on the device");
        }
        if (bed_)
            chunk_rows_ = (device_rows_ ? std::min(chunk_bytes_ / intersect::kMinBedRowBytes, std::max<size_t>(all_rows_.size() / 3, 1))
                                        : std::min(chunk_bytes_, std::max<size_t>(bed_file_->size(), 1)) / intersect::kMinBedRowBytes) + 16;
    }

    // Step three, after the caller's own device object (which may be sized by chunk_rows(), and whose build goes on behind the
    // call while the staging buffers are pinned here): the store.
    void create_store(int device) {
        if (gffx_hip_regions_create(device, 0, chunk_rows_, 0, OutPtr(store_)) != GFFX_OK) hip_fail("gffx_hip_regions_create");
    }

    size_t chunk_rows() const { return chunk_rows_; }  // the most rows of a chunk (+ 16): 1 for -r
    size_t chunks() const { return chunk_; }           // chunks served so far

    // Every chunk with at least one kept row, in input order: chunk i through staging buffer / slot k = i & 1.
    template <class Serve>
    void run(size_t threads, Serve &&serve) {
        // the n rows now in staging buffer k (it still holds them afterwards: it is refilled two chunks on)
        auto serve_slot = [&](int k, uint64_t n) {
            serve(store_.get(), k, static_cast<const uint32_t *>(gffx_hip_regions_staging(store_.get(), k)), n);
            ++chunk_;
        };
        auto staging = [&](int k) {
            if (gffx_hip_regions_wait_staging(store_.get(), k) != GFFX_OK) hip_fail("gffx_hip_regions_wait_staging");
            return gffx_hip_regions_staging(store_.get(), k);
        };
        if (!bed_ || device_rows_) {
            const size_t n_all = all_rows_.size() / 3, step = chunk_rows_ > 16 ? chunk_rows_ - 16 : 1;
            for (size_t at = 0; at < n_all; at += step) {
                const size_t n = std::min(step, n_all - at);
                const int k = static_cast<int>(chunk_ & 1);
                std::memcpy(staging(k), all_rows_.data() + 3 * at, n * 12);
                serve_slot(k, n);
            }
            return;
        }
        const std::string_view text = bed_file_->view();
        const intersect::SeqidTable seqids(index_.seqid_to_num);
        std::vector<std::vector<uint32_t>> piece;
        intersect::for_each_line_chunk(text, chunk_bytes_, [&](size_t pos, size_t z, bool last) {
            intersect::parse_bed_pieces(text, pos, z, last, seqids, threads, piece);
            const int k = static_cast<int>(chunk_ & 1);
            uint32_t *dst = staging(k);
            uint64_t n = 0;
            for (const auto &p : piece) {
                std::memcpy(dst + 3 * n, p.data(), p.size() * 4);
                n += p.size() / 3;
            }
            if (n) serve_slot(k, n);
            return true;
        });
    }

  private:
    const std::optional<std::string> bed_;
    const TreeIndexData &index_;
    std::vector<uint32_t> all_rows_;  // -r: the one region; the device reader: every row
    std::optional<MappedFile> bed_file_;
    bool device_rows_ = false;
    const size_t chunk_bytes_ = intersect::stream_chunk_bytes();
    size_t chunk_rows_ = 1, chunk_ = 0;
    RegionsHandle store_;
};

}  // namespace gffx::commands
