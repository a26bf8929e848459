// device_set.hpp -- shared on the way to the C-ABI: owning handles, `--device` / `--gpus N` -> devices, their indexes, the exchange
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "../../../include/gffx_hip.h"

namespace gffx {

[[noreturn]] void hip_fail(const char *what);  // throws Error("<what>: <gffx_hip_last_error()>")

template <auto Destroy>
struct HandleDeleter {
    template <typename T> void operator()(T *p) const { Destroy(p); }
};
template <typename T, auto Destroy>
using Handle = std::unique_ptr<T, HandleDeleter<Destroy>>;
using BatchHandle = Handle<gffx_hip_batch, gffx_hip_batch_destroy>;
using RegionsHandle = Handle<gffx_hip_regions, gffx_hip_regions_destroy>;
using IndexHandle = Handle<gffx_hip_index, gffx_hip_index_destroy>;
using DepthHandle = Handle<gffx_hip_depth, gffx_hip_depth_destroy>;
using LinesHandle = Handle<gffx_hip_lines, gffx_hip_lines_destroy>;
using UnionHandle = Handle<gffx_hip_union, gffx_hip_union_destroy>;
using PileupHandle = Handle<gffx_hip_pileup, gffx_hip_pileup_destroy>;
using ProfileHandle = Handle<gffx_hip_profile, gffx_hip_profile_destroy>;
using ClassMapHandle = Handle<gffx_hip_classmap, gffx_hip_classmap_destroy>;
using IdsHandle = Handle<gffx_hip_ids, gffx_hip_ids_destroy>;
using AttrsHandle = Handle<gffx_hip_attrs, gffx_hip_attrs_destroy>;

// gffx_hip_x_create(..., OutPtr(h)): the `T **out` argument of a C-ABI constructor; h owns what the call stored.  Only as a
// temporary inside the call's full expression (a hand-made std::out_ptr): h is set when the temporary dies.
template <typename H>
class OutPtr {
  public:
    explicit OutPtr(H &h) : h_(h) {}
    ~OutPtr() {
        if (p_) h_.reset(p_);
    }
    operator typename H::pointer *() { return &p_; }

  private:
    H &h_;
    typename H::pointer p_ = nullptr;
};

// The devices of a run: --device names a real device (out of range is an error, as in the engine); only the ADDITIONAL
// logical devices of --gpus N wrap around the visible ones.
class DeviceSet {
  public:
    // throws Error without a visible device or with --device out of range; warns when logical devices share GPUs
    static DeviceSet resolve(int device, int gpus);
    size_t size() const { return dev_.size(); }
    int operator[](size_t d) const { return dev_[d]; }
    // the index for logical device d: `first` (the first device's) where d shares its GPU, otherwise a clone owned by the set
    // (one caller per d at a time)
    gffx_hip_index *index_on(size_t d, gffx_hip_index *first);
    // The exchange step of a run on more than one device: counts = {a, b} per logical device, all-gathered over RCCL
    // (16 bytes per device) when the devices are distinct.  Every result already sits on the host, and a node without a usable
    // librccl must not lose a finished run to it: a failure is a warning.  adopt_gathered: counts become what device 0 received (an
    // Error if its `a`s differ from the host's).  Under `verbose` one "[INFO] device D: <a> what_a, <b> what_b" line per device.
    bool exchange_counts(std::vector<uint64_t> &counts, const char *what_a, const char *what_b, bool verbose, bool adopt_gathered) const;

  private:
    std::vector<int> dev_;
    bool distinct_ = true;
    std::vector<IndexHandle> clones_;
};

}  // namespace gffx
