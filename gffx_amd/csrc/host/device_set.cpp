// device_set.cpp -- see device_set.hpp
#include "device_set.hpp"

#include <algorithm>
#include <cstdio>
#include <string>

#include "text.hpp"

namespace gffx {

void hip_fail(const char *what) { throw Error(std::string(what) + ": " + gffx_hip_last_error()); }

DeviceSet DeviceSet::resolve(int device, int gpus) {
    const int visible = gffx_hip_device_count();
    if (visible <= 0) throw Error(std::string("no HIP device visible (the engine has no CPU fallback)"));
    if (device < 0 || device >= visible)
        throw Error("device " + std::to_string(device) + " out of range (" + std::to_string(visible) + " visible)");
    DeviceSet s;
    const size_t D = static_cast<size_t>(std::max(1, gpus));
    s.dev_.resize(D);
    for (size_t d = 0; d < D; ++d) s.dev_[d] = (device + static_cast<int>(d)) % visible;
    for (size_t d = 1; d < D; ++d)
        for (size_t e = 0; e < d; ++e) s.distinct_ &= s.dev_[d] != s.dev_[e];
    if (D > 1 && !s.distinct_)
        std::fprintf(stderr, "[WARN] --gpus %zu with %d visible device(s): logical devices share GPUs (no RCCL exchange)\n", D, visible);
    s.clones_.resize(D);
    return s;
}

gffx_hip_index *DeviceSet::index_on(size_t d, gffx_hip_index *first) {
    if (dev_[d] == dev_[0]) return first;
    if (gffx_hip_index_clone(first, dev_[d], OutPtr(clones_[d])) != GFFX_OK) hip_fail("gffx_hip_index_clone");
    return clones_[d].get();
}

bool DeviceSet::exchange_counts(std::vector<uint64_t> &counts, const char *what_a, const char *what_b, bool verbose, bool adopt_gathered) const {
    const size_t D = dev_.size();
    std::vector<uint64_t> gathered(2 * D * D, 0);
    bool exchanged = false;
    if (distinct_) {
        if (gffx_hip_allgather_counts(static_cast<int>(D), dev_.data(), counts.data(), gathered.data()) != GFFX_OK) {
            std::fprintf(stderr, "[WARN] hit-count all-gather over RCCL failed: %s\n", gffx_hip_last_error());
        } else {
            exchanged = true;
            if (adopt_gathered) {
                for (size_t d = 0; d < D; ++d)
                    if (gathered[2 * d] != counts[2 * d]) throw Error("the RCCL all-gather returned different region counts");
                counts.assign(gathered.begin(), gathered.begin() + 2 * D);
            }
        }
    }
    if (verbose)
        for (size_t d = 0; d < D; ++d)
            std::fprintf(stderr, "[INFO] device %d: %llu %s, %llu %s%s\n", dev_[d], (unsigned long long)counts[2 * d], what_a,
                         (unsigned long long)counts[2 * d + 1], what_b, exchanged ? " (all-gathered over RCCL)" : "");
    return exchanged;
}

}  // namespace gffx
