// source_stream.hpp -- the streaming pipeline of the source readers (bgzf.hip: BAM, sam.hip: SAM, bed.hip: BED), once: what a handle owns
// and does whatever the format of its bytes.
//
// Fed bytes go to the device in sub-batches.  Staging is double-buffered: while the kernels work on one sub-batch, the host
// copies the next one into pinned memory (stage[k]) and its host -> device transfer runs on a second stream; the kernels of
// that sub-batch wait for copied[k].  The order for every sub-batch is: stage, upload (stage_upload), drain the sub-batch in
// flight, enqueue this one.  The format supplies the last two: its enqueue puts its kernels on `stream` between ev[0..3] and
// reads its result struct back into the pinned `res_host`; its drain is drain_front (the sync, a member that failed to
// inflate), its own check of the result, and drain_back (the stage times, the kept rows back to the host at 12 B each, the
// unfinished record or line at D's end moved in front of the next sub-batch: the carry).  The device idles between the
// two.  A failure is kept (sticky): every later call on the handle returns it again with its first message.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "bgzf_device.hpp"

namespace gffx {

struct SourceStream {
    int device = 0;
    const char *who = "";        // the feed entry point's name (the prefix of the out-of-memory messages)
    uint64_t skip = 0;           // header bytes still to skip in the decompressed stream
    uint64_t chunk_bytes = 0;    // fed bytes per sub-batch (BGZF: compressed, at most)
    uint64_t out_cap = 0;        // decompressed bytes per sub-batch (without the carry)
    uint64_t file_off = 0;       // bytes fed so far
    hipStream_t stream = nullptr;       // the kernels, in order
    hipStream_t copy_stream = nullptr;  // host -> device copies of the next sub-batch, beside the kernels of this one
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};  // in[k] / dir[k] have arrived
    uint8_t *stage[2] = {nullptr, nullptr};     // pinned fed bytes, double-buffered
    uint64_t stage_cap[2] = {0, 0};
    int cur_stage = 0;
    BgzfDir *stage_dir[2] = {nullptr, nullptr};
    void *res_host = nullptr;  // pinned: the format's result struct of the sub-batch in flight (result<R>())
    DevArr<uint8_t> in[2], D[2];
    DevArr<BgzfDir> dir[2];  // dst relative to the end of the carry
    DevArr<int32_t> status;
    DevArr<uint32_t> rows;
    // the sub-batch in flight (enqueued, not drained)
    bool in_flight = false;
    int cur = 0;           // D[cur] holds its decompressed stream
    uint64_t carry = 0;    // bytes of the unfinished record / line at D[cur]'s start (before the in-flight batch: after drain)
    uint64_t n_D = 0;      // its D length
    std::vector<BgzfDir> fl_dir;  // its members (file offsets for messages)
    uint64_t fl_file_off = 0;
    // results
    std::vector<uint32_t> out_rows;
    uint64_t unmapped = 0, no_seq = 0, kept = 0;  // (unmapped: the format's first skip tally; BED: the skipped lines)
    double ms[3] = {0, 0, 0};  // ev[0] .. ev[1] (inflate), ev[1] .. ev[2], ev[2] .. ev[3]
    int error = GFFX_OK;
    std::string error_msg;

    SourceStream() = default;
    SourceStream(const SourceStream &) = delete;
    SourceStream &operator=(const SourceStream &) = delete;
    ~SourceStream() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        for (int k = 0; k < 2; ++k) {
            if (copied[k]) (void)hipEventDestroy(copied[k]);
            if (stage[k]) (void)hipHostFree(stage[k]);
            if (stage_dir[k]) (void)hipHostFree(stage_dir[k]);
        }
        if (res_host) (void)hipHostFree(res_host);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }

    // the streams, the events and res_bytes of pinned result (the device is current)
    int init(int device_, const char *feed_name, size_t res_bytes) {
        device = device_;
        who = feed_name;
        GFFX_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        GFFX_HIP_TRY(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        for (hipEvent_t &e : ev) GFFX_HIP_TRY(hipEventCreate(&e));
        for (hipEvent_t &e : copied) GFFX_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        GFFX_HIP_TRY(hipHostMalloc(&res_host, res_bytes));
        return GFFX_OK;
    }
    template <class R>
    R *result() const {
        return static_cast<R *>(res_host);
    }
    // decompressed bytes per sub-batch of BGZF members of at most `chunk` compressed bytes
    static uint64_t bgzf_out_cap(uint64_t chunk) { return std::min<uint64_t>(std::max<uint64_t>(4 * chunk, 1ull << 20), 1ull << 30); }

    int sticky(int rc) {
        if (rc != GFFX_OK && error == GFFX_OK) {
            error = rc;
            error_msg = g_last_error;
        }
        return rc;
    }

    // the next staging buffer, at least n bytes
    int next_stage(uint64_t n, int *k_out) {
        const int k = cur_stage;
        cur_stage ^= 1;
        if (n > stage_cap[k]) {
            if (stage[k]) (void)hipHostFree(stage[k]);
            stage[k] = nullptr;
            stage_cap[k] = 0;
            if (hipHostMalloc((void **)&stage[k], n) != hipSuccess)
                return fail(GFFX_E_OOM, "%s: pinned staging of %llu bytes", who, (unsigned long long)n);
            stage_cap[k] = n;
        }
        *k_out = k;
        return GFFX_OK;
    }

    // starts the copies of stage[k] (n_src bytes, nb members) to in[k] / dir[k] on the copy stream.  Their previous contents
    // belonged to the sub-batch before last, which has been drained.
    int stage_upload(int k, uint32_t nb, uint64_t n_src) {
        GFFX_HIP_TRY(in[k].ensure(std::max<uint64_t>(n_src, 1)));
        GFFX_HIP_TRY(hipMemcpyAsync(in[k].p, stage[k], n_src, hipMemcpyHostToDevice, copy_stream));
        if (nb) {
            GFFX_HIP_TRY(dir[k].ensure(nb));
            GFFX_HIP_TRY(hipMemcpyAsync(dir[k].p, stage_dir[k], nb * sizeof(BgzfDir), hipMemcpyHostToDevice, copy_stream));
        }
        GFFX_HIP_TRY(hipEventRecord(copied[k], copy_stream));
        return GFFX_OK;
    }

    // The whole BGZF members of bgzf[0, n) in sub-batches of at most chunk_bytes compressed, out_cap decompressed and
    // kMaxBlocksPerBatch members (at least one member).  Each is staged and on its way to in[k] / dir[k] while the previous
    // sub-batch still runs; then run(k, nb, T, file_off) -- nb members, T decompressed bytes, the first member's file
    // offset -- drains that one and enqueues this.
    template <class Run>
    int feed_members(const uint8_t *bgzf, uint64_t n, Run &&run) {
        std::vector<BgzfDir> all;
        if (int rc = walk_members(bgzf, n, file_off, &all)) return rc;
        size_t i = 0;
        while (i < all.size()) {
            size_t j = i;
            uint64_t src = 0, dst = 0;
            while (j < all.size() &&
                   (j == i || (src + all[j].len <= chunk_bytes && dst + all[j].isize <= out_cap && j - i < kMaxBlocksPerBatch))) {
                src += all[j].len;
                dst += all[j].isize;
                ++j;
            }
            int k = 0;
            if (int rc = next_stage(src, &k)) return rc;
            if (!stage_dir[k] && hipHostMalloc((void **)&stage_dir[k], kMaxBlocksPerBatch * sizeof(BgzfDir)) != hipSuccess)
                return fail(GFFX_E_OOM, "%s: pinned directory", who);
            std::memcpy(stage[k], bgzf + all[i].src, src);
            for (size_t x = i; x < j; ++x) {
                BgzfDir d = all[x];
                d.src -= all[i].src;
                d.dst -= all[i].dst;
                stage_dir[k][x - i] = d;
            }
            if (int rc = stage_upload(k, (uint32_t)(j - i), src)) return rc;
            if (int rc = run(k, (uint32_t)(j - i), dst, file_off + all[i].src)) return rc;
            i = j;
        }
        return GFFX_OK;
    }

    // the end of a format's enqueue: N bytes in D[cur] are in flight, inflated from members stage_dir[k][0, nb) (nb 0: none)
    void set_in_flight(uint64_t N, int k, uint32_t nb, uint64_t batch_file_off) {
        in_flight = true;
        n_D = N;
        if (nb) fl_dir.assign(stage_dir[k], stage_dir[k] + nb);
        else fl_dir.clear();
        fl_file_off = batch_file_off;
    }

    // The front of a drain (in_flight holds): waits for the sub-batch, whose result is in res_host from here on; fails on
    // the member that did not inflate.  bad_block: the field of the pinned result.
    int drain_front(const uint32_t *bad_block) {
        in_flight = false;
        GFFX_HIP_TRY(hipStreamSynchronize(stream));
        if (*bad_block != 0xFFFFFFFFu) {
            int32_t st = 0;
            GFFX_HIP_TRY(hipMemcpy(&st, status.p + *bad_block, sizeof st, hipMemcpyDeviceToHost));
            return fail(GFFX_E_INVALID, "BGZF block at file offset %llu: %s", (unsigned long long)(fl_file_off + fl_dir[*bad_block].src),
                        bgzf::status_name(st));
        }
        return GFFX_OK;
    }

    // The back of a drain, the sub-batch being sound: the stage times, its tallies, its n_kept rows, and D[tail, n_D) -- the
    // unfinished record or line -- to the start of the other D buffer, which becomes the current one.
    int drain_back(uint64_t tail, uint64_t n_kept, uint64_t n_unmapped, uint64_t n_no_seq) {
        float t = 0;
        for (int k = 0; k < 3; ++k)
            if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess) ms[k] += t;
        unmapped += n_unmapped;
        no_seq += n_no_seq;
        kept += n_kept;
        if (n_kept) {
            const size_t at = out_rows.size();
            out_rows.resize(at + 3 * n_kept);
            GFFX_HIP_TRY(hipMemcpy(out_rows.data() + at, rows.p, n_kept * 12, hipMemcpyDeviceToHost));
        }
        const uint64_t c = n_D - tail;
        const int nxt = 1 - cur;
        GFFX_HIP_TRY(D[nxt].ensure(c + out_cap));
        if (c) GFFX_HIP_TRY(hipMemcpyAsync(D[nxt].p, D[cur].p + tail, c, hipMemcpyDeviceToDevice, stream));
        cur = nxt;
        carry = c;
        return GFFX_OK;
    }

    uint64_t n_rows() const { return out_rows.size() / 3; }
    void copy_rows(uint32_t *out) const {
        if (!out_rows.empty()) std::memcpy(out, out_rows.data(), out_rows.size() * sizeof(uint32_t));
    }
    void stage_ms(double *a, double *b, double *c) const {
        if (a) *a = ms[0];
        if (b) *b = ms[1];
        if (c) *c = ms[2];
    }
};

}  // namespace gffx
