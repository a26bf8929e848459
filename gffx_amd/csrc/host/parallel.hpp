// parallel.hpp -- the host side's two fan-outs: parallel_for (threads spawned per call) and WorkerPool (threads that stay)
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace gffx {

// fn(i) for i in [0, n_items): the items are claimed from one counter by min(n_threads, n_items) - 1 fresh threads and the
// caller; returns when all are joined.  An exception from fn is kept, the other items still run, and the one of the LOWEST i
// is rethrown here (for items in file order: the first error of the file, as a serial loop reports it).  A site whose
// workers take contiguous shares calls parallel_for(W, W, share).
template <typename F>
void parallel_for(size_t n_items, size_t n_threads, F &&fn) {
    std::atomic<size_t> next{0};
    std::mutex mu;
    std::exception_ptr err;
    size_t err_item = 0;
    auto work = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n_items) return;
            try {
                fn(i);
            } catch (...) {
                std::lock_guard<std::mutex> lk(mu);
                if (!err || i < err_item) err = std::current_exception(), err_item = i;
            }
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < std::min(n_threads, n_items); ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (err) std::rethrow_exception(err);
}

// Host threads that stay alive across the chunks of a streamed file (spawning `threads` std::threads per 64 MB chunk cost more
// than parsing the chunk's 1 MB pieces).  run(n, fn): fn(0) .. fn(n-1) on the workers and the caller; returns when all are done.
class WorkerPool {
  public:
    explicit WorkerPool(size_t workers) {
        for (size_t i = 0; i < workers; ++i) threads_.emplace_back([this] { loop(); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : threads_) t.join();
    }
    void run(size_t n, const std::function<void(size_t)> &fn) {
        auto job = std::make_shared<Job>();
        job->fn = &fn;
        job->total = n;
        job->pending.store(n);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = job;
            ++generation_;
        }
        cv_.notify_all();
        help(*job);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return job->pending.load() == 0; });
        job_.reset();
    }

  private:
    struct Job {  // (one object per run(): a worker that wakes late holds the finished job, whose indices are used up)
        const std::function<void(size_t)> *fn = nullptr;
        size_t total = 0;
        std::atomic<size_t> next{0}, pending{0};
    };
    void help(Job &j) {
        for (;;) {
            const size_t i = j.next.fetch_add(1);
            if (i >= j.total) return;
            (*j.fn)(i);
            if (j.pending.fetch_sub(1) == 1) {
                std::lock_guard<std::mutex> lk(mu_);
                done_.notify_all();
            }
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                j = job_;
            }
            if (j) help(*j);
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::shared_ptr<Job> job_;
    uint64_t generation_ = 0;
    bool stop_ = false;
    std::vector<std::thread> threads_;
};

}  // namespace gffx
