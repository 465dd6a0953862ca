// rg_copy_pool.cpp — the copy pool of rg_copy_pool.h: spin / condvar fork-join
// over atomics.  The calling thread publishes a copy by bumping `gen`; every
// helper copies its piece and counts `remaining` down; the caller copies piece
// 0 and spins until the count is zero.
#include "rg_copy_pool.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

struct rg_copy_pool::Impl {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<bool> stop{false}, active{false};
    std::atomic<uint64_t> gen{0};
    std::atomic<int> remaining{0};
    unsigned char *dst = nullptr;
    const unsigned char *src = nullptr;
    size_t bytes = 0;
    int parts = 1;
};

rg_copy_pool::rg_copy_pool(int helpers) : p_(new Impl) {
    p_->parts = helpers + 1;
    for (int i = 0; i < helpers; ++i) p_->th.emplace_back([this, i] { run(i + 1); });
}

rg_copy_pool::~rg_copy_pool() {
    {
        std::lock_guard<std::mutex> g(p_->m);
        p_->stop.store(true);
    }
    p_->cv.notify_all();
    for (std::thread &t : p_->th) t.join();
    delete p_;
}

void rg_copy_pool::begin() {
    {
        std::lock_guard<std::mutex> g(p_->m);
        p_->active.store(true);
    }
    p_->cv.notify_all();
}

void rg_copy_pool::end() { p_->active.store(false); }

namespace {
// Piece i of n of [0, bytes), 4 KiB aligned (the last piece takes the rest).
inline void piece(size_t bytes, int i, int n, size_t &off, size_t &len) {
    const size_t per = (bytes / (size_t)n + 4095) & ~(size_t)4095;
    off = std::min(bytes, per * (size_t)i);
    len = i == n - 1 ? bytes - off : std::min(bytes - off, per);
}

// A band's copy out of pinned staging into the caller's pageable frame (non-temporal AVX2 stores
// measured no consistent change: DESIGN.md 5)
void copy_band(unsigned char *dst, const unsigned char *src, size_t n) { std::memcpy(dst, src, n); }
}  // namespace

void rg_copy_pool::run(int id) {
    uint64_t seen = 0;
    for (;;) {
        uint64_t g = p_->gen.load(std::memory_order_acquire);
        if (g == seen) {
            if (p_->stop.load()) return;
            if (p_->active.load(std::memory_order_relaxed)) {
                __builtin_ia32_pause();
                continue;
            }
            std::unique_lock<std::mutex> lk(p_->m);
            p_->cv.wait(lk, [&] {
                return p_->stop.load() || p_->active.load() || p_->gen.load(std::memory_order_acquire) != seen;
            });
            continue;
        }
        seen = g;
        size_t off, len;
        piece(p_->bytes, id, p_->parts, off, len);
        if (len) copy_band(p_->dst + off, p_->src + off, len);
        p_->remaining.fetch_sub(1, std::memory_order_acq_rel);
    }
}

void rg_copy_pool::copy(void *dst, const void *src, size_t bytes) {
    if (p_->parts == 1 || bytes < (256u << 10)) {
        std::memcpy(dst, src, bytes);
        return;
    }
    p_->dst = static_cast<unsigned char *>(dst);
    p_->src = static_cast<const unsigned char *>(src);
    p_->bytes = bytes;
    p_->remaining.store(p_->parts - 1, std::memory_order_relaxed);
    {
        std::lock_guard<std::mutex> g(p_->m);  // a sleeping helper sees the new generation
        p_->gen.fetch_add(1, std::memory_order_release);
    }
    p_->cv.notify_all();
    size_t off, len;
    piece(bytes, 0, p_->parts, off, len);
    if (len) copy_band(p_->dst + off, p_->src + off, len);
    while (p_->remaining.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
}
