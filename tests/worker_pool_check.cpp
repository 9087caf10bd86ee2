// Driver of tests/test_worker_pool.py: the worker pool of the lock-step LexLSI driver (lexls_amd/csrc/lsi_worker_pool.h), alone, on
// the host.  Built with -fsanitize=thread; exit status 0 = every check held.
#include "lsi_worker_pool.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

namespace
{
    int failures = 0;
    void check(bool ok, const char *what, uint32_t workers, uint32_t count)
    {
        if (ok) return;
        failures++;
        std::fprintf(stderr, "FAILED: %s (workers %u, count %u)\n", what, workers, count);
    }
    void nap() { std::this_thread::sleep_for(std::chrono::milliseconds(30)); }

    /// one run(): every index of [0, count) exactly once (hits: plain bytes, each written by the one thread that got the index)
    bool visits_once(WorkerPool &pool, uint32_t count, bool light = false, bool *inline_only = nullptr)
    {
        std::vector<uint8_t> hits(count, 0);
        std::atomic<uint32_t> elsewhere{0};
        const std::thread::id me = std::this_thread::get_id();
        pool.run(count, [&](uint32_t b) {
            hits[b]++;
            if (std::this_thread::get_id() != me) elsewhere.fetch_add(1, std::memory_order_relaxed);
        }, light);
        if (inline_only) *inline_only = elsewhere.load() == 0;
        for (uint32_t b = 0; b < count; b++)
            if (hits[b] != 1) return false;
        return true;
    }

    void exercise(uint32_t workers, uint32_t count)
    {
        {
            WorkerPool pool(workers); // default spin: the stages below follow each other faster than the workers fall asleep
            check(visits_once(pool, count), "every index once", workers, count);
            bool ok = true;
            std::atomic<uint64_t> sum{0};
            for (int r = 0; r < 3000; r++)
            {
                pool.run(count, [&](uint32_t b) { sum.fetch_add(b + 1, std::memory_order_relaxed); });
                ok = ok && sum.load() == (uint64_t)(r + 1) * count * (count + 1) / 2;
            }
            check(ok, "back-to-back runs (spin path)", workers, count);
            // some indices throw: rethrown once, every chunk without a throwing index still ran, and the pool works afterwards
            int caught = 0;
            try
            {
                pool.run(count, [&](uint32_t b) {
                    if (b % 50 == 7) throw std::runtime_error("index refuses");
                });
            }
            catch (const std::runtime_error &)
            {
                caught++;
            }
            check(caught == 1, "exception rethrown once", workers, count);
            check(visits_once(pool, count), "every index once after an exception", workers, count);
        } // destroyed while its workers spin
        {
            WorkerPool pool(workers, 0.0); // workers sleep at once
            nap();
            check(visits_once(pool, count), "run after the workers went to sleep", workers, count);
            nap();
            pool.prewake();
            check(visits_once(pool, count), "run after prewake", workers, count);
            pool.prewake();
            pool.prewake();
            check(visits_once(pool, count), "run after two prewakes", workers, count);
            nap();
            bool inline_only = false;
            check(visits_once(pool, count, true, &inline_only), "light run with sleeping workers", workers, count);
            check(inline_only, "light run with sleeping workers stays on the caller's thread", workers, count);
            nap();
        } // destroyed while its workers sleep
        {
            WorkerPool pool(workers, 0.0);
        } // destroyed at once: workers may not have started yet
    }
} // namespace

int main()
{
    const uint32_t workers[] = {0, 1, 5}, counts[] = {100, 1000}; // below and above the 128-element inline threshold
    for (uint32_t w : workers)
        for (uint32_t c : counts) exercise(w, c);
    check(WorkerPool::default_workers(32) == 0 && WorkerPool::default_workers(1 << 20) <= 15, "default_workers", 0, 0);
    if (failures) return 1;
    std::puts("worker pool ok");
    return 0;
}
