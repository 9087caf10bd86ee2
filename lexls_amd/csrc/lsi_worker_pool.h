// Host worker pool of the lock-step LexLSI driver.  Plain C++ (no HIP): tests/worker_pool_check.cpp builds it alone under ThreadSanitizer.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace // (internal linkage, as every helper of the driver: nothing of it is exported from the library)
{
/// Persistent host worker pool for the per-instance work of a lock-step batch (the instances are independent; each touches only
/// its own LexLSI object and its own slot of the staging arrays).  Created once per lexls_lsi_batch_solve call: the active-set
/// rounds are short (~1 ms of host work for 1024 instances), so threads must not be spawned per round.
class WorkerPool
{
public:
    /// spin_seconds_: how long an idle worker spins before it sleeps (0 = sleep at once)
    explicit WorkerPool(uint32_t workers, double spin_seconds_ = 300e-6) : spin_seconds(spin_seconds_)
    {
        for (uint32_t i = 0; i < workers; i++) th.emplace_back([this]() { loop(); });
    }
    ~WorkerPool()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop.store(true);
        }
        cv_start.notify_all();
        for (auto &t : th) t.join();
    }
    static uint32_t default_workers(uint32_t batch)
    {
        const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
        const uint32_t nt = std::min<uint32_t>(std::min<uint32_t>(hw, 16u), batch / 64);
        return nt > 1 ? nt - 1 : 0; // the calling thread works too
    }
    /// f(b) for b in [0, count); returns when all are done; rethrows the first exception.
    /// The stages of a batch solve follow each other every ~50 us: a condition-variable wake-up per stage would cost more than
    /// the stage's host work, so idle workers spin on the generation counter for a while (spin_seconds) before they go to sleep.
    /// light: a job of a few microseconds per element (copies, releases): when the workers have gone to sleep (the GPU ran for
    /// milliseconds meanwhile) waking sixteen threads through the condition variable costs more than running it here
    void run(uint32_t count_, const std::function<void(uint32_t)> &f, bool light = false)
    {
        while (pending.load(std::memory_order_acquire) != 0) relax(); // (a prewake() still being acknowledged)
        if (th.empty() || count_ < 128 || (light && sleepers.load() != 0))
        {
            for (uint32_t b = 0; b < count_; b++) f(b);
            return;
        }
        job   = &f;
        count = count_;
        next.store(0);
        err = nullptr;
        pending.store(static_cast<uint32_t>(th.size()), std::memory_order_relaxed);
        gen.fetch_add(1); // seq_cst with the sleepers' increment / generation check below: one side always sees the other
        if (sleepers.load() != 0)
        {
            std::lock_guard<std::mutex> lk(m); // a worker between its last check and its wait holds m: it sees the new generation
            cv_start.notify_all();
        }
        work();
        while (pending.load(std::memory_order_acquire) != 0) relax(); // every worker acknowledges every generation
        job = nullptr;
        if (err) std::rethrow_exception(err);
    }

    /// wakes sleeping workers ahead of a run() that is about to come (they spin again for spin_seconds): the wake-up latency of the
    /// condition variable (~0.1-0.3 ms for the last of sixteen threads) then overlaps what the caller does in between
    void prewake()
    {
        if (th.empty() || sleepers.load() == 0) return;
        while (pending.load(std::memory_order_acquire) != 0) relax();
        static const std::function<void(uint32_t)> nothing = [](uint32_t) {};
        job   = &nothing;
        count = 0;
        next.store(0);
        pending.store(static_cast<uint32_t>(th.size()), std::memory_order_relaxed);
        gen.fetch_add(1);
        {
            std::lock_guard<std::mutex> lk(m);
            cv_start.notify_all();
        }
    }

private:
    const double spin_seconds;
    static void relax()
    {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
    }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void work()
    {
        const uint32_t chunk = 16;
        for (;;)
        {
            const uint32_t b0 = next.fetch_add(chunk);
            if (b0 >= count) break;
            const uint32_t b1 = std::min(count, b0 + chunk);
            try
            {
                for (uint32_t b = b0; b < b1; b++) (*job)(b);
            }
            catch (...)
            {
                std::lock_guard<std::mutex> lk(m);
                if (!err) err = std::current_exception();
            }
        }
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;)
        {
            uint32_t spins = 0;
            double t_idle  = 0.0;
            while (gen.load(std::memory_order_acquire) == seen && !stop.load(std::memory_order_relaxed))
            {
                relax();
                if ((++spins & 255u) != 0) continue;
                const double t = now();
                if (t_idle == 0.0) t_idle = t;
                if (t - t_idle < spin_seconds) continue;
                std::unique_lock<std::mutex> lk(m);
                sleepers.fetch_add(1);
                cv_start.wait(lk, [&]() { return stop.load() || gen.load() != seen; });
                sleepers.fetch_sub(1);
            }
            if (stop.load()) return;
            seen = gen.load(std::memory_order_acquire);
            work();
            pending.fetch_sub(1, std::memory_order_release);
        }
    }
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv_start;
    const std::function<void(uint32_t)> *job = nullptr;
    uint32_t count                           = 0;
    std::atomic<uint32_t> next{0}, pending{0}, sleepers{0};
    std::atomic<uint64_t> gen{0};
    std::atomic<bool> stop{false};
    std::exception_ptr err;
};
} // namespace
