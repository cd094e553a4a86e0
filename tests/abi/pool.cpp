// The mapper's pool of threads (rawalign_amd/csrc/rawdtw_pool.h) as a plain C++ program: the header needs nothing but the standard
// library.  Built plain, under ThreadSanitizer and under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_pool_cpu.py).
// With 1 (no worker), 2, 4 and 8 threads:
//   shapes       n == 0, n <= grain (the inline path), n no multiple of grain, grain 1
//   spinning     a few thousand loops back to back: the workers are still looking for the next loop
//   asleep       loops 5 ms apart: the workers sleep and are woken through the condition variable
//   slow worker  a loop in which a worker's index sleeps 5 ms: the caller passes its 2 ms of spinning and waits to be notified
//   destruction  right after a loop (workers spinning), and after a pause (workers asleep)
// In every loop each index adds one to its own plain element of an array, and the caller checks after run() that every element is 1: a
// missing happens-before edge between the workers' writes and the caller's reads is a data race ThreadSanitizer reports, an index dealt
// twice or not at all fails the check.  Prints "ok <loops>"; the first failure otherwise.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>
#include <vector>

#include "rawdtw_pool.h"

using rawdtw_map::Pool;

static long loops = 0;

static bool loop(Pool &pool, size_t n, size_t grain, const char *what, bool slow_worker = false)
{
    std::vector<int> hit(n + 1, 0); // (plain memory: the pool's own synchronisation is all that orders these writes and reads)
    const std::thread::id caller = std::this_thread::get_id();
    std::atomic<bool> slept{false};
    pool.run(n, grain, [&](size_t i) {
        hit[i] += 1;
        if (slow_worker && std::this_thread::get_id() != caller && !slept.exchange(true)) std::this_thread::sleep_for(std::chrono::milliseconds(5));
    });
    loops++;
    for (size_t i = 0; i < n; i++)
        if (hit[i] != 1) { printf("FAIL %s: threads %d, n %zu, grain %zu: index %zu ran %d times\n", what, pool.threads(), n, grain, i, hit[i]); return false; }
    if (hit[n] != 0) { printf("FAIL %s: threads %d, n %zu, grain %zu: an index past the end ran\n", what, pool.threads(), n, grain); return false; }
    return true;
}

static bool with_threads(int threads)
{
    const auto pause = [] { std::this_thread::sleep_for(std::chrono::milliseconds(5)); };
    {
        Pool pool(threads);
        if (pool.threads() != threads) { printf("FAIL threads: %d of %d\n", pool.threads(), threads); return false; }
        if (!loop(pool, 0, 16, "shapes") || !loop(pool, 5, 8, "shapes") || !loop(pool, 8, 8, "shapes") || !loop(pool, 1000, 64, "shapes") ||
            !loop(pool, 257, 1, "shapes") || !loop(pool, 9, 8, "shapes"))
            return false;
        for (int k = 0; k < 3000; k++)
            if (!loop(pool, 48 + (size_t)(k % 7), 4, "spinning")) return false;
        for (int k = 0; k < 4; k++) {
            pause();
            if (!loop(pool, 300, 16, "asleep")) return false;
        }
        for (int k = 0; k < 3; k++)
            if (!loop(pool, 64 * (size_t)threads, 1, "slow worker", true)) return false;
    } // (destroyed right after a loop)
    {
        Pool pool(threads);
        if (!loop(pool, 100, 8, "destruction")) return false;
        pause();
    } // (... and with its workers asleep)
    { Pool idle(threads); } // (... and before any loop)
    return true;
}

int main()
{
    for (int threads : {1, 2, 4, 8})
        if (!with_threads(threads)) return 1;
    printf("ok %ld\n", loops);
    return 0;
}
