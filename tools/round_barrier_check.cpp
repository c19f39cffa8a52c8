// Host check of the barrier the partitions of a multi-device adaptive frame meet at (csrc/host/round_barrier.h; no HIP).  Build and run:
//   g++ -std=c++17 -O1 -g -pthread -Imetal-pathtracer-arm64_amd/csrc/host tools/round_barrier_check.cpp -o /tmp/round_barrier_check \
//       && timeout 20 /tmp/round_barrier_check
// (with -fsanitize=thread for a race check).  Part 1: 1, 2 and 9 threads run 1,000 rounds of two barriers each around a shared counter
// that every thread checks every round.  Part 2: for every thread and several rounds, that thread calls fail() instead of arriving - at
// the first or at the second barrier of the round - and every other thread must get `false` in that round and return.  A barrier that
// hangs on the missing thread never ends: run the program under a time limit.  Part 2 alone must take less than a second.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "round_barrier.h"

namespace {

constexpr uint32_t kNever = 0xFFFFFFFFu;

// `threads` threads, `rounds` rounds; thread `failer` (kNever: nobody) calls fail() at barrier `failAt` (0 or 1) of round `failRound`.
// Returns the number of findings.
int run(uint32_t threads, uint32_t rounds, uint32_t failer, uint32_t failRound, uint32_t failAt) {
    ptr::RoundBarrier barrier(threads);
    std::atomic<uint64_t> counter{0};
    std::atomic<int> findings{0};
    std::vector<uint32_t> leftAt(threads, kNever), leftBarrier(threads, kNever);
    auto body = [&](uint32_t t) {
        for (uint32_t r = 0; r < rounds; ++r) {
            counter.fetch_add(1);
            for (uint32_t which = 0; which < 2u; ++which) {
                if (t == failer && r == failRound && which == failAt) {
                    barrier.fail();
                    return;
                }
                if (!barrier.arriveAndWait()) {
                    leftAt[t] = r;
                    leftBarrier[t] = which;
                    return;
                }
                // between the two barriers of round r every thread has added its one
                if (which == 0u && counter.load() != static_cast<uint64_t>(threads) * (r + 1u)) findings.fetch_add(1);
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(body, t);
    body(0u);
    for (std::thread& th : pool) th.join();
    int bad = findings.load();
    for (uint32_t t = 0; t < threads; ++t) {
        if (failer == kNever) {
            if (leftAt[t] != kNever) ++bad;
        } else if (t != failer && (leftAt[t] != failRound || leftBarrier[t] != failAt)) {
            ++bad;   // everybody else is released at the barrier the failer stayed away from
        }
    }
    if (failer != kNever) {
        if (!barrier.failed() || barrier.arriveAndWait()) ++bad;   // ... and the barrier stays failed for later arrivals
    } else if (barrier.failed() || counter.load() != static_cast<uint64_t>(threads) * rounds) {
        ++bad;
    }
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    const uint32_t sizes[3] = {1u, 2u, 9u};
    for (uint32_t threads : sizes) bad += run(threads, 1000u, kNever, 0u, 0u);
    std::printf("round barrier check: 1, 2 and 9 threads x 1000 rounds: %d finding(s)\n", bad);
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t runs = 0;
    const uint32_t failRounds[3] = {0u, 1u, 7u};
    for (uint32_t threads : sizes) {
        for (uint32_t failer = 0; failer < threads; ++failer) {
            for (uint32_t r : failRounds) {
                for (uint32_t which = 0; which < 2u; ++which, ++runs) bad += run(threads, 10u, failer, r, which);
            }
        }
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("round barrier check: %u runs with a failing thread in %.3f s: %d finding(s) in all\n", runs, seconds, bad);
    if (seconds >= 1.0) {
        std::printf("round barrier check: the failing runs took a second or more\n");
        ++bad;
    }
    return bad == 0 ? 0 : 1;
}
