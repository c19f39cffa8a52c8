// The barrier the partitions of a multi-device adaptive frame meet at between the steps of a round (include/ptr_multi.h, multi.cpp).
// Host only, no HIP.  Unlike std::barrier it cannot hang on a participant that fails: a worker that cannot go on calls fail() instead
// of arriving, which releases every thread that waits now and every thread that arrives later, for good.
//
//   arriveAndWait()  blocks until all `count` participants of the current generation have arrived; true when they all did, false once
//                    any participant has called fail() (before, while or after this call waits).
//   fail()           may be called by anyone, any number of times, also by a thread that never arrives.
//
// After a false return a participant must not arrive again expecting company: every later call returns false at once.
// tools/round_barrier_check.cpp drives it with 1, 2 and 9 threads, with and without failures.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <mutex>

namespace ptr {

class RoundBarrier {
public:
    explicit RoundBarrier(uint32_t count) : count_(count ? count : 1u) {}
    RoundBarrier(const RoundBarrier&) = delete;
    RoundBarrier& operator=(const RoundBarrier&) = delete;

    bool arriveAndWait() {
        std::unique_lock<std::mutex> lock(m_);
        if (failed_) return false;
        const uint64_t generation = generation_;
        if (++arrived_ == count_) {   // the last one in opens the next generation
            arrived_ = 0u;
            ++generation_;
            lock.unlock();
            wake_.notify_all();
            return true;
        }
        wake_.wait(lock, [&] { return failed_ || generation_ != generation; });
        // a generation that completed before the failure was complete: its waiters go on and meet the failure at their next call
        return generation_ != generation;
    }

    void fail() {
        {
            std::lock_guard<std::mutex> lock(m_);
            failed_ = true;
        }
        wake_.notify_all();
    }

    bool failed() const {
        std::lock_guard<std::mutex> lock(m_);
        return failed_;
    }

private:
    mutable std::mutex m_;
    std::condition_variable wake_;
    const uint32_t count_;
    uint32_t arrived_ = 0u;
    uint64_t generation_ = 0u;
    bool failed_ = false;
};

}  // namespace ptr
