// hostwait.hpp -- the host's half of the completion protocol of the kernels that run a whole problem in one launch
// (window.hip, wincov.hip) or publish a score (solver.hip: publish_parts): the host clears the sequence number of every
// record in mapped pinned memory, hands the kernel a new number that is never 0, the kernel stores it LAST (release,
// system scope), and the host polls for it instead of waiting for the runtime's completion signal (5-10 us of a 60 us
// call). Plain C++ with no HIP type in it, as winbatch.hpp (tools/hostwait_check.cpp runs it under sanitizers).
#pragma once
#include <sched.h>

#include <chrono>
#include <cstddef>

namespace irh {

inline double now_seconds() {
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// The next sequence number, never 0 (which is what the host leaves in a record). Counted in unsigned: INT_MAX is followed
// by INT_MIN and -1 by 1 without signed overflow; the kernels compare for equality only.
inline int next_seq(int &seq) {
    const unsigned u = (unsigned)seq + 1u;
    return seq = (int)(u ? u : 1u);
}

// Waits until `count` records, `stride_bytes` apart from `first` on, all show `want`: walks them in order with acquire
// loads, pauses between looks, and reads the clock every 256 looks -- so a wait that runs out gives up some microseconds
// after `limit_s`, not at it. Past `yield_after_s` (0: never) the core is given away at every reading of the clock: a
// wait that outlasts every kernel of a step (l1ra's three polling threads on a host with few cores).
// false: the limit passed (long kernels, inputs still in flight, a kernel that died) -- the caller synchronises its stream.
inline bool wait_seq(const int *first, size_t stride_bytes, size_t count, int want, double limit_s,
                     double yield_after_s = 0.0) {
    const double t0 = now_seconds();
    size_t next = 0;
    for (unsigned looks = 1;; looks++) {
        while (next < count &&
               __atomic_load_n(reinterpret_cast<const int *>(reinterpret_cast<const unsigned char *>(first) + stride_bytes * next),
                               __ATOMIC_ACQUIRE) == want)
            next++;
        if (next == count) return true;
        if ((looks & 255u) == 0) {
            const double dt = now_seconds() - t0;
            if (dt > limit_s) return false;
            if (yield_after_s > 0.0 && dt > yield_after_s) sched_yield();
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

}  // namespace irh
