// hostwait_check.cpp -- the host's half of the completion protocol (irotavg_amd/csrc/hostwait.hpp: next_seq, wait_seq)
// and the staging layout of the window kernels (winbatch.hpp: win_stage) as a stand-alone program that needs no device;
// a std::thread plays the kernel. Meant to be built with sanitizers, once each:
//   g++ -std=c++17 -g -O2 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/hostwait_check.cpp -o hostwait_check && ./hostwait_check
//   g++ -std=c++17 -g -O2 -pthread -fsanitize=thread -Iirotavg_amd/csrc tools/hostwait_check.cpp -o hostwait_check_tsan
// Exit status 0 and "hostwait check ok" when every expectation holds.
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "hostwait.hpp"
#include "winbatch.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
            failures++;                                                  \
        }                                                                \
    } while (0)

static void nap(double seconds) { std::this_thread::sleep_for(std::chrono::duration<double>(seconds)); }

// `steps` numbers from `from` on: never 0, never the one before; returns the last
static int run_seq(int from, unsigned long long steps) {
    int seq = from;
    unsigned long long bad = 0;
    for (unsigned long long i = 0; i < steps; i++) {
        const int before = seq, got = next_seq(seq);
        bad += (got == 0) | (got == before) | (got != seq);
    }
    EXPECT(bad == 0);
    return seq;
}

// A row of records as a kernel leaves them: a payload, then the sequence number (release). The stride is larger than
// the record and no multiple of its size.
struct Rec {
    double payload[2];
    int status, seq;
};
constexpr size_t kStride = sizeof(Rec) + 40;
struct Row {
    std::vector<unsigned char> mem;
    size_t n;
    explicit Row(size_t count, int seq0 = 0) : mem(kStride * count, 0xee), n(count) {
        for (size_t b = 0; b < n; b++) at(b)->seq = seq0;  // the host's clearing, before the "launch"
    }
    Rec *at(size_t b) { return reinterpret_cast<Rec *>(mem.data() + kStride * b); }
    const int *first() { return &at(0)->seq; }
    void kernel_store(size_t b, int seq) {
        Rec *r = at(b);
        r->payload[0] = 1.5 * (double)b;
        r->payload[1] = (double)seq;
        r->status = (int)b;
        __atomic_store_n(&r->seq, seq, __ATOMIC_RELEASE);
    }
    bool payload_ok(int seq) {
        bool ok = true;
        for (size_t b = 0; b < n; b++)
            ok = ok && at(b)->payload[0] == 1.5 * (double)b && at(b)->payload[1] == (double)seq && at(b)->status == (int)b;
        return ok;
    }
};

int main() {
    // 1. sequence numbers
    {
        int s = 0;
        EXPECT(next_seq(s) == 1 && s == 1);
        s = -1;
        EXPECT(next_seq(s) == 1 && s == 1);
        s = INT_MAX;
        EXPECT(next_seq(s) == INT_MIN && s == INT_MIN);
        s = INT_MIN;
        EXPECT(next_seq(s) == INT_MIN + 1);
        EXPECT(run_seq(0, 1000) == 1000 && run_seq(-1, 3) == 3 && run_seq(INT_MAX, 2) == INT_MIN + 1);
        // once round and past the skipped 0: 2^32 - 1 steps bring 1 back to 1, four more to 5
        EXPECT(run_seq(1, (1ull << 32) + 3) == 5);
    }
    // 2. one record, stored after a short delay
    {
        Row R(1);
        std::thread k([&] {
            nap(200e-6);
            R.kernel_store(0, 7);
        });
        EXPECT(wait_seq(R.first(), 0, 1, 7, 1.0));
        k.join();
        EXPECT(R.payload_ok(7));
    }
    // 3. rows stored in reverse order: complete only once the first record, which is stored last, is there
    for (size_t n : {(size_t)1, (size_t)2, (size_t)65}) {
        Row R(n);
        const int want = -5;
        for (size_t b = n; b-- > 1;) R.kernel_store(b, want);
        EXPECT(!wait_seq(R.first(), kStride, n, want, 200e-6));  // all but the first: not enough
        Row S(n);
        std::atomic<bool> last_begun{false};
        std::thread k([&] {
            for (size_t b = n; b-- > 1;) {
                S.kernel_store(b, want);
                if (b % 16 == 1) nap(50e-6);
            }
            nap(100e-6);
            last_begun.store(true);
            S.kernel_store(0, want);
        });
        EXPECT(wait_seq(S.first(), kStride, n, want, 1.0));
        EXPECT(last_begun.load());
        k.join();
        EXPECT(S.payload_ok(want));
    }
    // 4. a record that never arrives: false, no sooner than the limit and not much later
    {
        Row R(3);
        R.kernel_store(0, 9);
        const double t0 = now_seconds();
        EXPECT(!wait_seq(R.first(), kStride, 3, 9, 1e-3));
        const double dt = now_seconds() - t0;
        EXPECT(dt >= 1e-3 && dt < 50e-3);
        const double t1 = now_seconds();
        EXPECT(!wait_seq(R.first(), kStride, 3, 9, 1e-3, 10e-6));  // yielding on the way
        const double dy = now_seconds() - t1;
        EXPECT(dy >= 1e-3 && dy < 50e-3);
    }
    // 5. the last call's number in every record is not this call's
    {
        int seq = 41;
        const int stale = seq, want = next_seq(seq);
        Row R(4, stale);
        EXPECT(!wait_seq(R.first(), kStride, 4, want, 1e-3));
        std::thread k([&] {
            for (size_t b = 0; b < 4; b++) R.kernel_store(b, want);
        });
        EXPECT(wait_seq(R.first(), kStride, 4, want, 1.0));
        k.join();
        EXPECT(R.payload_ok(want));
    }
    // 6. with and without yielding
    for (double yield_after : {0.0, 10e-6}) {
        Row R(2);
        std::thread k([&] {
            nap(300e-6);
            R.kernel_store(1, 3);
            R.kernel_store(0, 3);
        });
        EXPECT(wait_seq(R.first(), kStride, 2, 3, 1.0, yield_after));
        k.join();
        EXPECT(R.payload_ok(3));
    }
    // 7. the staging layout at both capacities: the literal sums the two host paths spelled out before they shared it
    {
        EXPECT(sizeof(WinResult) == 96 && sizeof(WinParams) == 48);
        const WinStage a = win_stage(WIN_MAX_NE), b = win_stage(SM_MAX_NE);
        EXPECT(a.oI == 0 && a.oQQ == 8 * 640 && a.oQ == a.oQQ + 32 * 640 && a.oW == a.oQ + 32 * 320 &&
               a.oR == a.oW + 8 * 640 && a.oP == a.oR + 96 && a.oP == 41056);
        EXPECT(b.oI == 0 && b.oQQ == 8 * 64 && b.oQ == b.oQQ + 32 * 64 && b.oW == b.oQ + 32 * 320 &&
               b.oR == b.oW + 8 * 64 && b.oP == b.oR + 96 && b.stride == ((b.oP + 48 + 255) & ~(size_t)255));
        EXPECT(a.oQQ == 5120 && a.oQ == 25600 && a.oW == 35840 && a.oR == 40960 && a.stride == 41216);
        EXPECT(b.oQQ == 512 && b.oQ == 2560 && b.oW == 12800 && b.oR == 13312 && b.oP == 13408 && b.stride == 13568);
    }
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("hostwait check ok\n");
    return 0;
}
