// cycles.hip -- the triangle test of every edge (irotavg_cycle_check, irotavg_cycle_check_dev; docs/cycle_check.md), four
// steps on one stream:
//   1. k_cyc_emit       range-checks both ends of every edge (a bad id stores 1 into the error word: every writer stores
//                       the same value, so no atomic) and emits its two half-edges (cycles.hpp: key, value);
//   2. rocprim::radix_sort_pairs over the key bits n_total needs: the rows of all views, neighbours ascending;
//   3. k_cyc_triangles  one group of G lanes per edge: the rows of both ends by binary search, the shorter one dealt to
//                       the lanes, each entry looked up in the longer one (cyc_entry), sums per lane, shuffles within the
//                       group, lane 0 stores; it returns at once when the error word is set, so nothing is indexed with
//                       a bad id and no output byte is written;
//   4. k_cyc_summary    the workgroups' four sums added up in a fixed order; error word and summary are read back.
// No atomics, no flag between workgroups, no loop that is not bounded by a row length or 32 rounds of a search. The sums
// are integers and the one floating-point reduction is a minimum: no result depends on an order. Memory: 2m keys and
// values twice (sort in, sort out), the sort's own storage, an AoS image of QQ unless the caller's rows are 16-byte rows
// already -- nothing grows with n_total.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <atomic>

#include "graph.hpp"
#include "kernels.hpp"   // tile_range
#include "winbatch.hpp"  // rows16
#include "cycles.hpp"

namespace irh {
namespace {

constexpr int kT = 256;
constexpr int kCycDefaultGroup = 8;  // the fastest of 8, 16, 32, 64 on all three measured graphs (docs/cycle_check.md)
constexpr int kCycMaxGrid = 4096;  // a multiple of 8: tile_range deals adjacent chunks to the workgroups of one XCD
constexpr int kCycPasses = 4;      // a small graph still gives every workgroup a few passes over its chunk

inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

__global__ __launch_bounds__(kT) void k_cyc_emit(long long m, long long n_total, const int2 *__restrict__ I,
                                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                 long long *__restrict__ err) {
    const long long k = (long long)blockIdx.x * kT + threadIdx.x;
    if (k >= m) return;
    const int2 e = I[k];
    const bool ok = cyc_id_ok(e.x, n_total) && cyc_id_ok(e.y, n_total);
    if (!ok) *err = 1;
    uint64_t key[2];
    uint32_t val[2];
    cyc_emit((uint32_t)k, e.x, e.y, ok, key, val);
    keys[2 * k] = key[0];
    keys[2 * k + 1] = key[1];
    reinterpret_cast<uint2 *>(vals)[k] = make_uint2(val[0], val[1]);
}

// the AoS image of a strided QQ (rows that are not 16-byte rows): one edge per thread
__global__ __launch_bounds__(kT) void k_cyc_image(long long m, const double *__restrict__ src, long long rs, long long cs,
                                                  double2 *__restrict__ img) {
    const long long k = (long long)blockIdx.x * kT + threadIdx.x;
    if (k >= m) return;
    const double *r = src + k * rs;
    img[2 * k] = make_double2(r[0], r[cs]);
    img[2 * k + 1] = make_double2(r[2 * cs], r[3 * cs]);
}

struct CycDevLoad {  // QQ_k as two 16-byte loads
    const double2 *q;
    __host__ __device__ CycQ operator()(uint32_t k) const {
        const double2 lo = q[2 * (size_t)k], hi = q[2 * (size_t)k + 1];
        return CycQ{lo.x, lo.y, hi.x, hi.y};
    }
};

template <int G>
__global__ __launch_bounds__(kT) void k_cyc_triangles(int m, long long n2, const uint64_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ vals, const int2 *__restrict__ I,
                                                      const double2 *__restrict__ qq, double threshold,
                                                      const long long *__restrict__ err, int32_t *__restrict__ tri_count,
                                                      int32_t *__restrict__ tri_ok, double *__restrict__ tri_min,
                                                      long long *__restrict__ parts) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a group lies within one wave");
    constexpr int kEdges = kT / G;  // edges of one pass
    __shared__ long long red[kT / 64][4];
    if (*err != 0) return;  // (uniform: a bad id; nothing is indexed with it and nothing is written)
    int e0, e1;
    tile_range(m, e0, e1);
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const CycDevLoad load{qq};
    long long sum[4] = {0, 0, 0, 0};  // triangles, supported, contradicted, untested (lane 0 of a group alone adds)
    for (int base = e0; base < e1; base += kEdges) {
        const int k = base + grp;
        const bool valid = k < e1;
        const int2 e = valid ? I[k] : make_int2(0, 0);
        const bool skip = !valid || e.x == e.y;
        // lanes 0..3 of the group look up one row boundary each: the start of row a, its end, the start of row b, its end
        long long r = 0;
        if (!skip && lane < 4) r = cyc_lower_bound(keys, 0, n2, cyc_key((uint32_t)((lane & 2) ? e.y : e.x) + (uint32_t)(lane & 1), 0u));
        const long long a0 = __shfl(r, 0, G), a1 = __shfl(r, 1, G), b0 = __shfl(r, 2, G), b1 = __shfl(r, 3, G);
        CycAcc acc = cyc_acc_zero();
        if (!skip) {
            const bool x_is_b = b1 - b0 <= a1 - a0;  // the shorter row is walked, the longer one searched
            const long long s0 = x_is_b ? b0 : a0, s1 = x_is_b ? b1 : a1, l0 = x_is_b ? a0 : b0, l1 = x_is_b ? a1 : b1;
            const uint32_t y = (uint32_t)(x_is_b ? e.x : e.y);
            const CycQ q0 = load((uint32_t)k);
            for (long long i = s0 + lane; i < s1; i += G) cyc_entry(keys, vals, i, y, x_is_b, l0, l1, q0, threshold, load, acc);
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1)
            cyc_acc_merge(acc, __shfl_xor(acc.count, o, G), __shfl_xor(acc.ok, o, G), __shfl_xor(acc.mn, o, G));
        if (valid && lane == 0) {
            const int32_t c = cyc_stored_count(acc.count), o = cyc_stored_count(acc.ok);
            if (tri_count) tri_count[k] = c;
            if (tri_ok) tri_ok[k] = o;
            if (tri_min) tri_min[k] = acc.mn;
            sum[0] += c;
            sum[o >= 1 ? 1 : c >= 1 ? 2 : 3]++;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        for (int o = 32; o > 0; o >>= 1) sum[j] += __shfl_xor(sum[j], o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = sum[j];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        long long s = 0;
        for (int w = 0; w < kT / 64; w++) s += red[w][threadIdx.x];
        parts[4 * (size_t)blockIdx.x + threadIdx.x] = s;
    }
}

// head[0] is the error word, head[1..4] the summary; with the error word set the partial sums were never written
__global__ __launch_bounds__(kT) void k_cyc_summary(int nparts, const long long *__restrict__ parts, long long *__restrict__ head) {
    __shared__ long long red[kT][4];
    if (head[0] != 0) return;
    long long s[4] = {0, 0, 0, 0};
    for (int p = threadIdx.x; p < nparts; p += kT)
        for (int j = 0; j < 4; j++) s[j] += parts[4 * (size_t)p + j];
    for (int j = 0; j < 4; j++) red[threadIdx.x][j] = s[j];
    __syncthreads();
    for (int o = kT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int j = 0; j < 4; j++) red[threadIdx.x][j] += red[threadIdx.x + o][j];
        __syncthreads();
    }
    if (threadIdx.x < 4) head[1 + threadIdx.x] = red[0][threadIdx.x];
}

std::atomic<int> g_group{kCycDefaultGroup};

template <int G>
void launch_triangles(int grid, hipStream_t s, int m, long long n2, const uint64_t *keys, const uint32_t *vals, const int2 *I,
                      const double2 *qq, double threshold, const long long *err, const CycleArrays &A, long long *parts) {
    hipLaunchKernelGGL(k_cyc_triangles<G>, dim3((unsigned)grid), dim3(kT), 0, s, m, n2, keys, vals, I, qq, threshold, err,
                       A.tri_count, A.tri_ok, A.tri_min, parts);
}

}  // namespace

int cycle_check_group(int lanes) {
    if (lanes == 0) lanes = kCycDefaultGroup;
    if (lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64) return IROTAVG_ERR_BAD_ARG;
    return g_group.exchange(lanes);
}

int cycle_check_dev(int64_t m, int64_t n_total, const CycleArrays &A, double threshold, int64_t *summary, hipStream_t stream) {
    const long long n2 = 2 * (long long)m;
    const bool triangles = A.tri_count || A.tri_ok || A.tri_min || summary;
    const bool own_rows = rows16(reinterpret_cast<uintptr_t>(A.QQ), A.qq_rs, A.qq_cs);
    const int G = g_group.load();
    // the workgroups of the triangle kernel: kCycPasses passes each while the graph is small, then longer chunks
    long long nwg = std::max<long long>(1, (m + (long long)(kT / G) * kCycPasses - 1) / ((long long)(kT / G) * kCycPasses));
    if (nwg > 8) nwg = std::min<long long>(kCycMaxGrid, (nwg + 7) / 8 * 8);
    // every temporary first (the pool): nothing after the first launch can fail for want of memory
    DevBuf<uint64_t> kin, kout;
    DevBuf<uint32_t> vin, vout;
    DevBuf<char> tmp;
    DevBuf<double2> img;
    DevBuf<long long> parts, head;
    const unsigned bits = (unsigned)cyc_key_bits(n_total);
    size_t bytes = 0;
    kin.alloc((size_t)n2);
    vin.alloc((size_t)n2);
    head.alloc(5);
    if (triangles) {  // (the id check alone ends behind the first kernel)
        IRH_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                            (uint32_t *)nullptr, (size_t)n2, 0u, bits, stream));
        kout.alloc((size_t)n2);
        vout.alloc((size_t)n2);
        tmp.alloc(std::max<size_t>(bytes, 1));
        if (!own_rows) img.alloc(2 * (size_t)m);
        parts.alloc(4 * (size_t)nwg);
    }
    const int2 *I2 = reinterpret_cast<const int2 *>(A.I);
    IRH_CHECK(hipMemsetAsync(head.p, 0, 5 * sizeof(long long), stream));
    hipLaunchKernelGGL(k_cyc_emit, dim3(grid_of(m)), dim3(kT), 0, stream, (long long)m, (long long)n_total, I2, kin.p, vin.p,
                       head.p);
    IRH_CHECK(hipGetLastError());
    if (triangles) {
        IRH_CHECK(rocprim::radix_sort_pairs(tmp.p, bytes, kin.p, kout.p, vin.p, vout.p, (size_t)n2, 0u, bits, stream));
        const double2 *qq = reinterpret_cast<const double2 *>(A.QQ);
        if (!own_rows) {
            hipLaunchKernelGGL(k_cyc_image, dim3(grid_of(m)), dim3(kT), 0, stream, (long long)m, A.QQ, A.qq_rs, A.qq_cs, img.p);
            IRH_CHECK(hipGetLastError());
            qq = img.p;
        }
        switch (G) {
        case 8: launch_triangles<8>((int)nwg, stream, (int)m, n2, kout.p, vout.p, I2, qq, threshold, head.p, A, parts.p); break;
        case 32: launch_triangles<32>((int)nwg, stream, (int)m, n2, kout.p, vout.p, I2, qq, threshold, head.p, A, parts.p); break;
        case 64: launch_triangles<64>((int)nwg, stream, (int)m, n2, kout.p, vout.p, I2, qq, threshold, head.p, A, parts.p); break;
        default: launch_triangles<16>((int)nwg, stream, (int)m, n2, kout.p, vout.p, I2, qq, threshold, head.p, A, parts.p);
        }
        IRH_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_cyc_summary, dim3(1), dim3(kT), 0, stream, (int)nwg, parts.p, head.p);
        IRH_CHECK(hipGetLastError());
    }
    long long h[5] = {0, 0, 0, 0, 0};
    IRH_CHECK(hipMemcpyAsync(h, head.p, sizeof(h), hipMemcpyDeviceToHost, stream));
    IRH_CHECK(hipStreamSynchronize(stream));  // (the temporaries go back to the pool idle)
    if (h[0] != 0) return IROTAVG_ERR_BAD_ARG;
    if (summary)
        for (int j = 0; j < 4; j++) summary[j] = h[1 + j];
    return IROTAVG_OK;
}

int cycle_check_host(int64_t m, int64_t n_total, const CycleArrays &A, double threshold, int64_t *summary) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m;
    DevBuf<int32_t> dI, dcount, dok;
    DevBuf<double> dqq, dmin;
    dI.alloc(2 * um);
    dqq.alloc(4 * um);  // four planes of m
    if (A.tri_count) dcount.alloc(um);
    if (A.tri_ok) dok.alloc(um);
    if (A.tri_min) dmin.alloc(um);
    IRH_CHECK(hipMemcpyAsync(dI.p, A.I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    for (int c = 0; c < 4; c++)
        IRH_CHECK(hipMemcpyAsync(dqq.p + c * um, A.QQ + c * A.qq_cs, um * sizeof(double), hipMemcpyHostToDevice, s));
    const CycleArrays D{dI.p, dqq.p, 1, (long long)m, A.tri_count ? dcount.p : nullptr, A.tri_ok ? dok.p : nullptr,
                        A.tri_min ? dmin.p : nullptr};
    int64_t sum[4] = {0, 0, 0, 0};
    const int rc = cycle_check_dev(m, n_total, D, threshold, summary ? sum : nullptr, s);
    if (rc != IROTAVG_OK) return rc;
    if (A.tri_count) IRH_CHECK(hipMemcpyAsync(A.tri_count, dcount.p, um * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (A.tri_ok) IRH_CHECK(hipMemcpyAsync(A.tri_ok, dok.p, um * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (A.tri_min) IRH_CHECK(hipMemcpyAsync(A.tri_min, dmin.p, um * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    if (summary)
        for (int j = 0; j < 4; j++) summary[j] = sum[j];
    return IROTAVG_OK;
}

}  // namespace irh
