// cemp.hip -- a corruption estimate for every edge by cycle-edge message passing over its triangles (irotavg_cycle_cemp,
// irotavg_cycle_cemp_dev; docs/cycle_check.md, "Corruption estimates"), on one stream:
//   1. emit, sort, AoS image   those of the triangle test (cycles.hip: cyc_prep_alloc / cyc_prep_run);
//   2. k_cemp_walk<COUNT>   the triangle kernel's geometry (one group of G lanes per edge, the shorter row dealt to the
//                           lanes, the longer one searched): a 64-bit count of the used triangles per edge, and per
//                           workgroup the sum of the counts and the edges without one;
//   3. rocprim::exclusive_scan of the counts: the 64-bit segment offsets; k_cyc_summary (cyc_finish) adds the workgroups'
//                           sums. The total, the untested edges and the error word come back in ONE host wait: the bad
//                           id and the cap on the records are decided there, before any output is touched, and only
//                           then is the table sized and taken from the pool;
//   4. k_cemp_walk<FILL>    the same enumeration once more: per round the lanes' hit counts go through a group-wide
//                           prefix, and every lane stores its 16-byte records at segment start + records of the rounds
//                           done + records of the lower lanes (cemp_slot): the order of the definition for every G. The
//                           lanes' sums of d in slot order and the shuffle tree give the start vector, tri_used is stored;
//   5. k_cemp_iter          the hot path, one launch per iteration: one group of G lanes per edge streams the edge's
//                           segment with 16-byte loads, coalesced across the group, gathers the two estimates of every
//                           record from the plane of the last iteration, forms the shift (the smallest sum), then the
//                           two weighted sums. A lane keeps the first kHold rounds of its segment in registers between
//                           the two steps; a longer segment is walked a second time from there on. Two planes of m
//                           doubles ping-pong; the last iteration stores into the caller's s. The in-order stream is the
//                           only barrier between iterations.
// No atomics, no flag between workgroups, no persistent or cooperative launch; every loop is bounded by a row or segment
// length or by 32 rounds of a search. Memory: the triangle test's O(m), 16 bytes per edge for counts and offsets, two
// planes of m doubles, and 16 bytes per used triangle.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "graph.hpp"
#include "kernels.hpp"  // tile_range
#include "cemp.hpp"
#include "cycload.hpp"

#ifndef IRH_CEMP_GROUP
#define IRH_CEMP_GROUP 8  // the faster of 8 and 16 on both measured graphs (docs/cycle_check.md); not an interface
#endif

namespace irh {
namespace {

constexpr int kT = 256;
constexpr int kG = IRH_CEMP_GROUP;
constexpr int kCempMaxGrid = 4096;  // a multiple of 8: tile_range deals adjacent chunks to the workgroups of one XCD
constexpr int kCempPasses = 4;      // a small graph still gives every workgroup a few passes over its chunk
constexpr int kHold = 4;            // rounds of a segment a lane of k_cemp_iter keeps in registers: 4 G records per edge
enum { CEMP_COUNT = 0, CEMP_FILL = 1 };

inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

// COUNT: cnt is written, parts get the workgroup's sums (records, -, -, edges without one; the layout of k_cyc_summary).
// FILL: cnt and off are read, the table, s0 and tri_used (either may be nullptr) are written.
template <int MODE, int G>
__global__ __launch_bounds__(kT) void k_cemp_walk(int m, long long n2, const uint64_t *__restrict__ keys,
                                                  const uint32_t *__restrict__ vals, const int2 *__restrict__ I,
                                                  const double2 *__restrict__ qq, const long long *__restrict__ err,
                                                  long long *__restrict__ cnt, const long long *__restrict__ off,
                                                  CempRec *__restrict__ table, double *__restrict__ s0,
                                                  int32_t *__restrict__ tri_used, long long *__restrict__ parts) {
    static_assert(G == 8 || G == 16, "a group lies within one wave");
    constexpr int kEdges = kT / G;  // edges of one pass
    __shared__ long long red[kT / 64][2];
    if (*err != 0) return;  // (uniform: a bad id; nothing is indexed with it and nothing is written)
    int e0, e1;
    tile_range(m, e0, e1);
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const CycDevLoad load{qq};
    long long sum[2] = {0, 0};  // records, edges without one (lane 0 of a group alone adds)
    for (int base = e0; base < e1; base += kEdges) {
        const int k = base + grp;
        const bool valid = k < e1;
        const int2 e = valid ? I[k] : make_int2(0, 0);
        const bool skip = !valid || e.x == e.y;
        // lanes 0..3 of the group look up one row boundary each: the start of row a, its end, the start of row b, its end
        long long r = 0;
        if (!skip && lane < 4) r = cyc_lower_bound(keys, 0, n2, cyc_key((uint32_t)((lane & 2) ? e.y : e.x) + (uint32_t)(lane & 1), 0u));
        const long long a0 = __shfl(r, 0, G), a1 = __shfl(r, 1, G), b0 = __shfl(r, 2, G), b1 = __shfl(r, 3, G);
        const long long seg = MODE == CEMP_FILL && valid ? off[k] : 0, count = MODE == CEMP_FILL && valid ? cnt[k] : 0;
        long long mine = 0;  // COUNT: the lane's used triangles
        double lsum = 0.0;   // FILL: the lane's sum of d, in slot order
        if (!skip) {
            const bool x_is_b = b1 - b0 <= a1 - a0;  // the shorter row is walked, the longer one searched
            const long long x0 = x_is_b ? b0 : a0, x1 = x_is_b ? b1 : a1, l0 = x_is_b ? a0 : b0, l1 = x_is_b ? a1 : b1;
            const uint32_t y = (uint32_t)(x_is_b ? e.x : e.y);
            const CycQ q0 = load((uint32_t)k);
            long long done = 0;
            for (long long round = x0; round < x1; round += G) {  // (uniform in the group: the shuffles below are whole)
                const long long i = round + lane;
                CempHits h{0, CempRec{0.0, 0u, 0u}};
                if (i < x1) cemp_entry(keys, vals, i, y, x_is_b, l0, l1, q0, load, h);
                if (MODE == CEMP_COUNT) {
                    mine += h.n;
                    continue;
                }
                int upto = h.n;  // the hits of this lane and the lower ones
#pragma unroll
                for (int o = 1; o < G; o <<= 1) {
                    const int v = __shfl_up(upto, o, G);
                    if (lane >= o) upto += v;
                }
                CempRec *const at = table + cemp_slot(seg, done, upto - h.n);
                if (h.n == 1) {
                    if (at < table + seg + count) *at = h.first;
                    lsum += h.first.d;
                } else if (h.n > 1) {
                    CempStore w{at, table + seg + count, lsum};
                    cemp_entry(keys, vals, i, y, x_is_b, l0, l1, q0, load, w);
                    lsum = w.sum;
                }
                done += __shfl(upto, G - 1, G);
            }
        }
        if (MODE == CEMP_COUNT) {
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, G);
            if (valid && lane == 0) {
                cnt[k] = mine;
                sum[0] += mine;
                sum[1] += mine == 0;
            }
        } else {
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, G);
            if (valid && lane == 0) {
                if (s0) s0[k] = cemp_mean(lsum, count);
                if (tri_used) tri_used[k] = cyc_stored_count(count);
            }
        }
    }
    if (MODE == CEMP_COUNT) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            for (int o = 32; o > 0; o >>= 1) sum[j] += __shfl_xor(sum[j], o, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = sum[j];
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            long long s = 0;
            if (threadIdx.x == 0 || threadIdx.x == 3)
                for (int w = 0; w < kT / 64; w++) s += red[w][threadIdx.x == 0 ? 0 : 1];
            parts[4 * (size_t)blockIdx.x + threadIdx.x] = s;
        }
    }
}

// tri_used alone was asked for: no table, no iteration
__global__ __launch_bounds__(kT) void k_cemp_used(long long m, const long long *__restrict__ cnt, int32_t *__restrict__ tri_used) {
    const long long k = (long long)blockIdx.x * kT + threadIdx.x;
    if (k < m) tri_used[k] = cyc_stored_count(cnt[k]);
}

template <int G>
__global__ __launch_bounds__(kT) void k_cemp_iter(int m, const long long *__restrict__ off, const long long *__restrict__ cnt,
                                                  const CempRec *__restrict__ table, const double *__restrict__ s_in,
                                                  double beta, double *__restrict__ s_out) {
    constexpr int kEdges = kT / G;
    int e0, e1;
    tile_range(m, e0, e1);
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int base = e0; base < e1; base += kEdges) {
        const int k = base + grp;
        const bool valid = k < e1;
        const long long beg = (valid ? off[k] : 0) + lane, end = valid ? off[k] + cnt[k] : 0;
        // the shift: the smallest e of the segment. The first kHold rounds stay in registers for the sums.
        double eh[kHold], dh[kHold], mu = std::numeric_limits<double>::infinity();
#pragma unroll
        for (int j = 0; j < kHold; j++) {
            eh[j] = dh[j] = 0.0;
            if (beg + j * G < end) {
                const CempRec rec = table[beg + j * G];
                eh[j] = cemp_e(s_in[rec.k1], s_in[rec.k2]);
                dh[j] = rec.d;
                cemp_min(mu, eh[j]);
            }
        }
        for (long long r = beg + kHold * G; r < end; r += G) {
            const CempRec rec = table[r];
            cemp_min(mu, cemp_e(s_in[rec.k1], s_in[rec.k2]));
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) cemp_min(mu, __shfl_xor(mu, o, G));
        CempSum a{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < kHold; j++)
            if (beg + j * G < end) cemp_term(a, dh[j], eh[j], beta, mu);
        for (long long r = beg + kHold * G; r < end; r += G) {
            const CempRec rec = table[r];
            cemp_term(a, rec.d, cemp_e(s_in[rec.k1], s_in[rec.k2]), beta, mu);
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            a.num += __shfl_xor(a.num, o, G);
            a.den += __shfl_xor(a.den, o, G);
        }
        if (valid && lane == 0) s_out[k] = cemp_quotient(a);
    }
}

}  // namespace

int cycle_cemp_dev(int64_t m, int64_t n_total, const CempArrays &A, int iters, const double *beta, int64_t max_records,
                   int64_t *summary, hipStream_t stream) {
    const long long n2 = 2 * (long long)m;
    const bool walk = A.s || A.tri_used || summary;
    long long nwg = std::max<long long>(1, (m + (long long)(kT / kG) * kCempPasses - 1) / ((long long)(kT / kG) * kCempPasses));
    if (nwg > 8) nwg = std::min<long long>(kCempMaxGrid, (nwg + 7) / 8 * 8);
    const int2 *I2 = reinterpret_cast<const int2 *>(A.I);
    // every temporary but the table first (the pool): its size is known only after the count
    CycPrep P;
    DevBuf<long long> parts, cnt, off;
    DevBuf<char> scan_tmp;
    DevBuf<double> plane[2];
    DevBuf<CempRec> table;
    size_t scan_bytes = 0;
    cyc_prep_alloc(P, m, n_total, A.QQ, A.qq_rs, A.qq_cs, walk, stream);
    if (walk) {
        parts.alloc(4 * (size_t)nwg);
        cnt.alloc((size_t)m);
        off.alloc((size_t)m);
        IRH_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, cnt.p, off.p, 0LL, (size_t)m, rocprim::plus<long long>(), stream));
        scan_tmp.alloc(std::max<size_t>(scan_bytes, 1));
        for (int p = 0; A.s && p < std::min(iters, 2); p++) plane[p].alloc((size_t)m);
    }
    cyc_prep_run(P, m, n_total, A.I, A.QQ, A.qq_rs, A.qq_cs, stream);
    if (walk) {
        hipLaunchKernelGGL((k_cemp_walk<CEMP_COUNT, kG>), dim3((unsigned)nwg), dim3(kT), 0, stream, (int)m, n2, P.kout.p, P.vout.p, I2,
                           P.qq, P.head.p, cnt.p, nullptr, nullptr, nullptr, nullptr, parts.p);
        IRH_CHECK(hipGetLastError());
        IRH_CHECK(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, cnt.p, off.p, 0LL, (size_t)m, rocprim::plus<long long>(), stream));
    }
    int64_t sum[4] = {0, 0, 0, 0};
    if (const int rc = cyc_finish(P, walk ? (int)nwg : 0, parts.p, sum, stream); rc != IROTAVG_OK || !walk) return rc;
    const int64_t records = sum[0];
    if (summary) summary[0] = records, summary[1] = sum[3];
    if (max_records > 0 && records > max_records) return IROTAVG_ERR_NOMEM;
    if (A.s) {
        try {
            table.alloc((size_t)records);
        } catch (const HipError &) {
            (void)hipGetLastError();
            return IROTAVG_ERR_NOMEM;  // (nothing but summary has been written)
        }
        hipLaunchKernelGGL((k_cemp_walk<CEMP_FILL, kG>), dim3((unsigned)nwg), dim3(kT), 0, stream, (int)m, n2, P.kout.p, P.vout.p, I2,
                           P.qq, P.head.p, cnt.p, off.p, table.p, iters == 0 ? A.s : plane[0].p, A.tri_used, nullptr);
        IRH_CHECK(hipGetLastError());
        for (int t = 0; t < iters; t++) {
            hipLaunchKernelGGL((k_cemp_iter<kG>), dim3((unsigned)nwg), dim3(kT), 0, stream, (int)m, off.p, cnt.p, table.p,
                               plane[t & 1].p, beta[t], t == iters - 1 ? A.s : plane[(t + 1) & 1].p);
            IRH_CHECK(hipGetLastError());
        }
    } else if (A.tri_used) {
        hipLaunchKernelGGL(k_cemp_used, dim3(grid_of(m)), dim3(kT), 0, stream, (long long)m, cnt.p, A.tri_used);
        IRH_CHECK(hipGetLastError());
    }
    IRH_CHECK(hipStreamSynchronize(stream));  // (the temporaries go back to the pool idle)
    return IROTAVG_OK;
}

int cycle_cemp_host(int64_t m, int64_t n_total, const CempArrays &A, int iters, const double *beta, int64_t max_records,
                    int64_t *summary) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m;
    DevBuf<int32_t> dI, dused;
    DevBuf<double> dqq, ds;
    dI.alloc(2 * um);
    dqq.alloc(4 * um);  // four planes of m
    if (A.s) ds.alloc(um);
    if (A.tri_used) dused.alloc(um);
    IRH_CHECK(hipMemcpyAsync(dI.p, A.I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    for (int c = 0; c < 4; c++)
        IRH_CHECK(hipMemcpyAsync(dqq.p + c * um, A.QQ + c * A.qq_cs, um * sizeof(double), hipMemcpyHostToDevice, s));
    const CempArrays D{dI.p, dqq.p, 1, (long long)m, ds.p, dused.p};
    const int rc = cycle_cemp_dev(m, n_total, D, iters, beta, max_records, summary, s);
    if (rc != IROTAVG_OK) return rc;
    if (A.s) IRH_CHECK(hipMemcpyAsync(A.s, ds.p, um * sizeof(double), hipMemcpyDeviceToHost, s));
    if (A.tri_used) IRH_CHECK(hipMemcpyAsync(A.tri_used, dused.p, um * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    return IROTAVG_OK;
}

}  // namespace irh
