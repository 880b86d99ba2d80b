// cemp4.hip -- a corruption estimate for the edges listed by cycle-edge message passing over their quadrilaterals
// (irotavg_cycle_cemp4, irotavg_cycle_cemp4_dev; docs/cycle_check.md, "Corruption estimates over four-cycles"), on one
// stream:
//   1. emit, sort, AoS image, edge ids, row bounds   those of the four-cycle test (cyc_prep_alloc / cyc_prep_run:
//                            cycles.hip; k_cyc_edge_ids, k_cyc_rows behind cyc4_edge_ids / cyc4_rows: cycles4.hip);
//   2. k_cemp4_walk<COUNT>   the geometry of k_cyc_quads (one wave per listed position, the longer row staged in the wave's
//                            LDS slab or searched in place, sub-groups of S lanes per entry of the walked row, the partial
//                            product in registers across a row), with a sink that counts the finite quadrilaterals: a
//                            64-bit count per listed position, and per workgroup the sum of the counts and the positions
//                            without one;
//   3. rocprim::exclusive_scan of the counts: the 64-bit segment offsets; k_cyc_summary (cyc_finish) adds the workgroups'
//                            sums. The total, the untested positions and the error word come back in ONE host wait: the
//                            bad id and the cap on the records are decided there, before any output is touched, and only
//                            then is the table sized and taken from the pool;
//   4. k_cemp4_walk<FILL>    the same enumeration in lockstep: an outer round gives every sub-group one entry of the walked
//                            row, an inner round gives every lane one entry of that entry's row, as many inner rounds as
//                            the longest of the rows needs (a wave-wide maximum by shuffles, so every shuffle below is
//                            whole). Per inner round the lanes' hit counts go through a wave-wide prefix, and every lane
//                            stores its 32-byte records at segment start + records of the rounds done + records of the
//                            lower lanes (cemp4_slot). The lanes' sums of d in slot order and the shuffle tree give S^0,
//                            quad_used is stored;
//   5. k_cemp4_iter          the hot path, one launch per iteration: one group of G lanes per listed position streams the
//                            segment with 16-byte loads, coalesced across the group, gathers the three estimates of every
//                            record from the plane of the last iteration, forms the shift (the smallest sum), then the two
//                            weighted sums. A lane keeps the first kHold rounds of its segment in registers between the
//                            two steps; a longer segment is walked a second time from there on. Two planes of m doubles,
//                            both copies of s_in, ping-pong; the last iteration stores into the caller's s4 by position.
//                            The in-order stream is the only barrier between iterations.
// No atomics, no flag between workgroups, no persistent or cooperative launch; every loop is bounded by a row or segment
// length or by 32 rounds of a search. Memory: the four-cycle test's O(m), 16 bytes per listed position for counts and
// offsets, two planes of m doubles, and 32 bytes per used quadrilateral of the listed positions.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "graph.hpp"
#include "kernels.hpp"  // tile_range
#include "cemp4.hpp"
#include "cycload.hpp"

#ifndef IRH_CEMP4_SUB
#define IRH_CEMP4_SUB 8  // lanes of a sub-group of the walk: the four-cycle test's default; not an interface
#endif
#ifndef IRH_CEMP4_GROUP
#define IRH_CEMP4_GROUP 8  // lanes per listed position in k_cemp4_iter: most segments hold a few records; not an interface
#endif

namespace irh {
namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / CYC4_WAVE;  // listed positions of one pass of the walk
constexpr int kS = IRH_CEMP4_SUB;
constexpr int kG = IRH_CEMP4_GROUP;
constexpr int kMaxGrid = 4096;  // a multiple of 8: tile_range deals adjacent chunks to the workgroups of one XCD
constexpr int kPasses = 4;
constexpr int kHold = 4;  // rounds of a segment a lane of k_cemp4_iter keeps in registers: 4 G records per position
enum { CEMP4_COUNT = 0, CEMP4_FILL = 1 };

inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }
inline long long grid_for(long long ne, int per_pass) {
    long long nwg = std::max<long long>(1, (ne + (long long)per_pass * kPasses - 1) / ((long long)per_pass * kPasses));
    if (nwg > 8) nwg = std::min<long long>(kMaxGrid, (nwg + 7) / 8 * 8);
    return nwg;
}

// stores of this wave to its slab before the reads that follow, reads before the stores that follow
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// FILL for one listed position, every lane of the wave in step (x0, x1 and the row y are uniform in the wave): the
// records of the segment [seg, seg + count) and the lane's sum of d in slot order
template <int S, class Row>
__device__ __forceinline__ double cemp4_fill(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                             const CycSpan *__restrict__ rows, long long x0, long long x1, int lane, uint32_t a,
                                             uint32_t b, bool x_is_b, const Row &y, const CycQ q0, const CycDevLoad &load,
                                             Cemp4Rec *__restrict__ table, long long seg, long long count) {
    constexpr int kSubs = CYC4_WAVE / S;
    const int sub = lane / S, sl = lane % S;
    const Cemp4Rec *const end = table + seg + count;
    double lsum = 0.0;
    long long done = 0;
    for (long long outer = x0; outer < x1; outer += kSubs) {
        const long long i = outer + sub;
        uint32_t kx = 0;
        CycQ qx{0.0, 0.0, 0.0, 0.0};
        CycSpan r{0, 0};
        if (i < x1 && cyc4_walked(keys, vals, i, a, b, x_is_b, q0, load, kx, qx)) r = rows[i];
        int longest = r.end - r.beg;
#pragma unroll
        for (int o = CYC4_WAVE / 2; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o, CYC4_WAVE));
        for (int inner = 0; inner < longest; inner += S) {  // (uniform in the wave: the shuffles below are whole)
            const long long j = (long long)r.beg + inner + sl;
            Cemp4Hits h{0, Cemp4Rec{0.0, 0u, 0u, 0u}};
            if (j < r.end) cyc4_entry(keys, vals, j, a, b, x_is_b, y, q0, kx, qx, load, h);
            int upto = h.n;  // the hits of this lane and the lower ones
#pragma unroll
            for (int o = 1; o < CYC4_WAVE; o <<= 1) {
                const int v = __shfl_up(upto, o, CYC4_WAVE);
                if (lane >= o) upto += v;
            }
            Cemp4Rec *const at = table + cemp4_slot(seg, done, upto - h.n);
            if (h.n == 1) {
                if (at < end) *at = h.first;
                lsum += h.first.d;
            } else if (h.n > 1) {
                Cemp4Store w{at, end, lsum};
                cyc4_entry(keys, vals, j, a, b, x_is_b, y, q0, kx, qx, load, w);
                lsum = w.sum;
            }
            done += __shfl(upto, CYC4_WAVE - 1, CYC4_WAVE);
        }
    }
    return lsum;
}

// COUNT: cnt is written, parts get the workgroup's sums (records, -, -, positions without one; the layout of
// k_cyc_summary). FILL: cnt and off are read; the table, the start values (s0_edge: by edge id, the plane of the first
// iteration; s0_pos: by position, the caller's s4 when there is no iteration) and quad_used (each may be nullptr) are
// written.
template <int MODE, int S>
__global__ __launch_bounds__(kT) void k_cemp4_walk(int ne, const int32_t *__restrict__ edges, long long n2,
                                                   const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                   const CycSpan *__restrict__ rows, const int2 *__restrict__ I,
                                                   const double2 *__restrict__ qq, const long long *__restrict__ err,
                                                   long long *__restrict__ cnt, const long long *__restrict__ off,
                                                   Cemp4Rec *__restrict__ table, double *__restrict__ s0_edge,
                                                   double *__restrict__ s0_pos, int32_t *__restrict__ quad_used,
                                                   long long *__restrict__ parts) {
    static_assert(S == 8 || S == 16 || S == 32 || S == 64, "a sub-group lies within one wave");
    constexpr int kSubs = CYC4_WAVE / S;
    __shared__ uint32_t slab[kWaves][2 * CYC4_STAGE];  // (neighbour, value) pairs: 8 KB per wave
    __shared__ long long red[kWaves][2];
    if (*err != 0) return;  // (uniform: a bad id; nothing is indexed with it and nothing is written)
    int e0, e1;
    tile_range(ne, e0, e1);
    const int wave = threadIdx.x / CYC4_WAVE, lane = threadIdx.x % CYC4_WAVE;
    const CycDevLoad load{qq};
    uint32_t *const mine = slab[wave];
    long long sum[2] = {0, 0};  // records, positions without one (lane 0 of a wave alone adds)
    for (long long base = e0; base < e1; base += kWaves) {
        const long long t = base + wave;  // (uniform in the wave)
        const bool valid = t < e1;
        const int k = !valid ? 0 : edges ? edges[t] : (int)t;
        const int2 e = valid ? I[k] : make_int2(0, 0);
        const bool skip = !valid || e.x == e.y;
        // lanes 0..3 look up one row boundary each: the start of row a, its end, the start of row b, its end
        long long r = 0;
        if (!skip && lane < 4) r = cyc_lower_bound(keys, 0, n2, cyc_key((uint32_t)((lane & 2) ? e.y : e.x) + (uint32_t)(lane & 1), 0u));
        const long long a0 = __shfl(r, 0, CYC4_WAVE), a1 = __shfl(r, 1, CYC4_WAVE), b0 = __shfl(r, 2, CYC4_WAVE), b1 = __shfl(r, 3, CYC4_WAVE);
        const long long seg = MODE == CEMP4_FILL && valid ? off[t] : 0, count = MODE == CEMP4_FILL && valid ? cnt[t] : 0;
        Cemp4Count hits{0};  // COUNT: the lane's used quadrilaterals
        double lsum = 0.0;   // FILL: the lane's sum of d, in slot order
        if (!skip) {
            const bool x_is_b = b1 - b0 <= a1 - a0;  // the shorter row is walked, the longer one staged and searched
            const long long x0 = x_is_b ? b0 : a0, x1 = x_is_b ? b1 : a1, y0 = x_is_b ? a0 : b0, y1 = x_is_b ? a1 : b1;
            const int ylen = (int)(y1 - y0);
            const CycQ q0 = load((uint32_t)k);
            if (ylen <= CYC4_STAGE) {
                for (int p = lane; p < ylen; p += CYC4_WAVE) {
                    mine[2 * p] = cyc_key_to(keys[y0 + p]);
                    mine[2 * p + 1] = vals[y0 + p];
                }
                wave_fence();
                const CycRowStaged y{mine, ylen};
                if (MODE == CEMP4_COUNT)
                    cyc4_lane(keys, vals, rows, x0, x1, lane / S, kSubs, lane % S, S, (uint32_t)e.x, (uint32_t)e.y, x_is_b, y, q0, load, hits);
                else
                    lsum = cemp4_fill<S>(keys, vals, rows, x0, x1, lane, (uint32_t)e.x, (uint32_t)e.y, x_is_b, y, q0, load, table, seg, count);
                wave_fence();  // (the next position's stores come behind every lane's reads)
            } else {  // a row too long for the slab: the sorted keys themselves are searched
                const CycRowGlobal y{keys, vals, y0, ylen};
                if (MODE == CEMP4_COUNT)
                    cyc4_lane(keys, vals, rows, x0, x1, lane / S, kSubs, lane % S, S, (uint32_t)e.x, (uint32_t)e.y, x_is_b, y, q0, load, hits);
                else
                    lsum = cemp4_fill<S>(keys, vals, rows, x0, x1, lane, (uint32_t)e.x, (uint32_t)e.y, x_is_b, y, q0, load, table, seg, count);
            }
        }
        if (MODE == CEMP4_COUNT) {
            long long n = hits.n;
#pragma unroll
            for (int o = CYC4_WAVE / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, CYC4_WAVE);
            if (valid && lane == 0) {
                cnt[t] = n;
                sum[0] += n;
                sum[1] += n == 0;
            }
        } else {
#pragma unroll
            for (int o = CYC4_WAVE / 2; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, CYC4_WAVE);
            if (valid && lane == 0) {
                const double s0 = cemp_mean(lsum, count);
                if (s0_edge) s0_edge[k] = s0;
                if (s0_pos) s0_pos[t] = s0;
                if (quad_used) quad_used[t] = cyc_stored_count(count);
            }
        }
    }
    if (MODE == CEMP4_COUNT) {
        if (lane == 0) red[wave][0] = sum[0], red[wave][1] = sum[1];
        __syncthreads();
        if (threadIdx.x < 4) {
            long long s = 0;
            if (threadIdx.x == 0 || threadIdx.x == 3)
                for (int w = 0; w < kWaves; w++) s += red[w][threadIdx.x == 0 ? 0 : 1];
            parts[4 * (size_t)blockIdx.x + threadIdx.x] = s;
        }
    }
}

// quad_used alone was asked for: no table, no iteration
__global__ __launch_bounds__(kT) void k_cemp4_used(long long ne, const long long *__restrict__ cnt, int32_t *__restrict__ quad_used) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (t < ne) quad_used[t] = cyc_stored_count(cnt[t]);
}

// out_edge: the plane of the next iteration, written at the edge id; out_pos: the caller's s4, written at the position
// (the last iteration). One of the two is nullptr.
template <int G>
__global__ __launch_bounds__(kT) void k_cemp4_iter(int ne, const int32_t *__restrict__ edges, const long long *__restrict__ off,
                                                   const long long *__restrict__ cnt, const Cemp4Rec *__restrict__ table,
                                                   const double *__restrict__ s_in, double beta, double *__restrict__ out_edge,
                                                   double *__restrict__ out_pos) {
    constexpr int kPos = kT / G;
    int e0, e1;
    tile_range(ne, e0, e1);
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    for (int base = e0; base < e1; base += kPos) {
        const int t = base + grp;
        const bool valid = t < e1;
        const long long beg = (valid ? off[t] : 0) + lane, end = valid ? off[t] + cnt[t] : 0;
        // the shift: the smallest e of the segment. The first kHold rounds stay in registers for the sums.
        double eh[kHold], dh[kHold], mu = std::numeric_limits<double>::infinity();
#pragma unroll
        for (int j = 0; j < kHold; j++) {
            eh[j] = dh[j] = 0.0;
            if (beg + j * G < end) {
                const Cemp4Rec rec = table[beg + j * G];
                eh[j] = cemp4_e(s_in[rec.k1], s_in[rec.k2], s_in[rec.k3]);
                dh[j] = rec.d;
                cemp_min(mu, eh[j]);
            }
        }
        for (long long r = beg + kHold * G; r < end; r += G) {
            const Cemp4Rec rec = table[r];
            cemp_min(mu, cemp4_e(s_in[rec.k1], s_in[rec.k2], s_in[rec.k3]));
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) cemp_min(mu, __shfl_xor(mu, o, G));
        CempSum a{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < kHold; j++)
            if (beg + j * G < end) cemp_term(a, dh[j], eh[j], beta, mu);
        for (long long r = beg + kHold * G; r < end; r += G) {
            const Cemp4Rec rec = table[r];
            cemp_term(a, rec.d, cemp4_e(s_in[rec.k1], s_in[rec.k2], s_in[rec.k3]), beta, mu);
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            a.num += __shfl_xor(a.num, o, G);
            a.den += __shfl_xor(a.den, o, G);
        }
        if (valid && lane == 0) {
            const double s = cemp_quotient(a);
            if (out_pos)
                out_pos[t] = s;
            else
                out_edge[edges ? edges[t] : t] = s;
        }
    }
}

}  // namespace

int cycle_cemp4_dev(int64_t m, int64_t n_total, const Cemp4Arrays &A, int64_t ne, int iters, const double *beta,
                    int64_t max_records, int64_t *summary, hipStream_t stream) {
    const long long n2 = 2 * (long long)m;
    // without an edge listed, and with every output NULL, the call is the id check
    const bool walk = ne > 0 && (A.s4 || A.quad_used || summary);
    const long long nwg = grid_for(ne, kWaves), nwg_iter = grid_for(ne, kT / kG);
    const int2 *I2 = reinterpret_cast<const int2 *>(A.I);
    // every temporary but the table first (the pool): its size is known only after the count
    CycPrep P;
    DevBuf<CycSpan> rows;
    DevBuf<long long> parts, cnt, off;
    DevBuf<char> scan_tmp;
    DevBuf<double> plane[2];
    DevBuf<Cemp4Rec> table;
    size_t scan_bytes = 0;
    cyc_prep_alloc(P, m, n_total, A.QQ, A.qq_rs, A.qq_cs, walk, stream);
    if (walk) {
        rows.alloc((size_t)n2);
        parts.alloc(4 * (size_t)nwg);
        cnt.alloc((size_t)ne);
        off.alloc((size_t)ne);
        IRH_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, cnt.p, off.p, 0LL, (size_t)ne, rocprim::plus<long long>(), stream));
        scan_tmp.alloc(std::max<size_t>(scan_bytes, 1));
        for (int p = 0; A.s4 && p < std::min(iters, 2); p++) plane[p].alloc((size_t)m);
    }
    cyc_prep_run(P, m, n_total, A.I, A.QQ, A.qq_rs, A.qq_cs, stream);
    if (A.edges && ne > 0) {
        cyc4_edge_ids(ne, m, A.edges, P.head.p, stream);
    }
    if (walk) {
        cyc4_rows(n2, P.kout.p, P.head.p, rows.p, stream);
        hipLaunchKernelGGL((k_cemp4_walk<CEMP4_COUNT, kS>), dim3((unsigned)nwg), dim3(kT), 0, stream, (int)ne, A.edges, n2, P.kout.p,
                           P.vout.p, rows.p, I2, P.qq, P.head.p, cnt.p, nullptr, nullptr, nullptr, nullptr, nullptr, parts.p);
        IRH_CHECK(hipGetLastError());
        IRH_CHECK(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, cnt.p, off.p, 0LL, (size_t)ne, rocprim::plus<long long>(), stream));
    }
    int64_t sum[4] = {0, 0, 0, 0};
    if (const int rc = cyc_finish(P, walk ? (int)nwg : 0, parts.p, sum, stream); rc != IROTAVG_OK) return rc;
    const int64_t records = sum[0];
    if (summary) summary[0] = records, summary[1] = sum[3];
    if (!walk) return IROTAVG_OK;
    if (max_records > 0 && records > max_records) return IROTAVG_ERR_NOMEM;
    if (A.s4) {
        try {
            table.alloc((size_t)records);
        } catch (const HipError &) {
            (void)hipGetLastError();
            return IROTAVG_ERR_NOMEM;  // (nothing but summary has been written)
        }
        // both planes start as s_in: an entry that is not listed is never written (all are listed without a list)
        for (int p = 0; A.edges && p < std::min(iters, 2); p++)
            IRH_CHECK(hipMemcpyAsync(plane[p].p, A.s_in, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL((k_cemp4_walk<CEMP4_FILL, kS>), dim3((unsigned)nwg), dim3(kT), 0, stream, (int)ne, A.edges, n2, P.kout.p,
                           P.vout.p, rows.p, I2, P.qq, P.head.p, cnt.p, off.p, table.p, iters == 0 ? nullptr : plane[0].p,
                           iters == 0 ? A.s4 : nullptr, A.quad_used, nullptr);
        IRH_CHECK(hipGetLastError());
        for (int t = 0; t < iters; t++) {
            const bool last = t == iters - 1;
            hipLaunchKernelGGL((k_cemp4_iter<kG>), dim3((unsigned)nwg_iter), dim3(kT), 0, stream, (int)ne, A.edges, off.p, cnt.p,
                               table.p, plane[t & 1].p, beta[t], last ? nullptr : plane[(t + 1) & 1].p, last ? A.s4 : nullptr);
            IRH_CHECK(hipGetLastError());
        }
    } else if (A.quad_used) {
        hipLaunchKernelGGL(k_cemp4_used, dim3(grid_of(ne)), dim3(kT), 0, stream, (long long)ne, cnt.p, A.quad_used);
        IRH_CHECK(hipGetLastError());
    }
    IRH_CHECK(hipStreamSynchronize(stream));  // (the temporaries go back to the pool idle)
    return IROTAVG_OK;
}

int cycle_cemp4_host(int64_t m, int64_t n_total, const Cemp4Arrays &A, int64_t ne, int iters, const double *beta,
                     int64_t max_records, int64_t *summary) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m, un = (size_t)ne;
    DevBuf<int32_t> dI, dedges, dused;
    DevBuf<double> dqq, dsin, ds4;
    dI.alloc(2 * um);
    dqq.alloc(4 * um);  // four planes of m
    if (A.edges) dsin.alloc(um);
    if (A.edges && un) dedges.alloc(un);
    if (A.s4 && un) ds4.alloc(un);
    if (A.quad_used && un) dused.alloc(un);
    IRH_CHECK(hipMemcpyAsync(dI.p, A.I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    for (int c = 0; c < 4; c++)
        IRH_CHECK(hipMemcpyAsync(dqq.p + c * um, A.QQ + c * A.qq_cs, um * sizeof(double), hipMemcpyHostToDevice, s));
    if (dsin.p) IRH_CHECK(hipMemcpyAsync(dsin.p, A.s_in, um * sizeof(double), hipMemcpyHostToDevice, s));
    if (dedges.p) IRH_CHECK(hipMemcpyAsync(dedges.p, A.edges, un * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const Cemp4Arrays D{dI.p, dqq.p, 1, (long long)m, dsin.p, dedges.p, ds4.p, dused.p};
    const int rc = cycle_cemp4_dev(m, n_total, D, ne, iters, beta, max_records, summary, s);
    if (rc != IROTAVG_OK) return rc;
    if (ds4.p) IRH_CHECK(hipMemcpyAsync(A.s4, ds4.p, un * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dused.p) IRH_CHECK(hipMemcpyAsync(A.quad_used, dused.p, un * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    return IROTAVG_OK;
}

}  // namespace irh
