// cycles4.hip -- the four-cycle test of the edges listed (irotavg_cycle_check4, irotavg_cycle_check4_dev;
// docs/cycle_check.md, "Four-cycles"), on one stream:
//   1. emit, sort, AoS image   those of the triangle test (cycles.hip: cyc_prep_alloc / cyc_prep_run);
//   2. k_cyc_edge_ids   range-checks the edge ids of the subset into the same error word (every writer stores 1);
//   3. k_cyc_rows       one thread per sorted half-edge: the bounds of the row of its TARGET view, two searches, 8 bytes.
//                       A walk that comes by half-edge x -> c finds row c there: once per half-edge, not once per use;
//   4. k_cyc_quads      one wave per tested edge: the longer of its two rows staged in the wave's own LDS slab, the
//                       shorter one dealt to sub-groups of S lanes, each of which walks the row of its entry S entries at a
//                       time and looks every neighbour up in the slab; sums per lane, shuffles, lane 0 stores. It returns
//                       at once when the error word is set, so nothing is indexed with a bad id and no byte is written;
//   5. k_cyc_summary    the triangle test's (cyc_finish).
// No atomics, no flag between workgroups, no loop that is not bounded by a row length or 32 rounds of a search. Waves do
// not share LDS: inside the edge loop a wave-level fence orders a slab's stores before its reads. Memory beyond the
// triangle test's: 8 bytes per sorted half-edge.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "graph.hpp"
#include "kernels.hpp"  // tile_range
#include "cycles4.hpp"
#include "cycload.hpp"

namespace irh {
namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / CYC4_WAVE;  // tested edges of one pass
constexpr int kQuadDefaultGroup = 8;    // the fastest of 8, 16, 32, 64 on the untested subset (docs/cycle_check.md)
constexpr int kQuadMaxGrid = 4096;      // a multiple of 8: tile_range deals adjacent chunks to the workgroups of one XCD
constexpr int kQuadPasses = 4;

inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

__global__ __launch_bounds__(kT) void k_cyc_edge_ids(long long ne, long long m, const int32_t *__restrict__ edges,
                                                     long long *__restrict__ err) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (t >= ne) return;
    const int32_t k = edges[t];
    if (k < 0 || (long long)k >= m) *err = 1;
}

__global__ __launch_bounds__(kT) void k_cyc_rows(long long n2, const uint64_t *__restrict__ keys, const long long *__restrict__ err,
                                                 CycSpan *__restrict__ rows) {
    if (*err != 0) return;
    const long long i = (long long)blockIdx.x * kT + threadIdx.x;
    if (i < n2) rows[i] = cyc_target_row(keys, n2, i);
}

// stores of this wave to its slab before the reads that follow, reads before the stores that follow
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int S>
__global__ __launch_bounds__(kT) void k_cyc_quads(int ne, const int32_t *__restrict__ edges, long long n2,
                                                  const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                  const CycSpan *__restrict__ rows, const int2 *__restrict__ I,
                                                  const double2 *__restrict__ qq, double threshold,
                                                  const long long *__restrict__ err, int32_t *__restrict__ quad_count,
                                                  int32_t *__restrict__ quad_ok, double *__restrict__ quad_min,
                                                  long long *__restrict__ parts) {
    static_assert(S == 8 || S == 16 || S == 32 || S == 64, "a sub-group lies within one wave");
    constexpr int kSubs = CYC4_WAVE / S;
    __shared__ uint32_t slab[kWaves][2 * CYC4_STAGE];  // (neighbour, value) pairs: 8 KB per wave
    __shared__ long long red[kWaves][4];
    if (*err != 0) return;  // (uniform: a bad id; nothing is indexed with it and nothing is written)
    int e0, e1;
    tile_range(ne, e0, e1);
    const int wave = threadIdx.x / CYC4_WAVE, lane = threadIdx.x % CYC4_WAVE;
    const CycDevLoad load{qq};
    uint32_t *const mine = slab[wave];
    long long sum[4] = {0, 0, 0, 0};  // quadrilaterals, supported, contradicted, untested (lane 0 of a wave alone adds)
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
        CycAcc acc = cyc_acc_zero();
        Cyc4Sums sums{acc, threshold};
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
                cyc4_lane(keys, vals, rows, x0, x1, lane / S, kSubs, lane % S, S, (uint32_t)e.x, (uint32_t)e.y, x_is_b, y, q0,
                          load, sums);
                wave_fence();  // (the next edge's stores come behind every lane's reads)
            } else {  // a row too long for the slab: the sorted keys themselves are searched
                const CycRowGlobal y{keys, vals, y0, ylen};
                cyc4_lane(keys, vals, rows, x0, x1, lane / S, kSubs, lane % S, S, (uint32_t)e.x, (uint32_t)e.y, x_is_b, y, q0,
                          load, sums);
            }
        }
#pragma unroll
        for (int o = CYC4_WAVE / 2; o > 0; o >>= 1)
            cyc_acc_merge(acc, __shfl_xor(acc.count, o, CYC4_WAVE), __shfl_xor(acc.ok, o, CYC4_WAVE), __shfl_xor(acc.mn, o, CYC4_WAVE));
        if (valid && lane == 0) {
            const int32_t c = cyc_stored_count(acc.count), o = cyc_stored_count(acc.ok);
            if (quad_count) quad_count[t] = c;
            if (quad_ok) quad_ok[t] = o;
            if (quad_min) quad_min[t] = acc.mn;
            sum[0] += c;
            sum[o >= 1 ? 1 : c >= 1 ? 2 : 3]++;
        }
    }
    if (lane == 0)
        for (int j = 0; j < 4; j++) red[wave][j] = sum[j];
    __syncthreads();
    if (threadIdx.x < 4) {
        long long s = 0;
        for (int w = 0; w < kWaves; w++) s += red[w][threadIdx.x];
        parts[4 * (size_t)blockIdx.x + threadIdx.x] = s;
    }
}

std::atomic<int> g_group{kQuadDefaultGroup};

template <int S>
void launch_quads(int grid, hipStream_t s, int ne, int m, const CycPrep &P, const CycSpan *rows, double threshold,
                  const Cycle4Arrays &A, long long *parts) {
    hipLaunchKernelGGL(k_cyc_quads<S>, dim3((unsigned)grid), dim3(kT), 0, s, ne, A.edges, 2 * (long long)m, P.kout.p, P.vout.p,
                       rows, reinterpret_cast<const int2 *>(A.I), P.qq, threshold, P.head.p, A.quad_count, A.quad_ok, A.quad_min,
                       parts);
}

}  // namespace

void cyc4_edge_ids(long long ne, long long m, const int32_t *edges, long long *err, hipStream_t stream) {
    hipLaunchKernelGGL(k_cyc_edge_ids, dim3(grid_of(ne)), dim3(kT), 0, stream, ne, m, edges, err);
    IRH_CHECK(hipGetLastError());
}

void cyc4_rows(long long n2, const uint64_t *keys, const long long *err, CycSpan *rows, hipStream_t stream) {
    hipLaunchKernelGGL(k_cyc_rows, dim3(grid_of(n2)), dim3(kT), 0, stream, n2, keys, err, rows);
    IRH_CHECK(hipGetLastError());
}

int cycle_check4_group(int lanes) {
    if (lanes == 0) lanes = kQuadDefaultGroup;
    if (lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64) return IROTAVG_ERR_BAD_ARG;
    return g_group.exchange(lanes);
}

int cycle_check4_dev(int64_t m, int64_t n_total, const Cycle4Arrays &A, double threshold, int64_t ne, int64_t *summary,
                     hipStream_t stream) {
    const long long n2 = 2 * (long long)m;
    // without an edge to test, and with every output NULL, the call is the id check
    const bool quads = ne > 0 && (A.quad_count || A.quad_ok || A.quad_min || summary);
    const int S = g_group.load();
    // the workgroups of the quadrilateral kernel: kQuadPasses passes each while the subset is small, then longer chunks
    long long nwg = std::max<long long>(1, (ne + (long long)kWaves * kQuadPasses - 1) / ((long long)kWaves * kQuadPasses));
    if (nwg > 8) nwg = std::min<long long>(kQuadMaxGrid, (nwg + 7) / 8 * 8);
    // every temporary first (the pool): nothing after the first launch can fail for want of memory
    CycPrep P;
    DevBuf<CycSpan> rows;
    DevBuf<long long> parts;
    cyc_prep_alloc(P, m, n_total, A.QQ, A.qq_rs, A.qq_cs, quads, stream);
    if (quads) {
        rows.alloc((size_t)n2);
        parts.alloc(4 * (size_t)nwg);
    }
    cyc_prep_run(P, m, n_total, A.I, A.QQ, A.qq_rs, A.qq_cs, stream);
    if (A.edges && ne > 0) {
        cyc4_edge_ids(ne, m, A.edges, P.head.p, stream);
    }
    if (quads) {
        cyc4_rows(n2, P.kout.p, P.head.p, rows.p, stream);
        switch (S) {
        case 8: launch_quads<8>((int)nwg, stream, (int)ne, (int)m, P, rows.p, threshold, A, parts.p); break;
        case 32: launch_quads<32>((int)nwg, stream, (int)ne, (int)m, P, rows.p, threshold, A, parts.p); break;
        case 64: launch_quads<64>((int)nwg, stream, (int)ne, (int)m, P, rows.p, threshold, A, parts.p); break;
        default: launch_quads<16>((int)nwg, stream, (int)ne, (int)m, P, rows.p, threshold, A, parts.p);
        }
        IRH_CHECK(hipGetLastError());
    }
    return cyc_finish(P, quads ? (int)nwg : 0, parts.p, summary, stream);
}

int cycle_check4_host(int64_t m, int64_t n_total, const Cycle4Arrays &A, double threshold, int64_t ne, int64_t *summary) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m, un = (size_t)ne;
    DevBuf<int32_t> dI, dedges, dcount, dok;
    DevBuf<double> dqq, dmin;
    dI.alloc(2 * um);
    dqq.alloc(4 * um);  // four planes of m
    if (A.edges && un) dedges.alloc(un);
    if (A.quad_count && un) dcount.alloc(un);
    if (A.quad_ok && un) dok.alloc(un);
    if (A.quad_min && un) dmin.alloc(un);
    IRH_CHECK(hipMemcpyAsync(dI.p, A.I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    for (int c = 0; c < 4; c++)
        IRH_CHECK(hipMemcpyAsync(dqq.p + c * um, A.QQ + c * A.qq_cs, um * sizeof(double), hipMemcpyHostToDevice, s));
    if (dedges.p) IRH_CHECK(hipMemcpyAsync(dedges.p, A.edges, un * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const Cycle4Arrays D{dI.p, dqq.p, 1, (long long)m, dedges.p, dcount.p, dok.p, dmin.p};
    int64_t sum[4] = {0, 0, 0, 0};
    const int rc = cycle_check4_dev(m, n_total, D, threshold, ne, summary ? sum : nullptr, s);
    if (rc != IROTAVG_OK) return rc;
    if (dcount.p) IRH_CHECK(hipMemcpyAsync(A.quad_count, dcount.p, un * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (dok.p) IRH_CHECK(hipMemcpyAsync(A.quad_ok, dok.p, un * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (dmin.p) IRH_CHECK(hipMemcpyAsync(A.quad_min, dmin.p, un * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    if (summary)
        for (int j = 0; j < 4; j++) summary[j] = sum[j];
    return IROTAVG_OK;
}

}  // namespace irh
