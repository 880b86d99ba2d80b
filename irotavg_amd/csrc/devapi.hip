// devapi.hip -- the `_dev` entry points of include/irotavg_hip.h (docs/device_api.md): a caller whose arrays live in HBM
// already (torch tensors, another library's buffers) builds, fills, solves and queries a handle without a host round trip.
//
// Nothing here computes: the entry points put a copy in front of and behind the kernels the host-pointer API runs, so
// every result is bitwise what the host call gives. What is new is
//  * the ordering contract: on entry the handle's stream waits for an event recorded on the caller's stream, before
//    returning the caller's stream waits for an event recorded on the handle's stream (order_streams);
//  * strided matrices (ptr, row_stride, col_stride) in elements, moved by kernels with three paths each:
//      AoS     rs == 4, cs == 1, 16-byte aligned: 16-byte accesses on both sides;
//      planes  rs == 1, cs even, 16-byte aligned: 16-byte accesses on both sides, two rows per thread;
//      generic anything else that does not alias: 8-byte accesses (coalesced on the handle's side);
//  * argument checks that keep a wrong pointer away from every kernel: strides that alias, and the lowest and highest
//    element of every array asked of the runtime (device memory of the handle's device and both in one allocation, so
//    that everything between them is mapped too, or BAD_ARG).
// The kernels stream: no reuse, one or two rows per thread, 256-thread workgroups, a grid that covers the array once.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <new>

#include "graph.hpp"
#include "kernels.hpp"
#include "marginals.hpp"
#include "winbatch.hpp"  // strides_ok, matrix_span, rows16, the plan of irotavg_window_solve_batch_dev

namespace irh {
namespace {

constexpr int kT = 256;
inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

enum Path { kAos = 0, kPlanes = 1, kGeneric = 2 };

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline Path path_of(const double *p, long long rs, long long cs, bool allow_aos) {
    if (allow_aos && rows16(reinterpret_cast<uintptr_t>(p), rs, cs)) return kAos;
    if (rs == 1 && (cs & 1) == 0 && aligned16(p)) return kPlanes;
    return kGeneric;
}

// one value between the caller's side and the handle's side; kOut: the handle's value goes out
template <bool kOut, typename T>
__device__ __forceinline__ void mv(T *user, T *own) {
    if (kOut) *user = *own;
    else *own = *user;
}

// ---- relative rotations: strided m x 4 -> the four planes of mpad doubles, [m, mpad) zero ------------------------------
// kAos / kPlanes: two consecutive edges per thread (mpad is a multiple of 64), kGeneric: one
template <int kPath>
__global__ __launch_bounds__(kT) void k_ingest_qq(long long m, long long mpad, const double *__restrict__ src, long long rs,
                                                  long long cs, double *__restrict__ planes) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (kPath == kGeneric) {
        if (t >= mpad) return;
#pragma unroll
        for (int c = 0; c < 4; c++) planes[c * mpad + t] = t < m ? src[t * rs + c * cs] : 0.0;
        return;
    }
    const long long k = 2 * t;
    if (k >= mpad) return;
    double2 v[4];  // per plane: the values of edges k, k + 1
    if (kPath == kAos) {
        const double2 *s2 = reinterpret_cast<const double2 *>(src);
        const double2 z = make_double2(0.0, 0.0);
        const double2 a0 = k < m ? s2[2 * k] : z, a1 = k < m ? s2[2 * k + 1] : z;
        const double2 b0 = k + 1 < m ? s2[2 * k + 2] : z, b1 = k + 1 < m ? s2[2 * k + 3] : z;
        v[0] = make_double2(a0.x, b0.x);
        v[1] = make_double2(a0.y, b0.y);
        v[2] = make_double2(a1.x, b1.x);
        v[3] = make_double2(a1.y, b1.y);
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const double *col = src + c * cs;
            if (k + 1 < m) v[c] = *reinterpret_cast<const double2 *>(col + k);
            else v[c] = make_double2(k < m ? col[k] : 0.0, 0.0);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) reinterpret_cast<double2 *>(planes + c * mpad)[t] = v[c];
}

// ---- rotations: the handle's double4 rows <-> strided n x 4 ------------------------------------------------------------
template <bool kOut, int kPath>
__global__ __launch_bounds__(kT) void k_rotations(long long n, double4 *__restrict__ Q, double *__restrict__ u, long long rs,
                                                  long long cs) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (kPath == kAos) {  // a row each: two 16-byte accesses on either side
        if (t >= n) return;
        double2 *q2 = reinterpret_cast<double2 *>(Q) + 2 * t, *u2 = reinterpret_cast<double2 *>(u) + 2 * t;
        mv<kOut>(u2, q2);
        mv<kOut>(u2 + 1, q2 + 1);
    } else if (kPath == kPlanes) {  // two rows each: 16-byte accesses on the caller's columns
        const long long k = 2 * t;
        if (k >= n) return;
        double *q = reinterpret_cast<double *>(Q + k);
        if (k + 1 < n) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                double2 *uc = reinterpret_cast<double2 *>(u + c * cs + k);
                if (kOut) *uc = make_double2(q[c], q[4 + c]);
                else {
                    const double2 w = *uc;
                    q[c] = w.x;
                    q[4 + c] = w.y;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) mv<kOut>(u + c * cs + k, q + c);
        }
    } else {
        if (t >= n) return;
        double *q = reinterpret_cast<double *>(Q + t);
#pragma unroll
        for (int c = 0; c < 4; c++) mv<kOut>(u + t * rs + c * cs, q + c);
    }
}

// ---- residuals: three planes of mpad doubles -> strided m x 3 (no AoS path: three columns have no 16-byte rows) --------
template <int kPath>
__global__ __launch_bounds__(kT) void k_residuals_out(long long m, long long mpad, const double *__restrict__ planes,
                                                      double *__restrict__ u, long long rs, long long cs) {
    const long long t = (long long)blockIdx.x * kT + threadIdx.x;
    if (kPath == kPlanes) {
        const long long k = 2 * t;
        if (k >= m) return;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (k + 1 < m) *reinterpret_cast<double2 *>(u + c * cs + k) = reinterpret_cast<const double2 *>(planes + c * mpad)[t];
            else u[c * cs + k] = planes[c * mpad + k];
        }
    } else {
        if (t >= m) return;
#pragma unroll
        for (int c = 0; c < 3; c++) u[t * rs + c * cs] = planes[c * mpad + t];
    }
}

// ---- argument checks (before any device work) ----------------------------------------------------------------------------
// (the stride rule itself -- strides_ok -- and the span of a strided matrix are host arithmetic: winbatch.hpp)
bool dev_ptr_ok(const void *p, int device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // an address the runtime does not know: not device memory
        return false;
    }
    return at.type == hipMemoryTypeDevice && at.device == device;
}
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
// The elements *first .. *last are device memory of `device` with no unmapped address between them. Asking the runtime
// about the two ends alone is not enough: an array claimed gigabytes longer than it is can end inside somebody else's
// allocation -- late in a long process much of the address space is somebody's -- and the kernel then faults on the way
// there. So the allocation around the first element must reach past the last, directly or through allocations that
// follow it without a gap (span_covered, winbatch.hpp). In the usual case this is one hipPointerGetAttributes and one
// hipMemGetAddressRange: as many runtime calls as the two ends took. Memory whose allocation the runtime cannot name is
// judged by its two ends, as it always was.
template <typename T>
bool dev_span_ok(const T *first, const T *last, int device) {
    if (!dev_ptr_ok(first, device)) return false;
    bool hop = false;
    const int covered = span_covered(reinterpret_cast<uintptr_t>(first), reinterpret_cast<uintptr_t>(last + 1),
                                     [&](uintptr_t at, uintptr_t &base, size_t &size) {
                                         void *p = reinterpret_cast<void *>(at);
                                         hipDeviceptr_t b = nullptr;
                                         if ((hop && !dev_ptr_ok(p, device)) || hipMemGetAddressRange(&b, &size, p) != hipSuccess) {
                                             (void)hipGetLastError();
                                             return false;
                                         }
                                         hop = true;
                                         base = reinterpret_cast<uintptr_t>(b);
                                         return true;
                                     });
    return covered < 0 ? dev_ptr_ok(last, device) : covered == 1;
}
// the lowest and the highest element of the matrix (negative strides reach below ptr)
bool dev_matrix_ok(const double *p, int64_t rows, int cols, int64_t rs, int64_t cs, int device) {
    if (!aligned8(p)) return false;
    int64_t lo, hi;
    matrix_span(rows, cols, rs, cs, lo, hi);
    return dev_span_ok(p + lo, p + hi, device);
}
bool dev_vector_ok(const double *p, int64_t n, int device) { return dev_matrix_ok(p, n, 1, 1, 1, device); }
// `rows` pairs of ids: the first and the last int32
bool dev_index_ok(const int32_t *p, int64_t rows, int device) { return dev_span_ok(p, p + 2 * rows - 1, device); }

// The checks every batched window call makes of its packed problem arrays (A: WinBatchArrays or WinCovArrays), in the
// order the calls have always had: before any device work alignment and the stride rule (BAD_ARG), then a device at all
// (NO_DEVICE), then the calling thread's current one -> `device`, then the lowest and the highest element of each array
// (BAD_ARG). A call's own host checks go in front of this, its own pointer checks behind it.
template <class Arrays>
int win_arrays_check(const Arrays &A, int64_t sum_m, int64_t sum_n, int &device) {
    if (!aligned8(A.I) || !aligned8(A.QQ) || !aligned8(A.Q) || !aligned8(A.weights) || !strides_ok(sum_m, 4, A.qq_rs, A.qq_cs) ||
        !strides_ok(sum_n, 4, A.q_rs, A.q_cs))
        return IROTAVG_ERR_BAD_ARG;
    if (irotavg_device_count() <= 0) return IROTAVG_ERR_NO_DEVICE;
    IRH_CHECK(hipGetDevice(&device));
    const bool ok = dev_index_ok(A.I, sum_m, device) && dev_matrix_ok(A.QQ, sum_m, 4, A.qq_rs, A.qq_cs, device) &&
                    dev_matrix_ok(A.Q, sum_n, 4, A.q_rs, A.q_cs, device) && (!A.weights || dev_vector_ok(A.weights, sum_m, device));
    return ok ? IROTAVG_OK : IROTAVG_ERR_BAD_ARG;
}

// the ordering contract of a call on an existing handle
struct Ordered {
    Graph &g;
    hipStream_t caller;
    Ordered(Graph &g_, void *stream) : g(g_), caller(static_cast<hipStream_t>(stream)) { order_streams(g, caller, g.stream, true); }
    void done() { order_streams(g, g.stream, caller, false); }
};

template <typename F>
int guarded(F &&body) {  // no exception crosses the C boundary
    try {
        return body();
    } catch (const HipError &) {
        return IROTAVG_ERR_HIP;
    } catch (const std::bad_alloc &) {
        return IROTAVG_ERR_NOMEM;
    } catch (...) {
        return IROTAVG_ERR_HIP;
    }
}

template <bool kOut>
void launch_rotations(Graph &g, double *u, long long rs, long long cs) {
    const long long n = g.n_total;
    switch (path_of(u, rs, cs, true)) {
    case kAos:
        hipLaunchKernelGGL((k_rotations<kOut, kAos>), dim3(grid_of(n)), dim3(kT), 0, g.stream, n, g.Q.p, u, rs, cs);
        break;
    case kPlanes:
        hipLaunchKernelGGL((k_rotations<kOut, kPlanes>), dim3(grid_of((n + 1) / 2)), dim3(kT), 0, g.stream, n, g.Q.p, u, rs, cs);
        break;
    default:
        hipLaunchKernelGGL((k_rotations<kOut, kGeneric>), dim3(grid_of(n)), dim3(kT), 0, g.stream, n, g.Q.p, u, rs, cs);
    }
    IRH_CHECK(hipGetLastError());
}

}  // namespace

void order_streams(Graph &g, hipStream_t from, hipStream_t to, bool in) {
    hipEvent_t &ev = in ? g.ev_in : g.ev_out;
    if (!ev) IRH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    IRH_CHECK(hipEventRecord(ev, from));
    IRH_CHECK(hipStreamWaitEvent(to, ev, 0));
}

void ingest_qq(Graph &g, const double *src, long long rs, long long cs) {
    const long long m = g.m, mpad = g.mpad;
    switch (path_of(src, rs, cs, true)) {
    case kAos:
        hipLaunchKernelGGL(k_ingest_qq<kAos>, dim3(grid_of(mpad / 2)), dim3(kT), 0, g.stream, m, mpad, src, rs, cs, g.qq.p);
        break;
    case kPlanes:
        hipLaunchKernelGGL(k_ingest_qq<kPlanes>, dim3(grid_of(mpad / 2)), dim3(kT), 0, g.stream, m, mpad, src, rs, cs, g.qq.p);
        break;
    default:
        hipLaunchKernelGGL(k_ingest_qq<kGeneric>, dim3(grid_of(mpad)), dim3(kT), 0, g.stream, m, mpad, src, rs, cs, g.qq.p);
    }
    IRH_CHECK(hipGetLastError());
}

}  // namespace irh

using namespace irh;

extern "C" {

int irotavg_graph_create_dev(irotavg_graph **out, int64_t m, int64_t n_total, int f, const int32_t *I_dev,
                             const double *QQ_dev, int64_t qq_rs, int64_t qq_cs, const irotavg_options *opt, void *stream) {
    if (!out) return IROTAVG_ERR_BAD_ARG;
    *out = nullptr;
    if (!I_dev || !QQ_dev || m <= 0 || m > 0x3fffffffLL || n_total <= 0 || f < 0 || n_total - f < 1 ||
        n_total > 0x7fffffffLL || !aligned8(I_dev) || !strides_ok(m, 4, qq_rs, qq_cs))
        return IROTAVG_ERR_BAD_ARG;
    if (irotavg_device_count() <= 0) return IROTAVG_ERR_NO_DEVICE;
    return guarded([&]() -> int {
        int device = opt ? opt->device : -1;
        if (device < 0) IRH_CHECK(hipGetDevice(&device));
        if (!dev_index_ok(I_dev, m, device) || !dev_matrix_ok(QQ_dev, m, 4, qq_rs, qq_cs, device)) return IROTAVG_ERR_BAD_ARG;
        DevEdgeSrc src;
        src.I = reinterpret_cast<const int2 *>(I_dev);
        src.qq = QQ_dev;
        src.qq_rs = qq_rs;
        src.qq_cs = qq_cs;
        src.ordered = true;
        src.caller = static_cast<hipStream_t>(stream);
        // (an edge index out of range is found by the build's first kernel: IROTAVG_ERR_BAD_ARG, the handle destroyed)
        const int rc = graph_create(out, m, n_total, f, nullptr, nullptr, 0, opt, &src, read_switches());
        if (rc == IROTAVG_OK) {
            Graph &g = graph_of(*out);
            order_streams(g, g.stream, src.caller, false);
        }
        return rc;
    });
}

int irotavg_graph_set_rotations_dev(irotavg_graph *h, const double *Q_dev, int64_t rs, int64_t cs, void *stream) {
    if (!h || !Q_dev || !strides_ok(graph_of(h).n_total, 4, rs, cs)) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        if (!dev_matrix_ok(Q_dev, g.n_total, 4, rs, cs, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        launch_rotations<false>(g, const_cast<double *>(Q_dev), rs, cs);
        o.done();
        return IROTAVG_OK;
    });
}

int irotavg_graph_get_rotations_dev(irotavg_graph *h, double *Q_dev, int64_t rs, int64_t cs, void *stream) {
    if (!h || !Q_dev || !strides_ok(graph_of(h).n_total, 4, rs, cs)) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        if (!dev_matrix_ok(Q_dev, g.n_total, 4, rs, cs, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        launch_rotations<true>(g, Q_dev, rs, cs);
        o.done();
        return IROTAVG_OK;
    });
}

int irotavg_graph_set_weights_dev(irotavg_graph *h, const double *w_dev, void *stream) {
    if (!h || !w_dev) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        if (!dev_vector_ok(w_dev, g.m, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        IRH_CHECK(hipMemcpyAsync(g.dw.p, w_dev, sizeof(double) * (size_t)g.m, hipMemcpyDeviceToDevice, g.stream));
        o.done();
        return IROTAVG_OK;
    });
}

int irotavg_graph_get_weights_dev(irotavg_graph *h, double *w_dev, void *stream) {
    if (!h || !w_dev) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        if (!dev_vector_ok(w_dev, g.m, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        IRH_CHECK(hipMemcpyAsync(w_dev, g.dw.p, sizeof(double) * (size_t)g.m, hipMemcpyDeviceToDevice, g.stream));
        o.done();
        return IROTAVG_OK;
    });
}

int irotavg_graph_get_residuals_dev(irotavg_graph *h, double *out_dev, int64_t rs, int64_t cs, void *stream) {
    if (!h || !out_dev || !strides_ok(graph_of(h).m, 3, rs, cs)) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        if (!dev_matrix_ok(out_dev, g.m, 3, rs, cs, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        const long long m = g.m, mpad = g.mpad;
        if (path_of(out_dev, rs, cs, false) == kPlanes)
            hipLaunchKernelGGL(k_residuals_out<kPlanes>, dim3(grid_of((m + 1) / 2)), dim3(kT), 0, g.stream, m, mpad, g.er.p,
                               out_dev, (long long)rs, (long long)cs);
        else
            hipLaunchKernelGGL(k_residuals_out<kGeneric>, dim3(grid_of(m)), dim3(kT), 0, g.stream, m, mpad, g.er.p, out_dev,
                               (long long)rs, (long long)cs);
        IRH_CHECK(hipGetLastError());
        o.done();
        return IROTAVG_OK;
    });
}

int irotavg_graph_rotation_variance_dev(irotavg_graph *h, double *var_dev, double *scale, void *stream) {
    if (!h || !var_dev) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        if (!dev_vector_ok(var_dev, g.n_total, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        const int rc = rotation_variance(g, nullptr, 0, nullptr, nullptr, scale, var_dev);
        o.done();
        return rc;
    });
}

int irotavg_graph_edge_diagnostics_dev(irotavg_graph *h, double *edge_var_dev, double *leverage_dev, double *chi2_dev,
                                       double *scale, void *stream) {
    if (!h || (!edge_var_dev && !leverage_dev && !chi2_dev && !scale)) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        Graph &g = graph_of(h);
        for (double *p : {edge_var_dev, leverage_dev, chi2_dev})
            if (p && !dev_vector_ok(p, g.m, g.device)) return IROTAVG_ERR_BAD_ARG;
        Ordered o(g, stream);
        const int rc = edge_diagnostics(g, edge_var_dev, leverage_dev, chi2_dev, scale, true);
        o.done();
        return rc;
    });
}

// Many small problems on packed device arrays, one workgroup each (docs/window_batch.md). Handle-free: the device is
// the calling thread's current one. The launches go on the caller's stream itself, so there is no event to wait for.
int irotavg_window_solve_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev, int64_t qq_rs,
                                   int64_t qq_cs, double *Q_dev, int64_t q_rs, int64_t q_cs, int cost, double sigma,
                                   int l1_iters, int irls_iters, double change_th, double *weights_dev, int32_t *results,
                                   int kernel, void *stream) {
    if (!I_dev || !QQ_dev || !Q_dev) return IROTAVG_ERR_BAD_ARG;
    if (cost < IROTAVG_L2 || cost > IROTAVG_WELSCH) return IROTAVG_ERR_UNKNOWN_COST;
    return guarded([&]() -> int {
        WinBatchPlan plan;
        if (!winbatch_plan(nb, sizes, kernel, plan)) return IROTAVG_ERR_BAD_ARG;
        const WinBatchArrays A{I_dev, QQ_dev, (long long)qq_rs, (long long)qq_cs, Q_dev, (long long)q_rs, (long long)q_cs,
                               weights_dev};
        int device = 0;
        if (const int rc = win_arrays_check(A, plan.sum_m, plan.sum_n, device); rc != IROTAVG_OK) return rc;
        return window_solve_batch_dev(plan, device, A, cost, sigma, l1_iters, irls_iters, change_th, results,
                                      static_cast<hipStream_t>(stream));
    });
}

// irotavg_init_mst on many small problems on packed device arrays, one workgroup each, one launch
// (docs/window_init_batch.md): the arrays, the plan and the checks of the call above; view 0 must be fixed.
int irotavg_window_init_mst_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev,
                                      int64_t qq_rs, int64_t qq_cs, double *Q_dev, int64_t q_rs, int64_t q_cs,
                                      int32_t *results, void *stream) {
    if (!I_dev || !QQ_dev || !Q_dev) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        WinBatchPlan plan;
        if (!winbatch_plan(nb, sizes, 1, plan)) return IROTAVG_ERR_BAD_ARG;  // kernel 1: one list, in the caller's order
        for (const WinDesc &d : plan.desc)
            if (d.f < 1) return IROTAVG_ERR_BAD_ARG;  // irotavg_init_mst refuses f <= 0
        const WinBatchArrays A{I_dev, QQ_dev, (long long)qq_rs, (long long)qq_cs, Q_dev, (long long)q_rs, (long long)q_cs,
                               nullptr};
        int device = 0;
        if (const int rc = win_arrays_check(A, plan.sum_m, plan.sum_n, device); rc != IROTAVG_OK) return rc;
        return window_init_mst_batch_dev(plan, device, A, results, static_cast<hipStream_t>(stream));
    });
}

// The uncertainty of many small problems on packed device arrays, one workgroup each, one launch
// (docs/window_uncertainty_batch.md). Handle-free and on the caller's stream itself, as irotavg_window_solve_batch_dev.
int irotavg_window_uncertainty_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev,
                                         int64_t qq_rs, int64_t qq_cs, const double *Q_dev, int64_t q_rs, int64_t q_cs,
                                         const double *weights_dev, double sigma, double *var_dev, const int32_t *npairs,
                                         const int32_t *pairs_dev, double *pair_var_dev, double *edge_var_dev,
                                         double *leverage_dev, double *chi2_dev, double *scale, int32_t *results, void *stream) {
    if (!I_dev || !QQ_dev || !Q_dev) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        WinCovPlan plan;
        if (!wincov_plan(nb, sizes, npairs, nullptr, plan)) return IROTAVG_ERR_BAD_ARG;
        if (!wincov_asked(var_dev, plan.sum_p, pairs_dev && pair_var_dev, edge_var_dev, leverage_dev, chi2_dev, scale))
            return IROTAVG_ERR_BAD_ARG;
        double *const per_edge[3] = {edge_var_dev, leverage_dev, chi2_dev};
        for (double *p : per_edge)
            if (!aligned8(p)) return IROTAVG_ERR_BAD_ARG;
        if (!aligned8(var_dev) || (plan.sum_p > 0 && (!aligned8(pairs_dev) || !aligned8(pair_var_dev)))) return IROTAVG_ERR_BAD_ARG;
        const WinCovArrays A{I_dev, QQ_dev, (long long)qq_rs, (long long)qq_cs, Q_dev, (long long)q_rs, (long long)q_cs,
                             weights_dev, var_dev, plan.sum_p > 0 ? pairs_dev : nullptr, plan.sum_p > 0 ? pair_var_dev : nullptr,
                             edge_var_dev, leverage_dev, chi2_dev};
        int device = 0;
        if (const int rc = win_arrays_check(A, plan.sum_m, plan.sum_n, device); rc != IROTAVG_OK) return rc;
        for (double *p : per_edge)
            if (p && !dev_vector_ok(p, plan.sum_m, device)) return IROTAVG_ERR_BAD_ARG;
        if (var_dev && !dev_vector_ok(var_dev, plan.sum_n, device)) return IROTAVG_ERR_BAD_ARG;
        if (plan.sum_p > 0 && (!dev_index_ok(pairs_dev, plan.sum_p, device) || !dev_vector_ok(pair_var_dev, plan.sum_p, device)))
            return IROTAVG_ERR_BAD_ARG;
        return wincov_batch_dev(plan, device, A, sigma, scale, results, static_cast<hipStream_t>(stream));
    });
}

// The closure gate of many small problems on packed device arrays, one workgroup each, one launch
// (docs/window_gate_batch.md): the candidates of k_window_gate_user, everything else as the call above.
int irotavg_window_gate_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev, int64_t qq_rs,
                                  int64_t qq_cs, const double *Q_dev, int64_t q_rs, int64_t q_cs, const double *weights_dev,
                                  double sigma, const int32_t *ncand, const int32_t *cand_I_dev, const double *cand_QQ_dev,
                                  int64_t cq_rs, int64_t cq_cs, double *angle_dev, double *pair_var_dev, double *chi2_dev,
                                  double *scale, int32_t *results, void *stream) {
    if (!I_dev || !QQ_dev || !Q_dev) return IROTAVG_ERR_BAD_ARG;
    return guarded([&]() -> int {
        WinCovPlan plan;
        if (!wincov_plan(nb, sizes, nullptr, ncand, plan)) return IROTAVG_ERR_BAD_ARG;
        const int64_t sum_c = plan.sum_c;
        if (!wingate_asked(sum_c, cand_I_dev && cand_QQ_dev, angle_dev, pair_var_dev, chi2_dev, scale)) return IROTAVG_ERR_BAD_ARG;
        double *const per_cand[3] = {angle_dev, pair_var_dev, chi2_dev};
        if (sum_c > 0) {
            for (double *p : per_cand)
                if (!aligned8(p)) return IROTAVG_ERR_BAD_ARG;
            if (!aligned8(cand_I_dev) || !aligned8(cand_QQ_dev) || !strides_ok(sum_c, 4, cq_rs, cq_cs)) return IROTAVG_ERR_BAD_ARG;
        }
        WinCovArrays A{I_dev, QQ_dev, (long long)qq_rs, (long long)qq_cs, Q_dev, (long long)q_rs, (long long)q_cs, weights_dev,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        int device = 0;
        if (const int rc = win_arrays_check(A, plan.sum_m, plan.sum_n, device); rc != IROTAVG_OK) return rc;
        A.gate = true;
        if (sum_c > 0) {  // (without candidates the kernel is handed no candidate array at all)
            if (!dev_index_ok(cand_I_dev, sum_c, device) || !dev_matrix_ok(cand_QQ_dev, sum_c, 4, cq_rs, cq_cs, device))
                return IROTAVG_ERR_BAD_ARG;
            for (double *p : per_cand)
                if (p && !dev_vector_ok(p, sum_c, device)) return IROTAVG_ERR_BAD_ARG;
            A.cand = cand_I_dev;
            A.cand_QQ = cand_QQ_dev;
            A.cq_rs = (long long)cq_rs;
            A.cq_cs = (long long)cq_cs;
            A.angle = angle_dev;
            A.cand_var = pair_var_dev;
            A.cand_chi2 = chi2_dev;
        }
        return wincov_batch_dev(plan, device, A, sigma, scale, results, static_cast<hipStream_t>(stream));
    });
}

// The triangle test of every edge (docs/cycle_check.md; the kernels: cycles.hip). Handle-free; the device form runs on the
// caller's stream itself, as the batched window calls do.
static bool cycle_sizes_ok(int64_t m, int64_t n_total, double threshold) {
    return m > 0 && m <= 0x3fffffffLL && n_total > 0 && n_total <= 0x7fffffffLL && threshold >= 0.0;  // (NaN: false)
}

int irotavg_cycle_check(int64_t m, int64_t n_total, const int32_t *I, const double *QQ, int64_t ldqq, double threshold,
                        int32_t *tri_count, int32_t *tri_ok, double *tri_min, int64_t summary[4]) {
    if (!I || !QQ || !cycle_sizes_ok(m, n_total, threshold) || ldqq < m) return IROTAVG_ERR_BAD_ARG;
    if (irotavg_device_count() <= 0) return IROTAVG_ERR_NO_DEVICE;
    return guarded([&]() -> int {
        const CycleArrays A{I, QQ, 1, (long long)ldqq, tri_count, tri_ok, tri_min};
        return cycle_check_host(m, n_total, A, threshold, summary);
    });
}

int irotavg_cycle_check_dev(int64_t m, int64_t n_total, const int32_t *I_dev, const double *QQ_dev, int64_t qq_rs,
                            int64_t qq_cs, double threshold, int32_t *tri_count_dev, int32_t *tri_ok_dev,
                            double *tri_min_dev, int64_t summary[4], void *stream) {
    if (!I_dev || !QQ_dev || !cycle_sizes_ok(m, n_total, threshold) || !strides_ok(m, 4, qq_rs, qq_cs)) return IROTAVG_ERR_BAD_ARG;
    if (!aligned8(I_dev) || !aligned8(QQ_dev) || !aligned8(tri_min_dev) || (reinterpret_cast<uintptr_t>(tri_count_dev) & 3) != 0 ||
        (reinterpret_cast<uintptr_t>(tri_ok_dev) & 3) != 0)
        return IROTAVG_ERR_BAD_ARG;
    if (irotavg_device_count() <= 0) return IROTAVG_ERR_NO_DEVICE;
    return guarded([&]() -> int {
        int device = 0;
        IRH_CHECK(hipGetDevice(&device));
        if (!dev_index_ok(I_dev, m, device) || !dev_matrix_ok(QQ_dev, m, 4, qq_rs, qq_cs, device)) return IROTAVG_ERR_BAD_ARG;
        int32_t *const counts[2] = {tri_count_dev, tri_ok_dev};
        for (int32_t *p : counts)
            if (p && !dev_span_ok(p, p + m - 1, device)) return IROTAVG_ERR_BAD_ARG;
        if (tri_min_dev && !dev_vector_ok(tri_min_dev, m, device)) return IROTAVG_ERR_BAD_ARG;
        const CycleArrays A{I_dev, QQ_dev, (long long)qq_rs, (long long)qq_cs, tri_count_dev, tri_ok_dev, tri_min_dev};
        return cycle_check_dev(m, n_total, A, threshold, summary, static_cast<hipStream_t>(stream));
    });
}

int irotavg_cycle_check_group(int lanes) { return cycle_check_group(lanes); }

// The order-free spanning-tree initialiser (docs/init_tree.md; the kernels: treeinit.hip). Handle-free; the device form runs
// on the caller's stream itself, as the cycle check does.
static bool tree_sizes_ok(int64_t m, int64_t n_total, int f) {
    return m > 0 && m <= 0x7fffffffLL && n_total > 0 && n_total <= 0x7fffffffLL && f >= 1 && f <= n_total;
}
static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

int irotavg_init_tree(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq, const int32_t *rank,
                      double *Q, int64_t ldq, int32_t *in_tree, int64_t info[4]) {
    if (!I || !QQ || !Q || !tree_sizes_ok(m, n_total, f) || ldqq < m || ldq < n_total) return IROTAVG_ERR_BAD_ARG;
    if (irotavg_device_count() <= 0) return IROTAVG_ERR_NO_DEVICE;
    return guarded([&]() -> int { return init_tree_host(m, n_total, f, I, QQ, ldqq, rank, Q, ldq, in_tree, info); });
}

int irotavg_init_tree_dev(int64_t m, int64_t n_total, int f, const int32_t *I_dev, const double *QQ_dev, int64_t qq_rs,
                          int64_t qq_cs, const int32_t *rank_dev, double *Q_dev, int64_t q_rs, int64_t q_cs,
                          int32_t *in_tree_dev, int64_t *info, void *stream) {
    if (!I_dev || !QQ_dev || !Q_dev || !tree_sizes_ok(m, n_total, f) || !strides_ok(m, 4, qq_rs, qq_cs) ||
        !strides_ok(n_total, 4, q_rs, q_cs))
        return IROTAVG_ERR_BAD_ARG;
    if (!aligned8(I_dev) || !aligned8(QQ_dev) || !aligned8(Q_dev) || !aligned4(rank_dev) || !aligned4(in_tree_dev))
        return IROTAVG_ERR_BAD_ARG;
    if (irotavg_device_count() <= 0) return IROTAVG_ERR_NO_DEVICE;
    return guarded([&]() -> int {
        int device = 0;
        IRH_CHECK(hipGetDevice(&device));
        if (!dev_index_ok(I_dev, m, device) || !dev_matrix_ok(QQ_dev, m, 4, qq_rs, qq_cs, device) ||
            !dev_matrix_ok(Q_dev, n_total, 4, q_rs, q_cs, device))
            return IROTAVG_ERR_BAD_ARG;
        const int32_t *const per_edge[2] = {rank_dev, in_tree_dev};
        for (const int32_t *p : per_edge)
            if (p && !dev_span_ok(p, p + m - 1, device)) return IROTAVG_ERR_BAD_ARG;
        const TreeArrays A{I_dev, QQ_dev, (long long)qq_rs, (long long)qq_cs, rank_dev, Q_dev, (long long)q_rs, (long long)q_cs,
                           in_tree_dev};
        return init_tree_dev(m, n_total, f, A, info, static_cast<hipStream_t>(stream));
    });
}

void irotavg_init_tree_counters(int64_t out[2]) {
    if (out) init_tree_counters(out);
}

}  // extern "C"
