// cycles.hpp -- the triangle test of relative rotations (irotavg_cycle_check, docs/cycle_check.md): the half-edge key, the
// directed measurement, the triangle error, the row lookup in the sorted half-edges, the walk of one entry of the shorter
// row, and two host forms to hold the kernels against. Plain C++ with no HIP type in it, as winmst.hpp:
// tools/cycles_host_check.cpp runs all of it under sanitizers on a machine without a device. k_cyc_emit and
// k_cyc_triangles (cycles.hip) take every piece from here, so there is one copy of each.
//
// Layout: edge k = (a, b) gives two half-edges, key (a << 32) | b with value 2k and key (b << 32) | a with value 2k + 1
// (the low bit: the half-edge runs against the stored direction). Sorted by key, the half-edges that leave view u are one
// contiguous row, its neighbours ascending, parallel edges next to each other. A self loop gives two keys of all ones:
// they sort behind every row (a neighbour id never has bit 31 set) and no lookup reaches them. Memory is 2m keys and 2m
// values whatever n_total is; a row is found by two binary searches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define IRH_CYC_HD __host__ __device__ __forceinline__
#else
#define IRH_CYC_HD inline
#endif

namespace irh {

constexpr uint64_t CYC_KEY_NONE = ~0ull;
constexpr long long CYC_COUNT_MAX = 0x7fffffffLL;
constexpr double CYC_PI = 3.141592653589793238462643383279502884;

IRH_CYC_HD uint64_t cyc_key(uint32_t u, uint32_t v) { return ((uint64_t)u << 32) | v; }
IRH_CYC_HD uint32_t cyc_key_to(uint64_t key) { return (uint32_t)key; }
IRH_CYC_HD uint32_t cyc_val(uint32_t k, bool against) { return 2u * k + (against ? 1u : 0u); }
IRH_CYC_HD uint32_t cyc_val_edge(uint32_t val) { return val >> 1; }
IRH_CYC_HD bool cyc_val_against(uint32_t val) { return (val & 1u) != 0; }
IRH_CYC_HD bool cyc_id_ok(int32_t v, int64_t n_total) { return v >= 0 && (int64_t)v < n_total; }
// the key bits a sort has to look at: 32 of the neighbour, and those of the largest source id
inline int cyc_key_bits(int64_t n_total) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) < n_total) b++;
    return 32 + b;
}
// the two half-edges of edge k; a self loop (and an id that failed the guard) gives two keys that no row holds
IRH_CYC_HD void cyc_emit(uint32_t k, int32_t a, int32_t b, bool usable, uint64_t key[2], uint32_t val[2]) {
    const bool row = usable && a != b;
    key[0] = row ? cyc_key((uint32_t)a, (uint32_t)b) : CYC_KEY_NONE;
    key[1] = row ? cyc_key((uint32_t)b, (uint32_t)a) : CYC_KEY_NONE;
    val[0] = cyc_val(k, false);
    val[1] = cyc_val(k, true);
}

struct CycQ {
    double x, y, z, w;
};
// the product, operand by operand as qmul (kernels.hpp); the products stay products on the host and on the device
IRH_CYC_HD CycQ cyc_qmul(const CycQ a, const CycQ b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    CycQ r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
// q(k, u -> v): the stored quaternion along the stored direction, only w negated against it (edge_log's inverse)
IRH_CYC_HD CycQ cyc_directed(CycQ q, bool against) {
    if (against) q.w = -q.w;
    return q;
}
// q0 = q(k, a -> b), q1 = q(k1, b -> c), q2 = q(k2, c -> a); the angle wrapped as edge_log wraps it
IRH_CYC_HD double cyc_triangle_error(const CycQ q0, const CycQ q1, const CycQ q2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const CycQ d = cyc_qmul(q2, cyc_qmul(q1, q0));
    const double s = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    double th = 2.0 * atan2(s, d.w);
    if (th < -CYC_PI)
        th += 2.0 * CYC_PI;
    else if (th >= CYC_PI)
        th -= 2.0 * CYC_PI;
    return fabs(th);
}

struct CycAcc {
    long long count, ok;
    double mn;
};
IRH_CYC_HD CycAcc cyc_acc_zero() {
    CycAcc a;
    a.count = 0;
    a.ok = 0;
    a.mn = std::numeric_limits<double>::infinity();
    return a;
}
// a NaN counts, is never ok and leaves the minimum alone: both comparisons are false
IRH_CYC_HD void cyc_acc_add(CycAcc &a, double err, double threshold) {
    a.count++;
    if (err <= threshold) a.ok++;
    if (err < a.mn) a.mn = err;
}
IRH_CYC_HD void cyc_acc_merge(CycAcc &a, long long count, long long ok, double mn) {
    a.count += count;
    a.ok += ok;
    if (mn < a.mn) a.mn = mn;
}
IRH_CYC_HD int32_t cyc_stored_count(long long c) { return (int32_t)(c > CYC_COUNT_MAX ? CYC_COUNT_MAX : c); }

// the first position in [lo, hi) whose key is not below `target` (hi if none); keys ascending. hi - lo < 2^31, and the
// span halves every round: 32 rounds end it whatever the keys hold.
IRH_CYC_HD long long cyc_lower_bound(const uint64_t *keys, long long lo, long long hi, uint64_t target) {
    for (int round = 0; round < 32 && lo < hi; round++) {
        const long long mid = lo + (hi - lo) / 2;
        if (keys[mid] < target)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// the row of view u among n2 sorted keys
IRH_CYC_HD void cyc_row(const uint64_t *keys, long long n2, uint32_t u, long long &beg, long long &end) {
    beg = cyc_lower_bound(keys, 0, n2, cyc_key(u, 0u));
    end = cyc_lower_bound(keys, beg, n2, cyc_key(u + 1u, 0u));
}

// Entry i of the shorter row (the row of x, one end of edge k = (a, b); y is the other end) against the longer row
// [l0, l1) of y: its neighbour c is looked up there, and every half-edge y -> c of the run of equals closes a triangle
// with it. x_is_b: the entry is k1 (b -> c) and the run holds k2 (as a -> c, to be turned); otherwise the other way round.
// load(k) gives QQ_k as a CycQ.
template <class Load>
IRH_CYC_HD void cyc_entry(const uint64_t *keys, const uint32_t *vals, long long i, uint32_t y, bool x_is_b, long long l0,
                          long long l1, const CycQ q0, double threshold, const Load &load, CycAcc &acc) {
    const uint32_t c = cyc_key_to(keys[i]);
    if (c == y) return;  // edge k itself or one parallel to it (c == x does not occur: self loops have no row)
    const uint64_t target = cyc_key(y, c);
    long long j = cyc_lower_bound(keys, l0, l1, target);
    if (j >= l1 || keys[j] != target) return;
    const uint32_t vx = vals[i];
    // x == b: the entry runs b -> c as k1 needs it; x == a: it runs a -> c and k2 needs c -> a
    const CycQ qx = cyc_directed(load(cyc_val_edge(vx)), x_is_b ? cyc_val_against(vx) : !cyc_val_against(vx));
    for (; j < l1 && keys[j] == target; j++) {
        const uint32_t vy = vals[j];
        const CycQ qy = cyc_directed(load(cyc_val_edge(vy)), x_is_b ? !cyc_val_against(vy) : cyc_val_against(vy));
        cyc_acc_add(acc, x_is_b ? cyc_triangle_error(q0, qx, qy) : cyc_triangle_error(q0, qy, qx), threshold);
    }
}

// ---- host forms -------------------------------------------------------------------------------------------------------------
enum { CYC_OK = 0, CYC_BAD_ID = 1 };
struct CycResult {
    std::vector<int32_t> count, ok;
    std::vector<double> mn;
    long long summary[4] = {0, 0, 0, 0};
};
struct CycAosLoad {  // QQ as m rows [x y z w]
    const double *qq;
    CycQ operator()(uint32_t k) const { return CycQ{qq[4 * (size_t)k], qq[4 * (size_t)k + 1], qq[4 * (size_t)k + 2], qq[4 * (size_t)k + 3]}; }
};
inline void cyc_store(CycResult &R, size_t k, const CycAcc &a) {
    R.count[k] = cyc_stored_count(a.count);
    R.ok[k] = cyc_stored_count(a.ok);
    R.mn[k] = a.mn;
    R.summary[0] += R.count[k];
    R.summary[R.ok[k] >= 1 ? 1 : R.count[k] >= 1 ? 2 : 3]++;
}
inline int cyc_begin(int64_t m, int64_t n_total, const int32_t *I, CycResult &R) {
    for (int64_t k = 0; k < m; k++)
        if (!cyc_id_ok(I[2 * k], n_total) || !cyc_id_ok(I[2 * k + 1], n_total)) return CYC_BAD_ID;
    R.count.assign((size_t)m, 0);
    R.ok.assign((size_t)m, 0);
    R.mn.assign((size_t)m, std::numeric_limits<double>::infinity());
    for (long long &s : R.summary) s = 0;
    return CYC_OK;
}

// The kernels' way on one thread: emit, sort, and per edge the two rows, the shorter one dealt to `group` lanes that each
// keep their own sums, merged at the end. I: m pairs, qq: m rows [x y z w].
inline int cycles_sorted(int64_t m, int64_t n_total, const int32_t *I, const double *qq, double threshold, int group,
                         CycResult &R) {
    if (cyc_begin(m, n_total, I, R) != CYC_OK) return CYC_BAD_ID;
    std::vector<std::pair<uint64_t, uint32_t>> half((size_t)(2 * m));
    for (int64_t k = 0; k < m; k++) {
        uint64_t key[2];
        uint32_t val[2];
        cyc_emit((uint32_t)k, I[2 * k], I[2 * k + 1], true, key, val);
        half[(size_t)(2 * k)] = {key[0], val[0]};
        half[(size_t)(2 * k + 1)] = {key[1], val[1]};
    }
    const uint64_t mask = cyc_key_bits(n_total) >= 64 ? ~0ull : (((uint64_t)1 << cyc_key_bits(n_total)) - 1);
    std::stable_sort(half.begin(), half.end(), [mask](const std::pair<uint64_t, uint32_t> &p, const std::pair<uint64_t, uint32_t> &q) {
        return (p.first & mask) < (q.first & mask);  // (what a radix sort of that many bits sees)
    });
    std::vector<uint64_t> keys(half.size());
    std::vector<uint32_t> vals(half.size());
    for (size_t t = 0; t < half.size(); t++) keys[t] = half[t].first, vals[t] = half[t].second;
    const long long n2 = (long long)keys.size();
    const CycAosLoad load{qq};
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        CycAcc total = cyc_acc_zero();
        if (a != b) {
            long long a0, a1, b0, b1;
            cyc_row(keys.data(), n2, (uint32_t)a, a0, a1);
            cyc_row(keys.data(), n2, (uint32_t)b, b0, b1);
            const bool x_is_b = b1 - b0 <= a1 - a0;
            const long long s0 = x_is_b ? b0 : a0, s1 = x_is_b ? b1 : a1, l0 = x_is_b ? a0 : b0, l1 = x_is_b ? a1 : b1;
            const uint32_t y = (uint32_t)(x_is_b ? a : b);
            const CycQ q0 = load((uint32_t)k);
            for (int lane = 0; lane < group; lane++) {
                CycAcc acc = cyc_acc_zero();
                for (long long i = s0 + lane; i < s1; i += group)
                    cyc_entry(keys.data(), vals.data(), i, y, x_is_b, l0, l1, q0, threshold, load, acc);
                cyc_acc_merge(total, acc.count, acc.ok, acc.mn);
            }
        }
        cyc_store(R, (size_t)k, total);
    }
    return CYC_OK;
}

// The definition, literally and in sequence: for edge k = (a, b), every half-edge b -> c with c outside {a, b}, and for
// each of them every edge that joins c and a.
inline int cycles_reference(int64_t m, int64_t n_total, const int32_t *I, const double *qq, double threshold, CycResult &R) {
    if (cyc_begin(m, n_total, I, R) != CYC_OK) return CYC_BAD_ID;
    typedef std::pair<uint32_t, bool> Half;                       // edge, against its stored direction
    std::map<int32_t, std::vector<std::pair<int32_t, Half>>> out;  // view -> (neighbour, half-edge)
    std::map<std::pair<int32_t, int32_t>, std::vector<Half>> between;  // (u, v) -> the half-edges u -> v
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        if (a == b) continue;
        out[a].push_back({b, Half((uint32_t)k, false)});
        out[b].push_back({a, Half((uint32_t)k, true)});
        between[{a, b}].push_back(Half((uint32_t)k, false));
        between[{b, a}].push_back(Half((uint32_t)k, true));
    }
    const CycAosLoad load{qq};
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        CycAcc acc = cyc_acc_zero();
        if (a != b)
            for (const std::pair<int32_t, Half> &e1 : out[b]) {
                const int32_t c = e1.first;
                if (c == a || c == b) continue;
                const auto it = between.find({c, a});
                if (it == between.end()) continue;
                for (const Half &e2 : it->second)
                    cyc_acc_add(acc, cyc_triangle_error(load((uint32_t)k), cyc_directed(load(e1.second.first), e1.second.second),
                                                        cyc_directed(load(e2.first), e2.second)), threshold);
            }
        cyc_store(R, (size_t)k, acc);
    }
    return CYC_OK;
}

}  // namespace irh
