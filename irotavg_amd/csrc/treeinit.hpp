// treeinit.hpp -- the order-free spanning-tree initialiser (irotavg_init_tree, irotavg_init_tree_dev; docs/init_tree.md):
// the key of an edge, its directed measurement, the quaternion product, the label algebra of the union-find, the step of
// every kernel as a function of one edge or one view, and two host forms to hold the kernels against. Plain C++ with no
// HIP type in it, as cycles.hpp and winmst.hpp: tools/treeinit_host_check.cpp runs all of it under sanitizers on a machine
// without a device. The kernels of treeinit.hip take every piece from here, so there is one copy of each.
//
// Definition: the tree is the minimum spanning forest under the keys (rank[k], k), which are distinct, so it is unique;
// T(0) = Q[0], T(b) = QQ_k (x) T(a) along a tree edge k = (a, b) walked from a, T(a) = QQ_k* (x) T(b) walked from b (QQ_k*:
// w negated); a free view v gets +-T(v) up to rounding.
//
// State per view: comp[v], the representative of its component, and rel[v] with T(v) = rel[v] (x) T(comp[v]) -- whatever
// T(comp[v]) turns out to be; rel of a representative is the identity. A Boruvka round: every usable edge between two
// components offers its key to both representatives (a minimum: order-free); a representative with an offer hooks under
// the other end's representative (of a mutual pair the smaller id stays); pointer jumping makes comp flat again.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define IRH_TREE_HD __host__ __device__ __forceinline__
#else
#define IRH_TREE_HD inline
#endif

namespace irh {

constexpr uint64_t TREE_KEY_NONE = ~0ull;  // no key is all ones: k < 2^31
constexpr int TREE_MAX_ROUNDS = 32;        // components at least halve per round, n_total < 2^31
constexpr int TREE_MAX_JUMPS = 32;         // a pointer covers 2^j hooks after j passes

IRH_TREE_HD bool tree_id_ok(int32_t v, int64_t n_total) { return v >= 0 && (int64_t)v < n_total; }
// rank < 0: never used; self loops: never used
IRH_TREE_HD bool tree_usable(int32_t a, int32_t b, int32_t rank) { return rank >= 0 && a != b; }
IRH_TREE_HD uint64_t tree_key(int32_t rank, uint32_t k) { return ((uint64_t)(uint32_t)rank << 32) | k; }
IRH_TREE_HD uint32_t tree_key_edge(uint64_t key) { return (uint32_t)key; }
IRH_TREE_HD int32_t tree_key_rank(uint64_t key) { return (int32_t)(key >> 32); }

struct alignas(16) TreeQ {
    double x, y, z, w;
};
IRH_TREE_HD TreeQ tree_identity() { return TreeQ{0.0, 0.0, 0.0, 1.0}; }
// the product, operand by operand as qmul (kernels.hpp) and cyc_qmul; the products stay products on the host and on the
// device, so both give the same bits
IRH_TREE_HD TreeQ tree_qmul(const TreeQ a, const TreeQ b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    TreeQ r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
// the library's inverse: only w negated (for a unit quaternion the conjugate up to sign)
IRH_TREE_HD TreeQ tree_inv(TreeQ q) {
    q.w = -q.w;
    return q;
}
// q(k, u -> v): the stored quaternion along the stored direction a -> b, its inverse against it
IRH_TREE_HD TreeQ tree_directed(const TreeQ q, bool against) { return against ? tree_inv(q) : q; }

// ---- the label algebra --------------------------------------------------------------------------------------------------
// r hooks under lo over the edge other -> mine (mine in r's component, other in lo's):
//   T(mine) = q (x) T(other), T(mine) = rel[mine] (x) T(r), T(other) = rel[other] (x) T(lo)
//   => T(r) = rel[mine]^-1 (x) q (x) rel[other] (x) T(lo)
IRH_TREE_HD TreeQ tree_hook_label(const TreeQ rel_mine, const TreeQ q_other_to_mine, const TreeQ rel_other) {
    return tree_qmul(tree_inv(rel_mine), tree_qmul(q_other_to_mine, rel_other));
}
// v points at p, p at comp[p]: T(v) = rel[v] (x) rel[p] (x) T(comp[p]) (p a representative: rel[p] is the identity and the
// product is exact)
IRH_TREE_HD TreeQ tree_jump_label(const TreeQ rel_v, const TreeQ rel_p) { return tree_qmul(rel_v, rel_p); }
// one component left, its representative r: T(0) = rel[0] (x) T(r) = Q[0], so T(r) = rel[0]^-1 (x) Q[0]; with r == 0 that
// is Q[0] itself and no product is formed
IRH_TREE_HD TreeQ tree_base(bool zero_is_root, const TreeQ rel0, const TreeQ q0) {
    return zero_is_root ? q0 : tree_qmul(tree_inv(rel0), q0);
}
IRH_TREE_HD TreeQ tree_row(const TreeQ rel_v, const TreeQ base) { return tree_qmul(rel_v, base); }

// ---- the kernels' steps ---------------------------------------------------------------------------------------------------
// Offer: the two representatives edge k = (a, b) offers its key to; false: not usable, or both ends in one component.
IRH_TREE_HD bool tree_offer_ends(int32_t a, int32_t b, int32_t rank, const int32_t *comp, int32_t &ca, int32_t &cb) {
    if (!tree_usable(a, b, rank)) return false;
    ca = comp[a];
    cb = comp[b];
    return ca != cb;
}

struct TreeHook {
    int32_t parent;  // the representative v hooks under
    uint32_t edge;   // over this edge
    int32_t rank;    // its rank
    TreeQ label;     // T(v) = label (x) T(parent)
};
// Hook: does view v hook this round, and how? comp, rel, best: the state of BEFORE the round (the caller writes elsewhere).
// load(k) gives QQ_k as a TreeQ.
template <class Load>
IRH_TREE_HD bool tree_hook(int32_t v, const int32_t *comp, const TreeQ *rel, const uint64_t *best, const int32_t *I,
                           const Load &load, TreeHook &h) {
    if (comp[v] != v) return false;
    const uint64_t key = best[v];
    if (key == TREE_KEY_NONE) return false;
    const uint32_t k = tree_key_edge(key);
    const int32_t a = I[2 * (size_t)k], b = I[2 * (size_t)k + 1];
    const int32_t ca = comp[a], cb = comp[b];
    if ((ca == v) == (cb == v)) return false;  // (does not occur: an offer reaches the representatives of its two ends)
    const bool mine_is_b = cb == v;
    const int32_t mine = mine_is_b ? b : a, other = mine_is_b ? a : b, lo = mine_is_b ? ca : cb;
    // the mutual pick: both chose this edge, the smaller id stays a representative. No other cycle can arise: along a
    // chain of picks the keys fall strictly, so a cycle needs two equal keys, and keys are distinct.
    if (best[lo] == key && v < lo) return false;
    h.parent = lo;
    h.edge = k;
    h.rank = tree_key_rank(key);
    h.label = tree_hook_label(rel[mine], tree_directed(load(k), !mine_is_b), rel[other]);
    return true;
}
// Jump: comp and rel of v one doubling further; true: the pointer moved.
IRH_TREE_HD bool tree_jump(int32_t v, const int32_t *comp, const TreeQ *rel, int32_t &comp_new, TreeQ &rel_new) {
    const int32_t p = comp[v];
    comp_new = comp[p];
    rel_new = tree_jump_label(rel[v], rel[p]);
    return comp_new != p;
}
// the passes one round is given: a chain of hooks among `reps` representatives is at most reps - 1 long, a view that is
// none hangs one further down; ceil(log2(reps)) passes move a pointer, one more sees that none did
inline int tree_jump_passes(int64_t reps) {
    int j = 0;
    while (j < TREE_MAX_JUMPS - 1 && ((int64_t)1 << j) < reps) j++;
    return j + 1;
}

// ---- host forms -------------------------------------------------------------------------------------------------------------
enum { TREE_OK = 0, TREE_BAD_ID = 1, TREE_NOT_SPANNING = 2, TREE_INTERNAL = 3 };
struct TreeResult {
    std::vector<TreeQ> T;          // n_total rows; meaningful for v >= f, on success (rows < f: untouched)
    std::vector<int32_t> in_tree;  // m, on success
    long long info[4] = {0, 0, 0, 0};  // rounds, components left, tree edges with rank > 0, largest rank in the tree
    long long launches = 0;        // tree_rounds: what the device form would launch (kernels and fills)
    int jumps_max = 0;             // tree_rounds: the most passes of one round that moved a pointer
};
struct TreeAosLoad {  // QQ as m rows [x y z w]
    const double *qq;
    TreeQ operator()(uint32_t k) const { return TreeQ{qq[4 * (size_t)k], qq[4 * (size_t)k + 1], qq[4 * (size_t)k + 2], qq[4 * (size_t)k + 3]}; }
};
inline bool tree_ids_ok(int64_t m, int64_t n_total, const int32_t *I) {
    for (int64_t k = 0; k < m; k++)
        if (!tree_id_ok(I[2 * k], n_total) || !tree_id_ok(I[2 * k + 1], n_total)) return false;
    return true;
}

// The kernels' way on one thread: init, then per round fill / offer / hook / jumps, every pass over the state of before
// it, written to the other copy where the kernels do so. I: m pairs, qq: m rows [x y z w], rank: m or nullptr, q0: Q[0].
inline int tree_rounds(int64_t m, int64_t n_total, int f, const int32_t *I, const double *qq, const int32_t *rank, const TreeQ q0,
                       TreeResult &R) {
    R = TreeResult();
    R.launches = 2;  // init, guard
    if (!tree_ids_ok(m, n_total, I)) return TREE_BAD_ID;
    const size_t n = (size_t)n_total;
    std::vector<int32_t> comp[2] = {std::vector<int32_t>(n), std::vector<int32_t>(n)};
    std::vector<TreeQ> rel[2] = {std::vector<TreeQ>(n, tree_identity()), std::vector<TreeQ>(n, tree_identity())};
    std::vector<uint64_t> best(n);
    std::vector<int32_t> via(n, -1);
    for (size_t v = 0; v < n; v++) comp[0][v] = comp[1][v] = (int32_t)v;
    const TreeAosLoad load{qq};
    long long comps = n_total, rank_pos = 0, rank_max = 0, rounds = 0;
    for (int round = 0; comps > 1; round++) {
        if (round >= TREE_MAX_ROUNDS) return TREE_INTERNAL;
        std::fill(best.begin(), best.end(), TREE_KEY_NONE);
        for (int64_t k = 0; k < m; k++) {
            int32_t ca, cb;
            if (!tree_offer_ends(I[2 * k], I[2 * k + 1], rank ? rank[k] : 0, comp[0].data(), ca, cb)) continue;
            const uint64_t key = tree_key(rank ? rank[k] : 0, (uint32_t)k);
            best[(size_t)ca] = std::min(best[(size_t)ca], key);
            best[(size_t)cb] = std::min(best[(size_t)cb], key);
        }
        // both copies hold the same state here; the hooks go into copy 1 alone
        long long hooks = 0;
        for (size_t v = 0; v < n; v++) {
            TreeHook h;
            if (!tree_hook((int32_t)v, comp[0].data(), rel[0].data(), best.data(), I, load, h)) continue;
            comp[1][v] = h.parent;
            rel[1][v] = h.label;
            via[v] = (int32_t)h.edge;
            hooks++;
            if (h.rank > 0) rank_pos++;
            rank_max = std::max<long long>(rank_max, h.rank);
        }
        const int passes = tree_jump_passes(comps);
        R.launches += 3 + passes;
        bool moved = true;
        int ran = 0;
        for (int j = 0; j < passes && moved; j++, ran++) {  // pass j: copy (j + 1) & 1 -> copy j & 1
            const int src = (j + 1) & 1, dst = j & 1;
            moved = false;
            for (size_t v = 0; v < n; v++)
                if (tree_jump((int32_t)v, comp[src].data(), rel[src].data(), comp[dst][v], rel[dst][v])) moved = true;
        }
        if (moved) return TREE_INTERNAL;  // (the last pass that ran moved nothing: both copies are the same again)
        R.jumps_max = std::max(R.jumps_max, ran - 1);
        if (hooks == 0) break;
        comps -= hooks;
        rounds++;
    }
    R.info[0] = rounds;
    R.info[1] = comps;
    R.info[2] = rank_pos;
    R.info[3] = rank_max;
    if (comps > 1) return TREE_NOT_SPANNING;
    R.launches += 2;  // the fill of in_tree, finish
    R.T.assign(n, tree_identity());
    R.in_tree.assign((size_t)m, 0);
    const TreeQ base = tree_base(comp[0][0] == 0, rel[0][0], q0);
    for (size_t v = 0; v < n; v++) {
        if (v >= (size_t)f) R.T[v] = tree_row(rel[0][v], base);
        if (via[v] >= 0) R.in_tree[(size_t)via[v]] = 1;
    }
    return TREE_OK;
}

// The definition, literally: Kruskal over the sorted keys, then a propagation from view 0 along the tree in long double.
// info[0] comes from a count of Boruvka rounds on a union-find of its own (no rotations, no pointer jumping).
inline int tree_reference(int64_t m, int64_t n_total, int f, const int32_t *I, const double *qq, const int32_t *rank, const TreeQ q0,
                          TreeResult &R) {
    R = TreeResult();
    if (!tree_ids_ok(m, n_total, I)) return TREE_BAD_ID;
    const size_t n = (size_t)n_total;
    std::vector<int32_t> parent(n);
    auto find = [&parent](int32_t v) {
        while (parent[(size_t)v] != v) v = parent[(size_t)v] = parent[(size_t)parent[(size_t)v]];
        return v;
    };
    std::vector<uint64_t> keys;
    for (int64_t k = 0; k < m; k++)
        if (tree_usable(I[2 * k], I[2 * k + 1], rank ? rank[k] : 0)) keys.push_back(tree_key(rank ? rank[k] : 0, (uint32_t)k));
    std::sort(keys.begin(), keys.end());
    for (size_t v = 0; v < n; v++) parent[v] = (int32_t)v;
    std::vector<std::vector<uint32_t>> adj(n);  // view -> its tree edges
    std::vector<int32_t> in_tree((size_t)m, 0);
    long long comps = n_total;
    for (const uint64_t key : keys) {
        const uint32_t k = tree_key_edge(key);
        const int32_t ra = find(I[2 * (size_t)k]), rb = find(I[2 * (size_t)k + 1]);
        if (ra == rb) continue;
        parent[(size_t)ra] = rb;
        comps--;
        in_tree[k] = 1;
        adj[(size_t)I[2 * (size_t)k]].push_back(k);
        adj[(size_t)I[2 * (size_t)k + 1]].push_back(k);
        if (tree_key_rank(key) > 0) R.info[2]++;
        R.info[3] = std::max<long long>(R.info[3], tree_key_rank(key));
    }
    R.info[1] = comps;
    // the rounds: every component picks its smallest key to another one, all picks are joined
    for (size_t v = 0; v < n; v++) parent[v] = (int32_t)v;
    for (int round = 0; round < 64; round++) {
        std::vector<uint64_t> best(n, TREE_KEY_NONE);
        for (const uint64_t key : keys) {
            const uint32_t k = tree_key_edge(key);
            const int32_t ra = find(I[2 * (size_t)k]), rb = find(I[2 * (size_t)k + 1]);
            if (ra == rb) continue;
            best[(size_t)ra] = std::min(best[(size_t)ra], key);
            best[(size_t)rb] = std::min(best[(size_t)rb], key);
        }
        bool joined = false;
        for (size_t v = 0; v < n; v++) {
            if (best[v] == TREE_KEY_NONE) continue;
            const uint32_t k = tree_key_edge(best[v]);
            const int32_t ra = find(I[2 * (size_t)k]), rb = find(I[2 * (size_t)k + 1]);
            if (ra != rb) parent[(size_t)ra] = rb;
            joined = true;
        }
        if (!joined) break;
        R.info[0]++;
    }
    if (comps > 1) return TREE_NOT_SPANNING;
    struct LQ {
        long double x, y, z, w;
    };
    auto mul = [](const LQ &a, const LQ &b) {
        return LQ{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                  a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
    };
    std::vector<LQ> T(n, LQ{0, 0, 0, 1});
    std::vector<char> seen(n, 0);
    std::vector<int32_t> queue(1, 0);
    T[0] = LQ{q0.x, q0.y, q0.z, q0.w};
    seen[0] = 1;
    for (size_t head = 0; head < queue.size(); head++) {
        const int32_t u = queue[head];
        for (const uint32_t k : adj[(size_t)u]) {
            const int32_t a = I[2 * (size_t)k], b = I[2 * (size_t)k + 1], v = a == u ? b : a;
            if (seen[(size_t)v]) continue;
            LQ e{qq[4 * (size_t)k], qq[4 * (size_t)k + 1], qq[4 * (size_t)k + 2], qq[4 * (size_t)k + 3]};
            if (v == a) e.w = -e.w;  // walked from b: the inverse
            T[(size_t)v] = mul(e, T[(size_t)u]);
            seen[(size_t)v] = 1;
            queue.push_back(v);
        }
    }
    R.T.assign(n, tree_identity());
    for (size_t v = (size_t)f; v < n; v++) R.T[v] = TreeQ{(double)T[v].x, (double)T[v].y, (double)T[v].z, (double)T[v].w};
    R.in_tree = in_tree;
    return TREE_OK;
}

}  // namespace irh
