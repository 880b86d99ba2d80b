// bcr_route.hpp -- which launches one solve of the banded direct solver (bcr.hip) is made of: decided HERE, once, from what
// the caller asks (BcrRequest) and what the handle is (BcrShape). Host-only, no HIP: tools/bcr_route_host_check.cpp walks
// the whole input space without a device. bcr.hip launches what the BcrRoute says; DESIGN.md 5a has the table.
#pragma once
#include <algorithm>

namespace irh {
constexpr int kUpLevels = 8;             // levels above level 0 that k_bcr_reduce_up takes in one launch
constexpr int kBcrMaxLevels = 16;        // (= kMaxLevels, common.hpp)
constexpr int kBcrApplySlotsMax = 2048;  // (= 4 kMaxParts: the doubles of the pinned block a score comes back in)

struct BcrRequest {         // what a caller asks of one solve
    int only = -1;          // >= 0: one launch alone (time_kernel): l = the reduction of level l, 100 + l = its way back
    int phase = 0;          // 0 the whole solve, 1 the reductions, 2 the ways back (closures and shards work in between)
    bool open_top = false;  // a shard: the last level writes its separator data like every other level
    bool assemble = false;  // level 0 assembles its own slices first (ls_solve skipped K3: bcr_can_assemble)
    int unit = 0;           // the unit-weight factor: 1 run_irls's first solve of a call; time_kernel: 2 the right-hand-
                            // side-only solve of a valid store, 3 its upper launch alone
    bool apply = false;     // the ways back also make the step (K6) and leave the score's partial sums in part_score
    void *out = nullptr;    // the solution goes here (double4 rows) instead of X: the guarded solve of the closure path
    int dbg = -1;           // the debug word of this solve (bcr_stamps*); -1: the handle's switch
};
struct BcrShape {                 // what the handle is
    int B = 0, nl = 0;            // rows of a block (0: no direct solver), levels (0: not allocated yet)
    int nch[kBcrMaxLevels] = {};  // chunks of eight per level
    bool top16 = false;           // the last level is one workgroup of <= 16 blocks that makes its own way back
    int nfar = 0, ng = 0;         // loop closures, ghost views
    bool shard = false, guard = false, asm_windowed = false;  // (guard: Graph::bcr_guard)
    int dbg = 0;                  // the switches the route reads
    bool no_fused_asm = false, no_unit_factor = false, no_fused_up = false;
    bool unit_valid = false;      // a kept unit-weight factor is valid (read after the epoch check released a trimmed one)
};
// the instantiation of k_bcr_reduce a level launched on its own takes: <B, 3, l0, top, wide ? 8 : 4, assemble, uf>
struct BcrLaunch {
    bool l0 = false, top = false, wide = false, assemble = false;
    int uf = 0;
};
enum BcrRed : unsigned char { kRedNone, kRedOwn, kRedUp, kRedTopAlone };
enum BcrBack : unsigned char { kBackNone, kBackOwn, kBackTop, kBackWithRed };
struct BcrRoute {             // what happens
    bool fused_up = false;    // the levels above level 0 in one launch (k_bcr_reduce_up; with top16 it ends in the top)
    int uf = 0;               // the unit-weight factor: 1 this solve fills the store, 2 it is served from it
    bool uf_up_only = false;  // ... its upper launch alone
    bool asm0 = false;        // level 0's launch assembles its slices first
    bool top_alone = false;   // the single-workgroup top in a launch of its own (k_bcr_top)
    bool fused_back = false;  // the ways back of the levels above level 0 in one launch (k_bcr_back_top)
    bool apply = false;       // the ways back make the step ...
    int apply_slots = 0;      // ... and leave this many partial sums
    unsigned char red[kBcrMaxLevels] = {};   // BcrRed: who reduces level l in this call (kRedUp: launched at level 1)
    unsigned char back[kBcrMaxLevels] = {};  // BcrBack: who makes its way back (kBackTop: launched at level 1;
                                             // kBackWithRed: the single-workgroup top did inside its reduction)
    BcrLaunch own[kBcrMaxLevels];            // for red[l] == kRedOwn
};

inline int bcr_dbg(const BcrShape &s, const BcrRequest &q) { return q.dbg >= 0 ? q.dbg : s.dbg; }
// ls_solve: no launch of K3 on a plain banded handle whose chunks of eight blocks are whole slices. Everything else
// assembles in a launch of its own: closures, shards, blocks of 12 / 20 / 28 rows, the classic assembly, the
// level-by-level repeat after a wait that gave up. (Reads no level: valid before the handle allocates them.)
inline bool bcr_can_assemble(const BcrShape &s) {
    return s.B > 0 && (8 * s.B) % 64 == 0 && s.asm_windowed && s.nfar == 0 && !s.shard && s.ng == 0 && !s.no_fused_up &&
           !s.no_fused_asm;
}
// partial sums of the score a solve that applies leaves in part_score (one per workgroup of the two ways back), or 0 when
// a solve cannot make the step itself: closures, a shard, one level, more slots than the pinned block has doubles
inline int bcr_apply_slots(const BcrShape &s) {
    if (!s.B || s.nfar != 0 || s.shard || s.ng != 0 || s.nl < 2) return 0;
    // (level 0's chunks and, when there is a level of chunks above them, level 1's: a mixed level 1 writes solution rows)
    const int slots = s.nch[0] + (s.top16 && s.nl == 2 ? 0 : s.nch[1]);
    return slots <= kBcrApplySlotsMax ? slots : 0;
}
// the reductions of all levels above level 0 in one launch: blocks up to 24 (the eight-wave workgroups), at least two such
// levels, level 1 of at most 256 chunks (one workgroup per CU: all resident), no closures (their inverses and dead-pivot
// count ride on the separate launches), not a shard, not when single levels are timed. The launch still has to be
// granted its share of the device (bcr_up_reserve, bcr.hip).
inline bool bcr_wants_up(const BcrShape &s, const BcrRequest &q) {
    return s.B <= 24 && s.nl >= 3 && s.nl - 1 <= kUpLevels && q.only < 0 && q.phase == 0 && !q.open_top && !s.shard &&
           s.nfar == 0 && s.nch[1] <= 256 && !(bcr_dbg(s, q) & 64) && !s.no_fused_up;
}
// the solve may fill the unit-weight store or be served from it: the plain route -- level 0 assembling its own slices, the
// upper levels in one launch, a sixteen-block top, blocks of 8 / 16 / 24, no debug word, not guarded. (bcr.hip releases a
// trimmed store between this and bcr_route, which reads BcrShape::unit_valid.)
inline bool bcr_wants_unit(const BcrShape &s, const BcrRequest &q, bool fused_up) {
    return (s.B == 8 || s.B == 16 || s.B == 24) && q.unit != 0 && fused_up && s.top16 && bcr_dbg(s, q) == 0 && !s.guard &&
           !q.out && !s.no_unit_factor && (q.assemble || q.unit == 3);
}
// up_reserved: bcr_up_reserve granted the upper launch its share (asked only when bcr_wants_up)
inline BcrRoute bcr_route(const BcrShape &s, const BcrRequest &q, bool up_reserved) {
    BcrRoute r;
    const int nl = s.nl;
    r.fused_up = up_reserved && bcr_wants_up(s, q);
    if (bcr_wants_unit(s, q, r.fused_up)) r.uf = s.unit_valid ? 2 : (q.unit == 1 ? 1 : 0);
    r.uf_up_only = r.uf == 2 && q.unit == 3;
    r.asm0 = (8 * s.B) % 64 == 0 && q.assemble && q.only < 0 && q.phase == 0 && !q.open_top && s.nfar == 0 && !s.shard &&
             !r.uf_up_only;
    for (int l = 0; l < nl && q.phase != 2; l++) {
        if ((q.only >= 0 && q.only != l) || (l == 0 && r.uf_up_only)) continue;
        if (s.top16 && l == nl - 1 && !r.fused_up) {
            r.red[l] = kRedTopAlone;
            r.top_alone = true;
        } else if (r.fused_up && l >= 1) {
            r.red[l] = kRedUp;
        } else {
            r.red[l] = kRedOwn;
            // (eight waves per chunk when every chunk has a CU to itself)
            r.own[l] = BcrLaunch{l == 0, l == nl - 1 && !q.open_top, s.B <= 24 && s.nch[l] <= 256, l == 0 && r.asm0,
                                 l == 0 && r.asm0 ? r.uf : 0};
        }
    }
    // (a single-workgroup top has made its own way back: the levels below it are left)
    const int ltop = s.top16 ? nl - 2 : nl - 1;
    r.fused_back = ltop >= 1 && !s.shard && !q.open_top;
    // K6 inside the ways back: every solution row of level 0 is written by k_bcr_back (level 0's chunks) or, on a mixed
    // level 1, by k_bcr_back_top
    r.apply = q.apply && q.only < 0 && q.phase == 0 && !r.uf_up_only && (r.fused_back || (s.top16 && nl == 2)) && !q.out &&
              s.ng == 0 && bcr_apply_slots(s) > 0;
    r.apply_slots = r.apply ? bcr_apply_slots(s) : 0;
    for (int l = ltop; l >= 0 && q.phase != 1 && !r.uf_up_only; l--) {
        if (r.fused_back && l >= 1) {
            if (q.only < 0 || q.only == 101) r.back[l] = kBackTop;
        } else if (q.only < 0 || q.only == 100 + l) {
            r.back[l] = kBackOwn;
        }
    }
    if (s.top16 && nl >= 1 && r.red[nl - 1] != kRedNone) r.back[nl - 1] = kBackWithRed;
    return r;
}
}  // namespace irh
