// switches.hpp -- every IROTAVG_* environment variable the library reads: the one place that calls getenv.
// Switches is filled ONCE when a handle is made (irotavg_graph_create, a sharded handle, a view-graph; per call by the
// one-shot entry points, where it is part of the kept handle's key) and travels with it: Graph::sw, copied to l1ra's
// solver clones, to every shard and to what a view-graph creates. No solve looks at the environment. The process-wide
// readers at the end belong to singletons and keep their own timing. README.md has the user's view of this table.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <tuple>

namespace irh {

struct Switches {
    // which solver, which build
    bool has_band_direct = false;  // BAND_DIRECT is set: band_direct replaces irotavg_options::band_direct
    int band_direct = 0;
    int host_build = -1;           // -1: by size; 1 / 0: patterns on the host / on the device
    int upload_threads = 4;        // host threads (0 .. 4) that upload the relative rotations of a large graph
    bool asm_classic = false, no_small_tuning = false;
    // iterative solver
    bool no_dense_refine = false, no_band_inverse = false, pcg_trace = false;
    int cg2_giveup = 0;            // 0: the library's rule; n >= 1: the recurrences hand over after n iterations
    // IRLS
    bool no_settle = false, no_fused_cl = false;
    int inexact = -1;              // -1: by size; 1 / 0: inexact solves on / off
    // direct solver
    bool bcr_no_mixed = false, bcr_no_top16 = false, bcr_fake_up_fail = false, bcr_fake_give_up = false;
    bool bcr_no_closures = false, bcr_s_tiles = false, bcr_no_fused_asm = false, bcr_no_unit_factor = false;
    int bcr_up_cap = 1024;         // 1/1024ths of the device the single-launch upper reductions may reserve
    int bcr_dbg = 0, bcr_stamp_chunk = 0;
    // sharded handles
    bool dist_no_closures = false, dist_halo_p2p = false;
    // view-graphs
    bool no_resident = false, window_stamps = false;
    long resident_min_edges = 20000;  // below: the host build of the general path (build.cpp) is the faster one
    // prints
    bool build_timing = false, rotavg_timing = false;
};

inline Switches read_switches() {
    Switches s;
    auto set = [](const char *name) { return std::getenv(name) != nullptr; };
    auto num = [](const char *name, int unset) {
        const char *e = std::getenv(name);
        return e ? std::atoi(e) : unset;
    };
    s.has_band_direct = set("IROTAVG_BAND_DIRECT");
    s.band_direct = num("IROTAVG_BAND_DIRECT", 0);
    s.host_build = set("IROTAVG_HOST_BUILD") ? (num("IROTAVG_HOST_BUILD", 0) != 0 ? 1 : 0) : -1;
    s.upload_threads = std::min(4, std::max(0, num("IROTAVG_UPLOAD_THREADS", 4)));
    s.asm_classic = set("IROTAVG_ASM_CLASSIC");
    s.no_small_tuning = set("IROTAVG_NO_SMALL_TUNING");
    s.no_dense_refine = set("IROTAVG_NO_DENSE_REFINE");
    s.no_band_inverse = set("IROTAVG_NO_BAND_INVERSE");
    s.pcg_trace = set("IROTAVG_PCG_TRACE");
    s.cg2_giveup = set("IROTAVG_CG2_GIVEUP") ? std::max(1, num("IROTAVG_CG2_GIVEUP", 0)) : 0;
    s.no_settle = set("IROTAVG_NO_SETTLE");
    s.no_fused_cl = set("IROTAVG_NO_FUSED_CL");
    s.inexact = set("IROTAVG_INEXACT") ? (num("IROTAVG_INEXACT", 0) != 0 ? 1 : 0) : -1;
    s.bcr_no_mixed = set("IROTAVG_BCR_NO_MIXED");
    s.bcr_no_top16 = set("IROTAVG_BCR_NO_TOP16");
    s.bcr_fake_up_fail = set("IROTAVG_BCR_FAKE_UP_FAIL");
    s.bcr_fake_give_up = set("IROTAVG_BCR_FAKE_GIVE_UP");
    s.bcr_no_closures = set("IROTAVG_BCR_NO_CLOSURES");
    s.bcr_s_tiles = set("IROTAVG_BCR_S_TILES");
    s.bcr_no_fused_asm = set("IROTAVG_BCR_NO_FUSED_ASM");
    s.bcr_no_unit_factor = set("IROTAVG_BCR_NO_UNIT_FACTOR");
    s.bcr_up_cap = num("IROTAVG_BCR_UP_CAP", 1024);
    s.bcr_dbg = num("IROTAVG_BCR_DBG", 0);
    s.bcr_stamp_chunk = num("IROTAVG_BCR_STAMP_CHUNK", 0);
    s.dist_no_closures = set("IROTAVG_DIST_NO_CLOSURES");
    s.dist_halo_p2p = set("IROTAVG_DIST_HALO_P2P");
    s.no_resident = set("IROTAVG_NO_RESIDENT");
    s.window_stamps = set("IROTAVG_WINDOW_STAMPS");
    if (const char *e = std::getenv("IROTAVG_RESIDENT_MIN_EDGES")) s.resident_min_edges = std::atol(e);
    s.build_timing = set("IROTAVG_BUILD_TIMING");
    s.rotavg_timing = set("IROTAVG_ROTAVG_TIMING");
    return s;
}

// (the one-shot entry points: a kept handle serves a call only under the switches it was made with)
inline bool operator==(const Switches &a, const Switches &b) {
    auto t = [](const Switches &s) {
        return std::make_tuple(
            s.has_band_direct, s.band_direct, s.host_build, s.upload_threads, s.asm_classic, s.no_small_tuning,
            s.no_dense_refine, s.no_band_inverse, s.pcg_trace, s.cg2_giveup, s.no_settle, s.no_fused_cl, s.inexact,
            s.bcr_no_mixed, s.bcr_no_top16, s.bcr_fake_up_fail, s.bcr_fake_give_up, s.bcr_no_closures, s.bcr_s_tiles,
            s.bcr_no_fused_asm, s.bcr_no_unit_factor, s.bcr_up_cap, s.bcr_dbg, s.bcr_stamp_chunk, s.dist_no_closures, s.dist_halo_p2p, s.no_resident, s.window_stamps,
            s.resident_min_edges, s.build_timing, s.rotavg_timing);
    };
    return t(a) == t(b);
}

// ---- process-wide: read by singletons, not by handles ----------------------------------------------------------------
// the device pool's cache limit in MiB as text (nullptr: not set); read when the pool is made, at the first allocation
inline const char *env_pool_limit_mb() { return std::getenv("IROTAVG_POOL_LIMIT_MB"); }
// pinned blocks without the mapped + coherent flags; latched by the pinned pool at its first allocation
inline bool env_pin_default() { return std::getenv("IROTAVG_PIN_DEFAULT") != nullptr; }
// small read-backs by copy + wait instead of polling a pinned word; latched at the first such read-back
inline bool env_no_poll() { return std::getenv("IROTAVG_NO_POLL") != nullptr || env_pin_default(); }
// the one-shot calls keep their last handle unless this is 0; latched at the first one, irotavg_oneshot_cache() overrides
inline bool env_oneshot_cache() {
    const char *e = std::getenv("IROTAVG_ONESHOT_CACHE");
    return !(e && std::atoi(e) == 0);
}
// host threads of parallel_for, 1 .. 16; 0: not set. Read at EVERY call: parallel_for also runs outside any handle (the
// one-shot content hash) and the thread-count test changes it between builds
inline int env_build_threads() {
    const char *e = std::getenv("IROTAVG_BUILD_THREADS");
    return e ? std::min(16, std::max(1, std::atoi(e))) : 0;
}

}  // namespace irh
