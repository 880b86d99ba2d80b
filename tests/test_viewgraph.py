"""The ViewGraph / Pose counterpart (irotavg_viewgraph_*): container semantics on the CPU, and
rotAvg against the oracle's literal restatement of src/ViewGraph.cpp:1263-1435 on the GPU."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

from irotavg_amd import capi, synth
from irotavg_amd.viewgraph import ViewGraph
from oracle import oracle as O
from oracle.viewgraph_oracle import ViewGraphOracle


def rot(q):
    return O.quat2rmat(np.asarray(q, dtype=np.float64))


def test_container_semantics_without_gpu():
    vg = ViewGraph()
    a, b, c = vg.addView(), vg.addView(rot([0, 0, np.sin(.1), np.cos(.1)])), vg.addView()
    assert (a, b, c) == (0, 1, 2) and vg.numViews() == 3
    np.testing.assert_array_equal(vg.R(0), np.eye(3))            # Pose() default
    assert vg.connect(0, 1, np.eye(3)) is True
    assert vg.connect(1, 0, np.eye(3)) is False                   # View::connect refuses duplicates
    with pytest.raises(capi.IrotavgError):
        vg.connect(1, 1, np.eye(3))
    assert vg.countFixedPoses() == 0 and not vg.isPoseFixed(1)
    R = rot([0.1, 0.2, 0.3, 0.9])
    vg.fixPose(1, R)                                              # sets the pose AND the mask
    assert vg.isPoseFixed(1) and vg.countFixedPoses() == 1
    np.testing.assert_array_equal(vg.R(1), R)
    with pytest.raises(capi.IrotavgError):
        vg.rotAvg(2)                                              # assert(winSize > 2)
    # early-outs of rotAvg never reach the GPU
    assert vg.rotAvg(10)["skipped"] == 2                          # 1 edge < winSize 3
    one = ViewGraph(); one.addView()
    assert one.rotAvg(10)["skipped"] == 1


def test_pose_conversions_and_save_poses(tmp_path):
    from irotavg_amd.viewgraph import quat2rmat, rmat2quat
    rng = np.random.default_rng(0)
    qs = list(rng.normal(size=(20, 4))) + [np.array([1, .01, .02, .01]), np.array([.01, 1, .02, .01]),
                                           np.array([.01, .02, 1, .01])]
    for q in qs:
        q = q / np.linalg.norm(q)
        np.testing.assert_array_equal(quat2rmat(q), O.quat2rmat(q))          # same statements as the oracle
        np.testing.assert_array_equal(rmat2quat(O.quat2rmat(q)), O.rmat2quat(O.quat2rmat(q)))
    vg = ViewGraph()
    Rs = [O.quat2rmat(q / np.linalg.norm(q)) for q in qs[:3]]
    for R in Rs:
        vg.addView(R)
    t = np.arange(9, dtype=np.float64).reshape(3, 3)
    vg.savePoses(tmp_path / "rotavg_poses.txt", t)
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "rotavg_poses.txt")]
    assert [int(r[0]) for r in rows] == [0, 1, 2] and all(len(r) == 8 for r in rows)
    for v, r in enumerate(rows):
        q = O.rmat2quat(Rs[v])
        np.testing.assert_allclose([float(x) for x in r[1:5]], [q[3], q[0], q[1], q[2]], rtol=1e-15)
        np.testing.assert_array_equal([float(x) for x in r[5:]], t[v])
        assert "e" in r[1]                                                    # std::scientific


def build_sequence(n, seed, k_prev=4, n_loops=6, noise=0.01):
    """A small SLAM-like stream: each view linked to up to k_prev predecessors + a few loop closures."""
    rng = np.random.default_rng(seed)
    Qgt = rng.normal(size=(n, 4)); Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    edges = []
    for j in range(1, n):
        for d in range(1, min(k_prev, j) + 1):
            edges.append((j - d, j))
    for _ in range(n_loops):
        a, b = sorted(rng.choice(n, size=2, replace=False))
        if b - a > k_prev:
            edges.append((a, b))
    rel = {}
    for (i, j) in edges:
        e = synth.qexp(rng.normal(scale=noise, size=(1, 3)))[0]
        rel[(i, j)] = rot(synth.qmul(e, synth.qmul(Qgt[j], synth.qconj(Qgt[i]))))
    return Qgt, rel


@pytest.mark.gpu
@pytest.mark.parametrize("win", [10, 5000000])
def test_rotavg_matches_oracle(win):
    n = 40
    Qgt, rel = build_sequence(n, seed=7)
    vg, vo = ViewGraph(), ViewGraphOracle()
    rng = np.random.default_rng(1)
    for v in range(n):
        # initial poses: ground truth perturbed by ~0.05 rad (what the front-end would hand over)
        R0 = rot(synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(1, 3)))[0], Qgt[v]))
        vg.addView(R0); vo.addView(R0)
    for (i, j), R in rel.items():
        assert vg.connect(i, j, R) == vo.connect(i, j, R)
    for idx in (0, 20, 35):                                        # GT corrections (src/IRotAvg.cpp:360-368)
        vg.fixPose(idx, rot(Qgt[idx])); vo.fixPose(idx, rot(Qgt[idx]))
    a, b = vg.rotAvg(win), vo.rotAvg(win)
    assert a["skipped"] == b["skipped"] == 0
    assert (a["n_views"], a["n_edges"], a["n_fixed"]) == (b["n_views"], b["n_edges"], b["n_fixed"])
    assert (a["l1_iters"], a["irls_iters"]) == (b["l1_iters"], b["irls_iters"])
    for v in range(n):
        np.testing.assert_allclose(vg.R(v), vo.R[v], atol=1e-8)
    for idx in (0, 20, 35):
        np.testing.assert_array_equal(vg.R(idx), rot(Qgt[idx]))   # fixed poses untouched
    if win >= n:
        err = [synth.angular_distance(O.rmat2quat(vg.R(v)), Qgt[v]) for v in range(n)]
        assert max(err) < 0.05


@pytest.mark.gpu
def test_incremental_stream_matches_oracle():
    """Config-5 call pattern (src/IRotAvg.cpp:360-378): local rotAvg(10) per admitted view, global
    re-solve when a loop closure arrives, a ground-truth fix every 20 frames."""
    n = 60
    Qgt, rel = build_sequence(n, seed=11, n_loops=5)
    vg, vo = ViewGraph(), ViewGraphOracle()
    by_new = {}
    for (i, j), R in rel.items():
        by_new.setdefault(j, []).append((i, R))
    for v in range(n):
        # the front-end's initial pose of a new view: chain the first relative rotation
        if v == 0:
            R0 = rot(Qgt[0])
        else:
            i, R = sorted(by_new[v], key=lambda t: -t[0])[0]
            R0 = R @ vo.R[i]
        vg.addView(R0); vo.addView(R0)
        loop = False
        for (i, R) in by_new.get(v, []):
            vg.connect(i, v, R); vo.connect(i, v, R)
            loop = loop or (v - i > 4)
        if v % 20 == 0:
            vg.fixPose(v, rot(Qgt[v])); vo.fixPose(v, rot(Qgt[v]))
        a = vg.rotAvg(5000000 if loop else 10)
        b = vo.rotAvg(5000000 if loop else 10)
        assert a["skipped"] == b["skipped"]
        if not a["skipped"]:
            assert (a["n_views"], a["n_fixed"], a["l1_iters"], a["irls_iters"]) == \
                   (b["n_views"], b["n_fixed"], b["l1_iters"], b["irls_iters"]), (v, a, b)
    for v in range(n):
        np.testing.assert_allclose(vg.R(v), vo.R[v], atol=1e-7)


@pytest.mark.gpu
def test_connect_with_swapped_arguments_stores_the_transpose():
    """irotavg_viewgraph_connect(j, i, R_ji) with j > i is the same constraint as connect(i, j, R_ji^T)
    (the reference only ever calls connect(prev, curr), src/ViewGraph.cpp:1438-1455)."""
    n = 30
    Qgt, rel = build_sequence(n, seed=3)
    a, b = ViewGraph(), ViewGraph()
    rng = np.random.default_rng(5)
    for v in range(n):
        R0 = rot(synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(1, 3)))[0], Qgt[v]))
        a.addView(R0); b.addView(R0)
    for k, ((i, j), R) in enumerate(rel.items()):
        a.connect(i, j, R)
        if k % 2:
            b.connect(j, i, R.T)
        else:
            b.connect(i, j, R)
    a.fixPose(0, rot(Qgt[0])); b.fixPose(0, rot(Qgt[0]))
    ra, rb = a.rotAvg(5000000), b.rotAvg(5000000)
    assert (ra["l1_iters"], ra["irls_iters"]) == (rb["l1_iters"], rb["irls_iters"])
    for v in range(n):
        np.testing.assert_allclose(a.R(v), b.R(v), atol=1e-12)


_STREAM_POSES = {}


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["resident", "rebuild"])
def test_incremental_stream_with_loop_closures_at_scale_matches_oracle(path, monkeypatch):
    """Config 5's call pattern at a size the oracle still covers: 2000 warm views, 1200 streamed one by
    one (rotAvg(10) each -- the single-launch window kernel), 3 loop closures (global re-solves through
    the multi-level handle path), a ground-truth fix every 20 frames. Every call's bookkeeping and
    iteration counts equal the oracle's, and so do the final poses. Both forms of the global re-solve: on the
    device-resident growing copy of the graph (resident.hip; its size threshold lowered to reach it here) and by
    extracting and rebuilding the whole problem per call -- with bit-identical poses."""
    if path == "resident":
        monkeypatch.setenv("IROTAVG_RESIDENT_MIN_EDGES", "1000")
    else:
        monkeypatch.setenv("IROTAVG_NO_RESIDENT", "1")
    warm, stream, n_loops = 2000, 1200, 3
    n = warm + stream
    rng = np.random.default_rng(21)
    Qgt = rng.normal(size=(n, 4)); Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)

    def relR(i, j):
        e = synth.qexp(rng.normal(scale=0.01, size=(1, 3)))[0]
        return rot(synth.qmul(e, synth.qmul(Qgt[j], synth.qconj(Qgt[i]))))
    vg, vo = ViewGraph(), ViewGraphOracle()
    for v in range(warm):        # a converged history: ground truth perturbed at the noise level
        R0 = rot(synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(1, 3)))[0], Qgt[v]))
        vg.addView(R0); vo.addView(R0)
        for d in range(1, min(4, v) + 1):
            R = relR(v - d, v)
            vg.connect(v - d, v, R); vo.connect(v - d, v, R)
        if v % 20 == 0:
            vg.fixPose(v, rot(Qgt[v])); vo.fixPose(v, rot(Qgt[v]))
    loop_at = set(rng.choice(np.arange(warm + 50, n), size=n_loops, replace=False).tolist())
    n_global = 0
    for v in range(warm, n):
        R1 = relR(v - 1, v)
        R0 = R1 @ vo.R[v - 1]
        vg.addView(R0); vo.addView(R0)
        vg.connect(v - 1, v, R1); vo.connect(v - 1, v, R1)
        for d in range(2, 5):
            R = relR(v - d, v)
            vg.connect(v - d, v, R); vo.connect(v - d, v, R)
        loop = v in loop_at
        if loop:
            u = int(rng.integers(0, v - 500))
            R = relR(u, v)
            vg.connect(u, v, R); vo.connect(u, v, R)
        if v % 20 == 0:
            vg.fixPose(v, rot(Qgt[v])); vo.fixPose(v, rot(Qgt[v]))
        a, b = vg.rotAvg(5000000 if loop else 10), vo.rotAvg(5000000 if loop else 10)
        n_global += 1 if loop else 0
        assert a["skipped"] == b["skipped"] == 0
        assert (a["n_views"], a["n_edges"], a["n_fixed"], a["l1_iters"], a["irls_iters"]) == \
               (b["n_views"], b["n_edges"], b["n_fixed"], b["l1_iters"], b["irls_iters"]), (v, loop, a, b)
    assert n_global == n_loops
    worst = max(np.abs(vg.R(v) - vo.R[v]).max() for v in range(n))
    assert worst < 1e-6, worst
    err = [synth.angular_distance(O.rmat2quat(vg.R(v)), Qgt[v]) for v in range(warm, n, 13)]
    assert max(err) < 0.05
    _STREAM_POSES[path] = np.stack([vg.R(v) for v in range(n)])
    if len(_STREAM_POSES) == 2:
        np.testing.assert_array_equal(_STREAM_POSES["resident"], _STREAM_POSES["rebuild"])


@pytest.mark.gpu
def test_resident_global_resolves_equal_rebuilt_ones_bit_for_bit(monkeypatch):
    """The device-resident growing graph (resident.hip) at its default size threshold: a 6000-view
    sequence with global re-solves between which the graph changes in every way the API allows -- views appended
    with their links (the append-only case), sliding windows moving the newest poses, a view fixed long after it
    was admitted, a pose overwritten by the caller, a loop closure between two OLD views (its record lands in the
    middle of the resident edge list) -- gives bit-identical poses and identical bookkeeping to the path that
    extracts, relabels and rebuilds the whole problem on every call."""
    n0, extra = 6000, 260
    rng = np.random.default_rng(5)
    Qgt = rng.normal(size=(n0 + extra, 4)); Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    noise = rng.normal(scale=0.01, size=(8 * (n0 + extra), 3))
    script = []      # (op, args) replayed on both graphs

    def rel(i, j, k):
        return rot(synth.qmul(synth.qexp(noise[k:k + 1])[0], synth.qmul(Qgt[j], synth.qconj(Qgt[i]))))
    k = 0
    for v in range(n0 + extra):
        script.append(("add", v, rot(synth.qmul(synth.qexp(noise[k:k + 1] * 2)[0], Qgt[v])))); k += 1
        for d in range(1, min(4, v) + 1):
            script.append(("connect", v - d, v, rel(v - d, v, k))); k += 1
        if v % 20 == 0:
            script.append(("fix", v, rot(Qgt[v])))
        if v >= n0:
            script.append(("avg", 10))
        if v == n0 - 1:
            script.append(("prepare",))                            # dry run: nothing may change
            script.append(("avg", 5000000))                        # first global solve: everything goes up
        if v == n0 + 40:
            script.append(("connect", 100, v, rel(100, v, k))); k += 1  # loop closure at the newest view
            script.append(("avg", 5000000))
        if v == n0 + 90:
            script.append(("fix", 3001, rot(Qgt[3001])))          # an old view becomes fixed: every row behind it moves
            script.append(("avg", 5000000))
        if v == n0 + 150:
            script.append(("set", 4000, rot(Qgt[4000])))           # the caller overwrites an old pose
            script.append(("connect", 700, 5200, rel(700, 5200, k))); k += 1   # closure between two old views
            script.append(("avg", 5000000))
        if v == n0 + 151:
            script.append(("avg", 5000000))                        # nothing but one view changed
    # second phase: the graph grows past the capacity of the resident arrays (half as much again as the first call
    # needed) and collects 150 loop closures between old views -- more than one LDS system holds, and their records
    # land all over the resident edge list
    n1 = n0 + extra
    more = 3900
    Qgt2 = rng.normal(size=(more, 4)); Qgt2 /= np.linalg.norm(Qgt2, axis=1, keepdims=True)
    Qgt = np.concatenate([Qgt, Qgt2])
    noise = np.concatenate([noise, rng.normal(scale=0.01, size=(8 * more + 400, 3))])
    for v in range(n1, n1 + more):
        script.append(("add", v, rot(synth.qmul(synth.qexp(noise[k:k + 1] * 2)[0], Qgt[v])))); k += 1
        for d in range(1, 5):
            script.append(("connect", v - d, v, rel(v - d, v, k))); k += 1
        if v % 20 == 0:
            script.append(("fix", v, rot(Qgt[v])))
        if v % 500 == 0:
            script.append(("avg", 10))
    cl = rng.integers(0, n1 + more - 200, size=(150, 2))
    for a, b in cl:
        a, b = int(min(a, b)), int(max(a, b))
        if b - a > 100:
            script.append(("connect", a, b, rel(a, b, k))); k += 1
    script.append(("avg", 5000000))
    n_all = n1 + more
    out = {}
    for path in ("resident", "rebuild"):
        if path == "rebuild":
            monkeypatch.setenv("IROTAVG_NO_RESIDENT", "1")
        vg = ViewGraph()
        infos = []
        for op in script:
            if op[0] == "add":
                vg.addView(op[2])
            elif op[0] == "connect":
                vg.connect(op[1], op[2], op[3])
            elif op[0] == "fix":
                vg.fixPose(op[1], op[2])
            elif op[0] == "set":
                vg.setR(op[1], op[2])
            elif op[0] == "prepare":
                before = np.stack([vg.R(v) for v in range(0, n0, 7)])
                vg.prepare()
                np.testing.assert_array_equal(before, np.stack([vg.R(v) for v in range(0, n0, 7)]))
            else:
                a = vg.rotAvg(op[1])
                if op[1] > 10:
                    infos.append((a["skipped"], a["n_views"], a["n_edges"], a["n_fixed"], a["l1_iters"], a["irls_iters"]))
        out[path] = (infos, np.stack([vg.R(v) for v in range(n_all)]))
    assert len(out["resident"][0]) == 6 and all(i[0] == 0 for i in out["resident"][0])
    assert out["resident"][0][-1][1] == n_all and out["resident"][0][-1][2] > 4 * n_all + 100
    assert out["resident"][0] == out["rebuild"][0]
    np.testing.assert_array_equal(out["resident"][1], out["rebuild"][1])
    err = synth.angular_distance(np.stack([O.rmat2quat(R) for R in out["resident"][1][::17]]), Qgt[::17])
    assert err.max() < 0.05


@pytest.mark.gpu
def test_config5_full_size_stream_properties():
    """BASELINE.json config 5 at FULL size (50k warm + 50k streamed views, 10 loop closures; the oracle
    cannot follow at this size): the stream completes, every pose stays a rotation, user-fixed poses
    are untouched, and the streamed poses stay within the drift a sequence with fixes every 20 frames
    allows (mean angular error vs ground truth < 0.02 rad). Rate and latencies are printed."""
    import json
    import subprocess
    import sys as _sys
    tool = os.path.join(os.path.dirname(HERE), "tools", "bench_incremental.py")
    r = subprocess.run([_sys.executable, tool, "--warm", "50000", "--stream", "50000", "--loops", "10"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    print(line)
    assert d["streamed_views"] == 50000 and d["loop_closures"] == 10
    assert d["mean_angular_error_rad"] < 0.02 and d["max_angular_error_rad"] < 0.2
    assert d["views_per_s"] > 1000.0


@pytest.mark.gpu
def test_batched_rotavg_over_independent_graphs_equals_separate_calls():
    """irotavg_viewgraph_rot_avg_batch: S view-graphs (different sequences, different lengths, one of them with a
    loop closure whose global re-solve does not fit the window kernel) advanced in lock-step -- one launch per step for
    all the windows -- give bit-for-bit the poses and iteration counts of S graphs advanced by separate rotAvg calls;
    one of the sessions is also held against the oracle."""
    from irotavg_amd.viewgraph import rotAvgBatch
    S, n = 7, 45
    seqs = [build_sequence(n + 3 * s, seed=20 + s, n_loops=(2 if s == 3 else 0)) for s in range(S)]
    A = [ViewGraph() for _ in range(S)]      # batched
    B = [ViewGraph() for _ in range(S)]      # one by one
    vo = ViewGraphOracle()                   # session 0
    by_new = []
    for Qgt, rel in seqs:
        d = {}
        for (i, j), R in rel.items():
            d.setdefault(j, []).append((i, R))
        by_new.append(d)
    for v in range(n + 3 * (S - 1)):
        active = [s for s in range(S) if v < n + 3 * s]
        loops = {}
        for s in active:
            Qgt, rel = seqs[s]
            if v == 0:
                R0 = rot(Qgt[0])
            else:
                i, R = sorted(by_new[s][v], key=lambda t: -t[0])[0]
                R0 = R @ B[s].R(i)
            for G in (A[s], B[s]) + ((vo,) if s == 0 else ()):
                G.addView(R0)
            loop = False
            for (i, R) in by_new[s].get(v, []):
                for G in (A[s], B[s]) + ((vo,) if s == 0 else ()):
                    G.connect(i, v, R)
                loop = loop or (v - i > 4)
            if v % 20 == 0:
                for G in (A[s], B[s]) + ((vo,) if s == 0 else ()):
                    G.fixPose(v, rot(Qgt[v]))
            loops[s] = loop
        # sessions with a loop closure take the global re-solve on their own, the others share one launch
        for s in active:
            if loops[s]:
                ia, ib = A[s].rotAvg(5000000), B[s].rotAvg(5000000)
                assert (ia["l1_iters"], ia["irls_iters"]) == (ib["l1_iters"], ib["irls_iters"])
        rest = [s for s in active if not loops[s]]
        infos = rotAvgBatch([A[s] for s in rest], 10)
        for s, ia in zip(rest, infos):
            ib = B[s].rotAvg(10)
            assert ia["skipped"] == ib["skipped"]
            if not ia["skipped"]:
                assert (ia["n_views"], ia["n_edges"], ia["n_fixed"], ia["l1_iters"], ia["irls_iters"]) == \
                       (ib["n_views"], ib["n_edges"], ib["n_fixed"], ib["l1_iters"], ib["irls_iters"]), (v, s, ia, ib)
        if 0 in active:
            vo.rotAvg(5000000 if loops[0] else 10)
    for s in range(S):
        for v in range(n + 3 * s):
            np.testing.assert_array_equal(A[s].R(v), B[s].R(v))
    for v in range(n):
        np.testing.assert_allclose(A[0].R(v), vo.R[v], atol=1e-7)
    # the same graph twice in one batch is refused: its windows depend on each other
    with pytest.raises(capi.IrotavgError):
        rotAvgBatch([A[0], A[0]], 10)


@pytest.mark.gpu
def test_batched_rotavg_staging_grows_and_is_reused():
    """irotavg_viewgraph_rot_avg_batch with 2, then 5, then the first 2 sessions again (three views, the first fixed, three
    connections with 0.01 rad of noise; the poses put back before every call): the staging of the first session's window
    solver is replaced by a larger block for the second call and reused by the third. The first and the third call give
    the same bits, and each of the five sessions of the second the bits of its own rotAvg(10)."""
    from irotavg_amd.viewgraph import rotAvgBatch
    S = 5
    seqs = [build_sequence(3, seed=70 + s, n_loops=0) for s in range(S)]
    rng = np.random.default_rng(3)
    R0 = [[rot(synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(1, 3)))[0], Qgt[v])) if v else rot(Qgt[0])
           for v in range(3)] for Qgt, _ in seqs]

    def session(s):
        G = ViewGraph()
        for v in range(3):
            G.addView(R0[s][v])
        for (i, j), R in seqs[s][1].items():
            assert G.connect(i, j, R)
        G.fixPose(0, R0[s][0])
        return G

    def batch(graphs):
        for s, G in enumerate(graphs):
            for v in (1, 2):
                G.setR(v, R0[s][v])
        infos = rotAvgBatch(graphs, 10)
        for i in infos:
            assert (i["skipped"], i["n_views"], i["n_edges"], i["n_fixed"]) == (0, 3, 3, 1), i
        return ([(i["l1_iters"], i["irls_iters"]) for i in infos],
                np.stack([G.R(v) for G in graphs for v in range(3)]))

    A = [session(s) for s in range(S)]
    first, many, third = batch(A[:2]), batch(A), batch(A[:2])
    assert first[0] == third[0] and first[1].tobytes() == third[1].tobytes()
    assert many[0][:2] == first[0] and many[1][:6].tobytes() == first[1].tobytes()
    for s in range(S):
        B = session(s)
        ib = B.rotAvg(10)
        assert (ib["skipped"], ib["n_views"], ib["n_edges"], ib["n_fixed"]) == (0, 3, 3, 1), ib
        assert many[0][s] == (ib["l1_iters"], ib["irls_iters"])
        assert many[1][3 * s:3 * s + 3].tobytes() == np.stack([B.R(v) for v in range(3)]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3000, 6000])
def test_global_rotavg_falls_back_to_the_iterative_solver_when_the_direct_one_gives_up(n, monkeypatch):
    """ViewGraph::rotAvg has one code path for every graph (src/ViewGraph.cpp:1400-1417 over ral/l1_irls.cpp:536-556).
    Here a global re-solve of a sequence with loop closures runs on the banded direct solver; when that solver gives a
    system up (IROTAVG_ERR_SOLVER from irls: a band part next to singular under the closures -- forced here by
    IROTAVG_BCR_FAKE_GIVE_UP), the call repeats on the iterative solver by itself: the general path (3000 views) and the
    device-resident one (6000 views: above 20000 connections), same poses as the undisturbed call."""
    Qgt, rel = build_sequence(n, seed=5, n_loops=12)
    res = []
    for fake in (False, True):
        if fake:
            monkeypatch.setenv("IROTAVG_BCR_FAKE_GIVE_UP", "1")
        vg = ViewGraph()
        rng = np.random.default_rng(1)
        for v in range(n):
            vg.addView(rot(synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(1, 3)))[0], Qgt[v])))
        for (i, j), R in rel.items():
            vg.connect(i, j, R)
        for idx in range(0, n, 500):
            vg.fixPose(idx, rot(Qgt[idx]))
        a = vg.rotAvg(5000000)
        assert a["skipped"] == 0 and a["n_views"] == n
        res.append((a, np.stack([vg.R(v) for v in range(n)])))
    assert res[0][0]["irls_iters"] == res[1][0]["irls_iters"]
    np.testing.assert_allclose(res[0][1], res[1][1], atol=1e-7)
