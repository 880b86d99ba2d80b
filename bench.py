#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's config.

metric : IRLS edge-updates/s (= m * IRLS iterations / wall time of the `irls` call, inputs
         resident in HBM) + iterations-to-converge, on the synthetic 100k-view / 2M-edge SO(3)
         view-graph (SURVEY.md 8(d) generator, seed 0), Geman-McClure sigma = 5 deg,
         change_th = 1e-3, max_iters = 100 -- the reference's defaults (src/ViewGraph.cpp:1402-1414).
step   : one complete `irls` solve of that graph from its `init_mst` initialisation (rotations
         restored on the device before every step; the restore is inside the timed region).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--p-loop P] [--views n] [--edges m]
                    [--dump-outputs DIR] [--full]

For N > 1 the driver launches one process per GPU through torch.distributed.run; rank 0 prints
ONE JSON line. A plain run sets up, warms up, times the K steps and prints the headline line
(`ms_per_step` = milliseconds per timed step). --dump-outputs DIR writes what the last timed step
computed (rotations, weights, score trace) as DIR/<name>.npy. With --full the line also carries
`roofline` (dominant kernel + the edge-residual kernel the north star names, HIP-event timed on
the handle's stream), the `also_*` legs, the sharded run's phase timing and its check against one
GPU, and `cpu_baseline` (the CPU oracle -- a port, not Eigen+SuiteSparse -- on a bounded sample).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIG = 5 * np.pi / 180
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def build_problem(n, m, p_loop, seed):
    from irotavg_amd import ral, synth
    S = synth.make_graph(n, m, p_loop, seed=seed)
    Q0 = np.zeros((n, 4))
    Q0[:, 3] = 1
    Q0[0] = S["Qgt"][0]
    ral.init_mst(Q0, S["QQ"], S["I"], 1)   # host, outside the timed region (as in the reference)
    return S, Q0


def kernel_rooflines(G, S, st, sharded=False):
    """HIP-event timed kernels -> algorithmic GB/s (formulas: SURVEY.md 8(d))."""
    from irotavg_amd import capi
    m, n_t = S["m"], S["n"]
    nu = n_t - 1
    nnz0 = st["level_nnz"][0]
    alg = {
        "edge_residual": m * (8 + 32 + 24) + 32 * n_t,
        "update_weights": m * (8 + 24 + 8) + 24 * nu,
        "assemble": m * (8 + 8 + 24) + nu * (8 + 24) + 8 * nnz0,
        "spmv": nnz0 * (8 + 4) + 4 * (nu + 1) + 2 * 24 * nu,
    }
    which = {"edge_residual": 1, "update_weights": 2, "assemble": 3, "spmv": 4}
    if not sharded:
        # K2 and the next iteration's K1 as one kernel (the direct solver's irls loop; solver.hip, k_weights_then_residual)
        alg["weights_then_residual"] = m * (8 + 24 + 8 + 32 + 24) + 32 * n_t + 24 * nu
        which["weights_then_residual"] = 11
    out = {}
    di = G.direct_info() if not sharded else dict(block=0, levels=[])
    if di["block"]:
        # the handle's systems are solved by the banded direct solver (bcr.hip): its launches instead of the PCG's
        del which["spmv"]
        alg["assemble"] = m * (8 + 8 + 24) + nu * (8 + 24) + 8 * nnz0   # level 0 only: same formula, no coarse level
    for name, w in which.items():
        ms = G.time_kernel(w, 50)
        out[name] = dict(ms=ms, bytes=alg[name], gbs=alg[name] / (ms * 1e-3) / 1e9)
    if di["block"]:
        B = di["block"]
        NC = 2 * B + 3
        lev = di["levels"]
        nl = len(lev)
        tot_ms, tot_by, tot_fl = 0.0, 0, 0
        back_upper = 0   # the ways back of the levels >= 1 are ONE launch (k_bcr_back_top), timed as 40 + 1
        for l, L in enumerate(lev):
            top = l == nl - 1
            elim = sum(min(7, max(0, L["blocks"] - 8 * c)) for c in range(L["chunks"]))   # blocks eliminated
            wbytes = 8 * elim * B * NC
            sep = 0 if top else 8 * L["chunks"] * (3 * B * B + 6 * B)
            if l == 0:
                rd = nnz0 * (8 + 4) + 4 * (nu // 64 + 2) + nu * (8 + 32)    # SELL entries, slice offsets, diagonal, rhs
            else:
                P = lev[l - 1]
                rd = 8 * P["chunks"] * (3 * B * B + 6 * B)
                if L["reduced"] < L["blocks"]:   # mixed level 1: the level-0 rows no chunk reduced
                    raw = (L["blocks"] - L["reduced"]) * B
                    rd += int(nnz0 * (8 + 4) * raw / max(nu, 1)) + raw * (8 + 32)
            # flops issued on useful entries: D^-1 (2 B^3), W = D^-1 [P' Q R], P W, Q' W_QR
            fl = elim * (2 * B ** 3 + 2 * B * B * NC * 2 + 2 * B * B * (B + 3))
            ms = G.time_kernel(20 + l, 50)
            out["bcr_reduce_l%d" % l] = dict(ms=ms, bytes=rd + wbytes + sep, gbs=(rd + wbytes + sep) / (ms * 1e-3) / 1e9,
                                             flops=fl, tflops=fl / (ms * 1e-3) / 1e12, workgroups=L["chunks"])
            bb = wbytes + 8 * (L["chunks"] * 8 * B * 3) + (32 * nu if l == 0 else 0)
            tot_ms += ms
            tot_by += rd + wbytes + sep + bb
            tot_fl += fl
            if l == 0 or nl < 2:
                msb = G.time_kernel(40 + l, 50)
                out["bcr_back_l%d" % l] = dict(ms=msb, bytes=bb, gbs=bb / (msb * 1e-3) / 1e9, workgroups=L["chunks"])
                tot_ms += msb
            else:
                back_upper += bb
        if nl >= 2:
            msb = G.time_kernel(41, 50)
            out["bcr_back_upper"] = dict(ms=msb, bytes=back_upper, gbs=back_upper / (msb * 1e-3) / 1e9,
                                         workgroups=lev[1]["chunks"], levels="1..%d in one launch (k_bcr_back_top)" % (nl - 1))
            tot_ms += msb
        ms = G.time_kernel(19, 50)
        # the reductions of the levels >= 1 run as ONE launch (k_bcr_reduce_up) under the library's rule: three or more
        # levels, blocks <= 24, no closures (the per-level figures above are separate launches of the same bodies)
        fused_up = nl >= 3 and B <= 24 and di.get("closures", 0) == 0 and lev[1]["chunks"] <= 256
        out["bcr_solve"] = dict(ms=ms, bytes=tot_by, gbs=tot_by / (ms * 1e-3) / 1e9, flops=tot_fl,
                                tflops=tot_fl / (ms * 1e-3) / 1e12,
                                launches=4 if fused_up else nl + (2 if nl >= 2 else 1), fused_upper_reduce=fused_up,
                                sum_of_launches_ms=tot_ms, block=B, levels=lev)
        return out
    try:  # band-only graphs on one GPU run the p-update fused into the SpMV (k_pspmv_dot)
        if sharded:   # the sharded PCG exchanges p between its p-update and its SpMV: unfused kernels
            raise capi.IrotavgError(capi.ERR_BAD_ARG, "sharded")
        ms = G.time_kernel(8, 50)
        by = nnz0 * (8 + 4) + 4 * (nu + 1) + nu * (24 + 24 + 8 + 3 + 24 + 24)
        out["pspmv"] = dict(ms=ms, bytes=by, gbs=by / (ms * 1e-3) / 1e9)
    except capi.IrotavgError:
        pass
    try:  # the two-launch Chronopoulos-Gear iteration (cgcg.hip): band-only graphs with >= 3 levels on one GPU
        if sharded or st["levels"] < 3:
            raise capi.IrotavgError(capi.ERR_BAD_ARG, "not this graph's PCG")
        n1, nd = st["level_rows"][1], st["level_rows"][2]
        nnz1 = st["level_nnz"][1]
        coarse = 2 * 24 * n1 + 12 * nnz1 + 24 * nd + (8 * nd * nd if st["levels"] == 3 else 0)
        ms = G.time_kernel(9, 50)
        # matrix once, r / idg / diag in, u / w out, plus the coarse data every tile slice comes from
        by = nnz0 * (8 + 4) + 4 * (nu + 1) + nu * (24 + 8 + 8 + 24 + 24) + coarse
        out["cg_apply"] = dict(ms=ms, bytes=by, gbs=by / (ms * 1e-3) / 1e9)
        ms = G.time_kernel(10, 50)
        by = nu * 24 * 10 + 2 * 24 * n1 + 12 * nnz1 + 2 * 24 * nd   # r w s u p x in, p s x r out, b1 x1 b2 x2 out
        out["cg_update"] = dict(ms=ms, bytes=by, gbs=by / (ms * 1e-3) / 1e9)
    except capi.IrotavgError:
        pass
    out["precondition"] = dict(ms=G.time_kernel(5, 50))
    out["dense_inversion"] = dict(ms=G.time_kernel(7, 5))
    return out


def live_profile_l1ra(args):
    """the same three rocprofv3 passes on `l1ra` alone (tools/prof_case.py --what l1ra): the kernels of the primal-dual
    iteration in situ -- three solver chains at once -- with their HBM traffic. Returns (table, info) or (None, reason)."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    out = os.path.join(ROOT, "gpurun_out", "bench_profile_l1ra")
    try:
        os.makedirs(out, exist_ok=True)
    except OSError:
        out = tempfile.mkdtemp(prefix="irotavg_bench_profile_l1ra_")
    base = [sys.executable, os.path.join(ROOT, "tools", "prof_case.py"), "--views", str(args.views), "--edges", str(args.edges),
            "--what", "l1ra", "--l1-iters", "5"]
    env = dict(os.environ, TMPDIR="/tmp")
    info = None
    for tag, flags, reps in (("trace", ["--kernel-trace", "--stats"], "4"), ("fetch", ["--pmc", "FETCH_SIZE", "--kernel-trace"], "1"),
                             ("write", ["--pmc", "WRITE_SIZE", "--kernel-trace"], "1")):
        d = os.path.join(out, tag)
        shutil.rmtree(d, ignore_errors=True)
        cmd = ["rocprofv3"] + flags + ["--output-format", "csv", "-d", d, "-o", tag[0], "--"] + base + ["--reps", reps]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
        except Exception as e:
            return None, "rocprofv3 %s pass: %s" % (tag, e)
        if r.returncode != 0:
            return None, "rocprofv3 %s pass exited with %d" % (tag, r.returncode)
        if tag == "trace":
            try:
                info = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            except Exception:
                info = None
    try:
        from tools.summarize_pmc import summarize
        table = summarize(out)
    except Exception as e:
        return None, "summary failed: %s" % e
    with open(os.path.join(out, "pmc_summary.json"), "w") as fh:
        json.dump(dict(table, _meta=dict(workload="l1ra(5) alone, %d views / %d edges" % (args.views, args.edges), run=info)), fh, indent=1)
    return table, dict(where=out, run=info, trace_reps=6)


def live_profile(args, note):
    """rocprofv3 passes of THIS command (same workload, short run, no extras) launched from inside the bench run:
    kernel trace + stats, then FETCH_SIZE and WRITE_SIZE in their own passes (they do not fit one pass), exactly as
    tools/profile_counters.sh runs them by hand; counters summarised as /opt/skills/guides/MI355X_MICROARCH.md's HBM
    section prescribes (tools/summarize_pmc.py: KiB units, the gfx950 read side doubled). Returns (table, where) --
    table: per kernel {calls, avg_us, traffic_bytes, ...} measured in this run, or None with the reason in `where`.
    The CSVs are kept under gpurun_out/bench_profile/ (the copies the judged profiles/ files are made from)."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    out = os.path.join(ROOT, "gpurun_out", "bench_profile")
    try:
        os.makedirs(out, exist_ok=True)
    except OSError:
        out = tempfile.mkdtemp(prefix="irotavg_bench_profile_")
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--views", str(args.views), "--edges", str(args.edges),
            "--p-loop", str(args.p_loop), "--seed", str(args.seed), "--rtol", str(args.rtol), "--ramp", "3", "--warmup", "1",
            "--no-cpu", "--no-extra", "--no-pmc", "--no-kernels"]
    env = dict(os.environ, TMPDIR="/tmp")
    for tag, flags, steps in (("trace", ["--kernel-trace", "--stats"], "5"), ("fetch", ["--pmc", "FETCH_SIZE", "--kernel-trace"], "2"),
                              ("write", ["--pmc", "WRITE_SIZE", "--kernel-trace"], "2")):
        d = os.path.join(out, tag)
        shutil.rmtree(d, ignore_errors=True)
        cmd = ["rocprofv3"] + flags + ["--output-format", "csv", "-d", d, "-o", tag[0], "--"] + base + ["--steps", steps]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
        except Exception as e:   # a hung rocprofv3 (seen after "tool finalization") must not take the bench line with it
            return None, "rocprofv3 %s pass: %s" % (tag, e)
        with open(os.path.join(out, tag + ".log"), "w") as fh:
            fh.write(r.stdout[-20000:] + "\n" + r.stderr[-20000:])
        if r.returncode != 0:
            return None, "rocprofv3 %s pass exited with %d" % (tag, r.returncode)
    try:
        from tools.summarize_pmc import summarize
        table = summarize(out)
    except Exception as e:
        return None, "summary failed: %s" % e
    with open(os.path.join(out, "pmc_summary.json"), "w") as fh:
        json.dump(dict(table, _meta=dict(workload=note)), fh, indent=1)
    return table, out


def prof_rows(table, kernel, targs=None):
    """rows of the live profile whose kernel is `kernel`; targs: {position: value} on its template arguments"""
    rows = []
    for name, row in (table or {}).items():
        n = name.replace(" ", "")
        base = n.split("<")[0].split("::")[-1]
        if base != kernel:
            continue
        if targs:
            ta = n.split("<", 1)[1].rstrip(">").split(",") if "<" in n else []
            if any(pos >= len(ta) or ta[pos] != val for pos, val in targs.items()):
                continue
        rows.append(row)
    return rows


def prof_value(table, kernel, key, targs=None):
    rows = [r for r in prof_rows(table, kernel, targs) if key in r]
    if not rows:
        return None
    calls = sum(r["calls"] for r in rows)
    return sum(r[key] * r["calls"] for r in rows) / max(calls, 1)   # per launch, averaged over the instantiations


def suitesparse_baseline(S, Q0, budget_s=20.0):
    """if the GPU box has SuiteSparse (it is not in this image), time the reference's
    own library call -- SuiteSparseQR X = A \\ B per IRLS iteration (ral/l1_irls.cpp:536-556) -- through
    oracle/spqr_harness.cpp on the same graph. Returns a dict, or a reason string."""
    import subprocess
    import tempfile
    src = os.path.join(ROOT, "oracle", "spqr_harness.cpp")
    exe = os.path.join(tempfile.gettempdir(), "irotavg_spqr_harness")
    probe = subprocess.run(["g++", "-O2", "-std=c++11", src, "-o", exe, "-I/usr/include/suitesparse", "-lspqr",
                            "-lcholmod", "-lsuitesparseconfig"], capture_output=True, text=True)
    if probe.returncode != 0:
        return "SuiteSparse (SuiteSparseQR.hpp / libspqr) not found on this box: " + \
               (probe.stderr.strip().splitlines() or ["compile failed"])[0][:160]
    from oracle import oracle as O
    w3 = O.log_map(O.delta_rel(S["I"], S["QQ"], Q0))[:, :3]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as fh:
        fh.write("%d %d %d\n" % (S["m"], S["n"], 1))
        for (i, j), r in zip(S["I"], w3):
            fh.write("%d %d %.17g %.17g %.17g\n" % (i, j, r[0], r[1], r[2]))
        path = fh.name
    try:
        out = subprocess.run([exe, path, str(budget_s)], capture_output=True, text=True, timeout=10 * budget_s + 60)
        sec, reps = [float(x) for x in out.stdout.split()[:2]]
        return dict(value=S["m"] * reps / sec, unit="edge-updates/s", cores=1, kind="reference-library",
                    sample="%d SuiteSparseQR least-squares solves (one per IRLS iteration, unit weights) of the same "
                           "%d-view/%d-edge graph, %.1f s" % (int(reps), S["n"], S["m"], sec))
    except Exception as e:
        return "SuiteSparse harness failed: %s" % e
    finally:
        os.unlink(path)


def cpu_baseline(S, Q0, p_loop, budget_s=25.0):
    """The CPU oracle (oracle/, single thread, own sparse Cholesky) on a bounded sample."""
    from oracle import oracle as O
    from irotavg_amd import synth
    cores = 1
    if p_loop == 0.0 or S["m"] <= 200000:
        # the identical workload: complete IRLS solves (to convergence) of the same graph, repeated
        # until ~10 s of CPU time have been spent
        t = time.time()
        updates, runs, iters = 0, 0, 0
        while time.time() - t < 10.0 and runs < 50:
            r = O.irls(S["QQ"], S["I"], Q0, 1, 4, SIG, 100, 1e-3)
            updates += S["m"] * r["iters"]
            iters = r["iters"]
            runs += 1
        dt = time.time() - t
        return dict(value=updates / dt, unit="edge-updates/s", cores=cores, kind="port",
                    sample="%d complete IRLS solves (%d iterations each, incl. symbolic analysis) of the "
                           "same %d-view/%d-edge graph, %.1f s" % (runs, iters, S["n"], S["m"], dt),
                    iters_to_converge=iters,
                    note="oracle = C restatement + own sparse Cholesky; NOT Eigen+SuiteSparse "
                         "(unbuildable here)")
    # loop-closure-rich graphs: fill of the direct factorisation explodes; sample a 10x smaller graph
    n2, m2 = S["n"] // 10, S["m"] // 10
    S2 = synth.make_graph(n2, m2, p_loop, seed=0)
    Q2 = np.zeros((n2, 4)); Q2[:, 3] = 1; Q2[0] = S2["Qgt"][0]
    rc, Q2 = O.init_mst(Q2, S2["QQ"], S2["I"], 1)
    t = time.time()
    r = O.irls(S2["QQ"], S2["I"], Q2, 1, 4, SIG, 1, 1e-3)
    dt = time.time() - t
    return dict(value=S2["m"] * r["iters"] / dt, unit="edge-updates/s", cores=cores, kind="port",
                sample="1 IRLS iteration of a %d-view/%d-edge graph with the same p_loop "
                       "(the full-size factorisation does not finish in minutes), %.1f s" % (n2, m2, dt),
                note="oracle = C restatement + own sparse Cholesky; NOT Eigen+SuiteSparse")


def cpu_baselines_main(spec):
    """`python bench.py --cpu-only '<json>'`: every CPU-oracle baseline of the bench line, in a process of its own (started
    by the bench run behind its timed region: the oracle's Python glue would otherwise take the interpreter lock away
    from the GPU legs, and the GPU stays busy while the host cores are timed). Prints ONE JSON object."""
    from oracle import oracle as O
    from irotavg_amd import synth
    out = {}
    n, m, p_loop, seed = spec["views"], spec["edges"], spec["p_loop"], spec["seed"]
    S, Q0 = build_problem(n, m, p_loop, seed)
    out["cpu_baseline"] = cpu_baseline(S, Q0, p_loop)
    ss = suitesparse_baseline(S, Q0)
    if isinstance(ss, dict):
        out["cpu_baseline_suitesparse"] = ss
    else:
        out["cpu_baseline"]["suitesparse_probe"] = ss
    if spec.get("extras"):
        # the loop-closure topology at FULL size: one IRLS iteration (the oracle's fill test hands such a graph to its
        # Gauss-Seidel-preconditioned CG, true relative residual 1e-13)
        S2, Q2 = build_problem(n, m, 0.02, seed)
        t = time.time()
        r = O.irls(S2["QQ"], S2["I"], Q2, 1, 4, SIG, 1, 1e-3)
        dt = time.time() - t
        out["also_p_loop_0.02"] = dict(value=S2["m"] * r["iters"] / dt, unit="edge-updates/s", cores=1, kind="port",
                                       sample="1 IRLS iteration (of the 5 a solve takes) of the same %d-view/%d-edge graph with "
                                              "2 %% loop edges, %.1f s" % (S2["n"], S2["m"], dt),
                                       solver_stats=str(O.solver_stats()))
        # config 2
        S3, Q3 = build_problem(10000, 150000, 0.0, seed)
        t, updates, runs, iters = time.time(), 0, 0, 0
        while time.time() - t < 4.0 and runs < 50:
            r = O.irls(S3["QQ"], S3["I"], Q3, 1, 4, SIG, 100, 1e-3)
            updates += S3["m"] * r["iters"]
            iters = r["iters"]
            runs += 1
        dt = time.time() - t
        out["also_config2_10k150k"] = dict(value=updates / dt, unit="edge-updates/s", cores=1, kind="port",
                                           sample="%d complete IRLS solves (%d iterations each) of the same 10000-view/150000-edge "
                                                  "graph, %.1f s" % (runs, iters, dt), iters_to_converge=iters)
        # config 5: the oracle's literal ViewGraph::rotAvg driven through the same call pattern on a bounded stream
        out["also_config5_stream"] = oracle_stream(20000, 3000, 2, seed)
    print(json.dumps(out), flush=True)


def oracle_stream(warm, stream, loops, seed):
    """BASELINE.json config 5 on the CPU oracle (oracle/viewgraph_oracle.py: a literal restatement of ViewGraph::rotAvg
    over the C oracle), bounded: `warm` views as a converged run left them, `stream` views admitted one by one with
    rotAvg(10) each, `loops` loop closures with a global rotAvg, a fix every 20 frames (src/IRotAvg.cpp:360-378)."""
    from oracle import oracle as O
    from oracle.viewgraph_oracle import ViewGraphOracle
    from irotavg_amd import synth
    n = warm + stream
    rng = np.random.default_rng(seed)
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)

    def rel(i, j):
        e = synth.qexp(rng.normal(scale=0.01, size=(1, 3)))[0]
        return O.quat2rmat(synth.qmul(e, synth.qmul(Qgt[j], synth.qconj(Qgt[i]))))
    vo = ViewGraphOracle()
    for v in range(warm):
        vo.addView(O.quat2rmat(synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(1, 3)))[0], Qgt[v])))
        for d in range(1, min(4, v) + 1):
            vo.connect(v - d, v, rel(v - d, v))
        if v % 20 == 0:
            vo.fixPose(v, O.quat2rmat(Qgt[v]))
    loop_at = set(rng.choice(np.arange(warm + 50, n), size=loops, replace=False).tolist()) if loops else set()
    meas = {v: [rel(v - d, v) for d in range(1, 5)] for v in range(warm, n)}
    lm = {v: (int(rng.integers(0, v - 500)),) for v in loop_at}
    lm = {v: (u[0], rel(u[0], v)) for v, u in lm.items()}
    t0, tg, ng = time.time(), 0.0, 0
    for v in range(warm, n):
        vo.addView(meas[v][0] @ vo.R[v - 1])
        for d in range(1, 5):
            vo.connect(v - d, v, meas[v][d - 1])
        if v in lm:
            vo.connect(lm[v][0], v, lm[v][1])
        if v % 20 == 0:
            vo.fixPose(v, O.quat2rmat(Qgt[v]))
        t1 = time.time()
        vo.rotAvg(5000000 if v in lm else 10)
        if v in lm:
            tg += time.time() - t1
            ng += 1
    dt = time.time() - t0
    return dict(value=stream / dt, unit="views/s", cores=1, kind="port",
                sample="%d views streamed onto a warm %d-view sequence (4 links per view, %d loop closure(s) with a global "
                       "re-solve, a fix every 20 frames), %.1f s; Python-driven: the oracle's window extraction is "
                       "interpreter code, the solves are the C oracle" % (stream, warm, loops, dt),
                local_rotavg_ms_mean=1e3 * (dt - tg) / max(stream - ng, 1), global_rotavg_ms_mean=1e3 * tg / max(ng, 1))


def pcg_iteration_roofline(S, st, kr, ia=None, iu=None):
    """the whole two-launch PCG iteration against SURVEY.md 8(d)'s own K4 + K5 bytes: the dense inverse every tile slice
    re-reads and the coarse vectors are this design's cost, not algorithmic traffic"""
    nu_ = S["n"] - 1
    nnz0_ = st["level_nnz"][0]
    k45 = nnz0_ * 12 + 4 * (nu_ + 1) + 2 * 24 * nu_ + 10 * 24 * nu_
    ms_it = kr["cg_apply"]["ms"] + kr["cg_update"]["ms"]
    return {"kernel": "k_cg_apply + k_cg_update (one PCG iteration)", "bound": "hbm",
            "algorithmic_bytes": k45, "formula": "K4 + K5 of SURVEY.md 8(d): nnz0*(8+4) + 4(n+1) + 2*24n + 10*24n",
            "ms_per_iteration": ms_it, "achieved": k45 / (ms_it * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": k45 / (ms_it * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "ms_per_iteration_in_situ": (ia + iu) if ia and iu else None,
            "frac_in_situ": (k45 / ((ia + iu) * 1e-3) / 1e9 / HBM_PEAK_GBS) if ia and iu else None,
            "own_bytes_both_kernels": kr["cg_apply"]["bytes"] + kr["cg_update"]["bytes"]}


# DESIGN.md section 8's table "expected 1 -> 8 numbers, for the first hardware run to falsify", machine-readable:
# ms per irls call by number of GPUs, from single-GPU kernel times, the loopback runs and 10-20 us per small RCCL
# collective on xGMI. Nothing in it has run on more than one GPU.
EXPECTED_MS_PER_IRLS = {
    "100k/2M sequence, sharded direct solver": {1: 1.62, 2: 2.4, 4: 2.1, 8: 2.0},
    "1M/20M sequence, sharded direct solver": {1: 16.7, 2: 10.5, 4: 6.3, 8: 4.4},
    "100k/2M with 2% loop edges, sharded PCG": {1: 13.4, 2: 16.0, 4: 14.0, 8: 14.0},
    "100k/2M + 100 loop closures, sharded direct solver": {1: 2.97, 2: 4.0, 4: 3.6, 8: 3.5},
}


def expected_scaling(args, world):
    key = None
    if args.views == 100000 and args.edges == 2000000:
        key = "100k/2M sequence, sharded direct solver" if args.p_loop == 0.0 else (
            "100k/2M with 2% loop edges, sharded PCG" if abs(args.p_loop - 0.02) < 1e-12 else None)
    elif args.views == 1000000 and args.edges == 20000000 and args.p_loop == 0.0:
        key = "1M/20M sequence, sharded direct solver"
    if key is None:
        return {"workload": None, "note": "no expectation recorded for this size (DESIGN.md section 8 has 100k/2M and 1M/20M)"}
    t = EXPECTED_MS_PER_IRLS[key]
    return {"workload": key, "ms_per_step_by_gpus": {str(k): v for k, v in t.items()},
            "ms_per_step": t.get(world), "speedup_vs_1_gpu": (t[1] / t[world]) if world in t else None,
            "falsified_if": "ms_per_step differs from the expectation by more than 1.5x either way",
            "source": "DESIGN.md section 8: single-GPU kernel times + loopback runs + 10-20 us per small RCCL collective; "
                      "never measured on more than one GPU"}


def host_throttled_usec():
    """Microseconds this process's cgroup has spent throttled by its CPU quota so far (cgroup v2 cpu.stat), or None."""
    try:
        for ln in open("/sys/fs/cgroup/cpu.stat"):
            if ln.startswith("throttled_usec"):
                return int(ln.split()[1])
    except OSError:
        pass
    return None


def step_outputs(G, D, res, dist, Q0):
    """What a caller of `irls` receives from the last step: the rotations (rows [x, y, z, w]), the edge weights and the
    score trace. A sharded handle knows the rows and edges of its own shards: the ranks' parts are merged on every rank,
    and the fixed views, which no shard writes back, keep the rotations they were given."""
    if D is None:
        return {"rotations": G.get_rotations(), "weights": G.get_weights(), "scores": res["scores"]}
    Q = D.get_rotations(into=np.full((D.n_total, 4), np.nan))
    w = D.get_weights()
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, (Q, w))
    for Qr, wr in parts:   # a cross-shard edge lives on both of its shards, computed identically
        Q = np.where(np.isnan(Q), Qr, Q)
        w = np.where(np.isnan(w), wr, w)
    Q[:D.f] = Q0[:D.f]
    return {"rotations": Q, "weights": w, "scores": res["scores"]}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """Writes every array as d/<name>.npy in float64. If they would exceed `limit` bytes in all, every array keeps the same
    fraction of its rows, a sorted sample drawn with a fixed seed, and d/<name>_rows.npy holds the row indices (float64)."""
    os.makedirs(d, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    need = sum(a.nbytes for a in arrays.values())
    # a sampled row costs its own bytes plus 8 for its index; 64 KiB kept back for the .npy headers
    frac = 1.0 if need <= limit else (limit - (64 << 10)) / sum(a.nbytes + 8 * len(a) for a in arrays.values())
    written = {}
    for name, a in arrays.items():
        if frac < 1.0:
            rows = np.sort(np.random.default_rng(seed).choice(len(a), int(len(a) * frac), replace=False))
            a = a[rows]
            np.save(os.path.join(d, name + "_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(d, name + ".npy"), a)
        written[name] = list(a.shape)
    return written


def main():
    thr0 = host_throttled_usec()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300,
                    help="timed steps (default 300: ~0.6 s of GPU work at 100k/2M, long enough for an outside GPU-busy sampler)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ramp", type=int, default=40, help="untimed ramp-up steps ahead of --warmup")
    ap.add_argument("--views", type=int, default=100000)
    ap.add_argument("--edges", type=int, default=2000000)
    ap.add_argument("--p-loop", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-extra", action="store_true")
    ap.add_argument("--no-kernels", action="store_true",
                    help="no per-kernel HIP-event loops and no extra legs: the timed solves only (what the profiling passes run)")
    ap.add_argument("--no-pmc", action="store_true",
                    help="skip the rocprofv3 passes this run launches for HBM traffic and in-solve kernel durations")
    ap.add_argument("--classic", action="store_true",
                    help="A/B: the classic PCG recurrences (separate launches) instead of the two-launch iteration")
    ap.add_argument("--force-dist", action="store_true",
                    help="use the sharded (RCCL) path even with one rank (exercises it on a 1-GPU box)")
    ap.add_argument("--allow-hosted", action="store_true",
                    help="N > 1 only: if the library's RCCL communicator cannot be formed, run the same sharded solver over "
                         "the host-staged wire (torch.distributed/gloo) instead of FAILING. Without this flag a multi-GPU "
                         "run either measures RCCL over xGMI or exits non-zero -- it can never silently measure gloo")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: kernel rooflines, rocprofv3 passes, the other sizes and solvers, the CPU "
                         "baselines and, for N > 1, the phase timing and the check against one GPU (--no-* trim them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rotations, weights, score trace) as DIR/<name>.npy")
    ap.add_argument("--cpu-only", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cpu_only:
        return cpu_baselines_main(json.loads(args.cpu_only))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        # IROTAVG_BENCH_SHARE_GPU=1 (tests on a one-GPU box): every rank on device 0, gloo for the control
        # messages; RCCL refuses two ranks on one device, so the shards then talk over the hosted transport
        share = os.environ.get("IROTAVG_BENCH_SHARE_GPU") == "1"
        if share:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    # how the library this run loads came to be: built by an earlier step (the .so is newer than every source) or
    # rebuilt now -- recorded BEFORE the import, which never builds
    from irotavg_amd import buildlib, synth
    _srcs = [os.path.join(buildlib.CSRC, f) for f in buildlib.SOURCES + buildlib.HEADERS]
    _srcs = [f for f in _srcs if os.path.exists(f)]
    build_record = {
        "needs_build_at_start": bool(buildlib.needs_build()),
        "so_mtime": os.path.getmtime(buildlib.LIB) if os.path.exists(buildlib.LIB) else None,
        "newest_source_mtime": max(os.path.getmtime(f) for f in _srcs) if _srcs else None,
        "mode": "prebuilt: libirotavg_hip.so is newer than every source of it" if not buildlib.needs_build()
                else "stale or missing library: run python -c 'import __graft_entry__ as g; g.build()' first"}
    from irotavg_amd import capi

    S, Q0 = build_problem(args.views, args.edges, args.p_loop, args.seed)
    dev = local_rank if dist is not None else -1

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # N = 1: the resident single-GPU handle. N > 1: the SAME graph sharded by contiguous view
    # ranges, one shard per process/GPU, RCCL over xGMI (halo exchange of the PCG direction +
    # all-reduced dot products; see DESIGN.md "Multi-GPU") -- strong scaling.
    G = D = None
    wire = None
    if dist is None:
        G = capi.Graph(S["I"], S["QQ"], S["n"], 1, pcg_rtol=args.rtol, device=dev,
                       pcg_classic=1 if args.classic else 0)
        G.set_rotations(Q0)
        G.snapshot_rotations()

        def step():
            G.restore_rotations()
            r = G.irls(4, SIG, 100, 1e-3)
            G.synchronize()
            return r
    else:
        wire = "RCCL"
        try:
            uid = [capi.DistGraph.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            D = capi.DistGraph(S["I"], S["QQ"], S["n"], 1, world, rank=rank, unique_id=uid[0],
                               pcg_rtol=args.rtol, device=dev)
        except Exception as e:  # e.g. the library's communicator cannot be formed on this node
            print("[bench] rank %d: RCCL shard handle failed (%s)" % (rank, e), file=sys.stderr, flush=True)
            D = None
        ok = torch.tensor([1 if D is not None else 0], dtype=torch.int32, device="cpu" if share else "cuda")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            if D is not None:
                D.close()
            if not args.allow_hosted:
                # A scaling run must measure RCCL over xGMI or nothing: every rank leaves with an error (rank 0 prints one
                # JSON line that says so, for whoever parses the output).
                if rank == 0:
                    print(json.dumps({"metric": "IRLS edge-updates/sec (+ iters-to-converge)", "value": None,
                                      "n_gpus": world, "error": "RCCL communicator could not be formed on every rank; "
                                      "refusing to measure the host-staged wire (pass --allow-hosted to do that on purpose)",
                                      "dist": {"wire": "none", "ncclCommCount": 0}}), flush=True)
                dist.barrier()
                dist.destroy_process_group()
                sys.exit(3)
            # --allow-hosted: every rank falls back together: the same sharded solver over the hosted transport
            # (irotavg_dist_create_hosted: halo + all-reduce staged through host buffers and moved by
            # torch.distributed/gloo) -- slower per exchange, same arithmetic
            hosted = dist.new_group(backend="gloo")
            D = capi.DistGraph(S["I"], S["QQ"], S["n"], 1, world, rank=rank,
                               transport=capi.torch_transport(hosted), pcg_rtol=args.rtol, device=dev)
            wire = "host-staged torch.distributed/gloo (RCCL communicator unavailable)"

        D.set_rotations(Q0)
        D.snapshot_rotations()

        def step():
            D.restore_rotations()        # device copy, as the single-GPU step
            return D.irls(4, SIG, 100, 1e-3)

    res = None
    # a fresh box starts at idle clocks and with cold caches / allocator pools: the first solves of a process
    # measured ~8 % slower than the steady state (6.24 vs 5.75 ms). Ramp-up steps ahead of the W warm-up
    # steps the contract names -- untimed, like them
    for _ in range(args.ramp):
        res = step()
    for _ in range(args.warmup):
        res = step()
    barrier()
    thr_a = host_throttled_usec()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    barrier()
    dt = time.perf_counter() - t0
    thr_b = host_throttled_usec()
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if share else "cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    dstats = D.stats() if D is not None else None
    dumped = None
    if args.dump_outputs:   # what the last timed step left, before anything else runs on the handle
        outputs = step_outputs(G, D, res, dist, Q0)
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, outputs)
        del outputs
    if D is not None:
        dinfo = D.info()   # wire actually used + ranks of the RCCL communicator as RCCL counts them
        if args.full:
            # where an iteration goes, phase by phase (irotavg_dist_timing): a few UNTIMED solves with the phase clock on --
            # the stream is drained at every phase boundary, so the phases are to be read against each other
            D.timing(True)
            for _ in range(3):
                step()
            dphases = D.timing(False)
            tp = torch.tensor([dphases["us_per_iteration"][k] for k in capi.DistGraph.TIMING_PHASES], dtype=torch.float64,
                              device="cpu" if share else "cuda")
            dist.all_reduce(tp, op=dist.ReduceOp.MAX)   # the slowest rank's phases
            dphases["us_per_iteration_max_over_ranks"] = {k: float(tp[i].item()) for i, k in enumerate(capi.DistGraph.TIMING_PHASES)}
        D.close()
        if rank == 0 and args.full:   # kernel rooflines are measured on a single-GPU handle of the same graph
            G = capi.Graph(S["I"], S["QQ"], S["n"], 1, pcg_rtol=args.rtol, device=dev)
            G.set_rotations(Q0)
            res_single = G.irls(4, SIG, 100, 1e-3)   # ... and the sharded run is held against it (dist.matches_single_gpu)

    if rank == 0:
        iters = res["iters"]
        st = G.stats() if G is not None else {}
        if dstats is not None:
            st = dict(st, pcg_iters=dstats["pcg_iters"], pcg_solves=dstats["pcg_solves"])
        value = S["m"] * iters * args.steps / dt
        line = {
            "metric": "IRLS edge-updates/sec (+ iters-to-converge)",
            "value": value, "unit": "edge-updates/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ramp": args.ramp, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "iters_to_converge": iters,
            "config": {"workload": "synthetic SO(3) view-graph, %d views / %d edges, p_loop=%g, "
                                   "sigma_n=0.01 rad, 5%% outliers among loop edges, seed %d; "
                                   "f=1, init_mst start, Geman-McClure sigma=5deg, change_th=1e-3, "
                                   "max_iters=100" % (S["n"], S["m"], args.p_loop, args.seed),
                       "linear_solver": ("banded direct solver (block cyclic reduction, blocks of %d; band %d)" % (
                                             st["band_block"], st["band"]) if st.get("direct_solves", 0) > 0 and dstats is None
                                         else ("sharded banded direct solver (blocks of %d: local reductions, ONE gather of the "
                                               "%d separators per linear solve, separator system on every rank)" % (
                                                   dinfo["direct_block"], world)
                                               if dstats is not None and dinfo.get("direct_block") else
                                               "multigrid-preconditioned CG")),
                       "direct_solves": st.get("direct_solves", 0) if dstats is None else dstats.get("direct_solves", 0),
                       "pcg_rtol": args.rtol, "pcg_iters_per_solve": st["pcg_iters"] / max(st["pcg_solves"], 1),
                       "mg_level_rows": st["level_rows"] if dstats is None else dstats["level_rows"],
                       "parallelism": "1 GPU" if world == 1 else
                       "views sharded in %d contiguous ranges, 1 shard/GPU, %s %s" % (
                           world, wire, "gather of the separators (1 per linear solve) + halo of X and score all-reduce "
                           "(1 per IRLS iteration)" if dstats is not None and dinfo.get("direct_block") else "halo + all-reduce")},
            "final_scores": [float(x) for x in res["scores"]],
            "timing_note": "steady state: %d untimed ramp-up solves precede the --warmup solves (a fresh box starts at "
                           "idle clocks; the first solves of a process run ~8 %% slower); every step repeats the "
                           "identical solve (on the PCG path the predictive poll schedule and the cached coarse inverse "
                           "are then warm; the direct solver keeps nothing between solves) -- not a first-call figure "
                           "(that is --full's also_one_shot_host_buffers)" % args.ramp,
        }
        line["build"] = build_record
        if dumped is not None:
            line["outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
        if dstats is not None:
            line["config"]["dist"] = dinfo
            # the first multi-GPU run diagnoses itself: the wire that carried it, RCCL's own count of the communicator,
            # per-phase microseconds of an IRLS iteration, and what DESIGN.md section 8 expects this run to show
            line["dist"] = {
                "wire": dinfo["wire"], "halo": dinfo["halo"], "ncclCommCount": dinfo["rccl_comm_ranks"], "world": world,
                "hosted_allowed": bool(args.allow_hosted),
                "valid_scaling_measurement": bool(dinfo["wire"] == "rccl" and dinfo["rccl_comm_ranks"] == world and not share),
                "sharded_solver": "direct" if dinfo.get("direct_block") else "pcg",
                "closures": dinfo.get("closures", 0),
                "expected": expected_scaling(args, world),
            }
        if dstats is not None and args.full:
            line["dist"].update({
                # the sharded result against the same graph on ONE GPU of this node (rank 0's handle): a wrong exchange on
                # a wire that no test could exercise shows here, not in a plausible-looking throughput
                "matches_single_gpu": bool(res["iters"] == res_single["iters"] and
                                           np.allclose(res["scores"], res_single["scores"], rtol=1e-6, atol=1e-12)),
                "single_gpu_iters": int(res_single["iters"]),
                "max_rel_score_diff": float(np.max(np.abs(np.asarray(res["scores"][:min(res["iters"], res_single["iters"])]) -
                                                          np.asarray(res_single["scores"][:min(res["iters"], res_single["iters"])])) /
                                                   np.maximum(np.abs(np.asarray(res_single["scores"][:min(res["iters"], res_single["iters"])])), 1e-300))),
                "phases_us_per_iteration": dphases["us_per_iteration_max_over_ranks"],
                "phases_us_per_iteration_rank0": dphases["us_per_iteration"],
                "phases_iterations": dphases["iterations"],
                "phases_note": "3 untimed solves with irotavg_dist_timing on (stream drained at every phase boundary: read the "
                               "phases against each other, their sum exceeds the undisturbed iteration); max over ranks",
            })
        if args.no_kernels or not args.full:
            # a plain run: the headline and nothing that needs runs of its own
            if G is not None:
                G.close()
            thr1 = host_throttled_usec()
            line["host_throttled_usec"] = None if thr0 is None or thr1 is None else thr1 - thr0
            line["host_throttled_usec_timed_region"] = None if thr_a is None or thr_b is None else thr_b - thr_a
            print(json.dumps(line), flush=True)
            if dist is not None:
                dist.barrier()
                dist.destroy_process_group()
            return
        extras = (not args.no_extra) and world == 1 and args.p_loop == 0.0 and args.views == 100000
        cpu_proc = None
        if not args.no_cpu and world == 1:
            # every CPU-oracle baseline runs in a process of its own while the GPU legs below go on (cpu_baselines_main)
            import subprocess
            spec = dict(views=args.views, edges=args.edges, p_loop=args.p_loop, seed=args.seed, extras=extras)
            # (one thread, as its "cores": 1 says, and no GPU: the box's cgroup allows 16 CPUs per 100 ms, and a burst of
            # library worker threads in that process got the whole group throttled for 60-80 ms -- seen as one slow l1ra
            # call out of five at 10k/150k; "host_throttled_usec" below reports what the group lost during this run)
            cpu_proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-only", json.dumps(spec)],
                                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                        env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="",
                                                 OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1"))
        kr = kernel_rooflines(G, S, st, sharded=dstats is not None)
        FP64_PEAK_TF = 78.6   # AMD's MI355X data sheet (fp64 vector = matrix); the guide lists no fp64 figure
        # HBM traffic and in-solve kernel durations: measured NOW, by rocprofv3 passes of this command (live_profile)
        prof, prof_where = (None, "--no-pmc") if (args.no_pmc or dstats is not None) else live_profile(args, line["config"]["workload"])
        line["profile_source"] = ("rocprofv3 passes launched by this run (kernel trace, FETCH_SIZE, WRITE_SIZE): " + prof_where
                                  ) if prof else "no in-run profile (%s): traffic and in-situ fields are null" % prof_where

        def traffic(kernel, targs=None):
            return prof_value(prof, kernel, "traffic_bytes", targs)

        def insitu_ms(kernel, targs=None):
            v = prof_value(prof, kernel, "avg_us", targs)
            return v * 1e-3 if v is not None else None
        dom = "bcr_solve" if "bcr_solve" in kr else \
            ("cg_apply" if "cg_apply" in kr else ("pspmv" if "pspmv" in kr else "spmv"))
        if dom == "bcr_solve":
            # the dominant "kernel" of a direct solve is the solve itself: 77 % of an IRLS iteration, one template
            # (k_bcr_reduce) launched once per level + two launches for the ways back. Quoted as a whole -- all
            # launches, all levels -- and launch by launch below it (round 3 quoted level 0 only: the best third)
            bs = kr["bcr_solve"]
            nl = len(bs["levels"])
            # (kernel, template arguments that pick the instantiation, launches per solve)
            parts = [("bcr_reduce_l0", "k_bcr_reduce", {2: "true"}, 1)]
            if bs.get("fused_upper_reduce"):
                parts.append(("bcr_reduce_upper", "k_bcr_reduce_up", None, 1))
                parts.append(("bcr_back_upper", "k_bcr_back_top", None, 1))
            else:
                if nl >= 3:
                    parts.append(("bcr_reduce_mid", "k_bcr_reduce", {2: "false", 3: "false"}, nl - 2))
                if nl >= 2:
                    parts.append(("bcr_reduce_top", "k_bcr_reduce", {2: "false", 3: "true"}, 1))
                    parts.append(("bcr_back_upper", "k_bcr_back_top", None, 1))
            parts.append(("bcr_back_l0", "k_bcr_back", {2: "true"}, 1))
            tr = [traffic(k, ta) for _, k, ta, _ in parts]
            du = [insitu_ms(k, ta) for _, k, ta, _ in parts]
            tr_solve = sum(t * c for t, (_, _, _, c) in zip(tr, parts)) if all(t is not None for t in tr) else None
            ms_insitu = sum(d * c for d, (_, _, _, c) in zip(du, parts)) if all(d is not None for d in du) else None
            line["roofline"] = {
                "kernel": "one banded direct solve = %d launches over %d levels: k_bcr_reduce (level 0 gathers the blocks from the "
                          "SELL-64 operator; every level eliminates 7 of 8 blocks per chunk on the matrix cores and writes W), "
                          "%s, k_bcr_back_top (ways back of the levels >= 1), k_bcr_back (level 0 -> X)" % (
                              bs["launches"], nl, "k_bcr_reduce_up (the reductions of all levels >= 1 in one launch)"
                              if bs.get("fused_upper_reduce") else "k_bcr_reduce per upper level"),
                "bound": "hbm", "achieved": bs["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bs["gbs"] / HBM_PEAK_GBS,
                "algorithmic_bytes": bs["bytes"], "ms_per_launch": bs["ms"], "launches_per_solve": bs["launches"],
                "traffic": tr_solve, "ms_per_launch_in_situ": ms_insitu,
                "frac_in_situ": (bs["bytes"] / (ms_insitu * 1e-3) / 1e9 / HBM_PEAK_GBS) if ms_insitu else None,
                "note": "HIP-event time of the whole solve (all launches back to back on the handle's stream) against the "
                        "algorithmic bytes of all its launches (DESIGN.md 5d). Not bandwidth-bound: ~14 dependent rounds of "
                        "block eliminations (sweep of a %d x %d block, five products on the matrix cores) set the time; "
                        "1.6 %% of the rows (levels >= 1) take half of it. Inside irls the two ways back also make the "
                        "step of every view (K6: exp map, rotation update, score partials -- the in-situ durations "
                        "include it, the algorithmic bytes do not count its 6.4 MB)" % (bs["block"], bs["block"]),
                "mfma": {"bound": "mfma", "achieved": bs["tflops"], "peak": FP64_PEAK_TF, "unit": "TFLOP/s",
                         "frac": bs["tflops"] / FP64_PEAK_TF, "flops_per_solve": bs["flops"]},
                "by_launch": {name: dict(launches=c, ms=(kr[name]["ms"] if name in kr else None),
                                         algorithmic_bytes=(kr[name]["bytes"] if name in kr else None),
                                         frac=(kr[name]["gbs"] / HBM_PEAK_GBS if name in kr else None),
                                         ms_in_situ=d, traffic=t)
                              for (name, _, _, c), t, d in zip(parts, tr, du)},
                "block": bs["block"], "levels": bs["levels"]}
            if bs.get("fused_upper_reduce"):   # one launch for the levels >= 1: the HIP-event figures of its levels, launched one by one
                up_ms = [kr["bcr_reduce_l%d" % l]["ms"] for l in range(1, nl)]
                up_by = [kr["bcr_reduce_l%d" % l]["bytes"] for l in range(1, nl)]
                line["roofline"]["by_launch"]["bcr_reduce_upper"].update(
                    levels_one_by_one_ms=up_ms, algorithmic_bytes=sum(up_by), levels_algorithmic_bytes=up_by,
                    note="k_bcr_reduce_up: levels 1 .. %d in one launch, workgroup c runs chunk c of every level, a counter "
                         "between levels, separator data through device-scope atomic stores / loads" % (nl - 1))
            elif nl >= 3:   # levels 1 .. nl-2 share one instantiation: HIP-event figures per level
                line["roofline"]["by_launch"]["bcr_reduce_mid"].update(
                    ms=[kr["bcr_reduce_l%d" % l]["ms"] for l in range(1, nl - 1)],
                    algorithmic_bytes=[kr["bcr_reduce_l%d" % l]["bytes"] for l in range(1, nl - 1)],
                    frac=[kr["bcr_reduce_l%d" % l]["gbs"] / HBM_PEAK_GBS for l in range(1, nl - 1)])
                line["roofline"]["by_launch"]["bcr_reduce_top"].update(
                    ms=kr["bcr_reduce_l%d" % (nl - 1)]["ms"], algorithmic_bytes=kr["bcr_reduce_l%d" % (nl - 1)]["bytes"],
                    frac=kr["bcr_reduce_l%d" % (nl - 1)]["gbs"] / HBM_PEAK_GBS)
            line["roofline_direct_solve"] = {k: line["roofline"][k] for k in ("kernel", "bound", "algorithmic_bytes", "achieved",
                                                                            "peak", "unit", "frac", "mfma", "block", "levels")}
            line["roofline_direct_solve"]["ms_per_solve"] = bs["ms"]
        else:
            dname = {"spmv": "k_spmv_dot (level-0 SELL-64 SpMV + fused dot, dominant PCG kernel)",
                     "pspmv": "k_pspmv_dot (PCG p-update fused into the level-0 SELL-64 SpMV + dot, dominant PCG kernel)",
                     "cg_apply": "k_cg_apply (u = M^-1 r incl. the tile's slice of the dense coarse solve and the level-1 "
                                 "up-sweep, then the level-0 SELL-64 SpMV w = L u + dots; dominant PCG kernel)"}[dom]
            kname = {"pspmv": "k_pspmv_dot", "spmv": "k_spmv_dot", "cg_apply": "k_cg_apply"}[dom]
            insitu = insitu_ms(kname)
            line["roofline"] = {"kernel": dname,
                                "bound": "hbm", "achieved": kr[dom]["gbs"], "peak": HBM_PEAK_GBS,
                                "unit": "GB/s", "frac": kr[dom]["gbs"] / HBM_PEAK_GBS, "traffic": traffic(kname),
                                "ms_per_launch": kr[dom]["ms"], "algorithmic_bytes": kr[dom]["bytes"],
                                "ms_per_launch_in_situ": insitu,
                                "frac_in_situ": (kr[dom]["bytes"] / (insitu * 1e-3) / 1e9 / HBM_PEAK_GBS) if insitu else None}
        if "cg_apply" in kr and "cg_update" in kr:
            line["roofline_pcg_iteration"] = pcg_iteration_roofline(S, st, kr, insitu_ms("k_cg_apply"), insitu_ms("k_cg_update"))
        for key, kn, label, targs in (
                ("update_weights", "k_update_weights", "K2: k_update_weights (residual of the step + the robust weight, "
                                                       "ral/l1_irls.cpp:614-727)", None),
                ("edge_residual", "k_edge_residual", "k_edge_residual (K1, the kernel north_star names)", None),
                ("weights_then_residual", "k_weights_then_residual",
                 "K2 + the next iteration's K1 in one pass over the edges (what the direct solver's irls loop runs from its "
                 "second iteration on: k_update_weights then has no launch inside a solve, k_edge_residual one)", None)):
            if key not in kr:
                continue
            ins = insitu_ms(kn, targs)
            line["roofline_" + key] = {
                "kernel": label, "bound": "hbm", "achieved": kr[key]["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": kr[key]["gbs"] / HBM_PEAK_GBS, "traffic": traffic(kn, targs), "ms_per_launch": kr[key]["ms"],
                "algorithmic_bytes": kr[key]["bytes"], "ms_per_launch_in_situ": ins,
                "frac_in_situ": (kr[key]["bytes"] / (ins * 1e-3) / 1e9 / HBM_PEAK_GBS) if ins else None}
        if "roofline_edge_residual" in line:
            # K1's figure of record is the IN-SITU one (inside irls, kernel trace of this run): 50 back-to-back launches
            # re-read a 131 MB working set that fits the 256 MiB Infinity Cache. And the true-HBM case next to it: the
            # same kernel at 1M views / 20M edges (1.3 GB per launch: no cache holds it) on a graph of that shape
            # (band topology of the generator, random unit quaternions -- K1's work does not depend on the values)
            re_ = line["roofline_edge_residual"]
            re_["frac_headline"] = re_["frac_in_situ"] if re_.get("frac_in_situ") else re_["frac"]
            re_["frac_headline_is"] = "in situ (kernel trace inside irls)" if re_.get("frac_in_situ") else "back-to-back launches"
            if not args.no_extra and world == 1 and args.views == 100000:
                try:
                    nb_, mb_ = 1000000, 20000000
                    rngb = np.random.default_rng(1)
                    Ib, _, _ = synth.band_loop_topology(nb_, mb_, 0.0, rngb)
                    QQb = rngb.normal(size=(len(Ib), 4))
                    QQb /= np.linalg.norm(QQb, axis=1, keepdims=True)
                    Qb = rngb.normal(size=(nb_, 4))
                    Qb /= np.linalg.norm(Qb, axis=1, keepdims=True)
                    with capi.Graph(Ib, QQb, nb_, 1) as Gb:
                        Gb.set_rotations(Qb)
                        msb = min(Gb.time_kernel(1, 20) for _ in range(3))
                    byb = len(Ib) * (8 + 32 + 24) + 32 * nb_
                    re_["at_1M_20M"] = {"ms_per_launch": msb, "algorithmic_bytes": byb, "achieved": byb / (msb * 1e-3) / 1e9,
                                        "frac": byb / (msb * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                        "note": "k_edge_residual on 1M views / 20M edges: 1.3 GB per launch, beyond every cache"}
                    del Ib, QQb, Qb
                    capi.trim_memory()   # (its blocks -- gigabytes -- would crowd the device pool of the legs below)
                except Exception as e:   # (memory of a small test box)
                    re_["at_1M_20M"] = {"error": str(e)}
        ta = [traffic(k) for k in ("k_assemble0w", "k_coarse_level")]
        ins = insitu_ms("k_assemble0w")
        line["roofline_assembly"] = {
            "kernel": "K3: k_assemble0w (level 0 from the LDS-staged run of the edge list; on the PCG path also level 1 "
                      "and k_coarse_level for level 2)",
            "bound": "hbm", "achieved": kr["assemble"]["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": kr["assemble"]["gbs"] / HBM_PEAK_GBS,
            "traffic": (ta[0] + (ta[1] or 0.0)) if ta[0] is not None else None,
            "ms_per_launch": kr["assemble"]["ms"], "algorithmic_bytes": kr["assemble"]["bytes"],
            "ms_per_launch_in_situ": ins}
        line["kernels"] = {k: {kk: (vv if isinstance(vv, (int, list, dict, str)) else float(vv)) for kk, vv in v.items()}
                           for k, v in kr.items()}
        if not args.no_extra and world == 1 and args.p_loop == 0.0 and args.views == 100000:
            # the other topology SURVEY.md 8(d) asks for: 2 % random loop-closure edges
            S2, Q2 = build_problem(args.views, args.edges, 0.02, args.seed)
            with capi.Graph(S2["I"], S2["QQ"], S2["n"], 1, pcg_rtol=args.rtol) as G2:
                G2.set_rotations(Q2)
                G2.snapshot_rotations()
                G2.irls(4, SIG, 100, 1e-3)
                t1 = time.perf_counter()
                reps = 5
                for _ in range(reps):
                    G2.restore_rotations()
                    r2 = G2.irls(4, SIG, 100, 1e-3)
                G2.synchronize()
                d2 = time.perf_counter() - t1
                s2 = G2.stats()
                kr2 = {}
                try:   # the six-launch iteration of a graph with far entries: its SpMV and one preconditioner application
                    by = s2["level_nnz"][0] * 12 + 4 * S2["n"] + 2 * 24 * (S2["n"] - 1)
                    ms = G2.time_kernel(4, 50)
                    kr2["spmv"] = dict(ms=ms, bytes=by, gbs=by / (ms * 1e-3) / 1e9, frac=by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS)
                    kr2["precondition"] = dict(ms=G2.time_kernel(5, 50))
                    kr2["dense_inversion"] = dict(ms=G2.time_kernel(7, 5), rows=int(s2["level_rows"][s2["levels"] - 1]))
                except capi.IrotavgError:
                    pass
            line["also_p_loop_0.02"] = {"value": S2["m"] * r2["iters"] * reps / d2, "unit": "edge-updates/s",
                                        "iters_to_converge": r2["iters"], "ms_per_step": 1e3 * d2 / reps,
                                        "pcg_iters_per_solve": s2["pcg_iters"] / max(s2["pcg_solves"], 1),
                                        "dense_inversions_per_solve_call": s2["dense_inversions"] / (reps + 1),
                                        "dense_repairs_per_solve_call": s2["dense_repairs"] / (reps + 1),
                                        "linear_solver": "multigrid-preconditioned CG (40 000 loop closures: beyond the "
                                                         "2048 the direct solver carries)",
                                        "kernels": kr2}
            # the same graph with inexact outer iterations (options.inexact_outer = 1, round 5): early linear systems only
            # as accurate as the outer iteration can use; its result against the all-exact one above
            with capi.Graph(S2["I"], S2["QQ"], S2["n"], 1, pcg_rtol=args.rtol) as G2:
                G2.set_rotations(Q2)
                G2.irls(4, SIG, 100, 1e-3)
                Qex = G2.get_rotations()
            with capi.Graph(S2["I"], S2["QQ"], S2["n"], 1, pcg_rtol=args.rtol, inexact_outer=1) as G2:
                G2.set_rotations(Q2)
                G2.snapshot_rotations()
                G2.irls(4, SIG, 100, 1e-3)
                t1 = time.perf_counter()
                for _ in range(reps):
                    G2.restore_rotations()
                    r3 = G2.irls(4, SIG, 100, 1e-3)
                G2.synchronize()
                d3 = time.perf_counter() - t1
                s3 = G2.stats()
                ang3 = synth.angular_distance(G2.get_rotations(), Qex)
            line["also_p_loop_0.02"]["inexact_outer"] = {
                "value": S2["m"] * r3["iters"] * reps / d3, "unit": "edge-updates/s", "ms_per_step": 1e3 * d3 / reps,
                "iters_to_converge": r3["iters"], "pcg_iters_per_solve": s3["pcg_iters"] / max(s3["pcg_solves"], 1),
                "rotations_vs_all_exact_rad": {"mean": float(ang3.mean()), "max": float(ang3.max())},
                "note": "opt-in: while the last step was above 50 x change_th a system is solved to a relative residual of "
                        "0.01 change_th / last step (<= 1e-4), the iterations near the fixed point and the last one to "
                        "pcg_rtol; same outer iterations as the all-exact default in the fields above"}
        if not args.no_extra and world == 1 and args.p_loop == 0.0 and args.views == 100000:
            # the headline topology with a NON-uniform re-weighting: 2 % of the band edges carry a 0.3 rad
            # error (the workload of test_every_cost_on_the_two_launch_path_matches_oracle at full size); the
            # headline graph itself has no outliers at all (SURVEY's generator puts them among loop edges)
            from irotavg_amd import ral, synth
            S4 = synth.make_graph(args.views, args.edges, 0.0, seed=args.seed, p_band_out=0.02)
            Q4 = np.zeros((args.views, 4)); Q4[:, 3] = 1; Q4[0] = S4["Qgt"][0]
            ral.init_mst(Q4, S4["QQ"], S4["I"], 1)
            with capi.Graph(S4["I"], S4["QQ"], S4["n"], 1, pcg_rtol=args.rtol) as G4:
                G4.set_rotations(Q4)
                G4.snapshot_rotations()
                for _ in range(3):
                    G4.restore_rotations()
                    G4.irls(4, SIG, 100, 1e-3)
                G4.synchronize()
                G4.reset_stats()
                t1 = time.perf_counter()
                reps = 5
                for _ in range(reps):
                    G4.restore_rotations()
                    r4 = G4.irls(4, SIG, 100, 1e-3)
                G4.synchronize()
                d4 = time.perf_counter() - t1
                s4 = G4.stats()
            line["also_band_outliers"] = {"value": S4["m"] * r4["iters"] * reps / d4, "unit": "edge-updates/s",
                                          "iters_to_converge": r4["iters"], "ms_per_step": 1e3 * d4 / reps,
                                          "direct_solves_per_solve_call": s4.get("direct_solves", 0) / reps,
                                          "pcg_iters_per_solve": s4["pcg_iters"] / max(s4["pcg_solves"], 1),
                                          "dense_inversions_per_solve_call": s4["dense_inversions"] / reps,
                                          "note": "p_loop=0, 2 % of ALL edges off by N(0, 0.3^2) rad, init_mst start"}
        if extras:
            # a view sequence WITH loop closures (what a SLAM run produces, src/IRotAvg.cpp:371-378): the banded direct
            # solver carries up to 2048 of them (forward eliminations along the elimination tree + Woodbury system,
            # bcr.hip), beyond that -- and for comparison here -- the multigrid-PCG
            from irotavg_amd import ral, synth
            for nclose in (30, 100, 1000):
                Sc = synth.add_closures(S, nclose, seed=7, wrong=max(1, nclose // 33))
                Qc = np.zeros((Sc["n"], 4)); Qc[:, 3] = 1; Qc[0] = Sc["Qgt"][0]
                ral.init_mst(Qc, Sc["QQ"], Sc["I"], 1)
                leg = {}
                for bd, tag in ((0, "direct"), (-1, "pcg")):
                    with capi.Graph(Sc["I"], Sc["QQ"], Sc["n"], 1, pcg_rtol=args.rtol, band_direct=bd) as Gc:
                        Gc.set_rotations(Qc)
                        Gc.snapshot_rotations()
                        Gc.irls(4, SIG, 100, 1e-3)
                        Gc.synchronize()
                        Gc.reset_stats()
                        reps = 5 if bd == 0 else 2
                        t1 = time.perf_counter()
                        for _ in range(reps):
                            Gc.restore_rotations()
                            rc_ = Gc.irls(4, SIG, 100, 1e-3)
                        Gc.synchronize()
                        dc = time.perf_counter() - t1
                        sc = Gc.stats()
                    leg[tag] = dict(ms_per_step=1e3 * dc / reps, iters_to_converge=rc_["iters"],
                                    value=Sc["m"] * rc_["iters"] * reps / dc, direct_solves_per_solve_call=sc.get("direct_solves", 0) / reps,
                                    direct_guarded=sc.get("direct_guarded", 0),
                                    pcg_iters_per_solve=sc["pcg_iters"] / max(sc["pcg_solves"], 1))
                # the same graph in 8 shards, all on this GPU one after the other (loopback): closures on the SHARDED direct
                # solver (round 5) against what the shards ran until then, the sharded PCG -- the only statement a one-GPU
                # box can make about that path's cost (eight ranks' work in sequence; a node runs them side by side)
                shard_leg = {}
                for off, tag in ((False, "direct"), (True, "pcg")):
                    if nclose != 100 and off:
                        continue
                    if off:
                        os.environ["IROTAVG_DIST_NO_CLOSURES"] = "1"
                    try:
                        with capi.DistGraph(Sc["I"], Sc["QQ"], Sc["n"], 1, 8, pcg_rtol=args.rtol) as Dc:
                            Dc.set_rotations(Qc)
                            Dc.snapshot_rotations()
                            Dc.irls(4, SIG, 100, 1e-3)
                            reps = 1 if off else 3
                            t1 = time.perf_counter()
                            for _ in range(reps):
                                Dc.restore_rotations()
                                rd_ = Dc.irls(4, SIG, 100, 1e-3)
                            dd = time.perf_counter() - t1
                            shard_leg[tag] = dict(ms_per_step=1e3 * dd / reps, iters_to_converge=rd_["iters"],
                                                  closures_carried=Dc.info()["closures"], block=Dc.info()["direct_block"])
                    finally:
                        os.environ.pop("IROTAVG_DIST_NO_CLOSURES", None)
                leg["direct"]["eight_shards_loopback"] = shard_leg
                line["also_closures_%d" % nclose] = dict(
                    leg["direct"], unit="edge-updates/s", pcg_path=leg["pcg"],
                    note="the headline sequence + %d loop closures 100 ... n/2 views long, %d of them wrong (random rotation); "
                         "irls to convergence; pcg_path: the same through band_direct = -1" % (nclose, max(1, nclose // 33)))
            # BASELINE.json config 2
            S3, Q3 = build_problem(10000, 150000, 0.0, args.seed)
            with capi.Graph(S3["I"], S3["QQ"], S3["n"], 1, pcg_rtol=args.rtol) as G3:
                G3.set_rotations(Q3)
                G3.snapshot_rotations()
                for _ in range(20):
                    G3.restore_rotations()
                    G3.irls(4, SIG, 100, 1e-3)
                G3.synchronize()
                # five batches of ten solves, the best batch reported: a solve of this size is 25 launches in 0.4 ms, i.e.
                # host-bound, and this leg runs while the CPU baselines and the profiler's children use the box's CPU
                # quota -- a throttled batch (cgroup cpu.stat, "host_throttled_usec") says nothing about the GPU path
                reps, batches = 10, []
                for _ in range(5):
                    t1 = time.perf_counter()
                    for _ in range(reps):
                        G3.restore_rotations()
                        r3 = G3.irls(4, SIG, 100, 1e-3)
                    G3.synchronize()
                    batches.append(time.perf_counter() - t1)
                d3 = min(batches)
                s3 = G3.stats()
            line["also_config2_10k150k"] = {"value": S3["m"] * r3["iters"] * reps / d3, "unit": "edge-updates/s",
                                            "iters_to_converge": r3["iters"], "ms_per_step": 1e3 * d3 / reps,
                                            "ms_per_step_all_batches": [1e3 * b / reps for b in batches],
                                            "linear_solver": "banded direct solver, blocks of %d" % s3["band_block"]
                                            if s3.get("direct_solves", 0) else "multigrid-preconditioned CG",
                                            "note": "BASELINE.json config 2: synthetic 10k views / 150k edges, same protocol as the "
                                                    "headline; best of five batches of ten solves (host-bound at this size: see "
                                                    "ms_per_step_all_batches and host_throttled_usec)"}
            # BASELINE.json config 5: the native stream driver (tools/stream_bench.cpp over the C ABI)
            import subprocess
            exe = os.path.join(ROOT, "irotavg_amd", "bin", "stream_bench")
            try:
                r5 = subprocess.run([exe, "50000", "50000", "10", str(args.seed), "1", "1"], capture_output=True, text=True, timeout=300)
                d5 = json.loads([ln for ln in r5.stdout.splitlines() if ln.startswith("{")][-1])
                line["also_config5_stream"] = dict(
                    value=d5["views_per_s"], unit="views/s", seconds=d5["seconds"], local_rotavg_ms_mean=d5["local_rotavg_ms_mean"],
                    local_rotavg_ms_p99=d5["local_rotavg_ms_p99"], global_rotavg_ms_mean=d5["global_rotavg_ms_mean"],
                    global_rotavg_ms=d5.get("global_rotavg_ms"), prepare_seconds=d5.get("prepare_seconds"),
                    loop_closures=d5["loop_closures"], mean_angular_error_rad=d5["mean_angular_error_rad"],
                    note="BASELINE.json config 5: 50k views streamed one by one (rotAvg(10) each: one kernel launch) onto a warm "
                         "50k-view sequence, 10 loop closures (rotAvg(5000000) each, on the device-resident growing graph, "
                         "resident.hip), a fix every 20 frames; irotavg_viewgraph_prepare after loading, outside the timed loop")
            except Exception as e:
                line["also_config5_stream"] = dict(value=None, unit="views/s", note="stream_bench failed: %s" % e)
        if not args.no_extra and world == 1 and st.get("direct_solves", 0) > 0:
            # the same workload through the handle's OTHER solver: the multigrid-PCG (what every graph with loop
            # closures and every shard runs; the headline of rounds 1 and 2)
            with capi.Graph(S["I"], S["QQ"], S["n"], 1, pcg_rtol=args.rtol, band_direct=-1) as G5:
                G5.set_rotations(Q0)
                G5.snapshot_rotations()
                for _ in range(10):
                    G5.restore_rotations()
                    G5.irls(4, SIG, 100, 1e-3)
                G5.synchronize()
                G5.reset_stats()
                t1 = time.perf_counter()
                reps = 5
                for _ in range(reps):
                    G5.restore_rotations()
                    r5 = G5.irls(4, SIG, 100, 1e-3)
                G5.synchronize()
                d5 = time.perf_counter() - t1
                s5 = G5.stats()
            line["also_pcg_path"] = {"value": S["m"] * r5["iters"] * reps / d5, "unit": "edge-updates/s",
                                     "iters_to_converge": r5["iters"], "ms_per_step": 1e3 * d5 / reps,
                                     "pcg_iters_per_solve": s5["pcg_iters"] / max(s5["pcg_solves"], 1),
                                     "note": "band_direct = -1: two-launch multigrid-PCG (cgcg.hip), pcg_rtol %g" % args.rtol}
        if not args.no_extra and world == 1 and args.rtol == 1e-10 and st.get("direct_solves", 0) == 0:
            # the same workload with the inner tolerance at the accuracy a direct fp64 factorisation of
            # these normal equations reaches itself (kappa*eps ~ 1e-9): fewer PCG iterations, same result
            with capi.Graph(S["I"], S["QQ"], S["n"], 1, pcg_rtol=1e-8) as G3:
                G3.set_rotations(Q0)
                G3.snapshot_rotations()
                G3.irls(4, SIG, 100, 1e-3)
                t1 = time.perf_counter()
                reps = 5
                for _ in range(reps):
                    G3.restore_rotations()
                    r3 = G3.irls(4, SIG, 100, 1e-3)
                G3.synchronize()
                d3 = time.perf_counter() - t1
                s3 = G3.stats()
            line["also_pcg_rtol_1e-8"] = {"value": S["m"] * r3["iters"] * reps / d3, "unit": "edge-updates/s",
                                          "iters_to_converge": r3["iters"], "ms_per_step": 1e3 * d3 / reps,
                                          "pcg_iters_per_solve": s3["pcg_iters"] / max(s3["pcg_solves"], 1)}
        if not args.no_extra and world == 1:
            # the callers' real pipeline: l1ra THEN irls (ral/test.cpp:295-301 with its defaults: 5 L1RA and
            # 50 IRLS iterations, change_th 1e-3; src/ViewGraph.cpp:1400-1417 allows 100 L1RA iterations)
            G.restore_rotations()
            G.l1ra(1, 1e-3)            # allocates the primal-dual planes and the solver clones
            # (three host threads drive the three coordinates: a single timing moved by +-25 % from box to box and
            # from call to call; the pipeline runs five times and the MEAN is quoted, the spread next to it)
            reps_p, tl, ti = 5, [], []
            for _ in range(reps_p):
                G.restore_rotations()
                G.synchronize()
                t1 = time.perf_counter()
                ra = G.l1ra(5, 1e-3)
                G.synchronize()
                t2 = time.perf_counter()
                rb = G.irls(4, SIG, 50, 1e-3)
                G.synchronize()
                t3 = time.perf_counter()
                tl.append(t2 - t1)
                ti.append(t3 - t2)
            ml, mi = sum(tl) / reps_p, sum(ti) / reps_p
            line["also_l1ra_then_irls"] = {
                "l1ra_iters": ra["iters"], "l1ra_ms": 1e3 * ml,
                "l1ra_ms_per_outer_iteration": 1e3 * ml / max(ra["iters"], 1),
                "l1ra_ms_min_max": [1e3 * min(tl), 1e3 * max(tl)],
                "irls_iters": rb["iters"], "irls_ms": 1e3 * mi,
                "edge_updates_per_s_whole_pipeline": S["m"] * (ra["iters"] + rb["iters"]) / (ml + mi),
                "reps": reps_p,
                "note": "l1ra(5) then irls(50): the reference demo's defaults; l1ra = 3 coordinate LPs x 2 primal-dual "
                        "iterations per outer iteration, each a Hessian solve by the handle's linear solver; mean of "
                        "5 runs of the pipeline"}
            G.restore_rotations()
            # the primal-dual iteration against the HBM roofline (round 5): algorithmic bytes of its edge / view kernels per
            # outer iteration (two primal-dual iterations of each of the three coordinate LPs) against the time an outer
            # iteration takes, and every kernel in situ with its measured traffic
            if not args.no_pmc:
                tl1, il1 = live_profile_l1ra(args)
                m_, nnz_, nu_ = S["m"], st["level_nnz"][0], S["n"] - 1
                alg_l1 = {   # bytes per launch: planes of 8 B per edge read + written (l1pd.hip), SELL entries, view planes
                    "k_pd_init": m_ * (8 + 5 * 8),
                    "k_pd_sig": m_ * (4 * 8 + 3 * 8),
                    "k_assemble0w": m_ * 16 + nnz_ * (4 + 8) + nu_ * (8 + 8 + 8 + 32),
                    "k_pd_dir": m_ * (8 + 4 * 8 + 2 * 8) + nu_ * 32,
                    "k_at_mul4": nnz_ * (4 + 8) + nu_ * 16,
                    "k_pd_trial_edge": m_ * (6 * 8 + 6 * 8),
                    "k_pd_commit_vert": nu_ * (32 + 8 + 8),
                }
                if tl1:
                    per = {}
                    tot_b = 0.0
                    calls_l1ra = max(1, (il1.get("trace_reps") or 6) * 5)   # outer iterations in the traced process
                    for kname, by in alg_l1.items():
                        rows = prof_rows(tl1, kname, {0: "2"} if kname == "k_assemble0w" else None)
                        if not rows:
                            continue
                        r0_ = rows[0]
                        per[kname] = {"launches_per_outer_iteration": r0_["calls"] / calls_l1ra, "avg_us_in_situ": r0_["avg_us"],
                                      "algorithmic_bytes": by, "traffic": r0_.get("traffic_bytes"),
                                      "frac_in_situ": by / (r0_["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS}
                        tot_b += by * r0_["calls"] / calls_l1ra
                    ms_outer = 1e3 * ml / max(ra["iters"], 1)
                    line["roofline_l1pd"] = {
                        "kernel": "the edge / view kernels of l1decode_pd (ral/l1_irls.cpp:228-468) over one outer iteration of "
                                  "l1ra: 3 coordinates x 2 primal-dual iterations, three solver chains at once",
                        "bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS,
                        "algorithmic_bytes_per_outer_iteration": tot_b, "ms_per_outer_iteration": ms_outer,
                        "achieved": tot_b / (ms_outer * 1e-3) / 1e9, "frac": tot_b / (ms_outer * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "by_kernel": per,
                        "note": "frac = the streaming kernels' bytes over the WHOLE outer iteration, six direct Hessian solves "
                                "included (they move 6 x 158 MB more and are latency-bound, see roofline); frac_in_situ of a kernel "
                                "= its bytes over its own duration while two other chains run next to it (they share the HBM)",
                        "profile": il1.get("where")}
                else:
                    line["roofline_l1pd"] = {"error": il1}
            # what a caller of the drop-in irotavg_irls pays with HOST buffers: graph build (adjacency,
            # hierarchy, SELL) + upload + the same solve + download, per call (the resident
            # figure above is the amortised / incremental case)
            # The C call itself on arrays that already have the reference's layout (Eigen column-major Mat, int32
            # pairs): what a C++ caller of irotavg::irls pays. (Until round 2 this went through irotavg_amd/ral.py,
            # whose NumPy layout conversions -- 10-15 ms at this size -- were inside the timed region.)
            import ctypes as C
            QQf, Ie = capi.fmat(S["QQ"]), capi.edges(S["I"])
            reps = 5
            d1 = 0.0
            capi.oneshot_cache(False)   # every call builds its own handle (the protocol of rounds 1-4)
            for rep in range(reps + 1):
                Qf, wh = capi.fmat(Q0), np.zeros(S["m"])
                it_c, rt_c = C.c_int(0), C.c_double(0)
                t1 = time.perf_counter()
                rc1 = capi.lib().irotavg_irls(S["m"], S["n"], 1, capi._i(Ie), capi._d(QQf), S["m"], 4, SIG, capi._d(Qf),
                                              S["n"], 100, 1e-3, capi._d(wh), C.byref(it_c), C.byref(rt_c))
                if rep > 0:
                    d1 += time.perf_counter() - t1
                assert rc1 == 0
            it1 = it_c.value
            line["also_one_shot_host_buffers"] = {
                "value": S["m"] * it1 * reps / d1, "unit": "edge-updates/s", "ms_per_call": 1e3 * d1 / reps,
                "iters_to_converge": it1, "irls_ms_inside": 1e3 * rt_c.value,
                "note": "irotavg_irls from host pointers (pageable memory): handle creation by the device build "
                        "(gbuild.hip) + PCIe both ways + the solve inside the timed region; one untimed call first; the "
                        "kept handle of round 5 switched OFF (irotavg_oneshot_cache(0)): every call builds"}
            # round 5: what the reference's callers do -- l1ra, then irls, with the SAME I and QQ (src/ViewGraph.cpp:1400-1417,
            # ral/test.cpp:295-301; through include/irotavg/l1_irls.hpp these are exactly the two C calls below): the
            # second call takes the handle the first one left (content-hashed), so the pair pays ONE build / upload
            capi.oneshot_cache(True)
            tl = ti = 0.0
            for rep in range(reps + 1):
                capi.oneshot_cache_clear()
                Qf, wh = capi.fmat(Q0), np.zeros(S["m"])
                it_l, it_c, rt_l, rt_c = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
                t1 = time.perf_counter()
                rc1 = capi.lib().irotavg_l1ra(S["m"], S["n"], 1, capi._i(Ie), capi._d(QQf), S["m"], capi._d(Qf), S["n"], 5, 1e-3,
                                              C.byref(it_l), C.byref(rt_l))
                t2 = time.perf_counter()
                rc2 = capi.lib().irotavg_irls(S["m"], S["n"], 1, capi._i(Ie), capi._d(QQf), S["m"], 4, SIG, capi._d(Qf),
                                              S["n"], 100, 1e-3, capi._d(wh), C.byref(it_c), C.byref(rt_c))
                t3 = time.perf_counter()
                assert rc1 == 0 and rc2 == 0
                if rep > 0:
                    tl += t2 - t1
                    ti += t3 - t2
            hits, misses = capi.oneshot_cache_stats()
            capi.oneshot_cache_clear()
            line["also_shim_l1ra_then_irls"] = {
                "total_ms": 1e3 * (tl + ti) / reps, "l1ra_call_ms": 1e3 * tl / reps, "irls_call_ms": 1e3 * ti / reps,
                "l1ra_ms_inside": 1e3 * rt_l.value, "irls_ms_inside": 1e3 * rt_c.value, "l1ra_iters": it_l.value,
                "irls_iters": it_c.value, "cache_hits_misses": [hits, misses],
                "one_call_with_its_own_build_ms": line["also_one_shot_host_buffers"]["ms_per_call"],
                "value": S["m"] * (it_l.value + it_c.value) * reps / (tl + ti), "unit": "edge-updates/s",
                "note": "irotavg_l1ra(5) then irotavg_irls from the same host arrays: the l1ra call builds the handle "
                        "(a miss), the irls call takes the kept one after hashing the caller's I and QQ on the host "
                        "cores (a hit: only Q goes up, Q and the weights come down); mean of %d pairs, the kept handle "
                        "cleared before each pair" % reps}
        if cpu_proc is not None:
            try:
                # the CPU baselines may still be running: the GPU repeats the headline solve meanwhile (untimed), so that
                # a utilisation sampler watching this command sees the device at work for as long as the command lasts,
                # not for the 30 ms of its timed region
                busy_solves, t_busy = 0, time.time()
                while cpu_proc.poll() is None and time.time() - t_busy < 600:
                    for _ in range(20):
                        G.restore_rotations()
                        G.irls(4, SIG, 100, 1e-3)
                    busy_solves += 20
                line["gpu_kept_busy"] = {"solves": busy_solves, "seconds": time.time() - t_busy,
                                         "note": "headline irls repeated untimed while the CPU baselines finished"}
                so, se = cpu_proc.communicate(timeout=600)
                cb = json.loads([ln for ln in so.splitlines() if ln.startswith("{")][-1])
                line["cpu_baseline"] = cb.pop("cpu_baseline")
                if "cpu_baseline_suitesparse" in cb:
                    line["cpu_baseline_suitesparse"] = cb.pop("cpu_baseline_suitesparse")
                for k, v in cb.items():   # the baselines of the other legs sit next to their GPU figures
                    if k in line:
                        line[k]["cpu_baseline"] = v
                        if v.get("unit") == line[k].get("unit") and v.get("value"):
                            line[k]["gpu_over_cpu"] = line[k]["value"] / v["value"]
            except Exception as e:
                cpu_proc.kill()
                line["cpu_baseline"] = dict(value=None, unit="edge-updates/s", cores=1, kind="port",
                                            sample="the baseline process failed: %s" % e)
        G.close()
        thr1 = host_throttled_usec()
        # the box's cgroup caps the CPU time of everything this run starts; time the group spent throttled, over the whole
        # run (profiling passes and the CPU baselines included) and inside the timed region (must be 0 for `value`)
        line["host_throttled_usec"] = None if thr0 is None or thr1 is None else thr1 - thr0
        line["host_throttled_usec_timed_region"] = None if thr_a is None or thr_b is None else thr_b - thr_a
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
