"""Case generators for the window kernels (irotavg_amd/csrc/window.hip), shared by the CPU test of the cases
themselves (test_window_cases_cpu.py) and the GPU test (test_gpu_window_limits.py). A plain module: building a case
needs no device, and raw_window_solve needs one only for a case that the library accepts.

With l1_iters = 0 and irls_iters = 1 a window solve is exactly one pass: residual, unit-weight solve, weight update,
step. Two kinds of edge then have answers that do not depend on the linear solve:

* a PLANTED edge joins two fixed views. make_A drops its row, but its weight is still computed, from E = -r; with
  identity poses that is e2 = theta^2 of the measurement, chosen by the case alone. The reference's "inverse" negates
  w, not the vector part, so between identity poses the log map sees -QQ: QQ = -(sin(theta/2) axis, cos(theta/2))
  gives theta to full relative precision however small it is, while +(...) reaches it through the wrap, as
  2 (pi - theta/2) - 2 pi, to ~4e-16 absolute. The thresholds and the tiny angles are planted the first way, the
  generic angles the second;
* a STAR edge joins fixed view 0 to a free view that has no other informative edge: at unit weights the normal matrix
  is the identity, the step is the edge's residual, and the output rotation Q_v (x) exp(r_v) shows the whole log map.
"""
import ctypes as C

import numpy as np

from irotavg_amd import capi, synth
from oracle import np_twin as T

SIG = 5 * np.pi / 180
PAIR = 1e-6      # relative offset of a +- pair around a threshold of the formula (nine orders above fp64 rounding)
FLOOR_PAIR = 1e-3  # the same around a floor, where 1 - e2/t^2 cancels: 1e-6 there would cost four digits of the weight

# Every branch of every cost of ral/l1_irls.cpp:617-727, by the cost's number
BRANCHES = {
    0: ("keeps_previous",),                                      # L2
    1: ("cap", "below_cap"),                                     # L1
    2: ("cap", "below_cap"),                                     # L1.5
    3: ("cap", "below_cap"),                                     # L0.5
    4: ("formula",),                                             # Geman-McClure
    5: ("inlier_keeps_previous", "outlier"),                     # Huber
    6: ("formula",),                                             # pseudo-Huber
    7: ("e_ge_pi", "e_lt_1e-4", "floor_below_pi", "formula"),    # Andrews
    8: ("floor", "formula"),                                     # Bisquare
    9: ("formula",),                                             # Cauchy
    10: ("formula",),                                            # Fair
    11: ("e_lt_1e-4", "formula"),                                # Logistic
    12: ("inside", "outside"),                                   # Talwar
    13: ("floor", "formula"),                                    # Welsch
}
# branches whose weight is a constant of the formula (or the untouched previous weight): compared with ==
CONST_VALUE = {"keeps_previous": 1.0, "cap": 1e4, "inlier_keeps_previous": 1.0, "e_ge_pi": 1e-4, "e_lt_1e-4": 1.0,
               "floor_below_pi": 1e-4, "floor": 1e-4, "inside": 1.0001, "outside": 0.0}


def classify(cost, sigma, E):
    """Branch name of every row of E (the residual of the linearised system) under `cost`, from the statements of
    ral/l1_irls.cpp:617-727 as oracle/np_twin.py restates them."""
    e2 = np.sum(np.asarray(E, dtype=np.float64) ** 2, axis=1)
    e = np.sqrt(e2)
    out = []
    for k in range(len(e)):
        with np.errstate(divide="ignore", invalid="ignore"):
            if cost == 0:
                b = "keeps_previous"
            elif cost in (1, 2, 3):
                w = {1: 1.0 / np.sqrt(e[k]), 2: 1.0 / np.sqrt(np.sqrt(e[k])), 3: 1.0 / e2[k] ** (3. / 8.)}[cost]
                b = "cap" if w > 1e4 else "below_cap"
            elif cost == 5:
                b = "outlier" if e[k] / (1.345 * sigma) >= 1 else "inlier_keeps_previous"
            elif cost == 7:
                r = e[k] / (1.339 * sigma)
                if r >= np.pi:
                    b = "e_ge_pi"
                elif r < 1e-4:
                    b = "e_lt_1e-4"
                else:
                    b = "floor_below_pi" if np.sqrt(np.sin(r) / r) < 1e-4 else "formula"
            elif cost == 8:
                t = 4.685 * sigma
                b = "floor" if 1.0 - e2[k] / (t * t) < 1e-4 else "formula"
            elif cost == 11:
                b = "e_lt_1e-4" if e[k] / (1.205 * sigma) < 1e-4 else "formula"
            elif cost == 12:
                t = 2.795 * sigma
                b = "inside" if e2[k] < t * t else "outside"
            elif cost == 13:
                t = 2.985 * sigma
                b = "floor" if np.exp(-.5 * e2[k] / (t * t)) < 1e-4 else "formula"
            else:
                b = "formula"
        out.append(b)
    return out


def qrot(theta, axis=(1.0, 0.0, 0.0), scale=1.0):
    """scale * (sin(theta/2) axis, cos(theta/2)), row [x y z w]."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return scale * np.concatenate([np.sin(theta / 2) * a, [np.cos(theta / 2)]])


def _planted_thetas(cost, sigma):
    """[(theta, scale of the measurement, pair id or None)] of the planted edges of `cost`."""
    th = [(0.0, 1.0, None), (1e-9, 1.0, None), (0.05, 1.0, None), (3.0, 1.0, None)]

    def pair(centre, name, off=PAIR, scale=1.0):
        th.append((centre * (1 - off), scale, name + "-"))
        th.append((centre * (1 + off), scale, name + "+"))
    if cost == 1:
        pair(1e-8, "cap")                     # 1/sqrt(theta) = 1e4
    elif cost == 2:
        # 1/theta^(1/4) = 1e4 at theta = 1e-16, where a unit measurement has |vector part| = 5e-17 < EPS and the log
        # map returns zero: a measurement of norm 16 keeps the vector part above EPS and the angle what it is
        pair(1e-16, "cap", scale=16.0)
    elif cost == 3:
        pair(10 ** (-16. / 3.), "cap")        # 1/theta^(3/4) = 1e4
    elif cost == 5:
        pair(1.345 * sigma, "huber")
    elif cost == 7:
        pair(1.339 * np.pi * sigma, "pi")
        pair(1e-4 * 1.339 * sigma, "small")
        th.append((1.339 * np.pi * sigma * (1 - 1e-9), 1.0, None))   # e < pi, sqrt(sin(e)/e) = 3e-5: floored
    elif cost == 8:
        pair(4.685 * sigma * np.sqrt(1 - 1e-4), "floor", FLOOR_PAIR)
    elif cost == 11:
        pair(1e-4 * 1.205 * sigma, "small")
    elif cost == 12:
        pair(2.795 * sigma, "talwar")
    elif cost == 13:
        pair(2.985 * sigma * np.sqrt(2 * np.log(1e4)), "floor", FLOOR_PAIR)
    return th


def planted(cost, sigma=SIG):
    """A problem that fits both window kernels (11 views, 3 of them fixed at identity): a well-connected free part
    with moderate noise, then the planted fixed-fixed edges of `cost`. Returns dict(I, QQ, Q0, f, nv, planted (edge
    ids), theta, pairs {name: (edge id of -, edge id of +)}, direct (theta reached without the wrap))."""
    f, nu = 3, 8
    nv = f + nu
    rng = np.random.default_rng(1000 + cost)
    Qgt = rng.normal(size=(nv, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    Qgt[:f] = [0, 0, 0, 1.0]
    E = []
    for v in range(f, nv):
        E.append((v % f, v))                      # anchor on a fixed view
        for d in (1, 2, 3):
            if v - d >= f:
                E.append((v - d, v))
    E.append((nv - 1, 1))                          # second endpoint fixed: make_A drops the row
    E.append((f, nv - 1))
    I = np.array(E, dtype=np.int32)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.02, size=(len(I), 3))),
                    synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(nv, 3))), Qgt)
    Q0[:f] = Qgt[:f]
    ends = [(0, 1), (1, 2), (0, 2), (2, 0), (1, 0), (2, 1), (1, 1)]
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (1, 2, -2)]
    ids, thetas, pairs, exact = [], [], {}, []
    Ip, QQp = [], []
    for n, (theta, scale, tag) in enumerate(_planted_thetas(cost, sigma)):
        k = len(I) + n
        Ip.append(ends[n % len(ends)])
        # a +- pair shares its axis; the thresholds sit on the x axis, where |vector part| is exact
        direct = tag is not None or theta < 0.01 or n % 2 == 0       # see the module's docstring
        QQp.append((-1.0 if direct else 1.0) * qrot(theta, (1, 0, 0) if tag else axes[n % len(axes)], scale))
        exact.append(direct)
        ids.append(k)
        thetas.append(theta)
        if tag:
            a, b = pairs.get(tag[:-1], (None, None))
            pairs[tag[:-1]] = (k, b) if tag[-1] == "-" else (a, k)
    I = np.concatenate([I, np.array(Ip, dtype=np.int32)])
    QQ = np.concatenate([QQ, np.array(QQp)])
    assert nu <= 16 and len(I) <= 64
    return dict(I=I, QQ=QQ, Q0=Q0, f=f, nv=nv, planted=np.array(ids), theta=np.array(thetas), pairs=pairs,
                direct=np.array(exact))


def planted_reference(c, cost, sigma=SIG):
    """np_twin's E = -r and weights (previous weights 1) of the planted edges of planted(cost)."""
    r = T.log_map(T.delta_rel(c["I"], c["QQ"], c["Q0"]))[c["planted"], :3]
    return -r, T.weights_update(cost, sigma, -r, np.ones(len(r)))


def star():
    """The log / exp map table of test_k1_edge_cases (tests/test_gpu_parity.py) and more as the edges of a star:
    fixed view 0 at identity, free view v = k + 1 held by edge k alone. Returns dict(I, QQ, Q0, f, nv, rows {name:
    view}, unchanged (views whose rotation must come back bit for bit))."""
    s2 = np.sqrt(0.5)
    table = [
        # name             Q_v at the start        QQ                                          free view first
        ("identity",       (0, 0, 0, 1.0),         (0, 0, 0, 1.0),                             False),
        ("below_eps",      (0, 0, 0, 1.0),         (1e-17, 0, 0, 1.0),                         False),
        ("exactly_pi",     (0, 0, 0, 1.0),         (1.0, 0, 0, 0.0),                           False),
        ("qj_minus_id",    (0, 0, 0, -1.0),        (np.sin(.2), 0, 0, np.cos(.2)),             False),
        ("qj_norm_2",      (0, 0, 0, 2.0),         (0, np.sin(.3), 0, np.cos(.3)),             False),
        ("negative_w",     (0, 0, 0, 1.0),         (0, 0, np.sin(1.5), -np.cos(1.5)),          False),
        ("quirk",          (0, 0, 0, 1.0),         (0, np.sin(.4), 0, np.cos(.4)),             True),
        ("general_3.1",    (0, 0, 0, 1.0),         tuple(qrot(3.1, (1, -2, 3))),               False),
        ("general_start",  (s2, 0, 0, s2),         tuple(qrot(0.7, (2, 1, -1))),               False),
        ("qq_norm_3",      (0, 0, 0, 1.0),         tuple(qrot(1.1, (0, 3, 4), 3.0)),           False),
        ("tiny_above_eps", (0, 0, 0, 1.0),         (1e-15, 0, 0, 1.0),                         False),
    ]
    nv = len(table) + 1
    Q0 = np.zeros((nv, 4))
    Q0[0, 3] = 1.0
    I, QQ, rows = [], [], {}
    for k, (name, qv, qq, free_first) in enumerate(table):
        v = k + 1
        Q0[v] = qv
        I.append((v, 0) if free_first else (0, v))
        QQ.append(qq)
        rows[name] = v
    # identity / below EPS: zero residual, zero step, exp map of zero. quirk: the only edge of the view has its row
    # dropped, the view is held by nothing (a dead pivot), its step is zero as well.
    unchanged = [rows["identity"], rows["below_eps"], rows["quirk"]]
    return dict(I=np.array(I, dtype=np.int32), QQ=np.array(QQ, dtype=np.float64), Q0=Q0, f=1, nv=nv, rows=rows,
                unchanged=unchanged)


# (nu, nv, ne): the limits of the general kernel, then of the wave kernel
LIMITS_GENERAL = [(64, 320, 640), (64, 65, 640), (64, 320, 64), (1, 320, 640), (1, 2, 1)]
LIMITS_WAVE = [(16, 320, 64), (16, 17, 64), (1, 320, 64)]


def size_case(nu, nv, ne, seed=0):
    """A well-posed problem of exactly nu free views, nv views and ne edges. Every free view gets an edge from a fixed
    view, then edges from its 1st, 2nd, ... free predecessor, round by round while edges remain: at least 3
    informative edges (rows make_A keeps) per free view wherever ne allows it (ne >= 3 nu). What is left of ne after
    the informative share is filled with edges between two fixed views and edges whose SECOND endpoint is fixed (rows
    make_A drops); with a single fixed view, with the second kind alone."""
    f = nv - nu
    assert f >= 1 and nu >= 1 and ne >= 1
    rng = np.random.default_rng([seed, nu, nv, ne])
    Qgt = rng.normal(size=(nv, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    fixed_of = lambda v: int((v - f) * max(f // nu, 1)) % f          # spread the anchors over the fixed views
    inf_edges = [(fixed_of(v), v) for v in range(f, nv)]
    inf_edges = inf_edges[:ne]
    want_inf = max(min(ne, 3 * nu + 1), ne // 2)                     # about half of a large ne is informative
    d = 1
    while len(inf_edges) < want_inf and d < max(nu, 2):
        for v in range(f + d, nv):
            if len(inf_edges) < want_inf:
                inf_edges.append((v - d, v))
        d += 1
    while len(inf_edges) < want_inf:                                 # (nu = 1: more edges from fixed views)
        inf_edges.append((int(rng.integers(0, f)), f + int(rng.integers(0, nu))))
    rest = []
    k = 0
    while len(inf_edges) + len(rest) < ne:
        if k % 2 == 0 and f >= 2:
            a, b = rng.choice(f, size=2, replace=False)               # fixed-fixed
            rest.append((int(a), int(b)))
        else:
            rest.append((f + int(rng.integers(0, nu)), int(rng.integers(0, f))))   # free first, fixed second
        k += 1
    E = inf_edges + rest
    I = np.array(E, dtype=np.int32)
    I = I[rng.permutation(len(I))]
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(len(I), 3))),
                    synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    out = np.flatnonzero((I[:, 0] >= f) & (I[:, 1] >= f))
    out = out[rng.random(len(out)) < 0.04]                            # a few gross outliers among free-free edges
    if len(out):
        R = rng.normal(size=(len(out), 4))
        QQ[out] = R / np.linalg.norm(R, axis=1, keepdims=True)
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(nv, 3))), Qgt)
    Q0[:f] = Qgt[:f]
    return dict(I=I, QQ=QQ, Q0=Q0, f=f, nv=nv, nu=nu, ne=ne)


def limits():
    """[(name, wave (fits the wave kernel too), case)] of the size cases.

    (64, 320, 64) has one edge per free view, all 64 of them informative: its normal matrix is the identity, so it tests
    the carve-up of nv and ne around a full nu, not the dense solve. (64, 320, 640) and (64, 65, 640) test the solve."""
    out = []
    for nu, nv, ne in LIMITS_GENERAL:
        out.append(("%d-%d-%d" % (nu, nv, ne), nu <= 16 and ne <= 64, size_case(nu, nv, ne)))
    for nu, nv, ne in LIMITS_WAVE:
        out.append(("wave-%d-%d-%d" % (nu, nv, ne), True, size_case(nu, nv, ne)))
    return out


def informative_degree(c):
    """Number of rows make_A keeps that touch each free view."""
    I, f = c["I"], c["f"]
    deg = np.zeros(c["nv"] - f, dtype=np.int64)
    for i, j in I:
        if j < f:
            continue
        if i >= f and i == j:
            deg[i - f] += 1
            continue
        deg[j - f] += 1
        if i >= f:
            deg[i - f] += 1
    return deg


def _chain(nv, f, ne, seed):
    """A plain valid problem of any size (views in a chain, then random extra edges) for the refusal tests."""
    rng = np.random.default_rng(seed)
    E = [(max(v - 1, 0), v) for v in range(1, nv)][:ne]
    while len(E) < ne:
        a, b = sorted(rng.choice(nv, size=2, replace=False))
        E.append((int(a), int(b)))
    I = np.array(E, dtype=np.int32).reshape(-1, 2)
    QQ = np.tile([0, 0, 0, 1.0], (max(ne, 0), 1)).reshape(-1, 4)
    Q = synth.qexp(rng.normal(scale=0.1, size=(nv, 3)))
    return dict(I=I, QQ=QQ, Q0=Q, f=f, nv=nv, ne=ne)


def past_limits():
    """[(name, kernel, case)]: one past each size limit of the window kernels; every one must be refused."""
    return [
        ("nu=65", 0, _chain(66, 1, 100, 1)),
        ("nv=321", 0, _chain(321, 300, 100, 2)),
        ("ne=641", 0, _chain(70, 6, 641, 3)),
        ("nu=0", 0, _chain(20, 20, 30, 4)),
        ("ne=0", 0, _chain(20, 1, 0, 5)),
        ("nu=65,kernel=1", 1, _chain(66, 1, 100, 1)),
        ("wave nu=17", 2, _chain(18, 1, 40, 6)),
        ("wave ne=65", 2, _chain(12, 2, 65, 7)),
    ]


def raw_window_solve(c, kernel, sigma=SIG):
    """irotavg_window_solve_kernel (cost 4, 100 + 100 iterations) on the caller's own arrays, every output preset to a
    marker: (rc, Q as the library left it, Q before, weights (preset -7), (l1, irls) iteration counts (preset -1))."""
    I = capi.edges(c["I"])
    QQ = capi.fmat(c["QQ"])
    Q = capi.fmat(c["Q0"])
    before = Q.copy(order="F")
    w = np.full(max(len(I), 1), -7.0)
    a, b = C.c_int(-1), C.c_int(-1)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = capi.lib().irotavg_window_solve_kernel(len(I), Q.shape[0], c["f"], I.ctypes.data_as(ip),
                                                QQ.ctypes.data_as(dp), max(QQ.shape[0], 1), Q.ctypes.data_as(dp),
                                                Q.shape[0], 4, sigma, 100, 100, 1e-3, w.ctypes.data_as(dp),
                                                C.byref(a), C.byref(b), kernel)
    return rc, Q, before, w, (a.value, b.value)
