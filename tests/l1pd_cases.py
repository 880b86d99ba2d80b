"""Cases for the handle's primal-dual L1 decoder (irotavg_amd/csrc/l1pd.hip), shared by the CPU test of the cases
themselves (test_l1pd_cases_cpu.py) and the GPU test (test_gpu_l1decode.py). A plain module: nothing here needs a device.

A decode case is a small graph from synth.make_graph(n, m, p_loop, seed, p_band_out=0.05) with its first f views held
at the ground truth, the others at O.init_mst's start, and a right-hand side y_c = scale x column c of the residual
there. `rev`: every rev-th edge (k = 0, rev, 2 rev, ...) is stored the other way round after init_mst (endpoints
swapped, measurement conjugated): the same measurement, but an edge whose SECOND endpoint is fixed is an all-zero row
of make_A (ral/l1_irls.cpp:755-780 drops it whole), one whose FIRST endpoint is fixed a row with a single +1.

What the GPU test relies on (asserted from the reference alone in test_l1pd_cases_cpu.py): at every pdmaxiter used the
reference accepts the first trial of every iteration, so no comparison hangs on a rounding-decided back-tracking test;
all four guarded step bounds and the unclamped step decide a step somewhere; and `amp`, the change of the reference's
own answer under a linear solver that just meets pcg_rtol, is small enough that 10 x amp cannot hide a wrong constant.

The planar cases rotate about z only: columns 0 and 1 of the residual are exactly zero, the decoder's maxabs is 0 and
its first statement divides by zero (ral/l1_irls.cpp:252-259).
"""
import functools

import numpy as np

from irotavg_amd import synth
from oracle import np_twin as T
from oracle import oracle as O

SIG = 5 * np.pi / 180
PDITERS = (1, 2, 3, 4, 8)          # pdmaxiter of the four small cases (the GPU test adds 0)
PDITERS_PCG = (2, 3)               # ... of pcg2600
PCG_RTOL = 1e-10                   # irotavg_default_options: the relative residual the PCG stops at

#        name          n     m      p_loop f  scale rev   seed
TABLE = {
    "band129":    (129,   500,  0.0,  1, 1.0,  0,  7),
    "loops129f3": (129,   500,  0.1,  3, 1.0,  7,  7),
    "odd65":      (65,    257,  0.2,  1, 1.0,  0,  7),
    "small200f2": (200,   1001, 0.05, 2, 1e-3, 5,  7),
    "pcg2600":    (2600,  15600, 0.02, 1, 1.0, 0,  7),
}
SMALL = ("band129", "loops129f3", "odd65", "small200f2")
# (all-zero rows, one-entry rows) of make_A. One fixed view and no reversed edge: no edge ends at the fixed view, so no
# row is dropped, and the one-entry rows are the edges that start there
ROWS = {"band129": (0, 4), "loops129f3": (5, 8), "odd65": (0, 4), "small200f2": (3, 8), "pcg2600": (0, None)}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, n, f, m, I, QQ, Qgt, Q0 (fixed views at the ground truth + init_mst), Y (m x 3, scaled residual))."""
    n, m, p_loop, f, scale, rev, seed = TABLE[name]
    S = synth.make_graph(n, m, p_loop, seed=seed, p_band_out=0.05)
    Q = np.zeros((n, 4))
    Q[:, 3] = 1
    Q[:f] = S["Qgt"][:f]
    rc, Qm = O.init_mst(Q, S["QQ"], S["I"], f)
    assert rc == 0
    I, QQ = S["I"].copy(), S["QQ"].copy()
    if rev:
        k = np.arange(0, len(I), rev)
        I[k] = I[k][:, ::-1]
        QQ[k] = synth.qconj(QQ[k])
    I = np.ascontiguousarray(I, dtype=np.int32)
    Y = scale * np.asarray(O.log_map(O.delta_rel(I, QQ, Qm)))[:, :3]
    return dict(name=name, n=n, f=f, m=len(I), I=I, QQ=QQ, Qgt=S["Qgt"], Q0=np.asarray(Qm), Y=np.ascontiguousarray(Y),
                is_loop=S["is_loop"])


def row_counts(c):
    """(all-zero rows, one-entry rows) of make_A for the case."""
    nnz = np.diff(T.make_A(c["n"], c["f"], c["I"]).tocsr().indptr)
    return int((nnz == 0).sum()), int((nnz == 1).sum())


def y_of(c, coord):
    return np.ascontiguousarray(c["Y"][:, coord])


@functools.lru_cache(maxsize=None)
def _twin_ops(name):
    c = case(name)
    return T.make_A(c["n"], c["f"], c["I"]), T._H_builder(c["n"], c["f"], c["I"])


def barely_converged_solver(seed=5):
    """(H, rhs) -> dx + 1e-10 |dx| / sqrt(n) (+-1 per entry): an answer whose error has the size the PCG's stopping
    rule allows (relative to the solution rather than to the residual, which is the larger of the two for an SPD H)."""
    import scipy.sparse.linalg as sla
    rng = np.random.default_rng(seed)

    def solve(H, rhs):
        dx = sla.splu(H).solve(rhs)
        sign = rng.integers(0, 2, size=len(dx)) * 2.0 - 1.0
        return dx + PCG_RTOL * np.linalg.norm(dx) / np.sqrt(len(dx)) * sign
    return solve


@functools.lru_cache(maxsize=None)
def twin(name, coord, pdmaxiter):
    """The twin's answer with its trace and its amplification: dict(x, stuck, trace, amp)."""
    c = case(name)
    A, H = _twin_ops(name)
    y = y_of(c, coord)
    tr = []
    x, stuck = T.l1decode_pd(A, H, y, pdmaxiter, trace=tr)
    xp, _ = T.l1decode_pd(A, H, y, pdmaxiter, solve=barely_converged_solver())
    amp = float(np.abs(xp - x).max() / max(np.abs(x).max(), 1e-300)) if pdmaxiter > 0 else 0.0
    return dict(x=x, stuck=bool(stuck), trace=tr, amp=amp)


def amp(name, coord, pdmaxiter):
    """max |x_perturbed - x| / max |x| of the twin under barely_converged_solver; 0 at pdmaxiter 0 (x is exactly 0)."""
    return 0.0 if pdmaxiter == 0 else twin(name, coord, pdmaxiter)["amp"]


@functools.lru_cache(maxsize=None)
def oracle_decode(name, coord, pdmaxiter):
    """(rc, x, stuck) of the C oracle (sparse Cholesky), computed once per (case, coordinate, pdmaxiter)."""
    c = case(name)
    rc, x, stuck = O.l1decode_pd(c["n"], c["f"], c["I"], y_of(c, coord), pdmaxiter)
    x.setflags(write=False)
    return rc, x, stuck


@functools.lru_cache(maxsize=None)
def oracle_l1ra(name, iters=3):
    c = case(name)
    return O.l1ra(c["QQ"], c["I"], c["Q0"], c["f"], iters, 1e-3)


def perturbed(Q, f, sd, seed):
    """Q with every free view turned by qexp(N(0, sd^2)) in all three axes (applied on the left), fixed rows untouched."""
    rng = np.random.default_rng(seed)
    out = np.array(Q, dtype=np.float64, copy=True)
    out[f:] = synth.qmul(synth.qexp(rng.normal(scale=sd, size=(len(Q) - f, 3))), out[f:])
    return out


@functools.lru_cache(maxsize=None)
def planar(n):
    """n views rotated about z by uniform(-3, 3) rad, edges (i - d, i) for d = 1, 2, 3 grouped by the newer view, each
    measured with 0.02 rad of noise about z; view 0 fixed, the others at init_mst's start."""
    rng = np.random.default_rng(3)
    ang = rng.uniform(-3.0, 3.0, size=n)
    ii = np.concatenate([np.arange(d, n) - d for d in (1, 2, 3)])
    jj = np.concatenate([np.arange(d, n) for d in (1, 2, 3)])
    order = np.lexsort((jj - ii, jj))
    I = np.stack([ii[order], jj[order]], axis=1).astype(np.int32)
    noise = rng.normal(scale=0.02, size=len(I))

    def qz(a):
        a = np.asarray(a, dtype=np.float64)
        z = np.zeros_like(a)
        return np.stack([z, z, np.sin(a / 2), np.cos(a / 2)], axis=-1)
    Qgt = qz(ang)
    QQ = synth.qmul(qz(noise), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q = np.zeros((n, 4))
    Q[:, 3] = 1
    Q[0] = Qgt[0]
    rc, Qm = O.init_mst(Q, QQ, I, 1)
    assert rc == 0
    return dict(name="planar%d" % n, n=n, nv=n, f=1, m=len(I), I=I, QQ=QQ, Qgt=Qgt, Q0=np.asarray(Qm),
                Y=np.asarray(O.log_map(O.delta_rel(I, QQ, Qm)))[:, :3])
