"""torch front-end of the device-pointer handle API (irotavg_graph_*_dev of include/irotavg_hip.h,
docs/device_api.md): tensors on the ROCm device go in and come out, nothing passes through the host, and every call
runs on torch's current stream -- no synchronise before or after. Plumbing only: all numerics live in
libirotavg_hip.so (irotavg_amd/csrc/devapi.hip and the kernels behind the host-pointer API)."""
import ctypes as C

import torch

from . import capi

INT32_MAX = 2 ** 31 - 1


def matrix_strides(t):
    """(row_stride, col_stride) in elements of a 2-D tensor, as the C ABI takes a strided matrix."""
    if t.dim() != 2:
        raise ValueError("a 2-D tensor is needed, got %d-D" % t.dim())
    return int(t.stride(0)), int(t.stride(1))


def _check(t, name, dtypes, shape, device=None, placed=True):
    """dtype, then shape, then (placed) placement: TypeError / ValueError before anything reaches the C library."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in dtypes:
        raise TypeError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if t.dim() != len(shape) or any(s is not None and int(t.shape[k]) != s for k, s in enumerate(shape)):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple("*" if s is None else s for s in shape),
                                                            tuple(t.shape)))
    if not placed:
        return t
    if not t.is_cuda:
        raise TypeError("%s must live on the ROCm device, got a %s tensor" % (name, t.device.type))
    if device is not None and t.device != device:
        raise ValueError("%s is on %s, the handle on %s" % (name, t.device, device))
    return t


def _vector(t, name, n, device, dtype=torch.float64):
    """_check of n entries on `device`, and contiguous."""
    _check(t, name, (dtype,), (n,), device)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _output(want, name, n, device, dtype=torch.float64, fill=None):
    """An output argument: True -> a new tensor of n entries (preset to `fill`, or uninitialised), False / None -> None,
    a tensor -> itself once _vector accepts it."""
    if want is True:
        return torch.empty(n, dtype=dtype, device=device) if fill is None else torch.full((n,), fill, dtype=dtype, device=device)
    if want is False or want is None:
        return None
    return _vector(want, name, n, device, dtype)


def _allowed(rc, name, allow_rc):
    """rc, or IrotavgError for anything but OK that allow_rc does not list."""
    if rc != capi.OK and rc not in allow_rc:
        raise capi.IrotavgError(rc, name)
    return rc


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _narrow(ids):
    """int64 ids narrowed on the device: what does not fit becomes -1, an id the kernels' guard refuses."""
    if ids.dtype == torch.int64:
        ids = torch.where((ids < 0) | (ids > INT32_MAX), torch.full_like(ids, -1), ids).to(torch.int32)
    return ids.contiguous()


class TorchGraph(capi.Graph):
    """A graph handle built from tensors on the device (irotavg_graph_create_dev). edge_index: (m, 2) int32 or int64
    (narrowed on the device; a value outside int32 range makes the build reject the graph), QQ: (m, 4) float64 with
    any strides, columns [x, y, z, w]. The handle copies both; the tensors are only read. Everything a capi.Graph
    offers through host arrays (irls, l1ra, stats, fingerprint, ...) works on this handle too."""

    def __init__(self, edge_index, QQ, n_total, f, **opts):
        self._h = C.c_void_p()
        _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2), placed=False)
        _check(QQ, "QQ", (torch.float64,), (int(edge_index.shape[0]), 4), placed=False)  # dtypes and shapes of both first
        _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2))
        _check(QQ, "QQ", (torch.float64,), (int(edge_index.shape[0]), 4), edge_index.device)
        self.device = QQ.device
        self.m, self.n_total, self.f = int(edge_index.shape[0]), int(n_total), int(f)
        self.nu = self.n_total - self.f
        with torch.cuda.device(self.device):
            ei = _narrow(edge_index)  # what does not fit int32 becomes an index the build rejects
            o = capi.default_options(**opts)
            if o.device < 0:
                o.device = self.device.index
            rs, cs = matrix_strides(QQ)
            rc = capi.lib().irotavg_graph_create_dev(C.byref(self._h), self.m, self.n_total, self.f, _ptr(ei), _ptr(QQ),
                                                     rs, cs, C.byref(o), _stream(self.device))
        if rc != capi.OK:
            self._h = C.c_void_p()
            if rc == capi.ERR_BAD_ARG:
                raise ValueError("irotavg_graph_create_dev: bad argument (sizes, strides that alias, or an edge index "
                                 "outside [0, n_total) / outside int32 range)")
            raise capi.IrotavgError(rc, "irotavg_graph_create_dev")

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            return getattr(capi.lib(), name)(self._h, *args, _stream(self.device))

    def _new(self, *shape):
        return torch.empty(shape, dtype=torch.float64, device=self.device)

    # ---- copies: asynchronous, ordered on the current stream -----------------------------------------------------------
    def set_rotations(self, Q):
        _check(Q, "Q", (torch.float64,), (self.n_total, 4), self.device)
        capi.check(self._call("irotavg_graph_set_rotations_dev", _ptr(Q), *matrix_strides(Q)), "set_rotations_dev")

    def rotations(self, out=None):
        out = self._new(self.n_total, 4) if out is None else _check(out, "out", (torch.float64,), (self.n_total, 4),
                                                                    self.device)
        capi.check(self._call("irotavg_graph_get_rotations_dev", _ptr(out), *matrix_strides(out)), "get_rotations_dev")
        return out

    def set_weights(self, w):
        _check(w, "w", (torch.float64,), (self.m,), self.device)
        w = w.contiguous()
        capi.check(self._call("irotavg_graph_set_weights_dev", _ptr(w)), "set_weights_dev")

    def weights(self, out=None):
        out = self._new(self.m) if out is None else _check(out, "out", (torch.float64,), (self.m,), self.device)
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        capi.check(self._call("irotavg_graph_get_weights_dev", _ptr(out)), "get_weights_dev")
        return out

    def residuals(self, out=None):
        """(m, 3) residuals of the last edge_residual(); a new tensor is three planes (the handle's own layout)."""
        out = self._new(3, self.m).t() if out is None else _check(out, "out", (torch.float64,), (self.m, 3), self.device)
        capi.check(self._call("irotavg_graph_get_residuals_dev", _ptr(out), *matrix_strides(out)), "get_residuals_dev")
        return out

    # ---- queries ---------------------------------------------------------------------------------------------------------
    def variance(self, out=None, allow_rc=()):
        """irotavg_graph_rotation_variance_dev: dict(rc, var (n_total, on the device), scale). var is written only on
        success (pass `out` to see that)."""
        var = self._new(self.n_total) if out is None else _check(out, "out", (torch.float64,), (self.n_total,), self.device)
        if not var.is_contiguous():
            raise ValueError("out must be contiguous")
        scale = C.c_double(float("nan"))
        rc = _allowed(self._call("irotavg_graph_rotation_variance_dev", _ptr(var), C.byref(scale)),
                      "irotavg_graph_rotation_variance_dev", allow_rc)
        return dict(rc=rc, var=var, scale=scale.value)

    def edge_diagnostics(self, edge_var=True, leverage=True, chi2=True, allow_rc=()):
        """irotavg_graph_edge_diagnostics_dev: dict(rc, edge_var, leverage, chi2 (m each on the device, or None), scale).
        Each argument is True (a new tensor), False (not computed) or a contiguous float64 tensor of m entries to fill."""
        outs = [_output(want, name, self.m, self.device)
                for name, want in (("edge_var", edge_var), ("leverage", leverage), ("chi2", chi2))]
        scale = C.c_double(float("nan"))
        rc = _allowed(self._call("irotavg_graph_edge_diagnostics_dev", *[None if t is None else _ptr(t) for t in outs],
                                 C.byref(scale)), "irotavg_graph_edge_diagnostics_dev", allow_rc)
        return dict(rc=rc, edge_var=outs[0], leverage=outs[1], chi2=outs[2], scale=scale.value)

    def cycle_check(self, edge_index, QQ, threshold=5 * 3.141592653589793 / 180, **kw):
        """cycle_check (below) of the tensors passed, with the handle's n_total: the handle keeps no copy of the caller's
        arrays in their layout, and the screen needs neither its poses nor its weights."""
        _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2), self.device)
        return cycle_check(edge_index, QQ, self.n_total, threshold, **kw)

    def init_tree(self, edge_index, QQ, rank=None, **kw):
        """init_tree (below) of the tensors passed with the handle's n_total and f, then set_rotations: the handle starts
        from the tree's rotations without a host round trip. The anchor Q[0] and the other fixed rows are the identity.
        Returns init_tree's dict; its Q is the (n_total, 4) tensor handed to the handle."""
        _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2), self.device)
        Q = torch.zeros((self.n_total, 4), dtype=torch.float64, device=self.device)
        Q[:, 3] = 1.0
        out = init_tree(edge_index, QQ, self.n_total, Q, self.f, rank, **kw)
        if out["rc"] == capi.OK:
            self.set_rotations(Q)
        return out

    # the host-array forms of the parent stay reachable under their own names
    host_set_rotations = capi.Graph.set_rotations
    host_set_weights = capi.Graph.set_weights
    host_edge_diagnostics = capi.Graph.edge_diagnostics


# ---- many small problems in one call (irotavg_window_solve_batch_dev, docs/window_batch.md) ------------------------------
def batch_offsets(sizes):
    """sizes: host (nb, 3) integers (n_total, f, m) per problem -> (sizes as contiguous int32, first edge row of every
    problem, first view row of every problem, sum m, sum n_total): the packing the C call assumes."""
    import numpy as np
    if isinstance(sizes, torch.Tensor):
        if sizes.is_cuda:
            raise TypeError("sizes must be a host array, got a tensor on %s" % sizes.device)
        sizes = sizes.numpy()
    s = np.asarray(sizes)
    if s.dtype.kind not in "iu":
        raise TypeError("sizes must be integers, got %s" % s.dtype)
    if s.ndim != 2 or s.shape[1] != 3:
        raise ValueError("sizes must have shape (nb, 3), got %s" % (s.shape,))
    if s.size and (s.min() < -INT32_MAX or s.max() > INT32_MAX):
        raise ValueError("sizes outside int32 range")
    s64 = s.astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum(s64[:, 2])[:-1]]) if len(s) else np.zeros(0, dtype=np.int64)
    voff = np.concatenate([[0], np.cumsum(s64[:, 0])[:-1]]) if len(s) else np.zeros(0, dtype=np.int64)
    return np.ascontiguousarray(s, dtype=np.int32), eoff, voff, int(s64[:, 2].sum()), int(s64[:, 0].sum())


_IDS, _F64 = (torch.int32, torch.int64), (torch.float64,)


def _batch_tensors(sizes, edge_index, QQ, Q):
    """batch_offsets(sizes) and the first round of the checks every batched call makes of its packed tensors: dtype and
    shape, of all of them before the placement of any. Returns (sizes as int32, sum m, sum n_total, the (tensor, name,
    dtypes, shape) of the three): the call checks its further tensors with _shapes, appends them, then calls _placed."""
    s32, _, _, sum_m, sum_n = batch_offsets(sizes)
    specs = [(edge_index, "edge_index", _IDS, (sum_m, 2)), (QQ, "QQ", _F64, (sum_m, 4)), (Q, "Q", _F64, (sum_n, 4))]
    _shapes(specs)
    return s32, sum_m, sum_n, specs


def _shapes(specs):
    for spec in specs:
        _check(*spec, placed=False)
    return specs


def _placed(specs):
    """the second round: the first tensor on the ROCm device, the others on the same one -> that device"""
    _check(*specs[0])
    device = specs[0][0].device
    for spec in specs[1:]:
        _check(*spec, device)
    return device


def window_solve_batch(sizes, edge_index, QQ, Q, cost=4, sigma=5 * 3.141592653589793 / 180, l1_iters=100, irls_iters=100,
                       change_th=1e-3, kernel=0, weights=True, allow_rc=()):
    """nb independent window-size problems (<= 64 free views, <= 320 views, <= 640 edges each), every one l1ra + irls as
    capi.window_solve, one workgroup per problem, in at most two launches on torch's current stream.

    sizes: host (nb, 3) integers (n_total, f, m); edge_index: (sum m, 2) int32 or int64 (narrowed on the device), problem
    after problem, ids local to their problem; QQ: (sum m, 4) and Q: (sum n_total, 4) float64 with any strides, Q is
    updated in place (rows of fixed views are never written). weights: True (a new tensor), False / None, or a contiguous
    float64 tensor of sum m entries. Returns dict(rc, Q, weights, status, l1_iters, irls_iters, kernel); the last four
    are host numpy arrays of nb entries. rc is the first non-zero status in problem order; anything but OK raises unless
    listed in allow_rc."""
    import numpy as np
    s32, sum_m, sum_n, specs = _batch_tensors(sizes, edge_index, QQ, Q)
    device = _placed(specs)
    w = _output(weights, "weights", sum_m, device)
    nb = len(s32)
    res = np.zeros((nb, 4), dtype=np.int32)
    with torch.cuda.device(device):
        ei = _narrow(edge_index)
        rc = capi.lib().irotavg_window_solve_batch_dev(
            nb, s32.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(ei), _ptr(QQ), *matrix_strides(QQ), _ptr(Q),
            *matrix_strides(Q), int(cost), float(sigma), int(l1_iters), int(irls_iters), float(change_th),
            None if w is None else _ptr(w), res.ctypes.data_as(C.POINTER(C.c_int32)), int(kernel), _stream(device))
    _allowed(rc, "irotavg_window_solve_batch_dev", allow_rc)
    return dict(rc=rc, Q=Q, weights=w, status=res[:, 0].copy(), l1_iters=res[:, 1].copy(), irls_iters=res[:, 2].copy(),
                kernel=res[:, 3].copy())


# ---- their uncertainty in one call (irotavg_window_uncertainty_batch_dev, docs/window_uncertainty_batch.md) --------------
def pair_offsets(npairs, nb, name="npairs"):
    """npairs: host integers, one count per problem (or None: no pairs) -> (counts as contiguous int32, first pair row of
    every problem, sum): the packing the C call assumes, formed in 64 bits. The candidate counts of window_gate_batch go
    through here too (`name`: what an error calls them)."""
    import numpy as np
    if npairs is None:
        return None, np.zeros(nb, dtype=np.int64), 0
    if isinstance(npairs, torch.Tensor):
        if npairs.is_cuda:
            raise TypeError("%s must be a host array, got a tensor on %s" % (name, npairs.device))
        npairs = npairs.numpy()
    c = np.asarray(npairs)
    if c.dtype.kind not in "iu":
        raise TypeError("%s must be integers, got %s" % (name, c.dtype))
    if c.shape != (nb,):
        raise ValueError("%s must have shape (%d,), got %s" % (name, nb, c.shape))
    if c.size and (c.min() < 0 or c.max() > INT32_MAX):
        raise ValueError("%s must be counts in int32 range" % name)
    c64 = c.astype(np.int64)
    return np.ascontiguousarray(c, dtype=np.int32), np.cumsum(c64) - c64, int(c64.sum())


def window_uncertainty_batch(sizes, edge_index, QQ, Q, weights=None, sigma=5 * 3.141592653589793 / 180, pairs=None,
                             npairs=None, var=True, edge_var=True, leverage=True, chi2=True, allow_rc=()):
    """The uncertainty of nb independent window-size problems, each as capi.window_uncertainty, one workgroup per problem,
    in one launch on torch's current stream. sizes, edge_index, QQ, Q: as window_solve_batch takes them (Q is only read).

    weights: a contiguous float64 tensor of sum m entries (what window_solve_batch returned), or None for the
    Geman-McClure weights of the poses at `sigma`. pairs: (sum npairs, 2) int32 or int64 view ids local to their problem,
    with npairs the host counts per problem; or None. var / edge_var / leverage / chi2: True (a new tensor, preset to
    NaN), False / None (not computed), or a contiguous float64 tensor to fill (sum n_total entries for var, sum m for the
    others). Returns dict(rc, var, pair_var, edge_var, leverage, chi2, scale, status); scale and status are host numpy
    arrays of nb entries (scale NaN where the problem failed). rc is the first non-zero status in problem order; anything
    but OK raises unless listed in allow_rc. A problem that fails leaves its rows of every output as they were."""
    import numpy as np
    s32, sum_m, sum_n, specs = _batch_tensors(sizes, edge_index, QQ, Q)
    nb = len(s32)
    if (pairs is None) != (npairs is None):
        raise ValueError("pairs and npairs go together")
    np32, _, sum_p = pair_offsets(npairs, nb)
    if pairs is not None:
        specs += _shapes([(pairs, "pairs", _IDS, (sum_p, 2))])
    device = _placed(specs)
    w = None if weights is None else _vector(weights, "weights", sum_m, device)
    nan = float("nan")
    outs = {name: _output(want, name, n, device, fill=nan)
            for name, want, n in (("var", var, sum_n), ("edge_var", edge_var, sum_m), ("leverage", leverage, sum_m),
                                  ("chi2", chi2, sum_m))}
    pv = torch.full((sum_p,), nan, dtype=torch.float64, device=device) if sum_p else None
    scale = np.full(nb, np.nan)
    status = np.zeros(nb, dtype=np.int32)
    opt = lambda t: None if t is None else _ptr(t)
    with torch.cuda.device(device):
        ei = _narrow(edge_index)
        pr = _narrow(pairs) if sum_p else None
        rc = capi.lib().irotavg_window_uncertainty_batch_dev(
            nb, s32.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(ei), _ptr(QQ), *matrix_strides(QQ), _ptr(Q),
            *matrix_strides(Q), opt(w), float(sigma), opt(outs["var"]),
            None if np32 is None else np32.ctypes.data_as(C.POINTER(C.c_int32)), opt(pr), opt(pv), opt(outs["edge_var"]),
            opt(outs["leverage"]), opt(outs["chi2"]), scale.ctypes.data_as(C.POINTER(C.c_double)),
            status.ctypes.data_as(C.POINTER(C.c_int32)), _stream(device))
    _allowed(rc, "irotavg_window_uncertainty_batch_dev", allow_rc)
    return dict(rc=rc, pair_var=pv, scale=scale, status=status, **outs)


# ---- the closure gate on the same arrays (irotavg_window_gate_batch_dev, docs/window_gate_batch.md) ------------------------
def window_gate_batch(sizes, edge_index, QQ, Q, cand_index, cand_QQ, ncand, weights=None, sigma=5 * 3.141592653589793 / 180,
                      angle=True, pair_var=True, chi2=True, allow_rc=()):
    """The closure gate of nb independent window-size problems, each as capi.window_gate, one workgroup per problem, in one
    launch on torch's current stream. sizes, edge_index, QQ, Q, weights: as window_uncertainty_batch takes them (Q is only
    read).

    cand_index: (sum ncand, 2) int32 or int64 view ids local to their problem, cand_QQ: (sum ncand, 4) float64 with any
    strides, ncand: the host counts per problem. angle / pair_var / chi2: True (a new tensor, preset to NaN), False / None
    (not computed), or a contiguous float64 tensor of sum ncand entries to fill. Returns dict(rc, angle, pair_var, chi2,
    scale, status); scale and status are host numpy arrays of nb entries (scale NaN where the problem failed). rc is the
    first non-zero status in problem order; anything but OK raises unless listed in allow_rc. A problem that fails leaves
    its rows of every output as they were."""
    import numpy as np
    s32, sum_m, sum_n, specs = _batch_tensors(sizes, edge_index, QQ, Q)
    nb = len(s32)
    if ncand is None:
        raise ValueError("ncand is needed: one count per problem")
    nc32, _, sum_c = pair_offsets(ncand, nb, "ncand")
    specs += _shapes([(cand_index, "cand_index", _IDS, (sum_c, 2)), (cand_QQ, "cand_QQ", _F64, (sum_c, 4))])
    device = _placed(specs)
    w = None if weights is None else _vector(weights, "weights", sum_m, device)
    outs = {name: _output(want, name, sum_c, device, fill=float("nan"))
            for name, want in (("angle", angle), ("pair_var", pair_var), ("chi2", chi2))}
    scale = np.full(nb, np.nan)
    status = np.zeros(nb, dtype=np.int32)
    opt = lambda t: None if t is None or t.numel() == 0 else _ptr(t)
    with torch.cuda.device(device):
        ei = _narrow(edge_index)
        ci = _narrow(cand_index)
        rc = capi.lib().irotavg_window_gate_batch_dev(
            nb, s32.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(ei), _ptr(QQ), *matrix_strides(QQ), _ptr(Q),
            *matrix_strides(Q), None if w is None else _ptr(w), float(sigma), nc32.ctypes.data_as(C.POINTER(C.c_int32)),
            opt(ci), opt(cand_QQ), *matrix_strides(cand_QQ), opt(outs["angle"]), opt(outs["pair_var"]), opt(outs["chi2"]),
            scale.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_int32)), _stream(device))
    _allowed(rc, "irotavg_window_gate_batch_dev", allow_rc)
    return dict(rc=rc, scale=scale, status=status, **outs)


# ---- their initialisation in one call (irotavg_window_init_mst_batch_dev, docs/window_init_batch.md) ----------------------
def window_init_mst_batch(sizes, edge_index, QQ, Q, allow_rc=()):
    """capi.init_mst on nb independent window-size problems, one workgroup per problem, in one launch on torch's current
    stream: the call in front of window_solve_batch. sizes, edge_index, QQ, Q: as window_solve_batch takes them, every
    problem with f >= 1 (view 0 is the anchor).

    Q is updated in place: the rows of free views are written (they are never read, so they may be uninitialised), the
    rows of fixed views are read and never written. Returns dict(rc, Q, status); status is a host numpy array of nb
    entries. rc is the first non-zero status in problem order (ERR_BAD_ARG: an edge id outside the problem,
    ERR_NOT_SPANNING: a view no edge reaches from view 0); anything but OK raises unless listed in allow_rc. A problem
    that fails keeps its rows of Q as they were. On success the rows are bitwise those of capi.init_mst on each problem
    alone."""
    import numpy as np
    s32, _, _, specs = _batch_tensors(sizes, edge_index, QQ, Q)
    device = _placed(specs)
    nb = len(s32)
    status = np.zeros(nb, dtype=np.int32)
    with torch.cuda.device(device):
        ei = _narrow(edge_index)
        rc = capi.lib().irotavg_window_init_mst_batch_dev(
            nb, s32.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(ei), _ptr(QQ), *matrix_strides(QQ), _ptr(Q),
            *matrix_strides(Q), status.ctypes.data_as(C.POINTER(C.c_int32)), _stream(device))
    _allowed(rc, "irotavg_window_init_mst_batch_dev", allow_rc)
    return dict(rc=rc, Q=Q, status=status)


# ---- the triangle test before any solve (irotavg_cycle_check_dev, docs/cycle_check.md) ------------------------------------
def cycle_check(edge_index, QQ, n_total, threshold=5 * 3.141592653589793 / 180, count=True, ok=True, min_err=True,
                summary=True, allow_rc=()):
    """Cycle-consistency screening of relative rotations on torch's current stream: for every edge the triangles it closes
    with two other edges, how many of them are consistent within `threshold` radians, and the smallest inconsistency. No
    poses, no weights, no fixed views, any topology.

    edge_index: (m, 2) int32 or int64 (narrowed on the device: a value outside int32 range becomes an id the device check
    refuses), QQ: (m, 4) float64 with any strides. count / ok / min_err: True (a new tensor), False / None (not computed),
    or a contiguous tensor of m entries to fill (int32 for the counts, float64 for min_err). Returns dict(rc, tri_count,
    tri_ok, tri_min, summary); summary is a host dict of capi.SUMMARY_FIELDS, or None. An id outside [0, n_total) gives
    ERR_BAD_ARG with every output byte as it was; anything but OK raises unless listed in allow_rc. The call blocks until
    the summary is back."""
    _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2), placed=False)
    m = int(edge_index.shape[0])
    _check(QQ, "QQ", (torch.float64,), (m, 4), placed=False)
    wants = (("count", count, torch.int32), ("ok", ok, torch.int32), ("min_err", min_err, torch.float64))
    for name, want, dt in wants:
        if not (want is True or want is False or want is None):
            _check(want, name, (dt,), (m,), placed=False)
    n_total, threshold = int(n_total), float(threshold)
    if m < 1:
        raise ValueError("edge_index must have at least one row")
    if not 0 < n_total <= INT32_MAX:
        raise ValueError("n_total must lie in [1, 2^31 - 1], got %d" % n_total)
    if not threshold >= 0.0:
        raise ValueError("threshold must be a non-negative angle, got %r" % threshold)
    _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2))
    device = edge_index.device
    _check(QQ, "QQ", (torch.float64,), (m, 4), device)
    outs = [_output(want, name, m, device, dt) for name, want, dt in wants]
    s = (C.c_int64 * 4)(-1, -1, -1, -1)
    with torch.cuda.device(device):
        ei = _narrow(edge_index)
        rc = capi.lib().irotavg_cycle_check_dev(m, n_total, _ptr(ei), _ptr(QQ), *matrix_strides(QQ), threshold,
                                                *[None if t is None else _ptr(t) for t in outs], s if summary else None,
                                                _stream(device))
    _allowed(rc, "irotavg_cycle_check_dev", allow_rc)
    return dict(rc=rc, tri_count=outs[0], tri_ok=outs[1], tri_min=outs[2],
                summary=dict(zip(capi.SUMMARY_FIELDS, (int(v) for v in s))) if summary and rc == capi.OK else None)


# ---- the order-free spanning-tree initialiser (irotavg_init_tree_dev, docs/init_tree.md) ----------------------------------
def rank_from_cycle_check(tri_count, tri_ok):
    """The rank init_tree takes, from the counts of cycle_check, in plain torch on the device: 0 for a supported edge
    (tri_ok >= 1), 1 for an untested one (tri_count == 0), 2 for a contradicted one (triangles, none of them consistent).
    Returns an int32 tensor of m entries."""
    _check(tri_count, "tri_count", (torch.int32,), (None,), placed=False)
    _check(tri_ok, "tri_ok", (torch.int32,), (int(tri_count.shape[0]),), placed=False)
    if tri_ok.device != tri_count.device:
        raise ValueError("tri_ok is on %s, tri_count on %s" % (tri_ok.device, tri_count.device))
    rank = torch.full_like(tri_count, 2)
    rank[tri_count == 0] = 1
    rank[tri_ok >= 1] = 0
    return rank


def init_tree(edge_index, QQ, n_total, Q, f=1, rank=None, in_tree=False, allow_rc=()):
    """Initial rotations along the minimum spanning tree under the keys (rank[k], k), on torch's current stream: the tree
    does not depend on the order of the edge list beyond the index k that breaks ties, and the number of launches grows
    with log(n_total). A second initialiser next to capi / ral init_mst, whose sweep it does not reproduce.

    edge_index: (m, 2) int32 or int64 (narrowed on the device: a value outside int32 range becomes an id the device check
    refuses), QQ: (m, 4) and Q: (n_total, 4) float64 with any strides. Row 0 of Q is read, the rows from f on are written
    in place (they are never read and may hold NaN), rows 1 .. f-1 are neither read nor written. rank: None (all zero) or a
    contiguous int32 tensor of m entries, rank[k] < 0: edge k is never used (rank_from_cycle_check gives one). in_tree:
    True (a new int32 tensor), False / None, or a contiguous int32 tensor of m entries to fill. Returns dict(rc, Q,
    in_tree, info); info is a host dict of capi.INFO_FIELDS, also with ERR_NOT_SPANNING (then Q and in_tree are as they
    were). An id outside [0, n_total) gives ERR_BAD_ARG with every output byte as it was; anything but OK raises unless
    listed in allow_rc. The call blocks until the status is back."""
    _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2), placed=False)
    m = int(edge_index.shape[0])
    _check(QQ, "QQ", (torch.float64,), (m, 4), placed=False)
    n_total, f = int(n_total), int(f)
    _check(Q, "Q", (torch.float64,), (n_total, 4), placed=False)
    if rank is not None:
        _check(rank, "rank", (torch.int32,), (m,), placed=False)
    if not (in_tree is True or in_tree is False or in_tree is None):
        _check(in_tree, "in_tree", (torch.int32,), (m,), placed=False)
    if m < 1:
        raise ValueError("edge_index must have at least one row")
    if not 0 < n_total <= INT32_MAX:
        raise ValueError("n_total must lie in [1, 2^31 - 1], got %d" % n_total)
    if not 1 <= f <= n_total:
        raise ValueError("f must lie in [1, n_total], got %d" % f)
    _check(edge_index, "edge_index", (torch.int32, torch.int64), (None, 2))
    device = edge_index.device
    _check(QQ, "QQ", (torch.float64,), (m, 4), device)
    _check(Q, "Q", (torch.float64,), (n_total, 4), device)
    rk = None if rank is None else _vector(rank, "rank", m, device, torch.int32)
    tree = _output(in_tree, "in_tree", m, device, torch.int32)
    s = (C.c_int64 * 4)(-1, -1, -1, -1)
    with torch.cuda.device(device):
        ei = _narrow(edge_index)
        rc = capi.lib().irotavg_init_tree_dev(m, n_total, f, _ptr(ei), _ptr(QQ), *matrix_strides(QQ),
                                              None if rk is None else _ptr(rk), _ptr(Q), *matrix_strides(Q),
                                              None if tree is None else _ptr(tree), s, _stream(device))
    _allowed(rc, "irotavg_init_tree_dev", allow_rc)
    return dict(rc=rc, Q=Q, in_tree=tree,
                info=dict(zip(capi.INFO_FIELDS, (int(v) for v in s))) if rc in (capi.OK, capi.ERR_NOT_SPANNING) else None)
