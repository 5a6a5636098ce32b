"""Device backend: thin object wrapper over the libnbp C ABI (include/nbp.h).

The host-side mirror of the reference API (factorgraph.py / solver.py) talks to a *backend*
through this narrow interface: belief slots in, descriptor batches run, belief slots out.
The product backend is :class:`HipBackend`.  (The CPU oracle implements the same interface in
``oracle/`` -- test infrastructure, never imported from this package.)
"""
import ctypes as C
import weakref

import numpy as np

from . import abi


class NbpError(RuntimeError):
    """Hard error from libnbp (status < 0).  The Julia shim maps this to `error()`, which fails
    the clique Task and makes `monitorCSMs` tear the solve down with a CompositeException
    (reference: CliqStateMachineUtils.jl:184-246, test/testCSMMonitor.jl:51)."""


_IP, _DP = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _i32(seq):
    """a sequence as a contiguous int32 array and the pointer to it that libnbp takes (the pointer holds a reference to the array)"""
    a = np.ascontiguousarray(seq, dtype=np.int32)
    return a, a.ctypes.data_as(_IP)


def _f64(a, shape=None):
    """the float64 twin of _i32: a contiguous array (reshaped to `shape`) and the pointer to it"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    a = a if shape is None else a.reshape(shape)
    return a, a.ctypes.data_as(_DP)


def _ptr(a, to=None):
    """the pointer libnbp takes to an output array -- float64 or int32, or structured with records of the ctypes type `to`; None for
    None: an optional output nobody asked for"""
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(to) if to else _IP if a.dtype == np.int32 else _DP)


def _host_belief(manifold, pts, bw=None):
    """a belief held on the host as the nbp_kde_* entries take it -> (the pointer to its points c x P, c, the pointer to its bandwidth or
    None); the pointers hold references to the arrays made here"""
    pts, pp = _f64(pts, (-1, abi.MANIFOLD_P[manifold]))
    return pp, pts.shape[0], None if bw is None else _f64(bw)[1]


def _pack_queries(manifolds, queries, all_columns=False):
    """one array of queries per belief (q_i x D or x 3, or flat: rows of D) -> (the padded Q x 3 array, first[n + 1]): the layout of
    nbp_run_evaluate.  all_columns: the assignment covers all D columns whatever the queries' width, as kde_evaluate has always
    made it (numpy broadcasts one column and refuses any other narrower width); else narrower queries are zero-padded"""
    first = np.zeros(len(manifolds) + 1, dtype=np.int32)
    rows = []
    for i, m in enumerate(manifolds):
        D = abi.MANIFOLD_DIM.get(int(m), abi.MAXD)  # (an unknown manifold is the library's to refuse)
        q = np.asarray(queries[i], dtype=np.float64)
        q = q.reshape(-1, q.shape[-1] if q.ndim > 1 else D)
        pad = np.zeros((q.shape[0], abi.MAXD))
        pad[:, :D if all_columns else min(D, q.shape[1])] = q[:, :D]
        rows.append(pad)
        first[i + 1] = first[i] + q.shape[0]
    return (np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, abi.MAXD))), first


def _as_array(descs, ctype):
    if isinstance(descs, C.Array):
        return descs, len(descs)
    arr = (ctype * len(descs))(*descs)
    return arr, len(descs)


class HipBackend:
    name = "hip"

    def __init__(self, N, n_slots, side_ints=0, device=0, arena_ptr=None, arena_bytes=0):
        self.lib = abi.load_library()
        self.N, self.n_slots = int(N), int(n_slots)
        self._ctx = C.c_void_p()
        self._programs = weakref.WeakSet()  # live HipPrograms: closed before the context (close())
        self._check(self.lib.nbp_ctx_create(device, self.N, self.n_slots, arena_ptr, arena_bytes,
                                            max(int(side_ints), 1), C.byref(self._ctx)))

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.nbp_last_error()
            raise NbpError(f"libnbp status {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if self._ctx:
            for prog in list(getattr(self, "_programs", ())):  # a program must not outlive its context
                prog.close()
            self.comm_destroy()
            self.lib.nbp_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- belief I/O -----------------------------------------------------------------------
    def slot_write(self, slot, manifold, pts, bw=None):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(self.N, abi.MANIFOLD_P[manifold])
        bwp = None
        if bw is not None:
            bw = np.ascontiguousarray(bw, dtype=np.float64)
            bwp = bw.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.lib.nbp_slot_write(self._ctx, slot, manifold,
                                            pts.ctypes.data_as(C.POINTER(C.c_double)), bwp))

    def slot_read(self, slot, manifold):
        pts = np.empty((self.N, abi.MANIFOLD_P[manifold]))
        bw = np.empty(abi.MANIFOLD_DIM[manifold])
        self._check(self.lib.nbp_slot_read(self._ctx, slot, manifold,
                                           pts.ctypes.data_as(C.POINTER(C.c_double)),
                                           bw.ctypes.data_as(C.POINTER(C.c_double))))
        return pts, bw

    def belief_write(self, slot, manifold, pts, bw=None, ipc=None):
        """the full TreeBelief triple (val, bw, infoPerCoord)"""
        dp = C.POINTER(C.c_double)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[manifold])
        bw = None if bw is None else np.ascontiguousarray(bw, dtype=np.float64)
        ipc = None if ipc is None else np.ascontiguousarray(ipc, dtype=np.float64)
        self._check(self.lib.nbp_belief_write(self._ctx, slot, manifold, pts.ctypes.data_as(dp), pts.shape[0],
                                              bw.ctypes.data_as(dp) if bw is not None else None,
                                              ipc.ctypes.data_as(dp) if ipc is not None else None))

    def belief_read(self, slot, manifold):
        dp = C.POINTER(C.c_double)
        pts = np.empty((self.N, abi.MANIFOLD_P[manifold]))
        bw, ipc = np.empty(abi.MANIFOLD_DIM[manifold]), np.empty(abi.MANIFOLD_DIM[manifold])
        n = C.c_int32(0)
        self._check(self.lib.nbp_belief_read(self._ctx, slot, manifold, pts.ctypes.data_as(dp), C.byref(n),
                                             bw.ctypes.data_as(dp), ipc.ctypes.data_as(dp)))
        return pts[:n.value], bw, ipc

    def beliefs_write(self, slots, manifolds, beliefs):
        """many TreeBeliefs in one call (nbp_belief_write_batch): beliefs = [(pts, bw or None, ipc or None), ...]"""
        dp, n = C.POINTER(C.c_double), len(slots)
        keep, P, B, I, cnt = [], (dp * n)(), (dp * n)(), (dp * n)(), (C.c_int32 * n)()
        for i, (pts, bw, ipc) in enumerate(beliefs):
            pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, abi.MANIFOLD_P[manifolds[i]])
            keep.append(pts)
            P[i], cnt[i] = pts.ctypes.data_as(dp), pts.shape[0]
            for arr, tab in ((bw, B), (ipc, I)):
                if arr is not None:
                    arr = np.ascontiguousarray(arr, dtype=np.float64)
                    keep.append(arr)
                    tab[i] = arr.ctypes.data_as(dp)
        self._check(self.lib.nbp_belief_write_batch(self._ctx, n, (C.c_int32 * n)(*slots), (C.c_int32 * n)(*manifolds), P, cnt, B, I))
        # (packed into the staging buffer before the call returns: `keep` may go)

    def beliefs_read(self, slots, manifolds):
        """-> [(pts, bw, ipc), ...] (nbp_belief_read_batch)"""
        dp, n = C.POINTER(C.c_double), len(slots)
        P, B, I, cnt = (dp * n)(), (dp * n)(), (dp * n)(), (C.c_int32 * n)()
        out = []
        for i, m in enumerate(manifolds):
            pts, bw, ipc = np.empty((self.N, abi.MANIFOLD_P[m])), np.empty(abi.MANIFOLD_DIM[m]), np.empty(abi.MANIFOLD_DIM[m])
            out.append((pts, bw, ipc))
            P[i], B[i], I[i] = pts.ctypes.data_as(dp), bw.ctypes.data_as(dp), ipc.ctypes.data_as(dp)
        self._check(self.lib.nbp_belief_read_batch(self._ctx, n, (C.c_int32 * n)(*slots), (C.c_int32 * n)(*manifolds), P, cnt, B, I))
        return [(p[:cnt[i]], b, q) for i, (p, b, q) in enumerate(out)]

    def side_write(self, offset, ints):
        a, ap = _i32(ints)
        self._check(self.lib.nbp_side_write(self._ctx, offset, ap, a.size))

    def side_read(self, offset, n):
        a = np.empty(n, dtype=np.int32)
        self._check(self.lib.nbp_side_read(self._ctx, offset, a.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return a

    # ---- op batches -----------------------------------------------------------------------
    def run_proposals(self, descs):
        arr, n = _as_array(descs, abi.ProposalDesc)
        self._check(self.lib.nbp_run_proposals(self._ctx, arr, n))

    def run_products(self, descs):
        arr, n = _as_array(descs, abi.ProductDesc)
        self._check(self.lib.nbp_run_products(self._ctx, arr, n))

    def run_copies(self, descs):
        arr, n = _as_array(descs, abi.CopyDesc)
        self._check(self.lib.nbp_run_copies(self._ctx, arr, n))

    def run_deconv(self, descs, meas_slots=None):
        arr, n = _as_array(descs, abi.ProposalDesc)
        _, msp = _i32(meas_slots if meas_slots is not None else [-1] * n)
        self._check(self.lib.nbp_run_deconv(self._ctx, arr, msp, n))

    def run_bandwidth(self, slots, manifolds):
        (s, sp), (_, mp) = _i32(slots), _i32(manifolds)
        self._check(self.lib.nbp_run_bandwidth(self._ctx, sp, mp, s.size))

    def run_ppe(self, slots, manifolds):
        """calcPPE of resident beliefs (nbp_run_ppe) -> (mean[n, 3], max[n, 3], max_index[n]): the manifold mean and the point
        of the belief at which its own KDE is greatest, in tangent coordinates (entries beyond the manifold's dimension zero)"""
        (s, sp), (_, mp) = _i32(slots), _i32(manifolds)
        n = s.size
        mean, mx, idx = np.zeros((n, abi.MAXD)), np.zeros((n, abi.MAXD)), np.zeros(n, dtype=np.int32)
        self._check(self.lib.nbp_run_ppe(self._ctx, sp, mp, n, _ptr(mean), _ptr(mx), _ptr(idx)))
        return mean, mx, idx

    def run_resample(self, slots, manifolds, seed=0):
        """sample(oldBel, N - Npts): top beliefs with fewer than N points up to N, in place"""
        (s, sp), (_, mp) = _i32(slots), _i32(manifolds)
        self._check(self.lib.nbp_run_resample(self._ctx, sp, mp, s.size, C.c_uint64(seed)))

    # ---- host-buffer entry points (one call per reference function) -------------------------------
    def kde_bandwidth(self, manifold, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        bw = np.zeros(abi.MANIFOLD_DIM[manifold])
        dp = C.POINTER(C.c_double)
        self._check(self.lib.nbp_kde_bandwidth(self._ctx, manifold, pts.ctypes.data_as(dp), bw.ctypes.data_as(dp)))
        return bw

    def kde_ppe(self, manifold, pts, bw):
        """calcPPE of a belief held on the host (nbp_kde_ppe; clobbers slot 0) -> (mean[D], max[D], max_index)"""
        pp, c, bp = _host_belief(manifold, pts, bw)
        D = abi.MANIFOLD_DIM[manifold]
        mean, mx, idx = np.zeros(D), np.zeros(D), C.c_int32(0)
        self._check(self.lib.nbp_kde_ppe(self._ctx, manifold, pp, c, bp, _ptr(mean), _ptr(mx), C.byref(idx)))
        return mean, mx, idx.value

    def _run_evaluate(self, slots, manifolds, masks, queries):
        """run_evaluate (masks None) and run_evaluate_marginal: one packing of the queries, one slicing of the densities"""
        (s, sp), (m, mp) = _i32(slots), _i32(manifolds)
        n = s.size
        Q, first = _pack_queries(m, queries)
        out = np.zeros(int(first[-1]))
        tail = (n, _ptr(first), _ptr(Q), _ptr(out))
        if masks is None:
            self._check(self.lib.nbp_run_evaluate(self._ctx, sp, mp, *tail))
        else:
            self._check(self.lib.nbp_run_evaluate_marginal(self._ctx, sp, mp, _i32(masks)[1], *tail))
        return [out[first[i]:first[i + 1]] for i in range(n)]

    def run_evaluate(self, slots, manifolds, queries):
        """densities of resident beliefs at query points (nbp_run_evaluate): queries = one array (q_i x D or x 3, tangent
        coordinates; may be empty) per belief -> one array of q_i densities per belief, from one launch"""
        return self._run_evaluate(slots, manifolds, None, queries)

    def kde_evaluate(self, manifold, pts, bw, queries):
        """densities of a belief held on the host at query points in tangent coordinates (nbp_kde_evaluate; clobbers slot 0)"""
        pp, c, bp = _host_belief(manifold, pts, bw)
        Q, first = _pack_queries([manifold], [queries], all_columns=True)
        out = np.zeros(int(first[1]))
        self._check(self.lib.nbp_kde_evaluate(self._ctx, manifold, pp, c, bp, _ptr(Q), int(first[1]), _ptr(out)))
        return out

    @staticmethod
    def _grid_desc(slot, manifold, dims, n, extent=None, margin=4.0):
        """one nbp_grid_desc: dims / n scalars or sequences of one or two (0-based coordinates); extent = ((lo0, step0), (lo1,
        step1)) or (lo0, step0, lo1, step1) or, 1-D, (lo0, step0); None: the automatic extent with `margin`"""
        dims, n = np.atleast_1d(dims).astype(int).tolist(), np.atleast_1d(n).astype(int).tolist()
        if len(dims) not in (1, 2) or len(n) != len(dims):
            raise ValueError("a marginal grid has one or two coordinates and as many sizes")
        g = abi.GridDesc(slot=int(slot), manifold=int(manifold), margin=float(margin))
        g.dims[0], g.dims[1] = dims[0], dims[1] if len(dims) > 1 else -1
        g.n[0], g.n[1] = n[0], n[1] if len(n) > 1 else 1
        if extent is None:
            g.flags = abi.GRID_AUTO_EXTENT
        else:
            e = np.asarray(extent, dtype=np.float64).reshape(-1)
            if e.size != 2 * len(dims):
                raise ValueError("an extent is (lo, step) per axis")
            for a in range(len(dims)):
                g.lo[a], g.step[a] = e[2 * a], e[2 * a + 1]
        return g

    def run_marginal_grid(self, grids, return_extent=False):
        """marginal densities of resident beliefs on regular grids (nbp_run_marginal_grid), all in one call: grids = [(slot,
        manifold, dims, n[, extent[, margin]])] as `_grid_desc` takes them, or ready `abi.GridDesc`s -> one array per grid of shape
        (n0,) or (n0, n1), the first listed coordinate slowest; return_extent: also [(lo0, step0, lo1, step1)] as used"""
        descs = [g if isinstance(g, abi.GridDesc) else self._grid_desc(*g) for g in grids]
        nd = len(descs)
        arr = (abi.GridDesc * max(nd, 1))(*descs)
        shapes = [(g.n[0],) if g.dims[1] == -1 else (g.n[0], g.n[1]) for g in descs]
        first = np.zeros(nd + 1, dtype=np.int64)
        for i, sh in enumerate(shapes):
            first[i + 1] = first[i] + max(int(np.prod(sh)), 0)
        first = first.astype(np.int32)
        out, ext = np.zeros(int(first[-1])), np.zeros((nd, 4))
        self._check(self.lib.nbp_run_marginal_grid(self._ctx, arr, nd, _ptr(first), _ptr(out), _ptr(ext)))
        res = [out[first[i]:first[i + 1]].reshape(sh) for i, sh in enumerate(shapes)]
        return (res, ext) if return_extent else res

    def kde_marginal_grid(self, manifold, pts, bw, dims, n, extent=None, margin=4.0):
        """the marginal grid of a belief held on the host (nbp_kde_marginal_grid; clobbers slot 0) -> (grid, (lo0, step0, lo1,
        step1)); dims 0-based"""
        pp, c, bp = _host_belief(manifold, pts, bw)
        g = self._grid_desc(0, manifold, dims, n, extent, margin)
        shape = (g.n[0],) if g.dims[1] == -1 else (g.n[0], g.n[1])
        out, ext = np.zeros(max(int(np.prod(shape)), 0)), np.zeros(4)
        self._check(self.lib.nbp_kde_marginal_grid(self._ctx, manifold, pp, c, bp, C.byref(g), _ptr(out), _ptr(ext)))
        return out.reshape(shape), ext

    def run_evaluate_marginal(self, slots, manifolds, masks, queries):
        """marginal densities of resident beliefs at query points (nbp_run_evaluate_marginal): masks = one coordinate bit mask
        per belief (bit d = coordinate d); queries as in run_evaluate (q_i x D or x 3; entries outside the mask are not read)"""
        return self._run_evaluate(slots, manifolds, masks, queries)

    def run_mmd(self, slots_a, slots_b, manifolds, sigma=0.001):
        """mmd of pairs of resident beliefs (nbp_run_mmd) -> values[n], from one launch"""
        (a, ap), (_, bp), (_, mp) = _i32(slots_a), _i32(slots_b), _i32(manifolds)
        out = np.zeros(a.size)
        self._check(self.lib.nbp_run_mmd(self._ctx, ap, bp, mp, a.size, float(sigma), _ptr(out)))
        return out

    def kde_mmd(self, manifold, a, b, sigma=0.001):
        """mmd of two beliefs held on the host (nbp_kde_mmd; clobbers slots 0 and 1)"""
        (ap, na, _), (bp, nb, _) = _host_belief(manifold, a), _host_belief(manifold, b)
        out = C.c_double(0.0)
        self._check(self.lib.nbp_kde_mmd(self._ctx, manifold, ap, na, bp, nb, float(sigma), C.byref(out)))
        return out.value

    def run_meancov(self, slots, manifolds):
        """calcMeanCovar of resident beliefs (nbp_run_meancov) -> (mean[n, 3], cov[n, 3, 3]), tangent coordinates, entries beyond
        the manifold's dimension zero; the mean is run_ppe's, bit for bit"""
        (s, sp), (_, mp) = _i32(slots), _i32(manifolds)
        n = s.size
        mean, cov = np.zeros((n, abi.MAXD)), np.zeros((n, abi.MAXD, abi.MAXD))
        self._check(self.lib.nbp_run_meancov(self._ctx, sp, mp, n, _ptr(mean), _ptr(cov)))
        return mean, cov

    def kde_meancov(self, manifold, pts):
        """calcMeanCovar of a belief held on the host (nbp_kde_meancov; clobbers slot 0) -> (mean[D], cov[D, D])"""
        pp, c, _ = _host_belief(manifold, pts)
        D = abi.MANIFOLD_DIM[manifold]
        mean, cov = np.zeros(D), np.zeros((D, D))
        self._check(self.lib.nbp_kde_meancov(self._ctx, manifold, pp, c, _ptr(mean), _ptr(cov)))
        return mean, cov

    _MODE_REC = np.dtype([("location", np.float64, (abi.MAXD,)), ("density", np.float64), ("count", np.int32), ("leader", np.int32)])

    @staticmethod
    def _modes_opts(bw_scale, tol, max_iter, merge):
        return abi.ModesOpts(bw_scale=float(bw_scale), tol=float(tol), merge=float(merge), max_iter=int(max_iter), pad=0)

    def run_modes(self, slots, manifolds, bw_scale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, max_iter=abi.MODES_MAX_ITER,
                  merge=abi.MODES_MERGE):
        """the modes of resident beliefs (nbp_run_modes: mean-shift from every point, merging and ranking in one launch) ->
        (recs[n, 32], n_modes[n], labels[n, N], iters[n, N], n_unconverged[n]); recs is a structured array with the fields
        location[3], density, count, leader, mode r of belief i in recs[i, r]; rows of labels / iters beyond a belief's count
        hold -1 / 0"""
        assert self._MODE_REC.itemsize == C.sizeof(abi.ModeRec)
        (s, sp), (_, mp) = _i32(slots), _i32(manifolds)
        n = s.size
        recs = np.zeros((n, abi.MODES_MAX), dtype=self._MODE_REC)
        nm, unc = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        lab, its = np.zeros((n, self.N), dtype=np.int32), np.zeros((n, self.N), dtype=np.int32)
        opts = self._modes_opts(bw_scale, tol, max_iter, merge)
        self._check(self.lib.nbp_run_modes(self._ctx, sp, mp, n, C.byref(opts), _ptr(recs, abi.ModeRec), _ptr(nm), _ptr(lab), _ptr(its), _ptr(unc)))
        return recs, nm, lab, its, unc

    def kde_modes(self, manifold, pts, bw, bw_scale=abi.MODES_BW_SCALE, tol=abi.MODES_TOL, max_iter=abi.MODES_MAX_ITER,
                  merge=abi.MODES_MERGE):
        """the modes of a belief held on the host (nbp_kde_modes; clobbers slot 0) -> (recs[32], n_modes, labels[c], iters[c],
        n_unconverged)"""
        pp, c, bp = _host_belief(manifold, pts, bw)
        recs = np.zeros(abi.MODES_MAX, dtype=self._MODE_REC)
        nm, unc = C.c_int32(0), C.c_int32(0)
        lab, its = np.zeros(max(c, 1), dtype=np.int32), np.zeros(max(c, 1), dtype=np.int32)
        opts = self._modes_opts(bw_scale, tol, max_iter, merge)
        self._check(self.lib.nbp_kde_modes(self._ctx, manifold, pp, c, bp, C.byref(opts), _ptr(recs, abi.ModeRec), C.byref(nm), _ptr(lab),
                                           _ptr(its), C.byref(unc)))
        return recs, nm.value, lab[:c], its[:c], unc.value

    # ---- mixture summaries (nbp_run_mixture; mixture.py) -----------------------------------------------------------------------
    MIX_REC = np.dtype([("weight", np.float64, (abi.MIX_MAX,)), ("mean", np.float64, (abi.MIX_MAX, abi.MAXD)),
                        ("cov", np.float64, (abi.MIX_MAX, abi.MAXD, abi.MAXD)), ("objective", np.float64),
                        ("count", np.int32, (abi.MIX_MAX,)), ("n_comp", np.int32), ("iters", np.int32), ("converged", np.int32),
                        ("n_dropped", np.int32)])

    def run_mixture(self, slots, manifolds, labels, init_mean, tol=abi.MIX_TOL, max_iter=abi.MIX_MAX_ITER, rows=None):
        """Gaussian-mixture summaries of resident beliefs (nbp_run_mixture: the whole EM of every belief in one launch).  labels:
        int32 rows of N starting labels (-1 .. 7), row rows[i] for belief i (default: row i); init_mean: n x 8 x 3 starting means
        -> (recs[n], labels[n, N]): recs a structured array with the fields of nbp_mixture_rec, the components by weight
        descending; rows of labels beyond a belief's count hold -1"""
        assert self.MIX_REC.itemsize == C.sizeof(abi.MixtureRec)
        (s, sp), (m, mp) = _i32(slots), _i32(manifolds)
        n = s.size
        lab, lp = _i32(labels)
        lab = lab.reshape(-1, self.N)
        r, rp = _i32(np.arange(n) if rows is None else rows)
        mu, mup = _f64(init_mean)
        if m.size != n or r.size != n or mu.shape != (n, abi.MIX_MAX, abi.MAXD) or (n and int(r.max()) >= lab.shape[0]):
            raise ValueError("run_mixture: one slot, manifold, label row and 8 x 3 starting means per belief")
        recs = np.zeros(n, dtype=self.MIX_REC)
        out = np.zeros((n, self.N), dtype=np.int32)
        opts = abi.MixtureOpts(tol=float(tol), max_iter=int(max_iter))
        self._check(self.lib.nbp_run_mixture(self._ctx, sp, mp, n, lp, rp, mup, C.byref(opts), _ptr(recs, abi.MixtureRec), _ptr(out)))
        return recs, out

    def kde_mixture(self, manifold, pts, bw, labels, init_mean, tol=abi.MIX_TOL, max_iter=abi.MIX_MAX_ITER):
        """the mixture summary of a belief held on the host (nbp_kde_mixture; clobbers slot 0); labels: c starting labels; init_mean:
        8 x 3 -> (rec, labels[c])"""
        pp, c, bp = _host_belief(manifold, pts, bw)
        lab, lp = _i32(labels)
        mu, mup = _f64(init_mean)
        if lab.size != c or mu.shape != (abi.MIX_MAX, abi.MAXD):
            raise ValueError("kde_mixture: one label per point and 8 x 3 starting means")
        rec = np.zeros(1, dtype=self.MIX_REC)
        out = np.zeros(max(c, 1), dtype=np.int32)
        opts = abi.MixtureOpts(tol=float(tol), max_iter=int(max_iter))
        self._check(self.lib.nbp_kde_mixture(self._ctx, manifold, pp, c, bp, lp, mup, C.byref(opts), _ptr(rec, abi.MixtureRec), _ptr(out)))
        return rec[0], out[:c]

    def run_factor_likelihood(self, descs):
        """the likelihood of factors under resident beliefs (nbp_run_factor_likelihood: every item in one launch); descs: a
        sequence (or ctypes array) of abi.LikelihoodDesc -> (loglik[n], comp_loglik[n, 4]); entries of comp_loglik beyond an item's
        ncomp are NaN"""
        arr, n = _as_array(descs, abi.LikelihoodDesc)
        ll, cl = np.zeros(n), np.zeros((n, abi.MAXC))
        self._check(self.lib.nbp_run_factor_likelihood(self._ctx, arr, n, _ptr(ll), _ptr(cl)))
        return ll, cl

    def factor_likelihood(self, desc, a, b=None):
        """the likelihood of one factor under beliefs held on the host (nbp_factor_likelihood; clobbers slots 0 and 1); a, b: host
        points (n x P) of the two roles, b None for a unary factor -> (loglik, comp_loglik[4])"""
        ap, na, _ = _host_belief(desc.manifold, a)
        bp, nb, _ = (None, 0, None) if b is None else _host_belief(desc.manifold, b)
        ll, cl = C.c_double(0.0), np.zeros(abi.MAXC)
        self._check(self.lib.nbp_factor_likelihood(self._ctx, C.byref(desc), ap, na, bp, nb, C.byref(ll), _ptr(cl)))
        return ll.value, cl

    # ---- local products on a grid (nbp_run_product_grid; productgrid.py) ---------------------------------------------------------
    PGRID_REC = np.dtype([("logZ", np.float64), ("logmax", np.float64), ("argmax", np.int32), ("pad", np.int32)])

    @staticmethod
    def _pgrid_shape(g):
        return tuple(max(int(g.n[a]), 0) for a in range(abi.MANIFOLD_DIM.get(int(g.manifold), abi.MAXD)))

    def run_product_grid(self, grids, items):
        """the products of factor messages on grids (nbp_run_product_grid: every grid in one launch sequence); grids: a sequence of
        abi.ProductGridDesc, items: a sequence (or ctypes array) of abi.ProductItem the grids' item ranges index ->
        (one array per grid of shape n[:D], coordinate 0 slowest; records[n] of PGRID_REC; extents[n, 6] as used)"""
        grids = list(grids)
        nd = len(grids)
        garr = (abi.ProductGridDesc * max(nd, 1))(*grids)
        iarr, ni = _as_array(items, abi.ProductItem) if len(items) else (None, 0)
        shapes = [self._pgrid_shape(g) for g in grids]
        first = np.zeros(nd + 1, dtype=np.int64)
        for i, g in enumerate(grids):
            first[i + 1] = first[i] + max(int(g.n[0]), 0) * max(int(g.n[1]), 0) * max(int(g.n[2]), 0)
        if first[-1] >= 1 << 31:
            raise ValueError("run_product_grid: more than 2^31 cells in one call")
        first = first.astype(np.int32)
        out, rec, ext = np.zeros(int(first[-1])), np.zeros(nd, dtype=self.PGRID_REC), np.zeros((nd, 6))
        self._check(self.lib.nbp_run_product_grid(self._ctx, garr, nd, iarr, ni, _ptr(first), _ptr(out), _ptr(rec, abi.ProductGridRec), _ptr(ext)))
        return [out[first[i]:first[i + 1]].reshape(sh) for i, sh in enumerate(shapes)], rec, ext

    def product_grid(self, grid, items, others, own=None, own_bw=None):
        """one grid from beliefs held on the host (nbp_product_grid; clobbers slots 0 .. len(items)): others[k] the host points
        (n x P) of item k's other variable, None for a unary item; own, own_bw the variable's own points and bandwidth, read for the
        automatic extent only -> (grid of shape n[:D], record, extent[6])"""
        iarr, ni = _as_array(items, abi.ProductItem) if len(items) else (None, 0)
        m = int(grid.manifold)
        held = [None if o is None else _host_belief(m, o) for o in others]
        ptrs = (_DP * max(ni, 1))(*[None if h is None else h[0] for h in held])
        cnt, cp = _i32([0 if h is None else h[1] for h in held])
        op, on, obp = (None, 0, None) if own is None else _host_belief(m, own, own_bw)
        sh = self._pgrid_shape(grid)
        out, rec, ext = np.zeros(max(int(np.prod(sh)), 0)), np.zeros(1, dtype=self.PGRID_REC), np.zeros(6)
        self._check(self.lib.nbp_product_grid(self._ctx, C.byref(grid), iarr, ni, ptrs, cp, op, on, obp, _ptr(out),
                                              _ptr(rec, abi.ProductGridRec), _ptr(ext)))
        return out.reshape(sh), rec[0], ext

    def run_factor_mode_likelihood(self, descs, row_a, row_b, labels):
        """the likelihood of factors under resident beliefs, mode by mode (nbp_run_factor_mode_likelihood: every item in one launch);
        descs: a sequence (or ctypes array) of abi.LikelihoodDesc; row_a, row_b: per item the row of `labels` (n_rows x N, int32,
        entries in -1 .. 7) that groups the particles of its role, -1: every point in group 0 ->
        (table[n, 8, 8], counts[n, 2, 8]); a cell without a member pair is NaN"""
        arr, n = _as_array(descs, abi.LikelihoodDesc)
        (ra, rap), (rb, rbp) = _i32(row_a), _i32(row_b)
        if ra.size != n or rb.size != n:
            raise ValueError("run_factor_mode_likelihood: one row index per item and role")
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1, self.N)
        tab, cnt = np.zeros((n, abi.MAXK, abi.MAXK)), np.zeros((n, 2, abi.MAXK), dtype=np.int32)
        self._check(self.lib.nbp_run_factor_mode_likelihood(self._ctx, arr, rap, rbp, n, _ptr(lab), lab.shape[0], _ptr(tab), _ptr(cnt)))
        return tab, cnt

    def factor_mode_likelihood(self, desc, a, labels_a=None, b=None, labels_b=None):
        """the mode-by-mode likelihood of one factor under beliefs held on the host (nbp_factor_mode_likelihood; clobbers slots 0
        and 1); a, b: host points (n x P) of the two roles, b None for a unary factor; labels_*: one group per point, None: every
        point in group 0 -> (table[8, 8], counts[2, 8])"""
        ap, na, _ = _host_belief(desc.manifold, a)
        bp, nb, _ = (None, 0, None) if b is None else _host_belief(desc.manifold, b)
        la = None if labels_a is None else np.ascontiguousarray(labels_a, dtype=np.int32).reshape(-1)
        lb = None if labels_b is None or b is None else np.ascontiguousarray(labels_b, dtype=np.int32).reshape(-1)
        if (la is not None and la.size != na) or (lb is not None and lb.size != nb):
            raise ValueError("factor_mode_likelihood: one label per point")
        tab, cnt = np.zeros((abi.MAXK, abi.MAXK)), np.zeros((2, abi.MAXK), dtype=np.int32)
        self._check(self.lib.nbp_factor_mode_likelihood(self._ctx, C.byref(desc), ap, na, _ptr(la), bp, nb, _ptr(lb), _ptr(tab), _ptr(cnt)))
        return tab, cnt

    def run_kld(self, slots_a, slots_b, manifolds, terms=False):
        """kld of pairs of resident beliefs (nbp_run_kld) -> values[n], from one launch; terms=True: (values[n], terms[n, 2]) with
        terms = (Eaa, Eab), values = Eaa - Eab, entropy(a) = -Eaa"""
        (a, ap), (_, bp), (_, mp) = _i32(slots_a), _i32(slots_b), _i32(manifolds)
        out, tm = np.zeros(a.size), np.zeros((a.size, 2))
        self._check(self.lib.nbp_run_kld(self._ctx, ap, bp, mp, a.size, _ptr(out), _ptr(tm if terms else None)))
        return (out, tm) if terms else out

    def kde_kld(self, manifold, a, bw_a, b, bw_b, terms=False):
        """kld of two beliefs held on the host (nbp_kde_kld; clobbers slots 0 and 1) -> value, or (value, (Eaa, Eab))"""
        (ap, na, ha), (bp, nb, hb) = _host_belief(manifold, a, bw_a), _host_belief(manifold, b, bw_b)
        out, tm = C.c_double(0.0), np.zeros(2)
        self._check(self.lib.nbp_kde_kld(self._ctx, manifold, ap, na, ha, bp, nb, hb, C.byref(out), _ptr(tm if terms else None)))
        return (out.value, tm) if terms else out.value

    def run_overlap(self, slots_a, slots_b, manifolds_a, manifolds_b, masks_a, masks_b):
        """the overlap of pairs of resident beliefs (nbp_run_overlap: one launch); masks = one coordinate bit mask per belief (bit d =
        coordinate d), the pair admissible -> recs[n, 4]: logc, L_ab, L_aa, L_bb"""
        cols = [_i32(v) for v in (slots_a, slots_b, manifolds_a, manifolds_b, masks_a, masks_b)]
        n = cols[0][0].size
        if any(a.size != n for a, _ in cols):
            raise ValueError("run_overlap: six columns of one length")
        out = np.zeros((n, 4))
        self._check(self.lib.nbp_run_overlap(self._ctx, *(p for _, p in cols), n, _ptr(out, abi.OverlapRec)))
        return out

    def kde_overlap(self, manifold_a, a, bw_a, mask_a, manifold_b, b, bw_b, mask_b):
        """the overlap of two beliefs held on the host (nbp_kde_overlap; clobbers slots 0 and 1) -> rec[4]: logc, L_ab, L_aa, L_bb"""
        (ap, na, ha), (bp, nb, hb) = _host_belief(manifold_a, a, bw_a), _host_belief(manifold_b, b, bw_b)
        out = np.zeros(4)
        self._check(self.lib.nbp_kde_overlap(self._ctx, manifold_a, ap, na, ha, int(mask_a), manifold_b, bp, nb, hb, int(mask_b),
                                             _ptr(out, abi.OverlapRec)))
        return out

    def run_overlap_search(self, slots, manifolds, masks, topk=abi.OVERLAP_TOPK, min_coeff=abi.OVERLAP_MIN_COEFF, reach=abi.OVERLAP_REACH):
        """the overlap search over a list of mutually admissible resident beliefs (nbp_run_overlap_search) ->
        (idx[n, topk], logc[n, topk], n_found[n], n_evaluated[n]); unused entries -1 / -inf"""
        (s, sp), (m, mp), (k, kp) = _i32(slots), _i32(manifolds), _i32(masks)
        n = s.size
        if m.size != n or k.size != n:
            raise ValueError("run_overlap_search: three columns of one length")
        topk = int(topk)
        rows = max(topk, 0)
        idx, logc = np.zeros((n, rows), dtype=np.int32), np.zeros((n, rows))
        found, evaluated = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        opts = abi.OverlapOpts(reach=float(reach), min_coeff=float(min_coeff), topk=topk, pad=0)
        self._check(self.lib.nbp_run_overlap_search(self._ctx, sp, mp, kp, n, C.byref(opts), _ptr(idx), _ptr(logc), _ptr(found), _ptr(evaluated)))
        return idx, logc, found, evaluated

    def run_scene_grid(self, slots, manifolds, dims, n, extent=None, margin=abi.SCENE_MARGIN, reach=abi.SCENE_REACH, weights=None,
                       owner=False):
        """every belief of a list of mutually admissible resident beliefs on ONE grid (nbp_run_scene_grid; scene.py): dims = the one
        or two 0-BASED coordinates of every belief (one list for all, or one per belief), n = the points per axis, extent = (lo0,
        step0[, lo1, step1]) or None for the automatic one with `margin`, weights = one per belief or None ->
        (grid (n0,) or (n0, n1), extent[4] as used, owner grid or None, skipped[V], tile_beliefs)"""
        (s, sp), (m, mp) = _i32(slots), _i32(manifolds)
        V = s.size
        dd = np.asarray(dims, dtype=np.int64)
        if dd.ndim < 2:
            dd = np.tile(dd.reshape(1, -1), (V, 1))
        axes = dd.shape[1]
        if m.size != V or dd.shape[0] != V or axes not in (1, 2):
            raise ValueError("run_scene_grid: one manifold per slot and one or two coordinates per belief")
        col = np.full((V, 2), -1, dtype=np.int32)
        col[:, :axes] = dd
        n = [int(v) for v in np.atleast_1d(n)]
        n = n * axes if len(n) == 1 else n
        if len(n) != axes:
            raise ValueError("run_scene_grid: one size per axis")
        g = abi.SceneDesc(margin=float(margin), reach=float(reach))
        g.n[0], g.n[1] = n[0], n[1] if axes == 2 else 1
        if extent is None:
            g.flags = abi.SCENE_AUTO_EXTENT
        else:
            e = np.asarray(extent, dtype=np.float64).reshape(-1)
            if e.size != 2 * axes:
                raise ValueError("an extent is (lo, step) per axis")
            for a in range(axes):
                g.lo[a], g.step[a] = e[2 * a], e[2 * a + 1]
        pts = max(g.n[0], 0) * max(g.n[1], 0)
        w = None if weights is None else _f64(weights, (V,))
        out, ext = np.zeros(pts), np.zeros(4)
        own = np.full(pts, -1, dtype=np.int32) if owner else None
        skipped, tb = np.zeros(V, dtype=np.int32), C.c_int64(0)
        self._check(self.lib.nbp_run_scene_grid(self._ctx, sp, mp, _ptr(col), w[1] if w else None, V, C.byref(g), _ptr(out), _ptr(own),
                                                _ptr(skipped), _ptr(ext), C.byref(tb)))
        shape = (g.n[0],) if axes == 1 else (g.n[0], g.n[1])
        return out.reshape(shape), ext, (own.reshape(shape) if owner else None), skipped, tb.value

    # ---- credible regions (nbp_run_credible; credible.py) ----------------------------------------------------------------------
    CRED_REC = np.dtype([("log_level", np.float64, (abi.CRED_MAX,)), ("quant", np.float64, (abi.MAXD, abi.CRED_MAX)),
                         ("mean", np.float64, (abi.MAXD,)), ("log_min", np.float64), ("log_max", np.float64),
                         ("n_inside", np.int32, (abi.CRED_MAX,)), ("count", np.int32), ("pad", np.int32)])
    CREDIBILITY_REC = np.dtype([("logdens", np.float64), ("mass", np.float64), ("n_above", np.int32), ("pad", np.int32)])

    @staticmethod
    def _credible_opts(mass, probs):
        mass, probs = np.asarray(mass, dtype=np.float64).reshape(-1), np.asarray(probs, dtype=np.float64).reshape(-1)
        o = abi.CredibleOpts(n_mass=mass.size, n_prob=probs.size)  # (more than CRED_MAX entries: the library refuses the count)
        o.mass[:min(mass.size, abi.CRED_MAX)] = mass[:abi.CRED_MAX].tolist()
        o.prob[:min(probs.size, abi.CRED_MAX)] = probs[:abi.CRED_MAX].tolist()
        return o

    def run_credible(self, slots, manifolds, masks, mass=(), probs=(), queries=None, logdens=True, order=True):
        """credible regions of resident beliefs (nbp_run_credible: one launch); masks = one coordinate bit mask per belief (bit d =
        coordinate d); mass / probs: up to 8 each; queries: None, or one array (q_i x D or x 3, tangent coordinates; may be empty)
        per belief -> (recs[n], logdens[n, N] or None, order[n, N] or None, qrecs[Q] or None, first[n + 1] or None): recs / qrecs
        structured arrays with the fields of nbp_credible_rec / nbp_credibility_rec, the queries of belief i in
        qrecs[first[i]:first[i + 1]]; rows of logdens / order beyond a belief's count hold NaN / -1"""
        assert self.CRED_REC.itemsize == C.sizeof(abi.CredibleRec) and self.CREDIBILITY_REC.itemsize == C.sizeof(abi.CredibilityRec)
        (s, sp), (m, mp), (k, kp) = _i32(slots), _i32(manifolds), _i32(masks)
        n = s.size
        if m.size != n or k.size != n:
            raise ValueError("run_credible: three columns of one length")
        recs = np.zeros(n, dtype=self.CRED_REC)
        ld = np.zeros((n, self.N)) if logdens else None
        od = np.zeros((n, self.N), dtype=np.int32) if order else None
        Q = first = qrecs = None
        if queries is not None:
            Q, first = _pack_queries(m, queries)
            qrecs = np.zeros(int(first[-1]), dtype=self.CREDIBILITY_REC)
        opts = self._credible_opts(mass, probs)
        self._check(self.lib.nbp_run_credible(self._ctx, sp, mp, kp, n, C.byref(opts), _ptr(first), _ptr(Q), _ptr(recs, abi.CredibleRec), _ptr(ld),
                                              _ptr(od), _ptr(qrecs, abi.CredibilityRec)))
        return recs, ld, od, qrecs, first

    def kde_credible(self, manifold, pts, bw, mask, mass=(), probs=(), queries=None, logdens=True, order=True):
        """credible regions of a belief held on the host (nbp_kde_credible; clobbers slot 0); queries: None or q x D (or x 3) tangent
        coordinates -> (rec, logdens[c] or None, order[c] or None, qrecs[q] or None)"""
        pp, c, bp = _host_belief(manifold, pts, bw)
        rec = np.zeros(1, dtype=self.CRED_REC)
        ld = np.zeros(self.N) if logdens else None
        od = np.zeros(self.N, dtype=np.int32) if order else None
        Q, first = _pack_queries([manifold], [queries if queries is not None else np.zeros((0, abi.MAXD))])
        qrecs = np.zeros(int(first[1]), dtype=self.CREDIBILITY_REC)
        opts = self._credible_opts(mass, probs)
        self._check(self.lib.nbp_kde_credible(self._ctx, manifold, pp, c, bp, int(mask), C.byref(opts), _ptr(Q), int(first[1]),
                                              _ptr(rec, abi.CredibleRec), _ptr(ld), _ptr(od), _ptr(qrecs, abi.CredibilityRec)))
        return rec[0], (ld[:c] if logdens else None), (od[:c] if order else None), (qrecs if queries is not None else None)

    # ---- heatmap densities (nbp_heatmap_*; heatmap.py) -------------------------------------------------------------------------
    def heatmap_create(self, data, x, y, bw_factor=0.7):
        """nbp_heatmap_create: the field data[i, j] at (x[i], y[j]) -> a handle (heatmap_destroy it); the library checks the grid"""
        dp = C.POINTER(C.c_double)
        data = np.ascontiguousarray(data, dtype=np.float64)
        x, y = np.ascontiguousarray(x, dtype=np.float64).reshape(-1), np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if data.ndim != 2 or data.shape != (x.size, y.size):
            raise ValueError("heatmap: data must be len(x) by len(y)")
        hm = C.c_void_p()
        self._check(self.lib.nbp_heatmap_create(self._ctx, data.ctypes.data_as(dp), x.size, y.size, x.ctypes.data_as(dp),
                                                y.ctypes.data_as(dp), float(bw_factor), C.byref(hm)))
        return hm

    def heatmap_build(self, hm, M, seed=0, outputs=True):
        """nbp_heatmap_build: M pre-samples under `seed` -> (cell[M], pre[M, 2], d[M], W[M]), or None with outputs=False"""
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        M = int(M)
        if not outputs or M < 1:
            self._check(self.lib.nbp_heatmap_build(hm, M, C.c_uint64(seed), None, None, None, None))
            return None
        cell, pre, d, W = np.zeros(M, dtype=np.int32), np.zeros((M, 2)), np.zeros(M), np.zeros(M)
        self._check(self.lib.nbp_heatmap_build(hm, M, C.c_uint64(seed), cell.ctypes.data_as(ip), pre.ctypes.data_as(dp),
                                               d.ctypes.data_as(dp), W.ctypes.data_as(dp)))
        return cell, pre, d, W

    def heatmap_draw(self, hm, n, seed=0, jitter=0, slot=-1, outputs=True):
        """nbp_heatmap_draw: n points of the density under `seed` -> (pick[n], points[n, 2], bw[2]); slot >= 0: they also become
        the EUCLID2 belief of that slot; outputs=False (with a slot): nothing comes back to the host but the bandwidth"""
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        n, bw = int(n), np.zeros(2)
        if not outputs or n < 1:
            self._check(self.lib.nbp_heatmap_draw(hm, n, C.c_uint64(seed), int(jitter), int(slot), None, None, bw.ctypes.data_as(dp)))
            return None, None, bw
        pick, pts = np.zeros(n, dtype=np.int32), np.zeros((n, 2))
        self._check(self.lib.nbp_heatmap_draw(hm, n, C.c_uint64(seed), int(jitter), int(slot), pick.ctypes.data_as(ip),
                                              pts.ctypes.data_as(dp), bw.ctypes.data_as(dp)))
        return pick, pts, bw

    def heatmap_info(self, hm):
        """-> (bw[2], total, wtotal, M): M = 0 (and wtotal = 0) before a build"""
        dp = C.POINTER(C.c_double)
        bw, total, wtotal, M = np.zeros(2), C.c_double(0), C.c_double(0), C.c_int32(0)
        self._check(self.lib.nbp_heatmap_info(hm, bw.ctypes.data_as(dp), C.byref(total), C.byref(wtotal), C.byref(M)))
        return bw, total.value, wtotal.value, M.value

    def heatmap_destroy(self, hm):
        if hm:
            self._check(self.lib.nbp_heatmap_destroy(hm))
            hm.value = None

    def heatmap_scan_eval(self, a):
        """nbp_heatmap_scan_eval: the device's scan (csrc/nbp_heatmap.h) of w = a where 0 < a, else 0 -> all len(a) sums"""
        dp = C.POINTER(C.c_double)
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        out = np.empty_like(a)
        self._check(self.lib.nbp_heatmap_scan_eval(self._ctx, a.ctypes.data_as(dp), a.size, out.ctypes.data_as(dp)))
        return out

    def heatmap_search_eval(self, cdf, t):
        """nbp_heatmap_search_eval: the device's search of every probe t[k] in cdf (any array of doubles) -> int32 indices"""
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        cdf = np.ascontiguousarray(cdf, dtype=np.float64).reshape(-1)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        idx = np.empty(t.size, dtype=np.int32)
        self._check(self.lib.nbp_heatmap_search_eval(self._ctx, cdf.ctypes.data_as(dp), cdf.size, t.ctypes.data_as(dp), t.size,
                                                     idx.ctypes.data_as(ip)))
        return idx

    def conv(self, desc, var_pts, var_bw=None, mhidx_in=None, want_mhidx=False, want_bw=True):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        man = desc.manifold
        pts = [np.ascontiguousarray(p, dtype=np.float64) for p in var_pts]
        bws = [None if (var_bw is None or b is None) else np.ascontiguousarray(b, dtype=np.float64) for b in (var_bw or [None] * len(pts))]
        ppts = (dp * len(pts))(*[p.ctypes.data_as(dp) for p in pts])
        pbw = (dp * len(pts))(*[(b.ctypes.data_as(dp) if b is not None else C.cast(None, dp)) for b in bws])
        out = np.zeros((self.N, abi.MANIFOLD_P[man]))
        obw = np.zeros(abi.MANIFOLD_DIM[man])
        mh_in = None if mhidx_in is None else np.ascontiguousarray(mhidx_in, dtype=np.int32)
        mh_out = np.zeros(self.N, dtype=np.int32) if want_mhidx else None
        self._check(self.lib.nbp_conv(self._ctx, C.byref(desc), ppts, pbw,
                                      mh_in.ctypes.data_as(ip) if mh_in is not None else C.cast(None, ip),
                                      out.ctypes.data_as(dp), obw.ctypes.data_as(dp) if want_bw else C.cast(None, dp),
                                      mh_out.ctypes.data_as(ip) if want_mhidx else C.cast(None, ip)))
        return (out, obw, mh_out) if want_mhidx else (out, obw)

    def manifold_product(self, manifold, dens, seed, niter=1, partial_masks=None, old_pts=None, want_labels=False):
        """dens: list of (pts N x P, bw D)"""
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        F = len(dens)
        pts = [np.ascontiguousarray(p, dtype=np.float64) for p, _ in dens]
        bws = [np.ascontiguousarray(b, dtype=np.float64) for _, b in dens]
        ppts = (dp * F)(*[p.ctypes.data_as(dp) for p in pts])
        pbw = (dp * F)(*[b.ctypes.data_as(dp) for b in bws])
        masks = None if partial_masks is None else np.ascontiguousarray(partial_masks, dtype=np.uint8)
        old = None if old_pts is None else np.ascontiguousarray(old_pts, dtype=np.float64)
        out = np.zeros((self.N, abi.MANIFOLD_P[manifold]))
        obw = np.zeros(abi.MANIFOLD_DIM[manifold])
        lab = np.zeros(self.N * F, dtype=np.int32) if want_labels else None
        self._check(self.lib.nbp_manifold_product(
            self._ctx, manifold, F, ppts, pbw,
            masks.ctypes.data_as(C.POINTER(C.c_uint8)) if masks is not None else C.cast(None, C.POINTER(C.c_uint8)),
            old.ctypes.data_as(dp) if old is not None else C.cast(None, dp), niter, C.c_uint64(seed),
            out.ctypes.data_as(dp), obw.ctypes.data_as(dp), lab.ctypes.data_as(ip) if want_labels else C.cast(None, ip)))
        return (out, obw, lab) if want_labels else (out, obw)

    def synchronize(self):
        self._check(self.lib.nbp_synchronize(self._ctx))

    # ---- separator exchange between ranks: RCCL point-to-point from C, on the library stream -----------------------------
    def comm_unique_id(self):
        buf = (C.c_char * abi.COMM_ID_BYTES)()
        self._check(self.lib.nbp_comm_unique_id(buf))
        return bytes(buf)

    def comm_create(self, world, rank, uid):
        h = C.c_void_p()
        buf = (C.c_char * abi.COMM_ID_BYTES).from_buffer_copy(uid)
        self._check(self.lib.nbp_comm_create(self._ctx, world, rank, buf, C.byref(h)))
        self._comm = h
        return h

    def comm_info(self):
        """(nranks, rank) as RCCL reports them for the library's communicator"""
        n, r = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.nbp_comm_info(self._comm, C.byref(n), C.byref(r)))
        return n.value, r.value

    def math_eval(self, fn, a, b=None):
        """the shared elementary functions (include/nbp_math.h) evaluated on the device: (out0, out1)"""
        dp = C.POINTER(C.c_double)
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        o0, o1 = np.empty_like(a), np.empty_like(a)
        self._check(self.lib.nbp_math_eval(self._ctx, fn, a.ctypes.data_as(dp), b.ctypes.data_as(dp) if b is not None else C.cast(None, dp),
                                           o0.ctypes.data_as(dp), o1.ctypes.data_as(dp), a.size))
        return o0, o1

    def comm_destroy(self):
        if getattr(self, "_comm", None):
            self.lib.nbp_comm_destroy(self._comm)
            self._comm = None

    def exchange(self, sends, recvs):
        """one grouped ncclSend / ncclRecv of whole slots: sends / recvs = [(peer rank, slot)]; asynchronous (stream-ordered)"""
        sx = (abi.Xfer * max(1, len(sends)))(*[abi.Xfer(p, s) for p, s in sends])
        rx = (abi.Xfer * max(1, len(recvs)))(*[abi.Xfer(p, s) for p, s in recvs])
        self._check(self.lib.nbp_exchange(self._ctx, self._comm, sx, len(sends), rx, len(recvs)))

    # ---- resident programs (clique seam) -----------------------------------------------------
    def program(self, stages, lazy_bandwidth=False, fused_updates=True):
        return HipProgram(self, stages, lazy_bandwidth, fused_updates)

    def timing_enable(self, on=True):
        self._check(self.lib.nbp_timing_enable(self._ctx, int(on)))

    KERNELS = ("nbp_proposal_kernel", "nbp_prep_kernel", "nbp_product_kernel", "nbp_bandwidth_kernel", "nbp_update_kernel")

    def timing_read(self):
        """{kernel: (total ms, launches)} measured with HIP events on the library stream"""
        ms = (C.c_double * 5)()
        nl = (C.c_int64 * 5)()
        self._check(self.lib.nbp_timing_read_n(self._ctx, ms, nl, 5))
        return {k: (ms[i], nl[i]) for i, k in enumerate(self.KERNELS)}

    def diag(self, reset=False):
        d = abi.Diag()
        self._check(self.lib.nbp_diag_read(self._ctx, C.byref(d), int(reset)))
        return {k: getattr(d, k) for k, _ in abi.Diag._fields_}

    def last_plans(self):
        """{"product", "prep", "fits"}: what the last product / prep / plain bandwidth launch of this context ran, as dicts of the
        fields of nbp_product_plan_rec / nbp_fit_plan_rec (recorded on the host when the launch is issued)"""
        p, q, f = abi.ProductPlanRec(), abi.FitPlanRec(), abi.FitPlanRec()
        self._check(self.lib.nbp_last_plans(self._ctx, C.byref(p), C.byref(q), C.byref(f)))
        return {"product": p.as_dict(), "prep": q.as_dict(), "fits": f.as_dict()}

    def arena_ptr(self):
        return self.lib.nbp_arena_ptr(self._ctx)

    def stream_ptr(self):
        return self.lib.nbp_stream_ptr(self._ctx)


_STAGE_CTYPE = {abi.STAGE_PROPOSALS: abi.ProposalDesc, abi.STAGE_PRODUCTS: abi.ProductDesc,
                abi.STAGE_COPIES: abi.CopyDesc, abi.STAGE_DECONV: abi.ProposalDesc,
                abi.STAGE_COPY_POINTS: abi.CopyDesc}


class HipProgram:
    """A device-resident schedule: list of (kind, descriptor-array) stages uploaded once."""

    def __init__(self, backend, stages, lazy_bandwidth=False, fused_updates=True, lanes=None):
        self.backend, lib = backend, backend.lib
        self._p = C.c_void_p()
        backend._check(lib.nbp_program_create(backend._ctx, C.byref(self._p)))
        backend._programs.add(self)
        if lazy_bandwidth:  # whole-solve programs: intermediate bandwidths nobody reads are not fitted
            backend._check(lib.nbp_program_set_option(self._p, abi.OPT_LAZY_BANDWIDTH, 1))
        if not fused_updates:  # every round as three launches (proposal, prep, product)
            backend._check(lib.nbp_program_set_option(self._p, abi.OPT_FUSED_UPDATES, 0))
        for kind, descs in stages:
            arr, n = _as_array(descs, _STAGE_CTYPE[kind])
            backend._check(lib.nbp_program_add_stage(self._p, kind, C.cast(arr, C.c_void_p), n))
        for s, hint in (lanes or {}).items():  # {stage: [lane per descriptor]} (nbp_program_set_lanes); the Python host passes none
            arr = (C.c_int32 * max(len(hint), 1))(*[int(x) for x in hint])
            backend._check(lib.nbp_program_set_lanes(self._p, s, arr, len(hint)))
        backend._check(lib.nbp_program_finalize(self._p))
        self.n_stages = len(stages)

    def lane_plan(self):
        """the parts of a program with lanes, in list order: dicts of the fields of nbp_lane_part_rec ([]: no lanes)"""
        n = C.c_int32(0)
        self.backend._check(self.backend.lib.nbp_program_lane_plan(self._p, None, 0, C.byref(n)))
        recs = (abi.LanePartRec * max(n.value, 1))()
        self.backend._check(self.backend.lib.nbp_program_lane_plan(self._p, recs, n.value, C.byref(n)))
        return [{k: getattr(r, k) for k, _ in abi.LanePartRec._fields_} for r in recs[:n.value]]

    def sink_plan(self):
        """beside lane_plan(), per part: the descriptors it gained from earlier stages (nbp_program_sink_plan; all 0: no sinks)"""
        n = C.c_int32(0)
        self.backend._check(self.backend.lib.nbp_program_sink_plan(self._p, None, 0, C.byref(n)))
        arr = (C.c_int32 * max(n.value, 1))()
        self.backend._check(self.backend.lib.nbp_program_sink_plan(self._p, arr, n.value, C.byref(n)))
        return list(arr[:n.value])

    def num_fused(self):
        """rounds (PROPOSALS + PRODUCTS stage pairs) that run as one launch of the fused update kernel"""
        n = C.c_int32(0)
        self.backend._check(self.backend.lib.nbp_program_num_fused(self._p, C.byref(n)))
        return n.value

    def num_two_stream(self):
        """rounds whose two halves run on two streams one launch apart (NBP_PIPELINE_MIN)"""
        n = C.c_int32(0)
        self.backend._check(self.backend.lib.nbp_program_num_two_stream(self._p, C.byref(n)))
        return n.value

    def run(self, first=0, last=-1):
        self.backend._check(self.backend.lib.nbp_program_run(self._p, first, last))

    def reseed(self, salt):
        self.backend._check(self.backend.lib.nbp_program_reseed(self._p, C.c_uint64(salt)))

    def num_seeds(self):
        n = C.c_int32(0)
        self.backend._check(self.backend.lib.nbp_program_num_seeds(self._p, C.byref(n)))
        return n.value

    def set_seeds(self, seeds):
        """new seeds for every op, in stage order: per proposal / deconv descriptor its seed and (where the descriptor named a
        stored measurement at finalize) its meas_seed behind it; per product descriptor its seed (nbp_program_set_seeds).
        The order of the stages as they were handed to the program, also where a two-stream round moved descriptors."""
        arr = (C.c_uint64 * len(seeds))(*[int(x) for x in seeds])
        self.backend._check(self.backend.lib.nbp_program_set_seeds(self._p, arr, len(seeds)))

    def seed_order(self):
        """where the seeds of set_seeds() go: entry i = the place of seeds[i]'s field in a walk over the descriptors as they lie
        in the finalized program; range(num_seeds()) unless a two-stream round moved descriptors (nbp_program_seed_order)"""
        n = self.num_seeds()
        arr = (C.c_int32 * max(n, 1))()
        self.backend._check(self.backend.lib.nbp_program_seed_order(self._p, arr, n))
        return list(arr[:n])

    @staticmethod
    def seeds_of(stages):
        """the seed list set_seeds() takes, read off a list of (kind, descriptors) stages"""
        out = []
        for kind, descs in stages:
            if kind in (abi.STAGE_PROPOSALS, abi.STAGE_DECONV):
                for d in descs:
                    out.append(d.seed)
                    if d.meas_seed:
                        out.append(d.meas_seed)
            elif kind == abi.STAGE_PRODUCTS:
                out.extend(d.seed for d in descs)
        return out

    def close(self):
        if self._p:
            self.backend.lib.nbp_program_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
