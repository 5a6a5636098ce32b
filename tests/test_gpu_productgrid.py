"""-m gpu: local products on a grid on the device (nbp_run_product_grid / nbp_product_grid, csrc/nbp_productgrid.h) through the C
ABI, the mirror and a solve session, held to the numpy restatement of productgrid.py.  The tolerance is worked out per cell on the
host (productgrid_cases.restate): 16 max(|float64 - long double| of the restatement, 4 ulp(max(1, |l|))); -inf cells and argmax are
compared exactly; the identities are bit for bit."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import likelihood_cases as lc
import productgrid_cases as pgc
from parity_utils import abi, iif

pytestmark = pytest.mark.gpu
pg = iif.productgrid


def _item(host_item, other_slot):
    d, role, _, group, lp = host_item
    it = abi.ProductItem(role=role, other=other_slot, group=group, log_prior=lp)
    it.lik = d
    return it


def _desc(manifold, n, extent, first_item, n_items, slot=0, margin=4.0):
    D = abi.MANIFOLD_DIM[manifold]
    g = abi.ProductGridDesc(manifold=manifold, slot=slot, first_item=first_item, n_items=n_items, margin=margin)
    g.n[:] = list(n) + [1] * (3 - D)
    if extent is None:
        g.flags = abi.PGRID_AUTO_EXTENT
    else:
        for a in range(D):
            g.lo[a], g.step[a] = extent[2 * a], extent[2 * a + 1]
    return g


def _stage(be, specs):
    """specs = [(manifold, n, extent, host items)]: every item's other cloud goes to a slot of its own (ONE beliefs_write), every
    spec becomes one grid descriptor with its own item range -> (grids, items)"""
    grids, items, slots, mans, bels = [], [], [], [], []
    for m, n, ext, host in specs:
        grids.append(_desc(m, n, ext, len(items), len(host)))
        for h in host:
            s = -1
            if h[2] is not None:
                s = len(slots)
                slots.append(s)
                mans.append(m)
                bels.append((h[2], np.ones(abi.MANIFOLD_DIM[m]), None))
            items.append(_item(h, s))
    if slots:
        be.beliefs_write(slots, mans, bels)
    return grids, items


def _hold_all(be, specs, what):
    grids, items = _stage(be, specs)
    logp, rec, ext = be.run_product_grid(grids, items)
    worst = 0.0
    for i, (m, n, e, host) in enumerate(specs):
        assert np.array_equal(ext[i][:len(e)], e) and np.all(ext[i][len(e):] == 0.0)
        worst = max(worst, pgc.hold(logp[i], (rec["logZ"][i], rec["logmax"][i], rec["argmax"][i]), pgc.restate(m, n, e, host), f"{what} grid {i}"))
    print(f"{what}: largest error / tolerance {worst:.3f}")
    return grids, items, logp, rec


SHAPES = {abi.EUCLID1: [37], abi.EUCLID2: [7, 6], abi.EUCLID3: [5, 4, 3], abi.CIRCULAR: [33], abi.SE2: [5, 4, 3]}


# ---- 1. every kind x role x family x mask the planner admits, on all five manifolds ---------------------------------------------
@pytest.mark.parametrize("manifold", pgc.MANIFOLDS)
def test_every_kind_role_family_and_mask(hip_backend, manifold):
    cases = pgc.by_manifold(manifold)
    be = hip_backend(65, len(cases) + 1)
    try:
        rng = np.random.default_rng(1000 + manifold)
        n = SHAPES[manifold]
        ext = pgc.extent_for(manifold, n)
        specs = [(manifold, n, ext, pgc.items_for([c], [65], rng)) for c in cases]
        _hold_all(be, specs, f"manifold {manifold}")
    finally:
        be.close()


# ---- 2. neighbour counts around the wave and up to the context size -----------------------------------------------------------------
def test_neighbour_counts(hip_backend):
    be = hip_backend(512, 40)
    try:
        rng = np.random.default_rng(1100)
        specs = []
        for cnt in (1, 63, 64, 65, 200, 512):
            specs.append((abi.EUCLID2, [5, 4], pgc.extent_for(abi.EUCLID2, [5, 4]),
                          pgc.items_for([("linrel_e2_full", 0), ("linrel_e2_full", 1), ("dist_e2_rayleigh", 1)], [cnt] * 3, rng)))
            specs.append((abi.SE2, [3, 3, 4], pgc.extent_for(abi.SE2, [3, 3, 4]),
                          pgc.items_for([("se2_full", 0), ("se2_mix4", 1), ("se2_heading", 1)], [cnt] * 3, rng)))
        _hold_all(be, specs, "counts 1 .. 512")
    finally:
        be.close()


# ---- 3. cells around the chunk, 3-D grids, 0 / 1 / 6 items, groups of 1 / 2 / 3; a batch is its single launches ----------------------
def _shape_specs(rng):
    six = [("linrel_e1_normal", 0), ("linrel_e1_mix4", 1), ("dist_e1_normal", 0), ("linrel_e1_uniform", 1), ("linrel_e1_mix2", 0),
           ("prior_e1_normal", 0)]
    groups, lps = [0, 0, 0, 3, 3, 7], [math.log(0.2), math.log(0.3), math.log(0.5), math.log(0.4), math.log(0.6), 0.0]
    specs = []
    for cells in (1, 255, 256, 257, 513):
        specs.append((abi.EUCLID1, [cells], pgc.extent_for(abi.EUCLID1, [cells]), pgc.items_for(six, [40, 64, 7, 33, 65, 0], rng, groups, lps)))
    specs.append((abi.EUCLID1, [257], pgc.extent_for(abi.EUCLID1, [257]), []))
    specs.append((abi.EUCLID1, [257], pgc.extent_for(abi.EUCLID1, [257]), pgc.items_for([("linrel_e1_rayleigh", 1)], [50], rng)))
    specs.append((abi.EUCLID3, [5, 4, 3], pgc.extent_for(abi.EUCLID3, [5, 4, 3]),
                  pgc.items_for([("linrel_e3_full", 1), ("prior_e3_coords13", 0), ("dist_e3_normal", 0)], [30, 0, 20], rng, [0, 0, 1],
                                [math.log(0.5), math.log(0.5), 0.0])))
    specs.append((abi.SE2, [1, 1, 7], np.array([0.5, 1.0, -0.25, 1.0, -np.pi, 2 * np.pi / 7]),
                  pgc.items_for([("se2_full", 1), ("prior_se2_xy", 0)], [45, 0], rng)))
    specs.append((abi.EUCLID3, [1, 1, 7], pgc.extent_for(abi.EUCLID3, [1, 1, 7]), pgc.items_for([("linrel_e3_coords13", 0)], [12], rng)))
    return specs


def test_shapes_items_groups_and_the_batch_identity(hip_backend):
    be = hip_backend(65, 48)
    try:
        specs = _shape_specs(np.random.default_rng(1200))
        grids, items, logp, rec = _hold_all(be, specs, "shapes")
        assert np.all(logp[5] == 0.0) and rec["argmax"][5] == 0 and rec["logmax"][5] == 0.0  # (no items: L = 0 everywhere)
        again = be.run_product_grid(grids, items)
        assert all(np.array_equal(a, b) for a, b in zip(again[0], logp)) and again[1].tobytes() == rec.tobytes()
        for i, g in enumerate(grids):  # a batch equals the single launches, bit for bit
            l1, r1, _ = be.run_product_grid([g], items)
            assert np.array_equal(l1[0], logp[i]) and r1.tobytes() == rec[i:i + 1].tobytes(), i
        # several descriptors may name the same item range
        two = be.run_product_grid([grids[0], grids[3], grids[3]], items)
        assert np.array_equal(two[0][1], logp[3]) and np.array_equal(two[0][2], logp[3]) and np.array_equal(two[0][0], logp[0])
    finally:
        be.close()


# ---- 4. a cell is its point and its items alone; a group of one is the item untouched -----------------------------------------------
def test_cell_and_group_identities(hip_backend):
    be = hip_backend(65, 16)
    try:
        rng = np.random.default_rng(1300)
        host = pgc.items_for([("se2_full", 0), ("se2_mix4", 1), ("prior_se2_heading", 0)], [65, 40, 0], rng)
        n, ext = [6, 5, 9], pgc.extent_for(abi.SE2, [6, 5, 9])
        grids, items = _stage(be, [(abi.SE2, n, ext, host)])
        logp, rec, _ = be.run_product_grid(grids, items)
        axes = pg.grid_axes(ext, n)
        for k in (0, 1, 44, 133, 269):
            k3 = np.unravel_index(k, n)
            e1 = np.ravel([[axes[a][k3[a]], 1.0] for a in range(3)])
            one = be.run_product_grid([_desc(abi.SE2, [1, 1, 1], e1, 0, len(host))], items)
            assert np.array_equal(one[0][0].reshape(()), logp[0][k3]), k
            assert one[1]["logmax"][0] == logp[0][k3] and one[1]["argmax"][0] == 0
        # group numbers are labels: one item in group 5 is the item in group 0, and the item beside a hypothesis of prior 0 -- which
        # goes through the max-shift -- is the item alone
        alone = be.run_product_grid([_desc(abi.SE2, n, ext, 1, 1)], items)[0][0]
        it5 = abi.ProductItem.from_buffer_copy(items[1])
        it5.group = 5
        dead = abi.ProductItem.from_buffer_copy(items[1])
        dead.group, dead.log_prior = 5, -np.inf
        assert np.array_equal(be.run_product_grid([_desc(abi.SE2, n, ext, 0, 1)], [it5])[0][0], alone)
        assert np.array_equal(be.run_product_grid([_desc(abi.SE2, n, ext, 0, 2)], [it5, dead])[0][0], alone)
        assert np.array_equal(be.run_product_grid([_desc(abi.SE2, n, ext, 0, 2)], [dead, it5])[0][0], alone)
        # L is the sum of the single messages in list order
        parts = [be.run_product_grid([_desc(abi.SE2, n, ext, k, 1)], items)[0][0] for k in range(3)]
        assert np.array_equal((parts[0] + parts[1]) + parts[2], logp[0])
    finally:
        be.close()


# ---- 5. the automatic axes are the marginal grid's ---------------------------------------------------------------------------------------
def test_automatic_axes_equal_the_marginal_grids(hip_backend):
    be = hip_backend(100, 4)
    try:
        rng = np.random.default_rng(1400)
        X1, X2, XS, XC = rng.normal(1, 2, (100, 1)), rng.normal(-1, 3, (77, 2)), pgc.cloud(abi.SE2, 100, rng), pgc.cloud(abi.CIRCULAR, 30, rng)
        be.beliefs_write([0, 1, 2, 3], [abi.EUCLID1, abi.EUCLID2, abi.SE2, abi.CIRCULAR],
                         [(X1, [0.3], None), (X2, [0.25, 0.4], None), (XS, [0.3, 0.2, 0.1], None), (XC, [0.2], None)])
        grids = [_desc(abi.EUCLID1, [33], None, 0, 0, slot=0), _desc(abi.EUCLID2, [9, 12], None, 0, 0, slot=1, margin=2.5),
                 _desc(abi.SE2, [5, 6, 7], None, 0, 0, slot=2), _desc(abi.CIRCULAR, [16], None, 0, 0, slot=3)]
        _, _, ext = be.run_product_grid(grids, [])
        _, mext = be.run_marginal_grid([(0, abi.EUCLID1, [0], [33]), (1, abi.EUCLID2, [0, 1], [9, 12], None, 2.5),
                                        (2, abi.SE2, [0, 1], [5, 6]), (2, abi.SE2, [2], [7]), (3, abi.CIRCULAR, [0], [16])], return_extent=True)
        assert np.array_equal(ext[0][:2], mext[0][:2]) and np.array_equal(ext[1][:4], mext[1])
        assert np.array_equal(ext[2][:4], mext[2]) and np.array_equal(ext[2][4:], mext[3][:2]) and np.array_equal(ext[3][:2], mext[4][:2])
        want = pg.product_extent_numpy(abi.EUCLID2, X2, [0.25, 0.4], [9, 12], 2.5)
        assert np.array_equal(ext[1][:4], want)
    finally:
        be.close()


# ---- 6. refusals: a status before any launch, the index in the message -----------------------------------------------------------------
def test_argument_errors(hip_backend):
    be = hip_backend(64, 4)
    lib, ctx = be.lib, be._ctx
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    try:
        rng = np.random.default_rng(1500)
        for s in range(4):
            be.belief_write(s, abi.EUCLID1, rng.normal(0, 1, (64, 1)), [0.2])
        ARG, RANGE = -1, -4
        out = np.full(8, 7.0)

        def item(name="linrel_e1_normal", role=0, other=1, group=0, lp=0.0, **kw):
            it = abi.ProductItem(role=role, other=other, group=group, log_prior=lp)
            it.lik = lc.desc(name)
            for k, v in kw.items():
                if k.startswith("comp"):
                    it.lik.comp[int(k[4])][int(k[6:])] = v
                else:
                    setattr(it.lik, k, v)
            return it

        def grid(n=(8, 1, 1), manifold=abi.EUCLID1, lo=0.0, step=0.5, **kw):
            g = abi.ProductGridDesc(manifold=manifold, n_items=1, margin=4.0)
            g.n[:] = n
            g.lo[0], g.step[0] = lo, step
            for k, v in kw.items():
                setattr(g, k, v)
            return g

        def call(g, its, first=None, o=out):
            garr, iarr = (abi.ProductGridDesc * len(g))(*g), (abi.ProductItem * max(len(its), 1))(*its)
            f = np.array([0] + list(np.cumsum([x.n[0] * x.n[1] * x.n[2] for x in g])) if first is None else first, dtype=np.int32)
            rc = lib.nbp_run_product_grid(ctx, garr, len(g), iarr, len(its), f.ctypes.data_as(ip), o.ctypes.data_as(dp) if o is not None else None,
                                          None, None)
            assert rc == 0 or np.all(out == 7.0), "a refused call leaves the outputs untouched"
            return rc, lib.nbp_last_error()

        assert call([grid()], [item()])[0] == 0 and np.all(np.isfinite(out))
        out[:] = 7.0
        assert lib.nbp_run_product_grid(ctx, None, 0, None, 0, None, None, None, None) == 0
        assert lib.nbp_run_product_grid(None, None, 1, None, 0, None, None, None, None) == ARG
        assert call([grid()], [item()], o=None)[0] == ARG
        bad_items = [
            (item(kind=abi.F_MSGPRIOR), ARG), (item(kind=abi.F_PASSTHROUGH), ARG), (item(comp0_12=float(abi.DIST_TABLE)), ARG),
            (item(comp0_4=0.0), ARG), (item(ncomp=5), ARG), (item(comp0_0=-1.0), ARG), (item(kind=abi.F_CIRCULAR), ARG),
            (item(partial_mask=2), RANGE),                                              # (everything the factor likelihood refuses)
            (item(role=2), ARG), (item(role=-1), ARG), (item("prior_e1_normal", role=1, other=-1), ARG),
            (item("prior_e1_normal", other=1), ARG), (item(other=4), RANGE), (item(other=-1), RANGE),
            (item(lp=np.nan), ARG), (item(lp=np.inf), ARG),
        ]
        for k, (it, status) in enumerate(bad_items):
            rc, msg = call([grid(n_items=2)], [item(), it])
            assert rc == status and b"item 1" in msg, (k, rc, msg)
        assert call([grid()], [item(lp=-np.inf)])[0] == 0
        out[:] = 7.0
        rc, msg = call([grid(n_items=2)], [item(group=2), item(group=1)])
        assert rc == ARG and b"item 1" in msg and b"groups" in msg
        rc, msg = call([grid(n_items=2, first_item=1, manifold=abi.EUCLID1)], [item(), item(), item("linrel_e2_full")])
        assert rc == ARG and b"descriptor 0" in msg and b"item 2" in msg           # (an item whose manifold is not the grid's)
        bad_grids = [
            (grid(n=(0, 1, 1)), RANGE), (grid(n=(1025, 1, 1)), RANGE), (grid(n=(8, 2, 1)), RANGE), (grid(manifold=0), ARG), (grid(manifold=6), ARG),
            (grid(flags=2), ARG), (grid(lo=np.inf), RANGE), (grid(step=0.0), RANGE), (grid(step=-1.0), RANGE), (grid(step=np.nan), RANGE),
            (grid(flags=1, slot=4), RANGE), (grid(flags=1, slot=-1), RANGE), (grid(flags=1, margin=np.inf), RANGE), (grid(n=(1, 1, 1), flags=1), RANGE),
            (grid(first_item=1), RANGE), (grid(n_items=2), RANGE), (grid(n_items=-1), RANGE),
        ]
        for k, (g, status) in enumerate(bad_grids):
            rc, msg = call([grid(), g], [item()])
            assert rc == status and b"descriptor 1" in msg, (k, rc, msg)
        g3 = abi.ProductGridDesc(manifold=abi.EUCLID3, n_items=0)
        g3.n[:] = (1024, 1024, 8)
        for a in range(3):
            g3.step[a] = 1.0
        rc, msg = call([g3], [], first=[0, 0])
        assert rc == RANGE and b"2^22" in msg
        rc, msg = call([grid(), grid()], [item()], first=[0, 8, 15])
        assert rc == RANGE and b"descriptor 1" in msg and b"offsets" in msg
        assert call([grid()], [item()], first=[1, 9])[0] == RANGE
        with pytest.raises(iif.NbpError, match="-4"):
            be.run_product_grid([grid()], [item(other=9)])
        # the host-buffer form: refused before a slot is touched; needs 1 + n_items slots
        before = be.slot_read(1, abi.EUCLID1)[0].copy()
        pts = rng.normal(0, 1, (10, 1))
        with pytest.raises(iif.NbpError, match="-1"):
            be.product_grid(grid(), [item(comp0_4=0.0)], [pts])
        with pytest.raises(iif.NbpError, match="-4"):
            be.product_grid(grid(n_items=4), [item()] * 4, [pts] * 4)
        with pytest.raises(iif.NbpError, match="-1"):
            be.product_grid(grid(flags=1), [item()], [pts])                     # (the automatic extent needs the variable's own belief)
        assert np.array_equal(be.slot_read(1, abi.EUCLID1)[0], before)
        assert call([grid()], [item()])[0] == 0
    finally:
        be.close()


def test_host_buffer_form_equals_the_resident_form(hip_backend):
    be = hip_backend(100, 5)
    try:
        rng = np.random.default_rng(1600)
        host = pgc.items_for([("se2_full", 1), ("prior_se2_full", 0), ("se2_xy", 0)], [100, 0, 60], rng, [0, 1, 1], [0.0, math.log(0.25), math.log(0.75)])
        own = pgc.cloud(abi.SE2, 80, rng)
        for ext in (pgc.extent_for(abi.SE2, [6, 5, 4]), None):
            g = _desc(abi.SE2, [6, 5, 4], ext, 0, 3)
            l1, r1, e1 = be.product_grid(g, [_item(h, 3) for h in host], [h[2] for h in host], own, [0.3, 0.2, 0.1])
            be.beliefs_write([4, 2, 3], [abi.SE2] * 3, [(own, [0.3, 0.2, 0.1], None), (host[0][2], np.ones(3), None), (host[2][2], np.ones(3), None)])
            g.slot = 4
            l2, r2, e2 = be.run_product_grid([g], [_item(host[0], 2), _item(host[1], -1), _item(host[2], 3)])
            assert np.array_equal(l1, l2[0]) and r1.tobytes() == r2[0].tobytes() and np.array_equal(e1, e2[0])
    finally:
        be.close()


# ---- 7. the mirror and the session -----------------------------------------------------------------------------------------------------------
def _hold_to_numpy(fg, got, n, what):
    for label, r in got.items():
        p = pg.variable_items(fg, label)
        assert r.factors == p.factors and r.skipped == p.skipped
        host = [(d, role, None if o is None else fg.getVal(o), g, lp) for d, role, o, g, lp in p.items]
        pgc.hold(r.logp, (r.logZ, r.logmax, r.argmax), pgc.restate(p.manifold, pg._sizes(p.manifold, n), r.extent, host), f"{what} {label}")


def test_mirror_on_a_hand_set_graph(hip_backend):
    fg = lc.doors_graph()
    lc.outlier_chain(fg, n_poses=4)
    got = iif.localProductGridAll(fg, n=24, backend=hip_backend)
    assert list(got) == ["l1", "l2", "p0", "p1", "p2", "p3", "x"]
    assert got["x"].factors == ["door"] and got["l1"].skipped == ["door"] and got["p1"].factors == ["p0p1f1", "p1p2f1"]
    _hold_to_numpy(fg, got, 24, "hand-set")
    host = iif.localProductGridAll(fg, n=24)
    for v in got:  # the host route takes the same axes
        assert np.array_equal(host[v].extent, got[v].extent), v
    one = iif.localProductGrid(fg, "p1", n=24, backend=hip_backend)
    assert np.array_equal(one.logp, got["p1"].logp) and one.logZ == got["p1"].logZ and one.argmax == got["p1"].argmax
    part = iif.localProductGrid(fg, "p1", n=24, factors=["p1p2f1"], backend=hip_backend)
    assert part.factors == ["p1p2f1"] and not np.array_equal(part.logp, one.logp)
    with pytest.raises(ValueError, match="fractional"):
        iif.localProductGrid(fg, "l1", factors=["door"], backend=hip_backend)


def test_session_reads_the_resident_beliefs_where_they_lie(hip_backend):
    fg = iif.generateCircularDoors(nposes=10, N=64, sightEvery=5)
    with iif.SolveSession(fg, backend=hip_backend) as ses:
        ses.solve(seed=71)
        before = copy.deepcopy(ses.stats)
        got = ses.localProductGrids(n=32)
        assert ses.stats == before
        host = iif.localProductGridAll(fg, n=32, backend=hip_backend)
        assert list(got) == list(host) and len(got) >= 10
        assert any(len(pg.variable_items(fg, v).items) > len(r.factors) for v, r in got.items()), "a multihypo group entered"
        for v in got:
            assert np.array_equal(got[v].logp, host[v].logp) and np.array_equal(got[v].extent, host[v].extent), v
            assert (got[v].logZ, got[v].logmax, got[v].argmax) == (host[v].logZ, host[v].logmax, host[v].argmax), v
            assert got[v].factors == host[v].factors and got[v].skipped == host[v].skipped
        _hold_to_numpy(fg, got, 32, "session")
        some = list(got)[:3]
        assert list(ses.localProductGrids(some, n=32)) == some and ses.stats == before
