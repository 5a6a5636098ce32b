"""Scene densities on the host (-m "not gpu"): the numpy restatements of incrementalinference.jl_amd/scene.py against the marginal
grids they are made of, hand values, the truncation bound, the mass, the owner rule, and the argument forms of `sceneGrid`; the layout
of the new ABI struct."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import marginal_cases as mc
import scene_cases as scs
from parity_utils import abi, iif

sc, mg = iif.scene, iif.marginal
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E1, E2, E3, CI, SE2 = scs.E1, scs.E2, scs.E3, scs.CI, scs.SE2


# ---- 1. reach = inf: the sum, in list order, of the marginal grids on the common extent ----------------------------------------------
@pytest.mark.parametrize("specs,n,auto", [
    ([(E2, (0, 1), 33), (SE2, (0, 1), 31), (E3, (2, 0), 2), (E2, (1, 0), 1)], (33, 65), True),
    ([(SE2, (0, 2), 20), (SE2, (1, 2), 32)], (31, 33), False),
    ([(SE2, (1, 2), 20)] * 3, (17, 1), True),
    ([(E1, (0,), 64), (E3, (1,), 65), (E2, (1,), 5)], (130,), True),
    ([(CI, (0,), 31), (SE2, (2,), 7)], (63,), False),
], ids=lambda v: None)
def test_unculled_scene_is_the_sum_of_the_marginal_grids(specs, n, auto):
    scene = scs.compact(specs, 11)
    if auto:
        ext = sc.scene_extent_numpy(scene, n, 4.0)
        got, used, _, skipped = sc.scene_grid_numpy(scene, n, reach=np.inf)
        assert used.tobytes() == ext.tobytes()
    else:
        ext = scs.explicit_extent(scene, n, np.random.default_rng(12))
        full = np.zeros(4)
        full[:len(ext)] = ext
        got, used, _, skipped = sc.scene_grid_numpy(scene, n, ext[0::2], ext[1::2], reach=np.inf)
        assert used.tobytes() == full.tobytes()
    k = len(n)
    want = np.zeros(n)
    for m, X, bw, dims in scene:
        want = want + mg.marginal_grid_numpy(m, X, bw, dims, n, ext[0:2 * k:2], ext[1:2 * k:2])[0]
    assert np.array_equal(got, want) and not skipped.any() and np.all(got > 0)


# ---- 2. hand values ---------------------------------------------------------------------------------------------------------------------
def test_two_beliefs_of_one_point_each_by_hand():
    """A at (0, 0) with h = (0.5, 0.5), B at (3, 0) with h = (0.25, 0.5); the grid x = -1 .. 4, y = -1 .. 1 in steps of 1; reach 2:
    A is drawn on x in [-1, 1], B on x in [2.5, 3.5], both on every y.  Each value is a dozen float64 operations: 1e-14 relative."""
    A, B = (E2, np.array([[0.0, 0.0]]), np.array([0.5, 0.5]), (0, 1)), (E2, np.array([[3.0, 0.0]]), np.array([0.25, 0.5]), (0, 1))
    w = [1.0, 0.5]
    g, ext, own, skipped = sc.scene_grid_numpy([A, B], (6, 3), [-1.0, -1.0], [1.0, 1.0], reach=2.0, weights=w, owner=True)

    def term(b, x, y):
        (px, py), (hx, hy) = b[1][0], b[2]
        return math.exp(-0.5 * ((x - px) / hx) ** 2) * math.exp(-0.5 * ((y - py) / hy) ** 2) / (2 * math.pi * hx * hy)
    for k0, x in enumerate(range(-1, 5)):
        for k1, y in enumerate(range(-1, 2)):
            if x <= 1:
                want, who = w[0] * term(A, x, y), 0
            elif x == 3:
                want, who = w[1] * term(B, x, y), 1
            else:
                want, who = 0.0, -1     # x = 2 and x = 4: out of reach of both, exactly nothing
            assert (g[k0, k1] == 0.0 and own[k0, k1] == -1) if who < 0 else (math.isclose(g[k0, k1], want, rel_tol=1e-14) and own[k0, k1] == who), (x, y)
    # without culling both beliefs are everywhere
    g2, _, own2, _ = sc.scene_grid_numpy([A, B], (6, 3), [-1.0, -1.0], [1.0, 1.0], reach=np.inf, weights=w, owner=True)
    for k0, x in enumerate(range(-1, 5)):
        for k1, y in enumerate(range(-1, 2)):
            ta, tb = w[0] * term(A, x, y), w[1] * term(B, x, y)
            assert math.isclose(g2[k0, k1], ta + tb, rel_tol=1e-14) and own2[k0, k1] == (0 if ta >= tb else 1)
    assert ext.tolist() == [-1.0, 1.0, -1.0, 1.0] and not skipped.any()


# ---- 3. the truncation bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [1.5, 3.0, 6.0])
def test_what_culling_leaves_out_is_below_the_bound_cell_by_cell(reach):
    rng = np.random.default_rng(31)
    for scene, n in ((scs.poses_and_landmarks(5, 4, 33, 32), (40, 33)), (scs.compact([(SE2, (0, 2), 20)] * 4, 33), (33, 17)),
                     (scs.compact([(E1, (0,), 40)] * 6, 34), (130,))):
        w = rng.uniform(0.5, 2.0, len(scene))
        ext = sc.scene_extent_numpy(scene, n)
        k = len(n)
        full = sc.scene_grid_numpy(scene, n, ext[0:2 * k:2], ext[1:2 * k:2], reach=np.inf, weights=w, terms=True)
        cut = sc.scene_grid_numpy(scene, n, ext[0:2 * k:2], ext[1:2 * k:2], reach=reach, weights=w, terms=True)
        total = np.zeros(n)
        dropped = 0
        for v, (m, X, bw, dims) in enumerate(scene):
            out = cut[4][v] == 0
            b = sc.truncation_bound(bw, dims, reach, w[v])
            assert np.array_equal(cut[4][v][~out], full[4][v][~out])    # in reach: the same term
            assert np.all(full[4][v][out] < b), (v, full[4][v][out].max(), b)
            total += np.where(out, b, 0.0)
            dropped += int(out.sum())
        diff = full[0] - cut[0]
        print(f"reach {reach} grid {n}: {dropped} terms left out, largest loss {diff.max():.3e}, largest loss / bound {np.max(diff / np.maximum(total, 1e-300)):.3e}")
        assert np.all(diff >= -1e-12 * full[0]) and np.all(diff <= total + 1e-12 * full[0])
        assert dropped > 0 or reach == 6.0


# ---- 4. the mass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [4.0, 6.0, np.inf])
def test_mass_is_the_sum_of_the_weights(reach):
    scene = scs.poses_and_landmarks(4, 3, 31, 41)
    w = np.random.default_rng(42).uniform(0.2, 3.0, len(scene))
    n = (72, 72)
    g, ext, _, _ = sc.scene_grid_numpy(scene, n, margin=4.0, reach=reach, weights=w)
    hmin = min(bw[d] for _, _, bw, dims in scene for d in dims)
    assert ext[1] <= 0.7 * hmin and ext[3] <= 0.7 * hmin, (ext, hmin)
    mass = g.sum() * ext[1] * ext[3]
    print(f"reach {reach}: steps {ext[1]:.4f} {ext[3]:.4f}, min h {hmin:.4f}, mass / sum(w) = {mass / w.sum():.9f}")
    assert mc.MASS_LO * w.sum() <= mass <= mc.MASS_HI * w.sum()
    # 1-D
    scene = scs.compact([(E1, (0,), 20)] * 5, 43)
    g, ext, _, _ = sc.scene_grid_numpy(scene, (130,), margin=4.0, reach=reach)
    assert ext[1] <= 0.7 * min(b[2][0] for b in scene)
    assert mc.MASS_LO * 5 <= g.sum() * ext[1] <= mc.MASS_HI * 5


# ---- 5. the owner -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(scs.owner_cases()))
def test_owner_is_the_argmax_of_the_stacked_terms(name):
    scene, n, reach, g, ext, own, stack = scs.restated(name)
    top = stack.max(axis=0)
    assert np.array_equal(own, np.where(top > 0, np.argmax(stack, axis=0), -1))
    total = np.zeros(n)
    for t in stack:
        total = total + t
    assert np.array_equal(g, total)
    # what the device leg relies on: the restatement alone excepts no more than 1 cell in 1000
    best, second, exc = scs.owner_exceptions(stack, scs.bound(scene, g))
    print(f"{name}: V={len(scene)} cells {g.size}, unowned {int((own < 0).sum())}, excepted {int(exc.sum())} ({exc.mean():.2e})")
    assert exc.mean() <= scs.OWNER_EXCEPTED and np.array_equal(best, own)
    if np.isfinite(reach) and reach < 6:
        assert (own < 0).any() or n[0] < 64


def test_ties_go_to_the_lower_index_and_weight_zero_owns_nothing():
    b = (E2, np.array([[0.0, 0.0], [0.5, 0.2]]), np.array([0.3, 0.3]), (0, 1))
    g, _, own, _ = sc.scene_grid_numpy([b, b, b], (9, 9), weights=[0.0, 1.0, 1.0], owner=True)
    assert np.all(own[g > 0] == 1) and np.all(own[g == 0] == -1)
    bad = (E2, b[1], np.array([0.3, 0.0]), (0, 1))
    g2, _, own2, skipped = sc.scene_grid_numpy([bad, b, bad, b], (9, 9), weights=[1.0, 1.0, 5.0, 1.0], owner=True)
    assert skipped.tolist() == [1, 0, 1, 0] and np.array_equal(g2, g) and np.all(np.isfinite(g2)) and np.all(own2[g2 > 0] == 1)
    # ... but on a coordinate it has a bandwidth on, the same belief is drawn
    g3, _, _, sk3 = sc.scene_grid_numpy([(E2, b[1], np.array([0.3, 0.0]), (0,))], (17,))
    assert not sk3.any() and np.all(g3 > 0)


# ---- refusals of the restatement -------------------------------------------------------------------------------------------------------
def test_restatement_refuses_what_the_library_refuses():
    a, s, c = scs.compact([(E2, (0, 1), 8), (SE2, (0, 2), 8), (CI, (0,), 8)], 51)
    for bad in ([a, s], [a, c], [s, (s[0], s[1], s[2], (2, 0))]):
        with pytest.raises(ValueError, match="admissible"):
            sc.scene_grid_numpy(bad, (8, 8)[:len(bad[0][3])])
    for kw in (dict(weights=[-1.0]), dict(weights=[np.nan]), dict(reach=0.0), dict(reach=np.nan), dict(lo=[0.0, 0.0], step=[0.1, 0.0]),
               dict(lo=[np.inf, 0.0], step=[0.1, 0.1]), dict(lo=[0.0, 0.0])):
        with pytest.raises(ValueError):
            sc.scene_grid_numpy([a], (8, 8), **kw)
    for n in ((0, 8), (abi.SCENE_MAX + 1, 8), (4096, 2048), (1, 8)):
        with pytest.raises(ValueError):
            sc.scene_grid_numpy([a], n)
    assert sc.scene_grid_numpy([], (3, 2), [0.0, 0.0], [1.0, 1.0])[0].tolist() == [[0.0, 0.0]] * 3   # an empty list: a grid of zeros


# ---- 6. the graph-level call ------------------------------------------------------------------------------------------------------------
def _graph():
    rng = np.random.default_rng(61)
    fg = iif.initfg(iif.SolverParams(N=24))
    scene = scs.poses_and_landmarks(4, 3, 24, 62)
    names = []
    for i, (m, X, bw, _) in enumerate(scene):
        v = f"x{i // 2}" if m == SE2 else f"l{i // 2}"
        iif.addVariable(fg, v, iif.SpecialEuclidean2 if m == SE2 else iif.ContinuousEuclid(2))
        iif.setValKDE(fg, v, scs.pc.to_points(m, X), bw)
        names.append(v)
    iif.addVariable(fg, "x9", iif.SpecialEuclidean2)      # never initialised: not part of the default list
    iif.addVariable(fg, "s0", iif.ContinuousScalar)       # has no second coordinate
    iif.setValKDE(fg, "s0", rng.normal(0, 1, (24, 1)), [0.3])
    return fg, dict(zip(names, scene))


def test_scene_grid_takes_lists_regular_expressions_and_dicts():
    fg, by = _graph()
    every = iif.sceneGrid(fg, n=(33, 20), owner=True)
    assert every.labels == ["l0", "l1", "l2", "x0", "x1", "x2", "x3"] and every.grid.shape == (33, 20) and every.skipped == []
    assert every.tile_beliefs is None and len(every.axes) == 2 and np.array_equal(every.axes[0], mg.grid_axes(every.extent, (33, 20))[0])
    want = sc.scene_grid_numpy([by[v] for v in every.labels], (33, 20), owner=True)
    assert np.array_equal(every.grid, want[0]) and every.extent.tobytes() == want[1].tobytes() and np.array_equal(every.owner, want[2])
    # .at: the label under a location
    for v in ("l1", "x2"):
        x, y = by[v][1][:, 0].mean(), by[v][1][:, 1].mean()
        k = every.index(x, y)
        assert every.at(x, y) == every.labels[every.owner[k]]
    assert every.at(-50.0, 0.0) is None
    with pytest.raises(ValueError):
        iif.sceneGrid(fg, n=8).at(0.0, 0.0)
    # a regular expression, as in findVariablesNear; a list keeps its order
    assert iif.sceneGrid(fg, "^l", n=8).labels == ["l0", "l1", "l2"]
    assert iif.sceneGrid(fg, ["x2", "l0"], n=8).labels == ["x2", "l0"]
    # weights as a dict: the others weigh 1
    heavy = iif.sceneGrid(fg, "^l", n=16, weights={"l1": 3.0})
    want = sc.scene_grid_numpy([by[v] for v in ("l0", "l1", "l2")], (16, 16), weights=[1.0, 3.0, 1.0])
    assert np.array_equal(heavy.grid, want[0])
    # dims as a dict: the variables it names, each on its own coordinates (x of a pose against y of a landmark)
    mixed = iif.sceneGrid(fg, dims={"x1": (1,), "l2": (2,)}, n=40)
    assert mixed.labels == ["l2", "x1"] and mixed.grid.shape == (40,)
    want = sc.scene_grid_numpy([(E2, by["l2"][1], by["l2"][2], (1,)), (SE2, by["x1"][1], by["x1"][2], (0,))], (40,))
    assert np.array_equal(mixed.grid, want[0])
    one = iif.sceneGrid(fg, dims=(1,), n=20)      # every initialised variable has a first coordinate
    assert one.labels == ["l0", "l1", "l2", "s0", "x0", "x1", "x2", "x3"]
    with pytest.raises(ValueError, match="cannot be drawn"):
        iif.sceneGrid(fg, dims={"x1": (1, 3), "l2": (1, 2)}, n=8)
    with pytest.raises(ValueError):
        iif.sceneGrid(fg, "^nobody", n=8)
    # an explicit extent
    ex = iif.sceneGrid(fg, "^x", n=(5, 4), extent=((0.0, 0.5), (-1.0, 0.5)))
    assert ex.extent.tolist() == [0.0, 0.5, -1.0, 0.5] and ex.axes[1].tolist() == [-1.0, -0.5, 0.0, 0.5]


def test_a_session_without_a_context_draws_the_host_copy():
    fg, by = _graph()
    with iif.SolveSession(fg) as ses:
        got = ses.sceneGrid("^l", n=12)
    assert np.array_equal(got.grid, iif.sceneGrid(fg, "^l", n=12).grid)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_scene_desc_layout_and_exports(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbp.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n",'
                   'sizeof(nbp_scene_desc),offsetof(nbp_scene_desc,n),offsetof(nbp_scene_desc,flags),offsetof(nbp_scene_desc,lo),'
                   'offsetof(nbp_scene_desc,step),offsetof(nbp_scene_desc,margin),offsetof(nbp_scene_desc,reach),NBP_SCENE_MAX,'
                   'NBP_SCENE_AUTO_EXTENT);return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = abi.SceneDesc
    assert got == [C.sizeof(D), D.n.offset, D.flags.offset, D.lo.offset, D.step.offset, D.margin.offset, D.reach.offset, abi.SCENE_MAX,
                   abi.SCENE_AUTO_EXTENT]
    hdr = open(os.path.join(ROOT, "include", "nbp.h")).read()
    assert "nbp_run_scene_grid(" in hdr and "nbp_run_scene_grid" in abi.EXPORTS
    assert f"#define NBP_SCENE_REACH {abi.SCENE_REACH}" in hdr and f"#define NBP_SCENE_MARGIN {abi.SCENE_MARGIN}" in hdr
    assert iif.sceneGrid is sc.sceneGrid and iif.Scene is sc.Scene and hasattr(iif.HipBackend, "run_scene_grid") and hasattr(iif.SolveSession, "sceneGrid")
