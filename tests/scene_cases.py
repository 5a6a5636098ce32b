"""Shared cases of the scene-density tests (tests/test_scene.py on the CPU, tests/test_gpu_scene.py on the device): the scenes, the
shapes and the criteria.  The definition is DESIGN.md 3 ("Scene densities") / incrementalinference.jl_amd/scene.py.

The shapes are the ones at which the tile kernel can go wrong: counts around its chunk of 32 (2-D) and 64 (1-D) particles, grids
around its tile of 32 x 32 (and 64 in 1-D), lists around the 64 records one ballot takes.

The criteria:

  value      |dev - ref| <= DENS_RTOL ref + sum_v w_v floor_v against scene_grid_numpy (exact sums), DENS_RTOL = 1e-12 and floor of
             tests/marginal_cases.py.  Every term is one marginal grid value held to DENS_RTOL there; the terms are non-negative,
             so the relative bound of one carries to their sum (three more roundings per term -- the division is already counted,
             the product with w and the addition -- add 2^-52 each, V of them against a sum that only grows: at V <= 130 that is
             3e-14, inside the 1e-12 that the marginal's own derivation leaves mostly unused).  floor_v: the clamp of exp_nonpos, as
             there.  The in-reach decisions are the same float64 operations on both sides and agree exactly.
  owner      equal to the restatement's wherever its best and second-best terms differ by more than twice that bound; elsewhere one
             of the two.  The excepted cells are at most 1 in 1000 per case (checked on the restatement alone in the CPU leg).
             The owner scenes are compact (no grid point further than 26 h from any particle per axis), so that no term underflows
             on the host while the device's clamp keeps it positive.
  mass       sum step0 step1 in sum(w) [1 - 2e-4, 1 + 1e-9] (marginal_cases.MASS_LO / MASS_HI, for the reason given there: with
             margin = 4 and reach >= 4 a belief loses at most 2 Q(4) = 6.3e-5 per Euclidean axis) at a step <= 0.7 min h.
"""
import functools

import numpy as np

import marginal_cases as mc
import ppe_cases as pc
from parity_utils import abi, coords, iif

sc = iif.scene
E1, E2, E3, CI, SE2 = abi.EUCLID1, abi.EUCLID2, abi.EUCLID3, abi.CIRCULAR, abi.SE2
DENS_RTOL = mc.DENS_RTOL
COUNTS = (1, 2, 31, 32, 33, 64, 65)   # 64 and 65 need a context above 64: N = 80, so both are counts below the context's N as well
GRIDS = ((1, 1), (1, 17), (31, 33), (32, 32), (33, 65), (96, 40))
SIZES_1D = (1, 63, 64, 65, 130)
LIST_V = (1, 2, 63, 64, 65, 130)      # from 63 on at N = 16
REACHES = (np.inf, 6.0, 1.5)
# (manifold, 0-based dims): Euclid(2), Euclid(3) on each ordered pair, SE(2) on (x, y), (x, theta), (theta, y) -- and their transposes
DIMS_2D = [(E2, (0, 1)), (E2, (1, 0))] + [(E3, (a, b)) for a in range(3) for b in range(3) if a != b] + \
          [(SE2, (0, 1)), (SE2, (1, 0)), (SE2, (0, 2)), (SE2, (2, 0)), (SE2, (2, 1)), (SE2, (1, 2))]
DIMS_1D = [(E1, (0,)), (CI, (0,))]
OWNER_EXCEPTED = 1e-3


def cloud(manifold, c, rng, centre, sd=0.1):
    """c points around `centre` (one entry per coordinate); circular coordinates wrapped"""
    D = abi.MANIFOLD_DIM[manifold]
    X = rng.normal(np.asarray(centre, dtype=float)[:D], sd, (c, D))
    for d in pc.circular_coords(manifold):
        X[:, d] = pc.wrap(X[:, d])
    return X


def bandwidth(manifold, rng, lo=0.2, hi=0.3):
    return rng.uniform(lo, hi, abi.MANIFOLD_DIM[manifold])


def make(specs, seed, span=2.0, sd=0.1, h=(0.2, 0.3)):
    """specs = [(manifold, dims, count)] -> the scene [(manifold, X, bw, dims)], centres uniform in [0, span] per coordinate
    (circular coordinates: anywhere on the circle)"""
    rng = np.random.default_rng(seed)
    out = []
    for m, dims, c in specs:
        centre = rng.uniform(0.0, span, 3)
        for d in pc.circular_coords(m):
            centre[d] = rng.uniform(-np.pi, np.pi)
        bw = bandwidth(m, rng, *h)
        for d in pc.circular_coords(m):   # (a circular axis never culls: no point of it further than pi / 0.15 = 21 h away)
            bw[d] = max(bw[d], rng.uniform(0.15, 0.25))
        out.append((m, cloud(m, c, rng, centre, sd), bw, tuple(dims)))
    return out


def compact(specs, seed):
    """no grid point of the automatic extent (margin 4) lies further than 26 h from a particle on an axis: span 2, clouds of
    sd 0.1 (+-0.4 at most), h >= 0.2 -> (2 + 2 (0.4 + 4 0.3)) / 0.2 = 26"""
    return make(specs, seed, span=2.0, sd=0.1, h=(0.2, 0.3))


def spread(specs, seed):
    """beliefs far apart against their bandwidths: most tiles see few of them, and some grid points none"""
    return make(specs, seed, span=12.0, sd=0.1, h=(0.08, 0.12))


def poses_and_landmarks(n_pose, n_land, c, seed, span=2.0):
    """SE(2) poses on (x, y) mixed with Euclid(2) landmarks, alternating from the start of the list"""
    specs = []
    for i in range(max(n_pose, n_land)):
        if i < n_pose:
            specs.append((SE2, (0, 1), c))
        if i < n_land:
            specs.append((E2, (0, 1), c))
    return make(specs, seed, span=span)


def write(be, scene, first=0):
    """the scene into slots first .. -> (slots, manifolds, the scene as the device holds it: coordinates and bandwidths read back)"""
    slots = list(range(first, first + len(scene)))
    mans = [s[0] for s in scene]
    be.beliefs_write(slots, mans, [(pc.to_points(m, X), bw, None) for m, X, bw, _ in scene])
    back = be.beliefs_read(slots, mans)
    held = []
    for (m, X, bw, dims), (pts, bwb, _) in zip(scene, back):
        assert len(pts) == len(X)
        held.append((m, coords(m, pts), bwb, dims))
    return slots, mans, held


def explicit_extent(scene, n, rng, margin=(1.0, 3.0)):
    """flat (lo, step) per axis: a Euclidean axis from up to 3 h below the scene's clouds to up to 3 h above them; a circular axis a
    full turn from a random start (the grid crosses +-pi)"""
    ext = []
    m0, _, _, dims0 = scene[0]
    for a in range(len(dims0)):
        if dims0[a] in pc.circular_coords(m0):
            ext += [-np.pi + rng.uniform(0, 1), 2 * np.pi / n[a]]
        else:
            lo = min(X[:, dims[a]].min() - rng.uniform(*margin) * bw[dims[a]] for _, X, bw, dims in scene)
            hi = max(X[:, dims[a]].max() + rng.uniform(*margin) * bw[dims[a]] for _, X, bw, dims in scene)
            ext += [lo, (hi - lo) / max(n[a] - 1, 1)]
    return np.array(ext)


def can_auto(scene, n):
    """whether the automatic extent takes these sizes: n >= 2 on every Euclidean axis"""
    m, _, _, dims = scene[0]
    return all(n[a] >= 2 or d in pc.circular_coords(m) for a, d in enumerate(dims))


def usable(bel):
    m, X, bw, dims = bel
    return all(np.isfinite(bw[d]) and bw[d] > 0 for d in dims)


def floor_sum(scene, weights=None):
    w = np.ones(len(scene)) if weights is None else np.asarray(weights, dtype=float)
    return float(sum(wv * mc.floor(len(b[1]), b[2], b[3]) for wv, b in zip(w, scene) if usable(b)))


def bound(scene, ref, weights=None):
    """the value criterion, cell by cell"""
    return DENS_RTOL * ref + floor_sum(scene, weights)


def check_values(scene, dev, ref, weights=None, what=""):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    err, b = np.abs(dev - ref), bound(scene, ref, weights)
    print(f"{what}: V={len(scene)} grid {ref.shape}, ref in [{ref.min():.3e}, {ref.max():.3e}], zeros {int((ref == 0).sum())}, "
          f"largest error / bound = {np.max(err / b):.3e}")
    assert np.all(err <= b), (what, float(np.max(err / b)))


def owner_exceptions(stack, ref):
    """(best index or -1, second-best index or -1, excepted cells) of the restatement: excepted where the best and the second-best
    term differ by no more than twice the value bound (given as `ref` = the bound array)"""
    V = stack.shape[0]
    best = np.argmax(stack, axis=0)
    bv = np.take_along_axis(stack, best[None], axis=0)[0]
    if V > 1:
        rest = stack.copy()
        np.put_along_axis(rest, best[None], -1.0, axis=0)
        second = np.argmax(rest, axis=0)
        sv = np.take_along_axis(rest, second[None], axis=0)[0]
    else:
        second, sv = np.full(best.shape, -1), np.zeros(best.shape)
    best = np.where(bv > 0, best, -1)
    second = np.where(sv > 0, second, -1)
    excepted = (bv > 0) & (bv - np.maximum(sv, 0.0) <= 2 * ref)
    return best, second, excepted


def check_owner(scene, dev_owner, stack, ref, weights=None, what=""):
    best, second, exc = owner_exceptions(stack, bound(scene, ref, weights))
    share = exc.mean()
    print(f"{what}: owner cells {best.size}, excepted {int(exc.sum())} ({share:.2e}), unowned {int((best < 0).sum())}")
    assert share <= OWNER_EXCEPTED, (what, share)
    assert np.array_equal(dev_owner[~exc], best[~exc]), (what, int((dev_owner[~exc] != best[~exc]).sum()))
    assert np.all((dev_owner[exc] == best[exc]) | (dev_owner[exc] == second[exc])), what


# ---- the cases both legs share (the CPU leg checks what the restatement alone can say; the device leg holds the device to it) -----------
def owner_cases():
    """name -> (scene, n, reach): compact scenes for the owner criterion"""
    return {
        "poses+landmarks 96x40": (poses_and_landmarks(6, 4, 33, 21), (96, 40), 6.0),
        "euclid3 (2,0) 33x65 inf": (compact([(E3, (2, 0), c) for c in (31, 32, 33, 16)], 22), (33, 65), np.inf),
        "se2 (x,theta) 31x33 1.5": (compact([(SE2, (0, 2), 40)] * 5, 23), (31, 33), 1.5),
        "130 beliefs 32x32": (compact([(E2, (0, 1), 16)] * 130, 24), (32, 32), 6.0),
        "circular 130": (compact([(CI, (0,), 33)] * 3, 25), (130,), 6.0),
        "euclid1 65": (compact([(E1, (0,), 64)] * 4, 26), (65,), 1.5),
    }


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of an owner case on the HOST's own scene (the CPU leg): (scene, n, reach, grid, ext, owner, stack)"""
    scene, n, reach = owner_cases()[name]
    g, ext, own, skipped, stack = sc.scene_grid_numpy(scene, n, reach=reach, owner=True, terms=True)
    return scene, n, reach, g, ext, own, stack


def tile_hits(scene, n, ext, reach):
    """the (tile, belief) pairs the tile kernel works on: tiles of 32 x 32 points (64 in 1-D), a usable belief hit when the span of
    the tile's points meets its cull box on every Euclidean axis -- the device's test, in the same float64 operations"""
    tile = 32 if len(n) == 2 else 64
    G = iif.marginal.grid_axes(ext, n)
    reach = np.float64(reach)
    total = 0
    for m, X, bw, dims in scene:
        if not usable((m, X, bw, dims)):
            continue
        per_axis = []
        for a, d in enumerate(dims):
            starts = range(0, n[a], tile)
            if d in pc.circular_coords(m):
                per_axis.append(len(starts))
                continue
            cl, ch = X[:, d].min() - reach * bw[d], X[:, d].max() + reach * bw[d]
            hit = 0
            for o in starts:
                ga, gb = G[a][o], G[a][min(o + tile, n[a]) - 1]
                hit += int(cl <= max(ga, gb) and min(ga, gb) <= ch)
            per_axis.append(hit)
        total += int(np.prod(per_axis))
    return total


def n_tiles(n):
    return int(np.prod([-(-k // 32) for k in n])) if len(n) == 2 else -(-n[0] // 64)
