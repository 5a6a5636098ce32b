"""Cases shared by the two legs of the belief-overlap tests (test_overlap.py on the host, test_gpu_overlap.py on the device): every
(manifold, mask) and every admissible pair of them, the clouds, the device-against-restatement tolerance -- likelihood_cases.py's
rule, worked out per case from the restatement's own rounding noise --, and the scenes of the search tests."""
import itertools

import numpy as np

import ppe_cases as pc
from parity_utils import abi, iif

ov = iif.overlap
MANIFOLDS = pc.MANIFOLDS
# every (manifold, 0-based bit mask)
SIDES = [(m, k) for m in MANIFOLDS for k in range(1, 1 << abi.MANIFOLD_DIM[m])]
# every admissible ordered pair of them, a pair of one side with itself included: 99
ADMISSIBLE = [(a, b) for a, b in itertools.product(SIDES, SIDES) if ov.mask_kinds(*a) == ov.mask_kinds(*b)]
CLOUDS = ("gaussian", "bimodal", "identical", "far")


def bandwidth(manifold, scale=1.0):
    return scale * np.array([0.3, 0.4, 0.2])[:abi.MANIFOLD_DIM[manifold]]


def cloud(kind, manifold, n, rng, shift=0.0):
    """tangent coordinates (n x D); circular coordinates wrapped to [-pi, pi).  `far`: 10^3 bandwidths from the origin"""
    D = abi.MANIFOLD_DIM[manifold]
    if kind == "gaussian":
        X = rng.normal(0.3 + shift, 0.5, (n, D))
    elif kind == "bimodal":
        X = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)[:, None] + shift + rng.normal(0, 0.2, (n, D))
    elif kind == "identical":
        X = np.tile(rng.normal(0.2 + shift, 0.5, (1, D)), (n, 1))
    elif kind == "far":
        X = rng.normal(300.0 + shift, 0.5, (n, D))
    else:
        raise KeyError(kind)
    for d in pc.circular_coords(manifold):
        X[:, d] = rng.uniform(-np.pi, np.pi, n) if kind == "gaussian" else pc.wrap(X[:, d])
    return np.ascontiguousarray(X)


def restate(ma, A, ha, ka, mb, B, hb, kb):
    """the restatement of one pair in float64 and in long double -> (values[4], tol[4]) for logc, L_ab, L_aa, L_bb:
    16 max(|float64 - long double|, 4 ulp(max(1, |l|))), computed on the host, never from the device (likelihood_cases.restate's
    rule: the restatement's own rounding noise measures the case's conditioning; the factor 16 covers the device's exp and log,
    another block-sum tree and up to 512^2 terms)"""
    r64 = np.array([float(v) for v in ov.overlap_numpy(ma, A, ha, ka, mb, B, hb, kb)])
    r80 = np.array(ov.overlap_numpy(ma, A, ha, ka, mb, B, hb, kb, dtype=np.longdouble), dtype=np.longdouble)
    with np.errstate(invalid="ignore"):
        noise = np.abs((r64.astype(np.longdouble) - r80).astype(np.float64))
        tol = 16 * np.maximum(noise, 4 * np.spacing(np.maximum(1.0, np.abs(r64))))
    return r64, tol


def hold(got, ref, what):
    """a device record against `restate`; prints error / tolerance before it asserts; returns the largest ratio"""
    r64, tol = ref
    worst = 0.0
    for g, r, t, w in zip(got, r64, tol, ("logc", "L_ab", "L_aa", "L_bb")):
        if np.isnan(r):
            assert np.isnan(g), f"{what} {w}: device {g!r}, restatement NaN"
            continue
        ratio = abs(g - r) / t if np.isfinite(g) else np.inf
        worst = max(worst, ratio)
        print(f"{what} {w}: device {g!r} restatement {r!r} tol {t:.3e} ratio {ratio:.3f}")
        assert ratio <= 1.0, f"{what} {w}: device {g!r}, restatement {r!r}, tolerance {t:.3e}"
    return worst


# ---- the scenes of the search tests: lists of (manifold, tangent coordinates, bandwidth, mask) ------------------------------------------
def loop_chain(V=300, n=64, seed=5):
    """V Euclid(2) poses one unit apart on a closed loop: pose V - 1 stands next to pose 0"""
    rng = np.random.default_rng(seed)
    R = V / (2 * np.pi)
    th = 2 * np.pi * np.arange(V) / V
    return [(abi.EUCLID2, rng.normal([R * np.cos(t), R * np.sin(t)], 0.3, (n, 2)), np.array([0.15, 0.15]), 3) for t in th]


def poses_and_landmarks(n=64, seed=6):
    """40 SE(2) poses on a line, x-y compared, and 20 Euclid(2) landmarks beside every second one"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(40):
        X = np.c_[rng.normal([0.8 * i, 0.0], 0.25, (n, 2)), rng.uniform(-np.pi, np.pi, n)]
        out.append((abi.SE2, X, np.array([0.12, 0.12, 0.3]), 3))
    for k in range(20):
        out.append((abi.EUCLID2, rng.normal([1.6 * k, 0.6], 0.2, (n - 7, 2)), np.array([0.1, 0.1]), 3))
    return out


def circular_beliefs(V=40, n=64, seed=7):
    rng = np.random.default_rng(seed)
    return [(abi.CIRCULAR, pc.wrap(rng.normal(2 * np.pi * i / V, 0.25, (n, 1))), np.array([0.1]), 1) for i in range(V)]


def clusters(k=3, n=64, seed=8):
    """with topk = k: an isolated belief (0 partners), clusters of k, k + 1 and k + 2 beliefs (k - 1, k and k + 1 partners each: the
    last truncated), the clusters 100 units apart.  In the last cluster beliefs 1, 2 and 3 are bit-identical copies: every other
    belief ties on them.  The order is shuffled so that a copy with a lower list index is not the first one met."""
    rng = np.random.default_rng(seed)
    out = []
    for c, size in enumerate((1, k, k + 1, k + 2)):
        base = [rng.normal([100.0 * c, 0.0], 0.3, (n, 2)) for _ in range(size)]
        if size == k + 2:
            base[2], base[3] = base[1].copy(), base[1].copy()
        out += [(abi.EUCLID2, X, np.array([0.15, 0.15]), 3) for X in base]
    order = np.random.default_rng(seed + 1).permutation(len(out))
    return [out[i] for i in order]


def write_scene(be, scene, first=0):
    """the scene into slots first .. -> (slots, manifolds, masks)"""
    slots = list(range(first, first + len(scene)))
    mans = [s[0] for s in scene]
    be.beliefs_write(slots, mans, [(pc.to_points(m, X), bw, None) for m, X, bw, _ in scene])
    return slots, mans, [s[3] for s in scene]
