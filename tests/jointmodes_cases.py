"""Cases shared by the two legs of the joint-hypothesis tests (test_jointmodes.py on the host, test_gpu_jointmodes.py on the device):
the measurement models are those of likelihood_cases.CASES; here are the label rows, the per-cell restatement with its tolerance --
worked out per cell from the restatement's own two runs, never from the device --, and the scenes of the joint-score tests."""
import numpy as np

import likelihood_cases as lc
from parity_utils import abi, iif

jm = iif.jointmodes
MAXK = abi.MAXK
CASES = lc.CASES  # the measurement models: the table of the factor-likelihood tests


def labels(rng, n, K, minus=0.0, empty=None, last=None):
    """one group in 0 .. K-1 per point, every group with at least one member where n allows; `minus`: the share of points
    labelled -1; `empty`: a group that gets no member; `last`: a group whose members all sit behind index n - n % 64 (the last wave)
    and that no other point joins"""
    groups = [g for g in range(K) if g != empty and g != last]
    lab = np.array([groups[i % len(groups)] for i in range(n)], dtype=np.int32)
    rng.shuffle(lab)
    if last is not None:
        tail = max((n - 1) // 64 * 64, 0)
        lab[tail + (n - tail) // 2:] = last
    if minus:
        lab[rng.random(n) < minus] = -1
    return lab


def pair_terms(d, A, B):
    """e_ijc of an item in float64 and in long double: what `restate` shares among the groupings of the same clouds"""
    return iif.likelihood.pair_terms(d, A, B), iif.likelihood.pair_terms(d, A, B, np.longdouble)


def restate(d, A, la, B, lb, terms=None):
    """the restatement of one item in float64 and in long double, and the tolerance a device cell is held to:
    16 max(|float64 - long double|, 4 ulp(max(1, |T|))), as likelihood_cases.restate has it for loglik; terms: `pair_terms(d, A, B)`
    where several groupings of the same clouds are restated -> (table[8, 8], counts[2, 8], tol[8, 8])"""
    e64, e80 = (None, None) if terms is None else terms
    t64, c64 = jm.factor_mode_likelihood_numpy(d, A, la, B, lb, terms=e64)
    t80, _ = jm.factor_mode_likelihood_numpy(d, A, la, B, lb, dtype=np.longdouble, terms=e80)
    fin = np.isfinite(t64)
    with np.errstate(invalid="ignore"):
        noise = np.abs((t64.astype(np.longdouble) - t80).astype(np.float64))
        ulp = 4 * np.spacing(np.maximum(1.0, np.abs(t64)))
    tol = np.where(fin, 16 * np.maximum(np.where(fin, noise, 0.0), np.where(fin, ulp, 0.0)), 0.0)
    return np.asarray(t64, dtype=np.float64), c64, tol


def hold(got, ref, what, tol=None):
    """a table against `restate`: finite cells within the tolerance, -inf and NaN where the restatement has them.  Prints the ratio
    error / tolerance of every finite cell before it asserts; returns the largest.  tol: another tolerance table (the sub-cloud
    comparison brings its own)"""
    t64, _, t = ref
    t = t if tol is None else tol
    got = np.asarray(got, dtype=np.float64)
    worst = 0.0
    for k in range(MAXK):
        for l in range(MAXK):
            g, r = got[k, l], t64[k, l]
            if np.isfinite(r):
                ratio = abs(g - r) / t[k, l] if np.isfinite(g) else np.inf
                worst = max(worst, ratio)
                print(f"{what} T[{k},{l}]: got {g!r} restatement {r!r} tol {t[k, l]:.3e} ratio {ratio:.3f}")
                assert ratio <= 1.0, f"{what} T[{k},{l}]: got {g!r}, restatement {r!r}, tolerance {t[k, l]:.3e}"
            else:
                assert (np.isnan(g) and np.isnan(r)) or g == r, f"{what} T[{k},{l}]: got {g!r}, restatement {r!r}"
    return worst


# ---- the scenes of the joint-score tests ---------------------------------------------------------------------------------------------
RING_SEED = 2024


def ring_graph(with_cu=True, n=64, seed=RING_SEED):
    """Euclid(1), N = 64, bandwidth 0.05, clusters of sigma 0.1 ten units apart: a at {0, 10} with 32 / 32 points, b at {1, 11}
    with 40 / 24, c at {2, 12} with 24 / 40, u unimodal at 3; LinearRelative Normal(1, 0.2) on a-b, b-c and c-u, Normal(2, 0.2) on
    a-c.  The heavier cluster of b is the low one and that of c the high one, so mode rank and position do not go together."""
    rng = np.random.default_rng(seed)

    def two(lo, n_lo):
        x = np.concatenate([rng.normal(lo, 0.1, n_lo), rng.normal(lo + 10.0, 0.1, n - n_lo)])
        rng.shuffle(x)
        return x.reshape(-1, 1)
    vals = {"a": two(0.0, 32), "b": two(1.0, 40), "c": two(2.0, 24), "u": rng.normal(3.0, 0.1, (n, 1))}
    fg = iif.initfg(iif.SolverParams(N=n))
    for v in ("a", "b", "c", "u"):
        iif.addVariable(fg, v, iif.ContinuousScalar)
        iif.setValKDE(fg, v, vals[v], [0.05])
    iif.addFactor(fg, ["a", "b"], iif.LinearRelative(iif.Normal(1.0, 0.2)), label="ab")
    iif.addFactor(fg, ["b", "c"], iif.LinearRelative(iif.Normal(1.0, 0.2)), label="bc")
    iif.addFactor(fg, ["a", "c"], iif.LinearRelative(iif.Normal(2.0, 0.2)), label="ac")
    if with_cu:
        iif.addFactor(fg, ["c", "u"], iif.LinearRelative(iif.Normal(1.0, 0.2)), label="cu")
    return fg


def doors_graph(n=64, seed=77):
    """x bimodal at {0.05, 2.05} (24 / 40 points), l1 at 0, l2 at 2 (sigma 0.1, bandwidth 0.05); a door sighting Normal(0, 0.2) from
    x with the landmarks as two hypotheses [1, .5, .5]; a prior Normal(2, 0.2) on x"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.normal(0.05, 0.1, 24), rng.normal(2.05, 0.1, n - 24)])
    rng.shuffle(x)
    vals = {"x": x.reshape(-1, 1), "l1": rng.normal(0.0, 0.1, (n, 1)), "l2": rng.normal(2.0, 0.1, (n, 1))}
    fg = iif.initfg(iif.SolverParams(N=n))
    for v in ("x", "l1", "l2"):
        iif.addVariable(fg, v, iif.ContinuousScalar)
        iif.setValKDE(fg, v, vals[v], [0.05])
    iif.addFactor(fg, ["x", "l1", "l2"], iif.LinearRelative(iif.Normal(0.0, 0.2)), multihypo=[1.0, 0.5, 0.5], label="door")
    iif.addFactor(fg, ["x"], iif.Prior(iif.Normal(2.0, 0.2)), label="xprior")
    return fg


def mode_near(bm, where):
    """the rank of the mode of a one-dimensional belief that lies nearest `where`"""
    return int(np.argmin(np.abs(np.asarray(bm.modes)[:, 0] - where)))


def hold_joint(got, ref, fg, what):
    """a JointModes from the device against the numpy route: the same best, combos and labels; every table cell within restate's
    tolerance, the scores within the summed tolerances of the cells"""
    assert got.variables == ref.variables and got.best == ref.best and got.skipped == ref.skipped, what
    assert np.array_equal(got.combos, ref.combos), what
    for v in ref.modes:
        assert np.array_equal(got.modes[v].labels, ref.modes[v].labels), (what, v)
    total = 0.0
    for f, r in ref.tables.items():
        plan = iif.likelihood.factor_items(fg, f)
        for h, (d, (a, b)) in enumerate(zip(plan.descs, plan.roles)):
            rs = restate(d, fg.getVal(a), jm.label_row(ref.modes[a]), None if b is None else fg.getVal(b),
                         None if b is None else jm.label_row(ref.modes[b]))
            full = np.full((MAXK, MAXK), np.nan)
            t = got.tables[f].tables[h]
            full[:t.shape[0], :t.shape[1]] = t
            hold(full, rs, f"{what} {f}[{h}]")
            total += float(rs[2][np.isfinite(rs[0])].max(initial=0.0))
    fin = np.isfinite(ref.logscores)
    print(f"{what}: scores differ by {np.abs(got.logscores[fin] - ref.logscores[fin]).max(initial=0.0):.3e}, summed tolerance {total:.3e}")
    assert np.array_equal(np.isfinite(got.logscores), fin) and np.all(np.abs(got.logscores[fin] - ref.logscores[fin]) <= total), what
    assert abs(got.best_logscore - ref.best_logscore) <= total and abs(got.logZ - ref.logZ) <= total, what
