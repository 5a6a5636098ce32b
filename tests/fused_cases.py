"""Shared cases of the fused variable-update kernel's tests (csrc/nbp_fused.h; planned by fused_plan / schedule_fused_pair /
launch_update in csrc/nbp_api.hip): written once, run on the oracle alone (tests/test_fused_cases.py) and on the device
against the oracle and against the three-launch form of the same program (tests/test_gpu_fused_update.py).

A round is `nops` variable updates on Euclid(2), each the product of F proposals on its own target; a *recipe* per input
names the proposal that feeds it (RECIPES).  The criterion is the project's standing invariant (README, round 6): with the
same Philox keys the device's points, bandwidths and infoPerCoord are the oracle's bit for bit -- `np.array_equal`, no
tolerance -- for every output slot and every proposal slot the program leaves written, fused or not.

Arena of a case: slots 0 .. 5 hold the operands (A, B: the other variables of the relatives; T: the target; KDE: the
density a MsgPrior / a `meas_kde` relative samples; DEN: the density of a pass-through; one spare), update i owns the
slots BASE + stride * i ...: its F proposals, then its output.

What keeps a round in the fused kernel's class and what the planner refuses, as found in proposals_uniform_class and
fused_plan (nothing else writes this list down):

  ACCEPTED -- Euclid(2) throughout, full (non-partial) LinearRelative / Prior / MsgPrior / pass-through proposals, with
    nullhypo, has_multihypo (and nvars > 2), mixtures (ncomp > 1), injected and recorded hypothesis indices (mhidx_in /
    mhidx_out), stored measurements (meas_seed), a KDE as the measurement (meas_kde), either solve direction (sfidx),
    any inflate_cycles / niter; a pass-through as one input among several, or alone when it does not keep its count;
    skip_bandwidth on the single proposal of a pass-through product (F = 1); operand slots holding fewer than N points;
    1 <= F <= 4; proposals that later stages read from their slots (written by the launch as well).
  REFUSED -- fused_updates off (option, NBP_NO_FUSED_UPDATE), fewer than NBP_FUSED_MIN updates, Npad > 256, an LDS need
    above 158 KiB; another manifold, a partial proposal (partial_mask), a relative of another kind; a product with
    labels_out, with old_slot (hence every product with partial inputs: in_partial requires old_slot), with more than 4
    inputs, with an input that is not exactly one proposal of the stage in front, or a proposal that feeds no product
    or two; two ops writing one slot; a skip_bandwidth proposal (not a pass-through) feeding a product of several; a
    lone pass-through with keep_count (1: the density's own count; 2: topped up to N); a proposal that reads another
    update's output or another proposal's slot."""
import numpy as np

from parity_utils import abi, iif, rand_points, relative_factor_desc

MAN = abi.EUCLID2
A, B, T, KDE, DEN, SPARE = range(6)
BASE = 6
NOPS = 16  # with NBP_FUSED_MIN = 16 the smallest round that fuses

# ---- the LDS need of a fused workgroup, restated from nbp_update_lds_layout (csrc/nbp_fused.h) ---------------------------
NBP_EXPTAB, NBP_RED, NBP_KD_PARTS = 256, 64, 512
LDS_CEILING = 158 * 1024


def npad(N):
    return (N + 63) // 64 * 64


def kd_doubles(D, N, Npad, P):
    return (D * N + 3 * Npad + NBP_RED + 2 * NBP_KD_PARTS) + (2 * N + P * Npad + 2 + 1) // 2


def lds_bytes(Fmax, D, N, Npad, P, circ=False):
    SL = 3 * N + 8
    o = NBP_EXPTAB + Fmax * SL + Fmax * 3 + Fmax * 3
    tr = (o + 1) & ~1
    prop = 3 * N + NBP_RED + (N + 1) // 2
    fit = 2 * N + P * Npad + (P * Npad // 64) * 2 * N + NBP_RED + NBP_EXPTAB
    kd = kd_doubles(D, N, Npad, P) + (N + 1) // 2
    bulk = Fmax * D * N
    prod = 3 * bulk + (2 * Fmax * N if circ else 0) + Fmax * N + 6 * Fmax + N + 2 * Fmax * Npad + (Fmax * Npad * 2 + 1) // 2
    return (tr + max(prop, fit, kd, prod)) * 8


def admits(N, F):
    """does nbp_program_finalize run a round of products of F densities fused at N particles?  (fused_plan: Npad <= 256;
    the launch is sized for max(F, 2) densities, the bound is taken at two helper rows)"""
    return npad(N) <= 256 and lds_bytes(max(F, 2), 2, N, npad(N), 2) <= LDS_CEILING


# ---- recipes: (case, update i, input j, out slot, seed, target slot) -> nbp_proposal_desc ---------------------------------
MIX = [(0.6, [1.0, 1.0], [0.3, 0.3]), (0.4, [1.5, 0.5], [0.2, 0.4])]


def _rel(c, i, j, o, seed, tgt, **kw):
    return relative_factor_desc(abi.F_LINREL, MAN, 2, 1, [j % 2, tgt], o, seed, [1.0 - j, 1.0 - j], [0.1, 0.1], **kw)


def _prior(c, i, j, o, seed, tgt, kind=abi.F_PRIOR, other=None, **kw):
    return relative_factor_desc(kind, MAN, 1, 0, [tgt] if other is None else [tgt, other], o, seed, [1.0, 1.0], [0.3, 0.3], **kw)


def _with(d, **fields):
    for k, v in fields.items():
        setattr(d, k, v)
    return d


RECIPES = {
    # the two proposals every earlier test of the kernel ran (`_round` of test_gpu_fused_update.py)
    "rel": _rel,                                                                       # solves for the second variable (sfidx 1)
    "prior": _prior,
    "rel_sf0": lambda c, i, j, o, s, t: relative_factor_desc(abi.F_LINREL, MAN, 2, 0, [t, j % 2], o, s, [j - 1.0, j - 1.0], [0.1, 0.1]),
    "prior_nh": lambda c, i, j, o, s, t: _prior(c, i, j, o, s, t, nullhypo=0.5),
    "prior_nh_inj": lambda c, i, j, o, s, t: _prior(c, i, j, o, s, t, nullhypo=0.5, mhidx_in=c.inj_off),
    "rel_nh": lambda c, i, j, o, s, t: _rel(c, i, j, o, s, t, nullhypo=0.3, mhidx_out=c.rec_off(i, j)),
    "prior_mix": lambda c, i, j, o, s, t: _prior(c, i, j, o, s, t, ncomp=2, comps=MIX),
    "rel_mix": lambda c, i, j, o, s, t: _rel(c, i, j, o, s, t, ncomp=2, comps=MIX),
    "rel_mh": lambda c, i, j, o, s, t: relative_factor_desc(abi.F_LINREL, MAN, 3, 0, [t, A, B], o, s, [-1.0, -1.0], [0.1, 0.1],
                                                             multihypo=[0.0, 0.6, 0.4], mhidx_out=c.rec_off(i, j)),
    "msg": lambda c, i, j, o, s, t: _prior(c, i, j, o, s, t, kind=abi.F_MSGPRIOR, other=KDE),
    "rel_kde": lambda c, i, j, o, s, t: _with(_rel(c, i, j, o, s, t), meas_kde=KDE + 1),
    "rel_stored": lambda c, i, j, o, s, t: _with(_rel(c, i, j, o, s, t), meas_seed=77000 + 5 * i + j),
    "prior_stored": lambda c, i, j, o, s, t: _with(_prior(c, i, j, o, s, t), meas_seed=88000 + 5 * i + j),
    "rel_skipbw": lambda c, i, j, o, s, t: _with(_rel(c, i, j, o, s, t), skip_bandwidth=1),
    "pass": lambda c, i, j, o, s, t: _prior(c, i, j, o, s, t, kind=abi.F_PASSTHROUGH, other=DEN),
    "pass_init": lambda c, i, j, o, s, t: _with(_prior(c, i, j, o, s, t, kind=abi.F_PASSTHROUGH, other=DEN), keep_count=2),
    "pass_keep": lambda c, i, j, o, s, t: _with(_prior(c, i, j, o, s, t, kind=abi.F_PASSTHROUGH, other=DEN), keep_count=1),
    "rel_partial": lambda c, i, j, o, s, t: _rel(c, i, j, o, s, t, partial_mask=1),
}


def build_round(N, F, nops, recipes, base=4, stride=None, prop_off=0, out_off=None, target=None, seed0=900, pseed0=5000,
                case=None, **prod_kw):
    """`nops` updates, update i the product of F proposals on the target slot `target(i)` (default T): input j is fed by
    RECIPES[recipes[j]] (or recipes(i, j)); proposals at base + stride * i + prop_off + j, the output at ... + out_off.
    -> (proposal descriptors, product descriptors, stride).  `prod_kw`: niter / labels_out / partials / old_slot of the
    products (labels_out = True: each product its own area of the side buffer).  `case` gives the recipes that use the
    side buffer their offsets."""
    stride = F + 1 if stride is None else stride
    out_off = F if out_off is None else out_off
    props, prods = [], []
    for i in range(nops):
        o = base + stride * i
        tgt = T if target is None else target(i)
        ins = []
        for j in range(F):
            name = recipes(i, j) if callable(recipes) else recipes[j]
            props.append(RECIPES[name](case, i, j, o + prop_off + j, seed0 + 7 * i + j, tgt))
            ins.append(o + prop_off + j)
        kw = dict(prod_kw)
        if kw.get("labels_out") is True:
            kw["labels_out"] = case.lab_off(i)
        prods.append(iif.solver.product_desc(MAN, ins, o + out_off, pseed0 + i, **kw))
    return props, prods, stride


def legacy_round(nops, F):
    """the round of every earlier test of the kernel: relatives from slot 0 / 1 and, last of several inputs, a plain prior;
    operands in slots 0 .. 2, updates from slot 4 (imported as `_round` by test_gpu_product_first_label.py)"""
    return build_round(0, F, nops, ["prior" if (j == F - 1 and F > 1) else "rel" for j in range(F)], base=4)


class Case:
    """one program: operands, stages, the slots to read back.  The default program is one round (PROPOSALS, PRODUCTS)."""

    def __init__(self, N, F, recipes, nops=NOPS, counts=None, preset_bw=(), seed=11, name="", **prod_kw):
        self.N, self.F, self.nops, self.recipes, self.name = N, F, nops, recipes, name
        self.counts = dict(counts or {})       # operand slot -> points it holds (default N)
        self.preset_bw = tuple(preset_bw)      # inputs whose proposal slots hold a bandwidth beforehand (skip_bandwidth)
        self.seed, self.prod_kw = seed, prod_kw
        self.side_ints = (2 * nops * 4 + 1) * N
        self.inj_off = nops * 4 * N
        self.lazy = False
        self.out_count = N                     # points every output belief holds
        self._build()

    def rec_off(self, i, j):   # recorded hypothesis indices of proposal (i, j)
        return (4 * i + j) * self.N

    def lab_off(self, i):      # labels of product i
        return (self.nops * 4 + 1 + 4 * i) * self.N

    def _build(self):
        props, prods, stride = build_round(self.N, self.F, self.nops, self.recipes, base=BASE, case=self, **self.prod_kw)
        self.stages = [(abi.STAGE_PROPOSALS, props), (abi.STAGE_PRODUCTS, prods)]
        self.n_slots = BASE + stride * self.nops
        self.outputs = [BASE + stride * i + self.F for i in range(self.nops)]
        self.proposals = [BASE + stride * i + j for i in range(self.nops) for j in range(self.F)]
        self.rounds = 1

    def operands(self):
        """slot -> (points, bandwidth): drawn once per case from its seed"""
        rng = np.random.default_rng(self.seed)
        src = {}
        for slot, (centre, spread) in enumerate([(0.0, 0.4), (2.0, 0.4), (1.0, 0.6), (1.0, 0.5), (1.2, 0.7), (0.0, 1.0)]):
            pts = rand_points(rng, MAN, self.N, centre, spread)
            src[slot] = (pts[:self.counts.get(slot, self.N)], np.array([0.15, 0.2]))
        return src

    def run(self, make, fused=True, lazy=None):
        """-> dict(nf, out, prop, side, diag): num_fused (None on the oracle), belief_read of every output slot, of every
        proposal slot, the side buffer, the counters"""
        hip = getattr(make, "is_hip", False)
        be = make(self.N, self.n_slots, self.side_ints)
        try:
            for slot, (pts, bw) in self.operands().items():
                be.belief_write(slot, MAN, pts, bw)
            be.side_write(0, np.zeros(self.side_ints))
            be.side_write(self.inj_off, np.arange(self.N) % 3 != 0)  # injected hypotheses: every third particle the null one
            stride = self.F + 1
            for i in range(self.nops):
                for j in self.preset_bw:
                    be.belief_write(BASE + stride * i + j, MAN, np.zeros((self.N, 2)), np.array([0.3, 0.25]))
            be.diag(reset=True)
            prog = be.program(self.stages, lazy_bandwidth=self.lazy if lazy is None else lazy, **({"fused_updates": fused} if hip else {}))
            nf = prog.num_fused() if hip else None
            prog.run()
            be.synchronize()
            res = dict(nf=nf, out=[be.belief_read(s, MAN) for s in self.outputs], prop=[be.belief_read(s, MAN) for s in self.proposals],
                       side=be.side_read(0, self.side_ints), diag=be.diag())
            prog.close()
            return res
        finally:
            be.close()


class LazyTwoRounds(Case):
    """a fused pair, then a second fused pair whose updates take the first pair's outputs as their targets and overwrite
    them: under lazy_bandwidth nothing reads the bandwidth of the first outputs, so their fit is skipped (NBP_UPD_FIT_OUT
    clear; with F = 1 the proposal's fit goes with it)"""

    def _build(self):
        F, stride = self.F, 2 * self.F + 1
        p1, q1, _ = build_round(self.N, F, self.nops, self.recipes, base=BASE, stride=stride, out_off=F, case=self)
        p2, q2, _ = build_round(self.N, F, self.nops, self.recipes, base=BASE, stride=stride, prop_off=F + 1, out_off=F,
                                target=lambda i: BASE + stride * i + F, seed0=30000, pseed0=40000, case=self)
        self.stages = [(abi.STAGE_PROPOSALS, p1), (abi.STAGE_PRODUCTS, q1), (abi.STAGE_PROPOSALS, p2), (abi.STAGE_PRODUCTS, q2)]
        self.n_slots = BASE + stride * self.nops
        self.outputs = [BASE + stride * i + F for i in range(self.nops)]
        self.proposals = [BASE + stride * i + k for i in range(self.nops) for k in list(range(F)) + list(range(F + 1, 2 * F + 1))]
        self.rounds = 2
        self.lazy = True


class CopiesBehind(Case):
    """F = 4 and a STAGE_COPIES behind the round that reads inputs 0, 2 and 3 of three different updates, the last update
    of the launch among them; a second STAGE_COPIES then overwrites every proposal slot with the target's belief, so that
    nothing but those three reads asks for a proposal in its slot: three write-back flags (2 << j) set and 61 clear in one
    launch.  The copies are the outputs read back; the proposal slots read back hold the target's belief."""
    READS = ((3, 0), (9, 2), (-1, 3))

    def _build(self):
        Case._build(self)
        stride, extra = self.F + 1, self.n_slots
        copies = [abi.CopyDesc(BASE + stride * (i % self.nops) + j, extra + k) for k, (i, j) in enumerate(self.READS)]
        self.stages.append((abi.STAGE_COPIES, copies))
        self.stages.append((abi.STAGE_COPIES, [abi.CopyDesc(T, s) for s in self.proposals]))
        self.outputs = self.outputs + [extra + k for k in range(len(copies))]
        self.n_slots = extra + len(copies)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
SIZES = (8, 37, 64, 65, 128, 129, 200, 256)   # the minimum, each Npad in {64, 128, 192, 256} with and without idle lanes, the ceiling
SIZES_REFUSED = (257, 512)                    # Npad > 256
SIZE_F = (1, 2, 4)
CLASS_N = (65, 200)
BELOW = (1, 2, 63, 150)                       # points an operand holds in a context of N = 200

def size_case(N, F):
    return Case(N, F, ["prior" if (j == F - 1 and F > 1) else "rel" for j in range(F)], name=f"size-{N}-{F}")


# feature -> the recipes of inputs 0 .. 2 (F = 2 takes the first two); every one keeps the round fused
ACCEPTED = {
    "msgprior": ["msg", "rel", "prior"],
    "prior_nullhypo": ["prior_nh", "rel", "rel"],
    "prior_injected_hypotheses": ["prior_nh_inj", "rel", "rel"],
    "relative_nullhypo": ["rel_nh", "rel", "prior"],
    "mixture_prior": ["prior_mix", "rel", "rel"],
    "mixture_relative": ["rel_mix", "rel", "prior"],
    "multihypo_relative": ["rel_mh", "rel", "prior"],
    "passthrough_among_several": ["pass", "rel", "prior"],
    "stored_measurement": ["rel_stored", "prior_stored", "rel"],
    "measurement_kde": ["rel_kde", "rel", "prior"],
    "sfidx0_and_sfidx1": ["rel_sf0", "rel", "prior"],
}
# F = 1: the early return of the kernel (product_passthrough) -- recipe, points the pass-through's density holds (None: N)
ACCEPTED_F1 = {
    "skip_bandwidth": ("rel_skipbw", None),       # (its slot holds a bandwidth beforehand: the one the update hands on)
    "msgprior": ("msg", None),
    "prior_nullhypo": ("prior_nh", None),
    "mixture_relative": ("rel_mix", None),
    "lone_passthrough": ("pass", None),
    "lone_passthrough_resampled": ("pass", 50),
}
# feature -> (F, recipes, case keywords): the planner keeps the three-launch form
REFUSED = {
    "partial_relative": (2, ["rel_partial", "prior"], {}),                            # (the class exit alone)
    "partial_relative_and_input": (2, ["rel_partial", "prior"], dict(partials=[1, 0], old_slot=T)),
    "old_slot": (2, ["rel", "prior"], dict(partials=[0, 0], old_slot=T)),
    "labels_out": (2, ["rel", "prior"], dict(labels_out=True)),
    "lone_passthrough_keep_count": (1, ["pass_keep"], dict(counts={DEN: 50})),
    "lone_passthrough_topped_up": (1, ["pass_init"], dict(counts={DEN: 50})),   # (keep_count = 2: N points, refused all the same)
    "skip_bandwidth_into_product": (2, ["rel_skipbw", "prior"], dict(preset_bw=(0,))),
}


def accepted_case(feature, N, F):
    return Case(N, F, ACCEPTED[feature][:F], name=f"{feature}-{N}-{F}")


def accepted_f1_case(feature, N):
    recipe, cnt = ACCEPTED_F1[feature]
    return Case(N, 1, [recipe], counts={} if cnt is None else {DEN: cnt}, preset_bw=(0,) if recipe == "rel_skipbw" else (),
                name=f"{feature}-{N}-1")


def refused_case(feature, N):
    F, recipes, kw = REFUSED[feature]
    c = Case(N, F, recipes, name=f"refused-{feature}-{N}", **kw)
    if feature == "old_slot":  # (product_desc names an old_slot beside partial inputs only)
        for d in c.stages[1][1]:
            d.old_slot = T
    if feature == "lone_passthrough_keep_count":
        c.out_count = kw["counts"][DEN]  # the density's own count
    return c


def below_case(cnt):
    """N = 200; the relative's other variable and the MsgPrior's KDE hold `cnt` points (`anyn_index`, the KDE draw)"""
    return Case(200, 2, ["rel", "msg"], counts={A: cnt, KDE: cnt}, name=f"below-{cnt}")


def lazy_case(F):
    return LazyTwoRounds(200, F, ["rel", "prior", "rel"][:F], name=f"lazy-{F}")


def copies_case():
    return CopiesBehind(200, 4, ["rel", "rel", "msg", "prior"], name="copies")


def all_cases():
    """every case of this module, by name (the CPU leg runs each on the oracle)"""
    cs = [size_case(N, F) for N in SIZES + SIZES_REFUSED for F in SIZE_F]
    cs += [accepted_case(f, N, F) for f in ACCEPTED for N in CLASS_N for F in (2, 3)]
    cs += [accepted_f1_case(f, N) for f in ACCEPTED_F1 for N in CLASS_N]
    cs += [refused_case(f, N) for f in REFUSED for N in CLASS_N]
    cs += [below_case(c) for c in BELOW]
    cs += [lazy_case(1), lazy_case(2), copies_case()]
    return cs


def chain_graph():
    """the whole-solve case: a 48-variable Euclid(2) chain at N = 100, whose nested-dissection tree has rounds of >= 16 updates"""
    fg = iif.generateChainEuclid(48, vardims=2, priorEvery=12, N=100)
    return fg, iif.nestedDissectionOrder(fg)
