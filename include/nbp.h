/*
 * nbp.h -- C ABI of libnbp: the MI355X-native replacement for the per-clique
 * nonparametric Chapman-Kolmogorov hot path of IncrementalInference.jl (IIF).
 *
 * The reference has NO FFI for this path: it is extended by Julia multiple
 * dispatch.  This header therefore *defines* the boundary a Julia `ccall` shim binds to
 * (INTEGRATION.md shows the shim).  Every entry point cites the reference function it replaces
 * (paths relative to the IncrementalInference.jl source tree, v0.35.6).
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / C++ types.
 *  - all floating point is IEEE double (reference: Float64 everywhere).
 *  - the caller owns every host buffer; the library never keeps a host pointer past return.
 *  - return value: 0 = NBP_OK, <0 = hard error (the Julia shim turns it into `error()` so the
 *    clique Task fails and `monitorCSMs` propagates ERROR_STATUS, CliqStateMachineUtils.jl:184-246).
 *  - soft conditions are counted, not raised: non-converged per-particle solves are used anyway
 *    (NumericalCalculations.jl:128-131), NaN solves leave the particle unchanged (:348-351).
 *
 * Host point layout ("P doubles per point", packed AoS, exactly what Julia holds):
 *    NBP_EUCLID1/2/3 : P = D, SVector{D,Float64}                (Variables/DefaultVariables.jl:9-19)
 *    NBP_CIRCULAR    : P = 1, angle in [-pi,pi) (shim packs Vector{Vector{Float64}}, :52)
 *    NBP_SE2         : P = 6, ArrayPartition(t[2], R[2x2] column-major) = x,y,R11,R21,R12,R22
 *                      (test/testSpecialEuclidean2Mani.jl:14)
 * Device layout ("slot"): tangent coordinates at the identity, SoA: coord d of particle n at
 *    slot_base + d*N + n, d < D (SE2 is stored as x,y,theta), then bw[3], infoPerCoord[3], see DESIGN.md:
 *    a slot is the device form of a TreeBelief (val, bw, infoPerCoord; entities/BeliefTypes.jl:47-57).
 */
#ifndef NBP_H
#define NBP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBP_MAXV 6   /* variables attached to one factor (multihypo door sighting uses 5) */
#define NBP_MAXF 128 /* densities multiplied in one manifoldProduct (a landmark with many sightings);
                        products whose node statistics do not fit the 160 KB LDS keep them in HBM/L2 */
#define NBP_MAXD 3   /* tangent dimension                                                   */
#define NBP_MAXC 4   /* Mixture components                                                  */
#define NBP_MAXK 8   /* groups (modes) per belief in nbp_run_factor_mode_likelihood          */
#define NBP_MAXN 512 /* particles per belief                                                */
#define NBP_COMP_STRIDE 13 /* per component: weight, mean[3], sqrt-cov L[3][3] row-major    */
/* Family of a SCALAR measurement component, carried in its last slot (comp[c][12] = L[2][2], which a one-dimensional
 * measurement does not use; read only when the measurement has one dimension).  Multi-dimensional measurements are
 * Gaussian (MvNormal).  `rand(Z)` of the reference's Distributions.jl objects (sampleFactor, CalcFactor.jl). */
enum nbp_dist {
  NBP_DIST_GAUSSIAN = 0, /* z = mean[0] + L[0][0] * randn                                     */
  NBP_DIST_UNIFORM = 1,  /* Uniform(a, b): mean[0] = a, L[0][0] = b - a; z = a + (b - a) u   */
  NBP_DIST_RAYLEIGH = 2, /* Rayleigh(sigma): L[0][0] = sigma; z = sigma sqrt(-2 log u), u in (0, 1] */
  NBP_DIST_TABLE = 3     /* AliasingScalarSampler(domain, weights) (entities/AliasScalarSampling.jl:13-74): z = domain[i],
                            i ~ Categorical(weights) -- StatsBase.alias_sample! draws from that categorical, here by inverse
                            CDF on one uniform.  The table lives in a slot: row 0 = the domain, row 1 = the CUMULATIVE
                            normalised weights, count = its length (<= N); written like a belief on NBP_EUCLID2
                            (nbp_belief_write; clique calls: factor_density[f]).  nbp_proposal_desc.var_slot[NBP_MAXV - 1]
                            names the slot (factors with a table have at most NBP_MAXV - 1 variables); one table per factor.
                            A slot has N rows: a table with MORE than N entries does not fit -- nbp_clique_* refuse it
                            (NBP_ERR_RANGE) and the hosts (Python `table_belief(N)`, ext/IIFNbpExt.jl `supported(fct, N)`)
                            refuse it before writing; nbp_belief_write itself cannot tell a table from a belief and keeps
                            the first N rows of whatever it is given */
};

typedef int32_t nbp_status;
#define NBP_OK 0
#define NBP_ERR_ARG (-1)
#define NBP_ERR_HIP (-2)
#define NBP_ERR_NOGPU (-3)
#define NBP_ERR_RANGE (-4)

/* getManifold(variableType): Position{N} -> TranslationGroup(N), Circular -> RealCircleGroup,
 * SE(2) -> SpecialEuclidean(2; vectors=HybridTangentRepresentation()) */
enum nbp_manifold {
  NBP_EUCLID1 = 1,
  NBP_EUCLID2 = 2,
  NBP_EUCLID3 = 3,
  NBP_CIRCULAR = 4,
  NBP_SE2 = 5
};

/* the closed set of residual functors */
enum nbp_factor {
  NBP_F_PRIOR = 1,      /* Prior / PriorCircular / ManifoldPrior: point = wrap(mean + L n)
                           Factors/DefaultPrior.jl:17, Circular.jl:56-60, GenericFunctions.jl:181-214 */
  NBP_F_MSGPRIOR = 2,   /* MsgPrior{ManifoldKernelDensity}: draw from the KDE held in var_slot[1]
                           Factors/MsgPrior.jl:27-30, services/TreeMessageUtils.jl:86-89 */
  NBP_F_LINREL = 3,     /* LinearRelative{D}: r = z - (x2 - x1)       Factors/LinearRelative.jl:42-49 */
  NBP_F_CIRCULAR = 4,   /* CircularCircular                            Factors/Circular.jl:24-28       */
  NBP_F_SE2 = 5,        /* ManifoldFactor(SpecialEuclidean(2))         Factors/GenericFunctions.jl:39-44,98-100 */
  NBP_F_EUCLIDDIST = 6, /* EuclidDistance: r = z - ||x2 - x1||         Factors/EuclidDistance.jl:20    */
  NBP_F_PASSTHROUGH = 7 /* PartialPriorPassThrough(Z, partial): the proposal IS the density Z.heatmap.densityFnc, placed on
                           the coordinates of `.partial` (calcProposalBelief dispatch, ApproxConv.jl:196-227;
                           Factors/PartialPriorPassThrough.jl).  var_slot[1] = slot holding that density (points in the
                           variable's coordinates -- only the partial ones are read --, bandwidth, count); nothing is
                           sampled, solved or fitted, and no hypothesis machinery applies (evalFactor is bypassed) */
};

/*
 * One proposal = one `approxConvBelief(dfg, fct, target)` (services/ApproxConv.jl:4-45):
 * evalFactor -> evalPotentialSpecific (services/EvalFactor.jl:321-395 relative, :400-542 prior)
 * followed by manikde! (bandwidth fit).  Carries exactly the knobs the reference reads from
 * SolverParams / the factor (entities/SolverParams.jl:12-75, services/FactorGraph.jl:824-839).
 */
typedef struct nbp_proposal_desc {
  int32_t factor_kind;        /* enum nbp_factor                                              */
  int32_t manifold;           /* enum nbp_manifold of the solve-for variable                  */
  int32_t nvars;              /* variables attached to the factor (1 for priors)              */
  int32_t sfidx;              /* 0-based index of the solve-for variable in var_slot          */
  int32_t var_slot[NBP_MAXV]; /* belief slot of every attached variable (getVariableOrder);
                                 NBP_F_MSGPRIOR: var_slot[1] = slot holding the message KDE   */
  int32_t out_slot;           /* scratch slot that receives the proposal (never the belief itself:
                                 services/CalcFactor.jl:543-548)                              */
  int32_t ncomp;              /* 1, or the number of Mixture components (Factors/Mixture.jl)  */
  int32_t has_multihypo;      /* 0: hypotheses === nothing; else bit 0 set.  Optional isinit flags of the
                                 attached variables (ExplicitDiscreteMarginalizations.jl:161-172): bit 7 =
                                 flags present, bit 8+k = variable k is initialised                */
  int32_t inflate_cycles;     /* SolverParams.inflateCycles (default 3)                       */
  int32_t mhidx_in;           /* >=0: offset into the ctx int32 side buffer holding an injected
                                 mhidx[N] (exact-match tests); -1: sample internally           */
  int32_t mhidx_out;          /* >=0: offset in the side buffer where the used mhidx[N] is stored */
  int32_t skip_bandwidth;     /* 1: do not fit the bandwidth (caller discards it)              */
  int32_t partial_mask;       /* 0: full factor.  Otherwise bit k set = tangent coordinate k is in the
                                 factor's `.partial` tuple (ccw.partialDims, CalcFactor.jl:369-486):
                                 the measurement has popcount(mask) dimensions; a partial prior sets
                                 only those coordinates (setPointPartial!, EvalFactor.jl:457-538), a
                                 partial relative factor solves and inflates only them (:184-198);
                                 all other coordinates keep the target's current values          */
  int32_t meas_kde;           /* 0: the measurement model is `comp`.  k+1: the measurement is a kernel density
                                 estimate held in slot k (points + bandwidth), sampled as random kernel +
                                 bw*randn: the "differential" relative factors LinearRelative(::MKD) /
                                 CircularCircular(::MKD) of the useMsgLikelihoods upward messages
                                 (TreeMessageUtils.jl:279-335, Factors/LinearRelative.jl:32,
                                 manifolds/services/ManifoldSampling.jl:13-19); relative factors only */
  int32_t keep_count;         /* NBP_F_PASSTHROUGH only.  1: the proposal keeps the density's own particle count (the
                                 density is the only factor of the update: "PassThrough transfers the full point count
                                 to the graph, unless a product is calculated", test/testSpecialEuclidean2Mani.jl:394);
                                 0: it is resampled (multinomially, no kernel noise: the bandwidth stays) to the N
                                 points a product needs from every input;
                                 2: graph initialisation of a variable from this density alone: "the graph should stay
                                 restricted to N" (resample(bel, N), GraphInit.jl:174-177) -- the density's points
                                 stay, the rest up to N are draws from its KDE (random kernel + bw * randn) */
  double multihypo[NBP_MAXV]; /* parsed Categorical p: certain variables carry 0.0
                                 (services/FactorGraph.jl:639-651)                            */
  double nullhypo;            /* max(ccw.nullhypo, nullSurplus)   EvalFactor.jl:352            */
  double inflation;           /* ccw.inflation (default SolverParams.inflation = 5.0)          */
  double spread_nh;           /* SolverParams.spreadNH (3.0)                                   */
  double comp[NBP_MAXC][NBP_COMP_STRIDE]; /* measurement model, see NBP_COMP_STRIDE            */
  uint64_t seed;              /* Philox key of this op (counter-based RNG)          */
  uint64_t meas_seed;         /* 0: fresh measurements, drawn from `seed`.  Otherwise the measurement samples
                                 (and Mixture labels / KDE draws) are those of the op with this seed: the
                                 stored ccw.measurement reused when needFreshMeasurements = false, i.e. Gibbs
                                 iterations > 1 with SolverParams.alwaysFreshMeasurements = false
                                 (SolveTree.jl:119, services/CalcFactor.jl:492-510)            */
} nbp_proposal_desc;

/*
 * One product = the `AMP.manifoldProduct(dens, M; Niter=1, N)` call of propagateBelief
 * (services/GraphProductOperations.jl:53-60) plus the bandwidth fit of the result and the
 * `setBelief!` write-back (services/SolveTree.jl:74, services/FactorGraph.jl:250-263).
 */
typedef struct nbp_product_desc {
  int32_t manifold;
  int32_t nfactors;            /* 1 = pass-through (AMP returns the single density)            */
  int32_t niter;               /* Gibbs sweeps per tree level, 1 .. 8 (reference passes Niter=1) */
  int32_t out_slot;            /* belief slot that receives points + bandwidth                 */
  int32_t in_slot[NBP_MAXF];   /* proposal slots                                               */
  int32_t labels_out;          /* >=0: offset in the int32 side buffer for labels[N][nfactors] */
  int32_t old_slot;            /* oldPoints (GraphProductOperations.jl:39-45): coordinates that no input
                                  density informs are copied from this slot; -1 when every input is full */
  uint8_t in_partial[NBP_MAXF]; /* per input density: 0 = full, else the coordinate bit mask of a partial
                                  density (AMP.marginal(propBel, pardims), ApproxConv.jl:287-291): it
                                  multiplies into the product on those coordinates only              */
  uint64_t seed;
} nbp_product_desc;

/* belief copy: tree message traffic (TreeBelief val+bw, entities/BeliefTypes.jl:47-57) */
typedef struct nbp_copy_desc {
  int32_t src_slot;
  int32_t dst_slot;
} nbp_copy_desc;

typedef struct nbp_diag {
  int64_t solves;        /* per-particle optimiser runs                        */
  int64_t nonconverged;  /* NumericalCalculations.jl:128-131                   */
  int64_t nan_results;   /* NumericalCalculations.jl:348-351                   */
  int64_t residual_evals;
  int64_t lcv_evals;     /* leave-one-out likelihood evaluations in double precision (each = N(N-1)/2 kernel pairs) */
  int64_t lcv_evals_f32; /* bracketing evaluations of the bandwidth searches in single precision (each = N(N-1) ordered
                            pairs): they decide comparisons whose two sides are further apart than their error bounds;
                            the bandwidth selected is that of the all-double search, bit for bit (NBP_FIT_F64=1 in the
                            environment of nbp_ctx_create: every evaluation in double precision)                        */
  /* proposal launches by geometry, counted on the host where the launch is issued (a captured program counts at capture,
     not at replay): the workgroup kernels, one wave per proposal, two waves per proposal */
  int64_t proposal_launches_workgroup;
  int64_t proposal_launches_wave;
  int64_t proposal_launches_split;
  /* program lanes (nbp_program_set_lanes), counted on the host the same way: launches issued on lane 1, waits of one lane
     for the other, variable updates (product descriptors) that ran on lane 1 */
  int64_t lane_side_launches;
  int64_t lane_waits;
  int64_t lane_side_updates;
  /* sinks (NBP_OPT_UP_PASS_SINKS): variable updates (product descriptors) that ran in a later stage than their own, and the
     launches of the parts they ran in */
  int64_t sunk_updates;
  int64_t sink_launches;
} nbp_diag;

typedef struct nbp_ctx nbp_ctx;

/* ---- context ---------------------------------------------------------------------------- */
/* `arena` may be NULL (library allocates with hipMalloc) or a device pointer owned by the caller
 * (e.g. a torch tensor, so torch.distributed/RCCL can exchange slots); arena_bytes must be at
 * least nbp_arena_bytes(N, n_slots).  `side_ints` = size of the int32 side buffer (mhidx, labels). */
int64_t nbp_arena_bytes(int32_t N, int32_t n_slots);
int64_t nbp_slot_stride_doubles(int32_t N);
nbp_status nbp_ctx_create(int32_t device, int32_t N, int32_t n_slots, void *arena,
                          int64_t arena_bytes, int32_t side_ints, nbp_ctx **out);
nbp_status nbp_ctx_destroy(nbp_ctx *ctx);
/* One object of the layer above rides with the context (the native host's plan cache): `destroy(obj)` is called at the top of
 * nbp_ctx_destroy, while the context and its programs are still whole, or when another object takes its place. */
nbp_status nbp_ctx_attach(nbp_ctx *ctx, void *obj, void (*destroy)(void *obj));
void *nbp_ctx_attached(const nbp_ctx *ctx);
const char *nbp_last_error(void);
nbp_status nbp_synchronize(nbp_ctx *ctx);
void *nbp_arena_ptr(nbp_ctx *ctx);
void *nbp_stream_ptr(nbp_ctx *ctx); /* hipStream_t the library launches on */
int32_t nbp_ctx_particles(const nbp_ctx *ctx); /* N the context was created for (0: null) */
int32_t nbp_ctx_slots(const nbp_ctx *ctx);     /* belief slots of its arena (0: null) */
int32_t nbp_ctx_device(const nbp_ctx *ctx);    /* the HIP device it was created on (-1: null) */
/* Resident slots: the LAST n slots of the arena are set aside for beliefs that STAY on the device between clique calls --
 * the deep-copied sub graph of a clique between its up and its down solve, the up message a parent reads from its child
 * (a LikelihoodMessage that never visits the host: nbp_tree_belief.handle, nbp_host.h).  Handle h (1 .. n) names slot
 * nbp_ctx_slots - h; the clique calls plan their own slots below the resident ones. */
nbp_status nbp_ctx_reserve_resident(nbp_ctx *ctx, int32_t n);
int32_t nbp_ctx_resident(const nbp_ctx *ctx);

/* ---- belief I/O: setValKDE!/getVal at the boundary (FactorGraph.jl:250-297) ---------------
 * A slot is read and written BY MANIFOLD: the rows of the manifold's D coordinates (and bw / infoPerCoord entries 0 .. D-1)
 * are the belief; rows beyond D are unspecified -- a write from the host zeroes them, a kernel that produces a belief
 * leaves them as they were (a third of a Euclid(2) proposal's write traffic), and nothing in the library reads them (fits,
 * KD builds, products, proposals and the reads below all go by the manifold; whole-slot copies carry them along unread).
 * Read a slot with the manifold of the belief that was put there. */
nbp_status nbp_slot_write(nbp_ctx *ctx, int32_t slot, int32_t manifold, const double *pts_NxP,
                          const double *bw_D /* nullable */);
nbp_status nbp_slot_read(nbp_ctx *ctx, int32_t slot, int32_t manifold, double *pts_NxP,
                         double *bw_D /* nullable */);
/* The full TreeBelief / VariableNodeData triple (val, bw, infoPerCoord; BeliefTypes.jl:47-57, FactorGraph.jl:250-263).
 * infoPerCoord is produced on the device like the reference produces it: a proposal carries ones(D), zeroed outside
 * the factor's `.partial` (EvalFactor.jl:383-391); a variable update carries the sum over its factors of ones(D)
 * (proposalbeliefs!, ApproxConv.jl:277,298-303 -- the reference's `fct_ipc = ones(vardim)`, partial factors
 * included); slot copies (tree messages) carry it along.  nbp_slot_write stores zeros (a fresh VariableNodeData).
 * n_pts: particle count of the belief.  A slot holds up to N points (N of the context).  Fewer: the belief keeps its
 * own count (it must come with its bandwidth) and every consumer does what the reference does with a belief shorter
 * than N -- a convolution reads a random element for the particles beyond its end (_getindex_anyn,
 * NumericalCalculations.jl:377-381), the scratch copy of a target is filled up with the point default
 * (CalcFactor.jl:555-565), a MsgPrior / KDE measurement samples among the points it has, the oldPoints of a product are
 * topped up with sample(oldBel, N - Npts) (GraphProductOperations.jl:39-45), manikde! fits the points there are; every
 * kernel output holds N points.  More than N: the first N are kept (`_pts[1:N]`, GraphProductOperations.jl:44).
 * nbp_belief_read returns the count in *n_pts and fills the first *n_pts points (at most N rows: size `pts` for the N of the
 * context unless the count is known); with n_pts = NULL (nbp_slot_read) all N rows of the slot are written. */
nbp_status nbp_belief_write(nbp_ctx *ctx, int32_t slot, int32_t manifold, const double *pts_NxP, int32_t n_pts,
                            const double *bw_D /* nullable */, const double *ipc_D /* nullable: zeros */);
nbp_status nbp_belief_read(nbp_ctx *ctx, int32_t slot, int32_t manifold, double *pts_NxP, int32_t *n_pts /* nullable */,
                           double *bw_D /* nullable */, double *ipc_D /* nullable */);
/* Many beliefs in one call: packed into a pinned staging buffer and moved with one asynchronous copy per run of consecutive
 * slots on the library's stream (a clique call moves all its beliefs in one or two copies; a caller loading a whole graph
 * moves it in one).  Arrays of n entries; n_pts / bw / ipc may be NULL as a whole (N points, no bandwidth, infoPerCoord 0)
 * or per entry (bw, ipc).  _write_batch returns once the copies are queued: they are ordered before whatever is launched
 * next.  _read_batch returns the rows each belief holds in n_pts[i] (pts[i] sized for N rows), like nbp_belief_read. */
nbp_status nbp_belief_write_batch(nbp_ctx *ctx, int32_t n, const int32_t *slots, const int32_t *manifolds, const double *const *pts,
                                  const int32_t *n_pts, const double *const *bw, const double *const *ipc);
nbp_status nbp_belief_read_batch(nbp_ctx *ctx, int32_t n, const int32_t *slots, const int32_t *manifolds, double *const *pts,
                                 int32_t *n_pts, double *const *bw, double *const *ipc);
/* The same transfers without a host synchronisation (the asynchronous clique seam, nbp_clique_submit_batch): staged in
 * pinned buffers of a pool of the context, queued on the library stream behind whatever runs there.  _write_batch_async
 * returns once the copies are queued (the caller's buffers are free again: they were packed).  _read_batch_begin queues the
 * copies out and returns a token; _read_batch_end waits for them (an event, not the whole stream), unpacks into the caller's
 * buffers (entries with pts[i] == NULL are skipped) and consumes the token. */
typedef struct nbp_read_token nbp_read_token;
nbp_status nbp_belief_write_batch_async(nbp_ctx *ctx, int32_t n, const int32_t *slots, const int32_t *manifolds, const double *const *pts,
                                        const int32_t *n_pts, const double *const *bw, const double *const *ipc);
nbp_status nbp_belief_read_batch_begin(nbp_ctx *ctx, int32_t n, const int32_t *slots, nbp_read_token **out);
nbp_status nbp_belief_read_batch_end(nbp_read_token *token, const int32_t *manifolds, double *const *pts, int32_t *n_pts,
                                     double *const *bw, double *const *ipc);
/* sample(oldBel, N - Npts) in place: beliefs with fewer than N points are topped up to N with draws from their own KDE
 * (random kernel + bw * randn); the points they hold stay.  Multinomial resampling of a belief to the solver's N. */
nbp_status nbp_run_resample(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n, uint64_t seed);
nbp_status nbp_side_write(nbp_ctx *ctx, int32_t offset, const int32_t *src, int32_t n);
nbp_status nbp_side_read(nbp_ctx *ctx, int32_t offset, int32_t *dst, int32_t n);

/* ---- factor seam: approxConvOnElements!/evalFactor + manikde! (EvalFactor.jl:14-27,571-603) */
nbp_status nbp_run_proposals(nbp_ctx *ctx, const nbp_proposal_desc *descs, int32_t n);
/* ---- AMP.manikde!(M, pts) bandwidth selection for slots already resident ------------------ */
nbp_status nbp_run_bandwidth(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n);
/* calcPPE (FGOSUtils.jl:237-275) for beliefs resident in slots: manifold mean and the KDE's maximum among the belief's
 * own points.  Queued on the library stream behind whatever runs there; one copy back; synchronises.
 * mean = mean(M, pts, GeodesicInterpolation()) per coordinate over the points the belief holds; max = the point i (max_index, the
 * lowest among equals) with the greatest p_i = sum_j exp(-1/2 sum_d (delta_d(i, j) / bw_d)^2), delta wrapped on circular
 * coordinates (not KernelDensityEstimate.jl's getKDEMax: DESIGN.md 8).  Tangent coordinates (SE(2): x, y, theta),
 * entries beyond the manifold's dimension zero.  A bandwidth entry that is not positive and finite: max = NaN, max_index = -1. */
nbp_status nbp_run_ppe(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n,
                       double *mean_out /* n x NBP_MAXD */, double *max_out /* n x NBP_MAXD */,
                       int32_t *max_index_out /* n, nullable */);
/* host-buffer form, like nbp_kde_bandwidth: stages through slot 0 */
nbp_status nbp_kde_ppe(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, const double *bw_D,
                       double *mean_out_D, double *max_out_D, int32_t *max_index_out /* nullable */);
/* ---- belief queries (both DEFINED by this library, unpinned against the Julia packages: DESIGN.md 8) ----------
 * Density of resident beliefs at query points, the reference's getBelief(fg, :x)(pts): belief i is evaluated at the queries
 * q_first[i] .. q_first[i+1]-1 (tangent coordinates, NBP_MAXD doubles each; SE(2): x, y, theta; entries beyond the manifold's
 * dimension are not read).  p(q) = 1 / (c prod_d sqrt(2 pi) bw_d) sum_{j<c} exp(-1/2 sum_d (delta_d(q, x_j) / bw_d)^2), delta
 * wrapped to [-pi, pi) on circular coordinates (there the mass a kernel has beyond +-pi is lost), j = 0 .. c-1 in that order in
 * one lane: a value does not depend on the queries that travel with it.  All coordinates of the manifold enter.  A bandwidth entry
 * that is not positive and finite: every density of that belief is NaN.  Queued on the library stream; one copy each way;
 * synchronises. */
nbp_status nbp_run_evaluate(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n,
                            const int32_t *q_first /* n+1, ascending, q_first[0]=0 */,
                            const double *queries /* q_first[n] x NBP_MAXD */, double *dens_out /* q_first[n] */);
/* host-buffer form: stages through slot 0 */
nbp_status nbp_kde_evaluate(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, const double *bw_D,
                            const double *queries /* nq x NBP_MAXD */, int32_t nq, double *dens_out);
/* ---- marginal densities ("Marginal densities"; DEFINED by this library, unpinned: DESIGN.md 8) -----------------------
 * For a coordinate set K of the manifold (at least one coordinate; 0-based here, where the reference's `partial` is 1-based):
 * p_K(q) = 1 / (c prod_{d in K} sqrt(2 pi) bw_d) sum_{j<c} exp(-1/2 sum_{d in K} (delta_d(q, x_j) / bw_d)^2), the density above with
 * the coordinates outside K dropped.  Only the bandwidth entries in K must be positive and finite (else every value is NaN); the
 * others are not read, so the belief a lone partial factor leaves (bandwidth h0, h1, 0 on SE(2)) has a marginal on (0, 1).
 *
 * A grid descriptor asks for p_K of one resident belief on a regular grid: |K| = 1 (dims[1] = -1) or 2, n[a] points on axis a
 * (1 .. NBP_GRID_MAX), point k of axis a at lo[a] + (double)k * step[a].  The output is row-major with the FIRST listed coordinate
 * slowest; dims = {b, a} is the transpose of dims = {a, b} bit for bit.  The value is (sum_j E_0[k0][j] E_1[k1][j]) / norm with
 * E_a[k][j] = exp(-1/2 (delta(g_a[k], x_j) / bw_a)^2), j = 0 .. c-1 in that order in one lane: it depends on the belief and its grid
 * point alone.  flags & NBP_GRID_AUTO_EXTENT: lo and step are not read; a Euclidean axis spans min_j x - margin bw .. max_j x +
 * margin bw (step = (hi - lo) / (n - 1), n >= 2), a circular axis lo = -pi, step = 2 pi / n (margin plays no part there).
 * Fields that a 1-D grid or an automatic extent does not use are not read. */
#define NBP_GRID_MAX 1024
#define NBP_GRID_AUTO_EXTENT 1
typedef struct nbp_grid_desc {
  int32_t slot;
  int32_t manifold;
  int32_t dims[2];
  int32_t n[2];
  int32_t flags;
  double lo[2];
  double step[2];
  double margin;
} nbp_grid_desc;
/* Grids of any number of resident beliefs (the same slot may appear in several descriptors) in one launch sequence with one copy
 * back (a second, of 32 bytes a descriptor, where extent_out is given): descriptor i fills out[first[i] .. first[i+1]-1], first[0] = 0 and first[i+1] - first[i] = the points of grid i.  extent_out
 * (nullable): the extent used, lo0, step0, lo1, step1 per descriptor (a 1-D grid: lo1 = step1 = 0).  NBP_ERR_RANGE, with the
 * descriptor's index in the message and before anything is launched, for: a slot or a coordinate outside the context / manifold, a
 * repeated coordinate, n outside 1 .. NBP_GRID_MAX, n < 2 on a Euclidean axis with automatic extent, a non-finite lo / step (explicit
 * extent) or margin (automatic extent), offsets that do not match the grid sizes.  Queued on the library stream; synchronises. */
nbp_status nbp_run_marginal_grid(nbp_ctx *ctx, const nbp_grid_desc *descs, int32_t n_desc, const int32_t *first /* n_desc+1 */,
                                 double *out /* first[n_desc] */, double *extent_out /* n_desc x 4, nullable */);
/* host-buffer form: stages through slot 0; desc->slot and desc->manifold are not read */
nbp_status nbp_kde_marginal_grid(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, const double *bw_D,
                                 const nbp_grid_desc *desc, double *out, double *extent_out_4 /* nullable */);
/* p_K at arbitrary query points: nbp_run_evaluate with one coordinate bit mask per belief (bit d = coordinate d; a non-empty subset
 * of the manifold's coordinates, else NBP_ERR_RANGE naming the belief).  Queries are NBP_MAXD doubles each; entries outside the
 * mask are not read.  With the full mask the values are those of nbp_run_evaluate bit for bit. */
nbp_status nbp_run_evaluate_marginal(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                                     const int32_t *q_first /* n+1, ascending, q_first[0]=0 */,
                                     const double *queries /* q_first[n] x NBP_MAXD */, double *dens_out /* q_first[n] */);
/* mmd(p1, p2, varType; bw = [sigma]) (SolverUtilities.jl:25-47) of pairs of resident beliefs a (n points), b (m points) on one
 * manifold: k(p, q) = exp(-sigma d(p, q)^2), d^2 = sum_d delta_d^2 in tangent coordinates (circular ones wrapped; the heading of
 * SE(2) with weight 1), S_xy = sum_i sum_j k(x_i, y_j), mmd = Saa/(n n) + Sbb/(m m) - 2 Sab/(n m), evaluated as written with one
 * summation order for the three sums: a belief against a bit-identical copy (or slots_a[i] == slots_b[i]) gives exactly 0.0.  No
 * clamp at zero; the beliefs' bandwidths play no part.  sigma: finite, >= 0 (the reference's default is 0.001). */
nbp_status nbp_run_mmd(nbp_ctx *ctx, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds, int32_t n,
                       double sigma, double *mmd_out /* n */);
/* host-buffer form: stages through slots 0 and 1 */
nbp_status nbp_kde_mmd(nbp_ctx *ctx, int32_t manifold, const double *a_NxP, int32_t na, const double *b_NxP, int32_t nb,
                       double sigma, double *mmd_out);
/* ---- belief statistics ("Belief statistics") ----------------------------------------------------------------------
 * calcMeanCovar (VariableStatistics.jl:39-44; Statistics.cov(vartype, pts), VariableStatistics.jl:12-19) for beliefs resident in
 * slots.  mean = the mean nbp_run_ppe delivers, bit for bit; cov[d][e] = 1/(c-1) sum_i delta[i][d] delta[i][e] with
 * delta[i][d] = x[i][d] - mean[d], wrapped to [-pi, pi) on circular coordinates; c = the count the slot holds.  Tangent coordinates
 * (SE(2): x, y, theta: deviations in the world frame about the mean -- DEFINED here, unpinned against Manifolds.jl: DESIGN.md 8).
 * cov is NBP_MAXD x NBP_MAXD per belief, row-major, symmetric bit for bit, rows and columns beyond the manifold's dimension zero;
 * c < 2: the D x D block is NaN, the mean stands.  The bandwidth plays no part.  Queued on the library stream behind whatever runs
 * there; one copy back; synchronises. */
nbp_status nbp_run_meancov(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n,
                           double *mean_out /* n x NBP_MAXD */, double *cov_out /* n x NBP_MAXD x NBP_MAXD */);
/* host-buffer form, like nbp_kde_ppe: stages through slot 0 */
nbp_status nbp_kde_meancov(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, double *mean_out_D,
                           double *cov_out_DxD);
/* kld(p, q) (attic/examples/FixedPointIllustrationsSquare.jl:53-62) of pairs of resident beliefs a (n points, bandwidth h_a) and
 * b (m points, h_b) on one manifold: kld = Eaa - Eab, Eaa = 1/n sum_i l_a(a_i) (the self term stays in), Eab = 1/n sum_i l_b(a_i),
 * l_p(x) = the logarithm of the density nbp_run_evaluate defines, formed as M + log(sum_j exp(e_j - M)) - log(m prod_d sqrt(2 pi) h_d)
 * with e_j = -1/2 sum_d (delta_d(x, y_j) / h_d)^2 and M = max_j e_j, so that it is finite where the density underflows.  One
 * function and one summation order behind both terms: a belief against a bit-identical copy (or slots_a[i] == slots_b[i]) gives
 * exactly 0.0.  No clamp at zero; entropy(a) = -Eaa.  A bandwidth entry of either belief that is not positive and finite: kld and
 * both terms are NaN.  DEFINED by this library, unpinned against KernelDensityEstimate.jl. */
nbp_status nbp_run_kld(nbp_ctx *ctx, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds, int32_t n,
                       double *kld_out /* n */, double *terms_out /* n x 2: Eaa, Eab; nullable */);
/* host-buffer form: stages through slots 0 and 1 */
nbp_status nbp_kde_kld(nbp_ctx *ctx, int32_t manifold, const double *a_NxP, int32_t na, const double *bw_a_D, const double *b_NxP,
                       int32_t nb, const double *bw_b_D, double *kld_out, double *terms_out_2 /* nullable */);
/* ---- belief overlaps ("Belief overlaps"; DEFINED by this library, unpinned: DESIGN.md 8) ---------------------------
 * How much two resident beliefs overlap: a (n points, bandwidth h_a, manifold M_a, coordinate mask K_a) and b (m, h_b, M_b, K_b).
 * A mask is a bit mask as in nbp_run_evaluate_marginal (bit d = coordinate d); its coordinates are taken in ascending order, and
 * position k of a goes with position k of b.  A pair is ADMISSIBLE when the two lists have the same length D_K and, position by
 * position, the same kind (Euclidean or circular): an SE(2) pose masked to x, y against a Euclid(2) landmark is.
 *   s_k = h_a,k^2 + h_b,k^2,  e_ij = -1/2 sum_k delta_k(a_i, b_j)^2 / s_k  (delta wrapped to [-pi, pi) on circular positions; formed
 *   as delta^2 times the rounded 1 / s_k, added in position order),  M = max_ij e_ij,
 *   L_ab = ((M + log sum_i sum_j exp(e_ij - M)) - log(n m)) - sum_k 1/2 log(2 pi s_k), a term below exp(-700) dropped: the logarithm of
 *   the integral of the product of the two marginal KDEs (exact on Euclidean coordinates; on circular ones the mass beyond +-pi is
 *   not wrapped back), finite where every density underflows.
 *   logc = L_ab - 1/2 (L_aa + L_bb),  c = exp(logc): 1 for equal beliefs, <= 1 on Euclidean coordinates (Cauchy-Schwarz; not
 *   guaranteed on circular ones).  One function and one summation order behind the three L: a belief against a bit-identical copy
 *   (or slots_a[i] == slots_b[i] with equal masks) gives logc == 0.0 exactly.  A bandwidth entry IN the mask of either belief that is
 *   not positive and finite (or an s_k that is not): the record is NaN.  Entries outside the mask are not read.
 * Refused before anything is launched, naming the pair -- NBP_ERR_RANGE: a slot out of range, an empty mask, a coordinate outside
 * the manifold; NBP_ERR_ARG: an unknown manifold, an inadmissible pair.  Queued on the library stream; one copy back; synchronises. */
typedef struct nbp_overlap_rec {
  double logc, lab, laa, lbb;
} nbp_overlap_rec;
nbp_status nbp_run_overlap(nbp_ctx *ctx, const int32_t *slots_a, const int32_t *slots_b, const int32_t *manifolds_a,
                           const int32_t *manifolds_b, const int32_t *masks_a, const int32_t *masks_b, int32_t n,
                           nbp_overlap_rec *recs_out /* n */);
/* host-buffer form: stages through slots 0 and 1 */
nbp_status nbp_kde_overlap(nbp_ctx *ctx, int32_t manifold_a, const double *a_NxP, int32_t na, const double *bw_a_D, int32_t mask_a,
                           int32_t manifold_b, const double *b_NxP, int32_t nb, const double *bw_b_D, int32_t mask_b,
                           nbp_overlap_rec *rec_out);
/* The search: for every row i of a list of n mutually admissible beliefs, the partners j != i ranked by logc.  Every belief has a
 * box [lo_k, hi_k], the exact minimum and maximum of its points on each masked position.  Pair (i, j) is SKIPPED iff on some
 * Euclidean position  gap = max(lo_i - hi_j, lo_j - hi_i) > 0  and  gap^2 > reach^2 (h_i^2 + h_j^2)  (as written, one rounding per
 * operation); circular positions never prune.  A skipped pair has logc <= log(sqrt(n m)) - reach^2 / 2, so the options are refused
 * (NBP_ERR_RANGE) unless  log(min_coeff) >= log(N) - reach^2 / 2 + 1, N the context's particle count: the result then equals brute
 * force over all pairs.  Every other pair is evaluated with a = the belief of the LOWER list index: the value nbp_run_overlap gives
 * for (a, b), bit for bit, and symmetric bit for bit.
 * Per row: idx_out / logc_out hold the topk partners with logc >= log(min_coeff), descending, ties to the lower list index, unused
 * entries -1 / -inf; found_out: ALL partners at or above the threshold; evaluated_out: the pairs not skipped.  A belief with an
 * unusable bandwidth (see above) has found -1, evaluated 0, an empty row, and is nobody's partner (nor counted as evaluated).
 * opts == NULL: the defaults below.  reach, min_coeff positive and finite, else NBP_ERR_ARG; topk outside 1 .. NBP_OVERLAP_MAXK and
 * options that break the rule above: NBP_ERR_RANGE.  List errors as the pair form's, naming the belief; a belief that is not
 * admissible against belief 0: NBP_ERR_ARG.  Two launches (per-belief preparation, then one workgroup per row); one copy back. */
#define NBP_OVERLAP_MAXK 16
#define NBP_OVERLAP_REACH 6.0
#define NBP_OVERLAP_MIN_COEFF 1e-3
#define NBP_OVERLAP_TOPK 8
typedef struct nbp_overlap_opts {
  double reach;
  double min_coeff;
  int32_t topk;
  int32_t pad;
} nbp_overlap_opts;
nbp_status nbp_run_overlap_search(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                                  const nbp_overlap_opts *opts /* nullable */, int32_t *idx_out /* n x topk */,
                                  double *logc_out /* n x topk */, int32_t *found_out /* n */, int32_t *evaluated_out /* n */);
/* ---- scene densities ("Scene densities"; DEFINED by this library, unpinned: DESIGN.md 8) ------------------------------
 * Every belief of a list on ONE regular grid: the picture of a whole solution.  Belief v: slots[v], manifolds[v], the one or two
 * 0-based coordinates dims[2 v], dims[2 v + 1] (-1: a 1-D scene), weight weights[v] (weights == NULL: all 1).  ADMISSIBLE: every
 * belief names as many coordinates as belief 0 and, axis by axis, the same kind (Euclidean or circular) -- an SE(2) pose on (x, y)
 * beside a Euclid(2) landmark is.  A belief is USABLE when its bandwidth entries on its coordinates are positive and finite; an
 * unusable one adds nothing and has skipped_out[v] = 1.
 *   box    per axis a, d = dims_v[a], h = bw_v[d], mn / mx the exact minimum / maximum of the belief's points on d:
 *          cull_lo = mn - reach h, cull_hi = mx + reach h, ext_lo = mn - margin h, ext_hi = mx + margin h (one rounding per operation)
 *   grid   point k of axis a = lo[a] + (double)k step[a]; row-major, axis 0 slowest; a 1-D scene has n[1] = 1.  flags &
 *          NBP_SCENE_AUTO_EXTENT: lo and step are not read; a Euclidean axis has lo = min ext_lo and hi = max ext_hi over the usable
 *          beliefs, step = (hi - lo) / (n - 1) (no usable belief: lo = step = 0); a circular axis lo = -pi, step = 2 pi / n.
 *   reach  belief v is IN REACH of a grid point when cull_lo <= g <= cull_hi on every Euclidean axis; circular axes never cull;
 *          reach = +inf: every belief is in reach of every point.
 *   value  S[k0][k1] = sum_v w_v (P_v / norm_v) over the usable beliefs in reach of the point, in list order, P_v and norm_v the sum
 *          and the normalisation of the marginal grid above: one belief with weight 1 and reach = +inf gives that grid bit for bit.
 *          A point no belief reaches is exactly 0.0.  A value depends on the list, the weights and its grid point alone.
 *   owner  (owner_out != NULL) the list index of the largest term w_v (P_v / norm_v) > 0 among the beliefs in reach of the point,
 *          ties to the lower index; -1 where there is none.
 *   bound  a belief out of reach of a point has every particle further than reach h from it on some axis: each term left out is
 *          below  w_v exp(-reach^2 / 2) / prod_a (sqrt(2 pi) h_a).
 * extent_out_4: lo0, step0, lo1, step1 as used (1-D: lo1 = step1 = 0).  tile_beliefs_out: the (tile, belief) pairs the tiles worked
 * on, out of tiles x V.  V = 0 is NBP_OK and leaves a grid of zeros (owners -1).  Refused before anything is launched or written,
 * naming the belief -- NBP_ERR_RANGE: a slot or coordinate outside the context or manifold, a repeated coordinate, n outside 1 ..
 * NBP_SCENE_MAX or n0 n1 > 2^22 (or n[1] != 1 in a 1-D scene), n < 2 on a Euclidean axis with the automatic extent, a non-finite lo, a
 * step that is not finite and positive (explicit extent); NBP_ERR_ARG: an unknown manifold or flag, a belief inadmissible against
 * belief 0, a weight that is negative or not finite, a margin that is not finite, a reach that is NaN or not positive, V < 0, a NULL
 * required pointer.  Queued on the library stream (per-belief preparation, the extent where automatic, one wave per tile); the grid
 * and the owners are copied straight into out / owner_out, the other outputs in one more copy; synchronises.  There is no host-buffer form: a scene has many beliefs, write them with nbp_belief_write_batch. */
#define NBP_SCENE_AUTO_EXTENT 1
#define NBP_SCENE_MAX 4096
#define NBP_SCENE_REACH 6.0
#define NBP_SCENE_MARGIN 4.0
typedef struct nbp_scene_desc {
  int32_t n[2];
  int32_t flags;
  int32_t pad;
  double lo[2];
  double step[2];
  double margin;
  double reach;
} nbp_scene_desc;
nbp_status nbp_run_scene_grid(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, const int32_t *dims /* V x 2 */,
                              const double *weights /* V, nullable */, int32_t V, const nbp_scene_desc *desc,
                              double *out /* n0 * n1 */, int32_t *owner_out /* nullable */, int32_t *skipped_out /* V, nullable */,
                              double *extent_out_4 /* nullable */, int64_t *tile_beliefs_out /* nullable */);
/* ---- credible regions ("Credible regions"; DEFINED by this library, unpinned: DESIGN.md 8) ---------------------------
 * How much of a resident belief lies where: the levels of its highest-density regions (HDR), the credibility of reference points and
 * the quantiles of its coordinates.  The belief has c points x_i (the count the slot holds), bandwidth h and manifold M; K is a
 * non-empty coordinate mask as in nbp_run_evaluate_marginal (bit d = coordinate d).  Only the bandwidth entries in K are read.
 *   l_i = M_i + log(sum_{j != i} exp(e_ij - M_i)) - log((c - 1) prod_{d in K} sqrt(2 pi) h_d), e_ij the exponent of
 *     nbp_run_evaluate_marginal on K, M_i = max_{j != i} e_ij: the LEAVE-ONE-OUT log density of each own point, j ascending in one
 *     lane, two passes.  Exclusion is by index: a duplicate of x_i stays in.  Finite where every term underflows.
 *   order = the particle indices by ascending (l_i, i): ties break by index.
 *   log_level[a], for the mass m_a in (0, 1]: k = ceil(m_a (double)c) clamped to 1 .. c; the k-th largest l_i, l at position c - k of
 *     the ascending order.  The region is {x : log p_K(x) >= log_level}; its contour on a marginal grid of the same coordinates lies at
 *     exp(log_level).  n_inside[a] = #{i : l_i >= log_level[a]} (>= k, more only through ties).  log_min / log_max: the least and
 *     the greatest l_i.
 *   a query q: logdens = the log density of the whole KDE at q on K (all c points, normalised by c: l_p(q) of nbp_run_kld with the
 *     mask); n_above = #{i : l_i > logdens}; mass = (double)n_above / (double)c, the mass of the smallest region that still contains
 *     q (0 at the densest place, 1 in the far tail); q lies inside the m_a-region iff logdens >= log_level[a].  Entries of a query
 *     outside K are not read.
 *   quant[d][p], for every coordinate d of the manifold whatever K and the probability prob[p] in [0, 1]: v_i = x_id (a circular
 *     coordinate: x_id - mean[d] wrapped to [-pi, pi)), sorted; t = (double)(c - 1) prob, lo = floor(t), hi = min(lo + 1, c - 1),
 *     Q = v_lo + (t - lo) (v_hi - v_lo) (Julia's and numpy's default, type 7), one rounding per operation; a circular coordinate
 *     delivers mean[d] + Q wrapped.  mean = the mean nbp_run_ppe delivers, bit for bit.  The bandwidth plays no part.
 *   c == 1: levels, l_i, log_min / log_max and masses are NaN, n_inside 0, n_above -1, order = {0}; a query's logdens stands; every
 *     quantile is the point.  A bandwidth entry in K that is not positive and finite: levels, l_i and query results are NaN, n_inside
 *     0, n_above -1, order -1; the quantiles are delivered all the same.
 * Unused entries of a record are zero.  Refused with NBP_ERR_RANGE, naming the belief, before anything is launched: a slot out of
 * range, an empty mask or one that leaves the manifold, n_mass or n_prob outside 0 .. NBP_CRED_MAX, a mass outside (0, 1] or a
 * probability outside [0, 1] (non-finite ones too), a non-finite query entry, a q_first that does not ascend from 0.  An unknown
 * manifold and null pointers (with n > 0): NBP_ERR_ARG; n <= 0: NBP_OK.  q_first == NULL: no queries (queries and qrec_out are not
 * read).  One workgroup per belief in ONE launch; queued on the library stream; one copy each way; synchronises. */
#define NBP_CRED_MAX 8
typedef struct nbp_credible_opts {
  int32_t n_mass, n_prob;
  double mass[NBP_CRED_MAX], prob[NBP_CRED_MAX];
} nbp_credible_opts;
typedef struct nbp_credible_rec {
  double log_level[NBP_CRED_MAX];
  double quant[NBP_MAXD][NBP_CRED_MAX];
  double mean[NBP_MAXD];
  double log_min, log_max;
  int32_t n_inside[NBP_CRED_MAX];
  int32_t count, pad;
} nbp_credible_rec;
typedef struct nbp_credibility_rec {
  double logdens, mass;
  int32_t n_above, pad;
} nbp_credibility_rec;
nbp_status nbp_run_credible(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, const int32_t *masks, int32_t n,
                            const nbp_credible_opts *opts, const int32_t *q_first /* n+1, nullable: no queries */,
                            const double *queries /* q_first[n] x NBP_MAXD */, nbp_credible_rec *rec_out /* n */,
                            double *logdens_out /* n x N, nullable; NaN beyond the count */,
                            int32_t *order_out /* n x N, nullable; -1 beyond the count */,
                            nbp_credibility_rec *qrec_out /* q_first[n] */);
/* host-buffer form, like nbp_kde_meancov: stages through slot 0 (N = the context's particle count in the output shapes) */
nbp_status nbp_kde_credible(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, const double *bw_D, int32_t mask,
                            const nbp_credible_opts *opts, const double *queries /* nq x NBP_MAXD */, int32_t nq,
                            nbp_credible_rec *rec_out, double *logdens_out /* N, nullable */, int32_t *order_out /* N, nullable */,
                            nbp_credibility_rec *qrec_out /* nq */);
/* ---- modes of a belief ("Modes of a belief"; DEFINED by this library, unpinned: DESIGN.md 8) -----------------------
 * Mean-shift over the belief's own KDE at the bandwidth g = bw_scale * bw.  Every point x_i of the belief is a start y <- x_i;
 * one iteration is  w_j = exp(e(y, x_j)) (the exponent of nbp_run_evaluate with g in place of bw),  S = sum_j w_j,
 * m_d = sum_j w_j delta_d(x_j, y) (delta wrapped to [-pi, pi) on circular coordinates),  y_d <- y_d + m_d / S (wrapped on circular
 * coordinates); j = 0 .. c-1 in that order in one lane, one rounding per written operation: a trajectory depends on the belief
 * and the options alone.  A start stops after the first iteration with max_d |m_d / S| / g_d <= tol (converged) or after max_iter
 * iterations.  A start is a point of the belief, so S >= 1 at its first iteration, and a mean-shift step does not decrease the
 * density: S never vanishes.
 * The end points are merged by leader clustering in index order: the lowest unassigned i becomes a leader, every unassigned k > i
 * with max_d |delta_d(y_k, y_i)| / g_d <= merge joins it.  Modes are ranked by member count, descending, equal counts by the lower
 * leader index.  Record r of a belief is the mode of rank r: the leader's end point, the member count, the KDE at bandwidth g at that
 * point (S there / (c prod_d sqrt(2 pi) g_d)) and the leader's index; records from n_modes on (at most NBP_MODES_MAX are kept)
 * hold NaN, count 0 and leader -1.  n_modes is the true number of modes, also above NBP_MODES_MAX.  labels: the rank of each
 * point's mode (rows beyond the belief's count: -1); iters: the iterations each start took (rows beyond the count: 0).  A bandwidth
 * entry bw_d or g_d that is not positive and finite: n_modes = 0, labels -1, iters 0, every record empty.
 * Options: bw_scale, merge positive and finite, tol positive, max_iter >= 1, else NBP_ERR_ARG; merge < 1000 tol is NBP_ERR_RANGE (a
 * stopped start may still sit tol rho / (1 - rho) from its fixed point, rho the contraction rate).  opts == NULL: the defaults
 * below.  The fitted bandwidth is the leave-one-out one and under-smooths for mode finding: hence bw_scale = 2.
 * Argument errors as nbp_run_ppe's, before anything is launched.  Queued on the library stream; one copy back; synchronises. */
#define NBP_MODES_MAX 32
#define NBP_MODES_BW_SCALE 2.0
#define NBP_MODES_TOL 1e-6
#define NBP_MODES_MAX_ITER 500
#define NBP_MODES_MERGE 1e-2
typedef struct nbp_modes_opts {
  double bw_scale;
  double tol;
  double merge;
  int32_t max_iter;
  int32_t pad;
} nbp_modes_opts;
typedef struct nbp_mode_rec {
  double location[NBP_MAXD]; /* tangent coordinates, entries beyond the manifold's dimension zero */
  double density;
  int32_t count;
  int32_t leader;
} nbp_mode_rec;
nbp_status nbp_run_modes(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n, const nbp_modes_opts *opts /* nullable */,
                         nbp_mode_rec *recs_out /* n x NBP_MODES_MAX */, int32_t *n_modes_out /* n */,
                         int32_t *labels_out /* n x N, nullable */, int32_t *iters_out /* n x N, nullable */,
                         int32_t *n_unconverged_out /* n, nullable */);
/* host-buffer form, like nbp_kde_ppe: stages through slot 0; labels_out / iters_out hold n_pts entries (a belief of more than N
 * points keeps its first N, as in nbp_belief_write: the entries beyond them are -1 / 0) */
nbp_status nbp_kde_modes(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, const double *bw_D,
                         const nbp_modes_opts *opts /* nullable */, nbp_mode_rec *recs_out /* NBP_MODES_MAX */, int32_t *n_modes_out,
                         int32_t *labels_out /* n_pts, nullable */, int32_t *iters_out /* n_pts, nullable */,
                         int32_t *n_unconverged_out /* nullable */);
/* ---- mixture summaries ("Mixture summaries"; DEFINED by this library, unpinned: DESIGN.md 8) -------------------------
 * A resident belief as a Gaussian mixture of K <= NBP_MIX_MAX components (w_k, mu_k, Sigma_k): the form a belief can go back into a
 * graph in (NBP_F_PRIOR with components) or leave the library in.  Tangent coordinates at the identity (SE(2): x, y, theta in the
 * world frame); c the count the slot holds, D the dimension, delta(x, mu) = x - mu wrapped to [-pi, pi) on circular coordinates,
 * H = diag(h_d^2) the belief's own bandwidth.  The belief's KDE is itself a mixture of c Gaussians N(x_i, H); it is reduced by
 * hierarchical EM on the kernel centres, each kernel's width entering in expectation.
 *   start   one label row per belief (labels[row[i]], int32, -1 .. NBP_MIX_MAX - 1): particle i starts in the component its label
 *     names with r_ik = 1, a particle labelled -1 starts in none.  A component is live when a particle below the count carries its
 *     label; mu_k starts at init_mean[i][k] (the modes of nbp_run_modes and their ranks are what the Python layer passes).
 *   M-step  live components in ascending k: n_k = sum_i r_ik; a live component with n_k < 0.5 is dropped for good (weight 0, no
 *     part in later steps, counted in n_dropped); w_k = n_k / sum_{l live} n_l;
 *     mu_k <- wrap(mu_k + sum_i r_ik delta(x_i, mu_k) / n_k) (on a Euclidean coordinate the weighted mean in one step);
 *     Sigma_k = sum_i r_ik delta_i delta_i^T / n_k + H, delta_i about the new mean.  Sigma_k >= H: never singular, no floor.
 *   E-step  l_ik = log w_k + log N(delta(x_i, mu_k); 0, Sigma_k) - tr(Sigma_k^-1 H) / 2 (the Cholesky factor in closed form);
 *     lse_i = logsumexp_k l_ik in two passes (the maximum, then the sum), k ascending in one lane; r_ik = exp(l_ik - lse_i);
 *     J = (1 / c) sum_i lse_i, finite where every density underflows.  A proper EM: on Euclidean manifolds J never decreases.
 *   stop    after the E-step of iteration t >= 2 when J_t - J_(t-1) <= tol (converged = 1), or after max_iter iterations.  tol = 0
 *     runs max_iter iterations (converged = 0).
 *   result  live components ranked by weight descending, ties by the lower starting index: weight, mean, cov (NBP_MAXD x NBP_MAXD,
 *     row-major, zero beyond D, both triangles the same double), count = the particles whose greatest r is this component's (ties
 *     to the lower starting index); n_comp, iters, converged, n_dropped, objective = J.  Entries from n_comp on are zero.
 *     labels_out: each particle's component by its final rank, -1 beyond the count.
 *   a bandwidth entry that is not positive and finite, or a row with no label >= 0 below the count: n_comp = 0, iters = 0, every
 *     double of the record NaN, labels_out -1.  c = 1: one component, the point itself, Sigma = H.
 * Sums over the particles: a butterfly inside each wave, then the waves in order (the additions of nbp_run_meancov).  A belief's
 * result depends on the belief, its labels, its starting means and the options alone, not on the beliefs that share the launch.
 * opts == NULL: the defaults below.  NBP_ERR_ARG: tol negative or not finite, max_iter < 1, a label outside -1 .. NBP_MIX_MAX - 1
 * in a row an item names (all N entries of such a row are looked at; a row no item names is not read), a negative row, an unknown
 * manifold, null pointers (with n > 0); NBP_ERR_RANGE: a slot out of range.  Refused before anything is launched.  n <= 0: NBP_OK.
 * One workgroup per belief in ONE launch; queued on the library stream; one copy each way; synchronises. */
#define NBP_MIX_MAX 8
#define NBP_MIX_TOL 1e-8
#define NBP_MIX_MAX_ITER 500
typedef struct nbp_mixture_opts {
  double tol;
  int32_t max_iter, pad;
} nbp_mixture_opts;
typedef struct nbp_mixture_rec {
  double weight[NBP_MIX_MAX];
  double mean[NBP_MIX_MAX][NBP_MAXD];
  double cov[NBP_MIX_MAX][NBP_MAXD * NBP_MAXD];
  double objective;
  int32_t count[NBP_MIX_MAX];
  int32_t n_comp, iters, converged, n_dropped;
} nbp_mixture_rec;
nbp_status nbp_run_mixture(nbp_ctx *ctx, const int32_t *slots, const int32_t *manifolds, int32_t n,
                           const int32_t *labels /* n_rows x N */, const int32_t *row /* n: the label row of belief i */,
                           const double *init_mean /* n x NBP_MIX_MAX x NBP_MAXD */, const nbp_mixture_opts *opts /* nullable */,
                           nbp_mixture_rec *recs_out /* n */, int32_t *labels_out /* n x N, nullable */);
/* host-buffer form, like nbp_kde_modes: stages through slot 0; labels / labels_out hold n_pts entries (a belief of more than N
 * points keeps its first N: the entries of labels_out beyond them are -1) */
nbp_status nbp_kde_mixture(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, int32_t n_pts, const double *bw_D,
                           const int32_t *labels /* n_pts */, const double *init_mean /* NBP_MIX_MAX x NBP_MAXD */,
                           const nbp_mixture_opts *opts /* nullable */, nbp_mixture_rec *rec_out, int32_t *labels_out /* n_pts, nullable */);
/* ---- factor likelihoods ("Factor likelihoods"; DEFINED by this library, unpinned: DESIGN.md 8) ----------------------
 * The likelihood of a factor's measurement model under the current beliefs of its variables: which association of a multihypo
 * factor won, which Mixture component explains the data, which factor disagrees with the solution.  One ITEM is (measurement
 * model, slot A, slot B); slot_b = -1 for a unary factor (NBP_F_PRIOR).  n_a, n_b: the counts the slots hold (n_b = 1 for a unary
 * item).  A Monte-Carlo sum over the particles: bandwidths are never read.
 * Predicted measurement zhat(a_i, b_j), the root of the factor's residual, in tangent coordinates (SE(2): x, y, theta):
 *   NBP_F_LINREL      b - a, D coordinates
 *   NBP_F_CIRCULAR    wrap_pi(b - a)
 *   NBP_F_SE2         (c dx + s dy, -s dx + c dy, wrap_pi(b_th - a_th)), (s, c) = sincos(a_th), dx, dy = b_xy - a_xy
 *   NBP_F_EUCLIDDIST  sqrt(sum_d (b_d - a_d)^2)
 *   NBP_F_PRIOR       a_i
 *   partial_mask != 0 only the masked coordinates of the above, in ascending order: popcount(mask) dimensions (zd), as in
 *                     nbp_proposal_desc; admitted where the samplers admit it (Prior, SE(2), LinearRelative with one or two bits)
 * Component log-density log p_c(z); comp[c] = weight, mean[3], L[3][3] as the samplers read it, the family in comp[c][12] when zd = 1:
 *   Gaussian          delta = z - mean, wrapped to [-pi, pi) on circular coordinates (Circular; theta of SE(2)); L u = delta by
 *                     forward substitution (u_0 = delta_0 / L_00, u_1 = (delta_1 - L_10 u_0) / L_11,
 *                     u_2 = ((delta_2 - L_20 u_0) - L_21 u_1) / L_22); log p = -1/2 sum_k u_k^2 - (zd log(2 pi) / 2 + sum_k log L_kk),
 *                     the squares added in ascending order
 *   Uniform(a, a + w) -log w on [a, a + w], else -inf                (mean[0] = a, L[0][0] = w)
 *   Rayleigh(sigma)   (log z - 2 log sigma) - z^2 / (2 sigma^2) for z > 0, else -inf
 *   Uniform and Rayleigh are evaluated at zhat as formed, with no further wrap.
 * Sums, one rounding per written operation:
 *   e_ijc = log(w_c / sum w) + log p_c(zhat_ij)
 *   pass 1: M = max_ijc e_ijc (exact in any order)
 *   pass 2: S_c = sum_i sum_j exp(e_ijc - M); a term with e_ijc - M < -700 counts as zero; j = 0 .. n_b - 1 in that order in the
 *           lane that owns i, the lanes combined by the library's fixed-order block sum (no atomics)
 *   loglik = (M + log(sum_c S_c)) - log(n_a n_b);  comp_loglik[c] = (M + log S_c) - log(n_a n_b) (S_c = 0: -inf): the logsumexp of
 *           comp_loglik over c is loglik.  Entries c >= ncomp are NaN.
 * The result is finite where every density underflows (a factor 10^4 sigma off: about -5e7, not -inf).  M = -inf (nothing in the
 * support of a Uniform / Rayleigh model): loglik = -inf.  A belief without points (host-buffer form only: a slot always holds at
 * least one) gives NaN.
 * Posterior weights are host arithmetic on these numbers:
 *   hypotheses of a multihypo factor: pi_k proportional to p_k exp(l_k), p_k the normalised fractional entries of `multihypo`, l_k the
 *           loglik of the item with variable k in its role; the null hypothesis has no likelihood and stays out (nullhypo is ignored)
 *   Mixture responsibilities: exp(comp_loglik[c] - loglik)
 *   both formed by max-shift; all -inf gives NaN.
 * Refused before anything is launched, naming the item -- NBP_ERR_ARG: NBP_F_MSGPRIOR, NBP_F_PASSTHROUGH (and measurements held as
 * a KDE, which this descriptor cannot name), NBP_DIST_TABLE or an unknown family; an L with a non-zero above the diagonal or a
 * diagonal entry that is not positive and finite; a Uniform width or Rayleigh sigma that is not positive and finite; a weight that is
 * negative or not finite, or weights without a positive sum; ncomp outside 1 .. NBP_MAXC; a kind / manifold pair, a mask or a slot_b
 * the samplers do not admit for the kind.  NBP_ERR_RANGE: a slot out of range; a mask outside the manifold's coordinates.
 * n = 0 returns NBP_OK.  Queued on the library stream; one upload of the descriptors, one copy back; synchronises. */
typedef struct nbp_likelihood_desc {
  int32_t kind;         /* enum nbp_factor                                                     */
  int32_t manifold;     /* enum nbp_manifold of the factor's variables                         */
  int32_t slot_a;       /* the belief in the first role (getVariableOrder)                     */
  int32_t slot_b;       /* the belief in the second role; -1: unary                            */
  int32_t ncomp;        /* 1, or the number of Mixture components                              */
  int32_t partial_mask; /* 0: full factor, else as nbp_proposal_desc.partial_mask              */
  double comp[NBP_MAXC][NBP_COMP_STRIDE]; /* measurement model, see NBP_COMP_STRIDE            */
} nbp_likelihood_desc;
nbp_status nbp_run_factor_likelihood(nbp_ctx *ctx, const nbp_likelihood_desc *descs, int32_t n, double *loglik_out /* n */,
                                     double *comp_loglik_out /* n x NBP_MAXC, nullable */);
/* host-buffer form, like nbp_kde_kld: stages through slots 0 and 1 (a unary item: slot 0), which it clobbers; desc->slot_a / slot_b
 * are not read; b_NxP is not read for a unary item */
nbp_status nbp_factor_likelihood(nbp_ctx *ctx, const nbp_likelihood_desc *desc, const double *a_NxP, int32_t na, const double *b_NxP,
                                 int32_t nb, double *loglik_out, double *comp_loglik_out /* NBP_MAXC, nullable */);
/* ---- local products on a grid ("Local products on a grid"; DEFINED by this library, unpinned: DESIGN.md 8) ------------
 * The product of the messages a variable's factors send it, WITHOUT particles for the variable itself: its clouds are replaced by a
 * regular grid over its coordinates, every factor's message is the closed-form measurement density at the cell summed over the
 * neighbour's cloud, the logs are added and normalised by quadrature.  It is what one Gibbs update of the variable would return
 * with infinitely many particles and no kernel smoothing, given the same neighbour clouds.  No bandwidth enters a value.
 * GRID.  The variable lies on `manifold` with D = 1, 2 or 3 coordinates; the grid has one axis per coordinate, in coordinate order;
 * cell (k0, k1, k2) is the point x = (lo[a] + (double)k_a step[a])_a; n[a] for a >= D must be 1.  The output is row-major, coordinate
 * 0 slowest.  flags & NBP_PGRID_AUTO_EXTENT: lo and step are not read; per axis the rule of nbp_grid_desc from the resident belief
 * in `slot` (Euclidean: min_j x - margin bw .. max_j x + margin bw, step = (hi - lo) / (n - 1), n >= 2; circular: lo = -pi, step =
 * 2 pi / n) -- the same code, so for D <= 2 the axes are nbp_run_marginal_grid's bit for bit.  Without the flag `slot` is not read.
 * ITEM.  A measurement model (`lik`, read exactly as nbp_run_factor_likelihood reads it; its slot_a / slot_b are NOT read), the role
 * the grid's variable fills and the slot `other` of the other variable's resident belief u_0 .. u_{n-1} (n: the count of the slot):
 *   role 0   x stands for a_i and u_j for b_j;   role 1   u_j stands for a_i and x for b_j;   a unary item: role 0, other = -1, n = 1
 *   e_jc(x)  the e_ijc of nbp_run_factor_likelihood for that pair: zhat, log p_c, the wrap rules, the partial masks, the families
 *            and one rounding per written operation are those defined there; (sin, cos) of an SE(2) heading by the same sincos
 *   M        max_{j,c} e_jc(x);   S_c = sum_j exp(e_jc(x) - M), j ascending from 0.0, a term with e_jc - M < -700 counts as zero;
 *            S = sum_c S_c, c ascending from 0.0; both passes in the lane that owns the cell
 *   log m(x) (M + log S) - log((double)n);   M = -inf: -inf
 * GROUP.  Every item carries `group`, non-decreasing along the item range of every grid, and `log_prior`.  Consecutive items of one group are the
 * hypotheses of one multihypo factor whose certain variable is the grid's; t_k = log_prior_k + log m_k(x).  A group of ONE item:
 * l_g = t_0 (log_prior = 0: log m(x) untouched).  More: a running max-shift in item order, (mx, s) = (-inf, 0);
 *   t_k > mx:  s = (mx > -inf ? s exp(mx - t_k) : 0) + 1, mx = t_k;    else t_k > -inf:  s = s + exp(t_k - mx)
 * (the exponentials as in S, below -700 zero); l_g = mx + log s, or -inf where mx = -inf.
 * RESULT.  L(x) = sum_g l_g(x), the groups added in list order starting from 0.0: a grid without items is 0.0 everywhere.  A value
 * depends on its point and its item list alone -- not on the grid, the chunk of 256 cells or the launch around it.  A second kernel,
 * one workgroup of 256 lanes per grid, lane t owning the cells t, t + 256, .. in ascending order:
 *   logmax = max L (exact);  argmax = the lowest cell index among equals;  Z' = sum exp(L - logmax) (below -700: zero), the lanes
 *   added by the library's fixed-order block sum;  logZ = (logmax + log Z') + (sum_{a < D, n[a] > 1} log step[a]), a ascending from
 *   0.0 -- an axis with n = 1 is a slice and adds nothing.  Every cell -inf: logZ = logmax = -inf, argmax = -1.
 * BATCH.  Descriptor i fills logp_out[first[i] .. first[i+1] - 1] and names the items first_item .. first_item + n_items - 1 of
 * `items`; several descriptors may name the same range.  One upload, one launch sequence (extents, cells, normalisation), one copy
 * back of the records and extents beside the grids' own; synchronises.  extent_out: lo0, step0, lo1, step1, lo2, step2 as used
 * (axes >= D: 0, 0).  n_desc = 0 returns NBP_OK.
 * Refused before anything is launched, naming the descriptor or the item: everything nbp_run_factor_likelihood refuses (the same
 * check, with `other` in place of the slots); NBP_ERR_ARG: a role outside 0 / 1, role 1 or other != -1 on a unary item, groups that
 * decrease within a grid's range, a log_prior that is NaN or +inf, an item whose manifold is not the grid's, an unknown manifold or flag; NBP_ERR_RANGE: n
 * outside 1 .. NBP_GRID_MAX (or != 1 beyond D), more than 2^22 cells in a grid, n < 2 on a Euclidean axis with the automatic extent,
 * a slot out of range (automatic extent), a non-finite lo, a step that is not finite and positive (explicit extent), a non-finite
 * margin (automatic extent), an item range outside the list, offsets that do not match.
 * Out of this version: factors where the grid's variable is a FRACTIONAL variable of a multihypo (their message has a flat part
 * without a normaliser), and nullhypo, which is ignored. */
#define NBP_PGRID_AUTO_EXTENT 1
#define NBP_PGRID_MAX_CELLS (1 << 22)
#define NBP_PGRID_CHUNK 256 /* cells per workgroup, one per lane; also the lanes of the normalisation */
typedef struct nbp_product_item {
  nbp_likelihood_desc lik; /* the measurement model; slot_a / slot_b are not read                 */
  int32_t role;            /* 0: the grid's variable fills role a, 1: role b                      */
  int32_t other;           /* the slot of the other variable; -1: unary                           */
  int32_t group;           /* non-decreasing along the list                                       */
  int32_t pad;
  double log_prior;        /* log of the hypothesis' prior; 0 for a plain factor                  */
} nbp_product_item;
typedef struct nbp_product_grid_desc {
  int32_t manifold;
  int32_t slot; /* the variable's own resident belief: read for the automatic extent only       */
  int32_t n[3];
  int32_t flags;
  int32_t first_item;
  int32_t n_items;
  double lo[3];
  double step[3];
  double margin;
} nbp_product_grid_desc;
typedef struct nbp_product_grid_rec {
  double logZ;
  double logmax;
  int32_t argmax;
  int32_t pad;
} nbp_product_grid_rec;
nbp_status nbp_run_product_grid(nbp_ctx *ctx, const nbp_product_grid_desc *descs, int32_t n_desc, const nbp_product_item *items,
                                int32_t n_items, const int32_t *first /* n_desc + 1 */, double *logp_out /* first[n_desc] */,
                                nbp_product_grid_rec *recs_out /* n_desc, nullable */, double *extent_out /* n_desc x 6, nullable */);
/* host-buffer form for one grid, like nbp_factor_likelihood: the variable's own points own_NxP (n_own of them) and bandwidth own_bw_D
 * go through slot 0 -- read for the automatic extent only, and all three may be NULL / 0 without it -- and the cloud others[k] (counts[k]
 * points, NULL for a unary item) of item k through slot 1 + k: slots 0 .. n_items are clobbered and the context needs 1 + n_items
 * slots.  desc->slot, first_item and n_items and every item's `other` are not read.  Every refusal comes before a slot is touched. */
nbp_status nbp_product_grid(nbp_ctx *ctx, const nbp_product_grid_desc *desc, const nbp_product_item *items, int32_t n_items,
                            const double *const *others /* n_items */, const int32_t *counts /* n_items */, const double *own_NxP,
                            int32_t n_own, const double *own_bw_D, double *logp_out, nbp_product_grid_rec *rec_out /* nullable */,
                            double *extent_out_6 /* nullable */);
/* ---- factor likelihoods, mode by mode ("Joint hypotheses"; DEFINED by this library, unpinned: DESIGN.md 8) ----------
 * Which mode of one variable belongs with which mode of another: the likelihood of a factor's measurement model given "a is in its
 * group k and b is in its group l", for every pair of groups at once.  One ITEM is (measurement model, slot A, slot B, label row of
 * A, label row of B).  The measurement model is an nbp_likelihood_desc, read exactly as nbp_run_factor_likelihood reads it: zhat,
 * log p_c, e_ijc, the wrap rules, one rounding per written operation and the cut-off at -700 are those defined above.
 * labels holds n_rows rows of N int32 each (N: the context's particle count).  Entry i of a row is the group of particle i, in
 * -1 .. NBP_MAXK - 1; -1 leaves the particle out of both roles.  The kernel reads the first n_a (n_b) entries of a row, the count
 * its slot holds.  Row index -1 stands for "every point in group 0".  A unary item has one column: row_b is -1 and n_l = 1.
 * With n_k, n_l the member counts of group k of A and group l of B:
 *   pass 1: M_kl = max over i in k, j in l, c of e_ijc (exact in any order): one maximum per cell, so a cell 10^4 sigma off stays
 *           finite (about -5e7)
 *   pass 2: S_klc = sum_{i in k} sum_{j in l} exp(e_ijc - M_kl); j ascending in the lane that owns i, the lanes combined by the
 *           library's fixed-order block sum with an exact zero in every lane that is not a member, the components then added in
 *           ascending c.  Adding an exact zero changes nothing: a masked sum and a skipped term in the same order are one number.
 *   table_out[i][k][l] = (M_kl + log sum_c S_klc) - log((double)n_k (double)n_l);  M_kl = -inf: -inf;  no member pair (n_k = 0 or
 *           n_l = 0, which includes every unused row and column of the NBP_MAXK x NBP_MAXK output): NaN
 *   counts_out[i][0][k] = n_k, counts_out[i][1][l] = n_l (a unary item: 1, 0, 0, ...)
 * Two identities: with every label 0 (or both rows -1) table_out[i][0][0] is nbp_run_factor_likelihood's loglik of the same item
 * BIT FOR BIT (the same maximum, scan, block sum and order over the components); with no point left out,
 * logsumexp_kl(T[k][l] + log(n_k n_l)) - log(n_a n_b) is that loglik up to rounding.
 * The joint score of a choice of one mode per variable -- the sum of the cells the choice picks, a multihypo factor entering as
 * logsumexp_h(log p_h + T_h) -- and its maximisation are host arithmetic on these tables (jointmodes.py).
 * Refused before anything is launched, naming the item or the row: everything nbp_run_factor_likelihood refuses, through the same
 * check; NBP_ERR_ARG: a label outside -1 .. NBP_MAXK - 1 in a row that an item names (the counts live on the device, so all N
 * entries of such a row are looked at; a row no item names is not read), row_b != -1 on a unary item; NBP_ERR_RANGE: a row index
 * outside -1 .. n_rows - 1.  labels may be NULL when n_rows = 0.
 * n = 0 returns NBP_OK.  Queued on the library stream; one upload of the descriptors, the row indices and the label rows, one
 * launch, one copy back; synchronises. */
nbp_status nbp_run_factor_mode_likelihood(nbp_ctx *ctx, const nbp_likelihood_desc *descs, const int32_t *row_a /* n */,
                                          const int32_t *row_b /* n */, int32_t n, const int32_t *labels /* n_rows x N */,
                                          int32_t n_rows, double *table_out /* n x NBP_MAXK x NBP_MAXK */,
                                          int32_t *counts_out /* n x 2 x NBP_MAXK, nullable */);
/* host-buffer form, like nbp_factor_likelihood: stages through slots 0 and 1 (a unary item: slot 0), which it clobbers;
 * desc->slot_a / slot_b are not read; labels_a (na entries) and labels_b (nb entries) may each be NULL: every point in group 0;
 * b_NxP and labels_b are not read for a unary item.  A belief of more than N points keeps its first N, as in nbp_belief_write.
 * A belief without points: every cell NaN, every count 0, nothing launched. */
nbp_status nbp_factor_mode_likelihood(nbp_ctx *ctx, const nbp_likelihood_desc *desc, const double *a_NxP, int32_t na,
                                      const int32_t *labels_a /* na, nullable */, const double *b_NxP, int32_t nb,
                                      const int32_t *labels_b /* nb, nullable */, double *table_out /* NBP_MAXK x NBP_MAXK */,
                                      int32_t *counts_out /* 2 x NBP_MAXK, nullable */);
/* ---- heatmap densities ("Heatmap densities"; the deviations from the reference: DESIGN.md 8) --------------------------
 * HeatmapGridDensity / LevelSetGridNormal (ext/HeatmapSampler.jl:123-242): a scalar field on a regular x-y grid turned into a
 * samplable density, the measurement model of the pass-through prior (NBP_F_PASSTHROUGH).  data[i * ny + j] is the field at
 * (x[i], y[j]).  The arithmetic -- cell weights and the fixed-order prefix sum, the inverse-CDF draws, the bilinear formula, the
 * weights exp(-(d - dmin)) -- is written once in csrc/nbp_heatmap.h and restated in heatmap.py.  Everything runs on the context's
 * stream; a call with host outputs returns after they are filled.  A heatmap does not outlive its context: nbp_ctx_destroy frees
 * what it holds on the device, after which only nbp_heatmap_destroy accepts the handle.
 *
 * nbp_heatmap_create   sampleHeatmap(field, x, y, 0) and the bandwidth of fitKDE (:123-159): checks the grid ON THE HOST, before
 *                      anything is allocated or launched -- nx, ny >= 2, nx * ny <= 2^26, x and y strictly increasing with uniform
 *                      spacing (|x[i+1] - x[i] - dx| <= 1e-9 |dx|, dx = (x[nx-1] - x[0]) / (nx - 1)), every datum finite, at least
 *                      one positive, bw_factor positive and finite: else NBP_ERR_INVALID (the sizes are looked at before the
 *                      pointers) --, uploads the field and leaves cdf and total on the device.  h = bw_factor * 0.5 * (dx + dy).
 * nbp_heatmap_build    sample(density_, N), the interpolation and the weights (:179-199): M pre-samples (1 <= M <= 2^26) under
 *                      `seed`; may be called again: replaces the pre-samples.  Host outputs (all nullable): the cell index, the
 *                      point, the field value and the weight of every pre-sample.
 * nbp_heatmap_draw     the density as this library holds it (:205-209 keeps the M weighted pre-samples; a belief here is
 *                      unweighted and a slot holds at most N points): n points drawn from the pre-samples by weight under `seed`,
 *                      bandwidth (h, h); jitter != 0 adds h * randn, which is AMP.sample(hgd, n) (:113).  slot >= 0: the points
 *                      also become the NBP_EUCLID2 belief of that slot (rows 0 and 1, count n, bandwidth (h, h), infoPerCoord 0,
 *                      the layout nbp_belief_write leaves); n > N is refused then.  slot = -1: no slot.  Before a build:
 *                      NBP_ERR_INVALID.  Host outputs nullable: the pre-sample taken, the point, the bandwidth.
 * nbp_heatmap_info     h twice, total, wtotal and M (0 before a build; wtotal then 0); outputs nullable. */
#define NBP_ERR_INVALID (-5)
typedef struct nbp_heatmap nbp_heatmap;
nbp_status nbp_heatmap_create(nbp_ctx *ctx, const double *data /* nx x ny */, int32_t nx, int32_t ny, const double *x, const double *y,
                              double bw_factor, nbp_heatmap **out);
nbp_status nbp_heatmap_build(nbp_heatmap *hm, int32_t M, uint64_t seed, int32_t *cell_M, double *pre_Mx2, double *d_M, double *W_M);
nbp_status nbp_heatmap_draw(nbp_heatmap *hm, int32_t n, uint64_t seed, int32_t jitter, int32_t slot /* -1: none */, int32_t *pick_n,
                            double *pts_nx2, double *bw_2);
nbp_status nbp_heatmap_info(const nbp_heatmap *hm, double *bw_2, double *total, double *wtotal, int32_t *M);
nbp_status nbp_heatmap_destroy(nbp_heatmap *hm);
/* Self-tests of the two primitives every heatmap density is built on (csrc/nbp_heatmap.h; tests/test_gpu_heatmap_scan.py), host
 * buffers in and out.  scan_eval: out[n] = SCAN(w), w = in where 0 < in, else 0 -- the launches nbp_heatmap_create and
 * nbp_heatmap_build make, all n sums back.  search_eval: idx_out[k] = SEARCH(cdf, t[k]), k < nt, one lane per probe; cdf is any
 * n doubles, not necessarily a scan.  n (and nt) outside 1 .. 2^26: NBP_ERR_INVALID (the sizes are looked at before the
 * pointers); a null pointer: NBP_ERR_ARG.  Neither keeps anything on the device. */
nbp_status nbp_heatmap_scan_eval(nbp_ctx *ctx, const double *in, int32_t n, double *out);
nbp_status nbp_heatmap_search_eval(nbp_ctx *ctx, const double *cdf, int32_t n, const double *t, int32_t nt, int32_t *idx_out);
/* ---- variable seam: AMP.manifoldProduct + rebandwidth (GraphProductOperations.jl:53-60) --- */
nbp_status nbp_run_products(nbp_ctx *ctx, const nbp_product_desc *descs, int32_t n);
/* ---- host-buffer entry points: one call per reference function ----------------------------------
 * For callers that keep beliefs on the host (the factor / variable seams of the Julia shim).  Points are
 * packed AoS like nbp_slot_write; the calls stage through slots 0.. of the context (which they clobber)
 * and synchronise before returning.
 *
 * nbp_kde_bandwidth:     AMP.manikde!(M, pts) bandwidth selection (ApproxConv.jl:38,41; FGOSUtils.jl:118-128).
 * nbp_conv:              approxConvBelief(dfg, fct, target) (ApproxConv.jl:4-45): `tmpl` carries the factor
 *                        (kind, manifold, nvars, sfidx, comp, multihypo, nullhypo, ..., seed); its slot fields
 *                        are ignored.  var_pts[i] = points of variable i (MsgPrior: [target, message KDE] and
 *                        var_bw[1] = the KDE's bandwidth).  mhidx_in / out_mhidx nullable (needs 2N side ints);
 *                        out_bw NULL skips the bandwidth fit.  Context: >= nvars + 1 slots.
 * nbp_manifold_product:  AMP.manifoldProduct(dens, M; Niter, oldPoints) + rebandwidth
 *                        (GraphProductOperations.jl:53-60).  partial_masks / old_pts / out_labels nullable.
 *                        Context: >= F + 2 slots (and N*F side ints for the labels).                        */
nbp_status nbp_kde_bandwidth(nbp_ctx *ctx, int32_t manifold, const double *pts_NxP, double *bw_out_D);
nbp_status nbp_conv(nbp_ctx *ctx, const nbp_proposal_desc *tmpl, const double *const *var_pts, const double *const *var_bw,
                    const int32_t *mhidx_in, double *out_pts_NxP, double *out_bw_D, int32_t *out_mhidx);
nbp_status nbp_manifold_product(nbp_ctx *ctx, int32_t manifold, int32_t nfactors, const double *const *dens_pts,
                                const double *const *dens_bw, const uint8_t *partial_masks, const double *old_pts,
                                int32_t niter, uint64_t seed, double *out_pts_NxP, double *out_bw_D, int32_t *out_labels);

/* approxDeconv(dfg, fct) (services/DeconvUtils.jl:32-160): per particle, sample a measurement and
 * search from it for the measurement that zeroes the residual between the stored points of the two
 * variables (var_slot[0], var_slot[1]).  out_slot receives the predicted measurement (tangent
 * coordinates k < zDim, read it back with the Euclid manifold of that dimension), meas_slots[i] (may be
 * NULL / -1) the sampled one.  Relative factors without multihypo only (reference #467/#927). */
nbp_status nbp_run_deconv(nbp_ctx *ctx, const nbp_proposal_desc *descs, const int32_t *meas_slots, int32_t n);
nbp_status nbp_run_copies(nbp_ctx *ctx, const nbp_copy_desc *descs, int32_t n);
/* the same queued on the library stream without waiting (points_only != 0: the points and the count, not the bandwidth) */
nbp_status nbp_run_copies_async(nbp_ctx *ctx, const nbp_copy_desc *descs, int32_t n, int32_t points_only);

/* ---- clique seam: a whole up/down schedule resident on the device --------------------------
 * Replaces upGibbsCliqueDensity (SolveTree.jl:164-239) and solveCliqDownFrontalProducts!
 * (CliqStateMachineUtils.jl:479-571) for *all cliques of a tree level at once*: a program is an
 * ordered list of stages; a stage is a batch of independent proposals, products or copies.
 * Upload once, replay per solve.                                                              */
typedef struct nbp_program nbp_program;
enum nbp_stage_kind {
  NBP_STAGE_PROPOSALS = 1,
  NBP_STAGE_PRODUCTS = 2,
  NBP_STAGE_COPIES = 3,
  NBP_STAGE_DECONV = 4, /* nbp_proposal_desc[]: approxDeconv of a relative factor between var_slot[0] and
                           var_slot[1] (like nbp_run_deconv); out_slot receives the predicted measurements
                           AND their fitted bandwidth (manikde!), i.e. a KDE a later proposal can name in
                           meas_kde -- the child side of the differential messages
                           (addLikelihoodsDifferentialCHILD!, TreeMessageUtils.jl:279-335) */
  NBP_STAGE_COPY_POINTS = 5  /* nbp_copy_desc[]: copies the points of a slot only.  The destination's bandwidth is
                           left unspecified, nothing waits for a pending fit of the source: for values that are read
                           as points and never as a density -- the separator values a down message hands to a child
                           (updateSubFgFromDownMsgs!, TreeMessageUtils.jl:66-84) */
};
nbp_status nbp_program_create(nbp_ctx *ctx, nbp_program **out);
nbp_status nbp_program_add_stage(nbp_program *prog, int32_t kind, const void *descs, int32_t n);
/* Program options, to be set before nbp_program_finalize.
 * NBP_OPT_LAZY_BANDWIDTH (default 0): skip the bandwidth fit of a product output that a later stage
 * overwrites before anything reads its bandwidth (readers: a MsgPrior proposal sampling the slot, a
 * product taking it as input, slot copies; an EMPTY copy stage counts as "everything is read").  The
 * reference fits a bandwidth on every setBelief! (FactorGraph.jl:250-263), but inside a clique's Gibbs
 * sweeps only the last one of each variable is ever looked at, so no result changes.  With the option
 * on, the bandwidth of such an intermediate belief is undefined between stages.
 * NBP_OPT_GRAPH_REPLAY (default 1): nbp_program_run captures the launch sequence of a stage range into a hipGraph the
 * second time it runs and replays the graph afterwards (one submission instead of ~3 launches per variable update).
 * Ignored while per-kernel timing is enabled.
 * NBP_OPT_FUSED_UPDATES (default 1): a PROPOSALS stage followed by the PRODUCTS stage that multiplies exactly its proposals
 * (one round of Gibbs steps) may run as ONE launch of the fused update kernel -- proposals, their bandwidth fits, the KD
 * trees, the product and the fit of the result in one workgroup per variable, with nothing but the operand beliefs and
 * the new belief touching HBM -- when the round has at least NBP_FUSED_MIN updates (environment, read at nbp_ctx_create;
 * unset = never: the fused form trades time for traffic) and its factors are of a class the kernel is built
 * for (the list stands above fused_plan, csrc/nbp_api.hip); the same particles, bandwidths and infoPerCoord as the three-launch
 * form, bit for bit (one summation order in every geometry; tests/test_gpu_fused_update.py holds both forms to the oracle).
 * A stage range of nbp_program_run that ends between the two stages of a fused pair runs the pair in the three-launch form
 * (the proposals to their arena slots, their fits at the end of the range); a range that starts at the second stage of such a pair
 * fits every proposal of the pair again before the products (redundant after the previous range's end-of-range fits, never wrong). */
enum nbp_program_option { NBP_OPT_LAZY_BANDWIDTH = 1, NBP_OPT_GRAPH_REPLAY = 2, NBP_OPT_FUSED_UPDATES = 3,
                          NBP_OPT_ASYNC_UPLOAD = 4 /* (default 0) nbp_program_finalize sends the descriptors stream-ordered from a
                                                      pinned buffer and does not wait: for short-lived programs queued behind
                                                      running ones (the asynchronous clique seam, nbp_host.h) */,
                          NBP_OPT_UP_PASS_SINKS = 5 /* (default 0) the products of the up pass that nothing in that pass reads run
                                                       in one or two later "sink" stages of the pass instead of the stage of
                                                       their round, as one launch that fills the chip (include/nbp_sinks.h has
                                                       the rules; the up pass = the first run of stages between whole-slot copy
                                                       stages that holds products).  The stage list, the seed order and every
                                                       result stay what they are: the compiler works on gathered copies of the
                                                       descriptors.  For whole-tree programs of one rank (nbp_tree_compile sets
                                                       it).  Environment NBP_NO_SINKS=1 or NBP_NO_LANES=1 (read at
                                                       nbp_ctx_create): ignored */ };
/* options are set before nbp_program_finalize; NBP_OPT_GRAPH_REPLAY alone may also be switched afterwards (it is a property of the
 * runs: graphs already captured stay with the program) */
nbp_status nbp_program_set_option(nbp_program *prog, int32_t option, int32_t value);
nbp_status nbp_program_finalize(nbp_program *prog);              /* uploads descriptors        */
nbp_status nbp_program_run(nbp_program *prog, int32_t first_stage, int32_t last_stage /* excl, -1=all */);
nbp_status nbp_program_reseed(nbp_program *prog, uint64_t salt); /* xor-mix all op seeds on device */
/* New seeds for every op of a finalized program, in stage order: per proposal / deconvolution descriptor its seed and, where the
 * descriptor named a stored measurement when the program was finalized (meas_seed != 0), that one behind it; per product
 * descriptor its seed.  n = nbp_program_num_seeds.  Stream-ordered.  (The native host's plan cache: a batch of clique requests
 * whose structure has not changed is the same program with other seeds -- include/nbp_host.h.)
 * The order is the CALLER's: the stages and descriptors as nbp_program_add_stage took them.  nbp_program_finalize may move the
 * descriptors of a two-stream round inside their stage (NBP_PIPELINE_MIN); the library keeps track of where each one went, so
 * seeds[i] reaches the descriptor the caller gave i-th, and a stored measurement keeps naming the op that drew it.
 * nbp_program_seed_order tells where they went: order[i] = the place of seeds[i]'s field in a walk over the descriptors as
 * they lie in the finalized program (0, 1, 2 ... where nothing was moved). */
nbp_status nbp_program_num_seeds(nbp_program *prog, int32_t *out);
nbp_status nbp_program_set_seeds(nbp_program *prog, const uint64_t *seeds, int32_t n);
nbp_status nbp_program_seed_order(nbp_program *prog, int32_t *order, int32_t n);
nbp_status nbp_program_num_stages(nbp_program *prog, int32_t *out);
/* rounds of a finalized program that run as one launch of the fused update kernel (NBP_OPT_FUSED_UPDATES) */
nbp_status nbp_program_num_fused(nbp_program *prog, int32_t *out);
/* rounds of a finalized program whose two halves run on two streams, one launch apart (environment NBP_PIPELINE_MIN =
 * smallest product batch that is split; same particles and bandwidths as the single-stream order, bit for bit) */
nbp_status nbp_program_num_two_stream(nbp_program *prog, int32_t *out);
/* Lanes.  A hint for one stage, given before nbp_program_finalize: descriptor i may run on lane lane_of_descriptor[i] (0: the
 * library stream, 1: a second stream), beside whatever the other lane runs meanwhile -- for the updates of cliques whose
 * schedules are longer than their siblings', which would otherwise ride in chip-filling stages and finish alone (the native
 * host marks them: nbp_tree_schedule).  The stage list, the seed order and every result stay what they are without the
 * hint: what a lane waits for is derived from the slots, so a wrong hint costs time only.  Environment NBP_NO_LANES=1 (read
 * at nbp_ctx_create): hints are ignored. */
nbp_status nbp_program_set_lanes(nbp_program *prog, int32_t stage, const int32_t *lane_of_descriptor, int32_t n);
/* The plan of a finalized program, one record per part in list order (per stage its lane-0 descriptors, then its lane-1
 * descriptors): n_out = the number of parts (0: the program runs without lanes); at most cap records are written.
 * wait = the part of the other lane that must have finished before this one starts, -1: none. */
typedef struct nbp_lane_part_rec {
  int32_t stage, lane, first_desc, n, wait, signals;
} nbp_lane_part_rec;
nbp_status nbp_program_lane_plan(nbp_program *prog, nbp_lane_part_rec *out, int32_t cap, int32_t *n_out);
/* Beside it, per part in the same order: the descriptors the part gained from earlier stages (NBP_OPT_UP_PASS_SINKS; such a
 * part runs a gathered copy of its stage's remaining lane-0 descriptors and the gained ones: first_desc = 0, n = all of them).
 * A stage that lost descriptors shows in nbp_program_lane_plan as a lane-0 part shorter than the stage. */
nbp_status nbp_program_sink_plan(nbp_program *prog, int32_t *gained, int32_t cap, int32_t *n_out);
nbp_status nbp_program_destroy(nbp_program *prog);
/* destroy without waiting: the program is dropped once everything queued on the library stream so far has run */
nbp_status nbp_program_retire(nbp_program *prog);

/* ---- separator exchange between ranks (one process per GPU) -------------------------------------------------------
 * The reference moves a LikelihoodMessage through a Channel per tree edge (JunctionTreeUtils.jl:943-956,
 * CliqueStateMachine.jl:221-234/617-629); across GPUs the payload -- whole slots = TreeBelief (val, bw, infoPerCoord,
 * count) -- travels point to point over RCCL (xGMI), all messages of one exchange point in ONE grouped call on the
 * library's stream: stream-ordered with the producing and consuming kernels, no host synchronisation.
 * nbp_comm_unique_id: rank 0 makes the id (NBP_COMM_ID_BYTES bytes) and hands it to every rank by whatever means the
 * host has (a broadcast over torch.distributed, MPI, a file); nbp_comm_create is collective over the ranks. */
#define NBP_COMM_ID_BYTES 128
typedef struct nbp_comm nbp_comm;
#ifndef NBP_XFER_DEFINED
#define NBP_XFER_DEFINED
typedef struct nbp_xfer { int32_t peer; int32_t slot; } nbp_xfer;
#endif
nbp_status nbp_comm_unique_id(void *id_out /* NBP_COMM_ID_BYTES */);
nbp_status nbp_comm_create(nbp_ctx *ctx, int32_t world, int32_t rank, const void *id, nbp_comm **out);
nbp_status nbp_comm_destroy(nbp_comm *comm);
/* what RCCL itself says about the communicator: ncclCommCount / ncclCommUserRank (bench.py prints them: a scaling run shows
 * how many ranks the library's own communicator had, not how many the launcher was asked for) */
nbp_status nbp_comm_info(nbp_comm *comm, int32_t *nranks_out, int32_t *rank_out);
nbp_status nbp_exchange(nbp_ctx *ctx, nbp_comm *comm, const nbp_xfer *sends, int32_t n_sends, const nbp_xfer *recvs, int32_t n_recvs);

/* per-kernel timing with HIP events on the library stream (bench.py roofline leg) */
nbp_status nbp_timing_enable(nbp_ctx *ctx, int32_t on);
/* ms[4] / launches[4] per kernel: 0 = proposal kernel, 1 = prep kernel = bandwidth fits + KD-tree builds,
 *                      2 = product kernel, 3 = plain bandwidth kernel = early flushes; reset by the call */
nbp_status nbp_timing_read(nbp_ctx *ctx, double *ms, int64_t *launches);
/* the same with n <= 5 entries: 4 = the fused update kernel (NBP_OPT_FUSED_UPDATES); all five are reset by either call */
nbp_status nbp_timing_read_n(nbp_ctx *ctx, double *ms, int64_t *launches, int32_t n);
nbp_status nbp_diag_read(nbp_ctx *ctx, nbp_diag *out, int32_t reset);

/* ---- launch plans ------------------------------------------------------------------------
 * What a product, fit or proposal launch would run, as the library's own planners decide it: the queries need
 * no context and no GPU; they read the same environment switches (NBP_PRODUCT_*, NBP_LCV_*, NBP_NO_*, NBP_PROPOSAL_*, ...)
 * in the same way as context creation does, at the time of the call.  Arrays of requests, one record each. */
typedef struct nbp_product_plan_req {
  int32_t N;       /* particles of the context, 8 .. NBP_MAXN                                                   */
  int32_t n;       /* products in the launch                                                                     */
  int32_t F, D;    /* largest density count and largest manifold dimension of the launch                        */
  int32_t mani;    /* the manifold of a single-manifold launch, 0: mixed, -1: the widest workgroup any kernel takes */
  int32_t geom_n;  /* 0, or the whole batch of the two-stream round this launch is a half of                     */
} nbp_product_plan_req;
/* refusals of a product launch (status NBP_ERR_RANGE) */
#define NBP_PLAN_REFUSED_BIG_IN_ROUND 1 /* node statistics beyond the LDS inside a two-stream round */
#define NBP_PLAN_REFUSED_LDS 2          /* too many densities for the LDS label table               */
#define NBP_PLAN_REFUSED_NO_KERNEL 3    /* the kernel table has no row for the geometry             */
typedef struct nbp_product_plan_rec {
  int32_t status, refusal;       /* what the launch returns: NBP_OK / 0, or NBP_ERR_RANGE and which refusal; a query whose
                                    arguments no launch can have (D of a single manifold not its dimension): NBP_ERR_ARG */
  int32_t HL, wpb, G;            /* helper lanes per sample, waves per workgroup, workgroups per product                */
  int32_t big, xs, circ, nch, all_levels, w1;
  int32_t row;                   /* the row of the kernel table (-1: none) and what that row is:                        */
  int32_t row_HL, row_mani, row_xs, row_w1;
  int32_t launch_bound;          /* lanes the kernel of that row is compiled for                                        */
  int32_t N, n, F, D, mani, geom_n; /* the request (nbp_last_plans: what the launch was issued with; n = 0: none yet)   */
  int32_t pad;
  int64_t lds, gstats;           /* dynamic LDS bytes per workgroup; doubles of the global statistics area (big)        */
  char kernel[40];
} nbp_product_plan_rec;
typedef struct nbp_fit_plan_req {
  int32_t N;
  int32_t fits, coords;   /* bandwidth fits of the launch and their fitted coordinates (sum of the manifold dimensions)  */
  int32_t products, kdF;  /* > 0: a prep launch beside the KD builds of that many products of up to kdF densities         */
  int32_t geom_blocks;    /* 0, or the workgroups of the whole two-stream round this launch is a half of                  */
} nbp_fit_plan_req;
typedef struct nbp_fit_plan_rec {
  int32_t status;
  int32_t P, depth, KS, w5, threads;
  int32_t prep;           /* 1: a prep launch, 0: a plain bandwidth launch                                               */
  int32_t kd_nostats;     /* nbp_last_plans, prep launches: the KD builds left the node sums to an _xs product kernel     */
  int32_t N, fits, coords, products, kdF, geom_blocks; /* the request (nbp_last_plans: N = 0: no such launch yet)        */
  int32_t pad[2];
  int64_t lds;
  char kernel[40];
} nbp_fit_plan_rec;
typedef struct nbp_proposal_plan_req {
  int32_t N, n;
  int32_t manifold;       /* the manifold of a batch of one factor kind on one manifold, 0: anything else                */
  int32_t simple;         /* every proposal a binary relative (or a prior) on its one hypothesis                         */
} nbp_proposal_plan_req;
typedef struct nbp_proposal_plan_rec {
  int32_t status;
  int32_t geometry;       /* 0: a workgroup per proposal, 1: one wave, 2: two waves                                      */
  int32_t blocks, threads;
  int32_t N, n, manifold, simple;
  int64_t lds;
  char kernel[40];
} nbp_proposal_plan_rec;
nbp_status nbp_plan_products(const nbp_product_plan_req *req, nbp_product_plan_rec *out, int64_t n);
nbp_status nbp_plan_fits(const nbp_fit_plan_req *req, nbp_fit_plan_rec *out, int64_t n);
nbp_status nbp_plan_proposals(const nbp_proposal_plan_req *req, nbp_proposal_plan_rec *out, int64_t n);
/* The plans of the last product launch, the last prep launch and the last plain bandwidth launch of the context (any pointer
 * may be null), stored on the host when the launch is issued -- a captured program records at capture, not at replay. */
nbp_status nbp_last_plans(nbp_ctx *ctx, nbp_product_plan_rec *product, nbp_fit_plan_rec *prep, nbp_fit_plan_rec *fits);

/* Self-test of the elementary functions the kernels and the CPU checker share (include/nbp_math.h), evaluated ON THE DEVICE:
 * fn 0: out0 = log(a); 1: (out0, out1) = (sin, cos)(a); 2: out0 = atan2(a, b); 3: out0 = wrap to [-pi, pi) of a;
 * 4: (out0, out1) = the Box-Muller pair of the uniforms (a, b).  Host buffers of n doubles (b, out1 may be null where unused).
 * tests/test_gpu_device_math.py compares with the same header compiled by gcc: equal to the last bit. */
nbp_status nbp_math_eval(nbp_ctx *ctx, int32_t fn, const double *a, const double *b, double *out0, double *out1, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* NBP_H */
