"""MI355X-native drop-in for IncrementalInference.jl's per-clique nonparametric
Chapman-Kolmogorov hot path (approxConv -> per-particle solve -> manifold KDE product ->
clique Gibbs schedule).  Compute lives in csrc/libnbp.so (hand-written HIP, gfx950) behind the
C ABI of include/nbp.h; this package is the host-side mirror of the reference's API for that
path.  There is no CPU fallback: the compute entry points raise when libnbp.so or a GPU is
missing."""
from . import abi, bayestree, beliefquery, beliefstats, canonical, credible, heatmap, jointmodes, likelihood, marginal, mixture, modes, overlap, ppe, productgrid, scene, seeds  # noqa: F401
from .backend import HipBackend, NbpError  # noqa: F401
from .beliefquery import (Belief, density_numpy, getBelief, isapproxBeliefs, mmd, mmd_numpy, mmdVariables,  # noqa: F401
                          ppe_coords)
from .beliefstats import (calcMeanCovar, calcMeanCovarAll, entropy, kld, kld_numpy, meancov_numpy)  # noqa: F401
from .marginal import (Marginal, grid_axes, grid_extent_numpy, marginal_density_numpy, marginal_grid_numpy, marginalGrid)  # noqa: F401
from .modes import BeliefModes, getBeliefModes, getBeliefModesAll, modes_numpy  # noqa: F401
from .likelihood import (FactorLikelihood, FactorLikelihoods, factor_likelihood_numpy, factorLikelihood,  # noqa: F401
                         factorLikelihoodAll, likelihood_desc)
from .jointmodes import (FactorModeLikelihood, FactorModeLikelihoods, JointModes, JointSolution, MultihypoTerm,  # noqa: F401
                         factor_mode_likelihood_numpy, factorModeLikelihood, factorModeLikelihoodAll, joint_modes_from_tables,
                         jointModes)
from .overlap import (Overlap, Overlaps, beliefOverlap, findBeliefsNear, findOverlaps, findVariablesNear,  # noqa: F401
                      overlap_numpy, overlap_search_numpy, overlapVariables)
from .scene import Scene, scene_extent_numpy, scene_grid_numpy, sceneGrid  # noqa: F401
from .productgrid import ProductGrid, localProductGrid, localProductGridAll, product_grid_numpy  # noqa: F401
from .credible import (Credibility, CredibleRegion, coverage, credibility, credible_numpy, credibleRegion,  # noqa: F401
                       credibleRegionAll)
from .mixture import BeliefMixture, fitBeliefMixture, fitBeliefMixtureAll, mixture_numpy  # noqa: F401
from .heatmap import HeatmapGridDensity, LevelSetGridNormal, heatmap_density_numpy, sample  # noqa: F401
from .bayestree import (areCliqVariablesAllMarginalized, attemptTreeSimilarClique, buildTreeFromOrdering,  # noqa: F401
                        buildTreeReset, calcCliquesRecycled, getEliminationOrder, nestedDissectionOrder, setCliqueRecycling)
from .canonical import (generateChainEuclid, generateCircularDoors, generateGraph_Kaess,  # noqa: F401
                        generateGraph_LineStep, generateMixtureChain, generateSE2Lattice)
from .factorgraph import (AliasingScalarSampler, Circular, CircularCircular, ContinuousEuclid, ContinuousScalar,  # noqa: F401
                          EuclidDistance, LinearRelative, ManifoldFactor, ManifoldPrior, Mixture,
                          MsgPrior, MvNormal, Normal, PartialLinearRelative, PartialManifoldFactor, PartialPrior, PartialPriorPassThrough, Prior, Rayleigh, Uniform, PriorCircular, SolverParams,
                          SpecialEuclidean2, addFactor, addVariable, defaultFixedLagOnTree, deleteFactor, deleteVariable,
                          dontMarginalizeVariablesAll, fifoFreeze, getAddHistory, getSolverParams, initfg, isMarginalized,
                          isPartial, setMarginalized, setfreeze, unfreezeVariablesAll)
from .ppe import (MeanMaxPPE, calcPPE, getPPE, getPPEMax, getPPEMean, getPPESuggested, getPPESuggestedAll,  # noqa: F401
                  setPPE)
from .session import SolveSession  # noqa: F401
from .solver import (TreeProgram, approxConv, approxConvBelief, approxConvBeliefPath, approxDeconv, findShortestPath,  # noqa: F401
                     product_desc, proposal_desc,
                     initAll, initVariable, localProduct, localProductAndUpdate, manikde, propagateBelief,
                     setValKDE, solveTree)
