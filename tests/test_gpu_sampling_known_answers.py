"""-m gpu: the known answers of tests/sampling_cases.py for every random draw a proposal makes, on the HIP library (the same
cases run on the oracle in tests/test_sampling_known_answers.py).  Nothing here compares the kernels with the oracle: the
stream is held to a Philox4x32-10 written in Python, the draws to their distributions."""
import pytest

import sampling_cases as sc
from parity_utils import abi

MANIFOLDS = [abi.EUCLID1, abi.EUCLID2, abi.EUCLID3, abi.CIRCULAR, abi.SE2]
BELIEF_MANIFOLDS = [abi.EUCLID1, abi.EUCLID2, abi.CIRCULAR, abi.SE2]

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", sc.STREAM_N)
def test_stream_is_philox(hip_backend, N):
    assert sc.case_stream_is_philox(hip_backend, N) == ("ran" if 8 <= N <= abi.MAXN else "refused")


@pytest.mark.parametrize("manifold", MANIFOLDS)
def test_gaussian_measurement(hip_backend, manifold):
    sc.case_gaussian_measurement(hip_backend, manifold)


def test_uniform_and_rayleigh(hip_backend):
    sc.case_uniform_and_rayleigh(hip_backend)


def test_tabulated(hip_backend):
    sc.case_tabulated(hip_backend)


def test_mixture_labels(hip_backend):
    sc.case_mixture_labels(hip_backend)


def test_hypothesis_selection(hip_backend):
    sc.case_hypothesis_selection(hip_backend)


@pytest.mark.parametrize("manifold", MANIFOLDS)
def test_entropy_of_null_particles(hip_backend, manifold):
    sc.case_entropy_of_null_particles(hip_backend, manifold)


@pytest.mark.parametrize("manifold", BELIEF_MANIFOLDS)
def test_msgprior_draw(hip_backend, manifold):
    sc.case_msgprior_draw(hip_backend, manifold)


@pytest.mark.parametrize("manifold", BELIEF_MANIFOLDS)
def test_passthrough_topup(hip_backend, manifold):
    sc.case_passthrough_topup(hip_backend, manifold)


@pytest.mark.parametrize("manifold", BELIEF_MANIFOLDS)
def test_resample(hip_backend, manifold):
    sc.case_resample(hip_backend, manifold)


def test_kde_measurement_and_anyn(hip_backend):
    sc.case_kde_measurement_and_anyn(hip_backend)


def test_independence(hip_backend):
    sc.case_independence(hip_backend)
