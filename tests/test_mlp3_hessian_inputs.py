"""The inputs of the MLP sampled-ELBO-Hessian tests are usable, from the CPU alone: no hidden pre-activation of the float64 reference
lies near a relu kink, and the breakdown case breaks down."""
import numpy as np
import pytest

from tests import mlp3_hessian_cases as K


@pytest.mark.parametrize("case", K.ALL_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_no_pre_activation_is_near_the_kink(case):
    """A condition, not a measurement: with every |pre-activation| >= 1e-9 two float64 evaluations in different summation orders
    (error ~1e-13 at these magnitudes) agree on every mask.  A case that fails gets another seed in K.SEEDS."""
    worst = min(K.model(case, r).min_abs_pre() for r in range(K.R))
    print(f"{case}: smallest |pre-activation| over all hidden units, columns and replicas {worst:.3e}")
    assert worst >= K.MIN_PRE


def test_the_breakdown_case_breaks_down_on_the_cpu():
    """One column of `narrow` from a random start runs all 32 steps; from breakdown_start (the weights of Decoder/FC1 units dead in that
    column) H v0 = 0 exactly and the run ends at k = 1."""
    case = K.BREAKDOWN_CASE
    assert case == ("narrow", 1, 1)
    rnd = K.ref().lanczos(K.model(case).hvp, K.start_vector(case[0]), 32)
    assert rnd["k"] == 32 and rnd["beta"][-1] > 2.0 ** -40 * np.max(np.abs(rnd["alpha"]))
    for r in range(K.R):
        v0 = K.breakdown_start(case, r)
        assert np.count_nonzero(v0) >= 65 and not np.any(K.model(case, r).hvp(v0))
        run = K.ref().lanczos(K.model(case, r).hvp, v0, 32)
        assert run["k"] == 1 < 32 and run["alpha"][0] == 0.0 and run["beta"][0] == 0.0 and run["theta"].tolist() == [0.0]
