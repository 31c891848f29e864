"""Every input of tests/test_gpu_mlp3.py is free of relu kinks: on it the float32 torch restatement of the train step
(oracle/elbo_torch.py) agrees with the float64 oracle to 1e-5 -- ten times inside the bound the GPU kernels are held to -- in the
loss and in every gradient leaf (relative to the leaf's max-abs).  A case that fails here would fail on any float32 kernel and says
nothing about fused_mlp3.hip: pick another seed for it in tests/mlp3_cases.py, never a wider bound there."""
import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from oracle import elbo_torch as T
from tests.gpu_util import random_problem
from tests.mlp3_cases import CASES, FENCE, case_id


@pytest.mark.parametrize("case", CASES + FENCE, ids=case_id)
def test_float32_restatement_agrees_with_the_oracle(case):
    cfg, dk, B, seed, _ = case
    p, x, z1, z2 = random_problem(cfg, dk, B, seed=seed)
    loss, g = O.loss_and_grad(cfg, p, x, z1, z2)
    m = T.TorchVAE(cfg, p, dtype=torch.float32)
    t32 = lambda a: torch.as_tensor(a, dtype=torch.float32)
    got, _, _ = m.elbo(t32(x), t32(z1), t32(z2))
    got.backward()
    got = got.detach()
    print(f"loss rel err {abs(float(got) - loss) / abs(loss):.3g}")
    assert abs(float(got) - loss) <= 1e-5 * abs(loss)
    worst = 0.0
    for name, grad in T.grads_tree(m).items():
        want = np.asarray(g[name], dtype=np.float64).reshape(grad.shape)
        err = float(np.max(np.abs(grad.astype(np.float64) - want)) / (np.max(np.abs(want)) + 1e-30))
        worst = max(worst, err)
        assert err <= 1e-5, (name, err)
    print(f"worst leaf rel err {worst:.3g}")
