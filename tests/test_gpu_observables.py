"""The table of observables (vae_training_amd/observables.py) end to end on the GPU: run.main in a fresh child process with every
observable flag of a model, against the same line without one -- for a linear sweep, a single linear model and an mlp3 sweep.  The
run with the flags trains bitwise as the run without; every observable key is there with one entry per n_print event."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# run.main with n_print = 4: five batches hold two n_print events, at batches 0 and 4
CHILD = """
import sys
from vae_training_amd import run
get_model = run.get_model
def short_schedule(*a, **kw):
    m = get_model(*a, **kw)
    m.n_print = 4
    return m
run.get_model = short_schedule
raise SystemExit(run.main(run.parse_arguments(sys.argv[1:])))
"""
EVENTS = 2
LINEAR = ["--dataset", "linear_gaussian", "-dd", "3", "-did", "3", "--padding_dim", "4", "--latent_dim", "6", "--layer_sizes", "",
          "--encoder_layer_sizes", ""]
LINEAR_FLAGS = ["--log_likelihood_samples", "8", "--exact_log_likelihood", "--elbo_hessian", "4", "--eigenvalues", "--subspace", "auto"]
LINEAR_KEYS = ["Average Log Likelihood", "ELBO estimate", "Effective Sample Size",
               "Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning", "IWAE Gap",
               "ELBO Hessian Ritz Values", "ELBO Hessian Ritz Residuals", "Sharpness", "ELBO Hessian Min Ritz", "ELBO Gradient Norm",
               "learnt eigenvalue", "ground truth eigenvalue", "Principal Angles", "Subspace Distance"]
MLP3 = ["--dataset", "sphere", "-dd", "3", "--padding_dim", "3", "--latent_dim", "6", "--layer_sizes", "200|200|200",
        "--encoder_layer_sizes", "200|200|200", "--epsilon", "-3", "-tdv"]
MLP3_FLAGS = ["--mlp_log_likelihood_samples", "8", "--decoder_jacobian", "prior"]
MLP3_KEYS = ["Average Log Likelihood", "ELBO estimate", "Effective Sample Size",
             "Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"]
SWEEP = ["--sweep_dataset_seeds", "69,24"]
CASES = {"linear_sweep": (LINEAR + SWEEP, LINEAR_FLAGS, LINEAR_KEYS, ["_ds69", "_ds24"]),
         "linear_single": (LINEAR, LINEAR_FLAGS, LINEAR_KEYS, [""]),
         "mlp3_sweep": (MLP3 + SWEEP, MLP3_FLAGS, MLP3_KEYS, ["_ds69", "_ds24"])}


@pytest.mark.parametrize("case", list(CASES))
def test_run_py_with_every_observable_flag_trains_as_the_run_without(tmp_path, case):
    line, flags, keys, suffixes = CASES[case]
    out = {}
    for name, extra in (("plain", []), ("flags", flags)):
        cmd = [sys.executable, "-c", CHILD, name, *line, "--batch_size", "100", "--num_batches", "5", "-ow", *extra]
        r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.count("Batch | 4 |") == len(suffixes), r.stdout[-2000:]
        out[name] = [dict(np.load(os.path.join(str(tmp_path), "data", name + s, "losses.npz"), allow_pickle=True)) for s in suffixes]
    for plain, flagged in zip(out["plain"], out["flags"]):
        for k in ("VAE Loss", "KL divergence", "mse"):                    # VAE Loss: the two events' losses, then the five train losses
            a, b = np.asarray(plain[k]), np.asarray(flagged[k])
            assert a.size >= EVENTS and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        assert np.asarray(plain["VAE Loss"]).size == EVENTS + 5
        for k in keys:
            assert k in flagged and len(flagged[k]) == EVENTS, (k, len(flagged.get(k, ())))
        assert not any(k in plain for k in keys if k != "Average Log Likelihood")
        assert sorted(k for k in flagged if k not in keys + ["EigenValues"]) == sorted(k for k in plain if k != "Average Log Likelihood")
