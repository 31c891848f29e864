"""How well float32 can meet the bounds of tests/test_gpu_mlp3_stats_event.py, from the CPU ALONE (no GPU, no kernel).

For every (shape, rows) case of the test, with the test's parameters, dataset matrices and sample_eps, rows from the oracle's own
datasets (the device rows need the GPU; the distribution is the same) and latents from oracle/philox.py under the test's seeds and
steps, this evaluates the record in float64 (record64) and as a float32 NumPy restatement (record32: every per-element operation in
float32, every sum over rows in float64, as the kernel takes them) and prints the distance per slot in the unit of the slot's bound:
slots 0 .. 2 relative to |loss| (bound 1e-5), eps absolute (1e-6), each score relative to its own value (1e-5).  epsilon_p is a copy.
A (case, slot) further than a fifth of its bound is written into the LOOSE table of the test, which holds it to the larger of the
bound and five times the printed distance -- the rule of tests/test_gpu_mlp3_log_likelihood.py.  No case is left out.

    python tools/mlp3_stats_event_reference.py        # prints a table, then the LOOSE block for the test"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import elbo_oracle as O  # noqa: E402
from tests import test_gpu_mlp3_log_likelihood as LL  # noqa: E402
from tests import test_gpu_mlp3_stats_event as T  # noqa: E402

KIND = {0: "linear_gaussian", 1: "sigmoid", 2: "sphere"}


def main():
    loose, worst_all = {}, np.zeros(len(T.SLOTS))
    for name, s in T.SHAPES.items():
        cfg = LL._cfg(s)
        flats = LL.make_flats(name)
        trees = [O.unflatten(cfg, f.astype(np.float64)) for f in flats]
        alen = {0: s["dd"] * s["did"], 1: s["dd"], 2: 0}[s["kind"]]
        A = np.asarray(np.random.default_rng(29).standard_normal((T.R, alen)), np.float32).astype(np.float64) if alen else None      # the test's
        maxr = max(T.ROWS)
        draws = []
        for r in range(T.R):
            _, sampler = O.make_dataset(KIND[s["kind"]], seed=100 + r, dd=s["dd"], did=s["did"], pad=s["pad"], var_added=s["var"])
            x = np.asarray(sampler(np.random.default_rng(7 + r), maxr), np.float32).astype(np.float64)
            z = np.asarray(LL.xi64(T.Z_SEEDS[r], T.Z_STEPS[r], T.Z_TAG, maxr, 1, s["L"] + s["D"])[:, 0, :], np.float32).astype(np.float64)
            draws.append((x, z[:, :s["L"]], z[:, s["L"]:]))
        for rows in T.ROWS:
            worst, eps_worst = np.zeros(len(T.SLOTS)), 0.0
            for r in range(T.R):
                x, z1, z2 = (t[:rows] for t in draws[r])
                Ar = None if A is None else A[r]
                a = T.record64(s, trees[r], Ar, x, z1, z2, T.SAMPLE_EPS[r])
                b = T.record32(s, trees[r], Ar, x, z1, z2, T.SAMPLE_EPS[r])
                d, e = T.distances(s, b, a)
                worst[:len(d)] = np.maximum(worst[:len(d)], d)
                eps_worst = max(eps_worst, e)
            base = (T.LOSS_RTOL,) * 3 + (T.SCORE_RTOL,) * 2
            far = {k: float(f"{v:.1e}") for k, v, b in zip(T.SLOTS, worst, base) if v > b / 5}
            print(f"{name:9s} rows {rows:4d}: " + " ".join(f"{k} {v:.1e}" for k, v in zip(T.SLOTS, worst)) + f" eps {eps_worst:.1e}" +
                  (f"  LOOSE {sorted(far)}" if far else ""))
            assert eps_worst <= T.EPS_ATOL / 5, "eps is one float32 product: it cannot be far"
            worst_all = np.maximum(worst_all, worst)
            if far:
                loose[(name, rows)] = far
    print("largest distance per slot over all cases: " + " ".join(f"{k} {v:.1e}" for k, v in zip(T.SLOTS, worst_all)))
    print("LOOSE = {" + "".join(f"\n    {k!r}: {v!r}," for k, v in loose.items()) + ("\n" if loose else "") + "}")


if __name__ == "__main__":
    main()
