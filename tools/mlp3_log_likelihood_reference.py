"""How well the float64 reference of tests/test_gpu_mlp3_log_likelihood.py is defined, from that reference ALONE (no GPU, no kernel).

The device draws its normals and rows with a Box-Muller within 5e-6 of float64 (tests/test_rng.py), so the float64 evaluation "on the same
draws" is an evaluation on inputs that distance away.  For every (shape, rows, K) of the test, with the test's parameters, this moves
every row element and every normal by +-5e-6 (random signs, three trials) and prints the largest relative move of the three record
slots.  A case whose reference moves by more than a fifth of its bound cannot be held to that bound -- it would test the perturbation
--; the test holds such a case to five times its own reference's move instead (DROPPED, with the moves).
The rows are the oracle datasets' (the device rows need the GPU; the distribution is the same).

    python tools/mlp3_log_likelihood_reference.py        # prints a table, then the REFERENCE_MOVES / DROPPED block for the test"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import elbo_oracle as O  # noqa: E402
from tests import test_gpu_mlp3_log_likelihood as T  # noqa: E402

DIST = 5e-6
KIND = {0: "linear_gaussian", 1: "sigmoid", 2: "sphere"}


def main():
    moves, dropped = {}, []
    for name, s in T.SHAPES.items():
        cfg = T._cfg(s)
        trees = [O.unflatten(cfg, f.astype(np.float64)) for f in T.make_flats(name)]
        seeds, steps = [2 ** 64 - 3, 991, 31337], [3, 2 ** 32 - 1, 2]
        for K in T.KS:
            worst = {rows: np.zeros(3) for rows in T.ROWS}
            for r in range(T.R):
                _, sampler = O.make_dataset(KIND[s["kind"]], seed=100 + r, dd=s["dd"], did=s["did"], pad=s["pad"], var_added=s["var"])
                rng = np.random.default_rng(7 + r)
                x = np.asarray(sampler(rng, T.MAXR), np.float32).astype(np.float64)
                xi = T.xi64(seeds[r], steps[r], T.Z_TAG, T.MAXR, K, s["L"])
                base, _ = T.rows64(s, trees[r], x, xi)
                for _ in range(3):
                    moved, _ = T.rows64(s, trees[r], x + DIST * rng.choice([-1.0, 1.0], x.shape), xi + DIST * rng.choice([-1.0, 1.0], xi.shape))
                    for rows in T.ROWS:
                        a, b = base[:rows].mean(0), moved[:rows].mean(0)
                        worst[rows] = np.maximum(worst[rows], np.abs(a - b) / np.abs(a))
            for rows in T.ROWS:
                w = worst[rows]
                bound2 = 1e-4 if rows == 1 else 1e-5
                keep = w[0] <= 2e-6 and w[1] <= 2e-6 and w[2] <= bound2 / 5
                print(f"{name:9s} rows {rows:4d} K {K:3d}: reference moves {w[0]:.1e} {w[1]:.1e} {w[2]:.1e}  {'' if keep else 'DROPPED'}")
                key = ("rows 1" if rows == 1 else "rows >= 16")
                moves[key] = np.maximum(moves.get(key, np.zeros(3)), w)
                if not keep:
                    dropped.append(((name, rows, K), w))
    print("REFERENCE_MOVES = {")
    for k, w in moves.items():
        print(f'    "{k}": ({w[0]:.1e}, {w[1]:.1e}, {w[2]:.1e}),')
    print("}")
    print("DROPPED = {" + "".join(f"\n    {d!r}: ({w[0]:.1e}, {w[1]:.1e}, {w[2]:.1e})," for d, w in dropped) + ("\n" if dropped else "") + "}")


if __name__ == "__main__":
    main()
