"""How well the float64 reference of tests/test_gpu_linear_jacobian.py is defined, from that reference ALONE (no GPU, no kernel): run
it before any run of the kernel.

J(z) = K_d^T + diag(sigmoid'(z K_s + b_s)) K_s^T of a linear VAE is smooth in z: there are no kinks to stay away from.  What limits the
comparison is float64 itself.  Per case of tests/linear_jacobian_cases.py this measures:
  (i)  worst: the worst |G_64 - G_ld|_F / |G_64|_F over rows and replicas of G = J^T J evaluated in float64 against the same formula in
       numpy.longdouble (refused where longdouble's eps is not below 2^-60: there it measures nothing).  The GPU bound per row is
       (2^-43 + GRAM_FACTOR x worst + 64 L 2^-53) |G_ref|_F with the case's own `worst`;
  (ii) whether any lambda_k / lambda_1 lies in [rank_tol / 2, 2 rank_tol]: such a case gets another seed or rank_tol (--search).

    python tools/linear_jacobian_reference.py            # prints the table and writes it between the markers of the GPU test file
    python tools/linear_jacobian_reference.py --search   # writes SEEDS / RANK_TOLS between the markers of tests/linear_jacobian_cases.py"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import linear_jacobian_cases as LC  # noqa: E402
from tools.decoder_jacobian_reference import free_tol  # noqa: E402

TEST_FILE = os.path.join(ROOT, "tests", "test_gpu_linear_jacobian.py")
CASES_FILE = os.path.join(ROOT, "tests", "linear_jacobian_cases.py")
BEGIN, END = "# LINEAR_JACOBIAN_TABLE_BEGIN", "# LINEAR_JACOBIAN_TABLE_END"
S_BEGIN, S_END = "# SEARCH_BEGIN", "# SEARCH_END"
MAX_SEEDS = 64


def check_longdouble():
    eps = float(np.finfo(np.longdouble).eps)
    if not eps < 2.0 ** -60:
        raise SystemExit(f"numpy.longdouble has eps = {eps:.3e} here, not below 2^-60: it cannot measure float64's error")


def _replace(path, begin, end, text):
    src = open(path).read()
    new = re.sub(re.escape(begin) + r".*?" + re.escape(end), lambda _: text, src, flags=re.S)
    if new != src:
        open(path, "w").write(new)


def search():
    seeds, tols = {}, {}
    for case in LC.CASES:
        seed, tol = LC.DEFAULT_SEED, None
        while tol is None:
            tol = free_tol(LC.ratios64(case, seed=seed))
            if tol is None:
                seed += 1
                if seed - LC.DEFAULT_SEED >= MAX_SEEDS:
                    raise SystemExit(f"{case}: no seed of {MAX_SEEDS} leaves a rank threshold free")
        if seed != LC.DEFAULT_SEED:
            seeds[case] = seed
        if tol != LC.RANK_TOL:
            tols[case] = tol
        print(f"# {case}: seed {seed}, rank_tol {tol:g}", flush=True)
    text = "\n".join([f"{S_BEGIN} (written by tools/linear_jacobian_reference.py --search)",
                      "SEEDS = {" + "".join(f"\n    {c!r}: {s}," for c, s in seeds.items()) + "\n}",
                      "RANK_TOLS = {" + "".join(f"\n    {c!r}: {t!r}," for c, t in tols.items()) + "\n}", S_END])
    print(text)
    _replace(CASES_FILE, S_BEGIN, S_END, text)


def table_text():
    rows, worst = [], 0.0
    for case in LC.CASES:
        m = LC.measure(case)
        worst = max(worst, m["gram"])
        u = "" if m["u_min"] is None else f"  |u| in [{m['u_min']:.1e}, {m['u_max']:.1e}]"
        print(f"{case[0]:15s} rows {case[1]:3d}: worst {m['gram']:.2e}  ratio near tol: {m['ratio_hit']}{u}  "
              f"{'UNUSABLE' if m['ratio_hit'] else ''}")
        rows.append(f"    {case!r}: {m['gram']:.3e},")
    return "\n".join([f"{BEGIN} (written by tools/linear_jacobian_reference.py: per case the worst |G_64 - G_longdouble|_F / |G|_F)",
                      "TABLE = {", *rows, "}", f"GRAM_WORST = {worst:.3e}", END])


def main():
    check_longdouble()
    if "--search" in sys.argv:
        return search()
    text = table_text()
    print(text)
    if os.path.exists(TEST_FILE):
        _replace(TEST_FILE, BEGIN, END, text)


if __name__ == "__main__":
    main()
