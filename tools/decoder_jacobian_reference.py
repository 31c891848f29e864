"""What the float64 reference of tests/test_gpu_decoder_jacobian.py resolves, from that reference and a float32 emulation ALONE (no GPU,
no kernel): run it before any run of the kernel.

J(z) of a relu decoder is piecewise constant in the masks, so a hidden pre-activation that float32 and float64 put on different sides
of 0 moves J by a whole column, whatever kernel computes it.  Per case of tests/decoder_jacobian_cases.py this measures, against the
float64 reference:
  (i)   dist: the worst distance of a float32 forward with sequential k-order accumulation from float64 on any hidden pre-activation,
        and min_pre: the case's smallest |pre|.  A case is usable only if min_pre >= KINK_FACTOR x dist (8: the order inside an MFMA
        k-step is not the emulation's).  No row is left out of any comparison: a case that fails gets another seed (--search).
  (ii)  gram: the worst |G32 - G64|_F / |G64|_F of the same emulation carried through the tangents; GRAM_RTOL = GRAM_FACTOR x the worst
        over all cases.
  (iii) whether any lambda_k / lambda_1 lies in [rank_tol / 2, 2 rank_tol]: such a case gets another rank_tol (--search).

    python tools/decoder_jacobian_reference.py            # prints the table and writes it between the markers of the GPU test file
    python tools/decoder_jacobian_reference.py --search   # prints SEEDS / RANK_TOLS for tests/decoder_jacobian_cases.py"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import decoder_jacobian_cases as DC  # noqa: E402

TEST_FILE = os.path.join(ROOT, "tests", "test_gpu_decoder_jacobian.py")
BEGIN, END = "# JACOBIAN_TABLE_BEGIN", "# JACOBIAN_TABLE_END"
TOLS = (1e-4, 1e-3, 1e-2, 3e-4, 3e-3, 3e-2, 1e-5, 0.1)      # --search takes the first that no eigenvalue ratio comes near


def usable(m):
    return m["min_pre"] >= DC.KINK_FACTOR * m["dist"]


def free_tol(ratios):
    """The first of TOLS with no ratio in [tol / 2, 2 tol]; else the middle of the widest gap of the sorted ratios where that gap is
    wider than the window (a factor above 4.4), to two digits; else None."""
    ratios = ratios[ratios > 0]
    free = lambda t: not ((ratios >= t / 2) & (ratios <= 2 * t)).any()
    for t in TOLS:
        if free(t):
            return t
    if ratios.size > 1:
        g = ratios[1:] / ratios[:-1]
        i = int(g.argmax())
        t = float(f"{(ratios[i] * ratios[i + 1]) ** 0.5:.1e}")
        if g[i] > 4.4 and free(t):
            return t
    return None


def search():
    seeds, tols = {}, {}
    for case in DC.CASES:
        seed, tol = DC.DEFAULT_SEED, None
        while tol is None:
            if usable(DC.measure(case, seed=seed, tol=DC.RANK_TOL)):
                tol = free_tol(DC.ratios64(case, seed=seed))
            if tol is None:
                seed += 1
        if seed != DC.DEFAULT_SEED:
            seeds[case] = seed
        if tol != DC.RANK_TOL:
            tols[case] = tol
        print(f"# {case}: seed {seed}, rank_tol {tol:g}", flush=True)
    print("SEEDS = {" + "".join(f"\n    {c!r}: {s}," for c, s in seeds.items()) + "\n}")
    print("RANK_TOLS = {" + "".join(f"\n    {c!r}: {t!r}," for c, t in tols.items()) + "\n}")


def table_text():
    rows, worst = [], 0.0
    for case in DC.CASES:
        m = DC.measure(case)
        ok = usable(m) and not m["ratio_hit"]
        worst = max(worst, m["gram"])
        print(f"{case[0]:10s} rows {case[1]:3d}: dist {m['dist']:.2e}  min |pre| {m['min_pre']:.2e}  gram {m['gram']:.2e}  "
              f"ratio near tol: {m['ratio_hit']}  {'' if ok else 'UNUSABLE'}")
        rows.append(f"    {case!r}: ({m['dist']:.3e}, {m['min_pre']:.3e}, {m['gram']:.3e}),")
    return "\n".join([f"{BEGIN} (written by tools/decoder_jacobian_reference.py: per case (dist, min |pre|, gram) of its docstring)",
                      "TABLE = {", *rows, "}", f"GRAM_WORST = {worst:.3e}", END])


def main():
    if "--search" in sys.argv:
        return search()
    text = table_text()
    print(text)
    if os.path.exists(TEST_FILE):
        src = open(TEST_FILE).read()
        new = re.sub(re.escape(BEGIN) + r".*?" + re.escape(END), lambda _: text, src, flags=re.S)
        if new != src:
            open(TEST_FILE, "w").write(new)


if __name__ == "__main__":
    main()
