"""Replay of linear_jacobian_rows' arithmetic on the CPU, one rounding per device operation (no GPU, no kernel): what the slope's
rounding does to |G|_F.  It is where the figures in DESIGN 3.26 and below TABLE in tests/test_gpu_linear_jacobian.py come from.

Every operation of the kernel from u to |G|_F is done in float64 with the kernel's order of operations; an fma is ONE rounding of the
exact a b + c (fractions.Fraction).  u is the reference's bit for bit (products of two float32 values are exact in float64, the sums
run in l order).  Only exp is not the device's: it is NumPy's here, so every figure is given three times, with exp's result as it is
and moved one ulp up and down -- a figure that stays put does not hang on whose exp it is.  Two forms of the slope:
  plain    g = e / ((1 + e) (1 + e)), three roundings after exp;
  once     1 + e = th + tl exactly, (1 + e)^2 = ph + pl by one fma, q = e / ph corrected once by its residual: the kernel's text.
Per case and replica: the bound on |G|_F (GRAM_FACTOR x the case's worst |G_64 - G_longdouble|_F / |G|_F, measured here as
tools/linear_jacobian_reference.py measures it), and each form's worst distance over the rows from the float64 reference and from the
long double evaluation, relative to |G_ref|_F.  At L = 1 this is the kernel's |G|_F operation for operation (the device printed the
same 4.14e-16 and 1.38e-16 on ('sig_one_latent', 1), replica 1); at L > 1 the squares of G's entries are added here in index order, in
the kernel over a block tree, so those figures can differ from the device's in the last ulp.  It also counts the heads on which `once` is not the correctly rounded quotient.

    python tools/replay_linear_jacobian_slope.py                      # the L = 1 shape, seconds
    python tools/replay_linear_jacobian_slope.py sig_script1 sig_odd  # other two-decoder shapes (L = 24 and 32 take minutes)"""
import os
import sys
from fractions import Fraction as F

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import linear_jacobian_cases as LC  # noqa: E402
from tools.linear_jacobian_reference import check_longdouble  # noqa: E402


def fma(a, b, c):
    return float(F(a) * F(b) + F(c))


def slope(e, form, stats):
    if form == "plain":
        t = 1.0 + e
        return e / (t * t)
    th = 1.0 + e
    tl = e - (th - 1.0)
    ph = th * th
    pl = fma(th, th, -ph) + 2.0 * th * tl
    q = e / ph
    g = q + (fma(-q, ph, e) - q * pl) / ph
    t = F(1) + F(e)
    stats["heads"] += 1
    stats["not_correctly_rounded"] += g != float(F(e) / (t * t))
    return g


def replay_norm_g(p, z, form, shift, stats):
    """|G|_F per row as the kernel forms it, exp's result moved by `shift` ulp."""
    Kd = np.asarray(p["Decoder/FC0/kernel"], np.float64)
    Ks = np.asarray(p["SigDecoder/FC0/kernel"], np.float64)
    bs = np.asarray(p["SigDecoder/FC0/bias"], np.float64)
    L, D = Kd.shape
    out = np.zeros(z.shape[0])
    for row in range(z.shape[0]):
        J = np.zeros((L, D))
        for d in range(D):
            u = bs[d]
            for l in range(L):
                u = u + float(z[row, l]) * Ks[l, d]              # exact product: an fma and a plain sum agree
            e = float(np.exp(-abs(u)))
            if shift and e > 0.0:
                e = float(np.nextafter(e, 2.0 if shift > 0 else -1.0))
            g = slope(e, form, stats)
            for l in range(L):
                J[l, d] = fma(g, Ks[l, d], Kd[l, d])
        sq = 0.0                                                 # the kernel adds these over a block tree; at L = 1 there is one term
        for i in range(L):
            for j in range(i, L):
                v = 0.0
                for d in range(D):
                    v = fma(J[i, d], J[j, d], v)
                sq += v * v if i == j else 2.0 * v * v
        out[row] = np.sqrt(sq)
    return out


def main(names):
    check_longdouble()
    for name in names:
        if not LC.SHAPES[name]["sig"]:
            raise SystemExit(f"{name}: one decoder, J has no slope in it")
        for rows in LC.ROWS[name]:
            case = (name, rows)
            z = LC.case_latents(case)
            bound = LC.GRAM_FACTOR * LC.measure(case)["gram"]
            print(f"{case}: bound on |G|_F {bound:.3e} |G|")
            stats = dict(heads=0, not_correctly_rounded=0)
            for r, p in enumerate(LC.trees_of(name)):
                ng = LC.row_records64(LC.jacobian64(p, z[r])[0], LC.case_tol(case))[3]
                Gld = LC.gram(LC.jacobian(p, z[r], np.longdouble)[0])
                ngld = np.sqrt(np.square(Gld).sum((1, 2)))
                for form in ("plain", "once"):
                    cells = []
                    for shift in (0, 1, -1):
                        k = replay_norm_g(p, z[r], form, shift, stats)
                        ref = float((np.abs(k - ng) / ng).max())
                        ld = float((np.abs(k - ngld) / ng).max())
                        cells.append(f"exp{shift:+d}: {ref:.2e} / {ld:.2e}{'  MISSES' if ref > bound else ''}")
                    print(f"  replica {r} {form:5s} from float64 / from long double   " + "   ".join(cells))
            print(f"  once: {stats['not_correctly_rounded']} of {stats['heads']} slopes differ from the correctly rounded quotient")


if __name__ == "__main__":
    main(sys.argv[1:] or ["sig_one_latent"])
