"""No GPU: every case of tests/test_gpu_linear_jacobian.py is one the float64 reference defines (tests/linear_jacobian_cases.py,
tools/linear_jacobian_reference.py).  Per case, recomputed here from the float64 and long-double evaluations alone:
  (i)  `worst`, the distance of the float64 G from the long-double one, is the figure the GPU test file's TABLE holds.  It is rounding
       noise itself -- a few units of 2^-53, and exp may differ by an ulp between two builds of NumPy -- so it is compared within a
       factor of 2, and bounded: GRAM_FACTOR x worst stays below 2^-43, the solver's own stopping rule;
  (ii) no lambda_k / lambda_1 lies in [rank_tol / 2, 2 rank_tol] -- the rank the GPU test asks for exactly is not a coin toss;
and the cases are the ones the issue lists, with u reaching both the linear and the flat part of the sigmoid."""
import ast
import os
import re

import numpy as np
import pytest

from tests import linear_jacobian_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    """TABLE and GRAM_WORST of the GPU test file, read as text (the module itself needs nothing of the GPU, but it is the GPU suite's)."""
    src = open(os.path.join(ROOT, "tests", "test_gpu_linear_jacobian.py")).read()
    block = re.search(r"# LINEAR_JACOBIAN_TABLE_BEGIN.*?\n(.*?)# LINEAR_JACOBIAN_TABLE_END", src, flags=re.S).group(1)
    ns = {}
    for node in ast.parse(block).body:
        ns[node.targets[0].id] = ast.literal_eval(node.value)
    return ns["TABLE"], ns["GRAM_WORST"]


def test_long_double_can_measure_float64():
    assert float(np.finfo(np.longdouble).eps) < 2.0 ** -60


def test_the_table_covers_the_cases():
    table, worst = _table()
    assert list(table) == LC.CASES and len(LC.CASES) == 25
    assert worst == max(table.values()) and 0 < LC.GRAM_FACTOR * worst < 2.0 ** -43
    shapes = {(s["D"], s["L"], s["sig"]) for s in LC.SHAPES.values()}
    assert shapes == {(7, 6, True), (28, 24, True), (5, 32, True), (9, 1, True), (11, 13, True), (12, 20, False), (32, 32, False),
                      (32, 3, False)}
    for name in LC.SHAPES:
        assert LC.ROWS[name][:3] == (1, 2, 37)
    assert LC.ROWS["sig_script1"] == (1, 2, 37, 257) and LC.R == 3
    for case in LC.CASES:
        assert 0.0 <= LC.case_tol(case) < 0.5
    # the parameters follow the layout the kernel reads: encoder [D][L] + [L], K_d [L][D], b_d, K_s [L][D], b_s, epsilon_p, epsilon
    for name, s in LC.SHAPES.items():
        D, L = s["D"], s["L"]
        flats = LC.make_flats(name)
        assert len(flats) == 3 and flats[0].dtype == np.float32
        assert flats[0].size == D * L + L + (2 if s["sig"] else 1) * (L * D + D) + L + 1
        p = LC.trees_of(name)[0]
        off = D * L + L
        assert (p["Decoder/FC0/kernel"].ravel() == flats[0][off:off + L * D]).all()
        if s["sig"]:
            off += L * D + D
            assert (p["SigDecoder/FC0/kernel"].ravel() == flats[0][off:off + L * D]).all()
            assert (p["SigDecoder/FC0/bias"] == flats[0][off + L * D:off + L * D + D]).all()


@pytest.mark.parametrize("case", LC.CASES, ids=[f"{n}-rows{r}" for n, r in LC.CASES])
def test_a_case_is_defined_by_its_reference(case):
    table, _ = _table()
    m = LC.measure(case)
    print(case, m)
    assert not m["ratio_hit"], (case, LC.case_tol(case))                  # (ii)
    assert 0 < m["gram"] <= 2 * table[case] and table[case] <= 2 * m["gram"], (case, m["gram"], table[case])      # (i)
    if LC.SHAPES[case[0]]["sig"] and case[1] >= 37:       # both regimes of the sigmoid among the rows' heads
        assert m["u_min"] < 0.5 and m["u_max"] > 6.0, (case, m)


def test_the_reference_is_the_derivative_of_the_oracle_decoder():
    """J of the reference against central differences of oracle.forward's x_hat in z (sampling: mu = 0, so samples = z1), and the
    kernel's e / (1 + e)^2 form of the slope against the reference's s (1 - s)."""
    from oracle import elbo_oracle as O
    for name in ("sig_script1", "lin_narrow"):
        s = LC.SHAPES[name]
        cfg = LC.cfg_of(s)
        p = LC.trees_of(name)[0]
        z = LC.case_latents((name, 2))[0].astype(np.float64)
        J, u = LC.jacobian64(p, z)
        h = 1e-6
        for l in range(s["L"]):
            dz = np.zeros_like(z)
            dz[:, l] = h
            xs = []
            for zz in (z + dz, z - dz):
                xh = O.fcn_forward(p, "Decoder", zz, cfg.dec_sizes)[0]
                if cfg.sigmoid:
                    xh = xh + O.fcn_forward(p, "SigDecoder", zz, cfg.dec_sizes, if_sigmoid=True)[0]
                xs.append(xh)
            fd = (xs[0] - xs[1]) / (2 * h)
            assert np.abs(fd - J[:, :, l]).max() <= 1e-8 * max(1.0, np.abs(J).max()), (name, l)
        if u is not None:
            e = np.exp(-np.abs(u))
            sg = 1.0 / (1.0 + np.exp(-u))
            assert np.abs(e / ((1 + e) * (1 + e)) - sg * (1 - sg)).max() <= 4 * 2.0 ** -53
    for big in (745.2, 800.0, 1e6):
        e = np.exp(-np.abs(np.float64(big)))
        assert e / ((1 + e) * (1 + e)) == 0.0
