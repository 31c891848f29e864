"""No GPU: every case of tests/test_gpu_decoder_jacobian.py is one the float64 reference defines (tests/decoder_jacobian_cases.py,
tools/decoder_jacobian_reference.py).  Per case, recomputed here from the float64 reference and the float32 emulation alone:
  (i)   the smallest hidden |pre| is at least KINK_FACTOR = 8 times the worst distance of the float32 forward from float64 -- no row of
        any case sits where float32 and float64 could disagree on a relu mask;
  (iii) no lambda_k / lambda_1 lies in [rank_tol / 2, 2 rank_tol] -- the rank the GPU test asks for exactly is not a coin toss;
and the figures are the ones the GPU test file's TABLE holds (so GRAM_RTOL there is 8 x the worst measured error of G)."""
import ast
import os
import re

import pytest

from tests import decoder_jacobian_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    """TABLE and GRAM_WORST of the GPU test file, read as text (the module itself needs nothing of the GPU, but it is the GPU suite's)."""
    src = open(os.path.join(ROOT, "tests", "test_gpu_decoder_jacobian.py")).read()
    block = re.search(r"# JACOBIAN_TABLE_BEGIN.*?\n(.*?)# JACOBIAN_TABLE_END", src, flags=re.S).group(1)
    ns = {}
    for node in ast.parse(block).body:
        ns[node.targets[0].id] = ast.literal_eval(node.value)
    return ns["TABLE"], ns["GRAM_WORST"]


def test_the_table_covers_the_cases_and_sets_the_gram_tolerance():
    table, worst = _table()
    assert list(table) == DC.CASES and len(DC.CASES) == 18
    assert worst == max(v[2] for v in table.values()) and 0 < DC.GRAM_FACTOR * worst < 1e-4
    for name, s in DC.SHAPES.items():                     # a single row, a full tile and a partial last tile where a tile has rows to spare
        rpt = 64 // (s["L"] + 1)
        rows = DC.ROWS[name]
        assert 1 in rows and any(r >= rpt for r in rows) and (rpt == 1 or any(r % rpt for r in rows if r > rpt))
    for case in DC.CASES:
        assert 0.0 <= DC.case_tol(case) < 0.5


@pytest.mark.parametrize("case", DC.CASES, ids=[f"{n}-rows{r}" for n, r in DC.CASES])
def test_a_case_is_defined_by_its_reference(case):
    table, _ = _table()
    m = DC.measure(case)
    dist, min_pre, gram = table[case]
    print(case, m)
    assert m["min_pre"] >= DC.KINK_FACTOR * m["dist"], (case, m)          # (i)
    assert not m["ratio_hit"], (case, DC.case_tol(case))                  # (iii)
    for got, want in ((m["dist"], dist), (m["min_pre"], min_pre), (m["gram"], gram)):      # the table's three digits; the float64 side goes through BLAS
        assert abs(got - want) <= 2e-3 * want, (case, got, want)
