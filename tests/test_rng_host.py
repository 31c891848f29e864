"""The batch generator's references and bounds, on the host (tests/rng_cases.py has the cases, the bounds and their reasons): the
tail counters where u1 rounded to 1, the float32 uniforms the kernel forms, how far the ideal and the kernel-uniform Box-Muller are
apart and why, and a float32 emulation of csrc/rng_dev.h that stays inside every per-element bound at the reference's own error."""
import numpy as np
import pytest

from oracle import philox as P
from tests import rng_cases as RC


def _pairs(k, w2):
    """Philox words [n, 2] with w >> 8 = k in the u1 word and w2 in the u2 word."""
    return np.stack([(np.asarray(k, np.uint64) << np.uint64(8)).astype(np.uint32), np.asarray(w2, np.uint32)], axis=-1)


def _random_words(blocks, key=(7, 9)):
    ctr = np.zeros((blocks, 4), dtype=np.uint32); ctr[:, 0] = np.arange(blocks)
    return P.philox4x32(ctr, key)


@pytest.mark.parametrize("row,word,want", RC.TAIL_ROWS)
def test_tail_counters_give_the_stated_words(row, word, want):
    """Key (77, 0), step 0, tag 0, block 0 of these rows: a pair whose 24 bits are all ones."""
    got = [int(v) for v in P.stream_bits(RC.TAIL_SEED, 0, 0, row, 1, 0, 1).reshape(4)]
    assert all(w is None or g == w for g, w in zip(got, want)), [hex(g) for g in got]
    assert got[word] >> 8 == 2 ** 24 - 1
    u1, _ = P.kernel_uniforms(np.array(got, dtype=np.uint32))
    assert u1[word // 2] == P.U1_MAX
    n = P.normals_kernel_uniform(np.array(got, dtype=np.uint32))
    assert 3.4e-4 < np.hypot(n[word], n[word + 1]) < 3.5e-4                 # the smallest r: sqrt(-2 ln(1 - 2^-24)) = 3.45e-4


def test_kernel_uniforms_stay_inside_their_ranges():
    top = 2 ** 24 - 1
    u1, u2 = P.kernel_uniforms(_pairs([top, top - 1, top - 2, 2 ** 23 + 1, 2 ** 23 - 1, 1, 0], [0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F, 0, 1, 2, 3]))
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert np.float32(top) + np.float32(0.5) == np.float32(2 ** 24)        # the tie the clamp is there for
    assert u1[0] == np.float32(1 - 2.0 ** -24) and u1[0] < 1                # 2^24 - 1: rounded to 1.0, clamped back
    f64 = u1.astype(np.float64)
    assert f64[1] == (top - 1) * 2.0 ** -24 and f64[2] == (top - 1) * 2.0 ** -24          # from 2^23 on k + 0.5 is a tie: to even, down or up
    assert f64[3] == (2 ** 23 + 2) * 2.0 ** -24 and f64[4] == (2 ** 23 - 0.5) * 2.0 ** -24  # below 2^23 it is exact
    assert u1[6] == np.float32(2.0 ** -25) and u1[6] > 0 and np.all(u1 < 1) and np.all(np.diff(u1) <= 0)
    assert u2[0] == 1.0 and u2[1] == 1.0 and u2[2] == np.float32(1 - 2.0 ** -24) and u2[3] == 0.0      # u2 may be 1: a whole revolution
    n = P.normals_kernel_uniform(_pairs([top, 0], [0xFFFFFFFF, 0xFFFFFFFF]))
    assert np.all(np.isfinite(n)) and abs(n[0, 0] - 3.4527e-4) < 1e-7 and abs(n[1, 0] - 5.8871) < 1e-4 and np.all(np.abs(n[:, 1]) < 1e-14)


def test_ideal_and_kernel_uniform_references_agree_except_where_u1_rounded():
    """u1 is exact below w >> 8 = 2^23 and a tie from there on: (k + 0.5) needs 25 bits, goes to even -- down for even k, up for odd
    k -- so HALF of all pairs carry a u1 that is off by 2^-25, and only the odd ones can reach 1."""
    w = _random_words(1 << 18)
    k = w[:, 0::2] >> np.uint32(8)
    rounded = k >= 2 ** 23
    gap = np.abs(P.normals_from_bits(w) - P.normals_kernel_uniform(w))
    pair_gap = np.maximum(gap[:, 0::2], gap[:, 1::2])
    assert 0.49 < rounded.mean() < 0.51
    assert pair_gap[rounded].max() > 5e-6                                   # the design gap is real (2.5e-5 over 2^23 normals)
    assert pair_gap[~rounded].max() < 5e-6                                  # u2's rounding alone: r 2 pi 2^-25 <= 1.2e-6
    u1, _ = P.kernel_uniforms(w)
    exact = (k.astype(np.float64) + 0.5) * 2.0 ** -24
    assert np.array_equal(u1.astype(np.float64)[~rounded], exact[~rounded])
    assert np.all(u1.astype(np.float64)[rounded] - exact[rounded] == np.where(k[rounded] % 2 == 1, 2.0 ** -25, -2.0 ** -25))


def test_the_gap_between_the_two_references_is_the_rounding_of_u1():
    """Where u1 rounded (by 2^-25, w >> 8 >= 2^23) the radius moves by 2^-25 |dr/du1| = 2^-25 / (r u1); near 1, with
    1 - u1 = m 2^-24 and r = sqrt(2 m) 2^-12, that is 2^-13 / sqrt(2 m): 1.2e-4 at the clamp (m = 1/2 ideal, 1 clamped).  This is the
    DESIGN gap between normals_from_bits and the kernel: a tolerance against the ideal reference cannot be tightened below it, and
    one against the kernel-uniform reference does not contain it."""
    rng = np.random.default_rng(3)
    # (a) the tail: every w >> 8 with m <= 1024; m is the smaller of the two references' (the radius is concave in m)
    k = 2 ** 24 - 1 - np.arange(1024)
    w = _pairs(k, rng.integers(0, 2 ** 32, size=k.size, dtype=np.uint64))
    u1, _ = P.kernel_uniforms(w)
    m = np.minimum(2.0 ** 24 - k - 0.5, (1.0 - u1[:, 0].astype(np.float64)) * 2.0 ** 24)
    ideal, kern = P.normals_from_bits(w), P.normals_kernel_uniform(w)
    gap = np.max(np.abs(ideal - kern), axis=1)
    rot = 2 * np.pi * 2.0 ** -25 * np.hypot(ideal[:, 0], ideal[:, 1])      # u2's own rounding turns the pair by at most this
    assert np.all(gap <= 2.0 ** -13 / np.sqrt(2 * m) + rot)
    radius = lambda n: np.hypot(n[0, 0], n[0, 1])
    assert 1.0e-4 < radius(kern) - radius(ideal) < 2.0 ** -13               # the clamp: r 2.44e-4 ideal, 3.45e-4 in the kernel
    # (b) everywhere: |dr/du1| = 1 / (r u1) is largest at an end of the interval between the two u1
    w = _random_words(1 << 18)
    k = w[:, 0::2] >> np.uint32(8)
    u1 = P.kernel_uniforms(w)[0].astype(np.float64)
    exact = (k.astype(np.float64) + 0.5) * 2.0 ** -24
    slope = lambda u: 1.0 / (np.sqrt(-2.0 * np.log(u)) * u)
    ideal, kern = P.normals_from_bits(w), P.normals_kernel_uniform(w)
    gap = np.maximum(np.abs(ideal - kern)[:, 0::2], np.abs(ideal - kern)[:, 1::2])
    rot = 2 * np.pi * 2.0 ** -25 * np.hypot(ideal[:, 0::2], ideal[:, 1::2])
    assert np.all(gap <= np.abs(u1 - exact) * np.maximum(slope(u1), slope(exact)) + rot + 1e-15)


def test_emulation_is_at_the_floor_on_raw_normals():
    """A float32 Box-Muller with correctly rounded transcendentals on the kernel's uniforms is within EPS_FLOOR of the float64 one:
    what the reference itself costs, so no device bound can be below it."""
    w = np.concatenate([_random_words(1 << 19), _pairs([2 ** 24 - 1, 0], [0xFFFFFFFF, 0x40000000]).reshape(1, 4)])
    err = np.abs(RC.emulate_normals(w).astype(np.float64) - P.normals_kernel_uniform(w))
    assert 2e-7 < err.max() <= RC.EPS_FLOOR, err.max()
    assert RC.EPS_N >= RC.EPS_FLOOR


@pytest.mark.parametrize("name", RC.NAMES)
def test_emulation_stays_inside_every_bound_at_the_floor(name):
    """rng_dev.h's arithmetic in NumPy float32 against the float64 batch, every element of every row, at eps_n = EPS_FLOOR."""
    c = RC.BY_NAME[name]
    ref = RC.reference(c)
    got = RC.emulate_batch(c)
    ratios = RC.worst_ratios(c, ref, got, RC.EPS_FLOOR)
    assert all(r <= 1.0 for r in ratios.values()), ratios
    x, z1, z2, deps = ref
    assert x.shape == (RC.ROWS, c["D"]) and z1.shape == (RC.ROWS, c["L"]) and z2.shape == (RC.ROWS, c["D"])
    assert np.all(RC.x_bound(c, deps, RC.EPS_FLOOR)[:, c["dd"] + (c["kind"] == 1):] == 0) or c["var"] > 0


def test_the_case_table_is_the_one_the_tests_were_written_for():
    cs = RC.CASES
    assert len(cs) == 21 and len(set(RC.NAMES)) == 21 and all(c["rows"] == 257 for c in cs)
    for kind in range(3):
        mine = [c for c in cs if c["kind"] == kind]
        assert any(c["row0"] == 2 ** 32 - 100 for c in mine) and any(c["step"] == 2 ** 32 - 1 for c in mine)
        assert any(c["tag"] == 0x3FFFFFFF for c in mine) and any(c["seed"] == 0xFEDCBA9876543210 for c in mine)
    lin = [c for c in cs if c["kind"] == 0]
    assert {c["L"] % 4 for c in lin} == {0, 1, 2, 3} and {c["L"] for c in cs} == {20, 5, 6, 7, 1, 32}
    assert {P.noise_block_offset(c["did"]) for c in lin if c["var"] > 0} == {1, 2, 3, 4}
    assert any(c["D"] == 32 for c in cs) and any(c["kind"] == 1 and c["dd"] == 4 and c["D"] == 5 for c in cs)
    assert all(c["tag"] < 0x40000000 for c in cs)


@pytest.mark.parametrize("kind", ["linear_gaussian", "sigmoid", "sphere"])
def test_batch_reference_reproduces_the_per_row_formulas(kind):
    """The rows tests/test_rng.py::test_make_batch_reproduces_datasets_py forms one at a time from sample_normals, at its shape."""
    k, dd, did, pad, L, rows, seed, step = RC.KIND[kind], 3, (3 if kind == "linear_gaussian" else 1), (9 if kind == "linear_gaussian" else 3), 5, 300, 99, 12
    var = 0.04 if k == 0 else 0.0
    D = dd + pad + (k == 1)
    rng = np.random.default_rng(5)
    A = rng.standard_normal((dd, did)) if k == 0 else rng.standard_normal(dd)
    x, z1, z2, deps = P.batch_reference(k, A, dd, did, pad, var, rows, 0, seed, step, 0, L, D, normals=P.normals_from_bits)
    for i in (0, 1, 157, 299):
        q0 = P.noise_block_offset(did)
        n = P.sample_normals(seed, step, 0, i, 4 * q0 + D)
        if k == 0:
            want = np.concatenate([A @ n[:did], np.zeros(pad)]) + np.sqrt(var) * n[4 * q0:4 * q0 + D]
        elif k == 1:
            want = np.concatenate([n[:dd], [1 / (1 + np.exp(-(n[:dd] @ A)))], np.zeros(pad)])
        else:
            want = np.concatenate([n[:dd] / np.linalg.norm(n[:dd]), np.zeros(pad)])
        assert np.max(np.abs(x[i] - want)) < 1e-14
        z = P.sample_normals(seed, step, 0x40000000, i, L + D)
        assert np.array_equal(np.concatenate([z1[i], z2[i]]), z)
        assert np.array_equal(deps["n"][i], n[:did if k == 0 else dd])
    # sharding and the wrap of the row index: rows [100, 200) alone, and a batch that starts 100 rows before 2^32
    xs, z1s, _, _ = P.batch_reference(k, A, dd, did, pad, var, 100, 100, seed, step, 0, L, D, normals=P.normals_from_bits)
    assert np.array_equal(xs, x[100:200]) and np.array_equal(z1s, z1[100:200])
    xw, _, z2w, _ = P.batch_reference(k, A, dd, did, pad, var, 200, 2 ** 32 - 100, seed, step, 0, L, D, normals=P.normals_from_bits)
    assert np.array_equal(xw[100:], x[:100]) and np.array_equal(z2w[100:], z2[:100])
