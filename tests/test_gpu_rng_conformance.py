"""-m gpu: the device batch generator (csrc/rng_dev.h: normals4, dataset_normals, dataset_cols4, latent_block, make_batch_items)
against the float64 oracle at its edges.  Every kernel that draws in-launch is tested as "equals vaek_make_batch, bit for bit", so
vaek_make_batch is the root of trust; here it is held to oracle/philox.py's kernel-uniform reference element by element, on the
cases and with the bounds of tests/rng_cases.py (whose docstring has the reasons; tests/test_rng_host.py proves the bounds hold for
the reference alone).  Also: the raw normals of vaek_rng_fill, which is where EPS_N is measured (profiles/rng_conformance.txt); the
counters at which u1 rounded to 1 and a sphere row of dd <= 2 was 0 / 0 before normals4 clamped it; and the streamers' hand-written
copy of the dataset arithmetic (linear_moments_dev.h, gen_round) away from dd = did, with noise in the four-block form and with
all 256 floats of its LDS copy of A in use."""
import functools

import numpy as np
import pytest
import torch

from oracle import philox as P
from tests import rng_cases as RC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _engine(rows, D, L, sig=False):
    from vae_training_amd.engine import Engine
    return Engine(rows, D, L, sigmoid_decoder=sig)


def _host(t):
    return t.cpu().numpy()


# ---- raw normals -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fill_reference(i):
    """(Philox words [n / 4, 4], kernel-uniform normals [n]) of FILL_TRIPLES[i] at n = FILL_BIG, computed once."""
    seed, step, tag = RC.FILL_TRIPLES[i]
    nb = RC.FILL_BIG // 4
    ctr = np.zeros((nb, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 2], ctr[:, 3] = np.arange(nb), np.uint32(step), np.uint32(tag)
    words = P.philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return words, P.normals_kernel_uniform(words).reshape(-1)


@pytest.mark.parametrize("i", range(len(RC.FILL_TRIPLES)))
def test_raw_normals_bits_exact_and_normals_within_eps_n(i):
    """vaek_rng_fill at n = 2^22 and at 1, 2, 3, 5, 4099: the words bit for bit, every normal within EPS_N of the kernel-uniform
    reference; the normals-only and the bits-only form write what the form with both writes."""
    seed, step, tag = RC.FILL_TRIPLES[i]
    eng = _engine(64, 12, 20)
    words, ref = _fill_reference(i)
    normals, bits = eng.rng_fill(RC.FILL_BIG, seed, step, tag, bits=True)
    got_w, got_n = _host(bits).view(np.uint32), _host(normals).astype(np.float64)
    assert np.array_equal(got_w, words.reshape(-1))
    err = np.abs(got_n - ref)
    j = int(np.argmax(err))
    u1, u2 = P.kernel_uniforms(words)
    pair = np.unravel_index(j // 2, u1.shape)
    print(f"rng_fill seed {seed:#x} step {step} tag {tag:#x}: max |device - kernel-uniform| {err.max():.4e} = {err.max() / RC.EPS_N:.3f} of EPS_N at normal {j}, "
          f"u1 {float(u1[pair])!r} u2 {float(u2[pair])!r}; against the ideal reference {np.abs(got_n - P.normals_from_bits(words).reshape(-1)).max():.3e}")
    assert np.isfinite(got_n).all() and err.max() <= RC.EPS_N
    assert torch.equal(eng.rng_fill(RC.FILL_BIG, seed, step, tag), normals)
    assert torch.equal(eng.rng_fill(RC.FILL_BIG, seed, step, tag, bits=True, normals=False), bits)
    for n in RC.FILL_SMALL:
        sn, sb = eng.rng_fill(n, seed, step, tag, bits=True)
        assert sn.shape == (n,) and torch.equal(sn, normals[:n]) and torch.equal(sb, bits[:n]), n
        assert torch.equal(eng.rng_fill(n, seed, step, tag), sn) and torch.equal(eng.rng_fill(n, seed, step, tag, bits=True, normals=False), sb), n


# ---- the counters where u1 rounded to 1 ---------------------------------------------------------------------------------------------
def _tail_case(row, dd, tag=0):
    return dict(kind=2, kind_name="sphere", dd=dd, did=1, pad=0, var=0.0, L=5, D=dd, rows=1, row0=row, step=0, tag=tag, seed=RC.TAIL_SEED)


@pytest.mark.parametrize("row,word,want", RC.TAIL_ROWS)
def test_sphere_rows_are_finite_where_u1_rounded_to_one(row, word, want):
    """w >> 8 = 2^24 - 1 in the first pair: sphere rows of dd = 1 and 2 are that pair alone, 0 / 0 = NaN before the clamp; in the second
    pair: dd = 3 and 4 hold it.  Finite, of unit norm, and inside the bounds of the case table; the latents under the largest tag too."""
    for dd in ((1, 2) if word == 0 else (3, 4)):
        c = _tail_case(row, dd)
        x, z1, z2 = _engine(1, dd, c["L"]).make_batch(2, None, dd, 1, 0, 0.0, 1, RC.TAIL_SEED, step=0, tag=0, row0=row)
        xh = _host(x).astype(np.float64)
        assert np.isfinite(xh).all(), (row, dd, xh)
        assert abs(np.linalg.norm(xh) - 1.0) <= np.sqrt(dd) * 2.0 ** -22, (row, dd, xh)
        ratios = RC.worst_ratios(c, RC.reference(c), (_host(x), _host(z1), _host(z2)), RC.EPS_N)
        assert all(r <= 1.0 for r in ratios.values()), (row, dd, ratios)
        c = _tail_case(row, dd, tag=RC.TAG_EDGE)
        got = _engine(1, dd, c["L"]).make_batch(2, None, dd, 1, 0, 0.0, 1, RC.TAIL_SEED, step=0, tag=RC.TAG_EDGE, row0=row)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        ratios = RC.worst_ratios(c, RC.reference(c), tuple(_host(t) for t in got), RC.EPS_N)
        assert all(r <= 1.0 for r in ratios.values()), (row, dd, ratios)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def _draw(c, eng=None, rows=None, row0=None, **kw):
    A = RC.make_A(c)
    A = None if A is None else torch.as_tensor(A).cuda().contiguous()
    eng = eng or _engine(c["rows"], c["D"], c["L"], c["kind"] == 1)
    return eng.make_batch(c["kind"], A, c["dd"], c["did"], c["pad"], c["var"], c["rows"] if rows is None else rows, c["seed"], step=c["step"],
                          tag=c["tag"], row0=c["row0"] if row0 is None else row0, **kw)


@pytest.mark.parametrize("name", RC.NAMES)
def test_every_element_of_the_batch_is_within_its_bound(name):
    """x, z1 and z2 of the case against batch_reference, every element of all 257 rows; want_x = False and want_z = False each leave
    the other output's bits."""
    c = RC.BY_NAME[name]
    x, z1, z2 = _draw(c)
    ratios = RC.worst_ratios(c, RC.reference(c), (_host(x), _host(z1), _host(z2)), RC.EPS_N)
    print(f"{name}: largest error / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    nx, z1b, z2b = _draw(c, want_x=False)
    assert nx is None and torch.equal(z1b, z1) and torch.equal(z2b, z2)
    xb, nz1, nz2 = _draw(c, want_z=False)
    assert nz1 is None and nz2 is None and torch.equal(xb, x)


def test_rows_drawn_alone_equal_the_full_batch_off_the_square_matrix():
    """Rows [100, 200) drawn alone are the full batch's, bit for bit, at dd = 2, did = 5 with noise."""
    c = RC.BY_NAME["linear_gaussian_dd2_did5_pad3_var0.25_L7"]
    x, z1, z2 = _draw(c)
    xs, z1s, z2s = _draw(c, eng=_engine(100, c["D"], c["L"]), rows=100, row0=c["row0"] + 100)
    assert torch.equal(xs, x[100:200]) and torch.equal(z1s, z1[100:200]) and torch.equal(z2s, z2[100:200])


# ---- the streamers' own copy of the dataset arithmetic ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [130, 300])
@pytest.mark.parametrize("form,kind,D,L,dd,did,pad,var", [
    ("48-feature", 0, 16, 15, 16, 16, 0, 0.25),     # all 256 floats of the LDS copy of A, four dataset blocks, noise block offset 4
    ("48-feature", 0, 7, 10, 2, 5, 5, 0.25),        # did > dd, odd D
    ("48-feature", 2, 4, 4, 1, 1, 3, 0.0),          # sphere at dd = 1
    ("four-block", 0, 20, 20, 16, 9, 4, 0.04),      # noise in the four-block form
    ("four-block", 2, 24, 8, 16, 16, 8, 0.0),       # sphere at dd = 16
])
def test_in_launch_draw_equals_make_batch_plus_train_steps_off_the_tested_line(form, kind, D, L, dd, did, pad, var, B):
    """vaek_train_steps_gen(3) == vaek_make_batch(step = t), t = 0 .. 2, followed by vaek_train_steps, BITWISE, in the shape of
    tests/test_gpu_loop.py::test_in_launch_draw_equals_make_batch_plus_train_steps -- where did != dd, did > 4 with noise, dd = 1
    and dd = 16."""
    from vae_training_amd.engine import Engine
    n = 3
    assert D == dd + pad and (L + 2 * D + 1 <= 48) == (form == "48-feature") and L + 2 * D + 1 <= 64
    eng = Engine(B, D, L, (), (), -1.0, True, False)
    assert eng.supports_train_steps() and eng.supports_train_steps_gen(kind)
    A = torch.randn(dd, did, generator=torch.Generator().manual_seed(11)).cuda().contiguous() if kind == 0 else None
    torch.manual_seed(0)
    p0 = (torch.randn(eng.P, device="cuda") * 0.3).contiguous()
    seed, tag, row0 = 77, 5, 1000

    def state():
        return [p0.clone(), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(), torch.zeros(1, dtype=torch.int32, device="cuda")]
    a, b = state(), state()
    ring_a = torch.zeros(n + 4, dtype=torch.float32, device="cuda"); ring_b = torch.zeros_like(ring_a)
    eng.set_loss_history(ring_a)
    eng.train_steps_gen(*a, n, 1e-3, kind, A, dd, did, pad, var, seed, tag=tag, row0=row0)
    torch.cuda.synchronize()
    assert not eng.train_steps_gave_up()
    batches = [eng.make_batch(kind, A, dd, did, pad, var, B, seed, step=t, tag=tag, row0=row0) for t in range(n)]
    eng.set_loss_history(ring_b)
    eng.train_steps(*b, batches, 1e-3)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up()
    assert int(a[4].item()) == n == int(b[4].item())
    for x, y, what in zip(a[:4], b[:4], ("params", "grads", "m", "v")):
        assert torch.equal(x, y), what
    assert torch.equal(ring_a[:n], ring_b[:n]) and bool(torch.isfinite(ring_a[:n]).all())
