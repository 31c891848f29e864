"""The references of tests/lin_moment_ref.py are right and their comparisons have power (no GPU): the packed image round-trips and its
three cell classes partition it, exact_batch's sums stay exact in float32, step_ref equals the float64 oracle at every shape of
tests/test_gpu_lin_moments.py, and one defect per reference function -- a dropped row, a transposed block, the latents from 32 up
left out of P1, one wrong d logvar -- lands outside the bound the GPU test uses.  Also: vaek_debug_lin refuses bad arguments on the
host, before any launch."""
import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import lin_moment_ref as LM

# (D, L) of tests/test_gpu_lin_moments.py
SHAPES3 = [(12, 20), (1, 1), (3, 2), (16, 1), (16, 15), (15, 17), (7, 32), (8, 31)]
SHAPES3_STEP = [(17, 13), (7, 33), (3, 41)]
SHAPES4 = [(16, 16), (20, 20), (20, 10), (19, 13), (24, 15), (15, 32), (31, 1)]
SHAPES4_STEP = [(10, 40), (1, 61)]
ALL = SHAPES3 + SHAPES3_STEP + SHAPES4 + SHAPES4_STEP


def _fails(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def cfg_of(D, L, tdv=True, eps=-1.0):
    return O.Config(D, L, (), (), eps, tdv, "linear_gaussian")


def params_of(cfg, seed, lv_lo=-3.0, lv_hi=1.0):
    """The oracle's tree, float32-representable: Lecun weights, biases of scale 0.3, log-variances spread over [lv_lo, lv_hi]."""
    rng = np.random.default_rng(seed)
    r32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    p = O.init_params(cfg, seed=seed)
    for k in p:
        if k.endswith("bias"):
            p[k] = 0.3 * rng.standard_normal(p[k].shape)
    p["epsilon_p"] = np.linspace(lv_lo, lv_hi, cfg.L) if cfg.L > 1 else np.array([lv_hi])
    if cfg.tdv:
        p["epsilon"] = np.array([0.75])
    return {k: r32(v) for k, v in p.items()}


def test_block_count_and_image_length():
    for D, L in SHAPES3 + SHAPES3_STEP:
        assert LM.n_blocks(D, L) == 3 and L + 2 * D + 1 <= 48
    for D, L in SHAPES4 + SHAPES4_STEP:
        assert LM.n_blocks(D, L) == 4 and 49 <= L + 2 * D + 1 <= 64
    assert LM.image_len(3) == 1536 and LM.image_len(4) == 2560


@pytest.mark.parametrize("NB", [3, 4])
def test_pack_unpack_round_trip(NB):
    n = 16 * NB
    g = torch.Generator().manual_seed(NB)
    a = torch.randn(n, n, generator=g, dtype=torch.float64)
    M = a + a.t()
    img = LM.pack(M, NB)
    assert img.numel() == LM.image_len(NB)
    assert torch.equal(LM.unpack(img, NB), M)
    # every element of the symmetric matrix is read from the cell that holds it (lin_m_index)
    for r in range(n):
        for c in range(n):
            assert float(img[LM.m_index(NB, r, c)]) == float(M[r, c])
    # each cell of the image is some element's: the image is a bijection onto the upper block triangle with whole diagonal blocks
    hit = {LM.m_index(NB, r, c) for r in range(n) for c in range(n) if r // 16 <= c // 16}
    assert hit == set(range(LM.image_len(NB)))


@pytest.mark.parametrize("D,L", ALL)
def test_cell_classes_partition_the_image(D, L):
    NB = LM.n_blocks(D, L)
    real, mirror, zero = LM.cells(D, L, NB)
    assert int(real.sum() + mirror.sum() + zero.sum()) == LM.image_len(NB) == NB * (NB + 1) // 2 * 256
    assert not (real & mirror).any() and not (real & zero).any() and not (mirror & zero).any()
    nf = L + 2 * D + 1
    assert int(real.sum()) == nf * (nf + 1) // 2                       # the upper triangle of the real features, each once
    assert int(mirror.sum()) == sum(k * (k - 1) // 2 for k in (min(16, max(0, nf - 16 * a)) for a in range(NB)))
    # a matrix that is 1 on the real features packs to 1 exactly on real | mirror
    img = LM.pack(torch.ones(nf, nf, dtype=torch.float64), NB)
    assert torch.equal(img != 0, real | mirror)


@pytest.mark.parametrize("D,L", [(12, 20), (1, 1), (16, 16), (1, 61)])
def test_exact_batch_sums_are_exact_in_float32(D, L):
    for B in (1, 2, 9, 600):
        x, z1, z2 = LM.exact_batch(B, D, L, seed=B)
        for t, cols in ((x, D), (z1, L), (z2, D)):
            assert t.dtype == torch.float32 and t.shape == (B, cols)
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 7
            if B >= 2:
                assert bool((t != t[:1]).any(0).all()), "a constant column"
        u = LM.features(x, z1, z2)
        assert float(u.abs().max()) ** 2 * 512 < 2 ** 24               # every partial sum over at most 512 rows, in any order
        M, Mabs = LM.moments(x, z1, z2)
        assert torch.equal(M, M.round()) and float(Mabs.max()) <= 49 * B
        # a float32 chain over a tile's rows, in two different orders, is the float64 sum
        u32 = u[:512].to(torch.float32)
        acc_f, acc_b = torch.zeros_like(M, dtype=torch.float32), torch.zeros_like(M, dtype=torch.float32)
        for r in range(u32.shape[0]):
            acc_f += torch.outer(u32[r], u32[r])
            acc_b += torch.outer(u32[-1 - r], u32[-1 - r])
        want = (u[:512].t() @ u[:512])
        assert torch.equal(acc_f.to(torch.float64), want) and torch.equal(acc_b.to(torch.float64), want)
    a, b = LM.exact_batch(64, D, L, seed=1), LM.exact_batch(64, D, L, seed=2)
    assert not torch.equal(a[0], b[0]) and all(torch.equal(s, t) for s, t in zip(a, LM.exact_batch(64, D, L, seed=1)))


def test_wide_batch_spans_its_range():
    x, z1, z2 = LM.wide_batch(4096, 5, 7, seed=3)
    for t in (x, z1, z2):
        a = t.abs()
        assert float(a.min()) >= 0.0099 and float(a.max()) <= 10.001 and float(a.min()) < 0.02 and float(a.max()) > 5.0
        assert 0.4 < float((t > 0).double().mean()) < 0.6
        # full mantissas: the low bit is set about half of the time
        assert 0.4 < float((t.view(torch.int32) & 1).double().mean()) < 0.6


@pytest.mark.parametrize("D,L", ALL)
def test_step_ref_equals_the_oracle(D, L):
    B = 37
    for tdv in (True, False):
        for Bt in (B, 2 * B + 3):
            cfg = cfg_of(D, L, tdv)
            p = params_of(cfg, 100 * D + L)
            x, z1, z2 = LM.wide_batch(B, D, L, seed=D + 64 * L)
            M, _ = LM.moments(x, z1, z2)
            ref = LM.step_ref(cfg, p, M, B, Bt)
            x64, z164, z264 = (t.double().numpy() for t in (x, z1, z2))
            loss, g = O.loss_and_grad(cfg, p, x64, z164, z264, batch_total=Bt)
            flat = torch.as_tensor(O.flatten(cfg, g))
            got, mag = ref["grad"]
            assert got.shape == flat.shape == mag.shape
            assert bool(((got - flat).abs() <= 1e-11 * mag).all()), (D, L, tdv, Bt, float(((got - flat).abs() / mag).max()))
            assert bool((mag >= got.abs() * (1 - 1e-12)).all())
            assert abs(float(ref["loss"][0]) - loss) <= 1e-11 * float(ref["loss"][1])
            _, dkl, mse, _, _ = O.loss_eval(cfg, p, x64, z164, z264)
            assert abs(float(ref["dkl"][0]) - dkl * B / Bt) <= 1e-11 * float(ref["dkl"][1])
            assert abs(float(ref["mse"][0]) - mse * B / Bt) <= 1e-11 * float(ref["mse"][1])


# ---- the comparisons have power -------------------------------------------------------------------------------------------------
def _f32_of(cfg, ref):
    """What a correct updater leaves: the reference rounded to float32, and the zero slot."""
    r, _ = LM.step_vectors(ref)
    return torch.cat([r.to(torch.float32), torch.zeros(1)])


@pytest.mark.parametrize("D,L", [(12, 20), (1, 1), (16, 16), (7, 33), (1, 61)])
def test_check_step_takes_the_rounded_reference_at_half_its_bound(D, L):
    cfg = cfg_of(D, L)
    p = params_of(cfg, 5, lv_lo=-30.0, lv_hi=20.0)
    M, _ = LM.moments(*LM.exact_batch(300, D, L, seed=9))
    ref = LM.step_ref(cfg, p, M, 300, 300)
    got = _f32_of(cfg, ref)
    assert LM.check_step(got, cfg, ref) <= 0.5
    # ONE wrong d logvar, by five float32 ulps of its terms -- far inside 1e-4 of the leaf's largest element, outside this bound
    _, mag = LM.step_vectors(ref)
    off = 2 * D * L + L + D
    for l in {0, L // 2, L - 1}:
        bad = got.clone()
        bad[off + l] += 5 * LM.U24 * float(mag[off + l])
        _fails(LM.check_step, bad, cfg, ref)
    bad = got.clone()
    bad[-1] = 1e-30
    _fails(LM.check_step, bad, cfg, ref)


@pytest.mark.parametrize("D,L", SHAPES3_STEP[1:] + SHAPES4_STEP)
def test_latents_from_32_up_left_out_of_P1_fail(D, L):
    """The defect of LinUpd's run-time instantiation as it stood (its P1 = R M loop stopped at latent 32)."""
    cfg = cfg_of(D, L)
    p = params_of(cfg, 7)
    M, _ = LM.moments(*LM.exact_batch(300, D, L, seed=11))
    ref = LM.step_ref(cfg, p, M, 300, 300)
    _fails(LM.check_step, _f32_of(cfg, LM.step_ref(cfg, p, M, 300, 300, p1_latents=32)), cfg, ref)
    _fails(LM.check_step, _f32_of(cfg, LM.step_ref(cfg, p, M, 300, 300, p1_latents=L - 1)), cfg, ref)
    assert LM.check_step(_f32_of(cfg, LM.step_ref(cfg, p, M, 300, 300, p1_latents=L)), cfg, ref) <= 0.5


@pytest.mark.parametrize("D,L", [(12, 20), (20, 20)])
def test_a_dropped_row_fails_both_comparisons(D, L):
    NB = LM.n_blocks(D, L)
    cfg = cfg_of(D, L)
    p = params_of(cfg, 3)
    for B, T, cw in ((8443, 512, 4), (65664, 288, 4), (4097, 256, 8)):
        for make in (LM.exact_batch, LM.wide_batch):
            x, z1, z2 = make(B, D, L, seed=B)
            M, Mabs = LM.moments(x, z1, z2)
            Md, _ = LM.moments(x[:-1], z1[:-1], z2[:-1])
            nadd = None if make is LM.exact_batch else LM.n_add(T, cw)
            assert LM.check_moments(LM.pack(M, NB), M, Mabs, D, L, NB, nadd) == 0.0
            _fails(LM.check_moments, LM.pack(Md, NB), M, Mabs, D, L, NB, nadd)
        ref = LM.step_ref(cfg, p, M, B, B)
        _fails(LM.check_step, _f32_of(cfg, LM.step_ref(cfg, p, Md, B, B)), cfg, ref)


@pytest.mark.parametrize("D,L", [(12, 20), (16, 16), (31, 1)])
def test_image_defects_fail(D, L):
    NB = LM.n_blocks(D, L)
    x, z1, z2 = LM.exact_batch(100, D, L, seed=4)
    M, Mabs = LM.moments(x, z1, z2)
    img = LM.pack(M, NB)
    real, mirror, zero = LM.cells(D, L, NB)
    for nadd in (None, LM.n_add(256, 8)):
        assert LM.check_moments(img, M, Mabs, D, L, NB, nadd) == 0.0
        # an off-diagonal block stored transposed
        blk = LM.lin_blk(NB, 0, 1)
        t = img.clone()
        full = LM.unpack(img, NB)
        sub = full[0:16, 16:32].t().contiguous()
        r, c, _ = LM._coords(NB)
        sel = torch.arange(blk * 256, blk * 256 + 256)
        t[sel] = sub[r[sel], c[sel] - 16]
        _fails(LM.check_moments, t, M, Mabs, D, L, NB, nadd)
        # one cell of the mirrored half of a diagonal block off by one
        t = img.clone()
        t[int(torch.nonzero(mirror)[0])] += 1.0
        _fails(LM.check_moments, t, M, Mabs, D, L, NB, nadd)
        # something in a cell of an unused feature
        if zero.any():                                     # (64 features leave none)
            t = img.clone()
            t[int(torch.nonzero(zero)[-1])] = 1e-30
            _fails(LM.check_moments, t, M, Mabs, D, L, NB, nadd)
        # one real cell off by one
        t = img.clone()
        e = int(torch.nonzero(real & ~mirror)[-1])
        t[e] += 1.0
        _fails(LM.check_moments, t, M, Mabs, D, L, NB, nadd)
    # the wide bound is per cell and relative to Mabs: an error of twice the bound in one cell fails, half of it passes
    x, z1, z2 = LM.wide_batch(100, D, L, seed=5)
    M, Mabs = LM.moments(x, z1, z2)
    img, wabs = LM.pack(M, NB), LM.pack(Mabs, NB)
    nadd = LM.n_add(256, 8)
    e = int(torch.nonzero(real & ~LM._coords(NB)[2])[3])               # (an off-diagonal block: no mirror image to keep in step)
    t = img.clone()
    t[e] += 0.5 * (nadd + 1) * LM.U24 * float(wabs[e])
    assert 0.49 < LM.check_moments(t, M, Mabs, D, L, NB, nadd) < 0.51
    t[e] = img[e] + 2 * (nadd + 1) * LM.U24 * float(wabs[e])
    _fails(LM.check_moments, t, M, Mabs, D, L, NB, nadd)


def test_n_add_of_the_two_forms():
    assert LM.n_add(256, 8) == 40 and LM.n_add(288, 4) == 76 and LM.n_add(192, 4) == 52 and LM.n_add(512, 4) == 132


def test_roundings():
    k = LM.roundings(cfg_of(3, 2, True))
    P = 2 * 3 * 2 + 2 * 2 + 3 + 1
    assert k.numel() == P + 3 and k[:P - 1].eq(2).all() and k[P - 1] == 3 and k[P:].tolist() == [4, 3, 4]
    k = LM.roundings(cfg_of(3, 2, False))
    assert k.numel() == P - 1 + 3 and k[:P - 1].eq(2).all() and k[P - 1:].tolist() == [4, 3, 4]


# ---- vaek_debug_lin validates on the host ---------------------------------------------------------------------------------------
def test_debug_lin_refuses_null_arguments_before_launching():
    from vae_training_amd import _lib
    fn = LM.bind(_lib.load())
    a = LM.LinDebugArgs()
    for op in (0, 1, 2):
        assert fn(None, op, a, None, None) == -1          # VAEK_ERR_INVALID: no context
