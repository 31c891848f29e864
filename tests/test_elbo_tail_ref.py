"""The comparison of tests/test_gpu_elbo_tail.py has power: a float32 emulation of each kernel of the step's tail (torch float32 on
the CPU, the kernels' own expressions, the same splits and slab order) passes every check of tests/elbo_tail_ref.py at less than half
its bound, and the same emulation with one of the defects such kernels tend to have FAILS it.  Also: vaek_debug_tail
(csrc/debug_tail.hip) refuses bad arguments on the host, before any launch (no stream, no GPU)."""
import pytest
import torch

from tests import dense16_ref as R
from tests import elbo_tail_ref as T

F = torch.float32
RATIOS = {}


def _g(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def note(fam, r):
    RATIOS[fam] = max(RATIOS.get(fam, 0.0), r)
    return r


def _fails(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def t32(v):
    return torch.tensor(v, dtype=F)


# ---- float32 emulations: the kernels' expressions, term by term ----------------------------------------------------------------
def elbo_f32(x, y_lin, y_sig, z2, mu, eps, inv_bt, rps, owned=None, dsig_mut=False):
    """elbo_kernel: (d_lin, d_sig, partial [S][4]).  owned: per split the (first, one past last) row it sums (default: its own)."""
    eps = t32(eps)
    inv_var, sigma = torch.exp(-eps), torch.exp(0.5 * eps)
    dscale = inv_var * t32(inv_bt)
    xh = y_lin + sigma * z2
    sg = None
    if y_sig is not None:
        sg = 1.0 / (1.0 + torch.exp(-y_sig))
        xh = xh + sg
    r = xh - x
    q = r * r * inv_var
    mse, deps = 0.5 * q, -0.5 * q + 0.5 * sigma * z2 * r * inv_var
    d_lin = r * dscale
    d_sig = None if sg is None else (d_lin * sg if dsig_mut else d_lin * sg * (1.0 - sg))
    rows = x.shape[0]
    S = T.n_splits(rows, rps)
    owned = owned or [(s * rps, min(rows, (s + 1) * rps)) for s in range(S)]
    part = torch.zeros(S, 4, dtype=F)
    for s, (r0, r1) in enumerate(owned):
        part[s, 0], part[s, 1], part[s, 2] = mse[r0:r1].sum(), (mu[r0:r1] * mu[r0:r1]).sum(), deps[r0:r1].sum()
    return d_lin, d_sig, part


def reparam_f32(d, mu, z1, inv_bt, rps):
    rows = d.shape[0]
    S = T.n_splits(rows, rps)
    part = torch.stack([(d[s * rps:(s + 1) * rps] * z1[s * rps:(s + 1) * rps]).sum(0) for s in range(S)])
    return d + mu * t32(inv_bt), part


def seq_sum(t, n):
    """t[0] + t[1] + ... + t[n - 1] in float32, in that order (the slab order of finalize / bulk_finalize / sum_slabs)."""
    acc = torch.zeros_like(t[0])
    for s in range(n):
        acc = acc + t[s]
    return acc


def finalize_f32(slabs, segs, S, epart, rpart, params, off_epsp, off_eps, L, D, eps_cli, rows_over_bt, inv_bt, rows, mut=None):
    """finalize_kernel / bulk_finalize_kernel: grads [P + 4] in float32."""
    P = off_epsp + L + (1 if off_eps >= 0 else 0)
    g = torch.zeros(P + 4, dtype=F)
    start = 0
    for end, cnt in list(segs) + [(off_epsp, S)]:
        if end > start:
            g[start:end] = seq_sum(slabs[:, start:end], cnt)
        start = max(start, end)
    Se = epart.shape[0]
    rows_f, inv, rob = t32(float(rows)), t32(inv_bt), t32(1.0 if mut == "rows_over_bt" else rows_over_bt)
    lv = params[off_epsp:off_epsp + L]
    g[off_epsp:off_epsp + L] = 0.5 * torch.exp(0.5 * lv) * seq_sum(rpart, Se) - 0.5 * (1.0 - torch.exp(lv)) * rob
    s_mse, s_musq, s_deps = seq_sum(epart[:, 0], Se), seq_sum(epart[:, 1], Se), seq_sum(epart[:, 2], Se)
    eps = params[off_eps] * t32(eps_cli) if off_eps >= 0 else t32(eps_cli)
    if off_eps >= 0:
        c = t32(0.0) if mut == "deps_const" else 0.5 * rows_f * t32(float(D))
        g[off_eps] = t32(eps_cli) * (s_deps + c) * inv
    klc = (1.0 + lv + torch.exp(lv)).sum() if mut == "kl_sign" else (1.0 + lv - torch.exp(lv)).sum()
    dkl = (0.5 * s_musq - 0.5 * rows_f * klc) * inv
    mse = (s_mse + 0.5 * rows_f * t32(float(D)) * (t32(T.LOG2PI) + eps)) * inv
    g[P], g[P + 1], g[P + 2] = dkl + mse, dkl, mse
    return g


def adam_f32(p, m, v, g, t, lr, grad_scale=1.0, mut=None):
    """adam_apply with adam_bias_corrections.  (p', m', v')."""
    g = g * t32(1.0 if mut == "grad_scale" else grad_scale)
    one_b1, one_b2 = t32(1.0 - 0.9), (t32(1.0) - t32(0.999)) if mut == "one_minus_beta" else t32(1.0 - 0.999)
    m1 = t32(0.9) * m + one_b1 * g
    v1 = t32(0.999) * v + one_b2 * g * g
    tt = t32(float(t - 1 if mut == "bias_t" else t))
    bc1, bc2 = -torch.expm1(tt * t32(-0.10536051565782628)), -torch.expm1(tt * t32(-0.0010005003335835335))
    return p - t32(lr) * (m1 / bc1) / (torch.sqrt(v1 / bc2) + t32(1e-8)), m1, v1


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def elbo_inputs(rows, D, L, seed):
    g = _g(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(rows, D), y_lin=r(rows, D), y_sig=r(rows, D) * 2.0, z2=r(rows, D), mu=r(rows, L))


INV_BT = T.f32(1.0 / 777.0)


def check_elbo(out, inp, sig, eps, rps, fam="elbo"):
    d_lin, d_sig, part = out
    ys = inp["y_sig"] if sig else None
    y, mag, (rl, ml), rs = T.elbo_elements(inp["x"], inp["y_lin"], ys, inp["z2"], eps, INV_BT)
    note(fam + " d_lin", R.check_f32(d_lin, rl, ml, what="d_lin"))
    if sig:
        note(fam + " d_sig", R.check_f32(d_sig, rs[0], rs[1], what="d_sig"))
    ref, bound = T.elbo_partials(y, mag, inp["x"], inp["z2"], inp["mu"], eps, rps)
    note(fam + " partials", T.check_partials(part, ref, bound, what="partials"))


def test_row_sums_agree_with_elbo_sums():
    """The per-row form of the ELBO sums is dense16_ref.elbo_sums, only summed by split."""
    inp = elbo_inputs(129, 7, 3, 3)
    y, mag = inp["y_lin"].double(), inp["y_lin"].double().abs()
    (mse, deps), (bm, bd) = R.elbo_sums(y, mag, inp["x"], inp["z2"], -2.25)
    a, b, c, d = (float(t.sum()) for t in T.elbo_row_sums(y, mag, inp["x"], inp["z2"], -2.25))
    for got, want in ((a, mse), (b, deps), (c, bm), (d, bd)):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)


@pytest.mark.parametrize("sig", [False, True])
def test_elbo_emulation_passes_and_mutations_fail(sig):
    rows, D, L, rps = 257, 7, 6, 128
    inp = elbo_inputs(rows, D, L, 4)
    eps = T.eps_of(0.75, -3.0)
    args = (inp["x"], inp["y_lin"], inp["y_sig"] if sig else None, inp["z2"], inp["mu"], eps, INV_BT, rps)
    check_elbo(elbo_f32(*args), inp, sig, eps, rps)
    # a row dropped from one split; a split boundary one row off (the total unchanged, two splits wrong)
    for owned in ([(0, 128), (128, 255), (256, 257)], [(0, 129), (129, 256), (256, 257)]):
        _fails(check_elbo, elbo_f32(*args, owned=owned), inp, sig, eps, rps, fam="mutated")
    y, mag, _, _ = T.elbo_elements(inp["x"], inp["y_lin"], inp["y_sig"] if sig else None, inp["z2"], eps, INV_BT)
    ref, bound = T.elbo_partials(y, mag, inp["x"], inp["z2"], inp["mu"], eps, rps)
    part = elbo_f32(*args, owned=[(0, 129), (129, 256), (256, 257)])[2]
    assert T.ratio_of(part[:, :3].double().sum(0), ref.sum(0), bound.sum(0)) < 1.0      # only the per-split check sees it
    if sig:     # d_sig with sg in place of sg (1 - sg)
        _fails(check_elbo, elbo_f32(*args, dsig_mut=True), inp, sig, eps, rps, fam="mutated")
    # partial[s][3] must be exactly 0
    out = elbo_f32(*args)
    out[2][1, 3] = 1e-30
    _fails(check_elbo, out, inp, sig, eps, rps, fam="mutated")


def test_d_sig_bound_is_relative_to_one_plus_sg():
    """At y_sig = 4.5 the float32 1 - sg is good to ~1e-5 relative only: the emulation must still pass."""
    rows, D = 64, 4
    inp = elbo_inputs(rows, D, 2, 5)
    inp["y_sig"] = torch.full((rows, D), 4.5) + torch.randn(rows, D, generator=_g(6)) * 0.01
    check_elbo(elbo_f32(inp["x"], inp["y_lin"], inp["y_sig"], inp["z2"], inp["mu"], -2.0, INV_BT, 64), inp, True, -2.0, 64)


def test_elbo_reduce_emulation():
    rows, rps, bm, nbx, L = 1000, 256, 128, 3, 6
    g = _g(7)
    ntr = (rows + bm - 1) // bm
    part = 10.0 ** (torch.rand(ntr + 2, nbx, 2, generator=g) * 4 - 3) * torch.sign(torch.randn(ntr + 2, nbx, 2, generator=g))
    mu = torch.randn(rows, L, generator=g)
    S = T.n_splits(rows, rps)

    def emu(shift=0):
        out = torch.zeros(S, 4, dtype=F)
        for s in range(S):
            t0, t1 = s * rps // bm + shift, (min(rows, (s + 1) * rps) + bm - 1) // bm
            out[s, 0], out[s, 2] = part[t0:t1, :, 0].sum(), part[t0:t1, :, 1].sum()
            out[s, 1] = (mu[s * rps:(s + 1) * rps] ** 2).sum()
        return out
    ref, bound = T.tile_partials(part, bm, nbx, mu, rows, rps)
    note("elbo_reduce", T.check_partials(emu(), ref, bound))
    _fails(T.check_partials, emu(shift=1), ref, bound)


def test_reparam_bwd_emulation_passes_and_mutations_fail():
    rows, L, rps = 1000, 20, 334
    g = _g(8)
    d, mu, z1 = (torch.randn(rows, L, generator=g) for _ in range(3))
    lv = torch.randn(L, generator=g) * 0.5
    dmu, part = reparam_f32(d, mu, z1, INV_BT, rps)
    (r1, m1), (r2, m2) = T.reparam_bwd(d, mu, z1, INV_BT, rps)
    note("reparam_bwd dmu", R.check_f32(dmu, r1, m1))
    note("reparam_bwd partials", R.check_f32(part, r2, m2))
    rob = T.f32(rows / 777.0)
    got = 0.5 * torch.exp(0.5 * lv) * seq_sum(part, part.shape[0]) - 0.5 * (1.0 - torch.exp(lv)) * t32(rob)
    ref, mag = T.d_logvar(r2.sum(0), m2.sum(0), lv, rob)
    note("reparam_bwd d_logvar", R.check_f32(got, ref, mag))
    # a row owned by the neighbouring split; rows_over_bt taken as 1 at rows != bt
    _fails(R.check_f32, reparam_f32(d, mu, z1, INV_BT, rps + 1)[1][:3], r2, m2)
    bad = 0.5 * torch.exp(0.5 * lv) * seq_sum(part, part.shape[0]) - 0.5 * (1.0 - torch.exp(lv))
    _fails(R.check_f32, bad, ref, mag)


def finalize_inputs(seed=9, L=20, with_eps=True):
    g = _g(seed)
    D, Se, rows = 7, 9, 300.0
    segs = [(40, 4), (47, 9), (49, 64), (130, 1), (131, 9)]
    off_epsp = 131
    off_eps = off_epsp + L if with_eps else -1
    P = off_epsp + L + (1 if with_eps else 0)
    slabs = torch.randn(64, 192, generator=g) * 10.0 ** (torch.rand(64, 192, generator=g) * 3 - 2)
    epart = torch.rand(Se, 4, generator=g) * 100.0
    epart[:, 2] -= 60.0
    epart[:, 3] = 0
    rpart = torch.randn(Se, L, generator=g)
    params = torch.randn(P, generator=g) * 0.5
    return dict(slabs=slabs, segs=segs, S=64, epart=epart, rpart=rpart, params=params, off_epsp=off_epsp, off_eps=off_eps, L=L, D=D,
                eps_cli=-3.0, rows_over_bt=T.f32(rows / 777.0), inv_bt=INV_BT, rows=rows)


def check_finalize(g, ref, mag, kw, fam="finalize"):
    P, o, L = ref.numel() - 4, kw["off_epsp"], kw["L"]
    zero = torch.zeros(P + 4, dtype=torch.bool)
    zero[P + 3] = True
    R.check_f32(g, ref, mag, zero=zero, what=fam)
    parts = {"weights": slice(0, o), "epsilon_p": slice(o, o + L), "loss": slice(P, P + 3)}
    if kw["off_eps"] >= 0:
        parts["epsilon"] = slice(kw["off_eps"], kw["off_eps"] + 1)
    for name, sl in parts.items():
        note(f"{fam} {name}", R.check_f32(g[sl], ref[sl], mag[sl]))


@pytest.mark.parametrize("with_eps", [True, False])
def test_finalize_emulation_passes_and_mutations_fail(with_eps):
    kw = finalize_inputs(with_eps=with_eps)
    ref, mag = T.finalize(**kw)
    check_finalize(finalize_f32(**kw), ref, mag, kw)
    # one slab too many / one too few for one layer of the table (the (47, 9) layer between (40, 4) and (49, 64))
    for cnt in (10, 8):
        segs = [(e, cnt if e == 47 else c) for e, c in kw["segs"]]
        _fails(check_finalize, finalize_f32(**{**kw, "segs": segs}), ref, mag, kw, fam="mutated")
    # the two-element layer (47, 49] summed over its neighbour's count
    segs = [(e, 9 if e == 49 else c) for e, c in kw["segs"]]
    _fails(check_finalize, finalize_f32(**{**kw, "segs": segs}), ref, mag, kw, fam="mutated")
    muts = ["rows_over_bt", "kl_sign"] + (["deps_const"] if with_eps else [])
    for mut in muts:
        _fails(check_finalize, finalize_f32(**kw, mut=mut), ref, mag, kw, fam="mutated")
    bad = finalize_f32(**kw)
    bad[-1] = 1e-30
    _fails(check_finalize, bad, ref, mag, kw, fam="mutated")


def test_adam_emulation_passes_and_mutations_fail():
    g = _g(10)
    n, lr = 20000, 1e-3
    p = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 7 - 6)
    m0, v0 = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-3
    z = torch.zeros(n)
    for t, m, v, gs in [(1, z, z, 1.0), (2, m0, v0, 1.0), (1000, m0, v0, 0.25), (150000, m0, v0, 1.0)]:
        p1, m1, v1 = adam_f32(p, m, v, grad, t, lr, gs)
        for fam, r in zip(("adam m", "adam v", "adam p"), T.check_adam(p1, m1, v1, p, m, v, grad, t, lr, gs)):
            note(fam, r)
    # 1.f - 0.999f formed in float, at step 1 from m = v = 0: the 4.7e-5 of adam_apply's comment
    p1, m1, v1 = adam_f32(p, z, z, grad, 1, lr, mut="one_minus_beta")
    (_, _), (rv, mv), (rp, um) = T.adam(p, z, z, grad, 1, lr)
    _fails(R.check_f32, v1, rv, mv)
    _fails(T.check_param, p1, rp, um)
    # the bias correction of step t - 1; grad_scale ignored
    p1, m1, v1 = adam_f32(p, m0, v0, grad, 1000, lr, mut="bias_t")
    _fails(T.check_param, p1, T.adam(p, m0, v0, grad, 1000, lr)[2][0], T.adam(p, m0, v0, grad, 1000, lr)[2][1])
    _fails(T.check_adam, *adam_f32(p, m0, v0, grad, 2, lr, 0.25, mut="grad_scale"), p, m0, v0, grad, 2, lr, 0.25)


def test_noise_out4_and_slab_sums_emulation():
    g = _g(11)
    n = 1000
    y, ys, z2 = (torch.randn(n, generator=g) for _ in range(3))
    eps = T.eps_of(0.75, -3.0)
    for sig in (None, ys):
        got = y + torch.exp(0.5 * t32(eps)) * z2
        if sig is not None:
            got = got + 1.0 / (1.0 + torch.exp(-sig))
        note("add_noise", R.check_f32(got, *T.add_noise(y, sig, z2, eps)))
    _fails(R.check_f32, y + torch.exp(t32(eps)) * z2, *T.add_noise(y, None, z2, eps))
    slabs = torch.randn(1024, 17, generator=g)
    grp = torch.stack([seq_sum(slabs[i:i + 32], 32) for i in range(0, 1024, 32)])
    note("sum_slabs", R.check_f32(seq_sum(grp, 32), *T.sum_slabs(slabs, 1024, 17)))
    _fails(R.check_f32, seq_sum(grp, 31), *T.sum_slabs(slabs, 1024, 17))
    # out4: the loss terms from 500 partial rows
    kw = finalize_inputs(seed=12)
    e, lv = torch.rand(500, 4, generator=g) * 50.0, kw["params"][kw["off_epsp"]:kw["off_epsp"] + 20]
    t = T.loss_terms(e, lv, eps, 1000.0, 7, INV_BT)
    klc = (1.0 + lv - torch.exp(lv)).sum()
    dkl = (0.5 * e[:, 1].sum() - 0.5 * t32(1000.0) * klc) * t32(INV_BT)
    mse = (e[:, 0].sum() + 0.5 * t32(1000.0) * t32(7.0) * (t32(T.LOG2PI) + t32(eps))) * t32(INV_BT)
    deps = (e[:, 2].sum() + 0.5 * t32(1000.0) * t32(7.0)) * t32(INV_BT)
    for name, got in (("loss", dkl + mse), ("dkl", dkl), ("mse", mse), ("deps", deps)):
        note("out4", R.check_f32(got, *t[name]))


def test_positive_controls_stay_below_half_the_bound():
    """Runs last in this file: every family the emulations filled in is below 0.5 from the float32 side alone."""
    for sig in (False, True):
        test_elbo_emulation_passes_and_mutations_fail(sig)
    test_d_sig_bound_is_relative_to_one_plus_sg()
    test_elbo_reduce_emulation()
    test_reparam_bwd_emulation_passes_and_mutations_fail()
    for e in (True, False):
        test_finalize_emulation_passes_and_mutations_fail(e)
    test_adam_emulation_passes_and_mutations_fail()
    test_noise_out4_and_slab_sums_emulation()
    fams = {k: v for k, v in RATIOS.items() if not k.startswith("mutated")}
    print("\n".join(f"{k:28s} {v:.3f}" for k, v in sorted(fams.items())))
    assert len(fams) >= 15 and max(fams.values()) < 0.5, fams


# ---- vaek_debug_tail validates on the host -------------------------------------------------------------------------------------
def test_debug_tail_validates_before_launching():
    from vae_training_amd import _lib
    fn = T.bind(_lib.load())
    p = 4096          # a non-null address nothing reads: every call below stops before a launch
    OP = T.TAIL_OP

    def rc(op, **kw):
        a = T.tail_args(**kw)
        return fn(None, OP[op] if isinstance(op, str) else op, a, None), a

    elbo = dict(rows=257, D=7, L=6, S=3, rows_per_split=128, x=p, y_lin=p, z2=p, mu=p, partial=p)
    assert rc("elbo", **elbo)[0] == 0 and rc("elbo", **elbo)[1].scratch_bytes == 0
    assert rc("elbo", **elbo, y_sig=p, d_lin=p, d_sig=p, eps_param=p, step_dev=p)[0] == 0
    for bad in (dict(S=2), dict(S=4), dict(rows_per_split=0), dict(x=None), dict(partial=None), dict(mu=None), dict(D=0)):
        assert rc("elbo", **{**elbo, **bad})[0] == -1, bad
    assert rc("elbo", **elbo, y_sig=p, d_lin=p)[0] == -1          # a sigmoid decoder's gradients need d_sig
    assert rc("elbo", **elbo, d_sig=p)[0] == -1
    red = dict(rows=257, L=6, S=2, rows_per_split=256, bm=128, nbx=5, part=p, mu=p, partial=p)
    assert rc("elbo_reduce", **red)[0] == 0
    for bad in (dict(rows_per_split=192, bm=128), dict(S=3), dict(part=None), dict(bm=0), dict(nbx=0)):
        assert rc("elbo_reduce", **{**red, **bad})[0] == -1, bad
    rp = dict(rows=129, L=256, S=2, rows_per_split=128, dsamp=p, mu=p, z1=p, partial=p)
    assert rc("reparam_bwd", **rp)[0] == 0
    for bad in (dict(L=257), dict(S=1), dict(dsamp=None), dict(z1=None)):
        assert rc("reparam_bwd", **{**rp, **bad})[0] == -1, bad
    fin = dict(L=20, D=7, S=4, Se=3, nseg=2, seg_end=[40, 100], seg_S=[4, 2], P=121, off_epsp=100, off_eps=120, slab_stride=128,
               slabs=p, epart=p, rpart=p, params=p, grads=p, rows_f=300.0)
    adam = dict(params_rw=p, m=p, v=p, step_dev=p)
    assert rc("finalize", **fin)[0] == 0 and rc("finalize", **fin, hi=100)[0] == 0 and rc("finalize", **fin, lo=100)[0] == 0
    assert rc("finalize", **fin, **adam, fuse=1)[0] == 0
    assert rc("finalize", **{**fin, "L": 59, "P": 160, "off_eps": 159}, **adam, fuse=1)[0] == 0
    assert rc("finalize", **{**fin, "L": 60, "P": 161, "off_eps": 160}, **adam, fuse=1)[0] == -1      # fuse with L = 60
    assert rc("finalize", **{**fin, "L": 60, "P": 161, "off_eps": 160}, **adam, fuse=0)[0] == 0
    for bad in (dict(seg_end=[100, 40]), dict(seg_end=[40, 40]), dict(seg_end=[40, 101]), dict(hi=64), dict(hi=121), dict(lo=64),
                dict(hi=100, lo=100), dict(P=120), dict(off_eps=-1), dict(nseg=33), dict(grads=None), dict(slabs=None),
                dict(params=None), dict(fuse=1), dict(params_rw=p), dict(seg_S=[4, 0]), dict(slab_stride=99),
                dict(loss_hist=p, loss_hist_cap=0)):
        assert rc("finalize", **{**fin, **bad})[0] == -1, bad
    assert rc("finalize", **{**fin, "off_eps": -1, "P": 120})[0] == 0
    assert rc("finalize", **{**fin, **adam, "params_rw": 8192})[0] == -1
    assert rc("out4", S=5, L=2, D=3, partial=p, out=p, lv=p, want_deps=1)[0] == 0
    assert rc("out4", S=5, L=2, D=3, partial=p, out=p, lv=p, want_deps=0)[0] == -1
    assert rc("out4", S=5, L=2, D=3, partial=p, out=p, params=p, off_eps=-1)[0] == 0
    assert rc("out4", S=0, L=2, D=3, partial=p, out=p, params=p)[0] == -1
    assert rc("add_noise", n=5, y_lin=p, z2=p, out=p)[0] == 0 and rc("add_noise", n=5, y_lin=p, z2=p)[0] == -1
    assert rc("add_noise", n=0, y_lin=p, z2=p, out=p)[0] == -1
    assert rc("sum_slabs_inplace", n=17, S=128, slab_stride=17, slabs=p, out=p)[0] == 0
    assert rc("sum_slabs_inplace", n=17, S=128, slab_stride=16, slabs=p, out=p)[0] == -1
    assert rc("sum_slabs", n=17, S=3, slab_stride=17, slabs=p, out=p)[0] == 0
    assert rc(8, n=1)[0] == -1 and rc(-1, n=1)[0] == -1
    # scratch: nothing is needed, but what is given must be aligned; a launch needs a context
    a = T.tail_args(**elbo, scratch=p + 4, scratch_bytes=256)
    assert fn(None, OP["elbo"], a, None) == -4
    a = T.tail_args(**elbo, scratch=p, scratch_bytes=256)
    assert fn(None, OP["elbo"], a, None) == -1
    assert fn(None, OP["elbo"], None, None) == -1
