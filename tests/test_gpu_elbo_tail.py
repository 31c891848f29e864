"""-m gpu: every kernel of the step's tail (csrc/elbo.hip), one call at a time, output by output against the float64 references of
tests/elbo_tail_ref.py.  The calls go through vaek_debug_tail (csrc/debug_tail.hip) -- the step's own launch functions, for the
finalisation the step's own launch sequence (finalize_launches, api.hip) on segment tables made by hand -- and through the public
block entries (vaek_adam_step, vaek_reparam_bwd, vaek_elbo_fwd_bwd[_dev]).  Every debug call asserts the profiler labels it ran, every
output lies between guard bands (dense16_ref.guarded), inputs and outputs start 0-3 floats off their buffer's alignment, and every
area a kernel must not read (slabs beyond a layer's own count, partial rows beyond Se, tiles beyond the last tile row) holds the
guard's NaN: one read too many gives a NaN output, one too few misses a term of the reference."""
import ctypes as C

import pytest
import torch

from tests import dense16_ref as R
from tests import elbo_tail_ref as T
from tests import test_gpu_dense16 as T16
from tests.gpu_util import engine_for
from tests.test_gpu_dense32 import DENSE32, ROUTING, output, shifted
from oracle import elbo_oracle as O

pytestmark = pytest.mark.gpu

seed, randn = T16.seed, T16.randn
# every label the calls of this file hold to a reference
TAIL = {"elbo", "elbo_reduce", "reparam_bwd", "finalize", "finalize_adam", "bulk_finalize", "bulk_finalize_adam", "adam", "out4",
        "add_noise", "sum_slabs", "sum_slab_groups"}
INV_BT = T.f32(1.0 / 777.0)          # rows != batch_total everywhere
FILL = R.GUARD_FILL


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    T16.dump_ratios()


@pytest.fixture(scope="module")
def eng():
    e = engine_for(O.Config(6, 6, (64, 64), (64, 64), -3.0, True, "sphere"), 1024)
    e.tail = T.bind(e.lib)
    e.scratch = torch.zeros(256, dtype=torch.uint8, device="cuda")
    return e


def note(fam, ratio):
    T16.RATIOS["tail " + fam] = max(T16.RATIOS.get("tail " + fam, 0.0), ratio)


def call(eng, op, expect, **kw):
    """One vaek_debug_tail call (the query first); the kernels it ran carry exactly the labels `expect`."""
    a = T.tail_args(**kw)
    assert eng.tail(eng.h, T.TAIL_OP[op], a, None) == 0, eng.lib.vaek_last_error()
    assert a.scratch_bytes == 0
    a.scratch, a.scratch_bytes = eng.scratch.data_ptr(), eng.scratch.numel()
    eng.profile_begin(16)
    rc = eng.tail(eng.h, T.TAIL_OP[op], a, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rep = eng.profile_report()
    assert rc == 0, eng.lib.vaek_last_error()
    assert set(rep) == set(expect), (op, sorted(rep), sorted(expect))
    assert set(rep) <= TAIL


def public(fn):
    """A public block entry (vaek_adam_step, vaek_reparam_bwd, vaek_elbo_fwd_bwd): these do not bind the context's profiler, so there
    is no label to assert -- each reaches its one launcher unconditionally (api.hip)."""
    out = fn()
    torch.cuda.synchronize()
    return out


def filled(values, lead=0):
    """A guarded buffer holding `values`: (buffer, view of their shape).  What lies behind the view reads as NaN."""
    buf, v = output(tuple(values.shape), lead, init=values)
    return buf, v


def bits(t):
    return t.contiguous().view(torch.int32)


def mixed(*shape, lo=-3.0, hi=1.0):
    """Random signs, magnitudes 10^U(lo, hi)."""
    u = torch.rand(*shape, generator=T16._gen[0], device="cuda") * (hi - lo) + lo
    return torch.sign(randn(*shape)) * 10.0 ** u


# ---- elbo ---------------------------------------------------------------------------------------------------------------------
ELBO_ROWS = [(1, 1), (5, 2), (129, 3), (129, 128), (257, 128), (257, 192), (1000, 2), (1000, 128), (1000, 1024)]
EPS_VARIANTS = [(0.75, -3.0), (None, -2.0)]
ELBO_L = 5


def elbo_case(eng, rows, D, rps, sig, epsv, modes=("inplace", "separate", "nograds"), offs=({},)):
    seed("elbo", rows, D, rps, sig, epsv)
    x, y_lin, z2, mu = randn(rows, D), randn(rows, D), randn(rows, D), randn(rows, ELBO_L)
    y_sig = randn(rows, D, scale=2.5) if sig else None
    ep, cli = epsv
    eps = T.eps_of(ep, cli)
    epsp = torch.tensor([ep], device="cuda") if ep is not None else None
    y, mag, (rl, ml), rs = T.elbo_elements(x, y_lin, y_sig, z2, eps, INV_BT)
    pref, pbound = T.elbo_partials(y, mag, x, z2, mu, eps, rps)
    S = T.n_splits(rows, rps)
    fam = "elbo sig" if sig else "elbo"
    for off in offs:
        o = lambda k: off.get(k, 0)
        for mode in modes:
            what = f"elbo rows={rows} D={D} rps={rps} sig={sig} eps={eps} {mode} off={off}"
            grads = mode != "nograds"
            ins = {k: shifted(t, o(k)) for k, t in (("x", x), ("z2", z2), ("mu", mu))}
            by, yl = filled(y_lin, o("y_lin"))
            bs, ys = filled(y_sig, o("y_sig")) if sig else (None, None)
            bp, part = output((S, 4))
            kw = dict(ins, y_lin=yl, partial=part)
            if sig:
                kw["y_sig"] = ys
            if mode == "inplace":
                dl, ds, bdl, bds = yl, ys, by, bs
            elif mode == "separate":
                bdl, dl = output((rows, D), o("d_lin"))
                bds, ds = output((rows, D), o("d_sig")) if sig else (None, None)
            if grads:
                kw["d_lin"] = dl
                if sig:
                    kw["d_sig"] = ds
            step = torch.tensor([41], dtype=torch.int32, device="cuda") if mode == "inplace" else None
            if step is not None:
                kw["step_dev"] = step
            if epsp is not None:
                kw["eps_param"] = epsp
            call(eng, "elbo", {"elbo"}, rows=rows, D=D, L=ELBO_L, S=S, rows_per_split=rps, eps_cli=cli, inv_bt=INV_BT, **kw)
            R.check_guard(bp, part, what=what + " partial")
            note(fam + " partials", T.check_partials(part, pref, pbound, what=what))
            assert step is None or int(step) == 42, what
            for k, t in (("x", x), ("z2", z2), ("mu", mu)):
                assert torch.equal(ins[k], t), what + f": {k} was written"
            if grads:
                R.check_guard(bdl, dl, what=what + " d_lin")
                note(fam + " d_lin", R.check_f32(dl, rl, ml, what=what + " d_lin"))
                if sig:
                    R.check_guard(bds, ds, what=what + " d_sig")
                    note(fam + " d_sig", R.check_f32(ds, rs[0], rs[1], what=what + " d_sig"))
            if mode != "inplace":          # nothing but the outputs was written
                R.check_guard(by, yl, prefilled=True, what=what + " y_lin")
                assert torch.equal(yl, y_lin), what + ": y_lin was written"
                if sig:
                    R.check_guard(bs, ys, prefilled=True, what=what + " y_sig")
                    assert torch.equal(ys, y_sig), what + ": y_sig was written"


@pytest.mark.parametrize("rows,rps", ELBO_ROWS)
def test_elbo(eng, rows, rps):
    """All four <SIG, GRADS> variants, in place and into separate outputs, eps_param given and eps_cli alone."""
    for D in (1, 3, 4, 7, 33):
        for sig in (False, True):
            for epsv in EPS_VARIANTS:
                elbo_case(eng, rows, D, rps, sig, epsv)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("D", [7, 4])
def test_elbo_unaligned(eng, D, off):
    names = ("x", "y_lin", "y_sig", "z2", "d_lin", "d_sig", "mu")
    elbo_case(eng, 257, D, 128, True, EPS_VARIANTS[0], modes=("separate",), offs=tuple({n: off} for n in names))
    elbo_case(eng, 257, D, 128, True, EPS_VARIANTS[1], modes=("inplace", "nograds"), offs=tuple({n: off} for n in ("y_lin", "y_sig", "x")))
    elbo_case(eng, 257, D, 128, False, EPS_VARIANTS[0], modes=("inplace", "separate"), offs=tuple({n: off} for n in ("y_lin", "z2", "d_lin")))


# ---- elbo_reduce --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,rps,bm,nbx", [(1, 128, 32, 1), (129, 128, 64, 2), (257, 256, 128, 5), (1000, 128, 64, 1), (1000, 256, 128, 2),
                                             (4097, 2048, 64, 9)])
def test_elbo_reduce(eng, rows, rps, bm, nbx):
    seed("reduce", rows, rps, bm, nbx)
    ntr, S, L = (rows + bm - 1) // bm, T.n_splits(rows, rps), 6
    _, part = filled(mixed(ntr, nbx, 2))          # behind the last real tile row: the guard's NaN
    mu = randn(rows, L)
    ref, bound = T.tile_partials(part, bm, nbx, mu, rows, rps)
    for with_step in (False, True):
        bp, out = output((S, 4))
        step = torch.tensor([6], dtype=torch.int32, device="cuda")
        kw = dict(step_dev=step) if with_step else {}
        call(eng, "elbo_reduce", {"elbo_reduce"}, rows=rows, L=L, S=S, rows_per_split=rps, bm=bm, nbx=nbx, part=part, mu=mu, partial=out, **kw)
        what = f"elbo_reduce rows={rows} rps={rps} bm={bm} nbx={nbx}"
        R.check_guard(bp, out, what=what)
        note("elbo_reduce", T.check_partials(out, ref, bound, what=what))
        assert int(step) == (7 if with_step else 6)


# ---- reparam_bwd --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 6, 20, 32, 33, 64, 100, 128, 129, 255, 256])
def test_reparam_bwd(eng, L):
    for rows, rps in [(1, 128), (5, 128), (129, 128), (1000, 128), (1000, 334)]:
        seed("rbwd", L, rows, rps)
        d, mu, z1 = randn(rows, L), randn(rows, L), randn(rows, L)
        S = T.n_splits(rows, rps)
        (r1, m1), (r2, m2) = T.reparam_bwd(d, mu, z1, INV_BT, rps)
        for lead in (0, 1):
            bd, ds = filled(d, lead)
            bp, part = output((S, L), lead)
            call(eng, "reparam_bwd", {"reparam_bwd"}, rows=rows, L=L, S=S, rows_per_split=rps, inv_bt=INV_BT, dsamp=ds, mu=shifted(mu, lead),
                 z1=shifted(z1, 3 * lead), partial=part)
            what = f"reparam_bwd L={L} rows={rows} rps={rps} lead={lead}"
            R.check_guard(bd, ds, what=what + " dmu")
            R.check_guard(bp, part, what=what + " partial")
            note("reparam_bwd dmu", R.check_f32(ds, r1, m1, what=what + " dmu"))
            note("reparam_bwd partials", R.check_f32(part, r2, m2, what=what + " partial"))


@pytest.mark.parametrize("L", [6, 256])
@pytest.mark.parametrize("double_bt", [False, True])
def test_public_reparam_bwd(eng, L, double_bt):
    """vaek_reparam_bwd on a context of L = 6: at L = 256 the entry shrinks its split count to what the partial area holds."""
    rows = 1000
    seed("prbwd", L, double_bt)
    d, mu, z1, lv = randn(rows, L), randn(rows, L), randn(rows, L), randn(L, scale=0.5)
    bt = 2 * rows if double_bt else 0
    inv_bt, rob = T.f32(1.0 / (bt or rows)), T.f32(rows / (bt or rows))
    (r1, m1), (r2, m2) = T.reparam_bwd(d, mu, z1, inv_bt, rows)
    rg, mg = T.d_logvar(r2[0], m2[0], lv, rob)
    outs = []
    for _ in range(2):
        bd, ds = filled(d)
        bg, g = output((L,))
        public(lambda: eng.reparam_bwd(ds, mu, z1, lv, batch_total=bt, out=g))
        R.check_guard(bd, ds)
        R.check_guard(bg, g)
        note("reparam_bwd dmu", R.check_f32(ds, r1, m1, what="public dmu"))
        note("reparam_bwd d_logvar", R.check_f32(g, rg, mg, what="public d_logvar_e"))
        outs.append((ds, g))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- finalize -----------------------------------------------------------------------------------------------------------------
def fin_labels(hi, adam, fuse):
    s = {"finalize_adam" if adam and fuse else "finalize"}
    if hi:
        s.add("bulk_finalize_adam" if adam else "bulk_finalize")
    if adam and not fuse:
        s.add("adam")
    return s


def fin_case(eng, segs, L, Se, with_eps=True, rob=1.0, hi=0, lo=0, ts=(), leads=(0, 0, 0, 0), ring="step", D=7, tag=""):
    """One hand-made finalisation: grads only, then with Adam at every t of `ts`.  segs: [(end, slab count)], the last end = off_epsp.
    leads: float offsets of (grads, params, m, v)."""
    off_epsp = segs[-1][0]
    off_eps = off_epsp + L if with_eps else -1
    P = off_epsp + L + (1 if with_eps else 0)
    seed("fin", segs, L, Se, with_eps, rob, hi, lo, tag)
    Smax = max(c for _, c in segs)
    stride = (off_epsp + 63) // 64 * 64
    slabs = torch.full((Smax + 1, stride), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    start = 0
    for end, cnt in segs:          # a layer's slabs beyond its own count keep the NaN fill
        slabs[:cnt, start:end] = mixed(cnt, end - start, lo=-2.0, hi=1.0)
        start = end
    ep = torch.rand(Se, 4, generator=T16._gen[0], device="cuda") * 100.0
    ep[:, 2] -= 60.0
    ep[:, 3] = 0.0
    _, epart = filled(ep)
    _, rpart = filled(randn(Se, L))
    p0 = randn(P, scale=0.5)
    rows = 300.0
    rob32 = T.f32(rob)
    fam = "bulk_finalize" if hi else "finalize"
    common = dict(L=L, D=D, S=Smax, Se=Se, nseg=len(segs), seg_end=[e for e, _ in segs], seg_S=[c for _, c in segs], P=P,
                  off_epsp=off_epsp, off_eps=off_eps, slab_stride=stride, slabs=slabs, epart=epart, rpart=rpart, eps_cli=-3.0,
                  inv_bt=INV_BT, rows_over_bt=rob32, rows_f=rows, hi=hi, lo=lo)
    ref, mag = T.finalize(slabs, segs, Smax, epart, rpart, p0, off_epsp, off_eps, L, D, -3.0, rob32, INV_BT, rows)
    zero = torch.zeros(P + 4, dtype=torch.bool, device="cuda")
    zero[P + 3] = True
    groups = {"weights": slice(0, off_epsp), "epsilon_p": slice(off_epsp, off_epsp + L), "loss": slice(P, P + 3)}
    if with_eps:
        groups["epsilon"] = slice(off_eps, off_eps + 1)

    def check_grads(bg, g, what):
        if lo:          # the bucketed tail: below the floor nothing is stored
            R.check_guard(bg, g, prefilled=True, what=what)
            assert int((bits(g[:lo]) != FILL).sum()) == 0, what + ": stored below lo"
            assert int((bits(g[lo:]) == FILL).sum()) == 0, what + ": outputs above lo left unstored"
        else:
            R.check_guard(bg, g, what=what)
        R.check_f32(g[lo:], ref[lo:], mag[lo:], zero=zero[lo:], what=what)
        for name, sl in groups.items():
            if sl.start >= lo:
                note(f"{fam} {name}", R.check_f32(g[sl], ref[sl], mag[sl], what=f"{what} {name}"))

    what = f"finalize{tag} segs={segs} L={L} Se={Se} eps={with_eps} rob={rob} hi={hi} lo={lo} leads={leads}"
    # grads only; the loss ring with a step counter (slot (t - 1) % cap), without one, and no ring
    bg, g = output((P + 4,), leads[0])
    bpp, prm = filled(p0, leads[1])
    cap = 5
    hist = torch.full((cap,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    kw = dict(common, params=prm, grads=g)
    if ring == "step":
        kw.update(step_dev=torch.tensor([13], dtype=torch.int32, device="cuda"), loss_hist=hist, loss_hist_cap=cap)
    elif ring == "nostep":
        kw.update(loss_hist=hist, loss_hist_cap=cap)
    call(eng, "finalize", fin_labels(hi, False, False), **kw)
    check_grads(bg, g, what)
    assert torch.equal(prm, p0), what + ": params written without Adam"
    slot = 12 % cap if ring == "step" else -1
    for k in range(cap):
        assert int(bits(hist)[k]) == (int(bits(g)[P]) if k == slot else FILL), (what, "loss ring", k)
    # with Adam from a nonzero state, held to the float64 step from the gradient the kernel stored
    fuse = L + 5 <= 64
    for t in ts:
        m0, v0 = randn(P, scale=0.01), torch.rand(P, generator=T16._gen[0], device="cuda") * 1e-3
        bg, g = output((P + 4,), leads[0])
        bpp, prm = filled(p0, leads[1])
        bm, m = filled(m0, leads[2])
        bv, v = filled(v0, leads[3])
        step = torch.tensor([t], dtype=torch.int32, device="cuda")
        hist = torch.full((cap,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
        call(eng, "finalize", fin_labels(hi, True, fuse), **dict(common, params=prm, grads=g, params_rw=prm, m=m, v=v, step_dev=step, lr=1e-3,
                                                               fuse=int(fuse), loss_hist=hist, loss_hist_cap=cap))
        w = f"{what} adam t={t}"
        check_grads(bg, g, w)
        for b, view, n in ((bpp, prm, "params"), (bm, m, "m"), (bv, v, "v")):
            R.check_guard(b, view, prefilled=True, what=f"{w} {n}")
        rm, rv, rp = T.check_adam(prm, m, v, p0, m0, v0, g[:P], t, 1e-3, what=w)
        for n, r in (("m", rm), ("v", rv), ("p", rp)):
            note(f"{fam} adam {n}", r)
        assert int(step) == t
        assert int(bits(hist)[(t - 1) % cap]) == int(bits(g)[P]) and int((bits(hist) != FILL).sum()) == 1, w + " loss ring"


def table(off_epsp):
    """Five layers with slab counts 4, 9, 64, 1, 9 (a two-element layer among them), the last ending at off_epsp."""
    return [(40, 4), (47, 9), (49, 64), (130, 1), (off_epsp, 9)]


ADAM_TS = (1, 2, 1000, 150000)


def test_finalize_one_block(eng):
    """P + 4 < 64: a linear model of D = 3, L = 2."""
    for with_eps in (True, False):
        for rob in (1.0, 0.5):
            fin_case(eng, [(8, 1), (17, 4)], 2, 1, with_eps=with_eps, rob=rob, ts=ADAM_TS, D=3)


# P + 4 = off_epsp + L + 1 + 4 with epsilon: 0, 1 and 63 (mod 64) at L = 20
@pytest.mark.parametrize("off_epsp,Se", [(167, 7), (168, 128), (166, 129)])
def test_finalize_block_edges(eng, off_epsp, Se):
    assert (off_epsp + 25) % 64 in (0, 1, 63)
    fin_case(eng, table(off_epsp), 20, Se, rob=0.5, ts=ADAM_TS[:2])
    fin_case(eng, table(off_epsp), 20, Se, with_eps=False, ring="nostep", ts=ADAM_TS[2:])


@pytest.mark.parametrize("L", [2, 20, 59, 60, 100, 256])
def test_finalize_latent_widths(eng, L):
    """59: the last fused Adam; 60: the first separate adam launch; 100 and 256: epsilon_p in blocks other than 0."""
    for with_eps, Se, rob, ring in ((True, 1000, 0.5, "step"), (False, 7, 1.0, "none")):
        fin_case(eng, table(171), L, Se, with_eps=with_eps, rob=rob, ring=ring, ts=(1, 1000))


def test_finalize_unaligned(eng):
    for k in (1, 2, 3):
        fin_case(eng, table(171), 20, 7, ts=(2,), leads=(k, (k + 1) % 4, (k + 2) % 4, (k + 3) % 4))


@pytest.mark.parametrize("L", [6, 100])
def test_finalize_bucketed_tail(eng, L):
    """lo = off_epsp: grads below it keep the fill bit for bit."""
    for with_eps in (True, False):
        fin_case(eng, table(300), L, 129, with_eps=with_eps, rob=0.5, lo=300)


# bulk: layer boundaries at offsets 1, 2 and 3 (mod 4) with different counts on the two sides, a 9-slab layer, hi % 4 != 0
BULK_TABLE = [(41, 4), (86, 9), (131, 1), (1200, 64), (2307, 3)]


@pytest.mark.parametrize("L", [20, 60])
def test_bulk_finalize(eng, L):
    for with_eps in (True, False):
        fin_case(eng, BULK_TABLE, L, 129, with_eps=with_eps, rob=0.5, hi=2307, ts=ADAM_TS)
    fin_case(eng, [(e + 1 if e == 2307 else e, c) for e, c in BULK_TABLE], L, 7, hi=2308, ts=(2,))


def test_bulk_finalize_unaligned(eng):
    """grads, params, m and v in turn 1-3 floats off: the scalar branch."""
    for k in (1, 2, 3):
        for which in range(4):
            leads = tuple(k if j == which else 0 for j in range(4))
            fin_case(eng, BULK_TABLE, 20, 7, hi=2307, ts=(2,), leads=leads)


@pytest.mark.parametrize("middle,neighbours", [(9, 4), (4, 9), (64, 1), (1, 64)])
def test_bulk_finalize_two_element_layer_inside_one_float4(eng, middle, neighbours):
    """A 1 -> 1 layer (one weight, one bias) at offsets 41 and 42, inside the float4 unit 40..43 whose two ends belong to layers with
    the same slab count: its two outputs are sums over ITS slabs.  (Before this case existed bulk_finalize_kernel compared the slab
    counts of the unit's two ends only and summed the layer over its neighbours' count: NaN from the slabs it never wrote with the
    larger count, missing terms with the smaller.)"""
    segs = [(41, neighbours), (43, middle), (1200, neighbours), (2304, 9)]
    fin_case(eng, segs, 20, 7, hi=2304, ts=(1, 1000), tag=" two-element")
    fin_case(eng, segs, 20, 7, hi=0, ts=(2,), tag=" two-element, 64-output kernel")


# ---- adam (vaek_adam_step) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 524291])
def test_adam_step(eng, n):
    """Five steps, each against the float64 step from the kernel's own previous float32 state."""
    for gs in (1.0, 0.25):
        for use_dev in (False, True):
            for lead in ((0, 1, 2, 3) if n == 257 else (0, 3) if n == 1 else (0,)):
                seed("adam", n, gs, use_dev, lead)
                bp, p = filled(randn(n, scale=0.05), lead)
                bm, m = filled(torch.zeros(n, device="cuda"), (lead * 2) % 4)
                bv, v = filled(torch.zeros(n, device="cuda"), (lead * 3) % 4)
                step = torch.zeros(1, dtype=torch.int32, device="cuda")
                for t in range(1, 6):
                    g = shifted(mixed(n, lo=-6.0, hi=1.0), lead)
                    p0, m0, v0 = p.clone(), m.clone(), v.clone()
                    step.fill_(t)
                    fn = lambda: eng.adam_step(p, g, m, v, 1e-3, step=None if use_dev else t, step_dev=step if use_dev else None, grad_scale=gs)
                    public(fn)
                    what = f"adam n={n} grad_scale={gs} step_dev={use_dev} lead={lead} t={t}"
                    for b, view in ((bp, p), (bm, m), (bv, v)):
                        R.check_guard(b, view, prefilled=True, what=what)
                    for name, r in zip("mvp", T.check_adam(p, m, v, p0, m0, v0, g, t, 1e-3, gs, what=what)):
                        note(f"adam {name}", r)


# ---- out4, add_noise, the slab sums -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 20, 256])
@pytest.mark.parametrize("S", [1, 63, 65, 500])
def test_out4(eng, S, L):
    seed("out4", S, L)
    D, rows = 7, 300.0
    ep = torch.rand(S, 4, generator=T16._gen[0], device="cuda") * 100.0
    ep[:, 2] -= 60.0
    _, part = filled(ep)
    lv = randn(L, scale=0.5)
    for epp in (0.75, None):
        eps = T.eps_of(epp, -3.0)
        t = T.loss_terms(part, lv, eps, rows, D, INV_BT)
        # launch_elbo_out4: lv and eps_param by pointer, out4[3] = d eps
        bo, out = output((4,))
        kw = dict(eps_param=torch.tensor([epp], device="cuda")) if epp is not None else {}
        call(eng, "out4", {"out4"}, S=S, L=L, D=D, want_deps=1, partial=part, lv=lv, out=out, eps_cli=-3.0, inv_bt=INV_BT, rows_f=rows, **kw)
        R.check_guard(bo, out)
        for k, name in enumerate(("loss", "dkl", "mse", "deps")):
            note("out4", R.check_f32(out[k], *t[name], what=f"out4 S={S} L={L} {name}"))
        # launch_eval_out4: lv and epsilon inside params, out4[3] = eps
        off_epsp = 11
        params = randn(off_epsp + L + 1)
        params[off_epsp:off_epsp + L] = lv
        if epp is not None:
            params[off_epsp + L] = epp
        bo, out = output((4,))
        call(eng, "out4", {"out4"}, S=S, L=L, D=D, want_deps=0, partial=part, params=params, off_epsp=off_epsp,
             off_eps=off_epsp + L if epp is not None else -1, out=out, eps_cli=-3.0, inv_bt=INV_BT, rows_f=rows)
        R.check_guard(bo, out)
        for k, name in enumerate(("loss", "dkl", "mse")):
            note("out4", R.check_f32(out[k], *t[name], what=f"eval out4 S={S} L={L} {name}"))
        assert float(out[3]) == eps


@pytest.mark.parametrize("n", [1, 1000, 524291])
def test_add_noise(eng, n):
    seed("noise", n)
    y, ys, z2 = randn(n), randn(n, scale=2.5), randn(n)
    for sig in (None, ys):
        for epp, cli in EPS_VARIANTS:
            for lead in (0, 1):
                bo, out = output((n,), lead)
                kw = dict(eps_param=torch.tensor([epp], device="cuda")) if epp is not None else {}
                if sig is not None:
                    kw["y_sig"] = shifted(sig, lead)
                call(eng, "add_noise", {"add_noise"}, n=n, y_lin=shifted(y, (lead * 2) % 4), z2=z2, out=out, eps_cli=cli, **kw)
                R.check_guard(bo, out)
                note("add_noise", R.check_f32(out, *T.add_noise(y, sig, z2, T.eps_of(epp, cli)), what=f"add_noise n={n}"))


@pytest.mark.parametrize("S,n", [(127, 17), (128, 17), (1024, 544), (129, 1)])
def test_sum_slabs_inplace(eng, S, n):
    """Groups of 32 slabs, the last one short (129: one slab), against the plain sum_slabs on a copy and the same reference."""
    seed("slabs", S, n)
    stride = n + 3
    vals = mixed(S, stride)
    ref, mag = T.sum_slabs(vals, S, n)
    grouped = S >= 128
    for op, labels in (("sum_slabs_inplace", {"sum_slab_groups", "sum_slabs"} if grouped else {"sum_slabs"}), ("sum_slabs", {"sum_slabs"})):
        bs, sl = filled(vals)
        bo, out = output((n,))
        call(eng, op, labels, S=S, n=n, slab_stride=stride, slabs=sl, out=out)
        R.check_guard(bo, out, what=op)
        R.check_guard(bs, sl, prefilled=True, what=op + " slabs")
        note(op, R.check_f32(out, ref, mag, what=f"{op} S={S} n={n}"))
        if op == "sum_slabs":
            assert torch.equal(sl, vals)
        else:          # only the first slab of each group may be rewritten, and only its first n floats
            keep = torch.ones_like(vals, dtype=torch.bool)
            if grouped:
                keep[::32, :n] = False
            assert torch.equal(sl[keep], vals[keep])


# ---- the public block entry once more, element by element ---------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,L", [(5, 3, 2), (777, 33, 9)])
def test_public_elbo_block(eng, rows, D, L):
    seed("block", rows, D, L)
    x, y_lin, y_sig, z2, mu, lv = randn(rows, D), randn(rows, D), randn(rows, D, scale=2.5), randn(rows, D), randn(rows, L), randn(L, scale=0.5)
    rps = max(1, (rows + 511) // 512)
    for sig in (None, y_sig):
        for epp in (None, 0.75):
            for bt in (0, 2 * rows):
                eps = T.eps_of(epp, -3.0)
                inv_bt = T.f32(1.0 / (bt or rows))
                y, mag, (rl, ml), rs = T.elbo_elements(x, y_lin, sig, z2, eps, inv_bt)
                pref, pbound = T.elbo_partials(y, mag, x, z2, mu, eps, rps)
                e4 = torch.cat([pref, torch.zeros_like(pref[:, :1])], 1)
                t = T.loss_terms(e4, lv, eps, float(rows), D, inv_bt)
                pb = pbound.sum(0) * inv_bt          # what the partial sums' own bounds leave on the outputs
                extra = {"loss": pb[0] + 0.5 * pb[1], "dkl": 0.5 * pb[1], "mse": pb[0], "deps": pb[2]}
                for grads in (True, False):
                    epsp = torch.tensor([epp], device="cuda") if epp is not None else None
                    out4, dl, ds = public(lambda: eng.elbo_fwd_bwd(x, y_lin, sig, z2, mu, lv, -3.0, batch_total=bt, grads=grads, eps_param=epsp))
                    what = f"block rows={rows} sig={sig is not None} eps_param={epp} bt={bt} grads={grads}"
                    for k, name in enumerate(("loss", "dkl", "mse", "deps")):
                        ref, m = t[name]
                        note("block out4", T.ratio_of(out4[k], ref, R.F32_TOL * m + extra[name], what=f"{what} {name}"))
                    if grads:
                        note("block d_lin", R.check_f32(dl, rl, ml, what=what + " d_lin"))
                        if sig is not None:
                            note("block d_sig", R.check_f32(ds, rs[0], rs[1], what=what + " d_sig"))
                    else:
                        assert dl is None and ds is None


# ---- routing: every kernel a layer-by-layer f32 step, eval and forward run is pinned here or in tests/test_gpu_dense32.py -----
@pytest.mark.parametrize("hidden,B,D,L,ds", [r for r in ROUTING if r[1] != 65536] + [((48,), 300, 6, 64, "sphere")])
def test_step_kernels_are_all_covered(hidden, B, D, L, ds):
    cfg = O.Config(D, L, hidden, hidden, -3.0, True, ds)
    eng = engine_for(cfg, B, force_generic=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    params = torch.randn(eng.P, generator=g, device="cuda") * 0.05
    grads, m, v = eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat()
    x, z1, z2 = (torch.randn(B, n, generator=g, device="cuda") for n in (D, L, D))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    events = [torch.cuda.Event() for _ in eng.buckets()]
    for e in events:
        e.record()
    torch.cuda.synchronize()
    seen = {}
    for name, fn in (("train_step", lambda: eng.train_step(params, grads, m, v, step, x, z1, z2, 1e-4)),
                     ("loss_eval", lambda: eng.loss_eval(params, x, z1, z2)),
                     ("forward", lambda: eng.forward(params, None, z1, z2, sampling=True)),
                     ("bucketed", lambda: eng.grads_bucketed(params, grads, step, x, z1, z2, events))):
        eng.profile_begin(512)
        fn()
        torch.cuda.synchronize()
        seen[name] = set(eng.profile_report())
        print(f"{hidden} B={B} D={D} L={L} {ds} {name}: {sorted(seen[name])}")
        assert seen[name] <= DENSE32 | TAIL, (name, sorted(seen[name] - DENSE32 - TAIL))
    assert torch.isfinite(grads).all() and torch.isfinite(params).all()
    assert int(step) == 2
    assert "out4" in seen["loss_eval"] and "add_noise" in seen["forward"] and "finalize" in seen["bucketed"]
    big = eng.P - L - 1 >= 65536
    want = {"bulk_finalize_adam"} if big else set()
    want |= {"finalize", "adam"} if L + 5 > 64 else {"finalize_adam"}
    assert want <= seen["train_step"], sorted(seen["train_step"])


def test_two_element_layer_of_a_real_context_end_to_end():
    """The context that reaches the float4 unit of test_bulk_finalize_two_element_layer_inside_one_float4 by itself: encoder 6 -> 4095
    -> 1 -> 1 -> 4096 -> 6 at B = 8192.  The 1 -> 1 layer starts at float 32 761 (1 mod 4), its neighbours plan another slab count than
    it does, and off_epsp >= 65 536 sends the weights through bulk_finalize.  Its two gradients against the oracle, by the per-leaf
    rule of tests/test_gpu_parity.py."""
    import numpy as np
    from tests.gpu_util import dev, host, random_problem, rel_err
    cfg, B = O.Config(6, 6, (4095, 1, 1, 4096), (), -3.0, True, "sphere"), 8192
    p, x, z1, z2 = random_problem(cfg, dict(name="sphere", seed=69, dd=3, pad=3), B)
    # keep the two one-unit layers alive behind their relus
    p["Encoder/FC1/bias"] = np.full((1,), 1.5)
    p["Encoder/FC2/kernel"] = np.full((1, 1), 0.75)
    p["Encoder/FC2/bias"] = np.full((1,), 0.25)
    _, g = O.loss_and_grad(cfg, p, x, z1, z2)
    want = O.flatten(cfg, g)
    eng = engine_for(cfg, B, force_generic=True)
    off, _ = eng.leaves["Encoder/FC2/kernel"]
    assert off == 32761 and eng.leaves["Encoder/FC2/bias"][0] == off + 1 and eng.P - cfg.L - 1 >= 65536
    assert abs(want[off]) > 0 and abs(want[off + 1]) > 0
    params = dev(O.flatten(cfg, p))
    grads = eng.new_flat(eng.grad_len)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.profile_begin(512)
    eng.grads_only(params, grads, step, dev(x), dev(z1), dev(z2))
    torch.cuda.synchronize()
    labels = set(eng.profile_report())
    assert "bulk_finalize" in labels and labels <= DENSE32 | TAIL, sorted(labels)
    got = host(grads)
    for n in ("Encoder/FC1/kernel", "Encoder/FC1/bias", "Encoder/FC2/kernel", "Encoder/FC2/bias", "Encoder/FC3/kernel", "Encoder/FC3/bias"):
        o, shape = eng.leaves[n]
        k = int(np.prod(shape))
        assert np.isfinite(got[o:o + k]).all(), n
        assert rel_err(got[o:o + k], want[o:o + k]) <= 1e-4, (n, got[o:o + 2], want[o:o + 2])
