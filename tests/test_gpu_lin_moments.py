"""-m gpu: the linear-moment launch (csrc/linear_moments.hip, linear_moments_dev.h) role by role against the float64 references of
tests/lin_moment_ref.py.

  (a) streamers + reducers, launch-per-step form (vaek_train_steps_moments): the moment image of exact-integer batches bit for bit,
      of wide batches within (n_add + 1) 2^-24 Mabs per cell, n_add = T / 8 + 8;
  (b) the same through ONE persistent launch of n = 7 and n = 64 distinct batches (vaek_debug_lin), n_add = T / 4 + 4;
  (c) LinUpd (vaek_train_steps_update) on a host-made image: every gradient element and the three loss slots within k 2^-24 of
      their term-magnitude sums, Adam by elbo_tail_ref.check_adam on the kernel's own gradient bits;
  (d) LinUpdM (vaek_train_steps on exact-integer batches, so that M is exact and the error is the updater's): the same bounds at
      n = 1; with lr = 0 every step of n = 2 .. 130 is a pure function of (p0, batch k) -- the loss ring, the last gradients, the
      moment recursion (bound: a rounding count made term by term, see lr0_case) and the untouched parameters pin the in-launch
      hand-offs step by step.
Every call asserts its profiler labels, every persistent launch that nothing gave up; inputs, the image and the gradients lie between
NaN guard bands (dense16_ref.guarded).  The batch sizes are built from the plan's tile height T (vaek_debug_lin, op 0)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import elbo_oracle as O
from tests import dense16_ref as R
from tests import elbo_tail_ref as TR
from tests import lin_moment_ref as LM
from tests import test_gpu_dense16 as T16
from tests.gpu_util import engine_for

pytestmark = pytest.mark.gpu

SHAPES3 = [(12, 20), (1, 1), (3, 2), (16, 1), (16, 15), (15, 17), (7, 32), (8, 31)]
SHAPES3_STEP = [(17, 13), (7, 33), (3, 41)]          # D > 16; L > 32: launch-per-step form only
SHAPES4 = [(16, 16), (20, 20), (20, 10), (19, 13), (24, 15), (15, 32), (31, 1)]
SHAPES4_STEP = [(10, 40), (1, 61)]
PERSIST = SHAPES3 + SHAPES4
ALL = SHAPES3 + SHAPES3_STEP + SHAPES4 + SHAPES4_STEP
STREAM, PERSISTENT, UPDATE, STEPWISE = {"lin_moments_stream", "lin_moments_reduce"}, {"lin_moments_persistent"}, {"lin_moments_update"}, {"lin_moments_step", "lin_moments_drain"}
INVALID = -1
D64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    T16.dump_ratios()


def note(fam, ratio):
    T16.RATIOS[fam] = max(T16.RATIOS.get(fam, 0.0), ratio)
    return ratio


def cfg_of(D, L, tdv=True, eps=-1.0):
    return O.Config(D, L, (), (), eps, tdv, "linear_gaussian")


def engine(D, L, B, tdv=True, eps=-1.0, **kw):
    eng = engine_for(cfg_of(D, L, tdv, eps), B, **kw)
    eng.dbg = LM.bind(eng.lib)
    return eng


def plan(eng):
    a = LM.LinDebugArgs()
    assert eng.dbg(eng.h, 0, C.byref(a), None, None) == 0, eng.lib.vaek_last_error()
    return dict(zip(LM.PLAN_FIELDS, (int(v) for v in a.plan)))


@functools.lru_cache(maxsize=None)
def tile_rows(D, L):
    """The plan's T at small batches (three blocks: 256 until the batch outgrows 256 rows per streamer; four: a function of D, L)."""
    return plan(engine(D, L, 1000))["T"]


def batch_sizes(D, L):
    T = tile_rows(D, L)
    out = [-(-8 // min(D, L)), T - 1, T, T + 1, T + 3, T + 4, 2 * T + 5, 16 * T + 1, 33 * T - 5]
    if min(D, L) == 1:
        out.append(T + 2)              # with T + 1, T + 3, T + 4: a last tile of 4, 8, 12 and 16 bytes
    return sorted(set(b for b in out if b * min(D, L) >= 8))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def labelled(eng, call, expect):
    eng.profile_begin(512)
    rc = call()
    torch.cuda.synchronize()
    rep = set(eng.profile_report())
    assert rep == set(expect), (sorted(rep), sorted(expect))
    return rc


def guarded_in(t, lead):
    """A copy of `t` between NaN guard bands, `lead` floats (a multiple of 4: the entries ask for 16-byte alignment) off the buffer's."""
    buf, v = R.guarded(t.numel(), "cuda", lead)
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4 * (lead % 4)
    return buf, v.view(t.shape)


def guarded_f64(n):
    buf, v = R.guarded(2 * n, "cuda")
    return buf, v, v.view(D64)


def check_inputs(bufs, srcs, what):
    for (buf, v), t in zip(bufs, srcs):
        R.check_guard(buf, v.reshape(-1), prefilled=True, what=what + ": an input")
        assert torch.equal(v, t), what + ": an input was written"


def flat_params(cfg, seed, lv_lo=-3.0, lv_hi=1.0, eps_p=0.75):
    """float32 [P] in the flat leaf order: weights of scale fan_in^-1/2, biases of scale 0.3, log-variances spread over [lv_lo, lv_hi] in a
    shuffled order, the epsilon leaf."""
    g = torch.Generator().manual_seed(seed)
    D, L = cfg.D, cfg.L
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D64)
    lv = torch.linspace(lv_lo, lv_hi, L, dtype=D64) if L > 1 else torch.tensor([lv_hi], dtype=D64)
    lv = lv[torch.randperm(L, generator=g)]
    parts = [rn(D * L) * D ** -0.5, rn(L) * 0.3, rn(L * D) * L ** -0.5, rn(D) * 0.3, lv]
    if cfg.tdv:
        parts.append(torch.tensor([eps_p], dtype=D64))
    return torch.cat(parts).to(torch.float32).cuda()


def tree(cfg, flat):
    return O.unflatten(cfg, flat.detach().cpu().double().numpy())


# ---- the plans ------------------------------------------------------------------------------------------------------------------
def test_plans_reach_every_instantiation():
    steps, persists = set(), set()
    for D, L in ALL:
        pl = plan(engine(D, L, 1000))
        assert pl["ok"] and pl["NB"] == LM.n_blocks(D, L) and pl["NO"] == LM.image_len(pl["NB"]), (D, L, pl)
        assert pl["persist"] == int((D, L) in PERSIST), (D, L, pl)
        assert pl["ntiles"] == -(-1000 // pl["T"]) and pl["T"] % 32 == 0 and 32 <= pl["T"] <= 512
        assert pl["which_step"] == (2 if (D, L) == (12, 20) else pl["NB"] - 3)
        steps.add(pl["which_step"])
        if pl["persist"]:
            persists.add(pl["which_persist"])
            assert pl["n_stream"] >= 1 and pl["n_reduce"] >= 1
    for B, which, T in ((59136, 1, 256), (65536, 0, 288), (65664, 0, 288)):
        pl = plan(engine(12, 20, B))
        assert (pl["which_persist"], pl["T"]) == (which, T), (B, pl)
        persists.add(pl["which_persist"])
    assert plan(engine(20, 20, 1000))["which_persist"] == 3 and plan(engine(20, 10, 1000))["which_persist"] == 2
    assert steps == {0, 1, 2} and persists == {0, 1, 2, 3}


# ---- (a) streamers and reducers, launch-per-step form -----------------------------------------------------------------------------
def moments_call(eng, x, z1, z2, M):
    return eng.lib.vaek_train_steps_moments(eng.h, C.c_void_p(x.data_ptr()), C.c_void_p(z1.data_ptr()), C.c_void_p(z2.data_ptr()),
                                            C.c_void_p(M.data_ptr()), C.c_void_p(eng.workspace.data_ptr()), stream())


def stream_case(D, L, B, leads=(0, 4)):
    eng = engine(D, L, B)
    pl = plan(eng)
    NB, NO, T = pl["NB"], pl["NO"], pl["T"]
    # n_add: all 8 waves of a streamer share a tile's T rows (lin_tile_products' CW = LNW = 8), then the 8 images are combined
    nadd = LM.n_add(T, 8)
    worst = 0.0
    for make, na in ((LM.exact_batch, None), (LM.wide_batch, nadd)):
        for lead in leads:
            what = f"moments D={D} L={L} B={B} T={T} {make.__name__} lead={lead}"
            src = make(B, D, L, seed=1000 * B + 7 * D + L, device="cuda")
            bufs = [guarded_in(t, lead) for t in src]
            M, Mabs = LM.moments(*src)
            imgs = []
            for _ in range(2):
                mb, mv, img = guarded_f64(NO)
                rc = labelled(eng, lambda: moments_call(eng, bufs[0][1], bufs[1][1], bufs[2][1], img), STREAM)
                assert rc == 0, eng.lib.vaek_last_error()
                R.check_guard(mb, mv, what=what + " M")
                imgs.append(img)
            assert torch.equal(imgs[0].view(torch.int64), imgs[1].view(torch.int64)), what + ": two runs differ"
            worst = max(worst, LM.check_moments(imgs[0], M, Mabs, D, L, NB, na, what=what))
            check_inputs(bufs, src, what)
    return note("lin stream", worst)


@pytest.mark.parametrize("D,L", ALL)
def test_stream_and_reduce(D, L):
    for B in batch_sizes(D, L):
        stream_case(D, L, B)


@pytest.mark.parametrize("B", [65536, 65664])
def test_stream_and_reduce_at_the_metric_size(B):
    """288-row tiles (lin_plan's choice for the persistent form; the launch-per-step form takes the plan's tile too): 228 of them, the
    last ragged at 65 536 and whole at 65 664 = 228 * 288."""
    assert plan(engine(12, 20, B))["T"] == 288
    stream_case(12, 20, B, leads=(0,))


def test_misaligned_batch_pointers_are_refused():
    eng = engine(12, 20, 300)
    src = LM.exact_batch(300, 12, 20, seed=1, device="cuda")
    good = [guarded_in(t, 0)[1] for t in src]
    _, _, img = guarded_f64(plan(eng)["NO"])
    for k in range(3):
        bad = list(good)
        bad[k] = guarded_in(src[k], 1)[1]
        assert bad[k].data_ptr() % 16 == 4
        assert moments_call(eng, bad[0], bad[1], bad[2], img) == INVALID
        keep = [(C.c_void_p * 1)(C.c_void_p(t.data_ptr())) for t in bad]
        a = LM.LinDebugArgs()
        step = torch.zeros(1, dtype=torch.int32, device="cuda")
        a.n = 1
        a.xs, a.z1s, a.z2s = (C.cast(p, C.c_void_p) for p in keep)
        a.step_dev, a.M_out = step.data_ptr(), img.data_ptr()
        assert eng.dbg(eng.h, 1, C.byref(a), C.c_void_p(eng.workspace.data_ptr()), stream()) == INVALID
        st = [eng.new_flat(), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(), step]
        with pytest.raises(Exception):
            eng.train_steps(*st, [tuple(bad)], 0.0)
    torch.cuda.synchronize()
    eng2 = engine(7, 33, 300)                     # no persistent form: the debug launch is refused
    a = LM.LinDebugArgs()
    a.n = 1
    assert eng2.dbg(eng2.h, 1, C.byref(a), C.c_void_p(eng2.workspace.data_ptr()), stream()) == INVALID


# ---- (b) streamers and reducers of the persistent form ----------------------------------------------------------------------------
class Pool:
    """n distinct batches of B rows as windows of ONE guarded pool of B + 4 (n - 1) rows: batch i = rows [4 i, 4 i + B) (16-byte aligned
    whatever the column count).  Batch 0 starts at the front guard band, batch n - 1 ends at the back one."""

    def __init__(self, make, B, D, L, n, seed):
        self.B, self.n = B, n
        self.src = make(B + 4 * (n - 1), D, L, seed=seed, device="cuda")
        self.bufs = [guarded_in(t, 0) for t in self.src]
        self.u = LM.features(*self.src)

    def batch(self, i):
        return tuple(v[4 * i:4 * i + self.B] for _, v in self.bufs)

    def rows(self, i):
        return self.u[4 * i:4 * i + self.B]

    def moments(self, i):
        u = self.rows(i)
        return u.t() @ u, u.abs().t() @ u.abs()

    def pointers(self, k, n=None):
        return (C.c_void_p * (n or self.n))(*[C.c_void_p(self.batch(i)[k].data_ptr()) for i in range(n or self.n)])


def persist_moments(eng, pool, n, NO):
    mb, mv, img = guarded_f64(n * NO)
    step = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    keep = [pool.pointers(k, n) for k in range(3)]
    a = LM.LinDebugArgs()
    a.n = n
    a.xs, a.z1s, a.z2s = (C.cast(p, C.c_void_p) for p in keep)
    a.step_dev, a.M_out = step.data_ptr(), img.data_ptr()
    rc = labelled(eng, lambda: eng.dbg(eng.h, 1, C.byref(a), C.c_void_p(eng.workspace.data_ptr()), stream()), PERSISTENT)
    assert rc == 0, eng.lib.vaek_last_error()
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    assert int(step) == 5
    R.check_guard(mb, mv, what="persistent M")
    return img.view(n, NO)


def persist_case(D, L, B, ns=(7, 64)):
    eng = engine(D, L, B)
    pl = plan(eng)
    assert pl["persist"]
    NB, NO, T = pl["NB"], pl["NO"], pl["T"]
    # n_add: waves 0 .. 3 of a persistent streamer multiply (kLinCW = 4) and share a tile's T rows, then their 4 images are combined
    nadd = LM.n_add(T, 4)
    worst = 0.0
    for make, na in ((LM.exact_batch, None), (LM.wide_batch, nadd)):
        pool = Pool(make, B, D, L, max(ns), seed=77 * B + 3 * D + L)
        ref = [pool.moments(i) for i in range(max(ns))]
        M, Mabs = torch.stack([m for m, _ in ref]), torch.stack([m for _, m in ref])
        for n in ns:
            what = f"persistent moments D={D} L={L} B={B} T={T} n={n} {make.__name__}"
            img = persist_moments(eng, pool, n, NO)
            worst = max(worst, LM.check_moments(img, M[:n], Mabs[:n], D, L, NB, na, what=what))
        check_inputs(pool.bufs, pool.src, f"persistent moments D={D} L={L} B={B}")
    return note("lin persist stream", worst)


@pytest.mark.parametrize("D,L", PERSIST)
def test_persistent_stream_and_reduce(D, L):
    for B in batch_sizes(D, L):
        persist_case(D, L, B)


@pytest.mark.parametrize("B", [65536, 65664])
def test_persistent_stream_and_reduce_at_the_metric_size(B):
    assert plan(engine(12, 20, B))["which_persist"] == 0
    persist_case(12, 20, B)


# ---- (c), (d) the updaters --------------------------------------------------------------------------------------------------------
# (tdv, eps_cli, log-variance range, starting step counter, non-zero starting moments)
REGIMES = [(True, -8.0, (-30.0, 20.0), 0, False), (True, 0.0, (-3.0, 1.0), 1, True), (True, 4.0, (-30.0, 20.0), 999, True),
           (False, -1.0, (-30.0, 20.0), 100000, True)]


def start_state(eng, cfg, seed, lv, moments):
    p0 = flat_params(cfg, seed, *lv)
    g = torch.Generator().manual_seed(seed + 1)
    if moments:
        m0 = (torch.randn(eng.P, generator=g) * 0.1).cuda()
        v0 = (torch.rand(eng.P, generator=g) * 0.01).cuda()
    else:
        m0, v0 = eng.new_flat(), eng.new_flat()
    return p0, m0, v0


def check_update(eng, cfg, got, ref, state0, state1, t, lr, fam, what):
    """The gradient buffer against step_ref's result, Adam on the kernel's own gradient bits."""
    gb, gv = got
    R.check_guard(gb, gv, what=what + " grads")
    r = note(fam, LM.check_step(gv, cfg, ref, what=what))
    (p0, m0, v0), (p1, m1, v1) = state0, state1
    TR.check_adam(p1, m1, v1, p0, m0, v0, gv[:eng.P], t, lr, what=what + " adam")
    return r


def update_case(D, L, B, regime, world=1):
    tdv, eps, lv, step0, moments = regime
    kw = dict(world=2, rank=0, global_batch=2 * B) if world == 2 else {}
    eng = engine(D, L, B, tdv, eps, **kw)
    cfg = cfg_of(D, L, tdv, eps)
    pl = plan(eng)
    rows = 2 * B if world == 2 else B              # data parallel: the image of the FULL batch, rows = Bt != B
    what = f"LinUpd D={D} L={L} B={B} regime={regime} world={world}"
    src = LM.wide_batch(rows, D, L, seed=5 * D + L + step0, device="cuda")
    M, _ = LM.moments(*src)
    img = LM.pack(M, pl["NB"])                     # host-made: no streamer involved
    p0, m0, v0 = start_state(eng, cfg, 31 * D + L, lv, moments)
    ref = LM.step_ref(cfg, tree(cfg, p0), M, rows, rows)
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    gb, gv = R.guarded(eng.grad_len, "cuda")
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    ring = torch.zeros(8, dtype=torch.float32, device="cuda")
    eng.set_loss_history(ring)
    lr = 1e-3
    labelled(eng, lambda: eng.moments_update(p1, gv, m1, v1, step, img, lr), UPDATE)
    eng.set_loss_history(None)
    assert int(step) == step0 + 1, what
    assert torch.equal(ring[step0 % 8:step0 % 8 + 1].view(torch.int32), gv[eng.P:eng.P + 1].view(torch.int32)) and int((ring != 0).sum()) <= 1, what
    return check_update(eng, cfg, (gb, gv), ref, (p0, m0, v0), (p1, m1, v1), step0 + 1, lr, "lin upd", what)


@pytest.mark.parametrize("D,L", ALL)
def test_launch_per_step_updater(D, L):
    B = tile_rows(D, L) + 3
    for regime in REGIMES:
        update_case(D, L, B, regime)
    update_case(D, L, B, (True, -1.0, (-3.0, 1.0), 0, False), world=2)


def run_steps(eng, pool, n, state, lr, labels):
    p, m, v = (t.clone() for t in state)
    gb, gv = R.guarded(eng.grad_len, "cuda")
    ring = torch.zeros(n + 3, dtype=torch.float32, device="cuda")
    eng.set_loss_history(ring)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    batches = [pool.batch(i) for i in range(n)]
    labelled(eng, lambda: eng.train_steps(p, gv, m, v, step, batches, lr), labels)
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    assert int(step) == n
    return p, m, v, (gb, gv), ring


def one_step_case(D, L, B, regime, fam, labels):
    tdv, eps, lv, step0, moments = regime
    eng = engine(D, L, B, tdv, eps)
    cfg = cfg_of(D, L, tdv, eps)
    what = f"{fam} D={D} L={L} B={B} regime={regime}"
    pool = Pool(LM.exact_batch, B, D, L, 1, seed=9 * D + L)
    M, _ = pool.moments(0)
    p0, m0, v0 = start_state(eng, cfg, 17 * D + L, lv, moments)
    ref = LM.step_ref(cfg, tree(cfg, p0), M, B, B)
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    gb, gv = R.guarded(eng.grad_len, "cuda")
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    lr = 1e-3
    labelled(eng, lambda: eng.train_steps(p1, gv, m1, v1, step, [pool.batch(0)], lr), labels)
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    assert int(step) == step0 + 1, what
    return check_update(eng, cfg, (gb, gv), ref, (p0, m0, v0), (p1, m1, v1), step0 + 1, lr, fam, what)


@pytest.mark.parametrize("D,L", PERSIST)
def test_matrix_core_updater_one_step(D, L):
    B = tile_rows(D, L) + 3
    for regime in REGIMES:
        one_step_case(D, L, B, regime, "lin updM", PERSISTENT)


LR0_STEPS = (2, 3, 5, 64, 65, 69, 70, 130)


def lr0_case(D, L, ns, fam, labels, regime=REGIMES[2]):
    """lr = 0: the parameters never move, so step k is a pure function of (p0, batch k).  Returns the largest ratios."""
    tdv, eps, lv, _, _ = regime
    B = tile_rows(D, L) + 3
    eng = engine(D, L, B, tdv, eps)
    cfg = cfg_of(D, L, tdv, eps)
    P = eng.P
    pool = Pool(LM.exact_batch, B, D, L, max(ns), seed=13 * D + L)
    state = start_state(eng, cfg, 23 * D + L, lv, True)
    p0, m0, v0 = state
    pt = tree(cfg, p0)
    refs = [LM.step_ref(cfg, pt, pool.moments(i)[0], B, B) for i in range(max(ns))]
    vec = [LM.step_vectors(r) for r in refs]
    G, Gm = torch.stack([r[:P] for r, _ in vec]), torch.stack([m[:P] for _, m in vec])          # [n, P]
    loss, lossm = torch.stack([r[P] for r, _ in vec]), torch.stack([m[P] for _, m in vec])
    kg = LM.roundings(cfg, "cuda")[:P]
    worst = {"step": 0.0, "m": 0.0, "v": 0.0}
    for n in ns:
        what = f"{fam} lr=0 D={D} L={L} B={B} n={n}"
        p, m, v, (gb, gv), ring = run_steps(eng, pool, n, state, 0.0, labels)
        R.check_guard(gb, gv, what=what + " grads")
        assert torch.equal(p.view(torch.int32), p0.view(torch.int32)), what + ": the parameters moved"
        # the loss ring: entry k is batch k's loss (4 float32 roundings: lin_moment_ref.roundings)
        worst["step"] = max(worst["step"], R.check_f32(ring[:n], loss[:n], 4.0 * lossm[:n], tol=LM.U24, what=what + " loss ring"))
        assert int((ring[n:] != 0).sum()) == 0, what + ": the ring was written past step n"
        # the gradient buffer is the LAST batch's
        worst["step"] = max(worst["step"], LM.check_step(gv, cfg, refs[n - 1], what=what + " last gradients"))
        # m, v: the float64 recursion over the reference gradients (an inexact gradient's magnitude carried in place of its value, as
        # in elbo_tail_ref).  Term k = the gradient of step k, weight (1 - beta) beta^(n - k), reaches m through
        #     the gradient's own kg roundings, (float)(1 - beta1) and its product with g, the add -- kg + 3 --
        #     and the product with (float)beta1 and the add of each of the n - k later steps -- 2 (n - k);
        # v the same with the gradient twice and the square: 2 kg + 4 + 2 (n - k); the starting moment 2 n.  The bound is that
        # count, term by term.  (The shorter form first derived, n 2^-24 of the term sums for both, is wrong at small n: the newest
        # term alone carries 2 kg + 4 >= 8 roundings into v.  Measured at n = 2: v up to 1.21 of it, m up to 0.94 -- on a correct
        # kernel, 0.38 of the count above.  From n >= 2 kg + 4 on it holds and is asserted as well.)
        w1 = (1.0 - TR.B1) * TR.B1 ** torch.arange(n - 1, -1, -1, dtype=D64, device="cuda")
        w2 = (1.0 - TR.B2) * TR.B2 ** torch.arange(n - 1, -1, -1, dtype=D64, device="cuda")
        age = torch.arange(n - 1, -1, -1, dtype=D64, device="cuda")[:, None]
        m_ref = TR.B1 ** n * m0.double() + (w1[:, None] * G[:n]).sum(0)
        m_mag = TR.B1 ** n * m0.double().abs() + (w1[:, None] * Gm[:n]).sum(0)
        v_ref = TR.B2 ** n * v0.double() + (w2[:, None] * G[:n] ** 2).sum(0)
        v_mag = TR.B2 ** n * v0.double() + (w2[:, None] * Gm[:n] ** 2).sum(0)
        m_cnt = 2 * n * TR.B1 ** n * m0.double().abs() + (w1[:, None] * Gm[:n] * (kg[None, :] + 3 + 2 * age)).sum(0)
        v_cnt = 2 * n * TR.B2 ** n * v0.double() + (w2[:, None] * Gm[:n] ** 2 * (2 * kg[None, :] + 4 + 2 * age)).sum(0)
        em, ev = (m.double() - m_ref).abs(), (v.double() - v_ref).abs()
        rm, rv = float((em / (n * LM.U24 * m_mag)).max()), float((ev / (n * LM.U24 * v_mag)).max())
        print(f"{what}: m {rm:.3f} v {rv:.3f} of n 2^-24 term sums", end="; ")
        rmc = R.check_f32(m, m_ref, m_cnt, tol=LM.U24, what=what + " m")
        rvc = R.check_f32(v, v_ref, v_cnt, tol=LM.U24, what=what + " v")
        print(f"m {rmc:.3f} v {rvc:.3f} of the term-by-term count")
        worst.update({"m": max(worst["m"], rmc), "v": max(worst["v"], rvc)})
        if n >= 2 * float(kg.max()) + 4:
            R.check_f32(m, m_ref, n * m_mag, tol=LM.U24, what=what + " m, n 2^-24 form")
            R.check_f32(v, v_ref, n * v_mag, tol=LM.U24, what=what + " v, n 2^-24 form")
    note(fam, worst["step"])
    note(fam + " moments", max(worst["m"], worst["v"]))
    return worst


@pytest.mark.parametrize("D,L", PERSIST)
def test_matrix_core_updater_step_by_step_at_lr_0(D, L):
    lr0_case(D, L, LR0_STEPS, "lin updM", PERSISTENT)


def twin(D, L):
    """The launch-per-step twin of lr0_case (a child process under VAEK_LIN_PERSIST=0: the choice is read once per process)."""
    print(json.dumps(lr0_case(D, L, (2, 3, 5, 70), "lin upd", STEPWISE)))


@pytest.mark.parametrize("D,L", [(12, 20), (20, 20)])
def test_launch_per_step_twin_step_by_step_at_lr_0(D, L):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, {root!r}); from tests.test_gpu_lin_moments import twin; twin({D}, {L})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VAEK_LIN_PERSIST="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    worst = json.loads(r.stdout.strip().splitlines()[-1])
    print(r.stdout)
    assert worst["step"] <= 1.0 and worst["m"] <= 1.0 and worst["v"] <= 1.0, worst
    note("lin upd", worst["step"])
    note("lin upd moments", max(worst["m"], worst["v"]))
