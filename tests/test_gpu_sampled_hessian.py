"""-m gpu: vaek_sampled_elbo_hvp_replicas and vaek_sampled_elbo_hessian_lanczos_replicas -- Hessian-vector products, the gradient and a
Lanczos spectrum of the SAMPLE-AVERAGE ELBO f_K of N linear VAEs with one or two decoders (csrc/sampled_hessian.hip) -- the event class
and `run.py --sampled_elbo_hessian`.

References (cases and bounds: tests/sampled_hessian_cases.py):
  - the float64 restatement tools/sampled_hessian_reference.py on the identical rows, samples and parameters (itself held to torch
    autograd by tests/test_sampled_hessian_host.py): every element of H v and of the gradient, and f_K, within 64 (rows K + 2 D + 2 L)
    2^-53 times its magnitude image;
  - vaek_elbo_hvp_replicas, a merged kernel: with sigma-point samples f_K is the exact f identically in theta;
  - the eigenvalues of the restatement's dense Hessian (of torch's at D28_L32s): every Ritz value within its own rho plus ritz_slack;
  - itself, BITWISE: two runs, replica r of n = 3 against n = 1, drawing mode against explicit rows and samples, shared against
    per-replica strides, a captured replay."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sampled_hessian_cases as K
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
R = 3
X_TAG, Z_TAG = 11, 12
PAD = 3                                      # sentinel doubles behind every per-replica block
LEN, HEAD, MS = 142, 12, 32
STATE = 128                                  # doubles of a replica's state block in front of the partials (csrc/sampled_hessian.hip)
DRAW = {"D4_L2s": dict(kind=1, dd=2, did=1, pad=1, var=0.0), "D13_L5s": dict(kind=1, dd=7, did=1, pad=5, var=0.01)}
X_SEEDS, X_STEPS = [77, 2 ** 63 + 5, 1000003], [1, 4, 2 ** 31 + 7]
Z_SEEDS, Z_STEPS = [91, 2 ** 63 + 17, 424243], [3, 2 ** 31 + 9, 6]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _ref():
    return _tool("sampled_hessian_reference")


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def _full(*shape):
    return torch.full(shape, SENT, dtype=torch.float64, device="cuda")


class _Case:
    """One engine and R replicas of a case with distinct parameters, rows, samples and start vectors; the parameter stack's stride
    exceeds P by 5 sentinel floats, every output block is followed by PAD sentinel doubles and the workspace starts as sentinels."""

    def __init__(self, name, batch=100):
        from vae_training_amd.engine import Engine
        self.c = c = K.BY_NAME[name]
        self.eng = e = Engine(batch, c.D, c.L, (), (), c.eps_cli, c.tdv, c.sig)
        self.P = P = e.P
        assert P == K.param_count(c) and [off for off, _ in e.leaves.values()] == K.first_elements(c), e.leaves
        assert e.sampled_elbo_hessian_record_len == LEN and e.supports_sampled_elbo_hessian(2)
        self.rows_max = max(c.rows)
        self.thetas = [K.make_theta(c, r) for r in range(R)]
        self.params = torch.full((R, P + 5), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :P] = _dev(np.stack(self.thetas), torch.float32)
        self.x64 = [K.make_rows(c, self.rows_max, r) for r in range(R)]
        self.xi64 = [K.make_samples(c, self.rows_max, r) for r in range(R)]
        self.x = _dev(np.stack(self.x64), torch.float32)                                          # [R, rows_max, D]
        self.xi = _dev(np.stack(self.xi64), torch.float32)                                        # [R, rows_max, K, L]
        self.v0 = _dev(np.stack([K.start_vector(c, r) for r in range(R)]))
        self.V64 = K.directions(c)
        self.V = _dev(self.V64)
        self.draw = d = DRAW.get(name)
        if d is not None:
            self.A = _dev(np.random.default_rng(23).standard_normal((R, d["dd"])), torch.float32)
            self.tabs = (_i64(X_SEEDS), _i32(X_STEPS), _i64(Z_SEEDS), _i32(Z_STEPS))

    def workspace(self, n, rows):
        return torch.full((self.eng.sampled_elbo_hessian_workspace(n, rows, self.c.K) // 8,), SENT, dtype=torch.float64, device="cuda")

    def source_kw(self, rows, sl, draw):
        if not draw:
            return dict(x=self.x[sl, :rows].contiguous(), xi=self.xi[sl, :rows].contiguous())
        d = self.draw
        return dict(kind=d["kind"], A=self.A[sl], dd=d["dd"], did=d["did"], pad=d["pad"], var_added=d["var"], a_stride=d["dd"], samples=self.c.K,
                    x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], z_seeds=self.tabs[2][sl], z_steps=self.tabs[3][sl], x_tag=X_TAG, z_tag=Z_TAG)

    def hvp(self, rows, v=None, rs=None, draw=False, grad=True, **kw):
        """(hv [n, nvec * P + PAD], grad [n, P + PAD], out [n, 4 + PAD], workspace) of replicas `rs` (default all)."""
        sl = slice(None) if rs is None else rs
        n = self.params[sl].shape[0]
        v = self.V if v is None else v
        nvec = v.shape[-2]
        hv, g, out, ws = _full(n, nvec * self.P + PAD), _full(n, self.P + PAD), _full(n, 4 + PAD), self.workspace(n, rows)
        a = dict(params=self.params[sl], rows=rows, out=out, workspace=ws, v=v, hv=hv, grad=g if grad else None, nvec=nvec, hv_stride=hv.shape[1])
        a.update(self.source_kw(rows, sl, draw))
        a.update(kw)
        if a["nvec"] == 0:                                                # the gradient call: no directions, no products
            a.update(v=None, hv=None, hv_stride=0)
        self.eng.sampled_elbo_hvp_replicas(**a)
        return hv, g, out, ws

    def lanczos(self, rows, steps, rs=None, draw=False, **kw):
        """(basis [n, steps * P + PAD], out [n, 142 + PAD])."""
        sl = slice(None) if rs is None else rs
        n = self.params[sl].shape[0]
        basis, out = _full(n, steps * self.P + PAD), _full(n, LEN + PAD)
        a = dict(params=self.params[sl], rows=rows, steps=steps, v0=self.v0[sl], basis=basis, out=out, workspace=self.workspace(n, rows),
                 basis_stride=basis.shape[1])
        a.update(self.source_kw(rows, sl, draw))
        a.update(kw)
        self.eng.sampled_elbo_hessian_lanczos_replicas(**a)
        return basis, out

    def drawn(self, r, rows):
        """(x [rows, D], xi [rows, K, L]) float32 device tensors: replica r's rows as vaek_make_batch writes them and its samples by the
        block rule, cut from the row's latent stream as an engine of 32 + 32 latent normals per row draws it."""
        d, c = self.draw, self.c
        x = self.eng.make_batch(d["kind"], self.A[r].clone(), d["dd"], d["did"], d["pad"], d["var"], rows, X_SEEDS[r], step=X_STEPS[r], tag=X_TAG,
                                want_z=False)[0]
        wide = _wide_engine()
        _, z1, z2 = wide.make_batch(2, None, 16, 16, 16, 0.0, rows, Z_SEEDS[r], step=Z_STEPS[r], tag=Z_TAG, want_x=False)
        stream = torch.cat([z1, z2], dim=1)                                                       # the first 64 normals of every row's stream
        nlb = (c.L + 3) // 4
        assert c.K * nlb * 4 <= 64
        xi = torch.stack([stream[:, 4 * nlb * k:4 * nlb * k + c.L] for k in range(c.K)], dim=1)
        return x.contiguous(), xi.contiguous()


@functools.lru_cache(maxsize=None)
def _wide_engine():
    from vae_training_amd.engine import Engine
    return Engine(100, 32, 32, (), (), -1.0, False, False)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


@functools.lru_cache(maxsize=None)
def _models(name, r, rows):
    """(the restatement, its magnitude image) of replica r of a case on its first `rows` rows; computed once."""
    cs = _case(name)
    c = cs.c
    a = (cs.thetas[r], cs.x64[r][:rows], cs.xi64[r][:rows], c.D, c.L, c.eps_cli, c.tdv, c.sig)
    return _ref().Model(*a), _ref().Model(*a, mag=True)


@functools.lru_cache(maxsize=None)
def _spectrum(name, r, rows):
    """(eigenvalues ascending, |H|_2) of the dense reference Hessian: the restatement's for P <= 600, torch autograd's above; once."""
    cs = _case(name)
    c = cs.c
    if cs.P <= 600:
        H = _models(name, r, rows)[0].hessian()
        H = 0.5 * (H + H.T)
    else:
        H = _ref().autograd(cs.thetas[r], cs.x64[r][:rows], cs.xi64[r][:rows], c.D, c.L, c.eps_cli, c.tdv, c.sig, dense=True)[3]
    lam = np.linalg.eigvalsh(H)
    return lam, float(max(abs(lam[0]), abs(lam[-1])))


def _np(t):
    return t.cpu().numpy()


def _pads_untouched(t, length):
    return bool((t[:, length:] == SENT).all())


CASE_ROWS = [(c.name, rows) for c in K.CASES for rows in c.rows]


# ---- 1. the hvp call against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows", CASE_ROWS)
def test_hvp_gradient_and_f_match_the_restatement(name, rows):
    cs = _case(name)
    c, P = cs.c, cs.P
    m, mg = _models(name, 0, rows)
    hv, g, out, _ = cs.hvp(rows, rs=slice(0, 1))
    nvec = cs.V64.shape[0]
    assert _pads_untouched(hv, nvec * P) and _pads_untouched(g, P) and _pads_untouched(out, 4)
    rec = _np(out)[0]
    got_hv, got_g = _np(hv)[0, :nvec * P].reshape(nvec, P), _np(g)[0, :P]
    ratios = (K.worst_ratio(rec[0] - m.f(), K.value_bound(c, rows, mg.f())), K.worst_ratio(got_g - m.grad(), K.value_bound(c, rows, mg.grad())),
              K.worst_ratio(got_hv - m.hvp(cs.V64), K.value_bound(c, rows, mg.hvp(cs.V64))))
    print(f"{name} rows {rows}: |device - restatement| / bound: f {ratios[0]:.3e}  gradient {ratios[1]:.3e}  H v {ratios[2]:.3e}")
    assert max(ratios) <= 1.0
    assert rec[1] == pytest.approx(np.linalg.norm(m.grad()), rel=1e-12) and rec[2] == m.eps and rec[3] == rows
    # nvec = 0: the gradient and the record only, v and hv not read; grad = NULL: the record only
    hv0, g0, out0, _ = cs.hvp(rows, rs=slice(0, 1), nvec=0)
    assert torch.equal(g0, g) and torch.equal(out0, out)
    _, g1, out1, _ = cs.hvp(rows, rs=slice(0, 1), nvec=0, grad=False)
    assert bool((g1 == SENT).all()) and torch.equal(out1, out)


# ---- 2. sigma points: the sampled call reproduces the exact call of csrc/elbo_hessian.hip -----------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in K.SIGMA_CASES])
def test_sigma_points_reproduce_the_exact_call_on_the_device(name):
    cs = _case(name)
    c, P = cs.c, cs.P
    rows = c.rows[0]
    nvec = cs.V64.shape[0]
    hv, g, out, _ = cs.hvp(rows, rs=slice(0, 1))
    ehv, eg, eout = _full(1, nvec, P), _full(1, P), _full(1, 4)
    cs.eng.elbo_hvp_replicas(cs.params[:1], rows, eout, v=cs.V, hv=ehv, grad=eg, x=cs.x[0, :rows].contiguous())
    ex = _tool("elbo_hessian_reference")
    mg = _models(name, 0, rows)[1]
    eg_mag = ex.Model(cs.thetas[0], cs.x64[0][:rows], c.D, c.L, c.eps_cli, c.tdv, mag=True)
    both = lambda s, x: K.value_bound(c, rows, s) + K.exact_value_bound(c, rows, x)
    ratios = (K.worst_ratio(_np(out)[0, 0] - _np(eout)[0, 0], both(mg.f(), eg_mag.f())),
              K.worst_ratio(_np(g)[0, :P] - _np(eg)[0], both(mg.grad(), eg_mag.grad())),
              K.worst_ratio(_np(hv)[0, :nvec * P].reshape(nvec, P) - _np(ehv)[0], both(mg.hvp(cs.V64), eg_mag.hvp(cs.V64))))
    print(f"{name}: |sampled call - exact call| / (sum of the bounds): f {ratios[0]:.3e}  gradient {ratios[1]:.3e}  H v {ratios[2]:.3e}")
    assert max(ratios) <= 1.0


# ---- 3. Lanczos ----------------------------------------------------------------------------------------------------------------------------------
def _check_record(cs, rec, basis, rows, steps):
    """The structure of one record and its basis block; returns (k, theta, rho, omega)."""
    c, P = cs.c, cs.P
    k = int(rec[2])
    al, be = rec[HEAD + 2 * MS:HEAD + 2 * MS + k], rec[HEAD + 3 * MS:HEAD + 3 * MS + k]
    theta, rho = rec[HEAD:HEAD + k], rec[HEAD + MS:HEAD + MS + k]
    assert 1 <= k <= min(steps, P) and rec[7] == rows and rec[140] == c.K and rec[141] == (1.0 if c.sig else 0.0)
    if k < min(steps, P):                                                 # only a breakdown ends a run early
        assert be[k - 1] <= 2.0 ** -40 * max(np.max(np.abs(al)), np.max(be[:k - 1], initial=0.0))
    for blk in range(4):                                                  # slots >= k are 0
        assert not np.any(rec[HEAD + blk * MS + k:HEAD + (blk + 1) * MS])
    assert np.all(np.diff(theta) >= 0) and np.all(rho >= 0) and rec[9] == theta[-1] and rec[10] == theta[0] and rec[3] == be[k - 1]
    assert rec[11] <= K.OMEGA_MAX
    B = basis[:steps * P].reshape(steps, P)
    assert np.all(B[k:] == SENT) and np.all(basis[steps * P:] == SENT)    # rows >= k and the pad are untouched
    G = B[:k] @ B[:k].T
    assert np.max(np.abs(G - np.eye(k))) <= 2 * K.OMEGA_MAX and rec[11] == pytest.approx(np.max(np.abs(G - np.diag(np.diag(G)))), abs=1e-15)
    T = np.diag(al) + np.diag(be[:k - 1], 1) + np.diag(be[:k - 1], -1)
    assert np.max(np.abs(np.linalg.eigvalsh(T) - theta)) <= max(rec[5], 2.0 ** -43 * rec[6]) + 64 * k * K.U * rec[6]
    assert rec[5] <= 2.0 ** -40 * rec[6]
    return k, theta, rho, rec[11]


@pytest.mark.parametrize("name,rows,steps", [(c.name, rows, steps) for c in K.CASES for rows in c.rows for steps in c.steps])
def test_lanczos_ritz_values_lie_within_their_bounds_of_eigenvalues(name, rows, steps):
    cs = _case(name)
    c, P = cs.c, cs.P
    basis, out = cs.lanczos(rows, steps, rs=slice(0, 1))
    assert _pads_untouched(out, LEN)
    rec, bas = _np(out)[0], _np(basis)[0]
    k, theta, rho, omega = _check_record(cs, rec, bas, rows, steps)
    _, _, hout, _ = cs.hvp(rows, rs=slice(0, 1), nvec=0)
    assert rec[0] == float(hout[0, 0]) and rec[1] == float(hout[0, 1]) and rec[8] == float(hout[0, 2])      # one gradient text
    if P <= 600 or name == "D28_L32s":
        lam, norm_h = _spectrum(name, 0, rows)
        slack = K.ritz_slack(P, k, omega, norm_h)
        which = range(k) if P <= 600 else (0, k - 1)                      # above: theta_min and theta_max
        gap = np.array([np.min(np.abs(lam - theta[i])) - rho[i] for i in which])
        print(f"{name} rows {rows} steps {steps}: k {k}  omega {omega:.2e}  theta_max {theta[-1]:.9e} (lambda_max {lam[-1]:.9e}, rho {rho[-1]:.1e})  "
              f"theta_min {theta[0]:.6e} (lambda_min {lam[0]:.6e})  worst (gap - rho) / slack {np.max(gap) / slack:.3e}")
        assert np.all(gap <= slack)
        assert lam[0] - slack <= theta[0] and theta[-1] <= lam[-1] + slack      # Ritz values lie inside the spectrum
    else:
        # no dense reference: alpha_1 and alpha_k are Rayleigh quotients of the stored basis rows under the restatement's H
        m, mg = _models(name, 0, rows)
        B = bas[:steps * P].reshape(steps, P)
        for j in (0, k - 1):
            hv = m.hvp(B[j])
            bound = float(np.abs(B[j]) @ K.value_bound(c, rows, mg.hvp(B[j]))) + 8 * (omega + P * K.U) * float(np.linalg.norm(hv))
            assert abs(float(B[j] @ hv) - rec[HEAD + 2 * MS + j]) <= bound, (j, float(B[j] @ hv), rec[HEAD + 2 * MS + j], bound)


def test_lanczos_start_vectors_that_end_the_run_at_once():
    """v0 = 0 and a v0 that is not finite give k = 0 and touch no basis row; an eigen-direction breaks down at step 1."""
    cs = _case("D4_L2s")
    P, rows = cs.P, 7
    v0 = cs.v0.clone()
    v0[0].zero_()
    v0[1, 3] = float("nan")
    basis, out = cs.lanczos(rows, 5, v0=v0)
    rec, bas = _np(out), _np(basis)
    for r in (0, 1):
        assert rec[r, 2] == 0 and not np.any(rec[r, 3:7]) and not np.any(rec[r, 9:140]) and np.all(bas[r] == SENT) and rec[r, 140] == 3
        assert np.isfinite(rec[r, 0]) and rec[r, 1] > 0 and rec[r, 7] == rows
    assert rec[2, 2] == 5 and _pads_untouched(out, LEN)


# ---- 4. draws, replicas, runs, strides, padding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DRAW))
def test_drawing_mode_is_explicit_mode_on_the_drawn_bits(name):
    cs = _case(name)
    c, P = cs.c, cs.P
    rows, steps = min(c.rows[0], 37), 4
    d_hv, d_g, d_out, _ = cs.hvp(rows, draw=True)
    d_bas, d_rec = cs.lanczos(rows, steps, draw=True)
    for r in range(R):
        x, xi = cs.drawn(r, rows)
        assert x.shape == (rows, c.D) and xi.shape == (rows, c.K, c.L)
        sl = slice(r, r + 1)
        hv, g, out, _ = cs.hvp(rows, rs=sl, x=x, xi=xi)
        assert torch.equal(hv, d_hv[sl]) and torch.equal(g, d_g[sl]) and torch.equal(out, d_out[sl]), r
        bas, rec = cs.lanczos(rows, steps, rs=sl, x=x, xi=xi)
        assert torch.equal(bas, d_bas[sl]) and torch.equal(rec, d_rec[sl]), r
        # rows drawn, samples explicit, and the other way round
        dk = cs.source_kw(rows, sl, True)
        mixed = {k_: v for k_, v in dk.items() if k_ not in ("z_seeds", "z_steps")}
        hv2, _, out2, _ = cs.hvp(rows, rs=sl, **{"x": None, "xi": xi, **mixed})
        assert torch.equal(hv2, hv) and torch.equal(out2, out)
        hv3, _, out3, _ = cs.hvp(rows, rs=sl, x=x, xi=None, samples=c.K, z_seeds=dk["z_seeds"], z_steps=dk["z_steps"], z_tag=Z_TAG)
        assert torch.equal(hv3, hv) and torch.equal(out3, out)
    assert not torch.equal(d_out[0], d_out[1])


def test_sample_zero_is_make_batch_z1_and_the_batch_size_does_not_matter():
    from vae_training_amd.engine import Engine
    cs = _case("D13_L5s")
    c, d, rows = cs.c, cs.draw, 37
    other = Engine(257, c.D, c.L, (), (), c.eps_cli, c.tdv, c.sig)
    for r in range(R):
        sl = slice(r, r + 1)
        x, _ = cs.drawn(r, rows)
        _, z1, _ = cs.eng.make_batch(d["kind"], cs.A[r].clone(), d["dd"], d["did"], d["pad"], d["var"], rows, Z_SEEDS[r], step=Z_STEPS[r], tag=Z_TAG,
                                     want_x=False)
        dk = cs.source_kw(rows, sl, True)
        dk["samples"] = 1
        ws = lambda: torch.zeros(cs.eng.sampled_elbo_hessian_workspace(1, rows, 1), dtype=torch.uint8, device="cuda")
        outs = []
        for eng, src in ((cs.eng, dk), (other, dk), (cs.eng, dict(x=x, xi=z1.reshape(rows, 1, c.L).contiguous()))):
            hv, g, out = _full(1, 2, cs.P), _full(1, cs.P), _full(1, 4)
            eng.sampled_elbo_hvp_replicas(cs.params[sl], rows, out, ws(), v=cs.V[:2].contiguous(), hv=hv, grad=g, **src)
            outs.append((hv, g, out))
        assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0])), r


def test_replicas_runs_and_strides_are_bitwise():
    cs = _case("D13_L5s")
    c, P = cs.c, cs.P
    rows, steps = 300, 6
    all3 = cs.hvp(rows) + cs.lanczos(rows, steps)
    again = cs.hvp(rows) + cs.lanczos(rows, steps)
    for a, b in zip(all3[:3] + all3[4:], again[:3] + again[4:]):          # two runs (the workspace aside: its pads are checked below)
        assert torch.equal(a, b)
    for r in range(R):                                                    # replica r of n = 3 is the n = 1 call on its slices
        sl = slice(r, r + 1)
        one = cs.hvp(rows, rs=sl) + cs.lanczos(rows, steps, rs=sl)
        for a, b in zip(all3[:3] + all3[4:], one[:3] + one[4:]):
            assert torch.equal(a[sl], b), r
    nvec = cs.V64.shape[0]
    for t, length in zip(all3[:3] + all3[4:], (nvec * P, P, 4, steps * P, LEN)):
        assert _pads_untouched(t, length)
    # the workspace: between two partials (P + 1 doubles: the elements and f_K) an even P leaves one double, which nobody stores
    ws = _np(all3[3])
    tiles, pstride = (rows * c.K + 255) // 256, (P + 2) & ~1
    assert ws.size == R * STATE + R * tiles * pstride and pstride == P + 2
    parts = ws[R * STATE:].reshape(R * tiles, pstride)
    assert np.all(parts[:, P + 1] == SENT) and not np.any(parts[:, :P + 1] == SENT)
    # shared rows, samples, directions and start vector (stride 0) against per-replica copies of them
    x0, xi0 = cs.x[0, :rows].contiguous(), cs.xi[0, :rows].contiguous()
    sh = cs.hvp(rows, x=x0, xi=xi0, v=cs.V) + cs.lanczos(rows, steps, x=x0, xi=xi0, v0=cs.v0[0].contiguous())
    pr = (cs.hvp(rows, x=x0.expand(R, -1, -1).contiguous(), xi=xi0.expand(R, -1, -1, -1).contiguous(), v=cs.V.expand(R, -1, -1).contiguous())
          + cs.lanczos(rows, steps, x=x0.expand(R, -1, -1).contiguous(), xi=xi0.expand(R, -1, -1, -1).contiguous(),
                       v0=cs.v0[0].expand(R, -1).contiguous()))
    for a, b in zip(sh[:3] + sh[4:], pr[:3] + pr[4:]):
        assert torch.equal(a, b)
    assert torch.equal(sh[0][0], all3[0][0]) and not torch.equal(sh[0][1], all3[0][1])


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------------------------
def test_the_lanczos_call_is_capturable():
    """A captured call replayed twice = the eager call."""
    cs = _case("D13_L5s")
    rows, steps = 300, 8
    eb, eo = cs.lanczos(rows, steps, draw=True)                           # eager (also the warm-up)
    torch.cuda.synchronize()
    basis, out, ws = _full(*eb.shape), _full(*eo.shape), cs.workspace(R, rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a = dict(params=cs.params, rows=rows, steps=steps, v0=cs.v0, basis=basis, out=out, workspace=ws, basis_stride=basis.shape[1])
    a.update(cs.source_kw(rows, slice(None), True))
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            cs.eng.sampled_elbo_hessian_lanczos_replicas(**a)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                      # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eo) and torch.equal(basis, eb)
        out[:, :LEN] = 0.0


# ---- 6. the event class ------------------------------------------------------------------------------------------------------------------------
def _cli_model(tmp_path, seed, dataset):
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([f"m{seed}", "--dataset", dataset, "--padding_dim", "3", "-dd", "3", "-ds", str(seed)])
    ds = get_dataset(dataset, seed, 3, 100, args)
    d = tmp_path / f"{dataset}{seed}"
    d.mkdir()
    return VAEModel(dirname=str(d), num_batches=10, num_epochs=1, batch_size=100, learning_rate=1e-3, layer_sizes="",
                    encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=6, tunable_decoder_var=True, dataset_name=dataset)


def test_the_event_on_real_models(tmp_path):
    """trainer.ReplicaSampledElboHessian on two sigmoid (two-decoder) models: its stats are the record slots of a direct call under
    (dataset.key[0] ^ dataset.key[1], the counter, tags 11 / 12 / 13), bitwise, and the run's RNG state is left alone.  On two
    one-decoder models after a ReplicaElboHessian: the same rows, and the gap between the two sharpnesses is the stated difference."""
    from vae_training_amd.trainer import ReplicaElboHessian, ReplicaSampledElboHessian
    ms = [_cli_model(tmp_path, s, "sigmoid") for s in (69, 24)]
    state = [(m.key, getattr(m.dataset, "_draws", 0), getattr(m, "_latent_draws", 0)) for m in ms]
    with pytest.raises(RuntimeError, match="ONE decoder"):
        ReplicaElboHessian(ms, 4, rows=64)
    ev = ReplicaSampledElboHessian(ms, steps=6, samples=4, rows=64)
    stats = ev.event()
    for r, m in enumerate(ms):
        kind, A, dd, did, pad, var = m.dataset.device_spec()
        seed = m.dataset.key[0] ^ m.dataset.key[1]
        P = ev.P
        v0 = ev.eng.rng_fill(P, seed, step=1, tag=13).double().reshape(1, P)
        basis, out = _full(1, 6, P), _full(1, LEN)
        ws = torch.zeros(ev.eng.sampled_elbo_hessian_workspace(1, 64, 4), dtype=torch.uint8, device="cuda")
        ev.eng.sampled_elbo_hessian_lanczos_replicas(m.model.flat.reshape(1, -1), 64, 6, v0, basis, out, ws, samples=4, kind=kind,
                                                     A=None if A is None else A.reshape(1, -1).float().cuda().contiguous(), dd=dd, did=did, pad=pad,
                                                     var_added=var, x_seeds=_i64([seed % 2 ** 64]), x_steps=_i32([1]), z_seeds=_i64([seed % 2 ** 64]),
                                                     z_steps=_i32([1]), x_tag=11, z_tag=12)
        rec = _np(out)[0]
        k = int(rec[2])
        assert list(stats[r]) == list(ev.KEYS) and k == 6 and rec[141] == 1.0
        assert np.array_equal(stats[r][ev.KEYS[0]], rec[12:12 + k]) and np.array_equal(stats[r][ev.KEYS[1]], rec[44:44 + k])
        assert [stats[r][k_] for k_ in ev.KEYS[2:]] == [rec[9], rec[10], rec[1]] and m._sampled_hessian_draws == 1
    assert [(m.key, getattr(m.dataset, "_draws", 0), getattr(m, "_latent_draws", 0)) for m in ms] == state
    # one decoder: coupled with the exact Hessian
    ls = [_cli_model(tmp_path, s, "linear_gaussian") for s in (69, 24)]
    ex, sa = ReplicaElboHessian(ls, 8, rows=64), ReplicaSampledElboHessian(ls, steps=8, samples=64, rows=64)
    exact = ex.event_after()
    both = sa.event_after({"elbo_hessian": exact})
    again = sa.event(step=[m._elbo_hessian_draws for m in ls], x_tag=ReplicaElboHessian.X_TAG)
    for r in range(2):
        gap = both[r]["Sharpness Sampling Gap"]
        assert gap == both[r]["Sampled Sharpness"] - exact[r]["Sharpness"] and list(both[r])[:-1] == list(sa.KEYS)
        print(f"model {r}: sharpness {exact[r]['Sharpness']:.6e}, sampled (K = 64) {both[r]['Sampled Sharpness']:.6e}, gap {gap:.3e}")
        assert both[r]["Sampled Sharpness"] > 0 and exact[r]["Sharpness"] > 0 and again[r]["Sampled ELBO Gradient Norm"] > 0


# ---- 7. refusals on a live context ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context():
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    cs = _case("D13_L5s")
    c, P = cs.c, cs.P
    rows, steps = 37, 4
    outs = dict(hv=_full(R, 2 * P), grad=_full(R, P), hout=_full(R, 4), basis=_full(R, steps * P), lout=_full(R, LEN))
    ws = cs.workspace(R, rows)
    v = cs.V[:2].contiguous()

    def hvp_args(**kw):
        a = dict(params=cs.params, rows=rows, out=outs["hout"], workspace=ws, v=v, hv=outs["hv"], grad=outs["grad"], nvec=2)
        a.update(cs.source_kw(rows, slice(None), True))
        a.update(kw)
        if torch.is_tensor(a["hv"]):
            a.setdefault("hv_stride", a["hv"].shape[1])
        return a

    def lan_args(**kw):
        a = dict(params=cs.params, rows=rows, steps=steps, v0=cs.v0, basis=outs["basis"], out=outs["lout"], workspace=ws)
        a.update(cs.source_kw(rows, slice(None), True))
        a.update(kw)
        if torch.is_tensor(a["basis"]):
            a.setdefault("basis_stride", a["basis"].shape[1])
        return a

    def refused(why, match, which="both", **kw):
        before = cs.params.clone()
        for name, fn, args in (("vaek_sampled_elbo_hvp_replicas", "sampled_elbo_hvp_replicas", hvp_args),
                               ("vaek_sampled_elbo_hessian_lanczos_replicas", "sampled_elbo_hessian_lanczos_replicas", lan_args)):
            if which not in ("both", fn):
                continue
            a = args(**kw)
            eng = a.pop("eng", cs.eng)
            with pytest.raises(VaekError) as ei:
                getattr(eng, fn)(**a)
            assert ei.value.code == -1 and name + ": " in str(ei.value) and match in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs.values()) and bool((ws == SENT).all()) and torch.equal(cs.params, before), why

    mlp = Engine(100, 13, 5, (200, 200, 200), (200, 200, 200), -3.0, True, False)
    assert not mlp.supports_sampled_elbo_hessian(1)
    refused("an MLP context", "vaek_supports_sampled_elbo_hessian", eng=mlp)
    assert not Engine(100, 13, 5, (), (), -3.0, True, True, dtype="bf16").supports_sampled_elbo_hessian(1)
    assert not Engine(100, 29, 5, (), (), -3.0, True, True).supports_sampled_elbo_hessian(1)      # D > 28 with two decoders
    assert not Engine(100, 33, 5, (), (), -3.0, True, False).supports_sampled_elbo_hessian(2)
    for kind in (-1, 0, 1, 2, 3):                                          # = the log-likelihood's predicate
        assert cs.eng.supports_sampled_elbo_hessian(kind) == cs.eng.supports_log_likelihood(kind) == (0 <= kind <= 2)
    assert cs.eng.sampled_elbo_hessian_max_columns == 1 << 22
    # the caps
    refused("samples = 0", "0 samples, need 1 .. 1024 (vaek_log_likelihood_max_samples)", samples=0)
    refused("samples = 1025", "1025 samples", samples=1025)
    refused("rows x samples above 2^16", "4096 rows x 17 samples = 69632 columns per replica, at most 65536", rows=4096, samples=17)
    refused("rows = 4097", "4097 rows, need 1 .. 4096 (vaek_log_likelihood_max_rows)", rows=4097)
    many = torch.zeros(80, P, dtype=torch.float32, device="cuda")
    seeds80, steps80 = _i64([5] * 80), _i32([1] * 80)
    refused("n x rows x samples above 2^22", "80 replicas x 4096 rows x 16 samples = 5242880 columns, at most 4194304 "
            "(vaek_sampled_elbo_hessian_max_columns)", params=many, rows=4096, samples=16, x_seeds=seeds80, x_steps=steps80, z_seeds=seeds80,
            z_steps=steps80, A=cs.A[0].clone(), a_stride=0)
    with pytest.raises(VaekError, match="vaek_sampled_elbo_hessian_workspace_bytes"):
        cs.eng.sampled_elbo_hessian_workspace(1, 4096, 17)
    with pytest.raises(VaekError, match="vaek_sampled_elbo_hessian_workspace_bytes"):
        mlp.sampled_elbo_hessian_workspace(1, 10, 2)
    # the samples' source
    refused("z_seeds NULL", "z_seeds is NULL", z_seeds=None)
    refused("z_steps NULL", "z_steps is NULL", z_steps=None)
    refused("z_tag = 2^30", "tag >= 2^30", z_tag=2 ** 30)
    xi = cs.xi[:, :rows].contiguous()
    refused("0 < xi_stride < rows * K * L", f"xi_stride {rows * c.K * c.L - 1}", xi=xi, xi_stride=rows * c.K * c.L - 1)
    refused("xi_stride < 0", "xi_stride -1", xi=xi, xi_stride=-1)
    # buffers: a short workspace cannot be detected, a NULL or misaligned one is refused
    refused("workspace NULL", "workspace is NULL or not 16-byte aligned (vaek_sampled_elbo_hessian_workspace_bytes)", workspace=None)
    refused("workspace misaligned", "not 16-byte aligned", workspace=ws.data_ptr() + 8)
    h, l = "sampled_elbo_hvp_replicas", "sampled_elbo_hessian_lanczos_replicas"
    refused("out misaligned", "out is not 8-byte aligned", h, out=outs["hout"].data_ptr() + 4, out_stride=4)
    refused("hv misaligned", "hv is not 8-byte aligned", h, hv=outs["hv"].data_ptr() + 4, hv_stride=2 * P)
    refused("grad misaligned", "grad is not 8-byte aligned", h, grad=outs["grad"].data_ptr() + 4, grad_stride=P)
    refused("basis misaligned", "basis is not 8-byte aligned", l, basis=outs["basis"].data_ptr() + 4, basis_stride=steps * P)
    refused("v0 misaligned", "v0 is not 8-byte aligned", l, v0=cs.v0.data_ptr() + 4, v0_stride=0)
    refused("v and hv overlap", "v and hv overlap", h, v=outs["hv"].data_ptr() + 8 * P, v_stride=0)
    refused("hv inside the shared v", "v and hv overlap", h, v=outs["hv"].data_ptr(), v_stride=2 * P)
    refused("nvec = 65", "65 vectors, need 0 .. 64 (vaek_elbo_hvp_max_vectors)", h, nvec=65)
    refused("steps = 33", "33 steps, need 1 .. 32 (vaek_elbo_hessian_max_steps)", l, steps=33)
    refused("out_stride < 142", "out_stride 141 < 1 x record length 142 (vaek_sampled_elbo_hessian_record_len)", l, out_stride=LEN - 1)
    refused("struct_size", "struct_size 12", struct_size=12)
    # the legal neighbours run
    cs.eng.sampled_elbo_hvp_replicas(**hvp_args())
    cs.eng.sampled_elbo_hessian_lanczos_replicas(**lan_args())
    torch.cuda.synchronize()
    assert not bool((outs["hout"] == SENT).any()) and not bool((outs["lout"] == SENT).any())


# ---- 8. one run.py line: the script shape ----------------------------------------------------------------------------------------------------
NEW_KEYS = ("Sampled ELBO Hessian Ritz Values", "Sampled ELBO Hessian Ritz Residuals", "Sampled Sharpness", "Sampled ELBO Hessian Min Ritz",
            "Sampled ELBO Gradient Norm")


def _run_py(tmp_path, name, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "",
           "-ow", "--latent_dim", "24", "--padding_dim", "20", "-dd", "7", "--epsilon", "-3", "-tdv", "--num_batches", "40", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def test_run_py_on_the_two_decoder_script_shape(tmp_path):
    """sigmoid_dd7_pd20_ld_24 for 40 batches with --sampled_elbo_hessian in a fresh child process: the banner, the five keys in
    losses.npz (one entry per n_print event, at batch 0); --elbo_hessian on the same line is still refused, with its old message."""
    r = _run_py(tmp_path, "samp", "--sampled_elbo_hessian")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ("Sampled ELBO Hessian events: 32 Lanczos steps on 1000 rows x 8 samples (vaek_sampled_elbo_hessian_lanczos_replicas)" in r.stdout
            and "Sampled Sharpness |" in r.stdout), r.stdout[-1500:]
    got = dict(np.load(os.path.join(str(tmp_path), "data", "samp", "losses.npz"), allow_pickle=True))
    for k in NEW_KEYS:
        assert len(got[k]) == 1, (k, len(got[k]))
    th, rho = np.asarray(got[NEW_KEYS[0]][0], np.float64), np.asarray(got[NEW_KEYS[1]][0], np.float64)
    assert th.shape == rho.shape == (32,) and np.all(np.diff(th) >= 0) and np.all(rho >= 0) and np.isfinite(th).all()
    assert float(got["Sampled Sharpness"][0]) == th[-1] and float(got["Sampled ELBO Hessian Min Ritz"][0]) == th[0]
    assert float(got["Sampled ELBO Gradient Norm"][0]) > 0.0 and "Sharpness Sampling Gap" not in got
    print({k: np.asarray(got[k][-1]).tolist() for k in NEW_KEYS[2:]})
    r = _run_py(tmp_path, "exact", "--elbo_hessian")
    assert r.returncode != 0 and "--elbo_hessian needs" in r.stderr and "ONE decoder" in r.stderr and "Batch |" not in r.stdout, r.stderr[-1500:]
