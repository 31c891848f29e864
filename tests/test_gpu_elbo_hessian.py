"""-m gpu: vaek_elbo_hvp_replicas and vaek_elbo_hessian_lanczos_replicas -- Hessian-vector products, the exact gradient and a Lanczos
spectrum of f = -mean exact ELBO of N one-decoder linear VAEs in one launch (csrc/elbo_hessian.hip) -- and `run.py --elbo_hessian`.

References (cases and bounds: tests/elbo_hessian_cases.py):
  - the float64 restatement tools/elbo_hessian_reference.py on the identical rows and parameters (itself held to torch autograd by
    tests/test_elbo_hessian_host.py): every element of H v and of the gradient, and f, within 64 (rows + 2 D + L) 2^-53 times its
    magnitude image; f against minus the exact ELBO of vaek_exact_log_likelihood_replicas on the same rows;
  - the eigenvalues of the restatement's Hessian: every Ritz value within its own rho plus the slack of the cases file; T rebuilt from
    the record's alpha and beta; the basis and the Lanczos relation H V = V T + beta_k v_{k+1} e_k^T;
  - itself, BITWISE: two runs, replica r of n = 3 against n = 1 with strides above the lengths, drawing mode against explicit rows,
    shared rows and directions, engines of other batch sizes, a captured replay."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import elbo_hessian_cases as K
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
R = 3
X_TAG = 3
PAD = 3                                      # sentinel doubles behind every per-replica block
LEN, HEAD, MS = 140, 12, 32
DRAW = {"D12_L20": dict(kind=0, dd=3, did=3, pad=9, var=0.01), "D13_L5": dict(kind=2, dd=10, did=10, pad=3, var=0.0)}


@functools.lru_cache(maxsize=None)
def _ref():
    spec = importlib.util.spec_from_file_location("elbo_hessian_reference", os.path.join(ROOT, "tools", "elbo_hessian_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def _full(*shape):
    return torch.full(shape, SENT, dtype=torch.float64, device="cuda")


class _Case:
    """One engine and R replicas of a case with distinct parameters, rows and start vectors; the parameter stack's stride exceeds P by 5
    sentinel floats and every output block is followed by PAD sentinel doubles."""

    def __init__(self, name, batch=100):
        from vae_training_amd.engine import Engine
        self.c = c = K.BY_NAME[name]
        self.eng = e = Engine(batch, c.D, c.L, (), (), c.eps_cli, c.tdv, False)
        self.P = P = e.P
        assert P == K.param_count(c) and [off for off, _ in e.leaves.values()] == K.first_elements(c), e.leaves
        assert e.elbo_hessian_record_len == LEN and e.elbo_hvp_record_len == 4
        self.thetas = [K.make_theta(c, r) for r in range(R)]
        self.params = torch.full((R, P + 5), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :P] = _dev(np.stack(self.thetas), torch.float32)
        self.x64 = [K.make_rows(c, K.MAX_ROWS, r) for r in range(R)]
        self.x = _dev(np.stack(self.x64), torch.float32)                                          # [R, MAX_ROWS, D]
        self.v0s = np.stack([K.start_vector(c, r) for r in range(R)])
        self.v0 = _dev(self.v0s)
        self.V64 = K.directions(c)
        self.V = _dev(self.V64)
        d = DRAW.get(name)
        self.draw = d
        if d is not None:
            alen = {0: d["dd"] * d["did"], 2: 0}[d["kind"]]
            self.A = _dev(np.random.default_rng(23).standard_normal((R, alen)), torch.float32) if alen else None
            self.a_stride = alen
            self.x_seeds, self.x_steps = [77, 2 ** 63 + 5, 1000003], [1, 4, 2 ** 31 + 7]
            self.tabs = (_i64(self.x_seeds), _i32(self.x_steps))

    def rows_kw(self, rows, sl, draw):
        if not draw:
            return dict(x=self.x[sl, :rows].contiguous())
        d = self.draw
        return dict(kind=d["kind"], A=None if self.A is None else self.A[sl], dd=d["dd"], did=d["did"], pad=d["pad"], var_added=d["var"],
                    x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], a_stride=self.a_stride, x_tag=X_TAG)

    def hvp(self, rows, v=None, rs=None, draw=False, grad=True, **kw):
        """(hv [n, nvec * P + PAD], grad [n, P + PAD], out [n, 4 + PAD]) of replicas `rs` (default all) on the first `rows` rows."""
        sl = slice(None) if rs is None else rs
        n = self.params[sl].shape[0]
        v = self.V if v is None else v
        nvec = v.shape[-2]
        hv, g, out = _full(n, nvec * self.P + PAD), _full(n, self.P + PAD), _full(n, 4 + PAD)
        a = dict(params=self.params[sl], rows=rows, out=out, v=v, hv=hv, grad=g if grad else None, nvec=nvec, hv_stride=hv.shape[1])
        a.update(self.rows_kw(rows, sl, draw))
        a.update(kw)
        a.pop("eng", self.eng).elbo_hvp_replicas(**a)
        return hv, g, out

    def lanczos(self, rows, steps, rs=None, draw=False, v0=None, **kw):
        """(basis [n, steps * P + PAD], out [n, 140 + PAD])."""
        sl = slice(None) if rs is None else rs
        n = self.params[sl].shape[0]
        basis, out = _full(n, steps * self.P + PAD), _full(n, LEN + PAD)
        a = dict(params=self.params[sl], rows=rows, steps=steps, v0=self.v0[sl] if v0 is None else v0, basis=basis, out=out,
                 basis_stride=basis.shape[1])
        a.update(self.rows_kw(rows, sl, draw))
        a.update(kw)
        a.pop("eng", self.eng).elbo_hessian_lanczos_replicas(**a)
        return basis, out

    def drawn_rows(self, r, rows):
        d = self.draw
        Ar = None if self.A is None else self.A[r].clone()
        return self.eng.make_batch(d["kind"], Ar, d["dd"], d["did"], d["pad"], d["var"], rows, self.x_seeds[r], step=self.x_steps[r], tag=X_TAG,
                                   want_z=False)[0]


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


@functools.lru_cache(maxsize=None)
def _models(name, r, rows):
    """(the restatement, its magnitude image) of replica r of a case on its first `rows` rows; computed once."""
    cs = _case(name)
    c = cs.c
    a = (cs.thetas[r], cs.x64[r][:rows], c.D, c.L, c.eps_cli, c.tdv)
    return _ref().Model(*a), _ref().Model(*a, mag=True)


@functools.lru_cache(maxsize=None)
def _spectrum(name, r, rows):
    """(H, its eigenvalues ascending, |H|_2) of the restatement; computed once."""
    H = _models(name, r, rows)[0].hessian()
    H = 0.5 * (H + H.T)
    lam = np.linalg.eigvalsh(H)
    return H, lam, float(max(abs(lam[0]), abs(lam[-1])))


CASE_ROWS = [(c.name, rows) for c in K.CASES for rows in c.rows]


# ---- 1. H v, the gradient and f against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows", CASE_ROWS, ids=[f"{n}_rows{r}" for n, r in CASE_ROWS])
def test_hvp_gradient_and_f_against_the_restatement(name, rows):
    cs = _case(name)
    c, P = cs.c, cs.P
    before = cs.params.clone()
    hv, g, out = cs.hvp(rows)
    ex = torch.zeros(R, cs.eng.exact_log_likelihood_record_len, dtype=torch.float64, device="cuda")
    cs.eng.exact_log_likelihood_replicas(cs.params, rows, ex, x=cs.x[:, :rows].contiguous())
    torch.cuda.synchronize()
    hv, g, out, ex = hv.cpu().numpy(), g.cpu().numpy(), out.cpu().numpy(), ex.cpu().numpy()
    nvec = cs.V64.shape[0]
    assert np.all(hv[:, nvec * P:] == SENT) and np.all(g[:, P:] == SENT) and np.all(out[:, 4:] == SENT), "gap doubles were written"
    assert torch.equal(cs.params, before)
    worst = [0.0, 0.0, 0.0, 0.0]
    for r in range(R):
        m, mg = _models(name, r, rows)
        want, bound = m.hvp(cs.V64), K.value_bound(c, rows, mg.hvp(cs.V64))
        err = np.abs(hv[r, :nvec * P].reshape(nvec, P) - want)
        gerr, gbound = np.abs(g[r, :P] - m.grad()), K.value_bound(c, rows, mg.grad())
        fb = K.value_bound(c, rows, mg.f())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[0] = max(worst[0], np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
            worst[1] = max(worst[1], np.nanmax(np.where(gbound > 0, gerr / gbound, np.where(gerr > 0, np.inf, 0.0))))
        worst[2] = max(worst[2], abs(out[r, 0] - m.f()) / fb)
        worst[3] = max(worst[3], abs(out[r, 0] + ex[r, 1]) / (2.0 * fb))
        assert np.all(err <= bound), (r, float(np.max(err - bound)))
        assert np.all(gerr <= gbound), (r, float(np.max(gerr - gbound)))
        assert abs(out[r, 0] - m.f()) <= fb, (r, out[r, 0], m.f(), fb)
        gn = float(np.sqrt(np.sum(m.grad() ** 2)))
        assert abs(out[r, 1] - gn) <= float(np.sqrt(np.sum(gbound ** 2))) + 64.0 * P * K.U * gn
        assert out[r, 2] == m.eps == c.eps_cli and out[r, 3] == rows
        # f is minus the exact ELBO of the exact log-likelihood call on the same rows: both within the bound of the true value
        assert abs(out[r, 0] + ex[r, 1]) <= 2.0 * fb, (r, out[r, 0], ex[r, 1], fb)
    print(f"{name} rows {rows}: worst |d Hv| {worst[0]:.4f}, |d grad| {worst[1]:.4f}, |d f| {worst[2]:.4f} of the bound; "
          f"|f + exact ELBO| {worst[3]:.4f} of twice the bound")


# ---- 2. symmetry, and H against autograd -----------------------------------------------------------------------------------------------------
def test_symmetry_and_the_autograd_hessian():
    cs = _case("D3_L2")
    c, P, rows = cs.c, cs.P, 7
    eye = _dev(np.eye(P))
    hv, _, _ = cs.hvp(rows, v=eye, grad=False)
    torch.cuda.synchronize()
    hv = hv.cpu().numpy()
    for r in range(R):
        m, mg = _models("D3_L2", r, rows)
        H = hv[r, :P * P].reshape(P, P)
        B = K.value_bound(c, rows, mg.hvp(np.eye(P)))
        assert np.all(np.abs(H - H.T) <= B + B.T), float(np.max(np.abs(H - H.T) - B - B.T))
        _, _, Ha = _ref().autograd(cs.thetas[r], cs.x64[r][:rows], c.D, c.L, c.eps_cli, c.tdv)
        assert np.all(np.abs(H - Ha) <= B + B.T), float(np.max(np.abs(H - Ha) - B - B.T))
        print(f"replica {r}: |H - H^T| {np.max(np.abs(H - H.T)):.2e}, |H - autograd| {np.max(np.abs(H - Ha)):.2e}, |H| {np.max(np.abs(H)):.2e}")


# ---- 3., 4. the Lanczos run: the bound property, T, the basis ---------------------------------------------------------------------------------
def _check_run(name, r, rows, steps, rec, basis, converged=False, full=False):
    """Every property a record and its basis must have, against the restatement's Hessian of (case, replica, rows)."""
    X, c = _ref(), K.BY_NAME[name]
    P = K.param_count(c)
    m, _ = _models(name, r, rows)
    H, lam, norm_h = _spectrum(name, r, rows)
    k = int(rec[2])
    assert rec[2] == k and 1 <= k <= min(steps, P), rec[2]
    th, rho = rec[HEAD:HEAD + k], rec[HEAD + MS:HEAD + MS + k]
    al, be = rec[HEAD + 2 * MS:HEAD + 2 * MS + k], rec[HEAD + 3 * MS:HEAD + 3 * MS + k]
    for q in range(4):
        assert np.all(rec[HEAD + q * MS + k:HEAD + (q + 1) * MS] == 0.0), "slots >= k are 0"
    omega = rec[11]
    assert 0.0 <= omega <= K.OMEGA_MAX, omega
    slack = K.ritz_slack(P, k, omega, norm_h)
    gap = np.array([np.min(np.abs(lam - t)) for t in th])
    assert np.all(gap <= rho + slack), (float(np.max(gap - rho)), slack)
    if full:                                                             # the run spans the whole space: no rho, every Ritz value IS an eigenvalue
        assert k <= P and np.all(gap <= slack), (k, float(np.max(gap)), slack)
    assert np.all(np.diff(th) >= 0.0) and rec[9] == th[-1] and rec[10] == th[0] and rec[3] == be[k - 1] and np.all(rho >= 0.0)
    assert th[-1] <= lam[-1] + slack and th[0] >= lam[0] - slack
    T = X.tridiagonal(al, be)
    norm_t = float(np.sqrt(np.sum(T * T)))
    assert abs(rec[6] - norm_t) <= 64.0 * k * K.U * norm_t
    assert np.max(np.abs(np.linalg.eigvalsh(T) - th)) <= 2.0 ** -40 * norm_t
    assert rec[5] <= 2.0 ** -43 * rec[6] and rec[4] < 32, "the Jacobi solve stopped at its tolerance"
    assert rec[7] == rows and rec[8] == c.eps_cli
    if k < min(steps, P):
        assert be[k - 1] <= 2.0 ** -40 * max(np.max(np.abs(al)), np.max(be[:k - 1], initial=0.0)), "an early end is a breakdown"
    if converged:
        assert rho[-1] <= 1e-8 * abs(th[-1]), (rho[-1], th[-1])
    # the basis: orthonormal within omega (and the rounding of this check's own dots); H V = V T + beta_k v_{k+1} e_k^T
    V = basis[:k * P].reshape(k, P)
    G = V @ V.T
    tol = 64.0 * P * K.U
    assert np.max(np.abs(np.diag(G) - 1.0)) <= tol
    if k > 1:
        off = np.max(np.abs(G[np.triu_indices(k, 1)]))
        assert off <= omega + tol and omega <= off + tol, (off, omega)
    res = m.hvp(V) - T @ V                                               # row j: H v_j - sum_i T_ij v_i
    cols = np.sqrt(np.sum(res * res, axis=1))
    assert np.all(cols[:k - 1] <= slack), (float(np.max(cols[:k - 1], initial=0.0)), slack)
    assert abs(cols[k - 1] - be[k - 1]) <= slack, (cols[k - 1], be[k - 1], slack)
    return k, float(np.max(gap - rho)) / norm_h, omega


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_lanczos_bound_property_and_basis(name):
    cs = _case(name)
    c, P = cs.c, cs.P
    rows, steps = c.rows[0], c.steps[-1]
    n = 2 if P > 1000 else R                                              # the largest Hessian costs seconds per replica on the host
    f_g = cs.hvp(rows, rs=slice(0, n))[2]
    basis, out = cs.lanczos(rows, steps, rs=slice(0, n))
    torch.cuda.synchronize()
    basis, out, f_g = basis.cpu().numpy(), out.cpu().numpy(), f_g.cpu().numpy()
    assert np.all(out[:, LEN:] == SENT) and np.all(basis[:, steps * P:] == SENT)
    for r in range(n):
        k, worst, omega = _check_run(name, r, rows, steps, out[r], basis[r], converged=name in ("D12_L20", "D32_L32"), full=name == "D2_L1")
        assert np.all(basis[r, k * P:steps * P] == SENT), "basis rows >= k are not written"
        assert abs(out[r, 0] - f_g[r, 0]) <= 8.0 * K.U * abs(f_g[r, 0]) and abs(out[r, 1] - f_g[r, 1]) <= 8.0 * K.U * f_g[r, 1], \
            "f and |g| are the hvp call's (the same text in another kernel: to a few roundings)"
        print(f"{name} replica {r}: k {k}, sharpness {out[r, 9]:.6e} (rho {out[r, HEAD + MS + k - 1]:.1e}), min Ritz {out[r, 10]:.6e}, "
              f"omega {omega:.2e}, worst (gap - rho) / |H| {worst:.2e}, sweeps {int(out[r, 4])}, |g| {out[r, 1]:.3e}")
    if name == "D2_L1":
        assert np.all(out[:, 2] <= 8)                                     # P = 8 < steps


# ---- 5. shape edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,steps", [(7, 5), (7, 1), (1, 32), (1, 5)])
def test_shape_edges(rows, steps):
    cs = _case("D3_L2")
    basis, out = cs.lanczos(rows, steps)
    torch.cuda.synchronize()
    basis, out = basis.cpu().numpy(), out.cpu().numpy()
    for r in range(R):
        k, _, _ = _check_run("D3_L2", r, rows, steps, out[r], basis[r])
        assert k <= steps


def test_zero_start_vector_gives_k_zero():
    cs = _case("D3_L2")
    v0 = torch.zeros(R, cs.P, dtype=torch.float64, device="cuda")
    v0[1] = cs.v0[1]                                                      # replica 1 keeps its vector: the others do not affect it
    basis, out = cs.lanczos(7, 5, v0=v0)
    _, want = cs.lanczos(7, 5, rs=slice(1, 2))
    f_g = cs.hvp(7)[2]
    torch.cuda.synchronize()
    assert torch.equal(out[1], want[0])
    out, basis, f_g = out.cpu().numpy(), basis.cpu().numpy(), f_g.cpu().numpy()
    for r in (0, 2):
        assert np.all(out[r, 2:7] == 0.0) and np.all(out[r, 9:LEN] == 0.0), out[r]
        assert abs(out[r, 0] - f_g[r, 0]) <= 8.0 * K.U * abs(f_g[r, 0]) and abs(out[r, 1] - f_g[r, 1]) <= 8.0 * K.U * f_g[r, 1]
        assert out[r, 7] == 7 and out[r, 8] == cs.c.eps_cli
        assert np.all(basis[r] == SENT)


# ---- 6. house properties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D3_L2", "D12_L20"])
def test_two_runs_replicas_and_shared_inputs_are_bitwise(name):
    cs = _case(name)
    c, P = cs.c, cs.P
    rows, steps = c.rows[0], 8
    before = cs.params.clone()
    a, b = cs.hvp(rows), cs.hvp(rows)
    la, lb = cs.lanczos(rows, steps), cs.lanczos(rows, steps)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a + la, b + lb)), "two runs differ"
    for r in range(R):                                                    # n = 3 with strides above the lengths = three n = 1 calls
        one, lone = cs.hvp(rows, rs=slice(r, r + 1)), cs.lanczos(rows, steps, rs=slice(r, r + 1))
        torch.cuda.synchronize()
        assert all(torch.equal(u[r], v[0]) for u, v in zip(a + la, one + lone)), r
    # shared rows (x_stride 0) and shared directions / start vector (v_stride, v0_stride 0) = the same inputs given per replica
    x0 = cs.x[0, :rows].contiguous()
    xs, vs, v0s = x0.expand(R, -1, -1).contiguous(), cs.V.expand(R, -1, -1).contiguous(), cs.v0[0].expand(R, -1).contiguous()
    sh, per = cs.hvp(rows, x=x0), cs.hvp(rows, x=xs, v=vs)
    lsh, lper = cs.lanczos(rows, steps, x=x0, v0=cs.v0[0].contiguous()), cs.lanczos(rows, steps, x=xs, v0=v0s)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(sh + lsh, per + lper))
    # the context's batch size does not matter
    other = _Case(name, batch=7)
    assert torch.equal(other.params, cs.params)
    ob, lob = other.hvp(rows), other.lanczos(rows, steps)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a + la, ob + lob))
    assert torch.equal(cs.params, before), "params were written"


@pytest.mark.parametrize("name", sorted(DRAW))
def test_drawing_mode_equals_explicit_mode(name):
    """Kinds 0 (linear_gaussian) and 2 (sphere): the call that draws its rows = the call on the rows vaek_make_batch writes, bitwise."""
    cs = _case(name)
    rows, steps = 300, 8
    x = torch.stack([cs.drawn_rows(r, rows) for r in range(R)]).contiguous()
    assert x.shape == (R, rows, cs.c.D)
    d, e = cs.hvp(rows, draw=True), cs.hvp(rows, x=x)
    ld, le = cs.lanczos(rows, steps, draw=True), cs.lanczos(rows, steps, x=x)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(d + ld, e + le))
    assert float(le[1][0, 2]) >= 1 and not torch.equal(d[2][0], d[2][1])


def test_the_lanczos_call_is_capturable():
    """A captured call replayed twice = the eager call."""
    cs = _case("D12_L20")
    rows, steps = 300, 8
    eb, eo = cs.lanczos(rows, steps, draw=True)                           # eager (also the warm-up)
    torch.cuda.synchronize()
    basis, out = _full(*eb.shape), _full(*eo.shape)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a = dict(params=cs.params, rows=rows, steps=steps, v0=cs.v0, basis=basis, out=out, basis_stride=basis.shape[1])
    a.update(cs.rows_kw(rows, slice(None), True))
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            cs.eng.elbo_hessian_lanczos_replicas(**a)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                      # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eo) and torch.equal(basis, eb)
        out[:, :LEN] = 0.0


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_arguments_predicate_and_profile_labels():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message that names the call and leaves the outputs alone; the
    predicate on engines the calls do not cover; one profile record per call."""
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    cs, sph = _case("D12_L20"), _case("D13_L5")
    rows, steps, P = 37, 4, cs.P
    outs = dict(hv=_full(R, 2 * P), grad=_full(R, P), hout=_full(R, 4), basis=_full(R, steps * P), lout=_full(R, LEN))
    v = cs.V[:2].contiguous()

    def hvp_args(e=cs, **kw):
        a = dict(params=e.params, rows=rows, out=outs["hout"], v=v, hv=outs["hv"], grad=outs["grad"], nvec=2)
        a.update(e.rows_kw(rows, slice(None), True))
        a.update(kw)
        if torch.is_tensor(a["hv"]):                                      # [R, nvec * P]: replica r's block starts at row r, which the
            a.setdefault("hv_stride", a["hv"].shape[1])                    # engine's default (that of [n, nvec, P]) would not say
        return a

    def lan_args(e=cs, **kw):
        a = dict(params=e.params, rows=rows, steps=steps, v0=e.v0, basis=outs["basis"], out=outs["lout"])
        a.update(e.rows_kw(rows, slice(None), True))
        a.update(kw)
        if torch.is_tensor(a["basis"]):                                   # [R, steps * P]: as for hv
            a.setdefault("basis_stride", a["basis"].shape[1])
        return a

    def refused(why, which="both", e=cs, **kw):
        before = e.params.clone()
        for name, fn, args in (("vaek_elbo_hvp_replicas", "elbo_hvp_replicas", hvp_args), ("vaek_elbo_hessian_lanczos_replicas",
                                                                                          "elbo_hessian_lanczos_replicas", lan_args)):
            if which not in ("both", fn):
                continue
            a = args(e, **kw)
            eng = a.pop("eng", e.eng)
            with pytest.raises(VaekError) as ei:
                getattr(eng, fn)(**a)
            assert ei.value.code == -1 and name in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs.values()) and torch.equal(e.params, before), why

    two = Engine(100, 13, 5, (), (), -1.0, True, True)                     # a two-decoder (sigmoid) context
    assert two.supports_log_likelihood(1) and not two.supports_elbo_hessian(1)
    for why, eng in [("two decoders", two), ("mlp3", Engine(100, 13, 5, (200, 200, 200), (200, 200, 200), -1.0, False, False)),
                     ("one hidden layer", Engine(100, 13, 5, (64,), (64,), -1.0, False, False)),
                     ("bf16", Engine(100, 13, 5, (), (), -1.0, False, False, dtype="bf16"))]:
        assert not eng.supports_elbo_hessian(2), why
        refused(why, e=sph, eng=eng)
        with pytest.raises(VaekError):
            eng.elbo_hessian_basis_doubles(4)
    assert not Engine(100, 33, 6, (), (), -1.0, True, False).supports_elbo_hessian(0)      # D > 32
    assert not Engine(100, 6, 33, (), (), -1.0, True, False).supports_elbo_hessian(0)      # L > 32
    for kind in (-1, 0, 1, 2, 3):                                          # = the exact log-likelihood's predicate
        assert cs.eng.supports_elbo_hessian(kind) == cs.eng.supports_exact_log_likelihood(kind) == (0 <= kind <= 2)
    assert cs.eng.elbo_hessian_basis_doubles(steps) == steps * P and cs.eng.elbo_hvp_max_vectors == 64 and cs.eng.elbo_hessian_max_steps == 32
    for bad in (0, 33):
        with pytest.raises(VaekError):
            cs.eng.elbo_hessian_basis_doubles(bad)
    refused("struct_size", struct_size=12)
    refused("params NULL", params=None, n=R, state_stride=P + 5)
    for fn, who in ((cs.eng.lib.vaek_elbo_hvp_replicas, "vaek_elbo_hvp_replicas"),
                    (cs.eng.lib.vaek_elbo_hessian_lanczos_replicas, "vaek_elbo_hessian_lanczos_replicas")):      # a NULL description
        assert fn(cs.eng.h, cs.params.data_ptr(), None, 0, cs.A.data_ptr(), 3, 3, 9, 0.01, X_TAG, None) == -1
        assert who in cs.eng.lib.vaek_last_error().decode()
    refused("n = 0", n=0)
    refused("n over the cap", n=1025)
    refused("rows = 0", rows=0)
    refused("rows over the cap", rows=4097)
    refused("x_seeds NULL", x_seeds=None)
    refused("x_steps NULL", x_steps=None)
    refused("out NULL", out=None)
    refused("state_stride < P", state_stride=P - 1)
    refused("x_stride < 0", x=cs.x[:, :rows].contiguous(), x_stride=-1)
    refused("0 < x_stride < rows * D", x=cs.x[:, :rows].contiguous(), x_stride=rows * cs.c.D - 1)
    refused("a_stride < 0", a_stride=-1)
    refused("A NULL, kind 0", A=None)
    refused("dd = 17", dd=17)
    refused("did = 17", did=17)
    refused("kind 3", kind=3)
    refused("kind -1", kind=-1)
    refused("x_tag = 2^30", x_tag=2 ** 30)
    refused("dataset dimension != data_dim", pad=4)
    refused("A NULL, kind 1", kind=1, A=None, pad=8)
    refused("kind 1 counts one more column: 3 + 9 + 1 != 12", kind=1)
    h, l = "elbo_hvp_replicas", "elbo_hessian_lanczos_replicas"
    refused("nvec = -1", h, nvec=-1)
    refused("nvec = 65", h, nvec=65)
    refused("v NULL", h, v=None, nvec=2)
    refused("hv NULL", h, hv=None)
    refused("hv_stride < nvec * P", h, hv_stride=2 * P - 1)
    refused("0 < v_stride < nvec * P", h, v_stride=2 * P - 1)
    refused("v_stride < 0", h, v_stride=-1)
    refused("grad_stride < P", h, grad_stride=P - 1)
    refused("out_stride < 4", h, out_stride=3)
    refused("hv misaligned", h, hv=outs["hv"].data_ptr() + 4, hv_stride=2 * P)
    refused("v misaligned", h, v=v.data_ptr() + 4, v_stride=0)
    refused("grad misaligned", h, grad=outs["grad"].data_ptr() + 4, grad_stride=P)
    refused("out misaligned", h, out=outs["hout"].data_ptr() + 4, out_stride=4)
    refused("steps = 0", l, steps=0)
    refused("steps = 33", l, steps=33)
    refused("v0 NULL", l, v0=None)
    refused("basis NULL", l, basis=None)
    refused("basis_stride < steps * P", l, basis_stride=steps * P - 1)
    refused("0 < v0_stride < P", l, v0_stride=P - 1)
    refused("v0_stride < 0", l, v0_stride=-1)
    refused("out_stride < 140", l, out_stride=LEN - 1)
    refused("basis misaligned", l, basis=outs["basis"].data_ptr() + 4, basis_stride=steps * P)
    refused("v0 misaligned", l, v0=cs.v0.data_ptr() + 4, v0_stride=0)
    refused("out misaligned", l, out=outs["lout"].data_ptr() + 4, out_stride=LEN)
    # kind 1 with dd + pad + 1 = data_dim is legal; the caps and the empty product are legal; one profile record per call
    cs.eng.elbo_hessian_lanczos_replicas(**lan_args(kind=1, pad=8))
    cs.eng.profile_begin(16)
    a = hvp_args(v=None, hv=None, nvec=0)
    cs.eng.elbo_hvp_replicas(**a)
    cs.eng.elbo_hvp_replicas(**hvp_args(rows=4096))
    cs.eng.elbo_hessian_lanczos_replicas(**lan_args(A=cs.A[0].clone(), a_stride=0))
    sph.eng.elbo_hessian_lanczos_replicas(**lan_args(sph, A=None, basis=_full(R, steps * sph.P), basis_stride=steps * sph.P))
    torch.cuda.synchronize()
    rep = cs.eng.profile_report()
    assert sorted(rep) == ["elbo_hessian_replicas", "elbo_hvp_replicas"], rep
    assert rep["elbo_hvp_replicas"]["count"] == 2 and rep["elbo_hessian_replicas"]["count"] == 1, rep


# ---- 8. one run.py line --------------------------------------------------------------------------------------------------------------------------
def _run_py(tmp_path, name, *extra, dataset="linear_gaussian"):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", dataset, "--encoder_layer_sizes", "", "--layer_sizes", "",
           "-ow", "--latent_dim", "20", "--padding_dim", "9", "-dd", "3", "--epsilon", "-1", "-tdv", "--num_batches", "60", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


NEW_KEYS = ("ELBO Hessian Ritz Values", "ELBO Hessian Ritz Residuals", "Sharpness", "ELBO Hessian Min Ritz", "ELBO Gradient Norm")


def test_run_py_with_and_without_the_flag(tmp_path):
    """A 12 / 20 linear_gaussian line, 60 batches, --elbo_hessian 8, in a fresh child process: losses.npz gains the new keys, one entry
    per event (60 batches hold one n_print event, at batch 0); the run without the flag leaves byte-identical `VAE Loss`."""
    losses = {}
    for name, extra in (("plain", ()), ("hess", ("--elbo_hessian", "8"))):
        r = _run_py(tmp_path, name, *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("(vaek_elbo_hessian_lanczos_replicas)" in r.stdout) == (name == "hess"), r.stdout[-1500:]
        assert ("Sharpness |" in r.stdout) == (name == "hess"), r.stdout[-1500:]
        losses[name] = dict(np.load(os.path.join(str(tmp_path), "data", name, "losses.npz"), allow_pickle=True))
    plain, hess = losses["plain"], losses["hess"]
    assert sorted(k for k in hess if k not in NEW_KEYS) == sorted(plain) and not any(k in plain for k in NEW_KEYS)
    a, b = np.asarray(plain["VAE Loss"]), np.asarray(hess["VAE Loss"])
    events = 1
    assert a.size >= 1 and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for k in NEW_KEYS:
        assert len(hess[k]) == events, (k, len(hess[k]), events)
    for ev in range(events):
        th = np.asarray(hess[NEW_KEYS[0]][ev], dtype=np.float64)
        rho = np.asarray(hess[NEW_KEYS[1]][ev], dtype=np.float64)
        assert 1 <= th.size <= 8 and rho.shape == th.shape and np.all(np.diff(th) >= 0) and np.all(rho >= 0)
        assert float(hess["Sharpness"][ev]) == th[-1] and float(hess["ELBO Hessian Min Ritz"][ev]) == th[0]
        assert float(hess["ELBO Gradient Norm"][ev]) >= 0.0 and np.isfinite(th).all()
    print({k: np.asarray(hess[k][-1]).tolist() for k in NEW_KEYS})
    r = _run_py(tmp_path, "sig", "--elbo_hessian", dataset="sigmoid")
    assert r.returncode != 0 and "--elbo_hessian needs" in r.stderr and "Batch |" not in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
