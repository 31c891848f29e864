"""-m gpu: vaek_mlp3_sampled_elbo_hvp_replicas and vaek_mlp3_sampled_elbo_hessian_lanczos_replicas -- Hessian-vector products, the
gradient and a Lanczos spectrum of the SAMPLE-AVERAGE ELBO f_K of N three-hidden-layer MLP VAEs (csrc/mlp3_hessian.hip) -- the event
class and `run.py --mlp_sampled_elbo_hessian`.

References (cases and bounds: tests/mlp3_hessian_cases.py):
  - the float64 restatement tools/mlp3_hessian_reference.py on the identical rows, samples and parameters (itself held to torch autograd
    and to the oracle by tests/test_mlp3_hessian_host.py): every element of H v and of the gradient, and f_K, within 64 n_chain 2^-53
    times its magnitude image;
  - vaek_train_step_grads_only, the merged training kernel: with K = 1 and xi = z1 the gradient is the one it computes (float32);
  - the restatement applied to the device's own Lanczos basis (the three-term recurrence), numpy's eigvalsh of the record's own T, and
    the CPU Lanczos run on the restated H v;
  - itself, BITWISE: two runs, replica r of n = 3 against n = 1, drawing mode against explicit rows and samples, shared against
    per-replica strides, engines of two batch sizes, a captured replay."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import mlp3_hessian_cases as K
from tests.gpu_util import _i32, _i64, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
R = K.R
PAD = 3                                      # sentinel doubles behind every per-replica block and behind the workspace's stated size
LEN, HEAD, MS = 142, 12, 32
KEYS = ("Sampled ELBO Hessian Ritz Values", "Sampled ELBO Hessian Ritz Residuals", "Sampled Sharpness", "Sampled ELBO Hessian Min Ritz",
        "Sampled ELBO Gradient Norm")


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def _full(*shape):
    return torch.full(shape, SENT, dtype=torch.float64, device="cuda")


def _np(t):
    return t.cpu().numpy()


def _pads_untouched(t, length):
    return bool((t[:, length:] == SENT).all())


def _engine(name, batch=100, **kw):
    from vae_training_amd.engine import Engine
    s = K.SHAPES[name]
    return Engine(batch, s["D"], s["L"], s["enc"], s["dec"], K.EPS_CLI, s["tdv"], False, **kw)


class _Shape:
    """One engine and R replicas of a shape with distinct parameters; the parameter stack's stride exceeds P by 5 sentinel floats, every
    output block is followed by PAD sentinel doubles and the workspace starts as sentinels with PAD more behind its stated size."""

    def __init__(self, name, batch=100):
        self.name, self.s = name, K.SHAPES[name]
        self.eng = e = _engine(name, batch)
        self.P = P = e.P
        self.D, self.L = self.s["D"], self.s["L"]
        assert P == K.param_count(name) and e.supports_mlp3_sampled_elbo_hessian(2) and e.sampled_elbo_hessian_record_len == LEN
        self.params = torch.full((R, P + 5), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :P] = _dev(np.stack([K.make_theta(name, r) for r in range(R)]), torch.float32)
        big = (name, K.MAX_ROWS, K.MAX_K)
        self.x = _dev(np.stack([K.make_rows(big, r) for r in range(R)]), torch.float32)             # [R, 37, D]
        self.xi = _dev(np.stack([K.make_samples(big, r) for r in range(R)]), torch.float32)         # [R, 37, 3, L]
        self.v0 = _dev(np.stack([K.start_vector(name, r) for r in range(R)]))
        self.V64 = K.directions(name)
        self.V = _dev(self.V64)
        self.draw = dict(kind=2, dd=3, did=3, pad=self.D - 3, var=0.0)                              # the sphere dataset: no matrix
        self.tabs = (_i64(K.X_SEEDS), _i32(K.X_STEPS), _i64(K.Z_SEEDS), _i32(K.Z_STEPS))

    def workspace(self, n, rows, samples):
        nbytes = self.eng.mlp3_sampled_elbo_hessian_workspace(n, rows, samples)
        assert nbytes == K.workspace_bytes(self.name, n, rows, samples), (nbytes, K.workspace_bytes(self.name, n, rows, samples))
        return torch.full((nbytes // 8 + PAD,), SENT, dtype=torch.float64, device="cuda")

    def source_kw(self, rows, samples, sl, draw):
        if not draw:
            return dict(x=self.x[sl, :rows].contiguous(), xi=self.xi[sl, :rows, :samples].contiguous())
        d = self.draw
        return dict(kind=d["kind"], A=None, dd=d["dd"], did=d["did"], pad=d["pad"], var_added=d["var"], samples=samples, x_seeds=self.tabs[0][sl],
                    x_steps=self.tabs[1][sl], z_seeds=self.tabs[2][sl], z_steps=self.tabs[3][sl], x_tag=K.X_TAG, z_tag=K.Z_TAG)

    def hvp(self, rows, samples, v=None, rs=None, draw=False, grad=True, eng=None, **kw):
        """(hv [n, nvec * P + PAD], grad [n, P + PAD], out [n, 4 + PAD], workspace) of replicas `rs` (default all)."""
        sl = slice(None) if rs is None else rs
        n = self.params[sl].shape[0]
        v = self.V if v is None else v
        nvec = v.shape[-2]
        hv, g, out, ws = _full(n, nvec * self.P + PAD), _full(n, self.P + PAD), _full(n, 4 + PAD), self.workspace(n, rows, samples)
        a = dict(params=self.params[sl], rows=rows, out=out, workspace=ws, v=v, hv=hv, grad=g if grad else None, nvec=nvec, hv_stride=hv.shape[1])
        a.update(self.source_kw(rows, samples, sl, draw))
        a.update(kw)
        a["samples"] = samples
        if a["nvec"] == 0:
            a.update(v=None, hv=None, hv_stride=0)
        (eng or self.eng).mlp3_sampled_elbo_hvp_replicas(**a)
        return hv, g, out, ws

    def lanczos(self, rows, samples, steps, rs=None, draw=False, eng=None, **kw):
        """(basis [n, steps * P + PAD], out [n, 142 + PAD], workspace)."""
        sl = slice(None) if rs is None else rs
        n = self.params[sl].shape[0]
        basis, out, ws = _full(n, steps * self.P + PAD), _full(n, LEN + PAD), self.workspace(n, rows, samples)
        a = dict(params=self.params[sl], rows=rows, steps=steps, v0=self.v0[sl], basis=basis, out=out, workspace=ws, basis_stride=basis.shape[1])
        a.update(self.source_kw(rows, samples, sl, draw))
        a.update(kw)
        a["samples"] = samples
        (eng or self.eng).mlp3_sampled_elbo_hessian_lanczos_replicas(**a)
        return basis, out, ws

    def drawn(self, r, rows, samples):
        """(x [rows, D], xi [rows, K, L]) float32 device tensors: replica r's rows as vaek_make_batch writes them and its samples by the
        block rule, cut from the row's latent stream as an engine of 32 + 32 latent normals per row draws it."""
        d = self.draw
        x = self.eng.make_batch(d["kind"], None, d["dd"], d["did"], d["pad"], d["var"], rows, K.X_SEEDS[r], step=K.X_STEPS[r], tag=K.X_TAG,
                                want_z=False)[0]
        _, z1, z2 = _wide_engine().make_batch(2, None, 16, 16, 16, 0.0, rows, K.Z_SEEDS[r], step=K.Z_STEPS[r], tag=K.Z_TAG, want_x=False)
        stream = torch.cat([z1, z2], dim=1)                               # the first 64 normals of every row's stream
        nlb = (self.L + 3) // 4
        assert samples * nlb * 4 <= 64
        xi = torch.stack([stream[:, 4 * nlb * k:4 * nlb * k + self.L] for k in range(samples)], dim=1)
        return x.contiguous(), xi.contiguous()


@functools.lru_cache(maxsize=None)
def _wide_engine():
    from vae_training_amd.engine import Engine
    return Engine(100, 32, 32, (), (), -1.0, False, False)


@functools.lru_cache(maxsize=None)
def _shape(name):
    return _Shape(name)


_ID = lambda c: f"{c[0]}-{c[1]}x{c[2]}"


# ---- 7. the hvp call against the restatement (on the parent commit the symbols do not exist) -------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=_ID)
def test_hvp_gradient_and_f_match_the_restatement(case):
    name, rows, samples = case
    cs = _shape(name)
    P = cs.P
    hv, g, out, ws = cs.hvp(rows, samples)
    assert _pads_untouched(hv, 3 * P) and _pads_untouched(g, P) and _pads_untouched(out, 4) and bool((ws[-PAD:] == SENT).all())
    worst = [0.0, 0.0, 0.0]
    for r in range(R):
        m, mg = K.model(case, r), K.model(case, r, mag=True)
        rec = _np(out)[r]
        got_hv, got_g = _np(hv)[r, :3 * P].reshape(3, P), _np(g)[r, :P]
        ratios = (K.worst_ratio(rec[0] - m.f(), K.value_bound(case, mg.f())), K.worst_ratio(got_g - m.grad(), K.value_bound(case, mg.grad())),
                  K.worst_ratio(got_hv - m.hvp(cs.V64), K.value_bound(case, mg.hvp(cs.V64))))
        worst = [max(a, b) for a, b in zip(worst, ratios)]
        assert rec[1] == pytest.approx(np.linalg.norm(m.grad()), rel=1e-12) and rec[2] == m.eps and rec[3] == rows
    print(f"{case}: |device - restatement| / bound over {R} replicas: f {worst[0]:.3e}  gradient {worst[1]:.3e}  H v {worst[2]:.3e}")
    assert max(worst) <= 1.0
    # nvec = 0: the gradient and the record only, v and hv not read; grad = NULL: the record only
    hv0, g0, out0, _ = cs.hvp(rows, samples, nvec=0)
    assert torch.equal(g0, g) and torch.equal(out0, out) and bool((hv0 == SENT).all())
    _, g1, out1, _ = cs.hvp(rows, samples, nvec=0, grad=False)
    assert bool((g1 == SENT).all()) and torch.equal(out1, out)


# ---- 8. the tie to the merged training kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["narrow", "script1"])
def test_with_one_sample_the_gradient_is_the_training_kernels(name):
    """37 rows, K = 1, explicit xi = z1: grad f_K against vaek_train_step_grads_only (step path mlp3, batch 37, z2 = 0) under the
    tolerances tests/test_gpu_mlp3.py holds that float32 gradient to against the oracle."""
    cs = _shape(name)
    rows, P = 37, cs.P
    eng = _engine(name, rows)
    assert eng.fused and eng.step_path == "mlp3"
    x, z1 = cs.x[0, :rows].contiguous(), cs.xi[0, :rows, 0].contiguous()
    grads = eng.new_flat(eng.grad_len)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.grads_only(cs.params[0, :P].contiguous(), grads, step, x, z1, torch.zeros(rows, cs.D, device="cuda"))
    _, g, out, _ = cs.hvp(rows, 1, rs=slice(0, 1), nvec=0)
    want, got = _np(grads).astype(np.float64)[:P], _np(g)[0, :P]
    print(f"{name}: flat gradient rel err against vaek_train_step_grads_only {rel_err(got, want):.3g}")
    assert rel_err(got, want) <= 2e-5
    assert abs(float(out[0, 0]) - float(grads[P])) <= 1e-5 * abs(float(grads[P]))
    for leaf, (off, shape) in eng.leaves.items():
        n = int(np.prod(shape))
        err = np.max(np.abs(got[off:off + n] - want[off:off + n])) / (np.max(np.abs(want[off:off + n])) + 1e-30)
        assert err <= 1e-4, (leaf, err)


# ---- 9. symmetry -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("mixed", 5, 3), ("odd", 37, 2), ("narrow_notdv", 9, 1)], ids=_ID)
def test_the_operator_is_symmetric(case):
    """u^T (H v) = v^T (H u) within the sum of the two products' bounds, for a dense pair and for the dense direction against the one
    supported on epsilon_p and epsilon."""
    name, rows, samples = case
    cs = _shape(name)
    P = cs.P
    U2 = np.stack([cs.V64[0], np.random.default_rng(77).standard_normal(P), cs.V64[2]])
    hv, _, _, _ = cs.hvp(rows, samples, v=_dev(U2), rs=slice(0, 1))
    H = _np(hv)[0, :3 * P].reshape(3, P)
    mg = K.model(case, 0, mag=True)
    B = K.value_bound(case, mg.hvp(U2))
    for i, j in ((0, 1), (0, 2)):
        lhs, rhs = float(U2[i] @ H[j]), float(U2[j] @ H[i])
        bound = float(np.abs(U2[i]) @ B[j] + np.abs(U2[j]) @ B[i])
        print(f"{case} ({i}, {j}): u^T H v {lhs:.12e}  v^T H u {rhs:.12e}  |difference| / bound {abs(lhs - rhs) / bound:.3e}")
        assert abs(lhs - rhs) <= bound


# ---- 10. Lanczos -------------------------------------------------------------------------------------------------------------------------------
def _check_record(cs, case, rec, basis, steps):
    """The structure of one record and its basis block; returns (k, alpha, beta, theta, rho, omega)."""
    P = cs.P
    k = int(rec[2])
    al, be = rec[HEAD + 2 * MS:HEAD + 2 * MS + k], rec[HEAD + 3 * MS:HEAD + 3 * MS + k]
    theta, rho = rec[HEAD:HEAD + k], rec[HEAD + MS:HEAD + MS + k]
    assert 1 <= k <= steps and rec[7] == case[1] and rec[140] == case[2] and rec[141] == 0.0
    if k < steps:                                                         # only a breakdown ends a run early
        assert be[k - 1] <= 2.0 ** -40 * max(np.max(np.abs(al)), np.max(be[:k - 1], initial=0.0))
    for blk in range(4):                                                  # slots >= k are 0
        assert not np.any(rec[HEAD + blk * MS + k:HEAD + (blk + 1) * MS])
    assert np.all(np.diff(theta) >= 0) and np.all(rho >= 0) and rec[9] == theta[-1] and rec[10] == theta[0] and rec[3] == be[k - 1]
    B = basis[:steps * P].reshape(steps, P)
    assert np.all(B[k:] == SENT) and np.all(basis[steps * P:] == SENT)    # rows >= k and the pad are untouched
    # a. the basis is orthonormal to OMEGA_MAX and the record's omega is its measured value
    G = B[:k] @ B[:k].T
    assert rec[11] <= K.OMEGA_MAX and np.max(np.abs(G - np.eye(k))) <= 2 * K.OMEGA_MAX
    assert rec[11] == pytest.approx(np.max(np.abs(G - np.diag(np.diag(G)))), abs=1e-15)
    # c. the record's Ritz values are eigvalsh of the record's own (alpha, beta), rho_i = |beta_k s_ki|
    T = np.diag(al) + np.diag(be[:k - 1], 1) + np.diag(be[:k - 1], -1)
    norm_t = float(np.sqrt(np.sum(T * T)))
    lam, S = np.linalg.eigh(T)
    assert rec[6] == pytest.approx(norm_t, rel=1e-13) and np.max(np.abs(lam - theta)) <= 64 * k * K.U * norm_t
    # (an eigenvector moves by |dT| / gap, |dT| what the device's solve left off the diagonal plus numpy's own rounding)
    gap = np.array([np.min(np.abs(np.delete(lam, i) - lam[i])) if k > 1 else np.inf for i in range(k)])
    d_t = max(rec[5], 2.0 ** -43 * norm_t) + 64 * k * K.U * norm_t
    tol = be[k - 1] * (64 * k * K.U + (4.0 * d_t / np.maximum(gap, d_t) if d_t > 0.0 else 0.0))
    assert np.all(np.abs(rho - np.abs(be[k - 1] * S[k - 1])) <= tol), (rho, np.abs(be[k - 1] * S[k - 1]), tol)
    assert rec[5] <= 2.0 ** -40 * rec[6]
    return k, al, be, theta, rho, rec[11], B


@pytest.mark.parametrize("case,steps", K.LANCZOS_CASES, ids=lambda v: _ID(v) if isinstance(v, tuple) else str(v))
def test_lanczos_against_the_restated_operator_and_the_cpu_run(case, steps):
    name, rows, samples = case
    cs = _shape(name)
    P = cs.P
    basis, out, _ = cs.lanczos(rows, samples, steps, rs=slice(0, 1))
    assert _pads_untouched(out, LEN)
    rec, bas = _np(out)[0], _np(basis)[0]
    k, al, be, theta, rho, omega, B = _check_record(cs, case, rec, bas, steps)
    _, _, hout, _ = cs.hvp(rows, samples, rs=slice(0, 1), nvec=0)
    assert rec[0] == float(hout[0, 0]) and rec[1] == float(hout[0, 1]) and rec[8] == float(hout[0, 2])      # one gradient text
    m, mg = K.model(case), K.model(case, mag=True)
    cpu = K.ref().lanczos(m.hvp, K.start_vector(name), steps)
    norm_h = float(np.max(np.abs(cpu["theta"])))                          # a LOWER bound of |H|_2: the slack it scales is not inflated
    slack = K.ritz_slack(P, k, omega, norm_h)
    # b. the three-term recurrence under the restated operator applied to the device's basis rows
    HB, MB = m.hvp(B[:k]), mg.hvp(B[:k])
    worst = 0.0
    for j in range(k):
        res = HB[j] - al[j] * B[j] - (be[j - 1] * B[j - 1] if j else 0.0)
        bound = float(np.linalg.norm(K.value_bound(case, MB[j]))) + slack
        err = float(np.linalg.norm(res - be[j] * B[j + 1])) if j + 1 < k else abs(float(np.linalg.norm(res)) - be[j])
        worst = max(worst, err / bound)
        assert err <= bound, (j, err, bound)
    # d. every converged device Ritz value has a CPU-Lanczos Ritz value next to it
    conv = [i for i in range(k) if rho[i] <= 1e-6 * theta[-1]]
    for i in conv:
        assert np.min(np.abs(cpu["theta"] - theta[i]) - cpu["rho"]) <= rho[i] + slack, (i, theta[i], rho[i])
    print(f"{case} steps {steps}: k {k} (CPU {cpu['k']})  omega {omega:.2e}  theta_max {theta[-1]:.9e} (CPU {cpu['theta'][-1]:.9e}, rho {rho[-1]:.1e})  "
          f"theta_min {theta[0]:.6e} (CPU {cpu['theta'][0]:.6e})  converged {len(conv)}  worst recurrence residual / bound {worst:.3e}")
    assert k == cpu["k"]


# ---- 11. breakdown and degenerate starts ---------------------------------------------------------------------------------------------------
def test_breakdown_and_start_vectors_that_end_the_run_at_once():
    """The breakdown case of tests/mlp3_hessian_cases.py (one column, v0 on the weights of dead Decoder/FC1 units: H v0 = 0): k = 1 <
    steps, the done flag of every later step set, basis rows >= 1 untouched, the record complete.  v0 = 0 and a v0 with a NaN: k = 0."""
    case = K.BREAKDOWN_CASE
    name, rows, samples = case
    cs = _shape(name)
    P, steps = cs.P, 32
    v0 = _dev(np.stack([K.breakdown_start(case, r) for r in range(R)]))
    basis, out, ws = cs.lanczos(rows, samples, steps, v0=v0)
    rec, bas = _np(out), _np(basis)
    block = K.workspace_doubles(name, rows, samples)
    state = K.WS_HEAD + ((P + 1) & ~1) + K.WS_TAIL                        # one tile
    for r in range(R):
        k, al, be, theta, rho, omega, B = _check_record(cs, case, rec[r], bas[r], steps)
        assert k == 1 and al[0] == 0.0 and be[0] == 0.0 and theta[0] == 0.0 and rho[0] == 0.0 and omega == 0.0
        v = K.breakdown_start(case, r)
        assert np.allclose(B[0], v / np.linalg.norm(v), rtol=1e-14, atol=0.0)
        done = _np(ws)[r * block + state + 136:r * block + state + 136 + 33]
        assert done.tolist() == [0.0] + [1.0] * 32                       # flagged for every later step
        m = K.model(case, r)
        assert abs(rec[r, 0] - m.f()) <= K.value_bound(case, K.model(case, r, mag=True).f()) and rec[r, 1] > 0
    v0 = cs.v0.clone()
    v0[0].zero_()
    v0[1, 3] = float("nan")
    basis, out, _ = cs.lanczos(5, 3, 5, v0=v0)
    rec, bas = _np(out), _np(basis)
    for r in (0, 1):
        assert rec[r, 2] == 0 and not np.any(rec[r, 3:7]) and not np.any(rec[r, 9:140]) and np.all(bas[r] == SENT) and rec[r, 140] == 3
        assert np.isfinite(rec[r, 0]) and rec[r, 1] > 0 and rec[r, 7] == 5
    assert rec[2, 2] == 5 and _pads_untouched(out, LEN)


# ---- 12. draws, replicas, runs, strides, padding ----------------------------------------------------------------------------------------------
def test_drawing_mode_is_explicit_mode_on_the_drawn_bits():
    cs = _shape("narrow")
    rows, samples, steps = 5, 3, 4
    d_hv, d_g, d_out, _ = cs.hvp(rows, samples, draw=True)
    d_bas, d_rec, _ = cs.lanczos(rows, samples, steps, draw=True)
    for r in range(R):
        x, xi = cs.drawn(r, rows, samples)
        assert x.shape == (rows, cs.D) and xi.shape == (rows, samples, cs.L)
        sl = slice(r, r + 1)
        hv, g, out, _ = cs.hvp(rows, samples, rs=sl, x=x, xi=xi)
        assert torch.equal(hv, d_hv[sl]) and torch.equal(g, d_g[sl]) and torch.equal(out, d_out[sl]), r
        bas, rec, _ = cs.lanczos(rows, samples, steps, rs=sl, x=x, xi=xi)
        assert torch.equal(bas, d_bas[sl]) and torch.equal(rec, d_rec[sl]), r
        # rows drawn, samples explicit, and the other way round
        dk = cs.source_kw(rows, samples, sl, True)
        mixed = {k_: v for k_, v in dk.items() if k_ not in ("z_seeds", "z_steps", "samples")}
        hv2, _, out2, _ = cs.hvp(rows, samples, rs=sl, **{"x": None, "xi": xi, **mixed})
        assert torch.equal(hv2, hv) and torch.equal(out2, out)
        hv3, _, out3, _ = cs.hvp(rows, samples, rs=sl, x=x, xi=None, z_seeds=dk["z_seeds"], z_steps=dk["z_steps"], z_tag=K.Z_TAG)
        assert torch.equal(hv3, hv) and torch.equal(out3, out)
    assert not torch.equal(d_out[0], d_out[1])


def test_sample_zero_is_make_batch_z1_and_the_batch_size_does_not_matter():
    cs = _shape("script1")
    rows, d = 37, cs.draw
    other = _engine("script1", 257)
    for r in range(R):
        sl = slice(r, r + 1)
        x, _ = cs.drawn(r, rows, 1)
        _, z1, _ = cs.eng.make_batch(d["kind"], None, d["dd"], d["did"], d["pad"], d["var"], rows, K.Z_SEEDS[r], step=K.Z_STEPS[r], tag=K.Z_TAG,
                                     want_x=False)
        outs = [cs.hvp(rows, 1, rs=sl, draw=True, v=cs.V[:2].contiguous())[:3], cs.hvp(rows, 1, rs=sl, draw=True, v=cs.V[:2].contiguous(), eng=other)[:3],
                cs.hvp(rows, 1, rs=sl, v=cs.V[:2].contiguous(), x=x, xi=z1.reshape(rows, 1, cs.L).contiguous())[:3]]
        assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0])), r


def test_replicas_runs_and_strides_are_bitwise():
    cs = _shape("odd")
    P = cs.P
    rows, samples, steps = 37, 2, 3
    all3 = cs.hvp(rows, samples) + cs.lanczos(rows, samples, steps)
    again = cs.hvp(rows, samples) + cs.lanczos(rows, samples, steps)
    outs = lambda t: t[:3] + t[4:6]                                       # the workspaces aside: their pads are checked below
    for a, b in zip(outs(all3), outs(again)):                             # two runs
        assert torch.equal(a, b)
    for r in range(R):                                                    # replica r of n = 3 is the n = 1 call on its slices
        sl = slice(r, r + 1)
        one = cs.hvp(rows, samples, rs=sl) + cs.lanczos(rows, samples, steps, rs=sl)
        for a, b in zip(outs(all3), outs(one)):
            assert torch.equal(a[sl], b), r
    for t, length in zip(outs(all3), (3 * P, P, 4, steps * P, LEN)):
        assert _pads_untouched(t, length)
    for ws in (all3[3], all3[6]):                                         # nothing behind the workspace's stated size
        assert bool((ws[-PAD:] == SENT).all()) and ws.numel() == R * K.workspace_doubles("odd", rows, samples) + PAD
    # shared rows, samples, directions and start vector (stride 0) against per-replica copies of them
    x0, xi0 = cs.x[0, :rows].contiguous(), cs.xi[0, :rows, :samples].contiguous()
    sh = cs.hvp(rows, samples, x=x0, xi=xi0, v=cs.V) + cs.lanczos(rows, samples, steps, x=x0, xi=xi0, v0=cs.v0[0].contiguous())
    pr = (cs.hvp(rows, samples, x=x0.expand(R, -1, -1).contiguous(), xi=xi0.expand(R, -1, -1, -1).contiguous(),
                 v=cs.V.expand(R, -1, -1).contiguous())
          + cs.lanczos(rows, samples, steps, x=x0.expand(R, -1, -1).contiguous(), xi=xi0.expand(R, -1, -1, -1).contiguous(),
                       v0=cs.v0[0].expand(R, -1).contiguous()))
    for a, b in zip(outs(sh), outs(pr)):
        assert torch.equal(a, b)
    assert torch.equal(sh[0][0], all3[0][0]) and not torch.equal(sh[0][1], all3[0][1])


# ---- 13. capture -------------------------------------------------------------------------------------------------------------------------------
def test_the_lanczos_call_is_capturable():
    """A captured call replayed twice = the eager call."""
    cs = _shape("narrow")
    rows, samples, steps = 37, 2, 6
    eb, eo, _ = cs.lanczos(rows, samples, steps, draw=True)               # eager (also the warm-up)
    torch.cuda.synchronize()
    basis, out, ws = _full(*eb.shape), _full(*eo.shape), cs.workspace(R, rows, samples)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a = dict(params=cs.params, rows=rows, steps=steps, v0=cs.v0, basis=basis, out=out, workspace=ws, basis_stride=basis.shape[1])
    a.update(cs.source_kw(rows, samples, slice(None), True))
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            cs.eng.mlp3_sampled_elbo_hessian_lanczos_replicas(**a)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                      # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eo) and torch.equal(basis, eb)
        out[:, :LEN] = 0.0


def test_the_launch_count_is_a_function_of_nvec_and_steps_alone():
    cs = _shape("narrow")
    cs.eng.profile_begin(256)
    cs.hvp(5, 3)
    cs.lanczos(5, 3, 4)
    torch.cuda.synchronize()
    rep = cs.eng.profile_report()
    count = lambda prefix: sum(v["count"] for k, v in rep.items() if k.startswith(prefix))
    assert count("mlp3_hessian_") == (3 + 2 * 3) + (6 + 6 * 4), rep
    assert rep["mlp3_hessian_hvp_chain"]["count"] == 3 + 4 and rep["mlp3_hessian_grad_chain"]["count"] == 2 and rep["mlp3_hessian_final"]["count"] == 1


# ---- 14. refusals on a live context ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context():
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    cs = _shape("narrow")
    P, rows, samples, steps = cs.P, 5, 3, 4
    outs = dict(hv=_full(R, 2 * P), grad=_full(R, P), hout=_full(R, 4), basis=_full(R, steps * P), lout=_full(R, LEN))
    ws = cs.workspace(R, rows, samples)
    v = cs.V[:2].contiguous()
    h, l = "mlp3_sampled_elbo_hvp_replicas", "mlp3_sampled_elbo_hessian_lanczos_replicas"

    def hvp_args(**kw):
        a = dict(params=cs.params, rows=rows, out=outs["hout"], workspace=ws, v=v, hv=outs["hv"], grad=outs["grad"], nvec=2)
        a.update(cs.source_kw(rows, samples, slice(None), True))
        a.update(kw)
        if torch.is_tensor(a["hv"]):
            a.setdefault("hv_stride", a["hv"].shape[1])
        return a

    def lan_args(**kw):
        a = dict(params=cs.params, rows=rows, steps=steps, v0=cs.v0, basis=outs["basis"], out=outs["lout"], workspace=ws)
        a.update(cs.source_kw(rows, samples, slice(None), True))
        a.update(kw)
        if torch.is_tensor(a["basis"]):
            a.setdefault("basis_stride", a["basis"].shape[1])
        return a

    def refused(why, match, which="both", **kw):
        before = cs.params.clone()
        for fn, args in ((h, hvp_args), (l, lan_args)):
            if which not in ("both", fn):
                continue
            a = args(**kw)
            eng = a.pop("eng", cs.eng)
            with pytest.raises(VaekError) as ei:
                getattr(eng, fn)(**a)
            assert ei.value.code == -1 and "vaek_" + fn + ": " in str(ei.value) and match in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs.values()) and bool((ws == SENT).all()) and torch.equal(cs.params, before), why

    # contexts the predicate does not cover
    lin = Engine(100, 7, 6, (), (), -1.0, True, False)
    two = Engine(100, 7, 6, (64, 64), (64, 64), -1.0, True, False)
    b16 = Engine(100, 7, 6, (64, 64, 64), (64, 64, 64), -1.0, True, False, dtype="bf16")
    for what, e in (("a linear context", lin), ("two hidden layers", two), ("bf16", b16)):
        assert not e.supports_mlp3_sampled_elbo_hessian(2), what
        big = torch.zeros(R, max(e.P, P) + 5, dtype=torch.float32, device="cuda")
        refused(what, "needs a float32 VAE with one decoder and three hidden layers of 64 .. 256 units both ways, D, L <= 32 (see "
                "vaek_supports_mlp3_sampled_elbo_hessian)", eng=e, params=big)
        with pytest.raises(VaekError, match="vaek_mlp3_sampled_elbo_hessian_workspace_bytes: an unsupported context"):
            e.mlp3_sampled_elbo_hessian_workspace(1, 5, 3)
    for kind in (-1, 0, 1, 2, 3):                                          # = the mlp3 log-likelihood's predicate, whatever the batch
        assert cs.eng.supports_mlp3_sampled_elbo_hessian(kind) == cs.eng.supports_mlp3_log_likelihood(kind) == (0 <= kind <= 2)
    assert _engine("narrow", 257, force_generic=True).supports_mlp3_sampled_elbo_hessian(2)
    # the linear call on an mlp3 context is still refused with its present message
    lws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(VaekError, match=r"vaek_sampled_elbo_hvp_replicas: .*needs a float32 linear VAE \(no hidden layers\) with one or two "
                                        r"decoders.*vaek_supports_sampled_elbo_hessian"):
        cs.eng.sampled_elbo_hvp_replicas(**{**hvp_args(), "workspace": lws})
    assert cs.eng.mlp3_sampled_elbo_hessian_max_columns == 1 << 14
    # the caps, each at its first refused value
    refused("samples = 0", "0 samples, need 1 .. 1024 (vaek_log_likelihood_max_samples)", samples=0)
    refused("samples = 1025", "1025 samples", samples=1025)
    refused("rows = 0", "0 rows, need 1 .. 4096 (vaek_log_likelihood_max_rows)", rows=0)
    refused("rows = 4097", "4097 rows, need 1 .. 4096 (vaek_log_likelihood_max_rows)", rows=4097)
    refused("rows x samples above 2^13", "4096 rows x 3 samples = 12288 columns per replica, at most 8192", rows=4096)
    refused("rows x samples above 2^13", "2731 rows x 3 samples = 8193 columns per replica, at most 8192", rows=2731)
    refused("n x rows x samples above 2^14", "3 replicas x 2731 rows x 2 samples = 16386 columns, at most 16384 "
            "(vaek_mlp3_sampled_elbo_hessian_max_columns)", rows=2731, samples=2)
    with pytest.raises(VaekError, match="vaek_mlp3_sampled_elbo_hessian_workspace_bytes.*8193 columns per replica"):
        cs.eng.mlp3_sampled_elbo_hessian_workspace(1, 2731, 3)
    with pytest.raises(VaekError, match="vaek_mlp3_sampled_elbo_hessian_workspace_bytes.*16386 columns, at most 16384"):
        cs.eng.mlp3_sampled_elbo_hessian_workspace(3, 2731, 2)
    assert cs.eng.mlp3_sampled_elbo_hessian_workspace(2, 4096, 2) == K.workspace_bytes("narrow", 2, 4096, 2)      # exactly both caps
    refused("nvec = 65", "65 vectors, need 0 .. 64 (vaek_elbo_hvp_max_vectors)", h, nvec=65)
    refused("nvec = -1", "-1 vectors", h, nvec=-1)
    refused("steps = 33", "33 steps, need 1 .. 32 (vaek_elbo_hessian_max_steps)", l, steps=33)
    refused("steps = 0", "0 steps", l, steps=0)
    refused("n = 0", "0 replicas", n=0)
    # the samples' source
    refused("z_seeds NULL", "z_seeds is NULL", z_seeds=None)
    refused("z_steps NULL", "z_steps is NULL", z_steps=None)
    refused("z_tag = 2^30", "tag >= 2^30", z_tag=2 ** 30)
    xi = cs.xi[:, :rows, :samples].contiguous()
    refused("0 < xi_stride < rows * K * L", f"xi_stride {rows * samples * cs.L - 1}", xi=xi, xi_stride=rows * samples * cs.L - 1)
    refused("xi_stride < 0", "xi_stride -1", xi=xi, xi_stride=-1)
    # buffers and strides: a short workspace cannot be detected, a NULL or misaligned one is refused
    refused("workspace NULL", "workspace is NULL or not 16-byte aligned (vaek_mlp3_sampled_elbo_hessian_workspace_bytes)", workspace=None)
    refused("workspace misaligned", "not 16-byte aligned", workspace=ws.data_ptr() + 8)
    refused("state_stride < P", f"state_stride {P - 1}", state_stride=P - 1)
    refused("out misaligned", "out is not 8-byte aligned", h, out=outs["hout"].data_ptr() + 4, out_stride=4)
    refused("out_stride < 4", "out_stride 3 < 1 x record length 4 (vaek_elbo_hvp_record_len)", h, out_stride=3)
    refused("hv misaligned", "hv is not 8-byte aligned", h, hv=outs["hv"].data_ptr() + 4, hv_stride=2 * P)
    refused("hv_stride short", f"hv stride {2 * P - 1} < its length {2 * P}", h, hv_stride=2 * P - 1)
    refused("v_stride short", f"v stride {2 * P - 1} < its length {2 * P} (0: shared)", h, v_stride=2 * P - 1)
    refused("grad misaligned", "grad is not 8-byte aligned", h, grad=outs["grad"].data_ptr() + 4, grad_stride=P)
    refused("grad_stride short", f"grad stride {P - 1} < its length {P}", h, grad_stride=P - 1)
    refused("basis misaligned", "basis is not 8-byte aligned", l, basis=outs["basis"].data_ptr() + 4, basis_stride=steps * P)
    refused("basis_stride short", f"basis stride {steps * P - 1} < its length {steps * P}", l, basis_stride=steps * P - 1)
    refused("v0 misaligned", "v0 is not 8-byte aligned", l, v0=cs.v0.data_ptr() + 4, v0_stride=0)
    refused("v0_stride short", f"v0 stride {P - 1} < its length {P} (0: shared)", l, v0_stride=P - 1)
    refused("v and hv overlap", "v and hv overlap", h, v=outs["hv"].data_ptr() + 8 * P, v_stride=0)
    refused("hv inside the shared v", "v and hv overlap", h, v=outs["hv"].data_ptr(), v_stride=2 * P)
    refused("out_stride < 142", "out_stride 141 < 1 x record length 142 (vaek_sampled_elbo_hessian_record_len)", l, out_stride=LEN - 1)
    refused("struct_size", "struct_size 12", struct_size=12)
    # the legal neighbours run
    cs.eng.mlp3_sampled_elbo_hvp_replicas(**hvp_args())
    cs.eng.mlp3_sampled_elbo_hessian_lanczos_replicas(**lan_args())
    torch.cuda.synchronize()
    assert not bool((outs["hout"] == SENT).any()) and not bool((outs["lout"] == SENT).any())


# ---- 15. the event class and run.py ----------------------------------------------------------------------------------------------------------
class _Model:
    """What ReplicaSampledElboHessianMlp3 asks of a VAEModel, around real engines."""

    def __init__(self, name, flat, seed, batch=100, world=1):
        s = K.SHAPES[name]
        engines = {}

        def engine(B, gb=0):
            if B not in engines:
                engines[B] = _engine(name, B) if world == 1 else _engine(name, B, world=world, rank=0, global_batch=B * world)
            return engines[B]
        self.model = types.SimpleNamespace(module=types.SimpleNamespace(engine=engine, tunable_decoder_var=True), flat=torch.as_tensor(flat).cuda())
        self.batch_size, self.print_batch_size = batch, 1000
        self.optimizer = types.SimpleNamespace(global_batch=0)
        self.dataset = types.SimpleNamespace(device_spec=lambda: (2, None, 3, 3, s["D"] - 3, 0.0), key=(seed, 2), _draws=5)
        self.key, self._latent_draws, self.dirname = (3, 4), 9, name


def test_the_event_on_real_models_at_initialisation():
    """trainer.ReplicaSampledElboHessianMlp3 on two script-shape models: its stats are the record slots of a direct call under
    (dataset.key[0] ^ dataset.key[1], the counter, tags 14 / 15 / 16), bitwise, and the run's RNG state is left alone.  A world of 2
    is refused by the class (the C predicate reads parameters only and does not look at the world)."""
    from vae_training_amd.trainer import ReplicaSampledElboHessianMlp3 as Ev
    name = "script1"
    flats = [K.make_theta(name, r).astype(np.float32) for r in range(2)]
    ms = [_Model(name, f, seed) for f, seed in zip(flats, (69, 24))]
    ev = Ev(ms, steps=6, rows=64)
    assert ev.samples == 1
    stats = ev.event()
    P = ev.P
    for r, m in enumerate(ms):
        seed = m.dataset.key[0] ^ m.dataset.key[1]
        v0 = ev.eng.rng_fill(P, seed, step=1, tag=16).double().reshape(1, P)
        basis, out = _full(1, 6, P), _full(1, LEN)
        ws = torch.zeros(ev.eng.mlp3_sampled_elbo_hessian_workspace(1, 64, 1), dtype=torch.uint8, device="cuda")
        ev.eng.mlp3_sampled_elbo_hessian_lanczos_replicas(m.model.flat.reshape(1, -1), 64, 6, v0, basis, out, ws, samples=1, kind=2, A=None, dd=3,
                                                          did=3, pad=3, var_added=0.0, x_seeds=_i64([seed % 2 ** 64]), x_steps=_i32([1]),
                                                          z_seeds=_i64([seed % 2 ** 64]), z_steps=_i32([1]), x_tag=14, z_tag=15)
        rec = _np(out)[0]
        k = int(rec[2])
        assert list(stats[r]) == list(KEYS) and k == 6 and rec[140] == 1.0 and rec[141] == 0.0
        assert np.array_equal(stats[r][KEYS[0]], rec[12:12 + k]) and np.array_equal(stats[r][KEYS[1]], rec[44:44 + k])
        assert [stats[r][k_] for k_ in KEYS[2:]] == [rec[9], rec[10], rec[1]] and m._mlp_hessian_draws == 1
        assert m.key == (3, 4) and m._latent_draws == 9 and m.dataset._draws == 5
        print(f"model {r}: sharpness {rec[9]:.6e}  min Ritz {rec[10]:.6e}  |grad| {rec[1]:.6e}")
    assert stats[0][KEYS[2]] != stats[1][KEYS[2]]
    with pytest.raises(RuntimeError, match="world"):
        Ev([_Model(name, flats[0], 69, world=2)], rows=64)


def _run_py(tmp_path, name, *extra, layers="200|200|200"):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", "sphere", "--encoder_layer_sizes", layers, "--layer_sizes", layers,
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "200", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def _same(a, b):
    """Bitwise equality of two values as np.load / the checkpoint loader return them."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == object:
        return all(_same(u, v) for u, v in zip(a.reshape(-1), b.reshape(-1)))
    return a.tobytes() == b.tobytes()


def _outputs(tmp_path, name):
    from vae_training_amd.model import load_checkpoint
    d = os.path.join(str(tmp_path), "data", name)
    return dict(np.load(os.path.join(d, "losses.npz"), allow_pickle=True)), load_checkpoint(os.path.join(d, "model.pkl"))


def _check_pair(plain, flagged, ckpt_plain, ckpt_flagged, who, steps):
    """The run with the flag against the run without: every stat of the plain run and the checkpoint (the parameters) bitwise equal;
    the five keys, one entry per n_print event (200 batches: the event of step 0), with the right shapes."""
    for k in plain:
        if k not in KEYS:
            assert _same(plain[k], flagged[k]), (who, k)
    assert _same(ckpt_plain, ckpt_flagged), who
    for k in KEYS:
        assert len(flagged[k]) == 1 and len(plain.get(k, ())) == 0, (who, k)
    th, rho = np.asarray(flagged[KEYS[0]][0], np.float64), np.asarray(flagged[KEYS[1]][0], np.float64)
    assert th.shape == rho.shape == (steps,) and np.all(np.diff(th) >= 0) and np.all(rho >= 0) and np.isfinite(th).all()
    assert float(flagged[KEYS[2]][0]) == th[-1] and float(flagged[KEYS[3]][0]) == th[0] and float(flagged[KEYS[4]][0]) > 0.0
    print(who, {k: np.asarray(flagged[k][-1]).tolist() for k in KEYS[2:]})


def test_run_py_single_model_and_the_refusals(tmp_path):
    """Line 1 of sphere_vae_padding_expts.sh, 200 batches, with and without --mlp_sampled_elbo_hessian, in fresh child processes; a
    linear model is refused before any step with the hint (the other refusals: tests/test_mlp3_hessian_host.py)."""
    outs = {}
    for name, extra in (("plain1", ()), ("hs1", ("--mlp_sampled_elbo_hessian",))):
        r = _run_py(tmp_path, name, *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = "Sampled ELBO Hessian events: 32 Lanczos steps on 1000 rows x 1 samples (vaek_mlp3_sampled_elbo_hessian_lanczos_replicas)"
        assert (line in r.stdout) == (name == "hs1") and ("Sampled Sharpness |" in r.stdout) == (name == "hs1"), r.stdout[-1500:]
        outs[name] = _outputs(tmp_path, name)
    _check_pair(outs["plain1"][0], outs["hs1"][0], outs["plain1"][1], outs["hs1"][1], "single model", 32)
    r = _run_py(tmp_path, "lin", "--mlp_sampled_elbo_hessian", layers="")
    assert r.returncode != 0 and "--mlp_sampled_elbo_hessian needs" in r.stderr and "use --sampled_elbo_hessian" in r.stderr, r.stderr[-1500:]
    assert "Batch |" not in r.stdout


def test_run_py_sweep_with_and_without_the_flag(tmp_path):
    """The same line with --sweep_dataset_seeds 69,24: one call per event for both models; the evaluation does not perturb the runs."""
    runs = {}
    for name, extra in (("plain", ()), ("hs", ("--mlp_sampled_elbo_hessian", "8", "--mlp_sampled_elbo_hessian_samples", "2"))):
        r = _run_py(tmp_path, name, "--sweep_dataset_seeds", "69,24", *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = ("Sampled ELBO Hessian events: 8 Lanczos steps on 1000 rows x 2 samples per model, one call for 2 models "
                "(vaek_mlp3_sampled_elbo_hessian_lanczos_replicas)")
        assert (line in r.stdout) == (name == "hs"), r.stdout[-1500:]
        runs[name] = {seed: _outputs(tmp_path, f"{name}_ds{seed}") for seed in (69, 24)}
    for seed in (69, 24):
        _check_pair(runs["plain"][seed][0], runs["hs"][seed][0], runs["plain"][seed][1], runs["hs"][seed][1], f"seed {seed}", 8)
    assert not _same(runs["hs"][69][0][KEYS[2]], runs["hs"][24][0][KEYS[2]])
