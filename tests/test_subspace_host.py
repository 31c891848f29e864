"""Host side of the eigenvectors and principal angles (csrc/cov_spectrum.hip), no GPU: the float64 restatement
(tools/cov_eigen_reference.py) on EVERY input set of cov_spectrum_cases.all_host_sets() -- sweeps and eigenvalues are those of the
eigenvalue-only restatement, and the constants K1 and K2 of the GPU bounds E1 and E2 (tests/subspace_cases.py) are pinned to its worst
case -- its angles against scipy.linalg.subspace_angles, the C ABI surface of the five new entry points, trainer.ReplicaSubspace on a
stub engine (both routes, one solve call, one angles call, the run untouched, what it refuses) and run.py's --subspace flag."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import cov_spectrum_cases as K
from tests import subspace_cases as Z
from tests.abi_util import _c_args
from tests.test_cov_spectrum_host import _StubEngine, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_cov_eigen_record_len", "vaek_cov_eigen_rows", "vaek_eigen_event_replicas", "vaek_subspace_record_len", "vaek_subspace_angles")
KEYS = ["learnt eigenvalue", "ground truth eigenvalue", "Principal Angles", "Subspace Distance"]


def _reference():
    spec = importlib.util.spec_from_file_location("cov_eigen_reference", os.path.join(ROOT, "tools", "cov_eigen_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_restatement_keeps_the_spectrum_and_pins_k1_and_k2():
    """V does not feed back into A: on every set the sweep count and the eigenvalues are cov_spectrum_reference.record's.  K1 is the
    smallest power of two that leaves the worst E1 at or below 1/4 of its bound; K2 is four times the power of two (64) at which the
    worst E2 still meets its bound.  The sign rule and the order hold on every set."""
    ref = _reference()
    w1, w2, w2q, n = (0.0, ""), (0.0, ""), (0.0, ""), 0
    for name, x in K.all_host_sets():
        r, s = ref.record(x), ref.S.record(x)
        assert r["sweeps"] == s["sweeps"] and np.array_equal(r["eig"], s["eig"]) and r["off"] == s["off"], name
        D = x.shape[1]
        u1, u2 = Z.check_eigen(name, r)
        q = Z.K2 / 4.0
        bq = r["off"] + q * D * 2.0 ** -53 * r["norm"]
        uq = ref.e2(r) / bq if bq > 0 else 0.0
        w1, w2, w2q, n = max(w1, (u1, name)), max(w2, (u2, name)), max(w2q, (uq, name)), n + 1
    assert n == len(K.DIMS) * len(K.ROWS) * len(K.VARIANTS) + len(K.PADDED) * len(K.PADDED_ROWS)
    print(f"worst E1 {w1[0]:.3f} of the bound at K1 = {Z.K1} ({w1[1]}); worst E2 {w2[0]:.3f} of the bound at K2 = {Z.K2}, {w2q[0]:.3f} at "
          f"K2 / 4 ({w2[1]})")
    assert Z.K1 == 4.0 and Z.K2 == 256.0
    assert w1[0] <= 0.25 < 2.0 * w1[0], w1                    # K1 / 2 would leave the worst case above 1/4
    assert w2q[0] <= 1.0 < w2q[0] * 2.0, w2q                  # 64 holds the restatement, with less than a factor of 2 to spare
    assert w2[0] <= 1.0 / 3.0, w2


def test_the_restatement_angles_agree_with_scipy():
    """subspace_record on random orthonormal pairs, on the planted rotations of the GPU file and on the exact cases."""
    ref = _reference()
    rng = np.random.default_rng(7)
    for D, ka, kb in ((2, 1, 1), (3, 2, 1), (7, 4, 3), (12, 3, 3), (21, 21, 5), (32, 16, 16), (32, 32, 32)):
        Va, Vb = np.linalg.qr(rng.standard_normal((D, D)))[0], np.linalg.qr(rng.standard_normal((D, D)))[0]
        r = ref.subspace_record(Va, Vb, ka, kb)
        want = Z.scipy_sin2(Va, Vb, ka, kb)
        bound = Z.angle_bound(D, r["off"])
        assert np.max(np.abs(r["sin2"] - want)) <= bound, (D, ka, kb)
        assert abs(r["frob2"] - np.sum(r["sin2"])) <= bound and r["orth"] <= 64 * D * 2.0 ** -53
        assert np.allclose(ref.angles(r["sin2"]), np.sort(np.arcsin(np.sqrt(np.clip(want, 0, 1)))), atol=1e-7)
    for D in Z.ANGLE_DIMS:
        for th in Z.THETAS:
            for ka, kb in Z.angle_pairs(D):
                r = ref.subspace_record(np.eye(D), Z.rotated_basis(D, th), ka, kb)
                want = Z.scipy_sin2(np.eye(D), Z.rotated_basis(D, th), ka, kb)
                assert np.max(np.abs(r["sin2"] - want)) <= Z.angle_bound(D, r["off"]), (D, th, ka, kb)
                if (ka, kb) == (1, 1):
                    assert abs(r["sin2"][0] - np.sin(th) ** 2) <= Z.angle_bound(D, r["off"])
    same = ref.subspace_record(np.eye(5), np.eye(5), 3, 3)
    assert same["sin2"].tolist() == [0.0] * 3 and same["frob2"] == 0.0 and same["sweeps"] == 0
    apart = ref.subspace_record(np.eye(5), np.eye(5)[:, ::-1], 2, 2)
    assert apart["sin2"].tolist() == [1.0, 1.0] and apart["frob2"] == 2.0
    v = ref.fix_signs(np.array([[0.5, -0.5], [-0.5, -0.5]]))
    assert v.tolist() == [[0.5, 0.5], [-0.5, 0.5]]            # a tie goes to the lowest row


def test_abi_surface_of_the_eigen_and_angle_calls():
    from vae_training_amd import _lib
    from vae_training_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_cov_eigen_rows") == 8 and _c_args(hdr, "vaek_eigen_event_replicas") == 12 and _c_args(hdr, "vaek_subspace_angles") == 11
    assert [lib.vaek_subspace_record_len(k) for k in (1, 3, 32)] == [5, 7, 36]
    for name in ("cov_eigen_rows", "eigen_event_replicas", "subspace_angles", "cov_eigen_record_len", "subspace_record_len"):
        assert hasattr(Engine, name), name
    n = C.c_int64(7)
    assert lib.vaek_cov_eigen_record_len(None, C.byref(n)) == -1 and n.value == 7
    assert lib.vaek_cov_eigen_rows(None, None, 1, 5, 0, None, 0, None) == -1
    assert b"vaek_cov_eigen_rows" in lib.vaek_last_error()
    ev = _lib.VaekSpectrumEvent()
    ev.struct_size = C.sizeof(_lib.VaekSpectrumEvent)
    assert lib.vaek_eigen_event_replicas(None, None, C.byref(ev), 1, None, 3, 1, 3, 0.0, 5, 6, None) == -1
    assert b"vaek_eigen_event_replicas" in lib.vaek_last_error()
    assert lib.vaek_subspace_angles(None, None, 0, None, 0, 1, 1, 1, None, 0, None) == -1
    assert b"vaek_subspace_angles" in lib.vaek_last_error()


class _EigenStub(_StubEngine):
    """_StubEngine with the eigen calls: records are the spectrum stub's with V = I behind them; the angles call fills sin^2 = 0.25 (p + 1)."""

    def __init__(self, angle_off=0.0, **kw):
        super().__init__(**kw)
        self._angle_off = angle_off
        self.spec_len = self.cov_spectrum_record_len
        self.cov_eigen_record_len = self.spec_len + self.D * self.D
        self.angle_calls = []

    def subspace_record_len(self, kb):
        return kb + 4

    def _fill_eigen(self, out2d):
        self._fill(out2d[:, :self.spec_len])
        out2d[:, self.spec_len:] = torch.eye(self.D, dtype=torch.float64).reshape(-1)

    def eigen_event_replicas(self, params, rows, kind, A, dd, did, pad, var, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, **kw):
        self.calls.append(dict(route="fused", n=params.shape[0], rows=rows, kind=kind, z_steps=z_steps.tolist(), kw=kw))
        assert out.shape == (params.shape[0], 2 * self.cov_eigen_record_len) and out.dtype == torch.float64
        self._fill_eigen(out.view(-1, self.cov_eigen_record_len))

    def cov_eigen_rows(self, x, rows, out):
        self.calls.append(dict(route="rows", n=x.shape[0], rows=rows))
        assert out.shape == (x.shape[0], self.cov_eigen_record_len)
        self._fill_eigen(out)

    def spectrum_event_replicas(self, *a, **kw):
        raise AssertionError("ReplicaSubspace takes the eigen entry points: one device call serves eigenvalues and eigenvectors")

    cov_spectrum_rows = spectrum_event_replicas

    def subspace_angles(self, a, b, ka, kb, out, n=None, a_stride=None, b_stride=None):
        self.angle_calls.append(dict(n=n, ka=ka, kb=kb, a_stride=a_stride, b_stride=b_stride,
                                     offset=(b.data_ptr() - a.data_ptr()) // 8, a_shape=tuple(a.shape)))
        assert out.shape == (n, kb + 4)
        for p in range(n):
            out[p, :kb] = 0.25 * (p + 1)
            out[p, kb:] = torch.tensor([0.25 * (p + 1) * kb, 2.0, self._angle_off, 1e-16], dtype=torch.float64)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "host_route"])
def test_replica_subspace_makes_one_solve_and_one_angles_call(fused):
    from vae_training_amd.trainer import ReplicaSpectrum, ReplicaSubspace
    e = _EigenStub(fused=fused, D=7)
    ms = [_model(e, seed=s) for s in (69, 24, 48)]
    sp = ReplicaSubspace(ms)
    ln = 2 * 49 + 2 * 7 + 4
    assert issubclass(ReplicaSubspace, ReplicaSpectrum) and sp.R == 3 and sp.rows == 1000 and sp.fused == fused
    assert sp.k == 4 and sp.record_len == ln and sp.out.shape == (6, ln)          # sigmoid, dd = 3: k = dd + 1
    for event in range(2):
        stats = sp.event()
        assert len(e.calls) == event + 1 and len(e.angle_calls) == event + 1      # ONE solve call and ONE angles call for R models
        c, a = e.calls[-1], e.angle_calls[-1]
        assert c["route"] == ("fused" if fused else "rows") and c["n"] == (3 if fused else 6) and c["rows"] == 1000
        if fused:
            assert c["kw"]["x_tag"] == 5 and c["kw"]["z_tag"] == 6 and c["z_steps"] == [event + 1] * 3
        else:
            assert [d["tag"] for d in e.batches[-6:]] == [5, 6] * 3 and all(d["step"] == event + 1 for d in e.batches[-6:])
        assert a == dict(n=3, ka=4, kb=4, a_stride=2 * ln, b_stride=2 * ln, offset=ln, a_shape=(3, 2 * ln))   # a = fake, b = real
        for r, (m, st) in enumerate(zip(ms, stats)):
            assert list(st) == KEYS
            assert st[KEYS[0]].tolist() == [200.0 * r + j for j in range(7)] and st[KEYS[1]].tolist() == [200.0 * r + 100 + j for j in range(7)]
            assert np.array_equal(st[KEYS[2]], np.arcsin(np.sqrt(np.full(4, 0.25 * (r + 1)))))
            assert st[KEYS[3]] == np.sqrt(0.25 * (r + 1) * 4)
            assert m._spectrum_draws == event + 1 and m.key == (3, 4) and m.dataset._draws == 5 and m._latent_draws == 9 and m._loglik_draws == 2
            assert len(m.ht_eigen) == len(m.gt_eigen) == len(m.principal_angles) == len(m.subspace_distances) == event + 1
            assert m.vae_losses == [] and m.average_log_likelihoods == []


def test_replica_subspace_k_and_refusals():
    from vae_training_amd.trainer import ReplicaSubspace
    assert [ReplicaSubspace.default_k(kind, 6, 3) for kind in (0, 1, 2)] == [3, 7, 6]
    assert ReplicaSubspace.default_k(0, 3, 6) == 3
    e = _EigenStub(D=7)
    assert ReplicaSubspace([_model(e)]).k == 4 and ReplicaSubspace([_model(e)], k=2).k == 2 and ReplicaSubspace([_model(e)], k=7).k == 7
    assert ReplicaSubspace([_model(e)], rows=37).rows == 37
    for k in (0, 8, -1):
        with pytest.raises(RuntimeError, match=r"k = .*need 1 \.\. data_dim = 7"):
            ReplicaSubspace([_model(e)], k=k)
    with pytest.raises(RuntimeError, match="shape"):
        ReplicaSubspace([_model(e), _model(e, kind=0)])
    with pytest.raises(RuntimeError, match="data_dim <= 32.*data_dim: 33"):
        ReplicaSubspace([_model(_EigenStub(covered=False, D=33))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaSubspace([_model(_EigenStub(world=2))])
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaSubspace([_model(e)], rows=1)
    assert e.calls == [] and e.angle_calls == []
    # a solve above 2^-40 of its norm names the model: the covariance solves as in ReplicaSpectrum, and the angles' solve
    m = _model(_EigenStub(D=7, off=2.0 ** -39))
    with pytest.raises(RuntimeError, match=r"model 0 \(data/stub\).*learnt eigenvalue.*off_F"):
        ReplicaSubspace([m]).event()
    m = _model(_EigenStub(D=7, angle_off=2.0 ** -39))
    with pytest.raises(RuntimeError, match=r"model 0 \(data/stub\).*principal-angle solve.*off_F"):
        ReplicaSubspace([m]).event()
    ReplicaSubspace([_model(_EigenStub(D=7, angle_off=2.0 ** -42))]).event()


def test_the_stats_helper_adds_the_angles_only_when_asked():
    from vae_training_amd.model import GenerativeModel
    e = _EigenStub(D=7)
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0} and e.calls == [] and e.angle_calls == []
    m.subspace = True
    st = GenerativeModel._stats_event(m)
    assert list(st) == ["VAE Loss"] + KEYS[2:] and len(e.calls) == 1 and len(e.angle_calls) == 1        # --subspace alone: no eigenvalue keys
    m.eigenvalues = True
    st = GenerativeModel._stats_event(m)
    assert list(st) == ["VAE Loss"] + KEYS and len(e.calls) == 2 and len(e.angle_calls) == 2             # one device call serves both
    m.subspace_k, m._subspace = 2, None
    assert GenerativeModel._stats_event(m)[KEYS[2]].shape == (2,)


def test_run_py_parses_the_subspace_flag_and_refuses(monkeypatch):
    from vae_training_amd import run
    base = ["sig", "--dataset", "sigmoid"]
    assert run.parse_arguments(base).subspace is None                    # opt-in: without the flag nothing changes
    assert run.parse_arguments(base + ["--subspace", "auto"]).subspace == "auto"
    assert run.parse_arguments(base + ["--subspace", "3"]).subspace == 3
    a = run.parse_arguments(base + ["--subspace", "auto", "--eigenvalues", "--sweep_dataset_seeds", "69,24"])
    assert a.subspace == "auto" and a.eigenvalues is True and a.sweep_dataset_seeds == [69, 24]
    for bad in ("0", "-2", "all", "1.5"):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + ["--subspace", bad])
    ok = _model(_EigenStub(D=7))
    assert run.check_subspace_model(ok, "auto") is None and run.check_subspace_model(ok, 7) == 7 and run.check_subspace_model(ok, 1) == 1
    with pytest.raises(RuntimeError, match=r"--subspace 8 needs .*K in 1 \.\. data_dim.*data_dim: 7"):
        run.check_subspace_model(ok, 8)
    with pytest.raises(RuntimeError, match=r"--subspace needs data_dim <= 32.*data_dim: 33"):
        run.check_subspace_model(_model(_EigenStub(covered=False, D=33)), "auto")
    with pytest.raises(RuntimeError, match=r"--subspace needs .*world 2"):
        run.check_subspace_model(_model(_EigenStub(world=2)), "auto")
    with pytest.raises(RuntimeError, match="--subspace needs"):
        run.check_subspace_model(_model(_EigenStub(), dd=17), "auto")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="--subspace needs .* does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--subspace", "auto"]))
