"""What an exact log-likelihood event costs: R linear_gaussian models (D = 12, L = 20, one decoder, -tdv, batch 100), 1000 rows,
R = 1, 3, 64, evaluated two ways:

    host    for m in models: what a user writes today -- read the parameters back, vaek_make_batch under the event's (seed, step,
            tag), read the rows back, numpy.linalg.eigh of K^T K + the closed forms of include/vaek.h in NumPy float64, model by model
    fused   trainer.ReplicaExactLogLik(models).event()      one vaek_exact_log_likelihood_replicas launch and one device -> host copy

    python tools/time_exact_log_likelihood.py [--replicas 1,3,64] [--repeats 9] [--rows 1000] > profiles/exact_log_likelihood.txt

Per R: one warm-up event of each leg, then `repeats` timed events of each, the legs ALTERNATED repeat by repeat.  A timed event starts
after a device synchronise and ends in one and delivers R dicts of Python floats on the host.  Reported: min / median / max of the
wall time per event in ms, the median per model in us, the device time of the fused launch (the library's profile of 9 more calls)
and, on the warm-up draws -- the same seed, step and tag in both legs, so the same rows -- the largest difference between the legs.
No time or ratio is a pass condition."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3,64")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--rows", type=int, default=1000)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import ReplicaExactLogLik  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402

KEYS = ReplicaExactLogLik.KEYS[:3]


def model(root, seed):
    args = parse_arguments([f"m{seed}", "--dataset", "linear_gaussian", "--padding_dim", "9", "-dd", "3", "-ds", str(seed)])
    d = os.path.join(root, f"m{seed}")
    os.makedirs(d, exist_ok=True)
    m = VAEModel(dirname=d, num_batches=16, num_epochs=1, batch_size=100, learning_rate=1e-3, layer_sizes="", encoder_layer_sizes="",
                 state_dict=None, data_fn=None, epsilon=-1.0, tqdm=False, dataset=get_dataset("linear_gaussian", seed, 9, 100, args),
                 latent_dimension=20, tunable_decoder_var=True, dataset_name="linear_gaussian")
    m.print_batch_size = opt.rows
    return m


def host_event(ms, step):
    """The closed forms with today's entry points, model by model: two read-backs and NumPy per model."""
    out = []
    for m in ms:
        eng = m.model.module.engine(m.batch_size, m.optimizer.global_batch)
        D, L = eng.D, eng.L
        flat = m.model.flat.cpu().numpy()
        kind, A, dd, did, pad, var = m.dataset.device_spec()
        x = eng.make_batch(kind, A, dd, did, pad, var, opt.rows, m.dataset.key[0] ^ m.dataset.key[1], step=step, tag=3, want_z=False)[0]
        x = x.cpu().numpy().astype(np.float64)
        o = 0
        e = flat[o:o + D * L].reshape(D, L).astype(np.float64); o += D * L
        be = flat[o:o + L].astype(np.float64); o += L
        k = flat[o:o + L * D].reshape(L, D).astype(np.float64); o += L * D
        bd = flat[o:o + D].astype(np.float64); o += D
        lv = flat[o:o + L].astype(np.float64); o += L
        eps = float(np.float32(flat[o]) * np.float32(m.epsilon))
        lam, v = np.linalg.eigh(k.T @ k)
        s = np.maximum(lam, 0.0) + np.exp(eps)
        y = (x - bd) @ v
        logp = -0.5 * (np.sum(y * y / s, axis=1) + np.sum(np.log(s)) + D * np.log(2 * np.pi))
        mu = x @ e + be
        r = mu @ k + bd - x
        t = np.sum(np.exp(lv) * np.sum(k * k, axis=1))
        elbo = -0.5 * (np.exp(-eps) * (np.sum(r * r, axis=1) + t) + D * (eps + np.log(2 * np.pi))) - 0.5 * (np.sum(np.exp(lv) - 1 - lv) + np.sum(mu * mu, axis=1))
        out.append(dict(zip(KEYS, (logp.mean(), elbo.mean(), (logp - elbo).mean()))))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    floats = [{k: float(st[k]) for k in KEYS} for st in out]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, floats


with tempfile.TemporaryDirectory() as root:
    models = [model(root, 1000 + r) for r in range(max(int(s) for s in opt.replicas.split(",")))]
    for R in [int(s) for s in opt.replicas.split(",")]:
        ms = models[:R]
        fused = ReplicaExactLogLik(ms, rows=opt.rows)
        _, a = timed(lambda: host_event(ms, 1))                           # the warm-up of each leg, on the same draws
        _, b = timed(lambda: fused.event(step=1))
        diff = max(abs(a[r][k] - b[r][k]) for r in range(R) for k in KEYS)
        legs = [("host", lambda: host_event(ms, 2)), ("fused", fused.event)]
        secs = {name: [] for name, _ in legs}
        for _ in range(max(opt.repeats, 9)):
            for name, fn in legs:
                s, _ = timed(fn)
                secs[name].append(s)
        for name, _ in legs:
            ms_ = [s * 1e3 for s in secs[name]]
            print(f"R={R:4d} rows={opt.rows} {name:5s} ms/event min/median/max {min(ms_):9.3f} {statistics.median(ms_):9.3f} {max(ms_):9.3f}   "
                  f"median us/model {statistics.median(ms_) * 1e3 / R:9.1f}", flush=True)
        fused.eng.profile_begin(64)
        for _ in range(9):
            fused.event()
        torch.cuda.synchronize()
        rep = fused.eng.profile_report()
        dev = {k: round(v["total_ms"] / v["count"] * 1e3, 1) for k, v in rep.items()}
        print(f"R={R:4d} rows={opt.rows} device us per launch {dev}; warm-up draws, model 0: host {a[0]} fused {b[0]}; largest |host - fused| "
              f"over models and keys {diff:.3e}", flush=True)
