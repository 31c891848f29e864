"""What a subspace event of a sweep costs: R = 1, 3, 15 models, 1000 generated and 1000 real rows each, evaluated two ways:

    today   per model vaek_make_batch (rows), vaek_make_batch (latents), vaek_forward(sampling), a read-back of 2 x rows x D floats,
            numpy.cov and numpy.linalg.eigh of both sides and scipy.linalg.subspace_angles on the host -- the event assembled from
            entry points that existed before the eigenvector calls, under the same seeds, steps and tags
    new     trainer.ReplicaSubspace(models).event(): linear models (line 1 of sigmoid_vae_padding_expts.sh: D = 7, L = 6, two
            decoders, k = 4) through ONE vaek_eigen_event_replicas launch and ONE vaek_subspace_angles launch; mlp3 models (line 1 of
            sphere_vae_padding_expts.sh: 200|200|200, D = 6, L = 6, k = 3) through the host route (make_batch + forward per model,
            ONE vaek_cov_eigen_rows call, ONE vaek_subspace_angles call)

    python tools/time_subspace.py [--replicas 1,3,15] [--repeats 9] [--rows 1000]

The discipline of tools/time_cov_spectrum.py: per R one warm-up event of each leg, then `repeats` timed events of each, the legs
ALTERNATED repeat by repeat; a timed event starts after a device synchronise and ends in one and delivers the same thing on the host
(per model two float64 arrays of D eigenvalues, the k principal angles and their distance).  Reported: min / median / max of the
wall time per event in ms, the median per model in us, and the device time of the new kernels from the library's profile records.
No time is a pass condition."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3,15")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--rows", type=int, default=1000)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.linalg import subspace_angles  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import ReplicaSubspace  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402

FAMILIES = {"linear": ("sigmoid", "", True), "mlp3": ("sphere", "200|200|200", False)}
NEW_LABELS = ("eigen_event_replicas", "cov_eigen_rows", "subspace_angles")


def model(root, family, seed):
    dataset, layers, _ = FAMILIES[family]
    args = parse_arguments([f"{family}{seed}", "--dataset", dataset, "--padding_dim", "3", "-dd", "3"])
    d = os.path.join(root, f"{family}{seed}")
    os.makedirs(d, exist_ok=True)
    m = VAEModel(dirname=d, num_batches=16, num_epochs=1, batch_size=100, learning_rate=1e-4, layer_sizes=layers, encoder_layer_sizes=layers,
                 state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=get_dataset(dataset, seed, 3, 100, args),
                 latent_dimension=6, tunable_decoder_var=True, dataset_name=dataset, fast_loop=True)
    m.print_batch_size = opt.rows
    return m


def today(ms, sp):
    """The same event from vaek_make_batch, vaek_forward, a read-back, LAPACK and scipy, per model."""
    out, k = [], sp.k
    for r, m in enumerate(ms):
        eng = m.model.module.engine(sp.rows)
        ds = m.dataset
        seed, step = ds.key[0] ^ ds.key[1], getattr(m, "_spectrum_draws", 0) + 1
        Ar = None if sp.A is None else sp.A[r]
        x, _, _ = eng.make_batch(sp.kind, Ar, sp.dd, sp.did, sp.pad, sp.var, sp.rows, seed, step=step, tag=sp.X_TAG, want_z=False)
        _, z1, z2 = eng.make_batch(sp.kind, Ar, sp.dd, sp.did, sp.pad, sp.var, sp.rows, seed, step=step, tag=sp.Z_TAG, want_x=False)
        fake, _ = eng.forward(m.model.flat, None, z1, z2, sampling=True, eps=float(torch.as_tensor(m.current_epsilon).reshape(-1)[0]), want_mu=False)
        both = torch.stack([fake, x]).cpu().numpy().astype(np.float64)                # the read-back of 2 x rows x D floats
        st, spans = {}, []
        for key, b in zip(sp.KEYS, both):
            lam, vec = np.linalg.eigh(np.cov(b.T, ddof=1))
            st[key] = lam
            spans.append(vec[:, -k:])
        th = np.sort(subspace_angles(spans[0], spans[1]))
        st[sp.ANGLES], st[sp.DISTANCE] = th, float(np.sqrt(np.sum(np.sin(th) ** 2)))
        out.append(st)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


with tempfile.TemporaryDirectory() as root:
    sizes = [int(s) for s in opt.replicas.split(",")]
    for family in FAMILIES:
        models = [model(root, family, 1000 + r) for r in range(max(sizes))]
        for R in sizes:
            ms = models[:R]
            sp = ReplicaSubspace(ms, rows=opt.rows)
            assert sp.fused == FAMILIES[family][2], (family, sp.fused)
            legs = [("today", lambda: today(ms, sp)), ("new", sp.event)]
            secs = {name: [] for name, _ in legs}
            last = {}
            for name, fn in legs:
                _, last[name] = timed(fn)
            # the warm-up pair ran under the same seed, step and tag: the two legs must agree (LAPACK and scipy against the device)
            err = max(float(np.max(np.abs(a[k] - b[k]))) for a, b in zip(last["today"], last["new"]) for k in sp.KEYS)
            aerr = max(float(np.max(np.abs(np.sin(a[sp.ANGLES]) - np.sin(b[sp.ANGLES])))) for a, b in zip(last["today"], last["new"]))
            for _ in range(max(opt.repeats, 9)):
                for name, fn in legs:
                    s, _ = timed(fn)
                    secs[name].append(s)
            for name, _ in legs:
                ms_ = [s * 1e3 for s in secs[name]]
                print(f"{family:6s} R={R:3d} rows={opt.rows} k={sp.k} {name:5s} ms/event min/median/max {min(ms_):9.3f} {statistics.median(ms_):9.3f} "
                      f"{max(ms_):9.3f}   median us/model {statistics.median(ms_) * 1e3 / R:9.1f}", flush=True)
            sp.eng.profile_begin(64)
            sp.event()
            torch.cuda.synchronize()
            rep = sp.eng.profile_report()
            print(f"{family:6s} R={R:3d} today against new on the warm-up draws: max |d lambda| {err:.2e}, max |d sin theta| {aerr:.2e}; device "
                  f"time of the new kernels: { {k: v for k, v in rep.items() if k in NEW_LABELS} }", flush=True)
