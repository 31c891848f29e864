"""What an importance-weighted log-likelihood event costs: R models of the first line of sigmoid_vae_padding_expts.sh (D = 7, L = 6, two
decoders, -tdv, batch 100), K samples per row of 1000 rows, R = 1, 3, 64 and K = 1, 64, 1024, evaluated two ways:

    torch   for m in models: the estimator restated with torch ops on the device -- a dataset batch, rows x K x L normals, the
            encoder / decoder products, logsumexp -- what a user of the package would write today (a rows x K x L tensor chain and
            three read-backs PER MODEL)
    fused   trainer.ReplicaLogLik(models, K).event()      one vaek_log_likelihood_replicas call and one device -> host copy for all R

    python tools/time_log_likelihood.py [--replicas 1,3,64] [--samples 1,64,1024] [--repeats 9] [--rows 1000]

Per (R, K): one warm-up event of each leg, then `repeats` timed events of each, the legs ALTERNATED repeat by repeat.  A timed event
starts after a device synchronise and ends in one, and includes turning every value into a Python float, so both legs deliver the
same thing: R dicts of three floats on the host.  Reported: min / median / max of the wall time per event in ms, and the median per
model in us.  The torch leg takes its rows from `dataset.get_batch`, which advances the models' dataset draw counters (harmless
here: the models are the tool's own and are never trained); the fused leg advances only its own counter.  The legs draw different
normals (torch's generator against the library's Philox streams): the values are close, not equal."""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3,64")
ap.add_argument("--samples", default="1,64,1024")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--rows", type=int, default=1000)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import ReplicaLogLik  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402


def model(root, seed):
    args = parse_arguments([f"m{seed}", "--dataset", "sigmoid", "--padding_dim", "3", "-dd", "3"])
    d = os.path.join(root, f"m{seed}")
    os.makedirs(d, exist_ok=True)
    m = VAEModel(dirname=d, num_batches=16, num_epochs=1, batch_size=100, learning_rate=1e-4, layer_sizes="", encoder_layer_sizes="",
                 state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=get_dataset("sigmoid", seed, 3, 100, args),
                 latent_dimension=6, tunable_decoder_var=True, dataset_name="sigmoid", fast_loop=True)
    m.print_batch_size = opt.rows
    return m


def torch_event(ms, K):
    """The estimator of include/vaek.h (vaek_log_likelihood_replicas) restated with torch ops, model by model."""
    out = []
    for m in ms:
        eng = m.model.module.engine(m.batch_size, m.optimizer.global_batch)
        p = eng.views(m.model.flat)
        x = m.dataset.get_batch(opt.rows)
        D, L = x.shape[1], p["epsilon_p"].numel()
        eps = p["epsilon"] * m.epsilon
        lv = p["epsilon_p"]
        mu = x @ p["Encoder"]["FC0"]["kernel"] + p["Encoder"]["FC0"]["bias"]
        xi = torch.randn(opt.rows, K, L, device=x.device)
        z = mu[:, None, :] + torch.exp(0.5 * lv) * xi
        y = z @ p["Decoder"]["FC0"]["kernel"] + p["Decoder"]["FC0"]["bias"]
        y = y + torch.sigmoid(z @ p["SigDecoder"]["FC0"]["kernel"] + p["SigDecoder"]["FC0"]["bias"])
        rsq = (y - x[:, None, :]).square().sum(-1)
        lw = -0.5 * (rsq * torch.exp(-eps) + D * (eps + math.log(2 * math.pi))) + 0.5 * (xi.square() - z.square() + lv).sum(-1)
        lse = torch.logsumexp(lw, dim=1)
        ess = torch.exp(2 * lse - torch.logsumexp(2 * lw, dim=1)) / K
        out.append({"Average Log Likelihood": (lse - math.log(K)).mean(), "ELBO estimate": lw.mean(), "Effective Sample Size": ess.mean()})
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    floats = [{k: float(v) for k, v in st.items()} for st in out]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, floats


with tempfile.TemporaryDirectory() as root:
    models = [model(root, 1000 + r) for r in range(max(int(s) for s in opt.replicas.split(",")))]
    for R in [int(s) for s in opt.replicas.split(",")]:
        ms = models[:R]
        for K in [int(s) for s in opt.samples.split(",")]:
            fused = ReplicaLogLik(ms, K, rows=opt.rows)
            legs = [("torch", lambda: torch_event(ms, K)), ("fused", fused.event)]
            secs = {name: [] for name, _ in legs}
            for _, fn in legs:
                timed(fn)
            last = {}
            for _ in range(max(opt.repeats, 9)):
                for name, fn in legs:
                    s, last[name] = timed(fn)
                    secs[name].append(s)
            for name, _ in legs:
                ms_ = [s * 1e3 for s in secs[name]]
                print(f"R={R:4d} K={K:5d} rows={opt.rows} {name:5s} ms/event min/median/max {min(ms_):9.3f} {statistics.median(ms_):9.3f} "
                      f"{max(ms_):9.3f}   median us/model {statistics.median(ms_) * 1e3 / R:9.1f}", flush=True)
            print(f"R={R:4d} K={K:5d} last event, model 0: torch {({k: round(v, 4) for k, v in last['torch'][0].items()})} "
                  f"fused {({k: round(v, 4) for k, v in last['fused'][0].items()})}", flush=True)
            for m in ms:                             # the evaluation's own list: a timing tool keeps none
                m.average_log_likelihoods.clear()
