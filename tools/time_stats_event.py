"""What a stats event of a sweep costs: R models of the first line of sigmoid_vae_padding_expts.sh (D = 7, L = 6, two decoders, -tdv,
batch 100, 1000 rows per event), R = 1, 3, 64, 256, evaluated the two ways run.py --sweep_dataset_seeds can evaluate them:

    host    for m in models: m.compute_stats()      one vaek_make_batch pair, vaek_forward, vaek_loss_eval, score_batch and the
                                                    printed stats' read-backs PER MODEL (the code of the parent commit, unchanged)
    fused   trainer.ReplicaStats(models).event()    one vaek_stats_event_replicas launch and one device -> host copy for all R

    python tools/time_stats_event.py [--replicas 1,3,64,256] [--repeats 9] [--rows 1000]

Per R: one warm-up event of each leg, then `repeats` timed events of each, the legs ALTERNATED repeat by repeat.  A timed event
starts after a device synchronise and ends in one, and includes turning every stat into a Python float (what write_stats does with
them), so both legs deliver the same thing: R dicts of floats on the host.  Reported: min / median / max of the wall time per event
in ms, and the median per model in us.  Both legs advance the same host RNG state, so every event evaluates fresh draws."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3,64,256")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--rows", type=int, default=1000)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import ReplicaStats  # noqa: E402
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
        fused = ReplicaStats(ms, rows=opt.rows)
        legs = [("host", lambda: [m.compute_stats() for m in ms]), ("fused", fused.event)]
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
            print(f"R={R:4d} rows={opt.rows} {name:5s} ms/event min/median/max {min(ms_):9.3f} {statistics.median(ms_):9.3f} {max(ms_):9.3f}   "
                  f"median us/model {statistics.median(ms_) * 1e3 / R:9.1f}", flush=True)
        # the two legs evaluate different draws (each event advances the RNG state): the stats are close, not equal
        print(f"R={R:4d} last event, model 0: host {({k: round(v, 4) for k, v in last['host'][0].items()})} "
              f"fused {({k: round(v, 4) for k, v in last['fused'][0].items()})}", flush=True)
