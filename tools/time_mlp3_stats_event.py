"""What a stats event of the mlp3 sweep costs: R models of the first line of sphere_vae_padding_expts.sh (D = 6, L = 6, 200|200|200 both
ways, -tdv, batch 100, 1000 rows per event), R = 1, 3, 15 (the script trains 15), evaluated the two ways
`run.py --sweep_dataset_seeds` can evaluate them:

    host    for m in models: m.compute_stats()         two vaek_make_batch launches, a layer-by-layer vaek_forward(sampling) and
                                                       vaek_loss_eval, score_batch and the printed stats' read-backs PER MODEL (the code
                                                       of the parent commit, unchanged: the same build is its own A/B)
    fused   trainer.ReplicaStatsMlp3(models).event()   one vaek_mlp3_stats_event_replicas call (two launches) and one device -> host copy

    python tools/time_mlp3_stats_event.py [--replicas 1,3,15] [--repeats 9] [--rows 1000]
    python tools/time_mlp3_stats_event.py --device-time       # the two launches' device time, from a kernel trace of this script's own

Per R: one warm-up event of each leg, then `repeats` timed events of each, the legs ALTERNATED repeat by repeat.  A timed event
starts after a device synchronise and ends in one, and includes turning every stat into a Python float (what write_stats does with
them), so both legs deliver the same thing: R dicts of floats on the host.  Reported: min / median / max of the wall time per event
in ms, and the median per model in us.  Both legs advance the same host RNG state, so every event evaluates fresh draws.

--device-time starts ONE child process, `rocprofv3 --kernel-trace --stats -- python <this file> --fused-only`, which runs the fused
leg alone (a warm-up and `repeats` events per R), and prints the trace's rows for mlp3_stats_tile_kernel and
mlp3_stats_finalize_kernel: calls, total and average ns over every R together."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3,15")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--device-time", action="store_true")
ap.add_argument("--fused-only", action="store_true")
opt = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if opt.device_time:
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--fused-only", "--replicas", opt.replicas, "--repeats", str(opt.repeats), "--rows", str(opt.rows)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
        if r.returncode != 0:
            sys.exit(f"the traced child failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            sys.exit("no kernel_stats.csv in the trace's output: " + repr(glob.glob(os.path.join(out, "**", "*"), recursive=True)))
        print(f"# device time of the fused leg alone ({opt.replicas} models, a warm-up and {max(opt.repeats, 9)} events each), one kernel trace")
        for row in csv.DictReader(open(files[0])):
            if "mlp3_stats" in row.get("Name", ""):
                name = row["Name"].split("(")[0]
                print(f"{name:45s} " + "  ".join(f"{k} {v}" for k, v in row.items() if k not in ("Name", "Percentage")))
    sys.exit(0)

import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import ReplicaStatsMlp3  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402


def model(root, seed):
    args = parse_arguments([f"m{seed}", "--dataset", "sphere", "--padding_dim", "3", "-dd", "3"])
    d = os.path.join(root, f"m{seed}")
    os.makedirs(d, exist_ok=True)
    m = VAEModel(dirname=d, num_batches=16, num_epochs=1, batch_size=100, learning_rate=1e-4, layer_sizes="200|200|200",
                 encoder_layer_sizes="200|200|200", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False,
                 dataset=get_dataset("sphere", seed, 3, 100, args), latent_dimension=6, tunable_decoder_var=True, dataset_name="sphere",
                 fast_loop=True)
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
        fused = ReplicaStatsMlp3(ms, rows=opt.rows)
        legs = [("host", lambda: [m.compute_stats() for m in ms]), ("fused", fused.event)]
        if opt.fused_only:
            legs = legs[1:]
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
        print(f"R={R:4d} last event, model 0: " + " ".join(f"{name} {({k: round(v, 4) for k, v in last[name][0].items()})}" for name, _ in legs),
              flush=True)
