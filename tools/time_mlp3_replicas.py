"""What R three-hidden-layer MLP VAEs per step cost: trainer.ReplicaGraphLoop (every step ONE vaek_train_step_gen_replicas call,
two launches with gridDim.y = R) on the five shapes of sphere_vae_padding_expts.sh at the reference's batch size, R = 1, 4, 16, 36,
72, against the way such a sweep runs without it -- R trainer.GraphLoop runs one after another on the solo kernels, which the
replica form leaves instruction for instruction what they were, so the same build is its own A/B:

    python tools/time_mlp3_replicas.py [--shapes 0,1,2,3,4] [--batch 100] [--steps 20000] [--repeats 5] [--replicas 1,4,16,36,72]
                                       [--baseline_runs N] [--limit SECONDS] | tee profiles/mlp3_replicas.txt

The driver starts one child process per shape under its own `timeout -k 10 LIMIT` and stops at the first child that does not end
well.  Per shape and R, in the child: a warm-up of both legs (capture + one replay), then `repeats` timed runs of `steps` steps of
each leg, the legs ALTERNATED repeat by repeat, every timed run ending in a device synchronise.  Reported, min / median / max over
the repeats, in us per step of the loop (one step = one step of EVERY model of the leg):

    replicas     ReplicaGraphLoop over R models
    sequential   the sum over R GraphLoop(pipeline=True, moments=False, resident=False) runs of `steps` steps each

--baseline_runs N (default: R, the literal protocol) times only N of the R sequential runs and scales their sum by R / N: the runs
are the same launches on the same shapes, so their cost does not depend on which model of the sweep they train; the output says
which was done.  After the timing, 200 eager steps of each leg under the library's event profiler give the per-launch split (mean
us per launch of each label), so the growth of launch 2 with R is visible."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="0,1,2,3,4")
ap.add_argument("--batch", type=int, default=100)
ap.add_argument("--steps", type=int, default=20000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--replicas", default="1,4,16,36,72")
ap.add_argument("--baseline_runs", type=int, default=0, help="sequential GraphLoop runs actually timed per R (0: all R of them)")
ap.add_argument("--limit", type=int, default=3600, help="seconds one shape's child process may take")
ap.add_argument("--worker", action="store_true", help="(internal) time the one shape of --shapes in this process")
opt = ap.parse_args()
HERE = os.path.abspath(__file__)
SHAPES = [(3, 3, 6), (3, 13, 8), (5, 16, 16), (5, 5, 10), (7, 7, 13)]          # (dd, pad, L) of the script's five rows
HIDDEN = "200|200|200"

if not opt.worker:
    for i in [int(s) for s in opt.shapes.split(",")]:
        cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, HERE, "--worker", "--shapes", str(i), "--batch", str(opt.batch), "--steps",
               str(opt.steps), "--repeats", str(opt.repeats), "--replicas", opt.replicas, "--baseline_runs", str(opt.baseline_runs)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"shape {i}: the child ended with status {rc}; nothing more is started", flush=True)
            raise SystemExit(rc)
    raise SystemExit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import GraphLoop, ReplicaGraphLoop  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402


def build(dd, pad, L, seed):
    args = parse_arguments(["t", "--dataset", "sphere", "--padding_dim", str(pad), "-dd", str(dd)])
    ds = get_dataset("sphere", seed, pad, opt.batch, args)
    return VAEModel(dirname=tempfile.mkdtemp(), num_batches=10, num_epochs=1, batch_size=opt.batch, learning_rate=args.learning_rate,
                    layer_sizes=HIDDEN, encoder_layer_sizes=HIDDEN, state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=L, tunable_decoder_var=True, dataset_name="sphere", fast_loop=True)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fmt(xs):
    return f"{min(xs):8.2f} {statistics.median(xs):8.2f} {max(xs):8.2f}"


def split(eng, fn):
    """mean us per launch, by label, of the launches fn makes"""
    torch.cuda.synchronize()
    eng.profile_begin(4096)
    fn()
    torch.cuda.synchronize()
    return {k: 1e3 * v["total_ms"] / v["count"] for k, v in sorted(eng.profile_report().items())}


dd, pad, L = SHAPES[int(opt.shapes)]
counts = [int(s) for s in opt.replicas.split(",")]
models = [build(dd, pad, L, 1000 + r) for r in range(max(counts))]
tag = f"dd={dd} pad={pad:2d} L={L:2d} hidden={HIDDEN} B={opt.batch}"
for R in counts:
    nb = min(R, opt.baseline_runs) if opt.baseline_runs > 0 else R
    base_models = [build(dd, pad, L, 5000 + r) for r in range(nb)]
    base = [GraphLoop(m, pipeline=True, moments=False, resident=False, loss_capacity=1 << 16) for m in base_models]
    rep = ReplicaGraphLoop(models[:R], loss_capacity=1 << 16)
    assert rep.eng.step_path == "mlp3" and all(b.eng.step_path == "mlp3" and b.pipeline for b in base)

    def sequential():
        for b in base:
            b.run(opt.steps)

    def replicas():
        rep.run(opt.steps)

    for b in base:
        b.run(2 * b.G + 2)
    rep.run(2 * rep.G + 1)
    torch.cuda.synchronize()
    assert rep.graph is not None and all(b.graph is not None for b in base)
    secs = {"sequential": [], "replicas": []}
    for _ in range(opt.repeats):
        secs["sequential"].append(timed(sequential) * R / nb)
        secs["replicas"].append(timed(replicas))
    us = {k: [s / opt.steps * 1e6 for s in v] for k, v in secs.items()}
    how = f"all {R} runs timed" if nb == R else f"{nb} of the {R} runs timed, their sum scaled by {R}/{nb}"
    print(f"{tag} R={R:3d} sequential us/step min/median/max {fmt(us['sequential'])}   ({how})", flush=True)
    print(f"{tag} R={R:3d} replicas   us/step min/median/max {fmt(us['replicas'])}   sequential min / replicas max "
          f"{min(us['sequential']) / max(us['replicas']):.2f}x", flush=True)
    eager = ReplicaGraphLoop(models[:R], steps_per_graph=1 << 30, loss_capacity=1 << 16)          # never captures: every step is a call
    sp = split(eager.eng, lambda: eager.run(200))
    solo = GraphLoop(base_models[0], steps_per_graph=1 << 30, pipeline=True, moments=False, resident=False, loss_capacity=1 << 16)
    ss = split(solo.eng, lambda: solo.run(200))
    print(f"{tag} R={R:3d} per launch, us: " + ", ".join(f"{k} {v:.1f}" for k, v in sp.items()) + " | solo: "
          + ", ".join(f"{k} {v:.1f}" for k, v in ss.items()), flush=True)
    finite = all(bool(torch.isfinite(m.model.flat).all()) for m in models[:R] + base_models)
    print(f"{tag} R={R:3d} parameters finite: {finite}", flush=True)
    del base, rep, eager, solo
