"""us/step of trainer.GraphLoop on the small-batch linear VAEs the moment form does not cover: the six distinct shapes of
sigmoid_vae_padding_expts.sh (two decoders) and one one-decoder model with L + 2 D + 1 > 64 (D = 28, L = 24), at the reference's
batch size.  Two loops of the SAME build, alternated repeat by repeat in one sitting:

    resident=False   the hipGraph loop (vaek_train_step_gen, one launch per step, 200 steps per graph)
    resident=True    vaek_train_loop_gen (csrc/linear_resident.hip: the steps as a loop inside one workgroup)

    python tools/time_resident.py [--shapes 0,1,2,3,4,5,6] [--batch 100] [--steps 20000] [--repeats 5]

The hipGraph loop is unchanged by the resident kernel's existence, so the same commit is its own A/B here.  Per shape: 202 warm-up
steps on each loop (the two eager steps of the capture + one replay), then `repeats` timed runs of `steps` steps on each,
alternating; min / median / max of the repeats.  The last line says whether the gate of trainer.RESIDENT_DEFAULT holds on the shapes
timed: the resident loop's MAXIMUM below the hipGraph loop's MINIMUM on every one of them."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="0,1,2,3,4,5,6")
ap.add_argument("--batch", type=int, default=100)
ap.add_argument("--steps", type=int, default=20000)
ap.add_argument("--repeats", type=int, default=5)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import GraphLoop  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402

# (dataset, dd, pad, L): the script's six rows (D = dd + pad + 1), then the one-decoder shape without a moment form (D = dd + pad)
SHAPES = [("sigmoid", 3, 3, 6), ("sigmoid", 3, 13, 8), ("sigmoid", 5, 16, 16), ("sigmoid", 5, 5, 10), ("sigmoid", 7, 7, 13),
          ("sigmoid", 7, 20, 24), ("linear_gaussian", 7, 21, 24)]


def build(name, dd, pad, L, B):
    args = parse_arguments(["t", "--dataset", name, "--padding_dim", str(pad), "-dd", str(dd)])
    ds = get_dataset(name, args.dataset_seed, pad, B, args)
    return VAEModel(dirname=tempfile.mkdtemp(), num_batches=10, num_epochs=1, batch_size=B, learning_rate=args.learning_rate,
                    layer_sizes="", encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=L, tunable_decoder_var=True, dataset_name=name, fast_loop=True)


gate = True
for i in [int(s) for s in opt.shapes.split(",")]:
    name, dd, pad, L = SHAPES[i]
    loops = {res: GraphLoop(build(name, dd, pad, L, opt.batch), seed=9, resident=res) for res in (False, True)}
    us = {False: [], True: []}
    for lp in loops.values():
        lp.run(lp.G + 2)
    torch.cuda.synchronize()
    for _ in range(opt.repeats):
        for res, lp in loops.items():
            t0 = time.perf_counter()
            lp.run(opt.steps)
            torch.cuda.synchronize()
            us[res].append((time.perf_counter() - t0) / opt.steps * 1e6)
    D = loops[True].eng.D
    for res, lp in loops.items():
        u = us[res]
        print(f"{name:15s} D={D:2d} L={L:2d} B={opt.batch:3d}  {'resident' if res else 'hipGraph':8s}  us/step min/median/max "
              f"{min(u):7.2f} {statistics.median(u):7.2f} {max(u):7.2f}   last loss {float(lp.losses()[-1]):.4f}", flush=True)
    gate = gate and max(us[True]) < min(us[False])
print(f"gate (resident max < hipGraph min on every shape timed): {'holds' if gate else 'FAILS'}", flush=True)
