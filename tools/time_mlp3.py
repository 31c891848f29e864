"""us/step of trainer.GraphLoop (the hipGraph loop `run.py --fast_loop` runs: vaek_train_step_gen captured 200 steps at a time)
on the shapes of sphere_vae_padding_expts.sh -- the three-hidden-layer models csrc/fused_mlp3.hip covers -- plus 256|256|256.

    python tools/time_mlp3.py [--root TREE] [--label NAME] [--batches 100,128,256,512] [--steps 20000] [--repeats 5] [--force_generic]

--root: the source tree to import vae_training_amd from (default: the tree this file is in).  The file uses only interfaces older
commits have too, so the SAME file times a build of the parent commit kept in another directory (--root THAT_DIR): the code under
test is never its own baseline.  Alternate the two trees in one sitting.  Per (shape, batch): 202 warm-up steps (the two eager
steps of the capture + one replay), then `repeats` timed runs of `steps` steps each; min / median / max of the repeats."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default=None)
ap.add_argument("--batches", default="100,128,256,512")
ap.add_argument("--steps", type=int, default=20000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--force_generic", action="store_true", help="this tree's layer-by-layer kernels (a cross-check, not a baseline)")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))

import torch  # noqa: E402
from vae_training_amd.run import get_dataset, parse_arguments  # noqa: E402
from vae_training_amd.trainer import GraphLoop  # noqa: E402
from vae_training_amd.vae import VAEModel  # noqa: E402

SHAPES = [(3, 3, 6, "200|200|200"), (3, 13, 8, "200|200|200"), (5, 16, 16, "200|200|200"), (5, 5, 10, "200|200|200"),
          (7, 7, 13, "200|200|200"), (3, 3, 6, "256|256|256")]          # (dd, pad, L, hidden): the script's five rows, one wider


def build(dd, pad, L, hidden, B):
    args = parse_arguments(["t", "--dataset", "sphere", "--padding_dim", str(pad), "-dd", str(dd)])
    ds = get_dataset("sphere", args.dataset_seed, pad, B, args)
    return VAEModel(dirname=tempfile.mkdtemp(), num_batches=10, num_epochs=1, batch_size=B, learning_rate=args.learning_rate,
                    layer_sizes=hidden, encoder_layer_sizes=hidden, state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False,
                    dataset=ds, latent_dimension=L, tunable_decoder_var=True, dataset_name="sphere", fast_loop=True,
                    force_generic=opt.force_generic)


label = opt.label or os.path.basename(os.path.abspath(opt.root))
for B in [int(b) for b in opt.batches.split(",")]:
    for dd, pad, L, hidden in SHAPES:
        m = build(dd, pad, L, hidden, B)
        loop = GraphLoop(m, seed=9)
        loop.run(loop.G + 2)
        torch.cuda.synchronize()
        us = []
        for _ in range(opt.repeats):
            t0 = time.perf_counter()
            loop.run(opt.steps)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / opt.steps * 1e6)
        last = float(loop.losses()[-1])
        print(f"tree={label:8s} path={getattr(loop.eng, 'step_path', 'n/a'):7s} dd={dd} pad={pad:2d} L={L:2d} hidden={hidden} B={B:3d}  "
              f"us/step min/median/max {min(us):7.2f} {statistics.median(us):7.2f} {max(us):7.2f}   last loss {last:.4f}", flush=True)
