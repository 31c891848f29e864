"""us/step of the resident loop with and without its trajectory ring (vaek_train_loop_gen / vaek_train_loop_gen_traj,
csrc/linear_resident.hip) on the six distinct shapes of sigmoid_vae_padding_expts.sh at the reference's batch size, legs alternated
repeat by repeat in one sitting:

    (i)    the PARENT commit's build, untraced            (--parent-lib PATH: a libvaek.so built from the parent commit; else skipped)
    (ii)   this build, untraced
    (iii)  this build, traced with every = 1000, 100, 10, 1 (ring of min(steps / every, 4096) records)
    (iv)   the workaround the ring replaces: the loop cut by hand every 100 steps, params and grads copied out at each cut -- for
           one model (library calls + two device copies per cut) and for a trainer.ReplicaLoop of R = 64 models (run(100) again
           and again, with its 10 R small copies per cut), the latter beside ReplicaLoop(trajectory_every=100) in ONE run(steps)

    python tools/time_trajectory.py [--shapes 0,1,2,3,4,5] [--batch 100] [--steps 20000] [--repeats 5] [--replicas 64] [--parent-lib PATH]

One child process per shape, each under its own `timeout -k 10`; the first child that does not exit 0 ends the run.  Per leg: min /
median / max of the repeats.  The one condition (the last line): on every shape leg (ii)'s min-max range overlaps or lies below leg
(i)'s, i.e. min(ii) <= max(i) -- the untraced kernels must not have become slower.  Legs (i) - (iii) and (iv, one model) call the
engine directly on their own buffers, so they time the library, not the Python around it."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="0,1,2,3,4,5")
ap.add_argument("--batch", type=int, default=100)
ap.add_argument("--steps", type=int, default=20000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--replicas", type=int, default=64)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--child-limit", type=int, default=240, help="seconds a shape's child process may take")
ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
opt = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (dd, pad, L) of the script's six distinct rows; D = dd + pad + 1
SHAPES = [(3, 3, 6), (3, 13, 8), (5, 16, 16), (5, 5, 10), (7, 7, 13), (7, 20, 24)]
EVERY = (1000, 100, 10, 1)
CUT = 100

if opt.child is None:
    ok = True
    for i in [int(s) for s in opt.shapes.split(",")]:
        cmd = ["timeout", "-k", "10", str(opt.child_limit), sys.executable, os.path.abspath(__file__), "--child", str(i), "--batch", str(opt.batch),
               "--steps", str(opt.steps), "--repeats", str(opt.repeats), "--replicas", str(opt.replicas)]
        if opt.parent_lib:
            cmd += ["--parent-lib", opt.parent_lib]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(f"shape {i}: child exited {r.returncode}; stopping here\n{r.stderr[-2000:]}", flush=True)
            raise SystemExit(r.returncode)
        ok = ok and "condition: holds" in r.stdout
    if opt.parent_lib:
        print(f"condition (untraced min <= parent's untraced max on every shape timed): {'holds' if ok else 'FAILS'}", flush=True)
    else:
        print("condition: not evaluated (no --parent-lib: leg (i) was skipped)", flush=True)
    raise SystemExit(0)

import torch  # noqa: E402
from vae_training_amd import _lib  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

dd, pad, L = SHAPES[opt.child]
D, B, N = dd + pad + 1, opt.batch, opt.steps


def engine_of(lib_path):
    """An Engine on another build of the library (the parent commit's): the symbols that build lacks stay unbound."""
    if lib_path is None:
        return Engine(B, D, L, (), (), -3.0, True, True)
    lib = C.CDLL(os.path.abspath(lib_path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    _lib.load()
    own, _lib._lib = _lib._lib, lib
    try:
        return Engine(B, D, L, (), (), -3.0, True, True)
    finally:
        _lib._lib = own


class Solo:
    """One model's buffers and one way of running N steps on them."""

    def __init__(self, eng, every=None, cut=False):
        self.eng, self.every, self.cut = eng, every, cut
        g = torch.Generator().manual_seed(3)
        self.A = torch.randn(dd, generator=g).cuda()
        self.p = (torch.randn(eng.P, generator=g) * 0.1).cuda()
        self.g, self.m, self.v = eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat()
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ring = None
        if every is not None:
            self.ring = torch.zeros(min(-(-N // every), 4096), eng.trajectory_record_len, device="cuda")
        if cut:
            self.out_p, self.out_g = torch.zeros(N // CUT, eng.P, device="cuda"), torch.zeros(N // CUT, eng.grad_len, device="cuda")

    def call(self, n, **kw):
        self.eng.train_loop_gen(self.p, self.g, self.m, self.v, self.step, n, 1e-4, 1, self.A, dd, dd, pad, 0.0, 9, **kw)

    def run(self):
        if self.cut:
            for i in range(N // CUT):
                self.call(CUT)
                self.out_p[i].copy_(self.p)
                self.out_g[i].copy_(self.g)
        elif self.every is not None:
            self.call(N, trajectory=(self.ring, self.every))
        else:
            self.call(N)


def sweep_models(R):
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments(["t", "--dataset", "sigmoid", "--padding_dim", str(pad), "-dd", str(dd)])
    return [VAEModel(dirname=tempfile.mkdtemp(), num_batches=N * (opt.repeats + 1), num_epochs=1, batch_size=B, learning_rate=args.learning_rate,
                     layer_sizes="", encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False,
                     dataset=get_dataset("sigmoid", 100 + r, pad, B, args), latent_dimension=L, tunable_decoder_var=True,
                     dataset_name="sigmoid", fast_loop=True) for r in range(R)]


class Sweep:
    def __init__(self, R, traced):
        from vae_training_amd.trainer import ReplicaLoop
        self.traced = traced
        self.loop = ReplicaLoop(sweep_models(R), loss_capacity=1 << 12, **(dict(trajectory_every=CUT, trajectory_capacity=N // CUT) if traced else {}))
        if not traced:
            lp = self.loop
            self.out_p = torch.zeros(N // CUT, *lp.params.shape, device="cuda")
            self.out_g = torch.zeros(N // CUT, *lp.grads.shape, device="cuda")

    def run(self):
        if self.traced:
            self.loop.run(N)
            return
        for i in range(N // CUT):
            self.loop.run(CUT)
            self.out_p[i].copy_(self.loop.params)
            self.out_g[i].copy_(self.loop.grads)


own = engine_of(None)
legs = {}
if opt.parent_lib:
    legs["(i)   parent build, untraced"] = Solo(engine_of(opt.parent_lib))
legs["(ii)  this build, untraced"] = Solo(own)
for k in EVERY:
    legs[f"(iii) traced, every = {k}"] = Solo(own, every=k)
legs[f"(iv)  cut by hand every {CUT}, one model"] = Solo(own, cut=True)
if opt.replicas > 0:
    legs[f"(iv)  ReplicaLoop R = {opt.replicas}, run({CUT}) cut by hand"] = Sweep(opt.replicas, False)
    legs[f"      ReplicaLoop R = {opt.replicas}, trajectory_every = {CUT}"] = Sweep(opt.replicas, True)
us = {k: [] for k in legs}
for leg in legs.values():            # warm-up: lazy kernel attributes, allocator
    leg.run()
torch.cuda.synchronize()
for _ in range(opt.repeats):
    for k, leg in legs.items():
        t0 = time.perf_counter()
        leg.run()
        torch.cuda.synchronize()
        us[k].append((time.perf_counter() - t0) / N * 1e6)
print(f"sigmoid D={D:2d} L={L:2d} B={B}  P={own.P}  {N} steps x {opt.repeats} repeats, us per step (of each model's loop) min / median / max", flush=True)
for k, u in us.items():
    print(f"    {k:58s} {min(u):8.3f} {statistics.median(u):8.3f} {max(u):8.3f}", flush=True)
if opt.parent_lib:
    a, b = us["(i)   parent build, untraced"], us["(ii)  this build, untraced"]
    print(f"    condition: {'holds' if min(b) <= max(a) else 'FAILS'} (untraced min {min(b):.3f} <= parent's untraced max {max(a):.3f})", flush=True)
