"""Graph-captured training loop: the reference's hot loop (model.py:221-222 -- get_batch, sample_latent,
train_step, append loss) with NOTHING on the host per step.

The launches of a step -- the Philox dataset + latent draw (K7) and the two kernels of vaek_train_step --
are captured G steps at a time into a hipGraph; the Adam step counter, the RNG step and the loss ring
buffer all live on the device, so replays need no arguments.  At the reference's own batch size (100)
the per-step Python of the drop-in path (~50 us) is 3-4x the GPU time; this loop removes it without
changing what a step computes.

`pipeline=True` (default) draws batch n+1 WHILE step n trains (vaek_train_step_gen): the draw does not
depend on the weights, so its work items ride in the finalize launch of step n -- which by itself keeps
9 of 256 CUs busy -- and write the other of two batch buffers; at <= 256 rows the whole step, draw included,
is ONE launch (10 us per step at the reference's batch size 100).  The draw takes its step from a counter pair the
generator advances itself, not from the Adam step counter that same launch is incrementing.  Same
counters, same Philox streams: losses and parameters are bit-identical to `pipeline=False`
(vaek_make_batch, then vaek_train_step).  (A second stream / parallel graph branch for the draw was
measured first: cross-branch edges of a hipGraph cost far more than the 7 us they were meant to hide.)

`moments` (default: whenever the model qualifies -- a linear VAE on the linear_gaussian or sphere dataset): the steps go through
vaek_train_steps_gen, the headline kernel of bench.py (csrc/linear_moments.hip): up to 64 steps per persistent launch, every
step's batch drawn INSIDE the launch by the workgroups that multiply it -- the same Philox counters as above, so the same
batches bit for bit, but no batch buffer, no hipGraph and nothing per step on the host: one library call per run of steps
between two events of the reference's schedule (stats every 5 000, plot + save every 50 000: model.py:213-220).  The losses land
in the same device ring.  Losses and parameters agree with the per-sample loop to summation order (tests/test_gpu_loop.py).

`resident` (default: RESIDENT_DEFAULT where the model has no moments path and the engine supports it -- small-batch linear VAEs the
moment form does not cover: the two-decoder models of the sigmoid dataset above all; `moments=False` on a model that HAS a moments
path still means the hipGraph loop, resident=True asks for this one there too): the steps go through vaek_train_loop_gen
(csrc/linear_resident.hip), a plain loop of steps inside ONE workgroup with parameters and Adam state on chip and the batches drawn
in the kernel -- the same Philox counters again.  Like the moments path it is one library call per run of steps, no batch buffer and
no hipGraph; there is one workgroup, so there is nothing to wait for and check() has nothing to poll.  `moments` keeps priority:
every model that takes it today still does.

ReplicaLoop (below GraphLoop) is the resident loop for a SWEEP: R models of one shape, one workgroup each, in one launch per run of
steps (vaek_train_loop_gen_replicas); `run.py --sweep_dataset_seeds` drives it.  ReplicaGraphLoop (below it) is the sweep of the
models the resident loop does not cover but the whole-network "mlp3" step does: the pipelined hipGraph loop with every step ONE
vaek_train_step_gen_replicas call for all R models.

`trajectory_every=K` (GraphLoop with the resident loop, ReplicaLoop; opt-in): the resident kernel records, at every Adam step t with
t % K == 0, the parameters that step's gradient was evaluated at and the step's gradient buffer, into a device ring the loop owns
(vaek_train_loop_gen_traj / vaek_train_loop_gen_replicas_traj) -- the reference's `params_and_gradients` list (vae.py:207), which
the reference never fills.  `trajectory()` / `trajectory(r)` returns them in step order; run() stays one library call."""
from __future__ import annotations

import torch

# The evaluations of the n_print events live in events.py; their names stay importable from here.
from .events import (ReplicaElboHessian, ReplicaEvent, ReplicaExactLogLik, ReplicaJacobian, ReplicaJacobianLinear,      # noqa: F401
                     ReplicaJacobianMlp3, ReplicaLogLik, ReplicaLogLikMlp3, ReplicaSampledElboHessian, ReplicaSampledElboHessianMlp3, ReplicaSpectrum, ReplicaStats,
                     ReplicaStatsMlp3, ReplicaSubspace, _replica_setup, _seed_step_tensors, _signature, _wrap_signed)


def _trajectory_capacity(loop_name, models, every, capacity):
    """Records per ring: every recorded step of the longest schedule among the models, ceil(num_batches / K), unless given."""
    if int(every) < 1:
        raise RuntimeError(f"{loop_name}(trajectory_every={every}): need an integer >= 1")
    if capacity is not None:
        if int(capacity) < 1:
            raise RuntimeError(f"{loop_name}(trajectory_capacity={capacity}): need an integer >= 1")
        return int(capacity)
    nb = max(int(getattr(m, "num_batches", 0) or 0) for m in models)
    if nb < 1:
        raise RuntimeError(f"{loop_name}(trajectory_every={every}): the model has no num_batches to size the ring by; pass trajectory_capacity")
    return -(-nb // int(every))


def _trajectory_view(ring, every, first_step, last_step, P):
    """(steps, params [n, P], grads [n, P + 4]) of the records a ring [cap, >= 2 P + 4] (already on the host) holds for the Adam steps
    first_step < t <= last_step with t % every == 0, oldest first: the last `cap` of them, each from slot (t // every - 1) % cap."""
    cap = ring.shape[0]
    idx = list(range(first_step // every + 1, last_step // every + 1))[-cap:]
    slots = torch.tensor([(i - 1) % cap for i in idx], dtype=torch.int64)
    rec = ring[slots] if idx else ring[:0]
    return torch.tensor([i * every for i in idx], dtype=torch.int64), rec[:, :P], rec[:, P:2 * P + 4]


def _ring_in_order(ring, n):
    """The last min(n, cap) of the n values written round-robin into the device ring [cap], oldest first (device -> host once)."""
    cap = ring.numel()
    ring = ring.cpu()
    if n <= cap:
        return ring[:n]
    k = n % cap
    return torch.cat([ring[k:], ring[:k]])


# What GraphLoop(resident=None) resolves to where the engine supports the resident loop and the model has no moments path.  The gate
# is tools/time_resident.py: True only once the resident loop's slowest repeat has beaten the hipGraph loop's fastest on all seven
# shapes.  That table has NOT been measured yet, so the default is off: resident=True asks for the loop explicitly.
RESIDENT_DEFAULT = False


class GraphLoop:
    def __init__(self, vae_model, steps_per_graph=200, seed=None, loss_capacity=1 << 20, pipeline=True, moments=None, resident=None,
                 trajectory_every=None, trajectory_capacity=None):
        m = vae_model
        self.m = m
        ds = m.dataset
        self.kind, self.A, self.dd, self.did, self.pad, self.var = ds.device_spec()
        from .datasets import DEVICE_DRAW_MAX_DIM
        if self.dd > DEVICE_DRAW_MAX_DIM or self.did > DEVICE_DRAW_MAX_DIM:
            raise RuntimeError(f"--fast_loop draws its batches with libvaek's Philox kernel, which supports -dd / -did <= "
                               f"{DEVICE_DRAW_MAX_DIM} (got {self.dd} / {self.did}); run without --fast_loop")
        self.B = m.batch_size
        self.eng = m.model.module.engine(self.B, m.optimizer.global_batch)
        ex = m.optimizer.exchange
        if self.eng.world > 1 and not (ex is not None and ex.in_library) and not self.eng.supports_train_steps_gen(self.kind):
            raise RuntimeError("GraphLoop under data parallelism needs the in-library P2P exchange (GradExchange mode 'p2p'): "
                               "an RCCL all-reduce between the two halves of the step is not captured")
        can = self.eng.supports_train_steps_gen(self.kind)
        if moments and not can:
            raise RuntimeError("GraphLoop(moments=True): vaek_train_steps_gen does not cover this model / dataset")
        self.moments = can if moments is None else bool(moments)
        can_res = not self.moments and self.eng.supports_train_loop_gen(self.kind)
        if resident and not can_res:
            raise RuntimeError("GraphLoop(resident=True): " + ("the moments path has priority" if self.moments else
                                                               "vaek_train_loop_gen does not cover this model / dataset"))
        # by default only where there is no moments path to take: a caller who switches an available moments path off
        # (moments=False) has always been asking for the per-sample hipGraph loop, and still gets it
        self.resident = (can_res and not can and RESIDENT_DEFAULT) if resident is None else bool(resident)
        if trajectory_every is not None and not self.resident:
            raise RuntimeError(f"GraphLoop(trajectory_every={trajectory_every}): the trajectory ring is written by the resident loop "
                               "(vaek_train_loop_gen_traj); " + ("pass resident=True" if can_res else
                                                                  "vaek_train_loop_gen does not cover this model / dataset" if not self.moments
                                                                  else "the moments path has priority on this model"))
        self.row0 = self.eng.rank * self.B           # ranks draw disjoint rows of the global batch
        self.seed = (ds.key[0] ^ ds.key[1] ^ m.key[1]) if seed is None else seed
        self.pipeline = bool(pipeline) and not self.moments and not self.resident
        self.G = int(steps_per_graph)
        if self.pipeline and self.G % 2:
            self.G += 1                              # two batch buffers: a replay must start on the parity it was captured on
        dev = self.eng.device

        def bufs():
            return (torch.empty(self.B, self.eng.D, dtype=torch.float32, device=dev),
                    torch.empty(self.B, self.eng.L, dtype=torch.float32, device=dev),
                    torch.empty(self.B, self.eng.D, dtype=torch.float32, device=dev))
        self.bufs = [] if self.moments or self.resident else [bufs() for _ in range(2 if self.pipeline else 1)]
        self.loss_ring = torch.zeros(loss_capacity, dtype=torch.float32, device=dev)
        self.eng.set_loss_history(self.loss_ring)
        self.graph = None
        self.graph_parity = 0
        self.steps_done_at_attach = m.optimizer.state.step
        self.trajectory_every = None if trajectory_every is None else int(trajectory_every)
        self.traj_ring = None
        if trajectory_every is not None:         # every recorded step of the schedule, sized once
            cap = _trajectory_capacity("GraphLoop", [m], trajectory_every, trajectory_capacity)
            self.traj_ring = torch.zeros(cap, self.eng.trajectory_record_len, dtype=torch.float32, device=dev)
        if self.pipeline:
            n = m.optimizer.state.step
            # the generator's own step counter, a pair used alternately (vaek_make_batch_next): the draw of batch k
            # reads counter[k % 2] and stores k + 1 into the other slot.  Invariant between steps: the batch of the
            # next step n is in bufs[n % 2] and counter[(n + 1) % 2] == n + 1.
            self.counter = torch.tensor([n, n], dtype=torch.int32, device=dev)
            self._make(self.bufs[n % 2], counter=self.counter, which=n % 2)

    def _make(self, out, **kw):
        self.eng.make_batch(self.kind, self.A, self.dd, self.did, self.pad, self.var, self.B, self.seed,
                            tag=0, row0=self.row0, out=out, **kw)

    def _one(self):
        st = self.m.optimizer.state
        lr = self.m.optimizer.optimizer_def.learning_rate
        if self.pipeline:
            n = st.step
            self.eng.train_step_gen(self.m.model.flat, st.grads, st.m, st.v, st.step_dev, self.bufs[n % 2], lr,
                                    self.kind, self.A, self.dd, self.did, self.pad, self.var, self.bufs[(n + 1) % 2],
                                    self.seed, self.counter, (n + 1) % 2, tag=0, row0=self.row0)
        else:
            x, z1, z2 = self.bufs[0]
            self._make(self.bufs[0], step_dev=st.step_dev)
            self.eng.train_step(self.m.model.flat, st.grads, st.m, st.v, st.step_dev, x, z1, z2, lr)
        st.step += 1

    def _capture(self):
        for _ in range(2):                       # warm-up outside capture (lazy kernel attributes etc.)
            self._one()
        torch.cuda.synchronize()
        self.graph_parity = self.m.optimizer.state.step % 2
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(self.G):
                    self._one()
        torch.cuda.current_stream().wait_stream(side)
        # capture does not execute: take back the host-side step mirror it advanced
        self.m.optimizer.state.step -= self.G
        self.graph = g
        return 2

    def run(self, n_steps):
        """Exactly n_steps train steps."""
        if self.moments or self.resident:
            if n_steps > 0:
                st = self.m.optimizer.state
                call = self.eng.train_steps_gen if self.moments else self.eng.train_loop_gen
                kw = {} if self.traj_ring is None else dict(trajectory=dict(buf=self.traj_ring, every=self.trajectory_every))
                call(self.m.model.flat, st.grads, st.m, st.v, st.step_dev, n_steps,
                     self.m.optimizer.optimizer_def.learning_rate, self.kind, self.A, self.dd, self.did, self.pad,
                     self.var, self.seed, tag=0, row0=self.row0, **kw)
                st.step += n_steps
            return
        done = 0
        if self.graph is None and n_steps >= self.G + 2:
            done += self._capture()
        st = self.m.optimizer.state
        if self.graph is not None and self.pipeline and n_steps - done > self.G and st.step % 2 != self.graph_parity:
            self._one()                          # back onto the buffer parity the graph was captured on
            done += 1
        if self.graph is not None and (not self.pipeline or st.step % 2 == self.graph_parity):
            while n_steps - done >= self.G:
                self.graph.replay()
                st.step += self.G
                done += self.G
        for _ in range(n_steps - done):
            self._one()

    def describe(self):
        """One line for run.py: which of the three loops this is."""
        if self.moments:
            return "persistent moment launches (vaek_train_steps_gen)"
        if self.resident:
            return (f"resident linear kernel, {self.eng.train_loop_steps_per_launch} steps per launch" +
                    ("" if self.traj_ring is None else f", trajectory record every {self.trajectory_every} steps "
                                                       f"(ring of {self.traj_ring.shape[0]})"))
        return f"hipGraph of {self.G} steps" + (", next batch drawn inside the step's launch" if self.pipeline else "")

    def check(self):
        """Synchronous.  The persistent launches of the moments path wait for each other's hand-offs with bounded spins: one that
        expired has produced garbage -- stop loudly."""
        if self.moments:
            torch.cuda.synchronize()
            if self.eng.train_steps_gave_up():
                raise RuntimeError(f"a bounded in-launch wait of vaek_train_steps_gen expired (status {self.eng.train_steps_status_word:#x}): "
                                   "the steps since the last check are invalid")

    def losses(self):
        """Losses of all steps run so far in order (device -> host once)."""
        return _ring_in_order(self.loss_ring, self.m.optimizer.state.step)

    @property
    def records_trajectory(self):
        return self.traj_ring is not None

    def trajectory(self):
        """(steps, params [n, P], grads [n, P + 4]) of the records this loop's steps have left, in step order (one device -> host
        copy): record i is Adam step steps[i] (1-based), the parameters its gradient was evaluated at (the state after
        steps[i] - 1 steps) and its gradient buffer (loss, mean Dkl, mean mse, 0 in the last four slots)."""
        if self.traj_ring is None:
            raise RuntimeError("GraphLoop.trajectory(): this loop records none (pass trajectory_every=K with resident=True)")
        return _trajectory_view(self.traj_ring.cpu(), self.trajectory_every, self.steps_done_at_attach, self.m.optimizer.state.step,
                                self.m.model.flat.numel())


class _ReplicaLosses:
    """What VAEModel.model_save_data asks of `model._graph_loop`: the train losses of one replica of a ReplicaLoop."""

    def __init__(self, loop, r):
        self.loop, self.r = loop, r

    def losses(self):
        return self.loop.losses(self.r)

    @property
    def records_trajectory(self):
        return self.loop.traj_ring is not None

    def trajectory(self):
        return self.loop.trajectory(self.r)


class _ReplicaStacks:
    """What the two sweep loops share: the [R, stride] stacks of the models' states, the per-model seeds, learning rates and loss
    rings, and the copies at the boundaries of run()."""

    def _state_stacks(self, stride, loss_capacity):
        """Sets B, P, stride's stacks params / m / v, grads, step_dev, seed_list / seeds (GraphLoop's seed, model by model), lrs and
        rings ([R, loss_capacity]: by default every step of the longest schedule among the models); returns the float32 allocator."""
        ms, R, m0, dev = self.ms, self.R, self.ms[0], self.eng.device
        self.B, self.P = m0.batch_size, m0.model.flat.numel()
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.params, self.m, self.v, self.grads = f32(R, stride), f32(R, stride), f32(R, stride), f32(R, m0.optimizer.state.grads.numel())
        self.step_dev = torch.zeros(R, dtype=torch.int32, device=dev)
        self.seed_list = [(m.dataset.key[0] ^ m.dataset.key[1] ^ m.key[1]) & (2 ** 64 - 1) for m in ms]
        self.seeds = torch.tensor([_wrap_signed(s, 64) for s in self.seed_list], dtype=torch.int64, device=dev)
        self.lrs = torch.tensor([float(m.optimizer.optimizer_def.learning_rate) for m in ms], dtype=torch.float32, device=dev)
        if loss_capacity is None:
            loss_capacity = max(int(getattr(m, "num_batches", 0) or 0) for m in ms) or (1 << 16)
        self.rings = f32(R, int(loss_capacity))
        return f32

    def _rows(self, m, r):
        st = m.optimizer.state
        P = self.P
        return ((self.params[r, :P], m.model.flat), (self.grads[r], st.grads), (self.m[r, :P], st.m), (self.v[r, :P], st.v),
                (self.step_dev[r:r + 1], st.step_dev))

    def _copy_in(self):
        for r, m in enumerate(self.ms):
            for row, own in self._rows(m, r):
                row.copy_(own)

    def _copy_out(self, n_steps):
        for r, m in enumerate(self.ms):
            for row, own in self._rows(m, r):
                own.copy_(row)
            m.optimizer.state.step += n_steps

    def check(self):
        """Nothing to poll: no launch of a sweep loop waits for another."""

    def losses(self, r):
        """Losses of all steps model r has run so far, in order (device -> host once)."""
        return _ring_in_order(self.rings[r], self.ms[r].optimizer.state.step)

    def view(self, r):
        """Model r's `_graph_loop`: losses() without an argument, as VAEModel.model_save_data calls it."""
        return _ReplicaLosses(self, r)


class ReplicaLoop(_ReplicaStacks):
    """A sweep as ONE launch per run of steps: R VAEModels of one shape -- the same batch size, data and latent dimension,
    architecture (a linear VAE the resident loop covers), epsilon, dataset kind, -dd, -did, padding and dataset noise -- each with
    its own dataset matrix, its own parameters and Adam state and its own learning rate, trained by vaek_train_loop_gen_replicas
    (csrc/linear_resident.hip): workgroup r of the launch is model r's resident loop.  Model r's RNG seed is the one GraphLoop
    derives for it (ds.key[0] ^ ds.key[1] ^ m.key[1]), so replica r trains on the batches GraphLoop(model r, resident=True) would
    draw and ends bitwise where that loop ends.

    The states live in [R, stride] stacks owned by the loop.  COPIES AT THE BOUNDARIES OF run(): every run(n) first copies each
    model's `model.flat` and `optimizer.state.{grads, m, v, step_dev}` into its row of the stacks, makes one library call, and
    copies the rows back (and advances `state.step`), so between two run() calls the models are ordinary models: compute_stats,
    plot_epoch, save, checkpoints and anything else that reads or writes their own tensors works unchanged, and a state loaded in
    between is picked up by the next run().  The copies are 5 R small device copies on each side of the call, per run of steps
    between two events of the schedule -- not per step.

    One workgroup per model and no cross-workgroup state: nothing to wait for, check() polls nothing."""

    def __init__(self, vae_models, loss_capacity=None, trajectory_every=None, trajectory_capacity=None):
        def covered():
            if not self.eng.supports_train_loop_gen(self.kind):
                raise RuntimeError("ReplicaLoop: vaek_train_loop_gen does not cover this model / dataset (it needs a float32 linear VAE with "
                                   "one or two decoders, D, L <= 32 and a batch of at most 256 rows)")
        _replica_setup(self, vae_models, "ReplicaLoop", "launch", "batches", "trains", "train_loop_max_replicas", _signature, covered)
        ms, R, dev = self.ms, self.R, self.eng.device
        f32 = self._state_stacks(self.ms[0].model.flat.numel(), loss_capacity)
        nb = self.eng.train_loop_replicas_workspace(R)
        self.workspace = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
        self.trajectory_every = None if trajectory_every is None else int(trajectory_every)
        self.traj_ring = None
        if trajectory_every is not None:         # one ring per model: every recorded step of the longest schedule, sized once
            cap = _trajectory_capacity("ReplicaLoop", ms, trajectory_every, trajectory_capacity)
            self.traj_ring = f32(R, cap, self.eng.trajectory_record_len)
            self.traj_from = [int(m.optimizer.state.step) for m in ms]

    def run(self, n_steps):
        """Exactly n_steps train steps of every model: one library call between the copies in and out."""
        if n_steps <= 0:
            return
        self._copy_in()
        kw = {} if self.traj_ring is None else dict(trajectory=dict(buf=self.traj_ring, every=self.trajectory_every))
        self.eng.train_loop_gen_replicas(self.params, self.grads, self.m, self.v, self.step_dev, n_steps, 0.0, self.kind, self.A,
                                         self.dd, self.did, self.pad, self.var, self.seeds, lrs=self.lrs, a_stride=self.a_stride,
                                         loss_hist=self.rings, workspace=self.workspace, tag=0, row0=0, **kw)
        self._copy_out(n_steps)

    def describe(self):
        """One line for run.py."""
        return (f"resident linear kernel, {self.R} replicas in one launch (vaek_train_loop_gen_replicas), "
                f"{self.eng.train_loop_steps_per_launch} steps per launch" +
                ("" if self.traj_ring is None else f", trajectory record every {self.trajectory_every} steps "
                                                   f"(rings of {self.traj_ring.shape[1]})"))

    def trajectory(self, r):
        """(steps, params [n, P], grads [n, P + 4]) of the records model r's steps in this loop have left, in step order (one device
        -> host copy of its ring); see GraphLoop.trajectory."""
        if self.traj_ring is None:
            raise RuntimeError("ReplicaLoop.trajectory(): this loop records none (pass trajectory_every=K)")
        m = self.ms[r]
        return _trajectory_view(self.traj_ring[r].cpu(), self.trajectory_every, self.traj_from[r], m.optimizer.state.step,
                                m.model.flat.numel())

    def stats_event(self, rows=None):
        """One stats event of every model in ONE launch (ReplicaStats, vaek_stats_event_replicas): [compute_stats' dict of model 0,
        ...], with the models' keys, draw counters and lists advanced exactly as compute_stats would advance them."""
        if getattr(self, "_stats", None) is None or (rows is not None and int(rows) != self._stats.rows):
            self._stats = ReplicaStats(self.ms, rows=rows)
        return self._stats.event()


class ReplicaGraphLoop(_ReplicaStacks):
    """A sweep of three-hidden-layer MLP VAEs (step path "mlp3") as GraphLoop's pipelined hipGraph loop with R models per step: R
    VAEModels of one shape -- validated as in ReplicaLoop: one batch size, data and latent dimension, architecture, epsilon,
    dataset kind, -dd, -did, padding and dataset noise -- each with its own dataset matrix, parameters, Adam state and learning
    rate.  Every step is ONE vaek_train_step_gen_replicas call (csrc/fused_mlp3.hip: two launches, blockIdx.y = model): it trains
    model r on its slice of one stacked batch buffer and draws model r's next batch into its slice of the other.  Model r's RNG
    seed is the one GraphLoop derives for it, so model r ends bitwise where GraphLoop(model r, moments=False, resident=False) ends.

    The states live in [R, stride] stacks owned by the loop, stride = P rounded up to a multiple of 4 (the library's stride rule);
    they are COPIED at the boundaries of run(), in before the steps and out after them, as in ReplicaLoop: between two run() calls
    every model is an ordinary model.  The stacked batch buffers hold each model's NEXT batch between runs; a model whose step
    counter was changed between two runs (a loaded checkpoint) has the buffers drawn afresh.

    As in GraphLoop there are two batch buffers and a generator counter pair per model ([R, 2]); a graph of steps_per_graph steps
    (made even) is captured once, after one eager warm-up step, and replayed on the buffer parity it was captured on.  Single GPU
    only.  Neither launch waits for anything: check() polls nothing."""

    def __init__(self, vae_models, steps_per_graph=200, loss_capacity=None):
        def covered():
            if not self.eng.supports_train_step_replicas():
                raise RuntimeError("ReplicaGraphLoop: vaek_train_step_gen_replicas does not cover this model (it needs the \"mlp3\" train step: "
                                   "float32, three hidden layers of 64 .. 256 units in encoder and decoder, D, L <= 32, a batch of at most 128 rows)")
        _replica_setup(self, vae_models, "ReplicaGraphLoop", "step", "batches", "trains", "train_step_max_replicas", _signature,
                       covered)
        R, dev = self.R, self.eng.device
        self.G = int(steps_per_graph) + int(steps_per_graph) % 2      # two batch buffers: a replay starts on the parity it was captured on
        D, L = self.eng.D, self.eng.L
        self.stride = (self.ms[0].model.flat.numel() + 3) // 4 * 4
        f32 = self._state_stacks(self.stride, loss_capacity)
        self.bufs = [(f32(R, self.B, D), f32(R, self.B, L), f32(R, self.B, D)) for _ in range(2)]
        self.counter = torch.zeros(R, 2, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(max(self.eng.train_step_replicas_workspace(R), 16), dtype=torch.uint8, device=dev)
        self.par = 0                          # the buffer that holds the next step's batches
        self.expect = None                    # the models' step counters at which self.bufs[self.par] is valid
        self.graph = None
        self.graph_parity = 0

    def _prime(self):
        """Model r's batch of its next step n_r into self.bufs[self.par][.][r] and its counter pair to (n_r, n_r + 1) in the order
        the steps alternate in -- GraphLoop's invariant, model by model (vaek_make_batch_next on each model's slices)."""
        p = self.par
        steps = [int(m.optimizer.state.step) for m in self.ms]
        self.counter.copy_(torch.tensor([[n, n] for n in steps], dtype=torch.int32))
        for r in range(self.R):
            self.eng.make_batch(self.kind, None if self.A is None else self.A[r], self.dd, self.did, self.pad, self.var, self.B,
                                self.seed_list[r], tag=0, row0=0, out=tuple(t[r] for t in self.bufs[p]), counter=self.counter[r], which=p)
        self.expect = steps

    def _one(self):
        p = self.par
        self.eng.train_step_gen_replicas(self.params, self.grads, self.m, self.v, self.step_dev, self.bufs[p], 0.0, self.kind, self.A,
                                         self.dd, self.did, self.pad, self.var, self.bufs[p ^ 1], self.seeds, self.counter, p ^ 1,
                                         lrs=self.lrs, a_stride=self.a_stride, loss_hist=self.rings, workspace=self.workspace, tag=0,
                                         row0=0)
        self.par = p ^ 1

    def _capture(self):
        self._one()                              # warm-up outside capture (lazy kernel attributes)
        torch.cuda.synchronize()
        self.graph_parity = self.par
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(self.G):          # an even number of steps: self.par ends where it began
                    self._one()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = g
        return 1

    def run(self, n_steps):
        """Exactly n_steps train steps of every model: one library call per step (or per replayed graph node) between the copies
        in and out."""
        if n_steps <= 0:
            return
        self._copy_in()
        if self.expect != [int(m.optimizer.state.step) for m in self.ms]:
            self._prime()
        done = 0
        if self.graph is None and n_steps >= self.G + 1:
            done += self._capture()
        if self.graph is not None and n_steps - done > self.G and self.par != self.graph_parity:
            self._one()                          # back onto the buffer parity the graph was captured on
            done += 1
        if self.graph is not None and self.par == self.graph_parity:
            while n_steps - done >= self.G:
                self.graph.replay()
                done += self.G
        for _ in range(n_steps - done):
            self._one()
        self._copy_out(n_steps)
        self.expect = [int(m.optimizer.state.step) for m in self.ms]

    def describe(self):
        """One line for run.py."""
        return (f"hipGraph of {self.G} steps, {self.R} replicas per step (vaek_train_step_gen_replicas), "
                "next batches drawn inside the step's second launch")

    def stats_event(self, rows=None):
        """One stats event of every model in ONE call (ReplicaStatsMlp3, vaek_mlp3_stats_event_replicas): [compute_stats' dict of model
        0, ...], with the models' keys, draw counters and lists advanced exactly as compute_stats would advance them."""
        if getattr(self, "_stats", None) is None or (rows is not None and int(rows) != self._stats.rows):
            self._stats = ReplicaStatsMlp3(self.ms, rows=rows)
        return self._stats.event()
