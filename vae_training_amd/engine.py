"""Host-side handle on a libvaek context: flat parameter layout, workspace, raw kernel calls.

Everything here passes raw device pointers of PyTorch-ROCm tensors plus torch's current HIP
stream through the C ABI (include/vaek.h); torch is plumbing (memory, streams), not compute.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch

from . import _lib, layout


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "libvaek takes contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, device):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    return t.to(device=device, dtype=torch.float32).contiguous()


def _addr(v, dtype=None):
    """The address of device tensor v (of `dtype`, where one is given) or v itself where it is a raw device address; None stays."""
    assert v is None or isinstance(v, int) or dtype is None or v.dtype == dtype
    return None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr())


def _last_dim(v, given=None):
    """`given`, else the last dimension of tensor v: the stride of its records (0 for None or a raw address)."""
    return int((0 if v is None or isinstance(v, int) else v.shape[-1]) if given is None else given)


def _describe(d, params, rows, out, out_dtype, n, state_stride, out_stride, struct_size, draws, a_stride=None, given=None, raw_out=False):
    """Fill, in the fresh descriptor `d` of an evaluation call (vaek_stats_event, vaek_log_likelihood, ...), the fields they share:
    struct_size, n, rows and state_stride; per stream p of `draws` = {p: (seeds int64 [n], steps int32 [n])} the fields p_seeds and
    p_steps; a_stride where the call draws data rows; the caller's rows `given` = (p, float32 tensor [rows, .] or [n, rows, .] or
    None, stride or None) as p and p_stride (0: shared by all replicas); out (of `out_dtype`; with raw_out also a raw device
    address) and out_stride.  n and the strides default to the tensors' shapes."""
    d.struct_size = C.sizeof(type(d)) if struct_size is None else int(struct_size)
    d.n = int(params.shape[0] if n is None else n)
    d.rows = int(rows)
    d.state_stride = int(params.shape[1] if state_stride is None else state_stride)
    for p, (seeds, steps) in draws.items():
        assert seeds is None or seeds.dtype == torch.int64
        assert steps is None or steps.dtype == torch.int32
        setattr(d, p + "_seeds", _ptr(seeds))
        setattr(d, p + "_steps", _ptr(steps))
    if a_stride is not None:
        d.a_stride = int(a_stride)
    if given is not None:
        p, t, stride = given
        assert t is None or t.dtype == torch.float32
        setattr(d, p, _ptr(t))
        if stride is None:
            stride = 0 if t is None or t.dim() < 3 else t.shape[-2] * t.shape[-1]
        setattr(d, p + "_stride", int(stride))
    assert out is None or isinstance(out, int) or out.dtype == out_dtype
    d.out = _addr(out) if raw_out else _ptr(out)
    d.out_stride = _last_dim(out, out_stride)
    return d


class Engine:
    """One libvaek context = one (batch, architecture) shape on one GPU."""

    def __init__(self, batch, data_dim, latent_dim, enc_hidden=(), dec_hidden=(), epsilon=0.0,
                 tunable_decoder_var=False, sigmoid_decoder=False, device=None, world=1, rank=0,
                 global_batch=0, dtype="f32", force_generic=False, fused_impl="auto"):
        if not torch.cuda.is_available():
            raise RuntimeError("vae_training_amd needs an MI355X (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        cfg = _lib.VaekConfig()
        cfg.struct_size = C.sizeof(_lib.VaekConfig)
        cfg.batch, cfg.data_dim, cfg.latent_dim = int(batch), int(data_dim), int(latent_dim)
        enc_hidden, dec_hidden = list(enc_hidden), list(dec_hidden)
        if len(enc_hidden) > _lib.VAEK_MAX_HIDDEN or len(dec_hidden) > _lib.VAEK_MAX_HIDDEN:
            raise ValueError(f"at most {_lib.VAEK_MAX_HIDDEN} hidden layers per network")
        cfg.n_enc_hidden, cfg.n_dec_hidden = len(enc_hidden), len(dec_hidden)
        for i, h in enumerate(enc_hidden):
            cfg.enc_hidden[i] = int(h)
        for i, h in enumerate(dec_hidden):
            cfg.dec_hidden[i] = int(h)
        cfg.sigmoid_decoder = int(bool(sigmoid_decoder))
        cfg.tunable_eps = int(bool(tunable_decoder_var))
        cfg.eps_cli = float(epsilon)
        cfg.dtype = {"f32": _lib.VAEK_F32, "bf16": _lib.VAEK_BF16}[dtype]
        cfg.device = self.device.index
        cfg.world, cfg.rank, cfg.global_batch = int(world), int(rank), int(global_batch)
        self.world, self.rank = int(world), int(rank)
        cfg.force_generic = int(bool(force_generic))
        cfg.reserved[0] = {"auto": 0, "mfma": 0, "valu": 1}[fused_impl]      # which fused linear-VAE kernel
        self.cfg = cfg
        h = C.c_void_p()
        _lib.check(self.lib.vaek_ctx_create(C.byref(cfg), C.byref(h)))
        self.h = h
        n = C.c_int64()
        _lib.check(self.lib.vaek_param_count(h, C.byref(n)))
        self.P = n.value
        _lib.check(self.lib.vaek_grad_len(h, C.byref(n)))
        self.grad_len = n.value
        _lib.check(self.lib.vaek_train_steps_moment_len(h, C.byref(n)))
        self._moment_len = n.value
        nl = C.c_int32()
        _lib.check(self.lib.vaek_leaf_count(h, C.byref(nl)))
        self.leaves = OrderedDict()
        buf = C.create_string_buffer(64)
        for i in range(nl.value):
            off, r, c = C.c_int64(), C.c_int32(), C.c_int32()
            _lib.check(self.lib.vaek_leaf_info(h, i, buf, 64, C.byref(off), C.byref(r), C.byref(c)))
            name = buf.value.decode()
            shape = (c.value,) if r.value == 1 and not name.endswith("kernel") else (r.value, c.value)
            self.leaves[name] = (off.value, shape)
        want, want_p = layout.leaves(data_dim, latent_dim, enc_hidden, dec_hidden, sigmoid_decoder, tunable_decoder_var)
        assert want_p == self.P and list(want.items()) == list(self.leaves.items()), "layout.py disagrees with libvaek"
        ws = C.c_size_t()
        _lib.check(self.lib.vaek_workspace_bytes(h, C.byref(ws)))
        self.workspace = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=self.device)
        assert self.workspace.data_ptr() % 256 == 0
        f = C.c_int32()
        _lib.check(self.lib.vaek_uses_fused_path(h, C.byref(f)))
        self.fused = bool(f.value)
        _lib.check(self.lib.vaek_train_step_path(h, buf, 64))
        self.step_path = buf.value.decode()      # "linear", "mlp1", "mlp3", "linear_wide" or "layers"
        self.batch, self.D, self.L = int(batch), int(data_dim), int(latent_dim)

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.lib.vaek_ctx_destroy(h)
            except Exception:
                pass

    def _flag(self, fn, *args):
        """A yes / no query of the context: fn(ctx, *args, &int32)."""
        f = C.c_int32()
        _lib.check(fn(self.h, *args, C.byref(f)))
        return bool(f.value)

    def _count(self, fn, *args, ctype=C.c_int64):
        """A length (int64) or byte count (ctype=C.c_size_t) query of the context: fn(ctx, *args, &count)."""
        n = ctype()
        _lib.check(fn(self.h, *args, C.byref(n)))
        return int(n.value)

    # ---- flat buffers ----------------------------------------------------------------------
    def new_flat(self, n=None):
        return torch.zeros(self.P if n is None else n, dtype=torch.float32, device=self.device)

    def views(self, flat):
        return layout.views(flat, self.leaves)

    # ---- hot path ----------------------------------------------------------------------------
    def train_step(self, params, grads, m, v, step_dev, x, z1, z2, lr):
        _lib.check(self.lib.vaek_train_step(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev),
                                            _ptr(x), _ptr(z1), _ptr(z2), float(lr), _ptr(self.workspace), _stream()))

    def train_step_gen(self, params, grads, m, v, step_dev, cur, lr, kind, A, dd, did, pad, var_added, nxt, seed, counter,
                       which, tag=0, row0=0):
        """vaek_train_step on the batch `cur` = (x, z1, z2) and the draw of the next batch into `nxt` (its step is
        counter[which], and counter[which ^ 1] = step + 1 is stored) -- on the fused path inside the finalize launch."""
        assert counter.dtype == torch.int32 and counter.numel() == 2 and counter.is_cuda
        _lib.check(self.lib.vaek_train_step_gen(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev),
                                                _ptr(cur[0]), _ptr(cur[1]), _ptr(cur[2]), float(lr), _ptr(self.workspace),
                                                int(kind), _ptr(A), int(dd), int(did), int(pad), float(var_added),
                                                _ptr(nxt[0]), _ptr(nxt[1]), _ptr(nxt[2]), int(row0), int(seed) & (2**64 - 1),
                                                _ptr(counter), int(which), int(tag), _stream()))

    def supports_train_steps(self):
        return self._flag(self.lib.vaek_supports_train_steps)

    def train_steps(self, params, grads, m, v, step_dev, batches, lr):
        """len(batches) consecutive train steps, batch i = (x, z1, z2) device tensors, software-pipelined over launches
        (vaek_train_steps; linear VAEs only).  Asynchronous; capturable into a hipGraph."""
        n = len(batches)
        arr = lambda k: (C.c_void_p * n)(*[C.c_void_p(b[k].data_ptr()) for b in batches])
        for b in batches:
            assert all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in b)
        xs, z1s, z2s = arr(0), arr(1), arr(2)
        _lib.check(self.lib.vaek_train_steps(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), xs, z1s, z2s, n,
                                             float(lr), _ptr(self.workspace), _stream()))

    def supports_train_steps_gen(self, kind):
        return self._flag(self.lib.vaek_supports_train_steps_gen, int(kind))

    def train_steps_gen(self, params, grads, m, v, step_dev, n_steps, lr, kind, A, dd, did, pad, var_added, seed, tag=0, row0=0):
        """n_steps consecutive train steps whose batches are drawn INSIDE the launch (vaek_train_steps_gen): the batch of the step
        that takes the Adam counter from t to t + 1 is bit for bit the one make_batch(..., step = t) would write, but it never
        exists in HBM.  Asynchronous; capturable into a hipGraph."""
        _lib.check(self.lib.vaek_train_steps_gen(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), int(kind), _ptr(A),
                                                 int(dd), int(did), int(pad), float(var_added), int(row0), int(seed) & (2**64 - 1), int(tag),
                                                 int(n_steps), float(lr), _ptr(self.workspace), _stream()))

    def supports_train_loop_gen(self, kind):
        return self._flag(self.lib.vaek_supports_train_loop_gen, int(kind))

    @property
    def train_loop_steps_per_launch(self):
        return int(self.lib.vaek_train_loop_steps_per_launch())

    @property
    def trajectory_record_len(self):
        """Floats in one trajectory record (vaek_trajectory_record_len): 2 P + 4 = the parameters, then the gradient buffer."""
        return self._count(self.lib.vaek_trajectory_record_len)

    @staticmethod
    def _trajectory(trajectory):
        """vaek_trajectory from `trajectory` = (buf, every) or a dict(buf=, every=, cap=, record_stride=, replica_stride=): buf is a
        float32 device tensor [cap, record_stride] (solo) or [n, cap, record_stride] (replicas); cap and the strides default to its
        shape.  The tensor must stay alive until the call has run."""
        if not isinstance(trajectory, dict):
            trajectory = dict(buf=trajectory[0], every=trajectory[1])
        buf = trajectory["buf"]
        assert buf is None or buf.dtype == torch.float32
        tj = _lib.VaekTrajectory()
        tj.struct_size = int(trajectory.get("struct_size", C.sizeof(_lib.VaekTrajectory)))
        tj.every = int(trajectory["every"])
        tj.buf = _ptr(buf)
        shape = (1, 1, 1) if buf is None else tuple(buf.shape)
        tj.cap = int(trajectory["cap"]) if "cap" in trajectory else shape[-2]
        tj.record_stride = int(trajectory["record_stride"]) if "record_stride" in trajectory else shape[-1]
        tj.replica_stride = int(trajectory["replica_stride"]) if "replica_stride" in trajectory else tj.cap * tj.record_stride
        return tj

    def train_loop_gen(self, params, grads, m, v, step_dev, n_steps, lr, kind, A, dd, did, pad, var_added, seed, tag=0, row0=0,
                       trajectory=None):
        """n_steps consecutive train steps as a loop INSIDE one workgroup (vaek_train_loop_gen): small-batch linear VAEs with one or
        two decoders, parameters and Adam state on chip between steps, the batch of the step that takes the Adam counter from t
        to t + 1 bit for bit the one make_batch(..., step = t) would write.  Asynchronous; capturable into a hipGraph.
        `trajectory` (see _trajectory; vaek_train_loop_gen_traj): every Adam step t with t % every == 0 leaves its record -- the
        parameters before the update, then the gradient buffer -- in slot (t // every - 1) % cap of the ring."""
        if trajectory is not None:
            tj = self._trajectory(trajectory)
            _lib.check(self.lib.vaek_train_loop_gen_traj(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), int(kind), _ptr(A),
                                                         int(dd), int(did), int(pad), float(var_added), int(row0), int(seed) & (2**64 - 1),
                                                         int(tag), int(n_steps), float(lr), _ptr(self.workspace), _stream(), C.byref(tj)))
            return
        _lib.check(self.lib.vaek_train_loop_gen(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), int(kind), _ptr(A),
                                                int(dd), int(did), int(pad), float(var_added), int(row0), int(seed) & (2**64 - 1), int(tag),
                                                int(n_steps), float(lr), _ptr(self.workspace), _stream()))

    @property
    def train_loop_max_replicas(self):
        return int(self.lib.vaek_train_loop_max_replicas())

    def train_loop_replicas_workspace(self, n):
        """Bytes of the workspace Engine.train_loop_gen_replicas needs for n replicas (its own buffer, not self.workspace): n staged
        batches where the kernel's LDS has no room for one, else 0."""
        return self._count(self.lib.vaek_train_loop_replicas_workspace_bytes, int(n), ctype=C.c_size_t)

    def train_loop_gen_replicas(self, params, grads, m, v, step_dev, n_steps, lr, kind, A, dd, did, pad, var_added, seeds, lrs=None,
                                a_stride=0, loss_hist=None, workspace=None, tag=0, row0=0, n=None, state_stride=None, grads_stride=None,
                                loss_hist_cap=None, trajectory=None):
        """n_steps train steps of EACH of n independent models of this engine's shape in one launch, workgroup r training replica r
        (vaek_train_loop_gen_replicas).  params / m / v: [n, state_stride], grads: [n, grads_stride], step_dev: int32 [n], seeds:
        int64 [n] (the bits of the uint64 seeds), lrs: float32 [n] or None (then `lr` for all), A: replica r's at A + r * a_stride
        floats (0: shared), loss_hist: [n, cap] or None -- all device tensors; n, the strides and cap default to the tensors'
        shapes.  Replica r ends bitwise where train_loop_gen alone on its slices would.  Asynchronous; capturable.
        `trajectory` (see _trajectory; vaek_train_loop_gen_replicas_traj): replica r's ring is buf[r]."""
        rep = self._replicas_desc(params, grads, seeds, lrs, a_stride, loss_hist, n, state_stride, grads_stride, loss_hist_cap)
        args = (self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), C.byref(rep), int(kind), _ptr(A), int(dd), int(did),
                int(pad), float(var_added), int(row0), int(tag), int(n_steps), float(lr), _ptr(workspace), _stream())
        if trajectory is not None:
            tj = self._trajectory(trajectory)
            _lib.check(self.lib.vaek_train_loop_gen_replicas_traj(*args, C.byref(tj)))
            return
        _lib.check(self.lib.vaek_train_loop_gen_replicas(*args))

    def supports_stats_event(self, kind):
        """True where stats_event_replicas covers this engine and dataset kind: exactly where supports_train_loop_gen does."""
        return self._flag(self.lib.vaek_supports_stats_event, int(kind))

    @property
    def stats_record_len(self):
        """Floats in one stats record (vaek_stats_record_len): 8 + L = loss, mean Dkl, mean mse, eps, two score values, 0, 0, epsilon_p."""
        return self._count(self.lib.vaek_stats_record_len)

    @property
    def stats_event_max_rows(self):
        return int(self.lib.vaek_stats_event_max_rows())

    def stats_event_replicas(self, params, rows, kind, A, dd, did, pad, var_added, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out,
                             a_stride=0, x_tag=1, z_tag=2, n=None, state_stride=None, out_stride=None, struct_size=None):
        """The stats event of EACH of n independent models of this engine's shape in one launch, workgroup r evaluating replica r
        (vaek_stats_event_replicas): `rows` real rows drawn under (x_seeds[r], x_steps[r], x_tag) and `rows` latent rows under
        (z_seeds[r], z_steps[r], z_tag) exactly as make_batch draws them, VAE.loss on them, a fake batch sampled from the same
        latents with eps = sample_eps[r], and its score.  params: [n, state_stride] (read only), x_seeds / z_seeds: int64 [n] (the
        bits of the uint64 seeds), x_steps / z_steps: int32 [n] (the bits of the uint32 steps), sample_eps: float32 [n], A: replica
        r's at A + r * a_stride floats (0: shared), out: float32 [n, out_stride >= stats_record_len] -- all device tensors; n and
        the strides default to the tensors' shapes.  Record r lands in out[r, :stats_record_len]: loss, mean Dkl, mean mse, eps, the
        score values in score_batch's order, 0, 0, epsilon_p.  Asynchronous; capturable."""
        ev = self._stats_event_desc(params, rows, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, a_stride, n, state_stride, out_stride,
                                    struct_size)
        _lib.check(self.lib.vaek_stats_event_replicas(self.h, _ptr(params), C.byref(ev), int(kind), _ptr(A), int(dd), int(did), int(pad),
                                                      float(var_added), int(x_tag), int(z_tag), _stream()))

    @staticmethod
    def _replicas_desc(params, grads, seeds, lrs, a_stride, loss_hist, n, state_stride, grads_stride, loss_hist_cap):
        """The vaek_replicas description both replica train calls take, from tensors; n, the strides and cap default to the tensors' shapes."""
        rep = _lib.VaekReplicas()
        rep.struct_size = C.sizeof(_lib.VaekReplicas)
        rep.n = int(params.shape[0] if n is None else n)
        rep.state_stride = int(params.shape[1] if state_stride is None else state_stride)
        rep.grads_stride = int(grads.shape[1] if grads_stride is None else grads_stride)
        assert seeds is None or seeds.dtype == torch.int64
        assert lrs is None or lrs.dtype == torch.float32
        rep.seeds, rep.lrs = _ptr(seeds), _ptr(lrs)
        rep.a_stride = int(a_stride)
        rep.loss_hist = _ptr(loss_hist)
        rep.loss_hist_cap = _last_dim(loss_hist, loss_hist_cap)
        return rep

    @staticmethod
    def _stats_event_desc(params, rows, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, a_stride, n, state_stride, out_stride, struct_size):
        """The vaek_stats_event description both stats-event calls take, from tensors; strides default to the tensors' shapes."""
        ev = _describe(_lib.VaekStatsEvent(), params, rows, out, torch.float32, n, state_stride, out_stride, struct_size, a_stride=a_stride,
                       draws=dict(x=(x_seeds, x_steps), z=(z_seeds, z_steps)))
        assert sample_eps is None or sample_eps.dtype == torch.float32
        ev.sample_eps = _ptr(sample_eps)
        return ev

    def supports_mlp3_stats_event(self, kind):
        """True where mlp3_stats_event_replicas covers this engine and dataset kind: exactly where supports_mlp3_log_likelihood does --
        float32, one decoder, exactly three hidden layers of 64 .. 256 units both ways, D, L <= 32, whatever the engine's batch, world
        and force_generic are (vaek_supports_mlp3_stats_event)."""
        return self._flag(self.lib.vaek_supports_mlp3_stats_event, int(kind))

    def mlp3_stats_event_workspace(self, n, rows):
        """Bytes of the workspace mlp3_stats_event_replicas needs (its own buffer, 16-byte aligned, not self.workspace)."""
        return self._count(self.lib.vaek_mlp3_stats_event_workspace_bytes, int(n), int(rows), ctype=C.c_size_t)

    def mlp3_stats_event_replicas(self, params, rows, kind, A, dd, did, pad, var_added, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out,
                                  workspace, a_stride=0, x_tag=1, z_tag=2, n=None, state_stride=None, out_stride=None, struct_size=None):
        """stats_event_replicas for three-hidden-layer MLP VAEs (vaek_mlp3_stats_event_replicas): the same draws, record and arguments,
        with the relu stacks as Encoder and Decoder; workspace: uint8 of mlp3_stats_event_workspace(n, rows) bytes.  Two launches
        whatever n is.  Asynchronous; capturable."""
        ev = self._stats_event_desc(params, rows, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, a_stride, n, state_stride, out_stride,
                                    struct_size)
        _lib.check(self.lib.vaek_mlp3_stats_event_replicas(self.h, _ptr(params), C.byref(ev), int(kind), _ptr(A), int(dd), int(did), int(pad),
                                                           float(var_added), int(x_tag), int(z_tag), _addr(workspace), _stream()))

    def supports_log_likelihood(self, kind):
        """True where log_likelihood_replicas covers this engine and dataset kind: a float32 linear VAE with one or two decoders, D, L <= 32
        (D <= 28 with two decoders), whatever the engine's batch and world are (vaek_supports_log_likelihood)."""
        return self._flag(self.lib.vaek_supports_log_likelihood, int(kind))

    @property
    def log_likelihood_record_len(self):
        """Floats in one log-likelihood record: 4 = IWAE-K bound, K-sample ELBO estimate, normalised effective sample size, eps."""
        return int(self.lib.vaek_log_likelihood_record_len())

    @property
    def log_likelihood_max_rows(self):
        return int(self.lib.vaek_log_likelihood_max_rows())

    @property
    def log_likelihood_max_samples(self):
        return int(self.lib.vaek_log_likelihood_max_samples())

    def log_likelihood_workspace(self, n, rows):
        """Bytes of the workspace log_likelihood_replicas needs for n replicas of `rows` rows (its own buffer, not self.workspace)."""
        return self._count(self.lib.vaek_log_likelihood_workspace_bytes, int(n), int(rows), ctype=C.c_size_t)

    @staticmethod
    def _log_likelihood_desc(params, rows, samples, z_seeds, z_steps, out, x_seeds, x_steps, x, x_stride, a_stride, n, state_stride, out_stride,
                             struct_size):
        """The vaek_log_likelihood description both log-likelihood calls take, from tensors; strides default to the tensors' shapes."""
        ll = _describe(_lib.VaekLogLikelihood(), params, rows, out, torch.float32, n, state_stride, out_stride, struct_size, a_stride=a_stride,
                       draws=dict(x=(x_seeds, x_steps), z=(z_seeds, z_steps)), given=("x", x, x_stride))
        ll.samples = int(samples)
        return ll

    def log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, kind=2, A=None, dd=0, did=0, pad=0,
                                var_added=0.0, x_seeds=None, x_steps=None, x=None, x_stride=None, a_stride=0, x_tag=3, z_tag=4, n=None,
                                state_stride=None, out_stride=None, struct_size=None):
        """The importance-weighted log-likelihood of EACH of n independent models of this engine's shape in one call
        (vaek_log_likelihood_replicas): over `rows` data rows and `samples` posterior samples per row, record r = [IWAE bound, ELBO
        estimate, normalised effective sample size, eps] in out[r, :4].  The rows are the caller's (x: float32 [rows, D] shared by all
        replicas, or [n, rows, D]) or, with x None, drawn under (x_seeds[r], x_steps[r], x_tag) exactly as make_batch draws them from
        (kind, A, dd, did, pad, var_added); sample k of a row takes blocks k * ceil(L / 4) .. of the latent stream under (z_seeds[r],
        z_steps[r], z_tag).  params: [n, state_stride] (read only), seeds int64 [n], steps int32 [n], out: float32 [n, out_stride >=
        4], workspace: uint8 of log_likelihood_workspace(n, rows) bytes -- all device tensors; n and the strides default to the
        tensors' shapes.  Asynchronous; capturable."""
        ll = self._log_likelihood_desc(params, rows, samples, z_seeds, z_steps, out, x_seeds, x_steps, x, x_stride, a_stride, n, state_stride,
                                       out_stride, struct_size)
        _lib.check(self.lib.vaek_log_likelihood_replicas(self.h, _ptr(params), C.byref(ll), int(kind), _ptr(A), int(dd), int(did), int(pad),
                                                         float(var_added), int(x_tag), int(z_tag), _addr(workspace), _stream()))

    def supports_mlp3_log_likelihood(self, kind):
        """True where mlp3_log_likelihood_replicas covers this engine and dataset kind: float32, one decoder, exactly three hidden layers
        of 64 .. 256 units in the encoder and in the decoder, D, L <= 32 -- whatever the engine's batch, world and force_generic are
        (vaek_supports_mlp3_log_likelihood)."""
        return self._flag(self.lib.vaek_supports_mlp3_log_likelihood, int(kind))

    @property
    def mlp3_log_likelihood_max_columns(self):
        """The cap on n * rows * samples of one mlp3_log_likelihood_replicas call (vaek_mlp3_log_likelihood_max_columns)."""
        return int(self.lib.vaek_mlp3_log_likelihood_max_columns())

    def mlp3_log_likelihood_workspace(self, n, rows, samples):
        """Bytes of the workspace mlp3_log_likelihood_replicas needs (its own buffer, 16-byte aligned, not self.workspace)."""
        return self._count(self.lib.vaek_mlp3_log_likelihood_workspace_bytes, int(n), int(rows), int(samples), ctype=C.c_size_t)

    def mlp3_log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, kind=2, A=None, dd=0, did=0, pad=0,
                                     var_added=0.0, x_seeds=None, x_steps=None, x=None, x_stride=None, a_stride=0, x_tag=3, z_tag=4, n=None,
                                     state_stride=None, out_stride=None, struct_size=None):
        """log_likelihood_replicas for three-hidden-layer MLP VAEs (vaek_mlp3_log_likelihood_replicas): the same estimator, record, block
        rule, row modes and arguments, with the relu stacks as Encoder and Decoder; workspace: uint8 of
        mlp3_log_likelihood_workspace(n, rows, samples) bytes.  Four launches whatever n is.  Asynchronous; capturable."""
        ll = self._log_likelihood_desc(params, rows, samples, z_seeds, z_steps, out, x_seeds, x_steps, x, x_stride, a_stride, n, state_stride,
                                       out_stride, struct_size)
        _lib.check(self.lib.vaek_mlp3_log_likelihood_replicas(self.h, _ptr(params), C.byref(ll), int(kind), _ptr(A), int(dd), int(did), int(pad),
                                                              float(var_added), int(x_tag), int(z_tag), _addr(workspace), _stream()))

    def supports_mlp3_decoder_jacobian(self):
        """True where mlp3_decoder_jacobian_replicas covers this engine: supports_mlp3_log_likelihood's predicate without the dataset
        kind (the call draws no data rows) -- whatever the engine's batch, world and force_generic are
        (vaek_supports_mlp3_decoder_jacobian)."""
        return self._flag(self.lib.vaek_supports_mlp3_decoder_jacobian)

    @property
    def decoder_jacobian_record_len(self):
        """Doubles of a decoder-Jacobian model record: 2 L + 8 (vaek_decoder_jacobian_record_len)."""
        return self._count(self.lib.vaek_decoder_jacobian_record_len)

    @property
    def decoder_jacobian_row_record_len(self):
        """Doubles of a decoder-Jacobian row record: 2 L + 4 (vaek_decoder_jacobian_row_record_len)."""
        return self._count(self.lib.vaek_decoder_jacobian_row_record_len)

    @property
    def mlp3_decoder_jacobian_max_columns(self):
        """The cap on n * rows * L of one mlp3_decoder_jacobian_replicas call (vaek_mlp3_decoder_jacobian_max_columns)."""
        return int(self.lib.vaek_mlp3_decoder_jacobian_max_columns())

    def mlp3_decoder_jacobian_workspace(self, n, rows):
        """Bytes of the workspace mlp3_decoder_jacobian_replicas needs (its own buffer, 16-byte aligned, not self.workspace)."""
        return self._count(self.lib.vaek_mlp3_decoder_jacobian_workspace_bytes, int(n), int(rows), ctype=C.c_size_t)

    def mlp3_decoder_jacobian_replicas(self, params, rows, out, workspace, z_seeds=None, z_steps=None, z=None, z_stride=None, rank_tol=1e-4,
                                       row_out=None, row_out_stride=None, z_tag=5, n=None, state_stride=None, out_stride=None,
                                       struct_size=None):
        """The spectra of the decoder Jacobian J(z) = d Decoder(z) / dz of EACH of n independent three-hidden-layer MLP VAEs of this
        engine's shape in one call (vaek_mlp3_decoder_jacobian_replicas): per latent row the eigenvalues of J^T J (descending), its
        diagonal and the numerical rank #{lambda_k > rank_tol lambda_1}; model record r = [rows, mean / min / max rank, mean |J|_F^2,
        max sweeps, max off_F / |G|_F, rank_tol, L mean eigenvalues, L mean diagonals] in out[r, :2 L + 8], the row records in
        row_out[r, i, :2 L + 4] where row_out is given.  The latents are the caller's (z: float32 [rows, L] shared by all replicas, or
        [n, rows, L]) or, with z None, the z1 make_batch draws under (z_seeds[r], z_steps[r], z_tag).  params: [n, state_stride] (read
        only), seeds int64 [n], steps int32 [n], out / row_out: float64, workspace: uint8 of mlp3_decoder_jacobian_workspace(n, rows)
        bytes -- all device tensors; n and the strides default to the tensors' shapes.  Three launches whatever n is.  Asynchronous;
        capturable."""
        dj = self._decoder_jacobian_desc(params, rows, out, z_seeds, z_steps, z, z_stride, rank_tol, row_out, row_out_stride, n, state_stride,
                                         out_stride, struct_size)
        _lib.check(self.lib.vaek_mlp3_decoder_jacobian_replicas(self.h, _ptr(params), C.byref(dj), int(z_tag), _addr(workspace), _stream()))

    @staticmethod
    def _decoder_jacobian_desc(params, rows, out, z_seeds, z_steps, z, z_stride, rank_tol, row_out, row_out_stride, n, state_stride, out_stride,
                               struct_size):
        """The vaek_decoder_jacobian both decoder-Jacobian calls take."""
        dj = _describe(_lib.VaekDecoderJacobian(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size,
                       draws=dict(z=(z_seeds, z_steps)), given=("z", z, z_stride))
        assert row_out is None or row_out.dtype == torch.float64
        dj.rank_tol = float(rank_tol)
        dj.row_out = _ptr(row_out)
        if row_out_stride is None:
            row_out_stride = 0 if row_out is None else row_out.shape[-2] * row_out.shape[-1]
        dj.row_out_stride = int(row_out_stride)
        return dj

    def supports_linear_decoder_jacobian(self):
        """True where linear_decoder_jacobian_replicas covers this engine: supports_log_likelihood's predicate without the dataset kind
        (float32, no hidden layers, one or two decoders, D, L <= 32, D <= 28 with two decoders) -- whatever the engine's batch, world and
        force_generic are (vaek_supports_linear_decoder_jacobian)."""
        return self._flag(self.lib.vaek_supports_linear_decoder_jacobian)

    @property
    def linear_decoder_jacobian_max_rows(self):
        """The cap on n * rows of one linear_decoder_jacobian_replicas call (vaek_linear_decoder_jacobian_max_rows)."""
        return int(self.lib.vaek_linear_decoder_jacobian_max_rows())

    def linear_decoder_jacobian_workspace(self, n, rows):
        """Bytes of the workspace linear_decoder_jacobian_replicas needs (its own buffer, 16-byte aligned, not self.workspace)."""
        return self._count(self.lib.vaek_linear_decoder_jacobian_workspace_bytes, int(n), int(rows), ctype=C.c_size_t)

    def linear_decoder_jacobian_replicas(self, params, rows, out, workspace, z_seeds=None, z_steps=None, z=None, z_stride=None, rank_tol=1e-4,
                                         row_out=None, row_out_stride=None, z_tag=5, n=None, state_stride=None, out_stride=None,
                                         struct_size=None):
        """mlp3_decoder_jacobian_replicas for linear VAEs with one or two decoders (vaek_linear_decoder_jacobian_replicas): the same
        records, row modes and arguments, with J(z) = K_d^T + diag(sigmoid'(z K_s + b_s)) K_s^T (one decoder: K_d^T at every z) formed
        and solved in float64; workspace: uint8 of linear_decoder_jacobian_workspace(n, rows) bytes.  Two launches whatever n is.
        Asynchronous; capturable."""
        dj = self._decoder_jacobian_desc(params, rows, out, z_seeds, z_steps, z, z_stride, rank_tol, row_out, row_out_stride, n, state_stride,
                                         out_stride, struct_size)
        _lib.check(self.lib.vaek_linear_decoder_jacobian_replicas(self.h, _ptr(params), C.byref(dj), int(z_tag), _addr(workspace), _stream()))

    def supports_cov_spectrum(self):
        """True where cov_spectrum_rows covers this engine: data_dim <= 32, whatever its architecture, dtype, batch and world are
        (vaek_supports_cov_spectrum)."""
        return self._flag(self.lib.vaek_supports_cov_spectrum)

    @property
    def cov_spectrum_record_len(self):
        """Doubles in one spectrum record (vaek_cov_spectrum_record_len): D^2 + 2 D + 4 = D eigenvalues ascending, D column means, the
        covariance matrix row-major, then sweeps run, final off_F, |C|_F and rows."""
        return self._count(self.lib.vaek_cov_spectrum_record_len)

    @property
    def cov_spectrum_max_sets(self):
        return int(self.lib.vaek_cov_spectrum_max_sets())

    @property
    def cov_spectrum_max_sweeps(self):
        return int(self.lib.vaek_cov_spectrum_max_sweeps())

    def cov_spectrum_rows(self, x, rows, out, n=None, x_stride=None, out_stride=None, _vec=False):
        """The covariance spectrum of EACH of n sets of `rows` float32 rows of D columns in one launch, workgroup s turning set s into
        record s (vaek_cov_spectrum_rows).  x: float32 [n, rows, D] (or [rows, D]: one set), out: float64 [n, out_stride >=
        cov_spectrum_record_len] (or a raw device address) -- device tensors; n and the strides default to the tensors' shapes.  Asynchronous; capturable."""
        assert x is None or x.dtype == torch.float32
        op = _addr(out, torch.float64)
        if n is None:
            n = 1 if x is None or x.dim() < 3 else x.shape[0]
        if x_stride is None:
            x_stride = 0 if x is None or x.dim() < 3 else x.shape[-2] * x.shape[-1]
        fn = self.lib.vaek_cov_eigen_rows if _vec else self.lib.vaek_cov_spectrum_rows
        _lib.check(fn(self.h, _ptr(x), int(n), int(rows), int(x_stride), op, _last_dim(out, out_stride), _stream()))

    @property
    def cov_eigen_record_len(self):
        """Doubles in one eigen record (vaek_cov_eigen_record_len): 2 D^2 + 2 D + 4 = the spectrum record, then V row-major (column k
        the eigenvector of eigenvalue k, its component of largest magnitude positive)."""
        return self._count(self.lib.vaek_cov_eigen_record_len)

    def cov_eigen_rows(self, x, rows, out, n=None, x_stride=None, out_stride=None):
        """cov_spectrum_rows with eigenvectors (vaek_cov_eigen_rows): out is float64 [n, out_stride >= cov_eigen_record_len]; the first
        cov_spectrum_record_len doubles of a record are bitwise cov_spectrum_rows' record.  Asynchronous; capturable."""
        self.cov_spectrum_rows(x, rows, out, n=n, x_stride=x_stride, out_stride=out_stride, _vec=True)

    def subspace_record_len(self, kb):
        """Doubles in one record of subspace_angles (vaek_subspace_record_len): kb + 4."""
        return int(self.lib.vaek_subspace_record_len(int(kb)))

    def subspace_angles(self, a, b, ka, kb, out, n=None, a_stride=None, b_stride=None, out_stride=None):
        """The principal angles between the span of the ka leading eigenvectors of eigen record a[p] and the kb leading ones of b[p],
        1 <= kb <= ka <= D, for each of n pairs in one launch (vaek_subspace_angles).  a, b: float64 [n, stride >=
        cov_eigen_record_len] written by an EARLIER call (or raw device addresses); out: float64 [n, out_stride >= kb + 4]: sin^2
        ascending, |sin Theta|_F^2, sweeps, off_F, the bases' distance from orthonormal.  Asynchronous; capturable."""
        if n is None:
            n = 1 if a is None or isinstance(a, int) or a.dim() < 2 else a.shape[0]
        f64 = torch.float64
        _lib.check(self.lib.vaek_subspace_angles(self.h, _addr(a, f64), _last_dim(a, a_stride), _addr(b, f64), _last_dim(b, b_stride), int(n),
                                                 int(ka), int(kb), _addr(out, f64), _last_dim(out, out_stride), _stream()))

    def supports_spectrum_event(self, kind):
        """True where spectrum_event_replicas covers this engine and dataset kind: exactly where supports_log_likelihood does."""
        return self._flag(self.lib.vaek_supports_spectrum_event, int(kind))

    def spectrum_event_replicas(self, params, rows, kind, A, dd, did, pad, var_added, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out,
                                a_stride=0, x_tag=5, z_tag=6, n=None, state_stride=None, out_stride=None, struct_size=None, _vec=False):
        """The covariance spectra of a generated and of a real batch of EACH of n linear VAEs of this engine's shape in one launch of
        (n, 2) workgroups (vaek_spectrum_event_replicas): `rows` real rows drawn under (x_seeds[r], x_steps[r], x_tag) and `rows`
        latent rows under (z_seeds[r], z_steps[r], z_tag) exactly as make_batch draws them, the fake batch sampled from the latents
        with eps = sample_eps[r].  out: float64 [n, out_stride >= 2 * cov_spectrum_record_len]: the fake record, then the real one.
        The other arguments are stats_event_replicas'.  Asynchronous; capturable."""
        ev = _describe(_lib.VaekSpectrumEvent(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size, a_stride=a_stride,
                       draws=dict(x=(x_seeds, x_steps), z=(z_seeds, z_steps)), raw_out=True)
        assert sample_eps is None or sample_eps.dtype == torch.float32
        ev.sample_eps = _ptr(sample_eps)
        fn = self.lib.vaek_eigen_event_replicas if _vec else self.lib.vaek_spectrum_event_replicas
        _lib.check(fn(self.h, _ptr(params), C.byref(ev), int(kind), _ptr(A), int(dd), int(did), int(pad), float(var_added), int(x_tag),
                      int(z_tag), _stream()))

    def eigen_event_replicas(self, params, rows, kind, A, dd, did, pad, var_added, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, **kw):
        """spectrum_event_replicas with eigenvectors (vaek_eigen_event_replicas): out is float64 [n, out_stride >= 2 *
        cov_eigen_record_len]: the fake eigen record, then the real one.  Asynchronous; capturable."""
        self.spectrum_event_replicas(params, rows, kind, A, dd, did, pad, var_added, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out,
                                     _vec=True, **kw)

    def supports_exact_log_likelihood(self, kind):
        """True where exact_log_likelihood_replicas covers this engine and dataset kind: where supports_log_likelihood does AND the
        model has one decoder (the sigmoid second decoder has no closed form), whatever the engine's batch and world are
        (vaek_supports_exact_log_likelihood)."""
        return self._flag(self.lib.vaek_supports_exact_log_likelihood, int(kind))

    @property
    def exact_log_likelihood_record_len(self):
        """Doubles in one exact log-likelihood record (vaek_exact_log_likelihood_record_len): 10 + D = mean log p(x), mean ELBO, mean
        gap, eps, logdet, sweeps, off_F, |K^T K|_F, the conditioning figure, rows, then the D eigenvalues of K^T K ascending."""
        return self._count(self.lib.vaek_exact_log_likelihood_record_len)

    def exact_log_likelihood_replicas(self, params, rows, out, kind=2, A=None, dd=0, did=0, pad=0, var_added=0.0, x_seeds=None, x_steps=None,
                                      x=None, x_stride=None, a_stride=0, x_tag=3, row_out=None, row_stride=None, n=None, state_stride=None,
                                      out_stride=None, struct_size=None):
        """The exact log-likelihood, exact ELBO and their gap KL(q(z|x) || p(z|x)) of EACH of n one-decoder linear VAEs of this engine's
        shape in one launch, workgroup r evaluating model r (vaek_exact_log_likelihood_replicas): float64 throughout, p(x) = N(b_d, K^T K
        + e^eps I) through the eigenvectors of K^T K.  The rows are the caller's (x: float32 [rows, D] shared by all replicas, or
        [n, rows, D]) or, with x None, drawn under (x_seeds[r], x_steps[r], x_tag) exactly as make_batch draws them.  params:
        [n, state_stride] (read only), out: float64 [n, out_stride >= exact_log_likelihood_record_len], row_out: None or float64
        [n, rows, 2] (log p(x_i), ELBO(x_i)) -- device tensors or raw device addresses; n and the strides default to the tensors'
        shapes.  Asynchronous; capturable."""
        ll = _describe(_lib.VaekExactLogLikelihood(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size,
                       a_stride=a_stride, draws=dict(x=(x_seeds, x_steps)), given=("x", x, x_stride), raw_out=True)
        ll.row_out = _addr(row_out, torch.float64)
        if row_stride is None:
            row_stride = 0 if row_out is None or isinstance(row_out, int) else 2 * int(rows)
        ll.row_stride = int(row_stride)
        _lib.check(self.lib.vaek_exact_log_likelihood_replicas(self.h, _ptr(params), C.byref(ll), int(kind), _ptr(A), int(dd), int(did),
                                                               int(pad), float(var_added), int(x_tag), _stream()))

    def supports_elbo_hessian(self, kind):
        """True where elbo_hvp_replicas and elbo_hessian_lanczos_replicas cover this engine and dataset kind: exactly where
        supports_exact_log_likelihood does (vaek_supports_elbo_hessian)."""
        return self._flag(self.lib.vaek_supports_elbo_hessian, int(kind))

    @property
    def elbo_hvp_max_vectors(self):
        return int(self.lib.vaek_elbo_hvp_max_vectors())

    @property
    def elbo_hvp_record_len(self):
        """Doubles in one record of elbo_hvp_replicas (vaek_elbo_hvp_record_len): 4 = f, |grad f|_2, eps as used, rows."""
        return int(self.lib.vaek_elbo_hvp_record_len())

    @property
    def elbo_hessian_max_steps(self):
        return int(self.lib.vaek_elbo_hessian_max_steps())

    @property
    def elbo_hessian_record_len(self):
        """Doubles in one Lanczos record (vaek_elbo_hessian_record_len): 12 + 4 * 32 = f, |grad f|_2, k, beta_k, sweeps, off_F, |T|_F,
        rows, eps, theta_max, theta_min, omega, then theta ascending, rho, alpha and beta in blocks of 32."""
        return int(self.lib.vaek_elbo_hessian_record_len())

    def elbo_hessian_basis_doubles(self, steps):
        """Doubles of one replica's Lanczos basis (vaek_elbo_hessian_basis_doubles): steps * P."""
        return self._count(self.lib.vaek_elbo_hessian_basis_doubles, int(steps))

    def elbo_hvp_replicas(self, params, rows, out, v=None, hv=None, grad=None, nvec=None, kind=2, A=None, dd=0, did=0, pad=0, var_added=0.0,
                          x_seeds=None, x_steps=None, x=None, x_stride=None, a_stride=0, x_tag=3, n=None, state_stride=None,
                          v_stride=None, hv_stride=None, grad_stride=None, out_stride=None, struct_size=None):
        """Hessian-vector products of f = -mean exact ELBO of EACH of n one-decoder linear VAEs of this engine's shape in one launch
        (vaek_elbo_hvp_replicas): hv[r, i] = H_r v[r, i], float64, flat in the leaf order.  v: float64 [nvec, P] shared by all replicas,
        or [n, nvec, P]; hv: float64 [n, nvec, P]; grad: None or float64 [n, P] (the exact gradient); out: float64 [n, out_stride >= 4] =
        f, |grad f|_2, eps as used, rows.  v = None (nvec = 0): the gradient and the record only.  The rows are the caller's (x) or
        drawn, as in exact_log_likelihood_replicas.  Device tensors or raw device addresses; n, nvec and the strides default to the
        tensors' shapes.  Asynchronous; capturable."""
        hp = _describe(_lib.VaekElboHvp(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size, a_stride=a_stride,
                       draws=dict(x=(x_seeds, x_steps)), given=("x", x, x_stride), raw_out=True)
        f64 = torch.float64
        if nvec is None:
            nvec = 0 if v is None else v.shape[-2]
        hp.nvec = int(nvec)
        hp.v, hp.hv, hp.grad = _addr(v, f64), _addr(hv, f64), _addr(grad, f64)
        if v_stride is None:
            v_stride = 0 if v is None or isinstance(v, int) or v.dim() < 3 else v.shape[-2] * v.shape[-1]
        if hv_stride is None:
            hv_stride = 0 if hv is None or isinstance(hv, int) else hv.shape[-2] * hv.shape[-1]
        hp.v_stride, hp.hv_stride = int(v_stride), int(hv_stride)
        hp.grad_stride = _last_dim(grad, grad_stride)
        _lib.check(self.lib.vaek_elbo_hvp_replicas(self.h, _ptr(params), C.byref(hp), int(kind), _ptr(A), int(dd), int(did), int(pad),
                                                   float(var_added), int(x_tag), _stream()))

    def elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, kind=2, A=None, dd=0, did=0, pad=0, var_added=0.0,
                                      x_seeds=None, x_steps=None, x=None, x_stride=None, a_stride=0, x_tag=3, n=None, state_stride=None,
                                      v0_stride=None, basis_stride=None, out_stride=None, struct_size=None):
        """`steps` <= 32 Lanczos steps with full reorthogonalisation on the Hessian of f = -mean exact ELBO of EACH of n one-decoder
        linear VAEs of this engine's shape in one launch (vaek_elbo_hessian_lanczos_replicas).  v0: float64 [P] shared by all replicas,
        or [n, P]: the start vector; basis: float64 [n, steps, P]: the Lanczos vectors, an output (rows >= k are not written); out:
        float64 [n, out_stride >= elbo_hessian_record_len]: f, |grad f|_2, k, beta_k, sweeps, off_F, |T|_F, rows, eps, theta_max,
        theta_min, omega, then the Ritz values ascending, their residual bounds, alpha and beta.  The rows are the caller's (x) or drawn,
        as in exact_log_likelihood_replicas.  Device tensors or raw device addresses; n and the strides default to the tensors' shapes.
        Asynchronous; capturable."""
        hs = _describe(_lib.VaekElboHessian(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size, a_stride=a_stride,
                       draws=dict(x=(x_seeds, x_steps)), given=("x", x, x_stride), raw_out=True)
        f64 = torch.float64
        hs.steps = int(steps)
        hs.v0, hs.basis = _addr(v0, f64), _addr(basis, f64)
        if v0_stride is None:
            v0_stride = 0 if v0 is None or isinstance(v0, int) or v0.dim() < 2 else v0.shape[-1]
        if basis_stride is None:
            basis_stride = 0 if basis is None or isinstance(basis, int) else basis.shape[-2] * basis.shape[-1]
        hs.v0_stride, hs.basis_stride = int(v0_stride), int(basis_stride)
        _lib.check(self.lib.vaek_elbo_hessian_lanczos_replicas(self.h, _ptr(params), C.byref(hs), int(kind), _ptr(A), int(dd), int(did),
                                                               int(pad), float(var_added), int(x_tag), _stream()))

    def supports_sampled_elbo_hessian(self, kind):
        """True where sampled_elbo_hvp_replicas and sampled_elbo_hessian_lanczos_replicas cover this engine and dataset kind: exactly
        where supports_log_likelihood does -- one OR two decoders (vaek_supports_sampled_elbo_hessian)."""
        return self._flag(self.lib.vaek_supports_sampled_elbo_hessian, int(kind))

    @property
    def sampled_elbo_hessian_max_columns(self):
        """The cap on n * rows * samples of one sampled-Hessian call (vaek_sampled_elbo_hessian_max_columns); rows * samples of one
        replica is at most 2^16 besides."""
        return int(self.lib.vaek_sampled_elbo_hessian_max_columns())

    @property
    def sampled_elbo_hessian_record_len(self):
        """Doubles in one sampled Lanczos record (vaek_sampled_elbo_hessian_record_len): the 140 of elbo_hessian_record_len, then K and
        1.0 with two decoders."""
        return int(self.lib.vaek_sampled_elbo_hessian_record_len())

    def sampled_elbo_hessian_workspace(self, n, rows, samples):
        """Bytes of the workspace the two sampled-Hessian calls need (their own buffer, 16-byte aligned, not self.workspace)."""
        return self._count(self.lib.vaek_sampled_elbo_hessian_workspace_bytes, int(n), int(rows), int(samples), ctype=C.c_size_t)

    @staticmethod
    def _describe_samples(d, rows, samples, xi, xi_stride, z_seeds, z_steps):
        """The fields the sampled descriptions add: samples (default: xi's), the explicit samples xi (float32 [rows, K, L] shared by all
        replicas, or [n, rows, K, L]) or the streams that draw them."""
        assert xi is None or xi.dtype == torch.float32
        if samples is None:
            samples = xi.shape[-2]
        d.samples = int(samples)
        d.xi = _ptr(xi)
        if xi_stride is None:
            xi_stride = 0 if xi is None or xi.dim() < 4 else xi.shape[-3] * xi.shape[-2] * xi.shape[-1]
        d.xi_stride = int(xi_stride)
        assert z_seeds is None or z_seeds.dtype == torch.int64
        assert z_steps is None or z_steps.dtype == torch.int32
        d.z_seeds, d.z_steps = _ptr(z_seeds), _ptr(z_steps)

    def sampled_elbo_hvp_replicas(self, params, rows, out, workspace, samples=None, v=None, hv=None, grad=None, nvec=None, kind=2, A=None,
                                  dd=0, did=0, pad=0, var_added=0.0, x_seeds=None, x_steps=None, x=None, x_stride=None, z_seeds=None,
                                  z_steps=None, xi=None, xi_stride=None, a_stride=0, x_tag=11, z_tag=12, n=None, state_stride=None,
                                  v_stride=None, hv_stride=None, grad_stride=None, out_stride=None, struct_size=None, _fn=None):
        """Hessian-vector products of the SAMPLE-AVERAGE ELBO f_K of EACH of n linear VAEs (one or two decoders) of this engine's shape
        (vaek_sampled_elbo_hvp_replicas): elbo_hvp_replicas' arguments and outputs on `rows` data rows with `samples` latent samples
        each -- xi: float32 [rows, K, L] shared or [n, rows, K, L], or None: drawn by the block rule under (z_seeds[r], z_steps[r],
        z_tag), sample 0 being make_batch's z1.  workspace: uint8 of sampled_elbo_hessian_workspace(n, rows, samples) bytes.  2 + 2 nvec
        launches.  Asynchronous; capturable."""
        hp = _describe(_lib.VaekSampledElboHvp(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size,
                       a_stride=a_stride, draws=dict(x=(x_seeds, x_steps)), given=("x", x, x_stride), raw_out=True)
        self._describe_samples(hp, rows, samples, xi, xi_stride, z_seeds, z_steps)
        f64 = torch.float64
        if nvec is None:
            nvec = 0 if v is None else v.shape[-2]
        hp.nvec = int(nvec)
        hp.v, hp.hv, hp.grad = _addr(v, f64), _addr(hv, f64), _addr(grad, f64)
        if v_stride is None:
            v_stride = 0 if v is None or isinstance(v, int) or v.dim() < 3 else v.shape[-2] * v.shape[-1]
        if hv_stride is None:
            hv_stride = 0 if hv is None or isinstance(hv, int) else hv.shape[-2] * hv.shape[-1]
        hp.v_stride, hp.hv_stride = int(v_stride), int(hv_stride)
        hp.grad_stride = _last_dim(grad, grad_stride)
        fn = _fn or self.lib.vaek_sampled_elbo_hvp_replicas            # _fn: the MLP call of the same description (below)
        _lib.check(fn(self.h, _ptr(params), C.byref(hp), int(kind), _ptr(A), int(dd), int(did), int(pad), float(var_added), int(x_tag),
                      int(z_tag), _addr(workspace), _stream()))

    def sampled_elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, workspace, samples=None, kind=2, A=None, dd=0, did=0,
                                              pad=0, var_added=0.0, x_seeds=None, x_steps=None, x=None, x_stride=None, z_seeds=None,
                                              z_steps=None, xi=None, xi_stride=None, a_stride=0, x_tag=11, z_tag=12, n=None,
                                              state_stride=None, v0_stride=None, basis_stride=None, out_stride=None, struct_size=None,
                                              _fn=None):
        """`steps` <= 32 Lanczos steps with full reorthogonalisation on the Hessian of the SAMPLE-AVERAGE ELBO f_K of EACH of n linear
        VAEs (one or two decoders) of this engine's shape (vaek_sampled_elbo_hessian_lanczos_replicas): elbo_hessian_lanczos_replicas'
        arguments and outputs with the samples of sampled_elbo_hvp_replicas; out: float64 [n, out_stride >=
        sampled_elbo_hessian_record_len].  3 + 2 steps launches, the recursion across them.  Asynchronous; capturable."""
        hs = _describe(_lib.VaekSampledElboHessian(), params, rows, out, torch.float64, n, state_stride, out_stride, struct_size,
                       a_stride=a_stride, draws=dict(x=(x_seeds, x_steps)), given=("x", x, x_stride), raw_out=True)
        self._describe_samples(hs, rows, samples, xi, xi_stride, z_seeds, z_steps)
        f64 = torch.float64
        hs.steps = int(steps)
        hs.v0, hs.basis = _addr(v0, f64), _addr(basis, f64)
        if v0_stride is None:
            v0_stride = 0 if v0 is None or isinstance(v0, int) or v0.dim() < 2 else v0.shape[-1]
        if basis_stride is None:
            basis_stride = 0 if basis is None or isinstance(basis, int) else basis.shape[-2] * basis.shape[-1]
        hs.v0_stride, hs.basis_stride = int(v0_stride), int(basis_stride)
        fn = _fn or self.lib.vaek_sampled_elbo_hessian_lanczos_replicas
        _lib.check(fn(self.h, _ptr(params), C.byref(hs), int(kind), _ptr(A), int(dd), int(did), int(pad), float(var_added), int(x_tag),
                      int(z_tag), _addr(workspace), _stream()))

    def supports_mlp3_sampled_elbo_hessian(self, kind):
        """True where mlp3_sampled_elbo_hvp_replicas and mlp3_sampled_elbo_hessian_lanczos_replicas cover this engine and dataset kind:
        exactly where supports_mlp3_log_likelihood does (vaek_supports_mlp3_sampled_elbo_hessian)."""
        return self._flag(self.lib.vaek_supports_mlp3_sampled_elbo_hessian, int(kind))

    @property
    def mlp3_sampled_elbo_hessian_max_columns(self):
        """The cap on n * rows * samples of one MLP sampled-Hessian call (vaek_mlp3_sampled_elbo_hessian_max_columns) = 2^14; rows *
        samples of one replica is at most 2^13 besides."""
        return int(self.lib.vaek_mlp3_sampled_elbo_hessian_max_columns())

    def mlp3_sampled_elbo_hessian_workspace(self, n, rows, samples):
        """Bytes of the workspace the two MLP sampled-Hessian calls need (their own buffer, 16-byte aligned, not self.workspace)."""
        return self._count(self.lib.vaek_mlp3_sampled_elbo_hessian_workspace_bytes, int(n), int(rows), int(samples), ctype=C.c_size_t)

    def mlp3_sampled_elbo_hvp_replicas(self, params, rows, out, workspace, samples=None, x_tag=14, z_tag=15, **kw):
        """sampled_elbo_hvp_replicas for n three-hidden-layer MLP VAEs of this engine's shape (vaek_mlp3_sampled_elbo_hvp_replicas): the
        same arguments, description and outputs; workspace: uint8 of mlp3_sampled_elbo_hessian_workspace(n, rows, samples) bytes.
        3 + 2 nvec launches.  Asynchronous; capturable."""
        self.sampled_elbo_hvp_replicas(params, rows, out, workspace, samples=samples, x_tag=x_tag, z_tag=z_tag,
                                       _fn=self.lib.vaek_mlp3_sampled_elbo_hvp_replicas, **kw)

    def mlp3_sampled_elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, workspace, samples=None, x_tag=14, z_tag=15,
                                                   **kw):
        """sampled_elbo_hessian_lanczos_replicas for n three-hidden-layer MLP VAEs of this engine's shape
        (vaek_mlp3_sampled_elbo_hessian_lanczos_replicas): the same arguments, description and 142-double record.  6 + 6 steps launches,
        every vector operation spread over chunks of P.  Asynchronous; capturable."""
        self.sampled_elbo_hessian_lanczos_replicas(params, rows, steps, v0, basis, out, workspace, samples=samples, x_tag=x_tag, z_tag=z_tag,
                                                   _fn=self.lib.vaek_mlp3_sampled_elbo_hessian_lanczos_replicas, **kw)

    def supports_train_step_replicas(self):
        """True where train_step_gen_replicas covers this engine: the step path is "mlp3" and world == 1."""
        return self._flag(self.lib.vaek_supports_train_step_replicas)

    @property
    def train_step_max_replicas(self):
        return int(self.lib.vaek_train_step_max_replicas())

    def train_step_replicas_workspace(self, n):
        """Bytes of the workspace Engine.train_step_gen_replicas needs for n replicas (its own buffer, not self.workspace): n times
        the mlp3 step's region of stored activations."""
        return self._count(self.lib.vaek_train_step_replicas_workspace_bytes, int(n), ctype=C.c_size_t)

    def train_step_gen_replicas(self, params, grads, m, v, step_dev, cur, lr, kind, A, dd, did, pad, var_added, nxt, seeds, counter,
                                which, lrs=None, a_stride=0, loss_hist=None, workspace=None, tag=0, row0=0, n=None, state_stride=None,
                                grads_stride=None, loss_hist_cap=None):
        """ONE train step of EACH of n independent three-hidden-layer MLP VAEs of this engine's shape, two launches whatever n is
        (vaek_train_step_gen_replicas): replica r trains on cur = (x [n, B, D], z1 [n, B, L], z2 [n, B, D])[r] and draws its next
        batch into nxt[r] (generator step counter[r, which]; counter[r, which ^ 1] = step + 1 is stored; counter: int32 [n, 2]).
        nxt = None: nothing is drawn (n x train_step; seeds, A and counter may be None).  params / m / v: [n, state_stride] with
        state_stride a multiple of 4, grads: [n, grads_stride], step_dev: int32 [n], seeds: int64 [n], lrs: float32 [n] or None
        (then `lr` for all), A: replica r's at A + r * a_stride floats (0: shared), loss_hist: [n, cap] or None, workspace: uint8 of
        train_step_replicas_workspace(n) bytes -- all device tensors; n, the strides and cap default to the tensors' shapes.
        Replica r ends bitwise where train_step_gen alone on its slices would.  Asynchronous; capturable."""
        assert counter is None or (counter.dtype == torch.int32 and counter.is_cuda)
        rep = self._replicas_desc(params, grads, seeds, lrs, a_stride, loss_hist, n, state_stride, grads_stride, loss_hist_cap)
        nxt = (None, None, None) if nxt is None else nxt
        _lib.check(self.lib.vaek_train_step_gen_replicas(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), C.byref(rep),
                                                         _ptr(cur[0]), _ptr(cur[1]), _ptr(cur[2]), float(lr), _ptr(workspace), int(kind),
                                                         _ptr(A), int(dd), int(did), int(pad), float(var_added), _ptr(nxt[0]), _ptr(nxt[1]),
                                                         _ptr(nxt[2]), int(row0), _ptr(counter), int(which), int(tag), _stream()))

    def plan_train_steps(self, params, grads, m, v, step_dev, batches, lr):
        """The same call with its arguments marshalled once: returns a function that issues vaek_train_steps on these buffers
        again (the pointer arrays, not the data, are frozen) -- for loops that repeat a group of steps, where building three
        ctypes arrays per call would cost more host time than the launch."""
        n = len(batches)
        for b in batches:
            assert all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in b)
        arr = lambda k: (C.c_void_p * n)(*[C.c_void_p(b[k].data_ptr()) for b in batches])
        keep = (params, grads, m, v, step_dev, list(batches))                     # the plan keeps its tensors alive
        args = (self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), arr(0), arr(1), arr(2), n, C.c_float(lr), _ptr(self.workspace))
        fn, check = self.lib.vaek_train_steps, _lib.check

        def run(_keep=keep):
            check(fn(*args, _stream()))
        return run

    def moment_len(self):
        """doubles in the second-moment image of a batch (0: the moment form does not cover this model)."""
        return self._moment_len

    def moments(self, x, z1, z2, M):
        """M (float64 device tensor of moment_len()) <- the second-moment image of this rank's batch shard (vaek_train_steps_moments)."""
        assert M.dtype == torch.float64 and M.numel() >= self.moment_len()
        _lib.check(self.lib.vaek_train_steps_moments(self.h, _ptr(x), _ptr(z1), _ptr(z2), _ptr(M), _ptr(self.workspace), _stream()))

    def moments_update(self, params, grads, m, v, step_dev, M, lr):
        """loss, gradients, Adam from the (globally summed) moment image (vaek_train_steps_update)."""
        _lib.check(self.lib.vaek_train_steps_update(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(step_dev), _ptr(M), float(lr),
                                                    _ptr(self.workspace), _stream()))

    def train_steps_gave_up(self):
        """Synchronous: True if a bounded wait inside vaek_train_steps' persistent launch ever expired."""
        f = C.c_int32()
        _lib.check(self.lib.vaek_train_steps_status(self.h, _ptr(self.workspace), C.byref(f)))
        self.train_steps_status_word = f.value & 0xffffffff
        return f.value != 0

    def grads_only(self, params, grads, step_dev, x, z1, z2):
        _lib.check(self.lib.vaek_train_step_grads_only(self.h, _ptr(params), _ptr(grads), _ptr(step_dev), _ptr(x),
                                                       _ptr(z1), _ptr(z2), _ptr(self.workspace), _stream()))

    def buckets(self):
        """[(offset, count)] of the gradient buckets in the order the backward pass completes them."""
        n = C.c_int32()
        _lib.check(self.lib.vaek_bucket_count(self.h, C.byref(n)))
        out = []
        for i in range(n.value):
            off, cnt = C.c_int64(), C.c_int64()
            _lib.check(self.lib.vaek_bucket_info(self.h, i, C.byref(off), C.byref(cnt)))
            out.append((off.value, cnt.value))
        return out

    def grads_bucketed(self, params, grads, step_dev, x, z1, z2, events):
        """Like grads_only, but records events[i] (torch.cuda.Event, already created on this device) the moment
        bucket i of `grads` is final."""
        arr = (C.c_void_p * len(events))(*[C.c_void_p(e.cuda_event) for e in events])
        _lib.check(self.lib.vaek_train_step_grads_bucketed(self.h, _ptr(params), _ptr(grads), _ptr(step_dev), _ptr(x), _ptr(z1),
                                                           _ptr(z2), arr, _ptr(self.workspace), _stream()))

    def apply(self, params, grads, m, v, step_dev, lr):
        _lib.check(self.lib.vaek_train_step_apply(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v),
                                                  _ptr(step_dev), float(lr), _stream()))

    def loss_eval(self, params, x, z1, z2):
        out = torch.empty(4, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.vaek_loss_eval(self.h, _ptr(params), _ptr(x), _ptr(z1), _ptr(z2), _ptr(out),
                                           _ptr(self.workspace), _stream()))
        return out

    def forward(self, params, x, z1, z2, sampling=False, eps=0.0, want_mu=True):
        rows = z1.shape[0]
        x_hat = torch.empty(rows, self.D, dtype=torch.float32, device=self.device)
        mu = torch.empty(rows, self.L, dtype=torch.float32, device=self.device) if want_mu else None
        _lib.check(self.lib.vaek_forward(self.h, _ptr(params), _ptr(x), _ptr(z1), _ptr(z2), int(bool(sampling)),
                                         float(eps), _ptr(x_hat), _ptr(mu), rows, _ptr(self.workspace), _stream()))
        return x_hat, mu

    # ---- on-device inputs (K7) and the loss ring ------------------------------------------------
    def make_batch(self, kind, A, dd, did, pad, var_added, rows, seed, step_dev=None, step=0, tag=0, row0=0,
                   want_x=True, want_z=True, out=None, counter=None, which=0):
        """x[rows,D] (or None), z1[rows,L], z2[rows,D] drawn by libvaek's Philox kernel.  With `counter` (device
        int32[2]) the step is counter[which] and the kernel stores counter[which ^ 1] = step + 1 (vaek_make_batch_next)."""
        if out is None:
            Dx = dd + pad + (1 if kind == 1 else 0)
            x = torch.empty(rows, Dx, dtype=torch.float32, device=self.device) if want_x else None
            z1 = torch.empty(rows, self.L, dtype=torch.float32, device=self.device) if want_z else None
            z2 = torch.empty(rows, self.D, dtype=torch.float32, device=self.device) if want_z else None
        else:
            x, z1, z2 = out
        if counter is not None:
            assert counter.dtype == torch.int32 and counter.numel() == 2 and counter.is_cuda
            _lib.check(self.lib.vaek_make_batch_next(self.h, int(kind), _ptr(A), int(dd), int(did), int(pad), float(var_added),
                                                     _ptr(x), _ptr(z1), _ptr(z2), int(rows), int(row0),
                                                     int(seed) & (2**64 - 1), _ptr(counter), int(which), int(tag), _stream()))
            return x, z1, z2
        _lib.check(self.lib.vaek_make_batch(self.h, int(kind), _ptr(A), int(dd), int(did), int(pad), float(var_added),
                                            _ptr(x), _ptr(z1), _ptr(z2), int(rows), int(row0), int(seed) & (2**64 - 1),
                                            _ptr(step_dev), int(step), int(tag), _stream()))
        return x, z1, z2

    def rng_fill(self, n, seed, step=0, tag=0, bits=False, normals=True):
        """n normals of the raw stream (vaek_rng_fill: block b under counter (b lo, b hi, step, tag)), with bits=True also the
        Philox words they were formed from; normals=False gives the words alone."""
        out_n = torch.empty(n, dtype=torch.float32, device=self.device) if normals else None
        out_u = torch.empty(n, dtype=torch.int32, device=self.device) if bits else None
        _lib.check(self.lib.vaek_rng_fill(self.h, _ptr(out_n), _ptr(out_u), int(n), int(seed) & (2**64 - 1), int(step),
                                          int(tag), _stream()))
        return (out_n, out_u) if bits and normals else (out_n if normals else out_u)

    def set_loss_history(self, buf):
        self._loss_hist = buf                      # keep it alive
        _lib.check(self.lib.vaek_set_loss_history(self.h, _ptr(buf), 0 if buf is None else buf.numel()))

    # ---- in-process kernel timing (bench.py) ------------------------------------------------
    def profile_begin(self, max_records=4096):
        _lib.check(self.lib.vaek_profile_begin(self.h, int(max_records)))

    def profile_report(self):
        import json
        buf = C.create_string_buffer(8192)
        _lib.check(self.lib.vaek_profile_report(self.h, buf, 8192))
        return json.loads(buf.value.decode())

    def measure_peaks(self, copy_bytes=1 << 30, reps=5):
        """Achievable HBM bandwidth (float4 stream copy, read + write bytes) and f32 / bf16 MFMA rates measured on
        this device with the library's own micro-benchmarks."""
        src = torch.empty(copy_bytes, dtype=torch.uint8, device=self.device).random_(0, 255)
        dst = torch.empty_like(src)
        scratch = torch.zeros(16, dtype=torch.float32, device=self.device)
        flops = C.c_double()
        st = _stream()
        plan = [("microbench_mfma_f32", 0, 20000, 1), ("microbench_mfma_bf16", 1, 40000, 1)]     # ~1 ms each, one wave per SIMD
        for _ in range(2):                                   # warm-up
            _lib.check(self.lib.vaek_microbench_copy(self.h, _ptr(src), _ptr(dst), copy_bytes, st))
            for _, kind, iters, wps in plan:
                _lib.check(self.lib.vaek_microbench_mfma(self.h, kind, iters, wps, _ptr(scratch), C.byref(flops), st))
        torch.cuda.synchronize()
        self.profile_begin(64)
        fl = {}
        for _ in range(reps):
            _lib.check(self.lib.vaek_microbench_copy(self.h, _ptr(src), _ptr(dst), copy_bytes, st))
            for name, kind, iters, wps in plan:
                _lib.check(self.lib.vaek_microbench_mfma(self.h, kind, iters, wps, _ptr(scratch), C.byref(flops), st))
                fl[name] = flops.value
        torch.cuda.synchronize()
        rep = self.profile_report()
        out = {"hbm_copy_GBps": 2.0 * copy_bytes * rep["microbench_stream_copy"]["count"] / (rep["microbench_stream_copy"]["total_ms"] * 1e-3) / 1e9}
        for name, _, _, _ in plan:
            out[name.replace("microbench_", "") + "_TFLOPs"] = fl[name] * rep[name]["count"] / (rep[name]["total_ms"] * 1e-3) / 1e12
        return out

    def measure_launch_floor(self, n=100, reps=20):
        """Launch-to-launch interval (us) of a kernel that does nothing, replayed from a hipGraph chain of n launches:
        what any two-kernel step pays before it computes anything."""
        import time
        launch = lambda k: _lib.check(self.lib.vaek_microbench_launch(self.h, 0, 1, k, None, None, _stream()))
        launch(4)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                launch(n)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            g.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (n * reps) * 1e6

    # ---- building blocks -----------------------------------------------------------------------
    def dense_fwd(self, x, w, b, relu=False):
        rows, n_in = x.shape
        n_out = w.shape[1]
        y = torch.empty(rows, n_out, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.vaek_dense_fwd(self.h, _ptr(x), _ptr(w), _ptr(b), _ptr(y), rows, n_in, n_out,
                                           int(relu), _stream()))
        return y

    def dense_fwd_reparam(self, x, w, b, z1, logvar_e):
        """mu = x @ w + b, samples = mu + exp(logvar_e / 2) * z1 (networks.py:72-74) in one block."""
        rows, n_in = x.shape
        n_out = w.shape[1]
        mu = torch.empty(rows, n_out, dtype=torch.float32, device=self.device)
        samples = torch.empty_like(mu)
        _lib.check(self.lib.vaek_dense_fwd_reparam(self.h, _ptr(x), _ptr(w), _ptr(b), _ptr(mu), _ptr(samples), _ptr(z1), _ptr(logvar_e),
                                                   rows, n_in, n_out, _stream()))
        return mu, samples

    def reparam_bwd(self, d_samples, mu, z1, logvar_e, batch_total=0, out=None):
        """In place d_samples -> d_mu; returns d logvar_e (reparameterisation + KL parts)."""
        rows, L = mu.shape
        g = torch.empty(L, dtype=torch.float32, device=self.device) if out is None else out
        _lib.check(self.lib.vaek_reparam_bwd(self.h, _ptr(d_samples), _ptr(mu), _ptr(z1), _ptr(logvar_e), _ptr(g), rows, L,
                                             int(batch_total), _ptr(self.workspace), _stream()))
        return g

    def dense_bwd_dx(self, dy, w, x_post=None, relu=False, out=None, accumulate=False):
        rows, n_out = dy.shape
        n_in = w.shape[0]
        dx = torch.empty(rows, n_in, dtype=torch.float32, device=self.device) if out is None else out
        _lib.check(self.lib.vaek_dense_bwd_dx(self.h, _ptr(dy), _ptr(w), _ptr(x_post), _ptr(dx), rows, n_in, n_out,
                                              int(relu), int(accumulate), _stream()))
        return dx

    def dense_bwd_dw(self, x, dy):
        rows, n_in = x.shape
        n_out = dy.shape[1]
        dwb = torch.empty(n_in + 1, n_out, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.vaek_dense_bwd_dw(self.h, _ptr(x), _ptr(dy), _ptr(dwb), rows, n_in, n_out,
                                              _ptr(self.workspace), _stream()))
        return dwb

    def elbo_fwd_bwd(self, x, x_hat_lin, x_hat_sig, z2, mu, logvar_e, eps, batch_total=0, grads=True, eps_param=None):
        """eps_param (a one-element device tensor): eps = eps_param[0] * eps, read on the device (vaek_elbo_fwd_bwd_dev)."""
        rows, D = x.shape
        L = mu.shape[1]
        out4 = torch.empty(4, dtype=torch.float32, device=self.device)
        d_lin = torch.empty_like(x_hat_lin) if grads else None
        d_sig = torch.empty_like(x_hat_sig) if (grads and x_hat_sig is not None) else None
        if eps_param is not None:
            _lib.check(self.lib.vaek_elbo_fwd_bwd_dev(self.h, _ptr(x), _ptr(x_hat_lin), _ptr(x_hat_sig), _ptr(z2), _ptr(mu),
                                                      _ptr(logvar_e), _ptr(eps_param), float(eps), _ptr(d_lin), _ptr(d_sig), _ptr(out4),
                                                      rows, D, L, int(batch_total), _ptr(self.workspace), _stream()))
        else:
            _lib.check(self.lib.vaek_elbo_fwd_bwd(self.h, _ptr(x), _ptr(x_hat_lin), _ptr(x_hat_sig), _ptr(z2), _ptr(mu),
                                                  _ptr(logvar_e), float(eps), _ptr(d_lin), _ptr(d_sig), _ptr(out4),
                                                  rows, D, L, int(batch_total), _ptr(self.workspace), _stream()))
        return out4, d_lin, d_sig

    def adam_step(self, params, grads, m, v, lr, step=None, step_dev=None, grad_scale=1.0):
        _lib.check(self.lib.vaek_adam_step(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(),
                                           float(lr), int(step or 0), _ptr(step_dev), float(grad_scale), _stream()))
