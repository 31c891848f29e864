"""The observables evaluated at the n_print events, as ONE table: run.py's refusals and banners, the sweep's event runner
(run.main_sweep), GenerativeModel._stats_event and write_stats all read OBSERVABLES; none of them names an observable.

An Observable is one event (events.py: one device call for all models) behind one or two Flags:
  flags      each with its own NEEDS text, refusals and banners (Flag, below);
  events     (dest, cache, class) rows: the first whose `dest` is set picks the event class and the attribute the object is kept
             under (on the model, or on the sweep's settings) -- built on first use, then reused;
  covered    (eng, kind) -> bool: the engine's coverage predicate;
  build      (class, models, cfg) -> the event object; cfg carries the attributes the flags set;
  run        (event, ran, cfg) -> one stats dict per model.  `ran` maps every observable that already ran at this step to what it
             returned: the couplings between events are written here and nowhere else;
  array_keys (class) -> the keys that are arrays whatever their length: write_stats keeps them off the stats line;
  line       (key, label): what it shows instead -- element 0 of that key's array, under `key label`.
A Flag is the option and its argparse `dest` (also the attribute main() sets on a single model), `needs` (about_dim: the refusal
quotes the model's data_dim, not its step path; linear_hint: the refusal of a linear model), `extra(flag, m, eng, value, n_models,
path)` for further refusals (what it returns goes to `attrs`), `attrs(args, value, checked)` -> the attributes it sets (default
{dest: value}), the banners of a single model (m) and of a sweep (event, n_models, cfg), and save_flag: model_save_data reads it.

OBSERVABLES holds the seven flags tests/test_observables_host.py pins by equality; an observable added since stands in
LATER_OBSERVABLES with the name of the entry it follows, and TABLE is the two merged.  tests/test_sampled_hessian_host.py in turn pins
len(TABLE) == len(OBSERVABLES) + 1 and the row of sampled_elbo_hessian, so those three stay exactly as they are: what came after
(--mlp_sampled_elbo_hessian) stands in MLP_OBSERVABLES, again with the name of the entry it follows, and ALL_OBSERVABLES is the two
merged.  tests/test_mlp3_hessian_host.py pins len(ALL_OBSERVABLES) == len(TABLE) + 1, so the next one (--linear_decoder_jacobian)
stands in LINEAR_OBSERVABLES by the same pattern and EVERY_OBSERVABLE is the merged whole: everything below reads EVERY_OBSERVABLE.

The table's order is the order the results are merged into the stats dict -- the stats line and the keys of losses.npz -- and the
order both callers issue the device calls in.  Every event draws under its own counter and tags (events.py), so the order of the
calls changes no result: each record is bitwise what the event alone would give.  To add an observable: one entry here, its event
class in events.py, its binding in engine.py.  Nothing here imports torch before an event is built: run.py's parser stays cheap."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional


def _events():
    from . import events
    return events


@dataclass(frozen=True)
class Flag:
    flag: str
    dest: str
    needs: str
    banner_one: Callable
    banner_sweep: Callable
    about_dim: bool = False
    linear_hint: Optional[str] = None
    extra: Optional[Callable] = None
    attrs: Optional[Callable] = None
    save_flag: bool = False

    def value(self, args):
        """The flag's value in `args`, None where it was not given."""
        v = getattr(args, self.dest, None)
        return None if v is None or v is False else v


@dataclass(frozen=True)
class Observable:
    flags: tuple
    events: tuple
    covered: Callable
    build: Callable
    run: Callable
    array_keys: Callable = lambda cls: ()
    line: Optional[tuple] = None

    @property
    def name(self):
        return self.flags[0].dest

    def event_class(self, row=0):
        return getattr(_events(), self.events[row][2])


JACOBIAN_DEFAULT_TOL = 1e-4


def decoder_jacobian_tol(args):
    """The rank threshold of --decoder_jacobian: --decoder_jacobian_tol, else 1e-4."""
    tol = getattr(args, "decoder_jacobian_tol", None)
    return JACOBIAN_DEFAULT_TOL if tol is None else float(tol)


# ---- further refusals ---------------------------------------------------------------------------------------------------------
def _sample_cap(fl, m, eng, samples, n_models, path):
    if samples > eng.log_likelihood_max_samples:
        raise RuntimeError(f"{fl.flag} {samples}: at most {eng.log_likelihood_max_samples} samples per row fit one call "
                           "(vaek_log_likelihood_max_samples)")


def _mlp_sample_and_column_caps(fl, m, eng, samples, n_models, path):
    if samples > eng.log_likelihood_max_samples:
        raise RuntimeError(f"{fl.flag} {samples}: at most {eng.log_likelihood_max_samples} samples per row fit one call "
                           f"(vaek_log_likelihood_max_samples; this model's step path: {path})")
    cols = n_models * m.print_batch_size * samples
    if cols > eng.mlp3_log_likelihood_max_columns:
        raise RuntimeError(f"{fl.flag} {samples}: {n_models} models x {m.print_batch_size} rows x {samples} samples = {cols} "
                           f"columns, at most {eng.mlp3_log_likelihood_max_columns} fit one call (vaek_mlp3_log_likelihood_max_columns; this "
                           f"model's step path: {path})")


def _jacobian_column_cap(fl, m, eng, at, n_models, path):
    cols = n_models * m.print_batch_size * eng.L
    if cols > eng.mlp3_decoder_jacobian_max_columns:
        raise RuntimeError(f"{fl.flag}: {n_models} models x {m.print_batch_size} rows x {eng.L} latents = {cols} columns, at most "
                           f"{eng.mlp3_decoder_jacobian_max_columns} fit one call (vaek_mlp3_decoder_jacobian_max_columns; this model's "
                           f"step path: {path})")


SAMPLED_HESSIAN_DEFAULT_SAMPLES = 8


def sampled_elbo_hessian_samples(args):
    """K of --sampled_elbo_hessian: --sampled_elbo_hessian_samples, else 8."""
    k = getattr(args, "sampled_elbo_hessian_samples", None)
    return SAMPLED_HESSIAN_DEFAULT_SAMPLES if k is None else int(k)


def _sampled_caps(fl, m, eng, steps, n_models, path):
    """What the refusal of K needs, for _sampled_attrs (which sees the arguments)."""
    return dict(flag=fl.flag, n=n_models, rows=m.print_batch_size, max_samples=eng.log_likelihood_max_samples,
                max_columns=eng.sampled_elbo_hessian_max_columns, path=path)


def _sampled_attrs(args, steps, caps):
    samples = sampled_elbo_hessian_samples(args)
    if caps is not None:
        if samples > caps["max_samples"]:
            raise RuntimeError(f"{caps['flag']}_samples {samples}: at most {caps['max_samples']} samples per row fit one call "
                               f"(vaek_log_likelihood_max_samples; this model's step path: {caps['path']})")
        cols = caps["n"] * caps["rows"] * samples
        if cols > caps["max_columns"] or caps["rows"] * samples > 1 << 16:
            raise RuntimeError(f"{caps['flag']}_samples {samples}: {caps['n']} models x {caps['rows']} rows x {samples} samples = {cols} "
                               f"columns, at most {caps['max_columns']} fit one call and {1 << 16} one model "
                               f"(vaek_sampled_elbo_hessian_max_columns; this model's step path: {caps['path']})")
    return {"sampled_elbo_hessian": steps, "sampled_elbo_hessian_samples": samples}


def _subspace_k(fl, m, eng, k, n_models, path):
    """K of --subspace (None: auto), refused outside 1 .. data_dim."""
    k = None if k == "auto" else int(k)
    if k is not None and not 1 <= k <= eng.D:
        raise RuntimeError(f"{fl.flag} {k} needs {fl.needs} (this model's data_dim: {eng.D})")
    return k


def _eigen_entry(ev):
    return ("vaek_eigen_event_replicas" if ev.fused else "vaek_cov_eigen_rows") if ev.VEC else \
           ("vaek_spectrum_event_replicas" if ev.fused else "vaek_cov_spectrum_rows")


def _loglik_flag(flag, dest, needs, entry, **kw):
    return Flag(flag, dest, needs,
                banner_one=lambda m: f"Log-likelihood events: {getattr(m, dest)} samples × {m.print_batch_size} rows ({entry})",
                banner_sweep=lambda ev, n, cfg: f"Log-likelihood events: {ev.samples} samples × {ev.rows} rows ({entry})", **kw)


_MLP3_MODEL = ("float32, one decoder, exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, D, L <= 32, "
               "-dd / -did <= 16, on one GPU")

OBSERVABLES = (
    Observable(
        flags=(_loglik_flag("--log_likelihood_samples", "log_likelihood_samples",
                            "a model vaek_log_likelihood_replicas covers (vaek_supports_log_likelihood): a float32 linear VAE -- no hidden "
                            "layers -- with one or two decoders, D, L <= 32 (D <= 28 with two decoders), -dd / -did <= 16, on one GPU",
                            "vaek_log_likelihood_replicas", extra=_sample_cap),),
        events=(("log_likelihood_samples", "_loglik", "ReplicaLogLik"),),
        covered=lambda eng, kind: eng.supports_log_likelihood(kind),
        build=lambda cls, ms, cfg: cls(ms, cfg.log_likelihood_samples),
        run=lambda ev, ran, cfg: ev.event()),
    Observable(            # the same event for an mlp3 model: the two flags cover disjoint models (run.check_log_likelihood_flags)
        flags=(_loglik_flag("--mlp_log_likelihood_samples", "mlp_log_likelihood_samples",
                            "a model vaek_mlp3_log_likelihood_replicas covers (vaek_supports_mlp3_log_likelihood): " + _MLP3_MODEL,
                            "vaek_mlp3_log_likelihood_replicas", extra=_mlp_sample_and_column_caps,
                            linear_hint="this is a linear VAE: use --log_likelihood_samples"),),
        events=(("mlp_log_likelihood_samples", "_loglik_mlp3", "ReplicaLogLikMlp3"),),
        covered=lambda eng, kind: eng.supports_mlp3_log_likelihood(kind),
        build=lambda cls, ms, cfg: cls(ms, cfg.mlp_log_likelihood_samples),
        run=lambda ev, ran, cfg: ev.event()),
    Observable(
        flags=(Flag("--exact_log_likelihood", "exact_log_likelihood",
                    "a model vaek_exact_log_likelihood_replicas covers (vaek_supports_exact_log_likelihood): a float32 linear VAE -- no "
                    "hidden layers -- with ONE decoder (the sigmoid second decoder has no closed form), D, L <= 32, -dd / -did <= 16, on "
                    "one GPU",
                    banner_one=lambda m: f"Exact log-likelihood events: {m.print_batch_size} rows (vaek_exact_log_likelihood_replicas)",
                    banner_sweep=lambda ev, n, cfg: f"Exact log-likelihood events: {ev.rows} rows per model, one launch for {n} models "
                                                    "(vaek_exact_log_likelihood_replicas)"),),
        events=(("exact_log_likelihood", "_exact_loglik", "ReplicaExactLogLik"),),
        covered=lambda eng, kind: eng.supports_exact_log_likelihood(kind),
        build=lambda cls, ms, cfg: cls(ms),
        # on the rows the IWAE event just scored where there is one (then also "IWAE Gap")
        run=lambda ev, ran, cfg: ev.event_after(ran.get("log_likelihood_samples"))),
    Observable(
        flags=(Flag("--elbo_hessian", "elbo_hessian",
                    "a model vaek_elbo_hessian_lanczos_replicas covers (vaek_supports_elbo_hessian): a float32 linear VAE -- no hidden "
                    "layers -- with ONE decoder (the ELBO of other models has no closed form), D, L <= 32, -dd / -did <= 16, on one GPU",
                    banner_one=lambda m: f"ELBO Hessian events: {m.elbo_hessian} Lanczos steps on {m.print_batch_size} rows "
                                         "(vaek_elbo_hessian_lanczos_replicas)",
                    banner_sweep=lambda ev, n, cfg: f"ELBO Hessian events: {ev.steps} Lanczos steps on {ev.rows} rows per model, one launch "
                                                    f"for {n} models (vaek_elbo_hessian_lanczos_replicas)"),),
        events=(("elbo_hessian", "_elbo_hessian", "ReplicaElboHessian"),),
        covered=lambda eng, kind: eng.supports_elbo_hessian(kind),
        build=lambda cls, ms, cfg: cls(ms, cfg.elbo_hessian),
        # on the rows the exact event just scored where there is one (which are the IWAE event's where there was one)
        run=lambda ev, ran, cfg: ev.event_after(exact="exact_log_likelihood" in ran, iwae="log_likelihood_samples" in ran),
        array_keys=lambda cls: cls.KEYS[:2]),          # Sharpness, the smallest Ritz value and the gradient norm are on the line
    Observable(            # one event behind two flags: with --subspace its one device call serves --eigenvalues as well
        flags=(Flag("--eigenvalues", "eigenvalues", "data_dim <= 32 (vaek_supports_cov_spectrum), -dd / -did <= 16, on one GPU",
                    about_dim=True, save_flag=True,      # model_save_data writes "EigenValues"
                    banner_one=lambda m: f"Eigenvalue events: {m.print_batch_size} generated and {m.print_batch_size} real rows "
                                         "(csrc/cov_spectrum.hip)",
                    banner_sweep=lambda ev, n, cfg: f"Eigenvalue events: {ev.rows} generated and {ev.rows} real rows per model "
                                                    f"({_eigen_entry(ev)})"),
               Flag("--subspace", "subspace", "data_dim <= 32 (vaek_supports_cov_spectrum), K in 1 .. data_dim, -dd / -did <= 16, on one GPU",
                    about_dim=True, save_flag=True, extra=_subspace_k,
                    attrs=lambda args, value, k: {"subspace_k": k, "subspace": True},
                    banner_one=lambda m: f"Subspace events: {m.print_batch_size} generated and {m.print_batch_size} real rows "
                                         "(csrc/cov_spectrum.hip)",
                    banner_sweep=lambda ev, n, cfg: f"Subspace events: the {ev.k} leading eigenvectors of {ev.rows} generated and {ev.rows} "
                                                    f"real rows per model ({_eigen_entry(ev)}, vaek_subspace_angles)")),
        events=(("subspace", "_subspace", "ReplicaSubspace"), ("eigenvalues", "_spectrum", "ReplicaSpectrum")),
        covered=lambda eng, kind: eng.supports_cov_spectrum(),
        build=lambda cls, ms, cfg: cls(ms, k=getattr(cfg, "subspace_k", None)) if cls.VEC else cls(ms),
        # --subspace alone: the eigenvalue keys stay out
        run=lambda ev, ran, cfg: ev.event() if getattr(cfg, "eigenvalues", False) else
        [{k: v for k, v in st.items() if k not in _events().ReplicaSpectrum.KEYS} for st in ev.event()]),
    Observable(
        flags=(Flag("--decoder_jacobian", "decoder_jacobian",
                    "a model vaek_mlp3_decoder_jacobian_replicas covers (vaek_supports_mlp3_decoder_jacobian): " + _MLP3_MODEL,
                    extra=_jacobian_column_cap,
                    linear_hint="this is a linear VAE, whose J is the decoder kernel itself at every z: use --exact_log_likelihood, whose "
                                "record holds the eigenvalues of K^T K; per-row records and two-decoder models, which "
                                "--exact_log_likelihood refuses, are what --linear_decoder_jacobian is for",
                    attrs=lambda args, at, checked: {"decoder_jacobian": at, "decoder_jacobian_tol": decoder_jacobian_tol(args)},
                    banner_one=lambda m: f"Decoder Jacobian events: {m.print_batch_size} {m.decoder_jacobian} latent rows, rank threshold "
                                         f"{m.decoder_jacobian_tol:g} (vaek_mlp3_decoder_jacobian_replicas)",
                    banner_sweep=lambda ev, n, cfg: f"Decoder Jacobian events: {ev.rows} {ev.at} latent rows per model, rank threshold "
                                                    f"{ev.rank_tol:g}, one call for {n} models (vaek_mlp3_decoder_jacobian_replicas)"),),
        events=(("decoder_jacobian", "_jacobian", "ReplicaJacobianMlp3"),),
        covered=lambda eng, kind: eng.supports_mlp3_decoder_jacobian(),
        build=lambda cls, ms, cfg: cls(ms, at=cfg.decoder_jacobian, rank_tol=getattr(cfg, "decoder_jacobian_tol", JACOBIAN_DEFAULT_TOL)),
        run=lambda ev, ran, cfg: ev.event(),
        array_keys=lambda cls: cls.KEYS,               # arrays whatever L is; the stats line shows the mean rank
        line=("Decoder Jacobian Rank", "(mean)")),
)

# (the entry it follows, the observable)
LATER_OBSERVABLES = (
    ("elbo_hessian", Observable(
        flags=(Flag("--sampled_elbo_hessian", "sampled_elbo_hessian",
                    "a model vaek_sampled_elbo_hessian_lanczos_replicas covers (vaek_supports_sampled_elbo_hessian): a float32 linear VAE -- "
                    "no hidden layers -- with one or two decoders, D, L <= 32 (D <= 28 with two decoders), -dd / -did <= 16, on one GPU",
                    extra=_sampled_caps, attrs=_sampled_attrs,
                    banner_one=lambda m: f"Sampled ELBO Hessian events: {m.sampled_elbo_hessian} Lanczos steps on {m.print_batch_size} rows "
                                         f"x {m.sampled_elbo_hessian_samples} samples (vaek_sampled_elbo_hessian_lanczos_replicas)",
                    banner_sweep=lambda ev, n, cfg: f"Sampled ELBO Hessian events: {ev.steps} Lanczos steps on {ev.rows} rows x {ev.samples} "
                                                    f"samples per model, one call for {n} models "
                                                    "(vaek_sampled_elbo_hessian_lanczos_replicas)"),),
        events=(("sampled_elbo_hessian", "_sampled_hessian", "ReplicaSampledElboHessian"),),
        covered=lambda eng, kind: eng.supports_sampled_elbo_hessian(kind),
        build=lambda cls, ms, cfg: cls(ms, cfg.sampled_elbo_hessian,
                                       getattr(cfg, "sampled_elbo_hessian_samples", SAMPLED_HESSIAN_DEFAULT_SAMPLES)),
        # on the rows the exact Hessian just used where there was one (then also "Sharpness Sampling Gap")
        run=lambda ev, ran, cfg: ev.event_after(ran),
        array_keys=lambda cls: cls.KEYS[:2])),
)


def _merged():
    table = []
    for ob in OBSERVABLES:
        table.append(ob)
        table.extend(later for after, later in LATER_OBSERVABLES if after == ob.name)
    return tuple(table)


TABLE = _merged()

MLP_HESSIAN_DEFAULT_SAMPLES = 1              # the training loss's own estimator; a column costs 39 KB of workspace at 200|200|200
MLP_HESSIAN_MAX_REPLICA_COLUMNS = 1 << 13


def mlp_sampled_elbo_hessian_samples(args):
    """K of --mlp_sampled_elbo_hessian: --mlp_sampled_elbo_hessian_samples, else 1."""
    k = getattr(args, "mlp_sampled_elbo_hessian_samples", None)
    return MLP_HESSIAN_DEFAULT_SAMPLES if k is None else int(k)


def _mlp_sampled_caps(fl, m, eng, steps, n_models, path):
    return dict(flag=fl.flag, n=n_models, rows=m.print_batch_size, max_samples=eng.log_likelihood_max_samples,
                max_columns=eng.mlp3_sampled_elbo_hessian_max_columns, path=path)


def _mlp_sampled_attrs(args, steps, caps):
    samples = mlp_sampled_elbo_hessian_samples(args)
    if caps is not None:
        if samples > caps["max_samples"]:
            raise RuntimeError(f"{caps['flag']}_samples {samples}: at most {caps['max_samples']} samples per row fit one call "
                               f"(vaek_log_likelihood_max_samples; this model's step path: {caps['path']})")
        cols = caps["n"] * caps["rows"] * samples
        if cols > caps["max_columns"] or caps["rows"] * samples > MLP_HESSIAN_MAX_REPLICA_COLUMNS:
            raise RuntimeError(f"{caps['flag']}_samples {samples}: {caps['n']} models x {caps['rows']} rows x {samples} samples = {cols} "
                               f"columns, at most {caps['max_columns']} fit one call and {MLP_HESSIAN_MAX_REPLICA_COLUMNS} one model "
                               f"(vaek_mlp3_sampled_elbo_hessian_max_columns; this model's step path: {caps['path']})")
    return {"mlp_sampled_elbo_hessian": steps, "mlp_sampled_elbo_hessian_samples": samples}


# (the entry it follows, the observable): the same event and keys as sampled_elbo_hessian for an mlp3 model -- the two flags cover
# disjoint models, as the two log-likelihood flags do
MLP_OBSERVABLES = (
    ("sampled_elbo_hessian", Observable(
        flags=(Flag("--mlp_sampled_elbo_hessian", "mlp_sampled_elbo_hessian",
                    "a model vaek_mlp3_sampled_elbo_hessian_lanczos_replicas covers (vaek_supports_mlp3_sampled_elbo_hessian): " + _MLP3_MODEL,
                    extra=_mlp_sampled_caps, attrs=_mlp_sampled_attrs,
                    linear_hint="this is a linear VAE: use --sampled_elbo_hessian",
                    banner_one=lambda m: f"Sampled ELBO Hessian events: {m.mlp_sampled_elbo_hessian} Lanczos steps on {m.print_batch_size} "
                                         f"rows x {m.mlp_sampled_elbo_hessian_samples} samples "
                                         "(vaek_mlp3_sampled_elbo_hessian_lanczos_replicas)",
                    banner_sweep=lambda ev, n, cfg: f"Sampled ELBO Hessian events: {ev.steps} Lanczos steps on {ev.rows} rows x {ev.samples} "
                                                    f"samples per model, one call for {n} models "
                                                    "(vaek_mlp3_sampled_elbo_hessian_lanczos_replicas)"),),
        events=(("mlp_sampled_elbo_hessian", "_mlp_sampled_hessian", "ReplicaSampledElboHessianMlp3"),),
        covered=lambda eng, kind: eng.supports_mlp3_sampled_elbo_hessian(kind),
        build=lambda cls, ms, cfg: cls(ms, cfg.mlp_sampled_elbo_hessian,
                                       getattr(cfg, "mlp_sampled_elbo_hessian_samples", MLP_HESSIAN_DEFAULT_SAMPLES)),
        run=lambda ev, ran, cfg: ev.event_after(ran),
        array_keys=lambda cls: cls.KEYS[:2])),
)


def _merged_all():
    table = []
    for ob in TABLE:
        table.append(ob)
        table.extend(later for after, later in MLP_OBSERVABLES if after == ob.name)
    return tuple(table)


ALL_OBSERVABLES = _merged_all()


def linear_decoder_jacobian_tol(args):
    """The rank threshold of --linear_decoder_jacobian: --linear_decoder_jacobian_tol, else 1e-4."""
    tol = getattr(args, "linear_decoder_jacobian_tol", None)
    return JACOBIAN_DEFAULT_TOL if tol is None else float(tol)


def _linear_jacobian_extra(fl, m, eng, at, n_models, path):
    total = n_models * m.print_batch_size
    if total > eng.linear_decoder_jacobian_max_rows:
        raise RuntimeError(f"{fl.flag}: {n_models} models x {m.print_batch_size} rows = {total} rows, at most "
                           f"{eng.linear_decoder_jacobian_max_rows} fit one call (vaek_linear_decoder_jacobian_max_rows; this model's "
                           f"step path: {path})")


# (the entry it follows, the observable): the same event and keys as decoder_jacobian for a linear model -- the two flags cover
# disjoint models, as the two log-likelihood flags do (run.check_decoder_jacobian_flags refuses the two together).  Its NEEDS text
# ends with the hint for an MLP model: Flag.linear_hint is the hint for the opposite mistake
LINEAR_OBSERVABLES = (
    ("decoder_jacobian", Observable(
        flags=(Flag("--linear_decoder_jacobian", "linear_decoder_jacobian",
                    "a model vaek_linear_decoder_jacobian_replicas covers (vaek_supports_linear_decoder_jacobian): a float32 linear VAE -- "
                    "no hidden layers -- with one or two decoders, D, L <= 32 (D <= 28 with two decoders), -dd / -did <= 16, on one GPU; "
                    "a three-hidden-layer MLP model takes --decoder_jacobian",
                    extra=_linear_jacobian_extra,
                    attrs=lambda args, at, checked: {"linear_decoder_jacobian": at,
                                                     "linear_decoder_jacobian_tol": linear_decoder_jacobian_tol(args)},
                    banner_one=lambda m: f"Decoder Jacobian events: {m.print_batch_size} {m.linear_decoder_jacobian} latent rows, rank "
                                         f"threshold {m.linear_decoder_jacobian_tol:g} (vaek_linear_decoder_jacobian_replicas)",
                    banner_sweep=lambda ev, n, cfg: f"Decoder Jacobian events: {ev.rows} {ev.at} latent rows per model, rank threshold "
                                                    f"{ev.rank_tol:g}, one call for {n} models (vaek_linear_decoder_jacobian_replicas)"),),
        events=(("linear_decoder_jacobian", "_linear_jacobian", "ReplicaJacobianLinear"),),
        covered=lambda eng, kind: eng.supports_linear_decoder_jacobian(),
        build=lambda cls, ms, cfg: cls(ms, at=cfg.linear_decoder_jacobian,
                                       rank_tol=getattr(cfg, "linear_decoder_jacobian_tol", JACOBIAN_DEFAULT_TOL)),
        run=lambda ev, ran, cfg: ev.event(),
        array_keys=lambda cls: cls.KEYS,               # arrays whatever L is; the stats line shows the mean rank
        line=("Decoder Jacobian Rank", "(mean)"))),
)


def _merged_every():
    table = []
    for ob in ALL_OBSERVABLES:
        table.append(ob)
        table.extend(later for after, later in LINEAR_OBSERVABLES if after == ob.name)
    return tuple(table)


EVERY_OBSERVABLE = _merged_every()
FLAGS = {fl.dest: (ob, fl) for ob in EVERY_OBSERVABLE for fl in ob.flags}


# ---- the refusals ---------------------------------------------------------------------------------------------------------------
def refuse_data_parallel(args, world):
    """world > 1: refuse every observable flag in `args`, in table order, before a process group exists."""
    for ob, fl in FLAGS.values():
        if fl.value(args) is not None:
            raise RuntimeError(f"{fl.flag} needs {fl.needs}: it does not combine with data parallelism "
                               f"(step path of a world of {world}: one shard per rank)")


def check_model(dest, m, value=None, n_models=1):
    """Refuse, before any step, a model the observable's call does not cover, and what the flag's `extra` refuses; returns what
    `extra` returns (--subspace: K, None for auto)."""
    from .datasets import DEVICE_DRAW_MAX_DIM
    ob, fl = FLAGS[dest]
    eng = m.model.module.engine(m.batch_size, m.optimizer.global_batch)
    kind, _, dd, did, _, _ = m.dataset.device_spec()
    path = getattr(eng, "step_path", "?")
    if fl.linear_hint is not None and eng.world == 1 and eng.supports_log_likelihood(kind):
        raise RuntimeError(f"{fl.flag} needs {fl.needs}; {fl.linear_hint} (this model's step path: {path})")
    if eng.world > 1 or dd > DEVICE_DRAW_MAX_DIM or did > DEVICE_DRAW_MAX_DIM or not ob.covered(eng, kind):
        about = f"data_dim: {getattr(eng, 'D', '?')}" if fl.about_dim else f"step path: {path}"
        raise RuntimeError(f"{fl.flag} needs {fl.needs} (this model's {about}, world {eng.world})")
    return None if fl.extra is None else fl.extra(fl, m, eng, value, n_models, path)


def attach(args, models, cfg, build):
    """For every observable flag in `args`, in table order: check_model on model 0 (refusing before any step), set the flag's
    attributes on `cfg` (the model itself for a single model, the sweep's settings for a sweep) and yield the flag.  With `build`
    an observable's event object is built as soon as its flags are checked -- before any step; without, on its first event."""
    for ob in EVERY_OBSERVABLE:
        for fl in ob.flags:
            value = fl.value(args)
            if value is not None:
                checked = check_model(fl.dest, models[0], value, len(models))
                for name, v in ({fl.dest: value} if fl.attrs is None else fl.attrs(args, value, checked)).items():
                    setattr(cfg, name, v)
                yield fl
        if build:
            _event(ob, models, cfg)


# ---- the events -------------------------------------------------------------------------------------------------------------------
def _event(ob, models, cfg):
    """The event object of `ob` where one of its flags is set on `cfg`, else None: kept on `cfg` under the row's cache name, built
    on first use."""
    row = next((i for i, (dest, _, _) in enumerate(ob.events) if getattr(cfg, dest, None)), None)
    if row is None:
        return None
    cache = ob.events[row][1]
    if getattr(cfg, cache, None) is None:
        setattr(cfg, cache, ob.build(ob.event_class(row), models, cfg))
    return getattr(cfg, cache)


def active(models, cfg):
    """(observable, its event object) of every observable set on `cfg`, in table order."""
    for ob in EVERY_OBSERVABLE:
        ev = _event(ob, models, cfg)
        if ev is not None:
            yield ob, ev


def run_events(models, cfg):
    """One n_print event: every observable set on `cfg`, one device call each, in table order.  Returns one dict per model: what to
    merge into its stats."""
    out, ran = [{} for _ in models], {}
    for ob, ev in active(models, cfg):
        ran[ob.name] = stats = ob.run(ev, ran, cfg)
        for merged, st in zip(out, stats):
            merged.update(st)
    return out


# ---- write_stats ----------------------------------------------------------------------------------------------------------------
def array_keys(dest):
    ob = FLAGS[dest][0]
    return tuple(ob.array_keys(ob.event_class()))


def stats_line_rules(table=OBSERVABLES):
    """({array key: the text write_stats puts in front of element 0 of its value, or None: nothing on the line}) of `table` (model.py
    passes EVERY_OBSERVABLE)."""
    rules = {}
    for ob in table:
        for key in ob.array_keys(ob.event_class()):
            rules[key] = f"{key} {ob.line[1]}" if ob.line is not None and ob.line[0] == key else None
    return rules
