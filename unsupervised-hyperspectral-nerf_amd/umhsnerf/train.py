"""``python -m umhsnerf.train --data DIR [flags]`` and an importable ``Trainer``: what nerfstudio's ``ns-train umhsnerf`` does for this
method, without nerfstudio -- scene directory in, ``OUTPUT/<experiment-name>/umhsnerf/<timestamp>/`` out:

  config.json                            every config value, the scene path, and what the data manager derived (wavelengths, classes)
  nerfstudio_models/step-<step:09d>.ckpt {"step", "pipeline", "optimizers": {"fields": ...}, "schedulers": {}, "scalers": None,
                                          "umhs_trainer": {...}}: the first three keys as nerfstudio's trainer names them
                                          [upstream-recalled], so ``eval.load_checkpoint`` and the reference's ``load_pipeline`` read it
  log.jsonl                              the config, one JSON object per logged step / evaluation, and {"event": "done", ...} last

It is built on the stand-alone pipeline (``UMHSPipeline.from_packed_samples``, ``trainer_driven=False``): one ``get_train_loss_dict(step)``
is the whole iteration -- grid update, pixel batch, march, hot path, fused Adam + clamp, prefetch of the next batch.  ``"step"`` of a
checkpoint is the number of completed iterations, i.e. the index of the next one.

Flags are nerfstudio's dotted names (``--pipeline.model.far-plane 1000``), ``-`` and ``_`` interchangeable inside a name as tyro
allows.  The ``--pipeline.*`` flags are generated from the dataclass fields of ``UMHSPipelineConfig``, ``UMHSConfig``,
``UMHSDataManagerConfig`` and ``UMHSDataParserConfig``; the trainer's own from ``TrainerConfig`` below.

Resume is bit-exact: N steps, a save, and M more steps in a fresh process from ``--load-dir`` end with the parameter, moment and
occupancy-grid bits of N + M steps in one go.  Two things make it so.  (a) When step s returns the pipeline has normally drawn the
batch and the jitter of step s + 1 already (``_prefetch_next``); a generator state saved then would be one draw ahead of a batch that
is lost.  The trainer sets ``pipeline.hold_prefetch`` for the step in front of a save (and of an evaluation, whose own march would
discard the prefetched one): that step draws nothing ahead, and the trajectory has the same bits with and without prefetch
(tests/test_hip_sampler.py).  (b) Evaluation between two steps keeps and restores the device generator's state and draws its pixels
from the data manager's eval generator only.  With gradient accumulation a save waits for the end of its window.

``--log-gradients True`` takes, on logging steps only, ONE ``ops.segment_stats`` launch over ``flat.grad`` (bounds = the entries of the
field's flat layout, built once, on the device) instead of nerfstudio's ``.grad.norm()`` and host read per parameter.  On those steps
``pipeline.keep_gradient`` withholds the fused Adam arm so that the whole gradient lands in ``flat.grad`` (the two paths are tested
bit-identical).  ``Gradients/Total`` is the SUM of the per-parameter norms, as nerfstudio logs it [upstream-recalled], not the norm of
the whole gradient.  The same launch over ``flat.data`` gives the parameters' non-finite count; a non-zero count in either buffer ends
the run with ``FloatingPointError`` (step and parameter named) after the log line is written and without saving."""
from __future__ import annotations

import ast
import dataclasses
import json
import math
import os
import sys
import time
import typing
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional

METHOD_NAME = "umhsnerf"
MAX_DEVICES = 16


@dataclass
class MachineConfig:
    seed: int = 42
    num_devices: int = 1


@dataclass
class AdamConfig:
    lr: float = 2e-2
    eps: float = 1e-15


@dataclass
class SchedulerConfig:
    """The exponential decay built into ``UMHSAdam``.  ``max_steps`` None: ``--max-num-iterations``."""

    lr_final: float = 1e-5
    max_steps: Optional[int] = None


@dataclass
class GroupConfig:
    optimizer: AdamConfig = field(default_factory=AdamConfig)
    scheduler: SchedulerConfig = field(default_factory=SchedulerConfig)


@dataclass
class OptimizersConfig:
    fields: GroupConfig = field(default_factory=GroupConfig)  # --optimizers.fields.scheduler.max-steps ...


@dataclass
class TrainerConfig:
    """The trainer-level flags (nerfstudio ``TrainerConfig`` names; defaults of umhs_config.py where it sets them)."""

    data: Optional[Path] = None
    output_dir: Path = Path("outputs")
    experiment_name: Optional[str] = None
    timestamp: Optional[str] = None
    max_num_iterations: int = 30000
    steps_per_save: int = 2000
    save_only_latest_checkpoint: bool = False
    steps_per_eval_batch: int = 500
    steps_per_eval_image: int = 500
    steps_per_eval_all_images: int = 25000
    logging_steps: int = 10
    log_gradients: bool = False
    gradient_accumulation_steps: int = 1
    load_dir: Optional[Path] = None
    load_checkpoint: Optional[Path] = None
    load_step: Optional[int] = None
    vis: str = "viewer"
    machine: MachineConfig = field(default_factory=MachineConfig)
    optimizers: OptimizersConfig = field(default_factory=OptimizersConfig)
    pipeline: Any = None  # UMHSPipelineConfig (umhs_config.make_pipeline_config())
    viewer: Dict[str, str] = field(default_factory=dict)  # --viewer.*: accepted, kept, ignored

    def __post_init__(self):
        if self.pipeline is None:
            from .umhs_config import make_pipeline_config

            self.pipeline = make_pipeline_config()


# ---- flags -----------------------------------------------------------------------------------------------------------------
def _is_config(value) -> bool:
    return dataclasses.is_dataclass(value) and not isinstance(value, type)


def _hints(obj) -> Dict[str, Any]:
    try:
        return typing.get_type_hints(type(obj))
    except Exception:  # a hint that cannot be resolved here: its fields convert by their current value
        return {}


def flag_table(config) -> Dict[str, tuple]:
    """dotted flag name (``_`` spelling) -> (owning config object, field name, type hint), for every dataclass field of the tree."""
    table: Dict[str, tuple] = {}

    def walk(obj, prefix):
        hints = _hints(obj)
        for f in dataclasses.fields(obj):
            if f.name.startswith("_"):
                continue
            value = getattr(obj, f.name)
            if _is_config(value):
                walk(value, f"{prefix}{f.name}.")
            elif not (obj is config and f.name == "viewer"):
                table[f"{prefix}{f.name}"] = (obj, f.name, hints.get(f.name))

    walk(config, "")
    return table


def _bool(text: str) -> bool:
    if text.lower() in ("true", "1", "yes"):
        return True
    if text.lower() in ("false", "0", "no"):
        return False
    raise ValueError(f"expected True or False, got {text!r}")


def _convert(text: str, hint, current):
    """A flag's text as the field's type: the hint when it says enough, else the type of the current value, else a Python literal."""
    origin, args = typing.get_origin(hint), typing.get_args(hint)
    if origin is typing.Union:
        if type(None) in args and text.lower() == "none":
            return None
        for a in args:
            if a is type(None):
                continue
            try:
                return _convert(text, a, None)
            except (ValueError, SyntaxError):
                continue
        raise ValueError(f"{text!r} is none of {args}")
    if origin is typing.Literal:
        for choice in args:
            if str(choice) == text:
                return choice
        raise ValueError(f"{text!r}: one of {', '.join(map(str, args))}")
    if hint is bool or (hint is None and isinstance(current, bool)):
        return _bool(text)
    for t in (int, float, str, Path):
        if hint is t or (hint is None and type(current) is t):
            return t(text)
    if hint is Any or hint is None:
        try:
            return ast.literal_eval(text)
        except (ValueError, SyntaxError):
            return text
    value = ast.literal_eval(text)  # lists, tuples, dicts
    want = origin or hint
    if isinstance(want, type) and not isinstance(value, want):
        if want in (list, tuple) and isinstance(value, (list, tuple)):
            return want(value)
        raise ValueError(f"{text!r} is no {want.__name__}")
    return value


def parse_flags(argv: List[str], config: Optional[TrainerConfig] = None) -> TrainerConfig:
    """nerfstudio-spelled flags -> ``TrainerConfig``.  ``--flag value`` or ``--flag=value``; a boolean flag without a value means True.
    An optional leading method name (``umhsnerf`` / ``umhs``, as after ``ns-train``) is skipped."""
    config = config or TrainerConfig()
    table = flag_table(config)
    argv = list(argv)
    if argv and argv[0] in (METHOD_NAME, "umhs"):
        argv.pop(0)
    i = 0
    while i < len(argv):
        token = argv[i]
        i += 1
        if not token.startswith("--"):
            raise SystemExit(f"python -m umhsnerf.train: unexpected argument {token!r}")
        name, eq, value = token[2:].partition("=")
        name = name.replace("-", "_")
        following = argv[i] if i < len(argv) and not argv[i].startswith("--") else None
        if name.startswith("viewer."):  # accepted and ignored
            if not eq and following is not None:
                value, i = following, i + 1
            config.viewer[name[len("viewer."):]] = value
            continue
        if name == "pipeline.model.implementation":  # tcnn | torch | hip: there is one implementation here
            if not eq and following is not None:
                i += 1
            continue
        if name not in table:
            raise SystemExit(f"python -m umhsnerf.train: unknown flag --{name} (flags are generated from the config dataclasses)")
        owner, attr, hint = table[name]
        current = getattr(owner, attr)
        is_bool = hint is bool or isinstance(current, bool)
        if not eq:
            if following is not None and (not is_bool or following.lower() in ("true", "false", "1", "0", "yes", "no")):
                value, i = following, i + 1
            elif is_bool:
                value = "True"
            else:
                raise SystemExit(f"python -m umhsnerf.train: --{name} needs a value")
        try:
            setattr(owner, attr, _convert(value, hint, current))
        except (ValueError, SyntaxError) as e:
            raise SystemExit(f"python -m umhsnerf.train: --{name} {value}: {e}")
    if config.data is not None:  # nerfstudio's --data is the data parser's
        config.pipeline.datamanager.dataparser.data = Path(config.data)
    elif str(config.pipeline.datamanager.dataparser.data) not in ("", "."):
        config.data = Path(config.pipeline.datamanager.dataparser.data)
    config.pipeline.gradient_accumulation_steps = max(1, int(config.gradient_accumulation_steps))
    return config


def config_to_dict(obj) -> Any:
    """The config tree as JSON values (``_target`` and other private fields left out)."""
    if _is_config(obj):
        return {f.name: config_to_dict(getattr(obj, f.name)) for f in dataclasses.fields(obj) if not f.name.startswith("_")}
    if isinstance(obj, dict):
        return {str(k): config_to_dict(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [config_to_dict(v) for v in obj]
    if isinstance(obj, Path):
        return str(obj)
    if isinstance(obj, (str, int, float, bool)) or obj is None:
        return obj
    return repr(obj)


def _vis_notice(vis: str) -> Optional[str]:
    missing = [b for b in ("viewer", "wandb", "tensorboard") if b in vis.lower()]
    if not missing:
        return None
    return f"--vis {vis}: {', '.join(missing)} is not in this package; the log goes to log.jsonl in the run directory"


# ---- the trainer -----------------------------------------------------------------------------------------------------------
class Trainer:
    """``Trainer(config).train()``.  ``local_rank`` / ``world_size``: one process per device (``main`` starts them); with more than one
    the process group must be initialised.  Rank 0 writes the files."""

    def __init__(self, config: TrainerConfig, local_rank: int = 0, world_size: int = 1, pipeline=None):
        """``pipeline``: a stand-alone ``UMHSPipeline`` (``from_packed_samples`` with a data manager) to train as it is, with its own
        optimizer -- tools and tests that hold resident splits; None: built from ``config`` (scene on disk)."""
        import numpy as np
        import torch

        from . import ops
        from .umhs_pipeline import UMHSPipeline

        if config.data is None and pipeline is None:
            raise SystemExit("python -m umhsnerf.train: --data is required")
        self.config, self.rank, self.world = config, int(local_rank), int(world_size)
        self.device = torch.device(f"cuda:{self.rank}")
        torch.cuda.set_device(self.device)
        group = config.optimizers.fields  # the schedule built into UMHSAdam (lr_final = 1e-5) runs over --max-num-iterations steps
        self.schedule_steps = int(group.scheduler.max_steps if group.scheduler.max_steps is not None else config.max_num_iterations)
        if pipeline is not None:
            if pipeline.trainer_driven or pipeline.datamanager is None:
                raise ValueError("Trainer(pipeline=) needs a stand-alone pipeline with a data manager")
            self.pipeline, self.optimizer = pipeline, pipeline.optimizer
        else:
            seed = int(config.machine.seed)
            torch.manual_seed(seed + self.rank)  # nerfstudio: seed + global rank
            torch.cuda.manual_seed(seed + self.rank)
            np.random.seed(seed + self.rank)
            pc = config.pipeline
            dm = pc.datamanager.setup(device=self.device, test_mode="val", world_size=self.world, local_rank=self.rank,
                                      num_classes=pc.num_classes, seed=seed)
            self.pipeline = UMHSPipeline.from_packed_samples(pc.model, self.device, metadata={"num_classes": pc.num_classes},
                                                             world_size=self.world, local_rank=self.rank, seed=seed, datamanager=dm,
                                                             gradient_accumulation_steps=pc.gradient_accumulation_steps)
            self.pipeline.config.datamanager, self.pipeline.config.check_nan = pc.datamanager, pc.check_nan
            self.optimizer = self.pipeline.optimizer = self.pipeline.model.make_optimizer(
                lr=group.optimizer.lr, eps=group.optimizer.eps, lr_final=group.scheduler.lr_final, max_steps=self.schedule_steps)
        self.field = self.pipeline.model.field
        self.bounds = ops.SegmentBounds.of_layout(self.field.layout, self.device)  # built once, kept on the device
        self.names = list(self.bounds.names)
        self.start_step = 0
        self._pending: List[tuple] = []  # rows on their way to the host: (event, pinned row, keys, host values, step)
        self._log_file = None
        self._last_log = None  # (step, perf_counter) of the previous logged step
        experiment = config.experiment_name or (Path(config.data).resolve().name if config.data is not None else "") or "unnamed"
        self.timestamp = config.timestamp or time.strftime("%Y-%m-%d_%H%M%S")
        self.run_dir = Path(config.output_dir) / experiment / METHOD_NAME / self.timestamp
        self.checkpoint_dir = self.run_dir / "nerfstudio_models"
        self._resume()

    # ---- files -----------------------------------------------------------------------------------------------------------
    def config_dict(self) -> Dict:
        d = config_to_dict(self.config)
        d["method_name"] = METHOD_NAME
        d["data"] = str(Path(self.config.data)) if self.config.data is not None else None
        meta = self.pipeline.model.kwargs
        d["derived"] = {"wavelengths": [float(w) for w in meta["wavelengths"]], "num_classes": int(meta["num_classes"]),
                        "num_train_images": len(self.pipeline.datamanager.train_dataset), "world_size": self.world}
        return d

    def _open_run(self) -> None:
        if self.rank != 0:
            return
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)
        cfg = self.config_dict()
        (self.run_dir / "config.json").write_text(json.dumps(cfg, indent=1))
        self._log_file = open(self.run_dir / "log.jsonl", "a")
        self._write({"event": "config", "start_step": self.start_step, "config": cfg})
        notice = _vis_notice(self.config.vis)
        if notice:
            print(notice, flush=True)

    def _write(self, row: Dict) -> None:
        if self._log_file is not None:
            self._log_file.write(json.dumps(row) + "\n")
            self._log_file.flush()

    # ---- checkpoints -----------------------------------------------------------------------------------------------------
    def _rank_state(self) -> Dict:
        import torch

        return {"device_rng": torch.cuda.get_rng_state(self.device), "cpu_rng": torch.get_rng_state(),
                "datamanager": self.pipeline.datamanager.sampling_state()}

    def save_checkpoint(self, step: int) -> Optional[Path]:
        """``step`` = completed iterations.  Every rank hands in its generator states; rank 0 writes the file."""
        import torch
        import torch.distributed as dist

        torch.cuda.synchronize(self.device)
        self.flush_logs()
        assert getattr(self.pipeline, "_ahead", None) is None, "a batch was drawn ahead of a save (hold_prefetch was not set)"
        mine = self._rank_state()
        ranks = [mine]
        if self.world > 1:
            ranks = [None] * self.world if self.rank == 0 else None
            dist.gather_object(mine, ranks, dst=0)
        if self.rank != 0:
            return None
        path = self.checkpoint_dir / f"step-{step:09d}.ckpt"
        state = {"step": step, "pipeline": self.pipeline.state_dict(), "optimizers": {"fields": self.optimizer.state_dict()},
                 "schedulers": {}, "scalers": None,
                 "umhs_trainer": {"ranks": ranks, "world_size": self.world, "micro": 0,
                                  "gradient_accumulation_steps": self.pipeline.gradient_accumulation_steps}}
        tmp = path.with_suffix(".tmp")
        torch.save(state, tmp)
        os.replace(tmp, path)
        if self.config.save_only_latest_checkpoint:  # the older files go once the new one is written
            for old in self.checkpoint_dir.glob("step-*.ckpt"):
                if old != path:
                    old.unlink()
        return path

    def _resume(self) -> None:
        import torch

        c = self.config
        path = None
        if c.load_checkpoint is not None:
            path = Path(c.load_checkpoint)
        elif c.load_dir is not None:
            if c.load_step is not None:
                path = Path(c.load_dir) / f"step-{int(c.load_step):09d}.ckpt"
            else:
                found = sorted(Path(c.load_dir).glob("step-*.ckpt"))
                if not found:
                    raise FileNotFoundError(f"--load-dir {c.load_dir} holds no step-*.ckpt")
                path = found[-1]
        if path is None:
            return
        loaded = torch.load(path, map_location="cpu", weights_only=False)
        step = int(loaded["step"])
        self.pipeline.load_pipeline(loaded["pipeline"], step)
        if "optimizers" in loaded and "fields" in loaded["optimizers"]:
            self.optimizer.load_state_dict(loaded["optimizers"]["fields"])
            for group in self.optimizer.param_groups:  # this run's flags, not the saved run's
                group["max_steps"] = self.schedule_steps
        extra = loaded.get("umhs_trainer")
        if extra is not None:  # a bit-exact resume; a checkpoint without it (nerfstudio's) resumes with fresh generators
            if int(extra["world_size"]) != self.world:
                raise RuntimeError(f"{path} was written by {extra['world_size']} ranks; this run has {self.world}")
            mine = extra["ranks"][self.rank]
            torch.cuda.set_rng_state(mine["device_rng"], self.device)
            torch.set_rng_state(mine["cpu_rng"])
            self.pipeline.datamanager.load_sampling_state(mine["datamanager"])
        self.loaded_from, self.start_step = path, step

    # ---- logging ---------------------------------------------------------------------------------------------------------
    def log_step(self, step: int, loss_dict: Dict, metrics_dict: Dict, wait: bool = False) -> None:
        """Queues the row of a logged step: loss terms, psnr / psnr_spectral / num_samples_per_batch, the learning rate, steps per
        second and -- with ``log_gradients`` -- the statistics of ``flat.grad`` (one ``segment_stats`` launch) and the non-finite count
        of ``flat.data`` (one more).  Everything is packed into one device row and copied to pinned memory without blocking; the row
        is written by ``flush_logs`` once its event has completed (``wait``: now)."""
        import torch

        from . import ops

        keys, parts = [], []
        for k, v in loss_dict.items():
            keys.append(f"Train Loss Dict/{k}")
            parts.append(v.detach().reshape(1).double())
        keys.append("Train Loss")
        parts.append(sum(v.detach().double() for v in loss_dict.values()).reshape(1))
        for k in ("psnr", "psnr_spectral", "num_samples_per_batch"):
            if k in metrics_dict:
                keys.append(f"Train Metrics Dict/{k}")
                parts.append(torch.as_tensor(metrics_dict[k], device=self.device).detach().reshape(1).double())
        n_plain = len(keys)
        with_grads = bool(self.config.log_gradients)
        if with_grads:
            flat = self.field.flat
            if flat.grad is None:
                raise RuntimeError("log_gradients: flat.grad is empty (the step was not run with pipeline.keep_gradient)")
            parts.append(ops.segment_stats(flat.grad, self.bounds).reshape(-1))
            parts.append(ops.segment_stats(flat.data, self.bounds)[:, 2])
        row = torch.cat(parts)
        host = torch.empty(row.shape, dtype=row.dtype, pin_memory=True)
        host.copy_(row, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self.device))
        group = self.optimizer.param_groups[0]
        st = self.optimizer.state.get(group["params"][0], {})
        from .optim import exp_decay_lr

        done = max(int(st.get("step", 0)) - 1, 0)  # the update this step applied
        lr = exp_decay_lr(done, group["lr_init"], group["lr_final"], group["max_steps"]) if group["lr_final"] is not None else group["lr"]
        values = {"step": step, "learning_rate/fields": lr}
        now = time.perf_counter()
        if self._last_log is not None and step > self._last_log[0]:
            values["steps_per_sec"] = (step - self._last_log[0]) / max(now - self._last_log[1], 1e-9)
        self._last_log = (step, now)
        self._pending.append((event, host, keys, n_plain, with_grads, values))
        self.flush_logs(wait=wait)

    def flush_logs(self, wait: bool = False) -> None:
        """Writes the queued rows whose copy has landed (``wait``: all of them, after their events).  Raises ``FloatingPointError`` for a
        row with non-finite gradients or parameters -- after that row is written."""
        while self._pending and (wait or self._pending[0][0].query()):
            event, host, keys, n_plain, with_grads, values = self._pending.pop(0)
            event.synchronize()
            v = host.tolist()
            row = dict(values)
            row.update({k: v[i] for i, k in enumerate(keys)})
            bad = []
            if with_grads:
                k = len(self.names)
                stats, params = v[n_plain:n_plain + 3 * k], v[n_plain + 3 * k:n_plain + 4 * k]
                total, max_abs = 0.0, 0.0
                for i, name in enumerate(self.names):
                    norm = math.sqrt(stats[3 * i])
                    row[f"Gradients/field.{name}"] = norm
                    total, max_abs = total + norm, max(max_abs, stats[3 * i + 1])
                    if stats[3 * i + 2]:
                        bad.append(f"{int(stats[3 * i + 2])} non-finite gradient value(s) in field.{name}")
                    if params[i]:
                        bad.append(f"{int(params[i])} non-finite parameter value(s) in field.{name}")
                row["Gradients/Total"], row["Gradients/max_abs"] = total, max_abs
                row["Gradients/non_finite"] = sum(stats[2::3]) + sum(params)
            self.last_row = row
            self._write(row)
            if bad:
                raise FloatingPointError(f"step {values['step']}: " + "; ".join(bad))

    # ---- evaluation ------------------------------------------------------------------------------------------------------
    def _evaluate(self, step: int, last: bool) -> None:
        """``step`` = completed iterations.  The device generator's state is kept and restored around every evaluation, so the training
        stream of random numbers does not move; the eval batches draw from the data manager's eval generator."""
        import torch

        c = self.config
        due = lambda every: every > 0 and step % every == 0
        batch, image, everything = due(c.steps_per_eval_batch), due(c.steps_per_eval_image), due(c.steps_per_eval_all_images) or last
        if not (batch or image or everything):
            return
        torch.cuda.synchronize(self.device)
        keep_dev, keep_cpu = torch.cuda.get_rng_state(self.device), torch.get_rng_state()
        num = lambda x: float(x) if not torch.is_tensor(x) or x.numel() == 1 else None
        row: Dict[str, Any] = {"step": step, "event": "eval"}
        try:
            if batch:
                _, loss_dict, metrics = self.pipeline.get_eval_loss_dict(step)
                row.update({f"Eval Loss Dict/{k}": num(v) for k, v in loss_dict.items()})
                row.update({f"Eval Metrics Dict/{k}": num(v) for k, v in dict(metrics).items()})
            if image:
                metrics, _ = self.pipeline.get_eval_image_metrics_and_images(step)
                row.update({f"Eval Images Metrics/{k}": num(v) for k, v in metrics.items()})
            if everything and self.rank == 0:
                metrics = self.pipeline.get_average_eval_image_metrics(step=step)
                row.update({f"Eval Images Metrics Dict (all images)/{k}": num(v) for k, v in metrics.items()})
        finally:
            torch.cuda.synchronize(self.device)
            torch.cuda.set_rng_state(keep_dev, self.device)
            torch.set_rng_state(keep_cpu)
        self._write({k: v for k, v in row.items() if v is not None})

    # ---- the loop --------------------------------------------------------------------------------------------------------
    def _after(self, step: int):
        """What follows iteration ``step`` (0-based): (save, evaluate)."""
        c = self.config
        done, last = step + 1, step + 1 >= c.max_num_iterations
        window_end = done % self.pipeline.gradient_accumulation_steps == 0
        save = last or (c.steps_per_save > 0 and done % c.steps_per_save == 0 and window_end)
        evaluate = last or any(every > 0 and done % every == 0
                               for every in (c.steps_per_eval_batch, c.steps_per_eval_image, c.steps_per_eval_all_images))
        return save, evaluate

    def train_step(self, step: int):
        """One iteration; the trainer's only additions are two attributes of the pipeline and, on a logging step, the row."""
        c, p = self.config, self.pipeline
        save, evaluate = self._after(step)
        logging = c.logging_steps > 0 and step % c.logging_steps == 0
        p.hold_prefetch = save or evaluate
        p.keep_gradient = logging and c.log_gradients
        outputs, loss_dict, metrics_dict = p.get_train_loss_dict(step)
        p.hold_prefetch = p.keep_gradient = False
        if logging:
            self.log_step(step, loss_dict, metrics_dict)
        elif self._pending:
            self.flush_logs()
        return outputs, loss_dict, metrics_dict

    def train(self) -> Dict:
        import torch

        c = self.config
        self._open_run()
        t0, saved = time.perf_counter(), []
        try:
            for step in range(self.start_step, int(c.max_num_iterations)):
                self.train_step(step)
                save, evaluate = self._after(step)
                if save or evaluate:
                    torch.cuda.synchronize(self.device)
                    self.flush_logs(wait=True)
                if evaluate:
                    self._evaluate(step + 1, last=step + 1 >= c.max_num_iterations)
                if save:
                    path = self.save_checkpoint(step + 1)
                    if path is not None:
                        saved.append(str(path))
            torch.cuda.synchronize(self.device)
            self.flush_logs(wait=True)
            result = {"event": "done", "step": int(c.max_num_iterations), "start_step": self.start_step, "run_dir": str(self.run_dir),
                      "checkpoints": saved, "seconds": time.perf_counter() - t0}
            self._write(result)
            return result
        finally:
            if self._log_file is not None:
                self._log_file.close()
                self._log_file = None


# ---- processes -------------------------------------------------------------------------------------------------------------
def _rank_main(rank: int, world: int, port: int, argv: List[str]) -> None:
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        Trainer(parse_flags(argv), local_rank=rank, world_size=world).train()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main(argv: Optional[List[str]] = None) -> Optional[Dict]:
    argv = list(sys.argv[1:] if argv is None else argv)
    config = parse_flags(argv)
    world = int(config.machine.num_devices)
    if not 1 <= world <= MAX_DEVICES:
        raise SystemExit(f"python -m umhsnerf.train: --machine.num-devices {world}: 1..{MAX_DEVICES}")
    if world == 1:
        result = Trainer(config).train()
        print(json.dumps(result))
        return result
    # one fresh child process per device; this process never initialises the GPU
    import torch.multiprocessing as mp

    if config.timestamp is None:  # every rank names the same run directory
        argv += ["--timestamp", time.strftime("%Y-%m-%d_%H%M%S")]
    port, ctx = _free_port(), mp.get_context("spawn")
    children = [ctx.Process(target=_rank_main, args=(rank, world, port, argv)) for rank in range(world)]
    for child in children:
        child.start()
    failed = None
    while failed is None and any(child.is_alive() for child in children):
        for child in children:
            child.join(timeout=0.2)
            if child.exitcode not in (None, 0):
                failed = child.exitcode
    if failed is not None:  # one rank failed: the others would wait for it in a collective
        for child in children:
            if child.is_alive():
                child.terminate()
        for child in children:
            child.join()
        raise SystemExit(f"python -m umhsnerf.train: a rank ended with exit code {failed}")
    for child in children:
        child.join()
        if child.exitcode != 0:
            raise SystemExit(f"python -m umhsnerf.train: a rank ended with exit code {child.exitcode}")
    return None


if __name__ == "__main__":
    main()
    sys.exit(0)
