"""What the stand-alone trainer and its gradient statistics cost, on bench.py's sampler scene with the C2-shaped model:

  (a) steps per second of the trainer's loop (``Trainer.train_step``: logging every 10 steps, gradients logged, rows flushed) over 300
      steps, against the bare ``get_train_loss_dict`` loop of bench.py's ``sampler_step`` on the same pipeline: device events around
      each loop, warm, median of 7 alternated rounds;
  (b) ``ops.segment_stats`` over the flat gradient against a device copy of the same bytes;
  (c) the same statistics the way nerfstudio's ``--log-gradients`` takes them: ``view.norm()`` and a host read per named parameter.

    python tools/bench_train.py            ->  profiles/train/bench_train.json  (and the same JSON on stdout)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS, ROUNDS, REPS = 300, 7, 30


def _events_ms(fn, reps=REPS):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))


def main():
    import bench
    from umhsnerf import ops
    from umhsnerf.train import Trainer, TrainerConfig

    dev = torch.device("cuda:0")
    pipe, _ = bench.sampler_scene(bench.C2, dev)
    config = TrainerConfig(max_num_iterations=10 ** 9, logging_steps=10, log_gradients=True, steps_per_save=0, steps_per_eval_batch=0,
                           steps_per_eval_image=0, steps_per_eval_all_images=0)
    trainer = Trainer(config, pipeline=pipe)
    step = 300  # sampler_scene has run steps 0..299

    def loop(body, first):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for s in range(first, first + STEPS):
            body(s)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / STEPS, (time.perf_counter() - t0) / STEPS * 1e3

    def trainer_body(s):
        trainer.train_step(s)

    bare, trained = [], []
    for fn in (pipe.get_train_loss_dict, trainer_body):  # warm both
        loop(fn, step)
        step += STEPS
    for _ in range(ROUNDS):
        bare.append(loop(pipe.get_train_loss_dict, step))
        step += STEPS
        trained.append(loop(trainer_body, step))
        trainer.flush_logs(wait=True)
        step += STEPS
    ms_bare, ms_trainer = float(np.median([m for m, _ in bare])), float(np.median([m for m, _ in trained]))

    # (b), (c): the gradient of one more step, kept whole
    pipe.keep_gradient = True
    pipe.get_train_loss_dict(step)
    pipe.keep_gradient = False
    torch.cuda.synchronize()
    flat, layout = trainer.field.flat, trainer.field.layout
    grad = flat.grad.detach()
    out, dst = torch.empty(trainer.bounds.k, 3, dtype=torch.float64, device=dev), torch.empty_like(grad)
    ms_stats = _events_ms(lambda: ops.segment_stats(grad, trainer.bounds, out=out))
    ms_copy = _events_ms(lambda: dst.copy_(grad))
    views = [layout.view(grad, name) for name in layout.entries]

    def torch_norms():
        return [float(v.norm()) for v in views]  # a launch or two and a host read per parameter

    torch_norms()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        torch_norms()
    ms_torch = (time.perf_counter() - t0) / REPS * 1e3
    nbytes = grad.numel() * 4
    result = dict(
        scene="bench.sampler_scene(C2): 6 cameras of 64 x 64, 4096 rays per batch, 31 bands, 6 endmembers, specular, rgb+spectral",
        steps_per_round=STEPS, rounds=ROUNDS, logging_steps=10, log_gradients=True,
        bare_loop=dict(ms_per_step=round(ms_bare, 4), steps_per_s=round(1e3 / ms_bare, 1), wall_ms_per_step=round(float(np.median([w for _, w in bare])), 4),
                       rounds_ms=[round(m, 4) for m, _ in bare]),
        trainer_loop=dict(ms_per_step=round(ms_trainer, 4), steps_per_s=round(1e3 / ms_trainer, 1),
                          wall_ms_per_step=round(float(np.median([w for _, w in trained])), 4), rounds_ms=[round(m, 4) for m, _ in trained]),
        trainer_over_bare=round(ms_trainer / ms_bare, 4),
        gradient=dict(elements=int(grad.numel()), mbytes=round(nbytes / 1e6, 2), segments=trainer.bounds.k),
        segment_stats=dict(ms=round(ms_stats, 4), gbytes_per_s=round(nbytes / ms_stats / 1e6, 1)),
        device_copy=dict(ms=round(ms_copy, 4), gbytes_per_s_read=round(nbytes / ms_copy / 1e6, 1)),
        segment_stats_over_copy=round(ms_stats / ms_copy, 3),
        torch_per_parameter_norms=dict(ms=round(ms_torch, 4), note="view.norm() + host read per named parameter, wall clock"),
        torch_over_segment_stats=round(ms_torch / ms_stats, 1),
        note="ms per step between device events around each 300-step loop, median of 7 alternated rounds, both loops on the same "
             "pipeline; segment_stats and the copy between device events, median of 30",
    )
    os.makedirs(os.path.join(ROOT, "profiles", "train"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train", "bench_train.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
