"""Scene statistics: ``ops.gram_accumulate`` and ``ops.spectral_project`` (csrc/umhs_statistics.hip) against the torch compositions they
replace, a copy of their bytes and the matrix-core time of their products; and what ``--scene-statistics`` adds to a rendered frame (not
bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernels (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at 921,600 rows (one
1280 x 720 frame) x 31, 128 and 141 bands; the projection at K = B with P = 3:
  gram_b<B>_ms / project_b<B>_ms              the kernels (the projection on a prepared image, with the score)
  torch_gram_b<B>_ms / torch_project_b<B>_ms  ``c = x - mu; c.T @ c; c.sum(0)`` and ``((x - mu) @ W.T)`` then ``square().sum(1)``
  copy_gram_b<B>_ms / copy_project_b<B>_ms    a device copy of the bytes each reads and writes (gram: R B 4 read, the chunk partials
                                              written and read once; project: R B 4 + the image read, R (P + 1) 4 written)
  mfma_gram_b<B>_ms / mfma_project_b<B>_ms    2 R B B / 157.3 TFLOP/s (the full square: the kernel computes the upper tile triangle)
                                              and 2 R B K / 157.3 TFLOP/s: arithmetic, not a run
Model (bench.py's ``sampler_scene`` after 300 steps; one 1280 x 720 camera, ``get_outputs_for_camera_ray_bundle`` with the outputs a
frame of ``rgb`` / ``rgb pca_rgb rx_score`` is composed from, rays generated outside the clock), alternated in one run:
  frame_720_plain_ms / frame_720_statistics_ms   without and with the context; ``frame_720_statistics_minus_plain_ms`` = what it adds
Prints one JSON line and writes it to --out (default profiles/statistics/bench_statistics.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch

import bench
from bench_material import _cameras, alternate
from umhsnerf import ops
from umhsnerf.statistics import StatisticsAccumulator, first_frame_shift

DEV = torch.device("cuda", 0)
ROUNDS, ROWS = 7, 1280 * 720
BANDS = (31, 128, 141)
MFMA_F32_TFLOPS = 157.3


def kernel_part(rounds):
    g = torch.Generator().manual_seed(5)
    res = {"rows": ROWS}
    for B in BANDS:
        x = (torch.rand(ROWS, 3, generator=g) @ torch.rand(3, B, generator=g) / 3 + 0.01 * torch.randn(ROWS, B, generator=g)).to(DEV)
        mu = x[:4096].mean(0).contiguous()
        W = (torch.randn(B, B, generator=g) / B ** 0.5).to(DEV)
        image = ops.library_prepare(W)
        acc = torch.zeros(1 + B + B * B, dtype=torch.float64, device=DEV)
        gram_bytes = ROWS * B * 4 + 2 * -(-ROWS // ops.gram_chunk()) * (1 + B + B * B) * 4
        project_bytes = ROWS * B * 4 + image.numel() * 4 + ROWS * 4 * 4
        copies = {k: (torch.empty(n // 8, device=DEV), torch.empty(n // 8, device=DEV)) for k, n in (("gram", gram_bytes), ("project", project_bytes))}

        def torch_gram():
            c = x - mu
            return c.T @ c, c.sum(0)

        def torch_project():
            y = (x - mu) @ W.T
            return y[:, :3], y.square().sum(1)

        variants = {f"gram_b{B}_ms": lambda: ops.gram_accumulate(x, mu, acc), f"torch_gram_b{B}_ms": torch_gram,
                    f"copy_gram_b{B}_ms": lambda: copies["gram"][1].copy_(copies["gram"][0]),
                    f"project_b{B}_ms": lambda: ops.spectral_project(x, mu, image, B, 3), f"torch_project_b{B}_ms": torch_project,
                    f"copy_project_b{B}_ms": lambda: copies["project"][1].copy_(copies["project"][0])}
        res.update(alternate(variants, rounds, reps=2, warm=2))
        res[f"mfma_gram_b{B}_ms"] = res[f"mfma_project_b{B}_ms"] = 2.0 * ROWS * B * B / (MFMA_F32_TFLOPS * 1e12) * 1e3
        res[f"bytes_gram_b{B}"], res[f"bytes_project_b{B}"] = gram_bytes, project_bytes
        for k in ("gram", "project"):
            mine = res[f"{k}_b{B}_ms"]["median"]
            res[f"torch_{k}_b{B}_over_kernel"] = res[f"torch_{k}_b{B}_ms"]["median"] / mine
            res[f"{k}_b{B}_over_copy"] = mine / res[f"copy_{k}_b{B}_ms"]["median"]
            res[f"{k}_b{B}_over_mfma"] = mine / res[f"mfma_{k}_b{B}_ms"]
        # a record that both looked at the same thing: the largest relative difference of the two Gram matrices and of the scores
        acc.zero_()
        ops.gram_accumulate(x, mu, acc)
        G = acc[1 + B:].view(B, B)
        res[f"gram_b{B}_vs_torch"] = float((G - torch_gram()[0].double()).abs().max() / G.abs().max())
        score = ops.spectral_project(x, mu, image, B, 3)[1]
        res[f"project_b{B}_vs_torch"] = float((score - torch_project()[1]).abs().max() / score.abs().max())
        del x, copies
    return res


def model_part(rounds, pipe):
    model = pipe.model.eval()
    wl = [float(w) for w in model.kwargs["wavelengths"]]
    rays = _cameras(720, 1280).generate_rays(0, keep_shape=True)
    out = model.get_outputs_for_camera_ray_bundle(rays, output_names=["spectral", "accumulation"])
    accumulator = StatisticsAccumulator(len(wl), DEV, first_frame_shift(out["spectral"], out["accumulation"]))
    accumulator.add(out["spectral"], out["accumulation"])
    stats = accumulator.result(wl)

    def frame(s, names):
        with model.scene_statistics_context(s):
            return model.get_outputs_for_camera_ray_bundle(rays, output_names=names)

    res = alternate({"frame_720_plain_ms": lambda: frame(None, ["rgb"]),
                     "frame_720_statistics_ms": lambda: frame(stats, ["rgb", "pca_rgb", "rx_score"])}, rounds, reps=1, warm=2)
    plain, with_stats = res["frame_720_plain_ms"]["median"], res["frame_720_statistics_ms"]["median"]
    res.update(bands=len(wl), n=stats.n, frame_720_statistics_minus_plain_ms=with_stats - plain,
               frame_720_statistics_share=(with_stats - plain) / with_stats)
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistics", "bench_statistics.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    kernel = kernel_part(rounds)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    res = {"bench": "statistics", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel, "model": model_part(rounds, pipe)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
