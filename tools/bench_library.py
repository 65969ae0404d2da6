"""Spectral library matching: ``ops.library_match`` (csrc/umhs_library.hip) against the torch composition it replaces, a copy of its
bytes and the matrix-core time of its products; and what the match adds to a rendered frame (not bench.py: that measures the training
step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at 921,600 rays (one
1280 x 720 frame) x (31 bands, 256 entries), (141, 2048) and (128, 1024):
  match_b<B>_l<L>_ms    ``ops.library_match`` on a prepared image
  torch_b<B>_l<L>_ms    (a) ``normalize`` + ``matmul`` + ``topk(2)``: what one would write without the kernel; it forms the [R,L] matrix
  copy_b<B>_l<L>_ms     (b) a device copy of the bytes the kernel reads and writes (R B 4 + the image read, 16 R written)
  mfma_b<B>_l<L>_ms     (c) 2 R B L / 157.3 TFLOP/s, the fp32-input MFMA rate of the microarchitecture guide: arithmetic, not a run
Model (bench.py's ``sampler_scene`` after 300 steps; one 1280 x 720 camera, ``get_outputs_for_camera_ray_bundle`` with the outputs a
frame of ``rgb`` / ``rgb library_pred`` is composed from, rays generated outside the clock), alternated in one run:
  frame_720_plain_ms / frame_720_library_ms   without and with a 2,048-entry library; ``frame_720_library_share`` = what the match adds
Prints one JSON line and writes it to --out (default profiles/library/bench_library.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch

import bench
from bench_material import _cameras, alternate
from umhsnerf import ops
from umhsnerf.library import SpectralLibrary

DEV = torch.device("cuda", 0)
ROUNDS, RAYS = 7, 1280 * 720
SHAPES = ((31, 256), (141, 2048), (128, 1024))
MFMA_F32_TFLOPS = 157.3


def _unit(L, B, g):
    lib = torch.rand(L, B, generator=g, dtype=torch.float64) * 0.9 + 0.05
    return (lib / lib.norm(dim=1, keepdim=True)).float()


def kernel_part(rounds):
    g = torch.Generator().manual_seed(5)
    res = {"rays": RAYS}
    for B, L in SHAPES:
        key = f"b{B}_l{L}"
        unit = _unit(L, B, g).to(DEV)
        spectra = torch.rand(RAYS, B, generator=g).to(DEV)
        image = ops.library_prepare(unit)
        nbytes = RAYS * B * 4 + image.numel() * 4 + RAYS * 16
        src, dst = torch.empty(nbytes // 8, device=DEV), torch.empty(nbytes // 8, device=DEV)

        def composition():
            cos = torch.nn.functional.normalize(spectra, dim=1) @ unit.T
            return torch.topk(cos, 2, dim=1)

        variants = {f"match_{key}_ms": lambda: ops.library_match(spectra, image, L), f"torch_{key}_ms": composition,
                    f"copy_{key}_ms": lambda: dst.copy_(src)}
        res.update(alternate(variants, rounds, reps=2, warm=2))
        match = res[f"match_{key}_ms"]["median"]
        res[f"mfma_{key}_ms"] = 2.0 * RAYS * B * L / (MFMA_F32_TFLOPS * 1e12) * 1e3
        res[f"bytes_{key}"] = nbytes
        res[f"match_{key}_TFLOPs"] = 2.0 * RAYS * B * L / match / 1e9
        res[f"torch_{key}_over_match"] = res[f"torch_{key}_ms"]["median"] / match
        res[f"match_{key}_over_copy"] = match / res[f"copy_{key}_ms"]["median"]
        res[f"match_{key}_over_mfma"] = match / res[f"mfma_{key}_ms"]
        agree = (ops.library_match(spectra, image, L)[0][:, 0].long() == composition().indices[:, 0]).float().mean()
        res[f"agree_{key}"] = float(agree)  # (float32 ties may differ; a record that both looked at the same thing)
        del src, dst, spectra
    return res


def model_part(rounds, pipe):
    model = pipe.model.eval()
    B = model.field.endmembers.shape[1]
    wl = [float(w) for w in model.kwargs["wavelengths"]]
    rng = np.random.default_rng(7)
    library = SpectralLibrary([f"e{i}" for i in range(2048)], rng.random((2048, B)) * 0.9 + 0.05, wl)
    rays = _cameras(720, 1280).generate_rays(0, keep_shape=True)

    def frame(lib, names):
        with model.spectral_library_context(lib):
            return model.get_outputs_for_camera_ray_bundle(rays, output_names=names)

    res = alternate({"frame_720_plain_ms": lambda: frame(None, ["rgb"]), "frame_720_library_ms": lambda: frame(library, ["rgb", "library_pred"])},
                    rounds, reps=1, warm=2)
    plain, with_library = res["frame_720_plain_ms"]["median"], res["frame_720_library_ms"]["median"]
    res.update(bands=B, entries=2048, frame_720_library_minus_plain_ms=with_library - plain,
               frame_720_library_share=(with_library - plain) / with_library)
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "library", "bench_library.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    kernel = kernel_part(rounds)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    res = {"bench": "library", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel, "model": model_part(rounds, pipe)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
