"""Continuum removal: ``ops.continuum`` (csrc/umhs_continuum.hip) against a copy of its bytes and the host numpy function; and what
``cr_<b>`` and ``feature_depth_0`` add to a rendered frame (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at 921,600 rows (one
1280 x 720 frame) x 31, 128 and 141 bands on uniform wavelengths; eight feature windows of about B / 4 bands spread over the range;
three row kinds: ``smooth`` (three sinusoids over a slope: a handful of vertices), ``sawtooth`` (alternating bands: every low band is
pushed and popped, yet the hull keeps few vertices, so it is NOT the expensive kind) and ``dome`` (a concave arch with a per-row
amplitude: every band a vertex, the deepest stack and a new segment at every band of the evaluation -- the costly case of the three):
  continuum_<kind>_<mode>_b<B>_ms   the kernel; mode ``removed`` ([R,B] alone), ``features`` (8 features alone: no full-range hull) or
                                    ``both``
  copy_<mode>_b<B>_ms               a device copy of the bytes that mode reads and writes
  host_numpy_<kind>_b<B>_ms         ``umhsnerf.continuum.continuum_removed`` over a 4,000-row sample on 16 host threads, scaled to 921,600
  vertices_<kind>_b<B>              the mean and the largest number of vertices of the full-range hull
Model (bench.py's ``sampler_scene`` after 300 steps; one 1280 x 720 camera, rays generated outside the clock), alternated in one run:
  frame_720_plain_ms / frame_720_continuum_ms   ``rgb`` alone, and ``rgb cr_<B/2> feature_depth_0`` under ``continuum_context``
Prints one JSON line and writes it to --out (default profiles/continuum/bench_continuum.json)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch

import bench
from bench_material import _cameras, alternate
from umhsnerf import ops
from umhsnerf.continuum import ContinuumAnalysis, continuum_removed
from umhsnerf.library import scene_wavelengths

DEV = torch.device("cuda", 0)
ROUNDS, ROWS = 7, 1280 * 720
BANDS = (31, 128, 141)
HOST_ROWS, HOST_THREADS = 4000, 16


def windows(B):
    """Eight inclusive band ranges of about B / 4 bands, spread over the range."""
    w = max(B // 4, 3)
    return [(lo, lo + w - 1) for lo in (int(round(k * (B - w) / 7.0)) for k in range(8))]


def rows_of(kind, B, g):
    t = torch.linspace(0.0, 1.0, B)
    if kind == "smooth":
        f, p = 0.5 + 3.5 * torch.rand(ROWS, 3, 1, generator=g), torch.rand(ROWS, 3, 1, generator=g)
        x = 0.5 + 0.2 * t + (0.1 * torch.sin(2 * np.pi * (f * t + p))).sum(1)
    elif kind == "dome":
        x = 0.2 + (0.3 + 0.5 * torch.rand(ROWS, 1, generator=g)) * torch.sin(np.pi * (0.05 + 0.9 * t))
    else:
        x = 0.2 + 0.5 * (torch.arange(B) % 2) + 0.1 * t + 0.05 * torch.rand(ROWS, 1, generator=g)
    return x.float().contiguous().to(DEV)


def host_part(x, lam):
    rows = x[:HOST_ROWS].cpu().numpy()
    chunks = np.array_split(rows, HOST_THREADS)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        list(pool.map(lambda c: continuum_removed(c, lam), chunks))
    return (time.perf_counter() - t0) * 1e3 * ROWS / HOST_ROWS


def kernel_part(rounds):
    g = torch.Generator().manual_seed(5)
    res = {"rows": ROWS}
    for B in BANDS:
        lam = np.linspace(400.0, 1000.0, B).astype(np.float32)
        lam_d, ranges = torch.from_numpy(lam).to(DEV), windows(B)
        F = len(ranges)
        xs = {kind: rows_of(kind, B, g) for kind in ("smooth", "sawtooth", "dome")}
        modes = {"removed": ((), True, ROWS * B * 8), "features": (ranges, False, ROWS * (B + 3 * F) * 4),
                 "both": (ranges, True, ROWS * (2 * B + 3 * F) * 4)}
        variants, copies = {}, []
        for mode, (rg, want, nbytes) in modes.items():
            src, dst = torch.empty(nbytes // 8, device=DEV), torch.empty(nbytes // 8, device=DEV)
            copies.append((src, dst))
            variants[f"copy_{mode}_b{B}_ms"] = lambda src=src, dst=dst: dst.copy_(src)
            for kind, x in xs.items():
                variants[f"continuum_{kind}_{mode}_b{B}_ms"] = lambda x=x, rg=rg, want=want: ops.continuum(x, lam_d, rg, want_removed=want)
        res.update(alternate(variants, rounds, reps=1, warm=2))
        res[f"windows_b{B}"] = ranges
        for mode, (_, _, nbytes) in modes.items():
            res[f"bytes_{mode}_b{B}"] = nbytes
            for kind in xs:
                res[f"continuum_{kind}_{mode}_b{B}_over_copy"] = (res[f"continuum_{kind}_{mode}_b{B}_ms"]["median"]
                                                                   / res[f"copy_{mode}_b{B}_ms"]["median"])
        for kind, x in xs.items():
            status = ops.continuum(x, lam_d, (), want_removed=False, want_status=True)[2]
            res[f"vertices_{kind}_b{B}"] = [float(status.float().mean()), int(status.max())]
            res[f"host_numpy_{kind}_b{B}_ms"] = host_part(x, lam)
        del xs, copies, variants
    return res


def model_part(rounds, pipe):
    model = pipe.model.eval()
    rays = _cameras(720, 1280).generate_rays(0, keep_shape=True)
    wl = scene_wavelengths(model)
    B = len(wl)
    analysis = ContinuumAnalysis(wl, [("feature", (wl[B // 4], wl[(3 * B) // 4]))])
    names = ["rgb", f"cr_{B // 2}", "feature_depth_0"]

    def frame(a, out):
        with model.continuum_context(a):
            return model.get_outputs_for_camera_ray_bundle(rays, output_names=out)

    res = alternate({"frame_720_plain_ms": lambda: frame(None, ["rgb"]), "frame_720_continuum_ms": lambda: frame(analysis, names)},
                    rounds, reps=1, warm=2)
    plain, with_cr = res["frame_720_plain_ms"]["median"], res["frame_720_continuum_ms"]["median"]
    out = frame(analysis, ["feature_depth_0", "accumulation"])
    shown = out["accumulation"] > 0.5
    res.update(bands=B, names=names, ranges=analysis.ranges, frame_720_continuum_minus_plain_ms=with_cr - plain,
               frame_720_continuum_share=(with_cr - plain) / with_cr, rendered_share=float(shown.float().mean()),
               mean_depth=float(out["feature_depth_0"][shown].mean()) if bool(shown.any()) else None)
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continuum", "bench_continuum.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    kernel = kernel_part(rounds)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    res = {"bench": "continuum", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel, "model": model_part(rounds, pipe)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
