"""Regional material edits: the five kernels of csrc/umhs_region.hip against a copy of their bytes, and what a regional edit adds to its
global counterpart on a rendered frame (a sibling of tools/bench_material.py, whose helpers and scene it uses).  GPU box.  Records, not
gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), at the sample count N of one
1280 x 720 frame of the C2-shaped model cut into runs of 40 samples (S = N / 40 segments and more, R = 921,600 rays), K = 1:
  classify_ms        ``umhs_region_classify``: 13 N bytes
  segments_ms        ``umhs_region_segments`` with its 8-byte read of S: 2 x 9 N read (flags, then ranks), 8 N + 20 S + 16 R written,
                     16 R + 8 S read by the finish pass
  sigma_regions_ms   ``umhs_material_sigma_regions``, C = 6: (4 (C + 2) + 1) N bytes
  segment_sum_ms     ``umhs_segment_sum`` of [S, B] rows, B = 31: 4 B S + (16 + 4 B) R bytes
  remix_regions_*_ms ``umhs_material_remix_regions``, 15 classes, B = 31 and 128, with the specular term: (68 + 4 B) S + (16 + 12 B) R
  copy_<name>_ms     a device copy that moves as many bytes: the floor
Model (one camera, ``get_outputs_for_camera_ray_bundle``, rays generated outside the clock), 256 x 256 and 1280 x 720, alternated:
  frame_<H>_plain_ms / _recolour_ms / _remove_ms   unedited and the two GLOBAL edits of tools/bench_material.py (the path an edit
                                                   without regions takes, which this tool's commit left as it was)
  frame_<H>_box_recolour_ms / _box_remove_ms       the same two edits inside one box of half the scene's extent
  frame_<H>_segments                               S summed over the frame's chunks under the box
Prints one JSON line and writes it to --out (default profiles/material/bench_regions.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

import bench
import bench_material as BM
from umhsnerf import ops
from umhsnerf.materials import load_material_edits

DEV = BM.DEV
RUN = 40
BOX = {"center": [0.0, 0.0, 0.0], "rotation": [0.0, 0.0, 0.0], "scale": [1.0, 1.0, 1.0]}  # half of the [-1, 1]^3 scene box


def kernel_part(rounds, n_samples, n_classes):
    R, N = BM.RAYS, n_samples
    per_ray = max(1, N // R)
    N = per_ray * R
    ray = torch.arange(R, device=DEV).repeat_interleave(per_ray)
    pinfo = torch.stack([torch.arange(R, device=DEV) * per_ray, torch.full((R,), per_ray, device=DEV)], 1).contiguous()
    region = ((torch.arange(N, device=DEV) // RUN) % 2).to(torch.uint8)
    wpos = torch.rand(N, 3, device=DEV) * 2.0 - 1.0
    table = np.zeros((1, 16), np.float32)
    table[0, 3:12], table[0, 12:15] = np.eye(3, dtype=np.float32).reshape(9), 1.0
    seg_of, seg_info, seg_layer, ray_seg, S = ops.region_segments(region, ray, pinfo)
    del seg_of, seg_info
    variants, traffic = {}, {}
    traffic["classify"] = 13 * N
    variants["classify_ms"] = lambda: ops.region_classify(wpos, table)
    traffic["segments"] = 26 * N + 28 * S + 32 * R
    variants["segments_ms"] = lambda: ops.region_segments(region, ray, pinfo)
    sigma = torch.rand(N, device=DEV)
    ab = torch.softmax(torch.randn(N, n_classes, device=DEV), -1)
    gains = torch.tensor([[1.0] * n_classes, [0.0] + [1.0] * (n_classes - 1)], device=DEV)
    out = torch.empty_like(sigma)
    traffic["sigma_regions"] = N * (4 * (n_classes + 2) + 1)
    variants["sigma_regions_ms"] = lambda: ops.material_sigma_regions(sigma, ab, region, gains, out=out)
    values = torch.rand(S, 31, device=DEV)
    traffic["segment_sum"] = 4 * 31 * S + (16 + 4 * 31) * R
    variants["segment_sum_ms"] = lambda: ops.segment_sum(values, ray_seg)
    mix = torch.rand(S, 16, device=DEV)
    for B in (31, 128):
        E = torch.rand(2, BM.CLASSES, B, device=DEV)
        cs = torch.rand(S, B, device=DEV)
        s = torch.tensor([0.5, 2.0], device=DEV)
        key = f"remix_regions_b{B}"
        traffic[key] = (68 + 4 * B) * S + (16 + 12 * B) * R
        variants[key + "_ms"] = lambda E=E, cs=cs: ops.material_remix_regions(mix, cs, seg_layer, ray_seg, E, s)
    for key, nbytes in traffic.items():
        variants["copy_" + key + "_ms"] = BM._copy(nbytes)
    res = BM.alternate(variants, rounds, reps=3)
    res.update(rays=R, samples=N, segments=S, run=RUN, classes=BM.CLASSES, sigma_classes=n_classes, bytes_moved=traffic)
    for key, nbytes in traffic.items():
        res[key + "_GBps"] = nbytes / res[key + "_ms"]["median"] / 1e6
        res[key + "_over_copy"] = res[key + "_ms"]["median"] / res["copy_" + key + "_ms"]["median"]
    return res


def model_part(rounds, pipe):
    model = pipe.model.eval()
    Cn, B = model.field.endmembers.shape
    spec = bool(model.config.pred_specular)
    recolour = {"materials": [{"material": 2, "spectrum": [0.5 + 0.4 * ((-1) ** b) for b in range(B)]}, {"material": 0, "gain": 0.4}],
                **({"specular_gain": 0.5} if spec else {})}
    remove = {"materials": [{"material": 1, "density": 0.0}]}
    load = lambda doc: load_material_edits(doc, Cn, B, spec)
    edits = {"plain": None, "recolour": load(recolour), "remove": load(remove),
             "box_recolour": load({"regions": [dict(recolour, box=BOX)]}), "box_remove": load({"regions": [dict(remove, box=BOX)]})}
    res = {}
    for H, W in BM.FRAMES:
        rays = BM._cameras(H, W).generate_rays(0, keep_shape=True)

        def frame(e):
            with model.material_edits_context(e):
                return model.get_outputs_for_camera_ray_bundle(rays, output_names=BM.NAMES)

        res.update(BM.alternate({f"frame_{H}_{k}_ms": (lambda e=e: frame(e)) for k, e in edits.items()}, rounds, reps=1, warm=2))
        counted, real = [], ops.region_segments

        def counting(*a):
            out = real(*a)
            counted.append(out[4])
            return out

        ops.region_segments = counting
        try:
            frame(edits["box_recolour"])
        finally:
            ops.region_segments = real
        res[f"frame_{H}_segments"], res[f"frame_{H}_chunks"] = int(sum(counted)), len(counted)
        res[f"frame_{H}_samples"] = int(model.get_outputs_for_camera_ray_bundle(rays, output_names=["num_samples_per_ray"])[
            "num_samples_per_ray"].sum())
        for k in ("recolour", "remove"):
            res[f"frame_{H}_box_{k}_minus_global_ms"] = res[f"frame_{H}_box_{k}_ms"]["median"] - res[f"frame_{H}_{k}_ms"]["median"]
            res[f"frame_{H}_box_{k}_over_global"] = res[f"frame_{H}_box_{k}_ms"]["median"] / res[f"frame_{H}_{k}_ms"]["median"]
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material", "bench_regions.json"))
    ap.add_argument("--rounds", type=int, default=BM.ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    model = model_part(rounds, pipe)
    res = {"bench": "material_regions", "device": torch.cuda.get_device_name(0), "rounds": rounds,
           "kernel": kernel_part(rounds, model["frame_720_samples"], bench.C2["C"]), "model": model}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
