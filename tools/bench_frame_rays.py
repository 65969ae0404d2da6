"""Whole-frame ray generation: ``umhs_raygen_frame`` against the path it replaces and against a copy, and what a crop box does to a
rendered frame (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process), one 1280 x 720 frame:
  parent_ms            what ``Cameras.generate_rays`` did before: meshgrid / stack / reshape into a [H*W,3] int64 index tensor (24 B per
                       pixel, several torch launches), then ``umhs_raygen`` on it (parent_index_ms and parent_kernel_ms apart)
  frame_<type>_ms      ``ops.raygen_frame`` for perspective / fisheye / equirectangular, without a box
  frame_<type>_box_ms  the same with a crop box (nears / fars written too)
  copy_ms              a device copy of as many bytes as the kernel writes without a box (origins 12 + directions 12 + pixel_area 4 +
                       directions_norm 4 = 32 B per ray; 40 B with a box, copy_box_ms): the floor of a kernel that only writes
Model (bench.py's ``sampler_scene`` at C2 after 300 steps, as tools/bench_normals.py), one 1280 x 720 camera path frame through
``render_camera_path`` (host clock around the whole call: rays, outputs, composition, PNG encoding), alternated:
  render_frame_ms          uncropped
  render_frame_cropped_ms  cropped to a box of half the scene's extent (scale 1 about the origin of the +-1 scene box)
Prints one JSON line and writes it to --out (default profiles/frame_rays/bench_frame_rays.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd")]
import torch

import bench
from umhsnerf import ops
from umhsnerf.export import obb_from_params

DEV = torch.device("cuda", 0)
ROUNDS, H, W = 7, 720, 1280
TYPES = ("perspective", "fisheye", "equirectangular")


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "n": len(v)}


def device_ms(fn, reps=1):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _camera():
    g = torch.Generator().manual_seed(3)
    pos = torch.nn.functional.normalize(torch.randn(1, 3, generator=g), dim=-1) * 3.0
    z = torch.nn.functional.normalize(pos, dim=-1)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([[0.0, 0, 1]]), z), dim=-1)
    return torch.stack([x, torch.linalg.cross(z, x), z, pos], -1).contiguous()


def _intrinsics(camera_type):
    f = (H / 2.0) / 0.5  # (a 53 degree vertical field of view)
    fx, fy = (W / 2.0, float(H)) if camera_type == "equirectangular" else (f, f)
    return torch.tensor([[fx, fy, W / 2.0, H / 2.0]])


def kernel_part(rounds):
    c2w = _camera().to(DEV)
    intr = {t: _intrinsics(t).to(DEV) for t in TYPES}
    box = obb_from_params((0.1, -0.05, 0.2), (0.3, -0.2, 0.5), (0.9, 0.6, 1.2))
    n = H * W

    def index_tensor():
        yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
        return torch.stack([torch.full_like(yy, 0), yy, xx], -1).reshape(-1, 3).contiguous()

    idx = index_tensor()
    src, dst = torch.empty(n * 8, device=DEV), torch.empty(n * 8, device=DEV)
    src_box, dst_box = torch.empty(n * 10, device=DEV), torch.empty(n * 10, device=DEV)
    variants = {
        "parent_ms": lambda: ops.raygen(index_tensor(), c2w, intr["perspective"], want_area=True, want_norm=True),
        "parent_index_ms": index_tensor,
        "parent_kernel_ms": lambda: ops.raygen(idx, c2w, intr["perspective"], want_area=True, want_norm=True),
        "copy_ms": lambda: dst.copy_(src),
        "copy_box_ms": lambda: dst_box.copy_(src_box),
    }
    for t in TYPES:
        variants[f"frame_{t}_ms"] = lambda t=t: ops.raygen_frame(c2w, intr[t], 0, H, W, camera_type=t)
        variants[f"frame_{t}_box_ms"] = lambda t=t: ops.raygen_frame(c2w, intr[t], 0, H, W, camera_type=t, obb=box, near_floor=0.05)
    same = all(torch.equal(a, b) for a, b in zip(variants["parent_ms"](), variants["frame_perspective_ms"]()[:4]))
    for fn in variants.values():  # warm
        for _ in range(3):
            fn()
    t_ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t_ms[k].append(device_ms(fn, reps=5))
    res = {k: stats(v) for k, v in t_ms.items()}
    res["rays"], res["frame_equals_parent_bits"] = n, bool(same)
    res["bytes_written_per_ray"] = {"no_box": 32, "box": 40}
    res["parent_index_bytes_per_ray"] = 24
    for t in TYPES:
        res[f"frame_{t}_GBps"] = n * 32 / res[f"frame_{t}_ms"]["median"] / 1e6
        res[f"frame_{t}_over_copy"] = res[f"frame_{t}_ms"]["median"] / res["copy_ms"]["median"]
        res[f"frame_{t}_box_over_copy"] = res[f"frame_{t}_box_ms"]["median"] / res["copy_box_ms"]["median"]
    res["parent_over_frame"] = res["parent_ms"]["median"] / res["frame_perspective_ms"]["median"]
    return res


def model_part(rounds):
    from umhsnerf.data.umhs_dataparser import Cameras
    from umhsnerf.render import render_camera_path

    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    c2w = _camera()
    c2w[:, :, 3] *= 0.9 / 3.0  # the scene's cameras stand at radius 0.9
    cams = Cameras(c2w, *(_intrinsics("perspective")[:, k].clone() for k in range(4)), H, W).to(DEV)
    crop = {"obb": obb_from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), "background_color": [0.15, 0.15, 0.15]}
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        run = {"render_frame_ms": lambda: render_camera_path(pipe, cams, tmp, ["rgb"]),
               "render_frame_cropped_ms": lambda: render_camera_path(pipe, cams, tmp, ["rgb"], crop=crop)}
        for fn in run.values():
            for _ in range(2):
                fn()
        t_ms = {k: [] for k in run}
        for _ in range(rounds):
            for k, fn in run.items():
                t_ms[k].append(host_ms(fn)[0])
    res.update({k: stats(v) for k, v in t_ms.items()})
    m = pipe.model.eval()
    count = lambda **kw: int(m.get_outputs_for_camera_ray_bundle(cams.generate_rays(0, **kw), output_names=["num_samples_per_ray"])[
        "num_samples_per_ray"].sum())
    res["samples"] = {"uncropped": count(), "cropped": count(obb_box=crop["obb"], near_floor=float(m.config.near_plane))}
    rb = cams.generate_rays(0, obb_box=crop["obb"], near_floor=float(m.config.near_plane))
    res["rays_that_hit_the_box_share"] = float((rb.nears < 1e10).float().mean())
    res["cropped_over_uncropped"] = res["render_frame_cropped_ms"]["median"] / res["render_frame_ms"]["median"]
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_rays", "bench_frame_rays.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    res = {"bench": "frame_rays", "device": torch.cuda.get_device_name(0), "rounds": rounds, "height": H, "width": W,
           "kernel": kernel_part(rounds)}
    if not args.kernel_only:
        res["model"] = model_part(rounds)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
