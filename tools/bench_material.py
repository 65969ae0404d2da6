"""Material edits: the two kernels of csrc/umhs_material.hip against a copy of their bytes, and what an edit does to a rendered frame
(not bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process):
  remix_b<B>_<spec|nospec>_ms   ``ops.material_remix`` at 921,600 rays (one 1280 x 720 frame), 15 classes, B = 31 and 128 bands.  Bytes
                                per ray: 64 (mix16) + 4 B read and 4 B written without the specular head; 64 + 4 B read and 12 B
                                written with it
  copy_<same name>_ms           a device copy that moves as many bytes (half of them read, half written): the floor
  sigma_ms / copy_sigma_ms      ``ops.material_sigma`` at the sample count of one 1280 x 720 frame of the C2-shaped model (bench.py's
                                ``sampler_scene`` after 300 steps), C = 6: 4 (C + 2) bytes per sample
Model (the same scene; one camera, ``get_outputs_for_camera_ray_bundle`` with the base outputs a frame is composed from, rays
generated outside the clock), at 256 x 256 and 1280 x 720, alternated in one run:
  frame_<H>_plain_ms      unedited
  frame_<H>_recolour_ms   one replaced spectrum, one gain, specular_gain 0.5: the unedited frame + the remix + the colour conversion
  frame_<H>_remove_ms     one material's density at 0: one more transmittance scan, one more heads pass and the density kernel
Prints one JSON line and writes it to --out (default profiles/material/bench_material.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd")]
import torch

import bench
from umhsnerf import ops
from umhsnerf.materials import load_material_edits

DEV = torch.device("cuda", 0)
ROUNDS, RAYS, CLASSES = 7, 1280 * 720, 15
FRAMES = ((256, 256), (720, 1280))
NAMES = ["rgb", "spectral", "accumulation", "depth", "abundances", "seg_raw"]


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


def alternate(variants, rounds, reps, warm=3):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    t_ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t_ms[k].append(device_ms(fn, reps=reps))
    return {k: stats(v) for k, v in t_ms.items()}


def _copy(n_bytes):
    n = n_bytes // 8  # floats each way
    src, dst = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    return lambda: dst.copy_(src)


def kernel_part(rounds, n_samples, n_classes):
    g = torch.Generator().manual_seed(5)
    variants, traffic = {}, {}
    mix = torch.rand(RAYS, 16, generator=g).to(DEV)
    for B in (31, 128):
        E = torch.rand(CLASSES, B, generator=g).to(DEV)
        cs = torch.rand(RAYS, B, generator=g).to(DEV)
        for name, spec in (("nospec", None), ("spec", cs)):
            key = f"remix_b{B}_{name}"
            traffic[key] = RAYS * (64 + 4 * B) if spec is None else RAYS * (64 + 4 * B + 12 * B)
            variants[key + "_ms"] = lambda E=E, spec=spec: ops.material_remix(mix, spec, E, 0.5 if spec is not None else 1.0)
            variants["copy_" + key + "_ms"] = _copy(traffic[key])
    sigma = torch.rand(n_samples, device=DEV)  # (drawn on the device: a frame holds some 2e8 samples)
    ab = torch.softmax(torch.randn(n_samples, n_classes, device=DEV), -1)
    gain = torch.tensor([0.0] + [1.0] * (n_classes - 1), device=DEV)
    out = torch.empty_like(sigma)
    traffic["sigma"] = n_samples * 4 * (n_classes + 2)
    variants["sigma_ms"] = lambda: ops.material_sigma(sigma, ab, gain, out=out)
    variants["copy_sigma_ms"] = _copy(traffic["sigma"])
    res = alternate(variants, rounds, reps=5)
    res["rays"], res["classes"], res["sigma_samples"], res["sigma_classes"] = RAYS, CLASSES, n_samples, n_classes
    res["bytes_moved"] = traffic
    for key, nbytes in traffic.items():
        res[key + "_GBps"] = nbytes / res[key + "_ms"]["median"] / 1e6
        res[key + "_over_copy"] = res[key + "_ms"]["median"] / res["copy_" + key + "_ms"]["median"]
    return res


def _cameras(H, W):
    from umhsnerf.data.umhs_dataparser import Cameras

    g = torch.Generator().manual_seed(3)
    pos = torch.nn.functional.normalize(torch.randn(1, 3, generator=g), dim=-1) * 0.9  # the scene's cameras stand at radius 0.9
    z = torch.nn.functional.normalize(pos, dim=-1)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([[0.0, 0, 1]]), z), dim=-1)
    c2w = torch.stack([x, torch.linalg.cross(z, x), z, pos], -1).contiguous()
    f = torch.tensor([float(H)])  # (a 53 degree vertical field of view)
    return Cameras(c2w, f, f.clone(), torch.tensor([W / 2.0]), torch.tensor([H / 2.0]), H, W).to(DEV)


def model_part(rounds, pipe):
    model = pipe.model.eval()
    Cn, B = model.field.endmembers.shape
    spec = bool(model.config.pred_specular)
    recolour = load_material_edits({"materials": [{"material": 2, "spectrum": [0.5 + 0.4 * ((-1) ** b) for b in range(B)]},
                                                  {"material": 0, "gain": 0.4}], **({"specular_gain": 0.5} if spec else {})}, Cn, B, spec)
    remove = load_material_edits({"materials": [{"material": 1, "density": 0.0}]}, Cn, B, spec)
    res = {}
    for H, W in FRAMES:
        rays = _cameras(H, W).generate_rays(0, keep_shape=True)

        def frame(edits):
            with model.material_edits_context(edits):
                return model.get_outputs_for_camera_ray_bundle(rays, output_names=NAMES)

        variants = {f"frame_{H}_plain_ms": lambda: frame(None), f"frame_{H}_recolour_ms": lambda: frame(recolour),
                    f"frame_{H}_remove_ms": lambda: frame(remove)}
        res.update(alternate(variants, rounds, reps=1, warm=2))
        res[f"frame_{H}_samples"] = int(model.get_outputs_for_camera_ray_bundle(rays, output_names=["num_samples_per_ray"])[
            "num_samples_per_ray"].sum())
        for k in ("recolour", "remove"):
            res[f"frame_{H}_{k}_minus_plain_ms"] = res[f"frame_{H}_{k}_ms"]["median"] - res[f"frame_{H}_plain_ms"]["median"]
            res[f"frame_{H}_{k}_over_plain"] = res[f"frame_{H}_{k}_ms"]["median"] / res[f"frame_{H}_plain_ms"]["median"]
    pipe.model.train()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material", "bench_material.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    model = model_part(rounds, pipe)
    res = {"bench": "material", "device": torch.cuda.get_device_name(0), "rounds": rounds,
           "kernel": kernel_part(rounds, model["frame_720_samples"], bench.C2["C"]), "model": model}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
