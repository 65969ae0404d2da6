"""Density-gradient normals: the kernel against its yardsticks, and what the output costs an eval image and a point-cloud export (not
bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 5, the variants alternated inside one process).  N = 2^21 samples drawn as
rays (32,768 rays x 64 samples through the unit cube, contraction on), a C2 field (log2_T 19) with the table at U(-1, 1) x 0.1:
  normals_enc_ms       umhs_density_normals with the level-major features passed in (the render path's case)
  normals_gather_ms    the C entry point with enc = NULL: the kernel gathers the features itself first (all sixteen levels per lane)
  normals_op_ms        ops.density_normals without enc: umhs_hashgrid_fwd into a scratch, then the kernel with enc (what a caller gets)
  yardstick_ms         the parent's density query on the same samples: umhs_hashgrid_fwd + the density-only umhs_field_fwd -- one gather
                       and one pass of the same 32 -> 64 -> 16 network (hashgrid_ms and field_ms apart)
  bytes                what each must move once per sample: positions 12 (+ world position 12 + selector 4), features 128 read (or
                       written and read by the yardstick), 128 table fetches of 8 B = 1024 B from the L2 / Infinity Cache / HBM, the
                       [N,3] output 12; over the kernel time = achieved bytes/s (a gather rate, not an HBM rate: the table is 64 MiB)
  flops                2 x 2 x 64 x 32 per sample for the two products of the kernel (h and q), 2 x 64 x (32 + 16) for the yardstick's MLP
Model (bench.py's ``sampler_scene`` at C2 after 300 steps, as tools/bench_export.py):
  eval_image_ms        one 256 x 256 camera through get_outputs_for_camera_ray_bundle, without and with "normals" (host clock around a
                       device synchronise, alternated)
  export_ms            export_pointcloud of --num-points points on the six training cameras at 1024 x 1024, normal_method none / analytic
Prints one JSON line and writes it to --out."""
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
from umhsnerf import _hip, export, ops

DEV = torch.device("cuda", 0)
ROUNDS, RAYS, SAMPLES, SIDE = 7, 32768, 64, 1024


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


def kernel_part(rounds):
    cfg = bench.C2
    L = ops.FieldLayout(cfg["C"], cfg["B"], cfg["pred_specular"], 19)
    g = torch.Generator().manual_seed(1)
    flat = (torch.rand(L.total, generator=g) * 2 - 1) * 0.1
    flat = flat.to(DEV)
    spec = ops.FieldSpec(L, cfg["temperature"], True, scalings=ops.hash_scalings().to(DEV))
    n = RAYS * SAMPLES
    o = (torch.rand(RAYS, 1, 3, generator=g) * 2 - 1) * 1.5
    d = torch.nn.functional.normalize(torch.randn(RAYS, 1, 3, generator=g), dim=-1)
    t = torch.linspace(0.0, 3.0, SAMPLES).view(1, SAMPLES, 1)
    wpos_in = (o + d * t).reshape(n, 3).contiguous().to(DEV)
    wpos, pos01, sel = ops.positions_fwd(None, None, None, None, spec, world_pos_in=wpos_in)
    table = L.view(flat, "mlp_base.encoder.hash_table")
    enc = ops.hashgrid_fwd(pos01, table, spec.scalings, 19, True)
    enc2 = torch.empty_like(enc)
    normal = torch.empty(n, 3, device=DEV)
    w = [L.view(flat, "mlp_base.mlp.layers." + k) for k in ("0.weight", "0.bias", "1.weight", "1.bias")]

    def self_gather():
        _hip.check(_hip.lib().umhs_density_normals(_hip.ptr(pos01), _hip.ptr(wpos), _hip.ptr(sel), None, _hip.ptr(table), _hip.ptr(spec.scalings),
                                                   19, *(_hip.ptr(t) for t in w), 1, None, n, None, _hip.ptr(normal), None, _hip.stream()),
                   "umhs_density_normals")
        return {"normal": normal}

    variants = {
        "normals_enc_ms": lambda: ops.density_normals(spec, flat, pos01, wpos, sel, enc=enc),
        "normals_gather_ms": self_gather,
        "normals_op_ms": lambda: ops.density_normals(spec, flat, pos01, wpos, sel),
        "hashgrid_ms": lambda: ops.hashgrid_fwd(pos01, table, spec.scalings, 19, True, out=enc2),
        "field_ms": lambda: ops.field_fwd(spec, flat, enc, True, None, None, sel, density_only=True, want_emb=False),
    }
    same = torch.equal(variants["normals_enc_ms"]()["normal"], variants["normals_gather_ms"]()["normal"].clone())
    for fn in variants.values():  # warm
        for _ in range(3):
            fn()
    t_ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t_ms[k].append(device_ms(fn, reps=5))
    res = {k: stats(v) for k, v in t_ms.items()}
    res["yardstick_ms"] = {"median": res["hashgrid_ms"]["median"] + res["field_ms"]["median"], "min": res["hashgrid_ms"]["min"] + res["field_ms"]["min"]}
    by = {"normals_enc": 12 + 12 + 4 + 128 + 1024 + 12, "normals_gather": 12 + 12 + 4 + 2 * 1024 + 12, "yardstick": 12 + 1024 + 128 + 128 + 4 + 4}
    fl = {"normals_enc": 2 * 2 * 64 * 32, "normals_gather": 2 * 2 * 64 * 32, "yardstick": 2 * 64 * (32 + 16)}
    res["samples"], res["live_share"], res["enc_and_gather_bits_equal"] = n, float(sel.mean()), bool(same)
    res["bytes_per_sample"], res["flop_per_sample"] = by, fl
    for k in by:
        ms = res[k + "_ms"]["median"]
        res[k + "_GBps"], res[k + "_TFLOPs"] = n * by[k] / ms / 1e6, n * fl[k] / ms / 1e9
    res["normals_enc_over_yardstick"] = res["normals_enc_ms"]["median"] / res["yardstick_ms"]["median"]
    res["normals_gather_over_yardstick"] = res["normals_gather_ms"]["median"] / res["yardstick_ms"]["median"]
    res["normals_op_over_yardstick"] = res["normals_op_ms"]["median"] / res["yardstick_ms"]["median"]
    return res


def model_part(rounds, n_points):
    from umhsnerf.data.umhs_datamanager import ResidentSplit
    from umhsnerf.data.umhs_dataparser import Cameras

    pipe, c2w = bench.sampler_scene(bench.C2, DEV)
    res = {}
    # ---- an eval image -------------------------------------------------------------------------------------------------------------
    Hh = 256
    f = 30.0 * Hh / 64.0
    cams = Cameras(c2w[:1].clone(), torch.full((1,), f), torch.full((1,), f), torch.full((1,), Hh / 2), torch.full((1,), Hh / 2), Hh, Hh)
    rb = ResidentSplit(cams, torch.zeros(1, Hh, Hh, 3), None, DEV).image_rays(0)
    m = pipe.model.eval()
    names = ["rgb", "depth", "accumulation", "spectral", "abundances", "seg_pred"]
    run = {"eval_image_ms": lambda: m.get_outputs_for_camera_ray_bundle(rb, output_names=names),
           "eval_image_normals_ms": lambda: m.get_outputs_for_camera_ray_bundle(rb, output_names=names + ["normals"])}
    for fn in run.values():
        for _ in range(2):
            fn()
    t_ms = {k: [] for k in run}
    for _ in range(rounds):
        for k, fn in run.items():
            t_ms[k].append(host_ms(fn)[0])
    res.update({k: stats(v) for k, v in t_ms.items()})
    out = run["eval_image_normals_ms"]()
    res["eval_image_samples"] = int(m.get_outputs_for_camera_ray_bundle(rb, output_names=["num_samples_per_ray"])["num_samples_per_ray"].sum())
    hit = out["accumulation"].view(-1) > 0.5
    dots = ((out["normals"].view(-1, 3) * 2 - 1) * rb.directions.view(-1, 3).to(DEV)).sum(-1)[hit]
    res["eval_image_opaque_pixels"], res["facing_camera_share"] = int(hit.sum()), float((dots < 0).float().mean())
    res["median_n_dot_d"] = float(dots.median())
    pipe.model.train()
    # ---- the export ----------------------------------------------------------------------------------------------------------------
    n, fs = c2w.shape[0], 30.0 * SIDE / 64.0
    cams = Cameras(c2w.clone(), torch.full((n,), fs), torch.full((n,), fs), torch.full((n,), SIDE / 2), torch.full((n,), SIDE / 2), SIDE, SIDE)
    pipe.datamanager.train_split = ResidentSplit(cams, torch.zeros(n, SIDE, SIDE, 3, dtype=torch.uint8), None, DEV)
    with tempfile.TemporaryDirectory() as tmp:
        export.export_pointcloud(pipe, tmp, num_points=65536, normal_method="analytic")  # warm up
        t_ms = {"none": [], "analytic": []}
        parts = {"none": {}, "analytic": {}}
        for _ in range(max(3, rounds // 2)):
            for method in t_ms:
                timings = {}
                ms, info = host_ms(lambda: export.export_pointcloud(pipe, tmp, num_points=n_points, normal_method=method, timings=timings))
                t_ms[method].append(ms)
                for k, v in timings.items():
                    parts[method].setdefault(k, []).append(v * 1e3)
                res.setdefault("export_file_bytes", {})[method] = os.path.getsize(info["file"])
        res["export_ms"] = {k: stats(v) for k, v in t_ms.items()}
        res["export_parts_ms"] = {mth: {k: stats(v) for k, v in p.items()} for mth, p in parts.items()}
        res["export"] = {k: info[k] for k in ("points", "rays_drawn", "batches", "removed_outliers")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--num-points", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    res = {"bench": "normals", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel_part(rounds)}
    if not args.kernel_only:
        res["model"] = model_part(rounds, args.num_points)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
