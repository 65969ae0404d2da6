"""Point-cloud export, stage by stage (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Model: bench.py's ``sampler_scene`` at C2 (31 bands, 6 classes, pred_specular) after 300 training steps, as tools/bench_render.py.
Its training cameras hold 6 x 64 x 64 = 24,576 pixels; 10^6 draws with replacement would be ~40 exact copies of every point, which the
outlier rule drops (more copies than neighbours: a mean distance of 0) and which is no neighbour search to time.  The export is
therefore run on the SAME six cameras at 1024 x 1024 (6.3 M pixels): the model and the rays' geometry are the training ones.

Measured, warm, median (and min) of ROUNDS >= 5, the variants alternated inside one process:
  knn_kernel_ms   umhs_knn_mean_dist alone on 10^6 kept points (k = 20), device events
  knn_total_ms    ops.knn_mean_dist: grid (reads the bounding box back), binning, sort, cell table, the kernel, scatter; host clock
  tree_query_ms   scipy cKDTree(points).query(points, k=20, workers=16) on the host, the same points; tree_build_ms the construction;
                  d2h_ms the copy of the points to the host -- stated apart: it is what a user without the kernel pays first
  emit_ms         ops.pc_append on one rendered batch of 32,768 rays (count + scan + emit), device events
  torch_emit_ms   the same selection and packing with torch ops (boolean mask, index, casts, cat), device events; torch_equal
  export          the whole export_pointcloud of 10^6 points end to end, split into render / emit / neighbours / write (each behind a
                  device synchronisation, so the parts do not overlap and add up to slightly more than an unsplit run)
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
import numpy as np
import torch

import bench
from umhsnerf import export, ops
from umhsnerf.data.umhs_datamanager import ResidentSplit
from umhsnerf.data.umhs_dataparser import Cameras

DEV = torch.device("cuda", 0)
ROUNDS, K, RAYS, SIDE = 5, 20, 32768, 1024


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "n": len(v)}


def device_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_emit(rays, out, threshold=0.5):
    """The keep rule and the row packing of one batch with torch ops -> uint8 [K, 20 + 4 C]."""
    p = rays.directions * out["depth"] + rays.origins
    acc = out["accumulation"]
    keep = (acc[:, 0] > threshold) & torch.isfinite(p).all(dim=1)
    idx = torch.nonzero(keep)[:, 0]
    colour = (torch.cat([out["rgb"][idx], acc[idx]], dim=1).clamp(0, 1).nan_to_num(nan=0.0) * 255.0).to(torch.uint8)
    label = torch.argmax(out["seg_probs"][idx], dim=1).to(torch.int32)
    return torch.cat([p[idx].contiguous().view(torch.uint8), colour, label.view(-1, 1).view(torch.uint8),
                      out["abundances"][idx].contiguous().view(torch.uint8)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--num-points", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    n_points, rounds = args.num_points, max(args.rounds, 5)
    pipe, c2w = bench.sampler_scene(bench.C2, DEV)
    n, f = c2w.shape[0], 30.0 * SIDE / 64.0
    cams = Cameras(c2w.clone(), torch.full((n,), f), torch.full((n,), f), torch.full((n,), SIDE / 2), torch.full((n,), SIDE / 2), SIDE, SIDE)
    pipe.datamanager.train_split = ResidentSplit(cams, torch.zeros(n, SIDE, SIDE, 3, dtype=torch.uint8), None, DEV)
    res = {"bench": "export", "model": {"bands": bench.C2["B"], "classes": bench.C2["C"], "pred_specular": True}, "k": K,
           "num_points": n_points, "rays_per_batch": RAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the points: one export without outlier removal, read back from its file (model frame) --------------------------------
        export.export_pointcloud(pipe, tmp, num_points=min(n_points, 65536), num_rays_per_batch=RAYS)  # warm up
        first_ms, info = host_ms(lambda: export.export_pointcloud(pipe, tmp, num_points=n_points, num_rays_per_batch=RAYS, remove_outliers=False))
        raw = np.fromfile(info["file"], dtype=np.uint8)
        row = ops.pc_row_bytes(bench.C2["C"])
        table = raw[raw.size - n_points * row:].reshape(n_points, row)
        points = torch.from_numpy(np.ascontiguousarray(table[:, :12]).view(np.float32).reshape(n_points, 3).copy()).to(DEV)
        res["kept_fraction"] = n_points / info["rays_drawn"]
        res["distinct_points"] = int(torch.unique(points, dim=0).shape[0])

        # ---- neighbour search: the kernel, the whole op, the host tree -- alternated ---------------------------------------------
        from scipy.spatial import cKDTree

        plan = ops.knn_plan(points)
        res["grid"] = {"edge": plan["edge"], "dims": list(plan["dims"])}
        out = torch.empty(n_points, device=DEV)
        ops.knn_search(plan, K, out=out)
        t = {k: [] for k in ("knn_kernel_ms", "knn_total_ms", "d2h_ms", "tree_build_ms", "tree_query_ms")}
        for _ in range(rounds):
            t["knn_kernel_ms"].append(device_ms(lambda: ops.knn_search(plan, K, out=out)))
            ms, mean = host_ms(lambda: ops.knn_mean_dist(points, K))
            t["knn_total_ms"].append(ms)
            ms, host = host_ms(lambda: points.cpu().numpy())
            t["d2h_ms"].append(ms)
            ms, tree = host_ms(lambda: cKDTree(host))
            t["tree_build_ms"].append(ms)
            ms, (dist, _) = host_ms(lambda: tree.query(host, k=K, workers=16))
            t["tree_query_ms"].append(ms)
        res.update({k: stats(v) for k, v in t.items()})
        want = dist.astype(np.float64).mean(axis=1)
        err = np.abs(mean.cpu().numpy().astype(np.float64) - want)
        res["knn_max_err_over_bound"] = float((err / np.maximum((K + 8) * 2.0 ** -24 * want, 1e-300))[want > 0].max())
        res["zero_means"] = int((want == 0).sum())

        # ---- emit: the kernel pair against torch ops on one rendered batch -------------------------------------------------------
        model, split = pipe.model, pipe.datamanager.train_split
        model.eval()
        gen = torch.Generator(device=DEV)
        gen.manual_seed(0)
        with torch.no_grad():
            rays, _ = split.sample(RAYS, gen, want_batch=False)
            o = model(rays)
            rows = torch.empty(RAYS * row, dtype=torch.uint8, device=DEV)
            pts, kept = torch.empty(RAYS, 3, device=DEV), torch.empty(RAYS, dtype=torch.int64, device=DEV)
            base = torch.zeros(1, dtype=torch.int64, device=DEV)

            def hip_emit():
                a = ops.pc_args(rays.origins, rays.directions, o["depth"], o["accumulation"], o["rgb"], o["abundances"], o["seg_probs"])
                return ops.pc_append(a, rows, pts, kept, base, 0, RAYS)

            cnt = int(hip_emit())
            ref = torch_emit(rays, o)
            res["emit_kept"] = cnt
            res["torch_equal"] = bool(ref.shape[0] == cnt and torch.equal(ref.view(-1), rows[:cnt * row]))
            t = {"emit_ms": [], "torch_emit_ms": []}
            for _ in range(max(rounds, 10)):
                t["emit_ms"].append(device_ms(hip_emit))
                t["torch_emit_ms"].append(device_ms(lambda: torch_emit(rays, o)))
            res.update({k: stats(v) for k, v in t.items()})
        model.train()

        # ---- the whole export ------------------------------------------------------------------------------------------------------
        parts = {k: [] for k in ("total", "render", "emit", "neighbours", "write", "unsplit_total")}
        for _ in range(rounds if first_ms < 15e3 else 1):  # (a scene that keeps few rays per batch: one round, and "n" says so)
            timings = {}
            ms, info = host_ms(lambda: export.export_pointcloud(pipe, tmp, num_points=n_points, num_rays_per_batch=RAYS, timings=timings))
            parts["total"].append(ms)
            for k, v in timings.items():
                parts[k].append(v * 1e3)
            ms, _ = host_ms(lambda: export.export_pointcloud(pipe, tmp, num_points=n_points, num_rays_per_batch=RAYS))
            parts["unsplit_total"].append(ms)
        res["export_ms"] = {k: stats(v) for k, v in parts.items()}
        res["export"] = {k: info[k] for k in ("points", "rays_drawn", "batches", "removed_outliers", "threshold")}
        res["file_bytes"] = os.path.getsize(info["file"])
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
