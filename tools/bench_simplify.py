"""Mesh simplification: ``ops.mesh_simplify`` and the ``--simplify-faces`` search against a copy of the bytes they read and write, and the
whole textured export with and without the flag (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Mesh: bench.py's ``sampler_scene`` at C2 after 300 steps, its six cameras at 512 x 512 as tools/bench_mesh.py, fused and extracted at
``--resolutions`` (default 128 and 256; a resolution that does not fit the device's memory is recorded as skipped).  Per resolution,
device events, warm, median and min of ROUNDS >= 7, the variants alternated inside one process:
  simplify_ms      one ``ops.mesh_simplify`` at a cell of 2 voxels (the three host reads of its sizes included)
  count_ms         one ``ops.mesh_simplify_count`` at the same cell: what a probe of the search costs
  search_ms        the whole ``export.simplify_mesh(target_faces=50000)``: the probes of the bisection and the final simplification
  copy_ms / search_copy_ms   a device copy of as many bytes as the call reads (rows, faces) and writes (rows', faces'): the floor of a
                   pass that touched every byte once
Export (``--resolution 128``, ``--px-per-uv-triangle 4``, textures rgb and seg_pred, host clock, each stage behind a device
synchronisation): ``export.export_textured_mesh`` without and with ``simplify_faces=50000``, total and per stage, and the file sizes.
Prints one JSON line and writes it to --out (default profiles/simplify/bench_simplify.json)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tools")]
import torch

from bench_texture import DEV, SIDE, device_ms, host_ms, stats

ROUNDS, TARGET = 7, 50000


def scene():
    import bench
    from umhsnerf.data.umhs_datamanager import ResidentSplit
    from umhsnerf.data.umhs_dataparser import Cameras

    pipe, c2w = bench.sampler_scene(bench.C2, DEV)
    n, f = c2w.shape[0], 30.0 * SIDE / 64.0
    cams = Cameras(c2w.clone(), torch.full((n,), f), torch.full((n,), f), torch.full((n,), SIDE / 2), torch.full((n,), SIDE / 2), SIDE, SIDE)
    pipe.datamanager.train_split = ResidentSplit(cams, torch.zeros(n, SIDE, SIDE, 3, dtype=torch.uint8), None, DEV)
    return pipe


def kernel_part(pipe, rounds, resolution):
    from umhsnerf import export, ops

    try:
        fused = export.fuse_tsdf_volume(pipe, resolution)
        rows, faces, C = export.extract_mesh(fused["volume"])
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"skipped": f"out of memory: {str(e)[:120]}"}
    vol = fused["volume"]
    lo, h, dims = vol["lo"], vol["h"], vol["dims"]
    del fused
    e2 = export.simplify_edge(h, 2.0)
    g2 = export.simplify_origin(lo, e2)
    one = ops.mesh_simplify(rows, faces, C, g2, e2)
    found, info = export.simplify_mesh(rows, faces, C, lo, h, dims, target_faces=TARGET)
    moved = lambda m: rows.numel() + faces.numel() * 4 + (0 if m is None else m["rows"].numel() + m["faces"].numel() * 4)
    bufs = {k: (torch.empty(moved(m), dtype=torch.uint8, device=DEV), torch.empty(moved(m), dtype=torch.uint8, device=DEV))
            for k, m in (("copy_ms", one), ("search_copy_ms", found))}
    variants = {"simplify_ms": lambda: ops.mesh_simplify(rows, faces, C, g2, e2),
                "count_ms": lambda: ops.mesh_simplify_count(rows, faces, C, g2, e2),
                "search_ms": lambda: export.simplify_mesh(rows, faces, C, lo, h, dims, target_faces=TARGET),
                "copy_ms": lambda: bufs["copy_ms"][1].copy_(bufs["copy_ms"][0]),
                "search_copy_ms": lambda: bufs["search_copy_ms"][1].copy_(bufs["search_copy_ms"][0])}
    for fn in variants.values():  # warm (the allocator as well)
        for _ in range(2):
            fn()
    t_ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t_ms[k].append(device_ms(fn))
    res = {k: stats(v) for k, v in t_ms.items()}
    res.update(resolution=resolution, vertices=int(rows.shape[0]), faces=int(faces.shape[0]), classes=C, row_bytes=int(rows.shape[1]),
               simplify_2_voxels={"vertices": int(one["rows"].shape[0]), "faces": int(one["faces"].shape[0]), "bytes_moved": moved(one)},
               search={**info, "vertices": 0 if found is None else int(found["rows"].shape[0]),
                       "faces": int(faces.shape[0]) if found is None else int(found["faces"].shape[0]), "bytes_moved": moved(found)})
    res["simplify_over_copy"] = res["simplify_ms"]["median"] / res["copy_ms"]["median"]
    res["search_over_copy"] = res["search_ms"]["median"] / res["search_copy_ms"]["median"]
    del bufs
    torch.cuda.empty_cache()
    return res


def export_part(pipe, rounds, resolution):
    from umhsnerf import export

    names = ("rgb", "seg_pred")
    keys = ("total", "mesh", "rays", "render", "compose", "write")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        runs = {"plain": lambda **kw: export.export_textured_mesh(pipe, os.path.join(tmp, "plain"), resolution=resolution, px_per_uv_triangle=4,
                                                                  texture_output_names=names, **kw),
                "simplified": lambda **kw: export.export_textured_mesh(pipe, os.path.join(tmp, "simplified"), resolution=resolution,
                                                                       px_per_uv_triangle=4, texture_output_names=names, simplify_faces=TARGET, **kw)}
        for run in runs.values():
            run()  # warm up
        parts = {name: {k: [] for k in keys} for name in runs}
        infos = {}
        for _ in range(rounds):
            for name, run in runs.items():
                timings = {}
                ms, infos[name] = host_ms(lambda: run(timings=timings))
                parts[name]["total"].append(ms)
                for k, val in timings.items():
                    parts[name][k].append(val * 1e3)
        for name, info in infos.items():
            res[name] = {"export_ms": {k: stats(v) for k, v in parts[name].items()},
                         "export": {k: info.get(k) for k in ("vertices", "faces", "atlas_side", "ray_length", "simplified_from", "cell_voxels", "probes")},
                         "file_bytes": {os.path.basename(q): os.path.getsize(q) for q in (info["file"], *info["textures"].values())}}
    res["total_simplified_over_plain"] = res["simplified"]["export_ms"]["total"]["median"] / res["plain"]["export_ms"]["total"]["median"]
    res["resolution"], res["target_faces"] = resolution, TARGET
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify", "bench_simplify.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--resolution", type=int, default=128, help="of the whole export")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 7)
    pipe = scene()
    res = {"bench": "simplify", "device": torch.cuda.get_device_name(0), "rounds": rounds,
           "kernel": {f"res{r}": kernel_part(pipe, rounds, r) for r in args.resolutions}}
    if not args.kernel_only:
        res["export"] = export_part(pipe, rounds, args.resolution)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
