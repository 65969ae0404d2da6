"""Mesh components: labelling, statistics and emit against a copy of the bytes they read and write, and the whole textured export with
and without the cleaning stage (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Mesh: tools/bench_simplify.py's scene (bench.py's ``sampler_scene`` at C2 after 300 steps, six cameras at 512 x 512), fused and
extracted at ``--resolutions`` (default 128 and 256; a resolution that does not fit the device's memory is recorded as skipped).  Per
resolution, device events, warm, median and min of ROUNDS >= 7, the variants alternated inside one process:
  label_ms         the labelling rounds alone (their reads of the changed word included), and the rounds they took
  statistics_ms    dense ids, counts and areas from the labels (two sorts, the read of the component count)
  components_ms    one ``ops.mesh_components``: the two together
  emit_ms          one ``ops.mesh_keep_components`` with the keep mask of ``--min-component-fraction 0.02`` (the read of its two sizes)
  clean_ms         the whole ``export.clean_mesh(min_component_fraction=0.02)``: the above, the mask and the table
  copy_ms / emit_copy_ms   a device copy of as many bytes as the labelling and statistics read (rows, faces) and write (the two id
                   arrays, the three tables) / as the emit reads and writes: the floor of a pass that touched every byte once
Export (``--resolution 128``, ``--px-per-uv-triangle 4``, textures rgb and seg_pred, ``material`` the label with the most faces, host
clock, each stage behind a device synchronisation): ``export.export_textured_mesh(material=K, simplify_faces=50000)`` without and with
``min_component_fraction=0.02``, total and per stage, and the file sizes.
Prints one JSON line and writes it to --out (default profiles/components/bench_components.json)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tools")]
import torch

from bench_simplify import scene
from bench_texture import DEV, device_ms, host_ms, stats

ROUNDS, TARGET, FRACTION = 7, 50000, 0.02


def kernel_part(pipe, rounds, resolution):
    from umhsnerf import export, ops
    from umhsnerf.ops import export as ox

    try:
        fused = export.fuse_tsdf_volume(pipe, resolution)
        rows, faces, C = export.extract_mesh(fused["volume"])
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"skipped": f"out of memory: {str(e)[:120]}"}
    del fused
    rows, faces = rows.contiguous(), faces.contiguous()
    V, F, rb = rows.shape[0], faces.shape[0], rows.shape[1]
    comps = ops.mesh_components(rows, faces, C)
    K = comps["n_components"]
    keep = export.component_keep_mask(comps["faces"], min_component_fraction=FRACTION)
    kept = ops.mesh_keep_components(rows, faces, C, comps, keep)
    parent, _ = ox._components_label(faces, V, ox.COMPONENTS_ROUNDS_PER_READ)
    nbytes = {"copy_ms": rows.numel() + faces.numel() * 4 + 4 * (V + F) + 24 * K,
              "emit_copy_ms": rows.numel() + faces.numel() * 4 + 4 * F + K + kept["rows"].numel() + kept["faces"].numel() * 4
              + kept["positions"].numel() * 4 + 4 * V}
    bufs = {k: (torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)) for k, n in nbytes.items()}
    taken = []

    def label():
        taken.append(ox._components_label(faces, V, ox.COMPONENTS_ROUNDS_PER_READ)[1])

    variants = {"label_ms": label,
                "statistics_ms": lambda: ox._components_statistics(rows, faces, rb, parent),
                "components_ms": lambda: ops.mesh_components(rows, faces, C),
                "emit_ms": lambda: ops.mesh_keep_components(rows, faces, C, comps, keep),
                "clean_ms": lambda: export.clean_mesh(rows, faces, C, min_component_fraction=FRACTION),
                "copy_ms": lambda: bufs["copy_ms"][1].copy_(bufs["copy_ms"][0]),
                "emit_copy_ms": lambda: bufs["emit_copy_ms"][1].copy_(bufs["emit_copy_ms"][0])}
    for fn in variants.values():  # warm (the allocator as well)
        for _ in range(2):
            fn()
    del taken[:]
    t_ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t_ms[k].append(device_ms(fn))
    res = {k: stats(v) for k, v in t_ms.items()}
    nf = comps["faces"]
    res.update(resolution=resolution, vertices=V, faces=F, classes=C, row_bytes=rb, rounds_taken=sorted(set(taken)),
               rounds_per_read=ox.COMPONENTS_ROUNDS_PER_READ, components=K, components_with_faces=int((nf > 0).sum()),
               largest_faces=torch.sort(nf, descending=True).values[:5].tolist(), bytes_moved=nbytes,
               kept={"components": int(keep.sum()), "vertices": int(kept["rows"].shape[0]), "faces": int(kept["faces"].shape[0])})
    res["components_over_copy"] = res["components_ms"]["median"] / res["copy_ms"]["median"]
    res["emit_over_copy"] = res["emit_ms"]["median"] / res["emit_copy_ms"]["median"]
    del bufs
    torch.cuda.empty_cache()
    return res


def export_part(pipe, rounds, resolution):
    from umhsnerf import export

    fused = export.fuse_tsdf_volume(pipe, resolution)
    rows, faces, C = export.extract_mesh(fused["volume"])
    del fused
    label = rows[:, 15:19].contiguous().view(torch.int32).view(-1)
    per_label = [int((label[faces.long()] == k).all(dim=1).sum()) for k in range(C)]
    K = max(range(C), key=lambda k: per_label[k])
    names = ("rgb", "seg_pred")
    keys = ("total", "mesh", "rays", "render", "compose", "write")
    res = {"material": K, "faces_per_material": per_label}
    with tempfile.TemporaryDirectory() as tmp:
        base = dict(resolution=resolution, px_per_uv_triangle=4, texture_output_names=names, material=K, simplify_faces=TARGET)
        runs = {"simplified": lambda **kw: export.export_textured_mesh(pipe, os.path.join(tmp, "simplified"), **base, **kw),
                "cleaned": lambda **kw: export.export_textured_mesh(pipe, os.path.join(tmp, "cleaned"), min_component_fraction=FRACTION, **base, **kw)}
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
                         "export": {k: info.get(k) for k in ("vertices", "faces", "atlas_side", "ray_length", "simplified_from", "cell_voxels", "probes",
                                                             "components", "components_kept", "cleaned_from")},
                         "component_table": (info.get("component_table") or [])[:5],
                         "file_bytes": {os.path.basename(q): os.path.getsize(q) for q in (info["file"], *info["textures"].values())}}
    res["total_cleaned_over_simplified"] = res["cleaned"]["export_ms"]["total"]["median"] / res["simplified"]["export_ms"]["total"]["median"]
    res["resolution"], res["target_faces"], res["min_component_fraction"] = resolution, TARGET, FRACTION
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components", "bench_components.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--resolution", type=int, default=128, help="of the whole export")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 7)
    pipe = scene()
    res = {"bench": "components", "device": torch.cuda.get_device_name(0), "rounds": rounds,
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
