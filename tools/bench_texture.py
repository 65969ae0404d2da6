"""Textured mesh export: the texel-ray kernel against a copy of the bytes it writes, and the whole export stage by stage (not
bench.py: that measures the training step).  GPU box.  Records, not gates.

Kernel (device events, warm, median and min of ROUNDS >= 7, the variants alternated inside one process).  The mesh is a height field
over a G x G grid of vertices, two faces per cell in row order, cut to F = 10^5 and 10^6 faces: consecutive faces share vertices as
the faces of an extracted mesh do.  Per (F, p), p = 4 and 8, over the whole atlas:
  rays_ms          ``ops.texture_rays`` without the barycentric weights: 36 B written per texel (origins 12, directions 12, nears 4,
                   fars 4, texel_face 4), at most 48 B gathered per face
  rays_bary_ms     the same with the weights (48 B per texel)
  copy_ms          a device copy of as many bytes as rays_ms writes: the floor of a kernel that only writes
  uv_ms            ``ops.texture_uv`` (24 B per face)
  rays_over_copy   rays_ms / copy_ms;  rays_gbps: written bytes over time
Export (bench.py's ``sampler_scene`` at C2 after 300 steps, its six cameras at 512 x 512 as tools/bench_mesh.py), ``--resolution 128``,
``--px-per-uv-triangle 4``, textures rgb and seg_pred, host clock, each stage behind a device synchronisation:
  export_ms        total and mesh (depth renders, fusion, extraction) / rays / render / compose / write
Prints one JSON line and writes it to --out (default profiles/texture/bench_texture.json)."""
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

DEV = torch.device("cuda", 0)
ROUNDS, SIDE = 7, 512


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


def height_field(n_faces: int):
    """(positions [G*G, 3], faces [n_faces, 3] int32) on the device: z = a gentle wave over the unit square."""
    G = 2
    while 2 * (G - 1) * (G - 1) < n_faces:
        G += 1
    ax = torch.linspace(-1.0, 1.0, G, device=DEV)
    y, x = torch.meshgrid(ax, ax, indexing="ij")
    pos = torch.stack([x, y, 0.2 * torch.sin(3.0 * x) * torch.cos(2.0 * y)], -1).reshape(-1, 3).contiguous()
    cy, cx = torch.meshgrid(torch.arange(G - 1, device=DEV), torch.arange(G - 1, device=DEV), indexing="ij")
    v00 = (cy * G + cx).reshape(-1)
    lower = torch.stack([v00, v00 + 1, v00 + G], 1)
    upper = torch.stack([v00 + 1, v00 + G + 1, v00 + G], 1)
    faces = torch.stack([lower, upper], 1).reshape(-1, 3)[:n_faces].to(torch.int32).contiguous()
    return pos, faces


def kernel_part(rounds, face_counts, pxs):
    from umhsnerf import ops

    res = {}
    for F in face_counts:
        pos, faces = height_field(F)
        for p in pxs:
            _, T = ops.texture_atlas(F, p)
            n = T * T
            src, dst = torch.empty(n * 9, device=DEV), torch.empty(n * 9, device=DEV)
            L = 0.01
            variants = {"rays_ms": lambda: ops.texture_rays(pos, faces, p, L), "rays_bary_ms": lambda: ops.texture_rays(pos, faces, p, L, want_bary=True),
                        "copy_ms": lambda: dst.copy_(src), "uv_ms": lambda: ops.texture_uv(F, p, DEV)}
            for fn in variants.values():  # warm (the allocator as well: every variant allocates its outputs)
                for _ in range(3):
                    fn()
            t_ms = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    t_ms[k].append(device_ms(fn, reps=3))
            rr = {k: stats(v) for k, v in t_ms.items()}
            live = int((ops.texture_rays(pos, faces, p, L)["texel_face"] >= 0).sum())
            rr.update(faces=F, vertices=int(pos.shape[0]), px=p, atlas_side=T, texels=n, live_texels=live, bytes_written=36 * n,
                      bytes_gathered_at_most=48 * F)
            rr["rays_over_copy"] = rr["rays_ms"]["median"] / rr["copy_ms"]["median"]
            rr["rays_bary_over_rays"] = rr["rays_bary_ms"]["median"] / rr["rays_ms"]["median"]
            rr["rays_gbps"] = 36 * n / rr["rays_ms"]["median"] / 1e6
            rr["copy_gbps_read_plus_written"] = 2 * 36 * n / rr["copy_ms"]["median"] / 1e6
            res[f"F{F}_p{p}"] = rr
            del src, dst
            torch.cuda.empty_cache()
    return res


def export_part(rounds, resolution, px):
    import bench
    from umhsnerf import export
    from umhsnerf.data.umhs_datamanager import ResidentSplit
    from umhsnerf.data.umhs_dataparser import Cameras

    pipe, c2w = bench.sampler_scene(bench.C2, DEV)
    n, f = c2w.shape[0], 30.0 * SIDE / 64.0
    cams = Cameras(c2w.clone(), torch.full((n,), f), torch.full((n,), f), torch.full((n,), SIDE / 2), torch.full((n,), SIDE / 2), SIDE, SIDE)
    pipe.datamanager.train_split = ResidentSplit(cams, torch.zeros(n, SIDE, SIDE, 3, dtype=torch.uint8), None, DEV)
    names = ("rgb", "seg_pred")
    keys = ("total", "mesh", "rays", "render", "compose", "write")
    with tempfile.TemporaryDirectory() as tmp:
        run = lambda **kw: export.export_textured_mesh(pipe, tmp, resolution=resolution, px_per_uv_triangle=px, texture_output_names=names, **kw)
        run()  # warm up
        parts = {k: [] for k in keys}
        for _ in range(rounds):
            timings = {}
            ms, info = host_ms(lambda: run(timings=timings))
            parts["total"].append(ms)
            for k, val in timings.items():
                parts[k].append(val * 1e3)
        res = {"export_ms": {k: stats(v) for k, v in parts.items()},
               "export": {k: info[k] for k in ("vertices", "faces", "atlas_side", "px_per_uv_triangle", "ray_length")},
               "file_bytes": {os.path.basename(q): os.path.getsize(q) for q in (info["file"], *info["textures"].values())}}
    res["model"] = {"bands": bench.C2["B"], "classes": bench.C2["C"], "pred_specular": True}
    res["resolution"], res["texture_output_names"] = resolution, list(names)
    med = res["export_ms"]
    res["render_share_of_texturing"] = med["render"]["median"] / max(sum(med[k]["median"] for k in ("rays", "render", "compose", "write")), 1e-9)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture", "bench_texture.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--px", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 7)
    res = {"bench": "texture", "device": torch.cuda.get_device_name(0), "rounds": rounds, "kernel": kernel_part(rounds, args.faces, args.px)}
    if not args.kernel_only:
        res["export"] = export_part(rounds, args.resolution, 4)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
