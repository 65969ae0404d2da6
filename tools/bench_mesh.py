"""Mesh export, stage by stage (not bench.py: that measures the training step).  GPU box.  Records, not gates.

Model: bench.py's ``sampler_scene`` at C2 (31 bands, 6 classes, pred_specular) after 300 training steps, as tools/bench_render.py.
Its six training cameras are used at 512 x 512 and rendered at the export's default ``--downscale-factor 2``, i.e. 6 x 256 x 256 depth
maps; the box is the scene box [-1, 1]^3 at ``--resolution`` 128 and 256.

Measured per resolution, warm, median (and min) of ROUNDS >= 5, the variants alternated inside one process, device events:
  fuse_ms         ops.tsdf_integrate of the six cameras (one launch) into a zeroed volume
  torch_fuse_ms   the same fusion with torch ops (``torch_fuse`` below: one gather pass and a dozen volume-sized temporaries per
                  camera); torch_max_abs_diff_D / torch_counts_equal compare the two volumes
  fuse_bytes      what the launch must move: D, W and Wc read and written once (24 B per lattice point), the images once, and the
                  attribute planes where a sighting tints them (8 B per attribute and tinted sighting);  fuse_gbps = bytes / time
  copy_gbps       a plain device copy (``Tensor.copy_``) of 256 MiB, read plus written bytes over time: the yardstick of the machine
  fuse_over_copy  fuse_ms / (fuse_bytes / copy rate): 1.0 would be a fusion as fast as copying the bytes it must move
  extract_ms      ops.mesh_extract: mark, the scans, the 16-byte read of the totals, vertices, triangles (host clock around a
                  synchronise);  extract_kernels_ms: the three launches alone on pre-sized outputs (device events)
  volume_copy_ms  one plain device copy of the volume (D, W, Wc and the attribute planes)
  export_ms       the whole export_tsdf_mesh, split into render / fuse / extract / write (each behind a device synchronisation)
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
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
from umhsnerf import _hip, export, ops
from umhsnerf.data.umhs_datamanager import ResidentSplit
from umhsnerf.data.umhs_dataparser import Cameras

DEV = torch.device("cuda", 0)
ROUNDS, SIDE = 5, 512


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


def lattice(lo, h, dims):
    ax = [torch.arange(n, device=DEV, dtype=torch.float32) * h + l for n, l in zip(dims, lo)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)


def torch_fuse(vol, p, c2w, intr, depth, acc, rgb, abund, probs, thr, trunc):
    """umhs_tsdf_integrate's rules for undistorted cameras with torch ops, camera by camera."""
    D, W, Wc, A = vol["D"], vol["W"], vol["Wc"], vol["A"]
    n, hgt, wid = depth.shape[:3]
    for c in range(n):
        e = p - c2w[c, :, 3]
        pc = e @ c2w[c, :, :3]
        zc = -pc[:, 2]
        u, v = intr[c, 0] * (pc[:, 0] / zc) + intr[c, 2], intr[c, 1] * (-pc[:, 1] / zc) + intr[c, 3]
        ok = (zc > 0) & (u >= 0) & (u < wid) & (v >= 0) & (v < hgt)
        flat = v.clamp(0, hgt - 1).long() * wid + u.clamp(0, wid - 1).long()
        flat = torch.where(ok, flat, torch.zeros_like(flat))
        d, a = depth[c].reshape(-1)[flat], acc[c].reshape(-1)[flat]
        ok &= torch.isfinite(d)
        hit = ~(a <= thr)
        sdf = d - e.norm(dim=1)
        ok &= ~(hit & (sdf < -trunc))
        obs = torch.where(hit, (sdf / trunc).clamp(max=1.0), torch.ones_like(sdf))
        tint = ok & hit & (sdf.abs() <= trunc)
        attr = torch.cat([rgb[c].reshape(-1, 3)[flat], abund[c].reshape(-1, abund.shape[-1])[flat],
                          probs[c].reshape(-1, probs.shape[-1])[flat]], 1).t()
        A.copy_(torch.where(tint, (A * Wc + attr) / (Wc + 1), A))
        D.copy_(torch.where(ok, (D * W + obs) / (W + 1), D))
        W += ok
        Wc += tint


def zero(vol):
    for k in ("D", "W", "Wc", "A"):
        vol[k].zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    rounds = max(args.rounds, 5)
    pipe, c2w = bench.sampler_scene(bench.C2, DEV)
    n, f = c2w.shape[0], 30.0 * SIDE / 64.0
    cams = Cameras(c2w.clone(), torch.full((n,), f), torch.full((n,), f), torch.full((n,), SIDE / 2), torch.full((n,), SIDE / 2), SIDE, SIDE)
    pipe.datamanager.train_split = ResidentSplit(cams, torch.zeros(n, SIDE, SIDE, 3, dtype=torch.uint8), None, DEV)
    model, split = pipe.model, pipe.datamanager.train_split
    res = {"bench": "mesh", "model": {"bands": bench.C2["B"], "classes": bench.C2["C"], "pred_specular": True}, "cameras": n,
           "rendered": [SIDE // 2, SIDE // 2], "rounds": rounds, "device": torch.cuda.get_device_name(0)}

    # the yardstick: a plain device copy
    src = torch.empty(64 << 20, device=DEV)
    dst = torch.empty_like(src)
    dst.copy_(src)
    t = [device_ms(lambda: dst.copy_(src)) for _ in range(rounds)]
    copy_rate = 2 * src.numel() * 4 / (statistics.median(t) * 1e-3)
    res["copy_gbps"] = copy_rate / 1e9
    del src, dst

    tc = export.tsdf_cameras(split, 2)
    names = ["depth", "rgb", "accumulation", "abundances", "seg_probs"]
    model.eval()
    with torch.no_grad():
        out = export.render_cameras(model, tc, 0, n, names)
    model.train()
    C_ = out["abundances"].shape[-1]
    K = 3 + 2 * C_
    image_bytes = sum(out[k].numel() * 4 for k in names)
    c2w_d, intr_d = tc["c2w"], tc["intrinsics"]
    for r in args.resolutions:
        lo, h, dims = export.tsdf_lattice([-1, -1, -1], [1, 1, 1], r)
        trunc = float(np.float32(5.0 * h))
        N = dims[0] * dims[1] * dims[2]
        vol, tvol = ops.tsdf_volume(lo, h, dims, C_, DEV), ops.tsdf_volume(lo, h, dims, C_, DEV)
        p = lattice(lo, h, dims)
        hip = lambda: ops.tsdf_integrate(vol, tc["c2w_host"], tc["intrinsics_host"], None, out["depth"], out["accumulation"], out["rgb"],
                                         out["abundances"], out["seg_probs"], 0.5, trunc)
        tor = lambda: torch_fuse(tvol, p, c2w_d, intr_d, out["depth"], out["accumulation"], out["rgb"], out["abundances"],
                                 out["seg_probs"], 0.5, trunc)
        hip(), tor()  # warm up
        t = {"fuse_ms": [], "torch_fuse_ms": []}
        for _ in range(rounds):
            zero(vol), zero(tvol)
            t["fuse_ms"].append(device_ms(hip))
            t["torch_fuse_ms"].append(device_ms(tor))
        rr = {k: stats(v) for k, v in t.items()}
        seen = vol["W"] > 0
        rr["points"], rr["seen"], rr["tinted_sightings"] = N, int(seen.sum()), int(vol["Wc"].sum())
        rr["torch_counts_equal"] = bool(torch.equal(vol["W"], tvol["W"]) and torch.equal(vol["Wc"], tvol["Wc"]))
        rr["torch_count_mismatches"] = int((vol["W"] != tvol["W"]).sum() + (vol["Wc"] != tvol["Wc"]).sum())
        same = (vol["W"] == tvol["W"]) & (vol["Wc"] == tvol["Wc"])
        rr["torch_max_abs_diff_D"] = float((vol["D"] - tvol["D"])[same].abs().max())
        rr["fuse_bytes"] = 24 * N + image_bytes + 8 * K * rr["tinted_sightings"]
        rr["fuse_gbps"] = rr["fuse_bytes"] / (rr["fuse_ms"]["median"] * 1e-3) / 1e9
        rr["fuse_over_copy"] = rr["fuse_ms"]["median"] * 1e-3 / (rr["fuse_bytes"] / copy_rate)
        rr["torch_over_hip"] = rr["torch_fuse_ms"]["median"] / rr["fuse_ms"]["median"]
        del tvol, p

        # extraction: the whole op, the three launches alone, a copy of the volume
        mesh = ops.mesh_extract(vol)
        rr["vertices"], rr["faces"] = int(mesh["rows"].shape[0]), int(mesh["faces"].shape[0])
        lib, v = _hip.lib(), ops._tsdf_volume_c(vol)
        chunks = int(lib.umhs_mesh_chunks(N))
        mask = torch.empty(N, dtype=torch.uint8, device=DEV)
        counts = torch.empty(2, chunks, dtype=torch.int32, device=DEV)
        vbase = torch.empty(N, dtype=torch.int32, device=DEV)
        rows, faces = torch.empty_like(mesh["rows"]), torch.empty_like(mesh["faces"])
        lib.umhs_mesh_mark(C.byref(v), _hip.ptr(mask), C.c_void_p(counts[0].data_ptr()), C.c_void_p(counts[1].data_ptr()), _hip.stream())
        c64 = counts.to(torch.int64)
        off = (torch.cumsum(c64, 1) - c64).contiguous()

        def kernels():
            _hip.check(lib.umhs_mesh_mark(C.byref(v), _hip.ptr(mask), C.c_void_p(counts[0].data_ptr()), C.c_void_p(counts[1].data_ptr()),
                                          _hip.stream()), "mark")
            _hip.check(lib.umhs_mesh_vertices(C.byref(v), _hip.ptr(mask), C.c_void_p(off[0].data_ptr()), None, _hip.ptr(vbase),
                                              C.c_void_p(rows.data_ptr()), rows.shape[0], _hip.stream()), "vertices")
            _hip.check(lib.umhs_mesh_triangles(C.byref(v), _hip.ptr(mask), _hip.ptr(vbase), C.c_void_p(off[1].data_ptr()),
                                               C.c_void_p(faces.data_ptr()), faces.shape[0], _hip.stream()), "triangles")

        kernels()
        rr["kernels_equal_op"] = bool(torch.equal(rows, mesh["rows"]) and torch.equal(faces, mesh["faces"]))
        copies = {k: torch.empty_like(vol[k]) for k in ("D", "W", "Wc", "A")}

        def volume_copy():
            for k, dst_ in copies.items():
                dst_.copy_(vol[k])

        volume_copy()
        t = {"extract_ms": [], "extract_kernels_ms": [], "volume_copy_ms": []}
        for _ in range(rounds):
            t["extract_ms"].append(host_ms(lambda: ops.mesh_extract(vol))[0])
            t["extract_kernels_ms"].append(device_ms(kernels))
            t["volume_copy_ms"].append(device_ms(volume_copy))
        rr.update({k: stats(v) for k, v in t.items()})
        rr["extract_kernels_over_volume_copy"] = rr["extract_kernels_ms"]["median"] / rr["volume_copy_ms"]["median"]
        del copies, mask, counts, vbase, rows, faces, mesh, vol

        # the whole export
        with tempfile.TemporaryDirectory() as tmp:
            export.export_tsdf_mesh(pipe, tmp, resolution=r)  # warm up
            parts = {k: [] for k in ("total", "render", "fuse", "extract", "write", "unsplit_total")}
            for _ in range(rounds):
                timings = {}
                ms, info = host_ms(lambda: export.export_tsdf_mesh(pipe, tmp, resolution=r, timings=timings))
                parts["total"].append(ms)
                for k, val in timings.items():
                    parts[k].append(val * 1e3)
                parts["unsplit_total"].append(host_ms(lambda: export.export_tsdf_mesh(pipe, tmp, resolution=r))[0])
            rr["export_ms"] = {k: stats(val) for k, val in parts.items()}
            rr["export"] = {k: info[k] for k in ("vertices", "faces", "cameras", "resolution", "voxel_size", "truncation")}
            rr["file_bytes"] = os.path.getsize(info["file"])
        res[str(r)] = rr
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
