"""``python -m umhsnerf.export pointcloud --data DIR --checkpoint FILE --output-dir DIR``: what ``ns-export pointcloud`` does for a
trained model, without nerfstudio and without Open3D -- and with what sets this method apart: every point carries the model's material
label and its abundances, so the unsupervised 3-D material decomposition leaves a checkpoint as geometry.

The loop is nerfstudio's ``exporter_utils.generate_point_cloud``  [upstream-recalled]: draw a batch of training rays (``mask_path``
masks are respected: the draw goes through ``ResidentSplit.sample``), render without gradients, ``point = origin + direction * depth``,
keep the point if ``accumulation > opacity_threshold`` (strict), if it is finite and -- with a box -- strictly inside the box; repeat
until ``num_points`` are kept; then Open3D's ``remove_statistical_outlier(nb_neighbors, std_ratio)``  [upstream-recalled]: with m_i
the mean distance of point i to its ``nb_neighbors`` nearest points (itself included, as Open3D's ``SearchKNN`` returns the query
first), mu and sigma the mean and SAMPLE standard deviation of the m_i (float64), a point stays iff ``0 < m_i < mu + std_ratio * sigma``.

Everything between the draw and the file stays on the device: ``ops.pc_append`` turns a batch into packed rows (keep rule, ordered
compaction, row packing: two launches around a scan of a few hundred integers, no atomics), ``ops.knn_mean_dist`` is the exact
neighbour search.  The loop reads 8 bytes per batch (the running count).  Deliberate differences from nerfstudio:
the rays come from a generator of the export's own (``seed``) -- the datamanager's training stream, its eval cursor and the global
generators do not move; the model's train / eval mode is restored; exactly ``num_points`` points enter outlier removal (the surplus of
the last batch is cut in draw order); 64 consecutive batches that keep nothing raise instead of spinning; normals are written only
on request, ``--normal-method analytic``: the model's ``normals`` output, i.e. the analytic density gradient composited per ray
(``ops.density_normals``), not Open3D's PCA estimate (``open3d`` and ``model_output`` are refused), and they point out of the surface
by construction.  With ``--save-world-frame`` they are rotated by the linear part of the world affine and renormalised.

The file, ``point_cloud.ply``: binary little-endian PLY, ``float x y z`` (``float nx ny nz`` with normals), ``uchar red green blue
alpha`` and -- for ``spectral`` and ``rgb+spectral`` -- ``int material, float abundance_0 .. abundance_{C-1}``.  ``--spectra`` also writes ``point_cloud_spectral.npy``
(float32 [M, B], rows in file order); ``--material K`` keeps the points labelled K.

``python -m umhsnerf.export tsdf --data DIR --checkpoint FILE --output-dir DIR``: what ``ns-export tsdf`` does  [upstream-recalled] --
render depth from the training cameras (``--downscale-factor``), fuse the depth maps into a truncated signed distance volume over
``--bounding-box-min`` / ``--bounding-box-max`` (``ops.tsdf_integrate``), extract a triangle mesh (``ops.mesh_extract``: marching
tetrahedra, watertight where the level set is closed) -- with a colour, a material label and the abundances on every vertex.
``mesh.ply``: binary little-endian PLY, ``element vertex`` (``float x y z, uchar red green blue`` and, for the labelled methods, ``int
material, float abundance_0 ..``) and ``element face`` (``property list uchar int vertex_indices``).  ``--material K`` keeps the faces
whose three vertices are labelled K: a sub-mesh per material.  Deliberate differences from nerfstudio: the signed
distance is taken along the ray (depth here is the distance along a normalised ray) where nerfstudio compares against camera z;
colour is averaged only by the sightings inside the truncation band; marching tetrahedra instead of marching cubes; the mesh is
reduced by vertex clustering, not by edge collapse: ``--simplify-cell-voxels X`` merges the vertices of every cubic cell of X voxel
edges into the point that minimises the cell's plane quadric (``ops.mesh_simplify``; colour, label and abundances are the members'
mean, majority and mean), ``--simplify-faces N`` searches the ladder of cell edges ``h 2^(k/4)`` for the finest one that leaves at most
N faces (``ops.mesh_simplify_count`` per probe) -- it runs after ``--material``, so N holds for a sub-mesh too; floaters, interior
shells and the crumbs of a material sub-mesh are dropped by connected components instead of pymeshlab's filter: ``--min-component-faces
N``, ``--min-component-fraction R`` (of the largest component's faces) and ``--keep-largest-components K``, combined with AND, keep the
components that pass (``ops.mesh_components`` / ``ops.mesh_keep_components``), after ``--material`` and before the simplification, and
the summary lists the 16 largest kept components with their faces, vertices and model-frame area; ``--target-num-faces``
(pymeshlab's collapse to an exact count) stays refused; and the texture flags (``--texture-method`` / ``--unwrap-method``) are refused
in favour of

``python -m umhsnerf.export textured-mesh --data DIR --checkpoint FILE --output-dir DIR``: what ``ns-export tsdf --texture-method
nerf`` does  [upstream-recalled] -- the same mesh (``tsdf``'s flags, ``fuse_tsdf_volume`` and ``extract_mesh`` serve both) written as
``mesh.obj`` + ``material_0.mtl`` with a texture atlas: every face owns a triangle of the atlas (``ops.texture_atlas`` /
``ops.texture_uv``: two faces per square of ``--px-per-uv-triangle`` texels, corners at texel centres inset by 3 texels, so bilinear
filtering never mixes two faces), and every texel holds what the model renders along a ray of ``--ray-length`` that starts half its
length outside the surface and runs through it (``ops.texture_rays``; the atlas is walked in bands of rows).  ``material_0.png`` is
the first of ``--texture-output-names``, ``texture_<name>.png`` the others -- ``seg_pred``, ``abundances_k`` or ``wv_k`` give a
per-texel material map --, ``--cube-output-names`` writes whole outputs as ``texture_<name>.npy`` [T, T, channels].  Texels nobody owns
are 0.  The layout is this project's own (no unwrapping library), fixed to the bit in include/umhs_hip.h."""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

MAX_EMPTY_BATCHES = 64
PLY_NAME, SPECTRA_NAME = "point_cloud.ply", "point_cloud_spectral.npy"
MESH_NAME = "mesh.ply"


# ---- boxes and frames --------------------------------------------------------------------------------------------------------------
def obb_from_params(center: Sequence[float], rotation: Sequence[float], scale: Sequence[float]):
    """nerfstudio ``OrientedBox.from_params(pos, rpy, scale)``  [upstream-recalled]: Euler angles in radians, roll about x, pitch
    about y, yaw about z, ``R = Rz(yaw) Ry(pitch) Rx(roll)`` (viser's ``SO3.from_rpy_radians``); a point p is inside iff
    ``|(R^T (p - T))_k| < S_k / 2`` on every axis.  -> (T [3], R [3,3], S [3]) float32, composed in float64."""
    rx, ry, rz = (float(v) for v in rotation)
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
    return (np.asarray(center, dtype=np.float32).reshape(3), (Rz @ Ry @ Rx).astype(np.float32),
            np.asarray(scale, dtype=np.float32).reshape(3))


def world_frame_affine(transform, scale: float) -> np.ndarray:
    """[3,4] float32 affine that takes a model-frame point back to the scene's original frame: nerfstudio's
    ``transform_poses_to_original_space`` applied to a point  [upstream-recalled] -- ``p / dataparser_scale``, then the inverse of the
    [3,4] ``dataparser_transform``.  Composed in float64."""
    H = np.eye(4, dtype=np.float64)
    H[:3] = np.asarray(transform, dtype=np.float64).reshape(3, 4)
    inv = np.linalg.inv(H)
    A = np.concatenate([inv[:3, :3] / float(scale), inv[:3, 3:4]], axis=1)
    return A.astype(np.float32)


# ---- the file ----------------------------------------------------------------------------------------------------------------------
NORMAL_METHODS = ("none", "analytic")


def ply_header(n_points: int, n_classes: int, normals: bool = False) -> bytes:
    props = ["float x", "float y", "float z"] + (["float nx", "float ny", "float nz"] if normals else [])
    props += ["uchar red", "uchar green", "uchar blue", "uchar alpha"]
    if n_classes:
        props += ["int material"] + [f"float abundance_{i}" for i in range(n_classes)]
    lines = ["ply", "format binary_little_endian 1.0", "comment umhsnerf.export pointcloud", f"element vertex {int(n_points)}"]
    return ("\n".join(lines + ["property " + p for p in props] + ["end_header"]) + "\n").encode("ascii")


def write_ply(path, rows: torch.Tensor, n_classes: int, normals: bool = False) -> None:
    """``rows`` uint8 [M, row_bytes] (device or host) -> a binary little-endian PLY: the header and the rows, one ``write`` each, the
    rows from a pinned buffer."""
    m = rows.shape[0]
    host = rows
    if rows.is_cuda:
        host = torch.empty(rows.shape, dtype=torch.uint8).pin_memory()
        host.copy_(rows)
        torch.cuda.current_stream(rows.device).synchronize()
    with open(path, "wb") as f:
        f.write(ply_header(m, n_classes, normals))
        f.write(host.contiguous().numpy().data)


def rows_with_normals(table: torch.Tensor, normals: torch.Tensor) -> torch.Tensor:
    """The packed rows [M, row_bytes] of ``ops.pc_append`` with ``float nx ny nz`` put behind ``x y z`` (on the rows' device)."""
    n8 = normals.float().contiguous().view(torch.uint8).view(-1, 12)
    return torch.cat([table[:, :12], n8, table[:, 12:]], dim=1).contiguous()


def world_frame_normals(normals: torch.Tensor, world) -> torch.Tensor:
    """Unit normals [M,3] taken to the scene's original frame: the linear part of ``world_frame_affine`` and a renormalisation (its
    uniform scale drops out; no translation)."""
    A = torch.as_tensor(np.asarray(world, dtype=np.float32)[:, :3], device=normals.device)
    n = normals @ A.T
    return n / torch.linalg.vector_norm(n, dim=-1, keepdim=True).clamp_min(1e-20)


def mesh_ply_header(n_vertices: int, n_faces: int, n_classes: int) -> bytes:
    props = ["float x", "float y", "float z", "uchar red", "uchar green", "uchar blue"]
    if n_classes:
        props += ["int material"] + [f"float abundance_{i}" for i in range(n_classes)]
    lines = ["ply", "format binary_little_endian 1.0", "comment umhsnerf.export tsdf", f"element vertex {int(n_vertices)}"]
    lines += ["property " + p for p in props] + [f"element face {int(n_faces)}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def write_mesh_ply(path, rows: torch.Tensor, faces: torch.Tensor, n_classes: int) -> None:
    """``rows`` uint8 [V, row_bytes], ``faces`` int32 [F, 3] (device or host) -> a binary little-endian PLY: the header, the vertex
    rows, the face rows (a count byte 3 and three int32 each)."""
    frows = torch.empty(faces.shape[0], 13, dtype=torch.uint8, device=faces.device)
    frows[:, 0] = 3
    frows[:, 1:] = faces.contiguous().view(torch.uint8).view(faces.shape[0], 12)
    with open(path, "wb") as f:
        f.write(mesh_ply_header(rows.shape[0], faces.shape[0], n_classes))
        f.write(rows.contiguous().cpu().numpy().data)
        f.write(frows.cpu().numpy().data)


# ---- the export --------------------------------------------------------------------------------------------------------------------
def remove_statistical_outliers(points: torch.Tensor, nb_neighbors: int = 20, std_ratio: float = 10.0):
    """Open3D's ``remove_statistical_outlier``  [upstream-recalled] on device points [M,3] -> (keep [M] bool, threshold, means [M])."""
    from . import ops

    means = ops.knn_mean_dist(points, int(nb_neighbors))
    m64 = means.double()
    mu = m64.mean()
    sigma = m64.std(unbiased=True) if means.numel() > 1 else torch.zeros((), dtype=torch.float64, device=means.device)
    threshold = mu + float(std_ratio) * sigma
    return (means > 0) & (m64 < threshold), threshold, means


def export_pointcloud(pipeline, output_dir, num_points: int = 1000000, remove_outliers: bool = True, std_ratio: float = 10.0,
                      nb_neighbors: int = 20, depth_output_name: str = "depth", rgb_output_name: str = "rgb",
                      num_rays_per_batch: int = 32768, obb_center=None, obb_rotation=None, obb_scale=None,
                      save_world_frame: bool = False, opacity_threshold: float = 0.5, seed: int = 0, spectra: bool = False,
                      material: Optional[int] = None, timings: Optional[Dict[str, float]] = None, normal_method: str = "none") -> Dict:
    """Write ``point_cloud.ply`` (and ``point_cloud_spectral.npy`` with ``spectra``) into ``output_dir`` -> {"points", "rays_drawn",
    "batches", "removed_outliers", "threshold", "file"}.  See the module text for the rules.  ``timings``: a dict that receives the
    seconds spent in render / emit / neighbour search / file write (each behind a device synchronisation: a measuring aid)."""
    from . import ops

    if normal_method not in NORMAL_METHODS:
        raise ValueError(f"normal_method {normal_method!r}: 'none' or 'analytic' (the model's own density-gradient normals; there is no "
                         "Open3D estimate here)")
    want_normals = normal_method == "analytic"
    given = [v is not None for v in (obb_center, obb_rotation, obb_scale)]
    if any(given) and not all(given):
        raise ValueError("obb_center, obb_rotation and obb_scale come together: all three or none")
    num_points, R = int(num_points), int(num_rays_per_batch)
    if num_points < 1 or R < 1:
        raise ValueError(f"num_points {num_points} and num_rays_per_batch {R} must be positive")
    box = obb_from_params(obb_center, obb_rotation, obb_scale) if all(given) else None
    dm, model = pipeline.datamanager, pipeline.model
    world = None
    if save_world_frame:
        out = dm.train_dataparser_outputs
        world = world_frame_affine(out.dataparser_transform, out.dataparser_scale)
    split = dm.train_split
    dev = split.device
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    generator = torch.Generator(device=dev)
    generator.manual_seed(int(seed))
    ignore_mask = bool(getattr(dm.config, "ignore_mask", False))

    clock = None
    if timings is not None:
        timings.update({k: 0.0 for k in ("render", "emit", "neighbours", "write")})

        def clock(key, t0):
            torch.cuda.synchronize(dev)
            timings[key] += time.perf_counter() - t0
            return time.perf_counter()

    was_training, was_requested = model.training, getattr(model, "_normals_requested", False)
    model.eval()
    if want_normals:
        model._normals_requested = True
    rows = points = kept = spec_rows = normal_rows = None
    base = torch.zeros(1, dtype=torch.int64, device=dev)
    count = batches = empty = n_classes = 0
    try:
        with torch.no_grad():
            while count < num_points:
                t0 = time.perf_counter() if clock else 0.0
                rays, _ = split.sample(R, generator, ignore_mask=ignore_mask, want_batch=False)
                outputs = model(rays)
                for name in (depth_output_name, rgb_output_name, "accumulation"):
                    if name not in outputs:
                        raise ValueError(f"the model returned no {name!r} output; it returns: {', '.join(outputs)}")
                if clock:
                    t0 = clock("render", t0)
                labelled = "abundances" in outputs and "seg_probs" in outputs
                args = ops.pc_args(rays.origins, rays.directions, outputs[depth_output_name], outputs["accumulation"],
                                   outputs[rgb_output_name], outputs["abundances"] if labelled else None,
                                   outputs["seg_probs"] if labelled else None, opacity_threshold, box, world)
                if rows is None:
                    n_classes = args[2]
                    rows = torch.empty(num_points * ops.pc_row_bytes(n_classes), dtype=torch.uint8, device=dev)
                    points = torch.empty(num_points, 3, device=dev)
                    kept = torch.empty(num_points, dtype=torch.int64, device=dev)
                    if spectra:
                        if "spectral" not in outputs:
                            raise ValueError("--spectra needs a model with a `spectral` output (method spectral or rgb+spectral)")
                        spec_rows = torch.empty(num_points, outputs["spectral"].shape[-1], device=dev)
                    if want_normals:
                        if "normals" not in outputs:
                            raise ValueError(f"the model returned no 'normals' output; it returns: {', '.join(outputs)}")
                        normal_rows = torch.empty(num_points, 3, device=dev)
                base += ops.pc_append(args, rows, points, kept, base, batches * R, num_points)
                new_count = min(int(base), num_points)  # the one device read of a batch: 8 bytes
                if spec_rows is not None and new_count > count:
                    spec_rows[count:new_count] = outputs["spectral"][kept[count:new_count] - batches * R]
                if normal_rows is not None and new_count > count:  # the model's [0, 1] encoding back to a direction
                    normal_rows[count:new_count] = outputs["normals"][kept[count:new_count] - batches * R] * 2.0 - 1.0
                if clock:
                    clock("emit", t0)
                empty = empty + 1 if new_count == count else 0
                count, batches = new_count, batches + 1
                if empty >= MAX_EMPTY_BATCHES:
                    raise RuntimeError(f"nothing kept in {MAX_EMPTY_BATCHES} consecutive batches of {R} rays ({count} of {num_points} "
                                       "points so far): an empty crop box, an opacity threshold nothing reaches, or an untrained model")
    finally:
        model.train(was_training)
        if want_normals:
            model._normals_requested = was_requested

    row_bytes = ops.pc_row_bytes(n_classes)
    table = rows.view(num_points, row_bytes)
    removed, threshold = 0, None
    keep = torch.ones(num_points, dtype=torch.bool, device=dev)
    if remove_outliers:
        t0 = time.perf_counter() if clock else 0.0
        keep, thr, _ = remove_statistical_outliers(points, nb_neighbors, std_ratio)
        removed, threshold = int(num_points - keep.sum()), float(thr)
        if clock:
            clock("neighbours", t0)
    if material is not None:
        if not n_classes:
            raise ValueError("--material needs a model that labels its points (method spectral or rgb+spectral)")
        keep = keep & (table[:, 16:20].contiguous().view(torch.int32).view(-1) == int(material))
    t0 = time.perf_counter() if clock else 0.0
    table = table[keep]
    if normal_rows is not None:
        normals = normal_rows[keep]
        table = rows_with_normals(table, normals if world is None else world_frame_normals(normals, world))
    path = output_dir / PLY_NAME
    write_ply(path, table, n_classes, normal_rows is not None)
    if spec_rows is not None:
        np.save(output_dir / SPECTRA_NAME, spec_rows[keep].cpu().numpy())
    if clock:
        clock("write", t0)
    return {"points": int(table.shape[0]), "rays_drawn": batches * R, "batches": batches, "removed_outliers": removed,
            "threshold": threshold, "file": str(path)}


# ---- the mesh ----------------------------------------------------------------------------------------------------------------------
def tsdf_lattice(bounding_box_min, bounding_box_max, resolution):
    """-> (lo (3 floats), h, dims): ``resolution`` an integer N -- the longest side of the box gets N lattice points, the others as
    many as fit at the same voxel edge (voxels stay cubic) -- or three integers (nx, ny, nz): the edge is the largest of the three
    side / (n - 1), so the lattice covers the box."""
    lo, hi = np.asarray(bounding_box_min, dtype=np.float64).reshape(3), np.asarray(bounding_box_max, dtype=np.float64).reshape(3)
    ext = hi - lo
    if not (np.isfinite(ext).all() and (ext > 0).all()):
        raise ValueError(f"the bounding box {lo.tolist()} .. {hi.tolist()} is empty")
    res = [int(r) for r in (resolution if isinstance(resolution, (list, tuple)) else [resolution])]
    if len(res) == 1:
        if res[0] < 2:
            raise ValueError(f"resolution {res[0]}: at least 2")
        h = float(np.float32(ext.max() / (res[0] - 1)))
        dims = tuple(max(2, int(math.floor(e / h + 1e-6)) + 1) for e in ext)
    elif len(res) == 3 and min(res) >= 2:
        h = float(np.float32(max(e / (n - 1) for e, n in zip(ext, res))))
        dims = tuple(res)
    else:
        raise ValueError(f"resolution {resolution}: one integer or three, each at least 2")
    return tuple(float(np.float32(v)) for v in lo), h, dims


def tsdf_cameras(split, downscale_factor: float = 1.0) -> Dict:
    """The cameras of a split at ``1 / downscale_factor`` of their resolution, as nerfstudio's ``rescale_output_resolution`` scales them
    [upstream-recalled]: fx, fy, cx, cy times the factor, height and width floored.  -> device tensors for the ray generator and the
    same float32 values on the host for the fusion."""
    s = 1.0 / float(downscale_factor)
    if not s > 0:
        raise ValueError(f"downscale_factor {downscale_factor} must be positive")
    n, hgt, wid = split.image.shape[:3]
    hgt, wid = int(math.floor(hgt * s)), int(math.floor(wid * s))
    if hgt < 1 or wid < 1:
        raise ValueError(f"downscale_factor {downscale_factor} leaves no pixel")
    intr = (split.intrinsics.float() * s).contiguous()
    dist = split.distortion
    return {"n": int(n), "height": hgt, "width": wid, "c2w": split.c2w, "intrinsics": intr, "distortion": dist,
            "c2w_host": split.c2w.cpu().numpy(), "intrinsics_host": intr.cpu().numpy(),
            "distortion_host": None if dist is None else dist.cpu().numpy()}


def render_cameras(model, cams: Dict, begin: int, end: int, output_names) -> Dict[str, torch.Tensor]:
    """Cameras [begin, end) of ``tsdf_cameras`` rendered without gradients -> {name: [end - begin, H, W, k]} on the device."""
    from . import ops
    from ._ns_compat import RayBundle

    hgt, wid, dev = cams["height"], cams["width"], cams["c2w"].device
    cc, yy, xx = torch.meshgrid(torch.arange(begin, end, device=dev), torch.arange(hgt, device=dev), torch.arange(wid, device=dev),
                                indexing="ij")
    idx = torch.stack([cc, yy, xx], -1).reshape(-1, 3).contiguous()
    o, d, _, _ = ops.raygen(idx, cams["c2w"], cams["intrinsics"], want_area=False, distortion=cams["distortion"])
    shape = (end - begin, hgt, wid, 3)
    return model.get_outputs_for_camera_ray_bundle(RayBundle(origins=o.view(shape), directions=d.view(shape)), output_names=output_names)


def filter_mesh_material(rows: torch.Tensor, faces: torch.Tensor, material: int):
    """Keep the faces whose three vertices are all labelled ``material``; drop the vertices no face refers to and re-index."""
    label = rows[:, 15:19].contiguous().view(torch.int32).view(-1)
    f = faces.long()
    keep_f = (label[f] == int(material)).all(dim=1) if f.shape[0] else torch.zeros(0, dtype=torch.bool, device=faces.device)
    f = f[keep_f]
    used = torch.zeros(rows.shape[0], dtype=torch.bool, device=rows.device)
    used[f.reshape(-1)] = True
    new_id = torch.cumsum(used.to(torch.int64), 0) - 1
    return rows[used], new_id[f].to(torch.int32)


def _stage_clock(timings: Optional[Dict[str, float]], keys, dev):
    """``timings`` None: None.  Otherwise the keys are zeroed and ``clock(key, t0)`` adds the seconds since ``t0`` (behind a device
    synchronisation) to ``timings[key]`` and returns the new time."""
    if timings is None:
        return None
    timings.update({k: 0.0 for k in keys})

    def clock(key, t0):
        torch.cuda.synchronize(dev)
        timings[key] += time.perf_counter() - t0
        return time.perf_counter()

    return clock


def fuse_tsdf_volume(pipeline, resolution=128, bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
                     downscale_factor: float = 2, batch_size: int = 8, truncation_voxels: float = 5.0, opacity_threshold: float = 0.5,
                     depth_output_name: str = "depth", rgb_output_name: str = "rgb", clock=None) -> Dict:
    """The first half of the mesh exports: the training cameras rendered and fused -> {"volume" (``ops.tsdf_volume``), "cameras",
    "dims", "voxel_size", "truncation"}.  The model's train / eval mode is restored.  ``clock``: ``_stage_clock``'s, fed "render" and
    "fuse"."""
    from . import ops

    lo, h, dims = tsdf_lattice(bounding_box_min, bounding_box_max, resolution)
    batch_size = int(batch_size)
    if batch_size < 1 or not float(truncation_voxels) > 0:
        raise ValueError(f"batch_size {batch_size} and truncation_voxels {truncation_voxels} must be positive")
    trunc = float(np.float32(float(truncation_voxels) * h))
    model = pipeline.model
    split = pipeline.datamanager.train_split
    dev = split.device
    cams = tsdf_cameras(split, downscale_factor)
    was_training = model.training
    model.eval()
    vol = None
    try:
        with torch.no_grad():
            for b in range(0, cams["n"], batch_size):
                e = min(b + batch_size, cams["n"])
                t0 = time.perf_counter() if clock else 0.0
                names = [depth_output_name, rgb_output_name, "accumulation", "abundances", "seg_probs"]
                outputs = render_cameras(model, cams, b, e, names)
                for name in (depth_output_name, rgb_output_name, "accumulation"):
                    if name not in outputs:
                        raise ValueError(f"the model returned no {name!r} output; it returns: {', '.join(outputs)}")
                if clock:
                    t0 = clock("render", t0)
                labelled = "abundances" in outputs and "seg_probs" in outputs
                if vol is None:
                    vol = ops.tsdf_volume(lo, h, dims, outputs["abundances"].shape[-1] if labelled else 0, dev)
                pick = lambda a: None if a is None else a[b:e]
                ops.tsdf_integrate(vol, cams["c2w_host"][b:e], cams["intrinsics_host"][b:e], pick(cams["distortion_host"]),
                                   outputs[depth_output_name], outputs["accumulation"], outputs[rgb_output_name],
                                   outputs["abundances"] if labelled else None, outputs["seg_probs"] if labelled else None,
                                   opacity_threshold, trunc)
                if clock:
                    clock("fuse", t0)
    finally:
        model.train(was_training)
    if vol is None:
        raise ValueError("the training split has no camera to fuse")
    return {"volume": vol, "cameras": cams["n"], "dims": dims, "voxel_size": h, "truncation": trunc}


def extract_mesh(vol: Dict, world=None, material: Optional[int] = None):
    """The second half: ``ops.mesh_extract`` and the ``--material`` filter -> (rows uint8 [V, row_bytes], faces int32 [F, 3], n_classes).
    The filter reads the labels only, so with and without ``world`` it keeps the same faces in the same order."""
    from . import ops

    mesh = ops.mesh_extract(vol, world)
    rows, faces, n_classes = mesh["rows"], mesh["faces"], mesh["n_classes"]
    if material is not None:
        if not n_classes:
            raise ValueError("--material needs a model that labels its vertices (method spectral or rgb+spectral)")
        rows, faces = filter_mesh_material(rows, faces, material)
    return rows, faces, n_classes


# ---- simplification ----------------------------------------------------------------------------------------------------------------
def simplify_edge(h: float, cell_voxels: float) -> float:
    """``--simplify-cell-voxels X``: the cell edge ``X h`` as one float32 multiplication."""
    return float(np.float32(cell_voxels) * np.float32(h))


def simplify_origin(lo, edge: float):
    """The grid origin of a cell edge: the lattice's first point minus half a cell, per axis one float32 subtraction -- the extracted
    vertices lie on lattice edges, and the half-cell shift keeps them off the cell faces along two axes."""
    e = np.float32(edge)
    return tuple(float(np.float32(v) - e * np.float32(0.5)) for v in lo)


def simplify_ladder(lo, h: float, dims):
    """The cell edges ``--simplify-faces`` may choose: ``e_k = h 2^(k/4)``, each one float32 value formed on the host from the float64
    product, for k = 1, 2, ... up to the first whose grid (origin ``simplify_origin``) holds the whole lattice -- hence every vertex --
    in a single cell.  -> [e_1, ..., e_K] (floats)."""
    from .ops.export import simplify_grid_dims

    h32 = np.float32(h)
    far = [np.float32(v) + np.float32(d - 1) * h32 for v, d in zip(lo, dims)]
    rungs = []
    for k in range(1, 4096):
        e = float(np.float32(float(h32) * 2.0 ** (k / 4.0)))
        rungs.append(e)
        if simplify_grid_dims(far, simplify_origin(lo, e), e) == (1, 1, 1):
            return rungs
    raise ValueError(f"simplify_ladder: no single-cell rung above a voxel edge of {h}")


def simplify_search(count, n_rungs: int, target: int):
    """Bisect k in 1 .. n_rungs on ``count(k)`` (the faces left at rung k) -> (k, probes, {k: count}): the smallest probed k with
    ``count(k) <= target`` whose predecessor was probed with a larger count (rung 0, the unsimplified mesh, counts as probed and larger:
    the caller has checked).  A count that is not monotone in k still ends at such a pair.  The last rung must satisfy the target (a
    single cell leaves no face)."""
    seen = {}

    def probe(k):
        if k not in seen:
            seen[k] = int(count(k))
        return seen[k]

    below, above = 0, int(n_rungs)
    if above < 1 or probe(above) > target:
        raise RuntimeError(f"simplify_search: the coarsest rung {above} leaves more than {target} faces")
    while above - below > 1:
        mid = (below + above) // 2
        if probe(mid) <= target:
            above = mid
        else:
            below = mid
    k = min(j for j, c in seen.items() if c <= target and (j == 1 or (j - 1 in seen and seen[j - 1] > target)))
    return k, len(seen), seen


def _check_simplify(simplify_cell_voxels, simplify_faces):
    if simplify_cell_voxels is not None and simplify_faces is not None:
        raise ValueError("simplify_cell_voxels and simplify_faces exclude each other")
    if simplify_cell_voxels is not None and not (float(simplify_cell_voxels) > 0 and math.isfinite(float(simplify_cell_voxels))):
        raise ValueError(f"simplify_cell_voxels {simplify_cell_voxels} must be positive and finite")
    if simplify_faces is not None and int(simplify_faces) < 1:
        raise ValueError(f"simplify_faces {simplify_faces} must be at least 1")


def simplify_mesh(rows, faces, n_classes: int, lo, h: float, dims, world=None, cell_voxels=None, target_faces=None):
    """The simplification stage of the mesh exports, on the model-frame mesh (after the ``--material`` filter): one of ``cell_voxels``
    (the cell edge in voxel edges) and ``target_faces`` (the ladder search) -> (mesh dict of ``ops.mesh_simplify`` or None if the mesh
    already has at most ``target_faces`` faces and is left untouched, summary {"simplified_from", "cell_voxels", "probes"})."""
    from . import ops

    F = int(faces.shape[0])
    probes = 0
    if cell_voxels is not None:
        e = simplify_edge(h, cell_voxels)
    else:
        if F <= int(target_faces):
            return None, {"simplified_from": F, "cell_voxels": None, "probes": 0}
        rungs = simplify_ladder(lo, h, dims)
        k, probes, _ = simplify_search(lambda j: ops.mesh_simplify_count(rows, faces, n_classes, simplify_origin(lo, rungs[j - 1]), rungs[j - 1]),
                                       len(rungs), int(target_faces))
        e = rungs[k - 1]
    mesh = ops.mesh_simplify(rows, faces, n_classes, simplify_origin(lo, e), e, world)
    return mesh, {"simplified_from": F, "cell_voxels": e / float(np.float32(h)), "probes": probes}


# ---- connected components: floaters and crumbs --------------------------------------------------------------------------------------
COMPONENT_TABLE_ROWS = 16


def _check_clean(min_component_faces, min_component_fraction, keep_largest_components):
    if min_component_faces is not None and int(min_component_faces) < 1:
        raise ValueError(f"min_component_faces {min_component_faces} must be at least 1")
    if min_component_fraction is not None and not 0.0 < float(min_component_fraction) <= 1.0:
        raise ValueError(f"min_component_fraction {min_component_fraction} must lie in (0, 1]")
    if keep_largest_components is not None and int(keep_largest_components) < 1:
        raise ValueError(f"keep_largest_components {keep_largest_components} must be at least 1")


def _clean_criteria(min_component_faces, min_component_fraction, keep_largest_components) -> Dict:
    """The criteria that were given, as keywords of ``clean_mesh`` (empty: no cleaning stage)."""
    given = dict(min_component_faces=min_component_faces, min_component_fraction=min_component_fraction,
                 keep_largest_components=keep_largest_components)
    return {k: v for k, v in given.items() if v is not None}


def component_keep_mask(component_faces: torch.Tensor, min_component_faces=None, min_component_fraction=None,
                        keep_largest_components=None) -> torch.Tensor:
    """bool [K] on the device of ``component_faces`` int64 [K] (the face counts of ``ops.mesh_components``): a component is kept iff it
    has a face and meets every criterion given -- ``faces >= min_component_faces``; ``faces >= min_component_fraction * largest`` (the
    product formed in float64 and compared with the count); among the ``keep_largest_components`` components with the most faces, ties
    to the smaller component id.  No host read."""
    _check_clean(min_component_faces, min_component_fraction, keep_largest_components)
    nf = component_faces
    keep = nf > 0
    if nf.numel() == 0:
        return keep
    if min_component_faces is not None:
        keep &= nf >= int(min_component_faces)
    if min_component_fraction is not None:
        keep &= nf.double() >= float(min_component_fraction) * nf.max().double()
    if keep_largest_components is not None:
        order = torch.sort(nf, descending=True, stable=True).indices  # equal counts stay in id order
        top = torch.zeros_like(keep)
        top[order[:int(keep_largest_components)]] = True
        keep &= top
    return keep


def clean_mesh(rows, faces, n_classes: int, world=None, min_component_faces=None, min_component_fraction=None,
               keep_largest_components=None):
    """The cleaning stage of the mesh exports, on the model-frame mesh (after the ``--material`` filter, before simplification): label
    the connected components (``ops.mesh_components``), keep those that meet every criterion given (``component_keep_mask``) and emit
    their faces and vertices in input order (``ops.mesh_keep_components``; the world affine is applied there) -> (its mesh dict,
    summary {"components" (with at least one face), "components_kept", "cleaned_from" (faces before), "component_table": the 16 largest
    kept components by faces, each {"faces", "vertices", "area"}, area in the model frame}).  Reads the table back (a few hundred
    bytes) beside the operators' own reads."""
    from . import ops

    _check_clean(min_component_faces, min_component_fraction, keep_largest_components)
    comps = ops.mesh_components(rows, faces, n_classes)
    nf = comps["faces"]
    keep = component_keep_mask(nf, min_component_faces, min_component_fraction, keep_largest_components)
    mesh = ops.mesh_keep_components(rows, faces, n_classes, comps, keep, world)
    order = torch.sort(nf, descending=True, stable=True).indices
    top = order[keep[order]][:COMPONENT_TABLE_ROWS]
    head = torch.stack([(nf > 0).sum(), keep.sum()]).tolist()
    table = torch.stack([nf[top].double(), comps["vertices"][top].double(), comps["area"][top]], dim=1).tolist()
    return mesh, {"components": int(head[0]), "components_kept": int(head[1]), "cleaned_from": int(faces.shape[0]),
                  "component_table": [{"faces": int(f), "vertices": int(v), "area": float(a)} for f, v, a in table]}


def _rows_xyz(rows: torch.Tensor) -> torch.Tensor:
    return rows[:, :12].contiguous().view(torch.float32).view(-1, 3)


def staged_mesh(vol: Dict, world, material, clean: Dict, simplify_cell_voxels=None, simplify_faces=None):
    """The mesh of a fused volume through the optional stages, in their order: ``--material``, cleaning (``clean``: the criteria of
    ``clean_mesh``, or empty), simplification -> (rows as written, faces, n_classes, model-frame positions float32 [V, 3], the stages'
    summaries).  Every stage works on the model-frame mesh and the last one that runs applies ``world``; where ``simplify_faces`` leaves
    the mesh untouched, the rows of the stage before are made again in the world frame."""
    simplifying = simplify_cell_voxels is not None or simplify_faces is not None
    rows0, faces0, n_classes = extract_mesh(vol, None, material)
    rows, faces, positions, extra = rows0, faces0, None, {}
    if clean:
        mesh, info = clean_mesh(rows0, faces0, n_classes, None if simplifying else world, **clean)
        rows, faces, positions = mesh["rows"], mesh["faces"], mesh["positions"]
        extra.update(info)
    if simplifying:
        mesh, info = simplify_mesh(rows, faces, n_classes, vol["lo"], vol["h"], vol["dims"], world, simplify_cell_voxels, simplify_faces)
        extra.update(info)
        if mesh is not None:
            rows, faces, positions = mesh["rows"], mesh["faces"], mesh["positions"]
        elif world is not None:  # left untouched
            positions = _rows_xyz(rows)
            rows = clean_mesh(rows0, faces0, n_classes, world, **clean)[0]["rows"] if clean else extract_mesh(vol, world, material)[0]
    if positions is None:
        positions = _rows_xyz(rows0)
        if world is not None:
            rows = extract_mesh(vol, world, material)[0]
    return rows, faces, n_classes, positions, extra


def _world_affine(pipeline, save_world_frame: bool):
    if not save_world_frame:
        return None
    out = pipeline.datamanager.train_dataparser_outputs
    return world_frame_affine(out.dataparser_transform, out.dataparser_scale)


def export_tsdf_mesh(pipeline, output_dir, resolution=128, bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
                     downscale_factor: float = 2, batch_size: int = 8, truncation_voxels: float = 5.0, opacity_threshold: float = 0.5,
                     save_world_frame: bool = False, material: Optional[int] = None, depth_output_name: str = "depth",
                     rgb_output_name: str = "rgb", timings: Optional[Dict[str, float]] = None, simplify_cell_voxels: Optional[float] = None,
                     simplify_faces: Optional[int] = None, min_component_faces: Optional[int] = None,
                     min_component_fraction: Optional[float] = None, keep_largest_components: Optional[int] = None) -> Dict:
    """Write ``mesh.ply`` into ``output_dir`` -> {"vertices", "faces", "cameras", "resolution", "voxel_size", "truncation", "file"}.
    See the module text for the rules.  ``timings``: a dict that receives the seconds spent in render / fuse / extract / write (each
    behind a device synchronisation: a measuring aid).  ``simplify_cell_voxels`` / ``simplify_faces`` (one at most): the mesh is
    extracted in the model frame, filtered by ``material``, then simplified (``simplify_mesh``; the world affine is applied there), and
    the summary gains "simplified_from", "cell_voxels" and "probes".  ``min_component_faces`` / ``min_component_fraction`` /
    ``keep_largest_components`` (any of them, combined with AND): the components that fail are dropped after the ``material`` filter
    and before the simplification (``clean_mesh``), and the summary gains "components", "components_kept", "cleaned_from" and
    "component_table".  With none of them nothing of that runs."""
    _check_simplify(simplify_cell_voxels, simplify_faces)
    _check_clean(min_component_faces, min_component_fraction, keep_largest_components)
    clean = _clean_criteria(min_component_faces, min_component_fraction, keep_largest_components)
    clock = _stage_clock(timings, ("render", "fuse", "extract", "write"), pipeline.datamanager.train_split.device)
    world = _world_affine(pipeline, save_world_frame)
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    fused = fuse_tsdf_volume(pipeline, resolution, bounding_box_min, bounding_box_max, downscale_factor, batch_size, truncation_voxels,
                             opacity_threshold, depth_output_name, rgb_output_name, clock)
    t0 = time.perf_counter() if clock else 0.0
    extra = {}
    if simplify_cell_voxels is None and simplify_faces is None and not clean:
        rows, faces, n_classes = extract_mesh(fused["volume"], world, material)
    else:
        rows, faces, n_classes, _, extra = staged_mesh(fused["volume"], world, material, clean, simplify_cell_voxels, simplify_faces)
    if clock:
        t0 = clock("extract", t0)
    path = output_dir / MESH_NAME
    write_mesh_ply(path, rows, faces, n_classes)
    if clock:
        clock("write", t0)
    return {"vertices": int(rows.shape[0]), "faces": int(faces.shape[0]), "cameras": fused["cameras"], "resolution": list(fused["dims"]),
            "voxel_size": fused["voxel_size"], "truncation": fused["truncation"], "file": str(path), **extra}


# ---- the textured mesh -------------------------------------------------------------------------------------------------------------
OBJ_NAME, MTL_NAME, MATERIAL_NAME = "mesh.obj", "material_0.mtl", "material_0"
TEXTURE_BAND_TEXELS = 1 << 20  # texels rendered per band of atlas rows


def write_textured_obj(path, positions: np.ndarray, uv: np.ndarray, faces: np.ndarray, mtl_name: str = MTL_NAME,
                       material_name: str = MATERIAL_NAME) -> None:
    """``mesh.obj``: ``mtllib``, ``usemtl``, V lines ``v x y z``, 3 F lines ``vt u v`` (face f's corners are lines 3f .. 3f+2), F lines
    ``f a/ta b/tb c/tc``, 1-based.  Every float as ``%.9g``: a float32 read back is the float32 written."""
    positions = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    if uv.shape[0] != 3 * faces.shape[0]:
        raise ValueError(f"write_textured_obj: {uv.shape[0]} vt for {faces.shape[0]} faces (three each)")
    corner = 3 * np.arange(faces.shape[0], dtype=np.int64)[:, None] + np.arange(1, 4, dtype=np.int64)[None, :]
    pairs = np.stack([faces + 1, corner], axis=2).reshape(-1, 6)
    with open(path, "w", encoding="ascii", newline="\n") as f:
        f.write(f"mtllib {mtl_name}\nusemtl {material_name}\n")
        np.savetxt(f, positions.astype(np.float64), fmt="v %.9g %.9g %.9g")
        np.savetxt(f, uv.astype(np.float64), fmt="vt %.9g %.9g")
        np.savetxt(f, pairs, fmt="f %d/%d %d/%d %d/%d")


def write_mtl(path, texture_name: str, material_name: str = MATERIAL_NAME) -> None:
    """``material_0.mtl``: one unlit white material whose ``map_Kd`` is the first texture."""
    with open(path, "w", encoding="ascii", newline="\n") as f:
        f.write(f"newmtl {material_name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nd 1\nillum 1\nmap_Kd {texture_name}\n")


def default_ray_length(positions: torch.Tensor, faces: torch.Tensor) -> float:
    """Twice the mean length of edge V0 V1 over the faces  [upstream-recalled: nerfstudio's texture_utils takes
    ``2 * mean |v1 - v0|``]: a float64 mean on the device, read once, rounded to float32."""
    f = faces.long()
    edge = positions[f[:, 1]].double() - positions[f[:, 0]].double()
    return float(np.float32(2.0 * float(torch.linalg.vector_norm(edge, dim=1).mean())))


def texture_file_names(texture_output_names: Sequence[str]) -> Dict[str, str]:
    """name -> file: the first texture is ``material_0.png`` (what the .mtl points at), the others ``texture_<name>.png``."""
    names = list(texture_output_names)
    if len(names) < 1 or len(set(names)) != len(names):
        raise ValueError(f"texture_output_names {names}: at least one name, each once")
    return {name: (MATERIAL_NAME + ".png" if k == 0 else f"texture_{name}.png") for k, name in enumerate(names)}


def texture_bands(side: int, band_texels: Optional[int] = None):
    """[(first row, end row)] of the atlas walk: whole rows, at most ``band_texels`` texels each (None: ``TEXTURE_BAND_TEXELS``; one
    row if a row is longer)."""
    rows = max(1, int(TEXTURE_BAND_TEXELS if band_texels is None else band_texels) // int(side))
    return [(r, min(r + rows, side)) for r in range(0, side, rows)]


def render_texel_band(model, rays: Dict, rows: int, side: int, names: Sequence[str]) -> Dict[str, torch.Tensor]:
    """One band of ``ops.texture_rays`` rendered without gradients -> {name: [rows, side, k]}: the caller has put the model in eval
    mode."""
    from ._ns_compat import RayBundle

    shape = (rows, side)
    rb = RayBundle(origins=rays["origins"].view(*shape, 3), directions=rays["directions"].view(*shape, 3),
                   nears=rays["nears"].view(*shape, 1), fars=rays["fars"].view(*shape, 1))
    return model.get_outputs_for_camera_ray_bundle(rb, output_names=names)


def compose_texel_band(outputs: Dict[str, torch.Tensor], name: str, ray_length: float, texel_face: torch.Tensor, out: torch.Tensor) -> None:
    """The bytes of one named output of a band into ``out`` uint8 [rows, side, 3] (``render.compose_frame``, a depth output mapped over
    [0, ray_length]: the same scale in every band); texels nobody owns are 0."""
    from .render import compose_frame

    compose_frame(outputs, [name], depth_near_plane=0.0, depth_far_plane=float(ray_length), out=out)
    out[texel_face.view(out.shape[0], out.shape[1]) < 0] = 0


def write_png(image: torch.Tensor, path, png_encoder: str = "host") -> str:
    """``image`` (uint8 [H, W, 3] on the device) as a PNG file -> who encoded it.  ``gpu``: ``ops.png_encode``, unless the image is
    outside what it takes (a side above 65535, or no bound on the file): then the host encoder, with a message."""
    from . import ops

    H, W, ch = (int(v) for v in image.shape)
    if png_encoder == "gpu" and (H > 65535 or W > 65535 or ops.png_max_bytes(H, W, ch) == 0):
        print(f"{path}: {H} x {W} is outside what the device PNG encoder takes; encoding on the host", file=sys.stderr)
        png_encoder = "host"
    if png_encoder == "gpu":
        data, length = ops.png_encode(image.contiguous())
        Path(path).write_bytes(data[:int(length.item())].cpu().numpy().tobytes())
    else:
        from PIL import Image

        Image.fromarray(image.cpu().numpy()).save(path)
    return png_encoder


def export_textured_mesh(pipeline, output_dir, resolution=128, bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
                         downscale_factor: float = 2, batch_size: int = 8, truncation_voxels: float = 5.0, opacity_threshold: float = 0.5,
                         save_world_frame: bool = False, material: Optional[int] = None, depth_output_name: str = "depth",
                         rgb_output_name: str = "rgb", px_per_uv_triangle: int = 4, ray_length: Optional[float] = None,
                         texture_output_names: Sequence[str] = ("rgb",), cube_output_names: Sequence[str] = (),
                         timings: Optional[Dict[str, float]] = None, simplify_cell_voxels: Optional[float] = None,
                         simplify_faces: Optional[int] = None, min_component_faces: Optional[int] = None,
                         min_component_fraction: Optional[float] = None, keep_largest_components: Optional[int] = None,
                         png_encoder: str = "host") -> Dict:
    """Write ``mesh.obj``, ``material_0.mtl``, ``material_0.png`` (and ``texture_<name>.png`` / ``texture_<name>.npy``) into
    ``output_dir`` -> {"vertices", "faces", "atlas_side", "px_per_uv_triangle", "ray_length", "textures", "cubes", "file"}.  The mesh
    is ``export_tsdf_mesh``'s (same arguments, same faces); every face gets its own triangle of the atlas (``ops.texture_atlas``), and
    every texel holds what the model renders along a ray of ``ray_length`` through the surface there (``ops.texture_rays``; None:
    ``default_ray_length``).  The rays are made from the model-frame positions; ``save_world_frame`` moves the written ``v`` lines
    only.  Texels nobody owns are 0, in the cubes as well.  ``timings``: a dict that receives the seconds spent in mesh (render, fuse,
    extract) / rays / render / compose / write (each behind a device synchronisation: a measuring aid).  ``simplify_cell_voxels`` /
    ``simplify_faces`` (one at most): atlas, uv and texel rays are those of the simplified mesh (``simplify_mesh``), whose model-frame
    positions make the rays and whose rows give the ``v`` lines; the summary gains "simplified_from", "cell_voxels" and "probes".
    ``min_component_faces`` / ``min_component_fraction`` / ``keep_largest_components``: as in ``export_tsdf_mesh`` -- the atlas holds
    the faces of the kept components only.  ``png_encoder="gpu"``: the atlases, which are device tensors, are encoded there
    (``ops.png_encode``: lossless, the same pixels) and only the files' bytes come to the host; an atlas the device encoder does not
    take goes to the host encoder with a message."""
    from . import ops
    from .render import source_keys

    if png_encoder not in ("host", "gpu"):
        raise ValueError(f"png_encoder must be host or gpu, got {png_encoder!r}")

    _check_simplify(simplify_cell_voxels, simplify_faces)
    _check_clean(min_component_faces, min_component_fraction, keep_largest_components)
    clean = _clean_criteria(min_component_faces, min_component_fraction, keep_largest_components)
    p = int(px_per_uv_triangle)
    if p < 4:
        raise ValueError(f"px_per_uv_triangle {p} must be at least 4")
    if ray_length is not None and not (float(ray_length) > 0 and math.isfinite(float(ray_length))):
        raise ValueError(f"ray_length {ray_length} must be positive and finite")
    files = texture_file_names(texture_output_names)
    cube_names = list(cube_output_names)
    if len(set(cube_names)) != len(cube_names):
        raise ValueError(f"cube_output_names {cube_names}: each name once")
    model, dev = pipeline.model, pipeline.datamanager.train_split.device
    clock = _stage_clock(timings, ("mesh", "rays", "render", "compose", "write"), dev)
    world = _world_affine(pipeline, save_world_frame)
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)

    t0 = time.perf_counter() if clock else 0.0
    fused = fuse_tsdf_volume(pipeline, resolution, bounding_box_min, bounding_box_max, downscale_factor, batch_size, truncation_voxels,
                             opacity_threshold, depth_output_name, rgb_output_name)
    rows, faces, _, positions, extra = staged_mesh(fused["volume"], world, material, clean, simplify_cell_voxels, simplify_faces)
    F = int(faces.shape[0])
    if F < 1:
        raise ValueError("the mesh has no face to texture: nothing opaque inside the bounding box"
                         + ("" if material is None else f" is labelled {material}")
                         + (" and passes the component criteria" if clean else ""))
    _, T = ops.texture_atlas(F, p)  # (refuses an atlas above 16384 x 16384 before anything is rendered)
    faces = faces.contiguous()
    written = _rows_xyz(rows)  # the rays from the model-frame positions, the v lines from the rows (world applied there)
    L = default_ray_length(positions, faces) if ray_length is None else float(np.float32(float(ray_length)))
    if not (L > 0 and math.isfinite(L)):
        raise ValueError(f"the mean edge length of the mesh gives a ray length of {L}; pass ray_length")
    uv = ops.texture_uv(F, p, dev)
    if clock:
        t0 = clock("mesh", t0)

    atlases = {name: torch.empty(T, T, 3, dtype=torch.uint8, device=dev) for name in files}
    keys = source_keys(list(files), cube_names)
    cubes, cube_files = {}, {}
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for r0, r1 in texture_bands(T):
                rays = ops.texture_rays(positions, faces, p, L, r0 * T, r1 * T)
                if clock:
                    t0 = clock("rays", t0)
                outputs = render_texel_band(model, rays, r1 - r0, T, keys)
                if clock:
                    t0 = clock("render", t0)
                for name in files:
                    compose_texel_band(outputs, name, L, rays["texel_face"], atlases[name][r0:r1])
                if clock:
                    t0 = clock("compose", t0)
                empty = (rays["texel_face"] < 0).view(r1 - r0, T)
                for name in cube_names:
                    if name not in outputs:
                        raise ValueError(f"the model returned no {name!r} output for a cube; it returns: {', '.join(outputs)}")
                    band = outputs[name].float().masked_fill(empty[..., None], 0.0)
                    if name not in cubes:
                        cube_files[name] = str(output_dir / f"texture_{name}.npy")
                        cubes[name] = np.lib.format.open_memmap(cube_files[name], mode="w+", dtype=np.float32, shape=(T, T, band.shape[-1]))
                    cubes[name][r0:r1] = band.cpu().numpy()
                if clock:
                    t0 = clock("write", t0)
    finally:
        model.train(was_training)
    for mm in cubes.values():
        mm.flush()
    del cubes

    textures = {}
    for name, file in files.items():
        textures[name] = str(output_dir / file)
        write_png(atlases[name], textures[name], png_encoder)
    write_mtl(output_dir / MTL_NAME, files[next(iter(files))])
    path = output_dir / OBJ_NAME
    write_textured_obj(path, written.cpu().numpy(), uv.cpu().numpy(), faces.cpu().numpy())
    if clock:
        clock("write", t0)
    return {"vertices": int(positions.shape[0]), "faces": F, "atlas_side": T, "px_per_uv_triangle": p, "ray_length": L,
            "textures": textures, "cubes": cube_files, "file": str(path), **extra}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _bool(s: str) -> bool:
    return s.lower() in ("1", "true", "yes")


def _add_common_arguments(p) -> None:
    """The flags ``pointcloud`` and ``tsdf`` spell alike (each parser adds them where its own help lists them)."""
    p.add_argument("--save-world-frame", type=_bool, nargs="?", const=True, default=False,
                   help="undo dataparser_transform / dataparser_scale in the written xyz")
    p.add_argument("--opacity-threshold", type=float, default=0.5)
    # (absent from the namespace unless given, as --normal-method is)
    p.add_argument("--material-edits", default=argparse.SUPPRESS, metavar="FILE",
                   help="export the scene under the material edits of this JSON file, e.g. with a material removed (INTEGRATION.md)")


def _add_tsdf_parser(sub, textured: bool = False):
    """The ``tsdf`` parser, or with ``textured`` the ``textured-mesh`` one: the same flags, and the texture's own where ``tsdf`` keeps
    hidden ones to refuse."""
    from .eval import add_model_arguments

    if textured:
        ts = sub.add_parser("textured-mesh", help="export the tsdf mesh with a texture atlas rendered by the model (ns-export tsdf "
                                                  "--texture-method nerf)")
    else:
        ts = sub.add_parser("tsdf", help="export a material-labelled triangle mesh (ns-export tsdf)")
    add_model_arguments(ts)
    ts.add_argument("--output-dir", required=True, help="directory for mesh.obj, material_0.mtl and the textures" if textured
                    else "directory for mesh.ply")
    # the flags of ns-export tsdf  [upstream-recalled]
    ts.add_argument("--resolution", type=int, nargs="+", default=[128], metavar="N",
                    help="lattice points along the longest side of the box (voxels stay cubic), or three integers")
    ts.add_argument("--bounding-box-min", type=float, nargs=3, default=[-1.0, -1.0, -1.0], metavar=("X", "Y", "Z"))
    ts.add_argument("--bounding-box-max", type=float, nargs=3, default=[1.0, 1.0, 1.0], metavar=("X", "Y", "Z"))
    ts.add_argument("--downscale-factor", type=float, default=2, help="the training cameras are rendered at 1 / this of their resolution")
    ts.add_argument("--batch-size", type=int, default=8, help="cameras rendered and fused per launch")
    ts.add_argument("--truncation-voxels", type=float, default=5.0, help="truncation distance in voxel edges")
    ts.add_argument("--depth-output-name", default="depth")
    ts.add_argument("--rgb-output-name", default="rgb")
    _add_common_arguments(ts)
    ts.add_argument("--material", type=int, default=None, metavar="K", help="keep only the faces whose three vertices are labelled K")
    sg = ts.add_mutually_exclusive_group()
    sg.add_argument("--simplify-cell-voxels", type=float, default=None, metavar="X",
                    help="simplify by vertex clustering: merge the vertices of every cubic cell of X voxel edges (X > 0)")
    sg.add_argument("--simplify-faces", type=int, default=None, metavar="N",
                    help="simplify by vertex clustering with the finest cell edge h 2^(k/4) that leaves at most N faces (N >= 1)")
    ts.add_argument("--min-component-faces", type=int, default=None, metavar="N",
                    help="drop the connected components with fewer than N faces (N >= 1); runs after --material, before the simplification")
    ts.add_argument("--min-component-fraction", type=float, default=None, metavar="R",
                    help="drop the components with fewer than R times the faces of the largest one (0 < R <= 1)")
    ts.add_argument("--keep-largest-components", type=int, default=None, metavar="K",
                    help="keep only the K components with the most faces (K >= 1; ties to the one with the smaller first vertex)")
    if textured:
        ts.add_argument("--px-per-uv-triangle", type=int, default=4, metavar="P",
                        help="texels along the side of a face's atlas triangle, at least 4 (the atlas holds two faces per P x P square)")
        ts.add_argument("--ray-length", type=float, default=None, metavar="L",
                        help="length of a texel's ray through the surface (default: twice the mean length of the faces' first edge)")
        ts.add_argument("--texture-output-names", nargs="+", default=["rgb"], metavar="NAME",
                        help="rendered outputs written as textures; the first is material_0.png, the others texture_<NAME>.png")
        ts.add_argument("--cube-output-names", nargs="*", default=[], metavar="NAME",
                        help="rendered outputs written whole as texture_<NAME>.npy, float32 [T, T, channels]")
        # (absent from the namespace unless given, as --material-edits is; absent means host)
        ts.add_argument("--png-encoder", default=argparse.SUPPRESS, choices=["host", "gpu"],
                        help="who encodes material_0.png and texture_<NAME>.png: PIL on the host (the default), or the PNG encoder on the device")
    else:  # not built here  [upstream-recalled]; the textured-mesh command has the per-face atlas
        ts.add_argument("--texture-method", default=None, help=argparse.SUPPRESS)
        ts.add_argument("--unwrap-method", default=None, help=argparse.SUPPRESS)
        ts.add_argument("--px-per-uv-triangle", default=None, help=argparse.SUPPRESS)
    # not built  [upstream-recalled]
    ts.add_argument("--num-pixels-per-side", default=None, help=argparse.SUPPRESS)
    ts.add_argument("--target-num-faces", default=None, help=argparse.SUPPRESS)
    return ts


def _check_tsdf_args(ts, args) -> None:
    if args.command == "textured-mesh":
        from .ops.export import TEXTURE_MAX_SIDE

        if args.px_per_uv_triangle < 4:
            ts.error(f"--px-per-uv-triangle {args.px_per_uv_triangle}: at least 4 (a face's triangle is inset by 3 texels)")
        if args.px_per_uv_triangle > TEXTURE_MAX_SIDE:
            ts.error(f"--px-per-uv-triangle {args.px_per_uv_triangle}: the atlas would exceed {TEXTURE_MAX_SIDE} x {TEXTURE_MAX_SIDE} "
                     "texels; lower it (or --resolution)")
        if args.ray_length is not None and not (args.ray_length > 0 and math.isfinite(args.ray_length)):
            ts.error(f"--ray-length {args.ray_length}: positive and finite")
        if args.num_pixels_per_side is not None:
            ts.error("--num-pixels-per-side is not available: the atlas side follows from the face count and --px-per-uv-triangle")
    elif any(v is not None for v in (args.texture_method, args.unwrap_method, args.px_per_uv_triangle, args.num_pixels_per_side)):
        ts.error("texture unwrapping is not available in tsdf (no chart unwrapper here): the mesh carries vertex colours, material "
                 "labels and abundances; the textured-mesh command writes it with a per-face texture atlas")
    if args.target_num_faces is not None:
        ts.error("--target-num-faces is not available (no edge-collapse decimator to an exact count here): use --simplify-faces N, "
                 "vertex clustering that leaves at most N faces, or lower --resolution")
    if args.simplify_cell_voxels is not None and not (args.simplify_cell_voxels > 0 and math.isfinite(args.simplify_cell_voxels)):
        ts.error(f"--simplify-cell-voxels {args.simplify_cell_voxels}: positive and finite")
    if args.simplify_faces is not None and args.simplify_faces < 1:
        ts.error(f"--simplify-faces {args.simplify_faces}: at least 1")
    if args.min_component_faces is not None and args.min_component_faces < 1:
        ts.error(f"--min-component-faces {args.min_component_faces}: at least 1")
    if args.min_component_fraction is not None and not 0.0 < args.min_component_fraction <= 1.0:
        ts.error(f"--min-component-fraction {args.min_component_fraction}: above 0 and at most 1")
    if args.keep_largest_components is not None and args.keep_largest_components < 1:
        ts.error(f"--keep-largest-components {args.keep_largest_components}: at least 1")
    if len(args.resolution) not in (1, 3) or min(args.resolution) < 2:
        ts.error(f"--resolution {args.resolution}: one integer or three, each at least 2")
    if args.batch_size < 1 or not args.truncation_voxels > 0 or not args.downscale_factor > 0:
        ts.error("--batch-size, --truncation-voxels and --downscale-factor must be positive")
    if any(a >= b for a, b in zip(args.bounding_box_min, args.bounding_box_max)):
        ts.error("--bounding-box-min must lie below --bounding-box-max on every axis")


def parse_args(argv=None) -> argparse.Namespace:
    from .eval import add_model_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.export", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    pc = sub.add_parser("pointcloud", help="export a material-labelled point cloud (ns-export pointcloud)")
    add_model_arguments(pc)
    pc.add_argument("--output-dir", required=True, help="directory for point_cloud.ply (and point_cloud_spectral.npy)")
    pc.add_argument("--num-points", type=int, default=1000000)
    pc.add_argument("--remove-outliers", type=_bool, nargs="?", const=True, default=True)
    pc.add_argument("--std-ratio", type=float, default=10.0)
    pc.add_argument("--nb-neighbors", type=int, default=20)
    pc.add_argument("--depth-output-name", default="depth")
    pc.add_argument("--rgb-output-name", default="rgb")
    pc.add_argument("--num-rays-per-batch", type=int, default=32768)
    pc.add_argument("--obb-center", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    pc.add_argument("--obb-rotation", type=float, nargs=3, default=None, metavar=("RX", "RY", "RZ"), help="Euler angles, radians")
    pc.add_argument("--obb-scale", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"))
    _add_common_arguments(pc)
    pc.add_argument("--seed", type=int, default=0)
    pc.add_argument("--spectra", action="store_true", help="also write point_cloud_spectral.npy, float32 [M, B], rows in file order")
    pc.add_argument("--material", type=int, default=None, metavar="K", help="keep only the points whose material label is K")
    # (absent from the namespace unless given: the set of the point cloud's defaults is pinned by tests/test_mesh_cpu.py)
    pc.add_argument("--normal-method", default=argparse.SUPPRESS, metavar="{none,analytic}",
                    help="analytic: write float nx ny nz, the model's density-gradient normals (default none)")
    ts = _add_tsdf_parser(sub)
    tm = _add_tsdf_parser(sub, textured=True)
    args = ap.parse_args(argv)
    if args.command in ("tsdf", "textured-mesh"):
        _check_tsdf_args(ts if args.command == "tsdf" else tm, args)
        return args
    given = [v is not None for v in (args.obb_center, args.obb_rotation, args.obb_scale)]
    if any(given) and not all(given):
        pc.error("--obb-center, --obb-rotation and --obb-scale come together: all three or none")
    if getattr(args, "normal_method", "none") not in NORMAL_METHODS:
        pc.error(f"--normal-method {args.normal_method}: not available (no Open3D estimate and no learned normals here); use "
                 "--normal-method analytic, the normals of the model's own density gradient, or none")
    if not 2 <= args.nb_neighbors <= 32:
        pc.error(f"--nb-neighbors {args.nb_neighbors}: 2..32")
    return args


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from .materials import load_for_model

    args = parse_args(argv)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    edits_file = getattr(args, "material_edits", None)
    edits = load_for_model(edits_file, pipeline.model)  # (a bad edit file is refused here, before anything is rendered)
    with pipeline.model.material_edits_context(edits):  # (None: nothing changes)
        result = _run(pipeline, args)
    if edits_file is not None:
        result["material_edits"] = str(edits_file)
    print(json.dumps(result))
    return result


def _run(pipeline, args) -> dict:
    if args.command == "textured-mesh":
        return export_textured_mesh(pipeline, args.output_dir, args.resolution if len(args.resolution) == 3 else args.resolution[0],
                                    args.bounding_box_min, args.bounding_box_max, args.downscale_factor, args.batch_size,
                                    args.truncation_voxels, args.opacity_threshold, args.save_world_frame, args.material,
                                    args.depth_output_name, args.rgb_output_name, args.px_per_uv_triangle, args.ray_length,
                                    args.texture_output_names, args.cube_output_names, simplify_cell_voxels=args.simplify_cell_voxels,
                                    simplify_faces=args.simplify_faces, min_component_faces=args.min_component_faces,
                                    min_component_fraction=args.min_component_fraction,
                                    keep_largest_components=args.keep_largest_components,
                                    png_encoder=getattr(args, "png_encoder", "host"))
    if args.command == "tsdf":
        return export_tsdf_mesh(pipeline, args.output_dir, args.resolution if len(args.resolution) == 3 else args.resolution[0],
                                args.bounding_box_min, args.bounding_box_max, args.downscale_factor, args.batch_size,
                                args.truncation_voxels, args.opacity_threshold, args.save_world_frame, args.material,
                                args.depth_output_name, args.rgb_output_name, simplify_cell_voxels=args.simplify_cell_voxels,
                                simplify_faces=args.simplify_faces, min_component_faces=args.min_component_faces,
                                min_component_fraction=args.min_component_fraction, keep_largest_components=args.keep_largest_components)
    return export_pointcloud(pipeline, args.output_dir, args.num_points, args.remove_outliers, args.std_ratio, args.nb_neighbors,
                             args.depth_output_name, args.rgb_output_name, args.num_rays_per_batch, args.obb_center, args.obb_rotation,
                             args.obb_scale, args.save_world_frame, args.opacity_threshold, args.seed, args.spectra, args.material,
                             normal_method=getattr(args, "normal_method", "none"))


if __name__ == "__main__":
    main()
    sys.exit(0)
