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
the last batch is cut in draw order); 64 consecutive batches that keep nothing raise instead of spinning; normals are not estimated.

The file, ``point_cloud.ply``: binary little-endian PLY, ``float x y z, uchar red green blue alpha`` and -- for ``spectral`` and
``rgb+spectral`` -- ``int material, float abundance_0 .. abundance_{C-1}``.  ``--spectra`` also writes ``point_cloud_spectral.npy``
(float32 [M, B], rows in file order); ``--material K`` keeps the points labelled K."""
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
def ply_header(n_points: int, n_classes: int) -> bytes:
    props = ["float x", "float y", "float z", "uchar red", "uchar green", "uchar blue", "uchar alpha"]
    if n_classes:
        props += ["int material"] + [f"float abundance_{i}" for i in range(n_classes)]
    lines = ["ply", "format binary_little_endian 1.0", "comment umhsnerf.export pointcloud", f"element vertex {int(n_points)}"]
    return ("\n".join(lines + ["property " + p for p in props] + ["end_header"]) + "\n").encode("ascii")


def write_ply(path, rows: torch.Tensor, n_classes: int) -> None:
    """``rows`` uint8 [M, row_bytes] (device or host) -> a binary little-endian PLY: the header and the rows, one ``write`` each, the
    rows from a pinned buffer."""
    m = rows.shape[0]
    host = rows
    if rows.is_cuda:
        host = torch.empty(rows.shape, dtype=torch.uint8).pin_memory()
        host.copy_(rows)
        torch.cuda.current_stream(rows.device).synchronize()
    with open(path, "wb") as f:
        f.write(ply_header(m, n_classes))
        f.write(host.contiguous().numpy().data)


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
                      material: Optional[int] = None, timings: Optional[Dict[str, float]] = None) -> Dict:
    """Write ``point_cloud.ply`` (and ``point_cloud_spectral.npy`` with ``spectra``) into ``output_dir`` -> {"points", "rays_drawn",
    "batches", "removed_outliers", "threshold", "file"}.  See the module text for the rules.  ``timings``: a dict that receives the
    seconds spent in render / emit / neighbour search / file write (each behind a device synchronisation: a measuring aid)."""
    from . import ops

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

    was_training = model.training
    model.eval()
    rows = points = kept = spec_rows = None
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
                base += ops.pc_append(args, rows, points, kept, base, batches * R, num_points)
                new_count = min(int(base), num_points)  # the one device read of a batch: 8 bytes
                if spec_rows is not None and new_count > count:
                    spec_rows[count:new_count] = outputs["spectral"][kept[count:new_count] - batches * R]
                if clock:
                    clock("emit", t0)
                empty = empty + 1 if new_count == count else 0
                count, batches = new_count, batches + 1
                if empty >= MAX_EMPTY_BATCHES:
                    raise RuntimeError(f"nothing kept in {MAX_EMPTY_BATCHES} consecutive batches of {R} rays ({count} of {num_points} "
                                       "points so far): an empty crop box, an opacity threshold nothing reaches, or an untrained model")
    finally:
        model.train(was_training)

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
    path = output_dir / PLY_NAME
    write_ply(path, table, n_classes)
    if spec_rows is not None:
        np.save(output_dir / SPECTRA_NAME, spec_rows[keep].cpu().numpy())
    if clock:
        clock("write", t0)
    return {"points": int(table.shape[0]), "rays_drawn": batches * R, "batches": batches, "removed_outliers": removed,
            "threshold": threshold, "file": str(path)}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _bool(s: str) -> bool:
    return s.lower() in ("1", "true", "yes")


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
    pc.add_argument("--save-world-frame", type=_bool, nargs="?", const=True, default=False,
                    help="undo dataparser_transform / dataparser_scale in the written xyz")
    pc.add_argument("--opacity-threshold", type=float, default=0.5)
    pc.add_argument("--seed", type=int, default=0)
    pc.add_argument("--spectra", action="store_true", help="also write point_cloud_spectral.npy, float32 [M, B], rows in file order")
    pc.add_argument("--material", type=int, default=None, metavar="K", help="keep only the points whose material label is K")
    args = ap.parse_args(argv)
    given = [v is not None for v in (args.obb_center, args.obb_rotation, args.obb_scale)]
    if any(given) and not all(given):
        pc.error("--obb-center, --obb-rotation and --obb-scale come together: all three or none")
    if not 2 <= args.nb_neighbors <= 32:
        pc.error(f"--nb-neighbors {args.nb_neighbors}: 2..32")
    return args


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint

    args = parse_args(argv)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    result = export_pointcloud(pipeline, args.output_dir, args.num_points, args.remove_outliers, args.std_ratio, args.nb_neighbors,
                               args.depth_output_name, args.rgb_output_name, args.num_rays_per_batch, args.obb_center, args.obb_rotation,
                               args.obb_scale, args.save_world_frame, args.opacity_threshold, args.seed, args.spectra, args.material)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
