"""Export operators: packed point-cloud rows, exact k-NN mean distances, TSDF fusion and mesh extraction, the texture atlas and its
texel rays, mesh simplification by vertex clustering, connected components of a mesh and the mesh of the kept ones."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from .. import _hip
from .._hip import ptr


# ---- point-cloud export (umhs_pointcloud.hip) ---------------------------------------------------------------------------------------
PC_MAX_CELLS, PC_MAX_DIM = 1 << 21, 4096  # umhs_pc_cell_keys / umhs_knn_mean_dist: cells of a grid, cells along one axis


def pc_row_bytes(n_classes: int) -> int:
    """Bytes of one packed row: 16 (x y z, red green blue alpha) or 20 + 4 C (the same, int material, C float abundances)."""
    return 16 if n_classes == 0 else 20 + 4 * int(n_classes)


def _pc_rows(t, n: int, cols: int, what: str, dev):
    """(tensor kept alive, floats per row) of a float32 source of n rows with at least ``cols`` adjacent columns, read in place."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"pc: {what} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32 or t.device != dev:
        raise ValueError(f"pc: {what} must be float32 on {dev}, got {t.dtype} on {t.device}")
    rows = t.reshape(n, 1) if t.dim() <= 1 else t
    if rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < cols or (rows.shape[1] > 1 and rows.stride(1) != 1):
        raise ValueError(f"pc: {what} must be [{n}, >={cols}] with adjacent columns, got {tuple(t.shape)} strides {tuple(t.stride())}")
    stride = rows.stride(0) if n > 1 else rows.shape[1]
    if stride < cols or stride >= 1 << 31:
        raise ValueError(f"pc: the rows of {what} overlap or are too far apart (stride {stride})")
    return rows, stride


def pc_args(origins, directions, depth, accumulation, rgb, abundances=None, seg_probs=None, threshold: float = 0.5, box=None, world=None):
    """umhs_pc_args of one batch of rendered rays -> (struct, n_rays, n_classes, tensors to keep alive).  Sources: float32 [R, c] on one
    device, read in place at their own row stride.  ``abundances`` / ``seg_probs`` (both or neither, [R, C]) select the 20 + 4 C byte
    row.  ``box`` = (T [3], R [3,3], S [3]) of an oriented box (host values); ``world`` = [3,4] host affine for the written xyz."""
    if (abundances is None) != (seg_probs is None):
        raise ValueError("pc: abundances and seg_probs come together (or neither: the 16-byte row)")
    n, dev = origins.shape[0], origins.device
    C_ = 0 if abundances is None else int(abundances.shape[-1])
    if C_ and seg_probs.shape[-1] != C_:
        raise ValueError(f"pc: {C_} abundances but {seg_probs.shape[-1]} cluster probabilities per ray")
    a, keep = _hip.PcArgs(), []
    for name, t, cols in (("origins", origins, 3), ("directions", directions, 3), ("depth", depth, 1), ("accumulation", accumulation, 1),
                          ("rgb", rgb, 3), ("abundances", abundances, C_), ("seg_probs", seg_probs, C_)):
        if t is None:
            continue
        rows, stride = _pc_rows(t, n, cols, name, dev)
        keep.append(rows)
        setattr(a, name, rows.data_ptr() if n else 4)
        setattr(a, name + "_stride", stride)
    a.n_classes, a.threshold = C_, float(threshold)
    if box is not None:
        T, R, S = (np.asarray(v, dtype=np.float32) for v in box)
        if T.shape != (3,) or R.shape != (3, 3) or S.shape != (3,):
            raise ValueError("pc: box = (T [3], R [3,3], S [3])")
        a.has_box = 1
        a.box_center[:], a.box_rotation[:], a.box_scale[:] = T.tolist(), R.reshape(-1).tolist(), S.tolist()
    if world is not None:
        W = np.asarray(world, dtype=np.float32)
        if W.shape != (3, 4):
            raise ValueError("pc: world = [3,4] affine")
        a.has_world = 1
        a.world[:] = W.reshape(-1).tolist()
    return a, n, C_, keep


def pc_append(args, rows, points, kept, base, ordinal0: int, cap: int):
    """Append the kept rays of one batch (``args`` = ``pc_args(...)``) behind the ``base[0]`` rows written so far: count per chunk,
    exclusive scan (torch, a few hundred integers), emit.  ``rows`` uint8 [>= cap * row_bytes] (4-byte aligned), ``points`` float32
    [cap, 3], ``kept`` int64 [cap], ``base`` int64 [1] on the device.  -> the batch's kept count as a 0-dim int64 device tensor (the
    caller adds it to ``base``).  Rows at or beyond ``cap`` are dropped; no host sync."""
    a, n, C_, keep = args
    dev = base.device
    if (rows.dtype != torch.uint8 or not rows.is_contiguous() or rows.numel() < cap * pc_row_bytes(C_) or points.dtype != torch.float32
            or not points.is_contiguous() or points.numel() < 3 * cap or kept.dtype != torch.int64 or not kept.is_contiguous()
            or kept.numel() < cap or base.dtype != torch.int64 or base.numel() != 1):
        raise ValueError(f"pc_append: rows / points / kept / base do not hold {cap} rows of {pc_row_bytes(C_)} bytes")
    if n == 0:
        return torch.zeros((), dtype=torch.int64, device=dev)
    lib = _hip.lib()
    counts = torch.empty(int(lib.umhs_pc_chunks(n)), dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_pc_flag_count(C.byref(a), n, ptr(counts), _hip.stream()), "umhs_pc_flag_count")
    c64 = counts.to(torch.int64)
    incl = torch.cumsum(c64, 0)
    offsets = (incl - c64).contiguous()
    _hip.check(lib.umhs_pc_emit(C.byref(a), n, ptr(offsets), ptr(base), int(ordinal0), C.c_void_p(rows.data_ptr()), ptr(points),
                                ptr(kept), int(cap), _hip.stream()), "umhs_pc_emit")
    del keep
    return incl[-1]


def pc_grid(points, edge: Optional[float] = None, points_per_cell: float = 2.0):
    """The uniform grid of ``knn_mean_dist`` over the bounding box of points [M,3] -> (lo (3 floats), edge, dims (3 ints)).  Reads the
    box back (24 bytes).  ``edge`` None: the edge at which the box holds about ``points_per_cell`` points per cell; either way the edge
    grows until no axis has more than 4,096 cells and the grid no more than 2^21.  An axis without extent has one cell."""
    lo_t, hi_t = points.amin(0), points.amax(0)
    box = torch.stack([lo_t, hi_t]).double().cpu().numpy()
    lo, ext = box[0], box[1] - box[0]
    if not np.isfinite(box).all():
        raise ValueError("pc_grid: the points are not finite")
    if edge is None:
        live = ext[ext > 0]
        edge = 1.0 if live.size == 0 else float((np.prod(live) / max(points.shape[0] / points_per_cell, 1.0)) ** (1.0 / live.size))
    edge = float(np.float32(max(float(edge), float(np.finfo(np.float32).tiny))))
    while True:
        dims = [int(min(e / edge, 1e9)) + 1 for e in ext]
        if max(dims) <= PC_MAX_DIM and dims[0] * dims[1] * dims[2] <= PC_MAX_CELLS:
            return tuple(float(np.float32(v)) for v in lo), edge, tuple(dims)
        edge = float(np.float32(edge * 1.25))


def _pc_grid_c(lo, dims):
    return (_hip._f32 * 3)(*lo), (_hip._i32 * 3)(*dims)


def pc_cell_keys(points, lo, edge: float, dims):
    """int32 [M] cell keys (z-major) of points [M,3] in the grid ``pc_grid`` chose (umhs_pc_cell_keys)."""
    p = _hip.f32c(points)
    keys = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
    clo, cdims = _pc_grid_c(lo, dims)
    _hip.check(_hip.lib().umhs_pc_cell_keys(ptr(p), p.shape[0], clo, float(edge), cdims, ptr(keys), _hip.stream()), "umhs_pc_cell_keys")
    return keys


def knn_mean_dist(points, k: int, edge: Optional[float] = None):
    """float32 [M]: for every point of points [M,3] the mean Euclidean distance to its min(k, M) nearest points, itself included --
    what Open3D's ``remove_statistical_outlier`` thresholds  [upstream-recalled].  Exact.  Bin (HIP), sort by cell and build the
    cell-start table (torch: plumbing), search (HIP), scatter back to the points' order.  ``edge``: overrides the grid edge (the result
    does not depend on it; the time does)."""
    p = _hip.f32c(points)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"knn_mean_dist: points must be [M,3], got {tuple(p.shape)}")
    m, dev = p.shape[0], p.device
    if not 2 <= int(k) <= 32:
        raise ValueError(f"knn_mean_dist: k must be in 2..32, got {k}")
    if m == 0:
        return torch.empty(0, device=dev)
    plan = knn_plan(p, edge)
    mean = torch.empty(m, device=dev)
    mean[plan["order"]] = knn_search(plan, k)
    return mean


def knn_plan(p, edge: Optional[float] = None) -> Dict:
    """Everything ``knn_search`` needs of contiguous float32 points [M,3]: the grid, the points in cell order, the cell-start table."""
    lo, edge, dims = pc_grid(p, edge)
    keys = pc_cell_keys(p, lo, edge, dims)
    sorted_keys, order = torch.sort(keys, stable=True)
    cells = dims[0] * dims[1] * dims[2]
    start = torch.searchsorted(sorted_keys, torch.arange(cells + 1, dtype=torch.int32, device=p.device)).to(torch.int32)
    return {"lo": lo, "edge": edge, "dims": dims, "order": order, "points": p[order].contiguous(), "start": start}


def knn_search(plan: Dict, k: int, out=None):
    """umhs_knn_mean_dist on a ``knn_plan``: float32 [M] means in CELL order (``plan["order"]`` maps them back).  One launch."""
    sp = plan["points"]
    out = torch.empty(sp.shape[0], device=sp.device) if out is None else out
    clo, cdims = _pc_grid_c(plan["lo"], plan["dims"])
    _hip.check(_hip.lib().umhs_knn_mean_dist(ptr(sp), sp.shape[0], ptr(plan["start"]), clo, float(plan["edge"]), cdims, int(k), ptr(out),
                                             _hip.stream()), "umhs_knn_mean_dist")
    return out


# ---- mesh export (umhs_mesh.hip) ------------------------------------------------------------------------------------------------------
MESH_MAX_POINTS, MESH_MAX_CLASSES = 1 << 28, 16


def mesh_row_bytes(n_classes: int) -> int:
    """Bytes of one vertex row: 15 (x y z, red green blue) or 19 + 4 C (the same, int material, C float abundances)."""
    return 15 if n_classes == 0 else 19 + 4 * int(n_classes)


def tsdf_volume(lo, h: float, dims, n_classes: int, device) -> Dict:
    """An empty volume: lattice points ``lo + (x, y, z) * h``, ``dims`` = (nx, ny, nz), index ``(z * ny + y) * nx + x``.
    -> {"D", "W", "Wc" [N], "A" [3 + 2 C, N] (rgb, abundances, seg_probs planes), "lo", "h", "dims", "n_classes"}."""
    dims = tuple(int(d) for d in dims)
    lo = tuple(float(np.float32(v)) for v in lo)
    h = float(np.float32(h))
    n = dims[0] * dims[1] * dims[2] if len(dims) == 3 else 0
    if len(dims) != 3 or min(dims) < 1 or len(lo) != 3 or not h > 0 or not np.isfinite([*lo, h]).all():
        raise ValueError(f"tsdf_volume: dims {dims}, lo {lo}, h {h}")
    if n > MESH_MAX_POINTS or not 0 <= int(n_classes) <= MESH_MAX_CLASSES:
        raise ValueError(f"tsdf_volume: at most 2^28 lattice points and {MESH_MAX_CLASSES} classes, got {n} and {n_classes}")
    if torch.device(device).type != "cuda":
        raise RuntimeError("tsdf_volume: the volume lives on a HIP device (cuda:N); there is no CPU path")
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
    return {"D": z(n), "W": z(n), "Wc": z(n), "A": z(3 + 2 * int(n_classes), n), "lo": lo, "h": h, "dims": dims, "n_classes": int(n_classes)}


def _tsdf_volume_c(vol: Dict) -> "_hip.TsdfVolume":
    v = _hip.TsdfVolume()
    n = vol["dims"][0] * vol["dims"][1] * vol["dims"][2]
    k = 3 + 2 * vol["n_classes"]
    for name, numel in (("D", n), ("W", n), ("Wc", n), ("A", k * n)):
        t = vol[name]
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
            raise ValueError(f"tsdf: volume[{name!r}] must be a contiguous float32 device tensor of {numel} elements")
        setattr(v, name, t.data_ptr())
    v.dims[:], v.n_attr, v.lo[:], v.h = list(vol["dims"]), k, list(vol["lo"]), vol["h"]
    return v


def _tsdf_image(t, n: int, hgt: int, wid: int, cols: int, what: str, dev):
    """(tensor kept alive, (image, row, pixel) strides in floats) of a float32 [n, H, W(, >= cols)] source read in place."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"tsdf: {what} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32 or t.device != dev:
        raise ValueError(f"tsdf: {what} must be float32 on {dev}, got {t.dtype} on {t.device}")
    img = t.unsqueeze(-1) if t.dim() == 3 else t
    if img.dim() != 4 or tuple(img.shape[:3]) != (n, hgt, wid) or img.shape[3] < cols or (img.shape[3] > 1 and img.stride(3) != 1):
        raise ValueError(f"tsdf: {what} must be [{n}, {hgt}, {wid}, >={cols}] with adjacent channels, got {tuple(t.shape)} strides "
                         f"{tuple(t.stride())}")
    if min(img.stride()[:3]) < 0:
        raise ValueError(f"tsdf: {what} has a negative stride")
    return img, tuple(int(s) for s in img.stride()[:3])


def tsdf_integrate(vol: Dict, c2w, intrinsics, distortion, depth, accumulation, rgb, abundances=None, seg_probs=None,
                   opacity_threshold: float = 0.5, truncation: float = 0.1) -> None:
    """Fuse n rendered cameras into ``vol`` (umhs_tsdf_integrate; the rules are in include/umhs_hip.h).  ``c2w`` [n,3,4],
    ``intrinsics`` [n,4] = (fx, fy, cx, cy), ``distortion`` [n,6] or None: HOST values (numpy or CPU tensors).  ``depth`` /
    ``accumulation`` [n,H,W] or [n,H,W,1], ``rgb`` [n,H,W,3], ``abundances`` / ``seg_probs`` [n,H,W,C]: float32 device tensors read in
    place at their strides.  16 cameras go into one launch; more are fused in consecutive launches (the same bits either way)."""
    c2w = np.asarray(c2w, dtype=np.float32).reshape(-1, 3, 4)
    intr = np.asarray(intrinsics, dtype=np.float32).reshape(-1, 4)
    n = c2w.shape[0]
    dist = None if distortion is None else np.asarray(distortion, dtype=np.float32).reshape(-1, 6)
    if intr.shape[0] != n or (dist is not None and dist.shape[0] != n):
        raise ValueError("tsdf_integrate: c2w, intrinsics and distortion must describe the same cameras")
    if (abundances is None) != (seg_probs is None):
        raise ValueError("tsdf_integrate: abundances and seg_probs come together (or neither)")
    C_ = 0 if abundances is None else int(abundances.shape[-1])
    if C_ != vol["n_classes"] or (C_ and seg_probs.shape[-1] != C_):
        raise ValueError(f"tsdf_integrate: the volume holds {vol['n_classes']} classes, the images {C_}")
    if not (float(truncation) > 0 and np.isfinite(float(truncation))):
        raise ValueError(f"tsdf_integrate: truncation {truncation} must be positive")
    if n == 0:
        return
    v = _tsdf_volume_c(vol)
    dev = vol["D"].device
    if depth.dim() not in (3, 4) or depth.shape[0] != n:
        raise ValueError(f"tsdf_integrate: depth must be [{n}, H, W], got {tuple(depth.shape)}")
    hgt, wid = int(depth.shape[1]), int(depth.shape[2])
    srcs = {}
    for name, t, cols in (("depth", depth, 1), ("accumulation", accumulation, 1), ("rgb", rgb, 3), ("abundances", abundances, C_),
                          ("seg_probs", seg_probs, C_)):
        if t is not None:
            srcs[name] = _tsdf_image(t, n, hgt, wid, cols, name, dev)
    lib = _hip.lib()
    for b in range(0, n, _hip.TSDF_MAX_CAMERAS):
        m = min(_hip.TSDF_MAX_CAMERAS, n - b)
        a = _hip.TsdfImages()
        for name, (img, strides) in srcs.items():
            setattr(a, name, img.data_ptr() + 4 * b * strides[0])
            getattr(a, name + "_strides")[:] = list(strides)
        a.n_cameras, a.height, a.width, a.n_classes = m, hgt, wid, C_
        a.threshold, a.truncation = float(opacity_threshold), float(truncation)
        for j in range(m):
            cam = a.cameras[j]
            cam.rotation[:] = c2w[b + j, :, :3].reshape(-1).tolist()
            cam.origin[:] = c2w[b + j, :, 3].tolist()
            cam.fx, cam.fy, cam.cx, cam.cy = (float(x) for x in intr[b + j])
            if dist is not None and np.any(dist[b + j] != 0):
                cam.distortion[:] = dist[b + j].tolist()
                cam.distorted = 1
        _hip.check(lib.umhs_tsdf_integrate(C.byref(v), C.byref(a), _hip.stream()), "umhs_tsdf_integrate")
    del srcs


def mesh_extract(vol: Dict, world=None, guard_rows: int = 0) -> Dict:
    """Marching tetrahedra over ``vol`` -> {"rows" uint8 [V, row_bytes] (float x y z, uchar red green blue, and with classes int32
    material, float abundances), "faces" int32 [F, 3], "n_classes"}: mark, scan the per-chunk counts (torch), read the two totals
    once (16 bytes) to size the outputs exactly, vertices, triangles.  ``world``: [3,4] host affine for the written xyz.
    ``guard_rows``: that many untouched rows / faces of 0xA5 bytes are kept behind the outputs (tests) and returned as
    ``"rows_buffer"`` / ``"faces_buffer"``."""
    v = _tsdf_volume_c(vol)
    dev = vol["D"].device
    n = vol["dims"][0] * vol["dims"][1] * vol["dims"][2]
    C_ = vol["n_classes"]
    lib = _hip.lib()
    chunks = int(lib.umhs_mesh_chunks(n))
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, chunks, dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_mesh_mark(C.byref(v), ptr(mask), C.c_void_p(counts[0].data_ptr()), C.c_void_p(counts[1].data_ptr()), _hip.stream()),
               "umhs_mesh_mark")
    c64 = counts.to(torch.int64)
    incl = torch.cumsum(c64, 1)
    offsets = (incl - c64).contiguous()
    n_v, n_f = (int(x) for x in incl[:, -1].tolist())  # the one device read
    if n_v >= 1 << 31 or 3 * n_f >= 1 << 33:
        raise RuntimeError(f"mesh_extract: {n_v} vertices / {n_f} faces do not fit int32 indices")
    rb = mesh_row_bytes(C_)
    g = int(guard_rows)
    rows = torch.full(((n_v + g) * rb,), 0xA5, dtype=torch.uint8, device=dev) if g else torch.empty(n_v * rb, dtype=torch.uint8, device=dev)
    faces = (torch.full(((n_f + g) * 3,), -0x5A5A5A5B, dtype=torch.int32, device=dev) if g  # (0xA5A5A5A5 as int32)
             else torch.empty(n_f * 3, dtype=torch.int32, device=dev))
    vbase = torch.empty(n, dtype=torch.int32, device=dev)
    wc = None
    if world is not None:
        Wm = np.asarray(world, dtype=np.float32)
        if Wm.shape != (3, 4):
            raise ValueError("mesh_extract: world = [3,4] affine")
        wc = (_hip._f32 * 12)(*Wm.reshape(-1).tolist())
    _hip.check(lib.umhs_mesh_vertices(C.byref(v), ptr(mask), C.c_void_p(offsets[0].data_ptr()), wc, ptr(vbase),
                                      C.c_void_p(rows.data_ptr()), n_v, _hip.stream()), "umhs_mesh_vertices")
    _hip.check(lib.umhs_mesh_triangles(C.byref(v), ptr(mask), ptr(vbase), C.c_void_p(offsets[1].data_ptr()),
                                       C.c_void_p(faces.data_ptr()), n_f, _hip.stream()), "umhs_mesh_triangles")
    out = {"rows": rows[:n_v * rb].view(n_v, rb), "faces": faces[:n_f * 3].view(n_f, 3), "n_classes": C_}
    if g:
        out["rows_buffer"], out["faces_buffer"] = rows, faces
    return out


# ---- textured mesh export (umhs_texture.hip) -------------------------------------------------------------------------------------------
TEXTURE_MAX_SIDE = 16384  # T <= 16384: 2 T < 2^24 (the vt numerators are exact in float32) and T^2 <= 2^28


def texture_atlas(n_faces: int, px_per_uv_triangle: int = 4):
    """(Q, T) of the per-face atlas (include/umhs_hip.h): two faces per square of ``p`` x ``p`` texels, ``Q`` squares along a side (the
    least integer with ``Q^2 >= ceil(F / 2)``), side ``T = Q p``.  umhs_texture_atlas: host arithmetic, no launch; ``ValueError`` where
    it refuses."""
    F, p = int(n_faces), int(px_per_uv_triangle)
    if p < 4:
        raise ValueError(f"texture_atlas: px_per_uv_triangle {p} must be at least 4 (the 3-texel inset leaves no triangle below)")
    if not 1 <= F < 1 << 62:
        raise ValueError(f"texture_atlas: {F} faces: a mesh without a face has no texture")
    Q, T = _hip._i32(), _hip._i32()
    code = _hip.lib().umhs_texture_atlas(F, p, C.byref(Q), C.byref(T))
    if code == -2:  # UMHS_ERR_UNSUPPORTED
        raise ValueError(f"texture_atlas: {F} faces at {p} texels per triangle side need an atlas above {TEXTURE_MAX_SIDE} x "
                         f"{TEXTURE_MAX_SIDE}: lower --resolution (fewer faces) or --px-per-uv-triangle")
    _hip.check(code, "umhs_texture_atlas")
    return int(Q.value), int(T.value)


def _texture_mesh(positions, faces, what: str):
    if not torch.is_tensor(positions) or not positions.is_cuda or not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError(f"{what}: positions and faces must be tensors on a HIP device (there is no CPU path)")
    if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 3 or not positions.is_contiguous():
        raise ValueError(f"{what}: positions must be a contiguous float32 [V, 3], got {positions.dtype} {tuple(positions.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise ValueError(f"{what}: faces must be a contiguous int32 [F, 3], got {faces.dtype} {tuple(faces.shape)}")
    if faces.device != positions.device:
        raise ValueError(f"{what}: positions on {positions.device}, faces on {faces.device}")
    if positions.shape[0] < 1:
        raise ValueError(f"{what}: a mesh without a vertex has no texture")


def texture_uv(n_faces: int, px_per_uv_triangle: int = 4, device="cuda"):
    """float32 [F, 3, 2]: the ``vt`` of every face corner in the atlas of ``texture_atlas`` (umhs_texture_uv).  One launch."""
    texture_atlas(n_faces, px_per_uv_triangle)
    if torch.device(device).type != "cuda":
        raise RuntimeError("texture_uv: the result lives on a HIP device (cuda:N); there is no CPU path")
    uv = torch.empty(int(n_faces), 3, 2, dtype=torch.float32, device=device)
    with torch.cuda.device(uv.device):
        _hip.check(_hip.lib().umhs_texture_uv(int(n_faces), int(px_per_uv_triangle), ptr(uv), _hip.stream()), "umhs_texture_uv")
    return uv


def texture_rays(positions, faces, px_per_uv_triangle: int, ray_length: float, texel_begin: int = 0, texel_end: Optional[int] = None,
                 want_bary: bool = False, guard: int = 0) -> Dict:
    """The rays of texels [texel_begin, texel_end) of the atlas of ``faces`` int32 [F, 3] over ``positions`` float32 [V, 3]
    (umhs_texture_rays; the rules are in include/umhs_hip.h) -> {"origins", "directions" [n, 3], "nears", "fars" [n, 1], "texel_face"
    int32 [n], "bary" [n, 3] | None}.  A texel nobody owns, or one of a degenerate face or of a face with an index outside [0, V), is a
    miss: ``texel_face`` -1, ``nears = fars = 1e10``.  ``texel_end`` None: the end of the atlas.  ``guard``: that many untouched
    elements (NaN, or int32 0xA5A5A5A5) are kept behind every output (tests) and returned under ``"buffers"``.  One launch, no sync."""
    _texture_mesh(positions, faces, "texture_rays")
    p, L = int(px_per_uv_triangle), float(ray_length)
    _, T = texture_atlas(faces.shape[0], p)
    b, e = int(texel_begin), T * T if texel_end is None else int(texel_end)
    if not 0 <= b <= e <= T * T:
        raise ValueError(f"texture_rays: texels [{b}, {e}) are not a range of the {T} x {T} atlas")
    if not (L > 0 and np.isfinite(np.float32(L))):
        raise ValueError(f"texture_rays: ray_length {ray_length} must be positive and finite")
    n, g, dev = e - b, int(guard), positions.device
    f = lambda cols: torch.full((n * cols + g,), float("nan"), device=dev) if g else torch.empty(n * cols, device=dev)
    bufs = {"origins": f(3), "directions": f(3), "nears": f(1), "fars": f(1), "bary": f(3) if want_bary else None,
            "texel_face": (torch.full((n + g,), -0x5A5A5A5B, dtype=torch.int32, device=dev) if g  # (0xA5A5A5A5 as int32)
                           else torch.empty(n, dtype=torch.int32, device=dev))}
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().umhs_texture_rays(ptr(positions), positions.shape[0], ptr(faces), faces.shape[0], p, L, b, e,
                                                ptr(bufs["origins"]), ptr(bufs["directions"]), ptr(bufs["nears"]), ptr(bufs["fars"]),
                                                ptr(bufs["texel_face"]), ptr(bufs["bary"]), _hip.stream()), "umhs_texture_rays")
    cols = {"origins": 3, "directions": 3, "nears": 1, "fars": 1, "bary": 3}
    out = {k: None if bufs[k] is None else bufs[k][:n * c].view(n, c) for k, c in cols.items()}
    out["texel_face"] = bufs["texel_face"][:n]
    if g:
        out["buffers"] = bufs
    return out


# ---- mesh simplification (umhs_simplify.hip) ------------------------------------------------------------------------------------------
SIMPLIFY_MAX_CLASSES, SIMPLIFY_MAX_CELLS, SIMPLIFY_MAX_AXIS = 15, 1 << 62, (1 << 31) - 1


def simplify_grid_dims(max_coord, origin, edge):
    """(nx, ny, nz) of the clustering grid (include/umhs_hip.h): per axis ``(int)floor((M - g) / e) + 1`` in float32, at least 1, ``M``
    the largest coordinate of the finite vertices (-inf: there is none, one cell).  Host arithmetic; ``ValueError`` for an edge that
    is not positive and finite, an axis of 2^31 cells or more, or a grid of 2^62 cells or more."""
    g, e = np.asarray(origin, dtype=np.float32).reshape(3), np.float32(edge)
    if not (e > 0 and np.isfinite(e) and np.isfinite(g).all()):
        raise ValueError(f"mesh_simplify: origin {g.tolist()} must be finite and edge {float(e)} positive and finite")
    dims = []
    for a in range(3):
        m = np.float32(max_coord[a])
        if np.isnan(m) or m == np.float32(np.inf):
            raise ValueError(f"mesh_simplify: the largest finite coordinate of axis {a} is {float(m)}")
        if m == np.float32(-np.inf):
            dims.append(1)
            continue
        with np.errstate(all="ignore"):
            q = float(np.floor((m - g[a]) / e))  # two rounded float32 operations, as the kernel forms every index
        if not q < SIMPLIFY_MAX_AXIS:
            raise ValueError(f"mesh_simplify: edge {float(e)} gives {q:.4g} cells along axis {a}, at most 2^31 - 1; raise the edge")
        dims.append(max(int(q), 0) + 1)
    if dims[0] * dims[1] * dims[2] >= SIMPLIFY_MAX_CELLS:
        raise ValueError(f"mesh_simplify: edge {float(e)} gives a grid of {dims[0]} x {dims[1]} x {dims[2]} cells, 2^62 or more; raise the edge")
    return tuple(dims)


def _simplify_inputs(rows, faces, n_classes: int):
    C_ = int(n_classes)
    if not torch.is_tensor(rows) or not rows.is_cuda or not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError("mesh_simplify: rows and faces must be tensors on a HIP device (there is no CPU path)")
    if not 0 <= C_ <= SIMPLIFY_MAX_CLASSES:
        raise ValueError(f"mesh_simplify: n_classes {C_} must be in 0..{SIMPLIFY_MAX_CLASSES}")
    rb = mesh_row_bytes(C_)
    if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != rb:
        raise ValueError(f"mesh_simplify: rows must be uint8 [V, {rb}] for {C_} classes, got {rows.dtype} {tuple(rows.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or faces.device != rows.device:
        raise ValueError(f"mesh_simplify: faces must be int32 [F, 3] on {rows.device}, got {faces.dtype} {tuple(faces.shape)} on {faces.device}")
    if rows.shape[0] >= 1 << 31 or faces.shape[0] >= (1 << 31) // 3:
        raise ValueError("mesh_simplify: the mesh does not fit int32 indices")
    return rows.contiguous(), faces.contiguous(), C_, rb


def _flag_ranks(flags):
    """(exclusive rank int32 [n] of the set flags, their number as a 0-dim int64 device tensor): count per chunk (HIP), scan of the chunk
    counts (torch, n / 256 integers), rank (HIP)."""
    n, dev, lib = flags.numel(), flags.device, _hip.lib()
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return rank, torch.zeros((), dtype=torch.int64, device=dev)
    counts = torch.empty(int(lib.umhs_mesh_chunks(n)), dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_simplify_flag_count(ptr(flags), n, ptr(counts), _hip.stream()), "umhs_simplify_flag_count")
    c64 = counts.to(torch.int64)
    incl = torch.cumsum(c64, 0)
    offsets = (incl - c64).contiguous()
    _hip.check(lib.umhs_simplify_flag_rank(ptr(flags), n, ptr(offsets), ptr(rank), _hip.stream()), "umhs_simplify_flag_rank")
    return rank, incl[-1]


def _simplify_faces(rows, faces, rb: int, origin, edge, want_used: bool) -> Dict:
    """The passes the count and the full simplification share, V >= 1 and F >= 1: keys, clusters, face clusters, duplicate removal.
    Reads the extent of the mesh (12 bytes) and, with ``want_used``, the number of clusters (8 bytes)."""
    lib, dev = _hip.lib(), rows.device
    V, F = rows.shape[0], faces.shape[0]
    positions = torch.empty(V, 3, dtype=torch.float32, device=dev)
    chunk_max = torch.empty(int(lib.umhs_mesh_chunks(V)), 3, dtype=torch.float32, device=dev)
    _hip.check(lib.umhs_simplify_unpack(C.c_void_p(rows.data_ptr()), V, rb, ptr(positions), ptr(chunk_max), _hip.stream()),
               "umhs_simplify_unpack")
    dims = simplify_grid_dims(chunk_max.amax(0).tolist(), origin, edge)  # (refuses a grid too large before anything is made on it)
    g = tuple(float(np.float32(v)) for v in np.asarray(origin, dtype=np.float32).reshape(3))
    e = float(np.float32(edge))
    cg, cdims = (_hip._f32 * 3)(*g), (_hip._i32 * 3)(*dims)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    _hip.check(lib.umhs_simplify_keys(ptr(positions), V, cg, e, cdims, ptr(keys), _hip.stream()), "umhs_simplify_keys")
    sorted_keys, order = torch.sort(keys, stable=True)
    head = torch.empty(V, dtype=torch.uint8, device=dev)
    _hip.check(lib.umhs_simplify_heads(ptr(sorted_keys), V, ptr(head), _hip.stream()), "umhs_simplify_heads")
    head_rank, n_clusters = _flag_ranks(head)
    vertex_cluster = torch.empty(V, dtype=torch.int32, device=dev)
    cluster_start = torch.zeros(V + 1, dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_simplify_members(ptr(sorted_keys), ptr(order), ptr(head), ptr(head_rank), V, ptr(vertex_cluster),
                                         ptr(cluster_start), _hip.stream()), "umhs_simplify_members")
    face_cluster = torch.empty(F, 3, dtype=torch.int32, device=dev)
    key_hi = torch.empty(F, dtype=torch.int64, device=dev)
    key_lo = torch.empty(F, dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_simplify_faces(ptr(faces), F, ptr(vertex_cluster), V, ptr(face_cluster), ptr(key_hi), ptr(key_lo), _hip.stream()),
               "umhs_simplify_faces")
    by_lo = torch.sort(key_lo, stable=True).indices  # (c0, c1, c2) lexicographically: the last key first, both sorts stable
    perm = by_lo[torch.sort(key_hi[by_lo], stable=True).indices].contiguous()
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    Nc, used = 0, None
    if want_used:
        Nc = int(n_clusters)
        used = torch.zeros(Nc, dtype=torch.uint8, device=dev)
    _hip.check(lib.umhs_simplify_dedup(ptr(key_hi), ptr(key_lo), ptr(perm), ptr(face_cluster), F, Nc, ptr(keep),
                                       ptr(used) if Nc else None, _hip.stream()), "umhs_simplify_dedup")
    return {"positions": positions, "origin": g, "edge": e, "dims": dims, "order": order, "vertex_cluster": vertex_cluster,
            "cluster_start": cluster_start, "face_cluster": face_cluster, "keep": keep, "used": used, "n_clusters": Nc}


def mesh_simplify_count(rows, faces, n_classes: int, origin, edge: float) -> int:
    """The number of faces ``mesh_simplify`` would keep at this grid: the clustering and the duplicate removal alone, no quadrics, no
    rows.  Reads the extent (12 bytes) and the count (8 bytes)."""
    rows, faces, _, rb = _simplify_inputs(rows, faces, n_classes)
    if rows.shape[0] == 0 or faces.shape[0] == 0:
        simplify_grid_dims((-np.inf,) * 3, origin, edge)
        return 0
    with torch.cuda.device(rows.device):
        st = _simplify_faces(rows, faces, rb, origin, edge, want_used=False)
        lib, F = _hip.lib(), faces.shape[0]
        counts = torch.empty(int(lib.umhs_mesh_chunks(F)), dtype=torch.int32, device=rows.device)
        _hip.check(lib.umhs_simplify_flag_count(ptr(st["keep"]), F, ptr(counts), _hip.stream()), "umhs_simplify_flag_count")
        return int(counts.sum(dtype=torch.int64))


def mesh_simplify(rows, faces, n_classes: int, origin, edge: float, world=None, guard_rows: int = 0) -> Dict:
    """Vertex-clustering simplification of an extracted mesh (include/umhs_hip.h, "Mesh simplification") on the grid of cubic cells of
    ``edge`` from ``origin`` -> {"rows" uint8 [V', row_bytes], "faces" int32 [F', 3], "n_classes", "positions" float32 [V', 3] (model
    frame, before ``world``), "cluster" int32 [V] (the output vertex of every input vertex, or -1)}.  ``rows`` / ``faces`` as
    ``mesh_extract`` returns them (model frame).  ``world``: [3,4] host affine for the written xyz.  ``guard_rows``: as in
    ``mesh_extract``.  Sorts and the scans of chunk counts are torch's; everything per vertex, face or cluster is HIP.  Host reads: the
    extent (12 bytes), the number of clusters (8), the two output sizes (16)."""
    rows, faces, C_, rb = _simplify_inputs(rows, faces, n_classes)
    dev, V, F, g = rows.device, rows.shape[0], faces.shape[0], int(guard_rows)
    wc = None
    if world is not None:
        Wm = np.asarray(world, dtype=np.float32)
        if Wm.shape != (3, 4):
            raise ValueError("mesh_simplify: world = [3,4] affine")
        wc = Wm.reshape(-1).tolist()

    def outputs(n_v, n_f):
        r = torch.full(((n_v + g) * rb,), 0xA5, dtype=torch.uint8, device=dev) if g else torch.empty(n_v * rb, dtype=torch.uint8, device=dev)
        f = (torch.full(((n_f + g) * 3,), -0x5A5A5A5B, dtype=torch.int32, device=dev) if g  # (0xA5A5A5A5 as int32)
             else torch.empty(n_f * 3, dtype=torch.int32, device=dev))
        return r, f

    def result(r, f, n_v, n_f, positions, cluster):
        out = {"rows": r[:n_v * rb].view(n_v, rb), "faces": f[:n_f * 3].view(n_f, 3), "n_classes": C_, "positions": positions,
               "cluster": cluster}
        if g:
            out["rows_buffer"], out["faces_buffer"] = r, f
        return out

    if V == 0 or F == 0:  # no face, nothing kept: no launch
        simplify_grid_dims((-np.inf,) * 3, origin, edge)
        r, f = outputs(0, 0)
        return result(r, f, 0, 0, torch.empty(0, 3, dtype=torch.float32, device=dev), torch.full((V,), -1, dtype=torch.int32, device=dev))
    lib = _hip.lib()
    with torch.cuda.device(dev):
        st = _simplify_faces(rows, faces, rb, origin, edge, want_used=True)
        Nc = st["n_clusters"]
        face_rank, n_f_t = _flag_ranks(st["keep"])
        cluster_rank, n_v_t = _flag_ranks(st["used"]) if Nc else (torch.empty(0, dtype=torch.int32, device=dev), torch.zeros_like(n_f_t))
        n_f, n_v = (int(x) for x in torch.stack([n_f_t, n_v_t]).tolist())
        r, f = outputs(n_v, n_f)
        positions = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        cluster = torch.empty(V, dtype=torch.int32, device=dev)
        if n_v:
            sorted_corner, corner_order = torch.sort(st["face_cluster"].view(-1), stable=True)
            corner_start = torch.searchsorted(sorted_corner, torch.arange(Nc + 1, dtype=torch.int32, device=dev)).to(torch.int32)
            a = _hip.SimplifyArgs()
            for name, t in (("rows", rows), ("positions", st["positions"]), ("faces", faces), ("member_order", st["order"]),
                            ("cluster_start", st["cluster_start"]), ("corner_order", corner_order), ("corner_start", corner_start),
                            ("used", st["used"]), ("cluster_rank", cluster_rank), ("rows_out", r), ("positions_out", positions)):
                setattr(a, name, t.data_ptr())
            a.n_vertices, a.n_faces, a.n_clusters, a.cap, a.n_classes, a.has_world = V, F, Nc, n_v, C_, int(wc is not None)
            a.dims[:], a.origin[:], a.edge = list(st["dims"]), list(st["origin"]), st["edge"]
            if wc is not None:
                a.world[:] = wc
            _hip.check(lib.umhs_simplify_clusters(C.byref(a), _hip.stream()), "umhs_simplify_clusters")
        _hip.check(lib.umhs_simplify_emit(ptr(st["face_cluster"]), ptr(st["keep"]), ptr(face_rank), ptr(st["vertex_cluster"]),
                                          ptr(st["used"]) if Nc else None, ptr(cluster_rank) if Nc else None, F, V, Nc,
                                          C.c_void_p(f.data_ptr()), n_f, ptr(cluster), _hip.stream()), "umhs_simplify_emit")
    return result(r, f, n_v, n_f, positions, cluster)


# ---- mesh components (umhs_components.hip) ----------------------------------------------------------------------------------------------
COMPONENTS_CHUNK = 256  # faces / vertices per workgroup of every kernel of the unit, and the sorted positions of one area piece
COMPONENTS_ROUNDS_PER_READ = 4  # rounds launched between two reads of the changed word (at most 32: one bit each)


def components_round_cap(n_vertices: int) -> int:
    """The hard cap on labelling rounds: V + 1.  After round k every vertex within k faces of its component's smallest vertex carries
    it, so at most V - 1 rounds lower anything and one more sees that nothing falls."""
    return int(n_vertices) + 1


def _components_inputs(rows, faces, n_classes: int, what: str):
    C_ = int(n_classes)
    if not torch.is_tensor(rows) or not rows.is_cuda or not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError(f"{what}: rows and faces must be tensors on a HIP device (there is no CPU path)")
    if not 0 <= C_ <= SIMPLIFY_MAX_CLASSES:
        raise ValueError(f"{what}: n_classes {C_} must be in 0..{SIMPLIFY_MAX_CLASSES}")
    rb = mesh_row_bytes(C_)
    if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != rb:
        raise ValueError(f"{what}: rows must be uint8 [V, {rb}] for {C_} classes, got {rows.dtype} {tuple(rows.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or faces.device != rows.device:
        raise ValueError(f"{what}: faces must be int32 [F, 3] on {rows.device}, got {faces.dtype} {tuple(faces.shape)} on {faces.device}")
    if rows.shape[0] >= 1 << 31 or faces.shape[0] >= (1 << 31) // 3:
        raise ValueError(f"{what}: the mesh does not fit int32 indices")
    return rows.contiguous(), faces.contiguous(), C_, rb


def _components_label(faces, V: int, rounds_per_read: int):
    """(parent int32 [V] with parent[v] = the smallest vertex of v's component, rounds taken).  F >= 1 and V >= 1.  Reads the changed
    word (4 bytes) once per ``rounds_per_read`` rounds."""
    lib, dev, F = _hip.lib(), faces.device, faces.shape[0]
    per, cap = int(rounds_per_read), components_round_cap(V)
    if not 1 <= per <= 32:
        raise ValueError(f"mesh_components: rounds_per_read {per} must be in 1..32 (one bit of the changed word each)")
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_components_init(ptr(parent), V, _hip.stream()), "umhs_components_init")
    rounds = 0
    while rounds < cap:
        n = min(per, cap - rounds)
        if rounds:
            changed.zero_()
        _hip.check(lib.umhs_components_rounds(ptr(faces), F, V, ptr(parent), ptr(changed), n, _hip.stream()), "umhs_components_rounds")
        word = int(changed) & 0xFFFFFFFF  # the device read of this batch: 4 bytes
        for j in range(n):
            if not (word >> j) & 1:  # round j lowered nothing: it saw the final state
                return parent, rounds + j + 1
        rounds += n
    raise RuntimeError(f"mesh_components: the labelling still lowered a parent in round {rounds} of at most {cap} for {V} vertices; no "
                       "result is returned")


def mesh_components(rows, faces, n_classes: int, rounds_per_read: int = COMPONENTS_ROUNDS_PER_READ) -> Dict:
    """The connected components of a mesh (include/umhs_hip.h, "Mesh components") -> {"vertex_component" int32 [V], "face_component"
    int32 [F] (-1: a face with an index outside [0, V)), "n_components" K, "faces" int64 [K], "vertices" int64 [K], "area" float64 [K]
    (in the frame of the rows), "rounds"}.  Component ids number the components by their smallest vertex.  ``rows`` / ``faces`` as
    ``mesh_extract`` returns them.  The two sorts (vertex and face component ids) and the scans of chunk counts are torch's; everything
    per vertex, face or component is HIP.  V = 0 launches nothing; F = 0 labels every vertex its own component without a round.
    Host reads: the changed word (4 bytes) per ``rounds_per_read`` rounds, the number of components (8 bytes)."""
    rows, faces, _, rb = _components_inputs(rows, faces, n_classes, "mesh_components")
    dev, V, F = rows.device, rows.shape[0], faces.shape[0]
    i32 = lambda n, fill=None: (torch.empty(n, dtype=torch.int32, device=dev) if fill is None
                                else torch.full((n,), fill, dtype=torch.int32, device=dev))
    if V == 0:  # no vertex, no component, every face invalid: no launch
        z = lambda dt: torch.zeros(0, dtype=dt, device=dev)
        return {"vertex_component": i32(0), "face_component": i32(F, -1), "n_components": 0, "faces": z(torch.int64),
                "vertices": z(torch.int64), "area": z(torch.float64), "rounds": 0}
    with torch.cuda.device(dev):
        if F:
            parent, rounds = _components_label(faces, V, rounds_per_read)
        else:
            parent, rounds = torch.arange(V, dtype=torch.int32, device=dev), 0
        out = _components_statistics(rows, faces, rb, parent)
    out["rounds"] = rounds
    return out


def _components_statistics(rows, faces, rb: int, parent) -> Dict:
    """Dense ids, counts and areas from the labels of ``_components_label``: everything of ``mesh_components`` but "rounds".  V >= 1.
    Reads the number of components (8 bytes)."""
    lib, dev, V, F = _hip.lib(), rows.device, rows.shape[0], faces.shape[0]
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    root = torch.empty(V, dtype=torch.uint8, device=dev)
    _hip.check(lib.umhs_components_roots(ptr(parent), V, ptr(root), _hip.stream()), "umhs_components_roots")
    root_rank, k_t = _flag_ranks(root)
    K = int(k_t)  # the device read: 8 bytes
    vc, fc = i32(V), i32(F)
    _hip.check(lib.umhs_components_ids(ptr(parent), ptr(root_rank), ptr(faces), F, V, K, ptr(vc), ptr(fc), _hip.stream()),
               "umhs_components_ids")
    n_f = torch.empty(K, dtype=torch.int64, device=dev)
    n_v = torch.empty(K, dtype=torch.int64, device=dev)
    area = torch.empty(K, dtype=torch.float64, device=dev)
    sorted_v = torch.sort(vc).values
    sorted_f = order = face_area = head = first = None
    if F:
        positions = torch.empty(V, 3, dtype=torch.float32, device=dev)
        chunk_max = torch.empty(int(lib.umhs_mesh_chunks(V)), 3, dtype=torch.float32, device=dev)
        _hip.check(lib.umhs_simplify_unpack(C.c_void_p(rows.data_ptr()), V, rb, ptr(positions), ptr(chunk_max), _hip.stream()),
                   "umhs_simplify_unpack")
        face_area = torch.empty(F, dtype=torch.float32, device=dev)
        _hip.check(lib.umhs_components_areas(ptr(positions), V, ptr(faces), F, ptr(face_area), _hip.stream()), "umhs_components_areas")
        sorted_f, order = torch.sort(fc, stable=True)
        head = torch.empty(int(lib.umhs_mesh_chunks(F)), dtype=torch.float64, device=dev)
        first = torch.empty(K, dtype=torch.float64, device=dev)
    _hip.check(lib.umhs_components_stats(ptr(sorted_f), ptr(order), ptr(face_area), F, ptr(sorted_v), V, K, ptr(head), ptr(first),
                                         ptr(n_f), ptr(n_v), ptr(area), _hip.stream()), "umhs_components_stats")
    return {"vertex_component": vc, "face_component": fc, "n_components": K, "faces": n_f, "vertices": n_v, "area": area}


def mesh_keep_components(rows, faces, n_classes: int, components: Dict, keep, world=None, guard_rows: int = 0) -> Dict:
    """The mesh of the kept components (include/umhs_hip.h, "Mesh components") -> {"rows" uint8 [V', row_bytes], "faces" int32 [F', 3],
    "n_classes", "positions" float32 [V', 3] (model frame, before ``world``), "vertex_map" int32 [V] (the output vertex of every input
    vertex, or -1)}.  ``components``: what ``mesh_components`` returned for this mesh; ``keep``: uint8 or bool [K] on the device.  Faces
    and vertices keep their input order; a vertex no emitted face names is dropped; rows are copied byte for byte.  ``world``: [3,4]
    host affine for the written xyz (the rows are in the model frame).  ``guard_rows``: as in ``mesh_extract``.  Host reads: the two
    output sizes (16 bytes)."""
    rows, faces, C_, rb = _components_inputs(rows, faces, n_classes, "mesh_keep_components")
    dev, V, F, g = rows.device, rows.shape[0], faces.shape[0], int(guard_rows)
    K = int(components["n_components"])
    fc = components["face_component"]
    if not torch.is_tensor(keep) or keep.device != dev or keep.dtype not in (torch.uint8, torch.bool) or tuple(keep.shape) != (K,):
        raise ValueError(f"mesh_keep_components: keep must be uint8 or bool [{K}] on {dev}")
    if not torch.is_tensor(fc) or fc.device != dev or fc.dtype != torch.int32 or tuple(fc.shape) != (F,):
        raise ValueError(f"mesh_keep_components: components['face_component'] must be int32 [{F}] on {dev}: the components of this mesh")
    keep = keep.to(torch.uint8).contiguous()
    wc = None
    if world is not None:
        Wm = np.asarray(world, dtype=np.float32)
        if Wm.shape != (3, 4):
            raise ValueError("mesh_keep_components: world = [3,4] affine")
        wc = (_hip._f32 * 12)(*Wm.reshape(-1).tolist())

    def outputs(n_v, n_f):
        r = torch.full(((n_v + g) * rb,), 0xA5, dtype=torch.uint8, device=dev) if g else torch.empty(n_v * rb, dtype=torch.uint8, device=dev)
        f = (torch.full(((n_f + g) * 3,), -0x5A5A5A5B, dtype=torch.int32, device=dev) if g  # (0xA5A5A5A5 as int32)
             else torch.empty(n_f * 3, dtype=torch.int32, device=dev))
        return r, f

    def result(r, f, n_v, n_f, positions, vertex_map):
        out = {"rows": r[:n_v * rb].view(n_v, rb), "faces": f[:n_f * 3].view(n_f, 3), "n_classes": C_, "positions": positions,
               "vertex_map": vertex_map}
        if g:
            out["rows_buffer"], out["faces_buffer"] = r, f
        return out

    if V == 0 or F == 0:  # no face, nothing kept: no launch
        r, f = outputs(0, 0)
        return result(r, f, 0, 0, torch.empty(0, 3, dtype=torch.float32, device=dev), torch.full((V,), -1, dtype=torch.int32, device=dev))
    lib = _hip.lib()
    with torch.cuda.device(dev):
        face_keep = torch.empty(F, dtype=torch.uint8, device=dev)
        used = torch.zeros(V, dtype=torch.uint8, device=dev)
        _hip.check(lib.umhs_components_mark(ptr(faces), ptr(fc.contiguous()), ptr(keep), F, V, K, ptr(face_keep), ptr(used), _hip.stream()),
                   "umhs_components_mark")
        face_rank, n_f_t = _flag_ranks(face_keep)
        vertex_rank, n_v_t = _flag_ranks(used)
        n_f, n_v = (int(x) for x in torch.stack([n_f_t, n_v_t]).tolist())  # the device read: 16 bytes
        r, f = outputs(n_v, n_f)
        positions = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        vertex_map = torch.empty(V, dtype=torch.int32, device=dev)
        _hip.check(lib.umhs_components_emit(C.c_void_p(rows.data_ptr()), rb, ptr(faces), ptr(face_keep), ptr(face_rank), ptr(used),
                                            ptr(vertex_rank), F, V, wc, C.c_void_p(r.data_ptr()), ptr(positions), n_v,
                                            C.c_void_p(f.data_ptr()), n_f, ptr(vertex_map), _hip.stream()), "umhs_components_emit")
    return result(r, f, n_v, n_f, positions, vertex_map)
