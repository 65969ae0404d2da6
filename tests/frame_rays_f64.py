"""Whole-frame ray generation (``umhs_raygen_frame``) restated in torch for float32 and float64 (plain helper module, no tests in it).

Used by tests/test_frame_rays_cpu.py and tests/test_hip_frame_rays.py.

``frame_rays`` is the camera model of include/umhs_hip.h ("umhs_raygen_frame"), i.e. nerfstudio ``Cameras._generate_rays_from_coords``
[upstream-recalled] for the viewer's three camera types: the three image-plane points of a pixel (tests/raygen_f64.py
``image_plane_points``, undistorted by its ``undistort`` for a perspective camera with lens distortion), the camera-frame direction
of each by type, and from there oracle/torch_ref.py ``generate_rays`` op for op.  ``intersect_obb`` is nerfstudio ``intersect_obb`` /
``intersect_aabb``  [upstream-recalled] as that header states it.  nerfstudio is not vendored: parity with upstream is UNPINNED, the
header is the specification.

Every function computes in the dtype of its inputs: float32 is the arithmetic the HIP kernel is held to (same operations in the same
order, up to the device's own sinf / cosf), float64 the truth.

``gpu_cases`` / ``gpu_box``: the frames and crop boxes of the GPU tests, kept here so that the CPU test can assert the precondition
those tests rest on (no ray of them changes between hit and miss from float32 to float64)."""
from __future__ import annotations

import math

import numpy as np
import torch

import raygen_f64 as RG

CAMERA_TYPES = ("perspective", "fisheye", "equirectangular")
MISS = 1e10


def frame_indices(camera: int, H: int, W: int, rows=None) -> torch.Tensor:
    """[R,3] int64 rows (camera, y, x) of a frame (or of its rows ``(row0, n_rows)``) in ray order."""
    row0, n_rows = (0, H) if rows is None else rows
    yy, xx = torch.meshgrid(torch.arange(row0, row0 + n_rows), torch.arange(W), indexing="ij")
    return torch.stack([torch.full_like(yy, camera), yy, xx], -1).reshape(-1, 3).contiguous()


def camera_directions(u: torch.Tensor, v: torch.Tensor, camera_type: str) -> torch.Tensor:
    """Camera-frame direction [...,3] of image-plane points (u, v) (v UP), not normalised."""
    pi = torch.tensor(math.pi, dtype=u.dtype)
    if camera_type == "perspective":
        return torch.stack([u, v, -torch.ones_like(u)], -1)
    if camera_type == "fisheye":
        theta = torch.clamp(torch.sqrt(u * u + v * v), 0.0, math.pi)
        s = torch.where(theta == 0, torch.ones_like(theta), torch.sin(theta) / theta)  # (upstream: 0 / 0 at the principal point)
        return torch.stack([u * s, v * s, -torch.cos(theta)], -1)
    if camera_type == "equirectangular":
        theta, phi = -pi * u, pi * (0.5 - v)
        sp = torch.sin(phi)
        return torch.stack([-torch.sin(theta) * sp, torch.cos(phi), -torch.cos(theta) * sp], -1)
    raise ValueError(camera_type)


def frame_rays(c2w: torch.Tensor, intrinsics: torch.Tensor, camera: int, H: int, W: int, camera_type: str = "perspective",
               distortion=None, rows=None):
    """-> origins [R,3], unit directions [R,3], pixel_area [R,1], directions_norm [R,1] of camera ``camera``'s frame, ray i = pixel
    (i // W, i % W), in the dtype of ``intrinsics``."""
    dt = intrinsics.dtype
    c2w = c2w.to(dt)
    idx = frame_indices(camera, H, W, rows)
    xs, ys = RG.image_plane_points(idx, intrinsics)  # [3,R], y down
    if distortion is not None:
        assert camera_type == "perspective"
        k = distortion.to(dt)[camera]
        if bool((k != 0).any()):
            xs, ys = RG.undistort(xs, ys, k[None, None])
    ds = camera_directions(xs, -ys, camera_type)  # [3,R,3]
    rot = c2w[camera][None, :3, :3]
    ds = torch.sum(ds[..., None, :] * rot, dim=-1)
    nrm = torch.maximum(torch.linalg.vector_norm(ds, dim=-1, keepdim=True), torch.tensor([torch.finfo(torch.float32).eps], dtype=dt))
    ds = ds / nrm
    dx = torch.sqrt(torch.sum((ds[0] - ds[1]) ** 2, dim=-1))
    dy = torch.sqrt(torch.sum((ds[0] - ds[2]) ** 2, dim=-1))
    return c2w[camera][:3, 3].expand(idx.shape[0], 3).contiguous(), ds[0], (dx * dy)[:, None], nrm[0]


def box_frame(p: torch.Tensor, T: torch.Tensor, R: torch.Tensor, point: bool = True) -> torch.Tensor:
    """R^T (p - T) (``point=False``: R^T p) with the kernel's order of operations: ((R0k e0 + R1k e1) + R2k e2)."""
    e = p - T if point else p
    return torch.stack([(R[0, k] * e[..., 0] + R[1, k] * e[..., 1]) + R[2, k] * e[..., 2] for k in range(3)], -1)


def intersect_obb(o: torch.Tensor, d: torch.Tensor, T, R, S, near_floor: float = 0.0):
    """Rays o + t d ([R,3], unit d) against the box (T [3], R [3,3], S [3]) -> nears [R], fars [R], hit [R] bool, gap [R].
    ``gap`` = t_max - t_min after the clamp to [0, 1e10] and BEFORE the miss rule (a hit is gap > 0): how far a ray is from changing
    sides.  A zero component of d' divides to +-inf; fmin / fmax ignore a NaN (0 / 0), as fminf / fmaxf do on the device."""
    dt = o.dtype
    T, R, S = (torch.as_tensor(np.asarray(v)).to(dt) for v in (T, R, S))
    half = S * 0.5
    ob, db = box_frame(o, T, R), box_frame(d, T, R, point=False)
    ta, tb = (-half - ob) / db, (half - ob) / db
    lo, hi = torch.fmin(ta, tb), torch.fmax(ta, tb)
    t_min = torch.fmax(torch.fmax(lo[..., 0], lo[..., 1]), lo[..., 2])
    t_max = torch.fmin(torch.fmin(hi[..., 0], hi[..., 1]), hi[..., 2])
    t_min, t_max = t_min.clamp(0.0, MISS), t_max.clamp(0.0, MISS)
    hit = ~(t_max <= t_min)
    miss = torch.full_like(t_min, MISS)
    nears = torch.where(hit, torch.clamp(t_min, min=near_floor), miss)
    return nears, torch.where(hit, t_max, miss), hit, t_max - t_min


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
BOX_CENTER, BOX_RPY = (0.1, -0.05, 0.2), (0.3, -0.2, 0.5)
BOX_SCALE = {"perspective": (0.9, 0.6, 1.2), "fisheye": (2.4, 1.8, 3.0), "equirectangular": (2.4, 1.8, 3.0)}  # wide cameras: a larger box
N_CAMS = 3


def gpu_box(camera_type: str):
    from umhsnerf.export import obb_from_params

    return obb_from_params(BOX_CENTER, BOX_RPY, BOX_SCALE[camera_type])


def path_cameras(H: int, W: int, fov: float, camera_type: str):
    """c2w [3,3,4], intrinsics [3,4] float32: three cameras at radius 3 looking at the origin (test_hip_distortion._look_at_origin,
    seed 11, the cameras of tests/test_hip_render.py), with ``load_camera_path``'s intrinsics for the type."""
    from test_hip_distortion import _look_at_origin

    rng = np.random.default_rng(11)
    c2w = torch.tensor(np.stack([_look_at_origin(rng)[:3] for _ in range(N_CAMS)]), dtype=torch.float32).contiguous()
    if camera_type == "equirectangular":
        fx, fy = W / 2.0, float(H)
    else:
        fx = fy = (H / 2.0) / math.tan(fov * math.pi / 360.0)
    intr = torch.tensor([[fx, fy, W / 2.0, H / 2.0]], dtype=torch.float32).expand(N_CAMS, 4).contiguous()
    return c2w, intr


def gpu_cases():
    """(camera_type, H, W, fov) of every frame size the GPU tests run: 20 x 28 and the odd 21 x 27 (it has the theta = 0 pixel, and 567
    rays do not fill whole blocks) at fov 50 and 75 for the two pinhole-like types, 16 x 32 for the equirectangular one."""
    return [(t, h, w, fov) for t in ("perspective", "fisheye") for h, w, fov in ((20, 28, 50.0), (21, 27, 75.0))] + [
        ("equirectangular", 16, 32, 0.0)]
