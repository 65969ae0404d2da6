"""Ray generation with OpenCV lens distortion, restated in torch for float32 and float64 (plain helper module, no tests in it).

Used by tests/test_distortion_cpu.py and tests/test_hip_distortion.py.

``generate_rays_distorted`` is oracle/torch_ref.py ``generate_rays`` with the three image-plane points of a ray (the pixel centre, its
+x and its +y neighbour) undistorted first.  The undistortion restates nerfstudio==1.1.5
``camera_utils.radial_and_tangential_undistort``  [upstream-recalled]: nerfstudio's source is not vendored, so the 10 fixed Newton steps,
the analytic Jacobian and the ``|det| > 1e-3`` switch are written from its published behaviour, and their parity with upstream is
UNPINNED.  What does not rest on recollection is ``distort``: the closed-form forward OpenCV model
    r = x^2 + y^2,  d = 1 + r(k1 + r(k2 + r(k3 + r k4)))
    xd = d x + 2 p1 x y + p2 (r + 2 x^2),   yd = d y + 2 p2 x y + p1 (r + 2 y^2)
as OpenCV and COLMAP document it; a round trip through it checks the solve whatever its provenance.

Convention, stated once: the parameters (k1, k2, k3, k4, p1, p2), nerfstudio's order, act on OpenCV image-plane coordinates
``((x - cx) / fx, (y - cy) / fy)`` with y DOWN, which is what they mean in COLMAP and OpenCV.  The solve runs there; the camera frame
has y up, so y is negated AFTER the solve.  With all parameters zero every Newton step is an exact zero and the result is, bit for
bit, the ``-(y - cy) / fy`` of the undistorted generator.

Every function computes in the dtype of ``intrinsics``: float32 gives the arithmetic the HIP kernel is held to, float64 the truth."""
from __future__ import annotations

import torch

DET_EPS, NEWTON_STEPS = 1e-3, 10


def distort(x: torch.Tensor, y: torch.Tensor, k: torch.Tensor):
    """Forward OpenCV model (closed form): ideal image-plane point (y down) -> distorted point.  k [...,6]."""
    k1, k2, k3, k4, p1, p2 = (k[..., i] for i in range(6))
    r = x * x + y * y
    d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    return d * x + 2.0 * p1 * x * y + p2 * (r + 2.0 * x * x), d * y + 2.0 * p2 * x * y + p1 * (r + 2.0 * y * y)


def undistort(xd: torch.Tensor, yd: torch.Tensor, k: torch.Tensor, return_min_det: bool = False):
    """``radial_and_tangential_undistort``  [upstream-recalled]: distorted image-plane point (y down) -> ideal point, by 10 Newton steps
    from (xd, yd); a step is divided by the Jacobian's determinant only where |det| > 1e-3, else it is zero.  ``return_min_det``:
    also the smallest |det| each point met on the way."""
    k1, k2, k3, k4, p1, p2 = (k[..., i] for i in range(6))
    x, y = xd, yd
    min_det = torch.full_like(xd, float("inf"))
    for _ in range(NEWTON_STEPS):
        r = x * x + y * y
        d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        fx = d * x + 2.0 * p1 * x * y + p2 * (r + 2.0 * x * x) - xd
        fy = d * y + 2.0 * p2 * x * y + p1 * (r + 2.0 * y * y) - yd
        d_r = k1 + r * (2.0 * k2 + r * (3.0 * k3 + r * 4.0 * k4))
        d_x, d_y = 2.0 * x * d_r, 2.0 * y * d_r
        fx_x = d + d_x * x + 2.0 * p1 * y + 6.0 * p2 * x
        fx_y = d_y * x + 2.0 * p1 * x + 2.0 * p2 * y
        fy_x = d_x * y + 2.0 * p2 * y + 2.0 * p1 * x
        fy_y = d + d_y * y + 2.0 * p2 * x + 6.0 * p1 * y
        den = fy_x * fx_y - fx_x * fy_y
        xn, yn = fx * fy_y - fy * fx_y, fy * fx_x - fx * fy_x
        ok = den.abs() > DET_EPS
        zero = torch.zeros_like(den)
        x = x + torch.where(ok, xn / den, zero)
        y = y + torch.where(ok, yn / den, zero)
        min_det = torch.minimum(min_det, den.abs())
    return (x, y, min_det) if return_min_det else (x, y)


def image_plane_points(indices: torch.Tensor, intrinsics: torch.Tensor):
    """The three distorted image-plane points of every ray, y down: [3,R] x and y (pixel centre, +x neighbour, +y neighbour)."""
    dt = intrinsics.dtype
    c, y, x = indices[:, 0], indices[:, 1].to(dt) + 0.5, indices[:, 2].to(dt) + 0.5
    fx, fy, cx, cy = (intrinsics[c, i] for i in range(4))
    xs = torch.stack([(x - cx) / fx, (x - cx + 1) / fx, (x - cx) / fx], 0)
    ys = torch.stack([(y - cy) / fy, (y - cy) / fy, (y - cy + 1) / fy], 0)
    return xs, ys


def generate_rays_distorted(indices: torch.Tensor, c2w: torch.Tensor, intrinsics: torch.Tensor, distortion: torch.Tensor,
                            return_min_det: bool = False):
    """indices [R,3] (camera, y, x); c2w [n,3,4]; intrinsics [n,4] = fx, fy, cx, cy; distortion [n,6] = k1, k2, k3, k4, p1, p2.
    -> origins, unit directions, pixel_area [R,1], directions_norm [R,1] (and the smallest |det| of any Newton step of any of the
    three points, [R]) in the dtype of ``intrinsics``.  After the undistortion this is oracle/torch_ref.py generate_rays, op for op."""
    dt = intrinsics.dtype
    c2w, distortion = c2w.to(dt), distortion.to(dt)
    c = indices[:, 0]
    xs, ys = image_plane_points(indices, intrinsics)
    xs, ys, min_det = undistort(xs, ys, distortion[c][None], return_min_det=True)
    cs = torch.stack([xs, -ys], -1)  # [3,R,2], camera frame: y up
    ds = torch.cat([cs, -torch.ones_like(cs[..., :1])], -1)  # [3,R,3]
    rot = c2w[c][:, :3, :3]
    ds = torch.sum(ds[..., None, :] * rot, dim=-1)
    nrm = torch.maximum(torch.linalg.vector_norm(ds, dim=-1, keepdim=True), torch.tensor([torch.finfo(torch.float32).eps], dtype=dt))
    ds = ds / nrm
    dx = torch.sqrt(torch.sum((ds[0] - ds[1]) ** 2, dim=-1))
    dy = torch.sqrt(torch.sum((ds[0] - ds[2]) ** 2, dim=-1))
    out = (c2w[c][:, :3, 3], ds[0], (dx * dy)[:, None], nrm[0])
    return (*out, min_det.min(0).values) if return_min_det else out


def reproject(directions: torch.Tensor, indices: torch.Tensor, c2w: torch.Tensor, intrinsics: torch.Tensor, distortion: torch.Tensor):
    """World directions back to pixel coordinates through the closed-form model, in float64: into the camera frame (by the inverse of
    the pose's 3x3 block), project by (x / -z, y / -z), flip y down, distort, apply the intrinsics.  -> [R,2] (x, y) in pixels; a ray's
    own pixel centre is (x + .5, y + .5)."""
    c = indices[:, 0]
    d, rot, intr, k = directions.double(), c2w.double()[c][:, :3, :3], intrinsics.double()[c], distortion.double()[c]
    cam = torch.linalg.solve(rot, d[:, :, None])[:, :, 0]  # R^-1 d, not R^T d: a float32 rotation is orthonormal to ~1e-7 only
    x, y = cam[:, 0] / -cam[:, 2], -(cam[:, 1] / -cam[:, 2])
    xd, yd = distort(x, y, k)
    return torch.stack([xd * intr[:, 0] + intr[:, 2], yd * intr[:, 1] + intr[:, 3]], -1)


def draw_distortion(n: int, seed: int) -> torch.Tensor:
    """Per-camera parameters from the box the solve was checked on over the whole 640x480 grid at f = 500 (|det| >= 0.45 in every
    Newton step, float64 round trip <= 4e-16): k1 in [-0.15, 0.10], k2 in [-0.03, 0.03], k3 in [-0.005, 0.005], k4 = 0,
    p1, p2 in [-1e-3, 1e-3].  A wider box (k1 = -0.3 with k2 = -0.1) folds the model inside the image and Newton diverges."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 6, generator=g)
    lo = torch.tensor([-0.15, -0.03, -0.005, 0.0, -1e-3, -1e-3])
    hi = torch.tensor([0.10, 0.03, 0.005, 0.0, 1e-3, 1e-3])
    return (lo + u * (hi - lo)).contiguous()
