"""Data-side operators, run at load or once per batch / frame: pixel sampler, mask lists, ray generation, pixel gather."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _hip
from .._hip import ptr


def pixel_indices(uniform, n_images: int, height: int, width: int):
    """PixelSampler.sample_method: long(uniform[R,3] * (n, H, W)) -> [R,3] int64 rows (camera, y, x)."""
    u = _hip.f32c(uniform)
    out = torch.empty(u.shape, dtype=torch.int64, device=u.device)
    _hip.check(_hip.lib().umhs_pixel_indices(ptr(u), u.shape[0], n_images, height, width, ptr(out), _hip.stream()), "umhs_pixel_indices")
    return out


def mask_lists(mask_stack, device=None):
    """Set pixels of a uint8 mask stack [n,H,W] (set: byte != 0) -> (off [n+1] int64, list [M] int32), both on the device:
    ``off`` is the exclusive prefix sum of the per-image counts (M = off[n]) and ``list`` holds the flat ids y*W + x of the set
    pixels, ascending within an image, images in order -- the second column of ``torch.nonzero(mask.view(n, -1))``.  A stack in host
    memory (``device``: where the lists go) is uploaded one frame at a time and ends with the same bits.  Runs once per split, at
    load: it reads M back to size the list."""
    if mask_stack.dim() != 3 or mask_stack.dtype != torch.uint8:
        raise ValueError(f"mask stack must be uint8 [n,H,W], got {mask_stack.dtype} {tuple(mask_stack.shape)}")
    n, h, w = mask_stack.shape
    resident = mask_stack.is_cuda
    dev = mask_stack.device if resident else torch.device("cuda" if device is None else device)
    if n == 0 or h * w == 0:
        return torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    lib, pixels = _hip.lib(), h * w
    cpi = int(lib.umhs_mask_chunks(pixels))
    counts = torch.zeros((n, cpi), dtype=torch.int32, device=dev)
    if resident:
        pieces = [(mask_stack.contiguous(), 0, n)]
    else:  # one frame on the device at a time, in ONE buffer: both passes see the same address (the chunks depend on its alignment)
        frame = torch.empty((1, h, w), dtype=torch.uint8, device=dev)
        pieces = [(frame, i, 1) for i in range(n)]

    def each_piece():
        for buf, first, k in pieces:
            if not resident:
                buf.copy_(mask_stack[first : first + 1])
            yield buf, first, k

    for buf, first, k in each_piece():
        _hip.check(lib.umhs_mask_count(ptr(buf), k, pixels, ptr(counts[first : first + k]), _hip.stream()), "umhs_mask_count")
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(counts.sum(1, dtype=torch.int64), 0)
    flat = counts.view(-1).to(torch.int64)
    chunk_off = (torch.cumsum(flat, 0) - flat).view(n, cpi)  # exclusive scan: where each chunk's ids start in the whole list
    total = int(off[-1])
    lst = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        for buf, first, k in each_piece():
            _hip.check(lib.umhs_mask_compact(ptr(buf), k, pixels, ptr(chunk_off[first : first + k]), ptr(lst), total, _hip.stream()),
                       "umhs_mask_compact")
    return off, lst


def pixel_indices_masked(uniform, off, lst, width: int):
    """The mask-aware draw: rows (image, y, x) int64 [R,3], uniform over the set pixels ``mask_lists`` compacted, with replacement,
    from the same uniform[R,3] block ``pixel_indices`` takes (column 0 picks the image through ``off``, column 1 the rank within
    it, column 2 is unused).  No host sync."""
    u = _hip.f32c(uniform)
    if off.dtype != torch.int64 or lst.dtype != torch.int32 or off.dim() != 1 or off.shape[0] < 2:
        raise ValueError(f"off must be int64 [n+1] and list int32 [M], got {off.dtype} {tuple(off.shape)} / {lst.dtype} {tuple(lst.shape)}")
    out = torch.empty(u.shape, dtype=torch.int64, device=u.device)
    if u.shape[0] and not lst.numel():
        raise ValueError("the mask list is empty: no pixel to draw")
    _hip.check(_hip.lib().umhs_pixel_indices_masked(ptr(u), u.shape[0], off.shape[0] - 1, width, ptr(off), ptr(lst), ptr(out),
                                                    _hip.stream()), "umhs_pixel_indices_masked")
    return out


def raygen(indices, c2w, intrinsics, want_area: bool = True, want_norm: bool = False, distortion=None):
    """Cameras.generate_rays for perspective cameras: -> origins [R,3], directions [R,3], pixel_area [R,1] | None, norm | None.
    ``distortion`` [n,6] = (k1, k2, k3, k4, p1, p2) per camera: OpenCV lens distortion, undone per ray by ``umhs_raygen_distorted``."""
    r, dev = indices.shape[0], indices.device
    o, d = torch.empty(r, 3, device=dev), torch.empty(r, 3, device=dev)
    area = torch.empty(r, 1, device=dev) if want_area else None
    nrm = torch.empty(r, 1, device=dev) if want_norm else None
    if distortion is None:
        _hip.check(_hip.lib().umhs_raygen(ptr(indices), ptr(c2w), ptr(intrinsics), r, c2w.shape[0], ptr(o), ptr(d), ptr(area), ptr(nrm),
                                          _hip.stream()), "umhs_raygen")
        return o, d, area, nrm
    if distortion.shape != (c2w.shape[0], 6) or distortion.dtype != torch.float32:
        raise ValueError(f"distortion must be float32 [{c2w.shape[0]}, 6] (k1, k2, k3, k4, p1, p2), got {distortion.dtype} {tuple(distortion.shape)}")
    _hip.check(_hip.lib().umhs_raygen_distorted(ptr(indices), ptr(c2w), ptr(intrinsics), ptr(distortion), r, c2w.shape[0], ptr(o), ptr(d),
                                                ptr(area), ptr(nrm), _hip.stream()), "umhs_raygen_distorted")
    return o, d, area, nrm


CAMERA_TYPES = {"perspective": 0, "fisheye": 1, "equirectangular": 2}  # umhs_raygen_frame's camera_type


def obb_host15(obb):
    """(T [3], R [3,3], S [3]) -- the box of ``export.obb_from_params`` -- as the 15 host floats the C boundary takes."""
    T, R, S = (np.asarray(torch.as_tensor(v).detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32) for v in obb)
    if T.size != 3 or R.shape != (3, 3) or S.size != 3:
        raise ValueError(f"a box is (T [3], R [3,3], S [3]), got shapes {T.shape}, {R.shape}, {S.shape}")
    if not bool((S > 0).all()):
        raise ValueError(f"the scale of a box must be positive, got {S.reshape(-1).tolist()}")
    return (_hip._f32 * 15)(*T.reshape(-1).tolist(), *R.reshape(-1).tolist(), *S.reshape(-1).tolist())


def raygen_frame(c2w, intrinsics, camera: int, height: int, width: int, camera_type: str = "perspective", distortion=None, obb=None,
                 near_floor: float = 0.0, rows: Optional[Tuple[int, int]] = None):
    """The rays of one camera's frame -- or of its rows ``rows = (row0, n_rows)`` -- in one launch of ``umhs_raygen_frame``, no index
    tensor: ray i is pixel (row0 + i // width, i % width).  ``camera_type``: perspective (``distortion`` [n,6] as in ``raygen``: the same
    bits as ``raygen`` on meshgrid indices), fisheye or equirectangular.  ``obb`` = (T, R, S): a crop box, intersected per ray;
    ``near_floor`` is the least ``nears`` of a hit.
    -> origins [R,3], directions [R,3], pixel_area [R,1], directions_norm [R,1], nears [R,1] | None, fars [R,1] | None."""
    if camera_type not in CAMERA_TYPES:
        raise ValueError(f"camera_type {camera_type!r}: one of {', '.join(CAMERA_TYPES)}")
    n, dev = c2w.shape[0], c2w.device
    row0, n_rows = (0, int(height)) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= int(camera) < n:
        raise IndexError(f"camera index {camera} outside 0..{n - 1}")
    if height < 1 or width < 1 or row0 < 0 or n_rows < 0 or row0 + n_rows > height:
        raise ValueError(f"rows {row0}..{row0 + n_rows} outside a frame of {height} x {width}")
    if distortion is not None:
        if camera_type != "perspective":
            raise ValueError(f"lens distortion belongs to perspective cameras, not to {camera_type}")
        if distortion.shape != (n, 6) or distortion.dtype != torch.float32:
            raise ValueError(f"distortion must be float32 [{n}, 6] (k1, k2, k3, k4, p1, p2), got {distortion.dtype} {tuple(distortion.shape)}")
    if not near_floor >= 0:
        raise ValueError(f"near_floor must not be negative, got {near_floor}")
    box = None if obb is None else obb_host15(obb)
    r = n_rows * int(width)
    o, d = torch.empty(r, 3, device=dev), torch.empty(r, 3, device=dev)
    area, nrm = torch.empty(r, 1, device=dev), torch.empty(r, 1, device=dev)
    nears, fars = (torch.empty(r, 1, device=dev), torch.empty(r, 1, device=dev)) if box is not None else (None, None)
    if r == 0:  # no row: nothing to launch (an empty tensor has no address to hand over)
        return o, d, area, nrm, nears, fars
    _hip.check(_hip.lib().umhs_raygen_frame(ptr(_hip.f32c(c2w)), ptr(_hip.f32c(intrinsics)), ptr(distortion), n, int(camera),
                                            CAMERA_TYPES[camera_type], int(height), int(width), row0, n_rows, box, float(near_floor), ptr(o),
                                            ptr(d), ptr(area), ptr(nrm), ptr(nears), ptr(fars), _hip.stream()), "umhs_raygen_frame")
    return o, d, area, nrm, nears, fars


def pixel_gather(indices, stack):
    """batch[key] = stack[c, y, x] for a resident image stack [n,H,W,K] (fp32, or uint8 -> /255)."""
    assert stack.dim() == 4 and stack.is_contiguous() and stack.dtype in (torch.float32, torch.uint8)
    n, h, w, k = stack.shape
    out = torch.empty(indices.shape[0], k, device=indices.device)
    _hip.check(_hip.lib().umhs_pixel_gather(ptr(indices), ptr(stack), int(stack.dtype == torch.uint8), n, h, w, k, indices.shape[0],
                                            ptr(out), _hip.stream()), "umhs_pixel_gather")
    return out
