"""``python -m umhsnerf.render camera-path --data DIR --checkpoint FILE --camera-path-filename FILE --output-path DIR
--rendered-output-names rgb abundances_0 ...``: what ``ns-render camera-path`` does for a trained model (the reference's
scripts/render.sh: the abundance-map, per-band and residual fly-throughs), without nerfstudio.

A camera-path file (the viewer's export) becomes ``Cameras`` -- perspective, fisheye or equirectangular (360 degrees), with the viewer's
``crop`` box if it has one; every camera is rendered with the fused, chunked ``get_outputs_for_camera_ray_bundle`` on the rays of the
whole-frame ray kernel (``ops.raygen_frame``: no index tensor; a crop box becomes per-ray ``nears`` / ``fars`` there, and ``rgb`` is
composited over the crop's background colour), the named outputs are composed side by side into one uint8 frame ON THE DEVICE
(``ops.frame_compose``: colormaps, depth blending and quantisation in one launch, sources read in place -- ``wv_7`` is column 7 of
``spectral``, no column is copied), and only those 3 bytes per pixel and panel travel to the host, where a small thread pool encodes and
writes ``frame_<i:05d>.png`` / ``.jpg``.  ``--cube-output-names spectral abundances`` additionally writes the float32 cubes
``<name>_<i:05d>.npy`` -- the hyperspectral image of a novel view.

``dataset --split train|val|test|train+test`` renders every camera of a split at its own pose and intrinsics into
``OUT/<split>/<output name>/<image stem>.png`` (``ns-render dataset``'s layout, one panel per file); ``interpolate --pose-source
eval|train --interpolation-steps N`` renders N poses between consecutive cameras of a split (``ns-render interpolate``: quaternion slerp
of the rotation, linear blend of translation and intrinsics, both ends of every pair included) as a camera path.

``--output-format video --output-path NAME.avi`` writes the frames as Motion-JPEG instead (``utils/mjpeg_avi.py``): every composed
frame is encoded to baseline JPEG on the device (``ops.jpeg_encode``) and only its compressed bytes travel to the host;
``--jpeg-encoder gpu`` does the same for ``--image-format jpeg`` files, ``--png-encoder gpu`` (``ops.png_encode``, lossless) for
``--image-format png`` files.  ``ffmpeg -i NAME.avi -c:v libx264 -pix_fmt yuv420p NAME.mp4``
makes an mp4 of the file.

Not built: mp4 / H.264 output, camera paths of type ``omnidirectional`` / ``vr180`` (and orthographic cameras), ``ns-render spiral``, ``interpolate
--order-poses true``.

Names: an output with 3 channels is shown as it is (``rgb``, ``seg_pred``), one with 1 channel through a colormap (``accumulation``,
``seg_raw``), ``wv_i`` / ``abundances_i`` / ``residual_i`` are columns of ``spectral`` / ``abundances`` / ``specular``, and any name that
contains ``depth`` goes through nerfstudio's depth colormap: normalised by the frame's own (min, max) -- taken on the device -- or by the
planes given, and blended over white with ``accumulation``."""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import re
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .data.umhs_dataparser import Cameras

_COLUMNS = {"wv": "spectral", "abundances": "abundances", "residual": "specular"}
_COLUMN_NAME = re.compile(r"^(wv|abundances|residual)_(\d+)$")
MAX_PANELS = 16          # panels of one umhs_frame_compose launch
MAX_ENCODERS = 4         # encoder / writer threads
MAX_FRAMES_IN_FLIGHT = 16  # frames handed to the pool and not yet written: beyond it the loop waits instead of growing without limit


@dataclass
class ColormapOptions:
    """nerfstudio's ``colormaps.ColormapOptions``  [upstream-recalled]."""
    colormap: str = "default"
    normalize: bool = False
    colormap_min: float = 0.0
    colormap_max: float = 1.0
    invert: bool = False


# ---- camera paths ----------------------------------------------------------------------------------------------------------------
CAMERA_TYPES = ("perspective", "fisheye", "equirectangular")  # what the frame-ray kernel makes rays for


def _vec3(crop: dict, key: str, default=None) -> List[float]:
    v = crop.get(key, default)
    try:
        out = [float(x) for x in v]
    except (TypeError, ValueError):
        out = []
    if len(out) != 3 or not all(math.isfinite(x) for x in out):
        raise ValueError(f"crop: {key} must hold 3 finite numbers, got {v!r}")
    return out


def parse_crop(crop: dict) -> dict:
    """The viewer's ``crop`` entry -> {"obb": ``export.obb_from_params(crop_center, crop_rot, crop_scale)``, "background_color":
    [r, g, b] / 255}, as nerfstudio's ``get_crop_from_json`` reads it  [upstream-recalled].  ``crop_rot`` (Euler angles, radians) may be
    missing: zeros.  A malformed entry is a ``ValueError`` that names the field."""
    from .export import obb_from_params

    if not isinstance(crop, dict):
        raise ValueError(f"crop must be an object with crop_center, crop_scale and crop_bg_color, got {type(crop).__name__}")
    center, scale = _vec3(crop, "crop_center"), _vec3(crop, "crop_scale")
    rot = _vec3(crop, "crop_rot", (0.0, 0.0, 0.0))
    if not all(x > 0 for x in scale):
        raise ValueError(f"crop: crop_scale must be positive on every axis, got {scale}")
    bg = crop.get("crop_bg_color")
    if not isinstance(bg, dict) or any(k not in bg for k in "rgb"):
        raise ValueError(f"crop: crop_bg_color must be an object with r, g and b (0..255), got {bg!r}")
    try:
        colour = [float(bg[k]) / 255.0 for k in "rgb"]
    except (TypeError, ValueError):
        colour = [math.nan]
    if not all(0.0 <= c <= 1.0 for c in colour):
        raise ValueError(f"crop: crop_bg_color must hold r, g and b in 0..255, got {bg!r}")
    return {"obb": obb_from_params(center, rot, scale), "background_color": colour}


def load_camera_path(json_or_path: Union[dict, str, Path], downscale_factor: float = 1.0, device=None,
                     camera_types: Sequence[str] = ("perspective",), crop: bool = False) -> Tuple[Cameras, dict]:
    """nerfstudio ``camera_utils.get_path_from_json`` followed by ``Cameras.rescale_output_resolution(1 / downscale_factor)``, as
    ``ns-render camera-path`` calls them  [upstream-recalled]: nerfstudio's source is not vendored, so the rules are restated here.

    ``render_height`` x ``render_width`` frames; per entry of ``camera_path``: ``camera_to_world``, 16 row-major floats of which rows 0..2
    are used AS THEY ARE (a viewer path is in the model's coordinates already), and ``fov`` in degrees (vertical).  ``camera_type``
    ``perspective`` (the default) and ``fisheye``: ``fx = fy = (H / 2) / tan(fov * pi / 360)``, ``cx = W / 2``, ``cy = H / 2``;
    ``equirectangular``: ``fx = W / 2``, ``fy = H``, the same principal point, ``fov`` ignored; ``aspect`` is always ignored.  Other types
    (``omnidirectional``, ``vr180``) are refused by name.  ``downscale_factor`` d: the intrinsics are multiplied by 1 / d and the size
    becomes ``int(H / d)`` x ``int(W / d)``.  A ``crop`` entry is read by ``parse_crop``.

    What the CALLER can do with the result is said by the caller: ``camera_types`` are the types it renders (``CAMERA_TYPES`` for one
    that makes its rays with ``Cameras.generate_rays``) and ``crop=True`` says that it passes ``meta["crop"]`` on to
    ``render_camera_path``.  The defaults are the contract this function always had -- perspective paths without a crop, anything
    else a ``NotImplementedError`` -- so a caller written against it is refused loudly instead of being handed a fisheye path as if
    it were perspective, or rendering a cropped path whole.  The command line passes both.
    -> (Cameras, {"num_frames", "render_height", "render_width", "fps", "seconds", "camera_type", "crop": None | {"obb",
    "background_color"}})."""
    if isinstance(json_or_path, dict):
        path = json_or_path
    else:
        with open(json_or_path) as f:
            path = json.load(f)
    camera_type = str(path.get("camera_type", "perspective")).lower()
    if camera_type not in CAMERA_TYPES:
        raise NotImplementedError(f"camera_type {camera_type!r}: camera paths are rendered for {', '.join(CAMERA_TYPES)} cameras only")
    if camera_type not in camera_types:
        raise NotImplementedError(f"camera_type {camera_type!r}: this caller takes {', '.join(camera_types)} camera paths only "
                                  f"(load_camera_path(..., camera_types=CAMERA_TYPES) reads it)")
    if path.get("crop") is not None and not crop:
        raise NotImplementedError("the camera path has a crop box and this caller does not render one (load_camera_path(..., crop=True) "
                                  "reads it into meta[\"crop\"] for render_camera_path(..., crop=))")
    crop = None if path.get("crop") is None else parse_crop(path["crop"])
    entries = path.get("camera_path") or []
    if len(entries) == 0:
        raise ValueError("the camera path holds no camera")
    if not downscale_factor > 0:
        raise ValueError(f"downscale_factor must be positive, got {downscale_factor}")
    H, W = int(path["render_height"]), int(path["render_width"])
    c2w, fxs, fys = [], [], []
    for k, cam in enumerate(entries):
        m = [float(v) for v in cam["camera_to_world"]]
        if len(m) != 16:
            raise ValueError(f"camera {k}: camera_to_world must hold 16 values, got {len(m)}")
        c2w.append(m[:12])
        if camera_type == "equirectangular":
            fxs.append(W / 2.0), fys.append(float(H))
        else:
            focal = (H / 2.0) / math.tan(float(cam["fov"]) * math.pi / 360.0)
            fxs.append(focal), fys.append(focal)
    s = 1.0 / float(downscale_factor)
    n = len(entries)
    fx, fy = torch.tensor(fxs, dtype=torch.float64) * s, torch.tensor(fys, dtype=torch.float64) * s
    cameras = Cameras(torch.tensor(c2w, dtype=torch.float32).view(n, 3, 4), fx.float(), fy.float(),
                      torch.full((n,), (W / 2.0) * s, dtype=torch.float32), torch.full((n,), (H / 2.0) * s, dtype=torch.float32),
                      int(H / downscale_factor), int(W / downscale_factor), camera_type=camera_type)
    if cameras.height < 1 or cameras.width < 1:
        raise ValueError(f"downscale_factor {downscale_factor} leaves no pixel of {H} x {W}")
    meta = {"num_frames": n, "render_height": cameras.height, "render_width": cameras.width, "fps": path.get("fps"),
            "seconds": path.get("seconds"), "camera_type": camera_type, "crop": crop}
    return (cameras if device is None else cameras.to(device)), meta


# ---- interpolated poses (host, float64) --------------------------------------------------------------------------------------------
def _quaternion(R: np.ndarray) -> np.ndarray:
    """Unit quaternion (w, x, y, z) of a rotation matrix, by the branch with the largest pivot (Shepperd)."""
    t = np.trace(R)
    if t > 0:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        q = np.empty(4)
        q[0], q[1 + i], q[1 + j], q[1 + k] = R[k, j] - R[j, k], 1.0 + R[i, i] - R[j, j] - R[k, k], R[j, i] + R[i, j], R[k, i] + R[i, k]
    return q / np.linalg.norm(q)


def _rotation(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def interpolate_poses(c2w, steps: int) -> np.ndarray:
    """nerfstudio ``get_interpolated_poses_many``  [upstream-recalled]: between consecutive poses of ``c2w`` [n,3,4], ``steps`` poses at
    ``linspace(0, 1, steps)`` -- quaternion slerp (the short way round) of the rotation, linear blend of the translation; both ends of
    every pair are included (and are the inputs themselves), so joints repeat.  float64 on the host -> [(n - 1) * steps, 3, 4]."""
    c2w = np.asarray(c2w, dtype=np.float64).reshape(-1, 3, 4)
    if len(c2w) < 2:
        raise ValueError(f"interpolation needs at least two cameras, got {len(c2w)}")
    if int(steps) < 2:
        raise ValueError(f"interpolation_steps must be at least 2 (both ends of a pair are rendered), got {steps}")
    out = []
    for a, b in zip(c2w[:-1], c2w[1:]):
        qa, qb = _quaternion(a[:, :3]), _quaternion(b[:, :3])
        dot = float(np.dot(qa, qb))
        if dot < 0:
            qb, dot = -qb, -dot
        omega = math.acos(min(dot, 1.0))
        for t in np.linspace(0.0, 1.0, int(steps)):
            if t == 0.0 or t == 1.0:
                out.append((a if t == 0.0 else b).copy())
                continue
            if omega < 1e-8:  # (nearly) the same rotation: the blend is the limit of the formula
                q = (1 - t) * qa + t * qb
            else:
                q = (math.sin((1 - t) * omega) * qa + math.sin(t * omega) * qb) / math.sin(omega)
            out.append(np.concatenate([_rotation(q), ((1 - t) * a[:, 3] + t * b[:, 3])[:, None]], axis=1))
    return np.stack(out)


def interpolate_cameras(cameras: Cameras, steps: int) -> Cameras:
    """``steps`` cameras per consecutive pair of ``cameras`` (``interpolate_poses``), the intrinsics -- and the lens distortion, if the
    cameras carry one -- blended linearly with the same weights.  On the host, float64; the result is float32 on the CPU."""
    n, steps = len(cameras), int(steps)
    poses = interpolate_poses(cameras.camera_to_worlds.detach().cpu().double().numpy(), steps)
    w = torch.linspace(0.0, 1.0, steps, dtype=torch.float64)

    def blend(v):
        v = v.detach().cpu().double()
        a, b = v[:-1, None], v[1:, None]
        wt = w.view(1, steps, *([1] * (v.dim() - 1)))
        mixed = (1 - wt) * a + wt * b
        return mixed.reshape((n - 1) * steps, *v.shape[1:]).float()

    dist = None if cameras.distortion_params is None else blend(cameras.distortion_params).contiguous()
    return Cameras(torch.from_numpy(poses).float().contiguous(), blend(cameras.fx), blend(cameras.fy), blend(cameras.cx), blend(cameras.cy),
                   cameras.height, cameras.width, dist, cameras.camera_type)


# ---- names -> panels ---------------------------------------------------------------------------------------------------------------
def _showable(t) -> bool:
    return torch.is_tensor(t) and t.is_floating_point() and t.dim() >= 1 and t.shape[-1] in (1, 3)


def usable_output_names(outputs: Dict[str, torch.Tensor]) -> List[str]:
    """What ``compose_frame`` can show of an output dict: the 1- and 3-channel float entries, and the columns of the band tensors."""
    names = [k for k, v in outputs.items() if _showable(v) and not _COLUMN_NAME.match(k)]
    for prefix, base in _COLUMNS.items():
        if torch.is_tensor(outputs.get(base)) and outputs[base].is_floating_point():
            c = outputs[base].shape[-1]
            names.append(f"{prefix}_0" if c == 1 else f"{prefix}_0..{prefix}_{c - 1}")
    return names


def source_keys(names: Sequence[str], cube_names: Sequence[str] = ()) -> List[str]:
    """The entries of the output dict a render of ``names`` reads: the base tensors only (``wv_3`` -> ``spectral``), plus
    ``accumulation`` when a depth panel is blended with it."""
    keys: List[str] = []
    for name in [*names, *cube_names]:
        m = _COLUMN_NAME.match(name)
        keys.append(_COLUMNS[m.group(1)] if m else name)
        if "depth" in name:
            keys.append("accumulation")
    return list(dict.fromkeys(keys))


def resolve_output(outputs: Dict[str, torch.Tensor], name: str):
    """-> (tensor [..., c], first channel, kind) of one rendered output name; ``ValueError`` that lists the usable names otherwise."""
    from . import ops

    m = _COLUMN_NAME.match(name)
    if m and torch.is_tensor(outputs.get(_COLUMNS[m.group(1)])):
        base, i = outputs[_COLUMNS[m.group(1)]], int(m.group(2))
        if base.is_floating_point() and i < base.shape[-1]:
            return base, i, ops.PANEL_SCALAR
    if name in outputs and torch.is_tensor(outputs[name]) and outputs[name].is_floating_point():
        t = outputs[name]
        c = t.shape[-1] if t.dim() else 0
        if c == 3 and "depth" not in name:
            return t, 0, ops.PANEL_RGB
        if c == 1:
            return t, 0, ops.PANEL_DEPTH if "depth" in name else ops.PANEL_SCALAR
        raise ValueError(f"output {name!r} has {c} channels: only 1 (colormap) or 3 (shown as it is) can be rendered "
                         f"(nerfstudio would project it by PCA); usable names: {', '.join(usable_output_names(outputs))}")
    raise ValueError(f"no output named {name!r}; usable names: {', '.join(usable_output_names(outputs))}")


def compose_frame(outputs: Dict[str, torch.Tensor], names: Sequence[str], colormap_options: Optional[ColormapOptions] = None,
                  depth_near_plane: Optional[float] = None, depth_far_plane: Optional[float] = None, out=None) -> torch.Tensor:
    """uint8 [H, K * W, 3]: the K named outputs of one camera ([H, W, c] tensors on the device) side by side, as nerfstudio's render
    loop shows them (``apply_colormap`` per output, ``np.concatenate(axis=1)``) -- one launch of ``ops.frame_compose`` per 16 panels,
    no host sync."""
    from . import ops
    from .utils import colormaps

    opt = colormap_options or ColormapOptions()
    names = list(names)
    if len(names) < 1:
        raise ValueError("no rendered output name: a frame holds at least one panel")
    resolved = [resolve_output(outputs, name) for name in names]
    first = resolved[0][0]
    if first.dim() != 3:
        raise ValueError(f"outputs must be [H, W, c] images, got {tuple(first.shape)} for {names[0]!r}")
    H, W = first.shape[:2]
    panels = []
    for name, (t, ch, kind) in zip(names, resolved):
        if tuple(t.shape[:2]) != (H, W) or t.dim() != 3:
            raise ValueError(f"output {name!r} is {tuple(t.shape)}, the frame {H} x {W}")
        t = t if t.dtype == torch.float32 else t.float()
        p = ops.FramePanel(t, kind, ch, normalize=opt.normalize, invert=opt.invert, cmin=opt.colormap_min, cmax=opt.colormap_max)
        if kind == ops.PANEL_DEPTH:
            lo, hi = (None, None) if depth_near_plane is not None and depth_far_plane is not None else torch.aminmax(t)
            lo = lo if depth_near_plane is None else torch.full((), float(depth_near_plane), device=t.device)
            hi = hi if depth_far_plane is None else torch.full((), float(depth_far_plane), device=t.device)
            p.range = torch.stack([lo.float(), hi.float()])
            acc = outputs.get("accumulation")
            p.accumulation = None if acc is None else acc.float().contiguous().view(-1)
            p.normalize = False
        elif kind == ops.PANEL_SCALAR and opt.normalize:
            p.range = torch.stack(torch.aminmax(t[..., ch])).float()
        panels.append(p)
    lut = colormaps.device_table(opt.colormap, first.device)
    if len(panels) <= MAX_PANELS:
        return ops.frame_compose(panels, lut, H, W, out=out)
    # more panels than one launch takes (wv_0 .. wv_20): groups of 16 composed apart and joined, one strided copy per group
    parts = [ops.frame_compose(panels[k:k + MAX_PANELS], lut, H, W) for k in range(0, len(panels), MAX_PANELS)]
    if out is None:
        return torch.cat(parts, dim=1)
    if out.dtype != torch.uint8 or out.numel() != 3 * H * W * len(panels) or not out.is_contiguous():
        raise ValueError(f"out must be {3 * H * W * len(panels)} contiguous uint8, got {out.dtype} {tuple(out.shape)}")
    return torch.cat(parts, dim=1, out=out.view(H, len(panels) * W, 3))


# ---- the render loop ---------------------------------------------------------------------------------------------------------------
def _encode(array: np.ndarray, path: Path, image_format: str, jpeg_quality: int) -> None:
    from PIL import Image

    if image_format == "png":
        Image.fromarray(array).save(path)
    else:
        Image.fromarray(array).save(path, quality=int(jpeg_quality))


def path_fps(meta: dict, default: float = 24.0) -> float:
    """The frame rate of a camera path (``load_camera_path``'s meta): its ``fps``, else frames / ``seconds``, else 24."""
    fps, seconds = meta.get("fps"), meta.get("seconds")
    if fps is not None and float(fps) > 0:
        return float(fps)
    if seconds is not None and float(seconds) > 0 and meta.get("num_frames"):
        return float(meta["num_frames"]) / float(seconds)
    return float(default)


def video_path_error(output_path) -> Optional[str]:
    """None when ``output_path`` can take ``output_format="video"`` (NAME.avi), else what to say."""
    p = Path(output_path)
    if p.suffix.lower() == ".avi" and not p.is_dir():
        return None
    return (f"--output-format video writes Motion-JPEG: --output-path must be NAME.avi, got {str(output_path)!r} "
            f"(`ffmpeg -i NAME.avi -c:v libx264 -pix_fmt yuv420p NAME.mp4` makes an mp4 of it)")


def render_camera_path(pipeline, cameras: Cameras, output_path, names: Sequence[str], image_format: str = "png", jpeg_quality: int = 100,
                       cube_names: Sequence[str] = (), colormap_options: Optional[ColormapOptions] = None,
                       depth_near_plane: Optional[float] = None, depth_far_plane: Optional[float] = None,
                       compose_fn=None, crop: Optional[dict] = None, output_format: str = "images", jpeg_encoder: str = "host",
                       jpeg_subsampling: str = "420", restart_mcus: Optional[int] = None, fps: Optional[float] = None,
                       png_encoder: str = "host", png_stripe_rows: Optional[int] = None) -> Dict[str, float]:
    """Render every camera of ``cameras`` (on the model's device) and write ``frame_<i:05d>.<png|jpg>`` -- and ``<name>_<i:05d>.npy``,
    float32 [H, W, C], for every name of ``cube_names`` -- into ``output_path``.  ``crop`` (``load_camera_path``'s ``meta["crop"]``):
    only what lies inside ``crop["obb"]`` is rendered -- the rays carry the box as ``nears`` / ``fars``, floored at the model's near
    plane, which is what ``get_outputs_for_camera(camera, obb_box=)`` does -- inside the model's
    ``background_color_override_context(crop["background_color"])``, which is left again when this returns or raises.

    Per frame: rays (HIP ray generator), outputs (base tensors only: no per-band view is concatenated), ``compose_frame``, then an
    asynchronous copy into one of two pinned host buffers with an event behind it.  An encoder thread (at most 4) waits for the event,
    takes the bytes out of the pinned buffer, hands the buffer back and encodes; the loop itself reads nothing back from the device
    and waits only for that hand-over (or when ``MAX_FRAMES_IN_FLIGHT`` frames are still with the encoders).

    ``jpeg_encoder="gpu"`` (with ``image_format="jpeg"``): the composed frame is encoded ON THE DEVICE (``ops.jpeg_encode``: baseline
    JPEG, ``jpeg_subsampling`` "420" or "444", restart intervals of ``restart_mcus`` MCUs, default ``ops.JPEG_DEFAULT_RESTART_MCUS``)
    into one of two device buffers; what crosses to the host is the length word and then, from the thread, that many bytes, and the
    thread only writes them.  ``output_format="video"``: ``output_path`` is NAME.avi and the frames, encoded on the device in every
    case, go into it in order (``utils.mjpeg_avi``: Motion-JPEG, ``fps`` frames per second, default 24; a file past 1 GiB continues
    in NAME_part002.avi); the cubes are written next to it; if the loop raises, the file is closed valid with the frames it has.
    ``png_encoder="gpu"`` (with ``image_format="png"``, images only): the same on-device path with ``ops.png_encode`` behind it --
    adaptive filter, independent pieces of ``png_stripe_rows`` rows (default ``ops.png_default_stripe_rows``) -- so the files are
    lossless and decode to the pixels the host encoder's files decode to.
    The defaults -- ``images``, ``host`` -- are the loop as it always was.
    ``compose_fn``: a stand-in with ``compose_frame``'s signature (tools/bench_render.py times the loop around a torch composition).
    -> {"frames", "seconds", "fps", "num_rays_per_sec"} of the whole loop, the last file written included (video: also "files")."""
    compose = compose_fn or compose_frame
    image_format = {"jpeg": "jpg"}.get(image_format, image_format)
    if image_format not in ("png", "jpg"):
        raise ValueError(f"image_format must be png or jpeg, got {image_format!r}")
    if output_format not in ("images", "video"):
        raise ValueError(f"output_format must be images or video, got {output_format!r}")
    if jpeg_encoder not in ("host", "gpu"):
        raise ValueError(f"jpeg_encoder must be host or gpu, got {jpeg_encoder!r}")
    video = output_format == "video"
    if jpeg_encoder == "gpu" and not video and image_format != "jpg":
        raise ValueError("jpeg_encoder='gpu' encodes JPEG: pass image_format='jpeg' (or output_format='video')")
    if png_encoder not in ("host", "gpu"):
        raise ValueError(f"png_encoder must be host or gpu, got {png_encoder!r}")
    device_png = png_encoder == "gpu"
    if device_png and (video or image_format != "png"):
        raise ValueError("png_encoder='gpu' encodes PNG images: pass image_format='png' and output_format='images'")
    on_device = video or jpeg_encoder == "gpu" or device_png
    names, cube_names = list(names), list(cube_names)
    if len(names) < 1:
        raise ValueError("no rendered output name: a frame holds at least one panel")
    output_path = Path(output_path)
    if video:
        problem = video_path_error(output_path)
        if problem:
            raise ValueError(problem)
    directory = output_path.parent if video else output_path
    directory.mkdir(parents=True, exist_ok=True)
    model, n, H, W = pipeline.model, len(cameras), cameras.height, cameras.width
    if on_device:
        from . import ops

        # the device encoder behind the path: (bound on the file, workspace bytes, encode into a slot); bad values are refused here,
        # before anything is rendered
        if device_png:
            ops._png_params("adaptive", png_stripe_rows)
            max_bytes = lambda fh, fw: ops.png_max_bytes(fh, fw, 3, png_stripe_rows)
            workspace_bytes = lambda fh, fw: ops.png_workspace_bytes(fh, fw, 3, png_stripe_rows)
            encode = lambda frame, slot: ops.png_encode(frame, "adaptive", png_stripe_rows, out=slot["encoded"],
                                                        length=slot["device_length"], workspace=slot["workspace"])
        else:
            ops._jpeg_params(jpeg_quality, jpeg_subsampling, restart_mcus)
            max_bytes = lambda fh, fw: ops.jpeg_max_bytes(fh, fw, jpeg_subsampling, restart_mcus)
            workspace_bytes = lambda fh, fw: ops.jpeg_workspace_bytes(fh, fw, jpeg_subsampling, restart_mcus)
            encode = lambda frame, slot: ops.jpeg_encode(frame, jpeg_quality, jpeg_subsampling, restart_mcus, out=slot["encoded"],
                                                         length=slot["device_length"], workspace=slot["workspace"])
    wanted = source_keys(names, cube_names)
    box = None if crop is None else crop["obb"]
    rays = lambda i: cameras.generate_rays(i, keep_shape=True, obb_box=box, near_floor=float(model.config.near_plane) if box is not None else 0.0)
    background = contextlib.nullcontext() if crop is None else model.background_color_override_context(crop.get("background_color"))
    was_training = pipeline.training
    pipeline.eval()
    pool = ThreadPoolExecutor(max_workers=min(MAX_ENCODERS, max(1, n)))
    slots: List[Optional[dict]] = [None, None]
    in_flight = threading.Semaphore(MAX_FRAMES_IN_FLIGHT)
    futures = []
    writer = None
    ordered = {"lock": threading.Lock(), "next": 0, "pending": {}}  # video: frames enter the file in order, whichever thread is first

    def take_encoded(slot: dict) -> bytes:
        """The file the device encoder left in the slot's device buffer: ``length`` bytes, copied on the slot's own stream."""
        length = int(slot["length"][0])
        if length > slot["encoded"].numel():
            raise RuntimeError(f"the encoded frame needs {length} bytes, the buffer holds {slot['encoded'].numel()}")  # (max_bytes: cannot happen)
        if slot["host"] is None or slot["host"].numel() < length:
            slot["host"] = torch.empty(max(length + length // 4, 1 << 16), dtype=torch.uint8).pin_memory()
        with torch.cuda.stream(slot["stream"]):
            slot["host"][:length].copy_(slot["encoded"][:length], non_blocking=True)
        slot["stream"].synchronize()
        return slot["host"][:length].numpy().tobytes()

    def finish(slot: dict, event, index: int) -> None:
        try:
            event.synchronize()
            frame = take_encoded(slot) if on_device else slot["frame"].numpy().copy()
            cubes = {k: v.numpy().copy() for k, v in slot["cubes"].items()}
        finally:
            slot["free"].set()  # the pinned buffers may be written again
        try:
            if video:
                with ordered["lock"]:
                    ordered["pending"][index] = frame
                    while ordered["next"] in ordered["pending"]:
                        writer.add_frame(ordered["pending"].pop(ordered["next"]))
                        ordered["next"] += 1
            elif on_device:
                (directory / f"frame_{index:05d}.{image_format}").write_bytes(frame)
            else:
                _encode(frame, directory / f"frame_{index:05d}.{image_format}", image_format, jpeg_quality)
            for k, v in cubes.items():
                np.save(directory / f"{k}_{index:05d}.npy", v)
        finally:
            in_flight.release()

    start = time.time()
    try:
        with torch.no_grad(), background:
            device_frame = None
            for i in range(n):
                outputs = model.get_outputs_for_camera_ray_bundle(rays(i), output_names=wanted)
                missing = [k for k in wanted if k not in outputs]
                if missing:  # name the usable outputs from the model's full dict
                    full = model.get_outputs_for_camera_ray_bundle(rays(i))
                    for name in [*names, *cube_names]:
                        if name in cube_names and name not in full:
                            raise ValueError(f"no output named {name!r} to write as a cube; the model returns: {', '.join(full)}")
                        if name in names:
                            resolve_output(full, name)
                    raise ValueError(f"the model returned no {missing}")
                device_frame = compose(outputs, names, colormap_options, depth_near_plane, depth_far_plane, out=device_frame)
                slot = slots[i % 2]
                if slot is None:
                    slot = slots[i % 2] = {
                        "cubes": {k: torch.empty(outputs[k].shape, dtype=torch.float32).pin_memory() for k in cube_names},
                        "free": threading.Event()}
                    if on_device:
                        fh, fw, dev = int(device_frame.shape[0]), int(device_frame.shape[1]), device_frame.device
                        slot.update(encoded=torch.empty(max_bytes(fh, fw), dtype=torch.uint8, device=dev),
                                    device_length=torch.empty(1, dtype=torch.int64, device=dev),
                                    workspace=torch.empty(workspace_bytes(fh, fw), dtype=torch.uint8, device=dev),
                                    length=torch.empty(1, dtype=torch.int64).pin_memory(), host=None, stream=torch.cuda.Stream(dev))
                        if video and writer is None:
                            from .utils.mjpeg_avi import MjpegAviWriter

                            writer = MjpegAviWriter(output_path, fw, fh, 24 if fps is None else fps)
                    else:
                        slot["frame"] = torch.empty(device_frame.shape, dtype=torch.uint8).pin_memory()
                else:
                    slot["free"].wait()  # the hand-over: the encoder of frame i - 2 has taken its bytes out of this buffer
                slot["free"].clear()
                if on_device:
                    encode(device_frame, slot)
                    slot["length"].copy_(slot["device_length"], non_blocking=True)
                else:
                    slot["frame"].copy_(device_frame, non_blocking=True)
                for k in cube_names:
                    slot["cubes"][k].copy_(outputs[k], non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                in_flight.acquire()
                futures.append(pool.submit(finish, slot, event, i))
            for f in futures:
                f.result()  # (re-raises what an encoder raised)
    finally:
        pool.shutdown(wait=True)
        if writer is not None:
            writer.close()  # (valid with the frames it has, also when the loop raised)
        if was_training:
            pipeline.train()
    seconds = time.time() - start
    result = {"frames": n, "seconds": seconds, "fps": n / seconds, "num_rays_per_sec": n * H * W / seconds}
    if video:
        result["files"] = [str(p) for p in (writer.paths if writer is not None else [])]
    return result


def split_cameras(pipeline, split: str):
    """(Cameras, image file names) of ``train`` or of the eval split (``val`` / ``test`` / ``eval``: the one the pipeline holds)."""
    dm = pipeline.datamanager
    if split not in ("train", "val", "test", "eval"):
        raise ValueError(f"split {split!r}: train, val or test (or train+test)")
    ds = dm.train_dataset if split == "train" else dm.eval_dataset
    if ds is None or len(ds) == 0:
        raise ValueError(f"the scene has no {split} split")
    return ds.cameras, list(ds.image_filenames)


def render_dataset(pipeline, splits: Sequence[str], output_path, names: Sequence[str], image_format: str = "png", jpeg_quality: int = 100,
                   colormap_options: Optional[ColormapOptions] = None, depth_near_plane: Optional[float] = None,
                   depth_far_plane: Optional[float] = None, jpeg_encoder: str = "host", png_encoder: str = "host",
                   png_stripe_rows: Optional[int] = None) -> Dict[str, float]:
    """``ns-render dataset``: every camera of every split of ``splits`` at its own pose and intrinsics, each name of ``names`` composed
    as a frame of ONE panel (``compose_frame``) and written to ``output_path/<split>/<name>/<image stem>.<png|jpg>``.
    ``jpeg_encoder="gpu"`` (with ``image_format="jpeg"``): the panels are encoded on the device (``ops.jpeg_encode``, 4:2:0);
    ``png_encoder="gpu"`` (with ``image_format="png"``): by ``ops.png_encode`` in pieces of ``png_stripe_rows`` rows.
    -> {"frames", "files", "seconds", "fps", "num_rays_per_sec"}."""
    image_format = {"jpeg": "jpg"}.get(image_format, image_format)
    if image_format not in ("png", "jpg"):
        raise ValueError(f"image_format must be png or jpeg, got {image_format!r}")
    names = list(names)
    if len(names) < 1:
        raise ValueError("no rendered output name: every image is written once per name")
    if jpeg_encoder not in ("host", "gpu"):
        raise ValueError(f"jpeg_encoder must be host or gpu, got {jpeg_encoder!r}")
    if jpeg_encoder == "gpu" and image_format != "jpg":
        raise ValueError("jpeg_encoder='gpu' encodes JPEG: pass image_format='jpeg'")
    if png_encoder not in ("host", "gpu"):
        raise ValueError(f"png_encoder must be host or gpu, got {png_encoder!r}")
    if png_encoder == "gpu":
        if image_format != "png":
            raise ValueError("png_encoder='gpu' encodes PNG images: pass image_format='png'")
        from . import ops

        ops._png_params("adaptive", png_stripe_rows)  # (refused here, before anything is rendered)
    output_path, model = Path(output_path), pipeline.model
    wanted = source_keys(names)
    was_training = pipeline.training
    pipeline.eval()
    frames = files = pixels = 0
    start = time.time()
    try:
        with torch.no_grad():
            for split in splits:
                cameras, filenames = split_cameras(pipeline, split)
                for name in names:
                    (output_path / split / name).mkdir(parents=True, exist_ok=True)
                for i in range(len(cameras)):
                    outputs = model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True), output_names=wanted)
                    for name in names:
                        frame = compose_frame(outputs, [name], colormap_options, depth_near_plane, depth_far_plane)
                        target = output_path / split / name / f"{Path(str(filenames[i])).stem}.{image_format}"
                        if jpeg_encoder == "gpu" or png_encoder == "gpu":
                            from . import ops

                            data, length = (ops.png_encode(frame, "adaptive", png_stripe_rows) if png_encoder == "gpu"
                                            else ops.jpeg_encode(frame, jpeg_quality, "420"))
                            target.write_bytes(data[:int(length.item())].cpu().numpy().tobytes())
                        else:
                            _encode(frame.cpu().numpy(), target, image_format, jpeg_quality)
                        files += 1
                    frames, pixels = frames + 1, pixels + cameras.height * cameras.width
    finally:
        if was_training:
            pipeline.train()
    seconds = time.time() - start
    return {"frames": frames, "files": files, "seconds": seconds, "fps": frames / seconds, "num_rays_per_sec": pixels / seconds}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _bool(s: str) -> bool:
    return s.lower() in ("1", "true", "yes")


def _add_render_arguments(p, cubes: bool) -> None:
    """What every subcommand shares: the model, where the files go, which outputs, how they are coloured and encoded."""
    from .eval import add_model_arguments
    from .library import add_library_arguments
    from .statistics import add_statistics_arguments
    from .unmix import add_unmix_arguments
    from .sparse import add_sparse_arguments
    from .continuum import add_continuum_arguments
    from .cluster import add_cluster_arguments

    add_model_arguments(p)
    p.add_argument("--output-path", required=True, help="directory the images are written to (--output-format video: NAME.avi)")
    p.add_argument("--rendered-output-names", nargs="+", default=["rgb"], help="outputs to render, e.g. rgb abundances_0 wv_3 depth")
    if cubes:
        p.add_argument("--cube-output-names", nargs="*", default=[], help="outputs also written whole as float32 .npy, e.g. spectral abundances")
    p.add_argument("--colormap", default="default")
    p.add_argument("--colormap-min", type=float, default=0.0)
    p.add_argument("--colormap-max", type=float, default=1.0)
    p.add_argument("--colormap-normalize", type=_bool, nargs="?", const=True, default=False)
    p.add_argument("--colormap-invert", type=_bool, nargs="?", const=True, default=False)
    p.add_argument("--depth-near-plane", type=float, default=None)
    p.add_argument("--depth-far-plane", type=float, default=None)
    p.add_argument("--material-edits", default=None, metavar="FILE",
                   help="render under the material edits of this JSON file: recolour, dim or remove a material (INTEGRATION.md)")
    add_library_arguments(p)
    add_statistics_arguments(p)
    add_unmix_arguments(p)
    add_sparse_arguments(p)
    add_continuum_arguments(p)
    add_cluster_arguments(p)
    p.add_argument("--image-format", default="png", choices=["png", "jpeg"])
    p.add_argument("--jpeg-quality", type=int, default=100)
    p.add_argument("--jpeg-encoder", default="host", choices=["host", "gpu"],
                   help="who encodes --image-format jpeg: PIL on host threads, or the baseline-JPEG encoder on the device")
    p.add_argument("--png-encoder", default="host", choices=["host", "gpu"],
                   help="who encodes --image-format png: PIL on host threads, or the PNG encoder on the device (lossless either way)")
    p.add_argument("--png-stripe-rows", type=int, default=None, metavar="N",
                   help="rows per independent piece of the device PNG encoder (1..65535; one workgroup and one IDAT chunk each)")
    if cubes:  # (camera-path and interpolate)
        p.add_argument("--jpeg-subsampling", default="420", choices=["420", "444"], help="chroma subsampling of the device encoder")
        p.add_argument("--restart-mcus", type=int, default=None,
                       help="MCUs per restart interval of the device encoder (1..65535; one wavefront encodes one interval)")


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m umhsnerf.render", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    cp = sub.add_parser("camera-path", help="render the cameras of a camera-path file (ns-render camera-path)")
    _add_render_arguments(cp, cubes=True)
    cp.add_argument("--camera-path-filename", required=True, help="camera path exported by the viewer (JSON)")
    cp.add_argument("--downscale-factor", type=float, default=1.0)
    cp.add_argument("--output-format", default="images", choices=["images", "video"])
    ds = sub.add_parser("dataset", help="render every camera of a split at its own pose (ns-render dataset)")
    _add_render_arguments(ds, cubes=False)
    ds.add_argument("--split", default="test", choices=["train", "val", "test", "train+test"])
    ip = sub.add_parser("interpolate", help="render poses interpolated between the cameras of a split (ns-render interpolate)")
    _add_render_arguments(ip, cubes=True)
    ip.add_argument("--pose-source", default="eval", choices=["eval", "train"])
    ip.add_argument("--interpolation-steps", type=int, default=10)
    ip.add_argument("--order-poses", type=_bool, nargs="?", const=True, default=False)
    ip.add_argument("--output-format", default="images", choices=["images", "video"])
    sub.add_parser("spiral", help="not available", add_help=False)
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv[:1] == ["spiral"]:
        ap.error("spiral is not available: render a camera path exported by the viewer (camera-path), or interpolate")
    args = ap.parse_args(argv)
    cur = {"camera-path": cp, "dataset": ds, "interpolate": ip}[args.command]
    if getattr(args, "output_format", "images") == "video":
        problem = video_path_error(args.output_path)
        if problem:
            cur.error(problem)
        if not 1 <= args.jpeg_quality <= 100:
            cur.error("--jpeg-quality must be 1..100")
    elif args.jpeg_encoder == "gpu" and args.image_format != "jpeg":
        cur.error("--jpeg-encoder gpu encodes JPEG: pass --image-format jpeg (or --output-format video)")
    if args.png_encoder == "gpu" and (args.image_format != "png" or getattr(args, "output_format", "images") == "video"):
        cur.error("--png-encoder gpu encodes PNG images: it goes with --image-format png and --output-format images")
    if args.png_stripe_rows is not None and not 1 <= args.png_stripe_rows <= 65535:
        cur.error("--png-stripe-rows must be 1..65535")
    if getattr(args, "restart_mcus", None) is not None and not 1 <= args.restart_mcus <= 65535:
        cur.error("--restart-mcus must be 1..65535")
    if args.command == "interpolate":
        if args.order_poses:
            ip.error("--order-poses true is not available: the cameras are taken in the order of the split")
        if args.interpolation_steps < 2:
            ip.error("--interpolation-steps must be at least 2: both ends of a pair are rendered")
    from .utils import colormaps

    if args.colormap not in colormaps.NAMES:
        cur.error(f"--colormap {args.colormap}: one of {', '.join(colormaps.NAMES)}")
    from .library import requested_without_library

    requested_without_library([*args.rendered_output_names, *getattr(args, "cube_output_names", [])], args.spectral_library)  # ValueError
    from .statistics import requested_without_statistics

    requested_without_statistics([*args.rendered_output_names, *getattr(args, "cube_output_names", [])], args.scene_statistics)  # ValueError
    from .unmix import check_unmix_arguments

    check_unmix_arguments(args, [*args.rendered_output_names, *getattr(args, "cube_output_names", [])])  # ValueError
    from .sparse import check_sparse_arguments

    check_sparse_arguments(args, [*args.rendered_output_names, *getattr(args, "cube_output_names", [])])  # ValueError
    from .continuum import check_continuum_arguments

    check_continuum_arguments(args, [*args.rendered_output_names, *getattr(args, "cube_output_names", [])])  # ValueError
    from .cluster import requested_without_clusters

    requested_without_clusters([*args.rendered_output_names, *getattr(args, "cube_output_names", [])], args.clusters)  # ValueError
    return args


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from . import library as spectral_library
    from . import statistics as scene_statistics
    from .materials import load_for_model
    from .unmix import unmixer_from_args
    from .sparse import sparse_unmixer_from_args
    from .continuum import analysis_from_args
    from . import cluster as spectral_clusters

    args = parse_args(argv)
    device = torch.device(args.device)
    crop, fps = None, None
    if args.command == "camera-path":  # (read before the scene is loaded: a bad path file costs nothing)
        cameras, meta = load_camera_path(args.camera_path_filename, args.downscale_factor, camera_types=CAMERA_TYPES, crop=True)
        crop, fps = meta["crop"], path_fps(meta)
    pipeline = build_pipeline(args, device)
    load_checkpoint(pipeline, args.checkpoint)
    options = ColormapOptions(args.colormap, args.colormap_normalize, args.colormap_min, args.colormap_max, args.colormap_invert)
    # (a bad edit file is refused here, before anything is rendered; the context composes with a crop's background override)
    edits = load_for_model(args.material_edits, pipeline.model)
    library = spectral_library.load_for_model(args.spectral_library, pipeline.model)  # (a bad library file is refused here as well)
    scene = scene_statistics.context_arguments(args, pipeline.model)  # (and a bad statistics file)
    unmixer = unmixer_from_args(args, pipeline.model, library)  # (and endmembers too close to dependent)
    sparse_unmixer = sparse_unmixer_from_args(args, library)  # (and a library of more than 128 entries without --sparse-entries)
    # (and a bad features file; a cr / cr_<b> output needs no file: it gets an analysis without features)
    analysis = analysis_from_args(args, pipeline.model, [*args.rendered_output_names, *getattr(args, "cube_output_names", [])])
    clusters = spectral_clusters.load_for_model(args.clusters, pipeline.model)  # (and clusters fitted on another scene)
    with pipeline.model.material_edits_context(edits), pipeline.model.spectral_clusters_context(clusters), \
            pipeline.model.spectral_library_context(library, args.library_max_angle, args.library_continuum_removed), \
            pipeline.model.scene_statistics_context(**(scene or {"stats": None})), \
            pipeline.model.unmixing_context(unmixer), pipeline.model.sparse_unmixing_context(sparse_unmixer), \
            pipeline.model.continuum_context(analysis):  # (None: nothing changes)
        if args.command == "dataset":
            result = render_dataset(pipeline, args.split.split("+"), args.output_path, args.rendered_output_names, args.image_format,
                                    args.jpeg_quality, options, args.depth_near_plane, args.depth_far_plane, jpeg_encoder=args.jpeg_encoder,
                                    png_encoder=args.png_encoder, png_stripe_rows=args.png_stripe_rows)
            height, width = pipeline.datamanager.train_dataset.cameras.height, pipeline.datamanager.train_dataset.cameras.width
        else:
            if args.command == "interpolate":
                source, _ = split_cameras(pipeline, "train" if args.pose_source == "train" else "eval")
                cameras = interpolate_cameras(source, args.interpolation_steps)
            result = render_camera_path(pipeline, cameras.to(device), args.output_path, args.rendered_output_names, args.image_format,
                                        args.jpeg_quality, args.cube_output_names, options, args.depth_near_plane, args.depth_far_plane,
                                        crop=crop, output_format=args.output_format, jpeg_encoder=args.jpeg_encoder,
                                        jpeg_subsampling=args.jpeg_subsampling, restart_mcus=args.restart_mcus, fps=fps,
                                        png_encoder=args.png_encoder, png_stripe_rows=args.png_stripe_rows)
            height, width = cameras.height, cameras.width
    result.update(height=height, width=width, panels=len(args.rendered_output_names))
    if args.material_edits is not None:
        result["material_edits"] = str(args.material_edits)
    if args.spectral_library is not None:
        result["spectral_library"] = str(args.spectral_library)
    if args.scene_statistics is not None:
        result["scene_statistics"] = str(args.scene_statistics)
    if args.clusters is not None:
        result["clusters"] = str(args.clusters)
    if unmixer is not None:
        result["unmix"] = {"source": args.unmix, "constraint": unmixer.constraint, "endmembers": unmixer.names}
    if sparse_unmixer is not None:
        result["sparse_unmix"] = sparse_unmixer.summary()
    if analysis is not None:
        result["continuum"] = analysis.summary()
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
