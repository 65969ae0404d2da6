"""``python -m umhsnerf.render camera-path --data DIR --checkpoint FILE --camera-path-filename FILE --output-path DIR
--rendered-output-names rgb abundances_0 ...``: what ``ns-render camera-path`` does for a trained model (the reference's
scripts/render.sh: the abundance-map, per-band and residual fly-throughs), without nerfstudio.

A camera-path file (the viewer's export) becomes ``Cameras``; every camera is rendered with the fused, chunked
``get_outputs_for_camera_ray_bundle``, the named outputs are composed side by side into one uint8 frame ON THE DEVICE
(``ops.frame_compose``: colormaps, depth blending and quantisation in one launch, sources read in place -- ``wv_7`` is column 7 of
``spectral``, no column is copied), and only those 3 bytes per pixel and panel travel to the host, where a small thread pool encodes and
writes ``frame_<i:05d>.png`` / ``.jpg``.  ``--cube-output-names spectral abundances`` additionally writes the float32 cubes
``<name>_<i:05d>.npy`` -- the hyperspectral image of a novel view.

Not built: ``--output-format video`` (no encoder here; ``ffmpeg -framerate 24 -i frame_%05d.png out.mp4`` makes one from the
frames), ``crop``, non-perspective camera paths, ``ns-render interpolate`` / ``spiral`` / ``dataset``.

Names: an output with 3 channels is shown as it is (``rgb``, ``seg_pred``), one with 1 channel through a colormap (``accumulation``,
``seg_raw``), ``wv_i`` / ``abundances_i`` / ``residual_i`` are columns of ``spectral`` / ``abundances`` / ``specular``, and any name that
contains ``depth`` goes through nerfstudio's depth colormap: normalised by the frame's own (min, max) -- taken on the device -- or by the
planes given, and blended over white with ``accumulation``."""
from __future__ import annotations

import argparse
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
def load_camera_path(json_or_path: Union[dict, str, Path], downscale_factor: float = 1.0, device=None) -> Tuple[Cameras, dict]:
    """nerfstudio ``camera_utils.get_path_from_json`` followed by ``Cameras.rescale_output_resolution(1 / downscale_factor)``, as
    ``ns-render camera-path`` calls them  [upstream-recalled]: nerfstudio's source is not vendored, so the rules are restated here.

    ``render_height`` x ``render_width`` frames; per entry of ``camera_path``: ``camera_to_world``, 16 row-major floats of which rows 0..2
    are used AS THEY ARE (a viewer path is in the model's coordinates already), and ``fov`` in degrees (vertical):
    ``fx = fy = (H / 2) / tan(fov * pi / 360)``, ``cx = W / 2``, ``cy = H / 2``; ``aspect`` is ignored.  ``downscale_factor`` d: the
    intrinsics are multiplied by 1 / d and the size becomes ``int(H / d)`` x ``int(W / d)``.  -> (Cameras, {"num_frames", "render_height",
    "render_width", "fps", "seconds"})."""
    if isinstance(json_or_path, dict):
        path = json_or_path
    else:
        with open(json_or_path) as f:
            path = json.load(f)
    camera_type = str(path.get("camera_type", "perspective")).lower()
    if camera_type != "perspective":
        raise NotImplementedError(f"camera_type {camera_type!r}: only perspective camera paths are rendered")
    if path.get("crop") is not None:
        raise NotImplementedError("camera paths with a crop box are not rendered")
    entries = path.get("camera_path") or []
    if len(entries) == 0:
        raise ValueError("the camera path holds no camera")
    if not downscale_factor > 0:
        raise ValueError(f"downscale_factor must be positive, got {downscale_factor}")
    H, W = int(path["render_height"]), int(path["render_width"])
    c2w, focal = [], []
    for k, cam in enumerate(entries):
        m = [float(v) for v in cam["camera_to_world"]]
        if len(m) != 16:
            raise ValueError(f"camera {k}: camera_to_world must hold 16 values, got {len(m)}")
        c2w.append(m[:12])
        focal.append((H / 2.0) / math.tan(float(cam["fov"]) * math.pi / 360.0))
    s = 1.0 / float(downscale_factor)
    n = len(entries)
    f = torch.tensor(focal, dtype=torch.float64) * s
    cameras = Cameras(torch.tensor(c2w, dtype=torch.float32).view(n, 3, 4), f.float(), f.float().clone(),
                      torch.full((n,), (W / 2.0) * s, dtype=torch.float32), torch.full((n,), (H / 2.0) * s, dtype=torch.float32),
                      int(H / downscale_factor), int(W / downscale_factor))
    if cameras.height < 1 or cameras.width < 1:
        raise ValueError(f"downscale_factor {downscale_factor} leaves no pixel of {H} x {W}")
    meta = {"num_frames": n, "render_height": cameras.height, "render_width": cameras.width, "fps": path.get("fps"),
            "seconds": path.get("seconds")}
    return (cameras if device is None else cameras.to(device)), meta


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


def render_camera_path(pipeline, cameras: Cameras, output_path, names: Sequence[str], image_format: str = "png", jpeg_quality: int = 100,
                       cube_names: Sequence[str] = (), colormap_options: Optional[ColormapOptions] = None,
                       depth_near_plane: Optional[float] = None, depth_far_plane: Optional[float] = None,
                       compose_fn=None) -> Dict[str, float]:
    """Render every camera of ``cameras`` (on the model's device) and write ``frame_<i:05d>.<png|jpg>`` -- and ``<name>_<i:05d>.npy``,
    float32 [H, W, C], for every name of ``cube_names`` -- into ``output_path``.

    Per frame: rays (HIP ray generator), outputs (base tensors only: no per-band view is concatenated), ``compose_frame``, then an
    asynchronous copy into one of two pinned host buffers with an event behind it.  An encoder thread (at most 4) waits for the event,
    takes the bytes out of the pinned buffer, hands the buffer back and encodes; the loop itself reads nothing back from the device
    and waits only for that hand-over (or when ``MAX_FRAMES_IN_FLIGHT`` frames are still with the encoders).
    ``compose_fn``: a stand-in with ``compose_frame``'s signature (tools/bench_render.py times the loop around a torch composition).
    -> {"frames", "seconds", "fps", "num_rays_per_sec"} of the whole loop, the last file written included."""
    compose = compose_fn or compose_frame
    image_format = {"jpeg": "jpg"}.get(image_format, image_format)
    if image_format not in ("png", "jpg"):
        raise ValueError(f"image_format must be png or jpeg, got {image_format!r}")
    names, cube_names = list(names), list(cube_names)
    if len(names) < 1:
        raise ValueError("no rendered output name: a frame holds at least one panel")
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    model, n, H, W = pipeline.model, len(cameras), cameras.height, cameras.width
    wanted = source_keys(names, cube_names)
    was_training = pipeline.training
    pipeline.eval()
    pool = ThreadPoolExecutor(max_workers=min(MAX_ENCODERS, max(1, n)))
    slots: List[Optional[dict]] = [None, None]
    in_flight = threading.Semaphore(MAX_FRAMES_IN_FLIGHT)
    futures = []

    def finish(slot: dict, event, index: int) -> None:
        try:
            event.synchronize()
            frame = slot["frame"].numpy().copy()
            cubes = {k: v.numpy().copy() for k, v in slot["cubes"].items()}
        finally:
            slot["free"].set()  # the pinned buffers may be written again
        try:
            _encode(frame, output_path / f"frame_{index:05d}.{image_format}", image_format, jpeg_quality)
            for k, v in cubes.items():
                np.save(output_path / f"{k}_{index:05d}.npy", v)
        finally:
            in_flight.release()

    start = time.time()
    try:
        with torch.no_grad():
            device_frame = None
            for i in range(n):
                outputs = model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True), output_names=wanted)
                missing = [k for k in wanted if k not in outputs]
                if missing:  # name the usable outputs from the model's full dict
                    full = model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True))
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
                        "frame": torch.empty(device_frame.shape, dtype=torch.uint8).pin_memory(),
                        "cubes": {k: torch.empty(outputs[k].shape, dtype=torch.float32).pin_memory() for k in cube_names},
                        "free": threading.Event()}
                else:
                    slot["free"].wait()  # the hand-over: the encoder of frame i - 2 has taken its bytes out of this buffer
                slot["free"].clear()
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
        if was_training:
            pipeline.train()
    seconds = time.time() - start
    return {"frames": n, "seconds": seconds, "fps": n / seconds, "num_rays_per_sec": n * H * W / seconds}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _bool(s: str) -> bool:
    return s.lower() in ("1", "true", "yes")


def parse_args(argv=None) -> argparse.Namespace:
    from .eval import add_model_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.render", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    cp = sub.add_parser("camera-path", help="render the cameras of a camera-path file (ns-render camera-path)")
    add_model_arguments(cp)
    cp.add_argument("--camera-path-filename", required=True, help="camera path exported by the viewer (JSON)")
    cp.add_argument("--output-path", required=True, help="directory for frame_<i>.png / .jpg (and <name>_<i>.npy)")
    cp.add_argument("--rendered-output-names", nargs="+", default=["rgb"], help="outputs shown side by side, e.g. rgb abundances_0 wv_3 depth")
    cp.add_argument("--cube-output-names", nargs="*", default=[], help="outputs also written whole as float32 .npy, e.g. spectral abundances")
    cp.add_argument("--downscale-factor", type=float, default=1.0)
    cp.add_argument("--colormap", default="default")
    cp.add_argument("--colormap-min", type=float, default=0.0)
    cp.add_argument("--colormap-max", type=float, default=1.0)
    cp.add_argument("--colormap-normalize", type=_bool, nargs="?", const=True, default=False)
    cp.add_argument("--colormap-invert", type=_bool, nargs="?", const=True, default=False)
    cp.add_argument("--depth-near-plane", type=float, default=None)
    cp.add_argument("--depth-far-plane", type=float, default=None)
    cp.add_argument("--image-format", default="png", choices=["png", "jpeg"])
    cp.add_argument("--jpeg-quality", type=int, default=100)
    cp.add_argument("--output-format", default="images", choices=["images", "video"])
    args = ap.parse_args(argv)
    if args.output_format == "video":
        cp.error("--output-format video is not available (no video encoder here): render images and run "
                 "`ffmpeg -framerate 24 -i frame_%05d.png out.mp4` on them")
    from .utils import colormaps

    if args.colormap not in colormaps.NAMES:
        cp.error(f"--colormap {args.colormap}: one of {', '.join(colormaps.NAMES)}")
    return args


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint

    args = parse_args(argv)
    device = torch.device(args.device)
    cameras, meta = load_camera_path(args.camera_path_filename, args.downscale_factor)
    pipeline = build_pipeline(args, device)
    load_checkpoint(pipeline, args.checkpoint)
    options = ColormapOptions(args.colormap, args.colormap_normalize, args.colormap_min, args.colormap_max, args.colormap_invert)
    result = render_camera_path(pipeline, cameras.to(device), args.output_path, args.rendered_output_names, args.image_format,
                                args.jpeg_quality, args.cube_output_names, options, args.depth_near_plane, args.depth_far_plane)
    result.update(height=meta["render_height"], width=meta["render_width"], panels=len(args.rendered_output_names))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
