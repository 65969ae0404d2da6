"""Frame operators of the renderer: panels composed into a displayable frame, the baseline-JPEG and the PNG frame encoder."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _hip
from .._hip import ptr


PANEL_RGB, PANEL_SCALAR, PANEL_DEPTH = 0, 1, 2  # include/umhs_hip.h UMHS_PANEL_*


@dataclass
class FramePanel:
    """One panel of ``frame_compose`` (umhs_frame_panel).  ``src``: float32 rows on the device, [H*W], [H*W, c] or [H, W, c], read in
    place -- a column view such as ``spectral[:, 7]`` or ``abundances[:, 2:3]`` is taken at its own row stride, nothing is copied.
    ``channel``: first column of ``src`` read (RGB reads three).  ``range``: device (lo, hi) of DEPTH and of SCALAR with
    ``normalize``.  ``accumulation``: [H*W] floats a DEPTH panel is blended over white with."""
    src: torch.Tensor
    kind: int = PANEL_SCALAR
    channel: int = 0
    range: Optional[torch.Tensor] = None
    accumulation: Optional[torch.Tensor] = None
    normalize: bool = False
    invert: bool = False
    cmin: float = 0.0
    cmax: float = 1.0


def _frame_f32(t, what: str, dev=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"frame_compose: {what} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"frame_compose: {what} must be float32, got {t.dtype}")
    if dev is not None and t.device != dev:
        raise ValueError(f"frame_compose: {what} is on {t.device}, the colour table on {dev}")
    return t


def _frame_rows(src, n: int, what: str):
    """(tensor whose data_ptr is row 0, floats per row, columns) of a source of n rows that is read in place."""
    lead = src.numel() if src.dim() <= 1 else int(np.prod(src.shape[:-1]))
    if lead != n:
        raise ValueError(f"frame_compose: {what} of shape {tuple(src.shape)} does not hold {n} rows")
    try:
        rows = src.reshape(n, 1) if src.dim() <= 1 else src if src.dim() == 2 else src.view(n, src.shape[-1])
    except RuntimeError as e:
        raise ValueError(f"frame_compose: {what} of shape {tuple(src.shape)} is not {n} rows that can be read in place") from e
    c = rows.shape[1]
    if c == 0 or (c > 1 and rows.stride(1) != 1):
        raise ValueError(f"frame_compose: the columns of {what} must be adjacent floats (strides {tuple(rows.stride())})")
    stride = rows.stride(0) if n > 1 else c
    if stride < c:
        raise ValueError(f"frame_compose: the rows of {what} overlap (strides {tuple(rows.stride())})")
    return rows, stride, c


def frame_compose(panels: Sequence[FramePanel], lut, height: int, width: int, out=None):
    """uint8 [height, K * width, 3]: the K panels side by side, each the displayable form of one per-ray output (umhs_frame_compose:
    RGB quantised; SCALAR through nerfstudio's apply_float_colormap; DEPTH through apply_depth_colormap).  ``lut``: float32 [256, 3]
    colour table on the device.  ``out``: a contiguous uint8 tensor of that many elements at ANY byte offset (a view of a larger
    buffer).  One launch, no host sync; the sources are kept alive by ``panels`` until the launch has been queued."""
    panels = list(panels)
    height, width, K = int(height), int(width), len(panels)
    if height < 0 or width < 0 or not 1 <= K <= 16:
        raise ValueError(f"frame_compose: {K} panels of {height} x {width} (1..16 panels, sizes >= 0)")
    lut = _frame_f32(lut, "lut")
    if tuple(lut.shape) != (256, 3) or not lut.is_contiguous():
        raise ValueError(f"frame_compose: lut must be a contiguous [256, 3], got {tuple(lut.shape)}")
    dev, n = lut.device, height * width
    arr, keep = (_hip.FramePanel * K)(), []
    for k, p in enumerate(panels):
        if p.kind not in (PANEL_RGB, PANEL_SCALAR, PANEL_DEPTH):
            raise ValueError(f"frame_compose: panel {k} has kind {p.kind}")
        rows, stride, c = _frame_rows(_frame_f32(p.src, f"panel {k}", dev), n, f"panel {k}")
        need = 3 if p.kind == PANEL_RGB else 1
        if p.channel < 0 or p.channel + need > c:
            raise ValueError(f"frame_compose: panel {k} reads columns {p.channel}..{p.channel + need - 1} of {c}")
        wants_range = p.kind == PANEL_DEPTH or (p.kind == PANEL_SCALAR and p.normalize)
        rng = acc = None
        if wants_range:
            if p.range is None:
                raise ValueError(f"frame_compose: panel {k} needs a (lo, hi) range")
            rng = _frame_f32(p.range, f"range of panel {k}", dev)
            if rng.numel() != 2 or not rng.is_contiguous():
                raise ValueError(f"frame_compose: range of panel {k} must be 2 contiguous floats, got {tuple(rng.shape)}")
        if p.kind == PANEL_DEPTH and p.accumulation is not None:
            acc = _frame_f32(p.accumulation, f"accumulation of panel {k}", dev)
            if acc.numel() != n or not acc.is_contiguous():
                raise ValueError(f"frame_compose: accumulation of panel {k} must be {n} contiguous floats, got {tuple(acc.shape)}")
        keep += [rows, rng, acc]
        arr[k] = _hip.FramePanel(rows.data_ptr() if n else 4, rng.data_ptr() if rng is not None else None,
                                 acc.data_ptr() if acc is not None and n else None, max(stride, p.channel + need), p.channel, p.kind,
                                 int(bool(p.normalize)) | 2 * int(bool(p.invert)), float(p.cmin), float(p.cmax))
    if out is None:
        out = torch.empty(height, K * width, 3, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or out.numel() != 3 * K * n or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f"frame_compose: out must be {3 * K * n} contiguous uint8 on {dev}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if n == 0:
        return out.view(height, K * width, 3)
    _hip.check(_hip.lib().umhs_frame_compose(arr, K, ptr(lut), height, width, C.c_void_p(out.data_ptr()), _hip.stream()),
               "umhs_frame_compose")
    del keep
    return out.view(height, K * width, 3)


# ---- baseline-JPEG frame encoder (umhs_jpeg.hip) --------------------------------------------------------------------------------------
JPEG_SUBSAMPLING = {"444": 0, "420": 1}  # UMHS_JPEG_444 / UMHS_JPEG_420
JPEG_HEADER_BYTES = 629
# MCUs per restart interval (one wavefront each) when the caller names none: tools/bench_video.py's sweep
JPEG_DEFAULT_RESTART_MCUS = 16


def _jpeg_frame(frame):
    if not torch.is_tensor(frame) or not frame.is_cuda:
        raise ValueError("jpeg: the frame must be a tensor on a HIP device (there is no CPU path)")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():
        raise ValueError(f"jpeg: the frame must be a contiguous uint8 [H, W, 3], got {frame.dtype} {tuple(frame.shape)}")
    H, W = int(frame.shape[0]), int(frame.shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"jpeg: a frame of {H} x {W} has no pixel")
    return H, W


def _jpeg_params(quality, subsampling, restart_mcus):
    if str(subsampling) not in JPEG_SUBSAMPLING:
        raise ValueError(f"jpeg: subsampling must be one of {', '.join(JPEG_SUBSAMPLING)}, got {subsampling!r}")
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"jpeg: quality must be 1..100, got {quality}")
    restart_mcus = JPEG_DEFAULT_RESTART_MCUS if restart_mcus is None else int(restart_mcus)
    if not 1 <= restart_mcus <= 65535:
        raise ValueError(f"jpeg: restart_mcus must be 1..65535, got {restart_mcus}")
    return quality, JPEG_SUBSAMPLING[str(subsampling)], restart_mcus


def jpeg_blocks_per_mcu(subsampling) -> int:
    return 6 if str(subsampling) == "420" else 3


def jpeg_workspace_bytes(height: int, width: int, subsampling="420", restart_mcus=None) -> int:
    _, ss, r = _jpeg_params(100, subsampling, restart_mcus)
    return int(_hip.lib().umhs_jpeg_workspace_bytes(int(height), int(width), ss, r))


def jpeg_max_bytes(height: int, width: int, subsampling="420", restart_mcus=None) -> int:
    """An upper bound on the length of the file for ANY content of the frame."""
    _, ss, r = _jpeg_params(100, subsampling, restart_mcus)
    return int(_hip.lib().umhs_jpeg_max_bytes(int(height), int(width), ss, r))


def jpeg_coefficients(frame, quality: int = 100, subsampling="420"):
    """The transform stage of the frame encoder (umhs_jpeg_coefficients): uint8 [H, W, 3] at any byte address -> int16 [n_mcus, 3 or 6,
    64], the blocks of an MCU in scan order and their coefficients in zigzag order.  One launch, no sync."""
    H, W = _jpeg_frame(frame)
    quality, ss, _ = _jpeg_params(quality, subsampling, 1)
    bpm = jpeg_blocks_per_mcu(subsampling)
    n_blocks = int(_hip.lib().umhs_jpeg_blocks(H, W, ss))
    if n_blocks == 0:
        raise ValueError(f"jpeg: a frame of {H} x {W} is outside 1..65535")
    out = torch.empty(n_blocks // bpm, bpm, 64, dtype=torch.int16, device=frame.device)
    _hip.check(_hip.lib().umhs_jpeg_coefficients(C.c_void_p(frame.data_ptr()), H, W, quality, ss, C.c_void_p(out.data_ptr()), _hip.stream()),
               "umhs_jpeg_coefficients")
    return out


def _jpeg_out(out, length, dev, capacity):
    if out is None:
        out = torch.empty(int(capacity), dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"jpeg: out must be a contiguous uint8 vector on {dev}")
    if length is None:
        length = torch.empty(1, dtype=torch.int64, device=dev)
    elif not torch.is_tensor(length) or length.dtype != torch.int64 or length.numel() != 1 or length.device != dev:
        raise ValueError(f"jpeg: length must be one int64 on {dev}")
    return out, length


def jpeg_encode(frame, quality: int = 100, subsampling="420", restart_mcus=None, out=None, length=None, workspace=None):
    """One baseline-JPEG file of ``frame`` (uint8 [H, W, 3] on the device, any byte address), encoded on the device (umhs_jpeg_encode).
    -> (out uint8 [capacity], length int64 [1]), both on the device: the file is ``out[:length]``.  ``out``: the buffer to fill (its
    size is the capacity; default: ``jpeg_max_bytes``, which no content exceeds); when the file is longer than the capacity, nothing is
    written past it and ``length`` holds the size needed.  ``workspace``: uint8 of at least ``jpeg_workspace_bytes`` (default: a new
    one).  Four launches on the current stream, no sync."""
    H, W = _jpeg_frame(frame)
    quality, ss, r = _jpeg_params(quality, subsampling, restart_mcus)
    lib, dev = _hip.lib(), frame.device
    need = int(lib.umhs_jpeg_workspace_bytes(H, W, ss, r))
    if need == 0:
        raise ValueError(f"jpeg: a frame of {H} x {W} is outside 1..65535")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"jpeg: the workspace must be at least {need} contiguous uint8 on {dev}")
    out, length = _jpeg_out(out, length, dev, lib.umhs_jpeg_max_bytes(H, W, ss, r))
    _hip.check(lib.umhs_jpeg_encode(C.c_void_p(frame.data_ptr()), H, W, quality, ss, r, C.c_void_p(out.data_ptr()), out.numel(),
                                    C.c_void_p(length.data_ptr()), C.c_void_p(workspace.data_ptr()), workspace.numel(), _hip.stream()),
               "umhs_jpeg_encode")
    return out, length


def jpeg_entropy(coefficients, height: int, width: int, quality: int = 100, subsampling="420", restart_mcus=None, out=None, length=None):
    """The entropy stage alone (umhs_jpeg_entropy) on given coefficients, int16 [n_mcus, 3 or 6, 64] as ``jpeg_coefficients`` lays them
    out -> (out, length) as ``jpeg_encode``."""
    quality, ss, r = _jpeg_params(quality, subsampling, restart_mcus)
    lib, H, W = _hip.lib(), int(height), int(width)
    n_blocks = int(lib.umhs_jpeg_blocks(H, W, ss))
    if (not torch.is_tensor(coefficients) or not coefficients.is_cuda or coefficients.dtype != torch.int16 or not coefficients.is_contiguous()
            or n_blocks == 0 or coefficients.numel() != 64 * n_blocks):
        raise ValueError(f"jpeg: the coefficients of a {H} x {W} frame are {n_blocks} x 64 contiguous int16 on a HIP device")
    dev = coefficients.device
    n_mcus = n_blocks // jpeg_blocks_per_mcu(subsampling)
    table = torch.empty((n_mcus + r - 1) // r, dtype=torch.int64, device=dev)
    out, length = _jpeg_out(out, length, dev, lib.umhs_jpeg_max_bytes(H, W, ss, r))
    _hip.check(lib.umhs_jpeg_entropy(C.c_void_p(coefficients.data_ptr()), H, W, quality, ss, r, C.c_void_p(out.data_ptr()), out.numel(),
                                     C.c_void_p(length.data_ptr()), C.c_void_p(table.data_ptr()), 8 * table.numel(), _hip.stream()),
               "umhs_jpeg_entropy")
    return out, length


# ---- PNG frame encoder (umhs_png.hip) --------------------------------------------------------------------------------------------------
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}  # UMHS_PNG_FILTER_*
# a piece (one workgroup, one IDAT chunk) is the fewest rows whose filtered bytes reach this many when the caller names no stripe_rows
PNG_PIECE_TARGET_BYTES = 32 << 10
WS_PNG = "png_encode"  # ops/workspace.py slot of png_encode's default workspace: per-call scratch, never leased


def png_default_stripe_rows(width: int, channels: int = 3) -> int:
    """The fewest rows whose filtered bytes (1 + width * channels each) reach ``PNG_PIECE_TARGET_BYTES``."""
    row = 1 + int(width) * int(channels)
    return max(1, min(65535, -(-PNG_PIECE_TARGET_BYTES // row)))


def _png_frame(frame):
    if not torch.is_tensor(frame) or not frame.is_cuda:
        raise ValueError("png: the frame must be a tensor on a HIP device (there is no CPU path)")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] not in (1, 3) or not frame.is_contiguous():
        raise ValueError(f"png: the frame must be a contiguous uint8 [H, W, 3] or [H, W, 1], got {frame.dtype} {tuple(frame.shape)}")
    H, W, ch = (int(s) for s in frame.shape)
    if H < 1 or W < 1:
        raise ValueError(f"png: a frame of {H} x {W} has no pixel")
    return H, W, ch


def _png_params(filter="adaptive", stripe_rows=None, width: int = 1, channels: int = 3):
    """(UMHS_PNG_FILTER_*, stripe_rows) or ValueError; ``stripe_rows=None``: ``png_default_stripe_rows(width, channels)``."""
    if str(filter) not in PNG_FILTERS:
        raise ValueError(f"png: filter must be one of {', '.join(PNG_FILTERS)}, got {filter!r}")
    if int(channels) not in (1, 3):
        raise ValueError(f"png: channels must be 3 (RGB) or 1 (grey), got {channels}")
    stripe_rows = png_default_stripe_rows(width, channels) if stripe_rows is None else int(stripe_rows)
    if not 1 <= stripe_rows <= 65535:
        raise ValueError(f"png: stripe_rows must be 1..65535, got {stripe_rows}")
    return PNG_FILTERS[str(filter)], stripe_rows


def png_workspace_bytes(height: int, width: int, channels: int = 3, stripe_rows=None) -> int:
    _, s = _png_params("adaptive", stripe_rows, width, channels)
    return int(_hip.lib().umhs_png_workspace_bytes(int(height), int(width), int(channels), s))


def png_max_bytes(height: int, width: int, channels: int = 3, stripe_rows=None) -> int:
    """An upper bound on the length of the file for ANY content of the frame (0: the frame is outside what the encoder takes)."""
    _, s = _png_params("adaptive", stripe_rows, width, channels)
    return int(_hip.lib().umhs_png_max_bytes(int(height), int(width), int(channels), s))


def png_filter(frame, filter="adaptive"):
    """The filter stage of the frame encoder (umhs_png_filter): uint8 [H, W, C] at any byte address -> uint8 [H, 1 + W * C], every row's
    filter type and its filtered bytes.  One launch, no sync."""
    H, W, ch = _png_frame(frame)
    f, _ = _png_params(filter, 1, W, ch)
    if H > 65535 or W > 65535:
        raise ValueError(f"png: a frame of {H} x {W} is outside 1..65535")
    out = torch.empty(H, 1 + W * ch, dtype=torch.uint8, device=frame.device)
    _hip.check(_hip.lib().umhs_png_filter(C.c_void_p(frame.data_ptr()), H, W, ch, f, C.c_void_p(out.data_ptr()), _hip.stream()),
               "umhs_png_filter")
    return out


def _png_out(out, length, dev, capacity):
    if out is None:
        out = torch.empty(int(capacity), dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"png: out must be a contiguous uint8 vector on {dev}")
    if length is None:
        length = torch.empty(1, dtype=torch.int64, device=dev)
    elif not torch.is_tensor(length) or length.dtype != torch.int64 or length.numel() != 1 or length.device != dev:
        raise ValueError(f"png: length must be one int64 on {dev}")
    return out, length


def _png_workspace(workspace, need, dev):
    if workspace is None:
        from .workspace import _workspace

        return _workspace(need, dev, WS_PNG)
    if (not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != dev
            or not workspace.is_contiguous()):
        raise ValueError(f"png: the workspace must be at least {need} contiguous uint8 on {dev}")
    return workspace


def png_encode(frame, filter="adaptive", stripe_rows=None, out=None, length=None, workspace=None):
    """One PNG file of ``frame`` (uint8 [H, W, 3] or [H, W, 1] on the device, any byte address), filtered and deflated on the device
    (umhs_png_encode) -> (out uint8 [capacity], length int64 [1]), both on the device: the file is ``out[:length]``.  ``filter``:
    ``adaptive`` (per row, least sum of absolute differences) or one of none / sub / up / average / paeth for every row.
    ``stripe_rows``: rows per independent piece (one workgroup, one IDAT chunk; default ``png_default_stripe_rows``).  ``out``: the
    buffer to fill (its size is the capacity; default: ``png_max_bytes``, which no content exceeds); when the file is longer than the
    capacity, nothing is written past it and ``length`` holds the size needed.  ``workspace``: uint8 of at least
    ``png_workspace_bytes`` (default: the registry's ``png_encode`` slot).  Five launches on the current stream, no sync."""
    H, W, ch = _png_frame(frame)
    f, s = _png_params(filter, stripe_rows, W, ch)
    lib, dev = _hip.lib(), frame.device
    need = int(lib.umhs_png_workspace_bytes(H, W, ch, s))
    if need == 0:
        raise ValueError(f"png: a frame of {H} x {W} in pieces of {s} rows is outside what the encoder takes (sizes 1..65535, a piece "
                         "below 2^31 bytes)")
    workspace = _png_workspace(workspace, need, dev)
    out, length = _png_out(out, length, dev, lib.umhs_png_max_bytes(H, W, ch, s))
    _hip.check(lib.umhs_png_encode(C.c_void_p(frame.data_ptr()), H, W, ch, f, s, C.c_void_p(out.data_ptr()), out.numel(),
                                   C.c_void_p(length.data_ptr()), C.c_void_p(workspace.data_ptr()), workspace.numel(), _hip.stream()),
               "umhs_png_encode")
    return out, length


def png_deflate(filtered, width: int, channels: int = 3, stripe_rows=None, out=None, length=None, workspace=None):
    """Stage B and the container alone (umhs_png_deflate) on given filtered rows, uint8 [H, 1 + width * channels] as ``png_filter``
    lays them out (the type bytes are taken as they are) -> (out, length) as ``png_encode``."""
    W, ch = int(width), int(channels)
    _, s = _png_params("adaptive", stripe_rows, W, ch)
    if (not torch.is_tensor(filtered) or not filtered.is_cuda or filtered.dtype != torch.uint8 or filtered.dim() != 2
            or not filtered.is_contiguous() or W < 1 or filtered.shape[1] != 1 + W * ch or filtered.shape[0] < 1):
        raise ValueError(f"png: the filtered rows of a frame {W} wide are a contiguous uint8 [H, {1 + W * ch}] on a HIP device "
                         "(there is no CPU path)")
    lib, dev, H = _hip.lib(), filtered.device, int(filtered.shape[0])
    need = int(lib.umhs_png_workspace_bytes(H, W, ch, s))
    if need == 0:
        raise ValueError(f"png: a frame of {H} x {W} in pieces of {s} rows is outside what the encoder takes")
    workspace = _png_workspace(workspace, need, dev)
    out, length = _png_out(out, length, dev, lib.umhs_png_max_bytes(H, W, ch, s))
    _hip.check(lib.umhs_png_deflate(C.c_void_p(filtered.data_ptr()), H, W, ch, s, C.c_void_p(out.data_ptr()), out.numel(),
                                    C.c_void_p(length.data_ptr()), C.c_void_p(workspace.data_ptr()), workspace.numel(), _hip.stream()),
               "umhs_png_deflate")
    return out, length
