"""Hyperspectral frames (mirror of ``umhsnerf/data/utils/hs_dataloader.py``): ``hyperspectral_file_path`` points to an
``.npy`` cube H x W x B; values are converted to float32 and clamped to [0, 1] (``:49-50``).  The VCA endmember
initialisation the reference triggers from here (``:52-58``) runs on the resident stack instead: ``vca.vca_endmembers`` /
``ResidentSplit.vca_endmembers``, handed to the field by the pipeline when ``load_vca`` is set.

Masks (``DataparserOutputs.mask_filenames``, one per frame): one channel of the frame's H x W, a pixel is usable iff its value is
non-zero; the stack ``mask`` [n,H,W] uint8 is what the sampler's lists are built from (``ops.mask_lists``).  With ``mask_color`` set
the RGB of the pixels outside the mask is replaced by it at load, as nerfstudio's ``InputDataset.get_data`` does  [upstream-recalled];
``hs_image`` is never touched.

Material labels (``metadata["seg_filenames"]``, one per frame: the reference's ``seg_image``, ``:60-64``): one channel of the frame's
H x W, integers of 0..255 kept as uint8; the stack ``seg`` [n,H,W] is what evaluation scores the model's ``seg_raw`` against
(``ops.seg_confusion``, utils/seg_metrics.py).  ``seg_num_labels`` = the largest label other than ``seg_ignore_label``, plus one;
more than ``MAX_SEG_LABELS`` is refused at load (the table the kernel keeps per workgroup has that many columns)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch


def load_hs_image(path) -> torch.Tensor:
    cube = np.load(path)  # H, W, B
    if cube.ndim != 3:
        raise ValueError(f"{path}: expected an H x W x B cube, got shape {cube.shape}")
    return torch.from_numpy(np.ascontiguousarray(cube)).float().clamp(0, 1)


def load_image(path) -> torch.Tensor:
    """RGB(A) frame as float32 in [0,1] (InputDataset.get_image_float32); ``.npy`` or anything PIL opens."""
    path = str(path)
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        from PIL import Image

        arr = np.array(Image.open(path))
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, axis=2)
    if arr.dtype == np.uint8:
        return torch.from_numpy(arr.astype(np.float32) / 255.0)
    return torch.from_numpy(arr.astype(np.float32))


def load_mask(path) -> torch.Tensor:
    """One frame's mask as uint8 [H,W], a pixel usable iff non-zero; ``.npy`` or anything PIL opens.  Exactly one channel: a mask with a
    channel axis is a ``ValueError``.  uint8 values are kept (255, 1 and 7 all count); any other type becomes 0 / 1 by ``!= 0``."""
    path = str(path)
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        from PIL import Image

        arr = np.array(Image.open(path))
    if arr.ndim != 2:
        raise ValueError(f"{path}: a mask holds exactly one channel (H x W), got shape {arr.shape}")
    if arr.dtype != np.uint8:
        arr = (arr != 0).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(arr))


MAX_SEG_LABELS = 32  # columns of umhs_seg_confusion's table


def load_seg(path) -> torch.Tensor:
    """One frame's material labels as uint8 [H,W]; ``.npy`` or anything PIL opens.  Exactly one channel, an integer (or bool) type and
    values of 0..255: anything else is a ``ValueError`` that names the file -- a label is an identity, never rounded or wrapped."""
    path = str(path)
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        from PIL import Image

        arr = np.array(Image.open(path))
    if arr.ndim != 2:
        raise ValueError(f"{path}: a label image holds exactly one channel (H x W), got shape {arr.shape}")
    if arr.dtype != np.bool_ and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{path}: labels must be integers, got {arr.dtype}")
    if arr.size and (int(arr.min()) < 0 or int(arr.max()) > 255):
        raise ValueError(f"{path}: labels must lie in 0..255, got {int(arr.min())}..{int(arr.max())}")
    return torch.from_numpy(np.ascontiguousarray(arr.astype(np.uint8)))


def seg_num_labels(seg: torch.Tensor, ignore_label: int = 255) -> int:
    """The largest label of ``seg`` other than ``ignore_label``, plus one (0: every pixel is ignored)."""
    present = torch.bincount(seg.reshape(-1).long().cpu(), minlength=256) > 0
    if 0 <= int(ignore_label) < 256:
        present[int(ignore_label)] = False
    idx = torch.nonzero(present)
    return int(idx.max()) + 1 if idx.numel() else 0


def apply_mask_color(image: torch.Tensor, mask: torch.Tensor, mask_color) -> torch.Tensor:
    """``image`` [n,H,W,3] with the pixels OUTSIDE ``mask`` [n,H,W] (value 0) set to ``mask_color`` (three floats in [0,1])."""
    if image.shape[-1] != 3:
        raise ValueError(f"mask_color needs an RGB stack, got {image.shape[-1]} channels (an alpha channel has no masked colour)")
    color = torch.as_tensor([float(v) for v in mask_color], dtype=image.dtype, device=image.device)
    if color.shape != (3,):
        raise ValueError(f"mask_color must hold 3 values, got {tuple(mask_color)}")
    return torch.where((mask != 0)[..., None], image, color.expand_as(image)).contiguous()


def stack_frames(frames: Sequence[torch.Tensor]) -> torch.Tensor:
    """[n,H,W,K] contiguous stack -- the layout ``umhs_pixel_gather`` reads (one K-float row per pixel)."""
    shapes = {tuple(f.shape) for f in frames}
    if len(shapes) != 1:
        raise ValueError(f"frames differ in shape: {sorted(shapes)} (the resident stack needs one H x W x K)")
    return torch.stack(list(frames)).contiguous()


class HyperspectralDataset:
    """image + hs_image per frame, read once and kept (``--images-on-gpu``)."""

    def __init__(self, outputs, device="cpu"):
        if not outputs.metadata.get("hs_filenames"):
            raise AssertionError("hs_filenames missing: every frame needs hyperspectral_file_path")
        self.outputs, self.cameras, self.metadata = outputs, outputs.cameras, outputs.metadata
        self.image = stack_frames([load_image(p) for p in outputs.image_filenames]).to(device)
        self.hs_image = stack_frames([load_hs_image(p) for p in outputs.metadata["hs_filenames"]]).to(device)
        if self.image.shape[:3] != self.hs_image.shape[:3]:
            raise ValueError(f"image {tuple(self.image.shape)} and hs_image {tuple(self.hs_image.shape)} differ in n/H/W")
        self.mask = None  # [n,H,W] uint8, or None: a scene without mask_path
        mask_filenames = getattr(outputs, "mask_filenames", None)
        if mask_filenames:
            masks = [load_mask(p) for p in mask_filenames]
            for p, m in zip(mask_filenames, masks):
                if tuple(m.shape) != tuple(self.image.shape[1:3]):
                    raise ValueError(f"{p}: mask is {tuple(m.shape)}, the frames are {tuple(self.image.shape[1:3])}")
            if len(masks) != len(self):
                raise ValueError(f"{len(masks)} masks for {len(self)} frames")
            self.mask = torch.stack(masks).contiguous().to(device)
            if outputs.metadata.get("mask_color") is not None:
                self.image = apply_mask_color(self.image, self.mask, outputs.metadata["mask_color"])
        self.seg, self.seg_num_labels = None, 0  # [n,H,W] uint8, or None: a scene without seg_file_path
        seg_filenames = outputs.metadata.get("seg_filenames")
        if seg_filenames:
            if len(seg_filenames) != len(self):
                raise ValueError(f"{len(seg_filenames)} label images for {len(self)} frames")
            ignore = int(outputs.metadata.get("seg_ignore_label", 255))
            segs = []
            for p in seg_filenames:
                s = load_seg(p)
                if tuple(s.shape) != tuple(self.image.shape[1:3]):
                    raise ValueError(f"{p}: label image is {tuple(s.shape)}, the frames are {tuple(self.image.shape[1:3])}")
                if seg_num_labels(s, ignore) > MAX_SEG_LABELS:
                    raise ValueError(f"{p}: label {seg_num_labels(s, ignore) - 1} exceeds the {MAX_SEG_LABELS} labels (0..{MAX_SEG_LABELS - 1}) "
                                     f"that can be scored; ignore label {ignore}")
                segs.append(s)
            self.seg = torch.stack(segs).contiguous().to(device)
            self.seg_num_labels = seg_num_labels(self.seg, ignore)

    def __len__(self) -> int:
        return self.image.shape[0]

    def __getitem__(self, i: int):
        return {"image_idx": i, "image": self.image[i], "hs_image": self.hs_image[i]}
