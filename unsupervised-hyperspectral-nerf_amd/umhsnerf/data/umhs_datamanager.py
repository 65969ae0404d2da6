"""UMHSDataManager (mirror of ``umhsnerf/data/umhs_datamanager.py``) with the image stacks resident in HBM.

``next_train`` (``:95-108``) is: draw pixel indices, gather their rows from the image / hs_image stacks, generate the rays.
In the reference those are nerfstudio's PixelSampler, a fancy-index gather per key and ``Cameras.generate_rays``; here each
is one kernel of libumhs_hip.so (``umhs_pixel_indices`` / ``umhs_pixel_gather`` / ``umhs_raygen``, or ``umhs_raygen_distorted``
for cameras with lens distortion) on tensors that never leave the GPU.  The uniform draws come from ``torch.rand`` on the device
generator, so runs are seeded the same way.

A scene with a ``mask_path`` per frame trains only on the pixels its masks allow: the split compacts the set pixels of its mask stack
into lists once (``ops.mask_lists``), and ``umhs_pixel_indices_masked`` takes the place of ``umhs_pixel_indices`` -- same ``torch.rand``
block, same three launches, no host sync.  The draw is uniform over the set pixels of the split's whole mask stack, with replacement;
nerfstudio's sampler picks rows of ``nonzero(mask)`` with the host's Python RNG, without replacement  [upstream-recalled]."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Tuple, Type

import torch

from .. import ops
from .._ns_compat import InstantiateConfig, RayBundle
from .umhs_dataparser import Cameras, DataparserOutputs, UMHSDataParserConfig, save_dataparser_transform
from .utils.hs_dataloader import MAX_SEG_LABELS, HyperspectralDataset, seg_num_labels


@dataclass
class UMHSDataManagerConfig(InstantiateConfig):
    """``UMHSDataManagerConfig`` (umhs_datamanager.py:36-47): ``setup(device=, test_mode=, world_size=, local_rank=, num_classes=)``."""

    _target: Type = field(default_factory=lambda: UMHSDataManager)
    dataparser: Any = field(default_factory=UMHSDataParserConfig)
    train_num_rays_per_batch: int = 4096
    eval_num_rays_per_batch: int = 4096
    images_on_gpu: bool = True
    patch_size: int = 1
    ignore_mask: bool = False
    """nerfstudio's ``PixelSamplerConfig.ignore_mask``: the masks are loaded (and ``mask_color`` applied) but pixels are drawn everywhere."""


class _DatasetView:
    """What is read off ``datamanager.train_dataset`` / ``eval_dataset``: by the pipeline (umhs_pipeline.py:96-104: scene_box,
    metadata, len()) and by nerfstudio's Trainer / viewer before step 0 (``cameras``, ``dataset[i]["image"]``, ``image_filenames``:
    the viewer's init_scene draws the training cameras with their thumbnails)."""

    def __init__(self, split, scene_box, metadata, image_filenames=None):
        self._split, self.scene_box, self.metadata = split, scene_box, metadata
        self.image_filenames = list(image_filenames) if image_filenames is not None else [f"frame_{i:05d}" for i in range(len(split))]

    def __len__(self) -> int:
        return len(self._split)

    @property
    def cameras(self):
        return self._split.cameras

    def __getitem__(self, i: int) -> Dict:
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        item = {"image_idx": i, "image": self._split.image[i]}
        if item["image"].dtype == torch.uint8:
            item["image"] = item["image"].float() / 255.0
        if self._split.hs_image is not None:
            item["hs_image"] = self._split.hs_image[i]
        if self._split.mask is not None:
            item["mask"] = (self._split.mask[i] != 0)[..., None]
        if self._split.seg is not None:
            item["seg_image"] = self._split.seg[i]
        return item


class _ResidentOutputs:
    """``train_dataparser_outputs`` of a datamanager that was handed resident splits directly (tests, benchmarks): the metadata, and an
    identity world transform for the Trainer's ``save_dataparser_transform``."""

    def __init__(self, metadata):
        self.metadata, self.dataparser_scale = metadata, 1.0
        self.dataparser_transform = torch.eye(4)[:3]

    def save_dataparser_transform(self, path) -> None:
        save_dataparser_transform(self.dataparser_transform, self.dataparser_scale, path)


class ResidentSplit:
    """One split: cameras + contiguous [n,H,W,K] stacks -- on the device (``--images-on-gpu True``, scripts/hotdog.sh:8: the batch
    rows are gathered by ``umhs_pixel_gather``), or in host memory (``False``, scripts/pinecone.sh:14: the rows of a batch are indexed
    on the host, as the reference's dataloader does, and only they travel to the device).  ``mask`` [n,H,W] uint8 (or bool): the pixels
    ``sample`` may draw, those with a non-zero value.  The stack sits where the images sit; the lists the draw reads (``mask_off``
    [n+1] int64, ``mask_list`` [M] int32: 4 B per set pixel) always live on the device.  ``seg`` [n,H,W] uint8: ground-truth material
    labels (the reference's ``seg_image``), beside the images; they travel with whole eval frames only -- training batches never
    carry them -- and ``seg_num_labels`` (largest label other than ``seg_ignore_label``, plus one) is fixed once, when they are
    attached: ``ResidentSplit(...).with_seg(seg, ignore_label)`` (the constructor is called positionally, ``mask`` last)."""

    def __init__(self, cameras: Cameras, image: torch.Tensor, hs_image: Optional[torch.Tensor], device, on_gpu: bool = True, mask=None):
        self.device, self.on_gpu = torch.device(device), on_gpu
        self.cameras = cameras.to(device)
        self.c2w = self.cameras.camera_to_worlds.float().contiguous()
        self.intrinsics = self.cameras.intrinsics
        dist = self.cameras.distortion_params  # [n,6] on the device, or None: the undistorted kernel
        self.distortion = None if dist is None else dist.float().contiguous()
        place = (lambda t: t.to(device).contiguous()) if on_gpu else (lambda t: t.cpu().contiguous())
        self.image = place(image)
        self.hs_image = place(hs_image) if hs_image is not None else None
        n, h, w = self.image.shape[:3]
        if (h, w) != (cameras.height, cameras.width) or n != len(cameras):
            raise ValueError(f"stack {tuple(self.image.shape)} does not match {n} cameras of {cameras.height}x{cameras.width}")
        self.mask = self.mask_off = self.mask_list = None
        if mask is not None:
            if tuple(mask.shape) != (n, h, w) or mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError(f"mask must be uint8 or bool [{n}, {h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
            self.mask = place(mask.to(torch.uint8))
            self.mask_off, self.mask_list = ops.mask_lists(self.mask, device=self.device)
            if self.mask_list.numel() == 0:
                raise ValueError("the masks of this split leave no pixel to train on (every mask is all zero)")
        self.seg, self.seg_num_labels, self.seg_ignore_label = None, 0, 255

    def with_seg(self, seg: Optional[torch.Tensor], ignore_label: int = 255) -> "ResidentSplit":
        """Attaches the label stack [n,H,W] uint8 (``None``: a scene without labels) where the images sit; returns the split."""
        n, h, w = self.image.shape[:3]
        self.seg, self.seg_num_labels, self.seg_ignore_label = None, 0, int(ignore_label)
        if seg is not None:
            if tuple(seg.shape) != (n, h, w) or seg.dtype != torch.uint8:
                raise ValueError(f"seg must be uint8 [{n}, {h}, {w}], got {seg.dtype} {tuple(seg.shape)}")
            self.seg_num_labels = seg_num_labels(seg, self.seg_ignore_label)
            if self.seg_num_labels > MAX_SEG_LABELS:
                raise ValueError(f"label {self.seg_num_labels - 1} exceeds the {MAX_SEG_LABELS} labels that can be scored")
            self.seg = (seg.to(self.device) if self.on_gpu else seg.cpu()).contiguous()
        return self

    def __len__(self) -> int:
        return self.image.shape[0]

    def sample(self, num_rays: int, generator=None, ignore_mask: bool = False, want_batch: bool = True) -> Tuple[RayBundle, Optional[Dict]]:
        """``num_rays`` pixels drawn uniformly, with replacement: over the set pixels of the masks if the split has a mask (and
        ``ignore_mask`` is off), else over the whole stack.  Both draws consume the same ``torch.rand((num_rays, 3))`` block.
        ``want_batch=False``: the rays only, ``None`` for the batch -- no ground-truth row is gathered (the point-cloud export)."""
        n, h, w = self.image.shape[:3]
        u = torch.rand((num_rays, 3), device=self.device, generator=generator)
        if self.mask_list is not None and not ignore_mask:
            indices = ops.pixel_indices_masked(u, self.mask_off, self.mask_list, w)
        else:
            indices = ops.pixel_indices(u, n, h, w)
        return self.rays(indices), (self.batch(indices) if want_batch else None)

    def _rows(self, indices: torch.Tensor, stack: torch.Tensor) -> torch.Tensor:
        if self.on_gpu:
            return ops.pixel_gather(indices, stack)
        n, h, w = stack.shape[:3]
        i = indices.cpu()  # same clamping as umhs_pixel_gather (a uniform draw of exactly 1.0 rounds up to the extent)
        rows = stack[i[:, 0].clamp(0, n - 1), i[:, 1].clamp(0, h - 1), i[:, 2].clamp(0, w - 1)]
        rows = rows.float() / 255.0 if stack.dtype == torch.uint8 else rows.float()
        return rows.to(self.device, non_blocking=True)

    def vca_endmembers(self, num_classes: int, num_images: Optional[int] = 1, draws=None, seed: Optional[int] = 0):
        """VCA endmember initialisation from this split's ``hs_image`` stack (data.utils.vca) -> (endmembers [R,B] fp32, indices [R]
        into the flattened pixels of the frames used, info).  ``num_images=1``: frame 0, what the reference's dataset runs VCA on
        (hs_dataloader.py:52-58: the first frame it loads); ``None``: the whole stack.  A resident stack never leaves the GPU; a
        host-resident one (``images_on_gpu=False``) is uploaded one frame at a time."""
        from .utils.vca import vca_endmembers

        if self.hs_image is None:
            raise ValueError("this split has no hs_image stack to run VCA on")
        n = len(self) if num_images is None else int(num_images)
        if not 1 <= n <= len(self):
            raise ValueError(f"num_images {num_images} outside 1..{len(self)}")
        return vca_endmembers(self.hs_image[:n], num_classes, draws=draws, seed=seed, device=self.device)

    def batch(self, indices: torch.Tensor) -> Dict:
        b = {"image": self._rows(indices, self.image), "indices": indices}
        if self.hs_image is not None:
            b["hs_image"] = self._rows(indices, self.hs_image)
        return b

    def rays(self, indices: torch.Tensor) -> RayBundle:
        o, d, area, nrm = ops.raygen(indices, self.c2w, self.intrinsics, want_area=True, want_norm=True, distortion=self.distortion)
        return RayBundle(origins=o, directions=d, pixel_area=area, camera_indices=indices[:, :1].contiguous(),
                         metadata={"directions_norm": nrm})

    def image_rays(self, camera_index: int) -> RayBundle:
        """``cameras.generate_rays(camera_indices=i, keep_shape=True)``: one ray per pixel, [H,W,...]."""
        _, h, w = self.image.shape[:3]
        dev = self.device
        yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
        idx = torch.stack([torch.full_like(yy, camera_index), yy, xx], -1).reshape(-1, 3).contiguous()
        rb = self.rays(idx)
        return RayBundle(origins=rb.origins.view(h, w, 3), directions=rb.directions.view(h, w, 3), pixel_area=rb.pixel_area.view(h, w, 1),
                         camera_indices=rb.camera_indices.view(h, w, 1))

    def image_batch(self, i: int) -> Dict:
        """Frame ``i`` whole, on the device: what ``next_eval_image`` and ``eval_images`` hand out."""
        batch = {"image": self.image[i].to(self.device), "image_idx": i}
        if self.hs_image is not None:
            batch["hs_image"] = self.hs_image[i].to(self.device)
        if self.mask is not None:
            batch["mask"] = (self.mask[i] != 0)[..., None].to(self.device)  # [H,W,1] bool, as nerfstudio's datasets carry it
        if self.seg is not None:
            batch["seg_image"] = self.seg[i].to(self.device)  # [H,W] uint8
        return batch


class _EvalImages:
    """Every frame of a split exactly once, in order: ``(camera_ray_bundle [H,W,...], batch)`` for frames 0 .. n-1, and ``len()``.
    What nerfstudio's ``fixed_indices_eval_dataloader`` is to ``get_average_eval_image_metrics``  [upstream-recalled].  It reads the
    split only: neither the data manager's eval cursor nor its generator moves."""

    def __init__(self, split: ResidentSplit):
        self.split = split

    def __len__(self) -> int:
        return len(self.split)

    def __iter__(self):
        for i in range(len(self.split)):
            yield self.split.image_rays(i), self.split.image_batch(i)


class UMHSDataManager:
    """Train/eval splits of one scene, images on the GPU.  ``world_size``/``local_rank``: every rank keeps the full stacks
    and draws its own full per-rank batch from its own generator (seed + rank), as nerfstudio's data managers do."""

    def __init__(self, config: UMHSDataManagerConfig, device="cpu", test_mode: str = "val", world_size: int = 1, local_rank: int = 0,
                 num_classes: int = 5, seed: int = 42, train: Optional[ResidentSplit] = None, eval: Optional[ResidentSplit] = None,
                 metadata: Optional[Dict] = None, **kwargs):
        if config.patch_size != 1:
            raise NotImplementedError("patch_size > 1 (PatchPixelSampler) is not used by the reference's scripts")
        self.config, self.device, self.world_size, self.local_rank = config, torch.device(device), world_size, local_rank
        config.dataparser.num_classes = num_classes
        eval_names = None
        if train is None:
            parser = config.dataparser.setup()
            self.train_dataparser_outputs: DataparserOutputs = parser.get_dataparser_outputs("train")
            tr = HyperspectralDataset(self.train_dataparser_outputs)
            train = ResidentSplit(tr.cameras, tr.image, tr.hs_image, self.device, on_gpu=config.images_on_gpu, mask=tr.mask)
            train.with_seg(tr.seg, config.dataparser.seg_ignore_label)
            ev_out = parser.get_dataparser_outputs("val" if test_mode != "test" else "test")
            if len(ev_out.image_filenames):
                eval_names = ev_out.image_filenames
                ev = HyperspectralDataset(ev_out)
                eval = ResidentSplit(ev.cameras, ev.image, ev.hs_image, self.device, on_gpu=config.images_on_gpu, mask=ev.mask)
                eval.with_seg(ev.seg, config.dataparser.seg_ignore_label)
            metadata = self.train_dataparser_outputs.metadata
            self.scene_box = self.train_dataparser_outputs.scene_box
        self.train_split, self.eval_split, self.metadata = train, eval, metadata or {}
        names = getattr(getattr(self, "train_dataparser_outputs", None), "image_filenames", None)
        self.train_dataset = _DatasetView(train, getattr(self, "scene_box", None), self.metadata, names)
        self.eval_dataset = _DatasetView(eval, getattr(self, "scene_box", None), self.metadata, eval_names) if eval is not None else None
        if not hasattr(self, "train_dataparser_outputs"):  # resident splits handed in directly (tests): same attribute, no parser behind it
            self.train_dataparser_outputs = _ResidentOutputs(self.metadata)
        self.train_count = self.eval_count = 0
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(seed + local_rank)
        # the eval batches draw from a generator of their own: evaluating between two training steps leaves the training stream alone
        self.eval_generator = torch.Generator(device=self.device)
        self.eval_generator.manual_seed(seed + local_rank)
        self._eval_cursor = 0

    def to(self, device):  # the stacks were placed at construction (umhs_pipeline.py:94 calls datamanager.to(device))
        return self

    def get_param_groups(self) -> Dict:
        return {}

    def get_train_rays_per_batch(self) -> int:
        return self.config.train_num_rays_per_batch

    def get_eval_rays_per_batch(self) -> int:
        return self.config.eval_num_rays_per_batch

    def next_train(self, step: int) -> Tuple[RayBundle, Dict]:
        self.train_count += 1
        return self.train_split.sample(self.config.train_num_rays_per_batch, self.generator, ignore_mask=self.config.ignore_mask)

    def next_eval(self, step: int) -> Tuple[RayBundle, Dict]:
        self.eval_count += 1
        split = self.eval_split or self.train_split  # (the eval split's own mask)
        return split.sample(self.config.eval_num_rays_per_batch, self.eval_generator, ignore_mask=self.config.ignore_mask)

    def next_eval_image(self, step: int):
        split = self.eval_split or self.train_split
        i = self._eval_cursor % len(split)
        self._eval_cursor += 1
        return split.image_rays(i), split.image_batch(i)

    def sampling_state(self) -> Dict:
        """What a trainer's checkpoint needs to draw the same batches after a resume: both generators' states and the counters."""
        return {"generator": self.generator.get_state().cpu(), "eval_generator": self.eval_generator.get_state().cpu(),
                "train_count": self.train_count, "eval_count": self.eval_count, "eval_cursor": self._eval_cursor}

    def load_sampling_state(self, state: Dict) -> None:
        self.generator.set_state(state["generator"].cpu())
        self.eval_generator.set_state(state["eval_generator"].cpu())
        self.train_count, self.eval_count, self._eval_cursor = int(state["train_count"]), int(state["eval_count"]), int(state["eval_cursor"])

    def eval_images(self) -> _EvalImages:
        """The whole eval split (the train split if there is none, as ``next_eval_image``), each frame once and in order; sized."""
        return _EvalImages(self.eval_split or self.train_split)

    @property
    def fixed_indices_eval_dataloader(self) -> _EvalImages:  # the name nerfstudio's callers use
        return self.eval_images()
