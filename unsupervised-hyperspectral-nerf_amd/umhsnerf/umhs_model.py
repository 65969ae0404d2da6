"""UMHSModel -- mirror of the reference's ``umhsnerf/umhs_model.py`` (``UMHSConfig`` :61-119, ``UMHSModel`` :122-620)
driving the HIP hot path: field -> packed transmittance/compositing over all bands -> spectrum->sRGB -> losses.

Output keys, shapes, loss weights and callbacks follow the reference.  What differs by design:
  * the four per-stream renderer calls of ``get_outputs`` (:270-304) are ONE compositing launch;
  * ``scale_gradients_by_distance_squared`` (:241-242) is applied inside the compositing backward;
  * nerfacc's CUDA occupancy marcher does not exist on ROCm: ``get_outputs`` samples through the HIP marcher
    (``sampler.OccGridEstimator`` / ``VolumetricSampler``); ``get_outputs_from_samples`` takes any packed samples (this is
    what the benchmark and the parity tests feed).
"""
from __future__ import annotations

from collections import namedtuple
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Literal, Optional, Tuple, Type, Union

import numpy as np
import torch
from torch import Tensor, nn

from . import _hip, knobs, ops
from ._ns_compat import FieldHeadNames, ModelBase, ModelConfigBase, RayBundle, RaySamples, TrainingCallback, TrainingCallbackLocation
from .optim import UMHSAdam
from .sampler import OccGridEstimator, VolumetricSampler
from .umhs_field import UMHSField
from .umhs_renderer import SpectralRenderer
from .library import LIBRARY_OUTPUTS
from .statistics import is_statistics_output, statistics_outputs
from .cluster import CLUSTER_OUTPUTS
from .unmix import is_unmix_output, unmix_outputs
from .sparse import is_sparse_output, sparse_outputs
from .continuum import continuum_outputs, is_continuum_output
from .utils.clusterprobe import ClusterLookup
from .umhs_field_rgb import UMHSRGBField
from .utils.spec_to_rgb import ColourSystem

CLASS_COLORS = torch.tensor([
    [0.49, 0.29, 0.95], [0.29, 0.95, 0.30], [0.95, 0.29, 0.47], [0.29, 0.66, 0.95], [0.86, 0.95, 0.29],
    [0.85, 0.29, 0.95], [0.29, 0.95, 0.66], [0.95, 0.46, 0.29], [0.29, 0.30, 0.95], [0.50, 0.95, 0.29],
    [0.95, 0.29, 0.69], [0.29, 0.88, 0.95], [0.95, 0.82, 0.29], [0.63, 0.29, 0.95], [0.29, 0.95, 0.43],
])  # umhs_model.py:146-162


@dataclass
class UMHSConfig(ModelConfigBase):
    """``UMHSConfig(InstantNGPModelConfig)``, umhs_model.py:61-119: same names, same defaults (``method="rgb"``, :108, included: the
    reference's default method is NerfactoField's own colour head, served by umhs_field_rgb.py; every script of the reference but
    scripts/rgb.sh passes ``--pipeline.model.method rgb+spectral``, the path this package exists for).
    ``implementation`` keeps the reference's default ``"torch"`` (:104) and its ``"tcnn"`` (scripts/hotdog.sh:7): all values select the
    HIP kernels, whose arithmetic is the torch path's.  A nerfstudio ``ModelConfig`` when nerfstudio is importable
    -- not an ``InstantNGPModelConfig``, whose model would build tcnn / nerfacc modules first."""

    _target: Type = field(default_factory=lambda: UMHSModel)
    enable_collider: bool = False
    collider_params: Optional[Dict[str, float]] = field(default_factory=lambda: {"near_plane": 2.0, "far_plane": 6.0})
    grid_resolution: Union[int, List[int]] = 128
    grid_levels: int = 4
    max_res: int = 2048
    log2_hashmap_size: int = 19
    alpha_thre: float = 0.01
    cone_angle: float = 0.004
    render_step_size: Optional[float] = None
    near_plane: float = 0.05
    far_plane: float = 1e3
    use_gradient_scaling: bool = True
    use_appearance_embedding: bool = True
    # "last_sample" is what scripts/spectral.sh:6 passes; for the loss blend it is black (RGBRenderer.blend_background_for_loss_computation,
    # umhs_renderer.py:108-109), and this model's rgb is converter(spectral), never a renderer's last-sample composite
    background_color: Literal["random", "last_sample", "black", "white"] = "random"
    disable_scene_contraction: bool = False
    implementation: Literal["hip", "tcnn", "torch"] = "torch"
    method: Literal["rgb", "spectral", "rgb+spectral"] = "rgb"
    rgb_loss_weight: float = 1.0
    spectral_loss_weight: float = 1.0  # unused by the reference's loss too (hard-coded 5, umhs_model.py:369)
    temperature: float = 0.2
    pred_dino: bool = False
    pred_specular: bool = False
    load_vca: bool = False
    eval_num_rays_per_chunk: int = 512
    per_band_outputs: bool = True  # wv_i / residual_i / abundances_i views (umhs_model.py:273-304)
    compute_normals: bool = False  # a `normals` output outside training: the analytic density gradient (not in the reference)


class _LazyDict(dict):
    """A dict whose ``materialize()`` fills in the entries made on first access; anything that enumerates it sees them all."""

    def __iter__(self):
        return dict.__iter__(self.materialize())

    def __len__(self):
        return dict.__len__(self.materialize())

    def keys(self):
        return dict.keys(self.materialize())

    def items(self):
        return dict.items(self.materialize())

    def values(self):
        return dict.values(self.materialize())


class BandOutputs(_LazyDict):
    """Output dict whose per-band entries (``wv_i`` / ``residual_i`` / ``abundances_i``) are column views made on first access."""

    bands: Dict[str, Tensor] = {}

    def __missing__(self, key):
        stem, _, i = str(key).rpartition("_")
        src = self.bands.get(stem)
        if src is None or not i.isdigit() or int(i) >= src.shape[-1]:
            raise KeyError(key)
        v = self[key] = src[..., int(i)]
        return v

    def __contains__(self, key):
        if dict.__contains__(self, key):
            return True
        stem, _, i = str(key).rpartition("_")
        src = self.bands.get(stem)
        return src is not None and i.isdigit() and int(i) < src.shape[-1]

    def materialize(self) -> "BandOutputs":  # the full key set of the reference
        for stem, src in self.bands.items():
            for i in range(src.shape[-1]):
                self[f"{stem}_{i}"]
        return self


class LazyMetrics(_LazyDict):
    """Metrics dict whose entries are computed on first access.  nerfstudio's trainer reads the training metrics every
    ``steps_per_log`` steps only; the ~15 small reduction kernels behind them (1.4 % of a sampler-driven step) then run only when
    somebody looks.  The thunks hold the step's outputs / batch tensors, which nothing modifies in place afterwards."""

    def __init__(self, thunks: Dict[str, Callable[[], Tensor]]):
        super().__init__()
        self._thunks = dict(thunks)

    def __missing__(self, key):
        fn = self._thunks.pop(key, None)
        if fn is None:
            raise KeyError(key)
        v = self[key] = fn()
        return v

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._thunks

    def get(self, key, default=None):
        return self[key] if key in self else default

    def materialize(self) -> "LazyMetrics":
        for k in list(self._thunks):
            self[k]
        return self


# packed samples as the kernels take them: o, d [n,3] and t0, t1 [n] fp32, packed_info [R,2] (start, count), ray_indices [n] int64
_FlatSamples = namedtuple("_FlatSamples", "n o d t0 t1 packed_info ray_indices")


class _SidePrep:
    """Everything of a training step that depends on positions / parameters only -- the t_mid clip bounds, the weight pack images of
    the forward and the backward, the bucket histogram + scans of the hash-grid backward (~80 us of small launches) -- on a side
    stream, in the shadow of the two big forward kernels.  Issued in two waves: ``__init__`` right after positions_fwd,
    ``hash_prepare`` right after the hash features."""

    def __init__(self, side, spec, flat, n: int, t0, t1):
        dev = flat.device
        self.side, self.main, self.n = side, torch.cuda.current_stream(dev), n
        self.mm = torch.empty(2, device=dev, dtype=torch.float32)  # every allocation happens on the main stream
        self.can_partition = ops.reserve_step_workspaces(spec, n, dev)
        self.ev_ready, self.ev_done = torch.cuda.Event(), torch.cuda.Event()
        ev_in = torch.cuda.Event()
        ev_in.record(self.main)
        with torch.cuda.stream(side):
            side.wait_event(ev_in)
            ops.field_fwd_prepare(spec, flat)
            ops.tmid_minmax(t0, t1, out=self.mm)
            if self.can_partition and n > 0:
                ops.field_bwd_prepare(spec, flat, n)
            self.ev_ready.record(side)  # one event for all three: every cross-stream wait is a barrier packet (~5 us) on main

    def hash_prepare(self, pos01, spec, counted: bool) -> bool:
        """What is left of the hash-grid backward's prepare (the scans; with features from the sampler's cache the histogram too, a
        few workgroups per level) trickles along under everything up to the scatter pass, the first kernel that needs it (``ev_done``).
        The main stream then waits for the first wave.  -> whether the backward was prepared."""
        ev_hash = torch.cuda.Event()
        ev_hash.record(self.main)
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev_hash)
            if counted:
                prepared = ops.hashgrid_bwd_prepare_counted(pos01, spec.scalings, spec.layout.log2_hashmap_size)
            else:
                prepared = self.can_partition and self.n > 0 and ops.hashgrid_bwd_prepare(pos01, spec.scalings, spec.layout.log2_hashmap_size)
            self.ev_done.record(self.side)
        self.main.wait_event(self.ev_ready)
        return prepared


class UMHSModel(ModelBase):
    """UMHS model (``UMHSModel(NGPModel)``); built by ``config.setup(scene_box=, num_train_data=, metadata=, grad_scaler=,
    num_classes=, wavelengths=)`` exactly as the reference pipeline does (umhs_pipeline.py:98-105)."""

    def __init__(self, config: UMHSConfig, scene_box=None, num_train_data: int = 1, metadata: Optional[Dict] = None,
                 seed: Optional[int] = None, grad_scaler=None, num_classes: Optional[int] = None, wavelengths=None, **kwargs):
        nn.Module.__init__(self)  # nerfstudio's Model.__init__ would call populate_modules() before the fields below exist
        self.config = config
        self.scene_box, self.render_aabb, self.collider, self.callbacks = scene_box, None, None, None
        aabb = getattr(scene_box, "aabb", scene_box)
        self.scene_aabb_t = torch.as_tensor(aabb if aabb is not None else [[-1, -1, -1], [1, 1, 1]], dtype=torch.float32).reshape(2, 3)
        self.num_train_data = num_train_data
        self.grad_scaler = grad_scaler  # fp32 hot path: carried for interface parity, never used
        # the reference reads self.kwargs["metadata"]["wavelengths" | "num_classes"] (umhs_model.py:171-172,188-189); the two
        # explicit kwargs of its pipeline (:103-104) fill in what a metadata dict lacks
        self.kwargs = dict(metadata or {})
        if wavelengths is not None:
            self.kwargs.setdefault("wavelengths", wavelengths)
        if num_classes is not None:
            self.kwargs.setdefault("num_classes", num_classes)
        if self.kwargs.get("wavelengths") is None or "num_classes" not in self.kwargs:
            raise KeyError('metadata must carry "wavelengths" and "num_classes" (umhs_model.py:171-172,188-189)')
        self._seed = seed
        self._background_override = None  # background_color_override_context: the colour a cropped render is composited over
        self._material_edits = None  # material_edits_context: the materials.MaterialEdits a gradient-free render applies
        self._material_device = None  # ... and its (E'' [C,B], density gains [C]) on the model's device
        self._material_regions = None  # ... with regions: (HOST table [K,16], E'' [(K+1),C,B], d [(K+1),C], s [K+1]) of every layer
        self._normals_requested = False  # get_outputs_for_camera_ray_bundle(output_names=[.., "normals"]) and the exporter set it
        self._spectral_clusters = None  # spectral_clusters_context: the cluster.SpectralClusters
        self._scene_statistics = None  # scene_statistics_context: the keyword arguments of SceneStatistics.frame_outputs
        self._sparse_unmixer = None  # sparse_unmixing_context: the sparse.SparseUnmixer a camera render unmixes its spectral against
        self._unmixer = None  # unmixing_context: the unmix.Unmixer a camera render unmixes its spectral against
        self._continuum = None  # continuum_context: the continuum.ContinuumAnalysis a camera render divides its spectral's continuum out by
        self._spectral_library = None  # spectral_library_context: (library.SpectralLibrary, max_angle) a camera render matches against
        self.populate_modules()

    def populate_modules(self):
        c = self.config
        wl = self.kwargs["wavelengths"]
        self.step = 0
        self.register_buffer("class_colors", CLASS_COLORS.clone())
        if "spectral" in c.method:
            self.renderer_spectral = SpectralRenderer()
        self.converter = ColourSystem(bands=wl, cs="sRGB")
        if not c.use_appearance_embedding:
            # umhs_model.py:181: the reference's flag is inverted -- False is what switches its 32-d per-image embedding ON (no script
            # does); that input of the rgb / specular heads is not built here, and ignoring the flag would silently train another model
            raise NotImplementedError("use_appearance_embedding=False (= the reference's 32-d appearance embedding, umhs_model.py:181) is not supported")
        if c.method == "rgb":  # the reference's default method = NerfactoField's own colour head (umhs_field.py:280-294): umhs_field_rgb.py
            self.field = UMHSRGBField(aabb=self.scene_aabb_t, num_images=self.num_train_data, log2_hashmap_size=c.log2_hashmap_size,
                                      max_res=c.max_res, spatial_distortion=None if c.disable_scene_contraction else "linf",
                                      appearance_embedding_dim=0, seed=self._seed)
        else:
            self.field = self._spectral_field(c, wl)
        self.scene_aabb = nn.Parameter(self.scene_aabb_t.flatten(), requires_grad=False)
        if c.render_step_size is None:
            c.render_step_size = float(((self.scene_aabb_t[1] - self.scene_aabb_t[0]) ** 2).sum().sqrt() / 1000)
        # umhs_model.py:201-209: nerfacc.OccGridEstimator(roi_aabb, resolution, levels) + VolumetricSampler(grid, density_fn)
        self.occupancy_grid = OccGridEstimator(self.scene_aabb_t.flatten(), resolution=int(c.grid_resolution), levels=c.grid_levels)
        self.sampler = VolumetricSampler(self.occupancy_grid, density_fn=self.field.density_fn)
        self.cluster_probe = ClusterLookup(len(wl), self.kwargs["num_classes"])
        self.background_color = c.background_color

    def _spectral_field(self, c, wl) -> UMHSField:
        return UMHSField(
            aabb=self.scene_aabb_t, num_images=self.num_train_data, implementation=c.implementation,
            log2_hashmap_size=c.log2_hashmap_size, max_res=c.max_res,
            spatial_distortion=None if c.disable_scene_contraction else "linf",
            appearance_embedding_dim=0,  # the reference's inverted flag yields 0 with the default config (:181)
            method=c.method, wavelengths=len(wl) if "spectral" in c.method else 0, num_classes=self.kwargs["num_classes"],
            temperature=c.temperature, converter=self.converter, pred_dino=c.pred_dino, pred_specular=c.pred_specular,
            load_vca=c.load_vca, seed=self._seed,
            endmember_init=self.kwargs.get("vca_endmembers") if c.load_vca else None,  # (put there by UMHSPipeline from the train split)
        )

    @property
    def device(self):
        return self.field.flat.device

    def label_to_rgb(self, labels: Tensor) -> Tensor:
        return self.class_colors[labels.long().squeeze(-1)]

    # ---- optimisation surface --------------------------------------------------------------------
    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        return {"fields": [self.field.flat]}

    def make_optimizer(self, lr: float = 2e-2, eps: float = 1e-15, lr_final: Optional[float] = 1e-5, max_steps: int = 30000) -> UMHSAdam:
        L = self.field.layout
        off, shp = L.entries.get("endmembers", (0, ()))  # (method="rgb" has no endmembers: nothing to clamp)
        return UMHSAdam(self.get_param_groups()["fields"], lr=lr, eps=eps, clamp_range=(off, off + (int(np.prod(shp)) if shp else 0)),
                        lr_final=lr_final, max_steps=max_steps)

    def clamp_endmembers(self, step: int = 0) -> None:
        """AFTER_TRAIN_ITERATION callback of the reference (umhs_model.py:568-572); UMHSAdam already fuses it."""
        with torch.no_grad():
            self.field.endmembers[:] = self.field.endmembers.clamp(0, 1)

    def update_occupancy_grid(self, step: int) -> None:
        """BEFORE_TRAIN_ITERATION callback of the reference (umhs_model.py:549-554)."""
        self.step = step
        self.occupancy_grid.update_every_n_steps(step=step, occ_eval_fn=lambda x: self.field.density_fn(x) * self.config.render_step_size)

    def get_training_callbacks(self, training_callback_attributes=None) -> List[TrainingCallback]:
        """umhs_model.py:542-591: clamp_endmembers AFTER every iteration (spectral methods), update_occupancy_grid BEFORE."""
        callbacks = []
        if self.config.method != "rgb":
            callbacks.append(TrainingCallback(where_to_run=[TrainingCallbackLocation.AFTER_TRAIN_ITERATION], update_every_num_iters=1,
                                              func=self.clamp_endmembers))
        callbacks.append(TrainingCallback(where_to_run=[TrainingCallbackLocation.BEFORE_TRAIN_ITERATION], update_every_num_iters=1,
                                          func=self.update_occupancy_grid))
        return callbacks

    def update_to_step(self, step: int) -> None:
        """nerfstudio Model.update_to_step (called by load_pipeline, umhs_pipeline.py:167): nothing here depends on the step."""
        self.step = step

    # ---- forward -----------------------------------------------------------------------------------
    def get_outputs(self, ray_bundle: RayBundle) -> Dict[str, Tensor]:
        ray_samples, ray_indices = self.sample(ray_bundle)
        return self.get_outputs_from_samples(ray_samples, ray_indices, len(ray_bundle))

    def sample(self, ray_bundle: RayBundle):
        """The sampler call of umhs_model.py:229-237 (no-grad): packed ray samples + ray_indices."""
        c = self.config
        # The training forward gathers the survivors' hash features out of the encoding the sampler's density query produced for every
        # marched candidate (UMHS_REUSE_ENC=0: hashes them again; 0.07 ms per step slower at 3.5 M candidates / 0.9 M survivors).
        # Gradient-free rendering reuses them as well -- an eval image keeps nearly every marched candidate (21.1 -> 20.9 ms per 256x256
        # image, the heads kernel is what its time is made of).
        reuse = isinstance(self.sampler, VolumetricSampler) and knobs.reuse_enc() and (
            self.training or (not torch.is_grad_enabled() and knobs.render_per_ray()))
        self.field._enc_capture = {} if reuse else None
        try:
            ray_samples, ray_indices = self._sample(ray_bundle)
            cap = self.field._enc_capture
        finally:
            self.field._enc_capture = None
        keep = getattr(self.sampler.occupancy_grid, "last_keep_index", None) if reuse else None
        if reuse and keep is not None and "enc" in cap and keep.numel() == ray_indices.numel():
            # the sampler's density query encoded every marched candidate: the survivors' features are a row gather away
            ray_samples.metadata = {**(getattr(ray_samples, "metadata", None) or {}), "umhs_enc": (cap["enc"], keep)}
        pinfo = getattr(self.sampler, "last_packed_info", None)
        if pinfo is not None and pinfo.shape[0] == len(ray_bundle):  # (start, count) of every ray: the sampler has it already
            ray_samples.metadata = {**(getattr(ray_samples, "metadata", None) or {}), "umhs_packed_info": pinfo}
        return ray_samples, ray_indices

    def prefetch_sample(self, ray_bundle: RayBundle) -> bool:
        """Start the occupancy-grid march of a coming ``sample(ray_bundle)`` on the current stream (it depends on the rays and
        the grid only).  The trainer calls this one step ahead on a side stream; ``sample`` picks the result up."""
        c = self.config
        if not isinstance(self.sampler, VolumetricSampler):
            return False
        with torch.no_grad():
            self.sampler.prefetch(ray_bundle=ray_bundle, near_plane=c.near_plane, far_plane=c.far_plane,
                                  render_step_size=c.render_step_size, alpha_thre=c.alpha_thre, cone_angle=c.cone_angle)
        return True

    def occupancy_update_due(self, step: int) -> bool:
        """Will ``update_occupancy_grid(step)`` rewrite the grid (OccGridEstimator.update_every_n_steps, n=16)?"""
        return step % 16 == 0

    def _sample(self, ray_bundle: RayBundle):
        c = self.config
        with torch.no_grad():
            ray_samples, ray_indices = self.sampler(ray_bundle=ray_bundle, near_plane=c.near_plane, far_plane=c.far_plane,
                                                    render_step_size=c.render_step_size, alpha_thre=c.alpha_thre,
                                                    cone_angle=c.cone_angle)
        return ray_samples, ray_indices

    def forward(self, ray_bundle: RayBundle) -> Dict[str, Tensor]:
        return self.get_outputs(ray_bundle)

    @property
    def normals_on(self) -> bool:
        """Does a forward outside training add the ``normals`` output?  Never while training: there is no normal loss in this method,
        and no training path launches anything for it."""
        return (not self.training) and bool(self.config.compute_normals or self._normals_requested)

    def _with_normals(self, outputs, ray_samples, fo, weights, packed_info):
        """Add ``normals`` [R,3] in [0, 1] (include/umhs_hip.h, "Density-gradient normals", step 7) from the field's per-sample normals."""
        if ray_samples.frustums.origins.numel() == 0:
            n = torch.zeros(0, 3, device=packed_info.device)
        else:
            n = fo[FieldHeadNames.NORMALS] if fo is not None and FieldHeadNames.NORMALS in fo else self.field.get_normals(ray_samples)
        outputs["normals"] = ops.ray_normals(weights.detach(), n.reshape(-1, 3), packed_info)
        return outputs

    def get_outputs_from_samples(self, ray_samples: RaySamples, ray_indices: Tensor, num_rays: int,
                                 packed_info: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """Body of ``get_outputs`` after the sampler, umhs_model.py:239-327."""
        c = self.config
        fr = ray_samples.frustums
        s = self._flat_samples(ray_samples, ray_indices, num_rays, packed_info)
        packed_info = s.packed_info
        if self._material_edits is not None:
            self._check_material_edits()
        if (not torch.is_grad_enabled() and c.method != "rgb" and s.n > 0 and knobs.render_per_ray()
                and ops.field_heads_fwd_supported(self.field._spec())):
            return self._render_outputs_from_samples(ray_samples, s)
        if c.method == "rgb":
            return self._rgb_outputs_from_samples(ray_samples, packed_info)
        fo = self.field(ray_samples, compute_normals=True) if self.normals_on else self.field(ray_samples)
        values = [fo["spectral"]]
        if c.pred_specular:
            values += [fo["spectral2"].detach(), fo["specular"]]  # spectral2 carries no loss in the reference (:373-374)
        values.append(fo["abundances"])
        weights, accumulation, depth, *comp = ops.CompositeFn.apply(fo[FieldHeadNames.DENSITY], fr.starts, fr.ends, packed_info,
                                                                     bool(c.use_gradient_scaling), *values)
        mm = ops.tmid_minmax(fr.starts, fr.ends)  # DepthRenderer clips to the batch-wide [min, max] of t_mid
        spectral = comp[0]
        spec_for_rgb = spectral.detach() if c.method == "spectral" else spectral  # no_grad pseudo-rgb (:289-293)
        rgb, depth_c, seg_probs, seg_raw, seg_pred = ops.RayEpilogueFn.apply(
            spec_for_rgb, self.converter.transform_matrix, self.field.endmembers.detach(), accumulation, depth, mm,
            self.class_colors, 0.2)
        # what the reference renders under no_grad carries no gradient here either: the pseudo-rgb of method "spectral" (:289-291),
        # specular (:281-284) and abundances (:298-301) -- a loss a caller puts on them must not train the field through them
        if c.method == "spectral":
            rgb = rgb.detach()
        comp[-1] = comp[-1].detach()
        if c.pred_specular:
            comp[2] = comp[2].detach()
        outputs = self._assemble_outputs(accumulation, depth_c, comp, rgb, packed_info, seg_probs, seg_raw, seg_pred, weights)
        return self._with_normals(outputs, ray_samples, fo, weights, packed_info) if self.normals_on else outputs

    def _rgb_outputs_from_samples(self, ray_samples: RaySamples, packed_info: Tensor) -> Dict[str, Tensor]:
        """``method="rgb"`` (umhs_model.py:265-267): the field's colour composited per ray -> rgb, accumulation, depth.
        Deliberate deviation: the reference calls ``renderer_rgb(rgb=, weights=)`` WITHOUT ``ray_indices`` / ``num_rays`` on packed
        samples, which makes nerfstudio's RGBRenderer sum over ALL samples of the batch (one colour for every ray); this composites
        per ray, as the reference does for every other output.  Background: "random" leaves the colour unblended here (it is blended
        in the loss, ``blend_background_for_loss_computation``), "white" / "black" add ``bg (1 - accumulation)``, as RGBRenderer does."""
        c, fr = self.config, ray_samples.frustums
        if fr.origins.numel() == 0:  # no sample survived the march: every ray shows the background (and the step has a zero gradient)
            R, dev_ = packed_info.shape[0], packed_info.device
            zero = (self.field.flat[:1] * 0.0).sum() if torch.is_grad_enabled() else torch.zeros((), device=dev_)  # keeps loss.backward() legal
            acc = torch.zeros(R, 1, device=dev_) + zero
            rgb = torch.zeros(R, 3, device=dev_) + zero + self._rgb_background()
            out = {"accumulation": acc, "depth": torch.zeros(R, 1, device=dev_), "rgb": rgb, "num_samples_per_ray": packed_info[:, 1],
                   "weights": torch.zeros(0, 1, device=dev_)}
            return self._with_normals(out, ray_samples, None, out["weights"], packed_info) if self.normals_on else out
        fo = self.field(ray_samples, compute_normals=True) if self.normals_on else self.field(ray_samples)
        weights, accumulation, depth, rgb = ops.CompositeFn.apply(fo[FieldHeadNames.DENSITY], fr.starts, fr.ends, packed_info,
                                                                  bool(c.use_gradient_scaling), fo[FieldHeadNames.RGB])
        if self.background_color in ("white", "black") or self._background_override is not None:
            rgb = rgb + self._rgb_background() * (1.0 - accumulation)
        if not self.training:
            rgb = rgb.clamp(0.0, 1.0)
        tmid = (fr.starts + fr.ends) / 2  # DepthRenderer: expected depth (the compositing kernel's), clipped to the batch-wide [min, max] of t_mid
        depth_c = torch.minimum(torch.maximum(depth, tmid.min()), tmid.max()) if tmid.numel() else depth
        out = {"accumulation": accumulation, "depth": depth_c, "rgb": rgb, "num_samples_per_ray": packed_info[:, 1], "weights": weights}
        return self._with_normals(out, ray_samples, fo, weights, packed_info) if self.normals_on else out

    def _rgb_background(self):
        """What method ``rgb`` composites over: the override colour [3] of ``background_color_override_context`` while one is active,
        else the configured white (1.0) or black / random (0.0: random is blended in the loss)."""
        if self._background_override is not None:
            return self._background_override
        return 1.0 if self.background_color == "white" else 0.0

    def _render_outputs_from_samples(self, ray_samples, s: "_FlatSamples") -> Dict[str, Tensor]:
        """The same outputs without gradients (eval images, ``ns-render``): mlp_base -> transmittance weights -> heads with the per-ray
        sums formed inside the kernel -- an image's samples never exist as [N, bands] arrays (an eval chunk of 32 k rays
        x 529 samples x 31 bands x 3 streams is 6.4 GB written and read back otherwise)."""
        f = self.field
        spec, flat = f._spec(), f.flat.detach()
        wpos, pos01, sel = ops.positions_fwd(s.o, s.d, s.t0, s.t1, spec)
        enc, _ = self._encode(ray_samples, spec, flat, pos01)
        edits = self._material_edits
        regional = edits is not None and bool(edits.regions)
        if edits is None:
            _, weights, acc, depth, comp = self._split_forward(spec, flat, enc, sel, wpos, s, want_logits=False, pack_ready=False)
        elif regional:
            weights, acc, depth, comp, edited = self._regional_forward(spec, flat, enc, sel, wpos, s, edits)
        else:
            weights, acc, depth, comp, mix = self._edited_forward(spec, flat, enc, sel, wpos, s, edits)
        mm = ops.tmid_minmax(s.t0, s.t1)
        M = _hip.f32c(self.converter.transform_matrix)
        # (under an edit too: the UNEDITED composited spectrum against the model's own dictionary -- which of the original materials
        # is seen now; a recoloured dictionary does not move the labels)
        rgb, depth_c, seg_probs, seg_raw, seg_pred = ops.ray_epilogue_fwd(
            comp[0], M, f.endmembers.detach(), acc, depth, mm, _hip.f32c(self.class_colors), 0.2)
        if regional:  # (the per-segment sums are re-mixed layer by layer even where only the density is edited: one path)
            comp = edited + [comp[-1]]
            rgb = ops.ray_rgb_fwd(comp[0], M)
        elif edits is not None and edits.edits_dictionary:  # (density-only edits: the passes above already gave the edited image)
            comp = ops.material_remix(mix, comp[2] if self.config.pred_specular else None, self._material_device[0],
                                      edits.specular_gain) + [comp[-1]]
            rgb = ops.ray_rgb_fwd(comp[0], M)
        outputs = self._assemble_outputs(acc.view(-1, 1), depth_c, comp, rgb, s.packed_info, seg_probs, seg_raw, seg_pred, weights.view(-1, 1))
        if self.normals_on:  # one more launch on the enc / pos01 / wpos / sel already at hand, then the per-ray sum
            normal = ops.density_normals(spec, flat, pos01, wpos, sel, enc=enc)["normal"]
            outputs["normals"] = ops.ray_normals(weights, normal, s.packed_info)
        return outputs

    def _edited_forward(self, spec, flat, enc, sel, wpos, s: "_FlatSamples", edits):
        """``_split_forward`` of a render under material edits (include/umhs_hip.h, "Material edits") -> (weights, accumulation, depth,
        composites, mix [R,16]).  A density edit costs one more scan and one more heads pass: the abundances a sample's density factor
        is made of are those of the UNEDITED field, and they do not depend on the weights that pass is given (its per-ray sums are
        discarded).  The second heads pass runs with the model's own dictionary; ``mix`` is what the remix multiplies by the edited one."""
        fo = ops.field_base_fwd(spec, flat, enc, True, sel, pack_ready=False, rows16=True)
        sigma = fo["sigma"]
        if edits.edits_density:
            weights, _, _, _ = ops.composite_fwd(sigma, s.t0, s.t1, s.packed_info, [])
            ab = ops.field_heads_fwd(spec, flat, fo["base16"], wpos, s.d, weights, s.ray_indices, s.packed_info, want_logits=False,
                                     pack_ready=True, release=False, want_abundances=True)["abundances"]
            sigma = ops.material_sigma(sigma, ab, self._material_device[1], out=sigma)
        weights, acc, depth, _ = ops.composite_fwd(sigma, s.t0, s.t1, s.packed_info, [])
        ho = ops.field_heads_fwd(spec, flat, fo["base16"], wpos, s.d, weights, s.ray_indices, s.packed_info, want_logits=False,
                                 pack_ready=True, release=False, want_mix=True)
        return weights, acc, depth, ho["comp"] + [ho["comp_abundances"]], ho["mix"]

    def _regional_forward(self, spec, flat, enc, sel, wpos, s: "_FlatSamples", edits):
        """``_edited_forward`` of an edit with regions (include/umhs_hip.h, "Regional material edits") -> (weights, accumulation,
        depth, UNEDITED composites, edited [spectral(, spectral2, specular)]).  The transmittance scan keeps the real ray partition;
        the heads pass is handed the SEGMENT partition (runs of one ray's samples in one region) and returns its sums split by
        region in the same single pass; the per-ray unedited spectrum and abundances are their ordered sums."""
        table, E_all, d_all, s_all = self._material_regions
        region = ops.region_classify(wpos, table)
        fo = ops.field_base_fwd(spec, flat, enc, True, sel, pack_ready=False, rows16=True)
        sigma = fo["sigma"]
        if edits.edits_density:
            weights, _, _, _ = ops.composite_fwd(sigma, s.t0, s.t1, s.packed_info, [])
            ab = ops.field_heads_fwd(spec, flat, fo["base16"], wpos, s.d, weights, s.ray_indices, s.packed_info, want_logits=False,
                                     pack_ready=True, release=False, want_abundances=True)["abundances"]
            sigma = ops.material_sigma_regions(sigma, ab, region, d_all, out=sigma)
        weights, acc, depth, _ = ops.composite_fwd(sigma, s.t0, s.t1, s.packed_info, [])
        seg_of, seg_info, seg_layer, ray_seg, _ = ops.region_segments(region, s.ray_indices, s.packed_info)
        ho = ops.field_heads_fwd(spec, flat, fo["base16"], wpos, s.d, weights, seg_of, seg_info, want_logits=False, pack_ready=True,
                                 release=False, want_mix=True)
        spec_seg = ho["comp"][2] if self.config.pred_specular else None
        edited = ops.material_remix_regions(ho["mix"], spec_seg, seg_layer, ray_seg, E_all, s_all)
        # (what the epilogue and seg_* read: the unedited spectrum and the abundances; spectral2 / specular come from the remix)
        comp = [ops.segment_sum(ho["comp"][0], ray_seg), ops.segment_sum(ho["comp_abundances"], ray_seg)]
        return weights, acc, depth, comp, edited

    def _check_material_edits(self, forward: bool = True) -> None:
        """What an active material edit needs: of the model (checked when ``material_edits_context`` is entered) and, ``forward``, of
        the state a forward under it is made in."""
        if self.config.method == "rgb":
            raise NotImplementedError("material edits need a spectral method (spectral, rgb+spectral): method=\"rgb\" has no material "
                                      "dictionary to edit")
        if not knobs.render_per_ray() or not ops.field_heads_fwd_supported(self.field._spec()):
            raise NotImplementedError("material edits re-mix the per-ray sums of the per-ray render path, which is switched off "
                                      "(UMHS_RENDER_PER_RAY=0) or cannot serve this configuration")
        if forward and (self.training or torch.is_grad_enabled()):
            raise NotImplementedError("material edits are applied by the gradient-free render only: call model.eval() and render under "
                                      "torch.no_grad() (get_outputs_for_camera_ray_bundle does)")

    @contextmanager
    def material_edits_context(self, edits):
        """While active, every gradient-free render of this model applies ``edits`` (``materials.MaterialEdits``):
        ``spectral`` / ``spectral2`` / ``specular`` are mixed with the edited dictionary, ``rgb`` is their colour, and a density edit
        changes ``accumulation`` / ``depth`` / ``weights`` / ``abundances``; ``seg_*`` keep the model's own dictionary (which of the
        ORIGINAL materials is seen now) and ``normals`` sums the unedited field's per-sample normals under the edited weights.  The
        output keys are those of an unedited render.  ``None`` or an identity edit is the plain path, without one extra launch.
        The edited dictionary is formed from ``field.endmembers`` as they are when the context is entered.
        An edit with regions (boxes / spheres, each with an edit of its own that replaces the top level inside it) renders through
        ``_regional_forward``; one without takes the path it always took.
        Refused with NotImplementedError: ``method="rgb"`` and a switched-off per-ray render path, on entry; training mode and enabled
        gradients, by the forward that meets them (a command line enters the context before its render loop switches to eval and
        no_grad).  The previous state comes back on exit, an exception included."""
        if edits is not None and edits.is_identity:
            edits = None
        if edits is not None:
            self._check_material_edits(forward=False)
            E = self.field.endmembers
            if (edits.n_classes, edits.n_bands) != tuple(E.shape) or edits.pred_specular != bool(self.config.pred_specular):
                raise ValueError(f"material edits built for (C, B, pred_specular) = ({edits.n_classes}, {edits.n_bands}, "
                                 f"{edits.pred_specular}); the model has ({E.shape[0]}, {E.shape[1]}, {bool(self.config.pred_specular)})")
        # E'' and d on the device, once per context and not once per chunk (a 1280 x 720 frame is 29 chunks, and the small host-to-device
        # copies behind them cost more than the two launches of a recolour)
        device_side = None if edits is None else (edits.dictionary(self.field.endmembers), edits.density_gain(self.device))
        regions_side = None
        if edits is not None and edits.regions:
            regions_side = (edits.region_table(), edits.dictionaries(self.field.endmembers), edits.density_gains(self.device),
                            edits.specular_gains(self.device))
        previous = (self._material_edits, self._material_device, self._material_regions)
        self._material_edits, self._material_device, self._material_regions = edits, device_side, regions_side
        try:
            yield
        finally:
            self._material_edits, self._material_device, self._material_regions = previous

    def _flat_samples(self, ray_samples: RaySamples, ray_indices: Tensor, num_rays: int, packed_info: Optional[Tensor]) -> "_FlatSamples":
        fr = ray_samples.frustums
        n = fr.origins.numel() // 3
        if packed_info is None:
            packed_info = (getattr(ray_samples, "metadata", None) or {}).get("umhs_packed_info")
        if packed_info is None:
            packed_info = ops.pack_info(ray_indices, num_rays)
        ri = (ray_indices if ray_indices.dtype == torch.int64 else ray_indices.long()).contiguous()
        return _FlatSamples(n, _hip.f32c(fr.origins).view(n, 3), _hip.f32c(fr.directions).view(n, 3), _hip.f32c(fr.starts).view(-1),
                            _hip.f32c(fr.ends).view(-1), packed_info, ri)

    def _encode(self, ray_samples: RaySamples, spec, flat, pos01, count: bool = False) -> Tuple[Tensor, bool]:
        """Level-major hash features of the samples -> (enc, counted).  ``count``: take the bucket histogram of the hash-grid backward
        in the gather's launch when the shape has a partitioned backward (counted=True then)."""
        cached = (getattr(ray_samples, "metadata", None) or {}).get("umhs_enc")
        if cached is not None and cached[1].numel() == pos01.shape[0]:
            return ops.enc_gather(cached[0], cached[1]), False  # encoded once, by the sampler's density query (same positions, same table)
        L = spec.layout
        table = L.view(flat, "mlp_base.encoder.hash_table")
        # The gather kernel has every (sample, level) hashed and its vector ALU idle: the bucket histogram of the hash-grid backward
        # rides in the same launch (as a kernel of its own it cost 16 us of the step even hidden on the side stream).
        enc = ops.hashgrid_fwd_count(pos01, table, spec.scalings, L.log2_hashmap_size) if count else None
        if enc is not None:
            return enc, True
        return ops.hashgrid_fwd(pos01, table, spec.scalings, L.log2_hashmap_size, True), False

    def _split_forward(self, spec, flat, enc, sel, wpos, s: "_FlatSamples", want_logits: bool, pack_ready: bool):
        """mlp_base -> rendering weights (transmittance scan) -> heads, whose kernel forms the per-ray sums itself.
        ``pack_ready``: the forward's weight images come from field_fwd_prepare (training step) and the heads launch releases them;
        otherwise mlp_base builds them.  -> (fo with "emb" = the aligned [N,16] rows, weights, accumulation, depth, composites)"""
        fo = ops.field_base_fwd(spec, flat, enc, True, sel, pack_ready=pack_ready, rows16=True)
        fo["emb"] = fo["base16"]  # the aligned-row form feeds the heads kernel and the composited backward
        weights, acc, depth, _ = ops.composite_fwd(fo["sigma"], s.t0, s.t1, s.packed_info, [])
        ho = ops.field_heads_fwd(spec, flat, fo["emb"], wpos, s.d, weights, s.ray_indices, s.packed_info, want_logits=want_logits,
                                 pack_ready=True, release=pack_ready)
        fo["feat_logits"] = ho["feat_logits"]
        return fo, weights, acc, depth, ho["comp"] + [ho["comp_abundances"]]

    def _assemble_outputs(self, accumulation, depth_c, comp, rgb, packed_info, seg_probs, seg_raw, seg_pred, weights, lazy_bands=False):
        """The output dict of umhs_model.py:260-327 (same keys).  ``lazy_bands``: the per-band entries (``wv_i``, ``residual_i``,
        ``abundances_i``; 2B+C slicing ops per step in the reference) are created on first access instead of eagerly."""
        c = self.config
        spectral, abund = comp[0], comp[-1]
        outputs: Dict[str, Tensor] = BandOutputs() if lazy_bands else {}
        outputs.update({"accumulation": accumulation, "depth": depth_c, "spectral": spectral})
        if c.pred_specular:
            outputs["spectral2"], outputs["specular"] = comp[1], comp[2]
        outputs["rgb"] = rgb
        outputs["num_samples_per_ray"] = packed_info[:, 1]
        outputs["abundances"] = abund
        if c.per_band_outputs:
            if lazy_bands:
                outputs.bands = {"wv": spectral, "abundances": abund, **({"residual": comp[2]} if c.pred_specular else {})}
            else:
                for i in range(spectral.shape[-1]):
                    outputs[f"wv_{i}"] = spectral[..., i]
                if c.pred_specular:
                    for i in range(spectral.shape[-1]):
                        outputs[f"residual_{i}"] = comp[2][..., i]
                for i in range(abund.shape[-1]):
                    outputs[f"abundances_{i}"] = abund[:, i]
        outputs["seg_probs"], outputs["seg_raw"], outputs["seg_pred"] = seg_probs, seg_raw, seg_pred
        outputs["weights"] = weights
        return outputs

    # ---- training step without autograd -------------------------------------------------------------
    def direct_step_supported(self, batch) -> bool:
        if not self.field.use_grad_sink:
            return False
        sink = self.field._spec().grad_sink  # created on first use
        return (self.training and self.config.method in ("spectral", "rgb+spectral") and batch["image"].shape[-1] == 3
                and knobs.direct_step() and sink.owns_next_backward())

    def draw_training_background(self, batch: Dict) -> Optional[Tensor]:
        """The random background of this step's rgb loss (RGBRenderer.blend_background_for_loss_computation), drawn by the caller
        when it wants to fix the position of the draw in the generator's sequence (UMHSPipeline does, in front of its prefetch)."""
        if self.config.method != "rgb+spectral" or self.background_color != "random":
            return None
        return torch.rand_like(_hip.f32c(batch["image"].to(self.device)))

    def forward_backward_from_samples(self, ray_samples: RaySamples, ray_indices: Tensor, num_rays: int, batch: Dict,
                                      packed_info: Optional[Tensor] = None, background: Optional[Tensor] = None):
        """get_outputs (after the sampler) + get_loss_dict + backward of the summed loss, as one straight launch sequence with no
        autograd graph: the same kernels with the same arguments in the same order as the autograd path (which remains the general
        one), minus ~0.6 ms of host time per step.  Gradients land in the field's gradient sink (= ``field.flat.grad``).
        Returns (outputs, loss_dict); both are detached."""
        c, f = self.config, self.field
        spec, flat = f._spec(), f.flat.detach()
        n, o, d, t0, t1, packed_info, ri = s = self._flat_samples(ray_samples, ray_indices, num_rays, packed_info)
        # prepare: positions, then the gradient-independent launches on the side stream
        wpos, pos01, sel = ops.positions_fwd(o, d, t0, t1, spec)
        prep = _SidePrep(self._side_stream(), spec, flat, n, t0, t1)
        # encode
        enc, counted = self._encode(ray_samples, spec, flat, pos01, count=knobs.fused_count())
        prepared = prep.hash_prepare(pos01, spec, counted)
        # forward.  Above 32 bands the step runs without any per-sample [N,B] array: forward as two launches with the
        # rendering weights known in between, per-ray sums inside the heads kernel, the mixing product once per RAY; the value half of
        # the compositing backward folded into the field backward.  At 31 bands both forms take the same time (C2 0.82 ms), so the
        # per-sample form stays the default there.  UMHS_FUSED_BWD=0 / 1 forces either.
        knob = knobs.fused_bwd()
        folded = (n > 0 and knob is not False and (knob or spec.layout.wavelengths > 32) and ops.field_bwd_composited_supported(spec)
                  and ops.field_heads_fwd_supported(spec))
        if folded:
            fo, weights, acc, depth, comp = self._split_forward(spec, flat, enc, sel, wpos, s, want_logits=True, pack_ready=True)
        else:
            fo = ops.field_fwd(spec, flat, enc, True, wpos, d, sel, want_emb=True, pack_ready=True, want_logits=True)
            values = [fo["spectral"]] + ([fo["spectral2"], fo["specular"]] if c.pred_specular else []) + [fo["abundances"]]
        # tail: ray epilogue + both losses + their backward down to d_spectral / d_accumulation in one launch
        M = _hip.f32c(self.converter.transform_matrix)
        hs, image = _hip.f32c(batch["hs_image"].to(self.device)), _hip.f32c(batch["image"].to(self.device))
        both = c.method == "rgb+spectral"
        bg = (background if background is not None else torch.rand_like(image)) if (both and self.background_color == "random") else None
        w = (5.0, float(c.rgb_loss_weight)) if both else (1.0, 0.0)
        if not folded:
            weights, acc, depth, comp = ops.composite_fwd(fo["sigma"], t0, t1, packed_info, values)
        rgb, depth_c, seg_probs, seg_raw, seg_pred, losses, d_spec, d_acc = ops.ray_train_tail(
            comp[0], M, f.endmembers.detach(), acc, depth, prep.mm, _hip.f32c(self.class_colors), hs, image if both else None, bg, 0.2,
            w[0], w[1], both)
        # backward
        if folded:
            d_sigma = d_spectral_samples = None
            bwd_comp = dict(sigma=fo["sigma"], t0=t0, t1=t1, packed_info=packed_info, ray_indices=ri, weights=weights, d_comp=d_spec,
                            d_acc=d_acc, grad_scaling=bool(c.use_gradient_scaling))
        else:
            bwd_comp = None
            d_sigma, (d_spectral_samples,) = ops.composite_bwd(fo["sigma"], t0, t1, packed_info, weights, values[:1], [d_spec], [True], d_acc,
                                                               bool(c.use_gradient_scaling))
        left = ops.field_backward_into(spec, f.flat, pos01, sel, wpos, d, enc, fo["sigma_raw"], fo["emb"], d_sigma, d_spectral_samples, None,
                                       prepared=prepared, feat_logits=fo["feat_logits"], hash_ready=prep.ev_done, comp=bwd_comp)
        assert left is None  # direct_step_supported() guarantees the sink owned this backward
        outputs = self._assemble_outputs(acc.view(-1, 1), depth_c, comp, rgb, packed_info, seg_probs, seg_raw, seg_pred, weights.view(-1, 1),
                                         lazy_bands=True)
        loss_dict = {"spectral_loss": losses[0]}
        if both:
            loss_dict["rgb_loss"] = losses[1]
        return outputs, loss_dict

    def _side_stream(self):
        s = getattr(self, "_side", None)
        if s is None or s.device != self.device:
            s = self._side = torch.cuda.Stream(device=self.device)
        return s

    # ---- losses / metrics ----------------------------------------------------------------------------
    def blend_background_for_loss_computation(self, pred_image, pred_accumulation, gt_image, background: Optional[Tensor] = None):
        """nerfstudio RGBRenderer.blend_background_for_loss_computation as called at umhs_model.py:358-362 (``background``: a fixed
        draw of the random background instead of a fresh one -- parity tests)."""
        if self.background_color == "random":
            bg = background if background is not None else torch.rand_like(pred_image)
            pred_image = pred_image + bg * (1.0 - pred_accumulation)
        if gt_image.shape[-1] == 4:
            bgc = bg if self.background_color == "random" else torch.full_like(pred_image, 1.0 if self.background_color == "white" else 0.0)
            gt_image = gt_image[..., :3] * gt_image[..., 3:] + bgc * (1 - gt_image[..., 3:])
        return pred_image, gt_image

    def get_loss_dict(self, outputs, batch, metrics_dict=None, background: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """umhs_model.py:329-383: 5*MSE(spectral) + rgb_loss_weight*MSE(rgb blended with a random background).
        ``background`` (not in the reference): the [R,3] random-background draw, for callers that fix it (parity tests)."""
        loss_dict = {}
        image = batch["image"].to(self.device)
        m = self.config.method
        if m != "rgb" and image.shape[-1] == 3:  # fused path: both MSEs (+ random-background blend) in one launch
            hs = batch["hs_image"].to(self.device)
            if m == "spectral":
                loss_dict["spectral_loss"], _ = ops.LossFn.apply(outputs["spectral"], hs, None, None, None, None, 1.0, 0.0)
            else:
                bg = (background if background is not None else torch.rand_like(outputs["rgb"])) if self.background_color == "random" else None
                loss_dict["spectral_loss"], loss_dict["rgb_loss"] = ops.LossFn.apply(
                    outputs["spectral"], hs, outputs["rgb"], outputs["accumulation"], bg, image, 5.0, float(self.config.rgb_loss_weight))
            return loss_dict
        pred_rgb, gt_rgb = self.blend_background_for_loss_computation(outputs["rgb"], outputs["accumulation"], image, background)
        if m == "rgb":
            loss_dict["rgb_loss"] = torch.nn.functional.mse_loss(pred_rgb, gt_rgb)
        elif m == "spectral":
            loss_dict["spectral_loss"] = torch.nn.functional.mse_loss(outputs["spectral"], batch["hs_image"].to(self.device))
        else:
            loss_dict["spectral_loss"] = 5 * torch.nn.functional.mse_loss(outputs["spectral"], batch["hs_image"].to(self.device))
            loss_dict["rgb_loss"] = self.config.rgb_loss_weight * torch.nn.functional.mse_loss(pred_rgb, gt_rgb)
        return loss_dict

    @staticmethod
    def psnr(pred: Tensor, gt: Tensor) -> Tensor:
        return 10.0 * torch.log10(1.0 / torch.mean((pred - gt) ** 2))

    def get_metrics_dict(self, outputs, batch) -> Dict[str, Tensor]:
        """umhs_model.py:385-405.  Values stay device tensors (the reference's ``.item()`` calls would sync the stream)."""
        rgb, gt_rgb, nspr = outputs["rgb"].detach(), batch["image"].to(self.device)[..., :3], outputs["num_samples_per_ray"]
        md = {"psnr": lambda: self.psnr(rgb, gt_rgb), "rmse": lambda: torch.sqrt(torch.nn.functional.mse_loss(rgb, gt_rgb))}
        if "spectral" in self.config.method:
            spec, gt = outputs["spectral"].detach(), batch["hs_image"].to(self.device)
            md["psnr_spectral"] = lambda: self.psnr(spec, gt)
            md["rmse_spectral"] = lambda: torch.sqrt(torch.nn.functional.mse_loss(spec, gt))
        md["num_samples_per_batch"] = lambda: nspr.sum()
        lazy = LazyMetrics(md)
        return lazy if self.training else dict(lazy.materialize())

    @torch.no_grad()  # as nerfstudio's Model.get_outputs_for_camera_ray_bundle
    def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle: RayBundle, output_names=None) -> Dict[str, Tensor]:
        """umhs_model.py:593-620.  The reference walks the image in 512-ray chunks (its kernels are launch-bound there); here a
        chunk is ``max(eval_num_rays_per_chunk, 32768)`` rays, i.e. a 128x128 image or a quarter-megapixel strip is ONE fused
        inference launch per kernel, and outputs stay on the model device.  ``output_names`` (not in the reference): keep these keys
        only -- a camera-path render asks for the base tensors, so none of the 2B+C per-band views is concatenated per chunk.  Naming
        ``"normals"`` there (or ``config.compute_normals``) is what makes the model compute that output (``normals_on``)."""
        keep = None if output_names is None else set(output_names)
        requested, self._normals_requested = self._normals_requested, self._normals_requested or (keep is not None and "normals" in keep)
        match = self._spectral_library is not None and (keep is None or not keep.isdisjoint(LIBRARY_OUTPUTS))
        if match and self.training:
            raise NotImplementedError("library outputs belong to the gradient-free render only: call model.eval() before rendering under "
                                      "spectral_library_context")
        group = self._spectral_clusters is not None and (keep is None or not keep.isdisjoint(CLUSTER_OUTPUTS))
        if group and self.training:
            raise NotImplementedError("cluster outputs belong to the gradient-free render only: call model.eval() before rendering under "
                                      "spectral_clusters_context")
        project = self._scene_statistics is not None and (keep is None or any(is_statistics_output(k) for k in keep))
        if project:
            if self.training:
                raise NotImplementedError("statistics outputs belong to the gradient-free render only: call model.eval() before rendering "
                                          "under scene_statistics_context")
            offered = statistics_outputs(self._scene_statistics["components"])
            missing = [k for k in (keep or ()) if is_statistics_output(k) and k not in offered]
            if missing:
                raise ValueError(f"{', '.join(missing)}: the context keeps {self._scene_statistics['components']} components "
                                 "(pca_rgb needs 3): raise `components` (--pca-components)")
        unmix = self._unmixer is not None and (keep is None or any(is_unmix_output(k) for k in keep))
        if unmix:
            if self.training:
                raise NotImplementedError("unmixing outputs belong to the gradient-free render only: call model.eval() before rendering "
                                          "under unmixing_context")
            missing = [k for k in (keep or ()) if is_unmix_output(k) and k not in unmix_outputs(len(self._unmixer))]
            if missing:
                raise ValueError(f"{', '.join(missing)}: the context unmixes against {len(self._unmixer)} endmembers")
        sparse = self._sparse_unmixer is not None and (keep is None or any(is_sparse_output(k) for k in keep))
        if sparse:
            if self.training:
                raise NotImplementedError("sparse-unmixing outputs belong to the gradient-free render only: call model.eval() before "
                                          "rendering under sparse_unmixing_context")
            missing = [k for k in (keep or ()) if is_sparse_output(k) and k not in sparse_outputs(len(self._sparse_unmixer))]
            if missing:
                raise ValueError(f"{', '.join(missing)}: the context unmixes against {len(self._sparse_unmixer)} library entries")
        hull = self._continuum is not None and (keep is None or any(is_continuum_output(k) for k in keep))
        analysis, unnamed = self._continuum if hull else (None, None)
        if hull:
            if self.training:
                raise NotImplementedError("continuum outputs belong to the gradient-free render only: call model.eval() before rendering "
                                          "under continuum_context")
            offered = continuum_outputs(analysis.bands, len(analysis))
            missing = [k for k in (keep if keep is not None else unnamed or ()) if is_continuum_output(k) and k not in offered]
            if missing:
                raise ValueError(f"{', '.join(missing)}: the context has {analysis.bands} bands and {len(analysis)} features")
        try:
            outputs = self._camera_ray_bundle_outputs(
                camera_ray_bundle, keep if keep is None or not (match or project or unmix or sparse or hull or group) else keep | {"spectral", "accumulation"})
        finally:
            self._normals_requested = requested
        if hull:  # once, on the assembled frame (under material edits: the edited spectrum)
            outputs.update(analysis.frame_outputs(outputs["spectral"], outputs["accumulation"], keep if keep is not None else unnamed))
        if unmix:  # once, on the assembled frame (under material edits: the edited spectrum)
            outputs.update(self._unmixer.frame_outputs(outputs["spectral"], outputs["accumulation"]))
        if sparse:  # once, on the assembled frame (under material edits: the edited spectrum)
            outputs.update(self._sparse_unmixer.frame_outputs(outputs["spectral"], outputs["accumulation"]))
        if project:  # once, on the assembled frame (under material edits: the edited spectrum)
            s = self._scene_statistics
            outputs.update(s["stats"].frame_outputs(outputs["spectral"], outputs["accumulation"], s["components"], s["threshold"], s["floor"]))
        if match:  # once, on the assembled frame (under material edits: the edited spectrum)
            library, max_angle = self._spectral_library
            outputs.update(library.frame_outputs(outputs["spectral"], outputs["accumulation"], max_angle))
        if group:  # once, on the assembled frame (under material edits: the edited spectrum)
            outputs.update(self._spectral_clusters.frame_outputs(outputs["spectral"], outputs["accumulation"]))
        if (match or project or unmix or sparse or hull or group) and keep is not None:
            outputs = {k: v for k, v in outputs.items() if k in keep}
        return outputs

    @contextmanager
    def continuum_context(self, analysis, names=None):
        """While active, ``get_outputs_for_camera_ray_bundle`` adds the rendered ``spectral`` with its continuum -- the upper convex hull
        of the spectrum over wavelength -- divided out, and the absorption features of ``analysis`` (a ``continuum.ContinuumAnalysis`` on
        this model's wavelengths): ``cr`` [H,W,B] and ``cr_0`` .. ``cr_{B-1}`` [H,W,1]; per feature f ``feature_depth_<f>``,
        ``feature_center_<f>`` and ``feature_area_<f>`` [H,W,1] (on the hull of the feature's own window), and ``feature_depth`` [H,W,F].
        All are 0 where ``accumulation <= 0.5`` or the spectrum is not finite.  They are computed once per frame, by one launch of
        ``ops.continuum`` on the assembled ``spectral`` -- under ``material_edits_context`` that is the edited spectrum -- and only when
        ``output_names`` is None or names one of them; only the named ones are built (the [H,W,B] cube only when a ``cr`` name is among
        them), and a render whose ``output_names`` is None builds ``names`` (None: all of them); no other output changes.
        ``None`` leaves everything as it is.  Refused with NotImplementedError: ``method="rgb"`` (no spectrum), on entry; training
        mode, by the render that meets it.  ValueError: an analysis of another band count, on entry; ``cr_<b>`` with b >= B or
        ``feature_*_<f>`` with f >= F, by the render.  The previous state comes back on exit, an exception included."""
        if analysis is not None:
            if self.config.method == "rgb":
                raise NotImplementedError("continuum removal needs a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no "
                                          "spectrum")
            B = len(self.kwargs["wavelengths"])
            if analysis.bands != B:
                raise ValueError(f"the analysis is on {analysis.bands} wavelengths; the model has {B}")
        previous = self._continuum
        self._continuum = None if analysis is None else (analysis, None if names is None else tuple(names))
        try:
            yield
        finally:
            self._continuum = previous

    @contextmanager
    def unmixing_context(self, unmixer):
        """While active, ``get_outputs_for_camera_ray_bundle`` adds the classical linear unmixing of the rendered ``spectral`` against
        ``unmixer`` (an ``unmix.Unmixer`` on this model's wavelengths: the learnt endmembers, or entries of a spectral library):
        ``unmix_0`` .. ``unmix_{K-1}`` [H,W,1] and ``unmix`` [H,W,K], the abundances (a >= 0; FCLS: sum a = 1); ``unmix_raw`` [H,W,1],
        their argmax as float32 (-1 where ``accumulation <= 0.5`` or the spectrum is empty or not finite); ``unmix_pred`` [H,W,3], its
        colour; ``unmix_residual`` [H,W,1], the RMS misfit sqrt(|x - E^T a|^2 / B).  All are 0 where nothing is rendered.  They are
        computed once per frame, by one launch of ``ops.unmix`` on the assembled ``spectral`` -- under ``material_edits_context`` that is
        the edited spectrum -- and only when ``output_names`` is None or names one of them; no other output changes.  ``None`` leaves
        everything as it is.  Refused with NotImplementedError: ``method="rgb"`` (no spectrum to unmix), on entry; training mode, by the
        render that meets it.  ValueError: endmembers of another band count, on entry; ``unmix_k`` with k >= K, by the render.  The
        previous state comes back on exit, an exception included."""
        if unmixer is not None:
            if self.config.method == "rgb":
                raise NotImplementedError("unmixing needs a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no "
                                          "spectrum to unmix")
            B = len(self.kwargs["wavelengths"])
            if unmixer.bands != B:
                raise ValueError(f"the endmembers are on {unmixer.bands} wavelengths; the model has {B}")
        previous = self._unmixer
        self._unmixer = unmixer
        try:
            yield
        finally:
            self._unmixer = previous

    @contextmanager
    def sparse_unmixing_context(self, unmixer):
        """While active, ``get_outputs_for_camera_ray_bundle`` adds the sparse unmixing of the rendered ``spectral`` against the whole
        library of ``unmixer`` (a ``sparse.SparseUnmixer`` on this model's wavelengths): ``sparse_0`` .. ``sparse_{L-1}`` [H,W,1] and
        ``sparse`` [H,W,L], the abundances (a >= 0, most of them exactly 0); ``sparse_count`` [H,W,1], how many are > 0; ``sparse_raw``
        [H,W,1], the index of the largest as float32 (-1 where ``accumulation <= 0.5``, the spectrum is empty or not finite, or nothing
        is active); ``sparse_pred`` [H,W,3], that entry's library colour; ``sparse_residual`` [H,W,1], the RMS misfit
        sqrt(|x - A^T a|^2 / B).  All are 0 where nothing is rendered.  They are computed once per frame, by one launch of
        ``ops.sparse_unmix`` on the assembled ``spectral`` -- under ``material_edits_context`` that is the edited spectrum -- and only
        when ``output_names`` is None or names one of them; no other output changes.  ``None`` leaves everything as it is.  Refused
        with NotImplementedError: ``method="rgb"`` (no spectrum to unmix), on entry; training mode, by the render that meets it.
        ValueError: a library of another band count, on entry; ``sparse_k`` with k >= L, by the render.  The previous state comes back
        on exit, an exception included."""
        if unmixer is not None:
            if self.config.method == "rgb":
                raise NotImplementedError("sparse unmixing needs a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no "
                                          "spectrum to unmix")
            B = len(self.kwargs["wavelengths"])
            if unmixer.bands != B:
                raise ValueError(f"the library is on {unmixer.bands} wavelengths; the model has {B}")
        previous = self._sparse_unmixer
        self._sparse_unmixer = unmixer
        try:
            yield
        finally:
            self._sparse_unmixer = previous

    @contextmanager
    def scene_statistics_context(self, stats, components: int = 3, threshold: Optional[float] = None, floor: float = 1e-6):
        """While active, ``get_outputs_for_camera_ray_bundle`` adds what the scene's second-order statistics (``stats``, a
        ``statistics.SceneStatistics`` on this model's wavelengths) show in the rendered ``spectral``: ``rx_score`` [H,W,1], the squared
        Mahalanobis distance to the scene's mean (0 where ``accumulation <= 0.5``); ``rx_mask`` [H,W,1], 1.0 where it is above
        ``threshold`` (None: the chi-square quantile of B degrees of freedom at false-alarm rate 1e-3); ``pca_0`` .. ``pca_{components-1}``
        [H,W,1], the whitened principal components; ``pca_rgb`` [H,W,3] = clamp(0.5 + y_{0..2} / 6, 0, 1), black where nothing is
        rendered (it needs ``components >= 3``).  ``floor``: eigenvalues of the covariance are floored at ``floor`` x the largest.
        They are computed once per frame, by one launch of ``ops.spectral_project`` on the assembled ``spectral`` -- under
        ``material_edits_context`` that is the edited spectrum -- and only when ``output_names`` is None or names one of them; no other
        output changes.  ``None`` leaves everything as it is.  Refused with NotImplementedError: ``method="rgb"`` (no spectrum), on entry;
        training mode, by the render that meets it (the render itself runs without gradients).  ValueError: statistics of another band
        count, on entry; a name the context does not keep (``pca_k`` with k >= components, ``pca_rgb`` with fewer than 3), by the render.
        The previous state comes back on exit, an exception included."""
        if stats is not None:
            if self.config.method == "rgb":
                raise NotImplementedError("scene statistics need a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no "
                                          "spectrum to project")
            B = len(self.kwargs["wavelengths"])
            if stats.bands != B:
                raise ValueError(f"the statistics were taken on {stats.bands} wavelengths; the model has {B}")
            if not 0 <= int(components) <= B:
                raise ValueError(f"{components} components of {B} bands")
        previous = self._scene_statistics
        self._scene_statistics = None if stats is None else dict(stats=stats, components=int(components), threshold=threshold, floor=float(floor))
        try:
            yield
        finally:
            self._scene_statistics = previous

    @contextmanager
    def spectral_clusters_context(self, clusters):
        """While active, ``get_outputs_for_camera_ray_bundle`` adds, per pixel, the cluster of ``clusters`` (``cluster.SpectralClusters``,
        fitted on this model's wavelengths) nearest to the rendered ``spectral`` -- by spectral angle or by Euclidean distance, as they
        were fitted: ``cluster_raw`` [H,W,1] (the index as float32; -1 where ``accumulation <= 0.5`` or the spectrum is empty or not
        finite), ``cluster_pred`` [H,W,3] (the cluster's colour, black at -1) and ``cluster_score`` [H,W,1] (the cosine, or the squared
        distance; 0 at -1).  They are computed once per frame, by one launch of ``ops.cluster_step`` on the assembled ``spectral`` --
        under ``material_edits_context`` that is the edited spectrum -- and only when ``output_names`` is None or names one of them; no
        other output changes.  ``None`` leaves everything as it is.  Refused with NotImplementedError: ``method="rgb"`` (no spectrum
        to classify), on entry; training mode, by the render that meets it.  ValueError: clusters of another band count, on entry.
        The previous state comes back on exit, an exception included."""
        if clusters is not None:
            if self.config.method == "rgb":
                raise NotImplementedError("spectral clusters need a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no "
                                          "spectrum to classify")
            B = len(self.kwargs["wavelengths"])
            if clusters.bands != B:
                raise ValueError(f"the clusters were fitted on {clusters.bands} wavelengths; the model has {B}")
        previous = self._spectral_clusters
        self._spectral_clusters = clusters
        try:
            yield
        finally:
            self._spectral_clusters = previous

    @contextmanager
    def spectral_library_context(self, library, max_angle: Optional[float] = None, continuum_removed: bool = False):
        """While active, ``get_outputs_for_camera_ray_bundle`` adds, per pixel, the entry of ``library`` (``library.SpectralLibrary``,
        resampled onto this model's wavelengths) whose spectral angle to the rendered ``spectral`` is smallest: ``library_raw`` [H,W,1]
        (the index as float32; -1 where ``accumulation <= 0.5``, where the spectrum is empty or not finite, or where the angle is above
        ``max_angle``), ``library_pred`` [H,W,3] (the entry's colour, black at -1), ``library_angle`` [H,W,1] (radians) and
        ``library_margin`` [H,W,1] (how much further the runner-up is).  They are computed once per frame, by one launch of
        ``ops.library_match`` on the assembled ``spectral`` -- under ``material_edits_context`` that is the edited spectrum -- and only
        when ``output_names`` is None or names one of them; no other output changes.  ``None`` leaves everything as it is.
        A float32 cosine does not resolve angles below about 1e-3 rad: near-duplicate entries tie and the earlier one wins.
        ``continuum_removed``: match absorption shapes instead -- ``ops.continuum`` of the frame's ``spectral`` (one more launch and one
        [R,B] temporary per frame) against ``library.continuum_removed()``; without it nothing changes.
        Refused with NotImplementedError: ``method="rgb"`` (no spectrum to match), on entry; training mode, by the render that meets
        it.  The previous state comes back on exit, an exception included."""
        if library is not None:
            if self.config.method == "rgb":
                raise NotImplementedError("a spectral library needs a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no "
                                          "spectrum to match")
            B = len(self.kwargs["wavelengths"])
            if len(library.wavelengths) != B:
                raise ValueError(f"the library is resampled onto {len(library.wavelengths)} wavelengths; the model has {B}")
        previous = self._spectral_library
        self._spectral_library = None if library is None else (library.continuum_removed() if continuum_removed else library, max_angle)
        try:
            yield
        finally:
            self._spectral_library = previous

    def _camera_ray_bundle_outputs(self, camera_ray_bundle: RayBundle, keep) -> Dict[str, Tensor]:
        o = camera_ray_bundle.origins
        hw = o.shape[:-1]
        origins, directions = o.reshape(-1, 3).to(self.device), camera_ray_bundle.directions.reshape(-1, 3).to(self.device)
        nears, fars = camera_ray_bundle.nears, camera_ray_bundle.fars
        if nears is not None and fars is not None:  # a crop box: every chunk marches its own rays' [nears, fars]
            nears, fars = nears.reshape(-1, 1).to(self.device), fars.reshape(-1, 1).to(self.device)
        else:
            nears = fars = None
        # spectral methods under a background override: rgb needs the accumulation beside it, whether the caller keeps it or not
        over = self._background_override is not None and self.config.method != "rgb" and (keep is None or "rgb" in keep)
        need = keep if keep is None or not over else set(keep) | {"accumulation"}
        outs: Dict[str, List[Tensor]] = {}
        n, ch = origins.shape[0], max(int(self.config.eval_num_rays_per_chunk), 32768)
        for i in range(0, n, ch):
            rb = RayBundle(origins=origins[i:i + ch], directions=directions[i:i + ch])
            if nears is not None:
                rb.nears, rb.fars = nears[i:i + ch], fars[i:i + ch]
            for k, v in self.forward(rb).items():
                if isinstance(v, Tensor) and v.shape[:1] == (len(rb),) and (need is None or k in need):
                    outs.setdefault(k, []).append(v)
        outputs = {k: (v[0] if len(v) == 1 else torch.cat(v)).view(*hw, -1) for k, v in outs.items()}
        if over and "rgb" in outputs:
            outputs["rgb"] = outputs["rgb"] + self._background_override * (1.0 - outputs["accumulation"])
            if keep is not None and "accumulation" not in keep:
                del outputs["accumulation"]
        return outputs

    @contextmanager
    def background_color_override_context(self, color):
        """nerfstudio's ``background_color_override_context`` (``ns-render`` enters it with a crop's ``background_color``): while active,
        the ``rgb`` of ``get_outputs_for_camera_ray_bundle`` is composited over ``color`` [3] -- ``rgb + color (1 - accumulation)`` --
        instead of the configured background.  Method ``rgb``: ``color`` replaces its black / white where the field's colour is
        composited (``_rgb_background``).  The spectral methods, whose
        ``rgb`` is ``converter(spectral)`` with no background term in the reference, get the term added: a deliberate deviation
        (INTEGRATION.md), so that a cropped render is not an object floating in black whatever colour was picked.  No other output
        changes; ``None`` leaves everything as it is.  The previous state comes back on exit, an exception included."""
        previous = self._background_override
        self._background_override = None if color is None else torch.as_tensor(color, dtype=torch.float32).reshape(3).to(self.device)
        try:
            yield
        finally:
            self._background_override = previous

    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, Tensor]:
        """umhs_model.py:527-539: ``camera`` is anything with ``generate_rays(camera_indices=0, keep_shape=True)`` or a RayBundle.
        ``obb_box`` = (T, R, S), the box of ``export.obb_from_params``: only what lies inside it is rendered (the ray generator folds
        it into per-ray ``nears`` / ``fars``, floored at ``config.near_plane``)."""
        if isinstance(camera, RayBundle):
            rb = camera
        elif obb_box is None:
            rb = camera.generate_rays(camera_indices=0, keep_shape=True)
        else:
            rb = camera.generate_rays(camera_indices=0, keep_shape=True, obb_box=obb_box, near_floor=float(self.config.near_plane))
        return self.get_outputs_for_camera_ray_bundle(rb)

    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]):
        """umhs_model.py:407-512: psnr / ssim on rgb, psnr / ssim / sam / rmse on the spectral image; lpips is omitted (its
        pretrained weights cannot be fetched offline).  One host read at the end instead of one ``.item()`` per metric."""
        gt_rgb = batch["image"].to(self.device)
        if gt_rgb.shape[-1] == 4:  # renderer_rgb.blend_background: composite RGBA ground truth over the background colour
            bgv = 1.0 if self.background_color == "white" else 0.0
            gt_rgb = gt_rgb[..., :3] * gt_rgb[..., 3:] + bgv * (1 - gt_rgb[..., 3:])
        pred_rgb = outputs["rgb"]
        vals = {}
        sse, _, _ = ops.pixel_metrics(pred_rgb, gt_rgb)
        vals["psnr"] = 10.0 * torch.log10(pred_rgb.numel() / sse)
        vals["ssim"] = ops.ssim(gt_rgb, pred_rgb)
        if "spectral" in self.config.method:
            gt_s, pred_s = batch["hs_image"].to(self.device), outputs["spectral"]
            sse, sam, cnt = ops.pixel_metrics(pred_s, gt_s)
            mse = sse / pred_s.numel()
            vals["psnr_spectral"] = 10.0 * torch.log10(1.0 / mse)
            vals["ssim_spectral"] = ops.ssim(gt_s, pred_s)
            vals["sam_spectral"] = sam / cnt
            vals["rmse_spectral"] = torch.sqrt(mse)
        keys = list(vals)
        host = torch.stack([vals[k].double() for k in keys]).tolist()
        metrics_dict = dict(zip(keys, host))
        acc, depth = outputs["accumulation"], outputs["depth"]
        near, far = depth.min(), depth.max()
        images_dict = {"img": torch.cat([gt_rgb, pred_rgb], dim=1), "accumulation": acc.clamp(0, 1).expand(*acc.shape[:-1], 3),
                       "depth": ((depth - near) / (far - near + 1e-10)).clamp(0, 1).expand(*depth.shape[:-1], 3),
                       "se_per_pixel": ((gt_rgb - pred_rgb) ** 2).mean(dim=-1, keepdim=True)}
        return metrics_dict, images_dict

    @staticmethod
    def compute_sam(pred: Tensor, gt: Tensor, eps: float = 1e-8) -> Tensor:
        """umhs_model.py:514-525 (helper; mean spectral angle in radians, eps in the denominator)."""
        cos = (pred * gt).sum(dim=-1) / (torch.norm(pred, dim=-1) * torch.norm(gt, dim=-1) + eps)
        return torch.acos(torch.clamp(cos, -1, 1)).mean()
