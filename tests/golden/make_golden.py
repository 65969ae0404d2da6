#!/usr/bin/env python3
"""Generate the golden fixtures in this directory from the REFERENCE's own code.

Run in the build container only (needs /root/reference, which never travels):

    python tests/golden/make_golden.py              # everything below but G6 / G7
    python tests/golden/make_golden.py --only g8    # these fixtures only; the others are left as they are

What is pinned:
  G1  umhsnerf.utils.spec_to_rgb.ColourSystem      -- imported natively
  G2  umhsnerf.utils.clusterprobe.ClusterLookup    -- imported natively
  G3  umhsnerf.umhs_renderer.get_weights_spectral  -- imported under third-party stubs
  G4  umhsnerf.umhs_field.UMHSField.get_outputs / get_density -- executed UNMODIFIED on a
      hand-assembled instance under third-party stubs; the nerfstudio encoders / MLPs plugged into
      that instance are oracle/torch_ref.py's restatements (nerfstudio itself is not installable
      offline), so G4 pins the reference's glue arithmetic, shapes and autograd wiring -- NOT the
      third-party pieces (those stay "parity unpinned").
  G5  umhsnerf.umhs_renderer.SpectralRenderer.blend_background_for_loss_computation
  G6  umhsnerf.data.utils.vca (VCA endmember extraction)  -- written by make_golden_vca.py, not here
  G7  g7_endmembers_hotdog.npy: the endmember file the reference ships (data), read by G8 and the unmixing tests
  G8  umhsnerf.umhs_model.UMHSModel.get_outputs / get_loss_dict / get_metrics_dict -- executed
      UNMODIFIED on a hand-assembled instance (UMHSModel.__new__, attributes set by hand) under
      third-party stubs.  Its field is the G4 instance (the reference's own UMHSField), its
      SpectralRenderer / ColourSystem / ClusterLookup are the reference's own; the sampler returns a
      fixed packed batch; nerfacc's pack_info / render_weight_from_density, the depth / accumulation
      renderers, scale_gradients_by_distance_squared, the RGB renderer's background blend and PSNR
      are oracle/torch_ref.py's restatements.  So, like G4, G8 pins the reference's own glue -- which
      outputs are no_grad, the loss factors, the 0.5 / 0.2 constants, the depth clip, the blend, the
      key set -- NOT the third-party pieces.  The class colours are a seeded random table kept in
      the fixture (the indexing is pinned, not the constants).  Four cases: three spectral ones with
      outputs, flags, losses, metrics and parameter gradients; method "rgb" with outputs and loss.

The stubs below are empty stand-ins for *uninstalled third-party libraries* (jaxtyping, nerfacc,
tinycudann, nerfstudio, cv2, wandb, torchmetrics); no reference source is modified or copied.
Fixtures are data only.  This file cannot import the repository's own package: both are called
``umhsnerf``.
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from oracle import torch_ref as T  # noqa: E402


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Sub:
        def __class_getitem__(cls, _):
            return torch.Tensor

    mod("jaxtyping", Float=_Sub, Int=_Sub, Shaped=_Sub)
    mod("nerfacc", accumulate_along_rays=T.accumulate_along_rays)
    mod("tinycudann")

    class NerfactoField(nn.Module):
        def forward(self, ray_samples, compute_normals=False):
            """nerfstudio's base ``Field.forward`` without normals  [upstream-recalled]."""
            density, density_embedding = self.get_density(ray_samples)
            field_outputs = self.get_outputs(ray_samples, density_embedding=density_embedding)
            field_outputs[FieldHeadNames.DENSITY] = density
            return field_outputs

    class SemanticRenderer(nn.Module):
        pass

    class FieldHeadNames:
        RGB = "rgb"
        DENSITY = "density"

    class SceneBox:
        @staticmethod
        def get_normalized_positions(positions, aabb):
            return (positions - aabb[0]) / (aabb[1] - aabb[0])

    mod("nerfstudio")
    mod("nerfstudio.fields")
    mod("nerfstudio.fields.nerfacto_field", NerfactoField=NerfactoField)
    mod("nerfstudio.fields.base_field", get_normalized_directions=lambda d: (d + 1.0) / 2.0)
    mod("nerfstudio.cameras")
    mod("nerfstudio.cameras.rays", RaySamples=object)
    mod("nerfstudio.field_components")
    mod("nerfstudio.field_components.mlp", MLP=object, MLPWithHashEncoding=object)
    mod("nerfstudio.field_components.field_heads", FieldHeadNames=FieldHeadNames)
    mod("nerfstudio.field_components.activations", trunc_exp=T.trunc_exp)
    mod("nerfstudio.field_components.encodings", NeRFEncoding=object, SHEncoding=object)
    mod("nerfstudio.data")
    mod("nerfstudio.data.scene_box", SceneBox=SceneBox)
    mod("nerfstudio.model_components")
    mod("nerfstudio.model_components.renderers", SemanticRenderer=SemanticRenderer)
    mod("nerfstudio.utils")
    mod("nerfstudio.utils.colors", COLORS_DICT={"black": torch.tensor([0.0, 0.0, 0.0]), "white": torch.tensor([1.0, 1.0, 1.0])})


def _install_model_stubs():
    """What importing the reference's umhs_model.py needs beyond ``_install_stubs()``: more empty stand-ins for uninstalled
    third-party modules, and the few nerfacc / nerfstudio callables ``get_outputs`` really calls, which are the oracle's."""
    import dataclasses

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            pass

    @dataclasses.dataclass
    class InstantNGPModelConfig:
        pass

    class NGPModel(nn.Module):
        @property
        def device(self):
            return torch.device("cpu")

    def scale_gradients_by_distance_squared(field_outputs, ray_samples):
        return T.scale_gradients_by_distance_squared(field_outputs, ray_samples.frustums.starts, ray_samples.frustums.ends)

    for name in ("cv2", "wandb", "torchmetrics"):
        if name not in sys.modules:
            mod(name)
    mod("torchmetrics.image", SpectralAngleMapper=_Any)
    nerfacc = sys.modules["nerfacc"]
    nerfacc.pack_info, nerfacc.render_weight_from_density = T.pack_info, T.render_weight_from_density
    mod("nerfstudio.models")
    mod("nerfstudio.models.instant_ngp", NGPModel=NGPModel, InstantNGPModelConfig=InstantNGPModelConfig)
    mod("nerfstudio.models.nerfacto", NerfactoModel=_Any, NerfactoModelConfig=_Any)
    mod("nerfstudio.models.base_model", Model=_Any, ModelConfig=_Any)
    mod("nerfstudio.cameras.camera_optimizers", CameraOptimizer=_Any, CameraOptimizerConfig=_Any)
    mod("nerfstudio.cameras.cameras", Cameras=_Any)
    sys.modules["nerfstudio.cameras.rays"].RayBundle = object
    mod("nerfstudio.field_components.spatial_distortions", SceneContraction=_Any)
    mod("nerfstudio.utils.colormaps")
    sys.modules["nerfstudio.data.scene_box"].OrientedBox = _Any
    mod("nerfstudio.engine")
    mod("nerfstudio.engine.callbacks", TrainingCallback=_Any, TrainingCallbackAttributes=_Any, TrainingCallbackLocation=_Any)
    mod("nerfstudio.model_components.scene_colliders", NearFarCollider=_Any, AABBBoxCollider=_Any)
    mod("nerfstudio.model_components.ray_samplers", VolumetricSampler=_Any)
    mod("nerfstudio.model_components.losses", MSELoss=nn.MSELoss, distortion_loss=None, interlevel_loss=None, orientation_loss=None,
        pred_normal_loss=None, scale_gradients_by_distance_squared=scale_gradients_by_distance_squared)
    mod("nerfstudio.configs")
    mod("nerfstudio.configs.config_utils", to_immutable_dict=lambda d: tuple(sorted(d.items())))  # hashable: a dataclass default


BAND_SETS = {
    "b21": list(range(450, 651, 10)),
    "b31": list(range(400, 701, 10)),
    "b128": np.linspace(400, 1000, 128).tolist(),
    "b141": np.linspace(440, 720, 141).tolist(),
}


def g1_colour():
    from umhsnerf.utils.spec_to_rgb import ColourSystem

    out = {}
    for name, bands in BAND_SETS.items():
        cs = ColourSystem(bands=bands, cs="sRGB", device="cpu")
        g = torch.Generator().manual_seed(1)
        spec = torch.rand(64, len(bands), generator=g)
        spec[:8] *= 0.004  # rows whose rgb straddles the 0.0031308 gamma knee / goes negative
        spec[8:12] *= 3.0  # rows that clamp at 1
        for ch in range(3):  # one-hot spectra on the most negative matrix entry -> negative rgb -> clamps at 0
            spec[12 + ch] = 0.0
            spec[12 + ch, int(cs.transform_matrix[:, ch].argmin())] = 1.0
        out[f"{name}_bands"] = np.asarray(bands, dtype=np.float64)
        out[f"{name}_M"] = cs.transform_matrix.numpy()
        out[f"{name}_spec"] = spec.numpy()
        out[f"{name}_rgb"] = cs(spec).numpy()
    np.savez_compressed(os.path.join(HERE, "g1_colour.npz"), **out)


def g2_cluster():
    from umhsnerf.utils.clusterprobe import ClusterLookup

    E = np.load("/root/reference/endmembers_hotdog.npy")
    out = {"endmembers_hotdog": E}
    g = torch.Generator().manual_seed(2)
    x = torch.rand(48, E.shape[1], generator=g)
    cl = ClusterLookup(E.shape[1], E.shape[0])
    ip, pr = cl(x, alpha=0.2, clusters=torch.from_numpy(E))
    ip2, pr2 = cl(x, alpha=None, clusters=torch.from_numpy(E))
    out.update(x=x.numpy(), ip=ip.numpy(), probs_a02=pr.numpy(), probs_none=pr2.numpy())
    np.savez_compressed(os.path.join(HERE, "g2_cluster.npz"), **out)


def g3_weights():
    from umhsnerf.umhs_renderer import get_weights_spectral

    g = torch.Generator().manual_seed(3)
    R, S = 12, 40
    deltas = torch.rand(R, S, 1, generator=g) * 0.05
    dens = torch.exp(torch.randn(R, S, 1, generator=g) * 2.0)
    dens[0] = 0.0  # zero-density ray
    dens[1] *= 1e4  # saturating ray
    w = get_weights_spectral(deltas, dens)
    np.savez_compressed(os.path.join(HERE, "g3_weights.npz"), deltas=deltas.numpy(), densities=dens.numpy(), weights=w.numpy())


class _Enc(nn.Module):
    def __init__(self, fn, out_dim):
        super().__init__()
        self.fn, self._out = fn, out_dim

    def get_out_dim(self):
        return self._out

    def forward(self, x):
        return self.fn(x)


class _MLP(nn.Module):
    def __init__(self, ws, bs, out_act=None):
        super().__init__()
        self.ws, self.bs, self.out_act = ws, bs, out_act

    def forward(self, x):
        return T.mlp_forward(x, list(self.ws), list(self.bs), self.out_act)


class _Base(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x):
        return T.mlp_forward(T.hash_encode(x, self.p.hash_table, self.p.scalings, self.p.log2_T), list(self.p.base_w), list(self.p.base_b))


class _Frustums:
    def __init__(self, o, d, s, e):
        self.origins, self.directions, self.starts, self.ends = o, d, s, e
        self.shape = o.shape[:-1]

    def get_positions(self):
        return T.frustum_positions(self.origins, self.directions, self.starts, self.ends)


class _RaySamples:
    def __init__(self, o, d, s, e):
        self.frustums = _Frustums(o, d, s, e)
        self.camera_indices = torch.zeros(o.shape[0], 1, dtype=torch.long)


def _assemble_field(p: T.FieldParams, temperature: float):
    from umhsnerf.umhs_field import UMHSField

    f = UMHSField.__new__(UMHSField)
    nn.Module.__init__(f)
    f.method, f.num_classes, f.wavelengths = p.method, p.C, p.B
    f.pred_specular, f.pred_dino, f.use_scalar = p.pred_specular, False, True
    f.temperature, f.geo_feat_dim, f.appearance_embedding_dim = temperature, p.geo, 0
    f.embedding_appearance, f.average_init_density = None, 1
    f.direction_encoding = _Enc(T.sh_encoding_deg4, 16)
    f.position_encoding = _Enc(T.nerf_encoding, 12)
    f.mlp_base = _Base(p)
    if "spectral" in p.method:
        f.mlp_head = _MLP(p.head_w, p.head_b)
        f.feature_mlp = _MLP(p.feat_w, p.feat_b)
        f.mlp_directional = _MLP(p.dir_w, p.dir_b, "sigmoid")
        f.endmembers = p.endmembers
    else:  # method "rgb": NerfactoField's own colour head, out_activation=nn.Sigmoid()  [upstream-recalled]
        f.mlp_head = _MLP(p.head_w, p.head_b, "sigmoid")
    f.spatial_distortion = T.scene_contraction_linf
    f.aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    return f


def g4_field():
    cases = {
        "c6b31s": dict(C=6, B=31, spec=True, temp=0.4),
        "c9b128s": dict(C=9, B=128, spec=True, temp=0.3),
        "c4b141n": dict(C=4, B=141, spec=False, temp=0.7),
    }
    E141 = np.load("/root/reference/endmembers_hotdog.npy")
    for name, c in cases.items():
        p = T.FieldParams(c["C"], c["B"], c["spec"], log2_hashmap_size=12, table_scale=0.5, seed=7)
        if c["B"] == 141:
            with torch.no_grad():
                p.endmembers.copy_(torch.from_numpy(E141))
        batch = T.synthetic_batch(R=6, S=16, B=c["B"], seed=11)
        o, d, s, e = batch["origins"], batch["directions"], batch["starts"], batch["ends"]
        field = _assemble_field(p, c["temp"])
        rs = _RaySamples(o, d, s, e)
        density, emb = field.get_density(rs)  # reference code, umhs_field.py:300-329
        outs = field.get_outputs(rs, density_embedding=emb)  # reference code, umhs_field.py:151-296
        # a scalar functional of every differentiable output, so parameter grads are pinned too
        g = torch.Generator().manual_seed(5)
        cot_spec = torch.rand(outs["spectral"].shape, generator=g)
        cot_den = torch.rand(density.shape, generator=g)
        loss = (outs["spectral"] * cot_spec).sum() + (density * cot_den).sum()
        names = [k for k, _ in p.named_parameters()]
        grads = torch.autograd.grad(loss, [v for _, v in p.named_parameters()], allow_unused=True)
        out = dict(origins=o.numpy(), directions=d.numpy(), starts=s.numpy(), ends=e.numpy(), temperature=np.float64(c["temp"]),
                   density=density.detach().numpy(), emb=emb.detach().numpy(), cot_spec=cot_spec.numpy(), cot_den=cot_den.numpy())
        for k, v in outs.items():
            out[f"out_{k}"] = v.detach().numpy()
        for k, v in p.named_parameters():
            out[f"param_{k}"] = v.detach().numpy()
        for k, gv in zip(names, grads):
            if gv is not None:
                if k == "hash_table":  # sparse: store touched rows only
                    nz = gv.abs().sum(-1).nonzero()[:, 0]
                    out["grad_hash_rows"] = nz.numpy()
                    out["grad_hash_vals"] = gv[nz].numpy()
                else:
                    out[f"grad_{k}"] = gv.numpy()
        np.savez_compressed(os.path.join(HERE, f"g4_field_{name}.npz"), **out)


def g5_blend():
    from umhsnerf.umhs_renderer import SpectralRenderer

    r = SpectralRenderer()
    g = torch.Generator().manual_seed(6)
    pred = torch.rand(32, 3, generator=g)
    acc = torch.rand(32, 1, generator=g)
    gt = torch.rand(32, 3, generator=g)
    torch.manual_seed(1234)
    bg = torch.rand_like(pred)
    torch.manual_seed(1234)
    p2, g2 = r.blend_background_for_loss_computation(pred, acc, gt, gt)  # umhs_renderer.py:89-114 (rgba has 3 ch -> GT unchanged)
    np.savez_compressed(os.path.join(HERE, "g5_blend.npz"), pred=pred.numpy(), acc=acc.numpy(), gt=gt.numpy(), bg=bg.numpy(),
                        pred_out=p2.numpy(), gt_out=g2.numpy())


# ------------------------------------------------------------------------------------------------------------------------------ #
# G8: the model level
# ------------------------------------------------------------------------------------------------------------------------------ #
G8_COUNTS = [24, 0, 1, 17, 9, 22, 13, 5, 20, 11, 16, 12]  # samples per ray: one ray without a sample, one with exactly one; 150 in all
G8_CASES = {
    "rs_c6b31s": dict(method="rgb+spectral", C=6, B=31, bands="b31", spec=True, temp=0.4, gs=True, rgb_w=1.0, E=None, seed=81),
    "s_c4b141n": dict(method="spectral", C=4, B=141, bands="b141", spec=False, temp=0.7, gs=False, rgb_w=1.0, E="g7_endmembers_hotdog.npy", seed=82),
    "rs_c9b128s": dict(method="rgb+spectral", C=9, B=128, bands="b128", spec=True, temp=0.3, gs=True, rgb_w=0.3, E=None, seed=83),
    "rgb_c5b21": dict(method="rgb", C=5, B=21, bands="b21", spec=False, temp=0.5, gs=True, rgb_w=1.0, E=None, seed=84),
}
# what the builder may turn until the conditioning asserts hold: (rise of the density bias, stretch of every other ray's intervals,
# scale of the feature MLP's last layer), tried in this order
G8_KNOBS = [(b, s, f) for f in (4.0, 8.0, 2.0) for b in (2.0, 1.5, 2.5, 1.0, 3.0) for s in (16.0, 8.0, 24.0, 4.0, 30.0)]
G8_BAND_PREFIXES = ("wv_", "residual_", "abundances_")


def _g8_rays(seed, stretch):
    """12 rays towards the unit box from cameras 1.5 .. 2.7 away (so a share of the samples lies nearer than t = 1, where gradient
    scaling is not the identity), ``G8_COUNTS`` samples each, every other ray's intervals ``stretch`` times as long."""
    import math

    g = torch.Generator().manual_seed(seed)
    R = len(G8_COUNTS)
    u = torch.randn(R, 3, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    o = u * torch.linspace(1.5, 2.7, R)[torch.randperm(R, generator=g)][:, None] + (torch.rand(R, 3, generator=g) * 2 - 1) * 0.2
    d = -o + torch.randn(R, 3, generator=g) * 0.1
    d = d / d.norm(dim=-1, keepdim=True)
    cnt = torch.tensor(G8_COUNTS)
    ri = torch.repeat_interleave(torch.arange(R), cnt)
    k = torch.arange(int(cnt.sum())) - torch.repeat_interleave(cnt.cumsum(0) - cnt, cnt)
    step, stride = math.sqrt(12.0) / 1000.0, 2.6 / 24
    t_near = (o.norm(dim=-1) - 1.3).clamp(min=0.05) + torch.rand(R, generator=g) * step
    t0 = t_near[ri] + k * stride
    width = step * (1 + 0.004 * t0) * torch.where(ri % 2 == 1, torch.tensor(stretch), torch.tensor(1.0))
    assert float(width.max()) < stride  # intervals of a ray do not overlap
    return o[ri].contiguous(), d[ri].contiguous(), t0[:, None].contiguous(), (t0 + width)[:, None].contiguous(), ri, R


def _g8_bump_endmembers(C, B):
    """Well separated bump-shaped spectra: one Gaussian bump per material on a 0.1 floor."""
    x = torch.linspace(0, 1, B)[None, :]
    mu = ((torch.arange(C) + 0.5) / C)[:, None]
    return (0.1 + 0.8 * torch.exp(-(((x - mu) * C / 0.6) ** 2))).float()


class _Bundle:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _RGBRenderer:
    """Stand-in for nerfstudio's RGBRenderer with background_color="random"  [upstream-recalled]: the blend is the oracle's, its
    ``rand_like`` draw is seeded and kept; ``blend_background`` is the identity for 3-channel images; a call without ray_indices sums
    over dim -2 (what the reference's method "rgb" gets on packed samples)."""

    def __init__(self, seed):
        self.seed, self.bg = seed, None

    def __call__(self, rgb, weights):
        return torch.sum(weights * rgb, dim=-2)

    def blend_background(self, image):
        assert image.shape[-1] == 3
        return image

    def blend_background_for_loss_computation(self, pred_image, pred_accumulation, gt_image):
        torch.manual_seed(self.seed)
        self.bg = torch.rand_like(pred_image)
        return T.blend_background_for_loss(pred_image, pred_accumulation, gt_image, self.bg)


def _g8_run(name, c, bias, stretch, feat_scale):
    """One run of the reference's UMHSModel.get_outputs / get_loss_dict / get_metrics_dict on a hand-assembled instance."""
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel
    from umhsnerf.umhs_renderer import SpectralRenderer
    from umhsnerf.utils.clusterprobe import ClusterLookup
    from umhsnerf.utils.spec_to_rgb import ColourSystem

    C, B, seed = c["C"], c["B"], c["seed"]
    p = T.FieldParams(C, B, c["spec"], method=c["method"], log2_hashmap_size=12, table_scale=0.5, seed=seed)
    with torch.no_grad():
        p.base_b[1][0] += bias
        if "spectral" in c["method"]:
            p.feat_w[-1].mul_(feat_scale)  # sharper abundances: the composited spectra of different rays lie further apart
            if c["E"] is None:
                p.endmembers.copy_(_g8_bump_endmembers(C, B))
            else:
                p.endmembers.copy_(torch.from_numpy(np.load(os.path.join(HERE, c["E"]))))
    o, d, s, e, ri, R = _g8_rays(seed + 100, stretch)
    rs = _RaySamples(o, d, s, e)
    tmid = (s + e) / 2
    lo, hi = tmid.min(), tmid.max()

    m = UMHSModel.__new__(UMHSModel)
    nn.Module.__init__(m)
    m.config = UMHSConfig(method=c["method"], pred_specular=c["spec"], temperature=c["temp"], use_gradient_scaling=c["gs"],
                          rgb_loss_weight=c["rgb_w"], log2_hashmap_size=12)
    assert m.config.background_color == "random" and m.config.pred_dino is False
    m.field = _assemble_field(p, c["temp"])
    m.sampler = lambda **kw: (rs, ri)
    m.renderer_depth = lambda weights, ray_samples, ray_indices, num_rays: T.render_depth_expected(
        weights, ray_samples.frustums.starts, ray_samples.frustums.ends, ray_indices, num_rays, (lo, hi))
    m.renderer_accumulation = lambda weights, ray_indices, num_rays: T.accumulate_along_rays(weights[..., 0], None, ray_indices, num_rays)
    m.renderer_rgb = _RGBRenderer(seed + 200)
    m.rgb_loss, m.psnr = nn.MSELoss(), T.psnr
    g = torch.Generator().manual_seed(seed + 300)
    colors = torch.rand(15, 3, generator=g)  # NOT the reference's constants: the fixture pins the indexing
    m.class_colors = {i: colors[i] for i in range(15)}
    bands = BAND_SETS[c["bands"]]
    m.converter = ColourSystem(bands=bands, cs="sRGB", device="cpu")
    if "spectral" in c["method"]:
        m.renderer_spectral, m.spectral_loss = SpectralRenderer(), nn.MSELoss()
        m.cluster_probe = ClusterLookup(B, C)
    batch = {"image": torch.rand(R, 3, generator=g), "hs_image": torch.rand(R, B, generator=g)}  # independent of each other

    outputs = m.get_outputs(_Bundle(R))
    loss_dict = m.get_loss_dict(outputs, batch)
    metrics = m.get_metrics_dict(outputs, batch) if c["method"] != "rgb" else {}  # (method "rgb" never sets num_samples_per_ray)
    names = [k for k, _ in p.named_parameters()]
    grads = torch.autograd.grad(sum(loss_dict.values()), [v for _, v in p.named_parameters()], allow_unused=True)

    cond = {}
    if c["method"] != "rgb":
        acc = outputs["accumulation"][:, 0].detach()
        cond["acc_above"], cond["acc_below"] = int((acc > 0.5).sum()), int((acc < 0.5).sum())
        cond["acc_min_dist_to_half"] = float((acc - 0.5).abs().min())
        sampled = torch.tensor(G8_COUNTS) > 0  # (a ray without a sample has spectral = 0 and uniform probabilities: gap 0, label masked by acc_if)
        top2 = outputs["seg_probs"].detach().topk(2, dim=1).values
        cond["seg_min_top2_gap"] = float((top2[:, 0] - top2[:, 1])[sampled].min())
        cond["share_t_mid_below_1"] = float((tmid < 1).float().mean())
    inputs = dict(origins=o, directions=d, starts=s, ends=e, ray_indices=ri, image=batch["image"], hs_image=batch["hs_image"],
                  bg_random=m.renderer_rgb.bg, class_colors=colors)
    return p, inputs, bands, outputs, loss_dict, metrics, names, grads, cond


def _g8_conditioned(cond):
    return (cond["acc_above"] >= 3 and cond["acc_below"] >= 3 and cond["acc_min_dist_to_half"] >= 1e-2
            and cond["seg_min_top2_gap"] >= 1e-4 and cond["share_t_mid_below_1"] >= 0.1)


def g8_model():
    _install_model_stubs()
    for name, c in G8_CASES.items():
        for bias, stretch, feat_scale in G8_KNOBS:
            p, inputs, bands, outputs, loss_dict, metrics, names, grads, cond = _g8_run(name, c, bias, stretch, feat_scale)
            if c["method"] == "rgb" or _g8_conditioned(cond):
                break
        else:
            raise AssertionError(f"{name}: no knob setting meets the conditioning")
        if c["method"] != "rgb":
            assert _g8_conditioned(cond), cond
        print(name, "density bias +", bias, "stretch", stretch, "feature scale", feat_scale, cond)
        base = [k for k in outputs if not k.startswith(G8_BAND_PREFIXES)]
        for prefix, whole in (("wv_", "spectral"), ("residual_", "specular"), ("abundances_", "abundances")):
            views = [k for k in outputs if k.startswith(prefix)]
            assert views == ([f"{prefix}{i}" for i in range(outputs[whole].shape[-1])] if whole in outputs else [])
            for i, k in enumerate(views):  # the per-band views are the columns: not stored again
                assert torch.equal(outputs[k], outputs[whole][..., i]), k
        out = {k: v.numpy() for k, v in inputs.items() if v is not None}
        out.update(method=np.array(c["method"]), num_classes=np.int64(c["C"]), pred_specular=np.bool_(c["spec"]), temperature=np.float64(c["temp"]),
                   use_gradient_scaling=np.bool_(c["gs"]), rgb_loss_weight=np.float64(c["rgb_w"]), log2_hashmap_size=np.int64(12),
                   num_rays=np.int64(len(G8_COUNTS)), bands=np.asarray(bands, dtype=np.float64), output_keys=np.array(list(outputs)),
                   knob_density_bias=np.float64(bias), knob_stretch=np.float64(stretch), knob_feat_scale=np.float64(feat_scale))
        for k in base:
            out[f"out_{k}"] = outputs[k].detach().numpy()
            out[f"rg_{k}"] = np.bool_(outputs[k].requires_grad)
        for k, v in loss_dict.items():
            out[f"loss_{k}"] = np.float64(v.detach())
        for k, v in metrics.items():
            out[f"metric_{k}"] = np.float64(v)
        for k, v in cond.items():
            out[f"cond_{k}"] = np.float64(v)
        for k, v in p.named_parameters():
            out[f"param_{k}"] = v.detach().numpy()
        for k, gv in zip(names, grads):
            if gv is not None:
                if k == "hash_table":  # sparse: touched rows only
                    nz = gv.abs().sum(-1).nonzero()[:, 0]
                    out["grad_hash_rows"] = nz.numpy().astype(np.int32)
                    out["grad_hash_vals"] = gv[nz].numpy()
                else:
                    out[f"grad_{k}"] = gv.numpy()
        path = os.path.join(HERE, f"g8_model_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 1_000_000, (path, os.path.getsize(path))


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["g1", "g2", "g3", "g4", "g5", "g8"], action="append",
                    help="write these fixtures only (default: all); the others are left as they are")
    only = ap.parse_args().only
    want = lambda name: only is None or name in only
    torch.set_num_threads(4)
    if want("g1"):
        g1_colour()
    if want("g2"):
        g2_cluster()
    _install_stubs()
    if want("g3"):
        g3_weights()
    if want("g4"):
        g4_field()
    if want("g5"):
        g5_blend()
    if want("g8"):
        g8_model()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
