"""Ray generation with OpenCV lens distortion on the GPU: ``umhs_raygen_distorted`` against the float64 restatement
(tests/raygen_f64.py), its round trip through the closed-form model, the bit-equality of zero rows with ``umhs_raygen``, and the layers
above it -- ``ResidentSplit`` / ``UMHSDataManager``, ``Cameras.generate_rays`` -> ``UMHSModel.get_outputs_for_camera``, and training
from a ``transforms.json`` that carries k1, k2, p1, p2.

Inputs of the accuracy tests: 9 cameras with random orthonormal poses, 640x480 images, fx = fy = 500, principal point at the image
centre, 20,000 sampled pixels plus the four corners of every camera, parameters per camera from ``raygen_f64.draw_distortion``'s box.

Bounds (none comes from the kernel's own output):
  * origins: bit-equal (a copy).
  * directions (absolute) and directions_norm (relative): the float32 CPU restatement's own largest distance from float64 on the same
    inputs is the noise floor of the arithmetic the kernel shares (the Newton solve in float32 ends within ~2e-7 of the float64 one in
    image-plane units); the kernel is allowed twice that, and never less than the 2e-7 that tests/test_hip_data.py grants the
    undistorted kernel.
  * pixel_area (relative): the undistorted test's 2e-3 (a difference of nearly equal unit vectors: cancellation), or twice the float32
    restatement's own relative distance from float64 if that is larger.
  * round trip: a direction off by e moves the projected image-plane point by at most e (1 + |p|) |v| (p the image-plane point,
    |v|^2 = 1 + |p|^2; |p| <= 0.9 at the corners here: 2.6 e), the forward model stretches that by at most d + 2 r |k1| + ... <= 1.3
    in this box, and fx = 500 turns it into pixels: 500 * 4 * e is a safe ceiling, capped at 1e-3 px."""
import json

import numpy as np
import pytest
import torch

import raygen_f64 as RG
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CAMS, H, W, F = 9, 480, 640, 500.0


def _case(seed=0):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(N_CAMS, 3, 3, generator=g))
    c2w = torch.cat([q, torch.randn(N_CAMS, 3, 1, generator=g)], -1).contiguous()
    intr = torch.tensor([[F, F, W / 2, H / 2]]).expand(N_CAMS, 4).contiguous()
    idx = T.pixel_sample_indices(torch.rand(20000, 3, generator=g), N_CAMS, H, W)
    corners = torch.tensor([[c, y, x] for c in range(N_CAMS) for y in (0, H - 1) for x in (0, W - 1)])
    return torch.cat([idx, corners]).contiguous(), c2w, intr, RG.draw_distortion(N_CAMS, seed)


def _hip(idx, c2w, intr, k, **kw):
    from umhsnerf import ops

    return ops.raygen(idx.to(DEV), c2w.to(DEV), intr.to(DEV), distortion=None if k is None else k.to(DEV), **kw)


def _bounds(idx, c2w, intr, k):
    """float64 truth, and the bounds the float32 restatement's own error sets (module docstring)."""
    o64, d64, a64, n64, min_det = RG.generate_rays_distorted(idx, c2w.double(), intr.double(), k.double(), return_min_det=True)
    # precondition on the inputs, in float64: no ray of this box is anywhere near the |det| > 1e-3 switch, so none is excluded
    assert float(min_det.min()) > 0.1, float(min_det.min())
    _, d32, a32, n32 = RG.generate_rays_distorted(idx, c2w, intr, k)
    e_d = float((d32.double() - d64).abs().max())
    e_n = float(((n32.double() - n64) / n64).abs().max())
    e_a = float(((a32.double() - a64) / a64).abs().max())
    return (o64, d64, a64, n64), (e_d, e_n, e_a), (max(2e-7, 2 * e_d), max(2e-7, 2 * e_n), max(2e-3, 2 * e_a))


def test_kernel_against_float64():
    # Measured on an MI355X (kernel vs float64 | float32 restatement vs float64 | bound):
    #   directions       1.32e-7 | 1.41e-7 | 2.81e-7
    #   directions_norm  1.69e-7 | 1.58e-7 | 3.16e-7  (relative)
    #   pixel_area       1.22e-4 | 1.22e-4 | 2e-3     (relative)
    idx, c2w, intr, k = _case()
    (o64, d64, a64, n64), (e_d, e_n, e_a), (b_d, b_n, b_a) = _bounds(idx, c2w, intr, k)
    o, d, area, nrm = _hip(idx, c2w, intr, k, want_area=True, want_norm=True)
    g_d = float((d.cpu().double() - d64).abs().max())
    g_n = float(((nrm.cpu().double() - n64) / n64).abs().max())
    g_a = float(((area.cpu().double() - a64) / a64).abs().max())
    print(f"directions: hip {g_d:.3e} f32 {e_d:.3e} bound {b_d:.3e}; norm (rel): hip {g_n:.3e} f32 {e_n:.3e} bound {b_n:.3e}; "
          f"area (rel): hip {g_a:.3e} f32 {e_a:.3e} bound {b_a:.3e}")
    assert torch.equal(o.cpu(), o64.float())
    assert g_d <= b_d and g_n <= b_n and g_a <= b_a, (g_d, b_d, g_n, b_n, g_a, b_a)
    assert float((d.cpu() - T.generate_rays(idx, c2w, intr)[1]).abs().max()) > 1e-2  # and the distortion was not a no-op


def test_device_rays_land_on_their_pixel_through_the_closed_form_model():
    # Measured on an MI355X: 8.5e-5 px against a bound of 500 * 4 * 2.81e-7 = 5.6e-4 px (module docstring)
    idx, c2w, intr, k = _case()
    _, _, (b_d, _, _) = _bounds(idx, c2w, intr, k)
    _, d, _, _ = _hip(idx, c2w, intr, k, want_area=False)
    px = RG.reproject(d.cpu(), idx, c2w, intr, k)
    centre = torch.stack([idx[:, 2], idx[:, 1]], -1).double() + 0.5
    err = float((px - centre).abs().max())
    bound = min(1e-3, F * 4 * b_d)
    print(f"round trip: {err:.3e} px, bound {bound:.3e} px")
    assert err <= bound, (err, bound)


def test_zero_rows_are_the_undistorted_kernel_bit_for_bit():
    idx, c2w, intr, _ = _case()
    g = torch.Generator().manual_seed(7)  # the undistorted test's cameras too: off-centre principal points, fx != fy
    intr2 = torch.stack([torch.rand(N_CAMS, generator=g) * 500 + 100, torch.rand(N_CAMS, generator=g) * 500 + 100,
                         torch.full((N_CAMS,), W / 2) + torch.randn(N_CAMS, generator=g), torch.full((N_CAMS,), H / 2) + torch.randn(N_CAMS, generator=g)], -1)
    for intrinsics in (intr, intr2.contiguous()):
        a = _hip(idx, c2w, intrinsics, torch.zeros(N_CAMS, 6), want_area=True, want_norm=True)
        b = _hip(idx, c2w, intrinsics, None, want_area=True, want_norm=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_mixed_rows_zero_cameras_are_bit_equal():
    idx, c2w, intr, k = _case()
    zero = torch.tensor([0, 3, 4, 8])
    k = k.clone()
    k[zero] = 0.0
    a = _hip(idx, c2w, intr, k, want_area=True, want_norm=True)
    b = _hip(idx, c2w, intr, None, want_area=True, want_norm=True)
    is_zero = torch.isin(idx[:, 0], zero).to(DEV)
    assert 0 < int(is_zero.sum()) < len(idx)
    for x, y in zip(a, b):
        assert torch.equal(x[is_zero], y[is_zero])
    assert float((a[1][~is_zero] - b[1][~is_zero]).abs().max()) > 1e-2
    _, d64, _, _ = RG.generate_rays_distorted(idx, c2w.double(), intr.double(), k.double())
    assert float((a[1].cpu().double() - d64).abs().max()) <= _bounds(idx, c2w, intr, k)[2][0]


def test_edge_cases():
    from umhsnerf import ops

    idx, c2w, intr, k = _case()
    o, d, area, nrm = _hip(idx[:0], c2w, intr, k, want_area=True, want_norm=True)  # n_rays = 0: nothing is launched
    assert o.shape == (0, 3) and d.shape == (0, 3) and area.shape == (0, 1) and nrm.shape == (0, 1)
    o, d, area, nrm = _hip(idx, c2w, intr, k, want_area=False)
    assert area is None and nrm is None
    assert torch.equal(d, _hip(idx, c2w, intr, k, want_area=True, want_norm=True)[1])
    # out-of-range camera indices clamp to the first / last camera, as in umhs_raygen
    bad = idx[:64].clone()
    bad[:32, 0], bad[32:, 0] = -5, N_CAMS + 3
    want = bad.clone()
    want[:32, 0], want[32:, 0] = 0, N_CAMS - 1
    for x, y in zip(_hip(bad, c2w, intr, k, want_area=True, want_norm=True), _hip(want, c2w, intr, k, want_area=True, want_norm=True)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="distortion"):
        ops.raygen(idx.to(DEV), c2w.to(DEV), intr.to(DEV), distortion=k[:, :5].contiguous().to(DEV))


def _split(on_gpu=True, n=4, Hs=24, Ws=32, B=8, seed=3, const=None, distorted=True):
    """tests/test_hip_data.py's cameras on a sphere looking at the origin, the principal point on the centre of pixel (Hs/2, Ws/2)."""
    from umhsnerf.data.umhs_datamanager import ResidentSplit
    from umhsnerf.data.umhs_dataparser import Cameras

    g = torch.Generator().manual_seed(seed)
    pos = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 0.9
    z = torch.nn.functional.normalize(pos, dim=-1)
    x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([[0.0, 0, 1]]).expand(n, 3), z), dim=-1)
    y = torch.linalg.cross(z, x)
    c2w = torch.stack([x, y, z, pos], -1).contiguous()
    k = torch.tensor([[-0.1, 0.02, 0.0, 0.0, 1e-3, -1e-3]]).expand(n, 6).contiguous() if distorted else None
    cams = Cameras(c2w, torch.full((n,), 30.0), torch.full((n,), 30.0), torch.full((n,), Ws / 2 + 0.5), torch.full((n,), Hs / 2 + 0.5), Hs, Ws,
                   distortion_params=k)
    hs = torch.rand(n, Hs, Ws, B, generator=g) if const is None else torch.full((n, Hs, Ws, B), const)
    rgb = torch.rand(n, Hs, Ws, 3, generator=g)
    return ResidentSplit(cams, rgb, hs, DEV, on_gpu=on_gpu)


@pytest.mark.parametrize("on_gpu", [True, False])
def test_datamanager_rays_carry_the_distortion(on_gpu):
    from umhsnerf import ops
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig

    split, plain = _split(on_gpu), _split(on_gpu, distorted=False)
    assert split.distortion.is_cuda and split.distortion.shape == (4, 6) and plain.distortion is None
    dm = UMHSDataManager(UMHSDataManagerConfig(train_num_rays_per_batch=1000, images_on_gpu=on_gpu), device=DEV, seed=5, train=split)
    rb, batch = dm.next_train(0)
    o, d, area, nrm = ops.raygen(batch["indices"], split.c2w, split.intrinsics, want_area=True, want_norm=True, distortion=split.distortion)
    assert torch.equal(rb.origins, o) and torch.equal(rb.directions, d) and torch.equal(rb.pixel_area, area)
    assert torch.equal(rb.metadata["directions_norm"], nrm)
    assert not torch.equal(d, ops.raygen(batch["indices"], split.c2w, split.intrinsics)[1])
    assert dm.next_eval(0)[0].directions.shape == (4096, 3)
    cam, full = dm.next_eval_image(0)
    ref = plain.image_rays(0)
    assert cam.directions.shape == (24, 32, 3) and cam.origins.shape == (24, 32, 3) and full["hs_image"].shape == (24, 32, 8)
    # the principal point is the centre of pixel (12, 16): the model leaves that ray where it is ...
    assert float((cam.directions[12, 16] - ref.directions[12, 16]).abs().max()) <= 1e-6
    # ... and moves the corners: r^2 ~ 0.44 there, k1 = -0.1 undistorts them outwards by ~4 % of 0.67 -- far above rounding
    for yy, xx in ((0, 0), (0, 31), (23, 0), (23, 31)):
        assert float((cam.directions[yy, xx] - ref.directions[yy, xx]).abs().max()) > 5e-3, (yy, xx)


def _tiny_pipeline(split, B, classes=3, rays=1024):
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    dm = UMHSDataManager(UMHSDataManagerConfig(train_num_rays_per_batch=rays), device=DEV, seed=1, train=split)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    return UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": list(np.linspace(420, 680, B)), "num_classes": classes}, seed=2,
                                            datamanager=dm)


def test_model_renders_the_projects_own_cameras():
    torch.manual_seed(0)
    B = 8
    split = _split(B=B)
    pipe = _tiny_pipeline(split, B)
    for step in range(3):
        pipe.get_train_loss_dict(step)
    pipe.eval()
    cams = split.cameras
    rb = cams.generate_rays(camera_indices=0, keep_shape=True)
    assert rb.origins.shape == (24, 32, 3) and rb.pixel_area.shape == (24, 32, 1) and rb.camera_indices.shape == (24, 32, 1)
    assert torch.equal(rb.directions, split.image_rays(0).directions)
    assert cams.generate_rays(2, keep_shape=False).directions.shape == (24 * 32, 3)
    out = pipe.model.get_outputs_for_camera(cams)
    assert out["spectral"].shape == (24, 32, B) and out["rgb"].shape == (24, 32, 3) and out["accumulation"].shape == (24, 32, 1)
    want = pipe.model.get_outputs_for_camera_ray_bundle(split.image_rays(0))
    assert torch.equal(out["spectral"], want["spectral"]) and bool(torch.isfinite(out["spectral"]).all())


def _look_at_origin(rng):
    pos = rng.normal(size=3)
    pos = 3.0 * pos / np.linalg.norm(pos)
    z = pos / np.linalg.norm(pos)  # the camera looks down -z
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, pos
    return m


def make_scene(root, n_train=6, n_eval=2, Hs=24, Ws=32, B=8, hs_value=0.6, seed=0, **top):
    """The ``make_scene`` recipe of tests/test_data_cpu.py (unsorted frames, train / eval folders, uint8 RGBA + float32 cubes), with
    cameras that look at the scene and a constant spectrum, so that there is something to learn; ``top``: extra top-level keys."""
    rng = np.random.default_rng(seed)
    frames = []
    for split, cnt in (("train", n_train), ("eval", n_eval)):
        (root / split).mkdir(parents=True)
        (root / f"hs_{split}").mkdir()
        for i in reversed(range(cnt)):
            np.save(root / split / f"r_{i:03d}.npy", (rng.random((Hs, Ws, 4)) * 255).astype(np.uint8))
            np.save(root / f"hs_{split}" / f"r_{i:03d}.npy", np.full((Hs, Ws, B), hs_value, dtype=np.float32))
            frames.append({"file_path": f"{split}/r_{i:03d}.npy", "hyperspectral_file_path": f"hs_{split}/r_{i:03d}.npy",
                           "transform_matrix": _look_at_origin(rng).tolist()})
    meta = {"frames": frames, "wavelengths": [420 + 30 * k for k in range(B)], "fl_x": 30.0, "fl_y": 30.0, "cx": Ws / 2, "cy": Hs / 2, "h": Hs, "w": Ws}
    meta.update(top)
    (root / "transforms.json").write_text(json.dumps(meta))
    return meta


def test_training_from_a_distorted_scene_on_disk_reduces_the_loss(tmp_path):
    """``transforms.json`` with k1, k2, p1, p2 -> UMHSDataManager -> training steps (``get_train_loss_dict`` of a pipeline that owns its
    optimizer: next_train, sampler, field, losses, backward, Adam), as test_training_from_the_datamanager_reduces_the_loss does."""
    from umhsnerf import ops
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    B = 8
    meta = make_scene(tmp_path, B=B, camera_model="OPENCV", k1=-0.1, k2=0.02, p1=1e-3, p2=-1e-3)
    dm = UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=tmp_path), train_num_rays_per_batch=2048), device=DEV,
                         num_classes=3, seed=1)
    want = torch.tensor([-0.1, 0.02, 0.0, 0.0, 1e-3, -1e-3], device=DEV)
    for split, n in ((dm.train_split, 6), (dm.eval_split, 2)):
        assert torch.equal(split.distortion, want.expand(n, 6)) and split.distortion.is_cuda
    rb, batch = dm.next_train(0)
    assert not torch.equal(rb.directions, ops.raygen(batch["indices"], dm.train_split.c2w, dm.train_split.intrinsics)[1])
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2, datamanager=dm)
    split = dm.train_split
    with torch.no_grad():  # a self-consistent target: rgb = converter(hs)
        split.image = pipe.model.converter(split.hs_image.view(-1, B)).view(*split.hs_image.shape[:3], 3).contiguous()
    losses = []
    for step in range(80):
        _, loss_dict, metrics = pipe.get_train_loss_dict(step)
        losses.append(float(sum(loss_dict.values()).detach()))
    assert np.isfinite(losses).all() and np.mean(losses[-10:]) < 0.5 * np.mean(losses[:5]), (losses[:5], losses[-10:])
