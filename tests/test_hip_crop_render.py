"""Cropped and non-perspective rendering end to end on the GPU: ``get_outputs_for_camera(camera, obb_box=)``, the background override,
a fisheye camera path with a ``crop`` through ``load_camera_path`` / ``render_camera_path``, and the ``dataset`` / ``interpolate``
subcommands -- on the small trained pipeline of tests/test_hip_render.py (the ``make_scene`` recipe: 24 x 32 frames of 8 bands, 3 classes,
``pred_specular``, three training steps, ``background_color="black"``) and 20 x 28 path frames."""
import json

import numpy as np
import pytest
import torch

import frame_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
FLAGS = ["--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"]
CROP = {"crop_center": [0.1, -0.05, 0.2], "crop_scale": [0.9, 0.6, 1.2], "crop_rot": [0.3, -0.2, 0.5], "crop_bg_color": {"r": 38, "g": 120, "b": 255}}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Scene, trained pipeline, its checkpoint, and the perspective cameras of a path file: shared by the tests below."""
    from test_hip_distortion import _look_at_origin, make_scene
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.render import load_camera_path
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    root = tmp_path_factory.mktemp("crop")
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    dm = UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=scene), train_num_rays_per_batch=1024), device=DEV,
                         num_classes=3, seed=9)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2, datamanager=dm)
    for step in range(3):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    pipe.eval()
    torch.save({"step": 3, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    rng = np.random.default_rng(11)
    path = {"camera_type": "perspective", "render_height": H, "render_width": W, "fps": 24, "seconds": 0.125,
            "camera_path": [{"camera_to_world": _look_at_origin(rng).reshape(-1).tolist(), "fov": fov, "aspect": W / H} for fov in FOVS]}
    cameras, _ = load_camera_path(path, device=DEV)
    return dict(root=root, scene=scene, pipe=pipe, path=path, cameras=cameras)


def _one(cameras, i):
    """Camera ``i`` alone (``get_outputs_for_camera`` renders camera 0 of what it is given)."""
    from umhsnerf.data.umhs_dataparser import Cameras

    s = slice(i, i + 1)
    return Cameras(cameras.camera_to_worlds[s], cameras.fx[s], cameras.fy[s], cameras.cx[s], cameras.cy[s], cameras.height, cameras.width,
                   None, cameras.camera_type)


def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path))


def _box():
    from umhsnerf.render import parse_crop

    return parse_crop(CROP)


def test_a_box_that_swallows_the_scene_changes_nothing(world):
    """Scale 64 about the origin: every ray starts inside (t_min = 0, so nears = near_plane) and leaves the box beyond the occupancy
    grid's own exit -- every output is the uncropped one, bit for bit."""
    from umhsnerf.export import obb_from_params

    model = world["pipe"].model
    box = obb_from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (64.0, 64.0, 64.0))
    for i in (0, 1):
        cam = _one(world["cameras"], i)
        plain, cropped = model.get_outputs_for_camera(cam), model.get_outputs_for_camera(cam, obb_box=box)
        assert list(plain) == list(cropped) and int(plain["num_samples_per_ray"].sum()) > 0
        for k in plain:
            assert torch.equal(plain[k], cropped[k]), (i, k)
        rb = cam.generate_rays(0, obb_box=box, near_floor=model.config.near_plane)
        assert rb.nears.shape == (H, W, 1) and bool((rb.nears == model.config.near_plane).all()) and bool((rb.fars > 16.0).all())


def test_a_real_crop_renders_only_what_lies_inside_the_box(world):
    from umhsnerf._ns_compat import RayBundle

    model, crop = world["pipe"].model, _box()
    Tb, Rb, Sb = (torch.tensor(v, device=DEV) for v in crop["obb"])
    bg = torch.tensor(crop["background_color"], dtype=torch.float32, device=DEV)
    for i in (0, 1):
        cam = _one(world["cameras"], i)
        plain = model.get_outputs_for_camera(cam)
        with model.background_color_override_context(crop["background_color"]):
            cropped = model.get_outputs_for_camera(cam, obb_box=crop["obb"])
        rb = cam.generate_rays(0, obb_box=crop["obb"], near_floor=model.config.near_plane)
        miss = (rb.nears == 1e10).view(H, W)
        assert torch.equal(miss, (rb.fars == 1e10).view(H, W)) and 10 < int((~miss).sum()) < H * W - 10
        # rays that miss the box: nothing accumulated, and exactly the crop's colour
        assert bool((cropped["accumulation"][miss] == 0).all())
        assert torch.equal(cropped["rgb"][miss], bg.expand(int(miss.sum()), 3))
        # no output but rgb knows about the override: the same crop without it differs in rgb alone
        bare = model.get_outputs_for_camera(cam, obb_box=crop["obb"])
        assert all(torch.equal(bare[k], cropped[k]) for k in bare if k != "rgb") and bool((bare["rgb"][miss] == 0).all())
        assert torch.equal(cropped["rgb"], bare["rgb"] + bg * (1.0 - bare["accumulation"]))
        # the sampler on the cropped bundle: every sample's midpoint in [nears, fars] of its own ray, and inside the box
        flat = RayBundle(origins=rb.origins.view(-1, 3), directions=rb.directions.view(-1, 3), nears=rb.nears.view(-1, 1), fars=rb.fars.view(-1, 1))
        samples, ri = model.sample(flat)
        fr = samples.frustums
        n_cropped = int(cropped["num_samples_per_ray"].sum())
        assert n_cropped > 0 and fr.starts.shape[0] == n_cropped
        t = ((fr.starts + fr.ends) / 2).view(-1)
        assert bool((t >= flat.nears.view(-1)[ri]).all()) and bool((t <= flat.fars.view(-1)[ri]).all())
        assert not bool(miss.view(-1)[ri].any())
        p = fr.origins + fr.directions * t[:, None]
        local = (p - Tb) @ Rb  # rows: R^T (p - T)
        # float32 eps * (|o| + t <= 9) * a handful of operations
        assert bool((local.abs() <= Sb / 2 + 1e-5).all()), float((local.abs() - Sb / 2).max())
        assert n_cropped < int(plain["num_samples_per_ray"].sum())


def test_a_cropped_fisheye_path_through_the_loader(world, tmp_path):
    from umhsnerf.render import CAMERA_TYPES, load_camera_path, render_camera_path
    from umhsnerf.utils import colormaps

    path = dict(world["path"], camera_type="fisheye", crop=CROP)
    (tmp_path / "path.json").write_text(json.dumps(path))
    with pytest.raises(NotImplementedError, match="fisheye"):  # a caller that does not say it renders these is refused, as ever
        load_camera_path(tmp_path / "path.json", device=DEV)
    cameras, meta = load_camera_path(tmp_path / "path.json", device=DEV, camera_types=CAMERA_TYPES, crop=True)
    assert cameras.camera_type == "fisheye" and meta["crop"] is not None
    pipe = world["pipe"]
    res = render_camera_path(pipe, cameras, tmp_path / "out", ["rgb", "accumulation"], crop=meta["crop"])
    assert res["frames"] == 3 and not pipe.training
    colour = R.q(np.float32(meta["crop"]["background_color"]))
    zero = R.q(colormaps.table("default")[0])
    assert colour.tolist() == [38, 120, 255]
    for i in range(3):
        frame = _png(tmp_path / "out" / f"frame_{i:05d}.png")
        assert frame.shape == (H, 2 * W, 3)
        rb = cameras.generate_rays(i, obb_box=meta["crop"]["obb"], near_floor=pipe.model.config.near_plane)
        miss = (rb.nears == 1e10).view(H, W).cpu().numpy()
        assert 10 < miss.sum() < H * W - 10
        assert (frame[:, :W][miss] == colour).all() and (frame[:, W:][miss] == zero).all()
        assert not (frame[:, W:][~miss] == zero).all()  # something was rendered inside the box
    # the fisheye frame is not the perspective one
    assert not torch.equal(cameras.generate_rays(0).directions, world["cameras"].generate_rays(0).directions)


def test_the_override_is_gone_after_a_cropped_render_returns_or_raises(world, tmp_path):
    from umhsnerf.render import render_camera_path

    pipe, cameras, crop = world["pipe"], world["cameras"], _box()
    cam = _one(cameras, 2)
    before = pipe.model.get_outputs_for_camera(cam)
    render_camera_path(pipe, cameras, tmp_path / "a", ["rgb"], crop=crop)
    assert pipe.model._background_override is None
    after = pipe.model.get_outputs_for_camera(cam)
    with pytest.raises(ValueError, match="usable names"):
        render_camera_path(pipe, cameras, tmp_path / "b", ["rgb", "nope"], crop=crop)
    assert pipe.model._background_override is None
    raised = pipe.model.get_outputs_for_camera(cam)
    for k in before:
        assert torch.equal(before[k], after[k]) and torch.equal(before[k], raised[k]), k


def test_dataset_and_interpolate_subcommands(world, capsys):
    from umhsnerf import render

    root, pipe = world["root"], world["pipe"]
    common = ["--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"), *FLAGS]
    capsys.readouterr()
    got = render.main(["dataset", *common, "--output-path", str(root / "ds"), "--split", "test", "--rendered-output-names", "rgb", "depth"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and (got["frames"], got["files"], got["height"], got["width"]) == (2, 4, 24, 32)
    # nerfstudio's layout: <split>/<output name>/<image stem>.png, one file per eval image
    assert sorted(str(p.relative_to(root / "ds")) for p in (root / "ds").rglob("*.png")) == [
        f"test/{name}/r_{i:03d}.png" for name in ("depth", "rgb") for i in range(2)]
    # ... whose rgb is the frame render_camera_path composes for that camera
    eval_cameras = pipe.datamanager.eval_dataset.cameras
    render.render_camera_path(pipe, eval_cameras, root / "ds_path", ["rgb"])
    frames = [_png(root / "ds" / "test" / "rgb" / f"r_{i:03d}.png") for i in range(2)]
    for i in range(2):
        assert frames[i].shape == (24, 32, 3) and np.array_equal(frames[i], _png(root / "ds_path" / f"frame_{i:05d}.png"))
    assert not np.array_equal(frames[0], frames[1])
    # interpolate: 3 poses over the one pair of eval cameras; the ends are the cameras themselves
    got = render.main(["interpolate", *common, "--output-path", str(root / "ip"), "--interpolation-steps", "3", "--pose-source", "eval"])
    assert got["frames"] == 3 and sorted(p.name for p in (root / "ip").iterdir()) == [f"frame_{i:05d}.png" for i in range(3)]
    assert np.array_equal(_png(root / "ip" / "frame_00000.png"), frames[0]) and np.array_equal(_png(root / "ip" / "frame_00002.png"), frames[1])
    middle = _png(root / "ip" / "frame_00001.png")
    assert not np.array_equal(middle, frames[0]) and not np.array_equal(middle, frames[1])
