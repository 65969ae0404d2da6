"""Camera-path rendering end to end on the GPU: a scene on disk (the ``make_scene`` recipe: 24 x 32 frames, 8 bands), a model of 3
classes with ``pred_specular`` trained for three steps, and a path file of three 20 x 28 cameras with two fovs.

Every written frame is compared byte for byte with tests/frame_ref.py applied to a second ``get_outputs_for_camera_ray_bundle`` of the
same rays (inference is deterministic: tests/test_hip_seg.py relies on it for its checkpoint round trip), and the path's rays bit for
bit with the float32 oracle's and with the ray generator fed the intrinsics worked out by hand: there is no tolerance anywhere but on
``pixel_area``, which keeps the relative bound tests/test_hip_data.py gives it."""
import json
import math

import numpy as np
import pytest
import torch

import frame_ref as R
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
NAMES = ["rgb", "abundances_0", "wv_3", "residual_2", "depth", "accumulation", "seg_pred"]
FLAGS = ["--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"]


def _datamanager(root, seed):
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig

    return UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=root), train_num_rays_per_batch=1024), device=DEV,
                           num_classes=3, seed=seed)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Scene, trained pipeline, path file, and ONE ``render_camera_path`` run that the tests below share."""
    from test_hip_distortion import _look_at_origin, make_scene
    from umhsnerf.render import load_camera_path, render_camera_path
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    root = tmp_path_factory.mktemp("render")
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2,
                                            datamanager=_datamanager(scene, 9))
    for step in range(3):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    rng = np.random.default_rng(11)
    path = {"camera_type": "perspective", "render_height": H, "render_width": W, "fps": 24, "seconds": 0.125,
            "camera_path": [{"camera_to_world": _look_at_origin(rng).reshape(-1).tolist(), "fov": fov, "aspect": W / H} for fov in FOVS]}
    (root / "path.json").write_text(json.dumps(path))
    cameras, _ = load_camera_path(root / "path.json", device=DEV)
    pipe.train()
    result = render_camera_path(pipe, cameras, root / "out", NAMES, cube_names=["spectral", "abundances"])
    assert pipe.training and pipe.model.training  # train() is restored
    return dict(root=root, scene=scene, pipe=pipe, path=path, cameras=cameras, result=result)


def _outputs(world, i, **kw):
    pipe = world["pipe"]
    pipe.eval()
    try:
        return pipe.model.get_outputs_for_camera_ray_bundle(world["cameras"].generate_rays(i, keep_shape=True), **kw)
    finally:
        pipe.train()


def _reference_frame(outputs, names=NAMES, lut_name="default", normalize=False, invert=False, cmin=0.0, cmax=1.0, planes=None):
    """frame_ref applied to an output dict: the panel rules of umhsnerf/render.py restated on numpy arrays."""
    from umhsnerf.utils import colormaps

    host = {k: v.float().cpu().numpy().reshape(H * W, -1) for k, v in outputs.items()}
    columns = {"wv": "spectral", "abundances": "abundances", "residual": "specular"}
    panels = []
    for name in names:
        prefix, _, index = name.rpartition("_")
        rows, ch = (host[columns[prefix]], int(index)) if prefix in columns else (host[name], 0)
        p = dict(kind=R.RGB if prefix not in columns and rows.shape[1] == 3 else R.SCALAR, rows=rows, channel=ch, range=None, acc=None,
                 normalize=normalize, invert=invert, cmin=cmin, cmax=cmax)
        if "depth" in name:
            lo, hi = planes if planes else (rows[:, 0].min(), rows[:, 0].max())
            p.update(kind=R.DEPTH, range=np.array([lo, hi], dtype=np.float32), acc=host["accumulation"][:, 0], normalize=False)
        elif p["kind"] == R.SCALAR and normalize:
            p["range"] = np.array([rows[:, ch].min(), rows[:, ch].max()], dtype=np.float32)
        panels.append(p)
    return R.compose(panels, colormaps.table(lut_name), H, W)


def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path))


def test_camera_path_rays(world):
    """The path's cameras through the HIP ray generator: bit-equal to the generator fed the intrinsics worked out by hand, and the
    float32 oracle's rays within what tests/test_hip_data.py grants the generator (bit equality with the oracle: the next test)."""
    from umhsnerf import ops

    cams, path = world["cameras"], world["path"]
    assert len(cams) == 3 and (cams.height, cams.width) == (H, W) and cams.camera_to_worlds.is_cuda
    c2w = torch.tensor([c["camera_to_world"] for c in path["camera_path"]], dtype=torch.float32).view(3, 4, 4)[:, :3].contiguous()
    intr = torch.tensor([[(H / 2) / math.tan(f * math.pi / 360)] * 2 + [W / 2, H / 2] for f in FOVS], dtype=torch.float32)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for i in range(3):
        rb = cams.generate_rays(i)
        assert rb.origins.shape == (H, W, 3) and rb.directions.shape == (H, W, 3)
        idx = torch.stack([torch.full_like(yy, i), yy, xx], -1).reshape(-1, 3).contiguous()
        o, d, area, nrm = ops.raygen(idx.to(DEV), c2w.to(DEV), intr.to(DEV), want_area=True, want_norm=True)
        assert torch.equal(rb.origins.view(-1, 3), o) and torch.equal(rb.directions.view(-1, 3), d)
        assert torch.equal(rb.pixel_area.view(-1, 1), area) and torch.equal(rb.metadata["directions_norm"].view(-1, 1), nrm)
        ro, rd, rarea, rn = T.generate_rays(idx, c2w, intr)
        assert torch.equal(o.cpu(), ro)
        err = float((d.cpu() - rd).abs().max())
        print(f"camera {i}: directions differ from the float32 oracle by at most {err:.3e}")
        torch.testing.assert_close(d.cpu(), rd, rtol=0, atol=2e-7)
        torch.testing.assert_close(nrm.cpu(), rn, rtol=2e-7, atol=0)
        torch.testing.assert_close(area.cpu(), rarea, rtol=2e-3, atol=0)
    assert not torch.equal(cams.generate_rays(0).directions, cams.generate_rays(1).directions)


def test_camera_path_rays_are_bit_equal_to_the_float32_oracle(world):
    """``load_camera_path(...).generate_rays(i)`` against ``oracle/torch_ref.generate_rays`` in float32: origins, directions and
    ``directions_norm`` bit for bit.  (The ray generator sums the squares of a direction as ``torch.linalg.vector_norm`` does --
    ``v0 * v0``, then a fused multiply-add per component; with a plain float32 sum 208, 165 and 175 of the 1,680 direction components
    of these three cameras were one unit in the last place, 1.192e-07, off the oracle.)  ``pixel_area`` is a difference of nearly equal
    unit vectors and keeps the relative bound of tests/test_hip_data.py (test_camera_path_rays)."""
    cams = world["cameras"]
    c2w, intr = cams.camera_to_worlds.cpu(), cams.intrinsics.cpu()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for i in range(3):
        rb = cams.generate_rays(i)
        idx = torch.stack([torch.full_like(yy, i), yy, xx], -1).reshape(-1, 3).contiguous()
        ro, rd, _, rn = T.generate_rays(idx, c2w, intr)
        d, n = rb.directions.view(-1, 3).cpu(), rb.metadata["directions_norm"].view(-1, 1).cpu()
        print(f"camera {i}: {int((d != rd).sum())} of {d.numel()} direction components and {int((n != rn).sum())} of {n.numel()} norms "
              f"differ from the float32 oracle, by at most {float((d - rd).abs().max()):.3e}")
        assert torch.equal(rb.origins.view(-1, 3).cpu(), ro)
        assert torch.equal(d, rd) and torch.equal(n, rn)


def test_written_frames_equal_the_reference_composition(world):
    out, res = world["root"] / "out", world["result"]
    assert res["frames"] == 3 and res["seconds"] > 0 and res["fps"] == pytest.approx(3 / res["seconds"])
    assert res["num_rays_per_sec"] == pytest.approx(3 * H * W / res["seconds"])
    assert sorted(p.name for p in out.iterdir()) == sorted(
        [f"frame_{i:05d}.png" for i in range(3)] + [f"{k}_{i:05d}.npy" for k in ("spectral", "abundances") for i in range(3)])
    frames = []
    for i in range(3):
        outputs = _outputs(world, i)
        got = _png(out / f"frame_{i:05d}.png")
        assert got.dtype == np.uint8 and got.shape == (H, len(NAMES) * W, 3)
        assert np.array_equal(got, _reference_frame(outputs)), i
        for k in ("spectral", "abundances"):
            cube = np.load(out / f"{k}_{i:05d}.npy")
            assert cube.dtype == np.float32 and cube.shape == tuple(outputs[k].shape) and np.array_equal(cube, outputs[k].cpu().numpy())
        frames.append(got)
    assert not np.array_equal(frames[0], frames[1])  # three views, not one
    colours = {name: len(np.unique(frames[0][:, k * W:(k + 1) * W].reshape(-1, 3), axis=0)) for k, name in enumerate(NAMES)}
    print("distinct colours per panel of frame 0:", colours)
    assert all(colours[k] > 1 for k in ("rgb", "wv_3", "depth", "accumulation")), colours  # the comparison above is of pictures


def test_compose_frame_options(world):
    """Colormap options and depth planes through ``compose_frame`` itself, on one camera's outputs."""
    from umhsnerf.render import ColormapOptions, compose_frame

    outputs = _outputs(world, 1)
    names = ["wv_0", "depth", "seg_raw", "abundances_2", "rgb"]
    for opt, planes in ((ColormapOptions("viridis", normalize=True), None), (ColormapOptions("gray", invert=True), (0.5, 4.0)),
                        (ColormapOptions("magma", True, 0.2, 0.9, True), (None, 3.0))):
        got = compose_frame(outputs, names, opt, *(planes or (None, None)))
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (H, len(names) * W, 3)
        depth = outputs["depth"].cpu().numpy()
        lo, hi = planes or (None, None)
        ref_planes = (np.float32(depth.min() if lo is None else lo), np.float32(depth.max() if hi is None else hi))
        want = _reference_frame(outputs, names, opt.colormap, opt.normalize, opt.invert, opt.colormap_min, opt.colormap_max, ref_planes)
        assert np.array_equal(got.cpu().numpy(), want), opt
    with pytest.raises(ValueError, match="usable names: .*wv_0\\.\\.wv_7"):
        compose_frame(outputs, ["rgb", "spectral"])
    # more panels than one launch takes (the reference's wv_0 ... wv_20): 8 bands twice, the residuals and rgb = 25 panels
    many = [f"wv_{i}" for i in range(8)] * 2 + [f"residual_{i}" for i in range(8)] + ["rgb"]
    sentinel = torch.full((H * len(many) * W * 3 + 7,), 0xA5, dtype=torch.uint8, device=DEV)
    got = compose_frame(outputs, many, out=sentinel[5:-2])
    assert got.data_ptr() == sentinel.data_ptr() + 5 and tuple(got.shape) == (H, len(many) * W, 3)
    assert np.array_equal(got.cpu().numpy(), _reference_frame(outputs, many))
    assert bool((sentinel[:5] == 0xA5).all()) and bool((sentinel[-2:] == 0xA5).all())
    assert torch.equal(compose_frame(outputs, many), got)


def test_output_names_filter_returns_those_keys_with_the_same_bits(world):
    full = _outputs(world, 2)
    some = _outputs(world, 2, output_names=["spectral", "rgb"])
    assert set(some) == {"spectral", "rgb"} and "wv_0" in full and "abundances_0" in full
    for k in some:
        assert some[k].shape == full[k].shape and torch.equal(some[k], full[k]), k
    again = _outputs(world, 2, output_names=None)
    assert list(again) == list(full) and all(torch.equal(again[k], full[k]) for k in full)


def test_render_restores_the_mode_it_found_and_refuses_bad_names(world, tmp_path):
    from umhsnerf.render import render_camera_path

    pipe, cams = world["pipe"], world["cameras"]
    pipe.eval()
    try:
        res = render_camera_path(pipe, cams, tmp_path / "jpg", ["rgb"], image_format="jpeg", jpeg_quality=90)
        assert not pipe.training and res["frames"] == 3
    finally:
        pipe.train()
    from PIL import Image

    with Image.open(tmp_path / "jpg" / "frame_00002.jpg") as im:
        assert im.format == "JPEG" and im.size == (W, H)
    for bad in ("spectral", "wv_8", "nope"):  # 8 channels; no such band; no such output
        with pytest.raises(ValueError, match="usable names"):
            render_camera_path(pipe, cams, tmp_path / "bad", ["rgb", bad])
        assert pipe.training
    with pytest.raises(ValueError, match="image_format"):
        render_camera_path(pipe, cams, tmp_path / "bad", ["rgb"], image_format="gif")


def test_the_command_line_renders_the_same_files_from_a_checkpoint(world, capsys):
    from umhsnerf import render

    root, pipe = world["root"], world["pipe"]
    torch.save({"step": 3, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    capsys.readouterr()
    got = render.main(["camera-path", "--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"),
                       "--camera-path-filename", str(root / "path.json"), "--output-path", str(root / "cli"), "--rendered-output-names",
                       *NAMES, "--cube-output-names", "spectral", "abundances", *FLAGS])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got["frames"] == 3 and (got["height"], got["width"], got["panels"]) == (H, W, len(NAMES))
    assert sorted(p.name for p in (root / "cli").iterdir()) == sorted(p.name for p in (root / "out").iterdir())
    for p in (root / "out").iterdir():
        a, b = ((_png(p), _png(root / "cli" / p.name)) if p.suffix == ".png" else (np.load(p), np.load(root / "cli" / p.name)))
        assert np.array_equal(a, b), p.name
    # half size: the same cameras at 10 x 14
    half = render.main(["camera-path", "--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"),
                        "--camera-path-filename", str(root / "path.json"), "--output-path", str(root / "half"), "--rendered-output-names",
                        "rgb", "depth", "--downscale-factor", "2", *FLAGS])
    assert (half["height"], half["width"]) == (H // 2, W // 2) and _png(root / "half" / "frame_00000.png").shape == (H // 2, 2 * (W // 2), 3)
