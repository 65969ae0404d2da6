"""Scene statistics on the GPU: csrc/umhs_statistics.hip per element against float64 (tests/statistics_f64.py), the outputs of
``UMHSModel.scene_statistics_context`` on the small trained pipeline of tests/test_hip_library.py (``make_scene(B=8)``, 3 classes, three
steps at 1024 rays, 20 x 28 path frames), and ``--scene-statistics`` on the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import rays_f64 as RF
import statistics_f64 as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
BASE_FLAGS = ["--num-classes", "3", "--temperature", "0.4", "--background-color", "black"]
CROP = {"crop_center": [0.1, -0.05, 0.2], "crop_scale": [0.9, 0.6, 1.2], "crop_rot": [0.3, -0.2, 0.5], "crop_bg_color": {"r": 38, "g": 120, "b": 255}}
_WORST = {}


def _report(key, report):
    _WORST[key] = report
    with open(os.path.join(RF.report_dir(ROOT), "statistics_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernels
# ------------------------------------------------------------------------------------------------------------------------------ #
def _gram(case, shift=None, rows=slice(None), acc=None, x=None):
    from umhsnerf import ops

    B = case["B"]
    acc = torch.zeros(1 + B + B * B, dtype=torch.float64, device=DEV) if acc is None else acc
    x = case["x"].to(DEV)[rows] if x is None else x
    ops.gram_accumulate(x, (case["shift"] if shift is None else shift).to(DEV), acc, case["accumulation"].to(DEV)[rows])
    return acc


def _project(case, x=None, want_score=True):
    from umhsnerf import ops

    image = ops.library_prepare(case["W"].to(DEV))
    return ops.spectral_project(case["x"].to(DEV) if x is None else x, case["mean"].to(DEV), image, case["K"], case["P"], want_score)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("c", SF.GRAM_CASES, ids=SF.gram_id)
def test_gram_is_within_the_bound_of_float64_and_repeats_bit_for_bit(c):
    case, r64 = SF.gram_reference(*c)
    acc = _gram(case)
    report = {}
    fails = SF.check_gram(case, acc, r64, report=report)
    print(SF.gram_id(c), {k: round(v, 3) for k, v in report.items()})
    _report("gram " + SF.gram_id(c), report)
    assert not fails, fails
    assert _same_bits(acc, _gram(case))
    if c[0] == 0:  # R = 0 returns OK and leaves acc as it was
        kept = torch.arange(1 + c[1] + c[1] ** 2, dtype=torch.float64, device=DEV)
        assert _same_bits(_gram(case, acc=kept.clone()), kept)
    else:  # invalid rows are absent: the same bits with those rows' values replaced (the NaN and Inf rows stay invalid by their flag)
        x = case["x"].clone()
        x[~case["valid"]] = 1e30
        a = case["accumulation"].clone()
        a[~case["valid"]] = 0.5
        assert _same_bits(acc, _gram(dict(case, accumulation=a), x=x.to(DEV)))


def test_two_calls_add_up_and_the_shift_does_not_matter_beyond_rounding():
    case, r64 = SF.gram_reference(*SF.SPLIT_CASE)
    acc = _gram(case, rows=slice(0, SF.SPLIT_AT))
    first = float(acc[0])
    acc = _gram(case, rows=slice(SF.SPLIT_AT, None), acc=acc)
    report = {}
    assert not SF.check_gram(case, acc, r64, report=report), report
    assert first == int(case["valid"][:SF.SPLIT_AT].sum()) and float(acc[0]) == r64["n"]
    # the statement's own float64-of-chunks result, replayed in float32 on the CPU with the split's chunking, obeys the same rule
    want = SF.gram_oracle(case, splits=[SF.SPLIT_AT])
    assert not SF.check_gram(case, want, r64)
    _report("gram two calls", report)
    # shift invariance: from shift = 0 and from shift ~ mean the covariance meets its own rule against float64
    zero = torch.zeros(case["B"])
    report0 = {}
    acc0 = _gram(case, shift=zero)
    assert not SF.check_gram(case, acc0, SF.gram_ref64(case, zero), report=report0), report0
    _report("gram shift 0", report0)
    from umhsnerf.statistics import SceneStatistics

    wl = list(range(case["B"]))
    a, b = (SceneStatistics.from_accumulator(t.cpu().numpy(), s.numpy(), wl) for t, s in ((acc, case["shift"]), (acc0, zero)))
    mean, cov = SF.stats64(case["x"][case["valid"]])
    scale = np.abs(cov).max()
    assert np.abs(a.covariance - cov).max() < 1e-5 * scale and np.abs(b.covariance - cov).max() < 1e-3 * scale
    assert np.abs(a.mean - mean).max() < 1e-5 and np.abs(b.mean - mean).max() < 1e-5


def test_strided_and_unaligned_rows_give_the_same_bits_and_nothing_past_a_row_or_an_output_is_touched():
    from umhsnerf import _hip, ops

    case, _ = SF.gram_reference(*SF.STRIDED_CASE)
    R, B = case["R"], case["B"]
    want = _gram(case)
    wide = torch.full((R, B + 3), float("nan"), device=DEV)  # NaN in the columns past B: reading one would invalidate the row
    wide[:, :B] = case["x"].to(DEV)
    assert _same_bits(want, _gram(case, x=wide[:, :B]))
    flat = torch.full((R * (B + 3) + 1,), float("nan"), device=DEV)
    off = flat[1:].view(R, B + 3)
    off[:, :B] = case["x"].to(DEV)
    assert off.data_ptr() % 16 == 4
    assert _same_bits(want, _gram(case, x=off[:, :B]))
    # the accumulator inside guards
    guarded = torch.full((8 + 1 + B + B * B + 8,), -7.0, dtype=torch.float64, device=DEV)
    inner = guarded[8:-8]
    inner.zero_()
    _gram(case, acc=inner)
    assert _same_bits(inner, want) and bool((guarded[:8] == -7.0).all()) and bool((guarded[-8:] == -7.0).all())
    # the projection: the same three layouts, and its outputs inside guards
    pc, _ = SF.project_reference(130, 65, 33, 33)
    y, s = _project(pc)
    wide = torch.full((130, 65 + 3), float("nan"), device=DEV)
    wide[:, :65] = pc["x"].to(DEV)
    flat = torch.full((130 * 68 + 1,), float("nan"), device=DEV)
    off = flat[1:].view(130, 68)
    off[:, :65] = pc["x"].to(DEV)
    for x in (wide[:, :65], off[:, :65]):
        y2, s2 = _project(pc, x=x)
        assert _same_bits(y, y2) and _same_bits(s, s2)
    image = ops.library_prepare(pc["W"].to(DEV))
    out = torch.full((16 + 130 * 33 + 16,), -7.0, device=DEV)
    sc = torch.full((16 + 130 + 16,), -7.0, device=DEV)
    x = pc["x"].to(DEV)
    _hip.check(_hip.lib().umhs_spectral_project(_hip.ptr(x), 65, 130, _hip.ptr(pc["mean"].to(DEV)), _hip.ptr(image), 33, 65, 33,
                                                _hip.C.c_void_p(out.data_ptr() + 64), _hip.C.c_void_p(sc.data_ptr() + 64), _hip.stream()),
               "umhs_spectral_project")
    assert _same_bits(out[16:-16].view(130, 33), y) and _same_bits(sc[16:-16], s)
    assert bool((out[:16] == -7.0).all()) and bool((out[-16:] == -7.0).all()) and bool((sc[:16] == -7.0).all()) and bool((sc[-16:] == -7.0).all())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.spectral_project(pc["x"], pc["mean"].to(DEV), image, 33, 33)


@pytest.mark.parametrize("c", SF.PROJECT_CASES, ids=SF.project_id)
def test_projection_is_within_the_bound_of_float64_and_repeats_bit_for_bit(c):
    case, r64 = SF.project_reference(*c)
    y, score = _project(case)
    report = {}
    fails = SF.check_project(case, y, score, r64, report=report)
    print(SF.project_id(c), {k: round(v, 3) for k, v in report.items()})
    _report("project " + SF.project_id(c), report)
    assert not fails, fails
    y2, score2 = _project(case)
    assert _same_bits(y, y2) and _same_bits(score, score2)
    dead = ~case["finite"]
    if int(dead.sum()):  # exact zeros, in bits
        assert bool((y.cpu()[dead].view(torch.int32) == 0).all()) and bool((score.cpu()[dead].view(torch.int32) == 0).all())
    y3, none = _project(case, want_score=False)  # the score is optional and does not change the components
    assert none is None and _same_bits(y, y3)


@pytest.mark.parametrize("c", SF.E2E_CASES, ids=lambda c: f"R{c[0]}-B{c[1]}-C{c[2]}")
def test_end_to_end_every_planted_row_ranks_above_every_background_row(c):
    from umhsnerf.statistics import StatisticsAccumulator

    ref = SF.e2e_reference(*c)
    x, a = ref["x"].to(DEV), ref["accumulation"].to(DEV)
    accumulator = StatisticsAccumulator(ref["B"], DEV, ref["shift"])
    accumulator.add(x[:900], a[:900])
    accumulator.add(x[900:], a[900:])
    stats = accumulator.result(list(range(ref["B"])))
    assert stats.n == int(ref["valid"].sum())
    np.testing.assert_allclose(stats.mean, ref["mean64"], atol=1e-5)
    assert np.abs(stats.covariance - ref["cov64"]).max() < 1e-4 * np.abs(ref["cov64"]).max()
    out = stats.frame_outputs(x, a[:, None], components=3)
    score = out["rx_score"][:, 0].cpu().double()
    background = ref["valid"] & ~ref["planted"]
    assert float(score[ref["planted"]].min()) > float(score[background].max())
    assert bool((score[~ref["valid"]] == 0).all()) and bool((out["rx_mask"][:, 0].cpu()[ref["planted"]] == 1).all())
    np.testing.assert_allclose(score[ref["valid"]].numpy(), ref["score64"][ref["valid"]].numpy(), rtol=2e-2)


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
NAMES = ("rx_score", "rx_mask", "pca_0", "pca_1", "pca_2", "pca_rgb")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from library_f64 import make_library
    from test_hip_distortion import _look_at_origin, make_scene
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.render import load_camera_path
    from umhsnerf.statistics import StatisticsAccumulator, first_frame_shift
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("statistics")
    torch.manual_seed(0)
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    # make_scene's captured cubes hold one constant spectrum, whose covariance is zero: give the captured side something to have
    # statistics of -- mixtures of three smooth endmembers plus noise, the recipe of statistics_f64.make_rows without its bad rows
    g = torch.Generator().manual_seed(21)
    E = make_library(3, 8, g).double()
    for cube in sorted(scene.glob("hs_*/r_*.npy")):
        w = -torch.log(torch.rand(24 * 32, 3, generator=g, dtype=torch.float64).clamp_min(1e-12))
        x = (w / w.sum(1, keepdim=True)) @ E + 0.01 * torch.randn(24 * 32, 8, generator=g, dtype=torch.float64)
        np.save(cube, x.float().reshape(24, 32, 8).numpy())
    dm = UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=scene), train_num_rays_per_batch=1024), device=DEV,
                         num_classes=3, seed=9)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=False, temperature=0.4, background_color="black")
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
    (root / "path.json").write_text(json.dumps(path))
    cameras, _ = load_camera_path(path, device=DEV)
    wl = [float(w) for w in meta["wavelengths"]]
    # the statistics of the captured training stack
    stack = dm.train_split.hs_image
    accumulator = StatisticsAccumulator(8, DEV, first_frame_shift(stack[0].to(DEV)))
    for i in range(stack.shape[0]):
        accumulator.add(stack[i].to(DEV).float())
    stats = accumulator.result(wl)
    stats.save(root / "stats.npz")
    return dict(root=root, scene=scene, pipe=pipe, cameras=cameras, wl=wl, stats=stats, stack=stack)


def _frame(world, stats=None, camera=1, output_names=None, crop=False, **kw):
    from umhsnerf.render import parse_crop

    model = world["pipe"].model
    if crop:  # (the untrained scene is opaque everywhere: a crop box leaves rays that accumulate nothing)
        rb = world["cameras"].generate_rays(camera, keep_shape=True, obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane)
    else:
        rb = world["cameras"].generate_rays(camera, keep_shape=True)
    with model.scene_statistics_context(stats, **kw):
        return model.get_outputs_for_camera_ray_bundle(rb, output_names=output_names)


def test_the_accumulated_statistics_are_the_float64_ones(world):
    x = world["stack"].reshape(-1, 8).cpu()
    mean, cov = SF.stats64(x)
    s = world["stats"]
    assert s.n == x.shape[0]
    np.testing.assert_allclose(s.mean, mean, atol=1e-5)
    assert np.abs(s.covariance - cov).max() < 1e-4 * np.abs(cov).max()


def test_outside_the_context_nothing_changes_and_inside_only_the_asked_for_keys_are_added(world):
    plain = _frame(world)
    assert int(plain["num_samples_per_ray"].sum()) > 0 and not any(k in plain for k in NAMES)
    got = _frame(world, world["stats"])
    assert [k for k in got if k not in NAMES] == list(plain) and all(k in got for k in NAMES)
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    assert {k: tuple(got[k].shape) for k in NAMES} == {**{k: (H, W, 1) for k in NAMES[:5]}, "pca_rgb": (H, W, 3)}
    five = _frame(world, world["stats"], components=5)
    assert [k for k in five if k not in plain] == ["rx_score", "rx_mask", "pca_0", "pca_1", "pca_2", "pca_3", "pca_4", "pca_rgb"]
    assert torch.equal(five["pca_1"], got["pca_1"]) and torch.equal(five["rx_score"], got["rx_score"])
    two = _frame(world, world["stats"], components=2)
    assert "pca_rgb" not in two and "pca_1" in two and "pca_2" not in two
    # computed only when asked for
    some = _frame(world, world["stats"], output_names=["rgb", "depth"])
    assert sorted(some) == ["depth", "rgb"]
    some = _frame(world, world["stats"], output_names=["pca_rgb", "rx_score"])
    assert sorted(some) == ["pca_rgb", "rx_score"] and torch.equal(some["pca_rgb"], got["pca_rgb"])
    with pytest.raises(ValueError, match="components"):
        _frame(world, world["stats"], output_names=["pca_rgb"], components=2)
    with pytest.raises(ValueError, match="components"):
        _frame(world, world["stats"], output_names=["pca_3"])
    assert world["pipe"].model._scene_statistics is None


def test_the_outputs_are_frame_outputs_of_the_frames_own_spectral_and_empty_pixels_are_zero(world):
    from umhsnerf.statistics import chi_square_quantile

    stats = world["stats"]
    seen = 0
    for crop in (False, True):
        got = _frame(world, stats, crop=crop, threshold=11.0)
        want = stats.frame_outputs(got["spectral"], got["accumulation"], 3, 11.0)
        assert sorted(want) == sorted(NAMES)
        for k in NAMES:
            assert torch.equal(got[k], want[k]), k
        empty = got["accumulation"][..., 0] <= 0.5
        seen += int(empty.sum())
        assert bool((got["rx_score"][empty] == 0).all()) and bool((got["pca_rgb"][empty] == 0).all()) and bool((got["pca_0"][empty] == 0).all())
        assert torch.equal(got["rx_mask"], (got["rx_score"] > 11.0).float())
        # by hand, from the op: the score and the components of the rendered pixels
        y, score = _project(dict(W=torch.from_numpy(stats.whitening()[0]).float(), mean=torch.from_numpy(stats.mean).float(), K=8, P=3),
                            x=got["spectral"].reshape(-1, 8))
        rendered = ~empty.reshape(-1)
        assert torch.equal(got["rx_score"].reshape(-1)[rendered], score[rendered])
        assert torch.equal(got["pca_rgb"].reshape(-1, 3)[rendered], (0.5 + y[rendered] / 6.0).clamp(0.0, 1.0))
        assert bool((got["rx_score"] >= 0).all()) and float(got["pca_rgb"].min()) >= 0.0 and float(got["pca_rgb"].max()) <= 1.0
    assert seen > 100
    default = _frame(world, stats)
    assert torch.equal(default["rx_mask"], (default["rx_score"] > chi_square_quantile(8, 1e-3)).float())


def test_under_material_edits_the_edited_scene_is_scored(world):
    from umhsnerf.materials import load_material_edits

    model, stats = world["pipe"].model, world["stats"]
    edits = load_material_edits({"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}]}, 3, 8, False)
    rb = world["cameras"].generate_rays(1, keep_shape=True)
    with model.material_edits_context(edits), model.scene_statistics_context(stats):
        got = model.get_outputs_for_camera_ray_bundle(rb)
    plain = _frame(world, stats)
    assert not torch.equal(got["spectral"], plain["spectral"])
    want = stats.frame_outputs(got["spectral"], got["accumulation"])
    for k in NAMES:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["rx_score"], plain["rx_score"])


def test_refusals_and_the_state_after_an_exception(world):
    from umhsnerf.statistics import SceneStatistics
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model, stats = world["pipe"].model, world["stats"]
    rgb = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": world["wl"], "num_classes": 3}, seed=1)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with rgb.scene_statistics_context(stats):
            pass
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="model.eval"):
            with model.scene_statistics_context(stats):
                model.get_outputs_for_camera_ray_bundle(rb)
    finally:
        model.eval()
    assert model._scene_statistics is None
    with pytest.raises(KeyError):
        with model.scene_statistics_context(stats, 2, 5.0):
            assert model._scene_statistics["components"] == 2 and model._scene_statistics["threshold"] == 5.0
            raise KeyError("inside")
    assert model._scene_statistics is None
    with pytest.raises(ValueError, match="wavelengths"):
        with model.scene_statistics_context(SceneStatistics(10, np.zeros(5), np.eye(5), [1.0, 2.0, 3.0, 4.0, 5.0])):
            pass


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _model_flags(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *BASE_FLAGS]


def test_compute_then_render_dataset_with_the_statistics(world, capsys):
    from PIL import Image

    from umhsnerf import render, statistics

    root = world["root"]
    got = statistics.main(["compute", *_model_flags(world), "--source", "captured", "--split", "train", "--output", str(root / "cli.npz")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got["n"] == world["stats"].n and got["bands"] == 8 and len(got["eigenvalues"]) == 8 == len(got["explained_variance"])
    assert got["eigenvalues"] == sorted(got["eigenvalues"], reverse=True) and 0.99 < sum(got["explained_variance"]) <= 1.0 + 1e-9
    assert 0 <= got["eigenvalues_at_floor"] < 8
    loaded = statistics.SceneStatistics.load(root / "cli.npz", world["wl"])
    assert np.array_equal(loaded.covariance, world["stats"].covariance) and np.array_equal(loaded.mean, world["stats"].mean)
    rendered = statistics.main(["compute", *_model_flags(world), "--source", "rendered", "--split", "train", "--output", str(root / "rendered.npz")])
    capsys.readouterr()
    assert 2 <= rendered["n"] <= got["n"] and rendered["bands"] == 8
    out = render.main(["dataset", *_model_flags(world), "--split", "test", "--output-path", str(root / "ds"), "--scene-statistics",
                       str(root / "cli.npz"), "--rendered-output-names", "rgb", "pca_rgb", "rx_score"])
    capsys.readouterr()
    assert out["frames"] >= 1 and out["files"] == 3 * out["frames"] and out["scene_statistics"] == str(root / "cli.npz")
    for name in ("rgb", "pca_rgb", "rx_score"):
        files = sorted((root / "ds" / "test" / name).glob("*.png"))
        assert len(files) == out["frames"]
        assert np.asarray(Image.open(files[0])).shape[2] == 3
    assert world["pipe"].model._scene_statistics is None


def test_eval_with_the_statistics_prints_the_new_keys(world, capsys):
    from umhsnerf import eval as umhs_eval

    got = umhs_eval.main([*_model_flags(world), "--scene-statistics", str(world["root"] / "stats.npz")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "psnr" in got
    for key in ("rx_mean", "rx_exceed", "rx_captured_mean", "rx_captured_exceed"):
        assert key in got and np.isfinite(got[key]), key
    assert got["rx_captured_mean"] > 0 and got["rx_mean"] > 0 and 0 <= got["rx_exceed"] <= 1 and 0 <= got["rx_captured_exceed"] <= 1
