"""Spectral library matching on the GPU: csrc/umhs_library.hip per element against float64 (tests/library_f64.py), the outputs of
``UMHSModel.spectral_library_context`` on the small trained pipeline of tests/test_hip_crop_render.py (``make_scene(B=8)``, 3 classes,
three steps at 1024 rays, 20 x 28 path frames), and ``--spectral-library`` on the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import library_f64 as LF
import rays_f64 as RF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
BASE_FLAGS = ["--num-classes", "3", "--temperature", "0.4", "--background-color", "black"]
CROP = {"crop_center": [0.1, -0.05, 0.2], "crop_scale": [0.9, 0.6, 1.2], "crop_rot": [0.3, -0.2, 0.5], "crop_bg_color": {"r": 38, "g": 120, "b": 255}}
_WORST = {}


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernel
# ------------------------------------------------------------------------------------------------------------------------------ #
def _match(spectra, unit):
    from umhsnerf import ops

    image = ops.library_prepare(unit.to(DEV))
    return ops.library_match(spectra, image, unit.shape[0])


@pytest.mark.parametrize("c", LF.CASES, ids=LF.case_id)
def test_match_is_within_the_bound_of_float64_and_repeats_bit_for_bit(c):
    case, r64 = LF.reference(*c)
    s = case["spectra"].to(DEV)
    index, cos = _match(s, case["unit"])
    report = {}
    fails = LF.check_match(case, index, cos, r64, report=report)
    print(LF.case_id(c), {k: round(v["worst"], 3) for k, v in report.items()})
    _WORST[LF.case_id(c)] = {k: v["worst"] for k, v in report.items()}
    with open(os.path.join(RF.report_dir(ROOT), "library_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)
    assert not fails, fails
    assert index.dtype == torch.int32 and cos.dtype == torch.float32 and tuple(index.shape) == tuple(cos.shape) == (c[0], 2)
    again = _match(s, case["unit"])
    assert torch.equal(index, again[0]) and torch.equal(cos.view(torch.int32), again[1].view(torch.int32))


def test_exact_properties():
    case, _ = LF.reference(300, 31, 17)
    index, cos = (t.cpu() for t in _match(case["spectra"].to(DEV), case["unit"]))
    a, b = case["dup"]
    hit = index[:, 0] == a
    assert int(hit.sum()) >= 3 and bool((index[hit, 1] == b).all())  # identical rows: the smaller index first, the other right behind
    assert torch.equal(cos[hit, 0].view(torch.int32), cos[hit, 1].view(torch.int32))
    assert not bool((index[:, 0] == b).any())
    dead = case["degenerate"]
    assert int(dead.sum()) >= 4 and bool((index[dead] == -1).all()) and bool((cos[dead].view(torch.int32) == 0).all())
    assert bool((index[~dead] >= 0).all()) and bool((index[:, 0] != index[:, 1])[~dead].all())
    # one band, one entry
    i1, c1 = _match(torch.tensor([[0.7]], device=DEV), torch.ones(1, 1))
    assert i1.tolist() == [[0, -1]] and c1.tolist() == [[1.0, -1.0]]
    # positive rows at B = 1 against five identical entries: every cosine is exactly 1 and the first two win
    i5, c5 = _match(torch.rand(70, 1, device=DEV) + 0.1, torch.ones(5, 1))
    assert bool((i5.cpu() == torch.tensor([0, 1], dtype=torch.int32)).all()) and bool((c5 == 1.0).all())
    # a position-independent value: the same row at entry 3 and at entry 40 (another tile, another accumulator row)
    unit = LF.unit_rows(LF.make_library(70, 31, torch.Generator().manual_seed(5)))
    unit[40] = unit[3]
    s = (unit[3] * 2.0 + 0.01 * torch.randn(50, 31, generator=torch.Generator().manual_seed(6))).to(DEV)
    i2, c2 = _match(s, unit)
    assert i2.cpu().tolist() == [[3, 40]] * 50 and torch.equal(c2[:, 0].view(torch.int32), c2[:, 1].view(torch.int32))


def test_strided_and_unaligned_rows_give_the_same_bits_and_nothing_past_a_row_is_read():
    from umhsnerf import _hip, ops

    case, _ = LF.reference(130, 65, 33)
    R, B, L = case["R"], case["B"], case["L"]
    unit = case["unit"].to(DEV)
    image = ops.library_prepare(unit)
    want = ops.library_match(case["spectra"].to(DEV), image, L)
    wide = torch.full((R, B + 3), float("nan"), device=DEV)  # NaN in the columns past B: reading one would poison the row
    wide[:, :B] = case["spectra"].to(DEV)
    got = ops.library_match(wide[:, :B], image, L)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    flat = torch.full((R * (B + 3) + 1,), float("nan"), device=DEV)
    off = flat[1:].view(R, B + 3)
    off[:, :B] = case["spectra"].to(DEV)
    assert off.data_ptr() % 16 == 4
    got = ops.library_match(off[:, :B], image, L)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert int(_hip.lib().umhs_library_image_bytes(L, B)) == image.numel() * 4 >= L * B * 4
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.library_match(case["spectra"], image, L)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.library_prepare(case["unit"])


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
NAMES = ("library_raw", "library_pred", "library_angle", "library_margin")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from test_hip_distortion import _look_at_origin, make_scene
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.library import SpectralLibrary
    from umhsnerf.render import load_camera_path
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("library")
    torch.manual_seed(0)
    scene = root / "scene"
    meta = make_scene(scene, B=8)
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
    # the library: the model's own endmember rows, then 29 distractors of the case builder
    wl = [float(w) for w in meta["wavelengths"]]
    E = pipe.model.field.endmembers.detach().cpu().double().numpy()
    spectra = np.concatenate([E, LF.make_library(29, 8, torch.Generator().manual_seed(3)).double().numpy()])
    names = [f"endmember_{c}" for c in range(3)] + [f"distractor_{i}" for i in range(29)]
    np.savez(root / "library.npz", names=np.array(names), wavelengths=np.array(wl), spectra=spectra)
    return dict(root=root, scene=scene, pipe=pipe, cameras=cameras, wl=wl, library=SpectralLibrary.load(root / "library.npz", wl),
                own=SpectralLibrary(names[:3], E, wl))


def _frame(world, library=None, camera=1, output_names=None, max_angle=None, crop=False):
    from umhsnerf.render import parse_crop

    model = world["pipe"].model
    if crop:  # (the untrained scene is opaque everywhere: a crop box leaves rays that accumulate nothing)
        rb = world["cameras"].generate_rays(camera, keep_shape=True, obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane)
    else:
        rb = world["cameras"].generate_rays(camera, keep_shape=True)
    with model.spectral_library_context(library, max_angle):
        return model.get_outputs_for_camera_ray_bundle(rb, output_names=output_names)


def test_outside_the_context_nothing_changes_and_inside_only_the_four_keys_are_added(world):
    plain = _frame(world)
    assert int(plain["num_samples_per_ray"].sum()) > 0 and not any(k in plain for k in NAMES)
    got = _frame(world, world["library"])
    assert [k for k in got if k not in NAMES] == list(plain) and all(k in got for k in NAMES)
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    assert {k: tuple(got[k].shape) for k in NAMES} == {"library_raw": (H, W, 1), "library_pred": (H, W, 3), "library_angle": (H, W, 1),
                                                       "library_margin": (H, W, 1)}
    # computed only when asked for
    some = _frame(world, world["library"], output_names=["rgb", "depth"])
    assert sorted(some) == ["depth", "rgb"]
    some = _frame(world, world["library"], output_names=["library_pred"])
    assert list(some) == ["library_pred"] and torch.equal(some["library_pred"], got["library_pred"])
    assert world["pipe"].model._spectral_library is None


def test_library_raw_is_the_float64_best_and_seg_raw_on_the_models_own_rows(world):
    """Three cameras, each whole (the barely trained scene is opaque: every pixel is rendered) and through a crop box (rays that miss
    it, or cross little of it, accumulate <= 0.5)."""
    seen = {"rendered": 0, "empty": 0, "endmember closest": 0}
    for camera, crop in [(c, k) for c in range(3) for k in (False, True)]:
        plain = _frame(world, camera=camera, crop=crop)
        spec, acc = plain["spectral"].reshape(-1, 8), plain["accumulation"].reshape(-1)
        rendered = (acc > 0.5).cpu()
        seg = plain["seg_raw"].reshape(-1).long().cpu()
        # (a) the model's own dictionary as the library: the operation seg_raw is, so the same answer wherever float64 sees no tie
        own = _frame(world, world["own"], camera=camera, crop=crop)["library_raw"].reshape(-1).long().cpu()
        _, _, tied = RF.cluster_ties(spec, world["pipe"].model.field.endmembers)
        sure = rendered & (tied.sum(1) == 1)
        assert int(sure.sum()) >= 0.9 * int(rendered.sum())
        assert torch.equal(own[sure], seg[sure])
        assert torch.equal(own == -1, ~rendered)
        # (b) with the 29 distractors behind them: the float64 best of all 32 rows, which is seg_raw wherever an endmember is closest
        raw = _frame(world, world["library"], camera=camera, crop=crop)["library_raw"].reshape(-1).long().cpu()
        cos, _, tied = RF.cluster_ties(spec, torch.from_numpy(world["library"].spectra))
        best, sure = cos.argmax(1), rendered & (tied.sum(1) == 1)
        assert int(sure.sum()) >= 0.9 * int(rendered.sum())
        assert torch.equal(raw[sure], best[sure])
        assert torch.equal(raw == -1, ~rendered)
        mine = sure & (best < 3)
        assert torch.equal(raw[mine], seg[mine])
        seen["rendered"] += int(rendered.sum())
        seen["empty"] += int((~rendered).sum())
        seen["endmember closest"] += int(mine.sum())
    print(seen)
    assert seen["rendered"] > 100 and seen["empty"] > 100


def test_the_other_outputs_are_classify_of_the_ops_own_output(world):
    lib = world["library"]
    got = _frame(world, lib)
    index, cos = lib.match(got["spectral"])
    want = lib.classify(index, cos, got["accumulation"])
    for k in NAMES:
        assert torch.equal(got[k].reshape(-1, got[k].shape[-1]), want[k]), k
    rendered = got["library_raw"][..., 0] >= 0
    assert torch.equal(got["library_pred"][rendered], torch.from_numpy(lib.colors).to(DEV)[got["library_raw"][..., 0][rendered].long()])
    assert bool((got["library_pred"][~rendered] == 0).all()) and bool((got["library_margin"][rendered] >= 0).all())
    # max_angle: a pixel is unmatched where angle > max_angle.  At 0 that is every pixel but those whose float32 cosine is exactly 1
    # (this scene's spectra lie within the 1e-3 rad a float32 cosine does not resolve of an endmember: such pixels exist)
    angle, raw = got["library_angle"], got["library_raw"]
    for limit in (0.0, float(angle[rendered].median()), -1.0):
        cut = _frame(world, lib, max_angle=limit)
        assert torch.equal(cut["library_raw"], torch.where(angle > limit, torch.full_like(raw, -1.0), raw)), limit
        assert bool((cut["library_pred"][cut["library_raw"][..., 0] < 0] == 0).all()) and torch.equal(cut["library_angle"], angle)
        print(f"max_angle {limit:g}: {int((cut['library_raw'] >= 0).sum())} of {int(rendered.sum())} matched")
    assert bool((cut["library_raw"] == -1).all())  # (below every angle: nothing is matched)


def test_under_material_edits_the_edited_spectrum_is_matched(world):
    from umhsnerf.materials import load_material_edits

    model, lib = world["pipe"].model, world["library"]
    edits = load_material_edits({"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}]}, 3, 8, False)
    rb = world["cameras"].generate_rays(1, keep_shape=True)
    with model.material_edits_context(edits), model.spectral_library_context(lib):
        got = model.get_outputs_for_camera_ray_bundle(rb)
    plain = _frame(world, lib)
    assert not torch.equal(got["spectral"], plain["spectral"])
    want = lib.frame_outputs(got["spectral"], got["accumulation"])
    for k in NAMES:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["library_angle"], plain["library_angle"])


def test_refusals_and_the_state_after_an_exception(world):
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model, lib = world["pipe"].model, world["library"]
    rgb = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": world["wl"], "num_classes": 3}, seed=1)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with rgb.spectral_library_context(lib):
            pass
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="model.eval"):
            with model.spectral_library_context(lib):
                model.get_outputs_for_camera_ray_bundle(rb)
    finally:
        model.eval()
    assert model._spectral_library is None
    with pytest.raises(KeyError):
        with model.spectral_library_context(lib, 0.3):
            assert model._spectral_library == (lib, 0.3)
            raise KeyError("inside")
    assert model._spectral_library is None
    from umhsnerf.library import SpectralLibrary

    with pytest.raises(ValueError, match="wavelengths"):
        with model.spectral_library_context(SpectralLibrary(["a"], np.ones((1, 5)), [1.0, 2.0, 3.0, 4.0, 5.0])):
            pass


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _model_flags(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *BASE_FLAGS]


def test_render_camera_path_with_a_library(world, capsys):
    from PIL import Image

    from umhsnerf import render

    root = world["root"]
    got = render.main(["camera-path", *_model_flags(world), "--camera-path-filename", str(root / "path.json"), "--output-path", str(root / "cli"),
                       "--spectral-library", str(root / "library.npz"), "--rendered-output-names", "rgb", "library_pred", "library_angle"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got["frames"] == 3 and got["panels"] == 3 and got["spectral_library"] == str(root / "library.npz")
    frame = np.asarray(Image.open(root / "cli" / "frame_00001.png"))
    assert frame.shape == (H, 3 * W, 3)
    want = _frame(world, world["library"], camera=1)["library_pred"]
    assert np.array_equal(frame[:, W:2 * W], (want * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu().numpy())
    assert world["pipe"].model._spectral_library is None


def test_eval_and_identify_with_a_library(world, capsys):
    from umhsnerf import eval as umhs_eval
    from umhsnerf import library

    root = world["root"]
    got = umhs_eval.main([*_model_flags(world), "--spectral-library", str(root / "library.npz")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "psnr" in got
    top = got["library_top"]
    assert 1 <= len(top) <= 16 and all(set(t) == {"name", "share", "mean_angle"} for t in top)
    assert all(a["share"] >= b["share"] for a, b in zip(top, top[1:])) and 0 < sum(t["share"] for t in top) <= 1
    assert all(0 <= t["mean_angle"] <= np.pi for t in top)
    assert 0.0 <= got["library_agreement"] <= 1.0
    matches = got["endmember_matches"]
    assert len(matches) == 3 and all(len(m) == 3 for m in matches)
    for c, m in enumerate(matches):
        assert m[0]["name"] == f"endmember_{c}" and m[0]["index"] == c and m[0]["angle"] < 1e-3
        assert m[0]["angle"] <= m[1]["angle"] <= m[2]["angle"] and len({e["index"] for e in m}) == 3
    ident = library.main(["identify", *_model_flags(world), "--spectral-library", str(root / "library.npz")])
    out = capsys.readouterr().out
    assert ident["endmember_matches"] == matches and "endmember 0: endmember_0" in out
    five = library.main(["identify", *_model_flags(world), "--spectral-library", str(root / "library.npz"), "--top", "5"])
    capsys.readouterr()
    assert all(len(m) == 5 and m[:3] == w for m, w in zip(five["endmember_matches"], matches))
