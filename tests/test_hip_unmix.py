"""Spectral unmixing on the GPU: csrc/umhs_unmix.hip per row against the float64 oracle (tests/unmix_f64.py), the outputs of
``UMHSModel.unmixing_context`` on the small trained pipeline of tests/test_hip_library.py (``make_scene(B=8)``, 3 classes, 20 x 28 path
frames), and ``--unmix`` on the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import rays_f64 as RF
import unmix_f64 as UF
from test_hip_library import BASE_FLAGS, CROP, H, W, world  # noqa: F401  (the fixture: the module's own copy of the small pipeline)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}


def _report(key, report):
    _WORST[key] = report
    with open(os.path.join(RF.report_dir(ROOT), "unmix_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)


def _device_rows(case):
    """The case's rows on the device in the case's own layout (a slice case: a column slice of the wider array, read in place)."""
    wide = torch.from_numpy(case["wide"]).to(DEV)
    return wide[:, UF.SLICE_AT:UF.SLICE_AT + case["B"]] if case["layout"] == "slice" else wide


def _unmix(case, rows, mode):
    from umhsnerf import ops

    image = ops.library_prepare(torch.from_numpy(case["E"]).to(DEV))
    return ops.unmix(rows, image, torch.from_numpy(case["G"]).to(DEV), case["K"], mode, want_residual=True, want_status=True)


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernel
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("mode", UF.MODES, ids=["nnls", "fcls"])
@pytest.mark.parametrize("c", UF.CASES, ids=UF.unmix_id)
def test_unmix_is_within_the_bounds_of_float64_and_repeats_bit_for_bit(c, mode):
    case, ref = UF.reference(*c, mode)
    rows = _device_rows(case)
    if case["layout"] == "slice":
        assert rows.stride(0) == case["B"] + UF.SLICE_PAD and rows.data_ptr() % 16 != 0
    a, res, status = _unmix(case, rows, mode)
    assert tuple(a.shape) == (case["R"], case["K"]) and tuple(res.shape) == tuple(status.shape) == (case["R"],)
    assert a.dtype == res.dtype == torch.float32 and status.dtype == torch.int32
    report = {}
    fails = UF.check(case, a.cpu().numpy(), res.cpu().numpy(), status.cpu().numpy(), report)
    print(UF.unmix_id(c), "fcls" if mode else "nnls", {k: round(v, 4) for k, v in report.items()})
    _report(f"{UF.unmix_id(c)} {'fcls' if mode else 'nnls'}", report)
    assert not fails, fails
    assert all(v < 1.0 for k, v in report.items() if k != "cap_share")
    again = _unmix(case, rows, mode)
    for x, y in zip((a, res, status), again):  # the same bits on a second run
        assert torch.equal(_bits(x), _bits(y))
    if case["layout"] == "slice":  # a view gives the bits of its contiguous copy
        for x, y in zip((a, res, status), _unmix(case, rows.contiguous(), mode)):
            assert torch.equal(_bits(x), _bits(y))
    if case["R"] == 0:
        return
    # without the optional outputs: the same abundances
    from umhsnerf import ops

    image = ops.library_prepare(torch.from_numpy(case["E"]).to(DEV))
    only, none_r, none_s = ops.unmix(rows, image, torch.from_numpy(case["G"]).to(DEV), case["K"], mode, want_residual=False)
    assert none_r is None and none_s is None and torch.equal(_bits(only), _bits(a))


@pytest.mark.parametrize("mode", UF.MODES, ids=["nnls", "fcls"])
def test_a_row_alone_gives_its_bits_in_the_batch(mode):
    for c in (UF.CASES[6], UF.CASES[8], UF.CASES[13]):  # K16-B90 (T = 2), the hotdog slice, K16-B256 (T = 1)
        case, _ = UF.reference(*c, mode)
        rows = _device_rows(case)
        a, res, status = _unmix(case, rows, mode)
        for r in (0, 31, 32, 63, 64, 65, 95, 96, case["R"] - 1):
            one = _unmix(case, rows[r:r + 1], mode)
            for x, y in zip((a, res, status), one):
                assert torch.equal(_bits(x[r:r + 1]), _bits(y)), (UF.unmix_id(c), r)
        # and a batch that starts elsewhere: the bits do not depend on the row's place in its workgroup
        shifted = _unmix(case, rows[7:], mode)
        for x, y in zip((a, res, status), shifted):
            assert torch.equal(_bits(x[7:]), _bits(y))


def test_no_rows_and_the_ops_refusals():
    from umhsnerf import ops

    case, _ = UF.reference(*UF.CASES[4], UF.FCLS)  # R = 0
    a, res, status = _unmix(case, _device_rows(case), UF.FCLS)
    assert tuple(a.shape) == (0, 6) and tuple(res.shape) == (0,) and tuple(status.shape) == (0,)
    E = torch.from_numpy(UF.endmembers("syn", 6, 31)).to(DEV)
    image, G = ops.library_prepare(E), torch.from_numpy(UF.gram32(E.cpu().numpy())).to(DEV)
    x = torch.rand(5, 31, device=DEV)
    with pytest.raises(ValueError, match="mode"):
        ops.unmix(x, image, G, 6, 2)
    with pytest.raises(ValueError, match="gram"):
        ops.unmix(x, image, G[:5], 6, 1)
    with pytest.raises(ValueError, match="image"):
        ops.unmix(torch.rand(5, 33, device=DEV), image, G, 6, 1)
    with pytest.raises(ValueError, match="limits"):
        ops.unmix(torch.rand(5, 300, device=DEV), image, G, 6, 1)


def test_properties_of_the_solution():
    """What holds by construction: an exact endmember unmixes to its indicator; FCLS of a mix inside the simplex takes one solve; a
    scaled mix tells the modes apart; the abundances are never negative zero."""
    from umhsnerf import ops

    E = UF.endmembers("hotdog", 4, 141)
    image, G = ops.library_prepare(torch.from_numpy(E).to(DEV)), torch.from_numpy(UF.gram32(E)).to(DEV)
    inside = np.array([[0.4, 0.3, 0.2, 0.1], [0.25, 0.25, 0.25, 0.25]])
    x = torch.from_numpy(np.concatenate([E.astype(np.float64), inside @ E, 0.5 * (inside @ E)]).astype(np.float32)).to(DEV)
    for mode in UF.MODES:
        a, res, status = ops.unmix(x, image, G, 4, mode, want_status=True)
        a = a.cpu().numpy()
        assert np.abs(a[:4] - np.eye(4)).max() < 1e-4 and np.abs(a[4:6] - inside).max() < 1e-4
        assert not np.signbit(a).any() and (status.cpu().numpy()[4:6] == 1).all()
        if mode == UF.NNLS:
            assert np.abs(a[6:] - 0.5 * inside).max() < 1e-4
        else:
            assert np.abs(a[6:].sum(1) - 1).max() < 1e-5 and np.abs(a[6:] - 0.5 * inside).max() > 0.05
        ss = (x.double() ** 2).sum(1)
        assert bool((res[:6].double() <= UF.K_R * UF.U * ss[:6]).all())  # an exact fit, up to the residual's own rounding


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
def _frame(world, unmixer=None, camera=1, output_names=None, crop=False):
    from umhsnerf.render import parse_crop

    model = world["pipe"].model
    if crop:
        rb = world["cameras"].generate_rays(camera, keep_shape=True, obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane)
    else:
        rb = world["cameras"].generate_rays(camera, keep_shape=True)
    with model.unmixing_context(unmixer):
        return model.get_outputs_for_camera_ray_bundle(rb, output_names=output_names)


def _names(K=3):
    from umhsnerf.unmix import unmix_outputs

    return unmix_outputs(K)


@pytest.mark.parametrize("constraint", ["fcls", "nnls"])
def test_the_context_outputs_are_ops_unmix_of_the_frames_spectral(world, constraint):
    from umhsnerf import ops
    from umhsnerf.unmix import Unmixer

    model = world["pipe"].model
    u = Unmixer.from_model(model, constraint)
    assert np.array_equal(u.endmembers, model.field.endmembers.detach().clamp(0, 1).cpu().numpy()) and u.names == [f"endmember_{k}" for k in range(3)]
    seen = {"rendered": 0, "empty": 0}
    for camera, crop in [(c, k) for c in range(3) for k in (False, True)]:  # (through a crop box: rays that accumulate <= 0.5)
        plain = _frame(world, camera=camera, crop=crop)
        assert not any(k in plain for k in _names())
        got = _frame(world, u, camera=camera, crop=crop)
        assert [k for k in got if k not in _names()] == list(plain) and all(k in got for k in _names())
        for k in plain:
            assert torch.equal(got[k], plain[k]), k
        image, gram, colors = u.on(DEV)
        a, res, status = ops.unmix(got["spectral"], image, gram, 3, u.mode, want_status=True)
        rendered = (got["accumulation"].reshape(-1) > 0.5) & (status != -1)
        a = torch.where(rendered[:, None], a, torch.zeros_like(a))
        assert torch.equal(got["unmix"].reshape(-1, 3), a) and tuple(got["unmix"].shape) == (H, W, 3)
        assert torch.equal(got["unmix"], torch.cat([got[f"unmix_{k}"] for k in range(3)], -1))  # the cube is the stacked panels
        raw = got["unmix_raw"].reshape(-1)
        assert torch.equal(raw == -1, ~rendered) and torch.equal(raw[rendered].long(), a[rendered].argmax(1))
        assert torch.equal(got["unmix_pred"].reshape(-1, 3)[rendered], colors[raw[rendered].long()])
        assert bool((got["unmix_pred"].reshape(-1, 3)[~rendered] == 0).all()) and bool((got["unmix"].reshape(-1, 3)[~rendered] == 0).all())
        want = torch.where(rendered, torch.sqrt(res / 8.0), torch.zeros_like(res))
        assert torch.equal(got["unmix_residual"].reshape(-1), want)
        if constraint == "fcls" and bool(rendered.any()):
            assert float((a[rendered].sum(1) - 1).abs().max()) < 1e-5
        seen["rendered"] += int(rendered.sum())
        seen["empty"] += int((~rendered).sum())
    assert seen["rendered"] > 100 and seen["empty"] > 100
    # computed only when asked for
    assert sorted(_frame(world, u, output_names=["rgb", "depth"])) == ["depth", "rgb"]
    some = _frame(world, u, output_names=["unmix_pred", "unmix_1"])
    full = _frame(world, u)
    assert sorted(some) == ["unmix_1", "unmix_pred"] and torch.equal(some["unmix_1"], full["unmix_1"])
    assert model._unmixer is None


def test_the_float64_oracle_agrees_on_a_frame(world):
    from umhsnerf.unmix import Unmixer

    u = Unmixer.from_model(world["pipe"].model)
    got = _frame(world, u)
    x = got["spectral"].reshape(-1, 8).cpu().numpy()
    star, _, _ = UF.solve_f64(u.endmembers, x, UF.FCLS)
    bound = UF.K_A * UF.U * u.conditioning["cond"] * np.maximum(1.0, np.abs(star).max(1))
    assert (np.abs(got["unmix"].reshape(-1, 3).cpu().numpy() - star).max(1) <= bound).all()


def test_under_material_edits_the_edited_spectrum_is_unmixed(world):
    from umhsnerf.materials import load_material_edits
    from umhsnerf.unmix import Unmixer

    model = world["pipe"].model
    u = Unmixer.from_model(model)
    edits = load_material_edits({"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}]}, 3, 8, False)
    rb = world["cameras"].generate_rays(1, keep_shape=True)
    with model.material_edits_context(edits), model.unmixing_context(u):
        got = model.get_outputs_for_camera_ray_bundle(rb)
    plain = _frame(world, u)
    assert not torch.equal(got["spectral"], plain["spectral"])
    want = u.frame_outputs(got["spectral"], got["accumulation"])
    for k in _names():
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["unmix"], plain["unmix"])


def test_a_library_of_the_models_own_endmembers_gives_the_models_outputs(world):
    from umhsnerf.library import SpectralLibrary
    from umhsnerf.unmix import Unmixer

    model = world["pipe"].model
    E = model.field.endmembers.detach().clamp(0, 1).cpu().double().numpy()
    names = [f"endmember_{k}" for k in range(3)]
    lib = SpectralLibrary(["other", *names], np.concatenate([np.full((1, 8), 0.5), E]), world["wl"])
    ours, theirs = Unmixer.from_model(model), Unmixer.from_library(lib, names)
    assert np.array_equal(ours.endmembers, theirs.endmembers) and np.array_equal(ours.gram, theirs.gram)
    a, b = _frame(world, ours), _frame(world, theirs)
    for k in _names():
        if k != "unmix_pred":  # (the colours are the library's own)
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(b["unmix_pred"].reshape(-1, 3)[b["unmix_raw"].reshape(-1) >= 0],
                       torch.from_numpy(lib.colors).to(DEV)[1 + b["unmix_raw"].reshape(-1)[b["unmix_raw"].reshape(-1) >= 0].long()])


def test_refusals_and_the_state_after_an_exception(world):
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel
    from umhsnerf.unmix import Unmixer

    model = world["pipe"].model
    u = Unmixer.from_model(model)
    rgb = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": world["wl"], "num_classes": 3}, seed=1)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with rgb.unmixing_context(u):
            pass
    with pytest.raises(NotImplementedError, match="spectral method"):
        Unmixer.from_model(rgb)
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="model.eval"):
            with model.unmixing_context(u):
                model.get_outputs_for_camera_ray_bundle(rb)
    finally:
        model.eval()
    assert model._unmixer is None
    with pytest.raises(KeyError):
        with model.unmixing_context(u):
            assert model._unmixer is u
            raise KeyError("inside")
    assert model._unmixer is None
    with pytest.raises(ValueError, match="wavelengths"):
        with model.unmixing_context(Unmixer(UF.synthetic_endmembers(3, 5))):
            pass
    with pytest.raises(ValueError, match="3 endmembers"):
        _frame(world, u, output_names=["unmix_3"])
    with pytest.raises(ValueError, match="bands"):
        u.frame_outputs(torch.rand(4, 5, device=DEV), None)


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _model_flags(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *BASE_FLAGS]


def test_render_camera_path_with_unmixing(world, capsys):
    from PIL import Image

    from umhsnerf import render
    from umhsnerf.unmix import Unmixer

    root = world["root"]
    got = render.main(["camera-path", *_model_flags(world), "--camera-path-filename", str(root / "path.json"), "--output-path",
                       str(root / "cli_unmix"), "--unmix", "model", "--rendered-output-names", "rgb", "unmix_pred", "unmix_0",
                       "--cube-output-names", "unmix"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got["frames"] == 3 and got["panels"] == 3
    assert got["unmix"] == {"source": "model", "constraint": "fcls", "endmembers": [f"endmember_{k}" for k in range(3)]}
    frame = np.asarray(Image.open(root / "cli_unmix" / "frame_00001.png"))
    assert frame.shape == (H, 3 * W, 3)
    want = _frame(world, Unmixer.from_model(world["pipe"].model), camera=1)
    assert np.array_equal(frame[:, W:2 * W], (want["unmix_pred"] * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu().numpy())
    cubes = sorted(p for p in os.listdir(root / "cli_unmix") if p.endswith(".npy"))
    assert len(cubes) == 3
    assert np.array_equal(np.load(root / "cli_unmix" / cubes[1]), want["unmix"].cpu().numpy())
    assert world["pipe"].model._unmixer is None


def test_eval_with_unmixing_emits_the_keys_and_the_rmse_is_numpys(world, capsys):
    from umhsnerf import eval as umhs_eval
    from umhsnerf.unmix import Unmixer

    got = umhs_eval.main([*_model_flags(world), "--unmix", "model"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "psnr" in got
    keys = ("unmix_abundance_rmse", "unmix_abundance_rmse_per_material", "unmix_agreement", "unmix_residual_captured",
            "unmix_residual_rendered", "unmix_cap_share")
    assert all(k in got for k in keys)
    # the same numbers in numpy, from the same tensors
    pipe = world["pipe"]
    u = Unmixer.from_model(pipe.model)
    sq, n, agree, cap_r, ren_r, capped = np.zeros(3), 0, 0, 0.0, 0.0, 0
    for rb, batch in pipe.datamanager.eval_images():
        with pipe.model.unmixing_context(u):
            out = pipe.model.get_outputs_for_camera_ray_bundle(rb)
        counted = (out["accumulation"].reshape(-1) > 0.5).cpu().numpy()
        a, res, status = u.unmix(batch["hs_image"].to(DEV).float().reshape(-1, 8), True, True)
        a, res, status = a.double().cpu().numpy(), res.double().cpu().numpy(), status.cpu().numpy()
        ab = out["abundances"].reshape(-1, 3).double().cpu().numpy()
        sq += ((ab - a) ** 2)[counted].sum(0)
        n += int(counted.sum())
        agree += int((ab.argmax(1) == a.argmax(1))[counted].sum())
        cap_r += np.sqrt(res / 8)[counted].sum()
        ren_r += out["unmix_residual"].reshape(-1).double().cpu().numpy()[counted].sum()
        capped += int((status == -2)[counted].sum())
    assert n > 0
    assert got["unmix_abundance_rmse"] == pytest.approx(np.sqrt(sq.sum() / (3 * n)), rel=1e-9)
    assert got["unmix_abundance_rmse_per_material"] == pytest.approx(list(np.sqrt(sq / n)), rel=1e-9)
    assert got["unmix_agreement"] == pytest.approx(agree / n) and 0.0 <= got["unmix_agreement"] <= 1.0
    assert got["unmix_residual_captured"] == pytest.approx(cap_r / n, rel=1e-9)
    assert got["unmix_residual_rendered"] == pytest.approx(ren_r / n, rel=1e-9)
    assert got["unmix_cap_share"] == capped / n
    assert pipe.model._unmixer is None


def test_the_captured_command_writes_ops_unmix_of_the_frames(world, capsys):
    from umhsnerf import unmix
    from umhsnerf.unmix import Unmixer

    root, pipe = world["root"], world["pipe"]
    got = unmix.main(["captured", *_model_flags(world), "--split", "train", "--output-path", str(root / "captured")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got == json.loads((root / "captured" / "summary.json").read_text())
    stack = pipe.datamanager.train_split.hs_image
    assert len(got["frames"]) == stack.shape[0] > 0 and got["endmembers"] == [f"endmember_{k}" for k in range(3)]
    u = Unmixer.from_model(pipe.model)
    for i, frame in enumerate(got["frames"]):
        cube = np.load(root / "captured" / f"{frame['frame']}_unmix.npy")
        a, res, status = u.unmix(stack[i].to(DEV).float(), True, True)
        assert cube.shape == (*stack.shape[1:3], 3) and np.array_equal(cube.reshape(-1, 3), a.cpu().numpy())
        valid = (status != -1).cpu().numpy()
        assert frame["mean_abundance"] == pytest.approx(list(a.double().cpu().numpy()[valid].mean(0)), rel=1e-9)
        assert frame["mean_residual"] == pytest.approx(float(np.sqrt(res.double().cpu().numpy() / 8)[valid].mean()), rel=1e-9)
        assert frame["invalid"] == int((~valid).sum())
