"""Continuum removal on the GPU: csrc/umhs_continuum.hip against the float64 oracle and the derived bounds of tests/continuum_f64.py,
its bit-for-bit guarantees, the model context, the library matched on shapes, and the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import continuum_f64 as CF
import rays_f64 as RF
from test_hip_library import BASE_FLAGS, CROP, H, W, world  # noqa: F401  (the fixture: the module's own copy of the small pipeline)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}


def _report(key, report):
    _WORST[key] = report
    with open(os.path.join(RF.report_dir(ROOT), "continuum_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)


def _device_rows(case):
    """The case's rows on the device in the case's own layout (a slice case: a column slice of the wider array, read in place)."""
    wide = torch.from_numpy(case["wide"]).to(DEV)
    return wide[:, CF.SLICE_AT:CF.SLICE_AT + case["B"]] if case["layout"] == "slice" else wide


def _run(case, rows, want_removed=True, want_status=True, ranges=None):
    from umhsnerf import ops

    return ops.continuum(rows, torch.from_numpy(case["lam"]).to(DEV), case["ranges"] if ranges is None else ranges, want_removed, want_status)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _np(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernel
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("c", CF.CASES, ids=CF.case_id)
def test_continuum_is_within_the_bounds_of_float64_and_repeats_bit_for_bit(c):
    case, ref = CF.reference(*c)
    B, R, F = case["B"], case["R"], len(case["ranges"])
    rows = _device_rows(case)
    if case["layout"] == "slice" and R > 1:
        assert rows.stride(0) == B + CF.SLICE_PAD and rows.data_ptr() % 16 != 0
    removed, features, status = _run(case, rows)
    assert tuple(removed.shape) == (R, B) and tuple(status.shape) == (R,) and removed.dtype == torch.float32 and status.dtype == torch.int32
    assert (features is None) if F == 0 else (tuple(features.shape) == (R, F, 3) and features.dtype == torch.float32)
    report = {}
    fails = CF.check(case, _np(removed), _np(features), _np(status), report)
    print(CF.case_id(c), {k: float(f"{v:.3g}") for k, v in report.items()})
    _report(CF.case_id(c), report)
    assert not fails, fails
    assert all(v < 1.0 for v in report.values())
    for x, y in zip((removed, features, status), _run(case, rows)):  # the same bits on a second run
        assert _same(x, y)
    if case["layout"] == "slice":  # a view gives the bits of its contiguous copy
        for x, y in zip((removed, features, status), _run(case, rows.contiguous())):
            assert _same(x, y)
    if R == 0:
        return
    # optional outputs absent: the same bits for the rest (no removed and no status: the full-range hull is skipped)
    for want_removed, want_status in ((False, False), (False, True), (True, False)):
        r2, f2, s2 = _run(case, rows, want_removed, want_status)
        assert (r2 is None) == (not want_removed) and (s2 is None) == (not want_status)
        assert _same(f2, features) and (r2 is None or _same(r2, removed)) and (s2 is None or _same(s2, status))
    if F:
        r2, f2, s2 = _run(case, rows, ranges=[])  # and without the features
        assert f2 is None and _same(r2, removed) and _same(s2, status)
        # feature 0 is the full range: its minimum of r and its area are what `removed` gives, bit for bit
        assert case["ranges"][0] == (0, B - 1)
        v = torch.from_numpy(case["valid"]).to(DEV)
        depth = (1.0 - removed.min(1).values)[v]
        assert _same(features[:, 0, 0][v], depth)
        area = CF.area_from_removed(case["lam"], _np(removed), 0, B - 1)
        assert np.array_equal(_np(features[:, 0, 2])[case["valid"]].view(np.int32), area[case["valid"]].view(np.int32))
        first = np.argmin(_np(removed), 1)  # (numpy's argmin: the first band at the minimum)
        assert np.array_equal(_np(features[:, 0, 1])[case["valid"]], case["lam"][first][case["valid"]])


def test_a_row_alone_or_shifted_gives_its_bits_in_the_batch():
    for c in ((31, 300, "rows", "uni", 8), (141, 130, "slice", "uni", 1), (256, 130, "slice", "non", 8), (253, 65, "rows", "non", 8)):
        case, _ = CF.reference(*c)
        rows = _device_rows(case)
        whole = _run(case, rows)
        for r in (0, 31, 32, 63, 64, 65, case["R"] - 1):
            for x, y in zip(whole, _run(case, rows[r:r + 1])):
                assert _same(x[r:r + 1], y), (CF.case_id(c), r)
        for x, y in zip(whole, _run(case, rows[7:])):  # a batch that starts elsewhere: another lane, another tile
            assert _same(x[7:], y), CF.case_id(c)


def test_the_exact_rows_give_the_oracles_vertices_and_centres():
    seen = 0
    for c in [c for c in CF.CASES if c[3] == "int"]:
        case, ref = CF.reference(*c)
        removed, features, status = _run(case, _device_rows(case))
        v = case["valid"]
        assert np.array_equal(_np(status)[v], ref["status"][v]), CF.case_id(c)
        for k, (lo, hi) in enumerate(case["ranges"]):
            xw = case["x"][:, lo:hi + 1]
            sure = v & (xw[:, 1:-1] == 0).any(1) & (xw >= 0).all(1) & (xw > 0).any(1)
            want = case["lam"][ref["per_feature"][k]["m"]]
            assert np.array_equal(_np(features[:, k, 1])[sure], want[sure]), (CF.case_id(c), k)
            assert (_np(features[:, k, 0])[sure] == 1.0).all()  # r = 0 there, exactly
            seen += int(sure.sum())
    assert seen > 50


def test_no_rows_and_the_ops_refusals():
    from umhsnerf import ops

    case, _ = CF.reference(31, 0, "rows", "uni", 8)
    removed, features, status = _run(case, _device_rows(case))
    assert tuple(removed.shape) == (0, 31) and tuple(features.shape) == (0, 8, 3) and tuple(status.shape) == (0,)
    lam, x = torch.arange(31.0, device=DEV), torch.rand(5, 31, device=DEV)
    assert ops.continuum(x, lam, (), want_removed=False, want_status=False) == (None, None, None)
    with pytest.raises(ValueError, match="limits"):
        ops.continuum(torch.rand(5, 300, device=DEV), torch.arange(300.0, device=DEV))
    with pytest.raises(ValueError, match="limits"):
        ops.continuum(x, lam, [(0, 30)] * 9)
    with pytest.raises(ValueError, match=r"feature 1.*\[4, 31\] is outside"):
        ops.continuum(x, lam, [(0, 30), (4, 31)])
    with pytest.raises(ValueError, match="outside"):
        ops.continuum(x, lam, [(6, 5)])
    with pytest.raises(ValueError, match=r"feature 0.*fewer than 3"):
        ops.continuum(x, lam, [(4, 5)])
    with pytest.raises(ValueError, match="wavelengths"):
        ops.continuum(x, lam[:30])
    with pytest.raises(ValueError, match="wavelengths"):
        ops.continuum(x, lam.double())
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.continuum(x, lam.cpu())


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
def _analysis(world, features=True):
    from umhsnerf.continuum import ContinuumAnalysis

    wl = world["wl"]
    return ContinuumAnalysis(wl, [("low", (wl[0], wl[3])), ("mid", (wl[2], wl[6])), ("all", (wl[0], wl[7]))] if features else ())


def _frame(world, analysis=None, camera=1, output_names=None, crop=False):
    from umhsnerf.render import parse_crop

    model = world["pipe"].model
    if crop:  # (the untrained scene is opaque everywhere: a crop box leaves rays that accumulate nothing)
        rb = world["cameras"].generate_rays(camera, keep_shape=True, obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane)
    else:
        rb = world["cameras"].generate_rays(camera, keep_shape=True)
    with model.continuum_context(analysis):
        return model.get_outputs_for_camera_ray_bundle(rb, output_names=output_names)


def _frame_case(analysis, spectral):
    """The rows of a frame as a case of the comparator, and their float64 run."""
    x = np.ascontiguousarray(spectral.reshape(-1, analysis.bands).cpu().numpy())
    case = dict(B=analysis.bands, R=x.shape[0], layout="rows", lam_kind="scene", F=len(analysis), lam=analysis.wavelengths, x=x, wide=x,
                ranges=list(analysis.ranges), valid=CF.row_valid(x), exact=False)
    return case, CF.run(case["lam"], x, case["ranges"], np.float64)


def test_the_context_outputs_are_the_oracle_on_the_frames_own_spectral(world):
    from umhsnerf.continuum import continuum_outputs

    a = _analysis(world)
    names = continuum_outputs(8, 3)
    seen = {"rendered": 0, "empty": 0}
    for camera, crop in ((0, False), (1, True), (2, True)):
        plain = _frame(world, camera=camera, crop=crop)
        assert not any(k in plain for k in names)
        got = _frame(world, a, camera=camera, crop=crop)
        assert [k for k in got if k not in names] == list(plain) and all(k in got for k in names)
        for k in plain:  # every other output: the same bits
            assert torch.equal(got[k], plain[k]), k
        assert tuple(got["cr"].shape) == (H, W, 8) and tuple(got["feature_depth"].shape) == (H, W, 3)
        assert all(tuple(got[k].shape) == (H, W, 1) for k in names if k not in ("cr", "feature_depth"))
        rendered = (plain["accumulation"].reshape(-1) > 0.5).cpu().numpy()
        cr = got["cr"].reshape(-1, 8).cpu().numpy()
        feats = np.stack([np.concatenate([got[f"feature_{w}_{f}"].reshape(-1, 1).cpu().numpy() for w in ("depth", "center", "area")], 1)
                          for f in range(3)], 1)
        assert (cr[~rendered] == 0).all() and (feats[~rendered] == 0).all()
        assert np.array_equal(got["feature_depth"].reshape(-1, 3).cpu().numpy(), feats[:, :, 0])
        for b in range(8):
            assert np.array_equal(got[f"cr_{b}"].reshape(-1).cpu().numpy(), cr[:, b])
        case, ref = _frame_case(a, plain["spectral"].reshape(-1, 8)[torch.from_numpy(rendered).to(DEV)])
        report = {}
        fails = CF.check(case, cr[rendered], feats[rendered], None, report, ref=ref)
        assert not fails, (camera, crop, fails, report)
        _report(f"frame-camera{camera}{'-crop' if crop else ''}", report)
        seen["rendered"] += int(rendered.sum())
        seen["empty"] += int((~rendered).sum())
    print(seen)
    assert seen["rendered"] > 100 and seen["empty"] > 100
    # computed only when asked for, and only what is asked for
    full = _frame(world, a)
    assert sorted(_frame(world, a, output_names=["rgb", "depth"])) == ["depth", "rgb"]
    some = _frame(world, a, output_names=["feature_center_1", "cr_3", "rgb"])
    assert sorted(some) == ["cr_3", "feature_center_1", "rgb"]
    assert all(torch.equal(some[k], full[k]) and some[k].is_contiguous() for k in some)
    only = _frame(world, a, output_names=["feature_depth", "feature_area_2"])
    assert sorted(only) == ["feature_area_2", "feature_depth"] and torch.equal(only["feature_depth"], full["feature_depth"])
    # a render without output_names builds the names the context was given, and those only (what eval does for its tally)
    model, rb = world["pipe"].model, world["cameras"].generate_rays(1, keep_shape=True)
    plain = _frame(world)
    with model.continuum_context(a, ["feature_depth", "feature_center_1"]):
        named = model.get_outputs_for_camera_ray_bundle(rb)
    assert [k for k in named if k not in plain] == ["feature_depth", "feature_center_1"] and [k for k in named if k in plain] == list(plain)
    assert all(torch.equal(named[k], full[k]) for k in named)
    with pytest.raises(ValueError, match="feature_center_3: the context has 8 bands and 3 features"):
        with model.continuum_context(a, ["feature_center_3"]):
            model.get_outputs_for_camera_ray_bundle(rb)
    assert a.frame_outputs(plain["spectral"], plain["accumulation"], ["rgb", "depth"]) == {}  # nothing named: nothing launched
    bare = _frame(world, _analysis(world, features=False), output_names=["cr"])  # no features: a context for cr alone
    assert list(bare) == ["cr"] and torch.equal(bare["cr"], full["cr"])
    assert world["pipe"].model._continuum is None


def test_refusals_and_the_state_after_an_exception(world):
    from umhsnerf.continuum import ContinuumAnalysis
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model, a = world["pipe"].model, _analysis(world)
    rgb = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": world["wl"], "num_classes": 3}, seed=1)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with rgb.continuum_context(a):
            pass
    with pytest.raises(ValueError, match="7 wavelengths; the model has 8"):
        with model.continuum_context(ContinuumAnalysis(world["wl"][:7])):
            pass
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="model.eval"):
            with model.continuum_context(a):
                model.get_outputs_for_camera_ray_bundle(rb)
    finally:
        model.eval()
    assert model._continuum is None
    for name in ("cr_8", "feature_depth_3", "feature_area_3", "feature_center_7"):
        with pytest.raises(ValueError, match=f"{name}: the context has 8 bands and 3 features"):
            _frame(world, a, output_names=[name])
    with pytest.raises(ValueError, match="feature_depth"):
        _frame(world, _analysis(world, features=False), output_names=["feature_depth"])
    assert model._continuum is None


def test_a_library_is_matched_on_shapes_and_is_what_it_was_without_the_flag(world):
    from umhsnerf.continuum import ContinuumAnalysis

    model, lib = world["pipe"].model, world["library"]
    removed_lib = lib.continuum_removed()
    lam32 = ContinuumAnalysis(world["wl"]).wavelengths
    seen = {"rendered": 0, "sure": 0, "moved": 0}
    for camera, crop in ((0, False), (1, True)):
        from umhsnerf.render import parse_crop

        kw = dict(obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane) if crop else {}
        rb = world["cameras"].generate_rays(camera, keep_shape=True, **kw)
        plain = model.get_outputs_for_camera_ray_bundle(rb)
        with model.spectral_library_context(lib):
            before = model.get_outputs_for_camera_ray_bundle(rb)
        with model.spectral_library_context(lib, None, False):
            same = model.get_outputs_for_camera_ray_bundle(rb)
        with model.spectral_library_context(lib, continuum_removed=True):
            got = model.get_outputs_for_camera_ray_bundle(rb)
        for k in before:  # without the flag: what it was, bit for bit; with it: only the library outputs differ
            assert torch.equal(before[k], same[k]), k
        for k in plain:
            assert torch.equal(got[k], plain[k]), k
        spec = plain["spectral"].reshape(-1, 8).cpu().numpy()
        rendered = (plain["accumulation"].reshape(-1) > 0.5).cpu()
        r64 = CF.run(lam32, spec, [], np.float64)["removed"]
        cos = RF.cluster_ties(torch.from_numpy(r64), torch.from_numpy(removed_lib.spectra))[0]
        angle = torch.acos(cos.clamp(-1, 1))
        two = angle.topk(2, dim=1, largest=False).values
        sure = rendered & ((two[:, 1] - two[:, 0]) > 1e-3)  # (the matcher resolves no angle below about 1e-3 rad)
        raw = got["library_raw"].reshape(-1).long().cpu()
        assert torch.equal(raw[sure], angle.argmin(1)[sure])
        assert torch.equal(raw == -1, ~rendered)
        seen["rendered"] += int(rendered.sum())
        seen["sure"] += int(sure.sum())
        seen["moved"] += int((raw != before["library_raw"].reshape(-1).long().cpu()).sum())
    print(seen)
    assert seen["sure"] > 0
    assert model._spectral_library is None


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _model_flags(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *BASE_FLAGS]


def _features_file(world):
    wl = world["wl"]
    path = world["root"] / "features.json"
    path.write_text(json.dumps({"features": [{"name": "low", "window": [wl[0], wl[3]]}, {"name": "mid", "window": [wl[2], wl[6]]}]}))
    return path


def test_render_dataset_with_continuum_outputs(world, capsys):
    from PIL import Image

    from umhsnerf import render

    root = world["root"]
    out = render.main(["dataset", *_model_flags(world), "--split", "test", "--output-path", str(root / "ds_cr"), "--continuum-features",
                       str(_features_file(world)), "--rendered-output-names", "rgb", "cr_3", "feature_depth_0"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == out
    assert out["frames"] >= 1 and out["files"] == 3 * out["frames"]
    assert out["continuum"] == {"features": ["low", "mid"], "ranges": [[0, 3], [2, 6]]}
    for name in ("rgb", "cr_3", "feature_depth_0"):
        files = sorted((root / "ds_cr" / "test" / name).glob("*.png"))
        assert len(files) == out["frames"]
        assert np.asarray(Image.open(files[0])).shape == (out["height"], out["width"], 3)
    # cr needs no file; a feature does
    out = render.main(["dataset", *_model_flags(world), "--split", "test", "--output-path", str(root / "ds_cr2"), "--rendered-output-names", "cr_3"])
    capsys.readouterr()
    assert out["continuum"] == {"features": [], "ranges": []} and len(list((root / "ds_cr2" / "test" / "cr_3").glob("*.png"))) == out["frames"]
    with pytest.raises(ValueError, match="--continuum-features"):
        render.main(["dataset", *_model_flags(world), "--split", "test", "--output-path", str(root / "no"), "--rendered-output-names", "feature_depth_0"])
    assert not (root / "no").exists() and world["pipe"].model._continuum is None


def test_eval_with_features_emits_the_tallys_keys_and_they_are_numpys(world, capsys):
    from umhsnerf import eval as umhs_eval
    from umhsnerf.continuum import ContinuumAnalysis

    path = _features_file(world)
    got = umhs_eval.main([*_model_flags(world), "--continuum-features", str(path)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "psnr" in got
    keys = ("feature_depth_rmse", "feature_center_mae", "feature_depth_rendered_mean", "feature_depth_captured_mean")
    assert got["feature_names"] == ["low", "mid"] and all(len(got[k]) == 2 for k in keys)
    pipe = world["pipe"]
    a = ContinuumAnalysis.from_file(path, world["wl"])
    sq, ce, ren, cap, n = np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), 0
    for rb, batch in pipe.datamanager.eval_images():
        with pipe.model.continuum_context(a):
            out = pipe.model.get_outputs_for_camera_ray_bundle(rb)
        _, feats, status = a.run(batch["hs_image"].to(DEV).float().reshape(-1, 8), False, True)
        counted = ((out["accumulation"].reshape(-1) > 0.5) & (status != -1)).cpu().numpy()
        feats = feats.double().cpu().numpy()
        depth = out["feature_depth"].reshape(-1, 2).double().cpu().numpy()
        center = np.stack([out[f"feature_center_{f}"].reshape(-1).double().cpu().numpy() for f in range(2)], 1)
        sq += ((depth - feats[:, :, 0]) ** 2)[counted].sum(0)
        ce += np.abs(center - feats[:, :, 1])[counted].sum(0)
        ren += depth[counted].sum(0)
        cap += feats[:, :, 0][counted].sum(0)
        n += int(counted.sum())
    assert n > 0
    assert got["feature_depth_rmse"] == pytest.approx(list(np.sqrt(sq / n)), rel=1e-9)
    assert got["feature_center_mae"] == pytest.approx(list(ce / n), rel=1e-9)
    assert got["feature_depth_rendered_mean"] == pytest.approx(list(ren / n), rel=1e-9)
    assert got["feature_depth_captured_mean"] == pytest.approx(list(cap / n), rel=1e-9)
    assert pipe.model._continuum is None


def test_the_captured_command_writes_the_oracles_features_of_the_frames(world, capsys):
    from umhsnerf import continuum
    from umhsnerf.continuum import ContinuumAnalysis

    root, pipe = world["root"], world["pipe"]
    path = _features_file(world)
    got = continuum.main(["captured", *_model_flags(world), "--split", "train", "--continuum-features", str(path), "--output-path",
                          str(root / "captured_cr"), "--save-removed"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got == json.loads((root / "captured_cr" / "summary.json").read_text())
    stack = pipe.datamanager.train_split.hs_image
    assert len(got["frames"]) == stack.shape[0] > 0 and got["continuum"] == {"features": ["low", "mid"], "ranges": [[0, 3], [2, 6]]}
    a = ContinuumAnalysis.from_file(path, world["wl"])
    for i, frame in enumerate(got["frames"][:2]):
        feats = np.load(root / "captured_cr" / f"{frame['frame']}_features.npy")
        cube = np.load(root / "captured_cr" / f"{frame['frame']}_cr.npy")
        assert feats.shape == (*stack.shape[1:3], 2, 3) and cube.shape == (*stack.shape[1:3], 8) and feats.dtype == cube.dtype == np.float32
        case, ref = _frame_case(a, stack[i].float())
        report = {}
        fails = CF.check(case, cube.reshape(-1, 8), feats.reshape(-1, 2, 3), None, report, ref=ref)
        assert not fails, (frame["frame"], fails, report)
        v = case["valid"]
        assert frame["invalid"] == int((~v).sum())
        assert frame["mean_depth"] == pytest.approx(list(feats.reshape(-1, 2, 3)[v][:, :, 0].astype(np.float64).mean(0)), rel=1e-9)
        assert frame["mean_area"] == pytest.approx(list(feats.reshape(-1, 2, 3)[v][:, :, 2].astype(np.float64).mean(0)), rel=1e-9)


def test_the_endmembers_command_prints_the_host_numbers(world, capsys):
    from umhsnerf import continuum
    from umhsnerf.continuum import ContinuumAnalysis

    path = _features_file(world)
    got = continuum.main(["endmembers", *_model_flags(world), "--continuum-features", str(path)])
    captured = capsys.readouterr()
    lines = [ln for ln in captured.out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "low [" in captured.err and "endmember 0 depth" in captured.err
    a = ContinuumAnalysis.from_file(path, world["wl"])
    E = world["pipe"].model.field.endmembers.detach().float().clamp(0, 1).cpu().numpy()
    ref = CF.run(a.wavelengths, E, a.ranges, np.float64)["features"]
    assert [r["endmember"] for r in got["endmembers"]] == [0, 1, 2]
    for k, row in enumerate(got["endmembers"]):
        for f, name in enumerate(("low", "mid")):
            n = row["features"][name]
            assert (n["depth"], n["area"]) == pytest.approx((ref[k, f, 0], ref[k, f, 2]), abs=1e-12)
            if ref[k, f, 0] > 1e-9:
                assert n["center"] == ref[k, f, 1]
