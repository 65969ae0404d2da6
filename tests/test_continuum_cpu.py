"""Continuum removal without a GPU: the float64 oracle of tests/continuum_f64.py against a brute-force evaluation, the package's host
function against the oracle, a float32 replay of the kernel's arithmetic against every derived bound, the features file and its
refusals, the flags, the output names and the argument rules of the new C entry point (it returns before any launch)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import continuum_f64 as CF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--data", "scene", "--checkpoint", "model.ckpt"]
SYMBOLS = ("umhs_continuum_workspace_bytes", "umhs_continuum")
SMALL = [c for c in CF.CASES if c[0] <= 33 and c[1] > 0]
RUN = [c for c in CF.CASES if c[1] > 0]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SMALL, ids=CF.case_id)
def test_the_float64_oracle_is_the_brute_force_hull(c):
    case, ref = CF.reference(*c)
    rows = np.nonzero(case["valid"])[0][:48]  # (every row kind is among the first 14)
    assert rows.size
    for r in rows:
        brute = CF.brute_continuum(case["lam"], case["x"][r])
        scale = max(np.abs(case["x"][r].astype(np.float64)).max(), 1e-300)
        assert np.abs(brute - ref["c"][r]).max() <= 1e-12 * scale, (r, np.abs(brute - ref["c"][r]).max() / scale)
        for k, (lo, hi) in enumerate(case["ranges"]):  # a feature's hull is the hull of its own range
            brute = CF.brute_continuum(case["lam"][lo:hi + 1], case["x"][r, lo:hi + 1])
            assert np.abs(brute - ref["per_feature"][k]["c"][r]).max() <= 1e-12 * scale, (r, k)


@pytest.mark.parametrize("c", RUN, ids=CF.case_id)
def test_the_host_function_is_the_oracle(c):
    from umhsnerf import continuum

    case, ref = CF.reference(*c)
    x = np.ascontiguousarray(case["x"])
    removed = continuum.continuum_removed(x, case["lam"])
    assert removed.dtype == np.float64 and removed.shape == x.shape
    assert np.abs(removed - ref["removed"]).max() <= 1e-12 * max(1.0, np.abs(ref["removed"]).max())
    v = case["valid"]
    assert (removed[~v] == 0).all()
    if v.any():
        scale = max(np.abs(x[v].astype(np.float64)).max(), 1e-300)
        assert np.abs(continuum.continuum(x[v], case["lam"]) - ref["c"][v]).max() <= 1e-12 * scale
    if case["ranges"]:
        numbers = continuum.feature_numbers(x, case["lam"], case["ranges"])
        assert np.abs(numbers[..., 0] - ref["features"][..., 0]).max() <= 1e-12
        assert np.abs(numbers[..., 2] - ref["features"][..., 2]).max() <= 1e-12 * float(case["lam"][-1] - case["lam"][0])
        assert (numbers[~v] == 0).all()


def test_the_hull_of_a_known_row():
    lam, x = np.array([0, 1, 2, 3, 4], np.float32), np.array([[2, 1, 4, 1, 2], [1, 2, 3, 4, 5], [3, 3, 3, 3, 3]], np.float32)
    out = CF.run(lam, x, [(0, 4), (2, 4)], np.float64)
    assert out["status"].tolist() == [3, 2, 2]  # collinear and constant rows keep their endpoints only
    assert np.allclose(out["c"][0], [2, 3, 4, 3, 2]) and np.allclose(out["removed"][0], [1, 1 / 3, 1, 1 / 3, 1])
    assert np.allclose(out["features"][0, 0], [2 / 3, 1.0, 0.5 * (2 / 3) * 4])  # depth, the FIRST band at the minimum, trapezoid area
    assert np.allclose(out["features"][0, 1], [1 - 1 / 3, 3.0, 2 / 3])  # the local hull of bands 2..4: 4 -> 2
    assert np.allclose(out["features"][1:, :, 0], 0)


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def test_the_float32_replay_stays_inside_every_bound():
    worst, at, differing = dict(c=0.0, r=0.0, depth=0.0, centre=0.0, area=0.0), {}, 0
    for c in RUN:
        case, ref = CF.reference(*c)
        rep = CF.run(case["lam"], case["x"], case["ranges"], np.float32)
        report = {}
        fails = CF.check(case, rep["removed"], rep["features"] if case["ranges"] else None, rep["status"], report, c=rep["c"])
        assert not fails, (CF.case_id(c), fails, report)
        differing += int((rep["status"] != ref["status"]).sum())
        for k, v in report.items():
            if v > worst[k]:
                worst[k], at[k] = v, CF.case_id(c)
    # not vacuous: the bounds are worst-case ones, yet the replay comes within two orders of magnitude of them, and the vertex sets DO differ
    assert all(v < 1.0 for v in worst.values()) and worst["c"] > 1e-3 and worst["r"] > 1e-3 and differing > 0, (worst, at, differing)


def test_check_rejects_what_is_wrong():
    c = (31, 300, "rows", "uni", 8)
    case, ref = CF.reference(*c)
    good = CF.run(case["lam"], case["x"], case["ranges"], np.float32)
    v = np.nonzero(case["valid"])[0]
    full = CF.run(case["lam"], case["x"], [(0, 30)] * 8, np.float32)  # the full-range hull in place of the local ones
    assert any("depth" in f or "area" in f for f in CF.check(case, None, full["features"], None))
    bad = good["removed"].copy()
    bad[v[8], 15] *= 1.01
    assert any(f.startswith("r:") for f in CF.check(case, bad, None, None))
    feats = good["features"].copy()
    feats[v[8], 0, 1] = 123.456
    assert any("centre" in f for f in CF.check(case, None, feats, None))
    feats = good["features"].copy()
    k = np.argmax(ref["features"][:, 3, 0])  # a row with a real feature: its centre moved to the window's edge
    feats[k, 3, 1] = case["lam"][case["ranges"][3][0]]
    assert any("centre" in f for f in CF.check(case, None, feats, None))
    status = good["status"].copy()
    status[~case["valid"]] = 2
    assert any("status" in f for f in CF.check(case, None, None, status))
    dead = good["removed"].copy()
    dead[~case["valid"]] = 1.0
    assert any("invalid" in f for f in CF.check(case, dead, None, None))
    exact, eref = CF.reference(4, 65, "rows", "int", 8)
    wrong = eref["status"].copy()
    wrong[0] += 1
    assert any("exact" in f for f in CF.check(exact, None, None, wrong))


def test_the_cases_cover_what_they_must():
    assert {c[0] for c in CF.CASES} >= {1, 2, 3, 4, 31, 33, 141, 256} and {c[1] for c in CF.CASES} >= {0, 1, 63, 64, 65}
    assert any(c[1] > 256 and c[1] % 64 for c in CF.CASES) and {c[4] for c in CF.CASES} == {0, 1, 8}
    assert {c[2] for c in CF.CASES} == {"rows", "slice"} and {c[3] for c in CF.CASES} == {"uni", "non", "int", "golden"}
    # the golden scenes' own band lists, each of them, with features and as a slice; they are what the model fixtures carry
    golden = [c for c in CF.CASES if c[3] == "golden"]
    assert {c[0] for c in golden} == set(CF.GOLDEN_BANDS) >= {31, 128, 141}
    assert any(c[4] == 8 for c in golden) and any(c[2] == "slice" for c in golden) and any(c[2] == "slice" and c[4] for c in golden)
    for name, B in (("g8_model_rgb_c5b21", 21), ("g8_model_rs_c6b31s", 31), ("g8_model_rs_c9b128s", 128), ("g8_model_s_c4b141n", 141)):
        with np.load(os.path.join(CF.GOLDEN, name + ".npz")) as f:
            assert np.array_equal(np.asarray(f["bands"]).astype(np.float32), CF.wavelengths("golden", B)), name
    for c in CF.CASES:
        case = CF.make_case(*c)
        for lo, hi in case["ranges"]:
            assert 0 <= lo and hi < c[0] and hi - lo >= 2
        if c[4] == 8:
            r = case["ranges"]
            assert r[0] == (0, c[0] - 1) and r[1][0] == 0 and r[2][1] == c[0] - 1 and any(hi - lo == 2 for lo, hi in r)
        if c[1] >= 65 and c[3] != "int":
            assert (~case["valid"]).any() and case["valid"].any()
    case, ref = CF.reference(256, 64, "rows", "uni", 8)
    assert ref["status"][0] == 256 and ref["status"][1] == 2 and ref["status"][3] == 2 and ref["status"][4] == 2  # dome, bowl, collinear, constant
    assert ref["features"][8, 0, 0] > 0.5  # the deep narrow feature


# ---- the analysis and its file ---------------------------------------------------------------------------------------------------
def test_windows_become_band_ranges_at_exact_edges():
    from umhsnerf.continuum import ContinuumAnalysis, window_range

    lam = [400 + 10 * b for b in range(31)]
    assert window_range(np.float32(lam), (640, 700)) == (24, 30) and window_range(np.float32(lam), (640.001, 699.999)) == (25, 29)
    assert window_range(np.float32(lam), (100, 200)) == (0, -1)
    a = ContinuumAnalysis(lam, [{"name": "chlorophyll", "window": [640, 700]}, ("blue", (400, 420))])
    assert a.names == ["chlorophyll", "blue"] and a.ranges == [(24, 30), (0, 2)] and a.bands == 31 and len(a) == 2
    assert a.summary() == {"features": ["chlorophyll", "blue"], "ranges": [[24, 30], [0, 2]]}
    assert a.wavelengths.dtype == np.float32 and len(ContinuumAnalysis(lam)) == 0


def test_every_refusal_names_what_is_wrong(tmp_path):
    from umhsnerf.continuum import ContinuumAnalysis

    lam = [400 + 10 * b for b in range(31)]
    with pytest.raises(ValueError, match=r"wavelength 3 \(420\) does not exceed wavelength 2 \(430\)"):
        ContinuumAnalysis([400, 410, 430, 420, 440])
    with pytest.raises(ValueError, match="wavelength 2 .*does not exceed"):
        ContinuumAnalysis([400, 410, 410, 420])
    with pytest.raises(ValueError, match="wavelength 1 is not finite"):
        ContinuumAnalysis([400, float("nan"), 420])
    with pytest.raises(ValueError, match="1..256"):
        ContinuumAnalysis(list(range(257)))
    with pytest.raises(ValueError, match="'narrow'.*holds 2 of the scene's bands.*at least 3"):
        ContinuumAnalysis(lam, [("wide", (400, 500)), ("narrow", (405, 425))])
    with pytest.raises(ValueError, match="'outside'.*holds 0"):
        ContinuumAnalysis(lam, [("outside", (900, 1000))])
    with pytest.raises(ValueError, match="'f3' is named twice"):
        ContinuumAnalysis(lam, [(f"f{i}", (400, 500)) for i in (1, 2, 3, 3)])
    with pytest.raises(ValueError, match="9 features.*f8.*at most 8"):
        ContinuumAnalysis(lam, [(f"f{i}", (400, 500)) for i in range(9)])
    with pytest.raises(ValueError, match="'bad'.*two numbers"):
        ContinuumAnalysis(lam, [("bad", (400,))])
    path = tmp_path / "features.json"
    path.write_text(json.dumps({"features": [{"name": "chlorophyll", "window": [640, 700]}, {"name": "edge", "window": [680, 700]}]}))
    a = ContinuumAnalysis.from_file(path, lam)
    assert a.names == ["chlorophyll", "edge"] and a.ranges == [(24, 30), (28, 30)] and a.windows == [(640.0, 700.0), (680.0, 700.0)]
    path.write_text(json.dumps({"features": [{"name": "chlorophyll"}]}))
    with pytest.raises(ValueError, match="features file"):
        ContinuumAnalysis.from_file(path, lam)
    path.write_text("{not json")
    with pytest.raises(ValueError, match="not JSON"):
        ContinuumAnalysis.from_file(path, lam)
    path.write_text(json.dumps({"features": [{"name": "thin", "window": [401, 419]}]}))
    with pytest.raises(ValueError, match="'thin'"):
        ContinuumAnalysis.from_file(path, lam)


def test_a_library_with_its_continuum_removed():
    from umhsnerf.continuum import continuum_removed
    from umhsnerf.library import SpectralLibrary

    lam = [400 + 10 * b for b in range(31)]
    t = np.linspace(0, 1, 31)
    spectra = np.stack([0.2 + 0.5 * t, (0.2 + 0.5 * t) * (1 - 0.5 * np.exp(-0.5 * ((t - 0.5) / 0.05) ** 2))])
    library = SpectralLibrary(["flat", "dip"], spectra, lam)
    removed = library.continuum_removed()
    assert removed is library.continuum_removed() and removed.continuum_removed() is removed and removed.names == library.names
    assert np.array_equal(removed.spectra, continuum_removed(spectra, np.float32(lam)))
    assert np.allclose(removed.spectra[0], 1.0) and abs(removed.spectra[1].min() - 0.5) < 1e-3
    assert library._removed_with is None and np.array_equal(library.spectra, spectra)  # the library itself is what it was


# ---- flags and names -------------------------------------------------------------------------------------------------------------
def test_parsers_accept_the_new_flags_and_refuse_what_they_must():
    from umhsnerf import continuum, render
    from umhsnerf import eval as umhs_eval

    out = ["--output-path", "out"]
    for argv in (["camera-path", "--camera-path-filename", "path.json"], ["dataset"], ["interpolate"]):
        args = render.parse_args(argv[:1] + MODEL + out + argv[1:] + ["--continuum-features", "f.json", "--rendered-output-names", "rgb",
                                                                       "cr_3", "feature_depth_0", "feature_center_1", "feature_area_7"])
        assert args.continuum_features == "f.json" and not args.library_continuum_removed
        args = render.parse_args(argv[:1] + MODEL + out + argv[1:] + ["--rendered-output-names", "rgb", "cr_3"])  # cr needs no file
        assert args.continuum_features is None
    for name in ("feature_depth_0", "feature_center_0", "feature_area_2", "feature_depth"):
        with pytest.raises(ValueError, match="--continuum-features"):
            render.parse_args(["dataset"] + MODEL + out + ["--rendered-output-names", "rgb", name])
    args = render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + ["--cube-output-names", "cr"])
    assert args.cube_output_names == ["cr"]
    with pytest.raises(ValueError, match="--continuum-features"):
        render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + ["--cube-output-names", "feature_depth"])
    args = render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + [
        "--cube-output-names", "cr", "feature_depth", "--continuum-features", "f.json"])
    assert args.cube_output_names == ["cr", "feature_depth"]
    with pytest.raises(ValueError, match="--spectral-library"):
        render.parse_args(["dataset"] + MODEL + out + ["--library-continuum-removed"])
    args = render.parse_args(["dataset"] + MODEL + out + ["--library-continuum-removed", "--spectral-library", "lib.npz"])
    assert args.library_continuum_removed
    args = umhs_eval.build_parser().parse_args(MODEL + ["--continuum-features", "f.json", "--library-continuum-removed"])
    assert args.continuum_features == "f.json" and args.library_continuum_removed
    assert umhs_eval.build_parser().parse_args(MODEL).continuum_features is None
    args = continuum.build_parser().parse_args(["captured"] + MODEL + out + ["--split", "val", "--continuum-features", "f.json", "--save-removed"])
    assert (args.command, args.split, args.output_path, args.continuum_features, args.save_removed) == ("captured", "val", "out", "f.json", True)
    args = continuum.build_parser().parse_args(["endmembers"] + MODEL + ["--continuum-features", "f.json"])
    assert args.command == "endmembers"
    with pytest.raises(SystemExit):
        continuum.build_parser().parse_args(["captured"] + MODEL + out)


def test_output_name_helpers():
    from umhsnerf import continuum

    assert continuum.continuum_outputs(2, 1) == ("cr", "cr_0", "cr_1", "feature_depth", "feature_depth_0", "feature_center_0", "feature_area_0")
    assert continuum.continuum_outputs(1, 0) == ("cr", "cr_0")
    for name in ("cr", "cr_0", "cr_255", "feature_depth", "feature_depth_7", "feature_center_0", "feature_area_3"):
        assert continuum.is_continuum_output(name), name
    for name in ("cr_", "cr_x", "crop", "feature_center", "feature_area", "feature_width_0", "wv_3", "spectral", "unmix_0"):
        assert not continuum.is_continuum_output(name), name
    assert continuum.continuum_index("cr_12") == ("cr", 12) and continuum.continuum_index("feature_depth") == ("feature_depth", None)
    assert continuum.needs_removed("cr") and continuum.needs_removed("cr_3") and not continuum.needs_removed("feature_depth_0")
    continuum.requested_without_features(["rgb", "cr", "cr_3"], None)
    continuum.requested_without_features(["feature_depth_0"], "f.json")
    with pytest.raises(ValueError, match="feature_area_1.*--continuum-features"):
        continuum.requested_without_features(["rgb", "feature_area_1"], None)


def test_the_model_context_checks_on_entry():
    from types import SimpleNamespace

    from umhsnerf.continuum import ContinuumAnalysis
    from umhsnerf.umhs_model import UMHSModel

    lam = [400 + 10 * b for b in range(8)]
    model = SimpleNamespace(config=SimpleNamespace(method="rgb"), kwargs={"wavelengths": lam}, _continuum=None)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with UMHSModel.continuum_context(model, ContinuumAnalysis(lam)):
            pass
    model.config.method = "spectral"
    with pytest.raises(ValueError, match="9 wavelengths; the model has 8"):
        with UMHSModel.continuum_context(model, ContinuumAnalysis(lam + [480])):
            pass
    a = ContinuumAnalysis(lam)
    with UMHSModel.continuum_context(model, a):
        assert model._continuum == (a, None)
        with UMHSModel.continuum_context(model, None):
            assert model._continuum is None
        with UMHSModel.continuum_context(model, a, ["cr_3", "rgb"]):  # what a render without output_names builds
            assert model._continuum == (a, ("cr_3", "rgb"))
        assert model._continuum == (a, None)
    assert model._continuum is None


# ---- C ABI, host side only -------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(built_library):
    from umhsnerf import _hip, build, ops

    with open(os.path.join(ROOT, "include", "umhs_hip.h")) as f:
        header = f.read()
    assert "Continuum removal" in header and "#define UMHS_CONTINUUM_MAX_BANDS 256" in header and "#define UMHS_CONTINUUM_MAX_FEATURES 8" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in _hip.SIGNATURES and f"{name}(" in header and f" T {name}\n" in exported, name
    assert "umhs_continuum.hip" in build.SOURCES
    assert _hip.ABI_VERSION == 11 == _hip.lib().umhs_abi_version()
    assert (ops.CONTINUUM_MAX_BANDS, ops.CONTINUUM_MAX_FEATURES) == (256, 8) and callable(ops.continuum)


def test_argument_rules_run_before_any_launch(built_library):
    from umhsnerf import _hip

    lib, d = _hip.lib(), ctypes.c_void_p(4096)
    ARG = -1
    assert lib.umhs_continuum_workspace_bytes(921600, 256, 8) == 0 and lib.umhs_continuum_workspace_bytes(0, 1, 0) == 0
    ranges = lambda *r: ctypes.cast((ctypes.c_int32 * max(len(r), 1))(*r), ctypes.c_void_p)
    call = lambda **kw: lib.umhs_continuum(*[kw.get(k, v) for k, v in dict(
        spectra=d, stride=31, R=8, wavelengths=d, B=31, ranges=ranges(0, 30, 3, 5), F=2, removed=d, features=d, status=d, workspace=None,
        nbytes=0, stream=None).items()])
    assert call(spectra=None) == ARG and call(wavelengths=None) == ARG  # NULL inputs with R > 0
    assert call(B=0) == ARG and call(B=257, stride=257) == ARG and call(F=-1) == ARG and call(F=9) == ARG and call(R=-1) == ARG
    assert call(stride=30) == ARG and call(ranges=None) == ARG
    assert call(ranges=ranges(-1, 5, 3, 5)) == ARG and call(ranges=ranges(0, 31, 3, 5)) == ARG  # outside [0, B)
    assert call(ranges=ranges(0, 30, 6, 5)) == ARG and call(ranges=ranges(0, 30, 4, 5)) == ARG  # lo > hi; fewer than 3 bands
    assert call(ranges=ranges(0, 30, 4, 5), R=0) == ARG  # the ranges are judged whatever R is
    assert call(R=0) == 0 and call(R=0, spectra=None, wavelengths=None, removed=None, features=None, status=None) == 0
    assert call(R=0, F=0, ranges=None) == 0


def test_the_op_has_no_cpu_path_and_checks_its_arguments():
    import torch

    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.continuum(torch.rand(8, 5), torch.arange(5.0))
    with pytest.raises(ValueError, match="float32"):
        ops.continuum(torch.rand(8, 5).double(), torch.arange(5.0))
