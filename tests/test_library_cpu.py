"""CPU checks of the spectral-library layer: the loader (``umhsnerf.library.SpectralLibrary``), ``classify`` on a hand-written table,
the host-side argument rules of the three C entry points, and the new command-line flags."""
import ctypes

import numpy as np
import pytest
import torch

SCENE = [450.0, 500.0, 560.0, 610.0, 690.0]


def _library_arrays():
    wl = np.array([400.0, 480.0, 520.0, 600.0, 650.0, 700.0])
    spectra = np.array([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0.9, 0.7, 0.5, 0.3, 0.2, 0.1], [0.3, 0.3, 0.8, 0.3, 0.3, 0.3]])
    return ["grass", "brick", "paint"], wl, spectra


def _write_csv(path, names, wl, spectra):
    with open(path, "w") as f:
        f.write("wavelength," + ",".join(names) + "\n")
        for i, w in enumerate(wl):
            f.write(",".join([repr(float(w))] + [("" if np.isnan(v) else repr(float(v))) for v in spectra[:, i]]) + "\n")


# ---- loader --------------------------------------------------------------------------------------------------------------------
def test_npz_and_csv_round_trip_and_resampling_is_numpy_interp(tmp_path):
    from umhsnerf.library import SpectralLibrary
    from umhsnerf.umhs_model import CLASS_COLORS

    names, wl, spectra = _library_arrays()
    colors = np.array([[0.0, 0.5, 0.0], [0.6, 0.2, 0.1], [1.0, 1.0, 1.0]], np.float32)
    np.savez(tmp_path / "lib.npz", names=np.array(names), wavelengths=wl, spectra=spectra, colors=colors)
    np.savez(tmp_path / "plain.npz", names=np.array(names), wavelengths=wl, spectra=spectra)
    _write_csv(tmp_path / "lib.csv", names, wl, spectra)
    want = np.stack([np.interp(np.array(SCENE), wl, row) for row in spectra])
    a, b, c = (SpectralLibrary.load(tmp_path / n, SCENE) for n in ("lib.npz", "lib.csv", "plain.npz"))
    for lib in (a, b, c):
        assert lib.names == names and lib.wavelengths == SCENE and len(lib) == 3
        assert lib.spectra.dtype == np.float64 and np.array_equal(lib.spectra, want)
    assert np.array_equal(a.colors, colors)
    assert np.array_equal(b.colors, CLASS_COLORS.numpy()[:3]) and np.array_equal(c.colors, b.colors)
    unit = a.unit()
    assert unit.dtype == torch.float32 and torch.equal(unit, torch.from_numpy(want / np.linalg.norm(want, axis=1, keepdims=True)).float())
    # the palette cycles past 15 entries
    many = SpectralLibrary([f"e{i}" for i in range(17)], np.random.default_rng(0).random((17, 5)) + 0.1, SCENE)
    assert np.array_equal(many.colors[15:], CLASS_COLORS.numpy()[:2])


def test_scene_wavelengths_come_from_metadata_or_config_json(tmp_path):
    import json

    from umhsnerf.library import scene_wavelengths

    (tmp_path / "config.json").write_text(json.dumps({"derived": {"wavelengths": SCENE, "num_classes": 3}}))
    assert scene_wavelengths(tmp_path / "config.json") == SCENE
    assert scene_wavelengths({"wavelengths": np.array(SCENE)}) == SCENE

    class Outputs:
        metadata = {"wavelengths": SCENE}

    assert scene_wavelengths(Outputs()) == SCENE


def test_refusals_name_the_entries(tmp_path):
    from umhsnerf.library import SpectralLibrary

    names, wl, spectra = _library_arrays()
    with pytest.raises(ValueError, match="strictly ascending.*position 2"):
        SpectralLibrary.resampled(names, [400.0, 480.0, 480.0, 600.0, 650.0, 700.0], spectra, SCENE)
    short = spectra.copy()
    short[1, 0] = np.nan  # brick starts at 480 nm: the scene's 450 nm is not covered
    short[2, -1] = np.nan  # paint ends at 650 nm
    with pytest.raises(ValueError, match="do not cover.*brick, paint"):
        SpectralLibrary.resampled(names, wl, short, SCENE)
    _write_csv(tmp_path / "short.csv", names, wl, short)
    with pytest.raises(ValueError, match="do not cover.*brick, paint"):
        SpectralLibrary.load(tmp_path / "short.csv", SCENE)
    with pytest.raises(ValueError, match="do not cover.*grass, brick, paint"):
        SpectralLibrary.resampled(names, wl, spectra, [300.0, 500.0])
    bad = spectra.copy()
    bad[0, 2] = np.inf
    bad[2] = 0.0
    with pytest.raises(ValueError, match="not finite or all zero.*grass, paint"):
        SpectralLibrary.resampled(names, wl, bad, SCENE)
    seven = [f"e{i}" for i in range(7)]
    with pytest.raises(ValueError, match=r"e0, e1, e2, e3, e4 \(and 2 more\)"):
        SpectralLibrary.resampled(seven, wl, np.zeros((7, 6)), SCENE)
    with pytest.raises(ValueError, match="1..65536 entries"):
        SpectralLibrary.resampled([], wl, np.zeros((0, 6)), SCENE)
    with pytest.raises(ValueError, match="1..65536 entries"):
        SpectralLibrary.resampled(["x"] * 65537, wl, np.ones((65537, 6)), SCENE)
    with pytest.raises(ValueError, match="1..256 bands"):
        SpectralLibrary.resampled(names, wl, spectra, np.linspace(450, 690, 257))
    with pytest.raises(ValueError, match=".npz or a .csv"):
        SpectralLibrary.load(tmp_path / "lib.sli", SCENE)


# ---- classify ------------------------------------------------------------------------------------------------------------------
def test_classify_against_a_hand_written_table():
    from umhsnerf.library import SpectralLibrary

    colors = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
    lib = SpectralLibrary(*[_library_arrays()[0], np.ones((3, 5)), SCENE], colors=colors)
    half, r32 = float(np.cos(0.5)), float(np.cos(0.25))
    #                    matched      empty pixel   kernel said -1   angle too large   cosine past 1
    index = torch.tensor([[2, 0], [1, 2], [-1, -1], [0, 1], [1, 0]], dtype=torch.int32)
    cos = torch.tensor([[r32, half], [1.0, half], [0.0, 0.0], [half, 0.0], [1.0000001, r32]])
    acc = torch.tensor([[0.9], [0.5], [1.0], [1.0], [0.51]])
    out = lib.classify(index, cos, acc, max_angle=0.4)
    assert {k: tuple(v.shape) for k, v in out.items()} == {"library_raw": (5, 1), "library_pred": (5, 3), "library_angle": (5, 1),
                                                            "library_margin": (5, 1)}
    assert out["library_raw"].dtype == torch.float32 and out["library_raw"][:, 0].tolist() == [2.0, -1.0, -1.0, -1.0, 1.0]
    assert out["library_pred"].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 0]]
    assert torch.allclose(out["library_angle"][:, 0], torch.tensor([0.25, 0.0, np.pi / 2, 0.5, 0.0]), atol=1e-6)
    assert torch.allclose(out["library_margin"][:, 0], torch.tensor([0.25, 0.5, 0.0, np.pi / 2 - 0.5, 0.25]), atol=1e-6)
    # without the mask and the threshold only the kernel's -1 is unmatched
    assert lib.classify(index, cos)["library_raw"][:, 0].tolist() == [2.0, 1.0, -1.0, 0.0, 1.0]
    # max_angle = 0 unmatches everything that is not an exact hit
    assert lib.classify(index, cos, acc, max_angle=0.0)["library_raw"][:, 0].tolist() == [-1.0, -1.0, -1.0, -1.0, 1.0]
    # a library of one entry: the second is (-1, -1.0) and the margin is pi - angle
    one = SpectralLibrary(["only"], np.ones((1, 5)), SCENE)
    o = one.classify(torch.tensor([[0, -1]], dtype=torch.int32), torch.tensor([[r32, -1.0]]))
    assert o["library_raw"].tolist() == [[0.0]] and abs(float(o["library_margin"]) - (np.pi - 0.25)) < 1e-6
    assert o["library_pred"].tolist() == [one.colors[0].tolist()]


# ---- C ABI, host side only -----------------------------------------------------------------------------------------------------
def test_argument_rules_run_before_any_launch(built_library):
    from umhsnerf import _hip, build

    lib, d = _hip.lib(), ctypes.c_void_p(4096)
    ARG, UNSUPPORTED = -1, -2
    match = lambda **kw: lib.umhs_library_match(*[kw.get(k, v) for k, v in dict(
        spectra=d, stride=31, R=8, image=d, L=5, B=31, index=d, cos=d, stream=None).items()])
    for missing in ("spectra", "image", "index", "cos"):
        assert match(**{missing: None}) == ARG, missing
    assert match(L=0) == ARG and match(B=0) == ARG and match(R=-1) == ARG and match(stride=30) == ARG
    assert match(B=257, stride=257) == UNSUPPORTED and match(L=65537) == UNSUPPORTED
    assert match(R=0) == 0 and match(R=0, spectra=None, image=None, index=None, cos=None) == 0
    prepare = lambda **kw: lib.umhs_library_prepare(*[kw.get(k, v) for k, v in dict(unit=d, L=5, B=31, image=d, stream=None).items()])
    assert prepare(unit=None) == ARG and prepare(image=None) == ARG and prepare(L=0) == ARG and prepare(B=0) == ARG
    assert prepare(B=257) == UNSUPPORTED and prepare(L=65537) == UNSUPPORTED
    for L, B in ((1, 1), (5, 31), (33, 65), (2048, 141), (65536, 256)):
        assert lib.umhs_library_image_bytes(L, B) >= L * B * 4
    assert lib.umhs_library_image_bytes(0, 31) == 0 and lib.umhs_library_image_bytes(5, 257) == 0
    assert _hip.ABI_VERSION == 11 == lib.umhs_abi_version()
    assert "umhs_library.hip" in build.SOURCES
    for name in ("umhs_library_image_bytes", "umhs_library_prepare", "umhs_library_match"):
        assert name in _hip.SIGNATURES


def test_ops_have_no_cpu_path():
    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.library_prepare(torch.rand(5, 31))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.library_match(torch.rand(8, 31), torch.zeros(16), 5)


# ---- flags ---------------------------------------------------------------------------------------------------------------------
MODEL = ["--data", "scene", "--checkpoint", "model.ckpt"]


def test_parsers_accept_the_new_flags():
    from umhsnerf import eval as umhs_eval
    from umhsnerf import library, render

    common = MODEL + ["--output-path", "out", "--spectral-library", "lib.npz", "--library-max-angle", "0.2"]
    for argv in (["camera-path", "--camera-path-filename", "path.json"], ["dataset"], ["interpolate"]):
        args = render.parse_args(argv[:1] + common + argv[1:] + ["--rendered-output-names", "rgb", "library_pred", "library_angle"])
        assert args.spectral_library == "lib.npz" and args.library_max_angle == 0.2
    args = render.parse_args(["dataset"] + MODEL + ["--output-path", "out"])
    assert args.spectral_library is None and args.library_max_angle is None
    args = umhs_eval.build_parser().parse_args(MODEL + ["--spectral-library", "lib.csv"])
    assert args.spectral_library == "lib.csv" and args.library_max_angle is None
    args = library.build_parser().parse_args(["identify"] + MODEL + ["--spectral-library", "lib.csv", "--top", "5"])
    assert args.command == "identify" and args.spectral_library == "lib.csv" and args.top == 5
    assert library.build_parser().parse_args(["identify"] + MODEL + ["--spectral-library", "lib.csv"]).top == 3


@pytest.mark.parametrize("name", ["library_raw", "library_pred", "library_angle", "library_margin"])
def test_a_library_output_without_the_flag_names_the_flag(name):
    from umhsnerf import render

    with pytest.raises(ValueError, match="--spectral-library"):
        render.parse_args(["dataset"] + MODEL + ["--output-path", "out", "--rendered-output-names", "rgb", name])
    with pytest.raises(ValueError, match="--spectral-library"):
        render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + ["--output-path", "out", "--cube-output-names", name])
