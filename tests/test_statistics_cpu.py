"""Scene statistics without a GPU: the host math of umhsnerf/statistics.py, the file format and its refusals, the threshold, the flags,
and the argument rules of the new C entry points (they return before any launch)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--data", "scene", "--checkpoint", "model.ckpt"]
SYMBOLS = ("umhs_gram_chunk", "umhs_gram_workspace_bytes", "umhs_gram_accumulate", "umhs_spectral_project")


def _rows(n=700, B=6, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, B)) @ rng.normal(size=(B, B)) * 0.1 + rng.uniform(0.2, 0.8, size=B)


def _stats(x, shift=None):
    from umhsnerf.statistics import SceneStatistics

    shift = x[0] if shift is None else shift
    c = x - shift
    acc = np.concatenate([[x.shape[0]], c.sum(0), (c.T @ c).reshape(-1)])
    return SceneStatistics.from_accumulator(acc, shift, [400.0 + 10 * i for i in range(x.shape[1])])


# ---- host math -------------------------------------------------------------------------------------------------------------------
def test_statistics_of_an_accumulator_are_numpys_mean_and_covariance():
    x = _rows()
    for shift in (None, np.zeros(6), x.mean(0)):
        s = _stats(x, shift)
        assert s.n == 700 and s.bands == 6
        np.testing.assert_allclose(s.mean, x.mean(0), rtol=1e-10)
        np.testing.assert_allclose(s.covariance, np.cov(x.T, bias=True), rtol=1e-10, atol=1e-14)
        assert np.array_equal(s.covariance, s.covariance.T)


def test_whitening_gives_the_identity_and_the_sign_and_floor_rules_hold():
    s = _stats(_rows())
    W, lam = s.whitening()
    assert W.dtype == lam.dtype == np.float64 and W.shape == (6, 6)
    assert np.all(np.diff(lam) <= 0) and s.floored() == 0
    np.testing.assert_allclose(W @ s.covariance @ W.T, np.eye(6), atol=1e-8)
    assert np.all(W[np.arange(6), np.abs(W).argmax(1)] > 0)  # the entry of largest magnitude is positive
    # a covariance of rank 2 on 6 bands: four eigenvalues sit exactly on the floor, every direction is kept
    rng = np.random.default_rng(3)
    low = rng.normal(size=(500, 2)) @ rng.normal(size=(2, 6)) + 0.5
    flat = _stats(low)
    for floor in (1e-6, 1e-3):
        W, lam = flat.whitening(floor)
        assert np.array_equal(lam[2:], np.full(4, floor * lam[0])) and lam[1] > floor * lam[0] and flat.floored(floor) == 4
        assert W.shape == (6, 6) and np.isfinite(W).all()
        np.testing.assert_allclose(np.linalg.norm(W, axis=1), 1.0 / np.sqrt(lam), rtol=1e-12)
        assert np.all(W[np.arange(6), np.abs(W).argmax(1)] > 0)
    from umhsnerf.statistics import SceneStatistics

    with pytest.raises(ValueError, match="positive eigenvalue"):
        SceneStatistics(10, np.zeros(3), np.zeros((3, 3)), [1.0, 2.0, 3.0]).whitening()
    with pytest.raises(ValueError, match="floor"):
        s.whitening(0.0)


def test_the_file_round_trip_is_exact_and_load_refuses_what_it_must(tmp_path):
    from umhsnerf.statistics import SceneStatistics

    s = _stats(_rows())
    s.save(tmp_path / "stats.npz")
    with np.load(tmp_path / "stats.npz") as f:
        assert sorted(f.files) == ["covariance", "mean", "n", "wavelengths"]
    back = SceneStatistics.load(tmp_path / "stats.npz", s.wavelengths)
    assert back.n == s.n and back.wavelengths == s.wavelengths
    assert np.array_equal(back.mean, s.mean) and np.array_equal(back.covariance, s.covariance)
    assert SceneStatistics.load(tmp_path / "stats.npz").n == s.n  # (no scene given: nothing to compare with)

    def written(**change):
        fields = dict(n=np.int64(s.n), wavelengths=np.asarray(s.wavelengths), mean=s.mean.copy(), covariance=s.covariance.copy())
        fields.update(change)
        fields = {k: v for k, v in fields.items() if v is not None}
        np.savez(tmp_path / "bad.npz", **fields)
        return tmp_path / "bad.npz"

    with pytest.raises(ValueError, match="not the scene's"):
        SceneStatistics.load(tmp_path / "stats.npz", [w + 5.0 for w in s.wavelengths])
    with pytest.raises(ValueError, match="not the scene's"):
        SceneStatistics.load(tmp_path / "stats.npz", s.wavelengths[:-1])
    with pytest.raises(ValueError, match="at least 2"):
        SceneStatistics.load(written(n=np.int64(1)), s.wavelengths)
    nan = s.mean.copy()
    nan[2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        SceneStatistics.load(written(mean=nan), s.wavelengths)
    inf = s.covariance.copy()
    inf[1, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        SceneStatistics.load(written(covariance=inf), s.wavelengths)
    skew = s.covariance.copy()
    skew[0, 3] = np.nextafter(skew[0, 3], np.inf)
    with pytest.raises(ValueError, match="not symmetric"):
        SceneStatistics.load(written(covariance=skew), s.wavelengths)
    with pytest.raises(ValueError, match="no array named mean"):
        SceneStatistics.load(written(mean=None), s.wavelengths)
    with pytest.raises(ValueError, match="at least 2"):
        SceneStatistics.from_accumulator(np.zeros(1 + 6 + 36), np.zeros(6), s.wavelengths)


def test_the_threshold_is_the_chi_square_quantile():
    """Wilson-Hilferty against tabulated upper quantiles of the chi-square distribution (Abramowitz & Stegun, table 26.8).  The
    approximation sharpens with the degrees of freedom; at 30 and a rate of 1e-3 it is 1.7e-3 high (59.80 for 59.703)."""
    from umhsnerf.statistics import chi_square_quantile

    for dof, rate, tabulated in ((100, 1e-3, 149.449), (50, 1e-3, 86.661), (100, 0.05, 124.342)):
        assert chi_square_quantile(dof, rate) == pytest.approx(tabulated, rel=1e-3), (dof, rate)
    assert chi_square_quantile(31, 1e-3) > chi_square_quantile(31, 1e-2) > 31
    with pytest.raises(ValueError):
        chi_square_quantile(0, 1e-3)
    with pytest.raises(ValueError):
        chi_square_quantile(31, 1.0)


def test_output_names():
    from umhsnerf import statistics as S

    assert S.STATISTICS_OUTPUTS == ("rx_score", "rx_mask", "pca_0", "pca_1", "pca_2", "pca_rgb")
    assert S.statistics_outputs(2) == ("rx_score", "rx_mask", "pca_0", "pca_1") and S.statistics_outputs(0) == ("rx_score", "rx_mask")
    assert all(S.is_statistics_output(n) for n in ("rx_score", "rx_mask", "pca_0", "pca_17", "pca_rgb"))
    assert not any(S.is_statistics_output(n) for n in ("rgb", "pca", "pca_x", "wv_3", "library_raw", "rx"))


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def test_parsers_accept_the_new_flags():
    from umhsnerf import eval as umhs_eval
    from umhsnerf import render, statistics

    flags = ["--scene-statistics", "stats.npz", "--pca-components", "5", "--rx-false-alarm", "1e-2", "--rx-floor", "1e-4"]
    common = MODEL + ["--output-path", "out"] + flags
    for argv in (["camera-path", "--camera-path-filename", "path.json"], ["dataset"], ["interpolate"]):
        args = render.parse_args(argv[:1] + common + argv[1:] + ["--rendered-output-names", "rgb", "pca_rgb", "rx_score", "pca_4"])
        assert (args.scene_statistics, args.pca_components, args.rx_false_alarm, args.rx_floor, args.rx_threshold) == ("stats.npz", 5, 1e-2, 1e-4, None)
    args = render.parse_args(["dataset"] + MODEL + ["--output-path", "out"])
    assert (args.scene_statistics, args.pca_components, args.rx_threshold, args.rx_false_alarm, args.rx_floor) == (None, 3, None, None, 1e-6)
    args = umhs_eval.build_parser().parse_args(MODEL + flags[:2] + ["--rx-threshold", "80"])
    assert args.scene_statistics == "stats.npz" and args.rx_threshold == 80.0
    assert statistics.threshold_from_args(args, 31) == 80.0
    args = umhs_eval.build_parser().parse_args(MODEL + flags)
    assert statistics.threshold_from_args(args, 31) == statistics.chi_square_quantile(31, 1e-2)
    args.rx_threshold = 3.0
    with pytest.raises(ValueError, match="one of them"):
        statistics.threshold_from_args(args, 31)
    args = statistics.build_parser().parse_args(["compute"] + MODEL + ["--source", "rendered", "--split", "train", "--output", "s.npz"])
    assert (args.command, args.source, args.split, args.output) == ("compute", "rendered", "train", "s.npz")
    assert statistics.build_parser().parse_args(["compute"] + MODEL + ["--output", "s.npz"]).source == "captured"


@pytest.mark.parametrize("name", ["rx_score", "rx_mask", "pca_0", "pca_rgb"])
def test_a_statistics_output_without_the_flag_names_the_flag(name):
    from umhsnerf import render

    with pytest.raises(ValueError, match="--scene-statistics"):
        render.parse_args(["dataset"] + MODEL + ["--output-path", "out", "--rendered-output-names", "rgb", name])
    with pytest.raises(ValueError, match="--scene-statistics"):
        render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + ["--output-path", "out", "--cube-output-names", name])


# ---- C ABI, host side only -------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(built_library):
    from umhsnerf import _hip, build

    with open(os.path.join(ROOT, "include", "umhs_hip.h")) as f:
        header = f.read()
    assert "Scene statistics" in header and "#define UMHS_GRAM_CHUNK 1024" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in _hip.SIGNATURES and f"{name}(" in header and f" T {name}\n" in exported, name
    assert "umhs_statistics.hip" in build.SOURCES
    assert _hip.ABI_VERSION == 11 == _hip.lib().umhs_abi_version()
    assert _hip.lib().umhs_gram_chunk() == 1024


def test_argument_rules_run_before_any_launch(built_library):
    from umhsnerf import _hip

    lib, d = _hip.lib(), ctypes.c_void_p(4096)
    ARG, UNSUPPORTED = -1, -2
    slot = lambda B: (1 + B + B * B) * 4
    assert lib.umhs_gram_workspace_bytes(1, 1) == slot(1) and lib.umhs_gram_workspace_bytes(1024, 31) == slot(31)
    assert lib.umhs_gram_workspace_bytes(1025, 31) == 2 * slot(31) and lib.umhs_gram_workspace_bytes(921600, 128) == 512 * slot(128)
    assert lib.umhs_gram_workspace_bytes(10 ** 12, 256) == 512 * slot(256)  # it stops growing
    assert lib.umhs_gram_workspace_bytes(0, 31) == 0 and lib.umhs_gram_workspace_bytes(5, 0) == 0 and lib.umhs_gram_workspace_bytes(5, 257) == 0
    gram = lambda **kw: lib.umhs_gram_accumulate(*[kw.get(k, v) for k, v in dict(
        spectra=d, stride=31, R=8, B=31, shift=d, accumulation=None, acc=d, workspace=d, nbytes=slot(31), stream=None).items()])
    for missing in ("spectra", "shift", "acc", "workspace"):
        assert gram(**{missing: None}) == ARG, missing
    assert gram(nbytes=slot(31) - 1) == ARG
    assert gram(B=0) == ARG and gram(R=-1) == ARG and gram(stride=30) == ARG
    assert gram(B=257, stride=257) == UNSUPPORTED
    assert gram(R=0) == 0 and gram(R=0, spectra=None, shift=None, acc=None, workspace=None, nbytes=0) == 0
    project = lambda **kw: lib.umhs_spectral_project(*[kw.get(k, v) for k, v in dict(
        spectra=d, stride=31, R=8, mean=d, image=d, K=31, B=31, P=3, components=d, score=d, stream=None).items()])
    for missing in ("spectra", "mean", "image", "components"):
        assert project(**{missing: None}) == ARG, missing
    assert project(B=0) == ARG and project(K=0) == ARG and project(R=-1) == ARG and project(stride=30) == ARG
    assert project(P=32) == ARG and project(P=-1) == ARG
    assert project(B=257, stride=257) == UNSUPPORTED and project(K=257) == UNSUPPORTED
    assert project(R=0) == 0 and project(R=0, spectra=None, mean=None, image=None, components=None, score=None) == 0


def test_ops_have_no_cpu_path_and_check_their_arguments():
    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gram_accumulate(torch.rand(8, 5), torch.zeros(5), torch.zeros(31, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.spectral_project(torch.rand(8, 5), torch.zeros(5), torch.zeros(64), 5, 3)
    with pytest.raises(ValueError, match="float32"):
        ops.gram_accumulate(torch.rand(8, 5).double(), torch.zeros(5), torch.zeros(31, dtype=torch.float64))
