"""Spectral unmixing without a GPU: the float64 oracle of tests/unmix_f64.py against exact enumeration and scipy, the float32
restatement of the kernel against the comparator (the constants are re-measured here), planted faults, the conditioning guard, the flags
and the argument rules of the new C entry point (it returns before any launch)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import unmix_f64 as UF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--data", "scene", "--checkpoint", "model.ckpt"]
SYMBOLS = ("umhs_unmix_workspace_bytes", "umhs_unmix")
SMALL = [c for c in UF.CASES if c[1] <= 6 and c[3] > 0]


def _normal_equations(case):
    E64 = case["E"].astype(np.float64)
    return E64, E64 @ E64.T


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", UF.MODES, ids=["nnls", "fcls"])
@pytest.mark.parametrize("c", SMALL, ids=UF.unmix_id)
def test_the_float64_oracle_is_the_exact_optimum(c, mode):
    case, ref = UF.reference(*c, mode)
    E64, G = _normal_equations(case)
    rows = np.nonzero(case["valid"])[0][:80]
    for r in rows:
        b = E64 @ case["x"][r].astype(np.float64)
        assert np.abs(UF.brute_force(G, b, mode) - ref["a"][r]).max() <= 1e-10, r
    assert len(rows) > 0 and not (ref["status"] == -2).any()


@pytest.mark.parametrize("c", [c for c in UF.CASES if c[3] > 0], ids=UF.unmix_id)
def test_the_float64_oracle_in_nnls_mode_is_scipys(c):
    from scipy.optimize import nnls

    case, ref = UF.reference(*c, UF.NNLS)
    E64, _ = _normal_equations(case)
    for r in np.nonzero(case["valid"])[0][:60]:
        want, _ = nnls(E64.T, case["x"][r].astype(np.float64))
        assert np.abs(want - ref["a"][r]).max() <= 1e-9, r


# ---- the float32 restatement and the constants -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _measured(c, mode):
    """(fails, report) of the float32 restatement on one case, run once and shared."""
    case, ref = UF.reference(*c, mode)
    a, res, status = UF.solve_f32(case["E"], case["x"], mode)
    report = {}
    return tuple(UF.check(case, a, res, status, report)), report


@pytest.mark.parametrize("mode", UF.MODES, ids=["nnls", "fcls"])
@pytest.mark.parametrize("c", UF.CASES, ids=UF.unmix_id)
def test_the_float32_restatement_passes_the_comparator(c, mode):
    case, ref = UF.reference(*c, mode)
    assert not (ref["status"] == -2).any()  # the float64 oracle caps on no committed case
    fails, report = _measured(c, mode)
    print(UF.unmix_id(c), mode, {k: round(v, 4) for k, v in report.items()})
    assert not fails, fails
    assert report.get("cap_share", 0.0) <= UF.MAX_CAP_SHARE
    if case["kind"] == "syn":
        assert np.linalg.cond(case["E"].astype(np.float64)) <= UF.MAX_SYNTHETIC_COND


def test_the_constants_carry_four_times_the_measured_worst():
    """K = 4 x the worst raw ratio, rounded up to a power of two: so the worst ratio of its bound is in (1/8, 1/4]."""
    reports = [_measured(c, mode)[1] for c in UF.CASES for mode in UF.MODES]
    for key, K in (("sum", UF.K_S), ("objective", UF.K_F), ("abundance", UF.K_A), ("residual", UF.K_R)):
        worst = max(r[key] for r in reports) * K  # (the report holds ratios of the bound)
        print(key, "worst raw ratio", round(worst, 3), "K", K)
        assert 4.0 * worst <= K < 8.0 * worst, (key, worst, K)


def test_the_cases_cover_what_they_must():
    ids = [UF.unmix_id(c) for c in UF.CASES]
    assert len(set(ids)) == len(ids)
    assert {c[3] for c in UF.CASES} >= {0, 1, 63, 64, 65} and any(c[3] >= 1000 and c[4] == "slice" for c in UF.CASES)
    assert {c[1] for c in UF.CASES} >= {1, 2, 6, 15, 16} and {c[2] for c in UF.CASES} >= {2, 31, 33, 128, 141, 256}
    regimes = {min(nk for nk in (8, 16, 24, 32, 48, 64, 72, 96, 128) if nk >= (c[2] + 1) // 2) for c in UF.CASES}
    assert regimes == {8, 16, 24, 32, 48, 64, 72, 96, 128}  # every NK of LIB_DISPATCH
    assert {c[0] for c in UF.CASES} >= {"syn", "hotdog", "vca_b31", "vca_b128", "vca_b141"}
    case = UF.make_case(*UF.CASES[8])
    assert case["layout"] == "slice" and case["x"].strides[0] == 4 * (case["B"] + UF.SLICE_PAD) and not case["x"].flags["C_CONTIGUOUS"]
    x, valid = case["x"], case["valid"]
    assert (~valid).sum() >= 4 and np.isnan(x).any() and np.isinf(x).any() and (x == 0).all(1).any() and (np.abs(x) >= 1e30).any()
    hot = np.load(os.path.join(UF.GOLDEN, "g7_endmembers_hotdog.npy"))
    assert hot.shape == (4, 141) and hot.dtype == np.float32


def test_the_modes_differ_on_scaled_rows():
    case, nn = UF.reference(*UF.CASES[3], UF.NNLS)
    _, fc = UF.reference(*UF.CASES[3], UF.FCLS)
    v = case["valid"]
    assert np.abs(fc["a"][v].sum(1) - 1).max() < 1e-12 and np.abs(nn["a"][v].sum(1) - 1).max() > 0.2
    assert (fc["a"][v] == 0).any() and (nn["a"][v] == 0).any()  # constraints are active


# ---- planted faults --------------------------------------------------------------------------------------------------------------
FAULT_CASE = UF.CASES[3]  # syn-K6-B33-R65
SOLVER_FAULT_CASE = UF.CASES[5]  # syn-K15-B50-R129: rows whose optimum needs an endmember back that the first pass dropped, in both modes


def _good(mode):
    case, ref = UF.reference(*FAULT_CASE, mode)
    a, res, status = UF.solve_f32(case["E"], case["x"], mode)
    assert not UF.check(case, a, res, status)
    return case, a.copy(), res.copy(), status.copy()


@pytest.mark.parametrize("fault", ["clip", "no_multiplier", "lambda_sign"])
def test_check_rejects_a_faulty_solver(fault):
    for mode in (UF.MODES if fault != "lambda_sign" else (UF.FCLS,)):
        case, _ = UF.reference(*SOLVER_FAULT_CASE, mode)
        a, res, status = UF.solve_f32(case["E"], case["x"], mode, fault=fault)
        assert UF.check(case, a, res, status), (fault, mode)


def test_check_rejects_a_dropped_sum_constraint():
    case, _ = UF.reference(*FAULT_CASE, UF.FCLS)
    a, res, status = UF.solve_f32(case["E"], case["x"], UF.NNLS)
    assert any("sum" in f for f in UF.check(case, a, res, status))


def test_check_rejects_swapped_endmembers_a_wrong_residual_and_a_stale_row():
    for mode in UF.MODES:
        case, a, res, status = _good(mode)
        swapped = a.copy()
        swapped[:, [0, 1]] = swapped[:, [1, 0]]
        assert UF.check(case, swapped, res, status)
        E64, x64 = case["E"].astype(np.float64), np.where(case["valid"][:, None], case["x"], 0).astype(np.float64)
        G = E64 @ E64.T
        no_cross = ((x64 * x64).sum(1) + np.einsum("rk,kl,rl->r", a, G, a)).astype(np.float32) * case["valid"]
        assert any("residual" in f for f in UF.check(case, a, no_cross, status))
        stale = a.copy()
        r = int(np.nonzero(case["valid"])[0][5])
        stale[r] = a[r - 1]
        assert UF.check(case, stale, res, status)
        negative = a.copy()
        negative[r, 0] = -1e-6
        assert UF.check(case, negative, res, status)
        alive = a.copy()
        dead = int(np.nonzero(~case["valid"])[0][0])
        alive[dead, 0] = 0.5
        assert UF.check(case, alive, res, status)
        capped = status.copy()
        capped[case["valid"]] = -2
        assert any("cap" in f for f in UF.check(case, a, res, capped))


# ---- the conditioning guard and the unmixer --------------------------------------------------------------------------------------
def test_the_guard_refuses_a_near_duplicate_pair_and_names_it():
    from umhsnerf import unmix

    assert unmix.ABUNDANCE_BOUND == UF.K_A * UF.U and unmix.MAX_ABUNDANCE_ERROR == 0.01
    E = UF.synthetic_endmembers(6, 31).astype(np.float64)
    names = [f"m{k}" for k in range(6)]
    good = unmix.Unmixer(E, names)
    assert len(good) == 6 and good.bands == 31 and good.mode == 1 and good.gram.dtype == np.float32
    assert np.array_equal(good.gram, UF.gram32(E.astype(np.float32)))
    assert unmix.Unmixer(E, names, constraint="nnls").mode == 0
    near = E.copy()
    near[4] = 0.999 * E[1] + 0.001 * E[2]
    with pytest.raises(ValueError, match=r"cond_2.*'m1' and 'm4'"):
        unmix.Unmixer(near, names)
    with pytest.raises(ValueError, match="'m0' and 'm3'"):  # an exact duplicate: the same rule
        unmix.Unmixer(np.concatenate([E[:3], E[:1]]), names[:4])
    assert len(unmix.Unmixer(E[:1], ["only"])) == 1  # K = 1: cond = 1
    with pytest.raises(ValueError, match="1..16"):
        unmix.Unmixer(np.random.default_rng(0).uniform(size=(17, 40)))
    with pytest.raises(ValueError, match="constraint"):
        unmix.Unmixer(E, names, constraint="lasso")
    # the recorded hotdog endmembers pass; the 9 VCA endmembers on 128 bands (cond_2(E) = 230) do not
    unmix.Unmixer(UF.endmembers("hotdog", 4, 141))
    with pytest.raises(ValueError, match="too close to dependent"):
        unmix.Unmixer(UF.endmembers("vca_b128", 9, 128))


def test_an_unmixer_from_library_entries():
    from umhsnerf import unmix
    from umhsnerf.library import SpectralLibrary

    wl = [400.0 + 10 * i for i in range(31)]
    lib = SpectralLibrary([f"e{k}" for k in range(20)], UF.synthetic_endmembers(20, 31).astype(np.float64) + 0.0, wl)
    u = unmix.Unmixer.from_library(lib, ["e3", "e11", 17])
    assert u.names == ["e3", "e11", "e17"] and np.array_equal(u.endmembers, lib.spectra[[3, 11, 17]].astype(np.float32))
    assert np.array_equal(u.colors, lib.colors[[3, 11, 17]])
    with pytest.raises(ValueError, match="no entry named"):
        unmix.Unmixer.from_library(lib, ["e3", "nothing"])
    with pytest.raises(ValueError, match="1..16"):
        unmix.Unmixer.from_library(lib, list(range(17)))
    with pytest.raises(ValueError, match="twice"):
        unmix.Unmixer.from_library(lib, ["e3", 3])


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def test_parsers_accept_the_new_flags_and_refuse_what_they_must():
    from umhsnerf import eval as umhs_eval
    from umhsnerf import render, unmix

    out = ["--output-path", "out"]
    for argv in (["camera-path", "--camera-path-filename", "path.json"], ["dataset"], ["interpolate"]):
        args = render.parse_args(argv[:1] + MODEL + out + argv[1:] + ["--unmix", "model", "--unmix-constraint", "nnls",
                                                                       "--rendered-output-names", "rgb", "unmix_0", "unmix_pred", "unmix_residual"])
        assert (args.unmix, args.unmix_constraint, args.unmix_entries) == ("model", "nnls", None)
    args = render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + [
        "--unmix", "library", "--spectral-library", "lib.npz", "--unmix-entries", "grass", "soil", "--cube-output-names", "unmix"])
    assert (args.unmix, args.unmix_entries, args.unmix_constraint) == ("library", ["grass", "soil"], "fcls")
    assert render.parse_args(["dataset"] + MODEL + out).unmix is None
    for name in ("unmix", "unmix_0", "unmix_raw", "unmix_pred", "unmix_residual"):
        with pytest.raises(ValueError, match="--unmix"):
            render.parse_args(["dataset"] + MODEL + out + ["--rendered-output-names", "rgb", name])
    with pytest.raises(ValueError, match="--unmix"):
        render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + ["--cube-output-names", "unmix"])
    with pytest.raises(ValueError, match="--spectral-library"):
        render.parse_args(["dataset"] + MODEL + out + ["--unmix", "library", "--unmix-entries", "grass"])
    with pytest.raises(ValueError, match="--unmix-entries"):
        render.parse_args(["dataset"] + MODEL + out + ["--unmix", "library", "--spectral-library", "lib.npz"])
    with pytest.raises(ValueError, match="at most 16"):
        render.parse_args(["dataset"] + MODEL + out + ["--unmix", "library", "--spectral-library", "lib.npz", "--unmix-entries"]
                          + [f"e{i}" for i in range(17)])
    with pytest.raises(ValueError, match="goes with"):
        render.parse_args(["dataset"] + MODEL + out + ["--unmix", "model", "--unmix-entries", "grass"])
    args = umhs_eval.build_parser().parse_args(MODEL + ["--unmix", "model"])
    assert args.unmix == "model" and args.unmix_constraint == "fcls"
    assert umhs_eval.build_parser().parse_args(MODEL).unmix is None
    args = unmix.build_parser().parse_args(["captured"] + MODEL + out + ["--split", "val"])
    assert (args.command, args.unmix, args.split, args.output_path) == ("captured", "model", "val", "out")
    assert unmix.unmix_outputs(2) == ("unmix_0", "unmix_1", "unmix", "unmix_raw", "unmix_pred", "unmix_residual")
    assert not unmix.is_unmix_output("unmix_x") and not unmix.is_unmix_output("abundances_0") and unmix.unmix_index("unmix_12") == 12


# ---- C ABI, host side only -------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(built_library):
    from umhsnerf import _hip, build, ops

    with open(os.path.join(ROOT, "include", "umhs_hip.h")) as f:
        header = f.read()
    assert "Spectral unmixing" in header and "#define UMHS_UNMIX_MAX_ENDMEMBERS 16" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in _hip.SIGNATURES and f"{name}(" in header and f" T {name}\n" in exported, name
    assert "umhs_unmix.hip" in build.SOURCES
    assert _hip.ABI_VERSION == 11 == _hip.lib().umhs_abi_version()
    assert (ops.UNMIX_NNLS, ops.UNMIX_FCLS, ops.UNMIX_MAX_ENDMEMBERS, ops.UNMIX_MAX_BANDS) == (0, 1, 16, 256) and callable(ops.unmix)


def test_argument_rules_run_before_any_launch(built_library):
    from umhsnerf import _hip

    lib, d = _hip.lib(), ctypes.c_void_p(4096)
    ARG, UNSUPPORTED = -1, -2
    assert lib.umhs_unmix_workspace_bytes(921600, 16, 256) == 0 and lib.umhs_unmix_workspace_bytes(0, 1, 1) == 0
    unmix = lambda **kw: lib.umhs_unmix(*[kw.get(k, v) for k, v in dict(
        spectra=d, stride=31, R=8, image=d, gram=d, K=6, B=31, mode=1, abundances=d, residual=d, status=d, workspace=None, nbytes=0,
        stream=None).items()])
    for missing in ("spectra", "image", "gram", "abundances"):
        assert unmix(**{missing: None}) == ARG, missing
    assert unmix(B=0) == ARG and unmix(K=0) == ARG and unmix(R=-1) == ARG and unmix(stride=30) == ARG
    assert unmix(mode=2) == ARG and unmix(mode=-1) == ARG
    assert unmix(B=257, stride=257) == UNSUPPORTED and unmix(K=17) == UNSUPPORTED
    assert unmix(K=17, mode=2) == ARG and unmix(B=257, stride=256) == ARG  # bad sizes or mode come first
    assert unmix(K=17, spectra=None) == UNSUPPORTED and unmix(K=17, R=0) == UNSUPPORTED  # then the limits
    assert unmix(R=0) == 0 and unmix(R=0, spectra=None, image=None, gram=None, abundances=None, residual=None, status=None) == 0


def test_the_op_has_no_cpu_path_and_checks_its_arguments():
    import torch

    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.unmix(torch.rand(8, 5), torch.zeros(64 * 3), torch.eye(3), 3, ops.UNMIX_FCLS)
    with pytest.raises(ValueError, match="float32"):
        ops.unmix(torch.rand(8, 5).double(), torch.zeros(64 * 3), torch.eye(3), 3, ops.UNMIX_FCLS)
