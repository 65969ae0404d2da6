"""Sparse unmixing without a GPU: the float64 truth of tests/sparse_f64.py against exact enumeration and its own KKT conditions, the
float32 restatement of the kernel's iteration against the comparator (the constants are re-measured here), planted faults, the mu
rule, the flags and refusals of umhsnerf/sparse.py and the argument rules of the new C entry points (they return before any launch)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import sparse_f64 as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--data", "scene", "--checkpoint", "model.ckpt"]
SYMBOLS = ("umhs_sparse_image_bytes", "umhs_sparse_prepare", "umhs_sparse_unmix")
RUN = [c for c in SF.CASES if c[3] > 0]
SMALL = [c for c in RUN if c[1] <= 6]


# ---- the truth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SMALL, ids=SF.sparse_id)
def test_the_float64_truth_is_the_exact_optimum(c):
    case, ref = SF.reference(*c)
    A64 = case["A"].astype(np.float64)
    G = A64 @ A64.T
    rows = np.nonzero(case["valid"])[0][:80]
    for r in rows:
        x64 = case["x"][r].astype(np.float64)
        b = A64 @ x64 - case["lam"] * np.sqrt(x64 @ x64)
        assert np.abs(SF.brute_force(G, b) - ref["a"][r]).max() <= 1e-10 * max(1.0, np.abs(ref["a"][r]).max()), r
    assert len(rows) > 0


@pytest.mark.parametrize("c", RUN, ids=SF.sparse_id)
def test_the_float64_truth_meets_its_kkt_conditions(c):
    case, ref = SF.reference(*c)
    v = case["valid"]
    assert not (ref["status"] == -2).any()  # the active-set run stops at its cap on no committed case
    assert SF.kkt_violation(case["A"], case["x"][v], ref["a"][v], case["lam"]).max() <= 1e-12
    assert (ref["a"][v] >= 0).all() and ((ref["a"][v] > 0).sum(1) < max(2, case["L"])).any()  # and the penalty does make it sparse


def test_the_penalty_scales_with_the_row():
    """lambda_r = lambda sqrt(ss): a row scaled by 1000 has 1000 times the abundances, on the same support."""
    case = SF.make_case(*SF.CASES[5])
    x = case["x"][:4].astype(np.float64)
    x32, big = x.astype(np.float32), (x.astype(np.float32) * np.float32(1024))
    a, _, _ = SF.solve_f64(case["A"], x32)
    b, _, _ = SF.solve_f64(case["A"], big)
    assert np.array_equal(a > 0, b > 0) and np.abs(b - 1024 * a).max() <= 1e-9 * 1024


# ---- the float32 restatement and the constants -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _measured(c):
    """(fails, report) of the float32 restatement on one case, run once and shared."""
    case, ref = SF.reference(*c)
    a, res, status = SF.solve_f32(case["A"], case["x"])
    report = {}
    return tuple(SF.check(case, a, res, status, report)), report


@pytest.mark.parametrize("c", SF.CASES, ids=SF.sparse_id)
def test_the_float32_restatement_passes_the_comparator_within_the_cap_share(c):
    case, _ = SF.reference(*c)
    fails, report = _measured(c)
    print(SF.sparse_id(c), {k: round(v, 4) for k, v in report.items()})
    assert not fails, fails
    assert report.get("cap_share", 0.0) <= SF.MAX_CAP_SHARE
    if case["kind"] == "syn":
        assert np.linalg.cond(case["A"].astype(np.float64)) <= SF.MAX_SYNTHETIC_COND


def test_the_constants_carry_four_times_the_measured_worst():
    """K = 4 x the worst raw ratio, rounded up to a power of two: so the worst ratio of its bound is in (1/8, 1/4]."""
    reports = [_measured(c)[1] for c in RUN]
    for key, K in (("objective", SF.K_F), ("abundance", SF.K_A), ("residual", SF.K_R)):
        worst = max(r[key] for r in reports) * K  # (the report holds ratios of the bound)
        print(key, "worst raw ratio", round(worst, 4), "K", K)
        assert 4.0 * worst <= K < 8.0 * worst, (key, worst, K)
        assert np.log2(K) == round(np.log2(K))


def test_the_float64_iteration_shows_that_the_tolerance_not_float32_sets_the_error():
    """``solve_admm_f64`` passes the same comparator, and on the worst abundance case its ratio is the float32 one to 2 %: what is
    measured is the stopping rule's epsilon."""
    c = SF.CASES[9]
    case, _ = SF.reference(*c)
    a, res, status = SF.solve_admm_f64(case["A"], case["x"])
    report = {}
    assert not SF.check(case, a, res, status, report)
    assert abs(report["abundance"] - _measured(c)[1]["abundance"]) <= 0.02 * report["abundance"]


def test_the_cases_cover_what_they_must():
    ids = [SF.sparse_id(c) for c in SF.CASES]
    assert len(set(ids)) == len(ids) and len(ids) <= 16
    assert {c[1] for c in SF.CASES} >= {1, 2, 31, 32, 33, 64, 65, 96, 128}
    assert {c[2] for c in SF.CASES} >= {2, 31, 33, 128, 141, 256}
    assert {c[3] for c in SF.CASES} >= {0, 1, 31, 32, 33, 63, 65, 129, 257}
    assert {c[0] for c in SF.CASES} >= {"syn", "hotdog", "vca_b31", "vca_b128", "vca_b141"}
    assert {(c[1] + 31) // 32 for c in SF.CASES} == {1, 2, 3, 4}  # every specialisation of the kernel
    case = SF.make_case(*SF.CASES[9])
    assert case["layout"] == "slice" and case["x"].strides[0] == 4 * (case["B"] + SF.SLICE_PAD) and not case["x"].flags["C_CONTIGUOUS"]
    x, valid = case["x"], case["valid"]
    assert (~valid).sum() >= 4 and np.isnan(x).any() and np.isinf(x).any() and (x == 0).all(1).any() and (np.abs(x) >= 1e30).any()
    norms = np.sqrt((x[valid].astype(np.float64) ** 2).sum(1))
    assert norms.max() / norms.min() > 1e5  # the rows scaled by 1e-3 and by 1e3
    order = SF.chain_order(128)
    assert sorted(order) == list(range(128)) and list(order[:10]) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12]
    assert list(SF.chain_order(6)) == [0, 4, 1, 5, 2, 3]


# ---- planted faults --------------------------------------------------------------------------------------------------------------
FAULT_CASE = SF.CASES[3]  # syn-L32-B33-R33


def _good():
    case, _ = SF.reference(*FAULT_CASE)
    a, res, status = SF.solve_f32(case["A"], case["x"])
    assert not SF.check(case, a, res, status)
    return case, a.copy(), res.copy(), status.copy()


def test_check_rejects_a_missing_threshold():
    """At lambda = 0.05, where the threshold moves the optimum by more than the stopping rule leaves."""
    case = dict(SF.make_case(*FAULT_CASE), lam=0.05)
    ref = SF.truth(case)
    a, res, status = SF.solve_f32(case["A"], case["x"], lam=0.05)
    assert not SF.check(case, a, res, status, ref=ref)
    a, res, status = SF.solve_f32(case["A"], case["x"], lam=0.05, fault="no_threshold")
    fails = SF.check(case, a, res, status, ref=ref)
    assert any("objective" in f for f in fails), fails


def test_a_row_that_keeps_iterating_after_it_is_done_is_caught():
    case, _ = SF.reference(*FAULT_CASE)
    assert not SF.rows_are_independent(lambda A, x: SF.solve_f32(A, x), case)
    assert SF.rows_are_independent(lambda A, x: SF.solve_f32(A, x, fault="no_freeze"), case)


def test_check_rejects_a_negative_zero_and_other_wrong_outputs():
    case, a, res, status = _good()
    a0, res0, status0 = SF.solve_f32(case["A"], case["x"], fault="minus_zero")
    assert np.array_equal(a0, a) and SF.check(case, a0, res0, status0)  # equal as numbers, refused for the sign bit
    swapped = a.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    assert SF.check(case, swapped, res, status)
    assert any("residual" in f for f in SF.check(case, a, (res * np.float32(1.01) + np.float32(1e-3) * case["valid"]).astype(np.float32), status))
    r = int(np.nonzero(case["valid"])[0][5])
    negative = a.copy()
    negative[r, 0] = -1e-6
    assert SF.check(case, negative, res, status)
    alive = a.copy()
    alive[int(np.nonzero(~case["valid"])[0][0]), 0] = 0.5
    assert SF.check(case, alive, res, status)
    capped = status.copy()
    capped[case["valid"]] = -2
    assert any("cap" in f for f in SF.check(case, a, res, capped))
    zero = status.copy()
    zero[r] = 0
    assert any("status" in f for f in SF.check(case, a, res, zero))


# ---- the mu rule -----------------------------------------------------------------------------------------------------------------
def test_the_mu_rule_takes_the_rho_of_fewest_iterations():
    from umhsnerf.ops import sparse as ops_sparse

    table = SF.mu_table()
    print({rho: round(n, 1) for rho, n in table.items()})
    assert tuple(table) == SF.RHOS == (0.01, 0.03, 0.1, 0.3, 1.0)
    assert min(table, key=table.get) == SF.RHO == ops_sparse.SPARSE_RHO
    A = SF.library("syn", 31, 31)
    assert ops_sparse.sparse_auto_mu(A) == SF.auto_mu(A) == pytest.approx(0.1 * (A.astype(np.float64) ** 2).sum() / 31)


# ---- C ABI, host side only -------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(built_library):
    from umhsnerf import _hip, build, ops

    with open(os.path.join(ROOT, "include", "umhs_hip.h")) as f:
        header = f.read()
    assert "Sparse unmixing" in header and "#define UMHS_SPARSE_MAX_ENTRIES 128" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in _hip.SIGNATURES and f"{name}(" in header and f" T {name}\n" in exported, name
    assert "umhs_sparse.hip" in build.SOURCES
    assert _hip.ABI_VERSION == 11 == _hip.lib().umhs_abi_version()
    assert (ops.SPARSE_MAX_ENTRIES, ops.SPARSE_MAX_BANDS) == (SF.MAX_ENTRIES, SF.MAX_BANDS) == (128, 256)
    assert callable(ops.sparse_prepare) and callable(ops.sparse_unmix)


def test_argument_rules_run_before_any_launch(built_library):
    from umhsnerf import _hip

    lib, d = _hip.lib(), ctypes.c_void_p(4096)
    ARG, UNSUPPORTED = -1, -2
    assert [lib.umhs_sparse_image_bytes(L) for L in (0, 1, 32, 33, 96, 97, 128, 129)] == [0, 4096, 4096, 16384, 36864, 65536, 65536, 0]
    assert lib.umhs_sparse_prepare(d, 0, d, None) == ARG and lib.umhs_sparse_prepare(d, 129, d, None) == UNSUPPORTED
    assert lib.umhs_sparse_prepare(None, 8, d, None) == ARG and lib.umhs_sparse_prepare(d, 8, None, None) == ARG
    sparse = lambda **kw: lib.umhs_sparse_unmix(*[kw.get(k, v) for k, v in dict(
        spectra=d, stride=31, R=8, q=d, m=d, a=d, g=d, L=40, B=31, theta=0.1, epsilon=1e-4, iterations=100, abundances=d, residual=d,
        status=d, stream=None).items()])
    for missing in ("spectra", "q", "m", "a", "g"):
        assert sparse(**{missing: None}) == ARG, missing
    assert sparse(B=0) == ARG and sparse(L=0) == ARG and sparse(R=-1) == ARG and sparse(stride=30) == ARG
    assert sparse(iterations=0) == ARG and sparse(epsilon=0.0) == ARG and sparse(epsilon=float("nan")) == ARG
    assert sparse(theta=-1.0) == ARG and sparse(theta=float("nan")) == ARG
    assert sparse(B=257, stride=257) == UNSUPPORTED and sparse(L=129) == UNSUPPORTED
    assert sparse(L=129, iterations=0) == ARG and sparse(B=257, stride=256) == ARG  # bad sizes or scalars come first
    assert sparse(L=129, spectra=None) == UNSUPPORTED and sparse(L=129, R=0) == UNSUPPORTED  # then the limits
    assert sparse(R=0) == 0 and sparse(R=0, spectra=None, q=None, m=None, a=None, g=None, abundances=None, residual=None, status=None) == 0


def test_the_op_has_no_cpu_path_and_checks_its_arguments():
    import torch

    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sparse_prepare(torch.rand(8, 5), 1e-3, 0.1)
    with pytest.raises(ValueError, match="float32"):
        ops.sparse_prepare(torch.rand(8, 5).double(), 1e-3, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sparse_unmix(torch.rand(8, 5), None)


# ---- the unmixer and the flags -----------------------------------------------------------------------------------------------------
def _library(L=20, B=31):
    from umhsnerf.library import SpectralLibrary

    wl = [400.0 + 10 * i for i in range(B)]
    return SpectralLibrary([f"e{k}" for k in range(L)], np.random.default_rng(L).uniform(0.05, 1.0, (L, B)), wl)


def test_a_sparse_unmixer_from_a_library_and_its_refusals():
    from umhsnerf import sparse

    lib = _library()
    u = sparse.SparseUnmixer(lib)
    assert len(u) == 20 and u.bands == 31 and u.names == lib.names and u.spectra.dtype == np.float32
    assert (u.lambda_, u.epsilon, u.max_iterations, u.mu_rule) == (1e-3, 1e-4, 400, "auto") and u.mu == SF.auto_mu(u.spectra)
    assert (sparse.DEFAULT_LAMBDA, sparse.DEFAULT_EPSILON, sparse.DEFAULT_MAX_ITERATIONS) == (SF.LAMBDA, SF.EPSILON, SF.MAX_ITERATIONS)
    assert u.summary() == {"entries": 20, "lambda": 1e-3, "epsilon": 1e-4, "max_iterations": 400, "mu": u.mu, "mu_rule": "auto"}
    sub = sparse.SparseUnmixer(lib, ["e3", "e11", 17], mu=0.5)
    assert sub.names == ["e3", "e11", "e17"] and np.array_equal(sub.spectra, lib.spectra[[3, 11, 17]].astype(np.float32))
    assert np.array_equal(sub.colors, lib.colors[[3, 11, 17]]) and (sub.mu, sub.mu_rule) == (0.5, "given")
    with pytest.raises(ValueError, match="no entry named"):
        sparse.SparseUnmixer(lib, ["e3", "nothing"])
    with pytest.raises(ValueError, match="twice"):
        sparse.SparseUnmixer(lib, ["e3", 3])
    with pytest.raises(ValueError, match="outside 0..19"):
        sparse.SparseUnmixer(lib, [20])
    with pytest.raises(ValueError, match=r"129 library entries.*1\.\.128.*--sparse-entries"):
        sparse.SparseUnmixer(_library(129))
    assert len(sparse.SparseUnmixer(_library(129), list(range(1, 129)))) == 128
    with pytest.raises(ValueError, match=r"1\.\.128"):
        sparse.SparseUnmixer(lib, [])
    for kw, flag in ((dict(lambda_=-1.0), "--sparse-lambda"), (dict(epsilon=0.0), "--sparse-epsilon"), (dict(max_iterations=0), "--sparse-max-iterations"),
                     (dict(mu=0.0), "--sparse-mu"), (dict(mu=float("nan")), "--sparse-mu")):
        with pytest.raises(ValueError, match=flag):
            sparse.SparseUnmixer(lib, **kw)


def test_parsers_accept_the_new_flags_and_refuse_what_they_must():
    from umhsnerf import eval as umhs_eval
    from umhsnerf import render, sparse

    out = ["--output-path", "out"]
    on = ["--sparse-unmix", "--spectral-library", "lib.npz"]
    for argv in (["camera-path", "--camera-path-filename", "path.json"], ["dataset"], ["interpolate"]):
        args = render.parse_args(argv[:1] + MODEL + out + argv[1:] + on + ["--sparse-lambda", "0.01", "--sparse-mu", "0.5", "--rendered-output-names",
                                                                           "rgb", "sparse_0", "sparse_pred", "sparse_count", "sparse_residual"])
        assert (args.sparse_unmix, args.sparse_lambda, args.sparse_mu, args.sparse_entries) == (True, 0.01, 0.5, None)
        assert (args.sparse_epsilon, args.sparse_max_iterations) == (1e-4, 400)
    args = render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + on + [
        "--sparse-entries", "grass", "soil", "--cube-output-names", "sparse"])
    assert (args.sparse_entries, args.sparse_mu, args.sparse_lambda) == (["grass", "soil"], "auto", 1e-3)
    assert render.parse_args(["dataset"] + MODEL + out).sparse_unmix is False
    for name in ("sparse", "sparse_0", "sparse_raw", "sparse_pred", "sparse_count", "sparse_residual"):
        with pytest.raises(ValueError, match="--sparse-unmix"):
            render.parse_args(["dataset"] + MODEL + out + ["--rendered-output-names", "rgb", name])
    with pytest.raises(ValueError, match="--sparse-unmix"):
        render.parse_args(["camera-path", "--camera-path-filename", "p.json"] + MODEL + out + ["--cube-output-names", "sparse"])
    with pytest.raises(ValueError, match="--spectral-library"):
        render.parse_args(["dataset"] + MODEL + out + ["--sparse-unmix"])
    with pytest.raises(ValueError, match="at most 128"):
        render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-entries"] + [f"e{i}" for i in range(129)])
    with pytest.raises(ValueError, match="goes with"):
        render.parse_args(["dataset"] + MODEL + out + ["--sparse-entries", "grass"])
    with pytest.raises(ValueError, match="--sparse-lambda"):
        render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-lambda", "-1"])
    with pytest.raises(ValueError, match="--sparse-epsilon"):
        render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-epsilon", "0"])
    with pytest.raises(ValueError, match="--sparse-max-iterations"):
        render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-max-iterations", "0"])
    with pytest.raises(SystemExit):
        render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-mu", "fast"])
    with pytest.raises(SystemExit):
        render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-mu", "0"])
    args = umhs_eval.build_parser().parse_args(MODEL + on)
    assert args.sparse_unmix and args.sparse_mu == "auto"
    assert umhs_eval.build_parser().parse_args(MODEL).sparse_unmix is False
    args = sparse.build_parser().parse_args(["captured"] + MODEL + out + ["--spectral-library", "lib.npz", "--split", "val"])
    assert (args.command, args.sparse_unmix, args.split, args.output_path) == ("captured", True, "val", "out")
    with pytest.raises(ValueError, match="--spectral-library"):
        sparse.check_sparse_arguments(sparse.build_parser().parse_args(["captured"] + MODEL + out))
    assert sparse.sparse_outputs(2) == ("sparse_0", "sparse_1", "sparse", "sparse_raw", "sparse_pred", "sparse_count", "sparse_residual")
    assert not sparse.is_sparse_output("sparse_x") and not sparse.is_sparse_output("unmix_0") and sparse.sparse_index("sparse_12") == 12
    assert sparse.sparse_unmixer_from_args(render.parse_args(["dataset"] + MODEL + out), None) is None
    u = sparse.sparse_unmixer_from_args(render.parse_args(["dataset"] + MODEL + out + on + ["--sparse-entries", "e1", "e2", "--sparse-mu", "2"]), _library())
    assert u.names == ["e1", "e2"] and u.mu == 2.0
