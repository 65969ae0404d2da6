"""The comparators of tests/statistics_f64.py, on the CPU: they pass the float32 oracle, reject planted faults, K_G and K_Y are four
times what the oracle needs, and the cases meet the conditions their docstring states."""
import math

import pytest
import torch

import statistics_f64 as SF


@pytest.fixture(scope="module")
def gram_runs():
    """(case, float64 run, float32 oracle run) per gram case, computed once."""
    return {c: (*SF.gram_reference(*c), SF.gram_oracle(SF.gram_reference(*c)[0])) for c in SF.GRAM_CASES}


@pytest.fixture(scope="module")
def project_runs():
    return {c: (*SF.project_reference(*c), SF.project_oracle(SF.project_reference(*c)[0])) for c in SF.PROJECT_CASES}


def test_the_float32_oracle_passes_and_K_is_four_times_its_worst_ratio(gram_runs, project_runs):
    worst_g, worst_y, at_g, at_y = 0.0, 0.0, None, None
    for c, (case, r64, acc) in gram_runs.items():
        report = {}
        assert not SF.check_gram(case, acc, r64, report=report), SF.gram_id(c)
        print(SF.gram_id(c), {k: round(v, 2) for k, v in report.items()})
        if max(report.values()) > worst_g:
            worst_g, at_g = max(report.values()), SF.gram_id(c)
    for c, (case, r64, (y, score)) in project_runs.items():
        report = {}
        assert not SF.check_project(case, y, score, r64, report=report), SF.project_id(c)
        print(SF.project_id(c), {k: round(v, 3) for k, v in report.items()})
        if report["y"] > worst_y:
            worst_y, at_y = report["y"], SF.project_id(c)
    print(f"gram worst {worst_g:.3g} at {at_g}; y worst {worst_y:.3g} at {at_y}")
    for K, worst in ((SF.K_G, worst_g), (SF.K_Y, worst_y)):
        assert 4 * worst <= K and K == max(8.0, 2.0 ** math.ceil(math.log2(4 * worst)))


def test_two_calls_and_another_shift_pass_their_own_rule():
    case, r64 = SF.gram_reference(*SF.SPLIT_CASE)
    assert not SF.check_gram(case, SF.gram_oracle(case, splits=[SF.SPLIT_AT]), r64)
    zero = torch.zeros(case["B"])
    assert not SF.check_gram(case, SF.gram_oracle(case, shift=zero), SF.gram_ref64(case, zero))


def test_the_gram_comparator_rejects_planted_faults(gram_runs):
    c = SF.SPLIT_CASE
    case, r64, acc = gram_runs[c]
    B = case["B"]
    invalid = int((~case["valid"]).nonzero()[0])
    fails = SF.check_gram(case, SF.gram_oracle(case, count_invalid=invalid), r64)
    assert fails and "count" in fails[0]  # one invalid row counted
    assert any("gram" in f or "sums" in f for f in SF.check_gram(case, SF.gram_oracle(case, drop_chunk=1), r64))  # a partial dropped
    skew = acc.clone()
    G = skew[1 + B:].view(B, B)
    G[3, 7] = torch.nextafter(G[3, 7], torch.tensor(float("inf"), dtype=torch.float64))  # g[a,b] != g[b,a], by one float64 step
    assert any("symmetric" in f for f in SF.check_gram(case, skew, r64))
    assert SF.check_gram(case, acc.float(), r64)  # not float64


def test_the_projection_comparator_rejects_planted_faults(project_runs):
    c = (300, 31, 31, 3, 0.01)
    case, r64, (y, score) = project_runs[c]
    assert any(f.startswith("y") for f in SF.check_project(case, *SF.project_oracle(case, no_mean=True), r64))  # mean not subtracted
    moved = torch.roll(y, 1, 0)  # y of row r written to row r + 1
    assert SF.check_project(case, moved, score, r64)
    assert any(f.startswith("score") for f in SF.check_project(case, *SF.project_oracle(case, drop_last=True), r64))  # K - 1 components
    poisoned = score.clone()
    poisoned[~case["finite"]] = 1.0
    assert any("zeros" in f for f in SF.check_project(case, y, poisoned, r64))
    # the noise-free case is what it says: most of its eigenvalues sit on the floor (and a mean left out is still seen there)
    case, r64, _ = project_runs[(300, 31, 31, 3, 0.0)]
    assert int((case["lam"] <= SF.FLOOR * case["lam"][0] * (1 + 1e-12)).sum()) >= 20
    assert any(f.startswith("y") for f in SF.check_project(case, *SF.project_oracle(case, no_mean=True), r64))


def test_the_cases_meet_their_conditions(project_runs):
    for c in SF.E2E_CASES:
        got = SF.e2e_conditions(SF.e2e_reference(*c))
        print(c, got)
        assert got["margin"] >= 1.5 and 0.85 <= got["level"] <= 1.05, (c, got)
        assert int(SF.e2e_reference(*c)["planted"].sum()) == 5
    worst = 1.0
    for c, (case, r64, _) in project_runs.items():
        t = SF.teeth(case, r64)
        if t is not None:
            print(SF.project_id(c), "teeth", round(t, 4))
            worst = min(worst, t)
    assert worst >= SF.MIN_TEETH
    # every case with R >= 16 holds rows of each kind
    for c in SF.GRAM_CASES:
        case = SF.gram_reference(*c)[0]
        if c[0] >= 16:
            assert int((case["accumulation"] < 0.5).sum()) >= 2 and int((~case["finite"]).sum()) == 2 and int(case["valid"].sum()) > 0
