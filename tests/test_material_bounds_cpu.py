"""CPU checks of the material-edit comparators (tests/material_f64.py): the float32 oracle passes them, K is re-measured, the teeth
condition holds on the float64 run alone, and the planted faults are rejected."""
import math

import pytest
import torch

import material_f64 as MF

SIGMA_CASES = [(n, C) for n in MF.SIGMA_NS for C in MF.SIGMA_CS]


def _k_for(worst: float) -> float:
    return max(8.0, 2.0 ** math.ceil(math.log2(4.0 * worst))) if worst > 0 else 8.0


def test_float32_oracle_passes_remix_and_k_is_what_the_rule_gives():
    worst = {}
    for c in MF.REMIX_CASES:
        case = MF.make_remix_case(*c)
        report = {}
        fails = MF.check_remix(case, MF.remix_oracle(case, torch.float32), MF.remix_oracle(case, torch.float64), report)
        assert not fails, (MF.remix_id(c), fails)
        for k, v in report.items():
            worst[k] = max(worst.get(k, 0.0), v["worst"])
    print({k: round(v, 3) for k, v in worst.items()})
    assert set(worst) == {"spectral", "spectral2", "specular"}
    assert 4.0 * max(worst.values()) <= MF.K_REMIX == _k_for(max(worst.values()))


def test_float32_oracle_passes_sigma_and_k_is_what_the_rule_gives():
    worst = 0.0
    for n, C in SIGMA_CASES:
        case = MF.make_sigma_case(n, C)
        report = {}
        fails = MF.check_sigma(case, MF.sigma_oracle(case, torch.float32), MF.sigma_oracle(case, torch.float64), report)
        assert not fails, (n, C, fails)
        worst = max(worst, report["sigma"]["worst"])
    print(round(worst, 3))
    assert 4.0 * worst <= MF.K_SIGMA == _k_for(worst)


def test_teeth_on_the_float64_run_alone():
    for c in MF.REMIX_CASES:
        case = MF.make_remix_case(*c)
        r64, report = MF.remix_oracle(case, torch.float64), {}
        assert not MF.check_remix(case, r64, r64, report)
        assert not MF.teeth_failures(report), (MF.remix_id(c), report)
        if c[0] >= 5:
            assert 2 <= int(case["empty"].sum()) < c[0] and bool(torch.isnan(case["mix"][:, c[2]:]).all())
    for n, C in SIGMA_CASES:
        case = MF.make_sigma_case(n, C)
        r64, report = MF.sigma_oracle(case, torch.float64), {}
        assert not MF.check_sigma(case, r64, r64, report)
        assert not MF.teeth_failures(report), (n, C, report)
        if C > 1:
            assert {0.0, 1.0, 2.5} == set(case["gain"].tolist())


@pytest.mark.parametrize("c", [c for c in MF.REMIX_CASES if c[0] >= 5], ids=MF.remix_id)
def test_planted_a_class_dropped_from_the_sum(c):
    case = MF.make_remix_case(*c)
    r64 = MF.remix_oracle(case, torch.float64)
    for drop in (0, c[2] - 1):
        assert MF.check_remix(case, MF.remix_oracle(case, torch.float32, drop_class=drop), r64), drop


@pytest.mark.parametrize("c", [c for c in MF.REMIX_CASES if c[0] >= 5], ids=MF.remix_id)
def test_planted_the_gain_applied_twice(c):
    """E'' = g E' is what the kernel is handed; a render that multiplied by g once more mixes g^2 E'."""
    case = MF.make_remix_case(*c)
    g = torch.ones(c[2])
    g[c[2] // 2] = 0.5
    once = case["E"] * g[:, None]
    edited = dict(case, E=once)
    r64 = MF.remix_oracle(edited, torch.float64)
    assert not MF.check_remix(edited, MF.remix_oracle(edited, torch.float32), r64)
    assert MF.check_remix(edited, MF.remix_oracle(edited, torch.float32, E=once * g[:, None]), r64)


@pytest.mark.parametrize("C", MF.SIGMA_CS)
def test_planted_the_clamp_missing_with_all_zero_gains(C):
    """Rows that sum to 1 + 2^-23 in float32: without the clamp the density is -2^-23 sigma -- inside the rule's envelope, so it is the
    comparator's sign check that has to reject it."""
    n = 257
    case = MF.make_sigma_case(n, C, gains=[0.0] * C)
    case["a"] = MF.rows_summing_above_one(n, C)
    case["sigma"] = case["sigma"].clamp(min=1e-3)
    r64 = MF.sigma_oracle(case, torch.float64)
    assert bool((r64 == 0).all())
    good, bad = MF.sigma_oracle(case, torch.float32), MF.sigma_oracle(case, torch.float32, clamp=False)
    assert bool((good == 0).all()) and not MF.check_sigma(case, good, r64)
    assert bool((bad < 0).all())
    fails = MF.check_sigma(case, bad, r64)
    assert fails and "negative" in fails[-1]


def test_planted_a_class_dropped_from_the_density_factor():
    for C in (3, 15):
        case = MF.make_sigma_case(1000, C)
        r64 = MF.sigma_oracle(case, torch.float64)
        short = dict(case, a=case["a"].clone())
        short["a"][:, 0] = 0.0  # class 0 has gain 0: its term is dropped
        assert MF.check_sigma(case, MF.sigma_oracle(short, torch.float32), r64)


def test_all_ones_gains_are_exact_in_the_float32_statement():
    case = MF.make_sigma_case(1000, 15, gains=[1.0] * 15)
    assert torch.equal(MF.sigma_oracle(case, torch.float32), case["sigma"])
