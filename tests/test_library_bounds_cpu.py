"""CPU checks of the library-matching comparators (tests/library_f64.py): the float32 oracle passes them on every case, K is
re-measured, the tie cap and the teeth conditions hold on the float64 run alone, and the planted faults are rejected."""
import math

import pytest
import torch

import library_f64 as LF

FAULT_CASE = (300, 31, 17)


def _k_for(worst: float) -> float:
    return max(8.0, 2.0 ** math.ceil(math.log2(4.0 * worst))) if worst > 0 else 8.0


def test_float32_oracle_passes_and_k_is_what_the_rule_gives():
    worst = 0.0
    for c in LF.CASES:
        case, r64 = LF.reference(*c)
        report = {}
        index, cos = LF.oracle(case, torch.float32)
        fails = LF.check_match(case, index, cos, r64, report=report)
        assert not fails, (LF.case_id(c), fails)
        w = max(v["worst"] for v in report.values())
        print(LF.case_id(c), round(w, 3))
        worst = max(worst, w)
    print("worst", round(worst, 3))
    assert 4.0 * worst <= LF.K_COS == _k_for(worst)


def test_tie_cap_and_teeth_on_the_float64_run_alone():
    for c in LF.CASES:
        case, r64 = LF.reference(*c)
        cond = LF.conditions(case, r64)
        print(LF.case_id(c), cond)
        if cond["tied"] is not None:
            assert cond["tied"] <= LF.TIE_CAP, (LF.case_id(c), cond)
        if cond["teeth"] is not None:
            assert cond["teeth"] >= LF.MIN_TEETH, (LF.case_id(c), cond)
        index, cos = LF.oracle(case, torch.float64)
        assert not LF.check_match(case, index, cos, r64), LF.case_id(c)


def test_cases_carry_their_special_rows():
    for c in LF.CASES:
        case = LF.make_case(*c)
        s, dead = case["spectra"], case["degenerate"]
        if c[0] >= 16:
            assert int((s[dead] == 0).all(1).sum()) >= 2 and int(torch.isnan(s).any(1).sum()) == 1 and int(torch.isinf(s).any(1).sum()) == 1
            assert bool((~torch.isfinite(s).all(1) | (s == 0).all(1) == dead).all())
        if c[2] >= 3:
            a, b = case["dup"]
            assert a < b and torch.equal(case["unit"][a], case["unit"][b])
        u = case["unit"].double().norm(dim=1)
        assert bool(((u - 1).abs() < 1e-6).all())


def _planted():
    case, r64 = LF.reference(*FAULT_CASE)
    index, cos = LF.oracle(case, torch.float32)
    live = ~case["degenerate"]
    a, b = case["dup"]

    def off_by_one():
        i = index.clone()
        i[live] = (i[live] + 1) % case["L"]
        return i, cos

    def second_is_first():
        i, c = index.clone(), cos.clone()
        i[:, 1], c[:, 1] = i[:, 0], c[:, 0]
        return i, c

    def duplicate_to_later():
        i = index.clone()
        hit = (i[:, 0] == a) & (i[:, 1] == b)
        assert int(hit.sum()) >= 3
        i[hit, 0], i[hit, 1] = b, a
        return i, cos

    def nan_row_matched():
        i, c = index.clone(), cos.clone()
        r = int(torch.isnan(case["spectra"]).any(1).nonzero()[0])
        i[r], c[r] = torch.tensor([0, 1], dtype=i.dtype), torch.tensor([0.5, 0.25])
        return i, c

    return case, r64, {"last band dropped": lambda: LF.oracle(case, torch.float32, drop_last_band=True), "index off by one": off_by_one,
                       "second equals first": second_is_first, "duplicate resolved to the later index": duplicate_to_later,
                       "NaN row matched": nan_row_matched}


@pytest.mark.parametrize("fault", ["last band dropped", "index off by one", "second equals first",
                                   "duplicate resolved to the later index", "NaN row matched"])
def test_planted_fault_is_rejected(fault):
    case, r64, faults = _planted()
    index, cos = faults[fault]()
    fails = LF.check_match(case, index, cos, r64)
    print(fails)
    assert fails, fault
