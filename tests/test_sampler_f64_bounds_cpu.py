"""The sampler's comparators (tests/sampler_f64.py) have the power to see the bugs they are there for: fed the float32 restatement's
own results (oracle/torch_ref.py: march_ray_ref per ray with that ray's planes, render_visibility_from_density in float32) in place of
the kernels', every case passes -- this run is also where K is measured, and where the 10 % / 1 % caps on undecided rays / elements
and the teeth condition are held, on the float64 run alone; with a fault planted in those results, every case the fault applies to
(sampler_f64.FAULT_CASES) fails.

Marcher faults: (1) no_restart: the recurrence is not restarted at the voxel entry after empty space; (2) window_restart: it is
restarted inside a continuous run where a new lane's 12 voxels begin (a shift of less than one dt); (3) coarse_level: the level is one
too coarse for m in [1, 2); (4) hx_everywhere: hx for all three axes; (5) global_far: per-ray fars ignored; (6) jitter_after_max: the
jitter added after the max with the box entry; (7) le_midpoint: "<=" in the mid-point test; (8) window_hole: the samples of voxels
64 k .. 64 k + 11 of a ray missing; (9) next_offset: one ray's samples written at the next ray's offset.
Visibility faults: (10) the carry dropped at a 64-sample chunk; (11) an inclusive sum; (12) kept off by one on a row of 64."""
import math

import numpy as np
import pytest
import torch

import sampler_f64 as S
from oracle import torch_ref as T

_cache = {}
WORST = {}


def _cell(name):
    if name not in _cache:
        case = S.make_march_case(name)
        _cache[name] = (case, S.march_oracle(case), S.restatement(case))
    return _cache[name]


def _vis(name):
    if name not in _cache:
        _cache[name] = S.make_vis_case(name)
    return _cache[name]


@pytest.mark.parametrize("name", S.MARCH_CASES)
def test_float32_restatement_passes_and_the_caps_and_teeth_hold(name):
    case, ref, got = _cell(name)
    assert S.teeth_failures(case, ref) == []  # (on the float64 run alone)
    report = {}
    assert S.check_march(case, ref, got, report) == []
    for k in ("t_starts", "t_ends"):
        WORST[k] = max(WORST.get(k, 0.0), report[k])
    if name in S.NONEMPTY:
        assert report["samples_compared"] >= 0.8 * int(ref.counts.sum())
    else:
        assert int(ref.counts.sum()) == 0 and got["t0"].numel() == 0
    print(name, report)


@pytest.mark.parametrize("name", S.MARCH_CASES)
def test_faultless_walker_is_march_ray_ref_bit_for_bit(name):
    """march_ray_f32 is the function the walk's faults are planted in: without one it must BE the restatement."""
    case, _, got = _cell(name)
    mine = S.faulty_restatement(case, None)
    assert all(torch.equal(mine[k], got[k]) for k in got)


def test_the_cases_hold_what_they_are_there_for():
    case, ref, got = _cell("planes")
    assert float(case.fars[0]) < float(case.nears[0]) and int(ref.counts[0]) == 0 and int(ref.counts[50]) == 0
    assert int((ref.counts == 0).sum()) >= 6 and bool((case.d == 0).any()) and bool(torch.signbit(case.d[-1][2]))
    assert case.R % 4 != 0 and case.R % 64 != 0
    start = np.cumsum(ref.counts) - ref.counts
    at_near = [r for r in range(36) if ref.counts[r] and ref.ts[start[r]] == float(case.nears[r]) + float(case.jitter[r]) * case.jitter_step]
    assert len(at_near) >= 5  # near planes inside an occupied voxel: the first run starts on the plane itself
    case, ref, got = _cell("full")  # the two dyadic rays end on an exact mid-point == far tie, and are decided
    assert bool(ref.decided[-1]) and bool(ref.decided[-2]) and int(ref.counts[-1]) == 40 and int(ref.counts[-2]) == 40
    case, ref, got = _cell("deep")
    assert case.levels == 8 and float(ref.te.max()) > 30  # samples out in the coarsest levels
    assert S.make_march_case("cube_R1").R == 1 and S.make_march_case("cube_R0").R == 0


@pytest.mark.parametrize("fault", S.MARCH_FAULTS)
def test_planted_marcher_fault_fails_every_case_it_applies_to(fault):
    for name in S.FAULT_CASES[fault]:
        case, ref, got = _cell(name)
        bad = S.faulty_restatement(case, fault, ref)
        assert S.check_march(case, ref, bad) != [], (fault, name)


def test_K_covers_the_float32_restatement_four_times():
    for name in S.MARCH_CASES:  # (when run alone)
        case, ref, got = _cell(name)
        report = {}
        S.check_march(case, ref, got, report)
        for k in ("t_starts", "t_ends"):
            WORST[k] = max(WORST.get(k, 0.0), report[k])
    print("worst float32 ratios", WORST)
    for k, K in (("t_starts", S.K_STARTS), ("t_ends", S.K_ENDS)):
        assert WORST[k] > 0 and K == max(8.0, 2.0 ** math.ceil(math.log2(4 * WORST[k]))), (k, WORST[k], K)


# ---- visibility ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.VIS_CASES))
def test_float32_visibility_passes_and_its_cap_holds(name):
    case = _vis(name)
    assert case.R % 4 == S.VIS_CASES[name][1] % 4 and int(case.counts[-1]) == 0 and tuple(case.counts[:10].tolist()) == S.VIS_ROWS
    Tt, X, alpha = S.vis_oracle(case)
    if name.startswith("wall"):
        assert float(X.max()) > 1e4 and float(Tt.min()) == 0.0
    worst_T = worst_a = 0.0
    for eps, thre in S.VIS_PAIRS:
        und = S.vis_undecided(case, eps, thre)
        assert float(und.float().mean()) <= 0.01, (eps, thre)
        ref = T.render_visibility_from_density(case.t0, case.t1, case.sigma, case.packed_info(), eps, thre)
        mask, kept, T32, a32 = S.visibility_f32(case, eps, thre)
        for m in (ref, mask):
            rep = {}
            assert S.check_visibility(case, eps, thre, m, kept if m is mask else None, rep) == [], (eps, thre)
        if name.startswith("wall"):
            behind = X > 1e4
            assert bool(behind.any()) and bool(ref[behind].all()) == (eps == 0.0) and (eps == 0.0 or not bool(ref[behind].any()))
        else:
            assert 0 < int(ref.sum()) < ref.numel()
        # (measured where the sample's own x <= 1: the exclusive sum is inclusive - own in the restatement and in the kernel alike, so
        #  the first sample of a wall, x = 35,000, carries u x in its X; none of them is near a threshold -- they pass above)
        live = (X < 80) & (case.sigma.double() * (case.t1.double() - case.t0.double()) <= 1)
        worst_T = max(worst_T, float(((T32.double() - Tt).abs() / (S.U * Tt * (1 + X)))[live].max()))
        worst_a = max(worst_a, float((a32.double() - alpha).abs().max() / S.U))
    print(name, "worst float32 ratios: T", worst_T, "alpha", worst_a)
    assert S.K_VIS >= 8 and 4 * max(worst_T, worst_a) <= S.K_VIS


@pytest.mark.parametrize("fault", ["carry", "inclusive", "kept64"])
@pytest.mark.parametrize("name", list(S.VIS_CASES))
def test_planted_visibility_fault_fails(name, fault):
    case = _vis(name)
    for eps, thre in S.VIS_PAIRS:
        if fault != "kept64" and eps == 0.0:
            continue  # (eps = 0 keeps every T: the sum does not enter the decision)
        mask, kept, _, _ = S.visibility_f32(case, eps, thre, fault)
        assert S.check_visibility(case, eps, thre, mask, kept) != [], (eps, thre)
