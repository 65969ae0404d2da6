"""CPU checks of the image-metric comparators (tests/metrics_f64.py): the float64 truth agrees with the oracle's reflect-pad / convolve /
crop route, the float32 restatement passes every rule on every case, each K is re-measured, the conditions hold on the float64 run alone,
and the planted faults are rejected."""
import numpy as np
import pytest
import torch

import metrics_f64 as MF
from oracle import torch_ref as T

ALL_SSIM = MF.SSIM_CASES + [(MF.IMPULSE_SHAPE, f"impulse{i}") for i in range(len(MF.IMPULSES))]
ALL_PIXELS = MF.PIXEL_CASES + [(0, k) for k in MF.SPARSE_BANDS]


def _pixel_id(c):
    return f"sparse-K{c[1]}" if c[0] == 0 else MF.pixel_id(c)


def _n_partials(n):
    nb = MF.wrapper_blocks(n)
    return sorted({1, 3, nb, nb + 5})


def test_float64_truth_agrees_with_the_oracles_convolution_route():
    for c in MF.SSIM_CASES[:6]:
        case, r64 = MF.ssim_reference(*c)
        chw = lambda x: torch.moveaxis(torch.from_numpy(x).double(), -1, 0)[None]
        want = float(T.ssim_ref(chw(case["a"]), chw(case["b"]), float(case["L"])))
        got = float(r64["v"].mean())
        print(MF.ssim_id(c), got, want)
        assert abs(got - want) <= 1e-12
    case, r64 = MF.ssim_reference(*MF.SSIM_CASES[0])  # the default data_range is the oracle's
    chw = lambda x: torch.moveaxis(torch.from_numpy(x), -1, 0)[None]
    assert float(case["L"]) == float(max(chw(case["a"]).max() - chw(case["a"]).min(), chw(case["b"]).max() - chw(case["b"]).min()))


def test_float32_ssim_restatement_passes_and_k_is_what_the_rule_gives():
    worst, where, ceiling = 0.0, None, 0.0
    for c in ALL_SSIM:
        case, r64 = MF.ssim_reference(*c)
        report = {}
        v32 = MF.ssim32(case["a"], case["b"], case["L"])
        if case["exact"] is not None:
            assert bool((v32[np.broadcast_to(case["exact"], v32.shape)] == 1.0).all())
        fails = MF.check_ssim(case, MF.slot_sums(v32.astype(np.float64)), r64, report=report)
        assert not fails, (MF.ssim_id(c), fails)
        # per window too: the slot sum must not be what keeps the restatement inside
        per_window = float((np.abs(v32.astype(np.float64) - r64["v"]) / (MF.U * r64["mag"])).max())
        print(MF.ssim_id(c), {k: round(v["worst"], 3) for k, v in report.items()}, "per window", round(per_window, 3))
        assert per_window <= MF.K_SSIM
        w = max(report["ssim"]["worst"], per_window)
        if w > worst:
            worst, where = w, MF.ssim_id(c)
        ceiling = max(ceiling, report.get("ceiling", {"worst": 0.0})["worst"])
    print("K_SSIM: worst", round(worst, 3), "at", where, "-> K", MF.k_for(worst), "| ceiling: worst excess", round(ceiling, 3))
    assert 4.0 * worst <= MF.K_SSIM == MF.k_for(worst)
    assert 4.0 * ceiling <= MF.K_SSIM


def _sam_ratio(case, partial, nb):
    """The angle rule is an interval, not a difference: its "ratio" is the smallest power of two k at which the intervals built with
    K_SAM = k hold the sum in every slot (k_for rounds up to a power of two anyway, so nothing is lost)."""
    for e in range(-6, 8):
        r = MF.pixels64(case, 2.0 ** e)
        lo, hi = MF.block_sums(r["lo"], nb), MF.block_sums(r["hi"], nb)
        if bool(((lo <= partial[:, 1]) & (partial[:, 1] <= hi)).all()):
            return 2.0 ** e
    return float("inf")


def test_float32_pixel_restatement_passes_and_k_is_what_the_rule_gives():
    worst = {"sse": (0.0, None), "sam": (0.0, None)}
    for c in ALL_PIXELS:
        case, r64 = MF.pixel_reference(*c)
        for nb in _n_partials(case["n"]) + ([case["n"] // MF.BLOCK] if c[0] == 0 else []):
            report = {}
            got = MF.pixels32(case, nb)
            fails = MF.check_pixels(got, r64, nb, report=report)
            assert not fails, (_pixel_id(c), nb, fails)
            report["sam"]["worst"] = _sam_ratio(case, got, nb)
            for k in worst:
                if report[k]["worst"] > worst[k][0]:
                    worst[k] = (report[k]["worst"], f"{_pixel_id(c)} at n_partial {nb}")
        print(_pixel_id(c), {k: round(v["worst"], 3) for k, v in report.items()})
    print("K_SSE: worst", worst["sse"], "-> K", MF.k_for(worst["sse"][0]), "| K_SAM: worst", worst["sam"], "-> K", MF.k_for(worst["sam"][0]))
    assert 4.0 * worst["sse"][0] <= MF.K_SSE == MF.k_for(worst["sse"][0])
    assert 4.0 * worst["sam"][0] <= MF.K_SAM == MF.k_for(worst["sam"][0])


def test_conditions_on_the_float64_run_alone():
    worst = {"eD1": 0.0, "eD2": 0.0, "teeth": 1.0}
    for c in ALL_SSIM:
        case, r64 = MF.ssim_reference(*c)
        cond = MF.ssim_conditions(case, r64)
        print(MF.ssim_id(c), {k: float(f"{v:.3g}") for k, v in cond.items()})
        assert cond["eD1"] <= 1 / 16 and cond["eD2"] <= 1 / 16, (MF.ssim_id(c), cond)
        if case["kind"] not in MF.NO_TEETH:
            assert cond["teeth"] >= MF.MIN_TEETH, (MF.ssim_id(c), cond)
            worst["teeth"] = min(worst["teeth"], cond["teeth"])
        worst["eD1"], worst["eD2"] = max(worst["eD1"], cond["eD1"]), max(worst["eD2"], cond["eD2"])
        # the float64 run passes its own comparator with nothing to spare needed
        assert not MF.check_ssim(case, MF.slot_sums(r64["v"]), r64), MF.ssim_id(c)
    lo, hi = 1.0, 1.0
    for c in ALL_PIXELS:
        case, r64 = MF.pixel_reference(*c)
        m = MF.magnitudes(case, r64)
        lo, hi = min(lo, m[0]), max(hi, m[1])
        assert 1e-3 <= m[0] and m[1] <= 1e3, (_pixel_id(c), m)
    print("worst", worst, "magnitudes", (lo, hi))


def test_cases_reach_what_they_are_there_for():
    # slots: one window; one full block per channel; four blocks of which three hold one row, one column, one window
    assert [MF.grid(h, w) for (h, w, _) in MF.SSIM_SHAPES] == [(1, 1), (1, 1), (2, 2), (3, 3), (1, 5)]
    ones = np.ones((1, 9, 33))
    assert MF.slot_sums(ones).tolist() == [256.0, 8.0, 32.0, 1.0]
    # the impulses sit on the seams, and every impulse case has slots of all-zero windows and slots with touched ones
    assert {p[0][1] for p in MF.IMPULSES} | {p[1][1] for p in MF.IMPULSES} >= {31, 32, 41, 42}
    assert {p[0][0] for p in MF.IMPULSES} | {p[1][0] for p in MF.IMPULSES} >= {7, 8, 17, 18}
    for i in range(len(MF.IMPULSES)):
        case = MF.make_impulse_case(i)
        touched = MF.slot_sums((~case["exact"]).astype(np.float64))
        assert bool((touched == 0).any()) and bool((touched > 0).any())
    # the largest pixel case takes the second grid-stride trip at the wrapper's cap, by the smallest margin that fills a block and more
    n = max(c[0] for c in MF.PIXEL_CASES)
    assert MF.wrapper_blocks(n) == MF.MAX_BLOCKS and n == MF.MAX_BLOCKS * MF.BLOCK + 257
    # the sparse layout: one live pixel per 256 at most, every kind there, and a float32 cosine above 1 among the equal-bits pixels
    for k in MF.SPARSE_BANDS:
        case, r64 = MF.pixel_reference(0, k)
        nz = ((case["pred"] != 0) | (case["gt"] != 0)).any(1)
        assert bool((nz.nonzero()[0] % MF.BLOCK == 0).all()) and int(r64["live"].sum()) == len(MF.SPARSE_KINDS) - 4
        assert int(np.isnan(case["pred"]).any(1).sum()) == 1 and int(np.isinf(case["gt"]).any(1).sum()) == 1
    for c in MF.PIXEL_CASES:
        case, r64 = MF.pixel_reference(*c)
        if c[0] >= 255:
            assert int((~r64["live"]).sum()) == 7


SSIM_FAULT_CASES = {
    "halo column 10": [((19, 43, 2), "noise"), (MF.IMPULSE_SHAPE, "impulse2")],
    "tap 10 dropped": [((11, 11, 1), "noise"), (MF.IMPULSE_SHAPE, "impulse0")],
    "sigma 1.4": [((18, 42, 3), "noise")],
    "window validity <": [((19, 43, 2), "noise"), ((11, 11, 1), "noise")],
    "channel stride 1": [((19, 43, 2), "noise"), ((12, 140, 141), "noise")],
    "k2 = 0.02": [((18, 42, 3), "noise"), ((19, 43, 2), "negcov")],
    "variance not clamped": [((19, 43, 2), "const-zero")],
    "data_range from a": [((19, 43, 2), "noise"), ((19, 43, 2), "x100")],
}
PIXEL_FAULT_CASES = {
    "SAM clamp removed": [(0, 3), (0, 31)],
    "zero spectra counted": [(0, 31), (257, 3)],
    "second trip dropped": [(MF.MAX_BLOCKS * MF.BLOCK + 257, 1)],
}


@pytest.mark.parametrize("fault", MF.SSIM_FAULTS)
def test_planted_ssim_fault_is_rejected(fault):
    caught = []
    for c in SSIM_FAULT_CASES[fault]:
        case, r64 = MF.ssim_reference(*c)
        v = MF.ssim32(case["a"], case["b"], case["L"], fault=fault)
        fails = MF.check_ssim(case, MF.slot_sums(v.astype(np.float64)), r64)
        print(fault, "|", MF.ssim_id(c), "|", fails or "NOT rejected")
        if fails:
            caught.append(MF.ssim_id(c))
    print(f"fault '{fault}' rejected on: {caught}")
    assert caught, fault


@pytest.mark.parametrize("fault", MF.PIXEL_FAULTS)
def test_planted_pixel_fault_is_rejected(fault):
    caught = []
    for c in PIXEL_FAULT_CASES[fault]:
        case, r64 = MF.pixel_reference(*c)
        nb = MF.wrapper_blocks(case["n"])
        fails = MF.check_pixels(MF.pixels32(case, nb, fault=fault), r64, nb)
        print(fault, "|", _pixel_id(c), "|", fails or "NOT rejected")
        if fails:
            caught.append(_pixel_id(c))
    print(f"fault '{fault}' rejected on: {caught}")
    assert caught, fault


def test_unclamped_variance_is_invisible_to_the_symmetric_rule_alone():
    """Why the ceiling exists: the clamp only ever acts on a NEGATIVE float32 s2 - s0^2, which is rounding noise of a variance that is
    >= 0, and the slot rule must admit that noise in either direction.  So on every case the unclamped restatement stays inside the
    symmetric rule; only the one-sided ceiling of "const-zero" separates the two."""
    for c in MF.SSIM_CASES:
        case, r64 = MF.ssim_reference(*c)
        v = MF.ssim32(case["a"], case["b"], case["L"], fault="variance not clamped")
        fails = MF.check_ssim(case, MF.slot_sums(v.astype(np.float64)), r64)
        assert all("ceiling" in f for f in fails), (MF.ssim_id(c), fails)
    case, _ = MF.ssim_reference((19, 43, 2), "const-zero")
    differ = MF.ssim32(case["a"], case["b"], case["L"]) != MF.ssim32(case["a"], case["b"], case["L"], fault="variance not clamped")
    print("const-zero: windows whose float32 variance is negative:", int(differ.sum()), "of", differ.size)
    assert int(differ.sum()) >= differ.size // 10
