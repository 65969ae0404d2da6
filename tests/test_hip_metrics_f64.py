"""The eval image metrics on the GPU: csrc/umhs_metrics.hip per partial slot against float64 (tests/metrics_f64.py), through the C entries
so that every slot is read and not only the sum, then ``ops.ssim`` / ``ops.pixel_metrics`` and ``UMHSModel.get_image_metrics_and_images``
with the bounds propagated from the slot rules."""
import json
import math
import os

import numpy as np
import pytest
import torch

import metrics_f64 as MF
import rays_f64 as RF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
_WORST = {}


def _note(name, report):
    _WORST[name] = {k: v["worst"] for k, v in report.items()}
    print(name, {k: round(v["worst"], 3) for k, v in report.items()})
    with open(os.path.join(RF.report_dir(ROOT), "metrics_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ssim_slots(a, b, L):
    """partial [n] float64 (host) of one umhs_ssim call on device images; the NaN guard slots behind it must come back NaN."""
    from umhsnerf import _hip

    lib = _hip.lib()
    h, w, k = a.shape
    n = int(lib.umhs_ssim_partials(h, w, k))
    gy, gx = MF.grid(h, w)
    assert n == gy * gx * k
    dr = torch.full((1,), float(L), dtype=torch.float32, device=DEV)
    part = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    _hip.check(lib.umhs_ssim(_hip.ptr(a), _hip.ptr(b), h, w, k, _hip.ptr(dr), _hip.ptr(part), n, _hip.stream()), "umhs_ssim")
    part = part.cpu()
    assert bool(torch.isnan(part[n:]).all()), "a slot past n_partial was written"
    return part[:n].numpy()


def _pixel_slots(pred, gt, nb):
    """partial [nb,3] float64 (host) of one umhs_pixel_metrics call; NaN prefill, NaN guard rows behind."""
    from umhsnerf import _hip

    part = torch.full((nb + GUARD, 3), float("nan"), dtype=torch.float64, device=DEV)
    _hip.check(_hip.lib().umhs_pixel_metrics(_hip.ptr(pred), _hip.ptr(gt), pred.shape[0], pred.shape[1], _hip.ptr(part), nb, _hip.stream()),
               "umhs_pixel_metrics")
    part = part.cpu()
    assert bool(torch.isnan(part[nb:]).all()), "a slot past n_partial was written"
    return part[:nb].numpy()


# ------------------------------------------------------------------------------------------------------------------------------ #
# SSIM
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("c", MF.SSIM_CASES, ids=MF.ssim_id)
def test_every_ssim_slot_is_within_the_bound_of_float64(c):
    from umhsnerf import ops

    case, r64 = MF.ssim_reference(*c)
    a, b = _dev(case["a"]), _dev(case["b"])
    got = _ssim_slots(a, b, case["L"])
    report = {}
    fails = MF.check_ssim(case, got, r64, report=report)
    # ops.ssim: the mean, within sum bound / count; the default data_range path gives the explicit call's bits
    count = r64["v"].size
    mean = float(ops.ssim(a, b, data_range=float(case["L"]) if case["explicit"] else None))
    assert abs(mean - float(got.sum() / count)) <= got.size * 2.0 ** -52 * float(np.abs(got).sum()) / count  # (the order of a double sum)
    assert abs(mean - float(r64["v"].sum()) / count) <= MF.K_SSIM * MF.U * float(r64["mag"].sum()) / count
    if not case["explicit"]:
        explicit = float(ops.ssim(a, b, data_range=float(case["L"])))
        assert np.float64(explicit).tobytes() == np.float64(mean).tobytes()
    _note(MF.ssim_id(c), report)
    assert not fails, fails


@pytest.mark.parametrize("i", range(len(MF.IMPULSES)))
def test_impulse_windows_depend_on_single_taps_and_the_rest_is_exactly_one(i):
    case, r64 = MF.ssim_reference(MF.IMPULSE_SHAPE, f"impulse{i}")
    got = _ssim_slots(_dev(case["a"]), _dev(case["b"]), case["L"])
    report = {}
    fails = MF.check_ssim(case, got, r64, report=report)
    _note(f"impulse{i}", report)
    assert not fails, fails
    untouched = MF.slot_sums((~case["exact"]).astype(np.float64)) == 0
    assert int(untouched.sum()) >= 1 and np.array_equal(got[untouched], MF.slot_sums(np.ones((1, 17, 65)))[untouched])


def test_another_data_range_gives_another_result_within_its_own_bound():
    case, r64 = MF.ssim_reference((19, 43, 2), "noise")
    a, b = _dev(case["a"]), _dev(case["b"])
    base = _ssim_slots(a, b, case["L"])
    assert np.array_equal(base.view(np.int64), _ssim_slots(a, b, case["L"]).view(np.int64))  # fixed-order sums: the same bits
    other = _ssim_slots(a, b, 2.0)
    assert not np.array_equal(other, base)
    report = {}
    fails = MF.check_ssim(case, other, MF.ssim64(case["a"], case["b"], np.float32(2.0)), report=report)
    _note("H19-W43-K2-noise-range2", report)
    assert not fails, fails


@pytest.mark.parametrize("shape", [(19, 43, 2), (27, 75, 5)], ids=lambda s: "x".join(map(str, s)))
def test_an_image_against_itself_is_its_window_count_in_every_slot(shape):
    from umhsnerf import ops

    case, _ = MF.ssim_reference(shape, "noise")
    x = _dev(case["a"])
    L = MF.default_range(case["a"], case["a"])
    r64 = MF.ssim64(case["a"], case["a"], L)
    assert float(np.abs(r64["v"] - 1.0).max()) <= 1e-12
    got = _ssim_slots(x, x, L)
    report = {}
    fails = MF.check_ssim(dict(case, exact=None, kind="self"), got, r64, report=report)
    _note("self-" + "x".join(map(str, shape)), report)
    assert not fails, fails
    count = MF.slot_sums(np.ones_like(r64["v"]))
    assert bool((np.abs(got - count) <= MF.K_SSIM * MF.U * MF.slot_sums(r64["mag"])).all())
    assert abs(float(ops.ssim(x, x)) - 1.0) <= MF.K_SSIM * MF.U * float(r64["mag"].sum()) / r64["v"].size


# ------------------------------------------------------------------------------------------------------------------------------ #
# pixel metrics
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("c", MF.PIXEL_CASES, ids=MF.pixel_id)
def test_every_pixel_metrics_slot_is_within_the_bound_of_float64(c):
    from umhsnerf import ops

    case, r64 = MF.pixel_reference(*c)
    pred, gt = _dev(case["pred"]), _dev(case["gt"])
    nb = MF.wrapper_blocks(case["n"])
    worst = {}
    for n_partial in sorted({1, 3, nb, nb + 5}):
        got = _pixel_slots(pred, gt, n_partial)
        report = {}
        fails = MF.check_pixels(got, r64, n_partial, report=report)
        assert not fails, (n_partial, fails)
        empty = np.arange(n_partial) >= -(-case["n"] // MF.BLOCK)
        assert bool((got[empty] == 0).all()), "a block without pixels must write zeros"
        for k, v in report.items():
            worst[k] = v if k not in worst or v["worst"] > worst[k]["worst"] else worst[k]
        if n_partial == nb:
            first = ops.pixel_metrics(pred, gt)
            assert bool((np.abs(first.cpu().numpy() - got.sum(0)) <= nb * 2.0 ** -52 * np.abs(got).sum(0)).all())  # (the order of a double sum)
            assert torch.equal(first.view(torch.int64), ops.pixel_metrics(pred, gt).view(torch.int64))
    _note(MF.pixel_id(c), worst)


@pytest.mark.parametrize("K", MF.SPARSE_BANDS)
def test_the_sparse_layout_holds_every_live_pixel_on_its_own(K):
    case, r64 = MF.pixel_reference(0, K)
    m = case["n"] // MF.BLOCK
    got = _pixel_slots(_dev(case["pred"]), _dev(case["gt"]), m)
    report = {}
    fails = MF.check_pixels(got, r64, m, report=report)
    _note(f"sparse-K{K}", report)
    assert not fails, fails
    kind = {k: MF.SPARSE_KINDS.index(k) for k in set(MF.SPARSE_KINDS)}
    # what the rules already say, spelled out for the pixels that are there for it
    assert abs(got[kind["orthogonal"], 1] - math.pi / 2) <= 1e-6 and got[kind["orthogonal"], 2] == 1
    equal = [i for i, k in enumerate(MF.SPARSE_KINDS) if k == "equal bits"]
    assert bool((got[equal, 2] == 1).all()) and bool((got[equal, 0] == 0).all()) and bool((got[equal, 1] <= 1e-3).all())
    assert abs(got[kind["antiparallel"], 1] - math.pi) <= 1e-3 and abs(got[kind["parallel"], 1]) <= 1e-3
    for k in ("gt zero", "pred zero", "NaN band", "Inf band"):
        assert got[kind[k], 1] == 0 and got[kind[k], 2] == 0, k
    assert np.isnan(got[kind["NaN band"], 0]) and got[kind["Inf band"], 0] == np.inf
    assert got[kind["gt zero"], 0] > 0 and got[kind["pred zero"], 0] > 0


# ------------------------------------------------------------------------------------------------------------------------------ #
# argument errors that return before any launch
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_argument_errors_return_before_anything_is_launched():
    from umhsnerf import _hip

    lib, s = _hip.lib(), _hip.stream()
    img = torch.rand(11, 11, 2, device=DEV)
    dr = torch.ones(1, device=DEV)
    part = torch.full((8,), float("nan"), dtype=torch.float64, device=DEV)
    p = _hip.ptr
    assert lib.umhs_ssim_partials(10, 11, 2) == 0 == lib.umhs_ssim_partials(11, 10, 2) and lib.umhs_ssim_partials(11, 11, 0) == 0
    assert lib.umhs_ssim(p(img), p(img), 10, 11, 2, p(dr), p(part), 8, s) == ERR_UNSUPPORTED
    assert lib.umhs_ssim(p(img), p(img), 11, 10, 2, p(dr), p(part), 8, s) == ERR_UNSUPPORTED
    assert lib.umhs_ssim_partials(11, 11, 2) == 2
    assert lib.umhs_ssim(p(img), p(img), 11, 11, 2, p(dr), p(part), 1, s) == ERR_WORKSPACE
    for args in [(None, p(img), p(dr), p(part)), (p(img), None, p(dr), p(part)), (p(img), p(img), None, p(part)), (p(img), p(img), p(dr), None)]:
        assert lib.umhs_ssim(args[0], args[1], 11, 11, 2, args[2], args[3], 8, s) == ERR_ARG
    pix = img.view(-1, 2)
    for args in [(None, p(pix), p(part)), (p(pix), None, p(part)), (p(pix), p(pix), None)]:
        assert lib.umhs_pixel_metrics(args[0], args[1], 121, 2, args[2], 2, s) == ERR_ARG
    assert lib.umhs_pixel_metrics(p(pix), p(pix), 121, 2, p(part), 0, s) == ERR_ARG
    assert lib.umhs_pixel_metrics(p(pix), p(pix), 121, 0, p(part), 2, s) == ERR_ARG
    assert lib.umhs_pixel_metrics(p(pix), p(pix), -1, 2, p(part), 2, s) == ERR_ARG
    assert bool(torch.isnan(part).all())  # nothing ran


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
H, W, B = 24, 32, 8


def _model(background):
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    return UMHSModel(UMHSConfig(method="rgb+spectral", background_color=background),
                     metadata={"wavelengths": [420 + 30 * k for k in range(B)], "num_classes": 3}, seed=0).to(DEV)


def _pair(channels, seed):
    g = np.random.default_rng(seed)
    gt = (0.05 + 0.9 * g.random((H, W, channels))).astype(np.float32)
    pred = np.clip(gt + 0.1 * g.standard_normal((H, W, channels)), 1e-3, 2.0).astype(np.float32)
    return gt, pred


def _outputs(pred_rgb, pred_s):
    g = torch.Generator().manual_seed(3)
    return {"rgb": _dev(pred_rgb), "spectral": _dev(pred_s), "accumulation": torch.rand(H, W, 1, generator=g).to(DEV),
            "depth": (1.0 + torch.rand(H, W, 1, generator=g)).to(DEV)}


def test_model_metrics_are_within_the_bounds_propagated_from_the_slot_rules():
    """Propagation, with r = K_SSE u, N the number of values and every host step in float64 (its own rounding, ~1e-16, is inside EPS):
      psnr  = 10 log10(N / sse):  sse within (1 +- r) of sse64, so |psnr - psnr64| <= 10 log10(1 / (1 - r)) <= (10 / ln 10) r / (1 - r)
      rmse  = sqrt(sse / N):      sqrt(1 +- r) lies in 1 +- r, so |rmse - rmse64| <= r rmse64
      ssim  = sum of slots / n:   |ssim - mean v64| <= K_SSIM u sum mag / n  (the slot rule added up)
      sam   = angle sum / cnt:    cnt is exact, so sam lies in [sum lo / cnt, sum hi / cnt]  (the interval rule added up)"""
    EPS = 1e-12
    gt_rgb, pred_rgb = _pair(3, 1)
    gt_s, pred_s = _pair(B, 2)
    pred_s[5, 7], gt_s[9, 1] = 0.0, 0.0  # two pixels without an angle
    md, images = _model("black").get_image_metrics_and_images(_outputs(pred_rgb, pred_s), {"image": _dev(gt_rgb), "hs_image": _dev(gt_s)})
    assert sorted(md) == ["psnr", "psnr_spectral", "rmse_spectral", "sam_spectral", "ssim", "ssim_spectral"]
    r = MF.K_SSE * MF.U
    report = {}
    for name, (gt, pred) in {"": (gt_rgb, pred_rgb), "_spectral": (gt_s, pred_s)}.items():
        k = gt.shape[-1]
        case = dict(pred=pred.reshape(-1, k), gt=gt.reshape(-1, k), n=H * W, K=k)
        p64 = MF.pixels64(case)
        lo, hi = MF.magnitudes(case, p64)
        assert 1e-3 <= lo and hi <= 1e3
        sse64, n = float(p64["sse"].sum()), gt.size
        psnr64 = 10 * math.log10(n / sse64)
        bound = 10 / math.log(10) * r / (1 - r) + EPS
        report["psnr" + name] = {"worst": abs(md["psnr" + name] - psnr64) / bound}
        assert abs(md["psnr" + name] - psnr64) <= bound, (name, md["psnr" + name], psnr64)
        L = MF.default_range(gt, pred)
        s64 = MF.ssim64(gt, pred, L)  # (the model calls ops.ssim(gt, pred))
        cond = MF.ssim_conditions(dict(exact=None), s64)
        assert cond["eD1"] <= 1 / 16 and cond["eD2"] <= 1 / 16
        bound = MF.K_SSIM * MF.U * float(s64["mag"].sum()) / s64["v"].size + EPS
        report["ssim" + name] = {"worst": abs(md["ssim" + name] - float(s64["v"].mean())) / bound}
        assert abs(md["ssim" + name] - float(s64["v"].mean())) <= bound, (name, md["ssim" + name], float(s64["v"].mean()))
        if name:
            rmse64 = math.sqrt(sse64 / n)
            report["rmse_spectral"] = {"worst": abs(md["rmse_spectral"] - rmse64) / (r * rmse64 + EPS)}
            assert abs(md["rmse_spectral"] - rmse64) <= r * rmse64 + EPS
            cnt = int(p64["live"].sum())
            assert cnt == H * W - 2
            lo, hi = float(p64["lo"].sum()) / cnt, float(p64["hi"].sum()) / cnt
            report["sam_spectral"] = {"worst": abs(md["sam_spectral"] - (lo + hi) / 2) / ((hi - lo) / 2)}
            assert lo - EPS <= md["sam_spectral"] <= hi + EPS, (md["sam_spectral"], lo, hi)
    _note("model-24x32", report)
    assert torch.equal(images["img"], torch.cat([_dev(gt_rgb), _dev(pred_rgb)], dim=1))


@pytest.mark.parametrize("background", ["white", "black"])
def test_rgba_ground_truth_gives_the_bits_of_the_explicit_blend(background):
    gt_rgb, pred_rgb = _pair(3, 4)
    gt_s, pred_s = _pair(B, 5)
    alpha = np.random.default_rng(6).random((H, W, 1)).astype(np.float32)
    alpha[:4], alpha[4:8] = 0.0, 1.0
    rgba = _dev(np.concatenate([gt_rgb, alpha], -1))
    model = _model(background)
    outputs = _outputs(pred_rgb, pred_s)
    got, got_images = model.get_image_metrics_and_images(outputs, {"image": rgba, "hs_image": _dev(gt_s)})
    bg = 1.0 if background == "white" else 0.0
    blend = rgba[..., :3] * rgba[..., 3:] + bg * (1 - rgba[..., 3:])
    want, want_images = model.get_image_metrics_and_images(outputs, {"image": blend, "hs_image": _dev(gt_s)})
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), k
    for k in want_images:
        assert torch.equal(got_images[k], want_images[k]), k
    # the blend is the one the statement gives, and the two backgrounds differ
    a = alpha.astype(np.float32)
    assert np.array_equal(blend.cpu().numpy(), gt_rgb * a + np.float32(bg) * (np.float32(1) - a))
    plain, _ = model.get_image_metrics_and_images(outputs, {"image": _dev(gt_rgb), "hs_image": _dev(gt_s)})
    assert plain["psnr"] != got["psnr"] and plain["psnr_spectral"] == got["psnr_spectral"]
