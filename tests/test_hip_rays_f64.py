"""The per-ray kernels (csrc/umhs_rays.hip: pack_info, composite_fwd / bwd / bwd_dots, accumulate_fwd / bwd; csrc/umhs_tail.hip: spec2rgb,
tmid_minmax, ray_epilogue, loss, ray_train_tail) against a float64 oracle, element by element: cases, oracle runs, envelopes and the
constants K are tests/rays_f64.py's (its docstring says which case selects which kernel path); tests/test_rays_f64_bounds_cpu.py shows
that the comparators reject planted faults.

The kernels are called through umhsnerf.ops; where ops has no wrapper (umhs_composite_bwd_dots, accumulate_bwd with its d_weights, a
second forward into the same buffers) through _hip.lib().  Every output buffer is NaN before the launch -- ops allocates its outputs
with torch.empty / torch.empty_like, which ``nan_prefill`` replaces for the duration of the call -- so an element a kernel never writes
fails its comparison.  Figures measured on the way go to rays_f64.json in RF.report_dir(): per case and output, the worst |diff| / (u mag) and
the share of elements with teeth."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import rays_f64 as RF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    worst = {}
    for case, rep in REPORT.items():
        for k, v in rep.items():
            fam = _family(k)
            worst[fam] = max(worst.get(fam, 0.0), v["worst"])
    with open(os.path.join(RF.report_dir(ROOT), "rays_f64.json"), "w") as f:
        json.dump({"worst_ratio_per_family": worst, "cases": REPORT}, f, indent=1)


def _family(key: str) -> str:
    if key.startswith("accumulate.out"):
        return "accumulate"
    key = key.split(".")[-1]
    if key.startswith("d_sigma"):
        return "d_sigma"
    if key.startswith("d_values"):
        return "d_values"
    if key == "d_weights" or key.startswith("accumulate.out"):
        return "accumulate"
    if key == "weights":
        return "weights"
    if key in ("acc", "depth") or key.startswith("out"):
        return "per-ray sums"
    if key in ("rgb", "seg_probs"):
        return key
    return "losses" if key.endswith("losses") else "tail gradients"


@contextlib.contextmanager
def nan_prefill():
    """torch.empty / torch.empty_like hand out NaN-filled floating-point tensors: what ops allocates for a kernel to fill."""
    real = torch.empty, torch.empty_like

    def filled(fn):
        def f(*a, **k):
            t = fn(*a, **k)
            return t.fill_(NAN) if t.is_floating_point() else t
        return f

    torch.empty, torch.empty_like = filled(real[0]), filled(real[1])
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real


def _mods():
    from umhsnerf import _hip, ops

    return ops, _hip


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------ #
# compositing
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spec", RF.COMPOSITE_CASES, ids=RF.case_id)
def test_compositing_kernels_against_float64(spec):
    ops, _hip = _mods()
    lib, ptr = _hip.lib(), _hip.ptr
    case = RF.make_ray_case(*spec)
    r64 = RF.composite_oracle(case, torch.float64)
    env = RF.composite_envelopes(case, r64)
    R, n = case.R, case.n
    report = REPORT.setdefault("composite " + RF.case_id(spec), {})
    sigma, t0, t1 = case.sigma.to(DEV), case.t0.to(DEV), case.t1.to(DEV)
    values, d_outs, d_acc = [v.to(DEV) for v in case.values], [d.to(DEV) for d in case.d_outs], case.d_acc.to(DEV)
    pinfo = ops.pack_info(case.ray_indices().to(DEV), R)
    assert torch.equal(pinfo.cpu(), case.packed_info())  # index work: bit for bit, empty rays included

    with nan_prefill():
        weights, acc, depth, outs = ops.composite_fwd(sigma, t0, t1, pinfo, values)
    fails = RF.check_composite_forward(case, {"weights": weights, "outs": outs, "acc": acc, "depth": depth}, r64, env, report)

    # a second call into the same buffers: the base == 0 overwrite, and the kernel's stated reproducibility
    first = [t.clone() for t in [weights, acc, depth] + outs]
    st = _hip.ValueStreams()
    st.n_streams = len(values)
    for i, (v, o) in enumerate(zip(values, outs)):
        st.k[i], st.values[i], st.out[i] = v.shape[1], v.data_ptr(), o.data_ptr()
    _hip.check(lib.umhs_composite_fwd(ptr(sigma), ptr(t0), ptr(t1), ptr(pinfo), R, n, C.byref(st), ptr(weights), ptr(acc), ptr(depth),
                                      _hip.stream()), "umhs_composite_fwd")
    for a, b in zip(first, [weights, acc, depth] + outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second forward into the same buffers changed bits"

    with nan_prefill():
        d_sigma, d_values = ops.composite_bwd(sigma, t0, t1, pinfo, weights, values, d_outs, case.want, d_acc, case.grad_scaling)
    assert [g is not None for g in d_values] == case.want
    fails += RF.check_composite_backward(case, {"d_sigma": d_sigma, "d_values": d_values}, r64, env, report)  # d_sigma: fully written

    # the density half alone, from dots formed in float64 and rounded once
    dots, ds2 = RF.dots64(case).to(DEV), _nan(n)
    _hip.check(lib.umhs_composite_bwd_dots(ptr(sigma), ptr(t0), ptr(t1), ptr(pinfo), R, n, ptr(weights), ptr(dots), ptr(d_acc),
                                           int(case.grad_scaling), ptr(ds2), _hip.stream()), "umhs_composite_bwd_dots")
    fails += RF.check_composite_backward(case, {"d_sigma": ds2}, r64, env, report, prefix="dots.")

    # accumulate_fwd / accumulate_bwd on the forward's weights
    if values:
        ref = RF.accumulate_reference(case, weights)
        for i, v in enumerate(values):
            with nan_prefill():
                o = ops.accumulate_fwd(weights, v, pinfo)
            fails += RF.check(f"accumulate.out{i}", o, ref["outs"][i], ref["outs_mag"][i], RF.K_ACCUM, report)
        g = _hip.ValueGrads()
        g.n_streams = len(values)
        dvs = [_nan(*v.shape) if w else None for v, w in zip(values, case.want)]
        for i, (v, d, dv) in enumerate(zip(values, d_outs, dvs)):
            g.k[i], g.values[i], g.d_out[i], g.d_values[i] = v.shape[1], v.data_ptr(), d.data_ptr(), dv.data_ptr() if dv is not None else None
        d_w = _nan(n)
        _hip.check(lib.umhs_accumulate_bwd(ptr(weights), ptr(pinfo), R, n, C.byref(g), ptr(d_w), _hip.stream()), "umhs_accumulate_bwd")
        fails += RF.check("accumulate.d_weights", d_w, ref["d_weights"], ref["d_weights_mag"], RF.K_ACCUM, report)
        for i, dv in enumerate(dvs):
            if dv is not None:
                fails += RF.check(f"accumulate.d_values{i}", dv, ref["d_values"][i], ref["d_values_mag"][i], RF.K_DVALUES, report)
    print(RF.case_id(spec), {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})
    assert not fails, fails
    assert not RF.teeth_failures(case, report), RF.teeth_failures(case, report)


# ------------------------------------------------------------------------------------------------------------------------------ #
# tail
# ------------------------------------------------------------------------------------------------------------------------------ #
TAIL_SHAPES = [(1, 1, 1), (15, 3, 6), (16, 15, 16), (17, 16, 1), (1001, 17, 6), (15, 31, 16), (17, 65, 6), (1001, 141, 16), (16, 141, 1),
               (1, 31, 6),
               (16384 + 17, 3, 2),  # past 1024 workgroups x 16 rays: ray_train_tail's stride loop
               (1024 * 4 + 5, 3, 2)]  # past 256 workgroups x 4 waves x 4 rounds: loss_fwd's stride loop


@pytest.mark.parametrize("R,B,Cn", TAIL_SHAPES)
def test_tail_kernels_against_float64(R, B, Cn):
    ops, _hip = _mods()
    case = RF.make_tail_case(R, B, Cn)
    r64 = RF.tail_oracle(case, torch.float64)
    env = RF.tail_envelopes(case, r64)
    assert env["left_out_share"] <= 0.02
    report = REPORT.setdefault(f"tail R{R} B{B} C{Cn}", {})
    d = lambda t: t.to(DEV).contiguous()
    spec, M, E, acc, depth, colors = d(case.spec), d(case.M), d(case.E), d(case.acc), d(case.depth), d(case.colors)
    gt, gt_rgb, bg, rgb_in, cot = d(case.gt_spec), d(case.gt_rgb), d(case.bg), d(case.rgb_in), d(case.cot_rgb)
    mm = ops.tmid_minmax(d(case.tm0), d(case.tm1), out=_nan(2))
    a, ws, wr = case.alpha, case.w_spec, case.w_rgb

    # the separate kernels
    got = {}
    with nan_prefill():
        rgb = ops.spec2rgb_fwd(spec, M)
        got["s2r_d_spec"] = ops.spec2rgb_bwd(spec, M, cot)
        rgb_e, dclip, probs, raw, pred = ops.ray_epilogue_fwd(spec, M, E, acc, depth, mm, colors, a)
        got["sep_losses"] = ops.loss_fwd(spec, gt, rgb_in, acc, bg, gt_rgb, ws, wr)
        got["sep_d_spec"], got["sep_d_rgb"], got["sep_d_acc"] = ops.loss_bwd(spec, gt, rgb_in, acc, bg, gt_rgb, ws, wr,
                                                                             torch.tensor(case.g_up, device=DEV))
        l_only = ops.loss_fwd(spec, gt, None, None, None, None, ws, 0.0)
        got["sep_d_spec_only"], no_rgb, no_acc = ops.loss_bwd(spec, gt, None, None, None, None, ws, 0.0, torch.tensor(case.g_up, device=DEV))
    assert no_rgb is None and no_acc is None
    got["s2r_d_spec_acc"] = ops.spec2rgb_bwd(spec, M, cot, accumulate_into=d(case.prev))
    fails = RF.check_tail_separate(case, got, r64, env, report, prefix="separate.")
    fails += RF.check_tail(case, {"rgb": rgb}, r64, env, report=report, prefix="spec2rgb.")
    fails += RF.check_tail(case, {"rgb": rgb_e, "dclip": dclip, "probs": probs, "seg_raw": raw, "seg_pred": pred}, r64, env, report=report,
                           prefix="epilogue.")
    fails += RF.check("separate.loss_without_rgb", l_only[:1], r64["sep_losses"][:1], env["sep_losses"][:1], RF.K_LOSS, report)
    assert float(l_only[1]) == 0.0

    # the fused tail, with and without the rgb loss, three calls each
    for both in (True, False):
        o64 = r64 if both else RF.tail_oracle(case, torch.float64, rgb_loss=False)
        e64 = env if both else RF.tail_envelopes(case, o64, rgb_loss=False)
        first = None
        for rep in range(3):
            with nan_prefill():
                rgb_t, dclip_t, probs_t, raw_t, pred_t, losses, d_spec, d_acc = ops.ray_train_tail(
                    spec, M, E, acc, depth, mm, colors, gt, gt_rgb if both else None, bg if both else None, a, ws, wr, both)
            if rep == 0:
                fails += RF.check_tail(case, {"rgb": rgb_t, "dclip": dclip_t, "probs": probs_t, "seg_raw": raw_t, "seg_pred": pred_t,
                                              "losses": losses, "d_spec": d_spec, "d_acc": d_acc}, o64, e64, both, report,
                                       prefix="fused." if both else "fused_spectral_only.")
                assert (d_acc is None) == (not both)
                first = losses.clone()
            else:  # the block-order sum of the partials is reproducible; the arrival counter was left at zero
                assert torch.equal(losses.view(torch.int32), first.view(torch.int32))
        counter = ops._ws_cache[(torch.device(DEV).index or 0, ops.WS_TAIL)][:4].view(torch.int32)
        assert int(counter[0]) == 0
    print((R, B, Cn), {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------------ #
# tmid_minmax
# ------------------------------------------------------------------------------------------------------------------------------ #
def _decode(mm: torch.Tensor) -> np.ndarray:
    """The ordered encoding of (min, max) back to floats (umhs_tail.hip ord2f)."""
    u = mm.view(torch.int32).cpu().numpy().view(np.uint32)
    return np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("n", [0, 1, 255, 2049, 256 * 2048 + 3])  # the last: past 256 workgroups x 2048 elements, the stride loop
@pytest.mark.parametrize("last", ["max", "min"])
def test_tmid_minmax_is_exact(n, last):
    ops, _ = _mods()
    g = torch.Generator().manual_seed(n + 5)
    t0 = torch.randn(n, generator=g) * 2  # mid-points of both signs
    t1 = t0 + 0.01 * torch.rand(n, generator=g)
    if n:
        t0[0] = t1[0] = -0.0
        t0[-1] = t1[-1] = 64.0 if last == "max" else -64.0  # the extreme in the last element (2 randn stays far inside)
    if n == 1:
        t0[0] = t1[0] = -0.0
    mm = ops.tmid_minmax(t0.to(DEV), t1.to(DEV), out=_nan(2))
    if n == 0:  # the identity of (min, max) in the ordered encoding
        assert mm.view(torch.int32).cpu().tolist() == [-1, 0]
        return
    mid = (t0 + t1) / 2
    lo, hi = _decode(mm)
    assert lo == float(mid.min()) and hi == float(mid.max())
    if n == 1:
        assert np.signbit(lo) and np.signbit(hi)  # -0.0 stays -0.0
    else:
        assert (hi if last == "max" else lo) == float(mid[-1])
