"""The occupancy-grid sampler (csrc/umhs_sampler.hip through umhsnerf/sampler.py: the wave walk, the emission kernels in their count /
scratch / write forms, umhs_march_compact, visibility, ray_prefix, sample_midpoints, compact_samples) against a float64 oracle, sample
by sample: cases, oracles, tie rule and the constants K are tests/sampler_f64.py's (its docstring says what each case is there for);
tests/test_sampler_f64_bounds_cpu.py shows that the comparators reject planted faults.

Every marcher case runs through every host path; all of them must be bit-identical to the float32 restatement (march_ray_ref per ray
with that ray's planes) -- the kernels are written in its arithmetic, so no path is exempt -- and are judged by the float64 rule.
Output buffers are NaN before the launch (``nan_prefill``), so a sample a kernel never writes fails.  Figures measured on the way go
to sampler_f64.json in ``report_dir()``: per case and path the worst |diff| / (u mag) of t_starts / t_ends, per case the undecided share."""
import contextlib
import json
import os

import pytest
import torch

import sampler_f64 as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {"march": {}, "visibility": {}, "midpoints": {}}
NAN = float("nan")
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    worst = {k: max([p[k] for c in REPORT["march"].values() for p in c["paths"].values()] or [0.0]) for k in ("t_starts", "t_ends")}
    with open(os.path.join(S.report_dir(ROOT), "sampler_f64.json"), "w") as f:
        json.dump({"worst_ratio": worst, **REPORT}, f, indent=1)


@contextlib.contextmanager
def nan_prefill():
    """torch.empty hands out NaN-filled floating-point tensors: what the sampler allocates for a kernel to fill."""
    real = torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t

    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real


def _cell(name):
    """(case, float64 oracle, float32 restatement): computed once per module, never modified."""
    if name not in _cache:
        case = S.make_march_case(name)
        _cache[name] = (case, S.march_oracle(case), S.restatement(case))
    return _cache[name]


def _march(case, bin_u8):
    from umhsnerf.sampler import march_rays

    with nan_prefill():
        ri, t0, t1, pinfo = march_rays(case.o.to(DEV), case.d.to(DEV), bin_u8, case.roi, case.levels, case.res, case.near, case.far, case.step,
                                       case.cone, **case.march_kwargs(DEV))
    return {"ri": ri.cpu(), "t0": t0.cpu(), "t1": t1.cpu(), "pinfo": pinfo.cpu()}


@pytest.mark.parametrize("name", S.MARCH_CASES)
def test_marcher_on_every_host_path(name, monkeypatch):
    case, ref, rst = _cell(name)
    longest = int(rst["pinfo"][:, 1].max()) if case.R else 0
    paths = {"default": {}, "serial": {"UMHS_MARCH_SERIAL": 1}, "cap_0": {"UMHS_MARCH_CAP": 0},
             "cap_longest": {"UMHS_MARCH_CAP": max(1, longest)}, "cap_longest_minus_1": {"UMHS_MARCH_CAP": max(1, longest - 1)},
             "vseg_1": {"UMHS_MARCH_VSEG": 1}, "vcap_16": {"UMHS_MARCH_VCAP": 16}, "rpw_3": {"UMHS_MARCH_RPW": 3},
             "rpw_16": {"UMHS_MARCH_RPW": 16}, "rpw_64": {"UMHS_MARCH_RPW": 64}}
    bin_u8 = torch.from_numpy(case.binaries.astype("uint8")).to(DEV)
    rep = REPORT["march"][name] = {"undecided_share": ref.undecided_share, "samples": int(ref.counts.sum()), "paths": {}}
    fails = []
    for path, knobs in paths.items():
        with monkeypatch.context() as mp:
            for k, v in knobs.items():
                mp.setenv(k, str(v))
            got = _march(case, bin_u8)
        r = rep["paths"][path] = {}
        fails += [f"{path}: {f}" for f in S.check_march(case, ref, got, r)]
        r.pop("undecided_share", None)
        print(name, path, r)
        fails += [f"{path}: {k} differs from the float32 restatement" for k in ("pinfo", "ri", "t0", "t1")
                  if got[k].shape != rst[k].shape or not torch.equal(got[k], rst[k])]
    assert fails == []


@pytest.mark.parametrize("name", list(S.VIS_CASES))
def test_visibility_mask_with_and_without_counts(name):
    from umhsnerf.sampler import visibility_mask

    if name not in _cache:
        _cache[name] = S.make_vis_case(name)
    case = _cache[name]
    sigma, t0, t1, pinfo = (t.to(DEV) for t in (case.sigma, case.t0, case.t1, case.packed_info()))
    fails = []
    for eps, thre in S.VIS_PAIRS:
        keep = visibility_mask(sigma, t0, t1, pinfo, eps, thre)
        mask, kept = visibility_mask(sigma, t0, t1, pinfo, eps, thre, with_counts=True)
        assert keep.dtype == torch.bool and mask.dtype == torch.uint8 and torch.equal(mask.bool(), keep)
        rep = REPORT["visibility"][f"{name}:{eps}:{thre}"] = {}
        fails += [f"({eps}, {thre}): {f}" for f in S.check_visibility(case, eps, thre, keep)]
        fails += [f"({eps}, {thre}) with counts: {f}" for f in S.check_visibility(case, eps, thre, mask, kept, rep)]
    assert fails == []


@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2500])
def test_ray_prefix_against_an_int64_cumsum(R):
    """Counts of up to 2^40 (numbers only: nothing is allocated from them), so that the running total passes 2^31 within a few rays."""
    from umhsnerf.sampler import ray_prefix

    g = torch.Generator().manual_seed(600 + R)
    counts = torch.randint(0, 2 ** 40, (R,), generator=g, dtype=torch.int64)
    counts[torch.rand(R, generator=g) < 0.2] = 0
    counts[torch.rand(R, generator=g) < 0.3] %= 300
    pinfo, stats = ray_prefix(counts.to(DEV))
    ends = torch.cumsum(counts, 0)
    assert pinfo.shape == (R, 2) and torch.equal(pinfo.cpu(), torch.stack([ends - counts, counts], -1))
    assert stats.tolist() == ([int(ends[-1]), int(counts.max())] if R else [0, 0])
    assert R < 3 or int(ends[-1]) > 2 ** 31


COMPACT_ROWS = (0, 1, 63, 64, 65, 200)


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "last_of_64"])
@pytest.mark.parametrize("with_cam", [True, False])
def test_compact_samples_against_nonzero_and_index_select(pattern, with_cam):
    from umhsnerf.sampler import compact_samples, ray_prefix

    g = torch.Generator().manual_seed(77)
    counts = torch.tensor(COMPACT_ROWS, dtype=torch.int64)
    R, n = counts.numel(), int(counts.sum())
    start = torch.cumsum(counts, 0) - counts
    ri = torch.repeat_interleave(torch.arange(R), counts)
    pos = torch.arange(n) - start[ri]
    mask = {"all": torch.ones(n, dtype=torch.bool), "none": torch.zeros(n, dtype=torch.bool), "alternating": pos % 2 == 1,
            "last_of_64": pos % 64 == 63}[pattern]
    t0, t1, o, d = torch.rand(n, generator=g), torch.rand(n, generator=g), torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    cam = torch.randint(0, 9, (R, 1), generator=g) if with_cam else None
    kept = torch.zeros(R, dtype=torch.int64).index_add_(0, ri, mask.long())
    pin = torch.stack([start, counts], 1).to(DEV)
    pout, stats = ray_prefix(kept.to(DEV))
    sel = torch.nonzero(mask).view(-1)
    assert int(stats[0]) == sel.numel()
    with nan_prefill():
        out = compact_samples(mask.to(torch.uint8).to(DEV), pin, pout, sel.numel(), t0.to(DEV), t1.to(DEV), o.to(DEV), d.to(DEV),
                              None if cam is None else cam.to(DEV))
    out = {k: (v.cpu() if v is not None else None) for k, v in out.items()}
    assert torch.equal(out["sel"], sel) and torch.equal(out["ray_indices"], ri[sel])
    assert torch.equal(out["t_starts"], t0[sel]) and torch.equal(out["t_ends"], t1[sel])
    assert torch.equal(out["origins"], o[ri[sel]]) and torch.equal(out["directions"], d[ri[sel]])
    assert (out["camera_indices"] is None) if cam is None else torch.equal(out["camera_indices"], cam[ri[sel]])


@pytest.mark.parametrize("cap", [200, 333])
def test_march_compact_moves_the_scratch_rows_to_their_packed_places(cap):
    """umhs_march_compact on its own: rows of 0, 1, 63, 64, 65 and 200 samples in [R, cap] scratch rows, cap == the longest row and
    past it; what lies behind a row's count must not be copied."""
    from umhsnerf import _hip
    from umhsnerf._hip import ptr

    g = torch.Generator().manual_seed(78)
    counts = torch.tensor(COMPACT_ROWS + (0, 7, 0), dtype=torch.int64)
    R, n = counts.numel(), int(counts.sum())
    pinfo = torch.stack([torch.cumsum(counts, 0) - counts, counts], 1).contiguous()
    s0, s1 = torch.rand(R, cap, generator=g), torch.rand(R, cap, generator=g)
    live = torch.arange(cap)[None, :] < counts[:, None]
    dp, d0, d1 = pinfo.to(DEV), s0.to(DEV).contiguous(), s1.to(DEV).contiguous()
    t0, t1 = torch.full((n,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
    ri = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    _hip.check(_hip.lib().umhs_march_compact(ptr(dp), R, cap, ptr(d0), ptr(d1), ptr(t0), ptr(t1), ptr(ri), _hip.stream()), "umhs_march_compact")
    assert torch.equal(t0.cpu(), s0[live]) and torch.equal(t1.cpu(), s1[live])
    assert torch.equal(ri.cpu(), torch.repeat_interleave(torch.arange(R), counts))


def test_sample_midpoints_are_the_torch_expression_and_close_to_float64():
    from umhsnerf.sampler import sample_midpoints

    case, ref, rst = _cell("planes")
    o, d, ri, t0, t1 = (t.to(DEV) for t in (case.o, case.d, rst["ri"], rst["t0"], rst["t1"]))
    with nan_prefill():
        pos = sample_midpoints(o, d, ri, t0, t1)
    assert pos.shape == (ri.numel(), 3) and ri.numel() > 10000
    assert torch.equal(pos, o[ri] + d[ri] * (t0 + t1)[:, None] / 2.0)
    o64, d64, s64 = case.o.double()[rst["ri"]], case.d.double()[rst["ri"]], (rst["t0"].double() + rst["t1"].double()) / 2
    p64 = o64 + d64 * s64[:, None]
    ratio = (pos.cpu().double() - p64).abs() / (S.U * (o64.abs() + d64.abs() * s64.abs()[:, None]) + 2.0 ** -149)
    REPORT["midpoints"]["planes"] = {"worst": float(ratio.max())}
    assert float(ratio.max()) <= 4.0
