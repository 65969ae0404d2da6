"""The per-ray comparators (tests/rays_f64.py) have the power to see the bugs they are there for: fed the float32 oracle's own results
in place of the kernels', every case passes (this run is also where K is measured, and where the teeth condition and the 2 % cap on
left-out rays are held); with a fault planted in those results, every case the fault applies to fails.

Faults: (1) the transmittance carry dropped at a 64-sample chunk boundary; (2) d_sigma's exclusive suffix made inclusive by one sample;
(3) the gradient scale omitted; (4) the two halves of a paired-stream round swapped; (5) band 32 of a K = 33 stream missing from dw;
(6) a third chunk overwriting the per-ray sum instead of adding to it; (7) d_values of the last sample of a ragged chunk left at the
NaN prefill; (8) rays past 16,384 missing from the loss sums and keeping stale d_spectral; (9) the clamp gradient passed where y > 1;
(10) F.normalize's epsilon applied to the squared norm."""
import dataclasses
import math

import pytest
import torch

import rays_f64 as RF

CASES = {RF.case_id(c): c for c in RF.COMPOSITE_CASES}
TAIL_CASES = {"R17_B3_C1": (17, 3, 1), "R1001_B31_C6": (1001, 31, 6), "R65_B141_C16": (65, 141, 16), "R16401_B3_C2": (16384 + 17, 3, 2),
              "R1_B16_C2": (1, 16, 2)}
_cache = {}
WORST = {}  # family -> worst float32-oracle ratio seen by the clean runs


def _cell(name):
    if name not in _cache:
        torch.set_num_threads(max(1, min(torch.get_num_threads(), 16)))
        case = RF.make_ray_case(*CASES[name])
        r32, r64 = RF.composite_oracle(case, torch.float32), RF.composite_oracle(case, torch.float64)
        _cache[name] = (case, r32, r64, RF.composite_envelopes(case, r64))
    return _cache[name]


def _tail(name):
    if name not in _cache:
        case = RF.make_tail_case(*TAIL_CASES[name])
        r32, r64 = RF.tail_oracle(case, torch.float32), RF.tail_oracle(case, torch.float64)
        _cache[name] = (case, r32, r64, RF.tail_envelopes(case, r64))
    return _cache[name]


def _tail_family(key):
    if key in ("rgb", "seg_probs"):
        return key
    return "losses" if key.endswith("losses") else "tail gradients"


def _family(key):
    if key.startswith("d_sigma"):
        return "d_sigma"
    if key.startswith("d_values"):
        return "d_values"
    return "weights" if key == "weights" else "per-ray sums"


def _note(report, family=None):
    for k, v in report.items():
        f = family(k) if family else _family(k)
        WORST[f] = max(WORST.get(f, 0.0), v["worst"])


def _judge(name, fwd=None, bwd=None):
    case, r32, r64, env = _cell(name)
    report = {}
    fails = RF.check_composite_forward(case, r32 if fwd is None else fwd, r64, env, report)
    fails += RF.check_composite_backward(case, r32 if bwd is None else bwd, r64, env, report)
    return fails, report


@pytest.mark.parametrize("name", list(CASES))
def test_the_float32_oracle_passes_the_compositing_comparators(name):
    case = _cell(name)[0]
    fails, report = _judge(name)
    assert not fails, fails
    assert not RF.teeth_failures(case, report), RF.teeth_failures(case, report)
    _note(report)
    print(name, {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[0]])
def test_the_float32_oracle_passes_the_accumulate_comparators(name):
    """accumulate_fwd / accumulate_bwd take the forward's float32 weights as an input: float32 sums of those against float64 sums."""
    case, r32, _, _ = _cell(name)
    report = {}
    assert not _judge_accumulate(case, r32["weights"], report)
    _note(report, lambda k: "accumulate" if "d_values" not in k else "d_values")


def _judge_accumulate(case, w32, report):
    ri = case.ray_indices()
    ref = RF.accumulate_reference(case, w32)
    fails, d_w = [], torch.zeros(case.n)
    for i, (v, d) in enumerate(zip(case.values, case.d_outs)):
        fails += RF.check(f"out{i}", RF.T.accumulate_along_rays(w32, v, ri, case.R), ref["outs"][i], ref["outs_mag"][i], RF.K_ACCUM, report)
        fails += RF.check(f"d_values{i}", w32[:, None] * d[ri], ref["d_values"][i], ref["d_values_mag"][i], RF.K_DVALUES, report)
        d_w = d_w + (d[ri] * v).sum(1)
    return fails + RF.check("d_weights", d_w, ref["d_weights"], ref["d_weights_mag"], RF.K_ACCUM, report)


def _tail_judge(name, r=None, rgb_loss=True):
    case, r32, r64, env = _tail(name)
    r = r32 if r is None else r
    report = {}
    fails = RF.check_tail(case, r, r64, env, rgb_loss, report) + RF.check_tail_separate(case, r, r64, env, report)
    return fails, report


@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_the_float32_oracle_passes_the_tail_comparators(name):
    case, r32, r64, env = _tail(name)
    fails, report = _tail_judge(name)
    assert not fails, fails
    _note(report, _tail_family)
    assert env["left_out_share"] <= 0.02, env["left_out_share"]  # (float64 alone decides who is left out)
    x = case.spec.double() @ case.M.double()
    for key, (row, side, edge) in case.placed.items():  # the rows put at 10 x the margin are on their side and are compared
        assert not bool(env["edge"][row, 0]) and (float(x[row, 0]) - edge) * side > 0, key
    if case.R >= 15:
        assert len(case.placed) == (6 if case.B > 1 else 4)
        assert float(r64["rgb"].max()) == 1.0 and float(x.min()) < 0 and bool((x[0] == 0).all())
    # without the rgb loss: the spectral half alone
    n32, n64 = RF.tail_oracle(case, torch.float32, rgb_loss=False), RF.tail_oracle(case, torch.float64, rgb_loss=False)
    rep2 = {}
    assert not RF.check_tail(case, n32, n64, RF.tail_envelopes(case, n64, rgb_loss=False), False, rep2)
    _note(rep2, _tail_family)
    print(name, {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})


def test_k_leaves_the_float32_oracle_a_factor_of_four_and_is_at_least_8():
    """K per family = max(8, 4 x the worst float32-oracle ratio, rounded up to a power of two): every family's K is a power of two, at
    least 8, and at least 4 x what the float32 oracle reaches on the committed cases.  (Runs the clean cases it needs.)"""
    for name, c in CASES.items():
        _note(_judge(name)[1])
        if c[0]:
            rep = {}
            _judge_accumulate(_cell(name)[0], _cell(name)[1]["weights"], rep)
            _note(rep, lambda k: "accumulate" if "d_values" not in k else "d_values")
    for name in TAIL_CASES:
        _note(_tail_judge(name)[1], _tail_family)
    have = {"weights": RF.K_WEIGHTS, "per-ray sums": RF.K_SUMS, "d_sigma": RF.K_DSIGMA, "d_values": RF.K_DVALUES, "accumulate": RF.K_ACCUM,
            "rgb": RF.K_RGB,
            "seg_probs": RF.K_PROBS, "losses": RF.K_LOSS, "tail gradients": RF.K_TAILGRAD}
    print({f: round(w, 3) for f, w in WORST.items()}, have)
    assert set(WORST) == set(have)
    for f, k in have.items():
        assert k >= 8 and math.log2(k) == int(math.log2(k)) and 4 * WORST[f] <= k, (f, WORST[f], k)


# ------------------------------------------------------------------------------------------------------------------------------ #
# planted faults
# ------------------------------------------------------------------------------------------------------------------------------ #
def _weights32(case, reset_every=None):
    """The float32 weights again, ray by ray; reset_every: the exclusive optical depth restarts at every such sample (fault 1)."""
    x = case.sigma * (case.t1 - case.t0)
    w = torch.zeros_like(x)
    for s, c in case.packed_info().tolist():
        if c:
            xs = x[s:s + c]
            X = torch.cumsum(xs, 0) - xs
            if reset_every:
                X = X - X[(torch.arange(c) // reset_every) * reset_every]
            w[s:s + c] = (1 - torch.exp(-xs)) * torch.exp(-X)
    return w


def _sums32(case, w, first=0):
    """Per-ray sums of float32 weights; first: only samples from that position of the ray on (fault 6)."""
    ri = case.ray_indices()
    pos = torch.arange(case.n) - case.packed_info()[ri, 0]
    keep = (pos >= first).float()
    return [RF.T.accumulate_along_rays(w * keep, v, ri, case.R) for v in case.values]


def _pairs(streams):
    out, s = [], 0
    while s < len(streams):
        if s + 1 < len(streams) and streams[s] <= 32 and streams[s + 1] <= 32:
            out.append(s)
            s += 2
        else:
            s += 1
    return out


def _fault_cases():
    out = []
    for name, (streams, regime, gs) in CASES.items():
        fs = ["carry", "inclusive_suffix"]
        if gs:
            fs.append("no_scale")
        if _pairs(streams):
            fs.append("halves_swapped")
        if 33 in streams:
            fs.append("band32")
        if streams:
            fs += ["third_chunk_overwrites", "dvalues_last"]
        out += [pytest.param(name, f, id=f"{name}-{f}") for f in fs]
    return out


@pytest.mark.parametrize("name,fault", _fault_cases())
def test_a_planted_compositing_fault_is_rejected(name, fault):
    case, r32, r64, env = _cell(name)
    ri = case.ray_indices()
    mid = (case.t0 + case.t1) / 2
    scale = torch.square(mid).clamp(0, 1) if case.grad_scaling else torch.ones_like(mid)
    fwd, bwd = dict(r32), dict(r32)
    if fault == "carry":
        w = _weights32(case, reset_every=64)
        fwd.update(weights=w, outs=_sums32(case, w), acc=RF.T.accumulate_along_rays(w, None, ri, case.R)[:, 0])
        fails = _judge(name, fwd=fwd)[0]
        assert any(m.startswith("weights") for m in fails) and any(m.startswith("acc") for m in fails), fails
        assert all(any(m.startswith(f"out{i}") for m in fails) for i in range(len(case.streams))), fails
    elif fault == "inclusive_suffix":
        dw = case.d_acc[ri] + RF.dots64(case)
        bwd["d_sigma"] = r32["d_sigma"] - dw * r32["weights"] * (case.t1 - case.t0) * scale
        assert any(m.startswith("d_sigma") for m in _judge(name, bwd=bwd)[0])
    elif fault == "no_scale":
        assert bool((scale < 1).any()) and bool((scale == 1).any())  # the clamp is live
        bwd["d_sigma"] = r32["d_sigma"] / scale.clamp(min=1e-30)
        bwd["d_values"] = [g / scale.clamp(min=1e-30)[:, None] for g in r32["d_values"]]
        fails = _judge(name, bwd=bwd)[0]
        assert any(m.startswith("d_sigma") for m in fails), fails
        assert all(any(m.startswith(f"d_values{i}") for m in fails) for i in range(len(case.streams))), fails
    elif fault == "halves_swapped":
        outs = [o.clone() for o in r32["outs"]]
        for s in _pairs(case.streams):
            m = min(case.streams[s], case.streams[s + 1])
            outs[s][:, :m], outs[s + 1][:, :m] = r32["outs"][s + 1][:, :m], r32["outs"][s][:, :m]
        fwd["outs"] = outs
        fails = _judge(name, fwd=fwd)[0]
        for s in _pairs(case.streams):
            assert any(m.startswith(f"out{s}") for m in fails) and any(m.startswith(f"out{s + 1}") for m in fails), fails
    elif fault == "band32":
        i = case.streams.index(33)
        d_outs = [d.clone() for d in case.d_outs]
        d_outs[i][:, 32] = 0
        bwd["d_sigma"] = RF.composite_oracle(dataclasses.replace(case, d_outs=d_outs), torch.float32)["d_sigma"]
        assert any(m.startswith("d_sigma") for m in _judge(name, bwd=bwd)[0])
    elif fault == "third_chunk_overwrites":
        late = _sums32(case, r32["weights"], first=128)
        long = (case.counts > 128)[:, None]
        fwd["outs"] = [torch.where(long, b, a) for a, b in zip(r32["outs"], late)]
        fails = _judge(name, fwd=fwd)[0]
        assert all(any(m.startswith(f"out{i}") for m in fails) for i in range(len(case.streams))), fails
    elif fault == "dvalues_last":
        pinfo = case.packed_info()
        ragged = pinfo[(pinfo[:, 1] % 64) != 0]
        assert len(ragged)
        dvs = [g.clone() for g in r32["d_values"]]
        for g in dvs:
            g[ragged[:, 0] + ragged[:, 1] - 1, -1] = float("nan")
        bwd["d_values"] = dvs
        fails = _judge(name, bwd=bwd)[0]
        assert all(any(m.startswith(f"d_values{i}") for m in fails) for i in range(len(case.streams))), fails


def _colour_clamp_gradient_passed_above_one(spec, M):
    rgb = torch.matmul(spec, M.to(spec.dtype))
    rgb = torch.where(rgb < 0.0031308, 12.92 * rgb, 1.055 * (rgb.clamp(min=1e-6).pow(1 / 2.4)) - 0.055)
    low = rgb.clamp(min=0)
    return low + (low.clamp(max=1) - low).detach()  # the clamped value, with the gradient of clamp(min=0) alone


def _lookup_eps_on_the_squared_norm(x, alpha, clusters):
    nrm = lambda t: t / torch.sqrt((t * t).sum(1, keepdim=True).clamp(min=1e-12))
    ip = torch.matmul(nrm(x), nrm(clusters).t())
    return ip, torch.softmax(ip * alpha, dim=1)


def _tail_fault_cases():
    out = []
    for name, (R, B, C) in TAIL_CASES.items():
        fs = []
        if R > 16384:
            fs.append("stride_loop")
        if R >= 15:
            fs.append("clamp_gradient")
            if C >= 2:
                fs.append("normalize_eps")
        out += [pytest.param(name, f, id=f"{name}-{f}") for f in fs]
    return out


@pytest.mark.parametrize("name,fault", _tail_fault_cases())
def test_a_planted_tail_fault_is_rejected(name, fault):
    case, r32, r64, env = _tail(name)
    got = dict(r32)
    if fault == "stride_loop":
        head = 16384
        ds = case.spec[:head] - case.gt_spec[:head]
        d = r32["rgb"][:head] + case.bg[:head] * (1 - case.acc[:head, None]) - case.gt_rgb[:head]
        got["losses"] = torch.stack([case.w_spec * (ds * ds).sum() / (case.R * case.B), case.w_rgb * (d * d).sum() / (case.R * 3)])
        stale = r32["d_spec"].clone()
        stale[head:] = 0
        got["d_spec"] = stale
        fails = RF.check_tail(case, got, r64, env)
        assert any(m.startswith("losses") for m in fails) and any(m.startswith("d_spectral") for m in fails), fails
    elif fault == "clamp_gradient":
        bad = RF.tail_oracle(case, torch.float32, colour=_colour_clamp_gradient_passed_above_one)
        assert torch.equal(bad["rgb"], r32["rgb"])  # (the forward is the clean one: the gradients alone must give it away)
        fails = RF.check_tail(case, bad, r64, env) + RF.check_tail_separate(case, bad, r64, env)
        assert any(m.startswith("d_spectral") for m in fails) and any(m.startswith("s2r_d_spec") for m in fails), fails
    elif fault == "normalize_eps":
        bad = RF.tail_oracle(case, torch.float32, lookup=_lookup_eps_on_the_squared_norm)
        fails = RF.check_tail(case, bad, r64, env)
        assert any(m.startswith("seg_probs") for m in fails), fails
