"""Per-ray kernel cases, their float32 / float64 oracle runs and the element-wise comparators (plain helper module, no tests in it).

Used by tests/test_hip_rays_f64.py (csrc/umhs_rays.hip and csrc/umhs_tail.hip on the GPU) and tests/test_rays_f64_bounds_cpu.py (the
comparators pass the float32 oracle and reject planted faults; K is measured there).  It mirrors tests/field_f64.py one stage later.

The oracle is oracle/torch_ref.py as it is (scale_gradients_by_distance_squared, render_weight_from_density, accumulate_along_rays,
render_depth_expected, colour_system, cluster_lookup, blend_background_for_loss, F.mse_loss), run twice on the same float32 inputs:
in float32 (the reference's arithmetic) and in float64 (the truth).  colour_system and cluster_lookup run in float64 unchanged: their
constants are Python floats and F.normalize's epsilon is a double.

ONE RULE for every output element:   |got - ref64| <= K u (mag + tiny),   u = 2^-24.
``mag`` is the float64 sum of the absolute values of the terms that make up the element, times the growth of its exponent's argument;
it is tight where the element is well conditioned and loose only where cancellation is real.  ``tiny`` is ``mag`` with every quantity
that can be subnormal replaced by 2^-126 (one rounding there is 2 u 2^-126 absolute, not relative).  With x = sigma delta, X the
exclusive optical depth, T = exp(-X), alpha = 1 - exp(-x):
  weights        mag_w[n] = T_n (alpha_n (1 + X_n + x_n) + exp(-x_n))      (1 - exp(-x) carries an absolute error u, not a relative one)
  per-ray sums   sum over the ray of mag_w[n] |v[n,k]|   (streams; accumulation: v = 1; depth numerator: v = t_mid); the depth is
                 (mag_num + |depth| mag_acc) / (acc + 1e-10) + |depth|
  d_sigma        delta_n scale_n (DW_n T_{n+1} (1 + X_n + x_n) + sum_{m >= n} DW_m mag_w[m]),   DW_n = |d_acc| + sum_k |d_out[r,k] v[n,k]|
  d_values       scale_n mag_w[n] |d_out[r,k]|;   accumulate_bwd's d_weights: sum_k |d_out[r,k] v[n,k]|
The suffix sum of d_sigma's envelope is INCLUSIVE on purpose.  The oracle's exclusive_sum_packed is cumsum - own, so its backward is
reverse-cumsum - own, and composite_bwd_kernel forms its exclusive suffix sum S the same way, as suf - p.  A sample n whose own term
p_n = dw_n w_n dwarfs everything behind it therefore gets S_n = (p_n + rest) - p_n: the rounding of p_n, about u |p_n|, which can
exceed the true rest and even flip its sign (float32 oracle +1.31e-14 where float64 gives -7.59e-15, behind a sample with x = 23).
The effect is about 1e-10 of the ray's largest gradient and harmless; the inclusive envelope is what says so, element by element: the
error may reach u DW_n mag_w[n] and no more.  A kernel whose suffix were off by a whole sample fails (planted fault 2).

Tail (csrc/umhs_tail.hip), x_k = sum_b s_b M_bk, mag_x = sum_b |s_b M_bk|, y = gamma(x), d = y + beta (1 - acc) - gt:
  rgb            gamma'(x) mag_x + |y|
  d_spectral     |cs| (|s_b| + |gt_b|) + sum_k mag_g[k] |M_bk|,   mag_g = |cr| (gamma' mag_d + |d| |gamma''| mag_x) + |g|,
                 mag_d = mag_rgb + |beta| (1 + |acc|) + |gt|;  d_accumulation: sum_k |cr| mag_d |beta_k| + |d_acc|
  losses         scale (1 + log2 R) sum (d^2 + 2 |d| mag_d'): the sum of squared differences times the growth of the summation tree,
                 plus what d's own envelope contributes (mag_d' = 0 for the spectral loss, whose d = s - gt is one exact-rounded
                 subtraction of inputs; the rgb d is a three-term sum, in the fused tail of a computed rgb)
  seg_probs      p_c (|alpha| (mag_cos[c] + sum_j p_j mag_cos[j]) + 2),   mag_cos = sum_b |s_b E_cb| / (|s| |E_c|) + 2 |cos|
  depth clip, seg_raw, seg_pred, tmid_minmax, pack_info: exact.
Edges.  A float32 evaluation may legitimately take the other branch of the gamma knee (x = 0.0031308), of the clamp (x = 0 with
x != 0 representable on both sides; x = 1, where gamma(1) = 1) or of the argmax when the float64 value is within EDGE = 64 u of the
edge relative to its own envelope.  Such an element's forward value is compared against either branch; its ray is left out of the
gradient comparison; a tied ray may report either tied class.  The case builder places rows at 10 x that margin on each side of every
edge, and at most 2 % of a case may be left out (asserted on the float64 run alone, tests/test_rays_f64_bounds_cpu.py).

K per output family = max(8, 4 x the float32 CPU oracle's worst ratio over the committed cases, rounded up to a power of two): the
floor of 8 allows for device expf / powf being a couple of ulp where torch's are nearly correctly rounded and for the wave scans'
association, the factor 4 is the margin over a float32 evaluation in another order.  Measured on the CPU (float32 oracle, worst
|diff| / (u (mag + tiny)) over all cases; tests/test_rays_f64_bounds_cpu.py re-measures and asserts 4 x worst <= K):
  weights 1.60 | per-ray sums 2.58 | d_sigma 0.96 | d_values 1.62 | accumulate 14.8 | rgb 3.13 | seg_probs 1.05 | losses 0.38 |
  tail gradients 3.57
so K = 8 for weights, d_sigma, d_values, seg_probs and the losses, and K = 16 for the per-ray sums (a 1000-sample index_add_ of terms
of both signs), rgb and the tail's gradients (141-band dot products through gamma'), and K = 64 for accumulate_fwd's sums and
accumulate_bwd's d_weights: their weights are an input, so the envelope is the bare sum of |w v| with none of the transmittance's slack
in it, and a float32 sum of 1000 terms of both signs in sample order is 14.8 u of it away from float64.
tests/test_hip_rays_f64.py writes the kernels' own worst ratios per family, case and output to rays_f64.json in ``report_dir()``, the
run-output directory that .gitignore keeps out of history, next to default_batch_36864.json.

Teeth: the share of elements with |ref64| > 16 x bound -- there a missing or misplaced term must show.  Condition: in every thin
case at least 90 % of d_sigma, and of every stream's per-ray sums over non-empty rays, has teeth.  Opaque and wall cases carry no such
condition for d_sigma (behind a saturated sample the gradient is pure cancellation); they are there for the forward and the envelope.

Which case selects which path of the two compositing kernels (streams | regime | grad scaling):
  [31, 3]  thin on        forward: one pair, K < 32 in both halves; backward: LDS tile at strides 31 and 3; d_values null on stream 1
  [32, 32] thin on        forward: two streams sharing the wave with a full half; backward: LDS tile at stride 33 from K = 32
  [33, 3]  thin off       forward: K = 33 is no pair, so [33] alone then [3] alone; backward: 32-band slice walk with kw = 1
                          (band 32), grad_scaling = 0
  [5, 141, 7, 2] thin on  forward: pairing depends on position (5|141 no pair, 141 alone in three kc rounds, then 7|2 paired);
                          backward: strides 5, 7, 3 (K = 2), five slices of K = 141 with kw = 13; d_values wide path at 141
  [64]     opaque on      forward: kc loop exactly one round, every lane live; backward: two full slices
  [65]     wall on        forward: kc loop's second round with one live lane; backward: kw = 1 slice; d_values wide path just past 64
  [128, 1] zero on        forward: K = 128 two full rounds, then [1] alone; backward: four slices, LDS tile at stride 1
  [1]      opaque off     forward: one stream, one live lane; backward: stride 1, grad_scaling = 0
  []       opaque on      weights, accumulation and depth only; backward from d_acc alone (d_sigma = d_acc delta T_end there: the
                          kernel's dw T_next - S cancels down to it by nature, so no thin case -- with its teeth condition -- is stream-less)
  [32, 32] zero off       the pair again with zero-density rays
Every case's rays hold 0-256 samples on both sides of the 16- and 64-sample boundaries (the 16- and 8-sample unrolled blocks with a
scalar tail on a later chunk: 127 = 64 + 3 x 16 + 8 + 7; the read-modify-write of a third and later chunk: 129, 200, 256, 1000), a
run of ten empty rays across two whole 4-ray workgroups, one ray of 1000 samples, and end in an empty ray.  umhs_composite_bwd_dots,
accumulate_fwd / accumulate_bwd run on every case in tests/test_hip_rays_f64.py."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import torch_ref as T

U = 2.0 ** -24
TINY = 2.0 ** -126
EDGE = 64 * U
TEETH = 16.0
K_WEIGHTS = K_DSIGMA = K_DVALUES = K_LOSS = K_PROBS = 8.0
K_SUMS = K_RGB = K_TAILGRAD = 16.0
K_ACCUM = 64.0  # accumulate_fwd's sums and accumulate_bwd's d_weights: plain sums whose envelope has no transmittance slack in it
KNEE = 0.0031308

RAY_COUNTS = (0, 1, 2, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 0, 256, 1, 0) + (0,) * 9 + (1000, 3, 0)
REGIMES = {"thin": (2.0, 1.5), "opaque": (6.5, 1.5), "wall": (9.0, 0.5), "zero": (2.0, 1.5)}
# (streams, regime, grad_scaling)
COMPOSITE_CASES = [
    ([31, 3], "thin", True), ([32, 32], "thin", True), ([33, 3], "thin", False), ([5, 141, 7, 2], "thin", True), ([64], "opaque", True),
    ([65], "wall", True), ([128, 1], "zero", True), ([1], "opaque", False), ([], "opaque", True), ([32, 32], "zero", False),
]


def report_dir(root: str) -> str:
    """The run-output directory the GPU tests leave their figures in: the first ``*_out/`` entry of the repository's .gitignore."""
    with open(os.path.join(root, ".gitignore")) as f:
        name = next(ln.strip() for ln in f if ln.strip().endswith("_out/") and not ln.startswith(("#", "/")))
    d = os.path.join(root, name.rstrip("/"))
    os.makedirs(d, exist_ok=True)
    return d


def case_id(c) -> str:
    return f"{'_'.join(map(str, c[0])) or 'none'}-{c[1]}-{'gs' if c[2] else 'nogs'}"


# ------------------------------------------------------------------------------------------------------------------------------ #
# compositing: cases and oracle
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class RayCase:
    streams: List[int]
    regime: str
    grad_scaling: bool
    counts: torch.Tensor  # [R] int64
    sigma: torch.Tensor  # [n]
    t0: torch.Tensor
    t1: torch.Tensor
    values: List[torch.Tensor]  # [n,K] per stream
    d_outs: List[torch.Tensor]  # [R,K] per stream
    d_acc: torch.Tensor  # [R]
    want: List[bool]  # d_values pointer non-null

    @property
    def R(self) -> int:
        return self.counts.numel()

    @property
    def n(self) -> int:
        return int(self.counts.sum())

    def packed_info(self) -> torch.Tensor:
        return torch.stack([torch.cumsum(self.counts, 0) - self.counts, self.counts], 1).contiguous()

    def ray_indices(self) -> torch.Tensor:
        return torch.repeat_interleave(torch.arange(self.R), self.counts)


def make_ray_case(streams: Sequence[int], regime: str, grad_scaling: bool, seed: int = 0) -> RayCase:
    """Values and cotangents of mixed sign, mid-points on both sides of 1 (the clamp of the gradient scale is live), steps of about
    0.0035 as in oracle.synthetic_batch, sigma = exp(N(mu, sd)) of the regime; "zero": every third non-empty ray and a tenth of the other
    samples have sigma = 0."""
    g = torch.Generator().manual_seed(7000 + seed)
    counts = torch.tensor(RAY_COUNTS, dtype=torch.int64)
    R, n = counts.numel(), int(counts.sum())
    ri = torch.repeat_interleave(torch.arange(R), counts)
    near = 0.05 + 1.55 * torch.rand(R, generator=g)
    delta = 0.0035 * (0.5 + torch.rand(n, generator=g))
    start = torch.cumsum(counts, 0) - counts
    cum = torch.cumsum(delta.double(), 0)
    t0 = (near.double()[ri] + (cum - delta.double()) - (cum - delta.double())[start[ri]]).float()
    t1 = t0 + delta
    mu, sd = REGIMES[regime]
    sigma = torch.exp(torch.randn(n, generator=g) * sd + mu)
    if regime == "zero":
        live = torch.nonzero(counts > 0)[:, 0]
        dead = torch.zeros(R, dtype=torch.bool)
        dead[live[::3]] = True
        sigma[dead[ri] | (torch.rand(n, generator=g) < 0.1)] = 0.0
    values = [torch.randn(n, k, generator=g) for k in streams]
    d_outs = [torch.randn(R, k, generator=g) for k in streams]
    d_acc = torch.randn(R, generator=g)
    want = [True, True, False, True][: len(streams)] if len(streams) == 4 else [i % 2 == 0 for i in range(len(streams))]
    return RayCase(list(streams), regime, bool(grad_scaling), counts, sigma, t0, t1, values, d_outs, d_acc, want)


def composite_oracle(case: RayCase, dtype) -> Dict:
    """weights, per-ray sums, accumulation, unclipped expected depth, and the gradients of  sum_s sum(out_s d_out_s) + sum(acc d_acc)
    w.r.t. sigma and every stream's values (with grad_scaling: scale_gradients_by_distance_squared in front)."""
    cv = lambda t: t.to(dtype)
    sigma = cv(case.sigma).clone().requires_grad_()
    vals = [cv(v).clone().requires_grad_() for v in case.values]
    t0, t1 = cv(case.t0), cv(case.t1)
    fo = {"density": sigma[:, None], **{f"v{i}": v for i, v in enumerate(vals)}}
    if case.grad_scaling:
        fo = T.scale_gradients_by_distance_squared(fo, t0[:, None], t1[:, None])
    pinfo, ri = case.packed_info(), case.ray_indices()
    w = T.render_weight_from_density(t0, t1, fo["density"][:, 0], pinfo)[0]
    outs = [T.accumulate_along_rays(w, fo[f"v{i}"], ri, case.R) for i in range(len(vals))]
    acc = T.accumulate_along_rays(w, None, ri, case.R)
    inf = float("inf")
    depth = T.render_depth_expected(w[:, None], t0[:, None], t1[:, None], ri, case.R, clip_range=(-inf, inf))
    loss = (acc[:, 0] * cv(case.d_acc)).sum()
    for o, d in zip(outs, case.d_outs):
        loss = loss + (o * cv(d)).sum()
    g = torch.autograd.grad(loss, [sigma] + vals)
    return {"weights": w.detach(), "outs": [o.detach() for o in outs], "acc": acc[:, 0].detach(), "depth": depth[:, 0].detach(),
            "d_sigma": g[0], "d_values": list(g[1:])}


def composite_envelopes(case: RayCase, r64: Dict) -> Dict:
    """``mag + tiny`` of every compositing output (module docstring), float64, ray by ray (no cancellation across rays)."""
    f = lambda t: t.double()
    x = f(case.sigma) * (f(case.t1) - f(case.t0))
    delta = f(case.t1) - f(case.t0)
    mid = (f(case.t0) + f(case.t1)) / 2
    scale = torch.square(mid).clamp(0, 1) if case.grad_scaling else torch.ones_like(mid)
    n, R = case.n, case.R
    ri = case.ray_indices()
    dw_abs = f(case.d_acc).abs()[ri]
    dots_abs = torch.zeros(n, dtype=torch.float64)
    for v, d in zip(case.values, case.d_outs):
        dots_abs += (f(d)[ri] * f(v)).abs().sum(1)
    dw_abs = dw_abs + dots_abs
    mag_w, tiny_w, mag_ds = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for s, c in case.packed_info().tolist():
        if c == 0:
            continue
        sl = slice(s, s + c)
        xs = x[sl]
        X = torch.cumsum(xs, 0) - xs
        Tn, ex = torch.exp(-X), torch.exp(-xs)
        grow = 1 + X + xs
        mw = Tn * (-torch.expm1(-xs) * grow + ex)
        mag_w[sl], tiny_w[sl] = mw, 2 * TINY
        z = dw_abs[sl] * (mw + 2 * TINY)
        suf = torch.flip(torch.cumsum(torch.flip(z, [0]), 0), [0])  # inclusive
        mag_ds[sl] = delta[sl] * scale[sl] * (dw_abs[sl] * (Tn * ex * grow + TINY) + suf) + TINY
    mw = mag_w + tiny_w
    seg = lambda t: torch.zeros((R,) + tuple(t.shape[1:]), dtype=torch.float64).index_add_(0, ri, t)
    env = {"weights": mw, "d_sigma": mag_ds, "d_weights": dots_abs + TINY}
    env["outs"] = [seg(mw[:, None] * f(v).abs()) + TINY for v in case.values]
    env["acc"] = seg(mw) + TINY
    num = seg(mw * mid.abs())
    depth, acc = r64["depth"].double(), r64["acc"].double()
    env["depth"] = (num + depth.abs() * env["acc"]) / (acc + 1e-10) + depth.abs() + TINY
    env["d_values"] = [(scale * mw)[:, None] * f(d).abs()[ri] + TINY for d in case.d_outs]
    return env


def accumulate_reference(case: RayCase, weights32: torch.Tensor) -> Dict:
    """accumulate_fwd / accumulate_bwd on given float32 weights (the forward's own): float64 results and their envelopes."""
    w = weights32.detach().double().cpu()
    ri, R = case.ray_indices(), case.R
    seg = lambda t: torch.zeros((R,) + tuple(t.shape[1:]), dtype=torch.float64).index_add_(0, ri, t)
    out = {"outs": [], "outs_mag": [], "d_values": [], "d_values_mag": []}
    dwt = torch.zeros(case.n, dtype=torch.float64)
    dwt_mag = torch.zeros(case.n, dtype=torch.float64)
    for v, d in zip(case.values, case.d_outs):
        v, d = v.double(), d.double()
        out["outs"].append(T.accumulate_along_rays(w, v, ri, R))
        out["outs_mag"].append(seg((w[:, None] * v).abs()) + TINY)
        out["d_values"].append(w[:, None] * d[ri])
        out["d_values_mag"].append((w[:, None] * d[ri]).abs() + TINY)
        dwt += (d[ri] * v).sum(1)
        dwt_mag += (d[ri] * v).abs().sum(1)
    out["d_weights"], out["d_weights_mag"] = dwt, dwt_mag + TINY
    return out


def dots64(case: RayCase) -> torch.Tensor:
    """umhs_composite_bwd_dots's input: sum over streams and bands of d_out[ray(n)][k] value[n][k], formed in float64, rounded once."""
    ri = case.ray_indices()
    d = torch.zeros(case.n, dtype=torch.float64)
    for v, do in zip(case.values, case.d_outs):
        d += (do.double()[ri] * v.double()).sum(1)
    return d.float()


# ------------------------------------------------------------------------------------------------------------------------------ #
# the comparator
# ------------------------------------------------------------------------------------------------------------------------------ #
def check(name: str, got, ref64, mag, K: float, report: Optional[Dict] = None, alt=None, skip=None, teeth_mask=None) -> List[str]:
    """|got - ref64| <= K u mag for every element (``mag`` includes its tiny term).  ``alt``: a second legitimate value per element
    (NaN where there is none); ``skip``: elements left out (bool); ``teeth_mask``: the elements the teeth share is taken over.
    report[name] = {"worst": max |diff| / (u mag), "teeth": share with |ref64| > 16 K u mag, "n": elements compared}."""
    got, ref, mag = got.detach().double().cpu(), ref64.detach().double().cpu(), mag.detach().double().cpu()
    if got.shape != ref.shape:
        return [f"{name}: shape {tuple(got.shape)}, want {tuple(ref.shape)}"]
    keep = torch.ones_like(ref, dtype=torch.bool) if skip is None else ~skip.cpu().expand_as(ref)
    if ref.numel() == 0 or not bool(keep.any()):
        if report is not None:
            report[name] = {"worst": 0.0, "teeth": None, "n": 0}
        return []
    d = (got - ref).abs()
    if alt is not None:
        a = alt.detach().double().cpu()
        d = torch.where(torch.isnan(a), d, torch.minimum(d, (got - a).abs()))
    ratio = torch.where(d == 0, torch.zeros_like(d), d / (U * mag))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max())
    tm = keep if teeth_mask is None else keep & teeth_mask.cpu().expand_as(ref)
    teeth = float(((ref.abs() > TEETH * K * U * mag) & tm).sum()) / max(1, int(tm.sum())) if bool(tm.any()) else None
    if report is not None:
        report[name] = {"worst": worst, "teeth": teeth, "n": int(keep.sum())}
    if worst > K:
        i = int(ratio.reshape(-1).argmax())
        return [f"{name}: element {i}: {float(got.reshape(-1)[i]):.9g} vs float64 {float(ref.reshape(-1)[i]):.9g} = {worst:.3g} u mag "
                f"(mag {float(mag.reshape(-1)[i]):.3g}, K = {K:g}; {int((ratio > K).sum())} of {int(keep.sum())} over)"]
    return []


def check_composite_forward(case: RayCase, got: Dict, r64: Dict, env: Dict, report=None) -> List[str]:
    """got: weights [n], outs [[R,K]], acc [R], depth [R]."""
    live = case.counts > 0
    fails = check("weights", got["weights"], r64["weights"], env["weights"], K_WEIGHTS, report)
    for i, o in enumerate(got["outs"]):
        fails += check(f"out{i}", o, r64["outs"][i], env["outs"][i], K_SUMS, report, teeth_mask=live[:, None])
    fails += check("acc", got["acc"], r64["acc"], env["acc"], K_SUMS, report, teeth_mask=live)
    fails += check("depth", got["depth"], r64["depth"], env["depth"], K_SUMS, report, teeth_mask=live)
    return fails


def check_composite_backward(case: RayCase, got: Dict, r64: Dict, env: Dict, report=None, prefix="") -> List[str]:
    """got: d_sigma [n], d_values [[n,K] | None] (None: not asked for, or the pointer was null)."""
    fails = check(prefix + "d_sigma", got["d_sigma"], r64["d_sigma"], env["d_sigma"], K_DSIGMA, report)
    for i, dv in enumerate(got.get("d_values", [])):
        if dv is not None:
            fails += check(f"{prefix}d_values{i}", dv, r64["d_values"][i], env["d_values"][i], K_DVALUES, report)
    return fails


def teeth_failures(case: RayCase, report: Dict, min_share: float = 0.9) -> List[str]:
    """The condition on thin cases: at least 90 % of d_sigma and of every stream's per-ray sums (non-empty rays) has teeth."""
    if case.regime != "thin":
        return []
    keys = ["d_sigma"] + [f"out{i}" for i in range(len(case.streams))]
    return [f"{k}: only {report[k]['teeth']:.3f} of the elements has teeth" for k in keys
            if k in report and report[k]["teeth"] is not None and report[k]["teeth"] < min_share]


# ------------------------------------------------------------------------------------------------------------------------------ #
# tail: cases, oracle, envelopes
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class TailCase:
    R: int
    B: int
    C: int
    spec: torch.Tensor  # [R,B]
    M: torch.Tensor  # [B,3]
    E: torch.Tensor  # [C,B]
    acc: torch.Tensor  # [R]
    depth: torch.Tensor  # [R]
    tm0: torch.Tensor  # sample starts / ends whose mid-points give the clip range
    tm1: torch.Tensor
    colors: torch.Tensor  # [C,3]
    gt_spec: torch.Tensor
    gt_rgb: torch.Tensor
    bg: torch.Tensor
    rgb_in: torch.Tensor  # [R,3]: loss_fwd / loss_bwd's rgb input (the float32 oracle's)
    cot_rgb: torch.Tensor  # [R,3]: spec2rgb_bwd's upstream gradient
    prev: torch.Tensor  # [R,B]: what spec2rgb_bwd(accumulate) adds to
    alpha: float = 0.7
    w_spec: float = 5.0
    w_rgb: float = 0.7
    g_up: tuple = (2.0, 3.0)
    placed: Dict = field(default_factory=dict)  # name -> (row, expected float64 predicate on x[row, 0])


def _gamma_parts(x: torch.Tensor):
    """float64: (gamma'(x), |gamma''(x)|) of the unclamped curve on x's own branch."""
    low = x < KNEE
    xc = x.clamp(min=KNEE)
    g1 = torch.where(low, torch.full_like(x, 12.92), 1.055 / 2.4 * xc.pow(1 / 2.4 - 1))
    g2 = torch.where(low, torch.zeros_like(x), 1.055 / 2.4 * abs(1 / 2.4 - 1) * xc.pow(1 / 2.4 - 2))
    return g1, g2


def make_tail_case(R: int, B: int, C: int, seed: int = 0) -> TailCase:
    """Spectra in [-0.1, 1.1); from R >= 15 on: a zero row, a negative row (x < 0), rows scaled into the linear branch, rows of norm
    1e-8 and 1e-14 (F.normalize's epsilon), a bright row (rgb above 1), and rows placed at 10 x EDGE on each side of the knee, of
    x = 1 and of x = 0 in channel 0."""
    g = torch.Generator().manual_seed(9000 + 131 * R + 17 * B + C + seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    spec = rnd(R, B) * 1.2 - 0.1
    M = (rnd(B, 3) - 0.15) * (2.6 / B)
    M[int(torch.randint(B, (1,), generator=g)), 0] += 0.5 / B  # (channel 0 has a dominant band to place x = 0 with)
    placed = {}
    if R >= 15:
        spec[0] = 0
        spec[1] = -rnd(B)
        spec[2] *= 1e-3
        spec[3] *= 1e-8
        spec[4] *= 1e-14
        spec[5] = rnd(B) * 3 + 0.5
        m0 = M[:, 0].double()
        row = 6
        for name, edge in (("knee", KNEE), ("one", 1.0)):
            for side in (-1, 1):
                s = (rnd(B) + 0.2).double()
                xb, mb = float(s @ m0), float(s.abs() @ m0.abs())
                extra = 3.0 if name == "one" else 0.0
                fct = (edge + side * 10 * EDGE * extra) / (xb - side * 10 * EDGE * mb)
                spec[row] = (s * fct).float()
                placed[f"{name}{'+' if side > 0 else '-'}"] = (row, side, edge)
                row += 1
        if B > 1:
            j = int(m0.abs().argmax())
            for side in (-1, 1):
                s = (rnd(B) + 0.2).double()
                s[j] = 0
                rest, mb = float(s @ m0), float(s.abs() @ m0.abs())
                # x = rest + s_j m_j = side * 10 EDGE (mb + |s_j m_j|): solve with |s_j m_j| ~ |rest| (rest > 0, so s_j m_j < 0)
                t = side * 10 * EDGE * (mb + abs(rest))
                s[j] = (t - rest) / float(m0[j])
                spec[row] = s.float()
                placed[f"zero{'+' if side > 0 else '-'}"] = (row, side, 0.0)
                row += 1
    E = rnd(C, B)
    acc, depth = rnd(R), rnd(R) * 5
    tm0 = rnd(97) * 4 + 0.05
    tm1 = tm0 + 0.1
    colors, gt_spec, gt_rgb, bg = rnd(C, 3), rnd(R, B), rnd(R, 3), rnd(R, 3)
    cot_rgb, prev = rnd(R, 3) - 0.5, rnd(R, B) - 0.5
    rgb_in = T.colour_system(spec, M)
    return TailCase(R, B, C, spec, M, E, acc, depth, tm0, tm1, colors, gt_spec, gt_rgb, bg, rgb_in, cot_rgb, prev, placed=placed)


def tail_oracle(case: TailCase, dtype, rgb_loss: bool = True, colour=None, lookup=None) -> Dict:
    """Everything csrc/umhs_tail.hip computes, from oracle/torch_ref.py (``colour`` / ``lookup``: replacements that plant a fault):
    the fused tail (unit upstream gradients), spec2rgb_bwd on cot_rgb (plain and accumulated onto ``prev``), and loss_fwd / loss_bwd on
    the given rgb input with upstream gradients g_up."""
    colour = T.colour_system if colour is None else colour
    lookup = T.cluster_lookup if lookup is None else lookup
    cv = lambda t: t.to(dtype)
    spec = cv(case.spec).clone().requires_grad_()
    acc = cv(case.acc)[:, None].clone().requires_grad_()
    M = cv(case.M)
    rgb = colour(spec, M)
    ip, probs = lookup(spec.detach(), case.alpha, cv(case.E))
    arg = ip.argmax(1)
    on = (case.acc > 0.5).to(dtype)
    mids = (case.tm0 + case.tm1) / 2  # float32 on purpose: the clip range is the float32 kernel's, exactly
    o = {"x": (spec.detach() @ M), "rgb": rgb.detach(), "cos": ip, "probs": probs, "arg": arg, "seg_raw": arg.to(dtype) * on,
         "seg_pred": cv(case.colors)[arg] * on[:, None], "dclip": torch.clip(case.depth, mids.min(), mids.max())}
    l_s = case.w_spec * F.mse_loss(spec, cv(case.gt_spec))
    if rgb_loss:
        pred, gt = T.blend_background_for_loss(rgb, acc, cv(case.gt_rgb), cv(case.bg))
        l_r = case.w_rgb * F.mse_loss(pred, gt)
        gs, ga = torch.autograd.grad(l_s + l_r, [spec, acc], retain_graph=True)
        o["losses"], o["d_spec"], o["d_acc"] = torch.stack([l_s, l_r]).detach(), gs, ga[:, 0]
    else:
        (gs,) = torch.autograd.grad(l_s, [spec], retain_graph=True)
        o["losses"], o["d_spec"], o["d_acc"] = torch.stack([l_s, torch.zeros_like(l_s)]).detach(), gs, None
    (o["s2r_d_spec"],) = torch.autograd.grad((rgb * cv(case.cot_rgb)).sum(), [spec])
    o["s2r_d_spec_acc"] = o["s2r_d_spec"] + cv(case.prev)
    # the separate loss kernels: rgb is an input
    s2 = cv(case.spec).clone().requires_grad_()
    r2 = cv(case.rgb_in).clone().requires_grad_()
    a2 = cv(case.acc)[:, None].clone().requires_grad_()
    l_s2 = case.w_spec * F.mse_loss(s2, cv(case.gt_spec))
    pred, gt = T.blend_background_for_loss(r2, a2, cv(case.gt_rgb), cv(case.bg))
    l_r2 = case.w_rgb * F.mse_loss(pred, gt)
    g = torch.autograd.grad(case.g_up[0] * l_s2 + case.g_up[1] * l_r2, [s2, r2, a2])
    o["sep_losses"] = torch.stack([l_s2, l_r2]).detach()
    o["sep_d_spec"], o["sep_d_rgb"], o["sep_d_acc"] = g[0], g[1], g[2][:, 0]
    (o["sep_d_spec_only"],) = torch.autograd.grad(case.g_up[0] * case.w_spec * F.mse_loss(s2, cv(case.gt_spec)), [s2])
    return o


def cluster_ties(spec: torch.Tensor, E: torch.Tensor):
    """float64 (cos [R,C], mag_cos [R,C], tied [R,C]) of ClusterLookup on float32 inputs: ``tied`` marks the classes whose cosine is
    within EDGE x (its envelope + the best's) of the best -- any of them is a legitimate float32 argmax.  A ray has a tie when more
    than one class is marked (an all-zero spectrum has none: every cosine is exactly zero in any arithmetic, and the first wins)."""
    s, e = spec.detach().double().cpu(), E.detach().double().cpu()
    cos = T.cluster_lookup(s, 1.0, e)[0]
    ns, ne = s.norm(dim=1).clamp(min=1e-12), e.norm(dim=1).clamp(min=1e-12)
    mag_cos = (s.abs() @ e.abs().T) / (ns[:, None] * ne[None, :]) + 2 * cos.abs()
    best = cos.argmax(1, keepdim=True)
    tied = (cos.gather(1, best) - cos) < EDGE * (mag_cos + mag_cos.gather(1, best))
    tied.scatter_(1, best, True)
    return cos, mag_cos, tied


def tail_envelopes(case: TailCase, r64: Dict, rgb_loss: bool = True) -> Dict:
    """``mag + tiny`` of every tail output, the edge / tie sets and the alternative forward values (module docstring).  float64."""
    f = lambda t: t.double()
    s, M, E = f(case.spec), f(case.M), f(case.E)
    R, B, C = case.R, case.B, case.C
    x = s @ M
    mag_x = s.abs() @ M.abs()
    g1, g2 = _gamma_parts(x)
    y_raw = torch.where(x < KNEE, 12.92 * x, 1.055 * x.clamp(min=1e-6).pow(1 / 2.4) - 0.055)
    y = y_raw.clamp(0, 1)
    near_knee = (x - KNEE).abs() <= EDGE * mag_x
    near_zero = (x.abs() <= EDGE * mag_x) & (mag_x > 0) & (x != 0)
    near_one = (x - 1).abs() <= EDGE * (mag_x + 3)
    edge = near_knee | near_zero | near_one
    other = torch.where(x < KNEE, 1.055 * x.clamp(min=1e-6).pow(1 / 2.4) - 0.055, 12.92 * x).clamp(0, 1)
    env = {"edge": edge, "edge_rows": edge.any(1), "rgb_alt": torch.where(near_knee, other, torch.full_like(x, float("nan")))}
    passes = ((y_raw >= 0) & (y_raw <= 1)).double()
    mag_rgb = g1 * mag_x + y.abs() + TINY
    env["rgb"] = mag_rgb
    # cluster probe
    cos, mag_cos, tied = cluster_ties(case.spec, case.E)
    p = r64["probs"].double()
    env["probs"] = p * (abs(case.alpha) * (mag_cos + (p * mag_cos).sum(1, keepdim=True)) + 2) + TINY
    env["tied_classes"] = tied
    env["tie_rows"] = tied.sum(1) > 1
    # losses and gradients of the fused tail (unit upstream gradients)
    cs = case.w_spec * 2.0 / (R * B)
    cr = case.w_rgb * 2.0 / (R * 3)
    ds = s - f(case.gt_spec)
    grow = 1 + math.log2(R)
    mag_ls = case.w_spec / (R * B) * grow * (ds * ds).sum()
    beta, accv, gt = f(case.bg), f(case.acc)[:, None], f(case.gt_rgb)

    def rgb_terms(rgb, mag_of_rgb):
        d = rgb + beta * (1 - accv) - gt
        mag_d = mag_of_rgb + beta.abs() * (1 + accv.abs()) + gt.abs()
        return d, mag_d

    d, mag_d = rgb_terms(y, mag_rgb)
    mag_lr = case.w_rgb / (R * 3) * grow * (d * d + 2 * d.abs() * mag_d).sum()
    env["losses"] = torch.stack([mag_ls, mag_lr if rgb_loss else torch.zeros((), dtype=torch.float64)]) + TINY
    gk = cr * d * g1 * passes
    mag_g = (abs(cr) * (g1 * mag_d + d.abs() * g2 * mag_x) * passes + gk.abs()) if rgb_loss else torch.zeros_like(x)
    env["d_spec"] = abs(cs) * (s.abs() + f(case.gt_spec).abs()) + mag_g @ M.abs().T + TINY
    env["d_acc"] = (abs(cr) * mag_d * beta.abs()).sum(1) + (r64["d_acc"].double().abs() if rgb_loss else 0) + TINY
    # spec2rgb_bwd alone
    cot = f(case.cot_rgb)
    mag_g2 = cot.abs() * (g2 * mag_x + g1) * passes
    env["s2r_d_spec"] = mag_g2 @ M.abs().T + TINY
    env["s2r_d_spec_acc"] = env["s2r_d_spec"] + f(case.prev).abs()
    # the separate loss kernels on the rgb input
    gu = case.g_up
    d2, mag_d2 = rgb_terms(f(case.rgb_in), f(case.rgb_in).abs())
    env["sep_losses"] = torch.stack([mag_ls, case.w_rgb / (R * 3) * grow * (d2 * d2 + 2 * d2.abs() * mag_d2).sum()]) + TINY
    env["sep_d_spec"] = abs(cs * gu[0]) * (s.abs() + f(case.gt_spec).abs()) + TINY
    env["sep_d_rgb"] = abs(cr * gu[1]) * mag_d2 + TINY
    env["sep_d_acc"] = (abs(cr * gu[1]) * mag_d2 * beta.abs()).sum(1) + TINY
    n_left = int(env["edge_rows"].sum()) + int(env["tie_rows"].sum())
    env["left_out_share"] = n_left / max(1, R)
    return env


def check_seg(name: str, got_raw, got_pred, case: TailCase, r64: Dict, env: Dict) -> List[str]:
    """seg_raw / seg_pred exact outside the tie set; inside it any of the tied classes.  A ray with acc <= 0.5 reports class 0 and a
    zero colour; seg_pred is the colour of the class seg_raw reports, bit for bit."""
    raw, pred = got_raw.detach().double().cpu().reshape(-1), got_pred.detach().double().cpu().reshape(-1, 3)
    on = case.acc > 0.5
    idx = torch.nan_to_num(raw, nan=-1.0).long().clamp(0, case.C - 1)
    is_class = raw == idx.double()
    allowed = torch.where(env["tie_rows"], env["tied_classes"].gather(1, idx[:, None])[:, 0], idx == r64["arg"])
    bad = torch.where(on, ~(is_class & allowed), raw != 0)
    fails = []
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        fails.append(f"{name}seg_raw: ray {i}: {float(raw[i])} vs {float(r64['seg_raw'][i])} ({int(bad.sum())} rays; tie: "
                     f"{bool(env['tie_rows'][i])})")
    want = case.colors.double()[idx] * on.double()[:, None]
    badp = ~(pred == want).all(1)
    if bool(badp.any()):
        i = int(torch.nonzero(badp)[0])
        fails.append(f"{name}seg_pred: ray {i}: {pred[i].tolist()} is not the colour of class {int(idx[i])} x [acc > 0.5] ({int(badp.sum())} rays)")
    return fails


def check_tail(case: TailCase, got: Dict, r64: Dict, env: Dict, rgb_loss: bool = True, report=None, prefix="") -> List[str]:
    """got: any of rgb, dclip, probs, seg_raw + seg_pred, losses, d_spec, d_acc (the fused tail's or the epilogue's names)."""
    fails = []
    rows = env["edge_rows"]
    if "rgb" in got:
        fails += check(prefix + "rgb", got["rgb"], r64["rgb"], env["rgb"], K_RGB, report, alt=env["rgb_alt"])
    if "dclip" in got:
        if not torch.equal(got["dclip"].detach().cpu().reshape(-1), r64["dclip"].reshape(-1).float()):
            fails.append(prefix + "depth clip differs from torch.clip on the float32 mid-point range")
    if "probs" in got:
        fails += check(prefix + "seg_probs", got["probs"], r64["probs"], env["probs"], K_PROBS, report)
    if "seg_raw" in got:
        fails += check_seg(prefix, got["seg_raw"], got["seg_pred"], case, r64, env)
    if "losses" in got:
        m = 2 if rgb_loss else 1
        fails += check(prefix + "losses", got["losses"][:m], r64["losses"][:m], env["losses"][:m], K_LOSS, report)
        if not rgb_loss and float(got["losses"][1]) != 0.0:
            fails.append(prefix + "losses[1] must be zero without the rgb loss")
    if "d_spec" in got:
        fails += check(prefix + "d_spectral", got["d_spec"], r64["d_spec"], env["d_spec"], K_TAILGRAD, report,
                       skip=rows[:, None] if rgb_loss else None)
    if got.get("d_acc") is not None:
        fails += check(prefix + "d_accumulation", got["d_acc"], r64["d_acc"], env["d_acc"], K_TAILGRAD, report)
    return fails


def check_tail_separate(case: TailCase, got: Dict, r64: Dict, env: Dict, report=None, prefix="") -> List[str]:
    """got: any of s2r_d_spec, s2r_d_spec_acc (spec2rgb_bwd plain / accumulated), sep_losses, sep_d_spec, sep_d_rgb, sep_d_acc
    (loss_fwd / loss_bwd on the rgb input with upstream gradients g_up), sep_d_spec_only (loss_bwd without the rgb half)."""
    fails = []
    rows = env["edge_rows"][:, None]
    for k in ("s2r_d_spec", "s2r_d_spec_acc"):
        if k in got:
            fails += check(prefix + k, got[k], r64[k], env[k], K_TAILGRAD, report, skip=rows)
    for k in ("sep_losses", "sep_d_spec", "sep_d_rgb", "sep_d_acc"):
        if k in got:
            fails += check(prefix + k, got[k], r64[k], env[k], K_LOSS if k == "sep_losses" else K_TAILGRAD, report)
    if "sep_d_spec_only" in got:
        fails += check(prefix + "sep_d_spec_only", got["sep_d_spec_only"], r64["sep_d_spec_only"], env["sep_d_spec"], K_TAILGRAD, report)
    return fails
