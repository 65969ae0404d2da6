"""Field-kernel cases, their float32 / float64 oracle runs and the comparators (plain helper module, no tests in it).

Used by tests/test_hip_field_variants.py (every kernel instance the field launchers select), tests/field_tf_child.py (the same rows
on the fp32 chain, UMHS_BWD_TF=1) and tests/test_field_f64_bounds_cpu.py (the comparators reject planted faults).

A case starts from the hash features (random ``enc``), world positions, directions and a selector with some zeros -- the field
kernels' own inputs -- and packs its samples into rays (empty rays, rays shorter than a 16-sample tile, rays across many tiles).  The
oracle (oracle/torch_ref.py) runs on the same fp32 inputs twice: in float32 (the reference's arithmetic: its distance from float64 is
the noise floor the kernels share) and in float64 (the truth).  Bounds, in one place (the ones tests/test_hip_fullsize.py and
tests/test_hip_parity.py hold the same outputs to):
  * per-sample forward outputs and per-ray sums: every element within 1e-4 |f64| + 1e-6 max|f64| of float64, and the largest
    difference within 2e-5 of the largest entry (test_field_fwd's max-norm bound);
  * d_enc, d_sigma, every weight / bias / endmember gradient, max-norm relative to the tensor's largest float64 entry:
    err(hip, f64) <= 2 err(f32 oracle, f64) + 5e-6 and err(hip, f32 oracle) <= 5e-5 at the large-n rows, with no bias there: the
    regression slope of (hip - f32 oracle) on the gradient below 6e-6 (a truncating bf16 split shrinks every product by ~2^-17:
    slope -7.6e-6).  At the rows of a few hundred samples and less the float64 bound is 2 err(f32 oracle, f64) + 2e-5: the default
    backward forms dW from two-piece bf16 operands, which keep 16 of each operand's 24 bits, so one product is off by
    up to ~2^-16 of itself; over 262,144 samples that averages out below 5e-6 (tests/test_hip_fullsize.py), over one sample it does
    not (measured: 1.55e-5 of the largest entry, d endmembers at n = 1).  The fp32-oracle bound 5e-5 is test_field_bwd's.
    The folded form (umhs_field_bwd_composited) forms d_sigma itself (to 2e-7 of its largest entry), and mlp_base's gradients
    sum d_sigma sigma over samples of both signs: the cancellation magnifies that rounding (the fp32 oracle's own: up to 7e-6).
    There the bounds are 2 err(f32 oracle, f64) + 1e-4 and 1e-4 from the fp32 oracle (measured: 4.5e-5 / 5.1e-5, d base_b.1 without
    grad scaling; tests/test_hip_fullsize.py holds the training step's gradients, which take this path, to 2e-4);
  * a parameter the configuration does not use (mlp_directional without the specular head) comes back exactly zero.
A sample with a ReLU pre-activation within 1e-5 of its dot product's magnitude (sum |w x| + |b|) of zero has a hidden unit that is on
in one fp32 evaluation order and off in another, which moves its whole contribution to d_enc and dW (measured: 3.9e-3 of d head_w.0's
largest entry from one sample at a pre-activation of 9e-10).  The case builder makes such samples (about 1 %) inert: selector 0 and
zero cotangents, so neither side's gradient holds them; their forward outputs are compared like every other sample's."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from oracle import torch_ref as T

GEO = 15
FWD_RTOL, FWD_ATOL, FWD_MAXNORM = 1e-4, 1e-6, 2e-5
GRAD_K, GRAD_ABS, GRAD_ABS_FEW, GRAD_F32 = 2.0, 5e-6, 2e-5, 5e-5
GRAD_FOLDED = 1e-4  # both bounds of the folded form (docstring)
SLOPE = 6e-6
RELU_MARGIN = 1e-5
# reference state-dict key of every oracle parameter but the hash table (the field kernels never see it)
PARAM_KEYS = {}
for _stem, _pre in (("base", "mlp_base.mlp"), ("head", "mlp_head"), ("feat", "feature_mlp"), ("dir", "mlp_directional")):
    for _i in range(3):
        PARAM_KEYS[f"{_stem}_w.{_i}"] = f"{_pre}.layers.{_i}.weight"
        PARAM_KEYS[f"{_stem}_b.{_i}"] = f"{_pre}.layers.{_i}.bias"
PARAM_KEYS["endmembers"] = "endmembers"

RAY_PATTERN = (0, 3, 2, 0, 1, 40, 17, 16, 5, 4, 3, 200, 0, 7, 33, 1, 1, 1, 90, 0)


def ray_counts(n: int) -> torch.Tensor:
    """n samples packed into rays by cycling RAY_PATTERN (empty rays, sub-tile rays several to a tile, rays over many tiles); the
    last ray takes the remainder, and the batch ends in an empty ray."""
    counts, left, i = [], n, 0
    while left > 0:
        c = min(RAY_PATTERN[i % len(RAY_PATTERN)], left)
        counts.append(c)
        left -= c
        i += 1
    counts.append(0)
    return torch.tensor(counts, dtype=torch.int64)


@dataclass
class Case:
    C: int
    B: int
    spec: bool
    temp: float
    n: int
    seed: int
    p: T.FieldParams
    enc: torch.Tensor  # [n,32] sample-major (the oracle's layout)
    wpos: torch.Tensor
    dirs: torch.Tensor
    sel: torch.Tensor  # [n] float 0/1
    cot_s: torch.Tensor  # plain backward: cotangents of spectral [n,B], sigma [n], emb [n,15]
    cot_d: torch.Tensor
    cot_e: torch.Tensor
    counts: torch.Tensor  # rays
    t0: torch.Tensor
    t1: torch.Tensor
    d_comp: torch.Tensor  # folded backward: gradients of the per-ray band sums [R,B] and of the accumulation [R]
    d_acc: torch.Tensor
    extra: Dict = field(default_factory=dict)

    @property
    def R(self) -> int:
        return self.counts.numel()

    def packed_info(self) -> torch.Tensor:
        return torch.stack([torch.cumsum(self.counts, 0) - self.counts, self.counts], 1).contiguous()

    def ray_indices(self) -> torch.Tensor:
        return torch.repeat_interleave(torch.arange(self.R), self.counts)


def make_case(C: int, B: int, spec: bool, temp: float, n: int, seed: int = 0) -> Case:
    """Parameters as tests/test_hip_parity.make_case draws them (table unused: the features are given), inputs random."""
    p = T.FieldParams(C, B, spec, log2_hashmap_size=12, table_scale=0.5, seed=seed)
    with torch.no_grad():
        p.base_b[1][0] += 1.0  # raise sigma so that the compositing weights are not all ~0
    g = torch.Generator().manual_seed(1000 + seed)
    enc = torch.rand(n, 32, generator=g) - 0.5
    wpos = torch.rand(n, 3, generator=g) * 3 - 1.5
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    sel = (torch.rand(n, generator=g) > 0.15).float()
    cot_s = torch.rand(n, B, generator=g) - 0.3
    cot_d = torch.rand(n, generator=g) - 0.3
    cot_e = torch.rand(n, GEO, generator=g) - 0.5
    counts = ray_counts(n)
    t0 = torch.rand(n, generator=g) * 1.5
    t1 = t0 + 0.02 + 0.05 * torch.rand(n, generator=g)
    d_comp = torch.randn(counts.numel(), B, generator=g)
    d_acc = torch.randn(counts.numel(), generator=g)
    with torch.no_grad():
        inert = relu_margins(copy.deepcopy(p).double(), enc.double(), wpos.double(), dirs.double()) <= RELU_MARGIN
    sel[inert] = 0
    for t in (cot_s, cot_d, cot_e):
        t[inert] = 0
    return Case(C, B, spec, temp, n, seed, p, enc, wpos, dirs, sel, cot_s, cot_d, cot_e, counts, t0, t1, d_comp, d_acc,
                extra={"inert": int(inert.sum())})


# ------------------------------------------------------------------------------------------------------------------------------ #
# oracle
# ------------------------------------------------------------------------------------------------------------------------------ #
def field_forward(p: T.FieldParams, enc, wpos, dirs, sel, temp) -> Dict[str, torch.Tensor]:
    """mlp_base from the features, then T.field_outputs's arithmetic op for op -- restated only so that its shapes hold at one sample
    or one band (the reference squeezes every unit dimension of its [N,B] mixing product)."""
    n = enc.shape[0]
    h = T.mlp_forward(enc, list(p.base_w), list(p.base_b))
    sraw, emb = torch.split(h, [1, p.geo], dim=-1)
    out = {"sigma_raw": sraw[:, 0], "sigma": (T.trunc_exp(sraw) * sel[:, None])[:, 0], "emb": emb}
    d = T.sh_encoding_deg4((dirs + 1.0) / 2.0)
    pe = T.nerf_encoding(wpos)
    h1 = torch.cat([pe, emb], dim=-1)
    scalar = torch.sigmoid(T.mlp_forward(h1, list(p.head_w), list(p.head_b)).view(n, -1, p.C))  # [N,1,C]
    logits = T.mlp_forward(h1, list(p.feat_w), list(p.feat_b))
    out["feat_logits"] = logits
    if p.pred_specular:
        logits, s1 = torch.split(logits, [p.C, 1], dim=-1)
        s1 = torch.sigmoid(s1)
    abund = torch.softmax(logits / temp, dim=-1)  # [N,C]
    E = p.endmembers.unsqueeze(0).expand(n, -1, -1).transpose(1, 2)  # [N,B,C]
    spec = (scalar * E @ abund.unsqueeze(-1)).squeeze(-1)  # [N,B]
    out["abundances"] = abund
    if p.pred_specular:
        specular = T.mlp_forward(torch.cat([d, pe], dim=-1), list(p.dir_w), list(p.dir_b), "sigmoid")
        out["spectral"] = spec + s1 * specular
        out["spectral2"] = spec
        out["specular"] = (s1 * specular).detach()
    else:
        out["spectral"] = spec
    return out


def relu_margins(p: T.FieldParams, enc, wpos, dirs) -> torch.Tensor:
    """Per sample: min over every ReLU unit of |pre-activation| / (sum |w x| + |b|) (float64 inputs)."""
    def layer(x, w, b):
        z = x @ w.T + b
        return z, (x.abs() @ w.abs().T + b.abs())

    ms = []
    z, s = layer(enc, p.base_w[0], p.base_b[0])
    ms.append((z.abs() / s).min(1).values)
    emb = (torch.relu(z) @ p.base_w[1].T + p.base_b[1])[:, 1:]
    pe = T.nerf_encoding(wpos)
    x0 = torch.cat([pe, emb], dim=-1)
    for ws, bs in ((p.head_w, p.head_b), (p.feat_w, p.feat_b)):
        x = x0
        for i in range(2):
            z, s = layer(x, ws[i], bs[i])
            ms.append((z.abs() / s).min(1).values)
            x = torch.relu(z)
    if p.pred_specular:
        z, s = layer(torch.cat([T.sh_encoding_deg4((dirs + 1.0) / 2.0), pe], dim=-1), p.dir_w[0], p.dir_b[0])
        ms.append((z.abs() / s).min(1).values)
    return torch.stack(ms, 1).min(1).values


def _params(p):
    return [(k, v) for k, v in p.named_parameters() if k != "hash_table"]


def _chunk(B: int, C: int) -> int:
    return max(256, (1 << 22) // max(1, B * C))


def oracle_plain(p: T.FieldParams, case: Case, dtype, with_grads=True, drop_last=False, zero_band=None) -> Dict:
    """Forward outputs, and the gradients of  sum(spectral cot_s) + sum(sigma cot_d) + sum(emb cot_e)  w.r.t. enc and every parameter
    (chunks of samples; the parameter gradients are sums, so chunks add up).  drop_last / zero_band: planted faults (the last sample's
    outputs cut off the parameter graph; the spectral cotangent of one band ignored)."""
    cv = lambda t: t.to(dtype)
    names = [k for k, _ in _params(p)]
    params = [v for _, v in _params(p)]
    grads = [torch.zeros_like(v) for v in params]
    outs: Dict[str, List[torch.Tensor]] = {}
    d_enc = []
    n, step = case.n, _chunk(case.B, case.C)
    for a in range(0, max(n, 1), step):
        b = min(n, a + step)
        if b <= a:
            break
        enc = cv(case.enc[a:b]).detach().clone().requires_grad_(with_grads)
        o = field_forward(p, enc, cv(case.wpos[a:b]), cv(case.dirs[a:b]), cv(case.sel[a:b]), case.temp)
        for k, v in o.items():
            outs.setdefault(k, []).append(v.detach())
        if not with_grads:
            continue
        cs, cd, ce = cv(case.cot_s[a:b]).clone(), cv(case.cot_d[a:b]), cv(case.cot_e[a:b])
        if zero_band is not None:
            cs[:, zero_band] = 0
        sp, sg, em = o["spectral"], o["sigma"], o["emb"]
        if drop_last and b == n:
            keep = torch.ones(b - a, 1, dtype=dtype)
            keep[-1] = 0
            sp, sg, em = sp * keep + sp.detach() * (1 - keep), sg * keep[:, 0] + sg.detach() * (1 - keep[:, 0]), em * keep + em.detach() * (1 - keep)
        loss = (sp * cs).sum() + (sg * cd).sum() + (em * ce).sum()
        g = torch.autograd.grad(loss, [enc] + params, allow_unused=True)
        d_enc.append(g[0])
        for acc, gi in zip(grads, g[1:]):
            if gi is not None:
                acc.add_(gi)
    res = {"out": {k: torch.cat(v) for k, v in outs.items()}}
    if with_grads:
        res["d_enc"] = torch.cat(d_enc) if d_enc else torch.zeros(0, 32, dtype=dtype)
        res["grads"] = dict(zip(names, grads))
    return res


def oracle_composited(p: T.FieldParams, case: Case, dtype, grad_scaling: bool, drop_last=False, zero_band=None) -> Dict:
    """The field outputs through nerfacc's compositing (render_weight_from_density, accumulate_along_rays; with grad_scaling,
    scale_gradients_by_distance_squared in front): per-ray sums, and the gradients of  sum(comp d_comp) + sum(acc d_acc)  w.r.t. sigma
    (the field's output), enc and every parameter."""
    cv = lambda t: t.to(dtype)
    names = [k for k, _ in _params(p)]
    params = [v for _, v in _params(p)]
    enc = cv(case.enc).detach().clone().requires_grad_()
    o = field_forward(p, enc, cv(case.wpos), cv(case.dirs), cv(case.sel), case.temp)
    sigma, spectral = o["sigma"], o["spectral"]
    if drop_last and case.n:
        keep = torch.ones(case.n, dtype=dtype)
        keep[-1] = 0
        spectral = spectral * keep[:, None] + spectral.detach() * (1 - keep[:, None])
        sigma_f = sigma * keep + sigma.detach() * (1 - keep)
    else:
        sigma_f = sigma
    t0, t1 = cv(case.t0), cv(case.t1)
    fo = {"density": sigma_f[:, None], "spectral": spectral}
    if grad_scaling:
        fo = T.scale_gradients_by_distance_squared(fo, t0[:, None], t1[:, None])
    pinfo, ri = case.packed_info(), case.ray_indices()
    w = T.render_weight_from_density(t0, t1, fo["density"][:, 0], pinfo)[0]
    comp = T.accumulate_along_rays(w, fo["spectral"], ri, case.R)
    acc = T.accumulate_along_rays(w, None, ri, case.R)
    dc = cv(case.d_comp).clone()
    if zero_band is not None:
        dc[:, zero_band] = 0
    loss = (comp * dc).sum() + (acc[:, 0] * cv(case.d_acc)).sum()
    g = torch.autograd.grad(loss, [sigma, enc] + params, allow_unused=True)
    grads = {k: (gi if gi is not None else torch.zeros_like(v)) for k, v, gi in zip(names, params, g[2:])}
    return {"d_sigma": g[0], "d_enc": g[1], "grads": grads}


def oracle_per_ray(case: Case, out: Dict[str, torch.Tensor], weights=None) -> Dict[str, torch.Tensor]:
    """The per-ray sums the two-launch forward forms from per-sample outputs: SpectralRenderer over the given rendering weights (the
    heads kernel takes them as an input), or over render_weight_from_density of out["sigma"]."""
    pinfo, ri = case.packed_info(), case.ray_indices()
    w = weights
    if w is None:
        w = T.render_weight_from_density(case.t0.to(out["sigma"].dtype), case.t1.to(out["sigma"].dtype), out["sigma"], pinfo)[0]
    keys = ["spectral", "abundances"] + (["spectral2", "specular"] if "specular" in out else [])
    return {k: T.accumulate_along_rays(w, out[k], ri, case.R) for k in keys}


def oracle_pair(case: Case, kind: str, **kw):
    """(float32 run, float64 run) of oracle_plain / oracle_composited; the float64 run uses copy.deepcopy(p).double()."""
    fn = oracle_plain if kind == "plain" else oracle_composited
    p64 = copy.deepcopy(case.p).double()
    r32 = fn(case.p, case, torch.float32, **kw)
    kw64 = {k: v for k, v in kw.items() if k not in ("drop_last", "zero_band")}
    r64 = fn(p64, case, torch.float64, **kw64)
    return r32, r64


# ------------------------------------------------------------------------------------------------------------------------------ #
# comparators: each returns a list of failure messages (empty: within every bound) and records its measurements in ``report``
# ------------------------------------------------------------------------------------------------------------------------------ #
def check_values(name: str, got, ref64, report: Optional[Dict] = None) -> List[str]:
    got, ref = got.detach().double().cpu(), ref64.detach().double().cpu()
    if got.shape != ref.shape:
        return [f"{name}: shape {tuple(got.shape)}, want {tuple(ref.shape)}"]
    if ref.numel() == 0:
        return []
    top = float(ref.abs().max())
    d = (got - ref).abs()
    ratio = d / (FWD_RTOL * ref.abs() + FWD_ATOL * top + 1e-300)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst, mx = float(ratio.max()), float(d.max()) / (top + 1e-300)
    if torch.isnan(d).any():
        mx = float("inf")
    if report is not None:
        report[name] = {"elementwise": worst, "maxnorm": mx}
    fails = []
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        fails.append(f"{name}: element {i}: {float(got.reshape(-1)[i]):.8g} vs float64 {float(ref.reshape(-1)[i]):.8g} "
                     f"({worst:.2f} x the bound 1e-4 |ref| + 1e-6 max|ref|; {int((ratio > 1).sum())} of {ratio.numel()} over)")
    if mx > FWD_MAXNORM:
        fails.append(f"{name}: max|diff| / max|ref| = {mx:.2e} > {FWD_MAXNORM:.0e}")
    return fails


def check_grad(name: str, got, ref32, ref64, report: Optional[Dict] = None, slope: bool = False, abs_term: float = GRAD_ABS,
               f32_bound: float = GRAD_F32) -> List[str]:
    got, a32, a64 = (t.detach().double().cpu() for t in (got, ref32, ref64))
    if got.shape != a64.shape:
        return [f"d {name}: shape {tuple(got.shape)}, want {tuple(a64.shape)}"]
    if a64.numel() == 0:
        return []
    top = float(a64.abs().max())
    if top == 0.0:  # a parameter the configuration does not use
        bad = float(got.abs().max()) if not torch.isnan(got).any() else float("nan")
        if report is not None:
            report[name] = {"unused": True, "max_abs": bad}
        return [] if bad == 0.0 else [f"d {name}: an unused parameter's gradient must be exactly zero (max |g| = {bad:.3e})"]
    nanfix = lambda x: float("inf") if x != x else x
    e64 = nanfix(float((got - a64).abs().max()) / top)
    e3264 = float((a32 - a64).abs().max()) / top
    e32 = nanfix(float((got - a32).abs().max()) / top)
    rec = {"err_vs_f64": e64, "f32oracle_vs_f64": e3264, "err_vs_f32oracle": e32}
    fails = []
    if e64 > GRAD_K * e3264 + abs_term:
        fails.append(f"d {name}: {e64:.2e} from float64 (the fp32 oracle: {e3264:.2e})")
    if e32 > f32_bound:
        fails.append(f"d {name}: {e32:.2e} from the fp32 oracle")
    if slope and a32.numel() >= 256:
        s = float(((got - a32) * a32).sum() / (a32 * a32).sum())
        rec["slope"] = s
        if not abs(s) <= SLOPE:
            fails.append(f"d {name}: the error correlates with the gradient (slope {s:.2e}): a biased product")
    if report is not None:
        report[name] = rec
    return fails


def check_forward(got: Dict, ref64: Dict, keys, report=None, prefix="") -> List[str]:
    fails = []
    for k in keys:
        fails += check_values(prefix + k, got[k], ref64[k], report)
    return fails


def check_backward(got: Dict, r32: Dict, r64: Dict, large=False, report=None, prefix="") -> List[str]:
    """got: {"d_enc": [n,32] sample-major, "grads": {oracle name: tensor}, optional "d_sigma"}.  large: a row past 16,384 samples
    (float64 bound + 5e-6, and the slope check on every weight matrix).  A reference with "d_sigma" is the folded form's."""
    folded = "d_sigma" in r64
    a = GRAD_FOLDED if folded else GRAD_ABS if large else GRAD_ABS_FEW
    f = GRAD_FOLDED if folded else GRAD_F32
    fails = check_grad(prefix + "enc", got["d_enc"], r32["d_enc"], r64["d_enc"], report, abs_term=a, f32_bound=f)
    if folded:  # (d_sigma itself: the plain bounds)
        fails += check_grad(prefix + "sigma", got["d_sigma"], r32["d_sigma"], r64["d_sigma"], report, abs_term=GRAD_ABS_FEW)
    for k in r64["grads"]:
        weight = "_w." in k or k == "endmembers"
        fails += check_grad(prefix + k, got["grads"][k], r32["grads"][k], r64["grads"][k], report, slope=large and weight, abs_term=a,
                            f32_bound=f)
    return fails


def fwd_keys(spec: bool, density_only=False) -> List[str]:
    if density_only:
        return ["sigma", "sigma_raw", "emb"]
    return ["sigma", "sigma_raw", "emb", "feat_logits", "abundances", "spectral"] + (["spectral2", "specular"] if spec else [])
