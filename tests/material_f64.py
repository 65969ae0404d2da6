"""Material-edit cases, their float32 / float64 oracle runs, the element-wise comparators and the float64 edited render (plain helper
module, no tests in it).  It mirrors tests/rays_f64.py for csrc/umhs_material.hip.

Used by tests/test_hip_material.py (the two kernels and the edited model on the GPU) and tests/test_material_bounds_cpu.py (the
comparators pass the float32 oracle and reject planted faults; K is measured there).

Statements (include/umhs_hip.h, "Material edits"), on float32 inputs, evaluated in float32 (c ascending, one rounding per product and
per sum) and in float64 (the truth):
  sigma    sigma'[n] = sigma[n] max(0, 1 + sum_c (d_c - 1) a[n,c])
  remix    mix_term[r,b] = sum_{c<C} mix16[r,c] E''[c,b];  specular = s comp_specular;  spectral2 = mix_term;
           spectral = mix_term + specular  (without the specular head: spectral = mix_term)

ONE RULE for every output element:   |got - ref64| <= K u (mag + tiny),   u = 2^-24,   tiny = 2^-126.
  remix    mag = sum_c |mix16 E''| (spectral2) , |s comp_specular| (specular), their sum (spectral)
  sigma    mag = |sigma| (1 + sum_c |(d_c - 1) a_c|).  The clamp is 1-Lipschitz, so the rule holds on both of its sides; that no element
           is NEGATIVE is an exact property the comparator checks beside the rule (a missing clamp with all-zero gains on rows that
           sum to 1 + 2^-23 errs by 2^-23 sigma, inside the rule's 2 K u sigma: only the sign shows it).

K per family = max(8, 4 x the float32 CPU oracle's worst ratio over the committed cases, rounded up to a power of two).  Measured on the
CPU (float32 oracle, worst |diff| / (u (mag + tiny)) over all cases; tests/test_material_bounds_cpu.py re-measures and asserts
4 x worst <= K):
  remix spectral 2.60 | spectral2 2.56 | specular 1.00 | sigma 2.77
so K = 16 for both families: 4 x 2.60 = 10.4 and 4 x 2.77 = 11.1 round up to 16 (a 15-term chain of products of both signs, one rounding
per product and per sum, in float32 against the same chain in float64; the kernels fuse each pair into one fmaf, which can only halve
the roundings).

Teeth: the share of elements with |ref64| > 16 x bound.  Condition: in every case at least 90 % of the elements on non-empty rays
(remix) / of all elements (sigma) have teeth.  Measured on the float64 run alone: remix >= 0.9997 in every case; sigma >= 0.969 (what
lacks teeth there: a density of 0, and a sample made almost wholly of a material whose gain is 0).

The edited render (``edited_render``) is composed from oracle/torch_ref.py as it is: ``field_density``; ``field_outputs`` on a
FieldParams whose ``endmembers`` are E'' for the edited spectrum and on the original FieldParams for the abundances, the specular term
and the spectrum segmentation looks at; the density factor applied to ``density``; then ``render_weight_from_density``,
``spectral_renderer``, ``render_depth_expected``, ``colour_system`` and ``cluster_lookup``."""
from __future__ import annotations

import copy
from typing import Dict, List, Optional

import torch

from oracle import torch_ref as T
from rays_f64 import EDGE, TEETH, TINY, U, check, cluster_ties  # noqa: F401  (re-exported: one rule, one edge margin)

K_REMIX = 16.0
K_SIGMA = 16.0

# (R, B, C, specular): band counts on both sides of a wave, the project's own 31 / 141 / 256, C at both ends, R off every multiple of
# the workgroup and of the 32-ray tile
REMIX_CASES = [(0, 31, 3, False), (1, 1, 1, False), (5, 31, 6, True), (257, 64, 15, True), (130, 65, 4, False), (67, 141, 15, True),
               (33, 256, 2, True)]
SIGMA_NS = (0, 1, 63, 64, 65, 1000, 4099)
SIGMA_CS = (1, 3, 15)
GAIN_CYCLE = (0.0, 1.0, 2.5)


def remix_id(c) -> str:
    return f"R{c[0]}-B{c[1]}-C{c[2]}-{'spec' if c[3] else 'nospec'}"


def make_remix_case(R: int, B: int, C: int, specular: bool, seed: int = 0) -> Dict:
    """mix16 [R,16] with NaN in the columns >= C (never read) and a run of all-zero rows (empty rays: an exact 0 out), a dictionary
    with rows of both signs, the composited specular term and a specular gain."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + 3 * B + C)
    mix = torch.rand(R, 16, generator=g) * 3.0
    mix[:, C:] = float("nan")
    empty = torch.zeros(R, dtype=torch.bool)
    if R >= 5:
        empty[R // 3: R // 3 + max(2, R // 8)] = True
        empty[-1] = True
    mix[empty, :C] = 0.0
    E = torch.rand(C, B, generator=g) * 2.0 - 0.5
    E[::2] *= -1.0 if C > 1 else 1.0
    cs = torch.rand(R, B, generator=g) if specular else None
    if cs is not None:
        cs[empty] = 0.0
    return dict(R=R, B=B, C=C, mix=mix, E=E, comp_specular=cs, s=0.75 if specular else 1.0, empty=empty)


def remix_oracle(case: Dict, dtype, E: Optional[torch.Tensor] = None, drop_class: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The statement in ``dtype``, c ascending.  ``E``: another dictionary; ``drop_class``: leave that class out (planted faults)."""
    mix, E = case["mix"].to(dtype), (case["E"] if E is None else E).to(dtype)
    term = torch.zeros(case["R"], case["B"], dtype=dtype)
    for c in range(case["C"]):
        if c != drop_class:
            term = term + mix[:, c:c + 1] * E[c][None, :]
    if case["comp_specular"] is None:
        return {"spectral": term}
    sp = torch.tensor(case["s"], dtype=torch.float32).to(dtype) * case["comp_specular"].to(dtype)
    return {"spectral": term + sp, "spectral2": term, "specular": sp}


def remix_envelopes(mix16: torch.Tensor, E: torch.Tensor, comp_specular: Optional[torch.Tensor], s: float) -> Dict[str, torch.Tensor]:
    """``mag + tiny`` per output, float64.  (Takes arrays, not a case: the model tests call it on the mix a render returned.)"""
    C = E.shape[0]
    m = mix16.detach().double().cpu()[:, :C].abs() @ E.detach().double().cpu().abs()
    if comp_specular is None:
        return {"spectral": m + TINY}
    sp = (float(torch.tensor(s, dtype=torch.float32)) * comp_specular.detach().double().cpu()).abs()
    return {"spectral": m + sp + TINY, "spectral2": m + TINY, "specular": sp + TINY}


def remix64(mix16: torch.Tensor, E: torch.Tensor, comp_specular: Optional[torch.Tensor], s: float) -> Dict[str, torch.Tensor]:
    """The float64 statement on arrays (columns >= C of ``mix16`` are not touched)."""
    case = dict(R=mix16.shape[0], B=E.shape[1], C=E.shape[0], mix=mix16.detach().cpu(), E=E.detach().cpu(),
                comp_specular=None if comp_specular is None else comp_specular.detach().cpu(), s=s)
    return remix_oracle(case, torch.float64)


def check_remix(case: Dict, got: Dict, r64: Dict, report=None, prefix="") -> List[str]:
    env = remix_envelopes(case["mix"], case["E"], case["comp_specular"], case["s"])
    live = ~case["empty"][:, None]
    fails: List[str] = []
    if sorted(got) != sorted(r64):
        return [f"{prefix}outputs {sorted(got)}, want {sorted(r64)}"]
    for k in r64:
        fails += check(prefix + k, got[k], r64[k], env[k], K_REMIX, report, teeth_mask=live)
        if case["R"] and bool((got[k].detach().cpu()[case["empty"]] != 0).any()):
            fails.append(f"{prefix}{k}: an all-zero mix row did not give an exact 0")
    return fails


def sigma_id(c) -> str:
    return f"n{c[0]}-C{c[1]}"


def make_sigma_case(n: int, C: int, seed: int = 0, gains=None) -> Dict:
    """Densities over six decades, softmax abundance rows at two temperatures, gains mixing 0, 1 and 2.5 (C = 1: 2.5)."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * n + C)
    sigma = torch.exp(torch.rand(n, generator=g) * 14.0 - 7.0)
    sigma[5::97] = 0.0  # (a selector of 0)
    logits = torch.randn(n, C, generator=g) * torch.where(torch.rand(n, 1, generator=g) < 0.5, 1.0, 6.0)
    a = torch.softmax(logits, dim=-1)
    if gains is None:
        gains = [2.5] if C == 1 else [GAIN_CYCLE[c % 3] for c in range(C)]
    return dict(n=n, C=C, sigma=sigma, a=a, gain=torch.tensor(gains, dtype=torch.float32))


def rows_summing_above_one(n: int, C: int) -> torch.Tensor:
    """Abundance rows [n,C] whose float32 sum in ascending class order is exactly 1 + 2^-23 (a softmax may do that)."""
    a = torch.zeros(n, C)
    if C == 1:
        a[:, 0] = 1.0 + 2.0 ** -23
        return a
    a[:, 0] = 0.5
    a[:, 1] = 0.5 + 2.0 ** -23  # 0.5 + 2^-23 is representable; 0.5 + it = 1 + 2^-23 exactly
    return a


def sigma_oracle(case: Dict, dtype, clamp: bool = True) -> torch.Tensor:
    acc = torch.zeros(case["n"], dtype=dtype)
    a, d = case["a"].to(dtype), case["gain"].to(dtype)
    for c in range(case["C"]):
        acc = acc + (d[c] - 1.0) * a[:, c]
    f = 1.0 + acc
    return case["sigma"].to(dtype) * (f.clamp(min=0.0) if clamp else f)


def sigma_envelope(case: Dict) -> torch.Tensor:
    a, d = case["a"].double(), case["gain"].double()
    return case["sigma"].double().abs() * (1.0 + ((d - 1.0)[None, :] * a).abs().sum(1)) + TINY


def check_sigma(case: Dict, got: torch.Tensor, r64: torch.Tensor, report=None, prefix="") -> List[str]:
    fails = check(prefix + "sigma", got, r64, sigma_envelope(case), K_SIGMA, report)
    if bool((got.detach().cpu() < 0).any()):
        fails.append(f"{prefix}sigma: {int((got.detach().cpu() < 0).sum())} negative densities")
    return fails


def teeth_failures(report: Dict, min_share: float = 0.9) -> List[str]:
    return [f"{k}: only {v['teeth']:.3f} of the elements have teeth" for k, v in report.items()
            if v["teeth"] is not None and v["teeth"] < min_share]


# ------------------------------------------------------------------------------------------------------------------------------ #
# the edited render
# ------------------------------------------------------------------------------------------------------------------------------ #
def field_params_of(field, dtype=torch.float64) -> T.FieldParams:
    """The oracle's FieldParams holding the parameters of a UMHSField (its state dict carries the reference's key names)."""
    L = field.layout
    p = T.FieldParams(L.num_classes, L.wavelengths, bool(L.pred_specular), log2_hashmap_size=L.log2_hashmap_size, dtype=dtype)
    sd = {k: v.detach().cpu() for k, v in field.state_dict().items()}
    with torch.no_grad():
        for k, v in p.reference_state_dict().items():
            v.copy_(sd[k].to(dtype))
    p.scalings = p.scalings.to(dtype)
    return p


def edited_render(p: T.FieldParams, E_edit: torch.Tensor, density_gain: torch.Tensor, specular_gain: float, origins, directions, starts,
                  ends, ray_indices, num_rays: int, temperature: float, colour_M, contraction: bool = True) -> Dict[str, torch.Tensor]:
    """The edited render in ``p``'s dtype on the given samples (module docstring): abundances from the UNEDITED field, weights from
    the edited density, segmentation from the unedited spectrum under those weights against the model's own dictionary."""
    dt = p.hash_table.dtype
    o, d, t0, t1 = (x.detach().cpu().to(dt) for x in (origins, directions, starts, ends))
    t0, t1 = t0.view(-1, 1), t1.view(-1, 1)
    ri = ray_indices.detach().cpu().long()
    with torch.no_grad():
        density, emb, _, _ = T.field_density(p, o, d, t0, t1, contraction)
        fo = T.field_outputs(p, o, d, t0, t1, emb, temperature)
        pe = copy.deepcopy(p)
        pe.endmembers.copy_(E_edit.detach().cpu().to(dt))
        fe = T.field_outputs(pe, o, d, t0, t1, emb, temperature)
        N, C = o.shape[0], p.C
        a = fo["abundances"].reshape(N, C)
        factor = (1.0 + ((density_gain.detach().cpu().to(dt) - 1.0)[None, :] * a).sum(1)).clamp(min=0.0)
        density = density * factor[:, None]
        pinfo = T.pack_info(ri, num_rays)
        weights = T.render_weight_from_density(t0[..., 0], t1[..., 0], density[..., 0], pinfo)[0][..., None]
        out = {"depth": T.render_depth_expected(weights, t0, t1, ri, num_rays),
               "accumulation": T.accumulate_along_rays(weights[..., 0], None, ri, num_rays), "weights": weights}
        if p.pred_specular:
            out["spectral2"] = T.spectral_renderer(fe["spectral2"], weights, ri, num_rays)
            out["specular"] = float(torch.tensor(specular_gain, dtype=torch.float32)) * T.spectral_renderer(fo["specular"], weights, ri, num_rays)
            out["spectral"] = out["spectral2"] + out["specular"]
        else:
            out["spectral"] = T.spectral_renderer(fe["spectral"], weights, ri, num_rays)
        unedited = T.spectral_renderer(fo["spectral"], weights, ri, num_rays)
        out["rgb"] = T.colour_system(out["spectral"], colour_M.detach().cpu().to(dt))
        out["abundances"] = T.spectral_renderer(fo["abundances"], weights, ri, num_rays)
        _, probs = T.cluster_lookup(unedited, 0.2, p.endmembers)
        out["seg_probs"] = probs
        out["seg_raw"] = probs.argmax(1) * (out["accumulation"] > 0.5).to(dt).squeeze(-1)
        out["unedited_spectral"] = unedited
    return out
