"""Spectral-library matching cases, their float32 / float64 oracle runs and the comparators (plain helper module, no tests in it).  It
mirrors tests/material_f64.py for csrc/umhs_library.hip.

Used by tests/test_hip_library.py (the kernel and the model on the GPU) and tests/test_library_bounds_cpu.py (the comparators pass the
float32 oracle and reject planted faults; K, the tie cap and the teeth are measured there).

Statement (include/umhs_hip.h, "Spectral library matching"), on float32 spectra [R,B] and float32 unit rows [L,B]:
  cos[r,l] = (sum_b s_b e_b) / sqrt(sum_b s_b^2), b ascending; the two largest per row, ties to the smaller index, the second another
  entry than the first; (-1, -1.0) for a missing second; index (-1, -1) and cos (0, 0) for a row that is all zero or holds a NaN / Inf.
The float64 run (the truth) takes the SAME float32 inputs, so the unit rows' own rounding is not part of the error.

ONE RULE per reported cosine:   |got - cos64[r, index]| <= K u (mag + tiny),   u = 2^-24,   tiny = 2^-126,
  mag[r,l] = sum_b |s_b e_b| / |s| + 2 |cos64[r,l]|   (as rays_f64.cluster_ties builds it),
judged at the index the code under test reported.
ONE RULE per reported index: it lies in the float64 TIED SET: the entries whose cos64 is within EDGE x (mag + mag_best) of the best,
EDGE = 64 u (rays_f64); the second index likewise among the entries other than the reported first.
Exact properties beside the rules: the second differs from the first; degenerate rows give exactly (-1, -1) / (0, 0); L = 1 gives
(-1, -1.0) for the second; of the two DUPLICATED library rows (dup_a < dup_b, identical bits) dup_b is never first, and it is second
only behind dup_a.

K = max(8, 4 x the float32 CPU oracle's worst ratio over the cases, rounded up to a power of two).  Measured on the CPU (float32
oracle: one rounding per product and per sum, then sqrt and the division; tests/test_library_bounds_cpu.py re-measures and asserts
4 x worst <= K): worst 4.30 (at R200-B256-L64; 4.05 at R1000-B141-L2048), 4 x 4.30 = 17.2, so K = 32.

Conditions on the cases, asserted on the float64 run alone with the library DEDUPLICATED (dup_b left out: it ties by construction):
  tie cap  at most 2 % of a case's live rows have more than one entry in the first's or the second's tied set.  Measured worst: 1.8 %
           (one row of R67-B141-L257), counting both slots.  The builder's seed was picked once for this: at seed 0, (300, 4, 33) has 2.7 %.
  teeth    at least 90 % of the live rows have |cos0 - cos1| > 16 x (K u (mag0 + tiny)).  Measured worst: 0.965 (R67-B141-L257).
No case has many entries at B <= 3: 300 directions in a quadrant are closer than a float32 cosine resolves (at (257, 2, 300) 82 % of
the rows tie)."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import torch

from rays_f64 import EDGE, TEETH, TINY, U  # noqa: F401  (one rule, one edge margin)

K_COS = 32.0
TIE_CAP = 0.02
MIN_TEETH = 0.9

CASES = [(0, 31, 5), (1, 1, 1), (257, 2, 2), (300, 4, 33), (257, 8, 15), (300, 31, 16), (300, 31, 17), (130, 65, 33), (67, 141, 257),
         (513, 31, 1000), (200, 256, 64), (1000, 141, 2048)]


def case_id(c) -> str:
    return f"R{c[0]}-B{c[1]}-L{c[2]}"


def make_library(L: int, B: int, g: torch.Generator) -> torch.Tensor:
    """[L,B] float32 reflectances: rand 0.9 + 0.05, smoothed over three neighbouring bands when B >= 4."""
    lib = torch.rand(L, B, generator=g, dtype=torch.float64) * 0.9 + 0.05
    if B >= 4:
        pad = torch.cat([lib[:, :1], lib, lib[:, -1:]], dim=1)
        lib = (pad[:, :-2] + pad[:, 1:-1] + pad[:, 2:]) / 3.0
    return lib.float()


def unit_rows(lib: torch.Tensor) -> torch.Tensor:
    """The library rows at unit length: normalised in float64, rounded once."""
    d = lib.double()
    return (d / d.norm(dim=1, keepdim=True)).float()


@functools.lru_cache(maxsize=None)
def make_case(R: int, B: int, L: int, seed: int = 1) -> Dict:
    """First half of the rows: gain (entry + 0.05 randn) -- rows 0..2 from the duplicated entry when there is one; second half: gain
    rand.  A run of all-zero rows, one row with a NaN and one with an Inf when R >= 16; one duplicated pair of library rows when
    L >= 3 (at L = 2 a duplicate would leave no row with a distinct second)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + 3 * B + L)
    lib = make_library(L, B, g)
    dup = None
    if L >= 3:
        dup = (L // 3, L - 1 - L // 4)
        lib[dup[1]] = lib[dup[0]]
    entry = torch.randint(0, L, (R,), generator=g)
    if dup is not None and R >= 8:
        entry[:3] = dup[0]
    gain = 0.2 + 2.0 * torch.rand(R, 1, generator=g)
    spectra = gain * (lib[entry] + 0.05 * torch.randn(R, B, generator=g))
    half = R // 2
    spectra[half:] = gain[half:] * torch.rand(R - half, B, generator=g)
    degenerate = torch.zeros(R, dtype=torch.bool)
    if R >= 16:
        z0 = R // 3
        spectra[z0:z0 + max(2, R // 8)] = 0.0
        spectra[R - 1, B // 2] = float("nan")
        spectra[R - 2, B - 1] = float("inf")
        degenerate[z0:z0 + max(2, R // 8)] = True
        degenerate[R - 2:] = True
    return dict(R=R, B=B, L=L, library=lib, unit=unit_rows(lib), spectra=spectra.float(), degenerate=degenerate, dup=dup)


def top2(cos: torch.Tensor, degenerate: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(index int32 [R,2], cos [R,2]) of a cosine matrix [R,L] by the header's rules, whatever torch's own tie order is."""
    R, L = cos.shape
    ninf = float("-inf")
    c = torch.where(torch.isnan(cos), torch.full_like(cos, ninf), cos)
    ar, rows = torch.arange(L)[None, :], torch.arange(R)
    out_i, out_c = [], []
    for _ in range(2):
        m = c.max(1).values
        i = torch.where(c == m[:, None], ar, L).min(1).values
        valid = m > ninf
        i = torch.where(valid, i, torch.full_like(i, -1))
        out_i.append(i), out_c.append(torch.where(valid, m, torch.full_like(m, -1.0)))
        c = c.clone()
        c[rows[valid], i[valid]] = ninf
    index, cosv = torch.stack(out_i, 1).to(torch.int32), torch.stack(out_c, 1)
    dead = degenerate | (index[:, 0] < 0)
    index[dead] = -1
    cosv[dead] = 0.0
    return index, cosv


def oracle(case: Dict, dtype, drop_last_band: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The statement in ``dtype``: b ascending, one rounding per product and per sum.  ``drop_last_band``: a planted fault."""
    s, e = case["spectra"].to(dtype), case["unit"].to(dtype)
    B = case["B"] - (1 if drop_last_band else 0)
    dot, ss = torch.zeros(case["R"], case["L"], dtype=dtype), torch.zeros(case["R"], dtype=dtype)
    for b in range(B):
        dot = dot + s[:, b:b + 1] * e[None, :, b]
        ss = ss + s[:, b] * s[:, b]
    return top2(dot / torch.sqrt(ss)[:, None], case["degenerate"])


@functools.lru_cache(maxsize=None)
def _ref64_cached(key) -> Dict:
    return ref64(make_case(*key))


def ref64(case: Dict) -> Dict:
    """float64 on the float32 inputs: cos [R,L] and mag + tiny [R,L] (rows of ``degenerate`` hold nothing that is looked at)."""
    s, e = case["spectra"].double(), case["unit"].double()
    s = torch.where(case["degenerate"][:, None], torch.ones_like(s), s)
    ns = s.norm(dim=1, keepdim=True)
    cos = (s @ e.T) / ns
    return dict(cos=cos, mag=(s.abs() @ e.abs().T) / ns + 2 * cos.abs() + TINY)


def reference(R: int, B: int, L: int) -> Tuple[Dict, Dict]:
    """(case, float64 run), computed once per shape and shared; neither is to be changed."""
    return make_case(R, B, L), _ref64_cached((R, B, L))


def _tied(cos: torch.Tensor, mag: torch.Tensor, exclude: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bool [R,L]: within EDGE x (mag + mag_best) of the best (the best included); ``exclude`` [R] int64: a column left out per row."""
    c = cos.clone()
    if exclude is not None:
        c[torch.arange(c.shape[0]), exclude] = float("-inf")
    best = c.argmax(1, keepdim=True)
    tied = (c.gather(1, best) - c) < EDGE * (mag + mag.gather(1, best))
    tied.scatter_(1, best, True)
    if exclude is not None:
        tied[torch.arange(c.shape[0]), exclude] = False
    return tied


def check_match(case: Dict, index, cos, r64: Dict, K: float = K_COS, report: Optional[Dict] = None, prefix: str = "") -> List[str]:
    """Every rule of the module docstring; report[prefix + 'cos0' / 'cos1'] = {"worst", "n"}."""
    R, L = case["R"], case["L"]
    index, cos = index.detach().cpu().long(), cos.detach().cpu()
    if tuple(index.shape) != (R, 2) or tuple(cos.shape) != (R, 2):
        return [f"{prefix}shapes {tuple(index.shape)} / {tuple(cos.shape)}, want {(R, 2)}"]
    fails: List[str] = []
    dead, live = case["degenerate"], ~case["degenerate"]
    if bool(((index[dead] != -1) | (cos[dead] != 0)).any()):
        fails.append(f"{prefix}a row that is all zero or holds a NaN / Inf did not give index (-1, -1) and cos (0, 0)")
    idx, c = index[live], cos[live].double()
    c64, mag = r64["cos"][live], r64["mag"][live]
    n = idx.shape[0]
    if n == 0:
        if report is not None:
            report[prefix + "cos0"] = report[prefix + "cos1"] = {"worst": 0.0, "n": 0}
        return fails
    if bool(((idx[:, 0] < 0) | (idx[:, 0] >= L)).any()):
        return fails + [f"{prefix}first index outside 0..{L - 1} on {int(((idx[:, 0] < 0) | (idx[:, 0] >= L)).sum())} live rows"]
    has2 = L >= 2
    if not has2:
        if bool(((idx[:, 1] != -1) | (c[:, 1] != -1.0)).any()):
            fails.append(f"{prefix}L = 1: the second is not (-1, -1.0)")
    else:
        if bool(((idx[:, 1] < 0) | (idx[:, 1] >= L)).any()):
            return fails + [f"{prefix}second index outside 0..{L - 1}"]
        if bool((idx[:, 1] == idx[:, 0]).any()):
            fails.append(f"{prefix}the second equals the first on {int((idx[:, 1] == idx[:, 0]).sum())} rows")
    for slot in ((0, 1) if has2 else (0,)):
        ref, m = c64.gather(1, idx[:, slot:slot + 1])[:, 0], mag.gather(1, idx[:, slot:slot + 1])[:, 0]
        d = (c[:, slot] - ref).abs()
        ratio = torch.where(d == 0, torch.zeros_like(d), d / (U * m))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        worst = float(ratio.max())
        if report is not None:
            report[f"{prefix}cos{slot}"] = {"worst": worst, "n": n}
        if worst > K:
            i = int(ratio.argmax())
            fails.append(f"{prefix}cos{slot}: live row {i}: {float(c[i, slot]):.9g} vs float64 {float(ref[i]):.9g} = {worst:.3g} u mag "
                         f"(K = {K:g}; {int((ratio > K).sum())} of {n} over)")
        tied = _tied(c64, mag, None if slot == 0 else idx[:, 0])
        out = ~tied.gather(1, idx[:, slot:slot + 1])[:, 0]
        if bool(out.any()):
            i = int(out.nonzero()[0])
            fails.append(f"{prefix}index{slot}: {int(out.sum())} of {n} live rows outside the float64 tied set (first: live row {i}, "
                         f"entry {int(idx[i, slot])})")
    if case["dup"] is not None:
        a, b = case["dup"]
        if bool((idx[:, 0] == b).any()) or bool(((idx[:, 1] == b) & (idx[:, 0] != a)).any()):
            fails.append(f"{prefix}entry {b} duplicates entry {a}: the earlier one must come first")
        both = (idx[:, 0] == a) & (idx[:, 1] == b)
        if bool((cos[live][both][:, 0] != cos[live][both][:, 1]).any()):
            fails.append(f"{prefix}entries {a} and {b} are identical rows but their cosines differ in bits")
    return fails


def conditions(case: Dict, r64: Dict, K: float = K_COS) -> Dict:
    """{"tied": share of live rows with a tie for the first or the second, "teeth": share with |cos0 - cos1| > 16 x bound, "live": n},
    on the float64 run with dup_b left out; None where there is nothing to measure."""
    live = ~case["degenerate"]
    cos, mag = r64["cos"][live], r64["mag"][live]
    if case["dup"] is not None:
        keep = torch.ones(case["L"], dtype=torch.bool)
        keep[case["dup"][1]] = False
        cos, mag = cos[:, keep], mag[:, keep]
    n = cos.shape[0]
    if n == 0 or cos.shape[1] < 2:
        return {"tied": 0.0 if n else None, "teeth": None, "live": n}
    t0 = _tied(cos, mag)
    best = cos.argmax(1)
    t1 = _tied(cos, mag, best)
    tied = (t0.sum(1) > 1) | (t1.sum(1) > 1)
    top = cos.topk(2, dim=1).values
    bound = K * U * mag.gather(1, best[:, None])[:, 0]
    return {"tied": float(tied.sum()) / n, "teeth": float(((top[:, 0] - top[:, 1]) > TEETH * bound).sum()) / n, "live": n}
