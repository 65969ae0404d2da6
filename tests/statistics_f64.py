"""Scene-statistics cases, their float32 / float64 oracle runs and the comparators (plain helper module, no tests in it).  It mirrors
tests/library_f64.py for csrc/umhs_statistics.hip.

Used by tests/test_hip_statistics.py (the kernels and the model on the GPU) and tests/test_statistics_bounds_cpu.py (the comparators
pass the float32 oracle and reject planted faults; K_G, K_Y, the case conditions and the teeth are measured there).

Statement (include/umhs_hip.h, "Scene statistics"), on float32 spectra [R,B]:
  gram     c = x - shift (float32); rows are VALID when all B values are finite and accumulation > 0.5; per chunk of CH = 1024 rows of a
           call g[a,b] = the float32 chain of c[r,a] c[r,b] over the valid rows ascending and s[b] the float32 sum of c[r,b]; the chunk
           results are added in float64, chunks ascending, to acc = (count, s[B], G[B,B]).  G is exactly symmetric.
  project  c = x - mean (float32); y[r,k] = the float32 chain of c[b] W[k,b] over b; score[r] = the float32 chain of y[r,k]^2 over all K;
           components = y[:, :P]; a row with a NaN or an Inf gives zeros.
The float64 run (the truth) takes the SAME float32 x, shift, mean and W.

RULES, u = 2^-24:
  count    exact.                                  symmetry  G[a,b] and G[b,a] are the same bits.
  gram     |got - g64[a,b]| <= K_G u sum_r |c_a c_b|           sums   |got - s64[b]| <= K_G u sum_r |c_b|      (c in float64)
  y        |y - y64| <= e := K_Y u (sum_b |c_b W_kb| + tiny)
  score    |score - score64| <= sum_k (2 |y64_k| e_k + e_k^2) + K_Y u sum_k y64_k^2   (it follows from the y rule; nothing is measured)

K_G, K_Y = max(8, 4 x the float32 CPU oracle's worst ratio over the cases, rounded up to a power of two).  The oracle is a plain float32
replay in torch on the CPU (one rounding per product and per sum, the same chunking).  Measured on the CPU
(tests/test_statistics_bounds_cpu.py re-measures and asserts 4 x worst <= K):
  gram  worst 28.4 (a Gram entry at R1100-B141; 21.3 at R1025-B65; the sums: 17.6 at R1100-B141), 4 x 28.4 = 113.5, so K_G = 128.  The
        shift sits near the mean, so a chunk's chain is a random walk about 0 whose rounding is measured against sum |c_a c_b|; the
        worst of B^2 such walks grows with B.
  y     worst 11.97 (at R200-B256-K256-P16; 6.1 at R130-B65-K33-P33), 4 x 11.97 = 47.9, so K_Y = 64.

Conditions on the END-TO-END cases (R, B, C) of ``E2E_CASES``, asserted on the float64 run alone:
  planted  every planted row's rx_score is at least 1.5 x the largest background score.  Measured: 8.2 x at (2000, 31, 3), 4.25 x at
           (2000, 8, 3), at the builder's seed 1 (seeds 1..5: 8.2 .. 14.0 and 4.0 .. 5.0).
  level    the background's mean score / B is within 0.85 .. 1.05.  Measured 0.930 and 0.904.  (With this builder (600, 4, 2) does not
           qualify: five planted rows among 520 on 4 bands take 0.71 .. 0.79 of the trace, so it is not a case.)
Teeth, on every projection case with valid rows: at least 90 % of them have |y_0| above 16 x their own y bound.  Measured: 1.0 in
every case (|y_0| is of order 1, its bound of order 1e-4).
The noise-free case has 24 of its 31 eigenvalues on the floor: the background spans 2 directions and the 5 planted rows one each."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from library_f64 import make_library
from rays_f64 import TEETH, TINY, U  # noqa: F401

CH = 1024  # UMHS_GRAM_CHUNK
K_G = 128.0
K_Y = 64.0
MIN_TEETH = 0.9
FLOOR = 1e-6

GRAM_CASES = [(0, 5), (1, 1), (63, 2), (257, 31), (130, 33), (1025, 65), (2 * CH + 5, 31), (1100, 141), (600, 256)]
SPLIT_CASE, SPLIT_AT = (2 * CH + 5, 31), 777  # accumulated by two calls: rows [0, 777) and [777, R)
STRIDED_CASE = (130, 33)
# (R, B, K, P, sigma): the last one is noise-free with C = 3, so most of its eigenvalues sit on the floor
PROJECT_CASES = [(0, 5, 5, 0, 0.01), (1, 1, 1, 1, 0.01), (257, 2, 2, 2, 0.01), (300, 31, 31, 3, 0.01), (130, 65, 33, 33, 0.01),
                 (67, 141, 141, 0, 0.01), (200, 256, 256, 16, 0.01), (300, 31, 31, 3, 0.0)]
E2E_CASES = [(2000, 31, 3), (2000, 8, 3)]  # (R, B, C)


def gram_id(c) -> str:
    return f"R{c[0]}-B{c[1]}"


def project_id(c) -> str:
    return f"R{c[0]}-B{c[1]}-K{c[2]}-P{c[3]}" + ("-noisefree" if c[4] == 0 else "")


@functools.lru_cache(maxsize=None)
def make_rows(R: int, B: int, C: int = 3, sigma: float = 0.01, seed: int = 1, planted: int = 5) -> Dict:
    """Background rows: Dirichlet mixtures of C smooth endmembers (library_f64.make_library) plus Gaussian noise ``sigma``; ``planted``
    rows (when R >= 64) are 0.5 row + 0.5 foreign + noise.  When R >= 16: a run of rows with accumulation = 0.2, one row with a NaN and
    one with an Inf.  ``valid``: finite and accumulation > 0.5; ``finite``: finite alone (what the projection looks at)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + 3 * B + C)
    E = make_library(C, B, g).double()
    w = -torch.log(torch.rand(R, C, generator=g, dtype=torch.float64).clamp_min(1e-12))
    x = (w / w.sum(1, keepdim=True).clamp_min(1e-300)) @ E + sigma * torch.randn(R, B, generator=g, dtype=torch.float64)
    plant = torch.zeros(R, dtype=torch.bool)
    if R >= 64 and planted > 0:
        at = torch.tensor([2 + k * ((R // 3 - 2) // planted) for k in range(planted)])
        foreign = make_library(planted, B, g).double()
        x[at] = 0.5 * x[at] + 0.5 * foreign + sigma * torch.randn(planted, B, generator=g, dtype=torch.float64)
        plant[at] = True
    x = x.float()
    accumulation = torch.ones(R)
    if R >= 16:
        z0 = R // 3
        accumulation[z0:z0 + max(2, R // 8)] = 0.2
        x[R - 1, B // 2] = float("nan")
        x[R - 2, B - 1] = float("inf")
    finite = torch.isfinite(x).all(1)
    valid = finite & (accumulation > 0.5)
    shift = x[valid][:8].mean(0) if bool(valid.any()) else torch.zeros(B)
    return dict(R=R, B=B, C=C, x=x, accumulation=accumulation, finite=finite, valid=valid, planted=plant & valid, shift=shift.float())


# ---- gram --------------------------------------------------------------------------------------------------------------------- #
def gram_oracle(case: Dict, dtype=torch.float32, shift: Optional[torch.Tensor] = None, splits: Sequence[int] = (), count_invalid: int = -1,
                drop_chunk: int = -1) -> torch.Tensor:
    """The statement: acc float64 [1 + B + B B].  ``splits``: row indices at which a new call (and so a new chunking) starts.
    Planted faults: ``count_invalid`` = an invalid row index counted (and summed as zeros); ``drop_chunk`` = a chunk's partial dropped."""
    R, B = case["R"], case["B"]
    shift = case["shift"] if shift is None else shift
    x = torch.where(case["valid"][:, None], case["x"], torch.zeros_like(case["x"]))  # (invalid rows are skipped below)
    c = x.to(dtype) - shift.to(dtype)
    acc = torch.zeros(1 + B + B * B, dtype=torch.float64)
    bounds = [0, *splits, R]
    chunk = 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for c0 in range(lo, hi, CH):
            g, s, n = torch.zeros(B, B, dtype=dtype), torch.zeros(B, dtype=dtype), 0
            for r in range(c0, min(c0 + CH, hi)):
                if bool(case["valid"][r]):
                    g = g + c[r][:, None] * c[r][None, :]
                    s = s + c[r]
                    n += 1
                elif r == count_invalid:
                    n += 1
            if chunk != drop_chunk:
                acc[0] += n
                acc[1:1 + B] += s.double()
                acc[1 + B:] += g.double().reshape(-1)
            chunk += 1
    return acc


def gram_ref64(case: Dict, shift: Optional[torch.Tensor] = None) -> Dict:
    """float64 on the float32 inputs: n, s [B], G [B,B] and the magnitudes sum |c_b| [B], sum |c_a c_b| [B,B]."""
    shift = case["shift"] if shift is None else shift
    c = case["x"][case["valid"]].double() - shift.double()
    return dict(n=int(case["valid"].sum()), s=c.sum(0), G=c.T @ c, smag=c.abs().sum(0), gmag=c.abs().T @ c.abs())


@functools.lru_cache(maxsize=None)
def gram_reference(R: int, B: int) -> Tuple[Dict, Dict]:
    """(case, float64 run), computed once per shape and shared; neither is to be changed."""
    case = make_rows(R, B)
    return case, gram_ref64(case)


def _ratio(d: torch.Tensor, bound_unit: torch.Tensor) -> float:
    """max over elements of d / (u x magnitude), 0 where d == 0, inf where not a number."""
    if d.numel() == 0:
        return 0.0
    r = torch.where(d == 0, torch.zeros_like(d), d / (U * bound_unit))
    return float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())


def check_gram(case: Dict, acc, r64: Dict, K: float = K_G, report: Optional[Dict] = None) -> List[str]:
    """Every gram rule of the module docstring; report = {"sums", "gram"}: the worst ratios."""
    B = case["B"]
    acc = acc.detach().cpu()
    if acc.dtype != torch.float64 or tuple(acc.shape) != (1 + B + B * B,):
        return [f"acc is {acc.dtype} {tuple(acc.shape)}, want float64 {(1 + B + B * B,)}"]
    fails: List[str] = []
    if float(acc[0]) != float(r64["n"]):
        fails.append(f"count {float(acc[0])}, want {r64['n']}")
    s, G = acc[1:1 + B], acc[1 + B:].reshape(B, B)
    if not torch.equal(G.view(torch.int64), G.T.contiguous().view(torch.int64)):
        fails.append(f"G is not symmetric bit for bit at {int((G != G.T).sum())} places")
    worst_s, worst_g = _ratio((s - r64["s"]).abs(), r64["smag"]), _ratio((G - r64["G"]).abs(), r64["gmag"])
    if report is not None:
        report.update(sums=worst_s, gram=worst_g)
    if worst_s > K:
        fails.append(f"sums: {worst_s:.3g} u sum|c| (K = {K:g})")
    if worst_g > K:
        fails.append(f"gram: {worst_g:.3g} u sum|c_a c_b| (K = {K:g})")
    return fails


# ---- whitening and projection ------------------------------------------------------------------------------------------------- #
def whiten64(mean: np.ndarray, cov: np.ndarray, floor: float = FLOOR) -> Tuple[np.ndarray, np.ndarray]:
    """The recipe of SceneStatistics.whitening, written out again: (W [B,B], eigenvalues) in float64; identity for a zero covariance."""
    lam, V = np.linalg.eigh(cov)
    lam, V = lam[::-1].copy(), V[:, ::-1].T.copy()
    if not lam[0] > 0:
        return np.eye(cov.shape[0]), np.ones(cov.shape[0])
    lam = np.maximum(lam, floor * lam[0])
    V = V * np.where(V[np.arange(V.shape[0]), np.abs(V).argmax(1)] < 0, -1.0, 1.0)[:, None]
    return V / np.sqrt(lam)[:, None], lam


def stats64(x: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """(mean, biased covariance) of rows in float64; zeros for fewer than two rows."""
    x = x.double().numpy()
    if x.shape[0] < 2:
        return np.zeros(x.shape[1]), np.zeros((x.shape[1], x.shape[1]))
    m = x.mean(0)
    return m, (x - m).T @ (x - m) / x.shape[0]


@functools.lru_cache(maxsize=None)
def make_project_case(R: int, B: int, K: int, P: int, sigma: float = 0.01) -> Dict:
    """The rows of ``make_rows`` with the float32 mean and the first K whitening rows of their own valid rows' float64 statistics."""
    rows = make_rows(R, B, 3, sigma)
    mean, cov = stats64(rows["x"][rows["valid"]])
    W, lam = whiten64(mean, cov)
    return dict(rows, K=K, P=P, mean=torch.from_numpy(mean).float(), W=torch.from_numpy(W[:K].copy()).float().contiguous(), lam=lam)


def project_oracle(case: Dict, dtype=torch.float32, no_mean: bool = False, drop_last: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The statement in ``dtype``: (components [R,P], score [R]).  Planted faults: ``no_mean`` = the mean is not subtracted; ``drop_last``
    = the score is summed over K - 1 components."""
    R, B, K, P = case["R"], case["B"], case["K"], case["P"]
    x = torch.where(case["finite"][:, None], case["x"], torch.zeros_like(case["x"])).to(dtype)
    c = x if no_mean else x - case["mean"].to(dtype)
    W = case["W"].to(dtype)
    y = torch.zeros(R, K, dtype=dtype)
    for b in range(B):
        y = y + c[:, b:b + 1] * W[None, :, b]
    score = torch.zeros(R, dtype=dtype)
    for k in range(K - (1 if drop_last else 0)):
        score = score + y[:, k] * y[:, k]
    dead = ~case["finite"]
    y[dead] = 0
    score[dead] = 0
    return y[:, :P].contiguous(), score


def project_ref64(case: Dict) -> Dict:
    """float64 on the float32 inputs: y [R,K], its magnitude sum_b |c_b W_kb| + tiny, score [R] (rows that are not finite hold zeros)."""
    x = torch.where(case["finite"][:, None], case["x"], torch.zeros_like(case["x"])).double()
    c, W = x - case["mean"].double(), case["W"].double()
    y = c @ W.T
    return dict(y=y, ymag=c.abs() @ W.abs().T + TINY, score=(y * y).sum(1))


@functools.lru_cache(maxsize=None)
def project_reference(R: int, B: int, K: int, P: int, sigma: float = 0.01) -> Tuple[Dict, Dict]:
    case = make_project_case(R, B, K, P, sigma)
    return case, project_ref64(case)


def check_project(case: Dict, components, score, r64: Dict, K: float = K_Y, report: Optional[Dict] = None) -> List[str]:
    """Every projection rule of the module docstring; report = {"y", "score"}: the worst ratios (score: of its own bound)."""
    R, P = case["R"], case["P"]
    components, score = components.detach().cpu(), score.detach().cpu()
    if tuple(components.shape) != (R, P) or tuple(score.shape) != (R,) or components.dtype != torch.float32 or score.dtype != torch.float32:
        return [f"shapes {tuple(components.shape)} / {tuple(score.shape)}, want {(R, P)} / {(R,)} float32"]
    fails: List[str] = []
    dead, live = ~case["finite"], case["finite"]
    if bool((components[dead] != 0).any()) or bool((score[dead] != 0).any()):
        fails.append("a row with a NaN or an Inf did not give exact zeros")
    e = K * U * r64["ymag"][live]
    y64 = r64["y"][live]
    d = (components[live].double() - y64[:, :P]).abs()
    worst_y = _ratio(d, r64["ymag"][live][:, :P])
    sbound = (2 * y64.abs() * e + e * e).sum(1) + K * U * (y64 * y64).sum(1)
    ds = (score[live].double() - r64["score"][live]).abs()
    rs = torch.where(ds == 0, torch.zeros_like(ds), ds / sbound)
    worst_s = float(torch.where(torch.isnan(rs), torch.full_like(rs, float("inf")), rs).max()) if rs.numel() else 0.0
    if report is not None:
        report.update(y=worst_y, score=worst_s)
    if worst_y > K:
        i = int((d / r64["ymag"][live][:, :P]).max(1).values.argmax())
        fails.append(f"y: live row {i}: {worst_y:.3g} u mag (K = {K:g})")
    if worst_s > 1.0:
        fails.append(f"score: live row {int(rs.argmax())}: {worst_s:.3g} x its bound")
    return fails


def teeth(case: Dict, r64: Dict, K: float = K_Y) -> Optional[float]:
    """The share of the valid rows whose |y_0| is above 16 x its own bound; None where there is nothing to measure."""
    v = case["valid"]
    if int(v.sum()) == 0:
        return None
    return float((r64["y"][v][:, 0].abs() > TEETH * K * U * r64["ymag"][v][:, 0]).sum()) / int(v.sum())


# ---- end to end ----------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def e2e_reference(R: int, B: int, C: int) -> Dict:
    """Rows with planted anomalies and the float64 run of the whole chain on them: statistics of the valid rows, whitening, scores."""
    rows = make_rows(R, B, C)
    v = rows["valid"]
    mean, cov = stats64(rows["x"][v])
    W, lam = whiten64(mean, cov)
    y = (rows["x"][v].double().numpy() - mean) @ W.T
    score = torch.zeros(R, dtype=torch.float64)
    score[v] = torch.from_numpy((y * y).sum(1))
    return dict(rows, mean64=mean, cov64=cov, W64=W, lam=lam, score64=score)


def e2e_conditions(ref: Dict) -> Dict:
    """{"margin": smallest planted score / largest background score, "level": background mean score / B}."""
    background = ref["valid"] & ~ref["planted"]
    s = ref["score64"]
    return {"margin": float(s[ref["planted"]].min() / s[background].max()), "level": float(s[background].mean()) / ref["B"]}
