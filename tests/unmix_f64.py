"""Spectral-unmixing cases, their float64 oracle, a float32 restatement of the kernel and the comparator (plain helper module, no tests
in it).  It mirrors tests/statistics_f64.py for csrc/umhs_unmix.hip.

Used by tests/test_hip_unmix.py (the kernel and the model on the GPU) and tests/test_unmix_cpu.py (the oracle against exact enumeration
and scipy, the float32 restatement against the comparator, planted faults; the constants below are re-measured there).

Statement (include/umhs_hip.h, "Spectral unmixing"), on float32 spectra x [R,B] and float32 endmembers E [K,B]:
  G = E E^T and b = E x are the normal equations; a minimises f(a) = 1/2 |x - E^T a|^2 over a >= 0 (NNLS), and sum a = 1 as well (FCLS).
  A row is INVALID when it holds a NaN or an Inf or when sum x^2 is 0 or overflows float32: abundances 0, residual 0, status -1.
  The solver is an active-set method (Lawson-Hanson) on a symmetric sweep tableau of G with two right-hand columns (b and ones):
    sweep(k)   p = M_kk, r = 1 / p; M_ij -= M_ik M_kj r for i, j != k; row k becomes M_kj r (entering) or -M_kj r (leaving); M_kk = -r.
               With P swept in, column b holds u = G_PP^-1 b_P on P and b - G u off P; column ones holds v = G_PP^-1 1 on P, 1 - G v off P.
    solve      lambda = (sum u - 1) / sum v (FCLS; 0 for NNLS), z = u - lambda v on P.
    start      every endmember passive; a = 0 (NNLS), 1 / K (FCLS).
    step       if some z_i <= 0: alpha = min a_i / (a_i - z_i) over them, a += alpha (z - a), the minimiser and whatever is at 0 leave P.
               else a = z, and the index off P of largest w_i = (column b)_i - lambda (column ones)_i enters when w_i > 2^-21 max|b|.
    guard      an endmember that enters and gets z <= 0 at once leaves again and is banned until another one is accepted.
    cap        3 K + 3 solves; a row stopped there returns its last feasible iterate with status -2.
  residual = max(0, sum x^2 - 2 b.a + a.G a) in float32.
The float64 run (the truth, ``solve_f64``) takes the SAME float32 x and E, forms G and b in float64 and runs the same method at a
tolerance of 1e-14; ``brute_force`` enumerates all supports (K <= 6).

RULES for every valid row, u = 2^-24, a* the oracle's optimum, all judged in float64 from the float32 inputs:
  feasible    a finite, a_k >= 0; FCLS: |sum a - 1| <= K_S u K
  objective   f(a) - f(a*) <= K_F u 1/2 |x|^2                      (capped rows included)
  abundance   |a - a*|_inf <= K_A u cond_2(G) max(1, |a*|_inf)
  residual    |residual - |x - E^T a|^2| <= K_R u sum x^2
  status      0 <= status <= 3 K + 3, or -2; at most 2 % of a case's valid rows carry -2
K = 4 x the worst ratio of ``solve_f32`` against ``solve_f64`` over CASES x both modes, rounded up to a power of two.  Measured on the CPU
(tests/test_unmix_cpu.py re-measures and asserts 4 x worst <= K):
  K_S   worst 0.75 (syn-K2-B31-R64, FCLS), 4 x 0.75 = 3, so K_S = 4
  K_F   worst 4.04 (vca_b31-K6-B31-R200, FCLS: a sum that is off by d moves f by lambda d, and lambda is large for a pixel far outside
        the simplex; NNLS stays below 0.05), 4 x 4.04 = 16.1, so K_F = 32
  K_A   worst 1.90 (syn-K1-B2-R1, NNLS; 1.68 at vca_b141-K4-B141-R127; the cases of cond_2(E) > 60 stay below 0.4: u cond_2(G) is a
        worst-case amplification), 4 x 1.90 = 7.6, so K_A = 8
  K_R   worst 26.7 (vca_b128-K9-B128-R130, NNLS; 25.6 at hotdog: the float32 chains of sum x^2 and b over B bands), 4 x 26.7 = 107, so
        K_R = 128
  cap   ``solve_f32`` stops no row at the cap on the committed cases (its longest run is 17 solves at K = 16, cap 51), ``solve_f64`` none.
The kernel on an MI355X (tests/test_hip_unmix.py, ratios OF THE BOUNDS): sum 0.16, objective 0.04, abundance 0.20, residual 0.20 at
worst over the 30 runs; no row at the cap."""
from __future__ import annotations

import functools
import itertools
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

U = 2.0 ** -24
NNLS, FCLS = 0, 1
MODES = (NNLS, FCLS)
K_S = 4.0
K_F = 32.0
K_A = 8.0
K_R = 128.0
MAX_CAP_SHARE = 0.02
TOL_F32 = 2.0 ** -21  # the kernel's optimality tolerance, relative to max|b|
TOL_F64 = 1e-14
SIGMA = 0.01
MAX_SYNTHETIC_COND = 100.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (endmember set, K, B, R, layout): ``slice`` = a column slice of a wider array (stride B + 5, starting 3 floats in)
CASES = [("syn", 1, 2, 1, "rows"), ("syn", 2, 2, 63, "rows"), ("syn", 2, 31, 64, "rows"), ("syn", 6, 33, 65, "rows"),
         ("syn", 6, 31, 0, "rows"), ("syn", 15, 50, 129, "rows"), ("syn", 16, 90, 257, "rows"), ("syn", 16, 128, 65, "rows"),
         ("hotdog", 4, 141, 1000, "slice"), ("vca_b31", 6, 31, 200, "rows"), ("vca_b128", 9, 128, 130, "rows"),
         ("vca_b141", 4, 141, 127, "rows"), ("syn", 15, 160, 63, "rows"), ("syn", 16, 256, 200, "rows"), ("syn", 6, 256, 64, "slice")]
SLICE_PAD, SLICE_AT = 5, 3


def unmix_id(c) -> str:
    return f"{c[0]}-K{c[1]}-B{c[2]}-R{c[3]}" + ("-slice" if c[4] == "slice" else "")


def solve_cap(K: int) -> int:
    return 3 * K + 3


# ---- endmembers and rows ------------------------------------------------------------------------------------------------------ #
def synthetic_endmembers(K: int, B: int, seed: int = 1) -> np.ndarray:
    """float32 [K,B]: a Gaussian bump per endmember at (k + 1/2) / K over a floor in 0.15 .. 0.25, plus a small sinusoid."""
    g = np.random.default_rng(100 * seed + 7 * K + B)
    p = (np.arange(B) + 0.5) / B
    c = (np.arange(K) + 0.5) / K
    width = 0.85 / K
    floor = g.uniform(0.15, 0.25, (K, 1))
    bump = 0.7 * np.exp(-0.5 * ((p[None, :] - c[:, None]) / width) ** 2)
    wave = 0.03 * np.sin(2 * np.pi * (g.uniform(1.0, 3.0, (K, 1)) * p[None, :] + g.uniform(0.0, 1.0, (K, 1))))
    return (floor + bump + wave).astype(np.float32)


def endmembers(kind: str, K: int, B: int) -> np.ndarray:
    if kind == "syn":
        E = synthetic_endmembers(K, B)
        assert np.linalg.cond(E.astype(np.float64)) <= MAX_SYNTHETIC_COND, (K, B, np.linalg.cond(E.astype(np.float64)))
    elif kind == "hotdog":
        E = np.load(os.path.join(GOLDEN, "g7_endmembers_hotdog.npy")).astype(np.float32)
    else:
        E = np.load(os.path.join(GOLDEN, f"g6_{kind}.npz"))["Ae_f32"].T.astype(np.float32)
    assert E.shape == (K, B), (kind, E.shape)
    return np.ascontiguousarray(E)


def gram32(E: np.ndarray) -> np.ndarray:
    """What the entry point takes: E E^T formed in float64 from the float32 E, rounded once."""
    E = np.asarray(E, np.float32).astype(np.float64)
    return (E @ E.T).astype(np.float32)


def make_rows(E: np.ndarray, R: int, seed: int = 1) -> np.ndarray:
    """float32 [R,B]: the row kinds of the module's cases, cycled over r % 10; valid rows carry Gaussian noise of sigma 0.01, except
    the exact endmembers (kind 5)."""
    K, B = E.shape
    g = np.random.default_rng(1000 * seed + 13 * K + 3 * B + R)
    E64 = E.astype(np.float64)
    x = np.zeros((R, B))
    for r in range(R):
        kind, a = r % 10, np.zeros(K)
        i, j = int(g.integers(K)), int(g.integers(K))
        if kind == 0 or kind == 5:  # a pure pixel / an exact endmember
            a[i] = 1.0
        elif kind in (1, 9):  # a two-endmember mix
            t = g.uniform(0.1, 0.9)
            a[i] += t
            a[j] += 1.0 - t
        elif kind in (2, 6):  # an interior Dirichlet mix
            a = g.dirichlet(np.ones(K))
        elif kind == 3:  # a scaled mix: tells NNLS from FCLS
            a = g.dirichlet(np.ones(K)) * g.uniform(0.5, 1.5)
        elif kind == 4:  # outside the simplex, several constraints active
            a = g.dirichlet(np.ones(K)) + 0.6 * g.standard_normal(K) / np.sqrt(K)
            a += (1.0 - a.sum()) / K
        elif kind == 8:  # outside along one edge
            a[i] += 1.3
            a[j] -= 0.3
        x[r] = a @ E64
        if kind not in (5, 7):
            x[r] += SIGMA * g.standard_normal(B)
        if kind == 7:  # the invalid rows: zeros, a NaN, an Inf, an overflowing sum of squares
            which = (r // 10) % 4
            x[r] = g.dirichlet(np.ones(K)) @ E64
            if which == 0:
                x[r] = 0.0
            elif which == 1:
                x[r, B // 2] = np.nan
            elif which == 2:
                x[r, B - 1] = np.inf
            else:
                x[r, 0] = 1e30
    return x.astype(np.float32)


def row_valid(x: np.ndarray) -> np.ndarray:
    """The kernel's rule on float32 rows: finite, and the float32 sum of squares neither 0 nor overflowing."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        ss = (x.astype(np.float64) ** 2).sum(1)
    return np.isfinite(x).all(1) & (ss > 0) & (ss < 3.0e38)


# ---- the solvers ---------------------------------------------------------------------------------------------------------------- #
def brute_force(G: np.ndarray, b: np.ndarray, mode: int) -> np.ndarray:
    """The exact optimum in float64 by enumeration of every support (K <= 6): the feasible stationary point of least objective."""
    G, b = np.asarray(G, np.float64), np.asarray(b, np.float64)
    K = b.shape[0]
    best, best_f = np.zeros(K), 0.0 if mode == NNLS else np.inf
    for n in range(1, K + 1):
        for S in itertools.combinations(range(K), n):
            S = list(S)
            Gs, bs = G[np.ix_(S, S)], b[S]
            if mode == FCLS:
                A = np.block([[Gs, np.ones((n, 1))], [np.ones((1, n)), np.zeros((1, 1))]])
                z = np.linalg.solve(A, np.concatenate([bs, [1.0]]))[:n]
            else:
                z = np.linalg.solve(Gs, bs)
            if (z < 0).any():
                continue
            f = 0.5 * z @ Gs @ z - bs @ z
            if f < best_f:
                best_f, best = f, np.zeros(K)
                best[S] = z
    return best


def active_set(G, b, mode: int, dtype, tol_rel: float, fault: Optional[str] = None) -> Tuple[np.ndarray, int]:
    """The method of the module docstring on one row in ``dtype`` -> (a [K], status).  Planted faults: ``clip`` = the all-passive
    solution with its negatives set to 0 and no re-solve; ``no_multiplier`` = nothing ever enters again; ``lambda_sign`` = z = u + lambda v."""
    f = dtype
    G, b = np.asarray(G, f), np.asarray(b, f)
    K = b.shape[0]
    M, cb, c1 = G.copy(), b.copy(), np.ones(K, f)
    a = np.full(K, f(1) / f(K) if mode == FCLS else f(0), f)
    P, banned = np.zeros(K, bool), np.zeros(K, bool)
    pending, entering, solves = list(range(K)), -1, 0
    tol = f(tol_rel) * np.abs(b).max()

    def sweep(k):
        p = M[k, k]
        if not P[k] and not p > 0:  # a pivot that is not positive cannot enter
            banned[k] = True
            return
        r = f(1) / p
        col, bk, ok = M[:, k].copy(), cb[k], c1[k]
        t = col * r
        M[:, :] = M - np.outer(t, col)
        cb[:] = cb - t * bk
        c1[:] = c1 - t * ok
        s = f(-1) if P[k] else f(1)
        M[k, :] = t * s
        M[:, k] = t * s
        M[k, k] = -r
        cb[k], c1[k] = bk * r * s, ok * r * s
        P[k] = not P[k]

    with np.errstate(all="ignore"):
        while True:
            while pending:
                sweep(pending.pop(0))
            if solves >= solve_cap(K):
                return a, -2
            solves += 1
            lam = f(0)
            if mode == FCLS:
                lam = (cb[P].sum(dtype=f) - f(1)) / c1[P].sum(dtype=f)
            z = np.where(P, cb + lam * c1 if fault == "lambda_sign" else cb - lam * c1, f(0)).astype(f)
            if fault == "clip":
                return np.maximum(z, 0).astype(f), solves
            if entering >= 0:
                t, entering = entering, -1
                if P[t] and not z[t] > 0:
                    pending, banned[t] = [t], True
                    continue
                if P[t]:
                    banned[:] = False
            neg = P & ~(z > 0)
            if neg.any():
                den = a - z
                ratio = np.where(neg, np.where(den > 0, a / np.where(den > 0, den, 1), f(0)), f(2)).astype(f)
                imin = int(np.argmin(ratio))
                alpha = min(ratio[imin], f(1))
                a = np.where(P, np.maximum(a + alpha * (z - a), f(0)), f(0)).astype(f)
                a[imin] = 0
                pending = [int(i) for i in np.nonzero(neg & (a <= 0))[0]]
                continue
            a = z
            w = np.where(~P & ~banned, cb - lam * c1, -np.inf)
            t = int(np.argmax(w))
            if fault == "no_multiplier" or not w[t] > tol:
                return a, solves
            pending, entering = [t], t


def _solve(E, x, mode, dtype, tol, fault=None):
    E, x = np.asarray(E, np.float32), np.asarray(x, np.float32)
    R, K = x.shape[0], E.shape[0]
    valid = row_valid(x)
    if dtype == np.float64:
        G = E.astype(np.float64) @ E.astype(np.float64).T
    else:
        G = gram32(E)
    a, res, status = np.zeros((R, K), dtype), np.zeros(R, dtype), np.full(R, -1, np.int32)
    xv = np.where(valid[:, None], x, 0).astype(dtype)
    bs, half = np.zeros((R, K), dtype), [np.zeros(R, dtype), np.zeros(R, dtype)]
    for k in range(E.shape[1]):  # the chains over the bands ascending; ss = the even bands' chain + the odd bands'
        bs = bs + xv[:, k:k + 1] * E[:, k].astype(dtype)[None, :]
        half[k & 1] = half[k & 1] + xv[:, k] * xv[:, k]
    ss = half[0] + half[1]
    for r in np.nonzero(valid)[0]:
        b = bs[r]
        a[r], status[r] = active_set(G, b, mode, dtype, tol, fault)
        a[r] = np.where((a[r] > 0) & np.isfinite(a[r]), a[r], 0)
        res[r] = max(dtype(0), ss[r] - dtype(2) * (b @ a[r]) + a[r] @ (G.astype(dtype) @ a[r]))
    return a, res, status


def solve_f64(E, x, mode: int):
    """The truth: (abundances [R,K] float64, residual [R], status [R]) from the float32 E and x."""
    return _solve(E, x, mode, np.float64, TOL_F64)


def solve_f32(E, x, mode: int, fault: Optional[str] = None):
    """The kernel's algorithm restated in numpy float32 (one rounding per operation; the kernel contracts to fmaf)."""
    return _solve(E, x, mode, np.float32, TOL_F32, fault)


# ---- cases ---------------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def make_case(kind: str, K: int, B: int, R: int, layout: str = "rows") -> Dict:
    """E float32 [K,B], G float32 [K,K], x float32 [R,B] (a view into ``wide`` for a slice case), valid [R], cond_2(G)."""
    E = endmembers(kind, K, B)
    rows = make_rows(E, R)
    if layout == "slice":
        wide = np.full((R, B + SLICE_PAD), np.nan, np.float32)  # (columns outside the slice must never be read)
        wide[:, SLICE_AT:SLICE_AT + B] = rows
        x = wide[:, SLICE_AT:SLICE_AT + B]
    else:
        wide, x = rows, rows
    E64 = E.astype(np.float64)
    return dict(kind=kind, K=K, B=B, R=R, layout=layout, E=E, G=gram32(E), x=x, wide=wide, valid=row_valid(x),
                cond=float(np.linalg.cond(E64 @ E64.T)))


@functools.lru_cache(maxsize=None)
def reference(kind: str, K: int, B: int, R: int, layout: str, mode: int) -> Tuple[Dict, Dict]:
    """(case, float64 run), computed once per case and mode and shared; neither is to be changed."""
    case = dict(make_case(kind, K, B, R, layout), mode=mode)
    a, res, status = solve_f64(case["E"], case["x"], mode)
    return case, dict(a=a, residual=res, status=status)


def objective(E64: np.ndarray, x64: np.ndarray, a: np.ndarray) -> np.ndarray:
    d = x64 - a @ E64
    return 0.5 * (d * d).sum(1)


def check(case: Dict, abundances, residual, status, report: Optional[Dict] = None, ref: Optional[Dict] = None) -> List[str]:
    """Every rule of the module docstring; ``report`` gets the worst ratios {"sum", "objective", "abundance", "residual"} OF THEIR BOUNDS
    (below 1 passes) and "cap_share".  ``residual`` / ``status`` may be None (not checked)."""
    K, R, mode = case["K"], case["R"], case["mode"]
    if ref is None:
        ref = reference(case["kind"], K, case["B"], R, case["layout"], mode)[1]
    a = np.asarray(abundances)
    if a.shape != (R, K) or a.dtype not in (np.float32, np.float64):
        return [f"abundances are {a.dtype} {a.shape}, want float32 {(R, K)}"]
    fails: List[str] = []
    v, dead = case["valid"], ~case["valid"]
    if (a[dead] != 0).any() or np.signbit(a[dead]).any():
        fails.append("an invalid row did not give exact zeros")
    if residual is not None and (np.asarray(residual)[dead] != 0).any():
        fails.append("an invalid row has a residual")
    if status is not None:
        status = np.asarray(status)
        if (status[dead] != -1).any():
            fails.append("an invalid row's status is not -1")
        sv = status[v]
        if ((sv < 0) & (sv != -2)).any() or (sv > solve_cap(K)).any():
            fails.append(f"status outside 0..{solve_cap(K)} / -2 on a valid row")
        share = float((sv == -2).mean()) if sv.size else 0.0
        if report is not None:
            report["cap_share"] = share
        if share > MAX_CAP_SHARE:
            fails.append(f"{share:.3%} of the valid rows stopped at the cap (at most {MAX_CAP_SHARE:.0%})")
    if report is not None:
        report.update(sum=0.0, objective=0.0, abundance=0.0, residual=0.0)
    if not v.any():
        return fails
    E64, x64 = case["E"].astype(np.float64), case["x"][v].astype(np.float64)
    av, star = a[v].astype(np.float64), ref["a"][v]
    if not np.isfinite(av).all() or (av < 0).any() or np.signbit(av).any():
        fails.append("an abundance is negative or not finite")
        return fails
    ss = (x64 * x64).sum(1)
    r_sum = float((np.abs(av.sum(1) - 1.0) / (K_S * U * K)).max()) if mode == FCLS else 0.0
    r_obj = float(((objective(E64, x64, av) - objective(E64, x64, star)) / (K_F * U * 0.5 * ss)).max())
    r_ab = float((np.abs(av - star).max(1) / (K_A * U * case["cond"] * np.maximum(1.0, np.abs(star).max(1)))).max())
    worst = dict(sum=r_sum, objective=max(r_obj, 0.0), abundance=r_ab)
    if residual is not None:
        d = x64 - av @ E64
        worst["residual"] = float((np.abs(np.asarray(residual)[v].astype(np.float64) - (d * d).sum(1)) / (K_R * U * ss)).max())
        if (np.asarray(residual)[v] < 0).any():
            fails.append("a residual is negative")
    if report is not None:
        report.update(worst)
    for name, ratio in worst.items():
        if not ratio <= 1.0:
            fails.append(f"{name}: {ratio:.3g} x its bound")
    return fails
