"""Sparse-unmixing cases, their float64 truth, a float32 restatement of the kernel's iteration and the comparator (plain helper module,
no tests in it).  It mirrors tests/unmix_f64.py for csrc/umhs_sparse.hip.

Used by tests/test_hip_sparse.py (the kernel on the GPU) and tests/test_sparse_cpu.py (the truth against exact enumeration and its own
KKT conditions, the restatement against the comparator, planted faults, the mu rule; the constants below are re-measured there).

Statement (include/umhs_hip.h, "Sparse unmixing"), on float32 spectra x [R,B] and a float32 library A [L,B]:
  per row a minimises f(a) = 1/2 |x - A^T a|^2 + lambda_r sum a over a >= 0, lambda_r = lambda sqrt(ss), ss the sum of squares of x.
  A row is INVALID when it holds a NaN or an Inf or when ss is 0 or overflows float32: abundances 0, residual 0, status -1.
  Host, float64, each rounded to float32 once: G = A A^T, F = (G + mu I)^-1, Q = F A, M = mu F, theta = lambda / mu.
  Iteration, float32, from z = d = 0, c = Q x:
    a_k  = the fmaf chain  fmaf(M[k,j], z_j - d_j, .)  from c_k over j in the order ``chain_order(L)``
    t_k  = a_k + d_k;  u_k = t_k - tau, tau = theta * sqrtf(ss);  z'_k = u_k if u_k > 0 else +0;  d'_k = t_k - z'_k
    done after the first iteration with  max|a - z'| <= eps s  and  max|z' - z| <= eps s,  s = max|c|;  a done row is frozen, its
    result is z' and its status the iteration count; a row that reaches max_iterations returns its last z' with status -2.
  residual = max(0, fmaf(-2, b.z, ss) + z.(G z)), b = A x, G rounded to float32.
The truth (``solve_f64``) takes the SAME float32 x and A: the non-negative lasso is NNLS with b replaced by b - lambda_r 1, solved by
``unmix_f64.active_set`` in float64 at 1e-14; ``brute_force`` enumerates all supports (L <= 6), ``kkt_violation`` judges any L.
``solve_admm_f64`` is the iteration above in float64: it separates what eps costs from what float32 costs.

RULES for every valid row, u = 2^-24, a* the truth, all judged in float64 from the float32 inputs; e = eps + L u:
  feasible    a finite, a_k >= +0, the sign bit never set
  objective   f(a) - f(a*) <= K_F e 1/2 |x|^2                                          (capped rows included)
  abundance   |a - a*|_inf <= K_A e cond_2(G_SS) |x| / sigma_max(A), S the truth's support, on the rows with cond_2(G_SS) <=
              MAX_SUPPORT_COND (an error of e |x| sigma_max in the gradient, through G_SS^-1)
  residual    |residual - |x - A^T a|^2| <= K_R u ss
  status      1 <= status <= max_iterations, or -2; at most 2 % of a case's valid rows carry -2
K = 4 x the worst ratio of ``solve_f32`` against ``solve_f64`` over CASES at the defaults (lambda 1e-3, eps 1e-4, 400 iterations, mu
auto), rounded up to a power of two.  Measured on the CPU (tests/test_sparse_cpu.py re-measures and asserts 4 x worst <= K):
  K_F   worst 0.0212 (syn-L128-B141-R129-slice), 4 x 0.0212 = 0.085, so K_F = 1/8
  K_A   worst 174 (syn-L128-B141-R129-slice; 63 at syn-L64-B128-R65, below 30 elsewhere: what the stopping rule leaves, the float64
        iteration gives 173), 4 x 174 = 696, so K_A = 1024
  K_R   worst 22.7 (syn-L128-B256-R257: the float32 chains of ss and b over 256 bands), 4 x 22.7 = 91, so K_R = 128
  cap   ``solve_f32`` stops 1.7 % of vca_b128-L9-B128-R65 at the cap (one row), 0.9 % of syn-L128-B141-R129-slice, 0.4 % of
        syn-L128-B256-R257 and none elsewhere; ``solve_admm_f64`` the same rows; the truth none.
The kernel on an MI355X (tests/test_hip_sparse.py, ratios OF THE BOUNDS): objective 0.17, abundance 0.17, residual 0.18 at worst over
the 15 cases; the rows at the cap are those of ``solve_f32``.
The mu rule: mu = RHO trace(G) / L; RHO is the one of RHOS with the fewest mean iterations of ``solve_admm_f64`` over CASES
(``mu_table``; the table is in DESIGN.md and re-measured by tests/test_sparse_cpu.py)."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

import unmix_f64 as UF

U = UF.U
SIGMA = UF.SIGMA
MAX_SYNTHETIC_COND = UF.MAX_SYNTHETIC_COND
MAX_SUPPORT_COND = 1.0e4
MAX_CAP_SHARE = 0.02
K_F = 0.125
K_A = 1024.0
K_R = 128.0
LAMBDA = 1e-3
EPSILON = 1e-4
MAX_ITERATIONS = 400
RHOS = (0.01, 0.03, 0.1, 0.3, 1.0)
RHO = 0.1
MAX_ENTRIES, MAX_BANDS = 128, 256
GOLDEN = UF.GOLDEN
SLICE_PAD, SLICE_AT = UF.SLICE_PAD, UF.SLICE_AT

# (library, L, B, R, layout): ``slice`` = a column slice of a wider array (stride B + 5, starting 3 floats in)
CASES = [("syn", 1, 2, 1, "rows"), ("syn", 2, 2, 31, "rows"), ("syn", 31, 31, 32, "rows"), ("syn", 32, 33, 33, "rows"),
         ("syn", 33, 128, 63, "rows"), ("syn", 64, 128, 65, "rows"), ("syn", 65, 141, 129, "rows"), ("syn", 96, 141, 65, "rows"),
         ("syn", 128, 256, 257, "rows"), ("syn", 128, 141, 129, "slice"), ("syn", 6, 31, 0, "rows"), ("hotdog", 4, 141, 129, "slice"),
         ("vca_b31", 6, 31, 63, "rows"), ("vca_b128", 9, 128, 65, "rows"), ("vca_b141", 4, 141, 33, "rows")]


def sparse_id(c) -> str:
    return f"{c[0]}-L{c[1]}-B{c[2]}-R{c[3]}" + ("-slice" if c[4] == "slice" else "")


# ---- libraries and rows --------------------------------------------------------------------------------------------------------- #
def synthetic_library(L: int, B: int, seed: int = 1) -> np.ndarray:
    """float32 [L,B]: smooth positive random spectra (a floor, two Gaussian bumps and band noise) whose singular values are then
    raised to sigma_max / (0.9 MAX_SYNTHETIC_COND), so that cond_2(A) stays under the cap whatever L <= B."""
    assert L <= B
    g = np.random.default_rng(100 * seed + 7 * L + B)
    p = (np.arange(B) + 0.5) / B
    A = g.uniform(0.1, 0.3, (L, 1)) + 0.15 * g.uniform(0.0, 1.0, (L, B))
    for _ in range(2):
        A = A + g.uniform(0.2, 0.6, (L, 1)) * np.exp(-0.5 * ((p[None, :] - g.uniform(0.0, 1.0, (L, 1))) / g.uniform(0.05, 0.2, (L, 1))) ** 2)
    u, s, vt = np.linalg.svd(A, full_matrices=False)
    A = (u * np.maximum(s, s[0] / (0.9 * MAX_SYNTHETIC_COND))) @ vt
    return np.ascontiguousarray(A.astype(np.float32))


def library(kind: str, L: int, B: int) -> np.ndarray:
    if kind == "syn":
        A = synthetic_library(L, B)
        assert np.linalg.cond(A.astype(np.float64)) <= MAX_SYNTHETIC_COND, (L, B, np.linalg.cond(A.astype(np.float64)))
        return A
    return UF.endmembers(kind, L, B)


def make_rows(A: np.ndarray, R: int, seed: int = 1) -> np.ndarray:
    """float32 [R,B]: mixes of 1 to 4 entries (weights 0.2 .. 1) plus Gaussian noise of SIGMA, cycled over r % 10: kinds 0 .. 6 are
    mixes of 1 + r % 4 entries, 7 is invalid (zeros, a NaN, an Inf, an overflowing sum of squares), 8 a mix scaled by 1e-3 and 9 one
    scaled by 1e3 (noise and all)."""
    L, B = A.shape
    g = np.random.default_rng(1000 * seed + 13 * L + 3 * B + R)
    A64 = A.astype(np.float64)
    x = np.zeros((R, B))
    for r in range(R):
        kind, n = r % 10, min(L, 1 + r % 4)
        a = np.zeros(L)
        a[g.choice(L, n, replace=False)] = g.uniform(0.2, 1.0, n)
        x[r] = a @ A64 + SIGMA * g.standard_normal(B)
        if kind == 7:
            which = (r // 10) % 4
            if which == 0:
                x[r] = 0.0
            elif which == 1:
                x[r, B // 2] = np.nan
            elif which == 2:
                x[r, B - 1] = np.inf
            else:
                x[r, 0] = 1e30
        elif kind == 8:
            x[r] *= 1e-3
        elif kind == 9:
            x[r] *= 1e3
    return x.astype(np.float32)


row_valid = UF.row_valid


# ---- the host preparation --------------------------------------------------------------------------------------------------------- #
def auto_mu(A: np.ndarray, rho: float = RHO) -> float:
    A64 = np.asarray(A, np.float32).astype(np.float64)
    return float(rho * (A64 * A64).sum() / A64.shape[0])


def prepare(A: np.ndarray, lam: float, mu: float) -> Dict:
    """float64 (G, F, Q, M, theta) from the float32 A, and their float32 roundings (G32, Q32, M32, theta32)."""
    A64 = np.asarray(A, np.float32).astype(np.float64)
    L = A64.shape[0]
    G = A64 @ A64.T
    F = np.linalg.inv(G + mu * np.eye(L))
    F = 0.5 * (F + F.T)
    Q, M, theta = F @ A64, mu * F, lam / mu
    return dict(A=A64, G=G, Q=Q, M=M, theta=theta, G32=G.astype(np.float32), Q32=Q.astype(np.float32), M32=M.astype(np.float32),
                theta32=np.float32(theta), mu=mu, lam=lam)


def chain_order(L: int) -> np.ndarray:
    """The order of j in a_k's chain: tiles of 32 entries ascending; within a tile, for e = 0 .. 15 the entry (e & 3) + 8 (e >> 2) and
    then that entry + 4 -- 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ... -- the accumulator rows of one matrix-core product read as the k-steps of
    the next; entries >= L left out (they multiply zeros)."""
    order = [32 * t + (e & 3) + 8 * (e >> 2) + 4 * h for t in range((L + 31) // 32) for e in range(16) for h in (0, 1)]
    return np.array([j for j in order if j < L], np.int64)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64; the sum is rounded to float64 and then to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


# ---- the solvers ---------------------------------------------------------------------------------------------------------------- #
def _sums(x, valid, dtype):
    """(xv, ss): the valid rows' values (0 elsewhere) and ss = the even bands' chain + the odd bands'."""
    xv = np.where(valid[:, None], x, 0).astype(dtype)
    half = [np.zeros(x.shape[0], dtype), np.zeros(x.shape[0], dtype)]
    for b in range(x.shape[1]):
        half[b & 1] = _fma32(xv[:, b], xv[:, b], half[b & 1]) if dtype == np.float32 else half[b & 1] + xv[:, b] * xv[:, b]
    return xv, half[0] + half[1]


def _residual(P, xv, ss, z, dtype):
    if dtype == np.float64:
        b = xv @ P["A"].T
        return np.maximum(0.0, ss - 2.0 * (b * z).sum(1) + (z * (z @ P["G"])).sum(1))
    R, L = z.shape
    A32, order = P["A"].astype(np.float32), chain_order(L)
    b = np.zeros((R, L), np.float32)
    for k in range(xv.shape[1]):
        b = _fma32(xv[:, k:k + 1], A32[None, :, k], b)
    Gz = np.zeros((R, L), np.float32)
    for j in order:
        Gz = _fma32(P["G32"][None, :, j], z[:, j:j + 1], Gz)
    ba, zgz = [np.zeros(R, np.float32), np.zeros(R, np.float32)], [np.zeros(R, np.float32), np.zeros(R, np.float32)]
    for k in range(L):  # each half of a row's entries (k & 4) ascending, then the two halves added
        h = (k >> 2) & 1
        ba[h] = _fma32(b[:, k], z[:, k], ba[h])
        zgz[h] = _fma32(z[:, k], Gz[:, k], zgz[h])
    return np.maximum(np.float32(0), _fma32(np.float32(-2) * np.ones(R, np.float32), ba[0] + ba[1], ss) + (zgz[0] + zgz[1]))


def _admm(A, x, lam, mu, eps, max_iterations, dtype, fault: Optional[str] = None):
    """The iteration of the module docstring in ``dtype`` -> (z [R,L], residual [R], status [R]).  Planted faults: ``no_threshold`` =
    tau left out of z'; ``no_freeze`` = a done row keeps iterating while any row of the batch does; ``minus_zero`` = an inactive entry
    written as -0."""
    f = dtype
    A, x = np.asarray(A, np.float32), np.asarray(x, np.float32)
    R, L = x.shape[0], A.shape[0]
    P = prepare(A, lam, mu)
    valid = row_valid(x)
    xv, ss = _sums(x, valid, f)
    z, d = np.zeros((R, L), f), np.zeros((R, L), f)
    status = np.where(valid, -2, -1).astype(np.int32)
    if f == np.float32:
        Q, M, theta, order = P["Q32"], P["M32"], P["theta32"], chain_order(L)
        c = np.zeros((R, L), f)
        for b in range(x.shape[1]):
            c = _fma32(xv[:, b:b + 1], Q[None, :, b], c)
    else:
        Q, M, theta = P["Q"], P["M"], P["theta"]
        c = xv @ Q.T
    with np.errstate(all="ignore"):
        tau = (f(theta) * np.sqrt(ss.astype(f))).astype(f)
        es = (f(eps) * np.abs(c).max(1, initial=0)).astype(f)
        live = valid.copy()
        for it in range(1, max_iterations + 1):
            rows = np.nonzero(valid if fault == "no_freeze" else live)[0]
            if not live.any():
                break
            v = z[rows] - d[rows]
            if f == np.float32:
                a = c[rows].copy()
                for j in order:
                    a = _fma32(M[None, :, j], v[:, j:j + 1], a)
            else:
                a = c[rows] + v @ M.T
            t = a + d[rows]
            uu = t if fault == "no_threshold" else t - tau[rows, None]
            zn = np.where(uu > 0, uu, f(0)).astype(f)
            dn = t - zn
            conv = (np.abs(a - zn).max(1) <= es[rows]) & (np.abs(zn - z[rows]).max(1) <= es[rows])
            z[rows], d[rows] = zn, dn
            fresh = live[rows] & conv
            status[rows[fresh]] = it
            live[rows[fresh]] = False
    z = np.where(valid[:, None] & (z > 0) & np.isfinite(z), z, f(0)).astype(f)
    res = np.where(valid, _residual(P, xv, ss, z, f), 0).astype(f)
    if fault == "minus_zero":
        z = np.where(z > 0, z, -f(0)).astype(f)
    return z, res, status


def solve_f32(A, x, lam=LAMBDA, mu=None, eps=EPSILON, max_iterations=MAX_ITERATIONS, fault: Optional[str] = None):
    """The kernel's iteration restated in numpy float32, chains in the header's order."""
    return _admm(A, x, lam, auto_mu(A) if mu is None else mu, eps, max_iterations, np.float32, fault)


def solve_admm_f64(A, x, lam=LAMBDA, mu=None, eps=EPSILON, max_iterations=MAX_ITERATIONS):
    """The same iteration in float64 (operands not rounded)."""
    return _admm(A, x, lam, auto_mu(A) if mu is None else mu, eps, max_iterations, np.float64)


def _lambda_r(x64: np.ndarray, lam: float) -> np.ndarray:
    return lam * np.sqrt((x64 * x64).sum(1))


def solve_f64(A, x, lam=LAMBDA):
    """The truth: (abundances [R,L] float64, residual [R], status [R]) from the float32 A and x -- NNLS of (G, b - lambda_r 1).  For a
    library of full row rank (L <= B): the sweep tableau has no pivot to offer on a singular G, and ``kkt_violation`` says so."""
    A, x = np.asarray(A, np.float32), np.asarray(x, np.float32)
    R, L = x.shape[0], A.shape[0]
    valid = row_valid(x)
    A64 = A.astype(np.float64)
    G = A64 @ A64.T
    a, res, status = np.zeros((R, L)), np.zeros(R), np.full(R, -1, np.int32)
    for r in np.nonzero(valid)[0]:
        x64 = x[r].astype(np.float64)
        b = A64 @ x64 - _lambda_r(x64[None], lam)[0]
        if b.max() <= 0:  # the zero vector is optimal
            status[r] = 0
            res[r] = x64 @ x64
            continue
        a[r], status[r] = UF.active_set(G, b, UF.NNLS, np.float64, UF.TOL_F64)
        a[r] = np.where(a[r] > 0, a[r], 0)
        dlt = x64 - a[r] @ A64
        res[r] = dlt @ dlt
    return a, res, status


def brute_force(G: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The exact optimum of 1/2 a.G a - b.a over a >= 0 by enumeration of every support (L <= 6)."""
    return UF.brute_force(G, b, UF.NNLS)


def kkt_violation(A, x, a, lam=LAMBDA) -> np.ndarray:
    """Per row, relative to |b|_inf: the largest of max_k w_k (k anywhere) and max |w_k| on a's support, w = b - lambda_r - G a."""
    A64, x64, a = np.asarray(A, np.float32).astype(np.float64), np.asarray(x).astype(np.float64), np.asarray(a, np.float64)
    b = x64 @ A64.T
    w = b - _lambda_r(x64, lam)[:, None] - a @ (A64 @ A64.T)
    worst = np.maximum(w.max(1), np.where(a > 0, np.abs(w), 0).max(1))
    return np.maximum(worst, 0) / np.abs(b).max(1)


# ---- cases ---------------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def make_case(kind: str, L: int, B: int, R: int, layout: str = "rows") -> Dict:
    A = library(kind, L, B)
    rows = make_rows(A, R)
    if layout == "slice":
        wide = np.full((R, B + SLICE_PAD), np.nan, np.float32)  # (columns outside the slice must never be read)
        wide[:, SLICE_AT:SLICE_AT + B] = rows
        x = wide[:, SLICE_AT:SLICE_AT + B]
    else:
        wide, x = rows, rows
    A64 = A.astype(np.float64)
    return dict(kind=kind, L=L, B=B, R=R, layout=layout, A=A, x=x, wide=wide, valid=row_valid(x), mu=auto_mu(A), lam=LAMBDA,
                eps=EPSILON, max_iterations=MAX_ITERATIONS, smax=float(np.linalg.norm(A64, 2)))


def truth(case: Dict) -> Dict:
    """The float64 optimum of a case (at the case's own lambda) with ``support_cond`` [R] = cond_2(G_SS) of its support."""
    a, res, status = solve_f64(case["A"], case["x"], case["lam"])
    A64 = case["A"].astype(np.float64)
    cond = np.ones(case["R"])
    for r in np.nonzero(case["valid"])[0]:
        S = np.nonzero(a[r] > 0)[0]
        if S.size:
            cond[r] = np.linalg.cond(A64[S]) ** 2
    return dict(a=a, residual=res, status=status, support_cond=cond)


@functools.lru_cache(maxsize=None)
def reference(kind: str, L: int, B: int, R: int, layout: str = "rows") -> Tuple[Dict, Dict]:
    """(case, truth), computed once per case and shared; neither is to be changed."""
    case = make_case(kind, L, B, R, layout)
    return case, truth(case)


def objective(case: Dict, x64: np.ndarray, a: np.ndarray) -> np.ndarray:
    d = x64 - a @ case["A"].astype(np.float64)
    return 0.5 * (d * d).sum(1) + _lambda_r(x64, case["lam"]) * a.sum(1)


def check(case: Dict, abundances, residual, status, report: Optional[Dict] = None, ref: Optional[Dict] = None) -> List[str]:
    """Every rule of the module docstring; ``report`` gets the worst ratios {"objective", "abundance", "residual"} OF THEIR BOUNDS
    (below 1 passes) and "cap_share".  ``residual`` / ``status`` may be None (not checked)."""
    L, R = case["L"], case["R"]
    if ref is None:
        ref = reference(case["kind"], L, case["B"], R, case["layout"])[1]
    a = np.asarray(abundances)
    if a.shape != (R, L) or a.dtype not in (np.float32, np.float64):
        return [f"abundances are {a.dtype} {a.shape}, want float32 {(R, L)}"]
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
        if ((sv < 1) & (sv != -2)).any() or (sv > case["max_iterations"]).any():
            fails.append(f"status outside 1..{case['max_iterations']} / -2 on a valid row")
        share = float((sv == -2).mean()) if sv.size else 0.0
        if report is not None:
            report["cap_share"] = share
        if share > MAX_CAP_SHARE:
            fails.append(f"{share:.3%} of the valid rows stopped at the cap (at most {MAX_CAP_SHARE:.0%})")
    if report is not None:
        report.update(objective=0.0, abundance=0.0, residual=0.0)
    if not v.any():
        return fails
    x64 = case["x"][v].astype(np.float64)
    av, star = a[v].astype(np.float64), ref["a"][v]
    if not np.isfinite(av).all() or (av < 0).any() or np.signbit(a[v]).any():
        fails.append("an abundance is negative, not finite or a negative zero")
        return fails
    ss = (x64 * x64).sum(1)
    e = case["eps"] + L * U
    r_obj = float(((objective(case, x64, av) - objective(case, x64, star)) / (K_F * e * 0.5 * ss)).max())
    cond = ref["support_cond"][v]
    well = cond <= MAX_SUPPORT_COND
    r_ab = float((np.abs(av - star).max(1) / (K_A * e * cond * np.sqrt(ss) / case["smax"]))[well].max()) if well.any() else 0.0
    worst = dict(objective=max(r_obj, 0.0), abundance=r_ab)
    if residual is not None:
        d = x64 - av @ case["A"].astype(np.float64)
        worst["residual"] = float((np.abs(np.asarray(residual)[v].astype(np.float64) - (d * d).sum(1)) / (K_R * U * ss)).max())
        if (np.asarray(residual)[v] < 0).any():
            fails.append("a residual is negative")
    if report is not None:
        report.update(worst)
    for name, ratio in worst.items():
        if not ratio <= 1.0:
            fails.append(f"{name}: {ratio:.3g} x its bound")
    return fails


def rows_are_independent(solve, case: Dict, rows=(0, 1, 5)) -> List[str]:
    """The bits of row r depend neither on R nor on the other rows: ``solve(A, x) -> (a, residual, status)`` on the batch against each
    of ``rows`` alone."""
    a, res, status = solve(case["A"], case["x"])
    fails = []
    for r in rows:
        if r >= case["R"]:
            continue
        a1, res1, status1 = solve(case["A"], case["x"][r:r + 1])
        if a1[0].tobytes() != a[r].tobytes() or res1[0].tobytes() != res[r].tobytes() or status1[0] != status[r]:
            fails.append(f"row {r} alone differs from row {r} in the batch (status {int(status1[0])} against {int(status[r])})")
    return fails


def mu_table(cases=None) -> Dict[float, float]:
    """rho -> the mean iterations of ``solve_admm_f64`` over the valid rows of the cases (a capped row counts max_iterations)."""
    out = {}
    for rho in RHOS:
        counts = []
        for c in (CASES if cases is None else cases):
            case = make_case(*c)
            if not case["valid"].any():
                continue
            _, _, st = solve_admm_f64(case["A"], case["x"], case["lam"], auto_mu(case["A"], rho), case["eps"], case["max_iterations"])
            st = st[case["valid"]]
            counts.append(np.where(st == -2, case["max_iterations"], st))
        out[rho] = float(np.concatenate(counts).mean())
    return out
