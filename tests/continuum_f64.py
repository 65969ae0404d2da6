"""Continuum-removal cases, their float64 oracle, a brute-force check of that oracle, a float32 replay of the kernel's arithmetic and the
comparator with its DERIVED bounds (plain helper module, no tests in it).  It mirrors tests/unmix_f64.py for csrc/umhs_continuum.hip.

Used by tests/test_hip_continuum.py (the kernel and the model on the GPU) and tests/test_continuum_cpu.py (the oracle against the brute
force, the package's host function against the oracle, the float32 replay against every bound).

Statement (include/umhs_hip.h, "Continuum removal"), on float32 rows x [R,B] and float32 wavelengths l [B], strictly increasing:
  hull(lo, hi)   monotone chain left to right; before b is pushed the last vertex p1 is popped while, with p0 the vertex under it,
                   cross = (l1 - l0) * (x_b - x0) - (x1 - x0) * (l_b - l0)      is not < 0.
  c_b            = x_i + ((l_b - l_i) / (l_j - l_i)) * (x_j - x_i) between consecutive vertices i < b < j;  c_b = x_b at a vertex.
  r_b            = x_b / c_b where c_b > 0, else 1.
  feature        on the hull of its OWN range:  depth = 1 - min r;  centre = l_m, m the first band at the minimum;
                 area: from 0, for b = lo + 1 .. hi:  area += (0.5 * (l_b - l_{b-1})) * ((1 - r_{b-1}) + (1 - r_b)).
  invalid row    a NaN or an Inf anywhere in it: removed 0, features 0, status -1; else status = vertices of the full-range hull.
``run(..., np.float64)`` is the oracle (the truth: the same float32 inputs, every operation in float64); ``run(..., np.float32)`` is the
replay: numpy rounds every float32 operation once and contracts nothing, which is what the kernel does too -- plain operators under
``#pragma clang fp contract(off)``, so no product and sum are fused -- in the same order.  ``brute_continuum`` is c_b = max over
i <= b <= j of the chord (i, j) at l_b, O(B^3), to check the oracle at B <= 33.

BOUNDS.  u = 2^-24; a range of n bands; M = max |x| over it; L = l_hi - l_lo; d = its smallest spacing.  Every constant is a count of
float32 roundings in the order above, to first order in u, rounded up to absorb the second order (n^2 u < 0.4 % at n = 256).
  interpolation  t = (l_b - l_i) / (l_j - l_i) carries 3 roundings (two differences, one quotient), t <= 1; x_j - x_i one, |.| <= 2 M;
                 the product one more: 5 u |t (x_j - x_i)| <= 10 u M; the sum one on |c| <= M.  Through the SAME vertices
                 |c^ - c| <= 11 u M, taken as K_I = 12.
  orientation    each product of the cross carries 3 roundings (two differences, the product), the difference one on a result no larger
                 than |A| + |B|: |cross^ - cross| <= 4 u (|A| + |B|) <= 4 u (2 M (l_b - l_0) + 2 M (l_b - l_0)) = 16 u M (l_b - l_0).
                 p1 stands h = -cross / (l_b - l_0) above the chord p0 -> b, so a test can go the other way than float64's only when
                 |h| <= K_T u M, K_T = 16.
  vertex sets    are NOT assumed equal.  Let g be the exact interpolant through the vertices float32 kept.
                 above   a chain through data points lies on or below their least concave majorant c*:  g <= c*.
                 below   (a) when band i is pushed g(l_i) = x_i; afterwards only pops change g there, a pop lowers g by no more than
                         the popped vertex stood above its chord, <= K_T u M when it stood above at all, and each band is popped at
                         most once: x_i <= g(l_i) + (n - 2) K_T u M for every band.
                         (b) consecutive kept vertices p0, p1, p2 passed the test when p2 was pushed, so p1 is below the chord p0 -> p2
                         by d_k <= 4 u (|x2 - x0| + |x1 - x0|) at most; over the chain these sum to <= 12 u TV(g), and a chain that is
                         concave up to such defects inside [-M, M] has TV <= 4 M: sum d_k <= 48 u M.  Removing a convex kink of defect
                         d_k (slope change d_k (1/a + 1/b) <= 2 d_k / d) raises the chain by at most that times L / 4 anywhere, so its
                         concave majorant g~ has g~ - g <= 48 u M L / (2 d) = 24 u M L / d.
                         (c) g~ + (n - 2) K_T u M is concave and above every point, hence above c*.
                 |c^ - c*| <= E_c = u M (K_I + K_T (n - 2) + K_D L / d),  K_D = 24;  E_c = 0 at lo and hi (always vertices: c = x) and
                 for n <= 2.  (For uniform wavelengths L / d = n - 1: about 10^4 u M at n = 256.  The linear growth is real: a sloped,
                 faintly convex row keeps every band and sits 2 u n M below its chord.)
  r              x / c^ against x / c*:  |x| E_c / (c* (c* - E_c)), plus the quotient's rounding u |x| / (c* - E_c); with |x| <= M:
                 E_r = (M / c*) E_c / (c* - E_c) + u M / (c* - E_c)   where c* > 2 E_c;  0 where E_c = 0 and c* <= 0 (r = 1 both
                 sides);  unbounded elsewhere (a continuum within rounding of 0: r jumps to 1 there).
  depth          the minimum is taken exactly; the kernel's band m can only be one with r*_m - E_r[m] <= min r* + E_r[m*]:
                 E_min = the largest E_r over those bands;  E_depth = E_min + u (1 + |min r*| + E_min) for the one subtraction.
  centre         discrete.  With m the band whose float32 wavelength the kernel returned (it must be one of the range, exactly):
                 r*_m <= min r* + E_r[m] + E_r[m*].  Every valid row is checked.
  area           1 - r one rounding, each term 3 (difference, product, sum; 0.5 x is exact), n - 1 additions:
                 E_area = (1 + (n + 4) u) sum_b W_b E_r[b] + (n + 4) u sum_b W_b |1 - r*_b|,   W_b the trapezoid weights.
  exact rows     small-integer x on small-integer l: every cross product is exact in float32, so status equals the oracle's; where a
                 range holds an interior band of value 0 among non-negative values that are not all 0, r = 0 exactly there on both
                 sides and the centre equals the oracle's exactly.
The float32 replay against these bounds (tests/test_continuum_cpu.py records the worst ratios in its assertion message), ratios OF THE
BOUNDS over CASES: c 0.012 (B = 3), r 0.0095 (B = 3), depth 0.017 and area 0.017 (B = 141 on the golden band list, 8 features), centre
0.011 (B = 256); 10^-4 of E_c at B = 256.  They are worst-case bounds and it shows; the float32 vertex count differs from float64's on
170 rows of the cases.  The kernel on an MI355X
(tests/test_hip_continuum.py) gives the replay's ratios to every printed digit: its arithmetic is the replay's."""
from __future__ import annotations

import functools
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

U = 2.0 ** -24
K_I, K_T, K_D = 12.0, 16.0, 24.0
MAX_BANDS, MAX_FEATURES = 256, 8
SLICE_PAD, SLICE_AT = 5, 3
N_KINDS, N_INT_KINDS = 14, 6

# (B, R, layout, wavelengths, F): ``slice`` = a misaligned column slice of a wider array; wavelengths ``uni``form, ``non``-uniform,
# small ``int``egers (the exact rows) or ``golden``: the scenes' own band lists of tests/golden/g1_colour.npz (b21_bands, b31_bands,
# b128_bands, b141_bands: what the g8 model fixtures carry as ``bands``), cast to float32 as a scene does; F features from ``feature_ranges``
CASES = [(1, 1, "rows", "uni", 0), (1, 65, "rows", "non", 0), (2, 63, "rows", "non", 0), (2, 1, "slice", "uni", 0),
         (3, 64, "rows", "uni", 1), (3, 65, "slice", "non", 8), (4, 65, "rows", "int", 8), (4, 1, "rows", "non", 1),
         (31, 0, "rows", "uni", 8), (31, 300, "rows", "uni", 8), (31, 65, "slice", "non", 1), (31, 64, "rows", "int", 8),
         (33, 63, "rows", "non", 8), (33, 333, "slice", "uni", 0), (141, 65, "rows", "non", 8), (141, 130, "slice", "uni", 1),
         (252, 64, "slice", "uni", 1), (253, 65, "rows", "non", 8), (256, 64, "rows", "uni", 8), (256, 130, "slice", "non", 8),
         (256, 65, "rows", "int", 1),
         (21, 65, "rows", "golden", 8), (31, 130, "slice", "golden", 8), (128, 65, "rows", "golden", 8), (128, 130, "slice", "golden", 1),
         (141, 65, "rows", "golden", 8), (141, 64, "slice", "golden", 0)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_BANDS = (21, 31, 128, 141)


def case_id(c) -> str:
    return f"B{c[0]}-R{c[1]}-{c[3]}-F{c[4]}" + ("-slice" if c[2] == "slice" else "")


# ---- wavelengths, windows, rows ------------------------------------------------------------------------------------------------- #
def wavelengths(kind: str, B: int) -> np.ndarray:
    """float32 [B], strictly increasing."""
    if kind == "uni":
        lam = np.linspace(400.0, 1000.0, B) if B > 1 else np.array([400.0])
    elif kind == "non":
        g = np.random.default_rng(17 + B)
        lam = 400.0 + np.concatenate([[0.0], np.cumsum(g.uniform(0.5, 3.0, B - 1) * (600.0 / max(B, 2)))])
    elif kind == "golden":
        with np.load(os.path.join(GOLDEN, "g1_colour.npz")) as f:
            lam = np.asarray(f[f"b{B}_bands"], np.float64)
    else:  # small integers: steps of 1, 2 or 3
        g = np.random.default_rng(29 + B)
        lam = np.concatenate([[0.0], np.cumsum(g.integers(1, 4, B - 1))]).astype(np.float64)
    lam = lam.astype(np.float32)
    assert lam.shape == (B,) and (np.diff(lam) > 0).all()
    return lam


def feature_ranges(B: int, F: int) -> List[Tuple[int, int]]:
    """F inclusive band ranges of at least 3 bands: the full range first (its numbers must equal what ``removed`` gives, bit for bit),
    3 bands from band 0, 3 bands up to band B - 1, two long ones that overlap, and three more short ones."""
    if F == 0:
        return []
    assert B >= 3

    def fix(lo, hi):
        lo, hi = max(0, lo), min(B - 1, hi)
        if hi - lo < 2:
            lo = max(0, hi - 2)
            hi = lo + 2
        return lo, hi

    all8 = [(0, B - 1), fix(0, 2), fix(B - 3, B - 1), fix(B // 4, (3 * B) // 4), fix(B // 2 - 1, B // 2 + B // 3), fix(1, 3),
            fix(B - 5, B - 2), fix(B // 3, B // 3 + 2)]
    return all8[:F]


def make_rows(lam: np.ndarray, R: int, integer: bool, seed: int = 1) -> np.ndarray:
    """float32 [R,B]: the row kinds cycled over r, so that neighbouring lanes walk different hulls."""
    B = lam.shape[0]
    g = np.random.default_rng(1000 * seed + 7 * B + R)
    l64 = lam.astype(np.float64)
    t = (l64 - l64[0]) / max(l64[-1] - l64[0], 1.0)
    idx = np.arange(B)
    x = np.zeros((R, B), np.float32)
    for r in range(R):
        if integer:
            kind = r % N_INT_KINDS
            if kind == 0:  # small integers with interior zeros: the minimum of r is 0, exactly, on both sides
                v = g.integers(1, 16, B).astype(np.float64)
                if B >= 3:
                    v[g.integers(1, B - 1, 2)] = 0.0
            elif kind == 1:  # exactly collinear
                v = l64.copy()
            elif kind == 2:
                v = np.full(B, 5.0)
            elif kind == 3:
                v = np.zeros(B)
            elif kind == 4:  # integer saw-tooth
                v = 7.0 * (idx & 1) + (idx == 0) * 3.0
            else:
                v = g.integers(1, 16, B).astype(np.float64)
                v[B // 2] = np.nan
        else:
            kind = r % N_KINDS
            if kind == 0:  # a dome: every band a vertex, the deepest stack
                v = 0.2 + 0.6 * np.sin(np.pi * (0.05 + 0.9 * t))
            elif kind == 1:  # a bowl: only the endpoints are vertices
                v = 0.9 - 0.6 * np.sin(np.pi * (0.05 + 0.9 * t))
            elif kind == 2:  # saw-tooth: most pops
                v = 0.2 + 0.5 * (idx & 1) + 0.1 * t
            elif kind == 3:  # exactly collinear in float32 (a power-of-two multiple of the wavelengths)
                v = l64 * 2.0 ** -11
            elif kind == 4:
                v = np.full(B, 0.37)
            elif kind == 5:
                v = np.zeros(B)
            elif kind == 6:  # monotone up
                v = 0.02 + 0.9 * t ** 1.5
            elif kind == 7:  # monotone down
                v = 0.02 + 0.9 * (1.0 - t) ** 0.7
            elif kind == 8:  # one deep narrow feature
                v = (0.5 + 0.2 * t) * (1.0 - 0.8 * np.exp(-0.5 * ((t - g.uniform(0.2, 0.8)) / 0.03) ** 2))
            elif kind == 9:  # smooth random
                v = 0.6 + sum(0.12 * np.sin(2 * np.pi * (g.uniform(0.5, 4.0) * t + g.uniform())) for _ in range(3))
            elif kind == 10:  # a NaN or an Inf
                v = 0.3 + 0.4 * g.uniform(size=B)
                which = (r // N_KINDS) % 3
                v[(B // 2, B - 1, 0)[which]] = (np.nan, np.inf, -np.inf)[which]
            elif kind == 11:  # collinear up to the rounding of the data: the vertex set is float32's own
                v = (0.3 + 0.5 * t).astype(np.float32).astype(np.float64) + g.integers(-2, 3, B) * U * 0.5
            elif kind == 12:  # rough random: many vertices, many pops
                v = g.uniform(0.05, 1.0, B)
            else:  # a faintly convex slope: where keeping every band costs the most
                v = 0.2 + 0.6 * t + 4.0 * U * B * (t - 0.5) ** 2
        x[r] = v.astype(np.float32)
    return x


def row_valid(x: np.ndarray) -> np.ndarray:
    return np.isfinite(np.asarray(x, np.float32)).all(1)


# ---- the chain, in either precision ---------------------------------------------------------------------------------------------- #
def hull(lam, x, lo: int, hi: int, dtype) -> np.ndarray:
    """bool [R, hi - lo + 1]: the vertices of the upper hull of every row over lo..hi, by the monotone chain of the statement in
    ``dtype``, all rows in step (a row either pops or pushes per trip, as a lane of the kernel does)."""
    f = dtype
    l, x = np.asarray(lam, np.float32).astype(f)[lo:hi + 1], np.asarray(x, np.float32).astype(f)[:, lo:hi + 1]
    R, n = x.shape
    rows = np.arange(R)
    stack = np.zeros((R, n + 1), np.int64)
    top, b = np.ones(R, np.int64), np.ones(R, np.int64)
    with np.errstate(all="ignore"):
        while True:
            active = b < n
            if not active.any():
                break
            bb = np.minimum(b, n - 1)
            i1, i0 = stack[rows, top - 1], stack[rows, np.maximum(top - 2, 0)]
            cross = (l[i1] - l[i0]) * (x[rows, bb] - x[rows, i0]) - (x[rows, i1] - x[rows, i0]) * (l[bb] - l[i0])
            assert cross.dtype == f
            pop = active & (top >= 2) & ~(cross < 0)
            push = active & ~pop
            stack[rows[push], top[push]] = b[push]
            top = top + push - pop
            b = b + push
    vertex = np.zeros((R, n), bool)
    for d in range(n):
        live = top > d
        vertex[rows[live], stack[live, d]] = True
    return vertex


def evaluate(lam, x, lo: int, hi: int, vertex: np.ndarray, dtype):
    """(c [R,n], r [R,n], rmin [R], m [R] (band index), area [R]) of the statement in ``dtype`` from the vertices."""
    f = dtype
    l, x = np.asarray(lam, np.float32).astype(f)[lo:hi + 1], np.asarray(x, np.float32).astype(f)[:, lo:hi + 1]
    R, n = x.shape
    idx = np.broadcast_to(np.arange(n), (R, n))
    i = np.maximum.accumulate(np.where(vertex, idx, 0), axis=1)
    j = np.minimum.accumulate(np.where(vertex, idx, n - 1)[:, ::-1], axis=1)[:, ::-1]
    rows = np.arange(R)[:, None]
    with np.errstate(all="ignore"):
        xi, xj, li, lj = x[rows, i], x[rows, j], l[i], l[j]
        c = np.where(vertex, x, xi + ((l[None, :] - li) / (lj - li)) * (xj - xi)).astype(f)
        r = np.where(c > 0, x / c, f(1)).astype(f)
        q = (f(1) - r).astype(f)
        area = np.zeros(R, f)
        for b in range(1, n):
            area = area + (f(0.5) * (l[b] - l[b - 1])) * (q[:, b - 1] + q[:, b])
        assert c.dtype == f and r.dtype == f and area.dtype == f
    m = np.argmin(r, axis=1) if n else np.zeros(R, np.int64)  # (the first band at the minimum)
    return c, r, r[np.arange(R), m], m + lo, area


def run(lam, x, ranges: Sequence[Tuple[int, int]], dtype) -> Dict:
    """The whole entry point in ``dtype``: removed [R,B], c [R,B], features [R,F,3], status [R], and per feature its (c, r) arrays."""
    lam32, x32 = np.asarray(lam, np.float32), np.asarray(x, np.float32)
    R, B = x32.shape
    valid = row_valid(x32)
    xs = np.where(valid[:, None], x32, np.float32(0))
    out = dict(removed=np.zeros((R, B), dtype), c=np.zeros((R, B), dtype), features=np.zeros((R, len(ranges), 3), dtype),
               status=np.full(R, -1, np.int32), per_feature=[])
    if R == 0:
        return out
    v = hull(lam32, xs, 0, B - 1, dtype)
    c, r, _, _, _ = evaluate(lam32, xs, 0, B - 1, v, dtype)
    out["c"], out["removed"] = np.where(valid[:, None], c, 0), np.where(valid[:, None], r, 0)
    out["status"] = np.where(valid, v.sum(1), -1).astype(np.int32)
    for k, (lo, hi) in enumerate(ranges):
        v = hull(lam32, xs, lo, hi, dtype)
        c, r, rmin, m, area = evaluate(lam32, xs, lo, hi, v, dtype)
        feat = np.stack([dtype(1) - rmin, lam32.astype(dtype)[m], area], 1)
        out["features"][:, k] = np.where(valid[:, None], feat, 0)
        out["per_feature"].append(dict(c=c, r=r, m=m, vertices=v.sum(1)))
    return out


def brute_continuum(lam, x) -> np.ndarray:
    """c_b = max over i <= b <= j of the chord (i, j) at l_b, float64, one row [B] at a time: O(B^3), for B <= 33."""
    l, x = np.asarray(lam, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    B = l.shape[0]
    c = x.copy()
    for b in range(B):
        for i in range(b):
            for j in range(b + 1, B):
                c[b] = max(c[b], x[i] + (x[j] - x[i]) * (l[b] - l[i]) / (l[j] - l[i]))
    return c


# ---- cases ---------------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def make_case(B: int, R: int, layout: str, lam_kind: str, F: int) -> Dict:
    lam = wavelengths(lam_kind, B)
    rows = make_rows(lam, R, lam_kind == "int")
    if layout == "slice":
        wide = np.full((R, B + SLICE_PAD), np.nan, np.float32)  # (columns outside the slice must never be read)
        wide[:, SLICE_AT:SLICE_AT + B] = rows
        x = wide[:, SLICE_AT:SLICE_AT + B]
    else:
        wide, x = rows, rows
    return dict(B=B, R=R, layout=layout, lam_kind=lam_kind, F=F, lam=lam, x=x, wide=wide, ranges=feature_ranges(B, F), valid=row_valid(x),
                exact=lam_kind == "int")


@functools.lru_cache(maxsize=None)
def reference(B: int, R: int, layout: str, lam_kind: str, F: int) -> Tuple[Dict, Dict]:
    """(case, float64 run), computed once per case and shared; neither is to be changed."""
    case = make_case(B, R, layout, lam_kind, F)
    return case, run(case["lam"], case["x"], case["ranges"], np.float64)


# ---- bounds and comparator ------------------------------------------------------------------------------------------------------ #
def bounds(lam, x, lo: int, hi: int, c_star: np.ndarray, r_star: np.ndarray) -> Dict:
    """E_c [R,n], E_r [R,n], E_depth [R], E_area [R] of the module docstring for the valid rows ``x`` over lo..hi."""
    l = np.asarray(lam, np.float32).astype(np.float64)[lo:hi + 1]
    xr = np.abs(np.asarray(x, np.float32).astype(np.float64)[:, lo:hi + 1])
    R, n = xr.shape
    M = xr.max(1) if n else np.zeros(R)
    if n >= 3:
        Ec = U * M * (K_I + K_T * (n - 2) + K_D * (l[-1] - l[0]) / np.diff(l).min())
    else:
        Ec = np.zeros(R)
    Ec = np.repeat(Ec[:, None], n, 1)
    Ec[:, 0] = Ec[:, -1] = 0.0
    with np.errstate(all="ignore"):
        Er = np.where(c_star > 2 * Ec, (M[:, None] / c_star) * Ec / (c_star - Ec) + U * M[:, None] / (c_star - Ec), np.inf)
    Er = np.where((Ec == 0) & (c_star <= 0), 0.0, Er)
    rows = np.arange(R)
    ms = np.argmin(r_star, 1)
    rmin = r_star[rows, ms]
    with np.errstate(invalid="ignore"):
        cand = (r_star - Er) <= (rmin + Er[rows, ms])[:, None]
    Emin = np.where(cand, Er, 0.0).max(1)
    Edepth = Emin + U * (1.0 + np.abs(rmin) + Emin)
    W = np.zeros(n)
    if n > 1:
        W[:-1] += 0.5 * np.diff(l)
        W[1:] += 0.5 * np.diff(l)
    Earea = (1.0 + (n + 4) * U) * (Er * W).sum(1) + (n + 4) * U * (np.abs(1.0 - r_star) * W).sum(1)
    return dict(Ec=Ec, Er=Er, Edepth=Edepth, Earea=Earea, mstar=ms, rmin=rmin)


def _ratio(err: np.ndarray, bound: np.ndarray) -> float:
    """The worst err / bound; a zero bound demands a zero error; an unbounded entry (inf) counts 0 unless the error is not finite."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isfinite(err), q, np.inf)
    return float(q.max())


def check(case: Dict, removed, features, status, report: Optional[Dict] = None, ref: Optional[Dict] = None, c=None) -> List[str]:
    """Every rule of the module docstring; ``report`` gets the worst ratios {"c", "r", "depth", "centre", "area"} OF THEIR BOUNDS (below 1
    passes).  Any of ``removed`` / ``features`` / ``status`` / ``c`` (the replay's continuum) may be None (not checked)."""
    B, R, F = case["B"], case["R"], len(case["ranges"])
    if ref is None:
        ref = reference(B, R, case["layout"], case["lam_kind"], case["F"])[1]
    fails: List[str] = []
    v, dead = case["valid"], ~case["valid"]
    worst = dict(c=0.0, r=0.0, depth=0.0, centre=0.0, area=0.0)
    lam, x = case["lam"], np.ascontiguousarray(case["x"])
    if removed is not None:
        removed = np.asarray(removed)
        if removed.shape != (R, B):
            return [f"removed is {removed.shape}, want {(R, B)}"]
        if (removed[dead] != 0).any():
            fails.append("an invalid row's removed is not 0")
    if status is not None:
        status = np.asarray(status)
        if status.shape != (R,):
            return [f"status is {status.shape}, want {(R,)}"]
        if (status[dead] != -1).any():
            fails.append("an invalid row's status is not -1")
        if ((status[v] < min(B, 2)) | (status[v] > B)).any():
            fails.append(f"status outside {min(B, 2)}..{B} on a valid row")
        if case["exact"] and (status[v] != ref["status"][v]).any():
            fails.append("exact rows: status differs from the oracle's vertex count")
    if features is not None:
        features = np.asarray(features)
        if features.shape != (R, F, 3):
            return [f"features are {features.shape}, want {(R, F, 3)}"]
        if (features[dead] != 0).any():
            fails.append("an invalid row's features are not 0")
    if v.any() and R:
        xv = x[v]
        if removed is not None or c is not None:
            bd = bounds(lam, xv, 0, B - 1, ref["c"][v], ref["removed"][v])
            if c is not None:
                worst["c"] = max(worst["c"], _ratio(np.abs(np.asarray(c, np.float64)[v] - ref["c"][v]), bd["Ec"]))
            if removed is not None:
                worst["r"] = max(worst["r"], _ratio(np.abs(removed[v].astype(np.float64) - ref["removed"][v]), bd["Er"]))
        if features is not None:
            l64 = lam.astype(np.float64)
            for k, (lo, hi) in enumerate(case["ranges"]):
                pf = ref["per_feature"][k]
                cs, rs = pf["c"][v], pf["r"][v]
                bd = bounds(lam, xv, lo, hi, cs, rs)
                fk = features[v, k].astype(np.float64)
                worst["depth"] = max(worst["depth"], _ratio(np.abs(fk[:, 0] - ref["features"][v, k, 0]), bd["Edepth"]))
                worst["area"] = max(worst["area"], _ratio(np.abs(fk[:, 2] - ref["features"][v, k, 2]), bd["Earea"]))
                hit = fk[:, 1][:, None] == l64[None, lo:hi + 1]
                if not hit.any(1).all():
                    fails.append(f"feature {k}: a centre is not a wavelength of its range")
                    continue
                mk = hit.argmax(1)
                rows = np.arange(len(mk))
                slack = bd["Er"][rows, mk] + bd["Er"][rows, bd["mstar"]]
                worst["centre"] = max(worst["centre"], _ratio(np.maximum(rs[rows, mk] - bd["rmin"], 0.0), slack))
                if case["exact"]:
                    xw = xv[:, lo:hi + 1]
                    sure = (xw[:, 1:-1] == 0).any(1) & (xw >= 0).all(1) & (xw > 0).any(1)
                    if (mk[sure] + lo != pf["m"][v][sure]).any():
                        fails.append(f"feature {k}: exact rows: a centre differs from the oracle's")
    if report is not None:
        report.update(worst)
    for name, ratio in worst.items():
        if not ratio < 1.0:
            fails.append(f"{name}: {ratio:.3g} x its bound")
    return fails


def area_from_removed(lam, removed, lo: int, hi: int) -> np.ndarray:
    """The statement's trapezoid sum in float32 from float32 r: what a feature over the same range must give, bit for bit."""
    l, r = np.asarray(lam, np.float32), np.asarray(removed, np.float32)
    one, half = np.float32(1), np.float32(0.5)
    area = np.zeros(r.shape[0], np.float32)
    q = (one - r).astype(np.float32)
    for b in range(lo + 1, hi + 1):
        area = area + (half * (l[b] - l[b - 1])) * (q[:, b - 1] + q[:, b])
    assert area.dtype == np.float32
    return area
