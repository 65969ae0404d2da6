"""Image-metric cases, their float64 truth, float32 restatement and the comparators (plain helper module, no tests in it), for
csrc/umhs_metrics.hip.  It mirrors tests/library_f64.py.

Used by tests/test_hip_metrics_f64.py (the two kernels and the model on the GPU) and tests/test_metrics_bounds_cpu.py (the comparators
pass the float32 restatement and reject planted faults; every K and every condition is measured there).

Statement (include/umhs_hip.h, "SURVEY 8(f)-4", and torchmetrics' structural_similarity_index_measure), on float32 channel-last images:
  pixel metrics  per pixel p: sse = sum_k (a_k - b_k)^2, cos = <a,b> / (|a||b|), angle = acos(clamp(cos, -1, 1)); a pixel is LIVE when
                 both spectra are finite and neither is all zero, and only live pixels have an angle.  partial[b] = {sum sse, sum angle,
                 number of live pixels} over the pixels with (p / 256) % n_partial == b; a block without pixels writes zeros.
  SSIM           per channel c and window (oy, ox), 0 <= oy <= H - 11, 0 <= ox <= W - 11, with the 11 x 11 weights g_y g_x
                 (g_i ~ exp(-((i - 5) / 1.5)^2 / 2), sum 1): s0..s4 = the weighted sums of p, q, p^2, q^2, pq;
                 N1 = 2 s0 s1 + c1, N2 = 2 (s4 - s0 s1) + c2, D1 = s0^2 + s1^2 + c1, D2 = max(s2 - s0^2, 0) + max(s3 - s1^2, 0) + c2,
                 c1 = (.01 L)^2, c2 = (.03 L)^2, v = N1 N2 / (D1 D2).  Slot (c GY + by) GX + bx holds the sum of v over
                 8 by <= oy < 8 by + 8, 32 bx <= ox < 32 bx + 32; GX = ceil((W - 10) / 32), GY = ceil((H - 10) / 8).
The float64 run (the truth) takes the SAME float32 inputs (L included) and sums each window directly over its 121 taps.

ONE RULE per SSIM slot:   |got - sum v64| <= K_SSIM u sum (mag + tiny)   over the slot's windows, u = 2^-24, tiny = 2^-126, with
  M0..M4 = the same weighted sums of |p|, |q|, p^2, q^2, |pq|
  eN1 = 4 M0 M1 + |N1|    eN2 = 2 (M4 + 2 M0 M1) + |N2|    eD1 = 2 M0^2 + 2 M1^2 + |D1|    eD2 = (M2 + 2 M0^2) + (M3 + 2 M1^2) + |D2|
  mag = (|N2| eN1 + |N1| eN2) / (D1 D2) + |v| (eD1 / D1 + eD2 / D2) + |v|.
Exact properties beside it.  (a) A window in which both images are all zero is exactly 1.0 in float32 ((c1 c2) / (c1 c2)): the impulse
cases take such windows out of the bound, so a slot made of them equals its window count.  (b) THE CLAMP'S CEILING, on the case
"const-zero" (a constant, b = 0): there s1 = s3 = s4 = 0 exactly, so N2 = c2 exactly and D2 = max(s2 - s0^2, 0) + c2 >= c2: whatever
the rounding of s2 - s0^2 does, the clamp keeps v <= N1 / D1, and got <= sum v64 + K_SSIM u sum (mag1 + tiny) with
mag1 = |N2| eN1 / (D1 D2) + |v| eD1 / D1 + |v| (the eN2 and eD2 terms are gone).  Without the clamp a negative rounded variance lifts v
by |s2 - s0^2| / c2 ~ 1e-4, far above that; the symmetric rule cannot see it (the clamp only ever acts on rounding noise the rule admits).
ONE RULE per angle sum:   mag_c = sum_k |a_k b_k| / (|a||b|) + 2 |cos64|, delta = K_SAM u (mag_c + tiny); a block's angle sum lies in
  the sum over its live pixels of [acos(min(1, cos64 + delta)) - K_SAM u pi, acos(max(-1, cos64 - delta)) + K_SAM u pi].
SSE:   |got - sum sse64| <= K_SSE u sum sse64 per block (the same NaN / Inf where the float64 sum is not finite).   cnt: exact.

K = max(8, 4 x the float32 restatement's worst ratio over the cases, rounded up to a power of two).  Measured on the CPU
(tests/test_metrics_bounds_cpu.py re-measures and asserts 4 x worst <= K == k_for(worst)):
  K_SSIM = 8     worst 1.78, PER WINDOW (H27-W75-K1-impulse2, a window whose only non-zero taps are two corner taps; 1.48 on "negcov",
                 1.34 on H27-W75-K5-flat, 1.29 on "constant", 0.80 on noise); per slot the worst is 0.66 (H27-W75-K5-flat).  4 x 1.78 = 7.1.
  K_SAM  = 8     the angle rule is an interval, so its ratio is the smallest power of two k at which the intervals built with k hold
                 every slot's sum: 2 (n1-K31 and the sparse layout at K = 31; 1 at K = 3, <= 0.5 on the dense cases).  4 x 2 = 8.
  K_SSE  = 8     worst 1.35 (sparse layout, K = 3; 0.69 on n262401-K1)
  clamp's ceiling: the restatement is never above float64 on "const-zero" (worst excess -0.7 of the bound); unclamped it is 333 x over.
Conditions on the cases, asserted on the float64 run alone:
  linearisation   K u eD1 <= D1 / 16 and K u eD2 <= D2 / 16 in every window.  Measured worst: K u eD2 / D2 = 0.0027 ("edge"; 0.0016 on
                  "flat" and "constant"), K u eD1 / D1 = 4.0e-4 ("signed"); 1/16 = 0.0625.
  magnitudes      the non-zero values of live pixels have magnitude in [1e-3, 1e3].  Measured: [1.0e-3, 2.21] over the pixel cases.
  teeth           at least 90 % of a case's windows (of an impulse case: of its touched windows) have |v64 - 1| > 16 x their bound.
                  Measured: 1.0 on every case that counts.  "flat" (0.0) and "constant" (0.28) are near 1 by construction and cannot
                  meet it at any shape (NO_TEETH): they are there for K, as the worst conditioning the rule has to follow, and a
                  kernel that returned 1 would pass them, which is why no planted fault names them."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from rays_f64 import TEETH, TINY, U  # noqa: F401  (one u, one tiny, one teeth factor)

K_SSIM = 8.0
K_SAM = 8.0
K_SSE = 8.0
MIN_TEETH = 0.9
WIN, TX, TY, BLOCK = 11, 32, 8, 256
MAX_BLOCKS = 1024  # ops.pixel_metrics caps its grid here

SSIM_SHAPES = [(11, 11, 1), (18, 42, 3), (19, 43, 2), (27, 75, 5), (12, 140, 141)]
SSIM_KINDS = ["noise", "flat", "constant", "negcov", "signed", "edge", "x100"]
# (shape, kind): every kind on the four-block shape, every shape on noise, and the clamp's-ceiling case
SSIM_CASES = [(s, "noise") for s in SSIM_SHAPES] + [((19, 43, 2), k) for k in SSIM_KINDS[1:]] + [((27, 75, 5), "flat"), ((27, 75, 5), "edge"),
                                                                                               ((19, 43, 2), "const-zero")]
NO_TEETH = ("flat", "constant")  # kinds that are near 1 by construction: there for K, they count as no teeth
IMPULSE_SHAPE = (27, 75, 1)
# (row, col) of the bright pixel in a and in b: tile seams of the 8 x 32 window tiles and of their 10-wide halos
IMPULSES = [((7, 31), (7, 31)), ((8, 32), (8, 32)), ((17, 41), (17, 42)), ((18, 42), (18, 41)), ((7, 41), (8, 42)), ((17, 31), (18, 32)),
            ((0, 0), (26, 74)), ((26, 74), (26, 74))]
PIXEL_CASES = [(n, k) for n in (1, 255, 256, 257) for k in (1, 3, 31, 141)] + [(MAX_BLOCKS * BLOCK + 257, 1), (MAX_BLOCKS * BLOCK + 257, 3)]
SPARSE_BANDS = (3, 31)


def ssim_id(c) -> str:
    (h, w, k), kind = c
    return f"H{h}-W{w}-K{k}-{kind}"


def pixel_id(c) -> str:
    return f"n{c[0]}-K{c[1]}"


def k_for(worst: float) -> float:
    return max(8.0, 2.0 ** math.ceil(math.log2(4.0 * worst))) if worst > 0 else 8.0


# ------------------------------------------------------------------------------------------------------------------------------ #
# SSIM: cases
# ------------------------------------------------------------------------------------------------------------------------------ #
def default_range(a: np.ndarray, b: np.ndarray) -> np.float32:
    """data_range=None as the wrapper forms it: max(a.max - a.min, b.max - b.min), each difference one float32 operation."""
    return np.float32(max(np.float32(a.max()) - np.float32(a.min()), np.float32(b.max()) - np.float32(b.min())))


@functools.lru_cache(maxsize=None)
def make_ssim_case(shape, kind: str) -> Dict:
    """a, b float32 [H,W,K] and data_range (float32; ``explicit`` says whether the caller passes it or leaves the default)."""
    H, W, K = shape
    g = np.random.default_rng(7 * H + 3 * W + K + 1000 * SSIM_KINDS.index(kind) if kind in SSIM_KINDS else 99)
    explicit = None
    if kind == "noise":
        a = g.random((H, W, K))
        b = a + 0.1 * g.standard_normal((H, W, K))
    elif kind == "flat":
        a = 0.7 + 1e-4 * (2 * g.random((H, W, K)) - 1)
        b = 0.7 + 1e-4 * (2 * g.random((H, W, K)) - 1)
        explicit = 1.0
    elif kind == "constant":
        a = np.full((H, W, K), 0.7)
        b = a.copy()
        b[H // 2, W // 2, :] = 0.2
        explicit = 1.0
    elif kind == "negcov":
        a = g.random((H, W, K))
        b = 1.0 - a
    elif kind == "signed":
        a = g.standard_normal((H, W, K))
        b = a + 0.3 * g.standard_normal((H, W, K))
    elif kind == "edge":
        a, b = 0.1 + 0.05 * g.random((H, W, K)), 0.1 + 0.05 * g.random((H, W, K))
        a[:, W // 2:, :] += 0.8
        b[:, W // 2 + 1:, :] += 0.8
    elif kind == "x100":
        a = 100.0 * g.random((H, W, K))
        b = a + 10.0 * g.standard_normal((H, W, K))
    elif kind == "const-zero":
        a, b, explicit = np.full((H, W, K), 0.7), np.zeros((H, W, K)), 1.0
    else:
        raise KeyError(kind)
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    L = np.float32(explicit) if explicit is not None else default_range(a, b)
    return dict(a=a, b=b, L=L, explicit=explicit is not None, kind=kind, shape=shape, exact=None)


@functools.lru_cache(maxsize=None)
def make_impulse_case(i: int) -> Dict:
    """All zero but one bright pixel in a (3.0) and one in b (2.0); default data_range (3.0).  ``exact`` [K,OH,OW]: the windows that
    touch neither, which are exactly 1.0."""
    H, W, K = IMPULSE_SHAPE
    (ya, xa), (yb, xb) = IMPULSES[i]
    a, b = np.zeros((H, W, K), np.float32), np.zeros((H, W, K), np.float32)
    a[ya, xa, 0], b[yb, xb, 0] = 3.0, 2.0
    oy, ox = np.arange(H - WIN + 1)[:, None], np.arange(W - WIN + 1)[None, :]
    touch = lambda y, x: (oy <= y) & (y < oy + WIN) & (ox <= x) & (x < ox + WIN)
    exact = ~(touch(ya, xa) | touch(yb, xb))
    return dict(a=a, b=b, L=default_range(a, b), explicit=False, kind=f"impulse{i}", shape=IMPULSE_SHAPE, exact=exact[None])


# ------------------------------------------------------------------------------------------------------------------------------ #
# SSIM: float64 truth, slots, comparator
# ------------------------------------------------------------------------------------------------------------------------------ #
def weights64() -> np.ndarray:
    d = (np.arange(WIN, dtype=np.float64) - 5.0) / 1.5
    g = np.exp(-(d * d) / 2.0)
    return g / g.sum()


def _window_sums(planes: List[np.ndarray], w2: np.ndarray) -> List[np.ndarray]:
    """Direct 11 x 11 weighted sums of planes [H,W,K] -> [K,OH,OW]."""
    H, W, _ = planes[0].shape
    oh, ow = H - WIN + 1, W - WIN + 1
    out = [np.zeros((oh, ow, p.shape[2]), p.dtype) for p in planes]
    for dy in range(WIN):
        for dx in range(WIN):
            for o, p in zip(out, planes):
                o += w2[dy, dx] * p[dy:dy + oh, dx:dx + ow]
    return [np.moveaxis(o, -1, 0) for o in out]


def ssim64(a: np.ndarray, b: np.ndarray, L) -> Dict:
    """{"v", "mag" (tiny added), "mag1" (the ceiling's), "eD1/D1", "eD2/D2"}, each [K,OH,OW] float64."""
    p, q, L = a.astype(np.float64), b.astype(np.float64), float(L)
    g = weights64()
    w2 = np.outer(g, g)
    s0, s1, s2, s3, s4 = _window_sums([p, q, p * p, q * q, p * q], w2)
    m0, m1, m4 = _window_sums([np.abs(p), np.abs(q), np.abs(p * q)], w2)
    m2, m3 = s2, s3
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    n1, n2 = 2 * s0 * s1 + c1, 2 * (s4 - s0 * s1) + c2
    d1, d2 = s0 * s0 + s1 * s1 + c1, np.maximum(s2 - s0 * s0, 0.0) + np.maximum(s3 - s1 * s1, 0.0) + c2
    v = n1 * n2 / (d1 * d2)
    en1, en2 = 4 * m0 * m1 + np.abs(n1), 2 * (m4 + 2 * m0 * m1) + np.abs(n2)
    ed1, ed2 = 2 * m0 * m0 + 2 * m1 * m1 + np.abs(d1), (m2 + 2 * m0 * m0) + (m3 + 2 * m1 * m1) + np.abs(d2)
    mag = (np.abs(n2) * en1 + np.abs(n1) * en2) / (d1 * d2) + np.abs(v) * (ed1 / d1 + ed2 / d2) + np.abs(v)
    mag1 = np.abs(n2) * en1 / (d1 * d2) + np.abs(v) * ed1 / d1 + np.abs(v)
    return {"v": v, "mag": mag + TINY, "mag1": mag1 + TINY, "eD1/D1": ed1 / d1, "eD2/D2": ed2 / d2}


@functools.lru_cache(maxsize=None)
def ssim_reference(shape, kind) -> Tuple[Dict, Dict]:
    """(case, float64 run), computed once and shared; neither is to be changed.  ``kind`` "impulse<i>": the i-th impulse case."""
    case = make_impulse_case(int(kind[7:])) if kind.startswith("impulse") else make_ssim_case(shape, kind)
    return case, ssim64(case["a"], case["b"], case["L"])


def grid(H: int, W: int) -> Tuple[int, int]:
    """(GY, GX) of the header's slot mapping."""
    return -(-(H - WIN + 1) // TY), -(-(W - WIN + 1) // TX)


def slot_sums(x: np.ndarray) -> np.ndarray:
    """[K,OH,OW] -> [K * GY * GX]: the sum over each slot's windows, in the header's slot order."""
    k, oh, ow = x.shape
    gy, gx = -(-oh // TY), -(-ow // TX)
    pad = np.zeros((k, gy * TY, gx * TX), np.float64)
    pad[:, :oh, :ow] = x
    return pad.reshape(k, gy, TY, gx, TX).sum(axis=(2, 4)).reshape(-1)


def check_ssim(case: Dict, partial, r64: Dict, K: float = K_SSIM, report: Optional[Dict] = None, prefix: str = "") -> List[str]:
    """The slot rule, the exact-1.0 windows where the case has them and the clamp's ceiling on "const-zero";
    report[prefix + "ssim"] = {"worst", "n"} (and prefix + "ceiling")."""
    got = np.asarray(partial, dtype=np.float64).reshape(-1)
    v, mag = r64["v"], r64["mag"]
    ones = np.ones_like(v)
    if case["exact"] is not None:
        ex = np.broadcast_to(case["exact"], v.shape)
        v, mag = np.where(ex, 1.0, v), np.where(ex, 0.0, mag)
    want, bound, count = slot_sums(v), U * slot_sums(mag), slot_sums(ones)
    if got.shape != want.shape:
        return [f"{prefix}{got.size} slots, want {want.size}"]
    fails: List[str] = []
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d == 0, 0.0, d / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max())
    if report is not None:
        report[prefix + "ssim"] = {"worst": worst, "n": int(got.size)}
    if worst > K:
        i = int(ratio.argmax())
        fails.append(f"{prefix}slot {i}: {got[i]:.12g} vs float64 {want[i]:.12g} = {worst:.3g} u sum mag (K = {K:g}; "
                     f"{int((ratio > K).sum())} of {got.size} over)")
    if case["exact"] is not None:
        whole = bound == 0
        if bool((got[whole] != count[whole]).any()):
            fails.append(f"{prefix}{int((got[whole] != count[whole]).sum())} of {int(whole.sum())} slots of all-zero windows are not exactly "
                         f"their window count")
    if case["kind"] == "const-zero":
        over = (got - want) / (U * slot_sums(r64["mag1"]))
        if report is not None:
            report[prefix + "ceiling"] = {"worst": float(over.max()), "n": int(got.size)}
        if float(over.max()) > K:
            fails.append(f"{prefix}slot {int(over.argmax())} is {float(over.max()):.3g} u sum mag1 ABOVE float64: the variance clamp's "
                         f"ceiling does not hold (K = {K:g})")
    return fails


def ssim_conditions(case: Dict, r64: Dict, K: float = K_SSIM) -> Dict:
    """{"eD1", "eD2": worst K u eD / D (<= 1/16), "teeth": share of (not exact) windows with |v - 1| > 16 x bound}."""
    keep = np.ones(r64["v"].shape, bool) if case["exact"] is None else ~np.broadcast_to(case["exact"], r64["v"].shape)
    far = np.abs(r64["v"] - 1.0) > TEETH * K * U * r64["mag"]
    return {"eD1": float(K * U * r64["eD1/D1"].max()), "eD2": float(K * U * r64["eD2/D2"].max()),
            "teeth": float(far[keep].sum()) / max(1, int(keep.sum()))}


# ------------------------------------------------------------------------------------------------------------------------------ #
# SSIM: the float32 restatement in the kernel's operation order (for the K measurement and the planted faults; NOT an oracle)
# ------------------------------------------------------------------------------------------------------------------------------ #
def weights32(sigma: float = 1.5) -> np.ndarray:
    f = np.float32
    g, s = [], f(0)
    for i in range(WIN):
        d = f(i - 5) / f(sigma)
        g.append(np.exp(-(d * d) / f(2)).astype(np.float32))
        s = f(s + g[-1])
    return np.array([f(x / s) for x in g], dtype=np.float32)


def ssim32(a: np.ndarray, b: np.ndarray, L, fault: Optional[str] = None) -> np.ndarray:
    """v float32 [K,OH,OW]: weights by the float32 recurrence, a horizontal pass over the five planes, a vertical pass, nothing
    contracted, both variances clamped at 0.  ``fault``: one of SSIM_FAULTS."""
    f = np.float32
    H, W, K = a.shape
    oh, ow = H - WIN + 1, W - WIN + 1
    if fault == "channel stride 1":  # a[(y W + x) + c] instead of a[(y W + x) K + c]
        idx = (np.arange(H * W).reshape(H, W, 1) + np.arange(K)).reshape(-1)
        a, b = a.reshape(-1)[idx].reshape(H, W, K), b.reshape(-1)[idx].reshape(H, W, K)
    if fault == "data_range from a":
        L = f(f(a.max()) - f(a.min()))
    gk = weights32(1.4 if fault == "sigma 1.4" else 1.5)
    taps = WIN - 1 if fault == "tap 10 dropped" else WIN
    planes = [a, b, a * a, b * b, a * b]
    hz = [np.zeros((H, ow, K), f) for _ in planes]
    seam = (np.arange(ow) % TX == TX - 1)[None, :, None]  # the windows whose tap 10 is the tile's last halo column
    for t in range(taps):
        for h, p in zip(hz, planes):
            term = gk[t] * p[:, t:t + ow]
            if fault == "halo column 10" and t == WIN - 1:
                term = np.where(seam, f(0), term)
            h += term
    s = [np.zeros((oh, ow, K), f) for _ in planes]
    for t in range(taps):
        for o, h in zip(s, hz):
            o += gk[t] * h[t:t + oh]
    L = f(L)
    c1 = (f(0.01) * L) * (f(0.01) * L)
    c2 = (f(0.02 if fault == "k2 = 0.02" else 0.03) * L) * (f(0.02 if fault == "k2 = 0.02" else 0.03) * L)
    mpp, mqq, mpq = s[0] * s[0], s[1] * s[1], s[0] * s[1]
    vp, vq, cov = s[2] - mpp, s[3] - mqq, s[4] - mpq
    if fault != "variance not clamped":
        vp, vq = np.maximum(vp, f(0)), np.maximum(vq, f(0))
    v = ((f(2) * mpq + c1) * (f(2) * cov + c2)) / ((mpp + mqq + c1) * (vp + vq + c2))
    assert v.dtype == np.float32
    if fault == "window validity <":
        v[oh - 1], v[:, ow - 1] = 0, 0
    return np.moveaxis(v, -1, 0)


SSIM_FAULTS = ["halo column 10", "tap 10 dropped", "sigma 1.4", "window validity <", "channel stride 1", "k2 = 0.02", "variance not clamped",
               "data_range from a"]


# ------------------------------------------------------------------------------------------------------------------------------ #
# pixel metrics: cases
# ------------------------------------------------------------------------------------------------------------------------------ #
@functools.lru_cache(maxsize=None)
def make_pixel_case(n: int, K: int) -> Dict:
    """pred, gt float32 [n,K]: gt in [0.05, 0.95], pred = gt + 0.1 randn kept at magnitude >= 1e-3; every 7th pixel of pred negated
    (angles near pi), and from n >= 255 a run of pixels zero in both, one zero in pred only and one zero in gt only."""
    g = np.random.default_rng(100003 * K + n)
    gt = 0.05 + 0.9 * g.random((n, K))
    pred = gt + 0.1 * g.standard_normal((n, K))
    pred = np.where(np.abs(pred) < 1e-3, 1e-3, pred)
    pred[3::7] *= -1.0
    if n >= 255:
        z = n // 3
        pred[z:z + 5], gt[z:z + 5] = 0.0, 0.0
        pred[n - 2], gt[n - 9] = 0.0, 0.0
    return dict(pred=np.ascontiguousarray(pred, dtype=np.float32), gt=np.ascontiguousarray(gt, dtype=np.float32), n=n, K=K)


SPARSE_KINDS = ["parallel", "antiparallel", "orthogonal"] + ["equal bits"] * 48 + ["one ulp", "angle 1e-3", "angle pi - 1e-3", "gt zero",
                                                                                  "pred zero", "NaN band", "Inf band"]


@functools.lru_cache(maxsize=None)
def make_sparse_case(K: int) -> Dict:
    """One live pixel per 256 consecutive ones (pixel 256 i is of SPARSE_KINDS[i]), the other 255 all zero in both images: with one
    block per 256 pixels a slot is that pixel's own {sse, angle, 1}."""
    g = np.random.default_rng(31 + K)
    m = len(SPARSE_KINDS)
    pred, gt = np.zeros((m * BLOCK, K), np.float32), np.zeros((m * BLOCK, K), np.float32)
    for i, kind in enumerate(SPARSE_KINDS):
        p = 0.05 + 0.9 * g.random(K)
        o = g.standard_normal(K)
        o -= p * (o @ p) / (p @ p)
        o *= np.sqrt(p @ p) / np.sqrt(o @ o)
        if kind == "parallel":
            q = 2.5 * p
        elif kind == "antiparallel":
            q = -1.5 * p
        elif kind == "orthogonal":  # disjoint supports: the dot product is exactly 0
            p, q = p.copy(), 0.05 + 0.9 * g.random(K)
            p[1::2], q[0::2] = 0.0, 0.0
        elif kind == "equal bits":
            q = p
        elif kind == "one ulp":
            p = p.astype(np.float32)
            q = p.copy()
            q[K // 2] = np.nextafter(q[K // 2], np.float32(2))
        elif kind == "angle 1e-3":
            q = p * math.cos(1e-3) + o * math.sin(1e-3)
        elif kind == "angle pi - 1e-3":
            q = -(p * math.cos(1e-3) + o * math.sin(1e-3))
        elif kind == "gt zero":
            q = np.zeros(K)
        elif kind == "pred zero":
            p, q = np.zeros(K), p
        elif kind == "NaN band":
            p, q = p.copy(), p + 0.05
            p[K // 2] = np.nan
        elif kind == "Inf band":
            q = p + 0.05
            q[K - 1] = np.inf
        pred[i * BLOCK], gt[i * BLOCK] = p, q
    return dict(pred=pred, gt=gt, n=m * BLOCK, K=K)


# ------------------------------------------------------------------------------------------------------------------------------ #
# pixel metrics: float64 truth, comparator
# ------------------------------------------------------------------------------------------------------------------------------ #
def pixels64(case: Dict, K: float = K_SAM) -> Dict:
    """Per pixel, float64 on the float32 inputs: sse, live, cos, angle, and the angle's interval [lo, hi] (0 where not live)."""
    a, b = case["pred"].astype(np.float64), case["gt"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = a - b
        sse = (e * e).sum(1)
    live = np.isfinite(a).all(1) & np.isfinite(b).all(1) & (a != 0).any(1) & (b != 0).any(1)
    a1, b1 = np.where(live[:, None], a, 1.0), np.where(live[:, None], b, 1.0)
    norm = np.sqrt((a1 * a1).sum(1)) * np.sqrt((b1 * b1).sum(1))
    cos = np.clip((a1 * b1).sum(1) / norm, -1.0, 1.0)
    delta = K * U * (np.abs(a1 * b1).sum(1) / norm + 2 * np.abs(cos) + TINY)
    lo = np.arccos(np.minimum(1.0, cos + delta)) - K * U * math.pi
    hi = np.arccos(np.maximum(-1.0, cos - delta)) + K * U * math.pi
    z = lambda x: np.where(live, x, 0.0)
    return {"sse": sse, "live": live, "cos": z(cos), "angle": z(np.arccos(cos)), "lo": z(lo), "hi": z(hi)}


@functools.lru_cache(maxsize=None)
def pixel_reference(n: int, K: int) -> Tuple[Dict, Dict]:
    """(case, float64 run), computed once and shared; neither is to be changed.  n == 0: the sparse layout at K bands."""
    case = make_sparse_case(K) if n == 0 else make_pixel_case(n, K)
    return case, pixels64(case)


def block_sums(x: np.ndarray, n_partial: int) -> np.ndarray:
    """[n] -> [n_partial]: the sum over the pixels p with (p / 256) % n_partial == b (the header's ownership)."""
    owner = (np.arange(x.shape[0]) // BLOCK) % n_partial
    out = np.zeros(n_partial, np.float64)
    with np.errstate(invalid="ignore"):
        np.add.at(out, owner, x.astype(np.float64))
    return out


def check_pixels(partial, r64: Dict, n_partial: int, k_sse: float = K_SSE, report: Optional[Dict] = None, prefix: str = "") -> List[str]:
    """SSE rule, angle-sum rule and exact count per slot; report[prefix + "sse" / "sam"] = {"worst", "n"} (sam: the distance from the
    middle of the interval over its half width, so 1.0 is the edge of the rule)."""
    got = np.asarray(partial, dtype=np.float64).reshape(-1, 3)
    if got.shape[0] != n_partial:
        return [f"{prefix}{got.shape[0]} slots, want {n_partial}"]
    fails: List[str] = []
    sse, lo, hi, cnt = (block_sums(r64[k], n_partial) for k in ("sse", "lo", "hi", "live"))
    fin = np.isfinite(sse)
    same = (np.isnan(got[:, 0]) & np.isnan(sse)) | (got[:, 0] == sse)
    if bool((~fin & ~same).any()):
        fails.append(f"{prefix}sse: {int((~fin & ~same).sum())} slots whose float64 sum is NaN / Inf hold something else")
    d = np.abs(got[fin, 0] - sse[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d == 0, 0.0, d / (U * sse[fin]))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > k_sse:
        i = int(ratio.argmax())
        fails.append(f"{prefix}sse: finite slot {i}: {got[fin, 0][i]:.12g} vs float64 {sse[fin][i]:.12g} = {worst:.3g} u (K = {k_sse:g})")
    if bool((got[:, 2] != cnt).any()):
        i = int((got[:, 2] != cnt).nonzero()[0][0])
        fails.append(f"{prefix}cnt: slot {i} counts {got[i, 2]:g} angles, {cnt[i]:g} pixels of it are live ({int((got[:, 2] != cnt).sum())} slots)")
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = np.where(got[:, 1] == mid, 0.0, np.abs(got[:, 1] - mid) / half)
    rs = np.where(np.isnan(rs), np.inf, rs)
    if float(rs.max()) > 1.0:
        i = int(rs.argmax())
        fails.append(f"{prefix}sam: slot {i}: {got[i, 1]:.12g} outside [{lo[i]:.12g}, {hi[i]:.12g}] ({int((rs > 1).sum())} slots)")
    if report is not None:
        report[prefix + "sse"] = {"worst": worst, "n": int(fin.sum())}
        report[prefix + "sam"] = {"worst": float(rs.max()), "n": n_partial}
    return fails


def magnitudes(case: Dict, r64: Dict) -> Tuple[float, float]:
    """(smallest, largest) magnitude of the non-zero values of the live pixels."""
    x = np.abs(np.concatenate([case["pred"][r64["live"]].reshape(-1), case["gt"][r64["live"]].reshape(-1)]).astype(np.float64))
    x = x[x > 0]
    return (float(x.min()), float(x.max())) if x.size else (1.0, 1.0)


def wrapper_blocks(n: int) -> int:
    """The grid ops.pixel_metrics chooses."""
    return max(1, min(MAX_BLOCKS, (n + BLOCK - 1) // BLOCK))


# ------------------------------------------------------------------------------------------------------------------------------ #
# pixel metrics: the float32 restatement (NOT an oracle)
# ------------------------------------------------------------------------------------------------------------------------------ #
PIXEL_FAULTS = ["SAM clamp removed", "zero spectra counted", "second trip dropped"]


def pixels32(case: Dict, n_partial: int, fault: Optional[str] = None) -> np.ndarray:
    """partial float64 [n_partial,3] in the kernel's operation order: k ascending, one float32 rounding per operation, e * e widened
    and added in double, c = dot / (sqrt(pp) sqrt(gg)), skipped when NaN, acos of the clamp in float32."""
    f = np.float32
    a, b = case["pred"], case["gt"]
    n, K = a.shape
    sse, dot, pp, gg = np.zeros(n, np.float64), np.zeros(n, f), np.zeros(n, f), np.zeros(n, f)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            e = a[:, k] - b[:, k]
            sse += (e * e).astype(np.float64)
            dot, pp, gg = dot + a[:, k] * b[:, k], pp + a[:, k] * a[:, k], gg + b[:, k] * b[:, k]
        c = dot / (np.sqrt(pp) * np.sqrt(gg))
        assert c.dtype == np.float32
        if fault == "zero spectra counted":
            c = np.where((pp == 0) | (gg == 0), f(1), c)
        counted = ~np.isnan(c)
        ang = np.arccos(c if fault == "SAM clamp removed" else np.clip(c, f(-1), f(1))).astype(np.float64)
    if fault == "SAM clamp removed":
        counted &= ~np.isnan(ang)
    ang = np.where(counted, ang, 0.0)
    if fault == "second trip dropped":
        gone = np.arange(n) >= n_partial * BLOCK
        sse, ang, counted = np.where(gone, 0.0, sse), np.where(gone, 0.0, ang), counted & ~gone
    return np.stack([block_sums(sse, n_partial), block_sums(ang, n_partial), block_sums(counted.astype(np.float64), n_partial)], 1)
