"""Density-gradient normal cases, their float64 oracle, a float32 model of the kernel's arithmetic and the comparators (plain helper
module, no tests in it).

Used by tests/test_hip_normals.py (csrc/umhs_normals.hip on the GPU) and tests/test_normals_bounds_cpu.py (the comparators pass the
float32 model and reject planted faults; K and the teeth condition are measured there).  It mirrors tests/hash_f64.py one stage later
and takes its position sets and its geometry (``hash_f64.positions``, ``hash_f64.geometry``) from there.

ORACLE (``evaluate(..., np.float64)``).  The definitions are those of include/umhs_hip.h, "Density-gradient normals", steps 1-6.  As
for the hash grid's forward, the float32 ``pos01`` bits, the ONE float32 product pos01 * scale_l, its floor / ceil and the exact
offset DEFINE the cell and the offsets; the oracle takes them and the integer corners as they are (``hash_f64.geometry``) and does
everything downstream in float64: corner differences and their blends, h, the ReLU mask, q, g01, the position Jacobian from the
float32 ``wpos`` bits (the box extents from the float32 aabb), exp(clamp(sigma_raw)), grad, normal.  A genuine float64 x * scale, or
a pos01 recomputed in float64 from the world position, is the WRONG truth: it moves every offset by up to half an ulp of a coordinate
of ~2047 and the gradient with it (tests/test_normals_bounds_cpu.py measures both).
Next to each value stands its envelope ``mag``, the float64 sum of the absolute values of the same terms:
  d enc / d axis   the same blend tree over (|f_ceil| + |f_floor|)
  q_j              sum_k |c_k W0[k,j]|                      (c_k = W1[0,k] where h_k > 0, else 0)
  g01_a            sum_l scale_l (mag_q[2l] mag_d[l,0,a] + mag_q[2l+1] mag_d[l,1,a])
  gw_j             contraction: (|s| mag_g01_j + delta_jk |t| sum_i |x_i| mag_g01_i) / 4; inside the unit box mag_g01_j / 4;
                   box: mag_g01_j / extent_j
  grad             sel exp(clamp(sigma_raw, -15, 15)) mag_gw

RULES, u = 2^-24, tiny = 2^-126:
  g01, grad, every element:   |got - ref64| <= K u (mag + tiny)
  normal, per component:      |got - ref64| <= 2 B1 / |grad_ref| + 4 u,  B1 = the L1 norm of the sample's three grad bounds; asserted
                              on samples with teeth, |grad_ref| > 16 B1 (elsewhere the direction is not determined by the data)
  sel == 0:                   exactly +0 in every output (pos01 is 0 there: every axis sits on an integer coordinate)
  all hidden units inactive:  q = 0, so grad and normal are exactly 0
K = max(8, 4 x worst, rounded up to a power of two), with the reasons of tests/rays_f64.py (floor of 8: device expf and the kernel's
fma chains may differ by a couple of ulp from the model; factor 4: margin over a float32 evaluation in another order).  ``worst`` is
measured on the CPU from the float32 model (``evaluate(..., np.float32)``: the kernel's operation order with every multiply and add
rounded separately -- numpy has no fma, so the model rounds more often than the kernel, never less) over every committed case.
Measured worsts (tests/test_normals_bounds_cpu.py re-measures and asserts 4 x worst <= K):
  g01 0.51 | grad 0.63 (both on the envelope of every product, which is generous: the sums behind one element are long)
so K_G01 = K_GRAD = 8, the floor.
TEETH: at least 90 % of the sel = 1 samples of the "scattered" and "rays" cases have teeth (checked on the CPU from the float64 run
alone).  The table is U(-1, 1) x 0.1, which gives |g01| of some tens (median 54 and 68 in the two cases).

THE RELU KINK.  q is a step function of h: where a hidden pre-activation is within rounding of 0, a float32 evaluation and float64
legitimately disagree about a whole unit.  The cases stay clear of it: a random candidate position with |h_k| < 64 u mag_h for some k
(mag_h = |b0| + sum_j |W0[k,j] enc_j|) is replaced by the next candidate (``_kink_free``), and the CPU test asserts that no committed
sample, the fixed edge rows included, is closer than that.

CASES (``CASES``; position sets of tests/hash_f64.py where pos01 is given directly -- then sel = 1, wpos = pos01, no contraction and
the unit box, so gw = g01):
  one12 (N = 1) | edges13_63, edges12_64, edges13_65 (the edge set: integer coordinates on one, two and three axes, 0.0 and 1.0, the
  float neighbours of an integer; one lane short of a wave, a full wave, one lane into the second) | scattered12 (N = 3077), rays13
  (N = 3077) | scattered19 (N = 257)
  contract13 (N = 257), contract12 (N = 65): world positions through the L-inf contraction: inside the unit box, outside it up to
  |x| = 9, the largest component one float below 1, at 1 and one float above, on every axis and with both signs, and exact ties of
  the maximum (two and three axes, mixed signs: the LOWEST index wins)
  box13 (N = 257): no contraction, box (-1, -2, -0.5) .. (1, 2, 1.5), a quarter of the points outside it (sel = 0)
  inactive12 (N = 64): b0 = -1 and |W0| small: every hidden unit inactive
  sigma_hi13, sigma_lo13 (N = 65): b1[0] = +40 / -40, sigma_raw beyond the clamp of trunc_exp's derivative on either side
Weights: W0, W1 ~ U(-1, 1) x 0.3, b0 ~ U(-1, 1) x 0.05, b1 ~ U(-1, 1) x 0.1 (h is then of the size of b0: about half the units
active)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

import hash_f64 as H

U = 2.0 ** -24
TINY = 2.0 ** -126
TEETH = 16.0
K_G01 = 8.0
K_GRAD = 8.0
WORST_G01 = 0.51  # measured (see above)
WORST_GRAD = 0.63
KINK = 64.0  # a committed sample keeps |h_k| >= KINK u mag_h for every hidden unit
TABLE_SCALE = 0.1
UNIT_BOX = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
BOX = (-1.0, -2.0, -0.5, 1.0, 2.0, 1.5)
FAULTS = ("sign", "scale", "swap_x", "relu", "rank_one", "quarter", "extent", "clamp")

# name: (position set, log2_T, N, mode, weight variant); mode: "direct" (pos01 given), "contract", "box"
CASES: Dict[str, Tuple[str, int, int, str, str]] = {
    "one12": ("one_cell", 12, 1, "direct", "plain"),
    "edges13_63": ("edges", 13, 63, "direct", "plain"), "edges12_64": ("edges", 12, 64, "direct", "plain"),
    "edges13_65": ("edges", 13, 65, "direct", "plain"),
    "scattered12": ("scattered", 12, 3077, "direct", "plain"), "rays13": ("rays", 13, 3077, "direct", "plain"),
    "scattered19": ("scattered", 19, 257, "direct", "plain"),
    "contract13": ("world", 13, 257, "contract", "plain"), "contract12": ("world", 12, 65, "contract", "plain"),
    "box13": ("world", 13, 257, "box", "plain"),
    "inactive12": ("scattered", 12, 64, "direct", "inactive"),
    "sigma_hi13": ("scattered", 13, 65, "direct", "sigma_hi"), "sigma_lo13": ("scattered", 13, 65, "direct", "sigma_lo"),
}
TEETH_CASES = ("scattered12", "rays13")


def report_dir(root: str) -> str:
    import rays_f64

    return rays_f64.report_dir(root)


# ------------------------------------------------------------------------------------------------------------------------------ #
# inputs
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class Weights:
    table: torch.Tensor  # [16 << log2_T, 2]
    w0: torch.Tensor  # [64, 32]
    b0: torch.Tensor  # [64]
    w1: torch.Tensor  # [16, 64]
    b1: torch.Tensor  # [16]
    log2_T: int


def make_weights(log2_T: int, variant: str = "plain", seed: int = 0) -> Weights:
    g = torch.Generator().manual_seed(7400 + log2_T + 100 * seed)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    table = r(16 << log2_T, 2) * TABLE_SCALE
    w0, b0, w1, b1 = r(64, 32) * 0.3, r(64) * 0.05, r(16, 64) * 0.3, r(16) * 0.1
    if variant == "inactive":
        w0, b0 = w0 * 0.1, torch.full((64,), -1.0)
    elif variant == "sigma_hi":
        b1[0] = 40.0
    elif variant == "sigma_lo":
        b1[0] = -40.0
    elif variant != "plain":
        raise KeyError(variant)
    return Weights(table.contiguous(), w0.contiguous(), b0.contiguous(), w1.contiguous(), b1.contiguous(), log2_T)


def world_positions(n: int, mode: str, seed: int = 0) -> torch.Tensor:
    """float32 world positions [n + 32, 3]: the fixed rows first, random ones behind them (32 spare candidates for ``_kink_free``)."""
    g = torch.Generator().manual_seed(8500 + seed)
    m = n + 32
    if mode == "box":
        lo, hi = torch.tensor(BOX[:3]), torch.tensor(BOX[3:])
        x = lo + (hi - lo) * (torch.rand(m, 3, generator=g) * 1.1 - 0.05)  # a quarter or so outside, on every side
        return x.float().contiguous()
    one = np.float32(1.0)
    below, above = float(np.nextafter(one, np.float32(0))), float(np.nextafter(one, np.float32(2)))
    rows: List[List[float]] = []
    for v in (below, 1.0, above):  # one float either side of 1, on every axis and with both signs
        rows += [[v, 0.31, -0.47], [0.12, -v, 0.66], [-0.58, 0.23, v], [-v, -0.9, 0.2]]
    rows += [[1.5, 1.5, 0.3], [-2.0, 0.1, 2.0], [0.4, 3.0, -3.0], [2.5, -2.5, 2.5], [-1.0, 1.0, 0.5]]  # exact ties of the maximum
    fixed = torch.tensor(rows, dtype=torch.float32)
    k = m - fixed.shape[0]
    inside = torch.rand(k, 3, generator=g) * 1.9 - 0.95
    d = torch.nn.functional.normalize(torch.randn(k, 3, generator=g), dim=-1)
    outside = d * (1.0 + 8.0 * torch.rand(k, 1, generator=g) ** 2)
    pick = (torch.arange(k) % 2 == 0)[:, None]
    x = torch.cat([fixed, torch.where(pick, inside, outside)])
    return x[:m].float().contiguous()


def positions_model(wpos: torch.Tensor, contraction: bool, aabb) -> Tuple[torch.Tensor, torch.Tensor]:
    """positions_kernel of csrc/umhs_rays.hip in float32 torch, operation for operation -> (pos01 [N,3], sel [N])."""
    p = wpos.float()
    if contraction:
        mag = p.abs().amax(dim=-1, keepdim=True)
        sc = 2.0 - (1.0 / mag)
        q = torch.where(mag < 1.0, p, sc * (p / mag))
        q = (q + 2.0) / 4.0
    else:
        a, b = torch.tensor(aabb[:3], dtype=torch.float32), torch.tensor(aabb[3:], dtype=torch.float32)
        q = (p - a) / (b - a)
    sel = ((q > 0.0) & (q < 1.0)).all(dim=-1).float()
    return (q * sel[:, None]).contiguous(), sel.contiguous()


@dataclass
class Case:
    name: str
    weights: Weights
    contraction: bool
    aabb: Tuple[float, ...]
    wpos: torch.Tensor  # [N, 3] float32
    pos01: torch.Tensor  # [N, 3] float32
    sel: torch.Tensor  # [N] float32
    _runs: Dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return self.pos01.shape[0]

    def run(self, dt=np.float64, fault: Optional[str] = None) -> Dict[str, np.ndarray]:
        key = (np.dtype(dt).name, fault)
        if key not in self._runs:
            self._runs[key] = evaluate(self.weights, self.pos01, self.wpos, self.sel, self.contraction, self.aabb, dt, fault)
        return self._runs[key]


def _kink_free(w: Weights, pos01: torch.Tensor, sel: torch.Tensor, n: int, n_fixed: int) -> np.ndarray:
    """Indices of the first n candidates that keep every |h_k| >= 4 KINK u mag_h (the fixed rows are kept as they are)."""
    r = evaluate(w, pos01, pos01, sel, False, UNIT_BOX, np.float64, None, upto="h")
    ok = (np.abs(r["h"]) >= 4 * KINK * U * r["mag_h"]).all(axis=1)
    ok[:n_fixed] = True
    idx = np.nonzero(ok)[0][:n]
    assert idx.size == n, "not enough kink-free candidates"
    return idx


_cases: Dict[str, Case] = {}


def case(name: str, positions_fn: Optional[Callable] = None, weights: Optional[Weights] = None) -> Case:
    """The committed case ``name``.  positions_fn(wpos, contraction, aabb) -> (pos01, sel): whose bits define the cell (the GPU test
    passes umhs_positions_fwd; default: its float32 model).  weights: other weights for the same positions (not cached)."""
    if name in _cases and positions_fn is None and weights is None:
        return _cases[name]
    kind, log2_T, n, mode, variant = CASES[name]
    w = weights if weights is not None else make_weights(log2_T, variant)
    if mode == "direct":
        n_fixed = min(n, H.edge_positions().shape[0]) if kind == "edges" else (n if kind == "one_cell" else 0)
        cand = H.positions(kind, n if kind == "one_cell" else n + 32, seed=1)
        sel = torch.ones(cand.shape[0])
        keep = _kink_free(w, cand, sel, n, n_fixed)
        pos01 = cand[keep].contiguous()
        c = Case(name, w, False, UNIT_BOX, pos01.clone(), pos01, torch.ones(n))
    else:
        contraction = mode == "contract"
        aabb = UNIT_BOX if contraction else BOX
        cand = world_positions(n, mode)
        pos01, sel = positions_model(cand, contraction, aabb)
        n_fixed = 0 if mode == "box" else 17  # (the fixed rows of world_positions)
        keep = _kink_free(w, pos01, sel, n, n_fixed)
        wpos = cand[keep].contiguous()
        pos01, sel = (positions_fn or positions_model)(wpos, contraction, aabb)
        c = Case(name, w, contraction, aabb, wpos, pos01.contiguous(), sel.contiguous())
    if positions_fn is None and weights is None:
        _cases[name] = c
    return c


# ------------------------------------------------------------------------------------------------------------------------------ #
# the definitions, in float64 (oracle) or float32 in the kernel's operation order (model)
# ------------------------------------------------------------------------------------------------------------------------------ #
def _dblend(f, o, one, absolute: bool):
    """d(blend) / d(offset) on the three axes, [N, L, 2, 3]: the forward's tree with the corners of an axis replaced by ceil - floor
    (absolute: |ceil| + |floor|, the envelope)."""
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]
    rx, ry, rz = one - ox, one - oy, one - oz
    c = lambda i: np.abs(f[..., i, :]) if absolute else f[..., i, :]
    d = (lambda a, b: c(a) + c(b)) if absolute else (lambda a, b: c(a) - c(b))
    dx = (d(0, 3) * oy + d(1, 2) * ry) * oz + (d(4, 7) * oy + d(5, 6) * ry) * rz
    dy = (d(0, 1) * ox + d(3, 2) * rx) * oz + (d(4, 5) * ox + d(7, 6) * rx) * rz
    dz = (d(0, 4) * ox + d(3, 7) * rx) * oy + (d(1, 5) * ox + d(2, 6) * rx) * ry
    return np.stack([dx, dy, dz], axis=-1)


def evaluate(w: Weights, pos01, wpos, sel, contraction: bool, aabb, dt=np.float64, fault: Optional[str] = None,
             upto: Optional[str] = None) -> Dict[str, np.ndarray]:
    """Steps 1-6 on float32 inputs in arithmetic ``dt``.  float64: the oracle and its envelopes.  float32: the kernel's operation
    order (h as a chain over j, q and sigma_raw as chains over k, g01 as a chain over the levels).  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    f64 = np.dtype(dt) == np.float64
    geo = H.geometry(pos01, H.ALL_LEVELS, w.log2_T)
    n = geo.n
    t = w.table.numpy().reshape(16, 1 << w.log2_T, 2)
    f = t[np.arange(16)[None, :, None], geo.idx].astype(dt)  # [N, L, 8, 2]
    o, one = geo.off.astype(dt), dt(1.0)
    enc = H._blend(f, o[..., 0:1], o[..., 1:2], o[..., 2:3], one).reshape(n, 32)
    W0, b0, W1, b1 = (a.numpy().astype(dt) for a in (w.w0, w.b0, w.w1[0], w.b1[0]))
    out: Dict[str, np.ndarray] = {}
    if f64:
        h = enc @ W0.T + b0
        out["mag_h"] = np.abs(enc) @ np.abs(W0).T + np.abs(b0)
    else:
        h = np.broadcast_to(b0, (n, 64)).copy()
        for j in range(32):
            h = h + W0[None, :, j] * enc[:, j:j + 1]
    out["h"] = h
    if upto == "h":
        return out
    active = np.ones_like(h, bool) if fault == "relu" else h > 0
    c = np.where(active, W1[None, :], dt(0.0))  # [N, 64]
    if f64:
        sigma = b1 + (c * h).sum(1)
        q = c @ W0
        mag_q = np.abs(c) @ np.abs(W0)
    else:
        sigma, q = np.full(n, b1, dt), np.zeros((n, 32), dt)
        for k in range(64):
            sigma = sigma + c[:, k] * h[:, k]
            q = q + c[:, k:k + 1] * W0[k][None, :]
    d = _dblend(f, o, one, False)  # [N, L, 2, 3]
    if fault == "swap_x":
        d[..., 0] = -d[..., 0]
    sc = H.T.hash_scalings().numpy().astype(dt)
    if fault == "scale":
        sc = np.ones_like(sc)
    ql = q.reshape(n, 16, 2)
    if f64:
        g01 = (sc[None, :, None] * (ql[..., 0:1] * d[:, :, 0] + ql[..., 1:2] * d[:, :, 1])).sum(1)
        dm, qm = _dblend(f, o, one, True), mag_q.reshape(n, 16, 2)
        mag_g01 = (sc[None, :, None] * (qm[..., 0:1] * dm[:, :, 0] + qm[..., 1:2] * dm[:, :, 1])).sum(1)
    else:
        g01 = np.zeros((n, 3), dt)
        for l in range(16):
            g01 = g01 + sc[l] * (ql[:, l, 0:1] * d[:, l, 0] + ql[:, l, 1:2] * d[:, l, 1])
        mag_g01 = None
    x = wpos.numpy().astype(dt)
    quarter = dt(1.0) if fault == "quarter" else dt(0.25)
    if contraction:
        ax = np.abs(x)
        m = ax.max(1)
        k = ax.argmax(1)  # the first index of the maximum: ties go to the lowest
        outside = m >= 1
        ms = np.where(outside, m, dt(1.0))
        r = one / ms
        s, tt = dt(2.0) * r - r * r, dt(2.0) * r * r * r - dt(2.0) * r * r
        dot = (x * g01).sum(1)
        sgn = np.where(x[np.arange(n), k] < 0, dt(-1.0), dt(1.0))
        e = np.zeros((n, 3), dt)
        if fault != "rank_one":
            e[np.arange(n), k] = tt * dot * sgn
        gw = np.where(outside[:, None], (s[:, None] * g01 + e) * quarter, g01 * quarter)
        if f64:
            em = np.zeros((n, 3))
            em[np.arange(n), k] = np.abs(tt) * (ax * mag_g01).sum(1)
            mag_gw = np.where(outside[:, None], (np.abs(s)[:, None] * mag_g01 + em) * 0.25, mag_g01 * 0.25)
    else:
        a32 = np.asarray(aabb, np.float32)
        ext = np.ones(3, dt) if fault == "extent" else a32[3:].astype(dt) - a32[:3].astype(dt)
        gw = g01 / ext
        if f64:
            mag_gw = mag_g01 / np.abs(a32[3:].astype(dt) - a32[:3].astype(dt))
    ex = np.exp(sigma if fault == "clamp" else np.clip(sigma, dt(-15.0), dt(15.0))).astype(dt)
    live = sel.numpy() != 0
    grad = np.where(live[:, None], ex[:, None] * gw, dt(0.0))
    if fault == "sign":
        grad = -grad
    with np.errstate(over="ignore"):  # (the planted fault without the clamp overflows float32 on purpose)
        length = np.sqrt((grad * grad).sum(1)).astype(dt) + dt(1e-10)
    normal = np.where(live[:, None], -grad / length[:, None], dt(0.0))
    out.update(enc=enc, q=q, sigma=sigma, g01=g01, grad=grad, normal=normal, live=live)
    if f64:
        out.update(mag_g01=mag_g01, mag_grad=np.where(live[:, None], ex[:, None] * mag_gw, 0.0))
    return out


# ------------------------------------------------------------------------------------------------------------------------------ #
# comparators
# ------------------------------------------------------------------------------------------------------------------------------ #
def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def ratios(got, ref: np.ndarray, mag: np.ndarray) -> np.ndarray:
    """|got - ref64| / (u (mag + tiny)) per element; a non-finite value counts as infinitely far."""
    g = _np(got).astype(np.float64)
    d = np.abs(g - ref)
    r = np.where(d == 0, 0.0, d / (U * (mag + TINY)))
    return np.where(np.isfinite(g), r, np.inf)


def check_vec(name: str, what: str, got, ref: np.ndarray, mag: np.ndarray, K: float, report: Optional[Dict] = None) -> List[str]:
    r = ratios(got, ref, mag)
    worst = float(r.max()) if r.size else 0.0
    if report is not None:
        report.setdefault(name, {})[what] = worst
    if worst > K:
        i = np.unravel_index(int(r.argmax()), r.shape)
        return [f"{name} {what}{list(i)}: {float(_np(got)[i]):.9g} vs float64 {float(ref[i]):.9g} = {worst:.3g} u mag (K = {K:g}, mag "
                f"{float(mag[i]):.3g}; {int((r > K).sum())} of {r.size} over)"]
    return []


def teeth_mask(r64: Dict[str, np.ndarray], K: float = K_GRAD) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(teeth [N] bool, B1 [N], |grad_ref| [N]) from the float64 run alone."""
    b1 = (K * U * (r64["mag_grad"] + TINY)).sum(1)
    gn = np.sqrt((r64["grad"] ** 2).sum(1))
    return r64["live"] & (gn > TEETH * b1), b1, gn


def check_normal(name: str, got, r64: Dict[str, np.ndarray], K: float = K_GRAD, report: Optional[Dict] = None) -> List[str]:
    teeth, b1, gn = teeth_mask(r64, K)
    g = _np(got).astype(np.float64)
    bound = 2.0 * b1 / np.where(teeth, gn, 1.0) + 4.0 * U
    d = np.abs(g - r64["normal"]).max(1)
    r = np.where(teeth, np.where(np.isfinite(d), d / bound, np.inf), 0.0)
    worst = float(r.max()) if r.size else 0.0
    if report is not None:
        report.setdefault(name, {}).update(normal=worst, teeth=float(teeth.sum()) / max(1, int(r64["live"].sum())))
    if worst > 1.0:
        i = int(r.argmax())
        return [f"{name} normal[{i}]: {g[i]} vs float64 {r64['normal'][i]}: {worst:.3g} x its bound {bound[i]:.3g} ({int((r > 1).sum())} over)"]
    return []


def check_dead(name: str, outs: Dict[str, object], r64: Dict[str, np.ndarray]) -> List[str]:
    """sel == 0: exactly +0 (the bits) in every output."""
    dead = ~r64["live"]
    fails = []
    for what, got in outs.items():
        bits = _np(got).view(np.uint32)[dead]
        if bits.size and bits.any():
            fails.append(f"{name} {what}: {int((bits != 0).any(1).sum())} samples with sel = 0 are not exactly +0")
    return fails


def check_all(name: str, outs: Dict[str, object], r64: Dict[str, np.ndarray], report: Optional[Dict] = None) -> List[str]:
    """outs: any of "g01", "grad", "normal" ([N,3] float32 tensors or arrays) against the float64 run."""
    fails = check_dead(name, outs, r64)
    if "g01" in outs:
        fails += check_vec(name, "g01", outs["g01"], r64["g01"], r64["mag_g01"], K_G01, report)
    if "grad" in outs:
        fails += check_vec(name, "grad", outs["grad"], r64["grad"], r64["mag_grad"], K_GRAD, report)
    if "normal" in outs:
        fails += check_normal(name, outs["normal"], r64, K_GRAD, report)
    return fails


def k_from(worst: float) -> float:
    return max(8.0, 2.0 ** np.ceil(np.log2(max(4.0 * worst, 1e-30))))


# ------------------------------------------------------------------------------------------------------------------------------ #
# step 7 (per ray) in float64, for tests/test_hip_normals_model.py
# ------------------------------------------------------------------------------------------------------------------------------ #
def ray_normals64(weights, normal, packed_info) -> Tuple[np.ndarray, np.ndarray]:
    """(normals [R,3] in [0,1], mag [R,3] = sum |w n| per component) from float32 weights [N], per-sample normals [N,3] and
    packed_info [R,2], in float64."""
    wt, nm, pi = _np(weights).astype(np.float64).reshape(-1), _np(normal).astype(np.float64), _np(packed_info)
    R = pi.shape[0]
    ray = np.repeat(np.arange(R), pi[:, 1])
    order = np.concatenate([np.arange(s, s + c) for s, c in pi]) if R else np.zeros(0, np.int64)
    N, mag = np.zeros((R, 3)), np.zeros((R, 3))
    np.add.at(N, ray, wt[order, None] * nm[order])
    np.add.at(mag, ray, np.abs(wt[order, None] * nm[order]))
    nh = N / (np.sqrt((N * N).sum(1, keepdims=True)) + 1e-10)
    return (nh + 1.0) / 2.0, mag
