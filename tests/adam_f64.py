"""Replay, float64 oracle, error envelope, comparator and cases of the Adam update (csrc/umhs_adam.h: ``adam_update`` and ``adam_bias``;
csrc/umhs_adam.hip: adam_kernel, adam_rows_kernel, adam_rows_range_kernel; the ``step4`` epilogue of hg_reduce_kernel in
csrc/umhs_hashgrid_part.h).  Plain numpy, a helper module with no tests in it.

Used by tests/test_adam_f64_bounds_cpu.py (the helper itself: hand-made elements, torch.optim.Adam in float64, mutants the comparator
must reject), tests/test_adam_partition_cpu.py (``UMHSAdam.step`` cuts the flat buffer so that every element is updated exactly once),
tests/test_hip_adam_f64.py (the three kernels and ``UMHSAdam.step`` on the GPU) and tests/test_hip_hash_f64.py (the fused epilogue).
It follows tests/stats_f64.py and tests/hash_f64.py.

THE UPDATE, per element, with the host's two bias factors (``bias``: lr, b1, b2 rounded to float32 as the C ABI's float arguments are,
1 - b^step in double, then lr_bc1 = float32(lr / bc1) and sqrt_bc2 = float32(sqrt(bc2))):
    gk    = g * grad_scale
    m'    = m * b1 + gk * (1 - b1)
    v'    = v * b2 + (gk * gk) * (1 - b2)
    denom = sqrt(v') / sqrt_bc2 + eps
    p'    = p - lr_bc1 * (m' / denom)
    p'    = p' < 0 ? 0 : p' > 1 ? 1 : p'  for elements in [clamp_begin, clamp_end)   (``adam_clamp01``; not in the fused epilogue)
1 - b1 and 1 - b2 are exact in float32 for betas in [0.5, 1] (Sterbenz), so they carry no rounding in any precision.

REPLAY (``replay``): that expression in numpy float32, one IEEE operation per kernel operation, in the kernel's order, nothing fused.
umhs_adam.h switches contraction off and promises "the same bits" from every kernel it is inlined into: the replay is the
expectation for BITS.  m' and v' are made of multiplications and additions only, which IEEE fixes to the last bit: any difference there
means a contraction or a reordering.  p' also passes through sqrtf and two divisions, which IEEE rounds correctly and hipcc compiles to
the correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup, no bare v_rcp), so p' is expected to be bit-equal as well;
``check(p_bits=False)`` counts such differences and their distance in ulps instead of failing on them, the envelope below then being the
assertion for p'.  The clamp is torch.clamp_(0, 1) by two comparisons: it keeps a NaN (fminf(fmaxf(p', 0), 1) would return 0 for it,
and a parameter whose moments a non-finite gradient has poisoned would read 0 for ever) and it keeps -0.

ORACLE AND ENVELOPE (``oracle``): the same update in float64 from the same float32 inputs and the same float32 hyper-parameters, with a
running first-order envelope e_x beside every intermediate x: a bound on |float32 value - float64 value|.  Inputs are exact (e = 0).
Every kernel operation adds  u |result| + 2^-149  to the propagated input error; 2^-149 covers results in float32's subnormal range
(the code object keeps them: denorm_mode_32 = 3), where the rounding error is absolute, and results that underflow to zero.
    u = 2^-24 for *, +, -          (round to nearest)
    u = 2^-23 for sqrtf and /      (faithful rounding: the float64 assertion does not need them correctly rounded)
Propagation, t = 2^-149, U = 2^-24, U2 = 2^-23, |x~ - x| <= e_x for the float32 value x~ of x:
    product by an exact constant c     e = c e_x + U |x c| + t
    gk * gk                            e = 2 |gk| e_gk + e_gk^2 + U gk^2 + t
    sum a + b                          e = e_a + e_b + U |a + b| + t
    sqrt(v)                            e = sqrt(v + e_v) - sqrt(max(v - e_v, 0)) + U2 sqrt(v) + t
                                       (the width of the interval's image: sqrt is monotone, and v -> 0 needs no derivative)
    quotient a / b                     e = (|a| + e_a) / (|b| - e_b) - |a / b| + U2 |a / b| + t      with |b| > e_b asserted
                                       (the quotient farthest from a / b in the box; it holds because denom >= eps and sqrt_bc2 > 0)
    clamp                              exact and 1-Lipschitz: |clamp(x~) - clamp(x)| <= e_x, so the clamped oracle keeps p's envelope --
                                       where the oracle's p lies within its envelope of 0 or 1, either side passes.
On the cases below (2.1 million elements in the largest) the replay's worst |float32 - float64| / envelope is 0.999 for p, 0.972 for
m and 0.984 for v -- the kernels on an MI355X give the same figures, being bit-equal -- and the envelope's median is about one ulp
of p.  It has teeth: of the mutants of tests/test_adam_f64_bounds_cpu.py, "b2 = 0.99" leaves it on 45-72 % of the elements of a case,
"step + 1" on 55-76 %, "eps = 1e-8" on 18-38 % -- except "no sqrt_bc2" and "step + 1" from step 30000 on, where both bias terms are 1:
hence several steps in the case list.

RULES (``check``), per call: m', v' equal the replay's bits; p', m', v' each within the envelope of the oracle; p' equal to the replay's
bits (see above); NaN, +Inf and -Inf exactly where the replay has them (NaN payloads are not compared); every element the call must
not touch keeps its bits -- the buffers are filled with non-zero values everywhere, so a stray update shows.

CASES (``CASES``, built by ``case``): named and seeded.  Gradients log-uniform 1e-30 .. 1e18 of both signs (g * g stays finite in
float32), exact +0 / -0, a few NaN, +Inf, -Inf; moments zero (a first step) or alive: m of both signs, v >= 0 from subnormal to 1e20;
"gradient 0, moments alive" (the parameter still moves) and "gradient 0, moments 0" (p keeps its bits); around both ends of the clamp
range, inside and just outside, p within one step of 0 and of 1 on both sides, and a NaN gradient inside it.  Steps 1, 2, 10, 1000, 30000, 2^31 + 1; grad_scale 1,
0.5, 1/3; eps 1e-15 (the project's) and 1e-8.  Shapes are the smallest at which each kernel takes another path:
  dense       n = 1, 3, 4, 5 (scalar tail alone, one float4, float4 + tail), 1023, 1025 (a second workgroup), 262147, and
              2048 * 256 * 4 + 7 = 2097159: one grid stride of the capped grid plus a float4 plus a scalar tail, all in the second loop
              trip; the call is made on the slice [12, 12 + n) of a buffer; clamp ranges with ends off the float4 grid: one straddling
              a float4 boundary, one covering the scalar tail, one empty
  rows        1, 255, 256, 257 rows (around one workgroup) out of 4096, unique, unordered, with row 0 and the last row
  rows+range  (rows, range) = (0, 5), (257, 0), (1, 1), (257, 255), (300, 256 * 1024 + 5: past the 1024-workgroup cap, the stride loop);
              the range begins at an odd element; clamps in absolute elements, one inside the range, one reaching across its begin
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24  # *, +, -
U2 = 2.0 ** -23  # sqrtf, /
T = 2.0 ** -149  # float32's smallest subnormal
STEPS = (1, 2, 10, 1000, 30000, 2 ** 31 + 1)
SCALES = (1.0, 0.5, 1.0 / 3.0)
EPSS = (1e-15, 1e-8)
LEAD, TRAIL = 12, 9  # elements in front of and behind the dense call's slice
N_ROWS_BUFFER = 4096
RANGE_BEGIN = 2 * N_ROWS_BUFFER + 9  # odd


class Hyper(NamedTuple):
    lr: float
    b1: float
    b2: float
    eps: float
    step: int


def report_dir(root: str) -> str:
    import rays_f64

    return rays_f64.report_dir(root)


def exp_decay_lr(step: int, lr_init: float = 2e-2, lr_final: float = 1e-5, max_steps: int = 30000) -> float:
    """umhsnerf.optim.exp_decay_lr, repeated so that this module needs no torch."""
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def bias(lr: float, b1: float, b2: float, step: int) -> Tuple[np.float32, np.float32]:
    """(lr_bc1, sqrt_bc2) of ``adam_bias``: float32 arguments, 1 - b^step in double, two roundings to float32."""
    lr, b1, b2 = float(F32(lr)), float(F32(b1)), float(F32(b2))
    bc1, bc2 = 1.0 - math.pow(b1, float(step)), 1.0 - math.pow(b2, float(step))
    return F32(lr / bc1), F32(math.sqrt(bc2))


def _clamp_mask(n: int, clamp) -> np.ndarray:
    mask = np.zeros(n, bool)
    cb, ce = max(int(clamp[0]), 0), min(int(clamp[1]), n)
    if cb < ce:
        mask[cb:ce] = True
    return mask


def clamp01(p: np.ndarray) -> np.ndarray:
    """``adam_clamp01``: two comparisons, both false for a NaN."""
    return np.where(p < 0, p.dtype.type(0), np.where(p > 1, p.dtype.type(1), p))


def replay(p, m, v, g, hyper: Hyper, grad_scale: float = 1.0, clamp=(0, 0)):
    """(p', m', v') float32: the kernel's expression on float32 arrays, element i of the arrays being element i of the clamp range."""
    p, m, v, g = (np.asarray(a, F32) for a in (p, m, v, g))
    lr_bc1, sqrt_bc2 = bias(hyper.lr, hyper.b1, hyper.b2, hyper.step)
    b1, b2, eps, gs, one = F32(hyper.b1), F32(hyper.b2), F32(hyper.eps), F32(grad_scale), F32(1.0)
    with np.errstate(all="ignore"):
        gk = g * gs
        m2 = m * b1 + gk * (one - b1)
        v2 = v * b2 + (gk * gk) * (one - b2)
        denom = np.sqrt(v2) / sqrt_bc2 + eps
        p2 = p - lr_bc1 * (m2 / denom)
        inside = _clamp_mask(p2.size, clamp).reshape(p2.shape)
        p2 = np.where(inside, clamp01(p2), p2)
    assert p2.dtype == m2.dtype == v2.dtype == F32
    return p2, m2, v2


def oracle(p, m, v, g, hyper: Hyper, grad_scale: float = 1.0, clamp=(0, 0)):
    """((p', e_p), (m', e_m), (v', e_v)) float64: the update in double from the float32 inputs and float32 hyper-parameters, and the
    envelope of the module docstring beside each.  Elements with a non-finite input or result have a non-finite entry in both."""
    p, m, v, g = (np.asarray(a, F32).astype(np.float64) for a in (p, m, v, g))
    lr_bc1, sqrt_bc2 = (float(x) for x in bias(hyper.lr, hyper.b1, hyper.b2, hyper.step))
    b1, b2, eps, gs = float(F32(hyper.b1)), float(F32(hyper.b2)), float(F32(hyper.eps)), float(F32(grad_scale))
    omb1, omb2 = float(F32(1.0) - F32(hyper.b1)), float(F32(1.0) - F32(hyper.b2))
    assert omb1 == 1.0 - b1 and omb2 == 1.0 - b2, "1 - beta must be exact in float32: betas in [0.5, 1]"
    with np.errstate(all="ignore"):
        gk = g * gs
        e_gk = U * np.abs(gk) + T
        a = m * b1
        e_a = U * np.abs(a) + T
        b = gk * omb1
        e_b = omb1 * e_gk + U * np.abs(b) + T
        m2 = a + b
        e_m = e_a + e_b + U * np.abs(m2) + T
        c = gk * gk
        e_c = 2.0 * np.abs(gk) * e_gk + e_gk * e_gk + U * c + T
        d = c * omb2
        e_d = omb2 * e_c + U * d + T
        f = v * b2
        e_f = U * np.abs(f) + T
        v2 = f + d
        e_v = e_f + e_d + U * np.abs(v2) + T
        s = np.sqrt(v2)
        e_s = np.sqrt(v2 + e_v) - np.sqrt(np.maximum(v2 - e_v, 0.0)) + U2 * s + T
        q = s / sqrt_bc2
        e_q = e_s / sqrt_bc2 + U2 * q + T
        den = q + eps
        e_den = e_q + U * den + T
        finite = np.isfinite(den) & np.isfinite(m2)
        assert bool((den[finite] > e_den[finite]).all()), "denom >= eps keeps the quotient's box off zero"
        r = m2 / den
        e_r = (np.abs(m2) + e_m) / (den - e_den) - np.abs(r) + U2 * np.abs(r) + T
        w = lr_bc1 * r
        e_w = lr_bc1 * e_r + U * np.abs(w) + T
        p2 = p - w
        e_p = e_w + U * np.abs(p2) + T
        inside = _clamp_mask(p2.size, clamp).reshape(p2.shape)
        p2 = np.where(inside, clamp01(p2), p2)
    return (p2, e_p), (m2, e_m), (v2, e_v)


# ------------------------------------------------------------------------------------------------------------------------------ #
# one call: its buffers, what it must update, what it must give
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class Case:
    """One Adam call over whole float32 buffers p, m, v, g (the state BEFORE the call).  ``clamp`` is in elements of these buffers;
    ``touched`` marks the elements the call must update (None: all of them); ``call`` holds the arguments of the launch."""
    name: str
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    g: np.ndarray
    hyper: Hyper
    grad_scale: float = 1.0
    clamp: Tuple[int, int] = (0, 0)
    touched: Optional[np.ndarray] = None
    call: Dict = field(default_factory=dict)
    _replay: Optional[tuple] = None
    _oracle: Optional[tuple] = None

    @property
    def mask(self) -> np.ndarray:
        return np.ones(self.p.size, bool) if self.touched is None else self.touched

    def expected(self):
        """(p', m', v') float32 of the whole buffers: the replay on the touched elements, the old bits elsewhere."""
        if self._replay is None:
            rp, rm, rv = replay(self.p, self.m, self.v, self.g, self.hyper, self.grad_scale, self.clamp)
            t = self.mask
            self._replay = tuple(np.where(t, new, old) for new, old in ((rp, self.p), (rm, self.m), (rv, self.v)))
        return self._replay

    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle(self.p, self.m, self.v, self.g, self.hyper, self.grad_scale, self.clamp)
        return self._oracle


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, F32).view(np.int32)


def _ordered(a: np.ndarray) -> np.ndarray:
    """float32 bits as integers that grow with the value: the difference of two is their distance in ulps."""
    b = _bits(a).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _host(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    assert a.dtype == F32, a.dtype
    return a.reshape(-1)


def check(got_p, got_m, got_v, case: Case, report: Optional[Dict] = None, p_bits: bool = True) -> List[str]:
    """The rules of the module docstring on the whole buffers after the call (numpy or torch, any device) -> the list of failures.
    report[case.name] = the worst |got - oracle| / envelope of p, m, v, the number of touched elements whose bits differ from the
    replay's, the largest such distance of p in ulps, the number of untouched elements that changed.  p_bits=False: a p that differs
    from the replay in bits is reported, not failed (the envelope holds it)."""
    got = {"p": _host(got_p), "m": _host(got_m), "v": _host(got_v)}
    want = dict(zip("pmv", case.expected()))
    old = {"p": case.p, "m": case.m, "v": case.v}
    orc = dict(zip("pmv", case.oracle()))
    t = case.mask
    fails, rep = [], {"n": int(t.sum())}
    for k in "pmv":
        a, w = got[k], want[k]
        if a.shape != w.shape:
            fails.append(f"{case.name}: {k} has {a.size} elements, not {w.size}")
            continue
        # what the call must not touch
        stray = ~t & (_bits(a) != _bits(old[k]))
        rep[f"{k}_untouched_changed"] = int(stray.sum())
        if stray.any():
            i = int(stray.nonzero()[0][0])
            fails.append(f"{case.name}: {k}: {int(stray.sum())} elements outside the call changed, first {i}: {a[i]!r}, was {old[k][i]!r}")
        # NaN / Inf where the replay has them
        for what, fa, fw in (("NaN", np.isnan(a), np.isnan(w)), ("+Inf", a == np.inf, w == np.inf), ("-Inf", a == -np.inf, w == -np.inf)):
            bad = t & (fa != fw)
            if bad.any():
                i = int(bad.nonzero()[0][0])
                fails.append(f"{case.name}: {k}: {what} at {int(bad.sum())} other elements than the replay's, first {i}: {a[i]!r} vs {w[i]!r}")
        fin = t & np.isfinite(w) & np.isfinite(a)
        # bits of the replay
        differ = fin & (_bits(a) != _bits(w))
        rep[f"{k}_bits_differ"] = int(differ.sum())
        ulps = np.abs(_ordered(a) - _ordered(w))[differ]
        rep[f"{k}_max_ulp"] = int(ulps.max()) if ulps.size else 0
        if differ.any() and (k != "p" or p_bits):
            i = int(differ.nonzero()[0][0])
            fails.append(f"{case.name}: {k}: {int(differ.sum())} of {int(fin.sum())} elements differ from the replay in bits (up to "
                         f"{rep[f'{k}_max_ulp']} ulp), first {i}: {a[i]!r} vs {w[i]!r}")
        # the float64 envelope
        ref, env = orc[k]
        fin &= np.isfinite(ref) & np.isfinite(env)
        with np.errstate(all="ignore"):
            d = np.abs(a.astype(np.float64) - ref)
            ratio = np.where(fin, d / env, 0.0)
        rep[f"{k}_worst"] = float(ratio.max()) if ratio.size else 0.0
        over = ratio > 1.0
        if over.any():
            i = int(ratio.argmax())
            fails.append(f"{case.name}: {k}: {int(over.sum())} of {int(fin.sum())} elements outside the float64 envelope, worst {i}: {a[i]!r} vs "
                         f"{ref[i]!r} +- {env[i]:.3g} (x {ratio[i]:.3g})")
    if report is not None:
        report[case.name] = rep
    return fails


# ------------------------------------------------------------------------------------------------------------------------------ #
# elements and cases
# ------------------------------------------------------------------------------------------------------------------------------ #
def _log_uniform(rng, n, lo, hi, signed=True):
    x = 10.0 ** rng.uniform(lo, hi, n)
    return (x * rng.choice((-1.0, 1.0), n) if signed else x).astype(F32)


def elements(n: int, seed: int, moments: str = "alive"):
    """(p, m, v, g) float32 [n], no zero among them: p in (-2, 2); g log-uniform 1e-30 .. 1e18, both signs; moments "alive" (m
    log-uniform 1e-30 .. 1e10 of both signs, v log-uniform 1e-44 -- subnormal -- .. 1e20) or "zero" (m = v = 0: a first step)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-2.0, 2.0, n).astype(F32)
    p[p == 0] = F32(0.5)
    g = _log_uniform(rng, n, -30, 18)
    if moments == "zero":
        return p, np.zeros(n, F32), np.zeros(n, F32), g
    m, v = _log_uniform(rng, n, -30, 10), _log_uniform(rng, n, -44, 20, signed=False)
    v[v == 0] = F32(T)
    return p, m, v, g


def plant_specials(p, m, v, g, where: np.ndarray, seed: int) -> None:
    """Overwrites some of the elements ``where`` (indices the call updates), when there are at least 64 of them: g = +0 / -0 with the
    moments alive, g = m = v = 0, g = NaN / +Inf / -Inf, the smallest subnormal v and v = 1e20 beside a zero and a tiny gradient."""
    if where.size < 64:
        return
    rng = np.random.default_rng(seed + 1)
    pick = rng.permutation(where)[: 16 * max(1, min(where.size // 64, 8))].reshape(16, -1)
    alive_m = np.where(m[pick[0]] == 0, F32(1e-3), m[pick[0]])
    for rows, gv in ((pick[0], 0.0), (pick[1], -0.0)):
        g[rows] = F32(gv)
        m[rows], v[rows] = alive_m[: rows.size], F32(1e-6)
    g[pick[2]], m[pick[2]], v[pick[2]] = F32(0.0), F32(0.0), F32(0.0)
    g[pick[3]], m[pick[3]], v[pick[3]] = F32(-0.0), F32(0.0), F32(0.0)
    g[pick[4]], g[pick[5]], g[pick[6]] = F32(np.nan), F32(np.inf), F32(-np.inf)
    v[pick[7]], g[pick[7]] = F32(T), F32(0.0)
    v[pick[8]], g[pick[8]] = F32(T), F32(1e-30)
    v[pick[9]], g[pick[9]] = F32(1e20), F32(1e18)
    v[pick[10]], g[pick[10]] = F32(1e20), F32(-1e-30)
    m[pick[11]], v[pick[11]] = F32(-1e10), F32(T)  # the largest |m / denom|
    g[pick[12]] = F32(1e18)
    g[pick[13]] = F32(-1e-30)


def plant_clamp_elements(p, m, v, g, clamp, where_ok: np.ndarray, hyper: Hyper, grad_scale: float) -> None:
    """Around both ends of the clamp range -- two elements outside, the rest inside, as far as ``where_ok`` (bool: the call updates the
    element) allows -- p three tenths of its own step away from 0 or 1, by the element's distance d from the end of the range:
      d % 4 = 0  just above 0, moves below it     1  just below 0, moves above it
              2  just above 1, moves below it     3  just below 1, moves above it
    so the last element outside and the first inside each end (d = -1, 0) leave [0, 1] and show whether they were clamped."""
    cb, ce = clamp
    if ce <= cb:
        return
    spots = {i: i - cb for i in range(cb - 2, cb + 6) if 2 * i < cb + ce}  # (a short range: each end keeps its own half)
    spots.update({i: i - ce for i in range(ce - 6, ce + 2) if 2 * i >= cb + ce})
    spots = {i: d % 4 for i, d in spots.items() if 0 <= i < p.size and where_ok[i]}
    if not spots:
        return
    at, kind = np.array(list(spots)), np.array(list(spots.values()))
    sign = np.where((kind == 0) | (kind == 2), 1.0, -1.0)  # of the gradient: the parameter moves the other way
    g[at] = (sign * 1e-3 / grad_scale).astype(F32)
    alive = (m[at] != 0) | (v[at] != 0)  # moments alive: in step with the gradient
    m[at], v[at] = np.where(alive, sign * 1e-3, 0.0).astype(F32), np.where(alive, 1e-6, 0.0).astype(F32)
    move = replay(np.zeros(at.size, F32), m[at], v[at], g[at], hyper, grad_scale)[0].astype(np.float64)
    assert bool((np.sign(move) == -sign).all())
    p[at] = (np.where(kind < 2, 0.0, 1.0) - 0.3 * move).astype(F32)


def _hyper(k: int) -> Tuple[Hyper, float, str]:
    """The k-th combination of step, grad_scale, eps and moments: the step cycles fastest; betas (0.9, 0.99) now and then."""
    step = STEPS[k % len(STEPS)]
    betas = (0.9, 0.99) if k % 5 == 3 else (0.9, 0.999)
    moments = "zero" if (step == 1 or k % 7 == 4) else "alive"
    return Hyper(exp_decay_lr(step - 1), betas[0], betas[1], EPSS[(k // 2) % 2], step), SCALES[k % 3], moments


def _build(name, n, touched, clamp, k, call) -> Case:
    hyper, gs, moments = _hyper(k)
    seed = 1000 + 17 * k + n % 1000
    p, m, v, g = elements(n, seed, moments)
    if moments == "zero":  # what the call does not touch still holds non-zero values
        _, m_alive, v_alive, _ = elements(n, seed + 5, "alive")
        m, v = np.where(touched, m, m_alive), np.where(touched, v, v_alive)
    idx = touched.nonzero()[0]
    plant_specials(p, m, v, g, idx, seed)
    plant_clamp_elements(p, m, v, g, clamp, touched, hyper, gs)
    if clamp[1] - clamp[0] >= 5 and touched[clamp[0] + 2]:
        g[clamp[0] + 2] = F32(np.nan)  # a non-finite gradient inside the clamp range: the clamp must keep the NaN
    return Case(name, p, m, v, g, hyper, gs, clamp, touched, call)


DENSE_N = (1, 3, 4, 5, 1023, 1025, 262147, 2048 * 256 * 4 + 7)


def _dense_clamps(n: int) -> Dict[str, Tuple[int, int]]:
    """Clamp ranges relative to the call's slice.  tail: from inside the last whole float4 to the end, over the scalar tail; straddle:
    five elements across a float4 boundary in the middle; empty."""
    tail_begin = n - n % 4 - 3
    out = {"tail": (tail_begin if tail_begin >= 1 else min(1, n - 1), n), "empty": (n // 3, n // 3)}
    if n >= 8:
        cb = 4 * (n // 8) + 2
        out["straddle"] = (cb, cb + 5)
    return out


def _rows(n_rows: int, seed: int) -> np.ndarray:
    """Unique unordered rows of the 4096-row buffer, row 0 and the last row among them (one row: the last)."""
    if n_rows < 2:
        return np.array([N_ROWS_BUFFER - 1][:n_rows], np.int64)
    rng = np.random.default_rng(seed)
    others = rng.permutation(np.arange(1, N_ROWS_BUFFER - 1))[: n_rows - 2]
    return rng.permutation(np.concatenate([others, [N_ROWS_BUFFER - 1, 0]])).astype(np.int64)


def _row_mask(n: int, rows: np.ndarray) -> np.ndarray:
    t = np.zeros(n, bool)
    t[2 * rows], t[2 * rows + 1] = True, True
    return t


def _specs() -> Dict[str, tuple]:
    specs, k = {}, 0
    for n in DENSE_N:
        for cname, clamp in _dense_clamps(n).items():
            specs[f"dense/{n}/{cname}"] = ("dense", n, clamp, k)
            k += 1
    for n_rows in (1, 255, 256, 257):
        specs[f"rows/{n_rows}"] = ("rows", n_rows, (0, 0), k)
        k += 1
    for n_rows, count, clamps in ((0, 5, ("across",)), (257, 0, ("inside",)), (1, 1, ("across",)), (257, 255, ("inside",)),
                                  (300, 256 * 1024 + 5, ("inside", "across"))):
        for cname in clamps:
            clamp = (RANGE_BEGIN + count // 2 - 1, RANGE_BEGIN + count // 2 + 4) if cname == "inside" else (RANGE_BEGIN - 3, RANGE_BEGIN + max(count // 3, 1))
            specs[f"rows_range/{n_rows}+{count}/{cname}"] = ("rows_range", (n_rows, count), clamp, k)
            k += 1
    return specs


SPECS = _specs()
CASES = tuple(SPECS)
_cases: Dict[str, Case] = {}


def case(name: str) -> Case:
    """The named case, built once per process.  ``call``: dense -- begin, n, clamp (relative to the slice); rows -- rows; rows_range --
    rows, begin, end, clamp (absolute)."""
    if name not in _cases:
        kind, shape, clamp, k = SPECS[name]
        if kind == "dense":
            n = shape
            total = LEAD + n + TRAIL
            touched = np.zeros(total, bool)
            touched[LEAD:LEAD + n] = True
            c = _build(name, total, touched, (LEAD + clamp[0], LEAD + clamp[1]), k, dict(begin=LEAD, n=n, clamp=clamp))
        elif kind == "rows":
            rows = _rows(shape, 40 + shape)
            c = _build(name, 2 * N_ROWS_BUFFER, _row_mask(2 * N_ROWS_BUFFER, rows), (0, 0), k, dict(rows=rows))
        else:
            n_rows, count = shape
            rows = _rows(n_rows, 50 + n_rows)
            total = RANGE_BEGIN + count + TRAIL
            touched = _row_mask(total, rows)
            touched[RANGE_BEGIN:RANGE_BEGIN + count] = True
            c = _build(name, total, touched, clamp, k, dict(rows=rows, begin=RANGE_BEGIN, end=RANGE_BEGIN + count, clamp=clamp))
        _cases[name] = c
    return _cases[name]


# ------------------------------------------------------------------------------------------------------------------------------ #
# UMHSAdam.step's partitions of the flat buffer (tests/test_adam_partition_cpu.py; on the GPU tests/test_hip_adam_f64.py)
# ------------------------------------------------------------------------------------------------------------------------------ #
# A flat parameter of 715 floats: four "levels" of 64 rows x 2 -- levels 0-1 sparse ([0, 256): only the live rows ever see a gradient),
# levels 2-3 dense ([256, 512)) -- and a tail of 203 floats.
PART_N, PART_SPARSE_END, PART_DENSE_END = 715, 256, 512
PART_CLAMPS = ((600, 650), (380, 390), (0, 0))  # inside one piece; across the piece boundary at 384; none
PART_LR, PART_LR_FINAL, PART_MAX_STEPS, PART_STEP0 = 2e-2, 1e-3, 10, 4  # the learning rate changes from step to step; 4 steps were taken
# sparse: the parameter carries _umhs_live_rows; sink: it carries a gradient sink; done: the elements a backward has updated already
# (adam_done); segments: what the sink's reduced_segments yields; world: the number of ranks umhsnerf.optim.world reports
PART_SCENARIOS = {
    "a": dict(sparse=False, sink=False, done=None, segments=(), world=1),
    "b": dict(sparse=True, sink=False, done=None, segments=(), world=1),
    "c": dict(sparse=True, sink=True, done=(256, 512), segments=(), world=1),
    "d": dict(sparse=True, sink=True, done=(256, 715), segments=(), world=1),
    "e": dict(sparse=False, sink=True, done=(128, 384), segments=(), world=1),
    "g": dict(sparse=True, sink=True, done=None, segments=((512, 715), (0, 384), (384, 512)), world=2),
}


def partition_rows() -> np.ndarray:
    """40 unique unordered live rows (of 2 floats) of the sparse levels, the first and the last row among them."""
    rng = np.random.default_rng(715)
    others = rng.permutation(np.arange(1, PART_SPARSE_END // 2 - 1))[:38]
    return rng.permutation(np.concatenate([others, [0, PART_SPARSE_END // 2 - 1]])).astype(np.int64)


def partition_live() -> np.ndarray:
    """bool [715]: the elements an optimizer step updates when the sparse rows are in force."""
    live = _row_mask(PART_N, partition_rows())
    live[PART_SPARSE_END:] = True
    return live


def partition_state(seed: int = 0):
    """(p, m, v, g) float32 [715], moments alive; the rows of the sparse levels that are not live have g = m = v = 0, as in the model."""
    p, m, v, g = elements(PART_N, 7150 + seed)
    g = np.clip(g, -1e6, 1e6)  # (bounded: every value stays finite over consecutive steps)
    m, v = np.clip(m, -1e3, 1e3), np.clip(v, 1e-12, None)
    dead = ~partition_live()
    m[dead], v[dead], g[dead] = 0.0, 0.0, 0.0
    return p, m, v, g


class FakeSink:
    """What UMHSAdam.step reads of a parameter's gradient sink, and nothing else."""

    def __init__(self, segments=()):
        self.fused_adam, self.adam_done, self.sparse_levels, self.segments = None, None, 2, tuple(segments)

    def reduced_segments(self, grad):
        yield from self.segments


def partition_hyper(step: int) -> Hyper:
    return Hyper(exp_decay_lr(step - 1, PART_LR, PART_LR_FINAL, PART_MAX_STEPS), 0.9, 0.999, 1e-15, step)


def partition_steps(name: str, clamp, device: str, fused_update, n_steps: int = 2, wrong_step: bool = False):
    """Drives ``UMHSAdam.step`` through scenario ``name`` for ``n_steps`` consecutive steps; ``umhsnerf.optim.world`` (and, on the CPU,
    ``umhsnerf.optim.ops``) are the caller's to patch.  ``fused_update(p, g, m, v, hyper, (a, b), clamp)`` plays the backward that
    updates elements [a, b) of the torch buffers itself.  Yields, after every step, (the Case of the whole buffer before the step, p,
    m, v after it)."""
    import torch

    from umhsnerf.optim import UMHSAdam

    sc = PART_SCENARIOS[name]
    p0, m0, v0, _ = partition_state()
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(device))
    if sc["sparse"]:
        param._umhs_live_rows = (torch.from_numpy(partition_rows()).to(device), PART_SPARSE_END)
    sink = FakeSink(sc["segments"]) if sc["sink"] else None
    if sink is not None:
        param._umhs_grad_sink = sink
    opt = UMHSAdam([param], lr=PART_LR, clamp_range=clamp, lr_final=PART_LR_FINAL, max_steps=PART_MAX_STEPS)
    st = opt.state[param]
    st["step"], st["exp_avg"], st["exp_avg_sq"] = PART_STEP0, torch.from_numpy(m0.copy()).to(device), torch.from_numpy(v0.copy()).to(device)
    for k in range(n_steps):
        step = PART_STEP0 + k + 1
        hyper = partition_hyper(step)
        g = partition_state(seed=k)[3]
        param.grad = torch.from_numpy(g.copy()).to(device)
        before = Case(f"step/{name}/{clamp[0]}-{clamp[1]}/step{step}", param.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy(),
                      st["exp_avg_sq"].cpu().numpy().copy(), g, hyper, 1.0 / sc["world"], tuple(clamp))
        if sc["done"] is not None:
            fused_update(param.data, param.grad, st["exp_avg"], st["exp_avg_sq"], hyper, sc["done"], tuple(clamp))
            sink.adam_done = (step + 1 if wrong_step else step, *sc["done"])
        opt.step()
        assert st["step"] == step and (sink is None or (sink.adam_done is None and sink.fused_adam is None))
        yield before, param.data, st["exp_avg"], st["exp_avg_sq"]
