"""Occupancy-grid sampler cases, their float64 oracles and the per-sample comparators (plain helper module, no tests in it).

Used by tests/test_hip_sampler_f64.py (csrc/umhs_sampler.hip on the GPU, every host path of umhsnerf/sampler.py) and
tests/test_sampler_f64_bounds_cpu.py (the comparators pass the float32 restatement and reject planted faults; K, the caps and the teeth
are measured and held there).  It mirrors tests/rays_f64.py one stage earlier.

MARCHER ORACLE (``march_ray64``).  The algorithm of oracle/torch_ref.py::march_ray_ref in real arithmetic: Python floats (float64), true
divisions, the inputs being the float32 values as given (roi, planes, step and cone are rounded to float32 first, as the C ABI does).
The 1e-5 max(1, |t|) look-ahead, the "mid-point < clipped exit" rule and the one-float32-ulp step where a voxel's exit is not behind
its entry are part of the definition.  Per ray: near = nears[r] + jitter[r] jitter_step, far = fars[r].  Besides the samples it returns,
per sample, the conditioning of its run's entry and its index within the run, and per ray its TIE EVENTS -- places where a float32
evaluation may legitimately decide otherwise.  With u = 2^-24 and every margin K_TIE u x (the sum of the absolute values of the terms
that are rounded on the way, the same construction as EDGE x envelope in rays_f64.py):
  mag_t of a chain value   (|c| + h 2^l + |face| + |o|) |1/d| on the exit axis + |t|;  |near| + |nears| + |jitter jitter_step| at a near plane
  face         a look-ahead coordinate x = (p - vmin) / vs within  (u_p + u (|p| + |c| + h 2^l)) / vs + 3 u |x|  of an interior integer,
               u_p = u (|o| + |d tm| + |d| mag_t)
  level        |p - c| / h on an axis that can be the maximum within the same margin (over h) of a level boundary 2^k, k < levels
  creep        the exit is not behind the entry by more than the two margins (the nextafter fix-up, a sliver voxel)
  end          the first |t - t_end|, or a later |t_exit - t_end| where t_end is the far plane (at the box's own far side the two are
               the same face by construction, and leaving the grid is the level event), within mag_t(t_exit) + mag_t(t_end)
  mid-point    |mid - clipped exit| within mag_run + (k + 1) |mid| + mag_t(exit) at the END of a run (inside a run the sample is
               emitted from the next voxel instead: same samples).  An equality that is exact, on a chain whose every float32
               operation is exact (dyadic step, axis-aligned ray, far plane an input), is NOT a tie: float32 computes the very same
               numbers and the strict "<" decides -- that is what planted fault 7 is caught by.

ONE RULE per output element.  DECIDED rays (no tie event): exactly the oracle's count, and for sample i, the k-th of its run,
  |t_starts[i] - ref64| <= K u (mag_run + (k + 1) |t|),     |t_ends[i] - ref64| <= K u (mag_run + (k + 2) |t|)
(the entry's conditioning plus one rounding per term of the recurrence t += max(t cone, step)).  ray_indices and packed_info are exact
for every ray: packed_info is (exclusive prefix, count), ray_indices its expansion.  UNDECIDED rays: the count is within the ray's
number of tie events of the oracle's (the ray lying in a face plane has an event at every voxel, each worth a voxel's samples: it
holds in the committed cases, 40 against 58 in "fine", but not by nature); t_starts strictly increase, every t_end - t_start is max(t_start cone, step) to 4 u |t|; every
mid-point, in float64, lies in an occupied cell of its own level or a coarser one, or within the margins (3e-5 max(1, t) along the
ray, 64 u of the coordinates across it) of one.
CAP: at most 10 % of a case's rays undecided.  Measured (K_TIE = 1: the margins are sums of unit roundings already): cube 8.9 % |
box 8.1 % | deep 6.2 % | fine 1.9 % | one_cell 0.4 % | planes 6.2 % | wide_cone 9.3 % | full 2.7 % | empty 5.0 % | sparse 8.1 %.  Most of
them are face events of rays with a direction component below ~0.03: the look-ahead moves the point 1e-5 |d_k| t past the face it
has just crossed, the float32 error of that coordinate is ~16 u of the scene's size.  (The 16 rays scaled by 0.004 rarely cross a face
of their slow axis at all; where they do, they creep and are flagged.)  On 2,591 rays the float32 restatement's count differs from the
oracle's on 6, every one of them flagged.
TEETH: in every non-empty case at least 90 % of the rays are decided, with at least 50 samples per decided ray on average.
K per family = max(8, 4 x the float32 restatement's worst ratio over the committed cases, rounded up to a power of two).  Measured on
the CPU (march_ray_ref per ray with that ray's planes, tests/test_sampler_f64_bounds_cpu.py re-measures and asserts 4 x worst <= K):
  t_starts 1.70 | t_ends 1.66   ->   K = 8 for both.
tests/test_hip_sampler_f64.py writes the kernels' own worst ratios per case, path and output and the undecided shares to
sampler_f64.json in ``report_dir()``, next to rays_f64.json.

VISIBILITY ORACLE.  x = sigma (t1 - t0), X the exclusive optical depth, T = exp(-X), alpha = 1 - exp(-x) in float64 from the float32
inputs (x itself is the float32 product's real value; its rounding is inside the margins).  An element is decided unless
(eps > 0 and) |T - eps| <= K_VIS u T (1 + X)  or (thre > 0 and) |alpha - thre| <= K_VIS u -- with eps = 0 every T passes in any
arithmetic, an underflowed one too; decided elements of the mask match exactly; kept[r] is
the row sum of the mask the kernel itself wrote.  At most 1 % of a case may be undecided: ``make_vis_case`` moves sigma away from
every threshold of VIS_PAIRS by 10 x the margin (measured: 0 % undecided).  K_VIS = max(8, 4 x worst) = 8: the float32 restatement's T is 1.94 u T (1 + X)
from float64 (a 1000-term running sum), its alpha 1.05 u.

Marcher cases (259 rays each; which path each one is there for):
  cube       roi [-1, 1]^3, 3 levels, res 16, cone 0.004: the shape of tests/test_hip_sampler.py
  box        roi [-0.7, -1.1, -0.4, 1.3, 0.9, 0.8], 3 levels, res 12, cone 0: a half extent per axis, centre != 0, inexact voxel size
  deep       that roi, 8 levels, res 6, cone 0.01: every level of march_segment_start live; level boxes cut coarser voxels (6 % 4 != 0)
  fine       1 level, res 33, step 0.005: more than 64 voxels per ray -> several windows of the wave walk
  one_cell   1 level, res 1: the index clamp
  planes     box with per-ray nears in [0, 0.5], fars in [0.3, 8], jitter in [0, 1), jitter_step = step: far < near, a near plane behind
             the far side of the box, near planes inside occupied voxels
  wide_cone  cone 0.05: dt grows past a voxel width, samples span several voxels (and overlap the next run)
  full       every cell occupied, 2 levels, res 16, step 2^-5, far 2.265625 = a mid-point of the two dyadic axis-aligned rays: one
             continuous run per ray across every lane and window; the exact tie of fault 7
  empty      no cell occupied: n = 0 through every host path
  sparse     3 % occupancy at res 32, step 0.00075: runs of one voxel with long gaps
  cube_R1, cube_R0: the first ray of cube alone, and no ray at all
Rays of every case: cameras outside and inside the roi, 6 rays pointing away (they miss the box), 16 rays with one direction
component scaled by 0.004 (they creep; mostly undecided -- the cap's headroom is for them), a ray lying in a voxel-face plane, two
axis-aligned rays with +0.0 and -0.0 components; R = 259 is a multiple of neither 4 nor 64."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from rays_f64 import report_dir  # noqa: F401  (the GPU test's report goes next to rays_f64.json)

U = 2.0 ** -24
K_TIE = 1.0
K_STARTS = K_ENDS = 8.0
K_VIS = 8.0
BIG = float(np.float32(1e30))
F32 = np.float32
BOX = [-0.7, -1.1, -0.4, 1.3, 0.9, 0.8]
CUBE = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
N_RAYS = 259

# name -> grid, planes and occupancy (occ: share of occupied cells; 1 / 0: all / none)
MARCH_SPECS = {
    "cube": dict(roi=CUBE, levels=3, res=16, cone=0.004, step=0.01, occ=0.3),
    "box": dict(roi=BOX, levels=3, res=12, cone=0.0, step=0.01, occ=0.3),
    "deep": dict(roi=BOX, levels=8, res=6, cone=0.01, step=0.004, occ=0.4, far=60.0),
    "fine": dict(roi=CUBE, levels=1, res=33, cone=0.0, step=0.005, occ=0.3),
    "one_cell": dict(roi=CUBE, levels=1, res=1, cone=0.0, step=0.01, occ=1.0),
    "planes": dict(roi=BOX, levels=3, res=12, cone=0.0, step=0.008, occ=0.4, planes=True),
    "wide_cone": dict(roi=CUBE, levels=4, res=16, cone=0.05, step=0.002, occ=0.7),
    "full": dict(roi=CUBE, levels=2, res=16, cone=0.0, step=0.03125, occ=1.0, far=2.265625, dyadic=True),
    "empty": dict(roi=CUBE, levels=2, res=16, cone=0.004, step=0.01, occ=0.0),
    "sparse": dict(roi=CUBE, levels=1, res=32, cone=0.0, step=0.00075, occ=0.03),
    "cube_R1": dict(roi=CUBE, levels=3, res=16, cone=0.004, step=0.01, occ=0.3, like="cube", rays=1),
    "cube_R0": dict(roi=CUBE, levels=3, res=16, cone=0.004, step=0.01, occ=0.3, like="cube", rays=0),
}
MARCH_CASES = list(MARCH_SPECS)
NONEMPTY = [n for n in MARCH_CASES if n not in ("empty", "cube_R0")]


def _f32(x) -> float:
    return float(np.float32(x))


def _is32(x: float) -> bool:
    return float(np.float32(x)) == x


@dataclass
class MarchCase:
    name: str
    roi: List[float]
    levels: int
    res: int
    near: float
    far: float
    step: float
    cone: float
    binaries: np.ndarray  # bool [levels, res, res, res]
    o: torch.Tensor  # [R,3] float32
    d: torch.Tensor
    nears: Optional[torch.Tensor] = None
    fars: Optional[torch.Tensor] = None
    jitter: Optional[torch.Tensor] = None
    jitter_step: float = 0.0

    @property
    def R(self) -> int:
        return self.o.shape[0]

    def planes(self, r: int):
        """(near, far) of ray r as the kernel forms them, in float32 (what march_ray_ref is called with)."""
        near = F32(self.near) if self.nears is None else self.nears[r].numpy()
        if self.jitter is not None:
            near = F32(near + self.jitter[r].numpy() * F32(self.jitter_step))
        return F32(near), (F32(self.far) if self.fars is None else F32(self.fars[r].numpy()))

    def march_kwargs(self, dev) -> Dict:
        kw = {}
        if self.nears is not None:
            kw.update(nears=self.nears.to(dev), fars=self.fars.to(dev))
        if self.jitter is not None:
            kw.update(jitter=self.jitter.to(dev), jitter_step=self.jitter_step)
        return kw


def make_march_case(name: str, seed: int = 0) -> MarchCase:
    sp = MARCH_SPECS[name]
    seed = MARCH_CASES.index(sp.get("like", name)) + 100 * seed
    rng = np.random.default_rng(4100 + seed)
    g = torch.Generator().manual_seed(4200 + seed)
    levels, res = sp["levels"], sp["res"]
    binaries = rng.random((levels, res, res, res)) < sp["occ"]
    a = np.asarray(sp["roi"], np.float32).reshape(2, 3).astype(np.float64)
    c, h = torch.tensor((a[0] + a[1]) / 2).float(), torch.tensor((a[1] - a[0]) / 2).float()
    s = float(h.max())
    R = N_RAYS
    u = torch.randn(R, 3, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    o = c + 2.5 * s * u + (torch.rand(R, 3, generator=g) - 0.5) * s
    d = (c - o) + torch.randn(R, 3, generator=g) * 0.4 * s
    k = 36
    o[:k] = c + (torch.rand(k, 3, generator=g) * 2 - 1) * 0.9 * h  # cameras inside the roi
    d[:k] = torch.randn(k, 3, generator=g)
    d[100:106] = o[100:106] - c  # pointing away: they miss the box
    d = d / d.norm(dim=-1, keepdim=True)
    for i in range(106, 122):  # almost parallel to a grid axis: the walk creeps ulp by ulp at the faces of that axis
        d[i, i % 3] *= 0.004
        d[i] = d[i] / d[i].norm()
    i_face = res // 2 + (1 if res > 1 else 0)
    x_face = F32(F32(c[0].numpy() - h[0].numpy()) + F32(i_face) * F32(F32(h[0].numpy() * F32(2)) / F32(res)))
    o[122] = torch.tensor([float(x_face), float(c[1]) - 1.5 * s, float(c[2]) - 2.0 * s])  # lies in a voxel-face plane
    d[122] = torch.tensor([0.0, 0.6, 0.8])
    if sp.get("dyadic"):  # every float32 operation of these two rays' chains is exact
        o[-1], d[-1] = torch.tensor([-3.0, 0.1875, -0.3125]), torch.tensor([1.0, 0.0, -0.0])
        o[-2], d[-2] = torch.tensor([0.3125, 3.0, 0.4375]), torch.tensor([-0.0, -1.0, 0.0])
    else:
        o[-1], d[-1] = c + torch.tensor([-3.0 * s, 0.13 * s, -0.27 * s]), torch.tensor([1.0, 0.0, -0.0])
        o[-2], d[-2] = c + torch.tensor([0.31 * s, 5.0 * s, 0.2 * s]), torch.tensor([-0.0, -1.0, 0.0])
    case = MarchCase(name, [_f32(v) for v in sp["roi"]], levels, res, _f32(0.05), _f32(sp.get("far", 1e3)), _f32(sp["step"]),
                     _f32(sp["cone"]), binaries, o.contiguous(), d.contiguous())
    if sp.get("planes"):
        case.nears = torch.rand(R, generator=g) * 0.5
        case.fars = 0.3 + torch.rand(R, generator=g) * 7.7
        case.jitter = torch.rand(R, generator=g)
        case.jitter_step = case.step
        case.nears[0], case.fars[0] = 0.5, 0.3  # far < near
        case.nears[50], case.fars[50] = 7.9, 8.0  # the near plane lies behind the far side of the box
    n = sp.get("rays", R)
    if n != R:
        case.o, case.d = case.o[:n].contiguous(), case.d[:n].contiguous()
    return case


# ------------------------------------------------------------------------------------------------------------------------------ #
# the float64 marcher
# ------------------------------------------------------------------------------------------------------------------------------ #
def _tie(out: Dict, kind: str) -> None:
    out["ties"] += 1
    out["kinds"][kind] = out["kinds"].get(kind, 0) + 1


def march_ray64(o, d, binaries, roi, near, near_mag, far, step, cone, near_exact=True):
    """One ray in Python floats.  -> dict(ts, te, mag (conditioning of the run's entry), k (index in run), ties)."""
    levels, res = binaries.shape[0], binaries.shape[1]
    c = [(roi[q] + roi[q + 3]) / 2 for q in range(3)]
    h = [(roi[q + 3] - roi[q]) / 2 for q in range(3)]
    inv = [1.0 / d[q] if d[q] != 0 else (-BIG if math.copysign(1.0, d[q]) < 0 else BIG) for q in range(3)]
    top = 2.0 ** (levels - 1)
    tn, tf, mag_n, mag_f, tn_exact = -math.inf, math.inf, 0.0, 0.0, True
    for q in range(3):
        ho = h[q] * top
        ta, tb = (c[q] - ho - o[q]) * inv[q], (c[q] + ho - o[q]) * inv[q]
        mg = (abs(c[q]) + ho + abs(o[q])) * abs(inv[q]) if d[q] != 0 else 0.0
        lo, hi = min(ta, tb), max(ta, tb)
        if lo > tn:
            fc = c[q] - ho if ta < tb else c[q] + ho
            tn, mag_n, tn_exact = lo, mg + abs(lo), _is32(c[q]) and _is32(fc) and _is32(fc - o[q]) and _is32(inv[q]) and _is32(lo)
        if hi < tf:
            tf, mag_f = hi, mg + abs(hi)
    t, mag_t, t_exact = (tn, mag_n, tn_exact) if tn >= near else (near, near_mag, near_exact)
    t_end, mag_end, end_exact = (tf, mag_f, False) if tf <= far else (far, abs(far), True)
    out = {"ts": [], "te": [], "mag": [], "k": [], "ties": 0, "kinds": {}}
    if abs(t - t_end) <= K_TIE * U * (mag_t + mag_end):
        _tie(out, "end")
    if not t < t_end:
        return out
    cont, t_last, mag_run, k, run_exact, pending = False, t, mag_t, 0, t_exact, False
    guard = 0
    while t < t_end and guard < 100000:
        guard += 1
        tm = t + 1e-5 * max(1.0, abs(t))
        p = [o[q] + d[q] * tm for q in range(3)]
        up = [U * (abs(o[q]) + abs(d[q] * tm) + abs(d[q]) * mag_t) for q in range(3)]
        qn = [abs(p[q] - c[q]) / h[q] for q in range(3)]
        qe = [(up[q] + U * (abs(p[q]) + abs(c[q]))) / h[q] + 2 * U * qn[q] for q in range(3)]
        m = max(qn)
        for q in range(3):  # a level boundary (the outermost one ends the walk) on an axis that can be the maximum
            if qn[q] + K_TIE * qe[q] >= m and qn[q] > 0.5:
                b = 2.0 ** round(math.log2(qn[q]))
                if b <= top and abs(qn[q] - b) <= K_TIE * qe[q]:
                    _tie(out, "level")
        if not m < top:
            break
        lvl = 0 if m < 1.0 else min(max(math.frexp(m)[1], 0), levels - 1)
        sc = 2.0 ** lvl
        t_exit, mag_exit, exit_exact = BIG, 0.0, False
        idx = [0, 0, 0]
        for q in range(3):
            hl = h[q] * sc
            vmin, vs = c[q] - hl, hl * 2.0 / res
            x = (p[q] - vmin) / vs
            i = min(max(math.floor(x), 0), res - 1)
            idx[q] = i
            n_int = round(x)
            if 1 <= n_int <= res - 1 and abs(x - n_int) <= K_TIE * ((up[q] + U * (abs(p[q]) + abs(c[q]) + hl)) / vs + 3 * U * abs(x)):
                _tie(out, "face")
            if d[q] != 0:
                j = i + 1 if d[q] >= 0 else i
                face = vmin + j * vs
                tx = (face - o[q]) * inv[q]
                if tx < t_exit:
                    t_exit = tx
                    mag_exit = (abs(c[q]) + hl + abs(face) + abs(o[q])) * abs(inv[q]) + abs(tx)
                    exit_exact = (_is32(vmin) and _is32(vs) and _is32(j * vs) and _is32(face) and _is32(face - o[q]) and _is32(inv[q])
                                  and _is32(tx))
        if t_exit - t <= K_TIE * U * (mag_exit + mag_t):  # creeping / sliver voxel: float32 may take the nextafter step, or not
            _tie(out, "creep")
        if not t_exit > t:
            t_exit, exit_exact = t + float(np.spacing(np.float32(abs(t)))), False
            mag_exit = mag_t
        if end_exact and abs(t_exit - t_end) <= K_TIE * U * (mag_exit + mag_end):  # (t_end the far plane; at the box it IS a face)
            out["ties"] += 1
        t_clip, mag_clip, clip_exact = (t_exit, mag_exit, exit_exact) if t_exit <= t_end else (t_end, mag_end, end_exact)
        if binaries[lvl, idx[0], idx[1], idx[2]]:
            if not cont:
                t_last, mag_run, k, run_exact = t, mag_t, 0, t_exact
            pending = False  # (a mid-point tie at the previous voxel's exit: the run goes on, the same sample comes from here)
            while True:
                tc = t_last * cone
                dt = min(max(tc, step), BIG)
                mid = t_last + dt * 0.5
                run_exact = run_exact and (cone == 0.0 or _is32(tc)) and _is32(dt * 0.5) and _is32(mid)
                if abs(mid - t_clip) <= K_TIE * U * (mag_run + (k + 1) * abs(mid) + mag_clip):
                    pending = not (mid == t_clip and run_exact and clip_exact)
                if not mid < t_clip:
                    break
                out["ts"].append(t_last), out["te"].append(t_last + dt), out["mag"].append(mag_run), out["k"].append(k)
                t_last, k = t_last + dt, k + 1
                run_exact = run_exact and _is32(t_last)
            cont = True
        else:
            cont = False
            if pending:
                _tie(out, "mid")
            pending = False
        t, mag_t, t_exact = t_clip, mag_clip, clip_exact
    if pending:
        _tie(out, "mid")
    return out


@dataclass
class MarchRef:
    counts: np.ndarray  # [R] int64
    ties: np.ndarray  # [R] int64
    ts: np.ndarray  # packed float64
    te: np.ndarray
    mag_s: np.ndarray  # bound magnitudes of t_starts / t_ends
    mag_e: np.ndarray

    @property
    def decided(self) -> np.ndarray:
        return self.ties == 0

    @property
    def undecided_share(self) -> float:
        return float((self.ties > 0).mean()) if self.ties.size else 0.0

    def samples_per_decided_ray(self) -> float:
        return float(self.counts[self.decided].mean()) if self.decided.any() else 0.0


def march_oracle(case: MarchCase) -> MarchRef:
    o, d = case.o.double().tolist(), case.d.numpy()
    counts, ties, ts, te, ms, me = [], [], [], [], [], []
    for r in range(case.R):
        near, near_mag, near_exact = case.near, abs(case.near), True
        if case.nears is not None:
            near = float(case.nears[r])
            near_mag = abs(near)
        if case.jitter is not None:
            j = float(case.jitter[r]) * case.jitter_step
            near_exact = _is32(j) and _is32(near + j)
            near, near_mag = near + j, abs(near) + abs(j) + abs(near + j)
        far = case.far if case.fars is None else float(case.fars[r])
        dr = [float(v) for v in d[r]]  # (keeps the sign of -0.0)
        x = march_ray64(o[r], dr, case.binaries, case.roi, near, near_mag, far, case.step, case.cone, near_exact)
        counts.append(len(x["ts"])), ties.append(x["ties"])
        ts += x["ts"]
        te += x["te"]
        ms += [mg + (k + 1) * abs(t) for mg, k, t in zip(x["mag"], x["k"], x["ts"])]
        me += [mg + (k + 2) * abs(t) for mg, k, t in zip(x["mag"], x["k"], x["te"])]
    f = lambda v: np.asarray(v, np.float64)
    return MarchRef(np.asarray(counts, np.int64), np.asarray(ties, np.int64), f(ts), f(te), f(ms), f(me))


def restatement(case: MarchCase, march_one=None) -> Dict:
    """The float32 restatement on the case: oracle/torch_ref.py::march_ray_ref (or ``march_one``, same signature) per ray with that ray's
    planes -> dict(ri, t0, t1, pinfo) of CPU tensors, as umhsnerf.sampler.march_rays returns them."""
    from oracle import torch_ref as T

    fn = T.march_ray_ref if march_one is None else march_one
    ri, s, e = [], [], []
    for r in range(case.R):
        near, far = case.planes(r)
        a, b = fn(case.o[r].numpy(), case.d[r].numpy(), case.binaries, case.roi, near, far, case.step, case.cone)
        ri += [r] * len(a)
        s += a
        e += b
    return pack(ri, s, e, case.R)


MARCH_FAULTS = ("no_restart", "window_restart", "coarse_level", "hx_everywhere", "global_far", "jitter_after_max", "le_midpoint",
                "window_hole", "next_offset")
# the cases each fault can show in (the others do not reach the faulty code: one level, a cubic roi, no per-ray planes, ...)
FAULT_CASES = {
    "no_restart": [n for n in NONEMPTY if n not in ("one_cell", "full", "cube_R1")],  # (needs a second run on a ray)
    "window_restart": [n for n in NONEMPTY if n not in ("one_cell", "sparse", "cube_R1")],  # (needs a run across a 12-voxel boundary)
    "coarse_level": ["cube", "box", "deep", "planes", "wide_cone"],  # (three levels and more; with two the clamp hides it)
    "hx_everywhere": ["box", "deep", "planes"],
    "global_far": ["planes"],
    "jitter_after_max": ["planes"],
    "le_midpoint": ["full"],
    "window_hole": NONEMPTY,
    "next_offset": [n for n in NONEMPTY if n != "cube_R1"],
}


def march_ray_f32(o, d, binaries, roi_aabb, near, far, step, cone, fault=None, jitter=None, global_far=None):
    """oracle/torch_ref.py::march_ray_ref again (same float32 operations in the same order: tests/test_sampler_f64_bounds_cpu.py holds the
    two bit-identical without a fault), with a switch per planted fault of the walk.  ``jitter``: (near plane without it, jitter *
    jitter_step) for 'jitter_after_max'; ``global_far`` for 'global_far'."""
    levels, res = binaries.shape[0], binaries.shape[1]
    a = np.asarray(roi_aabb, dtype=np.float32).reshape(2, 3)
    c, h = (a[0] + a[1]) / F32(2), (a[1] - a[0]) / F32(2)
    if fault == "hx_everywhere":
        h = np.full(3, h[0], np.float32)
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    near, far, step, cone = F32(near), F32(far), F32(step), F32(cone)
    if fault == "global_far" and global_far is not None:
        far = F32(global_far)
    B = F32(1e30)
    inv = np.where(d != 0, F32(1) / np.where(d != 0, d, F32(1)), np.where(np.signbit(d), -B, B)).astype(np.float32)
    inv_h = (F32(1) / h).astype(np.float32)
    ho = h * F32(2 ** (levels - 1))
    t0, t1 = (c - ho - o) * inv, (c + ho - o) * inv
    tn, tf = np.max(np.minimum(t0, t1)), np.min(np.maximum(t0, t1))
    if fault == "jitter_after_max" and jitter is not None:
        t = F32(max(tn, F32(jitter[0])) + F32(jitter[1]))
    else:
        t = max(tn, near)
    t_end = min(tf, far)
    ts, te = [], []
    if not (t < t_end):
        return ts, te
    continuous, t_last = False, t
    guard = 0
    while t < t_end and guard < 100000:
        guard += 1
        tm = t + F32(1e-5) * max(F32(1), abs(t))
        p = o + d * tm
        m = np.max(np.abs(p - c) * inv_h)
        if not (m < F32(2 ** (levels - 1))):
            break
        lvl = 0 if m < F32(1) else int(np.frexp(m)[1])
        if fault == "coarse_level" and F32(1) <= m < F32(2):
            lvl += 1
        lvl = min(max(lvl, 0), levels - 1)
        hl = h * F32(2**lvl)
        vmin_l = c - hl
        vs = (hl * F32(2)) / F32(res)
        inv_vs = F32(1) / vs
        idx = np.clip(np.floor((p - vmin_l) * inv_vs).astype(np.int64), 0, res - 1)
        lo, hi = vmin_l + idx.astype(np.float32) * vs, vmin_l + (idx + 1).astype(np.float32) * vs
        tx = (np.where(d >= 0, hi, lo) - o) * inv
        t_exit = np.min(np.where(d != 0, tx, B))
        if not (t_exit > t):
            t_exit = np.nextafter(t, B, dtype=np.float32)
        t_clip = min(t_exit, t_end)
        if fault == "window_restart" and (guard - 1) % 12 == 0:  # a new lane of the wave walk forgets the run it is in
            continuous = False
        if binaries[lvl, idx[0], idx[1], idx[2]]:
            if not continuous and not (fault == "no_restart" and len(ts) > 0):
                t_last = t
            while True:
                dt = min(max(t_last * cone, step), B)
                mid = t_last + dt * F32(0.5)
                if not (mid <= t_clip if fault == "le_midpoint" else mid < t_clip):
                    break
                if not (fault == "window_hole" and (guard - 1) % 64 < 12):
                    ts.append(t_last)
                    te.append(t_last + dt)
                t_last = t_last + dt
            continuous = True
        else:
            continuous = False
        t = t_clip
    return ts, te


def faulty_restatement(case: MarchCase, fault: Optional[str], ref: Optional["MarchRef"] = None) -> Dict:
    """The float32 restatement's result on the case with ``fault`` planted (None: march_ray_f32 without one)."""
    if fault == "next_offset":  # one ray's samples written at the next ray's offset
        got = {k: v.clone() for k, v in restatement(case).items()}
        cnt = got["pinfo"][:, 1]
        dec = torch.from_numpy(ref.decided) if ref is not None else torch.ones_like(cnt, dtype=torch.bool)
        r = int(torch.nonzero((cnt[:-1] > 0) & (cnt[1:] > 0) & dec[:-1] & dec[1:])[0])
        a, b, m = int(got["pinfo"][r, 0]), int(got["pinfo"][r + 1, 0]), int(cnt[r])
        for k in ("t0", "t1"):
            rows = got[k][a:a + m].clone()
            end = min(b + m, got[k].numel())
            got[k][a:a + m] = float("nan")  # (never written: the buffers are NaN before the launch)
            got[k][b:end] = rows[:end - b]
        return got

    def one(o, d, binaries, roi, near, far, step, cone, r=[0]):
        i = r[0]
        r[0] += 1
        jit = None
        if case.jitter is not None:
            jit = (case.nears[i].numpy(), F32(case.jitter[i].numpy() * F32(case.jitter_step)))
        return march_ray_f32(o, d, binaries, roi, near, far, step, cone, fault, jit, case.far if case.fars is not None else None)

    return restatement(case, one)


def pack(ri, s, e, R: int) -> Dict:
    ri = torch.tensor(ri, dtype=torch.int64)
    counts = torch.bincount(ri, minlength=R)[:R] if R else torch.zeros(0, dtype=torch.int64)
    return {"ri": ri, "t0": torch.tensor(np.asarray(s, np.float32)), "t1": torch.tensor(np.asarray(e, np.float32)),
            "pinfo": torch.stack([torch.cumsum(counts, 0) - counts, counts], 1)}


# ------------------------------------------------------------------------------------------------------------------------------ #
# the marcher's comparator
# ------------------------------------------------------------------------------------------------------------------------------ #
def _occupied_near(case: MarchCase, rays: np.ndarray, mids: np.ndarray) -> np.ndarray:
    """bool per sample: the float64 mid-point, or a point within the margins of it (module docstring), lies in an occupied cell of
    its own level or a coarser one."""
    a = np.asarray(case.roi, np.float64).reshape(2, 3)
    c, h = (a[0] + a[1]) / 2, (a[1] - a[0]) / 2
    o, d = case.o.double().numpy()[rays], case.d.double().numpy()[rays]
    dt = 3e-5 * np.maximum(1.0, np.abs(mids))
    tt = np.stack([mids - dt, mids, mids + dt], 1)  # [n,3]
    P = o[:, None, :] + d[:, None, :] * tt[:, :, None]  # [n,3,3]
    eps = 64 * U * (np.abs(o) + np.abs(d * mids[:, None]) + np.abs(c) + h * 2.0 ** (case.levels - 1))  # [n,3]
    offs = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(27, 3)
    P = P[:, :, None, :] + offs[None, None] * eps[:, None, None, :]  # [n,3,27,3]
    m = (np.abs(P - c) / h).max(-1)
    ok = np.zeros(P.shape[:3], bool)
    for lvl in range(case.levels):
        hl = h * 2.0 ** lvl
        idx = np.clip(np.floor((P - (c - hl)) / (2 * hl / case.res)).astype(np.int64), 0, case.res - 1)
        ok |= (m < 2.0 ** lvl) & case.binaries[lvl][idx[..., 0], idx[..., 1], idx[..., 2]]
    return ok.reshape(ok.shape[0], -1).any(1)


def check_march(case: MarchCase, ref: MarchRef, got: Dict, report: Optional[Dict] = None) -> List[str]:
    """got: dict(ri, t0, t1, pinfo) tensors.  The rule of the module docstring; report: worst ratios of t_starts / t_ends over the
    decided rays, the number of samples compared, the undecided share."""
    ri, t0, t1, pinfo = (got[k].detach().cpu() for k in ("ri", "t0", "t1", "pinfo"))
    R = case.R
    fails = []
    if tuple(pinfo.shape) != (R, 2) or pinfo.dtype != torch.int64 or ri.dtype != torch.int64:
        return [f"packed_info {tuple(pinfo.shape)} {pinfo.dtype}, ray_indices {ri.dtype}"]
    counts = pinfo[:, 1]
    if bool((counts < 0).any()) or not torch.equal(pinfo[:, 0], torch.cumsum(counts, 0) - counts):
        return ["packed_info is not (exclusive prefix, count)"]
    n = int(counts.sum())
    if not (ri.numel() == t0.numel() == t1.numel() == n):
        return [f"{ri.numel()} / {t0.numel()} / {t1.numel()} samples for counts that sum to {n}"]
    if not torch.equal(ri, torch.repeat_interleave(torch.arange(R), counts)):
        fails.append("ray_indices is not the expansion of packed_info")
    cg, t0, t1 = counts.numpy(), t0.double().numpy(), t1.double().numpy()
    if not (np.isfinite(t0).all() and np.isfinite(t1).all()):
        return fails + ["non-finite samples"]
    sg, sr = np.cumsum(cg) - cg, np.cumsum(ref.counts) - ref.counts
    dec = ref.decided
    bad = np.nonzero(dec & (cg != ref.counts))[0]
    if bad.size:
        r = int(bad[0])
        fails.append(f"decided ray {r}: {int(cg[r])} samples, float64 has {int(ref.counts[r])} ({bad.size} such rays)")
    worst = {"t_starts": 0.0, "t_ends": 0.0}
    n_cmp = 0
    for r in np.nonzero(dec & (cg == ref.counts))[0]:
        a, b, m = int(sg[r]), int(sr[r]), int(cg[r])
        if m == 0:
            continue
        n_cmp += m
        for name, g, x, mag, K in (("t_starts", t0, ref.ts, ref.mag_s, K_STARTS), ("t_ends", t1, ref.te, ref.mag_e, K_ENDS)):
            ratio = np.abs(g[a:a + m] - x[b:b + m]) / (U * mag[b:b + m])
            w = float(ratio.max())
            worst[name] = max(worst[name], w)
            if w > K and len(fails) < 8:
                i = int(ratio.argmax())
                fails.append(f"{name}: ray {int(r)} sample {i}: {g[a + i]:.9g} vs float64 {x[b + i]:.9g} = {w:.3g} u mag (K = {K:g})")
    und = np.nonzero(~dec)[0]
    over = [int(r) for r in und if abs(int(cg[r]) - int(ref.counts[r])) > int(ref.ties[r])]
    if over:
        r = over[0]
        fails.append(f"undecided ray {r}: {int(cg[r])} samples vs {int(ref.counts[r])} with {int(ref.ties[r])} tie events ({len(over)} such rays)")
    rows, mids = [], []
    for r in und:
        a, m = int(sg[r]), int(cg[r])
        s, e = t0[a:a + m], t1[a:a + m]
        if m and not (bool((np.diff(s) > 0).all()) and bool((e > s).all())):
            fails.append(f"undecided ray {int(r)}: samples are not sorted")
        want = np.maximum(s * case.cone, case.step)
        if m and bool((np.abs((e - s) - want) > 4 * U * np.maximum(1.0, np.abs(e))).any()):
            fails.append(f"undecided ray {int(r)}: a sample's length is not max(t cone, step)")
        rows += [int(r)] * m
        mids.append((s + e) / 2)
    if rows:
        ok = _occupied_near(case, np.asarray(rows), np.concatenate(mids))
        if not bool(ok.all()):
            i = int(np.nonzero(~ok)[0][0])
            fails.append(f"undecided ray {rows[i]}: a mid-point lies in no occupied cell ({int((~ok).sum())} samples)")
    if report is not None:
        report.update({"t_starts": worst["t_starts"], "t_ends": worst["t_ends"], "samples_compared": n_cmp,
                       "undecided_share": ref.undecided_share})
    return fails


def teeth_failures(case: MarchCase, ref: MarchRef) -> List[str]:
    fails = []
    if ref.undecided_share > 0.10:
        fails.append(f"{ref.undecided_share:.3f} of the rays is undecided (cap 0.10)")
    if case.name in NONEMPTY and case.R > 1 and ref.samples_per_decided_ray() < 50:
        fails.append(f"only {ref.samples_per_decided_ray():.1f} samples per decided ray")
    return fails


# ------------------------------------------------------------------------------------------------------------------------------ #
# visibility
# ------------------------------------------------------------------------------------------------------------------------------ #
VIS_PAIRS = [(1e-4, 0.01), (1e-4, 0.0), (0.0, 0.02), (0.3, 0.0)]
VIS_ROWS = (0, 1, 63, 64, 65, 127, 128, 129, 200, 1000)
VIS_CASES = {"thin_r1": ("thin", 1), "thin_r2": ("thin", 2), "wall_r3": ("wall", 3), "thin_r0": ("thin", 4)}


@dataclass
class VisCase:
    name: str
    counts: torch.Tensor  # [R] int64
    sigma: torch.Tensor  # [n] float32
    t0: torch.Tensor
    t1: torch.Tensor

    @property
    def R(self) -> int:
        return self.counts.numel()

    def packed_info(self) -> torch.Tensor:
        return torch.stack([torch.cumsum(self.counts, 0) - self.counts, self.counts], 1).contiguous()


def vis_oracle(case: VisCase):
    """float64 (T, X, alpha) per sample."""
    x = case.sigma.double() * (case.t1.double() - case.t0.double())
    X = torch.zeros_like(x)
    for s, c in case.packed_info().tolist():
        X[s:s + c] = torch.cumsum(x[s:s + c], 0) - x[s:s + c]
    return torch.exp(-X), X, -torch.expm1(-x)


def vis_undecided(case: VisCase, eps: float, thre: float, scale: float = 1.0) -> torch.Tensor:
    T, X, alpha = vis_oracle(case)
    und = torch.zeros_like(T, dtype=torch.bool)
    if eps > 0:  # (T >= 0 holds in any arithmetic, for an underflowed T = 0 too)
        und |= (T - _f32(eps)).abs() <= scale * K_VIS * U * T * (1 + X)
    if thre > 0:
        und |= (alpha - _f32(thre)).abs() <= scale * K_VIS * U
    return und


def make_vis_case(name: str) -> VisCase:
    """The rows of VIS_ROWS, then 1-4 short rows (R % 4 = 1, 2, 3, 0), then ten empty rays: whole 4-ray workgroups of them, the last ray
    empty.  thin: sigma = exp(N(2, 1.5)), steps of about 0.0035 -- the long rows cross T = 0.3 and T = 1e-4; wall: the second half of
    every row has sigma = 1e7, the optical depth passes 1e4 there and T underflows to 0.  sigma is moved until no sample is within
    10 x the margin of a threshold of VIS_PAIRS."""
    regime, extra = VIS_CASES[name]
    g = torch.Generator().manual_seed(5100 + extra)
    counts = torch.tensor(VIS_ROWS + (17,) * extra + (0,) * 10, dtype=torch.int64)
    n = int(counts.sum())
    delta = 0.0035 * (0.5 + torch.rand(n, generator=g))
    ri = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    start = torch.cumsum(counts, 0) - counts
    cum = torch.cumsum(delta.double(), 0) - delta.double()
    t0 = (0.05 + torch.rand(counts.numel(), generator=g).double()[ri] + cum - cum[start[ri]]).float()
    t1 = t0 + delta
    sigma = torch.exp(torch.randn(n, generator=g) * 1.5 + 2.0)
    if regime == "wall":
        pos = torch.arange(n) - start[ri]
        sigma[pos * 2 >= counts[ri]] = 1e7
    case = VisCase(name, counts, sigma, t0, t1)
    for _ in range(50):
        close = torch.zeros(n, dtype=torch.bool)
        for eps, thre in VIS_PAIRS:
            close |= vis_undecided(case, eps, thre, scale=10.0)
        if not bool(close.any()):
            break
        i = int(torch.nonzero(close)[0])  # the first one: moving it moves every T behind it
        case.sigma[i] = case.sigma[i] * 1.37
    return case


def check_visibility(case: VisCase, eps: float, thre: float, mask, kept=None, report: Optional[Dict] = None) -> List[str]:
    """mask [n] (bool or uint8), kept [R] | None.  Decided elements equal the float64 decision; kept is the mask's own row sum."""
    mask = mask.detach().cpu().reshape(-1)
    n = int(case.counts.sum())
    if mask.numel() != n:
        return [f"mask has {mask.numel()} elements, want {n}"]
    if mask.dtype != torch.bool and bool((mask > 1).any()):
        return ["mask holds values other than 0 and 1"]
    mask = mask.bool()
    T, X, alpha = vis_oracle(case)
    want = T >= _f32(eps)
    if thre > 0:
        want &= alpha >= _f32(thre)
    und = vis_undecided(case, eps, thre)
    bad = (mask != want) & ~und
    fails = []
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        fails.append(f"mask[{i}] = {bool(mask[i])}: T = {float(T[i]):.6g}, alpha = {float(alpha[i]):.6g} vs ({eps}, {thre}); {int(bad.sum())} decided elements differ")
    if kept is not None:
        ri = torch.repeat_interleave(torch.arange(case.R), case.counts)
        rows = torch.zeros(case.R, dtype=torch.int64).index_add_(0, ri, mask.long())
        k = kept.detach().cpu()
        if k.dtype != torch.int64 or not torch.equal(k, rows):
            r = int(torch.nonzero(k != rows)[0]) if k.shape == rows.shape else -1
            fails.append(f"kept differs from the row sums of the mask (first at ray {r})")
    if report is not None:
        report.update({"undecided_share": float(und.float().mean()) if n else 0.0, "ties_taken_the_other_way": int(((mask != want) & und).sum())})
    return fails


def visibility_f32(case: VisCase, eps: float, thre: float, fault: Optional[str] = None):
    """render_visibility_from_density in float32, written as the kernel's chunked scan so that a fault can be planted:
    'carry' (dropped at a 64-sample chunk), 'inclusive' (sum includes the sample itself), 'kept64' (kept off by one on a row of 64)."""
    x = case.sigma * (case.t1 - case.t0)
    X = torch.zeros_like(x)
    for s, c in case.packed_info().tolist():
        carry = torch.zeros((), dtype=torch.float32)
        for b in range(s, s + c, 64):
            xs = x[b:min(b + 64, s + c)]
            inc = torch.cumsum(xs, 0)
            X[b:b + xs.numel()] = carry + (inc if fault == "inclusive" else inc - xs)
            carry = (carry + inc[-1]) if fault != "carry" else torch.zeros((), dtype=torch.float32)
    T, alpha = torch.exp(-X), 1.0 - torch.exp(-x)
    mask = T >= F32(eps).item()
    if thre > 0:
        mask &= alpha >= F32(thre).item()
    ri = torch.repeat_interleave(torch.arange(case.R), case.counts)
    kept = torch.zeros(case.R, dtype=torch.int64).index_add_(0, ri, mask.long())
    if fault == "kept64":
        kept[case.counts == 64] -= 1
    return mask, kept, T, alpha
