"""Hash-grid cases, their float64 oracle, a float32 model of the kernels' own arithmetic and the per-element / per-slot comparators
(plain helper module, no tests in it).

Used by tests/test_hip_hash_f64.py (csrc/umhs_hash.h, umhs_hashgrid.hip, umhs_hashgrid_part.h on the GPU) and by
tests/test_hash_f64_bounds_cpu.py (the comparators pass the float32 model and reject planted faults; K, the teeth condition and the
fixed-point quantum are measured there).  It mirrors tests/rays_f64.py and tests/field_f64.py for the stage in front of them.

ORACLE.  The reference (oracle/torch_ref.hash_encode = HashEncoding.pytorch_fwd) DEFINES the grid coordinate as one float32 product
x * scale_l; its floor, its ceil and offset = scaled - floor are then exact in float32.  The oracle therefore takes that float32
product, the integer corners and torch_ref.hash_fn as they are, and does everything downstream in float64: the trilinear blend
(forward), and w_c * g summed per table slot (backward, w_c the product of the three float64 weights of corner c).  A genuine float64
x * scale is the WRONG truth: it moves every offset by up to half an ulp of a coordinate of ~2047, i.e. about 1e-4 of a feature, and
would have the kernels fail for following the reference.  Next to every float64 value stands its envelope ``mag``: the float64 sum of
the absolute values of the same terms (sum_c w_c |f_c|; sum over the contributions of a slot of |w_c g|).

RULES, u = 2^-24, tiny = 2^-126:
  forward, every element of enc:   |got - ref64| <= K_f u (mag + tiny),  AND  got == float32 torch_ref.hash_encode bit for bit
      (hash_corners and hash_trilerp switch contraction off and copy the reference's expression tree: the source promises the bits).
  partitioned backward, every slot component a non-zero contribution reaches (n_s of them):
      |got - ref64| <= K_b u (mag + tiny) + n_s Q   (+ u |prior + ref64| when accumulating onto a prior table)
  atomic backward (float32 adds in arbitrary order):   |got - ref64| <= K_a u (n_s + 4) (mag + tiny);  when accumulating, the prior
      is one more term of that float32 sum -- every one of the n_s adds rounds at the prior's magnitude -- so mag includes |prior|
  every other slot component: exactly +0 in overwrite mode, exactly the prior's bits in accumulate mode (contributions with a zero
  weight or a zero gradient add an exact zero).
Q is the partitioned path's fixed-point quantum per addend, per (level, bucket), as an UPPER bound formed the way hg_reduce_kernel
forms its scale:  kfix = min(62 - hb - e, 150),  e = frexp exponent of 16 x the level's max |g| (a merged run sums up to 16 samples,
each |w g| <= |g|),  hb = bit_length(8 x the samples with a corner in the bucket) + 1 (at most 8 records per sample),
Q = E_FIX 2^-kfix.  E_FIX = 128 units is hb_fixed's worst error per addend: for a negative addend in (-1, 0) units of 2^32 the
remainder x - floorf(x) = 1 + x is NOT exact -- it rounds to the float32 grid of spacing 2^-24 below 1, half of which is 2^7 units of
2^-32 -- and where it rounds to 1.0f the conversion of 2^32 to uint32_t saturates (v_cvt_u32_f32) to 2^32 - 1.  Positive addends and
negative ones below -1 are exact up to the floor (< 1 unit).  tests/test_hash_f64_bounds_cpu.py sweeps a float32 emulation of
hb_fixed over both signs and binades -40..5: worst 128.0 units from floor(x 2^32) for negative addends, 0 for positive ones.

K = max(8, 4 x worst, rounded up to a power of two), with the reasons of tests/rays_f64.py (floor of 8: device arithmetic and
association may differ by a couple of ulp from the model; factor 4: margin over a float32 evaluation in another order).  ``worst`` is
measured on the CPU over every committed case: forward from float32 torch_ref.hash_encode; backward from a float32 MODEL of the
kernels' own arithmetic (``partition_model(exact=True)``: pair records (g * wyz) * ((1 - ox) 2^k), merged runs (rx * oy * oz) * g summed
by the segmented row scan in its own association, the addends then accumulated exactly and rounded once); atomic from w_c * g added in
float32 in sample order.  Measured worsts (tests/test_hash_f64_bounds_cpu.py re-measures and asserts 4 x worst <= K):
  forward 3.69 | partitioned backward 3.61 | atomic backward 0.55 (in units of u (n_s + 4) mag)
so K_f = K_b = 16 and K_a = 8.  (The non-exact ``partition_model`` follows hg_reduce_kernel's int64 fixed point too, with hb_fixed's
remainder as hipcc compiles it there -- vx * rx - floorf(.) contracted into one fma of the unrounded product -- or, contract=False, as
the source spells it; both pass the rule.  It emulates the arithmetic, not a compiler, so the GPU test REPORTS how many slot components
differ from it in bits and asserts nothing about them.)

TEETH: the share of touched slot components (elements) with |ref64| > 16 x bound.  Condition: in the "scattered" and "rays" cases at
least 90 % of the touched slot components have teeth under the partitioned rule (checked on the CPU from the float64 run alone).

GRADIENTS (``make_grads``): mixed signs, |g| = 10^(-9 r^3) with r uniform (nine decades inside every level, most of the mass in the
upper ones so that the teeth condition holds under Q); every 37th sample carries -1e-12 (1 + r) on every level and both components --
on the fine levels its slots have no other source, which is hb_fixed's inexact case, more than 11 decades below the level maximum;
samples 20 and 21 of every 48 are exact zeros (the middle of a ray's runs: the one-call form drops them and breaks the run there, the
prepare / apply form keeps them as zero records), sample 30 of every 48 has a zero second component.

POSITION SETS (all in [0, 1]; ``positions``):  edges | scattered | rays (64 rays x 48 samples + 5 of a 65th) | threshold (two waves
of 64 whose level-0 runs have exactly 15 and exactly 16 continuing lanes: below / at HB_MERGE_MIN) | tiny (2 in one cell) |
one_cell (N = 1).

WHICH CASE REACHES WHICH PATH (backward cases are (set, log2_T, levels)):
  scattered 12 (N = 3000)   nb = 1 (bucket_bits = 12), ~12,000 pair records in the one bucket: both register sets of the reduce's
                            record loop and its second round (records past 4096 and 8192); merge off; pair records, every k
  rays 13 (N = 3077)        nb = 1; merge ON on the coarse levels (runs of ~10 samples), runs cut by the 16-lane row, by sample 256
                            of a 512-sample run and by the end of the batch (5 samples in the last run); singles from merged runs
                            next to pair records of solo samples; zero-gradient samples inside runs (grad_mask 1 against 0)
  edges 13                  eq flags (x, y, z integer on one, two, three axes; singles with k = 15 and ox = 0), 0.0 and 1.0, the
                            float32 neighbours of an integer coordinate, k = 0..10 at the finest level, even / odd floor-x (paired
                            16-byte load against the separate fetch), exact duplicates (runs of 2: merge off -> two solo samples)
  threshold 13              merge off (15 continuing lanes) and on (16) in neighbouring waves of one run
  tiny 13 / one_cell 13     N = 2, N = 1: one partial wave, every lane but one or two inactive
  scattered 19 (N = 8193)   nb = 64: one full round of the bucket scan; 17 runs, the last with one sample
  scattered 20 (N = 1025, levels 12..15)   nb = 128: second half of the scan wave (buckets >= 64 need the first round's carry)
  split records (a pair whose partner lies in another bucket) need a resolution >= 8192; the committed scalings stop at 2047, so no
  case here emits them (tests/test_hip_parity.py has that case) and the model refuses them.
Scalar against vector accesses: tests/test_hip_hash_f64.py runs d_enc views that start one float into their storage with even and with
odd strides (hb_load's scalar gradient load) and an enc buffer of row stride 33 (the forward's scalar store)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from oracle import torch_ref as T

U = 2.0 ** -24
TINY = 2.0 ** -126
TEETH = 16.0
K_F = 16.0
K_B = 16.0
K_A = 8.0
E_FIX = 128.0  # hb_fixed's worst error per addend, in units of the fixed-point quantum
BUCKET_BITS, MERGE_MIN = 13, 16
FI, CI = (3, 2, 7, 6), (0, 1, 4, 5)  # floor-x / ceil-x corner of the four (y, z) combinations (c,c) (f,c) (c,f) (f,f)
# corner order of HashEncoding.pytorch_fwd, 1 = ceil on that axis (x, y, z)
CORNER_CEIL = ((1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0))
ALL_LEVELS = tuple(range(16))

# (position set, log2_T, levels, N)
BWD_CASES = {
    "scattered12": ("scattered", 12, ALL_LEVELS, 3000), "rays13": ("rays", 13, ALL_LEVELS, 3077), "edges13": ("edges", 13, ALL_LEVELS, 0),
    "threshold13": ("threshold", 13, ALL_LEVELS, 128), "tiny13": ("tiny", 13, ALL_LEVELS, 2), "one_cell13": ("one_cell", 13, ALL_LEVELS, 1),
    "scattered19": ("scattered", 19, ALL_LEVELS, 8193), "scattered20": ("scattered", 20, (12, 13, 14, 15), 1025),
}
TEETH_CASES = ("scattered12", "rays13", "scattered19", "scattered20")
# (position set, log2_T, N): edges followed by random positions up to N in all (one past a 256-thread block, one past a 512-sample
# run); a negative N: edges plus that many random positions
FWD_CASES = {"one12": ("one_cell", 12, 1), "edges13_257": ("edges", 13, 257), "edges13_513": ("edges", 13, 513),
             "edges19_plus4225": ("edges", 19, -(4096 + 129))}


def report_dir(root: str) -> str:
    import rays_f64

    return rays_f64.report_dir(root)


# ------------------------------------------------------------------------------------------------------------------------------ #
# positions and gradients
# ------------------------------------------------------------------------------------------------------------------------------ #
def _vertex(k: int, s: float) -> float:
    """A float32 x with float32(x * s) == k' exactly, k' the first of k, k + 1, ... that has one among the floats around k' / s (not
    every product lands on the integer: the products of neighbouring floats can step over it)."""
    for kk in range(k, k + 32):
        x0 = np.float32(kk / s)
        cand = [x0]
        lo = hi = x0
        for _ in range(8):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            cand += [lo, hi]
        for c in cand:
            if 0 <= c <= 1 and np.float32(c) * np.float32(s) == np.float32(kk):
                return float(c)
    raise AssertionError(f"no float32 x with x * {s} an integer from {k} on")


def edge_positions() -> torch.Tensor:
    sc = T.hash_scalings()
    rows: List[List[float]] = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.37], [1.0, 0.0, 0.61], [0.29, 0.0, 1.0]]
    for lv, ks in ((0, (3, 8, 16)), (7, (1, 77, 140)), (15, (2, 1023, 2046))):
        s = float(sc[lv])
        v = [_vertex(k, s) for k in ks]
        rows += [[v[0], 0.3141, 0.2718], [0.4142, v[1], 0.7321], [0.1234, 0.5678, v[2]]]  # one axis
        rows += [[v[0], v[1], 0.6180], [0.2236, v[1], v[2]], [v[2], 0.3333, v[0]]]  # two axes
        rows += [[v[0], v[1], v[2]], [v[1], v[1], v[1]]]  # three axes
    s15 = float(sc[15])
    for m in range(1, 11):  # floor-x = 2^m - 1 at the finest level: xf ^ xc = 2^(m+1) - 1, record k = m
        rows.append([(2 ** m - 1 + 0.37) / s15, 0.11 + 0.07 * m, 0.93 - 0.05 * m])
    for k in (4, 5, 10, 11):  # even and odd floor-x (level 0 and, scaled, every level)
        rows.append([(k + 0.25) / 16.0, (k + 0.5) / 16.0, (k + 0.75) / 16.0])
    for k in (1, 7, 12):  # the float32 neighbours of an integer coordinate (scale 16 is a power of two: the products are exact)
        x0 = np.float32(k / 16.0)
        below, above = float(np.nextafter(x0, np.float32(0))), float(np.nextafter(x0, np.float32(1)))
        rows += [[below, 0.45, 0.55], [above, 0.45, 0.55], [0.35, below, above], [above, above, below]]
    rows += [rows[7], rows[7], rows[20], rows[20], rows[20], rows[-1], rows[-1]]  # exact duplicates, neighbouring lanes
    return torch.tensor(rows, dtype=torch.float32)


def positions(kind: str, n: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(4100 + seed)
    if kind == "scattered":
        return torch.rand(n, 3, generator=g)
    if kind == "edges":
        e = edge_positions()
        n = e.shape[0] - n if n < 0 else n
        return e if n <= e.shape[0] else torch.cat([e, torch.rand(n - e.shape[0], 3, generator=g)])
    if kind == "rays":
        r = (n + 47) // 48
        o = torch.rand(r, 1, 3, generator=g) * 0.5 + 0.1
        d = torch.nn.functional.normalize(torch.randn(r, 1, 3, generator=g), dim=-1)
        return (o + d * torch.linspace(0, 0.3, 48).view(1, 48, 1)).reshape(-1, 3)[:n].clamp(0.0, 1.0).contiguous()
    if kind == "threshold":
        # level 0 (scale 16).  Lanes 0..15 of each wave in cell (5, 6, 7): 15 lanes continue a run.  The other 48 lanes walk through
        # four different cells so that no neighbour repeats; in the second wave lane 17 sits in lane 16's cell: 16 continue.
        assert n == 128
        cells = torch.tensor([[2, 3, 4], [9, 3, 4], [2, 11, 4], [2, 3, 12]], dtype=torch.float32)

        def wave(extra: bool):
            inside = torch.rand(64, 3, generator=g) * 0.9 + 0.05
            cell = torch.empty(64, 3)
            cell[:16] = torch.tensor([5.0, 6.0, 7.0])
            cell[16:] = cells[torch.arange(48) % 4]
            if extra:
                cell[17] = cell[16]
            return (cell + inside) / 16.0

        return torch.cat([wave(False), wave(True)])
    if kind == "tiny":
        assert n == 2
        return torch.tensor([[0.40010, 0.40020, 0.40030], [0.40013, 0.40024, 0.40035]])
    if kind == "one_cell":
        assert n == 1
        return torch.tensor([[0.3217, 0.6543, 0.1871]])
    raise KeyError(kind)


def make_grads(n: int, n_levels: int, seed: int = 0) -> torch.Tensor:
    """[n, n_levels, 2] float32 (module docstring, GRADIENTS)."""
    g = torch.Generator().manual_seed(5200 + seed)
    mag = torch.pow(10.0, -9.0 * torch.rand(n, n_levels, 2, generator=g) ** 3)
    out = mag * (torch.randint(0, 2, (n, n_levels, 2), generator=g) * 2 - 1).float()
    i = torch.arange(n)
    if n > 1:
        out[0], out[1, :, 0], out[1, :, 1] = 1.0, -1e-9, 1e-9  # the ends of the range are there on every level
    small = i % 37 == 3
    out[small] = -1e-12 * (1 + torch.rand(int(small.sum()), n_levels, 2, generator=g))
    out[(i % 48 == 20) | (i % 48 == 21)] = 0.0
    out[i % 48 == 30, :, 1] = 0.0
    return out.contiguous()


# ------------------------------------------------------------------------------------------------------------------------------ #
# geometry: the reference's float32 coordinate, integer corners and hashes
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class Geo:
    log2_T: int
    levels: Sequence[int]
    fl: np.ndarray  # [N, L, 3] int64 floor coordinates
    eq: np.ndarray  # [N, L, 3] bool: the coordinate is an integer (ceil == floor)
    off: np.ndarray  # [N, L, 3] float32 offsets (exact)
    idx: np.ndarray  # [N, L, 8] int64 slot inside the level, corner order of the reference
    idx_x1: np.ndarray  # [N, L, 4] slot of (floor-x + 1, y, z) for the four floor-x corners (planted fault 3 alone)

    @property
    def n(self) -> int:
        return self.fl.shape[0]


def geometry(x: torch.Tensor, levels: Sequence[int], log2_T: int) -> Geo:
    sc = T.hash_scalings()[list(levels)]
    scaled = x[:, None, :] * sc.to(x.dtype).view(-1, 1)  # ONE float32 product, as hash_encode
    ce, fl = torch.ceil(scaled).to(torch.int32), torch.floor(scaled).to(torch.int32)
    off = scaled - fl
    zero = torch.zeros(len(levels), dtype=torch.int64)
    pick = lambda a, b, c: torch.cat([a[..., 0:1], b[..., 1:2], c[..., 2:3]], dim=-1)
    src = (fl, ce)
    idx = torch.stack([T.hash_fn(pick(src[cx], src[cy], src[cz]), 1 << log2_T, zero) for cx, cy, cz in CORNER_CEIL], dim=-1)
    x1 = fl.clone()
    x1[..., 0] += 1
    idx_x1 = torch.stack([T.hash_fn(pick(x1, src[CORNER_CEIL[c][1]], src[CORNER_CEIL[c][2]]), 1 << log2_T, zero) for c in FI], dim=-1)
    return Geo(log2_T, tuple(levels), fl.long().numpy(), (ce == fl).numpy(), off.numpy().astype(np.float32), idx.numpy(), idx_x1.numpy())


def corner_weights64(off: np.ndarray) -> np.ndarray:
    """[..., 8] float64 trilinear weights of the 8 corners from float32 offsets [..., 3]."""
    o = off.astype(np.float64)
    r = 1.0 - o
    ax = lambda a, c: np.where(c, o[..., a], r[..., a])
    return np.stack([ax(0, cx) * ax(1, cy) * ax(2, cz) for cx, cy, cz in CORNER_CEIL], axis=-1)


# ------------------------------------------------------------------------------------------------------------------------------ #
# forward: float64 oracle, float32 model
# ------------------------------------------------------------------------------------------------------------------------------ #
def forward_oracle(geo: Geo, table: torch.Tensor):
    """(ref64 [N, L, 2], mag [N, L, 2]): the reference's blend tree in float64 on the float32 offsets, and sum_c w_c |f_c|."""
    t = table.numpy().reshape(-1, 1 << geo.log2_T, 2)
    lv = np.asarray(geo.levels)
    f = t[lv[None, :, None], geo.idx].astype(np.float64)  # [N, L, 8, 2]
    o = geo.off.astype(np.float64)
    ref = _blend(f, o[..., 0:1], o[..., 1:2], o[..., 2:3], 1.0)
    mag = (corner_weights64(geo.off)[..., None] * np.abs(f)).sum(-2)
    return torch.from_numpy(ref), torch.from_numpy(mag)


def _blend(f, ox, oy, oz, one):
    f03 = f[..., 0, :] * ox + f[..., 3, :] * (one - ox)
    f12 = f[..., 1, :] * ox + f[..., 2, :] * (one - ox)
    f56 = f[..., 5, :] * ox + f[..., 6, :] * (one - ox)
    f47 = f[..., 4, :] * ox + f[..., 7, :] * (one - ox)
    f0312 = f03 * oy + f12 * (one - oy)
    f4756 = f47 * oy + f56 * (one - oy)
    return f0312 * oz + f4756 * (one - oz)


def forward_model(geo: Geo, table: torch.Tensor, fault: Optional[int] = None) -> torch.Tensor:
    """The kernel's gather and blend in float32 numpy, [N, L, 2].  fault 6: the floor-x corner of an odd slot index takes the other half
    of its 16-byte pair."""
    t = table.numpy().reshape(-1, 1 << geo.log2_T, 2)
    lv = np.asarray(geo.levels)
    idx = geo.idx.copy()
    if fault == 6:
        for c in FI:
            idx[..., c] = np.where(idx[..., c] & 1, idx[..., c] ^ 1, idx[..., c])
    f = t[lv[None, :, None], idx]
    o = geo.off
    return torch.from_numpy(_blend(f, o[..., 0:1], o[..., 1:2], o[..., 2:3], np.float32(1.0)).astype(np.float32))


def check_forward(name: str, got, ref64, mag, ref32=None, report: Optional[Dict] = None) -> List[str]:
    """got, ref64, mag, ref32: [N, L, 2].  Both forward rules; report[name] = per level worst ratio, teeth share, elements whose bits
    differ from the float32 reference."""
    got = got.detach().cpu()
    fails = []
    g, r, m = got.double(), ref64.double(), mag.double() + TINY
    d = (g - r).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / (U * m))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    teeth = (r.abs() > TEETH * K_F * U * m).double().mean(dim=(0, 2))
    ne = (got.view(torch.int32) != ref32.view(torch.int32)).sum(dim=(0, 2)) if ref32 is not None else None
    if report is not None:
        report[name] = {"worst": ratio.amax(dim=(0, 2)).tolist(), "teeth": teeth.tolist(), "not_bit_equal": None if ne is None else ne.tolist()}
    if float(ratio.max()) > K_F:
        i = int(ratio.reshape(-1).argmax())
        fails.append(f"{name}: element {np.unravel_index(i, tuple(ratio.shape))}: {float(g.reshape(-1)[i]):.9g} vs float64 {float(r.reshape(-1)[i]):.9g} = "
                     f"{float(ratio.max()):.3g} u mag (K_f = {K_F:g}; {int((ratio > K_F).sum())} over)")
    if ne is not None and int(ne.sum()):
        i = int((got.view(torch.int32) != ref32.view(torch.int32)).reshape(-1).nonzero()[0])
        fails.append(f"{name}: {int(ne.sum())} elements differ in bits from float32 hash_encode, first {np.unravel_index(i, tuple(got.shape))}: "
                     f"{float(got.reshape(-1)[i]):.9g} vs {float(ref32.reshape(-1)[i]):.9g}")
    return fails


# ------------------------------------------------------------------------------------------------------------------------------ #
# backward: float64 oracle per touched slot
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class LevelOracle:
    slots: torch.Tensor  # [S] int64, ascending: slots with at least one non-zero contribution in either component
    ref: torch.Tensor  # [S, 2] float64
    mag: torch.Tensor  # [S, 2] float64
    cnt: torch.Tensor  # [S, 2] float64: non-zero contributions (n_s)
    q: torch.Tensor  # [S] float64: the bucket's quantum bound Q

    def to(self, device):
        return LevelOracle(*(t.to(device) for t in (self.slots, self.ref, self.mag, self.cnt, self.q)))


def quantum(geo: Geo, grads: torch.Tensor, li: int) -> np.ndarray:
    """Q of every bucket of level index li (module docstring): an upper bound of E_FIX x the kernel's fixed-point unit."""
    bb = min(geo.log2_T, BUCKET_BITS)
    nb = 1 << (geo.log2_T - bb)
    gmax = float(grads[:, li].abs().max()) if geo.n else 0.0
    e = math.frexp(16.0 * gmax)[1] if gmax > 0 else -126
    pairs = np.unique(np.repeat(np.arange(geo.n), 8) * nb + (geo.idx[:, li] >> bb).reshape(-1))
    per_bucket = np.bincount(pairs % nb, minlength=nb)  # samples with a corner in the bucket
    q = np.zeros(nb)
    for b in np.nonzero(per_bucket)[0]:
        hb = int(8 * per_bucket[b]).bit_length() + 1
        q[b] = E_FIX * 2.0 ** -min(62 - hb - e, 150)
    return q


def backward_oracle(geo: Geo, grads: torch.Tensor) -> List[LevelOracle]:
    """grads [N, L, 2] float32 (L = len(geo.levels)).  One LevelOracle per level of geo.levels."""
    bb = min(geo.log2_T, BUCKET_BITS)
    w = corner_weights64(geo.off)  # [N, L, 8]
    g = grads.numpy().astype(np.float64)
    out = []
    for li in range(len(geo.levels)):
        c = w[:, li, :, None] * g[:, li, None, :]  # [N, 8, 2]
        slots, inv = np.unique(geo.idx[:, li].reshape(-1), return_inverse=True)
        inv = inv.reshape(-1)
        col = lambda a: np.stack([np.bincount(inv, weights=a[..., k].reshape(-1), minlength=slots.size) for k in (0, 1)], 1)
        ref, mag, cnt = col(c), col(np.abs(c)), col((c != 0).astype(np.float64))
        keep = cnt.sum(1) > 0
        q = quantum(geo, grads, li)[slots[keep] >> bb]
        out.append(LevelOracle(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (slots[keep], ref[keep], mag[keep], cnt[keep], q))))
    return out


def check_backward(name: str, got, oracle: List[LevelOracle], path: str, prior=None, report: Optional[Dict] = None) -> List[str]:
    """got: [L, T, 2] float32 (any device; the oracle on the same one), the d_table slabs of the oracle's levels in order.  path:
    "partition" or "atomic".  prior: the table accumulated onto ([L, T, 2]) or None for overwrite mode.
    report[name] = per level {"worst": the largest (|diff| - n_s Q - prior term) / (u (mag + tiny)) [/ (n_s + 4), |prior| in mag, for atomic], to be held
    against K; "teeth": share of touched components with |ref64| > 16 x bound; "n": touched components}."""
    fails, rep = [], []
    K = K_B if path == "partition" else K_A
    for li, o in enumerate(oracle):
        gl = got[li]
        base = torch.zeros_like(gl) if prior is None else prior[li]
        g = gl[o.slots].double()
        m = o.mag + TINY
        rel = U * m * (o.cnt + 4 if path == "atomic" else 1.0)
        extra = o.cnt * o.q[:, None] if path == "partition" else torch.zeros_like(m)
        want = o.ref
        if prior is not None:
            want = base[o.slots].double() + o.ref
            if path == "atomic":
                rel = U * (m + base[o.slots].double().abs()) * (o.cnt + 4)
            else:
                extra = extra + U * want.abs()
        touched = o.cnt > 0
        d = (g - want).abs()
        ratio = torch.clamp(d - extra, min=0) / rel
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        ratio = torch.where(touched, ratio, torch.zeros_like(ratio))
        worst = float(ratio.max()) if ratio.numel() else 0.0
        bound = K * rel + extra
        teeth = float(((o.ref.abs() > TEETH * bound) & touched).sum()) / max(1, int(touched.sum()))
        rep.append({"worst": worst, "teeth": teeth, "n": int(touched.sum())})
        if worst > K:
            i = int(ratio.reshape(-1).argmax())
            s, k = int(o.slots[i // 2]), i % 2
            fails.append(f"{name}: level index {li} slot {s}[{k}] (bucket {s >> BUCKET_BITS}): {float(g.reshape(-1)[i]):.9g} vs float64 "
                         f"{float(want.reshape(-1)[i]):.9g} = {worst:.3g} (K = {K:g}; n_s {int(o.cnt.reshape(-1)[i])}, mag {float(m.reshape(-1)[i]):.3g}, "
                         f"Q {float(o.q[i // 2]):.3g}; {int((ratio > K).sum())} of {int(touched.sum())} over)")
        # everything no non-zero contribution reaches keeps the bits of its base (+0 or the prior)
        same = gl.view(torch.int32) == base.view(torch.int32)
        same[o.slots] |= touched
        if not bool(same.all()):
            bad = (~same).reshape(-1).nonzero()
            i = int(bad[0])
            fails.append(f"{name}: level index {li}: {bad.numel()} untouched slot components changed, first slot {i // 2}[{i % 2}]: "
                         f"{float(gl.reshape(-1)[i]):.9g}, base {float(base.reshape(-1)[i]):.9g}")
    if report is not None:
        report[name] = rep
    return fails


def teeth_share(rep: List[Dict]) -> float:
    n = sum(r["n"] for r in rep)
    return sum(r["teeth"] * r["n"] for r in rep) / max(1, n)


# ------------------------------------------------------------------------------------------------------------------------------ #
# float32 model of the kernels' arithmetic (numpy)
# ------------------------------------------------------------------------------------------------------------------------------ #
F32 = np.float32


def hb_fixed_model(x: np.ndarray, factors=None) -> np.ndarray:
    """hb_fixed of umhs_hashgrid_part.h on float32 x, as int64: hi = (int)floorf(x), lo = saturating (uint32)((x - floorf(x)) * 2^32).
    factors = (v, w) with x = float32(v * w): the remainder as hipcc compiles it inside hg_reduce_kernel, ONE fma(v, w, -floorf(x)) of
    the unrounded product (contraction is on there).  It is then negative where rounding carried x up to an integer, and the
    conversion saturates to 0 at that end as it does to 2^32 - 1 at the other."""
    x = x.astype(F32)
    fl = np.floor(x)
    if factors is None:
        rem = (x - fl).astype(F32)
    else:  # (the float64 product of two float32 is exact; the difference is rounded twice in rare cases, which is as close as numpy gets)
        rem = (factors[0].astype(np.float64) * factors[1].astype(np.float64) - fl.astype(np.float64)).astype(F32)
    lo = (rem * F32(4294967296.0)).astype(F32)
    lo = np.clip(lo.astype(np.float64), 0.0, 4294967295.0).astype(np.int64)  # v_cvt_u32_f32 saturates at both ends
    return (fl.astype(np.int64) << 32) + lo


def _runs(geo: Geo, li: int, g0, g1, grad_mask: bool):
    """The scatter pass's run structure of one level: (M padded to waves) act, head, tail, solo, merging, and nonhead count per wave."""
    n = geo.n
    M = (n + 63) // 64 * 64
    i = np.arange(M)
    act = np.zeros(M, bool)
    act[:n] = ((g0 != 0) | (g1 != 0)) if grad_mask else True
    key = np.zeros((M, 4), np.int64)
    key[:n, :3] = geo.fl[:, li]
    key[:n, 3] = geo.eq[:, li, 0] + 2 * geo.eq[:, li, 1] + 4 * geo.eq[:, li, 2]
    key[~act] = 0
    key[~act, 0] = -1 - i[~act]  # (unique per lane when inactive)
    head = np.ones(M, bool)
    head[1:] = (key[1:] != key[:-1]).any(1)
    head[i % 16 == 0] = True
    nonhead = (~head).reshape(-1, 64).sum(1)
    merging = np.repeat(nonhead >= MERGE_MIN, 64)
    head = head | ~merging
    nhead = np.concatenate([head[1:], [True]])
    tail = act & ((i % 16 == 15) | nhead)
    return act, head, tail, head & tail, merging, nonhead, key


def partition_model(geo: Geo, grads: torch.Tensor, grad_mask: bool, exact: bool = False, fault=None, stats: Optional[Dict] = None,
                    contract: bool = True) -> torch.Tensor:
    """The partitioned backward (hg_partition_kernel<true> + hg_reduce_kernel) in float32 / int64 numpy: [L, T, 2] float32, what
    overwrite mode writes.  exact: the float32 addends are accumulated in float64 and rounded once (no fixed point) -- the run K_b is
    measured from.  contract: hb_fixed's remainder as compiled (one fma, see hb_fixed_model) or as written.  fault: one of 1, 2, 3, 4, "5a", "5b", 7, 8 (tests/test_hash_f64_bounds_cpu.py).  stats: filled with what the case
    reaches (per level: records of the fullest bucket, pair records by k, merged runs, ...)."""
    Tn, bb = 1 << geo.log2_T, min(geo.log2_T, BUCKET_BITS)
    nb, lowmask = 1 << (geo.log2_T - bb), (1 << bb) - 1
    n, L = geo.n, len(geo.levels)
    out = np.zeros((L, Tn, 2), F32)
    gr = grads.numpy().astype(F32)
    for li in range(L):
        M = (n + 63) // 64 * 64
        pad = lambda a, fill=0: np.concatenate([a, np.full((M - n,) + a.shape[1:], fill, a.dtype)])
        g0, g1 = gr[:, li, 0], gr[:, li, 1]
        act, head, tail, solo, merging, nonhead, key = _runs(geo, li, g0, g1, grad_mask)
        g0, g1 = pad(g0), pad(g1)
        off, slot = pad(geo.off[:, li]), pad(geo.idx[:, li])
        ox, oy, oz = off[:, 0], off[:, 1], off[:, 2]
        rx, ry, rz = F32(1) - ox, F32(1) - oy, F32(1) - oz
        i = np.arange(M)
        # merged runs: (ax * ay) * az per corner, times g, summed by the segmented row scan
        ax = lambda a, c: (ox, oy, oz)[a] if c else (rx, ry, rz)[a]
        w = np.stack([(ax(0, cx) * ax(1, cy)) * ax(2, cz) for cx, cy, cz in CORNER_CEIL], 1)  # [M, 8]
        val = np.where(act[:, None, None], np.stack([w * g0[:, None], w * g1[:, None]], 2), F32(0)).astype(F32)  # [M, 8, 2]
        crosses = merging & (i % 16 == 0) & (i > 0) & ~solo & act
        crosses[1:] &= (key[1:] == key[:-1]).all(1)
        crosses[0] = False
        if fault == 4:
            val[crosses] = 0
        v4, f = val.reshape(-1, 16, 8, 2).copy(), head.reshape(-1, 16).copy()
        l16 = np.arange(16)[None, :]
        for D in (1, 2, 4, 8):
            take = (l16 >= D) & ~f
            prev = np.zeros_like(v4)
            prev[:, D:] = v4[:, :-D]
            v4 = np.where(take[:, :, None, None], (v4 + prev).astype(F32), v4)
            pf = np.zeros_like(f)
            pf[:, D:] = f[:, :-D]
            f = f | ((l16 >= D) & pf)
        val = v4.reshape(M, 8, 2)
        # records: slot, k (15: single), vx, vy, ox, owning sample
        pm = slot[:, FI[0]] ^ slot[:, CI[0]]
        one_bucket = (pm >> bb) == 0
        km = np.where(pm != 0, np.floor(np.log2(np.maximum(pm, 1))).astype(np.int64), 15)
        wyz = np.stack([oy * oz, ry * oz, oy * rz, ry * rz], 1)  # [M, 4]
        R = {k: [] for k in ("slot", "k", "vx", "vy", "ox", "i")}

        def emit(sel, s, k, vx, vy, o):
            for key_, a in zip(("slot", "k", "vx", "vy", "ox", "i"), (s, k, vx, vy, o, i)):
                R[key_].append(np.broadcast_to(a, (M,))[sel])

        pair = solo
        assert not (solo & ~one_bucket).any(), "a pair split over two buckets needs a resolution >= 8192: not modelled"
        for p in range(4):
            s_fl = slot[:, FI[p]]
            if fault == 3:
                s_fl = np.where(pad(geo.eq[:, li, 0]), pad(geo.idx_x1[:, li, p]), s_fl)
            emit(pair, s_fl, km, g0 * wyz[:, p], g1 * wyz[:, p], ox)
        run_tail = tail & ~solo
        for c in range(8):
            emit(run_tail, slot[:, c], 15, val[:, c, 0], val[:, c, 1], F32(0))
        rec = {k: np.concatenate(v) for k, v in R.items()}
        order = np.lexsort((rec["i"], rec["slot"] >> bb))
        rec = {k: v[order] for k, v in rec.items()}
        bucket = rec["slot"] >> bb
        counts = np.bincount(bucket, minlength=nb)
        start = np.cumsum(counts) - counts
        # level maximum as the scatter pass takes it: |g| of solo samples, |sum| of merged records
        lmax = 0.0
        if solo.any():
            lmax = max(lmax, float(np.abs(g0[solo]).max()), float(np.abs(g1[solo]).max()))
        if run_tail.any():
            lmax = max(lmax, float(np.abs(val[run_tail]).max()))
        if stats is not None:
            st = stats.setdefault(geo.levels[li], {})
            st.update(max_bucket_records=int(counts.max()) if counts.size else 0, nb=nb, pair_k=sorted(set(rec["k"].tolist())),
                      merged_records=int(run_tail.sum()) * 8, crossing_runs=int(crosses.sum()), eqx_solo=int((pair & pad(geo.eq[:, li, 0])).sum()),
                      nonhead_per_wave=nonhead.tolist(), buckets_used=int((counts > 0).sum()), high_buckets=int((counts[64:] > 0).sum()),
                      odd_floor_pairs=int((pair & (km > 0) & (km < 15)).sum()))
        if rec["slot"].size == 0 or lmax == 0.0:
            continue
        # the reduce pass reads bucket b's records from its offset
        read_start = start.copy()
        if fault == 7:
            read_start[64:] -= counts[:64].sum()
        rank = np.arange(bucket.size) - start[bucket]
        src = np.clip(read_start[bucket] + rank, 0, bucket.size - 1)
        use = {k: v[src] for k, v in rec.items()}
        keep = np.ones(bucket.size, bool)
        if fault == "5a":
            keep = rank < 4096
        if fault == "5b":
            keep = rank < 8192
        e = math.frexp(lmax)[1]
        hb = np.array([int(c).bit_length() + 1 for c in counts])
        kfix = np.minimum(62 - hb - e, 150) - (20 if fault == 8 else 0)
        kf_rec = kfix[bucket]
        fscale = np.ldexp(F32(1), (kf_rec - 32).astype(np.int32)).astype(F32) if not exact else np.ones(bucket.size, F32)
        s_fl = (bucket << bb) | (use["slot"] & lowmask)
        kk = use["k"]
        has_partner = kk != 15
        kp = kk - 1 if fault == 1 else kk
        kp = np.where((kk == 0) & (fault == 1), 0, kp)
        s_ce = s_fl ^ (((2 << np.clip(kp, 0, 14)) - 1) & lowmask)
        wr, wo = ((F32(1) - use["ox"]) * fscale).astype(F32), (use["ox"] * fscale).astype(F32)
        if fault == 2:
            wr, wo = np.where(has_partner, wo, wr), np.where(has_partner, wr, wo)
        a_fl = np.stack([use["vx"] * wr, use["vy"] * wr], 1).astype(F32)
        a_ce = np.stack([use["vx"] * wo, use["vy"] * wo], 1).astype(F32)
        m_fl, m_ce = keep, keep & has_partner
        # the tile, held for the slots that records land in only (every other slot of a slab that has records is +0)
        us, inv = np.unique(np.concatenate([s_fl[m_fl], s_ce[m_ce]]), return_inverse=True)
        add = np.concatenate([a_fl[m_fl], a_ce[m_ce]])
        fac = (np.concatenate([np.stack([use["vx"], use["vy"]], 1)[m] for m in (m_fl, m_ce)]),
               np.concatenate([wr[m_fl], wo[m_ce]])[:, None]) if contract else None
        if exact:
            tile = np.zeros((us.size, 2), np.float64)
            np.add.at(tile, inv.reshape(-1), add.astype(np.float64))
            out[li][us] = tile.astype(F32)
        else:
            tile = np.zeros((us.size, 2), np.int64)
            np.add.at(tile, inv.reshape(-1), hb_fixed_model(add, fac))
            out[li][us] = np.ldexp(tile.astype(np.float64), -kfix[us >> bb][:, None]).astype(F32)
    return torch.from_numpy(out)


def atomic_model(geo: Geo, grads: torch.Tensor) -> torch.Tensor:
    """hashgrid_bwd_kernel in float32: w_c = (ax * ay) * az, w_c * g added in float32 in sample order (the GPU's order is arbitrary)."""
    Tn = 1 << geo.log2_T
    out = np.zeros((len(geo.levels), Tn, 2), F32)
    gr = grads.numpy().astype(F32)
    for li in range(len(geo.levels)):
        off = geo.off[:, li]
        ox, oy, oz = off[:, 0], off[:, 1], off[:, 2]
        rx, ry, rz = F32(1) - ox, F32(1) - oy, F32(1) - oz
        ax = lambda a, c: (ox, oy, oz)[a] if c else (rx, ry, rz)[a]
        w = np.stack([(ax(0, cx) * ax(1, cy)) * ax(2, cz) for cx, cy, cz in CORNER_CEIL], 1)
        live = ((gr[:, li, 0] != 0) | (gr[:, li, 1] != 0))[:, None] & (w != 0)
        c = (w[:, :, None] * gr[:, li, None, :]).astype(F32)
        np.add.at(out[li], geo.idx[:, li][live], c[live])
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------------------------------ #
# cases, built once per process
# ------------------------------------------------------------------------------------------------------------------------------ #
@dataclass
class BwdCase:
    name: str
    log2_T: int
    levels: Sequence[int]
    x: torch.Tensor  # [N, 3]
    grads: torch.Tensor  # [N, len(levels), 2]
    geo: Geo
    oracle: List[LevelOracle]


_cases: Dict[str, BwdCase] = {}


def bwd_case(name: str) -> BwdCase:
    if name not in _cases:
        kind, log2_T, levels, n = BWD_CASES[name]
        x = positions(kind, n) if n else edge_positions()
        grads = make_grads(x.shape[0], len(levels), seed=len(name))
        geo = geometry(x, levels, log2_T)
        _cases[name] = BwdCase(name, log2_T, levels, x, grads, geo, backward_oracle(geo, grads))
    return _cases[name]


def fwd_table(log2_T: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(6300 + log2_T + seed)
    return (torch.rand(16 << log2_T, 2, generator=g) * 2 - 1) * 0.5
