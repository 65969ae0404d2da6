"""Float64 oracle and error bound of ``ops.segment_stats`` (csrc/umhs_stats.hip), plain torch (helper module, no tests in it).

Used by tests/test_stats_bounds_cpu.py (the oracle on hand-made inputs, the bound against the chain length) and
tests/test_hip_stats.py (the kernel on the GPU).  It follows tests/rays_f64.py and tests/hash_f64.py.

Per segment ``[bounds[k], bounds[k+1])`` of a float32 buffer the kernel returns, in float64,
  [0] the sum of x^2 over the finite elements   [1] the maximum of |x| over the finite elements   [2] the number of NaN / +-Inf.
The maximum and the count involve no rounding: they are compared with ``==``.

The sum.  A float32 has a 24-bit significand, so its square has at most 48 bits and is exact in float64 (and no square of a finite
float32 leaves float64's normal range: 2^-298 .. 2^256).  Every rounding is therefore an ADDITION of non-negative float64 terms, and
a sum of non-negative terms formed by any tree of additions satisfies
        |got - exact| <= gamma_d * exact,      gamma_d = d u / (1 - d u),   u = 2^-53,
where d is the largest number of additions any one term passes through (Higham, Accuracy and Stability, section 4.2: each addition
multiplies what it carries by one factor (1 + delta), |delta| <= u).  The float64 oracle below adds the same exact squares with
``math.fsum``, which returns the correctly rounded exact sum: it is within u of it, the ``ORACLE_DEPTH`` = 1 of ``sum_bound``.

d from the kernel's tiling (csrc/umhs_stats.hip; TILE = 8192 elements, 256 threads):
  thread     at most 1 scalar element in front of the first 16-byte boundary, 8 pieces of 4 elements, 1 scalar
             element behind the last whole piece                                                           1 + 32 + 1 = 34 additions
  wave       __shfl_down tree over 64 lanes                                                                              6
  workgroup  four wave sums added in order                                                                               3
  finish     one wave per segment: a lane adds every 64th tile partial in index order, then the tree   ceil(tiles / 64) + 6
so  chain_length(len) = 34 + 6 + 3 + ceil(ceil(len / TILE) / 64) + 6,  tiles counted from the segment's own start.
"""
import math

import torch

TILE = 8192  # ops.segment_stats_tile(): asserted equal on the GPU
U = 2.0 ** -53
ORACLE_DEPTH = 1  # math.fsum: one rounding of the exact sum


def chain_length(length: int) -> int:
    """Largest number of float64 additions a square passes through in a segment of ``length`` elements."""
    tiles = -(-int(length) // TILE)
    return 34 + 6 + 3 + -(-tiles // 64) + 6


def gamma(d: int) -> float:
    return d * U / (1.0 - d * U)


def sum_bound(length: int, ref_sum: float) -> float:
    """|kernel sum - oracle sum| allowed for a segment of ``length`` elements whose oracle sum is ``ref_sum``: the kernel's gamma plus the
    oracle's own, both relative to the exact sum, which is within gamma(ORACLE_DEPTH) of ``ref_sum``."""
    return (gamma(chain_length(length)) + gamma(ORACLE_DEPTH)) * ref_sum * (1.0 + gamma(ORACLE_DEPTH))


def oracle(x: torch.Tensor, bounds) -> torch.Tensor:
    """float64 [K,3] of the float32 tensor ``x`` (any device) and offsets ``bounds`` [K+1]; empty segments give 0, 0, 0."""
    assert x.dtype == torch.float32
    flat = x.detach().reshape(-1).cpu()
    b = [int(v) for v in (bounds.tolist() if torch.is_tensor(bounds) else bounds)]
    out = torch.zeros(len(b) - 1, 3, dtype=torch.float64)
    for k, (lo, hi) in enumerate(zip(b[:-1], b[1:])):
        seg = flat[lo:hi].double()
        fin = torch.isfinite(seg)
        good = seg[fin]
        if good.numel():
            out[k, 0] = math.fsum((good * good).tolist())  # exact squares, one rounding
            out[k, 1] = good.abs().max()
        out[k, 2] = float((~fin).sum())
    return out


def check(got: torch.Tensor, x: torch.Tensor, bounds, what: str = "") -> float:
    """Asserts ``got`` [K,3] against the oracle: the sum within ``sum_bound``, maximum and count equal.  -> the worst |diff| / bound."""
    ref = oracle(x, bounds)
    got = got.detach().cpu()
    b = [int(v) for v in (bounds.tolist() if torch.is_tensor(bounds) else bounds)]
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, got.shape)
    worst = 0.0
    for k in range(ref.shape[0]):
        g, r = float(got[k, 0]), float(ref[k, 0])
        bound = sum_bound(b[k + 1] - b[k], r)
        assert math.isfinite(g) and abs(g - r) <= bound, (what, k, b[k], b[k + 1], g, r, bound)
        if bound > 0:
            worst = max(worst, abs(g - r) / bound)
        assert float(got[k, 1]) == float(ref[k, 1]), (what, "max", k, float(got[k, 1]), float(ref[k, 1]))
        assert float(got[k, 2]) == float(ref[k, 2]), (what, "count", k, float(got[k, 2]), float(ref[k, 2]))
    return worst
