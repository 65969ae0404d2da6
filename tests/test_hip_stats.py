"""``ops.segment_stats`` (csrc/umhs_stats.hip) on the GPU against the float64 oracle of tests/stats_f64.py: the sum of squares within
the bound its tiling gives, the maximum and the non-finite count exact, equal bits on every launch, nothing outside the bounds read.

Shapes: the smallest at which the kernel takes another path -- an empty segment, fewer elements than the scalar head (1, 3), around a
wave (63, 64, 65), around one tile (TILE - 1, TILE, TILE + 1: the second tile of one element), and 2^20 + 3 (129 tiles: the finish pass
gives a lane more than one partial, and more than one workgroup walks the same segment); every start offset 0..7 against a 16-byte
boundary; K = 1 and the entry count of a real FieldLayout."""
import math

import pytest
import torch

import stats_f64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
LENGTHS = (0, 1, 3, 63, 64, 65, S.TILE - 1, S.TILE, S.TILE + 1, (1 << 20) + 3, 0)  # an empty first and an empty last segment


def _values(n, seed):
    """float32 magnitudes 2^-126 .. 2^60 (squares from float32's denormal range up to 2^120), both signs, with a few true subnormals and
    signed zeros."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-126, 60, (n,), generator=g).double()
    x = (torch.exp2(e) * (1.0 + torch.rand(n, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).float()
    if n >= 8:
        x[torch.randint(0, n, (max(1, n // 64),), generator=g)] = 2.0 ** -140
        x[torch.randint(0, n, (max(1, n // 64),), generator=g)] = -0.0
    return x


def _buffer(lengths, start, seed, plant=True):
    """NaN everywhere outside [bounds[0], bounds[K]); inside, ``_values`` with NaN / Inf at the first element, the last element and both
    sides of every tile boundary of the segments that have one."""
    bounds = [start]
    for n in lengths:
        bounds.append(bounds[-1] + n)
    x = torch.full((bounds[-1] + 5,), NAN, dtype=torch.float32)
    x[start:bounds[-1]] = _values(bounds[-1] - start, seed)
    if plant:
        for k, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            n = hi - lo
            if n >= 63:
                x[lo], x[hi - 1] = (NAN, -INF) if k % 2 else (INF, NAN)
            for t in range(S.TILE, n, S.TILE)[:3]:
                x[lo + t - 1], x[lo + t] = INF, NAN
    return x, bounds


@pytest.fixture(scope="module")
def ops():
    from umhsnerf import ops as O

    assert O.segment_stats_tile() == S.TILE
    return O


@pytest.mark.parametrize("start", range(8))
def test_every_length_at_every_start_offset(ops, start):
    x, bounds = _buffer(LENGTHS, start, seed=start)
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0
    sb = ops.SegmentBounds(bounds, DEV)
    got = ops.segment_stats(xd, sb)
    again = ops.segment_stats(xd, sb)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(LENGTHS), 3) and got.is_cuda
    worst = S.check(got, x, bounds, f"start {start}")
    print(f"start {start}: worst |sum - oracle| / bound = {worst:.3f}")
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))  # the same bits
    assert got[0].tolist() == [0.0, 0.0, 0.0] and got[-1].tolist() == [0.0, 0.0, 0.0]
    ref = S.oracle(x, bounds)
    assert float(ref[:, 2].sum()) >= 20 and float(ref[:, 0].max()) > 2.0 ** 100  # the planted NaN / Inf and the large squares are there


@pytest.mark.parametrize("length", [1, 3, 65, S.TILE + 1])
def test_one_segment(ops, length):
    for start in (0, 1, 6):
        x, bounds = _buffer([length], start, seed=100 + length, plant=False)
        x[start + length - 1] = 2.0 ** -140  # a lone subnormal at the tail
        got = ops.segment_stats(x.to(DEV), bounds)  # plain offsets: a SegmentBounds is built for the call
        S.check(got, x, bounds, f"K=1 length {length} start {start}")
        assert float(got[0, 2]) == 0.0 and float(got[0, 0]) > 0.0


def test_denormal_squares_and_large_squares_are_both_kept(ops):
    """2^-126 elements alone: the sum is 64 * 2^-252, far below float32's range and exact in float64; beside 2^60 they vanish in the sum
    (2^120 has 53 bits) but the maximum sees the large one and the count sees the NaN."""
    x = torch.full((64,), 2.0 ** -126, dtype=torch.float32)
    got = ops.segment_stats(x.to(DEV), [0, 64]).cpu()
    assert got.tolist() == [[64 * 2.0 ** -252, 2.0 ** -126, 0.0]]
    x[10], x[11] = -(2.0 ** 60), NAN
    got = ops.segment_stats(x.to(DEV), [0, 64]).cpu()
    assert got.tolist() == [[2.0 ** 120, 2.0 ** 60, 1.0]]
    S.check(got, x, [0, 64])


def test_the_segments_of_a_real_field_layout(ops):
    layout = ops.FieldLayout(3, 8, True, 12)
    sb = ops.SegmentBounds.of_layout(layout, DEV)
    assert sb.k == len(layout.entries) == 22 and sb.names == list(layout.entries) and sb.values[-1] == layout.total
    assert any(off % 4 == 0 and off % 8 != 0 for off, _ in layout.entries.values())
    x = _values(layout.total, seed=7)
    x[layout.offset("endmembers") + 5] = NAN
    x[layout.offset("mlp_head.layers.1.bias")] = -INF
    xd = x.to(DEV)
    got = ops.segment_stats(xd, sb)
    S.check(got, x, sb.values, "layout")
    counts = dict(zip(sb.names, got[:, 2].tolist()))
    assert counts["endmembers"] == 1.0 and counts["mlp_head.layers.1.bias"] == 1.0 and sum(counts.values()) == 2.0
    # a view that starts 8 bytes into an allocation: the buffer itself is not 16-byte aligned
    shifted = torch.cat([torch.full((2,), NAN), x]).to(DEV)[2:]
    assert shifted.data_ptr() % 16 == 8
    S.check(ops.segment_stats(shifted, sb), x, sb.values, "shifted")
    out = torch.full((sb.k, 3), -1.0, dtype=torch.float64, device=DEV)
    assert ops.segment_stats(xd, sb, out=out) is out and torch.equal(out, got)


def test_bad_bounds_raise_the_library_error_instead_of_reading(ops):
    x = torch.ones(100, device=DEV)
    for bad in ([0, 60, 50], [0, 50, 101], [-1, 50, 100]):
        with pytest.raises(RuntimeError, match="umhs_segment_stats failed: invalid argument"):
            ops.segment_stats(x, bad)
    with pytest.raises(ValueError):
        ops.segment_stats(x, [0])
    with pytest.raises(ValueError):
        ops.segment_stats(x.double(), [0, 100])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.segment_stats(torch.ones(4), [0, 4])
    assert ops.segment_stats(x, [0, 50, 100]).cpu().tolist() == [[50.0, 1.0, 0.0], [50.0, 1.0, 0.0]]
    assert ops.segment_stats(x[:0], [0, 0]).cpu().tolist() == [[0.0, 0.0, 0.0]]  # an empty buffer: one empty segment
    assert math.isfinite(float(ops.segment_stats(x, [100, 100])[0, 0]))
