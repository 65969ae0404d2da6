"""CPU checks of tests/stats_f64.py: the float64 oracle of ``ops.segment_stats`` on hand-made inputs, the bound against the chain
length of the kernel's tiling, and the host-side argument checks of the entry point (nothing is launched)."""
import ctypes
import math

import torch

import stats_f64 as S

NAN, INF = float("nan"), float("inf")
DENORMAL = 2.0 ** -140  # a float32 subnormal; its square, 2^-280, is a normal float64


def test_oracle_on_hand_made_segments():
    x = torch.tensor([9.0,                                # outside the first segment
                      3.0, -4.0, NAN, INF, -INF, -0.0,    # [1, 7): 9 + 16, max 4, three non-finite
                      DENORMAL, -2.0 ** -126,             # [7, 9): two tiny squares
                      NAN,                                # [9, 10): nothing finite
                      -0.0, 0.0,                          # [10, 12) after an empty segment [10, 10): zeros
                      5.0], dtype=torch.float32)          # outside the last segment
    bounds = [1, 7, 9, 10, 10, 12]
    got = S.oracle(x, bounds)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5, 3)
    assert got[0].tolist() == [25.0, 4.0, 3.0]
    assert got[1].tolist() == [2.0 ** -280 + 2.0 ** -252, 2.0 ** -126, 0.0] and got[1, 0] > 2.0 ** -252  # the denormal's square is not lost
    assert got[2].tolist() == [0.0, 0.0, 1.0]
    assert got[3].tolist() == [0.0, 0.0, 0.0]  # empty
    assert got[4].tolist() == [0.0, 0.0, 0.0] and math.copysign(1.0, float(got[4, 1])) == 1.0  # |-0| is +0
    assert float(x[7]) == DENORMAL and DENORMAL < 2.0 ** -126  # the input really is subnormal in float32


def test_oracle_sum_is_the_correctly_rounded_exact_sum():
    """1 and 2^16 copies of 2^-30: squares 1 and 2^-60; a float64 running sum would drop every one of them, the exact sum does not."""
    x = torch.full((1 + (1 << 16),), 2.0 ** -30, dtype=torch.float32)
    x[0] = 1.0
    assert float(S.oracle(x, [0, x.numel()])[0, 0]) == 1.0 + 2.0 ** -44
    naive = 1.0
    for _ in range(1 << 16):
        naive += 2.0 ** -60
    assert naive == 1.0


def test_bound_is_what_the_chain_length_gives():
    assert S.TILE == 8192 and S.U == 2.0 ** -53
    # thread 34 + wave 6 + workgroup 3 + finish (ceil(tiles / 64) + 6)
    for length, tiles in ((0, 0), (1, 1), (8192, 1), (8193, 2), (64 * 8192, 64), (64 * 8192 + 1, 65), ((1 << 20) + 3, 129), (16 << 20, 2048)):
        assert S.chain_length(length) == 34 + 6 + 3 + -(-tiles // 64) + 6, length
    assert S.chain_length(1) == 50 and S.chain_length((1 << 20) + 3) == 52 and S.chain_length(16 << 20) == 81
    for length in (1, 8193, (1 << 20) + 3):
        d = S.chain_length(length)
        assert S.gamma(d) == d * S.U / (1 - d * S.U) and d * S.U <= S.gamma(d) <= d * S.U * (1 + 1e-12)
        want = (S.gamma(d) + S.gamma(1)) * 3.5 * (1 + S.gamma(1))
        assert S.sum_bound(length, 3.5) == want and (d + 1) * S.U * 3.5 <= want <= (d + 1.001) * S.U * 3.5
    assert S.sum_bound(100, 0.0) == 0.0  # all zeros (or nothing finite): the sum is exactly 0


def test_check_rejects_a_sum_one_step_outside_the_bound_and_any_other_maximum_or_count():
    import pytest

    x = torch.tensor([1.0, 2.0, 3.0, NAN], dtype=torch.float32)
    ref = S.oracle(x, [0, 4])
    assert ref.tolist() == [[14.0, 3.0, 1.0]]
    assert S.check(ref.clone(), x, [0, 4]) == 0.0
    near = ref.clone()
    near[0, 0] = 14.0 * (1 + 40 * S.U)  # inside: chain_length(4) = 50
    assert 0.5 < S.check(near, x, [0, 4]) <= 1.0
    for col, value in ((0, 14.0 * (1 + 64 * S.U)), (1, math.nextafter(3.0, 4.0)), (2, 2.0), (0, NAN)):
        bad = ref.clone()
        bad[0, col] = value
        with pytest.raises(AssertionError):
            S.check(bad, x, [0, 4])


def test_bad_bounds_are_argument_errors_before_anything_is_launched(built_library):
    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, WS = -1, -3
    assert lib.umhs_segment_stats_tile() == S.TILE
    d = ctypes.c_void_p(4096)  # never dereferenced
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    need = lib.umhs_segment_stats_workspace_bytes(100, 2)
    assert need == (1 + 2) * 24 and lib.umhs_segment_stats_workspace_bytes(8193, 1) == (2 + 1) * 24
    assert lib.umhs_segment_stats_workspace_bytes(-1, 1) == 0 and lib.umhs_segment_stats_workspace_bytes(10, 0) == 0
    call = lambda host, n=100, k=2, x=d, bounds=d, out=d, ws=d, wsb=need: lib.umhs_segment_stats(x, n, bounds, host, k, out, ws, wsb, None)
    assert call(i64(0, 60, 50)) == ARG  # descends
    assert call(i64(0, 50, 101)) == ARG  # ends beyond the buffer
    assert call(i64(-1, 50, 100)) == ARG
    assert call(i64(0, 50, 100), k=0) == ARG and call(i64(0, 50, 100), n=-1) == ARG
    assert call(None) == ARG and call(i64(0, 50, 100), bounds=None) == ARG and call(i64(0, 50, 100), out=None) == ARG
    assert call(i64(0, 50, 100), x=None) == ARG and call(i64(0, 50, 100), x=ctypes.c_void_p(4098)) == ARG
    assert call(i64(0, 50, 100), ws=None) == WS and call(i64(0, 50, 100), wsb=need - 1) == WS
