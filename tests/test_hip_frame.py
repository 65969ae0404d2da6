"""``umhs_frame_compose`` / ``ops.frame_compose`` on the GPU against the numpy float32 restatement (tests/frame_ref.py).  The result is
bytes and the arithmetic is fixed to the bit, so every comparison is ``np.array_equal``: no tolerance, nothing left out.

Sizes are the smallest that can break the store path (every panel's part of a frame row is written as aligned 16-byte words, in
windows of at most 752 bytes, with dwords and bytes only at its two ends): 1 / 3 / 15 pixels, a wave's width and one either side, a
frame whose rows are no multiple of 4 or 16 bytes, the test scene's 24 x 32, 256 x 256 with 16 panels (two windows per row), and
1024 x 1031 -- 5,120 windows for a grid capped at 1,024 workgroups.  The values hold every
k / 255 and (k + 0.5) / 255 with both float neighbours, values outside [0, 1], NaN and +-inf (also inverted), lo == hi ranges, and
accumulation of exactly 0 and 1 (frame_ref.special_values / make_panel)."""
import numpy as np
import pytest
import torch

import frame_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5


def _lut(name="turbo"):
    from umhsnerf.utils import colormaps

    return colormaps.table(name)


def _offset_tensor(array, off_floats):
    """``array`` on the device, ``off_floats`` * 4 bytes off a 16-byte boundary."""
    flat = torch.empty(array.size + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    t = flat[off_floats:off_floats + array.size].view(array.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(array)))
    assert t.data_ptr() % 16 == 4 * off_floats
    return t


def _device_panels(case, src_off=0):
    """ops.FramePanel list of a frame_ref case.  Even panels hand over a real column view (``rows[:, 7]``, ``rows[:, 1:4]``), odd ones
    the rows and a channel.  ``src_off``: panel k's sources sit 4 * ((src_off + k) % 4) bytes off a 16-byte boundary."""
    from umhsnerf import ops

    panels = []
    for k, p in enumerate(case):
        off = (src_off + k) % 4 if src_off else 0
        rows, ch = _offset_tensor(p["rows"], off), p["channel"]
        if k % 2 == 0:
            src, ch = (rows[:, ch:ch + 3] if p["kind"] == R.RGB else rows[:, ch]), 0
            assert src.data_ptr() == rows.data_ptr() + 4 * p["channel"]  # a view: nothing was copied
        else:
            src = rows
        panels.append(ops.FramePanel(src, p["kind"], ch, None if p["range"] is None else _offset_tensor(p["range"], off),
                                     None if p["acc"] is None else _offset_tensor(p["acc"], off), p["normalize"], p["invert"],
                                     p["cmin"], p["cmax"]))
    return panels


def _run(case, H, W, lut, frame_off=None, src_off=0):
    from umhsnerf import ops

    dlut = torch.from_numpy(lut.copy()).to(DEV)
    panels = _device_panels(case, src_off)
    if frame_off is None:
        out = ops.frame_compose(panels, dlut, H, W)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (H, len(case) * W, 3)
        return out.cpu().numpy()
    nbytes = 3 * H * W * len(case)
    buf = torch.full((nbytes + 48,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    begin = 16 + frame_off
    out = ops.frame_compose(panels, dlut, H, W, out=buf[begin:begin + nbytes])
    assert out.data_ptr() == buf.data_ptr() + begin
    host = buf.cpu().numpy()
    assert (host[:begin] == SENTINEL).all() and (host[begin + nbytes:] == SENTINEL).all(), "bytes outside the frame were written"
    return host[begin:begin + nbytes].reshape(H, len(case) * W, 3)


SIZES = [(1, 1, 3), (1, 3, 3), (3, 5, 3), (2, 63, 3), (2, 64, 3), (2, 65, 3), (37, 29, 3), (24, 32, 3), (256, 256, 16), (1024, 1031, 1)]


@pytest.mark.parametrize("H,W,K", SIZES)
def test_sizes(H, W, K):
    case = R.make_case(H, W, K, seed=1, first_variant=(H + W) % 8 if K < 8 else 0)
    lut = _lut()
    assert np.array_equal(_run(case, H, W, lut), R.compose(case, lut, H, W))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 16])
def test_panel_sets(K):
    H, W = 37, 29
    case = R.make_case(H, W, K, seed=2, first_variant=K)
    assert {p["kind"] for p in R.make_case(H, W, 16, seed=2)} == {R.RGB, R.SCALAR, R.DEPTH}
    lut = _lut("viridis" if K % 2 else "turbo")
    assert np.array_equal(_run(case, H, W, lut), R.compose(case, lut, H, W))


def test_every_special_value_through_every_panel_variant():
    H, W = 64, 64  # 4,096 pixels hold all ~1,550 special values in every panel
    assert H * W >= len(R.special_values())
    for first in (0, 4):
        case = R.make_case(H, W, 4, seed=3, first_variant=first)
        for p in case:
            col = p["rows"][:, p["channel"]:p["channel"] + (3 if p["kind"] == R.RGB else 1)]
            assert np.isnan(col).any() and np.isinf(col).any()
        for name in ("turbo", "gray"):
            lut = _lut(name)
            assert np.array_equal(_run(case, H, W, lut), R.compose(case, lut, H, W))


@pytest.mark.parametrize("frame_off", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("H,W", [(3, 5), (37, 29)])
def test_frame_and_sources_at_any_alignment(H, W, frame_off):
    case = R.make_case(H, W, 3, seed=4, first_variant=frame_off)
    lut = _lut()
    want = R.compose(case, lut, H, W)
    for src_off in (1, 2, 3):
        assert np.array_equal(_run(case, H, W, lut, frame_off=frame_off, src_off=src_off), want)


def test_a_frame_smaller_than_one_aligned_word():
    """1 x 1, one panel: 3 bytes that straddle or sit inside an aligned dword / 16-byte piece, neighbours untouched."""
    case = R.make_case(1, 1, 1, seed=5)
    lut = _lut()
    want = R.compose(case, lut, 1, 1)
    for frame_off in range(16):
        assert np.array_equal(_run(case, 1, 1, lut, frame_off=frame_off), want)


def test_wrapper_argument_errors():
    from umhsnerf import ops

    lut = torch.from_numpy(_lut().copy()).to(DEV)
    rgb = torch.rand(6, 3, device=DEV)
    ok = ops.FramePanel(rgb, ops.PANEL_RGB)
    assert tuple(ops.frame_compose([ok], lut, 2, 3).shape) == (2, 3, 3)
    with pytest.raises(ValueError, match="HIP device"):
        ops.frame_compose([ops.FramePanel(rgb.cpu(), ops.PANEL_RGB)], lut, 2, 3)
    with pytest.raises(ValueError, match="HIP device"):
        ops.frame_compose([ok], lut.cpu(), 2, 3)
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_compose([ok], lut, 2, 3, out=torch.empty(2, 3, 3, device=DEV))
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_compose([ok], lut, 2, 3, out=torch.empty(2, 3, 2, dtype=torch.uint8, device=DEV))  # wrong size
    with pytest.raises(ValueError, match="float32"):
        ops.frame_compose([ops.FramePanel(rgb.double(), ops.PANEL_RGB)], lut, 2, 3)
    with pytest.raises(ValueError, match="rows"):
        ops.frame_compose([ok], lut, 2, 4)  # 8 pixels from 6 rows
    with pytest.raises(ValueError, match="columns"):
        ops.frame_compose([ops.FramePanel(rgb, ops.PANEL_RGB, channel=1)], lut, 2, 3)
    with pytest.raises(ValueError, match="range"):
        ops.frame_compose([ops.FramePanel(rgb[:, 0], ops.PANEL_DEPTH)], lut, 2, 3)
    with pytest.raises(ValueError, match="panels"):
        ops.frame_compose([ok] * 17, lut, 2, 3)
    assert tuple(ops.frame_compose([ops.FramePanel(rgb[:0], ops.PANEL_RGB)], lut, 0, 3).shape) == (0, 3, 3)
