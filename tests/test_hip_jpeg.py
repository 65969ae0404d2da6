"""``umhs_jpeg_*`` / ``ops.jpeg_*`` on the GPU against the restatement of the format in tests/jpeg_ref.py.  Per case: (a) the
coefficients equal the numpy float32 restatement exactly, (b) the whole file equals the reference encoder's bytes exactly, (c) PIL
decodes it.  The result is integers and bytes: every comparison is equality.

Shapes are the smallest at which each mechanism can break: 8 x 8 and 16 x 16 (one block, one MCU), 37 x 53 (partial MCUs on both axes,
35 MCUs at 4:4:4: R = 1, R = 3 -- 12 intervals, RSTm wraps past 7, the last one short --, R = 100 -- one interval, no RST), the render
test's 20 x 196 seven-panel frame, also as a view 1 and 3 bytes into a larger buffer, and 72 x 200 noise (225 MCUs: with R = 100 an
interval of 300 blocks runs through five 64-block chunks of its wavefront, with bits carried between them)."""
import io

import numpy as np
import pytest
import torch

import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5


def _smooth(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([128 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0), 2 * yy + 3 * xx, 255 * ((xx // 9 + yy // 5) % 2)], -1).clip(0, 255).astype(np.uint8)


def _noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _checker(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((255 * ((xx + yy) % 2)).astype(np.uint8)[..., None], 3, axis=2)


FRAMES = {"smooth8": lambda: _smooth(8, 8), "smooth16": lambda: _smooth(16, 16), "smooth": lambda: _smooth(37, 53),
          "panels": lambda: _smooth(20, 196), "grey": lambda: np.full((37, 53, 3), 128, np.uint8), "checker": lambda: _checker(37, 53),
          "noise": lambda: _noise(37, 53), "noise_long": lambda: _noise(72, 200, 1)}
# (frame, quality, subsampling, restart_mcus, byte offset of the frame in its buffer)
CASES = [("smooth8", 90, "444", 1, 0), ("smooth8", 90, "420", 1, 0), ("smooth16", 90, "444", 2, 0), ("smooth16", 50, "420", 1, 0),
         ("smooth", 90, "444", 4, 0), ("smooth", 90, "420", 4, 0), ("smooth", 25, "420", 2, 0), ("smooth", 1, "444", 4, 0),
         ("panels", 90, "420", 4, 0), ("panels", 90, "420", 4, 1), ("panels", 100, "444", 16, 3),
         ("smooth", 90, "444", 1, 0), ("smooth", 90, "444", 3, 0), ("smooth", 90, "444", 100, 0),
         ("grey", 90, "444", 3, 0), ("grey", 90, "420", 1, 0), ("checker", 100, "444", 3, 0), ("checker", 100, "420", 2, 0),
         ("noise", 100, "444", 1, 0), ("noise", 100, "420", 3, 0), ("noise_long", 100, "444", 100, 0), ("noise_long", 100, "420", 7, 0)]
_ref_cache = {}


def _reference(name, quality, ss, R):
    key = (name, quality, ss, R)
    if key not in _ref_cache:
        frame = FRAMES[name]()
        coefs = J.coefficients(frame, quality, ss)
        _ref_cache[key] = (frame, coefs, J.encode_coefficients(coefs, frame.shape[0], frame.shape[1], quality, ss, R))
    return _ref_cache[key]


def _device_frame(frame, offset):
    buf = torch.zeros(frame.size + 32, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + frame.size].view(frame.shape)
    view.copy_(torch.from_numpy(frame))
    assert view.data_ptr() % 16 == offset
    return view


def _file(out, length):
    n = int(length.item())
    assert n <= out.numel()
    return out[:n].cpu().numpy().tobytes()


@pytest.mark.parametrize("name,quality,ss,R,offset", CASES)
def test_coefficients_file_and_decode(name, quality, ss, R, offset):
    from PIL import Image, JpegImagePlugin

    from umhsnerf import ops

    frame, coefs, expect = _reference(name, quality, ss, R)
    H, W, _ = frame.shape
    dframe = _device_frame(frame, offset)
    got = ops.jpeg_coefficients(dframe, quality, ss).cpu().numpy()
    assert got.shape == coefs.shape and np.array_equal(got, coefs), f"{(got != coefs).sum()} coefficients differ"      # (a)
    data = _file(*ops.jpeg_encode(dframe, quality, ss, R))
    assert len(data) <= ops.jpeg_max_bytes(H, W, ss, R)
    assert data == expect, f"{len(data)} bytes against {len(expect)}"                                                      # (b)
    image = Image.open(io.BytesIO(data))
    image.load()                                                                                                            # (c)
    assert image.size == (W, H) and JpegImagePlugin.get_sampling(image) == (0 if ss == "444" else 2)
    assert data == _file(*ops.jpeg_encode(dframe, quality, ss, R)), "a second call wrote other bytes"


def test_reference_streams_hold_stuffed_bytes_inside_and_at_the_end_of_an_interval():
    """The seed of ``noise`` was picked on the CPU for this: at 4:4:4, quality 100, R = 1 its stream has 0xFF data bytes inside
    intervals, and at least one interval whose LAST byte is an 0xFF that the 1-padding completed.  (The case above compares it.)"""
    _, coefs, _ = _reference("noise", 100, "444", 1)
    inside = padded = 0
    for m in range(coefs.shape[0]):
        bits, n = J.interval_bits(coefs, m, m + 1, "444")
        raw = J.interval_bytes(coefs, m, m + 1, "444", stuffed=False)
        inside += b"\xff" in raw[:-1]
        padded += n % 8 != 0 and raw[-1] == 0xFF
    assert inside > 0 and padded > 0


def _zrl_coefficients(ss):
    """Hand-made blocks: a lone coefficient 63 (three ZRL and no EOB), runs of 16, 17, 31 and 32 zeros, a full block of +-1023, DC at
    both clamps (differences of +-2047: category 11), and an all-zero block."""
    bpm = 6 if ss == "420" else 3
    H, W = (32, 48) if ss == "420" else (16, 24)  # 6 MCUs
    k = np.zeros((6, bpm, 64), np.int16)
    k[0, 0, 63] = 5
    k[0, 1, 0], k[0, 1, 17] = -3, -1
    k[1, 0, 0], k[1, 0, 18], k[1, 0, 50], k[1, 0, 63] = 1023, 7, -300, -1023
    k[1, bpm - 1, 32], k[1, bpm - 1, 33] = 1, -1
    k[2, :, :] = 1023
    k[2, :, 1::2] = -1023
    k[2, 0, 0] = -1024
    k[3, 0, 0], k[3, bpm - 2, 0], k[3, bpm - 1, 0] = 1023, -1024, 1023
    k[4, 0, 16], k[4, 0, 48] = 2, 2
    k[5, bpm - 1, 63] = -1
    return k, H, W


@pytest.mark.parametrize("ss,R", [("444", 1), ("444", 4), ("420", 2), ("420", 65535)])
def test_entropy_stage_on_hand_made_coefficients(ss, R):
    from PIL import Image

    from umhsnerf import ops

    k, H, W = _zrl_coefficients(ss)
    expect = J.encode_coefficients(k, H, W, 100, ss, R)
    data = _file(*ops.jpeg_entropy(torch.from_numpy(k).to(DEV), H, W, 100, ss, R))
    assert data == expect
    Image.open(io.BytesIO(data)).load()


@pytest.mark.parametrize("ss", ["444", "420"])
def test_longest_streams_stay_inside_the_bounds(ss):
    """Blocks of alternating +-1023 with DC swinging between the clamps: every AC symbol is run 0 / size 10 (a 16-bit code at 4:4:4
    luminance), so every block is at the 1,660 bits the bound is made of, minus what shorter chrominance codes save."""
    from umhsnerf import ops

    H, W = (32, 64) if ss == "420" else (16, 64)
    bpm, n = (6, 8) if ss == "420" else (3, 16)
    k = np.full((n, bpm, 64), 1023, np.int16)
    k[:, :, 1::2] = -1023
    k[0::2, :, 0], k[1::2, :, 0] = -1024, 1023
    for R in (1, 5):
        expect = J.encode_coefficients(k, H, W, 100, ss, R)
        assert len(expect) <= ops.jpeg_max_bytes(H, W, ss, R)
        assert _file(*ops.jpeg_entropy(torch.from_numpy(k).to(DEV), H, W, 100, ss, R)) == expect
    assert ops.jpeg_workspace_bytes(H, W, ss, 5) >= 128 * n * bpm + 8 * ((n + 4) // 5)


def test_capacity_one_byte_short_leaves_the_tail_alone_and_names_the_size():
    from umhsnerf import ops

    frame, _, expect = _reference("noise", 100, "444", 3)
    dframe = _device_frame(frame, 0)
    for short in (1, 700, len(expect) - 100):
        cap = len(expect) - short
        buf = torch.full((len(expect) + 64,), CANARY, dtype=torch.uint8, device=DEV)
        out, length = ops.jpeg_encode(dframe, 100, "444", 3, out=buf[:cap])
        assert int(length.item()) == len(expect)
        host = buf.cpu().numpy()
        assert (host[cap:] == CANARY).all(), "bytes past the capacity were written"
        assert host[:cap].tobytes() == expect[:cap]


@pytest.mark.parametrize("name,quality,ss", [("smooth", 90, "444"), ("smooth", 90, "420"), ("noise", 100, "444"), ("noise", 100, "420")])
def test_coefficients_against_float64(name, quality, ss):
    """Fewer than 1 % of the float64 values lie in the tie band (jpeg_ref.tie_band: derived, not tuned); the GPU's coefficients equal
    the float64 ones outside it and are within 1/2 + the band of the float64 v everywhere (where no clamp acts)."""
    from umhsnerf import ops

    frame = FRAMES[name]()
    k64, v64 = J.coefficients(frame, quality, ss, np.float64, with_v=True)
    band = J.tie_band(quality, ss)[None]
    tie = J.in_tie_band(v64, band)
    assert tie.mean() < 0.01
    got = ops.jpeg_coefficients(_device_frame(frame, 0), quality, ss).cpu().numpy()
    assert np.array_equal(got[~tie], k64[~tie])
    free = np.abs(v64) < 1023
    assert (np.abs(got - v64)[free] <= 0.5 + np.broadcast_to(band, v64.shape)[free]).all()


def test_arguments():
    import ctypes

    from umhsnerf import _hip, ops

    lib, d = _hip.lib(), ctypes.c_void_p(4096)  # never dereferenced: every call below returns from its argument checks
    assert lib.umhs_jpeg_encode(None, 8, 8, 90, 0, 1, d, 100, d, d, 1 << 20, None) == -1
    assert lib.umhs_jpeg_encode(d, 8, 65536, 90, 0, 1, d, 100, d, d, 1 << 20, None) == -2
    assert lib.umhs_jpeg_encode(d, 8, 8, 101, 0, 1, d, 100, d, d, 1 << 20, None) == -1
    assert lib.umhs_jpeg_encode(d, 8, 8, 90, 2, 1, d, 100, d, d, 1 << 20, None) == -1
    assert lib.umhs_jpeg_encode(d, 8, 8, 90, 0, 65536, d, 100, d, d, 1 << 20, None) == -2
    assert lib.umhs_jpeg_encode(d, 8, 8, 90, 0, 1, d, 100, d, d, 8, None) == -3
    with pytest.raises(ValueError, match="no CPU path"):
        ops.jpeg_encode(torch.zeros(8, 8, 3, dtype=torch.uint8))
