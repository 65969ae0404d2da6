"""The frame encoder's format on the host (tests/jpeg_ref.py is what the GPU tests hold ``umhs_jpeg_*`` to, so it is held to PIL /
libjpeg here), the Motion-JPEG writer, and the command line of ``--output-format video``.  No GPU."""
import io
import struct

import numpy as np
import pytest

import jpeg_ref as J


def _frame(H=37, W=53):
    """Smooth gradients plus hard edges."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([128 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0), 2 * yy + 3 * xx, 255 * ((xx // 9 + yy // 5) % 2)], -1).clip(0, 255).astype(np.uint8)


def _pil(frame, quality, ss):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[ss])
    return b.getvalue()


def _decode(data):
    from PIL import Image

    image = Image.open(io.BytesIO(data))
    image.load()
    return image


def _psnr(image, frame):
    return 10 * np.log10(255.0 ** 2 / np.mean((np.asarray(image, np.float64) - frame) ** 2))


@pytest.mark.parametrize("ss", ["444", "420"])
@pytest.mark.parametrize("quality", [1, 25, 50, 90, 100])
def test_reference_streams_decode_in_pil_with_its_tables(quality, ss):
    from PIL import JpegImagePlugin

    frame = _frame()
    theirs = _decode(_pil(frame, quality, ss))
    for R in (3, 100):
        image = _decode(J.encode(frame, quality, ss, R))
        assert image.size == (53, 37) and image.mode == "RGB"
        assert JpegImagePlugin.get_sampling(image) == JpegImagePlugin.get_sampling(theirs) == (0 if ss == "444" else 2)
        assert image.quantization == theirs.quantization and len(image.quantization) == 2
    luma, chroma = J.quant_tables(quality)
    assert luma.min() >= 1 and chroma.max() <= 255 and (quality > 1 or luma.max() == 255)  # the clamp acts at quality 1


@pytest.mark.parametrize("ss", ["444", "420"])
@pytest.mark.parametrize("quality", [50, 90, 100])
def test_decoded_psnr_is_within_a_tenth_of_a_decibel_of_pil(quality, ss):
    """Both encoders use the same tables, so the quantisation noise is the same; what differs is which way a coefficient near a tie
    is rounded, and that reaches the decoded error only through the decoder's own rounding and its clipping at 0 and 255.  0.1 dB is
    2.3 % of the mean squared error, so the frame is 240 x 320 (230,400 samples), not the 37 x 53 of the other tests: on those 5,883
    samples the same pattern measured -0.029 / +0.006 (quality 50, 4:4:4 / 4:2:0), -0.105 / +0.008 (90) and -0.039 / -0.002 (100) dB
    against PIL -- one case 0.005 dB past the margin --, here -0.025 / -0.004, -0.040 / -0.005, +0.073 / -0.004.  At quality 100 the
    difference is the decoder's rounding alone and depends on the content: the pattern without its cos(y / 5) factor measured -0.289
    dB at 4:4:4 and this size, one with softer edges +0.878."""
    frame = _frame(240, 320)
    a, b = _psnr(_decode(J.encode(frame, quality, ss, 1200)), frame), _psnr(_decode(_pil(frame, quality, ss)), frame)
    print(f"quality {quality} {ss}: PSNR {a:.3f} dB, PIL {b:.3f} dB")
    assert a >= b - 0.1


def test_header_layout():
    h = J.header(720, 8960, 90, "420", 16)
    assert len(h) == J.HEADER_BYTES == 629
    # SOI APP0 DQT DQT SOF0 DHT DHT DHT DHT DRI SOS, walked by their lengths
    p, seen = 2, [0xD8]
    while p < len(h):
        assert h[p] == 0xFF
        seen.append(h[p + 1])
        p += 2 + struct.unpack(">H", h[p + 2:p + 4])[0]
    assert seen == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA] and p == len(h)
    sof = h.index(b"\xff\xc0")
    assert struct.unpack(">BHHB", h[sof + 4:sof + 10]) == (8, 720, 8960, 3) and h[sof + 10:sof + 19] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    dri = h.index(b"\xff\xdd")
    assert struct.unpack(">HH", h[dri + 2:dri + 6]) == (4, 16)


@pytest.mark.parametrize("ss", ["444", "420"])
def test_float32_coefficients_differ_from_float64_only_inside_the_derived_tie_band(ss):
    bound = J.f64_bound(ss)
    assert 1e-4 < bound < 3e-3  # of the order 1e-3 for 8-bit input
    rng = np.random.default_rng(3)
    for quality, frame in ((90, _frame()), (100, _frame(40, 64)), (100, rng.integers(0, 256, (37, 53, 3), dtype=np.uint8))):
        k32, v32 = J.coefficients(frame, quality, ss, np.float32, with_v=True)
        k64, v64 = J.coefficients(frame, quality, ss, np.float64, with_v=True)
        Q = J.divisors(quality, ss)[None]
        worst = float(np.abs((v32.astype(np.float64) - v64) * Q).max())
        tie = J.in_tie_band(v64, J.tie_band(quality, ss)[None])
        print(f"quality {quality} {ss}: max |F32 - F64| {worst:.3e} (bound {bound:.3e}), {int((k32 != k64).sum())} coefficients differ, "
              f"{100 * tie.mean():.3f} % in the tie band")
        assert worst <= bound
        assert np.array_equal(k32[~tie], k64[~tie])
        assert tie.mean() < 0.01


def test_entropy_coder_edge_cases():
    """A lone coefficient 63 is three ZRL and no EOB; an all-zero block is DC 0 and EOB; the padding is 1-bits; 0xFF is stuffed."""
    k = np.zeros((1, 3, 64), np.int16)
    k[0, 0, 63] = 1
    bits, n = J.block_bits(k[0, 0], 0, False)
    zrl, dc0 = J.huff_codes(J.AC_LUMA_BITS, J.AC_LUMA_VALS)[0xF0], J.huff_codes(J.DC_LUMA_BITS, J.DC_VALS)[0]
    last = J.huff_codes(J.AC_LUMA_BITS, J.AC_LUMA_VALS)[0xE1]  # run 14 after 48 zeros, size 1
    assert n == dc0[1] + 3 * zrl[1] + last[1] + 1
    assert J.block_bits(np.zeros(64, np.int16), 0, True) == (0b0000, 4)  # chroma: DC category 0 is 00, EOB is 00
    raw = J.interval_bytes(k, 0, 1, "444", stuffed=False)
    _, total = J.interval_bits(k, 0, 1, "444")
    assert len(raw) == -(-total // 8) and (total % 8 == 0 or raw[-1] & ((1 << (-total % 8)) - 1) == (1 << (-total % 8)) - 1)
    noise = np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    data = J.encode(noise, 100, "444", 1)
    body = data[J.HEADER_BYTES:-2]
    assert b"\xff\x00" in body and all(body[i + 1] == 0 or 0xD0 <= body[i + 1] <= 0xD7 for i in range(len(body) - 1) if body[i] == 0xFF)
    assert [body[i + 1] - 0xD0 for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] != 0] == [m % 8 for m in range(34)]
    _decode(data)


# ---- the Motion-JPEG writer ----------------------------------------------------------------------------------------------------------
def _jpegs(n, W=24, H=16):
    rng = np.random.default_rng(5)
    out = [_pil(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 60 + 5 * i, "420") for i in range(n)]
    parity = lambda j, odd: j if len(j) % 2 == odd else j[:-2] + b"\x00\xff\xd9"  # (a fill byte in front of EOI)
    return [parity(j, i % 2) for i, j in enumerate(out)]  # frames of even and of odd length


def _check_avi(data, jpegs, W, H, rate, scale):
    chunks = J.riff_chunks(data)
    assert [c[0] for c in chunks] == ["RIFF:AVI "] and chunks[0][2] == len(data) - 8
    assert [c[0] for c in chunks[0][3]] == ["LIST:hdrl", "LIST:movi", "idx1"]
    hdrl = chunks[0][3][0]
    assert [c[0] for c in hdrl[3]] == ["avih", "LIST:strl"] and [c[0] for c in hdrl[3][1][3]] == ["strh", "strf"]
    avih, strh, strf = (J.riff_find(chunks, k) for k in ("avih", "strh", "strf"))
    assert (avih[2], strh[2], strf[2]) == (56, 56, 40)
    a = struct.unpack_from("<14I", data, avih[1])
    assert a[0] == round(1e6 * scale / rate) and a[3] & 0x10 and a[4] == len(jpegs) and a[6] == 1 and (a[8], a[9]) == (W, H)
    assert a[7] == max(map(len, jpegs), default=0)
    s = struct.unpack_from("<4s4sIHHIIIIIIII4H", data, strh[1])
    assert s[:2] == (b"vids", b"MJPG") and (s[6], s[7]) == (scale, rate) and s[9] == len(jpegs) and s[-2:] == (W, H)
    f = struct.unpack_from("<IiiHH4sIiiII", data, strf[1])
    assert f[:7] == (40, W, H, 1, 24, b"MJPG", W * H * 3)
    movi, idx1 = J.riff_find(chunks, "LIST:movi"), J.riff_find(chunks, "idx1")
    frames = movi[3]
    assert [c[0] for c in frames] == ["00dc"] * len(jpegs) and idx1[2] == 16 * len(jpegs)
    for i, (cc, off, size, _) in enumerate(frames):
        assert data[off:off + size] == jpegs[i]
        if size & 1:
            assert data[off + size] == 0  # the pad byte, not counted in the size
        entry = struct.unpack_from("<4sIII", data, idx1[1] + 16 * i)
        assert entry == (b"00dc", 0x10, off - 8 - movi[1], size)  # offsets count from the movi tag
        assert data[movi[1] + entry[2]:movi[1] + entry[2] + 4] == b"00dc"


def test_avi_writer_layout_padding_and_index(tmp_path):
    from umhsnerf.utils.mjpeg_avi import MjpegAviWriter, rate_scale

    jpegs = _jpegs(5)
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs)
    with MjpegAviWriter(tmp_path / "a.avi", 24, 16, 24) as w:
        for j in jpegs:
            w.add_frame(j)
    assert w.paths == [tmp_path / "a.avi"] and w.frames == 5
    _check_avi((tmp_path / "a.avi").read_bytes(), jpegs, 24, 16, 24, 1)
    assert rate_scale(29.97) == (2997, 100) and rate_scale(24) == (24, 1) and rate_scale(12.5) == (25, 2)
    from fractions import Fraction

    with MjpegAviWriter(tmp_path / "b.avi", 24, 16, Fraction(30000, 1001)) as w:
        w.add_frame(jpegs[0])
    _check_avi((tmp_path / "b.avi").read_bytes(), jpegs[:1], 24, 16, 30000, 1001)
    with pytest.raises(ValueError, match="NAME.avi"):
        MjpegAviWriter(tmp_path / "c.mp4", 24, 16)
    with pytest.raises(ValueError, match="SOI"):
        with MjpegAviWriter(tmp_path / "d.avi", 24, 16) as w:
            w.add_frame(b"not a jpeg")
    _check_avi((tmp_path / "d.avi").read_bytes(), [], 24, 16, 24, 1)  # an empty file is still a valid one


def test_avi_is_valid_after_an_exception(tmp_path):
    from umhsnerf.utils.mjpeg_avi import MjpegAviWriter

    jpegs = _jpegs(4)
    with pytest.raises(RuntimeError, match="the loop broke"):
        with MjpegAviWriter(tmp_path / "x.avi", 24, 16, 12.5) as w:
            for i, j in enumerate(jpegs):
                if i == 3:
                    raise RuntimeError("the loop broke")
                w.add_frame(j)
    _check_avi((tmp_path / "x.avi").read_bytes(), jpegs[:3], 24, 16, 25, 2)
    with pytest.raises(ValueError, match="closed"):
        w.add_frame(jpegs[0])


def test_avi_rolls_over_into_parts(tmp_path):
    from umhsnerf.utils.mjpeg_avi import MjpegAviWriter

    jpegs = _jpegs(9)
    limit = 224 + 2 * (max(map(len, jpegs)) + 9) + 8 + 16 * 2  # a few KB: two of the largest frames fit, never five
    with MjpegAviWriter(tmp_path / "fly.avi", 24, 16, 24, max_bytes=limit) as w:
        for j in jpegs:
            w.add_frame(j)
    assert len(w.paths) >= 3 and w.frames == 9
    assert [p.name for p in w.paths] == ["fly.avi"] + [f"fly_part{k:03d}.avi" for k in range(2, len(w.paths) + 1)]
    seen = 0
    for p in w.paths:
        data = p.read_bytes()
        assert len(data) <= limit
        n = len(J.riff_find(J.riff_chunks(data), "LIST:movi")[3])
        assert n >= 1
        _check_avi(data, jpegs[seen:seen + n], 24, 16, 24, 1)
        seen += n
    assert seen == 9


# ---- the command line ------------------------------------------------------------------------------------------------------------------
BASE = ["camera-path", "--data", "scene", "--checkpoint", "c.ckpt", "--camera-path-filename", "p.json"]


def test_cli_video_and_encoder_flags(capsys):
    from umhsnerf.render import parse_args

    args = parse_args(BASE + ["--output-path", "out"])  # the defaults are what they were
    assert (args.output_format, args.image_format, args.jpeg_quality, args.jpeg_encoder, args.jpeg_subsampling, args.restart_mcus) == (
        "images", "png", 100, "host", "420", None)
    args = parse_args(BASE + ["--output-path", "x.avi", "--output-format", "video", "--jpeg-quality", "90", "--jpeg-subsampling", "444",
                              "--restart-mcus", "8"])
    assert (args.output_format, args.output_path, args.jpeg_quality, args.jpeg_subsampling, args.restart_mcus) == ("video", "x.avi", 90, "444", 8)
    for bad in ("x.mp4", "out", "dir/"):
        with pytest.raises(SystemExit) as e:
            parse_args(BASE + ["--output-path", bad, "--output-format", "video"])
        err = capsys.readouterr().err
        assert e.value.code != 0 and "NAME.avi" in err and "ffmpeg -i NAME.avi" in err
    args = parse_args(BASE + ["--output-path", "out", "--image-format", "jpeg", "--jpeg-encoder", "gpu"])
    assert args.jpeg_encoder == "gpu"
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--output-path", "out", "--jpeg-encoder", "gpu"])  # png frames are not JPEG
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--output-path", "x.avi", "--output-format", "video", "--restart-mcus", "0"])
    ip = parse_args(["interpolate", "--data", "scene", "--checkpoint", "c.ckpt", "--output-path", "y.avi", "--output-format", "video"])
    assert ip.output_format == "video" and ip.restart_mcus is None
    ds = parse_args(["dataset", "--data", "scene", "--checkpoint", "c.ckpt", "--output-path", "out", "--image-format", "jpeg", "--jpeg-encoder", "gpu"])
    assert ds.jpeg_encoder == "gpu" and not hasattr(ds, "jpeg_subsampling") and not hasattr(ds, "output_format")


def test_path_fps():
    from umhsnerf.render import path_fps

    assert path_fps({"fps": 30, "seconds": 2, "num_frames": 10}) == 30
    assert path_fps({"fps": None, "seconds": 2.0, "num_frames": 10}) == 5
    assert path_fps({"fps": None, "seconds": None, "num_frames": 10}) == 24
