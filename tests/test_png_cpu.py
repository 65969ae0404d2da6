"""The PNG stream on the host: tests/png_ref.py is what the GPU tests hold ``umhs_png_*`` to, so it is held to ``zlib`` (inflate,
CRC-32, Adler-32) and PIL (the decoder) here, and its size to PIL's encoder and to zlib's own ``Z_RLE``; then the argument checks of
``ops.png_*`` and the command line.  No GPU, and never the kernel."""
import io
import zlib

import numpy as np
import pytest

import png_ref as P

SHAPES = [(1, 1, 3), (1, 1, 1), (3, 5, 3), (17, 33, 3), (40, 87, 1), (64, 96, 3)]


def _frame(content, shape):
    H, W, C = shape
    yy, xx = np.mgrid[0:H, 0:W]
    if content == "smooth":
        f = np.stack([128 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0), 2 * yy + 3 * xx, 255 - 2 * xx - yy], -1)[..., :C]
    elif content == "noise":
        f = np.random.default_rng(H * 1000 + W).integers(0, 256, shape)
    elif content == "checker":
        f = np.repeat((255 * ((xx // 3 + yy // 2) % 2))[..., None], C, axis=2)
    else:
        f = np.full(shape, 77)
    return np.ascontiguousarray(np.clip(f, 0, 255).astype(np.uint8))


def _check(frame, filt, rows):
    from PIL import Image

    data = P.encode(frame, filt, rows)
    filtered = P.filter_rows(frame, filt)
    chunks = P.parse_chunks(data)  # (every CRC against zlib.crc32)
    assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * -(-frame.shape[0] // rows) + [b"IEND"]
    assert zlib.decompress(P.idat_payload(data)) == filtered.tobytes()  # (zlib checks the Adler-32)
    image = Image.open(io.BytesIO(data))
    assert image.mode == ("RGB" if frame.shape[2] == 3 else "L") and image.size == (frame.shape[1], frame.shape[0])
    assert np.array_equal(np.asarray(image).reshape(frame.shape), frame)
    return data


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("content", ["smooth", "noise", "checker", "constant"])
def test_reference_files_inflate_and_decode(content, shape):
    frame = _frame(content, shape)
    for rows in (1, 4, 16, 100):
        _check(frame, "adaptive", rows)
    for filt in ("none", "sub", "up", "average", "paeth"):
        data = _check(frame, filt, 4)
        assert set(P.filter_rows(frame, filt)[:, 0]) == {P.FILTERS[filt]}
        assert data[:8] == P.SIGNATURE


def test_run_tokens():
    """A run of n bytes: a literal, matches of 258 while three or more bytes are left, then up to two literals."""
    shape = lambda n: [(k, v) if k == "len" else k for k, v in P.tokens(bytes([5]) * n)]
    assert shape(1) == ["lit"] and shape(2) == ["lit"] * 2 and shape(3) == ["lit"] * 3
    assert shape(4) == ["lit", ("len", 3)] and shape(259) == ["lit", ("len", 258)]
    assert shape(260) == ["lit", ("len", 258), "lit"] and shape(261) == ["lit", ("len", 258), "lit", "lit"]
    assert shape(262) == ["lit", ("len", 258), ("len", 3)] and shape(517) == ["lit", ("len", 258), ("len", 258)]
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    for n in range(3, 259):  # RFC 1951's table
        sym, e, x = P.length_symbol(n)
        k = max(i for i in range(29) if base[i] <= n) if n < 258 else 28
        assert (sym, e, x) == (257 + k, extra[k], n - base[k])


def _fibonacci_piece():
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    flat = np.repeat(np.arange(24, dtype=np.uint8) * 3, fib)
    np.random.default_rng(5).shuffle(flat)
    return flat.reshape(281, 432)


def test_length_limit_and_bounds():
    """Fibonacci counts make the unlimited tree deeper than 15; the limited lengths are a complete code (``code_lengths`` asserts the
    Kraft equality), zlib inflates the piece, and the file stays under ``ops.png_max_bytes`` -- as does noise, deflate's worst case."""
    from umhsnerf import ops

    filtered = _fibonacci_piece()
    hist = P.histogram(P.tokens(filtered.tobytes()))
    _, per_depth = P.huffman_depth_counts(hist)
    assert max(per_depth) > 15
    lengths = P.code_lengths(hist)
    assert max(lengths) == 15 and sum(1 << (15 - l) for l in lengths if l) == 1 << 15
    data = P.encode_filtered(filtered, 431, 1, 281)
    assert zlib.decompress(P.idat_payload(data)) == filtered.tobytes()
    assert len(data) <= ops.png_max_bytes(281, 431, 1, 281)
    for shape, rows in (((64, 96, 3), 1), ((64, 96, 3), 16), ((40, 87, 1), 100)):
        noise = _frame("noise", shape)
        assert len(P.encode(noise, "none", rows)) <= ops.png_max_bytes(*shape, rows)
        assert len(P.encode(noise, "adaptive", rows)) <= ops.png_max_bytes(*shape, rows)
    assert ops.png_workspace_bytes(64, 96, 3, 16) >= 64 * 289 + 4 * 1184
    assert ops.png_max_bytes(65535, 65535, 3, 65535) == 0 and ops.png_max_bytes(65535, 65535, 3, 1) > 0  # a chunk stays below 2^31


# ---- size ----------------------------------------------------------------------------------------------------------------------------
def _size_frames():
    H, W = 360, 640
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(xx / 37.0) * np.cos(yy / 29.0), 0.3 * yy + 0.2 * xx, 128 + 90 * np.cos((xx + yy) / 53.0)], -1)
    noisy = (base + np.random.default_rng(1).normal(0, 6, base.shape)).clip(0, 255).astype(np.uint8)
    flat = noisy.copy()
    flat[((xx - 320) ** 2 / 200 ** 2 + (yy - 180) ** 2 / 120 ** 2) > 1] = 255
    colours = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200]], np.uint8)
    return {"noisy": noisy, "flat": flat, "label": colours[((xx // 80) + (yy // 60)) % 4]}


# measured png_ref / zlib Z_RLE level 9 (one raw stream over all filtered bytes), at 360 x 640 and 16-row pieces
RLE_RATIO = {"noisy": 1.00548, "flat": 1.01701, "label": 3.64802}


def test_sizes_against_pil_and_z_rle():
    """At 360 x 640, adaptive filter, 16-row pieces (23 pieces): a render-like noisy frame is 434,708 bytes against PIL's default PNG
    of 449,204 (0.968) and Z_RLE level 9's 432,339 (1.0055); the same frame over a flat background 151,755 against 152,925 (0.992) and
    149,218 (1.0170); a label frame of 80 x 60 blocks in four colours 5,410 bytes, 0.78 % of its 691,200 raw bytes, against Z_RLE's
    1,483 (3.648: 23 block headers, chunks and sync blocks are most of it) -- PIL's, with real LZ77 matches, is 1,666.  The Z_RLE ratios
    are asserted at the measured value x 1.02, so that a change of the length rule cannot quietly lose ratio."""
    from PIL import Image

    for name, frame in _size_frames().items():
        ours = len(P.encode(frame, "adaptive", 16))
        pil = io.BytesIO()
        Image.fromarray(frame).save(pil, "PNG")
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        rle = len(c.compress(P.filter_rows(frame).tobytes()) + c.flush())
        print(f"{name}: {ours} bytes, PIL {len(pil.getvalue())} ({ours / len(pil.getvalue()):.4f}), Z_RLE 9 {rle} ({ours / rle:.5f}), "
              f"{100 * ours / frame.size:.3f} % of raw")
        if name == "label":
            assert ours < 0.01 * frame.size
        else:
            assert ours <= 1.05 * len(pil.getvalue())
        assert ours / rle <= RLE_RATIO[name] * 1.02


# ---- arguments and the command line --------------------------------------------------------------------------------------------------
def test_ops_argument_errors():
    import torch

    from umhsnerf import ops

    assert ops.png_default_stripe_rows(8960, 3) == 2 and ops.png_default_stripe_rows(1280, 3) == 9 and ops.png_default_stripe_rows(1, 1) == 16384
    assert ops.png_default_stripe_rows(65535, 3) == 1
    assert 8 * (1 + 3 * 1280) < ops.PNG_PIECE_TARGET_BYTES <= 9 * (1 + 3 * 1280)  # the fewest rows that reach 32 KiB
    assert ops._png_params("paeth", 7) == (4, 7) and ops._png_params()[0] == 5
    with pytest.raises(ValueError, match="filter must be one of"):
        ops._png_params("best", 4)
    for bad in (0, 65536, -3):
        with pytest.raises(ValueError, match="stripe_rows must be 1..65535"):
            ops._png_params("adaptive", bad)
    with pytest.raises(ValueError, match="channels"):
        ops.png_max_bytes(8, 8, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.png_encode(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.png_filter(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.png_deflate(torch.zeros(8, 25, dtype=torch.uint8), 8)


def test_render_functions_refuse_bad_png_arguments_before_anything_is_rendered(tmp_path):
    from umhsnerf import export
    from umhsnerf.render import render_camera_path, render_dataset

    with pytest.raises(ValueError, match="png_encoder must be host or gpu"):
        render_camera_path(None, None, tmp_path / "out", ["rgb"], png_encoder="device")
    with pytest.raises(ValueError, match="image_format='png'"):
        render_camera_path(None, None, tmp_path / "out", ["rgb"], image_format="jpeg", png_encoder="gpu")
    with pytest.raises(ValueError, match="image_format='png'"):
        render_camera_path(None, None, tmp_path / "x.avi", ["rgb"], output_format="video", png_encoder="gpu")
    with pytest.raises(ValueError, match="image_format='png'"):
        render_dataset(None, ["test"], tmp_path / "out", ["rgb"], image_format="jpeg", png_encoder="gpu")
    with pytest.raises(ValueError, match="stripe_rows must be 1..65535"):
        render_dataset(None, ["test"], tmp_path / "out", ["rgb"], png_encoder="gpu", png_stripe_rows=0)
    with pytest.raises(ValueError, match="png_encoder must be host or gpu"):
        export.export_textured_mesh(None, tmp_path / "out", png_encoder="device")


BASE = ["camera-path", "--data", "scene", "--checkpoint", "c.ckpt", "--camera-path-filename", "p.json"]


def test_cli_png_flags(capsys):
    from umhsnerf import export
    from umhsnerf.render import parse_args

    args = parse_args(BASE + ["--output-path", "out"])  # the defaults are the host encoder
    assert (args.image_format, args.png_encoder, args.png_stripe_rows) == ("png", "host", None)
    args = parse_args(BASE + ["--output-path", "out", "--png-encoder", "gpu", "--png-stripe-rows", "8"])
    assert (args.png_encoder, args.png_stripe_rows) == ("gpu", 8)
    for more in (["--image-format", "jpeg"], ["--output-format", "video", "--output-path", "x.avi"]):
        with pytest.raises(SystemExit) as e:
            parse_args(BASE + ["--output-path", "out", "--png-encoder", "gpu"] + more)
        assert e.value.code != 0 and "--png-encoder gpu encodes PNG" in capsys.readouterr().err
    for bad in ("0", "65536"):
        with pytest.raises(SystemExit):
            parse_args(BASE + ["--output-path", "out", "--png-encoder", "gpu", "--png-stripe-rows", bad])
        assert "--png-stripe-rows must be 1..65535" in capsys.readouterr().err
    for command in (["dataset"], ["interpolate"]):
        a = parse_args(command + ["--data", "scene", "--checkpoint", "c.ckpt", "--output-path", "out", "--png-encoder", "gpu"])
        assert a.png_encoder == "gpu" and a.png_stripe_rows is None
    tm = ["textured-mesh", "--data", "scene", "--checkpoint", "c.ckpt", "--output-dir", "out"]
    assert not hasattr(export.parse_args(tm), "png_encoder")  # (absent unless given: the host encoder)
    assert export.parse_args(tm + ["--png-encoder", "gpu"]).png_encoder == "gpu" and export.parse_args(tm + ["--png-encoder", "host"]).png_encoder == "host"
    with pytest.raises(SystemExit):
        export.parse_args(tm + ["--png-encoder", "fast"])
