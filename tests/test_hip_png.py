"""``umhs_png_*`` / ``ops.png_*`` on the GPU against the restatement of the stream in tests/png_ref.py.  Per case: the filtered rows
equal the reference's, the whole file equals the reference encoder's bytes, and PIL decodes it to the frame.  Everything is integers
and bytes: every comparison is equality.

Shapes are the smallest at which each mechanism can break: one pixel; rows of 16, 88 and 100 bytes (not multiples of 4); pieces of 1, 4
and 16 rows and one larger than the frame; a 64 x 96 frame whose single piece of 18,496 bytes runs through five tiles of the
workgroup, as one run of zeros for the constant frame; the frame 0, 1 and 3 bytes into its allocation."""
import io
import zlib

import numpy as np
import pytest
import torch

import png_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
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
    elif content == "zeros":
        f = np.zeros(shape)
    else:
        f = np.full(shape, 77)
    return np.ascontiguousarray(np.clip(f, 0, 255).astype(np.uint8))


# (content, shape, filter, stripe_rows, byte offset of the frame in its buffer)
CASES = ([(c, s, "adaptive", 4, 0) for s in SHAPES for c in ("smooth", "noise")]
         + [(c, (64, 96, 3), "adaptive", 16, 0) for c in ("checker", "constant", "zeros")]
         + [("zeros", (64, 96, 3), "none", 100, 0), ("constant", (40, 87, 1), "none", 100, 0), ("checker", (17, 33, 3), "adaptive", 1, 0)]
         + [("smooth", (64, 96, 3), "adaptive", r, 0) for r in (1, 16, 100)]
         + [("noise", (64, 96, 3), "adaptive", r, 0) for r in (1, 16, 100)]
         + [("smooth", (17, 33, 3), "adaptive", 4, o) for o in (1, 3)] + [("noise", (40, 87, 1), "adaptive", 16, o) for o in (1, 3)]
         + [("smooth", (17, 33, 3), f, 4, 0) for f in ("none", "sub", "up", "average", "paeth")]
         + [("noise", (40, 87, 1), f, 16, 0) for f in ("none", "sub", "up", "average", "paeth")])
_ref_cache = {}


def _reference(content, shape, filt, rows):
    key = (content, shape, filt, rows)
    if key not in _ref_cache:
        frame = _frame(content, shape)
        _ref_cache[key] = (frame, P.filter_rows(frame, filt), P.encode(frame, filt, rows))
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


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return f"{len(a)} bytes against {len(b)}, first difference at {int(d[0]) if len(d) else n}"


@pytest.mark.parametrize("content,shape,filt,rows,offset", CASES)
def test_filtered_rows_file_and_decode(content, shape, filt, rows, offset):
    from PIL import Image

    from umhsnerf import ops

    frame, filtered, expect = _reference(content, shape, filt, rows)
    H, W, C = shape
    dframe = _device_frame(frame, offset)
    got = ops.png_filter(dframe, filt).cpu().numpy()
    assert got.shape == filtered.shape and np.array_equal(got, filtered), f"{(got != filtered).sum()} filtered bytes differ"
    data = _file(*ops.png_encode(dframe, filt, rows))
    assert len(data) <= ops.png_max_bytes(H, W, C, rows)
    assert data == expect, _first_difference(data, expect)
    assert zlib.decompress(P.idat_payload(data)) == filtered.tobytes()  # (the parser checks every CRC)
    image = np.asarray(Image.open(io.BytesIO(data)))
    assert np.array_equal(image.reshape(shape), frame)


def test_filter_choice_on_ties_and_on_residuals_of_128():
    """Row 0 of any frame: Up equals None and Paeth equals Sub (nothing above), so a row that Sub serves best ties 1 with 4 and a row
    that None serves best ties 0 with 2: the lower type wins.  A row that alternates 0 and 128 has Sub residuals of 128 everywhere,
    where min(f, 256 - f) is 128 from both sides."""
    from umhsnerf import ops

    ramp = (np.arange(40) * 5 % 256).astype(np.uint8)
    flat = np.zeros(40, np.uint8)
    flat[::7] = 1
    alt = (128 * (np.arange(40) % 2)).astype(np.uint8)
    for C in (1, 3):
        frame = np.repeat(np.stack([ramp, flat, alt, alt, ramp])[..., None], C, axis=2)
        ref = P.filter_rows(frame)
        costs = P.filter_costs(P.filter_candidates(frame))
        assert ref[0, 0] == 1 and costs[1, 0] == costs[4, 0] and costs[1, 0] < costs[0, 0]      # Sub ties Paeth
        assert ref[1, 0] == 0 or costs[0, 1] > costs[int(ref[1, 0]), 1]
        sub = P.filter_candidates(frame)[1, 2, C:]
        assert (sub == 128).all()
        got = ops.png_filter(torch.from_numpy(frame).to(DEV)).cpu().numpy()
        assert np.array_equal(got, ref)
    top = np.repeat(flat[None, :, None], 3, axis=2)  # one row, best left alone: None ties Up
    costs = P.filter_costs(P.filter_candidates(top))
    assert costs[0, 0] == costs[2, 0] == costs.min() and P.filter_rows(top)[0, 0] == 0
    assert np.array_equal(ops.png_filter(torch.from_numpy(top).to(DEV)).cpu().numpy(), P.filter_rows(top))


# ---- stage B on hand-made filtered bytes ---------------------------------------------------------------------------------------------
def _rows(flat, row):
    """uint8 [H, row]: ``flat`` padded to whole rows with bytes that differ from their neighbours."""
    flat = np.asarray(flat, np.uint8)
    pad = (-len(flat)) % row
    tail = (np.arange(pad) % 2 * 3 + 250).astype(np.uint8)  # 250 253 250 ..
    return np.concatenate([flat, tail]).reshape(-1, row)


def _runs(lengths):
    out = []
    for k, n in enumerate(lengths):
        out += [k % 200 + 1] * n
    return out


def _run_lengths():
    return _rows(_runs([1, 2, 3, 4, 258, 259, 260, 261, 262, 517]), 64)


def _boundaries():
    """Rows of 64 bytes, pieces of 4 rows: a run of 100 from byte 40 of row 1 (it crosses a row inside piece 0); 56 bytes of 9 that end
    with piece 0 and 30 more 9s that open piece 1 (two runs: pieces are independent)."""
    ramp = lambda n: (np.arange(n) % 2 + 20).tolist()
    flat = ramp(64) + ramp(40) + [7] * 100 + ramp(256 - 204 - 56) + [9] * 56 + [9] * 30 + ramp(100)
    return _rows(flat, 64)


def _all_symbols():
    """Every literal, and matches of 28 lengths, one in every length code 257 .. 285 but one."""
    lengths = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 258]
    flat = []
    for v in range(256):
        flat += [v] * (1 + (lengths[v] if v < len(lengths) else 0))
    return _rows(flat, 101)


def _fibonacci():
    """24 byte values whose counts are the Fibonacci numbers 1, 1, 2, .. 46,368, shuffled: 121,392 bytes = 281 rows of 432."""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    flat = np.repeat(np.arange(24, dtype=np.uint8) * 3, fib)
    np.random.default_rng(5).shuffle(flat)
    assert flat.size == 281 * 432
    return flat.reshape(281, 432)


# name -> (filtered rows, stripe_rows)
HAND = {"run_lengths": (_run_lengths, 1000), "run_lengths_in_pieces": (_run_lengths, 3), "boundaries": (_boundaries, 4),
        "one_byte": (lambda: np.zeros((2, 21), np.uint8), 2), "single": (lambda: np.full((1, 2), 200, np.uint8), 1),
        "all_symbols": (_all_symbols, 1000), "fibonacci": (_fibonacci, 281)}


@pytest.mark.parametrize("name", list(HAND))
def test_deflate_stage_on_hand_made_rows(name):
    from umhsnerf import ops

    make, rows = HAND[name]
    filtered = make()
    H, row = filtered.shape
    W = row - 1
    if name in ("one_byte", "single"):  # 42 zeros: a literal, a match of 41, the end of block; 200 200: two symbols of length 1
        lengths = P.code_lengths(P.histogram(P.tokens(filtered.tobytes())))
        assert sorted(l for l in lengths if l) == ([1, 2, 2] if name == "one_byte" else [1, 1])
    if name == "all_symbols":
        hist = P.histogram(P.tokens(filtered.tobytes()))
        assert all(hist[:256]) and sum(1 for c in hist[257:] if c) >= 10
    if name == "fibonacci":
        hist = P.histogram(P.tokens(filtered.tobytes()))
        _, per_depth = P.huffman_depth_counts(hist)
        assert max(per_depth) > 15, per_depth  # the unlimited tree IS too deep: the fix-up runs
        assert max(P.code_lengths(hist)) == 15
    expect = P.encode_filtered(filtered, W, 1, rows)
    data = _file(*ops.png_deflate(torch.from_numpy(filtered).to(DEV), W, 1, rows))
    assert len(data) <= ops.png_max_bytes(H, W, 1, rows)
    assert data == expect, _first_difference(data, expect)
    assert zlib.decompress(P.idat_payload(data)) == filtered.tobytes()


def test_capacity_one_byte_short_leaves_the_tail_alone_and_names_the_size():
    from umhsnerf import ops

    frame, _, expect = _reference("noise", (64, 96, 3), "adaptive", 16)
    dframe = _device_frame(frame, 0)
    for short in (1, 700, len(expect) - 100):
        cap = len(expect) - short
        buf = torch.full((len(expect) + 64,), CANARY, dtype=torch.uint8, device=DEV)
        out, length = ops.png_encode(dframe, "adaptive", 16, out=buf[:cap])
        assert int(length.item()) == len(expect)
        host = buf.cpu().numpy()
        assert (host[cap:] == CANARY).all(), "bytes past the capacity were written"
        assert host[:cap].tobytes() == expect[:cap]  # (a chunk's CRC lies behind its data: it is written only when no data byte was cut)


def test_the_same_frame_gives_the_same_bytes_whatever_used_the_workspace_before():
    from umhsnerf import ops

    frame, _, expect = _reference("smooth", (64, 96, 3), "adaptive", 16)
    dframe = _device_frame(frame, 0)
    ws = torch.empty(ops.png_workspace_bytes(64, 96, 3, 1), dtype=torch.uint8, device=DEV)
    first = _file(*ops.png_encode(dframe, "adaptive", 16, workspace=ws))
    assert first == _file(*ops.png_encode(dframe, "adaptive", 16, workspace=ws)) == expect
    for content, rows in (("noise", 1), ("zeros", 100), ("checker", 4)):
        other, _, want = _reference(content, (64, 96, 3), "adaptive", rows)
        assert _file(*ops.png_encode(_device_frame(other, 0), "adaptive", rows, workspace=ws)) == want
    assert _file(*ops.png_encode(dframe, "adaptive", 16, workspace=ws)) == first
    assert _file(*ops.png_encode(dframe, "adaptive", 16)) == first  # (the registry's slot)


def test_arguments():
    import ctypes

    from umhsnerf import _hip, ops

    lib, d = _hip.lib(), ctypes.c_void_p(4096)  # never dereferenced: every call below returns from its argument checks
    assert lib.umhs_png_encode(None, 8, 8, 3, 5, 1, d, 100, d, d, 1 << 20, None) == -1
    assert lib.umhs_png_encode(d, 8, 8, 2, 5, 1, d, 100, d, d, 1 << 20, None) == -1
    assert lib.umhs_png_encode(d, 8, 8, 3, 6, 1, d, 100, d, d, 1 << 20, None) == -1
    assert lib.umhs_png_encode(d, 8, 65536, 3, 5, 1, d, 100, d, d, 1 << 20, None) == -2
    assert lib.umhs_png_encode(d, 65536, 8, 3, 5, 1, d, 100, d, d, 1 << 20, None) == -2
    assert lib.umhs_png_encode(d, 8, 8, 3, 5, 65536, d, 100, d, d, 1 << 20, None) == -2
    assert lib.umhs_png_encode(d, 65535, 65535, 3, 5, 65535, d, 100, d, d, 1 << 20, None) == -2  # one chunk past 2^31 - 1 bytes
    assert lib.umhs_png_encode(d, 8, 8, 3, 5, 1, d, 100, d, d, 8, None) == -3
    assert lib.umhs_png_deflate(d, 8, 8, 3, 1, d, -1, d, d, 1 << 20, None) == -1
    assert lib.umhs_png_filter(d, 8, 8, 3, 5, None, None) == -1
    with pytest.raises(ValueError, match="no CPU path"):
        ops.png_encode(torch.zeros(8, 8, 3, dtype=torch.uint8))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
from test_hip_render import world  # noqa: E402,F401  (the scene, the trained pipeline and the three cameras of the render tests)

E2E_NAMES = ["rgb", "seg_pred", "depth"]


def _first_cameras(c, n):
    from umhsnerf.data.umhs_dataparser import Cameras

    return Cameras(c.camera_to_worlds[:n].contiguous(), c.fx[:n], c.fy[:n], c.cx[:n], c.cy[:n], c.height, c.width,
                   None if c.distortion_params is None else c.distortion_params[:n].contiguous(), c.camera_type)


def _decoded(directory):
    from PIL import Image

    files = sorted(p for p in directory.rglob("*.png"))
    return {str(p.relative_to(directory)): np.asarray(Image.open(p)) for p in files}, files


def _same_pictures(host_dir, gpu_dir, expect_files):
    host, _ = _decoded(host_dir)
    gpu, files = _decoded(gpu_dir)
    assert len(host) == expect_files and sorted(host) == sorted(gpu)
    for k in host:
        assert host[k].shape == gpu[k].shape and np.array_equal(host[k], gpu[k]), k
    for p in files:  # what the device wrote is this encoder's stream: one IDAT per piece, every CRC right
        kinds = [k for k, _ in P.parse_chunks(p.read_bytes())]
        assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}


def test_camera_path_frames_decode_to_the_host_encoder_s_pixels(world):
    from umhsnerf.render import render_camera_path

    pipe, cameras, root = world["pipe"], _first_cameras(world["cameras"], 2), world["root"]
    render_camera_path(pipe, cameras, root / "png_host", E2E_NAMES, png_encoder="host")
    res = render_camera_path(pipe, cameras, root / "png_gpu", E2E_NAMES, png_encoder="gpu", png_stripe_rows=7)
    assert res["frames"] == 2 and pipe.training
    _same_pictures(root / "png_host", root / "png_gpu", 2)
    assert len(P.parse_chunks((root / "png_gpu" / "frame_00000.png").read_bytes())) == 2 + 3  # 20 rows in pieces of 7


def test_dataset_files_decode_to_the_host_encoder_s_pixels(world):
    from umhsnerf.render import render_dataset

    pipe, root = world["pipe"], world["root"]
    a = render_dataset(pipe, ["test"], root / "ds_host", E2E_NAMES)
    b = render_dataset(pipe, ["test"], root / "ds_gpu", E2E_NAMES, png_encoder="gpu")
    assert a["files"] == b["files"] == 3 * a["frames"] and a["frames"] >= 1
    _same_pictures(root / "ds_host", root / "ds_gpu", a["files"])


def test_textured_mesh_atlases_decode_to_the_host_encoder_s_pixels(world):
    from test_hip_texture import KW, N_STEPS
    from umhsnerf import export

    assert N_STEPS == 3  # (the render tests' pipeline has had the steps that leave a surface inside the box)
    pipe, root = world["pipe"], world["root"]
    a = export.export_textured_mesh(pipe, root / "tex_host", px_per_uv_triangle=4, texture_output_names=("rgb", "seg_pred"), **KW)
    b = export.export_textured_mesh(pipe, root / "tex_gpu", px_per_uv_triangle=4, texture_output_names=("rgb", "seg_pred"),
                                    png_encoder="gpu", **KW)
    assert a["faces"] == b["faces"] and a["atlas_side"] == b["atlas_side"]
    _same_pictures(root / "tex_host", root / "tex_gpu", 2)
    assert (root / "tex_gpu" / "material_0.png").exists()
