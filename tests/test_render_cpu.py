"""CPU-only checks of camera-path rendering: ``load_camera_path`` against the formulas by hand, name resolution, the colour tables,
the C struct and the argument checks of ``umhs_frame_compose`` (returned before anything is launched), and the command line."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _path(fovs=(50.0, 75.0), H=20, W=28, **top):
    cams = []
    for k, fov in enumerate(fovs):
        m = np.eye(4)
        m[:3, :3] = np.linalg.qr(np.random.default_rng(k).normal(size=(3, 3)))[0]
        m[:3, 3] = [0.5 * k, -1.0, 2.0 + k]
        m[3] = [9.0, 9.0, 9.0, 9.0]  # the last row is not used
        cams.append({"camera_to_world": m.reshape(-1).tolist(), "fov": fov, "aspect": 3.0})
    return {"camera_type": "perspective", "render_height": H, "render_width": W, "camera_path": cams, "fps": 24, "seconds": 2.0, **top}


# ---- camera paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(20, 28), (31, 17)])
@pytest.mark.parametrize("d", [1.0, 2.0, 1.5])
def test_load_camera_path_follows_the_formulas(H, W, d, tmp_path):
    from umhsnerf.render import load_camera_path

    path = _path(H=H, W=W)
    (tmp_path / "path.json").write_text(json.dumps(path))
    for source in (path, tmp_path / "path.json", str(tmp_path / "path.json")):
        cams, meta = load_camera_path(source, downscale_factor=d)
        assert len(cams) == 2 and (cams.height, cams.width) == (int(H / d), int(W / d))
        assert meta["num_frames"] == 2 and (meta["render_height"], meta["render_width"]) == (cams.height, cams.width)
        for k, fov in enumerate((50.0, 75.0)):
            f = (H / 2) / math.tan(fov * math.pi / 360) * (1 / d)
            assert float(cams.fx[k]) == float(cams.fy[k]) == float(np.float32(f))
            assert float(cams.cx[k]) == float(np.float32(W / 2 * (1 / d))) and float(cams.cy[k]) == float(np.float32(H / 2 * (1 / d)))
            want = np.asarray(path["camera_path"][k]["camera_to_world"], dtype=np.float32).reshape(4, 4)[:3]
            assert np.array_equal(cams.camera_to_worlds[k].numpy(), want)  # used as it is: no re-orientation, no scaling
        assert cams.camera_to_worlds.dtype == cams.fx.dtype == torch.float32 and cams.distortion_params is None
        assert tuple(cams.intrinsics.shape) == (2, 4)
    assert float(cams.fx[0]) != float(cams.fx[1])


def test_load_camera_path_refusals():
    from umhsnerf.render import load_camera_path

    with pytest.raises(NotImplementedError, match="fisheye"):
        load_camera_path(_path(camera_type="fisheye"))
    with pytest.raises(NotImplementedError, match="crop"):
        load_camera_path(_path(crop={"crop_center": [0, 0, 0], "crop_scale": [1, 1, 1]}))
    with pytest.raises(ValueError, match="no camera"):
        load_camera_path(_path(fovs=()))
    load_camera_path(_path(crop=None))  # a null crop is no crop
    cams, _ = load_camera_path({k: v for k, v in _path().items() if k != "camera_type"})  # perspective is the default
    assert len(cams) == 2


# ---- names -----------------------------------------------------------------------------------------------------------------------
def _outputs(H=4, W=5, B=8, C=4):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    return {"rgb": r(H, W, 3), "accumulation": r(H, W, 1), "depth": r(H, W, 1), "spectral": r(H, W, B), "abundances": r(H, W, C),
            "specular": r(H, W, B), "spectral2": r(H, W, B), "seg_raw": r(H, W, 1), "seg_pred": r(H, W, 3), "seg_probs": r(H, W, C + 1),
            "num_samples_per_ray": torch.ones(H, W, 1, dtype=torch.int64), "pair": r(H, W, 2)}


def test_name_resolution():
    from umhsnerf import ops
    from umhsnerf.render import resolve_output, source_keys, usable_output_names

    o = _outputs()
    for name, key, ch, kind in (("rgb", "rgb", 0, ops.PANEL_RGB), ("seg_pred", "seg_pred", 0, ops.PANEL_RGB),
                                ("accumulation", "accumulation", 0, ops.PANEL_SCALAR), ("seg_raw", "seg_raw", 0, ops.PANEL_SCALAR),
                                ("depth", "depth", 0, ops.PANEL_DEPTH), ("wv_7", "spectral", 7, ops.PANEL_SCALAR),
                                ("abundances_2", "abundances", 2, ops.PANEL_SCALAR), ("residual_0", "specular", 0, ops.PANEL_SCALAR)):
        t, c, k = resolve_output(o, name)
        assert t is o[key] and (c, k) == (ch, kind), name  # the base tensor itself: no column is copied
    o["expected_depth"] = o["depth"].clone()
    assert resolve_output(o, "expected_depth")[2] == ops.PANEL_DEPTH  # any name that contains "depth"
    for bad in ("spectral", "abundances", "seg_probs", "pair", "wv_8", "abundances_4", "residual_9", "nope", "num_samples_per_ray", "wv_x"):
        with pytest.raises(ValueError, match="usable names: .*rgb.*wv_0\\.\\.wv_7.*abundances_0\\.\\.abundances_3.*residual_0\\.\\.residual_7"):
            resolve_output(o, bad)
    del o["specular"]
    with pytest.raises(ValueError, match="usable names") as e:
        resolve_output(o, "residual_0")
    assert "residual" not in str(e.value).split("usable names")[1]
    names = usable_output_names(o)
    assert "spectral" not in names and "pair" not in names and "num_samples_per_ray" not in names and "depth" in names
    assert source_keys(["rgb", "abundances_0", "wv_3", "wv_5", "residual_2", "depth", "seg_pred"], ["spectral"]) == [
        "rgb", "abundances", "spectral", "specular", "depth", "accumulation", "seg_pred"]


def test_compose_frame_refuses_bad_names_before_it_touches_the_device():
    from umhsnerf.render import compose_frame

    o = _outputs()
    with pytest.raises(ValueError, match="usable names"):
        compose_frame(o, ["rgb", "spectral"])
    with pytest.raises(ValueError, match="at least one panel"):
        compose_frame(o, [])
    with pytest.raises(ValueError, match="HIP device"):  # CPU tensors: there is no CPU path
        compose_frame(o, ["rgb"])


# ---- colour tables ---------------------------------------------------------------------------------------------------------------
def test_tables_shape_dtype_and_gray():
    from umhsnerf.utils import colormaps

    assert set(colormaps.NAMES) == {"default", "turbo", "viridis", "magma", "inferno", "plasma", "cividis", "gray"}
    for name in colormaps.NAMES:
        t = colormaps.table(name)
        assert t.shape == (256, 3) and t.dtype == np.float32 and t.flags.c_contiguous and not t.flags.writeable
        assert np.isfinite(t).all() and t.min() >= 0 and t.max() <= 1
    assert np.array_equal(colormaps.table("default"), colormaps.table("turbo"))
    assert np.array_equal(colormaps.table("gray"), np.repeat((np.arange(256, dtype=np.float32) / np.float32(255))[:, None], 3, 1))
    assert len({colormaps.table(n).tobytes() for n in colormaps.NAMES}) == 7
    with pytest.raises(ValueError, match="unknown colormap"):
        colormaps.table("jet")
    d = colormaps.device_table("viridis", "cpu")
    assert d.dtype == torch.float32 and np.array_equal(d.numpy(), colormaps.table("viridis")) and colormaps.device_table("viridis", "cpu") is d


def test_tables_equal_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from umhsnerf.utils import colormaps

    for name in ("turbo", "viridis", "magma", "inferno", "plasma", "cividis"):
        assert np.array_equal(colormaps.table(name), np.asarray(matplotlib.colormaps[name].colors, dtype=np.float32)), name


# ---- the C boundary --------------------------------------------------------------------------------------------------------------
def test_panel_struct_is_48_bytes_and_matches_the_header():
    from umhsnerf import _hip

    assert ctypes.sizeof(_hip.FramePanel) == 48
    text = open(os.path.join(ROOT, "include", "umhs_hip.h")).read()
    body = re.search(r"typedef struct umhs_frame_panel \{(.*?)\} umhs_frame_panel;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        m = re.fullmatch(r"(const float\*|int32_t|float)\s+(.*)", decl)
        fields += [(n.strip(), {"const float*": 8, "int32_t": 4, "float": 4}[m.group(1)]) for n in m.group(2).split(",")]
    assert [n for n, _ in fields] == [n for n, _ in _hip.FramePanel._fields_]
    assert sum(size for _, size in fields) == 48
    assert [size for _, size in fields] == [ctypes.sizeof(t) for _, t in _hip.FramePanel._fields_]
    assert "umhs_frame_compose" in _hip.SIGNATURES and "#define UMHS_ABI_VERSION 11" in text
    from umhsnerf import build

    assert "umhs_frame.hip" in build.SOURCES


def test_argument_errors_are_returned_without_a_launch(built_library):
    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, UNSUP = -1, -2
    d = ctypes.c_void_p(4096)  # never dereferenced: every call below returns from the host checks

    def panels(n=1, **kw):
        arr = (_hip.FramePanel * max(n, 1))()
        for k in range(max(n, 1)):
            f = dict(src=4096, range=None, accumulation=None, stride=3, channel=0, kind=0, flags=0, cmin=0.0, cmax=1.0)
            f.update(kw)
            arr[k] = _hip.FramePanel(*[f[name] for name, _ in _hip.FramePanel._fields_])
        return arr

    call = lambda arr, n=1, lut=d, h=4, w=4, frame=d: lib.umhs_frame_compose(arr, n, lut, h, w, frame, None)
    assert call(None) == ARG and call(panels(), lut=None) == ARG and call(panels(), frame=None) == ARG
    assert call(panels(), n=0) == ARG and call(panels(17), n=17) == UNSUP and call(panels(), n=-1) == ARG
    assert call(panels(), h=-1) == ARG and call(panels(), w=-1) == ARG
    assert call(panels(src=None)) == ARG
    assert call(panels(stride=2)) == ARG and call(panels(stride=5, channel=3)) == ARG  # RGB reads channel .. channel + 2
    assert call(panels(kind=1, stride=1, channel=1)) == ARG and call(panels(channel=-1)) == ARG
    assert call(panels(kind=3)) == ARG and call(panels(kind=-1)) == ARG
    assert call(panels(kind=2, stride=1)) == ARG  # DEPTH without a range
    assert call(panels(kind=1, stride=1, flags=1)) == ARG  # normalize without a range
    assert call(panels(src=4098)) == ARG and call(panels(), lut=ctypes.c_void_p(4097)) == ARG  # floats are 4-byte aligned
    assert call(panels(2), n=2, w=1 << 30) == UNSUP  # 2^31 columns in a row
    # nothing to do is a success: no pixel, whatever the other size is; the frame may sit at any byte address
    assert call(panels(), h=0) == 0 and call(panels(), w=0) == 0 and call(panels(16), n=16, h=0, w=0) == 0
    assert call(panels(), h=0, frame=ctypes.c_void_p(4099)) == 0
    assert call(panels(kind=2, stride=1, range=4096), h=0) == 0 and call(panels(kind=1, stride=31, channel=30), w=0) == 0


# ---- command line ----------------------------------------------------------------------------------------------------------------
BASE = ["camera-path", "--data", "scene", "--checkpoint", "c.ckpt", "--camera-path-filename", "p.json", "--output-path", "out"]


def test_cli_parsing():
    from umhsnerf.render import parse_args

    a = parse_args(BASE)
    assert a.rendered_output_names == ["rgb"] and a.cube_output_names == [] and a.downscale_factor == 1.0 and a.image_format == "png"
    assert (a.colormap, a.colormap_min, a.colormap_max, a.colormap_normalize, a.colormap_invert) == ("default", 0.0, 1.0, False, False)
    assert a.depth_near_plane is None and a.depth_far_plane is None and a.jpeg_quality == 100 and a.num_classes == 5 and a.device == "cuda:0"
    a = parse_args(BASE + ["--rendered-output-names", "rgb", "abundances_0", "wv_3", "--cube-output-names", "spectral", "--downscale-factor", "2",
                           "--colormap", "viridis", "--colormap-min", "0.1", "--colormap-max", "0.9", "--colormap-normalize", "--colormap-invert",
                           "true", "--depth-near-plane", "0.5", "--depth-far-plane", "4", "--image-format", "jpeg", "--jpeg-quality", "90",
                           "--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"])
    assert a.rendered_output_names == ["rgb", "abundances_0", "wv_3"] and a.cube_output_names == ["spectral"] and a.downscale_factor == 2.0
    assert (a.colormap, a.colormap_min, a.colormap_max, a.colormap_normalize, a.colormap_invert) == ("viridis", 0.1, 0.9, True, True)
    assert (a.depth_near_plane, a.depth_far_plane, a.image_format, a.jpeg_quality) == (0.5, 4.0, "jpeg", 90)
    assert (a.num_classes, a.pred_specular, a.temperature, a.background_color) == (3, True, 0.4, "black")


def test_cli_refuses_video_and_unknown_colormaps(capsys):
    from umhsnerf.render import main, parse_args

    with pytest.raises(SystemExit) as e:
        main(BASE + ["--output-format", "video"])  # refused while parsing: nothing is loaded, no device is needed
    assert e.value.code != 0
    assert "ffmpeg" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--colormap", "jet"])
    with pytest.raises(SystemExit):
        parse_args(["--data", "scene"])  # no subcommand
