"""``render_camera_path(..., output_format="video")`` and ``jpeg_encoder="gpu"`` end to end on the GPU, with the recipe of
tests/test_hip_render.py's ``world``: three 20 x 28 cameras, three classes, three training steps, seven panels.

The payloads of the .avi are compared byte for byte with the reference encoder (tests/jpeg_ref.py) applied to ``compose_frame`` of a
second render of the same rays (inference is deterministic: tests/test_hip_render.py relies on it), and with the .jpg files the
device encoder writes as images; the ``host`` default still writes a PIL JPEG of the same composed bytes."""
import io
import json
import struct

import numpy as np
import pytest
import torch

import jpeg_ref as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
NAMES = ["rgb", "abundances_0", "wv_3", "residual_2", "depth", "accumulation", "seg_pred"]
QUALITY, SS, RESTART = 90, "420", 3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from test_hip_distortion import _look_at_origin, make_scene
    from test_hip_render import _datamanager
    from umhsnerf.render import compose_frame, load_camera_path, path_fps, render_camera_path
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    root = tmp_path_factory.mktemp("video")
    meta = make_scene(root / "scene", B=8)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2,
                                            datamanager=_datamanager(root / "scene", 9))
    for step in range(3):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    rng = np.random.default_rng(11)
    path = {"camera_type": "perspective", "render_height": H, "render_width": W, "fps": 24, "seconds": 0.125,
            "camera_path": [{"camera_to_world": _look_at_origin(rng).reshape(-1).tolist(), "fov": fov, "aspect": W / H} for fov in FOVS]}
    (root / "path.json").write_text(json.dumps(path))
    cameras, path_meta = load_camera_path(root / "path.json", device=DEV)
    pipe.train()
    video = render_camera_path(pipe, cameras, root / "video" / "fly.avi", NAMES, jpeg_quality=QUALITY, cube_names=["spectral"],
                               output_format="video", jpeg_subsampling=SS, restart_mcus=RESTART, fps=path_fps(path_meta))
    assert pipe.training and pipe.model.training  # train() is restored
    render_camera_path(pipe, cameras, root / "gpu", NAMES, image_format="jpeg", jpeg_quality=QUALITY, jpeg_encoder="gpu",
                       jpeg_subsampling=SS, restart_mcus=RESTART)
    render_camera_path(pipe, cameras, root / "host", NAMES, image_format="jpeg", jpeg_quality=QUALITY)
    assert pipe.training
    pipe.eval()
    frames = []
    with torch.no_grad():
        for i in range(3):  # the second render of the same rays
            outputs = pipe.model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True))
            frames.append(compose_frame(outputs, NAMES).cpu().numpy())
    pipe.train()
    return dict(root=root, video=video, frames=frames)


def _payloads(data):
    chunks = J.riff_chunks(data)
    movi = J.riff_find(chunks, "LIST:movi")
    return chunks, [data[off:off + size] for cc, off, size, _ in movi[3] if cc == "00dc"]


def test_video_holds_the_reference_encoding_of_every_frame(world):
    root, res = world["root"], world["video"]
    assert res["frames"] == 3 and res["files"] == [str(root / "video" / "fly.avi")]
    assert sorted(p.name for p in (root / "video").iterdir()) == ["fly.avi"] + [f"spectral_{i:05d}.npy" for i in range(3)]
    data = (root / "video" / "fly.avi").read_bytes()
    chunks, payloads = _payloads(data)
    assert len(payloads) == 3
    for i, frame in enumerate(world["frames"]):
        assert frame.shape == (H, 7 * W, 3)
        assert payloads[i] == J.encode(frame, QUALITY, SS, RESTART), f"frame {i}"
        assert payloads[i] == (root / "gpu" / f"frame_{i:05d}.jpg").read_bytes()
    assert len(set(payloads)) == 3  # three different cameras
    avih, strh = J.riff_find(chunks, "avih"), J.riff_find(chunks, "strh")
    total_frames, width, height = struct.unpack_from("<I", data, avih[1] + 16)[0], *struct.unpack_from("<II", data, avih[1] + 32)
    scale, rate, _, length = struct.unpack_from("<IIII", data, strh[1] + 20)
    assert (total_frames, width, height, length) == (3, 7 * W, H, 3) and rate / scale == 24  # the path's fps


def test_host_default_still_writes_a_pil_jpeg_of_the_composed_bytes(world):
    from PIL import Image

    for i, frame in enumerate(world["frames"]):
        expect = io.BytesIO()
        Image.fromarray(frame).save(expect, "JPEG", quality=QUALITY)
        assert (world["root"] / "host" / f"frame_{i:05d}.jpg").read_bytes() == expect.getvalue()


def test_bad_arguments_are_refused_before_anything_is_rendered(tmp_path):
    from umhsnerf.render import render_camera_path

    with pytest.raises(ValueError, match="NAME.avi"):
        render_camera_path(None, None, tmp_path / "out.mp4", NAMES, output_format="video")
    with pytest.raises(ValueError, match="image_format='jpeg'"):
        render_camera_path(None, None, tmp_path / "out", NAMES, jpeg_encoder="gpu")
