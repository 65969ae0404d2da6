"""Lens distortion on the CPU: the dataparser reads OpenCV distortion parameters (fixed or per frame), and the torch restatement of the
distorted ray generator (tests/raygen_f64.py) inverts the closed-form model and reduces to the oracle's generator at zero."""
import json

import numpy as np
import pytest
import torch

import raygen_f64 as RG
from oracle import torch_ref as T
from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig


def _pose(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, rng.normal(size=3) * 3
    return m


def make_scene(root, n_train=5, n_eval=2, H=6, W=8, B=7, top=None, per_frame=None, seed=0):
    """The ``make_scene`` recipe of tests/test_data_cpu.py; ``top``: keys added at top level, ``per_frame(split, i)``: keys per frame."""
    rng = np.random.default_rng(seed)
    frames = []
    for split, cnt in (("train", n_train), ("eval", n_eval)):
        (root / split).mkdir(parents=True)
        (root / f"hs_{split}").mkdir()
        for i in reversed(range(cnt)):  # unsorted on purpose
            np.save(root / split / f"r_{i:03d}.npy", (rng.random((H, W, 4)) * 255).astype(np.uint8))
            np.save(root / f"hs_{split}" / f"r_{i:03d}.npy", (rng.random((H, W, B)) * 1.4 - 0.2).astype(np.float32))
            fr = {"file_path": f"{split}/r_{i:03d}.npy", "hyperspectral_file_path": f"hs_{split}/r_{i:03d}.npy", "transform_matrix": _pose(rng).tolist()}
            if per_frame is not None:
                fr.update(per_frame(split, i))
            frames.append(fr)
    meta = {"frames": frames, "wavelengths": [400 + 10 * k for k in range(B)], "fl_x": 10.0, "fl_y": 11.0, "cx": W / 2, "cy": H / 2, "h": H, "w": W}
    meta.update(top or {})
    (root / "transforms.json").write_text(json.dumps(meta))
    return meta


def _parse(path, split):
    return UMHSDataParserConfig(data=path, num_classes=3).setup().get_dataparser_outputs(split)


def test_fixed_distortion_parses_in_nerfstudio_order(tmp_path):
    make_scene(tmp_path, top={"camera_model": "OPENCV", "k1": -0.1, "k2": 0.02, "p1": 1e-3, "p2": -2e-3})
    tr, ev = _parse(tmp_path, "train"), _parse(tmp_path, "val")
    want = torch.tensor([-0.1, 0.02, 0.0, 0.0, 1e-3, -2e-3])  # (k1, k2, k3, k4, p1, p2); missing keys are 0
    for out, n in ((tr, 5), (ev, 2)):
        dp = out.cameras.distortion_params
        assert dp.shape == (n, 6) and dp.dtype == torch.float32 and dp.is_contiguous()
        assert torch.equal(dp, want.expand(n, 6))
    moved = tr.cameras.to("cpu")
    assert torch.equal(moved.distortion_params, tr.cameras.distortion_params) and len(moved) == 5


def test_distortion_params_list_at_top_level_wins_over_single_keys(tmp_path):
    make_scene(tmp_path, top={"distortion_params": [0.01, 0.02, 0.03, 0.04, 0.05, 0.06], "k1": 9.0})
    assert _parse(tmp_path, "train").cameras.distortion_params[0].tolist() == pytest.approx([0.01, 0.02, 0.03, 0.04, 0.05, 0.06])


def test_per_frame_distortion_follows_the_splits_rows(tmp_path):
    """Per-frame values (no distortion key at top level): row i of a split is the frame the split's i-th file name belongs to."""
    def per_frame(split, i):
        base = 0.01 * (i + 1) * (1 if split == "train" else -1)
        if i % 2:
            return {"distortion_params": [base, 0.0, 0.0, 0.0, 2 * base, 0.0]}
        return {"k1": base, "p1": 2 * base}

    make_scene(tmp_path, per_frame=per_frame)
    tr, ev = _parse(tmp_path, "train"), _parse(tmp_path, "val")
    assert [p.name for p in tr.image_filenames] == [f"r_{i:03d}.npy" for i in range(5)]
    want_tr = torch.tensor([[0.01 * (i + 1), 0, 0, 0, 0.02 * (i + 1), 0] for i in range(5)])
    want_ev = torch.tensor([[-0.01 * (i + 1), 0, 0, 0, -0.02 * (i + 1), 0] for i in range(2)])
    torch.testing.assert_close(tr.cameras.distortion_params, want_tr, rtol=0, atol=1e-9)
    torch.testing.assert_close(ev.cameras.distortion_params, want_ev, rtol=0, atol=1e-9)


def test_fixed_keys_win_over_per_frame_values(tmp_path):
    """The reference's rule (``distort_fixed``): any of k1, k2, k3, p1, p2, distortion_params at top level fixes every frame."""
    make_scene(tmp_path, top={"k2": 0.05}, per_frame=lambda split, i: {"k1": 0.3})
    dp = _parse(tmp_path, "train").cameras.distortion_params
    assert torch.equal(dp, torch.tensor([0.0, 0.05, 0.0, 0.0, 0.0, 0.0]).expand(5, 6))


def test_all_zero_distortion_is_none(tmp_path):
    make_scene(tmp_path, top={"k1": 0.0, "k2": 0.0, "p1": 0.0, "p2": 0.0, "camera_model": "OPENCV"})
    assert _parse(tmp_path, "train").cameras.distortion_params is None
    (tmp_path / "b").mkdir()
    make_scene(tmp_path / "b", per_frame=lambda split, i: {"k1": 0.0})
    assert _parse(tmp_path / "b", "val").cameras.distortion_params is None
    (tmp_path / "c").mkdir()
    make_scene(tmp_path / "c")  # no key anywhere
    assert _parse(tmp_path / "c", "train").cameras.distortion_params is None


def test_fisheye_still_raises(tmp_path):
    make_scene(tmp_path, top={"camera_model": "OPENCV_FISHEYE", "k1": 0.1})
    with pytest.raises(NotImplementedError, match="OPENCV_FISHEYE"):
        _parse(tmp_path, "train")


def _whole_grid(n, H, W):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.cat([torch.stack([torch.full_like(yy, c), yy, xx], -1).reshape(-1, 3) for c in range(n)])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_float64_round_trip_through_the_closed_form_model(seed):
    """Undistort every pixel centre of a 640x480 image at f = 500, distort the result with the closed-form model: the input comes back.
    Independent of anything recalled from upstream.  Also the facts the GPU test's box rests on: no Newton step of any pixel is near
    the |det| > 1e-3 switch, and the float32 solve is the float64 one to a few ulp of the image-plane coordinates."""
    n, H, W = 3, 480, 640
    intr = torch.tensor([[500.0, 500.0, W / 2, H / 2]], dtype=torch.float64).expand(n, 4).contiguous()
    k = RG.draw_distortion(n, seed)
    idx = _whole_grid(n, H, W)
    xs, ys = RG.image_plane_points(idx, intr)
    kk = k.double()[idx[:, 0]][None]
    xu, yu, min_det = RG.undistort(xs, ys, kk, return_min_det=True)
    xr, yr = RG.distort(xu, yu, kk)
    err = float(torch.maximum((xr - xs).abs(), (yr - ys).abs()).max())
    xs32, ys32 = RG.image_plane_points(idx, intr.float())
    xu32, yu32 = RG.undistort(xs32, ys32, kk.float())
    err32 = float(torch.maximum((xu32.double() - xu).abs(), (yu32.double() - yu).abs()).max())
    print(f"seed {seed}: round trip {err:.2e}, min |det| {float(min_det.min()):.3f}, float32 solve vs float64 {err32:.2e}")
    assert float(min_det.min()) > 0.1
    assert err <= 1e-15  # a few ulp of coordinates below 1 (measured: <= 4e-16)
    assert err32 <= 4e-7  # about 3 ulp of a float32 coordinate near 0.8 (measured: <= 2.0e-7)
    assert float((xu - xs).abs().max()) > 1e-2  # and the distortion is not a no-op at the image border


def test_zero_parameters_reduce_to_the_oracle_exactly():
    n, H, W = 9, 480, 640
    g = torch.Generator().manual_seed(0)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    c2w = torch.cat([q, torch.randn(n, 3, 1, generator=g)], -1).contiguous()
    intr = torch.stack([torch.rand(n, generator=g) * 500 + 100, torch.rand(n, generator=g) * 500 + 100,
                        torch.full((n,), W / 2) + torch.randn(n, generator=g), torch.full((n,), H / 2) + torch.randn(n, generator=g)], -1)
    idx = T.pixel_sample_indices(torch.rand(20000, 3, generator=g), n, H, W)
    got = RG.generate_rays_distorted(idx, c2w, intr, torch.zeros(n, 6))
    want = T.generate_rays(idx, c2w, intr)
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b)
