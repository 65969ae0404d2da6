"""CPU-only checks of whole-frame ray generation and cropped / non-perspective camera paths: the restatement tests/frame_rays_f64.py
itself (its perspective model against the oracle, the fisheye and equirectangular models through their closed-form inverses, the box
intersection against the box's geometry), the precondition the GPU tests of ``umhs_raygen_frame`` rest on, ``load_camera_path`` for the
three camera types and a ``crop``, the interpolated poses of ``render interpolate``, and the library's export of the new symbol."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import frame_rays_f64 as FR
from oracle import torch_ref as T


def _pose64(seed, radius=3.0):
    """A float64 look-at pose whose 3x3 block is orthonormal to float64 rounding."""
    from test_hip_distortion import _look_at_origin

    m = _look_at_origin(np.random.default_rng(seed))
    m[:3, 3] *= radius / 3.0
    return torch.tensor(m[:3], dtype=torch.float64)[None].contiguous()


def _intr(H, W, fov, camera_type, dtype=torch.float64):
    fx, fy = (W / 2.0, float(H)) if camera_type == "equirectangular" else ((H / 2.0) / math.tan(fov * math.pi / 360.0),) * 2
    return torch.tensor([[fx, fy, W / 2.0, H / 2.0]], dtype=dtype)


# ---- camera models -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,fov", [(20, 28, 50.0), (21, 27, 75.0)])
def test_perspective_restatement_is_the_oracle(H, W, fov):
    c2w, intr = FR.path_cameras(H, W, fov, "perspective")
    for cam in range(FR.N_CAMS):
        got = FR.frame_rays(c2w, intr, cam, H, W, "perspective")
        want = T.generate_rays(FR.frame_indices(cam, H, W), c2w, intr)
        for g, w in zip(got, want):
            assert g.dtype == torch.float32 and torch.equal(g, w)
    part = FR.frame_rays(c2w, intr, 1, H, W, "perspective", rows=(5, 7))
    whole = FR.frame_rays(c2w, intr, 1, H, W, "perspective")
    for p, w in zip(part, whole):
        assert torch.equal(p, w[5 * W:12 * W])
    # all-zero lens parameters are no distortion, bit for bit
    for g, w in zip(FR.frame_rays(c2w, intr, 0, H, W, "perspective", distortion=torch.zeros(FR.N_CAMS, 6)), FR.frame_rays(c2w, intr, 0, H, W)):
        assert torch.equal(g, w)


def _camera_frame(d, c2w):
    return torch.linalg.solve(c2w[0, :3, :3], d[:, :, None])[:, :, 0]


@pytest.mark.parametrize("H,W,fov", [(20, 28, 50.0), (21, 27, 75.0), (21, 27, 120.0)])  # (120: theta passes pi / 2 and stays below pi)
def test_fisheye_round_trip_lands_on_the_pixel_centre(H, W, fov):
    """theta = acos(-d_z), (u, v) = theta (d_x, d_y) / sin theta, in float64: within 1e-9 px of the centre the ray was made for."""
    c2w, intr = _pose64(3), _intr(H, W, fov, "fisheye")
    o, d, area, nrm = FR.frame_rays(c2w, intr, 0, H, W, "fisheye")
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(area).all()) and bool(torch.isfinite(nrm).all())
    assert float((d.norm(dim=-1) - 1).abs().max()) < 1e-14 and float((nrm - 1).abs().max()) < 1e-14  # a unit vector before the pose
    cam = _camera_frame(d, c2w)
    theta = torch.acos((-cam[:, 2]).clamp(-1.0, 1.0))
    s = torch.where(theta.sin() == 0, torch.ones_like(theta), theta / theta.sin())
    px = torch.stack([s * cam[:, 0] * intr[0, 0] + intr[0, 2], -(s * cam[:, 1]) * intr[0, 1] + intr[0, 3]], -1)
    idx = FR.frame_indices(0, H, W)
    centre = torch.stack([idx[:, 2], idx[:, 1]], -1).double() + 0.5
    err = float((px - centre).abs().max())
    print(f"fisheye {H}x{W} fov {fov}: round trip {err:.3e} px")
    assert err <= 1e-9
    if H % 2 and W % 2:  # the pixel on the principal point: theta == 0, where upstream divides 0 by 0
        mid = (H // 2) * W + W // 2
        assert bool(torch.isfinite(d[mid]).all()) and float((cam[mid] - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)).abs().max()) < 1e-15
        d32 = FR.frame_rays(c2w.float(), intr.float(), 0, H, W, "fisheye")[1]
        assert bool(torch.isfinite(d32).all())


@pytest.mark.parametrize("H,W", [(16, 32), (15, 31)])
def test_equirectangular_round_trip_lands_on_the_pixel_centre(H, W):
    """phi = acos(d_y), theta = atan2(-d_x, -d_z), in float64.  (d = (-sin theta sin phi, cos phi, -cos theta sin phi) and sin phi > 0
    inside the frame, so it is the NEGATED x and z that give theta back; atan2(d_x, d_z) is theta + pi.)"""
    c2w, intr = _pose64(4), _intr(H, W, 0.0, "equirectangular")
    o, d, area, nrm = FR.frame_rays(c2w, intr, 0, H, W, "equirectangular")
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(area).all()) and float((nrm - 1).abs().max()) < 1e-14
    cam = _camera_frame(d, c2w)
    phi, theta = torch.acos(cam[:, 1].clamp(-1.0, 1.0)), torch.atan2(-cam[:, 0], -cam[:, 2])
    u, v = -theta / math.pi, 0.5 - phi / math.pi
    px = torch.stack([u * intr[0, 0] + intr[0, 2], -v * intr[0, 1] + intr[0, 3]], -1)
    idx = FR.frame_indices(0, H, W)
    centre = torch.stack([idx[:, 2], idx[:, 1]], -1).double() + 0.5
    err = float((px - centre).abs().max())
    print(f"equirectangular {H}x{W}: round trip {err:.3e} px")
    assert err <= 1e-9
    # the frame spans the sphere: longitudes over (-pi, pi), latitudes over (0, pi)
    assert float(theta.min()) < -3.0 and float(theta.max()) > 3.0 and float(phi.min()) < 0.15 and float(phi.max()) > 3.0


# ---- the box -----------------------------------------------------------------------------------------------------------------------
def _random_rays(n, seed, inside=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g, dtype=torch.float64) * 1.5
    o[:inside] *= 0.05
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    return o, d


def test_intersect_obb_hits_touch_the_surface_and_misses_stay_outside():
    box = FR.gpu_box("perspective")
    Tb, Rb, Sb = (torch.tensor(np.asarray(v), dtype=torch.float64) for v in box)
    o, d = _random_rays(4000, 0, inside=200)
    o[:200] += Tb  # origins inside the box
    nears, fars, hit, gap = FR.intersect_obb(o, d, *box)
    assert 300 < int(hit.sum()) < 3700
    unit = lambda p: (FR.box_frame(p, Tb, Rb).abs() / (Sb / 2)).max(-1).values  # 1 on the surface, < 1 inside
    started_inside = unit(o) < 1
    assert bool(hit[:200].all()) and bool(started_inside[:200].all())
    entry, exit_ = o + nears[:, None] * d, o + fars[:, None] * d
    assert float((unit(exit_)[hit] - 1).abs().max()) <= 1e-12
    outside = hit & ~started_inside
    assert int(outside.sum()) > 100 and float((unit(entry)[outside] - 1).abs().max()) <= 1e-12
    assert bool((nears[hit & started_inside] == 0).all()) and bool((fars[hit] > nears[hit]).all())
    assert bool((gap[hit] > 0).all()) and bool((gap[~hit] <= 0).all())
    # misses: both arrays 1e10, and no point of the ray (1000 parameters each, out to well past the box) inside the box
    assert bool((nears[~hit] == 1e10).all()) and bool((fars[~hit] == 1e10).all())
    t = torch.linspace(0.0, 12.0, 1000, dtype=torch.float64)
    pts = o[~hit][:, None, :] + t[None, :, None] * d[~hit][:, None, :]
    assert float(unit(pts).min()) >= 1.0
    # near_floor lifts the entries below it and nothing else
    n2, f2, h2, _ = FR.intersect_obb(o, d, *box, near_floor=0.05)
    assert torch.equal(h2, hit) and torch.equal(f2, fars) and torch.equal(n2[hit], nears[hit].clamp(min=0.05)) and torch.equal(n2[~hit], nears[~hit])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_axis_parallel_rays_are_classified_on_both_sides_of_the_slab(dtype):
    """One component of d' exactly 0: the slab test of that axis is +-inf on both ends, and decides by the origin alone."""
    box = (np.zeros(3, np.float32), np.eye(3, dtype=np.float32), np.array([1.0, 2.0, 3.0], np.float32))
    d = torch.tensor([[1.0, 0.0, 0.0]] * 4 + [[0.6, 0.0, 0.8]] * 2, dtype=dtype)
    o = torch.tensor([[-2.0, 0.9, 0.0], [-2.0, 1.1, 0.0], [-2.0, -0.9, 1.4], [-2.0, -1.1, 0.0], [-0.3, 0.99, -0.4], [-0.3, -1.01, -0.4]], dtype=dtype)
    nears, fars, hit, _ = FR.intersect_obb(o, d, *box)
    assert hit.tolist() == [True, False, True, False, True, False]
    assert nears[0] == 1.5 and fars[0] == 2.5 and nears[2] == 1.5 and bool((nears[~hit] == 1e10).all()) and bool((fars[~hit] == 1e10).all())
    assert bool(torch.isfinite(nears).all()) and bool(torch.isfinite(fars).all())


def test_gpu_inputs_have_no_ray_whose_hit_differs_between_float32_and_float64():
    """The precondition of tests/test_hip_frame_rays.py's box tests: on every frame they run (tests/frame_rays_f64.py gpu_cases, three
    cameras each, the type's box) the float32 and the float64 restatement agree on hit or miss for EVERY ray -- the cap on rays
    excluded for grazing is zero.  If a change of inputs ever makes one flip, change the inputs, not the cap."""
    smallest = math.inf
    for camera_type, H, W, fov in FR.gpu_cases():
        c2w, intr = FR.path_cameras(H, W, fov, camera_type)
        box = FR.gpu_box(camera_type)
        for cam in range(FR.N_CAMS):
            o32, d32, _, _ = FR.frame_rays(c2w, intr, cam, H, W, camera_type)
            o64, d64, _, _ = FR.frame_rays(c2w.double(), intr.double(), cam, H, W, camera_type)
            _, _, h32, _ = FR.intersect_obb(o32, d32, *box)
            _, _, h64, gap = FR.intersect_obb(o64, d64, *box)
            flips = int((h32 != h64).sum())
            hits = int(h64.sum())
            print(f"{camera_type} {H}x{W} camera {cam}: {hits} of {H * W} rays hit, {flips} flips, smallest gap among hits "
                  f"{float(gap[h64].min()) if hits else math.nan:.3e}")
            assert flips == 0, (camera_type, H, W, cam, flips)
            assert 10 <= hits < H * W, (camera_type, H, W, cam, hits)  # more than a handful hit, and some miss
            smallest = min(smallest, float(gap[h64].min()))
    # no hit is within float32 rounding of the miss rule: t is O(3), float32 eps * 3 * a handful of operations is ~ 3e-6
    assert smallest > 1e-4, smallest


# ---- load_camera_path --------------------------------------------------------------------------------------------------------------
def _path(camera_type, H=20, W=28, fovs=(50.0, 75.0), **top):
    cams = []
    for k, fov in enumerate(fovs):
        m = np.eye(4)
        m[:3, :3] = np.linalg.qr(np.random.default_rng(k).normal(size=(3, 3)))[0]
        m[:3, 3] = [0.5 * k, -1.0, 2.0 + k]
        cams.append({"camera_to_world": m.reshape(-1).tolist(), "fov": fov, "aspect": 1.4})
    return {"camera_type": camera_type, "render_height": H, "render_width": W, "camera_path": cams, "fps": 24, "seconds": 2.0, **top}


def _loader():
    """``load_camera_path`` as ``python -m umhsnerf.render camera-path`` calls it: every camera type it has rays for, crop honoured."""
    import functools

    from umhsnerf.render import CAMERA_TYPES, load_camera_path

    return functools.partial(load_camera_path, camera_types=CAMERA_TYPES, crop=True)


def test_load_camera_path_reads_the_three_camera_types():
    load_camera_path = _loader()

    H, W = 20, 28
    cams, meta = load_camera_path(_path("fisheye"))
    assert cams.camera_type == meta["camera_type"] == "fisheye" and meta["crop"] is None
    for k, fov in enumerate((50.0, 75.0)):  # the perspective focal rule
        f = float(np.float32((H / 2) / math.tan(fov * math.pi / 360)))
        assert float(cams.fx[k]) == float(cams.fy[k]) == f
    cams, meta = load_camera_path(_path("equirectangular"), downscale_factor=2.0)
    assert cams.camera_type == "equirectangular" and (cams.height, cams.width) == (10, 14)
    assert cams.fx.tolist() == [W / 2 / 2] * 2 and cams.fy.tolist() == [H / 2] * 2  # fx = W / 2, fy = H, then 1 / d; fov is ignored
    assert cams.cx.tolist() == [W / 2 / 2] * 2 and cams.cy.tolist() == [H / 2 / 2] * 2
    assert load_camera_path(_path("perspective"))[0].camera_type == "perspective"
    assert cams.to("cpu").camera_type == "equirectangular"  # .to() carries the type
    for refused in ("vr180", "omnidirectional", "orthophoto"):
        with pytest.raises(NotImplementedError, match=refused):
            load_camera_path(_path(refused))


def test_load_camera_path_reads_a_crop():
    from umhsnerf.export import obb_from_params

    load_camera_path = _loader()
    crop = {"crop_center": [0.1, -0.05, 0.2], "crop_scale": [0.9, 0.6, 1.2], "crop_rot": [0.3, -0.2, 0.5], "crop_bg_color": {"r": 38, "g": 42, "b": 255}}
    _, meta = load_camera_path(_path("fisheye", crop=crop))
    assert meta["crop"]["background_color"] == [38 / 255, 42 / 255, 1.0]
    for got, want in zip(meta["crop"]["obb"], obb_from_params(crop["crop_center"], crop["crop_rot"], crop["crop_scale"])):
        assert got.dtype == np.float32 and np.array_equal(got, want)
    del crop["crop_rot"]  # optional: zeros
    _, meta = load_camera_path(_path("perspective", crop=crop))
    assert np.array_equal(meta["crop"]["obb"][1], np.eye(3, dtype=np.float32)) and np.array_equal(meta["crop"]["obb"][0], np.float32([0.1, -0.05, 0.2]))
    good = dict(crop)
    for field, bad in (("crop_center", [0, 0]), ("crop_center", None), ("crop_scale", [1, 0, 1]), ("crop_scale", "big"), ("crop_rot", [0, 1]),
                       ("crop_bg_color", {"r": 1, "g": 2}), ("crop_bg_color", [1, 2, 3]), ("crop_bg_color", {"r": 1, "g": 2, "b": 300}),
                       ("crop_center", [0, float("nan"), 0])):
        with pytest.raises(ValueError, match=field):
            load_camera_path(_path("perspective", crop={**good, field: bad}))
    for field in ("crop_center", "crop_scale", "crop_bg_color"):
        with pytest.raises(ValueError, match=field):
            load_camera_path(_path("perspective", crop={k: v for k, v in good.items() if k != field}))
    with pytest.raises(ValueError, match="crop"):
        load_camera_path(_path("perspective", crop=[1, 2, 3]))
    assert load_camera_path(_path("perspective", crop=None))[1]["crop"] is None


def test_load_camera_path_defaults_keep_the_contract_it_had():
    """Without ``camera_types`` / ``crop`` the loader is the one callers were written against: perspective paths without a crop."""
    from umhsnerf.render import CAMERA_TYPES, load_camera_path

    crop = {"crop_center": [0, 0, 0], "crop_scale": [1, 1, 1], "crop_bg_color": {"r": 0, "g": 0, "b": 0}}
    for camera_type in ("fisheye", "equirectangular"):
        with pytest.raises(NotImplementedError, match=f"{camera_type}.*camera_types=CAMERA_TYPES"):
            load_camera_path(_path(camera_type))
        assert load_camera_path(_path(camera_type), camera_types=CAMERA_TYPES)[0].camera_type == camera_type
    with pytest.raises(NotImplementedError, match="crop=True"):
        load_camera_path(_path("perspective", crop=crop))
    with pytest.raises(NotImplementedError, match="crop=True"):
        load_camera_path(_path("fisheye", crop=crop), camera_types=CAMERA_TYPES)
    with pytest.raises(NotImplementedError, match="fisheye"):
        load_camera_path(_path("fisheye", crop=crop), crop=True)
    assert load_camera_path(_path("perspective", crop=crop), crop=True)[1]["crop"] is not None
    cams, meta = load_camera_path(_path("perspective"))
    assert cams.camera_type == "perspective" and meta["crop"] is None


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), "x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])}[axis]


def test_interpolated_poses():
    from umhsnerf.data.umhs_dataparser import Cameras
    from umhsnerf.render import interpolate_cameras, interpolate_poses

    rng = np.random.default_rng(5)
    poses = np.zeros((4, 3, 4))
    for k in range(4):
        poses[k, :, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        poses[k, :, :3] *= np.sign(np.linalg.det(poses[k, :, :3]))  # a rotation, not a reflection
        poses[k, :, 3] = rng.normal(size=3)
    for steps in (2, 3, 10):
        out = interpolate_poses(poses, steps)
        assert out.shape == (3 * steps, 3, 4) and out.dtype == np.float64
        for pair in range(3):  # both ends of every pair are the inputs themselves: joints repeat
            assert np.array_equal(out[pair * steps], poses[pair]) and np.array_equal(out[pair * steps + steps - 1], poses[pair + 1])
        R = out[:, :, :3]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1).max() <= 1e-12
        w = np.linspace(0, 1, steps)
        assert np.allclose(out[:steps, :, 3], (1 - w)[:, None] * poses[0, :, 3] + w[:, None] * poses[1, :, 3], rtol=0, atol=1e-15)
    # halfway through a 90 degree turn is the 45 degree turn -- about z, and about x from a rotated start (trace < 0 branches too)
    for axis, start in (("z", np.eye(3)), ("x", _rot("z", 170.0) @ _rot("x", 100.0))):
        two = np.zeros((2, 3, 4))
        two[0, :, :3], two[1, :, :3] = start, start @ _rot(axis, 90.0)
        two[1, :, 3] = [2.0, 4.0, -6.0]
        mid = interpolate_poses(two, 3)[1]
        assert np.abs(mid[:, :3] - start @ _rot(axis, 45.0)).max() <= 1e-12 and np.allclose(mid[:, 3], [1.0, 2.0, -3.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="two cameras"):
        interpolate_poses(poses[:1], 3)
    with pytest.raises(ValueError, match="interpolation_steps"):
        interpolate_poses(poses, 1)
    cams = Cameras(torch.tensor(poses[:2], dtype=torch.float32), torch.tensor([30.0, 50.0]), torch.tensor([31.0, 51.0]), torch.tensor([16.0, 18.0]),
                   torch.tensor([12.0, 13.0]), 24, 32)
    got = interpolate_cameras(cams, 3)
    assert len(got) == 3 and (got.height, got.width, got.camera_type) == (24, 32, "perspective") and got.distortion_params is None
    assert got.fx.tolist() == [30.0, 40.0, 50.0] and got.fy.tolist() == [31.0, 41.0, 51.0] and got.cx.tolist() == [16.0, 17.0, 18.0]
    assert torch.equal(got.camera_to_worlds[0], cams.camera_to_worlds[0]) and torch.equal(got.camera_to_worlds[2], cams.camera_to_worlds[1])


def test_cli_knows_the_new_subcommands_and_refuses_the_rest_by_name(capsys):
    from umhsnerf.render import parse_args

    base = ["--data", "scene", "--checkpoint", "c.ckpt", "--output-path", "out"]
    a = parse_args(["dataset", *base])
    assert a.command == "dataset" and a.split == "test" and a.rendered_output_names == ["rgb"]
    assert parse_args(["dataset", *base, "--split", "train+test", "--rendered-output-names", "rgb", "depth"]).split == "train+test"
    a = parse_args(["interpolate", *base])
    assert (a.command, a.pose_source, a.interpolation_steps, a.order_poses) == ("interpolate", "eval", 10, False)
    assert parse_args(["interpolate", *base, "--pose-source", "train", "--interpolation-steps", "3"]).interpolation_steps == 3
    for argv, word in ((["interpolate", *base, "--order-poses", "true"], "order-poses"), (["spiral", *base], "spiral"),
                       (["interpolate", *base, "--interpolation-steps", "1"], "interpolation-steps")):
        with pytest.raises(SystemExit) as e:
            parse_args(argv)
        assert e.value.code != 0 and word in capsys.readouterr().err


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_frame_ray_generator(built_library):
    from umhsnerf import _hip, ops

    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, "umhs_raygen_frame") and "umhs_raygen_frame" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["umhs_raygen_frame"][1]) == 19 and _hip.ABI_VERSION == 11
    assert ops.CAMERA_TYPES == {"perspective": 0, "fisheye": 1, "equirectangular": 2}
    # the host-side refusals need no device: nothing is launched (tests/test_hip_frame_rays.py checks that nothing is written either)
    d = ctypes.c_void_p(4096)
    box = (ctypes.c_float * 15)(0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1)
    call = lambda **kw: _hip.lib().umhs_raygen_frame(*[kw.get(k, v) for k, v in dict(
        c2w=d, intr=d, dist=None, n_cams=3, camera=1, type=0, H=20, W=28, row0=0, n_rows=20, obb=None, floor=0.0, o=d, d=d, area=d, nrm=d,
        nears=None, fars=None, stream=None).items()])
    for bad in (dict(c2w=None), dict(intr=None), dict(o=None), dict(d=None), dict(camera=3), dict(camera=-1), dict(type=3), dict(type=-1),
                dict(dist=d, type=1), dict(row0=15, n_rows=6), dict(row0=-1), dict(n_rows=-1), dict(nears=d), dict(fars=d), dict(obb=box),
                dict(floor=-0.1), dict(H=0), dict(W=0)):
        assert call(**bad) == -1, bad
    for k in (12, 13, 14):
        flat = (ctypes.c_float * 15)(*box)
        flat[k] = 0.0
        assert call(obb=flat, nears=d, fars=d) == -1
    assert call(n_rows=0) == 0 and call(row0=20, n_rows=0) == 0  # nothing to do
    with pytest.raises(ValueError, match="camera_type"):
        ops.raygen_frame(torch.zeros(1, 3, 4), torch.ones(1, 4), 0, 4, 4, camera_type="vr180")
    with pytest.raises(ValueError, match="scale"):
        ops.raygen_frame(torch.zeros(1, 3, 4), torch.ones(1, 4), 0, 4, 4, obb=(np.zeros(3), np.eye(3), np.array([1.0, -1.0, 1.0])))
