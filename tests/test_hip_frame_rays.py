"""Whole-frame ray generation on the GPU: ``umhs_raygen_frame`` (``ops.raygen_frame``) against the sampled-pixel kernels bit for bit,
against the float64 restatement tests/frame_rays_f64.py for the three camera types and the crop box, and its argument checks.

Frames (frame_rays_f64.gpu_cases): 20 x 28 at fov 50 and the odd 21 x 27 at fov 75 -- it has the theta = 0 pixel of the fisheye model and
its 567 rays do not fill whole blocks -- for perspective and fisheye, 16 x 32 equirectangular; three cameras at radius 3 (seed 11, the
cameras of tests/test_hip_render.py); a second pass over rows (5, 7).  Boxes (frame_rays_f64.gpu_box): centre (0.1, -0.05, 0.2), rpy
(0.3, -0.2, 0.5), scale (0.9, 0.6, 1.2) for perspective and (2.4, 1.8, 3.0) for the wide cameras.

Bounds (none comes from the kernel's own output):
  * origins: bit-equal (a copy of the pose's translation).
  * perspective without a box: bit-equal to ``ops.raygen`` on meshgrid indices -- the kernels share their device functions.
  * directions (absolute), directions_norm and pixel_area (relative): max(floor, 2 x e32), e32 the float32 restatement's own largest
    distance from float64 on the same inputs, the floors those of tests/test_hip_distortion.py (2e-7, 2e-7, 2e-3); 2 is the project's
    standing margin for "the kernel may round differently from torch (here: the device's sinf / cosf), not worse in kind".
  * box: hit or miss equals the float64 restatement's on every ray (tests/test_frame_rays_cpu.py asserts that these inputs allow it:
    no ray is within 7.9e-4 of changing sides); for hits |t - t64| / max(1, t64) <= 2 x e32, e32 measured the same way."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import frame_rays_f64 as FR
import raygen_f64 as RG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (5, 7)
FLOORS = (2e-7, 2e-7, 2e-3)  # directions, directions_norm (relative), pixel_area (relative): tests/test_hip_distortion.py's


@functools.lru_cache(maxsize=None)
def _reference(camera_type, H, W, fov):
    """Cameras, box, and per camera the float64 truth and the float32 restatement (rays, and the box's nears / fars / hit): computed
    once, shared by the tests below, never modified."""
    c2w, intr = FR.path_cameras(H, W, fov, camera_type)
    box = FR.gpu_box(camera_type)
    per_camera = []
    for cam in range(FR.N_CAMS):
        r64 = FR.frame_rays(c2w.double(), intr.double(), cam, H, W, camera_type)
        r32 = FR.frame_rays(c2w, intr, cam, H, W, camera_type)
        b64 = FR.intersect_obb(r64[0], r64[1], *box)
        b32 = FR.intersect_obb(r32[0], r32[1], *box)
        per_camera.append(dict(r64=r64, r32=r32, b64=b64, b32=b32))
    return dict(c2w=c2w, intr=intr, box=box, cams=per_camera)


def _hip(ref, cam, H, W, camera_type, **kw):
    from umhsnerf import ops

    return ops.raygen_frame(ref["c2w"].to(DEV), ref["intr"].to(DEV), cam, H, W, camera_type=camera_type, **kw)


PERSPECTIVE = [c for c in FR.gpu_cases() if c[0] == "perspective"]


# ---- bit identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera_type,H,W,fov", PERSPECTIVE)
@pytest.mark.parametrize("distorted", [False, True])
def test_perspective_frames_carry_the_bits_of_the_sampled_pixel_kernels(camera_type, H, W, fov, distorted):
    from umhsnerf import ops

    ref = _reference(camera_type, H, W, fov)
    k = RG.draw_distortion(FR.N_CAMS, 0).to(DEV) if distorted else None
    for cam in range(FR.N_CAMS):
        idx = FR.frame_indices(cam, H, W).to(DEV)
        want = ops.raygen(idx, ref["c2w"].to(DEV), ref["intr"].to(DEV), want_area=True, want_norm=True, distortion=k)
        got = _hip(ref, cam, H, W, camera_type, distortion=k)
        assert got[4] is None and got[5] is None
        for name, g, w in zip(("origins", "directions", "pixel_area", "directions_norm"), got, want):
            assert g.shape == w.shape and torch.equal(g, w), (cam, name)
    if distorted:  # ... and the distortion was not a no-op
        assert float((got[1] - _hip(ref, FR.N_CAMS - 1, H, W, camera_type)[1]).abs().max()) > 1e-3


@pytest.mark.parametrize("camera_type,H,W,fov", FR.gpu_cases())
def test_a_row_range_is_the_matching_slice_of_the_whole_frame(camera_type, H, W, fov):
    ref = _reference(camera_type, H, W, fov)
    for near_floor in (0.0, 0.05):
        whole = _hip(ref, 1, H, W, camera_type, obb=ref["box"], near_floor=near_floor)
        part = _hip(ref, 1, H, W, camera_type, obb=ref["box"], near_floor=near_floor, rows=ROWS)
        for w, p in zip(whole, part):
            assert p.shape[0] == ROWS[1] * W and torch.equal(p, w[ROWS[0] * W:(ROWS[0] + ROWS[1]) * W])
    last = _hip(ref, 1, H, W, camera_type, rows=(H - 1, 1))  # the last row alone; and no row at all
    assert torch.equal(last[1], whole[1][(H - 1) * W:]) and _hip(ref, 1, H, W, camera_type, rows=(H, 0))[1].shape == (0, 3)


# ---- against float64 ---------------------------------------------------------------------------------------------------------------
def _errors(got, r64):
    _, d64, a64, n64 = r64
    return (float((got[1].cpu().double() - d64).abs().max()), float(((got[3].cpu().double() - n64) / n64).abs().max()),
            float(((got[2].cpu().double() - a64) / a64).abs().max()))


@pytest.mark.parametrize("camera_type,H,W,fov", FR.gpu_cases())
def test_kernel_against_float64(camera_type, H, W, fov):
    # Measured on an MI355X, largest over the three cameras (kernel vs float64 | float32 restatement vs float64 | bound):
    #   perspective     20x28  directions 1.006e-7 | 1.006e-7 | 2.012e-7   norm 1.261e-7 | 1.261e-7 | 2.521e-7   area 5.168e-6 | 5.168e-6 | 2e-3
    #   perspective     21x27  directions 1.126e-7 | 1.126e-7 | 2.252e-7   norm 1.335e-7 | 1.335e-7 | 2.669e-7   area 3.718e-6 | 3.718e-6 | 2e-3
    #   fisheye         20x28  directions 1.079e-7 | 1.079e-7 | 2.158e-7   norm 1.257e-7 | 1.289e-7 | 2.577e-7   area 4.202e-6 | 3.720e-6 | 2e-3
    #   fisheye         21x27  directions 1.367e-7 | 1.183e-7 | 2.367e-7   norm 1.691e-7 | 1.410e-7 | 2.819e-7   area 2.877e-6 | 3.924e-6 | 2e-3
    #   equirectangular 16x32  directions 1.889e-7 | 2.007e-7 | 4.014e-7   norm 1.665e-7 | 1.353e-7 | 2.706e-7   area 3.940e-6 | 3.168e-6 | 2e-3
    # (norm and area relative.)  The device's sinf / cosf keep the wide cameras inside 2 x e32: the floors are not raised.
    ref = _reference(camera_type, H, W, fov)
    worst = [0.0] * 3, [0.0] * 3
    for cam, c in enumerate(ref["cams"]):
        got = _hip(ref, cam, H, W, camera_type)
        assert torch.equal(got[0].cpu(), ref["c2w"][cam, :, 3].expand(H * W, 3))
        assert all(bool(torch.isfinite(t).all()) for t in got[:4])  # (the theta = 0 pixel of the odd fisheye frame included)
        g, e = _errors(got, c["r64"]), _errors([t for t in c["r32"]], c["r64"])
        worst = [max(a, b) for a, b in zip(worst[0], g)], [max(a, b) for a, b in zip(worst[1], e)]
    g, e = worst
    bound = [max(f, 2 * x) for f, x in zip(FLOORS, e)]
    print(f"{camera_type} {H}x{W}: directions hip {g[0]:.3e} f32 {e[0]:.3e} bound {bound[0]:.3e}; norm (rel) hip {g[1]:.3e} f32 {e[1]:.3e} "
          f"bound {bound[1]:.3e}; area (rel) hip {g[2]:.3e} f32 {e[2]:.3e} bound {bound[2]:.3e}")
    assert all(a <= b for a, b in zip(g, bound)), (g, bound)


# ---- the box -----------------------------------------------------------------------------------------------------------------------
def _t_error(nears, fars, b64):
    n64, f64, hit, _ = b64
    rel = lambda t, t64: float(((t.double() - t64).abs() / t64.clamp(min=1.0))[hit].max())
    return max(rel(nears, n64), rel(fars, f64))


@pytest.mark.parametrize("camera_type,H,W,fov", FR.gpu_cases())
def test_box_against_float64(camera_type, H, W, fov):
    # Measured on an MI355X, largest over the three cameras, |t - t64| / max(1, t64) over the hits (kernel | float32 restatement | bound):
    #   perspective     20x28  7.147e-7 | 7.147e-7 | 1.429e-6        perspective     21x27  1.572e-6 | 1.572e-6 | 3.145e-6
    #   fisheye         20x28  1.833e-6 | 1.833e-6 | 3.666e-6        fisheye         21x27  1.656e-6 | 1.600e-6 | 3.199e-6
    #   equirectangular 16x32  2.909e-6 | 3.192e-6 | 6.384e-6
    ref = _reference(camera_type, H, W, fov)
    g = e = 0.0
    for cam, c in enumerate(ref["cams"]):
        *_, nears, fars = _hip(ref, cam, H, W, camera_type, obb=ref["box"])
        nears, fars = nears.cpu().view(-1), fars.cpu().view(-1)
        hit64 = c["b64"][2]
        hit = ~((nears == 1e10) & (fars == 1e10))
        assert torch.equal(hit, hit64), (cam, int((hit != hit64).sum()))  # every ray: the cap on grazing rays is zero
        assert bool((nears[~hit64] == 1e10).all()) and bool((fars[~hit64] == 1e10).all())  # misses: exactly 1e10, both arrays
        assert bool((fars[hit64] > nears[hit64]).all()) and bool((nears[hit64] >= 0).all())
        g, e = max(g, _t_error(nears, fars, c["b64"])), max(e, _t_error(c["b32"][0], c["b32"][1], c["b64"]))
    print(f"{camera_type} {H}x{W}: t (rel) hip {g:.3e} f32 {e:.3e} bound {2 * e:.3e}")
    assert g <= 2 * e, (g, e)


def test_a_camera_inside_the_box_starts_at_the_near_floor():
    camera_type, H, W, fov = "fisheye", 21, 27, 75.0
    ref = _reference(camera_type, H, W, fov)
    centre = ref["c2w"][0, :, 3].numpy() + np.float32([0.05, -0.1, 0.02])
    box = (centre, FR.gpu_box(camera_type)[1], np.float32([1.0, 0.8, 1.2]))
    for floor in (0.0, 0.05, 0.3):
        *_, nears, fars = _hip(ref, 0, H, W, camera_type, obb=box, near_floor=floor)
        assert bool((nears == floor).all()) and bool((fars > 0.28).all()) and bool((fars < 1.2).all())
    for camera_type, H, W, fov in FR.gpu_cases()[1::2] + FR.gpu_cases()[-1:]:  # ... the other types too (odd perspective, equirectangular)
        ref = _reference(camera_type, H, W, fov)
        box = (ref["c2w"][2, :, 3].numpy(), np.eye(3, dtype=np.float32), np.float32([1.0, 1.0, 1.0]))
        *_, nears, fars = _hip(ref, 2, H, W, camera_type, obb=box, near_floor=0.05)
        assert bool((nears == 0.05).all()) and bool((fars >= 0.5 - 1e-6).all()) and bool((fars <= 0.75 ** 0.5 + 1e-6).all())


def test_the_near_floor_changes_only_the_rays_that_enter_below_it():
    """A box whose front face stands 0.03 in front of a fisheye camera, square to its axis: a ray at angle a from the axis enters at
    0.03 / cos a -- below 0.05 up to 53 degrees, above it beyond -- and the rays looking backwards miss."""
    camera_type, H, W, fov = "fisheye", 20, 28, 120.0
    c2w, intr = FR.path_cameras(H, W, fov, camera_type)
    ref = dict(c2w=c2w, intr=intr)
    R = c2w[0, :, :3].numpy()
    box = (c2w[0, :, 3].numpy() + R @ np.float32([0.0, 0.0, -0.53]), R.copy(), np.float32([40.0, 40.0, 1.0]))
    *rays0, n0, f0 = _hip(ref, 0, H, W, camera_type, obb=box)
    *rays1, n1, f1 = _hip(ref, 0, H, W, camera_type, obb=box, near_floor=0.05)
    for a, b in zip(rays0, rays1):
        assert torch.equal(a, b)
    hit, low = n0 < 1e10, n0 < 0.05
    assert 50 < int(low.sum()) < int(hit.sum()) < H * W  # all three kinds of ray are there
    assert torch.equal(f0, f1) and torch.equal(n1[~low], n0[~low]) and bool((n1[low] == 0.05).all())
    assert float(n0[hit].min()) == pytest.approx(0.03, abs=1e-3) and bool((n0[~hit] == 1e10).all()) and bool((n1[~hit] == 1e10).all())
    # the cameras of the other tests stand 3 away from their boxes: the floor changes nothing there
    ref = _reference("perspective", 20, 28, 50.0)
    a, b = _hip(ref, 0, 20, 28, "perspective", obb=ref["box"]), _hip(ref, 0, 20, 28, "perspective", obb=ref["box"], near_floor=0.05)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_refusals_return_a_code_and_write_nothing():
    """Every refusal of include/umhs_hip.h ("umhs_raygen_frame") happens on the host, before any launch: the pre-filled output
    buffers come back untouched.  Every pointer handed over is a real allocation of the right size (or NULL)."""
    from umhsnerf import _hip
    from umhsnerf._hip import ptr

    H, W, n = 20, 28, FR.N_CAMS
    c2w, intr = (t.to(DEV) for t in FR.path_cameras(H, W, 50.0, "perspective"))
    dist = RG.draw_distortion(n, 0).to(DEV)
    SENTINEL = -7.25
    bufs = {k: torch.full((H * W, c), SENTINEL, device=DEV) for k, c in (("o", 3), ("d", 3), ("area", 1), ("nrm", 1), ("nears", 1), ("fars", 1))}
    box = (ctypes.c_float * 15)(0.1, -0.05, 0.2, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.9, 0.6, 1.2)

    def call(**kw):
        a = dict(c2w=ptr(c2w), intr=ptr(intr), dist=None, n_cams=n, camera=1, type=0, H=H, W=W, row0=0, n_rows=H, obb=None, floor=0.0,
                 o=ptr(bufs["o"]), d=ptr(bufs["d"]), area=ptr(bufs["area"]), nrm=ptr(bufs["nrm"]), nears=None, fars=None, stream=_hip.stream())
        a.update(kw)
        return _hip.lib().umhs_raygen_frame(*a.values())

    both = dict(nears=ptr(bufs["nears"]), fars=ptr(bufs["fars"]))
    bad_scale = []
    for k in (12, 13, 14):
        for v in (0.0, -1.0, float("nan")):
            flat = (ctypes.c_float * 15)(*box)
            flat[k] = v
            bad_scale.append(dict(obb=flat, **both))
    refusals = [dict(c2w=None), dict(intr=None), dict(o=None), dict(d=None),           # NULL required pointers
                dict(camera=n), dict(camera=-1), dict(n_cams=0),                       # camera outside 0 .. n_cams - 1
                dict(type=3), dict(type=-1),                                           # camera_type outside 0 .. 2
                dict(dist=ptr(dist), type=1), dict(dist=ptr(dist), type=2),            # distortion with a non-perspective type
                dict(row0=H - 5, n_rows=6), dict(row0=-1), dict(n_rows=-1), dict(row0=H + 1, n_rows=0), dict(H=0), dict(W=0),  # rows
                dict(nears=ptr(bufs["nears"])), dict(fars=ptr(bufs["fars"])),           # one without the other
                dict(obb=box), dict(obb=box, nears=ptr(bufs["nears"])),                 # a box without nears / fars
                dict(floor=-0.01, obb=box, **both), *bad_scale]                         # near_floor < 0; a scale that is not positive
    for r in refusals:
        assert call(**r) != 0, r
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == SENTINEL).all()), k
    # and the same call with nothing wrong runs: rays, and with the box its nears / fars
    assert call(obb=box, **both) == 0 and call(dist=ptr(dist)) == 0 and call(type=2) == 0 and call(n_rows=0) == 0
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t != SENTINEL).all()) and bool(torch.isfinite(t).all()), k
