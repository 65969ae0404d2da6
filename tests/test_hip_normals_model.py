"""The ``normals`` output end to end on the tiny trained scene of tests/test_hip_render.py (``make_scene``, 3 classes,
``pred_specular``, three training steps): the model output against step 7 of include/umhs_hip.h restated in float64 from the kernel's
own per-sample normals and the rendering weights, an empty ray, the untouched key set and bits without the flag or the name, the
``normals`` panel of a camera-path frame byte for byte, and ``export pointcloud --normal-method``."""
import json

import numpy as np
import pytest
import torch

import normals_f64 as NF
import pointcloud_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
N_POINTS, N_RAYS = 2000, 1024
U = NF.U


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from test_hip_distortion import _look_at_origin, make_scene
    from test_hip_pointcloud import _pipeline
    from umhsnerf.render import load_camera_path

    root = tmp_path_factory.mktemp("normals")
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    pipe = _pipeline(scene, meta)
    pipe._ahead = None
    rng = np.random.default_rng(11)
    path = {"camera_type": "perspective", "render_height": H, "render_width": W, "fps": 24, "seconds": 0.125,
            "camera_path": [{"camera_to_world": _look_at_origin(rng).reshape(-1).tolist(), "fov": fov, "aspect": W / H} for fov in FOVS]}
    (root / "path.json").write_text(json.dumps(path))
    cameras, _ = load_camera_path(root / "path.json", device=DEV)
    pipe.train()
    return dict(root=root, scene=scene, pipe=pipe, cameras=cameras)


def _outputs(world, i, **kw):
    pipe = world["pipe"]
    pipe.eval()
    try:
        return pipe.model.get_outputs_for_camera_ray_bundle(world["cameras"].generate_rays(i, keep_shape=True), **kw)
    finally:
        pipe.train()


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def test_normals_equal_step_7_in_float64_from_the_kernels_own_samples(world):
    """Per component of N = sum_i w_i n_i over a ray of S samples, a float32 sum in any order is within (S + 2) u of the envelope
    sum_i |w_i n_i| (one rounding per product, at most S per partial sum chain, and the final store).  n^ = N / (|N| + 1e-10) then moves
    by at most 2 B1 / |N| + 4 u per component (B1 the L1 norm of the three bounds: the rule tests/normals_f64.py gives the sample
    normal), and (n^ + 1) / 2 halves that and adds its own two roundings of values <= 2 and <= 1: + 2 u.  Asserted on rays with
    |N| > 16 B1; a ray with no samples gives exactly 0.5."""
    from umhsnerf import ops
    from umhsnerf._ns_compat import RayBundle

    model = world["pipe"].model
    rb = world["cameras"].generate_rays(1, keep_shape=True)
    rays = RayBundle(origins=rb.origins.reshape(-1, 3), directions=rb.directions.reshape(-1, 3))
    R = H * W
    model.eval()
    model._normals_requested = True
    try:
        with torch.no_grad():
            ray_samples, ray_indices = model.sample(rays)
            out = model.get_outputs_from_samples(ray_samples, ray_indices, R)
            normal = model.field.get_normals(ray_samples).reshape(-1, 3)
            pinfo = ops.pack_info(ray_indices.long().contiguous(), R)
    finally:
        model._normals_requested = False
        model.train()
    assert out["normals"].shape == (R, 3) and out["weights"].shape[0] == normal.shape[0] > 0
    ref, mag = NF.ray_normals64(out["weights"], normal, pinfo)
    S = pinfo[:, 1].cpu().numpy().astype(np.float64)
    wt, nm = out["weights"].double().cpu().numpy().reshape(-1), normal.double().cpu().numpy()
    Nv = np.zeros((R, 3))
    np.add.at(Nv, ray_indices.cpu().numpy(), wt[:, None] * nm)
    b1 = ((S[:, None] + 2) * U * (mag + NF.TINY)).sum(1)
    length = np.linalg.norm(Nv, axis=1)
    teeth = (S > 0) & (length > 16 * b1)
    tol = (2 * b1 / np.where(teeth, length, 1.0) + 4 * U) / 2 + 2 * U
    got = out["normals"].double().cpu().numpy()
    err = np.abs(got - ref).max(1)
    print(f"{int((S > 0).sum())} of {R} rays have samples (up to {int(S.max())}), {int(teeth.sum())} with teeth; worst |normals - float64| "
          f"{err[teeth].max():.3e} = {(err / tol)[teeth].max():.3f} of its bound")
    assert teeth.sum() >= 0.9 * (S > 0).sum() and (S > 0).sum() > R // 4
    assert (err <= tol)[teeth].all()
    assert (got[S == 0] == 0.5).all()
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    # the per-sample normals are unit vectors (or exact zeros where the selector is 0)
    ln = np.linalg.norm(nm, axis=1)
    assert ((np.abs(ln - 1) < 1e-6) | (ln == 0)).all()


def test_an_empty_ray_gives_one_half(world):
    from umhsnerf._ns_compat import RayBundle

    model = world["pipe"].model
    o = torch.tensor([[0.0, 0.0, 30.0], [0.0, 0.0, -3.0]], device=DEV)  # the first looks away from the scene, from outside every grid level
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], device=DEV)
    model.eval()
    try:
        out = model.get_outputs_for_camera_ray_bundle(RayBundle(origins=o.view(1, 2, 3), directions=d.view(1, 2, 3)), output_names=["normals", "num_samples_per_ray"])
    finally:
        model.train()
    assert int(out["num_samples_per_ray"].view(-1)[0]) == 0
    assert (out["normals"].view(2, 3)[0] == 0.5).all()


def test_without_the_flag_or_the_name_nothing_changes(world):
    model = world["pipe"].model
    plain = _outputs(world, 0)
    assert "normals" not in plain and not model._normals_requested
    names = list(plain) + ["normals"]
    asked = _outputs(world, 0, output_names=names)
    assert set(asked) == set(plain) | {"normals"} and not model._normals_requested
    for k, v in plain.items():
        assert _bits_equal(v, asked[k]), k
    again = _outputs(world, 0)
    assert set(again) == set(plain) and all(_bits_equal(v, again[k]) for k, v in plain.items())
    only = _outputs(world, 0, output_names=["rgb", "depth"])
    assert set(only) == {"rgb", "depth"}
    # the config flag does what the name does
    model.config.compute_normals = True
    try:
        flagged = _outputs(world, 0)
        # ... but never while training
        rays, _ = world["pipe"].datamanager.train_split.sample(256, torch.Generator(device=DEV).manual_seed(0), want_batch=False)
        assert model.training and "normals" not in model(rays)
        # the path with gradients (eval mode, autograd on) forms the output from its own tensors
        model.eval()
        with torch.enable_grad():
            rb = world["cameras"].generate_rays(0, keep_shape=True)
            from umhsnerf._ns_compat import RayBundle

            split = model(RayBundle(origins=rb.origins.reshape(-1, 3), directions=rb.directions.reshape(-1, 3)))
        model.train()
    finally:
        model.config.compute_normals = False
        model.train()
    assert set(flagged) == set(plain) | {"normals"} and _bits_equal(flagged["normals"], asked["normals"])
    assert "normals" in split and not split["normals"].requires_grad
    hit = (plain["accumulation"].view(-1) > 0.5)
    d = (split["normals"].view(-1, 3) - asked["normals"].view(-1, 3)).abs()[hit].max()
    print(f"split path against the fused render: normals differ by at most {float(d):.3e} on {int(hit.sum())} opaque pixels")
    assert float(d) < 1e-3  # (other kernels form the weights there: not the same bits, the same picture)


def test_the_normals_panel_matches_the_frame_restatement_byte_for_byte(world):
    from test_hip_render import _png, _reference_frame
    from umhsnerf.render import render_camera_path

    names = ["rgb", "normals", "depth"]
    render_camera_path(world["pipe"], world["cameras"], world["root"] / "frames", names)
    for i in range(3):
        outputs = _outputs(world, i, output_names=["rgb", "normals", "depth", "accumulation"])
        want = _reference_frame(outputs, names=names)
        got = _png(world["root"] / "frames" / f"frame_{i:05d}.png")
        assert got.shape == (H, 3 * W, 3) and np.array_equal(got, want)
        panel = got[:, W:2 * W]
        assert panel.std() > 0  # not a flat grey panel


def test_normals_face_the_camera(world):
    """One check with physical meaning: over pixels with accumulation > 0.5 the median of n^ . ray direction is negative (the density
    rises along the ray where it enters the surface, and the normal is -grad)."""
    dots = []
    for i in range(3):
        rb = world["cameras"].generate_rays(i, keep_shape=True)
        out = _outputs(world, i, output_names=["normals", "accumulation"])
        n = out["normals"].view(-1, 3) * 2 - 1
        hit = out["accumulation"].view(-1) > 0.5
        dots.append(((n * rb.directions.view(-1, 3)).sum(-1))[hit])
    dots = torch.cat(dots)
    print(f"{dots.numel()} opaque pixels: median n.d {float(dots.median()):.3f}, share facing the camera {float((dots < 0).float().mean()):.3f}")
    assert dots.numel() > 100 and float(dots.median()) < 0


def _normal_columns(table):
    return np.stack([table["nx"], table["ny"], table["nz"]], 1)


def test_export_with_analytic_normals(world):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    kw = dict(num_points=N_POINTS, num_rays_per_batch=N_RAYS)
    none = export.export_pointcloud(pipe, root / "pc_none", **kw)
    default = export.export_pointcloud(pipe, root / "pc_default", normal_method="none", **kw)
    assert (root / "pc_none" / "point_cloud.ply").read_bytes() == (root / "pc_default" / "point_cloud.ply").read_bytes()
    res = export.export_pointcloud(pipe, root / "pc_analytic", normal_method="analytic", **kw)
    assert pipe.model.training and not pipe.model._normals_requested
    assert {**res, "file": ""} == {**none, "file": ""}
    table, raw = P.read_ply(res["file"])
    t0, raw0 = P.read_ply(none["file"])
    assert list(table.dtype.names) == ["x", "y", "z", "nx", "ny", "nz"] + list(t0.dtype.names)[3:]
    assert np.array_equal(np.concatenate([raw[:, :12], raw[:, 24:]], 1), raw0)  # every other byte is the file without normals
    n = _normal_columns(table)
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 1e-6
    # they equal the gathered outputs: the same batches replayed (no outlier removal: the first N_POINTS kept rays in draw order)
    all_rows = export.export_pointcloud(pipe, root / "pc_all", normal_method="analytic", remove_outliers=False, **kw)
    ta, rawa = P.read_ply(all_rows["file"])
    split, model = pipe.datamanager.train_split, pipe.model
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    model.eval()
    model._normals_requested = True
    want = []
    try:
        with torch.no_grad():
            for b in range(all_rows["batches"]):
                rays, _ = split.sample(N_RAYS, gen, want_batch=False)
                out = model(rays)
                h = lambda t: t.float().cpu().numpy()
                _, _, kept = P.emit(h(rays.origins), h(rays.directions), h(out["depth"]), h(out["accumulation"]), h(out["rgb"]),
                                    h(out["abundances"]), h(out["seg_probs"]), 0.5, None, None, b * N_RAYS)
                want.append((out["normals"][torch.from_numpy(kept - b * N_RAYS).to(DEV)] * 2.0 - 1.0).cpu().numpy())
    finally:
        model._normals_requested = False
        model.train()
    want = np.concatenate(want)[:N_POINTS]
    assert len(ta) == N_POINTS and np.array_equal(_normal_columns(ta), want)
    # with outlier removal: the same mask as every other column (rows are found again by their bytes)
    index = {bytes(r): i for i, r in enumerate(rawa)}  # (a ray drawn twice gives two identical rows, normals included: either will do)
    assert np.array_equal(n, want[[index[bytes(r)] for r in raw]])
    # --material applies the same mask
    m1 = export.export_pointcloud(pipe, root / "pc_m1", normal_method="analytic", material=1, **kw)
    tm, rawm = P.read_ply(m1["file"])
    assert np.array_equal(rawm, raw[table["material"] == 1])


def test_export_world_frame_rotates_normals_and_does_not_translate_them(world):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    kw = dict(num_points=500, num_rays_per_batch=N_RAYS, normal_method="analytic")
    model_frame = export.export_pointcloud(pipe, root / "wf_model", **kw)
    out = pipe.datamanager.train_dataparser_outputs
    saved = (out.dataparser_transform, out.dataparser_scale)
    a, b = 0.6, 0.8  # a rotation about z, a shift and a scale: the affine back to the original frame is R^T / 0.5 and a translation
    out.dataparser_transform = torch.tensor([[a, -b, 0.0, 0.3], [b, a, 0.0, -0.2], [0.0, 0.0, 1.0, 0.5]])
    out.dataparser_scale = 0.5
    try:
        A = export.world_frame_affine(out.dataparser_transform, out.dataparser_scale)
        res = export.export_pointcloud(pipe, root / "wf_world", save_world_frame=True, **kw)
    finally:
        out.dataparser_transform, out.dataparser_scale = saved
    tm, rawm = P.read_ply(model_frame["file"])
    tw, raww = P.read_ply(res["file"])
    assert np.array_equal(raww[:, 24:], rawm[:, 24:]) and len(tw) == len(tm)
    xyz = np.stack([tm["x"], tm["y"], tm["z"]], 1)
    assert np.array_equal(np.stack([tw["x"], tw["y"], tw["z"]], 1), P.world_of(xyz, A))  # the points: rotated, scaled AND translated
    n, nw = _normal_columns(tm).astype(np.float64), _normal_columns(tw).astype(np.float64)
    Rm = np.array([[a, b, 0.0], [-b, a, 0.0], [0.0, 0.0, 1.0]])  # R^T: the linear part of A without its scale
    assert np.abs(nw - n @ Rm.T).max() <= 1e-6
    assert np.abs(np.linalg.norm(nw, axis=1) - 1).max() <= 1e-6


def test_the_command_line_writes_normals(world, capsys):
    from test_hip_pointcloud import FLAGS
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    torch.save({"step": 3, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    want = export.export_pointcloud(pipe, root / "cli_want", num_points=500, num_rays_per_batch=N_RAYS, normal_method="analytic")
    got = export.main(["pointcloud", "--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"), "--output-dir",
                       str(root / "cli"), "--num-points", "500", "--num-rays-per-batch", str(N_RAYS), "--normal-method", "analytic", *FLAGS])
    capsys.readouterr()
    assert got == {**want, "file": str(root / "cli" / "point_cloud.ply")}
    assert (root / "cli" / "point_cloud.ply").read_bytes() == (root / "cli_want" / "point_cloud.ply").read_bytes()


def test_the_rgb_method_gets_the_output_the_same_way():
    """method="rgb" (UMHSRGBField has the same mlp_base): the output appears with the flag, is absent without it, and is step 7 on the
    field's own per-sample normals and the path's own weights."""
    from umhsnerf import ops
    from umhsnerf._ns_compat import RayBundle
    from umhsnerf.umhs_model import UMHSConfig

    m = UMHSConfig(log2_hashmap_size=14).setup(scene_box=None, num_train_data=1, metadata={"wavelengths": list(range(8)), "num_classes": 6},
                                               num_classes=6, seed=5).to(DEV)
    g = torch.Generator().manual_seed(0)
    o = torch.tensor([0.0, 0.0, -3.0]).repeat(64, 1) + 0.01 * torch.randn(64, 3, generator=g)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]).repeat(64, 1) + 0.1 * torch.randn(64, 3, generator=g), dim=-1)
    rays = RayBundle(origins=o.to(DEV), directions=d.to(DEV))
    m.train()
    m.update_occupancy_grid(0)
    assert "normals" not in m(rays)
    m.eval()
    with torch.no_grad():
        plain = m(rays)
        m.config.compute_normals = True
        ray_samples, ray_indices = m.sample(rays)
        out = m.get_outputs_from_samples(ray_samples, ray_indices, 64)
        normal = m.field.get_normals(ray_samples).reshape(-1, 3)
        want = ops.ray_normals(out["weights"], normal, ops.pack_info(ray_indices.long().contiguous(), 64))
    assert "normals" not in plain and set(out) == set(plain) | {"normals"}
    assert out["normals"].shape == (64, 3) and _bits_equal(out["normals"], want)
    assert bool(torch.isfinite(out["normals"]).all()) and float(out["normals"].min()) >= 0 and float(out["normals"].max()) <= 1
    assert float((out["normals"] - 0.5).abs().max()) > 0.01
