"""Textured mesh export on the GPU.

Kernels: ``umhs_texture_rays`` / ``umhs_texture_uv`` (``ops.texture_rays`` / ``ops.texture_uv``) must give the float32 replay of
tests/texture_ref.py bit for bit -- origins, directions, nears, fars, texel_face and bary -- on a tetrahedron, on a mesh with dead
faces and on the marching-tetrahedra sphere; a range split anywhere concatenates to the same bits and the words behind every output
stay untouched.  The definition itself is held to its float64 evaluation within a derived bound.
End to end: the tiny scene of tests/test_hip_mesh.py (``make_scene``, 3 classes, ``pred_specular``), trained for N_STEPS steps."""
import contextlib
import json

import numpy as np
import pytest
import torch

import texture_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 5
FLOATS = ("origins", "directions", "nears", "fars", "bary")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _mesh(name):
    if name == "tetrahedron":
        return R.tetrahedron()
    if name == "dead":
        return R.dead_mesh()[:2]
    return _sphere()


_cache = {}


def _sphere():
    if "sphere" not in _cache:
        _cache["sphere"] = R.sphere_mesh(12)
    return _cache["sphere"]


def _run(pos, faces, p, L, begin=0, end=None, guard=GUARD):
    from umhsnerf import ops

    out = ops.texture_rays(torch.from_numpy(pos).to(DEV), torch.from_numpy(faces).to(DEV), p, L, begin, end, want_bary=True, guard=guard)
    host = {k: out[k].cpu().numpy() for k in (*FLOATS, "texel_face")}
    host["nears"], host["fars"] = host["nears"][:, 0], host["fars"][:, 0]
    if guard:
        n = len(host["texel_face"])
        for k, cols in (("origins", 3), ("directions", 3), ("nears", 1), ("fars", 1), ("bary", 3)):
            tail = out["buffers"][k].cpu().numpy()[n * cols:]
            assert len(tail) == guard and np.isnan(tail).all(), k
        tail = out["buffers"]["texel_face"].cpu().numpy()[n:]
        assert len(tail) == guard and (tail.view(np.uint32) == 0xA5A5A5A5).all()
    return host


def _assert_equal(got, want, what):
    for k in (*FLOATS, "texel_face"):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        same = _bits(got[k]) == _bits(want[k])
        assert same.all(), (what, k, int((~same).sum()), np.argwhere(~same)[:4].tolist())


# ---- the kernels against the replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [("tetrahedron", 4), ("tetrahedron", 7), ("dead", 4), ("dead", 6), ("sphere", 4), ("sphere", 5)])
def test_rays_and_uv_equal_the_float32_replay(name, p):
    from umhsnerf import ops

    pos, faces = _mesh(name)
    L = 0.37
    want = R.rays(pos, faces, p, L)
    got = _run(pos, faces, p, L)
    _assert_equal(got, want, name)
    Q, T = R.atlas(len(faces), p)
    assert len(got["texel_face"]) == T * T
    assert np.array_equal(got["texel_face"].reshape(T, T) >= 0, (R.owner_map(len(faces), p) >= 0) & (want["texel_face"].reshape(T, T) >= 0))
    live = got["texel_face"] >= 0
    assert live.any() and (got["nears"][live] == 0).all() and (got["fars"][live] == np.float32(L)).all()
    miss = ~live
    if miss.any():  # as the crop path writes a miss
        assert (got["origins"][miss] == 0).all() and (got["directions"][miss] == np.array([0, 0, 1], np.float32)).all()
        assert (got["nears"][miss] == np.float32(1e10)).all() and (got["fars"][miss] == np.float32(1e10)).all() and (got["bary"][miss] == 0).all()
    uv = ops.texture_uv(len(faces), p, DEV).cpu().numpy()
    assert np.array_equal(_bits(uv), _bits(R.uv(len(faces), p)))
    if name == "dead":
        dead = R.dead_mesh()[2]
        assert not np.isin(got["texel_face"], dead).any() and set(np.unique(got["texel_face"]).tolist()) == {-1, 0, 2, 5}
        own = R.owner_map(len(faces), p).reshape(-1)
        assert (got["texel_face"][np.isin(own, dead)] == -1).all() and (own == -1).any()  # (F = 7: half of the last square is empty)
    if name == "sphere":
        assert 200 <= len(faces) <= 2000 and T * T > 4 * 256  # several workgroups, the last partial
        assert np.array_equal(np.unique(got["texel_face"][live]), np.arange(len(faces)))


@pytest.mark.parametrize("p", [4, 5])
def test_split_ranges_concatenate_to_the_same_bits(p):
    pos, faces = _sphere()
    L = 0.21
    Q, T = R.atlas(len(faces), p)
    n = T * T
    whole = _run(pos, faces, p, L)
    cuts = [0, 1, 777, n - 251, n]
    assert all(c % p and c % T and c % 64 for c in cuts[1:-1]) and n > 2000
    parts = [_run(pos, faces, p, L, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    joined = {k: np.concatenate([q[k] for q in parts]) for k in whole}
    _assert_equal(joined, whole, f"split p={p}")
    _assert_equal(parts[2], R.rays(pos, faces, p, L, 777, n - 251), "middle range")
    empty = _run(pos, faces, p, L, 123, 123)
    assert all(len(v) == 0 for v in empty.values())


def test_arguments_are_checked_in_python():
    from umhsnerf import ops

    pos, faces = R.tetrahedron()
    dp, df = torch.from_numpy(pos).to(DEV), torch.from_numpy(faces).to(DEV)
    T = R.atlas(4, 4)[1]
    for bad in (lambda: ops.texture_rays(dp, df, 3, 0.1), lambda: ops.texture_rays(dp, df, 4, 0.0), lambda: ops.texture_rays(dp, df, 4, float("nan")),
                lambda: ops.texture_rays(dp, df, 4, 0.1, 0, T * T + 1), lambda: ops.texture_rays(dp, df, 4, 0.1, 5, 4),
                lambda: ops.texture_rays(dp, df.long(), 4, 0.1), lambda: ops.texture_rays(dp.double(), df, 4, 0.1),
                lambda: ops.texture_rays(dp[:, :2], df, 4, 0.1), lambda: ops.texture_rays(dp, df[:0], 4, 0.1),
                lambda: ops.texture_uv(4, 3, DEV), lambda: ops.texture_uv(0, 4, DEV)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.texture_rays(torch.from_numpy(pos), df, 4, 0.1)
    with pytest.raises(RuntimeError):
        ops.texture_uv(4, 4, "cpu")
    assert ops.texture_rays(dp, df, 4, 0.1)["bary"] is None


# ---- the definition against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 5])
def test_the_definition_agrees_with_float64(p):
    """Per live texel, gutter included.  The surface point: origin - (L / 2) n^ (float64 arithmetic on the kernel's float32 values)
    against the float64 barycentric point within 4 * 2^-23 * sum_k |w_k| |V_kc| per component -- one rounding each for w_k, the
    product and two sums, 4 * 2^-24 to first order, doubled for the offset that the origin adds and this test takes off again.
    The direction: a unit vector within 4 * 2^-23 (sum of squares, sqrt, division: a few roundings of 2^-24 each), and antiparallel to
    the float64 normal: each component of a and b carries one rounding, each product one, the difference one, so a component of the
    float32 cross product is within 4 * 2^-24 |a| |b| of the float64 one (|a_i b_j| + |a_j b_i| <= |a| |b|), the vector within
    4 sqrt(3) 2^-24 |a| |b|, and normalising a vector perturbed by eps turns it by at most 2 |eps| / |n|."""
    pos, faces = _sphere()
    L = np.float32(0.29)
    got = _run(pos, faces, p, float(L), guard=0)
    r64 = R.rays(pos, faces, p, L, F=np.float64)
    live = got["texel_face"] >= 0
    assert np.array_equal(got["texel_face"], r64["texel_face"]) and live.sum() > 1000
    o, d = got["origins"][live].astype(np.float64), got["directions"][live].astype(np.float64)
    point = o + (0.5 * float(L)) * d  # (direction = -n^)
    bound = 4 * 2.0 ** -23 * r64["mag"][live]
    err = np.abs(point - r64["point"][live])
    gutter = (got["bary"][live].min(1) < 0)
    norm_err = np.abs(np.linalg.norm(d, axis=1) - 1.0)
    f = got["texel_face"][live]
    v = pos.astype(np.float64)[faces[f]]
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n64 = np.cross(a, b)
    turn = 8 * np.sqrt(3.0) * 2.0 ** -24 * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) / np.linalg.norm(n64, axis=1) + 4 * 2.0 ** -23
    anti = np.linalg.norm(d + r64["normal"][live], axis=1)
    print(f"p {p}: {int(live.sum())} live texels ({int(gutter.sum())} in the gutter), worst point error / bound {float((err / bound).max()):.3f}, "
          f"worst | |d| - 1 | {float(norm_err.max()):.3g} of {4 * 2.0 ** -23:.3g}, worst |d + n64| / bound {float((anti / turn).max()):.3f}")
    assert gutter.any() and (err <= bound).all()
    assert (norm_err <= 4 * 2.0 ** -23).all()
    assert (np.einsum("ij,ij->i", d, n64) < 0).all() and (anti <= turn).all()
    # the ray starts half its length outside (the sphere's faces look outwards) and runs through the surface
    centre_side = np.einsum("ij,ij->i", r64["point"][live][~gutter], d[~gutter])
    assert (centre_side < 0).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
N_STEPS, RES = 3, 24  # tests/test_hip_mesh.py's: the fewest steps of this scene and seed that leave a surface inside the box
BAND_TEXELS = 1500  # several bands of whole rows in an atlas of a few thousand texels
FLAGS = ["--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"]
NAMES, CUBES = ("rgb", "seg_pred"), ("abundances",)
KW = dict(resolution=RES, downscale_factor=1, batch_size=4)


@contextlib.contextmanager
def _small_bands():
    """The atlas walk in bands of BAND_TEXELS texels instead of 2^20 (every export of this file, so that equal files mean equal code
    on equal batches of rays)."""
    from umhsnerf import export

    default, export.TEXTURE_BAND_TEXELS = export.TEXTURE_BAND_TEXELS, BAND_TEXELS
    try:
        yield
    finally:
        export.TEXTURE_BAND_TEXELS = default


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from test_hip_distortion import make_scene
    from test_hip_render import _datamanager
    from umhsnerf import export
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("texture")
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    torch.manual_seed(0)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2,
                                            datamanager=_datamanager(scene, 9))
    for step in range(N_STEPS):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    dm = pipe.datamanager
    state = lambda: dict(gen=dm.generator.get_state().clone(), cursor=dm._eval_cursor, train_count=dm.train_count,
                         cuda=torch.cuda.get_rng_state(DEV).clone(), cpu=torch.get_rng_state().clone(), training=pipe.model.training)
    pipe.train()
    before = state()
    with _small_bands():
        result = export.export_textured_mesh(pipe, root / "out", px_per_uv_triangle=4, texture_output_names=NAMES, cube_output_names=CUBES, **KW)
    return dict(root=root, scene=scene, pipe=pipe, before=before, after=state(), result=result)


def _png(path):
    from PIL import Image

    return np.array(Image.open(path))


def test_export_writes_a_consistent_textured_mesh(world):
    import mesh_ref as M
    from umhsnerf import export

    res, root, pipe = world["result"], world["root"], world["pipe"]
    out = root / "out"
    assert set(res) == {"vertices", "faces", "atlas_side", "px_per_uv_triangle", "ray_length", "textures", "cubes", "file"}
    assert res["file"] == str(out / "mesh.obj") and res["px_per_uv_triangle"] == 4
    assert res["textures"] == {"rgb": str(out / "material_0.png"), "seg_pred": str(out / "texture_seg_pred.png")}
    assert res["cubes"] == {"abundances": str(out / "texture_abundances.npy")}
    assert sorted(q.name for q in out.iterdir()) == ["material_0.mtl", "material_0.png", "mesh.obj", "texture_abundances.npy", "texture_seg_pred.png"]
    obj = R.read_textured_obj(res["file"])
    F, T = res["faces"], res["atlas_side"]
    print(f"textured mesh after {N_STEPS} steps: {res['vertices']} vertices, {F} faces, atlas {T} x {T}, ray length {res['ray_length']:.4f}, "
          f"{len(export.texture_bands(T, BAND_TEXELS))} bands")
    assert F > 0 and len(obj["f"]) == F and len(obj["vt"]) == 3 * F and len(obj["v"]) == res["vertices"]
    assert (R.atlas(F, 4)[1] == T) and len(export.texture_bands(T, BAND_TEXELS)) > 1
    assert obj["mtllib"] == "material_0.mtl" and R.read_mtl(out / "material_0.mtl") == {"newmtl": "material_0", "map_Kd": "material_0.png"}
    assert np.array_equal(obj["ft"], np.arange(3 * F).reshape(F, 3)) and np.array_equal(_bits(obj["vt"]), _bits(R.uv(F, 4).reshape(-1, 2)))
    # the same mesh as export_tsdf_mesh's, whose bytes are those of the code path before the two exports shared a helper
    ply = export.export_tsdf_mesh(pipe, root / "ply", **KW)
    table, rows, faces = M.read_mesh_ply(ply["file"])
    assert np.array_equal(obj["f"], faces) and np.array_equal(_bits(obj["v"]), _bits(np.stack([table["x"], table["y"], table["z"]], 1)))
    assert (root / "ply" / "mesh.ply").read_bytes() == _parent_mesh_ply(pipe)
    # ray length: twice the mean length of the first edge
    e = obj["v"].astype(np.float64)[obj["f"][:, 1]] - obj["v"].astype(np.float64)[obj["f"][:, 0]]
    assert res["ray_length"] == float(np.float32(res["ray_length"])) == pytest.approx(2 * np.linalg.norm(e, axis=1).mean(), rel=1e-6)
    for name in NAMES:
        img = _png(res["textures"][name])
        assert img.shape == (T, T, 3) and img.dtype == np.uint8
    cube = np.load(res["cubes"]["abundances"])
    assert cube.shape == (T, T, 3) and cube.dtype == np.float32


def _parent_mesh_ply(pipe) -> bytes:
    """``mesh.ply`` as export_tsdf_mesh composed it before the fuse-and-extract helper: the same operators called in line."""
    import io

    from umhsnerf import export, ops

    model, split = pipe.model, pipe.datamanager.train_split
    lo, h, dims = export.tsdf_lattice((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), RES)
    trunc = float(np.float32(5.0 * h))
    cams = export.tsdf_cameras(split, 1)
    names = ["depth", "rgb", "accumulation", "abundances", "seg_probs"]
    was = model.training
    model.eval()
    vol = None
    try:
        with torch.no_grad():
            for b in range(0, cams["n"], 4):
                e = min(b + 4, cams["n"])
                o = export.render_cameras(model, cams, b, e, names)
                if vol is None:
                    vol = ops.tsdf_volume(lo, h, dims, o["abundances"].shape[-1], split.device)
                ops.tsdf_integrate(vol, cams["c2w_host"][b:e], cams["intrinsics_host"][b:e], None if cams["distortion_host"] is None
                                   else cams["distortion_host"][b:e], o["depth"], o["accumulation"], o["rgb"], o["abundances"], o["seg_probs"],
                                   0.5, trunc)
    finally:
        model.train(was)
    mesh = ops.mesh_extract(vol, None)
    frows = np.empty((mesh["faces"].shape[0], 13), np.uint8)
    frows[:, 0] = 3
    frows[:, 1:] = mesh["faces"].cpu().numpy().view(np.uint8).reshape(-1, 12)
    buf = io.BytesIO()
    buf.write(export.mesh_ply_header(mesh["rows"].shape[0], mesh["faces"].shape[0], mesh["n_classes"]))
    buf.write(mesh["rows"].cpu().numpy().tobytes())
    buf.write(frows.tobytes())
    return buf.getvalue()


def test_textures_equal_the_model_rendered_by_hand_on_the_replayed_rays(world):
    """The rays replayed by tests/texture_ref.py from the written mesh, rendered through ``get_outputs_for_camera_ray_bundle`` in the
    same bands and composed by ``render.compose_frame``: same code, same rays, equal bytes.  Texels nobody owns are 0."""
    from umhsnerf import export
    from umhsnerf._ns_compat import RayBundle
    from umhsnerf.render import compose_frame, source_keys

    res, pipe = world["result"], world["pipe"]
    model = pipe.model
    obj = R.read_textured_obj(res["file"])
    T, L = res["atlas_side"], res["ray_length"]
    want = R.rays(obj["v"], obj["f"].astype(np.int32), 4, L)
    owned = want["texel_face"].reshape(T, T) >= 0
    assert owned.any() and not owned.all()
    hand = {name: torch.zeros(T, T, 3, dtype=torch.uint8, device=DEV) for name in NAMES}
    cube = torch.zeros(T, T, 3, device=DEV)
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            for r0, r1 in export.texture_bands(T, BAND_TEXELS):
                up = lambda k, c: torch.from_numpy(np.ascontiguousarray(want[k][r0 * T:r1 * T])).to(DEV).view(r1 - r0, T, c)
                rb = RayBundle(origins=up("origins", 3), directions=up("directions", 3), nears=up("nears", 1), fars=up("fars", 1))
                outputs = model.get_outputs_for_camera_ray_bundle(rb, output_names=source_keys(NAMES, CUBES))
                for name in NAMES:
                    compose_frame(outputs, [name], depth_near_plane=0.0, depth_far_plane=L, out=hand[name][r0:r1])
                cube[r0:r1] = outputs["abundances"]
    finally:
        model.train(was)
    mask = torch.from_numpy(owned).to(DEV)
    differ = 0
    for name in NAMES:
        img = _png(res["textures"][name])
        assert (img[~owned] == 0).all(), name
        assert np.array_equal(img[owned], hand[name][mask].cpu().numpy()), name
        differ += int(len(np.unique(img[owned].reshape(-1, 3), axis=0)) > 1)
    assert differ  # (not one flat colour everywhere: the texture shows the model)
    got = np.load(res["cubes"]["abundances"])
    assert (got[~owned] == 0).all() and np.array_equal(got[owned].view(np.uint32), cube[mask].cpu().numpy().view(np.uint32))


def test_export_leaves_the_training_state_alone(world):
    pipe, before, after = world["pipe"], world["before"], world["after"]
    dm = pipe.datamanager
    assert before["training"] and after["training"]
    assert torch.equal(after["gen"], before["gen"]) and after["cursor"] == before["cursor"] and after["train_count"] == before["train_count"]
    assert torch.equal(after["cuda"], before["cuda"]) and torch.equal(after["cpu"], before["cpu"])
    assert torch.equal(dm.generator.get_state(), before["gen"]) and dm._eval_cursor == before["cursor"] and dm.train_count == before["train_count"]
    assert pipe.model.training and pipe.model._material_edits is None


def test_world_frame_moves_only_the_written_positions(world):
    from umhsnerf import export

    root, pipe, res = world["root"], world["pipe"], world["result"]
    with _small_bands():
        wf = export.export_textured_mesh(pipe, root / "wf", px_per_uv_triangle=4, texture_output_names=("rgb",), save_world_frame=True, **KW)
    a, b = R.read_textured_obj(res["file"]), R.read_textured_obj(wf["file"])
    out = pipe.datamanager.train_dataparser_outputs
    A = export.world_frame_affine(out.dataparser_transform, out.dataparser_scale)
    p = a["v"]
    want = np.stack([((A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]) + A[r, 3] for r in range(3)], 1).astype(np.float32)
    assert np.array_equal(_bits(b["v"]), _bits(want)) and np.array_equal(a["f"], b["f"]) and np.array_equal(_bits(a["vt"]), _bits(b["vt"]))
    assert wf["ray_length"] == res["ray_length"] and wf["cubes"] == {}
    assert np.array_equal(_png(wf["textures"]["rgb"]), _png(res["textures"]["rgb"]))  # the rays are the model frame's


def test_a_removed_material_changes_the_texture(world):
    """``--material-edits`` with a removal: the texture is the edited scene's.  The material removed is the one most vertices of the
    unedited mesh are labelled with."""
    import mesh_ref as M
    from umhsnerf import export
    from umhsnerf.materials import load_for_model

    root, pipe, res = world["root"], world["pipe"], world["result"]
    table, _, _ = M.read_mesh_ply(export.export_tsdf_mesh(pipe, root / "ply_for_labels", **KW)["file"])
    removed = int(np.bincount(table["material"][table["material"] >= 0], minlength=3).argmax())
    edits = load_for_model({"materials": [{"material": removed, "density": 0.0}]}, pipe.model)
    with pipe.model.material_edits_context(edits), _small_bands():
        ed = export.export_textured_mesh(pipe, root / "edited", px_per_uv_triangle=4, texture_output_names=("rgb",), **KW)
    assert pipe.model._material_edits is None
    a, b = _png(res["textures"]["rgb"]), _png(ed["textures"]["rgb"])
    print(f"material {removed} removed: {ed['faces']} faces (unedited {res['faces']}), atlas {ed['atlas_side']} (unedited {res['atlas_side']})")
    assert a.shape != b.shape or not np.array_equal(a, b)


def test_the_command_line_writes_the_same_files_from_a_checkpoint(world, capsys):
    from umhsnerf import export

    root, pipe, res = world["root"], world["pipe"], world["result"]
    torch.save({"step": N_STEPS, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    capsys.readouterr()
    with _small_bands():
        got = export.main(["textured-mesh", "--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"), "--output-dir",
                           str(root / "cli"), "--resolution", str(RES), "--downscale-factor", "1", "--batch-size", "4", "--px-per-uv-triangle",
                           "4", "--texture-output-names", *NAMES, "--cube-output-names", *CUBES, *FLAGS])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    swap = lambda s: s.replace(str(root / "out"), str(root / "cli"))
    assert got == {**res, "file": swap(res["file"]), "textures": {k: swap(v) for k, v in res["textures"].items()},
                   "cubes": {k: swap(v) for k, v in res["cubes"].items()}}
    for q in sorted((root / "out").iterdir()):
        assert (root / "cli" / q.name).read_bytes() == q.read_bytes(), q.name
