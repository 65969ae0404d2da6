"""Mesh components on the GPU: ``ops.mesh_components`` / ``ops.mesh_keep_components`` (csrc/umhs_components.hip) against the numpy
restatement of tests/components_ref.py -- component ids, counts, faces, the vertex map and row bytes with ``==``, areas within the bound
of the float64 oracle derived there, the guard rows untouched, two runs the same bytes -- and the cleaning stage of both mesh exports
end to end on the tiny scene of tests/test_hip_mesh.py."""
import numpy as np
import pytest
import torch

import components_ref as R
import mesh_ref as M
import simplify_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_ROWS = 3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _device(rows, faces):
    return torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), torch.from_numpy(np.ascontiguousarray(faces)).to(DEV)


def _label(rows, faces, C, **kw):
    from umhsnerf import ops

    d_rows, d_faces = _device(rows, faces)
    got = ops.mesh_components(d_rows, d_faces, C, **kw)
    host = {k: got[k].cpu().numpy() for k in ("vertex_component", "face_component", "faces", "vertices", "area")}
    host["n_components"], host["rounds"] = got["n_components"], got["rounds"]
    return got, host


# ---- labelling and statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_components_equal_the_restatement(name):
    """random: 15- and 43-byte rows, 15,856 components, pieces that cross chunk borders; the permuted strip: deep chains; the fan: every
    face lowers one word; strips of chunk - 1, chunk and chunk + 1 faces; the hand-made mesh: every rule of the header."""
    from umhsnerf import ops

    assert R.CHUNK == ops.COMPONENTS_CHUNK
    rows, faces, C, want = R.case(name)
    _, got = _label(rows, faces, C)
    cap = ops.components_round_cap(len(rows))
    area64, bound = R.area_oracle(rows, faces, C, want["face_component"], want["n_components"])
    err = np.abs(got["area"] - area64)
    print(f"{name}: {len(rows)} vertices, {len(faces)} faces, {got['n_components']} components, {got['rounds']} rounds (cap {cap}), worst area "
          f"error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}, areas bit-equal to the restatement: "
          f"{bool(np.array_equal(got['area'].view(np.uint64), want['area'].view(np.uint64)))}")
    assert got["n_components"] == want["n_components"] and 1 <= got["rounds"] < cap
    assert got["vertex_component"].dtype == np.int32 and np.array_equal(got["vertex_component"], want["vertex_component"])
    assert got["face_component"].dtype == np.int32 and np.array_equal(got["face_component"], want["face_component"])
    assert got["faces"].dtype == np.int64 and np.array_equal(got["faces"], want["faces"])
    assert got["vertices"].dtype == np.int64 and np.array_equal(got["vertices"], want["vertices"])
    assert got["area"].dtype == np.float64 and (err <= bound).all()
    _, again = _label(rows, faces, C)
    for k in ("vertex_component", "face_component", "faces", "vertices", "area"):
        assert np.array_equal(again[k].view(np.uint8), got[k].view(np.uint8)), k  # two runs, the same bytes
    if name.startswith("random"):
        assert got["n_components"] == 15856 and int(got["faces"].max()) == 2502
    if name in ("sphere", "two_spheres", "permuted_strip", "fan") or name.startswith("strip"):
        assert got["n_components"] == 1 and int(got["faces"][0]) == len(faces) and int(got["vertices"][0]) == len(rows)
    if name == "interleaved_strips":
        assert got["n_components"] == 2 and got["vertex_component"][:4].tolist() == [0, 1, 0, 1]
    if name.startswith("hand"):
        assert got["face_component"].tolist() == [0, 0, 0, 2, 3, 4, -1, -1, -1, 0, 4] and got["area"][4] == 0.0


@pytest.mark.parametrize("per", [1, 32])
def test_the_rounds_per_read_do_not_change_the_labels(per):
    rows, faces, C, want = R.case("permuted_strip")
    _, got = _label(rows, faces, C, rounds_per_read=per)
    _, base = _label(rows, faces, C)
    print(f"permuted strip, {per} rounds per read: {got['rounds']} rounds ({base['rounds']} at the default)")
    assert np.array_equal(got["vertex_component"], want["vertex_component"])  # (how many rounds it takes may depend on the schedule)


def test_the_round_cap_raises(monkeypatch):
    """A cap below what the mesh needs: RuntimeError, never a partial result."""
    from umhsnerf.ops import export as ops_export

    rows, faces, C, _ = R.case("permuted_strip")
    monkeypatch.setattr(ops_export, "components_round_cap", lambda V: 1)
    with pytest.raises(RuntimeError, match="still lowered"):
        ops_export.mesh_components(*_device(rows, faces), C)


def test_empty_inputs_and_refused_arguments():
    from umhsnerf import ops

    rows, faces = R.hand_mesh(3)
    d_rows, d_faces = _device(rows, faces)
    got = ops.mesh_components(d_rows[:0], d_faces, 3)  # no vertex: every face is invalid
    assert got["n_components"] == 0 and got["rounds"] == 0 and got["vertex_component"].shape == (0,) and got["faces"].shape == (0,)
    assert got["face_component"].tolist() == [-1] * len(faces) and got["area"].dtype == torch.float64
    out = ops.mesh_keep_components(d_rows[:0], d_faces, 3, got, torch.zeros(0, dtype=torch.uint8, device=DEV), guard_rows=GUARD_ROWS)
    assert out["rows"].shape == (0, 31) and out["faces"].shape == (0, 3) and (out["rows_buffer"] == 0xA5).all()
    got = ops.mesh_components(d_rows, d_faces[:0], 3)  # no face: every vertex its own component, no round
    V = len(rows)
    assert got["n_components"] == V and got["rounds"] == 0 and got["vertex_component"].tolist() == list(range(V))
    assert got["faces"].tolist() == [0] * V and got["vertices"].tolist() == [1] * V and got["area"].tolist() == [0.0] * V
    out = ops.mesh_keep_components(d_rows, d_faces[:0], 3, got, torch.ones(V, dtype=torch.uint8, device=DEV))
    assert out["rows"].shape == (0, 31) and out["faces"].shape == (0, 3) and out["positions"].shape == (0, 3) and (out["vertex_map"] == -1).all()
    comps = ops.mesh_components(d_rows, d_faces, 3)
    keep = torch.ones(comps["n_components"], dtype=torch.uint8, device=DEV)
    for bad in (lambda: ops.mesh_components(d_rows, d_faces, 0), lambda: ops.mesh_components(d_rows, d_faces.long(), 3),
                lambda: ops.mesh_components(d_rows, d_faces, 16), lambda: ops.mesh_components(d_rows, d_faces, 3, rounds_per_read=33),
                lambda: ops.mesh_keep_components(d_rows, d_faces, 3, comps, keep[:-1]),
                lambda: ops.mesh_keep_components(d_rows, d_faces, 3, comps, keep.float()),
                lambda: ops.mesh_keep_components(d_rows, d_faces[:-1], 3, comps, keep),
                lambda: ops.mesh_keep_components(d_rows, d_faces, 3, comps, keep, world=np.eye(4))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mesh_components(torch.from_numpy(rows), d_faces, 3)


# ---- emit ----------------------------------------------------------------------------------------------------------------------------
def _keep_for(name, want):
    if name.startswith("random"):
        return R.keep_mask(want["faces"], min_component_faces=8)
    if name.startswith("hand"):
        return np.isin(np.arange(want["n_components"]), (0, 1, 4, 5))  # two with faces, one isolated vertex, one named by invalid faces only
    if name == "interleaved_strips":
        return np.array([False, True])
    return np.ones(want["n_components"], bool)


@pytest.mark.parametrize("use_world", [False, True])
@pytest.mark.parametrize("name", ["random_c0", "random_c3", "hand_c0", "hand_c3", "interleaved_strips", "sphere", "strip_chunk_plus_1"])
def test_the_emit_equals_the_restatement(name, use_world):
    from umhsnerf import ops

    rows, faces, C, want_c = R.case(name)
    world = M.WORLD if use_world else None
    keep = _keep_for(name, want_c)
    want = R.emit(rows, faces, C, want_c, keep, world)
    d_rows, d_faces = _device(rows, faces)
    comps = ops.mesh_components(d_rows, d_faces, C)
    d_keep = torch.from_numpy(keep.astype(np.uint8)).to(DEV)
    got = ops.mesh_keep_components(d_rows, d_faces, C, comps, d_keep, world=world, guard_rows=GUARD_ROWS)
    host = {k: got[k].cpu().numpy() for k in ("rows", "faces", "positions", "vertex_map")}
    rb = S.row_bytes(C)
    print(f"{name}{' (world)' if use_world else ''}: {int(keep.sum())} of {len(keep)} components kept, {len(rows)} -> {len(host['rows'])} vertices, "
          f"{len(faces)} -> {len(host['faces'])} faces")
    tail = got["rows_buffer"].cpu().numpy()[len(host["rows"]) * rb:]
    assert len(tail) == GUARD_ROWS * rb and (tail == 0xA5).all()
    tail = got["faces_buffer"].cpu().numpy()[len(host["faces"]) * 3:]
    assert len(tail) == 3 * GUARD_ROWS and (tail.view(np.uint32) == 0xA5A5A5A5).all()
    assert got["n_classes"] == C and torch.equal(d_rows.cpu(), torch.from_numpy(np.ascontiguousarray(rows)))  # the input is not written
    assert torch.equal(d_faces.cpu(), torch.from_numpy(np.ascontiguousarray(faces)))
    assert host["faces"].dtype == np.int32 and host["faces"].shape == want["faces"].shape and np.array_equal(host["faces"], want["faces"])
    assert host["vertex_map"].dtype == np.int32 and np.array_equal(host["vertex_map"], want["vertex_map"])
    assert host["rows"].shape == want["rows"].shape and np.array_equal(host["rows"][:, 12:], want["rows"][:, 12:])
    assert np.array_equal(_bits(host["positions"]), _bits(want["positions"]))  # model frame, bit for bit (a NaN included: a copy)
    written, fin = S.positions_of(host["rows"]), np.isfinite(host["positions"]).all(1)
    expect = host["positions"] if world is None else S.apply_world(world, host["positions"])
    assert np.array_equal(_bits(written[fin]), _bits(expect[fin]))  # the rows hold the (world-frame) float32 of the returned positions
    assert np.isnan(written[~fin]).any(1).all()  # (the payload of a NaN that went through the affine is not a rule)
    if world is None:
        assert np.array_equal(host["rows"], want["rows"])
    else:
        assert np.array_equal(host["rows"][fin], want["rows"][fin])
    assert len(host["faces"]) == 0 or (host["faces"].min() >= 0 and np.array_equal(np.unique(host["faces"]), np.arange(len(host["rows"]))))
    again = ops.mesh_keep_components(d_rows, d_faces, C, comps, d_keep.bool(), world=world)  # a bool mask is the same mask
    for k in host:
        assert np.array_equal(again[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8)), k  # two runs, the same bytes
    if keep.all() and not use_world and name in ("sphere", "strip_chunk_plus_1"):  # no unused vertex: the input comes back
        assert np.array_equal(host["rows"], rows) and np.array_equal(host["faces"], faces) and np.array_equal(host["vertex_map"], np.arange(len(rows)))


def test_the_emit_with_world_writes_what_the_extraction_writes():
    """The xyz of a kept vertex under ``world`` are the bytes ``mesh_extract(vol, world)`` writes for it."""
    from umhsnerf import ops

    lo, h, dims = M.cube_lattice(24)
    D, W, Wc, A = M.field("random", lo, h, dims, C=3)
    n = dims[0] * dims[1] * dims[2]
    vol = ops.tsdf_volume(lo, h, dims, 3, DEV)
    for key, a in (("D", D), ("W", W), ("Wc", Wc), ("A", A)):
        vol[key].copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(vol[key].shape))
    assert vol["D"].numel() == n
    model, world = ops.mesh_extract(vol), ops.mesh_extract(vol, M.WORLD)
    comps = ops.mesh_components(model["rows"], model["faces"], 3)
    keep = (comps["faces"] >= 8).to(torch.uint8)
    got = ops.mesh_keep_components(model["rows"], model["faces"], 3, comps, keep, world=M.WORLD)
    sel = got["vertex_map"] >= 0
    assert 0 < int(sel.sum()) < len(sel) and torch.equal(got["rows"], world["rows"][sel])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from test_hip_distortion import make_scene
    from test_hip_render import _datamanager
    from test_hip_texture import N_STEPS
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("components")
    meta = make_scene(root / "scene", B=8)
    torch.manual_seed(0)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2,
                                            datamanager=_datamanager(root / "scene", 9))
    for step in range(N_STEPS):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    return dict(root=root, pipe=pipe)


NEW_KEYS = {"components", "components_kept", "cleaned_from", "component_table"}


def test_tsdf_keeps_the_largest_component_and_composes_with_the_other_stages(scene):
    from test_hip_texture import FLAGS, KW, N_STEPS, RES
    from umhsnerf import export

    root, pipe = scene["root"], scene["pipe"]
    plain = export.export_tsdf_mesh(pipe, root / "plain", **KW)
    none = export.export_tsdf_mesh(pipe, root / "none", min_component_faces=None, min_component_fraction=None, keep_largest_components=None, **KW)
    assert set(plain) == {"vertices", "faces", "cameras", "resolution", "voxel_size", "truncation", "file"} == set(none)
    assert (root / "none" / "mesh.ply").read_bytes() == (root / "plain" / "mesh.ply").read_bytes()  # no criterion: nothing new runs
    _, rows, faces = M.read_mesh_ply(plain["file"])
    ref = R.components(rows, faces, 3)
    res = export.export_tsdf_mesh(pipe, root / "one", min_component_fraction=1.0, **KW)
    _, got_rows, got_faces = M.read_mesh_ply(res["file"])
    after = R.components(got_rows, got_faces, 3)
    print(f"tiny scene: {len(faces)} faces in {int((ref['faces'] > 0).sum())} components with faces ({ref['n_components']} with the unused "
          f"vertices) -> {len(got_faces)} faces; table {res['component_table']}")
    assert after["n_components"] == 1 and after["faces"].tolist() == [len(got_faces)]  # exactly one component, no unused vertex
    keep = R.keep_mask(ref["faces"], min_component_fraction=1.0)
    want = R.emit(rows, faces, 3, ref, keep)
    assert np.array_equal(got_rows, want["rows"]) and np.array_equal(got_faces, want["faces"])
    assert set(res) == set(plain) | NEW_KEYS and res["faces"] == len(got_faces) and res["vertices"] == len(got_rows)
    assert res["components"] == int((ref["faces"] > 0).sum()) and res["components_kept"] == int(keep.sum()) == 1
    assert res["cleaned_from"] == plain["faces"] and len(res["component_table"]) == 1
    row, c = res["component_table"][0], int(np.argmax(keep))
    area64, bound = R.area_oracle(rows, faces, 3, ref["face_component"], ref["n_components"])
    assert (row["faces"], row["vertices"]) == (int(ref["faces"][c]), int(ref["vertices"][c])) and abs(row["area"] - area64[c]) <= bound[c]
    # with --material and --simplify-faces: the stages in their order, composed by hand from the operators
    from umhsnerf import ops

    label = np.ascontiguousarray(rows[:, 15:19]).view("<i4").reshape(-1)
    K = int(np.argmax([(label[faces] == k).all(1).sum() for k in range(3)]))
    sub = export.export_tsdf_mesh(pipe, root / "sub", material=K, **KW)
    _, s_rows, s_faces = M.read_mesh_ply(sub["file"])
    sref = R.components(s_rows, s_faces, 3)
    skeep = R.keep_mask(sref["faces"], min_component_faces=2, keep_largest_components=2)
    out = pipe.datamanager.train_dataparser_outputs
    A = export.world_frame_affine(out.dataparser_transform, out.dataparser_scale)
    cleaned, cleaned_wf = R.emit(s_rows, s_faces, 3, sref, skeep), R.emit(s_rows, s_faces, 3, sref, skeep, A)
    N = max(len(cleaned["faces"]) // 4, 1)
    both = export.export_tsdf_mesh(pipe, root / "both", material=K, keep_largest_components=2, min_component_faces=2, simplify_faces=N,
                                   save_world_frame=True, **KW)
    _, b_rows, b_faces = M.read_mesh_ply(both["file"])
    lo, h, dims = export.tsdf_lattice((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), RES)
    mesh, info = export.simplify_mesh(*_device(cleaned["rows"], cleaned["faces"]), 3, lo, h, dims, A, target_faces=N)
    print(f"material {K}: {sub['faces']} faces in {int((sref['faces'] > 0).sum())} components -> {len(cleaned['faces'])} cleaned -> {both['faces']} "
          f"(target {N})")
    assert set(both) == set(plain) | NEW_KEYS | {"simplified_from", "cell_voxels", "probes"}
    assert both["cleaned_from"] == sub["faces"] and both["simplified_from"] == len(cleaned["faces"]) and both["components_kept"] == int(skeep.sum())
    assert both["faces"] <= N and {k: both[k] for k in info} == info
    if mesh is None:  # (a cleaned mesh of a single face: left untouched, the cleaned rows in the world frame)
        assert np.array_equal(b_rows, cleaned_wf["rows"]) and np.array_equal(b_faces, cleaned_wf["faces"])
    else:
        assert np.array_equal(b_rows, mesh["rows"].cpu().numpy()) and np.array_equal(b_faces, mesh["faces"].cpu().numpy())
    # the command line, from a checkpoint: the same summary and the same bytes
    torch.save({"step": N_STEPS, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    cli = export.main(["tsdf", "--data", str(root / "scene"), "--checkpoint", str(root / "step-000000003.ckpt"), "--output-dir", str(root / "cli"),
                       "--resolution", str(RES), "--downscale-factor", "1", "--batch-size", "4", "--min-component-fraction", "1.0", *FLAGS])
    assert cli == {**res, "file": str(root / "cli" / "mesh.ply")}
    assert (root / "cli" / "mesh.ply").read_bytes() == (root / "one" / "mesh.ply").read_bytes()
    # the world frame moves the written positions only
    wf = export.export_tsdf_mesh(pipe, root / "one_wf", min_component_fraction=1.0, save_world_frame=True, **KW)
    _, wf_rows, wf_faces = M.read_mesh_ply(wf["file"])
    assert np.array_equal(wf_faces, got_faces) and np.array_equal(wf_rows[:, 12:], got_rows[:, 12:])
    assert np.array_equal(_bits(S.positions_of(wf_rows)), _bits(S.apply_world(A, S.positions_of(got_rows))))
    # a face target the cleaned mesh already meets, in the world frame: the cleaned rows, made again with the affine
    same = export.export_tsdf_mesh(pipe, root / "one_same", min_component_fraction=1.0, simplify_faces=res["faces"], save_world_frame=True, **KW)
    assert same["probes"] == 0 and same["cell_voxels"] is None and same["simplified_from"] == res["faces"]
    assert (root / "one_same" / "mesh.ply").read_bytes() == (root / "one_wf" / "mesh.ply").read_bytes()


def test_textured_mesh_of_the_cleaned_faces(scene):
    import texture_ref as T
    from test_hip_texture import KW, _png, _small_bands
    from umhsnerf import export

    root, pipe = scene["root"], scene["pipe"]
    with _small_bands():
        plain = export.export_textured_mesh(pipe, root / "tex_plain", px_per_uv_triangle=4, **KW)
        none = export.export_textured_mesh(pipe, root / "tex_none", px_per_uv_triangle=4, min_component_faces=None, min_component_fraction=None,
                                           keep_largest_components=None, **KW)
        res = export.export_textured_mesh(pipe, root / "tex_one", px_per_uv_triangle=4, min_component_fraction=1.0, **KW)
    assert {k: v for k, v in none.items() if k not in ("file", "textures")} == {k: v for k, v in plain.items() if k not in ("file", "textures")}
    for q in sorted((root / "tex_plain").iterdir()):
        assert (root / "tex_none" / q.name).read_bytes() == q.read_bytes(), q.name  # no criterion: the same files
    ply = export.export_tsdf_mesh(pipe, root / "tex_ply", min_component_fraction=1.0, **KW)
    table, _, faces = M.read_mesh_ply(ply["file"])
    F, Tside = res["faces"], res["atlas_side"]
    obj = T.read_textured_obj(res["file"])
    print(f"textured mesh: {plain['faces']} faces -> {F} in the largest component, atlas {plain['atlas_side']} -> {Tside}")
    assert set(res) == set(plain) | NEW_KEYS and res["cleaned_from"] == plain["faces"] and res["components_kept"] == 1
    assert F == ply["faces"] == len(obj["f"]) and len(obj["vt"]) == 3 * F and len(obj["v"]) == res["vertices"] == ply["vertices"]
    assert np.array_equal(obj["f"], faces) and np.array_equal(_bits(obj["v"]), _bits(np.stack([table["x"], table["y"], table["z"]], 1)))
    assert Tside == T.atlas(F, 4)[1] and np.array_equal(_bits(obj["vt"]), _bits(T.uv(F, 4).reshape(-1, 2)))  # an atlas for the cleaned face count
    img = _png(res["textures"]["rgb"])
    owner = T.owner_map(F, 4)
    assert img.shape == (Tside, Tside, 3) and (img[owner < 0] == 0).all() and (img[owner >= 0] != 0).any()
