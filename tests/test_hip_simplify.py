"""Mesh simplification on the GPU: ``ops.mesh_simplify`` / ``ops.mesh_simplify_count`` (csrc/umhs_simplify.hip) against the numpy
restatement of tests/simplify_ref.py -- faces, the vertex map, colour bytes and labels with ``==``, positions and abundances within the
bounds derived there, the guard rows untouched, two runs the same bytes -- the ``--simplify-faces`` search against the restatement's
search, and both mesh exports end to end on the tiny scene of tests/test_hip_mesh.py."""
import numpy as np
import pytest
import torch

import mesh_ref as M
import simplify_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_ROWS = 3
_cache = {}


def _volume_mesh(name, C):
    if (name, C) not in _cache:
        _cache[name, C] = S.volume_mesh(name, 24, C)
    return _cache[name, C]


def _want(key, rows, faces, C, origin, edge):
    if key not in _cache:
        _cache[key] = S.simplify(rows, faces, C, origin, edge)
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(rows, faces, C, origin, edge, world=None):
    from umhsnerf import ops

    d_rows, d_faces = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), torch.from_numpy(np.ascontiguousarray(faces)).to(DEV)
    got = ops.mesh_simplify(d_rows, d_faces, C, [float(v) for v in origin], float(edge), world=world, guard_rows=GUARD_ROWS)
    host = {k: got[k].cpu().numpy() for k in ("rows", "faces", "positions", "cluster")}
    rb = S.row_bytes(C)
    tail = got["rows_buffer"].cpu().numpy()[len(host["rows"]) * rb:]
    assert len(tail) == GUARD_ROWS * rb and (tail == 0xA5).all()
    tail = got["faces_buffer"].cpu().numpy()[len(host["faces"]) * 3:]
    assert len(tail) == 3 * GUARD_ROWS and (tail.view(np.uint32) == 0xA5A5A5A5).all()
    assert got["n_classes"] == C and torch.equal(d_rows.cpu(), torch.from_numpy(np.ascontiguousarray(rows)))  # the input is not written
    again = ops.mesh_simplify(d_rows, d_faces, C, [float(v) for v in origin], float(edge), world=world)
    for k in host:
        assert np.array_equal(again[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8)), k  # two runs, the same bytes
    return host


def _compare(got, want, C, world=None, what=""):
    assert got["faces"].shape == want["faces"].shape and got["rows"].shape == want["rows"].shape, (what, got["rows"].shape, want["rows"].shape)
    assert got["faces"].dtype == np.int32 and np.array_equal(got["faces"], want["faces"]), what
    assert np.array_equal(got["cluster"], want["cluster"]), what
    assert np.array_equal(got["rows"][:, 12:19 if C else 15], want["rows"][:, 12:19 if C else 15]), what  # colour bytes, label
    err = np.abs(got["positions"].astype(np.float64) - want["pos64"])
    ratio = float((err / want["pos_bound"]).max()) if err.size else 0.0
    same = bool(np.array_equal(_bits(got["positions"]), _bits(want["positions"])))
    print(f"{what}: {len(got['rows'])} vertices, {len(got['faces'])} faces, worst position error / bound {ratio:.3g} (float64 term "
          f"{want['f64_term']:.3g}), positions bit-equal to the restatement: {same}, L_max {want['L_max']}, M_max {want['M_max']}")
    assert (err <= want["pos_bound"]).all(), what
    written = S.positions_of(got["rows"])
    expect = got["positions"] if world is None else S.apply_world(world, got["positions"])
    assert np.array_equal(_bits(written), _bits(expect)), what  # the rows hold the (world-frame) float32 of the returned positions
    assert S.abund_within(got["rows"], want, C), what


# ---- the kernels against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_world", [False, True])
@pytest.mark.parametrize("C", [0, 6])
@pytest.mark.parametrize("ratio", [2.0 ** -12, 1.0, 2.0, 64.0])
def test_the_sphere_equals_the_restatement(ratio, C, use_world):
    """15-byte and 43-byte rows: no row but the first is 4-byte aligned."""
    rows, faces, lo, h = _volume_mesh("sphere", C)
    edge = np.float32(ratio) * h
    want = _want(("sphere", C, ratio), rows, faces, C, lo, edge)
    world = M.WORLD if use_world else None
    got = _run(rows, faces, C, lo, edge, world)
    _compare(got, want, C, world, f"sphere e = {ratio} h, C = {C}")
    if ratio == 64.0:
        assert got["rows"].shape == (0, S.row_bytes(C)) and got["faces"].shape == (0, 3) and (got["cluster"] == -1).all()
    if ratio == 2.0 ** -12 and not use_world:  # identity: every vertex bit for bit, faces up to the renumbering by key
        c = got["cluster"]
        assert np.array_equal(got["rows"][c], rows) and np.array_equal(got["faces"], c[faces]) and len(np.unique(c)) == len(rows)
    if ratio == 1.0:
        assert len(got["faces"]) == 1674 and len(got["rows"]) == 839


@pytest.mark.parametrize("name,ratio", [("slab", 8.0), ("two_spheres", 1.0), ("two_spheres", 3.0)])
def test_long_segments_and_a_non_manifold_mesh(name, ratio):
    """The slab at e = 8 h: clusters of several hundred members and more than a thousand corner records.  two_spheres touch at the
    origin."""
    rows, faces, lo, h = _volume_mesh(name, 3)
    edge = np.float32(ratio) * h
    want = _want((name, 3, ratio), rows, faces, 3, lo, edge)
    if name == "slab":
        assert want["M_max"] >= 200 and want["L_max"] > 1000
    _compare(_run(rows, faces, 3, lo, edge), want, 3, None, f"{name} e = {ratio} h")
    assert len(want["faces"]) > 0


@pytest.mark.parametrize("C", [0, 3])
def test_the_hand_made_mesh(C):
    rows, faces, g, e = S.hand_mesh(C)
    want = _want(("hand", C), rows, faces, C, g, e)
    assert want["tr0"] == 3 and len(want["faces"]) == 13
    got = _run(rows, faces, C, g, e, M.WORLD)
    _compare(got, want, C, M.WORLD, f"hand-made mesh C = {C}")
    assert got["cluster"][11] == -1 and got["cluster"][12] == -1


def test_empty_inputs_and_refused_grids():
    from umhsnerf import ops

    rows, faces, g, e = S.hand_mesh(3)
    d_rows, d_faces = torch.from_numpy(rows).to(DEV), torch.from_numpy(faces).to(DEV)
    for r, f in ((d_rows[:0], d_faces), (d_rows, d_faces[:0]), (d_rows[:0], d_faces[:0])):
        got = ops.mesh_simplify(r, f, 3, [0, 0, 0], 1.0, guard_rows=GUARD_ROWS)
        assert got["rows"].shape == (0, 31) and got["faces"].shape == (0, 3) and got["positions"].shape == (0, 3)
        assert got["cluster"].shape == (r.shape[0],) and (got["cluster"] == -1).all() and (got["rows_buffer"] == 0xA5).all()
        assert ops.mesh_simplify_count(r, f, 3, [0, 0, 0], 1.0) == 0
    for bad_edge in (2.0 ** -22, 1e-12):  # 2^62 cells or more; an axis of 2^31 or more
        with pytest.raises(ValueError):
            ops.mesh_simplify(d_rows, d_faces, 3, [0, 0, 0], bad_edge)
        with pytest.raises(ValueError):
            ops.mesh_simplify_count(d_rows, d_faces, 3, [0, 0, 0], bad_edge)
    for bad in (lambda: ops.mesh_simplify(d_rows, d_faces, 3, [0, 0, 0], 0.0), lambda: ops.mesh_simplify(d_rows, d_faces, 3, [0, np.nan, 0], 1.0),
                lambda: ops.mesh_simplify(d_rows, d_faces, 0, [0, 0, 0], 1.0), lambda: ops.mesh_simplify(d_rows, d_faces.long(), 3, [0, 0, 0], 1.0),
                lambda: ops.mesh_simplify(d_rows, d_faces, 3, [0, 0, 0], 1.0, world=np.eye(4))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.mesh_simplify(torch.from_numpy(rows), d_faces, 3, [0, 0, 0], 1.0)


# ---- the search ----------------------------------------------------------------------------------------------------------------------
def test_the_search_equals_the_restatements_search():
    from umhsnerf import export, ops

    rows, faces, lo, h = _volume_mesh("sphere", 3)
    lo_t, h_f, dims = tuple(float(v) for v in lo), float(h), (24, 24, 24)
    d_rows, d_faces = torch.from_numpy(rows).to(DEV), torch.from_numpy(faces).to(DEV)
    rungs = export.simplify_ladder(lo_t, h_f, dims)
    F = len(faces)
    ref_count = lambda k: S.count(rows, faces, 3, S.rung_origin(lo, rungs[k - 1]), rungs[k - 1])
    for k in (1, 4, len(rungs)):
        assert ops.mesh_simplify_count(d_rows, d_faces, 3, export.simplify_origin(lo_t, rungs[k - 1]), rungs[k - 1]) == ref_count(k)
    for N in (F, F - 1, 500, 1):
        mesh, info = export.simplify_mesh(d_rows, d_faces, 3, lo_t, h_f, dims, target_faces=N)
        if N >= F:  # left untouched: not even deduplicated
            assert mesh is None and info == {"simplified_from": F, "cell_voxels": None, "probes": 0}
            continue
        k, probes, seen = export.simplify_search(ref_count, len(rungs), N)
        assert info == {"simplified_from": F, "cell_voxels": rungs[k - 1] / h_f, "probes": probes}
        want = S.simplify(rows, faces, 3, S.rung_origin(lo, rungs[k - 1]), rungs[k - 1])
        got = {q: mesh[q].cpu().numpy() for q in ("rows", "faces", "positions", "cluster")}
        _compare(got, want, 3, None, f"search N = {N}: rung {k}, {probes} probes")
        assert len(got["faces"]) <= N and (k == 1 or ref_count(k - 1) > N)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from test_hip_distortion import make_scene
    from test_hip_render import _datamanager
    from test_hip_texture import N_STEPS
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("simplify")
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


def test_tsdf_with_cell_voxels_writes_the_simplified_unsimplified_export(scene):
    from test_hip_texture import KW, RES, _parent_mesh_ply
    from umhsnerf import export, ops

    root, pipe = scene["root"], scene["pipe"]
    plain = export.export_tsdf_mesh(pipe, root / "plain", **KW)
    assert set(plain) == {"vertices", "faces", "cameras", "resolution", "voxel_size", "truncation", "file"}
    assert (root / "plain" / "mesh.ply").read_bytes() == _parent_mesh_ply(pipe)  # without the flags: the bytes of the code before them
    _, rows, faces = M.read_mesh_ply(plain["file"])
    lo, h, dims = export.tsdf_lattice((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), RES)
    e = export.simplify_edge(h, 2)
    want = ops.mesh_simplify(torch.from_numpy(rows.copy()).to(DEV), torch.from_numpy(faces.copy()).to(DEV), 3, export.simplify_origin(lo, e), e)
    res = export.export_tsdf_mesh(pipe, root / "cell2", simplify_cell_voxels=2, **KW)
    _, got_rows, got_faces = M.read_mesh_ply(res["file"])
    assert np.array_equal(got_rows, want["rows"].cpu().numpy()) and np.array_equal(got_faces, want["faces"].cpu().numpy())
    assert 0 < res["faces"] == len(got_faces) < plain["faces"] and res["vertices"] == len(got_rows)
    assert res["simplified_from"] == plain["faces"] and res["cell_voxels"] == 2.0 and res["probes"] == 0
    ref = S.simplify(rows, faces, 3, export.simplify_origin(lo, e), e)
    assert np.array_equal(got_faces, ref["faces"]) and np.array_equal(got_rows[:, 12:19], ref["rows"][:, 12:19])
    # the command line, from a checkpoint: the same summary and the same bytes
    from test_hip_texture import FLAGS, N_STEPS

    torch.save({"step": N_STEPS, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    cli = export.main(["tsdf", "--data", str(root / "scene"), "--checkpoint", str(root / "step-000000003.ckpt"), "--output-dir", str(root / "cli"),
                       "--resolution", str(RES), "--downscale-factor", "1", "--batch-size", "4", "--simplify-cell-voxels", "2", *FLAGS])
    assert cli == {**res, "file": str(root / "cli" / "mesh.ply")}
    assert (root / "cli" / "mesh.ply").read_bytes() == (root / "cell2" / "mesh.ply").read_bytes()
    # the world frame moves the written positions only
    wf = export.export_tsdf_mesh(pipe, root / "cell2_wf", simplify_cell_voxels=2, save_world_frame=True, **KW)
    _, wf_rows, wf_faces = M.read_mesh_ply(wf["file"])
    out = pipe.datamanager.train_dataparser_outputs
    A = export.world_frame_affine(out.dataparser_transform, out.dataparser_scale)
    assert np.array_equal(wf_faces, got_faces) and np.array_equal(wf_rows[:, 12:], got_rows[:, 12:])
    assert np.array_equal(_bits(S.positions_of(wf_rows)), _bits(S.apply_world(A, S.positions_of(got_rows))))


def test_textured_mesh_with_a_face_target(scene):
    import texture_ref as R
    from test_hip_texture import KW, _png, _small_bands
    from umhsnerf import export

    root, pipe = scene["root"], scene["pipe"]
    with _small_bands():
        plain = export.export_textured_mesh(pipe, root / "tex_plain", px_per_uv_triangle=4, **KW)
        same = export.export_textured_mesh(pipe, root / "tex_same", px_per_uv_triangle=4, simplify_faces=plain["faces"], **KW)
        N = max(plain["faces"] // 4, 1)
        res = export.export_textured_mesh(pipe, root / "tex_n", px_per_uv_triangle=4, simplify_faces=N, **KW)
    # a target the mesh already meets: every file untouched, and the summary says so
    assert {k: v for k, v in same.items() if k in plain and k not in ("file", "textures")} == {k: v for k, v in plain.items() if k not in ("file", "textures")}
    assert same["simplified_from"] == plain["faces"] and same["cell_voxels"] is None and same["probes"] == 0
    for q in sorted((root / "tex_plain").iterdir()):
        assert (root / "tex_same" / q.name).read_bytes() == q.read_bytes(), q.name
    # without the flags the OBJ is the one composed by hand from the unflagged mesh
    table, _, faces = M.read_mesh_ply(export.export_tsdf_mesh(pipe, root / "tex_ply", **KW)["file"])
    obj = R.read_textured_obj(plain["file"])
    assert np.array_equal(obj["f"], faces) and np.array_equal(_bits(obj["v"]), _bits(np.stack([table["x"], table["y"], table["z"]], 1)))
    # the target
    F, T = res["faces"], res["atlas_side"]
    print(f"textured mesh: {plain['faces']} faces -> {F} (target {N}), atlas {plain['atlas_side']} -> {T}, cell {res['cell_voxels']:.3f} voxels, "
          f"{res['probes']} probes")
    obj = R.read_textured_obj(res["file"])
    assert 0 < F <= N and len(obj["f"]) == F and len(obj["vt"]) == 3 * F and len(obj["v"]) == res["vertices"]
    assert res["simplified_from"] == plain["faces"] and res["probes"] >= 1 and res["cell_voxels"] > 1.0
    assert T == R.atlas(F, 4)[1] and T < plain["atlas_side"]
    assert obj["f"].min() >= 0 and obj["f"].max() < res["vertices"] and np.array_equal(_bits(obj["vt"]), _bits(R.uv(F, 4).reshape(-1, 2)))
    img = _png(res["textures"]["rgb"])
    owner = R.owner_map(F, 4)
    assert img.shape == (T, T, 3) and (img[owner < 0] == 0).all() and (img[owner >= 0] != 0).any()  # no texel of a face that is gone
