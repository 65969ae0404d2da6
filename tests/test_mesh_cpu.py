"""Mesh export without a GPU: the numpy restatements of tests/mesh_ref.py must earn their keep before the kernels are held to them
(tests/test_hip_mesh.py), then the PLY writer and the command line."""
import itertools

import numpy as np
import pytest
import torch

import mesh_ref as M


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def _mesh(name, n):
    lo, h, dims = M.cube_lattice(n)
    D, W, Wc, A = M.field(name, lo, h, dims)
    return M.extract(D, W, Wc, A, lo, h, dims), (D, W, Wc, A, lo, h, dims)


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0), ("two_spheres", 2)])
def test_closed_level_sets_give_watertight_oriented_meshes(name, chi):
    """33^3 lattice.  Every undirected edge lies in exactly two triangles, once in each direction; V - E + F is 2 for the sphere, 0
    for the torus and -- as computed -- 2 for the two spheres that touch at the origin: the lattice is shifted off the origin, the
    touching point falls inside one cell and the two balls come out as ONE closed surface of genus 0 (joined by a neck a voxel
    wide), not as two components (which would give 4)."""
    r, _ = _mesh(name, 33)
    V = len(r["pos"])
    assert V > 1000 and len(r["faces"]) > 2000
    assert r["faces"].min() >= 0 and r["faces"].max() < V
    assert M.closed_and_oriented(r["faces"], V)
    assert M.euler(r["faces"], V) == chi
    vol, _ = M.volume_area(r["pos"], r["faces"])
    assert vol > 0  # the normals point to the non-negative side: outwards


def test_sphere_volume_and_area_converge():
    """Signed volume and area of the r = 0.6 sphere against 4/3 pi r^3 = 0.904779 and 4 pi r^2 = 4.523893.  Measured relative errors:
    17^3: volume -2.15e-2, area -1.12e-2;  33^3: volume -5.41e-3, area -2.79e-3  (both from below: the chords of a convex surface lie
    inside it; a factor 4 per halving of the voxel edge, i.e. second order)."""
    want_v, want_a = 4.0 / 3.0 * np.pi * 0.6 ** 3, 4.0 * np.pi * 0.6 ** 2
    errs = []
    for n in (17, 33):
        r, _ = _mesh("sphere", n)
        v, a = M.volume_area(r["pos"], r["faces"])
        errs.append(((v - want_v) / want_v, (a - want_a) / want_a))
        print(f"sphere {n}^3: volume {v:.6f} ({errs[-1][0]:+.3e}), area {a:.6f} ({errs[-1][1]:+.3e})")
    assert abs(errs[1][0]) < abs(errs[0][0]) and abs(errs[1][1]) < abs(errs[0][1])
    assert errs[0][0] < 0 and errs[1][0] < 0  # inscribed


def test_every_sign_case_occurs_in_every_tetrahedron():
    lo, h, dims = M.cube_lattice(9)
    D, W, Wc, A = M.field("random", lo, h, dims)
    W = np.ones_like(W)
    nx, ny, nz = dims
    xyz = M.lattice_xyz(dims)
    cell = np.nonzero((xyz[:, 0] + 1 < nx) & (xyz[:, 1] + 1 < ny) & (xyz[:, 2] + 1 < nz))[0]
    inside = D < 0
    for perm in M.PERMS:
        assert set(_tet_codes(inside, cell, dims, perm).tolist()) == set(range(16)), perm
    r = M.extract(D, W, Wc, A, lo, h, dims)
    # a random field has no boundary inside the lattice either: every interior edge is shared correctly (edges on the lattice's hull
    # are open), so check the counting instead: triangles per tetrahedron code
    n_tri = sum(int(np.isin(code, [1, 2, 4, 8, 7, 11, 13, 14]).sum() + 2 * np.isin(code, [3, 5, 6, 9, 10, 12]).sum())
                for code in [_tet_codes(inside, cell, dims, p) for p in M.PERMS])
    assert len(r["faces"]) == n_tri


def _tet_codes(inside, cell, dims, perm):
    nx, ny, _ = dims
    offs = [np.zeros(3, int)]
    for ax in perm[:2]:
        o = offs[-1].copy()
        o[ax] += 1
        offs.append(o)
    offs.append(np.ones(3, int))
    return sum(inside[cell + o[0] + o[1] * nx + o[2] * nx * ny].astype(int) << k for k, o in enumerate(offs))


def test_holes_emit_nothing_and_every_index_is_a_vertex():
    lo, h, dims = M.cube_lattice(9)
    D, W, Wc, A = M.field("random", lo, h, dims)
    assert (W == 0).sum() > 50
    r = M.extract(D, W, Wc, A, lo, h, dims)
    V = len(r["pos"])
    assert len(r["faces"]) > 0 and r["faces"].min() >= 0 and r["faces"].max() < V
    # no vertex on an edge with an unseen end; no triangle from a cell with an unseen corner: rebuild the owners of every face's
    # vertices and check that the 8 corners of some cell containing all three are valid -- via the count: with the holes filled
    # there are strictly more faces, and the faces of the cells that are whole either way are the same triples up to the renumbering
    full = M.extract(D, np.ones_like(W), Wc, A, lo, h, dims)
    assert len(full["faces"]) > len(r["faces"])
    nx, ny, nz = dims
    own, slot = np.nonzero((r["mask"][:, None] >> np.arange(7)) & 1)
    off = np.array(M.SLOT_OFFSETS)[slot]
    other = own + off[:, 0] + off[:, 1] * nx + off[:, 2] * nx * ny
    assert (W[own] > 0).all() and (W[other] > 0).all() and ((D[own] < 0) != (D[other] < 0)).all()
    # a face's three vertices lie in one cell whose corners are all valid
    xyz = M.lattice_xyz(dims)
    lo_c = np.minimum.reduce([xyz[own[r["faces"][:, k]]] for k in range(3)])
    hi_c = np.maximum.reduce([xyz[other[r["faces"][:, k]]] for k in range(3)])
    assert ((hi_c - lo_c) <= 1).all()
    for o in itertools.product((0, 1), repeat=3):
        c = hi_c - 1 + np.array(o)
        assert (W[c[:, 0] + c[:, 1] * nx + c[:, 2] * nx * ny] > 0).all()
    out = M.extract(*M.field("outside", lo, h, dims), lo, h, dims)
    assert len(out["pos"]) == 0 and out["faces"].shape == (0, 3)


def test_a_swapped_winding_is_rejected():
    _, (D, W, Wc, A, lo, h, dims) = _mesh("sphere", 17)
    bad = M.extract(D, W, Wc, A, lo, h, dims, swap_winding=True)
    assert M.closed_and_oriented(bad["faces"], len(bad["pos"]))  # consistently wrong ...
    assert M.volume_area(bad["pos"], bad["faces"])[0] < 0  # ... and inside out: the signed volume says so
    good = M.extract(D, W, Wc, A, lo, h, dims)
    assert not np.array_equal(good["faces"], bad["faces"])
    # one tetrahedron's rule alone flipped breaks the orientation of the shared edges
    mixed = good["faces"].copy()
    mixed[::6] = mixed[::6][:, [0, 2, 1]]
    assert not M.closed_and_oriented(mixed, len(good["pos"]))


def test_rows_carry_the_interpolated_attributes_and_labels():
    r, (D, W, Wc, A, lo, h, dims) = _mesh("sphere", 17)
    C = 3
    rows = r["rows"]
    assert rows.shape[1] == M.row_bytes(C) == 31
    pos = np.ascontiguousarray(rows[:, :12]).view(np.float32).reshape(-1, 3)
    assert np.array_equal(pos.view(np.uint32), r["pos"].view(np.uint32))
    assert np.abs(np.linalg.norm(pos.astype(np.float64), axis=1) - 0.6).max() < 0.01  # on the sphere, to second order in h
    label = np.ascontiguousarray(rows[:, 15:19]).view(np.int32).ravel()
    assert set(np.unique(label).tolist()) <= {-1, 0, 1, 2} and (label == -1).any() and (label >= 0).any()
    untinted = label == -1
    assert (rows[untinted, 12:15] == 0).all() and (np.ascontiguousarray(rows[untinted, 19:]).view(np.float32) == 0).all()
    moved = M.extract(D, W, Wc, A, lo, h, dims, world=M.WORLD)["rows"]
    assert np.array_equal(moved[:, 12:], rows[:, 12:]) and not np.array_equal(moved[:, :12], rows[:, :12])


# ---- fusion ------------------------------------------------------------------------------------------------------------------------
CASES = [((13, 10, 9), 0), ((13, 10, 9), 3), ((13, 10, 9), 16), ((1, 1, 1), 3)]


@pytest.fixture(scope="module")
def fused():
    out = {}
    for dims, C in CASES:
        case = M.fusion_case(dims, C)
        out[dims, C] = (case, M.fuse_case(case, np.float64), M.fuse_case(case, np.float32))
    return out


def test_fusion_bound_holds_for_the_float32_restatement_with_the_projects_margin(fused):
    """K_FUSE = max(8, 4 x the float32 restatement's worst ratio, rounded up to a power of two).  Measured worst |f32 - f64| /
    (u (mag + tiny)) over the cases: D 0.35, attributes 0.93 -> K_FUSE = 8."""
    worst = {"D": 0.0, "A": 0.0}
    for (dims, C), (case, r64, r32) in fused.items():
        ratios, left_out = M.fuse_ratios(r32, r64)
        print(dims, C, ratios, f"left out {left_out:.4f}")
        keep = ~r64["edge"]
        assert np.array_equal(r32["W"][keep], r64["W"][keep].astype(np.float32))
        assert np.array_equal(r32["Wc"][keep], r64["Wc"][keep].astype(np.float32))
        for k in worst:
            worst[k] = max(worst[k], ratios[k])
    print("worst ratios", worst)
    k = max(8.0, 2.0 ** np.ceil(np.log2(4.0 * max(worst.values()))))
    assert k == M.K_FUSE


def test_edges_leave_out_at_most_two_per_cent_and_the_case_has_every_situation(fused):
    for (dims, C), (case, r64, _) in fused.items():
        n = int(np.prod(dims))
        if n == 1:
            assert not r64["edge"].any() and r64["W"][0] == 2  # the single point is seen by both front cameras
            continue
        assert r64["edge"].mean() <= 0.02
        W, Wc = r64["W"], r64["Wc"]
        assert W.max() == 2  # the camera behind the volume sees nothing
        assert (W == 1).sum() > 0.2 * n  # the wall occludes part of the volume for the first camera
        assert (Wc == 0).sum() > 0 and (Wc == 1).sum() > 0 and (Wc == 2).sum() > 0
        assert (r64["D"] < 0).sum() > 0.05 * n and (r64["D"] > 0).sum() > 0.05 * n and (r64["D"] == 1.0).sum() > 0
        # each camera alone: the first (wall, NaN) and second (background) see a part, the third nothing
        seen = [M.fuse_case(case, np.float64, cameras=[c])["W"].sum() for c in range(3)]
        assert 0 < seen[0] < seen[1] <= n and seen[2] == 0


def test_split_calls_give_the_same_bits(fused):
    case, _, one = fused[(13, 10, 9), 3]
    for first in ([0], [0, 1]):
        rest = [c for c in range(3) if c not in first]
        two = M.fuse_case(case, np.float32, cameras=rest, state=M.fuse_case(case, np.float32, cameras=first))
        for k in ("D", "W", "Wc", "A"):
            assert np.array_equal(two[k].view(np.uint32), one[k].view(np.uint32)), (first, k)


@pytest.mark.parametrize("fault", ["camera_z", "pixel", "colour_w"])
def test_planted_faults_are_rejected(fused, fault):
    """Camera z instead of the Euclidean distance, the pixel to the right, and the colour mean weighted by W instead of Wc."""
    case, r64, _ = fused[(13, 10, 9), 3]
    bad = M.fuse_case(case, np.float32, fault=fault)
    ratios, _ = M.fuse_ratios(bad, r64)
    print(fault, ratios)
    keep = ~r64["edge"]
    counts_differ = not (np.array_equal(bad["W"][keep], r64["W"][keep].astype(np.float32))
                         and np.array_equal(bad["Wc"][keep], r64["Wc"][keep].astype(np.float32)))
    assert max(ratios.values()) > 100 * M.K_FUSE or counts_differ
    if fault == "colour_w":
        assert ratios["A"] > 100 * M.K_FUSE and ratios["D"] <= M.K_FUSE


def test_projection_inverts_ray_generation_for_a_distorted_camera():
    """origin + direction * depth of every pixel centre's ray projects back into that pixel (at its centre, to 1e-6 of a pixel)."""
    case = M.fusion_case()
    for cam in case["cams"][:2]:
        o, d = M.pixel_rays(cam, 16, 24)
        for depth in (0.7, 2.9):
            u, v, zc = M.project(cam, o + d * depth)
            yy, xx = np.meshgrid(np.arange(16), np.arange(24), indexing="ij")
            assert (zc > 0).all()
            assert np.array_equal(np.floor(u).astype(int), xx.ravel()) and np.array_equal(np.floor(v).astype(int), yy.ravel())
            assert np.abs(u - xx.ravel() - 0.5).max() < 1e-6 and np.abs(v - yy.ravel() - 0.5).max() < 1e-6
    assert case["cams"][1]["dist"] is not None and case["cams"][0]["dist"] is None


# ---- the file and the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [0, 3])
def test_ply_header_agrees_with_the_payload(tmp_path, C):
    from umhsnerf import export

    lo, h, dims = M.cube_lattice(9)
    D, W, Wc, A = M.field("sphere", lo, h, dims, C=C)
    r = M.extract(D, W, Wc, A, lo, h, dims)
    path = tmp_path / "mesh.ply"
    export.write_mesh_ply(path, torch.from_numpy(r["rows"]), torch.from_numpy(r["faces"]), C)
    table, rows, faces = M.read_mesh_ply(path)
    names = ["x", "y", "z", "red", "green", "blue"] + (["material"] + [f"abundance_{i}" for i in range(C)] if C else [])
    assert list(table.dtype.names) == names and table.dtype.itemsize == M.row_bytes(C)
    assert np.array_equal(rows, r["rows"]) and np.array_equal(faces, r["faces"])
    assert np.array_equal(np.stack([table["x"], table["y"], table["z"]], 1).view(np.uint32), r["pos"].view(np.uint32))
    header = path.read_bytes().split(b"end_header\n")[0].decode()
    assert f"element vertex {len(rows)}\n" in header and f"element face {len(faces)}\n" in header
    assert "property list uchar int vertex_indices" in header
    # an empty mesh is a valid file
    export.write_mesh_ply(path, torch.zeros(0, M.row_bytes(C), dtype=torch.uint8), torch.zeros(0, 3, dtype=torch.int32), C)
    table, rows, faces = M.read_mesh_ply(path)
    assert len(table) == 0 and faces.shape == (0, 3)


def test_material_filter_drops_unreferenced_vertices_and_reindexes():
    from umhsnerf import export

    r, _ = _mesh("sphere", 17)
    rows, faces = torch.from_numpy(r["rows"]), torch.from_numpy(r["faces"])
    label = np.ascontiguousarray(r["rows"][:, 15:19]).view(np.int32).ravel()
    total = 0
    for K in range(3):
        rk, fk = export.filter_mesh_material(rows, faces, K)
        lk = np.ascontiguousarray(rk.numpy()[:, 15:19]).view(np.int32).ravel()
        assert (lk == K).all() and fk.dtype == torch.int32
        want = r["faces"][(label[r["faces"]] == K).all(1)]
        assert len(fk) == len(want) > 0 and np.array_equal(np.unique(fk.numpy()), np.arange(len(rk)))
        assert np.array_equal(rk.numpy()[fk.numpy()], r["rows"][want])  # the same triangles, vertex for vertex
        total += len(fk)
    assert total < len(faces)  # faces across a material boundary belong to no sub-mesh


def test_lattice_from_the_box_and_the_resolution():
    from umhsnerf import export

    lo, h, dims = export.tsdf_lattice([-1, -1, -1], [1, 1, 1], 128)
    assert dims == (128, 128, 128) and lo == (-1.0, -1.0, -1.0) and h == float(np.float32(2.0 / 127))
    lo, h, dims = export.tsdf_lattice([-1, -1, -0.5], [1, 0, 0.5], 24)
    assert dims == (24, 12, 12) and h == float(np.float32(2.0 / 23))
    lo, h, dims = export.tsdf_lattice([0, 0, 0], [1, 2, 4], [5, 5, 5])
    assert dims == (5, 5, 5) and h == 1.0
    with pytest.raises(ValueError):
        export.tsdf_lattice([0, 0, 0], [1, 0, 1], 16)
    with pytest.raises(ValueError):
        export.tsdf_lattice([0, 0, 0], [1, 1, 1], 1)


def test_parser_defaults_refusals_and_the_unchanged_pointcloud_defaults(capsys):
    from umhsnerf import export

    base = ["--data", "scene", "--checkpoint", "step.ckpt", "--output-dir", "out"]
    a = export.parse_args(["tsdf", *base])
    assert a.command == "tsdf" and a.resolution == [128] and a.bounding_box_min == [-1.0, -1.0, -1.0] and a.bounding_box_max == [1.0, 1.0, 1.0]
    assert a.downscale_factor == 2 and a.batch_size == 8 and a.truncation_voxels == 5.0 and a.opacity_threshold == 0.5
    assert a.save_world_frame is False and a.material is None and a.depth_output_name == "depth" and a.rgb_output_name == "rgb"
    assert a.method == "rgb+spectral" and a.device == "cuda:0"  # eval.add_model_arguments
    a = export.parse_args(["tsdf", *base, "--resolution", "64", "32", "16", "--save-world-frame", "--material", "2"])
    assert a.resolution == [64, 32, 16] and a.save_world_frame is True and a.material == 2
    for bad, word in ((["--target-num-faces", "50000"], "decimator"), (["--texture-method", "nerf"], "unwrap"),
                      (["--unwrap-method", "xatlas"], "unwrap"), (["--resolution", "64", "32"], "one integer or three"),
                      (["--batch-size", "0"], "positive"), (["--bounding-box-min", "1", "0", "0"], "below")):
        with pytest.raises(SystemExit):
            export.parse_args(["tsdf", *base, *bad])
        assert word in capsys.readouterr().err
    p = vars(export.parse_args(["pointcloud", *base]))
    assert p == dict(command="pointcloud", data="scene", checkpoint="step.ckpt", output_dir="out", num_points=1000000, remove_outliers=True,
                     std_ratio=10.0, nb_neighbors=20, depth_output_name="depth", rgb_output_name="rgb", num_rays_per_batch=32768,
                     obb_center=None, obb_rotation=None, obb_scale=None, save_world_frame=False, opacity_threshold=0.5, seed=0, spectra=False,
                     material=None, **{k: p[k] for k in ("method", "num_classes", "pred_specular", "temperature", "background_color",
                                                          "log2_hashmap_size", "eval_mode", "seg_ignore_label", "images_on_gpu", "device")})
    with pytest.raises(SystemExit):
        export.parse_args(["pointcloud", *base, "--resolution", "64"])  # the mesh flags are not the point cloud's
    capsys.readouterr()


def test_argument_errors_of_the_mesh_entries_come_before_any_launch(built_library):
    import ctypes

    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, UNSUP = -1, -2
    d = 4096  # never dereferenced
    vol = _hip.TsdfVolume(d, d, d, d, (ctypes.c_int32 * 3)(4, 4, 4), 9, (ctypes.c_float * 3)(0, 0, 0), 0.1)
    img = _hip.TsdfImages()
    img.depth = img.accumulation = img.rgb = img.abundances = img.seg_probs = d
    img.n_cameras, img.height, img.width, img.n_classes, img.threshold, img.truncation = 1, 4, 4, 3, 0.5, 0.5
    call = lambda v=vol, i=img: lib.umhs_tsdf_integrate(ctypes.byref(v), ctypes.byref(i), None)
    assert lib.umhs_tsdf_integrate(None, ctypes.byref(img), None) == ARG and lib.umhs_tsdf_integrate(ctypes.byref(vol), None, None) == ARG
    for field_, value, code in (("n_cameras", 17, UNSUP), ("n_cameras", -1, ARG), ("n_classes", 2, ARG), ("truncation", 0.0, ARG),
                                ("height", 0, ARG), ("depth", None, ARG), ("seg_probs", None, ARG)):
        old = getattr(img, field_)
        setattr(img, field_, value)
        assert call() == code, field_
        setattr(img, field_, old)
    img.n_cameras = 0
    assert call() == 0  # nothing to fuse
    img.n_cameras = 1
    for field_, value, code in (("D", None, ARG), ("A", None, ARG), ("h", 0.0, ARG), ("n_attr", 4, ARG), ("n_attr", 3 + 2 * 17, UNSUP)):
        old = getattr(vol, field_)
        setattr(vol, field_, value)
        assert call() == code, field_
        assert lib.umhs_mesh_mark(ctypes.byref(vol), d, d, d, None) == code
        setattr(vol, field_, old)
    vol.dims[0] = 0
    assert call() == ARG
    vol.dims[:] = [1 << 10, 1 << 10, 1 << 10]
    assert call() == UNSUP and lib.umhs_mesh_mark(ctypes.byref(vol), d, d, d, None) == UNSUP  # more than 2^28 points
    vol.dims[:] = [4, 4, 4]
    assert lib.umhs_mesh_mark(ctypes.byref(vol), None, d, d, None) == ARG
    assert lib.umhs_mesh_vertices(ctypes.byref(vol), d, d, None, d, None, 5, None) == ARG  # rows missing with cap > 0
    assert lib.umhs_mesh_vertices(ctypes.byref(vol), d, d, None, d, d, -1, None) == ARG
    assert lib.umhs_mesh_vertices(ctypes.byref(vol), d, None, None, d, d, 5, None) == ARG
    assert lib.umhs_mesh_triangles(ctypes.byref(vol), d, d, d, None, 5, None) == ARG
    assert lib.umhs_mesh_triangles(ctypes.byref(vol), d, None, d, d, 5, None) == ARG
    assert lib.umhs_mesh_chunks(0) == 0 and lib.umhs_mesh_chunks(256) == 1 and lib.umhs_mesh_chunks(1170) == 5
    assert ctypes.sizeof(_hip.TsdfCamera) == 92 and ctypes.sizeof(_hip.TsdfVolume) == 64
    assert ctypes.sizeof(_hip.TsdfImages) == 40 + 120 + 24 + 16 * 92
