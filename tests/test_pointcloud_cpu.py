"""Point-cloud export without a GPU: the restatement's own properties (tests/pointcloud_ref.py), the PLY writer against the test's
reader, the argument checks of the new exports (nothing is launched), the command line, and the float32 bound the GPU neighbour test
uses -- checked here by emulating the kernel's arithmetic in numpy over the very point sets the GPU test runs."""
import ctypes

import numpy as np
import pytest
import torch

import pointcloud_ref as P

F = np.float32


def test_accumulation_at_the_threshold_is_dropped_and_one_step_above_is_kept():
    p = np.zeros((3, 3), dtype=F)
    acc = np.array([0.5, np.nextafter(F(0.5), F(1)), np.nan], dtype=F)
    assert P.keep_rule(p, acc, 0.5).tolist() == [False, True, False]
    assert P.keep_rule(np.array([[np.inf, 0, 0], [0, np.nan, 0], [0, 0, -np.inf], [P.FMAX, 0, 0]], dtype=F), np.ones(4, dtype=F)).tolist() == [
        False, False, False, True]


def test_a_point_on_a_box_face_is_dropped():
    T, R, S = P.AXIS_BOX
    for axis in range(3):
        for sign in (-1.0, 1.0):
            on = T.copy()
            on[axis] = T[axis] + F(sign) * S[axis] * F(0.5)  # exact: the box is made of binary fractions
            inside = on.copy()
            inside[axis] = np.nextafter(on[axis], T[axis])
            outside = on.copy()
            outside[axis] = np.nextafter(on[axis], F(sign * np.inf))
            got = P.keep_rule(np.stack([on, inside, outside, T]), np.ones(4, dtype=F), 0.5, P.AXIS_BOX)
            assert got.tolist() == [False, True, False, True], (axis, sign)


def test_a_rotated_box_agrees_with_float64_away_from_its_faces():
    T, R, S = P.rotated_box()
    rng = np.random.default_rng(5)
    p = rng.uniform(-2, 2, (20000, 3)).astype(F)
    q64 = (p.astype(np.float64) - T.astype(np.float64)) @ R.astype(np.float64)  # R^T (p - T), row by row
    margin = np.abs(np.abs(q64) - S.astype(np.float64) / 2).min(axis=1)
    inside64 = (np.abs(q64) < S.astype(np.float64) / 2).all(axis=1)
    clear = margin > 1e-5  # (float32 rounding of q is below 1e-6 for coordinates of this size)
    got = P.keep_rule(p, np.ones(len(p), dtype=F), 0.5, (T, R, S))
    assert clear.sum() > 19000 and 1000 < inside64.sum() < 19000
    assert np.array_equal(got[clear], inside64[clear])
    # the Euler angles of the command line give the same kind of box: Rz(yaw) Ry(pitch) Rx(roll)
    from umhsnerf.export import obb_from_params

    Tc, Rc, Sc = obb_from_params([1, 2, 3], [0.0, 0.0, np.pi / 2], [2, 4, 6])
    assert np.allclose(Rc, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-7) and Tc.tolist() == [1, 2, 3] and Sc.tolist() == [2, 4, 6]
    Tc, Rc, Sc = obb_from_params([0, 0, 0], [np.pi / 2, 0.0, 0.0], [1, 1, 1])
    assert np.allclose(Rc, [[1, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-7)
    assert np.allclose(obb_from_params([0, 0, 0], [0.3, -0.2, 0.5], [1, 1, 1])[1] @ obb_from_params([0, 0, 0], [0.3, -0.2, 0.5], [1, 1, 1])[1].T,
                       np.eye(3), atol=1e-6)


def test_bytes_and_labels_of_the_restatement():
    v = np.array([-1.0, 0.0, np.nan, 1 / 255, 0.5, 0.999999, 1.0, 7.0, np.inf, -np.inf], dtype=F)
    assert P.byte_of(v).tolist() == [0, 0, 0, 1, 127, 254, 255, 255, 255, 0]
    probs = np.array([[0.2, 0.5, 0.5], [np.nan, 0.1, 0.05], [np.nan, np.nan, np.nan], [0.3, 0.3, 0.3]], dtype=F)
    assert P.material_of(probs).tolist() == [1, 1, 0, 0]
    A = P.world_of(np.array([[1.0, 2.0, 3.0]], dtype=F), np.array([[1, 0, 0, 10], [0, 2, 0, 20], [0, 0, 3, 30]], dtype=F))
    assert A.tolist() == [[11.0, 24.0, 39.0]]


def test_world_frame_affine_undoes_the_dataparser_transform():
    from umhsnerf.export import world_frame_affine

    rng = np.random.default_rng(2)
    Rm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    t, scale = rng.normal(size=3), 0.37
    transform = np.concatenate([Rm, t.reshape(3, 1)], axis=1)
    world = rng.normal(size=(50, 3))
    model = (world @ Rm.T + t) * scale  # what the dataparser does to a position
    A = world_frame_affine(transform, scale).astype(np.float64)
    assert np.allclose(model @ A[:, :3].T + A[:, 3], world, atol=1e-5)


@pytest.mark.parametrize("C", [0, 4])
def test_writer_and_reader_round_trip(tmp_path, C):
    from umhsnerf.export import ply_header, write_ply

    x = P.emit_inputs(300, C, "all")
    rows, pts, kept = P.emit(x["o"], x["d"], x["depth"], x["acc"], x["rgb"], x["abund"], x["probs"])
    assert rows.shape == (300, P.row_bytes(C)) and rows.shape[1] == (16 if C == 0 else 36)
    write_ply(tmp_path / "a.ply", torch.from_numpy(rows), C)
    table, raw = P.read_ply(tmp_path / "a.ply")
    assert np.array_equal(raw, rows) and len(table) == 300
    names = ["x", "y", "z", "red", "green", "blue", "alpha"] + (["material"] + [f"abundance_{i}" for i in range(C)] if C else [])
    assert list(table.dtype.names) == names
    assert np.array_equal(np.stack([table["x"], table["y"], table["z"]], 1), pts)
    assert np.array_equal(np.stack([table["red"], table["green"], table["blue"]], 1), P.byte_of(x["rgb"]))
    assert np.array_equal(table["alpha"], P.byte_of(x["acc"].reshape(-1)))
    if C:
        assert np.array_equal(table["material"], P.material_of(x["probs"]))
        assert np.array_equal(np.stack([table[f"abundance_{i}"] for i in range(C)], 1), x["abund"])
    blob = (tmp_path / "a.ply").read_bytes()
    assert blob.startswith(b"ply\nformat binary_little_endian 1.0\n") and blob[: len(ply_header(300, C))] == ply_header(300, C)
    write_ply(tmp_path / "empty.ply", torch.zeros((0, P.row_bytes(C)), dtype=torch.uint8), C)
    assert len(P.read_ply(tmp_path / "empty.ply")[0]) == 0


def test_new_exports_refuse_bad_arguments_before_anything_is_launched(built_library):
    from umhsnerf import _hip

    lib = _hip.lib()
    ARG, UNSUP = -1, -2
    d = ctypes.c_void_p(4096)  # never dereferenced

    def args(**kw):
        a = _hip.PcArgs()
        for k in ("origins", "directions", "depth", "accumulation", "rgb", "abundances", "seg_probs"):
            setattr(a, k, 4096)
        a.origins_stride = a.directions_stride = a.rgb_stride = 3
        a.depth_stride = a.accumulation_stride = 1
        a.abundances_stride = a.seg_probs_stride = a.n_classes = 6
        a.threshold = 0.5
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert lib.umhs_pc_chunks(0) == 0 and lib.umhs_pc_chunks(1) == 1 and lib.umhs_pc_chunks(256) == 1 and lib.umhs_pc_chunks(257) == 2
    assert lib.umhs_pc_flag_count(None, 8, d, None) == ARG
    assert lib.umhs_pc_flag_count(args(), 8, None, None) == ARG
    assert lib.umhs_pc_flag_count(args(), -1, d, None) == ARG
    assert lib.umhs_pc_flag_count(args(), 0, d, None) == 0  # nothing to do
    for missing in ("origins", "directions", "depth", "accumulation", "rgb", "abundances", "seg_probs"):
        assert lib.umhs_pc_flag_count(args(**{missing: None}), 8, d, None) == ARG, missing
        assert lib.umhs_pc_emit(args(**{missing: None}), 8, d, d, 0, d, d, d, 8, None) == ARG, missing
    assert lib.umhs_pc_flag_count(args(abundances=None, seg_probs=None, n_classes=0), 0, d, None) == 0  # the 16-byte row needs neither
    assert lib.umhs_pc_flag_count(args(origins_stride=2), 8, d, None) == ARG
    assert lib.umhs_pc_flag_count(args(abundances_stride=5), 8, d, None) == ARG
    assert lib.umhs_pc_flag_count(args(n_classes=-1), 8, d, None) == ARG
    assert lib.umhs_pc_flag_count(args(n_classes=17, abundances_stride=17, seg_probs_stride=17), 8, d, None) == UNSUP
    assert lib.umhs_pc_emit(args(), 8, d, d, 0, d, d, d, -1, None) == ARG  # cap < 0
    assert lib.umhs_pc_emit(args(), 8, d, d, 0, ctypes.c_void_p(4098), d, d, 8, None) == ARG  # rows not 4-byte aligned
    for hole in range(5):
        ptrs = [d] * 5
        ptrs[hole] = None
        assert lib.umhs_pc_emit(args(), 8, ptrs[0], ptrs[1], 0, ptrs[2], ptrs[3], ptrs[4], 8, None) == ARG, hole
    assert lib.umhs_pc_emit(args(), 0, None, None, 0, None, None, None, 0, None) == 0
    lo, dims = (ctypes.c_float * 3)(0, 0, 0), lambda *v: (ctypes.c_int32 * 3)(*v)
    knn = lambda m=8, start=d, pts=d, out=d, lo=lo, edge=0.5, dims=dims(4, 4, 4), k=20: lib.umhs_knn_mean_dist(pts, m, start, lo, edge, dims, k, out, None)
    assert knn(k=1) == ARG and knn(k=0) == ARG and knn(k=33) == UNSUP and knn(m=-1) == ARG
    assert knn(pts=None) == ARG and knn(start=None) == ARG and knn(out=None) == ARG and knn(lo=None) == ARG and knn(dims=None) == ARG
    assert knn(edge=0.0) == ARG and knn(edge=float("nan")) == ARG and knn(edge=float("inf")) == ARG and knn(dims=dims(4, 0, 4)) == ARG
    assert knn(dims=dims(128, 128, 129)) == UNSUP and knn(dims=dims(4097, 1, 1)) == UNSUP  # over 2^21 cells; over 4,096 along an axis
    assert knn(m=0, pts=None, start=None, out=None) == 0
    keys = lambda m=8, pts=d, out=d, edge=0.5, dims=dims(4, 4, 4): lib.umhs_pc_cell_keys(pts, m, lo, edge, dims, out, None)
    assert keys(pts=None) == ARG and keys(out=None) == ARG and keys(m=-1) == ARG and keys(edge=-1.0) == ARG
    assert keys(dims=dims(128, 128, 129)) == UNSUP and keys(dims=dims(1, 1, 0)) == ARG and keys(m=0) == 0
    assert lib.umhs_abi_version() == 11  # new symbols only


def test_command_line_parsing():
    from umhsnerf import export

    base = ["pointcloud", "--data", "scene", "--checkpoint", "c.ckpt", "--output-dir", "out"]
    a = export.parse_args(base)
    assert (a.num_points, a.remove_outliers, a.std_ratio, a.nb_neighbors, a.depth_output_name, a.rgb_output_name) == (
        1000000, True, 10.0, 20, "depth", "rgb")
    assert (a.num_rays_per_batch, a.save_world_frame, a.opacity_threshold, a.seed, a.spectra, a.material) == (32768, False, 0.5, 0, False, None)
    assert a.obb_center is None and a.obb_rotation is None and a.obb_scale is None
    a = export.parse_args(base + ["--remove-outliers", "false", "--save-world-frame", "true", "--obb-center", "0", "0", "0", "--obb-rotation",
                                  "0", "0", "1.5", "--obb-scale", "1", "2", "3", "--spectra", "--material", "2", "--num-points", "5000"])
    assert not a.remove_outliers and a.save_world_frame and a.obb_scale == [1.0, 2.0, 3.0] and a.spectra and a.material == 2
    for partial in (["--obb-center", "0", "0", "0"], ["--obb-rotation", "0", "0", "0", "--obb-scale", "1", "1", "1"]):
        with pytest.raises(SystemExit):
            export.parse_args(base + partial)
    with pytest.raises(SystemExit):
        export.parse_args(base + ["--nb-neighbors", "40"])
    with pytest.raises(ValueError, match="all three or none"):
        export.export_pointcloud(None, "out", obb_center=[0, 0, 0])


def test_grid_choice_fits_the_limits():
    """ops.pc_grid's arithmetic on host tensors: any edge, however small, ends in a grid the kernels accept."""
    from umhsnerf import ops

    pts = torch.from_numpy(P.knn_points("cube", 4096).copy())
    for edge in (None, 1e-6, 1e6):
        lo, e, dims = ops.pc_grid(pts, edge)
        assert all(1 <= v <= ops.PC_MAX_DIM for v in dims) and dims[0] * dims[1] * dims[2] <= ops.PC_MAX_CELLS and e > 0
    assert ops.pc_grid(pts, 1e6)[2] == (1, 1, 1) and ops.pc_grid(pts, 1e-6)[2][0] > 64
    assert ops.pc_grid(torch.from_numpy(P.knn_points("plane", 333).copy()))[2][2] == 1
    assert ops.pc_grid(torch.from_numpy(P.knn_points("identical", 21).copy()))[2] == (1, 1, 1)


@pytest.mark.parametrize("name", P.KNN_SETS)
def test_float32_arithmetic_of_the_neighbour_kernel_stays_within_the_bound(name):
    """The arithmetic umhs_knn_mean_dist is specified to use, emulated in numpy float32, against float64 on the same float32 points:
    within (k + 8) * 2^-24 * mean64 (P.knn_bound states the derivation) on every point set, size and k the GPU test runs."""
    worst = 0.0
    for s, m, k in P.knn_cases():
        if s != name:
            continue
        want = P.knn_reference(s, m, k)
        got = P.knn_mean32(P.knn_points(s, m), k).astype(np.float64)
        err, bound = np.abs(got - want), P.knn_bound(want, k)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0)
        assert (err <= bound).all(), (s, m, k, float((err - bound).max()))
        if s == "identical" or (s == "copies" and k <= 64):
            assert (got[want == 0] == 0).all()
    print(f"{name}: largest error / bound = {worst:.3f}")
    assert worst <= 1.0
