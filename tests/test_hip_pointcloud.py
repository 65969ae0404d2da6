"""Point-cloud export on the GPU.

Rows: ``umhs_pc_flag_count`` / ``umhs_pc_emit`` (``ops.pc_append``) must give the bytes of tests/pointcloud_ref.py -- ``==`` on every byte
of ``rows``, ``points`` and ``kept``, and every byte behind them untouched.  The launch grid is one workgroup per chunk of 256 rays and is
not capped, so there is no size "with more chunks than one grid step"; 1,031 rays are five chunks, the last one partial.

Neighbours: ``umhs_knn_mean_dist`` (``ops.knn_mean_dist``) against float64 on scipy's cKDTree within (k + 8) * 2^-24 * mean64 -- the
bound tests/test_pointcloud_cpu.py checks by emulation over the same point sets -- then mu, sigma and the keep mask of the outlier rule.

End to end: the tiny trained scene of tests/test_hip_render.py (``make_scene``, 3 classes, ``pred_specular``, three training steps)."""
import json

import numpy as np
import pytest
import torch

import pointcloud_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def _strided(a, pad_left, pad_right):
    """The array as columns [pad_left, pad_left + c) of a wider device tensor: a source read in place at its own stride."""
    t = torch.from_numpy(a)
    wide = torch.full((a.shape[0], pad_left + a.shape[1] + pad_right), 123.0, dtype=torch.float32)
    wide[:, pad_left:pad_left + a.shape[1]] = t
    return wide.to(DEV)[:, pad_left:pad_left + a.shape[1]]


def _run_emit(x, threshold=0.5, box=None, world=None, base=0, cap=None, ordinal0=0, strided=False):
    """-> (rows, points, kept) device buffers as numpy, the count the call returned, and the restatement's (rows, points, kept)."""
    from umhsnerf import ops

    n = x["o"].shape[0]
    C = 0 if x["abund"] is None else x["abund"].shape[1]
    want = P.emit(x["o"], x["d"], x["depth"], x["acc"], x["rgb"], x["abund"], x["probs"], threshold, box, world, ordinal0)
    cap = base + len(want[2]) if cap is None else cap
    rb = P.row_bytes(C)
    up = (lambda a, l, r: _strided(a, l, r)) if strided else (lambda a, l, r: torch.from_numpy(a).to(DEV))
    src = [up(x["o"], 1, 2), up(x["d"], 0, 3), up(x["depth"], 2, 0), up(x["acc"], 1, 1), up(x["rgb"], 3, 1)]
    src += [None, None] if C == 0 else [up(x["abund"], 2, 1), up(x["probs"], 0, 5)]
    extra = 3  # guard rows behind the buffers
    rows = torch.full(((cap + extra) * rb,), GUARD, dtype=torch.uint8, device=DEV)
    points = torch.full((cap + extra, 3), -7.0, device=DEV)
    kept = torch.full((cap + extra,), -7, dtype=torch.int64, device=DEV)
    base_t = torch.tensor([base], dtype=torch.int64, device=DEV)
    args = ops.pc_args(*src, threshold=threshold, box=box, world=world)
    total = ops.pc_append(args, rows, points, kept, base_t, ordinal0, cap)
    assert int(base_t) == base  # the caller adds
    return (rows.cpu().numpy().reshape(cap + extra, rb), points.cpu().numpy(), kept.cpu().numpy()), int(total), want, cap


def _check_emit(got, total, want, cap, base=0):
    rows, points, kept = got
    wrows, wpts, wkept = want
    assert total == len(wkept)
    w = max(0, min(len(wkept), cap - base))  # what fits below cap
    assert np.array_equal(rows[base:base + w], wrows[:w])
    assert np.array_equal(points[base:base + w].view(np.uint32), wpts[:w].view(np.uint32))  # bits: NaN-safe, -0 != +0
    assert np.array_equal(kept[base:base + w], wkept[:w])
    assert (rows[:base] == GUARD).all() and (rows[base + w:] == GUARD).all()
    assert (points[:base] == -7.0).all() and (points[base + w:] == -7.0).all()
    assert (kept[:base] == -7).all() and (kept[base + w:] == -7).all()
    return w


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1031])
def test_rows_equal_the_restatement_at_every_size(n):
    """Mixed accumulations and every special value, 6 classes, a rotated box with points on and next to its faces, the world affine,
    strided sources, a non-zero running base and a non-zero ordinal."""
    box = P.rotated_box()
    x = P.emit_inputs(n, 6, "mixed", box)
    got, total, want, cap = _run_emit(x, box=box, world=P.WORLD, base=37, ordinal0=5000, strided=True)
    w = _check_emit(got, total, want, cap, base=37)
    if n >= 256:
        assert 0 < w < n
    # and the plain form: no box, no affine, contiguous sources, base 0
    got, total, want, cap = _run_emit(P.emit_inputs(n, 6, "mixed"))
    _check_emit(got, total, want, cap)


@pytest.mark.parametrize("pattern", ["all", "none", "alternate"])
def test_all_kept_none_kept_and_alternating(pattern):
    x = P.emit_inputs(1031, 6, pattern)
    got, total, want, cap = _run_emit(x)
    _check_emit(got, total, want, cap)
    assert total == {"all": 1031, "none": 0, "alternate": 516}[pattern]


@pytest.mark.parametrize("C", [0, 1, 6, 15])
@pytest.mark.parametrize("boxname", ["none", "axis", "rotated"])
def test_row_layouts_and_boxes(C, boxname):
    box = {"none": None, "axis": P.AXIS_BOX, "rotated": P.rotated_box()}[boxname]
    x = P.emit_inputs(257, C, "mixed", box)
    for world in (None, P.WORLD):
        got, total, want, cap = _run_emit(x, box=box, world=world, strided=(C % 2 == 1))
        assert got[0].shape[1] == (16 if C == 0 else 20 + 4 * C)
        w = _check_emit(got, total, want, cap)
        assert w > 0
    if box is not None:
        assert len(want[2]) < len(P.emit(x["o"], x["d"], x["depth"], x["acc"], x["rgb"], x["abund"], x["probs"])[2])  # the box cuts
    if boxname == "axis":  # the rays that sit exactly on the +x face (its faces are binary fractions: no rounding) are not in the file
        on = np.nonzero(np.arange(257) % 32 == 18)[0]
        assert len(on) == 8 and not np.isin(on, want[2]).any()


def test_threshold_edges_and_a_lower_threshold():
    x = P.emit_inputs(512, 3, "mixed")
    kept_default = _run_emit(x)[2][2]
    at, above = np.arange(512) % 32 == 8, np.arange(512) % 32 == 9
    assert not np.isin(np.nonzero(at)[0], kept_default).any() and np.isin(np.nonzero(above)[0], kept_default).all()
    got, total, want, cap = _run_emit(x, threshold=0.1)
    _check_emit(got, total, want, cap)
    assert total > len(kept_default)


def test_cap_smaller_than_the_kept_count_leaves_the_guard_bytes_alone():
    x = P.emit_inputs(1031, 6, "all")
    for base, cap in ((0, 700), (300, 301), (1031, 1031), (2000, 1500), (0, 0)):
        got, total, want, cap = _run_emit(x, base=base, cap=cap)
        assert total == 1031
        rows, points, kept = got
        w = max(0, min(1031, cap - base))
        if w:
            assert np.array_equal(rows[base:base + w], want[0][:w]) and np.array_equal(kept[base:base + w], want[2][:w])
        lo = min(base, cap + 3)
        assert (rows[:lo] == GUARD).all() and (rows[lo + w:] == GUARD).all()
        assert (points[:lo] == -7.0).all() and (points[lo + w:] == -7.0).all() and (kept[:lo] == -7).all() and (kept[lo + w:] == -7).all()


def test_batches_append_behind_each_other():
    """Two batches through one running base give the rows of their concatenation."""
    from umhsnerf import ops

    a, b = P.emit_inputs(300, 2, "mixed", seed=1), P.emit_inputs(257, 2, "mixed", seed=2)
    wa, wb = (P.emit(x["o"], x["d"], x["depth"], x["acc"], x["rgb"], x["abund"], x["probs"], ordinal0=o) for x, o in ((a, 0), (b, 300)))
    cap = len(wa[2]) + len(wb[2]) - 5  # the surplus of the last batch is cut in draw order
    rows = torch.zeros(cap * 28, dtype=torch.uint8, device=DEV)
    points, kept = torch.zeros(cap, 3, device=DEV), torch.zeros(cap, dtype=torch.int64, device=DEV)
    base = torch.zeros(1, dtype=torch.int64, device=DEV)
    for x, o in ((a, 0), (b, 300)):
        t = [torch.from_numpy(x[k]).to(DEV) for k in ("o", "d", "depth", "acc", "rgb", "abund", "probs")]
        base += ops.pc_append(ops.pc_args(*t), rows, points, kept, base, o, cap)
    assert int(base) == cap + 5
    assert np.array_equal(rows.cpu().numpy().reshape(cap, 28), np.concatenate([wa[0], wb[0]])[:cap])
    assert np.array_equal(kept.cpu().numpy(), np.concatenate([wa[2], wb[2]])[:cap])
    assert np.array_equal(points.cpu().numpy().view(np.uint32), np.concatenate([wa[1], wb[1]])[:cap].view(np.uint32))


# ---- neighbours --------------------------------------------------------------------------------------------------------------------
def _check_knn(name, m, k, edge=None):
    from umhsnerf import ops

    pts = P.knn_points(name, m)
    want = P.knn_reference(name, m, k)
    got = ops.knn_mean_dist(torch.from_numpy(pts.copy()).to(DEV), k, edge=edge)
    assert got.dtype == torch.float32 and got.shape == (m,)
    got = got.cpu().numpy().astype(np.float64)
    err, bound = np.abs(got - want), P.knn_bound(want, k)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{name} M={m} k={k} edge={edge}: largest error / bound = {ratio:.3f}, largest error {float(err.max()):.3e}")
    assert (err <= bound).all(), (name, m, k, int((err > bound).sum()), float((err - bound).max()))
    return got, want


@pytest.mark.parametrize("name,m,k", P.knn_cases())
def test_mean_neighbour_distance_against_float64(name, m, k):
    got, want = _check_knn(name, m, k)
    if name == "identical":
        assert (got == 0).all()
    if name == "copies":
        copies = (P.knn_points(name, m) == np.array([0.125, -0.5, 0.75], dtype=np.float32)).all(axis=1)
        assert copies.sum() == 64 and (got[copies] == 0).all() and (got[~copies] > 0).all()


@pytest.mark.parametrize("name,m", [("cube", 4096), ("clusters", 333), ("plane", 4096), ("copies", 333)])
@pytest.mark.parametrize("scale", [1 / 16, 64.0])
def test_a_bad_grid_edge_changes_nothing(name, m, scale):
    """Exactness does not depend on the host's choice of the edge: much too small (nearly every cell empty, many rings) and much too
    large (a handful of cells, brute force inside them)."""
    from umhsnerf import ops

    _, edge, dims = ops.pc_grid(torch.from_numpy(P.knn_points(name, m).copy()).to(DEV))
    _, _, bad = ops.pc_grid(torch.from_numpy(P.knn_points(name, m).copy()).to(DEV), edge * scale)
    assert bad != dims
    _check_knn(name, m, 20, edge=edge * scale)


@pytest.mark.parametrize("name,m,k", [(s, m, k) for s, m, k in P.knn_cases() if k == 20 or m == 333])
def test_outlier_rule_against_float64(name, m, k):
    """mu, sigma (divisor M - 1) and the keep mask of ``remove_statistical_outliers`` against the float64 rule.  Every mean is within
    b_i = (k + 8) 2^-24 mean64_i, so |mu - mu64| <= mean(b) and, sigma being the norm of the centred vector over sqrt(M - 1),
    |sigma - sigma64| <= |got - want|_2 / sqrt(M - 1) <= sqrt(M / (M - 1)) max(b); a point's flag is compared when its float64 mean is
    farther from the float64 threshold than b_i plus the threshold's own error."""
    from umhsnerf.export import remove_statistical_outliers

    ratio = 2.0
    pts = torch.from_numpy(P.knn_points(name, m).copy()).to(DEV)
    keep, thr, means = remove_statistical_outliers(pts, k, ratio)
    want = P.knn_reference(name, m, k)
    b = P.knn_bound(want, k)
    mu64, s64, thr64, keep64 = P.outlier_rule(want, ratio)
    g = means.double()
    mu = float(g.mean())
    sigma = float(g.std(unbiased=True)) if m > 1 else 0.0
    tol_mu = float(b.mean()) + 1e-13 * mu64
    tol_s = (float(np.sqrt(m / (m - 1)) * b.max()) if m > 1 else 0.0) + 1e-13 * s64
    assert abs(mu - mu64) <= tol_mu and abs(sigma - s64) <= tol_s, (mu, mu64, sigma, s64)
    assert abs(float(thr) - thr64) <= tol_mu + ratio * tol_s
    sure = (np.abs(want - thr64) > b + tol_mu + ratio * tol_s) | (want == 0)  # (a mean of 0 is exact, and dropped whatever the threshold)
    got = keep.cpu().numpy()
    assert np.array_equal(got[sure], keep64[sure]) and sure.sum() >= m - 2
    assert not got[want == 0].any()  # exact duplicates more numerous than k drop out, as in Open3D
    if name == "copies":
        assert (~got).sum() >= 64
    if name == "clusters" and m == 4096 and k == 20:
        assert 0 < (~got).sum() < 200  # the stragglers go, the clusters stay


# ---- end to end --------------------------------------------------------------------------------------------------------------------
FLAGS = ["--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"]
N_POINTS, N_RAYS = 2000, 1024


def _pipeline(scene, meta):
    from test_hip_render import _datamanager
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=True, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2,
                                            datamanager=_datamanager(scene, 9))
    for step in range(3):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    return pipe


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Scene, two identically trained pipelines (one exports, its twin does not) and ONE export that the tests below share."""
    from test_hip_distortion import make_scene
    from umhsnerf.export import export_pointcloud

    root = tmp_path_factory.mktemp("export")
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    pipe, twin = _pipeline(scene, meta), _pipeline(scene, meta)
    dm = pipe.datamanager
    state = lambda: dict(gen=dm.generator.get_state().clone(), cursor=dm._eval_cursor, train_count=dm.train_count,
                         cuda=torch.cuda.get_rng_state(DEV).clone(), cpu=torch.get_rng_state().clone(), training=pipe.model.training)
    pipe.train()
    before = state()
    result = export_pointcloud(pipe, root / "out", num_points=N_POINTS, num_rays_per_batch=N_RAYS, spectra=True)
    return dict(root=root, scene=scene, pipe=pipe, twin=twin, before=before, after=state(), result=result)


def _replay(pipe, batches, seed=0, threshold=0.5, box=None):
    """The same batches (same seed) through ``model.forward``, and the restatement applied to them -> rows, points, kept, spectral."""
    split, model = pipe.datamanager.train_split, pipe.model
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    was = model.training
    model.eval()
    parts = []
    try:
        with torch.no_grad():
            for b in range(batches):
                rays, _ = split.sample(N_RAYS, gen)
                out = model(rays)
                h = lambda t: t.float().cpu().numpy()
                rows, pts, kept = P.emit(h(rays.origins), h(rays.directions), h(out["depth"]), h(out["accumulation"]), h(out["rgb"]),
                                         h(out["abundances"]), h(out["seg_probs"]), threshold, box, None, b * N_RAYS)
                parts.append((rows, pts, kept, h(out["spectral"])[kept - b * N_RAYS], h(out["seg_raw"])[kept - b * N_RAYS]))
    finally:
        model.train(was)
    return [np.concatenate([p[i] for p in parts]) for i in range(5)]


def test_export_equals_the_restatement_on_a_replay_of_its_batches(world):
    res, root = world["result"], world["root"]
    assert set(res) == {"points", "rays_drawn", "batches", "removed_outliers", "threshold", "file"}
    assert res["file"] == str(root / "out" / "point_cloud.ply") and res["rays_drawn"] == res["batches"] * N_RAYS
    assert res["points"] + res["removed_outliers"] == N_POINTS and res["threshold"] > 0
    table, raw = P.read_ply(res["file"])
    assert len(table) == res["points"] and raw.shape[1] == 20 + 4 * 3
    assert list(table.dtype.names) == ["x", "y", "z", "red", "green", "blue", "alpha", "material", "abundance_0", "abundance_1", "abundance_2"]
    rows, pts, kept, spectral, seg_raw = _replay(world["pipe"], res["batches"])
    assert len(kept) >= N_POINTS and (len(kept) - N_POINTS) < N_RAYS  # the last batch was needed; its surplus is cut in draw order
    rows, pts, kept, spectral, seg_raw = (a[:N_POINTS] for a in (rows, pts, kept, spectral, seg_raw))
    # the outlier rule on the float64 means of the replayed points: rows that are clear of the threshold must agree; with so few removed
    # the file must be the replay's rows minus a subset
    want64 = P.knn_mean64(pts, 20)
    b = P.knn_bound(want64, 20)
    mu64, s64, thr64, keep64 = P.outlier_rule(want64, 10.0)
    slack = b + float(b.mean()) + 10.0 * float(np.sqrt(N_POINTS / (N_POINTS - 1)) * b.max())
    sure = np.abs(want64 - thr64) > slack
    assert abs(res["threshold"] - thr64) <= slack.max()
    assert sure.all(), "a point of this scene sits within rounding of the outlier threshold: pick another seed for the test"
    assert np.array_equal(raw, rows[keep64])
    # every point satisfies the keep rule, independently of the replay
    assert (table["alpha"] >= 127).all()  # accumulation > 0.5: (uint8)(a * 255) >= 127
    assert np.isfinite(np.stack([table["x"], table["y"], table["z"]], 1)).all()
    assert ((table["material"] >= 0) & (table["material"] < 3)).all()
    assert np.array_equal(table["material"], seg_raw[keep64].astype(np.int32))  # accumulation > 0.5: seg_raw is the label itself
    # inside the scene: between a camera (within the unit box) and the outermost occupancy level, the +/-1 scene box x 2^(4 - 1)
    assert np.abs(np.stack([table["x"], table["y"], table["z"]], 1)).max() <= 8.0 + 1e-4
    # --spectra: the rows of outputs["spectral"] at `kept`, in file order
    cube = np.load(root / "out" / "point_cloud_spectral.npy")
    assert cube.dtype == np.float32 and np.array_equal(cube, spectral[keep64])


def test_two_runs_give_the_same_bytes_and_another_seed_other_bytes(world):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    first = (root / "out" / "point_cloud.ply").read_bytes()
    again = export.export_pointcloud(pipe, root / "again", num_points=N_POINTS, num_rays_per_batch=N_RAYS, spectra=True)
    assert (root / "again" / "point_cloud.ply").read_bytes() == first and again == {**world["result"], "file": again["file"]}
    assert (root / "again" / "point_cloud_spectral.npy").read_bytes() == (root / "out" / "point_cloud_spectral.npy").read_bytes()
    other = export.export_pointcloud(pipe, root / "seed1", num_points=N_POINTS, num_rays_per_batch=N_RAYS, seed=1)
    assert (root / "seed1" / "point_cloud.ply").read_bytes() != first and other["points"] > 0


def test_the_command_line_writes_the_same_file_from_a_checkpoint(world, capsys):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    torch.save({"step": 3, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    want = export.export_pointcloud(pipe, root / "inproc", num_points=N_POINTS, num_rays_per_batch=N_RAYS, spectra=True)
    capsys.readouterr()
    got = export.main(["pointcloud", "--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"), "--output-dir",
                       str(root / "cli"), "--num-points", str(N_POINTS), "--num-rays-per-batch", str(N_RAYS), "--spectra", *FLAGS])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got == {**want, "file": str(root / "cli" / "point_cloud.ply")}
    assert (root / "cli" / "point_cloud.ply").read_bytes() == (root / "inproc" / "point_cloud.ply").read_bytes()
    assert (root / "cli" / "point_cloud_spectral.npy").read_bytes() == (root / "inproc" / "point_cloud_spectral.npy").read_bytes()
    table, _ = P.read_ply(root / "cli" / "point_cloud.ply")
    assert len(table) == got["points"] and np.abs(np.stack([table["x"], table["y"], table["z"]], 1)).max() <= 8.0 + 1e-4


def test_material_world_frame_box_and_the_empty_box(world):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    base = export.export_pointcloud(pipe, root / "m_all", num_points=N_POINTS, num_rays_per_batch=N_RAYS, spectra=True)
    table, raw = P.read_ply(base["file"])
    cube = np.load(root / "m_all" / "point_cloud_spectral.npy")
    counts = np.bincount(table["material"], minlength=3)
    print("points per material:", counts.tolist())
    for K in range(3):
        res = export.export_pointcloud(pipe, root / f"m_{K}", num_points=N_POINTS, num_rays_per_batch=N_RAYS, spectra=True, material=K)
        _, rawk = P.read_ply(res["file"])
        assert res["points"] == counts[K] and np.array_equal(rawk, raw[table["material"] == K])
        assert np.array_equal(np.load(root / f"m_{K}" / "point_cloud_spectral.npy"), cube[table["material"] == K])
    # world frame: the same rows, xyz through the affine (identity transform and scale of a resident datamanager: p * 1 + 0 ...)
    out = pipe.datamanager.train_dataparser_outputs
    A = export.world_frame_affine(out.dataparser_transform, out.dataparser_scale)
    res = export.export_pointcloud(pipe, root / "wf", num_points=N_POINTS, num_rays_per_batch=N_RAYS, save_world_frame=True)
    tw, raww = P.read_ply(res["file"])
    assert np.array_equal(raww[:, 12:], raw[:, 12:])
    assert np.array_equal(np.stack([tw["x"], tw["y"], tw["z"]], 1), P.world_of(np.stack([table["x"], table["y"], table["z"]], 1), A))
    # a box: exactly the replayed rows that the restatement keeps with it; every point strictly inside
    box = dict(obb_center=[0.1, 0.0, -0.1], obb_rotation=[0.2, -0.3, 0.5], obb_scale=[3.0, 3.6, 2.4])
    res = export.export_pointcloud(pipe, root / "box", num_points=500, num_rays_per_batch=N_RAYS, remove_outliers=False, **box)
    tb, rawb = P.read_ply(res["file"])
    obb = export.obb_from_params(box["obb_center"], box["obb_rotation"], box["obb_scale"])
    rows = _replay(pipe, res["batches"], box=obb)[0]
    print(f"box: 500 points from {res['rays_drawn']} rays")
    assert res["points"] == 500 and np.array_equal(rawb, rows[:500]) and res["threshold"] is None and res["removed_outliers"] == 0
    q = P.box_coordinates(np.stack([tb["x"], tb["y"], tb["z"]], 1), obb)
    assert (np.abs(q) < obb[2] / 2).all()
    # an empty box: 64 batches that keep nothing, then the error -- and the mode is restored
    with pytest.raises(RuntimeError, match="nothing kept in 64 consecutive batches"):
        export.export_pointcloud(pipe, root / "empty", num_points=10, num_rays_per_batch=256, obb_center=[50, 50, 50], obb_rotation=[0, 0, 0],
                                 obb_scale=[0.1, 0.1, 0.1])
    assert pipe.model.training


def test_export_leaves_the_training_state_alone(world):
    """(Last: it takes a training step.)"""
    pipe, twin, before, after = world["pipe"], world["twin"], world["before"], world["after"]
    dm = pipe.datamanager
    # around the fixture's export: mode, the datamanager's generator, cursor and count, and the global generators
    assert before["training"] and after["training"]
    assert torch.equal(after["gen"], before["gen"]) and after["cursor"] == before["cursor"] and after["train_count"] == before["train_count"]
    assert torch.equal(after["cuda"], before["cuda"]) and torch.equal(after["cpu"], before["cpu"])
    # and still, after every other export of this module (the command line built a pipeline of its own: the global generators moved)
    assert torch.equal(dm.generator.get_state(), before["gen"]) and dm._eval_cursor == before["cursor"] and dm.train_count == before["train_count"]
    pipe.model.eval()
    from umhsnerf.export import export_pointcloud

    export_pointcloud(pipe, world["root"] / "evalmode", num_points=300, num_rays_per_batch=N_RAYS, remove_outliers=False)
    assert not pipe.model.training
    pipe.model.train()
    # the next training step is the one a pipeline that never exported takes
    # (both pipelines draw their stratified jitter and random background from the global generators: each takes the step from the
    # state in which the three steps of the fixture left them)
    states = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    _, la, _ = pipe.get_train_loss_dict(3)
    torch.cuda.set_rng_state(states[0], DEV)
    torch.set_rng_state(states[1])
    _, lb, _ = twin.get_train_loss_dict(3)
    assert set(la) == set(lb)
    for k in la:
        assert torch.equal(la[k].detach(), lb[k].detach()), k
