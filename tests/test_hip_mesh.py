"""Mesh export on the GPU.

Fusion: ``umhs_tsdf_integrate`` (``ops.tsdf_integrate``) against the float64 run of tests/mesh_ref.py within the one rule
|got - ref64| <= K_FUSE u (mag + tiny) on every element that is not on an edge, W and Wc exact; the split calls bit for bit.
Extraction: ``umhs_mesh_mark`` / ``umhs_mesh_vertices`` / ``umhs_mesh_triangles`` (``ops.mesh_extract``) must give the restatement's
integers and bits -- ``==`` on every index, on every byte of every row and on the guard bytes behind both outputs.
End to end: the tiny scene of tests/test_hip_render.py (``make_scene``, 3 classes, ``pred_specular``), trained for N_STEPS steps."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_ROWS = 3
_report = {}


# ---- fusion ------------------------------------------------------------------------------------------------------------------------
def _strided(a, chan):
    """The image stack as the interior of a wider, taller device tensor with spare channels: read in place at its strides."""
    t = torch.from_numpy(a if chan else a[..., None])
    n, h, w, k = t.shape
    wide = torch.full((n, h + 1, w + 3, k + 2), 77.0, dtype=torch.float32)
    wide[:, :h, 2:2 + w, 1:1 + k] = t
    v = wide.to(DEV)[:, :h, 2:2 + w, 1:1 + k]
    return v if chan else v[..., 0]


def _volume(case):
    from umhsnerf import ops

    return ops.tsdf_volume(case["lo"], case["h"], case["dims"], case["C"], DEV)


def _integrate(case, vol, cameras, strided):
    from umhsnerf import ops

    idx = list(cameras)
    up = (lambda a, chan: _strided(a[idx], chan)) if strided else (lambda a, chan: torch.from_numpy(a[idx]).to(DEV))
    cams = [case["cams"][i] for i in idx]
    c2w = np.stack([np.concatenate([c["R"], c["t"][:, None]], 1) for c in cams])
    intr = np.array([[c["fx"], c["fy"], c["cx"], c["cy"]] for c in cams], np.float32)
    dist = np.stack([np.zeros(6, np.float32) if c["dist"] is None else c["dist"] for c in cams])
    ops.tsdf_integrate(vol, c2w, intr, dist, up(case["depth"], False), up(case["acc"], False), up(case["rgb"], True),
                       up(case["abund"], True) if case["C"] else None, up(case["probs"], True) if case["C"] else None,
                       case["threshold"], case["trunc"])


def _host(vol):
    return {k: vol[k].cpu().numpy() for k in ("D", "W", "Wc", "A")}


@pytest.mark.parametrize("dims", [(13, 10, 9), (1, 1, 1)])
@pytest.mark.parametrize("C", [0, 3, 16])
def test_fusion_is_within_the_bound_of_float64(dims, C):
    """13 x 10 x 9 = 1,170 points are five chunks, the last partial.  Strided images, background pixels, NaN / inf depths, a wall that
    occludes half the volume, a distorted camera and one behind the volume (tests/mesh_ref.py ``fusion_case``)."""
    case = M.fusion_case(dims, C)
    r64 = M.fuse_case(case, np.float64)
    vol = _volume(case)
    _integrate(case, vol, range(3), strided=True)
    got = _host(vol)
    keep = ~r64["edge"]
    ratios, left_out = M.fuse_ratios(got, r64)
    r32 = M.fuse_case(case, np.float32)
    same = {k: bool(np.array_equal(got[k].view(np.uint32), r32[k].view(np.uint32))) for k in ("D", "W", "Wc", "A")}
    print(f"dims {dims} C {C}: worst ratios {ratios}, left out {left_out:.4f}, bits equal to the float32 restatement: {same}")
    _report[f"{'x'.join(map(str, dims))}-C{C}"] = {**ratios, "left_out": left_out, "bits_equal_f32": same}
    with open(os.path.join(_report_dir(), "mesh_f64.json"), "w") as f:
        json.dump(_report, f, indent=1)
    assert left_out <= 0.02
    assert np.array_equal(got["W"][keep], r64["W"][keep].astype(np.float32)) and np.array_equal(got["Wc"][keep], r64["Wc"][keep].astype(np.float32))
    assert ratios["D"] <= M.K_FUSE and ratios["A"] <= M.K_FUSE
    if np.prod(dims) > 1:
        assert (got["W"] == 1).any() and (got["W"] == 2).any() and (got["Wc"] == 0).any() and (got["Wc"] == 2).any()


def _report_dir():
    from rays_f64 import report_dir

    return report_dir(ROOT)


@pytest.mark.parametrize("C", [0, 3])
def test_split_calls_are_bit_identical(C):
    case = M.fusion_case((13, 10, 9), C)
    one = _volume(case)
    _integrate(case, one, range(3), strided=False)
    one = _host(one)
    for first in ([0], [0, 1]):
        vol = _volume(case)
        _integrate(case, vol, first, strided=True)
        _integrate(case, vol, [c for c in range(3) if c not in first], strided=False)
        two = _host(vol)
        for k in one:
            assert np.array_equal(one[k].view(np.uint32), two[k].view(np.uint32)), (first, k)


def test_more_cameras_than_one_launch_holds():
    """20 cameras are two launches (16 + 4): the bits of 20 single-camera calls."""
    case = M.fusion_case((13, 10, 9), 3)
    order = [0, 1, 2, 1, 0] * 4
    big = {**case, "cams": [case["cams"][i] for i in order], **{k: case[k][order] for k in ("depth", "acc", "rgb", "abund", "probs")}}
    a, b = _volume(big), _volume(big)
    _integrate(big, a, range(20), strided=False)
    for i in range(20):
        _integrate(big, b, [i], strided=False)
    a, b = _host(a), _host(b)
    assert a["W"].max() == 16  # (the camera behind the volume, 4 times, adds nothing)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def _device_volume(D, W, Wc, A, lo, h, dims):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return {"D": t(D), "W": t(W), "Wc": t(Wc), "A": t(A), "lo": tuple(float(v) for v in lo), "h": float(h), "dims": tuple(dims),
            "n_classes": (A.shape[0] - 3) // 2}


def _check_extract(name, dims, C=3, world=None):
    from umhsnerf import ops

    lo, h, _ = M.cube_lattice(max(max(dims), 3))
    D, W, Wc, A = M.field(name, lo, h, dims, C=C)
    want = M.extract(D, W, Wc, A, lo, h, dims, world=world)
    got = ops.mesh_extract(_device_volume(D, W, Wc, A, lo, h, dims), world=world, guard_rows=GUARD_ROWS)
    rows, faces = got["rows"].cpu().numpy(), got["faces"].cpu().numpy()
    assert rows.shape == want["rows"].shape and faces.shape == want["faces"].shape, (rows.shape, want["rows"].shape, faces.shape)
    assert np.array_equal(faces, want["faces"])
    assert np.array_equal(rows, want["rows"])
    rb = M.row_bytes(C)
    assert (got["rows_buffer"].cpu().numpy()[len(rows) * rb:] == 0xA5).all() and got["rows_buffer"].numel() == (len(rows) + GUARD_ROWS) * rb
    tail = got["faces_buffer"].cpu().numpy()[len(faces) * 3:]
    assert len(tail) == 3 * GUARD_ROWS and (tail.view(np.uint32) == 0xA5A5A5A5).all()
    return want


@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 2, 2), (17, 9, 5), (33, 33, 33)])
@pytest.mark.parametrize("name", ["sphere", "random", "outside", "slab"])
def test_extraction_equals_the_restatement(dims, name):
    want = _check_extract(name, dims)
    if name == "outside":
        assert len(want["rows"]) == 0 and len(want["faces"]) == 0
    if name == "slab" or (name == "random" and np.prod(dims) > 100):
        assert len(want["faces"]) > 0
    if name == "random" and np.prod(dims) < 100:  # the holes leave no whole cell: vertices, but not one face
        assert len(want["rows"]) > 0 and len(want["faces"]) == 0
    if name == "slab":  # the plane cuts every row along x: every chunk of 256 lattice indices owns vertices
        owners = np.nonzero(want["mask"])[0] // 256
        assert len(np.unique(owners)) == (np.prod(dims) + 255) // 256
    if name == "sphere" and dims == (33, 33, 33):
        assert M.closed_and_oriented(want["faces"], len(want["rows"])) and M.euler(want["faces"], len(want["rows"])) == 2


@pytest.mark.parametrize("C", [0, 16])
def test_extraction_row_layouts_and_the_world_affine(C):
    _check_extract("random", (17, 9, 5), C=C)
    _check_extract("sphere", (17, 9, 5), C=C, world=M.WORLD)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
N_STEPS = 3  # the fewest training steps of this scene and seed that leave a surface inside the box (a non-empty mesh)
RES = 24
FLAGS = ["--num-classes", "3", "--pred-specular", "--temperature", "0.4", "--background-color", "black"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from test_hip_distortion import make_scene
    from test_hip_render import _datamanager
    from umhsnerf.export import export_tsdf_mesh
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    root = tmp_path_factory.mktemp("mesh")
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
    result = export_tsdf_mesh(pipe, root / "out", resolution=RES, downscale_factor=1, batch_size=4)
    return dict(root=root, scene=scene, pipe=pipe, before=before, after=state(), result=result)


def test_export_writes_a_consistent_labelled_mesh(world):
    res, root = world["result"], world["root"]
    assert set(res) == {"vertices", "faces", "cameras", "resolution", "voxel_size", "truncation", "file"}
    assert res["file"] == str(root / "out" / "mesh.ply") and res["cameras"] == 6 and res["resolution"] == [RES] * 3
    assert res["voxel_size"] == float(np.float32(2.0 / (RES - 1))) and res["truncation"] == float(np.float32(5.0 * res["voxel_size"]))
    table, rows, faces = M.read_mesh_ply(res["file"])  # (the reader asserts that the header matches the payload)
    print(f"mesh after {N_STEPS} steps: {len(table)} vertices, {len(faces)} faces, labels {np.bincount(table['material'] + 1, minlength=4).tolist()}")
    assert len(table) == res["vertices"] > 0 and len(faces) == res["faces"] > 0
    assert list(table.dtype.names) == ["x", "y", "z", "red", "green", "blue", "material", "abundance_0", "abundance_1", "abundance_2"]
    assert faces.min() >= 0 and faces.max() < len(table)
    assert ((table["material"] >= -1) & (table["material"] < 3)).all()
    pos = np.stack([table["x"], table["y"], table["z"]], 1)
    assert np.isfinite(pos).all() and np.abs(pos).max() <= 1.0 + 1e-5  # inside the box


def test_export_equals_the_restatement_on_the_same_renders(world):
    """The same cameras rendered by hand (same batches), fused and extracted by tests/mesh_ref.py in float32: the same faces, and --
    the kernels being the restatement operation for operation -- the same rows.  No fused point may lie within its bound of zero
    (there a float32 evaluation in another order could decide the sign otherwise): asserted on the float64 run."""
    from umhsnerf import export

    pipe, res = world["pipe"], world["result"]
    model, split = pipe.model, pipe.datamanager.train_split
    cams = export.tsdf_cameras(split, 1)
    assert (cams["height"], cams["width"]) == (24, 32)
    names = ["depth", "rgb", "accumulation", "abundances", "seg_probs"]
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            parts = [export.render_cameras(model, cams, b, min(b + 4, 6), names) for b in (0, 4)]
    finally:
        model.train(was)
    img = {k: torch.cat([p[k] for p in parts]).float().cpu().numpy() for k in names}
    lo, h, dims = export.tsdf_lattice([-1, -1, -1], [1, 1, 1], RES)
    dist = cams["distortion_host"]
    mcams = [M.camera(cams["c2w_host"][i], *cams["intrinsics_host"][i], None if dist is None else dist[i]) for i in range(6)]
    args = (lo, h, dims, mcams, img["depth"][..., 0], img["accumulation"][..., 0], img["rgb"], img["abundances"], img["seg_probs"], 0.5,
            res["truncation"])
    r32, r64 = M.fuse(*args, F=np.float32), M.fuse(*args, F=np.float64)
    seen = r64["W"] > 0
    bound = M.K_FUSE * M.U * (r64["mag_D"] + M.TINY)
    print(f"points seen {int(seen.sum())} of {seen.size}, on an edge {int(r64['edge'].sum())}, smallest |D| / bound "
          f"{float((np.abs(r64['D'][seen]) / bound[seen]).min()):.3g}")
    assert (np.abs(r64["D"][seen]) > bound[seen]).all(), "a fused point sits within rounding of zero: pick another seed for the test"
    want = M.extract(r32["D"], r32["W"], r32["Wc"], r32["A"], lo, h, dims)
    _, rows, faces = M.read_mesh_ply(res["file"])
    assert np.array_equal(faces, want["faces"])
    assert np.array_equal(rows, want["rows"])


def test_material_and_world_frame(world):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    table, rows, faces = M.read_mesh_ply(world["result"]["file"])
    label = table["material"]
    kept = 0
    for K in range(3):
        res = export.export_tsdf_mesh(pipe, root / f"m_{K}", resolution=RES, downscale_factor=1, batch_size=4, material=K)
        tk, rk, fk = M.read_mesh_ply(res["file"])
        want = faces[(label[faces] == K).all(1)]
        assert res["faces"] == len(want) == len(fk) and res["vertices"] == len(tk)
        assert (tk["material"] == K).all()
        if len(fk):
            assert np.array_equal(np.unique(fk), np.arange(len(tk)))  # no unreferenced vertex
            assert np.array_equal(rk[fk], rows[want])
        kept += len(fk)
    assert 0 < kept <= len(faces)
    out = pipe.datamanager.train_dataparser_outputs
    A = export.world_frame_affine(out.dataparser_transform, out.dataparser_scale)
    res = export.export_tsdf_mesh(pipe, root / "wf", resolution=RES, downscale_factor=1, batch_size=4, save_world_frame=True)
    tw, rw, fw = M.read_mesh_ply(res["file"])
    assert np.array_equal(fw, faces) and np.array_equal(rw[:, 12:], rows[:, 12:])
    p = np.stack([table["x"], table["y"], table["z"]], 1)
    want = np.stack([((A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]) + A[r, 3] for r in range(3)], 1).astype(np.float32)
    assert np.array_equal(np.stack([tw["x"], tw["y"], tw["z"]], 1).view(np.uint32), want.view(np.uint32))


def test_the_command_line_writes_the_same_file_from_a_checkpoint(world, capsys):
    from umhsnerf import export

    root, pipe = world["root"], world["pipe"]
    torch.save({"step": N_STEPS, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    capsys.readouterr()
    got = export.main(["tsdf", "--data", str(world["scene"]), "--checkpoint", str(root / "step-000000003.ckpt"), "--output-dir",
                       str(root / "cli"), "--resolution", str(RES), "--downscale-factor", "1", "--batch-size", "4", *FLAGS])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got == {**world["result"], "file": str(root / "cli" / "mesh.ply")}
    assert (root / "cli" / "mesh.ply").read_bytes() == (root / "out" / "mesh.ply").read_bytes()


def test_export_leaves_the_training_state_alone(world):
    pipe, before, after = world["pipe"], world["before"], world["after"]
    dm = pipe.datamanager
    assert before["training"] and after["training"]
    assert torch.equal(after["gen"], before["gen"]) and after["cursor"] == before["cursor"] and after["train_count"] == before["train_count"]
    assert torch.equal(after["cuda"], before["cuda"]) and torch.equal(after["cpu"], before["cpu"])
    assert torch.equal(dm.generator.get_state(), before["gen"]) and dm._eval_cursor == before["cursor"] and dm.train_count == before["train_count"]
    pipe.model.eval()
    from umhsnerf.export import export_tsdf_mesh

    export_tsdf_mesh(pipe, world["root"] / "evalmode", resolution=12, downscale_factor=2, batch_size=8)
    assert not pipe.model.training
    pipe.model.train()
