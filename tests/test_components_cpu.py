"""Mesh components without a GPU: the numpy restatement of tests/components_ref.py against a brute-force flood fill, its float32 areas
inside the bound derived there of the float64 oracle on every mesh tests/test_hip_components.py uses, the keep rules (the restatement's
and ``export.component_keep_mask`` on CPU tensors), and the command line."""
import numpy as np
import pytest
import torch

import components_ref as R

BASE = ["--data", "scene", "--checkpoint", "step.ckpt", "--output-dir", "out"]


def _flood_labels(V, faces):
    """The smallest vertex reachable from every vertex through the edges of valid faces: adjacency sets and a flood per vertex."""
    adj = [set() for _ in range(V)]
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        if all(0 <= i < V for i in (a, b, c)):
            for i, j in ((a, b), (b, c), (a, c)):
                adj[i].add(j), adj[j].add(i)
    out = np.full(V, -1, np.int64)
    for v in range(V):  # ascending: the first vertex to reach a component is its smallest
        if out[v] >= 0:
            continue
        out[v], todo = v, [v]
        while todo:
            for j in adj[todo.pop()]:
                if out[j] < 0:
                    out[j] = v
                    todo.append(j)
    return out


@pytest.mark.parametrize("name", ["hand_c3", "interleaved_strips", "strip_chunk_plus_1", "permuted_strip", "fan", "random_c0"])
def test_the_restatement_equals_a_flood_fill(name):
    rows, faces, C, comp = R.case(name)
    V = len(rows)
    want = _flood_labels(V, faces)
    assert np.array_equal(comp["label"], want)
    ids = np.unique(want)
    assert comp["n_components"] == len(ids) and np.array_equal(ids[comp["vertex_component"]], want)  # ids ascend by smallest vertex
    ok = R.valid_faces(faces, V)
    assert (comp["face_component"][~ok] == -1).all()
    assert np.array_equal(comp["face_component"][ok], comp["vertex_component"][faces[ok, 0]])
    for k in range(3):  # one component per valid face
        assert np.array_equal(comp["face_component"][ok], comp["vertex_component"][faces[ok, k]])
    assert comp["faces"].sum() == ok.sum() and comp["vertices"].sum() == V
    assert np.array_equal(comp["faces"], np.bincount(comp["face_component"][ok], minlength=comp["n_components"]))


def test_the_hand_made_mesh_by_hand():
    rows, faces, C, comp = R.case("hand_c3")
    assert comp["label"].tolist() == [0, 0, 0, 0, 4, 5, 5, 7, 8, 8, 8, 11, 12, 0]
    assert comp["vertex_component"].tolist() == [0, 0, 0, 0, 1, 2, 2, 3, 4, 4, 4, 5, 6, 0]
    assert comp["face_component"].tolist() == [0, 0, 0, 2, 3, 4, -1, -1, -1, 0, 4]
    assert comp["faces"].tolist() == [4, 0, 1, 1, 2, 0, 0] and comp["vertices"].tolist() == [5, 1, 2, 1, 3, 1, 1]
    assert comp["face_area"][5] == 0 and comp["face_area"][3] == 0 and comp["face_area"][0] == 0.5  # NaN corner; repeated index; half a unit square
    assert comp["area"][4] == 0 and comp["area"][0] > 1.0


def test_the_volumes_of_the_issue():
    """The figures the issue measured on the n = 24, C = 3 volumes."""
    rows, faces, C, comp = R.case("random_c3")
    assert (len(rows), len(faces), comp["n_components"]) == (29257, 15844, 15856)
    assert int((comp["faces"] == 0).sum()) == 15386 and int((comp["faces"] < 8).sum()) == 15605
    assert sorted(comp["faces"].tolist(), reverse=True)[:5] == [2502, 1018, 840, 606, 588]
    for name in ("sphere", "two_spheres"):
        assert R.case(name)[3]["n_components"] == 1


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_the_float32_areas_are_within_the_bound_of_the_float64_oracle(name):
    rows, faces, C, comp = R.case(name)
    area64, bound = R.area_oracle(rows, faces, C, comp["face_component"], comp["n_components"])
    err = np.abs(comp["area"] - area64)
    assert np.isfinite(comp["area"]).all() and (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    faced = comp["faces"] > 0
    if name.startswith(("random", "sphere", "two_spheres")):
        assert (bound[faced] < 1e-5 * np.maximum(area64[faced], 1e-3)).all()  # the bound is tight enough to mean something
    # a face area off by one part in 10^5 is outside it
    if faced.any() and area64[faced].max() > 0:
        c = int(np.argmax(area64))
        assert abs(area64[c] * (1 + 1e-5) - area64[c]) > bound[c]


def test_the_keep_rules():
    from umhsnerf import export

    nf = np.array([5, 0, 9, 5, 1, 9, 2, 0, 5], np.int64)
    t = torch.from_numpy(nf)
    cases = [dict(), dict(min_component_faces=1), dict(min_component_faces=5), dict(min_component_faces=10),
             dict(min_component_fraction=1.0), dict(min_component_fraction=5 / 9), dict(min_component_fraction=0.56), dict(min_component_fraction=1e-9),
             dict(keep_largest_components=1), dict(keep_largest_components=2), dict(keep_largest_components=3), dict(keep_largest_components=4),
             dict(keep_largest_components=100), dict(min_component_faces=5, keep_largest_components=3),
             dict(min_component_faces=6, min_component_fraction=0.5, keep_largest_components=1)]
    for kw in cases:
        want = R.keep_mask(nf, **kw)
        assert np.array_equal(export.component_keep_mask(t, **kw).numpy(), want), kw
        assert not want[nf == 0].any(), kw  # a component without a face is never kept
    assert R.keep_mask(nf).tolist() == [True, False, True, True, True, True, True, False, True]
    assert R.keep_mask(nf, min_component_fraction=1.0).tolist() == [c in (2, 5) for c in range(9)]
    assert R.keep_mask(nf, keep_largest_components=1).tolist() == [c == 2 for c in range(9)]  # the tie of 9 and 9: the smaller id
    assert R.keep_mask(nf, keep_largest_components=3).tolist() == [c in (0, 2, 5) for c in range(9)]  # the tie of the three fives too
    assert R.keep_mask(nf, keep_largest_components=4).tolist() == [c in (0, 2, 3, 5) for c in range(9)]
    assert R.keep_mask(nf, min_component_faces=5, keep_largest_components=3).tolist() == [c in (0, 2, 5) for c in range(9)]  # AND, not "then"
    assert R.keep_mask(nf, min_component_fraction=5 / 9).tolist() == [n >= 5 for n in nf]  # 9 * (5 / 9) in float64 is exactly 5
    assert R.keep_mask(nf, min_component_fraction=0.56).tolist() == [n >= 9 for n in nf]
    assert export.component_keep_mask(t[:0], keep_largest_components=2).shape == (0,) and R.keep_mask(nf[:0], min_component_fraction=0.5).shape == (0,)
    comp = dict(faces=nf, vertices=nf + 2, area=nf * 0.5)
    assert [r["faces"] for r in R.table(comp, R.keep_mask(nf))] == [9, 9, 5, 5, 5, 2, 1]
    assert R.table(comp, R.keep_mask(nf, keep_largest_components=1)) == [{"faces": 9, "vertices": 11, "area": 4.5}]


def test_the_emit_restated():
    rows, faces, C, comp = R.case("hand_c3")
    out = R.emit(rows, faces, C, comp, np.ones(comp["n_components"], bool))
    assert out["vertex_map"].tolist() == [0, 1, 2, 3, -1, 4, 5, 6, 7, 8, 9, -1, -1, 10]  # 4, 11 and 12: no emitted face names them
    assert out["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [4, 4, 5], [6, 6, 6], [7, 8, 9], [10, 2, 3], [9, 7, 9]]
    assert np.array_equal(out["rows"], rows[out["vertex_map"] >= 0])
    only = R.emit(rows, faces, C, comp, np.arange(comp["n_components"]) == 4)
    assert only["faces"].tolist() == [[0, 1, 2], [2, 0, 2]] and np.array_equal(only["rows"], rows[8:11])


@pytest.mark.parametrize("command", ["tsdf", "textured-mesh"])
def test_the_command_line(command, capsys):
    from umhsnerf import export

    before = {"command", "data", "checkpoint", "output_dir", "resolution", "bounding_box_min", "bounding_box_max", "downscale_factor", "batch_size",
              "truncation_voxels", "depth_output_name", "rgb_output_name", "save_world_frame", "opacity_threshold", "material",
              "simplify_cell_voxels", "simplify_faces"}
    a = export.parse_args([command, *BASE])
    assert a.min_component_faces is None and a.min_component_fraction is None and a.keep_largest_components is None
    assert before <= set(vars(a)) and (a.resolution, a.material, a.simplify_faces, a.simplify_cell_voxels, a.save_world_frame) == ([128], None, None, None, False)
    assert (a.downscale_factor, a.batch_size, a.truncation_voxels, a.opacity_threshold) == (2, 8, 5.0, 0.5) and not hasattr(a, "material_edits")
    a = export.parse_args([command, *BASE, "--min-component-faces", "8", "--min-component-fraction", "0.02", "--keep-largest-components", "3",
                           "--material", "1", "--simplify-faces", "50000"])
    assert (a.min_component_faces, a.min_component_fraction, a.keep_largest_components, a.material, a.simplify_faces) == (8, 0.02, 3, 1, 50000)
    assert export.parse_args([command, *BASE, "--min-component-fraction", "1"]).min_component_fraction == 1.0
    for bad, word in ((["--min-component-faces", "0"], "at least 1"), (["--min-component-faces", "-3"], "at least 1"),
                      (["--min-component-fraction", "0"], "above 0"), (["--min-component-fraction", "1.5"], "at most 1"),
                      (["--min-component-fraction", "nan"], "above 0"), (["--min-component-fraction", "-0.1"], "above 0"),
                      (["--keep-largest-components", "0"], "at least 1"), (["--keep-largest-components", "-1"], "at least 1")):
        with pytest.raises(SystemExit):
            export.parse_args([command, *BASE, *bad])
        assert word in capsys.readouterr().err, bad


def test_the_flags_are_the_mesh_exports_own_and_the_functions_refuse_the_same_values(capsys):
    from umhsnerf import export

    p = vars(export.parse_args(["pointcloud", *BASE]))
    assert not {"min_component_faces", "min_component_fraction", "keep_largest_components"} & set(p)
    for flag in ("--min-component-faces", "--min-component-fraction", "--keep-largest-components"):
        with pytest.raises(SystemExit):
            export.parse_args(["pointcloud", *BASE, flag, "1"])
    capsys.readouterr()
    for kw in (dict(min_component_faces=0), dict(min_component_fraction=0.0), dict(min_component_fraction=1.01), dict(min_component_fraction=float("nan")),
               dict(keep_largest_components=0)):
        with pytest.raises(ValueError, match="component"):
            export.clean_mesh(None, None, 3, **kw)  # refused before anything is touched
        with pytest.raises(ValueError, match="component"):
            export.export_tsdf_mesh(None, "out", **kw)
        with pytest.raises(ValueError, match="component"):
            export.export_textured_mesh(None, "out", **kw)
        with pytest.raises(ValueError, match="component"):
            export.component_keep_mask(torch.zeros(3, dtype=torch.int64), **kw)
