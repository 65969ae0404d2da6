"""Mesh simplification without a GPU: the parser, the numpy restatement of tests/simplify_ref.py on the marching-tetrahedra sphere and
torus (identity, topology, volume, the empty result), the host logic of ``--simplify-faces`` (ladder, bisection) and planted faults."""
import numpy as np
import pytest

import mesh_ref as M
import simplify_ref as S

BASE = ["--data", "scene", "--checkpoint", "step.ckpt", "--output-dir", "out"]


# ---- parser --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("command", ["tsdf", "textured-mesh"])
def test_parser_flags_defaults_exclusion_and_refusals(command, capsys):
    from umhsnerf import export

    a = export.parse_args([command, *BASE])
    assert a.simplify_cell_voxels is None and a.simplify_faces is None
    a = export.parse_args([command, *BASE, "--simplify-cell-voxels", "2.5"])
    assert a.simplify_cell_voxels == 2.5 and a.simplify_faces is None
    a = export.parse_args([command, *BASE, "--simplify-faces", "50000"])
    assert a.simplify_faces == 50000 and a.simplify_cell_voxels is None
    for bad, word in ((["--simplify-cell-voxels", "2", "--simplify-faces", "10"], "not allowed with"), (["--simplify-faces", "0"], "at least 1"),
                      (["--simplify-cell-voxels", "0"], "positive"), (["--simplify-cell-voxels", "-1"], "positive"),
                      (["--simplify-cell-voxels", "nan"], "positive")):
        with pytest.raises(SystemExit):
            export.parse_args([command, *BASE, *bad])
        assert word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        export.parse_args([command, *BASE, "--target-num-faces", "50000"])
    err = capsys.readouterr().err
    assert "decimator" in err and "--simplify-faces" in err


def test_the_pointcloud_parser_is_unchanged(capsys):
    from umhsnerf import export

    p = vars(export.parse_args(["pointcloud", *BASE]))
    assert "simplify_faces" not in p and "simplify_cell_voxels" not in p
    for flag in ("--simplify-faces", "--simplify-cell-voxels"):
        with pytest.raises(SystemExit):
            export.parse_args(["pointcloud", *BASE, flag, "3"])
    capsys.readouterr()


def test_the_export_functions_refuse_both_flags_and_bad_values():
    from umhsnerf import export

    for kw in (dict(simplify_cell_voxels=2.0, simplify_faces=10), dict(simplify_faces=0), dict(simplify_cell_voxels=0.0),
               dict(simplify_cell_voxels=float("inf"))):
        with pytest.raises(ValueError):
            export._check_simplify(kw.get("simplify_cell_voxels"), kw.get("simplify_faces"))
    export._check_simplify(None, None), export._check_simplify(2.0, None), export._check_simplify(None, 1)


# ---- the restatement on the sphere and the torus -------------------------------------------------------------------------------------
_meshes = {}


def _mesh(name):
    if name not in _meshes:
        _meshes[name] = S.volume_mesh(name, 24, 3)
    return _meshes[name]


def _identity_holds(rows, faces, r) -> bool:
    """Every vertex its own cluster: rows bit-equal (positions, colours, labels, abundances), faces equal up to the renumbering."""
    c = r["cluster"]
    return bool(len(r["rows"]) == len(rows) and (c >= 0).all() and np.array_equal(r["rows"][c], rows)
                and np.array_equal(r["faces"], c[faces]) and len(np.unique(c)) == len(rows))


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_identity_below_the_smallest_vertex_spacing(name):
    """e = h 2^-12: every cluster is one vertex, and a one-vertex cluster returns its vertex bit for bit (every incident plane passes
    through it and the mean is it; the clamp box is widened to the members).  Condition of the systems: 3001.0 at worst."""
    rows, faces, lo, h = _mesh(name)
    r = S.simplify(rows, faces, 3, lo, np.float32(2.0 ** -12) * h)
    assert _identity_holds(rows, faces, r)
    assert np.array_equal(r["positions"].view(np.uint32), S.positions_of(rows)[np.argsort(r["cluster"], kind="stable")].view(np.uint32))
    assert r["M_max"] == 1 and r["tr0"] == 0 and 2000.0 < r["cond"] <= S.COND_MAX * (1 + 1e-9)
    assert S.count(rows, faces, 3, lo, np.float32(2.0 ** -12) * h) == len(faces)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_one_voxel_cells_keep_the_surface_closed_and_the_volume(name):
    """e = h.  Values of the committed restatement (vertices / faces / enclosed volume), input sphere 2,678 / 5,352 / 0.8953, torus
    3,038 / 6,076 / 0.5605:
      origin = the lattice's lo:             sphere 839 / 1,674 / 0.8930;  torus 976 / 1,960 / 0.5592  (the issue's prototype)
      origin = lo - e / 2 (the export's):    sphere 692 / 1,380 / 0.8952;  torus 743 / 1,486 / 0.5604
    The volume stays within 1 % at both origins.  Closed and consistently oriented holds at the export's origin on both and at lo on
    the sphere; at lo the torus has a pinch -- an edge of four triangles -- which vertex clustering does not exclude."""
    rows, faces, lo, h = _mesh(name)
    v0 = M.volume_area(S.positions_of(rows), faces)[0]
    want = {("sphere", 0): (839, 1674), ("sphere", 1): (692, 1380), ("torus", 0): (976, 1960), ("torus", 1): (743, 1486)}
    for shifted, origin in enumerate((lo, S.rung_origin(lo, h))):
        r = S.simplify(rows, faces, 3, origin, h)
        v1 = M.volume_area(r["positions"], r["faces"])[0]
        print(f"{name} origin {'lo - e/2' if shifted else 'lo'}: {len(r['rows'])} vertices, {len(r['faces'])} faces, volume {v0:.4f} -> {v1:.4f}, "
              f"condition {r['cond']:.1f}")
        assert (len(r["rows"]), len(r["faces"])) == want[name, shifted]
        assert abs(v1 - v0) <= 0.01 * v0
        assert r["cond"] <= S.COND_MAX * (1 + 1e-9)
        assert np.array_equal(np.unique(r["faces"]), np.arange(len(r["rows"])))  # no unreferenced vertex
        if shifted or name == "sphere":
            assert M.closed_and_oriented(r["faces"], len(r["rows"]))
        assert (np.abs(r["pos64"] - r["positions"]) <= r["pos_bound"]).all()  # (the restatement within its own bound: the rounding)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_one_cell_over_everything_leaves_nothing(name):
    rows, faces, lo, h = _mesh(name)
    r = S.simplify(rows, faces, 3, lo, np.float32(64) * h)
    assert r["dims"] == (1, 1, 1) and r["rows"].shape == (0, S.row_bytes(3)) and r["faces"].shape == (0, 3) and (r["cluster"] == -1).all()


def test_the_hand_made_mesh_exercises_every_rule():
    rows, faces, g, e = S.hand_mesh(3)
    r = S.simplify(rows, faces, 3, g, e)
    kept = r["faces"].tolist()
    assert len(faces) == 24 and len(kept) == 13 and r["tr0"] == 3
    assert kept[0] == [0, 1, 5] and kept[1] == [0, 5, 1]  # the first of the duplicates and the opposite twin; the rotated one is gone
    assert [2, 3, 4] in kept and [4, 3, 2] in kept  # the two zero-area faces
    assert r["cluster"][11] == -1 and r["cluster"][12] == -1 and (np.delete(r["cluster"], [11, 12]) >= 0).all()
    label = np.ascontiguousarray(r["rows"][:, 15:19]).view("<i4").ravel()
    assert label[0] == 1 and label[1] == 0 and label[5] == -1  # ties to the smallest; C + 5 clamps to C - 1, -7 to -1
    assert r["rows"][0, 12:15].tolist() == [255, 1, 2]  # (255 + 254 -> 255, 0 + 1 -> 1, 1 + 2 -> 2: halves round up)
    # tr A = 0: the mean of the (single) member
    for v in (13, 14, 15):
        assert np.array_equal(r["positions"][r["cluster"][v]], S.positions_of(rows)[v])


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def test_the_ladder_is_float32_and_ends_at_the_single_cell():
    from umhsnerf import export
    from umhsnerf.ops.export import simplify_grid_dims

    lo, h, dims = M.cube_lattice(24)
    lo_t, h_f = tuple(float(v) for v in lo), float(h)
    rungs = export.simplify_ladder(lo_t, h_f, dims)
    assert all(e == float(np.float32(e)) for e in rungs)
    assert rungs == [float(S.ladder_edge(h, k)) for k in range(1, len(rungs) + 1)]
    assert rungs[3] == float(np.float32(2.0) * h) and rungs[7] == float(np.float32(4.0) * h)  # k = 4, 8: exact powers of two
    far = [float(np.float32(l) + np.float32(d - 1) * h) for l, d in zip(lo, dims)]
    cells = [simplify_grid_dims(far, export.simplify_origin(lo_t, e), e) for e in rungs]
    assert cells[-1] == (1, 1, 1) and all(c != (1, 1, 1) for c in cells[:-1])
    assert 23.0 <= rungs[-1] / h_f <= 2 * 23.0 * 2 ** 0.25  # the first edge that holds 23 voxels and the half-cell shift
    assert export.simplify_origin(lo_t, rungs[0]) == tuple(float(v) for v in S.rung_origin(lo, rungs[0]))
    assert export.simplify_edge(h_f, 2.5) == float(np.float32(2.5) * h)
    for bad in ((0.0, (1 << 31) * 1.0), (0.0, -1.0), (np.nan, 1.0)):
        with pytest.raises(ValueError):
            simplify_grid_dims((1.0, bad[0], 1.0), (0.0, 0.0, 0.0), 1.0 / bad[1] if bad[1] > 0 else bad[1])
    with pytest.raises(ValueError):  # 2^62 cells or more
        simplify_grid_dims((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 2.0 ** -21)
    assert simplify_grid_dims((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 2.0 ** -20) == ((1 << 20) + 1,) * 3
    assert simplify_grid_dims((-np.inf,) * 3, (0.0, 0.0, 0.0), 1.0) == (1, 1, 1) and simplify_grid_dims((-5.0, 0.5, 2.0), (0, 0, 0), 1.0) == (1, 1, 3)


@pytest.mark.parametrize("target", [1, 7, 100, 999])
def test_bisection_on_a_stubbed_count(target):
    from umhsnerf import export

    mono = lambda k: 1000 // k if k < 40 else 0
    bumpy = {k: mono(k) for k in range(1, 41)}
    bumpy.update({5: 3, 6: 900, 11: 0, 12: 500, 20: 2, 21: 300})  # not monotone
    for table in (mono, bumpy.__getitem__):
        calls = []
        k, probes, seen = export.simplify_search(lambda j: (calls.append(j), table(j))[1], 40, target)
        assert probes == len(calls) == len(set(calls)) == len(seen) <= 7  # ceil(log2(40)) + 1: every rung probed at most once
        assert seen[k] == table(k) <= target and (k == 1 or (k - 1 in seen and seen[k - 1] > target))
        assert not any(c <= target and (j == 1 or seen.get(j - 1, -1) > target) for j, c in seen.items() if j < k)
        if table is mono:
            assert k == min(j for j in range(1, 41) if mono(j) <= target)
    with pytest.raises(RuntimeError):
        export.simplify_search(lambda j: 5, 40, 4)


def test_the_search_on_the_restatement_honours_the_target():
    """The ladder and the bisection against the restatement's counts on the sphere: faces <= N, and the rung before leaves more."""
    from umhsnerf import export

    rows, faces, lo, h = _mesh("sphere")
    lo_t = tuple(float(v) for v in lo)
    rungs = export.simplify_ladder(lo_t, float(h), (24, 24, 24))
    cnt = lambda k: S.count(rows, faces, 3, export.simplify_origin(lo_t, rungs[k - 1]), rungs[k - 1])
    for N in (len(faces) - 1, 500, 1):
        k, probes, seen = export.simplify_search(cnt, len(rungs), N)
        assert seen[k] <= N and (k == 1 or cnt(k - 1) > N) and probes <= 7
    assert cnt(len(rungs)) == 0


# ---- planted faults ------------------------------------------------------------------------------------------------------------------
def _assertions_of_this_file(fault):
    """The assertions above that a fault can touch, as one list of booleans."""
    rows, faces, lo, h = _mesh("sphere")
    ident = S.simplify(rows, faces, 3, lo, np.float32(2.0 ** -12) * h, fault=fault)
    hr, hf, g, e = S.hand_mesh(3)
    hand = S.simplify(hr, hf, 3, g, e, fault=fault)
    label = np.ascontiguousarray(hand["rows"][:, 15:19]).view("<i4").ravel()
    return [_identity_holds(rows, faces, ident), ident["cond"] <= S.COND_MAX * (1 + 1e-9), len(hand["faces"]) == 13,
            bool(label[0] == 1 and label[1] == 0)]


def test_each_planted_fault_is_noticed():
    assert all(_assertions_of_this_file(None))
    for fault in S.FAULTS:
        assert not all(_assertions_of_this_file(fault)), fault
