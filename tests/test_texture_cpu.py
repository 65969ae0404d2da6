"""Textured mesh export without a GPU: the atlas layout's properties on tests/texture_ref.py (and that the reference catches planted
faults), the OBJ / MTL writers, the ``textured-mesh`` parser, and the argument checks of the C entries on the built library."""
import numpy as np
import pytest

import texture_ref as R

FACES, PX = (1, 2, 3, 7, 8, 9, 50), (4, 5, 8)
GRID = [(F, p) for F in FACES for p in PX]


# ---- layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,p", GRID)
def test_atlas_sizes_are_as_defined(F, p):
    Q, T = R.atlas(F, p)
    S = (F + 1) // 2
    assert Q * Q >= S and (Q - 1) * (Q - 1) < S and T == Q * p


@pytest.mark.parametrize("F,p", GRID)
def test_every_texel_has_at_most_one_owner(F, p):
    R.check_single_owner(F, p)
    own = R.owner_map(F, p)
    Q, T = R.atlas(F, p)
    i, j = np.arange(T)[None, :] % p, np.arange(T)[:, None] % p
    used = own >= 0
    assert ((own[used] % 2 == 0) == ((i + j) <= p - 1)[used]).all()  # the even face owns i + j <= p - 1, the odd face the rest
    assert int(used.sum()) == (F // 2) * p * p + (F % 2) * p * (p + 1) // 2


@pytest.mark.parametrize("F,p", GRID)
def test_corners_are_owned_texel_centres(F, p):
    R.check_corners(F, p)


@pytest.mark.parametrize("F,p", GRID)
def test_bilinear_footprints_stay_inside_the_face(F, p):
    R.check_bilinear(F, p)


@pytest.mark.parametrize("F,p", GRID)
def test_vt_equal_the_stated_divisions(F, p):
    """Independent of ``texture_ref.uv``: the quotient of the exact integers in float64, rounded once to float32 (a float64 quotient of
    two integers below 2^24 rounds to float32 as the exact quotient does: double rounding cannot bite at 53 >= 2 * 24 + 2 bits)."""
    Q, T = R.atlas(F, p)
    got = R.uv(F, p)
    assert got.dtype == np.float32 and got.shape == (F, 3, 2)
    e = p - 3
    for f in range(F):
        sx, sy = (f // 2) % Q, (f // 2) // Q
        cs = [(p - 1, p - 1), (2, p - 1), (p - 1, 2)] if f % 2 else [(0, 0), (e, 0), (0, e)]
        for c, (ic, jc) in enumerate(cs):
            u = np.float32((2 * (sx * p + ic) + 1) / (2 * T))
            v = np.float32((2 * (T - (sy * p + jc)) - 1) / (2 * T))
            assert got[f, c, 0].view(np.uint32) == u.view(np.uint32) and got[f, c, 1].view(np.uint32) == v.view(np.uint32)
            # a viewer's sample at the corner is the centre of the owned texel (col, row), row 0 on top
            assert u * T - 0.5 == pytest.approx(sx * p + ic, abs=1e-3) and (1 - v) * T - 0.5 == pytest.approx(sy * p + jc, abs=1e-3)


@pytest.mark.parametrize("p", PX)
def test_the_reference_catches_planted_faults(p):
    with pytest.raises(AssertionError):
        R.check_bilinear(8, p, inset=2)  # a 2-texel inset lets a footprint reach the other face
    with pytest.raises(AssertionError):
        R.check_corners(8, p, swap=True)  # the faces of a square owning each other's texels
    R.check_corners(8, p, inset=2)  # (the inset alone leaves the corners owned: it is the bilinear property that needs 3)


# ---- writers -----------------------------------------------------------------------------------------------------------------------
def test_a_tetrahedron_round_trips_through_the_writers(tmp_path):
    from umhsnerf import export

    pos, faces = R.tetrahedron()
    pos = pos.copy()
    pos[0] = [np.float32(1) / np.float32(3), np.float32(1e-7), np.float32(-123456.789)]  # values that need all 9 digits
    uv = R.uv(4, 4)
    export.write_textured_obj(tmp_path / export.OBJ_NAME, pos, uv, faces)
    export.write_mtl(tmp_path / export.MTL_NAME, "material_0.png")
    obj = R.read_textured_obj(tmp_path / "mesh.obj")
    assert obj["mtllib"] == "material_0.mtl" and obj["usemtl"] == "material_0"
    assert np.array_equal(obj["v"].view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(obj["vt"].view(np.uint32), uv.reshape(-1, 2).view(np.uint32))
    assert np.array_equal(obj["f"], faces) and np.array_equal(obj["ft"], np.arange(12).reshape(4, 3))
    floats = np.concatenate([pos.reshape(-1), uv.reshape(-1)])
    assert obj["tokens"] == ["%.9g" % float(x) for x in floats]
    assert R.read_mtl(tmp_path / "material_0.mtl") == {"newmtl": "material_0", "map_Kd": "material_0.png"}
    lines = (tmp_path / "mesh.obj").read_text().splitlines()
    assert lines[:2] == ["mtllib material_0.mtl", "usemtl material_0"] and [ln.split()[0] for ln in lines[2:]] == ["v"] * 4 + ["vt"] * 12 + ["f"] * 4
    assert lines[-1] == "f 2/10 3/11 4/12"
    with pytest.raises(ValueError):
        export.write_textured_obj(tmp_path / "bad.obj", pos, uv[:3], faces)
    assert export.texture_file_names(["rgb", "seg_pred"]) == {"rgb": "material_0.png", "seg_pred": "texture_seg_pred.png"}
    with pytest.raises(ValueError):
        export.texture_file_names([])
    assert export.texture_bands(10, 25) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)] and export.texture_bands(7, 3) == [(r, r + 1) for r in range(7)]
    assert all((b - a) * 4000 <= 1 << 20 for a, b in export.texture_bands(4000)) and export.texture_bands(4000)[-1][1] == 4000


# ---- parser ------------------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_refusals(capsys):
    from umhsnerf import export

    base = ["--data", "scene", "--checkpoint", "step.ckpt", "--output-dir", "out"]
    a = export.parse_args(["textured-mesh", *base])
    t = export.parse_args(["tsdf", *base])
    assert a.command == "textured-mesh" and a.px_per_uv_triangle == 4 and a.ray_length is None
    assert a.texture_output_names == ["rgb"] and a.cube_output_names == []
    own = {"command", "px_per_uv_triangle", "ray_length", "texture_output_names", "cube_output_names", "texture_method", "unwrap_method"}
    assert {k: v for k, v in vars(a).items() if k not in own} == {k: v for k, v in vars(t).items() if k not in own}  # tsdf's flags, tsdf's defaults
    assert not hasattr(a, "material_edits")
    a = export.parse_args(["textured-mesh", *base, "--px-per-uv-triangle", "8", "--ray-length", "0.05", "--texture-output-names", "rgb", "seg_pred",
                           "--cube-output-names", "abundances", "--material", "1", "--material-edits", "edits.json", "--save-world-frame"])
    assert (a.px_per_uv_triangle, a.ray_length, a.texture_output_names, a.cube_output_names) == (8, 0.05, ["rgb", "seg_pred"], ["abundances"])
    assert a.material == 1 and a.material_edits == "edits.json" and a.save_world_frame is True
    for bad, word in ((["--px-per-uv-triangle", "3"], "at least 4"), (["--px-per-uv-triangle", "16385"], "16384"),
                      (["--target-num-faces", "50000"], "decimator"), (["--ray-length", "0"], "positive"),
                      (["--ray-length", "inf"], "positive"), (["--num-pixels-per-side", "2048"], "--px-per-uv-triangle"),
                      (["--resolution", "64", "32"], "one integer or three")):
        with pytest.raises(SystemExit):
            export.parse_args(["textured-mesh", *base, *bad])
        assert word in capsys.readouterr().err, bad
    for bad in (["--texture-method", "nerf"], ["--unwrap-method", "custom"], ["--px-per-uv-triangle", "4"]):  # tsdf still refuses
        with pytest.raises(SystemExit):
            export.parse_args(["tsdf", *base, *bad])
        err = capsys.readouterr().err
        assert "unwrap" in err and "textured-mesh" in err


def test_an_atlas_above_the_limit_is_refused_with_a_message(built_library):
    """``ops.texture_atlas`` is umhs_texture_atlas (host arithmetic): what the export calls before anything is rendered."""
    from umhsnerf import ops

    for F, p in GRID:
        assert ops.texture_atlas(F, p) == R.atlas(F, p)
    assert ops.texture_atlas(2 * 4096 * 4096, 4) == (4096, 16384)
    with pytest.raises(ValueError, match="--resolution.*--px-per-uv-triangle"):
        ops.texture_atlas(2 * 4096 * 4096 + 1, 4)
    with pytest.raises(ValueError, match="--resolution"):
        ops.texture_atlas(2_000_000, 17)
    with pytest.raises(ValueError, match="at least 4"):
        ops.texture_atlas(10, 3)
    with pytest.raises(ValueError):
        ops.texture_atlas(0, 4)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_texture_entries_come_before_any_launch(built_library):
    import ctypes

    from umhsnerf import _hip

    lib = _hip.lib()
    OK, ARG, UNSUP = 0, -1, -2
    for name in ("umhs_texture_atlas", "umhs_texture_uv", "umhs_texture_rays"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.umhs_abi_version() == 11 == _hip.ABI_VERSION
    Q, T = ctypes.c_int32(-7), ctypes.c_int32(-7)
    atlas = lambda F, p: lib.umhs_texture_atlas(F, p, ctypes.byref(Q), ctypes.byref(T))
    for F in (*FACES, 2_000_000, 2 * 4096 * 4096):
        for p in ((4,) if F > 2_000_000 else PX):
            assert atlas(F, p) == OK and (Q.value, T.value) == R.atlas(F, p), (F, p)
    assert R.atlas(2_000_000, 4) == (1000, 4000)
    Q.value = T.value = -7
    for F, p, code in ((10, 3, ARG), (0, 4, ARG), (-1, 4, ARG), (10, -4, ARG), (2 * 4096 * 4096 + 1, 4, UNSUP), (2_000_000, 17, UNSUP),
                       (1, 16385, UNSUP), (1 << 62, 4, UNSUP)):
        assert atlas(F, p) == code, (F, p)
        assert (Q.value, T.value) == (-7, -7)  # written only with UMHS_OK
    assert lib.umhs_texture_atlas(10, 4, None, ctypes.byref(T)) == ARG and lib.umhs_texture_atlas(10, 4, ctypes.byref(Q), None) == ARG

    d = 4096  # never dereferenced
    uv = lambda F, p, out=None: lib.umhs_texture_uv(F, p, out, None)
    assert uv(10, 4) == ARG and uv(10, 3, d) == ARG and uv(0, 4, d) == ARG and uv(10, 3) == ARG
    assert uv(2_000_000, 17) == UNSUP and uv(2_000_000, 17, d) == UNSUP

    def rays(F=10, p=4, L=0.1, begin=0, end=0, V=8, ptrs=(None,) * 8):
        pos, fac, o, dd, nr, fr, tf, bary = ptrs
        return lib.umhs_texture_rays(pos, V, fac, F, p, L, begin, end, o, dd, nr, fr, tf, bary, None)

    side = R.atlas(10, 4)[1]
    cases = (dict(p=3), dict(F=0), dict(F=-3), dict(begin=-1), dict(begin=5, end=4), dict(end=side * side + 1),
             dict(begin=side * side + 1, end=side * side + 1), dict(L=0.0), dict(L=-1.0), dict(L=float("inf")), dict(L=float("nan")),
             dict(V=0))
    for kw in cases:  # with NULL device pointers: nothing can have been launched
        assert rays(**kw) == ARG, kw
        assert rays(**kw, ptrs=(d,) * 8) == ARG, kw
    assert rays(F=2_000_000, p=17) == UNSUP and rays(F=2 * 4096 * 4096 + 1) == UNSUP
    assert rays() == ARG  # every pointer NULL
    for k in range(7):  # one required pointer NULL; bary (the eighth) is optional
        assert rays(end=side * side, ptrs=tuple(None if m == k else d for m in range(8))) == ARG, k
    assert rays(ptrs=(d,) * 7 + (None,)) == OK and rays(begin=9, end=9, ptrs=(d,) * 8) == OK  # an empty range launches nothing
    assert rays(begin=side * side, end=side * side, ptrs=(d,) * 8) == OK
