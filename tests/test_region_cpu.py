"""Regional material edits without a GPU: the parser of the ``"regions"`` key, the float32 membership replay against float64, and
the comparators of tests/region_f64.py on the float32 oracle and on planted faults (K is re-measured here)."""
import math

import numpy as np
import pytest
import torch

import region_f64 as RF
from umhsnerf.materials import MAX_REGIONS, MaterialEdits, RegionEdit, load_material_edits

C, B = 3, 8
BOX = {"center": [0.1, 0.0, -0.2], "rotation": [0.3, -0.2, 0.5], "scale": [1.0, 0.5, 2.0]}
SPHERE = {"center": [0.0, 0.25, 0.0], "radius": 0.75}


def _load(doc, specular=True):
    return load_material_edits(doc, C, B, specular)


# ------------------------------------------------------------------------------------------------------------------------------ #
# the parser
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_a_file_with_regions_loads():
    doc = {"materials": [{"material": 0, "gain": 0.5}],
           "regions": [{"box": BOX, "materials": [{"material": 1, "density": 0.0}]},
                       {"sphere": SPHERE, "materials": [{"material": 2, "spectrum": [0.5] * B}], "specular_gain": 0.25}]}
    e = _load(doc)
    assert len(e.regions) == 2 and all(isinstance(r, RegionEdit) for r in e.regions)
    box, sph = e.regions
    assert box.kind == "box" and box.scale == (1.0, 0.5, 2.0) and box.edit.densities == (1.0, 0.0, 1.0) and box.edit.gains == (1.0,) * 3
    assert sph.kind == "sphere" and sph.radius == 0.75 and sph.edit.specular_gain == 0.25 and sph.edit.spectra[2] == (0.5,) * B
    assert e.gains == (0.5, 1.0, 1.0) and e.edits_density and e.edits_dictionary and not e.is_identity
    # a region REPLACES the top level: its layers carry nothing of it
    assert [l.gains for l in e.layers] == [(0.5, 1.0, 1.0), (1.0,) * 3, (1.0,) * 3] and all(not l.regions for l in e.layers)
    table = e.region_table()
    assert table.shape == (2, 16) and table.dtype == np.float32
    assert np.array_equal(table[0], RF.box_record(BOX["center"], BOX["rotation"], BOX["scale"]))
    assert np.array_equal(table[1], RF.sphere_record(SPHERE["center"], SPHERE["radius"]))
    E = torch.rand(C, B)
    D = e.dictionaries(E)
    assert tuple(D.shape) == (3, C, B) and torch.equal(D[0], e.dictionary(E)) and torch.equal(D[1], E) and torch.equal(D[2][2], torch.full((B,), 0.5))
    assert torch.equal(e.density_gains("cpu"), torch.tensor([[1.0, 1, 1], [1, 0, 1], [1, 1, 1]]))
    assert torch.equal(e.specular_gains("cpu"), torch.tensor([1.0, 1.0, 0.25]))


def test_the_properties_look_through_the_regions():
    top_identity = _load({"regions": [{"box": BOX, "materials": [{"material": 1, "density": 0.0}]}]})
    assert top_identity.edits_density and not top_identity.edits_dictionary and not top_identity.is_identity
    recolour = _load({"regions": [{"sphere": SPHERE, "materials": [{"material": 1, "from_material": 0}]}]})
    assert recolour.edits_dictionary and not recolour.edits_density and not recolour.is_identity
    nothing = _load({"regions": [{"sphere": SPHERE}, {"box": BOX, "materials": [{"material": 0, "gain": 1.0}]}]})
    assert nothing.is_identity and len(nothing.regions) == 2
    assert _load({"regions": []}).regions == () and _load({}).regions == ()
    # the positional constructor and the default stay
    plain = MaterialEdits(C, B, False, (None,) * C, (1.0,) * C, (1.0,) * C, 1.0)
    assert plain.regions == () and plain.layers == (plain,)
    eight = _load({"regions": [{"sphere": SPHERE}] * MAX_REGIONS})
    assert len(eight.regions) == 8


REFUSED = [
    ({"regions": [{"sphere": SPHERE}] * 9}, r"9 regions, at most 8"),
    ({"regions": {"box": BOX}}, r"\"regions\" must be a list"),
    ({"regions": [{"box": BOX, "sphere": SPHERE}]}, r"region 1: .*either.*both"),
    ({"regions": [{"sphere": SPHERE}, {"materials": []}]}, r"region 2: .*either.*neither"),
    ({"regions": [{"box": BOX, "colour": 1}]}, r"region 1: unknown keys \['colour'\]"),
    ({"regions": [{"box": dict(BOX, size=1)}]}, r"region 1: unknown keys \['size'\]"),
    ({"regions": [{"sphere": {"center": [0, 0, 0]}}]}, r"region 1: the sphere lacks \['radius'\]"),
    ({"regions": [{"box": dict(BOX, scale=[1.0, 0.0, 1.0])}]}, r"region 1: scale 0.0 must be > 0"),
    ({"regions": [{"box": dict(BOX, scale=[1.0, -2.0, 1.0])}]}, r"region 1: scale -2.0 must be > 0"),
    ({"regions": [{"sphere": SPHERE}, {"sphere": dict(SPHERE, radius=0)}]}, r"region 2: radius 0 must be > 0"),
    ({"regions": [{"sphere": dict(SPHERE, radius=-1.0)}]}, r"region 1: radius -1.0 must be > 0"),
    ({"regions": [{"sphere": dict(SPHERE, radius=math.inf)}]}, r"region 1: radius inf must be a finite number"),
    ({"regions": [{"sphere": dict(SPHERE, center=[0.0, math.nan, 0.0])}]}, r"region 1: center nan must be a finite number"),
    ({"regions": [{"box": dict(BOX, rotation=[0.0, math.inf, 0.0])}]}, r"region 1: rotation inf must be a finite number"),
    ({"regions": [{"box": dict(BOX, scale=[1.0, 1.0])}]}, r"region 1: scale must be a list of 3 numbers"),
    ({"regions": [{"sphere": dict(SPHERE, radius=1e-60)}]}, r"region 1: radius 1e-60 must be > 0 and finite in float32"),
    ({"regions": ["box"]}, r"region 1 must be an object"),
    # what the per-entry checks refuse, with the region named
    ({"regions": [{"sphere": SPHERE, "materials": [{"material": 3, "gain": 2.0}]}]}, r"region 1: entry 0: material 3 is outside 0\.\.2"),
    ({"regions": [{"sphere": SPHERE, "materials": [{"material": 1, "gain": -1.0}]}]}, r"region 1: entry 0 \(material 1\): gain -1.0 must be"),
    ({"regions": [{"sphere": SPHERE, "materials": [{"material": 1}, {"material": 1}]}]}, r"region 1: entry 1 \(material 1\): material 1 is listed twice"),
    ({"regions": [{"sphere": SPHERE, "materials": [{"material": 1, "spectrum": [0.5] * 7}]}]}, r"region 1: entry 0 \(material 1\): the spectrum has 7"),
    ({"regions": [{"sphere": SPHERE, "materials": [{"material": 1, "tint": 1}]}]}, r"region 1: entry 0: unknown keys \['tint'\]"),
    ({"regions": [{"sphere": SPHERE, "specular_gain": -0.5}]}, r"region 1: specular_gain -0.5 must be"),
    ({"regions": [{"sphere": SPHERE, "materials": {}}]}, r"region 1: \"materials\" must be a list"),
]


@pytest.mark.parametrize("doc,words", REFUSED, ids=[w[:40] for _, w in REFUSED])
def test_refusals_name_the_region_and_the_reason(doc, words):
    with pytest.raises(ValueError, match=words):
        _load(doc)


def test_a_region_specular_gain_needs_the_specular_head_and_the_old_texts_stay():
    with pytest.raises(ValueError, match=r"region 1: specular_gain 0.5 needs a model with the specular head"):
        _load({"regions": [{"sphere": SPHERE, "specular_gain": 0.5}]}, specular=False)
    with pytest.raises(ValueError, match=r"material edits: entry 0: material 3 is outside 0\.\.2"):
        _load({"materials": [{"material": 3}]})
    with pytest.raises(ValueError, match=r"unknown keys \['zones'\] in the file"):
        _load({"zones": []})
    with pytest.raises(ValueError, match="at most 8"):
        MaterialEdits(C, B, False, (None,) * C, (1.0,) * C, (1.0,) * C, 1.0, (_load({"regions": [{"sphere": SPHERE}]}, False).regions[0],) * 9)


# ------------------------------------------------------------------------------------------------------------------------------ #
# membership
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("K", [1, 3, 8])
def test_the_float32_replay_agrees_with_float64_away_from_the_faces(K):
    table = RF.make_table(K)
    p = np.random.default_rng(K).uniform(-1.5, 1.5, (20000, 3)).astype(np.float32)
    got = RF.classify32(p, table)
    want, dist = RF.classify64(p, table)
    far = dist > RF.MARGIN
    assert far.mean() > 0.99 and np.array_equal(got[far], want[far])
    assert set(np.unique(got)) >= set(range(min(K, 2) + 1))  # outside, and the first regions, all occur
    if K > 1:  # overlap: points inside two regions carry the first
        inside = np.stack([RF._inside32(p, rec) for rec in table])
        both = inside.sum(0) > 1
        assert both.sum() > 10 and (got[both] == inside[:, both].argmax(0) + 1).all()


def test_points_on_a_face_are_outside_and_nan_is_in_no_region():
    table = RF.DYADIC_TABLE[:2]
    planted = RF.on_face_points(table)
    assert len(planted) == 9
    assert (RF.classify32(planted, table) == 0).all()
    assert (RF.classify32(planted, RF.DYADIC_TABLE) == 3).all()  # the big box behind them takes what the faces refuse
    inward = planted + np.sign(np.stack([table[0, 0:3]] * 6 + [table[1, 0:3]] * 3) - planted).astype(np.float32) * np.float32(2.0 ** -10)
    assert (RF.classify32(inward, table) > 0).all()
    bad = np.array([[np.nan, 0, 0], [0, np.nan, 0], [np.nan] * 3, [np.inf, 0, 0], [-np.inf, np.inf, 0]], np.float32)
    assert (RF.classify32(bad, RF.DYADIC_TABLE) == 0).all()
    p = RF.make_points(1000, RF.DYADIC_TABLE)
    ids = RF.classify32(p, RF.DYADIC_TABLE)
    assert np.isnan(p).any() and (ids[np.isnan(p).any(1)] == 0).all() and len(np.unique(ids)) == 4


# ------------------------------------------------------------------------------------------------------------------------------ #
# segments
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_the_segment_builder():
    region = np.array([1, 1, 0, 0, 0, 2, 2, 2, 2], np.uint8)
    ray = np.array([1, 1, 1, 3, 3, 3, 3, 4, 4], np.int64)
    pinfo = np.array([[0, 0], [0, 3], [3, 0], [3, 4], [7, 2], [9, 0]], np.int64)
    s = RF.build_segments(region, ray, pinfo)
    assert s["S"] == 5 and s["seg_of"].tolist() == [0, 0, 1, 2, 2, 3, 3, 4, 4]
    assert s["seg_info"].tolist() == [[0, 2], [2, 1], [3, 2], [5, 2], [7, 2]] and s["seg_layer"].tolist() == [1, 0, 0, 2, 2]
    assert s["ray_seg"].tolist() == [[0, 0], [0, 2], [2, 0], [2, 2], [4, 1], [5, 0]]
    for n in (0, 1, 257, 4099):
        for pattern in ("alternate", "single", "runs"):
            counts = RF.ray_counts(n)
            region, ray, pinfo = RF.make_stream(counts, pattern)
            s = RF.build_segments(region, ray, pinfo)
            assert s["seg_info"][:, 1].sum() == n and (s["seg_info"][:, 1] > 0).all() and s["ray_seg"][:, 1].sum() == s["S"]
            if pattern == "alternate":
                assert s["S"] == n
            if pattern == "single":
                assert s["S"] == (counts > 0).sum()


# ------------------------------------------------------------------------------------------------------------------------------ #
# comparators
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_k_is_measured_here_and_four_times_the_worst_fits():
    worst = RF.measure_worst()
    print({k: round(v, 3) for k, v in worst.items()})
    assert 4 * max(worst["spectral"], worst["spectral2"], worst["specular"]) <= RF.K_REMIX
    assert 4 * worst["segment_sum"] <= RF.K_SEGSUM and 4 * worst["sigma"] <= RF.K_SIGMA
    assert min(RF.K_REMIX, RF.K_SEGSUM, RF.K_SIGMA) >= 8 and all(math.log2(k).is_integer() for k in (RF.K_REMIX, RF.K_SEGSUM, RF.K_SIGMA))
    # no looser than the rule asks: half of each K would not cover 4 x worst (or K is at its floor)
    assert RF.K_REMIX / 2 < 4 * max(worst["spectral"], worst["spectral2"], worst["specular"]) or RF.K_REMIX == 8
    assert RF.K_SEGSUM / 2 < 4 * worst["segment_sum"] or RF.K_SEGSUM == 8
    assert RF.K_SIGMA / 2 < 4 * worst["sigma"] or RF.K_SIGMA == 8


@pytest.mark.parametrize("c", RF.REGION_CASES, ids=RF.region_case_id)
def test_the_remix_comparator_passes_float32_has_teeth_and_rejects_planted_faults(c):
    case, report = RF.make_region_case(*c), {}
    r64 = RF.remix_regions_oracle(case, torch.float64)
    assert not RF.check_remix_regions(case, RF.remix_regions_oracle(case, torch.float32), r64, report)
    assert not RF.teeth_failures(report), report
    if case["S"] == 0:
        return
    multi = torch.nonzero(case["ray_seg"][:, 1] > 1).reshape(-1)
    # a swapped layer: one segment mixed with another layer's dictionary
    j = int(case["ray_seg"][multi[0], 0]) if len(multi) else 0
    layer = case["seg_layer"].clone()
    layer[j] = (layer[j] + 1) % (case["K"] + 1)
    assert RF.check_remix_regions(case, RF.remix_regions_oracle(case, torch.float32, seg_layer=layer), r64)
    if len(multi):
        r = int(multi[0])
        dropped = case["ray_seg"].clone()
        dropped[r, 1] -= 1  # a dropped segment: the ray's last
        assert RF.check_remix_regions(case, RF.remix_regions_oracle(case, torch.float32, ray_seg=dropped), r64)
        shifted = case["ray_seg"].clone()
        shifted[r, 0] += 1  # a wrong summation partner: the ray takes its neighbour's first segment for its own first
        if int(shifted[r, 0] + shifted[r, 1]) <= case["S"]:
            assert RF.check_remix_regions(case, RF.remix_regions_oracle(case, torch.float32, ray_seg=shifted), r64)


@pytest.mark.parametrize("c", RF.SEGSUM_CASES, ids=[f"R{c[0]}-k{c[1]}" for c in RF.SEGSUM_CASES])
def test_the_segment_sum_comparator_passes_float32_and_rejects_planted_faults(c):
    case, report = RF.make_segsum_case(*c), {}
    r64 = RF.segsum_oracle(case, torch.float64)
    assert not RF.check_segsum(case, RF.segsum_oracle(case, torch.float32), r64, report)
    assert not RF.teeth_failures(report), report
    multi = torch.nonzero(case["ray_seg"][:, 1] > 1).reshape(-1)
    if len(multi):
        r = int(multi[0])
        dropped = case["ray_seg"].clone()
        dropped[r, 1] -= 1
        assert RF.check_segsum(case, RF.segsum_oracle(case, torch.float32, ray_seg=dropped), r64)
        shifted = case["ray_seg"].clone()
        shifted[r, 0] += 1
        if int(shifted[r, 0] + shifted[r, 1]) <= case["S"]:
            assert RF.check_segsum(case, RF.segsum_oracle(case, torch.float32, ray_seg=shifted), r64)


@pytest.mark.parametrize("c", RF.SIGMA_CASES, ids=[f"n{c[0]}-C{c[1]}-K{c[2]}" for c in RF.SIGMA_CASES])
def test_the_sigma_comparator_passes_float32_and_rejects_a_swapped_layer(c):
    case, report = RF.make_sigma_regions_case(*c), {}
    r64 = RF.sigma_regions_oracle(case, torch.float64)
    assert not RF.check_sigma_regions(case, RF.sigma_regions_oracle(case, torch.float32), r64, report)
    assert not RF.teeth_failures(report), report
    if case["n"] >= 63:
        swapped = (case["region"].long() + 1) % (case["K"] + 1)  # every sample takes its neighbour layer's gains
        assert RF.check_sigma_regions(case, RF.sigma_regions_oracle(case, torch.float32, layer_of=swapped), r64)
