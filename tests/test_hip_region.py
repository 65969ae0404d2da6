"""Regional material edits on the GPU: csrc/umhs_region.hip against tests/region_f64.py (membership and segments bit for bit, the
three arithmetic kernels per element against float64), the assumption the feature rests on (umhs_field_heads_fwd forms its sums per
contiguous run, whatever the run is), the regional render of ``UMHSModel.material_edits_context`` on the small trained scene of
tests/test_hip_material.py, and the command lines."""
import contextlib
import ctypes
import json

import numpy as np
import pytest
import torch

import material_f64 as MF
import region_f64 as RF
from test_hip_material import BASE_FLAGS, H, W, _common, _make_world, _samples, _unmixed_checkpoint  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAR = {"sphere": {"center": [1e6, 1e6, 1e6], "radius": 1.0}}  # a region that no sample meets
EVERYWHERE = {"box": {"center": [0.0, 0.0, 0.0], "rotation": [0.0, 0.0, 0.0], "scale": [1e30, 1e30, 1e30]}}
HALF_BOX = {"center": [0.0, 0.0, 0.0], "rotation": [0.0, 0.0, 0.0], "scale": [1.0, 1.0, 1.0]}
SPHERE = {"center": [0.0, 0.0, 0.0], "radius": 0.5}


def _dev(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------ #
# classify, segments
# ------------------------------------------------------------------------------------------------------------------------------ #
def _table(K):
    if K == 1:
        return RF.make_table(1)  # one rotated box
    if K == 3:
        return RF.DYADIC_TABLE  # faces that the float32 arithmetic meets exactly; the big box behind them
    return np.concatenate([RF.DYADIC_TABLE[:2], RF.make_table(6)])  # dyadic faces, then rotated boxes and spheres that overlap


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 4099])
def test_classify_is_the_replay_bit_for_bit(n, K):
    from umhsnerf import ops

    table = _table(K)
    p = RF.make_points(n, table)
    want = RF.classify32(p, table)
    got = ops.region_classify(_dev(p).contiguous() if n else torch.empty((0, 3), device=DEV), table)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n,)
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    if n >= 1000:
        assert np.isnan(p).any() and (want[np.isnan(p).any(1)] == 0).all()
    if n >= 1000 and K > 1:
        planted = RF.on_face_points(table)
        assert len(planted) >= 9
        assert len(np.unique(want)) >= min(K, 3) + 1  # outside and the first regions all occur
        behind = 3 if K == 3 else None  # (K = 3: the big box takes what the faces in front of it refuse)
        face_ids = want[1:10]  # (the first nine: six on the first box's faces, three at the sphere's radius)
        assert (face_ids != 1).all() and (face_ids[6:9] != 2).all() and (behind is None or (face_ids == behind).all())
    none = ops.region_classify(_dev(p).contiguous() if n else torch.empty((0, 3), device=DEV), np.zeros((0, 16), np.float32))
    assert not bool(none.any())


SEGMENT_NS = [0, 1, 255, 256, 257, 4099, 256 * 1024 + 300]  # the last: more block counts than one round of the scan takes (a carry)


@pytest.mark.parametrize("pattern", ["runs", "alternate", "single"])
@pytest.mark.parametrize("n", SEGMENT_NS)
def test_segments_equal_the_numpy_builder_and_repeat_byte_for_byte(n, pattern):
    from umhsnerf import ops

    counts = RF.ray_counts(n)
    region, ray, pinfo = RF.make_stream(counts, pattern)
    want = RF.build_segments(region, ray, pinfo)
    if n >= 4099:
        assert counts[0] == 0 and counts[-1] == 0 and (counts[2:-2] == 0).any() and (counts == 1).any() and (counts > 256).any()
    if pattern == "alternate":
        assert want["S"] == n
    if pattern == "single":
        assert want["S"] == int((counts > 0).sum())
    if pattern == "runs" and n >= 4099:
        info = want["seg_info"]
        ends = info[:, 0] + info[:, 1] - 1
        assert ((info[:, 0] // 64 != ends // 64).any() and (info[:, 0] // 256 != ends // 256).any())  # runs over wave and block boundaries
    args = (_dev(region), _dev(ray), _dev(pinfo))
    runs = [ops.region_segments(*args) for _ in range(2)]
    seg_of, seg_info, seg_layer, ray_seg, S = runs[0]
    assert S == want["S"] and tuple(seg_info.shape) == (S, 2) and tuple(seg_layer.shape) == (S,)
    assert seg_of.dtype == seg_info.dtype == ray_seg.dtype == torch.int64 and seg_layer.dtype == torch.int32
    if n:
        assert np.array_equal(seg_of.cpu().numpy(), want["seg_of"])
        assert np.array_equal(seg_info.cpu().numpy(), want["seg_info"])
        assert np.array_equal(seg_layer.cpu().numpy(), want["seg_layer"])
    assert np.array_equal(ray_seg.cpu().numpy(), want["ray_seg"])
    assert runs[1][4] == S and all(torch.equal(a, b) for a, b in zip(runs[0][:4], runs[1][:4]))


# ------------------------------------------------------------------------------------------------------------------------------ #
# sigma_regions, segment_sum, remix_regions
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("c", RF.SIGMA_CASES, ids=[f"n{c[0]}-C{c[1]}-K{c[2]}" for c in RF.SIGMA_CASES])
def test_sigma_regions_is_within_the_bound_of_float64(c):
    from umhsnerf import ops

    case = RF.make_sigma_regions_case(*c)
    s, a, r, g = (_dev(case[k]) for k in ("sigma", "a", "region", "gain"))
    got, report = ops.material_sigma_regions(s, a, r, g), {}
    fails = RF.check_sigma_regions(case, got, RF.sigma_regions_oracle(case, torch.float64), report)
    print(c, report)
    assert not fails, fails
    assert not RF.teeth_failures(report), report
    inplace = s.clone()
    assert ops.material_sigma_regions(inplace, a, r, g, out=inplace) is inplace and torch.equal(inplace, got)
    assert torch.equal(ops.material_sigma_regions(s, a, r, torch.ones_like(g)), s)  # all-ones gains: the input, bit for bit
    # one layer everywhere is umhs_material_sigma with that layer's gains, bit for bit
    for k in (0, case["K"]):
        assert torch.equal(ops.material_sigma_regions(s, a, torch.full_like(r, k), g), ops.material_sigma(s, a, g[k].contiguous()))


@pytest.mark.parametrize("c", RF.SEGSUM_CASES, ids=[f"R{c[0]}-k{c[1]}" for c in RF.SEGSUM_CASES])
def test_segment_sum_is_within_the_bound_of_float64(c):
    from umhsnerf import ops

    case, report = RF.make_segsum_case(*c), {}
    got = ops.segment_sum(_dev(case["values"]), _dev(case["ray_seg"]))
    fails = RF.check_segsum(case, got, RF.segsum_oracle(case, torch.float64), report)
    print(c, report)
    assert not fails, fails
    assert not RF.teeth_failures(report), report
    assert torch.equal(got, ops.segment_sum(_dev(case["values"]), _dev(case["ray_seg"])))
    # the order is the definition: the float32 oracle adds the same rows in the same order, so the bits agree
    assert torch.equal(got.cpu(), RF.segsum_oracle(case, torch.float32))


def _run_remix(case):
    from umhsnerf import ops

    outs = ops.material_remix_regions(_dev(case["mix"]), _dev(case["comp_specular"]), _dev(case["seg_layer"]), _dev(case["ray_seg"]),
                                      _dev(case["E"]), _dev(case["s"]))
    return dict(zip(("spectral", "spectral2", "specular"), outs))


@pytest.mark.parametrize("c", RF.REGION_CASES, ids=RF.region_case_id)
def test_remix_regions_is_within_the_bound_of_float64_and_repeats_bit_for_bit(c):
    case = RF.make_region_case(*c)
    got, report = _run_remix(case), {}
    fails = RF.check_remix_regions(case, got, RF.remix_regions_oracle(case, torch.float64), report)
    print(RF.region_case_id(c), {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})
    assert not fails, fails
    assert not RF.teeth_failures(report), report
    assert all(tuple(v.shape) == (c[0], c[1]) and bool(torch.isfinite(v).all()) for v in got.values())  # the NaN columns were not read
    again = _run_remix(case)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_one_segment_per_ray_in_layer_zero_is_the_global_remix_bit_for_bit():
    from umhsnerf import ops

    case = MF.make_remix_case(257, 64, 15, True)
    R = case["R"]
    want = ops.material_remix(_dev(case["mix"]), _dev(case["comp_specular"]), _dev(case["E"]), case["s"])
    ray_seg = torch.stack([torch.arange(R), torch.ones(R, dtype=torch.int64)], 1)
    E_all = torch.stack([case["E"], torch.full_like(case["E"], float("nan"))])  # (layer 1 is never looked at)
    got = ops.material_remix_regions(_dev(case["mix"]), _dev(case["comp_specular"]), torch.zeros(R, dtype=torch.int32, device=DEV),
                                     _dev(ray_seg), _dev(E_all), torch.tensor([case["s"], 9.0], device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("c", [(257, 64, 15, True, 8), (9, 256, 15, True, 8)], ids=RF.region_case_id)
def test_remix_regions_takes_the_same_bits_on_unaligned_rows(c):
    """B % 4 == 0 with a row array off the 16-byte grid takes the one-float form; the second case also has dictionaries beyond what is
    staged in LDS in both forms.  The same chain per element: the same bits."""
    from umhsnerf import _hip

    case = RF.make_region_case(*c)
    want = _run_remix(case)
    R, B, C, K, S = (case[k] for k in ("R", "B", "C", "K", "S"))
    held = [_dev(case[k]) for k in ("mix", "seg_layer", "ray_seg", "E", "s")]  # (held: freed blocks would be reused before the launch)
    pad = lambda rows: torch.zeros(rows * B + 1, device=DEV)[1:].view(rows, B)
    cs = pad(S)
    cs.copy_(case["comp_specular"])
    outs = [pad(R), pad(R), pad(R)]
    assert cs.data_ptr() % 16 == 4 and outs[0].data_ptr() % 16 == 4
    mix, layer, ray_seg, E, s = held
    rc = _hip.lib().umhs_material_remix_regions(_hip.ptr(mix), ctypes.c_void_p(cs.data_ptr()), _hip.ptr(layer), _hip.ptr(ray_seg), _hip.ptr(E),
                                                _hip.ptr(s), S, R, B, C, K, *(ctypes.c_void_p(o.data_ptr()) for o in outs), _hip.stream())
    assert rc == 0
    assert all(torch.equal(o, want[k]) for o, k in zip(outs, ("spectral", "spectral2", "specular")))


def test_argument_rules():
    from umhsnerf import _hip, ops

    lib, d, ARG, UNSUP = _hip.lib(), ctypes.c_void_p(4096), -1, -2
    call = lambda fn, defaults, **kw: fn(*[kw.get(k, v) for k, v in defaults.items()])
    table = (ctypes.c_float * 16)()
    cl = dict(wpos=d, n=8, table=table, K=1, out=d, stream=None)
    assert call(lib.umhs_region_classify, cl, wpos=None) == ARG and call(lib.umhs_region_classify, cl, out=None) == ARG
    assert call(lib.umhs_region_classify, cl, table=None) == ARG and call(lib.umhs_region_classify, cl, K=9) == ARG
    assert call(lib.umhs_region_classify, cl, K=-1) == ARG and call(lib.umhs_region_classify, cl, n=-1) == ARG
    assert call(lib.umhs_region_classify, cl, n=0, wpos=None, out=None) == 0
    sg = dict(region=d, ray=d, pinfo=d, n=8, R=2, seg_of=d, seg_info=d, seg_layer=d, ray_seg=d, count=d, ws=d, wsb=1 << 20, stream=None)
    for missing in ("region", "ray", "pinfo", "seg_of", "seg_info", "seg_layer", "ray_seg", "count"):
        assert call(lib.umhs_region_segments, sg, **{missing: None}) == ARG, missing
    assert call(lib.umhs_region_segments, sg, ws=None) == -3 and call(lib.umhs_region_segments, sg, wsb=8) == -3
    assert call(lib.umhs_region_segments, sg, ws=ctypes.c_void_p(4100)) == -3
    assert call(lib.umhs_region_segments, sg, n=-1) == ARG and call(lib.umhs_region_segments, sg, R=-1) == ARG
    assert call(lib.umhs_region_segments, sg, n=0, region=None, ws=None) == 0 and call(lib.umhs_region_segments, sg, R=0, pinfo=None) == 0
    assert lib.umhs_region_segments_workspace_bytes(257) >= 2 * 12 and lib.umhs_region_segments_workspace_bytes(-1) == 0
    sr = dict(s=d, a=d, region=d, g=d, n=8, C=3, K=2, out=d, stream=None)
    for missing in ("s", "a", "region", "g", "out"):
        assert call(lib.umhs_material_sigma_regions, sr, **{missing: None}) == ARG, missing
    assert all(call(lib.umhs_material_sigma_regions, sr, **kw) == ARG for kw in (dict(C=0), dict(C=16), dict(K=-1), dict(K=9), dict(n=-1)))
    assert call(lib.umhs_material_sigma_regions, sr, n=0, s=None, a=None, region=None, g=None, out=None) == 0
    ss = dict(values=d, ray_seg=d, S=4, R=2, k=3, out=d, stream=None)
    for missing in ("values", "ray_seg", "out"):
        assert call(lib.umhs_segment_sum, ss, **{missing: None}) == ARG, missing
    assert call(lib.umhs_segment_sum, ss, k=0) == ARG and call(lib.umhs_segment_sum, ss, S=-1) == ARG and call(lib.umhs_segment_sum, ss, k=257) == UNSUP
    assert call(lib.umhs_segment_sum, ss, R=0, values=None, ray_seg=None, out=None) == 0
    o1, o2, o3 = (ctypes.c_void_p(4096 * i) for i in (2, 3, 4))
    rm = dict(mix=d, cs=ctypes.c_void_p(8192 * 4), layer=d, ray_seg=d, E=d, s=d, S=4, R=2, B=31, C=3, K=1, spectral=o1, spectral2=o2, specular=o3,
              stream=None)
    remix = lambda **kw: call(lib.umhs_material_remix_regions, rm, **kw)
    for missing in ("mix", "layer", "ray_seg", "E", "s", "spectral", "spectral2", "specular"):
        assert remix(**{missing: None}) == ARG, missing
    assert remix(cs=None) == ARG and remix(cs=None, spectral2=None) == ARG and remix(cs=None, specular=None) == ARG
    assert remix(cs=o3) == ARG  # an output may not be an input array
    assert all(remix(**kw) == ARG for kw in (dict(C=0), dict(C=16), dict(B=0), dict(R=-1), dict(S=-1), dict(K=-1), dict(K=9)))
    assert remix(B=257) == UNSUP
    assert remix(R=0) == 0 and remix(R=0, cs=None, spectral2=None, specular=None, mix=None, E=None, spectral=None, layer=None, ray_seg=None, s=None) == 0
    for fn, args in ((ops.region_classify, (torch.rand(4, 3), RF.DYADIC_TABLE)),
                     (ops.material_sigma_regions, (torch.rand(4), torch.rand(4, 3), torch.zeros(4, dtype=torch.uint8), torch.ones(2, 3))),
                     (ops.segment_sum, (torch.rand(4, 3), torch.zeros(2, 2, dtype=torch.int64))),
                     (ops.region_segments, (torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), torch.tensor([[0, 4]])))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args)


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def world_spec(tmp_path_factory):
    return _make_world(tmp_path_factory.mktemp("region_spec"), True)


@pytest.fixture(scope="module")
def world_plain(tmp_path_factory):
    return _make_world(tmp_path_factory.mktemp("region_plain"), False)


@pytest.fixture(params=["specular", "no_specular"])
def world(request):
    return request.getfixturevalue("world_spec" if request.param == "specular" else "world_plain")


def _edits(world, doc):
    from umhsnerf.materials import load_material_edits

    return load_material_edits(doc, 3, 8, world["specular"])


def _edit_x(world):
    doc = {"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}, {"material": 0, "gain": 0.4},
                         {"material": 1, "density": 0.25}]}
    if world["specular"]:
        doc["specular_gain"] = 0.5
    return doc


def _frame_samples(world):
    """The samples of frame 1, flat, and their model-frame positions as the render computes them."""
    from umhsnerf import ops

    model = world["pipe"].model
    ray_samples, ray_indices = _samples(world)
    s = model._flat_samples(ray_samples, ray_indices, H * W, None)
    wpos = ops.positions_fwd(s.o, s.d, s.t0, s.t1, model.field._spec())[0]
    return ray_samples, ray_indices, s, wpos


def _middle(points):
    """(centre, extent) of a point set: the per-axis median and the 1 % .. 99 % span (a contracted scene throws a few samples far out),
    rounded to what a file would carry."""
    p = np.asarray(points, np.float64)
    p = p[np.isfinite(p).all(1)]
    lo, hi = np.quantile(p, 0.01, axis=0), np.quantile(p, 0.99, axis=0)
    return [round(float(v), 3) for v in np.median(p, axis=0)], [round(float(v), 3) for v in hi - lo]


def _half_box(points):
    """A box of half the extent of the points, about their middle."""
    centre, extent = _middle(points)
    return {"center": centre, "rotation": [0.0, 0.0, 0.0], "scale": [round(0.5 * v, 3) for v in extent]}


def _outputs(world, ray_samples, ray_indices, edits=None):
    model = world["pipe"].model
    ctx = contextlib.nullcontext() if edits is None else model.material_edits_context(edits)
    with torch.no_grad(), ctx:
        return model.get_outputs_from_samples(ray_samples, ray_indices, H * W)


def _close(got, ref, keys):
    worst = {}
    for k in keys:
        a, b = got[k].double().cpu().reshape(-1), ref[k].double().cpu().reshape(-1)
        worst[k] = float(((a - b).abs() / (1e-4 * b.abs() + 1e-6)).max()) if a.numel() else 0.0
    return worst


def _float_keys(world):
    return ["spectral", "rgb", "abundances", "seg_probs"] + (["spectral2", "specular"] if world["specular"] else [])


def test_the_heads_pass_forms_its_sums_per_run_whatever_the_run_is(world):
    """The assumption the feature rests on: handed a SEGMENT partition and the same weights, umhs_field_heads_fwd returns per-segment
    sums which, added per ray, are the ray-partition call's."""
    from umhsnerf import ops

    model = world["pipe"].model
    _, _, s, wpos = _frame_samples(world)
    spec, flat = model.field._spec(), model.field.flat.detach()
    assert 2000 < s.n
    with torch.no_grad():
        pos01, sel = ops.positions_fwd(s.o, s.d, s.t0, s.t1, spec)[1:]
        enc = ops.hashgrid_fwd(pos01, spec.layout.view(flat, "mlp_base.encoder.hash_table"), spec.scalings, spec.layout.log2_hashmap_size, True)
        fo = ops.field_base_fwd(spec, flat, enc, True, sel, pack_ready=False, rows16=True)
        weights = ops.composite_fwd(fo["sigma"], s.t0, s.t1, s.packed_info, [])[0]
        heads = lambda ri, pi: ops.field_heads_fwd(spec, flat, fo["base16"], wpos, s.d, weights, ri, pi, want_logits=False, pack_ready=True,
                                                   release=False, want_mix=True)
        by_ray = heads(s.ray_indices, s.packed_info)
        by_ray = dict(comp=by_ray["comp"], ab=by_ray["comp_abundances"], mix=by_ray["mix"].clone())
        rng = np.random.default_rng(4)
        region = np.zeros(s.n, np.uint8)
        i = 0
        while i < s.n:  # runs of 1..40 samples, cut again wherever a ray ends
            run = int(rng.integers(1, 41))
            region[i:i + run] = rng.integers(0, 4)
            i += run
        seg_of, seg_info, seg_layer, ray_seg, S = ops.region_segments(_dev(region), s.ray_indices, s.packed_info)
        assert S > 2 * int((s.packed_info[:, 1] > 0).sum())
        by_seg = heads(seg_of, seg_info)
        mix_seg = by_seg["mix"].clone()
        assert all(tuple(c.shape) == (S, 8) for c in by_seg["comp"]) and tuple(by_seg["comp_abundances"].shape) == (S, 3)
        pairs = [(ops.segment_sum(c, ray_seg), r) for c, r in zip(by_seg["comp"], by_ray["comp"])]
        pairs += [(ops.segment_sum(by_seg["comp_abundances"], ray_seg), by_ray["ab"])]
        pairs += [(ops.segment_sum(mix_seg[:, :3].contiguous(), ray_seg), by_ray["mix"][:, :3])]
    assert len(pairs) == (5 if world["specular"] else 3)
    live = (s.packed_info[:, 1] > 0).cpu()
    for got, ref in pairs:
        a, b = got.double().cpu(), ref.double().cpu()
        assert bool(((a - b).abs()[live] <= 1e-4 * b.abs()[live] + 1e-6).all()), float((a - b).abs().max())
        assert float(b.abs()[live].max()) > 1e-3 and bool((a[~live] == 0).all())


def test_a_region_that_no_sample_meets_changes_nothing(world):
    ray_samples, ray_indices, s, wpos = _frame_samples(world)
    doc = _edit_x(world)
    with_far = _edits(world, dict(doc, regions=[dict(FAR, materials=[{"material": 0, "density": 0.0}, {"material": 1, "gain": 3.0}])]))
    assert not RF.classify32(wpos.cpu().numpy(), with_far.region_table()).any()
    ref = _outputs(world, ray_samples, ray_indices, _edits(world, doc))
    got = _outputs(world, ray_samples, ray_indices, with_far)
    assert list(got) == list(ref)
    for k in ("weights", "accumulation", "depth", "num_samples_per_ray"):
        assert torch.equal(got[k], ref[k]), k
    worst = _close(got, ref, _float_keys(world))
    print(worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert torch.equal(got["seg_raw"], ref["seg_raw"]) or float((got["seg_raw"] != ref["seg_raw"]).float().mean()) <= 0.02
    assert world["pipe"].model._material_edits is None and world["pipe"].model._material_regions is None


def test_a_box_around_everything_is_the_global_edit(world):
    ray_samples, ray_indices, s, wpos = _frame_samples(world)
    x = _edit_x(world)
    boxed = _edits(world, {"regions": [dict(EVERYWHERE, **x)]})
    assert (RF.classify32(wpos.cpu().numpy(), boxed.region_table()) == 1).all()
    ref = _outputs(world, ray_samples, ray_indices, _edits(world, x))
    got = _outputs(world, ray_samples, ray_indices, boxed)
    plain = _outputs(world, ray_samples, ray_indices)
    assert list(got) == list(ref) == list(plain) and not torch.equal(ref["weights"], plain["weights"])
    for k in ("weights", "accumulation", "depth", "num_samples_per_ray"):
        assert torch.equal(got[k], ref[k]), k
    worst = _close(got, ref, _float_keys(world))
    print(worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert float((got["spectral"] - plain["spectral"]).abs().max()) > 1e-3  # the edit is not a small one


def _regional_reference(world, edits, ray_samples, ray_indices, wpos):
    model = world["pipe"].model
    layer = torch.from_numpy(RF.classify32(wpos.cpu().numpy(), edits.region_table()).astype(np.int64))
    fr = ray_samples.frustums
    p = MF.field_params_of(model.field)
    E = model.field.endmembers.detach()
    ref = RF.regional_render(p, edits.dictionaries(E), edits.density_gains("cpu"), edits.specular_gains("cpu"), layer, fr.origins,
                             fr.directions, fr.starts, fr.ends, ray_indices, H * W, 0.4, model.converter.transform_matrix,
                             contraction=model.field.spatial_distortion is not None)
    return ref, layer


def test_removing_a_material_inside_a_box_equals_the_float64_regional_render(world):
    """Material 1 removed inside a box of half the scene's extent, against tests/region_f64.regional_render in float64 on the same
    samples with the layers of the float32 replay: every output within 1e-4 |ref| + 1e-6; seg_raw as in
    test_hip_material.test_removing_a_material_equals_the_float64_edited_render."""
    model = world["pipe"].model
    ray_samples, ray_indices, s, wpos = _frame_samples(world)
    edits = _edits(world, {"regions": [{"box": _half_box(wpos.cpu().numpy()), "materials": [{"material": 1, "density": 0.0}]}]})
    got = _outputs(world, ray_samples, ray_indices, edits)
    plain = _outputs(world, ray_samples, ray_indices)
    everywhere = _outputs(world, ray_samples, ray_indices, _edits(world, {"materials": [{"material": 1, "density": 0.0}]}))
    ref, layer = _regional_reference(world, edits, ray_samples, ray_indices, wpos)
    share = float((layer == 1).double().mean())
    print("samples inside the box:", share)
    assert 0.05 < share < 0.95
    assert list(got) == list(plain)
    assert not torch.equal(got["accumulation"], plain["accumulation"]) and not torch.equal(got["accumulation"], everywhere["accumulation"])
    keys = ["accumulation", "depth", "weights"] + _float_keys(world)
    worst = {}
    for k in keys:
        a, b = got[k].double().cpu().reshape(ref[k].shape), ref[k].double()
        worst[k] = float(((a - b).abs() / (1e-4 * b.abs() + 1e-6)).max())
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    acc64 = ref["accumulation"].reshape(-1)
    tied = MF.cluster_ties(ref["unedited_spectral"], model.field.endmembers.detach().double().cpu())[2].sum(1) > 1
    edge = (acc64 - 0.5).abs() <= 1e-4 * 0.5 + 1e-6
    left_out = tied | edge
    assert float(left_out.double().mean()) <= 0.02
    same = got["seg_raw"].reshape(-1).double().cpu() == ref["seg_raw"].reshape(-1)
    assert bool((same | left_out).all()), int((~same & ~left_out).sum())
    assert float(acc64.max()) > 0.01 and int((plain["num_samples_per_ray"] > 0).sum()) > H * W // 4
    # teeth: the regional render's weights are neither the plain ones nor the global removal's: somewhere they differ by more than
    # ten times the tolerance (the scene is a fog of ~1000 small weights per ray, most of them below the tolerance's absolute term)
    w64 = ref["weights"].double().reshape(-1)
    for name, other in (("plain", plain), ("removed everywhere", everywhere)):
        d = (other["weights"].double().cpu().reshape(-1) - w64).abs() / (1e-4 * w64.abs() + 1e-6)
        print(f"weights against {name}: worst {float(d.max()):.1f} tolerances, {float((d > 1).double().mean()):.4f} of the samples beyond one")
        assert float(d.max()) > 10


def test_a_recolour_inside_a_sphere(world):
    """Rays with no sample in the sphere carry the top-level edit's spectrum; rays with one carry the float64 regional render's."""
    ray_samples, ray_indices, s, wpos = _frame_samples(world)
    top = {"materials": [{"material": 0, "gain": 0.4}]}
    inside = {"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}, {"material": 1, "from_material": 0}]}
    if world["specular"]:
        top["specular_gain"], inside["specular_gain"] = 0.5, 2.0
    # the sphere: about the middle of the samples of the image's top-left block, the largest of a few radii that leaves rays on both
    # sides (chosen from the positions alone, with the float32 membership rule)
    pos, ri = wpos.cpu().numpy(), ray_indices.cpu().long()
    corner = ((ri // W < H // 3) & (ri % W < W // 3)).numpy()
    centre, extent = _middle(pos[corner])[0], _middle(pos)[1]
    sphere = None
    for share in (0.3, 0.2, 0.15, 0.1, 0.05):
        sphere = {"center": centre, "radius": round(share * min(extent), 4)}
        hit = torch.zeros(H * W, dtype=torch.bool)
        hit[ri[torch.from_numpy(RF.classify32(pos, RF.sphere_record(sphere["center"], sphere["radius"])[None]) == 1)]] = True
        if int(hit.sum()) > 20 and int((~hit & (s.packed_info[:, 1] > 0).cpu()).sum()) > 20:
            break
    edits = _edits(world, dict(top, regions=[dict(inside, sphere=sphere)]))
    assert edits.edits_dictionary and not edits.edits_density
    got = _outputs(world, ray_samples, ray_indices, edits)
    top_only = _outputs(world, ray_samples, ray_indices, _edits(world, top))
    ref, layer = _regional_reference(world, edits, ray_samples, ray_indices, wpos)
    touched = torch.zeros(H * W, dtype=torch.bool)
    touched[ray_indices.cpu().long()[layer == 1]] = True
    live = (s.packed_info[:, 1] > 0).cpu()
    print("rays through the sphere:", int(touched.sum()), "of", int(live.sum()))
    assert int(touched.sum()) > 20 and int((live & ~touched).sum()) > 20
    for k in ("weights", "accumulation", "depth", "num_samples_per_ray"):
        assert torch.equal(got[k], top_only[k]), k  # a recolour moves no density
    flat = lambda v: v.double().cpu().reshape(H * W, -1)
    tol = lambda b: 1e-4 * b.abs() + 1e-6
    keys = ["spectral"] + (["spectral2", "specular"] if world["specular"] else [])
    for k in keys:
        a, t, r = flat(got[k]), flat(top_only[k]), ref[k].double().reshape(H * W, -1)
        assert bool(((a - t).abs() <= tol(t))[~touched].all()), k
        assert bool(((a - r).abs() <= tol(r)).all()), (k, float(((a - r).abs() / tol(r)).max()))
    a, t = flat(got["spectral"]), flat(top_only["spectral"])
    assert float(((a - t).abs() > 10 * tol(t))[touched].double().mean()) > 0.5  # inside, the recolour shows
    worst = _close(got, ref, ["rgb", "abundances", "seg_probs"])
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path))


def test_camera_path_renders_a_regions_file_and_refuses_a_bad_region(world_spec, monkeypatch):
    from umhsnerf import render

    world = world_spec
    root, model = world["root"], world["pipe"].model
    doc = {"materials": [{"material": 0, "gain": 0.4}],
           "regions": [{"sphere": SPHERE, "materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}], "specular_gain": 2.0},
                       {"box": HALF_BOX, "materials": [{"material": 1, "density": 0.0}]}]}
    (root / "regions.json").write_text(json.dumps(doc))
    names = ["rgb", "accumulation"]
    argv = ["camera-path", *_common(world), "--camera-path-filename", str(root / "path.json"), "--rendered-output-names", *names]
    got = render.main([*argv, "--output-path", str(root / "regional"), "--material-edits", str(root / "regions.json")])
    assert got["frames"] == 3 and got["material_edits"] == str(root / "regions.json")
    render.main([*argv, "--output-path", str(root / "bare")])
    edits = _edits(world, doc)
    for i in range(3):
        with model.material_edits_context(edits):
            outputs = model.get_outputs_for_camera_ray_bundle(world["cameras"].generate_rays(i, keep_shape=True))
        frame = _png(root / "regional" / f"frame_{i:05d}.png")
        assert np.array_equal(frame, render.compose_frame(outputs, names).cpu().numpy())
        assert not np.array_equal(frame, _png(root / "bare" / f"frame_{i:05d}.png"))
    assert model._material_edits is None and model._material_regions is None
    (root / "bad_region.json").write_text(json.dumps({"regions": [{"sphere": SPHERE}, {"box": dict(HALF_BOX, scale=[1.0, 0.0, 1.0])}]}))

    def never(*a, **k):
        raise AssertionError("rendering started")

    monkeypatch.setattr(render, "render_camera_path", never)
    with pytest.raises(ValueError, match=r"region 2: scale 0.0 must be > 0"):
        render.main([*argv, "--output-path", str(root / "no"), "--material-edits", str(root / "bad_region.json")])
    assert not (root / "no").exists()


def _opaque_unmixed_checkpoint(world, log_gain=4.0):
    """``test_hip_material._unmixed_checkpoint`` with the density multiplied by e^log_gain (the bias of mlp_base's density output;
    the density is its exponential): a ray stops where it meets matter, so a point of the cloud lies ON the material it is labelled
    with.  The three-step scene as trained is a fog: a ray's weights spread over its whole length, its expected depth falls in the
    middle of the scene and says little about where the material it is labelled with lies."""
    flags = _unmixed_checkpoint(world)
    root = world["root"]
    ck = torch.load(root / "unmixed.ckpt")
    key = [k for k in ck["pipeline"] if k.endswith("field.mlp_base.mlp.layers.1.bias")]
    assert len(key) == 1, key
    ck["pipeline"][key[0]][0] += log_gain
    torch.save(ck, root / "opaque.ckpt")
    flags[flags.index("--checkpoint") + 1] = str(root / "opaque.ckpt")
    return flags


def test_a_point_cloud_with_a_material_removed_inside_a_box_has_no_such_point_there(world_plain):
    """``export pointcloud`` under "material K removed inside the box": no point that lies inside the box (the float32 membership rule
    on the written coordinates) is labelled K.  The scene is ``_opaque_unmixed_checkpoint``: what the statement is about (a point is
    where its ray stops, and a sample is made of one material).  The box is the octant of the scene from its middle outwards, far
    beyond its rim: a ray from a camera outside meets it before it meets anything else of the scene, or after it has been stopped.
    K is the label most points inside the box carry without the edit."""
    import pointcloud_ref as P
    from umhsnerf import export

    world = world_plain
    root = world["root"]
    pc = ["pointcloud", *_opaque_unmixed_checkpoint(world), "--num-points", "4000", "--num-rays-per-batch", "4096", "--remove-outliers", "false"]
    export.main([*pc, "--output-dir", str(root / "pc_unedited")])
    table, _ = P.read_ply(root / "pc_unedited" / "point_cloud.ply")
    xyz = lambda t: np.stack([t["x"], t["y"], t["z"]], 1).astype(np.float32)
    centre, extent = _middle(xyz(table))
    octant = {"center": [round(c + 25.0 * e, 3) for c, e in zip(centre, extent)], "rotation": [0.0, 0.0, 0.0],
              "scale": [round(50.0 * e, 3) for e in extent]}
    box = RF.box_record(octant["center"], octant["rotation"], octant["scale"])[None]
    inside = RF.classify32(xyz(table), box) == 1
    counts = np.bincount(table["material"][inside] + 1, minlength=4)[1:]
    K = int(counts.argmax())
    assert counts[K] > 20 and 0.02 < inside.mean() < 0.5
    (root / "remove_in_box.json").write_text(json.dumps({"regions": [{"box": octant, "materials": [{"material": K, "density": 0.0}]}]}))
    got = export.main([*pc, "--output-dir", str(root / "pc_boxed"), "--material-edits", str(root / "remove_in_box.json")])
    assert got["material_edits"] == str(root / "remove_in_box.json") and got["points"] > 0
    edited, _ = P.read_ply(root / "pc_boxed" / "point_cloud.ply")
    inside = RF.classify32(xyz(edited), box) == 1
    after = np.bincount(edited["material"][inside] + 1, minlength=4)[1:]
    everywhere = np.bincount(edited["material"] + 1, minlength=4)[1:]
    print(f"labels inside the box: unedited {counts.tolist()}, with material {K} removed there {after.tolist()}; everywhere {everywhere.tolist()}")
    bad = inside & (edited["material"] == K)
    if bad.any():  # (what a failure is read from: where the offending points lie relative to the box's three inner faces)
        print("offending points minus the box's inner corner, in extents:", ((xyz(edited)[bad] - np.asarray(centre)) / np.asarray(extent)).round(3).tolist()[:20])
        print("their composited abundances:", np.stack([edited[f"abundance_{i}"][bad] for i in range(3)], 1).round(3).tolist()[:20])
    assert after[K] == 0
    assert everywhere[K] > 0  # outside the box the material is still there
