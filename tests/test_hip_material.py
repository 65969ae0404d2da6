"""Material edits on the GPU: csrc/umhs_material.hip per element against float64 (tests/material_f64.py), the edited render of
``UMHSModel.material_edits_context`` on the small trained pipeline of tests/test_hip_crop_render.py (``make_scene(B=8)``, 3 classes, three
steps at 1024 rays, 20 x 28 path frames; with and without the specular head), and ``--material-edits`` on the command lines."""
import contextlib
import ctypes
import json

import numpy as np
import pytest
import torch

import material_f64 as MF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FOVS = 20, 28, (50.0, 75.0, 50.0)
BASE_FLAGS = ["--num-classes", "3", "--temperature", "0.4", "--background-color", "black"]
CROP = {"crop_center": [0.1, -0.05, 0.2], "crop_scale": [0.9, 0.6, 1.2], "crop_rot": [0.3, -0.2, 0.5], "crop_bg_color": {"r": 38, "g": 120, "b": 255}}
SIGMA_CASES = [(n, C) for n in MF.SIGMA_NS for C in MF.SIGMA_CS]


def _dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernels
# ------------------------------------------------------------------------------------------------------------------------------ #
def _run_remix(case):
    from umhsnerf import ops

    outs = ops.material_remix(_dev(case["mix"]), _dev(case["comp_specular"]), _dev(case["E"]), case["s"])
    return dict(zip(("spectral", "spectral2", "specular"), outs))


@pytest.mark.parametrize("c", MF.REMIX_CASES, ids=MF.remix_id)
def test_remix_is_within_the_bound_of_float64_and_repeats_bit_for_bit(c):
    case = MF.make_remix_case(*c)
    got, report = _run_remix(case), {}
    fails = MF.check_remix(case, got, MF.remix_oracle(case, torch.float64), report)
    print(MF.remix_id(c), {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})
    assert not fails, fails
    assert all(tuple(v.shape) == (c[0], c[1]) and bool(torch.isfinite(v).all()) for v in got.values())  # the NaN columns were not read
    again = _run_remix(case)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_remix_takes_the_same_bits_on_unaligned_rows():
    """B % 4 == 0 with a row array off the 16-byte grid takes the one-float form: the same fmaf chain, the same bits."""
    from umhsnerf import _hip, ops

    case = MF.make_remix_case(257, 64, 15, True)
    want = _run_remix(case)
    R, B, C = case["R"], case["B"], case["C"]
    mix, E = _dev(case["mix"]), _dev(case["E"])  # (held: a temporary would be freed, and its block reused, before the launch)
    pad = lambda: torch.zeros(R * B + 1, device=DEV)[1:].view(R, B)
    cs = pad()
    cs.copy_(case["comp_specular"])
    outs = [pad(), pad(), pad()]
    assert cs.data_ptr() % 16 == 4
    rc = _hip.lib().umhs_material_remix(_hip.ptr(mix), ctypes.c_void_p(cs.data_ptr()), _hip.ptr(E), case["s"], R, B, C,
                                        *(ctypes.c_void_p(o.data_ptr()) for o in outs), _hip.stream())
    assert rc == 0
    assert all(torch.equal(o, want[k]) for o, k in zip(outs, ("spectral", "spectral2", "specular")))
    # specular written over comp_specular
    rc = _hip.lib().umhs_material_remix(_hip.ptr(mix), ctypes.c_void_p(cs.data_ptr()), _hip.ptr(E), case["s"], R, B, C,
                                        ctypes.c_void_p(outs[0].data_ptr()), ctypes.c_void_p(outs[1].data_ptr()), ctypes.c_void_p(cs.data_ptr()),
                                        _hip.stream())
    assert rc == 0 and torch.equal(cs, want["specular"]) and torch.equal(outs[0], want["spectral"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.material_remix(case["mix"], None, case["E"], 1.0)


def test_null_pointer_rules_are_argument_errors():
    from umhsnerf import _hip

    lib, d, ARG = _hip.lib(), ctypes.c_void_p(4096), -1
    remix = lambda **kw: lib.umhs_material_remix(*[kw.get(k, v) for k, v in dict(
        mix=d, cs=d, E=d, s=1.0, R=8, B=31, C=3, spectral=d, spectral2=d, specular=d, stream=None).items()])
    for missing in ("mix", "E", "spectral", "spectral2", "specular"):
        assert remix(**{missing: None}) == ARG, missing
    assert remix(cs=None) == ARG and remix(cs=None, spectral2=None) == ARG and remix(cs=None, specular=None) == ARG
    assert remix(C=0) == ARG and remix(C=16) == ARG and remix(B=0) == ARG and remix(R=-1) == ARG and remix(B=257) == -2
    assert remix(R=0) == 0 and remix(R=0, cs=None, spectral2=None, specular=None, mix=None, E=None, spectral=None) == 0
    sigma = lambda **kw: lib.umhs_material_sigma(*[kw.get(k, v) for k, v in dict(s=d, a=d, g=d, n=8, C=3, out=d, stream=None).items()])
    for missing in ("s", "a", "g", "out"):
        assert sigma(**{missing: None}) == ARG, missing
    assert sigma(C=0) == ARG and sigma(C=16) == ARG and sigma(n=-1) == ARG
    assert sigma(n=0, s=None, a=None, g=None, out=None) == 0
    cfg = _hip.FieldCfg(31, 6, 1, 0, 0.4)
    off = lib.umhs_field_heads_fwd_mix_offset(ctypes.byref(cfg), 64, 4)
    assert off >= 0 and off % 16 == 0 and off + 4 * 64 <= lib.umhs_field_heads_fwd_scratch_bytes(ctypes.byref(cfg), 64, 4)
    assert lib.umhs_field_heads_fwd_mix_offset(ctypes.byref(_hip.FieldCfg(31, 16, 1, 0, 0.4)), 64, 4) == -1
    assert lib.umhs_field_heads_fwd_mix_offset(None, 64, 4) == -1 and lib.umhs_field_heads_fwd_mix_offset(ctypes.byref(cfg), -1, 4) == -1


@pytest.mark.parametrize("n,C", SIGMA_CASES, ids=[MF.sigma_id(c) for c in SIGMA_CASES])
def test_sigma_is_within_the_bound_of_float64(n, C):
    from umhsnerf import ops

    case = MF.make_sigma_case(n, C)
    s, a, g = _dev(case["sigma"]), _dev(case["a"]), _dev(case["gain"])
    got, report = ops.material_sigma(s, a, g), {}
    fails = MF.check_sigma(case, got, MF.sigma_oracle(case, torch.float64), report)
    print(n, C, report)
    assert not fails, fails
    assert torch.equal(s.cpu(), case["sigma"])  # out of place left its input alone
    inplace = s.clone()
    assert ops.material_sigma(inplace, a, g, out=inplace) is inplace and torch.equal(inplace, got)
    ones = ops.material_sigma(s, a, torch.ones(C, device=DEV))
    assert torch.equal(ones, s)  # all-ones gains: the input, bit for bit
    above = _dev(MF.rows_summing_above_one(n, C))
    zero = ops.material_sigma(s, above, torch.zeros(C, device=DEV))
    assert bool((zero >= 0).all()) and bool((zero == 0).all())  # all-zero gains on rows that sum to 1 + 2^-23: never negative
    soft = ops.material_sigma(s, a, torch.zeros(C, device=DEV))
    assert bool((soft >= 0).all()) and bool((soft <= s * 2.0 ** -18).all())  # |1 - sum a| <= 2 C u


def test_sigma_has_no_cpu_path():
    from umhsnerf import ops

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.material_sigma(torch.rand(4), torch.rand(4, 3), torch.ones(3))


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
def _make_world(root, pred_specular):
    from test_hip_distortion import _look_at_origin, make_scene
    from umhsnerf.data.umhs_datamanager import UMHSDataManager, UMHSDataManagerConfig
    from umhsnerf.data.umhs_dataparser import UMHSDataParserConfig
    from umhsnerf.render import load_camera_path
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    torch.manual_seed(0)
    scene = root / "scene"
    meta = make_scene(scene, B=8)
    dm = UMHSDataManager(UMHSDataManagerConfig(dataparser=UMHSDataParserConfig(data=scene), train_num_rays_per_batch=1024), device=DEV,
                         num_classes=3, seed=9)
    cfg = UMHSConfig(method="rgb+spectral", pred_specular=pred_specular, temperature=0.4, background_color="black")
    pipe = UMHSPipeline.from_packed_samples(cfg, DEV, metadata={"wavelengths": meta["wavelengths"], "num_classes": 3}, seed=2, datamanager=dm)
    for step in range(3):
        pipe.get_train_loss_dict(step)
    torch.cuda.synchronize()
    pipe._ahead = None
    pipe.eval()
    torch.save({"step": 3, "pipeline": pipe.state_dict()}, root / "step-000000003.ckpt")
    rng = np.random.default_rng(11)
    path = {"camera_type": "perspective", "render_height": H, "render_width": W, "fps": 24, "seconds": 0.125,
            "camera_path": [{"camera_to_world": _look_at_origin(rng).reshape(-1).tolist(), "fov": fov, "aspect": W / H} for fov in FOVS]}
    (root / "path.json").write_text(json.dumps(path))
    cameras, _ = load_camera_path(path, device=DEV)
    flags = BASE_FLAGS + (["--pred-specular"] if pred_specular else [])
    return dict(root=root, scene=scene, pipe=pipe, path=path, cameras=cameras, specular=pred_specular, flags=flags)


@pytest.fixture(scope="module")
def world_spec(tmp_path_factory):
    return _make_world(tmp_path_factory.mktemp("material_spec"), True)


@pytest.fixture(scope="module")
def world_plain(tmp_path_factory):
    return _make_world(tmp_path_factory.mktemp("material_plain"), False)


@pytest.fixture(params=["specular", "no_specular"])
def world(request):
    return request.getfixturevalue("world_spec" if request.param == "specular" else "world_plain")


def _edits(world, doc):
    from umhsnerf.materials import load_material_edits

    return load_material_edits(doc, 3, 8, world["specular"])


def _render(world, edits="plain", camera=1):
    model = world["pipe"].model
    rb = world["cameras"].generate_rays(camera, keep_shape=True)
    ctx = contextlib.nullcontext() if isinstance(edits, str) else model.material_edits_context(edits)
    with ctx:
        return model.get_outputs_for_camera_ray_bundle(rb)


@contextlib.contextmanager
def _spy_remix():
    """Record what every ``ops.material_remix`` call was handed (the mix is a view into a scratch: cloned at once)."""
    from umhsnerf import ops

    calls, real = [], ops.material_remix

    def spy(mix, comp_specular, E_edit, specular_gain=1.0):
        calls.append(dict(mix=mix.clone(), comp_specular=None if comp_specular is None else comp_specular.clone(), E=E_edit.clone(),
                          s=float(specular_gain)))
        return real(mix, comp_specular, E_edit, specular_gain)

    ops.material_remix = spy
    try:
        yield calls
    finally:
        ops.material_remix = real


def _recolour_doc(world):
    doc = {"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}, {"material": 0, "gain": 0.4}]}
    if world["specular"]:
        doc["specular_gain"] = 0.5
    return doc


def _flat(v):
    return v.reshape(-1, v.shape[-1])


def test_identity_and_none_are_the_plain_render(world):
    from umhsnerf.materials import MaterialEdits

    plain = _render(world)
    assert int(plain["num_samples_per_ray"].sum()) > 0
    with _spy_remix() as calls:
        for edits in (None, MaterialEdits.identity(3, 8, world["specular"]), _edits(world, {"materials": [{"material": c, "density": 1.0} for c in range(3)]})):
            got = _render(world, edits)
            assert list(got) == list(plain)
            for k in plain:
                assert torch.equal(got[k], plain[k]), k
    assert not calls and world["pipe"].model._material_edits is None


def test_a_recolour_changes_the_spectrum_and_nothing_else(world):
    from umhsnerf import _hip, ops

    model = world["pipe"].model
    edits = _edits(world, _recolour_doc(world))
    assert edits.edits_dictionary and not edits.edits_density
    plain = _render(world)
    with _spy_remix() as calls:
        got = _render(world, edits)
    assert list(got) == list(plain) and len(calls) == 1
    for k in ("accumulation", "depth", "abundances", "seg_probs", "seg_raw", "seg_pred", "weights", "num_samples_per_ray"):
        if k in plain:
            assert torch.equal(got[k], plain[k]), k
    assert not torch.equal(got["spectral"], plain["spectral"]) and not torch.equal(got["rgb"], plain["rgb"])
    call = calls[0]
    E2 = edits.dictionary(model.field.endmembers)
    assert torch.equal(call["E"], E2) and call["s"] == edits.specular_gain and (call["comp_specular"] is not None) == world["specular"]
    if world["specular"]:
        assert torch.equal(call["comp_specular"], _flat(plain["specular"]))
    # spectral / spectral2 / specular against the float64 remix of that mix
    ref = MF.remix64(call["mix"], call["E"], call["comp_specular"], call["s"])
    env = MF.remix_envelopes(call["mix"], call["E"], call["comp_specular"], call["s"])
    fails, report = [], {}
    live = (plain["num_samples_per_ray"].reshape(-1) > 0).cpu()[:, None]
    for k in ref:
        fails += MF.check(k, _flat(got[k]), ref[k], env[k], MF.K_REMIX, report, teeth_mask=live)
    print(report)
    assert not fails, fails
    assert not MF.teeth_failures(report), report
    # per-band views follow the edited arrays
    assert torch.equal(got["wv_3"][..., 0], got["spectral"][..., 3]) and torch.equal(got["abundances_1"][..., 0], got["abundances"][..., 1])
    if world["specular"]:
        assert torch.equal(got["residual_2"][..., 0], got["specular"][..., 2])
    # rgb: the existing colour conversion of the returned spectrum, bit for bit
    M = _hip.f32c(model.converter.transform_matrix)
    spectral = _flat(got["spectral"]).contiguous()
    acc, depth = got["accumulation"].reshape(-1).contiguous(), got["depth"].reshape(-1).contiguous()
    mm = ops.tmid_minmax(depth, depth)
    rgb = ops.ray_epilogue_fwd(spectral, M, model.field.endmembers.detach(), acc, depth, mm, _hip.f32c(model.class_colors), 0.2)[0]
    assert torch.equal(_flat(got["rgb"]), rgb)
    # against a plain render with the model's dictionary overwritten by E'': the same mixing term, but ITS segmentation moved
    E = model.field.endmembers
    saved = E.detach().clone()
    try:
        with torch.no_grad():
            E.copy_(E2)
        swapped = _render(world)
    finally:
        with torch.no_grad():
            E.copy_(saved)
    key = "spectral2" if world["specular"] else "spectral"
    a, b = _flat(got[key]).double().cpu(), _flat(swapped[key]).double().cpu()
    assert bool(((a - b).abs() <= 1e-4 * b.abs() + 1e-6).all()), float((a - b).abs().max())
    assert not torch.equal(swapped["seg_probs"], got["seg_probs"]) and torch.equal(got["seg_probs"], plain["seg_probs"])
    again = _render(world)
    assert all(torch.equal(again[k], plain[k]) for k in plain)  # the dictionary is back


def test_the_mixing_term_is_linear_in_the_gains(world):
    model = world["pipe"].model
    gains = (0.4, 1.7, 0.0)
    key = "spectral2" if world["specular"] else "spectral"
    with _spy_remix() as calls:
        whole = _render(world, _edits(world, {"materials": [{"material": c, "gain": g} for c, g in enumerate(gains)]}))
        parts = [_render(world, _edits(world, {"materials": [{"material": k, "gain": 1.0 if k == c else 0.0} for k in range(3)]}))
                 for c in range(3)]
    assert len(calls) == 4 and all(torch.equal(c["mix"][:, :3], calls[0]["mix"][:, :3]) for c in calls)
    want = sum(float(torch.tensor(g, dtype=torch.float32)) * _flat(p[key]).double().cpu() for g, p in zip(gains, parts))
    # each single-material render and the whole one are within K u of their envelopes, which add up to the whole's; E'' = g E is one
    # more rounding per term
    mag = MF.remix_envelopes(calls[0]["mix"], calls[0]["E"], None, 1.0)["spectral"]
    err = (_flat(whole[key]).double().cpu() - want).abs()
    assert bool((err <= (2 * MF.K_REMIX + 1) * MF.U * mag).all()), float((err / (MF.U * mag)).max())
    assert float(want.abs().max()) > 0


def test_all_densities_zero_leave_nothing(world):
    from umhsnerf import _hip, ops

    model = world["pipe"].model
    plain = _render(world)
    got = _render(world, _edits(world, {"materials": [{"material": c, "density": 0.0} for c in range(3)]}))
    assert list(got) == list(plain) and float(plain["accumulation"].max()) > 0
    for k in ("accumulation", "spectral", "abundances"):
        print(k, float(got[k].abs().max()))
    for k in ("accumulation", "spectral", "abundances"):
        assert bool((got[k] == 0).all()), (k, float(got[k].abs().max()))
    zero_rgb = ops.spec2rgb_fwd(torch.zeros(4, 8, device=DEV), _hip.f32c(model.converter.transform_matrix))
    assert torch.equal(_flat(got["rgb"]), zero_rgb[:1].expand(H * W, 3))
    assert torch.equal(got["num_samples_per_ray"], plain["num_samples_per_ray"])


def _samples(world, camera=1):
    from umhsnerf._ns_compat import RayBundle

    model = world["pipe"].model
    rb = world["cameras"].generate_rays(camera, keep_shape=True)
    rays = RayBundle(origins=rb.origins.reshape(-1, 3), directions=rb.directions.reshape(-1, 3))
    with torch.no_grad():
        return model.sample(rays)


def test_removing_a_material_equals_the_float64_edited_render(world):
    """The order of operations end to end: abundances from the unedited pass, weights from the edited density, segmentation against
    the model's own dictionary.  Every output within 1e-4 |ref| + 1e-6 of tests/material_f64.edited_render in float64 on the same
    samples.  seg_raw may differ where the float64 argmax is tied within EDGE (rays_f64.cluster_ties) or the float64 accumulation is
    within its own tolerance of the 0.5 threshold; at most 2 % of the rays, asserted on the float64 run alone."""
    model = world["pipe"].model
    removed = 1
    edits = _edits(world, {"materials": [{"material": removed, "density": 0.0}]})
    ray_samples, ray_indices = _samples(world)
    R = H * W
    with torch.no_grad(), model.material_edits_context(edits):
        got = model.get_outputs_from_samples(ray_samples, ray_indices, R)
    with torch.no_grad():
        plain = model.get_outputs_from_samples(ray_samples, ray_indices, R)
    assert list(got) == list(plain) and not torch.equal(got["accumulation"], plain["accumulation"])
    assert bool((got["accumulation"] <= plain["accumulation"] + 1e-4).all())  # (a float32 sum of up to ~1000 weights: S u < 1e-4)
    fr = ray_samples.frustums
    p = MF.field_params_of(model.field)
    E = model.field.endmembers.detach()
    ref = MF.edited_render(p, edits.dictionary(E), edits.density_gain("cpu"), edits.specular_gain, fr.origins, fr.directions, fr.starts,
                           fr.ends, ray_indices, R, 0.4, model.converter.transform_matrix, contraction=model.field.spatial_distortion is not None)
    keys = ["accumulation", "depth", "spectral", "rgb", "abundances", "seg_probs", "weights"] + (["spectral2", "specular"] if world["specular"] else [])
    worst = {}
    for k in keys:
        a, b = got[k].double().cpu().reshape(ref[k].shape), ref[k].double()
        tol = 1e-4 * b.abs() + 1e-6
        worst[k] = float(((a - b).abs() / tol).max())
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    # seg_raw
    acc64 = ref["accumulation"].reshape(-1)
    tied = MF.cluster_ties(ref["unedited_spectral"], E.double().cpu())[2].sum(1) > 1
    edge = (acc64 - 0.5).abs() <= 1e-4 * 0.5 + 1e-6
    left_out = tied | edge
    assert float(left_out.double().mean()) <= 0.02
    same = got["seg_raw"].reshape(-1).double().cpu() == ref["seg_raw"].reshape(-1)
    assert bool((same | left_out).all()), int((~same & ~left_out).sum())
    assert float(acc64.max()) > 0.01 and int((plain["num_samples_per_ray"] > 0).sum()) > R // 4


def test_the_context_is_gone_after_the_block_returns_or_raises_and_refuses_what_it_cannot_do(world):
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model = world["pipe"].model
    edits = _edits(world, _recolour_doc(world))
    other = _edits(world, {"materials": [{"material": 0, "density": 0.5}]})
    plain = _render(world)
    with model.material_edits_context(edits):
        assert model._material_edits is edits
        with model.material_edits_context(other):
            assert model._material_edits is other
        with model.material_edits_context(None):
            assert model._material_edits is None
        assert model._material_edits is edits
    assert model._material_edits is None
    with pytest.raises(KeyError):
        with model.material_edits_context(edits):
            raise KeyError("inside")
    assert model._material_edits is None
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    flat = type(rb)(origins=rb.origins.reshape(-1, 3), directions=rb.directions.reshape(-1, 3))
    # gradients enabled
    with pytest.raises(NotImplementedError, match="gradient-free"):
        with model.material_edits_context(edits):
            model(flat)
    assert model._material_edits is None
    # training mode
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="gradient-free"):
            with torch.no_grad(), model.material_edits_context(edits):
                model(flat)
    finally:
        model.eval()
    assert model._material_edits is None
    # built for another model
    with pytest.raises(ValueError, match="built for"):
        with model.material_edits_context(_edits(dict(world, specular=not world["specular"]), {"materials": [{"material": 0, "gain": 2.0}]})):
            pass
    after = _render(world)
    assert all(torch.equal(after[k], plain[k]) for k in plain)
    if world["specular"]:  # method="rgb": no dictionary to edit; None is still the plain path there
        rgb_model = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": list(range(8)), "num_classes": 3}).to(DEV)
        from umhsnerf.materials import MaterialEdits

        with pytest.raises(NotImplementedError, match="rgb"):
            with rgb_model.material_edits_context(MaterialEdits(3, 8, False, (None,) * 3, (2.0, 1.0, 1.0), (1.0,) * 3)):
                pass
        with rgb_model.material_edits_context(None):
            pass
        assert rgb_model._material_edits is None


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path))


def _common(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *world["flags"]]


def test_camera_path_with_material_edits_and_a_crop(world_spec, capsys):
    from umhsnerf import render

    world = world_spec
    root, model = world["root"], world["pipe"].model
    doc = _recolour_doc(world)
    doc["materials"].append({"material": 1, "density": 0.25})
    (root / "edits.json").write_text(json.dumps(doc))
    names = ["rgb", "wv_2", "accumulation"]
    capsys.readouterr()
    got = render.main(["camera-path", *_common(world), "--camera-path-filename", str(root / "path.json"), "--output-path", str(root / "edited"),
                       "--rendered-output-names", *names, "--material-edits", str(root / "edits.json")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and got["material_edits"] == str(root / "edits.json") and got["frames"] == 3
    bare = render.main(["camera-path", *_common(world), "--camera-path-filename", str(root / "path.json"), "--output-path", str(root / "bare"),
                        "--rendered-output-names", *names])
    assert "material_edits" not in bare
    edits = _edits(world, doc)
    for i in range(3):
        with model.material_edits_context(edits):
            outputs = model.get_outputs_for_camera_ray_bundle(world["cameras"].generate_rays(i, keep_shape=True))
        want = render.compose_frame(outputs, names).cpu().numpy()
        frame = _png(root / "edited" / f"frame_{i:05d}.png")
        assert np.array_equal(frame, want)
        assert not np.array_equal(frame, _png(root / "bare" / f"frame_{i:05d}.png"))
    # with a crop: the background colour still shows where nothing is hit, in either nesting order of the two contexts
    (root / "crop_path.json").write_text(json.dumps(dict(world["path"], crop=CROP)))
    render.main(["camera-path", *_common(world), "--camera-path-filename", str(root / "crop_path.json"), "--output-path", str(root / "cropped"),
                 "--rendered-output-names", "rgb", "--material-edits", str(root / "edits.json")])
    crop = render.parse_crop(CROP)
    rb = world["cameras"].generate_rays(0, keep_shape=True, obb_box=crop["obb"], near_floor=float(model.config.near_plane))
    miss = (rb.nears == 1e10).view(H, W).cpu().numpy()
    frame = _png(root / "cropped" / "frame_00000.png")
    assert 10 < miss.sum() < H * W - 10 and (frame[miss] == np.array([38, 120, 255])).all()
    with model.material_edits_context(edits), model.background_color_override_context(crop["background_color"]):
        a = model.get_outputs_for_camera_ray_bundle(rb)
    with model.background_color_override_context(crop["background_color"]), model.material_edits_context(edits):
        b = model.get_outputs_for_camera_ray_bundle(rb)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert np.array_equal(frame, render.compose_frame(a, ["rgb"]).cpu().numpy())
    assert model._material_edits is None and model._background_override is None


def test_bad_edit_files_are_refused_before_anything_is_rendered(world_spec, monkeypatch):
    from umhsnerf import export, render

    world = world_spec
    root = world["root"]
    (root / "bad.json").write_text(json.dumps({"materials": [{"material": 3, "gain": 2.0}]}))

    def never(*a, **k):
        raise AssertionError("rendering started")

    for mod, names in ((render, ("render_camera_path", "render_dataset")), (export, ("export_pointcloud", "export_tsdf_mesh"))):
        for name in names:
            monkeypatch.setattr(mod, name, never)
    for argv in (["camera-path", "--camera-path-filename", str(root / "path.json"), "--output-path", str(root / "no")],
                 ["dataset", "--output-path", str(root / "no")], ["interpolate", "--output-path", str(root / "no")]):
        with pytest.raises(ValueError, match=r"entry 0: material 3 is outside 0\.\.2"):
            render.main([*argv, *_common(world), "--material-edits", str(root / "bad.json")])
    for sub in ("pointcloud", "tsdf"):
        with pytest.raises(ValueError, match=r"entry 0: material 3 is outside 0\.\.2"):
            export.main([sub, *_common(world), "--output-dir", str(root / "no"), "--material-edits", str(root / "bad.json")])
    assert not (root / "no").exists()


def _tsdf(world):
    return ["tsdf", *_common(world), "--resolution", "24", "--downscale-factor", "1", "--batch-size", "4"]


def test_exports_run_under_material_edits_and_report_the_file(world_spec, capsys):
    import mesh_ref as M
    from umhsnerf import export

    world = world_spec
    root = world["root"]
    (root / "dim.json").write_text(json.dumps({"materials": [{"material": 2, "density": 0.0}]}))
    plain = export.main([*_tsdf(world), "--output-dir", str(root / "mesh_plain")])
    capsys.readouterr()
    got = export.main([*_tsdf(world), "--output-dir", str(root / "mesh_dim"), "--material-edits", str(root / "dim.json")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and got["material_edits"] == str(root / "dim.json")
    assert "material_edits" not in plain and 0 < got["vertices"] < plain["vertices"]  # less matter: a smaller surface
    assert len(M.read_mesh_ply(got["file"])[0]) == got["vertices"]
    pc = export.main(["pointcloud", *_common(world), "--output-dir", str(root / "pc_dim"), "--num-points", "2000", "--num-rays-per-batch",
                      "4096", "--opacity-threshold", "0.05", "--material-edits", str(root / "dim.json")])
    assert pc["material_edits"] == str(root / "dim.json") and pc["points"] > 0 and (root / "pc_dim" / "point_cloud.ply").exists()
    assert world["pipe"].model._material_edits is None


def _unmixed_checkpoint(world):
    """A checkpoint and model flags of an UNMIXED scene, made from the trained one without the specular head (geometry and scalars
    as trained).  The dictionary gets well-separated rows (0.9 on two bands of its own, 0.05 elsewhere: the cosine between two rows
    is 0.12).  The abundance head is written by hand: its logits are (relu(p), relu(-p), 0) with p the first component of the
    position encoding, a sine of one world coordinate, so the scene is cut into slabs of material 0 and material 1; at the softmax
    temperature 0.01 a sample is one-hot wherever |p| > 0.05, and material 2 has a share only in the thin shells between slabs."""
    root, pipe = world["root"], world["pipe"]
    state = {k: v.detach().clone() for k, v in pipe.state_dict().items()}

    def entry(suffix):
        key = [k for k in state if k.endswith(suffix)]
        assert len(key) == 1, (suffix, key)
        return state[key[0]]

    E = entry("field.endmembers")
    E.fill_(0.05)
    for c in range(3):
        E[c, 2 * c: 2 * c + 2] = 0.9
    for i in range(3):
        entry(f"field.feature_mlp.layers.{i}.weight").zero_()
        entry(f"field.feature_mlp.layers.{i}.bias").zero_()
    w0, w1, w2 = (entry(f"field.feature_mlp.layers.{i}.weight") for i in range(3))
    assert tuple(w0.shape) == (64, 27) and tuple(w1.shape) == (64, 64) and tuple(w2.shape) == (3, 64)
    w0[0, 0], w0[1, 0] = 1.0, -1.0
    w1[0, 0] = w1[1, 1] = 1.0
    w2[0, 0] = w2[1, 1] = 1.0
    torch.save({"step": 3, "pipeline": state}, root / "unmixed.ckpt")
    return ["--data", str(world["scene"]), "--checkpoint", str(root / "unmixed.ckpt"), "--num-classes", "3", "--temperature", "0.01",
            "--background-color", "black"]


def test_a_mesh_with_a_material_removed_does_not_carry_its_label(world_plain):
    """``export tsdf --material-edits`` with material K removed: no vertex carries the label K.  K is the label most vertices of the
    UNEDITED mesh carry (a label that does not occur anyway would prove nothing).

    The scene is ``_unmixed_checkpoint``: what the statement is about.  A vertex's label is the argmax of the fused ``seg_probs``, the
    cosine between the unedited composited spectrum and the model's own dictionary, while a removal scales a sample's density by
    1 - a_K.  Where a_K is 0 or 1 per sample, what is left holds no share of E_K, and with rows a cosine of 0.12 apart a spectrum mixed
    from the other rows cannot be nearest to E_K.  On a MIXED scene the statement does not hold and is not meant to: on
    the three-step scene as trained (temperature 0.4, abundances near 1/3) removing material 2 takes a third of every sample's density
    and leaves its spectrum as it was -- measured on an MI355X: 8226 vertices, all labelled 2, become 515, all still labelled 2.
    On the unmixed scene: labels [11471, 873, 0] become [0, 911, 0] with material 0 removed."""
    import mesh_ref as M
    from umhsnerf import export

    world = world_plain
    root = world["root"]
    tsdf = ["tsdf", *_unmixed_checkpoint(world), "--resolution", "24", "--downscale-factor", "1", "--batch-size", "4"]
    plain = export.main([*tsdf, "--output-dir", str(root / "mesh_unedited")])
    table, _, _ = M.read_mesh_ply(plain["file"])
    counts = np.bincount(table["material"] + 1, minlength=4)[1:]
    K = int(counts.argmax())
    assert counts[K] > 0
    (root / "remove.json").write_text(json.dumps({"materials": [{"material": K, "density": 0.0}]}))
    got = export.main([*tsdf, "--output-dir", str(root / "mesh_removed"), "--material-edits", str(root / "remove.json")])
    edited, _, _ = M.read_mesh_ply(got["file"])
    after = np.bincount(edited["material"] + 1, minlength=4)[1:]
    print(f"labels of the unedited mesh {counts.tolist()}, with material {K} removed {after.tolist()}")
    assert after[K] == 0
    assert after.sum() > 0  # the slabs of the other material are still there
