"""Sparse unmixing on the GPU: csrc/umhs_sparse.hip per row against the float64 truth (tests/sparse_f64.py), the properties that hold by
construction, the outputs of ``UMHSModel.sparse_unmixing_context`` on the small trained pipeline of tests/test_hip_library.py
(``make_scene(B=8)``, 3 classes, 20 x 28 path frames), and ``--sparse-unmix`` on the command lines."""
import json
import os

import numpy as np
import pytest
import torch

import rays_f64 as RF
import sparse_f64 as SF
import unmix_f64 as UF
from test_hip_library import BASE_FLAGS, CROP, H, W, world  # noqa: F401  (the fixture: the module's own copy of the small pipeline)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}


def _report(key, report):
    _WORST[key] = report
    with open(os.path.join(RF.report_dir(ROOT), "sparse_f64.json"), "w") as f:
        json.dump(_WORST, f, indent=1)


def _device_rows(case):
    """The case's rows on the device in the case's own layout (a slice case: a column slice of the wider array, read in place)."""
    wide = torch.from_numpy(case["wide"]).to(DEV)
    return wide[:, SF.SLICE_AT:SF.SLICE_AT + case["B"]] if case["layout"] == "slice" else wide


_OPERANDS = {}


def _operands(A, lam=SF.LAMBDA, mu=None):
    from umhsnerf import ops

    key = (A.tobytes(), A.shape, lam, mu)
    if key not in _OPERANDS:
        _OPERANDS[key] = ops.sparse_prepare(torch.from_numpy(A).to(DEV), lam, SF.auto_mu(A) if mu is None else mu)
    return _OPERANDS[key]


def _sparse(case, rows, **kw):
    from umhsnerf import ops

    kw = dict(dict(epsilon=case["eps"], max_iterations=case["max_iterations"], want_residual=True, want_status=True), **kw)
    return ops.sparse_unmix(rows, _operands(case["A"], case["lam"], case["mu"]), **kw)


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------ #
# kernel
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("c", SF.CASES, ids=SF.sparse_id)
def test_sparse_unmix_is_within_the_bounds_of_float64_and_repeats_bit_for_bit(c):
    case, ref = SF.reference(*c)
    rows = _device_rows(case)
    if case["layout"] == "slice":
        assert rows.stride(0) == case["B"] + SF.SLICE_PAD and rows.data_ptr() % 16 != 0
    a, res, status = _sparse(case, rows)
    assert tuple(a.shape) == (case["R"], case["L"]) and tuple(res.shape) == tuple(status.shape) == (case["R"],)
    assert a.dtype == res.dtype == torch.float32 and status.dtype == torch.int32
    report = {}
    fails = SF.check(case, a.cpu().numpy(), res.cpu().numpy(), status.cpu().numpy(), report)
    print(SF.sparse_id(c), {k: round(v, 4) for k, v in report.items()})
    _report(SF.sparse_id(c), report)
    assert not fails, fails
    assert all(v < 1.0 for k, v in report.items() if k != "cap_share")
    for x, y in zip((a, res, status), _sparse(case, rows)):  # the same bits on a second run
        assert torch.equal(_bits(x), _bits(y))
    if case["layout"] == "slice":  # a view gives the bits of its contiguous copy
        for x, y in zip((a, res, status), _sparse(case, rows.contiguous())):
            assert torch.equal(_bits(x), _bits(y))
    if case["R"] == 0:
        return
    only, none_r, none_s = _sparse(case, rows, want_residual=False, want_status=False)  # without the optional outputs
    assert none_r is None and none_s is None and torch.equal(_bits(only), _bits(a))


def test_the_kernel_follows_the_float32_restatement():
    """Not a rule (the chains of numpy and of the matrix core may differ in the last bit), but the iteration counts of the two must
    agree on nearly every row: a kernel that walked j in another order, or froze late, would not."""
    for c in (SF.CASES[3], SF.CASES[6]):
        case, _ = SF.reference(*c)
        _, _, status = _sparse(case, _device_rows(case))
        _, _, want = SF.solve_f32(case["A"], case["x"])
        status = status.cpu().numpy()
        assert (np.abs(status - want) <= 1).mean() >= 0.9, (SF.sparse_id(c), status, want)
        assert np.array_equal(status == -1, want == -1)


def test_a_row_alone_gives_its_bits_in_the_batch():
    for c in (SF.CASES[5], SF.CASES[8], SF.CASES[11]):  # T = 2, T = 4 on 256 bands, the hotdog slice (T = 1)
        case, _ = SF.reference(*c)
        rows = _device_rows(case)
        a, res, status = _sparse(case, rows)
        for r in (0, 31, 32, 33, 63, 64, case["R"] - 1):
            for x, y in zip((a, res, status), _sparse(case, rows[r:r + 1])):
                assert torch.equal(_bits(x[r:r + 1]), _bits(y)), (SF.sparse_id(c), r)
        # and a batch that starts elsewhere: the bits do not depend on the row's place in its wave or workgroup
        for x, y in zip((a, res, status), _sparse(case, rows[7:])):
            assert torch.equal(_bits(x[7:]), _bits(y))


def test_no_rows_and_the_ops_refusals():
    from umhsnerf import ops

    case, _ = SF.reference(*SF.CASES[10])  # R = 0
    a, res, status = _sparse(case, _device_rows(case))
    assert tuple(a.shape) == (0, 6) and tuple(res.shape) == (0,) and tuple(status.shape) == (0,)
    A = torch.from_numpy(SF.library("syn", 6, 31)).to(DEV)
    operands = ops.sparse_prepare(A, 1e-3, 0.5)
    assert (operands.L, operands.B, operands.mu, operands.lambda_) == (6, 31, 0.5, 1e-3) and operands.theta == float(np.float32(2e-3))
    x = torch.rand(5, 31, device=DEV)
    with pytest.raises(ValueError, match="bands"):
        ops.sparse_unmix(torch.rand(5, 33, device=DEV), operands)
    with pytest.raises(ValueError, match="epsilon"):
        ops.sparse_unmix(x, operands, epsilon=0.0)
    with pytest.raises(ValueError, match="max_iterations"):
        ops.sparse_unmix(x, operands, max_iterations=0)
    with pytest.raises(ValueError, match="sparse_prepare"):
        ops.sparse_unmix(x, (A, A))
    with pytest.raises(ValueError, match="float32"):
        ops.sparse_unmix(x.double(), operands)
    with pytest.raises(ValueError, match="limits"):
        ops.sparse_prepare(torch.rand(129, 140, device=DEV), 1e-3, 0.5)
    with pytest.raises(ValueError, match="limits"):
        ops.sparse_prepare(torch.rand(5, 257, device=DEV), 1e-3, 0.5)
    with pytest.raises(ValueError, match="lambda"):
        ops.sparse_prepare(A, -1.0, 0.5)
    with pytest.raises(ValueError, match="mu"):
        ops.sparse_prepare(A, 1e-3, 0.0)
    bad = A.clone()
    bad[2, 3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ops.sparse_prepare(bad, 1e-3, 0.5)


# ------------------------------------------------------------------------------------------------------------------------------ #
# properties
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_a_penalty_above_every_correlation_gives_all_zeros():
    """max_k b_k <= lambda_r: the zero vector is optimal (the truth says so), and the kernel returns exact zeros: z' is +0 from the
    first iteration on.  The status is NOT 1: a_1 = c is not zero, so |a - z'| <= epsilon max|c| cannot hold at iteration 1, and under
    so large a penalty a settles slowly (the float32 restatement runs these rows to the cap); any count or -2 is accepted."""
    from umhsnerf import ops

    case, _ = SF.reference(*SF.CASES[5])
    v = case["valid"]
    x64, A64 = case["x"][v].astype(np.float64), case["A"].astype(np.float64)
    lam = 1.01 * float(((x64 @ A64.T).max(1) / np.sqrt((x64 * x64).sum(1))).max())
    truth, _, _ = SF.solve_f64(case["A"], case["x"], lam)
    assert (truth == 0).all()
    a, res, status = ops.sparse_unmix(_device_rows(case), _operands(case["A"], lam), want_status=True)
    a, status = a.cpu().numpy(), status.cpu().numpy()
    assert (a == 0).all() and not np.signbit(a).any()
    assert (((status[v] >= 1) & (status[v] <= SF.MAX_ITERATIONS)) | (status[v] == -2)).all() and (status[~v] == -1).all()
    ss = (x64 * x64).sum(1)
    assert np.abs(res.cpu().numpy()[v].astype(np.float64) - ss).max() <= 4 * 256 * UF.U * ss.max()  # the residual of nothing is ss


def test_lambda_zero_agrees_with_nnls_on_a_well_conditioned_set():
    """lambda = 0 is NNLS: against ``ops.unmix`` on K = 15 endmembers, within the sum of both abundance bounds."""
    from umhsnerf import ops

    case, ref = UF.reference(*UF.CASES[5], UF.NNLS)  # syn-K15-B50-R129
    E, rows = case["E"], torch.from_numpy(case["wide"]).to(DEV)
    want, _, _ = ops.unmix(rows, ops.library_prepare(torch.from_numpy(E).to(DEV)), torch.from_numpy(case["G"]).to(DEV), 15, ops.UNMIX_NNLS)
    a, _, status = ops.sparse_unmix(rows, _operands(E, 0.0), want_status=True)
    v = case["valid"]
    a, want, star = a.cpu().numpy()[v].astype(np.float64), want.cpu().numpy()[v].astype(np.float64), ref["a"][v]
    x64, E64 = case["x"][v].astype(np.float64), E.astype(np.float64)
    norm = np.sqrt((x64 * x64).sum(1))
    cond = np.array([np.linalg.cond(E64[s > 0]) ** 2 if (s > 0).any() else 1.0 for s in star])
    bound_sparse = SF.K_A * (SF.EPSILON + 15 * SF.U) * cond * norm / np.linalg.norm(E64, 2)
    bound_unmix = UF.K_A * UF.U * case["cond"] * np.maximum(1.0, np.abs(star).max(1))
    ratio = (np.abs(a - want).max(1) / (bound_sparse + bound_unmix)).max()
    print("lambda = 0 against NNLS:", ratio, "of the sum of the bounds; cap share", (status.cpu().numpy()[v] == -2).mean())
    assert ratio <= 1.0


def test_rows_mixed_from_three_of_64_entries_recover_the_dominant_entry():
    from umhsnerf import ops

    A = SF.library("syn", 64, 128)
    g = np.random.default_rng(5)
    R = 96
    truth_a = np.zeros((R, 64))
    for r in range(R):
        truth_a[r, g.choice(64, 3, replace=False)] = (0.7, 0.2, 0.1)
    x = (truth_a @ A.astype(np.float64) + SF.SIGMA * g.standard_normal((R, 128))).astype(np.float32)
    star, _, _ = SF.solve_f64(A, x)
    assert (star.argmax(1) == truth_a.argmax(1)).all()  # the optimum itself names the dominant entry on these rows
    limit = int((star > 0).sum(1).max()) + 2  # (the stopping rule may leave an entry or two of size epsilon alive)
    a, _, _ = ops.sparse_unmix(torch.from_numpy(x).to(DEV), _operands(A))
    a = a.cpu().numpy()
    count = (a > 0).sum(1)
    print("count: truth mean", (star > 0).sum(1).mean(), "max", (star > 0).sum(1).max(), "kernel mean", count.mean(), "max", count.max())
    assert (a.argmax(1) == truth_a.argmax(1)).all()
    assert count.max() <= limit and count.mean() <= (star > 0).sum(1).mean() + 1


def test_scaling_a_row_by_four_scales_its_abundances_by_exactly_four():
    case, _ = SF.reference(*SF.CASES[6])
    rows = _device_rows(case)
    a, res, status = _sparse(case, rows)
    a4, res4, status4 = _sparse(case, rows * 4.0)
    v = torch.from_numpy(case["valid"] & (np.abs(case["x"]).max(1) < 1e30)).to(DEV)
    assert torch.equal(_bits(a4[v]), _bits(a[v] * 4.0)) and torch.equal(status4[v], status[v])
    assert torch.equal(_bits(res4[v]), _bits(res[v] * 16.0))


# ------------------------------------------------------------------------------------------------------------------------------ #
# model
# ------------------------------------------------------------------------------------------------------------------------------ #
L_WORLD = 32  # the fixture's library: the model's 3 endmembers and 29 distractors, on 8 bands


def _frame(world, unmixer=None, camera=1, output_names=None, crop=False):
    from umhsnerf.render import parse_crop

    model = world["pipe"].model
    if crop:
        rb = world["cameras"].generate_rays(camera, keep_shape=True, obb_box=parse_crop(CROP)["obb"], near_floor=model.config.near_plane)
    else:
        rb = world["cameras"].generate_rays(camera, keep_shape=True)
    with model.sparse_unmixing_context(unmixer):
        return model.get_outputs_for_camera_ray_bundle(rb, output_names=output_names)


def _names(L=L_WORLD):
    from umhsnerf.sparse import sparse_outputs

    return sparse_outputs(L)


def test_the_context_outputs_are_ops_sparse_unmix_of_the_frames_spectral(world):
    from umhsnerf import ops
    from umhsnerf.sparse import SparseUnmixer

    model = world["pipe"].model
    u = SparseUnmixer(world["library"])
    assert len(u) == L_WORLD and u.bands == 8 and u.names == world["library"].names and u.mu_rule == "auto"
    assert u.mu == SF.auto_mu(u.spectra) and np.array_equal(u.spectra, world["library"].spectra.astype(np.float32))
    seen = {"rendered": 0, "empty": 0}
    for camera, crop in [(c, k) for c in range(3) for k in (False, True)]:  # (through a crop box: rays that accumulate <= 0.5)
        plain = _frame(world, camera=camera, crop=crop)
        assert not any(k in plain for k in _names())
        got = _frame(world, u, camera=camera, crop=crop)
        assert [k for k in got if k not in _names()] == list(plain) and all(k in got for k in _names())
        for k in plain:
            assert torch.equal(got[k], plain[k]), k
        operands, colors = u.on(DEV)
        a, res, status = ops.sparse_unmix(got["spectral"], operands, u.epsilon, u.max_iterations, want_status=True)
        rendered = (got["accumulation"].reshape(-1) > 0.5) & (status != -1)
        a = torch.where(rendered[:, None], a, torch.zeros_like(a))
        assert torch.equal(got["sparse"].reshape(-1, L_WORLD), a) and tuple(got["sparse"].shape) == (H, W, L_WORLD)
        assert torch.equal(got["sparse"], torch.cat([got[f"sparse_{k}"] for k in range(L_WORLD)], -1))  # the cube is the stacked panels
        count = (a > 0).sum(1)
        assert torch.equal(got["sparse_count"].reshape(-1), count.float())
        named = rendered & (count > 0)
        raw = got["sparse_raw"].reshape(-1)
        assert torch.equal(raw == -1, ~named) and torch.equal(raw[named].long(), a[named].argmax(1))
        assert torch.equal(got["sparse_pred"].reshape(-1, 3)[named], colors[raw[named].long()])
        assert bool((got["sparse_pred"].reshape(-1, 3)[~named] == 0).all()) and bool((got["sparse"].reshape(-1, L_WORLD)[~rendered] == 0).all())
        want = torch.where(rendered, torch.sqrt(res / 8.0), torch.zeros_like(res))
        assert torch.equal(got["sparse_residual"].reshape(-1), want)
        seen["rendered"] += int(rendered.sum())
        seen["empty"] += int((~rendered).sum())
    assert seen["rendered"] > 100 and seen["empty"] > 100
    # computed only when asked for
    assert sorted(_frame(world, u, output_names=["rgb", "depth"])) == ["depth", "rgb"]
    some = _frame(world, u, output_names=["sparse_pred", "sparse_1"])
    full = _frame(world, u)
    assert sorted(some) == ["sparse_1", "sparse_pred"] and torch.equal(some["sparse_1"], full["sparse_1"])
    assert model._sparse_unmixer is None


def test_under_material_edits_the_edited_spectrum_is_unmixed(world):
    from umhsnerf.materials import load_material_edits
    from umhsnerf.sparse import SparseUnmixer

    model = world["pipe"].model
    u = SparseUnmixer(world["library"])
    edits = load_material_edits({"materials": [{"material": 2, "spectrum": [0.9, 0.05, 0.7, 0.1, 0.6, 0.2, 0.8, 0.3]}]}, 3, 8, False)
    rb = world["cameras"].generate_rays(1, keep_shape=True)
    with model.material_edits_context(edits), model.sparse_unmixing_context(u):
        got = model.get_outputs_for_camera_ray_bundle(rb)
    plain = _frame(world, u)
    assert not torch.equal(got["spectral"], plain["spectral"])
    want = u.frame_outputs(got["spectral"], got["accumulation"])
    for k in _names():
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["sparse"], plain["sparse"])


def test_a_subset_of_entries_and_the_refusals_of_the_unmixer(world):
    from umhsnerf.library import SpectralLibrary
    from umhsnerf.sparse import SparseUnmixer

    lib = world["library"]
    sub = SparseUnmixer(lib, ["endmember_2", 5, "endmember_0"], lambda_=0.0, mu=0.25)
    assert sub.names == ["endmember_2", lib.names[5], "endmember_0"] and (sub.mu, sub.mu_rule, sub.lambda_) == (0.25, "given", 0.0)
    assert np.array_equal(sub.colors, lib.colors[[2, 5, 0]])
    got = _frame(world, sub, output_names=["sparse", "sparse_raw"])
    assert tuple(got["sparse"].shape) == (H, W, 3) and float(got["sparse_raw"].max()) <= 2
    with pytest.raises(ValueError, match="3 library entries"):
        _frame(world, sub, output_names=["sparse_3"])
    with pytest.raises(ValueError, match="no entry named"):
        SparseUnmixer(lib, ["endmember_2", "nothing"])
    with pytest.raises(ValueError, match="twice"):
        SparseUnmixer(lib, ["endmember_2", 2])
    big = SpectralLibrary([f"e{i}" for i in range(129)], np.random.default_rng(0).uniform(0.1, 1, (129, 8)), world["wl"])
    with pytest.raises(ValueError, match=r"1\.\.128.*--sparse-entries"):
        SparseUnmixer(big)
    assert len(SparseUnmixer(big, list(range(128)))) == 128


def test_refusals_and_the_state_after_an_exception(world):
    from umhsnerf.library import SpectralLibrary
    from umhsnerf.sparse import SparseUnmixer
    from umhsnerf.umhs_model import UMHSConfig, UMHSModel

    model = world["pipe"].model
    u = SparseUnmixer(world["library"])
    rgb = UMHSModel(UMHSConfig(method="rgb", background_color="black"), metadata={"wavelengths": world["wl"], "num_classes": 3}, seed=1)
    with pytest.raises(NotImplementedError, match="spectral method"):
        with rgb.sparse_unmixing_context(u):
            pass
    rb = world["cameras"].generate_rays(0, keep_shape=True)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="model.eval"):
            with model.sparse_unmixing_context(u):
                model.get_outputs_for_camera_ray_bundle(rb)
    finally:
        model.eval()
    assert model._sparse_unmixer is None
    with pytest.raises(KeyError):
        with model.sparse_unmixing_context(u):
            assert model._sparse_unmixer is u
            raise KeyError("inside")
    assert model._sparse_unmixer is None
    other = SpectralLibrary(["a", "b"], np.random.default_rng(0).uniform(0.1, 1, (2, 5)), [400.0, 450.0, 500.0, 550.0, 600.0])
    with pytest.raises(ValueError, match="wavelengths"):
        with model.sparse_unmixing_context(SparseUnmixer(other)):
            pass
    with pytest.raises(ValueError, match="bands"):
        u.frame_outputs(torch.rand(4, 5, device=DEV), None)


# ------------------------------------------------------------------------------------------------------------------------------ #
# command lines
# ------------------------------------------------------------------------------------------------------------------------------ #
def _model_flags(world):
    return ["--data", str(world["scene"]), "--checkpoint", str(world["root"] / "step-000000003.ckpt"), *BASE_FLAGS]


def test_names_without_the_flag_are_refused_while_parsing(world):
    from umhsnerf import render

    for name in ("sparse", "sparse_0", "sparse_raw", "sparse_pred", "sparse_count", "sparse_residual"):
        with pytest.raises(ValueError, match="--sparse-unmix"):
            render.parse_args(["dataset", *_model_flags(world), "--output-path", "out", "--rendered-output-names", "rgb", name])


def test_render_camera_path_with_sparse_unmixing(world, capsys):
    from PIL import Image

    from umhsnerf import render
    from umhsnerf.sparse import SparseUnmixer

    root = world["root"]
    got = render.main(["camera-path", *_model_flags(world), "--camera-path-filename", str(root / "path.json"), "--output-path",
                       str(root / "cli_sparse"), "--sparse-unmix", "--spectral-library", str(root / "library.npz"),
                       "--rendered-output-names", "rgb", "sparse_pred", "sparse_0", "--cube-output-names", "sparse"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got
    assert got["frames"] == 3 and got["panels"] == 3
    u = SparseUnmixer(world["library"])
    assert got["sparse_unmix"] == u.summary() and got["sparse_unmix"]["entries"] == L_WORLD
    frame = np.asarray(Image.open(root / "cli_sparse" / "frame_00001.png"))
    assert frame.shape == (H, 3 * W, 3)
    want = _frame(world, u, camera=1)
    assert np.array_equal(frame[:, W:2 * W], (want["sparse_pred"] * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu().numpy())
    cubes = sorted(p for p in os.listdir(root / "cli_sparse") if p.endswith(".npy"))
    assert len(cubes) == 3
    assert np.array_equal(np.load(root / "cli_sparse" / cubes[1]), want["sparse"].cpu().numpy())
    assert world["pipe"].model._sparse_unmixer is None


def test_eval_with_sparse_unmixing_emits_the_keys_and_the_mean_count_is_numpys(world, capsys):
    from umhsnerf import eval as umhs_eval
    from umhsnerf.sparse import SparseUnmixer

    got = umhs_eval.main([*_model_flags(world), "--sparse-unmix", "--spectral-library", str(world["root"] / "library.npz")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got and "psnr" in got
    keys = ("sparse_top", "sparse_mean_count", "sparse_agreement", "sparse_residual_rendered", "sparse_residual_captured", "sparse_cap_share")
    assert all(k in got for k in keys)
    # the same numbers in numpy, from the same tensors
    pipe = world["pipe"]
    u = SparseUnmixer(world["library"])
    n, count, agree, cap_r, ren_r, capped, mean, active = 0, 0, 0, 0.0, 0.0, 0, np.zeros(L_WORLD), np.zeros(L_WORLD)
    for rb, batch in pipe.datamanager.eval_images():
        with pipe.model.sparse_unmixing_context(u):
            out = pipe.model.get_outputs_for_camera_ray_bundle(rb)
        counted = (out["accumulation"].reshape(-1) > 0.5).cpu().numpy()
        a, res, status = u.unmix(batch["hs_image"].to(DEV).float().reshape(-1, 8), True, True)
        a, res, status = a.double().cpu().numpy(), res.double().cpu().numpy(), status.cpu().numpy()
        rendered = out["sparse"].reshape(-1, L_WORLD).double().cpu().numpy()
        n += int(counted.sum())
        count += int((rendered > 0)[counted].sum())
        mean += rendered[counted].sum(0)
        active += (rendered > 0)[counted].sum(0)
        dominant = np.where((status != -1) & ((a > 0).sum(1) > 0), a.argmax(1), -1)
        agree += int((out["sparse_raw"].reshape(-1).long().cpu().numpy() == dominant)[counted].sum())
        cap_r += np.sqrt(res / 8)[counted].sum()
        ren_r += out["sparse_residual"].reshape(-1).double().cpu().numpy()[counted].sum()
        capped += int((status == -2)[counted].sum())
    assert n > 0
    assert got["sparse_mean_count"] == pytest.approx(count / n, rel=1e-12) and 0 < got["sparse_mean_count"] <= L_WORLD
    assert got["sparse_agreement"] == pytest.approx(agree / n) and 0.0 <= got["sparse_agreement"] <= 1.0
    assert got["sparse_residual_captured"] == pytest.approx(cap_r / n, rel=1e-9)
    assert got["sparse_residual_rendered"] == pytest.approx(ren_r / n, rel=1e-9)
    assert got["sparse_cap_share"] == capped / n
    order = np.argsort(-(mean / n), kind="stable")[:16]
    assert [t["name"] for t in got["sparse_top"]] == [u.names[k] for k in order] and len(got["sparse_top"]) == 16
    assert [t["mean_abundance"] for t in got["sparse_top"]] == pytest.approx(list(mean[order] / n), rel=1e-9)
    assert [t["active_share"] for t in got["sparse_top"]] == pytest.approx(list(active[order] / n), rel=1e-9)
    assert pipe.model._sparse_unmixer is None


def test_the_captured_command_writes_ops_sparse_unmix_of_the_frames(world, capsys):
    from umhsnerf import sparse
    from umhsnerf.sparse import SparseUnmixer

    root, pipe = world["root"], world["pipe"]
    got = sparse.main(["captured", *_model_flags(world), "--spectral-library", str(root / "library.npz"), "--split", "train",
                       "--output-path", str(root / "captured_sparse"), "--sparse-entries", *[str(i) for i in range(3, 23)]])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == got == json.loads((root / "captured_sparse" / "summary.json").read_text())
    stack = pipe.datamanager.train_split.hs_image
    u = SparseUnmixer(world["library"], list(range(3, 23)))
    assert len(got["frames"]) == stack.shape[0] > 0 and [e["name"] for e in got["entries"]] == u.names
    total, active, n, rms = np.zeros(20), np.zeros(20), 0, 0.0
    for i, frame in enumerate(got["frames"]):
        cube = np.load(root / "captured_sparse" / f"{frame['frame']}_sparse.npy")
        a, res, status = u.unmix(stack[i].to(DEV).float(), True, True)
        assert cube.shape == (*stack.shape[1:3], 20) and np.array_equal(cube.reshape(-1, 20), a.cpu().numpy())
        valid = (status != -1).cpu().numpy()
        assert frame["invalid"] == int((~valid).sum()) and frame["capped"] == int((status == -2).sum())
        a64 = a.double().cpu().numpy()[valid]
        total, active, n = total + a64.sum(0), active + (a64 > 0).sum(0), n + int(valid.sum())
        rms += float(np.sqrt(res.double().cpu().numpy() / 8)[valid].sum())
    assert [e["mean_abundance"] for e in got["entries"]] == pytest.approx(list(total / n), rel=1e-9)
    assert [e["active_share"] for e in got["entries"]] == pytest.approx(list(active / n), rel=1e-9)
    assert got["mean_count"] == pytest.approx(active.sum() / n, rel=1e-9) and got["mean_residual"] == pytest.approx(rms / n, rel=1e-9)
