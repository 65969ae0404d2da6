"""Pin oracle/torch_ref.py against fixtures produced by the reference's own code (tests/golden/make_golden.py)."""
import os

import numpy as np
import pytest
import torch

import model_golden as MG
from oracle import torch_ref as T


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


@pytest.mark.parametrize("bands", ["b21", "b31", "b128", "b141"])
def test_g1_colour_system(golden_dir, bands):
    g = _load(golden_dir, "g1_colour.npz")
    M = T.colour_matrix(g[f"{bands}_bands"])
    np.testing.assert_array_equal(M.numpy(), g[f"{bands}_M"])  # same numpy float64 recipe -> bit-exact
    rgb = T.colour_system(torch.from_numpy(g[f"{bands}_spec"]), M)
    np.testing.assert_allclose(rgb.numpy(), g[f"{bands}_rgb"], rtol=0, atol=1e-7)
    assert (g[f"{bands}_rgb"] == 0).any() and (g[f"{bands}_rgb"] == 1).any()  # both clamps exercised


def test_g2_cluster_lookup(golden_dir):
    g = _load(golden_dir, "g2_cluster.npz")
    E = torch.from_numpy(g["endmembers_hotdog"])
    assert E.shape == (4, 141)
    ip, pr = T.cluster_lookup(torch.from_numpy(g["x"]), 0.2, E)
    np.testing.assert_allclose(ip.numpy(), g["ip"], atol=1e-6)
    np.testing.assert_allclose(pr.numpy(), g["probs_a02"], atol=1e-6)
    _, pr2 = T.cluster_lookup(torch.from_numpy(g["x"]), None, E)
    np.testing.assert_array_equal(pr2.numpy(), g["probs_none"])


def test_g3_dense_weights_and_packed_twin(golden_dir):
    g = _load(golden_dir, "g3_weights.npz")
    deltas, dens = torch.from_numpy(g["deltas"]), torch.from_numpy(g["densities"])
    w = T.get_weights_spectral(deltas, dens)
    np.testing.assert_allclose(w.numpy(), g["weights"], rtol=1e-6, atol=1e-30)
    # the packed nerfacc restatement must agree with the reference's dense function on the same rays
    R, S, _ = deltas.shape
    t0 = torch.zeros(R * S)
    t1 = deltas.reshape(-1)
    pinfo = torch.stack([torch.arange(R) * S, torch.full((R,), S)], -1)
    wp, _, _ = T.render_weight_from_density(t0, t1, dens.reshape(-1), pinfo)
    np.testing.assert_allclose(wp.reshape(R, S, 1).numpy(), g["weights"], rtol=1e-5, atol=1e-12)  # cumsum order differs
    assert np.all(g["weights"][0] == 0)  # zero-density ray


@pytest.mark.parametrize("case,C,B,spec", [("c6b31s", 6, 31, True), ("c9b128s", 9, 128, True), ("c4b141n", 4, 141, False)])
def test_g4_field_outputs_and_grads(golden_dir, case, C, B, spec):
    g = _load(golden_dir, f"g4_field_{case}.npz")
    p = T.FieldParams(C, B, spec, log2_hashmap_size=12, seed=0)
    with torch.no_grad():
        for k, v in p.named_parameters():
            v.copy_(torch.from_numpy(g[f"param_{k}"]))
    o, d, s, e = (torch.from_numpy(g[k]) for k in ("origins", "directions", "starts", "ends"))
    temp = float(g["temperature"])
    density, emb, _, _ = T.field_density(p, o, d, s, e)
    outs = T.field_outputs(p, o, d, s, e, emb, temp)
    np.testing.assert_allclose(density.detach().numpy(), g["density"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(emb.detach().numpy(), g["emb"], rtol=1e-6, atol=1e-7)
    for k in ("spectral", "spectral2", "specular", "abundances"):
        if f"out_{k}" in g.files:
            assert tuple(outs[k].shape) == g[f"out_{k}"].shape, k  # reference's [1,N,*] / [N,*] shape quirks
            np.testing.assert_allclose(outs[k].detach().numpy(), g[f"out_{k}"], rtol=1e-5, atol=1e-6, err_msg=k)
    assert ("out_spectral2" in g.files) == spec
    loss = (outs["spectral"] * torch.from_numpy(g["cot_spec"])).sum() + (density * torch.from_numpy(g["cot_den"])).sum()
    names = [k for k, _ in p.named_parameters()]
    grads = torch.autograd.grad(loss, [v for _, v in p.named_parameters()], allow_unused=True)
    for k, gv in zip(names, grads):
        if k == "hash_table":
            rows = g["grad_hash_rows"]
            np.testing.assert_allclose(gv[rows].numpy(), g["grad_hash_vals"], rtol=1e-4, atol=1e-6)
            mask = torch.ones(gv.shape[0], dtype=torch.bool)
            mask[rows] = False
            assert float(gv[mask].abs().max()) == 0.0
        elif f"grad_{k}" in g.files:
            np.testing.assert_allclose(gv.numpy(), g[f"grad_{k}"], rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            assert gv is None or float(gv.abs().max()) == 0.0, k


def test_g5_blend_background(golden_dir):
    g = _load(golden_dir, "g5_blend.npz")
    p, gt = T.blend_background_for_loss(*(torch.from_numpy(g[k]) for k in ("pred", "acc", "gt", "bg")))
    np.testing.assert_allclose(p.numpy(), g["pred_out"], atol=1e-7)
    np.testing.assert_array_equal(gt.numpy(), g["gt_out"])


def test_scalings_float32_quirk():
    s = T.hash_scalings()
    assert s.dtype == torch.float32 and s[0] == 16 and s[15] == 2047  # float32 pow: 2047, not 2048


def test_hash_index_uint32_equivalence():
    """int64 product/xor/mod of nerfstudio == uint32 wrap-around arithmetic used by the HIP kernel."""
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2049, size=(1000, 3)).astype(np.int32)
    ref = T.hash_fn(torch.from_numpy(c), 1 << 19, torch.zeros((), dtype=torch.int64)).numpy()
    u = c.astype(np.uint32)
    h = (u[:, 0] * np.uint32(1)) ^ (u[:, 1] * np.uint32(2654435761)) ^ (u[:, 2] * np.uint32(805459861))
    np.testing.assert_array_equal(ref, (h & np.uint32((1 << 19) - 1)).astype(np.int64))


def test_float64_oracle_close_to_float32():
    p32 = T.FieldParams(6, 31, True, log2_hashmap_size=12, table_scale=0.5, seed=3)
    p64 = T.FieldParams(6, 31, True, log2_hashmap_size=12, table_scale=0.5, seed=3, dtype=torch.float64)
    b = T.synthetic_batch(8, 16, 31, seed=5)
    M = T.colour_matrix(np.linspace(400, 700, 31))
    o32 = T.model_outputs(p32, b["origins"], b["directions"], b["starts"], b["ends"], b["ray_indices"], 8, 0.4, M)
    o64 = T.model_outputs(p64, *(b[k].double() for k in ("origins", "directions", "starts", "ends")), b["ray_indices"], 8, 0.4, M)
    np.testing.assert_allclose(o32["spectral"].detach().numpy(), o64["spectral"].detach().numpy(), rtol=2e-4, atol=1e-6)


def test_oracle_marcher_analytic_cases():
    """No reference fixture exists for nerfacc's marcher (CUDA-only, not installable): pin the restatement on closed-form cases."""
    full = np.ones((1, 4, 4, 4), dtype=bool)
    roi = [-1, -1, -1, 1, 1, 1]
    # axis ray through a fully occupied single-level grid: samples tile [t_in, t_out) with constant dt
    ts, te = T.march_ray_ref([-3.0, 0.1, 0.2], [1.0, 0.0, 0.0], full, roi, 0.05, 1e3, 0.125, 0.0)
    ts, te = np.array(ts), np.array(te)
    assert len(ts) == 16 and abs(ts[0] - 2.0) < 1e-6 and abs(te[-1] - 4.0) < 1e-5
    np.testing.assert_allclose(te[:-1], ts[1:], atol=1e-6)  # contiguous while the voxels stay occupied
    # cone angle: dt = max(t*cone, step)
    ts, te = T.march_ray_ref([-3.0, 0.1, 0.2], [1.0, 0.0, 0.0], full, roi, 0.05, 1e3, 0.01, 0.05)
    np.testing.assert_allclose(np.array(te) - np.array(ts), np.maximum(np.array(ts) * 0.05, 0.01), rtol=1e-5)
    # empty grid, ray that misses, far plane before the box
    assert T.march_ray_ref([-3, 0, 0], [1, 0, 0], np.zeros((2, 4, 4, 4), bool), roi, 0.05, 1e3, 0.1, 0.0) == ([], [])
    assert T.march_ray_ref([-3, 5, 0], [1, 0, 0], full, roi, 0.05, 1e3, 0.1, 0.0) == ([], [])
    assert T.march_ray_ref([-3, 0, 0], [1, 0, 0], full, roi, 0.05, 1.5, 0.1, 0.0) == ([], [])
    # a gap of empty voxels restarts the run at the next occupied voxel's entry
    gap = full.copy()
    gap[0, 1:3] = False
    ts, te = T.march_ray_ref([-3.0, 0.1, 0.2], [1.0, 0.0, 0.0], gap, roi, 0.05, 1e3, 0.2, 0.0)
    ts = np.array(ts)
    assert (ts < 2.5).sum() >= 2 and abs(ts[ts >= 2.5][0] - 3.5) < 1e-5
    # two levels: the coarse level takes over outside the roi (voxels twice as large)
    two = np.zeros((2, 4, 4, 4), bool)
    two[1] = True
    ts, te = T.march_ray_ref([-3.0, 0.1, 0.2], [1.0, 0.0, 0.0], two, roi, 0.05, 1e3, 0.25, 0.0)
    ts = np.array(ts)
    assert ts.min() >= 1.0 - 1e-6 and not ((ts > 2.05) & (ts < 3.8)).any() and (ts > 3.9).any()  # [-2,-1] and [1,2] only
    aabbs = T.occ_grid_aabbs(roi, 3)
    np.testing.assert_array_equal(aabbs[2], [-4, -4, -4, 4, 4, 4])


def test_c1_rgb_plumbing_forward_on_cpu():
    """BASELINE config C1 (scripts/rgb.sh shape: method="rgb", 256 rays x 64 samples, forward render on the CPU path) through the
    oracle: field ``umhs_field.py:280-294`` (NerfactoField's mlp_head on [SH(dir) | emb] -> 3 with its Sigmoid) + packed compositing,
    and its loss branch.  (The HIP side of this method is umhs_field_rgb.py, held to the oracle in test_hip_rgb_method.py and
    test_hip_rgb_f64.py; the reference's own run of it is fixture G8 ``rgb_c5b21``.)"""
    R, S = 256, 64
    p = T.FieldParams(5, 21, False, method="rgb", table_scale=0.5, seed=1)
    with torch.no_grad():
        p.base_b[1][0] += 1.0
    b = T.synthetic_batch(R, S, 21, seed=2)
    with torch.no_grad():
        density, emb, sigma_raw, sel = T.field_density(p, b["origins"], b["directions"], b["starts"], b["ends"])
        fo = T.field_outputs(p, b["origins"], b["directions"], b["starts"], b["ends"], emb, 0.5)
        assert set(fo) == {"rgb"} and fo["rgb"].shape == (R * S, 3) and density.shape == (R * S, 1) and emb.shape == (R * S, 15)
        pinfo = T.pack_info(b["ray_indices"], R)
        w = T.render_weight_from_density(b["starts"][..., 0], b["ends"][..., 0], density[..., 0], pinfo)[0]
        rgb = T.accumulate_along_rays(w, fo["rgb"], b["ray_indices"], R)          # upstream NGPModel: per-ray colour
        acc = T.accumulate_along_rays(w, None, b["ray_indices"], R)
        assert rgb.shape == (R, 3) and acc.shape == (R, 1) and torch.isfinite(rgb).all()
        assert float(acc.min()) >= 0 and float(acc.max()) <= 1 + 1e-6 and float(acc.mean()) > 0.05
        # the reference calls renderer_rgb WITHOUT ray_indices/num_rays in this mode (umhs_model.py:266): a packed [N,3] input is then
        # summed over dim -2 into ONE colour for the whole batch (latent bug) -- restated, not imitated by the build
        quirk = torch.sum(w[:, None] * fo["rgb"], dim=-2)
        torch.testing.assert_close(quirk, rgb.sum(0), rtol=1e-4, atol=1e-5)
        loss = T.model_loss({"rgb": rgb, "accumulation": acc}, None, torch.rand(R, 3), b["bg_random"], "rgb")
        assert set(loss) == {"rgb_loss"} and torch.isfinite(loss["rgb_loss"])
    sd = p.reference_state_dict()
    assert sd["mlp_head.layers.0.weight"].shape == (64, 31) and sd["mlp_head.layers.2.weight"].shape == (3, 64)
    assert not any(k.startswith(("feature_mlp", "mlp_directional", "endmembers")) for k in sd)


def test_the_chunked_oracle_step_of_the_full_size_tests_equals_one_call():
    """tests/test_hip_fullsize.py runs the oracle in ray chunks at 8192 rays (it is separable per ray): same outputs, batch losses and
    summed parameter gradients as one call over the whole batch -- checked here on the CPU at a size both forms finish in seconds."""
    import test_hip_fullsize as F

    R, S, B, C = 48, 12, 31, 6
    p = F._bench_state(C, B, True)
    b = T.synthetic_batch(R, S, B, seed=1)
    M = T.colour_matrix(list(np.linspace(400, 700, B)))
    one, many = F._oracle_step(p, b, R, 0.4, M), F._oracle_step_chunked(p, b, R, S, 0.4, M, chunk=16)
    for k in ("spectral", "rgb", "depth", "accumulation", "abundances", "seg_probs", "spectral2", "specular"):
        assert float((one[0][k].detach() - many[0][k]).abs().max()) <= 2e-7, k
    for k in one[1]:
        assert abs(float(one[1][k].detach()) - float(many[1][k])) <= 1e-6 * abs(float(one[1][k].detach())), k
    for name, g1, g2 in zip(one[3], one[5], many[5]):
        assert float((g1 - g2).abs().max()) <= 1e-6 * float(g1.abs().max()) + 1e-12, name


# ------------------------------------------------------------------------------------------------------------------------------ #
# G8: the model level -- the reference's own UMHSModel.get_outputs / get_loss_dict / get_metrics_dict
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("case", MG.SPECTRAL_CASES)
def test_g8_model_matches_the_reference(golden_dir, case):
    """``T.model_outputs`` / ``T.model_loss`` / ``T.psnr`` against what the reference's UMHSModel computed on the same inputs: every
    output (shape included), which outputs carry a gradient, the key set, both losses, all metrics and every parameter gradient
    (untouched hash rows exactly zero).  Tolerances: the G4 test's own."""
    fx = MG.load(golden_dir, case)
    g = fx.g
    # the fixture is conditioned: the labels can be compared exactly, both sides of the 0.5 threshold are populated, gradient
    # scaling is not the identity, and one ray has no sample / one exactly one
    assert g["cond_acc_above"] >= 3 and g["cond_acc_below"] >= 3 and g["cond_acc_min_dist_to_half"] >= 1e-2
    assert g["cond_seg_min_top2_gap"] >= 1e-4 and g["cond_share_t_mid_below_1"] >= 0.1
    counts = g["out_num_samples_per_ray"]
    assert (counts == 0).sum() == 1 and (counts == 1).sum() == 1 and counts.max() <= 24 and counts.sum() == fx.origins.shape[0]
    out, loss, metrics, grads = step = MG.oracle_step(fx)
    # key set: the oracle's keys (without its per-sample ``weights``, which is no output of the reference) + the per-band names
    bands = [f"wv_{i}" for i in range(fx.B)] + [f"abundances_{i}" for i in range(fx.C)] + ([f"residual_{i}" for i in range(fx.B)] if fx.spec else [])
    assert set(out) - {"weights"} | set(bands) == set(fx.output_keys) and len(set(fx.output_keys)) == len(fx.output_keys)
    assert set(loss) == {k[5:] for k in g.files if k.startswith("loss_")}
    assert set(metrics) == {k[7:] for k in g.files if k.startswith("metric_")}
    for k in MG.base_outputs(fx):
        assert tuple(out[k].shape) == g[f"out_{k}"].shape, k
        assert out[k].requires_grad == bool(g[f"rg_{k}"]), k
    ratios = MG.oracle_ratios(fx, step)
    assert {k for k in g.files if k.startswith(("out_", "loss_", "metric_", "grad_")) and k not in ("grad_hash_rows", "grad_hash_vals")} <= set(ratios)
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, over
    # the ray without a sample: nothing accumulated, depth = 0 / 1e-10 clipped up to the batch's smallest t_mid, label 0
    empty = int(np.flatnonzero(counts == 0)[0])
    assert g["out_accumulation"][empty, 0] == 0 and g["out_depth"][empty, 0] == ((fx.starts + fx.ends) / 2).min() and g["out_seg_raw"][empty] == 0


def test_g8_rgb_method_matches_the_reference(golden_dir):
    """Method "rgb" (get_outputs and get_loss_dict only: the reference's get_metrics_dict reads an output that branch never sets).
    Named deviation: the reference composites its rgb WITHOUT ray indices, i.e. one colour [3] summed over every sample of the batch;
    the oracle (and the build) composite per ray.  The fixture's colour is the sum of the oracle's per-ray colours, and the
    reference's loss is the oracle's loss on that colour."""
    fx = MG.load(golden_dir, MG.RGB_CASE)
    g = fx.g
    assert fx.output_keys == ["accumulation", "depth", "rgb"] and g["out_rgb"].shape == (3,)
    out = T.model_outputs(fx.p, fx.origins, fx.directions, fx.starts, fx.ends, fx.ray_indices, fx.R, fx.temperature, fx.M, use_gradient_scaling=fx.gs)
    for k in ("accumulation", "depth"):
        assert MG.ratio(out[k], g[f"out_{k}"], **MG.OUT_TOL) <= 1.0 and out[k].requires_grad == bool(g[f"rg_{k}"]), k
    assert out["rgb"].shape == (fx.R, 3) and out["rgb"].requires_grad == bool(g["rg_rgb"])
    quirk = dict(out, rgb=out["rgb"].sum(0))
    assert MG.ratio(quirk["rgb"], g["out_rgb"], **MG.OUT_TOL) <= 1.0
    loss = T.model_loss(quirk, None, fx.image, fx.bg_random, "rgb")
    assert set(loss) == {"rgb_loss"} and MG.ratio(loss["rgb_loss"], g["loss_rgb_loss"], **MG.OUT_TOL) <= 1.0
    names = [k for k, _ in fx.p.named_parameters()]
    grads = torch.autograd.grad(loss["rgb_loss"], [v for _, v in fx.p.named_parameters()], allow_unused=True)
    want = MG.fixture_grads(fx)
    for k, gv in zip(names, grads):
        assert MG.ratio(gv if gv is not None else torch.zeros_like(want[k]), want[k], **MG.GRAD_TOL) <= 1.0, k


def _g8_faults(monkeypatch):
    """Planted wiring faults, each a wrapper around the oracle: name -> a function (fx) -> oracle step."""

    def patched(name, replacement):
        def run(fx):
            with monkeypatch.context() as m:
                m.setattr(T, name, replacement)
                return MG.oracle_step(fx)
        return run

    def spectral_factor_1(loss):
        return dict(loss, spectral_loss=loss["spectral_loss"] / 5) if "rgb_loss" in loss else loss

    def threshold_run(fx):
        def threshold_0(out):
            with torch.no_grad():
                on = (out["accumulation"] > 0.0).to(out["spectral"].dtype)
                label = out["seg_probs"].argmax(1)
                return dict(out, seg_raw=label * on.squeeze(), seg_pred=fx.class_colors[label] * on)

        return MG.oracle_step(fx, post_outputs=threshold_0)

    depth, lookup = T.render_depth_expected, T.cluster_lookup
    return {
        "spectral factor 5 -> 1": lambda fx: MG.oracle_step(fx, post_loss=spectral_factor_1),
        "rgb_loss_weight ignored": lambda fx: MG.oracle_step(fx, rgb_loss_weight=1.0),
        "gradient scaling flipped": lambda fx: MG.oracle_step(fx, use_gradient_scaling=not fx.gs),
        "depth clip omitted": patched("render_depth_expected", lambda w, s, e, ri, n, clip_range=None: depth(w, s, e, ri, n, (-np.inf, np.inf))),
        "accumulation threshold 0.5 -> 0.0": threshold_run,
        "cluster alpha 0.2 -> None": patched("cluster_lookup", lambda x, alpha, clusters: lookup(x, None, clusters)),
        "background blend dropped": patched("blend_background_for_loss", lambda pred, acc, gt, bg: (pred, gt)),
    }


def test_g8_rejects_planted_wiring_faults(golden_dir, monkeypatch):
    """The teeth of G8: each planted fault misses some stored quantity by at least 10x its tolerance on at least one case (an exact
    quantity -- the labels -- by any amount), while the oracle as it is stays inside every tolerance."""
    fixtures = [MG.load(golden_dir, case) for case in MG.SPECTRAL_CASES]
    for fx in fixtures:
        assert max(MG.oracle_ratios(fx, MG.oracle_step(fx)).values()) <= 1.0
    caught = {}
    for name, run in _g8_faults(monkeypatch).items():
        worst = [max(MG.oracle_ratios(fx, run(fx)).items(), key=lambda kv: kv[1]) for fx in fixtures]
        caught[name] = max(worst, key=lambda kv: kv[1])
    print(caught)
    missed = {k: v for k, v in caught.items() if not v[1] >= 10.0}
    assert not missed, missed
