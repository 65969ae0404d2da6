"""The HIP model against G8: what the reference's own ``UMHSModel.get_outputs`` / ``get_loss_dict`` / ``get_metrics_dict`` computed
on a fixed packed batch (tests/golden/g8_model_<case>.npz, data only; built by tests/golden/make_golden.py).

Every model-level path is held to the same fixture: the autograd path, ``UMHSPipeline.train_iteration`` in both forms of the step,
the gradient-free render path, and the metrics.  Tolerances are the model-level ones of tests/test_hip_parity.py: outputs within 1e-4
of the tensor's maximum AND every element within rtol 1e-4 / atol 1e-6; losses and metrics 1e-4 relative; gradients 2e-4 and
post-step parameters 1e-4 of the tensor's maximum.  The labels (``seg_raw``, ``seg_pred``) and ``num_samples_per_ray`` are compared
exactly: the fixtures keep every top-2 gap of ``seg_probs`` above 1e-4 and every accumulation 1e-2 away from the 0.5 threshold.

Named deviations of the build from the reference, stated here and nowhere silently skipped:
  * ``weights`` [N,1], the per-sample rendering weights, is an output the reference does not have;
  * ``spectral2`` is detached (it carries no loss in the reference): its VALUE is compared, its ``requires_grad`` flag is exempt;
  * ``depth`` and ``seg_probs`` carry a gradient in the reference and none here (the per-ray epilogue kernel has a backward through
    ``rgb`` only; no loss of the reference reads either): ``test_autograd_path`` asserts exactly that, flag by flag.
Every other output carries a gradient exactly where the reference's does.  (This file found three that did not -- ``specular``,
``abundances`` and the pseudo-rgb of method "spectral", rendered under no_grad in the reference, were differentiable here -- and
``get_outputs_from_samples`` now detaches them.)

The worst |diff| / tolerance per case, path and tensor goes to ``model_golden.json`` in the run-output directory."""
import os

import numpy as np
import pytest
import torch

import model_golden as MG
from oracle import torch_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("seg_raw", "seg_pred", "num_samples_per_ray")
PRODUCT_ONLY = {"weights"}
GRAD_FLAG_EXEMPT = {"spectral2"}
NO_GRADIENT_HERE = {"depth", "seg_probs"}  # requires_grad in the reference, not in the build (module docstring)


@pytest.fixture(scope="module", params=MG.SPECTRAL_CASES)
def fx(request, golden_dir):
    return MG.load(golden_dir, request.param)


def _pipeline(fx):
    from umhsnerf.umhs_model import UMHSConfig
    from umhsnerf.umhs_pipeline import UMHSPipeline

    cfg = UMHSConfig(method=fx.method, pred_specular=fx.spec, temperature=fx.temperature, log2_hashmap_size=fx.log2_T,
                     use_gradient_scaling=fx.gs, rgb_loss_weight=fx.rgb_w)
    assert cfg.background_color == "random"  # the reference's default
    pipe = UMHSPipeline.from_packed_samples(cfg, torch.device(DEV), metadata={"wavelengths": fx.bands, "num_classes": fx.C}, seed=3)
    pipe.model.field.load_state_dict(fx.p.reference_state_dict())
    with torch.no_grad():
        pipe.model.class_colors.copy_(fx.class_colors)
    return pipe


def _samples(fx):
    from umhsnerf._ns_compat import packed_ray_samples

    rs = packed_ray_samples(fx.origins.to(DEV), fx.directions.to(DEV), fx.starts.to(DEV), fx.ends.to(DEV))
    batch = {"image": fx.image.to(DEV), "hs_image": fx.hs_image.to(DEV)}
    return rs, fx.ray_indices.to(DEV), batch, fx.bg_random.to(DEV)


def _check_outputs(r, fx, outputs, flags: bool):
    g = fx.g
    keys = set(outputs.keys())
    r.check("key set", 0.0 if keys - PRODUCT_ONLY == set(fx.output_keys) and PRODUCT_ONLY <= keys else MG.INF,
            f" (missing {sorted(set(fx.output_keys) - keys)}, extra {sorted(keys - set(fx.output_keys) - PRODUCT_ONLY)})")
    for k in MG.base_outputs(fx):
        got, want = outputs[k], g[f"out_{k}"]
        if k in EXACT:
            same = tuple(got.shape) == want.shape and np.array_equal(got.detach().double().cpu().numpy(), want.astype(np.float64))
            r.check(f"{k} (exact)", 0.0 if same else MG.INF)
        else:
            r.check(f"{k} / max", MG.max_ratio(got, want, MG.GPU_OUT_MAX))
            r.check(f"{k} / element", MG.ratio(got, want, **MG.GPU_OUT_ELEM))
        if flags and k not in GRAD_FLAG_EXEMPT:
            ref_flag = bool(g[f"rg_{k}"])
            if k in NO_GRADIENT_HERE:
                assert ref_flag  # (were the reference's flag False, this would be no deviation)
            r.check(f"requires_grad[{k}]", 0.0 if got.requires_grad == (ref_flag and k not in NO_GRADIENT_HERE) else MG.INF,
                    f" (got {got.requires_grad}, the reference has {ref_flag})")
    for prefix, whole in (("wv_", "spectral"), ("residual_", "specular"), ("abundances_", "abundances")):
        if whole in outputs:
            views = all(torch.equal(outputs[f"{prefix}{i}"], outputs[whole][..., i]) for i in range(outputs[whole].shape[-1]))
            r.check(f"{prefix}i are the columns of {whole}", 0.0 if views else MG.INF)


def _check_losses(r, fx, loss_dict):
    want = {k[5:]: float(fx.g[k]) for k in fx.g.files if k.startswith("loss_")}
    r.check("loss keys", 0.0 if set(loss_dict) == set(want) else MG.INF)
    for k, v in want.items():
        r.check(f"loss[{k}]", MG.scalar_ratio(loss_dict[k], v, MG.GPU_SCALAR))


def _check_metrics(r, fx, metrics, tag):
    want = {k[7:]: float(fx.g[k]) for k in fx.g.files if k.startswith("metric_")}
    r.check(f"metric keys ({tag})", 0.0 if set(metrics.keys()) == set(want) else MG.INF)
    for k, v in want.items():
        r.check(f"metric[{k}] ({tag})", MG.scalar_ratio(metrics[k], v, 0.0 if k == "num_samples_per_batch" else MG.GPU_SCALAR))


def test_autograd_path(fx):
    """``get_outputs_from_samples`` -> ``get_loss_dict(background=)`` -> ``backward()``: every base output, the per-band views, the key
    set, which outputs carry a gradient, both losses, and EVERY entry of the flat gradient through the layout (hash rows: the touched
    ones match, the untouched ones and the alignment padding are exactly zero)."""
    r = MG.Report(fx.case, "autograd")
    pipe = _pipeline(fx)
    model, field = pipe.model, pipe.model.field
    rs, ri, batch, bg = _samples(fx)
    model.train()
    pipe.optimizer.zero_grad(set_to_none=True)
    outputs = model.get_outputs_from_samples(rs, ri, fx.R)
    loss_dict = model.get_loss_dict(outputs, batch, background=bg)
    sum(loss_dict.values()).backward()
    torch.cuda.synchronize()
    _check_outputs(r, fx, outputs, flags=True)
    _check_losses(r, fx, loss_dict)
    L, gflat = field.layout, field.flat.grad.detach().cpu()
    want = MG.fixture_grads_by_state_key(fx)
    r.check("layout entries", 0.0 if set(L.entries) == set(want) else MG.INF)
    covered = torch.zeros(L.total, dtype=torch.bool)
    for k, (off, shp) in L.entries.items():
        covered[off : off + int(np.prod(shp))] = True
        r.check(f"grad[{k}]", MG.max_ratio(L.view(gflat, k), want[k], MG.GPU_GRAD))
    table = L.view(gflat, "mlp_base.encoder.hash_table")
    untouched = torch.ones(table.shape[0], dtype=torch.bool)
    untouched[torch.from_numpy(fx.g["grad_hash_rows"]).long()] = False
    r.check("grad: untouched hash rows are zero", 0.0 if float(table[untouched].abs().max()) == 0.0 else MG.INF)
    r.check("grad: alignment padding is zero", 0.0 if (~covered).sum() == 0 or float(gflat[~covered].abs().max()) == 0.0 else MG.INF)
    r.finish(ROOT)


@pytest.mark.parametrize("fused", ["0", "1"], ids=["per-sample arrays", "per-ray sums in the field kernels"])
def test_train_iteration(fx, fused, monkeypatch):
    """``UMHSPipeline.train_iteration`` (the launch-sequence step) in both forms: outputs, the loss dict, and the parameters after one
    step against ``T.adam_step`` on the FIXTURE's gradients followed by the endmember clamp.  Where the folded backward declines a
    configuration the per-sample form must have run instead, and is compared all the same."""
    from umhsnerf import ops

    monkeypatch.setenv("UMHS_FUSED_BWD", fused)
    r = MG.Report(fx.case, f"train_iteration fused_bwd={fused}")
    pipe = _pipeline(fx)
    model = pipe.model
    rs, ri, batch, bg = _samples(fx)
    pipe.train()
    assert model.direct_step_supported(batch)
    spec = model.field._spec()
    folded = fused == "1" and ops.field_bwd_composited_supported(spec) and ops.field_heads_fwd_supported(spec)
    calls = {"split": 0, "composite_bwd": 0}
    split, composite_bwd = model._split_forward, ops.composite_bwd

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(model, "_split_forward", spy("split", split))
    monkeypatch.setattr(ops, "composite_bwd", spy("composite_bwd", composite_bwd))
    outputs, loss_dict = pipe.train_iteration(rs, ri, fx.R, batch, background=bg)
    torch.cuda.synchronize()
    assert (calls["split"] == 1, calls["composite_bwd"] == 0) == (folded, folded), (calls, folded)  # the form asked for, or its fallback
    _check_outputs(r, fx, outputs, flags=False)
    _check_losses(r, fx, loss_dict)
    p = MG.new_params(fx, lambda k: fx.g[f"param_{k}"])
    grads = MG.fixture_grads(fx)
    with torch.no_grad():
        params = [v for _, v in p.named_parameters()]
        T.adam_step(params, [grads[k] for k, _ in p.named_parameters()], [torch.zeros_like(v) for v in params],
                    [torch.zeros_like(v) for v in params], 1, T.exp_decay_lr(0))
        p.endmembers.clamp_(0, 1)
    after = model.field.state_dict()
    for k, v in p.reference_state_dict().items():
        r.check(f"param after step[{k}]", MG.max_ratio(after[k], v, MG.GPU_PARAM))
    r.finish(ROOT)


def test_gradient_free_render_path(fx, monkeypatch):
    """``model.eval()`` under ``torch.no_grad()``: ``_render_outputs_from_samples`` is the path taken, and it gives the same outputs."""
    r = MG.Report(fx.case, "render")
    pipe = _pipeline(fx)
    model = pipe.model
    rs, ri, batch, _ = _samples(fx)
    taken = []
    render = model._render_outputs_from_samples
    monkeypatch.setattr(model, "_render_outputs_from_samples", lambda *a, **k: taken.append(1) or render(*a, **k))
    model.eval()
    with torch.no_grad():
        outputs = model.get_outputs_from_samples(rs, ri, fx.R)
        metrics = model.get_metrics_dict(outputs, batch)
    torch.cuda.synchronize()
    assert taken == [1]
    _check_outputs(r, fx, outputs, flags=False)
    assert type(metrics) is dict  # materialised outside training
    _check_metrics(r, fx, metrics, "eval")
    r.finish(ROOT)


def test_training_metrics_are_lazy_and_match(fx):
    """``get_metrics_dict`` in training: nothing computed until somebody looks, then the reference's values."""
    from umhsnerf.umhs_model import LazyMetrics

    r = MG.Report(fx.case, "metrics")
    pipe = _pipeline(fx)
    model = pipe.model
    rs, ri, batch, bg = _samples(fx)
    model.train()
    outputs = model.get_outputs_from_samples(rs, ri, fx.R)
    metrics = model.get_metrics_dict(outputs, batch)
    assert isinstance(metrics, LazyMetrics) and dict.__len__(metrics) == 0
    _check_metrics(r, fx, metrics, "training")
    r.finish(ROOT)
