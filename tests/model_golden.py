"""Helpers of the model-level golden tests (G8): fixtures produced by the reference's own ``UMHSModel.get_outputs`` /
``get_loss_dict`` / ``get_metrics_dict`` (tests/golden/make_golden.py, ``g8_model``), read here as data only.

Used by tests/test_oracle_golden.py (the oracle against the fixture, on the CPU) and tests/test_hip_model_golden.py (the HIP model
against the fixture, on the GPU)."""
import json
import os
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import numpy as np
import torch

from oracle import torch_ref as T

SPECTRAL_CASES = ["rs_c6b31s", "s_c4b141n", "rs_c9b128s"]
RGB_CASE = "rgb_c5b21"
BAND_PREFIXES = ("wv_", "residual_", "abundances_")
# the oracle against the fixture: the G4 test's own tolerances
OUT_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-4, atol=1e-5)
INF = float("inf")


def load(golden_dir: str, case: str) -> SimpleNamespace:
    """The fixture ``g8_model_<case>.npz`` -> its arrays (``fx.g``), config scalars, input tensors, and the parameters loaded into a
    fresh ``T.FieldParams`` (``fx.p``)."""
    g = np.load(os.path.join(golden_dir, f"g8_model_{case}.npz"))
    fx = SimpleNamespace(g=g, case=case, method=str(g["method"]), C=int(g["num_classes"]), spec=bool(g["pred_specular"]),
                         temperature=float(g["temperature"]), gs=bool(g["use_gradient_scaling"]), rgb_w=float(g["rgb_loss_weight"]),
                         log2_T=int(g["log2_hashmap_size"]), R=int(g["num_rays"]), bands=[float(b) for b in g["bands"]],
                         output_keys=[str(k) for k in g["output_keys"]])
    fx.B = len(fx.bands)
    for k in ("origins", "directions", "starts", "ends", "ray_indices", "image", "hs_image", "bg_random", "class_colors"):
        setattr(fx, k, torch.from_numpy(g[k]))
    fx.ray_indices = fx.ray_indices.long()
    fx.p = new_params(fx, lambda k: g[f"param_{k}"])
    fx.M = T.colour_matrix(fx.bands)
    return fx


def new_params(fx, value_of: Callable[[str], Optional[np.ndarray]]) -> T.FieldParams:
    """A ``T.FieldParams`` of the fixture's shape whose tensors hold ``value_of(name)`` (None: zeros)."""
    p = T.FieldParams(fx.C, fx.B, fx.spec, method=fx.method, log2_hashmap_size=fx.log2_T, seed=0)
    with torch.no_grad():
        for k, v in p.named_parameters():
            a = value_of(k)
            v.zero_() if a is None else v.copy_(torch.from_numpy(np.asarray(a)))
    return p


def fixture_grads(fx) -> Dict[str, torch.Tensor]:
    """The stored gradient of every parameter, dense (the hash table from its touched rows; a parameter the loss does not reach: zeros)."""
    g, out = fx.g, {}
    for k, v in fx.p.named_parameters():
        if k == "hash_table":
            d = torch.zeros_like(v)
            d[torch.from_numpy(g["grad_hash_rows"]).long()] = torch.from_numpy(g["grad_hash_vals"])
            out[k] = d
        else:
            out[k] = torch.from_numpy(g[f"grad_{k}"]) if f"grad_{k}" in g.files else torch.zeros_like(v)
    return out


def fixture_grads_by_state_key(fx) -> Dict[str, torch.Tensor]:
    """``fixture_grads`` under the reference's state-dict key names (what ``FieldLayout`` is keyed by)."""
    gr = fixture_grads(fx)
    return new_params(fx, lambda k: gr[k].numpy()).reference_state_dict()


# ------------------------------------------------------------------------------------------------------------------------------ #
# the oracle's step
# ------------------------------------------------------------------------------------------------------------------------------ #
def oracle_step(fx, p=None, dtype=torch.float32, use_gradient_scaling=None, rgb_loss_weight=None, post_outputs=None, post_loss=None):
    """``T.model_outputs`` / ``T.model_loss`` / ``T.psnr`` on the fixture's inputs -> (outputs, loss dict, metrics, gradients by name).
    The keyword arguments are where a planted wiring fault goes in; ``dtype=torch.float64`` runs the same step in double."""
    p = fx.p if p is None else p
    cast = (lambda t: t.to(dtype)) if dtype != torch.float32 else (lambda t: t)
    out = T.model_outputs(p, cast(fx.origins), cast(fx.directions), cast(fx.starts), cast(fx.ends), fx.ray_indices, fx.R, fx.temperature,
                          fx.M, use_gradient_scaling=fx.gs if use_gradient_scaling is None else use_gradient_scaling,
                          class_colors=cast(fx.class_colors))
    if post_outputs is not None:
        out = post_outputs(out)
    loss = T.model_loss(out, cast(fx.hs_image), cast(fx.image), cast(fx.bg_random), fx.method,
                        fx.rgb_w if rgb_loss_weight is None else rgb_loss_weight)
    if post_loss is not None:
        loss = post_loss(loss)
    metrics = {}
    if fx.method != "rgb":  # (the reference's get_metrics_dict cannot run on its method "rgb": no fixture either)
        metrics = {"psnr": T.psnr(out["rgb"], cast(fx.image)), "rmse": torch.sqrt(torch.nn.functional.mse_loss(out["rgb"], cast(fx.image))),
                   "psnr_spectral": T.psnr(out["spectral"], cast(fx.hs_image)),
                   "rmse_spectral": torch.sqrt(torch.nn.functional.mse_loss(out["spectral"], cast(fx.hs_image))),
                   "num_samples_per_batch": out["num_samples_per_ray"].sum()}
    names = [k for k, _ in p.named_parameters()]
    params = [v for _, v in p.named_parameters()]
    grads = torch.autograd.grad(sum(loss.values()), params, allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(v)) for k, g, v in zip(names, grads, params)}
    return out, loss, metrics, grads


def base_outputs(fx):
    return [k for k in fx.output_keys if not k.startswith(BAND_PREFIXES)]


def ratio(got, want, rtol, atol) -> float:
    """Worst |got - want| / (rtol |want| + atol) over the elements; inf on a shape mismatch."""
    a, b = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    if a.shape != b.shape:
        return INF
    if a.numel() == 0:
        return 0.0
    return float(((a - b).abs() / (rtol * b.abs() + atol)).max())


def oracle_ratios(fx, step) -> Dict[str, float]:
    """Every stored quantity of a spectral fixture against an oracle step -> {name: worst |diff| / tolerance} (exact quantities: 0 or
    inf).  A faithful oracle has every entry <= 1."""
    out, loss, metrics, grads = step
    g, r = fx.g, {}
    for k in base_outputs(fx):
        if k in ("seg_raw", "seg_pred", "num_samples_per_ray"):  # exact: the fixtures keep every top-2 gap 100x above the tolerance
            same = k in out and tuple(out[k].shape) == g[f"out_{k}"].shape and np.array_equal(out[k].double().numpy(), g[f"out_{k}"].astype(np.float64))
            r[f"out_{k}"] = 0.0 if same else INF
        else:
            r[f"out_{k}"] = ratio(out[k], g[f"out_{k}"], **OUT_TOL) if k in out else INF
    for k in (f for f in g.files if f.startswith("loss_")):
        r[k] = ratio(loss[k[5:]], g[k], **OUT_TOL) if k[5:] in loss else INF
    for k in (f for f in g.files if f.startswith("metric_")):
        r[k] = ratio(metrics[k[7:]], g[k], **OUT_TOL)
    want = fixture_grads(fx)
    for k, gv in grads.items():
        r[f"grad_{k}"] = ratio(gv, want[k], **GRAD_TOL)
    rows = torch.from_numpy(g["grad_hash_rows"]).long()
    untouched = torch.ones(grads["hash_table"].shape[0], dtype=torch.bool)
    untouched[rows] = False
    r["grad_hash_untouched_rows"] = 0.0 if float(grads["hash_table"][untouched].abs().max()) == 0.0 else INF
    return r


# ------------------------------------------------------------------------------------------------------------------------------ #
# the HIP model against the fixture (the model-level tolerances of tests/test_hip_parity.py)
# ------------------------------------------------------------------------------------------------------------------------------ #
GPU_OUT_MAX, GPU_OUT_ELEM = 1e-4, dict(rtol=1e-4, atol=1e-6)
GPU_SCALAR, GPU_GRAD, GPU_PARAM = 1e-4, 2e-4, 1e-4


def max_ratio(got, want, rtol) -> float:
    """max|got - want| / max|want|, in units of ``rtol`` (``assert_close`` of tests/test_hip_parity.py)."""
    a, b = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    if a.shape != b.shape:
        return INF
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) / rtol


def scalar_ratio(got, want, rtol) -> float:
    got = float(got.detach()) if torch.is_tensor(got) else float(got)
    return abs(got - float(want)) / (rtol * abs(float(want)) + 1e-30)


class Report:
    """Worst |diff| / tolerance per (case, path, tensor), written to ``model_golden.json`` of the run-output directory; ``check``
    collects instead of stopping at the first miss, so that one run shows every figure."""

    def __init__(self, case: str, path: str):
        self.case, self.path, self.figures, self.misses = case, path, {}, []

    def check(self, name: str, r: float, note: str = ""):
        self.figures[name] = r
        if not r <= 1.0:
            self.misses.append(f"{name}: {r:.3g} x its tolerance{note}")

    def finish(self, root: str):
        import rays_f64

        path = os.path.join(rays_f64.report_dir(root), "model_golden.json")
        try:
            with open(path) as f:
                doc = json.load(f)
        except (OSError, ValueError):
            doc = {}
        doc.setdefault(self.case, {})[self.path] = self.figures
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
        assert not self.misses, f"{self.case} / {self.path}:\n  " + "\n  ".join(self.misses)
