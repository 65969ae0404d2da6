"""Scene statistics: the mean and the B x B covariance of a scene's spectra, and what they show -- principal components as false colour
(``pca_0`` .., ``pca_rgb``) and the Reed-Xiaoli anomaly detector (``rx_score``, ``rx_mask``: the squared Mahalanobis distance of a pixel's
spectrum to the scene's mean under the scene's covariance).

    python -m umhsnerf.statistics compute --load-config RUN/config.json --source captured|rendered --split train --output stats.npz

accumulates them over a split (``StatisticsAccumulator``: ``ops.gram_accumulate``, csrc/umhs_statistics.hip);
``UMHSModel.scene_statistics_context(stats)`` makes a render emit the outputs; ``--scene-statistics FILE`` does so on the render and eval
command lines.  The two passes over pixels are HIP kernels; everything else here is host code in float64 on B x B matrices."""
from __future__ import annotations

import argparse
import json
import math
import statistics as _pystat
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_BANDS = 256  # the kernels' limit (include/umhs_hip.h)
RX_OUTPUTS = ("rx_score", "rx_mask")
DEFAULT_FALSE_ALARM = 1e-3
DEFAULT_FLOOR = 1e-6
TOP_EIGENVALUES = 16  # what ``compute`` prints


def pca_index(name: str) -> Optional[int]:
    """k of ``pca_<k>``, else None."""
    if name.startswith("pca_") and name[4:].isdigit():
        return int(name[4:])
    return None


def is_statistics_output(name: str) -> bool:
    return name in RX_OUTPUTS or name == "pca_rgb" or pca_index(name) is not None


def statistics_outputs(components: int) -> Tuple[str, ...]:
    """STATISTICS_OUTPUTS of a context with ``components`` stored components."""
    return (*RX_OUTPUTS, *(f"pca_{k}" for k in range(components)), *(("pca_rgb",) if components >= 3 else ()))


STATISTICS_OUTPUTS = statistics_outputs(3)  # the default context's names


def requested_without_statistics(names: Sequence[str], statistics_file) -> None:
    """``ValueError`` naming the flag when a render asks for a statistics output without ``--scene-statistics``."""
    asked = [n for n in names if is_statistics_output(n)]
    if asked and statistics_file is None:
        raise ValueError(f"{', '.join(asked[:5])}: statistics outputs need the scene's statistics; pass --scene-statistics FILE "
                         "(python -m umhsnerf.statistics compute makes one)")


def chi_square_quantile(dof: int, false_alarm: float) -> float:
    """The value a chi-square variable of ``dof`` degrees of freedom exceeds with probability ``false_alarm``, by the Wilson-Hilferty
    cube-root approximation.  It sharpens with ``dof``: at a rate of 1e-3 it is 1.7e-3 high at 30 degrees of freedom and within 1e-3
    from 50."""
    if dof < 1 or not 0.0 < false_alarm < 1.0:
        raise ValueError(f"a chi-square quantile needs dof >= 1 and 0 < false alarm < 1, got {dof}, {false_alarm}")
    z = _pystat.NormalDist().inv_cdf(1.0 - false_alarm)
    v = 2.0 / (9.0 * dof)
    return dof * (1.0 - v + z * math.sqrt(v)) ** 3


class SceneStatistics:
    """n spectra's mean [B] and covariance [B,B] (the biased one: divided by n), float64 on the host, on ``wavelengths`` [B]."""

    def __init__(self, n, mean, covariance, wavelengths: Sequence[float]):
        self.n = int(n)
        self.mean = np.asarray(mean, dtype=np.float64).reshape(-1)
        self.covariance = np.asarray(covariance, dtype=np.float64)
        self.wavelengths = [float(w) for w in wavelengths]
        B = self.mean.shape[0]
        if self.covariance.shape != (B, B) or len(self.wavelengths) != B or not 1 <= B <= MAX_BANDS:
            raise ValueError(f"statistics are a mean [B], a covariance [B,B] and B wavelengths, 1 <= B <= {MAX_BANDS}; got mean "
                             f"{self.mean.shape}, covariance {self.covariance.shape}, {len(self.wavelengths)} wavelengths")
        if self.n < 2:
            raise ValueError(f"statistics of n = {self.n} spectra: a covariance needs at least 2")
        if not (np.isfinite(self.mean).all() and np.isfinite(self.covariance).all()):
            raise ValueError("the mean or the covariance holds a value that is not finite")
        if not np.array_equal(self.covariance, self.covariance.T):
            raise ValueError("the covariance is not symmetric")
        self._whitening: Dict = {}
        self._device_state: Dict = {}

    @property
    def bands(self) -> int:
        return self.mean.shape[0]

    @classmethod
    def from_accumulator(cls, acc, shift, wavelengths: Sequence[float]) -> "SceneStatistics":
        """``acc`` [1 + B + B*B] = (n, s, G) about ``shift`` (include/umhs_hip.h): mean = shift + s / n, covariance = G / n - d d^T with
        d = s / n, in float64."""
        acc, shift = np.asarray(acc, dtype=np.float64).reshape(-1), np.asarray(shift, dtype=np.float64).reshape(-1)
        B = shift.shape[0]
        if acc.shape[0] != 1 + B + B * B:
            raise ValueError(f"an accumulator of {B} bands holds {1 + B + B * B} values, got {acc.shape[0]}")
        n = int(acc[0])
        if n < 2:
            raise ValueError(f"the accumulator counted {n} valid spectra: a covariance needs at least 2")
        d = acc[1:1 + B] / n
        G = acc[1 + B:].reshape(B, B) / n
        return cls(n, shift + d, G - np.outer(d, d), wavelengths)

    # ---- files -------------------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """``.npz``: ``n``, ``wavelengths`` [B], ``mean`` [B], ``covariance`` [B,B] (float64)."""
        with open(path, "wb") as f:  # (a file object: numpy appends no suffix of its own)
            np.savez(f, n=np.int64(self.n), wavelengths=np.asarray(self.wavelengths, np.float64), mean=self.mean, covariance=self.covariance)

    @classmethod
    def load(cls, path, wavelengths: Optional[Sequence[float]] = None) -> "SceneStatistics":
        """Reads what ``save`` wrote.  ``ValueError`` saying why for: a missing array; wavelengths that are not the scene's
        (``wavelengths``, when given: statistics are not resampled); n < 2; values that are not finite; a covariance that is not
        symmetric."""
        path = Path(path)
        with np.load(path, allow_pickle=False) as f:
            missing = [k for k in ("n", "wavelengths", "mean", "covariance") if k not in f.files]
            if missing:
                raise ValueError(f"{path}: no array named {', '.join(missing)} (scene statistics hold n, wavelengths, mean, covariance)")
            n, wl, mean, cov = int(f["n"]), np.asarray(f["wavelengths"], np.float64).reshape(-1), f["mean"], f["covariance"]
        if wavelengths is not None:
            scene = np.asarray([float(w) for w in wavelengths], np.float64)
            if wl.shape != scene.shape or not np.allclose(wl, scene, rtol=1e-9, atol=1e-9):
                raise ValueError(f"{path}: the statistics were taken on {wl.shape[0]} wavelengths "
                                 f"({wl[:3].tolist()}..) that are not the scene's {scene.shape[0]} ({scene[:3].tolist()}..)")
        try:
            return cls(n, mean, cov, wl.tolist())
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None

    # ---- the whitening -----------------------------------------------------------------------------------------------------------
    def whitening(self, floor: float = DEFAULT_FLOOR) -> Tuple[np.ndarray, np.ndarray]:
        """(W [B,B], eigenvalues [B]), float64: ``numpy.linalg.eigh`` of the covariance, eigenvalues descending and each floored at
        ``floor`` x the largest -- all B directions are kept: flooring instead of dropping keeps the detector sensitive in low-variance
        directions while bounding their amplification at 1 / sqrt(floor) -- every eigenvector's sign fixed so that its entry of largest
        magnitude is positive, W[k] = v_k / sqrt(eigenvalue_k).  Then |W (x - mean)|^2 is the squared Mahalanobis distance and
        W (x - mean) the principal components at unit variance.  A covariance whose largest eigenvalue is <= 0 is refused."""
        floor = float(floor)
        if not 0.0 < floor <= 1.0:
            raise ValueError(f"the eigenvalue floor must be in (0, 1], got {floor}")
        if floor not in self._whitening:
            lam, V = np.linalg.eigh(self.covariance)
            lam, V = lam[::-1].copy(), V[:, ::-1].T.copy()  # rows: eigenvectors, eigenvalues descending
            if not lam[0] > 0.0:
                raise ValueError(f"the covariance has no positive eigenvalue (largest: {lam[0]:g}): nothing to whiten")
            lam = np.maximum(lam, floor * lam[0])
            rows = np.arange(V.shape[0])
            V = V * np.where(V[rows, np.abs(V).argmax(1)] < 0, -1.0, 1.0)[:, None]
            self._whitening[floor] = (V / np.sqrt(lam)[:, None], lam)
        return self._whitening[floor]

    def floored(self, floor: float = DEFAULT_FLOOR) -> int:
        """How many eigenvalues sit on the floor."""
        lam = self.whitening(floor)[1]
        return int((lam <= floor * lam[0]).sum())

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def on(self, device, floor: float = DEFAULT_FLOOR):
        """(operand image of W, float32 mean [B]) on ``device``, made once per (device, floor)."""
        from . import ops

        key = (str(torch.device(device)), float(floor))
        if key not in self._device_state:
            W = torch.from_numpy(self.whitening(floor)[0]).float().contiguous()
            self._device_state[key] = (ops.library_prepare(W.to(device)), torch.from_numpy(self.mean).float().to(device))
        return self._device_state[key]

    def frame_outputs(self, spectral: torch.Tensor, accumulation: Optional[torch.Tensor], components: int = 3,
                      threshold: Optional[float] = None, floor: float = DEFAULT_FLOOR) -> Dict[str, torch.Tensor]:
        """The outputs of an assembled frame, by ONE ``ops.spectral_project`` launch: ``spectral`` [H,W,B] (or [R,B]) and ``accumulation``
        [H,W,1] (or None) -> ``rx_score`` [H,W,1] (0 where accumulation <= 0.5), ``rx_mask`` [H,W,1] (1.0 where rx_score > threshold;
        None: the chi-square quantile of B degrees of freedom at false-alarm rate 1e-3), ``pca_k`` [H,W,1] for k < ``components`` (the
        whitened component values, 0 where not rendered) and, with at least 3 components, ``pca_rgb`` [H,W,3] =
        clamp(0.5 + y_{0..2} / 6, 0, 1), i.e. +-3 sigma, black where not rendered."""
        from . import ops

        B, P = self.bands, int(components)
        if spectral.shape[-1] != B:
            raise ValueError(f"spectra of {spectral.shape[-1]} bands against statistics of {B}")
        if not 0 <= P <= B:
            raise ValueError(f"{P} components of {B} bands")
        if threshold is None:
            threshold = chi_square_quantile(B, DEFAULT_FALSE_ALARM)
        lead = spectral.shape[:-1]
        image, mean = self.on(spectral.device, floor)
        y, score = ops.spectral_project(spectral.float(), mean, image, B, P, want_score=True)
        if accumulation is not None:
            rendered = (accumulation.reshape(-1) > 0.5)
            score = torch.where(rendered, score, torch.zeros_like(score))
            y = torch.where(rendered[:, None], y, torch.zeros_like(y))
        else:
            rendered = torch.ones_like(score, dtype=torch.bool)
        out = {"rx_score": score.view(*lead, 1), "rx_mask": (score > float(threshold)).to(score.dtype).view(*lead, 1)}
        for k in range(P):
            out[f"pca_{k}"] = y[:, k].contiguous().view(*lead, 1)
        if P >= 3:
            out["pca_rgb"] = ((0.5 + y[:, :3] / 6.0).clamp(0.0, 1.0) * rendered[:, None].to(y.dtype)).view(*lead, 3)
        return out


class StatisticsAccumulator:
    """The device-resident (count, sum, Gram) of every valid spectrum handed to ``add``, about a fixed ``shift`` (float32 [B]; anything
    near the mean: the covariance does not depend on it beyond rounding, and a shift near the mean keeps that rounding small)."""

    def __init__(self, B: int, device, shift):
        if not 1 <= int(B) <= MAX_BANDS:
            raise ValueError(f"{B} bands are outside what the kernel takes: 1..{MAX_BANDS}")
        self.B, self.device = int(B), torch.device(device)
        self.shift = torch.as_tensor(shift, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        if self.shift.shape[0] != self.B:
            raise ValueError(f"a shift of {self.shift.shape[0]} values for {self.B} bands")
        self.acc = torch.zeros(1 + self.B + self.B * self.B, dtype=torch.float64, device=self.device)

    def add(self, spectra: torch.Tensor, accumulation: Optional[torch.Tensor] = None) -> None:
        """Rows [...,B] of float32 device spectra; ``accumulation`` [...,1]: rows at <= 0.5 are left out.  No host sync."""
        from . import ops

        ops.gram_accumulate(spectra, self.shift, self.acc, accumulation)

    def result(self, wavelengths: Sequence[float]) -> SceneStatistics:
        """Reads the accumulator (the one host sync)."""
        return SceneStatistics.from_accumulator(self.acc.cpu().numpy(), self.shift.cpu().numpy(), wavelengths)


def first_frame_shift(spectra: torch.Tensor, accumulation: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The float32 mean of a frame's valid rows (finite; accumulation > 0.5): the shift of an accumulation.  Zeros without one."""
    x = spectra.detach().float().reshape(-1, spectra.shape[-1])
    ok = torch.isfinite(x).all(1)
    if accumulation is not None:
        ok = ok & (accumulation.reshape(-1) > 0.5)
    w = ok.to(x.dtype)[:, None]
    return (torch.where(ok[:, None], x, torch.zeros_like(x)).sum(0) / w.sum().clamp(min=1.0)).contiguous()


class StatisticsTally:
    """What ``eval --scene-statistics`` sums over the split, on the device: rx_score / B and the pixels above the threshold, over the
    rendered pixels, and the same on the captured ``hs_image``.  Read once, by ``result``."""

    def __init__(self, stats: SceneStatistics, device, threshold: float, floor: float = DEFAULT_FLOOR):
        self.stats, self.threshold, self.floor = stats, float(threshold), float(floor)
        self.sums = torch.zeros(6, dtype=torch.float64, device=device)  # rendered: score, exceed, pixels; captured: the same

    def add(self, outputs: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        score = outputs["rx_score"].reshape(-1)
        self.sums[:3] += self._sums(score, outputs["accumulation"].reshape(-1) > 0.5)
        if "hs_image" in batch:
            gt = batch["hs_image"].to(score.device).float().reshape(-1, self.stats.bands)
            captured = self.stats.frame_outputs(gt, None, 0, self.threshold, self.floor)["rx_score"].reshape(-1)
            self.sums[3:] += self._sums(captured, torch.isfinite(gt).all(1))

    def _sums(self, score: torch.Tensor, counted: torch.Tensor) -> torch.Tensor:
        """(sum of the counted scores, how many of them are above the threshold, how many are counted), float64, no host sync."""
        kept = torch.where(counted, score, torch.zeros_like(score)).double()
        return torch.stack([kept.sum(), (counted & (score > self.threshold)).sum().double(), counted.sum().double()])

    def result(self) -> Dict:
        s, B = self.sums.cpu().tolist(), self.stats.bands
        return {"rx_mean": s[0] / (B * s[2]) if s[2] > 0 else None, "rx_exceed": s[1] / s[2] if s[2] > 0 else None,
                "rx_captured_mean": s[3] / (B * s[5]) if s[5] > 0 else None, "rx_captured_exceed": s[4] / s[5] if s[5] > 0 else None}


# ---- command-line plumbing shared with render and eval ---------------------------------------------------------------------------
def add_statistics_arguments(p) -> None:
    p.add_argument("--scene-statistics", default=None, metavar="FILE",
                   help="the scene's mean and covariance (.npz of `python -m umhsnerf.statistics compute`): rx_score, rx_mask, pca_<k>, pca_rgb")
    p.add_argument("--pca-components", type=int, default=3, metavar="P", help="how many whitened principal components are output (pca_0..)")
    p.add_argument("--rx-threshold", type=float, default=None, metavar="X", help="rx_mask is 1 where rx_score is above this")
    p.add_argument("--rx-false-alarm", type=float, default=None, metavar="Q",
                   help=f"set the threshold to the chi-square quantile at this false-alarm rate (default {DEFAULT_FALSE_ALARM:g})")
    p.add_argument("--rx-floor", type=float, default=DEFAULT_FLOOR, metavar="F",
                   help="eigenvalues of the covariance are floored at F x the largest")


def threshold_from_args(args, bands: int) -> float:
    if args.rx_threshold is not None and args.rx_false_alarm is not None:
        raise ValueError("--rx-threshold and --rx-false-alarm both set the threshold: pass one of them")
    if args.rx_threshold is not None:
        return float(args.rx_threshold)
    return chi_square_quantile(bands, DEFAULT_FALSE_ALARM if args.rx_false_alarm is None else args.rx_false_alarm)


def load_for_model(path, model) -> Optional[SceneStatistics]:
    """``--scene-statistics FILE`` for a built model (None: no statistics)."""
    from .library import scene_wavelengths

    return None if path is None else SceneStatistics.load(path, scene_wavelengths(model))


def context_arguments(args, model) -> Optional[Dict]:
    """The keyword arguments of ``scene_statistics_context`` from the flags (None: the flag is absent)."""
    stats = load_for_model(args.scene_statistics, model)
    if stats is None:
        return None
    if not 0 <= args.pca_components <= stats.bands:
        raise ValueError(f"--pca-components {args.pca_components}: the scene has {stats.bands} bands")
    stats.whitening(args.rx_floor)  # (a covariance that cannot be whitened is refused here, before anything is rendered)
    return dict(stats=stats, components=args.pca_components, threshold=threshold_from_args(args, stats.bands), floor=args.rx_floor)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .eval import add_model_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.statistics", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    comp = sub.add_parser("compute", help="accumulate the mean and covariance of a split's spectra and save them")
    add_model_arguments(comp)
    comp.add_argument("--source", default="captured", choices=["captured", "rendered"],
                      help="captured: the split's hs_image stack, no model run; rendered: every camera of the split rendered once")
    comp.add_argument("--split", default="train", choices=["train", "val", "test"])
    comp.add_argument("--output", required=True, metavar="FILE", help="the .npz to write")
    comp.add_argument("--rx-floor", type=float, default=DEFAULT_FLOOR, metavar="F", help="the floor the printed summary counts against")
    return ap


def accumulate_split(pipeline, source: str, split: str) -> StatisticsAccumulator:
    """Every frame of the split into one accumulator; the shift is the float32 mean of the first frame's valid rows."""
    from .render import split_cameras

    dm, model = pipeline.datamanager, pipeline.model
    device = model.device
    accumulator = None
    if source == "captured":
        resident = dm.train_split if split == "train" else dm.eval_split
        stack = getattr(resident, "hs_image", None)
        if stack is None:
            raise ValueError(f"the {split} split has no hyperspectral stack (hs_image): nothing captured to take statistics of")
        for i in range(stack.shape[0]):  # (a host-resident stack is uploaded a frame at a time)
            frame = stack[i].to(device).float()
            if accumulator is None:
                accumulator = StatisticsAccumulator(frame.shape[-1], device, first_frame_shift(frame))
            accumulator.add(frame)
    else:
        if model.config.method == "rgb":
            raise NotImplementedError("rendered statistics need a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no spectrum")
        cameras, _ = split_cameras(pipeline, split)
        pipeline.eval()
        with torch.no_grad():
            for i in range(len(cameras)):
                out = model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True), output_names=["spectral", "accumulation"])
                if accumulator is None:
                    accumulator = StatisticsAccumulator(out["spectral"].shape[-1], device, first_frame_shift(out["spectral"], out["accumulation"]))
                accumulator.add(out["spectral"], out["accumulation"])
    if accumulator is None:
        raise ValueError(f"the {split} split holds no frame")
    return accumulator


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from .library import scene_wavelengths

    args = build_parser().parse_args(argv)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    stats = accumulate_split(pipeline, args.source, args.split).result(scene_wavelengths(pipeline.model))
    stats.save(args.output)
    lam = stats.whitening(args.rx_floor)[1]
    raw = np.linalg.eigvalsh(stats.covariance)[::-1]
    total = float(np.clip(raw, 0.0, None).sum())
    result = {"output": str(args.output), "source": args.source, "split": args.split, "n": stats.n, "bands": stats.bands,
              "eigenvalues": [float(v) for v in lam[:TOP_EIGENVALUES]],
              "explained_variance": [float(max(v, 0.0) / total) if total > 0 else 0.0 for v in raw[:TOP_EIGENVALUES]],
              "eigenvalues_at_floor": stats.floored(args.rx_floor)}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
