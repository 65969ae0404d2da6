"""Unsupervised classification: k-means of a scene's spectra (Euclidean), or spherical k-means (spectral angle), on the GPU.

``fit(frames, K, metric, init)`` runs Lloyd's algorithm over device-resident frames: every iteration is one fused pass per frame
(``ops.cluster_step``, csrc/umhs_cluster.hip: every row is assigned and the rows of each cluster are summed in the same pass), ONE host
read (the accumulator) and a float64 update of the centres on the host.  ``SpectralClusters`` holds the result, saves / loads it
(``.npz``; an angle file is also a valid ``--spectral-library`` file) and classifies frames: ``cluster_raw`` /
``cluster_pred`` / ``cluster_score``.

    python -m umhsnerf.cluster fit --load-config RUN/config.json --source captured --split train --clusters 6 --metric angle --output clusters.npz
    python -m umhsnerf.cluster captured --load-config RUN/config.json --split train --clusters-file clusters.npz --output-path OUT

Needs nothing learnt or supplied: no dictionary, no library, no endmember set.  It is the baseline an unsupervised material segmentation
is judged against."""
from __future__ import annotations

import argparse
import io
import json
import sys
import zipfile
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

CLUSTER_OUTPUTS = ("cluster_raw", "cluster_pred", "cluster_score")
METRICS = ("angle", "euclidean")
MAX_CLUSTERS, MAX_BANDS = 64, 256  # the kernel's limits (include/umhs_hip.h)
SUBSAMPLE = 65536  # rows k-means++ draws its centres from


def requested_without_clusters(names: Sequence[str], clusters_file) -> None:
    """``ValueError`` naming the flag when a render asks for a cluster output without ``--clusters``."""
    from .library import _some

    asked = [n for n in names if n in CLUSTER_OUTPUTS]
    if asked and clusters_file is None:
        raise ValueError(f"{_some(asked)}: cluster outputs need fitted clusters; pass --clusters FILE")


def _check_metric(metric: str) -> str:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {', '.join(METRICS)}; got {metric!r}")
    return metric


class SpectralClusters:
    """K cluster centres on the scene's B wavelengths.  ``centres`` float64 [K,B] (for ``angle`` their direction is what counts),
    ``metric`` "angle" or "euclidean", ``counts`` int64 [K] (the rows of each cluster at the last assignment of the fit), ``colors``
    float32 [K,3] in 0..1 (default: the model's class colours, cycled, as a spectral library's)."""

    def __init__(self, centres: np.ndarray, metric: str, wavelengths: Sequence[float], counts: Optional[np.ndarray] = None,
                 colors: Optional[np.ndarray] = None, objective: float = float("nan")):
        from .umhs_model import CLASS_COLORS

        self.centres = np.asarray(centres, dtype=np.float64)
        self.metric = _check_metric(str(metric))
        self.wavelengths = [float(w) for w in wavelengths]
        K, B = self.centres.shape if self.centres.ndim == 2 else (0, 0)
        if self.centres.ndim != 2 or len(self.wavelengths) != B:
            raise ValueError(f"clusters are centres [K,B] and B wavelengths; got centres {self.centres.shape}, {len(self.wavelengths)} wavelengths")
        if not 1 <= K <= MAX_CLUSTERS or not 1 <= B <= MAX_BANDS:
            raise ValueError(f"{K} clusters on {B} bands are outside what the clustering kernel takes: 1..{MAX_CLUSTERS} clusters, "
                             f"1..{MAX_BANDS} bands")
        if not np.isfinite(self.centres).all() or (self.metric == "angle" and not self.centres.any(1).all()):
            raise ValueError("cluster centres must be finite (and, for the angle metric, not all zero)")
        self.counts = np.zeros(K, np.int64) if counts is None else np.asarray(counts, dtype=np.int64).reshape(-1)
        if self.counts.shape[0] != K:
            raise ValueError(f"counts must be [{K}], got {self.counts.shape}")
        if colors is None:
            palette = CLASS_COLORS.numpy()
            colors = palette[np.arange(K) % len(palette)]
        self.colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if self.colors.shape[0] != K or not np.isfinite(self.colors).all() or self.colors.min() < 0 or self.colors.max() > 1:
            raise ValueError(f"colors must be [K,3] in 0..1, got {self.colors.shape}")
        self.objective = float(objective)
        self.names = [f"cluster_{k}" for k in range(K)]
        self._device_state: Dict = {}

    def __len__(self) -> int:
        return self.centres.shape[0]

    @property
    def bands(self) -> int:
        return self.centres.shape[1]

    # ---- files -------------------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """``.npz``: names [K], wavelengths [B], spectra [K,B] (the centres), colors [K,3], metric, counts [K], objective.  The same
        clusters give the same bytes (the archive carries no time stamp)."""
        arrays = {"names": np.asarray(self.names), "wavelengths": np.asarray(self.wavelengths, np.float64), "spectra": self.centres,
                  "colors": self.colors, "metric": np.asarray(self.metric), "counts": self.counts,
                  "objective": np.asarray(self.objective, np.float64)}
        with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
            for name, a in arrays.items():
                buffer = io.BytesIO()
                np.lib.format.write_array(buffer, np.asanyarray(a), allow_pickle=False)
                z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buffer.getvalue())

    @classmethod
    def load(cls, path, wavelengths: Sequence[float]) -> "SpectralClusters":
        """Nothing is resampled: ``ValueError`` when the file's band count or wavelengths are not the scene's."""
        from .library import _some

        path = Path(path)
        with np.load(path, allow_pickle=False) as f:
            missing = [k for k in ("wavelengths", "spectra", "metric") if k not in f.files]
            if missing:
                raise ValueError(f"{path}: no array named {_some(missing)} (fitted clusters hold wavelengths, spectra, metric[, colors, counts])")
            wl, centres, metric = np.asarray(f["wavelengths"], np.float64).reshape(-1), np.asarray(f["spectra"], np.float64), str(f["metric"])
            colors = np.asarray(f["colors"], np.float32) if "colors" in f.files else None
            counts = np.asarray(f["counts"], np.int64) if "counts" in f.files else None
            objective = float(f["objective"]) if "objective" in f.files else float("nan")
        scene = np.asarray([float(w) for w in wavelengths], np.float64)
        if centres.ndim != 2 or centres.shape[1] != scene.shape[0]:
            raise ValueError(f"{path}: clusters fitted on {centres.shape[-1] if centres.ndim == 2 else '?'} bands, the scene has "
                             f"{scene.shape[0]}: fit them on this scene (nothing is resampled)")
        if wl.shape != scene.shape or not np.allclose(wl, scene, rtol=1e-6, atol=0.0):
            raise ValueError(f"{path}: the clusters' wavelengths are not the scene's: fit them on this scene (nothing is resampled)")
        return cls(centres, metric, scene.tolist(), counts, colors, objective)

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def device_centres(self) -> torch.Tensor:
        """float32 [K,B], what the kernel takes: for ``angle`` the rows at unit length (normalised in float64, rounded once), for
        ``euclidean`` the centres rounded once."""
        c = torch.from_numpy(self.centres)
        return (c / c.norm(dim=1, keepdim=True) if self.metric == "angle" else c).float()

    def on(self, device):
        """(operand image, half_norm float32 [K] or None, colours [K,3]) on ``device``, made once per device."""
        from . import ops

        key = str(torch.device(device))
        if key not in self._device_state:
            c = self.device_centres()
            half = (c.double().pow(2).sum(1) / 2).float().to(device) if self.metric == "euclidean" else None
            self._device_state[key] = (ops.library_prepare(c.to(device)), half, torch.from_numpy(self.colors).to(device))
        return self._device_state[key]

    def step(self, spectra: torch.Tensor, mask: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None,
             want_label: bool = True, want_score: bool = True):
        from . import ops

        if spectra.shape[-1] != self.bands:
            raise ValueError(f"spectra of {spectra.shape[-1]} bands against clusters of {self.bands}")
        image, half, _ = self.on(spectra.device)
        return ops.cluster_step(spectra.float(), image, len(self), self.metric, half, mask, acc, want_label, want_score)

    def assign(self, spectra: torch.Tensor, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``ops.cluster_step`` of float32 device rows [...,B] -> (label int32 [R], score float32 [R]); one launch."""
        return self.step(spectra, mask)

    def frame_outputs(self, spectral: torch.Tensor, accumulation: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The outputs of an assembled frame, by ONE launch: ``spectral`` [H,W,B] (or [R,B]) and ``accumulation`` [H,W,1] (or None) ->
        ``cluster_raw`` [H,W,1] (the index as float32; -1 where nothing is rendered, ``accumulation <= 0.5``, or the spectrum is empty
        or not finite), ``cluster_pred`` [H,W,3] (the cluster's colour, black at -1), ``cluster_score`` [H,W,1] (the cosine or the
        squared distance, 0 at -1)."""
        lead = spectral.shape[:-1]
        label, score = self.step(spectral, None if accumulation is None else accumulation.float())
        colors = self.on(spectral.device)[2]
        at = label.long()
        pred = colors[at.clamp(min=0)] * (at >= 0)[:, None].to(colors.dtype)
        return {"cluster_raw": label.float().view(*lead, 1), "cluster_pred": pred.view(*lead, 3), "cluster_score": score.view(*lead, 1)}


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
def _pairs(frames) -> Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    for f in frames:
        yield (f[0], f[1]) if isinstance(f, (tuple, list)) else (f, None)


def _valid_rows(x: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    rows = x.detach().float().reshape(-1, x.shape[-1])
    ok = torch.isfinite(rows).all(1) & (rows != 0).any(1)
    if mask is not None:
        ok = ok & ~(mask.reshape(-1) <= 0.5)
    return ok


def subsample(frames, seed: int = 0, limit: int = SUBSAMPLE) -> np.ndarray:
    """At most ``limit`` valid rows, float64 [n,B] on the host, drawn evenly over the frames (the same share of ``limit`` from each, all
    of a frame that has fewer) with ``numpy.random.default_rng(seed)``, in frame and row order."""
    rng = np.random.default_rng(seed)
    pairs = list(_pairs(frames))
    if not pairs:
        raise ValueError("no frame to cluster")
    share = -(-limit // len(pairs))
    taken = []
    for x, mask in pairs:
        at = _valid_rows(x, mask).nonzero()[:, 0]
        n = int(at.numel())
        if n > share:
            at = at[torch.from_numpy(np.sort(rng.choice(n, size=share, replace=False))).to(at.device)]
        taken.append(x.detach().reshape(-1, x.shape[-1])[at].double().cpu().numpy())
    rows = np.concatenate(taken, 0)[:limit]
    if rows.shape[0] == 0:
        raise ValueError("the frames hold no valid spectrum (every row is empty, not finite or masked out)")
    return rows


def kmeanspp(rows: np.ndarray, K: int, metric: str, seed: int = 0) -> np.ndarray:
    """k-means++ (D^2 sampling) on the host in float64: the first centre uniformly, every further one with probability proportional to
    the distance to the nearest centre so far -- the squared distance, or 1 - cos for ``angle``.  float64 [K,B] rows of ``rows``."""
    _check_metric(metric)
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, np.float64)
    n = rows.shape[0]
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True) if metric == "angle" else rows

    def distance(i: int) -> np.ndarray:
        return np.clip(1.0 - unit @ unit[i], 0.0, None) if metric == "angle" else ((rows - rows[i]) ** 2).sum(1)

    chosen = [int(rng.integers(n))]
    d = distance(chosen[0])
    while len(chosen) < K:
        total = d.sum()
        i = int(rng.choice(n, p=d / total)) if total > 0 else int(rng.integers(n))
        chosen.append(i)
        d = np.minimum(d, distance(i))
    return rows[chosen].copy()


def initial_centres(frames, K: int, metric: str, init="kmeans++", seed: int = 0, endmembers=None) -> np.ndarray:
    """float64 [K,B]: ``init`` "kmeans++" (on ``subsample(frames, seed)``), "endmembers" (``endmembers`` [C,B], C == K) or an array."""
    if isinstance(init, str):
        if init == "kmeans++":
            return kmeanspp(subsample(frames, seed), K, metric, seed)
        if init == "endmembers":
            if endmembers is None:
                raise ValueError('init="endmembers" needs the model\'s learnt endmembers')
            E = (endmembers.detach().double().cpu().numpy() if isinstance(endmembers, torch.Tensor) else np.asarray(endmembers, np.float64))
            if E.ndim != 2 or E.shape[0] != K:
                raise ValueError(f'init="endmembers": the model has {E.shape[0]} endmembers, --clusters asks for {K}; they must be equal')
            return E.copy()
        raise ValueError(f'init must be "kmeans++", "endmembers" or an array [K,B]; got {init!r}')
    centres = np.asarray(init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else init, np.float64)
    if centres.ndim != 2 or centres.shape[0] != K:
        raise ValueError(f"initial centres must be [K,B] = [{K}, bands], got {centres.shape}")
    return centres.copy()


def update(centres: np.ndarray, acc: np.ndarray, metric: str) -> Tuple[np.ndarray, int]:
    """The Lloyd update on the host in float64 from acc = (valid, objective, n[K], s[K,B]): s / |s| (angle) or s / n (euclidean).  An
    empty cluster keeps its centre.  -> (centres, how many clusters were empty)."""
    K, B = centres.shape
    n, s = acc[2:2 + K], acc[2 + K:].reshape(K, B)
    with np.errstate(divide="ignore", invalid="ignore"):
        new = s / np.linalg.norm(s, axis=1, keepdims=True) if metric == "angle" else s / n[:, None]
    keep = (n == 0) | ~np.isfinite(new).all(1)
    return np.where(keep[:, None], centres, new), int((n == 0).sum())


def fit(frames, K: int, metric: str, init="kmeans++", iterations: int = 50, tolerance: float = 1e-4, seed: int = 0,
        wavelengths: Optional[Sequence[float]] = None, endmembers=None) -> Tuple[SpectralClusters, Dict]:
    """Lloyd's algorithm over ``frames``: an iterable (walked once per iteration) of float32 device tensors [...,B], or of (tensor,
    mask) pairs, mask [...,1] or [R] with rows at <= 0.5 left out.  Per iteration: ``ops.cluster_step`` of every frame into one
    accumulator, ONE host read, the centres updated on the host in float64 and rounded once to float32 for the next pass.  An empty
    cluster keeps its centre.  Stops after ``iterations``, when the objective's relative decrease is <= ``tolerance``, or when the
    float32 centres did not change in a bit.  -> (clusters, log): log = {"objective": [per iteration], "counts": [[K] per iteration],
    "iterations", "converged", "empty" (clusters without a row at the last assignment), "valid" (rows that took part)}.
    The same seed and the same data give the same bytes."""
    _check_metric(metric)
    K = int(K)
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f"{K} clusters are outside what the clustering kernel takes: 1..{MAX_CLUSTERS}")
    if iterations < 1:
        raise ValueError("iterations must be at least 1")
    if iter(frames) is frames:
        frames = list(frames)
    centres = initial_centres(frames, K, metric, init, seed, endmembers)
    B = centres.shape[1]
    wavelengths = list(range(B)) if wavelengths is None else wavelengths
    log: Dict = {"objective": [], "counts": [], "iterations": 0, "converged": False, "empty": 0, "valid": 0}
    clusters = SpectralClusters(centres, metric, wavelengths)
    for _ in range(int(iterations)):
        used = clusters.device_centres()
        acc = None
        for x, mask in _pairs(frames):
            if acc is None:
                acc = torch.zeros(2 + K + K * B, dtype=torch.float64, device=x.device)
            clusters.step(x, mask, acc, want_label=False, want_score=False)
        if acc is None:
            raise ValueError("no frame to cluster")
        host = acc.cpu().numpy()  # the iteration's one host read
        new, empty = update(clusters.centres, host, metric)
        log["objective"].append(float(host[1]))
        log["counts"].append([int(v) for v in host[2:2 + K]])
        log["iterations"] += 1
        log["empty"], log["valid"] = empty, int(host[0])
        clusters = SpectralClusters(new, metric, wavelengths, host[2:2 + K].astype(np.int64), objective=float(host[1]))
        if log["valid"] == 0:
            raise ValueError("the frames hold no valid spectrum (every row is empty, not finite or masked out)")
        o = log["objective"]
        if torch.equal(clusters.device_centres(), used) or (len(o) > 1 and o[-2] - o[-1] <= tolerance * o[-2]):
            log["converged"] = True
            break
    return clusters, log


# ---- eval ----------------------------------------------------------------------------------------------------------------------------
class ClusterTally:
    """What ``eval --clusters`` counts over the split, on the device: per cluster the rendered pixels and the sum of their scores; the
    rendered pixels whose cluster equals the cluster of the captured spectrum at the same pixel; the table of cluster against the
    model's ``seg_raw``; for a scene with label images, the confusion of the CAPTURED frames' clusters against them
    (``ops.seg_confusion``).  Read once, by ``result``."""

    def __init__(self, clusters: SpectralClusters, device, num_classes: int, seg_num_labels: int = 0, seg_ignore_label: int = 255):
        K = len(clusters)
        self.clusters, self.num_classes = clusters, max(int(num_classes), 1)
        self.seg_num_labels, self.seg_ignore_label = int(seg_num_labels), int(seg_ignore_label)
        self.count = torch.zeros(K, dtype=torch.float64, device=device)
        self.score = torch.zeros(K, dtype=torch.float64, device=device)
        self.pixels = torch.zeros((), dtype=torch.float64, device=device)
        self.agree = torch.zeros(2, dtype=torch.float64, device=device)  # (agreeing, compared)
        self.table = torch.zeros(K * self.num_classes, dtype=torch.int64, device=device)  # [cluster, the model's class]
        self.confusion = None  # int64 [K + 1, labels]: the captured frames' cluster x the ground-truth label

    def add(self, outputs: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        from . import ops

        raw = outputs["cluster_raw"].reshape(-1).long()
        hit = raw >= 0
        at = raw[hit]
        self.count.index_add_(0, at, torch.ones_like(at, dtype=torch.float64))
        self.score.index_add_(0, at, outputs["cluster_score"].reshape(-1)[hit].double())
        self.pixels += raw.numel()
        if "seg_raw" in outputs:
            seg = outputs["seg_raw"].reshape(-1).long()
            both = hit & (seg >= 0) & (seg < self.num_classes)
            self.table.index_add_(0, raw[both] * self.num_classes + seg[both], torch.ones_like(raw[both]))
        if "hs_image" in batch:  # the same op on the ground truth
            gt = batch["hs_image"].to(raw.device).float()
            captured = self.clusters.assign(gt.reshape(-1, gt.shape[-1]))[0]
            self.agree += torch.stack([(captured.long()[hit] == at).sum(), hit.sum()]).double()
            if "seg_image" in batch and self.seg_num_labels > 0:
                self.confusion = ops.seg_confusion(captured.float(), torch.ones_like(captured, dtype=torch.float32),
                                                   batch["seg_image"].to(raw.device), len(self.clusters), self.seg_num_labels,
                                                   ignore_label=self.seg_ignore_label, out=self.confusion)

    def result(self) -> Dict:
        from .utils.seg_metrics import match_clusters, seg_scores

        count, score, pixels, agree = self.count.cpu(), self.score.cpu(), float(self.pixels), self.agree.cpu()
        top = [{"name": self.clusters.names[k], "share": float(count[k]) / max(pixels, 1.0), "mean_score": float(score[k] / count[k])}
               for k in range(len(count)) if count[k] > 0]
        out = {"cluster_top": top, "cluster_agreement": float(agree[0] / agree[1]) if agree[1] > 0 else None, "cluster_model_agreement": None}
        table = self.table.cpu().view(len(self.clusters), self.num_classes)
        if int(table.sum()) > 0:  # (every class of the model is given the cluster that shares most pixels with it, none used twice)
            assignment = match_clusters(table)
            out["cluster_model_agreement"] = sum(int(table[r, k]) for k, r in enumerate(assignment) if r >= 0) / int(table.sum())
        if self.confusion is not None:
            scores = seg_scores(self.confusion.cpu())
            scores.pop("assignment", None)
            out.update({f"cluster_{k}": v for k, v in scores.items()})
        return out


# ---- command-line plumbing shared with render and eval -----------------------------------------------------------------------------
def add_cluster_arguments(p) -> None:
    p.add_argument("--clusters", default=None, metavar="FILE",
                   help="fitted clusters (.npz of `python -m umhsnerf.cluster fit`): cluster_raw, cluster_pred, cluster_score")


def load_for_model(path, model) -> Optional[SpectralClusters]:
    """``--clusters FILE`` for a built model (None: no clusters)."""
    from .library import scene_wavelengths

    return None if path is None else SpectralClusters.load(path, scene_wavelengths(model))


# ---- command line ------------------------------------------------------------------------------------------------------------------
class SplitFrames:
    """The frames of a fit, walked once per iteration: cubes that fit under the device budget stay on the device, the rest stay on the
    host and are uploaded a frame at a time."""

    def __init__(self, device, budget_bytes: float):
        self.device, self.left = torch.device(device), float(budget_bytes)
        self.items: List[Tuple[torch.Tensor, Optional[torch.Tensor]]] = []

    def add(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        nbytes = x.numel() * 4
        if nbytes <= self.left:
            self.left -= nbytes
            x = x.to(self.device).float()
        else:
            x = x.cpu()
        self.items.append((x, None if mask is None else mask.to(self.device).float()))

    def __len__(self) -> int:
        return len(self.items)

    def __iter__(self):
        for x, mask in self.items:
            yield x.to(self.device).float(), mask


def split_frames(pipeline, source: str, split: str, device_cache_gb: float = 16.0) -> SplitFrames:
    """``captured``: the split's ``hs_image`` stack, no model run.  ``rendered``: every camera of the split rendered ONCE, with
    ``accumulation`` as the mask."""
    from .render import split_cameras

    dm, model = pipeline.datamanager, pipeline.model
    frames = SplitFrames(model.device, device_cache_gb * 2.0 ** 30)
    if source == "captured":
        resident = dm.train_split if split == "train" else dm.eval_split
        stack = getattr(resident, "hs_image", None)
        if stack is None:
            raise ValueError(f"the {split} split has no hyperspectral stack (hs_image): nothing captured to cluster")
        if stack.is_cuda:
            frames.left = float("inf")  # (already resident: nothing is copied)
        for i in range(stack.shape[0]):
            frames.add(stack[i])
    else:
        if model.config.method == "rgb":
            raise NotImplementedError("rendered clusters need a spectral method (spectral, rgb+spectral): method=\"rgb\" renders no spectrum")
        cameras, _ = split_cameras(pipeline, split)
        pipeline.eval()
        with torch.no_grad():
            for i in range(len(cameras)):
                out = model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True), output_names=["spectral", "accumulation"])
                frames.add(out["spectral"], out["accumulation"])
    if len(frames) == 0:
        raise ValueError(f"the {split} split holds no frame")
    return frames


def build_parser() -> argparse.ArgumentParser:
    from .eval import add_model_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.cluster", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="k-means (or spherical k-means) of a split's spectra; saves the centres")
    add_model_arguments(f)
    f.add_argument("--source", default="captured", choices=["captured", "rendered"],
                   help="captured: the split's hs_image stack, no model run; rendered: every camera of the split rendered once")
    f.add_argument("--split", default="train", choices=["train", "val", "test"])
    f.add_argument("--clusters", type=int, required=True, metavar="K", help=f"how many clusters (1..{MAX_CLUSTERS})")
    f.add_argument("--metric", default="angle", choices=list(METRICS), help="angle: spherical k-means (spectral angle); euclidean: k-means")
    f.add_argument("--init", default="kmeans++", choices=["kmeans++", "endmembers"],
                   help="endmembers: start from the model's learnt endmembers (needs K equal to their count)")
    f.add_argument("--iterations", type=int, default=50)
    f.add_argument("--tolerance", type=float, default=1e-4, help="stop when the objective's relative decrease is at most this")
    f.add_argument("--seed", type=int, default=0)
    f.add_argument("--device-cache-gb", type=float, default=16.0, help="rendered cubes stay on the device up to this; the rest on the host")
    f.add_argument("--output", required=True, metavar="FILE", help="the .npz to write")
    c = sub.add_parser("captured", help="classify every captured frame of a split with fitted clusters")
    add_model_arguments(c)
    c.add_argument("--split", default="train", choices=["train", "val", "test"])
    c.add_argument("--clusters-file", required=True, metavar="FILE")
    c.add_argument("--output-path", required=True, metavar="DIR")
    return ap


def classify_captured(pipeline, clusters: SpectralClusters, split: str, output_path) -> Dict:
    """``OUT/<stem>_cluster.npy`` [H,W] int32 per captured frame and ``OUT/summary.json``."""
    from .render import split_cameras

    out_dir = Path(output_path)
    out_dir.mkdir(parents=True, exist_ok=True)
    frames = split_frames(pipeline, "captured", split, 0.0)
    _, names = split_cameras(pipeline, split)
    K = len(clusters)
    count = torch.zeros(K, dtype=torch.float64, device=pipeline.model.device)
    score = torch.zeros(K, dtype=torch.float64, device=pipeline.model.device)
    invalid, pixels = [], 0
    for i, (x, _) in enumerate(frames):
        label, s = clusters.assign(x)
        at = label.long()
        hit = at >= 0
        count.index_add_(0, at[hit], torch.ones_like(at[hit], dtype=torch.float64))
        score.index_add_(0, at[hit], s[hit].double())
        stem = Path(str(names[i])).stem if names is not None and i < len(names) else f"frame_{i:05d}"
        np.save(out_dir / f"{stem}_cluster.npy", label.view(*x.shape[:-1]).cpu().numpy())
        invalid.append(int((~hit).sum()))
        pixels += int(at.numel())
    count, score = count.cpu(), score.cpu()
    summary = {"split": split, "metric": clusters.metric, "frames": len(invalid), "invalid_pixels": invalid,
               "clusters": [{"name": clusters.names[k], "share": float(count[k]) / max(pixels, 1),
                             "mean_score": float(score[k] / count[k]) if count[k] > 0 else None} for k in range(K)]}
    (out_dir / "summary.json").write_text(json.dumps(summary))
    return summary


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from .library import scene_wavelengths

    args = build_parser().parse_args(argv)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    model = pipeline.model
    if args.command == "fit":
        endmembers = None
        if args.init == "endmembers":
            if model.config.method == "rgb":
                raise NotImplementedError("--init endmembers needs a spectral method (spectral, rgb+spectral): method=\"rgb\" has no endmembers")
            endmembers = model.field.endmembers
        frames = split_frames(pipeline, args.source, args.split, args.device_cache_gb)
        clusters, log = fit(frames, args.clusters, args.metric, args.init, args.iterations, args.tolerance, args.seed,
                            scene_wavelengths(model), endmembers)
        clusters.save(args.output)
        result = {"output": str(args.output), "source": args.source, "split": args.split, "metric": args.metric, "clusters": len(clusters),
                  "bands": clusters.bands, "frames": len(frames), "valid": log["valid"], "iterations": log["iterations"],
                  "converged": log["converged"], "empty": log["empty"], "objective": log["objective"][-1], "counts": log["counts"][-1]}
    else:
        clusters = load_for_model(args.clusters_file, model)
        result = classify_captured(pipeline, clusters, args.split, args.output_path)
        result = {"clusters_file": str(args.clusters_file), "output_path": str(args.output_path), **result}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
