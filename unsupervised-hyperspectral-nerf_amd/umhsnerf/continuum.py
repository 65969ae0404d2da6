"""Continuum removal and absorption-feature maps: every spectrum divided by its continuum -- the upper convex hull of the spectrum over
wavelength -- and, per named feature window, how deep the absorption is, where it sits and how much area it takes (the USGS-style
workflow: ENVI "continuum removed", spectral feature fitting).  A feature uses the hull over its OWN window, so it does not depend on
the rest of the spectrum.

``ContinuumAnalysis(wavelengths, features)`` holds the scene's wavelengths and the named windows; ``UMHSModel.continuum_context(analysis)``
makes a render emit ``cr``, ``cr_<b>``, ``feature_depth``, ``feature_depth_<f>``, ``feature_center_<f>`` and ``feature_area_<f>``;
``--continuum-features FILE`` does so on the render and eval command lines, and

    python -m umhsnerf.continuum captured --load-config RUN/config.json --split train --continuum-features F --output-path OUT
    python -m umhsnerf.continuum endmembers --checkpoint CKPT --load-config RUN/config.json --continuum-features F

analyse the captured ``hs_image`` stack of a split without rendering anything, and the learnt endmembers on the host ("which material
carries the 680 nm feature").  Pixels go through one HIP kernel (``ops.continuum``, csrc/umhs_continuum.hip; include/umhs_hip.h,
"Continuum removal", is the definition); library entries and endmembers through ``continuum_removed`` / ``feature_numbers`` here, pure
float64 numpy."""
from __future__ import annotations

import argparse
import json
import re
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_BANDS, MAX_FEATURES, MIN_FEATURE_BANDS = 256, 8, 3  # the kernel's limits (include/umhs_hip.h)
_NAME = re.compile(r"^(cr|feature_depth|feature_center|feature_area)_(\d+)$")
STACKED_OUTPUTS = ("cr", "feature_depth")


# ---- names ------------------------------------------------------------------------------------------------------------------------
def continuum_index(name: str) -> Optional[Tuple[str, Optional[int]]]:
    """("cr" | "feature_depth" | "feature_center" | "feature_area", index or None for the stacked ``cr`` / ``feature_depth``), else None."""
    if name in STACKED_OUTPUTS:
        return name, None
    m = _NAME.match(name)
    return (m.group(1), int(m.group(2))) if m else None


def is_continuum_output(name: str) -> bool:
    return continuum_index(name) is not None


def needs_removed(name: str) -> bool:
    """Is it ``cr`` or a ``cr_<b>``: an output that needs the [R,B] continuum-removed cube?"""
    k = continuum_index(name)
    return k is not None and k[0] == "cr"


def continuum_outputs(B: int, F: int) -> Tuple[str, ...]:
    """The names a context of B bands and F features offers."""
    return ("cr", *(f"cr_{b}" for b in range(B)), *(("feature_depth",) if F else ()),
            *(f"feature_{what}_{f}" for f in range(F) for what in ("depth", "center", "area")))


def requested_without_features(names: Sequence[str], features_file) -> None:
    """``ValueError`` naming the flag when a render asks for a ``feature_*`` output without ``--continuum-features``."""
    asked = [n for n in names if is_continuum_output(n) and not needs_removed(n)]
    if asked and features_file is None:
        raise ValueError(f"{', '.join(asked[:5])}: feature outputs need the feature windows; pass --continuum-features FILE "
                         '({"features": [{"name": ..., "window": [lo, hi]}, ...]})')


# ---- the host side: float64 numpy -------------------------------------------------------------------------------------------------
def check_wavelengths(wavelengths) -> np.ndarray:
    """float32 [B] (what the kernel reads).  ``ValueError`` naming the first offending index unless they are finite and strictly
    increasing as float32, 1..256 of them."""
    w = np.asarray([float(v) for v in np.asarray(wavelengths).reshape(-1)], np.float64)
    if not 1 <= w.shape[0] <= MAX_BANDS:
        raise ValueError(f"{w.shape[0]} wavelengths are outside what the continuum kernel takes: 1..{MAX_BANDS} bands")
    w32 = w.astype(np.float32)
    bad = np.nonzero(~np.isfinite(w32))[0]
    if bad.size:
        raise ValueError(f"wavelength {int(bad[0])} is not finite ({w[bad[0]]!r})")
    bad = np.nonzero(~(np.diff(w32) > 0))[0]
    if bad.size:
        i = int(bad[0]) + 1
        raise ValueError(f"wavelengths must be strictly increasing (as float32): wavelength {i} ({w[i]:g}) does not exceed wavelength "
                         f"{i - 1} ({w[i - 1]:g})")
    return w32


def window_range(wavelengths: np.ndarray, window: Sequence[float]) -> Tuple[int, int]:
    """The inclusive band range of all b with window[0] <= l_b <= window[1] (both edges belong to the window); (0, -1) when empty."""
    w = np.asarray(wavelengths, np.float64)
    inside = np.nonzero((w >= float(window[0])) & (w <= float(window[1])))[0]
    return (int(inside[0]), int(inside[-1])) if inside.size else (0, -1)


def _hull_vertices(l: np.ndarray, x: np.ndarray) -> List[int]:
    """The strict vertices of the upper hull of (l, x), ascending, by walking from each vertex to the LAST band of steepest slope
    ahead of it (gift wrapping: a band on a chord is skipped)."""
    n, v = l.shape[0], [0]
    while v[-1] < n - 1:
        i = v[-1]
        slope = (x[i + 1:] - x[i]) / (l[i + 1:] - l[i])
        best = slope.max()
        v.append(i + 1 + int(np.nonzero(slope == best)[0][-1]))
    return v


def continuum(spectra, wavelengths) -> np.ndarray:
    """float64 [...,B]: the upper convex hull of every row over the wavelengths, evaluated at every band.  Rows must be finite."""
    l = np.asarray(wavelengths, np.float64).reshape(-1)
    x = np.asarray(spectra, np.float64)
    flat = x.reshape(-1, l.shape[0])
    out = np.empty_like(flat)
    for r, row in enumerate(flat):
        v = _hull_vertices(l, row)
        out[r] = np.interp(l, l[v], row[v])
        out[r, v] = row[v]
    return out.reshape(x.shape)


def continuum_removed(spectra, wavelengths) -> np.ndarray:
    """float64 [...,B]: x / continuum where the continuum is positive, else 1; a row with a NaN or an Inf gives 0.  The host twin of
    ``ops.continuum``'s ``removed``, for library entries and endmembers."""
    x = np.asarray(spectra, np.float64)
    B = x.shape[-1]
    flat = x.reshape(-1, B)
    ok = np.isfinite(flat).all(1)
    out = np.zeros_like(flat)
    if ok.any():
        c = continuum(flat[ok], wavelengths)
        out[ok] = np.where(c > 0, flat[ok] / np.where(c > 0, c, 1.0), 1.0)
    return out.reshape(x.shape)


def feature_numbers(spectra, wavelengths, ranges: Sequence[Tuple[int, int]]) -> np.ndarray:
    """float64 [...,F,3]: (depth, centre, area) of every band range on the hull of its own range, as the kernel defines them."""
    l = np.asarray(wavelengths, np.float64).reshape(-1)
    x = np.asarray(spectra, np.float64)
    out = np.zeros((*x.shape[:-1], len(ranges), 3))
    for f, (lo, hi) in enumerate(ranges):
        r = continuum_removed(x[..., lo:hi + 1], l[lo:hi + 1])
        q = 1.0 - r
        m = r.argmin(-1)
        out[..., f, 0] = 1.0 - r.min(-1)
        out[..., f, 1] = l[lo + m]
        out[..., f, 2] = (0.5 * np.diff(l[lo:hi + 1]) * (q[..., :-1] + q[..., 1:])).sum(-1)
    ok = np.isfinite(x).all(-1)
    out[~ok] = 0.0
    return out


class ContinuumAnalysis:
    """The scene's wavelengths (float32, finite, strictly increasing) and up to 8 named feature windows [l_lo, l_hi], in the units of
    the wavelengths; a window becomes the band range of all b with l_lo <= l_b <= l_hi and must hold at least 3 bands."""

    def __init__(self, wavelengths, features: Sequence = ()):
        self.wavelengths = check_wavelengths(wavelengths)
        feats = [(str(f["name"]), f["window"]) if isinstance(f, dict) else (str(f[0]), f[1]) for f in features]
        if len(feats) > MAX_FEATURES:
            raise ValueError(f"{len(feats)} features ({', '.join(n for n, _ in feats[MAX_FEATURES:][:5])} and the like are too many): the "
                             f"continuum kernel takes at most {MAX_FEATURES}")
        self.names: List[str] = []
        self.windows: List[Tuple[float, float]] = []
        self.ranges: List[Tuple[int, int]] = []
        for name, window in feats:
            if name in self.names:
                raise ValueError(f"feature {name!r} is named twice")
            try:
                lo_w, hi_w = (float(v) for v in window)
            except (TypeError, ValueError):
                raise ValueError(f"feature {name!r}: the window must be two numbers [lo, hi], got {window!r}") from None
            if not lo_w <= hi_w:
                raise ValueError(f"feature {name!r}: the window [{lo_w:g}, {hi_w:g}] is empty or not finite")
            lo, hi = window_range(self.wavelengths, (lo_w, hi_w))
            if hi - lo + 1 < MIN_FEATURE_BANDS:
                raise ValueError(f"feature {name!r}: the window [{lo_w:g}, {hi_w:g}] holds {max(hi - lo + 1, 0)} of the scene's bands; a "
                                 f"feature needs at least {MIN_FEATURE_BANDS} (the scene covers {self.wavelengths[0]:g}..{self.wavelengths[-1]:g})")
            self.names.append(name)
            self.windows.append((lo_w, hi_w))
            self.ranges.append((lo, hi))
        self._device_state: Dict = {}

    def __len__(self) -> int:
        return len(self.names)

    @property
    def bands(self) -> int:
        return int(self.wavelengths.shape[0])

    @classmethod
    def from_file(cls, path, wavelengths) -> "ContinuumAnalysis":
        """``{"features": [{"name": "chlorophyll", "window": [640, 700]}, ...]}``, windows in the units of ``wavelengths``."""
        path = Path(path)
        try:
            doc = json.loads(path.read_text())
        except json.JSONDecodeError as e:
            raise ValueError(f"{path}: not JSON ({e})") from None
        feats = doc.get("features") if isinstance(doc, dict) else None
        if not isinstance(feats, list) or any(not isinstance(f, dict) or "name" not in f or "window" not in f for f in feats):
            raise ValueError(f'{path}: a features file is {{"features": [{{"name": NAME, "window": [lo, hi]}}, ...]}}')
        return cls(wavelengths, feats)

    def summary(self) -> Dict:
        return {"features": list(self.names), "ranges": [[lo, hi] for lo, hi in self.ranges]}

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def on(self, device) -> torch.Tensor:
        """The float32 wavelengths on ``device``, made once per device."""
        key = str(torch.device(device))
        if key not in self._device_state:
            self._device_state[key] = torch.from_numpy(self.wavelengths).to(device).contiguous()
        return self._device_state[key]

    def run(self, spectra: torch.Tensor, want_removed: bool = True, want_status: bool = True):
        """``ops.continuum`` of float32 device rows [...,B] -> (removed [R,B] | None, features [R,F,3] | None, status [R] | None)."""
        return ops_continuum(spectra.float(), self.on(spectra.device), self.ranges, want_removed, want_status, self.bands)

    def frame_outputs(self, spectral: torch.Tensor, accumulation: Optional[torch.Tensor], names: Optional[Sequence[str]] = None):
        """The outputs of an assembled frame, by ONE ``ops.continuum`` launch: ``spectral`` [H,W,B] (or [R,B]) and ``accumulation``
        [H,W,1] (or None) -> ``cr`` [H,W,B] and ``cr_<b>`` [H,W,1], the continuum-removed spectrum; ``feature_depth`` [H,W,F] and
        ``feature_depth_<f>``, ``feature_center_<f>``, ``feature_area_<f>`` [H,W,1].  Everything is 0 where ``accumulation <= 0.5``
        and where the spectrum holds a NaN or an Inf.  ``names``: the outputs that are wanted (None: all of them; other names are
        ignored).  Only those are built: the [R,B] cube is not computed when no ``cr`` / ``cr_<b>`` is among them, the features are not
        when no ``feature_*`` is (an analysis without features computes none), and nothing is launched when neither is."""
        lead, B, F = spectral.shape[:-1], self.bands, len(self)
        wanted = list(continuum_outputs(B, F)) if names is None else [n for n in dict.fromkeys(names) if is_continuum_output(n)]
        cube = any(needs_removed(n) for n in wanted)
        feat = F > 0 and any(not needs_removed(n) for n in wanted)
        out: Dict[str, torch.Tensor] = {}
        if not (cube or feat):
            return out
        removed, feats, status = ops_continuum(spectral.float(), self.on(spectral.device), self.ranges if feat else (), cube, True, self.bands)
        shown = status != -1
        if accumulation is not None:
            shown = shown & (accumulation.reshape(-1) > 0.5)
        if cube:
            removed = torch.where(shown[:, None], removed, torch.zeros_like(removed))
        if feat:
            feats = torch.where(shown[:, None, None], feats, torch.zeros_like(feats))
        column = {"feature_depth": 0, "feature_center": 1, "feature_area": 2}
        for name in wanted:
            kind, index = continuum_index(name)
            if kind == "cr":
                out[name] = removed.view(*lead, B) if index is None else removed[:, index].contiguous().view(*lead, 1)
            elif index is None:
                out[name] = feats[:, :, 0].contiguous().view(*lead, F)
            else:
                out[name] = feats[:, index, column[kind]].contiguous().view(*lead, 1)
        return out


def ops_continuum(spectra: torch.Tensor, wavelengths: torch.Tensor, ranges, want_removed: bool, want_status: bool, bands: int):
    """``ops.continuum`` behind the band-count check the analysis makes."""
    from . import ops

    if spectra.shape[-1] != bands:
        raise ValueError(f"spectra of {spectra.shape[-1]} bands against {bands} wavelengths")
    return ops.continuum(spectra, wavelengths, ranges, want_removed, want_status)


class ContinuumTally:
    """What ``eval --continuum-features`` sums over the split, on the device, over the pixels with rendered ``accumulation > 0.5``
    whose captured spectrum is finite: per feature the squared difference of the rendered and the captured depth, the absolute
    difference of their centres, and both depths.  Read once, by ``result``."""

    def __init__(self, analysis: ContinuumAnalysis, device):
        self.analysis = analysis
        self.sums = torch.zeros(4, max(len(analysis), 1), dtype=torch.float64, device=device)  # square, |centre|, rendered, captured
        self.pixels = torch.zeros((), dtype=torch.float64, device=device)

    def output_names(self) -> Tuple[str, ...]:
        """The continuum outputs ``add`` reads: what an eval render under ``continuum_context(analysis, names)`` has to build."""
        F = len(self.analysis)
        return (("feature_depth",) if F else ()) + tuple(f"feature_center_{f}" for f in range(F))

    def add(self, outputs: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        F = len(self.analysis)
        if "hs_image" not in batch or F == 0:
            return
        device = self.sums.device
        gt = batch["hs_image"].to(device).float().reshape(-1, self.analysis.bands)
        _, cap, status = self.analysis.run(gt, False, True)
        w = ((outputs["accumulation"].reshape(-1) > 0.5) & (status != -1)).double()
        depth = outputs["feature_depth"].reshape(-1, F).double()
        center = torch.cat([outputs[f"feature_center_{f}"].reshape(-1, 1) for f in range(F)], 1).double()
        cap = cap.double()
        self.sums += torch.stack([(((depth - cap[:, :, 0]) ** 2) * w[:, None]).sum(0), ((center - cap[:, :, 1]).abs() * w[:, None]).sum(0),
                                  (depth * w[:, None]).sum(0), (cap[:, :, 0] * w[:, None]).sum(0)])
        self.pixels += w.sum()

    def result(self) -> Dict:
        F, n = len(self.analysis), float(self.pixels)
        keys = ("feature_depth_rmse", "feature_center_mae", "feature_depth_rendered_mean", "feature_depth_captured_mean")
        if n <= 0 or F == 0:
            return {"feature_names": list(self.analysis.names), **{k: None for k in keys}}
        s = self.sums.cpu().numpy()[:, :F]
        return {"feature_names": list(self.analysis.names), keys[0]: [float(v) for v in np.sqrt(s[0] / n)],
                keys[1]: [float(v) for v in s[1] / n], keys[2]: [float(v) for v in s[2] / n], keys[3]: [float(v) for v in s[3] / n]}


# ---- command-line plumbing shared with render and eval ---------------------------------------------------------------------------
def add_continuum_arguments(p) -> None:
    p.add_argument("--continuum-features", default=None, metavar="FILE",
                   help='absorption-feature windows, {"features": [{"name": NAME, "window": [lo, hi]}, ...]} in the units of the scene\'s '
                        "wavelengths: feature_depth, feature_depth_<f>, feature_center_<f>, feature_area_<f> (cr and cr_<b>, the "
                        "continuum-removed spectrum, need no file)")
    p.add_argument("--library-continuum-removed", action="store_true",
                   help="with --spectral-library: match continuum-removed spectra against continuum-removed entries (absorption shapes, not "
                        "slope and albedo)")


def check_continuum_arguments(args, names: Sequence[str] = ()) -> None:
    """The refusals that need no file: a ``feature_*`` output without ``--continuum-features``; ``--library-continuum-removed`` without
    ``--spectral-library``.  ``ValueError``."""
    requested_without_features(names, args.continuum_features)
    if getattr(args, "library_continuum_removed", False) and getattr(args, "spectral_library", None) is None:
        raise ValueError("--library-continuum-removed changes how a spectral library is matched: pass --spectral-library FILE")


def analysis_from_args(args, model, names: Optional[Sequence[str]] = ()) -> Optional[ContinuumAnalysis]:
    """The ``ContinuumAnalysis`` of the flags for a built model: the file's features; without a file, one with no features when a
    ``cr`` / ``cr_<b>`` output is named; else None."""
    from .library import scene_wavelengths

    if args.continuum_features is not None:
        return ContinuumAnalysis.from_file(args.continuum_features, scene_wavelengths(model))
    if any(needs_removed(n) for n in (names or ())):
        return ContinuumAnalysis(scene_wavelengths(model))
    return None


# ---- command line ----------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .eval import add_model_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.continuum", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    cap = sub.add_parser("captured", help="feature maps of the captured hs_image stack of a split; no model run")
    add_model_arguments(cap)
    cap.add_argument("--continuum-features", required=True, metavar="FILE")
    cap.add_argument("--split", default="train", choices=["train", "val", "test"])
    cap.add_argument("--output-path", required=True, metavar="OUT", help="directory for <stem>_features.npy [H,W,F,3] and summary.json")
    cap.add_argument("--save-removed", action="store_true", help="also write <stem>_cr.npy [H,W,B], the continuum-removed cube")
    end = sub.add_parser("endmembers", help="depth, centre and area of every feature in every learnt endmember (host float64)")
    add_model_arguments(end)
    end.add_argument("--continuum-features", required=True, metavar="FILE")
    return ap


def continuum_captured(pipeline, analysis: ContinuumAnalysis, split: str, output_path, save_removed: bool = False) -> List[Dict]:
    """Every frame of the split's ``hs_image`` stack through ``ops.continuum``: ``OUT/<stem>_features.npy`` float32 [H,W,F,3] per frame
    (``<stem>_cr.npy`` [H,W,B] with ``save_removed``) and its summary {"frame", "mean_depth" [F], "mean_area" [F], "invalid"} over the
    valid pixels."""
    dm = pipeline.datamanager
    resident = dm.train_split if split == "train" else dm.eval_split
    stack = getattr(resident, "hs_image", None)
    if stack is None:
        raise ValueError(f"the {split} split has no hyperspectral stack (hs_image): nothing captured to analyse")
    dataset = dm.train_dataset if split == "train" else dm.eval_dataset
    filenames = getattr(dataset, "image_filenames", None)
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    device, F = pipeline.model.device, len(analysis)
    frames = []
    for i in range(stack.shape[0]):  # (a host-resident stack is uploaded a frame at a time)
        frame = stack[i].to(device).float()
        removed, feats, status = analysis.run(frame, save_removed, True)
        valid = (status != -1).double()
        n = valid.sum().clamp(min=1.0)
        if F:
            sums = torch.cat([(feats[:, :, 0].double() * valid[:, None]).sum(0) / n, (feats[:, :, 2].double() * valid[:, None]).sum(0) / n,
                              (status == -1).sum().double()[None]]).cpu().tolist()  # (the frame's one read)
        else:
            sums = [float((status == -1).sum())]
        stem = Path(str(filenames[i])).stem if filenames is not None and i < len(filenames) else f"frame_{i:05d}"
        shape = tuple(frame.shape[:-1])
        np.save(output_path / f"{stem}_features.npy",
                (feats.view(*shape, F, 3).cpu().numpy() if F else np.zeros((*shape, 0, 3), np.float32)))
        if save_removed:
            np.save(output_path / f"{stem}_cr.npy", removed.view(*shape, analysis.bands).cpu().numpy())
        frames.append({"frame": stem, "mean_depth": sums[:F], "mean_area": sums[F:2 * F], "invalid": int(sums[-1])})
    return frames


def endmember_features(analysis: ContinuumAnalysis, endmembers) -> List[Dict]:
    """Per learnt endmember (clamped to [0,1], as the renderer uses them) the numbers of every feature, in host float64:
    [{"endmember", "features": {name: {"depth", "center", "area"}}}]."""
    E = endmembers.detach().float().clamp(0.0, 1.0).cpu().numpy() if torch.is_tensor(endmembers) else np.asarray(endmembers, np.float32)
    if E.ndim != 2 or E.shape[1] != analysis.bands:
        raise ValueError(f"endmembers are {E.shape}; the analysis has {analysis.bands} wavelengths")
    numbers = feature_numbers(E, analysis.wavelengths, analysis.ranges)
    return [{"endmember": k, "features": {name: {"depth": float(numbers[k, f, 0]), "center": float(numbers[k, f, 1]),
                                                 "area": float(numbers[k, f, 2])} for f, name in enumerate(analysis.names)}}
            for k in range(E.shape[0])]


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from .library import scene_wavelengths

    args = build_parser().parse_args(argv)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    analysis = ContinuumAnalysis.from_file(args.continuum_features, scene_wavelengths(pipeline.model))
    if args.command == "captured":
        frames = continuum_captured(pipeline, analysis, args.split, args.output_path, args.save_removed)
        result = {"output_path": str(args.output_path), "split": args.split, "continuum": analysis.summary(), "frames": frames}
        (Path(args.output_path) / "summary.json").write_text(json.dumps(result))
    else:
        if pipeline.model.config.method == "rgb":
            raise NotImplementedError("continuum features need a spectral method (spectral, rgb+spectral): method=\"rgb\" has no endmembers")
        rows = endmember_features(analysis, pipeline.model.field.endmembers)
        result = {"continuum": analysis.summary(), "endmembers": rows}
        for f, name in enumerate(analysis.names):  # "which material carries the feature": deepest first
            order = sorted(rows, key=lambda r: -r["features"][name]["depth"])
            print(f"{name} [{analysis.windows[f][0]:g}, {analysis.windows[f][1]:g}]: " + ", ".join(
                f"endmember {r['endmember']} depth {r['features'][name]['depth']:.4f} at {r['features'][name]['center']:g} "
                f"(area {r['features'][name]['area']:.4g})" for r in order), file=sys.stderr)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
