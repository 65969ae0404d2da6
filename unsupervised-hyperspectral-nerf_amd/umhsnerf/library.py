"""Spectral libraries: name every pixel's material by spectral angle (SAM classification) against a library of known reflectances.

``SpectralLibrary.load(FILE, wavelengths)`` reads a library (``.npz`` or ``.csv``), resamples it onto the scene's
wavelengths and refuses what cannot be matched; ``UMHSModel.spectral_library_context(library)`` makes a render emit ``library_raw`` /
``library_pred`` / ``library_angle`` / ``library_margin``; ``--spectral-library FILE`` does so on the render and eval command lines, and

    python -m umhsnerf.library identify --checkpoint CKPT --load-config RUN/config.json --spectral-library FILE [--top 3]

prints, per learnt endmember, the library entries closest to it.  The matching itself is one HIP kernel (``ops.library_match``,
csrc/umhs_library.hip); everything here is host code or torch on [R]-sized tensors.

Resolution: the kernel's cosine is float32.  Near 1 it moves in steps of 6e-8, so angles below about 1e-3 rad are not resolved:
library entries closer to each other than that tie, and the EARLIER one wins."""
from __future__ import annotations

import argparse
import csv
import json
import math
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

LIBRARY_OUTPUTS = ("library_raw", "library_pred", "library_angle", "library_margin")
MAX_ENTRIES, MAX_BANDS = 65536, 256  # the kernel's limits (include/umhs_hip.h)
TOP_ENTRIES = 16  # rows of eval's library_top


def _some(names: Sequence) -> str:
    names = [str(n) for n in names]
    return ", ".join(names[:5]) + (f" (and {len(names) - 5} more)" if len(names) > 5 else "")


def scene_wavelengths(source) -> List[float]:
    """The scene's wavelengths from a dataparser's outputs / metadata dict (``metadata["wavelengths"]``), a model (its ``kwargs``) or
    a run's ``config.json`` (``derived.wavelengths``)."""
    if isinstance(source, (str, Path)):
        return [float(w) for w in json.loads(Path(source).read_text())["derived"]["wavelengths"]]
    meta = getattr(source, "metadata", None) or getattr(source, "kwargs", None) or source
    return [float(w) for w in meta["wavelengths"]]


def requested_without_library(names: Sequence[str], library_file) -> None:
    """``ValueError`` naming the flag when a render asks for a library output without ``--spectral-library``."""
    asked = [n for n in names if n in LIBRARY_OUTPUTS]
    if asked and library_file is None:
        raise ValueError(f"{_some(asked)}: library outputs need a spectral library; pass --spectral-library FILE")


class SpectralLibrary:
    """L named reflectance spectra on the scene's B wavelengths.  ``spectra`` float64 [L,B] (resampled, every row finite and not all
    zero), ``names`` [L], ``colors`` float32 [L,3] in 0..1 (the file's, or the model's 15 class colours, cycled)."""

    def __init__(self, names: Sequence[str], spectra: np.ndarray, wavelengths: Sequence[float], colors: Optional[np.ndarray] = None):
        from .umhs_model import CLASS_COLORS

        self.names = [str(n) for n in names]
        self.spectra = np.asarray(spectra, dtype=np.float64)
        self.wavelengths = [float(w) for w in wavelengths]
        L, B = self.spectra.shape if self.spectra.ndim == 2 else (0, 0)
        if self.spectra.ndim != 2 or len(self.names) != L or len(self.wavelengths) != B:
            raise ValueError(f"a library is names [L], spectra [L,B] and B wavelengths; got {len(self.names)} names, spectra "
                             f"{self.spectra.shape}, {len(self.wavelengths)} wavelengths")
        if not 1 <= L <= MAX_ENTRIES or not 1 <= B <= MAX_BANDS:
            raise ValueError(f"a library of {L} entries on {B} bands is outside what the matching kernel takes: 1..{MAX_ENTRIES} entries, "
                             f"1..{MAX_BANDS} bands")
        bad = [n for n, row in zip(self.names, self.spectra) if not np.isfinite(row).all() or not row.any()]
        if bad:
            raise ValueError(f"library entries that are not finite or all zero on the scene's wavelengths: {_some(bad)}")
        if colors is None:
            palette = CLASS_COLORS.numpy()
            colors = palette[np.arange(L) % len(palette)]
        self.colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if self.colors.shape[0] != L or not np.isfinite(self.colors).all() or self.colors.min() < 0 or self.colors.max() > 1:
            raise ValueError(f"colors must be [L,3] in 0..1, got {self.colors.shape}")
        self._device_state: Dict = {}
        self._removed: Optional["SpectralLibrary"] = None  # continuum_removed(): made once
        self._removed_with = None  # on that library: the continuum.ContinuumAnalysis its match puts the rows through

    def __len__(self) -> int:
        return len(self.names)

    # ---- files -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def load(cls, path, wavelengths: Sequence[float]) -> "SpectralLibrary":
        """``.npz``: ``names`` [L], ``wavelengths`` [W], ``spectra`` [L,W], optionally ``colors`` [L,3] in 0..1.  ``.csv``: a header
        ``wavelength,<name>,<name>,...`` and one row per wavelength.  Resampled onto ``wavelengths`` (the scene's) by linear interpolation
        in float64.  ``ValueError``, naming up to five entries, for: wavelengths that are not strictly ascending; an entry that does not
        cover the scene's range (its finite samples must reach both ends: nothing is extrapolated); an entry that is not finite or all
        zero after resampling; a number of entries or bands outside the kernel's limits."""
        path = Path(path)
        colors = None
        if path.suffix.lower() == ".npz":
            with np.load(path, allow_pickle=False) as f:
                missing = [k for k in ("names", "wavelengths", "spectra") if k not in f.files]
                if missing:
                    raise ValueError(f"{path}: no array named {_some(missing)} (a library holds names, wavelengths, spectra[, colors])")
                names, wl, spectra = [str(n) for n in f["names"]], np.asarray(f["wavelengths"], np.float64), np.asarray(f["spectra"], np.float64)
                colors = np.asarray(f["colors"], np.float32) if "colors" in f.files else None
        elif path.suffix.lower() == ".csv":
            with open(path, newline="") as f:
                rows = [r for r in csv.reader(f) if r and any(c.strip() for c in r)]
            if not rows or rows[0][0].strip().lower() != "wavelength" or len(rows[0]) < 2:
                raise ValueError(f"{path}: the header must be wavelength,<name>,<name>,...")
            names = [c.strip() for c in rows[0][1:]]
            if any(len(r) != len(rows[0]) for r in rows[1:]):
                raise ValueError(f"{path}: every row needs {len(rows[0])} columns")
            table = np.array([[float(c) if c.strip() else np.nan for c in r] for r in rows[1:]], dtype=np.float64).reshape(-1, len(rows[0]))
            wl, spectra = table[:, 0], table[:, 1:].T
        else:
            raise ValueError(f"{path}: a spectral library is a .npz or a .csv file")
        return cls.resampled(names, wl, spectra, wavelengths, colors)

    @classmethod
    def resampled(cls, names, library_wavelengths, spectra, wavelengths, colors=None) -> "SpectralLibrary":
        wl, spectra = np.asarray(library_wavelengths, np.float64).reshape(-1), np.asarray(spectra, np.float64)
        scene = np.asarray([float(w) for w in wavelengths], np.float64)
        if spectra.ndim != 2 or spectra.shape != (len(names), wl.shape[0]):
            raise ValueError(f"spectra must be [names, wavelengths] = [{len(names)}, {wl.shape[0]}], got {spectra.shape}")
        if not np.isfinite(wl).all() or (np.diff(wl) <= 0).any():
            at = np.nonzero(~(np.diff(wl) > 0))[0] + 1
            raise ValueError(f"library wavelengths must be strictly ascending; not so at position {_some(at.tolist())}")
        if not 1 <= len(names) <= MAX_ENTRIES:
            raise ValueError(f"a library of {len(names)} entries is outside what the matching kernel takes: 1..{MAX_ENTRIES} entries")
        lo, hi = scene.min(), scene.max()
        out, short = np.zeros((len(names), scene.shape[0]), np.float64), []
        for i, row in enumerate(spectra):
            ok = ~np.isnan(row)  # (missing samples are skipped; an Inf stays and is refused below)
            if not ok.any() or wl[ok][0] > lo or wl[ok][-1] < hi:
                short.append(names[i])
                continue
            out[i] = np.interp(scene, wl[ok], row[ok])
        if short:
            raise ValueError(f"library entries that do not cover the scene's {lo:g}..{hi:g}: {_some(short)}")
        return cls(names, out, scene.tolist(), colors)

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def unit(self) -> torch.Tensor:
        """float32 [L,B]: the rows at unit length, normalised in float64 and rounded once (what the kernel takes)."""
        s = torch.from_numpy(self.spectra)
        return (s / s.norm(dim=1, keepdim=True)).float()

    def on(self, device):
        """(operand image, colours [L,3]) on ``device``, made once per device."""
        from . import ops

        key = str(torch.device(device))
        if key not in self._device_state:
            self._device_state[key] = (ops.library_prepare(self.unit().to(device)), torch.from_numpy(self.colors).to(device))
        return self._device_state[key]

    def match(self, spectra: torch.Tensor):
        """``ops.library_match`` of float32 device rows [...,B] against this library -> (index int32 [R,2], cos float32 [R,2])."""
        from . import ops

        if spectra.shape[-1] != len(self.wavelengths):
            raise ValueError(f"spectra of {spectra.shape[-1]} bands against a library resampled onto {len(self.wavelengths)}")
        if self._removed_with is not None:  # entries with their continuum divided out are matched by rows treated the same way
            spectra = self._removed_with.run(spectra, True, False)[0]
        return ops.library_match(spectra.float(), self.on(spectra.device)[0], len(self))

    def continuum_removed(self) -> "SpectralLibrary":
        """The library whose entries went through the host ``continuum.continuum_removed`` and whose ``match`` puts the rows through
        ``ops.continuum`` first (one more launch and one [R,B] temporary): absorption shapes are compared, not slope and albedo.  Made
        once.  ``ValueError`` for wavelengths that are not strictly increasing as float32."""
        from .continuum import ContinuumAnalysis, continuum_removed

        if self._removed_with is not None:
            return self
        if self._removed is None:
            analysis = ContinuumAnalysis(self.wavelengths)
            self._removed = SpectralLibrary(self.names, continuum_removed(self.spectra, analysis.wavelengths), self.wavelengths, self.colors)
            self._removed._removed_with = analysis
        return self._removed

    def classify(self, index: torch.Tensor, cos: torch.Tensor, accumulation: Optional[torch.Tensor] = None,
                 max_angle: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """The four outputs of R rays from the kernel's (index [R,2], cos [R,2]); pure torch, any device.
        ``library_angle`` [R,1] = acos(clamp(cos0, -1, 1)); ``library_margin`` [R,1] = acos(clamp(cos1, -1, 1)) - angle, how much
        further the runner-up is (pi - angle for a library of one entry); ``library_raw`` [R,1] = the best index as float32, -1 where
        nothing is rendered (``accumulation <= 0.5``, the rule of ``seg_pred``), where the kernel gave -1 (an empty or non-finite
        spectrum) or where angle > ``max_angle``; ``library_pred`` [R,3] = the entry's colour, black at -1.
        Angles below about 1e-3 rad are not resolved by a float32 cosine: near-duplicate entries tie and the earlier one wins."""
        c = cos.float().clamp(-1.0, 1.0)
        angle = torch.acos(c[:, 0])
        margin = torch.acos(c[:, 1]) - angle
        best = index[:, 0].long()
        matched = best >= 0
        if accumulation is not None:
            matched = matched & (accumulation.reshape(-1) > 0.5)
        if max_angle is not None:
            matched = matched & ~(angle > float(max_angle))
        raw = torch.where(matched, best, torch.full_like(best, -1))
        colors = torch.from_numpy(self.colors).to(index.device) if index.device.type == "cpu" else self.on(index.device)[1]
        pred = colors[raw.clamp(min=0)] * matched[:, None].to(colors.dtype)
        return {"library_raw": raw.float()[:, None], "library_pred": pred, "library_angle": angle[:, None], "library_margin": margin[:, None]}

    def frame_outputs(self, spectral: torch.Tensor, accumulation: Optional[torch.Tensor], max_angle: Optional[float] = None):
        """The four outputs of an assembled frame: ``spectral`` [H,W,B] (or [R,B]) and ``accumulation`` [H,W,1] -> [H,W,k] each."""
        lead = spectral.shape[:-1]
        index, cos = self.match(spectral)
        out = self.classify(index, cos, accumulation, max_angle)
        return {k: v.view(*lead, v.shape[-1]) for k, v in out.items()}


# ---- the endmembers and the eval split -------------------------------------------------------------------------------------------
def endmember_matches(library: SpectralLibrary, endmembers: torch.Tensor, top: int = 3) -> List[List[Dict]]:
    """Per row of the dictionary [C,B] (a device tensor) the ``top`` closest entries, closest first: [{"index", "name", "angle"}].
    The kernel gives two per call; further ones come from calls against the library without the entries already found."""
    from . import ops

    E = endmembers.detach().float()
    if library._removed_with is not None:  # (a continuum-removed library is compared with continuum-removed endmembers)
        E = library._removed_with.run(E.contiguous(), True, False)[0]
    unit = library.unit().to(E.device)
    rows: List[List[Dict]] = []
    for c in range(E.shape[0]):
        left, found = torch.arange(len(library), device=E.device), []
        while len(found) < top and left.numel() > 0:
            index, cos = ops.library_match(E[c:c + 1], ops.library_prepare(unit[left].contiguous()), int(left.numel()))
            got = [(int(left[i]), float(v)) for i, v in zip(index[0].tolist(), cos[0].tolist()) if i >= 0]
            if not got:
                break
            found += got
            keep = torch.ones(left.numel(), dtype=torch.bool, device=E.device)
            keep[index[0][index[0] >= 0].long()] = False
            left = left[keep]
        rows.append([{"index": i, "name": library.names[i], "angle": math.acos(max(-1.0, min(1.0, v)))} for i, v in found[:top]])
    return rows


class LibraryTally:
    """What ``eval --spectral-library`` counts over the split, on the device: per entry the matched pixels and the sum of their angles;
    the rendered pixels whose match equals the match of the captured spectrum at the same pixel.  Read once, by ``result``."""

    def __init__(self, library: SpectralLibrary, device):
        self.library = library
        self.count = torch.zeros(len(library), dtype=torch.float64, device=device)
        self.angle = torch.zeros(len(library), dtype=torch.float64, device=device)
        self.pixels = torch.zeros((), dtype=torch.float64, device=device)
        self.agree = torch.zeros(2, dtype=torch.float64, device=device)  # (agreeing, compared)

    def add(self, outputs: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        raw = outputs["library_raw"].reshape(-1).long()
        hit = raw >= 0
        at = raw[hit]
        self.count.index_add_(0, at, torch.ones_like(at, dtype=torch.float64))
        self.angle.index_add_(0, at, outputs["library_angle"].reshape(-1)[hit].double())
        self.pixels += raw.numel()
        if "hs_image" in batch:  # the same op on the ground truth
            gt = batch["hs_image"].to(raw.device).float()
            captured = self.library.match(gt.reshape(-1, gt.shape[-1]))[0][:, 0].long()
            self.agree += torch.stack([(captured[hit] == at).sum(), hit.sum()]).double()

    def result(self, model) -> Dict:
        count, angle, pixels, agree = self.count.cpu(), self.angle.cpu(), float(self.pixels), self.agree.cpu()
        order = sorted(range(len(count)), key=lambda i: (-float(count[i]), i))[:TOP_ENTRIES]
        top = [{"name": self.library.names[i], "share": float(count[i]) / max(pixels, 1.0), "mean_angle": float(angle[i] / count[i])}
               for i in order if count[i] > 0]
        return {"library_top": top, "library_agreement": float(agree[0] / agree[1]) if agree[1] > 0 else None,
                "endmember_matches": endmember_matches(self.library, model.field.endmembers)}


def load_for_model(path, model) -> Optional[SpectralLibrary]:
    """``--spectral-library FILE`` for a built model (None: no library)."""
    return None if path is None else SpectralLibrary.load(path, scene_wavelengths(model))


def add_library_arguments(p) -> None:
    p.add_argument("--spectral-library", default=None, metavar="FILE",
                   help="match every pixel's spectrum against this library (.npz / .csv, INTEGRATION.md): library_raw, library_pred, "
                        "library_angle, library_margin")
    p.add_argument("--library-max-angle", type=float, default=None, metavar="RAD",
                   help="leave a pixel unmatched when its best spectral angle is above this")


# ---- command line ----------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .eval import add_model_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.library", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    ident = sub.add_parser("identify", help="name the learnt endmembers: the closest library entries of each, with their angles")
    add_model_arguments(ident)
    ident.add_argument("--spectral-library", required=True, metavar="FILE")
    ident.add_argument("--top", type=int, default=3)
    return ap


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint

    args = build_parser().parse_args(argv)
    if args.top < 1:
        raise ValueError("--top must be at least 1")
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    model = pipeline.model
    if model.config.method == "rgb":
        raise NotImplementedError("identify needs a spectral method (spectral, rgb+spectral): method=\"rgb\" has no endmembers")
    library = load_for_model(args.spectral_library, model)
    rows = endmember_matches(library, model.field.endmembers, args.top)
    for c, row in enumerate(rows):
        print(f"endmember {c}: " + "; ".join(f"{m['name']} ({m['angle']:.4f} rad)" for m in row))
    result = {"spectral_library": str(args.spectral_library), "endmember_matches": rows}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
