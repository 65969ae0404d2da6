"""Classical linear unmixing: per pixel the abundances a >= 0 that minimise |x - E^T a|^2 against K <= 16 endmembers -- with sum a = 1
(FCLS, the default) or without (NNLS).  It answers what the method itself raises: do the abundances the network learnt agree with what
a textbook solver gets from the same endmembers?

``Unmixer.from_model(model)`` takes the learnt endmembers, ``Unmixer.from_library(library, entries)`` named reflectances of a spectral
library; ``UMHSModel.unmixing_context(unmixer)`` makes a render emit ``unmix_0`` .., ``unmix``, ``unmix_raw``, ``unmix_pred`` and
``unmix_residual``; ``--unmix model|library`` does so on the render and eval command lines, and

    python -m umhsnerf.unmix captured --load-config RUN/config.json --split train --output-path OUT

unmixes the captured ``hs_image`` stack of a split without rendering anything.  The solver is one HIP kernel (``ops.unmix``,
csrc/umhs_unmix.hip) on float32 normal equations; everything here is host code in float64 on K x K matrices, or torch on [R]-sized
tensors.

Conditioning: float32 normal equations lose about u cond_2(E E^T) of an abundance (u = 2^-24).  An endmember set for which
``ABUNDANCE_BOUND`` x cond_2 exceeds 0.01 -- nearly dependent spectra -- is refused, naming its two most collinear endmembers."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_ENDMEMBERS, MAX_BANDS = 16, 256  # the kernel's limits (include/umhs_hip.h)
CONSTRAINTS = {"nnls": 0, "fcls": 1}  # UMHS_UNMIX_NNLS, UMHS_UNMIX_FCLS
ABUNDANCE_BOUND = 8.0 * 2.0 ** -24  # K_A u of tests/unmix_f64.py: |a - a*| <= K_A u cond_2(G) max(1, |a*|)
MAX_ABUNDANCE_ERROR = 0.01
FIXED_OUTPUTS = ("unmix", "unmix_raw", "unmix_pred", "unmix_residual")


def unmix_index(name: str) -> Optional[int]:
    """k of ``unmix_<k>``, else None."""
    if name.startswith("unmix_") and name[6:].isdigit():
        return int(name[6:])
    return None


def is_unmix_output(name: str) -> bool:
    return name in FIXED_OUTPUTS or unmix_index(name) is not None


def unmix_outputs(K: int) -> Tuple[str, ...]:
    """The names a context of K endmembers offers."""
    return (*(f"unmix_{k}" for k in range(K)), *FIXED_OUTPUTS)


def requested_without_unmix(names: Sequence[str], unmix) -> None:
    """``ValueError`` naming the flag when a render asks for an unmixing output without ``--unmix``."""
    asked = [n for n in names if is_unmix_output(n)]
    if asked and unmix is None:
        raise ValueError(f"{', '.join(asked[:5])}: unmixing outputs need the endmembers to unmix against; pass --unmix model or "
                         "--unmix library --unmix-entries NAME ...")


def conditioning(endmembers: np.ndarray) -> Dict:
    """cond_2(E E^T) in float64 and the two most collinear rows (largest cosine): {"cond", "pair", "cosine"}."""
    E = np.asarray(endmembers, np.float64)
    G = E @ E.T
    lam = np.linalg.eigvalsh(G)
    cond = float(lam[-1] / lam[0]) if lam[0] > 0 else float("inf")
    pair, cosine = (0, 0), 1.0
    if E.shape[0] > 1:
        n = np.sqrt(np.diag(G))
        c = G / np.maximum(np.outer(n, n), 1e-300)
        c[np.tril_indices(E.shape[0])] = -np.inf
        pair = tuple(int(i) for i in np.unravel_index(int(np.argmax(c)), c.shape))
        cosine = float(c[pair])
    return {"cond": cond, "pair": pair, "cosine": cosine}


class Unmixer:
    """K named endmembers on the scene's B bands and the constraint they are unmixed under.  ``endmembers`` [K,B] is rounded to float32
    (what the kernel reads); the Gram matrix is formed from those float32 values in float64 and rounded once."""

    def __init__(self, endmembers, names: Optional[Sequence[str]] = None, colors=None, constraint: str = "fcls"):
        from .umhs_model import CLASS_COLORS

        E = endmembers.detach().cpu().numpy() if torch.is_tensor(endmembers) else np.asarray(endmembers)
        if E.ndim != 2:
            raise ValueError(f"endmembers must be [K,B], got {E.shape}")
        self.endmembers = np.ascontiguousarray(E, dtype=np.float32)
        K, B = self.endmembers.shape
        if not 1 <= K <= MAX_ENDMEMBERS or not 1 <= B <= MAX_BANDS:
            raise ValueError(f"{K} endmembers on {B} bands are outside what the unmixing kernel takes: 1..{MAX_ENDMEMBERS} endmembers, "
                             f"1..{MAX_BANDS} bands")
        if constraint not in CONSTRAINTS:
            raise ValueError(f"constraint must be one of {', '.join(CONSTRAINTS)}, got {constraint!r}")
        self.constraint, self.mode = constraint, CONSTRAINTS[constraint]
        self.names = [f"endmember_{k}" for k in range(K)] if names is None else [str(n) for n in names]
        if len(self.names) != K:
            raise ValueError(f"{len(self.names)} names for {K} endmembers")
        if not np.isfinite(self.endmembers).all():
            raise ValueError("an endmember holds a value that is not finite")
        if colors is None:
            palette = CLASS_COLORS.numpy()
            colors = palette[np.arange(K) % len(palette)]
        colors = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
        self.colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if self.colors.shape[0] != K:
            raise ValueError(f"colors must be [{K},3], got {self.colors.shape}")
        c = self.conditioning = conditioning(self.endmembers)
        if not ABUNDANCE_BOUND * c["cond"] <= MAX_ABUNDANCE_ERROR:
            i, j = c["pair"]
            raise ValueError(f"the endmembers are too close to dependent to unmix in float32: cond_2(E E^T) = {c['cond']:.3g} puts the "
                             f"abundance error bound at {ABUNDANCE_BOUND * c['cond']:.3g} (> {MAX_ABUNDANCE_ERROR}); the two most collinear "
                             f"are {self.names[i]!r} and {self.names[j]!r} (cosine {c['cosine']:.6f}): drop one of them")
        E64 = self.endmembers.astype(np.float64)
        self.gram = (E64 @ E64.T).astype(np.float32)
        self._device_state: Dict = {}

    def __len__(self) -> int:
        return self.endmembers.shape[0]

    @property
    def bands(self) -> int:
        return self.endmembers.shape[1]

    @classmethod
    def from_model(cls, model, constraint: str = "fcls") -> "Unmixer":
        """The learnt endmembers (``field.endmembers`` clamped to [0,1], as the renderer uses them) with the model's class colours."""
        if model.config.method == "rgb":
            raise NotImplementedError("unmixing needs a spectral method (spectral, rgb+spectral): method=\"rgb\" has no endmembers")
        E = model.field.endmembers.detach().float().clamp(0.0, 1.0)
        return cls(E, None, model.class_colors[torch.arange(E.shape[0]) % model.class_colors.shape[0]], constraint)

    @classmethod
    def from_library(cls, library, entries: Sequence, constraint: str = "fcls") -> "Unmixer":
        """Named (or indexed) rows of a ``SpectralLibrary`` that is already resampled onto the scene's wavelengths, at most 16."""
        entries = list(entries)
        if not 1 <= len(entries) <= MAX_ENDMEMBERS:
            raise ValueError(f"{len(entries)} library entries to unmix against: the kernel takes 1..{MAX_ENDMEMBERS} (--unmix-entries)")
        rows = []
        for e in entries:
            if isinstance(e, (int, np.integer)) or (isinstance(e, str) and e not in library.names and e.lstrip("-").isdigit()):
                i = int(e)
                if not 0 <= i < len(library):
                    raise ValueError(f"library entry {i} is outside 0..{len(library) - 1}")
            elif e in library.names:
                i = library.names.index(e)
            else:
                raise ValueError(f"the library has no entry named {e!r}; it holds {', '.join(library.names[:5])}"
                                 + (f" (and {len(library) - 5} more)" if len(library) > 5 else ""))
            rows.append(i)
        if len(set(rows)) != len(rows):
            raise ValueError("a library entry is named twice in --unmix-entries")
        return cls(library.spectra[rows], [library.names[i] for i in rows], library.colors[rows], constraint)

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def on(self, device):
        """(operand image of E, gram float32 [K,K], colours [K,3]) on ``device``, made once per device."""
        from . import ops

        key = str(torch.device(device))
        if key not in self._device_state:
            E = torch.from_numpy(self.endmembers).to(device)
            self._device_state[key] = (ops.library_prepare(E), torch.from_numpy(self.gram).to(device).contiguous(),
                                       torch.from_numpy(self.colors).to(device))
        return self._device_state[key]

    def unmix(self, spectra: torch.Tensor, want_residual: bool = True, want_status: bool = False):
        """``ops.unmix`` of float32 device rows [...,B] -> (abundances [R,K], residual [R] | None, status [R] | None)."""
        from . import ops

        if spectra.shape[-1] != self.bands:
            raise ValueError(f"spectra of {spectra.shape[-1]} bands against endmembers of {self.bands}")
        image, gram, _ = self.on(spectra.device)
        return ops.unmix(spectra.float(), image, gram, len(self), self.mode, want_residual, want_status)

    def frame_outputs(self, spectral: torch.Tensor, accumulation: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The outputs of an assembled frame, by ONE ``ops.unmix`` launch: ``spectral`` [H,W,B] (or [R,B]) and ``accumulation`` [H,W,1]
        (or None) -> ``unmix`` [H,W,K] and ``unmix_k`` [H,W,1], the abundances; ``unmix_raw`` [H,W,1], their argmax as float32 (-1 where
        nothing is rendered or the spectrum is empty or not finite); ``unmix_pred`` [H,W,3], its colour; ``unmix_residual`` [H,W,1] =
        sqrt(|x - E^T a|^2 / B), the RMS misfit.  Everything is 0 (and -1) where ``accumulation <= 0.5``."""
        lead, K = spectral.shape[:-1], len(self)
        a, res, status = self.unmix(spectral, True, True)
        solved = status != -1
        if accumulation is not None:
            solved = solved & (accumulation.reshape(-1) > 0.5)
        a = torch.where(solved[:, None], a, torch.zeros_like(a))
        rms = torch.where(solved, torch.sqrt(res / float(self.bands)), torch.zeros_like(res))
        best = a.argmax(1)
        raw = torch.where(solved, best, torch.full_like(best, -1))
        colors = self.on(spectral.device)[2]
        out = {"unmix": a.view(*lead, K), "unmix_raw": raw.float().view(*lead, 1),
               "unmix_pred": (colors[best] * solved[:, None].to(colors.dtype)).view(*lead, 3), "unmix_residual": rms.view(*lead, 1)}
        for k in range(K):
            out[f"unmix_{k}"] = a[:, k].contiguous().view(*lead, 1)
        return out


class UnmixTally:
    """What ``eval --unmix`` sums over the split, on the device, over the pixels with rendered ``accumulation > 0.5``: the squared
    difference between the rendered ``abundances`` and the unmixing of the CAPTURED spectrum (``compare_abundances``: with the learnt
    endmembers, where the two are the same quantity), the pixels whose argmax agree, both RMS misfits, and the captured rows stopped at
    the solver's cap.  Read once, by ``result``."""

    def __init__(self, unmixer: Unmixer, device, compare_abundances: bool):
        self.unmixer, self.compare = unmixer, bool(compare_abundances)
        K = len(unmixer)
        self.square = torch.zeros(K, dtype=torch.float64, device=device)
        self.sums = torch.zeros(5, dtype=torch.float64, device=device)  # pixels, agreeing, captured rms, rendered rms, capped

    def add(self, outputs: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        if "hs_image" not in batch:
            return
        K = len(self.unmixer)
        counted = outputs["accumulation"].reshape(-1) > 0.5
        gt = batch["hs_image"].to(counted.device).float().reshape(-1, self.unmixer.bands)
        a, res, status = self.unmixer.unmix(gt, True, True)
        w = counted.double()
        rendered = outputs["abundances"].reshape(-1, K).double() if self.compare else outputs["unmix"].reshape(-1, K).double()
        if self.compare:
            self.square += ((rendered - a.double()) ** 2 * w[:, None]).sum(0)
        agree = (rendered.argmax(1) == a.argmax(1)) & counted
        captured_rms = torch.sqrt(res.double() / self.unmixer.bands)
        self.sums += torch.stack([w.sum(), agree.sum().double(), (captured_rms * w).sum(),
                                  (outputs["unmix_residual"].reshape(-1).double() * w).sum(), ((status == -2) & counted).sum().double()])

    def result(self) -> Dict:
        s, sq = self.sums.cpu().tolist(), self.square.cpu().numpy()
        n, K = s[0], len(self.unmixer)
        if n <= 0:
            return {"unmix_abundance_rmse": None, "unmix_abundance_rmse_per_material": None, "unmix_agreement": None,
                    "unmix_residual_captured": None, "unmix_residual_rendered": None, "unmix_cap_share": None}
        return {"unmix_abundance_rmse": float(np.sqrt(sq.sum() / (n * K))) if self.compare else None,
                "unmix_abundance_rmse_per_material": [float(v) for v in np.sqrt(sq / n)] if self.compare else None,
                "unmix_agreement": s[1] / n, "unmix_residual_captured": s[2] / n, "unmix_residual_rendered": s[3] / n,
                "unmix_cap_share": s[4] / n}


# ---- command-line plumbing shared with render and eval ---------------------------------------------------------------------------
def add_unmix_arguments(p) -> None:
    p.add_argument("--unmix", default=None, choices=["model", "library"],
                   help="unmix every pixel against the learnt endmembers (model) or entries of --spectral-library (library): unmix_<k>, "
                        "unmix, unmix_raw, unmix_pred, unmix_residual")
    p.add_argument("--unmix-entries", nargs="+", default=None, metavar="NAME", help="with --unmix library: the entries (names or indices), at most 16")
    p.add_argument("--unmix-constraint", default="fcls", choices=list(CONSTRAINTS), help="fcls: a >= 0 and sum a = 1; nnls: a >= 0 alone")


def check_unmix_arguments(args, names: Sequence[str] = ()) -> None:
    """The refusals that need no file: an unmixing output without ``--unmix``; ``library`` without ``--spectral-library`` or without
    entries; entries without ``library``; more than 16 entries.  ``ValueError``."""
    requested_without_unmix(names, args.unmix)
    if args.unmix == "library":
        if getattr(args, "spectral_library", None) is None:
            raise ValueError("--unmix library unmixes against entries of a spectral library: pass --spectral-library FILE")
        if not args.unmix_entries:
            raise ValueError("--unmix library needs the entries to unmix against: pass --unmix-entries NAME ...")
        if len(args.unmix_entries) > MAX_ENDMEMBERS:
            raise ValueError(f"--unmix-entries names {len(args.unmix_entries)} entries: the unmixing kernel takes at most {MAX_ENDMEMBERS}")
    elif args.unmix_entries:
        raise ValueError("--unmix-entries goes with --unmix library")


def unmixer_from_args(args, model, library=None) -> Optional[Unmixer]:
    """The ``Unmixer`` of the flags for a built model (None: the flag is absent).  ``library``: the loaded ``--spectral-library``."""
    if args.unmix is None:
        return None
    check_unmix_arguments(args)
    if args.unmix == "model":
        return Unmixer.from_model(model, args.unmix_constraint)
    return Unmixer.from_library(library, args.unmix_entries, args.unmix_constraint)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .eval import add_model_arguments
    from .library import add_library_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.unmix", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    cap = sub.add_parser("captured", help="unmix the captured hs_image stack of a split; no model run")
    add_model_arguments(cap)
    add_library_arguments(cap)
    add_unmix_arguments(cap)
    cap.set_defaults(unmix="model")
    cap.add_argument("--split", default="train", choices=["train", "val", "test"])
    cap.add_argument("--output-path", required=True, metavar="OUT", help="directory for <stem>_unmix.npy [H,W,K] and summary.json")
    return ap


def unmix_captured(pipeline, unmixer: Unmixer, split: str, output_path) -> List[Dict]:
    """Every frame of the split's ``hs_image`` stack through ``ops.unmix``: ``OUT/<stem>_unmix.npy`` float32 [H,W,K] per frame and its
    summary {"frame", "mean_abundance" [K], "mean_residual" (RMS misfit), "invalid", "capped"} over the valid pixels."""
    dm = pipeline.datamanager
    resident = dm.train_split if split == "train" else dm.eval_split
    stack = getattr(resident, "hs_image", None)
    if stack is None:
        raise ValueError(f"the {split} split has no hyperspectral stack (hs_image): nothing captured to unmix")
    dataset = dm.train_dataset if split == "train" else dm.eval_dataset
    filenames = getattr(dataset, "image_filenames", None)
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    device, K = pipeline.model.device, len(unmixer)
    frames = []
    for i in range(stack.shape[0]):  # (a host-resident stack is uploaded a frame at a time)
        frame = stack[i].to(device).float()
        a, res, status = unmixer.unmix(frame, True, True)
        valid = (status != -1).double()
        n = valid.sum().clamp(min=1.0)
        sums = torch.cat([(a.double() * valid[:, None]).sum(0) / n, ((torch.sqrt(res.double() / unmixer.bands) * valid).sum() / n)[None],
                          (status == -1).sum().double()[None], (status == -2).sum().double()[None]]).cpu().tolist()  # (the frame's one read)
        stem = Path(str(filenames[i])).stem if filenames is not None and i < len(filenames) else f"frame_{i:05d}"
        np.save(output_path / f"{stem}_unmix.npy", a.view(*frame.shape[:-1], K).cpu().numpy())
        frames.append({"frame": stem, "mean_abundance": sums[:K], "mean_residual": sums[K], "invalid": int(sums[K + 1]),
                       "capped": int(sums[K + 2])})
    return frames


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from . import library as spectral_library

    args = build_parser().parse_args(argv)
    check_unmix_arguments(args)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    library = spectral_library.load_for_model(args.spectral_library, pipeline.model)
    unmixer = unmixer_from_args(args, pipeline.model, library)
    frames = unmix_captured(pipeline, unmixer, args.split, args.output_path)
    result = {"output_path": str(args.output_path), "split": args.split, "unmix": args.unmix, "constraint": unmixer.constraint,
              "endmembers": unmixer.names, "cond": unmixer.conditioning["cond"], "frames": frames}
    (Path(args.output_path) / "summary.json").write_text(json.dumps(result))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
