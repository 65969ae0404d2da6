"""Sparse unmixing: every pixel against a WHOLE spectral library (up to 128 entries) -- the few entries, with non-negative abundances,
that explain its spectrum.  It is the non-negative lasso  min 1/2 |x - A^T a|^2 + lambda |x| sum a,  a >= 0,  solved per pixel by ADMM
as in SUnSAL (Bioucas-Dias and Figueiredo, 2010).  Library matching names one entry per pixel and gives no abundances; ``--unmix
library`` gives abundances against at most 16 entries picked by hand; this needs no picking.

``SparseUnmixer(library)`` takes a ``SpectralLibrary`` already resampled onto the scene's wavelengths (optionally a subset of its
entries); ``UMHSModel.sparse_unmixing_context(unmixer)`` makes a render emit ``sparse_0`` .., ``sparse``, ``sparse_raw``,
``sparse_pred``, ``sparse_count`` and ``sparse_residual``; ``--sparse-unmix`` does so on the render and eval command lines, and

    python -m umhsnerf.sparse captured --load-config RUN/config.json --spectral-library lib.npz --split train --output-path OUT

unmixes the captured ``hs_image`` stack of a split without rendering anything.  The solver is one HIP kernel (``ops.sparse_unmix``,
csrc/umhs_sparse.hip); everything here is host code in float64 on L x L matrices, or torch on [R]-sized tensors.

The ADMM penalty mu only sets the speed: ``auto`` is 0.1 trace(A A^T) / L, the fastest of {0.01, 0.03, 0.1, 0.3, 1} on the test cases
(DESIGN.md has the table)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_ENTRIES, MAX_BANDS = 128, 256  # the kernel's limits (include/umhs_hip.h)
DEFAULT_LAMBDA, DEFAULT_EPSILON, DEFAULT_MAX_ITERATIONS = 1e-3, 1e-4, 400
FIXED_OUTPUTS = ("sparse", "sparse_raw", "sparse_pred", "sparse_count", "sparse_residual")
TOP = 16  # entries listed by eval's sparse_top


def sparse_index(name: str) -> Optional[int]:
    """k of ``sparse_<k>``, else None."""
    if name.startswith("sparse_") and name[7:].isdigit():
        return int(name[7:])
    return None


def is_sparse_output(name: str) -> bool:
    return name in FIXED_OUTPUTS or sparse_index(name) is not None


def sparse_outputs(L: int) -> Tuple[str, ...]:
    """The names a context of L entries offers."""
    return (*(f"sparse_{k}" for k in range(L)), *FIXED_OUTPUTS)


def requested_without_sparse(names: Sequence[str], sparse_unmix) -> None:
    """``ValueError`` naming the flag when a render asks for a sparse-unmixing output without ``--sparse-unmix``."""
    asked = [n for n in names if is_sparse_output(n)]
    if asked and not sparse_unmix:
        raise ValueError(f"{', '.join(asked[:5])}: sparse-unmixing outputs need a library to unmix against; pass --sparse-unmix "
                         "--spectral-library FILE")


def _entry_rows(library, entries: Sequence) -> List[int]:
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
        raise ValueError("a library entry is named twice in --sparse-entries")
    return rows


class SparseUnmixer:
    """The entries of a ``SpectralLibrary`` (all of them, or ``entries``: names or indices) on the scene's B bands, and the solver's
    settings.  The spectra are rounded to float32 (what the kernel reads); the operands are formed from those in float64."""

    def __init__(self, library, entries: Optional[Sequence] = None, lambda_: float = DEFAULT_LAMBDA, epsilon: float = DEFAULT_EPSILON,
                 max_iterations: int = DEFAULT_MAX_ITERATIONS, mu="auto"):
        rows = list(range(len(library))) if entries is None else _entry_rows(library, list(entries))
        if not 1 <= len(rows) <= MAX_ENTRIES:
            raise ValueError(f"{len(rows)} library entries to unmix against: the sparse-unmixing kernel takes 1..{MAX_ENTRIES}; name a "
                             "subset with --sparse-entries")
        self.spectra = np.ascontiguousarray(np.asarray(library.spectra)[rows], dtype=np.float32)
        if not 1 <= self.spectra.shape[1] <= MAX_BANDS:
            raise ValueError(f"{self.spectra.shape[1]} bands are outside what the sparse-unmixing kernel takes: 1..{MAX_BANDS}")
        if not np.isfinite(self.spectra).all():
            raise ValueError("a library entry holds a value that is not finite")
        self.names = [library.names[i] for i in rows]
        self.colors = np.asarray(library.colors, dtype=np.float32)[rows].reshape(-1, 3)
        self.lambda_, self.epsilon, self.max_iterations = float(lambda_), float(epsilon), int(max_iterations)
        if not self.lambda_ >= 0.0 or not np.isfinite(self.lambda_):
            raise ValueError(f"--sparse-lambda must be finite and >= 0, got {lambda_}")
        if not self.epsilon > 0.0 or not np.isfinite(self.epsilon):
            raise ValueError(f"--sparse-epsilon must be finite and > 0, got {epsilon}")
        if self.max_iterations < 1:
            raise ValueError(f"--sparse-max-iterations must be at least 1, got {max_iterations}")
        A64 = self.spectra.astype(np.float64)
        trace = float((A64 * A64).sum())
        if not trace > 0.0:
            raise ValueError("every library entry is zero: nothing to unmix against")
        from .ops.sparse import SPARSE_RHO

        if isinstance(mu, str):
            if mu != "auto":
                mu = float(mu)  # ValueError for anything that is neither
        self.mu = SPARSE_RHO * trace / len(rows) if isinstance(mu, str) else float(mu)
        self.mu_rule = "auto" if isinstance(mu, str) else "given"
        if not self.mu > 0.0 or not np.isfinite(self.mu):
            raise ValueError(f"--sparse-mu must be auto or a finite number > 0, got {mu}")
        self._device_state: Dict = {}

    def __len__(self) -> int:
        return self.spectra.shape[0]

    @property
    def bands(self) -> int:
        return self.spectra.shape[1]

    def summary(self) -> Dict:
        return {"entries": len(self), "lambda": self.lambda_, "epsilon": self.epsilon, "max_iterations": self.max_iterations,
                "mu": self.mu, "mu_rule": self.mu_rule}

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def on(self, device):
        """(``ops.SparseOperands``, colours [L,3]) on ``device``, made once per device."""
        from . import ops

        key = str(torch.device(device))
        if key not in self._device_state:
            self._device_state[key] = (ops.sparse_prepare(torch.from_numpy(self.spectra).to(device), self.lambda_, self.mu),
                                       torch.from_numpy(self.colors).to(device))
        return self._device_state[key]

    def unmix(self, spectra: torch.Tensor, want_residual: bool = True, want_status: bool = False):
        """``ops.sparse_unmix`` of float32 device rows [...,B] -> (abundances [R,L], residual [R] | None, status [R] | None)."""
        from . import ops

        if spectra.shape[-1] != self.bands:
            raise ValueError(f"spectra of {spectra.shape[-1]} bands against a library of {self.bands}")
        return ops.sparse_unmix(spectra.float(), self.on(spectra.device)[0], self.epsilon, self.max_iterations, want_residual, want_status)

    def frame_outputs(self, spectral: torch.Tensor, accumulation: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The outputs of an assembled frame, by ONE ``ops.sparse_unmix`` launch: ``spectral`` [H,W,B] (or [R,B]) and ``accumulation``
        [H,W,1] (or None) -> ``sparse`` [H,W,L] and ``sparse_k`` [H,W,1], the abundances; ``sparse_count`` [H,W,1], how many are > 0;
        ``sparse_raw`` [H,W,1], the index of the largest as float32 (-1 where nothing is rendered, the spectrum is empty or not finite,
        or nothing is active); ``sparse_pred`` [H,W,3], that entry's library colour; ``sparse_residual`` [H,W,1] =
        sqrt(|x - A^T a|^2 / B), the RMS misfit.  Everything is 0 (and -1) where ``accumulation <= 0.5``."""
        lead, L = spectral.shape[:-1], len(self)
        a, res, status = self.unmix(spectral, True, True)
        solved = status != -1
        if accumulation is not None:
            solved = solved & (accumulation.reshape(-1) > 0.5)
        a = torch.where(solved[:, None], a, torch.zeros_like(a))
        rms = torch.where(solved, torch.sqrt(res / float(self.bands)), torch.zeros_like(res))
        count = (a > 0).sum(1)
        named = solved & (count > 0)
        best = a.argmax(1)
        raw = torch.where(named, best, torch.full_like(best, -1))
        colors = self.on(spectral.device)[1]
        out = {"sparse": a.view(*lead, L), "sparse_raw": raw.float().view(*lead, 1), "sparse_count": count.float().view(*lead, 1),
               "sparse_pred": (colors[best] * named[:, None].to(colors.dtype)).view(*lead, 3), "sparse_residual": rms.view(*lead, 1)}
        for k in range(L):
            out[f"sparse_{k}"] = a[:, k].contiguous().view(*lead, 1)
        return out


class SparseTally:
    """What ``eval --sparse-unmix`` sums over the split, on the device, over the pixels with rendered ``accumulation > 0.5``: per entry
    the abundance and the active pixels of the RENDERED spectrum's unmixing; the active count; the pixels whose dominant entry is the
    one of the CAPTURED spectrum (``hs_image``) at the same pixel; both RMS misfits; the captured rows stopped at the iteration cap.
    Read once, by ``result``."""

    def __init__(self, unmixer: SparseUnmixer, device):
        self.unmixer = unmixer
        L = len(unmixer)
        self.abundance = torch.zeros(L, dtype=torch.float64, device=device)
        self.active = torch.zeros(L, dtype=torch.float64, device=device)
        self.sums = torch.zeros(7, dtype=torch.float64, device=device)  # pixels, count, rendered rms, compared, agreeing, captured rms, capped

    def add(self, outputs: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> None:
        L = len(self.unmixer)
        counted = outputs["accumulation"].reshape(-1) > 0.5
        w = counted.double()
        rendered = outputs["sparse"].reshape(-1, L)
        self.abundance += (rendered.double() * w[:, None]).sum(0)
        self.active += ((rendered > 0).double() * w[:, None]).sum(0)
        self.sums[:3] += torch.stack([w.sum(), (outputs["sparse_count"].reshape(-1).double() * w).sum(),
                                      (outputs["sparse_residual"].reshape(-1).double() * w).sum()])
        if "hs_image" not in batch:
            return
        gt = batch["hs_image"].to(counted.device).float().reshape(-1, self.unmixer.bands)
        a, res, status = self.unmixer.unmix(gt, True, True)
        dominant = torch.where((status != -1) & ((a > 0).sum(1) > 0), a.argmax(1), torch.full_like(status, -1, dtype=torch.int64))
        agree = (outputs["sparse_raw"].reshape(-1).long() == dominant) & counted
        self.sums[3:] += torch.stack([w.sum(), agree.sum().double(), (torch.sqrt(res.double() / self.unmixer.bands) * w).sum(),
                                      ((status == -2) & counted).sum().double()])

    def result(self) -> Dict:
        s = self.sums.cpu().tolist()
        n, m = s[0], s[3]
        if n <= 0:
            return {"sparse_top": None, "sparse_mean_count": None, "sparse_agreement": None, "sparse_residual_rendered": None,
                    "sparse_residual_captured": None, "sparse_cap_share": None}
        mean, share = (self.abundance / n).cpu().numpy(), (self.active / n).cpu().numpy()
        order = np.argsort(-mean, kind="stable")[:TOP]
        return {"sparse_top": [{"name": self.unmixer.names[k], "mean_abundance": float(mean[k]), "active_share": float(share[k])}
                               for k in order],
                "sparse_mean_count": s[1] / n, "sparse_agreement": s[4] / m if m > 0 else None, "sparse_residual_rendered": s[2] / n,
                "sparse_residual_captured": s[5] / m if m > 0 else None, "sparse_cap_share": s[6] / m if m > 0 else None}


# ---- command-line plumbing shared with render and eval ---------------------------------------------------------------------------
def _mu_argument(text: str):
    if text == "auto":
        return text
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"auto or a number > 0, got {text!r}")
    if not value > 0.0 or not np.isfinite(value):
        raise argparse.ArgumentTypeError(f"auto or a number > 0, got {text!r}")
    return value


def add_sparse_arguments(p) -> None:
    p.add_argument("--sparse-unmix", action="store_true",
                   help="unmix every pixel against the whole --spectral-library (non-negative lasso): sparse_<k>, sparse, sparse_raw, "
                        "sparse_pred, sparse_count, sparse_residual")
    p.add_argument("--sparse-lambda", type=float, default=DEFAULT_LAMBDA, metavar="X",
                   help="the sparsity penalty, relative to the pixel's norm (0: plain non-negative least squares)")
    p.add_argument("--sparse-epsilon", type=float, default=DEFAULT_EPSILON, metavar="X", help="the relative tolerance the iteration stops at")
    p.add_argument("--sparse-max-iterations", type=int, default=DEFAULT_MAX_ITERATIONS, metavar="N", help="the iteration cap per pixel")
    p.add_argument("--sparse-mu", type=_mu_argument, default="auto", metavar="auto|X", help="the ADMM penalty (auto: 0.1 trace(A A^T) / L)")
    p.add_argument("--sparse-entries", nargs="+", default=None, metavar="NAME",
                   help=f"unmix against these entries only (names or indices), at most {MAX_ENTRIES}")


def check_sparse_arguments(args, names: Sequence[str] = ()) -> None:
    """The refusals that need no file: a sparse output without ``--sparse-unmix``; the flag without ``--spectral-library``; its options
    without the flag; more than 128 entries named; scalars out of range.  ``ValueError``."""
    requested_without_sparse(names, args.sparse_unmix)
    if not args.sparse_unmix:
        if args.sparse_entries:
            raise ValueError("--sparse-entries goes with --sparse-unmix")
        return
    if getattr(args, "spectral_library", None) is None:
        raise ValueError("--sparse-unmix unmixes against a spectral library: pass --spectral-library FILE")
    if args.sparse_entries and len(args.sparse_entries) > MAX_ENTRIES:
        raise ValueError(f"--sparse-entries names {len(args.sparse_entries)} entries: the sparse-unmixing kernel takes at most {MAX_ENTRIES}")
    if not args.sparse_lambda >= 0.0 or not np.isfinite(args.sparse_lambda):
        raise ValueError(f"--sparse-lambda must be finite and >= 0, got {args.sparse_lambda}")
    if not args.sparse_epsilon > 0.0 or not np.isfinite(args.sparse_epsilon):
        raise ValueError(f"--sparse-epsilon must be finite and > 0, got {args.sparse_epsilon}")
    if args.sparse_max_iterations < 1:
        raise ValueError(f"--sparse-max-iterations must be at least 1, got {args.sparse_max_iterations}")


def sparse_unmixer_from_args(args, library=None) -> Optional[SparseUnmixer]:
    """The ``SparseUnmixer`` of the flags (None: the flag is absent).  ``library``: the loaded ``--spectral-library``."""
    if not args.sparse_unmix:
        return None
    check_sparse_arguments(args)
    return SparseUnmixer(library, args.sparse_entries, args.sparse_lambda, args.sparse_epsilon, args.sparse_max_iterations, args.sparse_mu)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .eval import add_model_arguments
    from .library import add_library_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.sparse", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    cap = sub.add_parser("captured", help="unmix the captured hs_image stack of a split against the library; no model run")
    add_model_arguments(cap)
    add_library_arguments(cap)
    add_sparse_arguments(cap)
    cap.set_defaults(sparse_unmix=True)
    cap.add_argument("--split", default="train", choices=["train", "val", "test"])
    cap.add_argument("--output-path", required=True, metavar="OUT", help="directory for <stem>_sparse.npy [H,W,L] and summary.json")
    return ap


def sparse_captured(pipeline, unmixer: SparseUnmixer, split: str, output_path) -> Dict:
    """Every frame of the split's ``hs_image`` stack through ``ops.sparse_unmix``: ``OUT/<stem>_sparse.npy`` float32 [H,W,L] per frame.
    Returns {"entries": per entry its name, mean abundance and active share over the valid pixels of the split, "mean_count",
    "mean_residual" (RMS misfit), "frames": per frame {"frame", "invalid", "capped"}}."""
    dm = pipeline.datamanager
    resident = dm.train_split if split == "train" else dm.eval_split
    stack = getattr(resident, "hs_image", None)
    if stack is None:
        raise ValueError(f"the {split} split has no hyperspectral stack (hs_image): nothing captured to unmix")
    dataset = dm.train_dataset if split == "train" else dm.eval_dataset
    filenames = getattr(dataset, "image_filenames", None)
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    device, L = pipeline.model.device, len(unmixer)
    total = torch.zeros(2 * L + 3, dtype=torch.float64, device=device)  # abundance [L], active [L], valid pixels, count, rms
    frames = []
    for i in range(stack.shape[0]):  # (a host-resident stack is uploaded a frame at a time)
        frame = stack[i].to(device).float()
        a, res, status = unmixer.unmix(frame, True, True)
        valid = (status != -1).double()
        active = (a > 0).double() * valid[:, None]
        total += torch.cat([(a.double() * valid[:, None]).sum(0), active.sum(0), valid.sum()[None], active.sum()[None],
                            (torch.sqrt(res.double() / unmixer.bands) * valid).sum()[None]])
        bad = torch.stack([(status == -1).sum(), (status == -2).sum()]).cpu().tolist()  # (the frame's one read)
        stem = Path(str(filenames[i])).stem if filenames is not None and i < len(filenames) else f"frame_{i:05d}"
        np.save(output_path / f"{stem}_sparse.npy", a.view(*frame.shape[:-1], L).cpu().numpy())
        frames.append({"frame": stem, "invalid": int(bad[0]), "capped": int(bad[1])})
    t = total.cpu().numpy()
    n = max(float(t[2 * L]), 1.0)
    return {"entries": [{"name": unmixer.names[k], "mean_abundance": float(t[k] / n), "active_share": float(t[L + k] / n)} for k in range(L)],
            "mean_count": float(t[2 * L + 1] / n), "mean_residual": float(t[2 * L + 2] / n), "frames": frames}


def main(argv=None) -> dict:
    from .eval import build_pipeline, load_checkpoint
    from . import library as spectral_library

    args = build_parser().parse_args(argv)
    check_sparse_arguments(args)
    pipeline = build_pipeline(args, torch.device(args.device))
    load_checkpoint(pipeline, args.checkpoint)
    library = spectral_library.load_for_model(args.spectral_library, pipeline.model)
    unmixer = sparse_unmixer_from_args(args, library)
    result = {"output_path": str(args.output_path), "split": args.split, "spectral_library": str(args.spectral_library),
              **unmixer.summary(), **sparse_captured(pipeline, unmixer, args.split, args.output_path)}
    (Path(args.output_path) / "summary.json").write_text(json.dumps(result))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
