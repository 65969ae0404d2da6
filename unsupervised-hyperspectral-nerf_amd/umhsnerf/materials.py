"""Material edits at render time: recolour, dim or remove a material of a trained model ("Material edits").

The field predicts, per sample, a softmax abundance over ``C`` materials and a per-material scalar; the spectrum is the linear mix of
the learned dictionary ``E [C,B]`` (+ the specular term).  An edit leaves the checkpoint alone and gives every material ``c``

* ``spectrum``: a replacement row ``E'_c [B]`` (default: the model's own ``E_c``),
* ``gain g_c >= 0``: the row's weight in the mix (default 1),
* ``density d_c >= 0``: a factor on the density of what is made of it (default 1; 0 removes the material),

and the specular term one ``specular_gain s >= 0`` (default 1; models with the specular head only).  The top level of a file holds
for the whole scene; up to ``MAX_REGIONS`` oriented boxes or spheres (``"regions"``, model frame) each carry a complete edit of their
own that REPLACES the top-level one for the samples inside (the first region in file order that contains a sample wins).  The heads
kernel forms its sums per contiguous run of samples, so it is handed the runs of one ray inside one region instead of whole rays and
a regional edit costs what a global one does plus a few memory-bound passes (include/umhs_hip.h, "Regional material edits").
``UMHSModel.material_edits_context(edits)`` renders under one; INTEGRATION.md gives the file format."""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple, Union

import numpy as np
import torch

ENTRY_KEYS = ("material", "spectrum", "from_material", "spectrum_file", "gain", "density")
FILE_KEYS = ("materials", "specular_gain")
REGION_KEYS = ("box", "sphere", "materials", "specular_gain")
BOX_KEYS = ("center", "rotation", "scale")
SPHERE_KEYS = ("center", "radius")
MAX_REGIONS = 8  # UMHS_MAX_REGIONS


@dataclass(frozen=True)
class RegionEdit:
    """One region of an edit file: an oriented box (``center``, ``rotation`` = Euler angles in radians as ``export.obb_from_params``
    takes them, ``scale`` = full extents) or a sphere (``center``, ``radius``) in the model's frame, and the complete edit (a
    ``MaterialEdits`` without regions of its own) that holds inside it."""
    kind: str
    center: Tuple[float, float, float]
    rotation: Tuple[float, float, float]
    scale: Tuple[float, float, float]
    radius: float
    edit: "MaterialEdits"

    def record(self) -> np.ndarray:
        """The 16 floats umhs_region_classify reads: T[3], R[9] row-major, S[3] (sphere: the radius in S[0]), kind."""
        from .export import obb_from_params

        rec = np.zeros(16, dtype=np.float32)
        rec[0:3] = self.center
        if self.kind == "box":
            _, R, S = obb_from_params(self.center, self.rotation, self.scale)
            rec[3:12], rec[12:15] = R.reshape(9), S
        else:
            rec[3:12], rec[12], rec[15] = np.eye(3, dtype=np.float32).reshape(9), self.radius, 1.0
        return rec


@dataclass(frozen=True)
class MaterialEdits:
    """An immutable edit for a model of ``n_classes`` materials, ``n_bands`` bands, with or without the specular head.  Per material:
    ``spectra[c]`` = a tuple of ``n_bands`` floats, a material index (``from_material``: that material's UNEDITED row) or None (its
    own row); ``gains[c]``; ``densities[c]``."""
    n_classes: int
    n_bands: int
    pred_specular: bool
    spectra: Tuple[Union[None, int, Tuple[float, ...]], ...]
    gains: Tuple[float, ...]
    densities: Tuple[float, ...]
    specular_gain: float = 1.0
    regions: Tuple[RegionEdit, ...] = ()

    def __post_init__(self):
        C, B = self.n_classes, self.n_bands
        if not (len(self.spectra) == len(self.gains) == len(self.densities) == C):
            raise ValueError(f"material edits: {C} materials need {C} spectra, gains and densities")
        for c, sp in enumerate(self.spectra):
            if isinstance(sp, int):
                if not 0 <= sp < C:
                    raise ValueError(f"material edits: material {c}: from_material {sp} is outside 0..{C - 1}")
            elif sp is not None:
                _check_spectrum(sp, B, f"material {c}")
        for name, values in (("gain", self.gains), ("density", self.densities)):
            for c, v in enumerate(values):
                _check_factor(v, name, f"material {c}")
        _check_factor(self.specular_gain, "specular_gain", "the file")
        if self.specular_gain != 1.0 and not self.pred_specular:
            raise ValueError(f"material edits: specular_gain {self.specular_gain} needs a model with the specular head (pred_specular)")
        if len(self.regions) > MAX_REGIONS:
            raise ValueError(f"material edits: {len(self.regions)} regions, at most {MAX_REGIONS} are supported")
        for k, r in enumerate(self.regions, 1):
            e = r.edit
            if r.kind not in ("box", "sphere") or e.regions or (e.n_classes, e.n_bands, e.pred_specular) != (C, B, self.pred_specular):
                raise ValueError(f"material edits: region {k}: a region is a box or a sphere with a complete edit for the same model")

    @property
    def layers(self) -> Tuple["MaterialEdits", ...]:
        """The edit of layer 0 (outside every region) and of every region, in file order; none carries regions."""
        top = self if not self.regions else MaterialEdits(self.n_classes, self.n_bands, self.pred_specular, self.spectra, self.gains,
                                                           self.densities, self.specular_gain)
        return (top,) + tuple(r.edit for r in self.regions)

    def region_table(self) -> np.ndarray:
        """HOST float32 [K,16]: the records of ``ops.region_classify``."""
        return np.stack([r.record() for r in self.regions]) if self.regions else np.zeros((0, 16), dtype=np.float32)

    def dictionaries(self, E: torch.Tensor) -> torch.Tensor:
        """``E'' [(K+1),C,B]``: ``dictionary(E)`` of every layer."""
        return torch.stack([e.dictionary(E) for e in self.layers]).contiguous()

    def density_gains(self, device) -> torch.Tensor:
        """``d [(K+1),C]`` float32 on ``device``."""
        return torch.tensor([e.densities for e in self.layers], dtype=torch.float32, device=device)

    def specular_gains(self, device) -> torch.Tensor:
        """``s [K+1]`` float32 on ``device``."""
        return torch.tensor([e.specular_gain for e in self.layers], dtype=torch.float32, device=device)

    @classmethod
    def identity(cls, n_classes: int, n_bands: int, pred_specular: bool) -> "MaterialEdits":
        return cls(n_classes, n_bands, bool(pred_specular), (None,) * n_classes, (1.0,) * n_classes, (1.0,) * n_classes, 1.0)

    @property
    def edits_density(self) -> bool:
        return any(d != 1.0 for d in self.densities) or any(r.edit.edits_density for r in self.regions)

    @property
    def edits_dictionary(self) -> bool:
        """Does ``dictionary(E)`` differ from ``E``, or the specular term from the model's?  (What makes a render launch the remix.)"""
        return (any(sp is not None for sp in self.spectra) or any(g != 1.0 for g in self.gains) or self.specular_gain != 1.0
                or any(r.edit.edits_dictionary for r in self.regions))

    @property
    def is_identity(self) -> bool:
        return not self.edits_density and not self.edits_dictionary

    def dictionary(self, E: torch.Tensor) -> torch.Tensor:
        """``E'' [C,B]`` with ``E''_c = g_c E'_c``: float32 on ``E``'s device, ONE float32 product per element."""
        C, B = self.n_classes, self.n_bands
        if tuple(E.shape) != (C, B):
            raise ValueError(f"material edits built for a [{C},{B}] dictionary, the model's is {list(E.shape)}")
        E = E.detach().to(torch.float32)
        rows = []
        for sp in self.spectra:
            if sp is None:
                rows.append(None)
            elif isinstance(sp, int):
                rows.append(E[sp])
            else:
                rows.append(torch.tensor(sp, dtype=torch.float32, device=E.device))
        Ep = torch.stack([E[c] if r is None else r for c, r in enumerate(rows)])
        return (torch.tensor(self.gains, dtype=torch.float32, device=E.device)[:, None] * Ep).contiguous()

    def density_gain(self, device) -> torch.Tensor:
        """``d [C]`` float32 on ``device``."""
        return torch.tensor(self.densities, dtype=torch.float32, device=device)


def _check_factor(v, name: str, where: str) -> None:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"material edits: {where}: {name} {v!r} must be a finite number >= 0")


def _check_spectrum(sp, n_bands: int, where: str) -> None:
    if len(sp) != n_bands:
        raise ValueError(f"material edits: {where}: the spectrum has {len(sp)} values, the model has {n_bands} bands")
    if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in sp):
        raise ValueError(f"material edits: {where}: the spectrum holds a non-finite value")


def load_material_edits(source, n_classes: int, n_bands: int, pred_specular: bool) -> MaterialEdits:
    """``source``: the dict form of the file, or the path of a JSON file

        {"materials": [{"material": 2, "spectrum": [B floats]}, {"material": 0, "from_material": 1, "gain": 0.5},
                       {"material": 1, "density": 0.0}, {"material": 3, "spectrum_file": "pigment.npy"}], "specular_gain": 1.0}

    ``spectrum``, ``from_material`` and ``spectrum_file`` (a 1-D float ``.npy``, relative to the JSON file) exclude each other within one
    entry; ``from_material`` copies the UNEDITED row of that material.  Refused with a ValueError that names the entry and the reason:
    unknown keys, a material outside ``0..C-1`` or listed twice, a spectrum of another length or with a non-finite value, a negative or
    non-finite ``gain`` / ``density`` / ``specular_gain``, ``specular_gain != 1`` without the specular head.

    An optional ``"regions"`` list (at most ``MAX_REGIONS``) restricts edits to oriented boxes and spheres in the model's frame:

        {"regions": [{"box": {"center": [x, y, z], "rotation": [rx, ry, rz], "scale": [sx, sy, sz]}, "materials": [...]},
                     {"sphere": {"center": [x, y, z], "radius": r}, "materials": [...], "specular_gain": 0.5}]}

    Each region carries a complete edit of its own (``materials`` / ``specular_gain`` as at the top level) that replaces the top-level
    edit inside it; the first region in file order that contains a sample wins.  Refused with a ValueError that names the region:
    more than 8 regions, both or neither of ``box`` / ``sphere``, unknown or missing keys, a scale or radius that is not > 0,
    non-finite numbers, and whatever the per-entry checks refuse."""
    C, B = int(n_classes), int(n_bands)
    base = Path(".")
    if not isinstance(source, dict):
        path = Path(source)
        base = path.parent
        try:
            source = json.loads(path.read_text())
        except json.JSONDecodeError as e:
            raise ValueError(f"material edits: {path} is not JSON: {e}") from None
        if not isinstance(source, dict):
            raise ValueError(f"material edits: {path} must hold a JSON object with a \"materials\" list")
    unknown = sorted(set(source) - set(FILE_KEYS) - {"regions"})
    if unknown:
        raise ValueError(f"material edits: unknown keys {unknown} in the file; it takes {list(FILE_KEYS) + ['regions']}")
    top = _parse_layer(source, C, B, bool(pred_specular), base, "", "the file")
    regions = source.get("regions", [])
    if not isinstance(regions, list):
        raise ValueError("material edits: \"regions\" must be a list of regions")
    if len(regions) > MAX_REGIONS:
        raise ValueError(f"material edits: {len(regions)} regions, at most {MAX_REGIONS} are supported")
    parsed = tuple(_parse_region(r, k, C, B, bool(pred_specular), base) for k, r in enumerate(regions, 1))
    return MaterialEdits(*top, parsed)


def _check_vector(v, n: int, name: str, where: str, positive: bool = False) -> Tuple[float, ...]:
    if not isinstance(v, (list, tuple)) or len(v) != n:
        raise ValueError(f"material edits: {where}: {name} must be a list of {n} numbers, got {v!r}")
    for x in v:
        _check_scalar(x, name, where, positive)
    return tuple(float(x) for x in v)


def _check_scalar(x, name: str, where: str, positive: bool = False) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
        raise ValueError(f"material edits: {where}: {name} {x!r} must be a finite number")
    if positive and not x > 0:
        raise ValueError(f"material edits: {where}: {name} {x!r} must be > 0")
    return float(x)


def _parse_region(r, k: int, C: int, B: int, pred_specular: bool, base: Path) -> RegionEdit:
    where = f"region {k}"
    if not isinstance(r, dict):
        raise ValueError(f"material edits: {where} must be an object, got {r!r}")
    unknown = sorted(set(r) - set(REGION_KEYS))
    if unknown:
        raise ValueError(f"material edits: {where}: unknown keys {unknown}; a region takes {list(REGION_KEYS)}")
    if ("box" in r) == ("sphere" in r):
        raise ValueError(f"material edits: {where}: a region is either a \"box\" or a \"sphere\", got "
                         f"{'both' if 'box' in r else 'neither'}")
    kind = "box" if "box" in r else "sphere"
    shape, keys = r[kind], BOX_KEYS if kind == "box" else SPHERE_KEYS
    if not isinstance(shape, dict):
        raise ValueError(f"material edits: {where}: {kind} must be an object with {list(keys)}")
    unknown = sorted(set(shape) - set(keys))
    if unknown:
        raise ValueError(f"material edits: {where}: unknown keys {unknown} in the {kind}; it takes {list(keys)}")
    missing = [key for key in keys if key not in shape]
    if missing:
        raise ValueError(f"material edits: {where}: the {kind} lacks {missing}")
    center = _check_vector(shape["center"], 3, "center", where)
    rotation, scale, radius = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0
    if kind == "box":
        rotation = _check_vector(shape["rotation"], 3, "rotation", where)
        scale = _check_vector(shape["scale"], 3, "scale", where, positive=True)
        if not all(np.isfinite(np.float32(v)) and np.float32(v) > 0 for v in scale):
            raise ValueError(f"material edits: {where}: scale {list(scale)} must be > 0 and finite in float32")
    else:
        radius = _check_scalar(shape["radius"], "radius", where, positive=True)
        if not (np.isfinite(np.float32(radius)) and np.float32(radius) > 0):
            raise ValueError(f"material edits: {where}: radius {radius!r} must be > 0 and finite in float32")
    layer = _parse_layer(r, C, B, pred_specular, base, f"{where}: ", where)
    try:
        edit = MaterialEdits(*layer)
    except ValueError as e:
        raise ValueError(str(e).replace("material edits: ", f"material edits: {where}: ", 1)) from None
    return RegionEdit(kind, center, rotation, scale, radius, edit)


def _parse_layer(source: dict, C: int, B: int, pred_specular: bool, base: Path, prefix: str, owner: str):
    """The ``materials`` list and ``specular_gain`` of the file's top level (``prefix`` "") or of one region (``prefix`` "region k: ")
    -> the positional arguments of ``MaterialEdits``."""
    entries = source.get("materials", [])
    if not isinstance(entries, list):
        raise ValueError(f"material edits: {prefix}\"materials\" must be a list of entries")
    spectra: list = [None] * C
    gains, densities, seen = [1.0] * C, [1.0] * C, set()
    for i, e in enumerate(entries):
        where = f"{prefix}entry {i}"
        if not isinstance(e, dict):
            raise ValueError(f"material edits: {where} must be an object, got {e!r}")
        unknown = sorted(set(e) - set(ENTRY_KEYS))
        if unknown:
            raise ValueError(f"material edits: {where}: unknown keys {unknown}; an entry takes {list(ENTRY_KEYS)}")
        c = e.get("material")
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < C:
            raise ValueError(f"material edits: {where}: material {c!r} is outside 0..{C - 1}")
        where = f"{prefix}entry {i} (material {c})"
        if c in seen:
            raise ValueError(f"material edits: {where}: material {c} is listed twice")
        seen.add(c)
        sources = [k for k in ("spectrum", "from_material", "spectrum_file") if k in e]
        if len(sources) > 1:
            raise ValueError(f"material edits: {where}: {' and '.join(sources)} exclude each other")
        if "spectrum" in e:
            sp = e["spectrum"]
            if not isinstance(sp, (list, tuple)):
                raise ValueError(f"material edits: {where}: spectrum must be a list of {B} numbers")
            _check_spectrum(sp, B, where)
            spectra[c] = tuple(float(v) for v in sp)
        elif "from_material" in e:
            k = e["from_material"]
            if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < C:
                raise ValueError(f"material edits: {where}: from_material {k!r} is outside 0..{C - 1}")
            spectra[c] = k
        elif "spectrum_file" in e:
            file = base / str(e["spectrum_file"])
            try:
                arr = np.load(file, allow_pickle=False)
            except (OSError, ValueError) as err:
                raise ValueError(f"material edits: {where}: cannot read spectrum_file {file}: {err}") from None
            if arr.ndim != 1 or arr.dtype.kind != "f":
                raise ValueError(f"material edits: {where}: spectrum_file {file} must hold a 1-D float array, got {arr.dtype} {list(arr.shape)}")
            sp = [float(v) for v in arr]
            _check_spectrum(sp, B, where)
            spectra[c] = tuple(sp)
        for name, dest in (("gain", gains), ("density", densities)):
            if name in e:
                _check_factor(e[name], name, where)
                dest[c] = float(e[name])
    s = source.get("specular_gain", 1.0)
    _check_factor(s, "specular_gain", owner)
    return C, B, pred_specular, tuple(spectra), tuple(gains), tuple(densities), float(s)


def model_shape(model) -> Tuple[int, int, bool]:
    """``(C, B, pred_specular)`` of a loaded UMHSModel: what its edits are built for."""
    E = getattr(model.field, "endmembers", None)
    if E is None:
        raise NotImplementedError("material edits need a spectral method (spectral, rgb+spectral): method=\"rgb\" has no material dictionary")
    return int(E.shape[0]), int(E.shape[1]), bool(model.config.pred_specular)


def load_for_model(source, model) -> Optional[MaterialEdits]:
    """``load_material_edits`` with the shape of ``model``; ``None`` stays ``None`` (the command lines' --material-edits)."""
    return None if source is None else load_material_edits(source, *model_shape(model))
