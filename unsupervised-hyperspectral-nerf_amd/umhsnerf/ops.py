"""Host-side operators of the UMHS hot path: thin tensor wrappers over the C ABI plus the
``torch.autograd.Function`` glue that lets nerfstudio's Trainer drive them.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); every number is produced by
libumhs_hip.so.  Nothing in this module has a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import ptr

NUM_LEVELS = 16
FEATURES_PER_LEVEL = 2
GEO_FEAT_DIM = 15
HIDDEN = 64


def hash_scalings(num_levels: int = NUM_LEVELS, min_res: int = 16, max_res: int = 2048) -> torch.Tensor:
    """``scalings`` buffer of nerfstudio's HashEncoding (mlp_base, umhs_field.py:51 / umhs_model.py:183-184).
    Deliberately the same expression: the numpy float64 growth factor is raised to an int64 tensor, which torch
    evaluates in float32, so the top level is floor(2047.99..) = 2047."""
    levels = torch.arange(num_levels)
    growth = np.exp((np.log(max_res) - np.log(min_res)) / (num_levels - 1)) if num_levels > 1 else 1.0
    return torch.floor(min_res * growth**levels)


# --------------------------------------------------------------------------------------------- #
# flat parameter layout (one fp32 buffer = param group "fields"; names = reference state-dict keys)
# --------------------------------------------------------------------------------------------- #
@dataclass
class FieldLayout:
    num_classes: int
    wavelengths: int
    pred_specular: bool
    log2_hashmap_size: int = 19
    entries: Dict[str, Tuple[int, Tuple[int, ...]]] = field(default_factory=dict)
    total: int = 0

    def __post_init__(self):
        Cn, B = self.num_classes, self.wavelengths
        T = 1 << self.log2_hashmap_size
        out_feat = Cn + 1 if self.pred_specular else Cn
        shapes = [("mlp_base.encoder.hash_table", (NUM_LEVELS * T, FEATURES_PER_LEVEL))]

        def mlp(prefix, dims):
            for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
                shapes.append((f"{prefix}.layers.{i}.weight", (b, a)))
                shapes.append((f"{prefix}.layers.{i}.bias", (b,)))

        mlp("mlp_base.mlp", [NUM_LEVELS * FEATURES_PER_LEVEL, HIDDEN, 1 + GEO_FEAT_DIM])
        mlp("mlp_head", [12 + GEO_FEAT_DIM, HIDDEN, HIDDEN, Cn])
        mlp("feature_mlp", [12 + GEO_FEAT_DIM, HIDDEN, HIDDEN, out_feat])
        mlp("mlp_directional", [16 + 12, 16, B])
        shapes.append(("endmembers", (Cn, B)))
        off = 0
        for name, shp in shapes:
            self.entries[name] = (off, shp)
            off += (int(np.prod(shp)) + 3) & ~3  # 16-byte aligned segments (float4 Adam, float2 table rows)
        self.total = off

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shp = self.entries[name]
        return flat[off : off + int(np.prod(shp))].view(shp)

    def offset(self, name: str) -> int:
        return self.entries[name][0]

    def tail_offset(self) -> int:
        """First element behind the hash table: the MLP weights / biases and the endmembers follow."""
        return self.entries["mlp_base.mlp.layers.0.weight"][0]

    # (C struct field, state-dict key)
    C_FIELDS = (
        ("base_w0", "mlp_base.mlp.layers.0.weight"), ("base_b0", "mlp_base.mlp.layers.0.bias"),
        ("base_w1", "mlp_base.mlp.layers.1.weight"), ("base_b1", "mlp_base.mlp.layers.1.bias"),
        ("head_w0", "mlp_head.layers.0.weight"), ("head_b0", "mlp_head.layers.0.bias"),
        ("head_w1", "mlp_head.layers.1.weight"), ("head_b1", "mlp_head.layers.1.bias"),
        ("head_w2", "mlp_head.layers.2.weight"), ("head_b2", "mlp_head.layers.2.bias"),
        ("feat_w0", "feature_mlp.layers.0.weight"), ("feat_b0", "feature_mlp.layers.0.bias"),
        ("feat_w1", "feature_mlp.layers.1.weight"), ("feat_b1", "feature_mlp.layers.1.bias"),
        ("feat_w2", "feature_mlp.layers.2.weight"), ("feat_b2", "feature_mlp.layers.2.bias"),
        ("dir_w0", "mlp_directional.layers.0.weight"), ("dir_b0", "mlp_directional.layers.0.bias"),
        ("dir_w1", "mlp_directional.layers.1.weight"), ("dir_b1", "mlp_directional.layers.1.bias"),
        ("endmembers", "endmembers"),
    )

    def c_struct(self, flat: torch.Tensor, cls, tail_only: Optional[torch.Tensor] = None):
        """``tail_only``: a tensor holding just the MLP / endmember segments (elements [tail_offset(), total) of the flat layout);
        the struct then points into it -- none of its fields lies in the hash table."""
        s = cls()
        base = flat.data_ptr() if tail_only is None else tail_only.data_ptr() - 4 * self.tail_offset()
        for cname, key in self.C_FIELDS:
            setattr(s, cname, base + 4 * self.entries[key][0])
        return s


@dataclass
class FieldSpec:
    """Static configuration the kernels need (everything that is not a tensor)."""

    layout: FieldLayout
    temperature: float
    contraction: bool = True
    aabb: Tuple[float, ...] = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    scalings: Optional[torch.Tensor] = None  # device [16] float32
    grad_sink: Optional[object] = None  # parallel.FlatGradSink: persistent flat-gradient buffer + early all-reduce

    def cfg(self, density_only: bool = False) -> _hip.FieldCfg:
        return _hip.FieldCfg(self.layout.wavelengths, self.layout.num_classes, int(self.layout.pred_specular),
                             int(density_only), float(self.temperature))


# --------------------------------------------------------------------------------------------- #
# raw operator calls
# --------------------------------------------------------------------------------------------- #
def positions_fwd(origins, directions, starts, ends, spec: FieldSpec, world_pos_in=None):
    src = world_pos_in if world_pos_in is not None else origins
    n = src.shape[0]
    wpos = torch.empty((n, 3), device=src.device, dtype=torch.float32) if world_pos_in is None else world_pos_in
    pos01 = torch.empty((n, 3), device=src.device, dtype=torch.float32)
    sel = torch.empty((n,), device=src.device, dtype=torch.float32)
    aabb = (C.c_float * 6)(*spec.aabb)
    _hip.check(
        _hip.lib().umhs_positions_fwd(ptr(origins), ptr(directions), ptr(starts), ptr(ends), ptr(world_pos_in), n,
                                      int(spec.contraction), aabb, ptr(wpos) if world_pos_in is None else None, ptr(pos01),
                                      ptr(sel), _hip.stream()),
        "umhs_positions_fwd",
    )
    return wpos, pos01, sel


def enc_strides(n: int, level_major: bool) -> Tuple[int, int]:
    return (2, 2 * n) if level_major else (2 * NUM_LEVELS, 2)


def hashgrid_fwd(pos01, table, scalings, log2_T: int, level_major: bool = True, out=None, part=None):
    """part = (offset, count): encode only that range of samples into ``out`` (the full-size enc tensor; level-major)."""
    n = pos01.shape[0]
    shape = (NUM_LEVELS, n, 2) if level_major else (n, NUM_LEVELS * 2)
    enc = out if out is not None else torch.empty(shape, device=pos01.device, dtype=torch.float32)
    sn, sl = enc_strides(n, level_major)
    off, cnt = part if part is not None else (0, n)
    _hip.check(_hip.lib().umhs_hashgrid_fwd(pos01.data_ptr() + 12 * off, ptr(table), ptr(scalings), cnt, NUM_LEVELS, log2_T,
                                            enc.data_ptr() + 4 * sn * off, sn, sl, _hip.stream()), "umhs_hashgrid_fwd")
    return enc


def enc_gather(enc, index):
    """Level-major features of the samples ``index`` (int64 [N], ascending) out of an encoded superset ``enc`` [L, M, 2]."""
    L_, m = enc.shape[0], enc.shape[1]
    n = index.shape[0]
    out = torch.empty((L_, n, 2), device=enc.device, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_enc_gather(ptr(enc), ptr(index), m, n, L_, ptr(out), _hip.stream()), "umhs_enc_gather")
    return out


def hashgrid_bwd(pos01, d_enc, scalings, log2_T: int, d_table, level_major: bool = True, method: str = "auto",
                 overwrite: bool = False, level_begin: int = 0, level_count: int = NUM_LEVELS):
    """d_table (+)= scatter(d_enc) for levels [level_begin, level_begin+level_count).  method: "partition" (atomics-free,
    needs a workspace), "atomic", or "auto".  overwrite=True: every slot of those levels is written (no zeroing needed)."""
    n = pos01.shape[0]
    sn, sl = enc_strides(n, level_major)
    nbytes = _hip.lib().umhs_hashgrid_bwd_workspace_bytes(n, level_count, log2_T) if method != "atomic" else 0
    if method == "partition" and nbytes == 0:
        raise RuntimeError("partitioned hash-grid backward unavailable for this shape")
    ws = _workspace(nbytes, pos01.device, slot=1) if nbytes else None
    _hip.check(_hip.lib().umhs_hashgrid_bwd(ptr(pos01), ptr(d_enc), sn, sl, ptr(scalings), n, level_begin, level_count, log2_T,
                                            ptr(d_table), int(overwrite), ptr(ws), ws.numel() if ws is not None else 0,
                                            _hip.stream()),
               "umhs_hashgrid_bwd")


def hashgrid_bwd_prepare(pos01, scalings, log2_T: int, level_begin: int = 0, level_count: int = NUM_LEVELS) -> bool:
    """Gradient-independent half of the partitioned backward (histogram + scan) into the cached workspace.  False: this shape
    has no partitioned path (the caller then uses hashgrid_bwd)."""
    n = pos01.shape[0]
    nbytes = _hip.lib().umhs_hashgrid_bwd_workspace_bytes(n, level_count, log2_T)
    if nbytes == 0:
        return False
    ws = _workspace(nbytes, pos01.device, slot=1)
    _hip.check(_hip.lib().umhs_hashgrid_bwd_prepare(ptr(pos01), ptr(scalings), n, level_begin, level_count, log2_T, ptr(ws), ws.numel(),
                                                    _hip.stream()), "umhs_hashgrid_bwd_prepare")
    _lease(pos01.device, WS_HASH_BWD, "hashgrid_bwd_prepare")
    return True


def hashgrid_fwd_count(pos01, table, scalings, log2_T: int):
    """hashgrid_fwd (level-major) whose launch also takes the bucket histogram of the partitioned backward for the same positions
    into the cached workspace (reserve_step_workspaces sized it); hashgrid_bwd_prepare_counted finishes the prepare.  None: this
    shape has no partitioned path."""
    n = pos01.shape[0]
    nbytes = _hip.lib().umhs_hashgrid_bwd_workspace_bytes(n, NUM_LEVELS, log2_T)
    if nbytes == 0 or n == 0:
        return None
    ws = _workspace(nbytes, pos01.device, slot=1)
    enc = torch.empty((NUM_LEVELS, n, 2), device=pos01.device, dtype=torch.float32)
    sn, sl = enc_strides(n, True)
    _hip.check(_hip.lib().umhs_hashgrid_fwd_count(ptr(pos01), ptr(table), ptr(scalings), n, NUM_LEVELS, log2_T, ptr(enc), sn, sl, ptr(ws),
                                                  ws.numel(), _hip.stream()), "umhs_hashgrid_fwd_count")
    return enc


def hashgrid_bwd_prepare_counted(pos01, scalings, log2_T: int) -> bool:
    """The two scans of hashgrid_bwd_prepare over the histogram hashgrid_fwd_count left in the workspace (all levels)."""
    n = pos01.shape[0]
    ws = _workspace(_hip.lib().umhs_hashgrid_bwd_workspace_bytes(n, NUM_LEVELS, log2_T), pos01.device, slot=1)
    _hip.check(_hip.lib().umhs_hashgrid_bwd_prepare_counted(ptr(pos01), ptr(scalings), n, NUM_LEVELS, log2_T, ptr(ws), ws.numel(),
                                                            _hip.stream()), "umhs_hashgrid_bwd_prepare_counted")
    _lease(pos01.device, WS_HASH_BWD, "hashgrid_bwd_prepare")
    return True


def hashgrid_bwd_apply(pos01, d_enc, scalings, log2_T: int, d_table, level_major: bool = True, overwrite: bool = False,
                       level_begin: int = 0, level_count: int = NUM_LEVELS, ws_range=(0, NUM_LEVELS), adam=None):
    """Scatter + reduce of levels [level_begin, +level_count) using the workspace hashgrid_bwd_prepare filled for ws_range.
    ``adam`` (overwrite mode, n > 0): dict(table, exp_avg, exp_avg_sq [L*T,2] views, lr, betas, eps, step, level_begin) -- the Adam
    step of the table entries of levels >= level_begin rides in the epilogue of the reduce pass."""
    n = pos01.shape[0]
    sn, sl = enc_strides(n, level_major)
    ws = _workspace(_hip.lib().umhs_hashgrid_bwd_workspace_bytes(n, ws_range[1], log2_T), pos01.device, slot=1)
    if adam is not None:
        assert overwrite and n > 0
        _hip.check(_hip.lib().umhs_hashgrid_bwd_apply_adam(ptr(pos01), ptr(d_enc), sn, sl, ptr(scalings), n, level_begin, level_count,
                                                           ws_range[0], ws_range[1], log2_T, ptr(d_table), ptr(ws), ws.numel(),
                                                           ptr(adam["table"]), ptr(adam["exp_avg"]), ptr(adam["exp_avg_sq"]),
                                                           float(adam["lr"]), float(adam["betas"][0]), float(adam["betas"][1]),
                                                           float(adam["eps"]), int(adam["step"]), int(adam["level_begin"]),
                                                           _hip.stream()), "umhs_hashgrid_bwd_apply_adam")
        if level_begin + level_count >= ws_range[0] + ws_range[1]:
            _release(pos01.device, WS_HASH_BWD)
        return
    _hip.check(_hip.lib().umhs_hashgrid_bwd_apply(ptr(pos01), ptr(d_enc), sn, sl, ptr(scalings), n, level_begin, level_count, ws_range[0],
                                                  ws_range[1], log2_T, ptr(d_table), int(overwrite), ptr(ws), ws.numel(), _hip.stream()),
               "umhs_hashgrid_bwd_apply")
    if level_begin + level_count >= ws_range[0] + ws_range[1]:  # the last level group of this prepare has been launched
        _release(pos01.device, WS_HASH_BWD)


def reserve_step_workspaces(spec: FieldSpec, n: int, device) -> bool:
    """Size the cached workspaces of one training step on the CURRENT stream, so that the *_prepare calls issued on a side
    stream never allocate there (blocks handed out under another stream would need record_stream bookkeeping).
    Returns whether the partitioned hash-grid backward is available for this n."""
    cfg = spec.cfg(False)
    for slot in (WS_FIELD_BWD, WS_HASH_BWD, WS_FIELD_FWD):  # a lease still open here belongs to a step that was abandoned
        _release(device, slot)
    _workspace(_hip.lib().umhs_field_fwd_workspace_bytes(C.byref(cfg)), device, slot=2)
    _workspace(_hip.lib().umhs_field_bwd_workspace_bytes(C.byref(cfg), n), device)
    nbytes = _hip.lib().umhs_hashgrid_bwd_workspace_bytes(n, NUM_LEVELS, spec.layout.log2_hashmap_size)
    if nbytes:
        _workspace(nbytes, device, slot=1)
    return nbytes != 0


def field_fwd_prepare(spec: FieldSpec, flat):
    """Build the forward pack image ahead of field_fwd(pack_ready=True) (same cached workspace)."""
    cfg = spec.cfg(False)
    pp = spec.layout.c_struct(flat, _hip.FieldParams)
    ws = _workspace(_hip.lib().umhs_field_fwd_workspace_bytes(C.byref(cfg)), flat.device, slot=2)
    _hip.check(_hip.lib().umhs_field_fwd_prepare(C.byref(cfg), C.byref(pp), ptr(ws), ws.numel(), _hip.stream()), "umhs_field_fwd_prepare")
    _lease(flat.device, WS_FIELD_FWD, "field_fwd_prepare")


def field_bwd_prepare(spec: FieldSpec, flat, n: int):
    """Build the backward's weight images ahead of field_bwd(packs_ready=True); n sizes the shared workspace once."""
    cfg = spec.cfg(False)
    pp = spec.layout.c_struct(flat, _hip.FieldParams)
    ws = _workspace(_hip.lib().umhs_field_bwd_workspace_bytes(C.byref(cfg), n), flat.device)
    _hip.check(_hip.lib().umhs_field_bwd_prepare(C.byref(cfg), C.byref(pp), ptr(ws), ws.numel(), _hip.stream()), "umhs_field_bwd_prepare")
    _lease(flat.device, WS_FIELD_BWD, "field_bwd_prepare")


def field_fwd_outputs(spec: FieldSpec, n: int, dev, density_only=False, want_emb=None, want_aux=True, want_logits=False):
    """``want_emb``: None = the density-only form returns the embedding, the full form does not; True / False force it."""
    L = spec.layout
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    want_emb = density_only if want_emb is None else want_emb
    out = dict(sigma=new(n), sigma_raw=new(n), emb=new(n, GEO_FEAT_DIM) if want_emb else None, spectral=None,
               spectral2=None, specular=None, abundances=None,
               feat_logits=new(n, 16) if (want_logits and not density_only) else None)  # saved for the split heads backward
    if not density_only:
        out["spectral"] = new(n, L.wavelengths)
        if want_aux:
            out["abundances"] = new(n, L.num_classes)
            if L.pred_specular:
                out["spectral2"], out["specular"] = new(n, L.wavelengths), new(n, L.wavelengths)
    return out


def field_fwd(spec: FieldSpec, flat, enc, level_major, wpos, dirs, sel, density_only=False, want_emb=None, want_aux=True, pack_ready=False,
              out=None, part=None, want_logits=False):
    """part = (offset, count): evaluate only that range of samples, writing into the full-size tensors of ``out``."""
    n = sel.shape[0]
    L = spec.layout
    dev = sel.device
    cfg = spec.cfg(density_only)
    pp = L.c_struct(flat, _hip.FieldParams)
    sn, sl = enc_strides(n, level_major)
    o = out if out is not None else field_fwd_outputs(spec, n, dev, density_only, want_emb, want_aux, want_logits)
    off, cnt = part if part is not None else (0, n)
    at = lambda t, width: (t.data_ptr() + 4 * width * off) if t is not None else None
    if not pack_ready:
        _require_free(dev, WS_FIELD_FWD, "field_fwd (pack image rebuild)")
    ws = _workspace(_hip.lib().umhs_field_fwd_workspace_bytes(C.byref(cfg)), dev, slot=2)
    _hip.check(_hip.lib().umhs_field_fwd(C.byref(cfg), C.byref(pp), at(enc, sn), sn, sl, at(wpos, 3), at(dirs, 3), at(sel, 1), cnt,
                                         at(o["sigma"], 1), at(o["sigma_raw"], 1), at(o["emb"], GEO_FEAT_DIM), at(o["spectral"], L.wavelengths),
                                         at(o["spectral2"], L.wavelengths), at(o["specular"], L.wavelengths),
                                         at(o["abundances"], L.num_classes), at(o.get("feat_logits"), 16), ptr(ws), ws.numel(), int(pack_ready),
                                         _hip.stream()),
               "umhs_field_fwd")
    if pack_ready:
        _release(dev, WS_FIELD_FWD)
    return o


def field_base_fwd(spec: FieldSpec, flat, enc, level_major, sel, pack_ready=False, rows16=False):
    """mlp_base only, from the full configuration's pack images (first launch of the two-launch training forward):
    -> {"sigma" [N], "sigma_raw" [N], "emb" [N,15]}; ``rows16``: instead of emb, "base16" [N,16] = aligned rows (sigma_raw, emb)."""
    n, dev, L = sel.shape[0], sel.device, spec.layout
    cfg = spec.cfg(False)
    pp = L.c_struct(flat, _hip.FieldParams)
    sn, sl = enc_strides(n, level_major)
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    o = dict(sigma=new(n), sigma_raw=new(n), emb=None if rows16 else new(n, GEO_FEAT_DIM), base16=new(n, 16) if rows16 else None)
    if not pack_ready:
        _require_free(dev, WS_FIELD_FWD, "field_base_fwd (pack image rebuild)")
    ws = _workspace(_hip.lib().umhs_field_fwd_workspace_bytes(C.byref(cfg)), dev, slot=2)
    _hip.check(_hip.lib().umhs_field_base_fwd(C.byref(cfg), C.byref(pp), ptr(enc), sn, sl, ptr(sel), n, ptr(o["sigma"]), ptr(o["sigma_raw"]),
                                              ptr(o["emb"]), ptr(o["base16"]), ptr(ws), ws.numel(), int(pack_ready), _hip.stream()),
               "umhs_field_base_fwd")
    return o


_step_scratch: Dict[Tuple[int, str], torch.Tensor] = {}


def _scratch(dev, key: str, nbytes: int) -> torch.Tensor:
    """Grow-only per-device scratch of the two-launch step (tile partials, per-ray sums); contents are dead after each call."""
    k = (dev.index or 0, key)
    sc = _step_scratch.get(k)
    if sc is None or sc.numel() < nbytes:
        sc = _step_scratch[k] = torch.empty(max(nbytes, 1 << 16), device=dev, dtype=torch.uint8)
    return sc


def field_heads_fwd(spec: FieldSpec, flat, emb, wpos, dirs, weights, ray_indices, packed_info, want_logits=True, pack_ready=True,
                    release=True, want_abundances=False, want_mix=False):
    """Second launch of the two-launch training forward: heads from ``emb`` ([N,15], or the [N,16] aligned rows of
    field_base_fwd(rows16=True)) with the per-ray sums formed in the kernel; no [N,B] array is written (the mixing term is summed
    per ray as w m and multiplied by the endmembers once per ray).
    -> {"abundances" [N,C] | None, "feat_logits" [N,16] | None, "comp": [spectral, spectral2, specular] ([R,B]; one entry without the
        specular head), "comp_abundances" [R,C]}.
    ``pack_ready``: the images field_fwd_prepare / field_base_fwd left in the forward workspace are reused.
    ``want_mix``: the result also carries "mix" [R,16], the per-ray sums of w m the mixing product was formed from -- a VIEW into the
    kernel's scratch (umhs_field_heads_fwd_mix_offset), valid until the next field_heads_fwd on this device: consume it at once, on
    the same stream (material_remix does).  Columns >= C hold nothing that may be relied on."""
    n, dev, L = emb.shape[0], emb.device, spec.layout
    R = packed_info.shape[0]
    cfg = spec.cfg(False)
    pp = L.c_struct(flat, _hip.FieldParams)
    new = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    B = L.wavelengths
    o = dict(abundances=new(n, L.num_classes) if want_abundances else None, feat_logits=new(n, 16) if want_logits else None,
             comp_abundances=new(R, L.num_classes))
    comp = [new(R, B)] + ([new(R, B), new(R, B)] if L.pred_specular else [])
    sc = _scratch(dev, "heads_fwd", _hip.lib().umhs_field_heads_fwd_scratch_bytes(C.byref(cfg), n, R))
    ws = _workspace(_hip.lib().umhs_field_fwd_workspace_bytes(C.byref(cfg)), dev, slot=2)
    _hip.check(_hip.lib().umhs_field_heads_fwd(C.byref(cfg), C.byref(pp), ptr(emb), emb.shape[1], ptr(wpos), ptr(dirs), n, ptr(weights),
                                               ptr(ray_indices), ptr(packed_info), R, ptr(o["abundances"]), ptr(o["feat_logits"]),
                                               ptr(comp[0]), ptr(comp[1]) if len(comp) > 1 else None,
                                               ptr(comp[2]) if len(comp) > 1 else None, ptr(o["comp_abundances"]), ptr(sc), sc.numel(), ptr(ws),
                                               ws.numel(), int(pack_ready), _hip.stream()), "umhs_field_heads_fwd")
    if pack_ready and release:
        _release(dev, WS_FIELD_FWD)
    o["comp"] = comp
    if want_mix:
        off = _hip.lib().umhs_field_heads_fwd_mix_offset(C.byref(cfg), n, R)
        if off < 0:
            raise RuntimeError("umhs_field_heads_fwd_mix_offset: this configuration has no per-ray mixing sums")
        o["mix"] = sc[off: off + R * 64].view(torch.float32).view(R, 16)
    return o


def material_sigma(sigma, abundances, density_gain, out=None):
    """Density edit of a material-edited render (include/umhs_hip.h, "Material edits", step 1):
    sigma'[n] = sigma[n] * max(0, 1 + sum_c (d_c - 1) a[n,c]).  ``density_gain`` [C] on the device; ``out`` may be ``sigma`` itself."""
    n, Cn = abundances.shape
    o = torch.empty_like(sigma) if out is None else out
    _hip.check(_hip.lib().umhs_material_sigma(ptr(sigma), ptr(abundances), ptr(density_gain), n, Cn, ptr(o), _hip.stream()),
               "umhs_material_sigma")
    return o


def material_remix(mix, comp_specular, E_edit, specular_gain: float = 1.0):
    """Re-mix the per-ray sums ``mix`` [R,16] of field_heads_fwd(want_mix=True) with an edited dictionary ``E_edit`` [C,B] ("Material
    edits", step 3).  ``comp_specular`` [R,B] (the composited specular term) or None
    -> [spectral] | [spectral, spectral2, specular]."""
    R, (Cn, B) = mix.shape[0], E_edit.shape
    new = lambda: torch.empty((R, B), device=mix.device, dtype=torch.float32)
    outs = [new()] if comp_specular is None else [new(), new(), new()]
    _hip.check(_hip.lib().umhs_material_remix(ptr(mix), ptr(comp_specular), ptr(E_edit), float(specular_gain), R, B, Cn, ptr(outs[0]),
                                              ptr(outs[1]) if len(outs) > 1 else None, ptr(outs[2]) if len(outs) > 1 else None,
                                              _hip.stream()), "umhs_material_remix")
    return outs


def field_density(spec: FieldSpec, flat, pos01, sel, want_emb: bool = True, keep=None):
    """density_fn: hash-grid gather + density-only field forward (two launches; the level-major features live in a per-device scratch,
    or in ``keep["enc"]`` for a caller that reuses them) -> {"sigma" [N], "sigma_raw" [N], "emb" [N,15] | None}."""
    n, L = sel.shape[0], spec.layout
    if keep is None:
        enc = _scratch(sel.device, "density_enc", NUM_LEVELS * n * 8)[: NUM_LEVELS * n * 8].view(torch.float32).view(NUM_LEVELS, n, 2)
    else:
        enc = keep["enc"] = torch.empty((NUM_LEVELS, n, 2), device=sel.device, dtype=torch.float32)
    hashgrid_fwd(pos01, L.view(flat, "mlp_base.encoder.hash_table"), spec.scalings, L.log2_hashmap_size, True, out=enc)
    return field_fwd(spec, flat, enc, True, None, None, sel, density_only=True, want_emb=want_emb)


NORMALS_OUTPUTS = ("grad", "normal", "g01")


def density_normals(spec, flat, pos01, wpos, sel, enc=None, want: Sequence[str] = ("normal",)) -> Dict[str, torch.Tensor]:
    """Density-gradient normals of the samples (include/umhs_hip.h, "Density-gradient normals"; one launch, no autograd).
    ``pos01``, ``wpos``, ``sel``: as ``positions_fwd`` returns them.  ``enc``: their level-major hash features [16, N, 2] when the
    caller has them; else ``hashgrid_fwd`` gathers them into a per-device scratch first (the kernel can gather them itself, with the
    same bits, but walks all sixteen levels per lane: measured at 2^21 samples, the level-by-level gather kernel and the ``enc`` form
    take 1.84 ms together, the self-gathering form 2.44).  ``spec``: anything with ``layout`` (``view`` under the
    reference's ``mlp_base`` key names, ``log2_hashmap_size``), ``contraction``, ``aabb`` and ``scalings`` -- the FieldSpec of
    UMHSField or the rgb field's.  ``want``: any of "grad" (d density / d world position), "normal" (-grad / (|grad| + 1e-10)),
    "g01" (d sigma_raw / d pos01) -> {name: [N,3] float32}."""
    want = tuple(want)
    if not want or any(w not in NORMALS_OUTPUTS for w in want):
        raise ValueError(f"density_normals: want {want!r} must name at least one of {NORMALS_OUTPUTS}")
    n, L = pos01.shape[0], spec.layout
    if enc is not None and (tuple(enc.shape) != (NUM_LEVELS, n, 2) or enc.dtype != torch.float32):
        raise ValueError(f"density_normals: enc must be the level-major float32 [{NUM_LEVELS}, {n}, 2] features, got {tuple(enc.shape)}")
    out = {w: torch.empty((n, 3), device=pos01.device, dtype=torch.float32) for w in want}
    view = lambda k: L.view(flat, "mlp_base." + k)
    if enc is None and n > 0:
        enc = _scratch(pos01.device, "normals_enc", NUM_LEVELS * n * 8)[: NUM_LEVELS * n * 8].view(torch.float32).view(NUM_LEVELS, n, 2)
        hashgrid_fwd(pos01, view("encoder.hash_table"), spec.scalings, L.log2_hashmap_size, True, out=enc)
    aabb = (C.c_float * 6)(*spec.aabb)
    _hip.check(_hip.lib().umhs_density_normals(
        ptr(pos01), ptr(wpos), ptr(sel), ptr(enc), ptr(view("encoder.hash_table")), ptr(spec.scalings), L.log2_hashmap_size,
        ptr(view("mlp.layers.0.weight")), ptr(view("mlp.layers.0.bias")), ptr(view("mlp.layers.1.weight")), ptr(view("mlp.layers.1.bias")),
        int(bool(spec.contraction)), aabb, n, ptr(out.get("grad")), ptr(out.get("normal")), ptr(out.get("g01")), _hip.stream()),
        "umhs_density_normals")
    return out


def ray_normals(weights, normal, packed_info) -> torch.Tensor:
    """The ``normals`` model output [R,3] in [0, 1] from the per-sample normals and the rendering weights: N = sum_i w_i n_i
    (``accumulate_fwd``), n^ = N / (|N| + 1e-10), (n^ + 1) / 2; a ray with no samples gives 0.5."""
    R = packed_info.shape[0]
    if normal.shape[0] == 0:
        return torch.full((R, 3), 0.5, device=packed_info.device, dtype=torch.float32)
    N = accumulate_fwd(_hip.f32c(weights).view(-1), _hip.f32c(normal).view(-1, 3), packed_info)
    return (N / (torch.linalg.vector_norm(N, dim=-1, keepdim=True) + 1e-10) + 1.0) / 2.0


_ws_cache: Dict[Tuple[int, int], torch.Tensor] = {}
_ws_leases: Dict[Tuple[int, int], str] = {}  # (device, slot) -> the *_prepare call whose consumer has not been launched yet

WS_FIELD_BWD, WS_HASH_BWD, WS_FIELD_FWD = 0, 1, 2  # slots of the per-device workspace cache


def _workspace(nbytes: int, device, slot: int = 0) -> torch.Tensor:
    """Cached per-(device, slot) scratch.  A slot is never re-grown while a ``*_prepare`` call has parked data in it for a consumer
    that has not been launched yet (``_lease`` / ``_release``): the consumer would be handed a fresh, unfilled buffer."""
    key = (device.index or 0, slot)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if key in _ws_leases:
            raise RuntimeError(f"workspace slot {slot} would be re-grown ({0 if ws is None else ws.numel()} -> {nbytes} bytes) while "
                               f"{_ws_leases[key]} holds data in it for a consumer that has not run; size it first "
                               "(ops.reserve_step_workspaces)")
        ws = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
        _ws_cache[key] = ws
    return ws


def _lease(device, slot: int, who: str) -> None:
    _ws_leases[(device.index or 0, slot)] = who


def _release(device, slot: int) -> None:
    _ws_leases.pop((device.index or 0, slot), None)


def _require_free(device, slot: int, who: str) -> None:
    """A call that rebuilds a slot's contents must not run between a ``*_prepare`` and its consumer."""
    held = _ws_leases.get((device.index or 0, slot))
    if held is not None:
        raise RuntimeError(f"{who} would overwrite workspace slot {slot} while {held} holds data in it for a consumer that has not run")


def _supported(spec: FieldSpec, attr: str, query) -> bool:
    """A capability of the library that depends on the configuration only: asked once, cached on the spec."""
    ok = getattr(spec, attr, None)
    if ok is None:
        cfg = spec.cfg(False)
        ok = bool(query(C.byref(cfg)))
        try:
            setattr(spec, attr, ok)
        except AttributeError:
            pass
    return ok


def field_heads_fwd_supported(spec: FieldSpec) -> bool:
    """Can field_base_fwd / field_heads_fwd (the two-launch forward with the per-ray sums in the kernel) serve this configuration?"""
    return _supported(spec, "_heads_fwd_ok", _hip.lib().umhs_field_heads_fwd_supported)


def field_bwd_composited_supported(spec: FieldSpec) -> bool:
    return _supported(spec, "_composited_ok", _hip.lib().umhs_field_bwd_composited_supported)


def field_bwd(spec: FieldSpec, flat, enc, level_major, wpos, dirs, sel, sigma_raw, emb, d_sigma, d_spectral, d_emb, d_flat,
              packs_ready=False, feat_logits=None, d_tail=None, comp=None):
    """Writes d_enc (returned) and the MLP / endmember gradients straight into ``d_flat`` (flat layout) -- or, when ``d_tail`` is
    given (a tensor of ``total - tail_offset()`` floats), into that instead (gradient accumulation adds it to the flat gradient).
    ``comp``: dict(sigma, t0, t1, packed_info, ray_indices, weights, d_comp, d_acc, grad_scaling) -- the value half of the compositing
    backward runs inside (umhs_field_bwd_composited); d_sigma / d_spectral are then ignored and comp["d_sigma"] receives d_sigma."""
    n = sel.shape[0]
    L = spec.layout
    cfg = spec.cfg(False)
    pp = L.c_struct(flat, _hip.FieldParams)
    gp = L.c_struct(d_flat, _hip.FieldGrads, tail_only=d_tail)
    sn, sl = enc_strides(n, level_major)
    d_enc = torch.empty_like(enc)
    nbytes = _hip.lib().umhs_field_bwd_workspace_bytes(C.byref(cfg), n)
    ws = _workspace(nbytes, sel.device)
    if comp is not None:
        comp["d_sigma"] = torch.empty(n, device=sel.device, dtype=torch.float32)
        pi = comp["packed_info"]
        sc = _scratch(sel.device, "bwd_comp", _hip.lib().umhs_field_bwd_composited_scratch_bytes(C.byref(cfg), n, pi.shape[0]))
        _hip.check(_hip.lib().umhs_field_bwd_composited(
            C.byref(cfg), C.byref(pp), ptr(enc), sn, sl, ptr(wpos), ptr(dirs), ptr(sel), ptr(sigma_raw), ptr(emb), emb.shape[1], ptr(feat_logits), n,
            ptr(comp["sigma"]), ptr(comp["t0"]), ptr(comp["t1"]), ptr(pi), pi.shape[0], ptr(comp["ray_indices"]), ptr(comp["weights"]),
            ptr(comp["d_comp"]), ptr(comp["d_acc"]), int(bool(comp["grad_scaling"])), ptr(comp["d_sigma"]), ptr(d_enc), C.byref(gp), ptr(sc),
            sc.numel(), ptr(ws), ws.numel(), int(packs_ready), _hip.stream()), "umhs_field_bwd_composited")
        if packs_ready:
            _release(sel.device, WS_FIELD_BWD)
        return d_enc
    _hip.check(_hip.lib().umhs_field_bwd(C.byref(cfg), C.byref(pp), ptr(enc), sn, sl, ptr(wpos), ptr(dirs), ptr(sel),
                                         ptr(sigma_raw), ptr(emb), ptr(feat_logits), n,
                                         ptr(d_sigma), ptr(d_spectral), ptr(d_emb), ptr(d_enc), C.byref(gp), ptr(ws),
                                         ws.numel(), int(packs_ready), _hip.stream()), "umhs_field_bwd")
    if packs_ready:
        _release(sel.device, WS_FIELD_BWD)
    return d_enc


def pack_info(ray_indices: torch.Tensor, num_rays: int) -> torch.Tensor:
    out = torch.empty((num_rays, 2), device=ray_indices.device, dtype=torch.int64)
    _hip.check(_hip.lib().umhs_pack_info(ptr(ray_indices), ray_indices.shape[0], num_rays, ptr(out), _hip.stream()),
               "umhs_pack_info")
    return out


def composite_fwd(sigma, t0, t1, packed_info, values: Sequence[torch.Tensor]):
    R, n, dev = packed_info.shape[0], sigma.shape[0], sigma.device
    st = _hip.ValueStreams()
    st.n_streams = len(values)
    outs = []
    for i, v in enumerate(values):
        o = torch.empty((R, v.shape[-1]), device=dev, dtype=torch.float32)
        st.k[i], st.values[i], st.out[i] = v.shape[-1], v.data_ptr(), o.data_ptr()
        outs.append(o)
    weights = torch.empty((n,), device=dev, dtype=torch.float32)
    acc = torch.empty((R,), device=dev, dtype=torch.float32)
    depth = torch.empty((R,), device=dev, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_composite_fwd(ptr(sigma), ptr(t0), ptr(t1), ptr(packed_info), R, n, C.byref(st), ptr(weights),
                                             ptr(acc), ptr(depth), _hip.stream()), "umhs_composite_fwd")
    return weights, acc, depth, outs


def composite_bwd(sigma, t0, t1, packed_info, weights, values, d_outs, want_dvalues, d_acc, grad_scaling: bool):
    R, n, dev = packed_info.shape[0], sigma.shape[0], sigma.device
    g = _hip.ValueGrads()
    d_values: List[Optional[torch.Tensor]] = []
    k = 0
    for v, do, want in zip(values, d_outs, want_dvalues):
        if do is None:
            d_values.append(None)
            continue
        dv = torch.empty_like(v) if want else None
        g.k[k], g.values[k], g.d_out[k] = v.shape[-1], v.data_ptr(), do.data_ptr()
        g.d_values[k] = dv.data_ptr() if dv is not None else None
        d_values.append(dv)
        k += 1
    g.n_streams = k
    d_sigma = torch.empty((n,), device=dev, dtype=torch.float32)  # every packed sample belongs to a ray: fully written
    _hip.check(_hip.lib().umhs_composite_bwd(ptr(sigma), ptr(t0), ptr(t1), ptr(packed_info), R, n, ptr(weights), C.byref(g),
                                             ptr(d_acc), int(grad_scaling), ptr(d_sigma), _hip.stream()), "umhs_composite_bwd")
    return d_sigma, d_values


def spec2rgb_fwd(spec_t, M):
    R, B = spec_t.shape
    rgb = torch.empty((R, 3), device=spec_t.device, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_spec2rgb_fwd(ptr(spec_t), ptr(M), R, B, ptr(rgb), _hip.stream()), "umhs_spec2rgb_fwd")
    return rgb


def spec2rgb_bwd(spec_t, M, d_rgb, accumulate_into=None):
    R, B = spec_t.shape
    d_spec = torch.empty_like(spec_t) if accumulate_into is None else accumulate_into
    _hip.check(_hip.lib().umhs_spec2rgb_bwd(ptr(spec_t), ptr(M), ptr(d_rgb), R, B, ptr(d_spec), int(accumulate_into is not None), _hip.stream()),
               "umhs_spec2rgb_bwd")
    return d_spec


def adam_step(p, g, m, v, step: int, lr: float, betas=(0.9, 0.999), eps=1e-15, grad_scale=1.0, clamp_range=(0, 0)):
    _hip.check(_hip.lib().umhs_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, step,
                                         grad_scale, clamp_range[0], clamp_range[1], _hip.stream()), "umhs_adam_step")


def pixel_indices(uniform, n_images: int, height: int, width: int):
    """PixelSampler.sample_method: long(uniform[R,3] * (n, H, W)) -> [R,3] int64 rows (camera, y, x)."""
    u = _hip.f32c(uniform)
    out = torch.empty(u.shape, dtype=torch.int64, device=u.device)
    _hip.check(_hip.lib().umhs_pixel_indices(ptr(u), u.shape[0], n_images, height, width, ptr(out), _hip.stream()), "umhs_pixel_indices")
    return out


def mask_lists(mask_stack, device=None):
    """Set pixels of a uint8 mask stack [n,H,W] (set: byte != 0) -> (off [n+1] int64, list [M] int32), both on the device:
    ``off`` is the exclusive prefix sum of the per-image counts (M = off[n]) and ``list`` holds the flat ids y*W + x of the set
    pixels, ascending within an image, images in order -- the second column of ``torch.nonzero(mask.view(n, -1))``.  A stack in host
    memory (``device``: where the lists go) is uploaded one frame at a time and ends with the same bits.  Runs once per split, at
    load: it reads M back to size the list."""
    if mask_stack.dim() != 3 or mask_stack.dtype != torch.uint8:
        raise ValueError(f"mask stack must be uint8 [n,H,W], got {mask_stack.dtype} {tuple(mask_stack.shape)}")
    n, h, w = mask_stack.shape
    resident = mask_stack.is_cuda
    dev = mask_stack.device if resident else torch.device("cuda" if device is None else device)
    if n == 0 or h * w == 0:
        return torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    lib, pixels = _hip.lib(), h * w
    cpi = int(lib.umhs_mask_chunks(pixels))
    counts = torch.zeros((n, cpi), dtype=torch.int32, device=dev)
    if resident:
        pieces = [(mask_stack.contiguous(), 0, n)]
    else:  # one frame on the device at a time, in ONE buffer: both passes see the same address (the chunks depend on its alignment)
        frame = torch.empty((1, h, w), dtype=torch.uint8, device=dev)
        pieces = [(frame, i, 1) for i in range(n)]

    def each_piece():
        for buf, first, k in pieces:
            if not resident:
                buf.copy_(mask_stack[first : first + 1])
            yield buf, first, k

    for buf, first, k in each_piece():
        _hip.check(lib.umhs_mask_count(ptr(buf), k, pixels, ptr(counts[first : first + k]), _hip.stream()), "umhs_mask_count")
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(counts.sum(1, dtype=torch.int64), 0)
    flat = counts.view(-1).to(torch.int64)
    chunk_off = (torch.cumsum(flat, 0) - flat).view(n, cpi)  # exclusive scan: where each chunk's ids start in the whole list
    total = int(off[-1])
    lst = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        for buf, first, k in each_piece():
            _hip.check(lib.umhs_mask_compact(ptr(buf), k, pixels, ptr(chunk_off[first : first + k]), ptr(lst), total, _hip.stream()),
                       "umhs_mask_compact")
    return off, lst


def pixel_indices_masked(uniform, off, lst, width: int):
    """The mask-aware draw: rows (image, y, x) int64 [R,3], uniform over the set pixels ``mask_lists`` compacted, with replacement,
    from the same uniform[R,3] block ``pixel_indices`` takes (column 0 picks the image through ``off``, column 1 the rank within
    it, column 2 is unused).  No host sync."""
    u = _hip.f32c(uniform)
    if off.dtype != torch.int64 or lst.dtype != torch.int32 or off.dim() != 1 or off.shape[0] < 2:
        raise ValueError(f"off must be int64 [n+1] and list int32 [M], got {off.dtype} {tuple(off.shape)} / {lst.dtype} {tuple(lst.shape)}")
    out = torch.empty(u.shape, dtype=torch.int64, device=u.device)
    if u.shape[0] and not lst.numel():
        raise ValueError("the mask list is empty: no pixel to draw")
    _hip.check(_hip.lib().umhs_pixel_indices_masked(ptr(u), u.shape[0], off.shape[0] - 1, width, ptr(off), ptr(lst), ptr(out),
                                                    _hip.stream()), "umhs_pixel_indices_masked")
    return out


def raygen(indices, c2w, intrinsics, want_area: bool = True, want_norm: bool = False, distortion=None):
    """Cameras.generate_rays for perspective cameras: -> origins [R,3], directions [R,3], pixel_area [R,1] | None, norm | None.
    ``distortion`` [n,6] = (k1, k2, k3, k4, p1, p2) per camera: OpenCV lens distortion, undone per ray by ``umhs_raygen_distorted``."""
    r, dev = indices.shape[0], indices.device
    o, d = torch.empty(r, 3, device=dev), torch.empty(r, 3, device=dev)
    area = torch.empty(r, 1, device=dev) if want_area else None
    nrm = torch.empty(r, 1, device=dev) if want_norm else None
    if distortion is None:
        _hip.check(_hip.lib().umhs_raygen(ptr(indices), ptr(c2w), ptr(intrinsics), r, c2w.shape[0], ptr(o), ptr(d), ptr(area), ptr(nrm),
                                          _hip.stream()), "umhs_raygen")
        return o, d, area, nrm
    if distortion.shape != (c2w.shape[0], 6) or distortion.dtype != torch.float32:
        raise ValueError(f"distortion must be float32 [{c2w.shape[0]}, 6] (k1, k2, k3, k4, p1, p2), got {distortion.dtype} {tuple(distortion.shape)}")
    _hip.check(_hip.lib().umhs_raygen_distorted(ptr(indices), ptr(c2w), ptr(intrinsics), ptr(distortion), r, c2w.shape[0], ptr(o), ptr(d),
                                                ptr(area), ptr(nrm), _hip.stream()), "umhs_raygen_distorted")
    return o, d, area, nrm


CAMERA_TYPES = {"perspective": 0, "fisheye": 1, "equirectangular": 2}  # umhs_raygen_frame's camera_type


def obb_host15(obb):
    """(T [3], R [3,3], S [3]) -- the box of ``export.obb_from_params`` -- as the 15 host floats the C boundary takes."""
    T, R, S = (np.asarray(torch.as_tensor(v).detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32) for v in obb)
    if T.size != 3 or R.shape != (3, 3) or S.size != 3:
        raise ValueError(f"a box is (T [3], R [3,3], S [3]), got shapes {T.shape}, {R.shape}, {S.shape}")
    if not bool((S > 0).all()):
        raise ValueError(f"the scale of a box must be positive, got {S.reshape(-1).tolist()}")
    return (_hip._f32 * 15)(*T.reshape(-1).tolist(), *R.reshape(-1).tolist(), *S.reshape(-1).tolist())


def raygen_frame(c2w, intrinsics, camera: int, height: int, width: int, camera_type: str = "perspective", distortion=None, obb=None,
                 near_floor: float = 0.0, rows: Optional[Tuple[int, int]] = None):
    """The rays of one camera's frame -- or of its rows ``rows = (row0, n_rows)`` -- in one launch of ``umhs_raygen_frame``, no index
    tensor: ray i is pixel (row0 + i // width, i % width).  ``camera_type``: perspective (``distortion`` [n,6] as in ``raygen``: the same
    bits as ``raygen`` on meshgrid indices), fisheye or equirectangular.  ``obb`` = (T, R, S): a crop box, intersected per ray;
    ``near_floor`` is the least ``nears`` of a hit.
    -> origins [R,3], directions [R,3], pixel_area [R,1], directions_norm [R,1], nears [R,1] | None, fars [R,1] | None."""
    if camera_type not in CAMERA_TYPES:
        raise ValueError(f"camera_type {camera_type!r}: one of {', '.join(CAMERA_TYPES)}")
    n, dev = c2w.shape[0], c2w.device
    row0, n_rows = (0, int(height)) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= int(camera) < n:
        raise IndexError(f"camera index {camera} outside 0..{n - 1}")
    if height < 1 or width < 1 or row0 < 0 or n_rows < 0 or row0 + n_rows > height:
        raise ValueError(f"rows {row0}..{row0 + n_rows} outside a frame of {height} x {width}")
    if distortion is not None:
        if camera_type != "perspective":
            raise ValueError(f"lens distortion belongs to perspective cameras, not to {camera_type}")
        if distortion.shape != (n, 6) or distortion.dtype != torch.float32:
            raise ValueError(f"distortion must be float32 [{n}, 6] (k1, k2, k3, k4, p1, p2), got {distortion.dtype} {tuple(distortion.shape)}")
    if not near_floor >= 0:
        raise ValueError(f"near_floor must not be negative, got {near_floor}")
    box = None if obb is None else obb_host15(obb)
    r = n_rows * int(width)
    o, d = torch.empty(r, 3, device=dev), torch.empty(r, 3, device=dev)
    area, nrm = torch.empty(r, 1, device=dev), torch.empty(r, 1, device=dev)
    nears, fars = (torch.empty(r, 1, device=dev), torch.empty(r, 1, device=dev)) if box is not None else (None, None)
    if r == 0:  # no row: nothing to launch (an empty tensor has no address to hand over)
        return o, d, area, nrm, nears, fars
    _hip.check(_hip.lib().umhs_raygen_frame(ptr(_hip.f32c(c2w)), ptr(_hip.f32c(intrinsics)), ptr(distortion), n, int(camera),
                                            CAMERA_TYPES[camera_type], int(height), int(width), row0, n_rows, box, float(near_floor), ptr(o),
                                            ptr(d), ptr(area), ptr(nrm), ptr(nears), ptr(fars), _hip.stream()), "umhs_raygen_frame")
    return o, d, area, nrm, nears, fars


def pixel_gather(indices, stack):
    """batch[key] = stack[c, y, x] for a resident image stack [n,H,W,K] (fp32, or uint8 -> /255)."""
    assert stack.dim() == 4 and stack.is_contiguous() and stack.dtype in (torch.float32, torch.uint8)
    n, h, w, k = stack.shape
    out = torch.empty(indices.shape[0], k, device=indices.device)
    _hip.check(_hip.lib().umhs_pixel_gather(ptr(indices), ptr(stack), int(stack.dtype == torch.uint8), n, h, w, k, indices.shape[0],
                                            ptr(out), _hip.stream()), "umhs_pixel_gather")
    return out


def vca_rows_per_partial() -> int:
    """K: rows a workgroup of ``vca_moments`` accumulates in fp32 before the partial goes to float64 (its error bound is that of an
    fp32 dot product of length K)."""
    return int(_hip.lib().umhs_vca_rows_per_partial())


def _vca_ws(nbytes: int, dev) -> torch.Tensor:
    # (a one-shot initialiser: the workspace goes back to the allocator, it is not parked in the step's slots)
    return torch.empty(max(int(nbytes), 8), device=dev, dtype=torch.uint8)


def vca_moments(rows, sum_out=None, s_out=None):
    """(sum [B], S [B,B]) float64 of pixel rows [N,B] fp32: sum_n y_nb and sum_n y_ni y_nj.  Given ``sum_out`` / ``s_out`` (both) the
    call ADDS to them -- a stack is fed one frame at a time.  Bitwise reproducible."""
    assert rows.dim() == 2 and rows.dtype == torch.float32 and (sum_out is None) == (s_out is None)
    n, b = rows.shape
    accumulate = sum_out is not None
    if not accumulate:
        sum_out, s_out = (torch.zeros(s, dtype=torch.float64, device=rows.device) for s in ((b,), (b, b)))
    lib = _hip.lib()
    ws = _vca_ws(lib.umhs_vca_moments_workspace_bytes(n, b), rows.device)
    _hip.check(lib.umhs_vca_moments(ptr(rows), n, b, int(accumulate), ptr(sum_out), ptr(s_out), ptr(ws), ws.numel(), _hip.stream()),
               "umhs_vca_moments")
    return sum_out, s_out


def vca_project(rows, basis16, num_classes: int, mean=None, out=None):
    """y [N,16] fp32 from rows [N,B] and basis16 [B,16].  ``mean`` None: the projective form (column 15 of the basis = Ud u,
    y = x / (x_15 + 1e-6)) -> (y, None); ``mean`` [B]: the affine form x = basis^T (row - mean) -> (y, max_n |x_n|^2 as a 1-element
    tensor).  ``out``: a [N,16] slice of a larger y to fill."""
    assert rows.dim() == 2 and rows.dtype == torch.float32 and tuple(basis16.shape) == (rows.shape[1], 16)
    n, b = rows.shape
    dev = rows.device
    y = torch.empty(n, 16, device=dev, dtype=torch.float32) if out is None else out
    assert tuple(y.shape) == (n, 16) and y.dtype == torch.float32
    affine = mean is not None
    mx = torch.zeros(1, device=dev, dtype=torch.float32) if affine else None
    lib = _hip.lib()
    ws = _vca_ws(lib.umhs_vca_project_workspace_bytes(n), dev)
    _hip.check(lib.umhs_vca_project(ptr(rows), n, b, ptr(_hip.f32c(basis16)), ptr(_hip.f32c(mean)) if affine else None, int(num_classes),
                                    int(affine), ptr(y), ptr(mx), ptr(ws), ws.numel(), _hip.stream()), "umhs_vca_project")
    return y, mx


def vca_argmax(y, f, bias: float = 0.0):
    """argmax_n |bias + f . y_n| over y [N,16] (``f``: up to 16 host floats), the lowest index among equal values
    -> (index [1] int64, row [16] fp32, value [1] fp32), all on the device."""
    assert y.dim() == 2 and y.shape[1] == 16 and y.dtype == torch.float32 and y.shape[0] > 0
    dev = y.device
    fh = (_hip._f32 * 16)(*[float(v) for v in f])
    index = torch.zeros(1, dtype=torch.int64, device=dev)
    row, value = torch.zeros(16, device=dev), torch.zeros(1, device=dev)
    lib = _hip.lib()
    ws = _vca_ws(lib.umhs_vca_argmax_workspace_bytes(y.shape[0]), dev)
    _hip.check(lib.umhs_vca_argmax(ptr(y), y.shape[0], fh, float(bias), ptr(index), ptr(row), ptr(value), ptr(ws), ws.numel(),
                                   _hip.stream()), "umhs_vca_argmax")
    return index, row, value


def pixel_metrics(pred, gt):
    """(sum of squared errors, sum of finite spectral angles, number of finite angles) over channel-last images [...,K]; float64."""
    k = pred.shape[-1]
    p, g = _hip.f32c(pred).view(-1, k), _hip.f32c(gt).view(-1, k)
    assert p.shape == g.shape
    nb = max(1, min(1024, (p.shape[0] + 255) // 256))
    part = torch.empty(nb, 3, dtype=torch.float64, device=p.device)
    _hip.check(_hip.lib().umhs_pixel_metrics(ptr(p), ptr(g), p.shape[0], k, ptr(part), nb, _hip.stream()), "umhs_pixel_metrics")
    return part.sum(0)


class SegmentBounds:
    """Ascending element offsets [K+1] of ``segment_stats``, kept in both places the call needs them: ``host`` (the argument checks and
    the grid size are host arithmetic) and ``device`` (what the kernels read).  Built once -- ``SegmentBounds(offsets, device)`` or
    ``SegmentBounds.of_layout(layout, device)`` -- and reused, so a call uploads nothing and reads nothing back."""

    def __init__(self, offsets, device):
        values = [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]  # (a device tensor is read once, here)
        if len(values) < 2:
            raise ValueError("segment bounds need at least two offsets (K >= 1)")
        self.k = len(values) - 1
        self.values = values
        self.host = (_hip._i64 * len(values))(*values)
        self.device = torch.tensor(values, dtype=torch.int64, device=device)
        self.names: Optional[List[str]] = None

    @classmethod
    def of_layout(cls, layout, device) -> "SegmentBounds":
        """One segment per entry of a flat parameter layout, in layout order: entry i = [offset_i, offset_i + numel_i).  The layout pads
        every entry to 16 bytes, so segment i is cut at offset_{i+1} and a statistics row covers the entry plus its (zero) padding."""
        names = list(layout.entries)
        offsets = [layout.entries[k][0] for k in names] + [layout.total]
        self = cls(offsets, device)
        self.names = names
        return self


def segment_stats_tile() -> int:
    """Elements per tile of ``segment_stats`` (its error bound is a function of it: tests/stats_f64.py)."""
    return int(_hip.lib().umhs_segment_stats_tile())


def segment_stats(x, bounds, out=None):
    """float64 [K,3] per segment ``[bounds[k], bounds[k+1])`` of the contiguous float32 device buffer ``x``: the sum of x^2 and the
    maximum of |x| over the finite elements, and the number of NaN / +-Inf.  ``bounds``: a ``SegmentBounds`` (nothing is uploaded) or
    int64 offsets [K+1] as a list / tensor (a ``SegmentBounds`` is built for the call; a device tensor costs a host read).  One pass over
    ``x``, float64 sums in a fixed order (the same bits on every launch), no host sync; descending offsets or offsets outside the buffer
    raise before anything is launched.  ``out``: a float64 [K,3] device tensor to fill."""
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise ValueError("segment_stats needs a float32 tensor")
    flat = x.detach().reshape(-1) if x.is_contiguous() else None
    pointer = ptr(flat if flat is not None else x.detach())  # (a CPU or non-contiguous tensor raises here: there is no CPU path)
    if not isinstance(bounds, SegmentBounds):
        bounds = SegmentBounds(bounds, flat.device)
    if bounds.device.device != flat.device:
        raise ValueError(f"segment bounds live on {bounds.device.device}, the buffer on {flat.device}")
    if out is None:
        out = torch.empty(bounds.k, 3, dtype=torch.float64, device=flat.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (bounds.k, 3) or out.device != flat.device:
        raise ValueError(f"out must be float64 [{bounds.k}, 3] on {flat.device}")
    lib = _hip.lib()
    ws = _scratch(flat.device, "segment_stats", lib.umhs_segment_stats_workspace_bytes(flat.numel(), bounds.k))
    _hip.check(lib.umhs_segment_stats(pointer, flat.numel(), ptr(bounds.device), bounds.host, bounds.k, ptr(out), ptr(ws), ws.numel(),
                                      _hip.stream()), "umhs_segment_stats")
    return out


def seg_confusion(seg_raw, accumulation, seg_image, n_classes: int, n_labels: int, ignore_label: int = 255, out=None):
    """Confusion table int64 [n_classes + 1, n_labels] of the labels the model emitted against a ground-truth label image: per pixel
    one count at [accumulation > 0.5 ? seg_raw : n_classes, seg_image] (the last row is "nothing rendered"); pixels whose label is
    ``ignore_label`` (-1: none) or >= n_labels, or whose ``seg_raw`` is no class, are skipped.  Any shapes with equal element counts;
    ``out``: a table to ADD into (returned).  One launch, no host sync."""
    raw, acc = _hip.f32c(seg_raw).reshape(-1), _hip.f32c(accumulation).reshape(-1)
    if seg_image.dtype != torch.uint8:
        raise ValueError(f"seg_image must be uint8, got {seg_image.dtype}")
    lab = seg_image.reshape(-1)  # (a view of a contiguous slice keeps its byte offset: the kernel takes any alignment)
    if not raw.numel() == acc.numel() == lab.numel():
        raise ValueError(f"seg_raw, accumulation and seg_image differ in size: {raw.numel()}, {acc.numel()}, {lab.numel()}")
    pointers = ptr(raw), ptr(acc), ptr(lab)  # (a CPU tensor raises here: there is no CPU path)
    if out is None:
        out = torch.zeros(n_classes + 1, n_labels, dtype=torch.int64, device=raw.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n_classes + 1, n_labels):
        raise ValueError(f"out must be int64 [{n_classes + 1}, {n_labels}], got {out.dtype} {tuple(out.shape)}")
    if raw.numel() == 0:
        return out
    _hip.check(_hip.lib().umhs_seg_confusion(*pointers, raw.numel(), int(n_classes), int(n_labels), int(ignore_label),
                                             ptr(out), _hip.stream()), "umhs_seg_confusion")
    return out


PANEL_RGB, PANEL_SCALAR, PANEL_DEPTH = 0, 1, 2  # include/umhs_hip.h UMHS_PANEL_*


@dataclass
class FramePanel:
    """One panel of ``frame_compose`` (umhs_frame_panel).  ``src``: float32 rows on the device, [H*W], [H*W, c] or [H, W, c], read in
    place -- a column view such as ``spectral[:, 7]`` or ``abundances[:, 2:3]`` is taken at its own row stride, nothing is copied.
    ``channel``: first column of ``src`` read (RGB reads three).  ``range``: device (lo, hi) of DEPTH and of SCALAR with
    ``normalize``.  ``accumulation``: [H*W] floats a DEPTH panel is blended over white with."""
    src: torch.Tensor
    kind: int = PANEL_SCALAR
    channel: int = 0
    range: Optional[torch.Tensor] = None
    accumulation: Optional[torch.Tensor] = None
    normalize: bool = False
    invert: bool = False
    cmin: float = 0.0
    cmax: float = 1.0


def _frame_f32(t, what: str, dev=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"frame_compose: {what} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"frame_compose: {what} must be float32, got {t.dtype}")
    if dev is not None and t.device != dev:
        raise ValueError(f"frame_compose: {what} is on {t.device}, the colour table on {dev}")
    return t


def _frame_rows(src, n: int, what: str):
    """(tensor whose data_ptr is row 0, floats per row, columns) of a source of n rows that is read in place."""
    lead = src.numel() if src.dim() <= 1 else int(np.prod(src.shape[:-1]))
    if lead != n:
        raise ValueError(f"frame_compose: {what} of shape {tuple(src.shape)} does not hold {n} rows")
    try:
        rows = src.reshape(n, 1) if src.dim() <= 1 else src if src.dim() == 2 else src.view(n, src.shape[-1])
    except RuntimeError as e:
        raise ValueError(f"frame_compose: {what} of shape {tuple(src.shape)} is not {n} rows that can be read in place") from e
    c = rows.shape[1]
    if c == 0 or (c > 1 and rows.stride(1) != 1):
        raise ValueError(f"frame_compose: the columns of {what} must be adjacent floats (strides {tuple(rows.stride())})")
    stride = rows.stride(0) if n > 1 else c
    if stride < c:
        raise ValueError(f"frame_compose: the rows of {what} overlap (strides {tuple(rows.stride())})")
    return rows, stride, c


def frame_compose(panels: Sequence[FramePanel], lut, height: int, width: int, out=None):
    """uint8 [height, K * width, 3]: the K panels side by side, each the displayable form of one per-ray output (umhs_frame_compose:
    RGB quantised; SCALAR through nerfstudio's apply_float_colormap; DEPTH through apply_depth_colormap).  ``lut``: float32 [256, 3]
    colour table on the device.  ``out``: a contiguous uint8 tensor of that many elements at ANY byte offset (a view of a larger
    buffer).  One launch, no host sync; the sources are kept alive by ``panels`` until the launch has been queued."""
    panels = list(panels)
    height, width, K = int(height), int(width), len(panels)
    if height < 0 or width < 0 or not 1 <= K <= 16:
        raise ValueError(f"frame_compose: {K} panels of {height} x {width} (1..16 panels, sizes >= 0)")
    lut = _frame_f32(lut, "lut")
    if tuple(lut.shape) != (256, 3) or not lut.is_contiguous():
        raise ValueError(f"frame_compose: lut must be a contiguous [256, 3], got {tuple(lut.shape)}")
    dev, n = lut.device, height * width
    arr, keep = (_hip.FramePanel * K)(), []
    for k, p in enumerate(panels):
        if p.kind not in (PANEL_RGB, PANEL_SCALAR, PANEL_DEPTH):
            raise ValueError(f"frame_compose: panel {k} has kind {p.kind}")
        rows, stride, c = _frame_rows(_frame_f32(p.src, f"panel {k}", dev), n, f"panel {k}")
        need = 3 if p.kind == PANEL_RGB else 1
        if p.channel < 0 or p.channel + need > c:
            raise ValueError(f"frame_compose: panel {k} reads columns {p.channel}..{p.channel + need - 1} of {c}")
        wants_range = p.kind == PANEL_DEPTH or (p.kind == PANEL_SCALAR and p.normalize)
        rng = acc = None
        if wants_range:
            if p.range is None:
                raise ValueError(f"frame_compose: panel {k} needs a (lo, hi) range")
            rng = _frame_f32(p.range, f"range of panel {k}", dev)
            if rng.numel() != 2 or not rng.is_contiguous():
                raise ValueError(f"frame_compose: range of panel {k} must be 2 contiguous floats, got {tuple(rng.shape)}")
        if p.kind == PANEL_DEPTH and p.accumulation is not None:
            acc = _frame_f32(p.accumulation, f"accumulation of panel {k}", dev)
            if acc.numel() != n or not acc.is_contiguous():
                raise ValueError(f"frame_compose: accumulation of panel {k} must be {n} contiguous floats, got {tuple(acc.shape)}")
        keep += [rows, rng, acc]
        arr[k] = _hip.FramePanel(rows.data_ptr() if n else 4, rng.data_ptr() if rng is not None else None,
                                 acc.data_ptr() if acc is not None and n else None, max(stride, p.channel + need), p.channel, p.kind,
                                 int(bool(p.normalize)) | 2 * int(bool(p.invert)), float(p.cmin), float(p.cmax))
    if out is None:
        out = torch.empty(height, K * width, 3, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or out.numel() != 3 * K * n or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f"frame_compose: out must be {3 * K * n} contiguous uint8 on {dev}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    if n == 0:
        return out.view(height, K * width, 3)
    _hip.check(_hip.lib().umhs_frame_compose(arr, K, ptr(lut), height, width, C.c_void_p(out.data_ptr()), _hip.stream()),
               "umhs_frame_compose")
    del keep
    return out.view(height, K * width, 3)


# ---- baseline-JPEG frame encoder (umhs_jpeg.hip) --------------------------------------------------------------------------------------
JPEG_SUBSAMPLING = {"444": 0, "420": 1}  # UMHS_JPEG_444 / UMHS_JPEG_420
JPEG_HEADER_BYTES = 629
# MCUs per restart interval (one wavefront each) when the caller names none: tools/bench_video.py's sweep
JPEG_DEFAULT_RESTART_MCUS = 16


def _jpeg_frame(frame):
    if not torch.is_tensor(frame) or not frame.is_cuda:
        raise ValueError("jpeg: the frame must be a tensor on a HIP device (there is no CPU path)")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():
        raise ValueError(f"jpeg: the frame must be a contiguous uint8 [H, W, 3], got {frame.dtype} {tuple(frame.shape)}")
    H, W = int(frame.shape[0]), int(frame.shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"jpeg: a frame of {H} x {W} has no pixel")
    return H, W


def _jpeg_params(quality, subsampling, restart_mcus):
    if str(subsampling) not in JPEG_SUBSAMPLING:
        raise ValueError(f"jpeg: subsampling must be one of {', '.join(JPEG_SUBSAMPLING)}, got {subsampling!r}")
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"jpeg: quality must be 1..100, got {quality}")
    restart_mcus = JPEG_DEFAULT_RESTART_MCUS if restart_mcus is None else int(restart_mcus)
    if not 1 <= restart_mcus <= 65535:
        raise ValueError(f"jpeg: restart_mcus must be 1..65535, got {restart_mcus}")
    return quality, JPEG_SUBSAMPLING[str(subsampling)], restart_mcus


def jpeg_blocks_per_mcu(subsampling) -> int:
    return 6 if str(subsampling) == "420" else 3


def jpeg_workspace_bytes(height: int, width: int, subsampling="420", restart_mcus=None) -> int:
    _, ss, r = _jpeg_params(100, subsampling, restart_mcus)
    return int(_hip.lib().umhs_jpeg_workspace_bytes(int(height), int(width), ss, r))


def jpeg_max_bytes(height: int, width: int, subsampling="420", restart_mcus=None) -> int:
    """An upper bound on the length of the file for ANY content of the frame."""
    _, ss, r = _jpeg_params(100, subsampling, restart_mcus)
    return int(_hip.lib().umhs_jpeg_max_bytes(int(height), int(width), ss, r))


def jpeg_coefficients(frame, quality: int = 100, subsampling="420"):
    """The transform stage of the frame encoder (umhs_jpeg_coefficients): uint8 [H, W, 3] at any byte address -> int16 [n_mcus, 3 or 6,
    64], the blocks of an MCU in scan order and their coefficients in zigzag order.  One launch, no sync."""
    H, W = _jpeg_frame(frame)
    quality, ss, _ = _jpeg_params(quality, subsampling, 1)
    bpm = jpeg_blocks_per_mcu(subsampling)
    n_blocks = int(_hip.lib().umhs_jpeg_blocks(H, W, ss))
    if n_blocks == 0:
        raise ValueError(f"jpeg: a frame of {H} x {W} is outside 1..65535")
    out = torch.empty(n_blocks // bpm, bpm, 64, dtype=torch.int16, device=frame.device)
    _hip.check(_hip.lib().umhs_jpeg_coefficients(C.c_void_p(frame.data_ptr()), H, W, quality, ss, C.c_void_p(out.data_ptr()), _hip.stream()),
               "umhs_jpeg_coefficients")
    return out


def _jpeg_out(out, length, dev, capacity):
    if out is None:
        out = torch.empty(int(capacity), dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"jpeg: out must be a contiguous uint8 vector on {dev}")
    if length is None:
        length = torch.empty(1, dtype=torch.int64, device=dev)
    elif not torch.is_tensor(length) or length.dtype != torch.int64 or length.numel() != 1 or length.device != dev:
        raise ValueError(f"jpeg: length must be one int64 on {dev}")
    return out, length


def jpeg_encode(frame, quality: int = 100, subsampling="420", restart_mcus=None, out=None, length=None, workspace=None):
    """One baseline-JPEG file of ``frame`` (uint8 [H, W, 3] on the device, any byte address), encoded on the device (umhs_jpeg_encode).
    -> (out uint8 [capacity], length int64 [1]), both on the device: the file is ``out[:length]``.  ``out``: the buffer to fill (its
    size is the capacity; default: ``jpeg_max_bytes``, which no content exceeds); when the file is longer than the capacity, nothing is
    written past it and ``length`` holds the size needed.  ``workspace``: uint8 of at least ``jpeg_workspace_bytes`` (default: a new
    one).  Four launches on the current stream, no sync."""
    H, W = _jpeg_frame(frame)
    quality, ss, r = _jpeg_params(quality, subsampling, restart_mcus)
    lib, dev = _hip.lib(), frame.device
    need = int(lib.umhs_jpeg_workspace_bytes(H, W, ss, r))
    if need == 0:
        raise ValueError(f"jpeg: a frame of {H} x {W} is outside 1..65535")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"jpeg: the workspace must be at least {need} contiguous uint8 on {dev}")
    out, length = _jpeg_out(out, length, dev, lib.umhs_jpeg_max_bytes(H, W, ss, r))
    _hip.check(lib.umhs_jpeg_encode(C.c_void_p(frame.data_ptr()), H, W, quality, ss, r, C.c_void_p(out.data_ptr()), out.numel(),
                                    C.c_void_p(length.data_ptr()), C.c_void_p(workspace.data_ptr()), workspace.numel(), _hip.stream()),
               "umhs_jpeg_encode")
    return out, length


def jpeg_entropy(coefficients, height: int, width: int, quality: int = 100, subsampling="420", restart_mcus=None, out=None, length=None):
    """The entropy stage alone (umhs_jpeg_entropy) on given coefficients, int16 [n_mcus, 3 or 6, 64] as ``jpeg_coefficients`` lays them
    out -> (out, length) as ``jpeg_encode``."""
    quality, ss, r = _jpeg_params(quality, subsampling, restart_mcus)
    lib, H, W = _hip.lib(), int(height), int(width)
    n_blocks = int(lib.umhs_jpeg_blocks(H, W, ss))
    if (not torch.is_tensor(coefficients) or not coefficients.is_cuda or coefficients.dtype != torch.int16 or not coefficients.is_contiguous()
            or n_blocks == 0 or coefficients.numel() != 64 * n_blocks):
        raise ValueError(f"jpeg: the coefficients of a {H} x {W} frame are {n_blocks} x 64 contiguous int16 on a HIP device")
    dev = coefficients.device
    n_mcus = n_blocks // jpeg_blocks_per_mcu(subsampling)
    table = torch.empty((n_mcus + r - 1) // r, dtype=torch.int64, device=dev)
    out, length = _jpeg_out(out, length, dev, lib.umhs_jpeg_max_bytes(H, W, ss, r))
    _hip.check(lib.umhs_jpeg_entropy(C.c_void_p(coefficients.data_ptr()), H, W, quality, ss, r, C.c_void_p(out.data_ptr()), out.numel(),
                                     C.c_void_p(length.data_ptr()), C.c_void_p(table.data_ptr()), 8 * table.numel(), _hip.stream()),
               "umhs_jpeg_entropy")
    return out, length


# ---- point-cloud export (umhs_pointcloud.hip) ---------------------------------------------------------------------------------------
PC_MAX_CELLS, PC_MAX_DIM = 1 << 21, 4096  # umhs_pc_cell_keys / umhs_knn_mean_dist: cells of a grid, cells along one axis


def pc_row_bytes(n_classes: int) -> int:
    """Bytes of one packed row: 16 (x y z, red green blue alpha) or 20 + 4 C (the same, int material, C float abundances)."""
    return 16 if n_classes == 0 else 20 + 4 * int(n_classes)


def _pc_rows(t, n: int, cols: int, what: str, dev):
    """(tensor kept alive, floats per row) of a float32 source of n rows with at least ``cols`` adjacent columns, read in place."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"pc: {what} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32 or t.device != dev:
        raise ValueError(f"pc: {what} must be float32 on {dev}, got {t.dtype} on {t.device}")
    rows = t.reshape(n, 1) if t.dim() <= 1 else t
    if rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < cols or (rows.shape[1] > 1 and rows.stride(1) != 1):
        raise ValueError(f"pc: {what} must be [{n}, >={cols}] with adjacent columns, got {tuple(t.shape)} strides {tuple(t.stride())}")
    stride = rows.stride(0) if n > 1 else rows.shape[1]
    if stride < cols or stride >= 1 << 31:
        raise ValueError(f"pc: the rows of {what} overlap or are too far apart (stride {stride})")
    return rows, stride


def pc_args(origins, directions, depth, accumulation, rgb, abundances=None, seg_probs=None, threshold: float = 0.5, box=None, world=None):
    """umhs_pc_args of one batch of rendered rays -> (struct, n_rays, n_classes, tensors to keep alive).  Sources: float32 [R, c] on one
    device, read in place at their own row stride.  ``abundances`` / ``seg_probs`` (both or neither, [R, C]) select the 20 + 4 C byte
    row.  ``box`` = (T [3], R [3,3], S [3]) of an oriented box (host values); ``world`` = [3,4] host affine for the written xyz."""
    if (abundances is None) != (seg_probs is None):
        raise ValueError("pc: abundances and seg_probs come together (or neither: the 16-byte row)")
    n, dev = origins.shape[0], origins.device
    C_ = 0 if abundances is None else int(abundances.shape[-1])
    if C_ and seg_probs.shape[-1] != C_:
        raise ValueError(f"pc: {C_} abundances but {seg_probs.shape[-1]} cluster probabilities per ray")
    a, keep = _hip.PcArgs(), []
    for name, t, cols in (("origins", origins, 3), ("directions", directions, 3), ("depth", depth, 1), ("accumulation", accumulation, 1),
                          ("rgb", rgb, 3), ("abundances", abundances, C_), ("seg_probs", seg_probs, C_)):
        if t is None:
            continue
        rows, stride = _pc_rows(t, n, cols, name, dev)
        keep.append(rows)
        setattr(a, name, rows.data_ptr() if n else 4)
        setattr(a, name + "_stride", stride)
    a.n_classes, a.threshold = C_, float(threshold)
    if box is not None:
        T, R, S = (np.asarray(v, dtype=np.float32) for v in box)
        if T.shape != (3,) or R.shape != (3, 3) or S.shape != (3,):
            raise ValueError("pc: box = (T [3], R [3,3], S [3])")
        a.has_box = 1
        a.box_center[:], a.box_rotation[:], a.box_scale[:] = T.tolist(), R.reshape(-1).tolist(), S.tolist()
    if world is not None:
        W = np.asarray(world, dtype=np.float32)
        if W.shape != (3, 4):
            raise ValueError("pc: world = [3,4] affine")
        a.has_world = 1
        a.world[:] = W.reshape(-1).tolist()
    return a, n, C_, keep


def pc_append(args, rows, points, kept, base, ordinal0: int, cap: int):
    """Append the kept rays of one batch (``args`` = ``pc_args(...)``) behind the ``base[0]`` rows written so far: count per chunk,
    exclusive scan (torch, a few hundred integers), emit.  ``rows`` uint8 [>= cap * row_bytes] (4-byte aligned), ``points`` float32
    [cap, 3], ``kept`` int64 [cap], ``base`` int64 [1] on the device.  -> the batch's kept count as a 0-dim int64 device tensor (the
    caller adds it to ``base``).  Rows at or beyond ``cap`` are dropped; no host sync."""
    a, n, C_, keep = args
    dev = base.device
    if (rows.dtype != torch.uint8 or not rows.is_contiguous() or rows.numel() < cap * pc_row_bytes(C_) or points.dtype != torch.float32
            or not points.is_contiguous() or points.numel() < 3 * cap or kept.dtype != torch.int64 or not kept.is_contiguous()
            or kept.numel() < cap or base.dtype != torch.int64 or base.numel() != 1):
        raise ValueError(f"pc_append: rows / points / kept / base do not hold {cap} rows of {pc_row_bytes(C_)} bytes")
    if n == 0:
        return torch.zeros((), dtype=torch.int64, device=dev)
    lib = _hip.lib()
    counts = torch.empty(int(lib.umhs_pc_chunks(n)), dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_pc_flag_count(C.byref(a), n, ptr(counts), _hip.stream()), "umhs_pc_flag_count")
    c64 = counts.to(torch.int64)
    incl = torch.cumsum(c64, 0)
    offsets = (incl - c64).contiguous()
    _hip.check(lib.umhs_pc_emit(C.byref(a), n, ptr(offsets), ptr(base), int(ordinal0), C.c_void_p(rows.data_ptr()), ptr(points),
                                ptr(kept), int(cap), _hip.stream()), "umhs_pc_emit")
    del keep
    return incl[-1]


def pc_grid(points, edge: Optional[float] = None, points_per_cell: float = 2.0):
    """The uniform grid of ``knn_mean_dist`` over the bounding box of points [M,3] -> (lo (3 floats), edge, dims (3 ints)).  Reads the
    box back (24 bytes).  ``edge`` None: the edge at which the box holds about ``points_per_cell`` points per cell; either way the edge
    grows until no axis has more than 4,096 cells and the grid no more than 2^21.  An axis without extent has one cell."""
    lo_t, hi_t = points.amin(0), points.amax(0)
    box = torch.stack([lo_t, hi_t]).double().cpu().numpy()
    lo, ext = box[0], box[1] - box[0]
    if not np.isfinite(box).all():
        raise ValueError("pc_grid: the points are not finite")
    if edge is None:
        live = ext[ext > 0]
        edge = 1.0 if live.size == 0 else float((np.prod(live) / max(points.shape[0] / points_per_cell, 1.0)) ** (1.0 / live.size))
    edge = float(np.float32(max(float(edge), float(np.finfo(np.float32).tiny))))
    while True:
        dims = [int(min(e / edge, 1e9)) + 1 for e in ext]
        if max(dims) <= PC_MAX_DIM and dims[0] * dims[1] * dims[2] <= PC_MAX_CELLS:
            return tuple(float(np.float32(v)) for v in lo), edge, tuple(dims)
        edge = float(np.float32(edge * 1.25))


def _pc_grid_c(lo, dims):
    return (_hip._f32 * 3)(*lo), (_hip._i32 * 3)(*dims)


def pc_cell_keys(points, lo, edge: float, dims):
    """int32 [M] cell keys (z-major) of points [M,3] in the grid ``pc_grid`` chose (umhs_pc_cell_keys)."""
    p = _hip.f32c(points)
    keys = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
    clo, cdims = _pc_grid_c(lo, dims)
    _hip.check(_hip.lib().umhs_pc_cell_keys(ptr(p), p.shape[0], clo, float(edge), cdims, ptr(keys), _hip.stream()), "umhs_pc_cell_keys")
    return keys


def knn_mean_dist(points, k: int, edge: Optional[float] = None):
    """float32 [M]: for every point of points [M,3] the mean Euclidean distance to its min(k, M) nearest points, itself included --
    what Open3D's ``remove_statistical_outlier`` thresholds  [upstream-recalled].  Exact.  Bin (HIP), sort by cell and build the
    cell-start table (torch: plumbing), search (HIP), scatter back to the points' order.  ``edge``: overrides the grid edge (the result
    does not depend on it; the time does)."""
    p = _hip.f32c(points)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"knn_mean_dist: points must be [M,3], got {tuple(p.shape)}")
    m, dev = p.shape[0], p.device
    if not 2 <= int(k) <= 32:
        raise ValueError(f"knn_mean_dist: k must be in 2..32, got {k}")
    if m == 0:
        return torch.empty(0, device=dev)
    plan = knn_plan(p, edge)
    mean = torch.empty(m, device=dev)
    mean[plan["order"]] = knn_search(plan, k)
    return mean


def knn_plan(p, edge: Optional[float] = None) -> Dict:
    """Everything ``knn_search`` needs of contiguous float32 points [M,3]: the grid, the points in cell order, the cell-start table."""
    lo, edge, dims = pc_grid(p, edge)
    keys = pc_cell_keys(p, lo, edge, dims)
    sorted_keys, order = torch.sort(keys, stable=True)
    cells = dims[0] * dims[1] * dims[2]
    start = torch.searchsorted(sorted_keys, torch.arange(cells + 1, dtype=torch.int32, device=p.device)).to(torch.int32)
    return {"lo": lo, "edge": edge, "dims": dims, "order": order, "points": p[order].contiguous(), "start": start}


def knn_search(plan: Dict, k: int, out=None):
    """umhs_knn_mean_dist on a ``knn_plan``: float32 [M] means in CELL order (``plan["order"]`` maps them back).  One launch."""
    sp = plan["points"]
    out = torch.empty(sp.shape[0], device=sp.device) if out is None else out
    clo, cdims = _pc_grid_c(plan["lo"], plan["dims"])
    _hip.check(_hip.lib().umhs_knn_mean_dist(ptr(sp), sp.shape[0], ptr(plan["start"]), clo, float(plan["edge"]), cdims, int(k), ptr(out),
                                             _hip.stream()), "umhs_knn_mean_dist")
    return out


# ---- mesh export (umhs_mesh.hip) ------------------------------------------------------------------------------------------------------
MESH_MAX_POINTS, MESH_MAX_CLASSES = 1 << 28, 16


def mesh_row_bytes(n_classes: int) -> int:
    """Bytes of one vertex row: 15 (x y z, red green blue) or 19 + 4 C (the same, int material, C float abundances)."""
    return 15 if n_classes == 0 else 19 + 4 * int(n_classes)


def tsdf_volume(lo, h: float, dims, n_classes: int, device) -> Dict:
    """An empty volume: lattice points ``lo + (x, y, z) * h``, ``dims`` = (nx, ny, nz), index ``(z * ny + y) * nx + x``.
    -> {"D", "W", "Wc" [N], "A" [3 + 2 C, N] (rgb, abundances, seg_probs planes), "lo", "h", "dims", "n_classes"}."""
    dims = tuple(int(d) for d in dims)
    lo = tuple(float(np.float32(v)) for v in lo)
    h = float(np.float32(h))
    n = dims[0] * dims[1] * dims[2] if len(dims) == 3 else 0
    if len(dims) != 3 or min(dims) < 1 or len(lo) != 3 or not h > 0 or not np.isfinite([*lo, h]).all():
        raise ValueError(f"tsdf_volume: dims {dims}, lo {lo}, h {h}")
    if n > MESH_MAX_POINTS or not 0 <= int(n_classes) <= MESH_MAX_CLASSES:
        raise ValueError(f"tsdf_volume: at most 2^28 lattice points and {MESH_MAX_CLASSES} classes, got {n} and {n_classes}")
    if torch.device(device).type != "cuda":
        raise RuntimeError("tsdf_volume: the volume lives on a HIP device (cuda:N); there is no CPU path")
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
    return {"D": z(n), "W": z(n), "Wc": z(n), "A": z(3 + 2 * int(n_classes), n), "lo": lo, "h": h, "dims": dims, "n_classes": int(n_classes)}


def _tsdf_volume_c(vol: Dict) -> "_hip.TsdfVolume":
    v = _hip.TsdfVolume()
    n = vol["dims"][0] * vol["dims"][1] * vol["dims"][2]
    k = 3 + 2 * vol["n_classes"]
    for name, numel in (("D", n), ("W", n), ("Wc", n), ("A", k * n)):
        t = vol[name]
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
            raise ValueError(f"tsdf: volume[{name!r}] must be a contiguous float32 device tensor of {numel} elements")
        setattr(v, name, t.data_ptr())
    v.dims[:], v.n_attr, v.lo[:], v.h = list(vol["dims"]), k, list(vol["lo"]), vol["h"]
    return v


def _tsdf_image(t, n: int, hgt: int, wid: int, cols: int, what: str, dev):
    """(tensor kept alive, (image, row, pixel) strides in floats) of a float32 [n, H, W(, >= cols)] source read in place."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"tsdf: {what} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32 or t.device != dev:
        raise ValueError(f"tsdf: {what} must be float32 on {dev}, got {t.dtype} on {t.device}")
    img = t.unsqueeze(-1) if t.dim() == 3 else t
    if img.dim() != 4 or tuple(img.shape[:3]) != (n, hgt, wid) or img.shape[3] < cols or (img.shape[3] > 1 and img.stride(3) != 1):
        raise ValueError(f"tsdf: {what} must be [{n}, {hgt}, {wid}, >={cols}] with adjacent channels, got {tuple(t.shape)} strides "
                         f"{tuple(t.stride())}")
    if min(img.stride()[:3]) < 0:
        raise ValueError(f"tsdf: {what} has a negative stride")
    return img, tuple(int(s) for s in img.stride()[:3])


def tsdf_integrate(vol: Dict, c2w, intrinsics, distortion, depth, accumulation, rgb, abundances=None, seg_probs=None,
                   opacity_threshold: float = 0.5, truncation: float = 0.1) -> None:
    """Fuse n rendered cameras into ``vol`` (umhs_tsdf_integrate; the rules are in include/umhs_hip.h).  ``c2w`` [n,3,4],
    ``intrinsics`` [n,4] = (fx, fy, cx, cy), ``distortion`` [n,6] or None: HOST values (numpy or CPU tensors).  ``depth`` /
    ``accumulation`` [n,H,W] or [n,H,W,1], ``rgb`` [n,H,W,3], ``abundances`` / ``seg_probs`` [n,H,W,C]: float32 device tensors read in
    place at their strides.  16 cameras go into one launch; more are fused in consecutive launches (the same bits either way)."""
    c2w = np.asarray(c2w, dtype=np.float32).reshape(-1, 3, 4)
    intr = np.asarray(intrinsics, dtype=np.float32).reshape(-1, 4)
    n = c2w.shape[0]
    dist = None if distortion is None else np.asarray(distortion, dtype=np.float32).reshape(-1, 6)
    if intr.shape[0] != n or (dist is not None and dist.shape[0] != n):
        raise ValueError("tsdf_integrate: c2w, intrinsics and distortion must describe the same cameras")
    if (abundances is None) != (seg_probs is None):
        raise ValueError("tsdf_integrate: abundances and seg_probs come together (or neither)")
    C_ = 0 if abundances is None else int(abundances.shape[-1])
    if C_ != vol["n_classes"] or (C_ and seg_probs.shape[-1] != C_):
        raise ValueError(f"tsdf_integrate: the volume holds {vol['n_classes']} classes, the images {C_}")
    if not (float(truncation) > 0 and np.isfinite(float(truncation))):
        raise ValueError(f"tsdf_integrate: truncation {truncation} must be positive")
    if n == 0:
        return
    v = _tsdf_volume_c(vol)
    dev = vol["D"].device
    if depth.dim() not in (3, 4) or depth.shape[0] != n:
        raise ValueError(f"tsdf_integrate: depth must be [{n}, H, W], got {tuple(depth.shape)}")
    hgt, wid = int(depth.shape[1]), int(depth.shape[2])
    srcs = {}
    for name, t, cols in (("depth", depth, 1), ("accumulation", accumulation, 1), ("rgb", rgb, 3), ("abundances", abundances, C_),
                          ("seg_probs", seg_probs, C_)):
        if t is not None:
            srcs[name] = _tsdf_image(t, n, hgt, wid, cols, name, dev)
    lib = _hip.lib()
    for b in range(0, n, _hip.TSDF_MAX_CAMERAS):
        m = min(_hip.TSDF_MAX_CAMERAS, n - b)
        a = _hip.TsdfImages()
        for name, (img, strides) in srcs.items():
            setattr(a, name, img.data_ptr() + 4 * b * strides[0])
            getattr(a, name + "_strides")[:] = list(strides)
        a.n_cameras, a.height, a.width, a.n_classes = m, hgt, wid, C_
        a.threshold, a.truncation = float(opacity_threshold), float(truncation)
        for j in range(m):
            cam = a.cameras[j]
            cam.rotation[:] = c2w[b + j, :, :3].reshape(-1).tolist()
            cam.origin[:] = c2w[b + j, :, 3].tolist()
            cam.fx, cam.fy, cam.cx, cam.cy = (float(x) for x in intr[b + j])
            if dist is not None and np.any(dist[b + j] != 0):
                cam.distortion[:] = dist[b + j].tolist()
                cam.distorted = 1
        _hip.check(lib.umhs_tsdf_integrate(C.byref(v), C.byref(a), _hip.stream()), "umhs_tsdf_integrate")
    del srcs


def mesh_extract(vol: Dict, world=None, guard_rows: int = 0) -> Dict:
    """Marching tetrahedra over ``vol`` -> {"rows" uint8 [V, row_bytes] (float x y z, uchar red green blue, and with classes int32
    material, float abundances), "faces" int32 [F, 3], "n_classes"}: mark, scan the per-chunk counts (torch), read the two totals
    once (16 bytes) to size the outputs exactly, vertices, triangles.  ``world``: [3,4] host affine for the written xyz.
    ``guard_rows``: that many untouched rows / faces of 0xA5 bytes are kept behind the outputs (tests) and returned as
    ``"rows_buffer"`` / ``"faces_buffer"``."""
    v = _tsdf_volume_c(vol)
    dev = vol["D"].device
    n = vol["dims"][0] * vol["dims"][1] * vol["dims"][2]
    C_ = vol["n_classes"]
    lib = _hip.lib()
    chunks = int(lib.umhs_mesh_chunks(n))
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, chunks, dtype=torch.int32, device=dev)
    _hip.check(lib.umhs_mesh_mark(C.byref(v), ptr(mask), C.c_void_p(counts[0].data_ptr()), C.c_void_p(counts[1].data_ptr()), _hip.stream()),
               "umhs_mesh_mark")
    c64 = counts.to(torch.int64)
    incl = torch.cumsum(c64, 1)
    offsets = (incl - c64).contiguous()
    n_v, n_f = (int(x) for x in incl[:, -1].tolist())  # the one device read
    if n_v >= 1 << 31 or 3 * n_f >= 1 << 33:
        raise RuntimeError(f"mesh_extract: {n_v} vertices / {n_f} faces do not fit int32 indices")
    rb = mesh_row_bytes(C_)
    g = int(guard_rows)
    rows = torch.full(((n_v + g) * rb,), 0xA5, dtype=torch.uint8, device=dev) if g else torch.empty(n_v * rb, dtype=torch.uint8, device=dev)
    faces = (torch.full(((n_f + g) * 3,), -0x5A5A5A5B, dtype=torch.int32, device=dev) if g  # (0xA5A5A5A5 as int32)
             else torch.empty(n_f * 3, dtype=torch.int32, device=dev))
    vbase = torch.empty(n, dtype=torch.int32, device=dev)
    wc = None
    if world is not None:
        Wm = np.asarray(world, dtype=np.float32)
        if Wm.shape != (3, 4):
            raise ValueError("mesh_extract: world = [3,4] affine")
        wc = (_hip._f32 * 12)(*Wm.reshape(-1).tolist())
    _hip.check(lib.umhs_mesh_vertices(C.byref(v), ptr(mask), C.c_void_p(offsets[0].data_ptr()), wc, ptr(vbase),
                                      C.c_void_p(rows.data_ptr()), n_v, _hip.stream()), "umhs_mesh_vertices")
    _hip.check(lib.umhs_mesh_triangles(C.byref(v), ptr(mask), ptr(vbase), C.c_void_p(offsets[1].data_ptr()),
                                       C.c_void_p(faces.data_ptr()), n_f, _hip.stream()), "umhs_mesh_triangles")
    out = {"rows": rows[:n_v * rb].view(n_v, rb), "faces": faces[:n_f * 3].view(n_f, 3), "n_classes": C_}
    if g:
        out["rows_buffer"], out["faces_buffer"] = rows, faces
    return out


def ssim(a, b, data_range=None):
    """torchmetrics structural_similarity_index_measure (gaussian 11x11, sigma 1.5) of channel-last images [H,W,K] -> 0-dim float64."""
    a, b = _hip.f32c(a), _hip.f32c(b)
    assert a.dim() == 3 and a.shape == b.shape
    h, w, k = a.shape
    n = _hip.lib().umhs_ssim_partials(h, w, k)
    if n == 0:
        raise ValueError(f"SSIM needs images of at least 11x11 pixels, got {h}x{w}")
    if data_range is None:
        (alo, ahi), (blo, bhi) = torch.aminmax(a), torch.aminmax(b)
        dr = torch.maximum(ahi - alo, bhi - blo).reshape(1)
    else:
        dr = torch.full((1,), float(data_range), device=a.device)
    part = torch.empty(n, dtype=torch.float64, device=a.device)
    _hip.check(_hip.lib().umhs_ssim(ptr(a), ptr(b), h, w, k, ptr(dr), ptr(part), n, _hip.stream()), "umhs_ssim")
    return part.sum() / float((h - 10) * (w - 10) * k)


def field_backward_into(spec: FieldSpec, flat, pos01, sel, wpos, d, enc, sigma_raw, emb, d_sigma, d_spectral, d_emb,
                        prepared: bool = False, feat_logits=None, hash_ready=None, comp=None):
    """``prepared``: field_bwd_prepare and hashgrid_bwd_prepare (all levels) already ran for this step's parameters/positions;
    ``hash_ready``: event of the stream hashgrid_bwd_prepare was issued on -- waited for only in front of the scatter pass, so the
    histogram may still be running under the field backward.
    Backward of the field (field_bwd + hash-grid scatter) into the flat gradient.  With a gradient sink that owns the next
    backward the buffer becomes ``param.grad`` directly, finished segments start their all-reduce, and None is returned;
    otherwise the freshly written flat gradient is returned (autograd accumulates it)."""
    L = spec.layout
    sink = spec.grad_sink
    own = sink is not None and sink.param is flat and sink.owns_next_backward()
    # the 64 MiB table segment is fully written by hashgrid_bwd(overwrite=True): no memset of the flat gradient
    d_flat = sink.begin() if own else torch.empty_like(flat)
    acc = own and sink.accumulating  # a further micro-step of an accumulation window: everything below ADDS to the buffer
    tail = L.tail_offset()
    if not own:  # field_reduce overwrites every weight / bias / endmember entry; only the alignment padding between the segments is
        d_flat[tail:].zero_()  # never written -- the sink's persistent buffer has it zeroed once, a fresh tensor needs it now
    d_tail = torch.zeros(L.total - tail, device=flat.device, dtype=torch.float32) if acc else None
    d_enc = field_bwd(spec, flat.detach(), enc, True, wpos, d, sel, sigma_raw, emb, d_sigma, d_spectral, d_emb, d_flat,
                      packs_ready=prepared, feat_logits=feat_logits, d_tail=d_tail, comp=comp)
    if acc:
        d_flat[tail:].add_(d_tail)
    if own:
        sink.segment_done(d_flat[tail:])
    table = L.view(d_flat, "mlp_base.encoder.hash_table")
    T = 1 << L.log2_hashmap_size
    if prepared and hash_ready is not None:
        torch.cuda.current_stream(flat.device).wait_event(hash_ready)
    groups = sink.groups(NUM_LEVELS) if own else [(0, NUM_LEVELS)]
    # armed by the trainer (one GPU, optimizer.step() follows): the table's Adam step rides in the reduce pass (UMHSAdam.arm_fused)
    fused = sink.take_fused_adam(flat) if (own and not acc and prepared and len(groups) == 1 and pos01.shape[0] > 0) else None
    ow = not acc  # overwrite mode writes every slot of the levels; accumulation runs the same kernels in their += mode
    for l0, cnt in groups:
        if prepared and fused is not None:
            lv = lambda t: L.view(t, "mlp_base.encoder.hash_table")
            hashgrid_bwd_apply(pos01, d_enc, spec.scalings, L.log2_hashmap_size, table, True, overwrite=True, level_begin=l0, level_count=cnt,
                               adam=dict(fused, table=lv(flat.data), exp_avg=lv(fused["exp_avg"]), exp_avg_sq=lv(fused["exp_avg_sq"])))
            tb = L.offset("mlp_base.encoder.hash_table")
            sink.adam_done = (fused["step"], tb + fused["level_begin"] * T * FEATURES_PER_LEVEL, tb + NUM_LEVELS * T * FEATURES_PER_LEVEL)
        elif prepared:  # histogram + scan of all levels were done ahead of time (hashgrid_bwd_prepare)
            hashgrid_bwd_apply(pos01, d_enc, spec.scalings, L.log2_hashmap_size, table, True, overwrite=ow, level_begin=l0, level_count=cnt)
        else:
            hashgrid_bwd(pos01, d_enc, spec.scalings, L.log2_hashmap_size, table, True, overwrite=ow, level_begin=l0, level_count=cnt)
        if own:
            sink.table_levels_done(table, l0, cnt)
    if own:  # the buffer becomes param.grad directly (autograd gets None: nothing to accumulate or copy)
        sink.commit()
        return None
    return d_flat


def ray_epilogue_fwd(s, m, E, accumulation, depth, tminmax, colors, alpha: float):
    R, B = s.shape
    Cn = E.shape[0]
    new = lambda *shp: torch.empty(shp, device=s.device, dtype=torch.float32)
    rgb, dclip, probs, raw, pred = new(R, 3), new(R, 1), new(R, Cn), new(R), new(R, 3)
    _hip.check(_hip.lib().umhs_ray_epilogue_fwd(ptr(s), ptr(m), ptr(E), ptr(accumulation), ptr(depth), ptr(tminmax), ptr(colors), R, B, Cn,
                                                float(alpha), ptr(rgb), ptr(dclip), ptr(probs), ptr(raw), ptr(pred), _hip.stream()),
               "umhs_ray_epilogue_fwd")
    return rgb, dclip, probs, raw, pred


def ray_rgb_fwd(s, m):
    """The ``rgb`` of ray_epilogue_fwd alone, from the same kernel (no class is compared, nothing else is written): the same bits."""
    rgb = torch.empty((s.shape[0], 3), device=s.device, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_ray_epilogue_fwd(ptr(s), ptr(m), None, None, None, None, None, s.shape[0], s.shape[1], 0, 0.0, ptr(rgb), None,
                                                None, None, None, _hip.stream()), "umhs_ray_epilogue_fwd")
    return rgb


_tail_scratch: Dict[int, torch.Tensor] = {}


def ray_train_tail(s, m, E, accumulation, depth, tminmax, colors, gt_spec, gt_rgb, bg, alpha: float, w_spec: float, w_rgb: float,
                   rgb_loss: bool):
    """Per-ray tail of a training step in one launch: ray_epilogue_fwd + loss_fwd + loss_bwd(unit upstream) + spec2rgb_bwd.
    -> (rgb, depth_clipped, seg_probs, seg_raw, seg_pred, losses[2], d_spectral, d_accumulation | None)"""
    R, B = s.shape
    Cn = E.shape[0]
    dev = s.device
    # ONE allocation for the nine outputs, carved into 16-byte-aligned views (fresh every call: callers keep what they get).  Nine
    # torch.empty calls were ~40 us of host time between a profiler's event pair around this operator -- more than the kernel's 19 us,
    # so whenever the GPU ran dry the "operator time" was the host's (BENCH_r03's kernels_ms row).
    sizes = [R * 3, R, R * Cn, R, R * 3, 2, R * B, R if rgb_loss else 0]
    offs, total = [], 0
    for n_ in sizes:
        offs.append(total)
        total += (n_ + 3) & ~3
    buf = torch.empty(total, device=dev, dtype=torch.float32)
    view = lambda i, *shp: buf[offs[i]:offs[i] + sizes[i]].view(*shp)
    rgb, dclip, probs, raw, pred = view(0, R, 3), view(1, R, 1), view(2, R, Cn), view(3, R), view(4, R, 3)
    losses, d_spec = view(5, 2), view(6, R, B)
    d_acc = view(7, R) if rgb_loss else None
    sc = _tail_scratch.get(dev.index or 0)
    if sc is None:
        sc = _tail_scratch[dev.index or 0] = torch.zeros(_hip.lib().umhs_ray_train_tail_scratch_bytes(), dtype=torch.uint8, device=dev)
    _hip.check(_hip.lib().umhs_ray_train_tail(ptr(s), ptr(m), ptr(E), ptr(accumulation), ptr(depth), ptr(tminmax), ptr(colors), ptr(gt_spec),
                                              ptr(gt_rgb), ptr(bg), R, B, Cn, float(alpha), float(w_spec), float(w_rgb), int(rgb_loss),
                                              ptr(rgb), ptr(dclip), ptr(probs), ptr(raw), ptr(pred), ptr(losses), ptr(d_spec), ptr(d_acc),
                                              ptr(sc), sc.numel(), _hip.stream()), "umhs_ray_train_tail")
    return rgb, dclip, probs, raw, pred, losses, d_spec, d_acc


def loss_fwd(s, g, r, a, bg, gr, w_spec: float, w_rgb: float):
    R, B = s.shape
    losses = torch.empty(2, device=s.device, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_loss_fwd(ptr(s), ptr(g), ptr(r), ptr(a), ptr(bg), ptr(gr), R, B, float(w_spec), float(w_rgb),
                                        ptr(losses), _hip.stream()), "umhs_loss_fwd")
    return losses


def loss_bwd(s, g, r, a, bg, gr, w_spec: float, w_rgb: float, grad_losses):
    R, B = s.shape
    d_spec = torch.empty_like(s)
    d_rgb = torch.empty_like(r) if r is not None else None
    d_acc = torch.empty_like(a) if r is not None else None
    _hip.check(_hip.lib().umhs_loss_bwd(ptr(s), ptr(g), ptr(r), ptr(a), ptr(bg), ptr(gr), R, B, float(w_spec), float(w_rgb), ptr(grad_losses),
                                        ptr(d_spec), ptr(d_rgb), ptr(d_acc), _hip.stream()), "umhs_loss_bwd")
    return d_spec, d_rgb, d_acc


def adam_step_rows(p, g, m, v, rows, step: int, lr: float, betas=(0.9, 0.999), eps=1e-15, grad_scale=1.0):
    """Adam on the 2-float rows ``rows`` (int64, device) of the flat buffers only."""
    _hip.check(_hip.lib().umhs_adam_step_rows(ptr(p), ptr(g), ptr(m), ptr(v), ptr(rows), rows.numel(), lr, betas[0], betas[1], eps, step,
                                              grad_scale, _hip.stream()), "umhs_adam_step_rows")


def adam_step_rows_range(p, g, m, v, rows, begin: int, end: int, step: int, lr: float, betas=(0.9, 0.999), eps=1e-15, grad_scale=1.0,
                         clamp_range=(0, 0)):
    """adam_step_rows(rows) + adam_step on elements [begin, end) of the same flat buffers (clamp_range in absolute elements): one launch."""
    _hip.check(_hip.lib().umhs_adam_step_rows_range(ptr(p), ptr(g), ptr(m), ptr(v), ptr(rows), rows.numel(), begin, end - begin, lr, betas[0],
                                                    betas[1], eps, step, grad_scale, clamp_range[0], clamp_range[1], _hip.stream()),
               "umhs_adam_step_rows_range")


# --------------------------------------------------------------------------------------------- #
# method="rgb": the two MLPs of NerfactoField as HIP kernels (csrc/umhs_rgb.hip)
# --------------------------------------------------------------------------------------------- #
def rgb_base_fwd(enc, sel, w0, b0, w1, b1, want_emb: bool = True, want_raw: bool = False):
    """mlp_base of the rgb field: enc [N,32] (sample-major) -> (density [N] = trunc_exp(out0) * sel, emb [N,15] | None, sigma_raw [N] | None)."""
    n = enc.shape[0]
    new = lambda *shp: torch.empty(shp, device=enc.device, dtype=torch.float32)
    density, emb, raw = new(n), (new(n, 15) if want_emb else None), (new(n) if want_raw else None)
    _hip.check(_hip.lib().umhs_rgb_base_fwd(ptr(enc), ptr(sel), ptr(w0), ptr(b0), ptr(w1), ptr(b1), n, ptr(density), ptr(emb), ptr(raw),
                                            _hip.stream()), "umhs_rgb_base_fwd")
    return density, emb, raw


def rgb_head_fwd(dirs, emb, w0, b0, w1, b1, w2, b2):
    """NerfactoField.mlp_head: [SH16((d + 1) / 2) | emb15] -> 64 -> 64 -> 3, sigmoid -> rgb [N,3]."""
    n = dirs.shape[0]
    rgb = torch.empty((n, 3), device=dirs.device, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_rgb_head_fwd(ptr(dirs), ptr(emb), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(w2), ptr(b2), n, ptr(rgb),
                                            _hip.stream()), "umhs_rgb_head_fwd")
    return rgb


class RgbBaseFn(torch.autograd.Function):
    """(enc [N,32], sel [N], w0, b0, w1, b1) -> (density [N], emb [N,15]); backward recomputes the forward inside the kernel."""

    @staticmethod
    def forward(ctx, enc, sel, w0, b0, w1, b1):
        enc, sel = enc.contiguous(), sel.contiguous()
        w = [t.detach().contiguous() for t in (w0, b0, w1, b1)]
        density, emb, _ = rgb_base_fwd(enc, sel, *w)
        ctx.save_for_backward(enc, sel, *w)
        return density, emb

    @staticmethod
    def backward(ctx, d_density, d_emb):
        enc, sel, w0, b0, w1, b1 = ctx.saved_tensors
        n = enc.shape[0]
        d_enc = torch.empty_like(enc)
        g = [torch.empty_like(t) for t in (w0, b0, w1, b1)]
        if n == 0:
            return (d_enc, None, *[t.zero_() for t in g])
        dd = d_density.contiguous().float() if d_density is not None else None
        de = d_emb.contiguous().float() if d_emb is not None else None
        if dd is None and de is None:
            dd = torch.zeros(n, device=enc.device)
        ws = _scratch(enc.device, "rgb_mlp_bwd", _hip.lib().umhs_rgb_mlp_bwd_workspace_bytes(0, n))
        _hip.check(_hip.lib().umhs_rgb_base_bwd(ptr(enc), ptr(sel), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(dd), ptr(de), n, ptr(d_enc),
                                                ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), 0, ptr(ws), ws.numel(), _hip.stream()),
                   "umhs_rgb_base_bwd")
        return (d_enc, None, *g)


class RgbHeadFn(torch.autograd.Function):
    """(directions [N,3], emb [N,15], w0, b0, w1, b1, w2, b2) -> rgb [N,3]."""

    @staticmethod
    def forward(ctx, dirs, emb, w0, b0, w1, b1, w2, b2):
        dirs, emb = dirs.contiguous(), emb.contiguous()
        w = [t.detach().contiguous() for t in (w0, b0, w1, b1, w2, b2)]
        rgb = rgb_head_fwd(dirs, emb, *w)
        ctx.save_for_backward(dirs, emb, *w)
        return rgb

    @staticmethod
    def backward(ctx, d_rgb):
        dirs, emb, w0, b0, w1, b1, w2, b2 = ctx.saved_tensors
        n = dirs.shape[0]
        d_emb = torch.empty_like(emb)
        g = [torch.empty_like(t) for t in (w0, b0, w1, b1, w2, b2)]
        if n == 0:
            return (None, d_emb, *[t.zero_() for t in g])
        dr = d_rgb.contiguous().float()
        ws = _scratch(dirs.device, "rgb_mlp_bwd", _hip.lib().umhs_rgb_mlp_bwd_workspace_bytes(1, n))
        _hip.check(_hip.lib().umhs_rgb_head_bwd(ptr(dirs), ptr(emb), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(dr), n,
                                                ptr(d_emb), *[ptr(t) for t in g], 0, ptr(ws), ws.numel(), _hip.stream()), "umhs_rgb_head_bwd")
        return (None, d_emb, *g)


# --------------------------------------------------------------------------------------------- #
# autograd glue
# --------------------------------------------------------------------------------------------- #
class FieldFn(torch.autograd.Function):
    """UMHSField.forward (get_density + get_outputs, umhs_field.py:151-329) on packed samples.

    inputs : flat params, origins [N,3], directions [N,3], starts [N,1], ends [N,1]
    outputs: density [N,1], emb [N,15], spectral [N,B], spectral2 | None, specular | None, abundances [N,C]
    """

    @staticmethod
    def forward(ctx, flat, origins, directions, starts, ends, spec: FieldSpec):
        ctx.set_materialize_grads(False)  # unused outputs arrive as None instead of freshly filled zero tensors
        L = spec.layout
        o, d = _hip.f32c(origins), _hip.f32c(directions)
        s, e = _hip.f32c(starts).view(-1), _hip.f32c(ends).view(-1)
        wpos, pos01, sel = positions_fwd(o, d, s, e, spec)
        table = L.view(flat.detach(), "mlp_base.encoder.hash_table")
        enc = hashgrid_fwd(pos01, table, spec.scalings, L.log2_hashmap_size, True)
        out = field_fwd(spec, flat.detach(), enc, True, wpos, d, sel, want_emb=True, want_logits=flat.requires_grad)
        ctx.spec = spec
        ctx.has_logits = out["feat_logits"] is not None
        ctx.save_for_backward(flat, pos01, sel, wpos, d, enc, out["sigma_raw"], out["emb"], *([out["feat_logits"]] if ctx.has_logits else []))
        n = o.shape[0]
        res = [out["sigma"].view(n, 1), out["emb"], out["spectral"], out["spectral2"], out["specular"], out["abundances"]]
        ctx.mark_non_differentiable(*[t for t in res[3:] if t is not None])
        return tuple(res)

    @staticmethod
    def backward(ctx, d_sigma, d_emb, d_spectral, *_):
        flat, pos01, sel, wpos, d, enc, sigma_raw, emb, *rest = ctx.saved_tensors
        logits = rest[0] if ctx.has_logits else None
        spec: FieldSpec = ctx.spec
        L = spec.layout
        n = sel.shape[0]
        zeros = lambda *s: torch.zeros(s, device=sel.device, dtype=torch.float32)
        d_sigma = _hip.f32c(d_sigma).view(-1) if d_sigma is not None else zeros(n)
        d_spectral = _hip.f32c(d_spectral) if d_spectral is not None else zeros(n, L.wavelengths)
        d_emb = _hip.f32c(d_emb) if d_emb is not None else None
        d_flat = field_backward_into(spec, flat, pos01, sel, wpos, d, enc, sigma_raw, emb, d_sigma, d_spectral, d_emb, feat_logits=logits)
        return d_flat, None, None, None, None, None


class DensityFn(torch.autograd.Function):
    """density_fn / get_density forward only (no-grad users: occupancy grid, sampler; umhs_model.py:208,553).
    ``keep``: a dict that receives the level-major hash features of the queried positions (``keep["enc"]``)."""

    @staticmethod
    def forward(ctx, flat, positions, spec: FieldSpec, keep=None, want_emb=True):
        L = spec.layout
        p = _hip.f32c(positions).view(-1, 3)
        _, pos01, sel = positions_fwd(None, None, None, None, spec, world_pos_in=p)
        out = field_density(spec, flat.detach(), pos01, sel, want_emb, keep)
        if out["emb"] is None:  # density_fn callers (sampler, occupancy grid) only want sigma: 60 B per sample not written
            out["emb"] = out["sigma"].new_empty(0)
        ctx.mark_non_differentiable(out["sigma"], out["emb"])
        return out["sigma"].view(-1, 1), out["emb"]

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("density_fn is a no-grad path (umhs_model.py:229-237); use UMHSField.forward for gradients")


class CompositeFn(torch.autograd.Function):
    """nerfacc.render_weight_from_density + accumulate_along_rays for every composited stream at once
    (umhs_model.py:245-304 -> umhs_renderer.py:28-30).  values: tuple of [N,k] tensors; returns
    (weights [N,1], accumulation [R,1], depth_unclipped [R,1], *composited [R,k])."""

    @staticmethod
    def forward(ctx, sigma, starts, ends, packed_info, grad_scaling: bool, *values):
        ctx.set_materialize_grads(False)
        s = _hip.f32c(sigma).view(-1)
        t0, t1 = _hip.f32c(starts).view(-1), _hip.f32c(ends).view(-1)
        vals = [_hip.f32c(v).view(v.shape[-2], v.shape[-1]) for v in values]
        weights, acc, depth, outs = composite_fwd(s, t0, t1, packed_info, vals)
        ctx.save_for_backward(s, t0, t1, packed_info, weights, *vals)
        ctx.grad_scaling = grad_scaling
        ctx.needs = [v.requires_grad for v in values]
        ctx.vshapes = [v.shape for v in values]
        ctx.mark_non_differentiable(weights, depth)
        return (weights.view(-1, 1), acc.view(-1, 1), depth.view(-1, 1), *outs)

    @staticmethod
    def backward(ctx, _dw, d_acc, _dd, *d_outs):
        s, t0, t1, pinfo, weights, *vals = ctx.saved_tensors
        d_outs = [(_hip.f32c(g) if g is not None else None) for g in d_outs]
        d_acc = _hip.f32c(d_acc).view(-1) if d_acc is not None else None
        d_sigma, d_values = composite_bwd(s, t0, t1, pinfo, weights, vals, d_outs, ctx.needs, d_acc, ctx.grad_scaling)
        d_values = [(g.view(shp) if g is not None else None) for g, shp in zip(d_values, ctx.vshapes)]
        return (d_sigma.view(-1, 1), None, None, None, None, *d_values)


class Spec2RgbFn(torch.autograd.Function):
    """ColourSystem.forward (utils/spec_to_rgb.py:112-127)."""

    @staticmethod
    def forward(ctx, spec_t, M):
        s, m = _hip.f32c(spec_t), _hip.f32c(M)
        ctx.save_for_backward(s, m)
        return spec2rgb_fwd(s, m)

    @staticmethod
    def backward(ctx, d_rgb):
        s, m = ctx.saved_tensors
        return spec2rgb_bwd(s, m, _hip.f32c(d_rgb)), None


def accumulate_fwd(weights, values, packed_info):
    """out[r] = sum over the samples n of ray r of weights[n] * values[n] (no autograd)."""
    R = packed_info.shape[0]
    out = torch.empty((R, values.shape[1]), device=values.device, dtype=torch.float32)
    st = _hip.ValueStreams()
    st.n_streams, st.k[0], st.values[0], st.out[0] = 1, values.shape[1], values.data_ptr(), out.data_ptr()
    _hip.check(_hip.lib().umhs_accumulate_fwd(ptr(weights), ptr(packed_info), R, weights.shape[0], C.byref(st), _hip.stream()),
               "umhs_accumulate_fwd")
    return out


class AccumulateFn(torch.autograd.Function):
    """nerfacc.accumulate_along_rays with caller-provided weights (SpectralRenderer.forward stand-alone,
    umhs_renderer.py:28-30): out[r] = sum_n w[n] v[n].  Differentiable in both weights and values."""

    @staticmethod
    def forward(ctx, weights, values, packed_info):
        w, v = _hip.f32c(weights).view(-1), _hip.f32c(values)
        v = v.view(v.shape[-2], v.shape[-1])
        out = accumulate_fwd(w, v, packed_info)
        ctx.save_for_backward(w, v, packed_info)
        ctx.shapes = (weights.shape, values.shape)
        return out

    @staticmethod
    def backward(ctx, d_out):
        w, v, pinfo = ctx.saved_tensors
        d_out = _hip.f32c(d_out)
        d_w, d_v = torch.zeros_like(w), torch.empty_like(v)
        g = _hip.ValueGrads()
        g.n_streams, g.k[0], g.values[0], g.d_out[0], g.d_values[0] = 1, v.shape[1], v.data_ptr(), d_out.data_ptr(), d_v.data_ptr()
        _hip.check(_hip.lib().umhs_accumulate_bwd(ptr(w), ptr(pinfo), pinfo.shape[0], w.shape[0], C.byref(g), ptr(d_w),
                                                  _hip.stream()), "umhs_accumulate_bwd")
        return d_w.view(ctx.shapes[0]), d_v.view(ctx.shapes[1]), None


def tmid_minmax(starts, ends, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Encoded (min, max) of the sample mid-points over the batch; consumed by RayEpilogueFn only."""
    t0, t1 = _hip.f32c(starts).view(-1), _hip.f32c(ends).view(-1)
    mm = out if out is not None else torch.empty(2, device=t0.device, dtype=torch.float32)
    _hip.check(_hip.lib().umhs_tmid_minmax(ptr(t0), ptr(t1), t0.shape[0], ptr(mm), _hip.stream()), "umhs_tmid_minmax")
    return mm


class RayEpilogueFn(torch.autograd.Function):
    """One launch for the per-ray tail of UMHSModel.get_outputs (umhs_model.py:254-313): ColourSystem, depth clip,
    ClusterLookup(alpha) + argmax + class colours.  Returns (rgb, depth, seg_probs, seg_raw, seg_pred); gradient flows
    through rgb only (no loss of the reference uses the segmentation outputs)."""

    @staticmethod
    def forward(ctx, spectral, M, endmembers, accumulation, depth, tminmax, colors, alpha: float):
        ctx.set_materialize_grads(False)
        s, m = _hip.f32c(spectral), _hip.f32c(M)
        E = _hip.f32c(endmembers)
        rgb, dclip, probs, raw, pred = ray_epilogue_fwd(s, m, E, _hip.f32c(accumulation).view(-1), _hip.f32c(depth).view(-1), tminmax,
                                                        _hip.f32c(colors), alpha)
        ctx.save_for_backward(s, m)
        ctx.mark_non_differentiable(dclip, probs, raw, pred)
        return rgb, dclip, probs, raw, pred

    @staticmethod
    def backward(ctx, d_rgb, *_):
        s, m = ctx.saved_tensors
        d_spec = spec2rgb_bwd(s, m, _hip.f32c(d_rgb)) if d_rgb is not None else None
        return d_spec, None, None, None, None, None, None, None


class LossFn(torch.autograd.Function):
    """(w_spec * MSE(spectral, gt), w_rgb * MSE(rgb + bg*(1-acc), gt_rgb)) in one launch; backward in one launch
    (umhs_model.py:358-370).  rgb/acc/bg/gt_rgb may be None (method == "spectral")."""

    @staticmethod
    def forward(ctx, spectral, gt_spectral, rgb, accumulation, background, gt_rgb, w_spec: float, w_rgb: float):
        ctx.set_materialize_grads(False)
        c = lambda t: _hip.f32c(t) if t is not None else None
        s, g, r, bg, gr = c(spectral), c(gt_spectral), c(rgb), c(background), c(gt_rgb)
        a = c(accumulation).view(-1) if accumulation is not None else None
        losses = loss_fwd(s, g, r, a, bg, gr, w_spec, w_rgb)
        ctx.save_for_backward(*[t for t in (s, g, r, a, bg, gr) if t is not None])
        ctx.has = [t is not None for t in (s, g, r, a, bg, gr)]
        ctx.w = (float(w_spec), float(w_rgb))
        ctx.acc_shape = accumulation.shape if accumulation is not None else None
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_spec, g_rgb):
        it = iter(ctx.saved_tensors)
        s, g, r, a, bg, gr = [(next(it) if h else None) for h in ctx.has]
        R, B = s.shape
        zero = lambda: torch.zeros((), device=s.device, dtype=torch.float32)
        gl = torch.stack([g_spec if g_spec is not None else zero(), g_rgb if g_rgb is not None else zero()]).to(torch.float32)
        d_spec, d_rgb, d_acc = loss_bwd(s, g, r, a, bg, gr, ctx.w[0], ctx.w[1], gl)
        return d_spec, None, d_rgb, (d_acc.view(ctx.acc_shape) if d_acc is not None else None), None, None, None, None
