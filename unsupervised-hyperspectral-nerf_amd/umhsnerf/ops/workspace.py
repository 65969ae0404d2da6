"""The one place the operators take device scratch memory from: grow-only ``uint8`` buffers cached per (device, name).

A ``*_prepare`` call that parks data in a buffer for a consumer launched later takes a lease on it (``_lease`` / ``_release``); a
buffer under lease is never re-grown or rebuilt.  A name nobody leases is plain per-call scratch: its contents are dead after the call.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

_ws_cache: Dict[Tuple[int, str], torch.Tensor] = {}
_ws_leases: Dict[Tuple[int, str], str] = {}  # (device, slot) -> the *_prepare call whose consumer has not been launched yet

# the three slots of a training step that are leased (reserve_step_workspaces sizes them), and the training tail's counter block
WS_FIELD_BWD, WS_HASH_BWD, WS_FIELD_FWD, WS_TAIL = "field_bwd", "hash_bwd", "field_fwd", "ray_train_tail"


def _workspace(nbytes: int, device, slot: str, floor: int = 1 << 20, zero: bool = False) -> torch.Tensor:
    """Cached per-(device, slot) scratch of at least ``nbytes``; a new buffer has max(nbytes, floor) bytes, zeroed if ``zero``.  A slot
    is never re-grown while a ``*_prepare`` call has parked data in it for a consumer that has not been launched yet (``_lease`` /
    ``_release``): the consumer would be handed a fresh, unfilled buffer."""
    key = (device.index or 0, slot)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if key in _ws_leases:
            raise RuntimeError(f"workspace slot {slot} would be re-grown ({0 if ws is None else ws.numel()} -> {nbytes} bytes) while "
                               f"{_ws_leases[key]} holds data in it for a consumer that has not run; size it first "
                               "(ops.reserve_step_workspaces)")
        ws = _ws_cache[key] = (torch.zeros if zero else torch.empty)(max(nbytes, floor), device=device, dtype=torch.uint8)
    return ws


def _lease(device, slot: str, who: str) -> None:
    _ws_leases[(device.index or 0, slot)] = who


def _release(device, slot: str) -> None:
    _ws_leases.pop((device.index or 0, slot), None)


def _require_free(device, slot: str, who: str) -> None:
    """A call that rebuilds a slot's contents must not run between a ``*_prepare`` and its consumer."""
    held = _ws_leases.get((device.index or 0, slot))
    if held is not None:
        raise RuntimeError(f"{who} would overwrite workspace slot {slot} while {held} holds data in it for a consumer that has not run")
