#!/usr/bin/env python3
"""Generate the VCA fixtures g6_vca_*.npz from the REFERENCE's own code.

Run in the build container only (needs /root/reference, which never travels; numpy + scipy are all its vca.py imports):

    python tests/golden/make_golden_vca.py

G6 pins ``umhsnerf.data.utils.vca.vca`` -- imported natively, called as its only caller does (hs_dataloader.py:54: the frame as
[B, H*W], ``verbose`` left False) -- on the synthetic cubes of tests/vca_f64.py.  Each cube is run twice: as float32, what the
caller passes, and cast to float64.  ``d_ref = max|Ae_f32 - Ae_f64|`` is the reference's own fp32 distance from float64: the
yardstick of the GPU tests.  The random stream: ``np.random.seed(1234)`` in front of each call; the same R calls of
``np.random.rand(R, 1)`` are replayed afterwards and stored as ``draws`` (column i = w_i).  Where the reference raises (the cube
below the SNR threshold: its projection to R-1 dimensions sits under ``if verbose:``), the exception's name is what is recorded.
Fixtures are data only."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from vca_f64 import draws_from_seed, make_cube  # noqa: E402

# name, shape, bands, classes, noise SNR [dB], cube seed
CUBES = [("b31", (32, 32), 31, 6, 45.0, 1), ("b128", (24, 24), 128, 9, 45.0, 2), ("b141", (24, 24), 141, 4, 45.0, 3),
         ("b31_low", (32, 32), 31, 6, 15.0, 4)]
DRAW_SEED = 1234


def _reference_vca():
    spec = importlib.util.spec_from_file_location("reference_vca", "/root/reference/umhsnerf/data/utils/vca.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.vca


def _run(vca, Y, R):
    np.random.seed(DRAW_SEED)
    with contextlib.redirect_stdout(io.StringIO()):  # (the file prints its loop counter)
        try:
            Ae, indice, _ = vca(Y, R)
        except Exception as e:  # noqa: BLE001 -- the caller swallows every exception too (hs_dataloader.py:57-58)
            return None, None, type(e).__name__
    return np.asarray(Ae), np.asarray(indice, np.int64), ""


def main():
    vca = _reference_vca()
    for name, shape, B, R, snr_db, seed in CUBES:
        cube = make_cube(shape, B, R, snr_db, seed)
        Y = cube.reshape(-1, B).T  # hs_dataloader.py:54
        assert Y.dtype == np.float32
        Ae32, ind32, err32 = _run(vca, Y, R)
        Ae64, ind64, err64 = _run(vca, Y.astype(np.float64), R)
        out = dict(cube=cube, num_classes=np.int64(R), draws=draws_from_seed(R, DRAW_SEED), noise_snr_db=np.float64(snr_db),
                   raised_f32=np.str_(err32), raised_f64=np.str_(err64))
        if not err32 and not err64:
            out.update(Ae_f32=Ae32.astype(np.float64), indice_f32=ind32, Ae_f64=Ae64, indice_f64=ind64,
                       d_ref=np.float64(np.max(np.abs(Ae32.astype(np.float64) - Ae64))))
        path = os.path.join(HERE, f"g6_vca_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, "raised", err32 or "-", err64 or "-", "d_ref", out.get("d_ref"), "indices", ind32, ind64,
              f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
