#!/usr/bin/env python3
"""Time the VCA initialiser's passes (csrc/umhs_vca.hip) on one [512,512,141] frame and on a [32,512,512,141] stack, with the
fraction of the two bounds of umhs_vca_moments: the fp32 matrix pipe (2 N B^2 useful FLOP against 157.3 TFLOP/s) and HBM
(4 N B bytes against 6.3 TB/s).  Prints one JSON line per case; DESIGN section 7 quotes it.

    python tools/bench_vca.py [--frames 32] [--side 512] [--bands 141] [--classes 4] [--reps 7]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"))

PEAK_FP32_MFMA, PEAK_HBM = 157.3e12, 6.3e12


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--bands", type=int, default=141)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from umhsnerf import ops
    from umhsnerf.data.utils.vca import vca_endmembers

    dev, B = "cuda:0", a.bands
    stack = torch.rand(a.frames, a.side, a.side, B, device=dev)
    for label, rows in (("frame", stack[0].view(-1, B)), ("stack", stack.view(-1, B))):
        n = rows.shape[0]
        t = _time(lambda: ops.vca_moments(rows), a.reps)
        s, S = ops.vca_moments(rows)
        basis = torch.zeros(B, 16, device=dev)
        basis[:, : a.classes] = torch.linalg.svd((S / n).float())[0][:, : a.classes]
        basis[:, 15] = 1.0 / B
        tp = _time(lambda: ops.vca_project(rows, basis, a.classes), a.reps)
        y, _ = ops.vca_project(rows, basis, a.classes)
        f = [1.0] * a.classes + [0.0] * (16 - a.classes)
        ta = _time(lambda: ops.vca_argmax(y, f), a.reps)
        print(json.dumps({
            "case": label, "rows": n, "bands": B, "rows_per_partial": ops.vca_rows_per_partial(),
            "moments_ms": round(t * 1e3, 3), "moments_tflops": round(2 * n * B * B / t / 1e12, 2),
            "moments_frac_fp32_mfma": round(2 * n * B * B / t / PEAK_FP32_MFMA, 3),
            "moments_frac_hbm": round(4 * n * B / t / PEAK_HBM, 3),
            "project_ms": round(tp * 1e3, 3), "project_frac_hbm": round((4 * n * B + 64 * n) / tp / PEAK_HBM, 3),
            "argmax_ms": round(ta * 1e3, 3), "argmax_frac_hbm": round(64 * n / ta / PEAK_HBM, 3)}), flush=True)
    import time

    for label, data in (("frame", stack[0]), ("stack", stack)):
        vca_endmembers(data, a.classes, seed=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, info = vca_endmembers(data, a.classes, seed=0)
        torch.cuda.synchronize()
        print(json.dumps({"case": f"vca_endmembers({label})", "wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                          "branch": info["branch"]}), flush=True)


if __name__ == "__main__":
    main()
