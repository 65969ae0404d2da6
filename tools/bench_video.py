"""The device JPEG encoder and the video render loop (not bench.py: that measures the training step).  GPU box.

Model and camera path: tools/bench_render.py's (C2-shaped, 300 training steps, 8 cameras on a circle), at 1280 x 720, one panel
(``rgb``) and seven (``rgb + abundances_0..5``).  The frames encoded are the composed frames of the last camera.

Per panel set, quality (90, 100) and subsampling (4:2:0, 4:4:4) -- device events around REPS calls, warm, the median of ROUNDS rounds in
which the variants alternate:
  transform_ms  ops.jpeg_coefficients (stage A)           entropy_ms  ops.jpeg_entropy on its result (stage B: three launches)
  encode_ms     ops.jpeg_encode, both, into given buffers  jpeg_bytes  the length of the file
  memcpy_ms     a device copy of the raw frame: what moving the frame once costs
  pil_jpeg_ms / pil_png_ms   PIL's encoders on ONE host thread, to memory, host clock (png once per panel set)
``restart_sweep``: entropy_ms over R = 4 .. 128 MCUs per restart interval (seven panels): ops.JPEG_DEFAULT_RESTART_MCUS comes from it.
``loops``: render_camera_path end to end, all 8 frames, files written: PNG images as the loop always ran (4 encoder threads), JPEG
images by PIL, JPEG images by the device encoder, and ``video`` (quality 100, 4:2:0, the defaults of the command line).
Prints one JSON line and writes it to --out.  ``--encode-only`` runs just the encoder (REPS calls per panel set, quality and
subsampling) and prints nothing measured: it is the command to put under ``rocprofv3 --kernel-trace --stats`` for the kernels' own
times (the event timings above include the host's issue time of four launches)."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tools")]
import torch

import bench
import bench_render
from umhsnerf import ops, render

DEV = torch.device("cuda", 0)
REPS, ROUNDS, FRAMES = 5, 7, bench_render.FRAMES
PANEL_SETS = {"rgb": ["rgb"], "rgb+abundances": bench_render.PANEL_SETS["rgb+abundances"]}
SWEEP = (4, 8, 16, 32, 64, 128)


def events_ms(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternated(variants, rounds=ROUNDS):
    """{name: fn} -> {name: median ms}: every fn warmed, then ``rounds`` rounds in which the variants take turns."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(events_ms(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def pil_bytes(array, fmt, **kw):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(array).save(b, fmt, **kw)
    return len(b.getvalue())


def encoder_variants(frame, quality, ss, R):
    H, W = frame.shape[:2]
    coefs = ops.jpeg_coefficients(frame, quality, ss)
    out = torch.empty(ops.jpeg_max_bytes(H, W, ss, R), dtype=torch.uint8, device=DEV)
    length = torch.empty(1, dtype=torch.int64, device=DEV)
    ws = torch.empty(ops.jpeg_workspace_bytes(H, W, ss, R), dtype=torch.uint8, device=DEV)
    return {"transform_ms": lambda: ops.jpeg_coefficients(frame, quality, ss),
            "entropy_ms": lambda: ops.jpeg_entropy(coefs, H, W, quality, ss, R, out=out, length=length),
            "encode_ms": lambda: ops.jpeg_encode(frame, quality, ss, R, out=out, length=length, workspace=ws)}, length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--encode-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    pipe.eval()
    W, H = (int(v) for v in args.size.split("x"))
    cameras, _ = render.load_camera_path(bench_render.camera_path(H, W), device=DEV)
    R0 = ops.JPEG_DEFAULT_RESTART_MCUS
    rows, sweep, loops = [], [], []
    for set_name, names in PANEL_SETS.items():
        with torch.no_grad():
            outputs = pipe.model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(FRAMES - 1), output_names=render.source_keys(names))
            frame = render.compose_frame(outputs, names)
        if args.encode_only:
            for quality in (90, 100):
                for ss in ("420", "444"):
                    encode = encoder_variants(frame, quality, ss, R0)[0]["encode_ms"]
                    for _ in range(REPS):
                        encode()
            torch.cuda.synchronize()
            continue
        other = torch.empty_like(frame)
        host = frame.cpu().numpy()
        png_ms, png_bytes = host_ms(lambda: pil_bytes(host, "PNG"))
        for quality in (90, 100):
            for ss in ("420", "444"):
                variants, length = encoder_variants(frame, quality, ss, R0)
                variants["memcpy_ms"] = lambda: other.copy_(frame)
                row = alternated(variants)
                pil_ms, pil_n = host_ms(lambda: pil_bytes(host, "JPEG", quality=quality, subsampling=0 if ss == "444" else 2))
                row.update(panels=set_name, n_panels=len(names), size=f"{W}x{H}", quality=quality, subsampling=ss, restart_mcus=R0,
                           frame_bytes=frame.numel(), jpeg_bytes=int(length.item()), pil_jpeg_ms=pil_ms, pil_jpeg_bytes=pil_n,
                           pil_png_ms=png_ms, png_bytes=png_bytes)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        if len(names) > 1:
            for quality, ss in ((90, "420"), (100, "444")):
                variants, lengths = {}, {}
                for R in SWEEP:
                    v, lengths[R] = encoder_variants(frame, quality, ss, R)
                    variants[R] = v["entropy_ms"]
                ms = alternated(variants)
                sweep.append({"panels": set_name, "quality": quality, "subsampling": ss,
                              "entropy_ms": {str(R): ms[R] for R in SWEEP}, "jpeg_bytes": {str(R): int(lengths[R].item()) for R in SWEEP}})
                print(json.dumps(sweep[-1]), file=sys.stderr, flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            loop = {"panels": set_name, "n_panels": len(names), "size": f"{W}x{H}", "frames": FRAMES}
            run = lambda sub, **kw: render.render_camera_path(pipe, cameras, os.path.join(tmp, sub), names, **kw)["fps"]
            run("warm.avi", output_format="video")  # (first use of the pinned buffers and of every kernel at this shape)
            loop["fps_png"] = run("png")
            loop["fps_jpeg_host"] = run("jpg_host", image_format="jpeg")
            loop["fps_jpeg_gpu"] = run("jpg_gpu", image_format="jpeg", jpeg_encoder="gpu")
            loop["fps_video"] = run("fly.avi", output_format="video")
            loop["fps_video_q90"] = run("fly90.avi", output_format="video", jpeg_quality=90)
            loop["video_bytes"] = os.path.getsize(os.path.join(tmp, "fly.avi"))
            with torch.no_grad():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(FRAMES):
                    pipe.model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(i, keep_shape=True), output_names=render.source_keys(names))
                torch.cuda.synchronize()
                loop["fps_render_alone"] = FRAMES / (time.perf_counter() - t0)
            loops.append(loop)
            print(json.dumps(loop), file=sys.stderr, flush=True)
    if args.encode_only:
        return
    result = {"bench": "video", "device": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS, "rows": rows, "restart_sweep": sweep,
              "loops": loops}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
