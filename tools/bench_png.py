"""The device PNG encoder, the image render loop and the textured-mesh export with it (not bench.py: that measures the training step).
GPU box.  Records, not gates.

Model and camera path: tools/bench_render.py's (C2-shaped, 300 training steps, 8 cameras on a circle), at 1280 x 720: seven panels
(``rgb + abundances_0..5``), one (``rgb``) and a label frame (``seg_pred``).  The frames encoded are the composed frames of the last
camera.

Per frame -- device events around REPS calls, warm, the median of ROUNDS rounds in which the variants alternate:
  filter_ms    ops.png_filter (stage A, one launch)        deflate_ms  ops.png_deflate on its result (statistics, scan, write, CRC)
  encode_ms    ops.png_encode, all five launches, into given buffers        png_bytes  the length of the file
  memcpy_ms    a device copy of the raw frame: what moving the frame once costs
  jpeg_ms      ops.jpeg_encode (quality 100, 4:2:0) of the same frame
  pil_png_ms / pil_png_bytes   PIL's PNG encoder on ONE host thread, to memory, host clock
``stripe_sweep``: encode_ms and png_bytes over pieces of about 1 .. 128 KiB of filtered bytes: ops.PNG_PIECE_TARGET_BYTES comes from it.
``loops``: render_camera_path end to end, all 8 frames, files written, with ``png_encoder`` host (4 encoder threads) and gpu, against
rendering alone.  ``export``: export_textured_mesh at resolution 128 with both encoders, total and its write stage, and the atlas files'
sizes.  Prints one JSON line and writes it to --out.  ``--encode-only`` runs just the encoder (REPS calls per frame) and prints nothing
measured: it is the command to put under ``rocprofv3 --kernel-trace --stats`` for the five kernels' own times."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd"), os.path.join(ROOT, "tools")]
import torch

import bench
import bench_render
from bench_video import alternated, host_ms, pil_bytes
from umhsnerf import ops, render

DEV = torch.device("cuda", 0)
REPS, ROUNDS, FRAMES = 5, 7, bench_render.FRAMES
PANEL_SETS = {"rgb+abundances": bench_render.PANEL_SETS["rgb+abundances"], "rgb": ["rgb"], "seg_pred": ["seg_pred"]}
SWEEP_BYTES = tuple(k << 10 for k in (1, 2, 4, 8, 16, 32, 64, 128))


def encoder_variants(frame, rows):
    H, W, ch = frame.shape
    filtered = ops.png_filter(frame)
    out = torch.empty(ops.png_max_bytes(H, W, ch, rows), dtype=torch.uint8, device=DEV)
    length = torch.empty(1, dtype=torch.int64, device=DEV)
    ws = torch.empty(ops.png_workspace_bytes(H, W, ch, rows), dtype=torch.uint8, device=DEV)
    return {"filter_ms": lambda: ops.png_filter(frame),
            "deflate_ms": lambda: ops.png_deflate(filtered, W, ch, rows, out=out, length=length, workspace=ws),
            "encode_ms": lambda: ops.png_encode(frame, "adaptive", rows, out=out, length=length, workspace=ws)}, length


def export_part(rounds=3, resolution=128):
    from bench_texture import SIDE
    from umhsnerf import export
    from umhsnerf.data.umhs_datamanager import ResidentSplit
    from umhsnerf.data.umhs_dataparser import Cameras

    pipe, c2w = bench.sampler_scene(bench.C2, DEV)
    n, f = c2w.shape[0], 30.0 * SIDE / 64.0
    cams = Cameras(c2w.clone(), torch.full((n,), f), torch.full((n,), f), torch.full((n,), SIDE / 2), torch.full((n,), SIDE / 2), SIDE, SIDE)
    pipe.datamanager.train_split = ResidentSplit(cams, torch.zeros(n, SIDE, SIDE, 3, dtype=torch.uint8), None, DEV)
    res = {"resolution": resolution, "texture_output_names": ["rgb", "seg_pred"]}
    with tempfile.TemporaryDirectory() as tmp:
        run = lambda enc, **kw: export.export_textured_mesh(pipe, os.path.join(tmp, enc), resolution=resolution, px_per_uv_triangle=4,
                                                            texture_output_names=("rgb", "seg_pred"), png_encoder=enc, **kw)
        total, write = {"host": [], "gpu": []}, {"host": [], "gpu": []}
        for enc in total:
            run(enc)  # warm up
        for _ in range(rounds):
            for enc in total:
                timings = {}
                ms, info = host_ms(lambda: run(enc, timings=timings))
                total[enc].append(ms), write[enc].append(timings["write"] * 1e3)
                res.setdefault("export", {k: info[k] for k in ("vertices", "faces", "atlas_side")})
                res.setdefault("file_bytes", {})[enc] = {os.path.basename(q): os.path.getsize(q) for q in info["textures"].values()}
        res["total_ms"] = {enc: statistics.median(v) for enc, v in total.items()}
        res["write_ms"] = {enc: statistics.median(v) for enc, v in write.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--encode-only", action="store_true")
    ap.add_argument("--skip-export", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured without one"
    pipe, _ = bench.sampler_scene(bench.C2, DEV)
    pipe.eval()
    W, H = (int(v) for v in args.size.split("x"))
    cameras, _ = render.load_camera_path(bench_render.camera_path(H, W), device=DEV)
    rows, sweep, loops = [], [], []
    for set_name, names in PANEL_SETS.items():
        with torch.no_grad():
            outputs = pipe.model.get_outputs_for_camera_ray_bundle(cameras.generate_rays(FRAMES - 1), output_names=render.source_keys(names))
            frame = render.compose_frame(outputs, names)
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        R0 = ops.png_default_stripe_rows(fw, 3)
        if args.encode_only:
            encode = encoder_variants(frame, R0)[0]["encode_ms"]
            for _ in range(REPS):
                encode()
            torch.cuda.synchronize()
            continue
        other = torch.empty_like(frame)
        host = frame.cpu().numpy()
        variants, length = encoder_variants(frame, R0)
        variants["memcpy_ms"] = lambda: other.copy_(frame)
        jpeg_out = torch.empty(ops.jpeg_max_bytes(fh, fw, "420"), dtype=torch.uint8, device=DEV)
        jpeg_len = torch.empty(1, dtype=torch.int64, device=DEV)
        jpeg_ws = torch.empty(ops.jpeg_workspace_bytes(fh, fw, "420"), dtype=torch.uint8, device=DEV)
        variants["jpeg_ms"] = lambda: ops.jpeg_encode(frame, 100, "420", out=jpeg_out, length=jpeg_len, workspace=jpeg_ws)
        row = alternated(variants)
        n = int(length.item())
        data = variants["encode_ms"]()[0][:n].cpu().numpy().tobytes()
        from PIL import Image

        decoded = Image.open(io.BytesIO(data))
        assert np.array_equal(np.asarray(decoded), host), "the file does not decode to the frame"
        pil_ms, pil_n = host_ms(lambda: pil_bytes(host, "PNG"))
        row.update(panels=set_name, n_panels=len(names), size=f"{W}x{H}", stripe_rows=R0, pieces=-(-fh // R0), frame_bytes=frame.numel(),
                   png_bytes=n, jpeg_bytes=int(jpeg_len.item()), pil_png_ms=pil_ms, pil_png_bytes=pil_n)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        if set_name != "seg_pred":
            row_bytes = 1 + 3 * fw
            targets = {t: max(1, -(-t // row_bytes)) for t in SWEEP_BYTES}
            variants, lengths = {}, {}
            for t, r in targets.items():
                v, lengths[t] = encoder_variants(frame, r)
                variants[t] = v["encode_ms"]
            ms = alternated(variants)
            sweep.append({"panels": set_name, "row_bytes": row_bytes, "stripe_rows": {str(t): r for t, r in targets.items()},
                          "encode_ms": {str(t): ms[t] for t in targets}, "png_bytes": {str(t): int(lengths[t].item()) for t in targets}})
            print(json.dumps(sweep[-1]), file=sys.stderr, flush=True)
            with tempfile.TemporaryDirectory() as tmp:
                loop = {"panels": set_name, "n_panels": len(names), "size": f"{W}x{H}", "frames": FRAMES}
                run = lambda sub, **kw: render.render_camera_path(pipe, cameras, os.path.join(tmp, sub), names, **kw)["fps"]
                run("warm", png_encoder="gpu")  # (first use of the pinned buffers and of every kernel at this shape)
                loop["fps_png_host"] = run("png_host")
                loop["fps_png_gpu"] = run("png_gpu", png_encoder="gpu")
                loop["png_host_bytes"] = sum(os.path.getsize(os.path.join(tmp, "png_host", f)) for f in os.listdir(os.path.join(tmp, "png_host")))
                loop["png_gpu_bytes"] = sum(os.path.getsize(os.path.join(tmp, "png_gpu", f)) for f in os.listdir(os.path.join(tmp, "png_gpu")))
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
    result = {"bench": "png", "device": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS, "rows": rows, "stripe_sweep": sweep,
              "loops": loops}
    if not args.skip_export:
        del pipe
        result["export"] = export_part()
        print(json.dumps(result["export"]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
