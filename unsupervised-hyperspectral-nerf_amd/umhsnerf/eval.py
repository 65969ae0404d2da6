"""``python -m umhsnerf.eval --data DIR --checkpoint FILE [--output-path DIR]`` (or ``--load-config RUN/config.json``): what ``ns-eval --load-config ...`` does for a trained
model (scripts/visualize/hotdog.sh), without nerfstudio -- build the pipeline on the scene, ``load_pipeline`` the checkpoint, run
``get_average_eval_image_metrics(output_path=..., get_std=True)`` over the whole eval split and print the result as one JSON line.

The checkpoint is what nerfstudio's Trainer writes (``{"step": ..., "pipeline": state_dict, ...}``) or a bare pipeline state dict.  The
model options must be those the model was trained with: flags, or ``--load-config RUN/config.json`` -- the file ``python -m
umhsnerf.train`` leaves in its run directory -- which supplies ``--data``, the model flags and the latest checkpoint under
``RUN/nerfstudio_models/`` as ``ns-eval --load-config`` does; explicit flags override the file."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch


def build_pipeline(args, device):
    from .data.umhs_datamanager import UMHSDataManagerConfig
    from .data.umhs_dataparser import UMHSDataParserConfig
    from .umhs_model import UMHSConfig
    from .umhs_pipeline import UMHSPipeline, UMHSPipelineConfig

    parser = UMHSDataParserConfig(data=Path(args.data), eval_mode=args.eval_mode, seg_ignore_label=args.seg_ignore_label)
    model = UMHSConfig(method=args.method, pred_specular=args.pred_specular, temperature=args.temperature,
                       background_color=args.background_color, log2_hashmap_size=args.log2_hashmap_size)
    config = UMHSPipelineConfig(datamanager=UMHSDataManagerConfig(dataparser=parser, images_on_gpu=args.images_on_gpu), model=model,
                                num_classes=args.num_classes)
    return UMHSPipeline(config, device=device, test_mode="val")


def add_model_arguments(ap) -> None:
    """The scene, checkpoint and model flags (shared with ``python -m umhsnerf.render``)."""
    ap.add_argument("--data", required=True, help="scene directory (or its transforms.json)")
    ap.add_argument("--checkpoint", required=True, help="step-*.ckpt of a training run, or a saved pipeline state dict")
    ap.add_argument("--method", default="rgb+spectral", choices=["rgb", "spectral", "rgb+spectral"])
    ap.add_argument("--num-classes", type=int, default=5)
    ap.add_argument("--pred-specular", action="store_true")
    ap.add_argument("--temperature", type=float, default=0.2)
    ap.add_argument("--background-color", default="random", choices=["random", "last_sample", "black", "white"])
    ap.add_argument("--log2-hashmap-size", type=int, default=19)
    ap.add_argument("--eval-mode", default="filename", choices=["fraction", "filename", "interval", "all"])
    ap.add_argument("--seg-ignore-label", type=int, default=255)
    ap.add_argument("--images-on-gpu", type=lambda s: s.lower() in ("1", "true", "yes"), default=True)
    ap.add_argument("--device", default="cuda:0")
    # (absent from the namespace unless given, so the commands' sets of defaults stay what they were)
    ap.add_argument("--load-config", default=argparse.SUPPRESS, metavar="RUN/config.json",
                    help="config.json of a `python -m umhsnerf.train` run: supplies --data, the model flags and the run's latest checkpoint")
    _read_load_config_first(ap)


def load_config_values(path) -> dict:
    """``RUN/config.json`` -> the values of ``add_model_arguments``' flags: the scene, the model options the run was trained with and the
    latest ``step-*.ckpt`` under ``RUN/nerfstudio_models/``."""
    path = Path(path)
    cfg = json.loads(path.read_text())
    pipeline = cfg["pipeline"]
    model, dm = pipeline["model"], pipeline["datamanager"]
    ckpts = sorted((path.parent / "nerfstudio_models").glob("step-*.ckpt"))
    if not ckpts:
        raise FileNotFoundError(f"{path.parent / 'nerfstudio_models'} holds no step-*.ckpt")
    return dict(data=cfg["data"], checkpoint=str(ckpts[-1]), method=model["method"], num_classes=int(pipeline["num_classes"]),
                pred_specular=bool(model["pred_specular"]), temperature=float(model["temperature"]),
                background_color=model["background_color"], log2_hashmap_size=int(model["log2_hashmap_size"]),
                eval_mode=dm["dataparser"]["eval_mode"], seg_ignore_label=int(dm["dataparser"]["seg_ignore_label"]),
                images_on_gpu=bool(dm["images_on_gpu"]))


def _read_load_config_first(ap) -> None:
    """``--load-config`` turns its file into this parser's DEFAULTS before the command line is parsed, whatever its position on it: a
    flag given explicitly then overrides the file, and ``--data`` / ``--checkpoint`` are no longer required."""
    parse = ap.parse_known_args

    def parse_known_args(args=None, namespace=None):
        argv = list(sys.argv[1:] if args is None else args)
        path = None
        for i, a in enumerate(argv):
            if a == "--load-config" and i + 1 < len(argv):
                path = argv[i + 1]
            elif a.startswith("--load-config="):
                path = a.split("=", 1)[1]
        if path is not None:
            try:
                values = load_config_values(path)
            except (OSError, KeyError, ValueError) as e:
                ap.error(f"--load-config {path}: {e}")
            ap.set_defaults(**values)
            for action in ap._actions:
                if action.dest in ("data", "checkpoint"):
                    action.required = False
        return parse(argv, namespace)

    ap.parse_known_args = parse_known_args


def load_checkpoint(pipeline, path) -> int:
    """``load_pipeline`` what nerfstudio's Trainer wrote, or a bare pipeline state dict; -> the step."""
    loaded = torch.load(path, map_location="cpu")
    state, step = (loaded["pipeline"], int(loaded.get("step", 0))) if "pipeline" in loaded else (loaded, 0)
    pipeline.load_pipeline(state, step)
    return step


def build_parser() -> argparse.ArgumentParser:
    from .library import add_library_arguments
    from .statistics import add_statistics_arguments
    from .unmix import add_unmix_arguments
    from .sparse import add_sparse_arguments
    from .continuum import add_continuum_arguments
    from .cluster import add_cluster_arguments

    ap = argparse.ArgumentParser(prog="python -m umhsnerf.eval", description=__doc__.split("\n\n")[0])
    add_model_arguments(ap)
    ap.add_argument("--output-path", default=None, help="directory for eval_<key>_<idx>.png / seg_raw_<idx>.png / seg_pred_<idx>.png")
    add_library_arguments(ap)
    add_statistics_arguments(ap)
    add_unmix_arguments(ap)
    add_sparse_arguments(ap)
    add_continuum_arguments(ap)
    add_cluster_arguments(ap)
    return ap


def main(argv=None) -> dict:
    from . import library as spectral_library
    from . import statistics as scene_statistics
    from . import unmix as unmixing
    from . import sparse as sparse_unmixing
    from . import continuum as continuum_removal
    from . import cluster as spectral_clusters

    args = build_parser().parse_args(argv)
    unmixing.check_unmix_arguments(args)  # ValueError, before the scene is loaded
    sparse_unmixing.check_sparse_arguments(args)
    continuum_removal.check_continuum_arguments(args)
    pipeline = build_pipeline(args, torch.device(args.device))
    step = load_checkpoint(pipeline, args.checkpoint)
    library = spectral_library.load_for_model(args.spectral_library, pipeline.model)
    scene = scene_statistics.context_arguments(args, pipeline.model)  # (a bad statistics file is refused here, before anything is rendered)
    unmixer = unmixing.unmixer_from_args(args, pipeline.model, library)  # (endmembers too close to dependent are refused here)
    sparse_unmixer = sparse_unmixing.sparse_unmixer_from_args(args, library)  # (too many entries are refused here)
    analysis = continuum_removal.analysis_from_args(args, pipeline.model)  # (a bad features file is refused here as well)
    clusters = spectral_clusters.load_for_model(args.clusters, pipeline.model)  # (clusters of another scene are refused here)
    tallies = []
    if clusters is not None:
        # ``cluster_top``: per cluster its share of all pixels and mean score over the rendered pixels; ``cluster_agreement``: the share
        # of rendered pixels whose cluster is the cluster of the captured ``hs_image`` at the same pixel; ``cluster_model_agreement``:
        # cluster_raw against the model's seg_raw after the best one-to-one matching; with label images, ``cluster_seg_acc`` /
        # ``cluster_seg_miou`` / ``cluster_seg_iou_<k>`` of the CAPTURED frames' clusters: the k-means baseline next to ``seg_acc``
        split = pipeline.datamanager.eval_images().split
        grouped = spectral_clusters.ClusterTally(clusters, pipeline.model.device, int(pipeline.model.kwargs["num_classes"]),
                                                 int(getattr(split, "seg_num_labels", 0) or 0), int(getattr(split, "seg_ignore_label", 255)))
        tallies.append((grouped, grouped.result))
    if analysis is not None:
        # per eval image the CAPTURED hs_image goes through the same kernel; over the pixels with rendered accumulation > 0.5, per
        # feature: ``feature_depth_rmse`` and ``feature_center_mae`` of rendered against captured, and both mean depths
        features = continuum_removal.ContinuumTally(analysis, pipeline.model.device)
        tallies.append((features, features.result))
    if library is not None:
        # ``library_top``: the 16 most frequent matched entries over the split (name, share of all pixels, mean angle);
        # ``library_agreement``: the share of rendered pixels (library_raw >= 0) whose match is the match of the captured spectrum
        # ``hs_image`` at the same pixel; ``endmember_matches``: per learnt endmember its three closest entries
        tally = spectral_library.LibraryTally(library.continuum_removed() if args.library_continuum_removed else library,
                                              pipeline.model.device)
        tallies.append((tally, lambda: tally.result(pipeline.model)))
    if scene is not None:
        # ``rx_mean``: the mean of rx_score / B over the rendered pixels (about 1 when the render looks like what the statistics were
        # taken from); ``rx_exceed``: their share above the threshold; ``rx_captured_*``: the same on the captured ``hs_image``
        rx = scene_statistics.StatisticsTally(scene["stats"], pipeline.model.device, scene["threshold"], scene["floor"])
        tallies.append((rx, rx.result))
    if unmixer is not None:
        # per eval image the CAPTURED hs_image is unmixed with the same unmixer; over the pixels with rendered accumulation > 0.5:
        # ``unmix_abundance_rmse`` (--unmix model): the rendered ``abundances`` against the unmixing of the captured spectrum, overall
        # and ``_per_material``; ``unmix_agreement``: the share whose argmax agree (--unmix library: the argmax of the rendered
        # spectrum's unmixing); ``unmix_residual_captured`` / ``_rendered``: the mean RMS misfit -- the captured one says whether the
        # endmembers span the data at all; ``unmix_cap_share``: captured rows the solver stopped at its cap
        mix = unmixing.UnmixTally(unmixer, pipeline.model.device, compare_abundances=args.unmix == "model")
        tallies.append((mix, mix.result))
    if sparse_unmixer is not None:
        # the rendered spectrum and, per eval image, the CAPTURED hs_image are unmixed against the whole library; over the pixels with
        # rendered accumulation > 0.5: ``sparse_top``: the 16 entries of largest mean abundance (name, mean abundance, share of pixels
        # where it is active); ``sparse_mean_count``: the mean number of active entries; ``sparse_agreement``: the share whose dominant
        # entry is the captured spectrum's; ``sparse_residual_rendered`` / ``_captured``: the mean RMS misfit; ``sparse_cap_share``:
        # captured rows stopped at the iteration cap
        lasso = sparse_unmixing.SparseTally(sparse_unmixer, pipeline.model.device)
        tallies.append((lasso, lasso.result))
    if not tallies:
        result = pipeline.get_average_eval_image_metrics(step=step, output_path=args.output_path, get_std=True)
    else:
        with pipeline.model.spectral_library_context(library, args.library_max_angle, args.library_continuum_removed), \
                pipeline.model.scene_statistics_context(**(scene or {"stats": None})), pipeline.model.unmixing_context(unmixer), \
                pipeline.model.sparse_unmixing_context(sparse_unmixer), \
                pipeline.model.continuum_context(analysis, features.output_names() if analysis is not None else None), \
                pipeline.model.spectral_clusters_context(clusters):
            result = pipeline.get_average_eval_image_metrics(step=step, output_path=args.output_path, get_std=True,
                                                             on_frame=lambda idx, outputs, batch: [t.add(outputs, batch) for t, _ in tallies])
        for _, read in tallies:
            result.update(read())
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
    sys.exit(0)
