"""Environment switches of the Python side, one function each (DESIGN.md section 10 has the whole list, the library's own included).
Read at call time, not at import: tests flip them with ``monkeypatch.setenv`` inside one process."""
import os


def direct_step() -> bool:  # =0: the training step through the autograd Functions instead of the launch sequence
    return os.environ.get("UMHS_DIRECT_STEP", "1") != "0"


def fused_bwd():  # =0 / =1: folded compositing backward off / on; None (unset): by band count
    v = os.environ.get("UMHS_FUSED_BWD", "")
    return v == "1" if v in ("0", "1") else None


def fused_count() -> bool:  # =0: the hash-grid backward's bucket histogram as its own kernel, not in the gather's launch
    return os.environ.get("UMHS_FUSED_COUNT", "1") != "0"


def render_per_ray() -> bool:  # =0: gradient-free rendering through the per-sample path
    return os.environ.get("UMHS_RENDER_PER_RAY", "1") != "0"


def reuse_enc() -> bool:  # =0: the forward hashes the survivors again instead of gathering the sampler's features
    return os.environ.get("UMHS_REUSE_ENC", "1") != "0"


def prefetch_march() -> bool:  # =0: every batch is marched in front of its own step
    return os.environ.get("UMHS_PREFETCH_MARCH", "1") != "0"


def march_cap() -> int:  # scratch row per ray of the single-pass march (0: always two passes)
    return int(os.environ.get("UMHS_MARCH_CAP", "1024"))


def march_serial() -> bool:  # =1: one thread per ray walks the grid inside the emission kernel (no umhs_march_walk)
    return os.environ.get("UMHS_MARCH_SERIAL", "0") == "1"


def fused_adam() -> bool:  # =0: the dense hash levels' Adam step as its own launch
    return os.environ.get("UMHS_FUSED_ADAM", "1") != "0"


def reduce_groups() -> int:  # level groups of the flat-gradient all-reduce
    return int(os.environ.get("UMHS_REDUCE_GROUPS", "2"))


def trust_unit_loss_scale() -> bool:  # =1: never read the loss scale back from the deposited gradient
    return os.environ.get("UMHS_TRUST_UNIT_LOSS_SCALE", "0") == "1"


def check_loss_scale() -> bool:  # =1: read the loss scale back even when the trainer's backward arrives with g = 1
    return os.environ.get("UMHS_CHECK_LOSS_SCALE", "0") == "1"
