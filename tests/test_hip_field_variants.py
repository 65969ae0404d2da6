"""Every field-kernel instance the launchers select, against a float64 oracle (cases, oracle runs and bounds: tests/field_f64.py).

The host side in csrc/umhs_field.hip (the backward through the launchers of csrc/umhs_field_bwd_p0z.hip, umhs_field_bwd_p0f.hip and
umhs_field_bwd_p1.hip) picks its kernels by the band count B (TB = ceil(B / 16) band tiles; the backward's TBMAX = 2, 4, 8, 12, 16 for
B <= 32, 64, 128, 192, 256), the specular head, the backward's form (plain umhs_field_bwd / umhs_field_bwd_composited, "folded") and
whether the forward has a workspace.  Per (B, specular head) the default path launches (``instances`` below, the launchers' rule):
  * forward with a workspace: field_fwd_kernel<spec, false, 2, 8, true> (bf16x3 chain); without: <spec, false, 2, 4> (fp32 chain);
    two-launch: the same instance as mlp_base, then <spec, false, 2, 8, true, true>; density-only: <false, true, 2, 4>;
  * backward part 0: the three-piece bf16 chain field_bwd_tfz0_kernel<spec, TBMAX, folded> with the specular head up to 64 bands
    (128 folded), without it up to 192 (256 folded); otherwise the fp32 chain field_bwd_tf_kernel<0, spec, TBMAX, folded>;
    part 1: field_bwd_tfz1_kernel<TBMAX>.  With the specular head above 192 bands the backward is not served (UMHS_ERR_UNSUPPORTED);
  * UMHS_BWD_TF=1 (read once per process) moves both parts to field_bwd_tf_kernel: test_the_fp32_chain_in_a_child_process.
Rows: B on both sides of every tile boundary with and without the specular head, C over 1..15, temperatures other than 1; sample-count
edges (1, 15, 16, 17, 63, 64, 65); per TBMAX one plain backward past 256 workgroups x 64 samples (each workgroup loops and folds) at
16,385 and 39,999 samples; one forward past 256 x 256 samples.  The measured errors of every row are written to field_variants.json in
pytest's temporary directory (its path is printed at the end of the module)."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import field_f64 as F
from field_hip import DEV, Hip, _logits, _ops  # noqa: F401  (tests/field_tf_child.py reads Hip through this module)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPORT = {}


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(n, 16)))


@pytest.fixture(scope="module", autouse=True)
def _report(tmp_path_factory):
    _threads()
    yield
    path = tmp_path_factory.mktemp("field_variants") / "field_variants.json"
    with open(path, "w") as f:
        json.dump(REPORT, f, indent=1)
    print(f"\nfield-variant measurements: {path}")


def tbmax(B: int) -> int:
    TB = (B + 15) // 16
    return next(t for t in (2, 4, 8, 12, 16) if TB <= t)


def part0_bf16(B: int, spec: bool, folded: bool) -> bool:
    """run_field_bwd's rule: part 0 on the three-piece bf16 chain?"""
    t = tbmax(B)
    return (t < 8 or (t == 8 and folded)) if spec else (t < 16 or folded)


def bwd_supported(B: int, spec: bool) -> bool:
    return not (spec and B > 192)


def instances(B: int, spec: bool, folded: bool, fp32_chain: bool = False) -> list:
    s, t, f = str(spec).lower(), tbmax(B), str(folded).lower()
    if not bwd_supported(B, spec):
        return []
    p0 = f"field_bwd_tfz0_kernel<{s}, {t}, {f}>" if part0_bf16(B, spec, folded) and not fp32_chain else \
        f"field_bwd_tf_kernel<0, {s}, {t}, {f}>"
    p1 = f"field_bwd_tf_kernel<1, false, {t}, false>" if fp32_chain else f"field_bwd_tfz1_kernel<{t}>"
    return [p0, p1]


# ------------------------------------------------------------------------------------------------------------------------------ #
# the kernels' side
# ------------------------------------------------------------------------------------------------------------------------------ #
def _fwd_got(o, case):
    got = {k: o[k] for k in F.fwd_keys(case.spec) if k != "feat_logits"}
    got["feat_logits"] = _logits(o, case)
    return got


# ------------------------------------------------------------------------------------------------------------------------------ #
# the table
# ------------------------------------------------------------------------------------------------------------------------------ #
BANDS = (1, 16, 17, 32, 33, 48, 64, 65, 100, 112, 113, 128, 129, 160, 192, 193, 208, 256)
CLASSES = (1, 4, 6, 9, 15)
TEMPS = (0.3, 0.7, 1.6, 0.45, 2.5, 0.9)
N_MAIN = 424  # F.RAY_PATTERN once: empty rays, sub-tile rays, a 200-sample ray; 424 = 26 tiles + 8


def _row(i, B, spec, n, C=None, temp=None):
    C = C if C is not None else CLASSES[i % len(CLASSES)]
    temp = temp if temp is not None else TEMPS[i % len(TEMPS)]
    rid = f"B{B}_{'spec' if spec else 'nospec'}_C{C}_n{n}"
    return pytest.param(C, B, spec, temp, n, i, id=rid)


MAIN = [_row(2 * i + s, B, bool(s), N_MAIN) for i, B in enumerate(BANDS) for s in (1, 0)]
EDGE = [_row(100 + j, B, spec, n, C, t) for j, (C, B, spec, t) in enumerate([(4, 17, True, 0.6), (15, 64, True, 0.8), (9, 113, False, 1.3),
                                                                              (6, 200, False, 0.35)])
        for n in (1, 15, 16, 17, 63, 64, 65)]
# one plain backward per band-tile instance past 256 workgroups x 64 samples: 16,385 (one tile more) and 39,999
LARGE = [_row(200 + j, B, spec, n, C, t) for j, (C, B, spec, t) in enumerate([(3, 32, True, 0.5), (5, 64, False, 0.9), (2, 128, True, 0.4),
                                                                               (4, 192, False, 1.2), (2, 256, False, 0.6)])
         for n in (16385, 39999)]


def _run_row(C, B, spec, temp, n, seed, tag):
    case = F.make_case(C, B, spec, temp, n, seed=seed)
    hip = Hip(case)
    rep = REPORT.setdefault(tag, {"instances_plain": instances(B, spec, False), "instances_folded": instances(B, spec, True)})
    fails = []
    r32, r64 = F.oracle_pair(case, "plain")
    rep["inert_samples"] = case.extra["inert"]
    assert case.extra["inert"] <= max(2, 0.03 * n), f"{case.extra['inert']} of {n} samples with a ReLU at its kink"
    # forward: with the workspace (bf16x3 chain), without it (fp32 chain), two launches, density-only
    fails += F.check_forward(_fwd_got(hip.fwd(), case), r64["out"], F.fwd_keys(spec), rep, "fwd.")
    fails += F.check_forward(_fwd_got(hip.fwd_no_workspace(), case), r64["out"], F.fwd_keys(spec), rep, "fwd_no_ws.")
    base, w, ho = hip.two_launch()
    fails += F.check_forward(base, r64["out"], ["sigma", "sigma_raw", "emb"], rep, "base.")
    fails += F.check_values("heads.abundances", ho["abundances"], r64["out"]["abundances"], rep)
    fails += F.check_values("heads.feat_logits", _logits(ho, case), r64["out"]["feat_logits"], rep)
    # per-ray sums over the kernels' own weights (an input of umhs_field_heads_fwd), in float64
    per_ray = F.oracle_per_ray(case, r64["out"], weights=w.cpu().double())
    comp = dict(zip(["spectral", "spectral2", "specular"], ho["comp"]), abundances=ho["comp_abundances"])
    fails += F.check_forward(comp, per_ray, list(per_ray), rep, "rays.")
    fails += F.check_forward(hip.density(), r64["out"], F.fwd_keys(spec, density_only=True), rep, "density.")
    # backward
    if not bwd_supported(B, spec):
        for call in (lambda: hip.bwd_plain(True), lambda: hip.bwd_folded(True)):
            with pytest.raises(RuntimeError, match=r"\(-2\)"):
                call()
        assert not _ops().field_bwd_composited_supported(hip.fs)
        rep["backward"] = "unsupported"
        return case, hip, fails
    for lm in (True, False):
        fails += F.check_backward(hip.bwd_plain(lm), r32, r64, large=n > 16384, report=rep, prefix=f"bwd_{'lm' if lm else 'sm'}.")
    if n <= 16384:
        assert _ops().field_bwd_composited_supported(hip.fs)
        for gs in (True, False):
            c32, c64 = F.oracle_pair(case, "composited", grad_scaling=gs)
            fails += F.check_backward(hip.bwd_folded(gs), c32, c64, report=rep, prefix=f"folded_gs{int(gs)}.")
    return case, hip, fails


@pytest.mark.parametrize("C,B,spec,temp,n,seed", MAIN + EDGE + LARGE)
def test_field_variant_against_float64(C, B, spec, temp, n, seed, request):
    _, _, fails = _run_row(C, B, spec, temp, n, seed, request.node.callspec.id)
    assert not fails, "; ".join(fails[:12]) + (f" (+{len(fails) - 12} more)" if len(fails) > 12 else "")


def test_forward_past_256_workgroups_of_256_samples():
    """The forward's grid is capped at 256 workgroups (bf16x3: 256 samples each per iteration; fp32 chain: 2 x 256 x 128): 70,001
    samples make every workgroup loop, the last one over a ragged tile."""
    case = F.make_case(4, 48, True, 0.55, 70001, seed=7)
    hip = Hip(case)
    r64 = F.oracle_plain(copy.deepcopy(case.p).double(), case, torch.float64, with_grads=False)
    rep = REPORT.setdefault("forward_n70001", {})
    fails = F.check_forward(_fwd_got(hip.fwd(), case), r64["out"], F.fwd_keys(True), rep, "fwd.")
    fails += F.check_forward(_fwd_got(hip.fwd_no_workspace(), case), r64["out"], F.fwd_keys(True), rep, "fwd_no_ws.")
    assert not fails, "; ".join(fails)


def test_more_than_256_bands_or_15_classes_is_refused_everywhere():
    """B = 257 and C = 16 have no kernel: every entry point of the full field says UMHS_ERR_UNSUPPORTED, the size queries say 0.
    (The density-only form evaluates mlp_base alone, which has no band or class dimension.)"""
    from umhsnerf import _hip

    ops = _ops()
    for C_, B_ in ((4, 257), (16, 31), (16, 257)):
        case = F.make_case(min(C_, 15), min(B_, 256), True, 0.5, 40, seed=3)
        hip = Hip(case)
        layout = ops.FieldLayout(C_, B_, True, 12)
        hip.layout, hip.flat = layout, torch.zeros(layout.total, device=DEV)
        hip.fs = ops.FieldSpec(layout, 0.5, True, scalings=ops.hash_scalings().to(DEV))
        cfg = hip.fs.cfg(False)
        assert _hip.lib().umhs_field_fwd_workspace_bytes(C.byref(cfg)) == 0
        assert _hip.lib().umhs_field_bwd_workspace_bytes(C.byref(cfg), 40) == 0
        assert not ops.field_heads_fwd_supported(hip.fs) and not ops.field_bwd_composited_supported(hip.fs)
        o = {"sigma_raw": torch.zeros(40, device=DEV), "sigma": torch.ones(40, device=DEV), "emb": torch.zeros(40, 15, device=DEV),
             "feat_logits": torch.zeros(40, 16, device=DEV)}
        hip._fwd = o
        hip.case.cot_s = torch.zeros(40, B_)
        hip.case.d_comp = torch.zeros(hip.case.R, B_)
        calls = {"field_fwd": lambda: ops.field_fwd(hip.fs, hip.flat, hip.enc_lm, True, hip.wpos, hip.dirs, hip.sel, want_emb=True),
                 "field_fwd without workspace": hip.fwd_no_workspace,
                 "field_base_fwd": lambda: ops.field_base_fwd(hip.fs, hip.flat, hip.enc_lm, True, hip.sel),
                 "field_heads_fwd": lambda: ops.field_heads_fwd(hip.fs, hip.flat, o["emb"], hip.wpos, hip.dirs, torch.ones(40, device=DEV),
                                                                hip.ray_idx, hip.pinfo, pack_ready=False, release=False),
                 "field_bwd": lambda: hip.bwd_plain(True), "field_bwd_composited": lambda: hip.bwd_folded(True)}
        for name, call in calls.items():
            with pytest.raises(RuntimeError, match=r"\(-2\)"):
                call()
                torch.cuda.synchronize()
                pytest.fail(f"C={C_} B={B_}: {name} accepted")


@pytest.mark.parametrize("C_,B,spec", [(6, 31, True), (4, 141, False), (1, 1, True), (15, 256, False), (9, 100, True)])
def test_a_backward_over_no_samples_writes_zero_gradients(C_, B, spec):
    """umhs_field_bwd's parameter gradients are OVERWRITTEN (header) -- with n = 0 as well: every entry of every weight / bias /
    endmember gradient reads exactly 0.0 afterwards in a buffer that held NaN, on both backward entry points.  (Until this test, n = 0
    returned before writing anything and the previous step's gradient survived.)"""
    ops = _ops()
    case = F.make_case(C_, B, spec, 0.5, 16, seed=5)
    hip = Hip(case)
    e = lambda *shape: torch.empty(shape, device=DEV)
    enc, sel, wpos, dirs = e(16, 0, 2), e(0), e(0, 3), e(0, 3)
    for form in ("umhs_field_bwd", "umhs_field_bwd_composited"):
        g = torch.full_like(hip.flat, float("nan"))
        if form == "umhs_field_bwd":
            ops.field_bwd(hip.fs, hip.flat, enc, True, wpos, dirs, sel, e(0), e(0, 15), e(0), e(0, B), None, g, feat_logits=e(0, 16))
        else:
            R = 5
            cp = dict(sigma=e(0), t0=e(0), t1=e(0), packed_info=torch.zeros(R, 2, dtype=torch.int64, device=DEV),
                      ray_indices=torch.empty(0, dtype=torch.int64, device=DEV), weights=e(0), d_comp=torch.ones(R, B, device=DEV),
                      d_acc=torch.ones(R, device=DEV), grad_scaling=True)
            ops.field_bwd(hip.fs, hip.flat, enc, True, wpos, dirs, sel, e(0), e(0, 15), None, None, None, g, feat_logits=e(0, 16), comp=cp)
        torch.cuda.synchronize()
        for name in hip.layout.entries:  # (the hash table is not the field backward's to write; nor the layout's alignment padding)
            got = hip.layout.view(g, name)
            if name == "mlp_base.encoder.hash_table":
                assert torch.isnan(got).all()
            else:
                assert torch.equal(got, torch.zeros_like(got)), f"{form}, n = 0: {name}: {int(torch.isnan(got).sum())} entries not written"


# ------------------------------------------------------------------------------------------------------------------------------ #
# the fp32 chain (UMHS_BWD_TF=1 is read once per process: a child process runs the backward rows with it)
# ------------------------------------------------------------------------------------------------------------------------------ #
CHILD_ROWS = [p for p in MAIN if bwd_supported(p.values[1], p.values[2])]


def child_rows():
    return [tuple(p.values) + (p.id,) for p in CHILD_ROWS]


def test_the_fp32_chain_in_a_child_process(tmp_path):
    """The backward rows of the table (plain and folded) on field_bwd_tf_kernel<0|1, ...>: tests/field_tf_child.py with UMHS_BWD_TF=1,
    through the same comparators.  This process hands it the default path's gradients of the same calls: where the default runs a
    part on the bf16x3 chain the child's gradients of that part must differ (the knob took effect), where it runs the fp32 chain they
    must be the same bits."""
    default = {}
    for C_, B, spec, temp, n, seed, rid in child_rows():
        hip = Hip(F.make_case(C_, B, spec, temp, n, seed=seed))
        default[rid] = {"plain": hip.bwd_plain(True)["flat"], "folded": hip.bwd_folded(True)["flat"]}
        del hip
    torch.save(default, tmp_path / "default.pt")
    env = dict(os.environ, UMHS_BWD_TF="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "field_tf_child.py"), str(tmp_path / "default.pt"), str(tmp_path / "report.json")],
                       env=env, capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    if os.path.exists(tmp_path / "report.json"):
        with open(tmp_path / "report.json") as f:
            REPORT["fp32_chain_child"] = json.load(f)
    assert r.returncode == 0, out[-4000:]
    assert "FP32 CHAIN OK" in r.stdout, out[-4000:]
