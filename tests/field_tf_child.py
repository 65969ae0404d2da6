"""Helper launched by test_hip_field_variants.test_the_fp32_chain_in_a_child_process with UMHS_BWD_TF=1 (read once per process, so
it cannot be switched inside the test process): the table's backward rows, plain and folded, on the fp32 chain
(field_bwd_tf_kernel<0|1, ...>) through the same comparators as the default path.

argv: the default path's gradients of the same calls (torch.save'd by the parent), a JSON report to write.  Where the default path runs
a part on the bf16x3 chain, this process's gradients of that part must differ from them (the knob took effect); where it runs the fp32
chain already (part 0: the specular head beyond 64 bands, 128 folded; 193-256 bands without it, plain), they must be the same bits.
Prints "FP32 CHAIN OK" when every row passed; exits non-zero otherwise."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "unsupervised-hyperspectral-nerf_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    import torch

    import field_f64 as F
    import test_hip_field_variants as V

    assert os.environ.get("UMHS_BWD_TF") == "1"
    V._threads()
    default = torch.load(sys.argv[1])
    report, failures = {}, []
    part0 = ("head_", "dir_")  # the gradients part 0 alone forms (endmembers: the folded form's per-ray pass)
    for C, B, spec, temp, n, seed, rid in V.child_rows():
        case = F.make_case(C, B, spec, temp, n, seed=seed)
        hip = V.Hip(case)
        rep = report.setdefault(rid, {"instances_plain": V.instances(B, spec, False, True), "instances_folded": V.instances(B, spec, True, True)})
        r32, r64 = F.oracle_pair(case, "plain")
        got = hip.bwd_plain(True)
        failures += [f"{rid}: {m}" for m in F.check_backward(got, r32, r64, report=rep, prefix="bwd_lm.")]
        c32, c64 = F.oracle_pair(case, "composited", grad_scaling=True)
        got_f = hip.bwd_folded(True)
        failures += [f"{rid}: {m}" for m in F.check_backward(got_f, c32, c64, report=rep, prefix="folded_gs1.")]
        for form, g in (("plain", got), ("folded", got_f)):
            mine, theirs = hip.grads(g["flat"].to(V.DEV)), hip.grads(default[rid][form].to(V.DEV))
            p0 = [k for k in mine if k.startswith(part0)]
            p1 = [k for k in mine if k.startswith(("base_", "feat_"))]
            same0 = all(torch.equal(mine[k], theirs[k]) for k in p0 if theirs[k].abs().max() > 0)
            same1 = all(torch.equal(mine[k], theirs[k]) for k in p1)
            if V.part0_bf16(B, spec, form == "folded") == same0:
                failures.append(f"{rid} {form}: part 0's gradients {'equal' if same0 else 'differ from'} the default path's "
                                f"(default part 0 on the {'bf16x3' if V.part0_bf16(B, spec, form == 'folded') else 'fp32'} chain)")
            if same1:
                failures.append(f"{rid} {form}: part 1's gradients are the default path's bits: UMHS_BWD_TF=1 did not take effect")
        del hip
    with open(sys.argv[2], "w") as f:
        json.dump(report, f, indent=1)
    if failures:
        print("\n".join(failures[:40]))
        sys.exit(1)
    print(f"FP32 CHAIN OK ({len(report)} rows, plain and folded)")


if __name__ == "__main__":
    main()
