"""CPU checks of the clustering comparators (tests/cluster_f64.py): the float32 replay passes them on every case and both metrics, the
constants are re-measured, the tie cap and the teeth conditions hold on the float64 run alone, the planted faults are rejected, and
the float32 Lloyd replay stays within K_CENTRE of the float64 run."""
import pytest
import torch

import cluster_f64 as CF

FAULT_CASE = (2100, 141, 64)  # three chunks, two cluster tiles
ALL_CASES = CF.CASES + [CF.BOUNDARY_CASE]


def test_float32_replay_passes_and_the_constants_are_what_the_rule_gives():
    worst = {"score": 0.0, "sums": 0.0, "objective": 0.0}
    for c in ALL_CASES:
        for metric in CF.METRICS:
            p, r64 = CF.reference(*c, metric)
            report = {}
            fails = CF.check_step(p, CF.step(p["x"], p["centres"], p["h"], metric), r64, report=report)
            assert not fails, (CF.case_id(c), metric, fails)
            print(CF.case_id(c), metric, {k: round(v, 3) for k, v in report.items()})
            for k, v in report.items():
                worst[k] = max(worst[k], v)
    print("worst", worst)
    assert 4.0 * worst["score"] <= CF.K_S == CF.k_for(worst["score"])
    assert 4.0 * worst["sums"] <= CF.K_SUM == CF.k_for(worst["sums"])
    assert 4.0 * worst["objective"] <= CF.K_OBJ == CF.k_for(worst["objective"])


def test_tie_cap_teeth_and_the_empty_clusters_on_the_float64_run_alone():
    for c in ALL_CASES:
        for metric in CF.METRICS:
            p, r64 = CF.reference(*c, metric)
            cond = CF.conditions(p, r64)
            print(CF.case_id(c), metric, cond)
            if cond["tied"] is not None:
                assert cond["tied"] <= CF.TIE_CAP, (CF.case_id(c), metric, cond)
            if cond["teeth"] is not None:
                assert cond["teeth"] >= CF.MIN_TEETH, (CF.case_id(c), metric, cond)
            if c == CF.EMPTY_CASE:  # (dup_b is one of them by construction)
                assert cond["empty"] >= 5, cond
            assert not CF.check_step(p, CF.step(p["x"], p["centres"], p["h"], metric, torch.float64), r64), (CF.case_id(c), metric)


def test_a_masked_replay_passes_with_the_masked_rows_dead():
    for metric in CF.METRICS:
        p, r64 = CF.reference(1100, 31, 6, metric)
        mask = torch.ones(p["R"])
        mask[::7] = 0.5
        out = CF.step(p["x"], p["centres"], p["h"], metric, mask=mask)
        dead = p["dead"] | (mask <= 0.5)
        assert not CF.check_step(p, out, r64, dead=dead)
        assert CF.check_step(p, out, r64)  # (without the mask those rows are live and must have a label)


FAULTS = {"last band dropped": ("last band", ("angle", "euclidean")), "half_norm not subtracted": ("half norm", ("euclidean",)),
          "ties to the larger index": ("larger index", ("angle", "euclidean")), "one chunk's partial dropped": ("chunk", ("angle", "euclidean")),
          "an invalid row counted": ("invalid counted", ("angle", "euclidean")), "the division of v left out": ("division", ("angle",))}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_rejected(fault):
    name, metrics = FAULTS[fault]
    for metric in metrics:
        p, r64 = CF.reference(*FAULT_CASE, metric)
        assert p["dup"] is not None and int(p["dead"].sum()) >= 4
        fails = CF.check_step(p, CF.step(p["x"], p["centres"], p["h"], metric, fault=name), r64)
        print(metric, fails)
        assert fails, (fault, metric)


def test_the_float32_lloyd_replay_stays_within_k_centre_of_the_float64_run():
    from umhsnerf import cluster

    worst = 0.0
    for shape in CF.FIT_CASES:
        for metric in CF.METRICS:
            data = CF.planted(*shape, metric)
            for seed in range(3):
                init = torch.from_numpy(cluster.kmeanspp(cluster.subsample(data["frames"], seed), shape[2], metric, seed))
                r64 = CF.lloyd(data["frames"], init, metric, torch.float64)
                recovered = CF.partition_agreement(r64["labels"], data["truth"], shape[2])
                if seed == CF.FIT_CASES[shape][metric]:
                    assert recovered >= 0.99, (shape, metric, seed, recovered)
                if recovered < 0.99:
                    continue  # (a seed at which float64 itself stops in a local minimum measures nothing)
                r32 = CF.lloyd(data["frames"], init, metric, torch.float32)
                assert all(torch.equal(a, b) for a, b in zip(r32["partitions"], r64["partitions"])), (shape, metric, seed)
                ratio = CF.centre_ratio(r32["centres"], r64["centres"])
                margin = CF.objective_margin(metric, shape[0])
                assert all(b <= a * (1 + margin[0]) + margin[1] for a, b in zip(r32["objective"][:-1], r32["objective"][1:]))
                print(shape, metric, seed, round(ratio, 3))
                worst = max(worst, ratio)
    print("worst", worst)
    assert 4.0 * worst <= CF.K_CENTRE == CF.k_for(worst)
