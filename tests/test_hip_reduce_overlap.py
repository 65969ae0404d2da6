"""The bucket reduce of the hash-grid backward (hg_reduce_kernel) streams its records in and its gradient slab and Adam moments out
with non-temporal accesses, and reads the operands of the Adam step that rides in its epilogue (in accumulate mode: the slab's own
gradient) per float4 chunk under clamps.  However those accesses are placed or hinted, every result must stay bit for bit what
the unfused path computes:

  side A   hashgrid_bwd_prepare + hashgrid_bwd_apply(overwrite=True, adam=...)      (Adam in the reduce pass's epilogue)
  side B   hashgrid_bwd_prepare + hashgrid_bwd_apply(overwrite=True, adam=None), then ops.adam_step on the same entries

The two sides run different code for the Adam step, so a stale operand, a wrong clamp or an operand of another chunk shows on
side A only.  Shapes are the smallest at which the epilogue's chunking can go wrong: slabs shorter than one chunk (every chunk
clamped), half of the four chunks valid, exactly one epilogue iteration, two buckets, the shipped table; sample counts that
leave buckets without records (N = 1: all but a few), with less than one batch, with a count that is no multiple of the batch
and with several batches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, step=3)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal, with NaN equal to NaN (torch.equal alone calls two identical tensors that hold a NaN different)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na], b[~nb]))


def _inputs(log2_T: int, n: int, seed: int):
    from umhsnerf import ops

    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g).to(DEV)
    d_enc = (torch.randn(ops.NUM_LEVELS, n, 2, generator=g) * 1e-2).to(DEV)
    E = ops.NUM_LEVELS << log2_T
    state = dict(table=(torch.randn(E, 2, generator=g) * 0.1).to(DEV), exp_avg=(torch.randn(E, 2, generator=g) * 1e-3).to(DEV),
                 exp_avg_sq=(torch.rand(E, 2, generator=g) * 1e-6).to(DEV))  # non-zero starting moments
    sc = ops.hash_scalings(ops.NUM_LEVELS, 16, 2048).to(DEV)
    return pos, d_enc, state, sc


def _both_sides(log2_T: int, pos, d_enc, state, sc, level_begin: int):
    """(A, B): dicts of table / exp_avg / exp_avg_sq / grad after one step, the gradient buffers pre-filled with different junk."""
    from umhsnerf import ops

    out = []
    for fused in (True, False):
        st = {k: v.clone() for k, v in state.items()}
        grad = torch.full_like(st["table"], 7.0 if fused else -3.0)  # overwrite mode: every slot must be written
        assert ops.hashgrid_bwd_prepare(pos, sc, log2_T)
        adam = dict(**st, **HYPER, level_begin=level_begin) if fused else None
        ops.hashgrid_bwd_apply(pos, d_enc, sc, log2_T, grad, True, overwrite=True, adam=adam)
        if not fused:
            e0 = level_begin << log2_T
            ops.adam_step(st["table"][e0:], grad[e0:], st["exp_avg"][e0:], st["exp_avg_sq"][e0:], HYPER["step"], HYPER["lr"],
                          HYPER["betas"], HYPER["eps"])
        torch.cuda.synchronize()
        out.append(dict(**st, grad=grad))
    return out


def _assert_sides_equal(A, B, what):
    for k in ("grad", "table", "exp_avg", "exp_avg_sq"):
        assert _same(A[k], B[k]), f"{what}: {k} differs in {int((A[k] != B[k]).sum())} elements"


SHAPES = [(4, 1), (4, 513), (4, 4097), (12, 1), (12, 513), (12, 4097), (13, 1), (13, 513), (13, 4097), (14, 1), (14, 513), (14, 4097),
          (19, 20000)]


@pytest.mark.parametrize("log2_T,n", SHAPES)
def test_adam_in_the_reduce_epilogue_equals_the_separate_step(log2_T, n):
    pos, d_enc, state, sc = _inputs(log2_T, n, seed=100 * log2_T + n % 97)
    A, B = _both_sides(log2_T, pos, d_enc, state, sc, level_begin=5)
    _assert_sides_equal(A, B, f"log2_T={log2_T} n={n}")
    e0 = 5 << log2_T  # levels below the Adam range are left alone, the others moved (zero gradient or not: the moments are not zero)
    assert torch.equal(A["table"][:e0], state["table"][:e0]) and torch.equal(A["exp_avg"][:e0], state["exp_avg"][:e0])
    assert not bool((A["table"][e0:] == state["table"][e0:]).all())
    assert not torch.isnan(A["grad"]).any()


@pytest.mark.parametrize("level_begin", [0, 5])
def test_adam_range_with_levels_on_both_sides(level_begin):
    """All 16 levels are reduced in one launch; the Adam step covers those from ``level_begin`` on (0: every level)."""
    log2_T, n = 14, 4097
    pos, d_enc, state, sc = _inputs(log2_T, n, seed=5 + level_begin)
    A, B = _both_sides(log2_T, pos, d_enc, state, sc, level_begin=level_begin)
    _assert_sides_equal(A, B, f"level_begin={level_begin}")
    e0 = level_begin << log2_T
    assert torch.equal(A["table"][:e0], state["table"][:e0])
    assert not bool((A["table"][e0:] == state["table"][e0:]).all())


def test_level_with_zero_gradient_still_steps():
    """The gradient of one level is exactly zero: its slabs hold zeros and still take their Adam step (the moments decay and move
    the entry).  (Buckets without any record, which take the same path with no tile at all, are what N = 1 above leaves.)"""
    log2_T, n, lev = 14, 4097, 7
    pos, d_enc, state, sc = _inputs(log2_T, n, seed=21)
    d_enc[lev] = 0.0
    A, B = _both_sides(log2_T, pos, d_enc, state, sc, level_begin=0)
    _assert_sides_equal(A, B, "zero-gradient level")
    sl = slice(lev << log2_T, (lev + 1) << log2_T)
    assert torch.equal(A["grad"][sl], torch.zeros_like(A["grad"][sl]))
    assert not bool((A["table"][sl] == state["table"][sl]).all())


def test_level_with_a_nan_gradient():
    """One NaN in a level's gradient: the slabs its records land in are NaN in the gradient (log2_T = 13: one bucket per level,
    so the whole level), every other level is untouched by it, and the parameters are whatever the separate step makes of that."""
    log2_T, n, lev = 13, 4097, 9
    pos, d_enc, state, sc = _inputs(log2_T, n, seed=22)
    d_enc[lev, 3, 0] = float("nan")
    A, B = _both_sides(log2_T, pos, d_enc, state, sc, level_begin=5)
    _assert_sides_equal(A, B, "NaN level")
    sl = slice(lev << log2_T, (lev + 1) << log2_T)
    assert bool(torch.isnan(A["grad"][sl]).all())
    rest = torch.ones(A["grad"].shape[0], dtype=torch.bool, device=DEV)
    rest[sl] = False
    assert not torch.isnan(A["grad"][rest]).any() and not torch.isnan(A["table"][rest]).any()


@pytest.mark.parametrize("log2_T,n", [(12, 4097), (19, 20000)])
def test_accumulate_mode_equals_the_one_call_form(log2_T, n):
    """overwrite=False reads the slab's own gradient in the epilogue: prepare + apply into a pre-filled table == the one-call
    hashgrid_bwd accumulating into a copy of it (no gradient is zero, so both forms emit the same records)."""
    from umhsnerf import ops

    pos, d_enc, state, sc = _inputs(log2_T, n, seed=31 + log2_T)
    want = state["table"].clone()
    ops.hashgrid_bwd(pos, d_enc, sc, log2_T, want, True, method="partition", overwrite=False)
    got = state["table"].clone()
    assert ops.hashgrid_bwd_prepare(pos, sc, log2_T)
    ops.hashgrid_bwd_apply(pos, d_enc, sc, log2_T, got, True, overwrite=False)
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"
    assert not torch.equal(got, state["table"])
