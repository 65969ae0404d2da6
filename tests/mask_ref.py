"""CPU restatement of the mask-aware pixel sampler (csrc/umhs_mask.hip): the lists a uint8 mask stack is compacted into and the draw
over them.  Every product is a single float32 multiplication and everything else is integer arithmetic, so the kernels must match
this BIT FOR BIT: no tolerance is involved in any test that uses it.

  lists:  cnt[i] = non-zero pixels of image i;  off = exclusive prefix sum, int64 [n+1], M = off[n];  list = int32 [M], the flat ids
          y*W + x of the set pixels, ascending within an image, images in order (second column of nonzero(mask.view(n, -1))).
  draw:   t = min((int64)(u0 * (float)M), M-1);  image i with off[i] <= t < off[i+1];  k = min((int64)(u1 * (float)cnt[i]), cnt[i]-1);
          p = list[off[i] + k];  row = (i, p / W, p % W).  u[:, 2] is drawn and unused."""
import torch


def mask_lists(mask):
    """mask [n,H,W] uint8 (CPU) -> (off [n+1] int64, list [M] int32)."""
    n = mask.shape[0]
    flat = mask.reshape(n, -1) != 0
    off = torch.zeros(n + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(flat.sum(1, dtype=torch.int64), 0)
    return off, torch.nonzero(flat)[:, 1].to(torch.int32).contiguous()


def pixel_indices_masked(u, off, lst, width):
    """u [R,3] float32 (CPU) -> rows (image, y, x) int64 [R,3]."""
    u = u.to(torch.float32)
    if u.shape[0] == 0:
        return torch.zeros((0, 3), dtype=torch.int64)
    M = off[-1]
    t = (u[:, 0] * M.to(torch.float32)).to(torch.int64).clamp(max=int(M) - 1)
    i = torch.searchsorted(off, t, right=True) - 1
    cnt = off[i + 1] - off[i]
    k = torch.minimum((u[:, 1] * cnt.to(torch.float32)).to(torch.int64), cnt - 1)
    p = lst[off[i] + k].to(torch.int64)
    return torch.stack([i, p // width, p % width], -1).contiguous()


# ---- the cases of tests/test_hip_masks.py (the smallest shapes at which the kernels can go wrong) ------------------------------
def case_a():
    """n=5, 37x53: H*W = 1961 is odd (no image but the first starts on a 16-byte boundary) and no multiple of 64; the stack of 9,805
    pixels crosses a chunk.  Images: empty; random 30 % of 255; only the very last pixel set, to 7; all ones; empty."""
    g = torch.Generator().manual_seed(11)
    m = torch.zeros(5, 37, 53, dtype=torch.uint8)
    m[1] = (torch.rand(37, 53, generator=g) < 0.3).to(torch.uint8) * 255
    m[2, -1, -1] = 7
    m[3] = 1
    return m


def case_b():
    """n=3, 64x64 (an image is exactly one power-of-two run of chunks), random 50 %, pixels 0 and 4095 of every image forced on."""
    g = torch.Generator().manual_seed(12)
    m = (torch.rand(3, 64, 64, generator=g) < 0.5).to(torch.uint8)
    m[:, 0, 0] = 1
    m[:, -1, -1] = 1
    return m


def case_c():
    """n=6, 2048x2048, all set except image 1 (empty) and one further pixel: M = 20,971,519 is odd and above 2^24, so (float)M rounds."""
    m = torch.ones(6, 2048, 2048, dtype=torch.uint8)
    m[1] = 0
    m[4, 1000, 77] = 0
    return m


def case_d():
    """n=1, 1x1, set."""
    return torch.ones(1, 1, 1, dtype=torch.uint8)


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d}


def crafted_rows():
    """u = 0, u = 1.0 (torch.rand never gives it, a caller's block may), u = 1 - 2^-24, (1.0, 0) and (0, 1.0)."""
    below = 1.0 - 2.0 ** -24
    return torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [below, below, below], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]], dtype=torch.float32)


def uniform_rows(n_random=200_000, seed=5):
    """200,005 rows: ``torch.rand`` plus the crafted rows -- deliberately no multiple of 256."""
    return torch.cat([torch.rand(n_random, 3, generator=torch.Generator().manual_seed(seed)), crafted_rows()]).contiguous()
