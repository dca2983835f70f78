"""Independent reference for the RESAMPLING definition of include/fiveeq.h, in Python integers only: the cumulative list and
bisect_right on (j W + rho) // M.  Shares no code with the product."""
import hashlib
from bisect import bisect_right
from itertools import accumulate


def source_list(weights, n_out, rho=0):
    """source(j) for j = 0 .. n_out - 1 over ALL members: the first m whose inclusive cumulative weight exceeds p_j."""
    w = [int(v) for v in weights]
    cum = list(accumulate(w))
    W = cum[-1]
    assert W >= 1 and 0 <= rho < W and n_out >= 1
    return [bisect_right(cum, (j * W + rho) // n_out) for j in range(n_out)]


def first_output(C, W, n_out, rho):
    """j(C): the first output whose position is at or beyond the cumulative weight C."""
    j = -((rho - C * n_out) // W)                                  # ceil((C M - rho) / W)
    return min(n_out, max(0, j))


def offset(seed, n_out, W):
    if seed is None:
        return 0
    return int.from_bytes(hashlib.sha256(f"{seed}:{n_out}:{W}".encode()).digest()[:8], "little") % W


def weight_patterns(n, rng):
    """name -> int64-range Python-int weights of n members: the patterns the CPU and the GPU tests share."""
    half = [int(v) for v in rng.integers(0, 2 ** 32 + 1, size=n)]
    for i in rng.permutation(n)[:n // 2]:
        half[int(i)] = 0
    if not any(half):
        half[0] = 7
    mask = [int(v) for v in rng.integers(0, 2, size=n)]
    mask[int(rng.integers(0, n))] = 1
    one = [0] * n
    one[int(rng.integers(0, n))] = 12345
    return {"equal": [3] * n, "one_member": one, "random_half_zero": half, "all_2_32": [2 ** 32] * n, "mask": mask}
