"""An independent NumPy statement of the AR(1) noise rows (include/fiveeq.h, "AR(1) NOISE ROWS"), written from the header's
text and sharing no code with fiveeqscm_amd.forcing: the deviate in wrapping uint64 arithmetic, the recursion in fp64 with
every operation rounded on its own.  deviate_ints() states the deviate once more in Python integers, for a handful of
(member, step) pairs."""
import numpy as np

MASK = (1 << 64) - 1
GOLD, ODD = 0x9E3779B97F4A7C15, 0xD1342543DE82EF95


def _mix_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def deviate_ints(seed, M, t):
    """z_t(M) in Python integers: (integer numerator, the float)."""
    mk = _mix_int((seed + GOLD * (M + 1)) & MASK)
    total = 0
    for j in range(6):
        word = _mix_int(mk ^ ((ODD * (6 * (t + 1) + j + 1)) & MASK))
        total += (word >> 32) + (word & 0xFFFFFFFF)
    num = total - 6 * (2 ** 32 - 1)
    return num, num / 2.0 ** 32


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def deviates(seed, members, t):
    """z_t(M) [len(members)] fp64 for one counter t >= -1."""
    M = np.asarray(members, dtype=np.uint64)
    with np.errstate(over="ignore"):
        mk = _mix(np.uint64(seed) + np.uint64(GOLD) * (M + np.uint64(1)))
        total = np.zeros(M.shape, dtype=np.uint64)
        for j in range(6):
            word = _mix(mk ^ np.uint64((ODD * (6 * (t + 1) + j + 1)) & MASK))
            total = total + (word >> np.uint64(32)) + (word & np.uint64(0xFFFFFFFF))
    return (total.astype(np.int64) - 6 * (2 ** 32 - 1)).astype(np.float64) / 2.0 ** 32


def noise_steps(seed, m0, n, t_begin, t_end, phi, s, xi, dtype=np.float64):
    """One call of the generator: (rows [t_end - t_begin, n] in dtype, xi after) for members [m0, m0 + n); phi, s [n] are
    rounded to dtype first, xi [n] is fp64.  [-1, 0) is the start call and returns no rows."""
    ph = np.asarray(phi, dtype=dtype).astype(np.float64)
    sm = np.asarray(s, dtype=dtype).astype(np.float64)
    xi = np.array(xi, dtype=np.float64)
    members = np.arange(m0, m0 + n)
    rows = []
    for t in range(t_begin, t_end):
        w = sm * deviates(seed, members, t)
        xi = ph * xi + w
        if t >= 0:
            rows.append(xi.astype(dtype))
    return (np.stack(rows) if rows else np.empty((0, n), dtype=dtype)), xi


def noise_rows(seed, n_total, n_steps, sigma, phi, lo=0, hi=None, dtype=np.float64, cuts=()):
    """[n_steps, hi - lo]: stationary AR(1) rows of members [lo, hi) — the start at counter -1 times sigma, then the steps,
    cut into calls at `cuts`.  sigma, phi: scalars or rows over the n_total members."""
    hi = n_total if hi is None else hi
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n_total,))[lo:hi]
    ph = np.broadcast_to(np.asarray(phi, dtype=np.float64), (n_total,))[lo:hi]
    s = sg * np.sqrt(1.0 - ph * ph)
    _, xi = noise_steps(seed, lo, hi - lo, -1, 0, ph, sg, np.zeros(hi - lo), dtype)
    edges = [0] + [c for c in cuts if 0 < c < n_steps] + [n_steps]
    parts = []
    for a, b in zip(edges[:-1], edges[1:]):
        rows, xi = noise_steps(seed, lo, hi - lo, a, b, ph, s, xi, dtype)
        parts.append(rows)
    return np.concatenate(parts)
