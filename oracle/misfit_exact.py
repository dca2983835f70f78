"""Exact arithmetic for the misfit score (TEST INFRASTRUCTURE ONLY: tests/test_misfit_gpu.py, tests/test_constrain.py).

chi2_exact() evaluates one member's score  sum_t p_t (T_t - sum_t b_t T_t - o_t)^2  with no rounding at all, on the member's
own T values (any float dtype, widened exactly) and the observation table's fp64 entries.  chi2_bound() is the derived bound
on how far the fp64 evaluation (the misfit accumulators of include/fiveeq.h "CONSTRAINED RUNS", then
chi2 = V - 2 A U + A^2 P) may lie from it; the derivation is in the docstring of tests/test_misfit_gpu.py::test_r3_score
and of chi2_bound below.

Every fp64 value is a dyadic rational n / 2^k, so one member's inputs are put on the common denominator 2^K (K the largest k
among them) and the sums are taken in Python integers: the same value as fractions.Fraction arithmetic, which is what the
results are returned as, at a fraction of the cost.
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)                 # unit roundoff of fp64


def gamma(k):
    """gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return k * U / (1 - k * U)


def _live(table):
    t = np.asarray(table, dtype=np.float64)
    return np.nonzero((t[:, 1] != 0) | (t[:, 2] != 0))[0]


def window_steps(table):
    """Steps of the observation window [first, last + 1) of nonzero weight (constrain.Observations.window)."""
    live = _live(table)
    return int(live[-1]) - int(live[0]) + 1


def _dyadic(values):
    """Integers n_i and K with values_i == n_i / 2^K exactly (the values: finite floats)."""
    ratios = [float(v).as_integer_ratio() for v in values]
    K = max(d.bit_length() - 1 for _, d in ratios)
    return [n << (K - (d.bit_length() - 1)) for n, d in ratios], K


def member_sums(T_col, table):
    """Exact (chi2, sum_t b_t |T_t|, sum_t p_t |d_t|, sum_t p_t d_t^2, sum_t p_t) of one member as Fractions, with
    d_t = T_t - o_t: the score and the absolute sums the bound is built from.  T_col [n_steps]: the member's T after each step."""
    tab = np.asarray(table, dtype=np.float64)
    live = _live(tab)
    T = np.asarray(T_col)[live].astype(np.float64)                       # fp32 widens exactly
    o, p, b = tab[live, 0], tab[live, 1], tab[live, 2]
    ints, K = _dyadic(np.concatenate([T, o, p, b]))
    n = live.size
    Ti, oi, pi, bi = ints[:n], ints[n:2 * n], ints[2 * n:3 * n], ints[3 * n:]
    A2 = sum(bb * tt for bb, tt in zip(bi, Ti))                            # A = A2 / 2^(2K)
    chi2 = sb = sd = sd2 = 0
    for tt, oo, pp, bb in zip(Ti, oi, pi, bi):
        sb += bb * abs(tt)                                                 # / 2^(2K)
        d = tt - oo                                                        # / 2^K
        sd += pp * abs(d)                                                  # / 2^(2K)
        sd2 += pp * d * d                                                  # / 2^(3K)
        r = (d << K) - A2                                                  # T - o - A, / 2^(2K)
        chi2 += pp * r * r                                                 # / 2^(5K)
    return (Fraction(chi2, 1 << 5 * K), Fraction(sb, 1 << 2 * K), Fraction(sd, 1 << 2 * K), Fraction(sd2, 1 << 3 * K),
            Fraction(sum(pi), 1 << K))


def chi2_exact(T_col, table):
    """sum_t p_t (T_t - sum_t b_t T_t - o_t)^2 of one member, exactly (a Fraction)."""
    return member_sums(T_col, table)[0]


def chi2_bound(T_col, table, acc, P):
    """Bound on |chi2 - chi2_exact(T_col, table)| for chi2 evaluated in fp64 from accumulators acc = (A', U', V') (the
    member's computed fp64 words, added up from zero in step order with every operation rounded on its own) and
    P' = the table's fp64 sum of p_t, as fl(fl(V' - fl(2 A' U')) + fl(fl(A' A') P')).  Returns (exact chi2, bound).

    With k = (steps of the window) + 3 and gamma_k = k u / (1 - k u), u = 2^-53, recursive summation of n <= k - 3 terms
    whose every term carries at most 1 (A: b T), 2 (U: p (T - o)) or 4 (V: (p d) d, d = fl(T - o) counting twice) roundings
    of its own gives |A' - A| <= gamma_k sum b|T| = eA, |U' - U| <= gamma_k sum p|d| = eU, |V' - V| <= gamma_k sum p d^2 = eV
    (Higham eq. 3.4 / lemma 3.3, d = T - o exact), and the fp64 sum of the n_obs <= k nonzero p_t gives |P' - P| <= gamma_k
    sum p = eP.  The exact score is chi2 = V - 2 A U + A^2 P.  Then
      |V' - V|                    <= eV
      |2 A' U' - 2 A U|           <= 2 (eA |U'| + |A'| eU + eA eU)
      |A'^2 P' - A^2 P|           <= (2 |A'| eA + eA^2) P' + (|A'| + eA)^2 eP
    and the evaluation itself — a sum of three terms, each a product of at most two roundings followed by at most two
    additions: fl(2 A' U') (2 A' exact), fl(fl(A' A') P'), V' - x, + y — errs by at most gamma_3 (|V'| + 2 |A' U'| + A'^2 P')
    (the final three roundings each term passes through).  The bound is the sum of the four lines."""
    chi2, sb, sd, sd2, sp = member_sums(T_col, table)
    g = gamma(window_steps(table) + 3)
    eA, eU, eV, eP = g * sb, g * sd, g * sd2, g * sp
    A, Uc, V = (Fraction(float(x)) for x in acc)
    Pc = Fraction(float(P))
    aA, aU = abs(A), abs(Uc)
    bound = (eV + 2 * (eA * aU + aA * eU + eA * eU) + (2 * aA * eA + eA * eA) * Pc + (aA + eA) ** 2 * eP
             + gamma(3) * (abs(V) + 2 * aA * aU + A * A * Pc))
    return chi2, bound
