"""The shape of the two end-of-run summaries (fiveeqscm_amd.distributed: gather_summary, gather_weighted_summary) pinned
without a GPU: the C-ABI passes they call with their sizes, the collectives with their payloads, `stats` and the results bit for
bit, against tests/golden/summary_call_trace.json (recorded by tools/summary_call_trace.py, whose header names the commit);
and the two pure host stages on their own: the selection plan against brute force, the bin-mask packing bit for bit."""
import functools
import json
import os
import sys

import numpy as np
import pytest

from fiveeqscm_amd import distributed as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [f"{kind}{mode}" for kind in ("unweighted", "weighted") for mode in ("", "/split", "/forced", "/forced/split")]


@functools.lru_cache(maxsize=None)
def _traces():
    """(recorded now, the fixture): all eight cases are recorded in one go (one process group for the forced ones)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import summary_call_trace
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    with open(summary_call_trace.FIXTURE) as fh:
        want = json.load(fh)
    return json.loads(json.dumps(summary_call_trace.record())), want["cases"]


@pytest.mark.parametrize("case", CASES)
def test_summary_call_trace_equals_the_recorded_one(case):
    got, want = _traces()
    assert sorted(got) == sorted(want) == sorted(CASES)
    assert got[case]["trace"] == want[case]["trace"]
    assert got[case]["stats"] == want[case]["stats"]
    assert got[case]["result"] == want[case]["result"]


def test_recorded_cases_take_the_paths_they_are_named_for():
    """The fixture itself: the lowered SELECT_CAND_BYTES did split (halves re-run the histogram; row blocks repeat the
    selection), the forced cases did run every collective, values before weights."""
    _, want = _traces()
    names = {c: [t[0] for t in want[c]["trace"]] for c in CASES}
    assert want["unweighted/split"]["stats"]["split_rows"] is True and names["unweighted/split"].count("fiveeq_hist_rows_ranged_f64") == 3
    assert names["weighted/split"].count("fiveeq_wselect_bins_f64") == 2 and names["weighted/split"].count("fiveeq_whist_rows_ranged_f64") == 1
    assert not any(n in ("all_gather", "all_reduce", "gather") for c in CASES if "forced" not in c for n in names[c])
    assert [n for n in names["unweighted/forced"] if not n.startswith("fiveeq")] == ["all_gather", "all_reduce", "all_gather", "gather"]
    coll = [t for t in want["weighted/forced"]["trace"] if not t[0].startswith("fiveeq")]
    assert [t[0] for t in coll] == ["all_gather", "all_reduce", "all_gather", "gather", "gather"]
    assert [t[1] for t in coll[3:]] == ["torch.float64", "torch.int64"]
    assert want["unweighted/forced"]["stats"]["allreduce_bytes"] == 3 * 4096 * 8


# ---- the selection plan against brute force ---------------------------------------------------------------------------------
def _brute_plan(members, want, side, skip):
    """members: per row the list of (bin, amount) in ascending bin order — amount 1 per member for side "right", the member's
    weight for "left".  Walks the sorted members: the bin of each wanted position, then the position among the members of the
    marked bins alone."""
    K, Q = len(members), want.shape[1]
    bins = np.zeros((K, Q), dtype=np.int64)
    pos = np.zeros((K, Q), dtype=np.int64)
    marked = [set() for _ in range(K)]
    for k in range(K):
        if skip[k]:
            continue
        for q in range(Q):
            run, found = 0, members[k][-1][0]
            for b, amount in members[k]:
                run += amount
                if (run > want[k, q]) if side == "right" else (run >= want[k, q]):
                    found = b
                    break
            bins[k, q] = found
            marked[k].add(found)
    for k in range(K):
        for q in range(Q):
            below_all = sum(a for b, a in members[k] if b < bins[k, q])
            below_marked = sum(a for b, a in members[k] if b < bins[k, q] and b in marked[k])
            pos[k, q] = below_marked + want[k, q] - below_all
    return pos, marked


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("per_row", [False, True])
def test_selection_plan_against_brute_force(side, per_row):
    rng = np.random.default_rng(7 + (side == "left") + 2 * per_row)
    K, n_bins, n = 3, 8, 30
    members = []
    for k in range(K):
        b = np.sort(rng.integers(0, n_bins, size=n))
        b[-1] = n_bins - 1                                     # the last bin is never empty: a wanted rank can lie in it
        amount = rng.integers(1, 6, size=n) if side == "left" else np.ones(n, dtype=np.int64)
        members.append([(int(x), int(a)) for x, a in zip(b, amount)])
    counts = np.zeros((K, n_bins), dtype=np.int64)
    for k in range(K):
        for b, a in members[k]:
            counts[k, b] += a
    cum = np.cumsum(counts, axis=1)
    total = cum[:, -1]
    # positions: the first, the last (it lies in the last bin), one on a bin's edge, two in between, one of them twice
    first, last = (0, total - 1) if side == "right" else (1, total)
    edge = np.maximum(cum[:, 2], 1) - (side == "right")
    want = np.stack([np.full(K, first), last, edge, total // 3, total // 2, total // 2], axis=1)
    if not per_row:
        want = np.broadcast_to(want[0], want.shape).clip(max=last.min() if side == "right" else total.min())
    skip = np.array([False, True, False])
    fill = -1 if side == "right" else 0
    pos, n_cand, mask = D._selection_plan(counts, cum, want if per_row else want[0], side, skip, fill)
    ref_pos, ref_marked = _brute_plan(members, want, side, skip)
    assert pos.dtype == np.int64 and pos.shape == (K, 6)
    assert (pos[1] == fill).all() and n_cand[1] == 0 and not mask[1].any()
    for k in (0, 2):
        assert pos[k].tolist() == ref_pos[k].tolist()
        assert n_cand[k] == sum(a for b, a in members[k] if b in ref_marked[k])
        assert mask[k].tolist() == [sum(1 << b for b in ref_marked[k])]
        if want[k, 1] == last[k]:                              # the wanted rank in the last bin (a shared rank is some row's last)
            assert (n_bins - 1) in ref_marked[k]
        if side == "right":                                    # a member index among the candidates
            assert (0 <= pos[k]).all() and (pos[k] < n_cand[k]).all()
        else:                                                  # a cumulative weight to reach among the candidates
            assert (1 <= pos[k]).all() and (pos[k] <= n_cand[k]).all()


def test_weighted_plan_is_the_selection_plan_on_weighted_ranks():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 50, size=(2, 40)).astype(np.int64)
    counts[1] = counts[0]                                      # the weights are shared by the rows: every row sums to W
    cum = np.cumsum(counts, axis=1)
    W, pct, skip = int(cum[0, -1]), (0.0, 5.0, 50.0, 100.0), np.array([False, False])
    targets, mask = D._weighted_plan(counts, cum, W, pct, skip)
    kp = np.array([D.weighted_rank(p, W) for p in pct], dtype=np.int64)
    pos, _, mask2 = D._selection_plan(counts, cum, kp, "left", skip, 0)
    assert targets.dtype == np.int64 and np.array_equal(targets, pos) and np.array_equal(mask, mask2) and mask.shape == (2, 2)


@pytest.mark.parametrize("n_bins", [1, 31, 32, 33, 4096])
def test_bin_mask_packing_bit_for_bit(n_bins):
    rng = np.random.default_rng(n_bins)
    marked = rng.uniform(size=(3, n_bins)) < 0.3
    marked[0] = False
    marked[1] = True
    marked[2, -1] = True
    mask = D._pack_bin_mask(marked)
    words = (n_bins + 31) // 32
    assert mask.dtype == np.uint32 and mask.shape == (3, words)
    for k in range(3):
        for b in range(words * 32):
            bit = (int(mask[k, b // 32]) >> (b % 32)) & 1
            assert bit == (1 if b < n_bins and marked[k, b] else 0), (k, b)
