"""numpy restatement of the rate–distortion pruning rule (include/fracenc.h, "rate–distortion-optimal partitions")
over quadtree_rate_ref.Tree, the oracle's records of the full tree.  Integers throughout (int64 arrays, Python
ints for the multiplier); independent of the library.  test_quadtree_rd_ref.py pins it on the CPU (optimality by
enumeration, sizes and leaves against the host packer); test_gpu_quadtree_rd.py compares the engines with it.

The rule.  Node v of level k has side n = max_size >> k and distortion q(v) = rint(d(v)·64n²), 0 for a negative or
NaN distance.  rb_k = the level's record bits.  A leaf costs rb_k + 1 bits above the last level and rb_k on it, a
split node 1 bit.  For a multiplier lam, bottom-up: J = q + lam·rb on the last level; above it
leafJ = q + lam·(rb_k + 1), splitJ = lam + Σ_children J, the node splits exactly when splitJ < leafJ, and J is the
smaller.  Level 0 is reached, a node is reached when its parent is reached and splits, a reached node that does
not split is a leaf."""
from __future__ import annotations

import numpy as np

import quadtree_frames as Q
import quadtree_rate_ref as R

LAMBDA_MAX = 1 << 32
# the multipliers of the size tests: the ends, small ones, the round values around which the test frames'
# partitions change, and 50 log-spaced ones over the whole interval
SWEEP = sorted({0, 1, 2, 30, 1000, 3000, 10**4, 10**5, 10**7, LAMBDA_MAX}
               | {int(v) for v in np.round(np.logspace(0, 32 * np.log10(2), 50))})


def q(tree: R.Tree) -> list[np.ndarray]:
    """Per level the nodes' integer distortions (int64)."""
    out = []
    for n, rec in zip(tree.sides, tree.recs):
        d = rec["dist"].astype(np.float64)
        v = np.rint(np.where(d > 0, d, 0.0) * (64 * n * n)).astype(np.int64)  # (NaN > 0 is False)
        v.setflags(write=False)
        out.append(v)
    return out


def prune(tree: R.Tree, lam: int, contrast_bits=5, brightness_bits=7):
    """(split, J): per level above the last whether each node would split (decided bottom-up, whether or not the
    node is reached), and level 0's J."""
    assert 0 <= lam <= LAMBDA_MAX
    lam = int(lam)
    qs, rb, L = q(tree), tree.record_bits(contrast_bits, brightness_bits), tree.levels
    J = qs[L - 1] + lam * rb[L - 1]
    split = [None] * (L - 1)
    for k in range(L - 2, -1, -1):
        split_j = lam + J.reshape(-1, 4).sum(axis=1)
        leaf_j = qs[k] + lam * (rb[k] + 1)
        split[k] = split_j < leaf_j
        J = np.minimum(split_j, leaf_j)
    return split, J


def partition(tree: R.Tree, lam: int, contrast_bits=5, brightness_bits=7):
    """(reached, leaf): per level a bool per node."""
    split, _ = prune(tree, lam, contrast_bits, brightness_bits)
    reached, leaf = [], []
    r = np.ones(len(tree.recs[0]), bool)
    for k in range(tree.levels):
        s = r & split[k] if k + 1 < tree.levels else np.zeros(len(r), bool)
        reached.append(r)
        leaf.append(r & ~s)
        r = np.repeat(s, 4)
    return reached, leaf


def size(tree: R.Tree, lam: int, contrast_bits=5, brightness_bits=7) -> tuple[int, int, list[int], int]:
    """(bytes, leaves, S_k padded to four levels, distortion) of the pruned partition's FRQ1 stream."""
    reached, leaf = partition(tree, lam, contrast_bits, brightness_bits)
    rb, qs = tree.record_bits(contrast_bits, brightness_bits), q(tree)
    total, n_leaves, S, dist = R.HEADER, 0, [], 0
    for k in range(tree.levels):
        N, M = int(reached[k].sum()), int(leaf[k].sum())
        if k + 1 < tree.levels:
            total += 4 * ((N + 31) // 32)
            S.append(N - M)
        total += 4 * ((M * rb[k] + 31) // 32)
        n_leaves += M
        dist += int(qs[k][leaf[k]].sum())
    return total, n_leaves, (S + [0, 0, 0, 0])[:4], dist


def leaves(tree: R.Tree, lam: int, contrast_bits=5, brightness_bits=7) -> np.ndarray:
    """The QT_LEAF leaves of the pruned partition in the canonical order: by level, then node order."""
    _, leaf = partition(tree, lam, contrast_bits, brightness_bits)
    recs = [tree.recs[k][leaf[k]] for k in range(tree.levels)]
    sizes = [np.full(int(leaf[k].sum()), n, np.uint32) for k, n in enumerate(tree.sides)]
    return Q.leaves_from_records(Q.as_items(np.concatenate(recs), np.concatenate(sizes)), tree.case.W)


def fit(tree: R.Tree, max_bytes: int, contrast_bits=5, brightness_bits=7):
    """(lam, bytes, leaves, distortion) with size(lam) within the budget and size(lam − 1) above it (or lam = 0),
    by bisection; None when the stream at 2^32, the smallest there is, is above the budget."""
    def fits(lam):
        return size(tree, lam, contrast_bits, brightness_bits)[0] <= max_bytes

    if not fits(LAMBDA_MAX):
        return None
    lo, hi = -1, LAMBDA_MAX  # lo: −1 or a multiplier that does not fit; hi fits
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            hi = mid
        else:
            lo = mid
    b, n, _, d = size(tree, hi, contrast_bits, brightness_bits)
    return hi, b, n, d


def sweep_sizes(tree: R.Tree, contrast_bits=5, brightness_bits=7) -> np.ndarray:
    """The distinct sizes over SWEEP, ascending."""
    return np.unique([size(tree, lam, contrast_bits, brightness_bits)[0] for lam in SWEEP])


def fit_budgets(tree: R.Tree) -> list[tuple[int, bool]]:
    """The budgets of the fit test, from the case's own size list: (budget, whether anything fits)."""
    s = sweep_sizes(tree)
    out = [(int(s[0]), True), (int(s[0]) - 1, False), (int(s[-1]), True), (int(s[-1]) + 1000, True)]
    for m in [int(s[len(s) * f // 4]) for f in (1, 2, 3)]:
        out += [(m, True), (m - 1, m - 1 >= int(s[0]))]
    return out
