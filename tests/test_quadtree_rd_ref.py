"""The rate–distortion pruning rule's numpy restatement (quadtree_rd_ref.py) on the CPU: the distortions are exact
integers, the pruned partition is the cheapest of ALL partitions of a subtree (by enumeration, L ≤ 3) and among
the cheapest the one with the fewest nodes, it is never dearer than a split distance's partition (L = 4), the
partitions nest and the sizes do not grow as the multiplier grows, and the size and the leaves are the host
packer's.  Everything here pins the restatement, never the code under test — except the last test, which asks the
built library for the four entry points (it fails on a library without them)."""
import ctypes
import itertools

import numpy as np
import pytest

import fractencode_amd as F
import quadtree_frames as Q
import quadtree_rate_ref as R
import quadtree_rd_ref as RD

LAMBDAS = [0, 1, 1000, 10**5, 1 << 32]


def _ids(c):
    return c.name


@pytest.mark.parametrize("case", Q.ALL, ids=_ids)
def test_distortions_are_exact_integers(oracle, case):
    tree = R.tree(oracle, case)
    for n, rec, qk in zip(tree.sides, tree.recs, RD.q(tree)):
        assert qk.dtype == np.int64
        assert np.array_equal(qk / (64 * n * n), rec["dist"]), case.name  # ==, every node
        assert len(qk) == 0 or (0 <= qk.min() and qk.max() < 1 << 32)
    if case.name == "d31x31_16_4":  # the default record, the largest there is
        assert RD.q(tree)[0].tolist() == [1_638_400_000]


def _enumerate(qs, rb, L, lam, k, j):
    """(cost, nodes) of every partition of the subtree under node j of level k."""
    out = [(int(qs[k][j]) + lam * (rb[k] + (1 if k + 1 < L else 0)), 1)]
    if k + 1 < L:
        kids = [_enumerate(qs, rb, L, lam, k + 1, 4 * j + c) for c in range(4)]
        for combo in itertools.product(*kids):
            out.append((lam + sum(c[0] for c in combo), 1 + sum(c[1] for c in combo)))
    return out


@pytest.mark.parametrize("case", [Q.BY_NAME[n] for n in ("e33x47_16_8", "m98x74_16_4", "d31x31_16_4")], ids=_ids)
def test_the_pruned_partition_is_optimal_by_enumeration(oracle, case):
    tree = R.tree(oracle, case)
    L, qs, rb = tree.levels, RD.q(tree), tree.record_bits()
    assert L in (2, 3) and len(qs[0]) >= 1
    differs = 0
    for lam in LAMBDAS:
        _, J0 = RD.prune(tree, lam)
        reached, leaf = RD.partition(tree, lam)
        for j in range(len(qs[0])):
            every = _enumerate(qs, rb, L, lam, 0, j)
            assert len(every) == (2 if L == 2 else 17)
            best = min(c for c, _ in every)
            fewest = min(n for c, n in every if c == best)
            # the pruned partition of this subtree: its cost from its leaves and splits, its node count
            cost = nodes = 0
            for k in range(L):
                sl = slice(j << (2 * k), (j + 1) << (2 * k))
                lf, rc = leaf[k][sl], reached[k][sl]
                cost += int(qs[k][sl][lf].sum()) + lam * (int(lf.sum()) * (rb[k] + (1 if k + 1 < L else 0))
                                                            + int((rc & ~lf).sum()))
                nodes += int(rc.sum())
            assert cost == int(J0[j]) == best, (case.name, lam, j)
            assert nodes == fewest, (case.name, lam, j)
            differs += len({c for c, _ in every}) > 1
    assert differs  # the partitions of a subtree do not all cost the same: the minimum says something


def test_never_dearer_than_a_split_distance_at_four_levels(oracle):
    case = Q.BY_NAME["m70x58_16_2"]
    tree = R.tree(oracle, case)
    L, qs, rb = tree.levels, RD.q(tree), tree.record_bits()
    assert L == 4
    strictly = 0
    for lam in LAMBDAS:
        J = int(RD.prune(tree, lam)[1].sum())
        b, n, S, d = RD.size(tree, lam)
        reached, leaf = RD.partition(tree, lam)
        bits = sum(int(leaf[k].sum()) * (rb[k] + (1 if k + 1 < L else 0)) + int((reached[k] & ~leaf[k]).sum())
                   for k in range(L))
        assert J == d + lam * bits
        for t in tree.candidates():
            r = np.ones(len(qs[0]), bool)
            cost = 0
            for k in range(L):
                s = r & (tree.recs[k]["dist"] > t) if k + 1 < L else np.zeros(len(r), bool)
                lf = r & ~s
                cost += int(qs[k][lf].sum()) + lam * (int(lf.sum()) * (rb[k] + (1 if k + 1 < L else 0)) + int(s.sum()))
                r = np.repeat(s, 4)
            assert J <= cost, (lam, t)
            strictly += J < cost
    assert strictly


@pytest.mark.parametrize("case", [R.FULL] + R.SPREAD, ids=_ids)
def test_partitions_nest_and_sizes_do_not_grow(oracle, case):
    # (no case here has a size that grows where the dword padding of two sections trades a word; the fit's
    # contract does not rely on it)
    tree = R.tree(oracle, case)
    prev, prev_size = None, None
    for lam in RD.SWEEP:
        reached, _ = RD.partition(tree, lam)
        b = RD.size(tree, lam)[0]
        if prev is not None:
            for k in range(tree.levels):
                assert not (reached[k] & ~prev[k]).any(), (case.name, lam, k)  # reached at lam ⊆ reached below it
            assert b <= prev_size, (case.name, lam)
        prev, prev_size = reached, b
    # the ends: nothing splits at 2^32; at 0 only the distortion counts
    assert RD.size(tree, RD.LAMBDA_MAX)[2] == [0, 0, 0, 0]
    assert RD.size(tree, RD.LAMBDA_MAX)[0] == RD.sweep_sizes(tree)[0]


@pytest.mark.parametrize("case", [R.FULL] + R.SPREAD, ids=_ids)
def test_size_and_leaves_against_the_host_packer(oracle, case):
    tree = R.tree(oracle, case)
    for cb, bb in ((5, 7), (2, 2), (16, 16)):
        for lam in (0, 30, 3000, 10**5, 10**7, 1 << 32):
            lv = RD.leaves(tree, lam, cb, bb)
            b, n, S, d = RD.size(tree, lam, cb, bb)
            # (the packer refuses leaves that are not a partition in canonical order)
            stream = F.pack_frq1(lv, case.W, case.H, case.max_size, case.min_size, case.T, case.cls, cb, bb)
            assert len(stream) == b and len(lv) == n, (case.name, lam, cb, bb)
            assert F.frq1_size(case.W, case.H, case.max_size, case.min_size, S[:max(tree.levels - 1, 1)], case.T, cb,
                               bb) == b
            assert d == int(sum(int(x) for x in np.rint(lv["distance"] * 64.0 * (1 << (lv["code"] >> 28)) ** 2)))
    f = RD.fit(tree, 1 << 20)
    assert f is not None and f[0] == 0


def test_fit_of_the_restatement(oracle):
    tree = R.tree(oracle, R.FULL)
    budgets = RD.fit_budgets(tree)
    assert [ok for _, ok in budgets].count(False) == 1
    lams = set()
    for b, ok in budgets:
        f = RD.fit(tree, b)
        assert (f is not None) == ok
        if ok:
            lam, size, n, d = f
            assert size <= b and (lam == 0 or RD.size(tree, lam - 1)[0] > b)
            assert (size, n, d) == (RD.size(tree, lam)[0], RD.size(tree, lam)[1], RD.size(tree, lam)[3])
            lams.add(lam)
    assert len(lams) >= 5
    z = R.tree(oracle, Q.BY_NAME["z15x15"])
    assert RD.size(z, 5) == (64, 0, [0, 0, 0, 0], 0) and RD.fit(z, 64) == (0, 64, 0, 0) and RD.fit(z, 63) is None


def test_the_library_has_the_entry_points():
    L = F.lib()
    for name in ("frac_quadtree_rd_sizes", "frac_quadtree_rd_fit", "frac_quadtree_rd_leaves",
                 "frac_quadtree_rd_stream"):
        assert hasattr(L, name), name
    n = ctypes.c_size_t(0)
    assert L.frac_quadtree_rd_sizes(None, 5, 7, None, 0, None, None, None, None) == -1  # FRAC_E_INVALID
    assert L.frac_quadtree_rd_fit(None, 5, 7, 1000, None, None, None, None) == -1
    assert L.frac_quadtree_rd_leaves(None, 5, 7, 0, None, 0, ctypes.byref(n)) == -1
    assert L.frac_quadtree_rd_stream(None, 0, 5, 7, None, 0, ctypes.byref(n)) == -1
