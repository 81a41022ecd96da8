"""numpy restatement of the quadtree rate rule (include/fracenc.h, "quadtree rate sweep") over the oracle's
distances of the full tree: the candidates, the FRQ1 size at a split distance, the fit for a budget and the
leaves at a split distance.  test_quadtree_rate_ref.py pins it to oracle.quadtree + codec.pack_quadtree_stream
on the CPU; test_gpu_quadtree_rate.py compares the engines with it.

The full tree: level 0 is createUniformGrid(W, H, max, max) in row-major order, level k + 1 holds for each node
of level k in order its quadrants TL, TR, BL, BR.  Each level is searched by oracle.estimate against
createUniformGrid(W, H, 2n, n) exactly as oracle.quadtree searches the nodes it reaches."""
from __future__ import annotations

import numpy as np

import quadtree_frames as Q

HEADER = 64


class Tree:
    """The searched full tree of one case: per level the side, the oracle's records and the domain count;
    e[k] (levels above min_size) the split keys min(d(v), e(parent(v)))."""

    def __init__(self, oracle, case: Q.Case):
        from oracle.oracle import ITEM_DTYPE

        self.case = case
        W, H = case.W, case.H
        src, tgt = case.planes()
        self.sides = []
        n = case.max_size
        while n >= case.min_size:
            self.sides.append(n)
            n //= 2

        def grid(size, offset):
            return oracle.uniform_grid(W, H, size, offset) if W >= size and H >= size else np.zeros(0, ITEM_DTYPE)

        nodes = grid(case.max_size, case.max_size)
        self.recs, self.ndoms, self.e = [], [], []
        self.rejected = 0  # the levels' rejected mappings, as oracle.estimate counts them
        for k, n in enumerate(self.sides):
            doms, rngs = grid(2 * n, n), nodes
            if case.cls:
                doms = oracle.classify(src, doms)
                rngs = oracle.classify(src if tgt is None else tgt, rngs)
            res, rej, _ = oracle.estimate(src, doms, rngs, T=case.T, thr=case.thr, use_classifier=case.cls, tgt=tgt)
            self.rejected += rej
            self.recs.append(res)
            self.ndoms.append(len(doms))
            if k + 1 < len(self.sides):
                d = res["dist"].astype(np.float64)
                self.e.append(d if k == 0 else np.minimum(d, np.repeat(self.e[k - 1], 4)))
                h = n // 2
                nxt = np.zeros(4 * len(nodes), ITEM_DTYPE)
                for q, (qx, qy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                    nxt["x"][q::4], nxt["y"][q::4] = nodes["x"] + qx * h, nodes["y"] + qy * h
                nxt["w"] = nxt["h"] = h
                nxt["category"] = -1
                nodes = nxt
        for a in self.recs + self.e:
            a.setflags(write=False)

    @property
    def levels(self) -> int:
        return len(self.sides)

    def candidates(self) -> np.ndarray:
        """{0.0} ∪ {e(v)}, ascending and distinct."""
        return np.unique(np.concatenate([np.zeros(1)] + self.e))

    def splits(self, t: float) -> list[int]:
        """S_k(t) for the levels above min_size."""
        return [int((e > t).sum()) for e in self.e]

    def record_bits(self, contrast_bits=5, brightness_bits=7) -> list[int]:
        tb = max(1, int(self.case.T - 1).bit_length())
        return [max(1, int(nd).bit_length()) + tb + contrast_bits + brightness_bits for nd in self.ndoms]

    def size(self, t: float, contrast_bits=5, brightness_bits=7) -> tuple[int, int, list[int]]:
        """(bytes, leaves, S_k padded to four levels) of the FRQ1 stream at split distance t."""
        S = self.splits(t)
        rb = self.record_bits(contrast_bits, brightness_bits)
        N, size, leaves = len(self.recs[0]), HEADER, 0
        for k in range(self.levels):
            last = k + 1 == self.levels
            if not last:
                size += 4 * ((N + 31) // 32)
            M = N - (0 if last else S[k])
            size += 4 * ((M * rb[k] + 31) // 32)
            leaves += M
            N = 0 if last else 4 * S[k]
        return size, leaves, (S + [0, 0, 0, 0])[:4]

    def sizes(self, contrast_bits=5, brightness_bits=7) -> np.ndarray:
        """size(t) at every candidate, in candidate order."""
        return np.array([self.size(t, contrast_bits, brightness_bits)[0] for t in self.candidates()], dtype=np.int64)

    def fit(self, max_bytes: int, contrast_bits=5, brightness_bits=7):
        """(t*, bytes, leaves): the least candidate whose size is within the budget; None when none is."""
        for t in self.candidates():
            size, leaves, _ = self.size(float(t), contrast_bits, brightness_bits)
            if size <= max_bytes:
                return float(t), size, leaves
        return None

    def leaves(self, t: float) -> np.ndarray:
        """The QT_LEAF leaves at split distance t, by the rule itself (reached = the parent split; split =
        reached, above min_size and d > t), in the canonical order: by level, then node order."""
        recs, sizes = [], []
        reached = np.ones(len(self.recs[0]), bool)
        for k, n in enumerate(self.sides):
            split = reached & (self.recs[k]["dist"] > t) if k + 1 < self.levels else np.zeros(len(reached), bool)
            leaf = reached & ~split
            recs.append(self.recs[k][leaf])
            sizes.append(np.full(int(leaf.sum()), n, np.uint32))
            reached = np.repeat(split, 4)
        return Q.leaves_from_records(Q.as_items(np.concatenate(recs), np.concatenate(sizes)), self.case.W)


_trees: dict[str, Tree] = {}


def tree(oracle, case: Q.Case) -> Tree:
    """The case's tree, searched once per process and read-only."""
    if case.name not in _trees:
        _trees[case.name] = Tree(oracle, case)
    return _trees[case.name]


def spread(cands: np.ndarray, count: int) -> np.ndarray:
    """`count` candidates spread over the sorted list, both ends included (all of them when there are fewer)."""
    if len(cands) <= count:
        return cands
    return cands[np.unique(np.round(np.linspace(0, len(cands) - 1, count)).astype(int))]


def fit_budgets(t: Tree) -> list[tuple[int, bool]]:
    """The budgets of the fit test, from the case's own size list: (budget, whether anything fits)."""
    s = np.unique(t.sizes())
    mid = [int(s[len(s) * q // 4]) for q in (1, 2, 3)]
    out = [(int(s[0]), True), (int(s[0]) - 1, False), (int(s[-1]), True), (int(s[-1]) + 1000, True)]
    for m in mid:
        out += [(m, True), (m - 1, True)]
    return out


# the cases of the CPU check: every candidate of the first, a spread of the others
FULL = Q.BY_NAME["m98x74_16_4"]
SPREAD = [Q.BY_NAME[n] for n in ("m130x66_8_2", "m70x58_16_2", "e33x47_16_8", "d31x31_16_4", "z15x15", "h98x74_thr",
                                 "p98x74_two", "t342x278_16_4")]
