"""The planted frames of tp_tie_frames.py have, on the CPU, the ties their GPU cases rely on (test_gpu_tp_records.py):
from the numpy restatement of the tiled form's layout, and from the oracle for the winner."""
import numpy as np
import pytest

import tp_tie_frames as T

H_THR4 = 16384  # the hit limit of rms threshold 4 at n = 8: 4² · 16 · 64


def _model(name):
    src, tgt, thr = T.case(name)
    hitH = H_THR4 if thr > 0 else -1
    lay = T.layout(src, tgt, hitH)
    least, att, rest = T.attaining(src, tgt, lay, hitH=hitH)
    print(f"{name}: least {least}, attaining (domain, tile, chunk, half, error) {att}, next {min(r[4] for r in rest)}")
    return src, tgt, thr, lay, least, att, rest


def _oracle_winner(oracle, src, tgt, thr):
    doms, rngs = oracle.uniform_grid(T.S, T.S, 16, 8), oracle.uniform_grid(T.S, T.S, 8, 8)
    want, _, _ = oracle.estimate(src, doms, rngs[T.RANGE_INDEX:T.RANGE_INDEX + 1], T=4, thr=thr, tgt=tgt, threads=1)
    assert (int(rngs["x"][T.RANGE_INDEX]), int(rngs["y"][T.RANGE_INDEX])) == T.RANGE_XY
    d = np.flatnonzero((doms["x"] == want["dx"][0]) & (doms["y"] == want["dy"][0]))
    assert len(d) == 1
    return int(d[0]), float(want["dist"][0])


@pytest.mark.parametrize("name", list(T.CASES))
def test_every_window_is_the_whole_bucket(name):
    """A group's seed bound is its noise ranges': every window is the whole bucket, so chunks count from tile 0."""
    _, _, _, lay, _, _, _ = _model(name)
    assert lay["share"] == 1.0 and len(lay["groups"]) == 4
    assert all((t0, t1) == (0, 31) for _, t0, t1, _, _, _ in lay["groups"])
    assert lay["evals"] == lay["eligible"] == 1024 * 961


def test_two(oracle):
    """Exactly two domains attain the least error, in different chunks of one row half: a list of two, in full."""
    src, tgt, thr, _, least, att, rest = _model("two")
    assert least == 16384 and len(att) == 2
    assert att[1][1] - att[0][1] >= 4 and att[0][2] != att[1][2]  # tiles at least 4 apart: two chunks
    assert att[0][3] == att[1][3]                                  # one row half: one record holds both
    assert min(r[4] for r in rest) > 10 * least
    d, dist = _oracle_winner(oracle, src, tgt, thr)
    assert d == min(a[0] for a in att) and dist * 4096.0 == least


def test_three(oracle):
    """Exactly three domains attain it, in three chunks of one row half: more than a record lists (overflow)."""
    src, tgt, thr, _, least, att, rest = _model("three")
    assert least == 16384 and len(att) == 3
    assert len({a[2] for a in att}) == 3 and all(b[1] - a[1] >= 4 for a, b in zip(att, att[1:]))
    assert len({a[3] for a in att}) == 1
    assert min(r[4] for r in rest) > 10 * least
    d, dist = _oracle_winner(oracle, src, tgt, thr)
    assert d == min(a[0] for a in att) and dist * 4096.0 == least


def test_three_in_a_bucket_that_is_not_the_last():
    """The overflow of "three" in a first bucket whose window ends mid-chunk, with a decoy of the same error, earlier
    in domain order, in the next bucket's first tile and in the same row half."""
    src, tgt, rcat, dcat = T.inner_bucket()
    lay = T.layout(src, tgt, -1, rcat=rcat, dcat=dcat)
    least, att, rest = T.attaining(src, tgt, lay)
    _, t0, t1, _, _, _ = lay["groups"][lay["rng_group"][T.RANGE_INDEX]]
    ntiles = int(lay["dom_tile"].max()) + 1
    assert lay["share"] == 1.0 and (t0, t1, ntiles) == (0, 30, 31)
    assert least == 16384 and len(att) == 3 and len({a[2] for a in att}) == 3 and len({a[3] for a in att}) == 1
    assert T.DECOY not in [a[0] for a in att] and min(r[4] for r in rest) > 10 * least
    dx, dy = T.grid(T.S, T.S, 16, 8)
    rx, ry = T.grid(T.S, T.S, 8, 8)
    e = T.errors(src, tgt, rx[T.RANGE_INDEX:T.RANGE_INDEX + 1], ry[T.RANGE_INDEX:T.RANGE_INDEX + 1], dx[T.DECOY:T.DECOY + 1],
                 dy[T.DECOY:T.DECOY + 1])
    assert int(e[0, 0]) == least and T.DECOY < min(a[0] for a in att)
    tile, half = int(lay["dom_tile"][T.DECOY]), int((lay["dom_row"][T.DECOY] // 4) % 2)
    assert t1 <= tile < t0 + 4 * -(-(t1 - t0) // 4) and half == att[0][3]  # inside the last chunk's overhang


def test_superseded(oracle):
    """Two chunks tie at 16384, then a later chunk of the same row half beats both: the list starts again."""
    src, tgt, thr, _, least, att, rest = _model("superseded")
    assert least == 1024 and len(att) == 1
    tied = [r for r in rest if r[4] == 16384]
    assert len(tied) == 2 and all(r[4] > 10 * 16384 for r in rest if r not in tied)
    assert tied[0][2] < tied[1][2] < att[0][2]              # tie, then beaten, in tile (chunk) order
    assert tied[0][3] == tied[1][3] == att[0][3]            # all in one row half
    d, dist = _oracle_winner(oracle, src, tgt, thr)
    assert d == att[0][0] and dist * 4096.0 == least


def test_two_hits(oracle):
    """"two" at threshold 4 (H = 16384): both tied domains are hits, in different chunks; the first in domain order
    wins."""
    src, tgt, thr, _, least, att, _ = _model("two_hits")
    assert thr == 4.0 and least == 16384 and len(att) == 2 and all(a[4] <= H_THR4 for a in att)
    assert att[0][2] != att[1][2] and att[0][3] == att[1][3]
    d, dist = _oracle_winner(oracle, src, tgt, thr)
    assert d == min(a[0] for a in att) and dist * 4096.0 == least


def test_exact(oracle):
    """A single exact match."""
    src, tgt, thr, _, least, att, rest = _model("exact")
    assert least == 0 and len(att) == 1 and min(r[4] for r in rest) > 100000
    d, dist = _oracle_winner(oracle, src, tgt, thr)
    assert d == att[0][0] and dist == 0.0
