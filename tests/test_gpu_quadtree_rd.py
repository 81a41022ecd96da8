"""The rate–distortion readers of the rate state (Engine.rd_sizes, rd_fit, rd_leaves, rd_stream and
encode_quadtree_to_size(rd=True)) on the frames of quadtree_frames.py.  Each engine is compared with the numpy
restatement of the rule (quadtree_rd_ref.py, pinned on the CPU by test_quadtree_rd_ref.py) over the oracle's full
tree — never with another engine or with the code under test — and every value is exact: sizes, counts and
distortions as integers, leaves bit for bit, streams byte for byte.

The cases, by what the pruning kernel does with them (a wave holds whole level-0 subtrees of 4^(L−1) lanes):
  L = 1   d16x16_16_16, d20x20_16_16     no decision, one node
  L = 2   e33x47_16_8, m98x74_16_8       groups of 4 lanes
  L = 3   m98x74_16_4 (six full waves), m130x66_8_2; d31x31_16_4: one subtree in a quarter wave, its level-0
          record the default one at 1e5 (the largest q); t342x278_16_4: 357 subtrees × 16 lanes = 5,712 lanes, a
          wave and a block that end mid-tree; h98x74_thr (records that stopped at a threshold), p98x74_two
  L = 4   m70x58_16_2                    one subtree per wave
  empty   z15x15, z12x40                 no level-0 range: no launch"""
import ctypes

import numpy as np
import pytest

import fractencode_amd as F
import frq1_synth as S
import quadtree_frames as Q
import quadtree_rate_ref as R
import quadtree_rd_ref as RD

pytestmark = pytest.mark.gpu

ENGINES = [F.ENGINE_AUTO, F.ENGINE_VALU]
ENGINE_IDS = {F.ENGINE_AUTO: "auto", F.ENGINE_VALU: "valu"}
EMPTY = [Q.BY_NAME[n] for n in ("z15x15", "z12x40")]
ONE_LEVEL = [Q.BY_NAME[n] for n in ("d16x16_16_16", "d20x20_16_16")]
TREES = [Q.BY_NAME[n] for n in ("e33x47_16_8", "m98x74_16_8", "m98x74_16_4", "m130x66_8_2", "m70x58_16_2",
                                "d31x31_16_4", "t342x278_16_4", "h98x74_thr", "p98x74_two")]
CASES = ONE_LEVEL + TREES + EMPTY
FIT_CASES = [Q.BY_NAME[n] for n in ("e33x47_16_8", "m98x74_16_4", "m130x66_8_2", "m70x58_16_2", "t342x278_16_4",
                                    "h98x74_thr", "p98x74_two")]
OTHER_BITS = {"m98x74_16_4": (2, 2), "m130x66_8_2": (16, 16)}  # beside (5, 7), each on one case
FIVE = [0, 1000, 10**5, 10**7, 1 << 32]


def _ids(v):
    return v.name if isinstance(v, Q.Case) else ENGINE_IDS.get(v, str(v))


def _engine(case, engine=F.ENGINE_AUTO):
    return F.Engine(0, case.T, case.cls, case.thr, -1.0, engine)


def _set(e, case):
    src, tgt = case.planes()
    if tgt is None:
        e.set_frame(src)
    else:
        e.set_planes(src, tgt)


def _built(case, engine=F.ENGINE_AUTO):
    e = _engine(case, engine)
    _set(e, case)
    e.quadtree_rate(case.max_size, case.min_size)
    return e


def _pinned(n):
    import torch

    return torch.zeros(max(n, 1) * F.QT_LEAF.itemsize, dtype=torch.uint8).pin_memory().numpy().view(F.QT_LEAF)


def _cap(case):
    return max((case.W // case.min_size) * (case.H // case.min_size), 1)


def _pack(case, leaves, cb=5, bb=7):
    return F.pack_frq1(leaves, case.W, case.H, case.max_size, case.min_size, case.T, case.cls, cb, bb)


def test_the_cases_reach_what_they_are_kept_for(oracle):
    finest = {c.name: len(R.tree(oracle, c).recs[-1]) if R.tree(oracle, c).recs else 0 for c in CASES}
    assert sorted({R.tree(oracle, c).levels for c in ONE_LEVEL + TREES}) == [1, 2, 3, 4]
    assert finest["d16x16_16_16"] == 1 and finest["d31x31_16_4"] == 16 and finest["t342x278_16_4"] == 5712
    assert finest["m98x74_16_4"] == 6 * 64 and finest["m70x58_16_2"] == 12 * 64
    assert 5712 % 64 and 5712 % 256  # a wave and a block end mid-tree
    assert all(finest[c.name] == 0 for c in EMPTY)
    assert RD.q(R.tree(oracle, Q.BY_NAME["d31x31_16_4"]))[0].tolist() == [1_638_400_000]
    for c in TREES:  # every tree case has several partitions over the sweep, the larger trees many
        assert len(RD.sweep_sizes(R.tree(oracle, c))) >= (20 if finest[c.name] >= 384 else 3), c.name


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_sizes_of_a_sweep_of_multipliers(oracle, case, engine):
    tree = R.tree(oracle, case)
    lams = np.array(RD.SWEEP, np.uint64)
    assert len(lams) > 50 and lams[0] == 0 and lams[-1] == 1 << 32
    with _built(case, engine) as e:
        for cb, bb in [(5, 7)] + [OTHER_BITS[n] for n in OTHER_BITS if n == case.name]:
            want = [RD.size(tree, int(lam), cb, bb) for lam in lams]
            size, leaves, splits, dist = e.rd_sizes(lams, cb, bb)  # one call: several chunks of multipliers
            assert (size.dtype, leaves.dtype, splits.dtype, dist.dtype) == (np.uint64, np.uint32, np.uint32, np.uint64)
            np.testing.assert_array_equal(size, np.array([w[0] for w in want], np.uint64), err_msg=case.name)
            np.testing.assert_array_equal(leaves, np.array([w[1] for w in want], np.uint32), err_msg=case.name)
            np.testing.assert_array_equal(splits, np.array([w[2] for w in want], np.uint32), err_msg=case.name)
            np.testing.assert_array_equal(dist, np.array([w[3] for w in want], np.uint64), err_msg=case.name)
            for lam, w in zip(lams, want):  # one per call: the same answers
                one = e.rd_sizes([lam], cb, bb)
                assert (int(one[0][0]), int(one[1][0]), one[2][0].tolist(), int(one[3][0])) == w, (case.name, lam)
        assert e.rd_sizes([])[0].shape == (0,)
        # optional outputs may be NULL
        b = np.zeros(2, np.uint64)
        two = np.array([0, 1 << 32], np.uint64)
        e._check(F.lib().frac_quadtree_rd_sizes(e._ctx, 5, 7, two.ctypes.data, 2, b.ctypes.data, None, None, None))
        assert b.tolist() == [RD.size(tree, 0)[0], RD.size(tree, 1 << 32)[0]]


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_leaves_and_streams_at_five_multipliers(oracle, case, engine):
    tree = R.tree(oracle, case)
    pinned = _pinned(_cap(case) + 3)
    cb, bb = OTHER_BITS.get(case.name, (5, 7))
    with _built(case, engine) as e:
        for lam in FIVE:
            want = RD.leaves(tree, lam, cb, bb)
            got = e.rd_leaves(lam, cb, bb)  # pageable: staged on the device
            assert got.dtype == F.QT_LEAF and len(got) == len(want), (case.name, lam)
            np.testing.assert_array_equal(got, want, err_msg=f"{case.name} {lam}")
            stream = e.rd_stream(lam, cb, bb)
            assert stream == _pack(case, want, cb, bb), (case.name, lam)
            assert len(stream) == RD.size(tree, lam, cb, bb)[0]
            assert F.frq1_info(stream)["n_leaves"] == len(want)
        # the device writes pinned memory directly; a short buffer gets its first items, the count stays
        lam = 1000
        want = RD.leaves(tree, lam)
        pin = e.rd_leaves(lam, out=pinned)
        np.testing.assert_array_equal(pin, want)
        assert len(pin) == 0 or np.shares_memory(pin, pinned)
        assert not pinned[len(want):].tobytes().strip(b"\0")  # nothing past the leaves
        if len(want) > 2:
            m = len(want) // 2
            pinned.view(np.uint8)[:] = 0
            n = ctypes.c_size_t(0)
            e._check(F.lib().frac_quadtree_rd_leaves(e._ctx, 5, 7, lam, pinned.ctypes.data, m, ctypes.byref(n)))
            assert n.value == len(want)  # the count is the partition's, whatever the capacity
            np.testing.assert_array_equal(pinned[:m], want[:m])
            assert not pinned[m:].tobytes().strip(b"\0")  # nothing past the capacity
            page = np.zeros(m + 2, F.QT_LEAF)
            short = e.rd_leaves(lam, out=page[:m], allow_short=True)
            np.testing.assert_array_equal(short, want[:m])
            assert not page[m:].tobytes().strip(b"\0")
            e._check(F.lib().frac_quadtree_rd_leaves(e._ctx, 5, 7, lam, None, 0, ctypes.byref(n)))  # the count only
            assert n.value == len(want)


def test_a_stream_decodes_as_its_dequantized_leaves(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    with _built(case) as e:
        tree = R.tree(oracle, case)
        lam = next(m for m in RD.SWEEP if all(lf.any() for lf in RD.partition(tree, m)[1]))  # leaves at every level
        stream = e.rd_stream(lam)
        assert all(F.frq1_info(stream)["leaves"][:3])
        plane, it, rms = e.decode_frq1(stream)
        wp, wit, wrms = S.oracle_decode_quadtree_stream(oracle, stream)
        np.testing.assert_array_equal(plane, wp)
        assert (it, rms) == (wit, wrms)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", FIT_CASES, ids=_ids)
def test_fit_meets_the_budget_and_its_predecessor_does_not(oracle, case, engine):
    tree = R.tree(oracle, case)
    budgets = RD.fit_budgets(tree)
    smallest = budgets[0][0]
    seen = set()
    with _built(case, engine) as e:
        for b, fits in budgets:
            if not fits:
                with pytest.raises(F.FracError, match=f"rc=-1.*smallest size is {smallest} bytes"):
                    e.rd_fit(b)
                continue
            lam, size, leaves, dist = e.rd_fit(b)
            assert 0 <= lam <= 1 << 32
            w = RD.size(tree, lam)
            assert w[0] <= b, (case.name, b, lam)
            assert lam == 0 or RD.size(tree, lam - 1)[0] > b, (case.name, b, lam)
            assert (size, leaves, dist) == (w[0], w[1], w[3]), (case.name, b, lam)
            seen.add(lam)
        assert len(seen) >= 4, case.name
        assert e.rd_fit(smallest)[1] == smallest  # the refusal left the state readable
        assert e.rd_fit(budgets[3][0])[0] == 0  # anything fits: only the distortion counts
        # other record widths, other sizes, another fit; NULL outputs
        b22 = int(RD.sweep_sizes(tree, 2, 2)[1])
        lam = e.rd_fit(b22, 2, 2)[0]
        assert RD.size(tree, lam, 2, 2)[0] <= b22 and (lam == 0 or RD.size(tree, lam - 1, 2, 2)[0] > b22)
        e._check(F.lib().frac_quadtree_rd_fit(e._ctx, 5, 7, budgets[3][0], None, None, None, None))


def test_fit_of_one_level_and_of_empty_states(oracle):
    for case in ONE_LEVEL + EMPTY:
        tree = R.tree(oracle, case)
        only = RD.size(tree, 0)
        with _built(case) as e:
            assert e.rd_fit(1 << 20) == (0, only[0], only[1], only[3]), case.name
            assert e.rd_fit(only[0]) == (0, only[0], only[1], only[3]), case.name
            with pytest.raises(F.FracError, match=f"rc=-1.*smallest size is {only[0]} bytes"):
                e.rd_fit(only[0] - 1)
    assert RD.size(R.tree(oracle, EMPTY[0]), 7) == (64, 0, [0, 0, 0, 0], 0)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_budget_to_stream(oracle, engine):
    case = Q.BY_NAME["m98x74_16_4"]
    tree = R.tree(oracle, case)
    with _engine(case, engine) as e:
        _set(e, case)
        for b, fits in RD.fit_budgets(tree):
            if not fits:
                with pytest.raises(F.FracError, match="rc=-1"):
                    e.encode_quadtree_to_size(b, case.max_size, case.min_size, rd=True)
                continue
            stream, info = e.encode_quadtree_to_size(b, case.max_size, case.min_size, rd=True)
            lam, size, n, dist = e.rd_fit(b)
            assert stream == e.rd_stream(lam) == _pack(case, RD.leaves(tree, lam)), b
            assert (info["lambda"], info["bytes"], info["items"], info["distortion"]) == (lam, size, n, dist)
            assert len(stream) == size <= b and "split_distance" not in info
            host, hinfo = e.encode_quadtree_to_size(b, case.max_size, case.min_size, host_pack=True, rd=True)
            assert host == stream and hinfo["lambda"] == lam
            # the default is the split distance's route, its bytes unchanged
            plain, pinfo = e.encode_quadtree_to_size(b, case.max_size, case.min_size)
            t, tsize, tn = e.rate_fit(b)
            assert plain == e.rate_stream(t) == _pack(case, tree.leaves(t))
            assert (pinfo["split_distance"], pinfo["bytes"], pinfo["items"]) == (t, tsize, tn)
            assert "lambda" not in pinfo and "distortion" not in pinfo
            assert plain == e.encode_quadtree_to_size(b, case.max_size, case.min_size, rd=False)[0]


def _readers(e, lam=1000):
    return (lambda: e.rd_sizes([lam]), lambda: e.rd_fit(1 << 20), lambda: e.rd_leaves(lam), lambda: e.rd_stream(lam))


def _readers_refuse(e):
    for call in _readers(e):
        with pytest.raises(F.FracError, match="rc=-3"):
            call()


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_state_rules(oracle, engine):
    case = Q.BY_NAME["m98x74_16_4"]
    tree = R.tree(oracle, case)
    src, _ = case.planes()
    t = float(case.split)
    with _engine(case, engine) as e:
        _readers_refuse(e)  # no frame, no build
        _set(e, case)
        _readers_refuse(e)

        def run():
            e.set_domains(F.create_uniform_grid(case.W, case.H, 16, 8))
            e.set_ranges(F.create_uniform_grid(case.W, case.H, 8, 8))
            e.run()

        for end in (lambda: e.set_frame(src), run, lambda: e.encode_quadtree(case.max_size, case.min_size, t)):
            e.quadtree_rate(case.max_size, case.min_size)
            # the split distance's readers answer the same before and after the RD readers, and these after them
            before = (e.rate_leaves(t).tobytes(), e.rate_stream(t), e.rate_fit(1 << 12),
                      [a.tolist() for a in e.rate_sizes([0.0, t])])
            rd_before = (e.rd_leaves(3000).tobytes(), e.rd_stream(3000))
            for call in _readers(e):
                call()
            assert before == (e.rate_leaves(t).tobytes(), e.rate_stream(t), e.rate_fit(1 << 12),
                              [a.tolist() for a in e.rate_sizes([0.0, t])])
            assert rd_before == (e.rd_leaves(3000).tobytes(), e.rd_stream(3000))
            assert rd_before[0] == RD.leaves(tree, 3000).tobytes()
            # refused arguments, before any launch: the state stays readable
            for call in (lambda: e.rd_sizes([0, (1 << 32) + 1]), lambda: e.rd_leaves((1 << 32) + 1),
                         lambda: e.rd_stream((1 << 32) + 1), lambda: e.rd_sizes([0], 1, 7), lambda: e.rd_fit(4096, 5, 17),
                         lambda: e.rd_leaves(0, 17, 7), lambda: e.rd_stream(0, 5, 1)):
                with pytest.raises(F.FracError, match="rc=-1"):
                    call()
            assert e.rd_stream(3000) == rd_before[1]
            with pytest.raises(F.FracError, match="rc=-3"):  # the build ended the last run's results
                e.fetch()
            end()
            _readers_refuse(e)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_one_engine_across_frames(oracle, engine):
    # the distortions are made on the first RD call after a build and made again after the next one: a larger
    # frame, an empty one, one subtree, a wider frame, the first again
    lams = np.array([0, 30, 3000, 10**5, 1 << 32], np.uint64)
    with _engine(Q.SEQUENCE[0], engine) as e:
        for case in Q.SEQUENCE:
            tree = R.tree(oracle, case)
            _set(e, case)
            e.quadtree_rate(case.max_size, case.min_size)
            want = [RD.size(tree, int(lam)) for lam in lams]
            got = e.rd_sizes(lams)
            assert [(int(a), int(b), s.tolist(), int(d)) for a, b, s, d in zip(*got)] == want, case.name
            np.testing.assert_array_equal(e.rd_leaves(3000), RD.leaves(tree, 3000), err_msg=case.name)
            assert e.rd_stream(3000) == _pack(case, RD.leaves(tree, 3000)), case.name
            f = e.rd_fit(want[2][0])
            assert RD.size(tree, f[0])[0] <= want[2][0] and (f[0] == 0 or RD.size(tree, f[0] - 1)[0] > want[2][0])
