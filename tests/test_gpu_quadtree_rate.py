"""The quadtree rate sweep (Engine.quadtree_rate, rate_sizes, rate_fit, rate_leaves, encode_quadtree_to_size)
on the frames of quadtree_frames.py.  Each engine is compared with the oracle (oracle.quadtree at the split
distance) or with the oracle-derived restatement of the rule (quadtree_rate_ref.py, pinned to the oracle on the
CPU by test_quadtree_rate_ref.py) — never with another engine or with the code under test — and every value is
exact: leaves bit for bit, sizes and counts as integers, the fit's split distance with == on the double."""
import ctypes

import numpy as np
import pytest

import fractencode_amd as F
import quadtree_frames as Q
import quadtree_rate_ref as R

pytestmark = pytest.mark.gpu

ENGINES = [F.ENGINE_AUTO, F.ENGINE_VALU]
ENGINE_IDS = {F.ENGINE_AUTO: "auto", F.ENGINE_VALU: "valu"}
LEAF_CASES = Q.MIXED + Q.EMPTY + Q.NODOM + Q.NORANGE + [Q.HIT_THR, Q.TWO_PLANES, Q.TILE_CARRY]
FIT_CASES = [Q.BY_NAME[n] for n in ("m98x74_16_4", "m130x66_8_2", "m70x58_16_2")] + [Q.HIT_THR, Q.TWO_PLANES,
                                                                                    Q.TILE_CARRY]


def _ids(v):
    return v.name if isinstance(v, Q.Case) else ENGINE_IDS.get(v, str(v))


@pytest.fixture(scope="module")
def oracle_leaves(oracle):
    """The oracle's leaves of a case at a split distance, computed once and read-only."""
    cache = {}

    def get(case, t):
        if (case.name, t) not in cache:
            src, tgt = case.planes()
            recs, sizes = oracle.quadtree(src, case.max_size, case.min_size, t, T=case.T, use_classifier=case.cls,
                                          thr=case.thr, tgt=tgt)
            leaves = Q.leaves_from_records(Q.as_items(recs, sizes), case.W)
            leaves.setflags(write=False)
            cache[(case.name, t)] = leaves
        return cache[(case.name, t)]

    return get


def _engine(case, engine):
    return F.Engine(0, case.T, case.cls, case.thr, -1.0, engine)


def _set(e, case):
    src, tgt = case.planes()
    if tgt is None:
        e.set_frame(src)
    else:
        e.set_planes(src, tgt)


def _pinned(n):
    import torch

    return torch.zeros(max(n, 1) * F.QT_LEAF.itemsize, dtype=torch.uint8).pin_memory().numpy().view(F.QT_LEAF)


def _cap(case):
    return max((case.W // case.min_size) * (case.H // case.min_size), 1)


def _thresholds(case, tree):
    c = tree.candidates()
    ts = [case.split, -1.0, 0.0, 1e9, float(c[len(c) // 2]), float(c[-1]), float(c[max(len(c) - 2, 0)])]
    return list(dict.fromkeys(float(t) for t in ts))


def _sweep(case, tree):
    """The thresholds of the size test: every candidate of the full case, 60 spread over the others', and −1,
    +inf and midpoints between neighbouring candidates."""
    c = tree.candidates()
    picked = c if case.name == R.FULL.name else R.spread(c, 60)
    mids = 0.5 * (c[:-1] + c[1:]) if case.name == R.FULL.name else R.spread(0.5 * (c[:-1] + c[1:]), 2)
    ts = np.concatenate([picked, [-1.0, np.inf], mids])
    assert case.name == R.FULL.name or len(ts) <= 64
    return ts


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", LEAF_CASES, ids=_ids)
def test_leaves_at_any_split_distance(oracle, oracle_leaves, case, engine):
    tree = R.tree(oracle, case)
    pinned = _pinned(_cap(case) + 3)
    with _engine(case, engine) as e:
        _set(e, case)
        st = e.quadtree_rate(case.max_size, case.min_size)
        for t in _thresholds(case, tree):
            want = oracle_leaves(case, t)
            got = e.rate_leaves(t)
            assert got.dtype == F.QT_LEAF and len(got) == len(want), (case.name, t)
            np.testing.assert_array_equal(got, want, err_msg=f"{case.name} {t}")
        # the device writes pinned memory directly; a short buffer gets its first items, the count stays
        t = float(case.split)
        want = oracle_leaves(case, t)
        pin = e.rate_leaves(t, out=pinned)
        np.testing.assert_array_equal(pin, want)
        assert len(pin) == 0 or np.shares_memory(pin, pinned)
        assert not pinned[len(want):].tobytes().strip(b"\0")  # nothing past the leaves
        if len(want) > 2:
            m = len(want) // 2
            pinned.view(np.uint8)[:] = 0
            n = ctypes.c_size_t(0)
            e._check(F.lib().frac_quadtree_rate_leaves(e._ctx, t, pinned.ctypes.data, m, ctypes.byref(n)))
            assert n.value == len(want)  # the count is the partition's, whatever the capacity
            np.testing.assert_array_equal(pinned[:m], want[:m])
            assert not pinned[m:].tobytes().strip(b"\0")  # nothing past the capacity
            short = e.rate_leaves(t, out=np.zeros(m, F.QT_LEAF), allow_short=True)  # pageable: staged on the device
            np.testing.assert_array_equal(short, want[:m])
    # the full tree's counters: every node against every domain of its level
    assert st["total_mappings"] == sum(len(r) * nd for r, nd in zip(tree.recs, tree.ndoms))
    assert st["empty_ranges"] == sum(int((r["dw"] == 0).sum()) for r in tree.recs)
    assert st["rejected_mappings"] == tree.rejected


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", LEAF_CASES, ids=_ids)
def test_sizes_of_a_sweep(oracle, case, engine):
    tree = R.tree(oracle, case)
    ts = _sweep(case, tree)
    with _engine(case, engine) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        for cb, bb in ((5, 7), (2, 2)):
            size, leaves, splits = e.rate_sizes(ts, cb, bb)
            want = [tree.size(float(t), cb, bb) for t in ts]
            np.testing.assert_array_equal(size, np.array([w[0] for w in want], np.uint64), err_msg=case.name)
            np.testing.assert_array_equal(leaves, np.array([w[1] for w in want], np.uint32), err_msg=case.name)
            np.testing.assert_array_equal(splits, np.array([w[2] for w in want], np.uint32), err_msg=case.name)
            # the reported size is the packed stream's
            for i in (0, len(ts) // 3, len(ts) - 1):
                stream = F.pack_frq1(e.rate_leaves(float(ts[i])), case.W, case.H, case.max_size, case.min_size,
                                     case.T, case.cls, cb, bb)
                assert len(stream) == size[i], (case.name, ts[i], cb, bb)
        assert e.rate_sizes([])[0].shape == (0,)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", FIT_CASES, ids=_ids)
def test_fit_is_the_least_candidate_within_the_budget(oracle, oracle_leaves, case, engine):
    tree = R.tree(oracle, case)
    budgets = R.fit_budgets(tree)
    smallest = budgets[0][0]
    with _engine(case, engine) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        for b, fits in budgets:
            if not fits:
                with pytest.raises(F.FracError, match=f"rc=-1.*smallest size is {smallest} bytes"):
                    e.rate_fit(b)
                continue
            t, size, leaves = e.rate_fit(b)
            wt, wsize, wleaves = tree.fit(b)
            assert t == wt and (size, leaves) == (wsize, wleaves), (case.name, b)
        assert e.rate_fit(smallest)[0] == tree.fit(smallest)[0]  # the refusal left the state readable
        assert e.rate_fit(budgets[2][0])[0] == e.rate_fit(budgets[3][0])[0] == tree.candidates()[0]
        # other record widths, other sizes, another fit
        b22 = int(np.unique(tree.sizes(2, 2))[3])
        assert e.rate_fit(b22, 2, 2) == tree.fit(b22, 2, 2)
        # one call from a budget to a stream: the oracle's leaves at t*, packed; decodes as the fixed-threshold stream
        b = budgets[6][0]
        wt = tree.fit(b)[0]
        stream, info = e.encode_quadtree_to_size(b, case.max_size, case.min_size)
        assert stream == F.pack_frq1(oracle_leaves(case, wt), case.W, case.H, case.max_size, case.min_size, case.T,
                                     case.cls)
        assert len(stream) == info["bytes"] <= b and info["split_distance"] == wt
        assert info["items"] == len(oracle_leaves(case, wt))
        fixed, _ = e.encode_quadtree_stream(case.max_size, case.min_size, wt)
        np.testing.assert_array_equal(e.decode_frq1(stream)[0], e.decode_frq1(fixed)[0])


def test_fit_of_frames_without_ranges_or_domains(oracle):
    for case in Q.NORANGE + [Q.BY_NAME["d31x31_16_4"]]:
        tree = R.tree(oracle, case)
        with _engine(case, F.ENGINE_AUTO) as e:
            _set(e, case)
            e.quadtree_rate(case.max_size, case.min_size)
            assert e.rate_fit(1 << 20) == tree.fit(1 << 20)
            assert e.rate_fit(1 << 20)[0] == 0.0
    assert R.tree(oracle, Q.NORANGE[0]).fit(64) == (0.0, 64, 0)


def _readers_refuse(e):
    for call in (lambda: e.rate_sizes([1.0]), lambda: e.rate_fit(1 << 20), lambda: e.rate_leaves(1.0)):
        with pytest.raises(F.FracError, match="rc=-3"):
            call()


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_the_state_ends_with_the_next_setter_or_search(oracle, oracle_leaves, engine):
    case = Q.BY_NAME["m98x74_16_4"]
    tree = R.tree(oracle, case)
    want = tree.fit(1 << 20)
    src, _ = case.planes()
    with _engine(case, engine) as e:
        _readers_refuse(e)  # no frame, no build
        _set(e, case)
        _readers_refuse(e)
        def search():
            e.set_domains(F.create_uniform_grid(case.W, case.H, 16, 8))
            e.set_ranges(F.create_uniform_grid(case.W, case.H, 8, 8))
            e.quadtree_rate(case.max_size, case.min_size)  # (consumes the range list, keeps the domains)
            e.set_ranges(F.create_uniform_grid(case.W, case.H, 8, 8))
            e.run()

        def run_without_ranges():
            with pytest.raises(F.FracError, match="rc=-3"):  # the build consumed the range list
                e.run()

        enders = [lambda: e.set_frame(src), lambda: e.set_params(rms_threshold=case.thr),
                  lambda: e.set_domains(F.create_uniform_grid(case.W, case.H, 16, 8)),
                  lambda: e.set_ranges(F.create_uniform_grid(case.W, case.H, 8, 8)), run_without_ranges, search,
                  lambda: e.encode_quadtree(case.max_size, case.min_size, case.split),
                  lambda: e.encode_quadtree(case.max_size, case.min_size, case.split, leaves=True)]
        for end in enders:
            e.quadtree_rate(case.max_size, case.min_size)
            assert e.rate_fit(1 << 20) == want  # readable, and the readers leave it so
            e.rate_sizes([0.0, 1.0])
            e.rate_leaves(case.split)
            e.sync()
            assert e.rate_fit(1 << 20) == want
            with pytest.raises(F.FracError, match="rc=-3"):  # the build ended the last run's results
                e.fetch()
            end()
            _readers_refuse(e)
        # a build, then the fixed-threshold encode on the same engine: still the oracle's
        e.quadtree_rate(case.max_size, case.min_size)
        got, _ = e.encode_quadtree(case.max_size, case.min_size, case.split, leaves=True)
        np.testing.assert_array_equal(got, oracle_leaves(case, float(case.split)))


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_one_engine_across_frames(oracle, oracle_leaves, engine):
    # the cached level grids and the state's buffers, sized by an earlier, larger frame; frames without ranges
    # and without 16-level domains in between
    first = Q.SEQUENCE[0]
    with _engine(first, engine) as e:
        for case in Q.SEQUENCE:
            tree = R.tree(oracle, case)
            _set(e, case)
            e.quadtree_rate(case.max_size, case.min_size)
            c = tree.candidates()
            ts = np.concatenate([R.spread(c, 16), [-1.0, np.inf]])
            size, leaves, splits = e.rate_sizes(ts)
            want = [tree.size(float(t)) for t in ts]
            assert [(int(a), int(b), list(s)) for a, b, s in zip(size, leaves, splits)] == \
                [(w[0], w[1], w[2]) for w in want], case.name
            assert e.rate_fit(1 << 20) == tree.fit(1 << 20)
            for t in (float(case.split), float(c[len(c) // 2])):
                np.testing.assert_array_equal(e.rate_leaves(t), oracle_leaves(case, t), err_msg=f"{case.name} {t}")
