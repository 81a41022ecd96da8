"""FRQ1 streams packed on the device: Engine.rate_stream (frac_quadtree_rate_stream, from the rate state) and
Engine.encode_quadtree_stream(host_pack=False) (frac_encode_quadtree_stream, from a search), with
encode_quadtree_to_size and the colour container on top of them.  The expected bytes always come from the host
packer over leaves the other GPU tests pin to the oracle: F.pack_frq1 over rate_leaves(t) or over
encode_quadtree(leaves=True) (test_frq1_codec.py pins that packer to codec.pack_quadtree_stream).  Every comparison
is byte equality."""
import ctypes

import numpy as np
import pytest

import fractencode_amd as F
import quadtree_frames as Q
import quadtree_rate_ref as R

pytestmark = pytest.mark.gpu

ENGINES = [F.ENGINE_AUTO, F.ENGINE_VALU]
ENGINE_IDS = {F.ENGINE_AUTO: "auto", F.ENGINE_VALU: "valu"}
BITS = [(5, 7), (2, 2), (11, 13), (16, 16)]  # the last: records above 32 bits, which straddle three dwords
SPREAD_CASES = [Q.BY_NAME[n] for n in ("m98x74_8_2", "m98x74_16_2", "m130x66_8_2", "m70x58_16_2", "e33x47_16_8")] + \
    [Q.HIT_THR, Q.TWO_PLANES] + Q.NODOM + Q.NORANGE
TIMING = ("ms_device", "ms_search", "ms_prep", "ms_finish")


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


def _host(e, case, t, cb=5, bb=7):
    """The host packer over the rate state's leaves at t."""
    return F.pack_frq1(e.rate_leaves(float(t)), case.W, case.H, case.max_size, case.min_size, case.T, case.cls, cb, bb)


def _split(oracle, case):
    return Q.one_split_distance(oracle, case)[0] if case.split is None else float(case.split)


def test_every_candidate_of_one_tree(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    ts = [float(t) for t in R.tree(oracle, case).candidates()] + [-np.inf, -1.0, np.inf]
    with _engine(case) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        sizes, counts, _ = e.rate_sizes(ts)
        for t, size, count in zip(ts, sizes, counts):
            got = e.rate_stream(t)
            assert got == _host(e, case, t), t
            assert len(got) == size, t
            assert F.frq1_info(got)["n_leaves"] == count == len(e.rate_leaves(t)), t
        # −inf splits every node above min_size (bitmaps of all ones), +inf none (N_1 = 0: no bytes for level 1)
        assert F.frq1_info(e.rate_stream(-np.inf))["leaves"][:3] == [0, 0, 16 * 24]
        assert F.frq1_info(e.rate_stream(np.inf))["leaves"][:3] == [24, 0, 0]


@pytest.mark.parametrize("case", SPREAD_CASES, ids=_ids)
def test_geometries_and_record_widths(oracle, case):
    ts = [float(t) for t in R.spread(R.tree(oracle, case).candidates(), 16)]
    with _engine(case) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        for cb, bb in BITS:
            for t in ts:
                got = e.rate_stream(t, cb, bb)
                assert got == _host(e, case, t, cb, bb), (case.name, t, cb, bb)
                if case in Q.NORANGE:
                    assert len(got) == 64


def test_bitmaps_and_sections_of_many_words(oracle):
    case = Q.TILE_CARRY  # 357, 1,428 and 5,712 nodes a level: level 0's bitmap ends mid-word (357 = 11·32 + 5)
    c = R.tree(oracle, case).candidates()
    ts = [float(t) for t in R.spread(c, 8)] + [-np.inf, np.inf]
    with _engine(case) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        for t in ts:
            got = e.rate_stream(t)
            assert got == _host(e, case, t), t
            F.frq1_info(got)  # the parser refuses a set padding bit
        assert F.frq1_info(e.rate_stream(-np.inf))["nodes"][:3] == [357, 1428, 5712]


def test_degenerate_quantizer():
    plane = np.full((48, 64), 93, np.uint8)
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO) as e:
        e.set_frame(plane)
        e.quadtree_rate(16, 4)
        for t in (-1.0, 0.0, np.inf):
            got = e.rate_stream(t)
            assert got == F.pack_frq1(e.rate_leaves(t), 64, 48, 16, 4, 4, False), t
            h = F.frq1_info(got)
            assert h["contrast_min"] == h["contrast_max"] and h["brightness_min"] == h["brightness_max"]
        dev, _ = e.encode_quadtree_stream(16, 4, -1.0, host_pack=False)
        host, _ = e.encode_quadtree_stream(16, 4, -1.0, host_pack=True)
        assert dev == host


def test_cap_and_out():
    case = Q.BY_NAME["m98x74_16_4"]
    t = float(case.split)
    fn = F.lib().frac_quadtree_rate_stream
    with _engine(case) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        want = _host(e, case, t)
        n = ctypes.c_size_t(0)
        e._check(fn(e._ctx, t, 5, 7, None, 0, ctypes.byref(n)))  # NULL: the size only
        assert n.value == len(want) > 65
        for cap in (10, 64, 65, len(want) - 1, len(want), len(want) + 9):
            buf = np.full(len(want) + 16, 0xA5, np.uint8)
            n = ctypes.c_size_t(0)
            e._check(fn(e._ctx, t, 5, 7, buf.ctypes.data, cap, ctypes.byref(n)))
            m = min(cap, len(want))
            assert n.value == len(want), cap
            assert buf[:m].tobytes() == want[:m], cap
            assert (buf[m:] == 0xA5).all(), cap  # nothing past the capacity or the stream
        for cb, bb in ((1, 7), (17, 7), (5, 1), (5, 17)):
            assert fn(e._ctx, t, cb, bb, None, 0, ctypes.byref(n)) == -1  # FRAC_E_INVALID
            with pytest.raises(F.FracError, match="rc=-1"):
                e.rate_stream(t, cb, bb)
            with pytest.raises(F.FracError, match="rc=-1"):
                e.encode_quadtree_stream(case.max_size, case.min_size, t, cb, bb, host_pack=False)
        e.set_frame(case.planes()[0])
        assert fn(e._ctx, t, 5, 7, None, 0, None) == -3  # the state comes first


def test_state_rules(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    t = float(case.split)
    src, _ = case.planes()

    def refused():
        with pytest.raises(F.FracError, match="rc=-3"):
            e.rate_stream(t)

    def run():
        e.set_domains(F.create_uniform_grid(case.W, case.H, 16, 8))
        e.set_ranges(F.create_uniform_grid(case.W, case.H, 8, 8))
        e.quadtree_rate(case.max_size, case.min_size)  # (consumes the range list, keeps the domains)
        e.set_ranges(F.create_uniform_grid(case.W, case.H, 8, 8))
        e.run()

    with _engine(case) as e:
        refused()  # no frame, no build
        _set(e, case)
        refused()
        for end in (lambda: e.set_frame(src), run, lambda: e.encode_quadtree(case.max_size, case.min_size, t),
                    lambda: e.encode_quadtree_stream(case.max_size, case.min_size, t, host_pack=False)):
            e.quadtree_rate(case.max_size, case.min_size)

            def answers():
                sizes = [a.tolist() for a in e.rate_sizes([0.0, t, 1e9])]
                return e.rate_fit(1 << 20), sizes, e.rate_leaves(t).tobytes()

            before = answers()
            stream = e.rate_stream(t)
            assert stream == e.rate_stream(t) == _host(e, case, t)
            assert before == answers()
            with pytest.raises(F.FracError, match="rc=-3"):  # the build ended the last run's results
                e.fetch()
            end()
            refused()
        # a run's results stay readable through a device decode of a stream packed before it
        e.quadtree_rate(case.max_size, case.min_size)
        stream = e.rate_stream(t)
        run()
        e.sync()
        want = e.fetch()[0].copy()
        e.decode_frq1(stream)
        np.testing.assert_array_equal(e.fetch()[0], want)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", Q.ALL, ids=_ids)
def test_the_search_route(oracle, case, engine):
    t = _split(oracle, case)
    with _engine(case, engine) as e:
        _set(e, case)
        dev, st = e.encode_quadtree_stream(case.max_size, case.min_size, t, host_pack=False)
        with pytest.raises(F.FracError, match="rc=-3"):
            e.fetch()
        host, hst = e.encode_quadtree_stream(case.max_size, case.min_size, t, host_pack=True)
        assert dev == host, case.name
        assert {k: v for k, v in st.items() if k not in TIMING} == {k: v for k, v in hst.items() if k not in TIMING}
        dev2, _ = e.encode_quadtree_stream(case.max_size, case.min_size, t, 16, 16, host_pack=False)
        host2, _ = e.encode_quadtree_stream(case.max_size, case.min_size, t, 16, 16, host_pack=True)
        assert dev2 == host2, case.name


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_one_engine_across_frames(oracle, engine):
    # the packer's buffers, slots and zeroed words after a larger frame, a frame without ranges, one without domains
    def rated(e, case):
        e.quadtree_rate(case.max_size, case.min_size)
        got = e.rate_stream(200.0)
        assert got == _host(e, case, 200.0), case.name
        return got

    def searched(e, case):
        return e.encode_quadtree_stream(case.max_size, case.min_size, 400.0, host_pack=False)[0]

    want = []
    for case in Q.SEQUENCE:
        with _engine(case, engine) as f:
            _set(f, case)
            want.append((rated(f, case), searched(f, case)))
    with _engine(Q.SEQUENCE[0], engine) as e:
        for i, case in enumerate(Q.SEQUENCE):
            _set(e, case)
            if i % 2:
                s = searched(e, case)
                streams = (rated(e, case), s)
            else:
                streams = (rated(e, case), searched(e, case))
            assert streams == want[i], case.name


def test_budget_to_stream(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    with _engine(case) as e:
        _set(e, case)
        for b, fits in R.fit_budgets(R.tree(oracle, case)):
            if not fits:
                for hp in (False, True):
                    with pytest.raises(F.FracError, match="rc=-1"):
                        e.encode_quadtree_to_size(b, case.max_size, case.min_size, host_pack=hp)
                continue
            dev, info = e.encode_quadtree_to_size(b, case.max_size, case.min_size, host_pack=False)
            host, hinfo = e.encode_quadtree_to_size(b, case.max_size, case.min_size, host_pack=True)
            assert dev == host and len(dev) <= b, b
            assert {k: v for k, v in info.items() if k not in TIMING} == \
                {k: v for k, v in hinfo.items() if k not in TIMING}


def test_colour_container():
    from fractencode_amd.color import ColorEncoder

    rng = np.random.default_rng(712)
    W, H = 66, 50
    coarse = rng.integers(0, 256, (7, 9, 3)).astype(np.float64)
    rgb = np.clip(np.kron(coarse, np.ones((8, 8, 1)))[:H, :W] + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
    with ColorEncoder(0, 8, 16, 4) as enc:
        enc.load(rgb)
        got, stats = enc.encode_quadtree_frc3(8, 4, 10.0, host_pack=False)
        planes = [e.encode_quadtree_stream(8, 4, 10.0, host_pack=True) for e in enc.engines]
    assert got == F.pack_frc3([s for s, _ in planes], W, H)
    assert [st["items"] for st in stats] == [st["items"] for _, st in planes]
    out = F.decode_color_stream(got)[0]
    assert out.shape == (H, W, 3)
