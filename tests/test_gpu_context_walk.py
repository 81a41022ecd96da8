"""One context walked from state to state (context_states.py): after every change of geometry, route or
parameters, made through the setters for what changed and nothing else, the run's records, tuples and stats
equal a fresh context's in that state, which itself equals the oracle.  Every comparison is exact.

  every ordered pair (A, B)      A, run, fetch; the difference A → B; run, fetch
  the same with A only enqueued  for the states that leave work in flight (a deferred fp32 fallback, the pruned
                                 route's plan, the largest buffers)
  seeded walks                   40 steps with a consumer between steps (FRC1, decode, tuples, device copies,
                                 classify, a quadtree frame, colour conversion, a tuple sink, a stream switch)
  results end at a setter        every reader raises between a setter and the next run
  errors leave it usable         refused geometries, then the corrected call
  frame sizes while streaming    set_frame_async / set_frame_device_async through growing and shrinking frames
  host row strides               the ABI's stride argument, both branches of the plane copy
  classify(target_plane=True)
"""
import dataclasses
import itertools

import numpy as np
import pytest

import context_states as CS
import fractencode_amd as F
from golden_util import FIELDS
from test_gpu_parity import as_oracle_fields

pytestmark = pytest.mark.gpu

STATS = ("engine", "search_form", "matrix_flops", "evaluated_mappings", "rejected_mappings", "hit_ranges",
         "fallback_ranges", "empty_ranges", "total_mappings")

_EXP = {}   # state name → the fresh context's and the oracle's results, for the session
_CONS = {}  # (state name, consumer) → the consumer's output on a fresh context in that state


def _stats(st):
    return {k: st[k] for k in STATS}


def _reach(e, st):
    CS.apply(e, None, st)
    e.run()


def exp(oracle, st):
    """The expectation for a state (a catalogue name or a State): a fresh context's (records, tuples, stats),
    checked against the oracle's fields and reject count before anything is compared with it."""
    st = CS.state(st) if isinstance(st, str) else st
    if st.name not in _EXP:
        with F.Engine(0) as e:
            _reach(e, st)
            out, stats = e.fetch()
            tup = e.fetch_tuples()
        want, rej = CS.expected(oracle, st)
        got = as_oracle_fields(out)
        for k in FIELDS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"fresh context, state {st.name}: field {k}")
        assert stats["rejected_mappings"] == rej, f"fresh context, state {st.name}: reject count"
        assert stats["total_mappings"] == len(st.doms) * len(st.rngs)
        assert stats["empty_ranges"] == int((want["dw"] == 0).sum())
        _EXP[st.name] = (out.tobytes(), tup.tobytes(), _stats(stats), out)
    return _EXP[st.name]


def check(oracle, e, st, what=""):
    """The context's last run against the expectation of `st`: records, tuples, stats."""
    st = CS.state(st) if isinstance(st, str) else st
    rec, tup, stats, want = exp(oracle, st)
    out, got = e.fetch()
    if out.tobytes() != rec:
        bad = {k: int((out[k] != want[k]).sum()) for k in out.dtype.names if k != "_pad" and (out[k] != want[k]).any()} \
            if len(out) == len(want) else {"count": (len(out), len(want))}
        raise AssertionError(f"{what}state {st.name}: records differ from a fresh context's in {bad}")
    assert e.fetch_tuples().tobytes() == tup, f"{what}state {st.name}: tuples differ"
    assert _stats(got) == stats, f"{what}state {st.name}: stats {_stats(got)} != {stats}"
    return out


# ---- every ordered pair -----------------------------------------------------------------------------------------

PAIRS = list(itertools.permutations(CS.NAMES, 2))
ENQUEUED = [(a, b) for a, b in PAIRS if a in CS.ENQUEUE_ONLY]


def test_pairs_are_all_there():
    n = len(CS.NAMES)
    assert len(PAIRS) == n * (n - 1) == len(set(PAIRS)) and len(ENQUEUED) == len(CS.ENQUEUE_ONLY) * (n - 1)


@pytest.mark.parametrize("name", CS.NAMES)
def test_fresh_context_equals_the_oracle(oracle, name):
    exp(oracle, name)


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}->{b}" for a, b in PAIRS])
def test_pair(oracle, a, b):
    A, B = CS.state(a), CS.state(b)
    exp(oracle, A), exp(oracle, B)
    with F.Engine(0) as e:
        _reach(e, A)
        check(oracle, e, A, "first ")
        CS.apply(e, A, B)
        e.run()
        check(oracle, e, B, f"after {a}: ")


@pytest.mark.parametrize("a,b", ENQUEUED, ids=[f"{a}->{b}" for a, b in ENQUEUED])
def test_pair_with_the_first_run_only_enqueued(oracle, a, b):
    """No sync and no fetch after A's run: its deferred fallback is dropped, and buffers it still uses in flight
    are reallocated by B's preparation."""
    A, B = CS.state(a), CS.state(b)
    exp(oracle, B)
    with F.Engine(0) as e:
        _reach(e, A)
        CS.apply(e, A, B)
        e.run()
        check(oracle, e, B, f"after {a} (enqueued only): ")


# ---- seeded walks -----------------------------------------------------------------------------------------------

CONSUMERS = ("frc1", "decode", "tuples", "copy_results", "classify", "quadtree", "rgb", "sink", "stream")
_RGB = np.random.default_rng(4200).integers(0, 256, (12, 20, 3), dtype=np.uint8)


def _outcome(fn):
    """A consumer's output, or the refusal it meets (a fresh and a walked context must agree on either)."""
    try:
        return fn()
    except F.FracError as err:
        return ("FracError", str(err).split(":", 1)[-1].strip())


def _plain(v):
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, (tuple, list)):
        return tuple(_plain(x) for x in v)
    if isinstance(v, dict):
        return tuple((k, _plain(x)) for k, x in sorted(v.items()) if not k.startswith("ms_"))
    return v


def consume(e, st, kind):
    """One consumer on a context whose last run was of `st`; returns its comparable output."""
    W, H = st.source.shape[1], st.source.shape[0]
    if kind == "frc1":
        def go():
            s = e.pack_frc1()
            return s, e.decode_frc1(s, max_iter=3)
        return _plain(_outcome(go))
    if kind == "decode":
        return _plain(_outcome(lambda: e.decode(None, W, H, max_iter=3)))
    if kind == "tuples":
        out = np.zeros(len(st.rngs), dtype=F.TUPLE)
        return _plain(e.fetch_tuples(out))
    if kind == "copy_results":
        import torch

        buf = torch.full((max(len(st.rngs), 1) * F.ENCODE_ITEM.itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        e.copy_results_device(buf.data_ptr())
        e.sync()
        got = buf.cpu().numpy()[:len(st.rngs) * F.ENCODE_ITEM.itemsize].tobytes()
        assert got == e.fetch()[0].tobytes(), "copy_results_device differs from fetch"
        return got
    if kind == "classify":
        return _plain((e.classify(st.doms), e.classify(st.rngs, target_plane=True)))
    if kind == "quadtree":
        return _plain(_outcome(lambda: e.encode_quadtree(16, 4, 10.0)))
    if kind == "rgb":
        return _plain(e.rgb_to_yuv(_RGB))
    raise ValueError(kind)


def consumer_expect(st, kind):
    if (st.name, kind) not in _CONS:
        with F.Engine(0) as e:
            _reach(e, st)
            e.sync()
            _CONS[(st.name, kind)] = consume(e, st, kind)
    return _CONS[(st.name, kind)]


@pytest.mark.parametrize("seed", [4301, 4302, 4303])
def test_seeded_walk(oracle, seed):
    import torch

    rng = np.random.default_rng(seed)
    cat = CS.catalogue()
    cap = max(len(s.rngs) for s in cat) * F.TUPLE.itemsize
    sink = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    other = torch.cuda.Stream()
    torch.cuda.synchronize()
    trail = []
    with F.Engine(0) as e:
        prev, sink_until = None, -1
        for step in range(40):
            st = cat[int(rng.integers(len(cat)))]
            while prev is not None and st.name == prev.name:
                st = cat[int(rng.integers(len(cat)))]
            kind = CONSUMERS[int(rng.integers(len(CONSUMERS)))]
            trail.append(f"{st.name}/{kind}")
            try:
                if step == sink_until:
                    e.set_tuple_sink(None)
                CS.apply(e, prev, st)
                e.run()
                check(oracle, e, st)
                if step < sink_until:  # the run wrote its tuples into the sink as well
                    e.sync()
                    assert sink.cpu().numpy()[:len(st.rngs) * 32].tobytes() == exp(oracle, st)[1], "tuple sink"
                if kind == "sink":
                    if step >= sink_until:
                        e.set_tuple_sink(sink.data_ptr())
                        sink_until = step + 2
                    e.run()
                    e.sync()
                    assert sink.cpu().numpy()[:len(st.rngs) * 32].tobytes() == exp(oracle, st)[1], "tuple sink"
                elif kind == "stream":
                    e.set_stream(other.cuda_stream)
                    check(oracle, e, st, "on the other stream: ")
                    e.run()
                    e.set_stream(None)
                    check(oracle, e, st, "back on its own stream: ")
                elif kind == "quadtree":
                    assert consume(e, st, kind) == consumer_expect(st, kind), "quadtree frame"
                    e.search(st.rngs)  # no set_domains: the caller's are handed back; the ranges were cleared
                else:
                    assert consume(e, st, kind) == consumer_expect(st, kind), f"consumer {kind}"
                check(oracle, e, st, f"after the consumer {kind}: ")
            except (AssertionError, F.FracError) as err:
                raise AssertionError(f"seed {seed}, step {step} ({' '.join(trail[-4:])}): {err}") from err
            prev = st


# ---- results end at a setter ------------------------------------------------------------------------------------

def _variant(name, base="base", **kw):
    return dataclasses.replace(CS.state(base), name=name, **kw)


def _other_plane():
    return CS.state("sea_per_range").source  # 64×64 value noise, not the base's


def _readers(e, st):
    import torch

    nr = max(len(st.rngs), 1)
    buf = torch.zeros(nr * F.ENCODE_ITEM.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    W, H = st.source.shape[1], st.source.shape[0]
    return {"fetch": e.fetch, "fetch_tuples": e.fetch_tuples,
            "copy_tuples_device": lambda: e.copy_tuples_device(buf.data_ptr()),
            "copy_results_device": lambda: e.copy_results_device(buf.data_ptr()),
            "pack_frc1": e.pack_frc1, "decode": lambda: e.decode(None, W, H, max_iter=2)}, buf


def _assert_unreadable(e, st, what):
    readers, buf = _readers(e, st)
    for name, fn in readers.items():
        with pytest.raises(F.FracError):
            fn()
            pytest.fail(f"{what}: {name} returned results that belong to the state before the change")
    assert e.device_results_ptr() == 0, f"{what}: device_results_ptr"
    e.sync()  # (buf outlives anything a reader might have enqueued on it)


class TestResultsEndAtASetter:
    """Between a setter and the next run no reader returns the old run's results (FRAC_E_STATE); after the run they
    give the new state's."""

    def _go(self, oracle, A, B, change):
        exp(oracle, A), exp(oracle, B)
        with F.Engine(0) as e:
            _reach(e, A)
            check(oracle, e, A)
            assert e.device_results_ptr() != 0
            change(e)
            _assert_unreadable(e, A, f"{A.name} → {B.name}")
            e.run()
            check(oracle, e, B, f"after {A.name}: ")
            for name, fn in _readers(e, B)[0].items():
                if name != "pack_frc1" or B.frc1:
                    fn()  # readable again
            e.sync()
            return _outcome(e.pack_frc1)

    def test_pack_frc1_after_t8_then_set_params_t4(self, oracle):
        """The defect this class was written for: a T = 8 result packed under transforms = 4 put 3-bit transforms
        into 2 bits with transforms = 4 in the header."""
        A, B = CS.state("t8"), CS.state("base")
        stream = self._go(oracle, A, B, lambda e: e.set_params(transforms=4))
        assert F.frc1_info(stream)["transforms"] == 4
        with F.Engine(0) as e:
            _reach(e, B)
            assert e.pack_frc1() == stream

    @pytest.mark.parametrize("b,kw", [("t8", {"transforms": 8}), ("cls", {"use_classifier": True}),
                                      ("thr40", {"rms_threshold": 40.0}), ("smax05", {"s_max": 0.5})])
    def test_set_params(self, oracle, b, kw):
        self._go(oracle, CS.state("base"), CS.state(b), lambda e: e.set_params(**kw))

    def test_set_params_with_a_fallback_pending(self, oracle):
        """The fp32-regime ranges' deferred fallback is dropped with the results it would have completed."""
        B = _variant("fp32_t8", "fp32", transforms=8)
        self._go(oracle, CS.state("fp32"), B, lambda e: e.set_params(transforms=8))

    def test_set_domains(self, oracle):
        B = CS.state("dom_stride4")
        self._go(oracle, CS.state("base"), B, lambda e: e.set_domains(B.doms))

    def test_set_ranges(self, oracle):
        B = CS.state("perm37")
        self._go(oracle, CS.state("base"), B, lambda e: e.set_ranges(B.rngs))

    def test_set_frame(self, oracle):
        B = _variant("base_plane2", source=_other_plane())
        self._go(oracle, CS.state("base"), B, lambda e: e.set_frame(B.source))

    def test_set_planes(self, oracle):
        B = _variant("base_target2", target=_other_plane())
        self._go(oracle, CS.state("base"), B, lambda e: e.set_planes(B.source, B.target))

    def test_set_frame_async(self, oracle):
        import torch

        B = _variant("base_plane2", source=_other_plane())
        host = torch.from_numpy(B.source.copy()).pin_memory()
        self._go(oracle, CS.state("base"), B, lambda e: e.set_frame_async(host))

    def test_set_frame_device_async(self, oracle):
        import torch

        B = _variant("base_plane2", source=_other_plane())
        dev = torch.from_numpy(B.source.copy()).to("cuda:0")
        torch.cuda.synchronize()
        self._go(oracle, CS.state("base"), B, lambda e: e.set_frame_device_async(dev))


# ---- errors leave the context usable ----------------------------------------------------------------------------

def _plane48():
    return np.ascontiguousarray(CS.state("base").source[:48, :48])


def _refused(e, st, what):
    with pytest.raises(F.FracError):
        e.run()
    _assert_unreadable(e, st, what)


def test_frame_shrunk_under_ranges_that_no_longer_fit(oracle):
    base = CS.state("base")
    B = _variant("base48", source=_plane48(), doms=CS.grid(48, 48, 16, 8), rngs=CS.grid(48, 48, 8, 8))
    with F.Engine(0) as e:
        _reach(e, base)
        check(oracle, e, base)
        e.set_frame(B.source)
        _refused(e, base, "ranges outside the shrunk frame")
        e.set_domains(B.doms)
        _refused(e, base, "ranges still outside")
        e.set_ranges(B.rngs)
        e.run()
        check(oracle, e, B)


def test_frame_shrunk_under_domains_that_no_longer_fit(oracle):
    r8 = CS.state("base").rngs
    inside = r8[(r8["x"] < 48) & (r8["y"] < 48)]
    A = _variant("base_inner_ranges", rngs=inside)
    B = _variant("base48", source=_plane48(), doms=CS.grid(48, 48, 16, 8), rngs=CS.grid(48, 48, 8, 8))
    assert B.rngs.tobytes() == inside.tobytes()
    with F.Engine(0) as e:
        _reach(e, A)
        check(oracle, e, A)
        e.set_frame(B.source)  # the ranges fit the new frame, the 64² domain grid does not
        _refused(e, A, "domains outside the shrunk frame")
        e.set_domains(B.doms)
        e.run()
        check(oracle, e, B)


def test_ranges_of_two_sizes(oracle):
    base = CS.state("base")
    with F.Engine(0) as e:
        _reach(e, base)
        e.set_ranges(np.concatenate([base.rngs[:10], CS.grid(64, 64, 4, 4)[:54]]))
        _refused(e, base, "ranges of two sizes")
        e.set_ranges(base.rngs)
        e.run()
        check(oracle, e, base)


def test_domains_no_wider_than_the_ranges(oracle):
    base = CS.state("base")
    with F.Engine(0) as e:
        _reach(e, base)
        e.set_domains(CS.grid(64, 64, 8, 8))
        _refused(e, base, "domains as wide as the ranges")
        e.set_domains(base.doms)
        e.run()
        check(oracle, e, base)


# ---- frame sizes through the streaming calls --------------------------------------------------------------------

def _stream_states():
    big2 = _variant("frame_264x248_b", "frame_264x248", source=np.ascontiguousarray(CS.state("frame_264x248").source[::-1]))
    return [CS.state("base"), CS.state("frame_264x248"), CS.state("frame_70x58"), big2]


@pytest.mark.parametrize("fetch_between", [False, True], ids=["runs_only", "fetch_between"])
@pytest.mark.parametrize("route", ["set_frame_async", "set_frame_device_async"])
def test_frame_sizes_through_the_streaming_calls(oracle, route, fetch_between):
    """64×64 → 264×248 → 70×58 → 264×248 on one context: the second plane buffer and every prepared buffer grow
    under work in flight, then serve a smaller frame; each frame's tuples (a pinned sink) and the last frame's
    records equal a synchronous fresh search of that frame."""
    import torch

    states = _stream_states()
    want = [exp(oracle, s) for s in states]
    hosts = [torch.from_numpy(s.source.copy()).pin_memory() for s in states]
    planes = hosts if route == "set_frame_async" else [h.to("cuda:0") for h in hosts]
    sinks = [torch.zeros(max(len(s.rngs), 1) * 32, dtype=torch.uint8).pin_memory() for s in states]
    torch.cuda.synchronize()
    with F.Engine(0) as e:
        for k, s in enumerate(states):
            getattr(e, route)(planes[k])
            e.set_domains(s.doms)
            e.set_ranges(s.rngs)
            e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
            if fetch_between:
                check(oracle, e, s, f"frame {k}: ")
        e.set_tuple_sink(None)
        check(oracle, e, states[-1], "last frame: ")
    for k, s in enumerate(states):
        assert sinks[k].numpy()[:len(s.rngs) * 32].tobytes() == want[k][1], f"frame {k} ({s.name}): sink tuples"


# ---- host row strides -------------------------------------------------------------------------------------------

def _pitch(w):
    return (w + 63) & ~63


def _strided(plane, stride):
    """The plane in rows of `stride` bytes, the padding filled with 0xAB."""
    buf = np.full((plane.shape[0], stride), 0xAB, np.uint8)
    buf[:, :plane.shape[1]] = plane
    return buf


STRIDES = {"pitch": _pitch, "w+1": lambda w: w + 1, "w+64": lambda w: w + 64}


@pytest.mark.parametrize("route", ["frac_set_frame", "frac_set_planes", "set_frame_async"])
@pytest.mark.parametrize("kind", list(STRIDES))
@pytest.mark.parametrize("w", [60, 64, 100])
def test_host_row_strides(oracle, w, kind, route):
    """The ABI's host row stride: a stride equal to the device pitch is one linear copy, any other a 2-D copy;
    the records equal those of the contiguous plane (and the oracle's), whatever lies in the padding."""
    import torch

    H = 40
    src = CS._plane(4400 + w, w, H, "noise")
    two = route == "frac_set_planes"
    st = dataclasses.replace(CS.state("base"), name=f"strided_{w}_{'two' if two else 'one'}", source=src,
                             target=CS._plane(4500 + w, w, H, "uniform") if two else None,
                             doms=CS.grid(w, H, 16, 8), rngs=CS.grid(w, H, 8, 8))
    stride = STRIDES[kind](w)
    # the target plane's stride is chosen independently of the source's
    tstride = STRIDES[{"pitch": "w+1", "w+1": "w+64", "w+64": "pitch"}[kind]](w)
    with F.Engine(0) as e:
        if route == "set_frame_async":
            host = torch.full((H, stride), 0xAB, dtype=torch.uint8).pin_memory()
            host[:, :w] = torch.from_numpy(src.copy())
            view = host[:, :w]
            assert view.stride(0) == stride
            e.set_frame_async(view)
        elif two:
            s, t = _strided(src, stride), _strided(st.target, tstride)
            e._check(F.lib().frac_set_planes(e._ctx, s.ctypes.data, w, H, stride, t.ctypes.data, w, H, tstride))
        else:
            s = _strided(src, stride)
            e._check(F.lib().frac_set_frame(e._ctx, s.ctypes.data, w, H, stride))
        e.set_domains(st.doms)
        e.set_ranges(st.rngs)
        e.run()
        check(oracle, e, st, f"stride {stride}: ")


# ---- classify on the target plane -------------------------------------------------------------------------------

def test_classify_on_the_target_plane(oracle):
    d = CS.state("distinct_planes")
    with F.Engine(0) as e:
        e.set_planes(d.source, d.target)
        got_t = e.classify(d.rngs, target_plane=True)
        got_s = e.classify(d.doms, target_plane=False)
        np.testing.assert_array_equal(got_t["category"], oracle.classify(d.target, d.rngs)["category"])
        np.testing.assert_array_equal(got_s["category"], oracle.classify(d.source, d.doms)["category"])
        # the target's categories are not the source's at the same positions
        assert (got_t["category"] != oracle.classify(d.source, d.rngs)["category"]).any()
        # one plane: the target plane is the source plane
        b = CS.state("base")
        e.set_frame(b.source)
        want = oracle.classify(b.source, b.rngs)["category"]
        np.testing.assert_array_equal(e.classify(b.rngs, target_plane=True)["category"], want)
        np.testing.assert_array_equal(e.classify(b.rngs, target_plane=False)["category"], want)
