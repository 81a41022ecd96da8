"""Blocking frame uploads that overlap the previous run (frac_set_frame / frac_set_planes after a frame of the
same geometry: the copy goes into the plane's twin on the context's copy stream, the host waits for the copy
alone, the buffers swap).  Frames go through one context back to back, with no sync or fetch in between, on the
pruned route, the exhaustive MFMA engine and the VALU engine; every frame's records, tuples and stats equal,
byte for byte, those of a fresh context that searched that frame alone."""
import os
import sys

import numpy as np
import pytest

import fractencode_amd as F
from fractencode_amd.synth import value_noise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

ROUTES = {"prune": (F.ENGINE_AUTO, F.FLAG_PRUNE), "mfma": (F.ENGINE_MFMA, 0), "valu": (F.ENGINE_VALU, 0)}
route = pytest.mark.parametrize("route", list(ROUTES))


def engine(route, cls=False):
    eng, flags = ROUTES[route]
    return F.Engine(0, 4, cls, 0.0, -1.0, eng, False, flags)


_GRIDS = {}


def grids(S):
    if S not in _GRIDS:
        _GRIDS[S] = (F.create_uniform_grid(S, S, 16, 8), F.create_uniform_grid(S, S, 8, 8))
    return _GRIDS[S]


_FRAMES = {}


def frames64():
    """Six distinct 64×64 frames: the crop, its flips and its transposes."""
    if 64 not in _FRAMES:
        p = np.fromfile(os.path.join(HERE, "golden", "crop64.u8"), dtype=np.uint8).reshape(64, 64)
        _FRAMES[64] = [np.ascontiguousarray(q) for q in (p, p[::-1], p[:, ::-1], p[::-1, ::-1], p.T, p.T[::-1])]
    return _FRAMES[64]


def frames96():
    """Three ordinary 96×96 frames (value noise)."""
    if 96 not in _FRAMES:
        _FRAMES[96] = [value_noise(96, 96, 1234 + k) for k in range(3)]
    return _FRAMES[96]


def fp32_frames():
    """Three 96×96 frames with isolated white ranges in black patches: the fp32 regime (tools/fallback_probe.py)."""
    if "fp32" not in _FRAMES:
        from fallback_probe import frame

        _FRAMES["fp32"] = [frame(k, 96) for k in (3, 5, 8)]
    return _FRAMES["fp32"]


_WANT = {}


def fresh(route, p, cls=False, tgt=None):
    """(records, tuples, stats) of a fresh context that searched the frame (or the plane pair) alone: computed
    once per route and frame, and never changed."""
    key = (route, cls, p.shape, p.tobytes(), None if tgt is None else tgt.tobytes())
    if key not in _WANT:
        doms, rngs = grids(p.shape[0])
        with engine(route, cls) as e:
            if tgt is None:
                e.set_frame(p.copy())
            else:
                e.set_planes(p.copy(), tgt.copy())
            e.set_domains(doms)
            out, st = e.search(rngs)
            _WANT[key] = (out.tobytes(), e.fetch_tuples().tobytes(), st)
    return _WANT[key]


def pinned_sinks(n, nr):
    import torch

    return [torch.zeros(nr * F.TUPLE.itemsize, dtype=torch.uint8).pin_memory() for _ in range(n)]


def check_sinks(route, sinks, frames, cls=False):
    for k, (s, p) in enumerate(zip(sinks, frames)):
        assert s.cpu().numpy().tobytes() == fresh(route, p, cls)[1], f"frame {k}: tuples"


def check_last(route, e, p, cls=False, tgt=None):
    out, st = e.fetch()
    want = fresh(route, p, cls, tgt)
    assert out.tobytes() == want[0], "records"
    assert st == want[2], "stats"
    assert e.fetch_tuples().tobytes() == want[1], "tuples"


@route
@pytest.mark.parametrize("sink", ["pinned", "device", "none"])
def test_back_to_back_frames(route, sink):
    """Six distinct frames through the blocking set_frame + run, nothing in between; each run's tuples into a
    sink of its own (pinned memory, device memory) or nowhere."""
    import torch

    frames = frames64()
    doms, rngs = grids(64)
    if sink == "pinned":
        sinks = pinned_sinks(len(frames), len(rngs))
    elif sink == "device":
        sinks = [torch.zeros(len(rngs) * F.TUPLE.itemsize, dtype=torch.uint8, device="cuda:0") for _ in frames]
        torch.cuda.synchronize()
    else:
        sinks = []
    with engine(route) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, p in enumerate(frames):
            e.set_frame(p)
            if sinks:
                e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, frames[-1])
        check_sinks(route, sinks, frames)
        assert F.debug_frame_upload(e)["copy_stream"]


@route
@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_host_plane_is_free_on_return(route, memory):
    """The caller's buffer is overwritten with 0xA5 as soon as set_frame has returned, before run(): the results
    are the original frame's, from pinned and from pageable memory."""
    import torch

    frames = frames64()[:4]
    doms, rngs = grids(64)
    sinks = pinned_sinks(len(frames), len(rngs))
    if memory == "pinned":
        keep = torch.zeros((64, 64), dtype=torch.uint8).pin_memory()
        buf = keep.numpy()
    else:
        buf = np.zeros((64, 64), np.uint8)
    with engine(route) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, p in enumerate(frames):
            buf[:] = p
            e.set_frame(buf)
            buf[:] = 0xA5
            e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, frames[-1])
        check_sinks(route, sinks, frames)


@route
@pytest.mark.parametrize("sink", ["pinned", "none"])
def test_fp32_fallback_in_flight(route, sink):
    """fp32-regime frames between ordinary ones, three of them in a row: a plane buffer is written again while
    the deferred fallback_grid of two frames back has only just been settled.  Without a sink the fallback of
    every run is still pending when the next frame arrives."""
    n, f = frames96(), fp32_frames()
    for p in f:
        assert fresh(route, p)[2]["fallback_ranges"] > 0
    frames = [n[0], f[0], f[1], f[2], n[1], f[0], n[2], f[1]]
    doms, rngs = grids(96)
    sinks = pinned_sinks(len(frames), len(rngs)) if sink == "pinned" else []
    with engine(route) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, p in enumerate(frames):
            e.set_frame(p)
            if sinks:
                e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, frames[-1])
        check_sinks(route, sinks, frames)
        e.set_frame(n[0])  # with the last run's fallback settled by the fetch, and once more pending
        e.run()
        e.set_frame(f[2])
        e.run()
        check_last(route, e, f[2])


@route
def test_mixed_entry_points(route):
    """set_frame, set_frame_async, set_frame(device tensor) and set_frame_device_async interleaved on one context
    (sync → async → sync and device → sync among them)."""
    import torch

    f = frames64()
    order = [("sync", 0), ("async", 1), ("sync", 2), ("device", 3), ("sync", 4), ("device_async", 5), ("async", 0),
             ("async", 2), ("sync", 1), ("device_async", 3), ("sync", 5)]
    hosts = [torch.from_numpy(p.copy()).pin_memory() for p in f]
    devs = [torch.from_numpy(p).to("cuda:0") for p in f]
    torch.cuda.synchronize()
    doms, rngs = grids(64)
    sinks = pinned_sinks(len(order), len(rngs))
    with engine(route) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, (how, i) in enumerate(order):
            if how == "sync":
                e.set_frame(f[i])
            elif how == "async":
                e.set_frame_async(hosts[i])
            elif how == "device":
                e.set_frame(devs[i])
            else:
                e.set_frame_device_async(devs[i])
            e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, f[order[-1][1]])
        check_sinks(route, sinks, [f[i] for _, i in order])


@route
def test_geometry_change_with_work_in_flight(route):
    """64×64 → 96×96 → 64×64, two frames each, no sync between a run and the next set_frame: the first frame of
    a geometry goes into the current buffer, the twin is reallocated with both streams idle."""
    f64, f96 = frames64(), frames96()
    frames = [f64[0], f64[1], f96[0], f96[1], f64[2], f64[3], f64[4]]
    sinks = [pinned_sinks(1, len(grids(p.shape[0])[1]))[0] for p in frames]
    with engine(route) as e:
        size = 0
        for k, p in enumerate(frames):
            e.set_frame(p)
            if p.shape[0] != size:
                size = p.shape[0]
                e.set_domains(grids(size)[0])
                e.set_ranges(grids(size)[1])
            e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, frames[-1])
        check_sinks(route, sinks, frames)


@route
def test_classifier_on(route):
    """The classifier on: every frame re-prepares on the host.  Three frames back to back."""
    frames = frames64()[1:4]
    doms, rngs = grids(64)
    sinks = pinned_sinks(len(frames), len(rngs))
    with engine(route, True) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, p in enumerate(frames):
            e.set_frame(p)
            e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, frames[-1], True)
        check_sinks(route, sinks, frames, True)


@route
def test_set_planes_with_a_distinct_target(route):
    """Three (source, target) pairs back to back through set_planes, then a frame through set_frame."""
    f = frames64()
    pairs = [(f[0], f[1]), (f[2], f[3]), (f[4], f[0])]
    doms, rngs = grids(64)
    sinks = pinned_sinks(len(pairs), len(rngs))
    with engine(route) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, (s, t) in enumerate(pairs):
            e.set_planes(s, t)
            e.set_tuple_sink(sinks[k].data_ptr())
            e.run()
        e.set_tuple_sink(None)
        check_last(route, e, pairs[-1][0], tgt=pairs[-1][1])
        for k, (s, t) in enumerate(pairs):
            assert sinks[k].numpy().tobytes() == fresh(route, s, tgt=t)[1], f"pair {k}: tuples"
        e.set_frame(f[5])
        e.run()
        check_last(route, e, f[5])


@route
def test_stream_switch(route):
    """set_frame; run; set_stream(other); set_frame; run; fetch: the second frame's upload and run are ordered
    behind the first run, whose tuples are the first frame's."""
    import torch

    f = frames64()
    doms, rngs = grids(64)
    sinks = pinned_sinks(3, len(rngs))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with engine(route) as e:
        e.set_stream(s1.cuda_stream)
        e.set_domains(doms)
        e.set_ranges(rngs)
        e.set_frame(f[0])
        e.set_tuple_sink(sinks[0].data_ptr())
        e.run()
        e.set_frame(f[1])
        e.set_tuple_sink(sinks[1].data_ptr())
        e.run()
        e.set_stream(s2.cuda_stream)
        e.set_frame(f[2])
        e.set_tuple_sink(sinks[2].data_ptr())
        e.run()
        e.set_tuple_sink(None)
        check_last(route, e, f[2])
        s1.synchronize()
        check_sinks(route, sinks, f[:3])


@route
def test_engine_closed_after_set_frame_with_a_run_in_flight(route):
    """An engine closed right after set_frame returned, the previous run still in flight: the context goes idle on
    both of its streams before anything is released, and a second engine on the device searches the crop as a
    fresh context does."""
    f = frames64()
    doms, rngs = grids(64)
    for k in range(4):
        first = engine(route)
        first.set_domains(doms)
        first.set_ranges(rngs)
        first.set_frame(f[k])
        first.run()
        first.set_frame(f[k + 1])
        if k & 1:
            first.run()
            first.set_frame(f[k + 2])
        first.close()
        with engine(route) as second:
            second.set_frame(f[0])
            second.set_domains(doms)
            second.set_ranges(rngs)
            second.run()
            check_last(route, second, f[0])


def test_one_shot_allocates_no_twin():
    """A single set_frame on a fresh context, and the first frame of another geometry, allocate no second plane
    and create no copy stream; the first frame that follows one of its geometry does."""
    f64, f96 = frames64(), frames96()
    with engine("prune") as e:
        e.set_frame(f64[0])
        e.set_domains(grids(64)[0])
        e.search(grids(64)[1])
        assert F.debug_frame_upload(e) == {"twin_bytes": 0, "copy_stream": False}
        e.set_frame(f96[0])
        e.set_domains(grids(96)[0])
        e.search(grids(96)[1])
        assert F.debug_frame_upload(e) == {"twin_bytes": 0, "copy_stream": False}
        e.set_frame(f96[1])
        got = F.debug_frame_upload(e)
        assert got["copy_stream"] and got["twin_bytes"] >= 96 * 96
        e.set_ranges(grids(96)[1])
        e.run()
        check_last("prune", e, f96[1])
