"""The fused n = 8 resolvers write each range's record and tuple as whole stores from several lanes
(fit_rstat_range_wave), and the sorted resolve walks the ranges in range order when the sink is host memory and in
slot order otherwise (kTpRangeOrder, launch_tp).  Every case
compares the sink's bytes with fetch_tuples() of the same run and the records with an ENGINE_VALU run of the same
inputs (another writer), with the sink inside a larger 0xAB buffer whose other bytes must stay untouched: odd
geometries, a sink that is only 8-byte aligned, partial grids (slot order ≠ range order, partial blocks), fp32-regime
and empty ranges, hit-format keys, T = 8's paired resolve, and two frames alternating into one sink."""
import os
import sys

import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
from golden_util import plane

pytestmark = pytest.mark.gpu

GUARD = 64
SEA, AUTO_PRUNE, AUTO_EXH = (F.ENGINE_SEA, 0), (F.ENGINE_AUTO, F.FLAG_PRUNE), (F.ENGINE_AUTO, F.FLAG_EXHAUSTIVE)

_valu = {}


def _fallback_frame():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from fallback_probe import frame

    return frame(6, 512)


_frames = {
    "mosaic256": lambda: A.mosaic(256, 256, amp=2),
    "mosaic264": lambda: A.mosaic(264, 248, amp=2),
    "mosaic256b": lambda: A.mosaic(256, 256, amp=3, noise_seed=99),
    "fallback512": _fallback_frame,
    "lenna": lambda: plane("lenna_y"),
}
_planes = {}


def _plane(name):
    if name not in _planes:
        _planes[name] = _frames[name]()
    return _planes[name]


def _grids(p, sel=None):
    H, W = p.shape
    rngs = F.create_uniform_grid(W, H, 8, 8)
    if sel is not None:
        rngs = np.ascontiguousarray(rngs[sel])
    return F.create_uniform_grid(W, H, 16, 8), rngs


def _reference(name, sel_key=None, sel=None, T=4, cls=False, thr=0.0):
    """The ENGINE_VALU records and stats of a case, computed once."""
    key = (name, sel_key, T, cls, thr)
    if key not in _valu:
        p = _plane(name)
        doms, rngs = _grids(p, sel)
        with F.Engine(0, T, cls, thr, -1.0, F.ENGINE_VALU) as e:
            e.set_frame(p)
            e.set_domains(doms)
            _valu[key] = e.search(rngs)
    return _valu[key]


class Sink:
    """nr tuples at `offset` bytes into a 0xAB buffer with GUARD bytes (and more) on either side."""

    def __init__(self, nr, where, offset=0):
        import torch

        self.n, self.at = nr * F.TUPLE.itemsize, GUARD + offset
        total = self.at + self.n + GUARD + 64
        self.buf = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda:0") if where == "device" else \
            torch.full((total,), 0xAB, dtype=torch.uint8).pin_memory()
        assert self.buf.data_ptr() % 64 == 0
        self.ptr = self.buf.data_ptr() + self.at

    def run(self, e):
        import torch

        e.set_tuple_sink(self.ptr)
        e.run()
        e.set_tuple_sink(None)
        e.sync()
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert bool((b[:self.at] == 0xAB).all()), "bytes before the sink were written"
        assert bool((b[self.at + self.n:] == 0xAB).all()), "bytes after the sink were written"
        return b[self.at:self.at + self.n].tobytes()


def _check(name, route, where, offset=0, sel_key=None, sel=None, T=4, cls=False, thr=0.0):
    engine, flags = route
    p = _plane(name)
    doms, rngs = _grids(p, sel)
    want, wst = _reference(name, sel_key, sel, T, cls, thr)
    with F.Engine(0, T, cls, thr, -1.0, engine, flags=flags) as e:
        e.set_frame(p)
        e.set_domains(doms)
        e.set_ranges(rngs)
        got = Sink(len(rngs), where, offset).run(e)
        out, st = e.fetch()
        tuples = e.fetch_tuples()
    print(f"{name} {route} {where} +{offset} {sel_key}: form {st['search_form']}, fallback {st['fallback_ranges']}, "
          f"hits {st['hit_ranges']}, empty {int((tuples['domain'] == F.NO_DOMAIN).sum())}")
    assert got == tuples.tobytes()
    assert out.tobytes() == want.tobytes()
    assert (st["hit_ranges"], st["fallback_ranges"]) == (wst["hit_ranges"], wst["fallback_ranges"])
    return st, tuples


# ---- 1: the sorted route at odd geometries ---------------------------------------------------------------------

@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("route", [SEA, AUTO_PRUNE], ids=["sea", "auto_prune"])
@pytest.mark.parametrize("name", ["mosaic256", "mosaic264"])
def test_sorted_route(name, route, where):
    st, _ = _check(name, route, where)
    if route is SEA:
        assert st["search_form"] == F.FORM_SEA_MFMA


# ---- 2: a sink that is only 8-byte aligned: every tuple straddles a 64-byte line ---------------------------------

@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("route", [SEA, AUTO_EXH], ids=["sorted", "exhaustive"])
def test_misaligned_sink(route, where):
    st, _ = _check("mosaic264", route, where, offset=8)
    assert (st["search_form"] == F.FORM_SEA_MFMA) == (route is SEA)


# ---- 3: partial grids: slot order and range order differ, blocks are partial ------------------------------------

_SLICES = {"first1021": slice(0, 1021), "every_third": slice(0, None, 3), "one": slice(0, 1), "three": slice(0, 3),
           "thirty_three": slice(0, 33)}


@pytest.mark.parametrize("sel_key", list(_SLICES))
def test_partial_grids(sel_key):
    st, _ = _check("mosaic256", SEA, "pinned", sel_key=sel_key, sel=_SLICES[sel_key])
    assert st["search_form"] == F.FORM_SEA_MFMA


# ---- 4: fp32-regime ranges (fallback_grid writes them later), empty ranges and ordinary ones in one run ------------

@pytest.mark.parametrize("cls", [False, True], ids=["plain", "classifier"])
def test_every_kind_of_outcome(cls):
    st, tuples = _check("fallback512", SEA, "pinned", cls=cls)
    if not cls:
        assert st["fallback_ranges"] > 0


# ---- 5: hit-format keys -------------------------------------------------------------------------------------------

def test_hit_format_keys_on_the_sorted_route():
    st, _ = _check("mosaic264", SEA, "pinned", thr=2.0)
    assert st["search_form"] == F.FORM_SEA_MFMA
    assert st["hit_ranges"] > 0


# ---- 6: T = 8's paired resolve --------------------------------------------------------------------------------------

def test_paired_resolve_t8():
    st, _ = _check("lenna", (F.ENGINE_MFMA, 0), "pinned", T=8)
    assert st["search_form"] == F.FORM_FOURIER


# ---- 7: two frames alternately into one sink on one context -----------------------------------------------------------

def test_alternating_frames_into_one_sink():
    names = ["mosaic256", "mosaic256b"]
    doms, rngs = _grids(_plane(names[0]))
    sink = Sink(len(rngs), "pinned")
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_SEA) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        seen = []
        for k in range(4):
            name = names[k & 1]
            e.set_frame(_plane(name))
            got = sink.run(e)
            out, st = e.fetch()
            assert st["search_form"] == F.FORM_SEA_MFMA
            assert got == e.fetch_tuples().tobytes()
            assert out.tobytes() == _reference(name)[0].tobytes()
            seen.append(got)
    assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0] != seen[1]


def test_sink_kinds_in_turn_on_one_context():
    """The sorted resolve walks in range order for a host sink and in slot order otherwise: device, pinned, device
    and no sink in turn on one context give the same tuples and records."""
    name = "mosaic264"
    doms, rngs = _grids(_plane(name))
    want = _reference(name)[0].tobytes()
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_SEA) as e:
        e.set_frame(_plane(name))
        e.set_domains(doms)
        e.set_ranges(rngs)
        seen = []
        for where in ("device", "pinned", "device"):
            got = Sink(len(rngs), where, offset=8).run(e)
            out, st = e.fetch()
            assert st["search_form"] == F.FORM_SEA_MFMA
            assert got == e.fetch_tuples().tobytes() and out.tobytes() == want
            seen.append(got)
        e.run()
        out, _ = e.fetch()
        assert out.tobytes() == want and e.fetch_tuples().tobytes() == seen[0]
    assert seen[0] == seen[1] == seen[2]
