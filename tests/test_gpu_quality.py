"""Decoded quality on the device: Engine.decode_error, rate_errors, rate_quality and encode_quadtree_to_psnr.

The checker of an error is quality_ref.sse (numpy int64) over the plane Engine.decode_frq1 / decode_frc1 returns
for the same stream (pinned to the oracle's decoder by test_gpu_frq1.py and test_gpu_frc1_decode.py, and once
more here) and the frame as the test made it; the checker of the fit is quality_ref.bisect over the host's list
of such errors.  Every comparison is exact: sums, block maps, sizes, counts, the split distance with == on the
double."""
import math

import numpy as np
import pytest

import fractencode_amd as F
import frq1_synth as S
import quadtree_frames as Q
import quadtree_rate_ref as R
import quality_ref as QR
from frc1_synth import synth_stream

pytestmark = pytest.mark.gpu

ENGINES = [F.ENGINE_AUTO, F.ENGINE_VALU]
ENGINE_IDS = {F.ENGINE_AUTO: "auto", F.ENGINE_VALU: "valu"}
FRQ1_CASES = [Q.BY_NAME[n] for n in ("m98x74_16_4", "m130x66_8_2", "m70x58_16_2", "d31x31_16_4", "d20x20_16_16",
                                     "z15x15", "p98x74_two")]
# (W, H, range side): 8 × 8 ranges with margins (covered 64 × 56), 12-pixel ranges (g no power of two, 48 × 36)
FRC1_CASES = [(70, 58, 8), (50, 38, 12)]
FIT_CASES = [Q.BY_NAME[n] for n in ("m98x74_16_4", "m70x58_16_4")]


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


def _frame(case):
    src, tgt = case.planes()
    return src if tgt is None else tgt


def _same_error(got, plane_it_rms, frame, g):
    """decode_error's dict against the host's sums over a decoder's (plane, iterations, rms)."""
    plane, it, rms = plane_it_rms
    total, blocks = QR.sse(plane, frame, g)
    cw, ch = QR.covered(frame.shape[1], frame.shape[0], g)
    assert (got["sse"], got["pixels"], got["iterations"], got["rms"]) == (total, cw * ch, it, rms)
    assert got["psnr"] == (math.inf if total == 0 else 10.0 * math.log10(255.0 ** 2 * cw * ch / total))
    if "block_sse" in got:
        assert got["block_sse"].dtype == np.uint64 and got["block_sse"].shape == blocks.shape
        np.testing.assert_array_equal(got["block_sse"], blocks.astype(np.uint64))


# --- 1. decode_error against the decoded plane ------------------------------------------------------

@pytest.mark.parametrize("case", FRQ1_CASES, ids=_ids)
def test_error_of_a_quadtree_stream(oracle, case):
    frame = _frame(case)
    with _engine(case) as e:
        _set(e, case)
        stream, _ = e.encode_quadtree_stream(case.max_size, case.min_size, case.split)
        for m in (-1, 0, 1):
            got = e.decode_error(stream, max_iter=m, blocks=True)
            _same_error(got, e.decode_frq1(stream, max_iter=m), frame, case.max_size)
            plain = e.decode_error(stream, max_iter=m)
            assert "block_sse" not in plain and plain == {k: v for k, v in got.items() if k != "block_sse"}
        # no iteration: the zero plane against the frame
        cw, ch = QR.covered(case.W, case.H, case.max_size)
        assert e.decode_error(stream, max_iter=0)["sse"] == int((frame[:ch, :cw].astype(np.int64) ** 2).sum())
        if case.name == "m98x74_16_4":  # the reference does not rest on the device decoder alone
            _same_error(e.decode_error(stream, blocks=True), S.oracle_decode_quadtree_stream(oracle, stream), frame,
                        case.max_size)
            assert (cw, ch) == (96, 64) and got["block_sse"].shape == (4, 6)
        if case.name == "z15x15":
            assert (got["sse"], got["pixels"], got["psnr"]) == (0, 0, np.inf) and got["block_sse"].shape == (0, 0)
        if case.name == "d20x20_16_16":  # one leaf, without a domain: its pixels stay zero and are counted
            assert got["pixels"] == 256 and got["sse"] == int((frame[:16, :16].astype(np.int64) ** 2).sum())


def test_error_of_a_two_plane_stream_is_against_the_target():
    case = Q.BY_NAME["p98x74_two"]
    src, tgt = case.planes()
    with _engine(case) as e:
        _set(e, case)
        stream, _ = e.encode_quadtree_stream(case.max_size, case.min_size, case.split)
        plane = e.decode_frq1(stream)[0]
        got = e.decode_error(stream)["sse"]
        assert got == QR.sse(plane, tgt, 16)[0] != QR.sse(plane, src, 16)[0]


@pytest.mark.parametrize("W,H,n", FRC1_CASES, ids=lambda v: str(v))
def test_error_of_a_uniform_stream(W, H, n):
    frame = Q.mixed(W, H)
    stream = synth_stream(W, H, n, 2 * n, 8, 300 + n)
    with F.Engine(0, 8) as e:
        e.set_frame(frame)
        for m in (-1, 0, 1):
            _same_error(e.decode_error(stream, max_iter=m, blocks=True), e.decode_frc1(stream, max_iter=m), frame, n)
        got = e.decode_error(stream, blocks=True)
        assert got["pixels"] == (W - W % n) * (H - H % n) and got["block_sse"].shape == (H // n, W // n)
        assert got["sse"] > 0


def test_block_capacity_and_null_outputs():
    import ctypes as C

    case = Q.BY_NAME["m98x74_16_4"]
    with _engine(case) as e:
        _set(e, case)
        stream, _ = e.encode_quadtree_stream(case.max_size, case.min_size, case.split)
        want = e.decode_error(stream, blocks=True)
        buf = np.frombuffer(stream, np.uint8)
        short = np.full(24 + 3, 0xFFFFFFFFFFFFFFFF, np.uint64)
        nb, sse = C.c_size_t(0), C.c_uint64(0)
        e._check(F.lib().frac_decode_error(e._ctx, buf.ctypes.data, len(buf), -1, 1e-5, C.byref(sse), None,
                                           short.ctypes.data, 10, C.byref(nb), None, None))
        assert nb.value == 24 and sse.value == want["sse"]  # the count is the rectangle's, whatever the capacity
        np.testing.assert_array_equal(short[:10], want["block_sse"].reshape(-1)[:10])
        assert (short[10:] == 0xFFFFFFFFFFFFFFFF).all()  # nothing past the capacity
        e._check(F.lib().frac_decode_error(e._ctx, buf.ctypes.data, len(buf), -1, 1e-5, None, None, None, 0, None,
                                           None, None))


# --- 2. the frame compared is the current one ---------------------------------------------------------

def test_the_frame_is_the_one_the_next_run_would_search():
    import torch

    W, H = 98, 74
    A, B, Cf = Q.mixed(W, H), Q.mixed(W, H, Q.TGT_SEED), Q.mixed(W, H, 13)
    stream = S.synth_quadtree_stream(W, H, 61, T=4)
    with F.Engine(0, 4) as e:
        with pytest.raises(F.FracError, match="rc=-3"):  # no frame
            e.decode_error(stream)
        e.set_frame(A)
        plane = e.decode_frq1(stream)[0]
        want = {k: QR.sse(plane, f, 16)[0] for k, f in (("A", A), ("B", B), ("C", Cf))}
        assert len(set(want.values())) == 3
        assert e.decode_error(stream)["sse"] == want["A"]
        e.set_domains(F.create_uniform_grid(W, H, 16, 8))
        e.set_ranges(F.create_uniform_grid(W, H, 8, 8))
        e.run()
        e.set_frame(B)  # a frame after one of its geometry: uploaded into the spare plane, the buffers swap
        assert F.debug_frame_upload(e)["copy_stream"]
        assert e.decode_error(stream)["sse"] == want["B"]
        e.run()
        pinned = torch.from_numpy(Cf.copy()).pin_memory()
        e.set_frame_async(pinned)  # not waited for: the comparison is ordered behind the copy
        assert e.decode_error(stream)["sse"] == want["C"]
        assert e.decode_error(stream)["sse"] == want["C"]
        # a stream of another geometry
        for other in (S.synth_quadtree_stream(W, H - 1, 62, T=4), S.synth_quadtree_stream(W + 16, H, 63, T=4),
                      synth_stream(96, 74, 8, 16, 4, 64)):
            with pytest.raises(F.FracError, match="rc=-1.*frame"):
                e.decode_error(other)
        with pytest.raises(F.FracError, match="rc=-1"):
            e.decode_error(b"FRC9" + stream[4:])
        with pytest.raises(F.FracError, match="rc=-1"):
            e.decode_error(stream[:-4])
        assert e.decode_error(stream)["sse"] == want["C"]  # the refusals left everything as it was


# --- 3. rate_errors ---------------------------------------------------------------------------------

def _probes(case, tree):
    c = tree.candidates()
    picked = c if case.name == R.FULL.name else R.spread(c, 9)
    return np.concatenate([picked, [-1.0, np.inf]])


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", [Q.BY_NAME["m98x74_16_4"], Q.BY_NAME["m70x58_16_4"], Q.TILE_CARRY], ids=_ids)
def test_rate_errors_equal_decode_error_of_rate_stream(oracle, case, engine):
    tree = R.tree(oracle, case)
    ts = _probes(case, tree)
    assert len(ts) == (115 if case.name == R.FULL.name else 11)
    with _engine(case, engine) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        sse, size, it = e.rate_errors(ts)
        assert (sse.dtype, size.dtype, it.dtype) == (np.uint64, np.uint64, np.int32)
        for i, t in enumerate(ts):
            stream = e.rate_stream(float(t))
            want = e.decode_error(stream)
            assert (int(sse[i]), int(size[i]), int(it[i])) == (want["sse"], len(stream), want["iterations"]), \
                (case.name, t)
        assert sse[-2] == sse[0] and size[-2] == size[0]  # below every candidate: the partition at 0.0 ...
        assert size[-1] == tree.size(np.inf)[0]           # ... and nothing splits at +inf
        # other widths, a bounded decode, NULL outputs, no threshold
        s22, z22, _ = e.rate_errors(ts[:3], 2, 2, max_iter=2)
        for i in range(3):
            stream = e.rate_stream(float(ts[i]), 2, 2)
            assert (int(s22[i]), int(z22[i])) == (e.decode_error(stream, max_iter=2)["sse"], len(stream))
        e._check(F.lib().frac_quadtree_rate_errors(e._ctx, 5, 7, ts.ctypes.data, 2, -1, 1e-5, None, None, None))
        assert [a.shape for a in e.rate_errors([])] == [(0,)] * 3


# --- 4. rate_quality --------------------------------------------------------------------------------

def _errors_of(case, cands):
    """E(i) of the candidates on the host: quality_ref.sse of decode_frq1(rate_stream(c[i]))."""
    frame = _frame(case)
    with _engine(case) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        return [QR.sse(e.decode_frq1(e.rate_stream(float(t)))[0], frame, case.max_size)[0] for t in cands]


_E = {}


def _E_list(oracle, case):
    if case.name not in _E:
        _E[case.name] = tuple(_errors_of(case, R.tree(oracle, case).candidates()))
    return _E[case.name]


def _targets(E):
    s = sorted(E)
    q = [s[len(s) * k // 4] for k in (1, 2, 3)]
    return [E[-1], E[-1] - 1, E[0], min(E) - 1, E[0] - 1] + q + [v - 1 for v in q]


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", FIT_CASES, ids=_ids)
def test_rate_quality_is_the_stated_bisection(oracle, case, engine):
    tree = R.tree(oracle, case)
    cands = tree.candidates()
    E = _E_list(oracle, case)
    m = len(E)
    assert len(set(E)) == m and list(E) != sorted(E)  # distinct, not monotone: the rule shows
    assert QR.bisect(E, E[-1]) == (m - 1, 1)
    assert QR.bisect(E, min(E) - 1)[0] is None and QR.bisect(E, E[0] - 1)[0] is None
    with _engine(case, engine) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        for target in _targets(E):
            idx, probes = QR.bisect(E, target)
            if idx is None:
                with pytest.raises(F.FracError, match=f"rc=-1.*smallest split distance, {E[0]},"):
                    e.rate_quality(max_sse=target)
                continue
            size, leaves, _ = tree.size(float(cands[idx]))
            got = e.rate_quality(max_sse=target)
            assert got == (float(cands[idx]), size, leaves, E[idx], probes), (case.name, target)
            assert E[idx] <= target and (idx == m - 1 or E[idx + 1] > target)  # the guarantee
        # a PSNR target: the same rule at the translated bound
        pixels = QR.covered(case.W, case.H, case.max_size)[0] * QR.covered(case.W, case.H, case.max_size)[1]
        mid = sorted(E)[m // 2]
        psnr = float(np.floor(10.0 * np.log10(255.0 ** 2 * pixels / mid)))
        idx, probes = QR.bisect(E, QR.max_sse_of(psnr, pixels))
        got = e.rate_quality(min_psnr=psnr)
        assert got[0] == float(cands[idx]) and got[3] == E[idx] and got[4] == probes
        assert 10.0 * np.log10(255.0 ** 2 * pixels / got[3]) >= psnr
        with pytest.raises(ValueError):
            e.rate_quality()
        with pytest.raises(ValueError):
            e.rate_quality(max_sse=1, min_psnr=30.0)
        # NULL outputs
        e._check(F.lib().frac_quadtree_rate_quality(e._ctx, 5, 7, E[-1], -1, 1e-5, None, None, None, None, None))


def test_rate_quality_of_a_frame_without_ranges():
    case = Q.BY_NAME["z15x15"]
    with _engine(case) as e:
        _set(e, case)
        e.quadtree_rate(case.max_size, case.min_size)
        assert e.rate_quality(max_sse=0) == (0.0, 64, 0, 0, 1)
        assert e.rate_quality(min_psnr=99.0) == (0.0, 64, 0, 0, 1)
        sse, size, _ = e.rate_errors([0.0, 5.0])
        assert sse.tolist() == [0, 0] and size.tolist() == [64, 64]


# --- 5. state rules ---------------------------------------------------------------------------------

def test_the_quality_calls_are_readers(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    doms, rngs = F.create_uniform_grid(case.W, case.H, 16, 8), F.create_uniform_grid(case.W, case.H, 8, 8)
    stream = S.synth_quadtree_stream(case.W, case.H, 71, T=4)
    with _engine(case) as ref:  # a run nothing came between
        _set(ref, case)
        ref.set_domains(doms)
        ref.set_ranges(rngs)
        ref.run()
        want_items, want_stats = ref.fetch()
    with _engine(case) as e:
        _set(e, case)
        for call in (lambda: e.rate_errors([1.0]), lambda: e.rate_quality(max_sse=1 << 40)):
            with pytest.raises(F.FracError, match="rc=-3"):  # no rate state
                call()
        e.set_domains(doms)
        e.set_ranges(rngs)
        e.run()
        err = e.decode_error(stream)  # between run() and fetch()
        for call in (lambda: e.rate_errors([1.0]), lambda: e.rate_quality(max_sse=1 << 40)):
            with pytest.raises(F.FracError, match="rc=-3"):  # a run is no rate state; the refusal changes nothing
                call()
        items, stats = e.fetch()
        np.testing.assert_array_equal(items, want_items)
        assert stats["rejected_mappings"] == want_stats["rejected_mappings"]
        assert e.decode_error(stream) == err
        np.testing.assert_array_equal(e.fetch()[0], want_items)
        # with a rate state: the other readers answer as before
        e.quadtree_rate(case.max_size, case.min_size)
        ts = R.spread(R.tree(oracle, case).candidates(), 5)
        before = (e.rate_sizes(ts), e.rate_leaves(float(ts[2])), e.rate_fit(1 << 20))
        errs = e.rate_errors(ts)
        quality = e.rate_quality(max_sse=int(errs[0].max()))
        e.decode_error(stream)
        for a, b in zip(before[0], e.rate_sizes(ts)):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(before[1], e.rate_leaves(float(ts[2])))
        assert before[2] == e.rate_fit(1 << 20)
        for a, b in zip(errs, e.rate_errors(ts)):
            np.testing.assert_array_equal(a, b)
        assert e.rate_quality(max_sse=int(errs[0].max())) == quality
        for bits in ((1, 7), (5, 17)):  # widths outside [2, 16]
            with pytest.raises(F.FracError, match="rc=-1"):
                e.rate_errors(ts, *bits)
            with pytest.raises(F.FracError, match="rc=-1"):
                e.rate_quality(max_sse=1 << 40, contrast_bits=bits[0], brightness_bits=bits[1])
        e.set_frame(_frame(case))  # a setter ends the rate state for these readers too
        for call in (lambda: e.rate_errors([1.0]), lambda: e.rate_quality(max_sse=1 << 40)):
            with pytest.raises(F.FracError, match="rc=-3"):
                call()


# --- 6. one call from a PSNR to a stream ---------------------------------------------------------------

@pytest.mark.parametrize("case", FIT_CASES, ids=_ids)
def test_encode_quadtree_to_psnr(oracle, case):
    E = _E_list(oracle, case)
    pixels = QR.covered(case.W, case.H, case.max_size)[0] * QR.covered(case.W, case.H, case.max_size)[1]
    psnr = float(np.floor(10.0 * np.log10(255.0 ** 2 * pixels / sorted(E)[len(E) // 2])))
    with _engine(case) as e:
        _set(e, case)
        stream, info = e.encode_quadtree_to_psnr(psnr, case.max_size, case.min_size)
        assert stream == e.rate_stream(info["split_distance"])
        err = e.decode_error(stream)
        assert err["sse"] == info["sse"] and err["pixels"] == info["pixels"] == pixels
        assert info["psnr"] == err["psnr"] >= psnr
        assert info["bytes"] == len(stream) and info["items"] == F.frq1_info(stream)["n_leaves"]
        idx, probes = QR.bisect(E, QR.max_sse_of(psnr, pixels))
        assert info["probes"] == probes and info["sse"] == E[idx]
        assert info["total_mappings"] > 0  # the search's stats ride along
