"""Colour quality on the device: Engine.decode_error_frc3, Engine.rate_candidates and ColorEncoder's rate_* and
encode_quadtree_to_size / _to_psnr.

The checker of an error is color_quality_ref.channel_sse (numpy int64) over the RGB Engine.decode_frc3 returns for
the same container (pinned by test_gpu_frc3_decode.py, and once more here through yuv2rgb_ref over the three
single-plane decodes) and the `rgb` array the test made; the checker of the fits is color_quality_ref.fit_size and
quality_ref.bisect over the host's lists.  Every comparison is exact: sums, sizes, counts, the split distance with
== on the double."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import color_quality_ref as CR
import fractencode_amd as F
import quadtree_frames as Q
import quadtree_rate_ref as R
import quality_ref as QR
import yuv2rgb_ref as Y
from fractencode_amd.color import ColorEncoder
from frc1_synth import synth_stream
from frq1_synth import synth_quadtree_stream

pytestmark = pytest.mark.gpu

FIT_CASES = [Q.BY_NAME[n] for n in ("m98x74_16_4", "m70x58_16_4")]


@pytest.fixture(scope="module")
def eng():
    with F.Engine(0) as e:
        yield e


def frc1_planes(W, H, n, seed, T=4, **kw):
    """FRC1 plane streams of range side n (an int, or one per plane), domains of twice the side."""
    ny, nu, nv = (n, n, n) if np.isscalar(n) else n
    cw, ch = W // 2, H // 2
    return [synth_stream(W, H, ny, 2 * ny, T, seed, **kw), synth_stream(cw, ch, nu, 2 * nu, T, seed + 1, **kw),
            synth_stream(cw, ch, nv, 2 * nv, T, seed + 2, **kw)]


def frq1_planes(W, H, sizes, seed, T=4):
    cw, ch = W // 2, H // 2
    return [synth_quadtree_stream(W, H, seed, sizes, T=T), synth_quadtree_stream(cw, ch, seed + 1, sizes, T=T),
            synth_quadtree_stream(cw, ch, seed + 2, sizes, T=T)]


def _mixed_kinds():
    q, c = frq1_planes(96, 64, (16, 8, 4), 730), frc1_planes(96, 64, 8, 733, cmax=0.7)
    return [q[0], c[1], q[2]]


# name → (W, H, plane streams, (g_Y, g_U, g_V), the covered rectangle)
CASES = {
    "q96x64": (96, 64, lambda: frq1_planes(96, 64, (16, 8, 4), 700), (16, 16, 16), (96, 64)),
    "q98x74": (98, 74, lambda: frq1_planes(98, 74, (16, 8, 4), 710), (16, 16, 16), (96, 64)),
    "c37x27": (37, 27, lambda: frc1_planes(37, 27, 4, 720, cmax=0.7), (4, 4, 4), (32, 24)),
    "c38x28": (38, 28, lambda: frc1_planes(38, 28, (3, 7, 7), 725, cmax=0.7), (3, 7, 7), (28, 27)),
    "k96x64": (96, 64, _mixed_kinds, (16, 8, 16), (96, 64)),
    "c12x12": (12, 12, lambda: frc1_planes(12, 12, (4, 8, 8), 740), (4, 8, 8), (0, 0)),
}


def reference(W, H, seed):
    """The RGB frame a case is compared with: seeded noise (the streams are synthetic too)."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def want_error(e, s, rgb, g, **kw):
    """decode_error_frc3's dict from the host: decode_frc3's pixels, numpy's sums."""
    dec, it, rms = e.decode_frc3(s, 1, **kw)
    H, W = rgb.shape[:2]
    rw, rh = CR.covered(W, H, g)
    chan = CR.channel_sse(dec, rgb, rw, rh)
    return {"sse": sum(chan), "channel_sse": chan, "pixels": rw * rh, "psnr": CR.psnr(sum(chan), rw * rh),
            "iterations": it, "rms": rms}


def strided(rgb, stride):
    """The frame as a CUDA tensor whose rows lie `stride` bytes apart."""
    import torch

    H, W = rgb.shape[:2]
    big = torch.full((H, stride), 0x5A, dtype=torch.uint8, device="cuda")
    t = big.as_strided((H, W, 3), (stride, 3, 1))
    t.copy_(torch.from_numpy(rgb).cuda())
    return t


# --- 1. decode_error_frc3 against the decoded frame ---------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_error_of_a_container(eng, name):
    import torch

    W, H, planes, g, rect = CASES[name]
    assert CR.covered(W, H, g) == rect
    s = F.pack_frc3(planes(), W, H)
    rgb = reference(W, H, 800 + len(name) + W)
    tight = torch.from_numpy(rgb).cuda()
    for m in (-1, 0, 1):
        want = want_error(eng, s, rgb, g, max_iter=m)
        assert eng.decode_error_frc3(s, rgb, max_iter=m) == want       # the host variant: rows 3·W apart
        assert eng.decode_error_frc3(s, tight, max_iter=m) == want     # the device variant, the same rows
    want = want_error(eng, s, rgb, g)
    assert want["pixels"] == rect[0] * rect[1]
    if rect != (0, 0):
        assert min(want["channel_sse"]) > 0
    # rows 4-aligned (with rw % 4 == 0 and rh even: the 4 × 2 path) and rows at an odd distance (the quad path)
    for stride in ((3 * W + 3) // 4 * 4 + 8, 3 * W + 1 + (3 * W) % 2):
        assert eng.decode_error_frc3(s, strided(rgb, stride)) == want, stride
    assert F.color_stream_error(s, rgb) == want                           # a context of its own


def test_the_two_paths_at_one_shape(eng):
    # 98×74: rectangle 96 × 64.  Rows 294 bytes apart (the host variant, the tight tensor) are not dword-aligned:
    # one lane per 2 × 2 quad.  The same frame with rows 296 bytes apart takes the 4 × 2 path.  The same sums.
    W, H, planes, g, rect = CASES["q98x74"]
    assert (3 * W) % 4 != 0 and rect[0] % 4 == 0 and rect[1] % 2 == 0
    s = F.pack_frc3(planes(), W, H)
    rgb = reference(W, H, 811)
    want = want_error(eng, s, rgb, g)
    padded = strided(rgb, 296)
    assert padded.stride(0) == 296 and padded.data_ptr() % 4 == 0
    assert eng.decode_error_frc3(s, rgb) == want
    assert eng.decode_error_frc3(s, padded) == want
    # the margins are excluded: a reference that differs only outside 96 × 64 gives the same sums
    other = rgb.copy()
    other[64:] ^= 0xFF
    other[:, 96:] ^= 0xFF
    assert eng.decode_error_frc3(s, other) == want
    assert eng.decode_error_frc3(s, strided(other, 296)) == want


def test_against_the_single_plane_decodes(eng):
    # the reference does not rest on decode_frc3 alone: the host conversion over the three single-plane decodes
    W, H, planes, g, rect = CASES["q96x64"]
    p = planes()
    rgb = reference(W, H, 812)
    dec = [eng.decode_frq1(x)[0] for x in p]
    chan = CR.channel_sse(Y.yuv2rgb_ref(*dec), rgb, *rect)
    got = eng.decode_error_frc3(F.pack_frc3(p, W, H), rgb)
    assert got["channel_sse"] == chan and got["sse"] == sum(chan) and got["pixels"] == 96 * 64


def test_no_iteration_is_the_zero_planes_colour(eng):
    # zero planes convert to yuv_pixel(0, −128, −128) = (0, 135, 0) at every pixel
    assert Y.yuv2rgb_ref(np.zeros((2, 2), np.uint8), np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8))[0, 0] \
        .tolist() == [0, 135, 0]
    for name in ("q98x74", "c38x28"):
        W, H, planes, g, (rw, rh) = CASES[name]
        rgb = reference(W, H, 813)
        r = rgb[:rh, :rw].astype(np.int64)
        want = [int((r[..., 0] ** 2).sum()), int(((r[..., 1] - 135) ** 2).sum()), int((r[..., 2] ** 2).sum())]
        got = eng.decode_error_frc3(F.pack_frc3(planes(), W, H), rgb, max_iter=0)
        assert got["channel_sse"] == want and got["iterations"] == [0, 0, 0]


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_a_difference_in_one_channel_stays_there(eng, channel):
    for name in ("q96x64", "c38x28"):  # both paths
        W, H, planes, g, (rw, rh) = CASES[name]
        s = F.pack_frc3(planes(), W, H)
        dec = eng.decode_frc3(s)[0]
        ref = dec.copy()
        ref[..., channel] ^= 0x55
        d = dec[:rh, :rw, channel].astype(np.int64) - ref[:rh, :rw, channel].astype(np.int64)
        want = [0, 0, 0]
        want[channel] = int((d * d).sum())
        assert want[channel] > 0
        assert eng.decode_error_frc3(s, ref)["channel_sse"] == want
        assert eng.decode_error_frc3(s, dec)["psnr"] == np.inf


def test_no_covered_pixel(eng):
    W, H, planes, g, rect = CASES["c12x12"]
    p = planes()
    assert F.frc1_info(p[1])["n_ranges"] == 0
    s = F.pack_frc3(p, W, H)
    got = eng.decode_error_frc3(s, reference(W, H, 814))
    it = eng.decode_frc3(s)[1]
    assert (got["sse"], got["channel_sse"], got["pixels"], got["psnr"]) == (0, [0, 0, 0], 0, np.inf)
    assert got["iterations"] == it and it[0] > 0  # the decode ran


# --- 2. refusals, NULL outputs ------------------------------------------------------------------------

def raw(e, s, rgb, stride, outs=True, device=False):
    buf = np.frombuffer(s, np.uint8)
    sse, px = (C.c_uint64 * 3)(7, 7, 7), C.c_uint64(7)
    it, rms = (C.c_int * 3)(7, 7, 7), (C.c_double * 3)(7.0, 7.0, 7.0)
    fn = F.lib().frac_decode_error_frc3_device if device else F.lib().frac_decode_error_frc3
    rc = fn(e._ctx, buf.ctypes.data, len(buf), rgb, stride, -1, 1e-5, *((sse, C.byref(px), it, rms) if outs else
                                                                         (None, None, None, None)))
    return rc, (list(sse), px.value, list(it), list(rms))


def test_refusals_change_nothing(eng):
    import torch

    W, H, planes, g, rect = CASES["q98x74"]
    s = F.pack_frc3(planes(), W, H)
    rgb = reference(W, H, 815)
    dev = torch.from_numpy(rgb).cuda()
    want = want_error(eng, s, rgb, g)
    untouched = ([7, 7, 7], 7, [7, 7, 7], [7.0, 7.0, 7.0])
    host, devp = rgb.ctypes.data, C.c_void_p(dev.data_ptr())
    bad = [(s, None, 3 * W), (s, host, 3 * W - 1),                       # NULL rgb, a short stride
           (s[:6] + b"\x01" + s[7:], host, 3 * W),                       # the flags are not zero
           (s[:-8], host, 3 * W),                                        # the V section runs past the end
           (s[:32] + b"FRC9" + s[36:], host, 3 * W)]                     # a plane stream of no kind
    for stream, ptr, stride in bad:
        assert raw(eng, stream, ptr, stride) == (-1, untouched)
        assert raw(eng, stream, devp if ptr else None, stride, device=True) == (-1, untouched)
    rc, (sse, px, it, rms) = raw(eng, s, host, 3 * W)
    assert (rc, sse, px, it, rms) == (0, want["channel_sse"], want["pixels"], want["iterations"], want["rms"])
    assert raw(eng, s, devp, 3 * W, device=True) == (rc, (sse, px, it, rms))
    assert raw(eng, s, host, 3 * W, outs=False)[0] == 0 and raw(eng, s, devp, 3 * W, outs=False, device=True)[0] == 0
    assert F.lib().frac_decode_error_frc3(None, None, 0, None, 0, -1, 1e-5, None, None, None, None) == -1
    # the binding's own checks
    with pytest.raises(F.FracError, match="rc=-1"):
        eng.decode_error_frc3(s[:-8], rgb)
    with pytest.raises(F.FracError, match="98x74"):
        eng.decode_error_frc3(s, rgb[:, :97])
    with pytest.raises(F.FracError):
        eng.decode_error_frc3(s, dev.to(torch.int16))
    with pytest.raises(F.FracError):  # pixels not packed
        eng.decode_error_frc3(s, torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")[:, :, :3])
    assert eng.decode_error_frc3(s, rgb) == want


# --- 3. the reader rule ---------------------------------------------------------------------------------

def test_the_colour_error_is_a_reader(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    frame = case.planes()[0]
    doms, rngs = F.create_uniform_grid(case.W, case.H, 16, 8), F.create_uniform_grid(case.W, case.H, 8, 8)
    W, H, planes, g, rect = CASES["q96x64"]
    s = F.pack_frc3(planes(), W, H)
    rgb = reference(W, H, 816)
    with F.Engine(0, case.T, case.cls) as ref:  # a run nothing came between
        ref.set_frame(frame)
        ref.set_domains(doms)
        ref.set_ranges(rngs)
        ref.run()
        want_items, want_stats = ref.fetch()
    with F.Engine(0, case.T, case.cls) as e:
        err = e.decode_error_frc3(s, rgb)  # no frame set: any context can
        assert err == want_error(e, s, rgb, g)
        with pytest.raises(F.FracError, match="rc=-3"):  # no rate state
            e.rate_candidates()
        e.set_frame(frame)
        e.set_domains(doms)
        e.set_ranges(rngs)
        e.run()
        assert e.decode_error_frc3(s, rgb) == err  # between run() and fetch()
        with pytest.raises(F.FracError, match="rc=-3"):  # a run is no rate state; the refusal changes nothing
            e.rate_candidates()
        items, stats = e.fetch()
        np.testing.assert_array_equal(items, want_items)
        assert stats["rejected_mappings"] == want_stats["rejected_mappings"]
        assert e.decode_error_frc3(s, rgb) == err
        np.testing.assert_array_equal(e.fetch()[0], want_items)
        # with a rate state: the readers answer as before
        e.quadtree_rate(case.max_size, case.min_size)
        cands = e.rate_candidates()
        ts = R.spread(cands, 5)
        before = (e.rate_sizes(ts), e.rate_leaves(float(ts[2])), e.rate_fit(1 << 20), e.rate_errors(ts))
        assert e.decode_error_frc3(s, rgb) == err
        np.testing.assert_array_equal(e.rate_candidates(), cands)
        for a, b in zip(before[0] + before[3], e.rate_sizes(ts) + e.rate_errors(ts)):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(before[1], e.rate_leaves(float(ts[2])))
        assert before[2] == e.rate_fit(1 << 20)
        e.set_frame(frame)  # a setter ends the rate state for this reader too
        with pytest.raises(F.FracError, match="rc=-3"):
            e.rate_candidates()


# --- 4. rate_candidates ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["m98x74_16_4", "m70x58_16_4", "z15x15", "e33x47_16_8", "p98x74_two"])
def test_rate_candidates_are_the_trees(oracle, name):
    case = Q.BY_NAME[name]
    want = R.tree(oracle, case).candidates()
    src, tgt = case.planes()
    with F.Engine(0, case.T, case.cls, case.thr) as e:
        if tgt is None:
            e.set_frame(src)
        else:
            e.set_planes(src, tgt)
        e.quadtree_rate(case.max_size, case.min_size)
        got = e.rate_candidates()
        assert got.dtype == np.float64 and got.shape == want.shape and (got == want).all()
        assert got[0] == 0.0 and (np.diff(got) > 0).all()
        if name == "z15x15":
            assert got.tolist() == [0.0]
        # the count whatever the capacity; nothing past it
        short = np.full(5, -7.0)
        n = C.c_size_t(0)
        e._check(F.lib().frac_quadtree_rate_candidates(e._ctx, short.ctypes.data, 3, C.byref(n)))
        assert n.value == len(want)
        k = min(3, len(want))
        assert short[:k].tolist() == want[:k].tolist() and (short[k:] == -7.0).all()
        e._check(F.lib().frac_quadtree_rate_candidates(e._ctx, None, 0, None))


@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: c.name)
def test_rate_quality_bisects_that_list(case):
    # factoring the list out changed nothing: the answers are the stated bisection over rate_errors of
    # rate_candidates (test_gpu_quality.py pins the same answers to the host's errors), and lie in the list
    with F.Engine(0, case.T, case.cls, case.thr) as e:
        e.set_frame(case.planes()[0])
        e.quadtree_rate(case.max_size, case.min_size)
        cands = e.rate_candidates()
        E = [int(v) for v in e.rate_errors(cands)[0]]
        s = sorted(E)
        for target in [E[-1], E[0], E[-1] - 1] + [s[len(s) * k // 4] for k in (1, 2, 3)]:
            idx, probes = QR.bisect(E, target)
            if idx is None:
                with pytest.raises(F.FracError, match="rc=-1"):
                    e.rate_quality(max_sse=target)
                continue
            got = e.rate_quality(max_sse=target)
            assert got[0] == float(cands[idx]) and got[0] in cands and (got[3], got[4]) == (E[idx], probes)


# --- 5. ColorEncoder: one split distance steers the three planes ---------------------------------------------

GEOM = (16, 4)


@pytest.fixture(scope="module", params=[(98, 74), (70, 58)], ids=lambda p: "%dx%d" % p)
def colour(request):
    """An encoder with the frame loaded and the rate states built, and the union enumerated once on the host:
    sizes through each engine's rate_stream lengths, errors through decode_frc3 + numpy."""
    W, H = request.param
    rgb = np.ascontiguousarray(np.stack([Q.mixed(W, H, seed) for seed in (Q.SEED, Q.TGT_SEED, 13)], axis=-1))
    rect = CR.covered(W, H, GEOM[0])
    with ColorEncoder(0, transforms=4) as enc:
        enc.load(rgb)
        enc.quadtree_rate(*GEOM)
        per_plane = [e.rate_candidates() for e in enc.engines]
        u = CR.union(per_plane)
        planes, sizes, chan, containers = [], [], [], []
        for t in u:
            streams = [e.rate_stream(float(t)) for e in enc.engines]
            planes.append([len(x) for x in streams])
            sizes.append(CR.container_bytes(planes[-1]))
            containers.append(F.pack_frc3(streams, W, H))
            assert len(containers[-1]) == sizes[-1]
            chan.append(CR.channel_sse(enc.engines[0].decode_frc3(containers[-1])[0], rgb, *rect))
        E = [sum(c) for c in chan]
        print(f"{W}x{H}: union {len(u)} of {[len(c) for c in per_plane]}, sizes {sizes[0]}..{sizes[-1]}, "
              f"E {E[0]}..{E[-1]}, monotone E {E == sorted(E)}, monotone sizes {sizes == sorted(sizes, reverse=True)}")
        yield SimpleNamespace(W=W, H=H, rgb=rgb, enc=enc, u=u, planes=planes, sizes=sizes, chan=chan, E=E,
                              containers=containers, pixels=rect[0] * rect[1], per_plane=per_plane)


def test_colour_candidates_and_sizes(colour):
    c = colour
    m = len(c.u)
    assert m > max(len(p) for p in c.per_plane)  # a union, not one plane's list
    got = c.enc.rate_candidates()
    assert got.dtype == np.float64 and got.shape == c.u.shape and (got == c.u).all()
    size, planes = c.enc.rate_sizes(c.u)
    assert size.dtype == planes.dtype == np.uint64 and planes.shape == (m, 3)
    assert size.tolist() == c.sizes and planes.tolist() == c.planes
    for i in (0, m // 2, m - 1):
        assert c.enc.rate_stream(float(c.u[i])) == c.containers[i]
    assert c.enc.decode_error(c.containers[m // 2])["channel_sse"] == c.chan[m // 2]
    assert c.enc.decode_error(c.containers[m // 2]) == c.enc.engines[1].decode_error_frc3(c.containers[m // 2], c.rgb)


def test_colour_size_rule(colour):
    c = colour
    m = len(c.u)
    s = sorted(set(c.sizes))
    interior = 0
    for q in (s[len(s) // 4], s[len(s) // 2], s[3 * len(s) // 4]):
        for budget in (q, q - 1):
            i = CR.fit_size(c.sizes, budget)
            assert c.enc.rate_fit(budget) == (float(c.u[i]), c.sizes[i], c.planes[i]), budget
            assert c.sizes[i] <= budget and all(v > budget for v in c.sizes[:i])
            interior += 0 < i < m - 1
    assert interior  # a fit that only ever returned an end of the list would hide a broken search
    assert c.enc.rate_fit(s[-1] + 1000)[0] == 0.0
    i = CR.fit_size(c.sizes, s[0])
    assert c.enc.rate_fit(s[0]) == (float(c.u[i]), s[0], c.planes[i])
    with pytest.raises(F.FracError, match=f"smallest container has {s[0]} bytes"):
        c.enc.rate_fit(s[0] - 1)


def test_colour_errors(colour):
    c = colour
    idx = np.unique(np.round(np.linspace(0, len(c.u) - 1, 7)).astype(int))
    sse, chan, size = c.enc.rate_errors(c.u[idx])
    assert sse.dtype == chan.dtype == size.dtype == np.uint64
    assert sse.tolist() == [c.E[i] for i in idx] and chan.tolist() == [c.chan[i] for i in idx]
    assert size.tolist() == [c.sizes[i] for i in idx]
    assert [a.shape for a in c.enc.rate_errors([])] == [(0,), (0, 3), (0,)]


def _quality_targets(E):
    m = len(E)
    inner = [E[m // 4], E[m // 2], E[3 * m // 4]]  # errors at interior candidates
    return [E[-1], E[-1] - 1, E[0], E[0] - 1] + inner + [v - 1 for v in inner]


def _psnr_targets(c):
    """PSNRs (quarter dB, rounded down: the bound is no tighter) of the errors at three interior candidates that the
    smallest candidate meets and the largest does not, so the bisection has something to do; E is not monotone
    (at 70×58 the error at the middle candidate lies below E[0], and a target taken from it is refused)."""
    m = len(c.E)
    ks = [k for k in range(1, m - 1) if c.E[0] <= c.E[k] < c.E[-1]]
    assert len(ks) >= 3
    return [float(np.floor(CR.psnr(c.E[k], c.pixels) * 4) / 4) for k in (ks[len(ks) // 4], ks[len(ks) // 2],
                                                                          ks[3 * len(ks) // 4])]


def test_colour_quality_rule(colour):
    c = colour
    m = len(c.u)
    interior = 0
    for target in _quality_targets(c.E):
        i, probes = QR.bisect(c.E, target)
        if i is None:
            with pytest.raises(F.FracError, match=f"smallest split distance, {c.E[0]},"):
                c.enc.rate_quality(max_sse=target)
            continue
        got = c.enc.rate_quality(max_sse=target)
        assert got == {"split_distance": float(c.u[i]), "bytes": c.sizes[i], "sse": c.E[i],
                       "channel_sse": c.chan[i], "pixels": c.pixels, "psnr": CR.psnr(c.E[i], c.pixels),
                       "probes": probes}, target
        assert c.E[i] <= target and (i == m - 1 or c.E[i + 1] > target)  # the guarantee
        interior += 0 < i < m - 1
    assert interior
    # PSNR targets: the same rule at the translated bound
    for psnr in _psnr_targets(c):
        i, probes = QR.bisect(c.E, CR.max_sse_of(psnr, c.pixels))
        got = c.enc.rate_quality(min_psnr=psnr)
        assert (got["split_distance"], got["sse"], got["probes"]) == (float(c.u[i]), c.E[i], probes)
        assert got["psnr"] >= psnr
    with pytest.raises(ValueError):
        c.enc.rate_quality()
    with pytest.raises(ValueError):
        c.enc.rate_quality(max_sse=1, min_psnr=30.0)


def test_colour_encode_to_size(colour):
    c = colour
    m = len(c.u)
    s = sorted(set(c.sizes))
    budget = s[len(s) // 2] + 3
    i = CR.fit_size(c.sizes, budget)
    assert 0 < i < m - 1
    stream, info = c.enc.encode_quadtree_to_size(budget, *GEOM)
    assert stream == c.containers[i] and len(stream) <= budget
    assert stream == F.pack_frc3([e.rate_stream(info["split_distance"]) for e in c.enc.engines], c.W, c.H)
    assert (info["split_distance"], info["bytes"], info["plane_bytes"]) == (float(c.u[i]), c.sizes[i], c.planes[i])
    assert len(info["stats"]) == 3 and all(st["total_mappings"] > 0 for st in info["stats"])
    with pytest.raises(F.FracError, match=f"smallest container has {s[0]} bytes"):
        c.enc.encode_quadtree_to_size(s[0] - 1, *GEOM)


def test_colour_encode_to_psnr(colour):
    c = colour
    m = len(c.u)
    answers = []
    for psnr in _psnr_targets(c):
        i, probes = QR.bisect(c.E, CR.max_sse_of(psnr, c.pixels))
        stream, info = c.enc.encode_quadtree_to_psnr(psnr, *GEOM)
        err = c.enc.decode_error(stream)
        assert info["sse"] == err["sse"] and info["channel_sse"] == err["channel_sse"]
        assert info["psnr"] == err["psnr"] >= psnr and info["pixels"] == err["pixels"] == c.pixels
        assert stream == c.containers[i] and info["bytes"] == len(stream)
        assert (info["split_distance"], info["sse"], info["probes"]) == (float(c.u[i]), c.E[i], probes)
        assert len(info["stats"]) == 3
        answers.append(i)
    assert any(0 < i < m - 1 for i in answers)
