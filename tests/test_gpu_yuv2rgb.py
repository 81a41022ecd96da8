"""Device yuv2rgb (fracenc_color.hip yuv2rgb_quads4 / yuv2rgb_generic) against the reference build's goldens
(all 2^24 triples, Lenna, odd and smallest frames) and, at the shapes where each kernel can go wrong, against the
host restatement (tests/yuv2rgb_ref.py, itself pinned to the same goldens by test_yuv2rgb_host.py).  Every
comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest

import fractencode_amd as F
import yuv2rgb_ref as R
from fractencode_amd.synth import sha256
from golden_util import GOLD, plane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with F.Engine(0) as e:
        yield e


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_all_triples(eng):
    with open(f"{GOLD}/yuv2rgb.json") as f:
        digests = json.load(f)["chunks"]
    for c in range(4):
        y, u, v = R.all_triples_planes(c)
        rgb = eng.yuv_to_rgb(cuda(y), cuda(u), cuda(v))  # 4096²: the fast path
        assert sha256(np.ascontiguousarray(rgb[::2, ::2].cpu().numpy())) == digests[c], c


def test_lenna_host_buffers(eng):
    with open(f"{GOLD}/yuv2rgb.json") as f:
        want = json.load(f)["lenna"]
    rgb = eng.yuv_to_rgb(plane("lenna_y"), plane("lenna_u"), plane("lenna_v"))
    assert rgb.shape == (512, 512, 3) and sha256(rgb) == want


@pytest.mark.parametrize("name", ["67x101", "3x5", "2x2"])
@pytest.mark.parametrize("device", [False, True])
def test_odd_and_smallest_goldens(eng, name, device):
    z = np.load(f"{GOLD}/rgb_from_yuv_odd.npz")
    y, u, v, want = (z[f"{k}_{name}"] for k in ("y", "u", "v", "rgb"))
    got = eng.yuv_to_rgb(cuda(y), cuda(u), cuda(v)).cpu().numpy() if device else eng.yuv_to_rgb(y, u, v)
    np.testing.assert_array_equal(got, want)


# (W, H): 2×2 the smallest frame; 4×2 one fast-path lane; 6×4 width no multiple of 4 (generic); 8×6 fast path,
# three lane rows; 1024×2 more than one workgroup (256 lanes) in a row; 5×3 and 101×67 the chroma clamp;
# 2052×4 a fast-path grid whose last workgroup is partial
SHAPES = [(2, 2), (4, 2), (6, 4), (8, 6), (1024, 2), (1028, 6), (5, 3), (101, 67), (2052, 4)]


@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes_against_the_restatement(eng, W, H):
    y, u, v = R.seeded_planes(W, H, 1000 + W)
    want = R.yuv2rgb_ref(y, u, v)
    np.testing.assert_array_equal(eng.yuv_to_rgb(y, u, v), want)  # host buffers: planes at the library's pitch
    got = eng.yuv_to_rgb(cuda(y), cuda(u), cuda(v))               # tight device planes
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("pad", [4, 5, 64])
def test_device_planes_with_padded_rows(eng, pad):
    # every plane's rows padded by `pad` bytes: 4 and 64 keep the fast path's alignment, 5 breaks it (generic)
    import torch

    W, H = 72, 10
    y, u, v = R.seeded_planes(W, H, 2000 + pad)
    want = R.yuv2rgb_ref(y, u, v)

    def padded(a, p):
        big = torch.full((a.shape[0], a.shape[1] + p), 0xA5, dtype=torch.uint8, device="cuda")
        big[:, :a.shape[1]] = cuda(a)
        return big[:, :a.shape[1]]

    ty, tu, tv = padded(y, pad), padded(u, pad), padded(v, pad)
    assert ty.stride(0) == W + pad and not ty.is_contiguous()
    np.testing.assert_array_equal(eng.yuv_to_rgb(ty, tu, tv).cpu().numpy(), want)


def test_misaligned_luma_takes_the_generic_kernel(eng):
    # a Y tensor that starts at byte offset 1 of its allocation: no aligned dword loads
    import torch

    W, H = 64, 8
    y, u, v = R.seeded_planes(W, H, 2100)
    flat = torch.zeros(W * H + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = cuda(y).reshape(-1)
    ty = flat[1:].view(H, W)
    assert ty.data_ptr() % 4 == 1
    np.testing.assert_array_equal(eng.yuv_to_rgb(ty, cuda(u), cuda(v)).cpu().numpy(), R.yuv2rgb_ref(y, u, v))
    # and misaligned chroma
    fu = torch.zeros(u.size + 1, dtype=torch.uint8, device="cuda")
    fu[1:] = cuda(u).reshape(-1)
    tu = fu[1:].view(H // 2, W // 2)
    np.testing.assert_array_equal(eng.yuv_to_rgb(cuda(y), tu, cuda(v)).cpu().numpy(), R.yuv2rgb_ref(y, u, v))


def test_rgb_stride_in_bytes_and_untouched_padding(eng):
    # frac_yuv_to_rgb_device with an RGB row stride above 3·w: bytes, and the padding stays as it was
    import torch

    W, H = 12, 6
    y, u, v = R.seeded_planes(W, H, 2200)
    ty, tu, tv = cuda(y), cuda(u), cuda(v)
    for stride in (3 * W + 4, 3 * W + 7):  # fast path / generic
        out = torch.full((H, stride), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = F.lib().frac_yuv_to_rgb_device(eng._ctx, C.c_void_p(ty.data_ptr()), W, H, W, C.c_void_p(tu.data_ptr()),
                                            W // 2, C.c_void_p(tv.data_ptr()), W // 2, C.c_void_p(out.data_ptr()),
                                            stride)
        assert rc == 0
        eng.sync()
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:, :3 * W].reshape(H, W, 3), R.yuv2rgb_ref(y, u, v))
        assert (got[:, 3 * W:] == 0x5A).all()


@pytest.mark.parametrize("W,H", [(1, 8), (8, 1), (1, 1), (0, 4), (4, 0)])
def test_frames_below_two_pixels_are_refused(eng, W, H):
    import torch

    out = torch.full((max(H, 1), 3 * max(W, 1)), 0x5A, dtype=torch.uint8, device="cuda")
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = C.c_void_p(src.data_ptr())
    rc = F.lib().frac_yuv_to_rgb_device(eng._ctx, p, W, H, max(W, 1), p, 1, p, 1, C.c_void_p(out.data_ptr()),
                                        3 * max(W, 1))
    assert rc == -1 and "chroma" in F.last_error(eng._ctx)  # FRAC_E_INVALID
    eng.sync()
    assert (out.cpu().numpy() == 0x5A).all()  # nothing launched
    y = np.zeros((H, W), np.uint8)
    c = np.zeros((H // 2, W // 2), np.uint8)
    with pytest.raises(F.FracError):
        eng.yuv_to_rgb(y, c, c)


def test_bad_strides_and_shapes_are_refused_in_python(eng):
    import torch

    y, u, v = (cuda(a) for a in R.seeded_planes(16, 8, 2300))
    with pytest.raises(F.FracError):
        eng.yuv_to_rgb(y[:, ::2], u[:, :4], v[:, :4])  # column stride 2
    with pytest.raises(F.FracError):
        eng.yuv_to_rgb(y[0:1].expand(8, 16), u, v)  # row stride 0, below the width
    with pytest.raises(F.FracError):
        eng.yuv_to_rgb(y, u[:3], v)  # chroma of another size
    with pytest.raises(F.FracError):
        eng.yuv_to_rgb(y.to(torch.int16), u, v)
    with pytest.raises(F.FracError):
        eng.yuv_to_rgb(y, u.cpu().numpy(), v)  # mixed host and device
    # the library's own check: a luma stride below the width
    rgb = torch.zeros((8, 48), dtype=torch.uint8, device="cuda")
    rc = F.lib().frac_yuv_to_rgb_device(eng._ctx, C.c_void_p(y.data_ptr()), 16, 8, 15, C.c_void_p(u.data_ptr()), 8,
                                        C.c_void_p(v.data_ptr()), 8, C.c_void_p(rgb.data_ptr()), 48)
    assert rc == -1


def test_grey_ramp_round_trip_is_the_references(eng, oracle):
    # rgb_to_yuv then yuv_to_rgb on a grey ramp: the reference's result, which is not the ramp (its chroma
    # weights do not sum to zero, so grey has U = V = 127; test_yuv2rgb_host.py checks that side)
    g = np.arange(256, dtype=np.uint8)
    rgb = np.repeat(np.repeat(g, 3).reshape(1, 256, 3), 2, 0)
    y, u, v = eng.rgb_to_yuv(rgb)
    wy, wu, wv = oracle.rgb2yuv(rgb)
    for a, b in ((y, wy), (u, wu), (v, wv)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.yuv_to_rgb(y, u, v), R.yuv2rgb_ref(wy, wu, wv))


def test_conversion_leaves_a_runs_results_readable(eng):
    p = plane("crop64")
    with F.Engine(0, 4) as e:
        e.set_frame(p)
        e.set_domains(F.create_uniform_grid(64, 64, 16, 8))
        out, _ = e.search(F.create_uniform_grid(64, 64, 8, 8))
        y, u, v = R.seeded_planes(8, 6, 2400)
        e.yuv_to_rgb(y, u, v)
        e.yuv_to_rgb(cuda(y), cuda(u), cuda(v))
        again, _ = e.fetch()
    assert again.tobytes() == out.tobytes()
