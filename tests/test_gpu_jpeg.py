"""GPU: the baseline JPEG encoder (rd_jpeg_*) byte for byte against the numpy oracle (tests/jpeg_oracle.py), which the CPU
suite pins to libjpeg through Pillow."""
import ctypes as C
import io

import numpy as np
import pytest

from raweditor_amd import _lib
from raweditor_amd._lib import check
from tests import jpeg_oracle as jo
from tests.gpu_util import DevBuf, sync
from tests.helpers import CM_IDENTITY, CM_TEST, WB_DAYLIGHT, mild_params

pytestmark = pytest.mark.gpu

SUBS = ("4:2:0", "4:4:4")


def test_image(rng, h, w, kind, c=3):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, c).astype(np.uint8), (h, w, c)).copy()
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx * 3 + yy * 5) % 256] + [np.full_like(xx, 255)] * (c - 3), -1)
    return img.astype(np.uint8)


test_image.__test__ = False


def encode_frames(ra, imgs, fmt, q, sub, R, extra_pitch=0, enc=None, stream=0):
    """Encode host frames (h, w, c) through device surfaces with rows `extra_pitch` bytes longer than a row.  Returns
    (encoder, [dst DevBuf], len DevBuf, [src DevBuf]) without synchronising."""
    h, w, c = imgs[0].shape
    enc = enc or ra.JpegEncoder(0, w, h, fmt, q, sub, R)
    pitch = w * c + extra_pitch
    srcs = []
    for a in imgs:
        host = np.zeros((h, pitch), np.uint8)
        host[:, :w * c] = a.reshape(h, w * c)
        srcs.append(DevBuf.from_array(host))
    dsts = [DevBuf(enc.max_bytes) for _ in imgs]
    lens = DevBuf(8 * len(imgs))
    enc.encode([s.ptr for s in srcs], [d.ptr for d in dsts], lens.ptr, stream=stream, pitch=pitch)
    return enc, dsts, lens, srcs


def fetch(dsts, lens):
    n = lens.to_array(np.uint64, (len(dsts),))
    return [d.to_array(np.uint8, (int(k),)).tobytes() for d, k in zip(dsts, n)]


SIZES = [(1, 1), (7, 5), (17, 9), (33, 31), (640, 427), (453, 301)]


@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_small_frames_match_the_oracle(gpu_lib, W, H):
    ra = gpu_lib
    rng = np.random.default_rng(W * 1000 + H)
    combos = [(90, "4:2:0", 32), (75, "4:4:4", 7), (1, "4:2:0", 1), (100, "4:4:4", 32), (50, "4:2:0", 7), (95, "4:4:4", 1)]
    for fmt in (ra.FMT_RGB_U8, ra.FMT_RGBA_U8):
        c = 4 if fmt == ra.FMT_RGBA_U8 else 3
        for q, sub, R in combos:
            imgs = [test_image(rng, H, W, k, c) for k in ("noise", "smooth", "flat")]
            enc, dsts, lens, srcs = encode_frames(ra, imgs, fmt, q, sub, R, extra_pitch=int(rng.integers(1, 40)))
            sync()
            for img, got in zip(imgs, fetch(dsts, lens)):
                want = jo.encode(img, q, sub, R)
                assert got == want, (W, H, fmt, q, sub, R, len(got), len(want))
            enc.close()


def test_dst_cap_below_the_worst_case_is_an_argument_error(gpu_lib):
    ra = gpu_lib
    enc = ra.JpegEncoder(0, 64, 48, ra.FMT_RGB_U8, 90, "4:2:0", 32)
    src, dst, lens = DevBuf(64 * 48 * 3), DevBuf(enc.max_bytes), DevBuf(8)
    with pytest.raises(ra.RawdevError) as e:
        enc.encode([src.ptr], [dst.ptr], lens.ptr, dst_cap=enc.max_bytes - 1)
    assert e.value.code == _lib.RD_ERR_INVALID_ARG and "worst case" in e.value.message
    with pytest.raises(ra.RawdevError) as e:
        enc.encode([src.ptr], [dst.ptr], lens.ptr, pitch=64 * 3 - 1)
    assert e.value.code == _lib.RD_ERR_INVALID_ARG
    # the worst case holds the largest stream the tables allow: q 100 noise stays far below it
    assert enc.max_bytes > len(jo.encode(np.random.default_rng(0).integers(0, 256, (48, 64, 3), dtype=np.uint8), 100, "4:2:0", 32))
    enc.close()


def test_heterogeneous_multi_frame_call_spans_launches(gpu_lib):
    """More frames than one launch takes (RD_JPEG_LAUNCH_MAX = 8), noise, gradients and flat frames mixed."""
    ra = gpu_lib
    rng = np.random.default_rng(21)
    W, H = 157, 93
    imgs = [test_image(rng, H, W, ("noise", "smooth", "flat")[k % 3]) for k in range(19)]
    enc, dsts, lens, srcs = encode_frames(ra, imgs, ra.FMT_RGB_U8, 85, "4:2:0", 5)
    sync()
    for img, got in zip(imgs, fetch(dsts, lens)):
        assert got == jo.encode(img, 85, "4:2:0", 5)
    enc.close()


def test_two_contexts_on_two_streams_interleaved(gpu_lib):
    ra = gpu_lib
    L = _lib.lib()
    rng = np.random.default_rng(22)
    s = [C.c_void_p(), C.c_void_p()]
    for x in s:
        check(L.rd_stream_create(0, C.byref(x)))
    specs = [(320, 211, ra.FMT_RGBA_U8, 90, "4:2:0", 32), (301, 200, ra.FMT_RGB_U8, 60, "4:4:4", 3)]
    encs = [None, None]
    calls = []
    for rep in range(3):
        for k, (W, H, fmt, q, sub, R) in enumerate(specs):
            c = 4 if fmt == ra.FMT_RGBA_U8 else 3
            imgs = [test_image(rng, H, W, "noise" if i else "smooth", c) for i in range(2)]
            enc, dsts, lens, srcs = encode_frames(ra, imgs, fmt, q, sub, R, enc=encs[k], stream=s[k].value)
            encs[k] = enc
            calls.append((k, imgs, dsts, lens, srcs))
    for x in s:
        check(L.rd_stream_synchronize(0, x))
    for k, imgs, dsts, lens, srcs in calls:
        _, _, _, q, sub, R = specs[k]
        for img, got in zip(imgs, fetch(dsts, lens)):
            assert got == jo.encode(img, q, sub, R)
    for e in encs:
        e.close()
    for x in s:
        check(L.rd_stream_destroy(0, x))


@pytest.mark.parametrize("site", ["jpeg.scratch", "jpeg.launch", "rd_jpeg_encode"])
def test_injected_fault_leaves_the_context_usable(gpu_lib, site):
    ra = gpu_lib
    rng = np.random.default_rng(23)
    img = test_image(rng, 61, 90, "noise")
    if site == "jpeg.scratch":
        _lib.inject_fault(site, _lib.FAULT_BAD_ALLOC)
        with pytest.raises(ra.RawdevError) as e:
            ra.JpegEncoder(0, 90, 61)
        assert e.value.code == _lib.RD_ERR_OOM
        enc = ra.JpegEncoder(0, 90, 61)
    else:
        enc = ra.JpegEncoder(0, 90, 61)
        _lib.inject_fault(site, _lib.FAULT_RUNTIME)
        with pytest.raises(ra.RawdevError) as e:
            encode_frames(ra, [img], ra.FMT_RGB_U8, 90, "4:2:0", 32, enc=enc)
        assert e.value.code == _lib.RD_ERR_INTERNAL
    _lib.inject_fault(None, 0)
    assert enc.encode_array(img) == jo.encode(img, 90, "4:2:0", 32)
    enc.close()


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def scene_cfa(rng, H, W):
    """A mosaic with structure: smooth waves and edges of random phase, plus sensor-like noise."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    p = rng.uniform(0, 6.3, 4).astype(np.float32)
    v = 1800 + 900 * np.sin(xx / 211 + p[0]) * np.cos(yy / 157 + p[1]) + 500 * np.sin((xx + 2 * yy) / 53 + p[2])
    v += 400 * (np.sin(xx / 37 + p[3]) > 0.6)
    v += rng.normal(0, 25, (H, W)).astype(np.float32)
    return np.clip(v, 0, 4095).astype(np.uint16)


def _develop_rgb8(ra, W, H, seed, n=1):
    rng = np.random.default_rng(seed)
    cfas = [scene_cfa(rng, H, W) for _ in range(n)]
    d_in = [DevBuf.from_array(c) for c in cfas]
    d_out = [DevBuf(W * H * 3) for _ in range(n)]
    be = ra.BatchExporter(0, W, H, ra.FMT_RGB_U8, False)
    frames = be.make_frames([b.ptr for b in d_in], [b.ptr for b in d_out], [ra.EditParams(**mild_params(rng)) for _ in range(n)],
                            WB_DAYLIGHT, CM_TEST)
    be.develop(frames)
    return be, frames, d_in, d_out


@pytest.mark.parametrize("W,H", [(6016, 4016), (6001, 4001)])
def test_full_size_developed_frame(gpu_lib, W, H):
    ra = gpu_lib
    be, frames, d_in, d_out = _develop_rgb8(ra, W, H, W)
    enc = ra.JpegEncoder(0, W, H, ra.FMT_RGB_U8, 90, "4:2:0", 32)
    dst, lens = DevBuf(enc.max_bytes), DevBuf(8)
    enc.encode([d_out[0].ptr], [dst.ptr], lens.ptr)
    sync()
    img = d_out[0].to_array(np.uint8, (H, W, 3))
    got = fetch([dst], lens)[0]
    hdr, parts, tail = jo.split_scan(got)
    assert hdr == jo.header(W, H, 90, "4:2:0", 32) and tail == b"\xff\xd9"
    assert len(parts) == jo.n_intervals(W, H, "4:2:0", 32)
    rng = np.random.default_rng(H)
    picks = sorted(set([0, len(parts) - 1] + [int(x) for x in rng.integers(0, len(parts), 62)]))
    for r in picks:
        assert parts[r] == jo.encode_interval(img, r, 90, "4:2:0", 32), r
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        dec = np.asarray(Image.open(io.BytesIO(got)).convert("RGB"))
        assert dec.shape == img.shape
        assert _psnr(dec, img) > 30.0, _psnr(dec, img)
    enc.close(); be.close()


def test_render_tier_jpegs_match_the_oracle(gpu_lib):
    ra = gpu_lib
    rng = np.random.default_rng(24)
    W, H = 611, 407
    cfa = rng.integers(0, 4096, (H, W), dtype=np.uint16)
    p = ra.EditParams(**mild_params(rng))
    arrays = ra.render_tiers(cfa, W, H, p, WB_DAYLIGHT, CM_IDENTITY, black_level=16, fmt=ra.FMT_RGB_U8)
    files = ra.render_tier_jpegs(cfa, W, H, p, WB_DAYLIGHT, CM_IDENTITY, black_level=16, quality=88)
    assert len(files) == 3
    for a, f in zip(arrays, files):
        assert f == jo.encode(a, 88, "4:2:0", 32)


def test_develop_to_jpeg_matches_the_oracle(gpu_lib):
    ra = gpu_lib
    W, H = 523, 347
    be, frames, d_in, d_out = _develop_rgb8(ra, W, H, 25, n=3)
    sync()
    want = [jo.encode(o.to_array(np.uint8, (H, W, 3)), 80, "4:4:4", 9) for o in d_out]
    got = ra.develop_to_jpeg(frames, W, H, quality=80, subsampling="4:4:4", restart_mcus=9)
    assert got == want
    assert [f.out_dev for f in frames] == [o.ptr for o in d_out]     # the caller's frames are left as they were
    be.close()
