"""CPU: the JPEG encoder's contract -- the numpy oracle pinned byte for byte to libjpeg through Pillow,
the library's header against the oracle's, the reciprocal quantiser proved against the division, argument errors through
the C ABI, the catalog writer and the new kernels' resources.  No GPU needed."""
import io
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import raweditor_amd as ra
from raweditor_amd import _lib, catalog
from raweditor_amd.build import load_resources
from tests import jpeg_oracle as jo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 5), (17, 9), (33, 31), (640, 427), (453, 301)]
QUALITIES = (1, 10, 50, 75, 90, 95, 100)


def frame(rng, h, w, kind):
    if kind == "noise":                                    # forces 0xFF stuffing and the longest codes
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127.5 + 120 * np.sin(xx / 23.0 + yy / 41.0), 127.5 + 120 * np.cos(yy / 17.0),
                    (xx + yy) * 255.0 / max(w + h - 2, 1)], -1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def pillow(img, q, sub, R):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[:, :, :3].copy(), "RGB").save(b, "JPEG", quality=q, subsampling=0 if sub == "4:4:4" else 2,
                                                     restart_marker_blocks=R)
    return b.getvalue()


# ---- the oracle is libjpeg's default path ------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_oracle_equals_pillow_byte_for_byte(W, H):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(W * 7 + H)
    big = W * H > 10000
    n = 0
    for kind in ("noise", "smooth", "flat"):
        img = frame(rng, H, W, kind)
        for q in QUALITIES:
            for sub in ("4:2:0", "4:4:4"):
                for R in (1, 7, 32):
                    # the large frames take every quality once, with R and the subsampling rotating
                    if big and (QUALITIES.index(q) + (sub == "4:4:4") + (1, 7, 32).index(R)) % 3:
                        continue
                    got, want = jo.encode(img, q, sub, R), pillow(img, q, sub, R)
                    assert got == want, (W, H, kind, q, sub, R, len(got), len(want))
                    n += 1
    assert n >= (3 * 7 * 2 * 3 if not big else 3 * 7 * 2 * 3 // 3)


def test_noise_exercises_stuffing_and_the_longest_codes():
    rng = np.random.default_rng(3)
    img = frame(rng, 64, 64, "noise")
    yy, xx = np.mgrid[0:32, 0:64]
    img[:32] = np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)[..., None]       # a checkerboard: the top AC band
    data = jo.encode(img, 100, "4:4:4", 32)
    _, parts, _ = jo.split_scan(data)
    body = b"".join(parts)
    assert body.count(b"\xff\x00") > 10                    # stuffed bytes
    coef = jo.coefficients(img, 100, "4:4:4")
    assert np.abs(coef[:, :, 1:]).max() >= 512             # category-10 AC values: 16-bit codes + 10 extra bits
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert data == pillow(img, 100, "4:4:4", 32)


def test_intervals_split_and_reassemble():
    rng = np.random.default_rng(4)
    for (w, h, sub, R) in [(101, 77, "4:2:0", 3), (101, 77, "4:4:4", 5), (64, 33, "4:2:0", 1), (17, 9, "4:2:0", 32)]:
        img = frame(rng, h, w, "noise")
        hdr, parts, tail = jo.split_scan(jo.encode(img, 75, sub, R))
        assert hdr == jo.header(w, h, 75, sub, R) and tail == b"\xff\xd9"
        assert len(parts) == jo.n_intervals(w, h, sub, R)
        for r in range(len(parts)):
            assert parts[r] == jo.encode_interval(img, r, 75, sub, R)


def test_alpha_is_ignored():
    rng = np.random.default_rng(5)
    rgb = frame(rng, 19, 23, "smooth")
    rgba = np.concatenate([rgb, rng.integers(0, 256, (19, 23, 1), dtype=np.uint8)], -1)
    assert jo.encode(rgba, 90) == jo.encode(rgb, 90)


def test_pillow_decodes_the_oracle_within_jpeg_error():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(6)
    img = frame(rng, 301, 453, "smooth")
    for q, bound in ((90, 34.0), (75, 31.0), (50, 29.0)):
        dec = np.asarray(Image.open(io.BytesIO(jo.encode(img, q, "4:2:0", 32))).convert("RGB")).astype(np.float64)
        mse = float(np.mean((dec - img) ** 2))
        psnr = 10 * np.log10(255.0 ** 2 / mse)
        assert psnr > bound, (q, psnr)
    assert PIL is not None


# ---- the library's header ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES + [(6016, 4016), (6001, 4001), (65535, 65535)])
def test_library_header_equals_the_oracle(W, H):
    for q in QUALITIES:
        for sub in ("4:2:0", "4:4:4"):
            for R in (1, 7, 32, 65535):
                assert ra.jpeg_header(W, H, q, sub, R) == jo.header(W, H, q, sub, R), (W, H, q, sub, R)


def test_header_marker_order():
    h = jo.header(640, 427, 90, "4:2:0", 32)
    markers, i = [], 2
    while i < len(h):
        markers.append(h[i + 1])
        i += 2 + int.from_bytes(h[i + 2:i + 4], "big")
    assert h[:2] == b"\xff\xd8"
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]


# ---- the reciprocal quantiser --------------------------------------------------------------------------------------------
def test_reciprocal_quantiser_equals_the_division_exhaustively():
    """rd_jpeg_dct quantises |x| as umulhi(|x| + 4q, ceil(2^32 / 8q)); the contract is (|x| + 4q) // 8q.  Every |x| < 2^15
    and every q in 1..255 (8.4 M pairs of each sign; the sign is restored after)."""
    x = np.arange(1 << 15, dtype=np.uint64)
    for q in range(1, 256):
        d = np.uint64(8 * q)
        m = np.uint64(((1 << 32) + 8 * q - 1) // (8 * q))
        n = x + np.uint64(4 * q)
        got = (n * m) >> np.uint64(32)                     # n < 2^16, m < 2^30: the product fits 64 bits
        assert np.array_equal(got, n // d), q


# ---- argument errors through the C ABI (a child process: nothing may throw) ---------------------------------------------
_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from raweditor_amd import _lib
L = _lib.lib()
out = {}
def rec(name, rc):
    out[name] = [rc, L.rd_last_error().decode()]
h = C.c_void_p(123)
rec("bad_format", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGBA_F32, 90, 0, 32, C.byref(h)))
out["bad_format_out_cleared"] = h.value is None
rec("bad_format_f16", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGBA_F16, 90, 0, 32, C.byref(h)))
rec("quality_0", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGB_U8, 0, 0, 32, C.byref(h)))
rec("quality_101", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGB_U8, 101, 0, 32, C.byref(h)))
rec("bad_sub", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGB_U8, 90, 2, 32, C.byref(h)))
rec("restart_0", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGB_U8, 90, 0, 0, C.byref(h)))
rec("restart_big", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGB_U8, 90, 0, 65536, C.byref(h)))
rec("empty", L.rd_jpeg_create(0, 0, 48, _lib.FMT_RGB_U8, 90, 0, 32, C.byref(h)))
rec("too_big", L.rd_jpeg_create(0, 65536, 48, _lib.FMT_RGB_U8, 90, 0, 32, C.byref(h)))
rec("null_out", L.rd_jpeg_create(0, 64, 48, _lib.FMT_RGB_U8, 90, 0, 32, None))
rec("encode_null_ctx", L.rd_jpeg_encode(None, None, 1, 192, None, 1 << 20, None, None))
rec("info_null", L.rd_jpeg_info(None, None, None))
n = C.c_size_t()
rec("header_null_len", L.rd_jpeg_header(64, 48, 90, 0, 32, None, 0, None))
rec("header_quality", L.rd_jpeg_header(64, 48, 0, 0, 32, None, 0, C.byref(n)))
buf = (C.c_uint8 * 16)()
rec("header_small", L.rd_jpeg_header(64, 48, 90, 0, 32, buf, 16, C.byref(n)))
out["header_need"] = n.value
rec("header_sizing", L.rd_jpeg_header(64, 48, 90, 0, 32, None, 0, C.byref(n)))
L.rd_jpeg_destroy(None)
print(json.dumps(out))
"""


def test_argument_errors_are_statuses_in_a_child_process():
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    INV, UNS = _lib.RD_ERR_INVALID_ARG, _lib.RD_ERR_UNSUPPORTED
    want = {"bad_format": UNS, "bad_format_f16": UNS, "quality_0": INV, "quality_101": INV, "bad_sub": INV, "restart_0": INV,
            "restart_big": INV, "empty": INV, "too_big": INV, "null_out": INV, "encode_null_ctx": INV, "info_null": INV,
            "header_null_len": INV, "header_quality": INV, "header_small": INV}
    for k, code in want.items():
        rc, msg = r[k]
        assert rc == code, (k, rc, msg)
        assert msg, k                                              # rd_last_error says why
    assert r["header_sizing"][0] == _lib.RD_OK
    assert r["bad_format_out_cleared"]
    assert "format" in r["bad_format"][1] and "quality" in r["quality_0"][1] and "restart" in r["restart_0"][1]
    assert r["header_need"] == len(jo.header(64, 48, 90, "4:2:0", 32))


def test_every_new_entry_point_is_declared_bound_and_a_function_try_block():
    import re
    names = ("rd_jpeg_header", "rd_jpeg_create", "rd_jpeg_destroy", "rd_jpeg_info", "rd_jpeg_encode")
    header = open(os.path.join(ROOT, "include", "rawdev.h")).read()
    src = open(os.path.join(ROOT, "raweditor_amd", "csrc", "rd_host_jpeg.inl")).read()
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
        assert re.search(r'extern "C" [^;{]*\b' + name + r"\([^{]*\)\s*try\s*\{", src), name
        assert re.search(r"RD_CATCH_(INT|VOID)\(" + name + r"\)", src), name
    assert '"jpeg.scratch"' in src and '"jpeg.launch"' in src
    assert "jpeg.scratch" in header and "jpeg.launch" in header
    assert _lib.lib().rd_abi_version() == 5


# ---- catalog ----------------------------------------------------------------------------------------------------------
def test_write_catalog_tier_jpegs(tmp_path):
    conn = sqlite3.connect(tmp_path / "library.db")
    catalog.init_schema(conn)
    conn.execute("INSERT INTO images (path, filename, width, height, imported_at) VALUES (?,?,?,?,?)",
                 ("/photos/0.dng", "0.dng", 6016, 4016, 0))
    conn.commit()
    rng = np.random.default_rng(7)
    files = [jo.encode(frame(rng, h, w, "smooth"), 90) for w, h in [(256, 171), (384, 256), (1280, 854)]]
    paths = ra.write_catalog_tier_jpegs(conn, 1, files, str(tmp_path / "cache"))
    assert paths == tuple(str(tmp_path / "cache" / n / "1.jpg") for n in ("thumb", "instant", "working"))
    for p, f in zip(paths, files):
        assert open(p, "rb").read() == f
    row = conn.execute("SELECT cache_status, cache_path_thumb, cache_path_instant, cache_path_working FROM images WHERE id = 1").fetchone()
    assert row == ("cached",) + paths
    with pytest.raises(ValueError):
        ra.write_catalog_tier_jpegs(conn, 1, files[:2], str(tmp_path / "cache"))


# ---- kernel resources -------------------------------------------------------------------------------------------------
def test_jpeg_kernels_use_no_scratch_and_do_not_spill():
    res = load_resources()
    for kname in ("rd_jpeg_dct", "rd_jpeg_huff", "rd_jpeg_concat"):
        names = [k for k in res if kname in k]
        assert len(names) == 1, (kname, names)
        r = res[names[0]]
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spills", 0) == 0 and r.get("sgpr_spills", 0) == 0, (kname, r)
