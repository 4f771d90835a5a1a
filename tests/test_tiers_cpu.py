"""CPU: the cache tiers' host side -- tier sizes, the weight tables, the numpy oracle's own
properties, argument errors through the C ABI, the catalog statement and the new kernels' resources.  No GPU needed."""
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
from tests import tier_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tier size ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,want", [
    (6016, 4016, [(256, 171), (384, 256), (1280, 854)]),
    (4016, 6016, [(256, 383), (384, 575), (1280, 1917)]),
    (11648, 8736, [(256, 192), (384, 288), (1280, 960)]),
])
def test_tier_dims_reference_examples(W, H, want):
    assert [ra.tier_dims(W, H, bw, bh) for bw, bh in ra.REFERENCE_TIERS] == want
    assert [to.tier_dims(W, H, bw, bh) for bw, bh in to.REFERENCE_TIERS] == want
    assert tuple(ra.REFERENCE_TIERS) == tuple(to.REFERENCE_TIERS)


def test_tier_dims_edges():
    assert ra.tier_dims(1, 1, 256, 2560) == (256, 256)             # a 1 x 1 frame is upscaled to the box's limiting side
    assert ra.tier_dims(100, 50, 256, 2560) == (256, 128)          # upscaling
    assert ra.tier_dims(256, 171, 256, 2560) == (256, 171)         # equal size
    assert ra.tier_dims(10000, 3, 256, 2560) == (256, 1)           # a side that would round to 0 is 1
    assert ra.tier_dims(3, 10000, 2560, 256) == (1, 256)
    rng = np.random.default_rng(7)
    for _ in range(300):
        W, H, bw, bh = (int(v) for v in rng.integers(1, 20000, 4))
        assert ra.tier_dims(W, H, bw, bh) == to.tier_dims(W, H, bw, bh), (W, H, bw, bh)
    for bad in [(0, 10, 5, 5), (10, 0, 5, 5), (10, 10, 0, 5), (10, 10, 5, 0)]:
        with pytest.raises(ra.RawdevError) as e:
            ra.tier_dims(*bad)
        assert e.value.code == _lib.RD_ERR_INVALID_ARG


# ---- weights ---------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("n_in,n_out", [(6016, 256), (6016, 384), (6016, 1280), (4016, 171), (8736, 960), (11648, 1280),
                                        (7, 3), (5, 17), (100, 256), (1, 1), (1, 7), (9, 9), (171, 171), (3, 1), (16384, 1)])
def test_tier_weights_match_an_independent_computation(n_in, n_out):
    left, count, w = ra.tier_weights(n_in, n_out)
    l2, c2, w2 = to.weights(n_in, n_out)
    assert np.array_equal(left, l2) and np.array_equal(count, c2)
    assert w.shape == w2.shape and int(_ulps(w, w2).max()) <= 1
    # bounds: every window is non-empty and inside [0, n_in)
    assert (count >= 1).all() and (left.astype(np.int64) + count <= n_in).all()
    # each output's weights sum to 1 (f32, ascending): within 4 ulp for the short windows of upscaling and equal sizes, and
    # within the textbook bound of a rounded sum, count x 2^-24, for the long ones (measured: 8 ulp at 142 taps)
    off = 0
    for c in count:
        s = np.float32(0)
        for v in w[off:off + c]:
            s = np.float32(s + v)
        d = abs(int(np.float32(s).view(np.int32)) - int(np.float32(1).view(np.int32)))
        assert d <= max(4, int(c)) and (c > 8 or d <= 4), (c, d)
        off += int(c)


def test_tier_weights_tap_counts():
    for n_out, lo, hi in [(256, 83, 142), (1280, 17, 30)]:
        c = ra.tier_weights(6016, n_out)[1]
        assert (int(c.min()), int(c.max())) == (lo, hi)
    assert 4 <= int(ra.tier_weights(100, 256)[1].min()) and int(ra.tier_weights(100, 256)[1].max()) <= 7


# ---- the oracle on its own ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,tw,th", [(40, 60, 17, 11), (9, 13, 30, 21), (5, 3, 1, 1), (64, 96, 64, 96)])
def test_oracle_constant_image_comes_back(H, W, tw, th):
    for v in (0, 1, 77, 128, 254, 255):
        codes = np.full((H, W, 4), v, np.uint8)
        got = to.resample(codes, tw, th)
        assert got.shape == (th, tw, 3) and (got == v).all(), v


def test_oracle_equal_size_gives_the_codes_back(refc, rng):
    from tests.helpers import random_params, random_cfa, WB_DAYLIGHT, CM_TEST
    cfa = random_cfa(rng, 37, 53)
    codes = refc.pack_u8(refc.render_f32(cfa, refc.make_uniforms(random_params(rng), WB_DAYLIGHT, CM_TEST)))
    assert np.array_equal(to.resample(codes, 53, 37), codes[:, :, :3])
    left, count, w = ra.tier_weights(53, 53)                       # an equal-size pass is not the identity table,
    assert count.max() > 1                                         # but it reproduces integer codes exactly


def test_vertical_first_differs_from_horizontal_first_by_at_most_one_code(refc):
    """The figure DESIGN.md section 11 records: how often the image crate's order (vertical pass first) would give another
    byte than the pinned horizontal-first order, on developed frames."""
    from tests.helpers import mild_params, random_cfa, WB_DAYLIGHT, CM_IDENTITY
    rng = np.random.default_rng(0x54494552)
    n = diff = 0
    for _ in range(3):
        H, W = 301, 452
        cfa = random_cfa(rng, H, W)
        codes = refc.pack_u8(refc.render_f32(cfa, refc.make_uniforms(mild_params(rng), WB_DAYLIGHT, CM_IDENTITY)))
        for bw, bh in ((256, 2560), (384, 3840), (97, 970)):
            tw, th = to.tier_dims(W, H, bw, bh)
            a = to.resample(codes, tw, th)
            b = to.resample(codes, tw, th, vertical_first=True)
            d = np.abs(a.astype(np.int16) - b.astype(np.int16))
            assert d.max() <= 1
            n += a.size; diff += int((d != 0).sum())
    frac = diff / n
    print(f"vertical-first vs horizontal-first: {diff} of {n} bytes differ by one code ({frac:.2e})")
    assert frac < 0.02


# ---- argument errors through the C ABI (a child process: nothing may throw) --------------------------------
_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from raweditor_amd import _lib
L = _lib.lib()
out = {}
def rec(name, rc):
    out[name] = [rc, L.rd_last_error().decode()]
bw = (C.c_uint32 * 5)(256, 384, 1280, 64, 32); bh = (C.c_uint32 * 5)(2560, 3840, 12800, 640, 320)
zero = (C.c_uint32 * 2)(256, 0)
h = C.c_void_p(123)
rec("bad_format", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGBA_F32, 3, bw, bh, C.byref(h)))
out["bad_format_out_cleared"] = h.value is None
rec("bad_format_f16", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGBA_F16, 3, bw, bh, C.byref(h)))
rec("zero_tiers", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGBA_U8, 0, bw, bh, C.byref(h)))
rec("five_tiers", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGBA_U8, 5, bw, bh, C.byref(h)))
rec("zero_box", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGB_U8, 2, bw, zero, C.byref(h)))
rec("null_boxes", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGBA_U8, 1, None, None, C.byref(h)))
rec("null_out", L.rd_tiers_create(0, 64, 48, _lib.FMT_RGBA_U8, 1, bw, bh, None))
rec("empty_frame", L.rd_tiers_create(0, 0, 48, _lib.FMT_RGBA_U8, 1, bw, bh, C.byref(h)))
rec("too_wide", L.rd_tiers_create(0, 40000, 48, _lib.FMT_RGBA_U8, 1, bw, bh, C.byref(h)))
rec("develop_null_ctx", L.rd_tiers_develop(None, None, 1, None, None))
rec("info_null", L.rd_tiers_info(None, 0, None, None))
w, hh = C.c_uint32(), C.c_uint32()
rec("dims_null", L.rd_tier_dims(10, 10, 5, 5, None, None))
rec("dims_zero_box", L.rd_tier_dims(10, 10, 0, 5, C.byref(w), C.byref(hh)))
need = C.c_size_t()
rec("weights_empty", L.rd_tier_weights(0, 5, None, None, None, 0, C.byref(need)))
rec("weights_null_need", L.rd_tier_weights(5, 3, None, None, None, 0, None))
buf = (C.c_float * 2)()
rec("weights_small", L.rd_tier_weights(50, 3, None, None, buf, 2, C.byref(need)))
out["weights_need"] = need.value
L.rd_tiers_destroy(None)
print(json.dumps(out))
"""


def test_argument_errors_are_statuses_in_a_child_process():
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    INV, UNS = _lib.RD_ERR_INVALID_ARG, _lib.RD_ERR_UNSUPPORTED
    want = {"bad_format": UNS, "bad_format_f16": UNS, "zero_tiers": INV, "five_tiers": INV, "zero_box": INV,
            "null_boxes": INV, "null_out": INV, "empty_frame": INV, "too_wide": UNS, "develop_null_ctx": INV, "info_null": INV,
            "dims_null": INV, "dims_zero_box": INV, "weights_empty": INV, "weights_null_need": INV, "weights_small": INV}
    for k, code in want.items():
        rc, msg = r[k]
        assert rc == code, (k, rc, msg)
        assert msg, k                                              # rd_last_error says why
    assert r["bad_format_out_cleared"]
    assert "format" in r["bad_format"][1] and "LDS" in r["too_wide"][1]
    assert r["weights_need"] > 2


def test_every_new_entry_point_is_declared_and_bound():
    for name in ("rd_tier_dims", "rd_tier_weights", "rd_tiers_create", "rd_tiers_destroy", "rd_tiers_info", "rd_tiers_develop"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().rd_abi_version() == 5


# ---- catalog --------------------------------------------------------------------------------------------------
def _catalog(tmp_path):
    conn = sqlite3.connect(tmp_path / "library.db")
    catalog.init_schema(conn)
    for k in range(2):
        conn.execute("INSERT INTO images (path, filename, width, height, imported_at) VALUES (?,?,?,?,?)",
                     (f"/photos/{k}.dng", f"{k}.dng", 6016, 4016, 0))
    conn.commit()
    return conn


def test_set_image_cache_paths(tmp_path):
    conn = _catalog(tmp_path)
    catalog.set_image_cache_paths(conn, 2, "/c/thumb/2.jpg", "/c/instant/2.jpg", "/c/working/2.jpg")
    rows = conn.execute("SELECT id, cache_status, cache_path_thumb, cache_path_instant, cache_path_working FROM images "
                        "ORDER BY id").fetchall()
    assert rows[0] == (1, "pending", None, None, None)
    assert rows[1] == (2, "cached", "/c/thumb/2.jpg", "/c/instant/2.jpg", "/c/working/2.jpg")


def test_write_catalog_tiers(tmp_path):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    conn = _catalog(tmp_path)
    rng = np.random.default_rng(3)
    tiers = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for (w, h), c in zip([(256, 171), (384, 256), (1280, 854)], (4, 4, 3))]
    paths = ra.write_catalog_tiers(conn, 1, tiers, str(tmp_path / "cache"))
    assert paths == tuple(str(tmp_path / "cache" / n / "1.jpg") for n in ("thumb", "instant", "working"))
    for p, t in zip(paths, tiers):
        with Image.open(p) as im:
            assert im.format == "JPEG" and im.size == (t.shape[1], t.shape[0]) and im.mode == "RGB"
    row = conn.execute("SELECT cache_status, cache_path_thumb, cache_path_working FROM images WHERE id = 1").fetchone()
    assert row == ("cached", paths[0], paths[2])
    assert PIL is not None


# ---- kernel resources -------------------------------------------------------------------------------------------
def test_tier_kernels_use_no_scratch_and_do_not_spill():
    res = load_resources()
    names = [k for k in res if "rd_tiers_hpass" in k or "rd_tiers_vpass" in k]
    assert any("rd_tiers_hpass" in k for k in names) and sum("rd_tiers_vpass" in k for k in names) == 2, names
    for k in names:
        r = res[k]
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spills", 0) == 0 and r.get("sgpr_spills", 0) == 0, (k, r)
