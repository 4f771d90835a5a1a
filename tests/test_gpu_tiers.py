"""GPU: the cache tiers (rd_tiers_*) byte for byte against the numpy oracle (tests/tier_oracle.py) run on the frame's RGBA8
export codes, with the library's own weight tables."""
import ctypes as C

import numpy as np
import pytest

from raweditor_amd import _lib
from raweditor_amd._lib import check
from tests import tier_oracle as to
from tests.gpu_util import DevBuf
from tests.helpers import CM_IDENTITY, CM_TEST, WB_DAYLIGHT, mild_params, random_params

pytestmark = pytest.mark.gpu


def sync():
    check(_lib.lib().rd_device_synchronize(0))


def expected_tiers(refc, cfa, params, wb, cm, dims, black_level=0, rgba=True, codes=None):
    if codes is None:
        u = refc.make_uniforms(params, wb, cm, black_level=black_level)
        codes = refc.pack_u8(refc.render_f32(cfa, u))
    H, W = codes.shape[:2]
    out = []
    for tw, th in dims:
        hx = to_tables(W, tw)
        vy = to_tables(H, th)
        out.append(to.tier_surface(to.resample(codes, tw, th, hx, vy), rgba))
    return out


_TABLES = {}


def to_tables(n_in, n_out):
    import raweditor_amd as ra
    key = (n_in, n_out)
    if key not in _TABLES:
        _TABLES[key] = ra.tier_weights(n_in, n_out)
    return _TABLES[key]


def run_tiers(ra, W, H, boxes, fmt, frames_in, stream=0, renderer=None):
    """frames_in: list of (cfa, params dict, wb, cm, black_level).  Returns per frame a list of tier arrays."""
    r = renderer or ra.TierRenderer(0, W, H, boxes, fmt)
    d_in = [DevBuf.from_array(f[0]) for f in frames_in]
    outs = [[DevBuf(max(r.tier_bytes(k), 1)) for k in range(len(r.dims))] for _ in frames_in]
    frames = ra.BatchExporter.make_frames([b.ptr for b in d_in], [0] * len(d_in), [ra.EditParams(**f[1]) for f in frames_in],
                                          WB_DAYLIGHT, CM_IDENTITY)
    for fr, f in zip(frames, frames_in):
        fr.wb_multipliers[:] = [float(x) for x in f[2]]
        fr.color_matrix[:] = [float(x) for x in f[3]]
        fr.black_level = int(f[4])
    r.develop(frames, [o.ptr for per in outs for o in per], stream)
    return r, d_in, outs


def fetch(r, outs):
    res = []
    for per in outs:
        res.append([o.to_array(np.uint8, (h, w, r.channels)) for o, (w, h) in zip(per, r.dims)])
    return res


SMALL = [(64, 48), (65, 47), (131, 7), (7, 131), (1, 1), (2, 3), (3, 2), (97, 5), (600, 401), (1024, 9), (133, 134)]


@pytest.mark.parametrize("W,H", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
def test_tiers_small_frames_match_the_oracle(gpu_lib, refc, W, H):
    ra = gpu_lib
    rng = np.random.default_rng(W * 1000 + H)
    for fmt in (ra.FMT_RGBA_U8, ra.FMT_RGB_U8):
        n_t = int(rng.integers(1, 5))
        pool = list(ra.REFERENCE_TIERS) + [(17, 23), (W * 3, H * 3), (5, 500), (W, H), (1, 1), (int(rng.integers(1, 300)), 40)]
        boxes = [pool[int(i)] for i in rng.choice(len(pool), n_t, replace=False)]
        frames_in = []
        for k in range(3):
            cfa = rng.integers(0, 4096, (H, W), dtype=np.uint16)
            p = random_params(rng) if k == 0 else mild_params(rng)
            frames_in.append((cfa, p, WB_DAYLIGHT, CM_TEST if k == 1 else CM_IDENTITY, (0, 64, 300)[k]))
        r, d_in, outs = run_tiers(ra, W, H, boxes, fmt, frames_in)
        sync()
        got = fetch(r, outs)
        for f, g in zip(frames_in, got):
            want = expected_tiers(refc, f[0], f[1], f[2], f[3], r.dims, black_level=f[4], rgba=fmt == ra.FMT_RGBA_U8)
            for k, (a, b) in enumerate(zip(g, want)):
                assert np.array_equal(a, b), (W, H, fmt, boxes[k], int((a != b).sum()))
        r.close()


def test_heterogeneous_multi_frame_call_spans_launches(gpu_lib, refc):
    """More frames than one launch takes (RD_TIERS_LAUNCH_MAX = 8), each with its own stack, black level and matrix."""
    ra = gpu_lib
    rng = np.random.default_rng(11)
    W, H = 157, 93
    frames_in = []
    for k in range(19):
        cfa = rng.integers(0, 4096, (H, W), dtype=np.uint16)
        frames_in.append((cfa, random_params(rng) if k % 3 == 0 else mild_params(rng), tuple(rng.uniform(0.5, 2.5, 4)),
                          CM_TEST if k % 2 else CM_IDENTITY, int(rng.integers(0, 200))))
    r, d_in, outs = run_tiers(ra, W, H, [(64, 640), (200, 2000), (31, 9)], ra.FMT_RGBA_U8, frames_in)
    sync()
    for f, g in zip(frames_in, fetch(r, outs)):
        want = expected_tiers(refc, f[0], f[1], tuple(np.float32(f[2])), f[3], r.dims, black_level=f[4])
        for a, b in zip(g, want):
            assert np.array_equal(a, b)
    r.close()


def test_two_contexts_on_two_streams_interleaved(gpu_lib, refc):
    ra = gpu_lib
    L = _lib.lib()
    rng = np.random.default_rng(12)
    s = [C.c_void_p(), C.c_void_p()]
    for x in s:
        check(L.rd_stream_create(0, C.byref(x)))
    specs = [(320, 211, [(256, 2560), (96, 960)], ra.FMT_RGBA_U8), (301, 200, [(384, 3840)], ra.FMT_RGB_U8)]
    runs = []
    for rep in range(3):
        for k, (W, H, boxes, fmt) in enumerate(specs):
            frames_in = [(rng.integers(0, 4096, (H, W), dtype=np.uint16), mild_params(rng), WB_DAYLIGHT, CM_IDENTITY, 0)
                         for _ in range(2)]
            r = runs[k][0] if rep else None
            r, d_in, outs = run_tiers(ra, W, H, boxes, fmt, frames_in, stream=s[k].value, renderer=r)
            if rep == 0:
                runs.append((r, []))
            runs[k][1].append((frames_in, d_in, outs))
    for x in s:
        check(L.rd_stream_synchronize(0, x))
    for r, calls in runs:
        for frames_in, d_in, outs in calls:
            for f, g in zip(frames_in, fetch(r, outs)):
                want = expected_tiers(refc, f[0], f[1], f[2], f[3], r.dims, rgba=r.fmt == ra.FMT_RGBA_U8)
                for a, b in zip(g, want):
                    assert np.array_equal(a, b)
        r.close()
    for x in s:
        check(L.rd_stream_destroy(0, x))


@pytest.mark.parametrize("site", ["tiers.tables", "tiers.launch", "rd_tiers_develop"])
def test_injected_fault_leaves_the_context_usable(gpu_lib, refc, site):
    ra = gpu_lib
    rng = np.random.default_rng(13)
    W, H = 90, 61
    frames_in = [(rng.integers(0, 4096, (H, W), dtype=np.uint16), mild_params(rng), WB_DAYLIGHT, CM_IDENTITY, 0)]
    if site == "tiers.tables":
        _lib.inject_fault(site, _lib.FAULT_BAD_ALLOC)
        with pytest.raises(ra.RawdevError) as e:
            ra.TierRenderer(0, W, H, ra.REFERENCE_TIERS, ra.FMT_RGBA_U8)
        assert e.value.code == _lib.RD_ERR_OOM
        r = ra.TierRenderer(0, W, H, ra.REFERENCE_TIERS, ra.FMT_RGBA_U8)
    else:
        r = ra.TierRenderer(0, W, H, ra.REFERENCE_TIERS, ra.FMT_RGBA_U8)
        _lib.inject_fault(site, _lib.FAULT_RUNTIME)
        with pytest.raises(ra.RawdevError) as e:
            run_tiers(ra, W, H, None, None, frames_in, renderer=r)
        assert e.value.code == _lib.RD_ERR_INTERNAL
    _lib.inject_fault(None, 0)
    _, d_in, outs = run_tiers(ra, W, H, None, None, frames_in, renderer=r)
    sync()
    want = expected_tiers(refc, *frames_in[0][:4], r.dims)
    for a, b in zip(fetch(r, outs)[0], want):
        assert np.array_equal(a, b)
    r.close()


def test_render_tiers_convenience(gpu_lib, refc):
    ra = gpu_lib
    rng = np.random.default_rng(14)
    W, H = 211, 150
    cfa = rng.integers(0, 4096, (H, W), dtype=np.uint16)
    p = mild_params(rng)
    got = ra.render_tiers(cfa, W, H, ra.EditParams(**p), WB_DAYLIGHT, CM_TEST, black_level=40, fmt=ra.FMT_RGB_U8)
    dims = [ra.tier_dims(W, H, *b) for b in ra.REFERENCE_TIERS]
    want = expected_tiers(refc, cfa, p, WB_DAYLIGHT, CM_TEST, dims, black_level=40, rgba=False)
    assert [g.shape for g in got] == [(h, w, 3) for w, h in dims]
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


from tests.test_wgsl_pin_cpu import FULL, fullsize_check, fullsize_inputs  # noqa: E402


def _full_sizes():
    seen = {}
    for fr in FULL["frames"]:
        seen.setdefault((fr["w"], fr["h"]), []).append(fr)
    return sorted(seen.items())


@pytest.mark.parametrize("size,group", _full_sizes(), ids=[f"{s[0]}x{s[1]}" for s, _ in _full_sizes()])
def test_full_size_frames_reference_tiers(gpu_lib, size, group):
    """The frames of tests/golden/wgsl_fullsize.json at full size: the RGBA8 export is first checked against its pinned SHA-256,
    then the three reference tiers against the oracle run on that export."""
    ra = gpu_lib
    W, H = size
    cfas = [fullsize_inputs(fr) for fr in group]
    d_in = [DevBuf.from_array(c) for c in cfas]
    d_out = [DevBuf(W * H * 4) for _ in group]
    be = ra.BatchExporter(0, W, H, ra.FMT_RGBA_U8, False)
    frames = be.make_frames([b.ptr for b in d_in], [b.ptr for b in d_out], [ra.EditParams(**fr["params"]) for fr in group],
                            FULL["wb"], group[0]["cm"])
    for f, fr in zip(frames, group):
        f.color_matrix[:] = fr["cm"]
    be.develop(frames)
    r = ra.TierRenderer(0, W, H, ra.REFERENCE_TIERS, ra.FMT_RGBA_U8)
    outs = [[DevBuf(r.tier_bytes(k)) for k in range(3)] for _ in group]
    r.develop(frames, [o.ptr for per in outs for o in per])
    sync()
    got = fetch(r, outs)
    for fr, o, g in zip(group, d_out, got):
        codes = o.to_array(np.uint8, (H, W, 4))
        fullsize_check(fr, rgba8=codes)
        want = expected_tiers(None, None, None, None, None, r.dims, codes=codes)
        for k, (a, b) in enumerate(zip(g, want)):
            assert np.array_equal(a, b), (fr["name"], k, int((a != b).sum()))
    be.close()
    r.close()
