"""Cache tiers: a frame developed from its CFA plane and resampled by Lanczos3 into the Library grid's and the Develop view's
images (reference src/raw/processor.rs:13-15, :67-88 makes them from the embedded JPEG with image::imageops::resize).

The numerical contract is DESIGN.md section 11: the source is the frame's RGBA8 export codes, the tier size is resize's fit
rule, the weights come from the host tables rd_tier_weights returns, the horizontal pass runs first, everything is f32
without contraction and each byte is round_half_away(clamp(v, 0, 255)).  Every pixel is computed by HIP kernels inside
librawdev (rd_tiers_develop); there is no host path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Sequence, Tuple

from . import _lib
from ._lib import RdFrame, check
from .edit import EditParams

# processor.rs:13-15: (max width, max height) of the thumb, instant and working tiers; resize is called as (t, 10 t)
REFERENCE_TIERS: Tuple[Tuple[int, int], ...] = ((256, 2560), (384, 3840), (1280, 12800))
TIER_NAMES = ("thumb", "instant", "working")


def tier_dims(width: int, height: int, box_w: int, box_h: int) -> Tuple[int, int]:
    """(w, h) of a width x height frame's tier in a box_w x box_h box (rd_tier_dims)."""
    w, h = C.c_uint32(), C.c_uint32()
    check(_lib.lib().rd_tier_dims(int(width), int(height), int(box_w), int(box_h), C.byref(w), C.byref(h)))
    return w.value, h.value


def tier_weights(n_in: int, n_out: int):
    """The tables of one pass n_in -> n_out as the kernels use them: (left, count, w) numpy arrays; output j takes
    samples left[j] .. left[j] + count[j] - 1 with w[sum(count[:j]) ..] (rd_tier_weights)."""
    import numpy as np
    need = C.c_size_t()
    L = _lib.lib()
    check(L.rd_tier_weights(int(n_in), int(n_out), None, None, None, 0, C.byref(need)))
    left = np.zeros(int(n_out), np.uint32)
    count = np.zeros(int(n_out), np.uint32)
    w = np.zeros(max(need.value, 1), np.float32)
    check(L.rd_tier_weights(int(n_in), int(n_out), left.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                            w.ctypes.data_as(C.c_void_p), w.size, C.byref(need)))
    return left, count, w[:need.value]


class TierRenderer:
    """rd_tiers: develop + Lanczos3 tiers for frames of one size on one device, one stream per renderer."""

    def __init__(self, device: int, width: int, height: int, boxes: Sequence[Tuple[int, int]] = REFERENCE_TIERS,
                 fmt: int = _lib.FMT_RGBA_U8):
        self._h = C.c_void_p()
        self.device, self.width, self.height, self.fmt = int(device), int(width), int(height), int(fmt)
        self.boxes = [(int(bw), int(bh)) for bw, bh in boxes]
        n = len(self.boxes)
        bw = (C.c_uint32 * max(n, 1))(*[b[0] for b in self.boxes])
        bh = (C.c_uint32 * max(n, 1))(*[b[1] for b in self.boxes])
        check(_lib.lib().rd_tiers_create(self.device, self.width, self.height, self.fmt, n, bw, bh, C.byref(self._h)))
        self.dims = []
        for k in range(n):
            w, h = C.c_uint32(), C.c_uint32()
            check(_lib.lib().rd_tiers_info(self._h, k, C.byref(w), C.byref(h)))
            self.dims.append((w.value, h.value))

    @property
    def channels(self) -> int:
        return 4 if self.fmt == _lib.FMT_RGBA_U8 else 3

    def tier_bytes(self, k: int) -> int:
        w, h = self.dims[k]
        return w * h * self.channels

    def develop(self, frames, tier_ptrs: Sequence[int], stream: int = 0) -> None:
        """Enqueue frames (an RdFrame array, e.g. BatchExporter.make_frames; out_dev is ignored) on `stream`; tier_ptrs holds
        len(frames) x n_tiers device pointers, frame-major.  Not synchronised."""
        n = len(frames) * len(self.dims)
        if len(tier_ptrs) != n:
            raise ValueError(f"{len(tier_ptrs)} tier pointers for {len(frames)} frames x {len(self.dims)} tiers")
        arr = (C.c_void_p * max(n, 1))(*[int(p) for p in tier_ptrs])
        check(_lib.lib().rd_tiers_develop(self._h, frames, len(frames), arr, C.c_void_p(stream) if stream else None))

    def close(self) -> None:
        if self._h:
            _lib.lib().rd_tiers_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def render_tiers(cfa, width: int, height: int, params: EditParams, wb, cm, black_level: int = 0,
                 boxes: Sequence[Tuple[int, int]] = REFERENCE_TIERS, fmt: int = _lib.FMT_RGBA_U8, device: int = 0,
                 matrix_layout: int = _lib.MATRIX_REFERENCE) -> List:
    """One frame's tiers from its host CFA plane (height x width u16): a list of (h, w, c) uint8 arrays, c = 4 (RGBA8) or
    3 (RGB8), in the order of `boxes`."""
    import numpy as np
    cfa = np.ascontiguousarray(np.asarray(cfa, np.uint16).reshape(int(height), int(width)))
    L = _lib.lib()
    r = TierRenderer(device, width, height, boxes, fmt)
    bufs = []
    try:
        cfa_dev = C.c_void_p()
        check(L.rd_device_malloc(device, cfa.nbytes, C.byref(cfa_dev)))
        bufs.append(cfa_dev)
        check(L.rd_memcpy_h2d(device, cfa_dev, cfa.ctypes.data_as(C.c_void_p), cfa.nbytes))
        outs = []
        for k in range(len(r.dims)):
            p = C.c_void_p()
            check(L.rd_device_malloc(device, r.tier_bytes(k), C.byref(p)))
            bufs.append(p)
            outs.append(p)
        frames = (RdFrame * 1)()
        frames[0].cfa_dev = cfa_dev.value
        frames[0].out_dev = None
        frames[0].params = params.to_c()
        frames[0].wb_multipliers[:] = [float(x) for x in wb]
        frames[0].color_matrix[:] = [float(x) for x in cm]
        frames[0].black_level = int(black_level)
        frames[0].matrix_layout = int(matrix_layout)
        r.develop(frames, [p.value for p in outs])
        check(L.rd_device_synchronize(device))
        result = []
        for k, p in enumerate(outs):
            w, h = r.dims[k]
            a = np.empty((h, w, r.channels), np.uint8)
            check(L.rd_memcpy_d2h(device, a.ctypes.data_as(C.c_void_p), p, a.nbytes))
            result.append(a)
        return result
    finally:
        for p in bufs:
            L.rd_device_free(device, p)
        r.close()


def write_catalog_tiers(conn, image_id: int, tiers: Sequence, cache_root: str, quality: int = 90) -> Tuple[str, str, str]:
    """Store three tiers (thumb, instant, working: (h, w, 3|4) uint8 arrays, as render_tiers returns them) as
    {cache_root}/{thumb,instant,working}/{image_id}.jpg and record the paths (catalog.set_image_cache_paths).  The JPEG
    encoder is Pillow's; the library has none of its own."""
    from . import catalog
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("write_catalog_tiers needs Pillow to encode JPEG files (pip install Pillow); "
                           "the tiers themselves are plain arrays") from e
    if len(tiers) != 3:
        raise ValueError(f"three tiers (thumb, instant, working) expected, got {len(tiers)}")
    paths = []
    for name, a in zip(TIER_NAMES, tiers):
        d = os.path.join(cache_root, name)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"{int(image_id)}.jpg")
        rgb = a[:, :, :3] if a.ndim == 3 and a.shape[2] == 4 else a      # JPEG has no alpha (main.rs strips it too)
        Image.fromarray(rgb.copy(), "RGB").save(path, "JPEG", quality=int(quality))
        paths.append(path)
    catalog.set_image_cache_paths(conn, image_id, *paths)
    return tuple(paths)


def render_tier_jpegs(cfa, width: int, height: int, params: EditParams, wb, cm, black_level: int = 0, quality: int = 90,
                      subsampling="4:2:0", restart_mcus: int = 32, device: int = 0,
                      matrix_layout: int = _lib.MATRIX_REFERENCE) -> Tuple[bytes, bytes, bytes]:
    """One frame's three reference tiers (thumb, instant, working) as JPEG files, made on the device: rd_tiers_develop into
    RGB8 surfaces, then rd_jpeg_encode (DESIGN.md sections 11 and 12).  The bytes are the ones libjpeg's default path
    writes for render_tiers(..., fmt=FMT_RGB_U8)'s arrays."""
    import numpy as np
    from .jpeg import JpegEncoder, encode_device
    cfa = np.ascontiguousarray(np.asarray(cfa, np.uint16).reshape(int(height), int(width)))
    L = _lib.lib()
    r = TierRenderer(device, width, height, REFERENCE_TIERS, _lib.FMT_RGB_U8)
    bufs = []
    try:
        cfa_dev = C.c_void_p()
        check(L.rd_device_malloc(device, cfa.nbytes, C.byref(cfa_dev)))
        bufs.append(cfa_dev)
        check(L.rd_memcpy_h2d(device, cfa_dev, cfa.ctypes.data_as(C.c_void_p), cfa.nbytes))
        outs = []
        for k in range(len(r.dims)):
            p = C.c_void_p()
            check(L.rd_device_malloc(device, r.tier_bytes(k), C.byref(p)))
            bufs.append(p)
            outs.append(p)
        frames = (RdFrame * 1)()
        frames[0].cfa_dev = cfa_dev.value
        frames[0].out_dev = None
        frames[0].params = params.to_c()
        frames[0].wb_multipliers[:] = [float(x) for x in wb]
        frames[0].color_matrix[:] = [float(x) for x in cm]
        frames[0].black_level = int(black_level)
        frames[0].matrix_layout = int(matrix_layout)
        r.develop(frames, [p.value for p in outs])              # the same (null) stream as the encodes below
        files = []
        for k, p in enumerate(outs):
            w, h = r.dims[k]
            enc = JpegEncoder(device, w, h, _lib.FMT_RGB_U8, quality, subsampling, restart_mcus)
            try:
                files.append(encode_device(enc, [p])[0])
            finally:
                enc.close()
        return tuple(files)
    finally:
        for p in bufs:
            L.rd_device_free(device, p)
        r.close()


def write_catalog_tier_jpegs(conn, image_id: int, jpegs: Sequence[bytes], cache_root: str) -> Tuple[str, str, str]:
    """Store three JPEG files (thumb, instant, working, as render_tier_jpegs returns them) at the paths write_catalog_tiers
    uses, {cache_root}/{thumb,instant,working}/{image_id}.jpg, and record them (catalog.set_image_cache_paths)."""
    from . import catalog
    if len(jpegs) != 3:
        raise ValueError(f"three JPEG files (thumb, instant, working) expected, got {len(jpegs)}")
    paths = []
    for name, data in zip(TIER_NAMES, jpegs):
        if not bytes(data[:2]) == b"\xff\xd8":
            raise ValueError(f"the {name} tier is not a JPEG file")
        d = os.path.join(cache_root, name)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"{int(image_id)}.jpg")
        with open(path, "wb") as f:
            f.write(bytes(data))
        paths.append(path)
    catalog.set_image_cache_paths(conn, image_id, *paths)
    return tuple(paths)
