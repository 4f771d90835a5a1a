"""Baseline JPEG on the GPU: RGB8 / RGBA8 device surfaces -> JFIF files, libjpeg's default compression path byte for byte
(DESIGN.md section 12).  The reference encodes its exports (main.rs:1744-1799, image::save_buffer) and its cache tiers
(raw/processor.rs:67-88) as JPEG on the CPU; here every byte of the entropy-coded data is made by HIP kernels inside
librawdev (rd_jpeg_encode); the host only builds the header and the tables once per context.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

from . import _lib
from ._lib import check

SUBSAMPLING = {"4:2:0": 0, "4:4:4": 1}      # rd_jpeg_subsampling


def _sub(subsampling) -> int:
    if isinstance(subsampling, str):
        if subsampling not in SUBSAMPLING:
            raise ValueError(f"subsampling {subsampling!r} (4:2:0 or 4:4:4)")
        return SUBSAMPLING[subsampling]
    return int(subsampling)


def jpeg_header(width: int, height: int, quality: int = 90, subsampling="4:2:0", restart_mcus: int = 32) -> bytes:
    """The exact bytes before the entropy-coded data (SOI .. SOS) of such a file (rd_jpeg_header; no device needed)."""
    L = _lib.lib()
    n = C.c_size_t()
    args = (int(width), int(height), int(quality), _sub(subsampling), int(restart_mcus))
    check(L.rd_jpeg_header(*args, None, 0, C.byref(n)))
    buf = (C.c_uint8 * n.value)()
    check(L.rd_jpeg_header(*args, buf, n.value, C.byref(n)))
    return bytes(buf)


class JpegEncoder:
    """rd_jpeg: the encoder for frames of one size and format on one device, one stream per encoder."""

    def __init__(self, device: int, width: int, height: int, fmt: int = _lib.FMT_RGB_U8, quality: int = 90,
                 subsampling="4:2:0", restart_mcus: int = 32):
        self._h = C.c_void_p()
        self.device, self.width, self.height, self.fmt = int(device), int(width), int(height), int(fmt)
        self.quality, self.subsampling, self.restart_mcus = int(quality), _sub(subsampling), int(restart_mcus)
        check(_lib.lib().rd_jpeg_create(self.device, self.width, self.height, self.fmt, self.quality, self.subsampling,
                                        self.restart_mcus, C.byref(self._h)))
        mb, hb = C.c_size_t(), C.c_size_t()
        check(_lib.lib().rd_jpeg_info(self._h, C.byref(mb), C.byref(hb)))
        self.max_bytes, self.header_bytes = mb.value, hb.value

    @property
    def channels(self) -> int:
        return 4 if self.fmt == _lib.FMT_RGBA_U8 else 3

    def encode(self, src_ptrs: Sequence[int], dst_ptrs: Sequence[int], len_ptr: int, stream: int = 0, pitch: int = 0,
               dst_cap: int = 0) -> None:
        """Enqueue the encode of len(src_ptrs) device surfaces (rows `pitch` bytes apart, default width x channels) into
        dst_ptrs (dst_cap bytes each, default max_bytes); frame i's length lands at the device u64 len_ptr[i].  Not
        synchronised."""
        n = len(src_ptrs)
        if len(dst_ptrs) != n:
            raise ValueError(f"{len(dst_ptrs)} destinations for {n} frames")
        src = (C.c_void_p * max(n, 1))(*[int(p) for p in src_ptrs])
        dst = (C.c_void_p * max(n, 1))(*[int(p) for p in dst_ptrs])
        check(_lib.lib().rd_jpeg_encode(self._h, src, n, int(pitch or self.width * self.channels), dst,
                                        int(dst_cap or self.max_bytes), C.c_void_p(len_ptr) if len_ptr else None,
                                        C.c_void_p(stream) if stream else None))

    def encode_array(self, a) -> bytes:
        """One host frame ((height, width, channels) uint8) -> its JPEG file, through device buffers of its own."""
        import numpy as np
        a = np.ascontiguousarray(np.asarray(a, np.uint8))
        if a.shape != (self.height, self.width, self.channels):
            raise ValueError(f"frame of shape {a.shape}, the encoder takes {(self.height, self.width, self.channels)}")
        return encode_device(self, [_upload(self.device, a)], owned=True)[0]

    def close(self) -> None:
        if self._h:
            _lib.lib().rd_jpeg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def _malloc(device: int, nbytes: int) -> C.c_void_p:
    p = C.c_void_p()
    check(_lib.lib().rd_device_malloc(device, max(int(nbytes), 1), C.byref(p)))
    return p


def _upload(device: int, a) -> C.c_void_p:
    p = _malloc(device, a.nbytes)
    try:
        check(_lib.lib().rd_memcpy_h2d(device, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
    except Exception:
        _lib.lib().rd_device_free(device, p)
        raise
    return p


def encode_device(enc: JpegEncoder, src: Sequence[C.c_void_p], owned: bool = False, pitch: int = 0) -> List[bytes]:
    """Encode device surfaces, read every length back in one copy, then only `len` bytes per frame.  owned=True frees the
    sources afterwards."""
    import numpy as np
    L = _lib.lib()
    dev = enc.device
    bufs = []
    try:
        dst = [_malloc(dev, enc.max_bytes) for _ in src]
        bufs += dst
        lens_dev = _malloc(dev, 8 * len(src))
        bufs.append(lens_dev)
        enc.encode([p.value for p in src], [p.value for p in dst], lens_dev.value, pitch=pitch)
        check(L.rd_device_synchronize(dev))
        lens = np.zeros(len(src), np.uint64)
        check(L.rd_memcpy_d2h(dev, lens.ctypes.data_as(C.c_void_p), lens_dev, lens.nbytes))
        out = []
        for p, n in zip(dst, lens):
            b = (C.c_uint8 * int(n))()
            check(L.rd_memcpy_d2h(dev, b, p, int(n)))
            out.append(bytes(b))
        return out
    finally:
        for p in bufs:
            L.rd_device_free(dev, p)
        if owned:
            for p in src:
                L.rd_device_free(dev, p)


def develop_to_jpeg(frames, width: int, height: int, quality: int = 90, subsampling="4:2:0", restart_mcus: int = 32,
                    device: int = 0) -> List[bytes]:
    """Develop frames with the RGB8 batch path (rd_batch_develop) into device surfaces and encode them on the device.
    `frames` is an RdFrame array (BatchExporter.make_frames; out_dev is replaced by surfaces of this call's own).  Returns
    one JPEG file per frame."""
    from .batch import BatchExporter
    L = _lib.lib()
    n = len(frames)
    be = BatchExporter(device, width, height, _lib.FMT_RGB_U8, False)
    enc = JpegEncoder(device, width, height, _lib.FMT_RGB_U8, quality, subsampling, restart_mcus)
    surf = []
    try:
        surf = [_malloc(device, int(width) * int(height) * 3) for _ in range(n)]
        keep = [f.out_dev for f in frames]
        for f, p in zip(frames, surf):
            f.out_dev = p.value
        try:
            be.develop(frames)
        finally:
            for f, k in zip(frames, keep):
                f.out_dev = k
        return encode_device(enc, surf)
    finally:
        for p in surf:
            L.rd_device_free(device, p)
        enc.close()
        be.close()
