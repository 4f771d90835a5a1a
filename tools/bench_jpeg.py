"""The JPEG encoder on developed 24 MP frames: 32 frames of 6016 x 4016 with randomised slider stacks and the camera matrix
(mosaics with smooth structure, edges and sensor noise: tests/test_gpu_jpeg.py scene_cfa), developed into RGB8 surfaces by rd_batch_develop, then encoded at q90 4:2:0 with R = 32 by rd_jpeg_encode.  Prints ONE
JSON line:

  * encode_us_per_frame: the three encode kernels, HIP events (torch.cuda.Event on the null stream, which the library's
    launches also use) around one rd_jpeg_encode call of all frames, median of the repetitions;
  * pipeline_us_per_frame: develop + encode + read-back (one copy of all lengths, then `len` bytes per frame into host
    memory), host clock, median;
  * mb_per_frame: the mean compressed size;
  * pillow_*: Pillow (libjpeg-turbo) on the same frames, same settings, on 1 and 16 host threads;
  * pillow_identical: whether every GPU file equals Pillow's byte for byte (checked after the timed region).

    timeout -k 10 900 python tools/bench_jpeg.py [--frames 32] [--reps 5] [--no-pillow]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import raweditor_amd as ra
from raweditor_amd import _lib
from raweditor_amd._lib import check
from tests.gpu_util import DevBuf, sync
from tests.test_gpu_jpeg import scene_cfa

W, H = 6016, 4016
WB = (2.0, 1.0, 1.5, 1.0)
CM = (1.6, -0.4, -0.2, -0.3, 1.5, -0.2, 0.0, -0.5, 1.5)
NIN = 8
Q, SUB, R = 90, "4:2:0", 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pillow", action="store_true")
    a = ap.parse_args()
    import torch
    L = _lib.lib()
    rng = np.random.default_rng(0x4a504547)
    planes = [scene_cfa(rng, H, W) for _ in range(NIN)]                      # structure + sensor noise
    ins = [DevBuf.from_array(p) for p in planes]
    params = [ra.EditParams.random(np.random.default_rng([10, i])) for i in range(a.frames)]
    be = ra.BatchExporter(0, W, H, ra.FMT_RGB_U8, False)
    surf = [DevBuf(W * H * 3) for _ in range(a.frames)]
    fb = be.make_frames([ins[i % NIN].ptr for i in range(a.frames)], [s.ptr for s in surf], params, WB, CM)
    enc = ra.JpegEncoder(0, W, H, ra.FMT_RGB_U8, Q, SUB, R)
    dst = [DevBuf(enc.max_bytes) for _ in range(a.frames)]
    lens_dev = DevBuf(8 * a.frames)
    src_p, dst_p = [s.ptr for s in surf], [d.ptr for d in dst]
    be.develop(fb); enc.encode(src_p, dst_p, lens_dev.ptr); sync()                   # warm-up: code objects
    lens = np.zeros(a.frames, np.uint64)

    def read_back():
        check(L.rd_memcpy_d2h(0, lens.ctypes.data_as(C.c_void_p), C.c_void_p(lens_dev.ptr), lens.nbytes))
        out = []
        for d, n in zip(dst, lens):
            b = np.empty(int(n), np.uint8)
            check(L.rd_memcpy_d2h(0, b.ctypes.data_as(C.c_void_p), C.c_void_p(d.ptr), b.nbytes))
            out.append(b)
        return out

    t_enc, t_pipe = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enc.encode(src_p, dst_p, lens_dev.ptr)
        e1.record()
        torch.cuda.synchronize(); sync()
        t_enc.append(e0.elapsed_time(e1) * 1e3 / a.frames)
        t0 = time.perf_counter()
        be.develop(fb); enc.encode(src_p, dst_p, lens_dev.ptr)
        files = read_back()
        t_pipe.append((time.perf_counter() - t0) / a.frames * 1e6)
    med = lambda v: sorted(v)[len(v) // 2]                                         # noqa: E731
    mb = float(np.mean([f.size for f in files])) / 1e6
    rec = {"tool": "bench_jpeg", "frame": [W, H], "quality": Q, "subsampling": SUB, "restart_mcus": R, "frames_per_call": a.frames,
           "reps": a.reps, "encode_us_per_frame": round(med(t_enc), 2), "pipeline_us_per_frame": round(med(t_pipe), 2),
           "mb_per_frame": round(mb, 3), "max_bytes": enc.max_bytes, "target_encode_us": 500, "met": med(t_enc) <= 500,
           "encode_us_all": [round(v, 2) for v in t_enc], "pipeline_us_all": [round(v, 2) for v in t_pipe]}
    if not a.no_pillow:
        from PIL import Image
        imgs = [s.to_array(np.uint8, (H, W, 3)) for s in surf]

        def pil(img):
            b = io.BytesIO()
            Image.fromarray(img, "RGB").save(b, "JPEG", quality=Q, subsampling=2, restart_marker_blocks=R)
            return b.getvalue()
        t0 = time.perf_counter()
        ref = [pil(x) for x in imgs]
        t1 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(pil, imgs))
        t2 = time.perf_counter()
        rec["pillow_1t_us_per_frame"] = round((t1 - t0) / a.frames * 1e6, 1)
        rec["pillow_16t_us_per_frame"] = round((t2 - t1) / a.frames * 1e6, 1)
        rec["speedup_vs_pillow_1t"] = round(rec["pillow_1t_us_per_frame"] / rec["encode_us_per_frame"], 1)
        rec["pillow_identical"] = all(f.tobytes() == r for f, r in zip(files, ref))
    print(json.dumps(rec))
    enc.close(); be.close()
    return 0 if rec.get("pillow_identical", True) else 1


if __name__ == "__main__":
    sys.exit(main())
