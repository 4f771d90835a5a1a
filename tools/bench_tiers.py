"""Cache tiers against the RGBA8 batch develop: 24 MP frames (6016 x 4016) with randomised slider stacks and the camera matrix,
the three reference tiers (256 / 384 / 1280 px, processor.rs:13-15) through rd_tiers_develop, and the same frames through
rd_batch_develop(RD_FMT_RGBA_U8, no histogram), in one process, alternating.  Prints ONE JSON line: microseconds per frame of
each path (median of the repetitions; host clock around calls that end in a synchronise), their ratio against the 2.5x target,
and whether one timed frame's tiers match the oracle (checked after the timed region).

    timeout -k 10 600 python tools/bench_tiers.py [--frames 32] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import raweditor_amd as ra
from tests.gpu_util import DevBuf, sync

W, H = 6016, 4016
WB = (2.0, 1.0, 1.5, 1.0)
CM = (1.6, -0.4, -0.2, -0.3, 1.5, -0.2, 0.0, -0.5, 1.5)
NIN = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(0x54494552)
    planes = [rng.integers(0, 4096, (H, W), dtype=np.uint16) for _ in range(NIN)]
    ins = [DevBuf.from_array(p) for p in planes]
    params = [ra.EditParams.random(np.random.default_rng([9, i])) for i in range(a.frames)]
    be = ra.BatchExporter(0, W, H, ra.FMT_RGBA_U8, False)
    outs = [DevBuf(H * W * 4) for _ in range(4)]
    fb = be.make_frames([ins[i % NIN].ptr for i in range(a.frames)], [outs[i % 4].ptr for i in range(a.frames)], params, WB, CM)
    tr = ra.TierRenderer(0, W, H, ra.REFERENCE_TIERS, ra.FMT_RGBA_U8)
    tbuf = [[DevBuf(tr.tier_bytes(k)) for k in range(3)] for _ in range(a.frames)]
    tptr = [b.ptr for per in tbuf for b in per]
    be.develop(fb); tr.develop(fb, tptr); sync()                 # warm-up: code objects, tables
    t_batch, t_tiers = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); be.develop(fb); sync(); t_batch.append((time.perf_counter() - t0) / a.frames * 1e6)
        t0 = time.perf_counter(); tr.develop(fb, tptr); sync(); t_tiers.append((time.perf_counter() - t0) / a.frames * 1e6)
    med = lambda v: sorted(v)[len(v) // 2]                       # noqa: E731
    # after the timed region: the last frame's tiers against the oracle run on its RGBA8 export
    from oracle import ref_c
    from tests import tier_oracle as to
    k = a.frames - 1
    codes = ref_c.pack_u8(ref_c.render_f32(planes[k % NIN], ref_c.make_uniforms({f: getattr(params[k], f) for f in ra.FIELDS}, WB, CM)))
    ok = True
    for t, (tw, th) in enumerate(tr.dims):
        want = to.tier_surface(to.resample(codes, tw, th, ra.tier_weights(W, tw), ra.tier_weights(H, th)), True)
        ok = ok and np.array_equal(tbuf[k][t].to_array(np.uint8, (th, tw, 4)), want)
    ratio = med(t_tiers) / med(t_batch)
    print(json.dumps({"tool": "bench_tiers", "frame": [W, H], "tiers": tr.dims, "frames_per_call": a.frames, "reps": a.reps,
                      "rgba8_batch_us_per_frame": round(med(t_batch), 2), "tiers_us_per_frame": round(med(t_tiers), 2),
                      "ratio": round(ratio, 3), "target_ratio": 2.5, "met": ratio <= 2.5, "oracle_match": bool(ok),
                      "rgba8_batch_us_all": [round(v, 2) for v in t_batch], "tiers_us_all": [round(v, 2) for v in t_tiers]}))
    tr.close(); be.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
