#!/usr/bin/env python3
"""Re-evaluate the reference's shader text against the committed fixtures made from it (tests/golden/wgsl_golden.npz,
tests/golden/wgsl_fullsize.json): the text's SHA-256, four small cases through the scalar evaluator (both rasterisations),
every small case through the vector evaluator, and one band of the full-size frames.  The suite pins the oracles and the HIP
path to the fixtures; this checks the fixtures against the text, so it needs the reference's source tree, which the
repository does not carry:

    python tools/check_wgsl_fixtures.py <reference checkout>/src/gpu/shaders.rs
"""
import hashlib
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import wgsl_eval as we, wgsl_render as wr  # noqa: E402
from tests.test_wgsl_pin_cpu import CASES, FULL, META, bits, fullsize_inputs  # noqa: E402


def check_scalar_evaluator(src):
    by = {c["name"]: c for c in CASES}
    for name in ("random_odd_7x9", "preview_zoom_pan", "tex_coord_one", "range_ends_2"):
        c = by[name]
        block = wr.uniform_block(c["params"], c["wb"], c["cm"], c["zoom"], *c["pan"])
        r = wr.render(src, c["cfa"], block, c["tw"], c["th"], lowering=we.Lowering(pow=we.pow_f64_rounded))
        assert np.array_equal(bits(r["rgba"]), bits(c["f32_libm"])), name
        assert np.array_equal(bits(r["tex"]), bits(c["tex"])), name
        b = wr.render(src, c["cfa"], block, c["tw"], c["th"], lowering=we.Lowering(pow=we.pow_f64_rounded),
                      raster="barycentric_f64")
        assert np.array_equal(bits(b["rgba"]), bits(c["f32_libm"])), name


def check_vector_evaluator(src):
    for c in CASES:
        block = wr.uniform_block(c["params"], c["wb"], c["cm"], c["zoom"], *c["pan"])
        rgba, mod = wr.render_rows(src, c["cfa"], block, we.Lowering(pow=wr.pow_pinned_lanes), 0, c["th"], c["tw"], c["th"])
        assert np.array_equal(bits(rgba), bits(c["f32_pinned"])), c["name"]
        assert (mod.texture.oob_loads, mod.nan_to_int) == (c["oob_loads"], c["nan_to_int"]), c["name"]


def check_fullsize_bands(src):
    rows = FULL["band_rows"]
    for n, fr in enumerate(FULL["frames"]):
        if fr["w"] * fr["h"] > 30_000_000 and n % 2:
            continue
        cfa = fullsize_inputs(fr)
        k = (7 * n + 3) % len(fr["crc32_f32_bands"])
        block = wr.uniform_block(fr["params"], FULL["wb"], fr["cm"])
        rgba, _ = wr.render_rows(src, cfa, block, we.Lowering(pow=wr.pow_pinned_lanes), k * rows, min((k + 1) * rows, fr["h"]))
        assert zlib.crc32(np.ascontiguousarray(rgba).tobytes()) == fr["crc32_f32_bands"][k], (fr["name"], k)


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    with open(argv[1], encoding="utf-8") as f:
        src = we.extract_rust_raw_string(f.read(), META["shader_const"])
    assert hashlib.sha256(src.encode()).hexdigest() == FULL["shader_sha256"] == META["shader_sha256"], "the shader text changed"
    for check in (check_scalar_evaluator, check_vector_evaluator, check_fullsize_bands):
        check(src)
        print(f"{check.__name__}: ok", flush=True)


if __name__ == "__main__":
    main(sys.argv)
