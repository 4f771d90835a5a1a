"""numpy oracle of the cache tiers: tier size, an independent weight computation and the two strict
f32 passes.  The passes are vectorised over the outputs and loop over the taps in ascending order -- one RN(w * v) and one
f32 add per tap, starting from +0 -- so they reproduce the kernels' sums bit for bit when given the same weights.

Its input is the frame's RGBA8 export codes: ref_c.pack_u8(ref_c.render_f32(...)).
"""
from __future__ import annotations

import math

import numpy as np

REFERENCE_TIERS = ((256, 2560), (384, 3840), (1280, 12800))


def round_half_away(x: float) -> int:
    f = math.floor(x)
    return int(f + (1 if x - f >= 0.5 else 0))


def tier_dims(W: int, H: int, bw: int, bh: int):
    ratio = min(bw / W, bh / H)
    return max(1, round_half_away(W * ratio)), max(1, round_half_away(H * ratio))


def _lanczos3(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    def sinc(t):
        a = np.pi * t
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(t == 0.0, 1.0, np.sin(a) / np.where(t == 0.0, 1.0, a))
    return np.where(np.abs(x) < 3.0, sinc(x) * sinc(x / 3.0), 0.0)


def weights(n_in: int, n_out: int):
    """(left, count, w) of one pass, computed here without the library: f32 steps, the kernel in double."""
    f = np.float32
    r = f(n_in) / f(n_out)
    sr = max(r, f(1.0))
    s = f(3.0) * sr
    left, count, ws = [], [], []
    for j in range(n_out):
        c = (f(j) + f(0.5)) * r
        lo = int(np.floor(c - s)); lo = min(max(lo, 0), n_in - 1)
        hi = int(np.ceil(c + s)); hi = min(max(hi, lo + 1), n_in)
        i = np.arange(lo, hi, dtype=np.float32)
        x = (i - (c - f(0.5))) / sr
        k = _lanczos3(x).astype(np.float32)
        tot = f(0.0)
        for v in k:
            tot = f(tot + v)
        left.append(lo); count.append(hi - lo); ws.append(k / tot)
    return np.array(left, np.uint32), np.array(count, np.uint32), np.concatenate(ws).astype(np.float32)


def _pass(src: np.ndarray, left, count, w, axis: int) -> np.ndarray:
    """src (.., n_in along `axis`, ..) f32 -> n_out along axis.  Taps ascending, per output, vectorised over outputs."""
    src = np.moveaxis(src.astype(np.float32, copy=False), axis, 0)
    n_out = len(left)
    left = np.asarray(left, np.int64); count = np.asarray(count, np.int64)
    off = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    out = np.zeros((n_out,) + src.shape[1:], np.float32)
    for k in range(int(count.max())):
        m = count > k
        js = np.nonzero(m)[0]
        wk = w[off[js] + k].astype(np.float32).reshape((-1,) + (1,) * (src.ndim - 1))
        prod = (wk * src[left[js] + k]).astype(np.float32)
        out[js] = (out[js] + prod).astype(np.float32)
    return np.moveaxis(out, 0, axis)


def to_bytes(v: np.ndarray) -> np.ndarray:
    """round_half_away(clamp(v, 0, 255)) -> uint8."""
    c = np.clip(v.astype(np.float32), np.float32(0), np.float32(255))
    fl = np.floor(c)
    return (fl + ((c - fl) >= np.float32(0.5))).astype(np.uint8)


def resample(codes: np.ndarray, tw: int, th: int, hx=None, vy=None, vertical_first: bool = False) -> np.ndarray:
    """codes (H, W, >=3) uint8 -> (th, tw, 3) uint8 tier; hx / vy: (left, count, w) tables (default: weights() here)."""
    H, W = codes.shape[:2]
    hx = hx if hx is not None else weights(W, tw)
    vy = vy if vy is not None else weights(H, th)
    src = codes[:, :, :3].astype(np.float32)
    if vertical_first:
        return to_bytes(_pass(_pass(src, *vy, axis=0), *hx, axis=1))
    return to_bytes(_pass(_pass(src, *hx, axis=1), *vy, axis=0))


def tier_surface(rgb: np.ndarray, fmt_rgba: bool) -> np.ndarray:
    if not fmt_rgba:
        return rgb
    a = np.full(rgb.shape[:2] + (1,), 255, np.uint8)
    return np.concatenate([rgb, a], axis=2)
