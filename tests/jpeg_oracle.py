"""numpy oracle of the baseline JPEG encoder, written from the contract: libjpeg's default
compression path (JFIF, islow DCT, standard Huffman tables, restart interval R MCUs) byte for byte.

    header(w, h, q, sub, R)        -> the bytes before the entropy-coded data (SOI .. SOS)
    coefficients(img, q, sub)      -> (n_mcu, blocks_per_mcu, 64) int32 quantised coefficients in zigzag order, MCU order
    encode_interval(img, r, ...)   -> the stuffed, 1-padded bytes of restart interval r
    encode(img, q, sub, R)         -> the whole file
    split_scan(stream)             -> (header bytes, [interval bytes], trailer bytes)

`img` is an (h, w, 3|4) uint8 array (alpha ignored); `sub` is "4:2:0" or "4:4:4".  Everything is integer arithmetic on
int64 numpy arrays, vectorised over blocks; the Huffman stream is built symbol by symbol with numpy and packed MSB first.
"""
from __future__ import annotations

import numpy as np

# ---- tables (ITU-T T.81 Annex K) ------------------------------------------------------------------------
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], np.int64)
# ZIGZAG[k] = natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63], np.int64)

# (bits[1..16], values) of the four standard Huffman tables (K.3)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])


def huff_codes(spec):
    """(code[256], length[256]) of a table from its (bits, values) spec (Annex C); length 0 = no code."""
    bits, vals = spec
    code = np.zeros(256, np.int64)
    size = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], size[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, size


_DC = (huff_codes(DC_LUMA), huff_codes(DC_CHROMA))
_AC = (huff_codes(AC_LUMA), huff_codes(AC_CHROMA))


def quant_tables(q: int):
    """(luma, chroma) in natural order: Annex K scaled by the IJG quality rule, clamped to 1..255."""
    if not 1 <= q <= 100:
        raise ValueError(f"quality {q}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def mcu_geometry(w: int, h: int, sub: str):
    """(mcu_w, mcu_h in pixels, MCUs across, MCUs down, blocks per MCU)."""
    m = 16 if sub == "4:2:0" else 8
    return m, m, -(-w // m), -(-h // m), 6 if sub == "4:2:0" else 3


# ---- header ---------------------------------------------------------------------------------------------------
def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(w: int, h: int, q: int, sub: str = "4:2:0", R: int = 32) -> bytes:
    lq, cq = quant_tables(q)
    out = bytearray(b"\xff\xd8")
    out += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tid, t in ((0, lq), (1, cq)):
        out += _seg(0xDB, bytes([tid]) + bytes(int(v) for v in t[ZIGZAG]))
    hv = 0x22 if sub == "4:2:0" else 0x11
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, bytes([cls_id]) + bytes(spec[0]) + bytes(spec[1]))
    out += _seg(0xDD, R.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return bytes(out)


# ---- samples -------------------------------------------------------------------------------------------------
def ycc(img: np.ndarray):
    """IJG integer RGB -> YCbCr (16-bit fixed point), full resolution, int64 planes."""
    r, g, b = (img[:, :, i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """Replicate the last row / column out to rows x cols."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def component_planes(img: np.ndarray, sub: str):
    """The three component planes as the DCT sees them, each padded to whole blocks of its own (h_blocks*8, w_blocks*8):
    4:4:4 replicates the last row and column; 4:2:0 replicates the full-resolution columns out to the MCU width and the
    rows to an even count, downsamples with the alternating 1, 2 bias, then replicates the last chroma row."""
    h, w = img.shape[:2]
    y, cb, cr = ycc(img)
    if sub == "4:4:4":
        bh, bw = -(-h // 8) * 8, -(-w // 8) * 8
        return [_pad(p, bh, bw) for p in (y, cb, cr)]
    mw, mh = -(-w // 16) * 16, -(-h // 16) * 16
    Y = _pad(y, -(-h // 8) * 8, -(-w // 8) * 8)
    out = [Y]
    for c in (cb, cr):
        c = _pad(c, h + (h & 1), mw)
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)[None, :]
        d = (s + bias) >> 2
        out.append(_pad(d, mh // 2, mw // 2))
    return out


# ---- DCT + quantisation -----------------------------------------------------------------------------------------
CONST_BITS, PASS1_BITS = 13, 2
F = dict(F0298=2446, F0390=3196, F0541=4433, F0765=6270, F0899=7373, F1175=9633, F1501=12299, F1847=15137, F1961=16069,
         F2053=16819, F2562=20995, F3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_1d(d, first: bool):
    """One islow pass over axis -1 of d (..., 8)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        o[0], o[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F["F0541"]
    o[2] = _descale(z1 + t13 * F["F0765"], n)
    o[6] = _descale(z1 - t12 * F["F1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["F1175"]
    t4, t5, t6, t7 = t4 * F["F0298"], t5 * F["F2053"], t6 * F["F3072"], t7 * F["F1501"]
    z1, z2, z3, z4 = -z1 * F["F0899"], -z2 * F["F2562"], -z3 * F["F1961"] + z5, -z4 * F["F0390"] + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """(N, 8, 8) samples 0..255 -> (N, 8, 8) islow coefficients (scaled by 8)."""
    d = blocks.astype(np.int64) - 128
    d = _dct_1d(d, True)                                   # rows
    d = _dct_1d(d.transpose(0, 2, 1), False)               # columns
    return d.transpose(0, 2, 1)


def quantize(coef: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """(|x| + 4q) // 8q with the sign restored; coef (N, 64) natural order, qt (64,) natural order."""
    d = 8 * qt.astype(np.int64)
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


def _plane_blocks(p: np.ndarray) -> np.ndarray:
    """(bh*8, bw*8) -> (bh, bw, 64)."""
    bh, bw = p.shape[0] // 8, p.shape[1] // 8
    return p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(bh, bw, 64)


def coefficients(img: np.ndarray, q: int, sub: str = "4:2:0") -> np.ndarray:
    """(n_mcu, blocks_per_mcu, 64) quantised coefficients in zigzag order, MCUs in raster order.  4:2:0 MCUs hold Y00 Y01
    Y10 Y11 Cb Cr; a luma block outside the Y plane's ceil(w/8) x ceil(h/8) blocks is a dummy block: all AC 0, DC that of
    the block before it in the MCU (right of a real block: its left neighbour; the bottom row: the MCU's top-right
    block, itself possibly a dummy)."""
    h, w = img.shape[:2]
    lq, cq = quant_tables(q)
    _, _, mx, my, bpm = mcu_geometry(w, h, sub)
    planes = component_planes(img, sub)
    qz = []
    for ci, p in enumerate(planes):
        b = _plane_blocks(p)
        c = fdct_islow(b.reshape(-1, 8, 8).astype(np.int64)).reshape(-1, 64)
        qz.append(quantize(c, lq if ci == 0 else cq)[:, ZIGZAG].reshape(b.shape[0], b.shape[1], 64))
    out = np.zeros((my, mx, bpm, 64), np.int64)
    if sub == "4:4:4":
        for ci in range(3):
            out[:, :, ci] = qz[ci]
        return out.reshape(my * mx, bpm, 64)
    Y = qz[0]
    hb, wb = Y.shape[:2]
    Yp = np.zeros((my * 2, mx * 2, 64), np.int64)
    Yp[:hb, :wb] = Y
    if wb < mx * 2:                                        # right dummy column: DC of the left neighbour
        Yp[:hb, wb, 0] = Yp[:hb, wb - 1, 0]
    if hb < my * 2:                                        # bottom dummy row: DC of the MCU's top-right block
        Yp[hb, :, 0] = np.repeat(Yp[hb - 1, 1::2, 0], 2)
    for dy in range(2):
        for dx in range(2):
            out[:, :, dy * 2 + dx] = Yp[dy::2, dx::2]
    out[:, :, 4] = qz[1]
    out[:, :, 5] = qz[2]
    return out.reshape(my * mx, bpm, 64)


# ---- entropy coding ---------------------------------------------------------------------------------------------
def _nbits(v: np.ndarray) -> np.ndarray:
    a = np.abs(v)
    n = np.zeros(a.shape, np.int64)
    while (a >> n).any():
        n += (a >> n) > 0
    return n


def _pack(codes: np.ndarray, lens: np.ndarray) -> bytes:
    """Concatenate the codes (MSB first), pad with 1-bits to a byte, stuff 0xFF with 0x00."""
    if codes.size == 0:
        return b""
    sh = np.arange(31, -1, -1)[None, :]
    bits = ((codes[:, None] << (32 - lens[:, None])) >> sh) & 1
    mask = np.arange(32)[None, :] < lens[:, None]
    stream = bits[mask].astype(np.uint8)
    pad = (-stream.size) % 8
    stream = np.concatenate([stream, np.ones(pad, np.uint8)])
    by = np.packbits(stream)
    ff = by == 0xFF
    out = np.zeros(by.size + int(ff.sum()), np.uint8)
    pos = np.arange(by.size) + np.concatenate([[0], np.cumsum(ff)[:-1]])
    out[pos] = by
    return out.tobytes()


def encode_blocks(coef: np.ndarray, sub: str) -> bytes:
    """The stuffed, padded bytes of the MCUs in coef (n, bpm, 64) as ONE restart interval (DC predictors start at 0)."""
    n, bpm = coef.shape[:2]
    comp = np.array([0, 0, 0, 0, 1, 2] if sub == "4:2:0" else [0, 1, 2])
    tab = np.minimum(comp, 1)
    blocks = coef.reshape(n * bpm, 64)
    bcomp = np.tile(comp, n)
    btab = np.tile(tab, n)
    dc = blocks[:, 0]
    pred = np.zeros_like(dc)
    for c in range(3):
        idx = np.nonzero(bcomp == c)[0]
        pred[idx[1:]] = dc[idx[:-1]]
    diff = dc - pred
    # symbols: (block, order within block, code, length)
    sym_b, sym_o, sym_c, sym_l = [], [], [], []
    s = _nbits(diff)
    extra = np.where(diff < 0, diff - 1, diff) & ((1 << s) - 1)
    dcc = np.where(btab == 0, _DC[0][0][s], _DC[1][0][s])
    dcl = np.where(btab == 0, _DC[0][1][s], _DC[1][1][s])
    b_all = np.arange(n * bpm)
    sym_b.append(b_all); sym_o.append(np.zeros(n * bpm, np.int64))
    sym_c.append((dcc << s) | extra); sym_l.append(dcl + s)
    ac = blocks[:, 1:]
    bi, ki = np.nonzero(ac)
    ki = ki + 1
    prev = np.zeros_like(ki)
    if bi.size:
        same = np.concatenate([[False], bi[1:] == bi[:-1]])
        prev[same] = ki[np.nonzero(same)[0] - 1]
    run = ki - prev - 1
    v = ac[bi, ki - 1]
    nzrl = run // 16
    r = run % 16
    sz = _nbits(v)
    ex = np.where(v < 0, v - 1, v) & ((1 << sz) - 1)
    t = btab[bi]
    symv = (r << 4) | sz
    acc = np.where(t == 0, _AC[0][0][symv], _AC[1][0][symv])
    acl = np.where(t == 0, _AC[0][1][symv], _AC[1][1][symv])
    # ZRLs: each coefficient's preceding nzrl copies of 0xF0, ordered by 2 * k - 1 (before the coefficient at 2 * k)
    zb = np.repeat(bi, nzrl)
    zo = np.repeat(2 * ki - 1, nzrl)
    zt = np.repeat(t, nzrl)
    sym_b.append(zb); sym_o.append(zo)
    sym_c.append(np.where(zt == 0, _AC[0][0][0xF0], _AC[1][0][0xF0])); sym_l.append(np.where(zt == 0, _AC[0][1][0xF0], _AC[1][1][0xF0]))
    sym_b.append(bi); sym_o.append(2 * ki)
    sym_c.append((acc << sz) | ex); sym_l.append(acl + sz)
    # EOB where the last nonzero AC is before 63
    last = np.zeros(n * bpm, np.int64)
    if bi.size:
        last[bi] = ki                                      # bi ascending: the last write per block wins
    eb = np.nonzero(last < 63)[0]
    et = btab[eb]
    sym_b.append(eb); sym_o.append(np.full(eb.size, 200))
    sym_c.append(np.where(et == 0, _AC[0][0][0], _AC[1][0][0])); sym_l.append(np.where(et == 0, _AC[0][1][0], _AC[1][1][0]))
    B, O, Cc, Ll = (np.concatenate(x) for x in (sym_b, sym_o, sym_c, sym_l))
    order = np.lexsort((O, B))
    return _pack(Cc[order], Ll[order])


def n_intervals(w: int, h: int, sub: str, R: int) -> int:
    _, _, mx, my, _ = mcu_geometry(w, h, sub)
    return -(-(mx * my) // R)


def encode_interval(img: np.ndarray, r: int, q: int = 90, sub: str = "4:2:0", R: int = 32, coef=None) -> bytes:
    """The stuffed bytes of restart interval r (MCUs r*R .. r*R + R - 1), padded with 1-bits to a byte.  Without `coef`
    only the MCU rows the interval touches are transformed (a crop at MCU-row boundaries has the same blocks)."""
    if coef is not None:
        return encode_blocks(coef[r * R:(r + 1) * R], sub)
    h, w = img.shape[:2]
    _, mh, mx, my, _ = mcu_geometry(w, h, sub)
    m0, m1 = r * R, min((r + 1) * R, mx * my)
    y0, y1 = m0 // mx, (m1 - 1) // mx + 1
    crop = img[y0 * mh:min(h, y1 * mh)]
    c = coefficients(crop, q, sub)
    return encode_blocks(c[m0 - y0 * mx:m1 - y0 * mx], sub)


def encode(img: np.ndarray, q: int = 90, sub: str = "4:2:0", R: int = 32) -> bytes:
    h, w = img.shape[:2]
    coef = coefficients(img, q, sub)
    out = bytearray(header(w, h, q, sub, R))
    n = n_intervals(w, h, sub, R)
    for r in range(n):
        out += encode_blocks(coef[r * R:(r + 1) * R], sub)
        if r + 1 < n:
            out += bytes([0xFF, 0xD0 + r % 8])
    out += b"\xff\xd9"
    return bytes(out)


def split_scan(stream: bytes):
    """(header through SOS, [interval bytes], trailer = EOI); checks the RSTn cycle on the way."""
    i = 2
    while True:
        assert stream[i] == 0xFF, i
        m = stream[i + 1]
        ln = int.from_bytes(stream[i + 2:i + 4], "big")
        i += 2 + ln
        if m == 0xDA:
            break
    hdr = stream[:i]
    body = np.frombuffer(stream, np.uint8)
    assert stream[-2:] == b"\xff\xd9"
    ffs = np.nonzero(body[i:-2] == 0xFF)[0] + i
    marks = [int(p) for p in ffs if 0xD0 <= body[p + 1] <= 0xD7]
    for k, p in enumerate(marks):
        assert body[p + 1] == 0xD0 + k % 8, (k, p)
    bounds = [i] + [p for m in marks for p in (m, m + 2)] + [len(stream) - 2]
    parts = [stream[bounds[2 * k]:bounds[2 * k + 1]] for k in range(len(bounds) // 2)]
    return hdr, parts, stream[-2:]
