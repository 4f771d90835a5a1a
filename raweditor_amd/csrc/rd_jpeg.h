// rd_jpeg.h -- gfx950 kernels of the baseline JPEG encoder: RGB8 / RGBA8 surfaces -> baseline sequential JFIF files, libjpeg's
// default compression path byte for byte (IJG integer colour conversion, islow DCT, Annex K tables scaled by the IJG quality
// rule, standard Huffman tables, restart interval R MCUs).  The numerical contract is DESIGN.md section 12.
//
//   rd_jpeg_dct    : one thread per 8x8 block.  Threads are laid out component-major (4:2:0: the luma blocks in plane raster
//                    order, then Cb, then Cr), so a wave takes one code path; each thread gathers its block's samples with
//                    libjpeg's edge replication, converts colour (and downsamples), runs the two islow passes in registers,
//                    quantises with a reciprocal multiply and stores 64 int16 coefficients in zigzag order (128 B) in MCU
//                    order to the context's coefficient scratch.  A luma dummy block (outside the plane's blocks, inside
//                    the MCU) runs the same code on the block whose DC it copies and stores AC 0.
//   rd_jpeg_huff   : one wave (= one workgroup) per restart interval, lanes own blocks, 64 blocks per round.  A lane walks
//                    its block once for its exact bit length; a wave scan gives the offsets; a second walk ORs the codes
//                    into an LDS bit window (a code that straddles a word takes two ORs); the wave then writes the window's
//                    complete bytes with 0xFF stuffing (a ballot counts the 0xFF bytes before each lane) to the interval's
//                    scratch slot and carries the partial byte into the next round.  The interval ends padded with 1-bits;
//                    its stuffed byte length goes to an array.
//   rd_jpeg_concat : per frame, workgroups own groups of intervals: each sums the lengths before its group, copies the
//                    header (group 0), its intervals with their RSTn markers, and EOI + the frame's length (last group).
// No global atomics: every output byte has one owner.  The host (rd_host_jpeg.inl) builds the tables and the header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define RD_JPEG_LAUNCH_MAX 8u      // frames per launch (their pointers travel as kernel arguments)
#define RD_JPEG_DCT_BLOCK 256      // threads of the DCT kernel
#define RD_JPEG_CONCAT_BLOCK 256   // threads of the concat kernel
// The longest code + extra bits of one block, from the standard tables (rd_host_jpeg.inl checks it): DC <= 11 + 11 bits,
// every AC symbol <= 16 + 10 bits, 63 of them.
#define RD_JPEG_BLOCK_MAX_BITS (22u + 63u * 26u)
#define RD_JPEG_WIN_WORDS (((64u * RD_JPEG_BLOCK_MAX_BITS + 8u) + 31u) / 32u + 1u)

// Device tables, built on the host: the quantiser (natural order) and the Huffman codes (code | length << 16).
struct rd_jpeg_tables {
    uint32_t qmul[2][64];          // ceil(2^32 / (8 q)): (|x| + 4 q) / (8 q) == umulhi(|x| + 4 q, qmul) for |x| < 2^15
    uint32_t qhalf[2][64];         // 4 q
    uint32_t dc[2][16];            // [table][size category]
    uint32_t ac[2][256];           // [table][run << 4 | size]
};

struct rd_jpeg_geom {
    uint32_t W, H, bpp;            // bytes per source pixel: 3 or 4
    uint32_t mcux, mcuy, n_mcu, bpm;   // MCUs across / down / total; blocks per MCU (6 for 4:2:0, 3 for 4:4:4)
    uint32_t sub420, R, n_int;     // restart interval (MCUs) and intervals per frame
    uint32_t hdr_len, groups, group_n; // concat: groups of group_n intervals per frame
    uint64_t slot_bytes;           // one interval's scratch slot (its worst case, stuffed)
    uint64_t coef_frame;           // int16 per frame in the coefficient scratch
    const rd_jpeg_tables *tab;
    const uint8_t *hdr;
    int16_t *coef;
    uint8_t *bits;
    uint32_t *lens;
};

struct rd_jpeg_launch {
    const uint8_t *src[RD_JPEG_LAUNCH_MAX];
    uint8_t *dst[RD_JPEG_LAUNCH_MAX];
    uint64_t *len;                 // this launch's first frame's length
    uint64_t pitch;
};

__constant__ static const uint8_t rd_jpeg_zigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63};

// ---- colour ------------------------------------------------------------------------------------------------------
// IJG rgb_ycc_convert, 16-bit fixed point (FIX(0.29900) = 19595 ...); comp 0 = Y, 1 = Cb, 2 = Cr.
__device__ __forceinline__ int rd_jpeg_ycc(const uint8_t *p, uint32_t comp)
{
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// ---- islow DCT ---------------------------------------------------------------------------------------------------
#define RD_JPEG_CB 13
#define RD_JPEG_P1 2
__device__ __forceinline__ int rd_jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One islow pass over d[o], d[o + s], ..., d[o + 7 s] (jfdctint.c); FIRST = the row pass.
template <bool FIRST>
__device__ __forceinline__ void rd_jpeg_dct8(int *d, int o, int s)
{
    const int t0 = d[o] + d[o + 7 * s], t7 = d[o] - d[o + 7 * s];
    const int t1 = d[o + s] + d[o + 6 * s], t6 = d[o + s] - d[o + 6 * s];
    const int t2 = d[o + 2 * s] + d[o + 5 * s], t5 = d[o + 2 * s] - d[o + 5 * s];
    const int t3 = d[o + 3 * s] + d[o + 4 * s], t4 = d[o + 3 * s] - d[o + 4 * s];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? RD_JPEG_CB - RD_JPEG_P1 : RD_JPEG_CB + RD_JPEG_P1;
    if (FIRST) {
        d[o] = (t10 + t11) << RD_JPEG_P1;
        d[o + 4 * s] = (t10 - t11) << RD_JPEG_P1;
    } else {
        d[o] = rd_jpeg_descale(t10 + t11, RD_JPEG_P1);
        d[o + 4 * s] = rd_jpeg_descale(t10 - t11, RD_JPEG_P1);
    }
    int z1 = (t12 + t13) * 4433;
    d[o + 2 * s] = rd_jpeg_descale(z1 + t13 * 6270, n);
    d[o + 6 * s] = rd_jpeg_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 = -z1 * 7373; z2 = -z2 * 20995; z3 = -z3 * 16069 + z5; z4 = -z4 * 3196 + z5;
    d[o + 7 * s] = rd_jpeg_descale(a4 + z1 + z3, n);
    d[o + 5 * s] = rd_jpeg_descale(a5 + z2 + z4, n);
    d[o + 3 * s] = rd_jpeg_descale(a6 + z2 + z3, n);
    d[o + s] = rd_jpeg_descale(a7 + z1 + z4, n);
}

// grid (ceil(n_mcu * bpm / RD_JPEG_DCT_BLOCK), frames)
__global__ void __launch_bounds__(RD_JPEG_DCT_BLOCK)
rd_jpeg_dct(const rd_jpeg_geom g, const rd_jpeg_launch L)
{
    __shared__ uint32_t rd_jpeg_dct_lds[RD_JPEG_DCT_BLOCK * 33];
    const uint32_t t = blockIdx.x * RD_JPEG_DCT_BLOCK + threadIdx.x;
    if (t >= g.n_mcu * g.bpm) return;
    const uint32_t f = blockIdx.y;
    const uint8_t *src = L.src[f];
    const uint64_t pitch = L.pitch;
    const uint32_t W = g.W, H = g.H, bpp = g.bpp;
    uint32_t comp, mcu, slot, sx, sy;              // sx, sy: the block (in its component plane) whose samples are used
    bool dummy = false;
    if (g.sub420) {
        const uint32_t nY = 4u * g.n_mcu;
        if (t < nY) {
            const uint32_t pw = 2u * g.mcux;
            const uint32_t by = t / pw, bx = t - by * pw;
            comp = 0; mcu = (by >> 1) * g.mcux + (bx >> 1); slot = (by & 1u) * 2u + (bx & 1u);
            const uint32_t wb = (W + 7u) >> 3, hb = (H + 7u) >> 3;
            sx = bx; sy = by;
            if (by >= hb) {                        // bottom dummy row: DC of the MCU's top-right block (itself maybe a dummy)
                dummy = true;
                sy = by - 1u;
                sx = (bx | 1u) < wb ? (bx | 1u) : (bx & ~1u);
            } else if (bx >= wb) {                 // right dummy: DC of the left neighbour
                dummy = true;
                sx = bx - 1u;
            }
        } else {
            comp = t < nY + g.n_mcu ? 1u : 2u;
            mcu = t - nY - (comp - 1u) * g.n_mcu;
            slot = 3u + comp;
            sy = mcu / g.mcux; sx = mcu - sy * g.mcux;
        }
    } else {
        comp = t / g.n_mcu;
        mcu = t - comp * g.n_mcu;
        slot = comp;
        sy = mcu / g.mcux; sx = mcu - sy * g.mcux;
    }
    // the block's centred samples go through this thread's row of LDS (64 int16 in 32 words, stride 33 words: no bank
    // conflicts), one sample row at a time -- gathering straight into registers lets the compiler hoist every load
    uint32_t *blk = rd_jpeg_dct_lds + threadIdx.x * 33u;
    const bool c420 = g.sub420 && comp;
    const uint32_t hc = (H + 1u) >> 1;
#pragma unroll 1
    for (uint32_t r = 0; r < 8u; ++r) {
        int e[8];
        if (c420) {
            // 4:2:0 chroma: columns replicate out to the MCU width, rows to an even count, the downsampled rows past the
            // last replicate that last row; bias 1, 2, 1, 2 ... along the output row
            const uint32_t cy = min(sy * 8u + r, hc - 1u);
            const uint8_t *r0 = src + (uint64_t)min(2u * cy, H - 1u) * pitch;
            const uint8_t *r1 = src + (uint64_t)min(2u * cy + 1u, H - 1u) * pitch;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t x0 = min(sx * 16u + 2u * c, W - 1u), x1 = min(sx * 16u + 2u * c + 1u, W - 1u);
                const int sum = rd_jpeg_ycc(r0 + x0 * bpp, comp) + rd_jpeg_ycc(r0 + x1 * bpp, comp) +
                                rd_jpeg_ycc(r1 + x0 * bpp, comp) + rd_jpeg_ycc(r1 + x1 * bpp, comp);
                e[c] = ((sum + 1 + (c & 1)) >> 2) - 128;
            }
        } else {
            const uint8_t *row = src + (uint64_t)min(sy * 8u + r, H - 1u) * pitch;
#pragma unroll
            for (int c = 0; c < 8; ++c) e[c] = rd_jpeg_ycc(row + min(sx * 8u + c, W - 1u) * bpp, comp) - 128;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) blk[r * 4u + c] = (uint32_t)(uint16_t)(int16_t)e[2 * c] | ((uint32_t)(uint16_t)(int16_t)e[2 * c + 1] << 16);
    }
    int d[64];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const uint32_t w = blk[i];
        d[2 * i] = (int)(int16_t)(uint16_t)(w & 0xffffu);
        d[2 * i + 1] = (int)(int16_t)(uint16_t)(w >> 16);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) rd_jpeg_dct8<true>(d, r * 8, 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) rd_jpeg_dct8<false>(d, c, 8);
    const uint32_t tq = comp ? 1u : 0u;
    const uint32_t *qm = g.tab->qmul[tq], *qh = g.tab->qhalf[tq];
    uint32_t packed[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int zi = rd_jpeg_zigzag[k];
        const int x = d[zi];
        const uint32_t a = (uint32_t)(x < 0 ? -x : x);
        int v = (int)__umulhi(a + qh[zi], qm[zi]);
        v = x < 0 ? -v : v;
        if (dummy && k) v = 0;
        const uint32_t h = (uint32_t)(uint16_t)(int16_t)v;
        if (k & 1) packed[k >> 1] |= h << 16;
        else packed[k >> 1] = h;
    }
    uint4 *out = reinterpret_cast<uint4 *>(g.coef + (uint64_t)f * g.coef_frame + ((uint64_t)mcu * g.bpm + slot) * 64u);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = make_uint4(packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]);
}

// ---- Huffman -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rd_jpeg_nbits(int v)
{
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32u - __clz(a) : 0u;
}

__device__ __forceinline__ int rd_jpeg_coef(const uint4 *c, int k)      // zigzag coefficient k of a block held as 8 x uint4
{
    const uint4 q = c[k >> 3];
    const int w = (k >> 1) & 3;
    const uint32_t u = w == 0 ? q.x : w == 1 ? q.y : w == 2 ? q.z : q.w;
    return (int)(int16_t)(uint16_t)((k & 1) ? (u >> 16) : (u & 0xffffu));
}

// Walks one block's symbols: emit(value, nbits) for each code (+ extra bits) in stream order.
template <class Emit>
__device__ __forceinline__ void rd_jpeg_block(const uint4 *c, int pred, const uint32_t *dc, const uint32_t *ac, Emit &&emit)
{
    const int diff = rd_jpeg_coef(c, 0) - pred;
    const uint32_t s = rd_jpeg_nbits(diff);
    const uint32_t dcode = dc[s];
    emit(((dcode & 0xffffu) << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u)), (dcode >> 16) + s);
    uint32_t run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = rd_jpeg_coef(c, k);
        if (v == 0) {
            ++run;
        } else {
            while (run > 15u) {
                emit(ac[0xf0] & 0xffffu, ac[0xf0] >> 16);
                run -= 16u;
            }
            const uint32_t sz = rd_jpeg_nbits(v);
            const uint32_t code = ac[(run << 4) | sz];
            emit(((code & 0xffffu) << sz) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u)), (code >> 16) + sz);
            run = 0;
        }
    }
    if (run) emit(ac[0] & 0xffffu, ac[0] >> 16);
}

__device__ __forceinline__ uint32_t rd_jpeg_win_byte(const uint32_t *win, uint32_t b)
{
    return (win[b >> 2] >> (24u - 8u * (b & 3u))) & 0xffu;
}

// grid (n_int, frames), one wave per workgroup
__global__ void __launch_bounds__(64)
rd_jpeg_huff(const rd_jpeg_geom g, const rd_jpeg_launch)
{
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    __shared__ uint32_t win[RD_JPEG_WIN_WORDS];
    const uint32_t lane = threadIdx.x, f = blockIdx.y, r = blockIdx.x;
    for (uint32_t i = lane; i < 32u; i += 64u) s_dc[i >> 4][i & 15u] = g.tab->dc[i >> 4][i & 15u];
    for (uint32_t i = lane; i < 512u; i += 64u) s_ac[i >> 8][i & 255u] = g.tab->ac[i >> 8][i & 255u];
    const uint32_t m0 = r * g.R, m1 = min(m0 + g.R, g.n_mcu);
    const uint32_t b0 = m0 * g.bpm, b1 = m1 * g.bpm;
    const int16_t *coef = g.coef + (uint64_t)f * g.coef_frame;
    uint8_t *out = g.bits + ((uint64_t)f * g.n_int + r) * g.slot_bytes;
    const uint64_t cap = g.slot_bytes;
    uint64_t pos = 0;                              // stuffed bytes written
    uint32_t carry = 0, cbits = 0;                 // the partial byte (high bits) and its bit count, < 8
    const uint64_t lt = lane ? (~0ull >> (64u - lane)) : 0ull;
    __syncthreads();
    for (uint32_t base = b0; base < b1; base += 64u) {
        const uint32_t blk = base + lane;
        const bool valid = blk < b1;
        uint4 c[8];
        int pred = 0;
        uint32_t tsel = 0;
        if (valid) {
            const uint4 *p = reinterpret_cast<const uint4 *>(coef + (uint64_t)blk * 64u);
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = p[i];
            // the previous block of the same component, inside this interval
            const uint32_t slot = blk % g.bpm;
            uint32_t prev;
            if (g.sub420) { prev = slot == 0u ? blk - 3u : slot < 4u ? blk - 1u : blk - 6u; tsel = slot < 4u ? 0u : 1u; }
            else { prev = blk - 3u; tsel = slot ? 1u : 0u; }
            // (blk - 3 or blk - 6 below b0 -- or wrapped below 0 -- is the interval's first block of its component: predictor 0)
            if (prev >= b0 && prev < blk) pred = (int)coef[(uint64_t)prev * 64u];
        }
        // pass 1: exact bit length
        uint32_t nb = 0;
        if (valid) rd_jpeg_block(c, pred, s_dc[tsel], s_ac[tsel], [&](uint32_t, uint32_t n) { nb += n; });
        // wave inclusive scan
        uint32_t inc = nb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o, 64);
            if (lane >= (uint32_t)o) inc += v;
        }
        const uint32_t total = __shfl(inc, 63, 64);
        const uint32_t end = cbits + total;        // bits in the window
        const uint32_t nw = (end + 31u) >> 5;
        for (uint32_t i = lane; i < nw; i += 64u) win[i] = 0u;
        __syncthreads();
        if (lane == 0) win[0] |= carry << 24;
        __syncthreads();
        // pass 2: OR the codes into the window
        if (valid) {
            uint32_t p = cbits + inc - nb;
            rd_jpeg_block(c, pred, s_dc[tsel], s_ac[tsel], [&](uint32_t v, uint32_t n) {
                const uint32_t w = p >> 5, o = p & 31u;
                const uint64_t x = (uint64_t)v << (64u - o - n);
                atomicOr(&win[w], (uint32_t)(x >> 32));
                if (o + n > 32u) atomicOr(&win[w + 1u], (uint32_t)x);
                p += n;
            });
        }
        __syncthreads();
        // the window's complete bytes, stuffed
        const uint32_t full = end >> 3;
        for (uint32_t i0 = 0; i0 < full; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const bool in = i < full;
            const uint32_t b = in ? rd_jpeg_win_byte(win, i) : 0u;
            const uint64_t ff = __ballot(in && b == 0xffu);
            const uint64_t at = pos + lane + (uint64_t)__popcll(ff & lt);
            if (in && at < cap) out[at] = (uint8_t)b;
            if (in && b == 0xffu && at + 1u < cap) out[at + 1u] = 0u;
            pos += min(64u, full - i0) + (uint64_t)__popcll(ff);
        }
        cbits = end & 7u;
        carry = cbits ? rd_jpeg_win_byte(win, full) : 0u;
        __syncthreads();                           // the window is cleared by the next round
    }
    if (lane == 0) {
        if (cbits) {                               // pad the last byte with 1-bits
            const uint32_t b = carry | (0xffu >> cbits);
            if (pos < cap) out[pos] = (uint8_t)b;
            ++pos;
            if (b == 0xffu) { if (pos < cap) out[pos] = 0u; ++pos; }
        }
        g.lens[(uint64_t)f * g.n_int + r] = (uint32_t)pos;
    }
}

// ---- concatenation --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rd_jpeg_block_sum(uint64_t v, uint64_t *red)
{
    // workgroup sum of RD_JPEG_CONCAT_BLOCK values (red: RD_JPEG_CONCAT_BLOCK / 64 entries)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < RD_JPEG_CONCAT_BLOCK / 64; ++i) s += red[i];
    __syncthreads();
    return s;
}

// grid (groups, frames): group k copies intervals [k * group_n, min((k + 1) * group_n, n_int))
__global__ void __launch_bounds__(RD_JPEG_CONCAT_BLOCK)
rd_jpeg_concat(const rd_jpeg_geom g, const rd_jpeg_launch L)
{
    __shared__ uint64_t red[RD_JPEG_CONCAT_BLOCK / 64];
    const uint32_t f = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const uint32_t *lens = g.lens + (uint64_t)f * g.n_int;
    const uint32_t j0 = k * g.group_n, j1 = min(j0 + g.group_n, g.n_int);
    uint64_t part = 0;
    for (uint32_t j = tid; j < j0; j += RD_JPEG_CONCAT_BLOCK) part += lens[j];
    const uint64_t before = rd_jpeg_block_sum(part, red);
    uint8_t *dst = L.dst[f];
    if (k == 0)
        for (uint32_t i = tid; i < g.hdr_len; i += RD_JPEG_CONCAT_BLOCK) dst[i] = g.hdr[i];
    const uint8_t *bits = g.bits + (uint64_t)f * g.n_int * g.slot_bytes;
    uint64_t o = g.hdr_len + before + 2ull * j0;   // every thread walks the group's offsets (uniform loads)
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t n = lens[j];
        const uint8_t *s = bits + (uint64_t)j * g.slot_bytes;
        uint8_t *d = dst + o;
        for (uint32_t i = tid; i < n; i += RD_JPEG_CONCAT_BLOCK) d[i] = s[i];
        if (tid == 0) {
            // RSTn between intervals; EOI after the last
            d[n] = 0xffu;
            d[n + 1u] = j + 1u < g.n_int ? (uint8_t)(0xd0u + (j & 7u)) : 0xd9u;
        }
        o += n + 2ull;
    }
    if (j1 == g.n_int && tid == 0) L.len[f] = o;
}
