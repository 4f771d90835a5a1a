// rd_tiers.h -- gfx950 kernels of the cache tiers: a frame's RGBA8 export codes resampled by a separable Lanczos3 filter into
// up to four smaller (or larger) images -- the 256 / 384 / 1280 px tiers behind the Library grid and the Develop view
// (reference src/raw/processor.rs:13-15, :67-88, which runs image::imageops::resize(.., FilterType::Lanczos3) on the embedded
// JPEG; here the source is the developed frame itself).  The numerical contract is DESIGN.md section 11.
//
//   rd_tiers_hpass : develop + horizontal pass.  A workgroup owns whole row pairs (units, the export kernel's
//                    (2u-1, 2u) pairing over one CFA row pair, rd_kernels.h "rd_develop_quads"): it develops both rows into
//                    LDS as packed RGBA8 codes -- the CFA is read once, every pixel is developed once, no full-resolution
//                    surface goes to HBM -- and then computes every tier's horizontal taps for those rows from LDS into the
//                    context's f32 scratch T (RGB, 12 B per sample); a lane owns one output sample of one row.
//   rd_tiers_vpass : vertical pass over T.  One workgroup per (frame, tier, output row), one lane per output column; the row's
//                    taps (uniform over the workgroup: scalar loads) are walked in ascending order, the sum is rounded, clamped
//                    and packed, and the tier is stored.
// Both are strict f32 with no contraction (the library is built with -ffp-contract=off): every tap is RN(w * v) added to the
// running sum, which starts at +0.  The weight tables are built on the host (rd_host_tiers.inl) and are the ones
// rd_tier_weights hands out.
#pragma once

#include "rd_kernels.h"

#define RD_TIERS_MAX 4u            // tiers per context
#define RD_TIERS_LAUNCH_MAX 8u     // frames per launch (their descriptors travel as kernel arguments)
#define RD_TIERS_HBLOCK 512        // threads of the horizontal kernel: 8 waves
#define RD_TIERS_VBLOCK 256        // threads of the vertical kernel
#define RD_TIERS_LDS_MAX 163840u   // the CU's 160 KiB: one workgroup may take all of it

// One axis of one tier: output j takes input samples left[j] .. left[j] + count[j] - 1.  Vertical axis: its weights are
// w[off[j] ..] (the whole workgroup walks one output row's taps: scalar loads).  Horizontal axis (off unused): the table is
// TAP-MAJOR, tap i of output j at w[i * n_out + j], zero beyond count[j] -- the 64 lanes of a wave own 64 neighbouring
// outputs, so one tap's weights are one contiguous 256-byte load instead of 64 scattered ones.
struct rd_tier_axis {
    const uint32_t *left, *count, *off;
    const float *w;
};

struct rd_tiers_geom {
    uint32_t W, H, n_tiers, hitems;              // hitems = sum of the tiers' widths
    uint32_t tw[RD_TIERS_MAX], th[RD_TIERS_MAX];
    uint32_t hbase[RD_TIERS_MAX];                // first horizontal item of tier t (prefix sum of tw)
    uint32_t vbase[RD_TIERS_MAX + 1];            // first output row of tier t in the vertical grid (prefix sum of th)
    rd_tier_axis hx[RD_TIERS_MAX], vy[RD_TIERS_MAX];
    uint64_t t_off[RD_TIERS_MAX];                // float offset of tier t's T inside a frame's scratch slice
    uint64_t t_frame;                            // floats per frame slice
    float *scratch;                              // RD_TIERS_LAUNCH_MAX (or fewer) frame slices
};

struct rd_tiers_fdesc {
    const uint16_t *cfa;
    uint8_t *out[RD_TIERS_MAX];
    rd_ku u;
};

struct rd_tiers_launch {
    rd_tiers_fdesc f[RD_TIERS_LAUNCH_MAX];
};

__device__ __forceinline__ uint32_t rd_tiers_pack(uint32_t sr, uint32_t sg, uint32_t sb)      // rd_q8_lut_bits results -> 0xffbbggrr
{
    return ((sr >> 16) & 0xffu) | (((sg >> 16) & 0xffu) << 8) | (((sb >> 16) & 0xffu) << 16) | 0xff000000u;
}

__device__ __forceinline__ void rd_tiers_tap(float w, uint32_t p, float &r, float &g, float &b)
{
    r = r + w * (float)(p & 0xffu);
    g = g + w * (float)((p >> 8) & 0xffu);
    b = b + w * (float)((p >> 16) & 0xffu);
}

// Dynamic LDS: the 8-bit threshold table (RD_Q8_LUT_LDS_WORDS, a multiple of 4 words), then two rows of W packed codes.
__global__ void __launch_bounds__(RD_TIERS_HBLOCK)
rd_tiers_hpass(const rd_tiers_geom g, const rd_tiers_launch L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rd_tiers_lds[];
    uint32_t *lut = rd_tiers_lds;
    uint32_t *rows = rd_tiers_lds + RD_Q8_LUT_LDS_WORDS;
    rd_q8_lut_load(lut);                                         // (ends in a barrier)
    const uint32_t f = blockIdx.y;
    const uint16_t *cfa = L.f[f].cfa;
    const rd_ku &u = L.f[f].u;
    const uint32_t W = g.W, H = g.H;
    const uint32_t units = H / 2u + 1u, nq = (W + 1u) / 2u;
    float *T = g.scratch + (size_t)f * g.t_frame;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        // rows a = 2 unit - 1 and b = 2 unit (a = -1 and b = H do not exist); the CFA rows clamp to the frame, which is
        // get_neighbor's edge clamp (shaders.rs:163-166) for the first and last row
        const bool has_a = unit > 0u, has_b = 2u * unit < H;
        const uint32_t ra = has_a ? 2u * unit - 1u : 0u, rb = has_b ? 2u * unit : H - 1u;
        const uint16_t *pa = cfa + (size_t)ra * W, *pb = cfa + (size_t)rb * W;
        for (uint32_t q = threadIdx.x; q < nq; q += RD_TIERS_HBLOCK) {
            // an odd width's last column: its right-hand neighbour clamps onto itself, so the pair (x0, x0) gives the
            // selection rd_develop_px makes there
            const uint32_t x0 = 2u * q, x1 = x0 + 1u < W ? x0 + 1u : x0;
            const float A = rd_norm(pa[x0], u.black_level), B = rd_norm(pa[x1], u.black_level);
            const float Cv = rd_norm(pb[x0], u.black_level), D = rd_norm(pb[x1], u.black_level);
            // row a: (C, A, B) at both columns; row b: (C, D, A) at x0 and (C, D, B) at x0 + 1 (rd_develop_quads)
            float r[3] = { Cv, Cv, Cv }, gg[3] = { A, D, D }, b[3] = { B, A, B };
            rd_colour_n<3, RD_MATH_STRICT, false>(u, r, gg, b);
            const uint32_t p0 = rd_tiers_pack(rd_q8_lut_bits(r[0], lut), rd_q8_lut_bits(gg[0], lut), rd_q8_lut_bits(b[0], lut));
            const uint32_t p1 = rd_tiers_pack(rd_q8_lut_bits(r[1], lut), rd_q8_lut_bits(gg[1], lut), rd_q8_lut_bits(b[1], lut));
            const uint32_t p2 = rd_tiers_pack(rd_q8_lut_bits(r[2], lut), rd_q8_lut_bits(gg[2], lut), rd_q8_lut_bits(b[2], lut));
            rows[x0] = p0;
            rows[W + x0] = p1;
            if (x1 != x0) { rows[x1] = p0; rows[W + x1] = p2; }
        }
        __syncthreads();
        for (uint32_t it = threadIdx.x; it < 2u * g.hitems; it += RD_TIERS_HBLOCK) {
            const uint32_t sel = it >= g.hitems ? 1u : 0u;
            if (sel ? !has_b : !has_a) continue;
            const uint32_t k = it - sel * g.hitems;
            uint32_t t = 0;
#pragma unroll
            for (uint32_t j = 1; j < RD_TIERS_MAX; ++j) t += (j < g.n_tiers && k >= g.hbase[j]) ? 1u : 0u;
            const uint32_t x = k - g.hbase[t];
            const rd_tier_axis ax = g.hx[t];
            const uint32_t left = ax.left[x], cnt = ax.count[x];
            const float *wcol = ax.w + x;                           // tap-major table: tap i of every output is one row
            const uint32_t tw = g.tw[t];
            const uint32_t *src = rows + sel * W + left;
            float vr = 0.0f, vg = 0.0f, vb = 0.0f;
#pragma unroll 4
            for (uint32_t i = 0; i < cnt; ++i) rd_tiers_tap(wcol[(size_t)i * tw], src[i], vr, vg, vb);
            const uint32_t y = sel ? 2u * unit : 2u * unit - 1u;
            float *o = T + g.t_off[t] + ((size_t)y * g.tw[t] + x) * 3u;
            o[0] = vr; o[1] = vg; o[2] = vb;
        }
        __syncthreads();                                         // the rows are rewritten by the next unit
    }
}

// round_half_away(clamp(v, 0, 255)) as an integer: floor, then up when the exact fraction is at least one half.
__device__ __forceinline__ uint32_t rd_tiers_code(float v)
{
    const float c = fminf(fmaxf(v, 0.0f), 255.0f);
    const float fl = floorf(c);
    return (uint32_t)fl + (c - fl >= 0.5f ? 1u : 0u);
}

// grid (vbase[n_tiers], frames): blockIdx.x is an output row of one tier.  RGBA = true stores RGBA8 (alpha 255), else RGB8.
template <bool RGBA>
__global__ void __launch_bounds__(RD_TIERS_VBLOCK)
rd_tiers_vpass(const rd_tiers_geom g, const rd_tiers_launch L)
{
    const uint32_t f = blockIdx.y, row = blockIdx.x;
    uint32_t t = 0;
#pragma unroll
    for (uint32_t j = 1; j < RD_TIERS_MAX; ++j) t += (j < g.n_tiers && row >= g.vbase[j]) ? 1u : 0u;
    const uint32_t y = row - g.vbase[t], tw = g.tw[t];
    const rd_tier_axis ax = g.vy[t];
    const uint32_t top = ax.left[y], cnt = ax.count[y];
    const float *wv = ax.w + ax.off[y];
    const float *T = g.scratch + (size_t)f * g.t_frame + g.t_off[t] + (size_t)top * tw * 3u;
    uint8_t *out = L.f[f].out[t];
    for (uint32_t x = threadIdx.x; x < tw; x += RD_TIERS_VBLOCK) {
        const float *src = T + (size_t)x * 3u;
        float vr = 0.0f, vg = 0.0f, vb = 0.0f;
        for (uint32_t i = 0; i < cnt; ++i) {
            const float w = wv[i];
            const float *s = src + (size_t)i * tw * 3u;
            vr = vr + w * s[0];
            vg = vg + w * s[1];
            vb = vb + w * s[2];
        }
        const uint32_t qr = rd_tiers_code(vr), qg = rd_tiers_code(vg), qb = rd_tiers_code(vb);
        const size_t px = (size_t)y * tw + x;
        if constexpr (RGBA) {
            reinterpret_cast<uint32_t *>(out)[px] = qr | (qg << 8) | (qb << 16) | 0xff000000u;
        } else {
            uint8_t *o = out + px * 3u;
            o[0] = (uint8_t)qr; o[1] = (uint8_t)qg; o[2] = (uint8_t)qb;
        }
    }
}
