// rd_host_tiers.inl -- host side of the cache tiers (rd_tier_dims, rd_tier_weights, rd_tiers_*; kernels in rd_tiers.h).
// Included once from rawdev.hip.  The numerical contract (tier size, weights, pass order, rounding) is DESIGN.md section 11.

// image::imageops::resize's fit rule: the largest size with the frame's aspect inside the box, ratio in f64, each side
// rounded half away from zero and at least 1.
static int rd_tier_fit(uint32_t W, uint32_t H, uint32_t bw, uint32_t bh, uint32_t *w, uint32_t *h)
{
    const double ratio = std::min((double)bw / (double)W, (double)bh / (double)H);
    const double fw = std::round((double)W * ratio), fh = std::round((double)H * ratio);
    if (!(fw <= 4294967295.0) || !(fh <= 4294967295.0)) return rd_fail(RD_ERR_INVALID_ARG, "tier of %ux%u in a %ux%u box does not fit 32 bits", W, H, bw, bh);
    *w = fw < 1.0 ? 1u : (uint32_t)fw;
    *h = fh < 1.0 ? 1u : (uint32_t)fh;
    return RD_OK;
}

static double rd_sinc(double t)
{
    if (t == 0.0) return 1.0;
    const double a = M_PI * t;
    return sin(a) / a;
}

static double rd_lanczos3(double x) { return fabs(x) < 3.0 ? rd_sinc(x) * rd_sinc(x / 3.0) : 0.0; }

// The weights of one pass n_in -> n_out, every step in f32 except the kernel itself (double, then rounded to f32):
// output j covers [left, left + count) and its weights sum to 1 within rounding.  `padded` = true lays each output's weights
// out from a multiple of 4 with zeros up to the next multiple of 4 (the kernels' float4 loads; `off` receives the offsets);
// false packs them back to back (rd_tier_weights).
static void rd_tier_axis_build(uint32_t n_in, uint32_t n_out, bool padded, std::vector<uint32_t> &left,
                               std::vector<uint32_t> &count, std::vector<uint32_t> &off, std::vector<float> &w)
{
    left.assign(n_out, 0u); count.assign(n_out, 0u); off.assign(n_out, 0u);
    w.clear();
    const float r = (float)n_in / (float)n_out;
    const float sr = r > 1.0f ? r : 1.0f;
    const float s = 3.0f * sr;
    std::vector<float> k;
    for (uint32_t j = 0; j < n_out; ++j) {
        const float c = ((float)j + 0.5f) * r;
        double lo = floorf(c - s), hi = ceilf(c + s);
        lo = lo < 0.0 ? 0.0 : lo > (double)(n_in - 1u) ? (double)(n_in - 1u) : lo;
        hi = hi < lo + 1.0 ? lo + 1.0 : hi > (double)n_in ? (double)n_in : hi;
        const uint32_t l = (uint32_t)lo, n = (uint32_t)hi - l;
        k.resize(n);
        float sum = 0.0f;
        for (uint32_t i = 0; i < n; ++i) {
            const float x = ((float)(l + i) - (c - 0.5f)) / sr;
            k[i] = (float)rd_lanczos3((double)x);
            sum = sum + k[i];
        }
        left[j] = l; count[j] = n; off[j] = (uint32_t)w.size();
        for (uint32_t i = 0; i < n; ++i) w.push_back(k[i] / sum);
        if (padded) while (w.size() % 4u) w.push_back(0.0f);
    }
}

extern "C" int rd_tier_dims(uint32_t W, uint32_t H, uint32_t box_w, uint32_t box_h, uint32_t *w, uint32_t *h) try
{
    RD_ENTRY(rd_tier_dims);
    if (!w || !h) return rd_fail(RD_ERR_INVALID_ARG, "rd_tier_dims: NULL output");
    if (!W || !H) return rd_fail(RD_ERR_INVALID_ARG, "rd_tier_dims: empty frame %ux%u", W, H);
    if (!box_w || !box_h) return rd_fail(RD_ERR_INVALID_ARG, "rd_tier_dims: empty box %ux%u", box_w, box_h);
    return rd_tier_fit(W, H, box_w, box_h, w, h);
}
RD_CATCH_INT(rd_tier_dims)

extern "C" int rd_tier_weights(uint32_t n_in, uint32_t n_out, uint32_t *left, uint32_t *count, float *w, size_t w_cap,
                               size_t *w_needed) try
{
    RD_ENTRY(rd_tier_weights);
    if (!n_in || !n_out) return rd_fail(RD_ERR_INVALID_ARG, "rd_tier_weights: empty axis %u -> %u", n_in, n_out);
    if (!w_needed) return rd_fail(RD_ERR_INVALID_ARG, "rd_tier_weights: w_needed is NULL");
    std::vector<uint32_t> l, c, o;
    std::vector<float> wt;
    rd_tier_axis_build(n_in, n_out, false, l, c, o, wt);
    *w_needed = wt.size();
    if (w && w_cap < wt.size()) return rd_fail(RD_ERR_INVALID_ARG, "rd_tier_weights: %zu weights do not fit %zu", wt.size(), w_cap);
    if (left) memcpy(left, l.data(), l.size() * sizeof(uint32_t));
    if (count) memcpy(count, c.data(), c.size() * sizeof(uint32_t));
    if (w) memcpy(w, wt.data(), wt.size() * sizeof(float));
    return RD_OK;
}
RD_CATCH_INT(rd_tier_weights)

struct rd_tiers {
    int device = 0;
    uint32_t W = 0, H = 0, fmt = 0, n_tiers = 0;
    int n_cu = 256;
    uint32_t frames_per_launch = 1;
    size_t lds = 0;
    rd_tiers_geom geom{};
    void *tables = nullptr;                      // every axis table of every tier, one allocation
    float *scratch = nullptr;                    // frames_per_launch slices of T
};

extern "C" void rd_tiers_destroy(rd_tiers *t) try
{
    if (!t) return;
    {
        rd_devguard g(t->device);
        (void)hipDeviceSynchronize();                            // launches on the caller's stream still read the tables and T
        if (t->tables) (void)hipFree(t->tables);
        if (t->scratch) (void)hipFree(t->scratch);
    }
    delete t;
}
RD_CATCH_VOID(rd_tiers_destroy)

// T of all frames of one launch should stay in the 256 MiB Infinity Cache between the two passes.
#define RD_TIERS_SCRATCH_TARGET (192ull << 20)

extern "C" int rd_tiers_create(int device, uint32_t W, uint32_t H, uint32_t format, uint32_t n_tiers, const uint32_t *box_w,
                               const uint32_t *box_h, rd_tiers **out) try
{
    RD_ENTRY(rd_tiers_create);
    if (!out) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_create: out is NULL");
    *out = nullptr;
    if (!W || !H) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_create: empty frame %ux%u", W, H);
    if (format != RD_FMT_RGBA_U8 && format != RD_FMT_RGB_U8)
        return rd_fail(RD_ERR_UNSUPPORTED, "rd_tiers_create: format %u (tiers are RD_FMT_RGBA_U8 or RD_FMT_RGB_U8)", format);
    if (n_tiers < 1u || n_tiers > RD_TIERS_MAX) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_create: %u tiers (1 to %u)", n_tiers, RD_TIERS_MAX);
    if (!box_w || !box_h) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_create: NULL box array");
    uint32_t tw[RD_TIERS_MAX] = {}, th[RD_TIERS_MAX] = {};
    for (uint32_t i = 0; i < n_tiers; ++i) {
        if (!box_w[i] || !box_h[i]) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_create: tier %u has an empty box %ux%u", i, box_w[i], box_h[i]);
        const int rc = rd_tier_fit(W, H, box_w[i], box_h[i], &tw[i], &th[i]);
        if (rc) return rc;
        if (tw[i] > 65536u || th[i] > 65536u)
            return rd_fail(RD_ERR_UNSUPPORTED, "rd_tiers_create: tier %u would be %ux%u (at most 65536 per side)", i, tw[i], th[i]);
    }
    // the horizontal kernel holds two developed rows (4 B per pixel) beside the 8-bit threshold table in one CU's LDS
    const size_t lds = (size_t)RD_Q8_LUT_LDS_WORDS * 4u + (size_t)W * 8u;
    if (lds > RD_TIERS_LDS_MAX)
        return rd_fail(RD_ERR_UNSUPPORTED, "rd_tiers_create: a %u px wide frame does not fit the row-pair stage in LDS (at most %u px)",
                       W, (uint32_t)((RD_TIERS_LDS_MAX - RD_Q8_LUT_LDS_WORDS * 4u) / 8u));
    if (!rd_identity_map(W) || !rd_identity_map(H)) return rd_fail(RD_ERR_UNSUPPORTED, "export map is not the identity for %ux%u", W, H);
    int n_cu = 0;
    int rc = rd_check_device(device, &n_cu);
    if (rc) return rc;
    rd_devguard g(device);
    if (!g.ok) return rd_fail(RD_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    rc = rd_q8_lut_ensure(device);
    if (rc) return rc;
    rd_tiers *t = new (std::nothrow) rd_tiers;
    if (!t) return rd_fail(RD_ERR_OOM, "host allocation failed");
    struct undo { void operator()(rd_tiers *q) const { rd_tiers_destroy(q); } };
    std::unique_ptr<rd_tiers, undo> hold(t);
    t->device = device; t->W = W; t->H = H; t->fmt = format; t->n_tiers = n_tiers; t->n_cu = n_cu; t->lds = lds;
    rd_tiers_geom &gm = t->geom;
    gm.W = W; gm.H = H; gm.n_tiers = n_tiers;

    // tables: per tier and axis left / count / off (u32) then the weights (horizontal: tap-major), each array 16-byte aligned
    RD_FAULT_POINT("tiers.tables");
    std::vector<uint8_t> blob;
    auto put = [&blob](const void *p, size_t bytes) {
        const size_t at = (blob.size() + 15u) & ~(size_t)15u;
        blob.resize(at + bytes);
        if (bytes) memcpy(blob.data() + at, p, bytes);
        return at;
    };
    size_t at[RD_TIERS_MAX][2][4];
    uint64_t tfloats = 0;
    uint32_t hitems = 0, vrows = 0;
    for (uint32_t i = 0; i < n_tiers; ++i) {
        gm.tw[i] = tw[i]; gm.th[i] = th[i];
        gm.hbase[i] = hitems; gm.vbase[i] = vrows;
        hitems += tw[i]; vrows += th[i];
        gm.t_off[i] = tfloats;
        tfloats += (uint64_t)H * tw[i] * 3u;
        for (int a = 0; a < 2; ++a) {
            std::vector<uint32_t> l, c, o;
            std::vector<float> wt;
            if (a == 0) {                                        // horizontal: tap-major (rd_tiers.h, rd_tier_axis)
                rd_tier_axis_build(W, tw[i], false, l, c, o, wt);
                const uint32_t maxc = *std::max_element(c.begin(), c.end());
                std::vector<float> tm((size_t)maxc * tw[i], 0.0f);
                for (uint32_t j = 0; j < tw[i]; ++j)
                    for (uint32_t k = 0; k < c[j]; ++k) tm[(size_t)k * tw[i] + j] = wt[o[j] + k];
                wt.swap(tm);
            } else {
                rd_tier_axis_build(H, th[i], true, l, c, o, wt);
            }
            at[i][a][0] = put(l.data(), l.size() * 4u);
            at[i][a][1] = put(c.data(), c.size() * 4u);
            at[i][a][2] = put(o.data(), o.size() * 4u);
            at[i][a][3] = put(wt.data(), wt.size() * 4u);
        }
    }
    gm.hitems = hitems; gm.vbase[n_tiers] = vrows;
    gm.t_frame = (tfloats + 63u) & ~(uint64_t)63u;               // slices start on 256-byte boundaries
    const uint64_t frame_bytes = gm.t_frame * sizeof(float);
    uint64_t fpl = RD_TIERS_SCRATCH_TARGET / frame_bytes;
    t->frames_per_launch = (uint32_t)(fpl < 1u ? 1u : fpl > RD_TIERS_LAUNCH_MAX ? RD_TIERS_LAUNCH_MAX : fpl);
    RD_HIP(hipMalloc(&t->tables, blob.size()));
    RD_HIP(hipMemcpy(t->tables, blob.data(), blob.size(), hipMemcpyHostToDevice));
    RD_HIP(hipMalloc((void **)&t->scratch, (size_t)frame_bytes * t->frames_per_launch));
    gm.scratch = t->scratch;
    const uint8_t *base = (const uint8_t *)t->tables;
    for (uint32_t i = 0; i < n_tiers; ++i)
        for (int a = 0; a < 2; ++a) {
            rd_tier_axis &ax = a == 0 ? gm.hx[i] : gm.vy[i];
            ax.left = (const uint32_t *)(base + at[i][a][0]);
            ax.count = (const uint32_t *)(base + at[i][a][1]);
            ax.off = (const uint32_t *)(base + at[i][a][2]);
            ax.w = (const float *)(base + at[i][a][3]);
        }
    if (lds > 65536u) RD_HIP(hipFuncSetAttribute((const void *)rd_tiers_hpass, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    *out = hold.release();
    return RD_OK;
}
RD_CATCH_INT(rd_tiers_create)

extern "C" int rd_tiers_info(const rd_tiers *t, uint32_t tier, uint32_t *w, uint32_t *h) try
{
    RD_ENTRY(rd_tiers_info);
    if (!t || !w || !h) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_info: NULL argument");
    if (tier >= t->n_tiers) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_info: tier %u of %u", tier, t->n_tiers);
    *w = t->geom.tw[tier];
    *h = t->geom.th[tier];
    return RD_OK;
}
RD_CATCH_INT(rd_tiers_info)

extern "C" int rd_tiers_develop(rd_tiers *t, const rd_frame *frames, size_t n_frames, void *const *tier_dev, void *stream) try
{
    RD_ENTRY(rd_tiers_develop);
    if (!t) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_develop: NULL context");
    if (!n_frames) return RD_OK;
    if (!frames || !tier_dev) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_develop: NULL frame or tier array");
    for (size_t i = 0; i < n_frames; ++i) {
        const rd_frame &fr = frames[i];
        if (!fr.cfa_dev || ((uintptr_t)fr.cfa_dev & 1u)) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_develop: frame %zu: CFA plane NULL or misaligned", i);
        if (fr.matrix_layout > RD_MATRIX_ROW_MAJOR) return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_develop: frame %zu: matrix layout %u", i, fr.matrix_layout);
        for (uint32_t k = 0; k < t->n_tiers; ++k) {
            const void *p = tier_dev[i * t->n_tiers + k];
            if (!p || (t->fmt == RD_FMT_RGBA_U8 && ((uintptr_t)p & 3u)))
                return rd_fail(RD_ERR_INVALID_ARG, "rd_tiers_develop: frame %zu tier %u: surface NULL or not 4-byte aligned", i, k);
        }
    }
    rd_devguard g(t->device);
    if (!g.ok) return rd_fail(RD_ERR_NO_DEVICE, "hipSetDevice(%d) failed", t->device);
    RD_FAULT_POINT("tiers.launch");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t units = t->H / 2u + 1u;
    (void)hipGetLastError();
    for (size_t f0 = 0; f0 < n_frames; f0 += t->frames_per_launch) {
        const uint32_t nf = (uint32_t)std::min<size_t>(t->frames_per_launch, n_frames - f0);
        rd_tiers_launch L{};
        for (uint32_t i = 0; i < nf; ++i) {
            const rd_frame &fr = frames[f0 + i];
            L.f[i].cfa = fr.cfa_dev;
            for (uint32_t k = 0; k < t->n_tiers; ++k) L.f[i].out[k] = (uint8_t *)tier_dev[(f0 + i) * t->n_tiers + k];
            L.f[i].u = rd_frame_ku(fr.params, fr.wb_multipliers, fr.color_matrix, 1.0f, 0.0f, 0.0f, fr.black_level, RD_MATH_STRICT,
                                   fr.matrix_layout);
        }
        // about four resident workgroups' worth of row pairs per CU over the launch's frames; a workgroup loads the
        // threshold table once for all of its row pairs
        uint32_t gx = (uint32_t)(((uint64_t)t->n_cu * 4u + nf - 1u) / nf);
        gx = gx < units ? gx : units;
        hipLaunchKernelGGL(rd_tiers_hpass, dim3(gx, nf), dim3(RD_TIERS_HBLOCK), t->lds, s, t->geom, L);
        if (t->fmt == RD_FMT_RGBA_U8)
            hipLaunchKernelGGL(rd_tiers_vpass<true>, dim3(t->geom.vbase[t->n_tiers], nf), dim3(RD_TIERS_VBLOCK), 0, s, t->geom, L);
        else
            hipLaunchKernelGGL(rd_tiers_vpass<false>, dim3(t->geom.vbase[t->n_tiers], nf), dim3(RD_TIERS_VBLOCK), 0, s, t->geom, L);
        RD_HIP(hipGetLastError());
    }
    return RD_OK;
}
RD_CATCH_INT(rd_tiers_develop)
