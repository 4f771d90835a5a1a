// rd_host_jpeg.inl -- host side of the baseline JPEG encoder (rd_jpeg_header, rd_jpeg_*; kernels in rd_jpeg.h).
// Included once from rawdev.hip.  The contract (marker layout, tables, colour, edges, DCT, entropy coding) is DESIGN.md
// section 12.

static const uint8_t rd_jpeg_zz_host[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.1, natural order
static const uint16_t rd_jpeg_base_q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: bits[1..16] then the values, for DC luma, AC luma, DC chroma, AC chroma
static const uint8_t rd_jpeg_dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                               {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t rd_jpeg_dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t rd_jpeg_ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                               {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t rd_jpeg_ac_vals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
     0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
     0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
     0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
     0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
     0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
     0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
     0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
     0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
     0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
     0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa}};

// Annex C: code | length << 16 per symbol (length 0: no code)
static void rd_jpeg_huff_codes(const uint8_t bits[16], const uint8_t *vals, uint32_t *out, size_t n_out)
{
    for (size_t i = 0; i < n_out; ++i) out[i] = 0u;
    uint32_t code = 0, k = 0;
    for (uint32_t len = 1; len <= 16u; ++len) {
        for (uint32_t i = 0; i < bits[len - 1u]; ++i, ++k, ++code) out[vals[k]] = code | (len << 16);
        code <<= 1;
    }
}

// the IJG quality rule (jpeg_quality_scaling + jpeg_add_quant_table with force_baseline), natural order
static void rd_jpeg_quant(uint32_t q, uint16_t out[2][64])
{
    const uint32_t scale = q < 50u ? 5000u / q : 200u - 2u * q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            uint32_t v = (rd_jpeg_base_q[t][i] * scale + 50u) / 100u;
            out[t][i] = (uint16_t)(v < 1u ? 1u : v > 255u ? 255u : v);
        }
}

static void rd_jpeg_seg(std::vector<uint8_t> &o, uint8_t marker, const std::vector<uint8_t> &payload)
{
    const size_t n = payload.size() + 2u;
    o.push_back(0xff); o.push_back(marker); o.push_back((uint8_t)(n >> 8)); o.push_back((uint8_t)n);
    o.insert(o.end(), payload.begin(), payload.end());
}

// libjpeg's marker order: SOI, APP0 JFIF 1.01, DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, DRI, SOS
static void rd_jpeg_build_header(uint32_t W, uint32_t H, uint32_t q, uint32_t sub, uint32_t R, std::vector<uint8_t> &o)
{
    o.clear();
    o.push_back(0xff); o.push_back(0xd8);
    rd_jpeg_seg(o, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    uint16_t qt[2][64];
    rd_jpeg_quant(q, qt);
    for (int t = 0; t < 2; ++t) {
        std::vector<uint8_t> p{(uint8_t)t};
        for (int k = 0; k < 64; ++k) p.push_back((uint8_t)qt[t][rd_jpeg_zz_host[k]]);
        rd_jpeg_seg(o, 0xdb, p);
    }
    const uint8_t hv = sub == RD_JPEG_420 ? 0x22 : 0x11;
    rd_jpeg_seg(o, 0xc0, {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t) {
        std::vector<uint8_t> p{(uint8_t)t};
        p.insert(p.end(), rd_jpeg_dc_bits[t], rd_jpeg_dc_bits[t] + 16);
        p.insert(p.end(), rd_jpeg_dc_vals, rd_jpeg_dc_vals + 12);
        rd_jpeg_seg(o, 0xc4, p);
        std::vector<uint8_t> a{(uint8_t)(0x10 | t)};
        a.insert(a.end(), rd_jpeg_ac_bits[t], rd_jpeg_ac_bits[t] + 16);
        a.insert(a.end(), rd_jpeg_ac_vals[t], rd_jpeg_ac_vals[t] + 162);
        rd_jpeg_seg(o, 0xc4, a);
    }
    rd_jpeg_seg(o, 0xdd, {(uint8_t)(R >> 8), (uint8_t)R});
    rd_jpeg_seg(o, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

static int rd_jpeg_check_args(const char *fn, uint32_t W, uint32_t H, uint32_t q, uint32_t sub, uint32_t R)
{
    if (W < 1u || W > 65535u || H < 1u || H > 65535u) return rd_fail(RD_ERR_INVALID_ARG, "%s: frame %ux%u (1 to 65535 per side)", fn, W, H);
    if (q < 1u || q > 100u) return rd_fail(RD_ERR_INVALID_ARG, "%s: quality %u (1 to 100)", fn, q);
    if (sub != RD_JPEG_420 && sub != RD_JPEG_444) return rd_fail(RD_ERR_INVALID_ARG, "%s: subsampling %u (RD_JPEG_420 or RD_JPEG_444)", fn, sub);
    if (R < 1u || R > 65535u) return rd_fail(RD_ERR_INVALID_ARG, "%s: restart interval %u MCUs (1 to 65535)", fn, R);
    return RD_OK;
}

extern "C" int rd_jpeg_header(uint32_t W, uint32_t H, uint32_t quality, uint32_t subsampling, uint32_t restart_mcus,
                              uint8_t *buf, size_t cap, size_t *len) try
{
    RD_ENTRY(rd_jpeg_header);
    if (!len) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_header: len is NULL");
    const int rc = rd_jpeg_check_args("rd_jpeg_header", W, H, quality, subsampling, restart_mcus);
    if (rc) return rc;
    std::vector<uint8_t> h;
    rd_jpeg_build_header(W, H, quality, subsampling, restart_mcus, h);
    *len = h.size();
    if (buf && cap < h.size()) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_header: %zu bytes do not fit %zu", h.size(), cap);
    if (buf) memcpy(buf, h.data(), h.size());
    return RD_OK;
}
RD_CATCH_INT(rd_jpeg_header)

struct rd_jpeg {
    int device = 0;
    uint32_t fmt = 0;
    uint32_t frames_per_launch = 1;
    size_t max_bytes = 0, hdr_bytes = 0;
    rd_jpeg_geom geom{};
    void *tables = nullptr;                      // rd_jpeg_tables + the header, one allocation
    void *scratch = nullptr;                     // frames_per_launch x (coefficients, interval slots, interval lengths)
};

extern "C" void rd_jpeg_destroy(rd_jpeg *j) try
{
    if (!j) return;
    {
        rd_devguard g(j->device);
        (void)hipDeviceSynchronize();                            // launches on the caller's stream still read the scratch
        if (j->tables) (void)hipFree(j->tables);
        if (j->scratch) (void)hipFree(j->scratch);
    }
    delete j;
}
RD_CATCH_VOID(rd_jpeg_destroy)

// The scratch of all frames of one launch: mostly worst-case interval slots that are never touched in full, so the bound is
// on the allocation, not on traffic.
#define RD_JPEG_SCRATCH_TARGET (1ull << 30)

extern "C" int rd_jpeg_create(int device, uint32_t W, uint32_t H, uint32_t format, uint32_t quality, uint32_t subsampling,
                              uint32_t restart_mcus, rd_jpeg **out) try
{
    RD_ENTRY(rd_jpeg_create);
    if (!out) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_create: out is NULL");
    *out = nullptr;
    int rc = rd_jpeg_check_args("rd_jpeg_create", W, H, quality, subsampling, restart_mcus);
    if (rc) return rc;
    if (format != RD_FMT_RGBA_U8 && format != RD_FMT_RGB_U8)
        return rd_fail(RD_ERR_UNSUPPORTED, "rd_jpeg_create: format %u (the encoder takes RD_FMT_RGB_U8 or RD_FMT_RGBA_U8)", format);
    int n_cu = 0;
    rc = rd_check_device(device, &n_cu);
    if (rc) return rc;
    rd_devguard g(device);
    if (!g.ok) return rd_fail(RD_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    rd_jpeg *j = new (std::nothrow) rd_jpeg;
    if (!j) return rd_fail(RD_ERR_OOM, "host allocation failed");
    struct undo { void operator()(rd_jpeg *q) const { rd_jpeg_destroy(q); } };
    std::unique_ptr<rd_jpeg, undo> hold(j);
    j->device = device; j->fmt = format;

    rd_jpeg_tables tab{};
    uint16_t qt[2][64];
    rd_jpeg_quant(quality, qt);
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const uint64_t d = 8u * (uint64_t)qt[t][i];
            tab.qmul[t][i] = (uint32_t)(((1ull << 32) + d - 1u) / d);
            tab.qhalf[t][i] = (uint32_t)(d >> 1);
        }
    uint32_t block_bits[2] = {0, 0};                             // the longest block of each table pair
    for (int t = 0; t < 2; ++t) {
        rd_jpeg_huff_codes(rd_jpeg_dc_bits[t], rd_jpeg_dc_vals, tab.dc[t], 16);
        rd_jpeg_huff_codes(rd_jpeg_ac_bits[t], rd_jpeg_ac_vals[t], tab.ac[t], 256);
        uint32_t dmax = 0, amax = 0;
        for (uint32_t s = 0; s < 12u; ++s) dmax = std::max(dmax, (tab.dc[t][s] >> 16) + s);
        for (uint32_t s = 0; s < 256u; ++s)
            if (tab.ac[t][s] >> 16) amax = std::max(amax, (tab.ac[t][s] >> 16) + (s & 15u));
        block_bits[t] = dmax + 63u * amax;
        if (block_bits[t] > RD_JPEG_BLOCK_MAX_BITS) return rd_fail(RD_ERR_INTERNAL, "rd_jpeg_create: table bound %u bits", block_bits[t]);
    }
    std::vector<uint8_t> hdr;
    rd_jpeg_build_header(W, H, quality, subsampling, restart_mcus, hdr);

    rd_jpeg_geom &gm = j->geom;
    const bool s420 = subsampling == RD_JPEG_420;
    const uint32_t m = s420 ? 16u : 8u;
    gm.W = W; gm.H = H; gm.bpp = format == RD_FMT_RGBA_U8 ? 4u : 3u;
    gm.mcux = (W + m - 1u) / m; gm.mcuy = (H + m - 1u) / m; gm.n_mcu = gm.mcux * gm.mcuy;
    gm.bpm = s420 ? 6u : 3u; gm.sub420 = s420 ? 1u : 0u; gm.R = restart_mcus;
    gm.n_int = (gm.n_mcu + restart_mcus - 1u) / restart_mcus;
    gm.hdr_len = (uint32_t)hdr.size();
    // concat: at most about 512 workgroups per frame (each sums the lengths before its group), at least 8 intervals each
    gm.group_n = std::max(8u, (gm.n_int + 511u) / 512u);
    gm.groups = (gm.n_int + gm.group_n - 1u) / gm.group_n;
    const uint64_t mcu_bits = s420 ? 4ull * block_bits[0] + 2ull * block_bits[1] : (uint64_t)block_bits[0] + 2ull * block_bits[1];
    const uint64_t int_bytes = 2ull * ((mcu_bits * std::min(restart_mcus, gm.n_mcu) + 7u) / 8u);   // every byte stuffed
    gm.slot_bytes = (int_bytes + 15u) & ~15ull;
    gm.coef_frame = (uint64_t)gm.n_mcu * gm.bpm * 64u;
    j->hdr_bytes = hdr.size();
    j->max_bytes = hdr.size() + (size_t)int_bytes * gm.n_int + 2u * (size_t)gm.n_int;             // RSTn x (n - 1) + EOI
    const uint64_t coef_b = gm.coef_frame * 2u, slot_b = gm.slot_bytes * gm.n_int, len_b = ((uint64_t)gm.n_int * 4u + 255u) & ~255ull;
    const uint64_t frame_b = ((coef_b + 255u) & ~255ull) + ((slot_b + 255u) & ~255ull) + len_b;
    const uint64_t fpl = RD_JPEG_SCRATCH_TARGET / frame_b;
    j->frames_per_launch = (uint32_t)(fpl < 1u ? 1u : fpl > RD_JPEG_LAUNCH_MAX ? RD_JPEG_LAUNCH_MAX : fpl);

    RD_FAULT_POINT("jpeg.scratch");
    const size_t tab_b = (sizeof(rd_jpeg_tables) + 255u) & ~(size_t)255u;
    RD_HIP(hipMalloc(&j->tables, tab_b + hdr.size()));
    RD_HIP(hipMemcpy(j->tables, &tab, sizeof(tab), hipMemcpyHostToDevice));
    RD_HIP(hipMemcpy((uint8_t *)j->tables + tab_b, hdr.data(), hdr.size(), hipMemcpyHostToDevice));
    const uint64_t nf = j->frames_per_launch;
    RD_HIP(hipMalloc(&j->scratch, (size_t)(frame_b * nf)));
    uint8_t *s = (uint8_t *)j->scratch;
    gm.coef = (int16_t *)s;
    gm.bits = s + ((coef_b + 255u) & ~255ull) * nf;
    gm.lens = (uint32_t *)(gm.bits + ((slot_b + 255u) & ~255ull) * nf);
    gm.tab = (const rd_jpeg_tables *)j->tables;
    gm.hdr = (const uint8_t *)j->tables + tab_b;
    *out = hold.release();
    return RD_OK;
}
RD_CATCH_INT(rd_jpeg_create)

extern "C" int rd_jpeg_info(const rd_jpeg *j, size_t *max_bytes, size_t *header_bytes) try
{
    RD_ENTRY(rd_jpeg_info);
    if (!j) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_info: NULL context");
    if (max_bytes) *max_bytes = j->max_bytes;
    if (header_bytes) *header_bytes = j->hdr_bytes;
    return RD_OK;
}
RD_CATCH_INT(rd_jpeg_info)

extern "C" int rd_jpeg_encode(rd_jpeg *j, const void *const *src_dev, size_t n_frames, size_t src_pitch, void *const *dst_dev,
                              size_t dst_cap, uint64_t *len_dev, void *stream) try
{
    RD_ENTRY(rd_jpeg_encode);
    if (!j) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_encode: NULL context");
    if (!n_frames) return RD_OK;
    if (!src_dev || !dst_dev) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_encode: NULL source or destination array");
    if (!len_dev || ((uintptr_t)len_dev & 7u)) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_encode: length array NULL or not 8-byte aligned");
    const rd_jpeg_geom &gm = j->geom;
    if (src_pitch < (size_t)gm.W * gm.bpp)
        return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_encode: pitch %zu is below a row of %u px x %u B", src_pitch, gm.W, gm.bpp);
    if (dst_cap < j->max_bytes)
        return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_encode: dst_cap %zu is below the worst case %zu (rd_jpeg_info)", dst_cap, j->max_bytes);
    for (size_t i = 0; i < n_frames; ++i)
        if (!src_dev[i] || !dst_dev[i]) return rd_fail(RD_ERR_INVALID_ARG, "rd_jpeg_encode: frame %zu: NULL surface or buffer", i);
    rd_devguard g(j->device);
    if (!g.ok) return rd_fail(RD_ERR_NO_DEVICE, "hipSetDevice(%d) failed", j->device);
    RD_FAULT_POINT("jpeg.launch");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t dct_groups = (gm.n_mcu * gm.bpm + RD_JPEG_DCT_BLOCK - 1u) / RD_JPEG_DCT_BLOCK;
    (void)hipGetLastError();
    for (size_t f0 = 0; f0 < n_frames; f0 += j->frames_per_launch) {
        const uint32_t nf = (uint32_t)std::min<size_t>(j->frames_per_launch, n_frames - f0);
        rd_jpeg_launch L{};
        for (uint32_t i = 0; i < nf; ++i) {
            L.src[i] = (const uint8_t *)src_dev[f0 + i];
            L.dst[i] = (uint8_t *)dst_dev[f0 + i];
        }
        L.len = len_dev + f0;
        L.pitch = src_pitch;
        hipLaunchKernelGGL(rd_jpeg_dct, dim3(dct_groups, nf), dim3(RD_JPEG_DCT_BLOCK), 0, s, gm, L);
        hipLaunchKernelGGL(rd_jpeg_huff, dim3(gm.n_int, nf), dim3(64), 0, s, gm, L);
        hipLaunchKernelGGL(rd_jpeg_concat, dim3(gm.groups, nf), dim3(RD_JPEG_CONCAT_BLOCK), 0, s, gm, L);
        RD_HIP(hipGetLastError());
    }
    return RD_OK;
}
RD_CATCH_INT(rd_jpeg_encode)
