// nyxhip_dispatch.hip -- from a device-resident batch to kernel launches: LDS / workspace layouts, argument blocks, size classes.
#include "nyxhip_ctx.h"
#include "features_plan.h"

using namespace nyxhip;

namespace {

uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

// One n x n complex Gabor kernel, interleaved re/im, L1-normalised by the sum of magnitudes:
// the formula and evaluation order of GaborFeature::Gabor (features/gabor.cpp:393-449), run
// on the host with libm exactly as the reference does.
void gabor_filter(double* Gex, double f0, double sig2lam, double gamma, double theta, double fi, int n)
{
    const double lambda = 2 * M_PI / f0, cos_theta = cos(theta), sin_theta = sin(theta), sig = sig2lam * lambda;
    std::vector<double> tx(n + 1), ty(n + 1);
    tx[0] = (n % 2 > 0) ? -((n - 1) / 2) : -(n / 2);
    for (int x = 1; x < n; x++) tx[x] = tx[x - 1] + 1;
    ty[0] = tx[0];
    for (int y = 1; y < n; y++) ty[y] = ty[y - 1] + 1;
    double sum = 0;
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++) {
            double xte = tx[x] * cos_theta + ty[y] * sin_theta;
            double yte = ty[y] * cos_theta - tx[x] * sin_theta;
            double rte = xte * xte + gamma * gamma * yte * yte;
            double ge = exp(-1 * rte / (2 * sig * sig));
            double argm = xte * f0 + fi;
            int idx = y * n * 2 + x * 2;
            Gex[idx] = ge * cos(argm);
            Gex[idx + 1] = ge * sin(argm);
            sum += sqrt(pow(Gex[idx], 2) + pow(Gex[idx + 1], 2));
        }
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n * 2; x++)
            Gex[y * n * 2 + x] /= sum;
}

// Low-pass baseline filter (f0LP at theta = pi/2, gabor.cpp:79) followed by the (f0, theta) pairs.
int ensure_gabor_bank(nyxhip_ctx* ctx, const nyxhip_settings* s)
{
    const int n = s->gabor_kersize, nF = s->gabor_n_filters;
    std::vector<double> key = {s->gabor_gamma, s->gabor_sig2lam, s->gabor_f0lp, (double)n, (double)nF};
    for (int i = 0; i < nF; i++) { key.push_back(s->gabor_f0[i]); key.push_back(s->gabor_theta[i]); }
    if (ctx->d_bank && key == ctx->bank_key)
        return NYXHIP_OK;
    std::vector<double> bank((size_t)(nF + 1) * n * n * 2);
    gabor_filter(bank.data(), s->gabor_f0lp, s->gabor_sig2lam, s->gabor_gamma, M_PI_2, 0, n);
    for (int f = 0; f < nF; f++)
        gabor_filter(bank.data() + (size_t)(f + 1) * n * n * 2, s->gabor_f0[f], s->gabor_sig2lam, s->gabor_gamma, s->gabor_theta[f], 0, n);
    for (int f = 0; f <= NYXHIP_MAX_GABOR_FILTERS; f++) ctx->bank_zero_rows[f] = 0;
    if (n == 16)
        for (int f = 0; f <= nF; f++)
            for (int j = 0; j < n; j++) {
                bool re0 = true, im0 = true;
                for (int i = 0; i < n; i++) {
                    const double* t = bank.data() + ((size_t)f * n * n + (size_t)j * n + i) * 2;
                    re0 = re0 && t[0] == 0.0;             // (+0 and -0 alike; a NaN or a denormal is not zero)
                    im0 = im0 && t[1] == 0.0;
                }
                ctx->bank_zero_rows[f] |= (re0 ? 1u << j : 0u) | (im0 ? 1u << (16 + j) : 0u);
            }
    ctx->bank_box_mask = 0;
    if (n == 16)
        for (int f = 0; f <= nF; f++) {
            const double* t = bank.data() + (size_t)f * n * n * 2;
            int e = 0;
            bool box = t[0] > 0.0 && std::frexp(t[0], &e) == 0.5 && t[0] >= 0x1p-64 && t[0] <= 1.0;   // a power of two (2^-8 in the default bank)
            for (int k = 0; k < n * n && box; k++)
                box = t[2 * k] == t[0] && t[2 * k + 1] == 0.0;
            if (box) ctx->bank_box_mask |= 1u << f;
        }
    // the low-pass filter as an outer product C_j B_i (ShapeArgs::gabor_lp_sep): pivot at the tap of largest magnitude
    ctx->bank_lp_sep = 0;
    if (n == 16) {
        const double* t = bank.data();
        int j0 = 0, i0 = 0;
        double best = -1.0, l1 = 0.0;
        for (int j = 0; j < 16; j++)
            for (int i = 0; i < 16; i++) {
                const double m = std::hypot(t[(j * 16 + i) * 2], t[(j * 16 + i) * 2 + 1]);
                l1 += m;
                if (m > best) { best = m; j0 = j; i0 = i; }
            }
        double B[16], resid = 0.0;
        bool ok = best > 0.0 && std::isfinite(l1);
        for (int i = 0; i < 16 && ok; i++) {
            // B_i = tap(j0, i) / tap(j0, i0), which must be real and non-negative
            const double ar = t[(j0 * 16 + i) * 2], ai = t[(j0 * 16 + i) * 2 + 1], pr = t[(j0 * 16 + i0) * 2], pi = t[(j0 * 16 + i0) * 2 + 1];
            B[i] = (ar * pr + ai * pi) / (pr * pr + pi * pi);
            ok = B[i] >= 0.0;
        }
        for (int j = 0; j < 16 && ok; j++)
            for (int i = 0; i < 16; i++) {
                const double cr = t[(j * 16 + i0) * 2], ci = t[(j * 16 + i0) * 2 + 1];
                resid += std::hypot(t[(j * 16 + i) * 2] - cr * B[i], t[(j * 16 + i) * 2 + 1] - ci * B[i]);
            }
        if (ok && resid <= 1e-12 * l1) {
            ctx->bank_lp_sep = 1;
            memset(ctx->bank_lp_C, 0, sizeof(ctx->bank_lp_C));
            for (int i = 0; i < 16; i++) ctx->bank_lp_B[i] = (float)B[i];
            for (int j = 0; j < 16; j++) { ctx->bank_lp_C[2 * (j + 3)] = (float)t[(j * 16 + i0) * 2]; ctx->bank_lp_C[2 * (j + 3) + 1] = (float)t[(j * 16 + i0) * 2 + 1]; }
        }
        if (knob::debug()) fprintf(stderr, "[nyxhip] gabor low-pass: separable %u (residual %.3g of %.3g)\n", ctx->bank_lp_sep, resid, l1);
    }
    if (ctx->d_bank) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream()));
    ctx->d_bank.release(); ctx->d_bank32.release(); ctx->d_bank16.release();      // (a new bank is a new block, whatever its size)
    HIP_TRY(ctx, ctx->d_bank.reserve(bank.size() * sizeof(double), nullptr));
    HIP_TRY(ctx, hipMemcpy(ctx->d_bank.p, bank.data(), bank.size() * sizeof(double), hipMemcpyHostToDevice));
    {
        std::vector<float> b32(bank.size());
        for (size_t i = 0; i < bank.size(); i++) b32[i] = (float)bank[i];      // round to nearest: relative 2^-24 (the bound of the screening pass counts it)
        HIP_TRY(ctx, ctx->d_bank32.reserve(b32.size() * sizeof(float), nullptr));
        HIP_TRY(ctx, hipMemcpy(ctx->d_bank32.p, b32.data(), b32.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (n == 16 && nF > 0) {
        // MFMA screening stage of roi_gabor_tiled_kernel (MODE 4): the band-pass filters in groups of four as B operands of
        // v_mfma_f32_16x16x32_f16.  Operand (group g, tap-row pair jp), lane l = (column nn = l % 16, k block kb = l / 16), element t:
        // tap (j', i') = (2 jp + kb / 2, 8 (kb % 2) + t) of the FLIPPED kernel -- the convolution as a correlation over the padded
        // plane: out(a, b) = sum P[b + j'][a + 1 + i'] G[15 - j'][15 - i'] -- of filter 1 + 4 g + (nn % 8) / 2, component nn % 2,
        // scaled by 2^14; columns 0 .. 7 carry the f16 nearest to the scaled tap, columns 8 .. 15 the f16 nearest to the rest.
        const int groups = (nF + 3) / 4;
        std::vector<_Float16> ops((size_t)groups * 8 * 64 * 8);
        for (int g = 0; g < groups; g++)
            for (int jp = 0; jp < 8; jp++)
                for (int l = 0; l < 64; l++)
                    for (int t = 0; t < 8; t++) {
                        const int nn = l & 15, kb = l >> 4, f = 1 + 4 * g + ((nn & 7) >> 1), c = nn & 1, jq = 2 * jp + (kb >> 1), iq = 8 * (kb & 1) + t;
                        _Float16 v = (_Float16)0.0f;
                        if (f <= nF) {
                            const double tap = bank[(((size_t)f * 16 + (15 - jq)) * 16 + (15 - iq)) * 2 + c] * kGaborTapScale;
                            const _Float16 hi = (_Float16)tap;
                            v = nn < 8 ? hi : (_Float16)(tap - (double)hi);
                        }
                        ops[(((size_t)g * 8 + jp) * 64 + l) * 8 + t] = v;
                    }
        HIP_TRY(ctx, ctx->d_bank16.reserve(ops.size() * sizeof(_Float16), nullptr));
        HIP_TRY(ctx, hipMemcpy(ctx->d_bank16.p, ops.data(), ops.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    }
    ctx->bank_key = key;
    return NYXHIP_OK;
}

int make_shape_layout(uint32_t mask, const nyxhip_settings* s, uint32_t max_area, uint32_t max_side, ShapeLayout& L, std::string& why, size_t cap = 0)
{
    memset(&L, 0, sizeof(L));
    const bool spill = cap != 0;
    if (cap == 0) cap = roi_features_max_lds();
    if (!(mask & NYXHIP_FAM_GABOR))
        return NYXHIP_OK;
    uint32_t off = 0;
    if (!spill && s->gabor_kersize == 16) {
        // register-tiled kernel: one zero-padded u32 plane, (roundup(w, 8) + 16) x (h + 15) words <= area + 38 side + 345
        L.tiled = 1;
        L.red = off; off = align16(off + 8u * kWaves * NYXHIP_MAX_GABOR_FILTERS);
        L.area_cap = max_area ? max_area : 1;
        L.side_cap = max_side ? max_side : 1;
        const uint64_t words = (uint64_t)L.area_cap + 42ull * L.side_cap + 405;   // (w + 27) (h + 15): tiles + padding, pitch made an odd number of 16-byte units
        if (4ull * words + off > cap) { why = "ROI bounding box too large for the LDS-resident Gabor plane"; return NYXHIP_ERR_ROI_TOO_LARGE; }
        L.plane = off; off = align16(off + 4u * (uint32_t)words);
        L.redo = off; off = align16(off + 4u * (512u + 4u));     // kGaborRedoCap of roi_shape.hip
        L.total = off;
        return NYXHIP_OK;
    }
    L.red = off; off = align16(off + 8u * kWaves * 8);
    L.area_cap = max_area ? max_area : 1;
    if (16ull * L.area_cap > cap) { why = "ROI bounding box too large for the LDS-resident Gabor planes"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    L.plane = off; off = align16(off + 8u * L.area_cap);
    L.energy = off; off = align16(off + 8u * L.area_cap);
    L.bank = off; off = align16(off + 16u * (uint32_t)(s->gabor_n_filters + 1) * s->gabor_kersize * s->gabor_kersize);
    L.total = off;
    if (L.total > cap) { why = "ROI bounding box too large for the LDS-resident Gabor planes"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    return NYXHIP_OK;
}

// LDS carve-out of the texture kernel (roi_texture.hip)
int make_tex_layout(uint32_t mask, const nyxhip_settings* s, int n_cols, uint32_t max_area, uint32_t max_side,
                    TexLayout& L, std::string& why, size_t cap = 0, uint32_t vmax = 0)
{
    memset(&L, 0, sizeof(L));
    const bool spill = cap != 0;
    if (!spill) cap = roi_features_max_lds();
    const int greyInfo = s->ibsi ? 0 : s->grey_depth;
    uint32_t off = 0;
    L.out = off; off = align16(off + 8u * (uint32_t)n_cols);
    L.red = off; off = align16(off + 8u * kWaves * 8);
    L.stat = off; off = align16(off + 8u * 16);
    L.dense_cap = max_area ? max_area : 1;
    L.side_cap = max_side ? max_side : 1;
    if (2ull * L.dense_cap > cap) { why = "ROI bounding box of " + std::to_string(max_area) + " px exceeds the LDS-resident plane"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    // IBSI: levels are the intensities themselves -- up to the group's largest intensity when the class header gave it (exact launch
    // groups), else the 8-bit range
    L.lvl_cap = greyInfo != 0 ? (uint32_t)abs(greyInfo) : (vmax ? vmax : 255u);
    if (L.lvl_cap > 4094) { why = "grey depth (or IBSI intensity) above 4094 is not supported by the texture kernel"; return NYXHIP_ERR_UNSUPPORTED; }
    L.dense8 = (!spill && L.lvl_cap <= 254) ? 1u : 0u;            // 8-bit plane (roi_texture_kernel<.., true>)
    L.dense = off; off = align16(off + (L.dense8 ? 1u : 2u) * L.dense_cap + 4);
    L.ng_cap = L.lvl_cap + 1;
    L.lvlmap = off; off = align16(off + 2u * (L.lvl_cap + 4));
    L.lv = off; off = align16(off + 4u * (L.ng_cap + 4));
    if (L.ng_cap <= 256 && (mask & (NYXHIP_FAM_GLRLM | NYXHIP_FAM_GLSZM))) { L.lvf = off; off = align16(off + 16u * (L.ng_cap + 2)); }
    // NGTDM accumulators (u64 S[ng_cap + 2], u32 N[ng_cap + 2]).  Few levels mean few addresses under 64-lane atomics, which LDS
    // serialises: R replicas (lane % R picks one) keep the lanes per address near one; an odd multiple of 8 bytes apart so that the
    // replicas start in different banks.
    L.ngt_rep = 1; L.ngt_stride = ((L.ng_cap + 2) * 12u + 7u) & ~7u;
    if ((mask & NYXHIP_FAM_NGTDM) && !spill && L.ng_cap <= 64) {
        L.ngt_rep = L.ng_cap <= 16 ? 8u : L.ng_cap <= 32 ? 4u : 2u;
        L.ngt_stride = (((L.ng_cap + 2) * 12u + 16u + 7u) & ~7u) | 8u;
    }
    if ((mask & NYXHIP_FAM_NGTDM) && (mask & NYXHIP_FAM_GLSZM) && !spill && L.ng_cap <= 64) {
        // accumulators of its own: the stencil overlaps the GLSZM sweep
        L.ngt_own = off; off = align16(off + L.ngt_rep * L.ngt_stride);
    }
    L.work = off;
    size_t need = 0;
    if (mask & NYXHIP_FAM_NGTDM) {
        L.ngt_p = L.ngt_own ? 0u : (L.ngt_rep * L.ngt_stride + 15u) & ~15u;      // P[ng_cap + 2], S / 840 [ng_cap + 2] as doubles, behind the aliased accumulators
        need = std::max(need, (size_t)L.ngt_p + (size_t)(L.ng_cap + 2) * 16 + 64);
    }
    if (mask & NYXHIP_FAM_GLSZM) {
        // distinct (level, size) pairs <= sqrt(2 * Ng * area) (sizes of one level sum to <= its area)
        // (load <= 2/3 in the worst case; zones of up to 32 pixels bypass the hash altogether when the direct table exists.  With
        //  2 * distinct the benchmark's carve-out was 4 KiB larger: six instead of seven workgroups per CU.)  The kernel uses
        // szm_hash_cap of each ROI's OWN box, which this carve-out -- the same monotone function of the largest box -- covers.
        L.hash_cap = szm_hash_cap(L.ng_cap, L.dense_cap);
        // zone sizes (16-bit entries, two per word, while a size fits), hash, zones per level; the owner-label plane only
        // exists for boxes wider than one wave (the DPP sweep of narrower boxes keeps labels in registers)
        L.szm_c16 = (!spill && L.dense_cap < 65535u) ? 1 : 0;
        size_t szm = 0;
        L.szm_count = (uint32_t)szm; szm += ((L.szm_c16 ? 2ull : 4ull) * (L.dense_cap + 8) + 15) & ~15ull;
        L.szm_hkey = (uint32_t)szm; szm += 8ull * L.hash_cap + 4ull * (L.ng_cap + 4);
        szm = (szm + 15) & ~15ull;
        // direct [level][size] counters for the small zones (nearly all of them on textured images): one atomic, no probing
        L.szm_small = L.ng_cap <= 33 ? 32u : 0u;
        L.szm_smalltab = (uint32_t)szm; szm += 4ull * L.ng_cap * L.szm_small;
        szm = (szm + 15) & ~15ull;
        L.szm_label = (uint32_t)szm; if (L.side_cap > (spill ? 512u : 256u)) szm += 4ull * L.dense_cap;   // (boxes up to 256 wide keep their labels in registers: kSzmChunks of roi_texture.hip)
        L.szm_ok = (off + szm <= cap) ? 1 : 0;
        if (!L.szm_ok) { why = "ROI too large for the LDS-resident GLSZM zone tables"; return NYXHIP_ERR_ROI_TOO_LARGE; }
        need = std::max(need, szm);
    }
    if (mask & NYXHIP_FAM_GLRLM) {
        size_t slot = 4ull * ((size_t)L.ng_cap * L.side_cap + L.ng_cap + L.side_cap + 4);
        if (off + 512 + slot > cap) { why = "ROI too large for the LDS-resident run-length matrix"; return NYXHIP_ERR_ROI_TOO_LARGE; }
        size_t k = 4;
        while (k > 1 && off + 512 + k * slot > cap) k--;
        // keep the carve-out modest when four matrices would crowd out co-resident workgroups
        while (!spill && k > 1 && 512 + k * slot > 48 * 1024) k--;
        need = std::max(need, 512 + k * slot);
    }
    L.work_bytes = (uint32_t)need;
    off = align16(off + (uint32_t)need);
    L.total = off;
    if (L.total > cap) { why = "ROI too large for the LDS-resident texture path"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    if (spill) {
        // what a workspace launch keeps in LDS all the same: the atomics-heavy small state (64 lanes adding into a handful of
        // addresses are 64 serialised L2 atomics in global memory)
        uint32_t o = 0;
        if ((mask & NYXHIP_FAM_NGTDM) && L.ng_cap <= 1024) {
            L.ngt_rep = L.ng_cap <= 16 ? 8u : L.ng_cap <= 32 ? 4u : L.ng_cap <= 64 ? 2u : 1u;
            L.ngt_stride = (((L.ng_cap + 2) * 12u + 16u + 7u) & ~7u) | 8u;
            L.gs_ngt = o; L.gs_ngt_ok = 1; o = align16(o + L.ngt_rep * L.ngt_stride);
        }
        if ((mask & NYXHIP_FAM_GLRLM) && 16ull * L.ng_cap * kRlmLdsCols <= 32768) {
            L.gs_rlm = o; L.gs_rlm_ok = 1; o = align16(o + 16u * L.ng_cap * kRlmLdsCols);
        }
        L.gs_lds_bytes = o;
    }
    return NYXHIP_OK;
}

// Carve-out of roi_dependence_kernel (GLDZM + GLDM + NGLDM).
int make_dep_layout(uint32_t mask, const nyxhip_settings* s, uint32_t max_area, uint32_t max_side, DepLayout& L, std::string& why, size_t cap = 0,
                    uint32_t vmax = 0)
{
    memset(&L, 0, sizeof(L));
    if (cap == 0) cap = roi_features_max_lds();
    const int greyInfo = s->ibsi ? 0 : s->grey_depth;
    uint32_t off = 0;
    L.red = off; off = align16(off + 8u * kWaves * 8);
    L.stat = off; off = align16(off + 8u * 16);
    L.dense_cap = max_area ? max_area : 1;
    L.side_cap = max_side ? max_side : 1;
    if (4ull * L.dense_cap > cap) { why = "ROI bounding box of " + std::to_string(max_area) + " px exceeds the LDS-resident planes"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    L.lvl_cap = greyInfo != 0 ? (uint32_t)abs(greyInfo) : (vmax ? vmax : 255u);   // IBSI: levels are the intensities themselves
    if (L.lvl_cap > 4094) { why = "grey depth (or IBSI intensity) above 4094 is not supported by the dependence kernel"; return NYXHIP_ERR_UNSUPPORTED; }
    L.planes8 = (cap == roi_features_max_lds() && L.lvl_cap <= 63) ? 1u : 0u;   // byte planes: level + two flags fit 8 bits
    L.dense = off; off = align16(off + (L.planes8 ? 1u : 2u) * L.dense_cap + 4);
    L.aux = off; off = align16(off + (L.planes8 ? 1u : 2u) * L.dense_cap + 4);
    L.ng_cap = L.lvl_cap + 1;
    L.lvlmap = off; off = align16(off + 2u * (L.lvl_cap + 4));
    L.lv = off; off = align16(off + 4u * (L.ng_cap + 4));
    L.lvlmap2 = off; off = align16(off + 2u * (L.lvl_cap + 4));
    L.lv2 = off; off = align16(off + 4u * (L.ng_cap + 4));
    L.work = off;
    L.nd_cap = L.side_cap / 2 + 2;
    size_t need = (size_t)4 * 9 * (L.ng_cap + 1);                       // GLDM / NGLDM matrices
    if (mask & NYXHIP_FAM_GLDZM)                                     // union-find parents + matrix
        need = std::max<size_t>(need, 4ull * L.dense_cap + 4ull * (size_t)L.ng_cap * L.nd_cap + 64);
    if (cap == roi_features_max_lds() && L.ng_cap <= 65 && !knob::dep_seq()) {   // (NYXHIP_DEP_SEQ: A/B knob, sequential tails)
        // small matrices: GLDM's and NGLDM's sit side by side at the start of `work` -- where GLDZM keeps its union-find parents,
        // which are dead once its own matrix (behind them) is built -- so the three tails can run in parallel at the end without
        // a byte of extra LDS (the carve-out of the benchmark ROI sits 400 B below the five-workgroups-per-CU line)
        const size_t mat = ((size_t)4 * 9 * (L.ng_cap + 1) + 15) & ~(size_t)15;
        size_t base = 0;
        if ((mask & NYXHIP_FAM_GLDZM) && 2 * mat > 4ull * L.dense_cap)       // small boxes, many levels: the pair would reach GLDZM's own
            base = (4ull * L.dense_cap + 4ull * (size_t)L.ng_cap * L.nd_cap + 64 + 15) & ~15ull;   // matrix -- it goes behind it instead
        L.par = 1; L.off_pdm = (uint32_t)base; L.off_m = (uint32_t)(base + mat);
        need = std::max<size_t>(need, base + 2 * mat);
    }
    if (off + need > cap) { why = "ROI too large for the LDS-resident dependence / distance-zone tables"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    L.work_bytes = (uint32_t)need;
    off = align16(off + (uint32_t)need);
    L.total = off;
    return NYXHIP_OK;
}

__global__ void add_offset_kernel(const uint32_t* in, uint32_t add, uint32_t n, uint32_t* out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (in ? in[i] : i) + add;           // (in == NULL: add, add + 1, ...)
}

// Fills the three argument blocks for one set of extrema; `cap` = 0 -> LDS carve-outs, else spill layouts.
int build_args(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld,
               const Extrema& E, size_t cap, RoiArgs& a, TexArgs& t, ShapeArgs& g, DepArgs& d, std::string& why, uint32_t groups = 0xF)
{   // groups: bit 0 features (INTENSITY + GLCM), 1 texture, 2 shape, 3 dependence -- the kernel groups to build (columns always follow `mask`)
    const uint32_t mask1 = mask & (NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM), mask2 = mask & kTexture, mask3 = mask & kShape, mask4 = mask & kDependence;
    const int n_cols2 = nyxhip_n_columns(mask2, s), n_cols4 = nyxhip_n_columns(mask4, s);
    // The outline families (roi_outline.hip) sit between the intensity block and GLCM: every base behind the intensity block moves by
    // their columns.  n_cols1: where the INTENSITY + GLCM span ends.  The feature kernels zero and fill one span of columns from
    // column 0, so a launch with GLCM covers the outline columns as well (launch_device_all enqueues the outline kernel behind it).
    const int outline_cols = nyxhip_n_columns(mask & kBehindIntensity, s);   // (the caliper columns lie among them: roi_caliper.hip)
    const int n_cols1 = nyxhip_n_columns(mask1, s) + outline_cols;
    const int n_cols_feat = (mask1 & NYXHIP_FAM_GLCM) ? n_cols1 : n_cols1 - outline_cols;   // columns the feature kernel owns
    memset(&a, 0, sizeof(a));
    memset(&t, 0, sizeof(t));
    memset(&g, 0, sizeof(g));
    memset(&d, 0, sizeof(d));
    // Feature2D order inside the row: INTENSITY, GLCM, GLRLM, GLDZM, GLSZM, GLDM, NGLDM, NGTDM, GABOR, ZERNIKE
    int c_glrlm = n_cols1, c_gldzm = c_glrlm + ((mask & NYXHIP_FAM_GLRLM) ? kGlrlmCols : 0);
    int c_glszm = c_gldzm + ((mask & NYXHIP_FAM_GLDZM) ? kGldzmCols : 0), c_gldm = c_glszm + ((mask & NYXHIP_FAM_GLSZM) ? kGlszmCols : 0);
    int c_ngldm = c_gldm + ((mask & NYXHIP_FAM_GLDM) ? kGldmCols : 0);
    if (mask1 && (groups & 1)) {
        if (int lrc = make_layout(mask1, s, n_cols_feat, E.px, E.area, E.range, a.L, why, cap, E.vmax, E.wide_only))
            return lrc;
        a.n_roi = b->n_roi;
        a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.inten = b->inten;
        a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h; a.min_inten = b->min_inten; a.max_inten = b->max_inten;
        a.slide_min = b->slide_min; a.slide_max = b->slide_max;
        a.out = d_out; a.ld = ld; a.status = ctx->d_status.as<int>();
        a.stamps = ctx->d_stamps.as<unsigned long long>();
        if (cap == 0) a.win = ctx->win_next;   // LDS launches only (the tile path asks for windows only when everything fits LDS)
        a.mask = mask1; a.n_cols = n_cols_feat;
        int c = 0;
        a.col_intensity = a.col_glcm = -1;
        if (mask1 & NYXHIP_FAM_INTENSITY) { a.col_intensity = c; c += kIntensityCols; }
        c += outline_cols;
        if (mask1 & NYXHIP_FAM_GLCM) { a.col_glcm = c; c += kGlcmAngled * s->glcm_n_angles + kGlcmAve; }
        a.soft_nan = s->soft_nan;
        a.grey_depth = s->grey_depth; a.ibsi = s->ibsi; a.glcm_grey_depth = s->glcm_grey_depth;
        a.glcm_offset = s->glcm_offset; a.glcm_na = s->glcm_n_angles; a.glcm_symmetric = s->glcm_symmetric;
        for (int i = 0; i < kMaxAngles; i++) a.glcm_angles[i] = s->glcm_angles[i];
        a.n_hist = abs(s->grey_depth);
        if ((mask1 & NYXHIP_FAM_INTENSITY) && cap == 0) {      // (sized and cleared once per call by launch_device_all)
            a.close_rec = ctx->d_close_rec.as<double>();
            a.close_flag = ctx->close_flag;
        }
        // small matrices (order <= 16, all angles in one pass, matlab or IBSI level values 1..Ng): the features run as their
        // own launch with one wave per ROI (glcm_features_kernel); the counts travel through a context-owned workspace
        const int gi = s->ibsi ? 0 : s->grey_depth;
        if ((mask1 & NYXHIP_FAM_GLCM) && cap == 0 && gi >= 0 && a.L.ng_cap <= 16 && (int)a.L.app >= s->glcm_n_angles && s->glcm_n_angles > 0) {
            const size_t stride = (size_t)s->glcm_n_angles * a.L.ng_cap * a.L.ng_cap;
            const size_t need = 4 * stride * (size_t)b->n_roi + 256;
            if (ctx->d_glcm_ws.reserve(need, nullptr) != hipSuccess || !ctx->glcm_ng) {   // (glcm_ng: sized and cleared once per call by launch_device_all)
                why = "out of device memory for the GLCM count workspace";
                return NYXHIP_ERR_HIP;
            }
            {
                a.glcm_ng = ctx->glcm_ng;
                a.glcm_ws = ctx->d_glcm_ws.as<uint32_t>();
                a.glcm_ws_stride = (uint32_t)stride;
            }
        }
    }
    if (mask2 && (groups & 2)) {
        if (int lrc = make_tex_layout(mask2, s, n_cols2, E.area, E.side, t.L, why, cap, E.vmax))
            return lrc;
        t.n_roi = b->n_roi;
        t.px_offset = b->px_offset; t.x = b->x; t.y = b->y; t.inten = b->inten;
        t.bbox_w = b->bbox_w; t.bbox_h = b->bbox_h; t.min_inten = b->min_inten; t.max_inten = b->max_inten;
        t.out = d_out; t.ld = ld; t.status = ctx->d_status.as<int>();
        t.mask = mask2; t.n_cols = n_cols2; t.col0 = n_cols1;
        t.gap_after_glrlm = (mask & NYXHIP_FAM_GLDZM) ? kGldzmCols : 0;
        t.gap_after_glszm = ((mask & NYXHIP_FAM_GLDM) ? kGldmCols : 0) + ((mask & NYXHIP_FAM_NGLDM) ? kNgldmCols : 0);
        t.soft_nan = s->soft_nan; t.grey_depth = s->grey_depth; t.ibsi = s->ibsi;
    }
    if (mask4 && (groups & 8)) {
        if (int lrc = make_dep_layout(mask4, s, E.area, E.side, d.L, why, cap, E.vmax))
            return lrc;
        d.n_roi = b->n_roi;
        d.px_offset = b->px_offset; d.x = b->x; d.y = b->y; d.inten = b->inten;
        d.bbox_w = b->bbox_w; d.bbox_h = b->bbox_h; d.min_inten = b->min_inten; d.max_inten = b->max_inten;
        d.out = d_out; d.ld = ld; d.status = ctx->d_status.as<int>();
        d.mask = mask4;
        d.col_gldzm = c_gldzm; d.col_gldm = c_gldm; d.col_ngldm = c_ngldm;
        d.soft_nan = s->soft_nan; d.grey_depth = s->grey_depth; d.ibsi = s->ibsi;
    }
    if (mask3 && (groups & 4)) {
        if (int lrc = make_shape_layout(mask3, s, E.area, E.side, g.L, why, cap))
            return lrc;
        g.L.zern_px_cap = std::min<uint32_t>((E.px + 3u) & ~3u, 4096);   // <= 32 KiB of dynamic LDS in the Zernike kernel
        g.n_roi = b->n_roi;
        g.px_offset = b->px_offset; g.x = b->x; g.y = b->y; g.inten = b->inten;
        g.bbox_w = b->bbox_w; g.bbox_h = b->bbox_h; g.min_inten = b->min_inten; g.max_inten = b->max_inten;
        g.out = d_out; g.ld = ld; g.status = ctx->d_status.as<int>();
        g.mask = mask3;
        // (FRAC_AT_D sits before Gabor, MEAN_FRAC and RADIAL_CV between Gabor and Zernike: featureset.h:352-357)
        g.col_gabor = n_cols1 + n_cols2 + n_cols4 + ((mask & NYXHIP_FAM_RADIAL) ? kRadialBins : 0);
        g.col_zernike = g.col_gabor + ((mask3 & NYXHIP_FAM_GABOR) ? s->gabor_n_filters : 0) + ((mask & NYXHIP_FAM_RADIAL) ? 2 * kRadialBins : 0);
        g.soft_nan = s->soft_nan;
        g.small_rois = (E.px <= kClassPx[0] && E.side <= kClassSide[0]) ? 1 : 0;   // the smallest size class (a function of the ROI: roi_class)
        g.gabor_bank = ctx->d_bank.as<double>(); g.gabor_bank32 = ctx->d_bank32.as<float>(); g.gabor_bank16 = ctx->d_bank16.p; g.dbg_phase = (int)knob::dbg_phase(); g.gabor_nf = s->gabor_n_filters; g.gabor_n = s->gabor_kersize; g.gabor_thr = s->gabor_graythr;
        for (int f = 0; f <= NYXHIP_MAX_GABOR_FILTERS; f++) g.gabor_zero_rows[f] = ctx->bank_zero_rows[f];
        g.gabor_box_mask = ctx->bank_box_mask;
        g.gabor_lp_sep = ctx->bank_lp_sep && !knob::gabor_no_lpsep();
        memcpy(g.gabor_lp_B, ctx->bank_lp_B, sizeof(g.gabor_lp_B)); memcpy(g.gabor_lp_C, ctx->bank_lp_C, sizeof(g.gabor_lp_C));
    }
    return NYXHIP_OK;
}

// ---- size classes ------------------------------------------------------------------------------------------------------------
// The reference has no coupling between the ROIs of a batch: every worker thread takes ROIs of any size
// (the reference's src/nyx/parallel.h:23-42, roi_cache.h:31-84).  Here a launch carves its LDS for the largest ROI it holds, so
// a call is split into launches per SIZE CLASS: a classifier kernel sorts the ROI indices into five size classes x
// {16-bit tables possible, not possible} by each ROI's OWN pixel count, box and intensity range (never by its companions), and
// every class is launched over its index list with a carve-out -- hence kernel build and occupancy -- of its own.  Classes whose
// carve-out does not fit a CU's LDS run the same kernels with their scratch in a global workspace.
enum { H_COUNT = 0, H_OFFSET, H_PX, H_AREA, H_RANGE, H_SIDE, H_CURSOR, H_VMAX,
       H_SUMPX, H_SUMPX_HI, H_SUMAREA, H_SUMAREA_HI, H_SUMRANGE, H_SUMRANGE_HI, H_WORDS };   // header words per class (the three sums: 64 bits, even offsets)

// pass 1: members and extrema of every class (block-local in LDS first: ten hot words would serialise 5 n_roi global atomics)
// lvl_on: IBSI levels matter to the call (a texture family under IBSI): an ROI's largest intensity is its level count (roi_class)
__global__ void class_count_kernel(uint64_t n_roi, const uint64_t* px_offset, const uint32_t* bw, const uint32_t* bh, const uint32_t* mn,
                                   const uint32_t* mx, uint32_t* hdr, uint32_t lvl_on)
{
    __shared__ __attribute__((aligned(8))) uint32_t s_h[kClasses * H_WORDS];
    for (int i = threadIdx.x; i < kClasses * H_WORDS; i += blockDim.x) s_h[i] = 0;
    __syncthreads();
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n_roi) {
        const uint64_t n64 = px_offset[i + 1] - px_offset[i];
        const uint32_t n = n64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n64, w = bw[i], h = bh[i], r = mx[i] - mn[i];
        const uint64_t a64 = (uint64_t)w * h;
        uint32_t* c = s_h + roi_class(n, w, h, r, lvl_on ? mx[i] : 0u) * H_WORDS;
        atomicAdd(&c[H_COUNT], 1u);
        atomicAdd((unsigned long long*)&c[H_SUMPX], (unsigned long long)n);
        atomicAdd((unsigned long long*)&c[H_SUMAREA], (unsigned long long)a64);
        if (r < kLargeRangeMax) atomicAdd((unsigned long long*)&c[H_SUMRANGE], (unsigned long long)r + 1ull);
        atomicMax(&c[H_PX], n);
        atomicMax(&c[H_AREA], a64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)a64);
        atomicMax(&c[H_RANGE], r);
        atomicMax(&c[H_SIDE], w > h ? w : h);
        atomicMax(&c[H_VMAX], mx[i]);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kClasses * H_WORDS; k += blockDim.x) {
        const int f = k % H_WORDS;
        if (f == H_SUMPX || f == H_SUMAREA || f == H_SUMRANGE) {
            const unsigned long long v = *(const unsigned long long*)&s_h[k];
            if (v) atomicAdd((unsigned long long*)&hdr[k], v);
            continue;
        }
        if (s_h[k] == 0) continue;
        if (f == H_COUNT) atomicAdd(&hdr[k], s_h[k]);
        else if ((f >= H_PX && f <= H_SIDE) || f == H_VMAX) atomicMax(&hdr[k], s_h[k]);
    }
}

// pass 2: ROI indices grouped by class (class c occupies list[offset_c .. offset_c + count_c), offsets = prefix of the counts);
// blocks reserve their ranges in arrival order, so a class's list follows the batch order closely (neighbouring workgroups of a
// launch read neighbouring clouds) without being a function of it -- rows are addressed by ROI index, the order is free.
__global__ void class_scatter_kernel(uint64_t n_roi, const uint64_t* px_offset, const uint32_t* bw, const uint32_t* bh, const uint32_t* mn,
                                     const uint32_t* mx, uint32_t* hdr, uint32_t* list, uint32_t lvl_on)
{
    __shared__ uint32_t s_cnt[kClasses], s_base[kClasses];
    if (threadIdx.x < kClasses) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    int c = -1;
    uint32_t rank = 0;
    if (i < n_roi) {
        const uint64_t n64 = px_offset[i + 1] - px_offset[i];
        c = roi_class(n64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n64, bw[i], bh[i], mx[i] - mn[i], lvl_on ? mx[i] : 0u);
        rank = atomicAdd(&s_cnt[c], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kClasses) {
        uint32_t off = 0;
        for (int k = 0; k < (int)threadIdx.x; k++) off += hdr[k * H_WORDS + H_COUNT];
        if (blockIdx.x == 0) hdr[threadIdx.x * H_WORDS + H_OFFSET] = off;
        s_base[threadIdx.x] = off + (s_cnt[threadIdx.x] ? atomicAdd(&hdr[threadIdx.x * H_WORDS + H_CURSOR], s_cnt[threadIdx.x]) : 0u);
    }
    __syncthreads();
    if (c >= 0) list[s_base[c] + rank] = (uint32_t)i;
}

static void set_slots(SpillArgs& sp, const uint32_t* list, uint32_t n_slots)
{
    sp.roi_index = list; sp.n_slots = n_slots;
}

// The GLCM-only view of a launch's arguments: the GLCM block (ncol columns, col_glcm onwards) as a table of its own
static void glcm_view(RoiArgs& a, int ncol)
{
    a.out += a.col_glcm;
    a.mask = NYXHIP_FAM_GLCM; a.n_cols = ncol; a.col_glcm = 0; a.col_intensity = -1;
}

// Extrema every member of size class cls / 2 stays below (roi_class): what "does this class run from LDS?" is decided on, so that
// the answer is a function of the class -- i.e. of the ROI -- and the settings, never of the members a call happens to hold.
static Extrema class_bounds(int cls, const nyxhip_settings* s)
{
    const int sc = cls / 2;
    Extrema E{};
    E.px = kClassPx[sc]; E.side = kClassSide[sc]; E.area = kClassSide[sc] * kClassSide[sc];
    E.range = (cls & 1) ? (sc == 2 ? 65535u : 0xFFFFFFFFu) : 16383u;
    E.vmax = s->ibsi ? kLdsLevels : 0u;
    E.wide_only = (cls & 1) != 0;
    return E;
}

// INTENSITY + GLCM of one class by the several-workgroups-per-ROI kernels of roi_large.hip.  Members whose intensity range the
// histogram workspace does not hold (kLargeRangeMax) are left to the caller (the one-workgroup sort path).
static int run_large(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, const Extrema& E,
                     const ClassTotals& tot, const uint32_t* list, uint32_t count, bool* served)
{   // *served = false: the settings do not fit the path's kernels (nothing launched; the one-workgroup workspace path takes the class)
    *served = true;
    const uint32_t mask1 = mask & (NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM);
    if (!mask1 || !count) return NYXHIP_OK;
    hipStream_t st = ctx->stream();
    LargeArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = b->n_roi;
    a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.inten = b->inten;
    a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h; a.min_inten = b->min_inten; a.max_inten = b->max_inten;
    a.slide_min = b->slide_min; a.slide_max = b->slide_max;
    a.out = d_out; a.ld = ld; a.status = ctx->d_status.as<int>();
    const int outline_cols = nyxhip_n_columns(mask & kBehindIntensity, s);   // between the intensity block and GLCM (build_args)
    a.mask = mask1; a.n_cols = nyxhip_n_columns(mask1, s) + ((mask1 & NYXHIP_FAM_GLCM) ? outline_cols : 0);
    a.col_intensity = (mask1 & NYXHIP_FAM_INTENSITY) ? 0 : -1;
    a.col_glcm = (mask1 & NYXHIP_FAM_GLCM) ? ((mask1 & NYXHIP_FAM_INTENSITY) ? kIntensityCols : 0) + outline_cols : -1;
    a.soft_nan = s->soft_nan;
    a.grey_depth = s->grey_depth; a.ibsi = s->ibsi; a.glcm_grey_depth = s->glcm_grey_depth;
    a.glcm_offset = s->glcm_offset; a.glcm_na = s->glcm_n_angles; a.glcm_symmetric = s->glcm_symmetric;
    for (int i = 0; i < kMaxAngles; i++) a.glcm_angles[i] = s->glcm_angles[i];
    a.n_hist = abs(s->grey_depth);
    a.dbg = (uint32_t)knob::large_dbg();
    a.dense = ctx->dense_next.inten; a.dense_dt = (uint32_t)ctx->dense_next.dt;   // whole-slide mode: the members are dense images (launch_dense_slides)
    a.vec_ok = (((uintptr_t)b->inten & 15u) == 0 && ((uintptr_t)b->x & 7u) == 0 && ((uintptr_t)b->y & 7u) == 0) ? 1u : 0u;
    const bool do_int = mask1 & NYXHIP_FAM_INTENSITY, do_glcm = mask1 & NYXHIP_FAM_GLCM;
    const int greyInfo = s->ibsi ? 0 : s->grey_depth;
    const uint32_t ng_max = greyInfo != 0 ? (uint32_t)abs(greyInfo) : E.vmax;       // largest matrix order of the class
    const uint32_t lvl_cap = greyInfo < 0 ? (uint32_t)(-greyInfo) : 0u;
    const uint32_t na = (uint32_t)s->glcm_n_angles;
    a.plane16 = ng_max > 255 ? 1u : 0u;
    // load kernel: histogram counted in LDS with 16-bit counters (a slab holds < 65536 pixels); up to 16384 entries at 256 threads and
    // 8192 pixels per slab, up to 65536 entries (128 KiB) at 1024 threads and 32768 pixels per slab (16-bit data: the flush of the
    // table -- one atomic add per non-empty entry -- must not outweigh the slab's pixels)
    const uint32_t r_max = std::min(E.range, kLargeRangeMax - 1);
    // Slab size: 32 pixels per thread at 256 / 512 / 1024 threads.  Large slabs flush the table less often (the flush of a 12-bit
    // table is 16 KB of atomic traffic per slab -- at 8192 pixels a quarter of what the slab reads); small slabs fill the chip when
    // the class holds few pixels: as large as leaves ~2000 workgroups.
    a.px_per_wg = tot.px / 2048 >= 32768 ? 32768u : tot.px / 2048 >= 16384 ? 16384u : 8192u;
    if (!do_int) a.tab_lds = 0;
    else if (r_max < 16384u) a.tab_lds = (r_max + 1 + 63u) & ~63u;
    else { a.tab_lds = 65536; a.px_per_wg = 32768; }
    a.lds_P_bytes = do_glcm ? (uint32_t)std::min<uint64_t>(72 * 1024, ((4ull * na * (ng_max + 1ull) * (ng_max + 1ull) + 15) & ~15ull) + ((2ull * (lvl_cap + 2) + 15) & ~15ull)) : 0u;
    // ... plus the strip of plane rows with its halo rows: kLargeCells cells + 2 * offset rows of the class's widest plane
    a.lds_strip_bytes = do_glcm ? (uint32_t)std::min<uint64_t>(40 * 1024, (a.plane16 ? 2ull : 1ull) * (kLargeCells + 2ull * (uint64_t)std::max(s->glcm_offset, 0) * std::min<uint32_t>(E.side, kLargeCells)) + 64) : 0u;
    // finishing kernel: histogram bin bounds, then (over the same bytes) the GLCM feature scratch and the matrices themselves
    {
        // (an ROI keeps its scratch in LDS when it needs at most kLargeScratchLds -- its own matrix order decides, roi_large.hip)
        const uint64_t scr = do_glcm ? ((std::min<uint64_t>(large_glcm_scratch_bytes(ng_max), kLargeScratchLds) + 15) & ~15ull) : 0ull;
        const uint64_t pm = 4ull * na * ng_max * ng_max;
        a.fin_P_bytes = (do_glcm && pm <= 32 * 1024) ? (uint32_t)pm : 0u;
        a.fin_tab_bytes = do_int ? (uint32_t)((4ull * (std::min<uint32_t>(r_max, 8191u) + 1) + 15) & ~15ull) : 0u;   // up to 32 KiB of histogram
        // (the bin bounds of the n-bin histogram sit behind the table: with thousands of bins the table shrinks, beyond ~16000 the
        //  finishing kernel's 64 KiB cannot hold the bounds at all -- round-4 advisor)
        const uint64_t bounds = 4ull * (112 + (uint64_t)abs(s->grey_depth));
        if (do_int && bounds + 16 > 64 * 1024) { *served = false; return NYXHIP_OK; }
        if (do_int && a.fin_tab_bytes + bounds > 64 * 1024) a.fin_tab_bytes = (uint32_t)((64 * 1024 - bounds) & ~15ull);
        a.lds_fin_bytes = (uint32_t)std::max<uint64_t>(a.fin_tab_bytes + bounds, scr + a.fin_P_bytes + 16);
    }
    // ---- workspace: the members' blocks back to back (offsets handed out by the prep kernel) when the class fits the budget, else
    // chunks of the list with room for the class's largest block each
    const size_t budget = knob::large_budget((size_t)8 << 30);
    const LargeWs Lmax = large_ws_layout(r_max, E.area, ng_max, lvl_cap, na, a.plane16 != 0, do_int, do_glcm);
    const LargeWs Lfix = large_ws_layout(0, 0, ng_max, lvl_cap, na, a.plane16 != 0, do_int, do_glcm);   // what every block holds whatever its ROI
    const uint64_t all_bytes = (uint64_t)count * (Lfix.total + 1024) + (do_int ? 4ull * tot.range1 : 0ull) + (do_glcm ? (a.plane16 ? 2ull : 1ull) * tot.area : 0ull);
    uint32_t chunk = count;
    uint64_t ws_need = all_bytes;
    if (all_bytes > budget) {
        if (Lmax.total > budget) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "an ROI's workspace block (" + std::to_string(Lmax.total >> 20) + " MiB) exceeds the large-ROI budget");
        chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(count, budget / Lmax.total));
        ws_need = (uint64_t)chunk * Lmax.total;
    }
    const uint64_t slabs_max = ((uint64_t)E.px + 3 + a.px_per_wg - 1) / a.px_per_wg, strips_max = 2ull * E.area / kLargeCells + 1;
    uint64_t cap_load = chunk == count ? tot.px / a.px_per_wg + 2ull * count : (uint64_t)chunk * slabs_max;   // (a slab more per ROI: slabs start at a multiple of four pixels)
    uint64_t cap_cooc = do_glcm ? (chunk == count ? 2 * tot.area / kLargeCells + count : (uint64_t)chunk * strips_max) : 0;
    if (cap_load > 0x7FFFFFFFull || cap_cooc > 0x7FFFFFFFull) {          // (grid limit: smaller chunks)
        const uint64_t per = std::max(slabs_max, strips_max);
        chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, 0x7FFFFFFFull / per));
        cap_load = (uint64_t)chunk * slabs_max; cap_cooc = do_glcm ? (uint64_t)chunk * strips_max : 0;
        ws_need = std::min<uint64_t>(ws_need, (uint64_t)chunk * Lmax.total);
        if (slabs_max > 0x7FFFFFFFull || strips_max > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "ROI too large for the large-ROI launch grid");
    }
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_ctr = 0, o_off = 256, o_ml = al(o_off + 8ull * chunk), o_mc = al(o_ml + 8ull * cap_load), aux_need = al(o_mc + 8ull * cap_cooc);
    HIP_TRY(ctx, ctx->d_large.reserve(ws_need, st));
    HIP_TRY(ctx, ctx->d_large_aux.reserve(aux_need, st, aux_need + aux_need / 4));
    char* const aux = ctx->d_large_aux.as<char>();
    a.ws = ctx->d_large.as<unsigned char>(); a.ws_bytes = ws_need;
    a.ctr = (uint32_t*)(aux + o_ctr); a.ws_off = (uint64_t*)(aux + o_off);
    a.map_load = (uint2*)(aux + o_ml); a.map_cooc = (uint2*)(aux + o_mc);
    a.cap_load = (uint32_t)cap_load; a.cap_cooc = (uint32_t)cap_cooc;
    for (uint32_t o = 0; o < count; o += chunk) {
        a.list = list + o; a.n_list = std::min(chunk, count - o);
        HIP_TRY(ctx, hipMemsetAsync(a.ws, 0, ws_need, st));
        HIP_TRY(ctx, hipMemsetAsync(a.ctr, 0, 256, st));
        if (int rc = launch_large_features(a, st))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("large-ROI kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    return NYXHIP_OK;
}

// Gabor of the ROIs `list[0 .. grid)` by several workgroups per ROI (roi_large_gabor.hip): tiles of 64 x 32 output pixels staged in LDS,
// the reference's arithmetic per pixel, integer counts across workgroups.  Boxes beyond 8192 px a side (or kernels beyond 32 taps) are
// left to the caller's one-workgroup kernel (*served stays false).  `g`: the shape arguments of the class (columns, bank, threshold).
static int run_large_gabor(nyxhip_ctx* ctx, const nyxhip_batch* b, const nyxhip_settings* s, double* d_out, size_t ld, const Extrema& E, const ShapeArgs& g,
                           const uint32_t* list, uint32_t grid, hipStream_t st, DevBuf& buf, bool* served)
{
    *served = false;
    // (no_coop_gabor: A/B knob, read per call -- the tests compare both paths in one process)
    if (knob::no_coop_gabor() || !list || grid == 0 || E.side > kLgabMaxSide || (uint32_t)s->gabor_kersize > kLgabMaxN) return NYXHIP_OK;
    LgabArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.n_roi = b->n_roi; ga.px_offset = b->px_offset; ga.x = b->x; ga.y = b->y; ga.inten = b->inten;
    ga.bbox_w = b->bbox_w; ga.bbox_h = b->bbox_h; ga.min_inten = b->min_inten; ga.max_inten = b->max_inten;
    ga.out = d_out; ga.ld = ld; ga.col_gabor = g.col_gabor; ga.nf = s->gabor_n_filters; ga.n = s->gabor_kersize;
    ga.thr = g.gabor_thr; ga.soft_nan = s->soft_nan; ga.bank = g.gabor_bank;
    const uint64_t area_cap = std::max<uint64_t>(E.area, 1);
    // tiles of a w x h box: ceil(w / 64) ceil(h / 32) <= w h / 2048 + w / 64 + h / 32 + 1, and w, h <= side, w h <= area for every ROI of the class
    ga.tiles_cap = (uint32_t)std::min<uint64_t>((uint64_t)((E.side + kLgabTileW - 1) / kLgabTileW) * ((E.side + kLgabTileH - 1) / kLgabTileH),
                                                area_cap / (kLgabTileW * kLgabTileH) + E.side / kLgabTileW + E.side / kLgabTileH + 2);
    ga.off_rec = (4 * area_cap + 255) & ~255ull;
    ga.off_cnt = (ga.off_rec + 24ull * ga.tiles_cap + 255) & ~255ull;
    ga.stride = (ga.off_cnt + 4ull * (uint64_t)(ga.nf + 1) + 255) & ~255ull;
    const size_t gbudget = (size_t)2 << 30;
    const uint32_t gchunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<uint32_t>(grid, 65535u), gbudget / ga.stride));
    const size_t gneed = ga.stride * gchunk;
    HIP_TRY(ctx, buf.reserve(gneed, st));
    ga.ws = buf.as<unsigned char>();
    for (uint32_t o = 0; o < grid; o += gchunk) {
        const uint32_t nb = std::min(gchunk, grid - o);
        set_slots(ga.sp, list + o, nb);
        if (int rc = launch_large_gabor(ga, st, nb, E.px))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("large-ROI Gabor launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    *served = true;
    return NYXHIP_OK;
}

// GLRLM + GLSZM + NGTDM of one class by the several-workgroups-per-ROI kernels of roi_large_tex.hip, on stream `st` with the
// workspace pair `slot`.  *served: 0 = the class does not qualify (nothing launched), 1 = every member was served, 2 = the members
// outside ltex_eligible are left to the caller (the one-workgroup launch with SpillArgs::skip_ltex).
static int run_large_tex(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t full, const nyxhip_settings* s, double* d_out, size_t ld, const Extrema& E,
                         const ClassTotals& tot, const uint32_t* list, uint32_t count, hipStream_t st, int slot, int* served)
{
    *served = 0;
    const uint32_t mask2 = full & kTexture;
    if (!mask2 || !count) return NYXHIP_OK;
    const int greyInfo = s->ibsi ? 0 : s->grey_depth;
    const uint32_t ng = greyInfo != 0 ? (uint32_t)abs(greyInfo) : E.vmax;         // bound of the class's level counts
    if (ng == 0 || ng > kLtexLevels) return NYXHIP_OK;
    LtexArgs a;
    memset(&a, 0, sizeof(a));
    a.n_roi = b->n_roi;
    a.px_offset = b->px_offset; a.x = b->x; a.y = b->y; a.inten = b->inten;
    a.bbox_w = b->bbox_w; a.bbox_h = b->bbox_h; a.min_inten = b->min_inten; a.max_inten = b->max_inten;
    a.out = d_out; a.ld = ld; a.status = ctx->d_status.as<int>();
    a.mask = mask2; a.n_cols = nyxhip_n_columns(mask2, s);
    a.col0 = nyxhip_n_columns(full & (NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM | kBehindIntensity), s);
    a.gap_after_glrlm = (full & NYXHIP_FAM_GLDZM) ? kGldzmCols : 0;
    a.gap_after_glszm = ((full & NYXHIP_FAM_GLDM) ? kGldmCols : 0) + ((full & NYXHIP_FAM_NGLDM) ? kNgldmCols : 0);
    a.soft_nan = s->soft_nan; a.grey_depth = s->grey_depth; a.ibsi = s->ibsi;
    a.vec_ok = (((uintptr_t)b->inten & 15u) == 0 && ((uintptr_t)b->x & 7u) == 0 && ((uintptr_t)b->y & 7u) == 0) ? 1u : 0u;
    a.plane16 = ng > 255 ? 1u : 0u;
    a.px_per_wg = 8192;
    const uint64_t cb = a.plane16 ? 2 : 1;
    auto al16 = [](uint64_t v) { return (v + 15) & ~15ull; };
    auto al256 = [](uint64_t v) { return (v + 255) & ~255ull; };
    // ---- dynamic LDS at the bounds of what the path serves in this class (box sides of eligible members: <= kLtexMaxW wide)
    const uint64_t side_w = std::min<uint32_t>(E.side, kLtexMaxW);
    const uint32_t ng1 = ng + 1;
    const uint64_t ngt_rep = ng1 <= 16 ? 8 : ng1 <= 32 ? 4 : ng1 <= 64 ? 2 : 1, ngt_stride = (((ng1 + 2) * 12ull + 16 + 7) & ~7ull) | 8;
    const uint64_t cells = std::max<uint64_t>(kLtexCells, side_w) + 2 * side_w + 64;       // a strip's rows and its two halo rows, staged as they lie in the plane
    // (under IBSI a member's level count is its own largest intensity, anything up to the class's: every term below covers the
    //  smaller counts as well)
    uint64_t strip = al16(2ull * (ng + 2)) + al16(cb * cells);
    if (mask2 & NYXHIP_FAM_NGTDM) strip += ng1 <= 1024 ? std::max<uint64_t>(2048, al16(ngt_rep * ngt_stride)) : al16(12ull * 1026 + 32);
    // (replicated short-run tables, roi_large_tex.hip: ltex_rl_rep x ltex_rl_words -- at most 8 x 65 x 16 words, reached at 16 levels)
    const uint64_t rl_bytes = (mask2 & NYXHIP_FAM_GLRLM) ? al16(4ull * 8 * 65 * std::min<uint32_t>(std::max<uint32_t>(ng, 1), 16)) : 0;
    strip += rl_bytes;
    // sweep: two rows of owners, the chunk hand-overs, the ring of plane rows (rows of up to 1008 bytes: 1040-byte slots)
    const uint64_t sweep = (mask2 & NYXHIP_FAM_GLSZM) ? al16(8 * (side_w + 2) + 16 * (side_w / 64 + 4)) + 1040 * (8 + side_w / 64 + 2 + 5) : 0;
    // a wave per 64 columns of the class's widest box, and the wave that feeds the ring
    a.strip_threads = 64u * (uint32_t)(std::min<uint64_t>(15, std::max<uint64_t>(3, (std::min<uint64_t>(side_w, 1024) + 62) / 64 + 1)) + 1);
    a.lds_load_bytes = 32 * 1024;
    if (!(mask2 & NYXHIP_FAM_GLSZM)) a.strip_threads = 256;            // no sweep in the launch
    a.strip_groups = std::max<uint32_t>(1, a.strip_threads / 256);
    a.lds_group_bytes = (uint32_t)((strip + 64 + 15) & ~15ull);
    while (a.strip_groups > 1 && (uint64_t)a.strip_groups * a.lds_group_bytes > 144 * 1024) a.strip_groups--;
    const uint64_t lds_strip = std::max<uint64_t>((uint64_t)a.strip_groups * a.lds_group_bytes, sweep + 64);
    const uint64_t S = ng <= 256 ? kLtexSmall : 0;
    // (tables that exist only below a level count: under IBSI a member may have any count up to the class's, else all have ng)
    const bool any_ng = greyInfo == 0;
    const uint64_t small_b = (mask2 & NYXHIP_FAM_GLSZM) ? (any_ng ? 4ull * std::min<uint32_t>(ng, 256) * kLtexSmall : ng <= 256 ? 4ull * ng * kLtexSmall : 0) : 0;
    const uint64_t rl2_b = (mask2 & NYXHIP_FAM_GLRLM) ? (any_ng ? 4ull * 2 * 65 * std::min<uint32_t>(ng, 128) : ng <= 128 ? 4ull * 2 * 65 * ng : 0) : 0;   // two replicas of the run table
    const uint64_t lds_zone = al16(2ull * (ng + 2)) + al16(small_b) + al16(rl2_b) +
                              ((mask2 & NYXHIP_FAM_GLSZM) ? al16(2 * std::max<uint64_t>(kLtexCells, side_w) + 8) : 0) + 64;   // ... and the strip's 16-bit zone counters
    const uint64_t side_e = std::min<uint64_t>(std::max<uint32_t>(E.side, 1), (1u << 20) - 1);     // an eligible box has fewer than 2^20 cells
    const uint64_t slot_max = (uint64_t)ng * side_e + ng + side_e + 4;
    const uint64_t fin_fixed = al16(8ull * a.n_cols) + al16(2ull * (ng + 2)) + al16(4ull * (ng + 2)) + al16(16ull * (std::min<uint32_t>(ng, 256) + 2));
    const uint64_t fin_work = std::max<uint64_t>(16ull * (ng + 2), std::min<uint64_t>(16 * slot_max, 64 * 1024));
    const uint64_t lds_fin = fin_fixed + al16(fin_work) + 64;
    if (knob::debug()) fprintf(stderr, "[nyxhip] large texture: count %u ng %u side %u area %u lds strip %llu zone %llu fin %llu\n", count, ng, E.side, E.area,
                                        (unsigned long long)lds_strip, (unsigned long long)lds_zone, (unsigned long long)lds_fin);
    if (lds_strip > 144 * 1024 || lds_zone > 128 * 1024 || lds_fin > 144 * 1024) return NYXHIP_OK;
    a.lds_strip_bytes = (uint32_t)lds_strip; a.lds_zone_bytes = (uint32_t)lds_zone; a.lds_fin_bytes = (uint32_t)lds_fin;
    // ---- workspace: bounds of a member's block and of the class as a whole (ltex_ws_layout)
    const uint64_t area_e = std::min<uint64_t>(std::max<uint32_t>(E.area, 1), (1u << 20) - 1);
    const uint64_t rmin = std::max<uint64_t>(1, kLtexCells / std::max<uint64_t>(side_w, 1));
    const uint64_t fixed = 256 + al256(ng + 8) + al256(12ull * (ng + 2)) + al256(16 * slot_max) + al256(4ull * std::min<uint32_t>(ng, 256) * kLtexSmall) +
                           al256(8ull * szm_hash_cap(ng + 1, (uint32_t)area_e)) + 12 * 256;
    auto var_bytes = [&](uint64_t area, uint64_t members) {
        return cb * area + 64 * members + 8 * (area + 2 * members) + 4 * (area / (S + 1) + 8 * members) + 28 * (area / rmin + members * side_w) + 64 * members;
    };
    const size_t budget = knob::large_budget((size_t)2 << 30);   // per slot, kept until nyxhip_destroy (nine slots: 8 GiB each could pin 72 GiB of a context)
    const uint64_t all_bytes = (uint64_t)count * fixed + var_bytes(tot.area, count);
    const uint64_t one_max = fixed + var_bytes(area_e, 1);
    uint32_t chunk = count;
    uint64_t ws_need = all_bytes;
    if (all_bytes > budget) {
        if (one_max > budget) return NYXHIP_OK;              // (the one-workgroup path serves the class)
        chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(count, budget / one_max));
        ws_need = (uint64_t)chunk * one_max;
    }
    const uint64_t slabs_max = ((uint64_t)E.px + 3 + a.px_per_wg - 1) / a.px_per_wg, strips_max = area_e / 4096 + 2;
    uint64_t cap_load = chunk == count ? tot.px / a.px_per_wg + 2ull * count : (uint64_t)chunk * slabs_max;
    uint64_t cap_strip = chunk == count ? tot.area / 4096 + 2ull * count : (uint64_t)chunk * strips_max;
    if (cap_load > 0x3FFFFFFFull || cap_strip > 0x3FFFFFFFull) return NYXHIP_OK;
    // a device short of memory: smaller chunks (the form the budget already knows); when not even one member's block can be had the
    // class goes to the one-workgroup kernels (*served stays 0) instead of failing the call
    while (ctx->ltex_buf[slot].reserve(ws_need, st) != hipSuccess) {
        (void)hipGetLastError();
        if (chunk <= 1) return NYXHIP_OK;
        chunk = (chunk + 1) / 2;
        ws_need = (uint64_t)chunk * one_max;
        cap_load = (uint64_t)chunk * slabs_max; cap_strip = (uint64_t)chunk * strips_max;
    }
    const size_t o_ctr = 0, o_off = 256, o_ml = al256(o_off + 8ull * chunk), o_ms = al256(o_ml + 8ull * cap_load), aux_need = al256(o_ms + 8ull * cap_strip);
    HIP_TRY(ctx, ctx->ltex_aux[slot].reserve(aux_need, st, aux_need + aux_need / 4));
    char* const aux = ctx->ltex_aux[slot].as<char>();
    a.ws = ctx->ltex_buf[slot].as<unsigned char>(); a.ws_bytes = ws_need;
    a.ctr = (uint32_t*)(aux + o_ctr); a.ws_off = (uint64_t*)(aux + o_off);
    a.map_load = (uint2*)(aux + o_ml); a.map_strip = (uint2*)(aux + o_ms);
    a.cap_load = (uint32_t)cap_load; a.cap_strip = (uint32_t)cap_strip;
    for (uint32_t o = 0; o < count; o += chunk) {
        a.list = list + o; a.n_list = std::min(chunk, count - o);
        HIP_TRY(ctx, hipMemsetAsync(a.ws, 0, ws_need, st));
        HIP_TRY(ctx, hipMemsetAsync(a.ctr, 0, 256, st));
        if (int rc = launch_large_texture(a, st))
            return fail(ctx, NYXHIP_ERR_HIP, std::string("large-ROI texture kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    *served = (E.side <= kLtexMaxW && (uint64_t)E.area < (1ull << 20)) ? 1 : 2;
    if (knob::debug()) fprintf(stderr, "[nyxhip] large texture: served %d, workspace %llu MiB, chunk %u, caps %llu / %llu\n", *served, (unsigned long long)(ws_need >> 20), chunk,
                                        (unsigned long long)cap_load, (unsigned long long)cap_strip);
    return NYXHIP_OK;
}

// One launch group.
//   list != NULL: the members of one class (cls), `grid` of them (exact launches).  Which kernel groups of the class run from LDS is
//   decided on the class BOUNDS (class_bounds); the carve-outs then follow the class's extrema E.  A group that does not fit runs
//   from a global workspace: INTENSITY + GLCM by the several-workgroups-per-ROI path (run_large), the others with one workgroup
//   per ROI.
//   list == NULL: the whole batch (slot = ROI, grid = n_roi); class_mask != 0 then restricts the launch to the classes of the
//   mask (SpillArgs::class_mask: everybody else returns at once) -- used when the host launches without knowing the member
//   counts; such a launch cannot fall back to the workspace (its chunks are sized by member counts): *needs_host is set instead
//   and nothing is launched.  dry: build the argument blocks only (do the carve-outs fit?).
//   group_sel: kernel groups to launch (bit 0 features, 1 texture, 2 shape, 3 dependence).
int run_class(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld, const Extrema& E,
              const uint32_t* list, uint32_t grid, bool dry, bool* needs_host, ClassRun* report, uint32_t class_mask = 0, uint32_t group_sel = 0xF,
              int cls = -1, const ClassTotals* tot = nullptr)
{
    std::string why;
    const uint32_t full = mask;                          // column positions follow the call's full mask: build_args always gets it
    if (!(group_sel & 1)) mask &= ~(uint32_t)(NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM);
    if (!(group_sel & 2)) mask &= ~kTexture;
    if (!(group_sel & 4)) mask &= ~kShape;
    if (!(group_sel & 8)) mask &= ~kDependence;
    const uint32_t fam_of_group[4] = {NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM, kTexture, kShape, kDependence};
    uint32_t want = 0;                                   // kernel groups this call has work for
    for (int k = 0; k < 4; k++) if (mask & fam_of_group[k]) want |= 1u << k;
    if (!want) return NYXHIP_OK;
    RoiArgs a; TexArgs t; ShapeArgs g; DepArgs d;
    uint32_t gs = 0;                                     // groups that run from a global workspace
    if (list) {
        const Extrema Eb = class_bounds(cls, s);
        for (int k = 0; k < 4; k++) {
            if (!(want & (1u << k))) continue;
            if (cls / 2 >= kFirstLargeSizeClass) { gs |= 1u << k; continue; }
            const int lrc = build_args(ctx, b, full, s, d_out, ld, Eb, 0, a, t, g, d, why, 1u << k);
            if (lrc == NYXHIP_ERR_ROI_TOO_LARGE || lrc == NYXHIP_ERR_UNSUPPORTED) gs |= 1u << k;
            else if (lrc) return fail(ctx, lrc, why);
        }
    }
    uint32_t lds = want & ~gs;
    if (lds) {
        int lrc = build_args(ctx, b, full, s, d_out, ld, E, 0, a, t, g, d, why, lds);
        if (lrc == NYXHIP_ERR_UNSUPPORTED && (lds & 1) && list == nullptr) {
            // whole-batch launches: a GLCM grey depth whose matrix does not fit LDS next to any ROI sends the feature group to the workspace
            gs |= 1; lds &= ~1u;
            lrc = lds ? build_args(ctx, b, full, s, d_out, ld, E, 0, a, t, g, d, why, lds) : NYXHIP_OK;
        }
        if (lrc == NYXHIP_ERR_UNSUPPORTED || lrc == NYXHIP_ERR_ROI_TOO_LARGE) {
            if (list == nullptr && lrc == NYXHIP_ERR_UNSUPPORTED) return fail(ctx, lrc, why);
            gs |= lds; lds = 0;                          // (exact launches: cannot happen -- the bounds fitted; served from the workspace all the same)
        } else if (lrc) return fail(ctx, lrc, why);
    }
    if (gs && needs_host) { *needs_host = true; return NYXHIP_OK; }
    if (gs && !list) return fail(ctx, NYXHIP_ERR_ROI_TOO_LARGE, "ROI too large for the LDS-resident path: " + why);
    if (dry) return NYXHIP_OK;
    if (gs && ctx->win_next.inten && !b->inten)          // window-mode call (no clouds materialised): the caller builds them and comes back
        return NYXHIP_INTERNAL_NEEDS_CLOUDS;
    if (report) report->workspace = (int)gs;

    hipStream_t st = ctx->stream();
    int rc = 0;
    auto enter_lane = [&](int lane) -> int { return use_lane(ctx, lane, &st); };   // the class's launches go to lane `lane`, forked from the main stream at the start of the call
    // The launch groups of the LDS size classes are independent of each other and could each take a stream of their own (the tail of
    // one class's grid beside the next class's launches).  Measured on the mixed batch with the config-4 families: 3.51 ms against
    // 3.28 ms on one stream -- the chip is busy either way, and the interleaved classes evict each other's L2 lines.  Off unless asked
    // for (NYXHIP_LDS_LANES=1, A/B knob).
    const bool on_lds_lane = lds && !gs && knob::lds_lanes() && list && cls >= 0 && cls / 2 < kFirstLargeSizeClass && !ctx->win_next.inten;
    if (on_lds_lane)
        if (int lrc = enter_lane(4 + cls / 2)) return lrc;
    // Size class 2 (boxes up to 128 x 128, up to 16384 pixels) fits LDS, but its texture kernel is one workgroup walking 16 k cells through
    // a dozen passes and a serial zone sweep: ~0.3 ms per ROI whatever the batch, and a class of two thousand such ROIs is a round and
    // a tail of them (0.7-0.9 ms of the mixed batch's 3.3).  Its GLRLM / GLSZM / NGTDM go through the several-workgroups-per-ROI path
    // as well (roi_large_tex.hip), on a lane beside the main stream.  A function of the class, i.e. of the ROI.
    if (list && cls / 2 == 2 && (lds & 2) && tot && !knob::no_sc2_tex()) {   // A/B knob
        // (a function of the class alone: a window-mode chunk -- INTENSITY / GLCM only by construction, so never here with texture families --
        //  would come back with its clouds rather than take the other texture kernel)
        if (!b->inten) return NYXHIP_INTERNAL_NEEDS_CLOUDS;
        const hipStream_t main_st = st;
        int served2 = 0;
        // (the lane of size class 3 -- usually a handful of ROIs: streams beyond the device's four hardware queues share one, and a
        //  lane of its own landed on the queue of the largest class's lane, behind 2 ms of its kernels)
        const int lane2 = cls & 1;
        if (int lrc = enter_lane(lane2)) return lrc;
        if (int lrc = run_large_tex(ctx, b, full, s, d_out, ld, E, *tot, list, grid, st, lane2, &served2)) return lrc;
        if (served2 == 1) {
            lds &= ~2u;
            if (report) {
                report->cooperative |= 2;
                if (ctx->timing >= 2) { if (!report->e2) HIP_TRY(ctx, hipEventCreate(&report->e2)); HIP_TRY(ctx, hipEventRecord(report->e2, st)); }
            }
        }
        st = main_st;
    }
    // (Size class 2 and Gabor: a 128 x 128 box takes 87 KB of LDS in the tiled kernel -- one workgroup per CU, 10.9 ms for the 2 031 such
    //  ROIs of the heavy-tailed batch.  Cut into 64 x 32 tiles by run_large_gabor the same ROIs took 15.5 ms -- boxes of 65..127 px fill
    //  40 % of their tiles, and the strips compute every tap in fp64 where the tiled kernel screens on the matrix pipe: not routed there.)
    if (lds) {
        for (SpillArgs* sp : {&a.sp, &t.sp, &g.sp, &d.sp}) { set_slots(*sp, list, grid); sp->class_mask = list ? 0u : class_mask; }
        // the smallest size class (roi_class == 0) runs INTENSITY / GLCM a wave per ROI (roi_small.hip; launch_roi_features decides whether
        // the settings allow it): its exact list, a whole-batch launch filtered to it, or a whole batch that IS it by the stated extrema
        if (list ? cls == 0 : class_mask == 0x1u) a.small_class = 1;
        if (!list && class_mask == 0x1u) a.census = ctx->d_status.as<uint32_t>() + 1;
        else if (!list && class_mask == 0 && E.px <= kClassPx[0] && E.side <= kClassSide[0] && E.range < 16384u) a.small_class = 2;
        // the two filtered feature launches of a call on stated extrema (launch_device_all): ONE GLCM feature launch, behind the second
        if (!list && class_mask == 0x1u) a.glcm_feats = 1;
        else if (!list && class_mask == 0x3FEu) a.glcm_feats = 2;
        // INTENSITY + GLCM at the reference's default grey depth (17..64 levels): two launches instead of one.  The 16-bit-matrix
        // kernel holds 43 KB of LDS per workgroup (three per CU); the intensity block inside it ran at that occupancy, 2.9 ms per
        // 196 k ROIs against 1.4 ms for the intensity-only build at eight workgroups per CU.  Each launch zeroes and fills its own
        // block of columns.
        auto launch_features_main = [&]() -> int {
            const uint32_t both = NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM;
            if ((a.mask & both) == both && a.L.g16 && !knob::g16_fused()) {
                RoiArgs ai = a, ag = a;
                std::string w2;
                const int ncol_g = a.n_cols - a.col_glcm;              // (col_glcm: behind the intensity block and the outline columns)
                if (make_layout(NYXHIP_FAM_INTENSITY, s, kIntensityCols, E.px, E.area, E.range, ai.L, w2) == NYXHIP_OK &&
                    make_layout(NYXHIP_FAM_GLCM, s, ncol_g, E.px, E.area, E.range, ag.L, w2) == NYXHIP_OK && ag.L.g16) {
                    ai.mask = NYXHIP_FAM_INTENSITY; ai.n_cols = kIntensityCols; ai.col_intensity = 0; ai.col_glcm = -1;
                    glcm_view(ag, ncol_g);
                    ag.census = nullptr;                               // (the intensity launch counts)
                    if (int r1 = launch_roi_features(ag, st, grid)) return r1;
                    return launch_roi_features(ai, st, grid);
                }
            }
            return launch_roi_features(a, st, grid);
        };
        // Wide-range classes whose ranges fit 16 bits (16-bit microscopy data): the first-order features from a presence bitmap and a
        // duplicate list instead of a sort (roi_wide.hip), the GLCM columns from the GLCM-only build.  (The sort engine inside the
        // fused kernel cost 43 ns per 2821-pixel ROI against 12.5 ns on 12-bit data.)  A/B knob: no_wide.
        // Which engine serves a member is decided by ITS range (<= 0xFFFF: roi_wide + the GLCM-only build; beyond: the fused sort
        // kernel), never by the class's observed extrema: both launches run over the class and each skips the other's members.
        auto launch_features_wide = [&](bool& done) -> int {
            done = false;
            if (knob::no_wide() || !list || !(cls & 1) || !(a.mask & NYXHIP_FAM_INTENSITY)) return 0;
            WideArgs wa;
            memset(&wa, 0, sizeof(wa));
            if (!make_wide_layout(E.px, (uint32_t)abs(s->grey_depth), wa)) return 0;
            RoiArgs ag = a;
            const bool with_glcm = (a.mask & NYXHIP_FAM_GLCM) != 0;
            if (with_glcm) {
                std::string w2;
                const int ncol_g = a.n_cols - a.col_glcm;
                if (make_layout(NYXHIP_FAM_GLCM, s, ncol_g, E.px, E.area, std::min(E.range, 0xFFFFu), ag.L, w2, 0, E.vmax) != NYXHIP_OK) return 0;
                glcm_view(ag, ncol_g);
                if (a.glcm_ws && ag.L.ng_cap != a.L.ng_cap) return 0;          // (the count workspace was sized for the fused layout)
            }
            if (!b->inten) return NYXHIP_INTERNAL_NEEDS_CLOUDS;               // window-mode chunk: this kernel reads the clouds
            wa.px_offset = b->px_offset; wa.inten = b->inten; wa.min_inten = b->min_inten; wa.max_inten = b->max_inten;
            wa.slide_min = b->slide_min; wa.slide_max = b->slide_max;
            wa.out = a.out; wa.ld = a.ld; wa.status = a.status;
            wa.col_intensity = a.col_intensity; wa.n_hist = a.n_hist;
            wa.list = list; wa.n_list = grid;
            if (int r1 = launch_roi_wide(wa, st)) return r1;
            done = true;
            ag.sp.max_range = 0xFFFFu;
            if (with_glcm)
                if (int r2 = launch_roi_features(ag, st, grid)) return r2;
            if (E.range > 0xFFFFu) {                                          // members beyond 16 bits: the fused kernel, as if they were alone
                a.sp.min_range = 0x10000u;
                return launch_features_main();
            }
            return 0;
        };
        if (lds & 1) {
            bool wide_done = false;
            rc = launch_features_wide(wide_done);
            if (rc == NYXHIP_INTERNAL_NEEDS_CLOUDS) return rc;
            if (rc == 0 && !wide_done) rc = launch_features_main();
        }
        if (rc == 0 && (lds & 2)) rc = launch_roi_texture(t, st, grid);
        if (rc == 0 && (lds & 8)) rc = launch_roi_dependence(d, st, grid);
        if (rc == 0 && (lds & 4)) {
            // Size class 2 and Gabor: boxes of 65..128 px hold 87 KB of LDS in the tiled kernel -- one workgroup per CU, ~11 ms for the
            // 2 031 such ROIs of the heavy-tailed batch, with three quarters of every CU's wave slots idle.  On a lane of its own the
            // smaller classes' launches (and this class's other families) run beside it instead of behind it.
            hipStream_t gst = st;
            if (!knob::no_gabor_lane() && list && cls / 2 == 2 && (mask & NYXHIP_FAM_GABOR) && !on_lds_lane && !ctx->win_next.inten)
                if (int lrc = use_lane(ctx, nyxhip_ctx::kGaborLane, &gst)) return lrc;
            rc = launch_roi_shape(g, gst, grid);
        }
        if (rc != 0)
            return fail(ctx, NYXHIP_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    if (!gs) {
        if (on_lds_lane && report && ctx->timing >= 2) {
            if (!report->e2) HIP_TRY(ctx, hipEventCreate(&report->e2));      // (the size-class-2 texture branch may have made it already: that one is on its lane's stream)
            else return NYXHIP_OK;
            HIP_TRY(ctx, hipEventRecord(report->e2, st));
        }
        return NYXHIP_OK;
    }

    // ---- INTENSITY + GLCM of the class by several workgroups per ROI (every member whose intensity range the histogram holds) ------
    const bool no_coop = knob::no_coop();   // A/B knob: the one-workgroup path
    bool coop = false;
    if ((gs & 1) && tot && !no_coop) {
        if (int lrc = run_large(ctx, b, full, s, d_out, ld, E, *tot, list, grid, &coop)) return lrc;
        if (coop) {
            if (report) report->cooperative = 1;
            if (E.range < kLargeRangeMax) gs &= ~1u;     // nobody left for the sort path below
            if (!gs) return NYXHIP_OK;
        }
    }

    // the lane of this class (nyxhip_ctx::lane_stream): large classes only -- the workspace fallback of an LDS class stays on the main stream
    const int lane = (!knob::no_lanes() && cls / 2 >= kFirstLargeSizeClass) ? (cls - 2 * kFirstLargeSizeClass) % 4 : -1;
    if (lane >= 0)
        if (int lrc2 = enter_lane(lane)) return lrc2;
    auto lane_stamp = [&]() -> int {
        if (lane >= 0 && report && ctx->timing >= 2) {
            if (!report->e2) HIP_TRY(ctx, hipEventCreate(&report->e2));
            HIP_TRY(ctx, hipEventRecord(report->e2, st));
        }
        return NYXHIP_OK;
    };

    // ---- GLRLM + GLSZM + NGTDM of the class by several workgroups per ROI (roi_large_tex.hip) ---------------------------------------
    int tex_served = 0;
    if ((gs & 2) && tot && !no_coop && !knob::no_coop_tex() && cls / 2 >= kFirstLargeSizeClass) {
        if (int lrc = run_large_tex(ctx, b, full, s, d_out, ld, E, *tot, list, grid, st, lane >= 0 ? lane : nyxhip_ctx::kLanes, &tex_served)) return lrc;
        if (tex_served && report) report->cooperative |= 2;
        if (tex_served == 1) gs &= ~2u;
        if (!gs) return lane_stamp();
    }

    // ---- one workgroup per ROI over a global workspace: the groups of `gs` ------------------------------------------------------
    RoiArgs a2; TexArgs t2; ShapeArgs g2; DepArgs d2;
    int lrc = build_args(ctx, b, full, s, d_out, ld, E, (size_t)1 << 31, a2, t2, g2, d2, why, gs);
    if (lrc) return fail(ctx, lrc, "large-ROI workspace: " + why);
    // ---- Gabor of the class by several workgroups per ROI (roi_large_gabor.hip) --------------------------------------------------------
    bool gabor_served = false;
    if ((gs & 4) && (mask & NYXHIP_FAM_GABOR) && !no_coop) {
        if (int grc = run_large_gabor(ctx, b, s, d_out, ld, E, g2, list, grid, st, lane >= 0 ? ctx->lane_buf[lane] : ctx->d_spill, &gabor_served)) return grc;
        if (gabor_served && report) report->cooperative |= 4;
    }
    if (coop) a2.sp.min_range = kLargeRangeMax;          // the histogram path served everybody below
    if (tex_served == 2) t2.sp.skip_ltex = 1;            // ... and the strip path every box it takes
    size_t stride = 0;
    if (gs & 1) stride = std::max<size_t>(stride, a2.L.total);
    if (gs & 2) stride = std::max<size_t>(stride, t2.L.total);
    if ((gs & 4) && (mask & NYXHIP_FAM_GABOR) && !gabor_served) stride = std::max<size_t>(stride, g2.L.total);
    if (gs & 8) stride = std::max<size_t>(stride, d2.L.total);
    stride = (stride + 255) & ~(size_t)255;
    const size_t budget = (size_t)4 << 30;         // at most 4 GiB of scratch in flight
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(grid, budget / std::max<size_t>(stride, 1)));
    const size_t need = stride * chunk;
    DevBuf& buf = lane >= 0 ? ctx->lane_buf[lane] : ctx->d_spill;
    HIP_TRY(ctx, buf.reserve(need, st));
    if ((gs & 4) && (mask & NYXHIP_FAM_ZERNIKE)) {   // Zernike keeps no ROI-sized state in LDS: one launch over the class, whatever its size
        ShapeArgs gz = g2;
        gz.mask = NYXHIP_FAM_ZERNIKE; gz.sp.scratch = nullptr; gz.small_rois = 0;
        set_slots(gz.sp, list, grid);
        rc = launch_roi_shape(gz, st, grid);
        if (rc != 0) return fail(ctx, NYXHIP_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    // The dependence trio of a large class (one workgroup per ROI over the workspace: a few hundred workgroups, ~11 ms for the heavy-tailed
    // batch) on a lane and a scratch buffer of its own: it runs beside the class's other chains instead of behind them.
    if ((gs & 8) && lane >= 0 && !knob::no_dep_lane() && gs != 8u) {
        hipStream_t dst = st;
        if (int lrc2 = use_lane(ctx, nyxhip_ctx::kDepLane, &dst)) return lrc2;
        const size_t dstride = (d2.L.total + 255) & ~(size_t)255;
        const uint32_t dchunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(grid, budget / std::max<size_t>(dstride, 1)));
        DevBuf& dbuf = ctx->lane_buf[nyxhip_ctx::kDepLane];
        HIP_TRY(ctx, dbuf.reserve(dstride * dchunk, dst));
        for (uint32_t o = 0; o < grid; o += dchunk) {
            const uint32_t nb = std::min(dchunk, grid - o);
            set_slots(d2.sp, list + o, nb);
            d2.sp.scratch = dbuf.as<unsigned char>(); d2.sp.stride = dstride;
            if (int drc = launch_roi_dependence(d2, dst, nb))
                return fail(ctx, NYXHIP_ERR_HIP, std::string("large-ROI kernel launch failed: ") + hipGetErrorString((hipError_t)drc));
        }
        gs &= ~8u;
    }
    for (uint32_t o = 0; o < grid; o += chunk) {
        const uint32_t nb = std::min(chunk, grid - o);
        set_slots(a2.sp, list + o, nb); set_slots(t2.sp, list + o, nb); set_slots(g2.sp, list + o, nb); set_slots(d2.sp, list + o, nb);
        a2.sp.scratch = t2.sp.scratch = g2.sp.scratch = d2.sp.scratch = buf.as<unsigned char>();
        a2.sp.stride = t2.sp.stride = g2.sp.stride = d2.sp.stride = stride;
        rc = (gs & 1) ? launch_roi_features(a2, st, nb) : 0;
        if (rc == 0 && (gs & 2)) rc = launch_roi_texture(t2, st, nb);
        if (rc == 0 && (gs & 8)) rc = launch_roi_dependence(d2, st, nb);
        if (rc == 0 && (gs & 4) && (mask & NYXHIP_FAM_GABOR) && !gabor_served) rc = launch_roi_shape(g2, st, nb);
        if (rc != 0)
            return fail(ctx, NYXHIP_ERR_HIP, std::string("large-ROI kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    return lane_stamp();
}

// Launch on device-resident arrays.
//   hinted: the extrema are the caller's statement about the batch (or exact, computed by the caller of this function).  When
//   they rule out everything but the two smallest size classes, nothing has to be counted: the kernel builds of those classes
//   differ only in whether the 16-bit tables apply (feature kernels) and in the one-wave shape kernels of the smallest class, so
//   the call enqueues whole-batch launches -- filtered by class where the build follows the class -- and returns without a
//   host round trip (the metric configuration: a stream of back-to-back calls stays back to back).  Otherwise the classifier
//   runs, its class headers come to the host once (two small kernels + one 320-byte copy), and every class gets an exact
//   grid and a carve-out of its own extrema.  Either way the kernel build an ROI runs through follows from ITS class and the
//   settings, not from its companions.
int launch_device_all(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out,
                      size_t ld, uint32_t max_px, uint32_t max_area, uint32_t max_range, uint32_t max_side, bool hinted)
{
    if (mask & NYXHIP_FAM_GABOR)
        if (int brc = ensure_gabor_bank(ctx, s))
            return brc;
    hipStream_t st = ctx->stream();
    const uint32_t n_roi = (uint32_t)b->n_roi;
    clear_runs(ctx);
    // workspace lanes (run_class): forked from here, joined into the main stream on every way out
    if (!ctx->lane_fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->lane_fork, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(ctx->lane_fork, st));
    struct LaneJoin {
        nyxhip_ctx* c; hipStream_t st;
        void join() {
            for (int k = 0; k < nyxhip_ctx::kLanes; k++)
                if (c->lane_used[k]) {
                    (void)hipEventRecord(c->lane_done[k], c->lane_stream[k]);
                    (void)hipStreamWaitEvent(st, c->lane_done[k], 0);
                    c->lane_used[k] = false;
                }
        }
        ~LaneJoin() { join(); }
    } lane_join{ctx, st};
    ctx->glcm_ng = ctx->close_flag = nullptr;
    if (mask & (NYXHIP_FAM_GLCM | NYXHIP_FAM_INTENSITY)) {
        // Matrix orders of the split GLCM launches (RoiArgs::glcm_ng; not part of the count workspace, which may be re-allocated between
        // the launch groups of a call) and pending flags of the deferred intensity closing (RoiArgs::close_flag), side by side in one
        // allocation: a call that asks for both clears both with one fill.
        //   order 0 = "nothing to derive": an ROI whose feature kernel returns before it states its matrix order (error paths) must not
        //   leave glcm_features_kernel a stale order from an earlier call;
        //   intensity_close_kernel clears the flags it consumes; the clearing here covers a call that ended between a feature launch
        //   and its closing launch.
        const bool want_ng = (mask & NYXHIP_FAM_GLCM) != 0, want_flag = (mask & NYXHIP_FAM_INTENSITY) != 0;
        const size_t table = (4ull * n_roi + 255) & ~(size_t)255;            // the second table's offset
        const size_t need = 2 * table + 256;
        HIP_TRY(ctx, ctx->d_roi_words.reserve(need, st, need + need / 4));
        uint32_t* const base = ctx->d_roi_words.as<uint32_t>();
        if (want_ng) ctx->glcm_ng = base;
        if (want_flag) ctx->close_flag = base + table / 4;
        if (want_ng && want_flag) HIP_TRY(ctx, hipMemsetAsync(base, 0, table + 4ull * n_roi, st));
        else HIP_TRY(ctx, hipMemsetAsync(want_ng ? ctx->glcm_ng : ctx->close_flag, 0, 4ull * n_roi, st));
    }
    if (mask & NYXHIP_FAM_INTENSITY) {
        // records of the deferred intensity closing (RoiArgs::close_rec)
        const size_t need_rec = 8ull * kCloseRec * n_roi + 256;
        HIP_TRY(ctx, ctx->d_close_rec.reserve(need_rec, st, need_rec + need_rec / 4));
    }
    auto timed_class = [&](int cls, uint32_t count, const Extrema& E, const uint32_t* lp, uint32_t grid, uint32_t class_mask = 0, uint32_t group_sel = 0xF,
                           const ClassTotals* tot = nullptr) -> int {
        ClassRun r{cls, count, E, 0, nullptr, nullptr};
        if (ctx->timing >= 2) {
            HIP_TRY(ctx, hipEventCreate(&r.e0));
            HIP_TRY(ctx, hipEventCreate(&r.e1));
            HIP_TRY(ctx, hipEventRecord(r.e0, st));
        }
        const int rc = run_class(ctx, b, mask, s, d_out, ld, E, lp, grid, false, nullptr, &r, class_mask, group_sel, cls, tot);
        if (ctx->timing >= 2 && rc == 0) HIP_TRY(ctx, hipEventRecord(r.e1, st));
        ctx->runs.push_back(r);
        return rc;
    };
    if ((mask & ~kTailFams) || !hinted) {               // (a batch without stated extrema gets them from the class headers)
        bool done = false;
        // (IBSI co-occurrence matrices are as large as the largest intensity, which a statement about the batch does not carry)
        const bool need_vmax = s->ibsi && (mask & (NYXHIP_FAM_GLCM | kTexture | kDependence));
        // (a stated range that allows wide-range ROIs takes the exact path as well: a whole-batch launch per table width would
        //  carve 43 KB for a class that 16-bit data leaves empty -- 100 k workgroups that only return, three per CU)
        const bool wide_possible = max_range >= 16384u && (mask & NYXHIP_FAM_INTENSITY);
        const bool has_m1 = !(max_px <= kClassPx[0] && max_side <= kClassSide[0]);
        const bool small_fits = !knob::no_small() && ((mask & NYXHIP_FAM_INTENSITY) || (!s->ibsi && s->grey_depth > 0 && s->grey_depth <= 64));
        const bool two_filtered = (mask & (NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM)) && has_m1 && small_fits;
        // (the recent calls held the smallest class in numbers: exact lists beat two launches that each skip the other's slots)
        const bool prefer_lists = two_filtered && !knob::no_adapt() && ctx->census_total != 0 && 4 * ctx->census_small >= ctx->census_total;
        if (hinted && !knob::class_sync() && !need_vmax && !wide_possible && !prefer_lists && max_px <= kClassPx[1] && max_side <= kClassSide[1]) {
            // ---- whole-batch launches, nothing counted -----------------------------------------------------------------------
            if (two_filtered) ctx->census_pending += n_roi;
            const Extrema Eall{max_px, max_area, max_range, max_side};
            struct Group { int cls; Extrema E; uint32_t class_mask, group_sel; };
            std::vector<Group> groups;
            // texture / dependence kernels: one build for both classes
            if (mask & (kTexture | kDependence)) groups.push_back({-1, Eall, 0u, 2u | 8u});
            // feature kernels: one launch, no filter (both size classes run the same build; a contradicting ROI raises the error flag
            // in the kernel)
            // ... except that the smallest size class has a kernel of its own (a wave per ROI, roi_small.hip) for INTENSITY and for
            // GLCM under matlab binning with <= 64 levels: then two launches, each filtered to its classes
            if (two_filtered) {
                const uint32_t sd0 = std::min(max_side, kClassSide[0]);
                groups.push_back({-2, Extrema{std::min(max_px, kClassPx[0]), std::min(max_area, sd0 * sd0), max_range, sd0}, 0x1u, 1u});
                groups.push_back({-3, Eall, 0x3FEu, 1u});
            } else
            if (mask & (NYXHIP_FAM_INTENSITY | NYXHIP_FAM_GLCM)) groups.push_back({-2, Eall, 0u, 1u});
            // shape kernels: one-wave builds for the smallest size class, four-wave builds for the other
            if (mask & kShape) {
                const uint32_t sd0 = std::min(max_side, kClassSide[0]);
                if (!has_m1) groups.push_back({-4, Eall, 0u, 4u});
                else {
                    groups.push_back({-4, Extrema{std::min(max_px, kClassPx[0]), std::min(max_area, sd0 * sd0), max_range, sd0}, 0x3u, 4u});
                    groups.push_back({-5, Eall, 0x3FCu, 4u});   // (every other class: an ROI beyond the stated extrema meets the kernel's cap check and raises the error flag)
                }
            }
            bool needs_host = false;
            for (const Group& g : groups)
                if (int rc = run_class(ctx, b, mask, s, d_out, ld, g.E, nullptr, n_roi, true, &needs_host, nullptr, g.class_mask, g.group_sel)) return rc;
            if (!needs_host) {                             // (else: the exact path, whose workspace chunks need member counts)
                for (const Group& g : groups)
                    if (int rc = timed_class(g.cls, n_roi, g.E, nullptr, n_roi, g.class_mask, g.group_sel)) return rc;
                done = true;
            }
        }
        if (!done) {
            // ---- classify, class headers to the host, one exact launch group per class ------------------------------------------
            const size_t list_bytes = 4ull * n_roi + 256;
            HIP_TRY(ctx, ctx->d_cls_list.reserve(list_bytes, st, list_bytes + list_bytes / 4));
            HIP_TRY(ctx, ctx->d_cls_hdr.reserve(sizeof(uint32_t) * kClasses * H_WORDS, nullptr));
            HIP_TRY(ctx, ctx->h_cls_hdr.ensure(sizeof(uint32_t) * kClasses * H_WORDS));
            uint32_t* const hdr = ctx->d_cls_hdr.as<uint32_t>();
            uint32_t* const list = ctx->d_cls_list.as<uint32_t>();
            HIP_TRY(ctx, hipMemsetAsync(hdr, 0, sizeof(uint32_t) * kClasses * H_WORDS, st));
            const unsigned blocks = (unsigned)((b->n_roi + 255) / 256);
            const uint32_t lvl_on = need_vmax ? 1u : 0u;
            hipLaunchKernelGGL(class_count_kernel, dim3(blocks), dim3(256), 0, st, b->n_roi, b->px_offset, b->bbox_w, b->bbox_h, b->min_inten, b->max_inten, hdr, lvl_on);
            hipLaunchKernelGGL(class_scatter_kernel, dim3(blocks), dim3(256), 0, st, b->n_roi, b->px_offset, b->bbox_w, b->bbox_h, b->min_inten, b->max_inten, hdr, list, lvl_on);
            if (hipError_t e = hipGetLastError(); e != hipSuccess)
                return fail(ctx, NYXHIP_ERR_HIP, std::string("classifier launch failed: ") + hipGetErrorString(e));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cls_hdr.p, hdr, sizeof(uint32_t) * kClasses * H_WORDS, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            const uint32_t* H = (const uint32_t*)ctx->h_cls_hdr.p;
            if (!ctx->census_pending) { ctx->census_small = H[H_COUNT]; ctx->census_total = n_roi; }   // (class 0 = the smallest size class, 16-bit tables)
            if (!hinted) {
                max_px = max_area = max_range = max_side = 0;
                for (int cls = 0; cls < kClasses; cls++) {
                    const uint32_t* h = H + cls * H_WORDS;
                    max_px = std::max(max_px, h[H_PX]); max_area = std::max(max_area, h[H_AREA]);
                    max_range = std::max(max_range, h[H_RANGE]); max_side = std::max(max_side, h[H_SIDE]);
                }
            }
            // The size classes beyond LDS (3 and 4, either table width) go through the same several-workgroups-per-ROI kernels, which cut
            // every ROI by its own box: they run as ONE launch group (their lists are neighbours in the class order) -- four groups of
            // a handful of ROIs each cost four times the ten-odd launches and workspace clears of a group (~0.1 ms apiece on the mixed
            // batch).  Nothing an ROI's row depends on changes: the slab / strip cut is invisible by construction.
            // A window-mode chunk (no clouds materialised) with a class that reads clouds -- the classes beyond LDS, and the wide-range
            // classes the bitmap kernel serves -- goes back for them BEFORE anything is launched: raised from inside the class loop it
            // made the caller run the whole chunk again, every LDS class computed twice (16-bit tiles: on every chunk).
            if (ctx->win_next.inten && !b->inten && (mask & ~kTailFams)) {
                for (int cls = 0; cls < kClasses; cls++) {
                    if (H[cls * H_WORDS + H_COUNT] == 0) continue;
                    if (cls / 2 >= kFirstLargeSizeClass || ((cls & 1) && (mask & NYXHIP_FAM_INTENSITY) && !knob::no_wide()))
                        return NYXHIP_INTERNAL_NEEDS_CLOUDS;
                }
            }
            int first_cls = kClasses - 1;
            if (!knob::no_merge_large() && (mask & ~kTailFams)) {
                uint32_t cnt = 0; int top = -1;
                Extrema Em{0, 0, 0, 0, 0, false};
                ClassTotals tm{0, 0, 0};
                for (int cls = 2 * kFirstLargeSizeClass; cls < kClasses; cls++) {
                    const uint32_t* h = H + cls * H_WORDS;
                    if (h[H_COUNT] == 0) continue;
                    cnt += h[H_COUNT]; top = cls;
                    Em.px = std::max(Em.px, h[H_PX]); Em.area = std::max(Em.area, h[H_AREA]); Em.range = std::max(Em.range, h[H_RANGE]);
                    Em.side = std::max(Em.side, h[H_SIDE]); Em.vmax = std::max(Em.vmax, h[H_VMAX]);
                    tm.px += ((uint64_t)h[H_SUMPX_HI] << 32) | h[H_SUMPX]; tm.area += ((uint64_t)h[H_SUMAREA_HI] << 32) | h[H_SUMAREA];
                    tm.range1 += ((uint64_t)h[H_SUMRANGE_HI] << 32) | h[H_SUMRANGE];
                }
                if (top >= 0)
                    if (int rc = timed_class(top, cnt, Em, list + H[2 * kFirstLargeSizeClass * H_WORDS + H_OFFSET], cnt, 0, 0xF, &tm))
                        return rc;
                first_cls = 2 * kFirstLargeSizeClass - 1;
            }
            for (int cls = first_cls; cls >= 0 && (mask & ~kTailFams); cls--) {   // largest ROIs first: their long workgroups start early
                const uint32_t* h = H + cls * H_WORDS;
                if (h[H_COUNT] == 0) continue;
                const Extrema E{h[H_PX], h[H_AREA], h[H_RANGE], h[H_SIDE], h[H_VMAX], (cls & 1) != 0 && cls / 2 < kSizeClasses - 1};
                const ClassTotals tot{((uint64_t)h[H_SUMPX_HI] << 32) | h[H_SUMPX], ((uint64_t)h[H_SUMAREA_HI] << 32) | h[H_SUMAREA],
                                      ((uint64_t)h[H_SUMRANGE_HI] << 32) | h[H_SUMRANGE]};
                if (int rc = timed_class(cls, h[H_COUNT], E, list + h[H_OFFSET], h[H_COUNT], 0, 0xF, &tot))
                    return rc;
            }
        }
    }
    if (mask & kTailFams) {
        // A feature launch with GLCM zeroes and fills its columns from column 0, across the outline columns: the outline kernel goes
        // behind every feature launch of the call -- the lanes join here and the contour chain stays on the call's stream.
        const bool after_all = (mask & kBehindIntensity) && (mask & NYXHIP_FAM_GLCM);
        if (after_all) lane_join.join();
        if (int mrc = launch_contour_families(ctx, b, mask, s, d_out, ld, max_px, max_area, max_side, !after_all))
            return mrc;
    }
    return NYXHIP_OK;
}

} // namespace

// ---- what the other host units call (declared in nyxhip_ctx.h) ----
namespace nyxhip {

// A workspace lane: a high-priority stream forked from the call's stream (nyxhip_ctx::lane_fork, recorded at the start of launch_device_all),
// joined into it at the end of the call (LaneJoin).  The lanes carry chains of short, latency-bound kernels -- a few hundred workgroups each --
// beside the main stream's chip-filling grids: at the device's highest priority their workgroups are placed first and the chain is not starved.
int use_lane(nyxhip_ctx* ctx, int lane, hipStream_t* st)
{
    if (!ctx->lane_stream[lane]) {
        int lo = 0, hi = 0;
        if (knob::no_lane_priority() || hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
        HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->lane_stream[lane], hipStreamNonBlocking, hi));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->lane_done[lane], hipEventDisableTiming));
    }
    if (!ctx->lane_used[lane]) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->lane_stream[lane], ctx->lane_fork, 0));   // the batch and the class lists are complete on the main stream
        ctx->lane_used[lane] = true;
    }
    *st = ctx->lane_stream[lane];
    return NYXHIP_OK;
}


uint32_t pow2ceil(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Carves the workgroup's LDS for one launch.  Returns NYXHIP_OK, or
// NYXHIP_ERR_UNSUPPORTED when the grey depth alone cannot be held in LDS, or
// NYXHIP_ERR_ROI_TOO_LARGE when the batch extrema do not fit the 160 KiB of a CU.
int make_layout(uint32_t mask, const nyxhip_settings* s, int n_cols, uint32_t max_px, uint32_t max_area,
                uint32_t max_range, LdsLayout& L, std::string& why, size_t cap, uint32_t vmax, bool wide_only)
{
    memset(&L, 0, sizeof(L));
    const bool do_int = mask & NYXHIP_FAM_INTENSITY, do_glcm = mask & NYXHIP_FAM_GLCM;
    const bool spill = cap != 0;               // scratch in the global workspace: only the 2 GiB offset range limits it
    if (!spill) cap = roi_features_max_lds();
    uint32_t off = 0;
    L.out = off;                               // (the kernel writes its output row in place: no staging copy)
    L.red = off; off = align16(off + 8u * kWaves * 8);
    L.stat = off; off = align16(off + 8u * 16);
    uint32_t n_hist = (uint32_t)abs(s->grey_depth);
    L.lbc = off; off = align16(off + 4u * (do_int ? n_hist + 8 : 8));
    const uint32_t fixed = off;               // everything that does not scale with the ROI
    // order-statistics engine (roi_features.hip): a counting table over [min, max] when the
    // batch's largest intensity range fits kCountCapMax entries -- then no ROI sorts and the
    // value buffer needs no power-of-two padding; otherwise ROIs with a small range still
    // count (table of kCountCapMixed) and the rest bitonic-sort a padded buffer.
    const uint32_t kCountCapMax = spill ? (1u << 22) : 16384u, kCountCapMixed = 4096;
    const bool radix = do_int && wide_only && !spill;   // every ROI sorts: LSD radix sort (roi_features.hip: radix_sort), no table, no padding
    if (radix) {
        L.count_cap = 0;
        L.sort_cap = max_px ? max_px : 1;
    } else if (do_int) {
        if ((uint64_t)max_range + 1 <= kCountCapMax) {
            L.count_cap = (max_range + 1 + 63u) & ~63u;
            L.sort_cap = max_px ? max_px : 1;
        } else {
            L.count_cap = kCountCapMixed;
            L.sort_cap = pow2ceil(max_px ? max_px : 1);
        }
    }
    // [val | cnt] is dead once the intensity block has finished, so the GLCM matrices and
    // their scratch alias the same bytes (the kernel separates the two uses by barriers);
    // the dense plane is written during the load phase and stays separate.
    L.dense_cap = do_glcm ? max_area : 0;
    L.dense = off;
    {   // 8-bit plane: matlab binning up to 16 levels in a launch that also gets the 16-bit tables and the split GLCM features
        // (build_args sets the split up under the same conditions) -- the carve-out of the benchmark ROI then fits 8 times per CU
        const int gi = s->ibsi ? 0 : s->grey_depth;
        const bool c16_pred = do_int && max_px < 65536u && (uint64_t)max_range + 1 <= kCountCapMax && max_range < 65536u;
        const bool split_pred = do_glcm && !spill && gi > 0 && gi <= 16 && s->glcm_n_angles > 0;
        L.dense8 = ((c16_pred || !do_int) && split_pred) ? 1u : 0u;           // (GLCM alone: nothing of the intensity block constrains the plane)
    }
    {   // the reference's default grey depth on LDS launches: 16-bit matrices + 8-bit plane (the TIER 9 builds of roi_features_kernel)
        const int gi = s->ibsi ? 0 : s->grey_depth;
        const bool c16_pred = (!do_int || (uint64_t)max_range + 1 <= kCountCapMax) && max_range < 65536u;
        L.g16 = (do_glcm && !spill && gi > 16 && gi <= 64 && max_px < 32768u && c16_pred && s->glcm_n_angles > 0) ? 1u : 0u;
        if (L.g16) L.dense8 = 1;
    }
    if ((L.dense8 ? 1ull : 2ull) * L.dense_cap > cap) { why = "ROI bounding box of " + std::to_string(max_area) + " px exceeds the LDS-resident plane"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    // (8-bit planes: + a zero row of 64 bytes + the out-of-box cell.  Grey-depth-64 launches: the plane is dead once the co-occurrence
    //  sweep is through, and the feature pass's scratch -- features, sums, row marginals: 4.6 KB -- takes its place: the carve-out
    //  of the benchmark ROI drops from 43.1 to 39.3 KB, four workgroups per CU instead of three)
    uint32_t plane_bytes = L.dense8 ? 1u * L.dense_cap + 64 + 8 : 2u * L.dense_cap + 8;
    const uint32_t g16_scratch = L.g16 ? 8u * ((uint32_t)s->grey_depth + kMaxAngles * 128u) : 0u;          // level values | a 1 KiB block per angle-wave (glcm_features_wave64_v2)
    if (plane_bytes < g16_scratch) plane_bytes = g16_scratch;
    off = align16(off + plane_bytes);
    if (do_glcm) {
        const int greyInfo = s->ibsi ? 0 : s->grey_depth;
        L.lvl_cap = greyInfo < 0 ? (uint32_t)(-greyInfo) : 0;
        L.lvlmap = off; off = align16(off + 2u * (L.lvl_cap + 8));
    }
    const uint32_t shared0 = off;
    L.val = off;
    // 16-bit tables: every ROI of the launch counts (range below the table) and has fewer than 65536 pixels, so counts,
    // per-wave prefix sums and the values' offsets from the ROI minimum all fit 16 bits
    L.cnt16 = (do_int && max_px < 65536u && (uint64_t)max_range + 1 <= kCountCapMax && max_range < 65536u) ? 1u : 0u;
    L.radix_k16 = (radix && max_range < 65536u) ? 1u : 0u;
    if ((L.cnt16 ? 2ull : 4ull) * L.sort_cap > cap) { why = "ROI pixel count " + std::to_string(max_px) + " exceeds the LDS-resident value buffer"; return NYXHIP_ERR_ROI_TOO_LARGE; }
    if (L.radix_k16) off = align16(off + 2u * 2u * ((L.sort_cap + 7u) & ~7u) + 16);      // two 16-bit key buffers
    else off = align16(off + (L.cnt16 ? 2u : 4u) * L.sort_cap + 16);
    L.cnt = off; off = align16(off + (L.cnt16 ? 2u : 4u) * L.count_cap + 16);
    if (radix) {                                          // (second 32-bit key buffer +) [4][256] digit counts + the four wave totals
        if (8ull * L.sort_cap > cap) { why = "ROI pixel count " + std::to_string(max_px) + " exceeds the LDS-resident sort buffers"; return NYXHIP_ERR_ROI_TOO_LARGE; }
        L.radix = off; off = align16(off + (L.radix_k16 ? 0u : 4u * L.sort_cap) + 4u * (kWaves * 256 + kWaves) + 16);
    }
    const uint32_t cnt_end = off;                         // (the first-moment prefixes go here once the GLCM regions are known: below)
    if (do_glcm && L.g16) {
        const uint32_t ng = (uint32_t)s->grey_depth, cellsw = ((ng + 1) * ((ng + 3) & ~1u)) / 2;     // rows 0..ng of an even pitch (roi_features.hip, G16 block)
        L.ng_cap = ng; L.app = 4;
        uint32_t goff = shared0;
        L.P = goff; goff = align16(goff + 4u * 4u * cellsw);
        L.gscr = L.dense;                                        // (unused) | features | sums | row marginals: over the dead plane
        if (goff > off) off = goff;
    } else if (do_glcm) {
        const int greyInfo = s->ibsi ? 0 : s->grey_depth;
        auto glcm_bytes = [&](uint32_t ng, uint32_t app) -> size_t {
            return (size_t)align16(4u * app * ng * ng) + 8ull * (25ull * ng + 128);
        };
        uint32_t ng;
        if (greyInfo != 0) {
            ng = (uint32_t)abs(greyInfo);
            if (fixed + 2ull * (L.lvl_cap + 8) + glcm_bytes(ng, 1) > cap) {
                why = "GLCM grey depth " + std::to_string(ng) + " too large for the LDS-resident co-occurrence matrix";
                return NYXHIP_ERR_UNSUPPORTED;
            }
        } else {
            // IBSI: matrix order = the ROI's largest intensity (glcm.cpp:400-419: the reference allocates max x max).  Known
            // (exact launch groups: the class header carries it): exactly that order -- and if it does not fit LDS next to the
            // ROIs the group goes to the global workspace like any grey depth beyond LDS.  Not known (stated extrema): the
            // largest order that fits next to this batch's ROIs, up to 128; a larger ROI raises the error flag.
            if (vmax != 0) {
                ng = vmax < 8 ? 8 : vmax;
                if (shared0 + glcm_bytes(ng, 1) > cap) {
                    why = "IBSI GLCM matrix order " + std::to_string(ng) + " too large for the LDS-resident co-occurrence matrix";
                    return NYXHIP_ERR_UNSUPPORTED;
                }
            } else {
                ng = 128;
                while (ng > 8 && shared0 + glcm_bytes(ng, 1) > cap) ng >>= 1;
            }
        }
        uint32_t app = 4;
        while (app > 1 && ((!spill && 4ull * app * ng * ng > 64 * 1024) || shared0 + glcm_bytes(ng, app) > cap)) app >>= 1;
        L.ng_cap = ng;
        L.app = app;
        uint32_t goff = shared0;
        L.P = goff; goff = align16(goff + 4u * app * (ng <= 16 ? (ng + 1) * (ng + 1) : ng * ng));   // split launches count with a skip row / column
        L.gscr = goff; goff = align16(goff + 8u * (25u * ng + 128));
        if (goff > off) off = goff;
    }
    if (L.cnt16 && !spill) {
        // First-moment prefixes of the counting table (roi_features_body: the robust statistics are read off the count and the
        // first-moment prefix tables), behind the table: one word per G = 2^fm_shift entries, G = 8 .. 512 (the engine scans 512
        // entries per wave and step, eight per lane; a lookup walks the G / 8 lane chunks of its word).  The smallest G that costs
        // the launch no workgroup per CU (eight at the most: 64-VGPR builds of four waves) -- the benchmark ROI, a 4096-entry
        // table: G = 8, 2 KiB, 20 192 B of the 20 480 B that eight workgroups leave each; a 16384-entry table next to a small
        // ROI: G = 16.  Like [val | cnt] the words are dead after the intensity block: the GLCM regions may lie over them.
        auto wgs = lds_workgroups_per_cu;
        uint32_t sh = 3, with = off;
        for (;; sh++) {
            with = std::max(off, align16(cnt_end + 4u * ((L.count_cap + (1u << sh) - 1u) >> sh)));
            if (sh == 9 || wgs(with) >= wgs(off)) break;
        }
        L.fm = cnt_end; L.fm_shift = sh;
        off = with;
    }
    if (L.dense8) {
        // 8-bit plane launches keep the plane at the START of the carve-out (the kernel then needs no base add per store):
        // [fixed | plane | ...] becomes [plane | fixed | ...], everything behind the two stays where it is
        const uint32_t dsz = align16(plane_bytes);            // the plane's bytes (dense8 implies GLCM; L.dense is 16-byte aligned)
        L.out += dsz; L.red += dsz; L.stat += dsz; L.lbc += dsz;
        L.dense = 0;
        if (L.g16) L.gscr = 0;
    }
#ifndef NYX_NO_OVERLAP      // (diagnostic builds: every launch in the serial order)
    if (do_int && do_glcm && L.cnt16 && L.dense8 && !L.g16 && !spill) {
        // The overlapped builds of roi_features_body (INTENSITY + GLCM at <= 16 levels) count co-occurrences while wave 0 and wave 1
        // still read the counting table and the first-moment prefixes behind it.  The matrices lie over the value buffer, dead by
        // then: up to kMaxAngles of them with a skip row and column each, from L.P on.  Where they would run on into the table --
        // small ROIs beside a large matrix order -- the launch keeps the serial order.
        const uint32_t p_end = L.P + 4u * (uint32_t)kMaxAngles * (L.ng_cap + 1u) * (L.ng_cap + 1u);
        L.overlap = (L.P == L.val && p_end <= L.cnt) ? 1u : 0u;
    }
#endif
    if (spill) {
        // ---- workspace launches: the ROI-sized buffers (values, binned plane) live in global memory, but everything small and
        // atomics-heavy stays in LDS when it fits 60 KiB -- the fixed scratch always, then the co-occurrence matrices with their
        // feature scratch, the counting table, the level map.  (With all of it in the workspace a 96 k-pixel ROI spent two thirds of
        // its 4 ms in the global atomics of the co-occurrence sweep and the load pass.)  LDS-resident regions are exactly those at
        // offsets below L.gs_lds_bytes; nothing aliases.
        const uint32_t esz = L.cnt16 ? 2u : 4u;
        const uint64_t sz_val = align16(esz * L.sort_cap + 16), sz_cnt = do_int ? (uint64_t)esz * L.count_cap + 32 : 0;
        const uint64_t sz_dense = 2ull * L.dense_cap + 24, sz_lvl = do_glcm ? 2ull * (L.lvl_cap + 8) + 16 : 0;
        const uint64_t ngc = L.ng_cap, sz_P = do_glcm ? 4ull * L.app * (ngc <= 16 ? (ngc + 1) * (ngc + 1) : ngc * ngc) + 16 : 0;
        const uint64_t sz_g = do_glcm ? 8ull * (25ull * ngc + 128) + 16 : 0;
        const uint64_t kLdsMax = 60 * 1024;
        uint64_t o = fixed;
        const bool p_lds = do_glcm && o + sz_P + sz_g <= kLdsMax;
        if (p_lds) { L.P = (uint32_t)o; o = (o + sz_P + 15) & ~15ull; L.gscr = (uint32_t)o; o = (o + sz_g + 15) & ~15ull; }
        const bool c_lds = do_int && o + sz_cnt <= kLdsMax;
        if (c_lds) { L.cnt = (uint32_t)o; o = (o + sz_cnt + 15) & ~15ull; }
        const bool l_lds = do_glcm && o + sz_lvl <= kLdsMax;
        if (l_lds) { L.lvlmap = (uint32_t)o; o = (o + sz_lvl + 15) & ~15ull; }
        L.gs_lds_bytes = (uint32_t)o;
        if (do_glcm && !l_lds) { L.lvlmap = (uint32_t)o; o = (o + sz_lvl + 15) & ~15ull; }
        L.dense = (uint32_t)o; o = (o + sz_dense + 15) & ~15ull;
        L.val = (uint32_t)o; o = (o + sz_val + 15) & ~15ull;
        if (do_int && !c_lds) { L.cnt = (uint32_t)o; o = (o + sz_cnt + 15) & ~15ull; }
        if (do_glcm && !p_lds) { L.P = (uint32_t)o; o = (o + sz_P + 15) & ~15ull; L.gscr = (uint32_t)o; o = (o + sz_g + 15) & ~15ull; }
        if (o > cap) { why = "ROI too large for the global workspace (2 GiB of offsets per workgroup)"; return NYXHIP_ERR_ROI_TOO_LARGE; }
        off = (uint32_t)o;
    }
    L.total = off;
    if (L.total > cap) {
        why = "ROI too large for the LDS-resident path (" + std::to_string(L.total) + " B of LDS needed; max_px=" +
              std::to_string(max_px) + ", max_bbox_area=" + std::to_string(max_area) + ")";
        return NYXHIP_ERR_ROI_TOO_LARGE;
    }
    return NYXHIP_OK;
}

int ensure_stage(nyxhip_ctx* ctx, size_t bytes)
{
    HIP_TRY(ctx, ctx->d_stage.reserve(bytes, nullptr, bytes + bytes / 4 + (1 << 20)));
    return NYXHIP_OK;
}

int check_status(nyxhip_ctx* ctx)
{
    int two[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(two, ctx->d_status.p, 2 * sizeof(int), hipMemcpyDeviceToHost));
    const int st = two[0];
    if (ctx->census_pending) {         // whole-batch launches on stated extrema ran since the last look: what their scan met
        ctx->census_small = (uint32_t)two[1]; ctx->census_total = ctx->census_pending; ctx->census_pending = 0;
    }
    if (two[1]) HIP_TRY(ctx, hipMemsetAsync(ctx->d_status.as<int>() + 1, 0, sizeof(int), ctx->stream()));
    if (st != 0) {
        int zero = 0;
        HIP_TRY(ctx, hipMemcpy(ctx->d_status.p, &zero, sizeof(int), hipMemcpyHostToDevice));
        if (st == NYXHIP_ERR_ROI_TOO_LARGE)
            return fail(ctx, st, "an ROI exceeds the LDS-resident capacity declared by the batch extrema");
        if (st == NYXHIP_ERR_UNSUPPORTED)
            return fail(ctx, st, "GLCM matrix order exceeds the LDS-resident capacity (IBSI mode with large intensities?)");
        return fail(ctx, st, "device-side error " + std::to_string(st));
    }
    return NYXHIP_OK;
}

// Whole-slide mode, the dense chain: INTENSITY + GLCM of a device batch whose ROIs are dense images -- b->x, b->y and b->inten are NULL, ROI r
// is the elements [px_offset[r], px_offset[r + 1]) of d_inten, row-major in its box -- by the several-workgroups-per-ROI kernels of
// roi_large.hip with the dense load kernel in front.  E / tot: extrema and totals of the batch, as the class headers of
// launch_device_all state them for a class.  Every ROI must have a range below kLargeRangeMax.  *served = false: the settings do not
// fit those kernels and nothing was launched.
int launch_dense_slides(nyxhip_ctx* ctx, const nyxhip_batch* b, const void* d_inten, int dt, uint32_t mask, const nyxhip_settings* s, double* d_out, size_t ld,
                        const Extrema& E, const ClassTotals& tot, bool* served)
{
    hipStream_t st = ctx->stream();
    const uint32_t n = (uint32_t)b->n_roi;
    clear_runs(ctx);
    const size_t list_bytes = 4ull * n + 256;
    HIP_TRY(ctx, ctx->d_cls_list.reserve(list_bytes, st, list_bytes + list_bytes / 4));
    uint32_t* const list = ctx->d_cls_list.as<uint32_t>();
    if (int rc = launch_add_offset(nullptr, 0, n, list, st))
        return fail(ctx, NYXHIP_ERR_HIP, std::string("list launch failed: ") + hipGetErrorString((hipError_t)rc));
    ctx->dense_next = DenseSrc{d_inten, dt};
    const int rc = run_large(ctx, b, mask, s, d_out, ld, E, tot, list, n, served);
    ctx->dense_next = DenseSrc{};
    if (rc == NYXHIP_OK && *served) {
        ClassRun r{2 * (kSizeClasses - 1) + (E.range < 16384u ? 0 : 1), n, E, 0, nullptr, nullptr};
        r.cooperative = 1 | 8;                          // bit 3: the load pass read dense images (nyxhip_launch_report)
        ctx->runs.push_back(r);
    }
    return rc;
}

int launch_add_offset(const uint32_t* in, uint32_t add, uint32_t n, uint32_t* out, hipStream_t st)
{
    hipLaunchKernelGGL(add_offset_kernel, dim3((n + 255) / 256), dim3(256), 0, st, in, add, n, out);
    return (int)hipGetLastError();
}

void clear_runs(nyxhip_ctx* ctx)
{
    for (ClassRun& r : ctx->runs) {
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
        if (r.e2) (void)hipEventDestroy(r.e2);
    }
    ctx->runs.clear();
}

// launch_device_all between two events on the launch stream: the timing hooks of include/nyxhip.h cover EVERY kernel the call
// enqueues (the LDS launch groups, the moments pair, the global-workspace and large-ROI passes), on every return path.
int launch_device(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* d_out,
                  size_t ld, uint32_t max_px, uint32_t max_area, uint32_t max_range, uint32_t max_side, bool hinted)
{
    if (!ctx->timing)
        return launch_device_all(ctx, b, mask, s, d_out, ld, max_px, max_area, max_range, max_side, hinted);
    hipStream_t st = ctx->stream();
    if (ctx->ev_used == ctx->ev.size()) {
        hipEvent_t x, y;
        HIP_TRY(ctx, hipEventCreate(&x));
        HIP_TRY(ctx, hipEventCreate(&y));
        ctx->ev.push_back({x, y});
    }
    hipEvent_t e0 = ctx->ev[ctx->ev_used].first, e1 = ctx->ev[ctx->ev_used].second;
    HIP_TRY(ctx, hipEventRecord(e0, st));
    const int rc = launch_device_all(ctx, b, mask, s, d_out, ld, max_px, max_area, max_range, max_side, hinted);
    HIP_TRY(ctx, hipEventRecord(e1, st));
    ctx->ev_used++;
    return rc;
}

int validate(nyxhip_ctx* ctx, const nyxhip_batch* b, uint32_t mask, const nyxhip_settings* s, double* out, size_t ld)
{
    if (!ctx) return NYXHIP_ERR_INVALID_ARG;
    if (!b || !s || !out) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "null batch / settings / out_table");
    if (mask == 0 || (mask & ~(NYXHIP_FAM_ALL | NYXHIP_FAM_RADIAL | kOutline | kCaliper | NYXHIP_FAM_CHORDS | kEllipseErosion | kCircleGeodetic))) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "bad family mask");
    if (mask & ~kImplemented)
        return fail(ctx, NYXHIP_ERR_UNSUPPORTED, "requested feature family is not implemented by the HIP path yet "
                    "(all seven hot-path families are implemented; bad mask?)");
    std::string why;
    if (!settings_ok(s, mask, why)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, why);
    if (b->n_roi && (!b->px_offset || !b->x || !b->y || !b->inten || !b->bbox_w || !b->bbox_h || !b->min_inten || !b->max_inten))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "batch has null array pointers");
    if ((b->slide_min == nullptr) != (b->slide_max == nullptr))
        return fail(ctx, NYXHIP_ERR_INVALID_ARG, "slide_min and slide_max must both be given or both NULL");
    if ((int)ld < nyxhip_n_columns(mask, s)) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "out_ld smaller than the column count");
    if (b->n_roi > 0x7FFFFFFFull) return fail(ctx, NYXHIP_ERR_INVALID_ARG, "too many ROIs in one batch");
    return NYXHIP_OK;
}

} // namespace nyxhip
