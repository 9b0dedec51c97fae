// device_prims_probe.hip -- TEST PROGRAM (tests/test_device_prims_gpu.py): calls the shared device primitives of
// nyxus_amd/csrc/device_math.h and sort_lds.h one by one, on inputs the Python side chose, and writes back what they returned.
// Built with the library's own flags (-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off); never shipped.
//
//   device_prims_probe OP request.bin result.bin
//
// Both files are a list of arrays: u64 count, then per array u64 byte length + the bytes (padded to 8).  What the arrays mean is
// fixed per OP (see the op_* functions below and run() in the test file); every expected value lives on the Python side.
//
// Launch rules: the cross-lane helpers (DPP, permlane, readlane, ballots of the sort) are only ever called by FULL waves -- block
// sizes are multiples of 64, the grids cover whole waves (the Python side pads), and no such call sits under divergent control
// flow; that is how the kernels call them.  Per-element arithmetic (divisions, binning, multiplies) runs under the usual
// `i < n` guard.  The wrappers store with plain C++ assignments.  Every HIP call is checked; an error prints and exits non-zero.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nyxus_amd/csrc/device_math.h"
#include "../../nyxus_amd/csrc/sort_lds.h"

using namespace nyxhip;

#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return 1; } } while (0)
#define NEED(c) do { if (!(c)) { fprintf(stderr, "%s:%d bad request: %s\n", __FILE__, __LINE__, #c); return 2; } } while (0)

typedef std::vector<std::vector<char>> Arrays;

static int up(const std::vector<char>& h, void** d, size_t min_bytes = 0)
{
    size_t nb = h.size() > min_bytes ? h.size() : min_bytes;
    TRY(hipMalloc(d, nb ? nb : 8));
    if (h.size()) TRY(hipMemcpy(*d, h.data(), h.size(), hipMemcpyHostToDevice));
    return 0;
}
static int zeros(void** d, size_t nb)
{
    TRY(hipMalloc(d, nb ? nb : 8));
    TRY(hipMemset(*d, 0, nb ? nb : 8));
    return 0;
}
static int down(Arrays& out, const void* d, size_t nb)
{
    out.emplace_back(nb);
    if (nb) TRY(hipMemcpy(out.back().data(), d, nb, hipMemcpyDeviceToHost));
    return 0;
}
static int done()
{
    TRY(hipGetLastError());
    TRY(hipDeviceSynchronize());
    return 0;
}
static unsigned blocks(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// ---- divisions: M = 0 fdiv(a, b), 1 frcp(b), 2 frsq(b) --------------------------------------------------------------------
template <int M>
__global__ void k_div(const double* a, const double* b, double* o, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = M == 0 ? fdiv(a[i], b[i]) : M == 1 ? frcp(b[i]) : frsq(b[i]);
}
static int op_div(int m, const Arrays& in, Arrays& out)     // in: [a f64[n]] b f64[n]; out: f64[n]
{
    NEED(in.size() == (m == 0 ? 2u : 1u));
    const uint64_t n = in.back().size() / 8;
    NEED(n > 0 && in[0].size() == n * 8);
    void *a = nullptr, *b, *o;
    if (m == 0 && up(in[0], &a)) return 1;
    if (up(in.back(), &b) || zeros(&o, n * 8)) return 1;
    if (m == 0) hipLaunchKernelGGL(k_div<0>, dim3(blocks(n, 256)), dim3(256), 0, 0, (const double*)a, (const double*)b, (double*)o, n);
    else if (m == 1) hipLaunchKernelGGL(k_div<1>, dim3(blocks(n, 256)), dim3(256), 0, 0, (const double*)b, (const double*)b, (double*)o, n);
    else hipLaunchKernelGGL(k_div<2>, dim3(blocks(n, 256)), dim3(256), 0, 0, (const double*)b, (const double*)b, (double*)o, n);
    return done() || down(out, o, n * 8);
}

// fdiv over the grid a[i] / b[j] (the integer quotients the kernels form): out f64[na][nb]
__global__ void k_div_grid(const double* a, uint32_t na, const double* b, uint32_t nb, double* o)
{
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (g >= (uint64_t)na * nb) return;
    o[g] = fdiv(a[g / nb], b[g % nb]);
}
static int op_div_grid(const Arrays& in, Arrays& out)       // in: a f64[na], b f64[nb]; out: f64[na][nb]
{
    NEED(in.size() == 2);
    const uint64_t na = in[0].size() / 8, nb = in[1].size() / 8;
    NEED(na > 0 && nb > 0 && na * nb <= (1ull << 25));
    void *a, *b, *o;
    if (up(in[0], &a) || up(in[1], &b) || zeros(&o, na * nb * 8)) return 1;
    hipLaunchKernelGGL(k_div_grid, dim3(blocks(na * nb, 256)), dim3(256), 0, 0, (const double*)a, (uint32_t)na, (const double*)b, (uint32_t)nb, (double*)o);
    return done() || down(out, o, na * nb * 8);
}

// ---- fast_log2f(x) and plogp(p, arg) -----------------------------------------------------------------------------------------
__global__ void k_log2f(const double* x, float* o, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = fast_log2f(x[i]);
}
__global__ void k_plogp(const double* p, const double* arg, double* o, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = plogp(p[i], arg[i]);
}
static int op_log2f(const Arrays& in, Arrays& out)          // in: x f64[n]; out: f32[n]
{
    NEED(in.size() == 1);
    const uint64_t n = in[0].size() / 8;
    NEED(n > 0);
    void *x, *o;
    if (up(in[0], &x) || zeros(&o, n * 4)) return 1;
    hipLaunchKernelGGL(k_log2f, dim3(blocks(n, 256)), dim3(256), 0, 0, (const double*)x, (float*)o, n);
    return done() || down(out, o, n * 4);
}
static int op_plogp(const Arrays& in, Arrays& out)          // in: p f64[n], arg f64[n]; out: f64[n]
{
    NEED(in.size() == 2);
    const uint64_t n = in[0].size() / 8;
    NEED(n > 0 && in[1].size() == n * 8);
    void *p, *a, *o;
    if (up(in[0], &p) || up(in[1], &a) || zeros(&o, n * 8)) return 1;
    hipLaunchKernelGGL(k_plogp, dim3(blocks(n, 256)), dim3(256), 0, 0, (const double*)p, (const double*)a, (double*)o, n);
    return done() || down(out, o, n * 8);
}

// ---- binning: M = 0 bin_pixel(x, mn, mx, info), 1 bin_radiomix(x, mn, mx, count), 2 bin_matlab(x, slope, levels),
//               3 to_grayscale(i, min, range, levels) -------------------------------------------------------------------------
template <int M>
__global__ void k_bin(const uint32_t* x, const uint32_t* p1, const uint32_t* p2, const int32_t* p3, const double* slope, uint32_t* o, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (M == 0) o[i] = bin_pixel(x[i], p1[i], p2[i], p3[i]);
    else if (M == 1) o[i] = bin_radiomix(x[i], p1[i], p2[i], p3[i]);
    else if (M == 2) o[i] = bin_matlab(x[i], slope[i], p3[i]);
    else o[i] = to_grayscale(x[i], p1[i], p2[i], (uint32_t)p3[i]);
}
static int op_bin(int m, const Arrays& in, Arrays& out)     // in: x u32[n], p1 u32[n], p2 u32[n], p3 i32[n], slope f64[n]; out: u32[n]
{
    NEED(in.size() == 5);
    const uint64_t n = in[0].size() / 4;
    NEED(n > 0 && in[1].size() == n * 4 && in[2].size() == n * 4 && in[3].size() == n * 4 && in[4].size() == n * 8);
    void *x, *p1, *p2, *p3, *sl, *o;
    if (up(in[0], &x) || up(in[1], &p1) || up(in[2], &p2) || up(in[3], &p3) || up(in[4], &sl) || zeros(&o, n * 4)) return 1;
#define BIN_LAUNCH(M) hipLaunchKernelGGL(k_bin<M>, dim3(blocks(n, 256)), dim3(256), 0, 0, (const uint32_t*)x, (const uint32_t*)p1, (const uint32_t*)p2, (const int32_t*)p3, (const double*)sl, (uint32_t*)o, n)
    if (m == 0) BIN_LAUNCH(0); else if (m == 1) BIN_LAUNCH(1); else if (m == 2) BIN_LAUNCH(2); else BIN_LAUNCH(3);
    return done() || down(out, o, n * 4);
}

// ---- 24-bit arithmetic, per-lane operands: out[0] mul24(a, b), out[1] mad24(a, b, c), out[2] mul_i24(a, b) ------------------------
__global__ void k_i24(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* o_mul, uint32_t* o_mad, uint32_t* o_imul, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    o_mul[i] = mul24(a[i], b[i]);
    o_mad[i] = mad24(a[i], b[i], c[i]);
    o_imul[i] = (uint32_t)mul_i24((int)a[i], (int)b[i]);
}
static int op_i24(const Arrays& in, Arrays& out)            // in: a, b, c u32[n]; out: 3 x u32[n]
{
    NEED(in.size() == 3);
    const uint64_t n = in[0].size() / 4;
    NEED(n > 0 && in[1].size() == n * 4 && in[2].size() == n * 4);
    void *a, *b, *c, *o0, *o1, *o2;
    if (up(in[0], &a) || up(in[1], &b) || up(in[2], &c) || zeros(&o0, n * 4) || zeros(&o1, n * 4) || zeros(&o2, n * 4)) return 1;
    hipLaunchKernelGGL(k_i24, dim3(blocks(n, 256)), dim3(256), 0, 0, (const uint32_t*)a, (const uint32_t*)b, (const uint32_t*)c, (uint32_t*)o0, (uint32_t*)o1, (uint32_t*)o2, n);
    return done() || down(out, o0, n * 4) || down(out, o1, n * 4) || down(out, o2, n * 4);
}
// the wave-uniform forms: the uniform operand is a kernel argument (one launch per value)
__global__ void k_u24_su(const uint32_t* a, const uint32_t* c, uint32_t b_uniform, uint32_t* o_mul, uint32_t* o_mad, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    o_mul[i] = mul_u24_su(a[i], b_uniform);
    o_mad[i] = mad_u24_su(a[i], b_uniform, c[i]);
}
static int op_u24_su(const Arrays& in, Arrays& out)         // in: a u32[n], c u32[n], b u32[m]; out: mul u32[m][n], mad u32[m][n]
{
    NEED(in.size() == 3);
    const uint64_t n = in[0].size() / 4, m = in[2].size() / 4;
    NEED(n > 0 && m > 0 && m <= 4096 && in[1].size() == n * 4);
    const uint32_t* hb = (const uint32_t*)in[2].data();
    void *a, *c, *o0, *o1;
    if (up(in[0], &a) || up(in[1], &c) || zeros(&o0, m * n * 4) || zeros(&o1, m * n * 4)) return 1;
    for (uint64_t j = 0; j < m; j++)
        hipLaunchKernelGGL(k_u24_su, dim3(blocks(n, 256)), dim3(256), 0, 0, (const uint32_t*)a, (const uint32_t*)c, hb[j], (uint32_t*)o0 + j * n, (uint32_t*)o1 + j * n, n);
    return done() || down(out, o0, m * n * 4) || down(out, o1, m * n * 4);
}
__global__ void k_med3(const uint32_t* x, uint32_t lo_uniform, uint32_t hi_uniform, uint32_t* o, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = med3_u32_ss(x[i], lo_uniform, hi_uniform);
}
static int op_med3(const Arrays& in, Arrays& out)           // in: x u32[n], lo u32[m], hi u32[m]; out: u32[m][n]
{
    NEED(in.size() == 3);
    const uint64_t n = in[0].size() / 4, m = in[1].size() / 4;
    NEED(n > 0 && m > 0 && m <= 4096 && in[2].size() == m * 4);
    const uint32_t *lo = (const uint32_t*)in[1].data(), *hi = (const uint32_t*)in[2].data();
    for (uint64_t j = 0; j < m; j++) NEED(lo[j] <= hi[j]);
    void *x, *o;
    if (up(in[0], &x) || zeros(&o, m * n * 4)) return 1;
    for (uint64_t j = 0; j < m; j++)
        hipLaunchKernelGGL(k_med3, dim3(blocks(n, 256)), dim3(256), 0, 0, (const uint32_t*)x, lo[j], hi[j], (uint32_t*)o + j * n, n);
    return done() || down(out, o, m * n * 4);
}
__global__ void k_cnt16(uint32_t* tab, uint32_t* o, uint32_t n)   // the byte offset of the word from the base (nothing is dereferenced)
{
    const uint32_t ci = blockIdx.x * blockDim.x + threadIdx.x;
    if (ci >= n) return;
    o[ci] = (uint32_t)((char*)cnt16_word(tab, ci) - (char*)tab);
}
static int op_cnt16(const Arrays& in, Arrays& out)          // in: n u32[1]; out: u32[n]
{
    NEED(in.size() == 1 && in[0].size() == 4);
    const uint32_t n = *(const uint32_t*)in[0].data();
    NEED(n > 0 && n <= (1u << 20));
    void *tab, *o;
    if (zeros(&tab, (size_t)n * 2 + 8) || zeros(&o, (size_t)n * 4)) return 1;
    hipLaunchKernelGGL(k_cnt16, dim3(blocks(n, 256)), dim3(256), 0, 0, (uint32_t*)tab, (uint32_t*)o, n);
    return done() || down(out, o, (size_t)n * 4);
}

// ---- RowCol ------------------------------------------------------------------------------------------------------------------
// small-operand constructor, exhaustive: thread g -> width (g >> 16) + 1, first = stride = g & 65535.  Rows and columns go back in
// full (u16 / u8); the device also counts the cases that differ from its own integer division and keeps the first 16.
__global__ void k_rowcol_small(uint32_t n_width, uint16_t* rows, uint8_t* cols, uint32_t* n_bad, uint32_t* bad)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_width * 65536u) return;
    const uint32_t width = (g >> 16) + 1u, first = g & 65535u;
    const RowCol rc(first, first, width, RowCol::small_t{});
    rows[g] = (uint16_t)rc.row; cols[g] = (uint8_t)rc.col;
    const uint32_t q = first / width, r = first - q * width;
    if (rc.row != q || rc.col != r || rc.step_r != q || rc.step_c != r || rc.w != width || rc.row > 65535u || rc.col > 255u) {
        const uint32_t slot = atomicAdd(n_bad, 1u);
        if (slot < 16u) { bad[4 * slot] = first; bad[4 * slot + 1] = width; bad[4 * slot + 2] = rc.row; bad[4 * slot + 3] = rc.col; }
    }
}
static int op_rowcol_small(const Arrays& in, Arrays& out)   // in: n_width u32[1] (<= 64); out: rows u16[nw * 65536], cols u8[..], n_bad u32[1], bad u32[16][4]
{
    NEED(in.size() == 1 && in[0].size() == 4);
    const uint32_t nw = *(const uint32_t*)in[0].data();
    NEED(nw >= 1 && nw <= 64);
    const size_t n = (size_t)nw * 65536;
    void *rows, *cols, *n_bad, *bad;
    if (zeros(&rows, n * 2) || zeros(&cols, n) || zeros(&n_bad, 4) || zeros(&bad, 16 * 4 * 4)) return 1;
    hipLaunchKernelGGL(k_rowcol_small, dim3(blocks(n, 256)), dim3(256), 0, 0, nw, (uint16_t*)rows, (uint8_t*)cols, (uint32_t*)n_bad, (uint32_t*)bad);
    return done() || down(out, rows, n * 2) || down(out, cols, n) || down(out, n_bad, 4) || down(out, bad, 16 * 4 * 4);
}
// either constructor, then `steps` calls of advance(): (row, col) before the first and after every step
template <bool SMALL>
__global__ void k_rowcol_walk(const uint32_t* first, const uint32_t* stride, const uint32_t* width, uint32_t steps, uint32_t* o, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RowCol rc = SMALL ? RowCol(first[i], stride[i], width[i], RowCol::small_t{}) : RowCol(first[i], stride[i], width[i]);
    uint32_t* const p = o + (size_t)i * (steps + 1) * 2;
    p[0] = rc.row; p[1] = rc.col;
    for (uint32_t k = 1; k <= steps; k++) {
        rc.advance();
        p[2 * k] = rc.row; p[2 * k + 1] = rc.col;
    }
}
static int op_rowcol_walk(bool small, const Arrays& in, Arrays& out)  // in: first, stride, width u32[n], steps u32[1]; out: u32[n][steps + 1][2]
{
    NEED(in.size() == 4 && in[3].size() == 4);
    const uint32_t n = (uint32_t)(in[0].size() / 4), steps = *(const uint32_t*)in[3].data();
    NEED(n > 0 && n <= (1u << 20) && steps <= 1024 && in[1].size() == (size_t)n * 4 && in[2].size() == (size_t)n * 4);
    const uint32_t *hf = (const uint32_t*)in[0].data(), *hs = (const uint32_t*)in[1].data(), *hw = (const uint32_t*)in[2].data();
    for (uint32_t i = 0; i < n; i++) {
        NEED(hw[i] >= 1);
        if (small) NEED(hf[i] < 65536u && hs[i] < 65536u && hw[i] <= 64u);
    }
    void *f, *s, *w, *o;
    const size_t nb = (size_t)n * (steps + 1) * 8;
    if (up(in[0], &f) || up(in[1], &s) || up(in[2], &w) || zeros(&o, nb)) return 1;
    if (small) hipLaunchKernelGGL(k_rowcol_walk<true>, dim3(blocks(n, 256)), dim3(256), 0, 0, (const uint32_t*)f, (const uint32_t*)s, (const uint32_t*)w, steps, (uint32_t*)o, n);
    else hipLaunchKernelGGL(k_rowcol_walk<false>, dim3(blocks(n, 256)), dim3(256), 0, 0, (const uint32_t*)f, (const uint32_t*)s, (const uint32_t*)w, steps, (uint32_t*)o, n);
    return done() || down(out, o, nb);
}

// ---- reductions, scans, shifts: one wave per case, 64 x u64 in (doubles by their bits), 64 x u64 out ------------------------
enum WaveOp { W_SUM_F64, W_SUM_U64, W_SUM_U32, W_SCAN_U32, W_SCAN_MIN_U32, W_MAX_NONNEG, W_MAX_U32, W_ROW16_SUM_F64, W_ROW16_SUM_U32,
              W_ROW16_MAX, W_PLUS1, W_PLUS1_LIT0, W_MINUS1, W_MINUS1_LIT0, W_PLUS1_Z, W_MINUS1_Z, W_ROL1, W_ROR1, W_RL63_F64, W_RL63_U64,
              W_RL63_U32, W_READLANE_U64, W_READLANE_F64, W_N_OPS };
static const char* const kWaveNames[W_N_OPS] = {"wave_sum", "wave_sum_u64", "wave_sum_u32", "wave_scan_u32", "wave_scan_min_u32", "wave_max_nonneg", "wave_max_u32",
    "row16_sum", "row16_sum_u32", "row16_max", "lane_plus1", "lane_plus1_lit0", "lane_minus1", "lane_minus1_lit0", "lane_plus1_z", "lane_minus1_z", "wave_rol1", "wave_ror1",
    "readlane63_f64", "readlane63_u64", "readlane63_u32", "readlane_u64", "readlane_f64"};
__device__ __forceinline__ uint64_t dbits(double d) { return (uint64_t)__double_as_longlong(d); }
template <int OP>
__global__ void k_wave(const uint64_t* in, uint64_t* out, uint32_t aux)   // aux: the fill of the shifts, the lane of readlane_* (wave-uniform)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;             // (the grid covers whole waves exactly)
    const uint64_t u = in[g];
    const uint32_t w = (uint32_t)u;
    const double d = __longlong_as_double((long long)u);
    uint64_t r = 0;
    if (OP == W_SUM_F64) r = dbits(wave_sum(d));
    else if (OP == W_SUM_U64) r = wave_sum_u64(u);
    else if (OP == W_SUM_U32) r = wave_sum_t<uint32_t>(w);
    else if (OP == W_SCAN_U32) r = wave_scan_u32(w);
    else if (OP == W_SCAN_MIN_U32) r = wave_scan_min_u32(w);
    else if (OP == W_MAX_NONNEG) r = dbits(wave_max_nonneg(d));
    else if (OP == W_MAX_U32) r = wave_max_u32(w);
    else if (OP == W_ROW16_SUM_F64) r = dbits(row16_sum(d));
    else if (OP == W_ROW16_SUM_U32) r = row16_sum(w);
    else if (OP == W_ROW16_MAX) r = dbits(row16_max(d));
    else if (OP == W_PLUS1) r = lane_plus1(w, aux);
    else if (OP == W_PLUS1_LIT0) r = lane_plus1(w, 0u);
    else if (OP == W_MINUS1) r = lane_minus1(w, aux);
    else if (OP == W_MINUS1_LIT0) r = lane_minus1(w, 0u);
    else if (OP == W_PLUS1_Z) r = lane_plus1_z(w);
    else if (OP == W_MINUS1_Z) r = lane_minus1_z(w);
    else if (OP == W_ROL1) r = wave_rol1(w);
    else if (OP == W_ROR1) r = wave_ror1(w);
    else if (OP == W_RL63_F64) r = dbits(readlane63(d));
    else if (OP == W_RL63_U64) r = readlane63((unsigned long long)u);
    else if (OP == W_RL63_U32) r = readlane63(w);
    else if (OP == W_READLANE_U64) r = readlane_u64(u, (int)aux);
    else if (OP == W_READLANE_F64) r = dbits(readlane_f64(d, (int)aux));
    out[g] = r;
}
template <int OP>
static void wave_launch(int op, const uint64_t* in, uint64_t* out, uint32_t aux, unsigned grid)
{
    if (op == OP) hipLaunchKernelGGL(k_wave<OP>, dim3(grid), dim3(256), 0, 0, in, out, aux);
    if constexpr (OP + 1 < W_N_OPS) wave_launch<OP + 1>(op, in, out, aux, grid);
}
static int op_wave(const Arrays& in, Arrays& out)           // in: name (chars), values u64[ncase][64] (ncase % 4 == 0), aux u32[m]; out: u64[m][ncase][64]
{
    NEED(in.size() == 3);
    const std::string name(in[0].data(), strnlen(in[0].data(), in[0].size()));
    int op = -1;
    for (int k = 0; k < W_N_OPS; k++) if (name == kWaveNames[k]) op = k;
    NEED(op >= 0);
    const uint64_t n = in[1].size() / 8, m = in[2].size() / 4;
    NEED(n > 0 && n % 256 == 0 && m >= 1 && m <= 64);
    const uint32_t* aux = (const uint32_t*)in[2].data();
    if (op == W_READLANE_U64 || op == W_READLANE_F64) for (uint64_t j = 0; j < m; j++) NEED(aux[j] < 64u);
    void *v, *o;
    if (up(in[1], &v) || zeros(&o, m * n * 8)) return 1;
    for (uint64_t j = 0; j < m; j++) wave_launch<0>(op, (const uint64_t*)v, (uint64_t*)o + j * n, aux[j], (unsigned)(n / 256));
    return done() || down(out, o, m * n * 8);
}

// ---- transposed sums: one wave per case.  Cases c < n_onehot are made here: a single val[c] in slot c / 64 of lane c % 64;
//      the others are read in full, [case][slot][lane] doubles.  out: f64[case][64] ------------------------------------------------
template <int K, bool U32>
__global__ void k_transpose(const double* val, uint32_t n_onehot, const double* dense, double* out)
{
    const uint32_t c = blockIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (c < n_onehot) v[k] = (c >> 6) == (uint32_t)k && (c & 63u) == (uint32_t)lane ? val[c] : 0.0;
        else v[k] = dense[((size_t)(c - n_onehot) * K + k) * 64 + lane];
    }
    double r;
    if constexpr (U32) {
        uint32_t w[K];
#pragma unroll
        for (int k = 0; k < K; k++) w[k] = (uint32_t)v[k];
        r = (double)wave_transpose_sum8_u32(w, lane);
    } else if constexpr (K == 4) r = wave_transpose_sum4(v);
    else if constexpr (K == 8) r = wave_transpose_sum8(v, lane);
    else if constexpr (K == 16) r = wave_transpose_sum16(v, lane);
    else r = wave_transpose_sum64(v, lane);
    out[(size_t)c * 64 + lane] = r;
}
static int op_transpose(int k, bool u32, const Arrays& in, Arrays& out)   // in: val f64[n_onehot] (n_onehot <= 64 k), dense f64[nd][k][64]
{
    NEED(in.size() == 2);
    const uint64_t n1 = in[0].size() / 8, per = (uint64_t)k * 64, nd = in[1].size() / 8 / per;
    NEED(n1 <= per && in[1].size() == nd * per * 8 && n1 + nd > 0 && n1 + nd <= (1u << 16));
    void *val, *dense, *o;
    const uint64_t nc = n1 + nd;
    if (up(in[0], &val) || up(in[1], &dense) || zeros(&o, nc * 64 * 8)) return 1;
#define TR_LAUNCH(K, U) hipLaunchKernelGGL((k_transpose<K, U>), dim3((unsigned)nc), dim3(64), 0, 0, (const double*)val, (uint32_t)n1, (const double*)dense, (double*)o)
    if (u32) { NEED(k == 8); TR_LAUNCH(8, true); }
    else if (k == 4) TR_LAUNCH(4, false);
    else if (k == 8) TR_LAUNCH(8, false);
    else if (k == 16) TR_LAUNCH(16, false);
    else { NEED(k == 64); TR_LAUNCH(64, false); }
    return done() || down(out, o, nc * 64 * 8);
}

// ---- for_each_cloud_pixel<256>: one workgroup per case; the case's arrays hold n elements and then `cap - n` sentinels, which only a
//      wrong loop would ever deliver (the helper's own bounded loads are the only reads) -------------------------------------------
__global__ __launch_bounds__(256) void k_cloud(const uint32_t* inten, const uint16_t* x, const uint16_t* y, const uint32_t* desc,
                                               uint32_t* visits, uint32_t* gv, uint32_t* gx, uint32_t* gy, uint32_t* beyond)
{
    const uint32_t c = blockIdx.x, off = desc[3 * c], n = desc[3 * c + 1], cap = desc[3 * c + 2];
    for_each_cloud_pixel<256>(inten + off, x + off, y + off, n, (int)threadIdx.x, [&](uint32_t i, uint32_t v, uint32_t px, uint32_t py) {
        if (i < cap) {
            atomicAdd(&visits[off + i], 1u);
            gv[off + i] = v; gx[off + i] = px; gy[off + i] = py;
        } else {
            atomicAdd(&beyond[c], 1u);
        }
    });
}
static int op_cloud(const Arrays& in, Arrays& out)          // in: inten u32[tot], x u16[tot], y u16[tot], desc u32[nc][3] = (offset, n, cap)
{
    NEED(in.size() == 4);
    const uint64_t tot = in[0].size() / 4, nc = in[3].size() / 12;
    NEED(tot > 0 && nc > 0 && nc <= 4096 && in[1].size() == tot * 2 && in[2].size() == tot * 2 && in[3].size() == nc * 12);
    const uint32_t* d = (const uint32_t*)in[3].data();
    for (uint64_t c = 0; c < nc; c++) NEED(d[3 * c] % 8 == 0 && d[3 * c + 1] <= d[3 * c + 2] && (uint64_t)d[3 * c] + d[3 * c + 2] <= tot && d[3 * c + 1] < (1u << 28));
    void *iv, *x, *y, *desc, *vis, *gv, *gx, *gy, *bey;
    if (up(in[0], &iv) || up(in[1], &x) || up(in[2], &y) || up(in[3], &desc)) return 1;
    if (zeros(&vis, tot * 4) || zeros(&gv, tot * 4) || zeros(&gx, tot * 4) || zeros(&gy, tot * 4) || zeros(&bey, nc * 4)) return 1;
    hipLaunchKernelGGL(k_cloud, dim3((unsigned)nc), dim3(256), 0, 0, (const uint32_t*)iv, (const uint16_t*)x, (const uint16_t*)y, (const uint32_t*)desc,
                       (uint32_t*)vis, (uint32_t*)gv, (uint32_t*)gx, (uint32_t*)gy, (uint32_t*)bey);
    return done() || down(out, vis, tot * 4) || down(out, gv, tot * 4) || down(out, gx, tot * 4) || down(out, gy, tot * 4) || down(out, bey, nc * 4);
}

// ---- radix_sort<GS, NW, KEY>: one workgroup of NW waves per case.  desc[c] = (offset, n, kmin, range); the case's keys are
//      keys[offset .. offset + n).  GS = false: both key buffers and the tables are LDS (dynamic); GS = true: they are global memory
//      (the uploaded keys themselves are buffer a).  out: the returned buffer's first n keys, which buffer it was (0 = a, 1 = b), and
//      what buffer a holds afterwards ---------------------------------------------------------------------------------------------
template <bool GS, int NW, typename KEY>
__global__ __launch_bounds__(NW * 64) void k_sort(KEY* keys, KEY* work_b, uint32_t* g_hist, const uint32_t* desc, uint32_t cap, KEY* sorted, uint32_t* which, KEY* a_after)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t c = blockIdx.x, off = desc[4 * c], n = desc[4 * c + 1], kmin = desc[4 * c + 2], range = desc[4 * c + 3];
    const int tid = (int)threadIdx.x;
    KEY *a, *b;
    uint32_t* hist;
    if (GS) {
        a = keys + off; b = work_b + off; hist = g_hist + (size_t)c * (NW * 256 + NW);
    } else {
        a = (KEY*)lds_raw; b = a + cap; hist = (uint32_t*)(b + cap);
        for (uint32_t i = (uint32_t)tid; i < n; i += NW * 64) a[i] = keys[off + i];
        __syncthreads();
    }
    KEY* const r = radix_sort<GS, NW, KEY>(a, b, hist, n, kmin, range, tid);
    blk_sync<GS>();
    for (uint32_t i = (uint32_t)tid; i < n; i += NW * 64) { sorted[off + i] = r[i]; a_after[off + i] = a[i]; }
    if (tid == 0) which[c] = r == a ? 0u : 1u;
}
template <bool GS, int NW, typename KEY>
static int sort_run(const Arrays& in, Arrays& out)          // in: keys KEY[tot], desc u32[nc][4]
{
    NEED(in.size() == 2);
    const uint64_t tot = in[0].size() / sizeof(KEY), nc = in[1].size() / 16;
    NEED(tot > 0 && nc > 0 && nc <= (1u << 16) && in[1].size() == nc * 16);
    const uint32_t* d = (const uint32_t*)in[1].data();
    const KEY* hk = (const KEY*)in[0].data();
    uint32_t cap = 8;
    for (uint64_t c = 0; c < nc; c++) {
        const uint32_t off = d[4 * c], n = d[4 * c + 1], kmin = d[4 * c + 2], range = d[4 * c + 3];
        NEED(off % 8 == 0 && n >= 1 && n <= 8192 && (uint64_t)off + n <= tot);
        for (uint32_t i = 0; i < n; i++) NEED((uint32_t)hk[off + i] >= kmin && (uint32_t)hk[off + i] - kmin <= range);   // the sort's contract
        if (((n + 7u) & ~7u) > cap) cap = (n + 7u) & ~7u;
    }
    const size_t lds = GS ? 0 : 2 * (size_t)cap * sizeof(KEY) + (NW * 256 + NW) * 4;
    NEED(lds <= 64 * 1024);
    void *keys, *wb, *hist, *desc, *sorted, *which, *after;
    if (up(in[0], &keys) || up(in[1], &desc) || zeros(&wb, tot * sizeof(KEY)) || zeros(&hist, GS ? nc * (NW * 256 + NW) * 4 : 8)) return 1;
    if (zeros(&sorted, tot * sizeof(KEY)) || zeros(&which, nc * 4) || zeros(&after, tot * sizeof(KEY))) return 1;
    hipLaunchKernelGGL((k_sort<GS, NW, KEY>), dim3((unsigned)nc), dim3(NW * 64), lds, 0, (KEY*)keys, (KEY*)wb, (uint32_t*)hist, (const uint32_t*)desc, cap,
                       (KEY*)sorted, (uint32_t*)which, (KEY*)after);
    return done() || down(out, sorted, tot * sizeof(KEY)) || down(out, which, nc * 4) || down(out, after, tot * sizeof(KEY));
}
// exactly the instantiations of the library: roi_features.hip <GS, NW, u16 | u32> with GS in {false, true} at NW = 4 and GS = false at
// NW = 8 (the 512-thread launch); roi_wide.hip <false, 4, u16>; roi_chords.hip <false, kHW = 4, u32>
static int op_sort(const std::string& v, const Arrays& in, Arrays& out)
{
    if (v == "lds_4_u16") return sort_run<false, 4, uint16_t>(in, out);
    if (v == "lds_4_u32") return sort_run<false, 4, uint32_t>(in, out);
    if (v == "gs_4_u16") return sort_run<true, 4, uint16_t>(in, out);
    if (v == "gs_4_u32") return sort_run<true, 4, uint32_t>(in, out);
    if (v == "lds_8_u16") return sort_run<false, 8, uint16_t>(in, out);
    if (v == "lds_8_u32") return sort_run<false, 8, uint32_t>(in, out);
    fprintf(stderr, "unknown sort variant %s\n", v.c_str());
    return 2;
}

// ---- request / result files -----------------------------------------------------------------------------------------------------
static int read_arrays(const char* path, Arrays& a)
{
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n > 64) { fclose(f); return 2; }
    for (uint64_t i = 0; i < n; i++) {
        uint64_t nb = 0;
        if (fread(&nb, 8, 1, f) != 1 || nb > (1ull << 31)) { fclose(f); return 2; }
        a.emplace_back(nb);
        const uint64_t padded = (nb + 7) & ~7ull;
        std::vector<char> buf(padded);
        if (padded && fread(buf.data(), 1, padded, f) != padded) { fclose(f); return 2; }
        if (nb) memcpy(a.back().data(), buf.data(), nb);
    }
    fclose(f);
    return 0;
}
static int write_arrays(const char* path, const Arrays& a)
{
    FILE* f = fopen(path, "wb");
    if (!f) return 2;
    const uint64_t n = a.size(), zero = 0;
    bool ok = fwrite(&n, 8, 1, f) == 1;
    for (uint64_t i = 0; ok && i < n; i++) {
        const uint64_t nb = a[i].size(), pad = ((nb + 7) & ~7ull) - nb;
        ok = fwrite(&nb, 8, 1, f) == 1 && (nb == 0 || fwrite(a[i].data(), 1, nb, f) == nb) && (pad == 0 || fwrite(&zero, 1, pad, f) == pad);
    }
    return (fclose(f) == 0 && ok) ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s OP request.bin result.bin\n", argv[0]); return 2; }
    const std::string op = argv[1];
    Arrays in, out;
    if (read_arrays(argv[2], in)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    int rc;
    if (op == "fdiv") rc = op_div(0, in, out);
    else if (op == "fdiv_grid") rc = op_div_grid(in, out);
    else if (op == "frcp") rc = op_div(1, in, out);
    else if (op == "frsq") rc = op_div(2, in, out);
    else if (op == "fast_log2f") rc = op_log2f(in, out);
    else if (op == "plogp") rc = op_plogp(in, out);
    else if (op == "bin_pixel") rc = op_bin(0, in, out);
    else if (op == "bin_radiomix") rc = op_bin(1, in, out);
    else if (op == "bin_matlab") rc = op_bin(2, in, out);
    else if (op == "to_grayscale") rc = op_bin(3, in, out);
    else if (op == "i24") rc = op_i24(in, out);
    else if (op == "u24_su") rc = op_u24_su(in, out);
    else if (op == "med3") rc = op_med3(in, out);
    else if (op == "cnt16") rc = op_cnt16(in, out);
    else if (op == "rowcol_small") rc = op_rowcol_small(in, out);
    else if (op == "rowcol_walk") rc = op_rowcol_walk(false, in, out);
    else if (op == "rowcol_walk_small") rc = op_rowcol_walk(true, in, out);
    else if (op == "cloud") rc = op_cloud(in, out);
    else if (op == "wave") rc = op_wave(in, out);
    else if (op == "transpose4") rc = op_transpose(4, false, in, out);
    else if (op == "transpose8") rc = op_transpose(8, false, in, out);
    else if (op == "transpose8_u32") rc = op_transpose(8, true, in, out);
    else if (op == "transpose16") rc = op_transpose(16, false, in, out);
    else if (op == "transpose64") rc = op_transpose(64, false, in, out);
    else if (op.rfind("sort_", 0) == 0) rc = op_sort(op.substr(5), in, out);
    else { fprintf(stderr, "unknown op %s\n", op.c_str()); return 2; }
    if (rc) return rc;
    if (write_arrays(argv[3], out)) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    return 0;
}
