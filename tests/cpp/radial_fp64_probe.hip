// radial_fp64_probe.hip -- TEST PROGRAM (tests/test_radial_gpu.py): the fp64 operation sequence that decides a ring of the radial
// distribution kernel (roi_radial.hip) -- sqrt, sqrt, divide, multiply by 7, truncate -- on caller-given integer pairs, built with
// the library's own flags.  in: n pairs of uint64 (d2, c2); out: per pair sqrt(d2), sqrt(d2) / sqrt(c2), the product, the ring.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

__global__ void probe(const uint64_t* in, double* out, uint64_t n)
{
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = sqrt((double)in[2 * i]), c = sqrt((double)in[2 * i + 1]);
    const double rat = a / c;
    const double t = rat * 7.0;
    int ring = (int)t;
    if (ring >= 8) ring = 7;
    out[4 * i] = a; out[4 * i + 1] = rat; out[4 * i + 2] = t; out[4 * i + 3] = (double)ring;
}

#define TRY(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n == 0 || n > (1ull << 26)) return 2;
    std::vector<uint64_t> in(2 * n);
    if (fread(in.data(), 8, 2 * n, f) != 2 * n) return 2;
    fclose(f);
    uint64_t* d_in; double* d_out;
    TRY(hipMalloc(&d_in, 16 * n));
    TRY(hipMalloc(&d_out, 32 * n));
    TRY(hipMemcpy(d_in, in.data(), 16 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
    TRY(hipGetLastError());
    std::vector<double> out(4 * n);
    TRY(hipMemcpy(out.data(), d_out, 32 * n, hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, 4 * n, f) != 4 * n) return 2;
    fclose(f);
    TRY(hipFree(d_in)); TRY(hipFree(d_out));
    return 0;
}
