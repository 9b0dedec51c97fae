// moments_close.h -- the closing math of the 2-D geometric moments (Smoms2D_feature / Imoms2D_feature of the reference,
// features/2d_geomoments_basic.cpp:152-253): from the sums about the box centre to one 90-column block.  Shared by the per-ROI kernel
// (roi_moments.hip) and the whole-slide sweep (roi_wsgroup.hip), which differ only in how they gather the sums.  Device code only.
//
// Column layout of one 90-wide block (Feature2D order): RM(13) CM(16) NRM(16) NCM(7) HU(7) WRM(10) WCM(7) WNCM(7) WHU(7)
#pragma once
#include <hip/hip_runtime.h>

namespace nyxhip {

// (p, q) of the 10 weighted raw moments and of the 7 (weighted / normalized) central ones
struct MomPQ {
    static constexpr int wr_p[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3}, wr_q[10] = {0, 1, 2, 3, 0, 1, 2, 0, 1, 0};
    static constexpr int nc_p[7] = {0, 0, 1, 1, 2, 2, 3}, nc_q[7] = {2, 3, 1, 2, 0, 1, 0};
};

__device__ __forceinline__ double ipow(double a, int b) { double r = 1.0; for (int i = 0; i < b; i++) r *= a; return r; }

static __device__ void hu7(double _02, double _03, double _11, double _12, double _20, double _21, double _30, double* h)
{   // calcHu_imp, 2d_geomoments_basic.cpp:231-253
    h[0] = _20 + _02;
    h[1] = ipow((_20 - _02), 2) + 4 * (ipow(_11, 2));
    h[2] = ipow((_30 - 3 * _12), 2) + ipow((3 * _21 - _03), 2);
    h[3] = ipow((_30 + _12), 2) + ipow((_21 + _03), 2);
    h[4] = (_30 - 3 * _12) * (_30 + _12) * (ipow(_30 + _12, 2) - 3 * ipow(_21 + _03, 2)) +
           (3 * _21 - _03) * (_21 + _03) * (3 * ipow(_30 + _12, 2) - ipow(_21 + _03, 2));
    h[5] = (_20 - _02) * (ipow(_30 + _12, 2) - ipow(_21 + _03, 2)) + 4 * _11 * (_30 + _12) * (_21 + _03);
    h[6] = (3 * _21 - _03) * (_30 + _12) * (ipow(_30 + _12, 2) - 3 * ipow(_21 + _03, 2)) -
           (_30 - 3 * _12) * (_21 + _03) * (3 * ipow(_30 + _12, 2) - ipow(_21 + _03, 2));
}

// m[p][q] about the origin o - e from the sums mo[k * 4 + l] about o, by the binomial theorem (coefficients of orders 0..3):
//     m[p][q] = sum_{k <= p, l <= q} C(p, k) C(q, l) e_x^(p - k) e_y^(q - l) mo[k][l]
// (no local arrays: an array indexed at run time lives in scratch memory)
__device__ __forceinline__ double mom_shifted(const double* mo, int p, int q, double ex, double ey)
{
    auto binom = [](int n, int k) -> double { return (n == 3 && (k == 1 || k == 2)) ? 3.0 : (n == 2 && k == 1) ? 2.0 : 1.0; };
    auto pw = [](double e, int n) -> double { const double e2 = e * e; return n == 0 ? 1.0 : n == 1 ? e : n == 2 ? e2 : e2 * e; };
    double r = 0.0;
    for (int k = 0; k <= p; k++)
        for (int l = 0; l <= q; l++) r += binom(p, k) * binom(q, l) * pw(ex, p - k) * pw(ey, q - l) * mo[k * 4 + l];
    return r;
}

// The 90 columns of one variant at o from raw[16] / cen[16] (index p * 4 + q), wraw[10] (MomPQ::wr_*) and wcen[7] (MomPQ::nc_*):
// normalised moments (:204-225) and the two sets of Hu invariants.
__device__ __forceinline__ void mom_write_block(double* o, const double* raw, const double* cen, const double* wraw, const double* wcen)
{
    const double m00 = raw[0], w00 = wraw[0];
    // x / pow(m, (p + q) / 2 + 1) for p + q = 0..6: the seven powers are m^(1 + j/2) = m^(1 + j div 2) * sqrt(m)^(j mod 2) -- one
    // square root, a few products and seven divisions per normalising mass, where thirty pow() calls (a couple of hundred
    // instructions each, on two lanes of one wave) were a tenth of the kernel.  Tolerance-class values; 1-2 ulp from pow().
    double rm[7], rw[7];
    {
        const double sm = sqrt(m00), sw = sqrt(w00);
        double pm = m00, pw = w00;
#pragma unroll
        for (int j = 0; j < 7; j += 2) {
            rm[j] = 1.0 / pm; rw[j] = 1.0 / pw;
            if (j + 1 < 7) { rm[j + 1] = 1.0 / (pm * sm); rw[j + 1] = 1.0 / (pw * sw); }
            pm *= m00; pw *= w00;
        }
    }
    for (int k = 0; k < 13; k++) o[k] = raw[k];                                       // RM 00..23, 30
    for (int k = 0; k < 16; k++) o[13 + k] = cen[k];                                          // CM
#pragma unroll
    for (int k = 0; k < 16; k++)                                                               // NRM :204-209
        o[29 + k] = raw[k] * rm[(k >> 2) + (k & 3)];
    double nu[7], wn[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {                                                              // NCM :212-217
        nu[k] = cen[MomPQ::nc_p[k] * 4 + MomPQ::nc_q[k]] * rm[MomPQ::nc_p[k] + MomPQ::nc_q[k]];
        o[45 + k] = nu[k];
    }
    hu7(nu[0], nu[1], nu[2], nu[3], nu[4], nu[5], nu[6], o + 52);
    for (int k = 0; k < 10; k++) o[59 + k] = wraw[k];                                          // WRM
    for (int k = 0; k < 7; k++) o[69 + k] = wcen[k];                                           // WCM
#pragma unroll
    for (int k = 0; k < 7; k++) {                                                              // WNCM :220-225
        wn[k] = wcen[k] * rw[MomPQ::nc_p[k] + MomPQ::nc_q[k]];
        o[76 + k] = wn[k];
    }
    hu7(wn[0], wn[1], wn[2], wn[3], wn[4], wn[5], wn[6], o + 83);
}

} // namespace nyxhip
