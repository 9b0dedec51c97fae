"""A restatement of the reference's IntensityHistogramFeatures (features/intensity_histogram.cpp:29-325) in Python floats: the 46 IH_*
values of every ROI of a host batch.  Sequential fp64 loops over the bins, in bin order, like the reference; Python's float arithmetic is
IEEE double without contraction, so every column but the two that go through log() carries the reference's bits.  The histogram itself is
the reference's binning expression evaluated by numpy over the ROI's pixels."""
import math

import numpy as np

_STATS = ["MEAN", "VARIANCE", "SKEWNESS", "EXCESS_KURTOSIS", "MEDIAN", "MINIMUM", "P10", "P90", "MAXIMUM", "MODE", "INTERQUANTILE_RANGE", "RANGE",
          "MEAN_ABSOLUTE_DEVIATION", "ROBUST_MEAN_ABSOLUTE_DEVIATION", "MEDIAN_ABSOLUTE_DEVIATION", "COEFFICIENT_OF_VARIATION",
          "QUANTILE_COEFFICIENT_OF_DISPERSION", "ENTROPY", "UNIFORMITY"]
NAMES = (["IH_%s_VAL" % k for k in _STATS] + ["IH_ROBUST_MEAN_VAL"] + ["IH_%s_IDX" % k for k in _STATS]
         + ["IH_MAX_GRADIENT", "IH_MAX_GRADIENT_IDX", "IH_MIN_GRADIENT", "IH_MIN_GRADIENT_IDX", "IH_ROBUST_MEAN_IDX", "IH_NUM_BINS", "IH_BIN_SIZE"])
ENTROPY = ["IH_ENTROPY_VAL", "IH_ENTROPY_IDX"]                # through log(): equal to rounding (parity.REL_TOL)
EXACT = [n for n in NAMES if n not in ENTROPY]                # bit for bit
DBL_MIN = 2.2250738585072014e-308                             # numeric_limits<double>::min(): the seed of IH_MAX_GRADIENT
DBL_MAX = 1.7976931348623157e308
INT_MIN = -2 ** 31


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _to_int(q):
    """(int) of a double as x86-64 converts it: INT_MIN for NaN and for whatever lies outside int."""
    if q != q or q in (math.inf, -math.inf) or not (-2147483648.0 <= q < 2147483648.0):
        return INT_MIN
    return int(q)


def counts(inten, mn, mx, N):
    """The N bin counts: idx = (int) floor((v - mn) / binWidth), clamped to [0, N - 1]."""
    bw = (float(mx) - float(mn)) / float(N)
    q = np.floor((np.asarray(inten, np.float64) - float(mn)) / bw)
    idx = np.clip(q, 0, N - 1).astype(np.int64)
    return np.bincount(idx, minlength=N).astype(np.int64)


def roi_values(inten, mn, mx, N, ibsi, soft_nan):
    cnt = len(inten)
    if not ibsi or mx <= mn or N < 2 or cnt == 0:
        return [float(soft_nan)] * 46
    mn, mx = float(mn), float(mx)
    bw = (mx - mn) / float(N)
    freq = [float(c) for c in counts(inten, mn, mx, N)]
    tot = float(cnt)

    def bin_min(i):
        return mn + float(i) * bw

    def bin_max(i):
        return mn + float(i + 1) * bw

    def bin_center(i):
        return mn + (float(i) + 0.5) * bw

    def index_of(v):
        q = _div(v - mn, bw)
        idx = _to_int(math.floor(q)) if q == q and q not in (math.inf, -math.inf) else INT_MIN
        return min(max(idx, 0), N - 1)

    def quantile(p):
        cumulated, p_n_prev, f_n = 0.0, 0.0, 0.0
        if p < 0.5:
            n, p_n = 0, 0.0
            while True:
                f_n = freq[n]
                cumulated += f_n
                p_n_prev = p_n
                p_n = cumulated / tot
                n += 1
                if not (n < N and p_n < p):
                    break
            prop = f_n / tot
            lo, hi = bin_min(n - 1), bin_max(n - 1)
            return lo + _div(p - p_n_prev, prop) * (hi - lo)
        n, m, p_n = N - 1, 0, 1.0
        while True:
            f_n = freq[n]
            cumulated += f_n
            p_n_prev = p_n
            p_n = 1.0 - cumulated / tot
            n -= 1
            m += 1
            if not (m < N and p_n > p):
                break
        prop = f_n / tot
        lo, hi = bin_min(n + 1), bin_max(n + 1)
        return hi - _div(p_n_prev - p, prop) * (hi - lo)

    total, half, b = 0.0, float(cnt // 2), 0
    while total <= half and b < N:
        total += freq[b]
        b += 1
    med_v = bin_center(b - 1)
    med_i = index_of(med_v)
    min_i, max_i = index_of(mn), index_of(mx)
    p10_v, p25_v, p75_v, p90_v = quantile(0.10), quantile(0.25), quantile(0.75), quantile(0.90)
    p10_i, p25_i, p75_i, p90_i = index_of(p10_v), index_of(p25_v), index_of(p75_v), index_of(p90_v)

    mean_v = mean_i = rmean_v = rmean_i = rcount = 0.0
    for i in range(N):
        f = freq[i]
        prob = f / tot
        vv = bin_center(i)
        mean_v += prob * vv
        mean_i += prob * float(i)
        if p10_i <= i <= p90_i:
            rmean_v += f * vv
            rmean_i += f * float(i)
            rcount += f
    rmean_v = _div(rmean_v, rcount)
    rmean_i = _div(rmean_i, rcount)

    var_v = var_i = skew_v = skew_i = kurt_v = kurt_i = 0.0
    mode_v = mode_i = mode_f = 0.0
    mad_v = mad_i = rmad_v = rmad_i = medad_v = medad_i = 0.0
    ent = uni = 0.0
    gmax, gmax_i, gmin, gmin_i = DBL_MIN, 0.0, DBL_MAX, 0.0
    log2 = math.log(2.0)
    for i in range(N):
        f = freq[i]
        prob = f / tot
        vv = bin_center(i)
        dv = vv - mean_v
        di = float(i) - mean_i
        var_v += prob * dv * dv
        var_i += prob * di * di
        skew_v += prob * dv * dv * dv
        skew_i += prob * di * di * di
        kurt_v += prob * dv * dv * dv * dv
        kurt_i += prob * di * di * di * di
        if mode_f < f:
            mode_f, mode_v, mode_i = f, vv, float(i)
        mad_v += prob * abs(dv)
        mad_i += prob * abs(di)
        if p10_i <= i <= p90_i:
            rmad_v += f * abs(vv - rmean_v)
            rmad_i += f * abs(float(i) - rmean_i)
        medad_v += prob * abs(vv - med_v)
        medad_i += prob * abs(float(i) - float(med_i))
        if prob > 0.0000001:
            ent -= prob * math.log(prob) / log2
        uni += prob * prob
        if i == 0:
            g = freq[1] - freq[0]
        elif i == N - 1:
            g = freq[i] - freq[i - 1]
        else:
            g = (freq[i + 1] - freq[i - 1]) / 2.0
        if g > gmax:
            gmax, gmax_i = g, float(i + 1)
        if g < gmin:
            gmin, gmin_i = g, float(i + 1)

    skew_v = _div(skew_v, var_v * math.sqrt(var_v))
    skew_i = _div(skew_i, var_i * math.sqrt(var_i))
    kurt_v = _div(kurt_v, var_v * var_v) - 3
    kurt_i = _div(kurt_i, var_i * var_i) - 3
    cov_v = _div(math.sqrt(var_v), mean_v)
    cov_i = _div(math.sqrt(var_i), mean_i + 1)
    qcod_v = _div(p75_v - p25_v, p75_v + p25_v)
    qcod_i = _div(float(p75_i) - float(p25_i), float(p75_i) + 1.0 + float(p25_i) + 1.0)
    rmad_v = _div(rmad_v, rcount)
    rmad_i = _div(rmad_i, rcount)
    return [mean_v, var_v, skew_v, kurt_v, med_v, mn, p10_v, p90_v, mx, mode_v, p75_v - p25_v, mx - mn, mad_v, rmad_v, medad_v, cov_v, qcod_v,
            ent, uni, rmean_v,
            mean_i + 1, var_i, skew_i, kurt_i, float(med_i) + 1, float(min_i) + 1, float(p10_i) + 1, float(p90_i) + 1, float(max_i) + 1,
            mode_i + 1, float(p75_i) - float(p25_i), float(max_i) - float(min_i), mad_i, rmad_i, medad_i, cov_i, qcod_i, ent, uni,
            gmax, gmax_i, gmin, gmin_i, rmean_i + 1, float(N), bw]


def table(b, s):
    """[n_roi x 46] of a host batch under settings s (grey_depth, ibsi, soft_nan).  NaN / inf are left in place."""
    out = np.empty((b.n_roi, 46))
    for r in range(b.n_roi):
        o, e = int(b.px_offset[r]), int(b.px_offset[r + 1])
        out[r] = roi_values(b.inten[o:e], int(b.min_inten[r]), int(b.max_inten[r]), int(s.grey_depth), int(s.ibsi), float(s.soft_nan))
    return out


def same(a, b):
    """Elementwise: equal, or both NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))
