// Conditional-independence tests on real-valued data: cor, zf and mi-g from the moments of dvs_gaussian.h.
// Included by k_bic.hip after dvs_gaussian.h.  Semantics, operation orders and refusals: include/dvs_gaussian_ci.h.
//
//   k_gbn_ci         one lane per test (x, y | Z), 64-lane workgroups.  The lane factors C[Z, x, y] row by row into its slice of
//                    static LDS (the stride-by-lane layout of gbn_L: consecutive lanes in consecutive banks), reads r and 1 - r^2
//                    off the last row and takes the tail.  gci_factor_row is gbn_factor_row with the row's and the columns'
//                    variables given by the test order (Z ascending, x, y) instead of a parent mask; gbn_factor_row and the
//                    kernels that call it are left as they are.
//   k_gbn_ci_group   one lane per (target, conditioning set) group: gci_base factors Z and the target once, gci_append puts one
//                    row per candidate into the same last slot, O(k^2) a candidate where k_gbn_ci pays O(k^3).  Both kernels
//                    go through gci_base and gci_append, so a grouped cell is the per-test kernel's bytes.
//
// Plain fp64 vector arithmetic, contraction off in every function that rounds (the tails included: the two kernels inline
// them separately and promise equal bytes); status by the integer atomicOr of the scorer.
#pragma once
#include "dvs_citest.h"              // next to ci_gamma_q
#include "dvs_gaussian.h"

static_assert(DVS_GCI_MAX_COND + 2 <= DVS_GBN_MAX_PARENTS + 1, "Z, x and y fit the lane's factor slice");

// ---------------------------------------------------------------------------------------------------------
// I_x(a, b), the regularised incomplete beta function, xc = 1 - x given by the caller (here r^2, which is not 1 - x rounded):
// a modified Lentz evaluation of the continued fraction, on (a, b, x) below the switch point (a + 1) / (a + b + 2) and as
// 1 - I_xc(b, a) above it.  The lead factor goes through bn_lgamma: lgamma(a + b) - lgamma(a) loses a few ulp of lgamma(a + b),
// which is what bounds the relative accuracy at large a (include/dvs_gaussian_ci.h).
// ---------------------------------------------------------------------------------------------------------
constexpr int CI_BETA_ITER = 20000;         // O(sqrt(max(a, b))) steps are needed; 38 were the most seen up to a = 32 768

__device__ inline double ci_beta_i(double a, double b, double x, double xc) {
#pragma clang fp contract(off)
    if (!(x > 0.0)) return 0.0;
    if (!(xc > 0.0)) return 1.0;
    const double lead = exp(bn_lgamma(a + b) - bn_lgamma(a) - bn_lgamma(b) + a * log(x) + b * log(xc));
    const bool mirror = !(x < (a + 1.0) / (a + b + 2.0));
    if (mirror) {
        const double t = a;
        a = b;
        b = t;
        x = xc;
    }
    const double tiny = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int i = 1; i <= CI_BETA_ITER; ++i) {
        const double m = (double)i, m2 = 2.0 * m;
        double an = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + an * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        an = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + an * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-15) break;
    }
    const double v = lead * h / a;
    return mirror ? 1.0 - v : v;
}

// the two erfc tails: two-sided normal for Fisher's z, chi-square with one degree of freedom for mi-g
__device__ __forceinline__ double ci_normal_two_sided(double z) {
#pragma clang fp contract(off)
    return erfc(fabs(z) / 1.4142135623730951);
}
__device__ __forceinline__ double ci_chisq1_upper(double s) {
#pragma clang fp contract(off)
    return erfc(sqrt(s / 2.0));
}

// ---------------------------------------------------------------------------------------------------------
// One test
// ---------------------------------------------------------------------------------------------------------
// Row i of the factor for variable ai; column j < i belongs to the j-th member of zm for j < k and to xv for j = k.  Returns the
// squared pivot; the caller checks it before the next row reads L[i][i].
__device__ __forceinline__ double gci_factor_row(const double* C, int n, uint64_t zm, int k, int xv, int i, int ai, double* L, double* diag) {
#pragma clang fp contract(off)
    uint64_t mj = zm;
    for (int j = 0; j < i; ++j) {
        int aj = xv;
        if (j < k) {
            aj = dvs_ctz64(mj);
            mj &= mj - 1ull;
        }
        double s = C[ai * n + aj];
        for (int t = 0; t < j; ++t) {
            const double prod = gbn_L(L, i, t) * gbn_L(L, j, t);
            s = s - prod;
        }
        gbn_L(L, i, j) = s / gbn_L(L, j, j);
    }
    double s = C[ai * n + ai];
    *diag = s;
    for (int t = 0; t < i; ++t) {
        const double prod = gbn_L(L, i, t) * gbn_L(L, i, t);
        s = s - prod;
    }
    gbn_L(L, i, i) = sqrt(s);
    return s;
}

// What a test needs before y: the ranges, k, the degrees of freedom, and rows 0 .. k of the factor (Z ascending, then x) in L.
// Returns k, or -1 for a refusal.
__device__ __forceinline__ int gci_base(const double* mom, int n, int type, int xv, uint64_t zm, double* L) {
#pragma clang fp contract(off)
    if (xv < 0 || xv >= n || (zm >> n) != 0ull || ((zm >> xv) & 1ull)) return -1;
    const int k = __popcll(zm);
    if (k > DVS_GCI_MAX_COND) return -1;
    if (mom[0] - (double)k - (type == DVS_GCI_ZF ? 3.0 : 2.0) < 1.0) return -1;
    const double* C = mom + 1 + n;
    double diag;
    uint64_t mi = zm;
    for (int i = 0; i < k; ++i, mi &= mi - 1ull) {
        const double d2 = gci_factor_row(C, n, zm, k, xv, i, dvs_ctz64(mi), L, &diag);
        if (!gbn_pivot_ok(d2, diag, k + 1)) return -1;
    }
    const double d2 = gci_factor_row(C, n, zm, k, xv, k, xv, L, &diag);
    return gbn_pivot_ok(d2, diag, k + 1) ? k : -1;
}

// Row k + 1 for y behind a base that succeeded, then the cells (statistic, df, p-value); false for a refusal (cells not written).
__device__ __forceinline__ bool gci_append(const double* mom, int n, int type, int xv, uint64_t zm, int k, int yv, double* L, double* out) {
#pragma clang fp contract(off)
    if (yv < 0 || yv >= n || yv == xv || ((zm >> yv) & 1ull)) return false;
    double diag;
    const double d2 = gci_factor_row(mom + 1 + n, n, zm, k, xv, k + 1, yv, L, &diag);
    if (!gbn_pivot_ok(d2, diag, k + 1)) return false;
    const double m = mom[0], l = gbn_L(L, k + 1, k);
    const double ll = l * l;
    const double q = ll + d2;
    const double r = l / sqrt(q);
    const double omr = d2 / q;
    if (type == DVS_GCI_COR) {
        const double df = m - (double)k - 2.0;
        out[0] = r * sqrt(df / omr);
        out[1] = df;
        out[2] = ci_beta_i(0.5 * df, 0.5, omr, ll / q);
    } else if (type == DVS_GCI_ZF) {
        const double df = m - (double)k - 3.0;
        const double z = (0.5 * log((1.0 + r) / (1.0 - r))) * sqrt(df);
        out[0] = z;
        out[1] = df;
        out[2] = ci_normal_two_sided(z);
    } else {
        const double s = -m * log(omr);
        out[0] = s;
        out[1] = 1.0;
        out[2] = ci_chisq1_upper(s);
    }
    return true;
}

__device__ __forceinline__ void gci_refuse(double* out) {
    out[0] = bn_nan();
    out[1] = bn_nan();
    out[2] = bn_nan();
}

__global__ __launch_bounds__(GBN_LANES) void k_gbn_ci(GbnCiArgs a) {
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const long long t = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (t >= (long long)a.T) return;
    double* L = s_L + threadIdx.x;
    const double* mom = a.moments + (size_t)(a.set_of != nullptr ? a.set_of[t] : 0) * DVS_GBN_STRIDE(a.n);
    const int xv = a.pairs[2 * t], yv = a.pairs[2 * t + 1];
    const uint64_t zm = a.cond[t];
    double* out = a.out + 3 * t;
    const int k = gci_base(mom, a.n, a.type, xv, zm, L);
    if (k < 0 || !gci_append(mom, a.n, a.type, xv, zm, k, yv, L, out)) {
        atomicOr(a.status, 16);
        gci_refuse(out);
    }
}

void dvs_launch_gbn_ci(const GbnCiArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_gbn_ci, dim3((unsigned)((a.T + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, a);
}

__global__ __launch_bounds__(GBN_LANES) void k_gbn_ci_group(GbnCiGroupArgs a) {
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const long long g = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (g >= (long long)a.G) return;
    double* L = s_L + threadIdx.x;
    const int n = a.n;
    const double* mom = a.moments + (size_t)(a.set_of != nullptr ? a.set_of[g] : 0) * DVS_GBN_STRIDE(n);
    const int xv = a.target[g];
    const uint64_t zm = a.cond[g], asked = a.candidates[g] & ((1ull << n) - 1ull);          // n <= 48
    double* out = a.out + (size_t)g * n * 3;
    const int k = asked != 0ull ? gci_base(mom, n, a.type, xv, zm, L) : -1;
    bool refused = false;
    for (int c = 0; c < n; ++c) {
        if (((asked >> c) & 1ull) && k >= 0 && gci_append(mom, n, a.type, xv, zm, k, c, L, out + 3 * c)) continue;
        refused = refused || ((asked >> c) & 1ull);
        gci_refuse(out + 3 * c);
    }
    if (refused) atomicOr(a.status, 16);
}

void dvs_launch_gbn_ci_group(const GbnCiGroupArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_gbn_ci_group, dim3((unsigned)((a.G + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, a);
}
