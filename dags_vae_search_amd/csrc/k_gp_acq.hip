// Acquisition of the GP predictor for latent-space Bayesian optimisation (predictor.py: fit_posterior /
// expected_improvement; search.py).  One launch takes Q query latents x to
//   mean = c + k_x . alpha,   var = max(c0 + k_x^T P k_x, 0),   EI = (mean - best - xi) Phi(u) + sigma phi(u),
//   u = (mean - best - xi) / sigma,   k_x = [o exp(-|x - z_m|^2 / (2 l^2))]_m,
// and optionally dEI/dx = sum_m w_m k_m (z_m - x) / l^2 with w = Phi(u) alpha + phi(u) / sigma (P k_x).
// P (symmetric M x M) and alpha are solved once on the host side; they arrive as one row-major f64 matrix
// W = [P | alpha] [M][ld], so the mean falls out of the same contraction as P k_x.  Everything is fp64; the Q x M kernel
// matrix never leaves LDS.
//
// Decomposition: a workgroup (8 waves) owns 16 queries.
//   1. k block: Kt[m][q] (f64, m-major so one MFMA A fragment is 64 consecutive doubles) computed from the points into LDS.
//   2. First contraction Y = K W on v_mfma_f64_16x16x4_f64: the 16-column tiles of W are dealt round-robin to the waves
//      (tile t -> wave t % 8, at most 8 tiles a wave, so M + 1 <= 1024); the k dimension (m) runs over the whole block.
//      A fragment: lane l holds K[q = l & 15][m = 4s + (l >> 4)]; B fragment: W[m = 4s + (l >> 4)][n = 16t + (l & 15)];
//      C/D (the f64 map, NOT the f32 one): lane l, register r holds Y[q = (l >> 4) + 4r][n = 16t + (l & 15)].
//   3. Row dot products k_q . Y[q][0..M) and the alpha column Y[q][M]: per lane, then a fixed xor butterfly over the 16
//      lanes of a row group, then the 8 waves' partials added in wave order: bitwise reproducible.  16 threads finish
//      mean / sigma / EI and the two weights (Phi, phi / sigma) per query.
//   4. Gradient (optional): each wave overwrites ITS columns of Kt with w_qm k_qm (its Y tiles are still in registers),
//      then waves 0 .. ceil(D/16)-1 each contract one 16-wide slice of the dimensions: G = (w o K) Z on the same MFMA,
//      grad = (G - x s) / l^2 with s = sum_m w_m k_m = Phi (mean - c) + phi / sigma k^T P k.
// sigma <= 1e-12 o: EI = max(imp, 0) and the gradient is d mean / dx where imp > 0, else 0.
#include "dvs_search_args.h"

typedef double dvs_d4 __attribute__((ext_vector_type(4)));

constexpr int GPA_Q = 16;                             // queries per workgroup: the MFMA's row block
constexpr int GPA_WAVES = 8;
constexpr int GPA_THREADS = GPA_WAVES * 64;
constexpr int GPA_TPW = 8;                            // column tiles of W a wave holds in registers (8 x 4 f64 = 64 VGPRs)
constexpr int GPA_MAX_COLS = GPA_WAVES * GPA_TPW * 16;
constexpr int GPA_MAX_M = GPA_MAX_COLS - 1;           // M columns of P + the alpha column
static_assert(GPA_MAX_M == DVS_GP_ACQ_MAX_INDUCING, "include/dvs.h");
constexpr int GPA_MAXD = 32;
constexpr int GPA_MAX_MP = (GPA_MAX_M + 3) / 4 * 4;   // k dimension padded to the MFMA's K = 4
// LDS: Kt [Mp][16] | xs [16][32] | red [2][8][16] | coef [3][16]  (doubles)
constexpr size_t gpa_lds_doubles(int Mp) { return (size_t)Mp * GPA_Q + GPA_Q * GPA_MAXD + 2 * GPA_WAVES * GPA_Q + 3 * GPA_Q; }
static_assert(gpa_lds_doubles(GPA_MAX_MP) * 8 <= 160 * 1024, "k block of the largest M must fit one CU's LDS");
// Registers: 2 workgroups of 8 waves per CU (LDS 70.5 KB each at M = 500) = 4 waves per SIMD = 128 VGPRs a lane.  The
// arrays that live across the k loop are the accumulators (GPA_TPW tiles x 4 f64 = 8 VGPRs each) and the current and
// prefetched B fragments (2 x GPA_TPW f64); at least 32 VGPRs stay for addresses, the A fragment and loop state.
constexpr int GPA_VGPR_BUDGET = 128;
constexpr int GPA_VGPR_ARRAYS = GPA_TPW * 4 * 2 + 2 * GPA_TPW * 2;
static_assert(GPA_VGPR_ARRAYS + 32 <= GPA_VGPR_BUDGET, "accumulators + B fragments must leave room at 4 waves per SIMD");
static_assert(GPA_MAXD <= 2 * 16, "gradient: one wave per 16 dimensions, at most 2 slices");
static_assert(GPA_MAXD / 16 <= GPA_WAVES, "gradient slices need a wave each");

__global__ __launch_bounds__(GPA_THREADS, 2) void k_gp_acquire(GpAcqArgs a) {
    extern __shared__ double gpa_lds[];
    double* Kt = gpa_lds;                                   // [Mp][16]
    double* xs = Kt + (size_t)a.Mp * GPA_Q;                 // [16][32]
    double* red = xs + GPA_Q * GPA_MAXD;                    // [2][8][16]
    double* coef = red + 2 * GPA_WAVES * GPA_Q;             // [3][16]: Phi weight, phi / sigma weight, s
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * GPA_Q;
    const int qc = lane & 15, kr = lane >> 4;               // A-fragment row / k slot; C-fragment column / row group

    for (int i = tid; i < GPA_Q * GPA_MAXD; i += GPA_THREADS) {
        const int q = i / GPA_MAXD, d = i - q * GPA_MAXD;
        xs[i] = (q0 + q < a.Q && d < a.D) ? (double)a.x[(size_t)(q0 + q) * a.D + d] : 0.0;
    }
    __syncthreads();
    // 1. k block (padded queries and padded m give 0: they add nothing to any contraction)
    for (int i = tid; i < a.Mp * GPA_Q; i += GPA_THREADS) {
        const int m = i >> 4, q = i & 15;
        double k = 0.0;
        if (m < a.M && q0 + q < a.Q) {
            const float* zm = a.z + (size_t)m * a.D;
            const double* xq = xs + q * GPA_MAXD;
            double d2 = 0.0;
            for (int d = 0; d < a.D; ++d) {
                const double t = (double)zm[d] - xq[d];
                d2 = fma(t, t, d2);
            }
            k = a.outputscale * exp(-d2 * a.inv2l2);
        }
        Kt[i] = k;
    }
    __syncthreads();

    // 2. Y = K W for this wave's column tiles t = wave + 8 j
    dvs_d4 acc[GPA_TPW];
#pragma unroll
    for (int j = 0; j < GPA_TPW; ++j) acc[j] = dvs_d4{0.0, 0.0, 0.0, 0.0};
    // The B fragments come from L2 (W is 2 MB at M = 500, read by every workgroup): the next k step's fragments are
    // loaded before this step's MFMAs are issued, so one L2 round trip overlaps a k step of MFMAs.
    const int ncols = a.M + 1;
    const int nsteps = a.Mp / 4;
    double bn[GPA_TPW];
    auto load_b = [&](int s, double* b) {
        const int m = 4 * s + kr;
        const double* wrow = a.W + (size_t)m * a.ld;
#pragma unroll
        for (int j = 0; j < GPA_TPW; ++j) {
            const int n = 16 * (wave + GPA_WAVES * j) + qc;
            b[j] = (m < a.M && n < ncols) ? wrow[n] : 0.0;
        }
    };
    load_b(0, bn);
    for (int s = 0; s < nsteps; ++s) {
        double bc[GPA_TPW];
#pragma unroll
        for (int j = 0; j < GPA_TPW; ++j) bc[j] = bn[j];
        if (s + 1 < nsteps) load_b(s + 1, bn);
        const double av = Kt[(4 * s + kr) * GPA_Q + qc];
#pragma unroll
        for (int j = 0; j < GPA_TPW; ++j) {
            if (wave + GPA_WAVES * j < a.NT)                    // wave-uniform
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bc[j], acc[j], 0, 0, 0);
        }
    }

    // 3. row dot products: quad[q] = sum_{n < M} K[q][n] Y[q][n], lin[q] = Y[q][M]
    double qp[4] = {0.0, 0.0, 0.0, 0.0}, lp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < GPA_TPW; ++j) {
        const int t = wave + GPA_WAVES * j;
        if (t < a.NT) {
            const int n = 16 * t + qc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = kr + 4 * r;
                if (n < a.M) qp[r] = fma(Kt[n * GPA_Q + q], acc[j][r], qp[r]);
                else if (n == a.M) lp[r] += acc[j][r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
            qp[r] += dvs_shfl_xor(qp[r], lane, s);
            lp[r] += dvs_shfl_xor(lp[r], lane, s);
        }
        if (qc == 0) {
            red[wave * GPA_Q + kr + 4 * r] = qp[r];
            red[(GPA_WAVES + wave) * GPA_Q + kr + 4 * r] = lp[r];
        }
    }
    __syncthreads();
    if (tid < GPA_Q) {
        const int q = tid;
        double quad = 0.0, lin = 0.0;
        for (int w = 0; w < GPA_WAVES; ++w) {
            quad += red[w * GPA_Q + q];
            lin += red[(GPA_WAVES + w) * GPA_Q + q];
        }
        const double mu = a.constant + lin;
        const double v = fmax(a.c0 + quad, 0.0);
        const double sig = sqrt(v);
        const double imp = mu - a.best - a.xi;
        double e, wa, wp;
        if (sig > a.sig_floor) {
            const double u = imp / sig;
            const double Phi = 0.5 * erfc(-u * 0.70710678118654752440);
            const double phi = 0.39894228040143267794 * exp(-0.5 * u * u);
            e = imp * Phi + sig * phi;
            wa = Phi;
            wp = phi / sig;
        } else {
            e = fmax(imp, 0.0);
            wa = imp > 0.0 ? 1.0 : 0.0;
            wp = 0.0;
        }
        coef[q] = wa;
        coef[GPA_Q + q] = wp;
        coef[2 * GPA_Q + q] = wa * lin + wp * quad;
        if (q0 + q < a.Q) {
            a.mean[q0 + q] = mu;
            a.var[q0 + q] = v;
            a.ei[q0 + q] = e;
        }
    }
    if (a.grad == nullptr) return;                              // uniform over the launch
    __syncthreads();

    // 4. gradient: Kt[n][q] <- (Phi_q alpha_n + phi_q / sigma_q Y[q][n]) K[q][n] on this wave's own columns
#pragma unroll
    for (int j = 0; j < GPA_TPW; ++j) {
        const int t = wave + GPA_WAVES * j;
        if (t < a.NT) {
            const int n = 16 * t + qc;
            if (n < a.M) {
                const double al = a.W[(size_t)n * a.ld + a.M];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = kr + 4 * r;
                    Kt[n * GPA_Q + q] *= fma(coef[q], al, coef[GPA_Q + q] * acc[j][r]);
                }
            }
        }
    }
    __syncthreads();
    if (wave * 16 < a.D) {
        const int d = wave * 16 + qc;
        dvs_d4 g = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < a.Mp / 4; ++s) {
            const int m = 4 * s + kr;
            const double av = Kt[m * GPA_Q + qc];
            const double bv = (m < a.M && d < a.D) ? (double)a.z[(size_t)m * a.D + d] : 0.0;
            g = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, g, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = kr + 4 * r;
            if (q0 + q < a.Q && d < a.D)
                a.grad[(size_t)(q0 + q) * a.D + d] = (float)((g[r] - xs[q * GPA_MAXD + d] * coef[2 * GPA_Q + q]) * a.inv_l2);
        }
    }
}

void dvs_launch_gp_acquire(const GpAcqArgs& in, double lengthscale, dvs_stream_t st) {
    GpAcqArgs a = in;
    a.Mp = (a.M + 3) / 4 * 4;
    a.NT = (a.M + 1 + 15) / 16;
    a.inv2l2 = dvs_gp_inv2l2(lengthscale);
    a.inv_l2 = dvs_gp_inv_l2(lengthscale);
    a.sig_floor = 1e-12 * a.outputscale;
    const size_t lds = gpa_lds_doubles(a.Mp) * sizeof(double);
    DVS_SET_LDS(k_gp_acquire, lds);
    DVS_LAUNCH(k_gp_acquire, dim3((unsigned)((a.Q + GPA_Q - 1) / GPA_Q)), dim3(GPA_THREADS), lds, st, a);
}
