// What the kernels of the three kinds of fitted network share: dvs_params.h (discrete), dvs_gaussian_params.h
// (Gaussian) and dvs_mixed_params.h (conditional Gaussian) include it.  The byte identities between the families (an
// all-continuous CG network gives the Gaussian entry points' bytes, every log-likelihood ends in dvs_bn_loglik's tree, a sampled
// row is a function of (seed, row)) hold because each piece below has one definition; k_gbn_sample alone repeats the text of
// the noise draw and of the store, for its speed.  Everything is forced inline but k_bn_loglik_sum and its launcher; contraction
// is off in every function that rounds.
#pragma once
#include "dvs_bn_common.h"

// ---- the topological order ------------------------------------------------------------------------------------------------
// order[0 .. n): the lowest variable whose parents are all placed, n times.  par(v) is Pa(v) as a mask with the self bit and
// every bit >= n off.  One thread calls it; false: a cycle (status bit 0 at every caller), order[] is then not to be read.
template <class Par>
__device__ __forceinline__ bool fit_order(const int n, Par&& par, int* order) {
    uint64_t placed = 0ull;
    for (int k = 0; k < n; ++k) {
        int pick = -1;
        for (int v = 0; v < n && pick < 0; ++v)
            if (!((placed >> v) & 1ull) && !(par(v) & ~placed)) pick = v;
        if (pick < 0) return false;
        order[k] = pick;
        placed |= 1ull << pick;
    }
    return true;
}

// ---- the image of 256 rows in LDS: column c of row r at x[c * GPAR_LD + r] ----------------------------------------------
constexpr int GPAR_ROWS = 256;                               // rows of a workgroup's image = dvs_bn_loglik's chunk
constexpr int GPAR_LD = GPAR_ROWS + 1;                       // odd stride: the staging writes of a 16-lane group hit 16 bank pairs

inline size_t gpar_image_lds(int cols) { return (size_t)GPAR_LD * cols * sizeof(double); }

__device__ __forceinline__ int fit_chunk_len(long long rows, int chunk) {
    const long long left = rows - (long long)chunk * GPAR_ROWS;
    return left < GPAR_ROWS ? (int)left : GPAR_ROWS;
}
// stages rows 256 chunk .. of src [rows][cols] into the image; returns the rows it holds.  Every thread calls it; a barrier follows.
__device__ __forceinline__ int fit_image_load(const double* src, long long rows, int cols, int chunk, double* x) {
    const int len = fit_chunk_len(rows, chunk);
    src += (size_t)chunk * GPAR_ROWS * cols;
    for (int e = threadIdx.x; e < len * cols; e += blockDim.x) {
        const int r = e / cols, c = e - r * cols;
        x[c * GPAR_LD + r] = src[e];
    }
    __syncthreads();
    return len;
}
// the reverse for the image's first len rows, contiguously (element e of the chunk by thread e mod 256).  Every thread calls it; a
// barrier comes first.  Every caller of the two launches GPAR_ROWS threads; the load strides by blockDim.x and the store by the
// constant, as the code they replace did, so that the kernels keep the instructions they had (k_gbn_sample holds this text itself).
__device__ __forceinline__ void fit_image_store(double* dst, int len, int cols, int chunk, const double* x) {
    dst += (size_t)chunk * GPAR_ROWS * cols;
    __syncthreads();
    for (int e = threadIdx.x; e < len * cols; e += GPAR_ROWS) {
        const int r = e / cols, c = e - r * cols;
        dst[e] = x[c * GPAR_LD + r];
    }
}

// ---- the quantile function: Wichura's AS 241, PPND16, on u = (k + 0.5) 2^-52 ------------------------------------------------
__device__ __forceinline__ double gpar_horner(const double* p, double r) {
#pragma clang fp contract(off)
    double t = p[7];
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        t = t * r;
        t = t + p[i];
    }
    return t;
}

__device__ __forceinline__ double gpar_quantile(uint64_t k) {
#pragma clang fp contract(off)
    const double A[8] = {3.3871328727963666080, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                         4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3};
    const double Bq[8] = {1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
                          3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3};
    const double C[8] = {1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
                         1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4};
    const double D[8] = {1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
                         1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9};
    const double E[8] = {6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
                         2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7};
    const double F[8] = {1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
                         1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15};
    if (k >= (1ull << 52)) return bn_nan();
    const double scale = 2.220446049250313e-16;              // 2^-52
    const double u = ((double)k + 0.5) * scale, uc = ((double)((1ull << 52) - 1ull - k) + 0.5) * scale;
    const double q = u - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = q * gpar_horner(A, r);
        return num / gpar_horner(Bq, r);
    }
    const double p = u < uc ? u : uc;
    double r = sqrt(-log(p)), z;
    if (r <= 5.0) {
        r = r - 1.6;
        z = gpar_horner(C, r) / gpar_horner(D, r);
    } else {
        r = r - 5.0;
        z = gpar_horner(E, r) / gpar_horner(F, r);
    }
    return q < 0.0 ? -z : z;
}

// the standard normal draw of variable v in the row of `key`: two counter-based draws make the 52-bit k
__device__ __forceinline__ double fit_noise(uint32_t key, int v) {
    const uint32_t h1 = dvs_draw(key, 2u * (uint32_t)v), h2 = dvs_draw(key, 2u * (uint32_t)v + 1u);
    return gpar_quantile(((uint64_t)(h1 >> 6) << 26) + (uint64_t)(h2 >> 6));
}

// ---- the Gaussian log-density -----------------------------------------------------------------------------------------------
// c of a node: log(sd) + log(sqrt(2 pi))
__device__ __forceinline__ double fit_log_norm(double sd) {
#pragma clang fp contract(off)
    return log(sd) + 0.9189385332046727;
}
// term + log N(x; mu, sd), in the order of include/dvs_gaussian_params.h
__device__ __forceinline__ double fit_log_density(double term, double x, double mu, double sd, double c) {
#pragma clang fp contract(off)
    const double e = (x - mu) / sd;
    const double half = 0.5 * (e * e);
    return term - (c + half);
}

// ---- the exact prediction: the target given its Markov blanket ----------------------------------------------------------------
// In: pred = mu of the target, s = its variance.  child(c, beta, sd_c, res) says whether c is a child of the target to count and,
// if so, gives its coefficient on the target, its sd and its residual with the target's term left out.  Out: pred, var.
template <class Child>
__device__ __forceinline__ void fit_blanket(const int n, const double s, double& pred, double& var, Child&& child) {
#pragma clang fp contract(off)
    double prec = 1.0 / s;
    double num = pred * prec;
    for (int c = 0; c < n; ++c) {
        double beta, sdc, res;
        if (!child(c, beta, sdc, res)) continue;
        const double w = beta / (sdc * sdc);
        const double wr = w * res;
        num = num + wr;
        const double bw = beta * w;
        prec = prec + bw;
    }
    pred = num / prec;
    var = 1.0 / prec;
}

// ---- dvs_bn_loglik's two levels ---------------------------------------------------------------------------------------------
// the fixed tree over the workgroup's 256 terms into *partial.  Every thread calls it; a barrier separates two calls.
__device__ __forceinline__ void fit_chunk_sum(double term, double* partial) {
    __shared__ double red[GPAR_ROWS];
    const int tid = threadIdx.x;
    red[tid] = term;
    __syncthreads();
    dvs_block_sum256(tid, red);
    if (tid == 0) *partial = red[0];
}

// one workgroup per structure: thread t adds the chunk partials t, t + 256, ... in ascending order, then the same tree
__global__ __launch_bounds__(256) void k_bn_loglik_sum(BnLoglikSumArgs a) {
    const double* p = a.partials + (size_t)blockIdx.x * a.chunks;
    double s = 0.0;
    for (int c = threadIdx.x; c < a.chunks; c += 256) s += p[c];
    fit_chunk_sum(s, &a.out[blockIdx.x]);
}

static void fit_launch_loglik_sum(int B, int chunks, const double* partials, double* out, dvs_stream_t st) {
    const BnLoglikSumArgs a = {chunks, partials, out};
    DVS_LAUNCH(k_bn_loglik_sum, dim3((unsigned)B), dim3(256), 0, st, a);
}
