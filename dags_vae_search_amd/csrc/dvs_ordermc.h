// Order MCMC over family lists: posterior arc probabilities and an order-space structure search for n <= 48,
// by Friedman and Koller's (2003) Metropolis sampler over variable orders.  Included by k_bic.hip after dvs_posterior.h, whose
// order-modular posterior is this sampler's stationary distribution.  Natural logs in fp64, only exp and log, no
// floating-point atomics, every sum in a fixed order: two runs give equal bytes, and so does a run cut into calls or shards
// (semantics: include/dvs.h, dvs_order_mcmc).  The prior is order-modular (uniform over orders), NOT uniform over DAGs.
//
//   k_omc_check     the list's properties on the device: offsets ascending from 0 to F with at least one family per variable,
//                   entry 0 of every variable the empty set, no mask with its own bit or a bit >= n, finite scores.  A failure
//                   ors a bit into flags[0] (integer atomic); k_omc_chain reads those bits and returns before it touches anything.
//   k_omc_chain     one workgroup of 256 threads per chain, the step loop inside.  LDS holds the order, every variable's
//                   predecessor mask, its cached term, bestf and arg, the chain's sums [n][n] and the lanes' arc accumulators.
//                   A term (omc_term) is two passes over the variable's families, lanes striding: the largest consistent
//                   score with its lowest index, then the sum of exp(score - largest).  Lane i takes the families lo + i,
//                   lo + i + 256, ... in that order; the 64 lanes of a wave meet in the xor butterfly of dvs_wave_sum /
//                   dvs_wave_max, the four waves are added in wave order.  A kept sample (omc_keep) gives lane i one f64 cell
//                   per parent u, to which it adds exp(score - term) of its families that contain u in the same order; thread
//                   (w, u) then adds the 64 cells of wave w in lane order and thread u the four waves in wave order, into
//                   sums[u][v].  Nothing waits on another workgroup, and every loop bound is an argument the host has checked
//                   or an offset k_omc_check has.
//   k_omc_finish    one workgroup per arc: thread i adds chains i, i + 256, ..., the 256 partial sums meet in
//                   dvs_block_sum256; kept is added as integers; prob = sum / kept, or 0 when nothing was kept.
#pragma once
#include "dvs_bn_common.h"

constexpr int OMC_MAX_VARS = 48;
constexpr int OMC_FLAG_OFFSETS = 1, OMC_FLAG_EMPTY_SET = 2, OMC_FLAG_MASK = 4, OMC_FLAG_SCORE = 8, OMC_FLAG_ORDER = 16;
constexpr int OMC_FLAG_LIST = OMC_FLAG_OFFSETS | OMC_FLAG_EMPTY_SET | OMC_FLAG_MASK | OMC_FLAG_SCORE;

__global__ void k_omc_reset(OrderMcmcArgs a) { a.flags[0] = 0; }

__global__ __launch_bounds__(256) void k_omc_check(OrderMcmcArgs a) {
    __shared__ long long off[OMC_MAX_VARS + 1];
    __shared__ int s_bad, s_list;
    const int n = a.n, tid = threadIdx.x;
    if (tid == 0) s_bad = s_list = 0;
    if (tid <= n) off[tid] = a.offsets[tid];
    __syncthreads();
    if (tid < n && (off[tid] < 0 || off[tid] >= off[tid + 1] || off[tid + 1] > a.F)) atomicOr(&s_bad, OMC_FLAG_OFFSETS);
    if (tid == 0 && (off[0] != 0 || off[n] != a.F)) atomicOr(&s_bad, OMC_FLAG_OFFSETS);
    __syncthreads();
    if (s_bad == 0) {                                            // the offsets are sound: family j belongs to one variable; s_bad is not written below
        const long long stride = (long long)gridDim.x * 256;
        for (long long j = (long long)blockIdx.x * 256 + tid; j < a.F; j += stride) {
            int v = 0;
            while (off[v + 1] <= j) ++v;                         // ends: j < F = off[n]
            const uint64_t m = a.sets[j];
            const double s = a.scores[j];
            int bad = 0;
            if (j == off[v] && m != 0ull) bad |= OMC_FLAG_EMPTY_SET;
            if (((m >> v) & 1ull) || (m >> n) != 0ull) bad |= OMC_FLAG_MASK;
            if (!(s - s == 0.0)) bad |= OMC_FLAG_SCORE;          // NaN and both infinities
            if (bad) atomicOr(&s_list, bad);
        }
    }
    __syncthreads();
    if (tid == 0 && (s_bad | s_list)) atomicOr(a.flags, s_bad | s_list);
}

// What k_omc_chain keeps of a chain in static LDS.
struct OmcState {
    int off[OMC_MAX_VARS + 1];           // the list's offsets (F < 2^31)
    int order[OMC_MAX_VARS];             // position -> variable
    uint64_t pred[OMC_MAX_VARS];         // variable -> the variables before it
    double term[OMC_MAX_VARS], bestf[OMC_MAX_VARS];      // variable -> term(v, pred), bestf(v, pred)
    uint64_t arg[OMC_MAX_VARS];          // variable -> arg(v, pred)
    double nterm[OMC_MAX_VARS], nbestf[OMC_MAX_VARS];    // the same for a proposal, by variable
    uint64_t narg[OMC_MAX_VARS], npred[OMC_MAX_VARS];
    uint64_t best_parents[OMC_MAX_VARS];
    double wd[4];                        // one slot per wave
    int wi[4], bad_order;
    double part[4 * OMC_MAX_VARS];       // omc_keep: (wave, u) sums
};

// term(v, Q), bestf(v, Q) and arg(v, Q) of include/dvs.h into slot v of the three arrays; every thread calls it, a barrier
// has passed since the last use of S.wd / S.wi, and one closes it.
__device__ __forceinline__ void omc_term(const OrderMcmcArgs& a, OmcState& S, int v, uint64_t Q, double* term, double* bestf, uint64_t* arg) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = S.off[v], hi = S.off[v + 1];
    double top = ex_neg_inf();
    int at = 0x7fffffff;
    for (int j = lo + tid; j < hi; j += 256) {
        if (a.sets[j] & ~Q) continue;
        const double s = a.scores[j];
        if (s > top) {                                           // ascending j: a tie keeps the lower index
            top = s;
            at = j;
        }
    }
    const double wtop = dvs_wave_max(top, lane);
    const int wat = dvs_wave_min(top == wtop ? at : 0x7fffffff, lane);
    if (lane == 0) {
        S.wd[wave] = wtop;
        S.wi[wave] = wat;
    }
    __syncthreads();
    double best = S.wd[0];
    int best_at = S.wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const double x = S.wd[w];
        const int i = S.wi[w];
        if (x > best || (x == best && i < best_at)) {
            best = x;
            best_at = i;
        }
    }
    __syncthreads();                                             // S.wd is reused below
    double sum = 0.0;
    for (int j = lo + tid; j < hi; j += 256) {
        if (a.sets[j] & ~Q) continue;
        sum += exp(a.scores[j] - best);
    }
    sum = dvs_wave_sum(sum, lane);
    if (lane == 0) S.wd[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        term[v] = best + log(((S.wd[0] + S.wd[1]) + S.wd[2]) + S.wd[3]);
        bestf[v] = best;
        arg[v] = a.sets[best_at];                                // entry lo is the empty set: best_at is always a family
    }
    __syncthreads();
}

// One kept sample: sums[u][v] += P(u -> v | order) for every arc, in the order the file comment states.
__device__ __forceinline__ void omc_keep(const OrderMcmcArgs& a, OmcState& S, double* acc, double* sums) {
    const int tid = threadIdx.x, n = a.n, np = n | 1;
    double* mine = acc + (size_t)tid * np;
    for (int v = 0; v < n; ++v) {
        const int lo = S.off[v], hi = S.off[v + 1];
        const uint64_t Q = S.pred[v];
        const double term = S.term[v];
        for (int u = 0; u < n; ++u) mine[u] = 0.0;
        for (int j = lo + tid; j < hi; j += 256) {
            const uint64_t m = a.sets[j];
            if (m & ~Q) continue;
            const double w = exp(a.scores[j] - term);
            for (uint64_t r = m; r; r &= r - 1ull) mine[dvs_ctz64(r)] += w;      // bits < n: k_omc_check
        }
        __syncthreads();
        if (tid < 4 * n) {
            const int w = tid / n, u = tid - w * n;
            const double* col = acc + (size_t)w * 64 * np + u;
            double s = 0.0;
            for (int l = 0; l < 64; ++l) s += col[(size_t)l * np];
            S.part[tid] = s;
        }
        __syncthreads();
        if (tid < n) sums[tid * n + v] += ((S.part[tid] + S.part[n + tid]) + S.part[2 * n + tid]) + S.part[3 * n + tid];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_omc_chain(OrderMcmcArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ OmcState S;
    if (a.flags[0] & OMC_FLAG_LIST) return;                      // k_omc_check's bits: the order bit is other chains' business
    const int n = a.n, nn = n * n, tid = threadIdx.x, c = blockIdx.x;
    double* acc = (double*)smem;                                 // [256][n | 1]
    double* sums = acc + (size_t)256 * (n | 1);                  // [n][n]
    const uint32_t g = a.chain_offset + (uint32_t)c;
    const uint32_t key = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_ORDER_MCMC, g);
    if (tid <= n) S.off[tid] = (int)a.offsets[tid];
    if (tid < n) S.best_parents[tid] = a.best_parents[(size_t)c * n + tid];
    for (int e = tid; e < nn; e += 256) sums[e] = a.sums[(size_t)c * nn + e];
    if (tid == 0) {
        if (a.init) {
            const uint32_t ikey = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_ORDER_MCMC_INIT, g);
            for (int k = 0; k < n; ++k) S.order[k] = k;
            for (int k = n - 1; k >= 1; --k) {
                const int j = (int)(((uint64_t)dvs_draw(ikey, (uint32_t)k) * (uint64_t)(k + 1)) >> 32);
                const int x = S.order[k];
                S.order[k] = S.order[j];
                S.order[j] = x;
            }
        } else {
            for (int k = 0; k < n; ++k) S.order[k] = a.order[(size_t)c * n + k];
        }
        uint64_t before = 0ull;
        int bad = 0;
        for (int k = 0; k < n; ++k) {
            const int v = S.order[k];
            if (v < 0 || v >= n || ((before >> v) & 1ull)) {     // a caller's order that is no permutation
                bad = 1;
                break;
            }
            S.pred[v] = before;
            before |= 1ull << v;
        }
        S.bad_order = bad;
        if (bad) atomicOr(a.flags, OMC_FLAG_ORDER);
    }
    __syncthreads();
    if (S.bad_order) return;                                     // this chain's outputs stay as they were
    for (int v = 0; v < n; ++v) omc_term(a, S, v, S.pred[v], S.term, S.bestf, S.arg);
    double best = a.best_score[c];
    int accepted = a.accepted[c], kept = a.kept[c];
    // the start order's best DAG: new on a first call, equal (so not replacing) when a run is continued
    bool better;
    {
        double bs = 0.0;
        for (int v = 0; v < n; ++v) bs += S.bestf[v];
        better = bs > best;
        if (better) best = bs;
    }
    if (better && tid < n) S.best_parents[tid] = S.arg[tid];
    __syncthreads();
    for (int s = 0; s < a.steps; ++s) {
        const uint32_t t = a.step_offset + (uint32_t)s;
        if (n > 1) {
            const uint32_t r0 = dvs_draw(key, 3u * t), r1 = dvs_draw(key, 3u * t + 1u), r2 = dvs_draw(key, 3u * t + 2u);
            const int i = (int)(((uint64_t)r0 * (uint64_t)(n - 1)) >> 32);
            const int m = a.window < n - 1 - i ? a.window : n - 1 - i;
            const int j = i + 1 + (int)(((uint64_t)r1 * (uint64_t)m) >> 32);
            // the proposal's order at positions i .. j: order[j], order[i + 1 .. j - 1], order[i]
            uint64_t Q = S.pred[S.order[i]];
            for (int p = i; p <= j; ++p) {
                const int v = S.order[p == i ? j : p == j ? i : p];
                if (tid == 0) S.npred[v] = Q;
                omc_term(a, S, v, Q, S.nterm, S.nbestf, S.narg);
                Q |= 1ull << v;
            }
            double s_old = 0.0, s_new = 0.0;
            for (int p = i; p <= j; ++p) {
                s_old += S.term[S.order[p]];
                s_new += S.nterm[S.order[p == i ? j : p == j ? i : p]];
            }
            const double delta = s_new - s_old;
            const bool accept = log(((double)r2 + 0.5) * (1.0 / 4294967296.0)) < delta;
            __syncthreads();
            if (accept) {
                ++accepted;
                if (tid >= i && tid <= j) {
                    const int v = S.order[tid];
                    S.pred[v] = S.npred[v];
                    S.term[v] = S.nterm[v];
                    S.bestf[v] = S.nbestf[v];
                    S.arg[v] = S.narg[v];
                }
                __syncthreads();
                if (tid == 0) {
                    const int x = S.order[i];
                    S.order[i] = S.order[j];
                    S.order[j] = x;
                }
                double bs = 0.0;
                for (int v = 0; v < n; ++v) bs += S.bestf[v];
                better = bs > best;
                if (better) {
                    best = bs;
                    if (tid < n) S.best_parents[tid] = S.arg[tid];
                }
                __syncthreads();
            }
        }
        if (t >= a.burn_in && (t - a.burn_in) % (uint32_t)a.thin == 0u) {
            omc_keep(a, S, acc, sums);
            ++kept;
        }
        if (a.trace && tid == 0) {
            double sc = 0.0;
            for (int v = 0; v < n; ++v) sc += S.term[v];
            a.trace[(size_t)c * a.steps + s] = sc;
        }
    }
    __syncthreads();
    for (int e = tid; e < nn; e += 256) a.sums[(size_t)c * nn + e] = sums[e];
    if (tid < n) {
        a.order[(size_t)c * n + tid] = S.order[tid];
        a.best_parents[(size_t)c * n + tid] = S.best_parents[tid];
    }
    if (tid == 0) {
        double sc = 0.0;
        for (int v = 0; v < n; ++v) sc += S.term[v];
        a.log_score[c] = sc;
        a.accepted[c] = accepted;
        a.kept[c] = kept;
        a.best_score[c] = best;
    }
}

__global__ __launch_bounds__(256) void k_omc_finish(OrderMcmcFinishArgs a) {
    __shared__ double red[256];
    __shared__ long long cnt[256];
    const int nn = a.n * a.n, e = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    long long k = 0;
    for (int c = tid; c < a.C; c += 256) {
        s += a.sums[(size_t)c * nn + e];
        k += a.kept[c];
    }
    red[tid] = s;
    cnt[tid] = k;
    __syncthreads();
    dvs_block_sum256(tid, red, cnt);
    if (tid == 0) a.prob[e] = cnt[0] > 0 ? red[0] / (double)cnt[0] : 0.0;
}

void dvs_launch_order_mcmc(const OrderMcmcArgs& in, uint64_t seed, dvs_stream_t st) {
    OrderMcmcArgs a = in;
    dvs_seed_split(a, seed);
    long long groups = (a.F + 256 * 16 - 1) / (256 * 16);        // about 16 families a thread
    if (groups > 1024) groups = 1024;
    DVS_LAUNCH(k_omc_reset, dim3(1), dim3(1), 0, st, a);
    DVS_LAUNCH(k_omc_check, dim3((unsigned)groups), dim3(256), 0, st, a);
    DVS_SET_LDS(k_omc_chain, dvs_omc_lds(a.n));
    DVS_LAUNCH(k_omc_chain, dim3((unsigned)a.C), dim3(256), dvs_omc_lds(a.n), st, a);
}

void dvs_launch_order_mcmc_finish(const OrderMcmcFinishArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_omc_finish, dim3((unsigned)(a.n * a.n)), dim3(256), 0, st, a);
}
