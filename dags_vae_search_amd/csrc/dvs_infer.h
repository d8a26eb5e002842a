// Inference on a fitted discrete Bayesian network (definitions in include/dvs.h): likelihood weighting with
// evidence — bnlearn's cpquery / cpdist and predict(method = "bayes-lw") — and the exact posterior of one variable given all
// the others.  Included by k_bic.hip after dvs_params.h, whose preparation (k_bn_sample_prep: order, slots, thresholds,
// refusal bits) and CPT layout it reuses.  fp64 with contraction off, every sum in a fixed order, no atomics but the status
// atomicOr: two runs give equal bytes.
//
//   k_bn_lw_check        one thread per query: an observed variable whose evidence level is >= its level count (or an
//                        observed bit >= n) marks the query (workspace) and sets bit 4.
//   k_bn_lw              a 256-thread workgroup walks (query, 256-particle chunk) work items in a grid-stride loop, one
//                        particle per thread: the variables in the prep's order, the levels in registers (BnRow), an
//                        observed variable clamped (weight *= theta), an unobserved one drawn as k_bn_sample draws.  The
//                        thresholds are staged once per workgroup (LDS up to DVS_BN_SAMPLE_LDS_CELLS), not once per chunk.
//                        Every cell of the chunk (sum w, sum w^2, sum w [event], then w [level = k] per target level) is
//                        added by the tree of k_bn_loglik_rows, BN_LW_BATCH cells per pass through one LDS array.
//   k_bn_lw_fold         one workgroup per (query, group of cells): slot t adds the chunk sums t, t + 256, ... and the same tree
//                        follows.  With fewer than 256 chunks the slots beyond the next power of two P hold +0 and are not
//                        visited (x + (+0) is x for every x that is not -0, and a slot starts from +0), so 256 / P cells share
//                        a workgroup; with 256 chunks or more every cell has a workgroup of its own.
//   k_bn_blanket         one thread per row, one workgroup per 256 rows of one structure: the products of the target's
//                        levels, their sum in ascending level, one division each.
#pragma once
#include "dvs_params.h"

constexpr int BN_LW_BATCH = 8;                               // cells reduced per pass: 8 * 256 doubles = 16 KiB of LDS
#ifndef BN_LW_GROUPS_PER_CU
#define BN_LW_GROUPS_PER_CU 3                                // workgroups launched per CU: what its LDS holds of the staged kernel
                                                             // (17 KiB + 32 KiB each); 8 and 16 measured no faster
#endif

// red: nb arrays of 256 slots; x[i] += x[i + s] for s = 128, ..., 1 in each, all threads sharing the additions of a step
__device__ __forceinline__ void bn_lw_tree(double* red, const int nb, const int tid) {
    for (int s = 128, sh = 7; s > 0; s >>= 1, --sh) {
        for (int idx = tid; idx < nb * s; idx += 256) {
            const int c = idx >> sh, i = idx & (s - 1);
            red[c * 256 + i] += red[c * 256 + i + s];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bn_lw_check(BnLwArgs a) {
    if (!a.header[BN_HDR_DRAWABLE]) return;                  // the prep refused the network: nothing is judged
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Q) return;
    const uint64_t obs = a.observed[q];
    bool bad = a.n < 64 && (obs >> a.n) != 0ull;
    const uint64_t* ev = a.evidence + (size_t)q * a.words;
    for (int v = 0; v < a.n; ++v)
        if ((obs >> v) & 1ull)
            if (bic_level(ev, v) >= a.card[v]) bad = true;
    a.qbad[q] = bad ? 1 : 0;
    if (bad) atomicOr(a.status, 16);
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_bn_lw(BnLwArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[BN_LW_BATCH * 256];
    __shared__ int s_order[48], s_base[48], s_tgt[48];
    __shared__ unsigned char s_card[48];
    __shared__ unsigned short s_event[48];
    __shared__ uint64_t s_par[48];
    const int tid = threadIdx.x, n = a.n;
    if (!a.header[BN_HDR_DRAWABLE]) return;                  // uniform: the prep refused the network
    if (tid < n) {
        s_order[tid] = a.header[tid];
        bn_stage_var(tid, tid, a.offsets, a.card, a.parents, s_base, s_card, s_par);
        s_event[tid] = a.event ? a.event[tid] : (unsigned short)0xffffu;
    }
    if (tid == 0) {
        int t = 0;
        for (uint64_t tm = a.targets; tm; tm &= tm - 1ull) s_tgt[t++] = dvs_ctz64(tm);
    }
    const uint32_t* thr = a.thr;
    if (STAGED) {
        uint32_t* lt = (uint32_t*)smem;
        for (int i = tid; i < (int)a.n_cells; i += blockDim.x) lt[i] = a.thr[i];
        thr = lt;
    }
    __syncthreads();
    const double* cpt = a.cpt + a.offsets[0];
    const long long items = (long long)a.Q * a.chunks;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int q = (int)(item / a.chunks), chunk = (int)(item - (long long)q * a.chunks);
        const long long p = (long long)chunk * 256 + tid;
        const bool live = p < a.M;
        const size_t slot = (size_t)q * (size_t)a.M + (size_t)p;
        if (a.qbad[q]) {                                     // uniform: the fold writes this query's NaN sums
            if (live && a.particles) {
                for (int i = 0; i < a.words; ++i) a.particles[slot * a.words + i] = 0ull;
                a.pweights[slot] = bn_nan();
            }
            continue;
        }
        const uint64_t obs = a.observed[q];
        const BnRow ev = bn_row_load(a.evidence + (size_t)q * a.words, a.words);
        const uint32_t key = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_BN_LW, a.query_offset + (uint32_t)q);
        BnRow x = {0ull, 0ull, 0ull};
        double w = 1.0;
        bool in_event = true;
        {
#pragma clang fp contract(off)
            for (int i = 0; i < n; ++i) {
                const int v = s_order[i], r = s_card[v];
                const int cfg = bn_row_config(x, s_par[v], s_card);
                uint64_t level;
                if ((obs >> v) & 1ull) {                     // uniform per work item: no divergence
                    level = (uint64_t)bn_level(ev, v);
                    w *= cpt[s_base[v] + cfg * r + (int)level];
                } else {
                    level = bn_draw_level(thr + s_base[v] + cfg * r, r, dvs_draw(dvs_draw(key, (uint32_t)v), (uint32_t)p) >> 1);
                }
                in_event = in_event && ((s_event[v] >> level) & 1u);
                x = bn_row_with(x, v, level);
            }
        }
        if (live && a.particles) {
            bn_row_store(a.particles + slot * a.words, x, a.words);
            a.pweights[slot] = w;
        }
        if (!live) w = 0.0;                                  // absent particles count +0 in every cell
        double* part = a.partials + (size_t)item * a.cells;
        __syncthreads();                                     // the previous item's last reads of red
        {
#pragma clang fp contract(off)
            red[tid] = w;
            red[256 + tid] = w * w;
            red[512 + tid] = in_event ? w : 0.0;
        }
        __syncthreads();
        bn_lw_tree(red, 3, tid);
        if (tid < 3) part[tid] = red[tid * 256];
        for (int t = 0; t < a.T; ++t) {
            const int v = s_tgt[t], r = s_card[v], lvl = bn_level(x, v);
            for (int k0 = 0; k0 < r; k0 += BN_LW_BATCH) {
                const int nb = r - k0 < BN_LW_BATCH ? r - k0 : BN_LW_BATCH;
                __syncthreads();
                for (int c = 0; c < nb; ++c) red[c * 256 + tid] = lvl == k0 + c ? w : 0.0;
                __syncthreads();
                bn_lw_tree(red, nb, tid);
                if (tid < nb) part[3 + t * 16 + k0 + tid] = red[tid * 256];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_bn_lw_fold(BnLwArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x, q = blockIdx.x;
    if (!a.header[BN_HDR_DRAWABLE]) return;
    const int outs = 3 + 16 * a.T;
    double* sums = a.sums + (size_t)q * 3;
    double* marg = a.marginals ? a.marginals + (size_t)q * a.T * 16 : nullptr;
    if (a.qbad[q]) {
        for (int c = tid; c < outs && blockIdx.y == 0; c += 256) {
            if (c < 3) sums[c] = bn_nan();
            else marg[c - 3] = bn_nan();
        }
        return;
    }
    int P = 1, sh = 0;                                       // the slots that can hold a chunk sum: min(256, 2^ceil(log2 chunks))
    while (P < 256 && P < a.chunks) {
        P <<= 1;
        ++sh;
    }
    const int G = 256 >> sh, g = tid >> sh, i = tid & (P - 1);
    const double* part = a.partials + (size_t)q * a.chunks * a.cells;
    {                                                        // blockIdx.y: which G cells of the query this workgroup folds
        const int c = (int)blockIdx.y * G + g;
        bool valid = c < 3;
        if (!valid && c < outs) {
            int v = 0, t = (c - 3) >> 4;                     // the t-th target in ascending id
            for (uint64_t tm = a.targets; tm; tm &= tm - 1ull, --t)
                if (t == 0) {
                    v = dvs_ctz64(tm);
                    break;
                }
            valid = ((c - 3) & 15) < a.card[v];
        }
        double s = 0.0;
        if (valid)
            for (int ch = i; ch < a.chunks; ch += 256) s += part[(size_t)ch * a.cells + c];
        red[tid] = s;
        __syncthreads();
        for (int k = P >> 1; k > 0; k >>= 1) {
            if (i < k) red[tid] += red[tid + k];
            __syncthreads();
        }
        if (i == 0 && c < outs) {
            const double x = red[tid];                       // +0 for the cells at or beyond the target's level count
            if (c < 3) sums[c] = x;
            else marg[c - 3] = x;
            if (c == 0 && x == 0.0) atomicOr(a.status, 128); // evidence of probability zero: information, not an error
        }
    }
}

// what k_bn_sample_prep reads of a likelihood-weighting call: the network and the sampler's workspace
static inline BnSampleArgs bn_lw_prep_args(const BnLwArgs& a) {
    BnSampleArgs p = {};
    p.n = a.n, p.words = a.words, p.n_cells = a.n_cells;
    p.card = a.card, p.parents = a.parents, p.offsets = a.offsets, p.cpt = a.cpt;
    p.header = a.header, p.thr = a.thr, p.status = a.status;
    return p;
}

void dvs_launch_bn_lw(const BnLwArgs& in, uint64_t seed, dvs_stream_t st) {
    BnLwArgs a = in;
    a.words = bic_words(a.n);
    dvs_seed_split(a, seed);
    a.T = 0;
    for (uint64_t tm = a.targets; tm; tm &= tm - 1ull) ++a.T;
    a.cells = 3 + 16 * a.T;
    DVS_LAUNCH(k_bn_sample_prep, dim3(1), dim3(256), 0, st, bn_lw_prep_args(a));
    DVS_LAUNCH(k_bn_lw_check, dim3((unsigned)((a.Q + 255) / 256)), dim3(256), 0, st, a);
    const long long items = (long long)a.Q * a.chunks;
    const long long cap = (long long)(a.cus > 0 ? a.cus : 256) * BN_LW_GROUPS_PER_CU;
    const unsigned grid = (unsigned)(items < cap ? items : cap);         // the rest of the items by the stride
    if (a.n_cells <= DVS_BN_SAMPLE_LDS_CELLS) {
        const size_t lds = (size_t)DVS_BN_SAMPLE_LDS_CELLS * sizeof(uint32_t);
        DVS_LAUNCH_AS("k_bn_lw_lds", k_bn_lw<true>, dim3(grid), dim3(256), lds, st, a);
    } else {
        DVS_LAUNCH_AS("k_bn_lw_global", k_bn_lw<false>, dim3(grid), dim3(256), 0, st, a);
    }
    int slots = 1;                                           // k_bn_lw_fold's P: 256 / P cells share a workgroup
    while (slots < 256 && slots < a.chunks) slots <<= 1;
    const int per_group = 256 / slots, outs = 3 + 16 * a.T;
    DVS_LAUNCH(k_bn_lw_fold, dim3((unsigned)a.Q, (unsigned)((outs + per_group - 1) / per_group)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_bn_blanket
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_blanket(BnBlanketArgs a) {
    __shared__ long long s_base[48];
    __shared__ int s_ok;
    __shared__ unsigned char s_card[48];
    __shared__ uint64_t s_par[48];
    const int tid = threadIdx.x, n = a.n, tg = a.target;
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x - b * a.chunks;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    if (tid < n) {
        const size_t fam = (size_t)b * n + tid;
        const long long lo = a.offsets[fam], hi = a.offsets[fam + 1], r = a.card[tid];
        const uint64_t pm = a.parents[fam] & ~(1ull << tid);
        bool ok = r >= 1 && r <= 16 && !(n < 64 && (pm >> n)) && lo >= 0 && hi <= a.cpt_cells;
        long long q = 1;                                     // bn_family_layout<false>'s walk, kept here: one lane per variable
        for (uint64_t m = pm; m && ok; m &= m - 1ull) {      // walks at once, and the shared routine's two exits cost this
            q *= a.card[dvs_ctz64(m)];                       // kernel three more SGPRs
            ok = q * r <= 0x7fffffffLL;
        }
        if (!ok || hi - lo != q * r) s_ok = 0;
        s_base[tid] = lo;
        s_card[tid] = (unsigned char)r;
        s_par[tid] = pm;
    }
    __syncthreads();
    const long long row = (long long)chunk * 256 + tid;
    if (row >= a.rows) return;
    const int rt = a.card[tg];                               // the width of a posterior row, whatever the family looks like
    double* post = a.posterior ? a.posterior + ((size_t)b * a.rows + row) * rt : nullptr;
    unsigned char* pred = a.pred + (size_t)b * a.rows + row;
    BnRow x = bn_row_load(a.data + (size_t)row * a.words, a.words);
    bool ok = s_ok != 0;
    for (int v = 0; v < n; ++v)
        if (v != tg && bn_level(x, v) >= s_card[v]) ok = false;                // the target's own column is ignored
    if (!ok) {
        if (s_ok) atomicOr(a.status, 16);                    // a level code >= card
        else if (row == 0) atomicOr(a.status, 16);           // a malformed family
        for (int k = 0; post && k < rt; ++k) post[k] = bn_nan();
        *pred = 255;
        return;
    }
    const uint64_t clear = ~(15ull << (4 * (tg & 15)));      // the target's nibble: product() puts each level there in turn
    if (tg < 16) x.w0 &= clear;
    else if (tg < 32) x.w1 &= clear;
    else x.w2 &= clear;
    const auto product = [&](const int k) -> double {        // theta_t(k | pa), then times the children in ascending id
#pragma clang fp contract(off)
        const BnRow xk = bn_row_with(x, tg, (uint64_t)k);
        const auto theta = [&](const int c) -> double {
            const int cfg = bn_row_config(xk, s_par[c], s_card);
            return a.cpt[s_base[c] + (long long)cfg * s_card[c] + bn_level(xk, c)];
        };
        double p = theta(tg);
        if (a.use_children)
            for (int c = 0; c < n; ++c)
                if ((s_par[c] >> tg) & 1ull) p *= theta(c);
        return p;
    };
    {
#pragma clang fp contract(off)
        double sum = 0.0;
        for (int k = 0; k < rt; ++k) sum += product(k);
        double best = -1.0;
        int arg = 255;
        bool nan = false;
        for (int k = 0; k < rt; ++k) {
            const double x = product(k) / sum;
            if (post) post[k] = x;
            if (x != x) nan = true;
            if (x > best) {
                best = x;
                arg = k;
            }
        }
        *pred = (unsigned char)(nan ? 255 : arg);
    }
}

void dvs_launch_bn_blanket(const BnBlanketArgs& in, dvs_stream_t st) {
    BnBlanketArgs a = in;
    a.words = bic_words(a.n);
    DVS_LAUNCH(k_bn_blanket, dim3((unsigned)a.B * a.chunks), dim3(256), 0, st, a);
}
