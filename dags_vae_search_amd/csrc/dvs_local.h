// Local constraint-based structure learning (include/dvs_local.h), next to the tests it groups.  Included by
// k_bic.hip after dvs_citest.h.  Integer counts and fp64 arithmetic, every reduction in a fixed order, no atomics but the integer
// LDS histogram adds, the status atomicOr and the integer refused total: two runs give equal bytes.
//
//   k_ci_group       one workgroup per group (y, Z, candidates): Z is laid out once by bn_family_layout; the accepted candidates
//                    go in passes of as many (z, x, y) tables as the dynamic LDS holds, and a pass scans the rows once — one
//                    key per row, one integer LDS atomic per candidate.  The statistic of a candidate is summed as k_ci_tests
//                    sums it (ci_config_sums of dvs_citest.h, which both kernels call; configuration z owned by thread
//                    z mod 256, ascending within a thread, the dvs_block_sum256 tree),
//                    so its bytes are those of dvs_ci_tests; up to 64 configurations a wave takes a candidate by itself, its
//                    xor butterfly being that tree with +0.0 in the upper 192 slots.  The p-values are taken one lane per
//                    candidate after the last pass.
//   k_mmpc_update    one wave per target, lane = candidate: what a round's p-values decide (who leaves, the max-min choice).
#pragma once
#include "dvs_citest.h"              // ci_config_sums, ci_gamma_q

__global__ __launch_bounds__(256) void k_ci_group(CiGroupArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[256];
    __shared__ int redi[256];
    __shared__ int z_id[48], z_stride[48];
    __shared__ int c_x[48], c_off[48], c_adf[48];            // the accepted candidates, ascending; c_off: where its table starts
    __shared__ unsigned char c_rx[48];
    __shared__ double c_sum[48];
    __shared__ int s_nz, s_q, s_nc;
    const size_t g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n;
    const int y = a.target[g];
    double* out = a.out + g * (size_t)n * 3;
    for (int i = tid; i < 3 * n; i += 256) out[i] = bn_nan();
    if (tid == 0) {
        const uint64_t zm = a.cond[g], below_n = (1ull << n) - 1ull;              // n <= 48
        bool refused = (a.candidates[g] & ~below_n) != 0ull;
        bool ok = y >= 0 && y < n && !((zm >> y) & 1ull);
        const int ry = ok ? a.card[y] : 0;
        long long q = 0;
        int nz = 0, nc = 0;
        if (ok) {
            nz = bn_family_layout(zm, n, a.card, ry, a.lds_cells, z_id, z_stride, &q);
            ok = nz >= 0 && ry >= 1 && q >= 1;               // a variable of no levels has no table
        }
        for (uint64_t m = a.candidates[g] & below_n; m; m &= m - 1ull) {
            const int x = dvs_ctz64(m), rx = a.card[x];
            if (!ok || x == y || ((zm >> x) & 1ull) || rx < 1 || q * rx * ry > a.lds_cells) {
                refused = true;
                continue;
            }
            c_x[nc] = x;
            c_rx[nc] = (unsigned char)rx;
            ++nc;
        }
        if (refused) atomicOr(a.status, 16);
        s_nz = nz;
        s_q = (int)q;
        s_nc = nc;
    }
    __syncthreads();
    const int nc = s_nc;
    if (nc == 0) return;
    const int nz = s_nz, q = s_q, ry = a.card[y];
    const bool g2 = a.type == DVS_CI_MI || a.type == DVS_CI_MI_ADF;
    unsigned* hist = (unsigned*)smem;
    for (int c0 = 0; c0 < nc;) {
        int c1 = c0, total = 0;                              // the pass: candidates c0 .. c1 - 1, `total` cells
        while (c1 < nc && total + q * c_rx[c1] * ry <= a.lds_cells) {
            if (tid == 0) c_off[c1] = total;
            total += q * c_rx[c1] * ry;
            ++c1;
        }
        for (int i = tid; i < total; i += 256) hist[i] = 0u;
        __syncthreads();
        for (int s = tid; s < a.S; s += 256) {
            const BnRow row = bn_row_load(a.data + (size_t)s * a.words, a.words);
            int key = 0;
            for (int i = 0; i < nz; ++i) key += bn_level(row, z_id[i]) * z_stride[i];
            const int ly = bn_level(row, y);
            for (int c = c0; c < c1; ++c) {
                const int rx = c_rx[c], idx = (key * rx + bn_level(row, c_x[c])) * ry + ly;
                if (idx < q * rx * ry) atomicAdd(&hist[c_off[c] + idx], 1u);      // guarded as k_ci_tests guards it
            }
        }
        __syncthreads();
        if (q <= 64) {                                       // a wave per candidate, lane = configuration
            for (int c = c0 + wave; c < c1; c += 4) {
                const int rx = c_rx[c];
                double acc = 0.0;
                int adf = 0;
                if (lane < q) ci_config_sums(hist + c_off[c] + (size_t)lane * rx * ry, rx, ry, g2, acc, adf);
                acc = dvs_wave_sum(acc, lane);
                adf = dvs_wave_sum(adf, lane);
                if (lane == 0) {
                    c_sum[c] = acc;
                    c_adf[c] = adf;
                }
            }
        } else {
            for (int c = c0; c < c1; ++c) {
                const int rx = c_rx[c];
                double acc = 0.0;
                int adf = 0;
                for (int j = tid; j < q; j += 256) ci_config_sums(hist + c_off[c] + (size_t)j * rx * ry, rx, ry, g2, acc, adf);
                red[tid] = acc;
                redi[tid] = adf;
                __syncthreads();
                dvs_block_sum256(tid, red, redi);
                if (tid == 0) {
                    c_sum[c] = red[0];
                    c_adf[c] = redi[0];
                }
                __syncthreads();
            }
        }
        __syncthreads();
        c0 = c1;
    }
    const int c = lane * 4 + wave;                           // the p-values: a lane per candidate, spread over the four waves
    if (c < nc) {
        const int x = c_x[c], rx = c_rx[c];
        double stat = g2 ? 2.0 * c_sum[c] : c_sum[c];
        if (!(stat > 0.0)) stat = 0.0;
        const bool classic = a.type == DVS_CI_MI || a.type == DVS_CI_X2;
        const double df = classic ? (double)(rx - 1) * (double)(ry - 1) * (double)q : (double)c_adf[c];
        out[3 * x] = stat;
        out[3 * x + 1] = df;
        out[3 * x + 2] = df > 0.0 ? ci_gamma_q(0.5 * df, 0.5 * stat) : 1.0;
    }
}

void dvs_launch_ci_tests_group(const CiGroupArgs& in, dvs_stream_t st) {
    CiGroupArgs a = in;
    a.words = bic_words(a.n);
    const size_t lds = (size_t)a.lds_cells * sizeof(unsigned);
    DVS_SET_LDS(k_ci_group, lds);
    DVS_LAUNCH(k_ci_group, dim3((unsigned)a.G), dim3(256), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_mmpc_update
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mmpc_update(MmpcUpdateArgs a) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), n = a.n;
    if (t >= n) return;
    const bool forward = a.phase == 0, live = lane < n;
    const uint64_t cpc = a.cpc[t], cand = a.cand[t];
    const bool open = live && lane != t && (((forward ? cand : cpc) >> lane) & 1ull);
    long long lo = a.offsets[t], hi = a.offsets[t + 1];
    if (lo < 0) lo = 0;
    if (hi > a.G) hi = a.G;
    const size_t cell = (size_t)t * n + (live ? lane : 0);
    double pm = a.pmax[cell], sm = a.smin[cell];
    bool left = false;
    uint64_t sep = 0ull;
    int refused = 0;
    for (long long g = lo; g < hi; ++g) {
        if (a.target[g] != t) continue;                      // wave-uniform
        if (!open || left || !((a.candidates[g] >> lane) & 1ull)) continue;
        const double* o = a.out + ((size_t)g * n + lane) * 3;
        const double stat = o[0], p = o[2];
        if (p != p) ++refused;
        else if (p > a.alpha) {
            left = true;
            sep = a.cond[g];
        } else if (forward) {
            if (p > pm) pm = p;
            if (stat < sm) sm = stat;
        }
    }
    const uint64_t gone = __ballot(left);
    refused = dvs_wave_sum(refused, lane);
    if (lane == 0 && refused != 0) atomicAdd(a.refused, refused);
    if (left) a.sepset[cell] = sep;
    if (!forward) {
        if (lane == 0) {
            a.cpc_next[t] = cpc & ~gone;
            a.cand_next[t] = cand;
            a.result[2 * (size_t)t] = -1;
            a.result[2 * (size_t)t + 1] = __popcll(gone);
        }
        return;
    }
    if (live) {
        a.pmax[cell] = pm;
        a.smin[cell] = sm;
    }
    const bool still = open && !left;
    const double key = !still ? 2.0 : pm < 0x1p-1022 ? 0.0 : pm;                // an underflowed and a denormal p-value tie
    const double best = dvs_wave_min(key, lane);
    const bool tie = still && key == best;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const double top = dvs_wave_max(tie ? sm : -inf, lane);
    const uint64_t win = __ballot(tie && sm == top);
    if (lane == 0) {
        const int F = win != 0ull ? dvs_ctz64(win) : -1;
        const uint64_t f = F >= 0 ? 1ull << F : 0ull;
        a.cpc_next[t] = cpc | f;
        a.cand_next[t] = cand & ~gone & ~f;
        a.last[t] = F;
        a.result[2 * (size_t)t] = F;
        a.result[2 * (size_t)t + 1] = __popcll(gone);
    }
}

void dvs_launch_mmpc_update(const MmpcUpdateArgs& a, dvs_stream_t st) {
    (void)hipMemsetAsync(a.refused, 0, sizeof(int), st);
    DVS_LAUNCH(k_mmpc_update, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}
