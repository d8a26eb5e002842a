// Monte Carlo permutation CI tests (include/dvs_permtest.h states the definitions), next to the asymptotic
// tests whose counting and observed statistic they share.  Included by k_bic.hip after dvs_local.h.  Integer counts and fp64
// arithmetic, every reduction in a fixed order, no atomics but the integer LDS histogram adds and the status atomicOr: two
// runs give equal bytes, whatever `slices` is.
//
//   k_ci_perm         grid (test, slice), 256 threads.  The workgroup counts the observed (z, x, y) table into dynamic LDS and
//                     takes the observed statistic exactly as k_ci_tests does; then thread = permutation within a block of
//                     256.  All lanes walk the same configurations and the same n_xz trip counts, so the LDS reads of the
//                     table are broadcasts and the draw ordinal and the pool size m are wave-uniform; the column pool and the
//                     current row's cells are unrolled 16-entry register arrays.  A block ends in a ballot (the exceed mask
//                     and count) and a dvs_block_sum256 tree (the statistic's sum), written to the workspace.
//   k_ci_perm_finish  one thread per test walks the blocks in ascending order: count, used, the sp mean and Q.
#pragma once
#include "dvs_citest.h"              // ci_config_sums, ci_gamma_q

constexpr uint32_t DVS_SITE_CI_PERM = 800u;      // keyed by the global test index; include/dvs_permtest.h states the draws

// c * log(c), one rounded multiplication: the LDS table and the direct path evaluate this one function, so a term's bytes do
// not depend on which path ran.  No fused multiply-add may absorb the product into a sum: contraction is off in both.
__device__ __forceinline__ double perm_klnk(const unsigned c) {
#pragma clang fp contract(off)
    const double d = (double)c;
    return c > 1u ? d * log(d) : 0.0;
}
__device__ __forceinline__ double perm_mul(const double a, const double b) {
#pragma clang fp contract(off)
    return a * b;
}

// u exactly uniform on [0, m): multiply-shift with rejection; m and ord are wave-uniform, so is the threshold
__device__ __forceinline__ uint32_t perm_draw(const uint32_t key_b, const uint32_t ord, const uint32_t m) {
    const uint32_t h0 = dvs_draw(key_b, ord);
    uint64_t prod = (uint64_t)h0 * m;
    if ((uint32_t)prod < m) {
        const uint32_t thr = (0u - m) % m;
        for (uint32_t a = 1u; (uint32_t)prod < thr; ++a) prod = (uint64_t)dvs_fmix32(h0 ^ (a * 0x632BE5ABu)) * m;
    }
    return (uint32_t)(prod >> 32);
}

// V of one table: the observed one (DRAW = false) or the one permutation key_b draws (DRAW = true).  hist is the observed
// table, lnk the klnk table in LDS or null.  With MARGINS the margin constant is returned in *margin: C for g2, S_counted else.
template <bool DRAW, bool MARGINS>
__device__ __forceinline__ double perm_statistic(const unsigned* hist, const int q, const int rx, const int ry, const bool g2,
                                                 const double* lnk, const uint32_t key_b, double* margin) {
#pragma clang fp contract(off)
    const auto klnk = [&](const unsigned c) { return lnk != nullptr ? lnk[c] : perm_klnk(c); };
    double V = 0.0, M = 0.0;
    uint32_t ord = 0u;
    for (int z = 0; z < q; ++z) {
        const unsigned* cell = hist + (size_t)z * rx * ry;
        unsigned pool[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) pool[k] = 0u;
        unsigned n_z = 0u;
        int last = -1;                                       // the last occupied row: it takes what remains
        for (int i = 0; i < rx; ++i) {
            unsigned n_xz = 0u;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < ry) {
                    const unsigned c = cell[i * ry + k];
                    pool[k] += c;
                    n_xz += c;
                }
            n_z += n_xz;
            if (n_xz != 0u) last = i;
        }
        if (n_z == 0u) continue;
        const double dz = (double)n_z;
        double dyz[16];
        if (!g2) {
#pragma unroll
            for (int k = 0; k < 16; ++k) dyz[k] = (double)pool[k];           // the column sums, before the pool is drawn from
        }
        double Mz = 0.0, rows = 0.0;
        if (MARGINS && g2) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < ry) Mz += klnk(pool[k]);
        }
        unsigned m = n_z;
        for (int i = 0; i <= last; ++i) {
            unsigned n_xz = 0u;
            for (int k = 0; k < ry; ++k) n_xz += cell[i * ry + k];
            if (n_xz == 0u) continue;
            unsigned row[16];
            if (!DRAW) {
#pragma unroll
                for (int k = 0; k < 16; ++k) row[k] = k < ry ? cell[i * ry + k] : 0u;
            } else if (i == last) {
#pragma unroll
                for (int k = 0; k < 16; ++k) row[k] = pool[k];
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) row[k] = 0u;
                for (unsigned d = 0u; d < n_xz; ++d) {
                    const uint32_t u = perm_draw(key_b, ord, m);
                    ++ord;
                    --m;
                    unsigned cum = 0u;
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (k < ry) {
                            const unsigned before = pool[k];
                            const unsigned hit = (u - cum) < before ? 1u : 0u;        // u < cum wraps to a large value: no hit
                            row[k] += hit;
                            pool[k] -= hit;
                            cum += before;
                        }
                }
            }
            if (g2) {
                if (MARGINS) {                               // the row's place in C = sum_z (sum_i + sum_k - klnk(n_z)): i before k
                    Mz = klnk(n_xz) + Mz;
                }
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < ry) V += klnk(row[k]);
            } else {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < ry && dyz[k] != 0.0) {
                        const double c = (double)row[k];
                        s += perm_mul(c, c) / dyz[k];
                    }
                rows += s / (double)n_xz;
            }
        }
        if (!g2) V += perm_mul(dz, rows);
        if (MARGINS) M += g2 ? Mz - klnk(n_z) : dz;
    }
    if (MARGINS) *margin = M;
    return V;
}

__global__ __launch_bounds__(256) void k_ci_perm(CiPermArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[256];
    __shared__ int redi[256];
    __shared__ int z_id[48], z_stride[48];
    __shared__ unsigned long long s_mask[4];
    __shared__ int s_nz, s_q, s_ok;
    const size_t t = blockIdx.x;
    const int tid = threadIdx.x, slice = blockIdx.y;
    const CiArgs& c = a.c;
    const int x = c.pairs[2 * t], y = c.pairs[2 * t + 1];
    if (tid == 0) {                                          // the refusals of k_ci_tests, word for word
        const uint64_t zm = c.cond[t];
        bool ok = x >= 0 && y >= 0 && x < c.n && y < c.n && x != y && !((zm >> x) & 1ull) && !((zm >> y) & 1ull);
        if (ok) {
            const long long plane = (long long)c.card[x] * c.card[y];
            long long q = 0;
            const int nz = bn_family_layout(zm, c.n, c.card, plane, c.max_cells, z_id, z_stride, &q);
            ok = nz >= 0 && q * plane >= 1;
            s_nz = nz;
            s_q = (int)q;
        }
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) {
        if (tid == 0 && slice == 0) {
            atomicOr(c.status, 16);
            c.out[3 * t] = bn_nan();
            c.out[3 * t + 1] = bn_nan();
            c.out[3 * t + 2] = bn_nan();
            a.counts[t * a.blocks] = -1;                     // k_ci_perm_finish: a refused test
        }
        return;
    }
    const int nz = s_nz, q = s_q, rx = c.card[x], ry = c.card[y], plane = rx * ry, cells = q * plane;
    unsigned* hist = (unsigned*)smem;
    bn_dense_count<false, true>(hist, cells, c.data, c.words, c.S, nullptr, nz, z_id, z_stride, [&](const uint64_t* row, int key) {
        return (key * rx + bic_level(row, x)) * ry + bic_level(row, y);
    });
    // the observed statistic: the lines of k_ci_tests
    const bool g2 = a.g2 != 0;
    double acc = 0.0;
    int adf = 0;
    for (int j = tid; j < q; j += blockDim.x) ci_config_sums(hist + (size_t)j * plane, rx, ry, g2, acc, adf);
    red[tid] = acc;
    redi[tid] = adf;
    __syncthreads();
    dvs_block_sum256(tid, red, redi);
    if (tid == 0 && slice == 0) {
        double stat = g2 ? 2.0 * red[0] : red[0];
        if (!(stat > 0.0)) stat = 0.0;
        c.out[3 * t] = stat;
        c.out[3 * t + 1] = (double)(rx - 1) * (double)(ry - 1) * (double)q;
    }
    // klnk(0 .. S) behind the counts, at the next multiple of 8 bytes, when the launcher found room for it
    const double* lnk = nullptr;
    if (g2 && a.lnk_cells > 0) {
        double* table = (double*)(smem + (((size_t)c.max_cells * sizeof(unsigned) + 7) & ~(size_t)7));
        for (int i = tid; i < a.lnk_cells; i += blockDim.x) table[i] = perm_klnk((unsigned)i);
        lnk = table;
    }
    __syncthreads();
    // every lane forms V_obs and the margin constant by the one function the permutations use, in its order
    double margin = 0.0;
    const double v_obs = perm_statistic<false, true>(hist, q, rx, ry, g2, lnk, 0u, &margin);
    const double bar = perm_mul(v_obs, 1.0 - 0x1p-32);
    const uint32_t key_t = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_CI_PERM, a.test_offset + (uint32_t)t);
    const int blk0 = (int)((long long)slice * a.blocks / a.slices), blk1 = (int)((long long)(slice + 1) * a.blocks / a.slices);
    int running = 0;
    for (int blk = blk0; blk < blk1; ++blk) {
        const int b = blk * 256 + tid;
        const double v = perm_statistic<true, false>(hist, q, rx, ry, g2, lnk, dvs_draw(key_t, (uint32_t)b), nullptr);
        const bool live = b < a.B;
        const unsigned long long mask = __ballot(live && v >= bar);
        if ((tid & 63) == 0) s_mask[tid >> 6] = mask;
        {
#pragma clang fp contract(off)
            red[tid] = !live ? 0.0 : g2 ? 2.0 * (v - margin) : v - margin;
        }
        __syncthreads();
        dvs_block_sum256(tid, red);
        const int count = __popcll(s_mask[0]) + __popcll(s_mask[1]) + __popcll(s_mask[2]) + __popcll(s_mask[3]);
        if (tid == 0) {
            const size_t cell = t * a.blocks + blk;
            a.counts[cell] = count;
            a.sums[cell] = red[0];
        }
        if (tid < 4) a.masks[(t * a.blocks + blk) * 4 + tid] = s_mask[tid];
        running += count;
        __syncthreads();                                     // s_mask and red are rewritten by the next block
        if (a.E > 0 && running >= a.E) break;                // smc: this slice alone has seen E exceeding permutations
    }
}

// The walk never reads a block that an early stop left unwritten: a slice leaves block j of its range unwritten only after
// its own count over the blocks before j reached E; those blocks precede j in the walk too, so the walk's running count has
// reached E before it comes to j, and it stops there.
__global__ __launch_bounds__(256) void k_ci_perm_finish(CiPermArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.c.T) return;
    const int* counts = a.counts + (size_t)t * a.blocks;
    if (counts[0] < 0) {
        a.used[t] = 0;
        return;
    }
    double* out = a.c.out + 3 * (size_t)t;
    const double B = (double)a.B;
    int count = 0, used = a.B;
    if (a.sp) {
        const double* sums = a.sums + (size_t)t * a.blocks;
        double total = 0.0;
        for (int j = 0; j < a.blocks; ++j) total += sums[j];
        double df = total / B;
        if (!(df > 0.0)) df = 0.0;
        out[1] = df;
        out[2] = df > 0.0 ? ci_gamma_q(0.5 * df, 0.5 * out[0]) : 1.0;
        a.used[t] = used;
        return;
    }
    for (int j = 0; j < a.blocks; ++j) {
        const int cj = counts[j];
        if (a.E > 0 && count + cj >= a.E) {                  // the E-th exceeding permutation is in this block: find it
            int want = a.E - count, pos = 0;
            const unsigned long long* mask = a.masks + ((size_t)t * a.blocks + j) * 4;
            for (int w = 0; w < 4; ++w) {
                unsigned long long m = mask[w];
                const int pc = __popcll(m);
                if (want > pc) {
                    want -= pc;
                    continue;
                }
                for (int r = 1; r < want; ++r) m &= m - 1ull;
                pos = 64 * w + dvs_ctz64(m);
                break;
            }
            count = a.E;
            used = j * 256 + pos + 1;
            break;
        }
        count += cj;
    }
    out[2] = (double)count / B;
    a.used[t] = used;
}

void dvs_launch_ci_perm(const CiPermArgs& in, uint64_t seed, dvs_stream_t st) {
    CiPermArgs a = in;
    a.c.words = bic_words(a.c.n);
    dvs_seed_split(a, seed);
    // dynamic LDS: the counts, then klnk(0 .. S) when it fits beside them within what a workgroup may ask for
    const size_t counts_bytes = ((size_t)a.c.max_cells * sizeof(unsigned) + 7) & ~(size_t)7;
    const size_t table_bytes = ((size_t)a.c.S + 1) * sizeof(double);
    a.lnk_cells = a.g2 && counts_bytes + table_bytes <= DVS_CI_PERM_LDS ? a.c.S + 1 : 0;
    const size_t lds = counts_bytes + (a.lnk_cells ? table_bytes : 0);
    DVS_SET_LDS(k_ci_perm, lds);
    DVS_LAUNCH(k_ci_perm, dim3((unsigned)a.c.T, (unsigned)a.slices), dim3(256), lds, st, a);
    DVS_LAUNCH(k_ci_perm_finish, dim3((unsigned)((a.c.T + 255) / 256)), dim3(256), 0, st, a);
}
