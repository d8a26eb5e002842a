// Available-case scoring on incomplete data (definitions in include/dvs_available.h): the node-average
// likelihood of a family over exactly the rows in which the family is wholly observed.  Included by k_bic.hip last.
//
//   bn_family_score_avail   the sibling of bn_family_score<0>: the same walk over the parent mask, the same two counting
//                           strategies and the same scoring loops, with a row that does not count left out.  It is a sibling,
//                           not a third template flag, so that the plain instantiations compile to the code they had.  The
//                           scoring loops are restated here word for word: they must stay the loops of bn_family_score<0>,
//                           because LL is defined as the plain scorer's bytes on the gathered rows (the tests compare them).
//       dense   a thread loads observed[s] first, skips the row if the family mask is not covered, and only then loads the
//               data words of the family's variables.  m is counted in integers: a ballot and popcount per wave and sweep,
//               one LDS integer atomic per wave at the end.
//       sort    a row that does not count gets the key ~0; no valid key has bit 63, so those sort behind the valid ones and
//               every loop and binary search runs over [0, m): the per-thread partial sums and the block tree are those of
//               the plain kernel on the m gathered rows.
//   k_bn_local_avail        one workgroup per (structure, variable); k_bic_sum adds the rows up.
//   k_bn_toggle_avail       one workgroup per cell, the grid and worklist logic of bn_toggle_cell.
// Both are family 0 only: 256 threads, the scorer's dynamic LDS.  Integer atomics only.
#pragma once
#include "dvs_hillclimb.h"

// Every thread of the workgroup calls it (it holds barriers).  Thread 0 gets the local score — NaN (status bit 4) when the
// family is refused, -inf (status bit 7) when no row counts — and *m_out, the rows that counted (0 when refused).
__device__ __forceinline__ double bn_family_score_avail(const BicArgs& a, const uint64_t* observed, const int v, const uint64_t* pmask,
                                                        const uint64_t flip, char* smem, int* m_out) {
    __shared__ double red[256];
    __shared__ int par_id[48], par_stride[48], par_shift[48];
    __shared__ int s_np, s_mode, s_rbits, s_m;
    __shared__ double s_q;
    const int r = a.card[v];
    const uint64_t fam = ((*pmask ^ flip) & ~(1ull << v)) | (1ull << v);      // the family mask: v and its parents
    if (threadIdx.x == 0) {
        uint64_t pm = (*pmask ^ flip) & ~(1ull << v);
        double q = 1.0;
        long long qi = 1;
        int np = 0, bits = bic_bits(r), mode = 0;          // mode 0 histogram, 1 sort, -1 unsupported
        for (; pm; pm &= pm - 1) {
            const int p = __builtin_ctzll(pm);
            if (p >= a.n) { mode = -1; break; }
            par_id[np] = p;
            par_stride[np] = (int)qi;
            par_shift[np] = bits;
            bits += bic_bits(a.card[p]);
            q *= a.card[p];
            if (mode == 0) {
                qi *= a.card[p];
                if (qi * r > BIC_MAX_BINS) mode = 1;
            }
            ++np;
        }
        if (mode == 1 && (bits > 63 || a.S > BIC_MAX_SORT)) mode = -1;      // decided on n_samples, not on m
        s_np = np;
        s_q = q;
        s_mode = mode;
        s_rbits = bic_bits(r);
        s_m = 0;
    }
    __syncthreads();
    const int np = s_np, mode = s_mode, S = a.S;
    if (mode < 0) {
        if (threadIdx.x == 0) {
            atomicOr(a.status, 16);
            *m_out = 0;
        }
        return bn_nan();
    }
    double acc = 0.0;
    int wave_m = 0;                                        // rows of this wave that count (the same in all its lanes)
    if (mode == 0) {
        unsigned* hist = (unsigned*)smem;
        const int q = (int)s_q, bins = q * r;
        for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0u;
        __syncthreads();
        for (int s0 = 0; s0 < S; s0 += blockDim.x) {       // uniform trips: the ballot sits outside the lane's branch
            const int s = s0 + (int)threadIdx.x;
            bool counts = false;
            if (s < S) counts = (observed[s] & fam) == fam;
            if (counts) {
                const uint64_t* row = a.data + (size_t)s * a.words;
                int key = 0;
                for (int i = 0; i < np; ++i) key += bic_level(row, par_id[i]) * par_stride[i];
                atomicAdd(&hist[key * r + bic_level(row, v)], 1u);
            }
            wave_m += __popcll(__ballot(counts));
        }
        if ((threadIdx.x & 63) == 0 && wave_m) atomicAdd(&s_m, wave_m);
        __syncthreads();
        for (int j = threadIdx.x; j < q; j += blockDim.x) {
            unsigned nj = 0;
            for (int k = 0; k < r; ++k) nj += hist[j * r + k];
            if (nj == 0) continue;
            const double dn = (double)nj;
            for (int k = 0; k < r; ++k) {
                const unsigned c = hist[j * r + k];
                if (c) acc += (double)c * log((double)c / dn);
            }
        }
    } else {
        uint64_t* keys = (uint64_t*)smem;
        const int rbits = s_rbits;
        int spad = 1;
        while (spad < S) spad <<= 1;
        for (int s0 = 0; s0 < spad; s0 += blockDim.x) {
            const int s = s0 + (int)threadIdx.x;
            uint64_t key = ~0ull;
            bool counts = false;
            if (s < S) counts = (observed[s] & fam) == fam;
            if (counts) {
                const uint64_t* row = a.data + (size_t)s * a.words;
                key = (uint64_t)bic_level(row, v);
                for (int i = 0; i < np; ++i) key |= (uint64_t)bic_level(row, par_id[i]) << par_shift[i];
            }
            if (s < spad) keys[s] = key;
            wave_m += __popcll(__ballot(counts));
        }
        if ((threadIdx.x & 63) == 0 && wave_m) atomicAdd(&s_m, wave_m);
        __syncthreads();
        for (int k = 2; k <= spad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < spad; i += blockDim.x) {
                    const int p = i ^ j;
                    if (p > i) {
                        const uint64_t x = keys[i], y = keys[p];
                        if ((x > y) == ((i & k) == 0)) {
                            keys[i] = y;
                            keys[p] = x;
                        }
                    }
                }
                __syncthreads();
            }
        const int m = s_m;                                 // the valid keys are keys[0 .. m)
        for (int i = threadIdx.x; i < m; i += blockDim.x) {
            const uint64_t key = keys[i];
            if (i > 0 && keys[i - 1] == key) continue;                 // not the first sample of its (j, k) cell
            const int c = bic_lower_bound(keys, m, key + 1) - i;
            const uint64_t j0 = (key >> rbits) << rbits;
            const int nj = bic_lower_bound(keys, m, j0 + (1ull << rbits)) - bic_lower_bound(keys, m, j0);
            acc += (double)c * log((double)c / (double)nj);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    dvs_block_sum256((int)threadIdx.x, red);
    double score = 0.0;
    if (threadIdx.x == 0) {
        const int m = s_m;
        *m_out = m;
        if (m == 0) {
            atomicOr(a.status, 128);
            score = -__builtin_inf();
        } else {
#pragma clang fp contract(off)
            const double mean = red[0] / (double)m;
            const double pen = a.arg * (double)(r - 1) * s_q;
            score = mean - pen;
        }
    }
    return score;
}

__global__ __launch_bounds__(256) void k_bn_local_avail(BicAvailArgs a) {
    DVS_DYN_LDS(smem);
    const int v = blockIdx.x % a.s.n, dag = blockIdx.x / a.s.n;
    const size_t cell = (size_t)dag * a.s.n + v;
    int m = 0;
    const double score = bn_family_score_avail(a.s, a.observed, v, a.s.parents + cell, 0ull, smem, &m);
    if (threadIdx.x == 0) {
        a.s.local[cell] = score;
        if (a.used != nullptr) a.used[cell] = m;
    }
}

__global__ __launch_bounds__(256) void k_bn_toggle_avail(ToggleAvailArgs a) {
    DVS_DYN_LDS(smem);
    const ToggleArgs& t = a.t;
    const int n = t.s.n;
    const int u = blockIdx.x % n, row = blockIdx.x / n;
    int dag, v;
    if (t.worklist != nullptr) {                             // as bn_toggle_cell
        v = t.worklist[row];
        dag = row >> 1;
        if (v < 0 || v >= n || u == v) return;
    } else {
        v = row % n;
        dag = row / n;
    }
    const size_t cell = (size_t)dag * n + v;
    int m = 0;
    const double score = bn_family_score_avail(t.s, a.observed, v, t.s.parents + cell, u == v ? 0ull : 1ull << u, smem, &m);
    if (threadIdx.x == 0) {
        if (u == v) {
            t.s.local[cell] = score;
            t.toggles[cell * n + u] = bn_nan();
        } else {
            t.toggles[cell * n + u] = score;
        }
    }
}

void dvs_launch_bn_avail(const BicAvailArgs& in, dvs_stream_t st) {
    BicAvailArgs a = in;
    a.s.words = bic_words(a.s.n);
    DVS_SET_LDS(k_bn_local_avail, bn_table_lds());
    DVS_LAUNCH(k_bn_local_avail, dim3((unsigned)a.s.B * a.s.n), dim3(256), bn_table_lds(), st, a);
    DVS_LAUNCH(k_bic_sum, dim3((a.s.B + 255) / 256), dim3(256), 0, st, a.s);
}

void dvs_launch_bn_toggle_avail(const ToggleAvailArgs& in, dvs_stream_t st) {
    ToggleAvailArgs a = in;
    a.t.s.words = bic_words(a.t.s.n);
    DVS_SET_LDS(k_bn_toggle_avail, bn_table_lds());
    DVS_LAUNCH(k_bn_toggle_avail, dim3(bn_toggle_grid(a.t)), dim3(256), bn_table_lds(), st, a);
}
