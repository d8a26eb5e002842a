// Bootstrap arc strengths and the averaged network, next to the scorer and the searches they batch.  Included
// by k_bic.hip after dvs_exact.h.  Semantics: include/dvs.h.
//
//   k_bic_local_rows<FAMILY>   k_bic_local / k_bn_toggle with a row set per structure: the plain kernels' bodies (bic_local_cell,
//   k_bn_toggle_rows<FAMILY>   bn_toggle_cell) with ROWS, where the workgroup resolves rows + set_of[dag] * set_size once and
//                              hands it to bn_family_score<FAMILY, true>, whose two row loads go through it.  So a structure's
//                              cells are the bytes the plain entry point writes on the gathered data set.
//   k_bootstrap_rows           one thread per drawn index: a function of (seed, global set index, position) only.
//   k_arc_strength             one wave per 64 structures, lane = structure.  For every variable v the lane loads its row v
//                              and a ballot per u turns the wave's 64 rows into the bit matrix M[v][u] (bit l: structure l has
//                              bit u in row v), kept in LDS.  Then the workgroup's threads walk the ordered pairs (u, v): the
//                              popcounts of M[v][u] and M[u][v] over its four waves are the pair's counts of up to 256
//                              structures, added to `counts` with one integer atomic per non-zero cell.  Integers only: the
//                              result does not depend on the order of the adds.
//   k_averaged_network         one wave per group.  The pairs' (A, |D - D'|) go to LDS; the threshold is a max / min over the
//                              pairs; the order of the significant pairs is a rank sort (a pair's rank = the pairs that go
//                              before it: a total order, so no ties); the insertion is serial over the ranks with lane =
//                              variable and the lane's ancestors in one u64, as k_hc_step keeps them.
#pragma once
#include "dvs_hillclimb.h"

template <int FAMILY>
__global__ __launch_bounds__(256) void k_bic_local_rows(BicRowsArgs a) {
    bic_local_cell<FAMILY, true>(a.s, &a.r);
}
template <int FAMILY>
__global__ __launch_bounds__(256) void k_bn_toggle_rows(ToggleRowsArgs a) {
    bn_toggle_cell<FAMILY, true>(a.t, &a.r);
}

void dvs_launch_bic_rows(const BicRowsArgs& in, dvs_stream_t st) {
    BicRowsArgs a = in;
    a.s.words = bic_words(a.s.n);
    BN_LAUNCH_FAMILY(a.s.type, k_bic_local_rows, "k_bic_local_rows", "k_bn_local_rows_dirichlet", dim3((unsigned)a.s.B * a.s.n), st, a);
    DVS_LAUNCH(k_bic_sum, dim3((a.s.B + 255) / 256), dim3(256), 0, st, a.s);
}

void dvs_launch_bn_toggle_rows(const ToggleRowsArgs& in, dvs_stream_t st) {
    ToggleRowsArgs a = in;
    a.t.s.words = bic_words(a.t.s.n);
    BN_LAUNCH_FAMILY(a.t.s.type, k_bn_toggle_rows, "k_bn_toggle_rows", "k_bn_toggle_rows_dirichlet", bn_toggle_grid(a.t), st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Bootstrap draw
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bootstrap_rows(BootRowsArgs a) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.n_sets * (size_t)a.set_size) return;
    const uint32_t r = (uint32_t)(idx / (size_t)a.set_size), i = (uint32_t)(idx - (size_t)r * (size_t)a.set_size);
    const uint32_t key = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_BOOTSTRAP, a.set_offset + r);     // mod 2^32
    a.rows[idx] = (int)(((uint64_t)dvs_draw(key, i) * (uint64_t)(uint32_t)a.n_samples) >> 32);
}

void dvs_launch_bootstrap_rows(const BootRowsArgs& in, uint64_t seed, dvs_stream_t st) {
    BootRowsArgs a = in;
    dvs_seed_split(a, seed);
    const size_t total = (size_t)a.n_sets * (size_t)a.set_size;
    DVS_LAUNCH(k_bootstrap_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Arc counts over a batch of networks
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_arc_strength(ArcStrengthArgs a) {
    DVS_DYN_LDS(smem);
    uint64_t* M = (uint64_t*)smem;                           // [4 waves][n][n]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.n, nn = n * n;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = b < (long long)a.B;                    // a lane past the batch holds an empty network
    uint64_t* Mw = M + (size_t)wave * nn;
    for (int v = 0; v < n; ++v) {
        const uint64_t row = live ? a.pdag[(size_t)b * n + v] : 0ull;
        uint64_t keep = 0ull;
        for (int u = 0; u < n; ++u) {
            const uint64_t m = __ballot((int)((row >> u) & 1ull));
            if (lane == u) keep = m;
        }
        if (lane < n) Mw[v * n + lane] = keep;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < nn; p += 256) {
        const int u = p / n, v = p - u * n;
        if (u == v) continue;
        int any = 0, dir2 = 0;
        for (int w = 0; w < 4; ++w) {
            const uint64_t in = M[(size_t)w * nn + v * n + u], back = M[(size_t)w * nn + u * n + v];     // u in row v; v in row u
            any += __popcll(in | back);
            dir2 += 2 * __popcll(in & ~back) + __popcll(in & back);
        }
        if (any) atomicAdd(a.counts + 2 * (size_t)p, any);
        if (dir2) atomicAdd(a.counts + 2 * (size_t)p + 1, dir2);
    }
}

void dvs_launch_arc_strength(const ArcStrengthArgs& a, dvs_stream_t st) {
    const size_t lds = (size_t)4 * a.n * a.n * sizeof(uint64_t);             // 72 KiB at n = 48
    DVS_SET_LDS(k_arc_strength, lds);
    DVS_LAUNCH(k_arc_strength, dim3((unsigned)((a.B + 255) / 256)), dim3(256), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Threshold and averaged network
// ---------------------------------------------------------------------------------------------------------
constexpr int AVG_MAX_PAIRS = 48 * 47 / 2;

__global__ __launch_bounds__(64) void k_averaged_network(AvgNetArgs a) {
    __shared__ int s_A[AVG_MAX_PAIRS], s_code[AVG_MAX_PAIRS], s_order[AVG_MAX_PAIRS];
    __shared__ uint32_t s_gap[AVG_MAX_PAIRS];                // |D - D'|
    const int lane = threadIdx.x, g = blockIdx.x, n = a.n;
    const int* C = a.counts + (size_t)g * n * n * 2;
    const int P = n * (n - 1) / 2;
    // the pairs u < v in ascending u n + v
    for (int u = 0, p0 = 0; u < n; p0 += n - 1 - u, ++u)
        for (int v = u + 1 + lane; v < n; v += 64) {
            const int p = p0 + (v - u - 1);
            const long long D = C[2 * (u * n + v) + 1], Dr = C[2 * (v * n + u) + 1];
            s_A[p] = C[2 * (u * n + v)];
            s_gap[p] = (uint32_t)(D > Dr ? D - Dr : Dr - D);
            s_code[p] = u * n + v;
        }
    dvs_wave_sync();
    int min_any = a.min_any[g];
    if (min_any < 0) {                                       // wave-uniform
        const long long R = a.n_networks[g];
        int below = (int)0x80000000, least = 0x7fffffff;     // the largest A with 2 A <= R; the smallest A
        bool some = false;
        for (int p = lane; p < P; p += 64) {
            const int A = s_A[p];
            if (2ll * A <= R) {
                some = true;
                below = A > below ? A : below;
            }
            least = A < least ? A : least;
        }
        const bool have = __ballot(some) != 0ull;
        below = dvs_wave_max(below, lane);
        least = dvs_wave_min(least, lane);
        min_any = (P == 0 ? 0 : (have ? below : least)) + 1;
    }
    // rank of every significant pair: A descending, |D - D'| descending, u n + v ascending
    int n_sig_lane = 0;
    for (int p = lane; p < P; p += 64) {
        const int A = s_A[p];
        if (A < min_any) continue;
        ++n_sig_lane;
        const uint32_t gp = s_gap[p];
        int rank = 0;
        for (int q = 0; q < P; ++q) {
            const int Aq = s_A[q];
            if (Aq < min_any) continue;
            const uint32_t gq = s_gap[q];
            rank += (Aq > A || (Aq == A && (gq > gp || (gq == gp && q < p)))) ? 1 : 0;
        }
        s_order[rank] = p;
    }
    const int n_sig = dvs_wave_sum(n_sig_lane, lane);
    dvs_wave_sync();
    uint64_t row = 0ull, reach = 0ull;                       // lane = variable: its parents, its ancestors
    int placed = 0, dropped = 0, ties = 0;
    for (int k = 0; k < n_sig; ++k) {                        // wave-uniform
        const int p = s_order[k], code = s_code[p];
        const int u = code / n, v = code - u * n;
        const int D = C[2 * (u * n + v) + 1], Dr = C[2 * (v * n + u) + 1];
        const bool tie = D == Dr;
        int t = D >= Dr ? u : v, h = D >= Dr ? v : u;        // t -> h; a tie tries u -> v first
        uint64_t reach_t = dvs_bcast64(reach, t);
        bool cyc = ((reach_t >> h) & 1ull) != 0ull;          // h is an ancestor of t
        if (tie) {
            ++ties;
            if (cyc) {                                       // then v -> u cannot close a cycle: the graph is acyclic
                t = v;
                h = u;
                reach_t = dvs_bcast64(reach, t);
                cyc = ((reach_t >> h) & 1ull) != 0ull;
            }
        }
        if (cyc) {
            ++dropped;
            continue;
        }
        ++placed;
        if (lane == h) row |= 1ull << t;
        if (lane == h || ((reach >> h) & 1ull)) reach |= reach_t | (1ull << t);
    }
    if (lane < n) a.parents[(size_t)g * n + lane] = row;
    if (lane == 0) {
        int* info = a.info + 4 * (size_t)g;
        info[0] = min_any;
        info[1] = placed;
        info[2] = dropped;
        info[3] = ties;
    }
}

void dvs_launch_averaged_network(const AvgNetArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_averaged_network, dim3((unsigned)a.G), dim3(64), 0, st, a);
}
