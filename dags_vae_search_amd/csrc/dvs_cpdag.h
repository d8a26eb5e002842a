// Structure comparison, next to the searches whose results it judges.  Included by k_bic.hip after
// dvs_tabu.h; both kernels are one wave per structure, lane = variable, the lane's row one u64, integers only, no atomics.
//
//   k_cpdag          parent masks of a DAG -> its CPDAG in the same layout (bit u of row v <=> u -> v or u - v; an undirected
//                    edge has both bits).  Skeleton by ballots, the v-structures, then Meek's rules R1 - R3 to a fixpoint:
//                    every lane v tests each of its undirected neighbours u for u -> v, a round's orientations are collected
//                    first and applied afterwards.  R1 and R2 read the rows of u by broadcast; R3 walks the pairs of
//                    S = U[u] & D[v] against the wave's adjacency rows in LDS (written once: the skeleton does not change).
//                    The round loop ends on a wave-uniform ballot and, whatever the input, after n (n - 1) / 2 + 1 rounds:
//                    every round but the last orients an edge.
//   k_pdag_compare   per unordered pair {u, v} the state (none, u -> v, v -> u, undirected) in two masks: lane v owns the
//                    pairs with u < v, reads its row and, transposed by ballots, its column; popcounts, one packed butterfly.
#pragma once
#include "dvs_bn_common.h"

// t[v] bit u = x[u] bit v over the lanes below n (the rows of lanes >= n are zero on entry)
__device__ __forceinline__ uint64_t pd_transpose(uint64_t x, int n, int lane) {
    uint64_t t = 0ull;
    for (int u = 0; u < n; ++u) {
        const uint64_t col = __ballot((int)((x >> u) & 1ull));
        if (lane == u) t = col;
    }
    return t;
}

// Meek's rules R1 - R3 to a fixpoint on one wave's PDAG, for k_cpdag and k_pc_orient (dvs_citest.h).  D: directed in
// (u -> lane), U: undirected (u - lane), adj: the lane's skeleton row, s_adj: the wave's skeleton rows in LDS, written and
// synchronised by the caller.  Every lane of the wave calls it.
__device__ __forceinline__ void pd_meek(uint64_t& D, uint64_t& U, const uint64_t adj, const uint64_t* s_adj, const int n,
                                        const int lane) {
    const uint64_t self = 1ull << lane;
    const int max_rounds = n * (n - 1) / 2 + 1;
    for (int round = 0; round < max_rounds; ++round) {
        uint64_t O = 0ull, via = 0ull;                       // O: u -> lane found this round; via: the parents of lane's parents
        for (int u = 0; u < n; ++u) {
            const uint64_t D_u = dvs_bcast64(D, u), U_u = dvs_bcast64(U, u);
            const uint64_t ubit = 1ull << u;
            if (D & ubit) via |= D_u;
            if (!(U & ubit)) continue;
            bool hit = (D_u & ~adj & ~self) != 0ull;                             // R1: w -> u - lane, w not adjacent to lane
            const uint64_t S = U_u & D;                                          // R3: u - w -> lane for two non-adjacent w
            for (uint64_t rest = S; !hit && rest; rest &= rest - 1ull) {
                const int w = dvs_ctz64(rest);
                hit = (S & ~s_adj[w] & ~(1ull << w)) != 0ull;
            }
            if (hit) O |= ubit;
        }
        O |= U & via;                                                            // R2: u -> w -> lane, u - lane
        if (!__ballot(O != 0ull)) break;                                         // wave-uniform: nothing oriented
        const uint64_t O_out = pd_transpose(O, n, lane);                         // lane -> w found this round
        D |= O;
        U &= ~O & ~O_out;
    }
}

__global__ __launch_bounds__(256) void k_cpdag(CpdagArgs a) {
    __shared__ uint64_t s_adj[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x * 4 + wave;
    if (b >= a.B) return;
    const int n = a.n;
    const size_t base = (size_t)b * n;
    const bool live = lane < n;
    const uint64_t row = live ? a.parents[base + lane] : 0ull;
    const uint64_t self = 1ull << lane, below_n = (1ull << n) - 1ull;           // n <= 48
    const uint64_t reach = bn_closure(row, n);
    const bool illegal = __ballot(live && (row & (~below_n | self)) != 0ull) != 0ull;
    const bool cyclic = __ballot(live && (reach & self) != 0ull) != 0ull;
    const int fl = illegal ? 2 : (cyclic ? 1 : 0);                               // a self-loop is an illegal bit, not a cycle
    if (lane == 0) a.flags[b] = fl;
    if (fl) {                                                                    // wave-uniform
        if (live) a.pdag[base + lane] = 0ull;
        return;
    }
    const uint64_t adj = row | pd_transpose(row, n, lane);
    s_adj[wave][lane] = adj;
    // v-structures: u -> v is compelled if v has a parent that is neither u nor adjacent to u
    uint64_t D = 0ull;                                                           // directed in: u -> lane
    for (int u = 0; u < n; ++u) {
        const uint64_t adj_u = dvs_bcast64(adj, u);
        const uint64_t ubit = 1ull << u;
        if ((row & ubit) && (row & ~adj_u & ~ubit)) D |= ubit;
    }
    uint64_t U = adj & ~D & ~pd_transpose(D, n, lane);                           // undirected: u - lane
    dvs_wave_sync();                                                             // s_adj is read by the other lanes below
    pd_meek(D, U, adj, s_adj[wave], n, lane);
    if (live) a.pdag[base + lane] = D | U;
}

void dvs_launch_cpdag(const CpdagArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_cpdag, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}

__global__ __launch_bounds__(256) void k_pdag_compare(PdagCompareArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int n = a.n;
    const size_t base = (size_t)b * n;
    const bool live = lane < n;
    const uint64_t below_n = (1ull << n) - 1ull, below_me = (1ull << lane) - 1ull;
    const uint64_t A = live ? a.a[base + lane] & below_n : 0ull;
    const uint64_t T = live ? a.b[(a.b_rows == 1 ? (size_t)0 : base) + lane] & below_n : 0ull;
    // the pairs {u, lane} with u < lane: in = u -> lane or u - lane, out = lane -> u or u - lane
    const uint64_t a_in = A & below_me, a_out = pd_transpose(A, n, lane) & below_me;
    const uint64_t t_in = T & below_me, t_out = pd_transpose(T, n, lane) & below_me;
    const uint64_t in_a = a_in | a_out, in_t = t_in | t_out;                     // present in the skeleton
    const uint64_t differ = (a_in ^ t_in) | (a_out ^ t_out);
    // shd, tp, fp, fn, hamming in 12-bit fields: each is at most 48 * 47 / 2 = 1128 over the whole wave
    uint64_t acc = (uint64_t)__popcll(differ) | (uint64_t)__popcll(in_a & ~differ) << 12 | (uint64_t)__popcll(in_a & differ) << 24 |
                   (uint64_t)__popcll(in_t & differ) << 36 | (uint64_t)__popcll(in_a ^ in_t) << 48;
    acc = dvs_wave_sum(acc, lane);
    if (lane < 5) a.counts[(size_t)b * 5 + lane] = (int)((acc >> (12 * lane)) & 0xfffull);
}

void dvs_launch_pdag_compare(const PdagCompareArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_pdag_compare, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}
