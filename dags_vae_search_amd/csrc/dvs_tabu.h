// Tabu search and random restarts over the moves of dvs_hillclimb.h.  Included by k_bic.hip after it; both
// kernels are one wave per structure, lane = variable, no LDS, on hc_load / hc_moves / hc_apply.
//
//   k_tabu_step    one move per structure whatever its sign: the best legal move whose result is not one of the structures in
//                  the ring (the last tabu_len stood on, the current one included), compared exactly.  An entry equals the
//                  result of a move only if it differs from the current rows by one bit in one row (an add or a delete) or
//                  by bit u of row v and bit v of row u with u in P[v], v not in P[u] (that reversal); anything else bars
//                  nothing.  So the ring (tabu_len n coalesced u64 loads, lane = row) reduces to three bit rows per lane: the
//                  barred adds, deletes and reversals on u -> lane.  The best structure seen is kept next to the walk.
//   k_hc_perturb   one uniformly random legal move per structure: per-lane bit rows of the legal adds, deletes and reversals,
//                  a shuffle prefix over lanes per op, the draw of site DVS_SITE_HC_PERTURB scaled to the count.
#pragma once
#include "dvs_hillclimb.h"

__global__ __launch_bounds__(256) void k_tabu_step(TabuArgs t) {
    const HcArgs& a = t.h;
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int n = a.n;
    const int nsteps = a.steps[b];
    const size_t base = (size_t)b * n;
    HcLane c;
    if (a.converged[b] != 0 || a.flags[b] != 0 || nsteps >= a.step_cap) return hc_sit_out(0, lane, b, a.flags, a.worklist);
    if (const int fl = hc_load(c, n, lane, a.parents, a.local, base)) return hc_sit_out(fl, lane, b, a.flags, a.worklist);
    const double* T = a.toggles + base * n;
    const int nn = n * n;
    // the best seen so far; on the first call the start itself, S = L[0] + L[1] + ... left to right (k_bic_sum's order)
    const int seen = t.visited[b];
    double best_s;
    bool write_best = seen == 0;
    uint64_t best_row = c.row;
    if (seen == 0) {
        best_s = 0.0;
        for (int v = 0; v < n; ++v) best_s += a.local[base + v];
    } else {
        best_s = t.best_score[b];
    }
    // push, then scan the valid entries; the slot just written is the current structure and bars no move
    const int slot = seen % t.tabu_len;
    const int valid = seen + 1 < t.tabu_len ? seen + 1 : t.tabu_len;
    uint64_t* ring = t.ring + (size_t)b * t.tabu_len * n;
    if (c.live) ring[(size_t)slot * n + lane] = c.row;
    uint64_t bar_add = 0ull, bar_del = 0ull, bar_rev = 0ull;
    for (int e = 0; e < valid; ++e) {
        if (e == slot) continue;
        const uint64_t diff = c.live ? ring[(size_t)e * n + lane] ^ c.row : 0ull;
        const uint64_t rows = __ballot(diff != 0ull);
        const int k = __popcll(rows);
        if (k != 1 && k != 2) continue;
        const int v1 = dvs_ctz64(rows), v2 = k == 2 ? dvs_ctz64(rows & (rows - 1ull)) : v1;
        const uint64_t d1 = dvs_bcast64(diff, v1), d2 = dvs_bcast64(diff, v2);
        const uint64_t r1 = dvs_bcast64(c.row, v1), r2 = dvs_bcast64(c.row, v2);
        if (k == 1) {
            if (__popcll(d1) != 1) continue;
            if (lane == v1) {
                if (r1 & d1) bar_del |= d1;
                else bar_add |= d1;
            }
        } else if (d1 == (1ull << v2) && d2 == (1ull << v1)) {
            const bool in1 = (r1 & d1) != 0ull, in2 = (r2 & d2) != 0ull;         // v2 in P[v1], v1 in P[v2]
            if (in1 && !in2 && lane == v1) bar_rev |= d1;                       // reversing v2 -> v1 gives the entry
            if (in2 && !in1 && lane == v2) bar_rev |= d2;
        }
    }
    double best = -__builtin_inf();
    int bcode = HC_NO_MOVE;
    hc_moves(c, T, a.max_parents, a.forbidden, [&](int op, int u, double d) {
        const uint64_t bar = op == 0 ? bar_add : (op == 1 ? bar_del : bar_rev);
        if (!((bar >> u) & 1ull)) hc_consider(d, op * nn + lane * n + u, best, bcode);
    });
    hc_reduce_best(best, bcode, lane);
    if (lane == 0) t.visited[b] = seen + 1;
    if (bcode == HC_NO_MOVE) {
        if (lane == 0) a.converged[b] = 1;
        hc_sit_out(0, lane, b, a.flags, a.worklist);
    } else {
        const int op = bcode / nn, mv = (bcode % nn) / n, mu = bcode % n;
        // S' from the local scores as they will stand, in the same order
        double s_new = 0.0;
        for (int v = 0; v < n; ++v)
            s_new += v == mv ? T[mv * n + mu] : ((op == 2 && v == mu) ? T[mu * n + mv] : a.local[base + v]);
        hc_apply(c, bcode, a.parents, a.local, T, base, a.worklist, b);
        int st = t.stall[b], conv = 0;
        if (s_new - best_s > a.min_delta) {
            best_s = s_new;
            best_row = lane == mv ? c.row ^ (1ull << mu) : ((op == 2 && lane == mu) ? c.row | (1ull << mv) : c.row);
            write_best = true;
            st = 0;
        } else {
            st += 1;
            conv = st >= t.max_stall ? 1 : 0;
        }
        if (lane == 0) {
            t.stall[b] = st;
            if (conv) a.converged[b] = 1;
            hc_record(a, b, nsteps, bcode, best);
        }
    }
    if (write_best) {
        if (c.live) t.best_parents[base + lane] = best_row;
        if (lane == 0) t.best_score[b] = best_s;
    }
}

void dvs_launch_tabu_step(const TabuArgs& t, dvs_stream_t st) {
    DVS_LAUNCH(k_tabu_step, dim3((unsigned)((t.h.B + 3) / 4)), dim3(256), 0, st, t);
}

// ---------------------------------------------------------------------------------------------------------
// One random legal move
// ---------------------------------------------------------------------------------------------------------
// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ int hc_scan(int x, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int y = __shfl(x, (lane - s) & 63);
        if (lane >= s) x += y;
    }
    return x;
}

__global__ __launch_bounds__(256) void k_hc_perturb(PerturbArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int n = a.n;
    const size_t base = (size_t)b * n;
    HcLane c;
    if (a.flags[b] != 0) return hc_sit_out(0, lane, b, a.flags, a.worklist);
    if (const int fl = hc_load(c, n, lane, a.parents, a.local, base)) return hc_sit_out(fl, lane, b, a.flags, a.worklist);
    const double* T = a.toggles + base * n;
    uint64_t m[3] = {0ull, 0ull, 0ull};                                            // bit u: the move op on u -> lane is legal
    hc_moves(c, T, a.max_parents, a.forbidden, [&](int op, int u, double) {
        if (op == 0) m[0] |= 1ull << u;
        else if (op == 1) m[1] |= 1ull << u;
        else m[2] |= 1ull << u;
    });
    // code order is op-major, then v = lane, then u: the moves before this lane's, per op
    int incl[3], total[3];
#pragma unroll
    for (int op = 0; op < 3; ++op) {
        incl[op] = hc_scan(__popcll(m[op]), lane);
        total[op] = __shfl(incl[op], 63);
    }
    const uint32_t M = (uint32_t)(total[0] + total[1] + total[2]);
    if (M == 0u) return hc_sit_out(0, lane, b, a.flags, a.worklist);
    const uint32_t r = dvs_draw(dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_HC_PERTURB, (uint32_t)b), a.draw_index);
    int k = (int)(((uint64_t)r * (uint64_t)M) >> 32);                               // < M; the bias is at most M / 2^32
    int op = 0;
    if (k >= total[0]) {
        k -= total[0];
        op = 1;
        if (k >= total[1]) {
            k -= total[1];
            op = 2;
        }
    }
    const uint64_t mine = op == 0 ? m[0] : (op == 1 ? m[1] : m[2]);
    const int hi = op == 0 ? incl[0] : (op == 1 ? incl[1] : incl[2]);
    const int lo = hi - __popcll(mine);
    const bool owner = k >= lo && k < hi;
    uint64_t rest = mine;
    for (int j = lo; owner && j < k; ++j) rest &= rest - 1ull;                      // drop the k - lo lowest set bits
    const int v = dvs_ctz64(__ballot(owner));
    const int u = __shfl(owner ? dvs_ctz64(rest) : 0, v);
    hc_apply(c, op * n * n + v * n + u, a.parents, a.local, T, base, a.worklist, b);
}

void dvs_launch_hc_perturb(const PerturbArgs& in, uint64_t seed, dvs_stream_t st) {
    PerturbArgs a = in;
    dvs_seed_split(a, seed);
    DVS_LAUNCH(k_hc_perturb, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}
