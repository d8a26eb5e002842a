// Greedy hill climbing over single-edge moves in structure space, next to the scorer it uses.  Included by
// k_bic.hip after bn_family_score.
//
//   k_bn_toggle<FAMILY>  T[b][v][u] = local score of variable v with parent set P[b][v] xor (1 << u), L[b][v] = the local
//                        score as it stands.  One workgroup per cell, each a bn_family_score call: the bytes of k_bic_local
//                        for that parent set.  bn_toggle_cell is its body and, with a row set, that of k_bn_toggle_rows
//                        (dvs_strength.h).  One table prices all three moves on u -> v:
//                            add / delete   T[v][u] - L[v]
//                            reverse        (T[v][u] - L[v]) + (T[u][v] - L[u])
//                        Full pass: all B n rows.  Incremental pass: the rows named in the worklist, whose slots 2b and
//                        2b + 1 belong to structure b and hold a variable index or -1 (k_hc_step writes them: no atomics,
//                        no order); workgroups of an empty slot exit at once.
//   k_hc_step            one wave per structure, lane = variable, the lane's parent row one u64: ancestor closure by n
//                        rounds of row broadcasts, legality and delta of every move, the best one across lanes (largest
//                        fp64 delta, exact ties to the lowest code = op n^2 + v n + u), applied if delta > min_delta.
//                        How a step starts and ends, closure, legality and pricing are device functions (hc_sit_out,
//                        hc_moves, hc_apply, hc_record) shared with k_tabu_step and k_hc_perturb (dvs_tabu.h).
#pragma once
#include "dvs_bn_common.h"

template <int FAMILY, bool ROWS>
__device__ __forceinline__ void bn_toggle_cell(const ToggleArgs& t, const RowSetArgs* r) {      // r is read with ROWS only
    DVS_DYN_LDS(smem);
    const int n = t.s.n;
    const int u = blockIdx.x % n, row = blockIdx.x / n;
    int dag, v;
    if (t.worklist != nullptr) {
        v = t.worklist[row];
        dag = row >> 1;
        if (v < 0 || v >= n || u == v) return;       // empty slot; L of a moved row is the T cell of the move (k_hc_step)
    } else {
        v = row % n;
        dag = row / n;
    }
    const size_t cell = (size_t)dag * n + v;
    const double score = bn_family_score<FAMILY, ROWS>(t.s, v, t.s.parents + cell, u == v ? 0ull : 1ull << u, smem,
                                                       ROWS ? rs_rows(*r, dag) : nullptr);
    if (threadIdx.x == 0) {
        if (u == v) {
            t.s.local[cell] = score;
            t.toggles[cell * n + u] = bn_nan();
        } else {
            t.toggles[cell * n + u] = score;
        }
    }
}
template <int FAMILY>
__global__ __launch_bounds__(256) void k_bn_toggle(ToggleArgs t) {
    bn_toggle_cell<FAMILY, false>(t, nullptr);
}

// one workgroup per cell of the rows a pass covers: the two worklist slots of every structure, or all its n rows
static inline dim3 bn_toggle_grid(const ToggleArgs& t) {
    const unsigned rows = t.worklist != nullptr ? 2u * (unsigned)t.s.B : (unsigned)t.s.B * (unsigned)t.s.n;
    return dim3(rows * (unsigned)t.s.n);
}
void dvs_launch_bn_toggle(const ToggleArgs& in, dvs_stream_t st) {
    ToggleArgs t = in;
    t.s.words = bic_words(t.s.n);
    BN_LAUNCH_FAMILY(t.s.type, k_bn_toggle, "k_bn_toggle", "k_bn_toggle_dirichlet", bn_toggle_grid(t), st, t);
}

// ---------------------------------------------------------------------------------------------------------
// One greedy step
// ---------------------------------------------------------------------------------------------------------
constexpr int HC_NO_MOVE = 0x7fffffff;

// (delta, code) beats (bd, bc): larger delta, exact ties to the lower code — a total order, so the reduction tree's shape
// cannot change the winner
__device__ __forceinline__ void hc_consider(double d, int c, double& bd, int& bc) {
    if (d > bd || (d == bd && c < bc)) {
        bd = d;
        bc = c;
    }
}

// ---- what k_hc_step, k_tabu_step and k_hc_perturb (dvs_tabu.h) share: one wave per structure, lane = variable -----------
struct HcLane {
    int n, lane;
    bool live;
    uint64_t row, reach, self;   // the lane's parent row, its ancestors, its own bit
    double Lv;                   // its local score
};

// loads the lane's row and local score and closes the structure -> the flags of include/dvs.h (1 cycle, 2 NaN local score)
__device__ __forceinline__ int hc_load(HcLane& c, int n, int lane, const uint64_t* parents, const double* local, size_t base) {
    c.n = n;
    c.lane = lane;
    c.live = lane < n;
    c.row = c.live ? parents[base + lane] : 0ull;
    c.Lv = c.live ? local[base + lane] : 0.0;
    c.self = 1ull << lane;
    c.reach = bn_closure(c.row, n);
    int fl = 0;
    if (__ballot(c.live && (c.reach & c.self) != 0)) fl |= 1;
    if (__ballot(c.live && c.Lv != c.Lv)) fl |= 2;
    return fl;
}

// How a step kernel starts, in the three of them: a structure that is finished or was flagged before sits the launch out
// (fl = 0); else hc_load, and a flag found now (fl != 0) is written and it sits out too.  Sitting out clears the structure's
// two worklist slots, so the next toggle pass skips it.  The kernels keep the two wave-uniform branches themselves and
// return hc_sit_out(...): a prologue that returned "go on" instead compiled to more registers in all three.
__device__ __forceinline__ void hc_sit_out(int fl, int lane, int b, int* flags, int* worklist) {
    if (fl && lane == 0) flags[b] = fl;
    if (lane < 2) worklist[2 * b + lane] = -1;
}

// How a step that moved ends (lane 0): the step count, the trace entry, one more active structure.
__device__ __forceinline__ void hc_record(const HcArgs& a, int b, int nsteps, int bcode, double best) {
    a.steps[b] = nsteps + 1;
    if (a.trace != nullptr) {
        int64_t* t = a.trace + ((size_t)b * a.step_cap + nsteps) * 2;
        t[0] = bcode;
        t[1] = (int64_t)__double_as_longlong(best);
    }
    atomicAdd(a.active, 1);
}

// Legality and pricing: f(op, u, delta) for every legal move on u -> v = lane (op 0 add, 1 delete, 2 reverse) whose delta
// reads no NaN cell, u ascending.  The ballots and broadcasts sit outside every lane-dependent branch.
template <class F>
__device__ __forceinline__ void hc_moves(const HcLane& c, const double* T, int max_parents, const uint64_t* forbidden, F&& f) {
    const int n = c.n, lane = c.lane;
    const bool capped = max_parents > 0;
    const int npar = __popcll(c.row);
    const uint64_t forb_v = (forbidden != nullptr && c.live) ? forbidden[lane] : 0ull;
    for (int u = 0; u < n; ++u) {
        const uint64_t child_u = __ballot(c.live && ((c.row >> u) & 1ull) != 0);
        const uint64_t row_u = dvs_bcast64(c.row, u), reach_u = dvs_bcast64(c.reach, u);
        const double L_u = dvs_bcast_f64(c.Lv, u);
        if (!c.live || u == lane) continue;
        const double t_vu = T[lane * n + u];
        if (t_vu != t_vu) continue;                               // a refused family: the move is not available
        const double d_v = t_vu - c.Lv;
        const uint64_t ubit = 1ull << u;
        if (!(c.row & ubit)) {
            if (!((reach_u >> lane) & 1ull) && !(capped && npar >= max_parents) && !(forb_v & ubit)) f(0, u, d_v);
        } else {
            f(1, u, d_v);
            const double t_uv = T[u * n + lane];
            const uint64_t forb_u = forbidden != nullptr ? forbidden[u] : 0ull;
            if (t_uv == t_uv && !((child_u & ~c.self) & (c.reach | c.self)) && !(capped && __popcll(row_u) >= max_parents) &&
                !(forb_u & c.self))
                f(2, u, d_v + (t_uv - L_u));
        }
    }
}

// the best (delta, code) of the wave, in every lane
__device__ __forceinline__ void hc_reduce_best(double& best, int& bcode, int lane) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double od = dvs_shfl_xor(best, lane, s);
        const int oc = dvs_shfl_xor(bcode, lane, s);
        hc_consider(od, oc, best, bcode);
    }
}

// applies the move `code`: the rows, local from the toggle table, the two worklist slots
__device__ __forceinline__ void hc_apply(const HcLane& c, int code, uint64_t* parents, double* local, const double* T, size_t base,
                                         int* worklist, int b) {
    const int n = c.n, nn = n * n;
    const int op = code / nn, v = (code % nn) / n, u = code % n;
    if (c.lane == v) {
        parents[base + v] = c.row ^ (1ull << u);
        local[base + v] = T[v * n + u];
    }
    if (op == 2 && c.lane == u) {
        parents[base + u] = c.row | (1ull << v);
        local[base + u] = T[u * n + v];
    }
    if (c.lane == 0) {
        worklist[2 * b] = v;
        worklist[2 * b + 1] = op == 2 ? u : -1;
    }
}

__global__ __launch_bounds__(256) void k_hc_step(HcArgs a) {
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
    double best = -__builtin_inf();
    int bcode = HC_NO_MOVE;
    hc_moves(c, T, a.max_parents, a.forbidden, [&](int op, int u, double d) { hc_consider(d, op * nn + lane * n + u, best, bcode); });
    hc_reduce_best(best, bcode, lane);
    if (bcode != HC_NO_MOVE && best > a.min_delta) {
        hc_apply(c, bcode, a.parents, a.local, T, base, a.worklist, b);
        if (lane == 0) hc_record(a, b, nsteps, bcode, best);
    } else {
        if (lane == 0) a.converged[b] = 1;
        hc_sit_out(0, lane, b, a.flags, a.worklist);
    }
}

void dvs_launch_hc_step(const HcArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_hc_step, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}
