// Exact inference on a fitted discrete Bayesian network by bucket (variable) elimination (definitions and the
// plan words in include/dvs_eliminate.h).  Included by k_bic.hip after dvs_infer.h, whose reduction tree (bn_lw_tree) it
// reuses.  The plan is built on the host (dags_vae_search_amd/eliminate.py); the kernels execute its words.  fp64 in the
// linear domain with contraction off, every sum in a stated order, no atomics but the status atomicOr: two runs give equal
// bytes, and the bytes do not depend on the rows per workgroup or on the grid.
//
//   k_bn_elim_check   one workgroup per plan.  Lanes 0..n-1 check the network's families (as k_bn_blanket does), then lane 0
//                     walks the plan's words once with every read bounded by the plan's length: a plan that passes can be
//                     executed without a further check.  A plan that does not is marked (plan_flags) and sets bit 4.
//   k_bn_eliminate    a 256-thread workgroup owns (plan, group of G rows).  The plan's words, the level counts and the table
//                     bases are staged in LDS once; each row of the group has an arena of arena_cells doubles in dynamic LDS
//                     (the call's need, not the cap).  Per step the threads stride over (row in group, output cell); a
//                     barrier separates steps.  The tables are read from global memory through the cache (a copy in LDS
//                     measured no faster on asia and 42 % slower on a 48-variable network).  z is the fixed
//                     tree over the cells of the last step, BN_ELIM_ZBATCH rows per pass.
//   bn_elim_family_ok, bn_elim_plan_ok, bn_elim_steps   the family check, the word walk and the step executor as device functions:
//                     dvs_incomplete.h builds its kernels on the same three.
#pragma once
#include "dvs_infer.h"

constexpr int BN_ELIM_ZBATCH = 4;                            // rows whose z is reduced per pass: 4 * 256 doubles = 8 KiB of LDS

// the plan's words, read by one lane: true when every access k_bn_eliminate will make stays inside the tables, the arena and
// out.  size[v]: the cells of variable v's table (the families were checked before this is called).
__device__ inline bool bn_elim_plan_ok(const BnElimArgs& a, const int p, const long long* size) {
    const long long lo = a.plan_offsets[p], hi = a.plan_offsets[p + 1];
    if (lo < 0 || hi > a.plans_words || hi - lo < 7 || hi - lo > a.plan_words) return false;
    const int* w = a.plans + lo;
    const int len = (int)(hi - lo), n = a.n;
    if (w[0] != DVS_BN_ELIM_TAG || w[1] != n) return false;
    const int steps = w[2], arena = w[3], outc = w[4], nk = w[5];
    if (steps < 1 || arena < 1 || arena > a.arena_cells || outc < 1 || outc > a.out_stride || nk < 0 || nk > DVS_BN_ELIM_MAX_SCOPE)
        return false;
    int cur = 6;
    if (cur + nk > len) return false;
    for (int i = 0, prev = -1; i < nk; ++i) {
        const int v = w[cur + i];
        if (v <= prev || v >= n) return false;
        prev = v;
    }
    cur += nk;
    for (int s = 0; s < steps; ++s) {
        if (cur + 5 > len) return false;
        const int x = w[cur], off = w[cur + 1], cells = w[cur + 2], ns = w[cur + 3], ni = w[cur + 4];
        const bool last = s == steps - 1;
        if (last ? (x != -1 || off != -1 || cells != outc)
                 : (x < 0 || x >= n || off < 0 || cells < 1 || (long long)off + cells > arena))
            return false;
        if (ns < 0 || ns > DVS_BN_ELIM_MAX_SCOPE || ni < 1 || ni > DVS_BN_ELIM_MAX_INPUTS) return false;
        const int need = ns + ni * (4 + ns);                 // <= 16 + 64 * 20
        if (cur + 5 + need > len) return false;
        const int* sc = w + cur + 5;
        long long prod = 1;
        for (int i = 0, prev = -1; i < ns; ++i) {
            const int v = sc[i];
            if (v <= prev || v >= n || v == x) return false;
            prev = v;
            prod *= a.card[v];
            if (prod > 0x7fffffffLL) return false;
        }
        if (prod != cells) return false;
        const int cx = last ? 1 : a.card[x];
        for (int j = 0; j < ni; ++j) {
            const int* in = sc + ns + j * (4 + ns);
            const int kind = in[0], ioff = in[1], icells = in[2], sx = in[3];
            long long span;
            if (kind >= 0) {
                if (kind >= n) return false;
                span = size[kind];
            } else if (kind == -1) {
                if (ioff < 0 || icells < 1 || (long long)ioff + icells > arena) return false;
                if (!last && ioff < off + cells && off < ioff + icells) return false;        // the output overlaps an input
                span = icells;
            } else {
                return false;
            }
            if (sx < 0) return false;
            long long reach = (long long)sx * (cx - 1);
            for (int i = 0; i < ns; ++i) {
                const int st = in[4 + i];
                if (st < 0) return false;
                reach += (long long)st * (a.card[sc[i]] - 1);
            }
            if (reach >= span) return false;
        }
        cur += 5 + need;
    }
    return cur == len;
}

// the network's families, one lane each (as k_bn_blanket checks them): a family that fails clears *s_ok; size[v] = the cells of
// variable v's table.  The caller sets *s_ok and puts a barrier on either side.
__device__ __forceinline__ void bn_elim_family_ok(const BnElimArgs& a, const int tid, long long* size, int* s_ok) {
    const int n = a.n;
    if (tid < n) {
        const long long lo = a.offsets[tid], hi = a.offsets[tid + 1], r = a.card[tid], first = a.offsets[0];
        const uint64_t pm = a.parents[tid] & ~(1ull << tid);
        bool ok = r >= 1 && r <= 16 && !(n < 64 && (pm >> n)) && lo >= first && hi <= first + a.n_cells;
        long long q = 1;
        for (uint64_t m = pm; m && ok; m &= m - 1ull) {
            q *= a.card[dvs_ctz64(m)];
            ok = q * r <= 0x7fffffffLL;
        }
        if (!ok || hi - lo != q * r) *s_ok = 0;
        size[tid] = hi - lo;
    }
}

__global__ __launch_bounds__(256) void k_bn_elim_check(BnElimArgs a) {
    __shared__ int s_ok;
    __shared__ long long s_size[48];
    const int tid = threadIdx.x, p = blockIdx.x;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    bn_elim_family_ok(a, tid, s_size, &s_ok);
    __syncthreads();
    if (tid == 0) {
        const bool ok = s_ok != 0 && bn_elim_plan_ok(a, p, s_size);
        a.plan_flags[p] = ok ? 0 : 1;
        if (!ok) atomicOr(a.status, 16);
    }
}

// The step executor, shared with dvs_incomplete.h: every thread of the 256-thread workgroup calls it with the plan's checked
// words `w` (in LDS) and their step count, `rows` rows whose arenas lie `arena_cells` apart behind `arena`, their level masks [rows][n] and the
// staged level counts and table bases.  The last step writes row r's cells to out[r * out_stride + c]: global memory for
// k_bn_eliminate, LDS for the kernels of dvs_incomplete.h.  It ends with the barrier behind the last step.
__device__ __forceinline__ void bn_elim_steps(const int* w, const int steps, const int rows, const int arena_cells, double* arena, const uint16_t* masks,
                                              const int n, const unsigned char* s_card, const long long* s_base, const double* cpt,
                                              double* out, const int out_stride, const int tid) {
    int cur = 6 + w[5];
    for (int s = 0; s < steps; ++s) {
        const int x = w[cur], off = w[cur + 1], cells = w[cur + 2], ns = w[cur + 3], ni = w[cur + 4], width = 4 + ns;
        const int* sc = w + cur + 5;
        const int* in0 = sc + ns;
        const int cx = x >= 0 ? s_card[x] : 1;
        for (int idx = tid; idx < rows * cells; idx += 256) {
            const int r = idx / cells, c = idx - r * cells;
            const uint16_t* m = masks + (size_t)r * n;
            const double* mine = arena + (size_t)r * arena_cells;
            uint64_t lv = 0ull;                              // the cell's levels, 4 bits per scope variable
            bool allowed = true;
            for (int i = 0, rem = c; i < ns; ++i) {
                const int cd = s_card[sc[i]], l = rem % cd;
                rem /= cd;
                lv |= (uint64_t)l << (4 * i);
                if (x < 0 && !((m[sc[i]] >> l) & 1)) allowed = false;      // the last step: a kept level the row does not allow
            }
            const unsigned mx = x >= 0 ? m[x] : 1u;
            double acc = 0.0;
            {
#pragma clang fp contract(off)
                for (int k = 0; k < cx && allowed; ++k) {
                    if (!((mx >> k) & 1u)) continue;
                    double pr = 0.0;
                    for (int j = 0; j < ni; ++j) {
                        const int* in = in0 + j * width;
                        int at = k * in[3];
                        for (int i = 0; i < ns; ++i) at += (int)((lv >> (4 * i)) & 15ull) * in[4 + i];
                        const double val = in[0] >= 0 ? cpt[s_base[in[0]] + at] : mine[in[1] + at];
                        pr = j == 0 ? val : pr * val;
                    }
                    acc += pr;
                }
            }
            if (x >= 0) arena[(size_t)r * arena_cells + off + c] = acc;
            else out[(size_t)r * out_stride + c] = acc;
        }
        cur += 5 + ns + ni * width;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bn_eliminate(BnElimArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[BN_ELIM_ZBATCH * 256];
    __shared__ long long s_base[48];
    __shared__ unsigned char s_card[48];
    const int tid = threadIdx.x, n = a.n;
    const int p = blockIdx.x / a.groups, g = blockIdx.x - p * a.groups;
    const long long row0 = (long long)g * a.G;
    const int rows = a.rows - row0 < a.G ? (int)(a.rows - row0) : a.G;
    double* out = a.out + ((size_t)p * a.rows + row0) * a.out_stride;
    double* z = a.z + (size_t)p * a.rows + row0;
    if (a.plan_flags[p]) {                                   // uniform: a malformed plan, nothing of it is read
        for (int i = tid; i < rows * a.out_stride; i += 256) out[i] = bn_nan();
        for (int i = tid; i < rows; i += 256) z[i] = bn_nan();
        return;
    }
    double* arena = (double*)smem;                           // [G][arena_cells]
    int* w = (int*)(smem + (size_t)a.G * a.arena_cells * 8);
    {
        const long long lo = a.plan_offsets[p];
        const int len = (int)(a.plan_offsets[p + 1] - lo);
        for (int i = tid; i < len; i += 256) w[i] = a.plans[lo + i];
    }
    if (tid < n) {
        s_card[tid] = a.card[tid];
        s_base[tid] = a.offsets[tid];
    }
    __syncthreads();
    const int steps = w[2], outc = w[4];
    bn_elim_steps(w, steps, rows, a.arena_cells, arena, a.masks + (size_t)row0 * n, n, s_card, s_base, a.cpt, out, a.out_stride, tid);
    const int pad = a.out_stride - outc;                     // the cells behind the last step's: +0
    for (int idx = tid; idx < rows * pad; idx += 256) {
        const int r = idx / pad;
        out[(size_t)r * a.out_stride + outc + (idx - r * pad)] = 0.0;
    }
    for (int r0 = 0; r0 < rows; r0 += BN_ELIM_ZBATCH) {      // the barrier above orders the last step's stores before these loads
        const int nb = rows - r0 < BN_ELIM_ZBATCH ? rows - r0 : BN_ELIM_ZBATCH;
        for (int b = 0; b < nb; ++b) {
            double sum = 0.0;
            for (int c = tid; c < outc; c += 256) sum += out[(size_t)(r0 + b) * a.out_stride + c];
            red[b * 256 + tid] = sum;
        }
        __syncthreads();
        bn_lw_tree(red, nb, tid);
        if (tid < nb) z[r0 + tid] = red[tid * 256];
        __syncthreads();
    }
}

void dvs_launch_bn_eliminate(const BnElimArgs& in, dvs_stream_t st) {
    BnElimArgs a = in;
    int G = a.rows_per_group;
    if (G == 0) {                                            // the library's rule: about 1024 output cells per step and workgroup
        G = 1024 / a.step_cells;
        G = G < 1 ? 1 : G > 64 ? 64 : G;
    }
    const int cap = DVS_BN_ELIM_MAX_CELLS / a.arena_cells;   // the arenas of a workgroup fit the cap
    if (G > cap) G = cap;
    if (G > a.rows) G = (int)a.rows;
    a.G = G;
    a.groups = (int)((a.rows + G - 1) / G);
    DVS_LAUNCH(k_bn_elim_check, dim3((unsigned)a.P), dim3(256), 0, st, a);
    const size_t lds = (size_t)G * a.arena_cells * 8 + (size_t)a.plan_words * 4;
    DVS_SET_LDS(k_bn_eliminate, lds);
    DVS_LAUNCH(k_bn_eliminate, dim3((unsigned)a.P * (unsigned)a.groups), dim3(256), lds, st, a);
}
