// Learning from incomplete data on a fitted discrete Bayesian network (definitions in
// include/dvs_incomplete.h): the expected counts of one EM step, the tables from such counts, and exact imputation.  Included by
// k_bic.hip after dvs_eliminate.h, whose plan check (bn_elim_plan_ok), step executor (bn_elim_steps) and z tree it reuses.  fp64
// in the linear domain with contraction off, every sum in a stated order; the atomics are the status atomicOr and integer adds
// (the counts of wholly observed families, the skipped rows): two runs give equal bytes, and the bytes do not depend on the
// rows per group or on the grid.
//
//   k_bn_inc_check     one workgroup per plan: k_bn_elim_check's checks, and the kept variables are what the slot asks for.
//   k_bn_inc_evidence  one workgroup per chunk of 256 rows: the evidence plan on every sound row, G rows at a time -> row_z, the
//                      rows' ok flags, the chunk's log-likelihood partial and skipped rows.
//   k_bn_inc_counts    one workgroup per (family, chunk): wholly observed ok rows are counted in an integer histogram in LDS
//                      (flushed with integer atomics); the others are compacted in ascending order and eliminated G at a
//                      time, arena and last step in LDS; the thread that owns a cell adds the quotients in row order, in a
//                      register over the whole chunk (its first four cells; beyond 1024 cells in the chunk's partial).
//   k_bn_inc_finish    the fixed tree over the chunk partials of four cells per workgroup, I + F; the last workgroup reduces
//                      the log-likelihood and the skipped rows.
//   k_bn_inc_impute    one workgroup per (variable, chunk): the rows that miss the variable, G at a time -> u8 levels.
//   k_bn_inc_pack      one thread per row: observed nibbles copied, imputed levels packed, observed_out.
//   k_bn_fit_counts    one workgroup per variable: the arithmetic of k_bn_fit on fp64 counts.
#pragma once
#include "dvs_eliminate.h"

constexpr size_t BN_INC_LDS_BUDGET = 148 * 1024;             // dynamic LDS of a workgroup: the cap's 128 KiB + 16 KiB of words fit at G = 1;
                                                             // the static arrays stay below 12 KiB (160 KiB per workgroup on gfx950)

__device__ __forceinline__ bool bn_inc_positive(const double z) { return z > 0.0 && z <= 1.7976931348623157e308; }

__global__ __launch_bounds__(256) void k_bn_inc_check(BnIncArgs a) {
    __shared__ int s_ok;
    __shared__ long long s_size[48];
    const int tid = threadIdx.x, n = a.e.n, p = blockIdx.x;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    bn_elim_family_ok(a.e, tid, s_size, &s_ok);
    __syncthreads();
    if (tid == 0) {
        bool ok = s_ok != 0 && bn_elim_plan_ok(a.e, p, s_size);
        if (ok) {                                            // the slot's kept variables: the family, {v}, or nothing
            const int* w = a.e.plans + a.e.plan_offsets[p];
            const uint64_t want = p == n ? 0ull : a.impute ? 1ull << p : a.e.parents[p] | (1ull << p);
            uint64_t have = 0ull;
            for (int i = 0; i < w[5]; ++i) have |= 1ull << w[6 + i];
            // ... and the last step's cells are the slot's: the table of the family, the levels of v, one cell.  The kept list
            // and the last step's scope are separate words; a last step over more cells would leave the table (k_bn_inc_counts)
            // or offer a level at or above card (k_bn_inc_impute).
            const long long cells = p == n ? 1 : a.impute ? (long long)a.e.card[p] : s_size[p];
            ok = have == want && w[4] == cells;
        }
        a.e.plan_flags[p] = ok ? 0 : 1;
        if (!ok) atomicOr(a.e.status, 16);
    }
}

// no observed bit at or above n, every observed level below its variable's level count
__device__ __forceinline__ bool bn_inc_row_sound(const BnRow& x, const uint64_t obs, const int n, const unsigned char* s_card) {
    if (obs >> n) return false;
    for (uint64_t m = obs; m; m &= m - 1ull) {
        const int v = dvs_ctz64(m);
        if (bn_level(x, v) >= s_card[v]) return false;
    }
    return true;
}

// The workgroup's dynamic LDS: G arenas, G last steps, the plan's words, G mask rows.
struct BnIncLds {
    double* arena;               // [G][arena_cells]
    double* outl;                // [G][out_stride]
    int* w;                      // [plan_words]
    uint16_t* masks;             // [G][n]
};
__device__ __forceinline__ BnIncLds bn_inc_lds(const BnIncArgs& a, char* smem) {
    BnIncLds l;
    l.arena = (double*)smem;
    l.outl = l.arena + (size_t)a.e.G * a.e.arena_cells;
    l.w = (int*)(l.outl + (size_t)a.e.G * a.e.out_stride);
    l.masks = (uint16_t*)(l.w + a.e.plan_words);
    return l;
}
static inline size_t bn_inc_lds_bytes(const BnIncArgs& a, int G) {
    return (size_t)G * ((size_t)a.e.arena_cells + a.e.out_stride) * 8 + (size_t)a.e.plan_words * 4 + (size_t)G * a.e.n * 2;
}

// stages plan p's words, the level counts and the table bases; a barrier follows in the caller
__device__ __forceinline__ void bn_inc_stage(const BnIncArgs& a, const int p, int* w, unsigned char* s_card, long long* s_base, const int tid) {
    const long long lo = a.e.plan_offsets[p];
    const int len = (int)(a.e.plan_offsets[p + 1] - lo);
    for (int i = tid; i < len; i += 256) w[i] = a.e.plans[lo + i];
    if (tid < a.e.n) {
        s_card[tid] = a.e.card[tid];
        s_base[tid] = a.e.offsets[tid];
    }
}

// The chunk's active rows in ascending order: list[i] = the thread (row within the chunk) of the i-th; returns their number.
// Every thread calls it; it ends with a barrier.
__device__ __forceinline__ int bn_inc_compact(const bool active, unsigned char* list, int* s_wave, const int tid) {
    const unsigned long long b = __ballot(active ? 1 : 0);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < 4; ++i) {
        if (i < wave) before += s_wave[i];
        total += s_wave[i];
    }
    if (active) list[before + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned char)tid;
    __syncthreads();
    return total;
}

// One group: the masks of the rows list[0 .. rows) of the chunk that starts at row0 are built in LDS, the plan's steps run with
// the last step's cells in l.outl [rows][outc], and s_z[g] is the fixed tree over row g's cells.  Ends with a barrier.
__device__ __forceinline__ void bn_inc_group(const BnIncArgs& a, const BnIncLds& l, const unsigned char* list, const int rows,
                                             const long long row0, double* red, double* s_z, const unsigned char* s_card,
                                             const long long* s_base, const int tid) {
    const int n = a.e.n, outc = l.w[4];
    for (int idx = tid; idx < rows * n; idx += 256) {
        const int g = idx / n, v = idx - g * n;
        const long long row = row0 + list[g];
        const uint64_t word = a.data[(size_t)row * a.words + (v >> 4)];
        l.masks[idx] = (a.observed[row] >> v) & 1ull ? (uint16_t)(1u << ((word >> (4 * (v & 15))) & 15ull)) : (uint16_t)0xFFFF;
    }
    __syncthreads();
    bn_elim_steps(l.w, l.w[2], rows, a.e.arena_cells, l.arena, l.masks, n, s_card, s_base, a.e.cpt, l.outl, outc, tid);
    for (int r0 = 0; r0 < rows; r0 += BN_ELIM_ZBATCH) {
        const int nb = rows - r0 < BN_ELIM_ZBATCH ? rows - r0 : BN_ELIM_ZBATCH;
        for (int b = 0; b < nb; ++b) {
            double sum = 0.0;
            for (int c = tid; c < outc; c += 256) sum += l.outl[(size_t)(r0 + b) * outc + c];
            red[b * 256 + tid] = sum;
        }
        __syncthreads();
        bn_lw_tree(red, nb, tid);
        if (tid < nb) s_z[r0 + tid] = red[tid * 256];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bn_inc_evidence(BnIncArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[BN_ELIM_ZBATCH * 256];
    __shared__ double s_z[64], s_rowz[256];
    __shared__ long long s_base[48];
    __shared__ unsigned char s_card[48], s_list[256];
    __shared__ int s_wave[4], s_flags, s_skip;
    const int tid = threadIdx.x, n = a.e.n, chunk = blockIdx.x;
    const long long row0 = (long long)chunk * 256, row = row0 + tid;
    const bool in = row < a.e.rows;
    if (a.e.plan_flags[n]) {                                 // uniform: no evidence plan, no row is ok
        if (in) {
            a.row_z[row] = bn_nan();
            a.row_ok[row] = 0;
        }
        return;
    }
    const BnIncLds l = bn_inc_lds(a, smem);
    bn_inc_stage(a, n, l.w, s_card, s_base, tid);
    if (tid == 0) s_flags = s_skip = 0;
    __syncthreads();
    const BnRow x = in ? bn_row_load(a.data + (size_t)row * a.words, a.words) : BnRow{0ull, 0ull, 0ull};
    const bool sound = in && bn_inc_row_sound(x, a.observed[row], n, s_card);
    const int active = bn_inc_compact(sound, s_list, s_wave, tid);
    for (int g0 = 0; g0 < active; g0 += a.e.G) {
        const int rows = active - g0 < a.e.G ? active - g0 : a.e.G;
        bn_inc_group(a, l, s_list + g0, rows, row0, red, s_z, s_card, s_base, tid);
        if (tid < rows) s_rowz[s_list[g0 + tid]] = s_z[tid];
        __syncthreads();
    }
    double term = 0.0;
    if (in) {
        const double z = sound ? s_rowz[tid] : bn_nan();
        const bool ok = sound && bn_inc_positive(z);
        a.row_z[row] = z;
        a.row_ok[row] = ok ? 1 : 0;
        if (ok) term = log(z);
        else {
            atomicOr(&s_flags, sound ? 128 : 16);
            atomicAdd(&s_skip, 1);
        }
    }
    red[tid] = term;
    __syncthreads();
    dvs_block_sum256(tid, red);
    if (tid == 0) {
        a.ll_partials[chunk] = red[0];
        a.skip_partials[chunk] = s_skip;
        if (s_flags) atomicOr(a.e.status, s_flags);
    }
}

constexpr int BN_INC_ACC = 4;                                // cells a thread of k_bn_inc_counts accumulates in registers

// the table cell j = key * r + k of the family plan's cell c (lowest id fastest over fam = {v} and its parents)
__device__ __forceinline__ int bn_inc_table_cell(const int c, const uint64_t fam, const int v, const int r, const unsigned char* s_card) {
    int j = 0, stride = r, rem = c;
    for (uint64_t m = fam; m; m &= m - 1ull) {
        const int u = dvs_ctz64(m), cd = s_card[u], lu = rem % cd;
        rem /= cd;
        if (u == v) j += lu;
        else {
            j += lu * stride;
            stride *= cd;
        }
    }
    return j;
}

__global__ __launch_bounds__(256) void k_bn_inc_counts(BnIncArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[BN_ELIM_ZBATCH * 256];
    __shared__ double s_z[64];
    __shared__ long long s_base[48];
    __shared__ unsigned char s_card[48], s_list[256];
    __shared__ int s_wave[4], s_flags;
    const int tid = threadIdx.x, n = a.e.n;
    const int v = blockIdx.x / a.chunks, chunk = blockIdx.x - v * a.chunks;
    if (a.e.plan_flags[v] || a.e.plan_flags[n]) return;     // uniform: k_bn_inc_finish writes this family's NaN
    const BnIncLds l = bn_inc_lds(a, smem);
    bn_inc_stage(a, v, l.w, s_card, s_base, tid);
    if (tid == 0) s_flags = 0;
    __syncthreads();
    const int outc = l.w[4], r = s_card[v];
    const uint64_t pm = a.e.parents[v] & ~(1ull << v), fam = pm | (1ull << v);
    const long long base = s_base[v] - s_base[0];
    double* part = a.partials + (size_t)chunk * a.e.n_cells + base;
    int* hist = (int*)smem;                                  // outc counters where the arenas will lie
    for (int j = tid; j < outc; j += 256) {
        part[j] = 0.0;
        hist[j] = 0;
    }
    __syncthreads();
    const long long row0 = (long long)chunk * 256, row = row0 + tid;
    const bool ok = row < a.e.rows && a.row_ok[row] != 0;
    const uint64_t obs = ok ? a.observed[row] : 0ull;
    if (ok && !(fam & ~obs)) {                               // the whole family observed: an integer count
        const BnRow x = bn_row_load(a.data + (size_t)row * a.words, a.words);
        atomicAdd(&hist[bn_row_config(x, pm, s_card) * r + bn_level(x, v)], 1);
    }
    const int active = bn_inc_compact(ok && (fam & ~obs) != 0ull, s_list, s_wave, tid);
    for (int j = tid; j < outc; j += 256)
        if (hist[j]) atomicAdd(a.icounts + base + j, hist[j]);
    __syncthreads();
    // The thread that owns the plan's cell c adds the quotients of c in row order.  Its first BN_INC_ACC cells (c = tid + 256 k)
    // stay in registers over all groups and are stored once; a table of more than 256 * BN_INC_ACC cells keeps the rest in the
    // chunk's partial, one read-modify-write per cell and group.
    double acc[BN_INC_ACC];
    int cell_j[BN_INC_ACC];
#pragma unroll
    for (int k = 0; k < BN_INC_ACC; ++k) {
        acc[k] = 0.0;
        cell_j[k] = tid + 256 * k < outc ? bn_inc_table_cell(tid + 256 * k, fam, v, r, s_card) : 0;
    }
    for (int g0 = 0; g0 < active; g0 += a.e.G) {
        const int rows = active - g0 < a.e.G ? active - g0 : a.e.G;
        bn_inc_group(a, l, s_list + g0, rows, row0, red, s_z, s_card, s_base, tid);
        {
#pragma clang fp contract(off)
            for (int g = 0; g < rows; ++g) {
                const double z = s_z[g];
                if (!bn_inc_positive(z)) {
                    if (tid == 0) atomicOr(&s_flags, 128);
                    continue;
                }
                const double* cells = l.outl + (size_t)g * outc;
#pragma unroll
                for (int k = 0; k < BN_INC_ACC; ++k)
                    if (tid + 256 * k < outc) acc[k] += cells[tid + 256 * k] / z;
            }
            for (int c = tid + 256 * BN_INC_ACC; c < outc; c += 256) {
                const int j = bn_inc_table_cell(c, fam, v, r, s_card);
                double far = part[j];
                for (int g = 0; g < rows; ++g)
                    if (bn_inc_positive(s_z[g])) far += l.outl[(size_t)g * outc + c] / s_z[g];
                part[j] = far;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < BN_INC_ACC; ++k)
        if (tid + 256 * k < outc) part[cell_j[k]] = acc[k];
    if (tid == 0 && s_flags) atomicOr(a.e.status, s_flags);
}

__global__ __launch_bounds__(256) void k_bn_inc_finish(BnIncArgs a) {
    __shared__ double red[BN_ELIM_ZBATCH * 256];
    __shared__ long long s_skip[256];
    const int tid = threadIdx.x, n = a.e.n;
    const long long cells = a.e.n_cells;
    const bool none = a.e.plan_flags[n] != 0;                // no evidence plan: nothing was counted
    if ((long long)blockIdx.x * BN_ELIM_ZBATCH >= cells) {   // the last workgroup: the log-likelihood, the skipped rows
        double s = 0.0;
        long long k = 0;
        if (!none)
            for (int c = tid; c < a.chunks; c += 256) {
                s += a.ll_partials[c];
                k += a.skip_partials[c];
            }
        red[tid] = s;
        s_skip[tid] = k;
        __syncthreads();
        dvs_block_sum256(tid, red, s_skip);
        if (tid == 0) {
            a.loglik[0] = none ? bn_nan() : red[0];
            a.skipped[0] = none ? a.e.rows : s_skip[0];
        }
        return;
    }
    const long long j0 = (long long)blockIdx.x * BN_ELIM_ZBATCH;
    const int nb = cells - j0 < BN_ELIM_ZBATCH ? (int)(cells - j0) : BN_ELIM_ZBATCH;
    for (int b = 0; b < nb; ++b) {
        double s = 0.0;
        for (int c = tid; c < a.chunks; c += 256) s += a.partials[(size_t)c * cells + j0 + b];
        red[b * 256 + tid] = s;
    }
    __syncthreads();
    bn_lw_tree(red, nb, tid);
    if (tid < nb) {
        const long long j = j0 + tid;
        int v = 0;
        while (v < n - 1 && j >= a.e.offsets[v + 1] - a.e.offsets[0]) ++v;
        a.counts[j] = none || a.e.plan_flags[v] ? bn_nan() : (double)a.icounts[j] + red[tid * 256];
    }
}

void dvs_launch_bn_expected_counts(const BnIncArgs& in, dvs_stream_t st) {
    BnIncArgs a = in;
    a.words = bic_words(a.e.n);
    a.impute = 0;
    int G = a.e.rows_per_group;
    if (G == 0) {                                            // the rule of dvs_launch_bn_eliminate
        G = 1024 / a.e.step_cells;
        G = G < 1 ? 1 : G > 64 ? 64 : G;
    }
    while (G > 1 && bn_inc_lds_bytes(a, G) > BN_INC_LDS_BUDGET) --G;
    a.e.G = G;
    const size_t lds = bn_inc_lds_bytes(a, G);
    // The evidence pass has one workgroup per chunk only, so its rows in flight come from G: under the rule it takes at least 8
    // (band48, 65 536 rows: 26.0 ms at G = 1, 10.5 ms at G = 8, 10.2 ms at G = 16 .. 64).
    BnIncArgs ev = a;
    if (a.e.rows_per_group == 0 && G < 8) {
        ev.e.G = 8;
        while (ev.e.G > 1 && bn_inc_lds_bytes(ev, ev.e.G) > BN_INC_LDS_BUDGET) --ev.e.G;
    }
    const size_t ev_lds = bn_inc_lds_bytes(ev, ev.e.G);
    const unsigned cell_blocks = (unsigned)((a.e.n_cells + BN_ELIM_ZBATCH - 1) / BN_ELIM_ZBATCH);
    (void)hipMemsetAsync(a.icounts, 0, (size_t)a.e.n_cells * 4, st);
    DVS_LAUNCH(k_bn_inc_check, dim3((unsigned)a.e.P), dim3(256), 0, st, a);
    DVS_SET_LDS(k_bn_inc_evidence, ev_lds);
    DVS_LAUNCH(k_bn_inc_evidence, dim3((unsigned)a.chunks), dim3(256), ev_lds, st, ev);
    DVS_SET_LDS(k_bn_inc_counts, lds);
    DVS_LAUNCH(k_bn_inc_counts, dim3((unsigned)a.e.n * (unsigned)a.chunks), dim3(256), lds, st, a);
    DVS_LAUNCH(k_bn_inc_finish, dim3(cell_blocks + 1), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_bn_inc_impute, k_bn_inc_pack
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_inc_impute(BnIncArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[BN_ELIM_ZBATCH * 256];
    __shared__ double s_z[64];
    __shared__ long long s_base[48];
    __shared__ unsigned char s_card[48], s_list[256];
    __shared__ int s_wave[4], s_flags;
    const int tid = threadIdx.x, n = a.e.n;
    const int v = blockIdx.x / a.chunks, chunk = blockIdx.x - v * a.chunks;
    const long long row0 = (long long)chunk * 256, row = row0 + tid;
    const bool in = row < a.e.rows, flagged = a.e.plan_flags[v] != 0;
    const BnIncLds l = bn_inc_lds(a, smem);
    if (!flagged) bn_inc_stage(a, v, l.w, s_card, s_base, tid);
    else if (tid < n) s_card[tid] = a.e.card[tid];
    if (tid == 0) s_flags = 0;
    __syncthreads();
    const uint64_t obs = in ? a.observed[row] : ~0ull;
    const bool missing = in && !((obs >> v) & 1ull);
    const bool active = missing && !flagged && bn_inc_row_sound(bn_row_load(a.data + (size_t)row * a.words, a.words), obs, n, s_card);
    if (missing && !active) a.levels[(size_t)row * n + v] = 255;
    if (flagged) return;                                     // uniform
    const int total = bn_inc_compact(active, s_list, s_wave, tid);
    for (int g0 = 0; g0 < total; g0 += a.e.G) {
        const int rows = total - g0 < a.e.G ? total - g0 : a.e.G;
        bn_inc_group(a, l, s_list + g0, rows, row0, red, s_z, s_card, s_base, tid);
        if (tid < rows) {
            const int outc = l.w[4];
            int best = 255;
            if (bn_inc_positive(s_z[tid])) {
                best = 0;
                for (int k = 1; k < outc; ++k)
                    if (l.outl[(size_t)tid * outc + k] > l.outl[(size_t)tid * outc + best]) best = k;
            } else {
                atomicOr(&s_flags, 128);
            }
            a.levels[(size_t)(row0 + s_list[g0 + tid]) * n + v] = (unsigned char)best;
        }
        __syncthreads();
    }
    if (tid == 0 && s_flags) atomicOr(a.e.status, s_flags);
}

__global__ __launch_bounds__(256) void k_bn_inc_pack(BnIncArgs a) {
    __shared__ unsigned char s_card[48];
    __shared__ int s_flags;
    const int tid = threadIdx.x, n = a.e.n;
    if (tid < n) s_card[tid] = a.e.card[tid];
    if (tid == 0) s_flags = 0;
    __syncthreads();
    const long long row = (long long)blockIdx.x * 256 + tid;
    if (row < a.e.rows) {
        const BnRow x = bn_row_load(a.data + (size_t)row * a.words, a.words);
        const uint64_t obs = a.observed[row];
        if (!bn_inc_row_sound(x, obs, n, s_card)) atomicOr(&s_flags, 16);
        BnRow y = {0ull, 0ull, 0ull};
        uint64_t seen = obs;
        for (int v = 0; v < n; ++v) {
            int level = bn_level(x, v);
            if (!((obs >> v) & 1ull)) {
                level = a.levels[(size_t)row * n + v];
                if (level == 255) continue;
                seen |= 1ull << v;
            }
            y = bn_row_with(y, v, (uint64_t)level);
        }
        bn_row_store(a.data_out + (size_t)row * a.words, y, a.words);
        a.observed_out[row] = seen;
    }
    __syncthreads();
    if (tid == 0 && s_flags) atomicOr(a.e.status, s_flags);
}

void dvs_launch_bn_impute(const BnIncArgs& in, dvs_stream_t st) {
    BnIncArgs a = in;
    a.words = bic_words(a.e.n);
    a.impute = 1;
    int G = a.e.rows_per_group;
    if (G == 0) {
        G = 1024 / a.e.step_cells;
        G = G < 1 ? 1 : G > 64 ? 64 : G;
    }
    while (G > 1 && bn_inc_lds_bytes(a, G) > BN_INC_LDS_BUDGET) --G;
    a.e.G = G;
    const size_t lds = bn_inc_lds_bytes(a, G);
    DVS_LAUNCH(k_bn_inc_check, dim3((unsigned)a.e.P), dim3(256), 0, st, a);
    DVS_SET_LDS(k_bn_inc_impute, lds);
    DVS_LAUNCH(k_bn_inc_impute, dim3((unsigned)a.e.n * (unsigned)a.chunks), dim3(256), lds, st, a);
    DVS_LAUNCH(k_bn_inc_pack, dim3((unsigned)a.chunks), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_bn_fit_counts
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_fit_counts(BnFitCountsArgs a) {
    __shared__ int s_q, s_bad;
    const int v = blockIdx.x, tid = threadIdx.x;
    const int r = a.card[v];
    const long long lo = a.offsets[v] - a.offsets[0], hi = a.offsets[v + 1] - a.offsets[0];
    if (tid == 0) {
        long long q = 0;
        const int np = bn_family_layout<false>(a.parents[v] & ~(1ull << v), a.n, a.card, r, 0x7fffffffLL, nullptr, nullptr, &q);
        s_q = np >= 0 && r >= 1 && r <= 16 && lo >= 0 && hi - lo == q * r && hi <= a.n_cells ? (int)q : -1;
        s_bad = 0;
    }
    __syncthreads();
    const int q = s_q;
    if (q < 0) {                                             // the slot itself is unsound: nothing of it is touched
        if (tid == 0) atomicOr(a.status, 16);
        return;
    }
    const double* cnt = a.counts + lo;
    double* out = a.cpt + lo;
    int bad = 0;
    for (long long i = tid; i < (long long)q * r; i += 256)
        if (!(cnt[i] >= 0.0 && cnt[i] <= 1.7976931348623157e308)) bad = 1;
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (s_bad) {
        for (long long i = tid; i < (long long)q * r; i += 256) out[i] = bn_nan();
        if (tid == 0) atomicOr(a.status, 16);
        return;
    }
    {
#pragma clang fp contract(off)
        const double dr = (double)r;
        const double alpha = a.method == 1 ? a.iss / (dr * (double)q) : 0.0;
        const double ralpha = dr * alpha;
        for (int j = tid; j < q; j += 256) {
            double dn = 0.0;
            for (int k = 0; k < r; ++k) dn += cnt[(size_t)j * r + k];
            for (int k = 0; k < r; ++k) {
                const double c = cnt[(size_t)j * r + k];
                double th;
                if (a.method == 1) th = (c + alpha) / (dn + ralpha);
                else if (dn != 0.0) th = c / dn;
                else th = a.unobserved ? 1.0 / dr : bn_nan();
                out[(size_t)j * r + k] = th;
            }
        }
    }
}

void dvs_launch_bn_fit_counts(const BnFitCountsArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_bn_fit_counts, dim3((unsigned)a.n), dim3(256), 0, st, a);
}
