// Conditional Gaussian networks on mixed data, next to the discrete and the Gaussian scorers whose parts they
// join.  Included by k_bic.hip after dvs_gaussian_params.h.  Semantics, summation orders and refusals: include/dvs_mixed.h.
//
//   k_cg_partition       one 256-thread workgroup per (request, span of 4096 rows), a request being a set D of discrete
//                        variables: the configuration key of every row (bn_row_config) is counted into an LDS histogram with
//                        integer atomics, the counts are scanned, and the span's rows are placed tile by tile: in a tile of
//                        256 consecutive rows a thread's rank among the equal keys before it comes from 256 broadcast reads of
//                        the tile's keys in LDS, so the order is the stable sort's whatever the atomics did.  Integer work,
//                        bound by LDS reads; D = {} is the identity.
//   k_cg_slots           the chunks of a request are numbered configuration by configuration: the exclusive prefix of
//   k_cg_colsum          ceil(count / DVS_GBN_CHUNK).  k_cg_colsum and k_cg_cross take one workgroup per chunk slot, find the
//   k_cg_mean            slot's configuration by binary search in that prefix and hand the segment of `order` to the chunk
//   k_cg_cross           routines of dvs_gaussian.h (gbn_stage_rows, gbn_chunk_colsum, gbn_chunk_cross); k_cg_mean and
//   k_cg_fold            k_cg_fold add a configuration's chunk values in chunk order (gbn_fold_chunks).  One summation, two
//                        callers: a block is the bytes of dvs_gbn_moments on the segment.
//   k_cg_prep            the copy of the structures the discrete scorer runs on: rows of continuous variables and rows with an
//                        illegal arc are emptied, continuous variables count as one-level factors, worklist slots that name a
//                        continuous row are emptied.
//   k_cg_local           one lane per family (b, v) / per cell (row, u) as k_gbn_local and k_gbn_toggle: a continuous family runs
//   k_cg_toggle          gbn_family on every non-empty block of its table in ascending configuration and adds the terms in
//                        that order; a discrete family is left as the discrete scorer wrote it unless it holds an illegal arc.
//   k_cg_fit             one lane per (family, configuration): gbn_family, then gbn_backsolve, the backward solve of k_gbn_fit.
#pragma once
#include "dvs_bn_common.h"

static_assert(2 * DVS_CG_MAX_CONFIGS * sizeof(int) + 256 * sizeof(int) <= 64 * 1024, "the partition's histogram and cursors are static LDS");

// ---------------------------------------------------------------------------------------------------------
// Partition
// ---------------------------------------------------------------------------------------------------------
// q of the request D, or -1: a bit at or above n, a continuous variable, q > limit.  One thread calls it.
__device__ __forceinline__ int cg_request_configs(uint64_t D, int n, const uint8_t* card, int limit) {
    long long q = 1;
    for (uint64_t m = D; m; m &= m - 1ull) {
        const int p = dvs_ctz64(m);
        if (p >= n || card[p] == 0) return -1;
        q *= card[p];
        if (q > limit) return -1;
    }
    return (int)q;
}
// the configuration of row s; a level code at or above its level count counts as the top level, so the key stays below q
__device__ __forceinline__ int cg_row_key(const CgPartitionArgs& a, int s, uint64_t D, const unsigned char* card) {
    const BnRow x = bn_row_load(a.data + (size_t)s * a.words, a.words);
    int cfg = 0, stride = 1;
    for (uint64_t m = D; m; m &= m - 1ull) {
        const int p = dvs_ctz64(m), r = card[p];
        const int level = bn_level(x, p);
        cfg += (level < r ? level : r - 1) * stride;
        stride *= r;
    }
    return cfg;
}

// A request is cut into spans of CG_SPAN consecutive rows, a workgroup each (blockIdx.y).  Every workgroup of a request counts
// all S rows (a cheap pass) and, next to the total, the rows before its own span; after the scan its cursor of a key starts at
// start[key] + the key's rows before the span, and it places its own rows only.  No workgroup waits for another and nothing
// is exchanged through memory: the order is that of one workgroup walking all tiles.  Span 0 writes count and start.
constexpr int CG_SPAN = 4096;

__global__ __launch_bounds__(256) void k_cg_partition(CgPartitionArgs a) {
    __shared__ int s_count[DVS_CG_MAX_CONFIGS], s_cursor[DVS_CG_MAX_CONFIGS];
    __shared__ int s_key[256], s_part[256];
    __shared__ unsigned char s_card[DVS_WTOK];
    __shared__ int s_q;
    const int r = blockIdx.x, S = a.S, tid = threadIdx.x;
    const int lo = (int)blockIdx.y * CG_SPAN, hi = S - lo < CG_SPAN ? S : lo + CG_SPAN;      // the span [lo, hi): lo < S by the grid
    const bool first = blockIdx.y == 0;
    const uint64_t D = a.masks[r];
    if (tid < a.n) s_card[tid] = a.card[tid];
    if (tid == 0) s_q = cg_request_configs(D, a.n, a.card, a.q_pitch < DVS_CG_MAX_CONFIGS ? a.q_pitch : DVS_CG_MAX_CONFIGS);
    __syncthreads();
    const int q = s_q;
    int* count = a.count + (size_t)r * a.q_pitch;
    int* start = a.start + (size_t)r * a.q_pitch;
    int* order = a.order + (size_t)r * S;
    if (q < 0) {
        if (first && tid == 0) {
            atomicOr(a.status, 16);
            count[0] = -1;
        }
        return;
    }
    if (q == 1) {                                            // one configuration: the rows in order
        if (first)
            for (int z = tid; z < a.q_pitch; z += 256) {
                count[z] = z == 0 ? S : 0;
                start[z] = z == 0 ? 0 : S;
            }
        for (int s = lo + tid; s < hi; s += 256) order[s] = s;
        return;
    }
    for (int z = tid; z < q; z += 256) {
        s_count[z] = 0;
        s_cursor[z] = 0;                                     // until the scan: the key's rows before the span
    }
    __syncthreads();
    for (int s = tid; s < S; s += 256) {
        const int key = cg_row_key(a, s, D, s_card);
        atomicAdd(&s_count[key], 1);
        if (s < lo) atomicAdd(&s_cursor[key], 1);
    }
    __syncthreads();
    // exclusive scan: thread t owns the `per` consecutive configurations from t * per
    const int per = (q + 255) / 256;
    int mine = 0;
    for (int z = tid * per; z < (tid + 1) * per && z < q; ++z) mine += s_count[z];
    s_part[tid] = mine;
    __syncthreads();
    int at = 0;
    for (int t = 0; t < tid; ++t) at += s_part[t];           // 256 broadcast reads
    for (int z = tid * per; z < (tid + 1) * per && z < q; ++z) {
        s_cursor[z] += at;
        if (first) {
            start[z] = at;
            count[z] = s_count[z];
        }
        at += s_count[z];
    }
    if (first)
        for (int z = q + tid; z < a.q_pitch; z += 256) {
            count[z] = 0;
            start[z] = S;
        }
    __syncthreads();
    for (int base = lo; base < hi; base += 256) {
        const int s = base + tid, live = hi - base < 256 ? hi - base : 256;
        const int key = s < hi ? cg_row_key(a, s, D, s_card) : -1;
        s_key[tid] = key;
        __syncthreads();
        int before = 0, total = 0;
        if (key >= 0) {
            for (int j = 0; j < live; ++j) {
                const int same = s_key[j] == key ? 1 : 0;
                total += same;
                before += j < tid ? same : 0;
            }
            order[s_cursor[key] + before] = s;               // below start[key] + count[key]: inside the request's S slots
        }
        __syncthreads();
        if (key >= 0 && before == total - 1) s_cursor[key] += total;      // the tile's last row of this key moves the cursor
        __syncthreads();
    }
}

void dvs_launch_cg_partition(const CgPartitionArgs& in, dvs_stream_t st) {
    CgPartitionArgs a = in;
    a.words = bic_words(a.n);
    DVS_LAUNCH(k_cg_partition, dim3((unsigned)a.n_req, (unsigned)((a.S + CG_SPAN - 1) / CG_SPAN)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Ragged moments
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cg_count(const CgMomentArgs& a, int r, int z) {
    const int c = a.count[(size_t)r * a.q_pitch + z];
    return c < 0 || a.count[(size_t)r * a.q_pitch] < 0 ? 0 : c;          // a refused request: no rows anywhere
}
__device__ __forceinline__ int cg_chunks(int count) { return (count + DVS_GBN_CHUNK - 1) / DVS_GBN_CHUNK; }

__global__ __launch_bounds__(64) void k_cg_slots(CgMomentArgs a) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_req) return;
    int* pre = a.pre + (size_t)r * a.pre_pitch;
    int at = 0;
    for (int z = 0; z < a.q_pitch; ++z) {
        pre[z] = at;
        at += cg_chunks(cg_count(a, r, z));
        if (at > a.slots) at = a.slots;                      // counts that sum beyond S are not the partition's: stay in the workspace
    }
    pre[a.q_pitch] = at;
}

// the workgroup's slot -> its request and configuration; stages the segment's chunk into x and returns its length (0: no such
// slot, nothing staged).  Every thread of the workgroup calls it.
__device__ __forceinline__ int cg_stage_slot(const CgMomentArgs& a, double* x, int* r_out, int* z_out) {
    const int r = blockIdx.x / a.slots, slot = blockIdx.x - r * a.slots;
    const int* pre = a.pre + (size_t)r * a.pre_pitch;
    *r_out = r;
    if (slot >= pre[a.q_pitch]) return 0;
    int lo = 0, hi = a.q_pitch - 1;                          // the first z with pre[z + 1] > slot
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid + 1] > slot) hi = mid;
        else lo = mid + 1;
    }
    *z_out = lo;
    const int p0 = (slot - pre[lo]) * DVS_GBN_CHUNK, count = cg_count(a, r, lo);
    int first = a.start[(size_t)r * a.q_pitch + lo];
    int len = count - p0 < DVS_GBN_CHUNK ? count - p0 : DVS_GBN_CHUNK;
    if (first < 0 || p0 < 0 || len < 1 || (long long)first + p0 + len > (long long)a.S) return 0;    // not the partition's: read nothing
    gbn_stage_rows(a.x, a.n, a.order + (size_t)r * a.S + first + p0, 0, len, x);
    return len;
}

__global__ __launch_bounds__(256) void k_cg_colsum(CgMomentArgs a) {
    __shared__ double s_x[DVS_GBN_CHUNK * DVS_WTOK];
    int r, z;
    const int len = cg_stage_slot(a, s_x, &r, &z);
    if (len == 0) return;
    gbn_chunk_colsum(s_x, len, a.n, a.sums + (size_t)blockIdx.x * a.n);
}

__global__ __launch_bounds__(256) void k_cg_mean(CgMomentArgs a) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n = a.n;
    if (idx >= (long long)a.n_req * a.q_pitch * n) return;
    const int block = (int)(idx / n), i = (int)(idx - (long long)block * n);
    const int r = block / a.q_pitch, z = block - r * a.q_pitch;
    const int* pre = a.pre + (size_t)r * a.pre_pitch;
    const int count = cg_count(a, r, z);
    double* mom = a.moments + (size_t)block * DVS_GBN_STRIDE(n);
    const double m = (double)count;
    if (i == 0) mom[0] = z == 0 && a.count[(size_t)r * a.q_pitch] < 0 ? bn_nan() : m;
    if (count == 0) {
        mom[1 + i] = 0.0;
        return;
    }
    const double s = gbn_fold_chunks(a.sums + ((size_t)r * a.slots + pre[z]) * n + i, pre[z + 1] - pre[z], (size_t)n);
    mom[1 + i] = s / m;
}

__global__ __launch_bounds__(256) void k_cg_cross(CgMomentArgs a) {
    __shared__ double s_x[DVS_GBN_CHUNK * DVS_WTOK];
    int r, z;
    const int len = cg_stage_slot(a, s_x, &r, &z);
    if (len == 0) return;
    const double* mean = a.moments + ((size_t)r * a.q_pitch + z) * DVS_GBN_STRIDE(a.n) + 1;
    gbn_chunk_cross(s_x, len, a.n, a.tri, mean, a.cells + (size_t)blockIdx.x * a.tri);
}

__global__ __launch_bounds__(256) void k_cg_fold(CgMomentArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n = a.n;
    if (idx >= (long long)a.n_req * a.q_pitch * a.tri) return;
    const int block = (int)(idx / a.tri), q = (int)(idx - (long long)block * a.tri);
    const int r = block / a.q_pitch, z = block - r * a.q_pitch;
    const int* pre = a.pre + (size_t)r * a.pre_pitch;
    int i, j;
    gbn_tri_cell(q, n, &i, &j);
    // an empty configuration folds no chunk: +0
    const double s = gbn_fold_chunks(a.cells + ((size_t)r * a.slots + pre[z]) * a.tri + q, pre[z + 1] - pre[z], (size_t)a.tri);
    double* C = a.moments + (size_t)block * DVS_GBN_STRIDE(n) + 1 + n;
    C[i * n + j] = s;
    C[j * n + i] = s;
}

void dvs_launch_cg_moments(const CgMomentArgs& in, dvs_stream_t st) {
    CgMomentArgs a = in;
    const CgMomentLayout l = dvs_cg_moment_layout(a.n, a.S, a.n_req, a.q_pitch);
    a.slots = (int)l.slots;
    a.tri = (int)l.tri;
    a.pre_pitch = (int)l.pre_pitch;
    const dim3 per_slot((unsigned)(a.n_req * a.slots));
    const long long blocks = (long long)a.n_req * a.q_pitch;
    DVS_LAUNCH(k_cg_slots, dim3((unsigned)((a.n_req + 63) / 64)), dim3(64), 0, st, a);
    DVS_LAUNCH(k_cg_colsum, per_slot, dim3(256), 0, st, a);
    DVS_LAUNCH(k_cg_mean, dim3((unsigned)((blocks * a.n + 255) / 256)), dim3(256), 0, st, a);
    DVS_LAUNCH(k_cg_cross, per_slot, dim3(256), 0, st, a);
    DVS_LAUNCH(k_cg_fold, dim3((unsigned)((blocks * a.tri + 255) / 256)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// One family
// ---------------------------------------------------------------------------------------------------------
// the kinds of the variables as two masks; -1 when n_cont is not the number of continuous variables
struct CgKinds {
    uint64_t cont, disc;
    bool ok;
};
__device__ __forceinline__ CgKinds cg_kinds(const uint8_t* card, int n, int nc) {
    CgKinds k = {0ull, 0ull, false};
    for (int v = 0; v < n; ++v) {
        if (card[v] == 0) k.cont |= 1ull << v;
        else k.disc |= 1ull << v;
    }
    k.ok = __popcll(k.cont) == nc;
    return k;
}
// the bits of pm that are continuous variables -> bits over the columns of x (ascending variable order)
__device__ __forceinline__ uint64_t cg_columns(uint64_t pm, uint64_t cont) {
    uint64_t out = 0ull;
    for (uint64_t m = pm & cont; m; m &= m - 1ull) out |= 1ull << __popcll(cont & ((m & (0ull - m)) - 1ull));
    return out;
}

struct CgFamily {
    int q, p, vc;                // configurations, continuous parents, v's column; q < 0: refused
    uint64_t gm;                 // the continuous parents as columns
};
// what a continuous family (v, pm) reads, before any block: refused for a bit at or above n, q beyond the cap, no table
__device__ __forceinline__ CgFamily cg_family(const CgKinds& k, const uint8_t* card, int n, int v, uint64_t pm, int table) {
    CgFamily f = {-1, 0, 0, 0ull};
    pm &= ~(1ull << v);
    if (!k.ok || (pm >> n) != 0ull || table < 0) return f;
    const int q = cg_request_configs(pm & k.disc, n, card, DVS_CG_MAX_CONFIGS);
    if (q < 0) return f;
    f.gm = cg_columns(pm, k.cont);
    f.p = __popcll(f.gm);
    if (f.p > DVS_GBN_MAX_PARENTS) return f;
    f.vc = __popcll(k.cont & ((1ull << v) - 1ull));
    f.q = q;
    return f;
}

// the local score of the continuous family (v, pm) over the blocks of its table; NaN and bit 4 of status for a refusal
__device__ __forceinline__ double cg_family_score(const CgScoreArgs& a, const CgKinds& k, int v, uint64_t pm, int table, double* L) {
#pragma clang fp contract(off)
    const CgFamily f = cg_family(k, a.card, a.n, v, pm, table);
    if (f.q < 0) {
        atomicOr(a.status, 16);
        return bn_nan();
    }
    GbnScoreArgs g = {};
    g.type = DVS_GSCORE_LOGLIK;                              // gbn_local's likelihood term, per configuration
    const double* block = (const double*)a.tables[table];
    double ll = 0.0;
    for (int z = 0; z < f.q; ++z, block += DVS_GBN_STRIDE(a.nc)) {
        if (block[0] == 0.0) continue;
        const GbnFamily fz = gbn_family(block, a.nc, f.vc, f.gm, 0.0, true, L);
        if (fz.p < 0) {
            atomicOr(a.status, 16);
            return bn_nan();
        }
        ll = ll + gbn_local(g, fz);
    }
    if (a.type == DVS_CGSCORE_LOGLIK) return ll;
    const double kk = a.arg != a.arg ? log((double)a.S) / 2.0 : a.arg;
    return ll - (kk * (double)f.q) * ((double)f.p + 2.0);
}

// a discrete row holds an illegal arc: a continuous parent
__device__ __forceinline__ bool cg_illegal(const CgKinds& k, int n, int v, uint64_t pm) {
    return !k.ok || ((pm & ~(1ull << v)) & k.cont & (n >= 64 ? ~0ull : (1ull << n) - 1ull)) != 0ull;
}

__global__ __launch_bounds__(256) void k_cg_prep(CgScoreArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n = a.n;
    if (idx < 64) a.bn_card[idx] = idx < n && a.card[idx] != 0 ? a.card[idx] : 1;
    const CgKinds k = cg_kinds(a.card, n, a.nc);
    if (idx < (long long)a.B * n) {
        const int v = (int)(idx % n);
        const uint64_t pm = a.parents[idx];
        a.bn_parents[idx] = a.card[v] == 0 || cg_illegal(k, n, v, pm) ? 0ull : pm;
    }
    if (a.worklist != nullptr && idx < 2ll * a.B) {
        const int v = a.worklist[idx];
        a.bn_worklist[idx] = v >= 0 && v < n && a.card[v] != 0 ? v : -1;
    }
}

// a thread per family, per worklist slot and per byte of the level counts' copy, whichever are most
static inline dim3 cg_prep_grid(const CgScoreArgs& a) {
    long long threads = (long long)a.B * a.n;
    if (threads < 2ll * a.B) threads = 2ll * a.B;
    if (threads < 64) threads = 64;
    return dim3((unsigned)((threads + 255) / 256));
}

__global__ __launch_bounds__(GBN_LANES) void k_cg_local(CgScoreArgs a) {
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const long long fam = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (fam >= (long long)a.B * a.n) return;
    const int v = (int)(fam % a.n);
    const CgKinds k = cg_kinds(a.card, a.n, a.nc);
    const uint64_t pm = a.parents[fam];
    if (a.card[v] != 0) {
        if (cg_illegal(k, a.n, v, pm)) {
            atomicOr(a.status, 16);
            a.local[fam] = bn_nan();
        }
        return;
    }
    a.local[fam] = cg_family_score(a, k, v, pm, a.table_of != nullptr ? a.table_of[fam] : -1, s_L + threadIdx.x);
}

void dvs_launch_cg_scores(const CgScoreArgs& a, const BicArgs& bn, dvs_stream_t st) {
    const long long fams = (long long)a.B * a.n;
    DVS_LAUNCH(k_cg_prep, cg_prep_grid(a), dim3(256), 0, st, a);
    dvs_launch_bic(bn, st);
    DVS_LAUNCH(k_cg_local, dim3((unsigned)((fams + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, a);
    GbnScoreArgs total = {};
    total.B = a.B;
    total.n = a.n;
    total.local = a.local;
    total.out = a.out;
    DVS_LAUNCH(k_gbn_total, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, st, total);
}

// One lane per cell (row, u) of the rows a pass covers, as k_gbn_toggle.
__global__ __launch_bounds__(GBN_LANES) void k_cg_toggle(CgScoreArgs a) {
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const int n = a.n;
    const long long rows = a.worklist != nullptr ? 2ll * a.B : (long long)a.B * n;
    const long long idx = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (idx >= rows * n) return;
    const int row = (int)(idx / n), u = (int)(idx - (long long)row * n);
    int b, v;
    if (a.worklist != nullptr) {
        v = a.worklist[row];
        b = row >> 1;
        if (v < 0 || v >= n || u == v) return;       // empty slot; L of a moved row is the T cell of the move (k_hc_step)
    } else {
        v = row % n;
        b = row / n;
    }
    const size_t cell = (size_t)b * n + v;
    const CgKinds k = cg_kinds(a.card, n, a.nc);
    const uint64_t pm = a.parents[cell];
    if (a.card[v] != 0) {
        // the discrete scorer wrote the row; an illegal arc as it stands refuses all of it, a continuous u is not available
        const bool bad = cg_illegal(k, n, v, pm);
        if (bad) atomicOr(a.status, 16);
        if (u == v) {
            if (bad) a.local[cell] = bn_nan();
        } else if (bad || ((k.cont >> u) & 1ull)) {
            a.toggles[cell * n + u] = bn_nan();
        }
        return;
    }
    const double score = cg_family_score(a, k, v, pm ^ (u == v ? 0ull : 1ull << u), a.table_of != nullptr ? a.table_of[idx] : -1, s_L + threadIdx.x);
    if (u == v) {
        a.local[cell] = score;
        a.toggles[cell * n + u] = bn_nan();
    } else {
        a.toggles[cell * n + u] = score;
    }
}

void dvs_launch_cg_toggle(const CgScoreArgs& a, const ToggleArgs& bn, dvs_stream_t st) {
    const long long fams = (long long)a.B * a.n;
    const long long rows = a.worklist != nullptr ? 2ll * a.B : fams;
    DVS_LAUNCH(k_cg_prep, cg_prep_grid(a), dim3(256), 0, st, a);
    dvs_launch_bn_toggle(bn, st);
    DVS_LAUNCH(k_cg_toggle, dim3((unsigned)((rows * a.n + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Fit
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBN_LANES) void k_cg_fit(CgFitArgs t) {
#pragma clang fp contract(off)
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const long long cell = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (cell >= (long long)t.cells) return;
    const int n = t.n;
    int lo = 0, hi = t.F - 1;                                // the family of the cell: the last one with offset <= cell
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.offset[mid] <= cell) lo = mid;
        else hi = mid - 1;
    }
    const long long z = cell - t.offset[lo];
    const int v = t.var[lo];
    double* L = s_L + threadIdx.x;
    double* coef = t.coef + (size_t)cell * n;
    const CgKinds k = cg_kinds(t.card, n, t.nc);
    CgFamily f = {-1, 0, 0, 0ull};
    if (v >= 0 && v < n && t.card[v] == 0 && z >= 0) f = cg_family(k, t.card, n, v, t.parents[lo], t.table[lo] != 0ull ? 0 : -1);
    GbnFamily fz;
    fz.p = -1;
    const double* mom = nullptr;
    bool empty = false;
    if (f.q >= 0 && z < f.q) {
        mom = (const double*)t.table[lo] + (size_t)z * DVS_GBN_STRIDE(t.nc);
        empty = mom[0] == 0.0;
        if (!empty) fz = gbn_family(mom, t.nc, f.vc, f.gm, 0.0, true, L);
    }
    t.count[cell] = mom != nullptr ? mom[0] : bn_nan();
    if (fz.p < 0) {
        if (!empty) atomicOr(t.status, 16);
        for (int u = 0; u < n; ++u) coef[u] = bn_nan();
        t.intercept[cell] = bn_nan();
        t.sd[cell] = bn_nan();
        return;
    }
    const int p = fz.p;
    gbn_backsolve(L, p);
    for (int u = 0; u < n; ++u) coef[u] = 0.0;
    double c0 = mom[1 + f.vc];
    uint64_t mi = t.parents[lo] & k.cont & ~(1ull << v);
    for (int i = 0; i < p; ++i, mi &= mi - 1ull) {
        const int u = dvs_ctz64(mi);
        const double beta = gbn_L(L, p, i);
        coef[u] = beta;
        const double prod = beta * mom[1 + __popcll(k.cont & ((1ull << u) - 1ull))];
        c0 = c0 - prod;
    }
    t.intercept[cell] = c0;
    t.sd[cell] = sqrt(fz.rss / (fz.m - (double)p - 1.0));
}

void dvs_launch_cg_fit(const CgFitArgs& t, dvs_stream_t st) {
    DVS_LAUNCH(k_cg_fit, dim3((unsigned)((t.cells + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, t);
}
