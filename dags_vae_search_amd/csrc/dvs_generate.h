// Training-graph generation on the device: Erdos-Renyi DAGs written straight into the compact row codec.
//
// Replaces LabeledDag.generate_random_graph_erdos_renyi (src/toolkit/labeled.py:281-333: igraph Erdos_Renyi(n, m),
// to_directed("acyclic"), a connectivity test and up to try_limit retries, one igraph object at a time) and the Python
// loop of synthetic.py.  Included by k_decode.hip only (the kernels and their launchers are defined here, once).
//
// Semantics (pinned bit for bit by tests/generate_corpus.py).  DAG b, n vertices, m = num_edges[b] edges,
// P = n (n - 1) / 2 slots; slot t = v (v - 1) / 2 + u is the edge u -> v (u < v), walked v = 1 .. n-1 outer, u = 0 .. v-1
// inner.  Attempt a is Knuth's selection sampling (Algorithm S) over the slots in that order from the draws
// h = dvs_draw(key_e, a * 1024 + t): slot t is taken iff umulhi(h, P - t) < m - chosen, so exactly m slots are taken.
// The result is the FIRST attempt in attempt order that is accepted (weakly connected over all vertices; over the
// vertices of degree >= 1 with DVS_GEN_ACCEPT_ISOLATES; always with DVS_GEN_ACCEPT_NO_CONNECTIVITY).  Labels are drawn
// once, by the accepted attempt, from key_l.  Nothing here depends on how attempts are mapped to lanes.
//
// Mapping: G = 2^gshift lanes share one DAG and try attempts k G .. k G + G - 1 of it side by side; a ballot picks the
// lowest accepted one.  A lane walks its attempt alone: row v is built in a register and retired to the lane's LDS column
// once per v (element [v][lane]: consecutive lanes, consecutive words — conflict-free for b32 and b64), connectivity is
// a fixed point over those bit rows, and the winner copies its column out with plain vector stores.  The walk has the
// same trip count in every lane (n is uniform), so a wave only diverges in the few passes of the fixed point.
// Control flow around the two ballots is wave-uniform.
#pragma once
#include "dvs_decode.h"
#include "dvs_search_args.h"

constexpr int GEN_LABELS_CHOICE = 1, GEN_ACCEPT_ISOLATES = 2, GEN_ACCEPT_NO_CONNECTIVITY = 4;

// one attempt of this lane: rows into col[v * 64]; true iff accepted
template <class Acc>
__device__ __forceinline__ bool gen_attempt(Acc* col, uint32_t key, uint32_t attempt, int n, int P, int m, int flags) {
    const uint32_t base = attempt << 10;
    uint32_t t = 0;
    int chosen = 0;
    Acc touched = 0;             // vertices of degree >= 1
    col[0] = 0;
    for (int v = 1; v < n; ++v) {
        Acc row = 0;
        for (int u = 0; u < v; ++u, ++t) {
            const uint32_t h = dvs_draw(key, base + t);
            const bool take = __umulhi(h, (uint32_t)P - t) < (uint32_t)(m - chosen);
            row |= take ? (Acc)1 << u : (Acc)0;
            chosen += take ? 1 : 0;
        }
        col[v * 64] = row;
        if (row) touched |= row | (Acc)1 << v;
    }
    if (flags & GEN_ACCEPT_NO_CONNECTIVITY) return true;
    const Acc all = (Acc)(((uint64_t)1 << n) - 1u);
    const Acc want = (flags & GEN_ACCEPT_ISOLATES) ? touched : all;
    Acc R = want & (~want + 1);  // lowest wanted vertex (m >= n - 1 >= 1: there is one)
    for (;;) {
        const Acc before = R;
        for (int v = 1; v < n; ++v) {
            const Acc row = col[v * 64];
            if ((R >> v) & 1u) R |= row;
            else if (row & R) R |= (Acc)1 << v;
        }
        for (int v = n - 1; v >= 1; --v) {
            const Acc row = col[v * 64];
            if ((R >> v) & 1u) R |= row;
            else if (row & R) R |= (Acc)1 << v;
        }
        if (R == before) break;
    }
    return R == want;
}

__device__ __forceinline__ void gen_labels(uint8_t* out, uint32_t key, int n, int card, int flags) {
    uint64_t unused = ((uint64_t)1 << card) - 1u;
    for (int v = 0; v < n; ++v) {
        const uint32_t h = dvs_draw(key, (uint32_t)v);
        int label;
        if (flags & GEN_LABELS_CHOICE) {
            label = (int)__umulhi(h, (uint32_t)card);
        } else {                 // the r-th value not yet used, lowest first
            const int r = (int)__umulhi(h, (uint32_t)(card - v));
            uint64_t left = unused;
            for (int i = 0; i < r; ++i) left &= left - 1u;
            label = dvs_ctz64(left);
            unused &= ~((uint64_t)1 << label);
        }
        out[v] = (uint8_t)label;
    }
}

template <class Row, class Acc>
__global__ __launch_bounds__(64) void k_generate_dags(GenArgs a) {
    DVS_DYN_LDS(smem);
    const int lane = dvs_tid() & 63;
    Acc* col = (Acc*)smem + lane;                    // [n][64], this lane's column
    const int G = 1 << a.gshift, j = lane & (G - 1), grp = lane >> a.gshift;
    const size_t dag = (size_t)blockIdx.x * (64 >> a.gshift) + grp;
    const bool live = dag < (size_t)a.B;
    const int n = a.n, P = n * (n - 1) / 2;
    const int m = live ? a.num_edges[dag] : 0;
    const uint32_t gdag = a.dag_offset + (uint32_t)dag;
    const uint32_t key_e = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_GEN_EDGES, gdag);
    const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (grp * G);
    Row* preds = (Row*)a.preds + dag * n;
    uint8_t* labels = a.labels + dag * n;
    bool open = live && m >= n - 1 && m <= P;        // this lane's DAG is still looking for an accepted attempt
    int result = open ? 0 : -1;
    for (int a0 = 0; a0 < a.try_limit; a0 += G) {
        if (__ballot(open) == 0ull) break;
        const int attempt = a0 + j;
        bool ok = false;
        if (open && attempt < a.try_limit) ok = gen_attempt<Acc>(col, key_e, (uint32_t)attempt, n, P, m, a.flags);
        const uint64_t won = __ballot(ok) & gmask;
        if (open && won) {
            const int first = dvs_ctz64(won) - grp * G;
            result = a0 + first + 1;
            open = false;
            if (j == first) {
                for (int v = 0; v < n; ++v) preds[v] = (Row)col[v * 64];
                gen_labels(labels, dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_GEN_LABELS, gdag), n, a.card, a.flags);
            }
        }
    }
    if (live && j == 0) {
        a.attempts[dag] = result;
        if (result <= 0)
            for (int v = 0; v < n; ++v) {
                preds[v] = 0;
                labels[v] = 0;
            }
    }
}

// Edge count of DAG b of a stream: entry i of the schema with probability weight_i / W, from one draw of site 302:
// r = umulhi(draw(key_m, 0), W), the first i with cum[i] > r (cum: running sums of the weights, cum[K - 1] = W).
__global__ __launch_bounds__(256) void k_generate_edge_counts(int B, int K, const int* counts, const int* cum, uint32_t seed_lo,
                                                              uint32_t seed_hi, uint32_t dag_offset, int* out) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (size_t)B) return;
    const uint32_t key = dvs_site_key(seed_lo, seed_hi, DVS_SITE_GEN_COUNTS, dag_offset + (uint32_t)b);
    const int r = (int)__umulhi(dvs_draw(key, 0u), (uint32_t)cum[K - 1]);
    int i = 0;
    while (i < K - 1 && cum[i] <= r) ++i;
    out[b] = counts[i];
}

void dvs_launch_generate_edge_counts(int B, int K, const int* counts, const int* cum, uint64_t seed, uint32_t dag_offset, int* out,
                                     dvs_stream_t st) {
    DVS_LAUNCH(k_generate_edge_counts, dim3((unsigned)(((size_t)B + 255) / 256)), dim3(256), 0, st, B, K, counts, cum, (uint32_t)seed,
               (uint32_t)(seed >> 32), dag_offset, out);
}

void dvs_launch_generate_dags(const GenArgs& in, uint64_t seed, bool wide, dvs_stream_t st) {
    GenArgs a = in;
    dvs_seed_split(a, seed);
    const int per = 64 >> a.gshift;
    const dim3 grid((unsigned)(((size_t)a.B + per - 1) / per));
    if (wide) DVS_LAUNCH_AS("k_generate_dags", (k_generate_dags<uint64_t, uint64_t>), grid, dim3(64), (size_t)a.n * 64 * 8, st, a);
    else DVS_LAUNCH_AS("k_generate_dags", (k_generate_dags<uint16_t, uint32_t>), grid, dim3(64), (size_t)a.n * 64 * 4, st, a);
}
