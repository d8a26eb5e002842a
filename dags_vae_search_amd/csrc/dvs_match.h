// Reconstruction judging on the device: exact (labelled) DAG isomorphism of decoded rows against their targets.
//
// Replaces the host loop of batch_test (experiments/03_synthetic_12/main.py:200-217: toolkit.is_valid_graph /
// graph_equals per decoded graph, networkx VF2 when labels repeat).  One wave64 per (target, decoded row) pair, one lane
// per vertex (n <= 45); no LDS.  Included by k_decode.hip only (the kernel and its launcher are defined here, once).
//
// Flags of decoded row k (target k / R):  bit 0 valid (nv == n_tokens, every label in [0, card)), bit 1 same structure
// (isomorphic, labels ignored), bit 2 same labelled graph, bit 3 undecided (a search ran out of `budget` nodes; bits 1
// and 2 are then unspecified).  A row with nv < n_tokens gets 0.  Bits 1/2 do not depend on bit 0.
//
// SOUNDNESS RULE (keep it when changing this file):
//   * "isomorphic" is answered only after a COMPLETE vertex mapping has been checked edge by edge (every parent row of
//     the decoded graph equals the image of the mapped target row) and, for bit 2, label by label (match_verify);
//   * "not isomorphic" is answered only from an isomorphism invariant computed by the SAME function on both graphs
//     (the colour histograms of match_refine, which also cover vertex and edge counts) or from an exhausted search
//     whose candidates were removed only by necessary conditions (equal stable colour, unused, consistent with the
//     partial mapping).
// Hash collisions in the colour refinement therefore cost pruning power, never correctness.
//
// Control flow is wave-uniform throughout (every loop bound and branch condition comes from a ballot, a broadcast
// shuffle or the pair index), so every ballot and shuffle runs with the full EXEC mask.
#pragma once
#include "dvs_decode.h"
#include "dvs_search_args.h"

constexpr int MATCH_MAX_N = 45;
constexpr int MATCH_VALID = 1, MATCH_STRUCT = 2, MATCH_LABELLED = 4, MATCH_UNDECIDED = 8;

// one vertex (lane) of both graphs: target (1) and decoded row (2)
struct MatchLane {
    uint64_t p1, c1, p2, c2;     // parent / child rows
    int l1, l2;                  // labels (the decoded one signed: PACE label - 3)
};

__device__ __forceinline__ unsigned match_mix(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// Directed 1-WL on both graphs at once.  Start colour: (in-degree, out-degree[, label]); a round maps every colour to
// mix(colour, sum h(parent colours), sum h'(child colours)).  Stops when the number of classes stops growing (or is n).
// Returns false when the two colour histograms differ in some round: then the graphs are not isomorphic.  On success
// col1 / col2 are the stable colours, cls the size of this lane's target colour class and classes their number.
__device__ bool match_refine(const MatchLane& g, int lane, int n, bool labelled, unsigned& col1, unsigned& col2, int& cls,
                             int& classes) {
    const bool real = lane < n;
    col1 = real ? match_mix(((unsigned)__popcll(g.p1) << 6 | (unsigned)__popcll(g.c1)) + (labelled ? (unsigned)g.l1 * 0x9e3779b1u : 0u)) : 0u;
    col2 = real ? match_mix(((unsigned)__popcll(g.p2) << 6 | (unsigned)__popcll(g.c2)) + (labelled ? (unsigned)g.l2 * 0x9e3779b1u : 0u)) : 0u;
    classes = 0;
    for (int round = 0; round <= n; ++round) {
        // one pass over the vertices: histogram counts of this lane's colours and the neighbour sums of the next round
        int n11 = 0, n12 = 0, n22 = 0, n21 = 0;
        bool first = true;
        unsigned sp1 = 0, sc1 = 0, sp2 = 0, sc2 = 0;
        for (int u = 0; u < n; ++u) {
            const unsigned a = (unsigned)__shfl((int)col1, u), b = (unsigned)__shfl((int)col2, u);
            n11 += a == col1;
            n12 += b == col1;
            n22 += b == col2;
            n21 += a == col2;
            if (u < lane && a == col1) first = false;
            const unsigned ha = match_mix(a ^ 0x85ebca6bu), hb = match_mix(b ^ 0x85ebca6bu);
            const unsigned ka = match_mix(a ^ 0xc2b2ae35u), kb = match_mix(b ^ 0xc2b2ae35u);
            if ((g.p1 >> u) & 1ull) sp1 += ha;
            if ((g.c1 >> u) & 1ull) sc1 += ka;
            if ((g.p2 >> u) & 1ull) sp2 += hb;
            if ((g.c2 >> u) & 1ull) sc2 += kb;
        }
        if (__ballot(real && (n11 != n12 || n22 != n21))) return false;
        cls = n11;
        const int k = __popcll(__ballot(real && first));
        if (k == classes || k == n) {
            classes = k;
            break;
        }
        classes = k;
        if (real) {
            col1 = match_mix(col1 * 0x27d4eb2fu + match_mix(sp1 + 0x165667b1u) * 3u + sc1);
            col2 = match_mix(col2 * 0x27d4eb2fu + match_mix(sp2 + 0x165667b1u) * 3u + sc2);
        }
    }
    return true;
}

// Complete mapping check: lane w (decoded vertex) holds inv = the target vertex mapped onto it.  True iff every decoded
// parent row equals the image of its target's parent row (labels too when `labelled`).
__device__ bool match_verify(const MatchLane& g, int lane, int n, bool labelled, int inv) {
    const bool real = lane < n;
    bool bad = real && inv < 0;
    for (int w = 0; w < n; ++w) {
        const int u = __shfl(inv, w);
        const uint64_t S = dvs_bcast64(g.p1, u < 0 ? 0 : u);
        const uint64_t img = __ballot(inv >= 0 && ((S >> (inv & 63)) & 1ull));
        if (lane == w) bad = bad || g.p2 != img;
    }
    const int lt = __shfl(g.l1, inv < 0 ? 0 : inv);
    if (labelled && real && lt != g.l2) bad = true;
    return __ballot(bad) == 0ull;
}

// Backtracking search for an isomorphism target -> decoded.  Returns 1 (found and verified), 0 (exhausted) or -1 (more
// than `budget` search nodes).  Target vertices are placed most-constrained first: most placed neighbours, then the
// smallest colour class, then the lowest index (plain vertex order when the colouring is discrete: every class is a
// singleton).  Per lane: ord (target vertex of depth `lane`), pick / stk (decoded vertex chosen at depth `lane` and the
// candidates left there), inv (target vertex mapped onto decoded vertex `lane`).
__device__ int match_search(const MatchLane& g, int lane, int n, bool labelled, unsigned col1, unsigned col2, int cls,
                            bool discrete, int budget) {
    const bool real = lane < n;
    int ord = lane;
    uint64_t placed = 0;
    for (int d = 0; d < n && !discrete; ++d) {
        const int near = __popcll((g.p1 | g.c1) & placed);
        int key = real && !((placed >> lane) & 1ull) ? ((64 - near) << 12 | cls << 6 | lane) : 0x7fffffff;
#pragma unroll
        for (int sh = 1; sh < 64; sh <<= 1) {
            const int o = __shfl_xor(key, sh);
            key = o < key ? o : key;
        }
        const int v = __builtin_amdgcn_readfirstlane(key) & 63;
        if (lane == d) ord = v;
        placed |= 1ull << v;
    }
    int inv = -1, pick = 0;
    uint64_t stk = 0, used = 0, cand = 0;
    int d = 0, nodes = 0;
    bool descend = true;
    for (;;) {
        if (descend) {           // candidates of depth d
            const int v = __shfl(ord, d);
            const uint64_t pv = dvs_bcast64(g.p1, v), cv = dvs_bcast64(g.c1, v);
            const unsigned colv = (unsigned)__shfl((int)col1, v);
            const int lv = __shfl(g.l1, v);
            const bool mapped = inv >= 0;
            const uint64_t imgp = __ballot(mapped && ((pv >> (inv & 63)) & 1ull));
            const uint64_t imgc = __ballot(mapped && ((cv >> (inv & 63)) & 1ull));
            const bool ok = real && !((used >> lane) & 1ull) && col2 == colv && (!labelled || g.l2 == lv) &&
                            (g.p2 & used) == imgp && (g.c2 & used) == imgc && ((g.p2 >> lane) & 1ull) == ((pv >> v) & 1ull);
            cand = __ballot(ok);
            descend = false;
        }
        if (cand == 0ull) {      // back to the previous depth
            if (d == 0) return 0;
            --d;
            const int w = __shfl(pick, d);
            if (lane == w) inv = -1;
            used &= ~(1ull << w);
            cand = dvs_bcast64(stk, d);
            continue;
        }
        if (nodes >= budget) return -1;
        ++nodes;
        const int w = dvs_ctz64(cand);
        cand &= cand - 1ull;
        if (lane == d) {
            stk = cand;
            pick = w;
        }
        const int v = __shfl(ord, d);
        if (lane == w) inv = v;
        used |= 1ull << w;
        if (d + 1 < n) {
            ++d;
            descend = true;
            continue;
        }
        if (match_verify(g, lane, n, labelled, inv)) return 1;
        if (lane == w) inv = -1;     // (unreachable with consistent candidates; kept so that only a verified map counts)
        used &= ~(1ull << w);
    }
}

// 1 isomorphic, 0 not, -1 undecided
__device__ int match_graphs(const MatchLane& g, int lane, int n, bool labelled, int budget) {
    unsigned col1, col2;
    int cls = 1, classes = 0;
    if (!match_refine(g, lane, n, labelled, col1, col2, cls, classes)) return 0;
    return match_search(g, lane, n, labelled, col1, col2, cls, classes == n, budget);
}

__global__ __launch_bounds__(256) void k_match_decoded(MatchArgs a) {
    const Lane L = dvs_lane();
    const int k = blockIdx.x * 4 + L.wave;           // pair index: wave-uniform
    if (k >= a.B * a.R) return;
    const int n = a.n, lane = L.lane;
    const bool real = lane < n;
    const DvsDecodeState* S = a.states + k;
    if (S->nv < n + 3) {                             // stopped growing early: the host's decode gives None
        if (lane == 0) a.flags[k] = 0;
        return;
    }
    const size_t t = (size_t)(k / a.R) * n + lane;
    MatchLane g;
    g.p1 = g.p2 = 0;
    g.l1 = g.l2 = 0;
    if (real) {
        g.l1 = a.labels[t];
        g.p1 = (a.wide ? ((const uint64_t*)a.preds)[t] : (uint64_t)((const uint16_t*)a.preds)[t]) & ((1ull << n) - 1ull);
        g.l2 = (int)S->label[lane + 2] - 3;                            // user vertex i = PACE vertex i + 2
        g.p2 = (S->parents[lane + 2] >> 2) & ((1ull << lane) - 1ull);  // u -> v (u < v) <=> bit u + 2 of parents[v + 2]
    }
    g.c1 = g.c2 = 0;
    for (int u = 0; u < n; ++u) {
        const uint64_t m1 = __ballot((g.p1 >> u) & 1ull), m2 = __ballot((g.p2 >> u) & 1ull);
        if (lane == u) {
            g.c1 = m1;
            g.c2 = m2;
        }
    }
    int f = __ballot(real && (g.l2 < 0 || g.l2 >= a.card)) ? 0 : MATCH_VALID;
    const int s = match_graphs(g, lane, n, false, a.budget);
    if (s < 0) {
        f |= MATCH_UNDECIDED;
    } else if (s > 0) {
        f |= MATCH_STRUCT;
        const int l = match_graphs(g, lane, n, true, a.budget);
        if (l < 0) f |= MATCH_UNDECIDED;
        else if (l > 0) f |= MATCH_LABELLED;
    }
    if (lane == 0) a.flags[k] = (uint8_t)f;
}

void dvs_launch_match_decoded(const MatchArgs& a, dvs_stream_t st) {
    const size_t pairs = (size_t)a.B * a.R;
    DVS_LAUNCH(k_match_decoded, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, a);
}
