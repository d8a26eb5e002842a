// Search candidates on the device: decoded rows -> validity, row codec, label-space structure key and hash
// (k_decoded_structures), and the exact "is this structure new" filter against a device-resident set
// (k_structset_filter).  Together they replace the host stage between decode and BIC of latent_bo_search
// (dags_vae_search_amd/search.py: graphs_from_states -> is_search_valid -> structure_key -> Python set -> encode_graphs),
// which is the specification both kernels are pinned to.  Included by k_decode.hip only (kernels and launchers are
// defined here, once), next to dvs_match.h.
//
// k_decoded_structures — one wave64 per decoded row, one lane per user vertex (n <= 45), no LDS, no atomics.
//   User vertex i is PACE vertex i + 2 with label - 3; edge u -> v iff bit u + 2 of parents[v + 2], for u < v among the user
//   vertices.  dvs_decode only ever adds edges from a lower to a higher vertex and the mask `(1 << v) - 1` keeps nothing
//   else, so the graph is ACYCLIC BY CONSTRUCTION and no Kahn pass is needed; edges from PACE vertices 0 / 1 and into the
//   closing `output` vertex are not part of the structure (graphs_from_states drops them too).
//   Lane v reads parents[v + 2] (8 B, contiguous across lanes) and label[v + 2] (1 B, contiguous) directly: both field
//   reads of a wave are coalesced as they stand, so the 440-byte state is not staged through shuffles first.
//   One loop over the vertices u broadcasts label[u]; every lane ORs `1 << label[u]` into `seen` (the permutation check:
//   popcount(seen) == n once all labels are in range) and, where u is one of its parents, into its relabelled row.
//   Lane v then owns key word label[v]:  key[label[v]] = OR over parents u of (1 << label[u]), which is what
//   dvs_bic_parent_masks makes of the row codec and what BNLearnWrapper._parent_masks makes of the graph object.
//   flags: bit 0 search-valid; otherwise exactly one reason: bit 1 short row (nv < n + 3), bit 2 a label outside
//   0..n-1 (PACE labels below 3 included), bit 3 a repeated label.  Invalid rows get zero codec and key words and the hash
//   DVS_STRUCT_HASH_INVALID.
//   hash = mix(sum over variables i of mix(key[i] ^ salt(i))) & hash_mask & 2^63 - 1.  The inner sum is order-free, so it
//   is a plain butterfly over the lanes that own the words; the salt ties every word to its variable index.  Hashes keep 63
//   bits so that signed and unsigned 64-bit sorts agree, and the invalid value (2^63 - 1) sorts last in both.
//
// k_structset_filter — one wave64 per SORTED position of the batch, lanes = key words, no LDS, no atomics.
//   Inputs: the batch's hashes in ascending order with the row index of every sorted position (a STABLE sort, so equal
//   hashes keep draw order), keys and flags in row order, and the set as (hash ascending, key) rows.
//   The wave binary-searches the start of its hash's run in the set and walks it, then binary-searches the start of its run
//   in the batch and walks that up to its own position; every step compares FULL keys (one ballot per comparison).
//   out[row]: 1 new | 2 already in the set | 4 duplicate of an earlier row of the batch | 0 not a valid row.
//
// SOUNDNESS RULE (keep it when changing this file): equality of structures is decided on the full key only.  The hash
// decides nothing but where a walk starts and ends, so collisions cost time, never correctness; rows whose flags lack
// bit 0 are skipped by flag, never by their hash value.  The result is a pure function of the inputs (the first
// occurrence in draw order wins because a row only ever looks at sorted positions BEFORE its own), hence deterministic.
// Cost: a row stops at the first equal key, so k copies of one structure cost one comparison each (with the head of the
// run).  A row walks past every DIFFERENT key of equal hash that sorts before it: with 63-bit hashes that is nothing in
// practice; under forced collisions (hash_mask = 0xF) it is O(run length) comparisons per row, quadratic in the run.
//
// Control flow is wave-uniform throughout (loop bounds and branch conditions come from ballots, broadcast shuffles, the
// row index or values every lane loads from the same address), so every ballot and shuffle runs with the full EXEC mask.
#pragma once
#include "dvs_decode.h"
#include "dvs_search_args.h"

constexpr int STRUCT_VALID = 1, STRUCT_SHORT = 2, STRUCT_LABEL_RANGE = 4, STRUCT_LABEL_REPEAT = 8;
constexpr int FILTER_NEW = 1, FILTER_SEEN = 2, FILTER_DUPLICATE = 4;
constexpr uint64_t STRUCT_HASH_INVALID = 0x7fffffffffffffffull;     // DVS_STRUCT_HASH_INVALID (include/dvs.h)

// splitmix64's finaliser
__device__ __forceinline__ uint64_t structs_mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ uint64_t structs_wave_sum64(uint64_t v) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, sh), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), sh);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_decoded_structures(StructArgs a) {
    const Lane L = dvs_lane();
    const int k = blockIdx.x * 4 + L.wave;           // row: wave-uniform
    if (k >= a.B) return;
    const int n = a.n, lane = L.lane;
    const bool real = lane < n;
    const DvsDecodeState* S = a.states + k;
    int l = -1;                                      // user label of vertex `lane`
    uint64_t p = 0;                                  // its parents among the user vertices (bit u <=> u -> lane, u < lane)
    if (real) {
        l = (int)S->label[lane + 2] - 3;
        p = (S->parents[lane + 2] >> 2) & ((1ull << lane) - 1ull);
    }
    int f = 0;
    if (S->nv < n + 3) f = STRUCT_SHORT;             // stopped growing early: the host's decode gives None
    else if (__ballot(real && (l < 0 || l >= n))) f = STRUCT_LABEL_RANGE;
    uint64_t row = 0;
    if (f == 0) {                                    // every label is in 0..n-1: shifts by it are defined
        uint64_t seen = 0;
        for (int u = 0; u < n; ++u) {
            const uint64_t bit = 1ull << (__shfl(l, u) & 63);
            seen |= bit;
            if ((p >> u) & 1ull) row |= bit;
        }
        f = __popcll(seen) == n ? STRUCT_VALID : STRUCT_LABEL_REPEAT;
    }
    const bool ok = f == STRUCT_VALID;
    uint64_t h = STRUCT_HASH_INVALID;
    if (ok) {
        const uint64_t t = real ? structs_mix64(row ^ (0x9e3779b97f4a7c15ull * (uint64_t)(l + 1))) : 0ull;
        h = structs_mix64(structs_wave_sum64(t)) & a.hash_mask & STRUCT_HASH_INVALID;
    }
    if (real) {
        const size_t base = (size_t)k * n;
        a.labels[base + lane] = (uint8_t)(ok ? l : 0);
        if (a.wide) ((uint64_t*)a.preds)[base + lane] = ok ? p : 0ull;
        else ((uint16_t*)a.preds)[base + lane] = (uint16_t)(ok ? p : 0ull);
        a.keys[base + (ok ? l : lane)] = ok ? row : 0ull;     // a permutation: every word of the row is written once
    }
    if (lane == 0) {
        a.flags[k] = (uint8_t)f;
        a.hashes[k] = h;
    }
}

// first index in a[0, n) whose value is >= h (a ascending)
__device__ __forceinline__ int structs_lower_bound(const uint64_t* a, int n, uint64_t h) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_structset_filter(FilterArgs a) {
    const Lane L = dvs_lane();
    const int pw = blockIdx.x * 4 + L.wave;
    if (pw >= a.B) return;
    const int p = __builtin_amdgcn_readfirstlane(pw);    // sorted position, uniform for the compiler too: the index
    const int n = a.n, lane = L.lane;                    // arithmetic of the two walks stays in scalar registers
    const bool real = lane < n;
    const uint64_t B = (uint64_t)a.B;
    const uint64_t r = (uint64_t)a.order[p];
    if (r >= B) return;                                  // `order` is not a permutation of the rows: touch nothing
    if (!(a.flags[r] & STRUCT_VALID)) {
        if (lane == 0) a.out[r] = 0;
        return;
    }
    const uint64_t h = a.sorted_hashes[p];
    const uint64_t mine = real ? a.keys[r * n + lane] : 0ull;
    for (int j = structs_lower_bound(a.seen_hashes, a.S, h); j < a.S && a.seen_hashes[j] == h; ++j) {
        const bool differs = real && a.seen_keys[(size_t)j * n + lane] != mine;
        if (__ballot(differs) == 0ull) {
            if (lane == 0) a.out[r] = FILTER_SEEN;
            return;
        }
    }
    for (int q = structs_lower_bound(a.sorted_hashes, p, h); q < p; ++q) {
        const uint64_t r2 = (uint64_t)a.order[q];
        if (r2 >= B || !(a.flags[r2] & STRUCT_VALID)) continue;
        const bool differs = real && a.keys[r2 * n + lane] != mine;
        if (__ballot(differs) == 0ull) {
            if (lane == 0) a.out[r] = FILTER_DUPLICATE;
            return;
        }
    }
    if (lane == 0) a.out[r] = FILTER_NEW;
}

void dvs_launch_decoded_structures(const StructArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_decoded_structures, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}
void dvs_launch_structset_filter(const FilterArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_structset_filter, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}
