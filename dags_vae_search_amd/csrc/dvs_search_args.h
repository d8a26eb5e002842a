// Argument blocks and launcher prototypes of the search side: reconstruction matching, search candidates, the graph
// generator (kernels in dvs_match.h / dvs_structs.h / dvs_generate.h, compiled into k_decode.hip), the BN scorers, hill
// climbing, tabu, structure comparison, CI tests and PC-stable, BN parameters, exact search, the exact arc posterior and the GP
// predictor (k_bic.hip with dvs_bn_common.h and dvs_hillclimb.h / dvs_tabu.h / dvs_cpdag.h / dvs_citest.h / dvs_params.h /
// dvs_infer.h / dvs_eliminate.h / dvs_incomplete.h / dvs_exact.h / dvs_posterior.h / dvs_strength.h / dvs_available.h / dvs_local.h / dvs_permtest.h / dvs_gaussian.h / dvs_gaussian_ci.h / dvs_gaussian_params.h / dvs_gaussian_incomplete.h / dvs_mixed.h / dvs_mixed_params.h; k_gp_acq.hip).  Plain C++, no device code: the kernel files and the C-ABI layer
// (dvs_api_search.inc) both include it.  An entry point validates and fills the
// block by field name; the launcher next to the kernel owns the grid, block, LDS size, the template or family choice, the
// profile name and the fields marked "launcher" below, which it derives from kernel constants or from its extra arguments.
#pragma once
#include "dvs_kernels.h"
#include "../../include/dvs_eliminate.h"
#include "../../include/dvs_incomplete.h"
#include "../../include/dvs_available.h"
#include "../../include/dvs_local.h"
#include "../../include/dvs_permtest.h"
#include "../../include/dvs_gaussian.h"
#include "../../include/dvs_gaussian_ci.h"
#include "../../include/dvs_gaussian_params.h"
#include "../../include/dvs_mixed.h"
#include "../../include/dvs_mixed_params.h"
#include "../../include/dvs_gaussian_incomplete.h"

struct DvsDecodeState;           // dvs_decode.h

// the seed_lo / seed_hi of an argument block (marked "launcher" below): the halves dvs_site_key takes
template <class Args>
inline void dvs_seed_split(Args& a, uint64_t seed) {
    a.seed_lo = (uint32_t)(seed & 0xffffffffull);
    a.seed_hi = (uint32_t)(seed >> 32);
}

// ---- reconstruction matching (dvs_match.h) ---------------------------------------------------------------------------
struct MatchArgs {
    int B, n, card, R, wide, budget;
    const uint8_t* labels;       // targets: u8 [B][n]
    const void* preds;           // targets: u16 / u64 [B][n], bit u of preds[v] <=> u -> v
    const DvsDecodeState* states;    // [B * R]
    uint8_t* flags;              // [B * R]
};
void dvs_launch_match_decoded(const MatchArgs& a, dvs_stream_t st);

// ---- search candidates (dvs_structs.h) -------------------------------------------------------------------------------
struct StructArgs {
    int B, n, wide;
    uint64_t hash_mask;
    const DvsDecodeState* states;    // [B]
    uint8_t* flags;                  // [B]
    uint8_t* labels;                 // [B][n]
    void* preds;                     // u16 / u64 [B][n]
    uint64_t* keys;                  // [B][n]
    uint64_t* hashes;                // [B]
};
void dvs_launch_decoded_structures(const StructArgs& a, dvs_stream_t st);

struct FilterArgs {
    int B, n, S;
    const uint64_t* sorted_hashes;   // [B] ascending
    const int64_t* order;            // [B] row index of sorted position p
    const uint64_t* keys;            // [B][n], row order
    const uint8_t* flags;            // [B], row order
    const uint64_t* seen_hashes;     // [S] ascending
    const uint64_t* seen_keys;       // [S][n]
    uint8_t* out;                    // [B], row order
};
void dvs_launch_structset_filter(const FilterArgs& a, dvs_stream_t st);

// ---- graph generator (dvs_generate.h) --------------------------------------------------------------------------------
struct GenArgs {
    int B, n, card, try_limit, flags, gshift;
    uint32_t seed_lo, seed_hi, dag_offset;       // seed_lo / seed_hi: launcher, from `seed`
    const int* num_edges;        // [B]
    uint8_t* labels;             // [B][n]
    void* preds;                 // [B][n] u16 / u64
    int* attempts;               // [B]
};
// wide: predecessor rows are u64 (else u16)
void dvs_launch_generate_dags(const GenArgs& a, uint64_t seed, bool wide, dvs_stream_t st);
void dvs_launch_generate_edge_counts(int B, int K, const int* counts, const int* cum, uint64_t seed, uint32_t dag_offset, int* out,
                                     dvs_stream_t st);

// ---- BN scorers (k_bic.hip) ------------------------------------------------------------------------------------------
struct BicArgs {
    int B, n, S, words;          // words: launcher
    const uint64_t* data;        // [S][words]
    const uint8_t* card;         // [n] levels of each variable (2..16)
    const uint64_t* parents;     // [B][n]: bit u of parents[b][v] <=> edge u -> v (dataset variable indices)
    double* local;               // [B][n] scratch: local scores
    double* out;                 // [B]
    int* status;
    int type;                    // dvs_score_type; family 1 reads it for the prior
    double arg;                  // family 0: k (NaN: log(S) / 2, taken on the device as dvs_bic_scores always has); family 1: iss
};
void dvs_launch_bic(const BicArgs& a, dvs_stream_t st);

// ---- hill climbing (dvs_hillclimb.h) ---------------------------------------------------------------------------------
struct ToggleArgs {
    BicArgs s;                   // s.local = L [B][n]; s.out unused
    const int* worklist;         // null: full pass; else i32 [2 B]
    double* toggles;             // T [B][n][n]
};
void dvs_launch_bn_toggle(const ToggleArgs& t, dvs_stream_t st);

struct HcArgs {
    int B, n, max_parents, step_cap;
    double min_delta;
    uint64_t* parents;           // [B][n], updated in place
    double* local;               // L [B][n], the moved rows updated from T
    const double* toggles;       // T [B][n][n]
    const uint64_t* forbidden;   // [n] or null: bit u of forbidden[v] bars u -> v
    int* worklist;               // [2 B]
    int* steps;                  // [B]
    int* converged;              // [B]
    int* flags;                  // [B]: 1 the start has a cycle, 2 a local score of the start is NaN
    int64_t* trace;              // null or [B][step_cap][2]: (code, delta bits)
    int* active;                 // += structures that moved in this launch
};
void dvs_launch_hc_step(const HcArgs& a, dvs_stream_t st);

// ---- tabu search and random restarts (dvs_tabu.h) --------------------------------------------------------------------
struct TabuArgs {
    HcArgs h;
    int tabu_len, max_stall;
    uint64_t* ring;              // [B][tabu_len][n]
    int* visited;                // [B]: structures pushed so far; the push slot is visited % tabu_len
    int* stall;                  // [B]: consecutive moves that did not raise the best
    double* best_score;          // [B]
    uint64_t* best_parents;      // [B][n]
};
void dvs_launch_tabu_step(const TabuArgs& t, dvs_stream_t st);

struct PerturbArgs {
    int B, n, max_parents;
    uint32_t seed_lo, seed_hi, draw_index;       // seed_lo / seed_hi: launcher, from `seed`
    uint64_t* parents;
    double* local;
    const double* toggles;
    const uint64_t* forbidden;
    int* worklist;
    int* flags;
};
void dvs_launch_hc_perturb(const PerturbArgs& a, uint64_t seed, dvs_stream_t st);

// ---- structure comparison (dvs_cpdag.h) ------------------------------------------------------------------------------
struct CpdagArgs {
    int B, n;
    const uint64_t* parents;     // [B][n]
    uint64_t* pdag;              // [B][n]: bit u of pdag[b][v] <=> u -> v or u - v (an undirected edge has both bits)
    int* flags;                  // [B], written: 0, 1 a directed cycle, 2 a parent bit >= n or a self-loop
};
void dvs_launch_cpdag(const CpdagArgs& a, dvs_stream_t st);

struct PdagCompareArgs {
    int B, n, b_rows;            // b_rows: 1 (one target for the batch) or B
    const uint64_t* a;           // [B][n]
    const uint64_t* b;           // [b_rows][n]
    int* counts;                 // [B][5]: shd, tp, fp, fn, hamming
};
void dvs_launch_pdag_compare(const PdagCompareArgs& a, dvs_stream_t st);

// ---- conditional-independence tests and PC-stable (dvs_citest.h) -----------------------------------------------------
constexpr int DVS_CI_MAX_CELLS = 36864;          // = BIC_MAX_BINS of k_bic.hip: the dense table that fits LDS
struct CiArgs {
    int T, n, S, words, type, max_cells;         // words: launcher
    const uint64_t* data;        // [S][words]
    const uint8_t* card;         // [n]
    const int* pairs;            // [T][2]: x, y
    const uint64_t* cond;        // [T]: bit z <=> z is in the conditioning set
    double* out;                 // [T][3]: statistic, df, p-value
    int* status;
};
void dvs_launch_ci_tests(const CiArgs& a, dvs_stream_t st);

struct PcExpandArgs {
    int P, n, level;
    long long T;
    const uint64_t* adj;         // [n]: the level's frozen adjacency rows
    const int* pair_xy;          // [P][2]
    const long long* offsets;    // [P + 1]: tests of pair p are offsets[p] .. offsets[p + 1] - 1
    int* pairs;                  // [T][2]
    uint64_t* cond;              // [T]
};
void dvs_launch_pc_expand(const PcExpandArgs& a, dvs_stream_t st);

struct PcReduceArgs {
    int P, n;
    long long T;
    double alpha;
    const int* pair_xy;          // [P][2]
    const long long* offsets;    // [P + 1]
    const uint64_t* cond;        // [T]
    const double* out;           // [T][3]
    const uint64_t* adj;         // [n]
    uint64_t* adj_next;          // [n]
    uint64_t* sepset;            // [n][n], the separated pairs' cells written
    long long* result;           // [P][2]: (index of the separating test or -1, refused tests of the pair)
    int* refused;                // [1], written
};
void dvs_launch_pc_reduce(const PcReduceArgs& a, dvs_stream_t st);

struct PcOrientArgs {
    int B, n;
    const uint64_t* skeleton;    // [B][n]
    const uint64_t* sepsets;     // [B][n][n]
    uint64_t* pdag;              // [B][n], the layout of CpdagArgs::pdag
    int* conflicts;              // [B]
    int* flags;                  // [B]
};
void dvs_launch_pc_orient(const PcOrientArgs& a, dvs_stream_t st);

// ---- BN parameters: fit, forward sampling, held-out log-likelihood (dvs_params.h) -------------------------------------
// CPT layout (include/dvs.h): cpt[offsets[b * n + v] + key * r + k], key the mixed-radix parent configuration.
constexpr int DVS_BN_SAMPLE_LDS_CELLS = 8192;    // thresholds staged in LDS up to here (32 KiB: five workgroups per CU)
struct BnFitArgs {
    int B, n, S, words, method, unobserved;      // words: launcher
    double iss;
    const uint64_t* data;        // [S][words]
    const uint8_t* card;         // [n]
    const uint64_t* parents;     // [B][n]
    const long long* offsets;    // [B * n + 1]
    double* cpt;
    long long cpt_cells;         // cpt_bytes / 8: a slot that ends beyond it is refused
    int* status;
};
void dvs_launch_bn_fit(const BnFitArgs& a, dvs_stream_t st);

// The workspace of dvs_bn_sample: a header of 64 i32 (order [48], then the "drawable" word at index 48), then the u32
// thresholds, cell for cell as the network's tables lie behind offsets[0].
struct BnSampleLayout {
    size_t order, thr, total;
};
inline BnSampleLayout dvs_bn_sample_layout(long long n_cells) {
    BnSampleLayout l;
    l.order = 0;
    l.thr = 256;
    l.total = l.thr + (((size_t)n_cells * 4 + 255) & ~(size_t)255);
    return l;
}
struct BnSampleArgs {
    int n, words;                // words: launcher
    long long rows, n_cells;
    uint32_t seed_lo, seed_hi, row_offset;       // seed_lo / seed_hi: launcher, from `seed`
    const uint8_t* card;         // [n]
    const uint64_t* parents;     // [n]
    const long long* offsets;    // [n + 1]
    const double* cpt;
    int* header;                 // workspace: order [48], drawable at [48]
    uint32_t* thr;               // workspace: [n_cells]
    uint64_t* out;               // [rows][words]
    int* status;
};
void dvs_launch_bn_sample(const BnSampleArgs& a, uint64_t seed, dvs_stream_t st);

// The workspace of dvs_bn_loglik: the chunk partials f64 [B][chunks], the family flags i32 [B][n], then log(theta), cell for
// cell as the tables lie behind offsets[0]; each array starts at a multiple of 256 bytes.
struct BnLoglikLayout {
    size_t partials, fam_ok, logs, chunks;       // logs: also the least workspace (a table of no cells)
};
inline BnLoglikLayout dvs_bn_loglik_layout(int batch, int n_vars, long long rows) {
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    BnLoglikLayout l;
    l.chunks = (size_t)((rows + 255) / 256);
    l.partials = 0;
    l.fam_ok = up((size_t)batch * l.chunks * 8);
    l.logs = l.fam_ok + up((size_t)batch * n_vars * 4);
    return l;
}
struct BnLoglikArgs {
    int B, n, words, chunks;     // words: launcher
    long long rows, log_cells;   // log_cells: doubles the workspace holds behind `logs`
    const uint64_t* data;        // [rows][words]
    const uint8_t* card;
    const uint64_t* parents;     // [B][n]
    const long long* offsets;    // [B * n + 1]
    const double* cpt;
    double* per_row;             // null or [B][rows]
    double* out;                 // [B]
    double* partials;            // workspace [B][chunks]
    int* fam_ok;                 // workspace [B][n]
    double* logs;                // workspace [log_cells]
    int* status;
};
void dvs_launch_bn_loglik(const BnLoglikArgs& a, dvs_stream_t st);
// The second level of dvs_bn_loglik, dvs_gbn_loglik and dvs_cgbn_loglik (dvs_fitted.h): one workgroup per structure
struct BnLoglikSumArgs {
    int chunks;
    const double* partials;      // [B][chunks]
    double* out;                 // [B]
};

// ---- inference on a fitted network: likelihood weighting, exact blanket posterior (dvs_infer.h) ------------------------
// The workspace of dvs_bn_lw: the sampler's workspace (header, thresholds), then the per-query "evidence level >= card" flags
// i32 [Q], then the chunk partials f64 [Q][chunks][3 + 16 T]; each array starts at a multiple of 256 bytes.
struct BnLwLayout {
    size_t order, thr, qbad, partials, total, chunks, cells;
};
inline BnLwLayout dvs_bn_lw_layout(long long n_cells, long long n_queries, long long n_particles, uint64_t targets) {
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const BnSampleLayout s = dvs_bn_sample_layout(n_cells);
    BnLwLayout l;
    int T = 0;
    for (uint64_t tm = targets; tm; tm &= tm - 1ull) ++T;
    l.order = s.order;
    l.thr = s.thr;
    l.qbad = s.total;
    l.chunks = (size_t)((n_particles + 255) / 256);
    l.cells = (size_t)(3 + 16 * T);
    l.partials = l.qbad + up((size_t)n_queries * 4);
    l.total = l.partials + up((size_t)n_queries * l.chunks * l.cells * 8);
    return l;
}
struct BnLwArgs {
    int n, words, Q, chunks, T, cells, cus;      // words, T, cells: launcher; cus: dvs_device_cus(), sizes the grid
    long long M, n_cells;
    uint32_t seed_lo, seed_hi, query_offset;     // seed_lo / seed_hi: launcher, from `seed`
    uint64_t targets;
    const uint8_t* card;         // [n]
    const uint64_t* parents;     // [n]
    const long long* offsets;    // [n + 1]
    const double* cpt;
    const uint64_t* evidence;    // [Q][words]
    const uint64_t* observed;    // [Q]
    const uint16_t* event;       // [n] or null
    int* header;                 // workspace: order [48], drawable at [48]
    uint32_t* thr;               // workspace: [n_cells]
    int* qbad;                   // workspace: [Q]
    double* partials;            // workspace: [Q][chunks][cells]
    double* sums;                // [Q][3]
    double* marginals;           // [Q][T][16] or null (then targets == 0)
    uint64_t* particles;         // [Q][M][words] or null
    double* pweights;            // [Q][M] or null, with particles
    int* status;
};
void dvs_launch_bn_lw(const BnLwArgs& a, uint64_t seed, dvs_stream_t st);

struct BnBlanketArgs {
    int B, n, words, chunks, target, use_children;       // words: launcher
    long long rows, cpt_cells;   // cpt_cells: cpt_bytes / 8: a slot that ends beyond it is malformed
    const uint64_t* data;        // [rows][words]
    const uint8_t* card;
    const uint64_t* parents;     // [B][n]
    const long long* offsets;    // [B * n + 1]
    const double* cpt;
    double* posterior;           // null or [B][rows][card[target]]
    uint8_t* pred;               // [B][rows]
    int* status;
};
void dvs_launch_bn_blanket(const BnBlanketArgs& a, dvs_stream_t st);

// ---- exact inference by variable elimination (dvs_eliminate.h; the plan words: include/dvs_eliminate.h) ---------------
struct BnElimArgs {
    int n, P, G, groups;         // G, groups: launcher (rows per workgroup, workgroups per plan)
    int plan_words, arena_cells, step_cells, rows_per_group, out_stride;
    long long rows, n_cells, plans_words;        // plans_words: plans_bytes / 4: a plan that ends beyond it is malformed
    const uint8_t* card;         // [n]
    const uint64_t* parents;     // [n]
    const long long* offsets;    // [n + 1]
    const double* cpt;
    const int* plans;            // the words of every plan
    const long long* plan_offsets;   // [P + 1]
    const uint16_t* masks;       // [rows][n]
    double* out;                 // [P][rows][out_stride]
    double* z;                   // [P][rows]
    int* plan_flags;             // [P], written by k_bn_elim_check
    int* status;
};
void dvs_launch_bn_eliminate(const BnElimArgs& a, dvs_stream_t st);

// ---- incomplete data: expected counts, tables from counts, exact imputation (dvs_incomplete.h; include/dvs_incomplete.h) ----
// The workspace of dvs_bn_expected_counts: the chunk partials f64 [chunks][n_cells], the integer counts i32 [n_cells], the
// chunks' log-likelihood partials f64 [chunks] and skipped rows i32 [chunks], the rows' ok flags u8 [n_rows]; the workspace of
// dvs_bn_impute: the levels u8 [n_rows][n_vars] and nothing else.  Each array starts at a multiple of 256 bytes.
struct BnIncLayout {
    size_t partials, icounts, ll, skip, row_ok, levels, total, chunks;
};
inline BnIncLayout dvs_bn_inc_layout(long long n_cells, int n_vars, long long rows, bool impute) {
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    BnIncLayout l = {};
    l.chunks = (size_t)((rows + 255) / 256);
    if (impute) {
        l.total = up((size_t)rows * n_vars);
        return l;
    }
    l.icounts = up(l.chunks * (size_t)n_cells * 8);
    l.ll = l.icounts + up((size_t)n_cells * 4);
    l.skip = l.ll + up(l.chunks * 8);
    l.row_ok = l.skip + up(l.chunks * 4);
    l.total = l.row_ok + up((size_t)rows);
    return l;
}
struct BnIncArgs {
    BnElimArgs e;                // the network, the plans and their limits; e.out_stride = out_cells, e.masks / e.out / e.z unused;
                                 // e.G: launcher (rows per group); e.P = n + 1 (expected counts) or n (impute)
    int words, chunks, impute;   // words: launcher
    const uint64_t* data;        // [rows][words]
    const uint64_t* observed;    // [rows]
    double* counts;              // [n_cells]
    double* row_z;               // [rows]
    double* loglik;              // [1]
    long long* skipped;          // [1]
    double* partials;            // workspace [chunks][n_cells]
    int* icounts;                // workspace [n_cells]
    double* ll_partials;         // workspace [chunks]
    int* skip_partials;          // workspace [chunks]
    unsigned char* row_ok;       // workspace [rows]
    unsigned char* levels;       // impute workspace [rows][n]: the level, or 255 for "stays missing"
    uint64_t* data_out;          // impute [rows][words]
    uint64_t* observed_out;      // impute [rows]
};
void dvs_launch_bn_expected_counts(const BnIncArgs& a, dvs_stream_t st);
void dvs_launch_bn_impute(const BnIncArgs& a, dvs_stream_t st);

struct BnFitCountsArgs {
    int n, method, unobserved;
    long long n_cells;
    double iss;
    const uint8_t* card;         // [n]
    const uint64_t* parents;     // [n]
    const long long* offsets;    // [n + 1]
    const double* counts;        // [n_cells]: the cell of offsets[v] + i is counts[offsets[v] - offsets[0] + i]
    double* cpt;                 // [n_cells], indexed as counts
    int* status;
};
void dvs_launch_bn_fit_counts(const BnFitCountsArgs& a, dvs_stream_t st);

// ---- exact search (dvs_exact.h) --------------------------------------------------------------------------------------
// The workspace of dvs_exact_search (include/dvs.h): four arrays, each starting at a multiple of 256 bytes.
struct ExactLayout {
    size_t best, arg, R, sink, total;            // byte offsets, and the size of the whole
};
inline ExactLayout dvs_exact_layout(int batch, int n_vars) {
    const size_t subsets = (size_t)batch << n_vars, cells = subsets * n_vars;
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    ExactLayout l;
    l.best = 0;
    l.arg = up(cells * 8);
    l.R = l.arg + up(cells * 4);
    l.sink = l.R + up(subsets * 8);
    l.total = l.sink + up(subsets * 4);
    return l;
}
struct ExactArgs {
    int B, n, max_parents;
    const double* table;         // [B][2^n][n]: cell [S][v] = local score of v with parents S & ~(1 << v), NaN = not available
    const uint64_t* forbidden;   // [n] or null
    double* best;                // workspace [B][2^n][n]
    uint32_t* arg;               // workspace [B][2^n][n]
    double* R;                   // workspace [B][2^n]
    int* sink;                   // workspace [B][2^n]
    uint64_t* parents;           // [B][n]
    int* order;                  // [B][n]
    double* score;               // [B]
    int* flags;                  // [B], written: 1 no admissible DAG (score -inf)
};
void dvs_launch_exact(const ExactArgs& a, dvs_stream_t st);

// ---- exact arc posterior (dvs_posterior.h) ---------------------------------------------------------------------------
// How k_post_arcs divides the 2^n parent sets of a table: a workgroup of 256 threads takes `rows` = 256 / n consecutive P
// per sweep (thread = (row, v)) and `sweeps` sweeps, so `groups` workgroups cover a table and leave one partial sum each.
struct PosteriorSplit {
    int rows, sweeps, groups;
};
inline PosteriorSplit dvs_posterior_split(int n_vars) {
    const long long total = 1ll << n_vars;
    PosteriorSplit s;
    s.rows = 256 / n_vars;
    const long long wide = (long long)s.rows * 2048;         // at most about 2048 partials per table
    s.sweeps = (int)((total + wide - 1) / wide);
    if (s.sweeps < 8) s.sweeps = 8;
    const long long per = (long long)s.rows * s.sweeps;
    s.groups = (int)((total + per - 1) / per);
    return s;
}
// The workspace of dvs_arc_posterior (include/dvs.h): four arrays, each starting at a multiple of 256 bytes.
struct PosteriorLayout {
    size_t alpha, L, Rb, partial, total;         // byte offsets, and the size of the whole
};
inline PosteriorLayout dvs_posterior_layout(int batch, int n_vars) {
    const size_t subsets = (size_t)batch << n_vars, cells = subsets * n_vars;
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    PosteriorLayout l;
    l.alpha = 0;
    l.L = up(cells * 8);
    l.Rb = l.L + up(subsets * 8);
    l.partial = l.Rb + up(subsets * 8);
    l.total = l.partial + up((size_t)batch * dvs_posterior_split(n_vars).groups * n_vars * n_vars * 8);
    return l;
}
struct PosteriorArgs {
    int B, n, max_parents;
    int rows, sweeps, groups;    // launcher: dvs_posterior_split(n)
    const double* table;         // [B][2^n][n], as ExactArgs::table
    const uint64_t* forbidden;   // [n] or null
    const double* size_prior;    // [n] or null: added to every admissible cell by popcount(P)
    double* alpha;               // workspace [B][2^n][n]: alpha, then gamma in the same cells
    double* L;                   // workspace [B][2^n]
    double* Rb;                  // workspace [B][2^n]
    double* partial;             // workspace [B][groups][n][n]
    double* prob;                // [B][n][n]: [u][v] = P(u -> v)
    double* log_z;               // [B][2]: L[all], Rb[all]
    double* family;              // null or [B][2^n][n]
    int* flags;                  // [B], written: 1 no admissible DAG (log_z -inf)
};
void dvs_launch_arc_posterior(const PosteriorArgs& a, dvs_stream_t st);

// ---- order MCMC over family lists (dvs_ordermc.h) --------------------------------------------------------------------
// The dynamic LDS of k_omc_chain: the lanes' arc accumulators [256][n | 1] and the chain's sums [n][n], both f64.
inline size_t dvs_omc_lds(int n_vars) { return ((size_t)256 * (n_vars | 1) + (size_t)n_vars * n_vars) * 8; }
struct OrderMcmcArgs {
    int C, n, steps, thin, window, init;
    long long F;                 // families in the list, < 2^31
    uint32_t seed_lo, seed_hi;   // launcher, from `seed`
    uint32_t chain_offset;       // the global chain index is taken mod 2^32
    uint32_t step_offset, burn_in;   // 3 (step_offset + steps) < 2^32 is checked; a burn_in beyond that keeps nothing
    const long long* offsets;    // [n + 1]
    const uint64_t* sets;        // [F]
    const double* scores;        // [F]
    int* order;                  // [C][n], in and out
    double* log_score;           // [C]
    int* accepted;               // [C], accumulated
    double* sums;                // [C][n][n], accumulated
    int* kept;                   // [C], accumulated
    double* best_score;          // [C], in and out
    uint64_t* best_parents;      // [C][n], in and out
    double* trace;               // null or [C][steps]
    int* flags;                  // [1], written by k_omc_check
};
void dvs_launch_order_mcmc(const OrderMcmcArgs& a, uint64_t seed, dvs_stream_t st);
struct OrderMcmcFinishArgs {
    int C, n;
    const double* sums;          // [C][n][n]
    const int* kept;             // [C]
    double* prob;                // [n][n]
};
void dvs_launch_order_mcmc_finish(const OrderMcmcFinishArgs& a, dvs_stream_t st);

// ---- row sets, bootstrap, arc strength, averaged network (dvs_strength.h) ---------------------------------------------
// The row-set fields live beside BicArgs / ToggleArgs, not inside them: the kernels of the plain entry points take the
// argument blocks they always took.
struct RowSetArgs {
    const int* rows;             // [n_sets][set_size], each in [0, n_samples): not range-checked on the device
    const int* set_of;           // [B] or null: structure b counts over set set_of[b] (null: set b)
    int set_size, n_sets;
};
struct BicRowsArgs {
    BicArgs s;                   // s.S = set_size
    RowSetArgs r;
};
void dvs_launch_bic_rows(const BicRowsArgs& a, dvs_stream_t st);
struct ToggleRowsArgs {
    ToggleArgs t;                // t.s.S = set_size
    RowSetArgs r;
};
void dvs_launch_bn_toggle_rows(const ToggleRowsArgs& a, dvs_stream_t st);

// ---- available-case scoring on incomplete data (dvs_available.h; include/dvs_available.h) -----------------------------------
// Beside BicArgs / ToggleArgs, as the row sets are.  s.type is DVS_SCORE_LOGLIK and s.arg the penalty coefficient k.
struct BicAvailArgs {
    BicArgs s;
    const uint64_t* observed;    // [S]: bit v set <=> variable v is observed in that row
    int* used;                   // null or [B][n]: the rows that counted for the family
};
void dvs_launch_bn_avail(const BicAvailArgs& a, dvs_stream_t st);
struct ToggleAvailArgs {
    ToggleArgs t;
    const uint64_t* observed;    // [S]
};
void dvs_launch_bn_toggle_avail(const ToggleAvailArgs& a, dvs_stream_t st);

// ---- grouped CI tests and the MMPC round (dvs_local.h; include/dvs_local.h) ------------------------------------------------
struct CiGroupArgs {
    int G, n, S, words, type, lds_cells;         // words: launcher
    const uint64_t* data;        // [S][words]
    const uint8_t* card;         // [n]
    const int* target;           // [G]: y
    const uint64_t* cond;        // [G]: bit z <=> z is in the conditioning set
    const uint64_t* candidates;  // [G]: bit x <=> x is tested against y
    double* out;                 // [G][n][3]: statistic, df, p-value; NaN where not asked or refused
    int* status;
};
void dvs_launch_ci_tests_group(const CiGroupArgs& a, dvs_stream_t st);

struct MmpcUpdateArgs {
    int n, G, phase;
    double alpha;
    const int* target;           // [G]
    const uint64_t* cond;        // [G]
    const uint64_t* candidates;  // [G]
    const long long* offsets;    // [n + 1]: groups of target t are offsets[t] .. offsets[t + 1] - 1
    const double* out;           // [G][n][3]
    const uint64_t* cpc;         // [n]
    const uint64_t* cand;        // [n]
    uint64_t* cpc_next;          // [n], written whole
    uint64_t* cand_next;         // [n], written whole
    int* last;                   // [n], written in the forward phase
    double* pmax;                // [n][n]
    double* smin;                // [n][n]
    uint64_t* sepset;            // [n][n], cell [t][x] of an x that left written
    int* refused;                // [1], written
    long long* result;           // [n][2]: (the member added or -1, candidates that left)
};
void dvs_launch_mmpc_update(const MmpcUpdateArgs& a, dvs_stream_t st);

// ---- Monte Carlo permutation CI tests (dvs_permtest.h; include/dvs_permtest.h) ---------------------------------------------
constexpr int DVS_CI_PERM_MAX = 1 << 20;         // n_perm
constexpr size_t DVS_CI_PERM_LDS = 159744;       // dynamic LDS a k_ci_perm workgroup may ask for: 160 KiB less 4 KiB of static
// The workspace of dvs_ci_perm_tests (include/dvs_permtest.h): three arrays, each starting at a multiple of 256 bytes.
struct CiPermLayout {
    size_t counts, sums, masks, total, blocks;
};
inline CiPermLayout dvs_ci_perm_layout(long long n_tests, int n_perm) {
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    CiPermLayout l;
    l.blocks = (size_t)((n_perm + 255) / 256);
    const size_t cells = (size_t)n_tests * l.blocks;
    l.counts = 0;
    l.sums = up(cells * 4);
    l.masks = l.sums + up(cells * 8);
    l.total = l.masks + up(cells * 32);
    return l;
}
struct CiPermArgs {
    CiArgs c;                    // the tests; c.type is DVS_CI_MI or DVS_CI_X2, c.out [T][3]
    int g2, sp, B, E, slices, blocks, lnk_cells;     // E: smc's stopping count, 0 otherwise; lnk_cells: launcher
    uint32_t seed_lo, seed_hi, test_offset;      // seed_lo / seed_hi: launcher, from `seed`
    int* counts;                 // workspace [T][blocks]
    double* sums;                // workspace [T][blocks]
    unsigned long long* masks;   // workspace [T][blocks][4]
    int* used;                   // [T]
};
void dvs_launch_ci_perm(const CiPermArgs& a, uint64_t seed, dvs_stream_t st);

// ---- Gaussian networks (dvs_gaussian.h; include/dvs_gaussian.h) ----------------------------------------------------------------
// The workspace of dvs_gbn_moments: the chunk column sums [n_sets][chunks][n], then the chunk cells [n_sets][chunks][n (n + 1) / 2].
struct GbnMomentLayout {
    size_t chunks, tri, cells, total;            // cells: byte offset of the chunk cells
};
inline GbnMomentLayout dvs_gbn_moment_layout(long long n, long long n_sets, long long set_size) {
    GbnMomentLayout l;
    l.chunks = (size_t)((set_size + DVS_GBN_CHUNK - 1) / DVS_GBN_CHUNK);
    l.tri = (size_t)(n * (n + 1) / 2);
    l.cells = (size_t)n_sets * l.chunks * (size_t)n * 8;
    l.total = l.cells + (size_t)n_sets * l.chunks * l.tri * 8;
    return l;
}
struct GbnMomentArgs {
    int n, n_sets, set_size, chunks, tri;        // chunks, tri: launcher
    const double* data;          // [n_samples][n]
    const int* rows;             // [n_sets][set_size] or null: the one set is the data in order
    double* sums;                // workspace [n_sets][chunks][n]
    double* cells;               // workspace [n_sets][chunks][tri]
    double* moments;             // [n_sets][DVS_GBN_STRIDE(n)]
};
void dvs_launch_gbn_moments(const GbnMomentArgs& a, dvs_stream_t st);

struct GbnScoreArgs {
    int B, n, type;              // type: dvs_gscore_type; the fit takes DVS_GSCORE_LOGLIK's refusals
    double arg, arg2, t;         // aic / bic: k (NaN: log(m) / 2 on the device); bge: alpha_mu, alpha_w and t
    const double* moments;       // [n_sets][DVS_GBN_STRIDE(n)]
    const int* set_of;           // [B] or null: set 0
    const uint64_t* parents;     // [B][n]
    double* local;               // [B][n]
    double* out;                 // [B]; unused by the toggle pass
    int* status;
};
void dvs_launch_gbn_scores(const GbnScoreArgs& a, dvs_stream_t st);
struct GbnToggleArgs {
    GbnScoreArgs s;
    const int* worklist;         // null: full pass; else i32 [2 B]
    double* toggles;             // T [B][n][n]
};
void dvs_launch_gbn_toggle(const GbnToggleArgs& a, dvs_stream_t st);
struct GbnFitArgs {
    GbnScoreArgs s;              // s.local, s.out unused
    double* coef;                // [B][n][n]
    double* intercept;           // [B][n]
    double* sd;                  // [B][n]
};
void dvs_launch_gbn_fit(const GbnFitArgs& a, dvs_stream_t st);

// ---- Gaussian CI tests (dvs_gaussian_ci.h; include/dvs_gaussian_ci.h) -----------------------------------------------------------
struct GbnCiArgs {
    int T, n, type;              // type: dvs_gci_type
    const double* moments;       // [n_sets][DVS_GBN_STRIDE(n)]
    const int* set_of;           // [T] or null: set 0
    const int* pairs;            // [T][2]: x, y
    const uint64_t* cond;        // [T]: bit z <=> z is in the conditioning set
    double* out;                 // [T][3]: statistic, df, p-value; NaN where refused
    int* status;
};
void dvs_launch_gbn_ci(const GbnCiArgs& a, dvs_stream_t st);
struct GbnCiGroupArgs {
    int G, n, type;
    const double* moments;       // [n_sets][DVS_GBN_STRIDE(n)]
    const int* set_of;           // [G] or null: set 0
    const int* target;           // [G]: x, factored once with Z
    const uint64_t* cond;        // [G]
    const uint64_t* candidates;  // [G]: bit c <=> c is tested against the target
    double* out;                 // [G][n][3]; NaN where not asked or refused
    int* status;
};
void dvs_launch_gbn_ci_group(const GbnCiGroupArgs& a, dvs_stream_t st);

// ---- a fitted Gaussian network (dvs_gaussian_params.h; include/dvs_gaussian_params.h) -------------------------------------------
struct GbnNet {
    int B, n;
    const uint64_t* parents;     // [B][n]
    const double* coef;          // [B][n][n], read at parent bits
    const double* intercept;     // [B][n]
    const double* sd;            // [B][n]
    int* status;
};
struct GbnJointArgs {
    GbnNet net;
    double* mean;                // [B][n]
    double* cov;                 // [B][n][n]
};
void dvs_launch_gbn_joint(const GbnJointArgs& a, dvs_stream_t st);
struct GbnQuantileArgs {
    long long count;
    const uint64_t* k;           // [count]
    double* z;                   // [count]
};
void dvs_launch_gbn_quantiles(const GbnQuantileArgs& a, dvs_stream_t st);
// The workspace of dvs_gbn_sample: a header of 64 i32, order [48] then the "drawable" word at index 48 (dvs_bn_sample's header).
constexpr size_t DVS_GBN_SAMPLE_WORKSPACE = 256;
struct GbnSampleArgs {
    GbnNet net;                  // net.B = 1
    long long rows;
    uint32_t seed_lo, seed_hi, row_offset;       // seed_lo / seed_hi: launcher, from `seed`
    int* header;                 // workspace: order [48], drawable at [48]
    double* out;                 // [rows][n]
};
void dvs_launch_gbn_sample(const GbnSampleArgs& a, uint64_t seed, dvs_stream_t st);
// dvs_gbn_loglik's workspace is dvs_bn_loglik_layout's: partials f64 [B][chunks], flags i32 (the first B of [B][n]), c f64 [B][n]
struct GbnRowArgs {
    GbnNet net;
    int chunks, bsplit, target, mode;            // bsplit: launcher, the parts the batch is cut into; target, mode: the prediction
    long long rows;
    const double* data;          // [rows][n]
    double* per_row;             // loglik: null or [B][rows]; predict: pred [B][rows]
    double* out;                 // loglik: [B]; predict: var [B]
    double* partials;            // loglik workspace [B][chunks]
    int* ok;                     // workspace [B]
    double* c;                   // loglik workspace [B][n]
};
void dvs_launch_gbn_loglik(const GbnRowArgs& a, dvs_stream_t st);
void dvs_launch_gbn_predict(const GbnRowArgs& a, dvs_stream_t st);

// ---- a multivariate normal conditioned on every row's observed part (dvs_gaussian_incomplete.h; include/dvs_gaussian_incomplete.h)
// The workspace of dvs_gbn_condition: the chunk sums f64 [chunks], the refused rows per chunk i32 [chunks], the chunks' covariance
// cells f64 [n (n + 1) / 2][chunks]; each array starts at a multiple of 256 bytes.
struct GbnConditionLayout {
    size_t partials, refused, cov, total, chunks;
};
inline GbnConditionLayout dvs_gbn_condition_layout(int n_vars, long long rows) {
    const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    GbnConditionLayout l;
    l.chunks = (size_t)((rows + 255) / 256);
    l.partials = 0;
    l.refused = up(l.chunks * 8);
    l.cov = l.refused + up(l.chunks * 4);
    l.total = l.cov + (size_t)n_vars * (n_vars + 1) / 2 * l.chunks * 8;
    return l;
}
struct GbnConditionArgs {
    int n, chunks;
    long long rows;
    const double* mean;          // [n]
    const double* cov;           // [n][n], the lower triangle is read
    const double* x;             // [rows][n]
    const uint64_t* observed;    // [rows]
    const int* order;            // null or [rows]
    double* completed;           // null or [rows][n]
    double* cvar;                // null or [rows][n]
    double* quad;                // null or [rows]
    double* logp;                // [rows]
    double* loglik;              // [1]
    double* ccov;                // null or [n][n]
    long long* counts;           // null or [1]
    double* partials;            // workspace [chunks]
    int* refused;                // workspace [chunks]
    double* cov_partials;        // workspace [n (n + 1) / 2][chunks]
    int* status;
};
void dvs_launch_gbn_condition(const GbnConditionArgs& a, dvs_stream_t st);

// ---- conditional Gaussian networks on mixed data (dvs_mixed.h; include/dvs_mixed.h) ----------------------------------------------
struct CgPartitionArgs {
    int n, S, n_req, q_pitch, words;             // words: launcher
    const uint64_t* data;        // [S][words]
    const uint8_t* card;         // [n], 0: continuous
    const uint64_t* masks;       // [n_req]
    int* count;                  // [n_req][q_pitch]
    int* start;                  // [n_req][q_pitch]
    int* order;                  // [n_req][S]
    int* status;
};
void dvs_launch_cg_partition(const CgPartitionArgs& a, dvs_stream_t st);
// The workspace of dvs_cg_moments: the exclusive prefix of every request's chunks per configuration, i32 [n_req][q_pitch + 1]
// (rows padded to 8 bytes), then the chunk column sums [n_req][slots][n] and the chunk cells [n_req][slots][n (n + 1) / 2].
struct CgMomentLayout {
    size_t slots, tri, pre_pitch, sums, cells, total;        // pre_pitch in i32; sums, cells: byte offsets
};
inline CgMomentLayout dvs_cg_moment_layout(long long n, long long S, long long n_req, long long q_pitch) {
    CgMomentLayout l;
    l.slots = (size_t)((S + DVS_GBN_CHUNK - 1) / DVS_GBN_CHUNK + q_pitch);
    l.tri = (size_t)(n * (n + 1) / 2);
    l.pre_pitch = (size_t)(2 * ((q_pitch + 2) / 2));
    l.sums = l.pre_pitch * 4 * (size_t)n_req;
    l.cells = l.sums + (size_t)n_req * l.slots * (size_t)n * 8;
    l.total = l.cells + (size_t)n_req * l.slots * l.tri * 8;
    return l;
}
struct CgMomentArgs {
    int n, S, n_req, q_pitch, slots, tri, pre_pitch;         // n: the continuous columns; slots, tri, pre_pitch: launcher
    const double* x;             // [S][n]
    const int* count;            // [n_req][q_pitch]
    const int* start;            // [n_req][q_pitch]
    const int* order;            // [n_req][S]
    int* pre;                    // workspace [n_req][pre_pitch]
    double* sums;                // workspace [n_req][slots][n]
    double* cells;               // workspace [n_req][slots][tri]
    double* moments;             // [n_req][q_pitch][DVS_GBN_STRIDE(n)]
};
void dvs_launch_cg_moments(const CgMomentArgs& a, dvs_stream_t st);

// dvs_cg_scores and dvs_cg_toggle_scores: the discrete cells come from the discrete scorer on `bn` (its parents, card and
// worklist are the copies k_cg_prep writes into the workspace); the continuous and the illegal ones are written after it
struct CgScoreArgs {
    int B, n, nc, S, type;       // type: dvs_cgscore_type
    double arg;                  // k; NaN: log(S) / 2 on the device
    const uint8_t* card;         // [n], 0: continuous
    const uint64_t* tables;      // [n_tables] addresses of moment blocks [q][DVS_GBN_STRIDE(nc)]
    const int* table_of;         // scores [B][n]; toggle pass [rows][n]
    const uint64_t* parents;     // [B][n]
    double* local;               // [B][n]
    double* out;                 // [B]; unused by the toggle pass
    int* status;
    uint64_t* bn_parents;        // workspace [B][n]
    uint8_t* bn_card;            // workspace [64]
    const int* worklist;         // toggle pass: null or [2 B]
    int* bn_worklist;            // workspace [2 B] (toggle pass with a worklist)
    double* toggles;             // toggle pass: T [B][n][n]
};
void dvs_launch_cg_scores(const CgScoreArgs& a, const BicArgs& bn, dvs_stream_t st);
void dvs_launch_cg_toggle(const CgScoreArgs& a, const ToggleArgs& bn, dvs_stream_t st);

struct CgFitArgs {
    int F, cells, n, nc;
    const uint8_t* card;
    const int* var;              // [F]
    const uint64_t* parents;     // [F]
    const uint64_t* table;       // [F]
    const long long* offset;     // [F + 1]
    double* coef;                // [cells][n]
    double* intercept;           // [cells]
    double* sd;                  // [cells]
    double* count;               // [cells]
    int* status;
};
void dvs_launch_cg_fit(const CgFitArgs& a, dvs_stream_t st);

// ---- a fitted conditional Gaussian network (dvs_mixed_params.h; include/dvs_mixed_params.h) ---------------------------------------
struct CgbnNet {
    int n, nc;
    long long cells;
    const uint8_t* card;         // [n], 0: continuous
    const uint64_t* parents;     // [n]
    const long long* offset;     // [n + 1]
    const double* coef;          // [cells][n], read at continuous parent bits
    const double* intercept;     // [cells]
    const double* sd;            // [cells]
    int* status;
};
// The workspace of the three entry points starts with a header of 64 i32: order [48], the "sound" word at index 48 (as
// dvs_bn_sample's header), the "a cell broke bit 6" word at index 49.  loglik: then the chunk sums f64 [chunks] (rounded up to 256
// bytes) and c f64 [cells]; predict: then c f64 [cells].
constexpr size_t DVS_CGBN_HEADER = 256;
inline size_t dvs_cgbn_loglik_c_offset(long long rows) { return DVS_CGBN_HEADER + ((((size_t)rows + 255) / 256 * 8 + 255) & ~(size_t)255); }
struct CgbnRowArgs {
    CgbnNet net;
    long long rows;
    int chunks, words, target, mode;             // chunks, words: launcher; target < 0: no target (sample, loglik)
    uint32_t seed_lo, seed_hi, row_offset;       // the sampler; seed_lo / seed_hi: launcher, from `seed`
    const uint64_t* packed;      // [rows][words]
    const double* x;             // [rows][nc]; unused by the sampler
    const double* prior;         // predict mode 2: null or [rows][r]
    double* per_row;             // sample: x_out [rows][nc]; loglik: null or [rows]; predict modes 0, 1: pred [rows]
    uint8_t* label;              // predict mode 2: pred [rows]
    double* out;                 // loglik: [1]; predict modes 0, 1: var [rows]
    double* posterior;           // predict mode 2: null or [rows][r]
    int* header;                 // workspace
    double* partials;            // loglik workspace [chunks]
    double* c;                   // loglik, predict workspace [cells]; null: the sampler
};
void dvs_launch_cgbn_sample(const CgbnRowArgs& a, uint64_t seed, dvs_stream_t st);
void dvs_launch_cgbn_loglik(const CgbnRowArgs& a, dvs_stream_t st);
void dvs_launch_cgbn_predict(const CgbnRowArgs& a, dvs_stream_t st);

struct BootRowsArgs {
    int n_sets, set_size, n_samples;
    uint32_t seed_lo, seed_hi, set_offset;       // seed_lo / seed_hi: launcher, from `seed`
    int* rows;                   // [n_sets][set_size]
};
void dvs_launch_bootstrap_rows(const BootRowsArgs& a, uint64_t seed, dvs_stream_t st);

struct ArcStrengthArgs {
    int B, n;
    const uint64_t* pdag;        // [B][n], the layout of CpdagArgs::pdag
    int* counts;                 // [n][n][2], accumulated into
};
void dvs_launch_arc_strength(const ArcStrengthArgs& a, dvs_stream_t st);

struct AvgNetArgs {
    int G, n;
    const int* counts;           // [G][n][n][2]
    const int* n_networks;       // [G]
    const int* min_any;          // [G]: < 0 asks for the estimated threshold
    uint64_t* parents;           // [G][n]
    int* info;                   // [G][4]: min_any used, arcs placed, pairs dropped for a cycle, ties
};
void dvs_launch_averaged_network(const AvgNetArgs& a, dvs_stream_t st);

// ---- row codec -> BIC parent masks (k_bic.hip) -----------------------------------------------------------------------
struct BicMaskArgs {
    int B, n, wide;
    const uint8_t* labels;       // [B][n]
    const void* preds;           // [B][n] u16 (wide == 0) or u64
    uint64_t* parents;           // [B][n]
    int* status;
};
void dvs_launch_bic_parent_masks(const BicMaskArgs& a, dvs_stream_t st);

// ---- GP predictor (k_bic.hip, k_gp_acq.hip) --------------------------------------------------------------------------
// The kernels take the length scale as the factors they multiply by: the launchers derive those fields from `lengthscale`.
inline double dvs_gp_inv2l2(double lengthscale) { return 0.5 / (lengthscale * lengthscale); }
inline double dvs_gp_inv_l2(double lengthscale) { return 1.0 / (lengthscale * lengthscale); }

struct GpArgs {
    int B, M, D;
    const float* x;              // [B][D] queries
    const float* z;              // [M][D] inducing points
    const double* alpha;         // [M]
    double outputscale, inv2l2, constant;        // inv2l2: launcher
    double* out;                 // [B]
};
void dvs_launch_gp_predict(const GpArgs& a, double lengthscale, dvs_stream_t st);

struct GpKernArgs {
    int na, nb, D, symmetric;
    const float* xa;
    const float* xb;
    double outputscale, inv2l2, inv_l2, inv_l3, inv_o;      // all but outputscale: launcher
    double* K;                   // forward: [na][nb]
    const double* G;             // backward: [na][nb]
    double* dxa;                 // backward: [na][D]
    double* rows;                // backward: [na][2]: d/dl, d/do partials
};
void dvs_launch_gp_kernel(const GpKernArgs& a, double lengthscale, dvs_stream_t st);
void dvs_launch_gp_kernel_bwd(const GpKernArgs& a, double lengthscale, dvs_stream_t st);

struct GpAcqArgs {
    int Q, M, D, ld, Mp, NT;     // Mp, NT: launcher
    const float* x;              // [Q][D]
    const float* z;              // [M][D]
    const double* W;             // [M][ld]: P in columns 0..M-1, alpha in column M
    double c0, outputscale, inv2l2, inv_l2, constant, best, xi, sig_floor;      // inv2l2, inv_l2, sig_floor: launcher
    double* mean;                // [Q]
    double* var;                 // [Q]
    double* ei;                  // [Q]
    float* grad;                 // [Q][D] or null
};
// Weak: the host-emulation build of the test suite (tests/emu/build.py) compiles a fixed list of sources without
// k_gp_acq.hip; there dvs_gp_acquire exists (the binding stays complete) and reports that the kernel is not built.
void dvs_launch_gp_acquire(const GpAcqArgs& a, double lengthscale, dvs_stream_t st) __attribute__((weak));
