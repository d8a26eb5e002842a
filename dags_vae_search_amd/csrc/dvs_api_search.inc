// Search-side entry points (included by dvs_api.hip): reconstruction matching, search candidates, the graph generator, the
// BN scorers, hill climbing, tabu, structure comparison, CI tests and PC-stable, BN parameters and inference (likelihood weighting, variable elimination), exact search, the exact arc posterior, order MCMC, arc strengths and the GP predictor.  Each validates, fills one argument block of dvs_search_args.h by
// field name and calls that block's launcher between call_begin() and call_end().

static int failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int fail_size(const char* what, size_t need) { return failf(14, "%s = %zu", what, need); }

// ---- reconstruction matching (dvs_match.h) ---------------------------------------------------------------------------
extern "C" int dvs_match_decoded(int32_t batch, int32_t n_vars, int32_t card, int32_t repeats, int32_t preds_are_u64,
                                 const uint8_t* labels, const void* preds, const void* states, size_t state_bytes,
                                 int32_t budget, uint8_t* flags, void* stream) {
    if (batch <= 0 || repeats <= 0) return fail(2, "dvs_match_decoded: batch and repeats must be > 0");
    if ((int64_t)batch * repeats > (int64_t)1 << 30) return fail(2, "dvs_match_decoded: batch * repeats must be <= 2^30");
    if (n_vars < 1 || n_vars > 45) return fail(3, "dvs_match_decoded: n_vars must be in [1, 45]");
    if (card < 1 || card > 45) return fail(3, "dvs_match_decoded: card must be in [1, 45]");
    if (!preds_are_u64 && n_vars > 16) return fail(12, "dvs_match_decoded: 16-bit predecessor rows hold at most 16 vertices");
    if (budget < 1) return fail(12, "dvs_match_decoded: budget must be >= 1");
    if (!labels || !preds || !states || !flags) return fail(10, "dvs_match_decoded: null pointer");
    const size_t need = (size_t)batch * repeats * sizeof(dvs_decode_state);
    if (state_bytes < need) return fail_size("dvs_match_decoded: state_bytes < batch * repeats * DVS_DECODE_STATE_BYTES", need);
    MatchArgs a;
    a.B = batch;
    a.n = n_vars;
    a.card = card;
    a.R = repeats;
    a.wide = preds_are_u64 ? 1 : 0;
    a.budget = budget;
    a.labels = labels;
    a.preds = preds;
    a.states = (const DvsDecodeState*)states;
    a.flags = flags;
    call_begin();
    dvs_launch_match_decoded(a, (dvs_stream_t)stream);
    return call_end("dvs_match_decoded");
}

// ---- search candidates (dvs_structs.h) -------------------------------------------------------------------------------
extern "C" int dvs_decoded_structures(int32_t batch, int32_t n_vars, int32_t preds_are_u64, const void* states,
                                      size_t state_bytes, uint64_t hash_mask, uint8_t* flags, uint8_t* labels, void* preds,
                                      uint64_t* keys, size_t keys_bytes, uint64_t* hashes, void* stream) {
    if (batch <= 0) return fail(2, "dvs_decoded_structures: batch must be > 0");
    if (batch > 1 << 30) return fail(2, "dvs_decoded_structures: batch must be <= 2^30");
    if (n_vars < 1 || n_vars > 45) return fail(3, "dvs_decoded_structures: n_vars must be in [1, 45]");
    if (!preds_are_u64 && n_vars > 16) return fail(12, "dvs_decoded_structures: 16-bit predecessor rows hold at most 16 vertices");
    if (!states || !flags || !labels || !preds || !keys || !hashes) return fail(10, "dvs_decoded_structures: null pointer");
    if (state_bytes < (size_t)batch * sizeof(dvs_decode_state))
        return fail_size("dvs_decoded_structures: state_bytes < batch * DVS_DECODE_STATE_BYTES", (size_t)batch * sizeof(dvs_decode_state));
    if (keys_bytes < (size_t)batch * n_vars * 8)
        return fail_size("dvs_decoded_structures: keys_bytes < batch * n_vars * 8", (size_t)batch * n_vars * 8);
    StructArgs a;
    a.B = batch;
    a.n = n_vars;
    a.wide = preds_are_u64 ? 1 : 0;
    a.hash_mask = hash_mask;
    a.states = (const DvsDecodeState*)states;
    a.flags = flags;
    a.labels = labels;
    a.preds = preds;
    a.keys = keys;
    a.hashes = hashes;
    call_begin();
    dvs_launch_decoded_structures(a, (dvs_stream_t)stream);
    return call_end("dvs_decoded_structures");
}

extern "C" int dvs_structset_filter(int32_t batch, int32_t n_vars, const uint64_t* sorted_hashes, const int64_t* order,
                                    const uint64_t* keys, size_t keys_bytes, const uint8_t* flags, int32_t seen_count,
                                    const uint64_t* seen_hashes, const uint64_t* seen_keys, size_t seen_keys_bytes,
                                    uint8_t* out, void* stream) {
    if (batch < 0 || seen_count < 0) return fail(2, "dvs_structset_filter: batch and seen_count must be >= 0");
    if (batch > 1 << 30) return fail(2, "dvs_structset_filter: batch must be <= 2^30");
    if (n_vars < 1 || n_vars > 45) return fail(3, "dvs_structset_filter: n_vars must be in [1, 45]");
    if (batch == 0) return 0;                    // an empty batch: nothing to judge, nothing is enqueued
    if (!sorted_hashes || !order || !keys || !flags || !out) return fail(10, "dvs_structset_filter: null pointer");
    if (seen_count > 0 && (!seen_hashes || !seen_keys)) return fail(10, "dvs_structset_filter: null pointer (seen set)");
    if (keys_bytes < (size_t)batch * n_vars * 8)
        return fail_size("dvs_structset_filter: keys_bytes < batch * n_vars * 8", (size_t)batch * n_vars * 8);
    if (seen_keys_bytes < (size_t)seen_count * n_vars * 8)
        return fail_size("dvs_structset_filter: seen_keys_bytes < seen_count * n_vars * 8", (size_t)seen_count * n_vars * 8);
    FilterArgs a;
    a.B = batch;
    a.n = n_vars;
    a.S = seen_count;
    a.sorted_hashes = sorted_hashes;
    a.order = order;
    a.keys = keys;
    a.flags = flags;
    a.seen_hashes = seen_hashes;
    a.seen_keys = seen_keys;
    a.out = out;
    call_begin();
    dvs_launch_structset_filter(a, (dvs_stream_t)stream);
    return call_end("dvs_structset_filter");
}

// ---- graph generator (dvs_generate.h) --------------------------------------------------------------------------------
extern "C" int dvs_generate_dags(int32_t batch, int32_t n_vars, int32_t card, int32_t preds_are_u64, const int32_t* num_edges,
                                 uint64_t seed, int64_t dag_offset, int32_t try_limit, int32_t flags, uint8_t* labels,
                                 void* preds, size_t preds_bytes, int32_t* attempts, void* stream) {
    if (batch <= 0) return fail(2, "dvs_generate_dags: batch must be > 0");
    if (batch > 1 << 30) return fail(2, "dvs_generate_dags: batch must be <= 2^30");
    if (n_vars < 2 || n_vars > 45) return fail(3, "dvs_generate_dags: n_vars must be in [2, 45]");
    if (card < 1 || card > 45) return fail(3, "dvs_generate_dags: card must be in [1, 45]");
    const int group = (flags >> DVS_GEN_GROUP_SHIFT) & 15;
    if ((flags & ~(7 | 15 << DVS_GEN_GROUP_SHIFT)) || group > 7) return fail(12, "dvs_generate_dags: unknown bits in flags");
    if (!(flags & DVS_GEN_LABELS_CHOICE) && card < n_vars)
        return fail(12, "dvs_generate_dags: labels without replacement ('sample') need card >= n_vars");
    if ((preds_are_u64 != 0) != (n_vars > 13))
        return fail(12, "dvs_generate_dags: predecessor rows are u16 for n_vars <= 13 and u64 above (preds_are_u64 does not match)");
    if (try_limit < 1 || try_limit > 4096) return fail(12, "dvs_generate_dags: try_limit must be in [1, 4096]");
    if (dag_offset < 0) return fail(12, "dvs_generate_dags: dag_offset must be >= 0");
    if (!num_edges || !labels || !preds || !attempts) return fail(10, "dvs_generate_dags: null pointer");
    const size_t need = (size_t)batch * n_vars * (preds_are_u64 ? 8 : 2);
    if (preds_bytes < need) return fail_size("dvs_generate_dags: preds_bytes < batch * n_vars * row bytes", need);
    // Lanes per DAG: attempts k G .. k G + G - 1 run side by side.  Spare lanes cost little until the launch holds about 16
    // waves per SIMD (measured, DESIGN.md §13: 64 lanes up to B = 4096, 16 at B = 65 536), and one lane is all an
    // always-accepted attempt 0 needs.
    int gshift = 0;
    if (group) {
        gshift = group - 1;
    } else if (!(flags & DVS_GEN_ACCEPT_NO_CONNECTIVITY)) {
        static const int cus = dvs_device_cus();
        const int64_t lanes = (int64_t)cus * 4 * 64 * 16;
        while (gshift < 6 && ((int64_t)batch << (gshift + 1)) <= lanes && (1 << gshift) < try_limit) ++gshift;
    }
    GenArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.card = card;
    a.try_limit = try_limit;
    a.flags = flags & 7;
    a.gshift = gshift;
    a.dag_offset = (uint32_t)dag_offset;
    a.num_edges = num_edges;
    a.labels = labels;
    a.preds = preds;
    a.attempts = attempts;
    call_begin();
    dvs_launch_generate_dags(a, seed, preds_are_u64 != 0, (dvs_stream_t)stream);
    return call_end("dvs_generate_dags");
}

extern "C" int dvs_generate_edge_counts(int32_t batch, int32_t n_entries, const int32_t* edge_counts, const int32_t* cum_weights,
                                        uint64_t seed, int64_t dag_offset, int32_t* num_edges, void* stream) {
    if (batch <= 0 || batch > 1 << 30) return fail(2, "dvs_generate_edge_counts: batch must be in [1, 2^30]");
    if (n_entries < 1 || n_entries > 1024) return fail(12, "dvs_generate_edge_counts: n_entries must be in [1, 1024]");
    if (dag_offset < 0) return fail(12, "dvs_generate_edge_counts: dag_offset must be >= 0");
    if (!edge_counts || !cum_weights || !num_edges) return fail(10, "dvs_generate_edge_counts: null pointer");
    call_begin();
    dvs_launch_generate_edge_counts(batch, n_entries, edge_counts, cum_weights, seed, (uint32_t)dag_offset, num_edges,
                                    (dvs_stream_t)stream);
    return call_end("dvs_generate_edge_counts");
}

// ---- BN scorers (k_bic.hip) ------------------------------------------------------------------------------------------
// score_type / score_arg of dvs_bn_scores and dvs_bn_toggle_scores -> the argument the kernels take (include/dvs.h): the
// resolved k (loglik 0, aic, bic; NaN = log(S) / 2 taken on the device) or iss (bde, bds)
static int bn_score_arg(const char* fn, int score_type, double score_arg, double* arg) {
    const bool dflt = score_arg != score_arg;               // NaN: the type's default
    *arg = score_arg;
    switch (score_type) {
        case DVS_SCORE_LOGLIK:
        case DVS_SCORE_K2:
        case DVS_SCORE_BDJ:
            if (!dflt) return failf(13, "%s: loglik, k2 and bdj take no argument (score_arg must be NaN)", fn);
            *arg = 0.0;                                     // loglik is the penalised likelihood at k = 0
            return 0;
        case DVS_SCORE_AIC:
        case DVS_SCORE_BIC:
            if (!dflt && !(score_arg >= 0.0 && isfinite(score_arg))) return failf(13, "%s: k must be finite and >= 0", fn);
            if (dflt && score_type == DVS_SCORE_AIC) *arg = 1.0;     // bic's default, log(S) / 2, is taken on the device
            return 0;
        case DVS_SCORE_BDE:
        case DVS_SCORE_BDS:
            if (!dflt && !(score_arg > 0.0 && isfinite(score_arg))) return failf(13, "%s: iss must be finite and > 0", fn);
            if (dflt) *arg = 1.0;
            return 0;
        default:
            return failf(12, "%s: score_type is not a dvs_score_type", fn);
    }
}

// ---- hill climbing, tabu, random restarts (dvs_hillclimb.h, dvs_tabu.h) ----------------------------------------------
// What dvs_bn_toggle_scores, dvs_hc_step, dvs_tabu_step and dvs_hc_perturb check alike, each at its own place in the entry
// point's order: the range of the toggle table's index and the caller's table and trace buffers (code 14 with the size).
struct HcCheck {
    const char* fn;
    int batch, n_vars;
    int dims() const {
        if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
        if ((int64_t)batch * n_vars * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: batch * n_vars^2 must be < 2^31", fn);
        return 0;
    }
    int toggles(size_t toggles_bytes) const {
        const size_t need = (size_t)batch * n_vars * n_vars * 8;
        return toggles_bytes < need ? failf(14, "%s: toggles_bytes < batch * n_vars^2 * 8 = %zu", fn, need) : 0;
    }
    int trace(const int64_t* trace, size_t trace_bytes, int step_cap) const {
        const size_t need = (size_t)batch * step_cap * 16;
        return trace && trace_bytes < need ? failf(14, "%s: trace_bytes < batch * step_cap * 16 = %zu", fn, need) : 0;
    }
};

// The five scorer entry points (dvs_bic_scores, dvs_bn_scores[_rows], dvs_bn_toggle_scores[_rows]) open with the same checks
// in the same order: sizes (2), n_vars (3; the toggle table's index range with it), pointers (10).
static int scorer_check(const char* fn, int batch, int n_vars, int n_samples, bool toggle_table, bool any_null) {
    if (batch <= 0 || n_samples <= 0) return failf(2, "%s: batch and n_samples must be > 0", fn);
    const HcCheck chk = {fn, batch, n_vars};
    if (toggle_table) {
        if (int e = chk.dims()) return e;
    } else if (n_vars < 1 || n_vars > DVS_WTOK) {
        return failf(3, "%s: n_vars must be in [1, 48]", fn);
    }
    return any_null ? failf(10, "%s: null pointer", fn) : 0;
}
// ... and fill one BicArgs; n_counted is the size of the data set a structure counts over (n_samples, or a row set's size).
// Fails as bn_score_arg does.
static int scorer_args(const char* fn, BicArgs& a, int batch, int n_vars, int n_counted, const uint64_t* data, const uint8_t* card,
                       const uint64_t* parents, int score_type, double score_arg, double* local, double* out, int32_t* status) {
    if (int e = bn_score_arg(fn, score_type, score_arg, &a.arg)) return e;
    a.B = batch;
    a.n = n_vars;
    a.S = n_counted;
    a.data = data;
    a.card = card;
    a.parents = parents;
    a.local = local;
    a.out = out;
    a.status = status;
    a.type = score_type;
    return 0;
}
// the caller's L and T buffers of the two toggle entry points (code 14 with the size)
static int toggle_buffers(const HcCheck& chk, size_t local_bytes, size_t toggles_bytes) {
    const size_t need = (size_t)chk.batch * chk.n_vars * 8;
    if (local_bytes < need) return failf(14, "%s: local_bytes < batch * n_vars * 8 = %zu", chk.fn, need);
    return chk.toggles(toggles_bytes);
}

static int bn_scores_call(const char* fn, int batch, int n_vars, int n_samples, const uint64_t* data, const uint8_t* card,
                          const uint64_t* parents, int score_type, double score_arg, double* scratch, double* out, int32_t* status,
                          void* stream) {
    if (int e = scorer_check(fn, batch, n_vars, n_samples, false, !data || !card || !parents || !scratch || !out || !status)) return e;
    BicArgs a = {};
    if (int e = scorer_args(fn, a, batch, n_vars, n_samples, data, card, parents, score_type, score_arg, scratch, out, status)) return e;
    call_begin();
    dvs_launch_bic(a, (dvs_stream_t)stream);
    return call_end(fn);
}
extern "C" int dvs_bic_scores(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                              const uint64_t* parents, double* scratch, double* out, int32_t* status, void* stream) {
    // bic with its default k: NaN stands for log(S) / 2, taken on the device
    return bn_scores_call("dvs_bic_scores", batch, n_vars, n_samples, data, card, parents, DVS_SCORE_BIC, __builtin_nan(""), scratch,
                          out, status, stream);
}
extern "C" int dvs_bn_scores(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                             const uint64_t* parents, int32_t score_type, double score_arg, double* scratch, double* out,
                             int32_t* status, void* stream) {
    return bn_scores_call("dvs_bn_scores", batch, n_vars, n_samples, data, card, parents, score_type, score_arg, scratch, out, status,
                          stream);
}

extern "C" int dvs_bn_toggle_scores(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                                    const uint64_t* parents, int32_t score_type, double score_arg, const int32_t* worklist,
                                    double* local, size_t local_bytes, double* toggles, size_t toggles_bytes, int32_t* status,
                                    void* stream) {
    const char* fn = "dvs_bn_toggle_scores";
    if (int e = scorer_check(fn, batch, n_vars, n_samples, true, !data || !card || !parents || !local || !toggles || !status)) return e;
    ToggleArgs t = {};
    if (int e = scorer_args(fn, t.s, batch, n_vars, n_samples, data, card, parents, score_type, score_arg, local, nullptr, status)) return e;
    if (int e = toggle_buffers({fn, batch, n_vars}, local_bytes, toggles_bytes)) return e;
    t.worklist = worklist;
    t.toggles = toggles;
    call_begin();
    dvs_launch_bn_toggle(t, (dvs_stream_t)stream);
    return call_end("dvs_bn_toggle_scores");
}

extern "C" int dvs_hc_step(int32_t batch, int32_t n_vars, uint64_t* parents, double* local, const double* toggles,
                           size_t toggles_bytes, int32_t max_parents, double min_delta, const uint64_t* forbidden,
                           int32_t step_cap, int32_t* worklist, int32_t* steps, int32_t* converged, int32_t* flags,
                           int64_t* trace, size_t trace_bytes, int32_t* active, void* stream) {
    const HcCheck chk = {"dvs_hc_step", batch, n_vars};
    if (batch <= 0) return fail(2, "dvs_hc_step: batch must be > 0");
    if (int e = chk.dims()) return e;
    if (!parents || !local || !toggles || !worklist || !steps || !converged || !flags || !active)
        return fail(10, "dvs_hc_step: null pointer");
    if (min_delta != min_delta) return fail(13, "dvs_hc_step: min_delta must not be NaN");
    if (step_cap < 1) return fail(13, "dvs_hc_step: step_cap must be >= 1");
    if (int e = chk.toggles(toggles_bytes)) return e;
    if (int e = chk.trace(trace, trace_bytes, step_cap)) return e;
    HcArgs a;
    a.B = batch;
    a.n = n_vars;
    a.max_parents = max_parents;
    a.step_cap = step_cap;
    a.min_delta = min_delta;
    a.parents = parents;
    a.local = local;
    a.toggles = toggles;
    a.forbidden = forbidden;
    a.worklist = worklist;
    a.steps = steps;
    a.converged = converged;
    a.flags = flags;
    a.trace = trace;
    a.active = active;
    call_begin();
    dvs_launch_hc_step(a, (dvs_stream_t)stream);
    return call_end("dvs_hc_step");
}

extern "C" int dvs_tabu_step(int32_t batch, int32_t n_vars, uint64_t* parents, double* local, const double* toggles,
                             size_t toggles_bytes, int32_t max_parents, double min_delta, const uint64_t* forbidden,
                             int32_t step_cap, int32_t* worklist, int32_t* steps, int32_t* converged, int32_t* flags,
                             int64_t* trace, size_t trace_bytes, int32_t* active, int32_t tabu_len, uint64_t* ring,
                             size_t ring_bytes, int32_t* visited, int32_t max_stall, int32_t* stall, double* best_score,
                             uint64_t* best_parents, size_t best_bytes, void* stream) {
    const HcCheck chk = {"dvs_tabu_step", batch, n_vars};
    if (batch <= 0) return fail(2, "dvs_tabu_step: batch must be > 0");
    if (int e = chk.dims()) return e;
    if (!parents || !local || !toggles || !worklist || !steps || !converged || !flags || !active || !ring || !visited || !stall ||
        !best_score || !best_parents)
        return fail(10, "dvs_tabu_step: null pointer");
    if (min_delta != min_delta) return fail(13, "dvs_tabu_step: min_delta must not be NaN");
    if (step_cap < 1) return fail(13, "dvs_tabu_step: step_cap must be >= 1");
    if (tabu_len < 1) return fail(13, "dvs_tabu_step: tabu_len must be >= 1");
    if (max_stall < 1) return fail(13, "dvs_tabu_step: max_stall must be >= 1");
    if (int e = chk.toggles(toggles_bytes)) return e;
    if (int e = chk.trace(trace, trace_bytes, step_cap)) return e;
    if (ring_bytes < (size_t)batch * tabu_len * n_vars * 8)
        return fail_size("dvs_tabu_step: ring_bytes < batch * tabu_len * n_vars * 8", (size_t)batch * tabu_len * n_vars * 8);
    if (best_bytes < (size_t)batch * n_vars * 8)
        return fail_size("dvs_tabu_step: best_bytes < batch * n_vars * 8", (size_t)batch * n_vars * 8);
    TabuArgs t;
    t.h.B = batch;
    t.h.n = n_vars;
    t.h.max_parents = max_parents;
    t.h.step_cap = step_cap;
    t.h.min_delta = min_delta;
    t.h.parents = parents;
    t.h.local = local;
    t.h.toggles = toggles;
    t.h.forbidden = forbidden;
    t.h.worklist = worklist;
    t.h.steps = steps;
    t.h.converged = converged;
    t.h.flags = flags;
    t.h.trace = trace;
    t.h.active = active;
    t.tabu_len = tabu_len;
    t.max_stall = max_stall;
    t.ring = ring;
    t.visited = visited;
    t.stall = stall;
    t.best_score = best_score;
    t.best_parents = best_parents;
    call_begin();
    dvs_launch_tabu_step(t, (dvs_stream_t)stream);
    return call_end("dvs_tabu_step");
}

extern "C" int dvs_hc_perturb(int32_t batch, int32_t n_vars, uint64_t* parents, double* local, const double* toggles,
                              size_t toggles_bytes, int32_t max_parents, const uint64_t* forbidden, int32_t* worklist,
                              int32_t* flags, uint64_t seed, uint32_t draw_index, void* stream) {
    const HcCheck chk = {"dvs_hc_perturb", batch, n_vars};
    if (batch <= 0) return fail(2, "dvs_hc_perturb: batch must be > 0");
    if (int e = chk.dims()) return e;
    if (!parents || !local || !toggles || !worklist || !flags) return fail(10, "dvs_hc_perturb: null pointer");
    if (int e = chk.toggles(toggles_bytes)) return e;
    PerturbArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.max_parents = max_parents;
    a.draw_index = draw_index;
    a.parents = parents;
    a.local = local;
    a.toggles = toggles;
    a.forbidden = forbidden;
    a.worklist = worklist;
    a.flags = flags;
    call_begin();
    dvs_launch_hc_perturb(a, seed, (dvs_stream_t)stream);
    return call_end("dvs_hc_perturb");
}

// ---- structure comparison (dvs_cpdag.h) ------------------------------------------------------------------------------
// What dvs_cpdag and dvs_pdag_compare check alike, first: the batch, n_vars and the range of the row index.
static int pdag_dims(const char* fn, int batch, int n_vars) {
    if (batch <= 0) return failf(2, "%s: batch must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if ((int64_t)batch * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: batch * n_vars must be < 2^31", fn);
    return 0;
}

extern "C" int dvs_cpdag(int32_t batch, int32_t n_vars, const uint64_t* parents, uint64_t* pdag, size_t pdag_bytes,
                         int32_t* flags, void* stream) {
    if (int e = pdag_dims("dvs_cpdag", batch, n_vars)) return e;
    if (!parents || !pdag || !flags) return fail(10, "dvs_cpdag: null pointer");
    if (pdag_bytes < (size_t)batch * n_vars * 8) return fail_size("dvs_cpdag: pdag_bytes < batch * n_vars * 8", (size_t)batch * n_vars * 8);
    CpdagArgs a;
    a.B = batch;
    a.n = n_vars;
    a.parents = parents;
    a.pdag = pdag;
    a.flags = flags;
    call_begin();
    dvs_launch_cpdag(a, (dvs_stream_t)stream);
    return call_end("dvs_cpdag");
}

extern "C" int dvs_pdag_compare(int32_t batch, int32_t n_vars, const uint64_t* a, const uint64_t* b, int32_t b_rows,
                                int32_t* counts, size_t counts_bytes, void* stream) {
    if (int e = pdag_dims("dvs_pdag_compare", batch, n_vars)) return e;
    if (!a || !b || !counts) return fail(10, "dvs_pdag_compare: null pointer");
    if (b_rows != 1 && b_rows != batch) return fail(12, "dvs_pdag_compare: b_rows must be 1 or batch");
    if (counts_bytes < (size_t)batch * 20) return fail_size("dvs_pdag_compare: counts_bytes < batch * 20", (size_t)batch * 20);
    PdagCompareArgs c;
    c.B = batch;
    c.n = n_vars;
    c.b_rows = b_rows;
    c.a = a;
    c.b = b;
    c.counts = counts;
    call_begin();
    dvs_launch_pdag_compare(c, (dvs_stream_t)stream);
    return call_end("dvs_pdag_compare");
}

// ---- conditional-independence tests and PC-stable (dvs_citest.h) -----------------------------------------------------
extern "C" int dvs_ci_tests(int32_t n_tests, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                            const int32_t* pairs, const uint64_t* cond, int32_t test_type, int32_t max_cells, double* out,
                            size_t out_bytes, int32_t* status, void* stream) {
    if (n_tests <= 0 || n_samples <= 0) return fail(2, "dvs_ci_tests: n_tests and n_samples must be > 0");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_ci_tests: n_vars must be in [1, 48]");
    if (test_type < DVS_CI_MI || test_type > DVS_CI_X2_ADF) return fail(12, "dvs_ci_tests: test_type is not a dvs_ci_type");
    if (max_cells < 1 || max_cells > DVS_CI_MAX_CELLS) return fail(13, "dvs_ci_tests: max_cells must be in [1, 36864]");
    if (!data || !card || !pairs || !cond || !out || !status) return fail(10, "dvs_ci_tests: null pointer");
    if (out_bytes < (size_t)n_tests * 24) return fail_size("dvs_ci_tests: out_bytes < n_tests * 24", (size_t)n_tests * 24);
    CiArgs a = {};
    a.T = n_tests;
    a.n = n_vars;
    a.S = n_samples;
    a.type = test_type;
    a.max_cells = max_cells;
    a.data = data;
    a.card = card;
    a.pairs = pairs;
    a.cond = cond;
    a.out = out;
    a.status = status;
    call_begin();
    dvs_launch_ci_tests(a, (dvs_stream_t)stream);
    return call_end("dvs_ci_tests");
}

// ---- grouped CI tests and the MMPC round (dvs_local.h; include/dvs_local.h) ----------------------------------------------
extern "C" int dvs_ci_tests_group(int32_t n_groups, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                                  const int32_t* target, const uint64_t* cond, const uint64_t* candidates, int32_t test_type,
                                  int32_t lds_cells, double* out, size_t out_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_ci_tests_group";
    if (n_groups <= 0 || n_samples <= 0) return failf(2, "%s: n_groups and n_samples must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (test_type < DVS_CI_MI || test_type > DVS_CI_X2_ADF) return failf(12, "%s: test_type is not a dvs_ci_type", fn);
    if (lds_cells < 1 || lds_cells > DVS_CI_MAX_CELLS) return failf(13, "%s: lds_cells must be in [1, 36864]", fn);
    if ((int64_t)n_groups * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: n_groups * n_vars must be < 2^31", fn);
    if (!data || !card || !target || !cond || !candidates || !out || !status) return failf(10, "%s: null pointer", fn);
    if (out_bytes < (size_t)n_groups * n_vars * 24)
        return fail_size("dvs_ci_tests_group: out_bytes < n_groups * n_vars * 24", (size_t)n_groups * n_vars * 24);
    CiGroupArgs a = {};
    a.G = n_groups;
    a.n = n_vars;
    a.S = n_samples;
    a.type = test_type;
    a.lds_cells = lds_cells;
    a.data = data;
    a.card = card;
    a.target = target;
    a.cond = cond;
    a.candidates = candidates;
    a.out = out;
    a.status = status;
    call_begin();
    dvs_launch_ci_tests_group(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_mmpc_update(int32_t n_vars, int32_t n_groups, int32_t phase, const int32_t* target, const uint64_t* cond,
                               const uint64_t* candidates, const int64_t* group_offsets, const double* out, size_t out_bytes,
                               double alpha, const uint64_t* cpc, const uint64_t* cand, uint64_t* cpc_next, uint64_t* cand_next,
                               int32_t* last, double* pmax, double* smin, uint64_t* sepset, size_t state_bytes, int32_t* refused,
                               int64_t* result, size_t result_bytes, void* stream) {
    const char* fn = "dvs_mmpc_update";
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (n_groups <= 0) return failf(2, "%s: n_groups must be > 0", fn);
    if ((int64_t)n_groups * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: n_groups * n_vars must be < 2^31", fn);
    if (phase != 0 && phase != 1) return failf(13, "%s: phase must be 0 (forward) or 1 (backward)", fn);
    if (!(alpha >= 0.0 && alpha <= 1.0)) return failf(13, "%s: alpha must be in [0, 1]", fn);
    if (!target || !cond || !candidates || !group_offsets || !out || !cpc || !cand || !cpc_next || !cand_next || !last || !pmax ||
        !smin || !sepset || !refused || !result)
        return failf(10, "%s: null pointer", fn);
    if (out_bytes < (size_t)n_groups * n_vars * 24)
        return fail_size("dvs_mmpc_update: out_bytes < n_groups * n_vars * 24", (size_t)n_groups * n_vars * 24);
    if (state_bytes < (size_t)n_vars * n_vars * 8)
        return fail_size("dvs_mmpc_update: state_bytes < n_vars^2 * 8", (size_t)n_vars * n_vars * 8);
    if (result_bytes < (size_t)n_vars * 16) return fail_size("dvs_mmpc_update: result_bytes < n_vars * 16", (size_t)n_vars * 16);
    MmpcUpdateArgs a = {};
    a.n = n_vars;
    a.G = n_groups;
    a.phase = phase;
    a.alpha = alpha;
    a.target = target;
    a.cond = cond;
    a.candidates = candidates;
    a.offsets = (const long long*)group_offsets;
    a.out = out;
    a.cpc = cpc;
    a.cand = cand;
    a.cpc_next = cpc_next;
    a.cand_next = cand_next;
    a.last = last;
    a.pmax = pmax;
    a.smin = smin;
    a.sepset = sepset;
    a.refused = refused;
    a.result = (long long*)result;
    call_begin();
    dvs_launch_mmpc_update(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- Monte Carlo permutation CI tests (dvs_permtest.h; include/dvs_permtest.h) -------------------------------------------
static bool ci_perm_too_many(int n_tests, int n_perm) { return (int64_t)n_tests * ((n_perm + 255) / 256) > (int64_t)0x7fffffff; }

extern "C" size_t dvs_ci_perm_workspace_bytes(int32_t n_tests, int32_t n_perm) {
    const char* fn = "dvs_ci_perm_workspace_bytes";
    if (n_tests <= 0) return failf(2, "%s: n_tests must be > 0", fn), 0;
    if (n_perm < 1 || n_perm > DVS_CI_PERM_MAX) return failf(13, "%s: n_perm must be in [1, 2^20]", fn), 0;
    if (ci_perm_too_many(n_tests, n_perm)) return failf(2, "%s: n_tests * blocks must be < 2^31", fn), 0;
    return dvs_ci_perm_layout(n_tests, n_perm).total;
}

extern "C" int dvs_ci_perm_tests(int32_t n_tests, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                                 const int32_t* pairs, const uint64_t* cond, int32_t perm_type, int32_t n_perm, double alpha,
                                 uint64_t seed, uint32_t test_offset, int32_t slices, int32_t max_cells, void* workspace,
                                 size_t workspace_bytes, double* out, size_t out_bytes, int32_t* used, int32_t* status, void* stream) {
    const char* fn = "dvs_ci_perm_tests";
    if (n_tests <= 0 || n_samples <= 0) return failf(2, "%s: n_tests and n_samples must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (perm_type < DVS_CI_MC_MI || perm_type > DVS_CI_SP_X2) return failf(12, "%s: perm_type is not a dvs_ci_perm_type", fn);
    if (n_perm < 1 || n_perm > DVS_CI_PERM_MAX) return failf(13, "%s: n_perm must be in [1, 2^20]", fn);
    const bool smc = perm_type == DVS_CI_SMC_MI || perm_type == DVS_CI_SMC_X2;
    if (smc && !(alpha > 0.0 && alpha < 1.0)) return failf(13, "%s: alpha must be in (0, 1)", fn);
    const CiPermLayout l = dvs_ci_perm_layout(n_tests, n_perm);
    if (slices < 1 || (size_t)slices > l.blocks) return failf(13, "%s: slices must be in [1, ceil(n_perm / 256)]", fn);
    if (max_cells < 1 || max_cells > DVS_CI_MAX_CELLS) return failf(13, "%s: max_cells must be in [1, 36864]", fn);
    if (ci_perm_too_many(n_tests, n_perm)) return failf(2, "%s: n_tests * blocks must be < 2^31", fn);
    if (!data || !card || !pairs || !cond || !workspace || !out || !used || !status) return failf(10, "%s: null pointer", fn);
    if (workspace_bytes < l.total) return fail_size("dvs_ci_perm_tests: workspace_bytes < dvs_ci_perm_workspace_bytes", l.total);
    if (out_bytes < (size_t)n_tests * 24) return fail_size("dvs_ci_perm_tests: out_bytes < n_tests * 24", (size_t)n_tests * 24);
    CiPermArgs a = {};
    a.g2 = (perm_type & 1) == 0;
    a.sp = perm_type == DVS_CI_SP_MI || perm_type == DVS_CI_SP_X2;
    a.c.T = n_tests;
    a.c.n = n_vars;
    a.c.S = n_samples;
    a.c.type = a.g2 ? DVS_CI_MI : DVS_CI_X2;
    a.c.max_cells = max_cells;
    a.c.data = data;
    a.c.card = card;
    a.c.pairs = pairs;
    a.c.cond = cond;
    a.c.out = out;
    a.c.status = status;
    a.B = n_perm;
    a.E = smc ? (int)floor(alpha * (double)n_perm) + 1 : 0;
    a.slices = slices;
    a.blocks = (int)l.blocks;
    a.test_offset = test_offset;
    a.counts = (int*)((char*)workspace + l.counts);
    a.sums = (double*)((char*)workspace + l.sums);
    a.masks = (unsigned long long*)((char*)workspace + l.masks);
    a.used = used;
    call_begin();
    dvs_launch_ci_perm(a, seed, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- Gaussian networks (dvs_gaussian.h; include/dvs_gaussian.h) ----------------------------------------------------------------
static int gbn_moment_dims(const char* fn, int n_vars, int n_sets, int set_size) {
    if (n_sets <= 0 || set_size <= 0) return failf(2, "%s: n_sets and set_size must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    return 0;
}
static bool gbn_moment_too_many(const GbnMomentLayout& l, int n_sets) {
    return (double)n_sets * (double)l.chunks * (double)l.tri > 2147483647.0;
}

extern "C" size_t dvs_gbn_moments_workspace_bytes(int32_t n_vars, int32_t n_sets, int32_t set_size) {
    const char* fn = "dvs_gbn_moments_workspace_bytes";
    if (gbn_moment_dims(fn, n_vars, n_sets, set_size)) return 0;
    const GbnMomentLayout l = dvs_gbn_moment_layout(n_vars, n_sets, set_size);
    if (gbn_moment_too_many(l, n_sets)) return failf(2, "%s: n_sets * chunks * n (n + 1) / 2 must be < 2^31", fn), 0;
    return l.total;
}

extern "C" int dvs_gbn_moments(int32_t n_vars, int32_t n_samples, const double* data, const int32_t* rows, int32_t n_sets,
                               int32_t set_size, void* workspace, size_t workspace_bytes, double* moments, size_t moments_bytes,
                               void* stream) {
    const char* fn = "dvs_gbn_moments";
    if (n_samples <= 0) return failf(2, "%s: n_samples must be > 0", fn);
    if (int e = gbn_moment_dims(fn, n_vars, n_sets, set_size)) return e;
    if (!rows && (n_sets != 1 || set_size != n_samples))
        return failf(13, "%s: without rows there is one set of n_samples rows", fn);
    const GbnMomentLayout l = dvs_gbn_moment_layout(n_vars, n_sets, set_size);
    if (gbn_moment_too_many(l, n_sets)) return failf(2, "%s: n_sets * chunks * n (n + 1) / 2 must be < 2^31", fn);
    if (!data || !workspace || !moments) return failf(10, "%s: null pointer", fn);
    if (workspace_bytes < l.total) return fail_size("dvs_gbn_moments: workspace_bytes < dvs_gbn_moments_workspace_bytes", l.total);
    const size_t need = (size_t)n_sets * DVS_GBN_STRIDE(n_vars) * 8;
    if (moments_bytes < need) return fail_size("dvs_gbn_moments: moments_bytes < n_sets * DVS_GBN_STRIDE(n_vars) * 8", need);
    GbnMomentArgs a = {};
    a.n = n_vars;
    a.n_sets = n_sets;
    a.set_size = set_size;
    a.data = data;
    a.rows = rows;
    a.sums = (double*)workspace;
    a.cells = (double*)((char*)workspace + l.cells);
    a.moments = moments;
    call_begin();
    dvs_launch_gbn_moments(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// score_type and its arguments -> the fields the kernels read (include/dvs_gaussian.h)
static int gbn_score_args(const char* fn, GbnScoreArgs& a, int n_vars, int score_type, double arg, double arg2) {
    const bool dflt = arg != arg, dflt2 = arg2 != arg2;
    a.type = score_type;
    a.arg = arg;
    a.arg2 = arg2;
    a.t = 0.0;
    switch (score_type) {
        case DVS_GSCORE_LOGLIK:
            if (!dflt || !dflt2) return failf(13, "%s: loglik-g takes no argument (score_arg and score_arg2 must be NaN)", fn);
            return 0;
        case DVS_GSCORE_AIC:
        case DVS_GSCORE_BIC:
            if (!dflt && !(arg >= 0.0 && isfinite(arg))) return failf(13, "%s: k must be finite and >= 0", fn);
            if (!dflt2) return failf(13, "%s: score_arg2 is bge's alpha_w (must be NaN)", fn);
            if (dflt && score_type == DVS_GSCORE_AIC) a.arg = 1.0;       // bic's default, log(m) / 2, is taken on the device
            return 0;
        case DVS_GSCORE_BGE:
            if (dflt) a.arg = 1.0;
            if (dflt2) a.arg2 = (double)n_vars + 2.0;
            if (!(a.arg > 0.0 && isfinite(a.arg))) return failf(13, "%s: alpha_mu must be finite and > 0", fn);
            if (!(a.arg2 > (double)n_vars + 1.0 && isfinite(a.arg2))) return failf(13, "%s: alpha_w must be finite and > n_vars + 1", fn);
            a.t = a.arg * (a.arg2 - (double)n_vars - 1.0) / (a.arg + 1.0);
            return 0;
        default:
            return failf(12, "%s: score_type is not a dvs_gscore_type", fn);
    }
}
// what the three family entry points check first: sizes (2), n_vars (3; the table's index range with it)
static int gbn_dims(const char* fn, int batch, int n_vars, int n_sets, bool table) {
    if (batch <= 0 || n_sets <= 0) return failf(2, "%s: batch and n_sets must be > 0", fn);
    if (table) return HcCheck{fn, batch, n_vars}.dims();
    return n_vars < 1 || n_vars > DVS_WTOK ? failf(3, "%s: n_vars must be in [1, 48]", fn) : 0;
}
static void gbn_fill(GbnScoreArgs& a, int batch, int n_vars, const double* moments, const int32_t* set_of, const uint64_t* parents,
                     double* local, double* out, int32_t* status) {
    a.B = batch;
    a.n = n_vars;
    a.moments = moments;
    a.set_of = set_of;
    a.parents = parents;
    a.local = local;
    a.out = out;
    a.status = status;
}

extern "C" int dvs_gbn_scores(int32_t batch, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                              const uint64_t* parents, int32_t score_type, double score_arg, double score_arg2, double* local,
                              double* out, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_scores";
    if (int e = gbn_dims(fn, batch, n_vars, n_sets, false)) return e;
    GbnScoreArgs a = {};
    if (int e = gbn_score_args(fn, a, n_vars, score_type, score_arg, score_arg2)) return e;
    if (!moments || !parents || !local || !out || !status) return failf(10, "%s: null pointer", fn);
    gbn_fill(a, batch, n_vars, moments, set_of, parents, local, out, status);
    call_begin();
    dvs_launch_gbn_scores(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_gbn_toggle_scores(int32_t batch, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                                     const uint64_t* parents, int32_t score_type, double score_arg, double score_arg2,
                                     const int32_t* worklist, double* local, size_t local_bytes, double* toggles,
                                     size_t toggles_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_toggle_scores";
    if (int e = gbn_dims(fn, batch, n_vars, n_sets, true)) return e;
    GbnToggleArgs t = {};
    if (int e = gbn_score_args(fn, t.s, n_vars, score_type, score_arg, score_arg2)) return e;
    if (!moments || !parents || !local || !toggles || !status) return failf(10, "%s: null pointer", fn);
    if (int e = toggle_buffers({fn, batch, n_vars}, local_bytes, toggles_bytes)) return e;
    gbn_fill(t.s, batch, n_vars, moments, set_of, parents, local, nullptr, status);
    t.worklist = worklist;
    t.toggles = toggles;
    call_begin();
    dvs_launch_gbn_toggle(t, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_gbn_fit(int32_t batch, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                           const uint64_t* parents, double* coef, size_t coef_bytes, double* intercept, double* sd,
                           int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_fit";
    if (int e = gbn_dims(fn, batch, n_vars, n_sets, true)) return e;
    if (!moments || !parents || !coef || !intercept || !sd || !status) return failf(10, "%s: null pointer", fn);
    const size_t need = (size_t)batch * n_vars * n_vars * 8;
    if (coef_bytes < need) return fail_size("dvs_gbn_fit: coef_bytes < batch * n_vars^2 * 8", need);
    GbnFitArgs t = {};
    t.s.type = DVS_GSCORE_LOGLIK;
    gbn_fill(t.s, batch, n_vars, moments, set_of, parents, nullptr, nullptr, status);
    t.coef = coef;
    t.intercept = intercept;
    t.sd = sd;
    call_begin();
    dvs_launch_gbn_fit(t, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- conditional Gaussian networks on mixed data (dvs_mixed.h; include/dvs_mixed.h) ----------------------------------------------
static int cg_pitch(const char* fn, int q_pitch) {
    return q_pitch < 1 || q_pitch > DVS_CG_MAX_CONFIGS ? failf(13, "%s: q_pitch must be in [1, %d]", fn, DVS_CG_MAX_CONFIGS) : 0;
}

extern "C" int dvs_cg_partition(int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card, int32_t n_requests,
                                const uint64_t* masks, int32_t q_pitch, int32_t* count, size_t count_bytes, int32_t* start,
                                int32_t* order, size_t order_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_cg_partition";
    if (n_requests <= 0 || n_samples <= 0) return failf(2, "%s: n_requests and n_samples must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (int e = cg_pitch(fn, q_pitch)) return e;
    if ((int64_t)n_requests * (q_pitch > n_samples ? q_pitch : n_samples) > (int64_t)0x7fffffff)
        return failf(2, "%s: n_requests * max(q_pitch, n_samples) must be < 2^31", fn);
    if (!data || !card || !masks || !count || !start || !order || !status) return failf(10, "%s: null pointer", fn);
    const size_t need = (size_t)n_requests * q_pitch * 4, need_order = (size_t)n_requests * n_samples * 4;
    if (count_bytes < need) return fail_size("dvs_cg_partition: count_bytes < n_requests * q_pitch * 4", need);
    if (order_bytes < need_order) return fail_size("dvs_cg_partition: order_bytes < n_requests * n_samples * 4", need_order);
    CgPartitionArgs a = {};
    a.n = n_vars;
    a.S = n_samples;
    a.n_req = n_requests;
    a.q_pitch = q_pitch;
    a.data = data;
    a.card = card;
    a.masks = masks;
    a.count = count;
    a.start = start;
    a.order = order;
    a.status = status;
    call_begin();
    dvs_launch_cg_partition(a, (dvs_stream_t)stream);
    return call_end(fn);
}

static int cg_moment_dims(const char* fn, int n_cont, int n_samples, int n_requests, int q_pitch) {
    if (n_requests <= 0 || n_samples <= 0) return failf(2, "%s: n_requests and n_samples must be > 0", fn);
    if (n_cont < 1 || n_cont > DVS_WTOK) return failf(3, "%s: n_cont must be in [1, 48]", fn);
    if (int e = cg_pitch(fn, q_pitch)) return e;
    const CgMomentLayout l = dvs_cg_moment_layout(n_cont, n_samples, n_requests, q_pitch);
    const double tri = (double)l.tri;
    if ((double)n_requests * (double)l.slots * tri > 2147483647.0 || (double)n_requests * (double)q_pitch * tri > 2147483647.0)
        return failf(2, "%s: n_requests * slots * n (n + 1) / 2 and n_requests * q_pitch * n (n + 1) / 2 must be < 2^31", fn);
    return 0;
}

extern "C" size_t dvs_cg_moments_workspace_bytes(int32_t n_cont, int32_t n_samples, int32_t n_requests, int32_t q_pitch) {
    if (cg_moment_dims("dvs_cg_moments_workspace_bytes", n_cont, n_samples, n_requests, q_pitch)) return 0;
    return dvs_cg_moment_layout(n_cont, n_samples, n_requests, q_pitch).total;
}

extern "C" int dvs_cg_moments(int32_t n_cont, int32_t n_samples, const double* x, int32_t n_requests, int32_t q_pitch,
                              const int32_t* count, const int32_t* start, const int32_t* order, void* workspace,
                              size_t workspace_bytes, double* moments, size_t moments_bytes, void* stream) {
    const char* fn = "dvs_cg_moments";
    if (int e = cg_moment_dims(fn, n_cont, n_samples, n_requests, q_pitch)) return e;
    if (!x || !count || !start || !order || !workspace || !moments) return failf(10, "%s: null pointer", fn);
    const CgMomentLayout l = dvs_cg_moment_layout(n_cont, n_samples, n_requests, q_pitch);
    if (workspace_bytes < l.total) return fail_size("dvs_cg_moments: workspace_bytes < dvs_cg_moments_workspace_bytes", l.total);
    const size_t need = (size_t)n_requests * q_pitch * DVS_GBN_STRIDE(n_cont) * 8;
    if (moments_bytes < need) return fail_size("dvs_cg_moments: moments_bytes < n_requests * q_pitch * DVS_GBN_STRIDE(n_cont) * 8", need);
    CgMomentArgs a = {};
    a.n = n_cont;
    a.S = n_samples;
    a.n_req = n_requests;
    a.q_pitch = q_pitch;
    a.x = x;
    a.count = count;
    a.start = start;
    a.order = order;
    a.pre = (int*)workspace;
    a.sums = (double*)((char*)workspace + l.sums);
    a.cells = (double*)((char*)workspace + l.cells);
    a.moments = moments;
    call_begin();
    dvs_launch_cg_moments(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// what dvs_cg_scores and dvs_cg_toggle_scores check alike and the two blocks they fill: a for the continuous and the illegal
// cells, bn for the discrete scorer on the workspace's copy of the structures
static int cg_score_check(const char* fn, int batch, int n_vars, int n_cont, int n_samples, bool table) {
    if (batch <= 0 || n_samples <= 0) return failf(2, "%s: batch and n_samples must be > 0", fn);
    if (table) {
        if (int e = HcCheck{fn, batch, n_vars}.dims()) return e;
    } else if (n_vars < 1 || n_vars > DVS_WTOK) {
        return failf(3, "%s: n_vars must be in [1, 48]", fn);
    }
    return n_cont < 0 || n_cont > n_vars ? failf(3, "%s: n_cont must be in [0, n_vars]", fn) : 0;
}
static size_t cg_workspace(int batch, int n_vars, bool toggle) {
    return (size_t)batch * n_vars * 8 + 64 + (toggle ? (size_t)batch * 8 : 0);
}
static int cg_fill(const char* fn, CgScoreArgs& a, BicArgs& bn, int batch, int n_vars, int n_cont, int n_samples, const uint64_t* data,
                   const uint8_t* card, const uint64_t* tables, const int32_t* table_of, const uint64_t* parents, int score_type,
                   double score_arg, void* workspace, double* local, double* out, int32_t* status) {
    a.B = batch;
    a.n = n_vars;
    a.nc = n_cont;
    a.S = n_samples;
    a.type = score_type;
    a.card = card;
    a.tables = tables;
    a.table_of = table_of;
    a.parents = parents;
    a.local = local;
    a.out = out;
    a.status = status;
    a.bn_parents = (uint64_t*)workspace;
    a.bn_card = (uint8_t*)workspace + (size_t)batch * n_vars * 8;
    a.bn_worklist = (int*)(a.bn_card + 64);
    // dvs_cgscore_type and dvs_score_type agree on loglik, aic, bic: the discrete scorer's own argument rules
    if (int e = scorer_args(fn, bn, batch, n_vars, n_samples, data, a.bn_card, a.bn_parents, score_type, score_arg, local, out, status))
        return e;
    a.arg = bn.arg;
    return 0;
}
static_assert(DVS_CGSCORE_LOGLIK == (int)DVS_SCORE_LOGLIK && DVS_CGSCORE_AIC == (int)DVS_SCORE_AIC && DVS_CGSCORE_BIC == (int)DVS_SCORE_BIC,
              "the mixed scores hand their type to the discrete scorer");

extern "C" size_t dvs_cg_scores_workspace_bytes(int32_t batch, int32_t n_vars) {
    if (cg_score_check("dvs_cg_scores_workspace_bytes", batch, n_vars, 0, 1, false)) return 0;
    return cg_workspace(batch, n_vars, false);
}
extern "C" size_t dvs_cg_toggle_workspace_bytes(int32_t batch, int32_t n_vars) {
    if (cg_score_check("dvs_cg_toggle_workspace_bytes", batch, n_vars, 0, 1, true)) return 0;
    return cg_workspace(batch, n_vars, true);
}

extern "C" int dvs_cg_scores(int32_t batch, int32_t n_vars, int32_t n_cont, int32_t n_samples, const uint64_t* data,
                             const uint8_t* card, const uint64_t* tables, const int32_t* table_of, const uint64_t* parents,
                             int32_t score_type, double score_arg, void* workspace, size_t workspace_bytes, double* local,
                             double* out, int32_t* status, void* stream) {
    const char* fn = "dvs_cg_scores";
    if (int e = cg_score_check(fn, batch, n_vars, n_cont, n_samples, false)) return e;
    if (score_type < DVS_CGSCORE_LOGLIK || score_type > DVS_CGSCORE_BIC) return failf(12, "%s: score_type is not a dvs_cgscore_type", fn);
    CgScoreArgs a = {};
    BicArgs bn = {};
    if (int e = cg_fill(fn, a, bn, batch, n_vars, n_cont, n_samples, data, card, tables, table_of, parents, score_type, score_arg,
                        workspace, local, out, status))
        return e;
    if (!data || !card || !parents || !workspace || !local || !out || !status || (n_cont > 0 && (!tables || !table_of)))
        return failf(10, "%s: null pointer", fn);
    const size_t need = cg_workspace(batch, n_vars, false);
    if (workspace_bytes < need) return fail_size("dvs_cg_scores: workspace_bytes < dvs_cg_scores_workspace_bytes", need);
    call_begin();
    dvs_launch_cg_scores(a, bn, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_cg_toggle_scores(int32_t batch, int32_t n_vars, int32_t n_cont, int32_t n_samples, const uint64_t* data,
                                    const uint8_t* card, const uint64_t* tables, const int32_t* table_of, const uint64_t* parents,
                                    int32_t score_type, double score_arg, const int32_t* worklist, void* workspace,
                                    size_t workspace_bytes, double* local, size_t local_bytes, double* toggles, size_t toggles_bytes,
                                    int32_t* status, void* stream) {
    const char* fn = "dvs_cg_toggle_scores";
    if (int e = cg_score_check(fn, batch, n_vars, n_cont, n_samples, true)) return e;
    if (score_type < DVS_CGSCORE_LOGLIK || score_type > DVS_CGSCORE_BIC) return failf(12, "%s: score_type is not a dvs_cgscore_type", fn);
    CgScoreArgs a = {};
    ToggleArgs bn = {};
    if (int e = cg_fill(fn, a, bn.s, batch, n_vars, n_cont, n_samples, data, card, tables, table_of, parents, score_type, score_arg,
                        workspace, local, nullptr, status))
        return e;
    if (!data || !card || !parents || !workspace || !local || !toggles || !status || (n_cont > 0 && (!tables || !table_of)))
        return failf(10, "%s: null pointer", fn);
    const size_t need = cg_workspace(batch, n_vars, true);
    if (workspace_bytes < need) return fail_size("dvs_cg_toggle_scores: workspace_bytes < dvs_cg_toggle_workspace_bytes", need);
    if (int e = toggle_buffers({fn, batch, n_vars}, local_bytes, toggles_bytes)) return e;
    a.worklist = worklist;
    a.toggles = toggles;
    bn.worklist = worklist ? a.bn_worklist : nullptr;
    bn.toggles = toggles;
    call_begin();
    dvs_launch_cg_toggle(a, bn, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_cg_fit(int32_t n_families, int32_t n_cells, int32_t n_vars, int32_t n_cont, const uint8_t* card,
                          const int32_t* var, const uint64_t* parents, const uint64_t* table, const int64_t* offset, double* coef,
                          size_t coef_bytes, double* intercept, double* sd, double* count, int32_t* status, void* stream) {
    const char* fn = "dvs_cg_fit";
    if (n_families <= 0 || n_cells <= 0) return failf(2, "%s: n_families and n_cells must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (n_cont < 1 || n_cont > n_vars) return failf(3, "%s: n_cont must be in [1, n_vars]", fn);
    if ((int64_t)n_cells * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: n_cells * n_vars must be < 2^31", fn);
    if (!card || !var || !parents || !table || !offset || !coef || !intercept || !sd || !count || !status)
        return failf(10, "%s: null pointer", fn);
    const size_t need = (size_t)n_cells * n_vars * 8;
    if (coef_bytes < need) return fail_size("dvs_cg_fit: coef_bytes < n_cells * n_vars * 8", need);
    CgFitArgs t = {};
    t.F = n_families;
    t.cells = n_cells;
    t.n = n_vars;
    t.nc = n_cont;
    t.card = card;
    t.var = var;
    t.parents = parents;
    t.table = table;
    t.offset = (const long long*)offset;
    t.coef = coef;
    t.intercept = intercept;
    t.sd = sd;
    t.count = count;
    t.status = status;
    call_begin();
    dvs_launch_cg_fit(t, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- a fitted conditional Gaussian network (dvs_mixed_params.h; include/dvs_mixed_params.h) ---------------------------------------
// what the entry points check first: n_rows, n_cells (2), n_vars, n_cont (3)
static int cgbn_dims(const char* fn, int n_vars, int n_cont, int64_t n_rows, int64_t n_cells) {
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return failf(2, "%s: n_rows must be in [1, 2^31 - 1]", fn);
    if (n_cells < 1 || n_cells * (n_vars > 0 ? n_vars : 1) > (int64_t)0x7fffffff || n_cells > (int64_t)0x7fffffff)
        return failf(2, "%s: n_cells must be >= 1 and n_cells * n_vars < 2^31", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (n_cont < 1 || n_cont > n_vars) return failf(3, "%s: n_cont must be in [1, n_vars]", fn);
    return 0;
}
static void cgbn_fill(CgbnRowArgs& a, int n_vars, int n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card, const uint64_t* parents,
                      const int64_t* offset, const double* coef, const double* intercept, const double* sd, const uint64_t* packed,
                      void* workspace, int32_t* status) {
    a.net.n = n_vars;
    a.net.nc = n_cont;
    a.net.cells = n_cells;
    a.net.card = card;
    a.net.parents = parents;
    a.net.offset = (const long long*)offset;
    a.net.coef = coef;
    a.net.intercept = intercept;
    a.net.sd = sd;
    a.net.status = status;
    a.rows = n_rows;
    a.chunks = (int)((n_rows + 255) / 256);
    a.target = -1;
    a.packed = packed;
    a.header = (int*)workspace;
}

extern "C" size_t dvs_cgbn_sample_workspace_bytes(int32_t n_vars) {
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", "dvs_cgbn_sample_workspace_bytes"), 0;
    return DVS_CGBN_HEADER;
}

extern "C" int dvs_cgbn_sample(int32_t n_vars, int32_t n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card,
                               const uint64_t* parents, const int64_t* offset, const double* coef, const double* intercept,
                               const double* sd, const uint64_t* packed, uint64_t seed, int64_t row_offset, void* workspace,
                               size_t workspace_bytes, double* x_out, int32_t* status, void* stream) {
    const char* fn = "dvs_cgbn_sample";
    if (int e = cgbn_dims(fn, n_vars, n_cont, n_rows, n_cells)) return e;
    if (row_offset < 0) return failf(12, "%s: row_offset must be >= 0", fn);
    if (!card || !parents || !offset || !coef || !intercept || !sd || !packed || !workspace || !x_out || !status)
        return failf(10, "%s: null pointer", fn);
    if (workspace_bytes < DVS_CGBN_HEADER) return fail_size("dvs_cgbn_sample: workspace_bytes < dvs_cgbn_sample_workspace_bytes", DVS_CGBN_HEADER);
    CgbnRowArgs a = {};
    cgbn_fill(a, n_vars, n_cont, n_rows, n_cells, card, parents, offset, coef, intercept, sd, packed, workspace, status);
    a.row_offset = (uint32_t)row_offset;
    a.per_row = x_out;
    call_begin();
    dvs_launch_cgbn_sample(a, seed, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" size_t dvs_cgbn_loglik_workspace_bytes(int32_t n_vars, int64_t n_rows, int64_t n_cells) {
    if (cgbn_dims("dvs_cgbn_loglik_workspace_bytes", n_vars, 1, n_rows, n_cells)) return 0;
    return dvs_cgbn_loglik_c_offset(n_rows) + (size_t)n_cells * 8;
}

extern "C" int dvs_cgbn_loglik(int32_t n_vars, int32_t n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card,
                               const uint64_t* parents, const int64_t* offset, const double* coef, const double* intercept,
                               const double* sd, const uint64_t* packed, const double* x, double* per_row, double* out,
                               void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_cgbn_loglik";
    if (int e = cgbn_dims(fn, n_vars, n_cont, n_rows, n_cells)) return e;
    if (!card || !parents || !offset || !coef || !intercept || !sd || !packed || !x || !out || !workspace || !status)
        return failf(10, "%s: null pointer", fn);
    const size_t c_at = dvs_cgbn_loglik_c_offset(n_rows), need = c_at + (size_t)n_cells * 8;
    if (workspace_bytes < need) return fail_size("dvs_cgbn_loglik: workspace_bytes < dvs_cgbn_loglik_workspace_bytes", need);
    CgbnRowArgs a = {};
    cgbn_fill(a, n_vars, n_cont, n_rows, n_cells, card, parents, offset, coef, intercept, sd, packed, workspace, status);
    a.x = x;
    a.per_row = per_row;
    a.out = out;
    a.partials = (double*)((char*)workspace + DVS_CGBN_HEADER);
    a.c = (double*)((char*)workspace + c_at);
    call_begin();
    dvs_launch_cgbn_loglik(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" size_t dvs_cgbn_predict_workspace_bytes(int32_t n_vars, int64_t n_cells) {
    if (cgbn_dims("dvs_cgbn_predict_workspace_bytes", n_vars, 1, 1, n_cells)) return 0;
    return DVS_CGBN_HEADER + (size_t)n_cells * 8;
}

extern "C" int dvs_cgbn_predict(int32_t n_vars, int32_t n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card,
                                const uint64_t* parents, const int64_t* offset, const double* coef, const double* intercept,
                                const double* sd, const uint64_t* packed, const double* x, int32_t target, int32_t mode,
                                const double* prior, void* pred, double* var, double* posterior, void* workspace,
                                size_t workspace_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_cgbn_predict";
    if (int e = cgbn_dims(fn, n_vars, n_cont, n_rows, n_cells)) return e;
    if (mode < DVS_CGBN_PREDICT_PARENTS || mode > DVS_CGBN_PREDICT_CLASS)
        return failf(12, "%s: mode must be 0 (parents), 1 (exact) or 2 (class)", fn);
    if (target < 0 || target >= n_vars) return failf(13, "%s: target must be in [0, n_vars)", fn);
    if (!card || !parents || !offset || !coef || !intercept || !sd || !packed || !x || !pred || !workspace || !status ||
        (mode != DVS_CGBN_PREDICT_CLASS && !var))
        return failf(10, "%s: null pointer", fn);
    const size_t need = DVS_CGBN_HEADER + (size_t)n_cells * 8;
    if (workspace_bytes < need) return fail_size("dvs_cgbn_predict: workspace_bytes < dvs_cgbn_predict_workspace_bytes", need);
    CgbnRowArgs a = {};
    cgbn_fill(a, n_vars, n_cont, n_rows, n_cells, card, parents, offset, coef, intercept, sd, packed, workspace, status);
    a.x = x;
    a.target = target;
    a.mode = mode;
    a.prior = prior;
    a.per_row = (double*)pred;
    a.label = (uint8_t*)pred;
    a.out = var;
    a.posterior = posterior;
    a.c = (double*)((char*)workspace + DVS_CGBN_HEADER);
    call_begin();
    dvs_launch_cgbn_predict(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- Gaussian CI tests (dvs_gaussian_ci.h; include/dvs_gaussian_ci.h) -----------------------------------------------------------
// what the two entry points check first: counts (2), n_vars (3), the range of the cell index (2), test_type (12)
static int gci_dims(const char* fn, const char* count, const char* cells_text, int items, int n_vars, int n_sets, bool per_var, int test_type) {
    if (items <= 0 || n_sets <= 0) return failf(2, "%s: %s and n_sets must be > 0", fn, count);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if ((int64_t)items * (per_var ? n_vars : 1) * 3 > (int64_t)0x7fffffff) return failf(2, "%s: %s must be < 2^31", fn, cells_text);
    if (test_type < DVS_GCI_COR || test_type > DVS_GCI_MI_G) return failf(12, "%s: test_type is not a dvs_gci_type", fn);
    return 0;
}

extern "C" int dvs_gbn_ci_tests(int32_t n_tests, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                                const int32_t* pairs, const uint64_t* cond, int32_t test_type, double* out, size_t out_bytes,
                                int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_ci_tests";
    if (int e = gci_dims(fn, "n_tests", "n_tests * 3", n_tests, n_vars, n_sets, false, test_type)) return e;
    if (!moments || !pairs || !cond || !out || !status) return failf(10, "%s: null pointer", fn);
    if (out_bytes < (size_t)n_tests * 24) return fail_size("dvs_gbn_ci_tests: out_bytes < n_tests * 24", (size_t)n_tests * 24);
    GbnCiArgs a = {};
    a.T = n_tests;
    a.n = n_vars;
    a.type = test_type;
    a.moments = moments;
    a.set_of = set_of;
    a.pairs = pairs;
    a.cond = cond;
    a.out = out;
    a.status = status;
    call_begin();
    dvs_launch_gbn_ci(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_gbn_ci_tests_group(int32_t n_groups, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                                      const int32_t* target, const uint64_t* cond, const uint64_t* candidates, int32_t test_type,
                                      double* out, size_t out_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_ci_tests_group";
    if (int e = gci_dims(fn, "n_groups", "n_groups * n_vars * 3", n_groups, n_vars, n_sets, true, test_type))
        return e;
    if (!moments || !target || !cond || !candidates || !out || !status) return failf(10, "%s: null pointer", fn);
    const size_t need = (size_t)n_groups * n_vars * 24;
    if (out_bytes < need) return fail_size("dvs_gbn_ci_tests_group: out_bytes < n_groups * n_vars * 24", need);
    GbnCiGroupArgs a = {};
    a.G = n_groups;
    a.n = n_vars;
    a.type = test_type;
    a.moments = moments;
    a.set_of = set_of;
    a.target = target;
    a.cond = cond;
    a.candidates = candidates;
    a.out = out;
    a.status = status;
    call_begin();
    dvs_launch_gbn_ci_group(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- a fitted Gaussian network (dvs_gaussian_params.h; include/dvs_gaussian_params.h) -------------------------------------------
static void gpar_net(GbnNet& net, int batch, int n_vars, const uint64_t* parents, const double* coef, const double* intercept,
                     const double* sd, int32_t* status) {
    net.B = batch;
    net.n = n_vars;
    net.parents = parents;
    net.coef = coef;
    net.intercept = intercept;
    net.sd = sd;
    net.status = status;
}

extern "C" int dvs_gbn_joint(int32_t batch, int32_t n_vars, const uint64_t* parents, const double* coef, const double* intercept,
                             const double* sd, double* mean, double* cov, size_t cov_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_joint";
    if (batch <= 0) return failf(2, "%s: batch must be > 0", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if ((int64_t)batch * n_vars * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: batch * n_vars^2 must be < 2^31", fn);
    if (!parents || !coef || !intercept || !sd || !mean || !cov || !status) return failf(10, "%s: null pointer", fn);
    const size_t need = (size_t)batch * n_vars * n_vars * 8;
    if (cov_bytes < need) return fail_size("dvs_gbn_joint: cov_bytes < batch * n_vars^2 * 8", need);
    GbnJointArgs a = {};
    gpar_net(a.net, batch, n_vars, parents, coef, intercept, sd, status);
    a.mean = mean;
    a.cov = cov;
    call_begin();
    dvs_launch_gbn_joint(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_gbn_quantiles(int64_t count, const uint64_t* k, double* z, void* stream) {
    const char* fn = "dvs_gbn_quantiles";
    if (count < 1 || count > (int64_t)0x7fffffff) return failf(2, "%s: count must be in [1, 2^31 - 1]", fn);
    if (!k || !z) return failf(10, "%s: null pointer", fn);
    GbnQuantileArgs a = {};
    a.count = count;
    a.k = k;
    a.z = z;
    call_begin();
    dvs_launch_gbn_quantiles(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" size_t dvs_gbn_sample_workspace_bytes(int32_t n_vars) {
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", "dvs_gbn_sample_workspace_bytes"), 0;
    return DVS_GBN_SAMPLE_WORKSPACE;
}

extern "C" int dvs_gbn_sample(int32_t n_vars, int64_t n_rows, const uint64_t* parents, const double* coef, const double* intercept,
                              const double* sd, uint64_t seed, int64_t row_offset, void* workspace, size_t workspace_bytes,
                              double* data_out, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_sample";
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return failf(2, "%s: n_rows must be in [1, 2^31 - 1]", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (row_offset < 0) return failf(12, "%s: row_offset must be >= 0", fn);
    if (!parents || !coef || !intercept || !sd || !workspace || !data_out || !status) return failf(10, "%s: null pointer", fn);
    if (workspace_bytes < DVS_GBN_SAMPLE_WORKSPACE)
        return fail_size("dvs_gbn_sample: workspace_bytes < dvs_gbn_sample_workspace_bytes", DVS_GBN_SAMPLE_WORKSPACE);
    GbnSampleArgs a = {};
    gpar_net(a.net, 1, n_vars, parents, coef, intercept, sd, status);
    a.rows = n_rows;
    a.row_offset = (uint32_t)row_offset;
    a.header = (int*)workspace;
    a.out = data_out;
    call_begin();
    dvs_launch_gbn_sample(a, seed, (dvs_stream_t)stream);
    return call_end(fn);
}

// what dvs_gbn_loglik and dvs_gbn_predict check first: batch, n_rows (2), n_vars (3), the index ranges (2)
static int gpar_row_dims(const char* fn, int batch, int n_vars, int64_t n_rows) {
    if (batch <= 0) return failf(2, "%s: batch must be > 0", fn);
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return failf(2, "%s: n_rows must be in [1, 2^31 - 1]", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if ((int64_t)batch * n_vars > (int64_t)0x7fffffff || (int64_t)batch * ((n_rows + 255) / 256) > (int64_t)0x7fffffff)
        return failf(2, "%s: batch * n_vars and batch * ceil(n_rows / 256) must be < 2^31", fn);
    return 0;
}

extern "C" int dvs_gbn_loglik(int32_t batch, int32_t n_vars, int64_t n_rows, const double* data, const uint64_t* parents,
                              const double* coef, const double* intercept, const double* sd, double* per_row, double* out,
                              void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_loglik";
    if (int e = gpar_row_dims(fn, batch, n_vars, n_rows)) return e;
    if (!data || !parents || !coef || !intercept || !sd || !out || !workspace || !status) return failf(10, "%s: null pointer", fn);
    const BnLoglikLayout l = dvs_bn_loglik_layout(batch, n_vars, n_rows);
    const size_t need = l.logs + (size_t)batch * n_vars * 8;
    if (workspace_bytes < need) return fail_size("dvs_gbn_loglik: workspace_bytes < partials + flags + batch * n_vars * 8", need);
    GbnRowArgs a = {};
    gpar_net(a.net, batch, n_vars, parents, coef, intercept, sd, status);
    a.chunks = (int)l.chunks;
    a.rows = n_rows;
    a.data = data;
    a.per_row = per_row;
    a.out = out;
    a.partials = (double*)((char*)workspace + l.partials);
    a.ok = (int*)((char*)workspace + l.fam_ok);
    a.c = (double*)((char*)workspace + l.logs);
    call_begin();
    dvs_launch_gbn_loglik(a, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_gbn_predict(int32_t batch, int32_t n_vars, int64_t n_rows, const double* data, const uint64_t* parents,
                               const double* coef, const double* intercept, const double* sd, int32_t target, int32_t mode,
                               double* pred, double* var, void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_predict";
    if (int e = gpar_row_dims(fn, batch, n_vars, n_rows)) return e;
    if (target < 0 || target >= n_vars) return failf(13, "%s: target must be in [0, n_vars)", fn);
    if (mode != DVS_GBN_PREDICT_PARENTS && mode != DVS_GBN_PREDICT_EXACT) return failf(12, "%s: mode must be 0 (parents) or 1 (exact)", fn);
    if (!data || !parents || !coef || !intercept || !sd || !pred || !var || !workspace || !status) return failf(10, "%s: null pointer", fn);
    const size_t need = ((size_t)batch * 4 + 255) & ~(size_t)255;
    if (workspace_bytes < need) return fail_size("dvs_gbn_predict: workspace_bytes < batch * 4 rounded up to 256", need);
    GbnRowArgs a = {};
    gpar_net(a.net, batch, n_vars, parents, coef, intercept, sd, status);
    a.chunks = (int)((n_rows + 255) / 256);
    a.target = target;
    a.mode = mode;
    a.rows = n_rows;
    a.data = data;
    a.per_row = pred;
    a.out = var;
    a.ok = (int*)workspace;
    call_begin();
    dvs_launch_gbn_predict(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- a normal conditioned on every row's observed part (dvs_gaussian_incomplete.h; include/dvs_gaussian_incomplete.h) -----------
extern "C" size_t dvs_gbn_condition_workspace_bytes(int32_t n_vars, int64_t n_rows) {
    const char* fn = "dvs_gbn_condition_workspace_bytes";
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return failf(2, "%s: n_rows must be in [1, 2^31 - 1]", fn), 0;
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn), 0;
    return dvs_gbn_condition_layout(n_vars, n_rows).total;
}

extern "C" int dvs_gbn_condition(int32_t n_vars, int64_t n_rows, const double* mean, const double* cov, const double* x,
                                 const uint64_t* observed, const int32_t* order, double* completed, double* cvar, double* quad,
                                 double* logp, double* loglik, double* ccov, int64_t* counts, void* workspace,
                                 size_t workspace_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_gbn_condition";
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return failf(2, "%s: n_rows must be in [1, 2^31 - 1]", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (!mean || !cov || !x || !observed || !logp || !loglik || !workspace || !status) return failf(10, "%s: null pointer", fn);
    const GbnConditionLayout l = dvs_gbn_condition_layout(n_vars, n_rows);
    if (workspace_bytes < l.total) return fail_size("dvs_gbn_condition: workspace_bytes < dvs_gbn_condition_workspace_bytes", l.total);
    GbnConditionArgs a = {};
    a.n = n_vars;
    a.chunks = (int)l.chunks;
    a.rows = n_rows;
    a.mean = mean;
    a.cov = cov;
    a.x = x;
    a.observed = observed;
    a.order = order;
    a.completed = completed;
    a.cvar = cvar;
    a.quad = quad;
    a.logp = logp;
    a.loglik = loglik;
    a.ccov = ccov;
    a.counts = (long long*)counts;
    a.partials = (double*)((char*)workspace + l.partials);
    a.refused = (int*)((char*)workspace + l.refused);
    a.cov_partials = (double*)((char*)workspace + l.cov);
    a.status = status;
    call_begin();
    dvs_launch_gbn_condition(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// What dvs_pc_expand and dvs_pc_reduce check alike, first: the pair count, n_vars and the level's test count.
static int pc_dims(const char* fn, int n_pairs, int n_vars, int64_t n_tests) {
    if (n_pairs < 1 || n_pairs > DVS_WTOK * (DVS_WTOK - 1) / 2) return failf(2, "%s: n_pairs must be in [1, 1128]", fn);
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (n_tests < 1 || n_tests > (int64_t)0x7fffffff) return failf(2, "%s: n_tests must be in [1, 2^31 - 1]", fn);
    return 0;
}

extern "C" int dvs_pc_expand(int32_t n_pairs, int32_t n_vars, int32_t level, const uint64_t* adj, const int32_t* pair_xy,
                             const int64_t* offsets, int64_t n_tests, int32_t* pairs, uint64_t* cond, size_t tests_bytes,
                             void* stream) {
    if (int e = pc_dims("dvs_pc_expand", n_pairs, n_vars, n_tests)) return e;
    if (level < 0 || level > DVS_WTOK - 2) return fail(13, "dvs_pc_expand: level must be in [0, 46]");
    if (!adj || !pair_xy || !offsets || !pairs || !cond) return fail(10, "dvs_pc_expand: null pointer");
    if (tests_bytes < (size_t)n_tests * 8) return fail_size("dvs_pc_expand: tests_bytes < n_tests * 8", (size_t)n_tests * 8);
    PcExpandArgs a = {};
    a.P = n_pairs;
    a.n = n_vars;
    a.level = level;
    a.T = n_tests;
    a.adj = adj;
    a.pair_xy = pair_xy;
    a.offsets = (const long long*)offsets;
    a.pairs = pairs;
    a.cond = cond;
    call_begin();
    dvs_launch_pc_expand(a, (dvs_stream_t)stream);
    return call_end("dvs_pc_expand");
}

extern "C" int dvs_pc_reduce(int32_t n_pairs, int32_t n_vars, const int32_t* pair_xy, const int64_t* offsets, int64_t n_tests,
                             const uint64_t* cond, const double* out, double alpha, const uint64_t* adj, uint64_t* adj_next,
                             uint64_t* sepset, size_t sepset_bytes, int64_t* result, size_t result_bytes, int32_t* refused,
                             void* stream) {
    if (int e = pc_dims("dvs_pc_reduce", n_pairs, n_vars, n_tests)) return e;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(13, "dvs_pc_reduce: alpha must be in [0, 1]");
    if (!pair_xy || !offsets || !cond || !out || !adj || !adj_next || !sepset || !result || !refused)
        return fail(10, "dvs_pc_reduce: null pointer");
    if (sepset_bytes < (size_t)n_vars * n_vars * 8)
        return fail_size("dvs_pc_reduce: sepset_bytes < n_vars^2 * 8", (size_t)n_vars * n_vars * 8);
    if (result_bytes < (size_t)n_pairs * 16) return fail_size("dvs_pc_reduce: result_bytes < n_pairs * 16", (size_t)n_pairs * 16);
    PcReduceArgs a = {};
    a.P = n_pairs;
    a.n = n_vars;
    a.T = n_tests;
    a.alpha = alpha;
    a.pair_xy = pair_xy;
    a.offsets = (const long long*)offsets;
    a.cond = cond;
    a.out = out;
    a.adj = adj;
    a.adj_next = adj_next;
    a.sepset = sepset;
    a.result = (long long*)result;
    a.refused = refused;
    call_begin();
    dvs_launch_pc_reduce(a, (dvs_stream_t)stream);
    return call_end("dvs_pc_reduce");
}

extern "C" int dvs_pc_orient(int32_t batch, int32_t n_vars, const uint64_t* skeleton, const uint64_t* sepsets,
                             size_t sepsets_bytes, uint64_t* pdag, size_t pdag_bytes, int32_t* conflicts, int32_t* flags,
                             void* stream) {
    if (batch <= 0) return fail(2, "dvs_pc_orient: batch must be > 0");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_pc_orient: n_vars must be in [1, 48]");
    if ((int64_t)batch * n_vars * n_vars > (int64_t)0x7fffffff) return fail(2, "dvs_pc_orient: batch * n_vars^2 must be < 2^31");
    if (!skeleton || !sepsets || !pdag || !conflicts || !flags) return fail(10, "dvs_pc_orient: null pointer");
    const size_t rows = (size_t)batch * n_vars * 8;
    if (sepsets_bytes < rows * n_vars) return fail_size("dvs_pc_orient: sepsets_bytes < batch * n_vars^2 * 8", rows * n_vars);
    if (pdag_bytes < rows) return fail_size("dvs_pc_orient: pdag_bytes < batch * n_vars * 8", rows);
    PcOrientArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.skeleton = skeleton;
    a.sepsets = sepsets;
    a.pdag = pdag;
    a.conflicts = conflicts;
    a.flags = flags;
    call_begin();
    dvs_launch_pc_orient(a, (dvs_stream_t)stream);
    return call_end("dvs_pc_orient");
}

// ---- BN parameters: fit, forward sampling, held-out log-likelihood (dvs_params.h) -------------------------------------
extern "C" int dvs_bn_fit(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                          const uint64_t* parents, int32_t method, double iss, int32_t unobserved, const int64_t* offsets,
                          double* cpt, size_t cpt_bytes, int32_t* status, void* stream) {
    if (batch <= 0 || n_samples <= 0) return fail(2, "dvs_bn_fit: batch and n_samples must be > 0");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_bn_fit: n_vars must be in [1, 48]");
    if ((int64_t)batch * n_vars > (int64_t)0x7fffffff) return fail(2, "dvs_bn_fit: batch * n_vars must be < 2^31");
    if (method != DVS_FIT_MLE && method != DVS_FIT_BAYES) return fail(12, "dvs_bn_fit: method is not a dvs_fit_method");
    if (method == DVS_FIT_BAYES && !(iss > 0.0 && isfinite(iss))) return fail(13, "dvs_bn_fit: iss must be finite and > 0");
    if (unobserved != 0 && unobserved != 1) return fail(12, "dvs_bn_fit: unobserved must be 0 (NaN) or 1 (uniform)");
    if (!data || !card || !parents || !offsets || !cpt || !status) return fail(10, "dvs_bn_fit: null pointer");
    const size_t need = (size_t)batch * n_vars * 8;          // every family has a cell; the slots themselves are on the device
    if (cpt_bytes < need) return fail_size("dvs_bn_fit: cpt_bytes < batch * n_vars * 8", need);
    BnFitArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.S = n_samples;
    a.method = method;
    a.unobserved = unobserved;
    a.iss = iss;
    a.data = data;
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.cpt = cpt;
    a.cpt_cells = (long long)(cpt_bytes / 8);
    a.status = status;
    call_begin();
    dvs_launch_bn_fit(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_fit");
}

static int bn_sample_dims(const char* fn, int64_t n_cells, int n_vars) {
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if (n_cells < n_vars || n_cells > (int64_t)0x7fffffff) return failf(2, "%s: n_cells must be in [n_vars, 2^31 - 1]", fn);
    return 0;
}

extern "C" size_t dvs_bn_sample_workspace_bytes(int64_t n_cells, int32_t n_vars) {
    if (bn_sample_dims("dvs_bn_sample_workspace_bytes", n_cells, n_vars)) return 0;
    return dvs_bn_sample_layout(n_cells).total;
}

extern "C" int dvs_bn_sample(int32_t n_vars, int64_t n_rows, const uint8_t* card, const uint64_t* parents, const int64_t* offsets,
                             const double* cpt, int64_t n_cells, uint64_t seed, int64_t row_offset, void* workspace,
                             size_t workspace_bytes, uint64_t* data_out, int32_t* status, void* stream) {
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return fail(2, "dvs_bn_sample: n_rows must be in [1, 2^31 - 1]");
    if (int e = bn_sample_dims("dvs_bn_sample", n_cells, n_vars)) return e;
    if (row_offset < 0) return fail(12, "dvs_bn_sample: row_offset must be >= 0");
    if (!card || !parents || !offsets || !cpt || !workspace || !data_out || !status) return fail(10, "dvs_bn_sample: null pointer");
    const BnSampleLayout l = dvs_bn_sample_layout(n_cells);
    if (workspace_bytes < l.total) return fail_size("dvs_bn_sample: workspace_bytes < dvs_bn_sample_workspace_bytes", l.total);
    BnSampleArgs a = {};
    a.n = n_vars;
    a.rows = n_rows;
    a.n_cells = n_cells;
    a.row_offset = (uint32_t)row_offset;
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.cpt = cpt;
    a.header = (int*)((char*)workspace + l.order);
    a.thr = (uint32_t*)((char*)workspace + l.thr);
    a.out = data_out;
    a.status = status;
    call_begin();
    dvs_launch_bn_sample(a, seed, (dvs_stream_t)stream);
    return call_end("dvs_bn_sample");
}

extern "C" int dvs_bn_loglik(int32_t batch, int32_t n_vars, int64_t n_rows, const uint64_t* data, const uint8_t* card,
                             const uint64_t* parents, const int64_t* offsets, const double* cpt, double* per_row, double* out,
                             void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    if (batch <= 0) return fail(2, "dvs_bn_loglik: batch must be > 0");
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return fail(2, "dvs_bn_loglik: n_rows must be in [1, 2^31 - 1]");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_bn_loglik: n_vars must be in [1, 48]");
    const int64_t chunks = (n_rows + 255) / 256;
    if ((int64_t)batch * n_vars > (int64_t)0x7fffffff || (int64_t)batch * chunks > (int64_t)0x7fffffff)
        return fail(2, "dvs_bn_loglik: batch * n_vars and batch * ceil(n_rows / 256) must be < 2^31");
    if (!data || !card || !parents || !offsets || !cpt || !out || !workspace || !status)
        return fail(10, "dvs_bn_loglik: null pointer");
    const BnLoglikLayout l = dvs_bn_loglik_layout(batch, n_vars, n_rows);
    const size_t need = l.logs + (size_t)batch * n_vars * 8;
    if (workspace_bytes < need) return fail_size("dvs_bn_loglik: workspace_bytes < partials + flags + batch * n_vars * 8", need);
    BnLoglikArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.chunks = (int)chunks;
    a.rows = n_rows;
    const size_t room = (workspace_bytes - l.logs) / 8;
    a.log_cells = room > (size_t)0x7fffffff ? 0x7fffffffLL : (long long)room;
    a.data = data;
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.cpt = cpt;
    a.per_row = per_row;
    a.out = out;
    a.partials = (double*)((char*)workspace + l.partials);
    a.fam_ok = (int*)((char*)workspace + l.fam_ok);
    a.logs = (double*)((char*)workspace + l.logs);
    a.status = status;
    call_begin();
    dvs_launch_bn_loglik(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_loglik");
}

// ---- inference on a fitted network: likelihood weighting, exact blanket posterior (dvs_infer.h) ------------------------
static int bn_lw_dims(const char* fn, int64_t n_cells, int n_vars, int64_t n_queries, int64_t n_particles, uint64_t targets) {
    if (n_queries < 1 || n_queries > (int64_t)0x7fffffff || n_particles < 1 || n_particles > (int64_t)0x7fffffff)
        return failf(2, "%s: n_queries and n_particles must be in [1, 2^31 - 1]", fn);
    if (int e = bn_sample_dims(fn, n_cells, n_vars)) return e;
    if (n_queries * ((n_particles + 255) / 256) > (int64_t)0x7fffffff)
        return failf(2, "%s: n_queries * ceil(n_particles / 256) must be < 2^31", fn);
    if (targets >> n_vars) return failf(12, "%s: targets has a bit at or above n_vars", fn);
    return 0;
}

extern "C" size_t dvs_bn_lw_workspace_bytes(int64_t n_cells, int32_t n_vars, int64_t n_queries, int64_t n_particles,
                                            uint64_t targets) {
    if (bn_lw_dims("dvs_bn_lw_workspace_bytes", n_cells, n_vars, n_queries, n_particles, targets)) return 0;
    return dvs_bn_lw_layout(n_cells, n_queries, n_particles, targets).total;
}

extern "C" int dvs_bn_lw(int32_t n_vars, int64_t n_queries, int64_t n_particles, const uint8_t* card, const uint64_t* parents,
                         const int64_t* offsets, const double* cpt, int64_t n_cells, const uint64_t* evidence,
                         const uint64_t* observed, const uint16_t* event, uint64_t targets, uint64_t seed, int64_t query_offset,
                         void* workspace, size_t workspace_bytes, double* sums, double* marginals, uint64_t* particles,
                         double* particle_weights, int32_t* status, void* stream) {
    if (int e = bn_lw_dims("dvs_bn_lw", n_cells, n_vars, n_queries, n_particles, targets)) return e;
    if (query_offset < 0) return fail(12, "dvs_bn_lw: query_offset must be >= 0");
    if (!card || !parents || !offsets || !cpt || !evidence || !observed || !workspace || !sums || !status)
        return fail(10, "dvs_bn_lw: null pointer");
    if ((targets != 0) != (marginals != nullptr)) return fail(12, "dvs_bn_lw: marginals goes with targets != 0, and only with it");
    if ((particles != nullptr) != (particle_weights != nullptr))
        return fail(12, "dvs_bn_lw: particles and particle_weights are both null or both given");
    const BnLwLayout l = dvs_bn_lw_layout(n_cells, n_queries, n_particles, targets);
    if (workspace_bytes < l.total) return fail_size("dvs_bn_lw: workspace_bytes < dvs_bn_lw_workspace_bytes", l.total);
    BnLwArgs a = {};
    a.n = n_vars;
    a.Q = (int)n_queries;
    static const int cus = dvs_device_cus();
    a.cus = cus;
    a.chunks = (int)l.chunks;
    a.M = n_particles;
    a.n_cells = n_cells;
    a.query_offset = (uint32_t)query_offset;
    a.targets = targets;
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.cpt = cpt;
    a.evidence = evidence;
    a.observed = observed;
    a.event = event;
    a.header = (int*)((char*)workspace + l.order);
    a.thr = (uint32_t*)((char*)workspace + l.thr);
    a.qbad = (int*)((char*)workspace + l.qbad);
    a.partials = (double*)((char*)workspace + l.partials);
    a.sums = sums;
    a.marginals = marginals;
    a.particles = particles;
    a.pweights = particle_weights;
    a.status = status;
    call_begin();
    dvs_launch_bn_lw(a, seed, (dvs_stream_t)stream);
    return call_end("dvs_bn_lw");
}

extern "C" int dvs_bn_blanket_posterior(int32_t batch, int32_t n_vars, int64_t n_rows, const uint64_t* data, const uint8_t* card,
                                        const uint64_t* parents, const int64_t* offsets, const double* cpt, size_t cpt_bytes,
                                        int32_t target, int32_t use_children, double* posterior, uint8_t* pred, int32_t* status,
                                        void* stream) {
    if (batch <= 0) return fail(2, "dvs_bn_blanket_posterior: batch must be > 0");
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return fail(2, "dvs_bn_blanket_posterior: n_rows must be in [1, 2^31 - 1]");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_bn_blanket_posterior: n_vars must be in [1, 48]");
    const int64_t chunks = (n_rows + 255) / 256;
    if ((int64_t)batch * n_vars > (int64_t)0x7fffffff || (int64_t)batch * chunks > (int64_t)0x7fffffff)
        return fail(2, "dvs_bn_blanket_posterior: batch * n_vars and batch * ceil(n_rows / 256) must be < 2^31");
    if (target < 0 || target >= n_vars) return fail(12, "dvs_bn_blanket_posterior: target must be in [0, n_vars)");
    if (use_children != 0 && use_children != 1) return fail(12, "dvs_bn_blanket_posterior: use_children must be 0 or 1");
    if (!data || !card || !parents || !offsets || !cpt || !pred || !status)
        return fail(10, "dvs_bn_blanket_posterior: null pointer");
    const size_t need = (size_t)batch * n_vars * 8;          // every family has a cell; the slots themselves are on the device
    if (cpt_bytes < need) return fail_size("dvs_bn_blanket_posterior: cpt_bytes < batch * n_vars * 8", need);
    BnBlanketArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.chunks = (int)chunks;
    a.target = target;
    a.use_children = use_children;
    a.rows = n_rows;
    a.cpt_cells = (long long)(cpt_bytes / 8);
    a.data = data;
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.cpt = cpt;
    a.posterior = posterior;
    a.pred = pred;
    a.status = status;
    call_begin();
    dvs_launch_bn_blanket(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_blanket_posterior");
}

// ---- exact inference by variable elimination (dvs_eliminate.h) ---------------------------------------------------------
extern "C" int dvs_bn_eliminate(int32_t n_vars, int32_t n_plans, int64_t n_rows, const uint8_t* card, const uint64_t* parents,
                                const int64_t* offsets, const double* cpt, int64_t n_cells, const int32_t* plans,
                                size_t plans_bytes, const int64_t* plan_offsets, int32_t plan_words, int32_t arena_cells,
                                int32_t step_cells, const uint16_t* masks, int32_t rows_per_group, int32_t out_stride,
                                double* out, size_t out_bytes, double* z, int32_t* plan_flags, int32_t* status, void* stream) {
    if (int e = bn_sample_dims("dvs_bn_eliminate", n_cells, n_vars)) return e;
    if (n_plans < 1 || n_rows < 1 || n_rows > (int64_t)0x7fffffff || (int64_t)n_plans * n_rows > (int64_t)0x7fffffff)
        return fail(2, "dvs_bn_eliminate: n_plans and n_rows must be in [1, 2^31 - 1] and n_plans * n_rows < 2^31");
    if (plan_words < 7 || plan_words > DVS_BN_ELIM_MAX_WORDS)
        return fail(12, "dvs_bn_eliminate: plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]");
    if (arena_cells < 1 || arena_cells > DVS_BN_ELIM_MAX_CELLS || step_cells < 1 || step_cells > DVS_BN_ELIM_MAX_CELLS)
        return fail(12, "dvs_bn_eliminate: arena_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]");
    if (out_stride < 1 || out_stride > DVS_BN_ELIM_MAX_CELLS)
        return fail(12, "dvs_bn_eliminate: out_stride must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]");
    if (rows_per_group < 0 || rows_per_group > 64) return fail(12, "dvs_bn_eliminate: rows_per_group must be in [0, 64]");
    if (!card || !parents || !offsets || !cpt || !plans || !plan_offsets || !masks || !out || !z || !plan_flags || !status)
        return fail(10, "dvs_bn_eliminate: null pointer");
    if (plans_bytes < (size_t)n_plans * 28) return fail_size("dvs_bn_eliminate: plans_bytes < n_plans * 28", (size_t)n_plans * 28);
    const size_t need = (size_t)n_plans * (size_t)n_rows * (size_t)out_stride * 8;
    if (out_bytes < need) return fail_size("dvs_bn_eliminate: out_bytes < n_plans * n_rows * out_stride * 8", need);
    BnElimArgs a = {};
    a.n = n_vars;
    a.P = n_plans;
    a.plan_words = plan_words;
    a.arena_cells = arena_cells;
    a.step_cells = step_cells;
    a.rows_per_group = rows_per_group;
    a.out_stride = out_stride;
    a.rows = n_rows;
    a.n_cells = n_cells;
    a.plans_words = (long long)(plans_bytes / 4);
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.cpt = cpt;
    a.plans = plans;
    a.plan_offsets = (const long long*)plan_offsets;
    a.masks = masks;
    a.out = out;
    a.z = z;
    a.plan_flags = plan_flags;
    a.status = status;
    call_begin();
    dvs_launch_bn_eliminate(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_eliminate");
}

// ---- incomplete data: expected counts, tables from counts, exact imputation (dvs_incomplete.h) -------------------------
static int bn_inc_dims(const char* fn, int64_t n_cells, int n_vars, int64_t n_rows, bool counts) {
    if (int e = bn_sample_dims(fn, n_cells, n_vars)) return e;
    if (n_rows < 1 || n_rows > (int64_t)0x7fffffff) return failf(2, "%s: n_rows must be in [1, 2^31 - 1]", fn);
    if (counts && ((n_rows + 255) / 256) * n_cells >= ((int64_t)1 << 40))
        return failf(2, "%s: ceil(n_rows / 256) * n_cells must be < 2^40", fn);
    return 0;
}

// impute: out_cells is the 16 levels a variable can have, not an argument
static int bn_inc_plans(const char* fn, int plan_words, int arena_cells, int out_cells, int step_cells, int rows_per_group, bool impute) {
    if (plan_words < 7 || plan_words > DVS_BN_ELIM_MAX_WORDS)
        return failf(12, "%s: plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]", fn);
    if (arena_cells < 1 || arena_cells > DVS_BN_ELIM_MAX_CELLS || out_cells < 1 || out_cells > DVS_BN_ELIM_MAX_CELLS ||
        step_cells < 1 || step_cells > DVS_BN_ELIM_MAX_CELLS)
        return failf(12, "%s: arena_cells%s and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", fn, impute ? "" : ", out_cells");
    if (arena_cells + out_cells > DVS_BN_ELIM_MAX_CELLS)
        return impute ? failf(12, "%s: arena_cells + 16 = %d exceeds DVS_BN_ELIM_MAX_CELLS = 16384", fn, arena_cells + 16)
                      : failf(12, "%s: arena_cells + out_cells = %d exceeds DVS_BN_ELIM_MAX_CELLS = 16384", fn, arena_cells + out_cells);
    if (rows_per_group < 0 || rows_per_group > 64) return failf(12, "%s: rows_per_group must be in [0, 64]", fn);
    return 0;
}

extern "C" size_t dvs_bn_expected_counts_workspace_bytes(int64_t n_cells, int32_t n_vars, int64_t n_rows) {
    if (bn_inc_dims("dvs_bn_expected_counts_workspace_bytes", n_cells, n_vars, n_rows, true)) return 0;
    return dvs_bn_inc_layout(n_cells, n_vars, n_rows, false).total;
}

extern "C" size_t dvs_bn_impute_workspace_bytes(int32_t n_vars, int64_t n_rows) {
    // no n_cells here: n_vars stands in its place, the least value bn_inc_dims accepts, so only n_vars and n_rows are judged
    if (bn_inc_dims("dvs_bn_impute_workspace_bytes", n_vars, n_vars, n_rows, false)) return 0;
    return dvs_bn_inc_layout(0, n_vars, n_rows, true).total;
}

static void bn_inc_fill(BnIncArgs& a, int n_vars, int n_plans, int64_t n_rows, const uint8_t* card, const uint64_t* parents,
                        const int64_t* offsets, const double* cpt, int64_t n_cells, const int32_t* plans, size_t plans_bytes,
                        const int64_t* plan_offsets, int plan_words, int arena_cells, int out_cells, int step_cells,
                        int rows_per_group, int32_t* plan_flags, int32_t* status) {
    a.e.n = n_vars;
    a.e.P = n_plans;
    a.e.plan_words = plan_words;
    a.e.arena_cells = arena_cells;
    a.e.step_cells = step_cells;
    a.e.rows_per_group = rows_per_group;
    a.e.out_stride = out_cells;
    a.e.rows = n_rows;
    a.e.n_cells = n_cells;
    a.e.plans_words = (long long)(plans_bytes / 4);
    a.e.card = card;
    a.e.parents = parents;
    a.e.offsets = (const long long*)offsets;
    a.e.cpt = cpt;
    a.e.plans = plans;
    a.e.plan_offsets = (const long long*)plan_offsets;
    a.e.plan_flags = plan_flags;
    a.e.status = status;
    a.chunks = (int)((n_rows + 255) / 256);
}

extern "C" int dvs_bn_expected_counts(int32_t n_vars, int64_t n_rows, const uint8_t* card, const uint64_t* parents,
                                      const int64_t* offsets, const double* cpt, int64_t n_cells, const int32_t* plans,
                                      size_t plans_bytes, const int64_t* plan_offsets, int32_t plan_words, int32_t arena_cells,
                                      int32_t out_cells, int32_t step_cells, const uint64_t* data, const uint64_t* observed,
                                      int32_t rows_per_group, double* counts, double* row_z, double* loglik, int64_t* skipped,
                                      int32_t* plan_flags, void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_bn_expected_counts";
    if (int e = bn_inc_dims(fn, n_cells, n_vars, n_rows, true)) return e;
    if (int e = bn_inc_plans(fn, plan_words, arena_cells, out_cells, step_cells, rows_per_group, false)) return e;
    if (!card || !parents || !offsets || !cpt || !plans || !plan_offsets || !data || !observed || !counts || !row_z || !loglik ||
        !skipped || !plan_flags || !workspace || !status)
        return fail(10, "dvs_bn_expected_counts: null pointer");
    const size_t words = (size_t)(n_vars + 1) * 28;
    if (plans_bytes < words) return fail_size("dvs_bn_expected_counts: plans_bytes < (n_vars + 1) * 28", words);
    const BnIncLayout l = dvs_bn_inc_layout(n_cells, n_vars, n_rows, false);
    if (workspace_bytes < l.total)
        return fail_size("dvs_bn_expected_counts: workspace_bytes < dvs_bn_expected_counts_workspace_bytes", l.total);
    BnIncArgs a = {};
    bn_inc_fill(a, n_vars, n_vars + 1, n_rows, card, parents, offsets, cpt, n_cells, plans, plans_bytes, plan_offsets, plan_words,
                arena_cells, out_cells, step_cells, rows_per_group, plan_flags, status);
    a.data = data;
    a.observed = observed;
    a.counts = counts;
    a.row_z = row_z;
    a.loglik = loglik;
    a.skipped = (long long*)skipped;
    a.partials = (double*)((char*)workspace + l.partials);
    a.icounts = (int*)((char*)workspace + l.icounts);
    a.ll_partials = (double*)((char*)workspace + l.ll);
    a.skip_partials = (int*)((char*)workspace + l.skip);
    a.row_ok = (unsigned char*)workspace + l.row_ok;
    call_begin();
    dvs_launch_bn_expected_counts(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_expected_counts");
}

extern "C" int dvs_bn_fit_counts(int32_t n_vars, const uint8_t* card, const uint64_t* parents, const int64_t* offsets,
                                 const double* counts, int64_t n_cells, int32_t method, double iss, int32_t unobserved,
                                 double* cpt_out, int32_t* status, void* stream) {
    if (int e = bn_sample_dims("dvs_bn_fit_counts", n_cells, n_vars)) return e;
    if (method != DVS_FIT_MLE && method != DVS_FIT_BAYES) return fail(12, "dvs_bn_fit_counts: method is not a dvs_fit_method");
    if (method == DVS_FIT_BAYES && !(iss > 0.0 && isfinite(iss))) return fail(13, "dvs_bn_fit_counts: iss must be finite and > 0");
    if (unobserved != 0 && unobserved != 1) return fail(12, "dvs_bn_fit_counts: unobserved must be 0 (NaN) or 1 (uniform)");
    if (!card || !parents || !offsets || !counts || !cpt_out || !status) return fail(10, "dvs_bn_fit_counts: null pointer");
    BnFitCountsArgs a = {};
    a.n = n_vars;
    a.method = method;
    a.unobserved = unobserved;
    a.n_cells = n_cells;
    a.iss = iss;
    a.card = card;
    a.parents = parents;
    a.offsets = (const long long*)offsets;
    a.counts = counts;
    a.cpt = cpt_out;
    a.status = status;
    call_begin();
    dvs_launch_bn_fit_counts(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_fit_counts");
}

extern "C" int dvs_bn_impute(int32_t n_vars, int64_t n_rows, const uint8_t* card, const uint64_t* parents, const int64_t* offsets,
                             const double* cpt, int64_t n_cells, const int32_t* plans, size_t plans_bytes,
                             const int64_t* plan_offsets, int32_t plan_words, int32_t arena_cells, int32_t step_cells,
                             const uint64_t* data, const uint64_t* observed, int32_t rows_per_group, uint64_t* data_out,
                             uint64_t* observed_out, int32_t* plan_flags, void* workspace, size_t workspace_bytes, int32_t* status,
                             void* stream) {
    const char* fn = "dvs_bn_impute";
    if (int e = bn_inc_dims(fn, n_cells, n_vars, n_rows, false)) return e;
    if (int e = bn_inc_plans(fn, plan_words, arena_cells, 16, step_cells, rows_per_group, true)) return e;
    if (!card || !parents || !offsets || !cpt || !plans || !plan_offsets || !data || !observed || !data_out || !observed_out ||
        !plan_flags || !workspace || !status)
        return fail(10, "dvs_bn_impute: null pointer");
    const size_t words = (size_t)n_vars * 28;
    if (plans_bytes < words) return fail_size("dvs_bn_impute: plans_bytes < n_vars * 28", words);
    const BnIncLayout l = dvs_bn_inc_layout(0, n_vars, n_rows, true);
    if (workspace_bytes < l.total) return fail_size("dvs_bn_impute: workspace_bytes < dvs_bn_impute_workspace_bytes", l.total);
    BnIncArgs a = {};
    bn_inc_fill(a, n_vars, n_vars, n_rows, card, parents, offsets, cpt, n_cells, plans, plans_bytes, plan_offsets, plan_words,
                arena_cells, 16, step_cells, rows_per_group, plan_flags, status);
    a.data = data;
    a.observed = observed;
    a.levels = (unsigned char*)workspace + l.levels;
    a.data_out = data_out;
    a.observed_out = observed_out;
    call_begin();
    dvs_launch_bn_impute(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_impute");
}

// ---- exact search (dvs_exact.h) --------------------------------------------------------------------------------------
static int exact_dims(const char* fn, int batch, int n_vars) {
    if (batch <= 0) return failf(2, "%s: batch must be > 0", fn);
    if (n_vars < 1 || n_vars > 20) return failf(3, "%s: n_vars must be in [1, 20]", fn);
    if (((int64_t)batch << n_vars) * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: batch * 2^n_vars * n_vars must be < 2^31", fn);
    return 0;
}

extern "C" size_t dvs_exact_workspace_bytes(int32_t batch, int32_t n_vars) {
    if (exact_dims("dvs_exact_workspace_bytes", batch, n_vars)) return 0;
    return dvs_exact_layout(batch, n_vars).total;
}

extern "C" int dvs_exact_search(int32_t batch, int32_t n_vars, const double* table, size_t table_bytes, int32_t max_parents,
                                const uint64_t* forbidden, void* workspace, size_t workspace_bytes, uint64_t* parents,
                                int32_t* order, double* score, int32_t* flags, void* stream) {
    if (int e = exact_dims("dvs_exact_search", batch, n_vars)) return e;
    if (!table || !workspace || !parents || !order || !score || !flags) return fail(10, "dvs_exact_search: null pointer");
    const size_t cells = ((size_t)batch << n_vars) * n_vars;
    if (table_bytes < cells * 8) return fail_size("dvs_exact_search: table_bytes < batch * 2^n_vars * n_vars * 8", cells * 8);
    const ExactLayout l = dvs_exact_layout(batch, n_vars);
    if (workspace_bytes < l.total) return fail_size("dvs_exact_search: workspace_bytes < dvs_exact_workspace_bytes", l.total);
    ExactArgs a;
    a.B = batch;
    a.n = n_vars;
    a.max_parents = max_parents;
    a.table = table;
    a.forbidden = forbidden;
    a.best = (double*)((char*)workspace + l.best);
    a.arg = (uint32_t*)((char*)workspace + l.arg);
    a.R = (double*)((char*)workspace + l.R);
    a.sink = (int*)((char*)workspace + l.sink);
    a.parents = parents;
    a.order = order;
    a.score = score;
    a.flags = flags;
    call_begin();
    dvs_launch_exact(a, (dvs_stream_t)stream);
    return call_end("dvs_exact_search");
}

// ---- exact arc posterior (dvs_posterior.h) ---------------------------------------------------------------------------
extern "C" size_t dvs_arc_posterior_workspace_bytes(int32_t batch, int32_t n_vars) {
    if (exact_dims("dvs_arc_posterior_workspace_bytes", batch, n_vars)) return 0;
    return dvs_posterior_layout(batch, n_vars).total;
}

extern "C" int dvs_arc_posterior(int32_t batch, int32_t n_vars, const double* table, size_t table_bytes, int32_t max_parents,
                                 const uint64_t* forbidden, const double* size_prior, void* workspace, size_t workspace_bytes,
                                 double* prob, double* log_z, double* family, size_t family_bytes, int32_t* flags, void* stream) {
    if (int e = exact_dims("dvs_arc_posterior", batch, n_vars)) return e;
    if (!table || !workspace || !prob || !log_z || !flags) return fail(10, "dvs_arc_posterior: null pointer");
    const size_t cells = ((size_t)batch << n_vars) * n_vars;
    if (table_bytes < cells * 8) return fail_size("dvs_arc_posterior: table_bytes < batch * 2^n_vars * n_vars * 8", cells * 8);
    const PosteriorLayout l = dvs_posterior_layout(batch, n_vars);
    if (workspace_bytes < l.total)
        return fail_size("dvs_arc_posterior: workspace_bytes < dvs_arc_posterior_workspace_bytes", l.total);
    if (family && family_bytes < cells * 8)
        return fail_size("dvs_arc_posterior: family_bytes < batch * 2^n_vars * n_vars * 8", cells * 8);
    PosteriorArgs a = {};
    a.B = batch;
    a.n = n_vars;
    a.max_parents = max_parents;
    a.table = table;
    a.forbidden = forbidden;
    a.size_prior = size_prior;
    a.alpha = (double*)((char*)workspace + l.alpha);
    a.L = (double*)((char*)workspace + l.L);
    a.Rb = (double*)((char*)workspace + l.Rb);
    a.partial = (double*)((char*)workspace + l.partial);
    a.prob = prob;
    a.log_z = log_z;
    a.family = family;
    a.flags = flags;
    call_begin();
    dvs_launch_arc_posterior(a, (dvs_stream_t)stream);
    return call_end("dvs_arc_posterior");
}

// ---- order MCMC over family lists (dvs_ordermc.h) --------------------------------------------------------------------
// after the counts: n_vars, then the size of sums
static int order_mcmc_shape(const char* fn, int chains, int n_vars) {
    if (n_vars < 1 || n_vars > DVS_WTOK) return failf(3, "%s: n_vars must be in [1, 48]", fn);
    if ((int64_t)chains * n_vars * n_vars > (int64_t)0x7fffffff) return failf(2, "%s: chains * n_vars^2 must be < 2^31", fn);
    return 0;
}

extern "C" int dvs_order_mcmc(int32_t chains, int32_t n_vars, int64_t n_families, int32_t steps, const int64_t* offsets,
                              const uint64_t* sets, size_t sets_bytes, const double* scores, size_t scores_bytes, uint64_t seed,
                              int64_t chain_offset, int64_t step_offset, int64_t burn_in, int32_t thin, int32_t window,
                              int32_t init, int32_t* order, double* log_score, int32_t* accepted, double* sums,
                              size_t sums_bytes, int32_t* kept, double* best_score, uint64_t* best_parents, double* trace,
                              size_t trace_bytes, int32_t* flags, void* stream) {
    const char* fn = "dvs_order_mcmc";
    if (chains <= 0) return fail(2, "dvs_order_mcmc: chains must be > 0");
    if (steps < 0) return fail(2, "dvs_order_mcmc: steps must be >= 0");
    if (n_families < 1 || n_families > (int64_t)0x7fffffff) return fail(2, "dvs_order_mcmc: n_families must be in [1, 2^31 - 1]");
    if (int e = order_mcmc_shape(fn, chains, n_vars)) return e;
    if (!offsets || !sets || !scores || !order || !log_score || !accepted || !sums || !kept || !best_score || !best_parents || !flags)
        return fail(10, "dvs_order_mcmc: null pointer");
    if (chain_offset < 0 || step_offset < 0) return fail(12, "dvs_order_mcmc: chain_offset and step_offset must be >= 0");
    const int widest = n_vars > 2 ? n_vars - 1 : 1;
    if (window < 1 || window > widest) return fail(13, "dvs_order_mcmc: window must be in [1, max(1, n_vars - 1)]");
    if (thin < 1) return fail(13, "dvs_order_mcmc: thin must be >= 1");
    if (burn_in < 0) return fail(13, "dvs_order_mcmc: burn_in must be >= 0");
    if (init != 0 && init != 1) return fail(13, "dvs_order_mcmc: init must be 0 or 1");
    if (step_offset > (int64_t)0xffffffff || 3 * (step_offset + (int64_t)steps) >= ((int64_t)1 << 32))
        return fail(13, "dvs_order_mcmc: 3 * (step_offset + steps) must be < 2^32");
    if (sets_bytes < (size_t)n_families * 8) return fail_size("dvs_order_mcmc: sets_bytes < n_families * 8", (size_t)n_families * 8);
    if (scores_bytes < (size_t)n_families * 8) return fail_size("dvs_order_mcmc: scores_bytes < n_families * 8", (size_t)n_families * 8);
    const size_t cells = (size_t)chains * n_vars * n_vars;
    if (sums_bytes < cells * 8) return fail_size("dvs_order_mcmc: sums_bytes < chains * n_vars^2 * 8", cells * 8);
    if (trace && trace_bytes < (size_t)chains * steps * 8)
        return fail_size("dvs_order_mcmc: trace_bytes < chains * steps * 8", (size_t)chains * steps * 8);
    OrderMcmcArgs a = {};
    a.C = chains;
    a.n = n_vars;
    a.steps = steps;
    a.thin = thin;
    a.window = window;
    a.init = init;
    a.F = n_families;
    a.chain_offset = (uint32_t)chain_offset;     // the global chain index is taken mod 2^32
    a.step_offset = (uint32_t)step_offset;
    a.burn_in = burn_in > (int64_t)0xffffffff ? 0xffffffffu : (uint32_t)burn_in;     // no step index reaches 2^32 / 3
    a.offsets = (const long long*)offsets;
    a.sets = sets;
    a.scores = scores;
    a.order = order;
    a.log_score = log_score;
    a.accepted = accepted;
    a.sums = sums;
    a.kept = kept;
    a.best_score = best_score;
    a.best_parents = best_parents;
    a.trace = trace;
    a.flags = flags;
    call_begin();
    dvs_launch_order_mcmc(a, seed, (dvs_stream_t)stream);
    return call_end(fn);
}

extern "C" int dvs_order_mcmc_finish(int32_t chains, int32_t n_vars, const double* sums, size_t sums_bytes, const int32_t* kept,
                                     double* prob, void* stream) {
    const char* fn = "dvs_order_mcmc_finish";
    if (chains <= 0) return fail(2, "dvs_order_mcmc_finish: chains must be > 0");
    if (int e = order_mcmc_shape(fn, chains, n_vars)) return e;
    if (!sums || !kept || !prob) return fail(10, "dvs_order_mcmc_finish: null pointer");
    const size_t cells = (size_t)chains * n_vars * n_vars;
    if (sums_bytes < cells * 8) return fail_size("dvs_order_mcmc_finish: sums_bytes < chains * n_vars^2 * 8", cells * 8);
    OrderMcmcFinishArgs a = {};
    a.C = chains;
    a.n = n_vars;
    a.sums = sums;
    a.kept = kept;
    a.prob = prob;
    call_begin();
    dvs_launch_order_mcmc_finish(a, (dvs_stream_t)stream);
    return call_end(fn);
}

// ---- row sets, bootstrap, arc strength, averaged network (dvs_strength.h) ---------------------------------------------
// What the two *_rows entry points check alike, after the score argument: the row-set arguments (code 13), into their block.
static int row_set_args(const char* fn, RowSetArgs& r, int batch, const int32_t* rows, int set_size, int n_sets, const int32_t* set_of) {
    if (set_size < 1 || n_sets < 1) return failf(13, "%s: set_size and n_sets must be >= 1", fn);
    if (!set_of && n_sets < batch) return failf(13, "%s: set_of is null (structure b uses set b), so n_sets must be >= batch", fn);
    r.rows = rows;
    r.set_of = set_of;
    r.set_size = set_size;
    r.n_sets = n_sets;
    return 0;
}

extern "C" int dvs_bn_scores_rows(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                                  const uint64_t* parents, int32_t score_type, double score_arg, double* scratch, double* out,
                                  int32_t* status, const int32_t* rows, int32_t set_size, int32_t n_sets, const int32_t* set_of,
                                  void* stream) {
    const char* fn = "dvs_bn_scores_rows";
    if (int e = scorer_check(fn, batch, n_vars, n_samples, false, !data || !card || !parents || !scratch || !out || !status || !rows))
        return e;
    BicRowsArgs a = {};
    if (int e = scorer_args(fn, a.s, batch, n_vars, set_size, data, card, parents, score_type, score_arg, scratch, out, status)) return e;
    if (int e = row_set_args(fn, a.r, batch, rows, set_size, n_sets, set_of)) return e;
    call_begin();
    dvs_launch_bic_rows(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_scores_rows");
}

extern "C" int dvs_bn_toggle_scores_rows(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data,
                                         const uint8_t* card, const uint64_t* parents, int32_t score_type, double score_arg,
                                         const int32_t* worklist, double* local, size_t local_bytes, double* toggles,
                                         size_t toggles_bytes, int32_t* status, const int32_t* rows, int32_t set_size,
                                         int32_t n_sets, const int32_t* set_of, void* stream) {
    const char* fn = "dvs_bn_toggle_scores_rows";
    if (int e = scorer_check(fn, batch, n_vars, n_samples, true, !data || !card || !parents || !local || !toggles || !status || !rows))
        return e;
    ToggleRowsArgs a = {};
    if (int e = scorer_args(fn, a.t.s, batch, n_vars, set_size, data, card, parents, score_type, score_arg, local, nullptr, status))
        return e;
    if (int e = row_set_args(fn, a.r, batch, rows, set_size, n_sets, set_of)) return e;
    if (int e = toggle_buffers({fn, batch, n_vars}, local_bytes, toggles_bytes)) return e;
    a.t.worklist = worklist;
    a.t.toggles = toggles;
    call_begin();
    dvs_launch_bn_toggle_rows(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_toggle_scores_rows");
}

// ---- available-case scoring on incomplete data (dvs_available.h; include/dvs_available.h) ------------------------------
// k of the two *_avail entry points, checked where the plain ones check score_arg; the block then holds loglik with arg = k
static int avail_args(const char* fn, BicArgs& a, int batch, int n_vars, int n_samples, const uint64_t* data, const uint8_t* card,
                      const uint64_t* parents, double k, double* local, double* out, int32_t* status) {
    if (!(k >= 0.0 && isfinite(k))) return failf(13, "%s: k must be finite and >= 0", fn);
    if (int e = scorer_args(fn, a, batch, n_vars, n_samples, data, card, parents, DVS_SCORE_LOGLIK, __builtin_nan(""), local, out, status))
        return e;
    a.arg = k;
    return 0;
}

extern "C" int dvs_bn_scores_avail(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint64_t* observed,
                                   const uint8_t* card, const uint64_t* parents, double k, double* local, double* out,
                                   int32_t* used, int32_t* status, void* stream) {
    const char* fn = "dvs_bn_scores_avail";
    if (int e = scorer_check(fn, batch, n_vars, n_samples, false, !data || !observed || !card || !parents || !local || !out || !status))
        return e;
    BicAvailArgs a = {};
    if (int e = avail_args(fn, a.s, batch, n_vars, n_samples, data, card, parents, k, local, out, status)) return e;
    a.observed = observed;
    a.used = used;
    call_begin();
    dvs_launch_bn_avail(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_scores_avail");
}

extern "C" int dvs_bn_toggle_scores_avail(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data,
                                          const uint64_t* observed, const uint8_t* card, const uint64_t* parents, double k,
                                          const int32_t* worklist, double* local, size_t local_bytes, double* toggles,
                                          size_t toggles_bytes, int32_t* status, void* stream) {
    const char* fn = "dvs_bn_toggle_scores_avail";
    if (int e = scorer_check(fn, batch, n_vars, n_samples, true, !data || !observed || !card || !parents || !local || !toggles || !status))
        return e;
    ToggleAvailArgs a = {};
    if (int e = avail_args(fn, a.t.s, batch, n_vars, n_samples, data, card, parents, k, local, nullptr, status)) return e;
    if (int e = toggle_buffers({fn, batch, n_vars}, local_bytes, toggles_bytes)) return e;
    a.observed = observed;
    a.t.worklist = worklist;
    a.t.toggles = toggles;
    call_begin();
    dvs_launch_bn_toggle_avail(a, (dvs_stream_t)stream);
    return call_end("dvs_bn_toggle_scores_avail");
}

extern "C" int dvs_bootstrap_rows(int32_t n_sets, int32_t set_size, int32_t n_samples, uint64_t seed, int64_t set_offset,
                                  int32_t* rows, void* stream) {
    if (n_sets <= 0) return fail(2, "dvs_bootstrap_rows: n_sets must be > 0");
    if (set_size < 1 || n_samples < 1) return fail(13, "dvs_bootstrap_rows: set_size and n_samples must be >= 1");
    if ((int64_t)n_sets * set_size > (int64_t)0x7fffffff) return fail(2, "dvs_bootstrap_rows: n_sets * set_size must be < 2^31");
    if (set_offset < 0) return fail(12, "dvs_bootstrap_rows: set_offset must be >= 0");
    if (!rows) return fail(10, "dvs_bootstrap_rows: null pointer");
    BootRowsArgs a = {};
    a.n_sets = n_sets;
    a.set_size = set_size;
    a.n_samples = n_samples;
    a.set_offset = (uint32_t)set_offset;         // the global set index is taken mod 2^32
    a.rows = rows;
    call_begin();
    dvs_launch_bootstrap_rows(a, seed, (dvs_stream_t)stream);
    return call_end("dvs_bootstrap_rows");
}

extern "C" int dvs_arc_strength(int32_t batch, int32_t n_vars, const uint64_t* pdag, int32_t* counts, size_t counts_bytes,
                                void* stream) {
    if (int e = pdag_dims("dvs_arc_strength", batch, n_vars)) return e;
    if (!pdag || !counts) return fail(10, "dvs_arc_strength: null pointer");
    if (counts_bytes < (size_t)n_vars * n_vars * 8)
        return fail_size("dvs_arc_strength: counts_bytes < n_vars^2 * 8", (size_t)n_vars * n_vars * 8);
    ArcStrengthArgs a;
    a.B = batch;
    a.n = n_vars;
    a.pdag = pdag;
    a.counts = counts;
    call_begin();
    dvs_launch_arc_strength(a, (dvs_stream_t)stream);
    return call_end("dvs_arc_strength");
}

extern "C" int dvs_averaged_network(int32_t groups, int32_t n_vars, const int32_t* counts, const int32_t* n_networks,
                                    const int32_t* min_any, uint64_t* parents, size_t parents_bytes, int32_t* info,
                                    void* stream) {
    if (groups <= 0) return fail(2, "dvs_averaged_network: groups must be > 0");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_averaged_network: n_vars must be in [1, 48]");
    if ((int64_t)groups * n_vars * n_vars * 2 > (int64_t)0x7fffffff)
        return fail(2, "dvs_averaged_network: groups * n_vars^2 * 2 must be < 2^31");
    if (!counts || !n_networks || !min_any || !parents || !info) return fail(10, "dvs_averaged_network: null pointer");
    if (parents_bytes < (size_t)groups * n_vars * 8)
        return fail_size("dvs_averaged_network: parents_bytes < groups * n_vars * 8", (size_t)groups * n_vars * 8);
    AvgNetArgs a;
    a.G = groups;
    a.n = n_vars;
    a.counts = counts;
    a.n_networks = n_networks;
    a.min_any = min_any;
    a.parents = parents;
    a.info = info;
    call_begin();
    dvs_launch_averaged_network(a, (dvs_stream_t)stream);
    return call_end("dvs_averaged_network");
}

extern "C" int dvs_bic_parent_masks(int32_t batch, int32_t n_vars, int32_t preds_are_u64, const uint8_t* labels,
                                    const void* preds, uint64_t* parents, int32_t* status, void* stream) {
    if (batch <= 0) return fail(2, "dvs_bic_parent_masks: batch must be > 0");
    if (n_vars < 1 || n_vars > DVS_WTOK) return fail(3, "dvs_bic_parent_masks: n_vars must be in [1, 48]");
    if (!preds_are_u64 && n_vars > 16) return fail(12, "dvs_bic_parent_masks: 16-bit predecessor rows hold at most 16 vertices");
    if (!labels || !preds || !parents || !status) return fail(10, "dvs_bic_parent_masks: null pointer");
    BicMaskArgs a;
    a.B = batch;
    a.n = n_vars;
    a.wide = preds_are_u64 ? 1 : 0;
    a.labels = labels;
    a.preds = preds;
    a.parents = parents;
    a.status = status;
    call_begin();
    dvs_launch_bic_parent_masks(a, (dvs_stream_t)stream);
    return call_end("dvs_bic_parent_masks");
}

// ---- GP predictor (k_bic.hip, k_gp_acq.hip) --------------------------------------------------------------------------
extern "C" int dvs_gp_predict(int32_t batch, int32_t n_inducing, int32_t dim, const float* x, const float* inducing,
                              const double* alpha, double outputscale, double lengthscale, double constant, double* out,
                              void* stream) {
    if (batch <= 0 || n_inducing <= 0 || dim <= 0) return fail(2, "dvs_gp_predict: sizes must be > 0");
    if (!(lengthscale > 0.0)) return fail(5, "dvs_gp_predict: lengthscale must be > 0");
    if (!x || !inducing || !alpha || !out) return fail(10, "dvs_gp_predict: null pointer");
    GpArgs a = {};
    a.B = batch;
    a.M = n_inducing;
    a.D = dim;
    a.x = x;
    a.z = inducing;
    a.alpha = alpha;
    a.outputscale = outputscale;
    a.constant = constant;
    a.out = out;
    call_begin();
    dvs_launch_gp_predict(a, lengthscale, (dvs_stream_t)stream);
    return call_end("dvs_gp_predict");
}

static int gp_check(const char* fn, int na, int nb, int dim, double outputscale, double lengthscale) {
    if (na <= 0 || nb <= 0 || dim <= 0 || dim > 32) return failf(2, "%s: sizes must be > 0 and dim <= 32", fn);
    if (!(lengthscale > 0.0) || !(outputscale > 0.0)) return failf(5, "%s: lengthscale and outputscale must be > 0", fn);
    return 0;
}
extern "C" int dvs_gp_kernel(int32_t na, int32_t nb, int32_t dim, const float* xa, const float* xb, double outputscale,
                             double lengthscale, double* K, void* stream) {
    if (int e = gp_check("dvs_gp_kernel", na, nb, dim, outputscale, lengthscale)) return e;
    if (!xa || !xb || !K) return fail(10, "dvs_gp_kernel: null pointer");
    GpKernArgs a = {};
    a.na = na;
    a.nb = nb;
    a.D = dim;
    a.xa = xa;
    a.xb = xb;
    a.outputscale = outputscale;
    a.K = K;
    call_begin();
    dvs_launch_gp_kernel(a, lengthscale, (dvs_stream_t)stream);
    return call_end("dvs_gp_kernel");
}
extern "C" int dvs_gp_kernel_backward(int32_t na, int32_t nb, int32_t dim, int32_t symmetric, const float* xa, const float* xb,
                                      double outputscale, double lengthscale, const double* G, double* dxa, double* row_sums,
                                      void* stream) {
    if (int e = gp_check("dvs_gp_kernel_backward", na, nb, dim, outputscale, lengthscale)) return e;
    if (!xa || !xb || !G || !dxa || !row_sums) return fail(10, "dvs_gp_kernel_backward: null pointer");
    if (symmetric && na != nb) return fail(12, "dvs_gp_kernel_backward: symmetric needs na == nb");
    GpKernArgs a = {};
    a.na = na;
    a.nb = nb;
    a.D = dim;
    a.symmetric = symmetric;
    a.xa = xa;
    a.xb = xb;
    a.outputscale = outputscale;
    a.G = G;
    a.dxa = dxa;
    a.rows = row_sums;
    call_begin();
    dvs_launch_gp_kernel_bwd(a, lengthscale, (dvs_stream_t)stream);
    return call_end("dvs_gp_kernel_backward");
}

extern "C" int dvs_gp_acquire(int32_t batch, int32_t n_inducing, int32_t dim, int32_t ld, const float* x, const float* inducing,
                              const double* weights, double c0, double outputscale, double lengthscale, double constant,
                              double best, double xi, double* mean, double* var, double* ei, float* grad, void* stream) {
    if (int e = gp_check("dvs_gp_acquire", batch, n_inducing, dim, outputscale, lengthscale)) return e;
    if (n_inducing > DVS_GP_ACQ_MAX_INDUCING) return fail(2, "dvs_gp_acquire: n_inducing must be <= 1023");
    if (ld < n_inducing + 1) return fail(12, "dvs_gp_acquire: ld must be >= n_inducing + 1 (P | alpha)");
    if (!(c0 >= 0.0)) return fail(12, "dvs_gp_acquire: c0 must be >= 0");
    if (!x || !inducing || !weights || !mean || !var || !ei) return fail(10, "dvs_gp_acquire: null pointer");
    if (!dvs_launch_gp_acquire) return fail(20, "dvs_gp_acquire: k_gp_acq.hip is not part of this build");   // weak: dvs_search_args.h
    GpAcqArgs a = {};
    a.Q = batch;
    a.M = n_inducing;
    a.D = dim;
    a.ld = ld;
    a.x = x;
    a.z = inducing;
    a.W = weights;
    a.c0 = c0;
    a.outputscale = outputscale;
    a.constant = constant;
    a.best = best;
    a.xi = xi;
    a.mean = mean;
    a.var = var;
    a.ei = ei;
    a.grad = grad;
    call_begin();
    dvs_launch_gp_acquire(a, lengthscale, (dvs_stream_t)stream);
    return call_end("dvs_gp_acquire");
}
