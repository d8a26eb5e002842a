// C ABI (include/dvs.h): parameter/workspace layout, the call context and the launch sequences of the PACE-VAE model path
// (pack, forward, encode, decode; backward in dvs_api_backward.inc); the search-side entry points are dvs_api_search.inc.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dvs_kernels.h"
#include "dvs_backward.h"
#include "dvs_wide.h"
#include "dvs_wimg.h"
#include "dvs_decode.h"
#include "dvs_search_args.h"

static thread_local char g_err[256] = "";

// ---- optional per-kernel timing (HIP events on the launch stream) -------------------------------------------------
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
namespace {
struct ProfRec {
    const char* name;
#ifndef DVS_EMU
    hipEvent_t a, b;
#endif
};
// The one piece of process-global mutable state of the library: begin/end pairs of concurrent callers may interleave
// (the record then pairs the wrong events), but the container itself is never corrupted.
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
thread_local int t_prof_slot = -1;      // index of this thread's open record
}  // namespace

void dvs_prof_begin(const char* name, dvs_stream_t st) {
    t_prof_slot = -1;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof_on) return;
    ProfRec r;
    r.name = name;
#ifndef DVS_EMU
    if (hipEventCreate(&r.a) != hipSuccess) return;
    if (hipEventCreate(&r.b) != hipSuccess) {
        (void)hipEventDestroy(r.a);
        return;
    }
    (void)hipEventRecord(r.a, st);
#endif
    t_prof_slot = (int)g_prof.size();
    g_prof.push_back(r);
}
void dvs_prof_end(dvs_stream_t st) {
    if (t_prof_slot < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
#ifndef DVS_EMU
    if (t_prof_slot < (int)g_prof.size()) (void)hipEventRecord(g_prof[t_prof_slot].b, st);
#endif
    t_prof_slot = -1;
}
extern "C" void dvs_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on = on != 0;
}
// Waits for the recorded events, then writes up to `cap` rows (name, launches, total milliseconds); returns the
// number of distinct kernels and clears the record.
extern "C" int dvs_profile_collect(char* names, int name_stride, int* counts, float* total_ms, int cap) {
    std::map<std::string, std::pair<int, float>> agg;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto& r : g_prof) {
        float ms = 0.f;
#ifndef DVS_EMU
        (void)hipEventSynchronize(r.b);
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
#endif
        auto& e = agg[r.name];
        e.first += 1;
        e.second += ms;
    }
    g_prof.clear();
    int i = 0;
    for (auto& kv : agg) {
        if (i >= cap) break;
        snprintf(names + (size_t)i * name_stride, name_stride, "%s", kv.first.c_str());
        counts[i] = kv.second.first;
        total_ms[i] = kv.second.second;
        ++i;
    }
    return (int)agg.size();
}

static int fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// ---- HIP runtime failures inside an entry point (DVS_LAUNCH / DVS_SET_LDS, dvs_kernels.h) ---------------------------
static thread_local int t_hip_err = 0;
static thread_local char t_hip_msg[200] = "";
void dvs_note_hip_error(const char* what, int hip_error, const char* hip_message) {
    if (t_hip_err != 0) return;             // keep the first failure of the call
    t_hip_err = hip_error ? hip_error : -1;
    snprintf(t_hip_msg, sizeof(t_hip_msg), "%s: HIP error %d (%s)", what, hip_error, hip_message ? hip_message : "?");
}
static void call_begin() {
    t_hip_err = 0;
    (void)hipGetLastError();                // errors that are not ours must not be attributed to our launches
}
static int call_end(const char* fn) {
    if (t_hip_err == 0) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, t_hip_msg);
    t_hip_err = 0;
    return 20;
}
#define DVS_HIP_CALL(expr)                                                             \
    do {                                                                               \
        const hipError_t dvs_ce_ = (expr);                                             \
        if (dvs_ce_ != hipSuccess) dvs_note_hip_error(#expr, (int)dvs_ce_, hipGetErrorString(dvs_ce_)); \
    } while (0)
// device-to-device copy on the call's stream (the emulator header brings its own shim)
static void copy_out(void* dst, const void* src, size_t bytes, dvs_stream_t st) {
#ifdef DVS_EMU
    DVS_HIP_CALL(hipMemcpyAsyncD2D(dst, src, bytes, st));
#else
    DVS_HIP_CALL(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
#endif
}

extern "C" int dvs_version(void) { return DVS_VERSION; }
extern "C" const char* dvs_last_error(void) { return g_err; }

extern "C" int dvs_device_cus(void) {
#ifdef DVS_EMU
    return 2;
#else
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
#endif
}

// ---- flat parameter layout ---------------------------------------------------------------------------------
namespace {
struct LayoutBuilder {
    int64_t off = 0;
    dvs_param_entry* table;
    int cap, count = 0;
    // the name is formatted only when a table asks for it: the entry points want the offsets alone, once per call
    int64_t add(int rows, int cols, const char* fmt, ...) {
        const int64_t o = off;
        if (table && count < cap) {
            dvs_param_entry& e = table[count];
            memset(&e, 0, sizeof(e));
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(e.name, sizeof(e.name), fmt, ap);
            va_end(ap);
            e.offset = o;
            e.rows = rows;
            e.cols = cols;
        }
        ++count;
        const int64_t n = (int64_t)rows * (cols ? cols : 1);
        off += (n + 3) & ~(int64_t)3;
        return o;
    }
};
}  // namespace

DvsLayout dvs_make_layout(int N, int C, dvs_param_entry* table, int cap, int* count) {
    LayoutBuilder b;
    b.table = table;
    b.cap = cap;
    DvsLayout l;
    auto attn = [&](const char* stack, int i, const char* which, DvsAttnP& p) {
        p.in_w = b.add(192, 64, "%s.layers.%d.%s.in_proj_weight", stack, i, which);
        p.in_b = b.add(192, 0, "%s.layers.%d.%s.in_proj_bias", stack, i, which);
        p.out_w = b.add(64, 64, "%s.layers.%d.%s.out_proj.weight", stack, i, which);
        p.out_b = b.add(64, 0, "%s.layers.%d.%s.out_proj.bias", stack, i, which);
    };
    auto ffn = [&](const char* stack, int i, DvsFfnP& p) {
        p.l1_w = b.add(64, 64, "%s.layers.%d.linear1.weight", stack, i);
        p.l1_b = b.add(64, 0, "%s.layers.%d.linear1.bias", stack, i);
        p.l2_w = b.add(64, 64, "%s.layers.%d.linear2.weight", stack, i);
        p.l2_b = b.add(64, 0, "%s.layers.%d.linear2.bias", stack, i);
    };
    auto norm = [&](const char* stack, int i, int k, DvsNormP& p) {
        p.w = b.add(64, 0, "%s.layers.%d.norm%d.weight", stack, i, k);
        p.b = b.add(64, 0, "%s.layers.%d.norm%d.bias", stack, i, k);
    };
    l.W1 = b.add(2 * N, 64, "vertex_position_embed.W1");
    l.W2 = b.add(64, 32, "vertex_position_embed.W2");
    l.lab_w = b.add(32, C, "vertex_label_embed.0.weight");
    l.lab_b = b.add(32, 0, "vertex_label_embed.0.bias");
    for (int i = 0; i < DVS_LAYERS; ++i) {
        attn("encoder", i, "self_attn", l.enc[i].sa);
        ffn("encoder", i, l.enc[i].ff);
        norm("encoder", i, 1, l.enc[i].n1);
        norm("encoder", i, 2, l.enc[i].n2);
    }
    l.fc1_w = b.add(32, N * 64, "fc1.weight");
    l.fc1_b = b.add(32, 0, "fc1.bias");
    l.fc2_w = b.add(32, N * 64, "fc2.weight");
    l.fc2_b = b.add(32, 0, "fc2.bias");
    for (int i = 0; i < DVS_LAYERS; ++i) {
        attn("decoder", i, "self_attn", l.dec[i].sa);
        attn("decoder", i, "multihead_attn", l.dec[i].ca);
        ffn("decoder", i, l.dec[i].ff);
        norm("decoder", i, 1, l.dec[i].n1);
        norm("decoder", i, 2, l.dec[i].n2);
        norm("decoder", i, 3, l.dec[i].n3);
    }
    l.node0_w = b.add(32, 64, "add_node.0.weight");
    l.node0_b = b.add(32, 0, "add_node.0.bias");
    l.node2_w = b.add(C, 32, "add_node.2.weight");
    l.node2_b = b.add(C, 0, "add_node.2.bias");
    l.edge0_w = b.add(64, 128, "add_edge.0.weight");
    l.edge0_b = b.add(64, 0, "add_edge.0.bias");
    l.edge2_w = b.add(1, 64, "add_edge.2.weight");
    l.edge2_b = b.add(1, 0, "add_edge.2.bias");
    l.fc3_w = b.add(N * 64, 32, "fc3.weight");
    l.fc3_b = b.add(N * 64, 0, "fc3.bias");
    l.total = b.off;
    if (count) *count = b.count;
    return l;
}

DvsWorkspace dvs_make_workspace(int B, int NT, int64_t P, int nslab, bool wide) {
    DvsWorkspace w;
    size_t off = 0;
    auto take = [&](size_t n) {
        const size_t o = off;
        off += (n + 63) & ~(size_t)63;
        return o;
    };
    const size_t tile = (size_t)B * NT * 1024;
    for (int s = 0; s < DVS_NSLOTS; ++s) {
        w.act[s] = take(tile);
        w.stats[s] = take((size_t)B * NT * 32);
    }
    w.enc_out = take(tile);
    w.mu = take((size_t)B * 32);
    w.logvar = take((size_t)B * 32);
    w.z = take((size_t)B * 32);
    w.epsv = take((size_t)B * 32);
    w.mem = take(tile);
    w.dag_loss = take((size_t)B * 2);
    w.gA = take(tile);
    w.gB = take(tile);
    w.gq = take(tile);
    w.gk = take(tile);
    w.gv = take(tile);
    w.gmem = take(tile);
    w.genc = take(tile);
    w.gz = take((size_t)B * 64);
    w.nslab = nslab;
    w.slabs = take((size_t)nslab * (size_t)P);
    w.fcpart = take((size_t)DVS_FC_PARTS * (size_t)P);
    w.wimg = take((DVS_WIMG_BF16 + 1) / 2);
    w.limg = take(DvsLatImg::floats(NT));
    for (int blk = 0; blk < 9; ++blk) w.qkv[blk] = take(wide ? (size_t)B * NT * 12 * 256 : 0);
    w.total_floats = off;
    return w;
}

// ---- shape checks / derived dims ------------------------------------------------------------------------------
static int check_shape(const dvs_shape* s) {
    if (!s) return fail(1, "dvs: null shape");
    if (s->batch <= 0) return fail(2, "dvs: batch must be > 0");
    if (s->n_tokens < 4 || s->n_tokens > DVS_WTOK)
        return fail(3, "dvs: n_tokens (= max_num_vertices + 3) must be in [4, 48] in this build");
    if (s->n_classes < 4 || s->n_classes > DVS_WTOK)
        return fail(4, "dvs: n_classes (= vertex_label_cardinality + 3) must be in [4, 48] in this build");
    if (!(s->dropout >= 0.f && s->dropout < 1.f)) return fail(5, "dvs: dropout must be in [0, 1)");
    return 0;
}

// One-tile path: a wave owns a whole DAG (N, C <= 16).  Wide path: NT tiles of 16 tokens per DAG, cross-token kernels
// of dvs_wide.h (also taken when only the class count exceeds one tile).
static bool is_wide(const dvs_shape* s) { return s->n_tokens > DVS_MAXTOK || s->n_classes > 16; }
static int tiles_of(const dvs_shape* s) { return (s->n_tokens + 15) / 16; }
static size_t record_size(bool wide) { return wide ? sizeof(DvsRecordW) : sizeof(DvsRecord); }

static DvsDims make_dims(const dvs_shape* s) {
    DvsDims d;
    d.NT = tiles_of(s);
    d.B = s->batch;
    d.N = s->n_tokens;
    d.C = s->n_classes;
    d.training = s->training ? 1 : 0;
    d.drop.thr16 = (uint32_t)lrintf(s->dropout * 65536.0f);
    d.drop.on = (d.training && d.drop.thr16 > 0) ? 1 : 0;
    d.drop.scale = 1.0f / (1.0f - (float)d.drop.thr16 / 65536.0f);
    d.seed_lo = (uint32_t)(s->seed & 0xFFFFFFFFull);
    d.seed_hi = (uint32_t)(s->seed >> 32);
    d.dag_offset = s->dag_offset;
    d.beta = s->beta;
    d.eps_scale = s->eps_scale;
    d.debug = 0;
    return d;
}

// Backward kernels run on at most this many workgroups (one gradient slab each): sizes the workspace and caps every
// persistent grid.
static int num_slabs() {
    const int cus = dvs_device_cus();
    return cus > 0 ? cus : 256;
}
static int grid_for(int units, int per_wg, int cap) {   // persistent kernels: `per_wg` units (tiles / DAGs) per pass
    const int want = (units + per_wg - 1) / per_wg;
    return want < cap ? want : cap;
}

// Waves per workgroup of the one-tile stack kernels (k_fwd_stack / k_bwd_stack and their per-phase twins).  8: two waves per
// SIMD, 8 DAGs per workgroup and pass — the mapping every kernel was tuned for; it fills the chip from 8 x #CU DAGs up.  Below
// 4 x #CU DAGs (1 024 on an MI355X: a 4 096 batch cut over 4 or 8 GPUs) half of the CUs or more would idle while the others
// run two waves per SIMD, so the NARROW mapping takes over: 4 waves (one cooperative weight-gradient group), 4 DAGs per
// workgroup, twice the workgroups, one wave per SIMD.  DVS_WAVES_PER_WG=4|8 forces either (A/B runs, tests).
static int waves_per_wg(const DvsDims& d, bool wide, int nslab) {
    const char* env = getenv("DVS_WAVES_PER_WG");         // read per call: the tests switch it between calls
    const int force = env ? atoi(env) : 0;
    if (wide) return 8;
    if (force == 4 || force == 8) return force;
    return d.B <= 4 * nslab ? 4 : 8;
}
// Workgroups of the backward kernels = gradient slabs that are written (and reduced) this step: all of them from 4 x #CU
// DAGs up; fewer for smaller batches, so that k_reduce_slabs does not stream slabs of zeros.
static int active_slabs(const DvsDims& d, bool wide, int nslab) {
    if (wide) return nslab;
    const int want = (d.B + 3) / 4;          // the narrowest backward kernels own 4 DAGs per workgroup and pass
    return want < nslab ? want : nslab;
}

// A/B switches, read once per process.  DVS_SPLIT_STACK=1 (per-phase profiling): every sublayer is a launch of its own.
// DVS_LATENT_KERNELS=1: the latent block keeps its own launches.
static bool env_on(const char* name) {
    const char* v = getenv(name);
    return v && atoi(v) != 0;
}
static bool split_stack() {
    static const bool on = env_on("DVS_SPLIT_STACK");
    return on;
}
static bool latent_kernels_off() {
    static const bool on = env_on("DVS_LATENT_KERNELS");
    return on;
}
// The latent block rides the encoder chain (forward: its last phase, backward: ahead of its first), in the same launch.  Only
// on the 8-wave mapping: a narrow workgroup owns 4 DAGs, a quarter of an MFMA column group.
static bool latent_in_chain(bool chain, int nw) { return chain && !latent_kernels_off() && nw == 8; }

// launch grids of the forward kernels
struct FwdGrids {
    int chain;      // k_fwd_stack / k_attn_fwd / narrow k_ffn_fwd, k_embed_fwd, k_loss_fwd: nw tiles per workgroup and pass
    int tiles16;    // 16-wave tile-parallel kernels (k_ffn_fwd, one-tile k_embed_fwd)
    int tiles8;     // 8-wave tile-parallel kernels (one-tile k_attn_fwd / k_embed_fwd / k_loss_fwd)
    int tiles4;     // 4-wave tile-parallel kernels (k_embed_fwd_w)
    int dags;       // workgroup-per-DAG kernels of the wide path
    int dags2;      // ... those that fit two workgroups per CU (k_loss_fwd_w)
    int dec4;       // k_decode_step: 4 DAGs per workgroup and pass
};

// ---- call context: what every launch of the train step, of dvs_encode and of dvs_decode is filled from ---------------------
struct Step {
    DvsDims d;
    DvsLayout L;
    DvsWorkspace W;
    bool wide;
    const float* P;             // flat parameters
    float* ws;                  // workspace
    const DvsRecord* rec;
    dvs_stream_t st;
    int nw;                     // waves per workgroup of the one-tile stack kernels (waves_per_wg)
    FwdGrids g;
    int slabs;                  // workgroups of every backward kernel (active_slabs)
};
// After check_shape(); layout and workspace are computed here, once per call.
static Step make_step(const dvs_shape* s, const void* records, const float* params, void* workspace, void* stream) {
    Step c;
    c.d = make_dims(s);
    c.L = dvs_make_layout(c.d.N, c.d.C, nullptr, 0, nullptr);
    c.wide = is_wide(s);
    const int nslab = num_slabs();
    c.W = dvs_make_workspace(c.d.B, c.d.NT, c.L.total, nslab, c.wide);
    c.P = params;
    c.ws = (float*)workspace;
    c.rec = (const DvsRecord*)records;
    c.st = (dvs_stream_t)stream;
    c.nw = waves_per_wg(c.d, c.wide, nslab);
    const int tiles = c.d.B * c.d.NT;
    c.g.chain = grid_for(tiles, c.nw, nslab);
    c.g.tiles16 = grid_for(tiles, 16, nslab);
    c.g.tiles8 = grid_for(tiles, 8, nslab);
    c.g.tiles4 = grid_for(tiles, 4, nslab);
    c.g.dags = grid_for(c.d.B, 1, nslab);
    c.g.dags2 = c.d.B < 2 * c.g.dags ? c.d.B : 2 * c.g.dags;
    c.g.dec4 = grid_for(c.d.B, 4, nslab);
    c.slabs = active_slabs(c.d, c.wide, nslab);
    return c;
}

// Caller-owned buffers against what the shape needs (include/dvs.h: code 14); nothing has been enqueued yet.
static int check_records(const char* fn, size_t records_bytes, int batch, bool wide) {
    const size_t need = (size_t)batch * record_size(wide);
    if (records_bytes >= need) return 0;
    char msg[240];
    snprintf(msg, sizeof(msg), "%s: records_bytes %zu < batch * dvs_record_bytes = %zu", fn, records_bytes, need);
    return fail(14, msg);
}
static int check_buffers(const Step& c, const char* fn, size_t records_bytes, int64_t n_params, size_t workspace_bytes) {
    if (int e = check_records(fn, records_bytes, c.d.B, c.wide)) return e;
    char msg[240];
    if (n_params < c.L.total) {
        snprintf(msg, sizeof(msg), "%s: n_params %lld < dvs_param_count = %lld", fn, (long long)n_params, (long long)c.L.total);
        return fail(14, msg);
    }
    const size_t need = c.W.total_floats * sizeof(float);
    if (workspace_bytes < need) {
        snprintf(msg, sizeof(msg), "%s: workspace_bytes %zu < dvs_workspace_bytes = %zu", fn, workspace_bytes, need);
        return fail(14, msg);
    }
    return 0;
}

extern "C" int64_t dvs_param_count(const dvs_shape* s) {
    if (check_shape(s)) return -1;
    return dvs_make_layout(s->n_tokens, s->n_classes, nullptr, 0, nullptr).total;
}

extern "C" int dvs_param_table(const dvs_shape* s, dvs_param_entry* out, int cap) {
    if (check_shape(s)) return -1;
    int count = 0;
    dvs_make_layout(s->n_tokens, s->n_classes, out, cap, &count);
    return count;
}

extern "C" size_t dvs_workspace_bytes(const dvs_shape* s) {
    if (check_shape(s)) return 0;
    return make_step(s, nullptr, nullptr, nullptr, nullptr).W.total_floats * sizeof(float);
}

extern "C" size_t dvs_record_bytes(const dvs_shape* s) {
    if (check_shape(s)) return 0;
    return record_size(is_wide(s));
}

extern "C" int dvs_pack_features(const dvs_shape* s, const float* label_onehot, const float* pos_onehot,
                                 const float* adjacency, const uint8_t* target_masks, void* records, size_t records_bytes,
                                 int32_t* status, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!label_onehot || !pos_onehot || !adjacency || !target_masks || !records || !status)
        return fail(10, "dvs_pack_features: null pointer");
    if (int e = check_records("dvs_pack_features", records_bytes, s->batch, is_wide(s))) return e;
    call_begin();
    PackArgs a;
    a.B = s->batch;
    a.N = s->n_tokens;
    a.C = s->n_classes;
    a.lab1h = label_onehot;
    a.pos1h = pos_onehot;
    a.adj = adjacency;
    a.tmask = target_masks;
    a.rec = (DvsRecord*)records;
    a.status = status;
    if (is_wide(s)) dvs_launch_pack_w(a, (dvs_stream_t)stream);
    else dvs_launch_pack(a, (dvs_stream_t)stream);
    return call_end("dvs_pack_features");
}

extern "C" int dvs_build_records(const dvs_shape* s, const uint8_t* labels, const void* preds, void* records,
                                 size_t records_bytes, int32_t* status, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!labels || !preds || !records || !status) return fail(10, "dvs_build_records: null pointer");
    if (int e = check_records("dvs_build_records", records_bytes, s->batch, is_wide(s))) return e;
    call_begin();
    if (is_wide(s)) {
        BuildWArgs a;
        a.B = s->batch;
        a.N = s->n_tokens;
        a.C = s->n_classes;
        a.labels = labels;
        a.preds = (const uint64_t*)preds;
        a.rec = (DvsRecordW*)records;
        a.status = status;
        dvs_launch_build_records_w(a, (dvs_stream_t)stream);
        return call_end("dvs_build_records");
    }
    BuildArgs a;
    a.B = s->batch;
    a.N = s->n_tokens;
    a.C = s->n_classes;
    a.labels = labels;
    a.preds = (const uint16_t*)preds;
    a.rec = (DvsRecord*)records;
    a.status = status;
    dvs_launch_build_records(a, (dvs_stream_t)stream);
    return call_end("dvs_build_records");
}

// slot numbering of saved activations
static inline int slot_enc(int layer, int sub) { return 1 + 2 * layer + sub; }        // sub 0 attn, 1 ffn
static inline int slot_dec(int layer, int sub) { return 8 + 3 * layer + sub; }        // sub 0 self, 1 cross, 2 ffn
// dropout sites (34 per step): 0,1 enc-embed; 2,3 dec-embed; 4+4l+{0..3} encoder; 16+6l+{0..5} decoder
static inline int site_enc(int layer, int k) { return 4 + 4 * layer + k; }
static inline int site_dec(int layer, int k) { return 16 + 6 * layer + k; }

// ---- per-step weight images (dvs_wimg.h) ------------------------------------------------------------------------------
static inline size_t img_attn(int block) { return (size_t)block * DvsAttnImg::SIZE; }                       // 0..8
static inline size_t img_ffn(int block) { return DVS_N_ATTN_BLOCKS * DvsAttnImg::SIZE + (size_t)block * DvsFfnImg::SIZE; }   // 0..5
static inline int blk_enc_attn(int layer) { return layer; }
static inline int blk_dec_self(int layer) { return 3 + 2 * layer; }
static inline int blk_dec_cross(int layer) { return 4 + 2 * layer; }
static inline int blk_enc_ffn(int layer) { return layer; }
static inline int blk_dec_ffn(int layer) { return 3 + layer; }

static inline const void* wimg_attn(const Step& c, int block) { return (const dvs_bf16*)(c.ws + c.W.wimg) + img_attn(block); }
static inline const void* wimg_ffn(const Step& c, int block) { return (const dvs_bf16*)(c.ws + c.W.wimg) + img_ffn(block); }

// ---- argument blocks: one builder each, from the call context plus what varies -------------------------------------------
// LayerNorm of the sublayer (or embedding) that wrote `slot`, applied in its consumer's prologue; no norm: identity
static DvsLN ln_of(const Step& c, int slot, const DvsNormP* n) {
    if (!n) return DvsLN{nullptr, nullptr, nullptr};
    return DvsLN{c.ws + c.W.stats[slot], c.P + n->w, c.P + n->b};
}

// forward: the caller sets `out` (and out2 / site2); backward: gout, slab and the gradient offsets
static EmbedArgs embed_args(const Step& c, int site) {
    EmbedArgs e;
    memset(&e, 0, sizeof(e));
    e.dims = c.d;
    e.rec = c.rec;
    e.W1 = c.P + c.L.W1;
    e.W2 = c.P + c.L.W2;
    e.lab_w = c.P + c.L.lab_w;
    e.lab_b = c.P + c.L.lab_b;
    e.embimg = (const float*)((const dvs_bf16*)(c.ws + c.W.wimg) + DVS_WIMG_EMB);
    e.site = site;
    return e;
}

// in / out: activation slots; norm: LayerNorm of the producer of `in` (null: an embedding); kv: null = self-attention;
// dropout sites site0 (probabilities), site0 + 1 (output)
static AttnArgs attn_args(const Step& c, const DvsAttnP& p, int block, int in, const DvsNormP* norm, const float* kv, int out,
                          int site0) {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.dims = c.d;
    a.rec = c.rec;
    a.xin = c.ws + c.W.act[in];
    a.ln = ln_of(c, in, norm);
    a.kv = kv;
    a.in_w = c.P + p.in_w;
    a.in_b = c.P + p.in_b;
    a.out_w = c.P + p.out_w;
    a.out_b = c.P + p.out_b;
    a.wimg = wimg_attn(c, block);
    a.qkv = c.wide ? c.ws + c.W.qkv[block] : nullptr;      // parked for the backward
    a.out_pre = c.ws + c.W.act[out];
    a.out_stats = c.ws + c.W.stats[out];
    a.site_prob = site0;
    a.site_post = site0 + 1;
    return a;
}

// dropout sites site0 (hidden), site0 + 1 (output)
static FfnArgs ffn_args(const Step& c, const DvsFfnP& p, int block, int in, const DvsNormP& norm, int out, int site0) {
    FfnArgs f;
    memset(&f, 0, sizeof(f));
    f.dims = c.d;
    f.xin = c.ws + c.W.act[in];
    f.ln = ln_of(c, in, &norm);
    f.l1_w = c.P + p.l1_w;
    f.l1_b = c.P + p.l1_b;
    f.l2_w = c.P + p.l2_w;
    f.l2_b = c.P + p.l2_b;
    f.wimg = wimg_ffn(c, block);
    f.out_pre = c.ws + c.W.act[out];
    f.out_stats = c.ws + c.W.stats[out];
    f.site_hidden = site0;
    f.site_post = site0 + 1;
    return f;
}

static LatentArgs latent_args(const Step& c, const float* eps, bool with_mem) {
    LatentArgs a;
    memset(&a, 0, sizeof(a));
    a.dims = c.d;
    a.xenc = c.ws + c.W.enc_out;
    a.fc1_w = c.P + c.L.fc1_w;
    a.fc1_b = c.P + c.L.fc1_b;
    a.fc2_w = c.P + c.L.fc2_w;
    a.fc2_b = c.P + c.L.fc2_b;
    a.fc3_w = c.P + c.L.fc3_w;
    a.fc3_b = c.P + c.L.fc3_b;
    a.limg = c.ws + c.W.limg;
    a.eps_in = eps;
    a.mu = c.ws + c.W.mu;
    a.logvar = c.ws + c.W.logvar;
    a.z = c.ws + c.W.z;
    a.epsv = c.ws + c.W.epsv;
    a.mem = with_mem ? c.ws + c.W.mem : nullptr;
    a.dag_loss = c.ws + c.W.dag_loss;
    return a;
}

// add_node / add_edge parameters as LossArgs, DecodeArgs and the head block of the weight images (DvsLossHeadArgs) name them
template <class A>
static void head_params(const Step& c, A& a) {
    a.node0_w = c.P + c.L.node0_w;
    a.node0_b = c.P + c.L.node0_b;
    a.node2_w = c.P + c.L.node2_w;
    a.node2_b = c.P + c.L.node2_b;
    a.edge0_b = c.P + c.L.edge0_b;
    a.edge2_w = c.P + c.L.edge2_w;
    a.edge2_b = c.P + c.L.edge2_b;
}
// ... and the head's input for the kernels that run it (LossArgs, DecodeArgs): the last decoder sublayer under its LayerNorm
template <class A>
static void head_input(const Step& c, A& a) {
    const int last = slot_dec(DVS_LAYERS - 1, 2);
    a.xin = c.ws + c.W.act[last];
    a.ln = ln_of(c, last, &c.L.dec[DVS_LAYERS - 1].n3);
    a.edge0_w = c.P + c.L.edge0_w;
    head_params(c, a);
}

static LossArgs loss_args(const Step& c) {
    LossArgs a;
    memset(&a, 0, sizeof(a));
    a.dims = c.d;
    a.rec = c.rec;
    head_input(c, a);
    a.wimg = (const dvs_bf16*)(c.ws + c.W.wimg) + DVS_WIMG_LOSS;
    a.dag_loss = c.ws + c.W.dag_loss;
    return a;
}

static void prepare_images(const Step& c) {
    const DvsLayout& L = c.L;
    const bool wide = c.wide;
    DvsImgJobs J;
    J.count = 0;
    auto add = [&](int64_t src, size_t dst, int rows, int flags) {
        DvsImgJob& j = J.job[J.count++];
        j.src = src;
        j.dst = (int64_t)dst;
        j.rows = rows;
        j.flags = flags;
    };
    auto attn = [&](const DvsAttnP& p, int block) {
        const size_t b = img_attn(block);
        // the one-tile kernels keep q, k, v in head-aligned slot order (dvs_pi: in-projection rows / out-projection columns
        // permuted); the wide kernels (k_wide_fwd.hip) use parameter order
        add(p.in_w, b + DvsAttnImg::Win, 192, wide ? 0 : 2);             // x6
        add(p.out_w, b + DvsAttnImg::Wout, 64, wide ? 0 : 4);            // x6
        add(p.out_w, b + DvsAttnImg::WoutT, 64, 1 | (wide ? 0 : 4));     // x3 transposed
        add(p.in_w, b + DvsAttnImg::WinB, 192, 16 | (wide ? 0 : 2));     // parts hi, mid again, behind WoutT
        for (int q = 0; q < 3; ++q)                                    // W_q^T, W_k^T, W_v^T for k_proj_bwd
            add(p.in_w + 4096 * q, b + DvsAttnImg::WinT + (size_t)q * 2 * DVS_IMG64, 64, 1 | (wide ? 0 : 2));
    };
    auto ffn = [&](const DvsFfnP& p, int block) {
        const size_t b = img_ffn(block);
        add(p.l1_w, b + DvsFfnImg::W1, 64, 0);
        add(p.l2_w, b + DvsFfnImg::W2, 64, 0);
        add(p.l2_w, b + DvsFfnImg::W2T, 64, 1);
        add(p.l1_w, b + DvsFfnImg::W1T, 64, 1);
    };
    for (int i = 0; i < DVS_LAYERS; ++i) {
        attn(L.enc[i].sa, blk_enc_attn(i));
        ffn(L.enc[i].ff, blk_enc_ffn(i));
        attn(L.dec[i].sa, blk_dec_self(i));
        attn(L.dec[i].ca, blk_dec_cross(i));
        ffn(L.dec[i].ff, blk_dec_ffn(i));
    }
    if (!wide) {                 // loss head (one-tile kernels): the two halves of add_edge.0.weight [64][128]
        add(L.edge0_w, DVS_WIMG_LOSS + DvsLossImg::Wa, 64, 8);
        add(L.edge0_w + 64, DVS_WIMG_LOSS + DvsLossImg::Wb, 64, 8);
        add(L.edge0_w, DVS_WIMG_LOSS + DvsLossImg::WaT, 64, 8 | 1);
        add(L.edge0_w + 64, DVS_WIMG_LOSS + DvsLossImg::WbT, 64, 8 | 1);
    }
    dvs_bf16* wimg = (dvs_bf16*)(c.ws + c.W.wimg);
    DvsLatImgArgs lat;
    lat.fc1_w = c.P + L.fc1_w;
    lat.fc2_w = c.P + L.fc2_w;
    lat.fc3_w = c.P + L.fc3_w;
    lat.fc3_b = c.P + L.fc3_b;
    lat.img = c.ws + c.W.limg;
    lat.N = c.d.N;
    lat.NT = c.d.NT;
    DvsLossHeadArgs head;
    memset(&head, 0, sizeof(head));
    if (!wide) {
        head_params(c, head);
        head.ln_g = c.P + L.dec[DVS_LAYERS - 1].n3.w;
        head.ln_b = c.P + L.dec[DVS_LAYERS - 1].n3.b;
        head.dst = (float*)(wimg + DVS_WIMG_LOSS + DvsLossImg::Head);
        head.C = c.d.C;
        head.W1 = c.P + L.W1;
        head.W2 = c.P + L.W2;
        head.lab_w = c.P + L.lab_w;
        head.lab_b = c.P + L.lab_b;
        head.dst_emb = (float*)(wimg + DVS_WIMG_EMB);
        head.N = c.d.N;
    }
    dvs_launch_prepare_images(J, c.P, wimg, lat, head, c.st);
}

// ---- forward launcher by (wide, nw): the wide kernels; the narrow mapping (4 waves, the chain's grid); the 8-wave mapping ----
static void launch_embed_fwd(const Step& c, const EmbedArgs& e) {
    if (c.wide) dvs_launch_embed_fwd_w(e, c.g.tiles4, c.st);
    else if (c.nw == 4) dvs_launch_embed_fwd(e, c.g.chain, 4, c.st);
    else dvs_launch_embed_fwd(e, c.g.tiles16, 16, c.st);
}
static void launch_attn_fwd(const Step& c, const AttnArgs& a) {
    if (c.wide) dvs_launch_attn_fwd_w(a, c.g.dags, c.st);
    else if (c.nw == 4) dvs_launch_attn_fwd(a, c.g.chain, 4, c.st);
    else dvs_launch_attn_fwd(a, c.g.tiles8, 8, c.st);
}
static void launch_ffn_fwd(const Step& c, const FfnArgs& f) {      // token-local: one kernel serves both paths
    if (c.nw == 4) dvs_launch_ffn_fwd(f, c.g.chain, 4, c.st);
    else dvs_launch_ffn_fwd(f, c.g.tiles16, 16, c.st);
}
static void launch_loss_fwd(const Step& c, const LossArgs& a) {
    if (c.wide) dvs_launch_loss_fwd_w(a, c.g.dags2, c.st);
    else if (c.nw == 4) dvs_launch_loss_fwd(a, c.g.chain, 4, c.st);
    else dvs_launch_loss_fwd(a, c.g.tiles8, 8, c.st);
}
// One-tile path: the sublayers of the encoder / decoder are chained into one launch each (k_fwd_stack); the wide path and
// DVS_SPLIT_STACK=1 launch every sublayer on its own.
struct FwdChain {
    FwdStackArgs stack;
    const Step& c;
    int tag;
    bool chain;
    FwdChain(const Step& step, int tag_) : c(step), tag(tag_), chain(!step.wide && !split_stack()) { memset(&stack, 0, sizeof(stack)); }
    FwdPhase& next(int kind) {
        if (stack.nphase == DVS_FWD_STACK_PHASES) flush();
        FwdPhase& ph = stack.ph[stack.nphase++];
        ph.kind = kind;
        return ph;
    }
    void attn(const AttnArgs& a) {
        if (chain) next(DVS_FPH_ATTN).u.a = a;
        else launch_attn_fwd(c, a);
    }
    void ffn(const FfnArgs& f) {
        if (chain) next(DVS_FPH_FFN).u.f = f;
        else launch_ffn_fwd(c, f);
    }
    // the latent block as the last phase of the encoder chain (the workgroups of the chain own 16 DAGs each: one MFMA
    // group); false: not chained, the caller launches k_latent_fwd
    bool latent(const LatentArgs& l) {
        if (!latent_in_chain(chain, c.nw) || stack.nphase == 0 || stack.nphase == DVS_FWD_STACK_PHASES) return false;
        next(DVS_FPH_LATENT).u.l = l;
        return true;
    }
    void flush() {
        if (stack.nphase > 0) dvs_launch_fwd_stack(stack, tag, c.g.chain, c.nw, c.st);
        stack.nphase = 0;
    }
};

// dec_embed: also write the decoder-side embedding (slot 7, dropout sites 2 / 3) from the same launch (one-tile path)
// lat: the latent block's arguments; it runs as the last phase of the encoder chain when there is one, as k_latent_fwd otherwise
// save_qkv: the wide attention kernels park q, k, v for the backward
static void encoder_forward(const Step& c, const LatentArgs& lat, bool dec_embed = false, bool save_qkv = false) {
    EmbedArgs e = embed_args(c, 0);
    e.out = c.ws + c.W.act[0];
    if (dec_embed) {
        e.out2 = c.ws + c.W.act[7];
        e.site2 = 2;
    }
    launch_embed_fwd(c, e);
    FwdChain chain(c, 0);
    const DvsNormP* norm = nullptr;
    int prev = 0;
    for (int i = 0; i < DVS_LAYERS; ++i) {
        const auto& pl = c.L.enc[i];
        const int sa = slot_enc(i, 0), sf = slot_enc(i, 1);
        AttnArgs a = attn_args(c, pl.sa, blk_enc_attn(i), prev, norm, nullptr, sa, site_enc(i, 0));
        if (!save_qkv) a.qkv = nullptr;
        chain.attn(a);
        FfnArgs f = ffn_args(c, pl.ff, blk_enc_ffn(i), sa, pl.n1, sf, site_enc(i, 2));
        if (i == DVS_LAYERS - 1) {
            f.out_norm = c.ws + c.W.enc_out;
            f.ng = c.P + pl.n2.w;
            f.nb = c.P + pl.n2.b;
        }
        chain.ffn(f);
        norm = &pl.n2;
        prev = sf;
    }
    const bool fused = chain.latent(lat);
    chain.flush();
    if (!fused) dvs_launch_latent_fwd(lat, c.st);
}

// TransformerDecoder forward (pace.py:163-182) from the embedding in slot `dec_in`; memory = W.mem.
static void decoder_forward(const Step& c, int dec_in) {
    FwdChain chain(c, 1);
    const DvsNormP* norm = nullptr;
    int prev = dec_in;
    for (int i = 0; i < DVS_LAYERS; ++i) {
        const auto& pl = c.L.dec[i];
        const int s0 = slot_dec(i, 0), s1 = slot_dec(i, 1), s2 = slot_dec(i, 2);
        chain.attn(attn_args(c, pl.sa, blk_dec_self(i), prev, norm, nullptr, s0, site_dec(i, 0)));
        chain.attn(attn_args(c, pl.ca, blk_dec_cross(i), s0, &pl.n1, c.ws + c.W.mem, s1, site_dec(i, 2)));
        chain.ffn(ffn_args(c, pl.ff, blk_dec_ffn(i), s1, pl.n2, s2, site_dec(i, 4)));
        norm = &pl.n3;
        prev = s2;
    }
    chain.flush();
}

// images, encoder (+ latent block), decoder: the forward up to the loss head; then the optional mu / logvar copies
static void forward_to_decoder(const Step& c, const float* eps) {
    prepare_images(c);
    // decoder input embedding: identical to the encoder's in eval mode / dropout 0 (pace.py:2000-2012 recomputes it only to
    // redraw the dropout masks); under dropout the encoder's embedding launch writes it as well (slot 7)
    encoder_forward(c, latent_args(c, eps, true), c.d.drop.on, true);
    decoder_forward(c, c.d.drop.on ? 7 : 0);
}
static void copy_out_latent(const Step& c, float* mu, float* logvar) {
    const size_t nb = (size_t)c.d.B * 32 * sizeof(float);
    if (mu) copy_out(mu, c.ws + c.W.mu, nb, c.st);
    if (logvar) copy_out(logvar, c.ws + c.W.logvar, nb, c.st);
}
static FinalizeArgs finalize_args(const Step& c, int32_t* status, float* losses, void* host_tail, uint32_t host_seq) {
    FinalizeArgs fa;
    fa.B = c.d.B;
    fa.beta = c.d.beta;
    fa.dag_loss = c.ws + c.W.dag_loss;
    fa.status = status;
    fa.losses = losses;
    fa.host_tail = (float*)host_tail;
    fa.host_seq = host_seq;
    return fa;
}

extern "C" int dvs_loss_forward(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                                int64_t n_params, void* workspace, size_t workspace_bytes, const float* eps,
                                const int32_t* status, float* losses, float* mu, float* logvar, void* stream) {
    return dvs_loss_forward_notify(s, records, records_bytes, params, n_params, workspace, workspace_bytes, eps,
                                   (int32_t*)status, losses, mu, logvar, nullptr, 0u, stream);     // no host_tail: status is only read
}

extern "C" int dvs_loss_forward_notify(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                                       int64_t n_params, void* workspace, size_t workspace_bytes, const float* eps,
                                       int32_t* status, float* losses, float* mu, float* logvar, void* host_tail,
                                       uint32_t host_seq, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!records || !params || !workspace || !losses) return fail(10, "dvs_loss_forward: null pointer");
    const Step c = make_step(s, records, params, workspace, stream);
    if (int e = check_buffers(c, "dvs_loss_forward", records_bytes, n_params, workspace_bytes)) return e;
    call_begin();
    forward_to_decoder(c, eps);
    launch_loss_fwd(c, loss_args(c));
    dvs_launch_finalize(finalize_args(c, status, losses, host_tail, host_seq), c.st);
    copy_out_latent(c, mu, logvar);
    return call_end("dvs_loss_forward");
}

extern "C" int dvs_loss_forward_defer(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                                      int64_t n_params, void* workspace, size_t workspace_bytes, const float* eps, float* mu,
                                      float* logvar, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!records || !params || !workspace) return fail(10, "dvs_loss_forward_defer: null pointer");
    const Step c = make_step(s, records, params, workspace, stream);
    if (int e = check_buffers(c, "dvs_loss_forward_defer", records_bytes, n_params, workspace_bytes)) return e;
    if (c.wide) return fail(13, "dvs_loss_forward_defer: one-tile path only (n_tokens, n_classes <= 16)");
    call_begin();
    forward_to_decoder(c, eps);
    copy_out_latent(c, mu, logvar);
    return call_end("dvs_loss_forward_defer");
}

extern "C" int dvs_encode(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                          int64_t n_params, void* workspace, size_t workspace_bytes, float* mu, float* logvar,
                          void* stream) {
    if (int e = check_shape(s)) return e;
    if (!records || !params || !workspace || !mu || !logvar) return fail(10, "dvs_encode: null pointer");
    const Step c = make_step(s, records, params, workspace, stream);
    if (int e = check_buffers(c, "dvs_encode", records_bytes, n_params, workspace_bytes)) return e;
    call_begin();
    prepare_images(c);
    LatentArgs la = latent_args(c, nullptr, false);
    la.dims.training = 0;
    encoder_forward(c, la);
    const size_t nb = (size_t)c.d.B * 32 * sizeof(float);
    copy_out(mu, c.ws + c.W.mu, nb, c.st);
    copy_out(logvar, c.ws + c.W.logvar, nb, c.st);
    return call_end("dvs_encode");
}

// ---- generation (k_decode.hip) -------------------------------------------------------------------------------------
extern "C" int dvs_decode(const dvs_shape* s, const float* params, int64_t n_params, void* workspace,
                          size_t workspace_bytes, void* records, size_t records_bytes, const float* z,
                          const float* uniforms, void* state_out, size_t state_bytes, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!params || !workspace || !records || !z || !state_out) return fail(10, "dvs_decode: null pointer");
    if (s->training) return fail(13, "dvs_decode: generation runs in eval mode (shape.training must be 0)");
    const Step c = make_step(s, records, params, workspace, stream);
    if (int e = check_buffers(c, "dvs_decode", records_bytes, n_params, workspace_bytes)) return e;
    if (state_bytes < (size_t)s->batch * sizeof(dvs_decode_state))
        return fail(14, "dvs_decode: state_bytes < batch * sizeof(dvs_decode_state)");
    call_begin();
    prepare_images(c);
    dvs_launch_decode_memory(c.d, z, c.P + c.L.fc3_w, c.P + c.L.fc3_b, c.ws + c.W.mem, c.st);
    DecodeArgs a;
    memset(&a, 0, sizeof(a));
    a.dims = c.d;
    a.wide = c.wide ? 1 : 0;
    a.rec = records;
    a.state = (DvsDecodeState*)state_out;
    head_input(c, a);
    a.uniforms = uniforms;
    dvs_launch_decode_init(a, c.st);
    EmbedArgs e = embed_args(c, 2);
    e.out = c.ws + c.W.act[7];
    for (int idx = 2; idx < c.d.N; ++idx) {
        launch_embed_fwd(c, e);
        decoder_forward(c, 7);
        a.idx = idx;
        dvs_launch_decode_step(a, c.g.dec4, c.st);
    }
    return call_end("dvs_decode");
}

extern "C" int dvs_debug_activation(const dvs_shape* s, const void* workspace, int slot, float* out, void* stream) {
    if (int e = check_shape(s)) return e;
    const Step c = make_step(s, nullptr, nullptr, (void*)workspace, stream);
    const float* ws = c.ws;
    const DvsWorkspace& W = c.W;
    const float* src = nullptr;
    if (slot >= 0 && slot < DVS_NSLOTS) src = ws + W.act[slot];
    else if (slot == 100) src = ws + W.enc_out;
    else if (slot == 101) src = ws + W.mem;
    else if (slot == 102) src = ws + W.gA;
    else if (slot == 103) src = ws + W.gB;
    else if (slot == 104) src = ws + W.gmem;
    else if (slot == 105) src = ws + W.genc;
    else return fail(11, "dvs_debug_activation: bad slot");
    call_begin();
    dvs_launch_unfrag(src, out, c.d.B * c.d.NT, c.st);
    return call_end("dvs_debug_activation");
}

extern "C" int dvs_debug_dag_losses(const dvs_shape* s, const void* workspace, float* out, void* stream) {
    if (int e = check_shape(s)) return e;
    if (!workspace || !out) return fail(10, "dvs_debug_dag_losses: null pointer");
    const Step c = make_step(s, nullptr, nullptr, (void*)workspace, stream);
    call_begin();
    copy_out(out, c.ws + c.W.dag_loss, (size_t)c.d.B * 2 * sizeof(float), c.st);
    return call_end("dvs_debug_dag_losses");
}

// Error-path test hook (include/dvs.h): an empty kernel through the product's launch macro.
__global__ void k_debug_empty(int* sink) {
    DVS_DYN_LDS(smem);
    if (sink && threadIdx.x == 1u << 20) *sink = smem[0];
}
extern "C" int dvs_debug_launch(size_t dynamic_lds_bytes, void* stream) {
    call_begin();
    DVS_LAUNCH(k_debug_empty, dim3(1), dim3(64), dynamic_lds_bytes, (dvs_stream_t)stream, (int*)nullptr);
    return call_end("dvs_debug_launch");
}

#include "dvs_api_backward.inc"
#include "dvs_api_search.inc"
