// Wide path (17..48 tokens per DAG), forward kernels: records, embedding, attention sublayer, loss head.
// See dvs_wide.h for the execution model (workgroup = DAG, wave = 16-token tile, tiles meet in LDS).
#include "dvs_wide.h"
#include "dvs_wimg.h"

// ---------------------------------------------------------------------------------------------------------
// dvs_pack_features, wide records.  Same checks as k_pack (k_forward.hip).  One workgroup per DAG: its label / position /
// adjacency rows and its 8 per-head mask copies are four CONTIGUOUS byte ranges of the batched feature tensors (32 KB at
// N = C = 40), streamed into LDS with whole-wave loads — 16 bytes per lane where the range is 16-byte aligned, 4 bytes
// otherwise (odd N*C) —, then one thread per token builds its record fields from LDS and all threads compare the mask copies.
// (Round 2's one-thread-per-token version walked the rows straight from global memory with per-lane strides of N*C floats:
// 107 us for 65 MB at B = 2048, a tenth of the HBM rate with 88 % of the wave cycles waiting.)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void packw_stream(char* dst, const char* __restrict__ src, int nbytes) {      // nbytes % 4 == 0
    const int tid = threadIdx.x, step = blockDim.x;
    if (((uintptr_t)src & 15) == 0 && (nbytes & 15) == 0) {
        const int n = nbytes >> 4;
        int i = tid;
        for (; i + 3 * step < n; i += 4 * step) {               // four 16-byte loads in flight per lane
            f4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const f4*)(src + 16 * (size_t)(i + u * step));
#pragma unroll
            for (int u = 0; u < 4; ++u) *(f4*)(dst + 16 * (size_t)(i + u * step)) = v[u];
        }
        for (; i < n; i += step) *(f4*)(dst + 16 * (size_t)i) = *(const f4*)(src + 16 * (size_t)i);
        return;
    }
    const int n = nbytes >> 2;
    int i = tid;
    for (; i + 7 * step < n; i += 8 * step) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *(const float*)(src + 4 * (size_t)(i + u * step));
#pragma unroll
        for (int u = 0; u < 8; ++u) *(float*)(dst + 4 * (size_t)(i + u * step)) = v[u];
    }
    for (; i < n; i += step) *(float*)(dst + 4 * (size_t)i) = *(const float*)(src + 4 * (size_t)i);
}
static size_t packw_lds_bytes(int N, int C) {
    const size_t r16 = 15;
    return (((size_t)N * C * 4 + r16) & ~r16) + 2 * (((size_t)N * N * 4 + r16) & ~r16) + (((size_t)8 * N * N + r16) & ~r16);
}
__global__ __launch_bounds__(256) void k_pack_w(PackArgs a) {
    DVS_DYN_LDS(smem);
    const int N = a.N, C = a.C;
    const int dag = (int)blockIdx.x;
    const size_t nlab = ((size_t)N * C * 4 + 15) & ~(size_t)15, nsq = ((size_t)N * N * 4 + 15) & ~(size_t)15;
    float* s_lab = (float*)smem;                       // [N][C]
    float* s_pos = (float*)(smem + nlab);              // [N][N]
    float* s_adj = (float*)(smem + nlab + nsq);        // [N][N]
    uint8_t* s_msk = (uint8_t*)(smem + nlab + 2 * nsq);   // [8][N][N]
    packw_stream((char*)s_lab, (const char*)(a.lab1h + (size_t)dag * N * C), N * C * 4);
    packw_stream((char*)s_pos, (const char*)(a.pos1h + (size_t)dag * N * N), N * N * 4);
    packw_stream((char*)s_adj, (const char*)(a.adj + (size_t)dag * N * N), N * N * 4);
    packw_stream((char*)s_msk, (const char*)(a.tmask + (size_t)dag * 8 * N * N), 8 * N * N);      // 8 N^2 bytes: a multiple of 4
    __syncthreads();
    int bad = 0;
    // heads 1..7 against head 0, all threads: (h, i, j) flattened
    const int per = N * N;
    for (int e = threadIdx.x; e < 7 * per; e += blockDim.x) {
        const int ij = e % per;
        if ((s_msk[per + e] != 0) != (s_msk[ij] != 0)) bad |= 2;
    }
    const int i = threadIdx.x;
    if (i < DVS_WTOK) {
        int label = 0, pos = 0;
        uint64_t parents = 0, allowed = 1ull << i;
        if (i < N) {
            const float* lr = s_lab + (size_t)i * C;
            int ones = 0;
            for (int c = 0; c < C; ++c) {
                const float v = lr[c];
                if (v == 1.0f) { label = c; ++ones; } else if (v != 0.0f) bad |= 1;
            }
            if (ones != 1) bad |= 1;
            const float* pr = s_pos + (size_t)i * N;
            ones = 0;
            for (int c = 0; c < N; ++c) {
                const float v = pr[c];
                if (v == 1.0f) { pos = c; ++ones; } else if (v != 0.0f) bad |= 1;
            }
            if (ones != 1) bad |= 1;
            for (int j = 0; j < N; ++j)
                if (s_adj[j * N + i] != 0.0f) parents |= 1ull << j;
            allowed = 0;
            const uint8_t* m0 = s_msk + (size_t)i * N;
            for (int j = 0; j < N; ++j)
                if (!m0[j]) allowed |= 1ull << j;
            if (!((allowed >> i) & 1ull)) bad |= 4;
        }
        DvsRecordW* r = (DvsRecordW*)a.rec + dag;
        r->label[i] = (uint8_t)label;
        r->pos[i] = (uint8_t)pos;
        r->parents[i] = parents;
        r->allowed[i] = allowed;
    }
    if (bad) atomicOr(a.status, bad);
}

void dvs_launch_pack_w(const PackArgs& a, dvs_stream_t st) {
    const size_t lds = packw_lds_bytes(a.N, a.C);
    DVS_SET_LDS(k_pack_w, lds);
    DVS_LAUNCH(k_pack_w, dim3((unsigned)a.B), dim3(256), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// dvs_build_records, wide: row codec -> records, one thread per DAG on 64-bit rows (k_build_records restated for
// N <= 48; same PACE wrapping pace.py:1250-1288, FIFO-Kahn positions with the positions[v] = order[v] quirk
// pace.py:1245-1248/1286, ancestor closure pace.py:1307-1343).
// ---------------------------------------------------------------------------------------------------------
constexpr int BW_T = 64;
__global__ __launch_bounds__(BW_T) void k_build_records_w(BuildWArgs a) {
    __shared__ uint64_t s_child[DVS_WTOK][BW_T];
    __shared__ uint64_t s_reach[DVS_WTOK][BW_T];
    __shared__ unsigned char s_indeg[DVS_WTOK][BW_T];
    __shared__ unsigned char s_order[DVS_WTOK][BW_T];
    const int tid = threadIdx.x;
    const int dag = blockIdx.x * BW_T + tid;
    if (dag >= a.B) return;
    const int N = a.N, n = N - 3, out_id = N - 1;
    int bad = 0;
    for (int v = 0; v < DVS_WTOK; ++v) s_child[v][tid] = 0;
    s_child[0][tid] = 1ull << 1;
    uint64_t haspred = 0;
    for (int v = 0; v < n; ++v) {
        const uint64_t p = a.preds[(size_t)dag * n + v];
        if (p >> v) bad |= 8;                                   // an edge u -> v needs u < v
        const uint64_t pm = p & ((1ull << v) - 1ull);
        uint64_t c = pm;
        while (c) {
            const int u = dvs_ctz64(c);
            c &= c - 1;
            s_child[u + 2][tid] |= 1ull << (v + 2);
        }
        if (pm) haspred |= 1ull << v;
    }
    for (int v = 0; v < n; ++v)
        if (!((haspred >> v) & 1ull)) s_child[1][tid] |= 1ull << (v + 2);
    for (int v = 0; v < N - 1; ++v)
        if (s_child[v][tid] == 0) s_child[v][tid] = 1ull << out_id;
    for (int v = 0; v < DVS_WTOK; ++v) s_indeg[v][tid] = 0;
    for (int u = 0; u < N; ++u) {
        uint64_t c = s_child[u][tid];
        while (c) {
            const int v = dvs_ctz64(c);
            c &= c - 1;
            s_indeg[v][tid]++;
        }
    }
    int tail = 0;
    for (int v = 0; v < N; ++v)
        if (s_indeg[v][tid] == 0) s_order[tail++][tid] = (unsigned char)v;
    for (int head = 0; head < tail && head < N; ++head) {
        uint64_t c = s_child[s_order[head][tid]][tid];
        while (c) {
            const int v = dvs_ctz64(c);
            c &= c - 1;
            if (--s_indeg[v][tid] == 0 && tail < DVS_WTOK) s_order[tail++][tid] = (unsigned char)v;
        }
    }
    if (tail != N) bad |= 8;
    for (int v = 0; v < N; ++v) s_reach[v][tid] = s_child[v][tid] | (1ull << v);
    for (int k = 0; k < N; ++k) {
        const uint64_t rk = s_reach[k][tid];
        for (int v = 0; v < N; ++v)
            if ((s_reach[v][tid] >> k) & 1ull) s_reach[v][tid] |= rk;
    }
    DvsRecordW* r = a.rec + dag;
    for (int i = 0; i < DVS_WTOK; ++i) {
        int label = 0, pos = 0;
        uint64_t parents = 0, allowed = 1ull << i;
        if (i < N) {
            if (i == 0) label = 2;
            else if (i == 1) label = 0;
            else if (i == out_id) label = 1;
            else {
                label = a.labels[(size_t)dag * n + (i - 2)] + 3;
                if (label >= a.C) { bad |= 1; label = 0; }
            }
            pos = s_order[i][tid];
            allowed = 0;
            for (int j = 0; j < N; ++j) {
                if ((s_child[j][tid] >> i) & 1ull) parents |= 1ull << j;
                if ((s_reach[j][tid] >> i) & 1ull) allowed |= 1ull << j;
            }
        }
        r->label[i] = (uint8_t)label;
        r->pos[i] = (uint8_t)pos;
        r->parents[i] = parents;
        r->allowed[i] = allowed;
    }
    if (bad) atomicOr(a.status, bad);
}

void dvs_launch_build_records_w(const BuildWArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_build_records_w, dim3((a.B + BW_T - 1) / BW_T), dim3(BW_T), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Embedding forward (pace.py:201-221, 1181-1184, 1624-1630), wide.  Token-parallel: a wave owns one tile; the hidden
// of the positional encoder is an LDS GATHER over the token's parent bit-row:
//   e1[i] = relu(W1[pos_i] + sum_{j in parents(i)} W1[N + pos_j])
// (the one-tile kernel does the same with selector-matrix MFMAs; with up to 48 positions the gather is cheaper).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_embed_fwd_w(EmbedArgs a) {
    DVS_DYN_LDS(smem);
    const EmbWLds l = embw_lds(smem);
    embw_stage(l, a);
    __syncthreads();
    const Lane L = dvs_lane();
    const DvsDrop D = dvs_drop_of(a.dims);
    const int N = a.dims.N;
    const int ntiles = a.dims.B * a.dims.NT;
    for (int tile = blockIdx.x * L.nwaves + L.wave; tile < ntiles; tile += gridDim.x * L.nwaves) {
        const DvsTile T = dvs_tile_of(tile, a.dims);
        const DvsRecordW* rec = (const DvsRecordW*)a.rec + T.dag;
        const bool valid = L.r < T.Nl;
        f4 e1h[4];
        embw_hidden(e1h, l.W1, rec, l.posl + 16 * L.wave, N, T.tok0, T.Nl, L);
        const uint32_t gdag = a.dims.dag_offset + T.dag;
        const int label = rec->label[valid ? T.tok0 + L.r : 0];
        f4 x[4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int f = 16 * t + 4 * L.g + kk;
                x[t][kk] = valid ? fmaxf(l.labw[f * EMBW_LABLD + label] + l.labb[f], 0.f) : 0.f;
            }
        // the encoder-side embedding and, when asked for (out2: the decoder-side one, other dropout sites), a second one from the
        // same parent walk (as the one-tile kernel does; it was a second launch)
        for (int rep = 0; rep < (a.out2 ? 2 : 1); ++rep) {
            const int site = rep == 0 ? a.site : a.site2;
            f4 e1[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) e1[t] = e1h[t];
            dvs_dropout_tile(e1, dvs_site_key(a.dims.seed_lo, a.dims.seed_hi, site, gdag), D, L, T.tok0);
            f4 e2[2] = {f4_zero(), f4_zero()};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f4 w0 = dvs_wcol(l.W2, EMB_LDW2, 0, t, L), w1 = dvs_wcol(l.W2, EMB_LDW2, 16, t, L);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    e2[0] = dvs_mfma(w0[kk], e1[t][kk], e2[0]);
                    e2[1] = dvs_mfma(w1[kk], e1[t][kk], e2[1]);
                }
            }
            dvs_dropout_tile<2>(e2, dvs_site_key(a.dims.seed_lo, a.dims.seed_hi, site + 1, gdag), D, L, T.tok0);
            x[2] = valid ? e2[0] : f4_zero();
            x[3] = valid ? e2[1] : f4_zero();
            dvs_store_tile(rep == 0 ? a.out : a.out2, tile, x, L);
        }
    }
}

void dvs_launch_embed_fwd_w(const EmbedArgs& a, int grid, dvs_stream_t st) {
    const size_t lds = EMBW_FLOATS * 4;
    DVS_SET_LDS(k_embed_fwd_w, lds);
    DVS_LAUNCH(k_embed_fwd_w, dim3(grid), dim3(256), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Attention sublayer forward, wide (same math as k_attn_fwd: pace.py:52-56 / 144 / 148), one workgroup (8 waves) per DAG.
//   stage 1  waves 0 .. 2 NT - 1: wave (tile w, half) computes half of the packed in-projection rows of tile w — q and
//            k[0:32] (half 0) or k[32:64] and v (half 1) — with the narrow path's fp32-accurate bf16x6 products from the
//            per-step weight images (dvs_wimg.h), and parks them row-major in LDS (Q pre-scaled by 1/sqrt(dh))  | barrier
//   stage 2  wave h = head h: for every query tile it the scores S^T[key][query] of the NT key tiles (2 MFMAs each, K = the
//            8 features of the head), the ancestor mask from the query's bit-row, softmax over up to 48 keys (in-lane + two
//            shuffles), dropout, O^T = V^T P^T (4 MFMAs per key tile on the 16 features of the head PAIR; the 8 rows of
//            the other head are discarded) written over the head's own slice of Q                                | barrier
//   stage 3  wave w < NT: y = Wo O + bo (bf16x6), dropout, residual, LayerNorm statistics, store                 | barrier
// Round 1 ran the core as a VALU walk of every (token, head) bit-row (15 k of the kernel's 24 k cycles per DAG) and the
// projections as exact-fp32 MFMAs on 3 of the 8 waves (8 k cycles).
// ---------------------------------------------------------------------------------------------------------
struct AttnWLds {
    dvs_bf16 *Win, *Wout;        // bf16x6 image triples, rows / columns in PARAMETER order (no head-slot permutation here)
    float *inb, *outb, *lg, *lb, *Q, *K, *V;       // O overwrites Q (every (token, head) slice is read before it is written)
    uint64_t* rows;              // [48]: ancestor bit-rows of the current DAG (0 for padding tokens)
};
__device__ __forceinline__ AttnWLds attnw_lds(char* smem) {
    AttnWLds l;
    l.Win = (dvs_bf16*)smem;
    l.Wout = l.Win + 3 * 192 * DVS_LDB;
    l.inb = (float*)(l.Wout + 3 * 64 * DVS_LDB);
    l.outb = l.inb + 192;
    l.lg = l.outb + 64;
    l.lb = l.lg + 64;
    l.Q = l.lb + 64;
    l.K = l.Q + DVS_WSCR;
    l.V = l.K + DVS_WSCR;
    l.rows = (uint64_t*)(l.V + DVS_WSCR);        // byte offset is a multiple of 8
    return l;
}
constexpr size_t ATTNW_BYTES = 3 * 256 * DVS_LDB * sizeof(dvs_bf16) + (192 + 64 + 128 + 3 * (size_t)DVS_WSCR) * 4 + DVS_WTOK * 8;


#ifdef DVS_STAMPS
DVS_ACC_STAMP_DECL(dvs_stamps_w);
DVS_STAMP_READER(w)
#endif
#define WSTAMP(k) DVS_ACC_STAMP(dvs_stamps_w, wst_, k)

__global__ __launch_bounds__(512) void k_attn_fwd_w(AttnArgs a) {
    DVS_DYN_LDS(smem);
    const AttnWLds l = attnw_lds(smem);
#ifdef DVS_STAMPS
    unsigned long long wst_ = __builtin_amdgcn_s_memtime();
#endif
    dvs_copy_image(l.Win, (const dvs_bf16*)a.wimg + DvsAttnImg::Win, (int)(DvsAttnImg::WoutT - DvsAttnImg::Win));
    dvs_stage_vector(l.inb, a.in_b, 192);
    dvs_stage_vector(l.outb, a.out_b, 64);
    if (a.ln.stats) {
        dvs_stage_vector(l.lg, a.ln.g, 64);
        dvs_stage_vector(l.lb, a.ln.b, 64);
    }
    for (int i = threadIdx.x; i < 3 * DVS_WSCR; i += blockDim.x) l.Q[i] = 0.f;
    __syncthreads();
    WSTAMP(0);
    const Lane L = dvs_lane();
    const DvsDrop D = dvs_drop_of(a.dims);
    const int N = a.dims.N, NT = a.dims.NT, NTOK = 16 * NT;
    const float scale = 0.35355339059327373f;   // 1/sqrt(8)
    const int pw = L.wave >> 1, phalf = L.wave & 1;              // stage 1: (tile, half of the in-projection rows)
    const bool proj = L.wave < 2 * NT;
    const int h = L.wave, hp = h >> 1, c0 = 8 * h;               // stage 2: head of this wave
    const bool mine = (L.g >> 1) == (h & 1);                     // rows 4g.. of a head-pair tile that belong to head h
    const bool has_tile = L.wave < NT;                           // stage 3: tile of this wave
    const int tok0 = 16 * L.wave, Nl = dvs_rows_of(N, L.wave);
    for (int dag = blockIdx.x; dag < a.dims.B; dag += gridDim.x) {
        const DvsRecordW* rec = (const DvsRecordW*)a.rec + dag;
        const uint32_t gdag = a.dims.dag_offset + dag;
        if (threadIdx.x >= 448 && threadIdx.x < 448 + DVS_WTOK) {     // wave 7 has no projection work: it fetches the rows
            const int i = threadIdx.x - 448;
            l.rows[i] = i < N ? rec->allowed[i] : 0ull;
        }
        // ---- stage 1 ------------------------------------------------------------------------------------------------
        if (proj) {
            const size_t tile = (size_t)dag * NT + pw;
            const int ptok0 = 16 * pw, pNl = dvs_rows_of(N, pw);
            f4 x[4], kv[4], dummy[4];
            float rstd;
            dvs_load_x<false>(x, dummy, rstd, a.xin, a.ln, l.lg, l.lb, tile, pNl, L);
            if (a.kv) {
                dvs_load_tile(kv, a.kv, tile, L);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) kv[t] = x[t];
            }
            const Split3T kvs = dvs_split3_T(kv);
            if (phalf == 0) {
                f4 q[4], k01[2];
#pragma unroll
                for (int t = 0; t < 4; ++t) q[t] = dvs_vecT(l.inb, t, L);
#pragma unroll
                for (int t = 0; t < 2; ++t) k01[t] = dvs_vecT(l.inb + 64, t, L);
                dvs_matb3<4>(q, dvs_split3_T(x), l.Win, 192, 0, L);
                dvs_matb3<2>(k01, kvs, l.Win, 192, 64, L);
#pragma unroll
                for (int t = 0; t < 4; ++t) dvs_park_col(l.Q, ptok0, t, q[t] * scale, L);
#pragma unroll
                for (int t = 0; t < 2; ++t) dvs_park_col(l.K, ptok0, t, k01[t], L);
                if (a.qkv) {          // the backward reads q, k, v back instead of recomputing them (k_attn_bwd_w): 1 KB per output tile
                    f4* sv = (f4*)(a.qkv + tile * 12 * 256) + L.lane;
#pragma unroll
                    for (int t = 0; t < 4; ++t) sv[t * 64] = q[t] * scale;
#pragma unroll
                    for (int t = 0; t < 2; ++t) sv[(4 + t) * 64] = k01[t];
                }
            } else {
                f4 k23[2], v[4];
#pragma unroll
                for (int t = 0; t < 2; ++t) k23[t] = dvs_vecT(l.inb + 96, t, L);
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = dvs_vecT(l.inb + 128, t, L);
                dvs_matb3<2>(k23, kvs, l.Win, 192, 96, L);
                dvs_matb3<4>(v, kvs, l.Win, 192, 128, L);
#pragma unroll
                for (int t = 0; t < 2; ++t) dvs_park_col(l.K, ptok0, 2 + t, k23[t], L);
#pragma unroll
                for (int t = 0; t < 4; ++t) dvs_park_col(l.V, ptok0, t, v[t], L);
                if (a.qkv) {
                    f4* sv = (f4*)(a.qkv + tile * 12 * 256) + L.lane;
#pragma unroll
                    for (int t = 0; t < 2; ++t) sv[(6 + t) * 64] = k23[t];
#pragma unroll
                    for (int t = 0; t < 4; ++t) sv[(8 + t) * 64] = v[t];
                }
            }
        }
        WSTAMP(1);
        __syncthreads();
        WSTAMP(2);
        // the residual input of stage 3: in flight while the core runs
        f4 x[4];
        if (has_tile) {
            f4 dummy[4];
            float rstd;
            dvs_load_x<false>(x, dummy, rstd, a.xin, a.ln, l.lg, l.lb, (size_t)dag * NT + L.wave, Nl, L);
        }
        // the projection waves touch their input tile(s) of the workgroup's NEXT DAG ahead of the core (one 4-byte load per lane:
        // every line of the tile; consumed behind the core): stage 1 opened with a cold load (4-7 k cycles on this machine).
        // Measured: k_attn_fwd_w 78.2 -> 76.6 us.  (Tried and dropped, `profiles/r03_ab_alarm1{6,8}.txt`: k / v of the next DAG
        // projected by the waves stage 3 leaves idle (+5 %: five waves need 7.9 k cycles for them, stage 3 lasts 3.6 k), stage 1
        // spread over all eight waves (no change: the stage is not bound by the output tiles per wave).)
        float tch0 = 0.f, tch1 = 0.f;
        if (proj && dag + (int)gridDim.x < a.dims.B) {
            const size_t nt = ((size_t)(dag + gridDim.x) * NT + pw) * 1024 + (size_t)L.lane * 16;
            tch0 = a.xin[nt];
            if (a.kv) tch1 = a.kv[nt];
        }
        // ---- stage 2: head h of every query tile ---------------------------------------------------------------------
        const uint32_t kprob = dvs_site_key(a.dims.seed_lo, a.dims.seed_hi, a.site_prob, gdag);
        // All NT query tiles in one unrolled pass: their chains (LDS reads -> 2 + 4 dependent MFMAs per key tile -> shuffles
        // of the softmax) are independent, and one tile alone leaves the wave waiting on every link (measured: the serial
        // version was no faster than round 1's VALU walk).
        // (query tile, key tile) pairs whose 16 x 16 block of the mask is empty are skipped — every pair above the diagonal for
        // DAGs in topological vertex order, more for sparse ones (bit 3 it + jt; k_attn_bwd_w's core does the same)
        uint32_t pairs = 0;
        {
            const uint64_t prow = L.lane < DVS_WTOK ? l.rows[L.lane] : 0ull;
#pragma unroll
            for (int jt = 0; jt < DVS_WNT; ++jt) {
                const unsigned long long b = __ballot(((prow >> (16 * jt)) & 0xFFFFull) != 0ull);
#pragma unroll
                for (int it = 0; it < DVS_WNT; ++it)
                    if ((b >> (16 * it)) & 0xFFFFull) pairs |= 1u << (3 * it + jt);
            }
        }
        float qb0[DVS_WNT], qb1[DVS_WNT];
        uint32_t okm[DVS_WNT][2];                                  // allowed bits of keys 4g.. + 16 jt: [0] jt = 0, 1; [1] jt = 2
        f4 s[DVS_WNT][DVS_WNT];
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) {
            const int i = 16 * (it < NT ? it : 0) + L.r;           // query of this lane (MFMA column)
            const uint64_t row = it < NT ? l.rows[i] : 0ull;
            okm[it][0] = (uint32_t)(row >> (4 * L.g));
            okm[it][1] = (uint32_t)(row >> (32 + 4 * L.g));
            qb0[it] = l.Q[i * DVS_LD + c0 + L.g];
            qb1[it] = l.Q[i * DVS_LD + c0 + 4 + L.g];
        }
#pragma unroll
        for (int jt = 0; jt < DVS_WNT; ++jt) {
            const float* kp = l.K + (16 * (jt < NT ? jt : 0) + L.r) * DVS_LD + c0 + L.g;
            const float ka0 = kp[0], ka1 = kp[4];
#pragma unroll
            for (int it = 0; it < DVS_WNT; ++it) {
                s[it][jt] = f4_zero();
                if ((pairs >> (3 * it + jt)) & 1u) {
                    s[it][jt] = dvs_mfma(ka0, qb0[it], s[it][jt]);
                    s[it][jt] = dvs_mfma(ka1, qb1[it], s[it][jt]);
                }
            }
        }
        // key j = 16 jt + 4g + reg is allowed iff bit j of the query's row is set
        float m[DVS_WNT], den[DVS_WNT];
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) {
            m[it] = -3.0e38f;
#pragma unroll
            for (int jt = 0; jt < DVS_WNT; ++jt) {
                if (!((pairs >> (3 * it + jt)) & 1u)) continue;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const bool ok = (okm[it][jt >> 1] >> (16 * (jt & 1) + reg)) & 1u;
                    m[it] = ok ? fmaxf(m[it], s[it][jt][reg]) : m[it];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) m[it] = dvs_max_x16(m[it]);
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) m[it] = dvs_max_x32(m[it]);
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) {
            den[it] = 0.f;
#pragma unroll
            for (int jt = 0; jt < DVS_WNT; ++jt) {
                if (!((pairs >> (3 * it + jt)) & 1u)) continue;         // s stays zero
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const bool ok = (okm[it][jt >> 1] >> (16 * (jt & 1) + reg)) & 1u;
                    s[it][jt][reg] = ok ? __expf(s[it][jt][reg] - m[it]) : 0.f;
                    den[it] += s[it][jt][reg];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) den[it] = dvs_add_x16(den[it]);
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) den[it] = dvs_add_x32(den[it]);
        f4 o[DVS_WNT];
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it) {
            o[it] = f4_zero();
            const float rden = den[it] > 0.f ? 1.0f / den[it] : 0.f;     // padding queries have no keys: all-zero rows
            const int i = 16 * it + L.r;
#pragma unroll
            for (int jt = 0; jt < DVS_WNT; ++jt) {
                if (!((pairs >> (3 * it + jt)) & 1u)) continue;
                s[it][jt] *= rden;
                if (D.on) {   // element (h, i, j): index (h NTOK + i) NTOK + j, two per draw (dvs_dropout_elem)
                    const uint32_t p0 = (uint32_t)((h * NTOK + i) * NTOK + 16 * jt + 4 * L.g) >> 1;
                    const uint32_t h0 = dvs_draw(kprob, p0), h1 = dvs_draw(kprob, p0 + 1);
                    s[it][jt][0] = ((h0 & 0xFFFFu) >= D.thr16) ? s[it][jt][0] * D.scale : 0.f;
                    s[it][jt][1] = ((h0 >> 16) >= D.thr16) ? s[it][jt][1] * D.scale : 0.f;
                    s[it][jt][2] = ((h1 & 0xFFFFu) >= D.thr16) ? s[it][jt][2] * D.scale : 0.f;
                    s[it][jt][3] = ((h1 >> 16) >= D.thr16) ? s[it][jt][3] * D.scale : 0.f;
                }
            }
        }
        // O^T[feature 16 hp + 4g + reg][query] += V[key 16 jt + 4g' + kk][feature 16 hp + r] P^T[key][query]: the V fragment of
        // a (key tile, kk) step serves all query tiles
#pragma unroll
        for (int jt = 0; jt < DVS_WNT; ++jt) {
            if (jt < NT) {
                const float* vp = l.V + (16 * jt + 4 * L.g) * DVS_LD + 16 * hp + L.r;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const float va = vp[kk * DVS_LD];
#pragma unroll
                    for (int it = 0; it < DVS_WNT; ++it)
                        if ((pairs >> (3 * it + jt)) & 1u) o[it] = dvs_mfma(va, s[it][jt][kk], o[it]);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < DVS_WNT; ++it)
            if (it < NT && mine) *(f4*)(l.Q + (16 * it + L.r) * DVS_LD + 16 * hp + 4 * L.g) = o[it];   // O over this head's slice of Q
#ifndef DVS_EMU
        asm volatile("" ::"v"(tch0), "v"(tch1));
#endif
        WSTAMP(3);
        __syncthreads();
        WSTAMP(4);
        // ---- stage 3 ------------------------------------------------------------------------------------------------
        if (has_tile) {
            f4 o[4], y[4];
            dvs_lds_T(o, l.Q, tok0, L);
#pragma unroll
            for (int t = 0; t < 4; ++t) y[t] = dvs_vecT(l.outb, t, L);
            dvs_matb3<4>(y, dvs_split3_T(o), l.Wout, 64, 0, L);
            dvs_dropout_tile(y, dvs_site_key(a.dims.seed_lo, a.dims.seed_hi, a.site_post, gdag), D, L, tok0);
            const bool valid = L.r < Nl;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) y[t][kk] = valid ? x[t][kk] + y[t][kk] : 0.f;
            dvs_store_pre(a.out_pre, a.out_stats, (size_t)dag * NT + L.wave, y, L);
        }
        WSTAMP(5);
        __syncthreads();            // stage 3 reads O (= Q) before the next DAG's stage 1 overwrites it
        WSTAMP(6);
    }
}

void dvs_launch_attn_fwd_w(const AttnArgs& a, int grid, dvs_stream_t st) {
    const size_t lds = ATTNW_BYTES;
    DVS_SET_LDS(k_attn_fwd_w, lds);
    DVS_LAUNCH(k_attn_fwd_w, dim3(grid), dim3(512), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Loss head forward, wide (pace.py:1880-1972; k_loss_fwd restated for 3 tiles, up to 48 classes).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_loss_fwd_w(LossArgs a) {
    DVS_DYN_LDS(smem);
    const LossWLds l = lossw_lds(smem);
    lossw_stage(l, a, false);
    float* const part = l.dlm;                            // (forward layout: dvs_lossw_lds_floats(false))
    __syncthreads();
    const Lane L = dvs_lane();
    const int N = a.dims.N, C = a.dims.C, NT = a.dims.NT;
    const int tok0 = 16 * L.wave, Nl = dvs_rows_of(N, L.wave);
    const bool has_tile = L.wave < NT;
    const float b2 = l.b2[0];
    for (int dag = blockIdx.x; dag < a.dims.B; dag += gridDim.x) {
        const DvsRecordW* rec = (const DvsRecordW*)a.rec + dag;
        const size_t tile = (size_t)dag * NT + L.wave;
        float nll = 0.f;
        f4 w2v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) w2v[t] = dvs_vecT(l.w2, t, L);
        const int tok = tok0 + L.r;                       // this lane's token
        if (has_tile) {
            f4 U[4];
            f4 h[4], dummy[4];
            float rstd;
            dvs_load_x<false>(h, dummy, rstd, a.xin, a.ln, l.lg, l.lb, tile, Nl, L);
            // ---- node head: 3 class tiles ------------------------------------------------------------------------
            f4 t1[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) t1[t] = dvs_vecT(l.bn1, t, L);
            dvs_mat_T<2, 4>(t1, h, l.Wn1, DVS_LD, 0, L);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) t1[t][kk] = fmaxf(t1[t][kk], 0.f);
            f4 lgt[3];
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) lgt[ct] = *(const f4*)(l.bn2 + 16 * ct + 4 * L.g);
            dvs_mat_T<3, 2>(lgt, t1, l.Wn2, LOSSW_LDN2, 0, L);
            float mx = -3.0e38f;
#pragma unroll
            for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) mx = (16 * ct + 4 * L.g + reg < C) ? fmaxf(mx, lgt[ct][reg]) : mx;
            mx = dvs_max_g(mx);
            float se = 0.f;
#pragma unroll
            for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) se += (16 * ct + 4 * L.g + reg < C) ? __expf(lgt[ct][reg] - mx) : 0.f;
            se = dvs_sum_g(se);
            const float lse = mx + __logf(se);
            const int target = rec->label[tok + 1 < DVS_WTOK ? tok + 1 : 0];
#pragma unroll
            for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    nll -= (16 * ct + 4 * L.g + reg == target && tok < N - 1) ? (lgt[ct][reg] - lse) : 0.f;
            // ---- edge head: U = Wa h (registers), V = Wb h + b1 (LDS, all tiles) -----------------------------------
            f4 V[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                U[t] = f4_zero();
                V[t] = dvs_vecT(l.be1, t, L);
            }
            dvs_mat_T<4, 4>(U, h, l.Wa, DVS_LD, 0, L);
            dvs_mat_T<4, 4>(V, h, l.Wb, DVS_LD, 0, L);
            dvs_park_T(l.V + tok0 * DVS_LD, V, L);
            dvs_park_T(l.U + tok0 * DVS_LD, U, L);
        }
        __syncthreads();
        // The pair walk — lane r = token i = 16 t + r walks j < i —, shared evenly by the FOUR waves (k_loss_bwd_w's pass 1): tile t
        // has min(N - 2, 16 t + 15) steps; the steps of all tiles, in tile order, are cut into four equal ranges, and a wave takes
        // U_t of the tiles its range touches from LDS.  (One tile per wave: the walk lasted as long as the last tile's, 38 of 84
        // steps at N = 40, and the fourth wave idled.)
        {
            auto steps1 = [&](int t) { const int e = N - 2 < 16 * t + 15 ? N - 2 : 16 * t + 15; return t < NT && e > 0 ? e : 0; };
            const int total = steps1(0) + steps1(1) + steps1(2), q = (total + 3) >> 2;
            const int g0 = L.wave * q, g1 = g0 + q;
            float enll = 0.f;
            int off = 0;
            for (int t = 0; t < DVS_WNT; ++t) {
                const int cnt = steps1(t);
                const int lo = (g0 > off ? g0 : off) - off, hi = (g1 < off + cnt ? g1 : off + cnt) - off;
                off += cnt;
                if (lo >= hi) continue;
                const int ptok = 16 * t + L.r;
                f4 Ut[4];
                dvs_lds_T(Ut, l.U, 16 * t, L);
                const uint64_t par = rec->parents[ptok + 1 < DVS_WTOK ? ptok + 1 : 0];
                for (int j = lo; j < hi; ++j) {
                    f4 ev = f4_zero();
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const f4 x = Ut[tt] + *(const f4*)(l.V + j * DVS_LD + 16 * tt + 4 * L.g);
                        f4 pre;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) pre[kk] = fmaxf(x[kk], 0.f);
                        ev += w2v[tt] * pre;
                    }
                    const float logit = dvs_sum_g((ev[0] + ev[1]) + (ev[2] + ev[3])) + b2;
                    const bool pv = (ptok > j) && (ptok <= N - 2);
                    const float truth = (float)((par >> (j + 1)) & 1ull);
                    // hardware exp / log (k_loss_fwd): log1p's range handling costs ~40 instructions for <= 1e-7 of a term in (0, ln 2]
                    const float bce = fmaxf(logit, 0.f) - logit * truth + __logf(1.0f + __expf(-fabsf(logit)));
                    enll += pv ? bce : 0.f;
                }
            }
            nll += (L.g == 0) ? enll : 0.f;
            nll = dvs_sum_wave(nll);
            if (L.lane == 0) part[L.wave] = nll;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int w = 0; w < 4; ++w) s += part[w];
            a.dag_loss[(size_t)dag * 2] = s;
        }
    }
}

void dvs_launch_loss_fwd_w(const LossArgs& a, int grid, dvs_stream_t st) {
    const size_t lds = dvs_lossw_lds_floats(false) * 4;
    DVS_SET_LDS(k_loss_fwd_w, lds);
    DVS_LAUNCH(k_loss_fwd_w, dim3(grid), dim3(256), lds, st, a);
}
