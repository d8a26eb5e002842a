// Backward of the loss head, the embedding, and the latent block (fc1/fc2/fc3).
#include "dvs_backward.h"
#include "dvs_wimg.h"
#include "dvs_latent_bwd.h"
#include "dvs_loss.h"

// ---------------------------------------------------------------------------------------------------------
// Loss head backward (autograd of pace.py:1880-1972) fused with the last decoder LayerNorm's backward.
// ---------------------------------------------------------------------------------------------------------
#ifdef DVS_STAMPS
// inner budget of k_loss_bwd (tools/loss_stamps.py): cycles summed over the wave's DAGs, per (workgroup, wave, segment)
__device__ unsigned long long dvs_stamps_lossb[256 * 4 * 12];
DVS_STAMP_READER(lossb)
#endif
#define LBSTAMP(k) DVS_ACC_STAMP_AT(dvs_stamps_lossb, lst_, 4, 12, k)      // 4 waves, ids 0-9
// EMIT (the fused train step, dvs_loss_backward_emit): the kernel also writes the per-DAG reconstruction loss k_loss_fwd would
// have written, dag_loss[2 dag] — logits, max, sum of exponentials and pair logits are all live here anyway.  The gradient's
// arithmetic is the same in both instances; the plain one is instruction for instruction the kernel without the switch.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_loss_bwd(LossArgs a, DvsStagePlan plan) {
#ifdef DVS_STAMPS
    unsigned long long lst_ = __builtin_amdgcn_s_memtime();
#endif
    DVS_DYN_LDS(smem);
    const LossLds l = loss_lds(smem);
    const int N = a.dims.N, C = a.dims.C;
    dvs_stage_now<(LOSS_CHUNKS + 3) / 4>(&plan, smem);        // the whole loss block (dvs_wimg.h) in one batch of loads
    __syncthreads();
    const Lane L = dvs_lane();
    float* scrV = l.scr + L.wave * 3 * DVS_SCR;
    float* scrU = scrV + DVS_SCR;
    float* dlm = scrU + DVS_SCR;      // [16][16] d logit matrix
    const float b2 = l.b2[0];
    const float gr = a.gcoef[0];
    // The two 64 x 64 edge matrices are accumulated COOPERATIVELY by the workgroup's four waves (one group of dvs_backward.h):
    // every wave parks dU, dV and h of its DAG as bf16 [hi | lo] pairs, wave w accumulates rows 16w .. of dWa / dWb over the
    // four DAGs on the bf16 pipe (dvs_coop_dw_bf) — 16 accumulator registers per matrix instead of 64 fp32-MFMA ones (round 2:
    // 512 registers + 4 spilled, 20 bytes of scratch), and d edge0.bias rides along as the column sums of dV.
    f4 dWn1[2][4], dWn2[1][2], aWa[4], aWb[4], abU = f4_zero(), abV = f4_zero(), dbn1[2], dbn2[1], dw2[4], dgam[4], dbet[4];
    float db2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) dw2[i] = dgam[i] = dbet[i] = aWa[i] = aWb[i] = f4_zero();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        dbn1[i] = f4_zero();
        dWn2[0][i] = f4_zero();
#pragma unroll
        for (int j = 0; j < 4; ++j) dWn1[i][j] = f4_zero();
    }
    dbn2[0] = f4_zero();
    LBSTAMP(0);                  // staging + barrier + accumulator init
    const dvs_bf16* const slots = (const dvs_bf16*)l.scr;        // wave w's three tiles at w * 3 * DVS_SCR floats
    constexpr int SLOT_STRIDE = 2 * 3 * DVS_SCR;                 // bf16 elements between the slots of two waves
    // every wave runs the same number of rounds (workgroup barriers inside): a wave beyond the batch parks zero tiles
    for (int base = blockIdx.x * L.nwaves; base < a.dims.B; base += gridDim.x * L.nwaves) {
        const int dag = base + L.wave;
        if (dag >= a.dims.B) {
            const f4 z[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
            dvs_park_bf((dvs_bf16*)scrV, z, L);
            dvs_park_bf((dvs_bf16*)scrU, z, L);
            dvs_park_bf((dvs_bf16*)dlm, z, L);
            __syncthreads();
            dvs_coop_dw_bf(aWa, abU, slots, slots + 2 * 2 * DVS_SCR, SLOT_STRIDE, L);
            dvs_coop_dw_bf(aWb, abV, slots + 2 * DVS_SCR, slots + 2 * 2 * DVS_SCR, SLOT_STRIDE, L);
            __syncthreads();
            continue;
        }
        f4 h[4], xhat[4];
        float rstd;
        dvs_load_x<true>(h, xhat, rstd, a.xin, a.ln, l.lg, l.lb, dag, N, L);
        // touch the wave's NEXT tile (one dword per 64-byte piece: one load instruction): this kernel runs one wave per SIMD,
        // nothing else hides the ~4 k cycles a cold tile load + LayerNorm statistics cost at the top of every round.  (Loading
        // that tile into registers a round ahead instead, record words included, took 2.5 us off this kernel's 72 at B = 4096
        // and 0.16 % off the step: under three times the run-to-run spread)
        const int nxt = dag + gridDim.x * L.nwaves;
        const float touch = a.xin[(size_t)(nxt < a.dims.B ? nxt : dag) * DVS_TILE + L.lane * 16];
        const DvsRecord* rec = a.rec + dag;
        f4 hN[4];
        dvs_t2n<4>(hN, h, scrV, L);
        LBSTAMP(1);              // tile load + LayerNorm + transpose
        f4 dh[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
        float nll = 0.f, enll = 0.f;          // EMIT: this lane's share of the node NLL and of the edge BCE, as k_loss_fwd splits them
        // ---- node head ----------------------------------------------------------------------------------
        {
            f4 t1p[2], t1[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) t1p[t] = dvs_vecT(l.bn1, t, L);
            dvs_mat_T<2, 4>(t1p, h, l.Wn1, DVS_LD, 0, L);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) t1[t][kk] = fmaxf(t1p[t][kk], 0.f);
            f4 lgt[1] = {*(const f4*)(l.bn2 + 4 * L.g)};
            dvs_mat_T<1, 2>(lgt, t1, l.Wn2, LOSS_LDN2, 0, L);
            float mx = -3.0e38f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) mx = (4 * L.g + reg < C) ? fmaxf(mx, lgt[0][reg]) : mx;
            mx = dvs_max_g(mx);
            f4 ex;
            float se = 0.f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                ex[reg] = (4 * L.g + reg < C) ? __expf(lgt[0][reg] - mx) : 0.f;
                se += ex[reg];
            }
            se = dvs_sum_g(se);
            const float rse = dvs_rcp(se);
            const int target = rec->label[(L.r + 1) & 15];
            const bool vt = L.r < N - 1;
            if constexpr (EMIT) {              // k_loss_fwd's node term from the same logits, maximum and sum
                const float lse = mx + __logf(se);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    nll -= (4 * L.g + reg == target && L.r < N - 1) ? (lgt[0][reg] - lse) : 0.f;
            }
            f4 dlg[1];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int c = 4 * L.g + reg;
                dlg[0][reg] = (vt && c < C) ? gr * (ex[reg] * rse - (c == target ? 1.f : 0.f)) : 0.f;
            }
            dbn2[0] += dlg[0];
            f4 dlgN[1], t1N[2];
            dvs_t2n<1>(dlgN, dlg, scrV, L);
            dvs_t2n<2>(t1N, t1, scrV, L);
            dvs_outer_acc<1, 2>(dWn2, dlgN, t1N);
            f4 dt1[2] = {f4_zero(), f4_zero()};
            dvs_mat_Tt<2, 1>(dt1, dlg, l.Wn2, LOSS_LDN2, 0, L);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) dt1[t][kk] = t1p[t][kk] > 0.f ? dt1[t][kk] : 0.f;
                dbn1[t] += dt1[t];
            }
            f4 dt1N[2];
            dvs_t2n<2>(dt1N, dt1, scrV, L);
            dvs_outer_acc<2, 4>(dWn1, dt1N, hN);
            dvs_mat_Tt<4, 2>(dh, dt1, l.Wn1, DVS_LD, 0, L);
        }
        LBSTAMP(2);              // node head forward + backward
        // ---- edge head ----------------------------------------------------------------------------------
        f4 U[4], V[4], w2v[4], dU[4], dV[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            U[t] = f4_zero();
            V[t] = dvs_vecT(l.be1, t, L);
            w2v[t] = dvs_vecT(l.w2, t, L);
            dU[t] = dV[t] = f4_zero();
        }
        {   // k_loss_fwd's own bf16x6 sequence, bit for bit: the sign of U_i + V_j is the ReLU mask
            const Split3T hs = dvs_split3_T(h);
            dvs_matb3<4>(U, hs, l.Wa, 64, 0, L);
            dvs_matb3<4>(V, hs, l.Wb, 64, 0, L);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            *(f4*)(scrV + L.r * DVS_LD + 16 * t + 4 * L.g) = V[t];
            *(f4*)(scrU + L.r * DVS_LD + 16 * t + 4 * L.g) = U[t];
        }
        dvs_wave_sync();
        const unsigned par = rec->parents[(L.r + 1) & 15];
        LBSTAMP(3);              // U, V recompute + park
        // Both passes are vector-instruction bound on one wave per SIMD, so they are written for instruction count: whole-f4
        // arithmetic (v_pk_add / v_pk_fma), w2 factored out of the dU / dV sums (dU = w2 * sum_j dl_j step(pre_j)), and the ReLU
        // derivative as a clamped multiply, step(x) = clamp(x * 1e30, 0, 1) — one instruction instead of compare + select; it
        // differs from (x > 0) only for 0 < x < 1e-30, far below the 1e-6 at which device and oracle can disagree on a unit.
        // pass 1: lane r = i walks j; accumulates sU (-> dU), dw2, db2; publishes d logit(i, j)
        f4 sU[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()}, sV[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
        // two j per iteration, written out (hipcc does not unroll this loop on request): the chain LDS read -> 48 vector
        // instructions -> cross-lane sum -> exp -> reciprocal -> 32 more runs twice side by side; an odd last j repeats j - 1
        // with d logit forced to zero
        for (int j0 = 0; j0 < N - 2; j0 += 2) {
            f4 pre[2][4], ev[2] = {f4_zero(), f4_zero()};
            const bool has2 = j0 + 1 < N - 2;
            const int jj[2] = {j0, has2 ? j0 + 1 : j0};
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f4 x = U[t] + *(const f4*)(scrV + jj[u] * DVS_LD + 16 * t + 4 * L.g);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) pre[u][t][kk] = fmaxf(x[kk], 0.f);
                    ev[u] += w2v[t] * pre[u][t];
                }
            float dl[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float logit = dvs_sum_g((ev[u][0] + ev[u][1]) + (ev[u][2] + ev[u][3])) + b2;
                const bool pv = (L.r > jj[u]) && (L.r <= N - 2) && (u == 0 || has2);
                const float truth = (float)((par >> (jj[u] + 1)) & 1u);
                const float sg = dvs_rcp(1.0f + __expf(-logit));
                dl[u] = pv ? gr * (sg - truth) : 0.f;
                if constexpr (EMIT) {          // k_loss_fwd's BCE term; lane g keeps the pairs j = g, g + 4, ... of its row, as there
                    const float x = logit;
                    const float bce = fmaxf(x, 0.f) - x * truth + __logf(1.0f + __expf(-fabsf(x)));
                    enll += (pv && (jj[u] & 3) == L.g) ? bce : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    dw2[t] += pre[u][t] * dl[u];
                    f4 st;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) st[kk] = fminf(fmaxf(pre[u][t][kk] * 1.0e30f, 0.f), 1.f);
                    sU[t] += st * dl[u];
                }
            if (L.g == 0) {
                db2 += dl[0] + dl[1];
                dlm[L.r * 16 + j0] = dl[0];
                if (has2) dlm[L.r * 16 + j0 + 1] = dl[1];
            }
        }
        dvs_wave_sync();
        LBSTAMP(4);              // pass 1
        // pass 2: lane r = j walks i; accumulates sV (-> dV)
#pragma unroll 2
        for (int i = 1; i <= N - 2; ++i) {
            const float dl = (L.r < i) ? dlm[i * 16 + L.r] : 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f4 x = *(const f4*)(scrU + i * DVS_LD + 16 * t + 4 * L.g) + V[t];
                f4 st;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) st[kk] = fminf(fmaxf(x[kk] * 1.0e30f, 0.f), 1.f);
                sV[t] += st * dl;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            dU[t] = w2v[t] * sU[t];
            dV[t] = w2v[t] * sV[t];
        }
        dvs_wave_sync();
        LBSTAMP(5);              // pass 2
        // park dU, dV, h over the wave's three tiles (V, U and the d logit matrix are dead) and accumulate with the group
        dvs_park_bf((dvs_bf16*)scrV, dU, L);
        dvs_park_bf((dvs_bf16*)scrU, dV, L);
        dvs_park_bf((dvs_bf16*)dlm, h, L);
        __syncthreads();
        dvs_coop_dw_bf(aWa, abU, slots, slots + 2 * 2 * DVS_SCR, SLOT_STRIDE, L);
        dvs_coop_dw_bf(aWb, abV, slots + 2 * DVS_SCR, slots + 2 * 2 * DVS_SCR, SLOT_STRIDE, L);
        __syncthreads();
        LBSTAMP(6);              // parks + cooperative dWa, dWb
        dvs_matb_T<4>(dh, dvs_split_T(dU), l.WaT, l.WaT + DVS_IMG64, 0, L);       // d h += Wa^T dU + Wb^T dV (bf16x3: smooth)
        dvs_matb_T<4>(dh, dvs_split_T(dV), l.WbT, l.WbT + DVS_IMG64, 0, L);
        dvs_ln_bwd(dh, xhat, rstd, l.lg, dgam, dbet, L);
        dvs_store_tile(a.gout, dag, dh, L);
        if constexpr (EMIT) {
            nll += enll;                       // every lane holds distinct pairs
            nll = dvs_sum_wave(nll);
            if (L.lane == 0) a.dag_loss[(size_t)dag * 2] = nll;
        }
#ifndef DVS_EMU
        asm volatile("" ::"v"(touch));         // keeps the touch load alive without using its value
#else
        (void)touch;
#endif
        LBSTAMP(7);              // d h products, LayerNorm backward, store
    }
    __syncthreads();
    LBSTAMP(8);                  // closing barrier
    float* slab = a.slab + (size_t)blockIdx.x * a.P;
    {
        // the edge matrices: rows 16w .. straight from wave w's accumulators (add_edge.0.weight is [64][128] = [Wa | Wb])
        dvs_coop_flush<4>(nullptr, slab + a.o_edge0_w, aWa, L, false, false, 128);
        dvs_coop_flush<4>(nullptr, slab + a.o_edge0_w + 64, aWb, L, false, false, 128);
        if (L.r == 0) {          // d edge0.bias: wave w holds features 16w + 4g + reg (every column r the same)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) slab[a.o_edge0_b + 16 * L.wave + 4 * L.g + reg] = abV[reg];
        }
        // node matrices + the remaining vectors through LDS
        float* rN1 = (float*)smem;                      // 4 * 2048
        float* rN2 = rN1 + 4 * 2048;                    // 4 * 512
        float* rv = rN2 + 4 * 512;
        dvs_stage_dw<2, 4>(rN1, dWn1, L);
        dvs_stage_dw<1, 2>(rN2, dWn2, L);
        float* es = rv + 192 + 4 * DVS_RED_VEC + 16 + L.wave * DVS_SCR;
        dvs_stage_vec<2>(rv, dbn1, es, L);
        dvs_stage_vec<1>(rv + 128, dbn2, es, L);
        dvs_stage_vec<4>(rv + 192 + DVS_RED_VEC, dw2, es, L);  // per-lane partials over pairs: summed over r like a bias
        dvs_stage_vec<4>(rv + 192 + 2 * DVS_RED_VEC, dgam, es, L);
        dvs_stage_vec<4>(rv + 192 + 3 * DVS_RED_VEC, dbet, es, L);
        const float sb2 = dvs_sum_wave(L.g == 0 ? db2 : 0.f);
        float* rb2 = rv + 192 + 4 * DVS_RED_VEC;
        if (L.lane == 0) rb2[L.wave] = sb2;
        __syncthreads();
        dvs_flush_dw<2, 4>(rN1, slab + a.o_node0_w, L);
        dvs_flush_dw<1, 2>(rN2, slab + a.o_node2_w, L, C, 32);
        dvs_flush_vec<2>(rv, slab + a.o_node0_b, L);
        dvs_flush_vec<1>(rv + 128, slab + a.o_node2_b, L, C);
        dvs_flush_vec<4>(rv + 192 + DVS_RED_VEC, slab + a.o_edge2_w, L);
        dvs_flush_vec<4>(rv + 192 + 2 * DVS_RED_VEC, slab + a.o_ln_g, L);
        dvs_flush_vec<4>(rv + 192 + 3 * DVS_RED_VEC, slab + a.o_ln_b, L);
        if (threadIdx.x == 0) {
            float s = rb2[0];
            for (int w = 1; w < L.nwaves; ++w) s += rb2[w];
            slab[a.o_edge2_b] = s;
        }
    }
    LBSTAMP(9);                  // slab epilogue
}

void dvs_launch_loss_bwd(const LossArgs& a, int grid, bool emit_loss, dvs_stream_t st) {
    const size_t lds = loss_lds_bytes(4, 3);       // (the epilogue's staging areas are smaller than the DAG loop's layout)
    DvsStagePlan plan;
    loss_plan(plan, a);
    if (emit_loss) {
        DVS_SET_LDS(k_loss_bwd<true>, lds);
        DVS_LAUNCH_AS("k_loss_bwd", k_loss_bwd<true>, dim3(grid), dim3(256), lds, st, a, plan);
    } else {
        DVS_SET_LDS(k_loss_bwd<false>, lds);
        DVS_LAUNCH_AS("k_loss_bwd", k_loss_bwd<false>, dim3(grid), dim3(256), lds, st, a, plan);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Embedding backward (autograd of pace.py:201-221, 1181-1184).  The one-hot first layers are row gathers forward,
// so their gradients are row scatters: per-wave LDS accumulators (ds_add_f32), summed over waves in fixed order.
// Handles up to two gradient sources per DAG (encoder-side and decoder-side embeddings: same weights, different
// dropout sites).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_embed_bwd(EmbedArgs a, const float* gout2, int site2, DvsStagePlan plan) {
    DVS_DYN_LDS(smem);
    const int N = a.dims.N, C = a.dims.C;
    float* W1 = (float*)smem;                        // [32][LD], rows >= 2N zero
    float* W2 = W1 + 2 * DVS_MAXTOK * DVS_LD;        // [64][36]
    float* labw = W2 + 64 * EMB_LDW2;                // [32][16]
    float* labb = labw + 32 * 16;                    // [32]
    float* scr0 = labb + 32;                         // nwaves tiles
    // the embedding block (dvs_wimg.h: DvsEmbImg) in one batch: 20 wave chunks on 8 waves (4 in the narrow mapping)
    if (blockDim.x >= 512) dvs_stage_now<3>(&plan, smem);
    else dvs_stage_now<5>(&plan, smem);
    __syncthreads();
    const Lane L = dvs_lane();
    const DvsDrop D = dvs_drop_of(a.dims);
    float* scr = scr0 + L.wave * DVS_SCR;
    f4 dW2[4][2], dlabb[2], dW1a[1][4], dW1b[1][4], dlab[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i) dW2[i][0] = dW2[i][1] = dW1a[0][i] = dW1b[0][i] = f4_zero();
    dlabb[0] = dlabb[1] = dlab[0][0] = dlab[1][0] = f4_zero();
    for (int dag = blockIdx.x * L.nwaves + L.wave; dag < a.dims.B; dag += gridDim.x * L.nwaves) {
        const DvsRecord* rec = a.rec + dag;
        const bool valid = L.r < N;
        const int label = rec->label[L.r];
        const uint32_t gdag = a.dims.dag_offset + dag;
        const EmbSel sel = dvs_emb_selectors(rec, N, scr, L);
        f4 e1[4];                                    // hidden (post-relu, pre-dropout), as in the forward
        dvs_emb_hidden(e1, W1, N, sel, L);
        for (int src = 0; src < 2; ++src) {
            const float* gsrc = src == 0 ? a.gout : gout2;
            if (!gsrc) continue;
            const int site = src == 0 ? a.site : site2;
            f4 gx[4];
            dvs_load_grad(gx, gsrc, dag, N, L);
            // label half: d(relu(labw[:, label] + b))
            f4 dle[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int f = 16 * t + 4 * L.g + kk;
                    const float pre = labw[f * 16 + label] + labb[f];
                    dle[t][kk] = (valid && pre > 0.f) ? gx[t][kk] : 0.f;
                }
            dlabb[0] += dle[0];
            dlabb[1] += dle[1];
            // positional half
            // the first dropout's mask as a tile of {0, scale}: drawn once, applied to the hidden here and to its gradient below
            // (was two passes over the same 8 draws per lane); the second site covers 32 features: two tiles, not four
            const uint32_t k1 = dvs_site_key(a.dims.seed_lo, a.dims.seed_hi, site, gdag);
            f4 m1[4] = {f4_splat(1.f), f4_splat(1.f), f4_splat(1.f), f4_splat(1.f)};
            dvs_dropout_tile(m1, k1, D, L);
            f4 e1d[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) e1d[t] = e1[t] * m1[t];
            f4 de2[2] = {gx[2], gx[3]};
            dvs_dropout_tile<2>(de2, dvs_site_key(a.dims.seed_lo, a.dims.seed_hi, site + 1, gdag), D, L);
            f4 e1dN[4], de2N[2], dleN[2];
            dvs_t2n<4>(e1dN, e1d, scr, L);
            dvs_t2n<2>(de2N, de2, scr, L);
            dvs_t2n<2>(dleN, dle, scr, L);
            dvs_outer_acc<4, 2>(dW2, e1dN, de2N);
            f4 de1[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
            dvs_mat_T<4, 2>(de1, de2, W2, EMB_LDW2, 0, L);
#pragma unroll
            for (int t = 0; t < 4; ++t) de1[t] *= m1[t];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) de1[t][kk] = e1[t][kk] > 0.f ? de1[t][kk] : 0.f;
            f4 de1N[4];
            dvs_t2n<4>(de1N, de1, scr, L);
            // row scatters as selector products: dW1a[p][c] += Sel[p][i] de1[i][c], dW1b likewise with Par;
            // d labw^T: dlab[f][c] += dle[i][f] [label_i == c]
            f4 selA[1] = {sel.selA}, parA[1] = {sel.parA}, labA[1] = {sel.labA};
            dvs_outer_acc<1, 4>(dW1a, selA, de1N);
            dvs_outer_acc<1, 4>(dW1b, parA, de1N);
            dvs_outer_acc<2, 1>(dlab, dleN, labA);
        }
    }
    __syncthreads();
    // 8 waves (round 3; two per SIMD — the DAG loop is a chain of LDS transposes and small MFMA products, latency-bound with one):
    // the per-wave partials meet in LDS in two passes (all four matrices at once would need 8 x 4608 floats = 147 KB)
    float* slab = a.slab + (size_t)blockIdx.x * a.P;
    float* r1a = (float*)smem;                 // 8 * 1024
    float* r1b = r1a + 8 * 1024;               // 8 * 1024
    float* rlab = r1b + 8 * 1024;              // 8 * 512
    float* rv = rlab + 8 * 512;                // 8 * 32
    dvs_stage_dw<1, 4>(r1a, dW1a, L);
    dvs_stage_dw<1, 4>(r1b, dW1b, L);
    dvs_stage_dw<2, 1>(rlab, dlab, L);
    dvs_stage_vec<2>(rv, dlabb, rv + 8 * 32 + L.wave * DVS_SCR, L);
    __syncthreads();
    dvs_flush_dw<1, 4>(r1a, slab + a.oW1, L, N, 64);
    dvs_flush_dw<1, 4>(r1b, slab + a.oW1 + (size_t)N * 64, L, N, 64);
    dvs_flush_dw<2, 1>(rlab, slab + a.olab_w, L, 32, C, C);
    dvs_flush_vec<2>(rv, slab + a.olab_b, L);
    __syncthreads();
    float* rW2 = (float*)smem;                 // 8 * 2048
    dvs_stage_dw<4, 2>(rW2, dW2, L);
    __syncthreads();
    dvs_flush_dw<4, 2>(rW2, slab + a.oW2, L);
}

void dvs_launch_embed_bwd(const EmbedArgs& a, const float* gout2, int site2, int grid, int nw, dvs_stream_t st) {
    size_t lds = (2 * DVS_MAXTOK * DVS_LD + 64 * EMB_LDW2 + 32 * 16 + 32 + 8 * DVS_SCR) * 4;
    const size_t red = (8 * (1024 + 1024 + 512) + 8 * 32 + 8 * DVS_SCR) * 4;          // first epilogue pass (the second: 8 * 2048 floats)
    if (lds < red) lds = red;
    DvsStagePlan plan;
    dvs_plan_clear(plan);
    dvs_plan_seg(plan, DVS_FAKE_LDS, DVS_FAKE_LDS, a.embimg, 2 * DvsEmbImg::FLOATS);
    dvs_plan_seal(plan);
    DVS_SET_LDS(k_embed_bwd, lds);
    DVS_LAUNCH(k_embed_bwd, dim3(grid), dim3(nw == 4 ? 256 : 512), lds, st, a, gout2, site2, plan);     // narrow mapping: 4 waves
}

// ---------------------------------------------------------------------------------------------------------
// Latent block backward, part 1 (one wave per 16 DAGs): dz^T = fc3^T dmem^T; through the reparameterisation and
// the KL term to (d mu, d logvar); then d enc_out^T = [fc1;fc2]^T [dmu;dlogvar]^T, stored frag order.
// ---------------------------------------------------------------------------------------------------------
constexpr int LATB_WAVES = 8;    // as the chained encoder backward runs it (k_bwd_stack): same summation order, bit for bit
__global__ __launch_bounds__(64 * LATB_WAVES) void k_latent_bwd(LatentBwdArgs a) {
    __shared__ f4 part[LATB_WAVES][2][64];
    dvs_latent_bwd_group<LATB_WAVES>(a, part, (int)blockIdx.x * 16, (int)blockIdx.x * 16 + 8);
}

void dvs_launch_latent_bwd(const LatentBwdArgs& a, dvs_stream_t st) {
    const int ngroups = (a.dims.B + 15) / 16;
    DVS_LAUNCH(k_latent_bwd, dim3(ngroups), dim3(64 * LATB_WAVES), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Latent block backward, part 2: weight gradients of fc1/fc2/fc3 — batch-contraction GEMMs over ALL DAGs.
//   dWfc[o][col(k')] = sum_dag dout[dag][o] X[dag][k'] ;  dW3[row(k')][o] = sum_dag dmem[dag][k'] z[dag][o]
// Workgroup (mg, q): 4 consecutive output column tiles (64 frag columns k') x batch part q (DVS_FC_PARTS parts); its
// 8 waves split the part's DAGs (two waves per SIMD: the contraction walk is a chain of load batches and MFMAs, latency-
// bound with one), meet in LDS (fixed order: w + (w+4), then 0..3) and write one partial per part to fcpart[q][param offset];
// k_reduce_slabs adds the parts.  Per 4-DAG contraction step a lane issues 14 loads for 24 MFMAs; the [dag][64]
// dout / [dag][32] z operands are shared by all column tiles (L2).  Bias gradients ride along as column sums.
// ---------------------------------------------------------------------------------------------------------
constexpr int FC_MT = 4;     // column tiles per workgroup
__global__ __launch_bounds__(512) void k_fc_dw(FcDwArgs a) {
    __shared__ f4 red[4][FC_MT * 6 + 2][64];
    const Lane L = dvs_lane();
    const int B = a.dims.B, N = a.dims.N;
    const int ldw = N * 64;
    const int nmg = 16 * a.dims.NT;                                // groups of FC_MT column tiles (64 * NT tiles in all)
    const int mg = blockIdx.x % nmg, q = blockIdx.x / nmg;
    const size_t dstride = (size_t)a.dims.NT * DVS_TILE;
    const int per_q = (B + DVS_FC_PARTS - 1) / DVS_FC_PARTS;
    const int per_w = (per_q + 7) / 8;
    const int d0 = q * per_q + L.wave * per_w;
    int d1 = d0 + per_w;
    if (d1 > (q + 1) * per_q) d1 = (q + 1) * per_q;
    if (d1 > B) d1 = B;
    f4 acc[FC_MT][4], acc3[FC_MT][2];
    f4 bs3 = f4_zero();                                            // d b3 partials: column k' = 16(4mg+j) + r in [j]
    f4 bsfc = f4_zero();                                           // d bfc partial: o = 16t + r (written by mg == 0)
#pragma unroll
    for (int j = 0; j < FC_MT; ++j) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[j][t] = f4_zero();
        acc3[j][0] = acc3[j][1] = f4_zero();
    }
    // 16 DAGs per round: all 56 loads of the round first, none under a condition (`dv ? load : 0` made every contraction step a
    // branch with its own memory round trip: 8 in a row per wave were most of this kernel's 21 us); rows beyond the part read
    // DAG 0 and are zeroed by a multiply
    for (int c0 = d0; c0 < d1; c0 += 16) {
        float ga[4][4], zb[4][2], xb[4][FC_MT], gm[4][FC_MT], live[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int d = c0 + 4 * ks + L.g;
            const bool dv = d < d1;
            const size_t dd = dv ? d : 0;
            live[ks] = dv ? 1.f : 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) ga[ks][t] = a.gz[dd * 64 + 16 * t + L.r];
#pragma unroll
            for (int t = 0; t < 2; ++t) zb[ks][t] = a.z[dd * 32 + 16 * t + L.r];
#pragma unroll
            for (int j = 0; j < FC_MT; ++j) {
                xb[ks][j] = a.xenc[dd * dstride + 16 * (FC_MT * mg + j) + L.r];
                gm[ks][j] = a.gmem[dd * dstride + 16 * (FC_MT * mg + j) + L.r];
            }
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int t = 0; t < 4; ++t) ga[ks][t] *= live[ks];
#pragma unroll
            for (int j = 0; j < FC_MT; ++j) {
                gm[ks][j] *= live[ks];
                bs3[j] += gm[ks][j];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) bsfc[t] += ga[ks][t];
#pragma unroll
            for (int j = 0; j < FC_MT; ++j) {
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[j][t] = dvs_mfma(ga[ks][t], xb[ks][j], acc[j][t]);
#pragma unroll
                for (int t = 0; t < 2; ++t) acc3[j][t] = dvs_mfma(gm[ks][j], zb[ks][t], acc3[j][t]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < FC_MT; ++j) bs3[j] = dvs_sum_g(bs3[j]);
#pragma unroll
    for (int t = 0; t < 4; ++t) bsfc[t] = dvs_sum_g(bsfc[t]);
    // waves 0..3 park their partials, waves 4..7 add theirs on top (wave w + 4 onto wave w's)
    if (L.wave < 4) {
#pragma unroll
        for (int j = 0; j < FC_MT; ++j) {
#pragma unroll
            for (int t = 0; t < 4; ++t) red[L.wave][6 * j + t][L.lane] = acc[j][t];
            red[L.wave][6 * j + 4][L.lane] = acc3[j][0];
            red[L.wave][6 * j + 5][L.lane] = acc3[j][1];
        }
        red[L.wave][6 * FC_MT][L.lane] = bsfc;
        red[L.wave][6 * FC_MT + 1][L.lane] = bs3;
    }
    __syncthreads();
    if (L.wave >= 4) {
        const int w = L.wave - 4;
#pragma unroll
        for (int j = 0; j < FC_MT; ++j) {
#pragma unroll
            for (int t = 0; t < 4; ++t) red[w][6 * j + t][L.lane] += acc[j][t];
            red[w][6 * j + 4][L.lane] += acc3[j][0];
            red[w][6 * j + 5][L.lane] += acc3[j][1];
        }
        red[w][6 * FC_MT][L.lane] += bsfc;
        red[w][6 * FC_MT + 1][L.lane] += bs3;
    }
    __syncthreads();
    if (L.wave >= 4) return;
    // wave w finalises column tile j = w
    const int j = L.wave;
    const int m = FC_MT * mg + j;
    f4 tot[8];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        tot[i] = red[0][6 * j + i][L.lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) tot[i] += red[w][6 * j + i][L.lane];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        tot[6 + i] = red[0][6 * FC_MT + i][L.lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) tot[6 + i] += red[w][6 * FC_MT + i][L.lane];
    }
    float* out = a.fcpart + (size_t)q * a.P;
    // tot[t][reg] = dWfc[o = 16t + 4g + reg][k' = 16m + r]
    const int mm = m & 63;
    {
        const int tok = 16 * (m >> 6) + 4 * (mm & 3) + (L.r >> 2);
        const int f = 16 * (mm >> 4) + 4 * ((mm >> 2) & 3) + (L.r & 3);
        if (tok < N) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int o = 16 * (t & 1) + 4 * L.g + reg;
                    out[(t < 2 ? a.o_fc1_w : a.o_fc2_w) + (size_t)o * ldw + tok * 64 + f] = tot[t][reg];
                }
            if (L.g == 0) {
                const float b3 = j == 0 ? tot[7][0] : j == 1 ? tot[7][1] : j == 2 ? tot[7][2] : tot[7][3];
                out[a.o_fc3_b + tok * 64 + f] = b3;
            }
        }
    }
    // tot[4+t][reg] = dW3[row(k' = 16m + 4g + reg)][o = 16t + r]
    {
        const int tok = 16 * (m >> 6) + 4 * (mm & 3) + L.g;
        const int fb = 16 * (mm >> 4) + 4 * ((mm >> 2) & 3);
        if (tok < N) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    out[a.o_fc3_w + (size_t)(tok * 64 + fb + reg) * 32 + 16 * t + L.r] = tot[4 + t][reg];
        }
    }
    if (mg == 0 && j == 0 && L.g == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) out[(t < 2 ? a.o_fc1_b : a.o_fc2_b) + 16 * (t & 1) + L.r] = tot[6][t];
    }
}

void dvs_launch_fc_dw(const FcDwArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_fc_dw, dim3(16 * a.dims.NT * DVS_FC_PARTS), dim3(512), 0, st, a);
}
