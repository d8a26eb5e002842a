// Latent block (fc1/fc2 -> reparameterize -> KL -> fc3), loss head (node NLL + edge BCE) and loss finalisation.
#include "dvs_kernels.h"
#include "dvs_wimg.h"
#include "dvs_latent.h"
#include "dvs_loss.h"

// ---------------------------------------------------------------------------------------------------------
// Latent block forward (pace.py:1639-1641, 1649-1664, 1997, 2030).  One wave owns 16 DAGs:
//   out^T[64 x 16 dags] = [fc1;fc2][64 x N*64] * Xenc^T     (contraction walks the frag-order tile in 16-float
//                                                            chunks; chunk (m,g) is 4 consecutive features of
//                                                            token 4(m&3)+g, so weights are read in place)
//   z^T = mu^T + eps * exp(logvar/2);  KL per DAG;  mem^T[N*64 x 16 dags] = fc3 * z^T + b3 (stored frag order)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * LAT_WAVES) void k_latent_fwd(LatentArgs a) {
    DVS_DYN_LDS(smem);
    dvs_latent_fwd_group(a, smem, (int)blockIdx.x * 16, (int)blockIdx.x * 16 + 8);
}

void dvs_launch_latent_fwd(const LatentArgs& a, dvs_stream_t st) {
    const int ngroups = (a.dims.B + 15) / 16;
    const size_t lds = (size_t)LAT_WAVES * 4 * 64 * sizeof(f4);
    DVS_SET_LDS(k_latent_fwd, lds);
    DVS_LAUNCH(k_latent_fwd, dim3(ngroups), dim3(64 * LAT_WAVES), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Loss head forward (loss_log_likelihood_full_vectorized, pace.py:1880-1972).
//   node: log_softmax(add_node(h))[i, label_{i+1}] for i < N-1
//   edge: logit(i,j) = w2 . relu(Wa h_i + Wb h_j + b1) + b2 for j < i <= N-2 (W1 cat(h_i,h_j) split into Wa|Wb),
//         truth = adj[j+1][i+1]; BCE-with-logits, summed.
// ---------------------------------------------------------------------------------------------------------
#ifdef DVS_STAMPS
// inner budget of k_loss_fwd (tools/loss_stamps.py): cycles summed over the wave's DAGs, per (workgroup, wave, segment)
DVS_ACC_STAMP_DECL(dvs_stamps_loss);
DVS_STAMP_READER(loss)
#endif
#define LSTAMP(k) DVS_ACC_STAMP(dvs_stamps_loss, lst_, k)
__global__ __launch_bounds__(512) void k_loss_fwd(LossArgs a, DvsStagePlan plan) {
#ifdef DVS_STAMPS
    unsigned long long lst_ = __builtin_amdgcn_s_memtime();
#endif
    DVS_DYN_LDS(smem);
    const LossLds l = loss_lds(smem);
    // the whole loss block in one batch of loads (8 waves per workgroup; 4 in the narrow mapping of small batches)
    if (blockDim.x >= 512) dvs_stage_now<(LOSS_CHUNKS + 7) / 8>(&plan, smem);
    else dvs_stage_now<(LOSS_CHUNKS + 3) / 4>(&plan, smem);
    __syncthreads();
    const Lane L = dvs_lane();
    const int N = a.dims.N, C = a.dims.C;
    float* scr = l.scr + L.wave * DVS_SCR;
    const float b2 = l.b2[0];
    LSTAMP(0);                   // staging + barrier
    for (int dag = blockIdx.x * L.nwaves + L.wave; dag < a.dims.B; dag += gridDim.x * L.nwaves) {
        f4 h[4], dummy[4];
        float rstd;
        dvs_load_x<false>(h, dummy, rstd, a.xin, a.ln, l.lg, l.lb, dag, N, L);
        LSTAMP(1);               // tile load + LayerNorm
        const DvsRecord* rec = a.rec + dag;
        // ---- node head -------------------------------------------------------------------------------
        f4 t1[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) t1[t] = dvs_vecT(l.bn1, t, L);
        dvs_mat_T<2, 4>(t1, h, l.Wn1, DVS_LD, 0, L);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) t1[t][kk] = fmaxf(t1[t][kk], 0.f);
        f4 lgt[1] = {*(const f4*)(l.bn2 + 4 * L.g)};
        dvs_mat_T<1, 2>(lgt, t1, l.Wn2, LOSS_LDN2, 0, L);
        float mx = -3.0e38f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) mx = (4 * L.g + reg < C) ? fmaxf(mx, lgt[0][reg]) : mx;
        mx = dvs_max_g(mx);
        float se = 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) se += (4 * L.g + reg < C) ? __expf(lgt[0][reg] - mx) : 0.f;
        se = dvs_sum_g(se);
        const float lse = mx + __logf(se);
        const int target = rec->label[(L.r + 1) & 15];
        float nll = 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            nll -= (4 * L.g + reg == target && L.r < N - 1) ? (lgt[0][reg] - lse) : 0.f;
        LSTAMP(2);               // node head
        // ---- edge head -------------------------------------------------------------------------------
        f4 U[4], V[4], w2v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            U[t] = f4_zero();
            V[t] = dvs_vecT(l.be1, t, L);
            w2v[t] = dvs_vecT(l.w2, t, L);
        }
        {   // fp32-accurate bf16x6 products; k_loss_bwd recomputes U, V with the same sequence (their sum's sign is a ReLU mask)
            const Split3T hs = dvs_split3_T(h);
            dvs_matb3<4>(U, hs, l.Wa, 64, 0, L);
            dvs_matb3<4>(V, hs, l.Wb, 64, 0, L);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) *(f4*)(scr + L.r * DVS_LD + 16 * t + 4 * L.g) = V[t];
        dvs_wave_sync();
        const unsigned par = rec->parents[(L.r + 1) & 15];
        float enll = 0.f;
        LSTAMP(3);               // U, V products + park
        // logit(i = r, j) for every j first — a plain multiply-add walk the compiler unrolls —, kept in registers (the 4 g lanes of
        // a row hold the same value); the BCE terms afterwards, lane g taking j = g, g + 4, ...: 4 instead of 13 (at n = 12) of the
        // exp / log pairs per lane, and those as hardware intrinsics (log1p's range handling costs ~40 instructions; the term is
        // in (0, ln 2], the absolute error of log(1 + e^-|x|) <= 1e-7 per pair against a per-DAG loss of O(10..100)).
        float logit[DVS_MAXTOK];
#pragma unroll
        for (int j = 0; j < DVS_MAXTOK - 2; ++j) {
            float e = 0.f;
            if (j < N - 2) {                               // uniform
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f4 vj = *(const f4*)(scr + j * DVS_LD + 16 * t + 4 * L.g);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) e += w2v[t][kk] * fmaxf(U[t][kk] + vj[kk], 0.f);
                }
            }
            logit[j] = dvs_sum_g(e) + b2;
        }
#pragma unroll
        for (int q = 0; q < (DVS_MAXTOK - 2 + 3) / 4; ++q) {
            // j = 4 q + g: pick this lane's logit with selects (no dynamic register indexing)
            float x = logit[4 * q];
            if (4 * q + 1 < DVS_MAXTOK - 2) x = L.g == 1 ? logit[4 * q + 1] : x;
            if (4 * q + 2 < DVS_MAXTOK - 2) x = L.g == 2 ? logit[4 * q + 2] : x;
            if (4 * q + 3 < DVS_MAXTOK - 2) x = L.g == 3 ? logit[4 * q + 3] : x;
            const int j = 4 * q + L.g;
            const bool pv = (j < N - 2) && (L.r > j) && (L.r <= N - 2);
            const float truth = (float)((par >> ((j + 1) & 31)) & 1u);
            const float bce = fmaxf(x, 0.f) - x * truth + __logf(1.0f + __expf(-fabsf(x)));
            enll += pv ? bce : 0.f;
        }
        dvs_wave_sync();
        LSTAMP(4);               // pair walk
        nll += enll;                       // every lane holds distinct pairs now
        nll = dvs_sum_wave(nll);
        if (L.lane == 0) a.dag_loss[(size_t)dag * 2] = nll;
        LSTAMP(5);               // reduction + store
    }
}

void dvs_launch_loss_fwd(const LossArgs& a, int grid, int nw, dvs_stream_t st) {
    const size_t lds = loss_lds_bytes(8, 1);
    DvsStagePlan plan;
    loss_plan(plan, a);
    DVS_SET_LDS(k_loss_fwd, lds);
    DVS_LAUNCH(k_loss_fwd, dim3(grid), dim3(nw == 4 ? 256 : 512), lds, st, a, plan);
}

// ---------------------------------------------------------------------------------------------------------
// Deterministic reduction of the per-DAG losses: recon = sum NLL, kld = sum KL, total = recon + beta * kld
// (pace.py:2030-2035).  losses[3] = 1 if anything is non-finite (replaces the per-layer isnan host sync,
// pace.py:97-98, by one device-side flag per step); losses[4] = 1 if the records' validation word is set.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_finalize(FinalizeArgs a) {
    __shared__ float s0[256], s1[256];
    float r = 0.f, k = 0.f;
    // two DAGs (= one 16-byte piece of the [B][2] array) per load, four loads in flight per pass: the loop used to pay one
    // memory round trip per DAG pair and thread (16 in a row at B = 4096: most of this kernel's 9 us)
    const int npair = a.B >> 1;
    const f4* dl4 = (const f4*)a.dag_loss;
    int i = threadIdx.x;
    for (; i + 3 * 256 < npair; i += 4 * 256) {
        f4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = dl4[i + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            r += v[u][0] + v[u][2];
            k += v[u][1] + v[u][3];
        }
    }
    for (; i < npair; i += 256) {
        const f4 v = dl4[i];
        r += v[0] + v[2];
        k += v[1] + v[3];
    }
    if ((a.B & 1) && threadIdx.x == 0) {
        r += a.dag_loss[(size_t)(a.B - 1) * 2];
        k += a.dag_loss[(size_t)(a.B - 1) * 2 + 1];
    }
    s0[threadIdx.x] = r;
    s1[threadIdx.x] = k;
    __syncthreads();
    dvs_block_sum256((int)threadIdx.x, s0, s1);
    if (threadIdx.x == 0) {
        const float recon = s0[0], kld = s1[0];
        const float total = recon + a.beta * kld;
        a.losses[0] = total;
        a.losses[1] = recon;
        a.losses[2] = kld;
        const float nonfinite = (total - total == 0.f) ? 0.f : 1.f;
        const int bits = a.status ? *a.status : 0;
        a.losses[3] = nonfinite;
        a.losses[4] = bits != 0 ? 1.f : 0.f;                        // invalid-features flag (travels with the scalars)
        if (a.host_tail) {
            // the host's copy, straight into pinned memory: no event, no copy, no side stream (an event recorded between the
            // forward and the backward cost the main stream ~12 us per step).  ONE 16-byte store = one write transaction: the
            // host reads the word that carries the sequence number first and the scalars after it (include/dvs.h); a version
            // with the sequence word in a store of its own needed the first stores acknowledged (s_waitcnt vmcnt(0): +4 us in
            // this kernel) or a system-scope fence (writes back the whole dirty L2 behind the forward)
            const uint32_t word = (a.host_seq << 8) | ((uint32_t)bits & 0x3Fu) | (nonfinite != 0.f ? 0x40u : 0u) | (bits != 0 ? 0x80u : 0u);
            f4 pkt;
            pkt[0] = total;
            pkt[1] = recon;
            pkt[2] = kld;
            pkt[3] = __uint_as_float(word);
            *(f4*)a.host_tail = pkt;
            if (a.status) *a.status = 0;                            // re-armed for the next pack
        }
    }
}

void dvs_launch_finalize(const FinalizeArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_finalize, dim3(1), dim3(256), 0, st, a);
}
