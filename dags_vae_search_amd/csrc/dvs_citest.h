// Constraint-based structure learning, next to the scorer whose counting it shares.  Included by k_bic.hip
// after dvs_cpdag.h.  Integer counts and fp64 arithmetic, every reduction in a fixed order, no atomics but the integer LDS
// histogram adds and the status atomicOr: two runs give equal bytes.
//
//   k_ci_tests       one workgroup per test (x, y | Z): the dense (z, x, y) table in dynamic LDS (max_cells * 4 bytes, sized
//                    per launch), laid out by bn_family_layout with Z for the parents and filled by bn_dense_count; the thread
//                    that owns configuration z forms its marginals and its partial sums; a fixed-order tree; thread 0 takes
//                    the p-value, Q(df / 2, statistic / 2).
//   k_pc_expand      one thread per test of a PC-stable level: its pair by binary search in the prefix offsets, its
//                    conditioning set by unranking in the combinatorial number system (u64 binomials, integers only).
//   k_pc_reduce_*    one wave per pair finds the lowest-index test with p > alpha and counts the refused ones; one workgroup
//                    then builds the next level's adjacency rows and the refused total.
//   k_pc_orient      one wave per structure, lane = variable: colliders from the separating sets, conflicts left undirected
//                    and counted, then pd_meek (dvs_cpdag.h), then the cycle check of the directed part.
#pragma once
#include "dvs_cpdag.h"               // pd_transpose, pd_meek

// ---------------------------------------------------------------------------------------------------------
// Q(a, x), the regularised upper incomplete gamma function: the series for P below a + 1, a modified Lentz continued
// fraction for Q above.  Both share the factor x^a e^-x / Gamma(a), taken through bn_lgamma.
// ---------------------------------------------------------------------------------------------------------
constexpr int CI_GAMMA_ITER = 20000;        // sqrt(a) terms are needed near x = a: a few hundred at a = 18 432

__device__ inline double ci_gamma_q(const double a, const double x) {
    if (!(x > 0.0)) return 1.0;
    const double lead = exp(a * log(x) - x - bn_lgamma(a));
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int i = 0; i < CI_GAMMA_ITER; ++i) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (del < sum * 1e-17) break;
        }
        return 1.0 - sum * lead;
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int i = 1; i <= CI_GAMMA_ITER; ++i) {
        const double an = -(double)i * ((double)i - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-15) break;
    }
    return lead * h;
}

// ---------------------------------------------------------------------------------------------------------
// The partial sums of one configuration z of a test: `cell` is its [rx][ry] block of counts, acc the statistic's sum and adf
// the adjusted degrees of freedom.  k_ci_tests and k_ci_group (dvs_local.h) both call it, and dvs_ci_tests_group promises the
// bytes of dvs_ci_tests, so what the compiler may or may not contract is stated: the G^2 term enters its sum by one fma on the
// device (the emulator build contracts nothing and has two roundings), whichever kernel it is inlined into.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ci_g2_add(const double acc, const double c, const double l) {
#ifdef DVS_EMU
    return acc + c * l;
#else
    return fma(c, l, acc);
#endif
}

__device__ __forceinline__ void ci_config_sums(const unsigned* cell, const int rx, const int ry, const bool g2, double& acc, int& adf) {
    unsigned col[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k] = 0u;
    unsigned n_z = 0u;
    for (int i = 0; i < rx; ++i) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < ry) {
                const unsigned c = cell[i * ry + k];
                col[k] += c;
                n_z += c;
            }
    }
    if (n_z == 0u) return;
    int rows_z = 0, cols_z = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) cols_z += (k < ry && col[k] != 0u) ? 1 : 0;
    const double dz = (double)n_z;
    for (int i = 0; i < rx; ++i) {
        unsigned n_xz = 0u;
        for (int k = 0; k < ry; ++k) n_xz += cell[i * ry + k];
        if (n_xz == 0u) continue;
        ++rows_z;
        const double dxz = (double)n_xz;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < ry && col[k] != 0u) {
                const double c = (double)cell[i * ry + k], dyz = (double)col[k];
                if (g2) {
                    if (c > 0.0) acc = ci_g2_add(acc, c, log((c * dz) / (dxz * dyz)));
                } else {
                    const double e = dxz * dyz / dz, d = c - e;
                    acc += d * d / e;
                }
            }
    }
    adf += (rows_z > 1 ? rows_z - 1 : 0) * (cols_z > 1 ? cols_z - 1 : 0);
}

// ---------------------------------------------------------------------------------------------------------
// k_ci_tests
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ci_tests(CiArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ double red[256];
    __shared__ int redi[256];
    __shared__ int z_id[48], z_stride[48];
    __shared__ int s_nz, s_q, s_ok;
    const size_t t = blockIdx.x;
    const int tid = threadIdx.x;
    const int x = a.pairs[2 * t], y = a.pairs[2 * t + 1];
    if (tid == 0) {
        const uint64_t zm = a.cond[t];
        bool ok = x >= 0 && y >= 0 && x < a.n && y < a.n && x != y && !((zm >> x) & 1ull) && !((zm >> y) & 1ull);
        if (ok) {
            const long long plane = (long long)a.card[x] * a.card[y];
            long long q = 0;
            const int nz = bn_family_layout(zm, a.n, a.card, plane, a.max_cells, z_id, z_stride, &q);
            ok = nz >= 0 && q * plane >= 1;                // a variable of no levels has no table
            s_nz = nz;
            s_q = (int)q;
        }
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) {
        if (tid == 0) {
            atomicOr(a.status, 16);
            a.out[3 * t] = bn_nan();
            a.out[3 * t + 1] = bn_nan();
            a.out[3 * t + 2] = bn_nan();
        }
        return;
    }
    const int nz = s_nz, q = s_q, rx = a.card[x], ry = a.card[y], plane = rx * ry, cells = q * plane;
    unsigned* hist = (unsigned*)smem;
    // guarded: a level code >= card is not counted, never written out of the table
    bn_dense_count<false, true>(hist, cells, a.data, a.words, a.S, nullptr, nz, z_id, z_stride, [&](const uint64_t* row, int key) {
        return (key * rx + bic_level(row, x)) * ry + bic_level(row, y);
    });
    const bool g2 = a.type == DVS_CI_MI || a.type == DVS_CI_MI_ADF;
    double acc = 0.0;
    int adf = 0;
    for (int j = tid; j < q; j += blockDim.x) ci_config_sums(hist + (size_t)j * plane, rx, ry, g2, acc, adf);
    red[tid] = acc;
    redi[tid] = adf;
    __syncthreads();
    dvs_block_sum256(tid, red, redi);
    if (tid == 0) {
        double stat = g2 ? 2.0 * red[0] : red[0];
        if (!(stat > 0.0)) stat = 0.0;
        const bool classic = a.type == DVS_CI_MI || a.type == DVS_CI_X2;
        const double df = classic ? (double)(rx - 1) * (double)(ry - 1) * (double)q : (double)redi[0];
        a.out[3 * t] = stat;
        a.out[3 * t + 1] = df;
        a.out[3 * t + 2] = df > 0.0 ? ci_gamma_q(0.5 * df, 0.5 * stat) : 1.0;
    }
}

void dvs_launch_ci_tests(const CiArgs& in, dvs_stream_t st) {
    CiArgs a = in;
    a.words = bic_words(a.n);
    const size_t lds = (size_t)a.max_cells * sizeof(unsigned);
    DVS_SET_LDS(k_ci_tests, lds);
    DVS_LAUNCH(k_ci_tests, dim3((unsigned)a.T), dim3(256), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// PC-stable: the tests of a level, and what they decide
// ---------------------------------------------------------------------------------------------------------
// C(c, k) in u64: exact for c <= 48 (every partial product is a binomial times at most 48)
__device__ __forceinline__ uint64_t pc_binom(const int c, int k) {
    if (k < 0 || k > c) return 0ull;
    if (k > c - k) k = c - k;
    uint64_t r = 1ull;
    for (int j = 1; j <= k; ++j) r = r * (uint64_t)(c - k + j) / (uint64_t)j;
    return r;
}

// the rank-th l-subset of the set bits of cand, in ascending numeric order of the masks (colex order of the positions)
__device__ __forceinline__ uint64_t pc_unrank(const uint64_t cand, const int l, uint64_t rank) {
    uint64_t m = 0ull;
    int bound = __popcll(cand);                              // positions still free: 0 .. bound - 1
    for (int i = l; i >= 1; --i) {
        int c = i - 1;                                       // C(i - 1, i) = 0 <= rank
        uint64_t below = 0ull;
        while (c + 1 < bound) {
            const uint64_t nb = pc_binom(c + 1, i);
            if (nb > rank) break;
            ++c;
            below = nb;
        }
        rank -= below;
        uint64_t rest = cand;
        for (int k = 0; k < c; ++k) rest &= rest - 1ull;     // drop the c lowest set bits
        m |= rest & (0ull - rest);
        bound = c;
    }
    return m;
}

// the tests of pair (x, y) at level l: those of side x first, then those of side y; level 0 has the one empty-set test
struct PcSides {
    uint64_t cx, cy, nx, ny;
};
__device__ __forceinline__ PcSides pc_sides(const uint64_t* adj, const int n, const int x, const int y, const int l) {
    PcSides s = {0ull, 0ull, 0ull, 0ull};
    if (x < 0 || y < 0 || x >= n || y >= n || x == y) return s;
    const uint64_t below_n = (1ull << n) - 1ull;             // n <= 48
    s.cx = adj[x] & below_n & ~(1ull << y) & ~(1ull << x);
    s.cy = adj[y] & below_n & ~(1ull << x) & ~(1ull << y);
    s.nx = pc_binom(__popcll(s.cx), l);
    s.ny = l == 0 ? 0ull : pc_binom(__popcll(s.cy), l);
    return s;
}

__global__ __launch_bounds__(256) void k_pc_expand(PcExpandArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    int lo = 0, hi = a.P - 1;                                // the last pair whose first test is <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const int x = a.pair_xy[2 * lo], y = a.pair_xy[2 * lo + 1];
    const PcSides s = pc_sides(a.adj, a.n, x, y, a.level);
    const long long r = t - a.offsets[lo];
    int ox = -1, oy = -1;                                    // offsets that do not match the rows: a test that is refused
    uint64_t z = 0ull;
    if (r >= 0 && (uint64_t)r < s.nx + s.ny) {
        ox = x;
        oy = y;
        z = (uint64_t)r < s.nx ? pc_unrank(s.cx, a.level, (uint64_t)r) : pc_unrank(s.cy, a.level, (uint64_t)r - s.nx);
    }
    a.pairs[2 * t] = ox;
    a.pairs[2 * t + 1] = oy;
    a.cond[t] = z;
}

void dvs_launch_pc_expand(const PcExpandArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_pc_expand, dim3((unsigned)((a.T + 255) / 256)), dim3(256), 0, st, a);
}

__global__ __launch_bounds__(256) void k_pc_reduce_pairs(PcReduceArgs a) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P) return;
    long long lo = a.offsets[p], hi = a.offsets[p + 1];
    if (lo < 0) lo = 0;
    if (hi > a.T) hi = a.T;
    const long long none = 0x7fffffffffffffffLL;
    long long first = none, refused = 0;
    for (long long i = lo + lane; i < hi; i += 64) {
        const double pv = a.out[3 * i + 2];
        if (pv != pv) ++refused;
        else if (pv > a.alpha && first == none) first = i;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {                       // min and sum in one butterfly
        const long long of = dvs_shfl_xor(first, lane, s);
        refused += dvs_shfl_xor(refused, lane, s);
        if (of < first) first = of;
    }
    if (lane == 0) {
        a.result[2 * (size_t)p] = first == none ? -1 : first;
        a.result[2 * (size_t)p + 1] = refused;
        const int x = a.pair_xy[2 * p], y = a.pair_xy[2 * p + 1];
        if (first != none && x >= 0 && y >= 0 && x < a.n && y < a.n) {
            const uint64_t z = a.cond[first];
            a.sepset[(size_t)x * a.n + y] = z;
            a.sepset[(size_t)y * a.n + x] = z;
        }
    }
}

constexpr int PC_MAX_PAIRS = 48 * 47 / 2;                    // dvs_pc_reduce refuses more

__global__ __launch_bounds__(256) void k_pc_reduce_rows(PcReduceArgs a) {
    __shared__ int redi[256];
    __shared__ unsigned char s_x[PC_MAX_PAIRS], s_y[PC_MAX_PAIRS];           // the separated pairs, 255 = not separated
    const int tid = threadIdx.x;
    long long r = 0;
    for (int p = tid; p < a.P; p += 256) {
        const int x = a.pair_xy[2 * p], y = a.pair_xy[2 * p + 1];
        const bool sep = a.result[2 * (size_t)p] >= 0 && x >= 0 && y >= 0 && x < a.n && y < a.n;
        s_x[p] = sep ? (unsigned char)x : 255;
        s_y[p] = sep ? (unsigned char)y : 255;
        r += a.result[2 * (size_t)p + 1];
    }
    __syncthreads();
    if (tid < a.n) {
        uint64_t row = a.adj[tid];
        for (int p = 0; p < a.P; ++p) {
            const int x = s_x[p], y = s_y[p];
            if (x == tid) row &= ~(1ull << y);
            if (y == tid) row &= ~(1ull << x);
        }
        a.adj_next[tid] = row;
    }
    redi[tid] = (int)(r > 0x7fffffffLL ? 0x7fffffffLL : r);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const long long sum = (long long)redi[tid] + redi[tid + s];
            redi[tid] = (int)(sum > 0x7fffffffLL ? 0x7fffffffLL : sum);
        }
        __syncthreads();
    }
    if (tid == 0) *a.refused = redi[0];
}

void dvs_launch_pc_reduce(const PcReduceArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_pc_reduce_pairs, dim3((unsigned)((a.P + 3) / 4)), dim3(256), 0, st, a);
    DVS_LAUNCH(k_pc_reduce_rows, dim3(1), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_pc_orient
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pc_orient(PcOrientArgs a) {
    __shared__ uint64_t s_adj[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x * 4 + wave;
    if (b >= a.B) return;
    const int n = a.n;
    const size_t base = (size_t)b * n;
    const bool live = lane < n;
    const uint64_t adj = live ? a.skeleton[base + lane] : 0ull;
    const uint64_t self = 1ull << lane, below_n = (1ull << n) - 1ull;           // n <= 48
    const uint64_t adj_t = pd_transpose(adj & below_n, n, lane);
    const bool illegal = __ballot(live && ((adj & (~below_n | self)) != 0ull || adj != adj_t)) != 0ull;
    if (illegal) {                                                               // wave-uniform
        if (lane == 0) {
            a.flags[b] = 2;
            a.conflicts[b] = 0;
        }
        if (live) a.pdag[base + lane] = 0ull;
        return;
    }
    s_adj[wave][lane] = adj;
    dvs_wave_sync();
    // colliders: x -> lane <- y for x, y adjacent to lane, not to each other, lane not in sepset[x][y]
    uint64_t C = 0ull;                                                           // claimed in: u -> lane
    const uint64_t* sep = a.sepsets + base * n;
    for (uint64_t xs = adj; xs; xs &= xs - 1ull) {
        const int x = dvs_ctz64(xs);
        for (uint64_t ys = adj & ~s_adj[wave][x] & ~(1ull << x); ys; ys &= ys - 1ull) {
            const int y = dvs_ctz64(ys);
            if (!((sep[(size_t)x * n + y] >> lane) & 1ull)) C |= 1ull << x;
        }
    }
    const uint64_t C_out = pd_transpose(C, n, lane);                             // claimed out: lane -> w
    const uint64_t both = C & C_out;                                             // claimed both ways: stays undirected
    int conf = __popcll(both & (self - 1ull));
    conf = dvs_wave_sum(conf, lane);
    uint64_t D = C & ~both;
    uint64_t U = adj & ~D & ~pd_transpose(D, n, lane);
    pd_meek(D, U, adj, s_adj[wave], n, lane);
    const uint64_t reach = bn_closure(D, n);
    const bool cyclic = __ballot(live && (reach & self) != 0ull) != 0ull;
    if (lane == 0) {
        a.flags[b] = cyclic ? 1 : 0;
        a.conflicts[b] = conf;
    }
    if (live) a.pdag[base + lane] = D | U;
}

void dvs_launch_pc_orient(const PcOrientArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_pc_orient, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, st, a);
}
