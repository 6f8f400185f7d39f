// K5 / K6 — GP-GNN gated propagation (block adjacency, L-hop propagation with fused head*tail
// gather, start-entity embeddings) and batched GraphConvolution.
//
// Replaces models/models.py:240-274 (and its copies :450-485, :660-694, :898-932),
// utils/context_utils.py:387-426 and models/layers.py:57-63.
//
// Propagation maths per graph b and channel c (a channel = one ordered entity pair):
//     h^l[c] = act(A_l h^l-1[c])         A_l [S,S], h [S]
// Channels never mix, so a workgroup owns (graph, chunk of <= 80 channels), keeps the channel
// states H^T [channels][S] resident in LDS for all L hops and streams each A_l exactly once from
// HBM straight into MFMA B-operand registers (v_mfma_f32_16x16x4_f32, exact fp32):
//     out^T[c][s] = sum_t H^T[c][t] * A[s][t]      M = channels, N = S, K = S
// Both operands are contiguous along the contraction index, so every lane fetches float4s and the
// K index is permuted consistently (k = 4*(lane>>4) + step) between the A- and B-fragments.
#include <math.h>
#include <stdlib.h>
#include "prop_common.h"

namespace recon {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// logical block index such that XCD x (blocks b with b % 8 == x) owns a contiguous chunk of the logical range
__device__ __forceinline__ int xcd_block(int b, int nb) {
    const int q = nb >> 3, r = nb & 7, x = b & 7, i = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ------------------------------------------------------------------------------- P1
__global__ void k_block_adj_fwd(const float* __restrict__ T, const float* __restrict__ I, int32_t B, int32_t n, int32_t dd,
                                float* __restrict__ A) {
    const int64_t S = 1LL * n * dd;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= B * S * S) return;
    const int col = static_cast<int>(idx % S), row = static_cast<int>((idx / S) % S);
    const int64_t b = idx / (S * S);
    const int i = row / dd, r = row % dd, j = col / dd, c = col % dd;
    float v;
    if (i == j) v = I[r * dd + c];
    else {
        const int e = i * (n - 1) + (j < i ? j : j - 1);
        v = T[(b * n * (n - 1) + e) * dd * dd + r * dd + c];
    }
    A[idx] = v;
}
__global__ void k_block_adj_bwd_T(const float* __restrict__ gA, int32_t B, int32_t n, int32_t dd, float* __restrict__ gT) {
    const int64_t S = 1LL * n * dd, Cn = 1LL * n * (n - 1), d2 = 1LL * dd * dd;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= B * Cn * d2) return;
    const int c = static_cast<int>(idx % dd), r = static_cast<int>((idx / dd) % dd);
    const int e = static_cast<int>((idx / d2) % Cn);
    const int64_t b = idx / (d2 * Cn);
    const int i = e / (n - 1);
    int j = e % (n - 1);
    if (j >= i) ++j;
    gT[idx] = gA[(b * S + i * dd + r) * S + j * dd + c];
}

// float4 variants for dd % 4 == 0 (every 4-float chunk lies inside one dd x dd block): grid = (chunks of one graph, B)
__global__ void __launch_bounds__(256) k_block_adj_fwd4(const float* __restrict__ T, const float* __restrict__ I, int32_t n, int32_t dd,
                                                        float* __restrict__ A) {
    const int S = n * dd, S4 = S >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= S * S4) return;
    const int b = blockIdx.y;
    const int row = t / S4, col = (t - row * S4) << 2;
    const int i = row / dd, r = row - i * dd, j = col / dd, c = col - j * dd;
    float4 v;
    if (i == j) v = *reinterpret_cast<const float4*>(I + r * dd + c);
    else {
        const int e = i * (n - 1) + (j < i ? j : j - 1);
        v = *reinterpret_cast<const float4*>(T + (static_cast<int64_t>(b) * n * (n - 1) + e) * dd * dd + r * dd + c);
    }
    *reinterpret_cast<float4*>(A + static_cast<int64_t>(b) * S * S + static_cast<int64_t>(row) * S + col) = v;
}
__global__ void __launch_bounds__(256) k_block_adj_bwd_T4(const float* __restrict__ gA, int32_t n, int32_t dd, float* __restrict__ gT) {
    const int S = n * dd, d2 = dd * dd, Cn = n * (n - 1);
    const int t = blockIdx.x * 256 + threadIdx.x;               // float4 index inside one graph's gT [Cn][dd][dd]
    if (t >= Cn * (d2 >> 2)) return;
    const int b = blockIdx.y;
    const int e = t / (d2 >> 2), rc = (t - e * (d2 >> 2)) << 2;
    const int r = rc / dd, c = rc - r * dd;
    const int i = e / (n - 1);
    int j = e - i * (n - 1);
    if (j >= i) ++j;
    const float4 v = *reinterpret_cast<const float4*>(gA + static_cast<int64_t>(b) * S * S + static_cast<int64_t>(i * dd + r) * S + j * dd + c);
    *reinterpret_cast<float4*>(gT + (static_cast<int64_t>(b) * Cn + e) * d2 + rc) = v;
}
// g_identity[r,c] = sum_{b,i} gA[b, i*dd+r, i*dd+c]; one block per (r,c), fixed-order tree
// d loss / d identity = sum over graphs b and diagonal positions i of the (i, i) block of gA.  Slice `blk` of the (b, i)
// pairs: thread e = (r, c) walks the slice's blocks (a wave reads 64-byte row pieces) with four independent chains and
// writes partial[blk][e]; k_sum_rows adds the slices in a fixed order.  (One workgroup per identity element,
// striding over all 9 216 blocks with 4-byte loads, fetched 300 MB for 9 MB of data.)
constexpr int kIdentSlices = 256;
__global__ void __launch_bounds__(256) k_block_adj_bwd_I(const float* __restrict__ gA, int32_t B, int32_t n, int32_t dd,
                                                         float* __restrict__ partial) {
    const int64_t S = 1LL * n * dd, pairs = 1LL * B * n;
    const int64_t per = (pairs + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = blockIdx.x * per, t1 = min(pairs, t0 + per);
    for (int e = threadIdx.x; e < dd * dd; e += 256) {
        const int r = e / dd, c = e % dd;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        auto at = [&](int64_t t) { const int64_t b = t / n; const int i = static_cast<int>(t % n); return gA[(b * S + i * dd + r) * S + i * dd + c]; };
        int64_t t = t0;
        for (; t + 4 <= t1; t += 4) { s0 += at(t); s1 += at(t + 1); s2 += at(t + 2); s3 += at(t + 3); }
        for (; t < t1; ++t) s0 += at(t);
        partial[static_cast<int64_t>(blockIdx.x) * dd * dd + e] = (s0 + s1) + (s2 + s3);
    }
}
// out[o] = sum_r partial[r][o]: 16 columns x 64 row groups per block, fixed-order LDS combine
__global__ void __launch_bounds__(1024) k_sum_rows(const float* __restrict__ partial, int32_t nrows, int32_t O, float* __restrict__ out) {
    __shared__ float red[64][17];
    const int c = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int o = blockIdx.x * 16 + c;
    const int per = (nrows + 63) / 64;
    const int r0 = grp * per, r1 = min(nrows, (grp + 1) * per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (o < O) {
        int r = r0;
        for (; r + 4 <= r1; r += 4) {
            s0 += partial[static_cast<int64_t>(r) * O + o];
            s1 += partial[static_cast<int64_t>(r + 1) * O + o];
            s2 += partial[static_cast<int64_t>(r + 2) * O + o];
            s3 += partial[static_cast<int64_t>(r + 3) * O + o];
        }
        for (; r < r1; ++r) s0 += partial[static_cast<int64_t>(r) * O + o];
    }
    red[grp][c] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (grp == 0 && o < O) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 64; ++g) t += red[g][c];
        out[o] = t;
    }
}

// ------------------------------------------------------------------------------- P4
__global__ void k_start_entity(const float* __restrict__ ent, const int64_t* __restrict__ pos, const float* __restrict__ templ,
                               int32_t B, int32_t n, int32_t d, float* __restrict__ out) {
    const int64_t S = 2LL * d * n, C = 1LL * n * (n - 1);
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= B * C * S) return;
    const int s = static_cast<int>(idx % S), c = static_cast<int>((idx / S) % C);
    const int64_t b = idx / (S * C);
    const int i = c / (n - 1);
    int j = c % (n - 1);
    if (j >= i) ++j;
    float v = 0.f;
    if (s >= 2 * d * i && s < 2 * d * i + d) v = ent[pos[(b * C + c) * 2 + 0] * d + (s - 2 * d * i)];
    else if (s >= 2 * d * j + d && s < 2 * d * (j + 1)) v = ent[pos[(b * C + c) * 2 + 1] * d + (s - 2 * d * j - d)];
    out[idx] = v * templ[c * S + s];
}

// rows [2][B C][d]: slot 0 = node i's first half-slot of (g * templ), slot 1 = node j's second half-slot; key [2][2 B C] = pos[..., slot]
__global__ void k_start_entity_bwd(const float* __restrict__ g, const int64_t* __restrict__ pos, const float* __restrict__ templ, int32_t B, int32_t n,
                                   int32_t d, float* __restrict__ rows, int64_t* __restrict__ key) {
    const int64_t S = 2LL * d * n, C = 1LL * n * (n - 1), BC = B * C;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= 2 * BC * d) return;
    const int k = static_cast<int>(idx % d);
    const int64_t r = idx / d;                                     // slot * BC + bc
    const int slot = r >= BC ? 1 : 0;
    const int64_t bc = r - slot * BC;
    const int c = static_cast<int>(bc % C);
    const int i = c / (n - 1);
    int j = c % (n - 1);
    if (j >= i) ++j;
    const int off = slot ? 2 * d * j + d : 2 * d * i;
    rows[idx] = g[bc * S + off + k] * templ[c * S + off + k];
    if (key && k == 0) { const int64_t e = pos[bc * 2 + slot]; key[r] = e; key[2 * BC + r] = e; }
}

// ------------------------------------------------------------------------------- P2 forward
template <bool VEC4>
__device__ __forceinline__ void load_a_row4(float (&v)[4], const float* A, int S, int row, int col, bool row_ok) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (!row_ok) return;
    const float* p = A + static_cast<int64_t>(row) * S + col;
    if constexpr (VEC4) {
        if (col < S) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (col + j < S) v[j] = p[j];
    }
}

// One wave per 16-wide column tile of H^T (up to 16 waves per block), ONE LDS buffer: every wave
// keeps its output tile in MFMA accumulators across the barrier that ends the hop's reads, then
// overwrites its own columns.  A rows are prefetched three 16-float slabs ahead, across hop boundaries.
template <int MT, bool VEC4>
__global__ void __launch_bounds__(1024) k_propagate_fwd(const PropK p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = blockDim.x >> 6;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int c0 = chunk * p.CC;
    const int pitch = p.pitch, S = p.S, CC = p.CC;
    const int NT = p.Sp >> 4;
    const bool dbl = NT > nwaves;                                  // S > 256: several passes, two buffers
    float* H = lds;                                                // state read by this hop
    float* Hn = dbl ? lds + static_cast<int64_t>(CC) * pitch : lds; // state written by this hop
    for (int idx = tid; idx < CC * pitch; idx += nthreads) {       // h^0 chunk, zero padded
        const int cl = idx / pitch, s = idx % pitch;
        const int c = c0 + cl;
        H[idx] = (c < p.C && s < S) ? p.h0[b * p.h0_bs + static_cast<int64_t>(c) * S + s] : 0.f;
    }
    __syncthreads();
    const int li = lane & 15, lq = lane >> 4;
    constexpr int G = 3;                                            // slabs per prefetch group
    const int ngroups = (NT + G - 1) / G;
    const int npass = (NT + nwaves - 1) / nwaves;
    // A rows are fetched one group of G slabs ahead of the MFMAs, ACROSS pass and hop boundaries (the rows of
    // the next hop's adjacency do not depend on the state), so HBM latency is never exposed at a barrier.
    auto fetch = [&](float (&dst)[G][4], int l, int pass, int grp) {
        const int nt = pass * nwaves + wave;
        const int row = 16 * nt + li;
        const bool ok = l < p.L && nt < NT && row < S;
        const float* A = p.adj[l < p.L ? l : 0] + static_cast<int64_t>(b) * S * S;
#pragma unroll
        for (int g = 0; g < G; ++g) load_a_row4<VEC4>(dst[g], A, S, row, 16 * (grp * G + g) + 4 * lq, ok && (grp * G + g) < NT);
    };
    float bq[G][4], bn[G][4];
    fetch(bq, 0, 0, 0);
    for (int l = 0; l < p.L; ++l) {
        for (int pass = 0; pass < npass; ++pass) {
            const int nt = pass * nwaves + wave;
            const bool tile_ok = nt < NT;                           // wave-uniform
            f32x4 acc[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int grp = 0; grp < ngroups; ++grp) {
                int nl = l, np = pass, ng = grp + 1;                // the step after this one
                if (ng == ngroups) { ng = 0; if (++np == npass) { np = 0; ++nl; } }
                fetch(bn, nl, np, ng);
                const int s0 = grp * G;
                if (tile_ok) {
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        if (s0 + g < NT) {
                            const int kc = 16 * (s0 + g) + 4 * lq;
                            float4 aq[MT];
#pragma unroll
                            for (int m = 0; m < MT; ++m) aq[m] = *reinterpret_cast<const float4*>(H + (16 * m + li) * pitch + kc);
                            // consecutive MFMAs hit DIFFERENT accumulators (dependent-accumulator latency is 40 cycles, issue 32)
#pragma unroll
                            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].x, bq[g][0], acc[m], 0, 0, 0);
#pragma unroll
                            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].y, bq[g][1], acc[m], 0, 0, 0);
#pragma unroll
                            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].z, bq[g][2], acc[m], 0, 0, 0);
#pragma unroll
                            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].w, bq[g][3], acc[m], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) bq[g][j] = bn[g][j];
            }
            if (!dbl) __syncthreads();                              // single buffer: all reads of H^{l-1} done
            // C layout: col (s) = lane&15, row (channel) = (lane>>4)*4 + r
            if (tile_ok) {
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Hn[(16 * m + 4 * lq + r) * pitch + 16 * nt + li] = act_fwd(acc[m][r], p.act);
            }
        }
        __syncthreads();
        if (dbl) { float* t = H; H = Hn; Hn = t; }                  // H now holds h^l
        // relation_l = gather(h, heads) * gather(h, tails)   (models/models.py:270-273)
        for (int idx = tid; idx < CC * p.dd; idx += nthreads) {
            const int cl = idx / p.dd, x = idx % p.dd;
            const int c = c0 + cl;
            if (c < p.C) {
                const int64_t io = b * p.idx_bs + static_cast<int64_t>(c) * p.dd + x;
                const int hi = static_cast<int>(p.head[io]), ti = static_cast<int>(p.tail[io]);
                p.out[(static_cast<int64_t>(b) * p.C + c) * (p.L * p.dd) + l * p.dd + x] = H[cl * pitch + hi] * H[cl * pitch + ti];
            }
        }
        if (p.hsave) {
            float* hs = p.hsave + ((static_cast<int64_t>(l) * p.B + b) * p.C) * S;
            for (int idx = tid; idx < CC * S; idx += nthreads) {
                const int cl = idx / S, s = idx % S;
                if (c0 + cl < p.C) hs[static_cast<int64_t>(c0 + cl) * S + s] = H[cl * pitch + s];
            }
        }
        // the next hop's post-compute barrier orders these reads before its writes
    }
}

// ------------------------------------------------------------------------------- P2 forward, wave-independent form
// Channels never mix, so ONE WAVE owns 16 channels of one graph for all L hops and needs no workgroup barrier:
// its state H^T [16][S] lives in REGISTERS as MFMA A-fragments (NT float4 per lane), every hop streams the whole
// A_l through B-fragment registers (the 4-5 waves of a graph re-read it from L2), and the hop's outputs go
// through a private LDS scratch [16][S+4] only to be re-laid out as next hop's A-fragments and for the
// head*tail gather.  Used when S <= 144 (NT <= 9 register fragments); larger S falls back to k_propagate_fwd.
template <int NT, bool VEC4>
__global__ void __launch_bounds__(256) k_propagate_fwd_w(const PropK p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NB = (NT >= 3) ? 3 : NT;                          // column tiles in flight (independent accumulators)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int MTn = (p.C + 15) >> 4;
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2); give every XCD a contiguous
    // chunk of units so that the waves of one graph, which stream the same A_l, hit the same L2 (PMC: 49 % L2 hits before)
    const int unit = xcd_block(blockIdx.x, gridDim.x) * 4 + wave;
    if (unit >= p.B * MTn) return;
    const int b = unit / MTn, m = unit % MTn;
    const int S = p.S, pitch = p.pitch;
    float* scr = lds + static_cast<int64_t>(wave) * 16 * pitch;
    const int li = lane & 15, lq = lane >> 4;
    const int cmine = 16 * m + li;                                  // channel whose row this lane holds as A-fragment
    float af[NT][4];
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const int k = 16 * s + 4 * lq;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            af[s][t] = (cmine < p.C && k + t < S) ? p.h0[b * p.h0_bs + static_cast<int64_t>(cmine) * S + k + t] : 0.f;
    }
    for (int l = 0; l < p.L; ++l) {
        const float* A = p.adj[l] + static_cast<int64_t>(b) * S * S;
#pragma unroll 1
        for (int nt0 = 0; nt0 < NT; nt0 += NB) {
            f32x4 acc[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            float bq[NB][4], bn[NB][4];
#pragma unroll
            for (int j = 0; j < NB; ++j) load_a_row4<VEC4>(bq[j], A, S, 16 * (nt0 + j) + li, 4 * lq, nt0 + j < NT && 16 * (nt0 + j) + li < S);
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                if (s + 1 < NT) {
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        load_a_row4<VEC4>(bn[j], A, S, 16 * (nt0 + j) + li, 16 * (s + 1) + 4 * lq, nt0 + j < NT && 16 * (nt0 + j) + li < S);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s][t], bq[j][t], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int t = 0; t < 4; ++t) bq[j][t] = bn[j][t];
            }
            // C layout: col (s) = lane&15, row (channel) = (lane>>4)*4 + r
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (nt0 + j < NT)
#pragma unroll
                    for (int r = 0; r < 4; ++r) scr[(4 * lq + r) * pitch + 16 * (nt0 + j) + li] = act_fwd(acc[j][r], p.act);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);                          // lgkmcnt(0): this wave's scratch writes have landed
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const float4 v = *reinterpret_cast<const float4*>(scr + li * pitch + 16 * s + 4 * lq);
            af[s][0] = v.x; af[s][1] = v.y; af[s][2] = v.z; af[s][3] = v.w;
        }
        // relation_l = gather(h, heads) * gather(h, tails)   (models/models.py:270-273)
        for (int idx = lane; idx < 16 * p.dd; idx += 64) {
            const int cl = idx / p.dd, x = idx % p.dd;
            const int c = 16 * m + cl;
            if (c < p.C) {
                const int64_t io = b * p.idx_bs + static_cast<int64_t>(c) * p.dd + x;
                const int hi = static_cast<int>(p.head[io]), ti = static_cast<int>(p.tail[io]);
                p.out[(static_cast<int64_t>(b) * p.C + c) * (p.L * p.dd) + l * p.dd + x] = scr[cl * pitch + hi] * scr[cl * pitch + ti];
            }
        }
        if (p.hsave) {
            float* hs = p.hsave + ((static_cast<int64_t>(l) * p.B + b) * p.C) * S;
            for (int idx = lane; idx < 16 * S; idx += 64) {
                const int cl = idx / S, sidx = idx % S;
                if (16 * m + cl < p.C) hs[static_cast<int64_t>(16 * m + cl) * S + sidx] = scr[cl * pitch + sidx];
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);                          // scratch reads done before the next hop overwrites it
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------- P2 backward (one hop per launch)
template <int MT, bool VEC4>
__global__ void __launch_bounds__(1024) k_propagate_bwd_hop(const PropBwdK p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = blockDim.x >> 6;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int c0 = chunk * p.CC;
    const int pitch = p.pitch, S = p.S, CC = p.CC;
    float* X = lds;                                       // H^l, later H^l-1
    float* Y = lds + static_cast<int64_t>(CC) * pitch;    // grad wrt H^l -> grad wrt pre-activation
    // VEC4 (S % 4 == 0, 16-byte aligned states, <= kStage 16-byte pieces per thread): every thread requests all its pieces of a
    // state at once, branch free (rows past C re-read row C - 1 and are zeroed on the way into LDS), so a phase is ONE round trip.
    // s_memtime stamps at cfg 3b with the row-by-row form below: of a workgroup's 92.6 k cycles 25.4 k went into this phase and
    // 14.2 k into the H^l-1 one — guarded 4-byte loads, one dependent round trip per row and 64-column step.
    constexpr int kStage = 4;
    const int nf4 = S >> 2, npieces = CC * nf4;
    const bool staged = VEC4 && npieces <= kStage * nthreads;
    auto stage = [&](const float* src0, int64_t row_stride, bool zero_all, float* dst) {      // dst[cl][0 .. pitch) = row c0 + cl of src0
        float4 v[kStage];
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            const int idx = min(tid + i * nthreads, npieces - 1);
            const int cl = idx / nf4, j = idx - cl * nf4;
            v[i] = *reinterpret_cast<const float4*>(src0 + static_cast<int64_t>(min(c0 + cl, p.C - 1)) * row_stride + 4 * j);
        }
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            const int idx = tid + i * nthreads;
            if (idx < npieces) {
                const int cl = idx / nf4, j = idx - cl * nf4;
                const bool ok = c0 + cl < p.C && !zero_all;
                *reinterpret_cast<float4*>(dst + cl * pitch + 4 * j) = ok ? v[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        for (int idx = tid; idx < CC * (pitch - S); idx += nthreads) {    // the pad columns S .. pitch
            const int cl = idx / (pitch - S), s = S + idx % (pitch - S);
            dst[cl * pitch + s] = 0.f;
        }
    };
    if (staged) {
        stage(p.Hl + static_cast<int64_t>(b) * p.C * S, S, false, X);
        stage(p.gH + static_cast<int64_t>(b) * p.C * S, S, p.first != 0, Y);
    } else {
        // one wave per channel row, lanes along s: coalesced, no per-element division
        for (int cl = wave; cl < CC; cl += nwaves) {
            const int c = c0 + cl;
            const int64_t g0 = (static_cast<int64_t>(b) * p.C + c) * S;
            for (int s = lane; s < pitch; s += 64) {
                const bool ok = c < p.C && s < S;
                X[cl * pitch + s] = ok ? p.Hl[g0 + s] : 0.f;
                Y[cl * pitch + s] = (ok && !p.first) ? p.gH[g0 + s] : 0.f;
            }
        }
    }
    __syncthreads();
    // relation gradient: d(h[head]*h[tail])
    for (int idx = tid; idx < CC * p.dd; idx += nthreads) {
        const int cl = idx / p.dd, x = idx % p.dd;
        const int c = c0 + cl;
        if (c < p.C) {
            const int64_t io = b * p.idx_bs + static_cast<int64_t>(c) * p.dd + x;
            const int hi = static_cast<int>(p.head[io]), ti = static_cast<int>(p.tail[io]);
            const float g = p.gout[(static_cast<int64_t>(b) * p.C + c) * (p.L * p.dd) + p.hop * p.dd + x];
            atomicAdd(&Y[cl * pitch + hi], g * X[cl * pitch + ti]);
            atomicAdd(&Y[cl * pitch + ti], g * X[cl * pitch + hi]);
        }
    }
    __syncthreads();
    for (int idx = tid; idx < CC * pitch; idx += nthreads) Y[idx] *= act_bwd(X[idx], p.act);
    __syncthreads();
    if (staged) {
        stage(p.Hprev + b * p.hprev_bs, S, false, X);
    } else {
        for (int cl = wave; cl < CC; cl += nwaves) {
            const int c = c0 + cl;
            const float* src = p.Hprev + b * p.hprev_bs + static_cast<int64_t>(c) * S;
            for (int s = lane; s < pitch; s += 64) X[cl * pitch + s] = (c < p.C && s < S) ? src[s] : 0.f;
        }
    }
    __syncthreads();
    const int li = lane & 15, lq = lane >> 4;
    const int NT = p.Sp >> 4;
    // (i) gA[s][t] = sum_c Y[c][s] * X[c][t]       (M = s, N = t, K = channel)
    // Work split.  (ii) gives column tile nt to wave nt (NT slabs x 4 x MT MFMAs); a tile of (i) costs CC/4 MFMAs, so NT
    // tiles of (i) weigh exactly one column of (ii): the waves beyond NT take NT tiles of (i) each while the first NT
    // waves run (ii), and whatever is left of (i) is dealt round-robin to everybody afterwards.  No barrier in between:
    // both products only read X, Y and A.
    const int wii = NT < nwaves ? NT : nwaves;                      // waves busy with (ii)
    const int nfree = nwaves - wii;
    const int tiles_a = p.gA ? min(NT * NT, nfree * NT) : 0;        // pass A: free waves only
    auto ga_tile = [&](int tile) {
        float* gA = p.gA + static_cast<int64_t>(b) * S * S;
        {
            const int ms = tile / NT, nt = tile % NT;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kc = 0; kc < CC; kc += 16) {
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int k = kc + 4 * lq + st;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Y[k * pitch + 16 * ms + li], X[k * pitch + 16 * nt + li], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * ms + 4 * lq + r, t = 16 * nt + li;
                if (s < S && t < S) {
                    if (p.chunks == 1) gA[static_cast<int64_t>(s) * S + t] = acc[r];
                    else atomicAdd(&gA[static_cast<int64_t>(s) * S + t], acc[r]);
                }
            }
        }
    };
    if (p.gA && wave >= wii)
        for (int tile = wave - wii; tile < tiles_a; tile += nfree) ga_tile(tile);
    // (ii) gHprev[c][t] = sum_s Y[c][s] * A[s][t]    (M = channel, N = t, K = s)
    {
        const float* A = p.A + static_cast<int64_t>(b) * S * S;
        for (int nt = wave; nt < NT; nt += nwaves) {
            f32x4 acc[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int col = 16 * nt + li;
            float bq[4], bn[4];
#pragma unroll
            for (int st = 0; st < 4; ++st) bq[st] = (4 * lq + st < S && col < S) ? A[static_cast<int64_t>(4 * lq + st) * S + col] : 0.f;
            for (int slab = 0; slab < NT; ++slab) {
                const int kc = 16 * slab + 4 * lq;
#pragma unroll
                for (int st = 0; st < 4; ++st)          // rows of the next slab are in flight during this slab's MFMAs
                    bn[st] = (slab + 1 < NT && kc + 16 + st < S && col < S) ? A[static_cast<int64_t>(kc + 16 + st) * S + col] : 0.f;
                float4 aq[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) aq[m] = *reinterpret_cast<const float4*>(Y + (16 * m + li) * pitch + kc);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].x, bq[0], acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].y, bq[1], acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].z, bq[2], acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[m].w, bq[3], acc[m], 0, 0, 0);
#pragma unroll
                for (int st = 0; st < 4; ++st) bq[st] = bn[st];
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = c0 + 16 * m + 4 * lq + r;
                    if (c < p.C && col < S) p.gH[(static_cast<int64_t>(b) * p.C + c) * S + col] = acc[m][r];
                }
        }
    }
    if (p.gA)
        for (int tile = tiles_a + wave; tile < NT * NT; tile += nwaves) ga_tile(tile);      // pass B: the rest of (i), all waves
}

struct PropGeom { int CC, Sp, pitch, chunks, MT, fwd_waves; size_t lds, fwd_lds; };
bool prop_geometry(int C, int S, PropGeom* g) {
    g->Sp = (S + 15) / 16 * 16;
    g->pitch = g->Sp + 4;
    const int Cp = (C + 15) / 16 * 16;
    int cc = Cp < 80 ? Cp : 80;                                     // <= 5 MFMA row tiles per block
    const size_t budget = static_cast<size_t>(cfg_int(CFG_PROP_LDS_KB, 150)) * 1024;      // S = 512: 32-channel chunks instead of 16 (half the re-reads of A_l)
    while (cc > 16 && 2ull * cc * g->pitch * sizeof(float) > budget) cc -= 16;
    if (2ull * cc * g->pitch * sizeof(float) > 160 * 1024) return false;
    g->CC = cc;
    g->MT = cc / 16;
    g->chunks = (C + cc - 1) / cc;
    g->lds = 2ull * cc * g->pitch * sizeof(float);                  // backward: two state buffers
    const int NT = g->Sp / 16;
    g->fwd_waves = NT < 16 ? NT : 16;                               // forward: one wave per column tile
    g->fwd_lds = (NT > 16 ? 2ull : 1ull) * cc * g->pitch * sizeof(float);
    return true;
}

int check_prop(const recon_prop_args* a) {
    if (!a) return RECON_ERR_INVALID;
    if (a->B < 0 || a->C <= 0 || a->S <= 0 || a->L <= 0 || a->dd <= 0) return RECON_ERR_INVALID;
    if (a->L > kMaxHops) return RECON_ERR_UNSUPPORTED;
    if (a->B > 65535) return RECON_ERR_UNSUPPORTED;
    if (a->act < 0 || a->act > 2) return RECON_ERR_INVALID;
    if (!a->h0 || !a->head_idx || !a->tail_idx || !a->out) return RECON_ERR_INVALID;
    if (a->trans) {                                                 // block mode: dd == 16, S = 16 n, C = n (n - 1)
        if (!a->identity) return RECON_ERR_INVALID;
        for (int l = 0; l < a->L; ++l) if (!a->trans[l]) return RECON_ERR_INVALID;
        const int n = a->S / 16;
        if (a->dd != 16 || a->S != 16 * n || a->C != n * (n - 1)) return RECON_ERR_UNSUPPORTED;
        return RECON_OK;
    }
    if (!a->adj) return RECON_ERR_INVALID;
    for (int l = 0; l < a->L; ++l) if (!a->adj[l]) return RECON_ERR_INVALID;
    return RECON_OK;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace recon

using namespace recon;

extern "C" int recon_block_adjacency_fwd(const float* T, const float* identity, int32_t B, int32_t n, int32_t dd, float* A,
                                         recon_stream_t stream) {
    if (B < 0 || n < 1 || dd < 1 || !identity || !A || (n > 1 && B > 0 && !T)) return RECON_ERR_INVALID;
    const int64_t total = 1LL * B * n * dd * n * dd;
    if (total == 0) return RECON_OK;
    const bool v4 = dd % 4 == 0 && B <= 65535 && !((reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(identity) | reinterpret_cast<uintptr_t>(A)) & 15);
    if (v4) hipLaunchKernelGGL(k_block_adj_fwd4, dim3(static_cast<unsigned>(ceil_div64(1LL * n * dd * n * dd / 4, 256)), static_cast<unsigned>(B)), dim3(256), 0,
                               as_stream(stream), T, identity, n, dd, A);
    else hipLaunchKernelGGL(k_block_adj_fwd, dim3(static_cast<unsigned>(ceil_div64(total, 256))), dim3(256), 0, as_stream(stream), T,
                            identity, B, n, dd, A);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" size_t recon_block_adjacency_bwd_workspace_floats(int32_t B, int32_t n, int32_t dd) {
    (void)B; (void)n;
    return static_cast<size_t>(kIdentSlices) * (dd > 0 ? dd : 1) * (dd > 0 ? dd : 1);
}

extern "C" int recon_block_adjacency_bwd(const float* gA, int32_t B, int32_t n, int32_t dd, float* gT, float* g_identity,
                                         float* workspace, recon_stream_t stream) {
    if (B < 0 || n < 1 || dd < 1 || !gA) return RECON_ERR_INVALID;
    if (g_identity && !workspace) return RECON_ERR_INVALID;
    hipStream_t st = as_stream(stream);
    const int64_t total = 1LL * B * n * (n - 1) * dd * dd;
    const bool v4 = dd % 4 == 0 && B <= 65535 && !((reinterpret_cast<uintptr_t>(gA) | reinterpret_cast<uintptr_t>(gT)) & 15);
    if (gT && total > 0) {
        if (v4) hipLaunchKernelGGL(k_block_adj_bwd_T4, dim3(static_cast<unsigned>(ceil_div64(1LL * n * (n - 1) * dd * dd / 4, 256)), static_cast<unsigned>(B)),
                                   dim3(256), 0, st, gA, n, dd, gT);
        else hipLaunchKernelGGL(k_block_adj_bwd_T, dim3(static_cast<unsigned>(ceil_div64(total, 256))), dim3(256), 0, st, gA, B, n, dd, gT);
    }
    if (g_identity) {
        const int64_t pairs = 1LL * B * n;
        const int slices = static_cast<int>(pairs < kIdentSlices ? (pairs > 0 ? pairs : 1) : kIdentSlices);
        hipLaunchKernelGGL(k_block_adj_bwd_I, dim3(slices), dim3(256), 0, st, gA, B, n, dd, workspace);
        hipLaunchKernelGGL(k_sum_rows, dim3(static_cast<unsigned>(ceil_div64(dd * dd, 16))), dim3(1024), 0, st, workspace, slices, dd * dd,
                           g_identity);
    }
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_start_entity_embeddings(const float* ent, const int64_t* pos, const float* templ, int32_t B, int32_t n,
                                             int32_t d, float* out, recon_stream_t stream) {
    if (B < 0 || n < 2 || d < 1 || !ent || !pos || !templ || !out) return RECON_ERR_INVALID;
    const int64_t total = 1LL * B * n * (n - 1) * 2 * d * n;
    if (total == 0) return RECON_OK;
    hipLaunchKernelGGL(k_start_entity, dim3(static_cast<unsigned>(ceil_div64(total, 256))), dim3(256), 0, as_stream(stream), ent, pos,
                       templ, B, n, d, out);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_start_entity_embeddings_bwd(const float* grad_out, const int64_t* pos, const float* templ, int32_t B, int32_t n, int32_t d,
                                                 float* rows, int64_t* key, recon_stream_t stream) {
    if (B < 0 || n < 2 || d < 1 || !grad_out || !pos || !templ || !rows) return RECON_ERR_INVALID;
    const int64_t total = 2LL * B * n * (n - 1) * d;
    if (total == 0) return RECON_OK;
    hipLaunchKernelGGL(k_start_entity_bwd, dim3(static_cast<unsigned>(ceil_div64(total, 256))), dim3(256), 0, as_stream(stream), grad_out, pos, templ, B,
                       n, d, rows, key);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

static bool prop_h_form_env() {
    const char* form = cfg(CFG_PROP_FWD);
    return !form || form[0] == 'h' || form[0] == '\0';
}

#define PROP_KEYS_MT(M_, FAM_) M_(FAM_, 1, true) M_(FAM_, 1, false) M_(FAM_, 2, true) M_(FAM_, 2, false) M_(FAM_, 3, true) M_(FAM_, 3, false) \
                               M_(FAM_, 4, true) M_(FAM_, 4, false) M_(FAM_, 5, true) M_(FAM_, 5, false)

// What recon_propagate_fwd launches for `a`: the kernel arguments, the geometry of the fp32 forms and the instance key (0: B == 0,
// nothing to launch).  Host arithmetic only — pointers are looked at for alignment — so recon_propagate_instance can ask it without
// a device.  Returns RECON_OK or the error the call answers with.
static int plan_fwd(const recon_prop_args* a, PropK& p, PropGeom& g, int32_t* key) {
    *key = -1;
    int rc = check_prop(a);
    if (rc != RECON_OK) return rc;
    if (a->B == 0) { *key = 0; return RECON_OK; }
    if (!prop_geometry(a->C, a->S, &g)) return RECON_ERR_UNSUPPORTED;
    bool v4 = (a->S % 4) == 0;
    const bool blk = a->trans != nullptr;
    for (int l = 0; l < kMaxHops; ++l) {
        p.adj[l] = (l < a->L && !blk) ? a->adj[l] : nullptr;
        p.trans[l] = (l < a->L && blk) ? a->trans[l] : nullptr;
        if (l < a->L && !al16(blk ? a->trans[l] : a->adj[l])) v4 = false;
    }
    p.identity = blk ? a->identity : nullptr;
    p.h0 = a->h0; p.h0_bs = a->h0_batch_stride; p.head = a->head_idx; p.tail = a->tail_idx; p.idx_bs = a->idx_batch_stride;
    p.out = a->out; p.hsave = a->h_saved;
    p.B = a->B; p.C = a->C; p.S = a->S; p.L = a->L; p.dd = a->dd; p.act = a->act;
    p.CC = g.CC; p.Sp = g.Sp; p.pitch = g.pitch;
    p.stats = a->h_saved ? a->stats : nullptr;
    p.ws = a->split_ws; p.ws_bytes = a->split_ws_bytes;
    // default: two-term half operands on the f16 matrix cores (prop_h.hip) wherever that form exists; RECON_PROP_FWD = w | b selects
    // one of the fp32 MFMA forms below (per wave / per workgroup), h forces the default
    if (prop_h_form_env()) {
        if ((*key = prop_fwd_h_key(p)) >= 0) return RECON_OK;
        if ((*key = prop_fwd_hl_key(p)) >= 0) return RECON_OK;          // wide states, given a workspace
    }
    if (blk) return RECON_ERR_UNSUPPORTED;                              // the other forms need a materialised adjacency
    const int NTn = g.Sp / 16;
    if (NTn <= 9 && cfg_char(CFG_PROP_FWD) != 'b')        // wave-independent form (RECON_PROP_FWD=w, or shapes the f16 forms do not take)
        *key = prop_key(PF_WAVE, NTn, 0, v4);
    else
        *key = prop_key(PF_BLOCK, g.MT, 0, v4);
    return RECON_OK;
}

extern "C" int32_t recon_propagate_instance(const recon_prop_args* a) {
    PropK p;
    PropGeom g;
    int32_t key;
    return plan_fwd(a, p, g, &key) == RECON_OK ? key : -1;
}

extern "C" int recon_propagate_fwd(const recon_prop_args* a, recon_stream_t stream) {
    PropK p;
    PropGeom g;
    int32_t key;
    const int rc = plan_fwd(a, p, g, &key);
    if (rc != RECON_OK) return rc;
    if (key == 0) return RECON_OK;
    hipStream_t st = as_stream(stream);
    if (prop_key_family(key) == PF_H) return prop_fwd_h(p, st);
    if (prop_key_family(key) == PF_HL) return prop_fwd_hl(p, st);
    const int64_t units = 1LL * a->B * ((a->C + 15) / 16);
    const dim3 wgrid(static_cast<unsigned>(ceil_div64(units, 4)));
    const size_t wlds = 4ull * 16 * g.pitch * sizeof(float);
    const dim3 grid(static_cast<unsigned>(g.chunks), static_cast<unsigned>(a->B));
#define CALL_W(FAM_, N_, V_) case prop_key(FAM_, N_, 0, V_): hipLaunchKernelGGL((k_propagate_fwd_w<N_, V_>), wgrid, dim3(256), wlds, st, p); break;
#define CALL_BLK(FAM_, M_, V_)                                                                                               \
    case prop_key(FAM_, M_, 0, V_):                                                                                          \
        if (g.fwd_lds > 64 * 1024)                                                                                           \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_propagate_fwd<M_, V_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                      static_cast<int>(g.fwd_lds));                                                          \
        hipLaunchKernelGGL((k_propagate_fwd<M_, V_>), grid, dim3(64 * g.fwd_waves), g.fwd_lds, st, p);                       \
        break;
    switch (key) {
        PROP_KEYS_MT(CALL_W, PF_WAVE)
        CALL_W(PF_WAVE, 6, true) CALL_W(PF_WAVE, 6, false) CALL_W(PF_WAVE, 7, true) CALL_W(PF_WAVE, 7, false) CALL_W(PF_WAVE, 8, true) CALL_W(PF_WAVE, 8, false)
        CALL_W(PF_WAVE, 9, true) CALL_W(PF_WAVE, 9, false)
        PROP_KEYS_MT(CALL_BLK, PF_BLOCK)
        default: return RECON_ERR_UNSUPPORTED;
    }
#undef CALL_W
#undef CALL_BLK
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" size_t recon_propagate_ws_bytes(const recon_prop_args* a) {
    if (!a || !prop_h_form_env() || (a->S % 4) != 0 || a->dd < 1) return 0;
    if (a->trans && (a->dd != 16 || a->S % 16 != 0 || a->C != (a->S / 16) * (a->S / 16 - 1))) return 0;
    return prop_hl_ws_bytes(a->B, a->S, a->L);
}

extern "C" size_t recon_propagate_identity_ws_floats(int32_t dd) {
    return static_cast<size_t>(prop_h_grid(1 << 30)) * (dd > 0 ? dd : 1) * (dd > 0 ? dd : 1);
}

extern "C" int recon_propagate_form(const recon_prop_args* a) {
    if (!a || a->B < 0 || a->C <= 0 || a->S <= 0 || a->L <= 0 || a->L > kMaxHops || a->dd <= 0 || !a->h0) return 0;
    PropGeom g;
    if (!prop_geometry(a->C, a->S, &g)) return 0;
    PropK p{};
    for (int l = 0; l < kMaxHops; ++l) p.adj[l] = nullptr;              // the adjacency pointers' alignment is checked at the call
    p.h0 = a->h0; p.h0_bs = a->h0_batch_stride; p.hsave = nullptr;
    p.B = a->B; p.C = a->C; p.S = a->S; p.L = 0; p.dd = a->dd; p.pitch = g.pitch;
    if (!(prop_h_form_env() && prop_fwd_h_supported(p))) return 0;
    return prop_bwd_h_shape_ok(a->C, a->S) ? 3 : 1;                     // bit 1: the backward's two-term form exists for this shape too
}

// ------------------------------------------------------------------------------- P2 backward for wide states (S > 160)
// At S = 512, C = 992 neither product of a hop fits a workgroup's LDS with all channels, and the channel-chunked kernel above pays for
// it (d A_l needs every channel: chunks meet in atomics; A_l is re-read per chunk).  Written as what they are, both products are plain
// batched GEMMs over the graphs, on the library's own fp32 matrix-core GEMM (gemm_f32.hip):
//     (d)  G_l[b]   = Y_l[b] [C x S] . A_l[b] [S x S]              -> d loss / d H^l-1 before the relation term
//     (c)  dA_l[b]  = Y_l[b]^T [S x C] . H^l-1[b] [C x S]
// with Y_l = (G_l+1 + relation gradient of hop l) . act'(H^l) produced in place by k_prop_bwd_post (one wave per (graph, channel) row:
// the row in LDS, the 2 dd scatter terms as LDS float atomics, act', one pass).  Needs one [B, C, S] workspace besides g_h.
namespace {
__global__ void __launch_bounds__(256) k_prop_bwd_post(const float* __restrict__ G, const float* __restrict__ Hl, const int64_t* __restrict__ head,
                                                        const int64_t* __restrict__ tail, int64_t idx_bs, const float* __restrict__ gout, float* __restrict__ Y,
                                                        int64_t rows, int32_t C, int32_t S, int32_t L, int32_t dd, int32_t hop, int32_t act) {
    extern __shared__ float rowbuf[];                                   // [4][S]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + w;
    if (row >= rows) return;
    const int64_t b = row / C;
    const int c = static_cast<int>(row - b * C);
    float* buf = rowbuf + w * S;
    const float* g = G ? G + row * S : nullptr;
    const float* h = Hl + row * S;
    for (int t = lane; t < S; t += 64) buf[t] = g ? g[t] : 0.f;
    __builtin_amdgcn_s_waitcnt(0xc07f);                                 // this wave's LDS writes have landed (one wave per row: no barrier)
    const int64_t io = b * idx_bs + static_cast<int64_t>(c) * dd;
    const float* go = gout + row * (static_cast<int64_t>(L) * dd) + static_cast<int64_t>(hop) * dd;
    for (int x = lane; x < dd; x += 64) {                               // out = h[head] * h[tail]  (models/models.py:270-273)
        const int hi = static_cast<int>(head[io + x]), ti = static_cast<int>(tail[io + x]);
        const float gv = go[x];
        atomicAdd(buf + hi, gv * h[ti]);
        atomicAdd(buf + ti, gv * h[hi]);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    float* y = Y + row * S;
    for (int t = lane; t < S; t += 64) y[t] = buf[t] * act_bwd(h[t], act);
}

int prop_bwd_wide(const recon_prop_args* a, const recon_prop_bwd_args* ba, hipStream_t st) {
    const int32_t B = a->B, C = a->C, S = a->S, L = a->L;
    const int64_t CS = 1LL * C * S, BCS = CS * B, rows = 1LL * B * C;
    // the last product must land in g_h: the L products alternate between the two buffers
    float* bufY = (L & 1) ? ba->wide_ws : ba->g_h;                      // holds Y_L first
    float* bufG = (L & 1) ? ba->g_h : ba->wide_ws;
    const dim3 pgrid(static_cast<unsigned>(ceil_div64(rows, 4)));
    const size_t plds = 4ull * S * sizeof(float);
    hipLaunchKernelGGL(k_prop_bwd_post, pgrid, dim3(256), plds, st, nullptr, a->h_saved + static_cast<int64_t>(L - 1) * BCS, a->head_idx, a->tail_idx,
                       a->idx_batch_stride, ba->grad_out, bufY, rows, C, S, L, a->dd, L - 1, a->act);
    for (int l = L; l >= 1; --l) {
        const float* Hprev = l == 1 ? a->h0 : a->h_saved + static_cast<int64_t>(l - 2) * BCS;
        const int64_t hprev_bs = l == 1 ? a->h0_batch_stride : CS;
        GemmBatch bt;
        bt.batch = B; bt.epilogue = 0;
        if (ba->g_adj && ba->g_adj[l - 1]) {                            // (c): A = Y_l as [K = c][M = s], B = H^l-1 as [K = c][N = t]
            bt.a_bs = CS; bt.b_bs = hprev_bs; bt.c_bs = 1LL * S * S;
            const int rc = gemm_f32_batched(S, S, C, plain_operand(bufY, S), false, plain_operand(Hprev, S), false, plain_output(ba->g_adj[l - 1], S), bt, 1,
                                            nullptr, st);
            if (rc != RECON_OK) return rc;
        }
        {                                                               // (d): A = Y_l [M = c][K = s], B = A_l as [K = s][N = t]
            bt.a_bs = CS; bt.b_bs = 1LL * S * S; bt.c_bs = CS;
            const int rc = gemm_f32_batched(C, S, S, plain_operand(bufY, S), true, plain_operand(a->adj[l - 1], S), false, plain_output(bufG, S), bt, 1,
                                            nullptr, st);
            if (rc != RECON_OK) return rc;
        }
        if (l > 1)
            hipLaunchKernelGGL(k_prop_bwd_post, pgrid, dim3(256), plds, st, bufG, a->h_saved + static_cast<int64_t>(l - 2) * BCS, a->head_idx, a->tail_idx,
                               a->idx_batch_stride, ba->grad_out, bufG, rows, C, S, L, a->dd, l - 2, a->act);
        float* t = bufY; bufY = bufG; bufG = t;
    }
    if (hipGetLastError() != hipSuccess) return RECON_ERR_LAUNCH;
    return RECON_OK;
}

// The same backward with the chain G_{l-1} = Y_l A_l, Y_{l-1} = (G_{l-1} + relation gradient) . act'(H^{l-1}) on the forward's two-term f16 kernel
// (prop_hl.hip: k_propagate_fwd_hl<.., true> over the TRANSPOSED adjacencies, all L steps of a slice of graphs in one launch — no G round
// trip, no row kernel between the hops); the Y_l leave as fp32 and feed the d A_l products.  Needs the gather indices as blocks of 16 columns
// (GP-GNN's: utils/embedding_utils.py:184-202), the forward's split workspace and L slices of [G, C, S] floats.
int prop_bwd_wide_chain(const recon_prop_args* a, const recon_prop_bwd_args* ba, hipStream_t st) {
    const int32_t B = a->B, C = a->C, S = a->S, L = a->L;
    const int64_t CS = 1LL * C * S, BCS = CS * B;
    const bool blk = a->trans != nullptr;                               // block mode: transition tensors read / d T written in place, no adjacency
    const int nn = S / 16;
    const int64_t G = prop_bwd_hl_slice(C, S, L, a->split_ws_bytes, B);
    if (G <= 0) return RECON_ERR_UNSUPPORTED;
    float* diag_ws = blk ? ba->chain_ws + prop_bwd_hl_ws_floats(C, S, L, G) : nullptr;      // [L][B][n][256]
    const bool want_ident = blk && ba->g_identity;
    for (int64_t g0 = 0; g0 < B; g0 += G) {
        const int32_t Gs = static_cast<int32_t>(B - g0 < G ? B - g0 : G);
        PropBwdHL c{};
        c.G = Gs; c.C = C; c.S = S; c.L = L; c.dd = a->dd; c.act = a->act; c.ws = a->split_ws; c.ws_bytes = a->split_ws_bytes;
        c.gout = ba->grad_out + g0 * C * L * a->dd; c.hblk = ba->head_blk; c.tblk = ba->tail_blk;
        c.identity = blk ? a->identity : nullptr;
        float* y_in; unsigned char* planes; float* isg; size_t pset, iset;
        prop_bwd_hl_ws_layout(C, S, L, G, ba->chain_ws, &y_in, &planes, &isg, &pset, &iset);
        c.yplanes = planes; c.yisg = isg;
        c.y_in = nullptr;
        c.hlast = a->h_saved + static_cast<int64_t>(L - 1) * BCS + g0 * CS;  // Y_L = relation gradient of the last hop . act'(H^L), formed by the chain kernel
        for (int k = 0; k < L; ++k) {
            const int l = L - k;
            c.adj_step[k] = blk ? a->trans[l - 1] + g0 * C * 256 : a->adj[l - 1] + g0 * S * S;
            c.hmask[k] = l >= 2 ? a->h_saved + static_cast<int64_t>(l - 2) * BCS + g0 * CS : nullptr;
            c.ysave[k] = l >= 2 ? nullptr : ba->g_h + g0 * CS;           // the Y_l leave as fragment planes
            c.gout_off[k] = l >= 2 ? (l - 2) * a->dd : 0;
        }
        int rc = prop_bwd_hl_chain(c, st);
        if (rc != RECON_OK) return rc;
        for (int k = 0; k < L; ++k) {                                   // d A_l[b] = Y_l[b]^T [S x C] . H^l-1[b] [C x S]
            const int l = L - k;
            float* gA = (!blk && ba->g_adj) ? ba->g_adj[l - 1] : nullptr;
            float* gT = (blk && ba->g_trans) ? ba->g_trans[l - 1] : nullptr;
            if (!gA && !gT && !want_ident) continue;
            const float* Hprev = l == 1 ? a->h0 + g0 * a->h0_batch_stride : a->h_saved + static_cast<int64_t>(l - 2) * BCS + g0 * CS;
            // NOTE: plane sets / scale sets are laid out for slices of G graphs; a short last slice uses the front of each set
            rc = prop_bwd_hl_gadj(planes + static_cast<size_t>(k) * (pset / G) * Gs, isg + static_cast<size_t>(k) * (iset / G) * Gs, Hprev,
                                  l == 1 ? a->h0_batch_stride : CS, gA ? gA + g0 * S * S : nullptr, gT ? gT + g0 * C * 256 : nullptr,
                                  blk ? diag_ws + (static_cast<int64_t>(l - 1) * B + g0) * nn * 256 : nullptr, Gs, C, S, st);
            if (rc != RECON_OK) return rc;
        }
    }
    if (want_ident)                                                     // d identity = the diagonal blocks of every hop, graph and node, fixed order
        hipLaunchKernelGGL(k_sum_rows, dim3(16), dim3(1024), 0, st, diag_ws, static_cast<int32_t>(1LL * L * B * nn), 256, ba->g_identity);
    if (hipGetLastError() != hipSuccess) return RECON_ERR_LAUNCH;
    return RECON_OK;
}
}  // namespace

extern "C" size_t recon_propagate_bwd_chain_ws_floats(const recon_prop_args* a) {
    if (!a || a->B <= 0 || a->dd != 16 || a->idx_batch_stride != 0 || !a->split_ws) return 0;
    if (a->trans && (!a->identity || a->S != 16 * (a->S / 16) || a->C != (a->S / 16) * (a->S / 16 - 1))) return 0;
    if (1LL * a->L * a->B * (a->S / 16) >= (1LL << 31)) return 0;
    const int64_t G = prop_bwd_hl_slice(a->C, a->S, a->L, a->split_ws_bytes, a->B);
    const bool off = cfg_char(CFG_PROP_BWD_CHAIN) == '0';
    if (G <= 0 || off) return 0;
    return prop_bwd_hl_ws_floats(a->C, a->S, a->L, G) + (a->trans ? static_cast<size_t>(a->L) * a->B * (a->S / 16) * 256 : 0);
}

extern "C" size_t recon_propagate_bwd_ws_floats(const recon_prop_args* a) {
    if (!a || a->trans || a->S <= 160 || a->B <= 0) return 0;
    return static_cast<size_t>(a->B) * a->C * a->S;
}

// What recon_propagate_bwd launches for `ba` (see plan_fwd): the instance key, the two-term form's arguments (PF_H) and the geometry
// of the per-hop kernel (PF_BWD_HOP).
static int plan_bwd(const recon_prop_bwd_args* ba, PropBwdH& q, PropGeom& g, int32_t* key) {
    *key = -1;
    if (!ba) return RECON_ERR_INVALID;
    const recon_prop_args* a = &ba->fwd;
    int rc = check_prop(a);
    if (rc != RECON_OK) return rc;
    if (!a->h_saved || !ba->grad_out || !ba->g_h) return RECON_ERR_INVALID;
    if (a->B == 0) { *key = 0; return RECON_OK; }
    const bool blk = a->trans != nullptr;
    if (a->S > 160 && ba->chain_ws && ba->head_blk && ba->tail_blk && recon_propagate_bwd_chain_ws_floats(a) > 0 &&
        cfg_char(CFG_PROP_BWD_WIDE) != '0') {
        // wide states, structured indices: chain + d A on the two-term f16 kernels (block mode too)
        *key = prop_bwd_hl_key(a->C, a->S, a->L, blk);
        return *key >= 0 ? RECON_OK : RECON_ERR_UNSUPPORTED;
    }
    if (a->stats && prop_h_form_env() && cfg_char(CFG_PROP_BWD) != 'f') {      // two-term f16 form (RECON_PROP_BWD=f: fp32 MFMA form)
        for (int l = 0; l < kMaxHops; ++l) {
            q.adj[l] = (l < a->L && !blk) ? a->adj[l] : nullptr; q.gadj[l] = (l < a->L && !blk && ba->g_adj) ? ba->g_adj[l] : nullptr;
            q.trans[l] = (l < a->L && blk) ? a->trans[l] : nullptr; q.gtrans[l] = (l < a->L && blk && ba->g_trans) ? ba->g_trans[l] : nullptr;
        }
        q.identity = blk ? a->identity : nullptr;
        q.gident_ws = (blk && ba->g_identity) ? ba->identity_ws : nullptr;
        if (blk && ba->g_identity && !ba->identity_ws) return RECON_ERR_INVALID;
        q.h0 = a->h0; q.h0_bs = a->h0_batch_stride; q.hsave = a->h_saved; q.head = a->head_idx; q.tail = a->tail_idx; q.idx_bs = a->idx_batch_stride;
        q.gout = ba->grad_out; q.gH = ba->g_h; q.stats = a->stats;
        q.B = a->B; q.C = a->C; q.S = a->S; q.L = a->L; q.dd = a->dd; q.act = a->act;
        if ((*key = prop_bwd_h_key(q)) >= 0) return RECON_OK;
        if (blk) return RECON_ERR_UNSUPPORTED;
    } else if (blk) return RECON_ERR_UNSUPPORTED;
    if (cfg_char(CFG_PROP_BWD_WIDE) != '0' && ba->wide_ws && a->S > 160 && 4ull * a->S * sizeof(float) <= 64 * 1024) {
        *key = prop_key(PF_BWD_GEMM, 0, 0, false);                      // wide states: both products as batched GEMMs
        return RECON_OK;
    }
    if (!prop_geometry(a->C, a->S, &g)) return RECON_ERR_UNSUPPORTED;
    // float4 staging of the states: every hop's H^l, H^l-1 (h0 for the first hop) and g_h 16-byte aligned — one instance for all hops
    const bool v4b = (a->S % 4) == 0 && al16(a->h_saved) && al16(a->h0) && al16(ba->g_h) && (a->h0_batch_stride % 4) == 0;
    *key = prop_key(PF_BWD_HOP, g.MT, 0, v4b);
    return RECON_OK;
}

extern "C" int32_t recon_propagate_bwd_instance(const recon_prop_bwd_args* ba) {
    PropBwdH q{};
    PropGeom g;
    int32_t key;
    return plan_bwd(ba, q, g, &key) == RECON_OK ? key : -1;
}

extern "C" int recon_propagate_bwd(const recon_prop_bwd_args* ba, recon_stream_t stream) {
    PropBwdH q{};
    PropGeom g;
    int32_t key;
    int rc = plan_bwd(ba, q, g, &key);
    if (rc != RECON_OK) return rc;
    if (key == 0) return RECON_OK;
    const recon_prop_args* a = &ba->fwd;
    hipStream_t st = as_stream(stream);
    const int fam = prop_key_family(key);
    if (fam == PF_HL_CHAIN8 || fam == PF_HL_CHAIN16) return prop_bwd_wide_chain(a, ba, st);
    if (fam == PF_H) {
        rc = prop_bwd_h(q, st);
        if (rc == RECON_OK && q.gident_ws)                              // per-workgroup partial sums -> g_identity, fixed order
            hipLaunchKernelGGL(k_sum_rows, dim3(16), dim3(1024), 0, st, q.gident_ws, prop_h_grid(a->B), 256, ba->g_identity);
        return rc;
    }
    if (fam == PF_BWD_GEMM) return prop_bwd_wide(a, ba, st);
    const int64_t BCS = 1LL * a->B * a->C * a->S;
    dim3 grid(static_cast<unsigned>(g.chunks), static_cast<unsigned>(a->B));
    for (int l = a->L; l >= 1; --l) {
        PropBwdK p;
        p.A = a->adj[l - 1];
        p.Hl = a->h_saved + static_cast<int64_t>(l - 1) * BCS;
        if (l == 1) { p.Hprev = a->h0; p.hprev_bs = a->h0_batch_stride; }
        else { p.Hprev = a->h_saved + static_cast<int64_t>(l - 2) * BCS; p.hprev_bs = 1LL * a->C * a->S; }
        p.head = a->head_idx; p.tail = a->tail_idx; p.idx_bs = a->idx_batch_stride;
        p.gout = ba->grad_out; p.gH = ba->g_h;
        p.gA = ba->g_adj ? ba->g_adj[l - 1] : nullptr;
        p.B = a->B; p.C = a->C; p.S = a->S; p.L = a->L; p.dd = a->dd; p.act = a->act;
        p.CC = g.CC; p.Sp = g.Sp; p.pitch = g.pitch; p.hop = l - 1; p.first = (l == a->L) ? 1 : 0; p.chunks = g.chunks;
        if (p.gA && g.chunks > 1 && hipMemsetAsync(p.gA, 0, sizeof(float) * a->B * a->S * a->S, st) != hipSuccess) return RECON_ERR_LAUNCH;
#define CALL_HOP(FAM_, M_, V_)                                                                                               \
    case prop_key(FAM_, M_, 0, V_):                                                                                          \
        if (g.lds > 64 * 1024 && l == a->L)                              /* once, ahead of the first hop's launch */          \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_propagate_bwd_hop<M_, V_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                      static_cast<int>(g.lds));                                                              \
        hipLaunchKernelGGL((k_propagate_bwd_hop<M_, V_>), grid, dim3(1024), g.lds, st, p);                                   \
        break;
        switch (key) {
            PROP_KEYS_MT(CALL_HOP, PF_BWD_HOP)
            default: return RECON_ERR_UNSUPPORTED;
        }
#undef CALL_HOP
        RECON_CHECK_LAUNCH();
    }
    return RECON_OK;
}

// ------------------------------------------------------------------------------- P5 / K6 GraphConvolution
namespace {

// Y[b][i][o] = epilogue( sum_j M[i][j] * Xin[b][j][o] ),  M = adj[b] (TRANS = false) or adj[b]^T (TRANS = true), on the
// matrix cores (v_mfma_f32_16x16x4_f32).  Block = (64-column tile, graph, 32-row tile); wave w owns 16 columns and both
// 16-row tiles; the contraction index is walked in chunks of 32 through LDS, so any n is accepted (n <= 32, the
// reference's regime, is one chunk and one row tile).
// MASK: Xin = gout * (fwd_out > 0)   (ReLU backward folded into the load)
// EPI : + bias, ReLU
// LDS images are k-major with pitches = 16 (mod 32) floats, so the two k groups a 32-lane read touches fall on disjoint
// banks.  (A VALU form with two LDS reads per four FMAs was LDS-issue bound: 37 us at cfg 3a for 80 MB of traffic.)
template <bool TRANS, bool MASK, bool EPI>
__global__ void __launch_bounds__(256) k_gcn_aggregate_mfma(const float* __restrict__ adj, const float* __restrict__ Xin,
                                                            const float* __restrict__ fwd_out, const float* __restrict__ bias,
                                                            int32_t n, int32_t O, float* __restrict__ Y) {
    constexpr int PM = 48, PX = 80;
    __shared__ float Mk[32 * PM];           // Mk[k][i] = M[i0 + i][k0 + k]
    __shared__ float Xs[32 * PX];           // Xs[k][o]
    const int b = blockIdx.y, o0 = blockIdx.x * 64, i0 = blockIdx.z * 32;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float* A = adj + static_cast<int64_t>(b) * n * n;
    const int li = lane & 15, lq = lane >> 4;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < n; k0 += 32) {
        if (k0) __syncthreads();
        for (int idx = t; idx < 32 * 32; idx += 256) {
            const int k = idx >> 5, i = idx & 31;
            float v = 0.f;
            if (k0 + k < n && i0 + i < n)
                v = TRANS ? A[static_cast<int64_t>(k0 + k) * n + i0 + i] : A[static_cast<int64_t>(i0 + i) * n + k0 + k];
            Mk[k * PM + i] = v;
        }
        for (int idx = t; idx < 32 * 64; idx += 256) {
            const int k = idx >> 6, o = o0 + (idx & 63);
            float v = 0.f;
            if (k0 + k < n && o < O) {
                const int64_t g = (static_cast<int64_t>(b) * n + k0 + k) * O + o;
                v = Xin[g];
                if constexpr (MASK) v = fwd_out[g] > 0.f ? v : 0.f;
            }
            Xs[k * PX + (idx & 63)] = v;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = 4 * s + lq;
            const float bx = Xs[k * PX + 16 * w + li];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(Mk[k * PM + li], bx, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(Mk[k * PM + 16 + li], bx, acc[1], 0, 0, 0);
        }
    }
    const int o = o0 + 16 * w + li;                                 // C layout: col = lane & 15, row = (lane >> 4) * 4 + r
    if (o < O) {
        const float bv = (EPI && bias) ? bias[o] : 0.f;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * tt + 4 * lq + r;
                if (i < n) {
                    float v = acc[tt][r];
                    if constexpr (EPI) { v += bv; v = v > 0.f ? v : 0.f; }
                    Y[(static_cast<int64_t>(b) * n + i) * O + o] = v;
                }
            }
    }
}

// g_adj[b][i][j] = sum_o gpre[b][i][o] * support[b][j][o]
__global__ void __launch_bounds__(256) k_gcn_grad_adj(const float* __restrict__ gout, const float* __restrict__ fwd_out,
                                                      const float* __restrict__ sup, int32_t n, int32_t O,
                                                      float* __restrict__ gadj) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx % n;
    const int64_t ri = (static_cast<int64_t>(b) * n + i) * O, rj = (static_cast<int64_t>(b) * n + j) * O;
    float s = 0.f;
    for (int o = 0; o < O; ++o) s = fmaf(fwd_out[ri + o] > 0.f ? gout[ri + o] : 0.f, sup[rj + o], s);
    gadj[static_cast<int64_t>(b) * n * n + idx] = s;
}

// g_bias[o] = sum_rows gpre[row][o]: per-block partial rows, then a fixed-order second pass
__global__ void __launch_bounds__(256) k_gcn_bias_partial(const float* __restrict__ gout, const float* __restrict__ fwd_out,
                                                          int64_t rows, int32_t O, int32_t rows_per_block,
                                                          float* __restrict__ partial) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= O) return;
    const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;                     // four independent chains: the loop is latency bound
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
        s0 += fwd_out[r * O + o] > 0.f ? gout[r * O + o] : 0.f;
        s1 += fwd_out[(r + 1) * O + o] > 0.f ? gout[(r + 1) * O + o] : 0.f;
        s2 += fwd_out[(r + 2) * O + o] > 0.f ? gout[(r + 2) * O + o] : 0.f;
        s3 += fwd_out[(r + 3) * O + o] > 0.f ? gout[(r + 3) * O + o] : 0.f;
    }
    for (; r < r1; ++r) s0 += fwd_out[r * O + o] > 0.f ? gout[r * O + o] : 0.f;
    partial[static_cast<int64_t>(blockIdx.y) * O + o] = (s0 + s1) + (s2 + s3);
}
int check_gcn(const recon_gcn_args* a) {
    if (!a || a->B < 0 || a->n <= 0 || a->in_features <= 0 || a->out_features <= 0) return RECON_ERR_INVALID;
    if (!a->x || !a->adj || !a->weight || !a->support || !a->out) return RECON_ERR_INVALID;
    if (a->B > 65535 || a->n > 65535 * 32) return RECON_ERR_UNSUPPORTED;      // grid.y = graphs, grid.z = 32-row tiles
    return RECON_OK;
}
constexpr int kBiasBlocks = 1024;

}  // namespace

static size_t gcn_split_part(int32_t rows, int32_t K) { return align_up(static_cast<size_t>(3) * rows * bx3_kp(K) * 2, 256); }
extern "C" size_t recon_gcn_split_bytes(int32_t in_features, int32_t out_features) {
    if (in_features <= 0 || out_features <= 0) return 256;
    return gcn_split_part(out_features, in_features) + gcn_split_part(in_features, out_features);
}

extern "C" int recon_gcn_fwd(const recon_gcn_args* a, recon_stream_t stream) {
    int rc = check_gcn(a);
    if (rc != RECON_OK) return rc;
    if (a->B == 0) return RECON_OK;
    hipStream_t st = as_stream(stream);
    const int32_t rows = a->B * a->n, I = a->in_features, O = a->out_features;
    // support = x @ W      (models/layers.py:58)
    GemmBatch one;
    one.batch = 1; one.a_bs = one.b_bs = one.c_bs = 0; one.epilogue = 0;
    const OperandDesc X = plain_operand(a->x, I);
    if (a->w_split && !(reinterpret_cast<uintptr_t>(a->w_split) & 15) && bx3_supported(X, I, one)) {
        // bf16 term planes of W^T [3][O][kp(I)] (this product) and of W [3][I][kp(O)] (g_x in the backward)
        char* ws = static_cast<char*>(a->w_split);
        rc = bx3_split_planes(a->weight, O, 0, true, O, I, 1, ws, st);
        if (rc == RECON_OK) rc = bx3_split_planes(a->weight, O, 0, false, I, O, 1, ws + gcn_split_part(O, I), st);
        if (rc == RECON_OK) rc = gemm_bx3_batched(rows, O, I, X, ws, plain_output(a->support, O), one, st);
    } else {
        rc = gemm_f32(rows, O, I, X, true, plain_operand(a->weight, O), false, plain_output(a->support, O), 1, nullptr, st);
    }
    if (rc != RECON_OK) return rc;
    // out = relu(adj @ support + bias)     (models/layers.py:59-63)
    dim3 grid(static_cast<unsigned>(ceil_div64(O, 64)), static_cast<unsigned>(a->B), static_cast<unsigned>(ceil_div64(a->n, 32)));
    hipLaunchKernelGGL((k_gcn_aggregate_mfma<false, false, true>), grid, dim3(256), 0, st, a->adj, a->support, nullptr, a->bias, a->n, O,
                       a->out);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" size_t recon_gcn_bwd_partial_floats(int32_t B, int32_t n, int32_t in_features, int32_t out_features) {
    size_t need = static_cast<size_t>(kBiasBlocks) * out_features;
    int sk = gemm_pick_split_k(in_features, out_features, B * n);
    const int sk3 = bx3_kmajor_splits(B * n, bx3_kmajor_split_k(in_features, out_features, B * n, 1));      // split-precision form
    if (sk3 > sk) sk = sk3;
    const size_t g = static_cast<size_t>(sk) * in_features * out_features;
    return g > need ? g : need;
}

extern "C" size_t recon_gcn_bwd_split_bytes(int32_t B, int32_t n, int32_t out_features) {
    if (B <= 0 || n <= 0 || out_features <= 0) return 256;
    return align_up(static_cast<size_t>(3) * B * n * bx3_kp(out_features) * 2, 256);
}

extern "C" int recon_gcn_bwd(const recon_gcn_bwd_args* b, recon_stream_t stream) {
    if (!b) return RECON_ERR_INVALID;
    const recon_gcn_args* a = &b->fwd;
    int rc = check_gcn(a);
    if (rc != RECON_OK) return rc;
    if (!b->grad_out || !b->g_support || !b->partial) return RECON_ERR_INVALID;
    if (a->B == 0) return RECON_OK;
    hipStream_t st = as_stream(stream);
    const int32_t rows = a->B * a->n, I = a->in_features, O = a->out_features, n = a->n;
    dim3 grid(static_cast<unsigned>(ceil_div64(O, 64)), static_cast<unsigned>(a->B), static_cast<unsigned>(ceil_div64(n, 32)));
    // g_support = adj^T @ (grad_out * (out > 0))
    hipLaunchKernelGGL((k_gcn_aggregate_mfma<true, true, false>), grid, dim3(256), 0, st, a->adj, b->grad_out, a->out, nullptr, n, O,
                       b->g_support);
    if (b->g_adj)
        hipLaunchKernelGGL(k_gcn_grad_adj, dim3(static_cast<unsigned>(ceil_div64(n * n, 256)), static_cast<unsigned>(a->B)), dim3(256), 0,
                           st, b->grad_out, a->out, a->support, n, O, b->g_adj);
    if (b->g_bias) {
        const int rpb = static_cast<int>(ceil_div64(rows, kBiasBlocks));
        const int nb = static_cast<int>(ceil_div64(rows, rpb));
        hipLaunchKernelGGL(k_gcn_bias_partial, dim3(static_cast<unsigned>(ceil_div64(O, 256)), static_cast<unsigned>(nb)), dim3(256), 0, st,
                           b->grad_out, a->out, static_cast<int64_t>(rows), O, rpb, b->partial);
        hipLaunchKernelGGL(k_sum_rows, dim3(static_cast<unsigned>(ceil_div64(O, 16))), dim3(1024), 0, st, b->partial, nb, O, b->g_bias);
    }
    RECON_CHECK_LAUNCH();
    // g_x = g_support @ W^T
    if (b->g_x) {
        GemmBatch one;
        one.batch = 1; one.a_bs = one.b_bs = one.c_bs = 0; one.epilogue = 0;
        const OperandDesc G = plain_operand(b->g_support, O);
        if (a->w_split && !(reinterpret_cast<uintptr_t>(a->w_split) & 15) && bx3_supported(plain_operand(a->x, I), I, one) &&
            bx3_supported(G, O, one))                                  // same condition as the forward, which filled the planes
            rc = gemm_bx3_batched(rows, I, O, G, static_cast<const char*>(a->w_split) + gcn_split_part(O, I), plain_output(b->g_x, I), one, st);
        else
            rc = gemm_f32(rows, I, O, G, true, plain_operand(a->weight, O), true, plain_output(b->g_x, I), 1, nullptr, st);
        if (rc != RECON_OK) return rc;
    }
    // g_W = x^T @ g_support   (split-K over the B*n rows, deterministic second pass)
    if (b->g_weight) {
        const int64_t ldp = bx3_kp(O);
        if (b->gs_split && a->w_split && !(reinterpret_cast<uintptr_t>(b->gs_split) & 15) && bx3_kmajor_supported(a->x, I, 0, ldp, 0, I, O)) {
            // split-precision, both operands k-major: x split on the fly, g_support from its bf16 term planes
            rc = bx3_split_planes(b->g_support, O, 0, false, rows, O, 1, b->gs_split, st);
            const int sk = bx3_kmajor_splits(rows, bx3_kmajor_split_k(I, O, rows, 1));
            if (rc == RECON_OK) rc = gemm_bx3_kmajor_batched(I, O, rows, a->x, I, 0, b->gs_split, ldp, static_cast<int64_t>(rows) * ldp, 0, 1, sk, b->partial, st);
            if (rc == RECON_OK) rc = splitk_reduce(b->partial, sk, I, O, plain_output(b->g_weight, O), 0, 1, 0, false, st);
        } else {
            const int sk = gemm_pick_split_k(I, O, rows);
            rc = gemm_f32(I, O, rows, plain_operand(a->x, I), false, plain_operand(b->g_support, O), false, plain_output(b->g_weight, O), sk,
                          b->partial, st);
        }
        if (rc != RECON_OK) return rc;
    }
    return RECON_OK;
}
