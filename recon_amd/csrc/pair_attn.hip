// E16 — ContextAware's "attention over ghosts" (models/baselines.py:86-112) as one device op.  R = states [B][C][D], Mem = R W^T
// (pair_trans.hip's product, not formed here):
//     S[b][i][j]  = Mem[b][i] . R[b][j]                 j != i
//     P[b][i][:]  = softmax over j != i of S[b][i][j],  P[b][i][i] = 0
//     ctx[b][i]   = sum_j P[b][i][j] R[b][j]
//     out[b][i]   = (R[b][i] | ctx[b][i])               [B][C][2 D]
// and its backward from g_out = (g_left | g_ctx):
//     T[i][j] = g_ctx[i] . R[j],  r[i] = sum_j P[i][j] T[i][j],  g_S = P (T - r)
//     g_Mem[i] = sum_j g_S[i][j] R[j]
//     g_R[j]   = g_left[j] + sum_i P[i][j] g_ctx[i] + sum_i g_S[i][j] Mem[i]
// Everything is fp32 on v_mfma_f32_16x16x4_f32, without atomics, every sum in an order the shape alone decides.
//
// Forward, one launch: workgroup (sentence b, tile of 16 target pairs).  Phase 1 forms the 16 x C score tile as a product over D, 64 k per
// step, both operands staged through LDS (the next step's rows wait in registers while this one is multiplied); wave w owns the column
// tiles w, w + 4, w + 8.  Phase 2 is the row softmax, 16 lanes per row.  Phase 3 forms ctx = P R over 64 columns of D per step, R's rows
// staged in LDS, P read from LDS; wave w owns 16 of the 64 columns.  k_pa_bwd_scores is phases 1 and 2 again with g_ctx in Mem's place
// and g_S in P's.  k_pa_bwd_grads: workgroup (b, 64-column chunk of D), three staged passes (R, g_ctx, Mem: one LDS buffer), the
// [C][C] operand (g_S, P^T, g_S^T) read from global (it is L1-resident: C C floats); wave w owns 16 of the 64 columns and all row tiles.
#include "recon_common.h"

namespace recon {
namespace {

constexpr int kPaMaxPairs = 160;                 // MAX_PAIRS of recon_amd/pair_attention.py (n = 13: 156 pairs)
constexpr int kPaTiles = kPaMaxPairs / 16;       // row / column tiles of 16 pairs
constexpr int kPaNT = 256;
constexpr int kPaChunk = 64;                     // k per step of the score product; columns of D per step of the others
constexpr int kPaLdK = kPaChunk + 4;             // LDS row of a chunk read along k (a fragment's 16 rows x 4 k: 32 lanes, 32 banks)
constexpr int kPaLdN = kPaChunk + 16;            // LDS row of a chunk read along n (a fragment's 4 k x 16 columns)
constexpr int kPaLdP = kPaMaxPairs + 4;          // LDS row of the score / P tile
constexpr int kPaBufFloats = kPaMaxPairs * kPaLdN;               // >= (kPaMaxPairs + 16) * kPaLdK
static_assert(kPaBufFloats >= (kPaMaxPairs + 16) * kPaLdK, "the score product's two operands share the buffer");
using pa_f32x4 = __attribute__((ext_vector_type(4))) float;

bool pa_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// One 64-column chunk of up to nt * 16 rows, global -> registers: thread t holds the quad (t & 15) of row 16 it + (t >> 4).  A quad outside
// [0, rows) x [0, ncols) reads the base instead and becomes zeros (ncols % 4 == 0: a quad is inside or outside as a whole).
__device__ __forceinline__ void pa_chunk_load(float4 (&pre)[kPaTiles], const float* __restrict__ base, int64_t ld, int rows, int col0, int ncols,
                                              int nt, int t) {
    const int c = col0 + (t & 15) * 4;
#pragma unroll
    for (int it = 0; it < kPaTiles; ++it) {
        if (it < nt) {
            const int row = it * 16 + (t >> 4);
            const bool ok = row < rows && c < ncols;
            const float4 v = *reinterpret_cast<const float4*>(ok ? base + row * ld + c : base);
            pre[it] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}
template <int LDS_LD>
__device__ __forceinline__ void pa_chunk_store(float* __restrict__ buf, const float4 (&pre)[kPaTiles], int nt, int t) {
#pragma unroll
    for (int it = 0; it < kPaTiles; ++it)
        if (it < nt) *reinterpret_cast<float4*>(buf + (it * 16 + (t >> 4)) * LDS_LD + (t & 15) * 4) = pre[it];
}

// Ss[16][kPaLdP] = A[i0 .. i0 + 16) x R_b^T over D: columns [0, 16 CT); rows past C and columns past C are zeros.
// buf: kPaBufFloats floats (R's chunk at 0, A's 16 rows behind kPaMaxPairs rows of it).  Ends with a barrier: Ss is complete.
__device__ __forceinline__ void pa_score_tile(const float* __restrict__ A, int64_t ld_a, const float* __restrict__ Rb, int64_t ld_s, int C, int D,
                                              int i0, float* __restrict__ buf, float* __restrict__ Ss) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 15, g = lane >> 4;
    const int CT = (C + 15) >> 4;
    float* As = buf + kPaMaxPairs * kPaLdK;
    pa_f32x4 acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) acc[s] = pa_f32x4{0.f, 0.f, 0.f, 0.f};
    float4 pre[kPaTiles], prea;
    auto load = [&](int k0) {
        pa_chunk_load(pre, Rb, ld_s, C, k0, D, CT, t);
        const int row = i0 + (t >> 4), c = k0 + (t & 15) * 4;
        const bool ok = row < C && c < D;
        const float4 v = *reinterpret_cast<const float4*>(ok ? A + row * ld_a + c : A);
        prea = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    load(0);
    for (int k0 = 0; k0 < D; k0 += kPaChunk) {
        pa_chunk_store<kPaLdK>(buf, pre, CT, t);
        *reinterpret_cast<float4*>(As + (t >> 4) * kPaLdK + (t & 15) * 4) = prea;
        __syncthreads();
        if (k0 + kPaChunk < D) load(k0 + kPaChunk);
#pragma unroll 4
        for (int ks = 0; ks < kPaChunk / 4; ++ks) {
            const float a = As[li * kPaLdK + 4 * ks + g];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int jt = w + 4 * s;
                if (jt < CT) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, buf[(jt * 16 + li) * kPaLdK + 4 * ks + g], acc[s], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C layout: column = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int jt = w + 4 * s;
        if (jt < CT)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ss[(4 * g + r) * kPaLdP + jt * 16 + li] = acc[s][r];
    }
    __syncthreads();
}

struct PaFwdArgs {
    const float* states; int64_t ld_s; const float* memory; int64_t ld_m;
    float* out; int64_t ld_out; float* P;
    int32_t C, D;
};

// grid: B ceil(C / 16) workgroups, tile-minor
__global__ void __launch_bounds__(kPaNT) k_pa_fwd(const PaFwdArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[kPaBufFloats];
    __shared__ __attribute__((aligned(16))) float Ss[16 * kPaLdP];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 15, g = lane >> 4;
    const int C = p.C, D = p.D, CT = (C + 15) >> 4;
    const int64_t b = blockIdx.x / CT;
    const int i0 = static_cast<int>(blockIdx.x - b * CT) * 16;
    const float* __restrict__ Rb = p.states + b * C * p.ld_s;
    const float* __restrict__ Mb = p.memory + b * C * p.ld_m;
    float* __restrict__ ob = p.out + b * C * p.ld_out;
    // the left half: the tile's own rows of states
    for (int idx = t; idx < 16 * (D >> 2); idx += kPaNT) {
        const int row = i0 + idx / (D >> 2), c = (idx % (D >> 2)) * 4;
        if (row < C) *reinterpret_cast<float4*>(ob + row * p.ld_out + c) = *reinterpret_cast<const float4*>(Rb + row * p.ld_s + c);
    }
    pa_score_tile(Mb, p.ld_m, Rb, p.ld_s, C, D, i0, buf, Ss);
    // softmax over j != i: 16 lanes per row, lane q holds j = q, q + 16, ...; the row sum is the lanes' partial sums (each over its j
    // ascending) added by group_sum<16>
    {
        const int row = t >> 4, q = t & 15, i = i0 + row;
        float* srow = Ss + row * kPaLdP;
        float m = -INFINITY;
        for (int j = q; j < C; j += 16)
            if (j != i) m = fmaxf(m, srow[j]);
        m = group_max16(m);
        float sum = 0.f;
        for (int j = q; j < 16 * CT; j += 16) {
            const float e = (j < C && j != i && i < C) ? expf(srow[j] - m) : 0.f;
            srow[j] = e;
            sum += e;
        }
        sum = group_sum<16>(sum);
        const float inv = sum > 0.f ? 1.f / sum : 0.f;               // C == 1: no ghost, P = 0 and ctx = 0
        float* prow = (p.P && i < C) ? p.P + (b * C + i) * C : nullptr;
        for (int j = q; j < 16 * CT; j += 16) {
            const float v = srow[j] * inv;
            srow[j] = v;
            if (prow && j < C) prow[j] = v;
        }
    }
    __syncthreads();
    // ctx = P R: 64 columns of D per step, wave w owns columns 16 w .. 16 w + 15 of them; the reduction runs over j ascending
    const int C4 = (C + 3) >> 2;
    float4 pre[kPaTiles];
    pa_chunk_load(pre, Rb, p.ld_s, C, 0, D, CT, t);
    for (int d0 = 0; d0 < D; d0 += kPaChunk) {
        pa_chunk_store<kPaLdN>(buf, pre, CT, t);
        __syncthreads();
        if (d0 + kPaChunk < D) pa_chunk_load(pre, Rb, p.ld_s, C, d0 + kPaChunk, D, CT, t);
        pa_f32x4 acc = pa_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < C4; ++ks)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ss[li * kPaLdP + 4 * ks + g], buf[(4 * ks + g) * kPaLdN + 16 * w + li], acc, 0, 0, 0);
        const int col = d0 + 16 * w + li;
        if (col < D)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + 4 * g + r;
                if (row < C) ob[row * p.ld_out + D + col] = acc[r];
            }
        __syncthreads();
    }
}

struct PaBwdArgs {
    const float* states; int64_t ld_s; const float* memory; int64_t ld_m;
    const float* P; const float* g_out; int64_t ld_g;
    float* gS; float* g_states; float* g_memory;
    int32_t C, D;
};

// grid: B ceil(C / 16) workgroups; g_S[b][i0 .. i0 + 16)[:] into the workspace
__global__ void __launch_bounds__(kPaNT) k_pa_bwd_scores(const PaBwdArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[kPaBufFloats];
    __shared__ __attribute__((aligned(16))) float Ss[16 * kPaLdP];
    const int t = threadIdx.x;
    const int C = p.C, D = p.D, CT = (C + 15) >> 4;
    const int64_t b = blockIdx.x / CT;
    const int i0 = static_cast<int>(blockIdx.x - b * CT) * 16;
    pa_score_tile(p.g_out + b * C * p.ld_g + D, p.ld_g, p.states + b * C * p.ld_s, p.ld_s, C, D, i0, buf, Ss);
    const int row = t >> 4, q = t & 15, i = i0 + row;
    if (i0 + row >= C) {                                              // (whole 16-lane groups leave: the DPP sums below stay inside a group)
        return;
    }
    const float* __restrict__ prow = p.P + (b * C + i) * C;
    float* __restrict__ grow = p.gS + (b * C + i) * C;
    const float* trow = Ss + row * kPaLdP;
    float r = 0.f;
    for (int j = q; j < C; j += 16) r += prow[j] * trow[j];
    r = group_sum<16>(r);
    for (int j = q; j < C; j += 16) grow[j] = prow[j] * (trow[j] - r);
}

// One staged pass of k_pa_bwd_grads: acc[rt] += X[rows of tile rt][k] x buf[k][16 w + li], k < C.  X[row][k] is Xb[row * C + k], or
// Xb[k * C + row] with TRANSPOSED; entries outside [0, C) x [0, C) read Xb[0] and count as zeros.
template <bool TRANSPOSED>
__device__ __forceinline__ void pa_pass(pa_f32x4 (&acc)[kPaTiles], const float* __restrict__ Xb, const float* __restrict__ buf, int C, int CT, int w,
                                        int li, int g) {
    const int C4 = (C + 3) >> 2;
    for (int ks = 0; ks < C4; ++ks) {
        const int k = 4 * ks + g;
        const float bv = buf[k * kPaLdN + 16 * w + li];
        float a[kPaTiles];
#pragma unroll
        for (int rt = 0; rt < kPaTiles; ++rt)
            if (rt < CT) {
                const int row = rt * 16 + li;
                const bool ok = row < C && k < C;
                const float v = Xb[ok ? (TRANSPOSED ? k * C + row : row * C + k) : 0];
                a[rt] = ok ? v : 0.f;
            }
#pragma unroll
        for (int rt = 0; rt < kPaTiles; ++rt)
            if (rt < CT) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bv, acc[rt], 0, 0, 0);
    }
}

// grid: B ceil(D / 64) workgroups, chunk-minor
__global__ void __launch_bounds__(kPaNT) k_pa_bwd_grads(const PaBwdArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[kPaBufFloats];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 15, g = lane >> 4;
    const int C = p.C, D = p.D, CT = (C + 15) >> 4, NCH = (D + kPaChunk - 1) / kPaChunk;
    const int64_t b = blockIdx.x / NCH;
    const int d0 = static_cast<int>(blockIdx.x - b * NCH) * kPaChunk;
    const float* __restrict__ Rb = p.states + b * C * p.ld_s;
    const float* __restrict__ Mb = p.memory + b * C * p.ld_m;
    const float* __restrict__ Gb = p.g_out + b * C * p.ld_g;
    const float* __restrict__ Pb = p.P + b * C * C;
    const float* __restrict__ gSb = p.gS + b * C * C;
    const int col = d0 + 16 * w + li;
    float4 pre[kPaTiles];
    pa_f32x4 acc[kPaTiles];
    if (p.g_memory) {                                                 // g_Mem[:, chunk] = g_S R[:, chunk]
        pa_chunk_load(pre, Rb, p.ld_s, C, d0, D, CT, t);
        pa_chunk_store<kPaLdN>(buf, pre, CT, t);
        __syncthreads();
#pragma unroll
        for (int rt = 0; rt < kPaTiles; ++rt) acc[rt] = pa_f32x4{0.f, 0.f, 0.f, 0.f};
        pa_pass<false>(acc, gSb, buf, C, CT, w, li, g);
        float* __restrict__ gm = p.g_memory + b * C * D;
        if (col < D)
#pragma unroll
            for (int rt = 0; rt < kPaTiles; ++rt)
                if (rt < CT)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = rt * 16 + 4 * g + r;
                        if (row < C) gm[row * D + col] = acc[rt][r];
                    }
        __syncthreads();
    }
    if (p.g_states) {                                                 // g_R[:, chunk] = g_left + (P^T g_ctx[:, chunk] + g_S^T Mem[:, chunk])
        pa_chunk_load(pre, Gb + D, p.ld_g, C, d0, D, CT, t);
        pa_chunk_store<kPaLdN>(buf, pre, CT, t);
        __syncthreads();
        pa_chunk_load(pre, Mb, p.ld_m, C, d0, D, CT, t);
#pragma unroll
        for (int rt = 0; rt < kPaTiles; ++rt) acc[rt] = pa_f32x4{0.f, 0.f, 0.f, 0.f};
        pa_pass<true>(acc, Pb, buf, C, CT, w, li, g);
        __syncthreads();
        pa_chunk_store<kPaLdN>(buf, pre, CT, t);
        __syncthreads();
        pa_pass<true>(acc, gSb, buf, C, CT, w, li, g);
        float* __restrict__ gs = p.g_states + b * C * D;
        if (col < D)
#pragma unroll
            for (int rt = 0; rt < kPaTiles; ++rt)
                if (rt < CT)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = rt * 16 + 4 * g + r;
                        if (row < C) gs[row * D + col] = Gb[row * p.ld_g + col] + acc[rt][r];
                    }
    }
}

bool pa_shape_ok(int64_t B, int32_t C, int32_t D) {
    return B >= 0 && C >= 1 && C <= kPaMaxPairs && D >= 4 && D <= 1024 && (D & 3) == 0 && B * C <= (int64_t{1} << 24);
}

// The argument checks the two entries share, in the order of their answers: signs (INVALID), the shape (UNSUPPORTED), then, for B > 0
// alone, the pointers and strides (INVALID) and the alignment (UNSUPPORTED).
int pa_check(const float* states, int64_t ld_s, const float* memory, int64_t ld_m, const float* io, int64_t ld_io, bool rest, int64_t B, int32_t C,
             int32_t D) {
    if (B < 0 || C < 0 || D < 0) return RECON_ERR_INVALID;
    if (!pa_shape_ok(B, C, D)) return RECON_ERR_UNSUPPORTED;
    if (B == 0) return RECON_OK;
    if (!states || !memory || !io || !rest || ld_s < D || ld_m < D || ld_io < 2 * static_cast<int64_t>(D)) return RECON_ERR_INVALID;
    if ((ld_s & 3) || (ld_m & 3) || (ld_io & 3) || !pa_aligned16(states) || !pa_aligned16(memory) || !pa_aligned16(io)) return RECON_ERR_UNSUPPORTED;
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_pair_attention_supported(int64_t B, int32_t C, int32_t D) { return recon::pa_shape_ok(B, C, D) ? 1 : 0; }

extern "C" size_t recon_pair_attention_workspace_bytes(int64_t B, int32_t C, int32_t D, int32_t backward) {
    if (!recon::pa_shape_ok(B, C, D) || !backward) return 0;
    return align_up(static_cast<size_t>(B) * C * C * sizeof(float), 16);
}

extern "C" int recon_pair_attention_fwd(const float* states, int64_t ld_s, const float* memory, int64_t ld_m, int64_t B, int32_t C, int32_t D,
                                        float* out, int64_t ld_out, float* P, recon_stream_t stream) {
    using namespace recon;
    const int rc = pa_check(states, ld_s, memory, ld_m, out, ld_out, true, B, C, D);
    if (rc != RECON_OK || B == 0) return rc;
    PaFwdArgs a{states, ld_s, memory, ld_m, out, ld_out, P, C, D};
    hipLaunchKernelGGL(k_pa_fwd, dim3(static_cast<unsigned>(B * ((C + 15) / 16))), dim3(kPaNT), 0, as_stream(stream), a);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_pair_attention_bwd(const float* states, int64_t ld_s, const float* memory, int64_t ld_m, const float* P, const float* g_out,
                                        int64_t ld_g, int64_t B, int32_t C, int32_t D, float* g_states, float* g_memory, void* workspace,
                                        size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    const int rc = pa_check(states, ld_s, memory, ld_m, g_out, ld_g, P != nullptr, B, C, D);
    if (rc != RECON_OK || B == 0 || (!g_states && !g_memory)) return rc;
    if (!workspace || !pa_aligned16(workspace)) return RECON_ERR_INVALID;
    if (workspace_bytes < recon_pair_attention_workspace_bytes(B, C, D, 1)) return RECON_ERR_WORKSPACE;
    PaBwdArgs a{states, ld_s, memory, ld_m, P, g_out, ld_g, static_cast<float*>(workspace), g_states, g_memory, C, D};
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_pa_bwd_scores, dim3(static_cast<unsigned>(B * ((C + 15) / 16))), dim3(kPaNT), 0, st, a);
    RECON_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_pa_bwd_grads, dim3(static_cast<unsigned>(B * ((D + kPaChunk - 1) / kPaChunk))), dim3(kPaNT), 0, st, a);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}
