// E10 — the pair states' transition projections (models/models.py:185-192 tied, :240-249 untied; RECON_EAC :395-402 / :450-459,
// RECON_EAC_KGGAT :605-612 / :660-669, RECON :843-850 / :898-907):  T_l = act(x W_l^T + b_l), l < L, as ONE product
// [M, K] x [K, L N1] with the bias and the activation in the epilogue, and its backward as three products whose A operand d_pre_l =
// g_T_l act'(T_l) is formed from g_out[l] and out[l] while it is staged and never written:
//     d_x            = sum_l d_pre_l W_l                 (reduction over l ascending, n ascending)
//     (d_W_l | d_b_l) = d_pre_l^T (x | 1)                (the rows cut into G groups, slab g written by the workgroups of group g, the slabs
//                                                          added in group order by k_pt_reduce)
// Everything is fp32 on v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain), no atomics, every sum in an order the shape alone decides.
//
// One tile scheme for the three products, gemm_tile32.h's (the 64 x 64 x 32 tile, its k-major LDS layout, the register-staged pipeline
// and the branch-free staging loads are explained there).  At the reference's widths (M = 3 600, K = 512, N1 = 256, L = 3) each product
// is 2.83 GFLOP against 20 MB of traffic: matrix-pipe bound, so the tiles are sized for the number of workgroups (684 / 456 / 768 on
// 256 CUs), not for bytes.
//
// The per-layer device pointers travel by value in the kernel arguments (L <= 8), as the segment descriptors of optim.hip do.
#include "gemm_tile32.h"

namespace recon {
namespace {

constexpr int kPtMaxLayers = 8;          // L <= 8: three pointer lists of eight fit the kernel arguments
constexpr int kPtMaxGroups = 8;          // WGRAD_MAX_ROW_GROUPS of recon_amd/transitions.py
constexpr int kPtGroupRows = 32;         // a row group holds at least this many rows (one full step) unless M itself is smaller
// one step's operands in flight, as loaded: a (the forward's x; the backward's g_out), t (the backward's out), b, and which of them count:
// bit 4 q + j for element j of a[q], bit 16 + q for b[q]
struct PtStage { float4 a[NP], t[NP], b[NP]; uint32_t ok; };

__device__ __forceinline__ float pt_act(float v, int act) {
    if (act == RECON_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == RECON_ACT_TANH) return tanhf(v);
    return v;
}
// g act'(T) from the OUTPUT: relu T > 0, tanh 1 - T^2, linear 1
__device__ __forceinline__ float pt_dpre(float g, float t, int act) {
    if (act == RECON_ACT_RELU) return t > 0.f ? g : 0.f;
    if (act == RECON_ACT_TANH) return g * (1.f - t * t);
    return g;
}
__device__ __forceinline__ float4 pt_dpre4(float4 g, float4 t, int act) {
    return make_float4(pt_dpre(g.x, t.x, act), pt_dpre(g.y, t.y, act), pt_dpre(g.z, t.z, act), pt_dpre(g.w, t.w, act));
}

// ------------------------------------------------------------------------------------------------------------------ forward
struct PtFwdArgs {
    const float* x; int64_t ld_x;
    const float* w[kPtMaxLayers]; const float* b[kPtMaxLayers]; float* out[kPtMaxLayers];
    int64_t M; int32_t K, N1, L, act;
};

// grid (row tiles, column tiles over L N1).  A column tile may straddle a layer boundary: column c is (l, n) = (c / N1, c % N1).
__global__ void __launch_bounds__(NT) k_pt_fwd(const PtFwdArgs p) {
    __shared__ __attribute__((aligned(16))) float As[2][TILE];
    __shared__ __attribute__((aligned(16))) float Bs[2][TILE];
    const Lane ln = tile_lane();
    const int t = ln.t, li = ln.li, g = ln.g, mb = ln.mb, nb = ln.nb;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
    const int n0 = blockIdx.y * BN, ncol = p.L * p.N1;
    const int lr = t >> 2, kq = (t & 3) * 4;
    const int64_t am = m0 + lr;
    const bool a_ok = am < p.M;
    const float* ap = p.x + (a_ok ? am : 0) * p.ld_x + kq;
    const int bc = n0 + lr;
    const bool b_ok = bc < ncol;
    const int bl = b_ok ? bc / p.N1 : 0, bn = b_ok ? bc - bl * p.N1 : 0;
    const float* bp = p.w[bl] + static_cast<int64_t>(bn) * p.K + kq;
    const float* w0 = p.w[0];
    TILE32_ZERO_ACC();
    auto load = [&](PtStage& s, int64_t step) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int k0 = static_cast<int>(step) * BK + 16 * q;
            const bool kin = k0 + kq < p.K;                              // K % 4 == 0: a quad is inside or outside as a whole
            s.a[q] = *reinterpret_cast<const float4*>(kin ? ap + k0 : p.x);          // (rows past M were clamped to row 0)
            s.b[q] = *reinterpret_cast<const float4*>(kin ? bp + k0 : w0);
            if (q == 0) s.ok = 0;
            s.ok |= ((a_ok && kin) ? 15u << (4 * q) : 0u) | ((b_ok && kin) ? 1u << (16 + q) : 0u);
        }
    };
    auto finish = [&](PtStage& s) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            s.a[q] = keep4(s.ok >> (4 * q), s.a[q]);
            s.b[q] = keep4((s.ok >> (16 + q)) & 1u ? 15u : 0u, s.b[q]);
        }
    };
    tile_pipeline<PtStage, true, true>(As, Bs, t, (p.K + BK - 1) / BK, NoInit{}, load, finish,
                                       [&](const float* A, const float* B) { tile_mma<false>(A, B, acc, accb, mb, nb, li, g); });
    // C layout: column = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + nb + 16 * j + li;
        if (col >= ncol) continue;
        const int l = col / p.N1, n = col - l * p.N1;
        const float bias = p.b[l] ? p.b[l][n] : 0.f;
        float* o = p.out[l] + n;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + mb + 16 * i + 4 * g + r;
                if (row < p.M) o[row * p.N1] = pt_act(acc[i][j][r] + bias, p.act);
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------ d_x
// The layers are the ones that HAVE a g_out (the host compacts the lists): a layer without one adds nothing.
struct PtDxArgs {
    const float* g[kPtMaxLayers]; const float* out[kPtMaxLayers]; const float* w[kPtMaxLayers];
    float* dx;
    int64_t M; int32_t K, N1, L, act;
};

// grid (row tiles, column tiles over K).  The reduction index r = l N1 + n runs over the concatenated layers, 16 per step.
// V4 (N1 % 4 == 0, 16-byte aligned g_out / out): a quad of r lies in one layer and is one float4 of each.
template <bool V4>
__global__ void __launch_bounds__(NT) k_pt_dx(const PtDxArgs p) {
    __shared__ __attribute__((aligned(16))) float As[2][TILE];
    __shared__ __attribute__((aligned(16))) float Bs[2][TILE];
    const Lane ln = tile_lane();
    const int t = ln.t, li = ln.li, g = ln.g, mb = ln.mb, nb = ln.nb;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
    const int c0 = blockIdx.y * BN, R = p.L * p.N1;
    const int lr = t >> 2, rq = (t & 3) * 4;                             // A: row, quad of r
    const int64_t am = m0 + lr;
    const bool a_ok = am < p.M;
    const int64_t arow = (a_ok ? am : 0) * p.N1;
    const int kr = t >> 4, bcol = c0 + (t & 15) * 4;                     // B: r row, quad of output columns
    const bool b_ok = bcol < p.K;                                        // K % 4 == 0
    const int bcs = b_ok ? bcol : 0;
    TILE32_ZERO_ACC();
    auto load = [&](PtStage& s, int64_t step) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int r0 = static_cast<int>(step) * BK + 16 * q;
            const int rr = r0 + rq;
            if (q == 0) s.ok = 0;
            if constexpr (V4) {
                const int rc = rr < R ? rr : 0, l = rc / p.N1, n = rc - l * p.N1;
                s.a[q] = *reinterpret_cast<const float4*>(p.g[l] + arow + n);
                s.t[q] = *reinterpret_cast<const float4*>(p.out[l] + arow + n);
                s.ok |= (a_ok && rr < R) ? 15u << (4 * q) : 0u;
            } else {
                float v[4], w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int rc = rr + j < R ? rr + j : 0, l = rc / p.N1, n = rc - l * p.N1;
                    v[j] = p.g[l][arow + n];
                    w[j] = p.out[l][arow + n];
                    s.ok |= (a_ok && rr + j < R) ? 1u << (4 * q + j) : 0u;
                }
                s.a[q] = make_float4(v[0], v[1], v[2], v[3]);
                s.t[q] = make_float4(w[0], w[1], w[2], w[3]);
            }
            const int rb_ = r0 + kr, rbc = rb_ < R ? rb_ : 0, lb = rbc / p.N1, nb_ = rbc - lb * p.N1;
            s.b[q] = *reinterpret_cast<const float4*>(p.w[lb] + static_cast<int64_t>(nb_) * p.K + bcs);
            s.ok |= (b_ok && rb_ < R) ? 1u << (16 + q) : 0u;
        }
    };
    auto finish = [&](PtStage& s) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            s.a[q] = keep4(s.ok >> (4 * q), pt_dpre4(s.a[q], s.t[q], p.act));
            s.b[q] = keep4((s.ok >> (16 + q)) & 1u ? 15u : 0u, s.b[q]);
        }
    };
    tile_pipeline<PtStage, true, false>(As, Bs, t, (R + BK - 1) / BK, NoInit{}, load, finish,
                                        [&](const float* A, const float* B) { tile_mma<false>(A, B, acc, accb, mb, nb, li, g); });
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = c0 + nb + 16 * j + li;
        if (col >= p.K) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + mb + 16 * i + 4 * g + r;
                if (row < p.M) p.dx[row * p.K + col] = acc[i][j][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------ weight and bias gradients
// The layers are the ones with a g_out AND a wanted parameter gradient (compacted by the host); slab g is [L N1][K + 1] of them.
struct PtWgArgs {
    const float* x; int64_t ld_x;
    const float* g[kPtMaxLayers]; const float* out[kPtMaxLayers];
    float* slab;
    int64_t M, per; int32_t K, N1, L, act, ntiles;
};

// grid (column tiles over K, L x row tiles over N1, row groups).  Output rows are n of one layer, columns the K columns of x; the column
// of ones (d_b, column K of the slab) is two more MFMAs per step in the waves that own output columns 0..31 of column tile 0.
template <bool V4>
__global__ void __launch_bounds__(NT) k_pt_wgrad(const PtWgArgs p) {
    __shared__ __attribute__((aligned(16))) float As[2][TILE];
    __shared__ __attribute__((aligned(16))) float Bs[2][TILE];
    const Lane ln = tile_lane();
    const int t = ln.t, li = ln.li, g = ln.g, mb = ln.mb, nb = ln.nb;
    const int lc = blockIdx.y / p.ntiles, n0 = (blockIdx.y - lc * p.ntiles) * BM, c0 = blockIdx.x * BN;
    const int64_t m_begin = static_cast<int64_t>(blockIdx.z) * p.per, m_end = min(p.M, m_begin + p.per);
    const bool ones = blockIdx.x == 0 && nb == 0;                        // wave-uniform
    const float* __restrict__ gl = p.g[lc];
    const float* __restrict__ ol = p.out[lc];
    const int kr = t >> 4, q4 = (t & 15) * 4;
    const int an = n0 + q4, bc = c0 + q4;
    const bool b_ok = bc < p.K;
    const int bcc = b_ok ? bc : 0;
    TILE32_ZERO_ACC();
    auto load = [&](PtStage& s, int64_t step) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int64_t m = m_begin + step * BK + 16 * q + kr;
            const bool m_ok = m < m_end;
            const int64_t mc = m_ok ? m : m_begin;
            if (q == 0) s.ok = 0;
            if constexpr (V4) {
                const int64_t off = mc * p.N1 + (an < p.N1 ? an : 0);
                s.a[q] = *reinterpret_cast<const float4*>(gl + off);
                s.t[q] = *reinterpret_cast<const float4*>(ol + off);
                s.ok |= (m_ok && an < p.N1) ? 15u << (4 * q) : 0u;
            } else {
                float v[4], w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t off = mc * p.N1 + (an + j < p.N1 ? an + j : 0);
                    v[j] = gl[off];
                    w[j] = ol[off];
                    s.ok |= (m_ok && an + j < p.N1) ? 1u << (4 * q + j) : 0u;
                }
                s.a[q] = make_float4(v[0], v[1], v[2], v[3]);
                s.t[q] = make_float4(w[0], w[1], w[2], w[3]);
            }
            s.b[q] = *reinterpret_cast<const float4*>(p.x + mc * p.ld_x + bcc);
            s.ok |= (m_ok && b_ok) ? 1u << (16 + q) : 0u;
        }
    };
    auto finish = [&](PtStage& s) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            s.a[q] = keep4(s.ok >> (4 * q), pt_dpre4(s.a[q], s.t[q], p.act));
            s.b[q] = keep4((s.ok >> (16 + q)) & 1u ? 15u : 0u, s.b[q]);
        }
    };
    tile_pipeline<PtStage, false, false>(As, Bs, t, (m_end - m_begin + BK - 1) / BK, NoInit{}, load, finish, [&](const float* A, const float* B) {
        if (ones) tile_mma<true>(A, B, acc, accb, mb, nb, li, g);
        else tile_mma<false>(A, B, acc, accb, mb, nb, li, g);
    });
    const int64_t ldw = p.K + 1;
    float* slab = p.slab + (static_cast<int64_t>(blockIdx.z) * p.L + lc) * p.N1 * ldw;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + mb + 16 * i + 4 * g + r;
            if (n >= p.N1) continue;
            float* srow = slab + n * ldw;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = c0 + nb + 16 * j + li;
                if (col < p.K) srow[col] = acc[i][j][r];
            }
            if (ones && li == 0) srow[p.K] = accb[i][r];
        }
}

// g_w[l] / g_b[l] = the slabs added in group order; a layer without a g_out (slot < 0) receives zeros
struct PtRedArgs {
    const float* slab; float* g_w[kPtMaxLayers]; float* g_b[kPtMaxLayers]; int32_t slot[kPtMaxLayers];
    int32_t K, N1, L, Lc, G;
};
__global__ void __launch_bounds__(256) k_pt_reduce(const PtRedArgs p) {
    const int64_t ldw = p.K + 1, per_layer = p.N1 * ldw;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= per_layer * p.L) return;
    const int l = static_cast<int>(idx / per_layer);
    const int64_t e = idx - l * per_layer;
    const int n = static_cast<int>(e / ldw), c = static_cast<int>(e - n * ldw);
    float* dst = c < p.K ? (p.g_w[l] ? p.g_w[l] + static_cast<int64_t>(n) * p.K + c : nullptr) : (p.g_b[l] ? p.g_b[l] + n : nullptr);
    if (!dst) return;
    float s = 0.f;
    if (p.slot[l] >= 0) {
        const float* src = p.slab + p.slot[l] * per_layer + e;
        const int64_t step = per_layer * p.Lc;
        for (int z = 0; z < p.G; ++z) s += src[z * step];
    }
    *dst = s;
}

int64_t pt_groups(int64_t M) { return row_groups(M, kPtGroupRows, kPtMaxGroups); }

bool pt_shape_ok(int64_t M, int32_t K, int32_t N1, int32_t L) {
    return M >= 0 && M <= (int64_t{1} << 24) && K >= 4 && K <= 1024 && (K & 3) == 0 && N1 >= 1 && N1 <= 1024 && L >= 1 && L <= kPtMaxLayers;
}

// The argument checks the two entries share, in the order of their answers: signs and act (INVALID), the shape (UNSUPPORTED), then, for
// M > 0 alone, the pointers (INVALID) and the alignment (UNSUPPORTED).  rest: the entry's further pointer arguments are there.
int pt_check(const float* x, int64_t ld_x, const float* const* w, const float* const* out, bool rest, int64_t M, int32_t K, int32_t N1, int32_t L,
             int32_t act) {
    if (M < 0 || K < 0 || N1 < 0 || L < 0 || act < RECON_ACT_LINEAR || act > RECON_ACT_TANH) return RECON_ERR_INVALID;
    if (!pt_shape_ok(M, K, N1, L)) return RECON_ERR_UNSUPPORTED;
    if (M == 0) return RECON_OK;
    if (!x || !w || !out || !rest || ld_x < K) return RECON_ERR_INVALID;
    for (int l = 0; l < L; ++l)
        if (!w[l] || !out[l]) return RECON_ERR_INVALID;
    if ((ld_x & 3) || !aligned16(x)) return RECON_ERR_UNSUPPORTED;
    for (int l = 0; l < L; ++l)
        if (!aligned16(w[l])) return RECON_ERR_UNSUPPORTED;
    return RECON_OK;
}

}  // namespace
}  // namespace recon

extern "C" int recon_pair_transitions_supported(int64_t M, int32_t K, int32_t N1, int32_t L) { return recon::pt_shape_ok(M, K, N1, L) ? 1 : 0; }

extern "C" size_t recon_pair_transitions_workspace_bytes(int64_t M, int32_t K, int32_t N1, int32_t L, int32_t backward) {
    using namespace recon;
    if (!pt_shape_ok(M, K, N1, L) || !backward || M == 0) return 0;
    return align_up(static_cast<size_t>(pt_groups(M)) * L * N1 * (K + 1) * sizeof(float), 16);
}

extern "C" int recon_pair_transitions_fwd(const float* x, int64_t ld_x, const float* const* w, const float* const* b, int64_t M, int32_t K, int32_t N1,
                                          int32_t L, int32_t act, float* const* out, recon_stream_t stream) {
    using namespace recon;
    const int rc = pt_check(x, ld_x, w, out, true, M, K, N1, L, act);
    if (rc != RECON_OK || M == 0) return rc;
    PtFwdArgs a{};
    a.x = x; a.ld_x = ld_x; a.M = M; a.K = K; a.N1 = N1; a.L = L; a.act = act;
    for (int l = 0; l < L; ++l) { a.w[l] = w[l]; a.b[l] = b ? b[l] : nullptr; a.out[l] = out[l]; }
    const dim3 grid(static_cast<unsigned>(ceil_div64(M, BM)), static_cast<unsigned>(ceil_div64(static_cast<int64_t>(L) * N1, BN)));
    hipLaunchKernelGGL(k_pt_fwd, grid, dim3(NT), 0, as_stream(stream), a);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_pair_transitions_bwd(const float* x, int64_t ld_x, const float* const* w, const float* const* out, const float* const* g_out,
                                          int64_t M, int32_t K, int32_t N1, int32_t L, int32_t act, float* g_x, float* const* g_w,
                                          float* const* g_b, void* workspace, size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    const int rc = pt_check(x, ld_x, w, out, g_out != nullptr, M, K, N1, L, act);
    if (rc != RECON_OK) return rc;
    hipStream_t st = as_stream(stream);
    bool params = false;
    for (int l = 0; l < L; ++l) params = params || (g_w && g_w[l]) || (g_b && g_b[l]);
    if (M == 0) {                                                        // zeros in every wanted gradient, no kernel
        for (int l = 0; l < L; ++l) {
            if (g_w && g_w[l] && hipMemsetAsync(g_w[l], 0, sizeof(float) * N1 * K, st) != hipSuccess) return RECON_ERR_LAUNCH;
            if (g_b && g_b[l] && hipMemsetAsync(g_b[l], 0, sizeof(float) * N1, st) != hipSuccess) return RECON_ERR_LAUNCH;
        }
        return RECON_OK;
    }
    if (params) {
        if (!workspace || !aligned16(workspace)) return RECON_ERR_INVALID;
        if (workspace_bytes < recon_pair_transitions_workspace_bytes(M, K, N1, L, 1)) return RECON_ERR_WORKSPACE;
    }
    if (g_x) {
        PtDxArgs a{};
        a.dx = g_x; a.M = M; a.K = K; a.N1 = N1; a.act = act;
        bool v4 = (N1 & 3) == 0;
        int n = 0;
        for (int l = 0; l < L; ++l)
            if (g_out[l]) {
                a.g[n] = g_out[l]; a.out[n] = out[l]; a.w[n] = w[l]; ++n;
                v4 = v4 && aligned16(g_out[l]) && aligned16(out[l]);
            }
        a.L = n;
        if (n == 0) {
            if (hipMemsetAsync(g_x, 0, sizeof(float) * static_cast<size_t>(M) * K, st) != hipSuccess) return RECON_ERR_LAUNCH;
        } else {
            const dim3 grid(static_cast<unsigned>(ceil_div64(M, BM)), static_cast<unsigned>(ceil_div64(K, BN)));
            if (v4) hipLaunchKernelGGL(k_pt_dx<true>, grid, dim3(NT), 0, st, a);
            else hipLaunchKernelGGL(k_pt_dx<false>, grid, dim3(NT), 0, st, a);
            RECON_CHECK_LAUNCH();
        }
    }
    if (params) {
        const int64_t G = pt_groups(M);
        PtWgArgs a{};
        a.x = x; a.ld_x = ld_x; a.slab = static_cast<float*>(workspace);
        a.M = M; a.per = ceil_div64(M, G); a.K = K; a.N1 = N1; a.act = act; a.ntiles = static_cast<int32_t>(ceil_div64(N1, BM));
        PtRedArgs r{};
        r.slab = a.slab; r.K = K; r.N1 = N1; r.L = L;
        bool v4 = (N1 & 3) == 0;
        int n = 0;
        for (int l = 0; l < L; ++l) {
            r.g_w[l] = g_w ? g_w[l] : nullptr;
            r.g_b[l] = g_b ? g_b[l] : nullptr;
            r.slot[l] = -1;
            if (g_out[l] && (r.g_w[l] || r.g_b[l])) {
                a.g[n] = g_out[l]; a.out[n] = out[l]; r.slot[l] = n; ++n;
                v4 = v4 && aligned16(g_out[l]) && aligned16(out[l]);
            }
        }
        a.L = n;
        const int64_t groups = ceil_div64(M, a.per);                     // every group holds at least one row
        r.Lc = n; r.G = static_cast<int32_t>(groups);
        if (n > 0) {
            const dim3 grid(static_cast<unsigned>(ceil_div64(K, BN)), static_cast<unsigned>(n * a.ntiles), static_cast<unsigned>(groups));
            if (v4) hipLaunchKernelGGL(k_pt_wgrad<true>, grid, dim3(NT), 0, st, a);
            else hipLaunchKernelGGL(k_pt_wgrad<false>, grid, dim3(NT), 0, st, a);
            RECON_CHECK_LAUNCH();
        }
        const int64_t total = static_cast<int64_t>(L) * N1 * (K + 1);
        hipLaunchKernelGGL(k_pt_reduce, dim3(static_cast<unsigned>(ceil_div64(total, 256))), dim3(256), 0, st, r);
        RECON_CHECK_LAUNCH();
    }
    return RECON_OK;
}
