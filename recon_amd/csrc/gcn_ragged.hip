// float32 GraphConvolution over a RAGGED batch (models/layers.py:57-63 applied to every graph of a batch whose graphs differ in size;
// BASELINE.json configs[4]):   out[r0_b + i] = relu(sum_j adj_b[i][j] * (x @ W)[r0_b + j] + bias)   for graph b = 0 .. B-1,
// graph b owning node rows r0_b = node_ptr[b] .. node_ptr[b + 1] and a dense n_b x n_b adjacency at adj + adj_ptr[b].
// x @ W, g_support @ W^T and x^T @ g_support run over all rows at once on the GEMMs of the dense layer (prop.hip recon_gcn_fwd / _bwd:
// gemm_f32, or the split-precision gemm_bx3 where the caller hands the term-plane workspaces); the per-graph products — the aggregate and
// g_adj — are the kernels below, on the exact-fp32 matrix-core instruction (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain).
// Work is a flat list of (graph, 32-row tile) items the caller builds from the graph sizes: a graph of 17 nodes costs one workgroup per
// 64 columns, one of 256 nodes eight — no workgroup is launched to find out that its graph has no such rows.
#include <stdlib.h>
#include "recon_common.h"

namespace recon {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kChunksAhead = 4;         // chunks of 32 contraction rows requested before the first is used: n_b <= 128 pays one memory round trip
constexpr int kPitchK = 48;             // M tile kept k-major  (adj^T: memory is contiguous in i):  Ms[k * 48 + i]
constexpr int kPitchI = 34;             // M tile kept i-major  (adj:   memory is contiguous in k):  Ms[i * 34 + k]
constexpr int kPitchX = 80;             // X tile, k-major: Xs[k * 80 + o]

// Y[r0 + i][o] = epilogue( sum_j M[i][j] * Xin[r0 + j][o] ),  M = adj_b (TRANS = false) or adj_b^T (TRANS = true).
// Block = (item = (graph, 32-row tile), 64-column tile); wave w owns 16 columns and both 16-row tiles, as in k_gcn_aggregate_mfma.
// MASK: Xin = gout * (fwd_out > 0);   EPI: + bias, ReLU.
// colsum (MASK instances): the per-graph column sums of the masked operand, [B][O] — the tile that has row tile 0 of a graph adds the
// chunks up in k order as they pass through LDS (the bias gradient's first pass; fixed order, no atomics).
// Memory: kChunksAhead chunks are requested into registers at once; every lane group walks the index that is contiguous in memory.
// LDS: two buffers, so a chunk costs ONE barrier (the write of chunk c + 1 goes to the buffer last read before chunk c's barrier).
// Banks (32 four-byte banks per 32-lane half for ds_read_b32 / ds_write_b32): a fragment read touches k = 4 s + {0, 1} and 16 rows per
// half — k-major pitch 48 puts the two k rows 16 banks apart, i-major pitch 34 gives bank 2 li + lq, pitch 80 again 16 apart: all
// distinct; the writes walk 32 consecutive floats of one LDS row.
template <bool TRANS, bool MASK, bool EPI>
__global__ void __launch_bounds__(256) k_gcn_ragged_aggregate(const float* __restrict__ adj, const float* __restrict__ Xin,
                                                              const float* __restrict__ fwd_out, const float* __restrict__ bias,
                                                              const int32_t* __restrict__ node_ptr, const int64_t* __restrict__ adj_ptr,
                                                              const int32_t* __restrict__ tiles, int32_t B, int32_t O, float* __restrict__ Y,
                                                              float* __restrict__ colsum) {
    constexpr int NCH = kChunksAhead;
    __shared__ float Ms[2][32 * kPitchK];
    __shared__ float Xs[2][32 * kPitchX];
    const int b = tiles[2 * blockIdx.x], i0 = tiles[2 * blockIdx.x + 1] * 32, o0 = blockIdx.y * 64;
    if (b < 0 || b >= B || i0 < 0) return;                             // uniform for the block
    const int64_t r0 = node_ptr[b];
    const int n = node_ptr[b + 1] - node_ptr[b];
    if (i0 >= n) return;
    const float* A = adj + adj_ptr[b];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int li = lane & 15, lq = lane >> 4;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    float csum = 0.f;
    const bool do_colsum = MASK && colsum != nullptr && i0 == 0 && t < 64;
    float mraw[NCH][4], xraw[NCH][8], fraw[MASK ? NCH : 1][8];
    int done = 0;                                                      // chunks consumed: the LDS buffer is done & 1
    for (int kg = 0; kg < n; kg += 32 * NCH) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int k0 = kg + 32 * c;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = t + 256 * u, k = TRANS ? idx >> 5 : idx & 31, i = TRANS ? idx & 31 : idx >> 5;
                float v = 0.f;
                if (k0 + k < n && i0 + i < n)
                    v = TRANS ? A[static_cast<int64_t>(k0 + k) * n + i0 + i] : A[static_cast<int64_t>(i0 + i) * n + k0 + k];
                mraw[c][u] = v;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = t + 256 * u, k = idx >> 6, o = o0 + (idx & 63);
                const bool ok = k0 + k < n && o < O;
                const int64_t g = (r0 + k0 + k) * O + o;
                xraw[c][u] = ok ? Xin[g] : 0.f;
                if constexpr (MASK) fraw[c][u] = ok ? fwd_out[g] : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (kg + 32 * c >= n) break;                               // uniform for the block
            float* Mb = Ms[done & 1];
            float* Xb = Xs[done & 1];
            ++done;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = t + 256 * u, k = TRANS ? idx >> 5 : idx & 31, i = TRANS ? idx & 31 : idx >> 5;
                Mb[TRANS ? k * kPitchK + i : i * kPitchI + k] = mraw[c][u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = t + 256 * u;
                float v = xraw[c][u];
                if constexpr (MASK) v = fraw[c][u] > 0.f ? v : 0.f;
                Xb[(idx >> 6) * kPitchX + (idx & 63)] = v;
            }
            __syncthreads();
            if (do_colsum) {
#pragma unroll 8
                for (int k = 0; k < 32; ++k) csum += Xb[k * kPitchX + t];
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int k = 4 * s + lq;
                const float bx = Xb[k * kPitchX + 16 * w + li];
                const float a0 = TRANS ? Mb[k * kPitchK + li] : Mb[li * kPitchI + k];
                const float a1 = TRANS ? Mb[k * kPitchK + 16 + li] : Mb[(16 + li) * kPitchI + k];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bx, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bx, acc[1], 0, 0, 0);
            }
        }
    }
    if (do_colsum && o0 + t < O) colsum[static_cast<int64_t>(b) * O + o0 + t] = csum;
    const int o = o0 + 16 * w + li;                                    // C layout: col = lane & 15, row = (lane >> 4) * 4 + r
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
                    Y[(r0 + i) * O + o] = v;
                }
            }
    }
}

// g_adj_b[i][j] = sum_o gpre[r0 + i][o] * support[r0 + j][o],  gpre = gout * (fwd_out > 0): 32 x 32 output tiles on the same MFMA, the
// contraction over `out` walked in chunks of 32 through LDS.  Block = (item = (graph, 32-row tile), 32-column tile of the graph);
// wave w owns the 16 x 16 tile (w >> 1, w & 1).  Both operands are contiguous in the contraction index: i-major images of pitch 34.
__global__ void __launch_bounds__(256) k_gcn_ragged_grad_adj(const float* __restrict__ gout, const float* __restrict__ fwd_out,
                                                             const float* __restrict__ sup, const int32_t* __restrict__ node_ptr,
                                                             const int64_t* __restrict__ adj_ptr, const int32_t* __restrict__ tiles, int32_t B,
                                                             int32_t O, float* __restrict__ gadj) {
    constexpr int NCH = kChunksAhead;
    __shared__ float Gs[2][32 * kPitchI];
    __shared__ float Ss[2][32 * kPitchI];
    const int b = tiles[2 * blockIdx.x], i0 = tiles[2 * blockIdx.x + 1] * 32, j0 = blockIdx.y * 32;
    if (b < 0 || b >= B || i0 < 0) return;
    const int64_t r0 = node_ptr[b];
    const int n = node_ptr[b + 1] - node_ptr[b];
    if (i0 >= n || j0 >= n) return;                                    // uniform for the block
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int li = lane & 15, lq = lane >> 4, ti = w >> 1, tj = w & 1;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float graw[NCH][4], fraw[NCH][4], sraw[NCH][4];
    int done = 0;
    for (int og = 0; og < O; og += 32 * NCH) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int oc = og + 32 * c;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = t + 256 * u, o = oc + (idx & 31), r = idx >> 5;
                const bool oki = o < O && i0 + r < n, okj = o < O && j0 + r < n;
                const int64_t gi = (r0 + i0 + r) * O + o, gj = (r0 + j0 + r) * O + o;
                graw[c][u] = oki ? gout[gi] : 0.f;
                fraw[c][u] = oki ? fwd_out[gi] : 0.f;
                sraw[c][u] = okj ? sup[gj] : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (og + 32 * c >= O) break;                               // uniform for the block
            float* Gb = Gs[done & 1];
            float* Sb = Ss[done & 1];
            ++done;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = t + 256 * u, at = (idx >> 5) * kPitchI + (idx & 31);
                Gb[at] = fraw[c][u] > 0.f ? graw[c][u] : 0.f;
                Sb[at] = sraw[c][u];
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int k = 4 * s + lq;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Gb[(16 * ti + li) * kPitchI + k], Sb[(16 * tj + li) * kPitchI + k], acc, 0, 0, 0);
            }
        }
    }
    const int j = j0 + 16 * tj + li;
    if (j < n) {
        float* out = gadj + adj_ptr[b];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 16 * ti + 4 * lq + r;
            if (i < n) out[static_cast<int64_t>(i) * n + j] = acc[r];
        }
    }
}

// g_bias[o] = sum over the graphs, in graph order, of their column sums: 16 columns x 16 runs of consecutive graphs per block, the runs
// combined in order
__global__ void __launch_bounds__(256) k_gcn_ragged_bias_reduce(const float* __restrict__ colsum, int32_t B, int32_t O, float* __restrict__ gbias) {
    __shared__ float red[16][17];
    const int c = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int o = blockIdx.x * 16 + c;
    const int per = (B + 15) / 16;
    const int b0 = grp * per, b1 = min(B, (grp + 1) * per);
    float s = 0.f;
    if (o < O)
        for (int b = b0; b < b1; ++b) s += colsum[static_cast<int64_t>(b) * O + o];
    red[grp][c] = s;
    __syncthreads();
    if (grp == 0 && o < O) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) v += red[g][c];
        gbias[o] = v;
    }
}

int ragged_sizes(int32_t B, int64_t total_rows, int32_t n_max, int32_t I, int32_t O) {
    if (B < 0 || total_rows < 0 || n_max < 0 || I <= 0 || O <= 0) return RECON_ERR_INVALID;
    if ((B == 0) != (total_rows == 0) || (B == 0) != (n_max == 0) || n_max > total_rows || total_rows > static_cast<int64_t>(B) * n_max)
        return RECON_ERR_INVALID;                                      // every graph has 1 .. n_max nodes
    // grid.y of the g_adj launch = 32-column tiles of the largest graph; the GEMMs take 32-bit row counts
    if (B > 65535 || total_rows > 0x7fffffffLL || n_max > 65535 * 32) return RECON_ERR_UNSUPPORTED;
    return RECON_OK;
}

size_t split_part(int32_t rows, int32_t K) { return align_up(static_cast<size_t>(3) * rows * bx3_kp(K) * 2, 256); }   // as prop.hip gcn_split_part

size_t gw_partial_floats(int64_t rows, int32_t I, int32_t O) {
    const int32_t r = static_cast<int32_t>(rows);
    int sk = gemm_pick_split_k(I, O, r);
    const int sk3 = bx3_kmajor_splits(r, bx3_kmajor_split_k(I, O, r, 1));
    if (sk3 > sk) sk = sk3;
    return static_cast<size_t>(sk) * I * O;
}

struct RaggedCall {
    const float* x; int64_t ldx; const float* adj; const float* weight; const int32_t* node_ptr; const int64_t* adj_ptr; const int32_t* tiles;
    int32_t n_tiles, B; int64_t total_rows; int32_t n_max, I, O; float* support; float* out;
};

// every rejection of both launchers, before any launch
int ragged_check(const RaggedCall& c) {
    const int rc = ragged_sizes(c.B, c.total_rows, c.n_max, c.I, c.O);
    if (rc != RECON_OK) return rc;
    if (!c.x || !c.adj || !c.weight || !c.node_ptr || !c.adj_ptr || !c.tiles || !c.support || !c.out) return RECON_ERR_INVALID;
    if (c.ldx < c.I || c.n_tiles < 0) return RECON_ERR_INVALID;
    // a graph of n nodes has ceil(n / 32) row tiles: between one per graph and (total_rows + 31 B) / 32 in all
    if (c.B > 0 && (c.n_tiles < c.B || c.n_tiles > (c.total_rows + 31LL * c.B) / 32)) return RECON_ERR_INVALID;
    return RECON_OK;
}

}  // namespace
}  // namespace recon

using namespace recon;

extern "C" int recon_gcn_ragged_supported(int32_t B, int64_t total_rows, int32_t n_max, int32_t in_features, int32_t out_features) {
    return ragged_sizes(B, total_rows, n_max, in_features, out_features);
}

extern "C" size_t recon_gcn_ragged_bwd_partial_floats(int32_t B, int64_t total_rows, int32_t in_features, int32_t out_features) {
    if (B <= 0 || total_rows <= 0 || total_rows > 0x7fffffffLL || in_features <= 0 || out_features <= 0) return 64;
    return gw_partial_floats(total_rows, in_features, out_features) + static_cast<size_t>(B) * out_features;
}

extern "C" int recon_gcn_ragged_fwd(const float* x, int64_t ldx, const float* adj, const float* weight, const float* bias, const int32_t* node_ptr,
                                    const int64_t* adj_ptr, const int32_t* tiles, int32_t n_tiles, int32_t B, int64_t total_rows, int32_t n_max,
                                    int32_t in_features, int32_t out_features, float* support, float* out, void* w_split, recon_stream_t stream) {
    const RaggedCall c{x, ldx, adj, weight, node_ptr, adj_ptr, tiles, n_tiles, B, total_rows, n_max, in_features, out_features, support, out};
    int rc = ragged_check(c);
    if (rc != RECON_OK) return rc;
    if (B == 0) return RECON_OK;
    hipStream_t st = as_stream(stream);
    const int32_t rows = static_cast<int32_t>(total_rows), I = in_features, O = out_features;
    // support = x @ W over all node rows      (models/layers.py:58)
    GemmBatch one;
    one.batch = 1; one.a_bs = one.b_bs = one.c_bs = 0; one.epilogue = 0;
    const OperandDesc X = plain_operand(x, ldx);
    if (w_split && !(reinterpret_cast<uintptr_t>(w_split) & 15) && bx3_supported(X, I, one)) {
        // bf16 term planes of W^T [3][O][kp(I)] (this product) and of W [3][I][kp(O)] (g_x in the backward)
        char* ws = static_cast<char*>(w_split);
        rc = bx3_split_planes(weight, O, 0, true, O, I, 1, ws, st);
        if (rc == RECON_OK) rc = bx3_split_planes(weight, O, 0, false, I, O, 1, ws + split_part(O, I), st);
        if (rc == RECON_OK) rc = gemm_bx3_batched(rows, O, I, X, ws, plain_output(support, O), one, st);
    } else {
        rc = gemm_f32(rows, O, I, X, true, plain_operand(weight, O), false, plain_output(support, O), 1, nullptr, st);
    }
    if (rc != RECON_OK) return rc;
    // out = relu(adj_b @ support_b + bias) per graph      (models/layers.py:59-63)
    const dim3 grid(static_cast<unsigned>(n_tiles), static_cast<unsigned>(ceil_div64(O, 64)));
    hipLaunchKernelGGL((k_gcn_ragged_aggregate<false, false, true>), grid, dim3(256), 0, st, adj, support, nullptr, bias, node_ptr, adj_ptr, tiles, B,
                       O, out, nullptr);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_gcn_ragged_bwd(const float* x, int64_t ldx, const float* adj, const float* weight, const int32_t* node_ptr,
                                    const int64_t* adj_ptr, const int32_t* tiles, int32_t n_tiles, int32_t B, int64_t total_rows, int32_t n_max,
                                    int32_t in_features, int32_t out_features, const float* support, const float* out, const void* w_split,
                                    const float* grad_out, float* g_support, float* partial, float* g_x, float* g_adj, float* g_weight,
                                    float* g_bias, void* gs_split, recon_stream_t stream) {
    const RaggedCall c{x, ldx, adj, weight, node_ptr, adj_ptr, tiles, n_tiles, B, total_rows, n_max, in_features, out_features,
                       const_cast<float*>(support), const_cast<float*>(out)};
    int rc = ragged_check(c);
    if (rc != RECON_OK) return rc;
    if (!grad_out || !g_support || !partial) return RECON_ERR_INVALID;
    if (B == 0) return RECON_OK;
    hipStream_t st = as_stream(stream);
    const int32_t rows = static_cast<int32_t>(total_rows), I = in_features, O = out_features;
    float* colsum = g_bias ? partial + gw_partial_floats(total_rows, I, O) : nullptr;      // [B][O], behind the split-K partials
    // g_support_b = adj_b^T @ (grad_out * (out > 0)); with a bias gradient the same launch leaves the per-graph column sums
    const dim3 grid(static_cast<unsigned>(n_tiles), static_cast<unsigned>(ceil_div64(O, 64)));
    hipLaunchKernelGGL((k_gcn_ragged_aggregate<true, true, false>), grid, dim3(256), 0, st, adj, grad_out, out, nullptr, node_ptr, adj_ptr, tiles, B, O,
                       g_support, colsum);
    if (g_adj)
        hipLaunchKernelGGL(k_gcn_ragged_grad_adj, dim3(static_cast<unsigned>(n_tiles), static_cast<unsigned>(ceil_div64(n_max, 32))), dim3(256), 0, st,
                           grad_out, out, support, node_ptr, adj_ptr, tiles, B, O, g_adj);
    if (g_bias)
        hipLaunchKernelGGL(k_gcn_ragged_bias_reduce, dim3(static_cast<unsigned>(ceil_div64(O, 16))), dim3(256), 0, st, colsum, B, O, g_bias);
    RECON_CHECK_LAUNCH();
    GemmBatch one;
    one.batch = 1; one.a_bs = one.b_bs = one.c_bs = 0; one.epilogue = 0;
    // g_x = g_support @ W^T
    if (g_x) {
        const OperandDesc G = plain_operand(g_support, O);
        if (w_split && !(reinterpret_cast<uintptr_t>(w_split) & 15) && bx3_supported(plain_operand(x, ldx), I, one) &&
            bx3_supported(G, O, one))                                  // the forward's condition (it filled the planes), and this product's
            rc = gemm_bx3_batched(rows, I, O, G, static_cast<const char*>(w_split) + split_part(O, I), plain_output(g_x, I), one, st);
        else
            rc = gemm_f32(rows, I, O, G, true, plain_operand(weight, O), true, plain_output(g_x, I), 1, nullptr, st);
        if (rc != RECON_OK) return rc;
    }
    // g_W = x^T @ g_support   (split-K over all node rows, deterministic second pass)
    if (g_weight) {
        const int64_t ldp = bx3_kp(O);
        if (gs_split && w_split && !(reinterpret_cast<uintptr_t>(gs_split) & 15) && bx3_kmajor_supported(x, ldx, 0, ldp, 0, I, O)) {
            rc = bx3_split_planes(g_support, O, 0, false, rows, O, 1, gs_split, st);
            const int sk = bx3_kmajor_splits(rows, bx3_kmajor_split_k(I, O, rows, 1));
            if (rc == RECON_OK) rc = gemm_bx3_kmajor_batched(I, O, rows, x, ldx, 0, gs_split, ldp, static_cast<int64_t>(rows) * ldp, 0, 1, sk, partial, st);
            if (rc == RECON_OK) rc = splitk_reduce(partial, sk, I, O, plain_output(g_weight, O), 0, 1, 0, false, st);
        } else {
            const int sk = gemm_pick_split_k(I, O, rows);
            rc = gemm_f32(I, O, rows, plain_operand(x, ldx), false, plain_operand(g_support, O), false, plain_output(g_weight, O), sk, partial, st);
        }
        if (rc != RECON_OK) return rc;
    }
    return RECON_OK;
}
