// Per-relation ConvKB tables of the GAT_sep_space scorer (GAT_sep_space/models.py:316-339, SpKBGATConvOnly.batch_test with model_gat):
// both entities of a triple are carried into its relation's space before ConvKB, e' = tanh(E[e] W_ent2rel[r]), so the entity halves of
// fc1 (W1 = [W_h | W_r | W_t]) become per-relation tables
//     P_h^r = tanh(E W_ent2rel[r]) W_h^T,      P_t^r = tanh(E W_ent2rel[r]) W_t^T
// that the relation-segmented rank and dense kernels of csrc/kg_eval.hip read in place of P_h / P_t.
//
// k_kgs_tables: one workgroup per (relation of the chunk, tile of 16 RB entity rows).  The gathered E tile is staged in LDS, T = tanh(E_tile W_r)
// goes to a second LDS tile (never to HBM), and T is multiplied by W_h^T and W_t^T; W_r and W1 are read from global memory (L2: every row tile
// of a relation reads the same matrices).  Products on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fma chain, no split precision); wave w
// owns the 16-column blocks w, w + 4, ... of all RB row blocks.  Inside a 16-wide k block lane group g (lane >> 4) supplies k = k0 + 4 g + s at
// MFMA step s, so a lane reads its A operand as one b128 from LDS.  Every output element is written by exactly one lane and nothing is
// accumulated across workgroups: the tables are bitwise identical from run to run.
//
// k_kgs_ent2rel: the rows the training step of the same scorer scores (GAT_sep_space/models.py:312-320, SpKBGATConvOnly.forward), T[m] =
// tanh(E[h_m] W_ent2rel[r_m]) and T[M + m] = tanh(E[t_m] W_ent2rel[r_m]), written to HBM as the entity table of the fused ConvKB training
// kernels (csrc/kg_train.hip).  The 2 M (entity, relation) items are walked in relation order; a workgroup takes up to
// 16 RB items of one relation, stages their E rows and runs the same staging and MFMA loop as k_kgs_tables, then writes tanh straight out.
#include "recon_common.h"

#pragma clang fp contract(off)

namespace recon {
namespace {

constexpr int kTblThreads = 256, kTblWaves = kTblThreads / kWave, kTblMaxD = 512;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS row stride of a [rows][D] tile: D rounded up to the 16-wide k block plus 4 (stride / 4 odd: the 16 rows one b128 lane group reads fall
// on distinct bank quads)
__host__ __device__ inline int kgs_ld(int D) { return (D + 15) / 16 * 16 + 4; }
inline size_t kgs_lds_bytes(int RB, int D) { return 2 * static_cast<size_t>(16 * RB) * kgs_ld(D) * sizeof(float); }

// B[k][n] of one MFMA k block (k = kb .. kb + 3 at steps s = 0..3) for output column n: p points at element (kb, n), stride between k
__device__ __forceinline__ void kgs_load_b(float (&b)[4], const float* __restrict__ p, int64_t stride, int kb, int n, int D) {
#pragma unroll
    for (int s = 0; s < 4; ++s) b[s] = (kb + s < D && n < D) ? p[s * stride] : 0.f;
}

__device__ __forceinline__ f32x4 kgs_mfma4(const float4 a, const float (&b)[4], f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], acc, 0, 0, 0);
}

// Stage the E rows of a tile in LDS, Es [BM][ld], zero padded to Dk columns: tile row m holds E[row_of(m)] when in_tile(m); a row outside
// the tile or an id outside E stages a zero row
template <class InTile, class RowOf>
__device__ __forceinline__ void kgs_stage_rows(float* __restrict__ Es, int BM, int ld, int Dk, int D, const float* __restrict__ E, int64_t n_rows,
                                               InTile in_tile, RowOf row_of) {
    for (int i = threadIdx.x; i < BM * Dk; i += kTblThreads) {
        const int m = i / Dk, k = i % Dk;
        float v = 0.f;
        if (in_tile(m) && k < D) {
            const int64_t e = row_of(m);
            if (e >= 0 && e < n_rows) v = E[e * D + k];                    // an id outside E stages a zero row
        }
        Es[m * ld + k] = v;
    }
}

// X = E_tile W_r for the 16 RB staged rows, W_r [D][D] laid out [in][out] (B[k][n] = W_r[k][n]), read from global memory: wave w owns the
// 16-column blocks w, w + 4, ... and hands every element to store(tile row, column n < Dk, x) (columns D .. Dk: x = 0)
template <int RB, class Store>
__device__ __forceinline__ void kgs_rows_times_w(const float* __restrict__ Es, int ld, int Dk, const float* __restrict__ Wr, int D, Store store) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, c = lane & 15, g = lane >> 4, NB = Dk / 16;
    for (int nb = wave; nb < NB; nb += kTblWaves) {
        const int n = nb * 16 + c;
        f32x4 acc[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Dk; k0 += 16) {
            const int kb = k0 + 4 * g;
            float b[4];
            kgs_load_b(b, Wr + static_cast<int64_t>(kb) * D + n, D, kb, n, D);
#pragma unroll
            for (int i = 0; i < RB; ++i) acc[i] = kgs_mfma4(*reinterpret_cast<const float4*>(&Es[(16 * i + c) * ld + kb]), b, acc[i]);
        }
        // C/D layout: lane (g, c) holds rows 4 g + j, column c of the 16 x 16 block
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) store(16 * i + 4 * g + j, n, acc[i][j]);
    }
}

template <int RB>
__global__ void __launch_bounds__(kTblThreads) k_kgs_tables(const float* __restrict__ E, int64_t n_rows, const int64_t* __restrict__ ids, int64_t U,
                                                            const float* __restrict__ W, int64_t n_rel, const int64_t* __restrict__ rel_ids,
                                                            const float* __restrict__ W1, int D, float* __restrict__ Ph, float* __restrict__ Pt) {
    extern __shared__ __attribute__((aligned(16))) float kgs_sm[];
    constexpr int BM = 16 * RB;
    const int ld = kgs_ld(D), Dk = (D + 15) / 16 * 16, NB = Dk / 16;
    float* Es = kgs_sm;                                                    // [BM][ld]: E rows of the tile, zero padded
    float* Ts = kgs_sm + BM * ld;                                          // [BM][ld]: tanh(E_tile W_r)
    const int rl = blockIdx.y;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
    const int64_t r = rel_ids[rl];
    const int64_t out0 = static_cast<int64_t>(rl) * U * D;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, c = lane & 15, g = lane >> 4;
    if (r < 0 || r >= n_rel) {                                             // relation outside W_ent2rel: NaN tables, nothing read
        for (int i = threadIdx.x; i < BM * D; i += kTblThreads) {
            const int64_t row = m0 + i / D;
            if (row < U) Ph[out0 + row * D + i % D] = Pt[out0 + row * D + i % D] = __builtin_nanf("");
        }
        return;
    }
    kgs_stage_rows(Es, BM, ld, Dk, D, E, n_rows, [&](int m) { return m0 + m < U; }, [&](int m) {
        const int64_t row = m0 + m;
        return ids ? ids[row] : row;
    });
    __syncthreads();

    // T = tanh(E_tile W_r); columns D .. Dk stay zero for the next products
    kgs_rows_times_w<RB>(Es, ld, Dk, W + r * D * D, D, [&](int row, int n, float x) { Ts[row * ld + n] = n < D ? tanhf(x) : 0.f; });
    __syncthreads();

    // P_h = T W_h^T, P_t = T W_t^T: B[k][n] = W1[n][k] (W_h) and W1[n][2 D + k] (W_t), row stride 3 D
    for (int nb = wave; nb < NB; nb += kTblWaves) {
        const int n = nb * 16 + c;
        const float* wh = W1 + static_cast<int64_t>(n < D ? n : 0) * 3 * D;
        f32x4 ah[RB], at[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) ah[i] = at[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Dk; k0 += 16) {
            const int kb = k0 + 4 * g;
            float bh[4], bt[4];
            kgs_load_b(bh, wh + kb, 1, kb, n, D);
            kgs_load_b(bt, wh + 2 * D + kb, 1, kb, n, D);
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const float4 a = *reinterpret_cast<const float4*>(&Ts[(16 * i + c) * ld + kb]);
                ah[i] = kgs_mfma4(a, bh, ah[i]);
                at[i] = kgs_mfma4(a, bt, at[i]);
            }
        }
        if (n < D)
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t row = m0 + 16 * i + 4 * g + j;
                    if (row < U) {
                        Ph[out0 + row * D + n] = ah[i][j];
                        Pt[out0 + row * D + n] = at[i][j];
                    }
                }
    }
}

// row blocks per workgroup: the most (4, 2, 1) whose two LDS tiles fit 80 KB, so that two workgroups share a CU
int kgs_row_blocks(int D) {
    for (int rb = 4; rb > 1; rb >>= 1)
        if (kgs_lds_bytes(rb, D) <= 80 * 1024) return rb;
    return 1;
}

template <int RB>
int kgs_launch(const float* E, int64_t n_rows, const int64_t* ids, int64_t U, const float* W, int64_t n_rel, const int64_t* rel_ids, int32_t Rc,
               const float* W1, int32_t D, float* P_h, float* P_t, hipStream_t s) {
    const size_t lds = kgs_lds_bytes(RB, D);
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kgs_tables<RB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(lds)) != hipSuccess)
        return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(k_kgs_tables<RB>, dim3(static_cast<unsigned>(ceil_div64(U, 16 * RB)), static_cast<unsigned>(Rc)), dim3(kTblThreads), lds, s, E,
                       n_rows, ids, U, W, n_rel, rel_ids, W1, D, P_h, P_t);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

// k_kgs_ent2rel: grid.x is the bound ceil(2 M / BM) + n_rel.  Relation r's tiles are workgroups [t(r), t(r + 1)) with t(r) = seg[r] / BM + r
// (t(r + 1) - t(r) >= ceil(items of r / BM)); a workgroup finds its relation by binary search on t and leaves when its tile is empty.
// Item i < M is the head of triple i, item M + i its tail; T row i belongs to item i.  An item whose entity id lies outside E or whose
// relation is not the tile's (the caller clamped an id outside W_ent2rel for the sort) gets a NaN row.
template <int RB>
__global__ void __launch_bounds__(kTblThreads) k_kgs_ent2rel(const void* __restrict__ triples, int index_bytes, int64_t M, const float* __restrict__ E,
                                                             int64_t n_ent, const float* __restrict__ W, int64_t n_rel, int D,
                                                             const int64_t* __restrict__ order, const int64_t* __restrict__ seg, float* __restrict__ T,
                                                             int64_t* __restrict__ remapped) {
    extern __shared__ __attribute__((aligned(16))) float kgs_sm[];
    constexpr int BM = 16 * RB;
    __shared__ int64_t tile[3];                                            // relation, first position in order, end of the relation's items
    __shared__ int64_t item[BM], ent[BM];                                  // item of each tile row (-1: none); its entity row (-1: NaN row)
    const int ld = kgs_ld(D), Dk = (D + 15) / 16 * 16;
    const int64_t items = 2 * M;
    const auto seg_at = [&](int64_t r) { const int64_t v = seg[r]; return v < 0 ? int64_t(0) : v > items ? items : v; };
    if (threadIdx.x == 0) {
        const int64_t b = blockIdx.x;
        int64_t lo = 0, hi = n_rel;                                        // the last r with t(r) <= b (t(0) = 0)
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) / 2;
            if (seg_at(mid) / BM + mid <= b) lo = mid; else hi = mid;
        }
        tile[0] = lo;
        tile[1] = seg_at(lo) + (b - seg_at(lo) / BM - lo) * BM;
        tile[2] = seg_at(lo + 1);
    }
    __syncthreads();
    const int64_t rel = tile[0], p0 = tile[1], p_end = tile[2];
    if (p0 >= p_end) return;
    if (threadIdx.x < BM) {
        const int m = threadIdx.x;
        int64_t it = -1, e = -1;
        if (p0 + m < p_end) {
            it = order[p0 + m];
            if (it < 0 || it >= items) it = -1;                            // a malformed order writes nothing
        }
        if (it >= 0) {
            const int64_t tr = it < M ? it : it - M;
            int64_t h, r, t;
            if (index_bytes == 8) {
                const int64_t* x = static_cast<const int64_t*>(triples) + 3 * tr;
                h = x[0]; r = x[1]; t = x[2];
            } else {
                const int32_t* x = static_cast<const int32_t*>(triples) + 3 * tr;
                h = x[0]; r = x[1]; t = x[2];
            }
            e = it < M ? h : t;
            if (e >= n_ent || r != rel) e = -1;
            if (it < M) {                                                  // the head item writes the triple's row of the remapped triples
                remapped[3 * it] = it;
                remapped[3 * it + 1] = r;
                remapped[3 * it + 2] = M + it;
            }
        }
        item[m] = it;
        ent[m] = e;
    }
    __syncthreads();
    float* Es = kgs_sm;                                                    // [BM][ld]: E rows of the tile, zero padded
    kgs_stage_rows(Es, BM, ld, Dk, D, E, n_ent, [&](int m) { return true; }, [&](int m) { return ent[m]; });
    __syncthreads();
    kgs_rows_times_w<RB>(Es, ld, Dk, W + rel * D * D, D, [&](int row, int n, float x) {
        const int64_t it = item[row];
        if (n < D && it >= 0) T[it * D + n] = ent[row] >= 0 ? tanhf(x) : __builtin_nanf("");
    });
}

// row blocks per workgroup of k_kgs_ent2rel: the most (4, 2) whose one LDS tile fits 80 KB (2 at D = 512)
int kge2r_row_blocks(int D) { return static_cast<size_t>(16 * 4) * kgs_ld(D) * sizeof(float) <= 80 * 1024 ? 4 : 2; }

template <int RB>
int kge2r_launch(const void* triples, int32_t index_bytes, int64_t M, const float* E, int64_t n_ent, const float* W, int64_t n_rel, int32_t D,
                 const int64_t* order, const int64_t* seg, float* T, int64_t* remapped, hipStream_t s) {
    const size_t lds = static_cast<size_t>(16 * RB) * kgs_ld(D) * sizeof(float);
    const int64_t blocks = ceil_div64(2 * M, 16 * RB) + n_rel;
    if (blocks > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kgs_ent2rel<RB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(lds)) != hipSuccess)
        return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL(k_kgs_ent2rel<RB>, dim3(static_cast<unsigned>(blocks)), dim3(kTblThreads), lds, s, triples, index_bytes, M, E, n_ent, W, n_rel,
                       D, order, seg, T, remapped);
    return hipGetLastError() == hipSuccess ? RECON_OK : RECON_ERR_LAUNCH;
}

}  // namespace
}  // namespace recon

extern "C" int recon_kgsep_ent2rel(const void* triples, int32_t index_bytes, int64_t M, const float* E, int64_t n_ent, const float* W_ent2rel,
                                   int64_t n_rel, int32_t D, const int64_t* order, const int64_t* seg, float* T, int64_t* remapped,
                                   recon_stream_t stream) {
    if (M < 0 || n_ent < 1 || n_rel < 1 || D < 1 || (index_bytes != 4 && index_bytes != 8)) return RECON_ERR_INVALID;
    if (D > recon::kTblMaxD || M > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    if (M == 0) return RECON_OK;
    if (!triples || !E || !W_ent2rel || !order || !seg || !T || !remapped) return RECON_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    if (recon::kge2r_row_blocks(D) == 4) return recon::kge2r_launch<4>(triples, index_bytes, M, E, n_ent, W_ent2rel, n_rel, D, order, seg, T, remapped, s);
    return recon::kge2r_launch<2>(triples, index_bytes, M, E, n_ent, W_ent2rel, n_rel, D, order, seg, T, remapped, s);
}

extern "C" int recon_kgsep_tables(const float* E, int64_t n_rows, const int64_t* ids, int64_t U, const float* W_ent2rel, int64_t n_rel,
                                  const int64_t* rel_ids, int32_t Rc, const float* W1, int32_t D, float* P_h, float* P_t, recon_stream_t stream) {
    if (n_rows < 1 || U < 0 || n_rel < 1 || Rc < 0 || D < 1) return RECON_ERR_INVALID;
    if (D > recon::kTblMaxD || Rc > 65535 || U > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    if (U == 0 || Rc == 0) return RECON_OK;
    if (!E || !W_ent2rel || !rel_ids || !W1 || !P_h || !P_t) return RECON_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    switch (recon::kgs_row_blocks(D)) {
        case 4: return recon::kgs_launch<4>(E, n_rows, ids, U, W_ent2rel, n_rel, rel_ids, Rc, W1, D, P_h, P_t, s);
        case 2: return recon::kgs_launch<2>(E, n_rows, ids, U, W_ent2rel, n_rel, rel_ids, Rc, W1, D, P_h, P_t, s);
        default: return recon::kgs_launch<1>(E, n_rows, ids, U, W_ent2rel, n_rel, rel_ids, Rc, W1, D, P_h, P_t, s);
    }
}
