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
    for (int i = threadIdx.x; i < BM * Dk; i += kTblThreads) {
        const int m = i / Dk, k = i % Dk;
        const int64_t row = m0 + m;
        float v = 0.f;
        if (row < U && k < D) {
            const int64_t e = ids ? ids[row] : row;
            if (e >= 0 && e < n_rows) v = E[e * D + k];                    // an id outside E stages a zero row
        }
        Es[m * ld + k] = v;
    }
    __syncthreads();

    // T = tanh(E_tile W_r), W_r [D][D] laid out [in][out]: B[k][n] = W_r[k][n]
    const float* Wr = W + r * D * D;
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
        // C/D layout: lane (g, c) holds rows 4 g + j, column c of the 16 x 16 block; columns D .. Dk stay zero for the next products
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) Ts[(16 * i + 4 * g + j) * ld + n] = n < D ? tanhf(acc[i][j]) : 0.f;
    }
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

}  // namespace
}  // namespace recon

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
