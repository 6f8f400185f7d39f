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

// The tile of workgroup blockIdx.x in the relation-ordered walk over `items` items: tile[0] = its relation (found by binary search on t),
// tile[1] = its first position in order, tile[2] = the end of the relation's items (tile[1] >= tile[2]: no tile).  seg is clamped to
// [0, items].
__device__ __forceinline__ void kgs_find_tile(int64_t (&tile)[3], const int64_t* __restrict__ seg, int64_t n_rel, int64_t items, int BM) {
    const auto seg_at = [&](int64_t r) { const int64_t v = seg[r]; return v < 0 ? int64_t(0) : v > items ? items : v; };
    const int64_t b = blockIdx.x;
    int64_t lo = 0, hi = n_rel;                                            // the last r with t(r) <= b (t(0) = 0)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (seg_at(mid) / BM + mid <= b) lo = mid; else hi = mid;
    }
    tile[0] = lo;
    tile[1] = seg_at(lo) + (b - seg_at(lo) / BM - lo) * BM;
    tile[2] = seg_at(lo + 1);
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
    if (threadIdx.x == 0) kgs_find_tile(tile, seg, n_rel, items, BM);
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


// ---- the stage-A translation loss of the GAT_sep_space tree (GAT_sep_space/main.py:347-391) --------------------------
// With T = recon_kgsep_ent2rel's rows of the batch's M = n_pos (1 + reps) triples (each ONCE: the reference tiles the positives reps times
// before it multiplies them), x_i = (T[i] + Rel[r_i]) - T[M + i], norm_i = |x_i|_1, term_j = max(0, norm_{j mod n_pos} - norm_{n_pos + j} +
// margin), loss = mean_j term_j.
//   k_kgsl_norms   a wave per triple: norm_i (lane l adds columns l, l + 64, ... in order, then the fixed butterfly of group_sum)
//   k_kgsl_terms   one workgroup: the terms and their mean in the order of loss.hip's k_transe_mean
// Backward, from the upstream scalar g, T and the terms; nothing per tiled copy, no [rows, D] block of the reference's gradient rows:
// A pair counts as active where its term is > 0, as in loss.hip; torch's clamp_min backward also passes the gradient at a pre-clamp value of
// exactly 0, so there (and only there) this path and the op-sequence fallback differ.
//   k_kgsl_prep    per position p of the relation-ordered walk: its entity row and c = +-(g / P) #active pairs of its triple (- for a tail
//                  item: gpre[M + i] = -gx_i (1 - T[M + i]^2))
//   k_kgsl_rows    the walk of k_kgs_ent2rel: a tile of up to 16 RB items of one relation stages gpre = c sign(x) (1 - T^2) in LDS (formed on
//                  the fly) and writes g_rows[item] = gpre W_r^T; B of a lane is four consecutive floats of one row of W_r (one b128 load)
//   k_kgsl_wgrad   g_W[r] = sum over r's items of E[e]^T gpre and g_Rel[r] = sum over r's head items of gx: one workgroup per (relation, 64
//                  rows of g_W[r], 32 columns), which walks ALL the relation's items in order, 64 at a time: the MFMA k index is the item, so
//                  every element is one k-ordered chain written once by one lane — no partials, no arrival counters, no atomics — and a
//                  relation that owns the whole batch still spreads over ceil(D / 64) ceil(D / 32) workgroups (28 at D = 200).
constexpr int kWgItems = 64, kWgRows = 64, kWgCols = 32, kWgLdE = 80, kWgLdG = 48;   // LDS strides: the 4 items of an MFMA step 16 banks apart (64 banks of 4 B)

__global__ void __launch_bounds__(256) k_kgsl_norms(const int64_t* __restrict__ tri, int64_t M, const float* __restrict__ T,
                                                     const float* __restrict__ Rel, int64_t n_relp, int D, float* __restrict__ norms) {
    const int lane = threadIdx.x % kWave;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + threadIdx.x / kWave;
    if (i >= M) return;
    const int64_t r = tri[3 * i + 1];
    float s = 0.f;
    if (r < 0 || r >= n_relp) {
        s = __builtin_nanf("");                                            // a relation outside Rel: NaN, nothing read
    } else {
        const float* a = T + i * D; const float* b = Rel + r * D; const float* t = T + (M + i) * D;
        for (int c = lane; c < D; c += kWave) s += fabsf((a[c] + b[c]) - t[c]);
    }
    s = group_sum<64>(s);
    if (lane == 0) norms[i] = s;
}

__global__ void __launch_bounds__(256) k_kgsl_terms(const float* __restrict__ norms, int64_t n_pos, int64_t P, float margin, float* __restrict__ terms,
                                                     float* __restrict__ loss, int32_t* __restrict__ nan_word) {
    __shared__ float red[256];
    float s = 0.f;
    for (int64_t j = threadIdx.x; j < P; j += 256) {                       // thread t: terms t, t + 256, ... in order
        // clamp_min of the reference propagates NaN (GAT_sep_space/main.py:389 then asserts on the loss); fmaxf alone would return the 0
        const float v = norms[j % n_pos] - norms[n_pos + j] + margin;
        const float term = (v != v) ? v : fmaxf(0.f, v);
        if (nan_word && !(fabsf(v) <= 3.0e38f)) *nan_word = 1;
        terms[j] = term;
        s += term;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] / static_cast<float>(P);
}

__global__ void __launch_bounds__(256) k_kgsl_prep(const int64_t* __restrict__ tri, int64_t M, int64_t n_pos, int reps, int64_t n_ent, int64_t n_relw,
                                                    const int64_t* __restrict__ order, const float* __restrict__ terms,
                                                    const float* __restrict__ g_loss, int64_t* __restrict__ pent, float* __restrict__ pcf) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= 2 * M) return;
    const int64_t it = order[p];
    int64_t e = -1;
    float c = 0.f;
    if (it >= 0 && it < 2 * M) {
        const int64_t i = it < M ? it : it - M, r = tri[3 * i + 1];
        e = tri[3 * i + (it < M ? 0 : 2)];
        if (e < 0 || e >= n_ent || r < 0 || r >= n_relw) e = -1;          // n_relw: rows of both W_ent2rel and Rel
        const float w = g_loss[0] / static_cast<float>(n_pos * reps);
        if (i < n_pos) {
            int cnt = 0;
            for (int k = 0; k < reps; ++k) cnt += terms[k * n_pos + i] > 0.f ? 1 : 0;
            c = w * static_cast<float>(cnt);
        } else {
            c = -(w * (terms[i - n_pos] > 0.f ? 1.f : 0.f));
        }
        if (it >= M) c = -c;
    }
    pent[p] = e;
    pcf[p] = c;
}

// gpre of column k of item `it` (triple i, coefficient c with the item's sign): x recomputed as the forward does; gx = c sign(x), sign(0) =
// sign(NaN) = 0 (torch's sgn); *gx_out receives it
__device__ __forceinline__ float kgsl_gpre(const float* __restrict__ T, const float* __restrict__ rel_row, int64_t M, int D, int64_t it, float c, int k,
                                           float* gx_out) {
    const int64_t i = it < M ? it : it - M;
    const float a = T[i * D + k], b = T[(M + i) * D + k];
    const float x = (a + rel_row[k]) - b;
    const float gx = c * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
    const float t = it < M ? a : b;
    if (gx_out) *gx_out = gx;
    return gx * (1.f - t * t);
}

template <int RB, bool VEC>
__global__ void __launch_bounds__(kTblThreads) k_kgsl_rows(int64_t M, const float* __restrict__ T, const float* __restrict__ Rel,
                                                           const float* __restrict__ W, int64_t n_rel, int D, const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ seg, const int64_t* __restrict__ pent,
                                                           const float* __restrict__ pcf, float* __restrict__ g_rows) {
    extern __shared__ __attribute__((aligned(16))) float kgs_sm[];
    constexpr int BM = 16 * RB;
    __shared__ int64_t tile[3];
    __shared__ int64_t item[BM];                                           // item of each tile row (-1: none)
    __shared__ float cf[BM];                                               // its signed coefficient (NaN: an id outside its table)
    const int ld = kgs_ld(D), Dk = (D + 15) / 16 * 16, NB = Dk / 16;
    const int64_t items = 2 * M;
    if (threadIdx.x == 0) kgs_find_tile(tile, seg, n_rel, items, BM);
    __syncthreads();
    const int64_t rel = tile[0], p0 = tile[1], p_end = tile[2];
    if (p0 >= p_end) return;
    if (threadIdx.x < BM) {
        const int m = threadIdx.x;
        int64_t it = -1;
        float c = 0.f;
        if (p0 + m < p_end) {
            it = order[p0 + m];
            if (it < 0 || it >= items) it = -1;                            // a malformed order writes nothing
            else c = pent[p0 + m] >= 0 ? pcf[p0 + m] : __builtin_nanf("");
        }
        item[m] = it;
        cf[m] = c;
    }
    __syncthreads();
    float* Gs = kgs_sm;                                                    // [BM][ld]: gpre rows of the tile, zero padded
    const float* rel_row = Rel + rel * D;
    for (int i = threadIdx.x; i < BM * Dk; i += kTblThreads) {
        const int m = i / Dk, k = i % Dk;
        const int64_t it = item[m];
        float v = 0.f;
        if (it >= 0 && k < D) {
            const float c = cf[m];
            v = (c == c) ? kgsl_gpre(T, rel_row, M, D, it, c, k, nullptr) : c;
        }
        Gs[m * ld + k] = v;
    }
    __syncthreads();
    // g_rows[item] = gpre W_r^T: B[k][n] = W_r[n][k], four consecutive floats of row n per lane and k block
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, c16 = lane & 15, g = lane >> 4;
    const float* Wr = W + rel * D * D;
    for (int nb = wave; nb < NB; nb += kTblWaves) {
        const int n = nb * 16 + c16;
        const float* wrow = Wr + static_cast<int64_t>(n < D ? n : 0) * D;
        f32x4 acc[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Dk; k0 += 16) {
            const int kb = k0 + 4 * g;
            float b[4];
            if constexpr (VEC) {                                           // D % 4 == 0: kb < D implies kb + 3 < D
                float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kb < D && n < D) w4 = *reinterpret_cast<const float4*>(wrow + kb);
                b[0] = w4.x; b[1] = w4.y; b[2] = w4.z; b[3] = w4.w;
            } else {
                kgs_load_b(b, wrow + kb, 1, kb, n, D);
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) acc[i] = kgs_mfma4(*reinterpret_cast<const float4*>(&Gs[(16 * i + c16) * ld + kb]), b, acc[i]);
        }
        if (n < D)
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t it = item[16 * i + 4 * g + j];
                    if (it >= 0) g_rows[it * D + n] = acc[i][j];
                }
    }
}

// grid.x = n_rel * RG * CG (RG = ceil(D / 64) row groups when g_W is wanted, else 1; CG = ceil(D / 32) column groups)
__global__ void __launch_bounds__(256) k_kgsl_wgrad(int64_t M, const float* __restrict__ E, const float* __restrict__ T, const float* __restrict__ Rel,
                                                     int64_t n_relp, int D, int RG, int CG, const int64_t* __restrict__ order,
                                                     const int64_t* __restrict__ seg, const int64_t* __restrict__ pent, const float* __restrict__ pcf,
                                                     float* __restrict__ g_W, float* __restrict__ g_Rel) {
    __shared__ float Ea[kWgItems * kWgLdE];                                // [item][row of the group]: E[e_item][row0 + .]
    __shared__ float Gs[kWgItems * kWgLdG];                                // [item][column of the group]: gpre
    __shared__ float Xs[kWgItems * kWgCols];                               // [item][column]: gx of a head item, 0 of a tail item
    __shared__ int64_t s_it[kWgItems], s_ent[kWgItems];
    __shared__ float s_cf[kWgItems];
    const int64_t b = blockIdx.x, items = 2 * M;
    const int cg = static_cast<int>(b % CG), rg = static_cast<int>((b / CG) % RG);
    const int64_t rel = b / (static_cast<int64_t>(CG) * RG);
    const int row0 = rg * kWgRows, col0 = cg * kWgCols;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, c16 = lane & 15, g = lane >> 4;
    const auto seg_at = [&](int64_t r) { const int64_t v = seg[r]; return v < 0 ? int64_t(0) : v > items ? items : v; };
    const int64_t p_begin = seg_at(rel), p_end = seg_at(rel + 1);
    const bool want_rel = g_Rel && rg == 0 && rel < n_relp;
    const bool mma = g_W && row0 + 16 * wave < D;                          // this wave's 16 rows of g_W[rel]
    const float* rel_row = Rel + (rel < n_relp ? rel : 0) * D;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    float gr = 0.f;                                                        // thread c < 32: g_Rel[rel][col0 + c]
    const float rel_col = rel_row[col0 + threadIdx.x % kWgCols < D ? col0 + threadIdx.x % kWgCols : 0];   // this thread's column of Rel[rel]
    // the ids and coefficient of item threadIdx.x of a step, read one step ahead (behind the MFMAs of the step before)
    int64_t n_it = -1, n_ent_row = -1;
    float n_cf = 0.f;
    const auto fetch_ids = [&](int64_t p0) {
        n_it = n_ent_row = -1;
        n_cf = 0.f;
        if (threadIdx.x < kWgItems && p0 + threadIdx.x < p_end) {
            n_it = order[p0 + threadIdx.x];
            n_ent_row = pent[p0 + threadIdx.x];
            n_cf = pcf[p0 + threadIdx.x];
            if (n_it < 0 || n_it >= items || n_ent_row < 0) n_it = n_ent_row = -1;   // a malformed order or an id outside its table adds nothing
        }
    };
    fetch_ids(p_begin);
    for (int64_t p0 = p_begin; p0 < p_end; p0 += kWgItems) {
        if (threadIdx.x < kWgItems) { s_it[threadIdx.x] = n_it; s_ent[threadIdx.x] = n_ent_row; s_cf[threadIdx.x] = n_cf; }
        __syncthreads();
        fetch_ids(p0 + kWgItems);
        // every global load of the step is issued before the first is used: the ids come from LDS, an id that adds nothing reads row 0 and
        // is masked afterwards (no branch between the loads)
        constexpr int NE = kWgItems * kWgRows / 256, NG = kWgItems * kWgCols / 256;
        float ea[NE], ta[NG], tb[NG];
        if (g_W) {
#pragma unroll
            for (int u = 0; u < NE; ++u) {                                 // element (item m, row k) = (wave + 4 u, lane)
                const int64_t e = s_ent[wave + 4 * u];
                ea[u] = E[(e >= 0 ? e : 0) * D + (row0 + lane < D ? row0 + lane : 0)];
            }
        }
        const int gk = threadIdx.x % kWgCols, gm = threadIdx.x / kWgCols, gcol = col0 + gk < D ? col0 + gk : 0;
#pragma unroll
        for (int u = 0; u < NG; ++u) {                                     // element (item m, column k) = (gm + 8 u, gk)
            const int64_t it = s_it[gm + 8 * u], i = it < 0 ? 0 : (it < M ? it : it - M);
            ta[u] = T[i * D + gcol];
            tb[u] = T[(M + i) * D + gcol];
        }
        if (g_W) {
#pragma unroll
            for (int u = 0; u < NE; ++u) Ea[(wave + 4 * u) * kWgLdE + lane] = (s_ent[wave + 4 * u] >= 0 && row0 + lane < D) ? ea[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int m = gm + 8 * u;
            const int64_t it = s_it[m];
            float v = 0.f, gx = 0.f;
            if (it >= 0 && col0 + gk < D) {                                // kgsl_gpre on the loaded values
                const float x = (ta[u] + rel_col) - tb[u];
                gx = s_cf[m] * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
                const float t = it < M ? ta[u] : tb[u];
                v = gx * (1.f - t * t);
            }
            Gs[m * kWgLdG + gk] = v;
            Xs[m * kWgCols + gk] = it < M ? gx : 0.f;
        }
        __syncthreads();
        if (mma) {
#pragma unroll 4
            for (int s = 0; s < kWgItems / 4; ++s) {                       // MFMA step s: items 4 s + g, in walk order
                const int m = 4 * s + g;
                const float a = Ea[m * kWgLdE + 16 * wave + c16];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Gs[m * kWgLdG + c16], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Gs[m * kWgLdG + 16 + c16], acc[1], 0, 0, 0);
            }
        }
        if (want_rel && threadIdx.x >= 192 && threadIdx.x < 192 + kWgCols) {   // the last wave (the first to run out of g_W rows)
            const int k = threadIdx.x - 192;
            for (int m = 0; m < kWgItems; ++m) gr += Xs[m * kWgCols + k];
        }
        __syncthreads();
    }
    if (mma)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = row0 + 16 * wave + 4 * g + j, col = col0 + 16 * cb + c16;
                if (row < D && col < D) g_W[(rel * D + row) * D + col] = acc[cb][j];
            }
    if (want_rel && threadIdx.x >= 192 && threadIdx.x < 192 + kWgCols && col0 + threadIdx.x - 192 < D)
        g_Rel[rel * D + col0 + threadIdx.x - 192] = gr;
}

template <int RB, bool VEC>
int kgsl_rows_launch(int64_t M, const float* T, const float* Rel, const float* W, int64_t n_rel, int32_t D, const int64_t* order, const int64_t* seg,
                     const int64_t* pent, const float* pcf, float* g_rows, hipStream_t s) {
    const size_t lds = static_cast<size_t>(16 * RB) * kgs_ld(D) * sizeof(float);
    const int64_t blocks = ceil_div64(2 * M, 16 * RB) + n_rel;
    if (blocks > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kgsl_rows<RB, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(lds)) != hipSuccess)
        return RECON_ERR_LAUNCH;
    hipLaunchKernelGGL((k_kgsl_rows<RB, VEC>), dim3(static_cast<unsigned>(blocks)), dim3(kTblThreads), lds, s, M, T, Rel, W, n_rel, D, order, seg, pent,
                       pcf, g_rows);
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

extern "C" int recon_kgsep_gat_loss_fwd(const int64_t* triples, int64_t n_pos, int32_t reps, const float* T, const float* Rel, int64_t n_relp, int32_t D,
                                        float margin, float* norms, float* terms, float* loss, recon_stream_t stream) {
    if (n_pos < 1 || reps < 1 || n_relp < 1 || D < 1 || !triples || !T || !Rel || !norms || !terms || !loss) return RECON_ERR_INVALID;
    if (n_pos > 0x7fffffffLL / (reps + 1)) return RECON_ERR_UNSUPPORTED;
    const int64_t M = n_pos * (reps + 1), P = n_pos * reps;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(recon::k_kgsl_norms, dim3(static_cast<unsigned>(ceil_div64(M, 4))), dim3(256), 0, s, triples, M, T, Rel, n_relp, D, norms);
    hipLaunchKernelGGL(recon::k_kgsl_terms, dim3(1), dim3(256), 0, s, norms, n_pos, P, margin, terms, loss, recon::nan_flag());
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" size_t recon_kgsep_gat_loss_bwd_workspace_bytes(int64_t M) { return M < 1 ? 0 : static_cast<size_t>(2 * M) * (sizeof(int64_t) + sizeof(float)); }

extern "C" int recon_kgsep_gat_loss_bwd(const int64_t* triples, int64_t n_pos, int32_t reps, const float* E, int64_t n_ent, const float* Rel, int64_t n_relp,
                                        const float* W_ent2rel, int64_t n_rel, int32_t D, const int64_t* order, const int64_t* seg, const float* T,
                                        const float* terms, const float* g_loss, void* workspace, size_t workspace_bytes, float* g_rows, float* g_W,
                                        float* g_Rel, recon_stream_t stream) {
    if (n_pos < 1 || reps < 1 || n_ent < 1 || n_relp < 1 || n_rel < 1 || D < 1) return RECON_ERR_INVALID;
    if (D > recon::kTblMaxD || n_pos > 0x7fffffffLL / (reps + 1)) return RECON_ERR_UNSUPPORTED;
    if (!triples || !E || !Rel || !W_ent2rel || !order || !seg || !T || !terms || !g_loss || !workspace) return RECON_ERR_INVALID;
    const int64_t M = n_pos * (reps + 1);
    if (workspace_bytes < recon_kgsep_gat_loss_bwd_workspace_bytes(M)) return RECON_ERR_WORKSPACE;
    if (!g_rows && !g_W && !g_Rel) return RECON_OK;
    hipStream_t s = as_stream(stream);
    int64_t* pent = static_cast<int64_t*>(workspace);
    float* pcf = reinterpret_cast<float*>(pent + 2 * M);
    hipLaunchKernelGGL(recon::k_kgsl_prep, dim3(static_cast<unsigned>(ceil_div64(2 * M, 256))), dim3(256), 0, s, triples, M, n_pos, reps, n_ent,
                       n_rel < n_relp ? n_rel : n_relp, order, terms, g_loss, pent, pcf);
    RECON_CHECK_LAUNCH();
    if (g_rows) {
        const bool vec = D % 4 == 0 && !(reinterpret_cast<uintptr_t>(W_ent2rel) & 15);
        const int rb = recon::kge2r_row_blocks(D);
        const int rc = rb == 4 ? (vec ? recon::kgsl_rows_launch<4, true>(M, T, Rel, W_ent2rel, n_rel, D, order, seg, pent, pcf, g_rows, s)
                                      : recon::kgsl_rows_launch<4, false>(M, T, Rel, W_ent2rel, n_rel, D, order, seg, pent, pcf, g_rows, s))
                               : (vec ? recon::kgsl_rows_launch<2, true>(M, T, Rel, W_ent2rel, n_rel, D, order, seg, pent, pcf, g_rows, s)
                                      : recon::kgsl_rows_launch<2, false>(M, T, Rel, W_ent2rel, n_rel, D, order, seg, pent, pcf, g_rows, s));
        if (rc != RECON_OK) return rc;
    }
    if (g_W || g_Rel) {
        const int RG = g_W ? (D + recon::kWgRows - 1) / recon::kWgRows : 1, CG = (D + recon::kWgCols - 1) / recon::kWgCols;
        const int64_t blocks = n_rel * RG * CG;
        if (blocks > 0x7fffffffLL) return RECON_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(recon::k_kgsl_wgrad, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, M, E, T, Rel, n_relp, D, RG, CG, order, seg, pent,
                           pcf, g_W, g_Rel);
        RECON_CHECK_LAUNCH();
    }
    return RECON_OK;
}
