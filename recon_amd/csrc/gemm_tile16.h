// The 128 x 208 x 32 tile of the 16-bit MFMA GEMMs, said once: gemm_bx3.hip (bf16 x 3), gemm_hx2.hip (f16 x 2) and
// gemm_b16.hip (plain bf16) are one design with T = 3, 2, 1 term planes per operand.  Included by those three files only.
//
// Block tile BM x BN x BK = 128 x 208 x 32, 4 waves stacked along M (8 in k_gemm_hx2<8>), each 32 rows x 208 columns =
// 2 x 13 tiles of v_mfma_f32_16x16x32_{bf16,f16} (104 accumulators), two workgroups per CU.  What lives here: the tile
// constants, the two LDS images with their bank layouts and the maps that fill and read them, the term-product group and
// the pair-pipelined fragment loop, the stores that depend on the images' column order, and the host-side roundings
// every launcher must agree on.  What does not: the kernels' pipelines (how many tiles are in flight, which waits and
// barriers separate them) — those are measured decisions of each kernel and are written where the kernel is.
//
// The two images of a B tile (A has the same two forms; the k-contiguous kernels keep A in registers):
//
//  * k-contiguous operands ([n][k] in memory).  Per term plane 208 rows of 64 bytes (32 k), the 16-byte slot of k group
//    kq rotated by 2 * (row >> 3) — lds_off() — so that the four lane groups of every ds_read_b128 and the 8-lane groups
//    of every 16-byte write hit disjoint banks.  Rows are PERMUTED on the way in: column tile 4q + t owns the columns
//    {64q + 4i + t}, so the accumulators of four neighbouring tiles are four consecutive output columns and the epilogue
//    stores float4s; the 13th tile holds columns 192 .. 207 in order.  The image is filled by LDS-DMA, which writes
//    lane-linear (wave base + 16 B x lane): rotation and permutation are therefore applied on the SOURCE address
//    (b_image_src: slot -> (plane, row, physical slot) -> the k group and column that live there).
//
//  * k-major operands ([k][n] in memory: the weight gradients, whose K is the node dimension).  Row-major images as the
//    tiles lie in memory, and the MFMA fragments — 8 consecutive k for one column — come out through the transposing
//    read ds_read_b64_tr_b16 (16 lanes read a [4 k][16 n] block, lane i receives column i), two reads per fragment
//    (tr_frag).  A rows are 256 B = 8 chunks of 32 B, chunk index XORed with ka_h(k) = (k&3 | (k>>3&1)<<2).  B rows are
//    28 slots of 16 B (KB_SLOTS) — 26 of data and two of padding — rotated by 2 slots when k & 8: found conflict-free for
//    every column tile by exhaustive check (in both images the 8 rows one transposing read touches per 32 lanes land on
//    disjoint bank groups; the unpadded 26-slot row with a wrapping rotation left 17 % of the LDS cycles as conflicts).
//    Again the rotations are applied on the DMA's source side (each kernel's copy plan); the padding slots re-read slot 0.
#pragma once
#include "gemm_common.h"

namespace recon {

constexpr int BM = 128, BN = 208, BK = 32, NT = 256, TN = 13;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using i16x4 = __attribute__((ext_vector_type(4))) short;

constexpr int B_PLANE = BN * 64;                                   // bytes of one term plane of the k-contiguous B image
constexpr int KB_SLOTS = 28;                                       // 16-byte slots per row of the k-major B image: 26 of data + 2 of padding
constexpr int KA_PLANE = BK * 256, KB_PLANE = BK * KB_SLOTS * 16;  // bytes per term plane of the k-major A / B image: 8192, 14336

// ---- k-contiguous image ----------------------------------------------------------------------------------------------------

// byte offset of (row, k group kq of 8 elements) inside one plane; the rotation depends on row & 8 only, so column tile j
// of a lane's fragment is lds_off(lane & 15, lane >> 4) + j * 1024
__device__ __forceinline__ int lds_off(int row, int kq) { return row * 64 + (((kq + 2 * (row >> 3)) & 3) << 4); }

// element offset (16-bit elements, from the batch entry's plane 0, K tile 0) of what 16-byte slot s of a T-plane image
// holds; slots past the image re-read its last one, columns past N the last column
template <int T>
__device__ __forceinline__ int b_image_src(int slot, int n0, int N, int64_t b_plane, int64_t b_row) {
    const int s = min(slot, T * B_PLANE / 16 - 1);
    const int plane = T == 1 ? 0 : s / (BN * 4), rem = T == 1 ? s : s % (BN * 4), rowL = rem >> 2, pslot = rem & 3;
    const int kq = (pslot - 2 * (rowL >> 3)) & 3;                     // inverse of lds_off's rotation
    const int j = rowL >> 4, rho = rowL & 15;
    const int col = j < 12 ? 64 * (j >> 2) + 4 * rho + (j & 3) : 192 + rho;      // tile 4q+t <-> columns 64q + 4i + t
    return static_cast<int>(plane * b_plane + static_cast<int64_t>(min(n0 + col, N - 1)) * b_row + 8 * kq);
}

// fragment reader of the image at Bt: the T terms of column tile j, one ds_read_b128 each
template <class V, int T>
struct KcReader {
    const unsigned char* Bt;
    int b_rd;                                                         // lds_off(lane & 15, lane >> 4)
    __device__ __forceinline__ void operator()(int j, V (&dst)[T]) const {
#pragma unroll
        for (int q = 0; q < T; ++q) dst[q] = *reinterpret_cast<const V*>(Bt + q * B_PLANE + b_rd + j * 1024);
    }
};

// MFMA C layout col = lane & 15, row = (lane >> 4) * 4 + r; columns through the row permutation of the image.  The
// general store: scatter / segments / vector width / column bounds decided per store.  SCALED: values are multiplied by
// their row's factor rsc[i][r] first (bf16 x 3 has none and passes nullptr).
template <bool SCALED>
__device__ __forceinline__ void store_permuted(const f32x4 (&acc)[2][TN], const OutputDesc& C, float* base, int M, int N, int m0, int n0,
                                               int mb, int li, int lq, int epi, int c_vec4, const float (*rsc)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float scale = 1.f;
            if constexpr (SCALED) scale = rsc[i][r];
            auto fin = [&](float v) {
                if constexpr (SCALED) return gemm_epilogue(v * scale, epi);
                else return gemm_epilogue(v, epi);
            };
            const int row = m0 + mb + 16 * i + 4 * lq + r;
            if (row >= M) continue;
            float* crow = base + out_row_off(C, row);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int col = n0 + 64 * q + 4 * li;
                if (c_vec4) {
                    if (col < N)
                        *reinterpret_cast<float4*>(crow + minor_off(C.Dseg, C.Sseg, col)) =
                            make_float4(fin(acc[i][4 * q][r]), fin(acc[i][4 * q + 1][r]), fin(acc[i][4 * q + 2][r]), fin(acc[i][4 * q + 3][r]));
                } else {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        if (col + jj < N) crow[minor_off(C.Dseg, C.Sseg, col + jj)] = fin(acc[i][4 * q + jj][r]);
                }
            }
            const int col = n0 + 192 + li;
            if (col < N) crow[minor_off(C.Dseg, C.Sseg, col)] = fin(acc[i][12][r]);
        }
}

// ---- term products -----------------------------------------------------------------------------------------------------------
// A scheme S names what differs between the split forms: the fragment type S::V, the term count S::T, the number of term
// pairs kept S::NP, and S::mfma(t, a, b, c) = c + a[TA[t]] . b[TB[t]] for the t-th pair (small terms first).

// the NP term products for a GROUP of independent accumulators, issued term by term: back-to-back MFMAs into the same
// accumulator would each wait for the previous result (dependent-issue latency of the 4-pass MFMA); NJ column tiles x 2
// row tiles keep 2 NJ - 1 independent MFMAs between two that hit the same accumulator
template <class S, int NJ>
__device__ __forceinline__ void products(f32x4 (&acc)[2][TN], const typename S::V (&a)[2][S::T], const typename S::V (&b)[2][S::T], int j0) {
#pragma unroll
    for (int t = 0; t < S::NP; ++t)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][j0 + jj] = S::mfma(t, a[i], b[jj], acc[i][j0 + jj]);
}

// one K tile of the wave's 32 x 208 block: column tiles in pairs, the fragments of the next pair are read (read(j, dst):
// the T terms of column tile j, from either image) while the MFMAs of this one run — two register sets pinned with
// sched_barrier: left alone the scheduler reads into one set and waits for every read.  (k_gemm_hx2_r3 issues its tile's
// requests behind the first group and keeps its own copy of this loop.)
template <class S, class Read>
__device__ __forceinline__ void mma_pairs(f32x4 (&acc)[2][TN], const typename S::V (&a)[2][S::T], Read read) {
    typename S::V b[2][2][S::T];
    auto read_pair = [&](int j0, typename S::V (&dst)[2][S::T]) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
            if (j0 + jj < TN) read(j0 + jj, dst[jj]);
    };
    read_pair(0, b[0]);
#pragma unroll
    for (int g = 0; g < (TN + 1) / 2; ++g) {
        if (2 * g + 2 < TN) read_pair(2 * g + 2, b[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (2 * g + 1 < TN) products<S, 2>(acc, a, b[g & 1], 2 * g);
        else products<S, 1>(acc, a, b[g & 1], 2 * g);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- k-major images ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int ka_h(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }

// one MFMA fragment through two transposing reads
template <class V>
__device__ __forceinline__ V tr_frag(const unsigned char* base, int off_lo, int off_hi) {
    const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(base + off_lo));
    const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(base + off_hi));
    return __builtin_bit_cast(V, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// K rounded up to whole K tiles: the padded row length of every pre-split / padded plane
inline int32_t tile_kp(int32_t K) { return (K + BK - 1) / BK * BK; }

// split-K of the k-major products: whole K tiles per split, rounded up — so fewer splits than requested may be used;
// launchers and the callers that size `partial` must round alike
struct SplitK { int32_t k_per_split, nsplit; };
inline SplitK splitk_plan(int32_t K, int32_t split_k) {
    int64_t kps = ceil_div64(K > 0 ? K : 1, split_k);
    kps = ceil_div64(kps, BK) * BK;
    return {static_cast<int32_t>(kps), static_cast<int32_t>(ceil_div64(K > 0 ? K : 1, kps))};
}

// float4 stores of four consecutive output columns are legal: alignment of every stride, whole segments
inline bool c_vec4_ok(const OutputDesc& C, int32_t N, int64_t c_bs) {
    return !(N & 3) && !(c_bs & 3) && !(reinterpret_cast<uintptr_t>(C.base) & 15) && !(C.S1 & 3) && !(C.S2 & 3) && !(C.Sseg & 3) &&
           (C.Dseg >= N || !(C.Dseg & 3));
}

}  // namespace recon
