// The 64 x 64 x 32 tile of the two fp32 MFMA ops, said once: pair_trans.hip (the transition projections) and
// rel_head.hip (the relation classifier over its feature blocks, section 23) are one design.  Included by those two files only.
//
// 64 x 64 outputs per workgroup, 32 of the reduction index per step, four waves as 2 x 2, each 2 x 2 tiles of v_mfma_f32_16x16x4_f32
// (four independent accumulators per wave: the 40-cycle dependent latency of the 32-cycle instruction is covered).  Operands go
// global -> registers -> LDS, two register stages and two LDS buffers deep (tile_pipeline; one barrier per step), and lie k-major in
// LDS: row k holds the 64 m (or n) values at k * 80 + (k / 4) * 8.  The row length 80 puts the two k rows a 32-lane group of a fragment
// read touches (k = 4 ks + g, g = 0, 1) 16 banks apart: ds_read_b32 is conflict free; the skew of 8 per four rows does the same for the
// transposed stores of operands that are contiguous along k in memory (a lane group writes rows 4 q + j, q = 0..3, for 8 consecutive
// m).  Operands contiguous along m / n are stored as float4.
//
// Staging loads are branch free: a load outside the operand reads a valid address instead (each kernel says which), so that a step's
// loads are issued back to back (behind a branch each, they waited for one another).  What was loaded is only looked at when the stage
// is stored to LDS, a step later (each kernel's `finish`): the stage carries one flag per element, and keep4 puts zeros where it is
// clear.
//
// What lives here: the constants, the layout, the staged step, the two LDS stores, the reduction pipeline, the lane roles and the two
// host-side rules both launchers follow.  What does not: the stage structs (what a step holds in flight is each op's own), the loads,
// and the epilogues — the guarded tile store of k_pt_dx and k_rh_dblock included, which as a function of this header changed both
// files' machine code ("The two fp32 MFMA ops say their tile once").
#pragma once
#include "recon_common.h"

namespace recon {
namespace {

constexpr int NT = 256, BM = 64, BN = 64, BK = 32, LD = 80;
constexpr int NP = BK / 16;              // float4 items per thread, operand and step
constexpr int TILE = BK * LD + 8 * (BK / 4);     // + the skew of the last four rows, rounded
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ int lds_at(int k, int c) { return k * LD + (k >> 2) * 8 + c; }

// bit j of m: element j of v counts
__device__ __forceinline__ float4 keep4(uint32_t m, float4 v) {
    return make_float4((m & 1u) ? v.x : 0.f, (m & 2u) ? v.y : 0.f, (m & 4u) ? v.z : 0.f, (m & 8u) ? v.w : 0.f);
}

// a thread's roles: t stages (row t / 4, k quad t % 4) or (k row t / 16, quad t % 16); wave (mb / 32, nb / 32) of the 2 x 2 owns the
// 32 x 32 outputs at (mb, nb); li, g: the lane's place in an MFMA fragment (below)
struct Lane { int t, li, g, mb, nb; };
__device__ __forceinline__ Lane tile_lane() {
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    return {t, lane & 15, lane >> 4, (wid >> 1) * 32, (wid & 1) * 32};
}

// one staged step: BK / 4 k groups x (2 + 2 fragment reads, 4 MFMAs).  A[l & 15][k = l >> 4], B[k = l >> 4][l & 15].
// ONES: a fifth and sixth MFMA against a B fragment whose column 0 is 1 — the column of ones behind the B operand, for the wave that owns d_b.
template <bool ONES>
__device__ __forceinline__ void tile_mma(const float* __restrict__ As, const float* __restrict__ Bs, f32x4 (&acc)[2][2], f32x4 (&accb)[2], int mb, int nb,
                                         int li, int g) {
    const float one = li == 0 ? 1.f : 0.f;
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
        const int kk = 4 * ks + g;
        const float* ar = As + lds_at(kk, mb + li);
        const float* br = Bs + lds_at(kk, nb + li);
        const float a0 = ar[0], a1 = ar[16], b0 = br[0], b1 = br[16];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        if constexpr (ONES) {
            accb[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, one, accb[0], 0, 0, 0);
            accb[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, one, accb[1], 0, 0, 0);
        }
    }
}

// an operand contiguous along k in memory: thread (row t / 4, k quad t % 4) holds 4 k of one row; transposed into the k-major tile
__device__ __forceinline__ void store_kminor(float* T, int t, const float4 (&r)[NP]) {
    const int row = t >> 2;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int k = 16 * q + (t & 3) * 4;
        T[lds_at(k, row)] = r[q].x; T[lds_at(k + 1, row)] = r[q].y; T[lds_at(k + 2, row)] = r[q].z; T[lds_at(k + 3, row)] = r[q].w;
    }
}
// an operand contiguous along m / n: thread (k row t / 16, quad t % 16) holds 4 m of one k
__device__ __forceinline__ void store_kmajor(float* T, int t, const float4 (&r)[NP]) {
#pragma unroll
    for (int q = 0; q < NP; ++q) *reinterpret_cast<float4*>(T + lds_at(16 * q + (t >> 4), (t & 15) * 4)) = r[q];
}

// the accumulators of a wave, declared and zeroed: acc[i][j] the 2 x 2 tiles, accb[i] the column of ones.  A macro: as a function the
// zeroing of gemm_tile16.h's accumulators changed machine code.
#define TILE32_ZERO_ACC()                                               \
    f32x4 acc[2][2], accb[2];                                           \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                     \
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};                            \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; \
    }

// The reduction loop of every product, over a stage type with members a[NP] and b[NP].  load(stage, i) issues the global loads of step i
// into a register stage, finish(stage) turns what was loaded into what is stored, mma(A, B) runs a staged step; init(stage, i) prepares
// the stages of steps 0 and 1 before their loads (NoInit: nothing to prepare).  TWO stages are in flight: while step i is multiplied out
// of one LDS buffer, step i + 1 waits in registers for its store into the other buffer and the loads of step i + 2 are on their way.
// The loads in the loop are unconditional (past the end they read a valid address and the stage is never stored): behind a condition
// the compiler cannot count what is in flight and every wait in the loop becomes vmcnt(0).  With guarded loads and one stage the
// transitions' forward took 93 us at the reference's widths, 40 us this way.
// Hand `finish` over as a lambda or a functor, never as a function's bare name: through the pointer it decays to, the kernels changed.
struct NoInit { template <class Stage> __device__ __forceinline__ void operator()(Stage&, int64_t) const {} };

template <class Stage, bool A_KMINOR, bool B_KMINOR, class Init, class Load, class Finish, class Mma>
__device__ __forceinline__ void tile_pipeline(float (*As)[TILE], float (*Bs)[TILE], int t, int64_t n, Init init, Load load, Finish finish, Mma mma) {
    auto store = [&](int buf, Stage& s) {
        finish(s);
        if constexpr (A_KMINOR) store_kminor(As[buf], t, s.a); else store_kmajor(As[buf], t, s.a);
        if constexpr (B_KMINOR) store_kminor(Bs[buf], t, s.b); else store_kmajor(Bs[buf], t, s.b);
    };
    Stage s0, s1;
    init(s0, 0);
    init(s1, 1);
    load(s0, 0);
    load(s1, 1);                                                         // (a step past the end loads from a valid address and is never stored)
    store(0, s0);
    __syncthreads();
    for (int64_t i = 0; i < n; i += 2) {
        load(s0, i + 2);                                                 // unconditional, so that the counted waits know what is in flight
        mma(As[0], Bs[0]);
        if (i + 1 < n) store(1, s1);
        __syncthreads();
        if (i + 1 >= n) break;
        load(s1, i + 3);
        mma(As[1], Bs[1]);
        if (i + 2 < n) store(0, s0);
        __syncthreads();
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the row groups of a weight-gradient pass: ceil(M / rows) of them, at least one and at most max_groups — a function of M alone
int64_t row_groups(int64_t M, int rows, int max_groups) {
    const int64_t g = ceil_div64(M, rows);
    return g < 1 ? 1 : (g > max_groups ? max_groups : g);
}

}  // namespace
}  // namespace recon
