// E11 — the relation classifier over its feature blocks (models/models.py:213, :234, :275 GPGNN and RECON_EAC; :693-697 RECON_EAC_KGGAT;
// :954-966 RECON):  logits = cat(block_0 .. block_{n-1}, scatter(scattered, positions)) W^T + b  without the concatenated operand: the
// reduction walks the blocks where they lie, and the scattered block (row positions[i] is scattered[i], every other row zero) is read
// through `positions`, never written out.  Its backward is three products:
//     d_block_i   = g W[:, cols_i]                       (only the blocks that want one; for the scattered block only the present rows:
//                                                          row i is g[positions[i]] W[:, cols_s])
//     (d_W | d_b) = g^T (cat | 1)                        (the rows cut into G groups, slab z written by the workgroups of group z, the slabs
//                                                          added in group order by k_rh_reduce; an absent row of the scattered block adds
//                                                          nothing: its column block reduces over the present rows of the group alone)
// Everything is fp32 on v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain), no atomics, every sum in an order the shapes, Mnz and the
// positions' row groups decide.
//
// The tile scheme, the LDS layout, the register-staged pipeline and the flag-then-zero staging are gemm_tile32.h's, shared with
// pair_trans.hip (DESIGN.md sections 22 and 23).  What differs from that op: the stage (no saved output, one flag per element of both
// operands, the prefetched positions); widths, strides and bases need no alignment (a block or a weight column range whose base, stride
// and width are 4-aligned is read as float4, any other element by element, each element clamped to a valid address on its own; in the
// two backward products the choice is per block, in the forward, where the block changes inside the loop, per operand and call); and a
// step or a column tile never straddles two blocks, so the block, its base and its stride are uniform per step / per workgroup: no
// per-lane lookup.  Block pointers, strides and widths travel by value in the kernel arguments.
#include "gemm_tile32.h"

#include <type_traits>

namespace recon {
namespace {

constexpr int kRhMaxDense = 4;           // dense blocks
constexpr int kRhMaxBlocks = 5;          // + the scattered one
constexpr int kRhMaxGroups = 8;          // WGRAD_MAX_ROW_GROUPS of recon_amd/relation_head.py
constexpr int kRhGroupRows = 32;         // a row group holds at least this many rows (one full step) unless M itself is smaller
constexpr int kRhMaxWidth = 2048, kRhMaxOut = 1024;
// one step's operands in flight, as loaded, and which of their elements count: bit 4 q + j for element j of a[q], bit 8 + 4 q + j for b[q]
// pi: the positions of the step's rows, fetched two steps ahead of their use (the weight gradient's scattered block alone)
struct RhStage { float4 a[NP], b[NP]; int64_t pi[NP]; uint32_t ok; };

// The column blocks of the concatenated operand, as one kernel walks them.  `end` is the running total of the kernel's units per block:
// reduction steps of 32 (forward), column tiles of 64 (the two backward products).  sb: the scattered block's place in the list, or -1.
struct RhCols {
    const float* p[kRhMaxBlocks]; int64_t ld[kRhMaxBlocks];
    int32_t K[kRhMaxBlocks], cb[kRhMaxBlocks], end[kRhMaxBlocks];
    int32_t nb, sb;
    uint32_t vec, wvec;                  // bit b: block b is read as float4; the weight's columns of block b are
    const int64_t* pos; int64_t Mnz;
};

// the block unit u (a step, a column tile) belongs to; uniform where u is.  A unit past the end belongs to the last block.
__device__ __forceinline__ int rh_block_of(const RhCols& c, int u) {
    int b = 0;
#pragma unroll
    for (int i = 0; i < kRhMaxBlocks - 1; ++i)
        if (i < c.nb - 1 && u >= c.end[i]) b = i + 1;
    return b;
}

// first index whose position is not below v (positions ascending); always inside [0, n]
__device__ __forceinline__ int64_t rh_lower(const int64_t* __restrict__ pos, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pos[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Staging loads never leave the operand: elements k .. k + 3 of a row of K, an element outside read from the row's first instead, and
// m says which were inside.  VEC: the row start is 16-byte aligned and K % 4 == 0, so a quad is inside or outside as a whole.  Which of
// the two forms a reduction loop runs is decided outside the loop (a kernel's template argument, or a workgroup-uniform branch around
// the whole loop): a branch around a load inside it would cost the counted waits gemm_tile32.h's pipeline lives on.
template <bool VEC>
__device__ __forceinline__ float4 rh_ld4(const float* __restrict__ row, int k, int K, uint32_t& m) {
    if constexpr (VEC) {
        const bool in = k < K;
        m = in ? 15u : 0u;
        return *reinterpret_cast<const float4*>(row + (in ? k : 0));
    }
    float v[4];
    m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = k + j < K;
        v[j] = row[in ? k + j : 0];
        m |= in ? 1u << j : 0u;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}
// what a stage stores: zeros where a flag is clear (tile_pipeline's `finish`, the same for the three products)
struct RhFinish {
    __device__ __forceinline__ void operator()(RhStage& s) const {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            s.a[q] = keep4(s.ok >> (4 * q), s.a[q]);
            s.b[q] = keep4(s.ok >> (8 + 4 * q), s.b[q]);
        }
    }
};

using rh_yes = std::true_type;
using rh_no = std::false_type;

// ------------------------------------------------------------------------------------------------------------------ forward
struct RhFwdArgs {
    RhCols c;                            // end: reduction steps
    const float* w; const float* bias; float* out;
    int64_t M; int32_t N, Kt;
};

// grid (row tiles, column tiles over N).  Step s reads 32 columns of ONE block: block b = rh_block_of(s), columns 32 (s - first step of b).
// AV: every block is read as float4; WV: the weight's columns of every block are.  One block that is not puts the operand's loads of
// the whole call on the element path: the block changes from step to step inside the loop, so the choice cannot be a branch there.
template <bool AV, bool WV>
__global__ void __launch_bounds__(NT) k_rh_fwd(const RhFwdArgs p) {
    __shared__ __attribute__((aligned(16))) float As[2][TILE];
    __shared__ __attribute__((aligned(16))) float Bs[2][TILE];
    const RhCols& c = p.c;
    const Lane ln = tile_lane();
    const int t = ln.t, li = ln.li, g = ln.g, mb = ln.mb, nb = ln.nb;
    const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
    const int n0 = blockIdx.y * BN;
    const int lr = t >> 2, kq = (t & 3) * 4;
    const int64_t am = m0 + lr;
    const bool a_ok = am < p.M;
    const int64_t arow = a_ok ? am : 0;
    // the staged row's place in the scattered block, if it has one: one search per thread and kernel
    int64_t srow = 0;
    bool s_ok = false;
    if (c.sb >= 0 && a_ok) {
        const int64_t i = rh_lower(c.pos, c.Mnz, am);
        s_ok = i < c.Mnz && c.pos[i < c.Mnz ? i : 0] == am;
        srow = s_ok ? i : 0;
    }
    const int bc = n0 + lr;
    const bool b_ok = bc < p.N;
    const float* wrow = p.w + static_cast<int64_t>(b_ok ? bc : 0) * p.Kt;
    TILE32_ZERO_ACC();
    auto load = [&](RhStage& s, int64_t step) {
        const int st = static_cast<int>(step), b = rh_block_of(c, st);
        const int kbase = (st - (b ? c.end[b - 1] : 0)) * BK, Kb = c.K[b];
        const bool sc = b == c.sb, r_ok = sc ? s_ok : a_ok;
        const float* ar = c.p[b] + (sc ? srow : arow) * c.ld[b];
        const float* br = wrow + c.cb[b];
        s.ok = 0;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int k = kbase + 16 * q + kq;
            uint32_t ma, mw;
            s.a[q] = rh_ld4<AV>(ar, k, Kb, ma);
            s.b[q] = rh_ld4<WV>(br, k, Kb, mw);
            s.ok |= (r_ok ? ma << (4 * q) : 0u) | (b_ok ? mw << (8 + 4 * q) : 0u);
        }
    };
    tile_pipeline<RhStage, true, true>(As, Bs, t, c.end[c.nb - 1], NoInit{}, load, RhFinish{}, [&](const float* A, const float* B) { tile_mma<false>(A, B, acc, accb, mb, nb, li, g); });
    // C layout: column = lane & 15, row = 4 (lane >> 4) + r
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + nb + 16 * j + li;
        if (col >= p.N) continue;
        const float bias = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + mb + 16 * i + 4 * g + r;
                if (row < p.M) p.out[row * p.N + col] = acc[i][j][r] + bias;
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------ block gradients
// The blocks are the ones that want a gradient (the host compacts the list); c.p is not read, d[b] [rows][K_b] contiguous is written.
struct RhDbArgs {
    RhCols c;                            // end: column tiles
    float* d[kRhMaxBlocks];
    const float* g; const float* w;
    int64_t M; int32_t N, Kt;
};

// grid (row tiles over max(M, Mnz), column tiles of the wanted blocks).  A workgroup's block is uniform; the reduction runs over n.
// For the scattered block the rows are i < Mnz and row i reads g at positions[i]; a position outside [0, M) gives a zero row.
// GV4: N % 4 == 0 and g 16-byte aligned.
template <bool GV4>
__global__ void __launch_bounds__(NT) k_rh_dblock(const RhDbArgs p) {
    __shared__ __attribute__((aligned(16))) float As[2][TILE];
    __shared__ __attribute__((aligned(16))) float Bs[2][TILE];
    const RhCols& c = p.c;
    const Lane ln = tile_lane();
    const int t = ln.t, li = ln.li, g = ln.g, mb = ln.mb, nb = ln.nb;
    const int b = rh_block_of(c, blockIdx.y);
    const bool sc = b == c.sb;
    const int64_t R = sc ? c.Mnz : p.M, m0 = static_cast<int64_t>(blockIdx.x) * BM;
    if (m0 >= R) return;                                                 // uniform: before any barrier
    const int c0 = (static_cast<int>(blockIdx.y) - (b ? c.end[b - 1] : 0)) * BN, Kb = c.K[b];
    const int lr = t >> 2, rq = (t & 3) * 4;                             // A: row, quad of n
    const int64_t am = m0 + lr;
    bool a_ok = am < R;
    int64_t gi = a_ok ? am : 0;
    if (sc) {
        const int64_t pi = c.pos[gi];
        a_ok = a_ok && pi >= 0 && pi < p.M;
        gi = a_ok ? pi : 0;
    }
    const float* ar = p.g + gi * p.N;
    const int kr = t >> 4, bcol = c0 + (t & 15) * 4;                     // B: n row, quad of output columns
    const float* wb = p.w + c.cb[b];
    TILE32_ZERO_ACC();
    auto run = [&](auto wv) {                                            // the whole reduction loop, for one form of the weight's loads
        constexpr bool WV = decltype(wv)::value;
        auto load = [&](RhStage& s, int64_t step) {
            s.ok = 0;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int r0 = static_cast<int>(step) * BK + 16 * q;
                uint32_t ma, mw;
                s.a[q] = rh_ld4<GV4>(ar, r0 + rq, p.N, ma);
                const int n = r0 + kr;
                const bool n_ok = n < p.N;
                s.b[q] = rh_ld4<WV>(wb + static_cast<int64_t>(n_ok ? n : 0) * p.Kt, bcol, Kb, mw);
                s.ok |= (a_ok ? ma << (4 * q) : 0u) | (n_ok ? mw << (8 + 4 * q) : 0u);
            }
        };
        tile_pipeline<RhStage, true, false>(As, Bs, t, (p.N + BK - 1) / BK, NoInit{}, load, RhFinish{},
                                            [&](const float* A, const float* B) { tile_mma<false>(A, B, acc, accb, mb, nb, li, g); });
    };
    if ((c.wvec >> b) & 1u) run(rh_yes{}); else run(rh_no{});           // workgroup-uniform
    float* d = p.d[b];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = c0 + nb + 16 * j + li;
        if (col >= Kb) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + mb + 16 * i + 4 * g + r;
                if (row < R) d[row * Kb + col] = acc[i][j][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------ weight and bias gradients
struct RhWgArgs {
    RhCols c;                            // end: column tiles
    const float* g; float* slab;
    int64_t M, per; int32_t N, Kt;
};

// grid (column tiles of the blocks, row tiles over N, row groups).  Output rows are n, columns the columns of ONE block; slab z is
// [N][Kt + 1].  A dense block reduces over the rows m of group z.  The scattered block reduces over the i whose position lies in the
// group (two searches per workgroup: the positions ascend, so they are consecutive) and reads g at positions[i].  The column of ones
// (d_b, column Kt) is two more MFMAs per step in the waves that own output columns 0..31 of column tile 0, which block 0 (dense) owns.
// GV4: N % 4 == 0 and g 16-byte aligned.
template <bool GV4>
__global__ void __launch_bounds__(NT) k_rh_wgrad(const RhWgArgs p) {
    __shared__ __attribute__((aligned(16))) float As[2][TILE];
    __shared__ __attribute__((aligned(16))) float Bs[2][TILE];
    const RhCols& c = p.c;
    const Lane ln = tile_lane();
    const int t = ln.t, li = ln.li, g = ln.g, mb = ln.mb, nb = ln.nb;
    const int b = rh_block_of(c, blockIdx.x);
    const bool sc = b == c.sb;
    const int c0 = (static_cast<int>(blockIdx.x) - (b ? c.end[b - 1] : 0)) * BN, Kb = c.K[b], n0 = blockIdx.y * BM;
    const int64_t m_begin = static_cast<int64_t>(blockIdx.z) * p.per, m_end = min(p.M, m_begin + p.per);
    const int64_t r_begin = sc ? rh_lower(c.pos, c.Mnz, m_begin) : m_begin, r_end = sc ? rh_lower(c.pos, c.Mnz, m_end) : m_end;
    const bool ones = blockIdx.x == 0 && nb == 0;                        // wave-uniform
    const float* __restrict__ xb = c.p[b];
    const int64_t ldb = c.ld[b];
    const int64_t* __restrict__ pos = c.pos;
    const int kr = t >> 4, q4 = (t & 15) * 4;
    const int an = n0 + q4, bc = c0 + q4;
    TILE32_ZERO_ACC();
    auto run = [&](auto xv, auto scat) {                                 // the whole reduction loop, for one form of the block's loads
        constexpr bool XV = decltype(xv)::value, SC = decltype(scat)::value;
        // row r of the reduction, clamped to a row that exists (row 0: M > 0, and Mnz > 0 where there is a scattered block)
        auto row_of = [&](int64_t step, int q, bool& r_ok) {
            const int64_t r = r_begin + step * BK + 16 * q + kr;
            r_ok = r < r_end;
            return r_ok ? r : 0;
        };
        // the positions of a step's rows are fetched two steps ahead: the load of g that depends on them never waits for them
        auto prefetch = [&](RhStage& s, int64_t step) {
            if constexpr (SC) {
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    bool r_ok;
                    s.pi[q] = pos[row_of(step, q, r_ok)];
                }
            }
        };
        auto load = [&](RhStage& s, int64_t step) {
            s.ok = 0;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                bool r_ok;
                const int64_t rc = row_of(step, q, r_ok);
                int64_t gm = rc;
                if constexpr (SC) {
                    const int64_t pi = s.pi[q];
                    r_ok = r_ok && pi >= 0 && pi < p.M;
                    gm = r_ok ? pi : 0;
                }
                uint32_t ma, mx;
                s.a[q] = rh_ld4<GV4>(p.g + gm * p.N, an, p.N, ma);
                s.b[q] = rh_ld4<XV>(xb + rc * ldb, bc, Kb, mx);
                s.ok |= r_ok ? (ma << (4 * q)) | (mx << (8 + 4 * q)) : 0u;
            }
            prefetch(s, step + 2);
        };
        tile_pipeline<RhStage, false, false>(As, Bs, t, (r_end - r_begin + BK - 1) / BK, prefetch, load, RhFinish{}, [&](const float* A, const float* B) {
            if (ones) tile_mma<true>(A, B, acc, accb, mb, nb, li, g);
            else tile_mma<false>(A, B, acc, accb, mb, nb, li, g);
        });
    };
    const bool xv = (c.vec >> b) & 1u;                                   // workgroup-uniform, like sc
    if (sc) { if (xv) run(rh_yes{}, rh_yes{}); else run(rh_no{}, rh_yes{}); }
    else { if (xv) run(rh_yes{}, rh_no{}); else run(rh_no{}, rh_no{}); }
    const int ldw = p.Kt + 1;
    float* slab = p.slab + static_cast<int64_t>(blockIdx.z) * p.N * ldw;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + mb + 16 * i + 4 * g + r;
            if (n >= p.N) continue;
            float* srow = slab + n * ldw;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = c0 + nb + 16 * j + li;
                if (col < Kb) srow[c.cb[b] + col] = acc[i][j][r];
            }
            if (ones && li == 0) srow[p.Kt] = accb[i][r];
        }
}

// g_w / g_b = the slabs added in group order; columns [zlo, zhi) (an empty scattered block's: no workgroup wrote them) receive zeros
struct RhRedArgs {
    const float* slab; float* g_w; float* g_b;
    int32_t N, Kt, G, zlo, zhi;
};
__global__ void __launch_bounds__(256) k_rh_reduce(const RhRedArgs p) {
    const int64_t ldw = p.Kt + 1, total = p.N * ldw;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= total) return;
    const int n = static_cast<int>(e / ldw), col = static_cast<int>(e - n * ldw);
    float* dst = col < p.Kt ? (p.g_w ? p.g_w + static_cast<int64_t>(n) * p.Kt + col : nullptr) : (p.g_b ? p.g_b + n : nullptr);
    if (!dst) return;
    float s = 0.f;
    if (col < p.zlo || col >= p.zhi)
        for (int z = 0; z < p.G; ++z) s += p.slab[z * total + e];
    *dst = s;
}

int64_t rh_groups(int64_t M) { return row_groups(M, kRhGroupRows, kRhMaxGroups); }

bool rh_shape_ok(int64_t M, int32_t n_blocks, int32_t Kt, int32_t N) {
    return M >= 0 && M <= (int64_t{1} << 24) && n_blocks >= 1 && n_blocks <= kRhMaxDense && Kt >= 1 && Kt <= kRhMaxWidth && N >= 1 && N <= kRhMaxOut;
}

// The argument checks the two entries share; on RECON_OK *Kt is the weight's row length.
int rh_check(const float* const* blocks, const int64_t* ld, const int32_t* widths, int32_t n_blocks, const float* scattered, int64_t ld_s, int32_t K_s,
             const int64_t* positions, int64_t Mnz, const float* weight, int64_t M, int32_t N, int32_t* Kt) {
    if (M < 0 || N < 0 || n_blocks < 0 || K_s < 0 || Mnz < 0 || !widths) return RECON_ERR_INVALID;
    if (n_blocks < 1 || n_blocks > kRhMaxDense) return RECON_ERR_UNSUPPORTED;
    int64_t total = K_s;
    for (int i = 0; i < n_blocks; ++i) {
        if (widths[i] < 1) return RECON_ERR_INVALID;
        total += widths[i];
    }
    if (total > kRhMaxWidth) return RECON_ERR_UNSUPPORTED;
    *Kt = static_cast<int32_t>(total);
    if (!rh_shape_ok(M, n_blocks, *Kt, N) || Mnz > (int64_t{1} << 24)) return RECON_ERR_UNSUPPORTED;
    if (M == 0) return RECON_OK;
    if (!blocks || !ld || !weight) return RECON_ERR_INVALID;
    for (int i = 0; i < n_blocks; ++i)
        if (!blocks[i] || ld[i] < widths[i]) return RECON_ERR_INVALID;
    if (K_s > 0 && Mnz > 0 && (!scattered || !positions || ld_s < K_s)) return RECON_ERR_INVALID;
    return RECON_OK;
}

// The list of blocks a kernel walks: the dense blocks `take` keeps, then the scattered one if it has rows and `take_s` keeps it.
// unit: what `end` counts (BK for reduction steps, BN for column tiles).
RhCols rh_cols(const float* const* blocks, const int64_t* ld, const int32_t* widths, int32_t n_blocks, const bool* take, const float* scattered,
               int64_t ld_s, int32_t K_s, const int64_t* positions, int64_t Mnz, bool take_s, const float* weight, int32_t Kt, int unit) {
    RhCols c{};
    c.sb = -1; c.pos = positions; c.Mnz = Mnz;
    const bool w_ok = aligned16(weight) && (Kt & 3) == 0;
    int n = 0, cb = 0, end = 0;
    auto put = [&](const float* p, int64_t l, int32_t K) {
        c.p[n] = p; c.ld[n] = l; c.K[n] = K; c.cb[n] = cb;
        end += static_cast<int>(ceil_div64(K, unit));
        c.end[n] = end;
        const bool quads = (K & 3) == 0;
        if (quads && p && aligned16(p) && (l & 3) == 0) c.vec |= 1u << n;
        if (quads && w_ok && (cb & 3) == 0) c.wvec |= 1u << n;
        ++n;
    };
    for (int i = 0; i < n_blocks; ++i) {
        if (!take || take[i]) put(blocks ? blocks[i] : nullptr, ld ? ld[i] : 0, widths[i]);
        cb += widths[i];
    }
    if (K_s > 0 && Mnz > 0 && take_s) {
        c.sb = n;
        put(scattered, ld_s, K_s);
    }
    c.nb = n;
    for (int i = n; i < kRhMaxBlocks; ++i) c.end[i] = end;
    return c;
}

}  // namespace
}  // namespace recon

extern "C" int recon_relation_logits_supported(int64_t M, int32_t n_blocks, int32_t Kt, int32_t N) { return recon::rh_shape_ok(M, n_blocks, Kt, N) ? 1 : 0; }

extern "C" size_t recon_relation_logits_workspace_bytes(int64_t M, int32_t n_blocks, int32_t Kt, int32_t N, int32_t backward) {
    using namespace recon;
    if (!rh_shape_ok(M, n_blocks, Kt, N) || !backward || M == 0) return 0;
    return align_up(static_cast<size_t>(rh_groups(M)) * N * (Kt + 1) * sizeof(float), 16);
}

extern "C" int recon_relation_logits_fwd(const float* const* blocks, const int64_t* ld, const int32_t* widths, int32_t n_blocks, const float* scattered,
                                         int64_t ld_s, int32_t K_s, const int64_t* positions, int64_t Mnz, const float* weight, const float* bias,
                                         int64_t M, int32_t N, float* out, recon_stream_t stream) {
    using namespace recon;
    int32_t Kt = 0;
    const int rc = rh_check(blocks, ld, widths, n_blocks, scattered, ld_s, K_s, positions, Mnz, weight, M, N, &Kt);
    if (rc != RECON_OK) return rc;
    if (M == 0) return RECON_OK;
    if (!out) return RECON_ERR_INVALID;
    RhFwdArgs a{};
    a.c = rh_cols(blocks, ld, widths, n_blocks, nullptr, scattered, ld_s, K_s, positions, Mnz, true, weight, Kt, BK);
    a.w = weight; a.bias = bias; a.out = out; a.M = M; a.N = N; a.Kt = Kt;
    const dim3 grid(static_cast<unsigned>(ceil_div64(M, BM)), static_cast<unsigned>(ceil_div64(N, BN)));
    const uint32_t all = (1u << a.c.nb) - 1u;
    const bool av = a.c.vec == all, wv = a.c.wvec == all;
    hipStream_t st = as_stream(stream);
    if (av && wv) hipLaunchKernelGGL((k_rh_fwd<true, true>), grid, dim3(NT), 0, st, a);
    else if (av) hipLaunchKernelGGL((k_rh_fwd<true, false>), grid, dim3(NT), 0, st, a);
    else if (wv) hipLaunchKernelGGL((k_rh_fwd<false, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((k_rh_fwd<false, false>), grid, dim3(NT), 0, st, a);
    RECON_CHECK_LAUNCH();
    return RECON_OK;
}

extern "C" int recon_relation_logits_bwd(const float* const* blocks, const int64_t* ld, const int32_t* widths, int32_t n_blocks, const float* scattered,
                                         int64_t ld_s, int32_t K_s, const int64_t* positions, int64_t Mnz, const float* weight, const float* g_out,
                                         int64_t M, int32_t N, float* const* g_blocks, float* g_scattered, float* g_w, float* g_b, void* workspace,
                                         size_t workspace_bytes, recon_stream_t stream) {
    using namespace recon;
    int32_t Kt = 0;
    const int rc = rh_check(blocks, ld, widths, n_blocks, scattered, ld_s, K_s, positions, Mnz, weight, M, N, &Kt);
    if (rc != RECON_OK) return rc;
    hipStream_t st = as_stream(stream);
    const bool params = g_w || g_b;
    if (M == 0) {                                                        // zeros in every wanted gradient that has elements, no kernel
        if (g_w && hipMemsetAsync(g_w, 0, sizeof(float) * N * Kt, st) != hipSuccess) return RECON_ERR_LAUNCH;
        if (g_b && hipMemsetAsync(g_b, 0, sizeof(float) * N, st) != hipSuccess) return RECON_ERR_LAUNCH;
        if (g_scattered && Mnz > 0 && K_s > 0 && hipMemsetAsync(g_scattered, 0, sizeof(float) * Mnz * K_s, st) != hipSuccess) return RECON_ERR_LAUNCH;
        return RECON_OK;
    }
    if (!g_out) return RECON_ERR_INVALID;
    if (params) {
        if (!workspace || !aligned16(workspace)) return RECON_ERR_INVALID;
        if (workspace_bytes < recon_relation_logits_workspace_bytes(M, n_blocks, Kt, N, 1)) return RECON_ERR_WORKSPACE;
    }
    const bool gv4 = (N & 3) == 0 && aligned16(g_out);
    bool take[kRhMaxDense] = {false, false, false, false};
    bool any = g_scattered && K_s > 0 && Mnz > 0;
    for (int i = 0; i < n_blocks; ++i) {
        take[i] = g_blocks && g_blocks[i];
        any = any || take[i];
    }
    if (any) {
        RhDbArgs a{};
        a.c = rh_cols(nullptr, nullptr, widths, n_blocks, take, nullptr, 0, K_s, positions, Mnz, g_scattered != nullptr, weight, Kt, BN);
        int n = 0;
        for (int i = 0; i < n_blocks; ++i)
            if (take[i]) a.d[n++] = g_blocks[i];
        if (a.c.sb >= 0) a.d[a.c.sb] = g_scattered;
        a.g = g_out; a.w = weight; a.M = M; a.N = N; a.Kt = Kt;
        bool dense = false;
        for (int i = 0; i < n_blocks; ++i) dense = dense || take[i];
        const int64_t rows = dense ? (a.c.sb >= 0 && Mnz > M ? Mnz : M) : Mnz;
        const dim3 grid(static_cast<unsigned>(ceil_div64(rows, BM)), static_cast<unsigned>(a.c.end[a.c.nb - 1]));
        if (gv4) hipLaunchKernelGGL(k_rh_dblock<true>, grid, dim3(NT), 0, st, a);
        else hipLaunchKernelGGL(k_rh_dblock<false>, grid, dim3(NT), 0, st, a);
        RECON_CHECK_LAUNCH();
    }
    if (params) {
        const int64_t G = rh_groups(M);
        RhWgArgs a{};
        a.c = rh_cols(blocks, ld, widths, n_blocks, nullptr, scattered, ld_s, K_s, positions, Mnz, true, weight, Kt, BN);
        a.g = g_out; a.slab = static_cast<float*>(workspace);
        a.M = M; a.per = ceil_div64(M, G); a.N = N; a.Kt = Kt;
        const int64_t groups = ceil_div64(M, a.per);                     // every group holds at least one row
        const dim3 grid(static_cast<unsigned>(a.c.end[a.c.nb - 1]), static_cast<unsigned>(ceil_div64(N, BM)), static_cast<unsigned>(groups));
        if (gv4) hipLaunchKernelGGL(k_rh_wgrad<true>, grid, dim3(NT), 0, st, a);
        else hipLaunchKernelGGL(k_rh_wgrad<false>, grid, dim3(NT), 0, st, a);
        RECON_CHECK_LAUNCH();
        RhRedArgs r{};
        r.slab = a.slab; r.g_w = g_w; r.g_b = g_b; r.N = N; r.Kt = Kt; r.G = static_cast<int32_t>(groups);
        r.zlo = r.zhi = 0;
        if (K_s > 0 && a.c.sb < 0) { r.zlo = Kt - K_s; r.zhi = Kt; }
        const int64_t total = static_cast<int64_t>(N) * (Kt + 1);
        hipLaunchKernelGGL(k_rh_reduce, dim3(static_cast<unsigned>(ceil_div64(total, 256))), dim3(256), 0, st, r);
        RECON_CHECK_LAUNCH();
    }
    return RECON_OK;
}
